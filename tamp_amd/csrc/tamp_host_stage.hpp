// tamp_host_stage.hpp -- the arithmetic of staging a host-memory call: the extent of the caller's rows, the dense slabs the results
// are produced in, and the layout of the device tables inside one kept buffer.  No HIP type, for the host alone, so that
// tests/test_host_stage_host.py compiles it into a stand-alone host program.  Who uses it: the host-memory calls of tamp_capi.hip,
// tamp_seek.hpp and tamp_pieces.hpp, behind their HostCall.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace tamp_amd {

// The extent [lo, hi) of a batch's rows on the host and their offsets counted from its start.  A row without bytes (len 0, or one
// that `keep` leaves out) takes no part and points at the start; a batch of such rows alone has lo = hi = 0.
struct HostExtent {
    uint64_t lo = 0, hi = 0;
    std::vector<uint64_t> off;
    template <class Keep>
    HostExtent(const uint64_t* row_off, const uint32_t* len, size_t n, Keep keep) : off(n, 0) {
        uint64_t l = ~0ull, h = 0;
        for (size_t i = 0; i < n; i++)
            if (len[i] && keep(i)) l = std::min(l, row_off[i]), h = std::max(h, row_off[i] + len[i]);
        if (h >= l) lo = l, hi = h;
        for (size_t i = 0; i < n; i++)
            if (len[i] && keep(i)) off[i] = row_off[i] - lo;
    }
    HostExtent(const uint64_t* row_off, const uint32_t* len, size_t n) : HostExtent(row_off, len, n, [](size_t) { return true; }) {}
    uint64_t bytes() const { return hi - lo; }
};

// Output slabs back to back: off[i] = the room of the rows in front, -> the room of all (a slab of no room takes none).
inline uint64_t dense_slabs(const uint32_t* cap, size_t n, uint64_t* off) {
    uint64_t room = 0;
    for (size_t i = 0; i < n; i++) off[i] = room, room += cap[i];
    return room;
}

// A table inside a carved buffer: where it starts, and the pointer once the buffer is there.
template <class T>
struct Carved {
    size_t at;
    T* in(void* base) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + at); }
};
// The tables of one buffer, taken one after another: the order of the takes IS the layout, and bytes() is what it needs -- the two
// cannot disagree.  Every table starts at a multiple of its element's alignment (or of `align`, when the caller asks for more); one
// of no elements takes no room.  bytes(): with the 64 bytes of slack the kernels' wide loads may run into.
struct TableCarver {
    size_t used = 0;
    template <class T>
    Carved<T> take(size_t count, size_t align = alignof(T)) {
        const size_t at = (used + align - 1) / align * align;
        if (count) used = at + count * sizeof(T);
        return {at};
    }
    size_t bytes() const { return used + 64; }
};

}  // namespace tamp_amd
