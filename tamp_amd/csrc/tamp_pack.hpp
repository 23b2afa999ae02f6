// tamp_pack.hpp -- the index arithmetic of tamp_batch_pack: a batch's streams, wherever their slabs lie, copied back
// to back into one buffer.  Stream i lands at dst_off[i], the exclusive scan of the lengths rounded up to `align`; the bytes between
// its end and dst_off[i + 1] are zero.  The copy's UNIT OF WORK is a TILE of kPackTile destination bytes cut at absolute addresses
// that are multiples of kPackTile, and inside it the 16-byte LINE, again at absolute multiples of 16: two units never store into the
// same line, and every line that lies inside the packed bytes is one aligned 16-byte store, whatever it holds -- the body of one
// stream (one 16-byte load at whatever alignment the source has), or the ends of several and their padding (assembled in registers
// from loads of 8, 4, 2 and 1 bytes).  Only the first and the last line of the whole buffer can be cut by its ends.
// Positions are counted in two ways: `rel`, from the destination's first byte (what dst_off holds), and `grid`, from the tile
// boundary at or in front of it (grid = rel + skew, skew = address of dst mod kPackTile), which never goes negative.
// Arithmetic and plain loads only, for the host and the device: no HIP type, so that tests/test_pack_host.py compiles it into a
// stand-alone host program.  The kernels that use it: tamp_pack_kernel.hpp.
#pragma once
#include <stdint.h>

#ifndef TAMP_HD
#if defined(__HIPCC__)
#define TAMP_HD __host__ __device__
#else
#define TAMP_HD
#endif
#endif

namespace tamp_amd {

constexpr uint32_t kPackTile = 16384;  // destination bytes per unit of work
constexpr uint32_t kPackLine = 16;     // bytes per store
constexpr uint32_t kPackMaxAlign = 4096;

TAMP_HD constexpr bool pack_align_ok(uint32_t align) { return align >= 1 && align <= kPackMaxAlign && (align & (align - 1)) == 0; }
// Bytes stream i takes in the packed buffer.
TAMP_HD constexpr uint64_t pack_padded(uint32_t len, uint32_t align) { return ((uint64_t)len + (align - 1)) & ~(uint64_t)(align - 1); }

// Tiles that hold a byte of [skew, skew + total) in grid positions.
TAMP_HD constexpr uint64_t pack_tile_count(uint32_t skew, uint64_t total) {
    return total ? total / kPackTile + (total % kPackTile + skew + kPackTile - 1) / kPackTile : 0;
}
struct PackSpan {
    uint64_t lo, hi;  // [lo, hi) in rel positions; empty when hi <= lo
};
// What grid positions [g, g + bytes) hold of the packed bytes.
TAMP_HD constexpr PackSpan pack_span(uint32_t skew, uint64_t total, uint64_t g, uint32_t bytes) {
    const uint64_t lo = g > skew ? g - skew : 0;
    const uint64_t hi = g + bytes > skew ? (g + bytes - skew < total ? g + bytes - skew : total) : 0;
    return {lo, hi > lo ? hi : lo};
}
TAMP_HD constexpr PackSpan pack_tile_span(uint32_t skew, uint64_t total, uint64_t t) { return pack_span(skew, total, t * kPackTile, kPackTile); }
TAMP_HD constexpr PackSpan pack_line_span(uint32_t skew, uint64_t total, uint64_t t, uint32_t line) {
    return pack_span(skew, total, t * kPackTile + (uint64_t)line * kPackLine, kPackLine);
}

// Owner of packed byte x: the last stream i in [lo, hi) with dst_off[i] <= x, given dst_off[lo] <= x < dst_off[hi] (empty streams
// repeat their successor's entry and are stepped over, as in batch_reset_owner).
TAMP_HD inline uint64_t pack_owner(const uint64_t* dst_off, uint64_t lo, uint64_t hi, uint64_t x) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (dst_off[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
// The same for an owner that is expected close behind `from`: doubling steps, then the search between the last two probes.
TAMP_HD inline uint64_t pack_owner_from(const uint64_t* dst_off, uint64_t from, uint64_t n, uint64_t x) {
    uint64_t lo = from, hi = from + 1, step = 1;
    while (hi < n && dst_off[hi] <= x) {
        lo = hi, step *= 2;
        hi = n - hi < step ? n : hi + step;
    }
    return pack_owner(dst_off, lo, hi, x);
}

// The data pieces of packed bytes [lo, hi), in order: piece(stream, at, pos, m) for m bytes from byte `at` of `stream` that land at
// rel position pos.  What no piece covers is padding.  i: the owner of lo; dst_off[i_end] > hi - 1 bounds the searches.
template <class Piece>
TAMP_HD inline void pack_walk(const uint64_t* dst_off, const uint32_t* src_len, uint64_t i, uint64_t i_end, uint64_t lo, uint64_t hi,
                              Piece&& piece) {
    uint64_t pos = lo;
    while (pos < hi) {
        const uint64_t o = dst_off[i], data_end = o + src_len[i];
        if (pos < data_end) piece(i, pos - o, pos, (uint32_t)((data_end < hi ? data_end : hi) - pos));
        pos = dst_off[i + 1];
        if (pos >= hi) break;
        i++;
        if (dst_off[i + 1] <= pos) i = pack_owner(dst_off, i, i_end, pos);  // (a run of empty streams: searched, not walked)
    }
}

// Loads at any address (gfx950 serves misaligned global loads in hardware; the compiler emits one instruction for an align-1 type).
struct __attribute__((packed, aligned(1))) PackU128 { uint32_t v[4]; };
struct __attribute__((packed, aligned(1))) PackU64 { uint64_t v; };
struct __attribute__((packed, aligned(1))) PackU32 { uint32_t v; };
struct __attribute__((packed, aligned(1))) PackU16 { uint16_t v; };

struct PackLine {
    uint64_t x0, x1;  // bytes 0-7 and 8-15 of a line, little endian
};
TAMP_HD inline PackLine pack_load16(const uint8_t* p) {
    const PackU128 v = *reinterpret_cast<const PackU128*>(p);
    return {v.v[0] | (uint64_t)v.v[1] << 32, v.v[2] | (uint64_t)v.v[3] << 32};
}
// m <= 15 bytes at p as the low bytes of a line: one load per set bit of m, the widest first, so that every one of them stands at a
// multiple of its own width and none straddles the two halves.  Nothing outside [p, p + m) is read.
TAMP_HD inline PackLine pack_gather(const uint8_t* p, uint32_t m) {
    PackLine g = {0, 0};
    uint32_t got = 0;
    auto put = [&](uint64_t v) {
        const uint64_t s = v << (8 * (got & 7));
        if (got & 8) g.x1 |= s;
        else g.x0 |= s;
    };
    if (m & 8) put(reinterpret_cast<const PackU64*>(p)->v), got = 8;
    if (m & 4) put(reinterpret_cast<const PackU32*>(p + got)->v), got += 4;
    if (m & 2) put(reinterpret_cast<const PackU16*>(p + got)->v), got += 2;
    if (m & 1) put(p[got]);
    return g;
}
// g moved up by k <= 15 bytes (what leaves the line is dropped).
TAMP_HD inline PackLine pack_shift(PackLine g, uint32_t k) {
    if (k >= 8) return {0, g.x0 << (8 * (k - 8))};
    if (k == 0) return g;
    return {g.x0 << (8 * k), g.x1 << (8 * k) | g.x0 >> (64 - 8 * k)};
}

// True when packed bytes [lo, lo + 16) all belong to the body of stream i, the owner of lo: the line is one load and one store.
TAMP_HD inline bool pack_line_is_body(const uint64_t* dst_off, const uint32_t* src_len, uint64_t i, PackSpan s) {
    return s.hi - s.lo == kPackLine && s.hi <= dst_off[i] + src_len[i];
}
// The value of the line that holds packed bytes [s.lo, s.hi) (at most 16 of them, s.lo standing at byte k0 of the line): data where
// a stream has some, zero elsewhere.  i, i_end: as for pack_walk.
TAMP_HD inline PackLine pack_line_value(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len, const uint64_t* dst_off,
                                        uint64_t i, uint64_t i_end, PackSpan s, uint32_t k0) {
    PackLine x = {0, 0};
    pack_walk(dst_off, src_len, i, i_end, s.lo, s.hi, [&](uint64_t stream, uint64_t at, uint64_t pos, uint32_t m) {
        const uint8_t* const p = src + src_off[stream] + at;
        const PackLine g = pack_shift(m >= kPackLine ? pack_load16(p) : pack_gather(p, m), k0 + (uint32_t)(pos - s.lo));
        x.x0 |= g.x0, x.x1 |= g.x1;
    });
    return x;
}

}  // namespace tamp_amd
