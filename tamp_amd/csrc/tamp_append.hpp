// tamp_append.hpp -- appending to reset-segmented streams so that the closed segments keep holding exactly N bytes
// (tamp_batch_append, DESIGN.md 3.13 "Appending"): how the open segment's m bytes and the L appended ones are cut into units, which
// rows of the call's tables a stream's units take, and what the new units come to in the new stream and its index.
// Arithmetic only, for the host and the device: no HIP type, so that tests/test_append_host.py compiles it into a stand-alone host
// program.  The kernels that use it: tamp_append_kernel.hpp.
#pragma once
#include "tamp_write_ranges.hpp"

namespace tamp_amd {

// Why a stream fails, in the order of the status table (include/tamp_amd.h): the rank of a rule, not its code.  A stream's word is
// write_fail_key(unit, rank, code) of the first rule that failed it (tamp_write_ranges.hpp), kWriteNoFail: none did.
enum AppendRank : uint32_t {
    kAppendRankBudget = 0,    // the stream's units alone outgrow the scratch budget
    kAppendRankConf = 1,      // the header is not what conf makes
    kAppendRankFirst = 2,     // the stream's rows of reset_first
    kAppendRankEntries = 3,   // entries out of range or order
    kAppendRankOob = 4,       // an offset of the open segment out of the window
    kAppendRankIndex = 5,     // the open segment does not parse from the last entry, or decodes to more than N bytes
    kAppendRankDecode = 6,    // the open segment did not decode to what the walk found
    kAppendRankExcess = 7,    // a source byte wider than the literals
    kAppendRankCompress = 8,  // whatever the compress kernel says of a unit
};

// Which streams' rows of reset_first HOLD.  In order and inside the table (read_index_usable) is a test of one row pair; two pairs
// that pass it may still claim the same entries (first = {0, 5, 3, 8}: streams 0 and 2).  So a stream's rows hold only when they
// also start at or behind the end of EVERY usable pair in front of it: the entries of streams that hold are disjoint, ascending and
// inside the table, their sum is reset_first[n] at most, and the bound of new_reset_off below suffices whatever the table holds.
// A stream whose rows do not hold fails alone (TAMP_AMD_BAD_INDEX) or, when nothing is appended to it, is copied without entries.
TAMP_HD inline void append_rows_hold(const uint64_t* first, uint64_t n, uint8_t* hold) {
    uint64_t end = 0;
    for (uint64_t i = 0; i < n; i++) {
        const bool usable = read_index_usable(first, n, i);
        hold[i] = usable && first[i] >= end ? 1 : 0;
        if (usable && first[i + 1] > end) end = first[i + 1];
    }
}

// Units of a stream whose open segment holds m <= N bytes and that receives L more: the m + L bytes cut at every N.  All but the
// last are closed.  (m + L < 2^33: 64 bits hold everything below.)
TAMP_HD constexpr uint64_t append_units(uint32_t m, uint32_t L, uint32_t N) {
    const uint64_t total = (uint64_t)m + L;
    return total ? (total + N - 1) / N : 1;
}
// What the caller can know without m: the new entries of a stream are append_units - 1 <= ceil(L / N) (m <= N) ...
TAMP_HD constexpr uint64_t append_entry_bound(uint32_t L, uint32_t N) { return ((uint64_t)L + N - 1) / N; }
// ... so an appending stream (L > 0) is given append_entry_bound CLOSED rows and one OPEN row, whatever m turns out to be: the call
// sizes its tables before the open segments are decoded.  Unit j < U of the stream stands in closed row j, the last one in the open
// row; U is the bound or one more, so at most the last closed row stays without a unit.
TAMP_HD constexpr bool append_closed_row_used(uint64_t j, uint64_t U) { return j + 1 < U; }
// Unit j's cut: its bytes of the row (old bytes first), and where its source bytes start in the stream's appended bytes.
struct AppendCut {
    uint32_t len;      // bytes of the unit, old and new
    uint32_t old_len;  // of them from the old open segment, in front: m for unit 0, else 0
    uint64_t src_at;   // the first source byte it takes
};
TAMP_HD inline AppendCut append_cut(uint32_t m, uint32_t L, uint32_t N, uint64_t j) {
    const uint64_t total = (uint64_t)m + L, begin = j * N;
    AppendCut c = {0, 0, 0};
    if (begin >= total && !(j == 0 && total == 0)) return c;
    const uint64_t left = total - begin;
    c.len = left < N ? (uint32_t)left : N;
    c.old_len = j == 0 ? (m < c.len ? m : c.len) : 0;
    c.src_at = j == 0 ? 0 : begin - m;
    return c;
}

// The splice of one stream on the host (the kernel scans the same values): the new units follow the old bytes in front of the open
// segment, which starts at `start`.  slab_len[j]: what unit j was compressed to, lead included.  -> the new length (which may not
// fit 32 bits: the caller's TAMP_OUTPUT_FULL); entry[j] for j < U - 1: the new index entries.
TAMP_HD inline uint64_t append_splice(uint32_t start, const uint32_t* slab_len, uint64_t U, uint64_t* entry /* U - 1 */) {
    uint64_t at = start;
    for (uint64_t j = 0; j < U; j++) {
        at += write_unit_span(slab_len[j], j + 1 < U);
        if (j + 1 < U) entry[j] = at;
    }
    return at;
}
TAMP_HD constexpr bool append_fits(uint64_t new_len, uint32_t out_cap) { return new_len <= out_cap && new_len <= 0xFFFFFFFFull; }

// Entries that new_reset_off must hold whatever the open segments decode to: the old ones and the bound of every stream.
TAMP_HD inline uint64_t append_reset_bound(uint64_t old_entries, const uint32_t* src_len, uint64_t n, uint32_t N) {
    uint64_t need = old_entries;
    for (uint64_t i = 0; i < n; i++) need += append_entry_bound(src_len[i], N);
    return need;
}

}  // namespace tamp_amd
