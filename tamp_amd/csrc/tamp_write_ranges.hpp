// tamp_write_ranges.hpp -- writing byte ranges into reset-segmented streams (tamp_batch_write_ranges, DESIGN.md 3.13 "Writing
// ranges"): which segments a write touches, how it is cut at their boundaries, and what a segment comes to in the new stream.
// Arithmetic only, for the host and the device: no HIP type, so that tests/test_write_ranges_host.py compiles it into a stand-alone
// host program.  The kernels that use it: tamp_write_ranges_kernel.hpp.
#pragma once
#include "tamp_reset_segments.hpp"

namespace tamp_amd {

// Why a stream fails, in the order of the status table (include/tamp_amd.h): the RANK of a rule, not its code -- two rules share
// TAMP_AMD_BAD_INDEX, two TAMP_AMD_BAD_ARGUMENT.  A stream's word holds the lowest (write, rank) that failed it; kWriteNoFail: none did.
enum WriteRank : uint32_t {
    kWriteRankBudget = 0,     // the stream's units alone outgrow the scratch budget
    kWriteRankOrder = 1,      // a write in front of, or into, its predecessor
    kWriteRankConf = 2,       // the header: not a reset stream, or not the call's conf
    kWriteRankFirst = 3,      // the stream's rows of reset_first
    kWriteRankEnd = 4,        // a write that begins or ends behind the decoded end
    kWriteRankOob = 5,        // a touched segment with an offset out of the window
    kWriteRankIndex = 6,      // a touched segment whose entries or sizes do not hold
    kWriteRankDecode = 7,     // a touched segment that did not decode to what the walk found
    kWriteRankExcess = 8,     // a source byte wider than the literals
    kWriteRankCompress = 9,   // whatever the compress kernel says of a unit
};
constexpr uint64_t kWriteNoFail = ~0ull;
// (write, rank, code) in one word whose order is the order of the rules: the lowest write first, of its rules the first.
TAMP_HD constexpr uint64_t write_fail_key(uint64_t q, uint32_t rank, int32_t code) {
    return (q << 16) | ((uint64_t)rank << 8) | (uint64_t)(uint8_t)(int8_t)code;
}
TAMP_HD constexpr int32_t write_fail_code(uint64_t key) { return (int32_t)(int8_t)(uint8_t)(key & 0xFFu); }

// Write q may follow write q - 1: a later stream, or the same one at or behind the predecessor's end (a sum 64 bits do not hold
// is behind everything).
TAMP_HD constexpr bool write_in_order(uint32_t prev_stream, uint64_t prev_begin, uint32_t prev_len, uint32_t stream, uint64_t begin) {
    return stream > prev_stream || (stream == prev_stream && prev_begin + prev_len >= prev_begin && begin >= prev_begin + prev_len);
}

// A write of len > 0 bytes at `begin` into a stream of E entries (segments 0 .. E, the last one open) touches segments k0 .. k1;
// ok = false: it begins or ends behind the open segment's first N bytes (whether it ends behind the open segment's true size is
// seen when that segment is decoded).  All of it in 64 bits, with ONE 64-bit division (read_range_plan's way).
struct WriteSpan {
    bool ok;
    uint64_t k0, k1;
    uint32_t lo;  // where it starts in segment k0
    uint32_t hi;  // behind its last byte in segment k1
};
TAMP_HD inline WriteSpan write_span(uint64_t E, uint32_t N, uint64_t begin, uint32_t len) {
    WriteSpan s = {false, begin / N, 0, 0, 0};
    if (s.k0 > E || len == 0) return s;
    const uint64_t rem = begin - s.k0 * N;
    const uint32_t more = (len - 1) / N, r2 = (len - 1) % N;
    const bool carry = rem + r2 >= N;
    const uint64_t beyond = (uint64_t)more + (carry ? 1 : 0);
    if (beyond > E - s.k0) return s;
    s.ok = true, s.k1 = s.k0 + beyond, s.lo = (uint32_t)rem, s.hi = (uint32_t)(rem + r2 - (carry ? N : 0) + 1);
    return s;
}
// The piece of the write that lies in segment k0 + j: bytes [lo, hi) of the segment, from `skip` bytes into the write's source.
struct WritePiece {
    uint32_t lo, hi;
    uint64_t skip;
};
TAMP_HD inline WritePiece write_piece(const WriteSpan& s, uint32_t N, uint64_t j) {
    WritePiece p;
    p.lo = j ? 0 : s.lo;
    p.hi = s.k0 + j == s.k1 ? s.hi : N;
    p.skip = j ? j * N - s.lo : 0;
    return p;
}

// What a segment takes in the new stream.  A unit's slab holds the 2-byte lead, the segment's tokens and, for a closed one, the FLUSH
// token padded to a byte; in its stream a closed segment is the tokens, that FLUSH and the NEXT segment's lead (the reset's second
// FLUSH: the same two bytes), the open one the tokens alone.
TAMP_HD constexpr uint32_t write_unit_span(uint32_t slab_len, bool closed) {
    return slab_len < kResetHeaderBytes ? 0 : (closed ? slab_len : slab_len - kResetHeaderBytes);
}
// The splice of one stream on the host (the kernel scans the same values): new_len[k] for k = 0 .. E -> where each segment starts
// (start[0] = the header's two bytes), the entries of the new index, and the new length.
TAMP_HD inline uint64_t write_splice(const uint32_t* new_len, uint64_t E, uint64_t* start /* E + 1 */, uint64_t* entry /* E */) {
    uint64_t at = kResetHeaderBytes;
    for (uint64_t k = 0; k <= E; k++) {
        start[k] = at, at += new_len[k];
        if (k < E) entry[k] = at;
    }
    return at;
}

// Bytes a unit takes in the call's scratch: its staging row (N rounded up to 16), its slab, its rows of the tables.
constexpr uint64_t kWriteUnitRow = 64;
TAMP_HD constexpr uint32_t write_row_bytes(uint32_t N) { return (uint32_t)(((uint64_t)N + 15) & ~15ull); }
TAMP_HD constexpr uint64_t write_unit_cost(uint32_t N, uint32_t slab) { return (uint64_t)write_row_bytes(N) + slab + kWriteUnitRow; }

}  // namespace tamp_amd
