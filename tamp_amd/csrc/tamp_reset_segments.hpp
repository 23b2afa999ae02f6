// tamp_reset_segments.hpp -- the segment table of a dictionary-reset call (tamp_amd_compress_resets): how a buffer
// is cut into segments, what a segment's slab holds, what the whole stream can take -- and, for a batch of such buffers
// (tamp_batch_compress_resets), which stream and cut a row of its two segment tables stands for, and the same for the rows a reset
// index claims on the way back (tamp_batch_decompress_resets).  Arithmetic only, for the host and the device: no HIP type, so that
// tests/test_reset_segments_host.py, tests/test_batch_resets_host.py and tests/test_batch_reset_index_host.py compile it into
// stand-alone host programs.  The kernels that use it:
// tamp_reset_segments_kernel.hpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TAMP_HD __host__ __device__
#else
#define TAMP_HD
#endif

namespace tamp_amd {

// Bytes a segment of n input bytes can take at most: lead (2) + every byte a literal + the FLUSH token, padded.
TAMP_HD constexpr uint64_t reset_segment_bound(uint64_t n, uint32_t literal, bool flush_token) {
    return 2 + (n * (literal + 1) + (flush_token ? 9 : 0) + 7) / 8;
}
TAMP_HD constexpr uint64_t reset_segment_count(uint64_t total, uint32_t interval) {
    return total ? (total + interval - 1) / interval : 1;  // (an empty input is one empty segment)
}
// Input cut of segment k < reset_segment_count(): where it starts, how long it is.
TAMP_HD constexpr uint64_t reset_segment_start(uint64_t k, uint32_t interval) { return k * (uint64_t)interval; }
TAMP_HD constexpr uint32_t reset_segment_len(uint64_t k, uint32_t interval, uint64_t total) {
    const uint64_t left = total - reset_segment_start(k, interval);
    return left < interval ? (uint32_t)left : interval;
}
// Stride of the slabs: the bound of the call's longest segment.  (The table's capacities are 32 bits wide: the entry point refuses a
// call whose longest segment could need more, so the cap below is never met by a launch.)
TAMP_HD constexpr uint32_t reset_slab_bytes(uint64_t total, uint32_t interval, uint32_t literal) {
    const uint64_t longest = interval < total ? interval : (total ? total : 1);
    const uint64_t b = reset_segment_bound(longest, literal, true);
    return b < 0xFFFFFFFFull ? (uint32_t)b : 0xFFFFFFFFu;
}
// Worst-case length of the whole stream: every segment but the last ends with a FLUSH token.
TAMP_HD constexpr uint64_t reset_stream_bound(uint64_t total, uint32_t interval, uint32_t literal) {
    const uint64_t K = reset_segment_count(total, interval);
    return (K - 1) * reset_segment_bound(interval, literal, true) + reset_segment_bound(total - (K - 1) * (uint64_t)interval, literal, false);
}

// ---- a BATCH of buffers, every one cut the same way (tamp_batch_compress_resets) ----
// Stream i has K_i = reset_segment_count(in_len[i], interval) segments.  All but its last one end with a reset: the CLOSED segments,
// counted through the batch in stream order (closed_first[i] = sum of K_j - 1 over j < i; n + 1 entries, closed_first[n] = their
// number = S - n for S segments in all).  Its last one is the stream's OPEN segment, and the open segments are counted by stream.
// With seg_first[i] = closed_first[i] + i the stream's first segment in the order of the whole batch, segment s of stream i is closed
// segment s - i.
struct BatchResetRow {
    uint64_t stream;   // the owner
    uint64_t k;        // which of the owner's segments
    uint64_t start;    // input cut, relative to the owner's first byte
    uint32_t len;
};
TAMP_HD constexpr uint64_t batch_reset_closed_count(uint32_t in_len, uint32_t interval) {
    return reset_segment_count(in_len, interval) - 1;
}
// Owner of closed segment c < closed_first[n]: the last stream whose first closed segment is not behind c (streams without closed
// segments repeat their successor's entry and are stepped over).
TAMP_HD inline uint64_t batch_reset_owner(const uint64_t* closed_first, uint64_t n, uint64_t c) {
    uint64_t lo = 0, hi = n;  // closed_first[lo] <= c < closed_first[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (closed_first[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}
TAMP_HD inline BatchResetRow batch_reset_closed_row(const uint64_t* closed_first, uint64_t n, uint64_t c, uint32_t interval) {
    const uint64_t i = batch_reset_owner(closed_first, n, c), k = c - closed_first[i];
    return {i, k, reset_segment_start(k, interval), interval};
}
TAMP_HD inline BatchResetRow batch_reset_open_row(const uint64_t* closed_first, uint64_t i, uint32_t in_len, uint32_t interval) {
    const uint64_t k = closed_first[i + 1] - closed_first[i];
    return {i, k, reset_segment_start(k, interval), reset_segment_len(k, interval, in_len)};
}
// Stride of the slabs of a batch whose longest stream has `longest` bytes (0: not known).
TAMP_HD constexpr uint32_t batch_reset_slab_bytes(uint32_t longest, uint32_t interval, uint32_t literal) {
    return reset_slab_bytes(longest ? longest : interval, interval, literal);
}

// ---- reading such a batch back with a RESET INDEX (tamp_batch_decompress_resets) ----
// The index is the compressor's (tamp_batch_compress_resets_index): reset_first[0 .. n] = closed_first, and per closed segment the
// offset, in its stream, of the byte behind its reset.  Here it is a HINT: any contents are taken, and what does not hold up makes
// its stream one WHOLE unit.  A stream with E >= 1 entries claims E + 1 segments, in the two-table order of the compress side: row
// r < C (C = reset_first[n]) is the closed segment that ENDS at entry r, row C + i the open segment of stream i, behind its last
// entry.  A stream that holds up is SPLIT: every one of its segments is a unit, staged behind a copy of the stream's two header
// bytes as a stream of its own.
constexpr uint32_t kResetHeaderBytes = 2;     // a stream with the reset bit has the two-byte header
constexpr uint32_t kResetNoOwner = 0xFFFFFFFFu;

// reset_first must be a running sum from 0 for every row to have ONE owner: true for stream i when its two entries are in order
// (and the table starts at 0).  One stream out of order and the whole call goes without an index.
TAMP_HD inline bool reset_first_in_order(const uint64_t* first, uint64_t i) {
    return first[i] <= first[i + 1] && (i != 0 || first[0] == 0);
}
// Entries of stream i, 0 when its rows of reset_first do not make sense (decreasing, or beyond the table's last entry).
TAMP_HD inline uint64_t reset_index_entries(const uint64_t* first, uint64_t n, uint64_t i) {
    const uint64_t a = first[i], b = first[i + 1];
    return (a <= b && b <= first[n]) ? b - a : 0;
}
// A claimed segment's cut of its stream, [start, end) in bytes from the stream's first, and where it stands: the range and order
// check of the entries it touches.
struct ResetIndexCut {
    uint32_t stream;  // kResetNoOwner: the row belongs to no stream, or its entries are out of range or order
    uint32_t seg;     // which of the stream's segments
    uint32_t start, end;
};
// Row r < C: entry r must lie strictly behind the entry in front of it (the header for the stream's first) and at or before the
// stream's end.
TAMP_HD inline ResetIndexCut reset_index_closed_cut(const uint64_t* first, const uint32_t* off, const uint32_t* in_len, uint64_t n, uint64_t c) {
    const ResetIndexCut none = {kResetNoOwner, 0, 0, 0};
    const uint64_t i = batch_reset_owner(first, n, c);  // (reads inside the table whatever it holds)
    if (!(first[i] <= c && c < first[i + 1] && first[i + 1] <= first[n])) return none;
    const uint64_t j = c - first[i];
    const uint32_t start = j ? off[c - 1] : kResetHeaderBytes, end = off[c];
    if (start < kResetHeaderBytes || start >= end || end > in_len[i]) return none;
    return {(uint32_t)i, (uint32_t)j, start, end};
}
// Row C + i: behind the stream's last entry, to its end (an empty cut is a stream that ends with a reset).
TAMP_HD inline ResetIndexCut reset_index_open_cut(const uint64_t* first, const uint32_t* off, const uint32_t* in_len, uint64_t n, uint64_t i) {
    const ResetIndexCut none = {kResetNoOwner, 0, 0, 0};
    const uint64_t E = reset_index_entries(first, n, i);
    if (!E) return none;
    const uint32_t start = off[first[i + 1] - 1];
    if (start < kResetHeaderBytes || start > in_len[i]) return none;
    return {(uint32_t)i, (uint32_t)E, start, in_len[i]};
}
// Bytes the staged units of a split stream of in_len bytes with E entries take: its bytes behind the header, and a header per unit.
TAMP_HD constexpr uint64_t reset_staged_bytes(uint32_t in_len, uint64_t E) {
    return (uint64_t)(in_len - kResetHeaderBytes) + kResetHeaderBytes * (E + 1);
}
// Where a unit lies in the stage (stage_base: its stream's first staged byte) and in its stream's output (size_scan: the exclusive
// scan of the decoded sizes of all closed rows, C + 1 entries).
TAMP_HD constexpr uint64_t reset_unit_stage_off(uint64_t stage_base, const ResetIndexCut& u) {
    return stage_base + (u.start - kResetHeaderBytes) + (uint64_t)kResetHeaderBytes * u.seg;
}
TAMP_HD inline uint64_t reset_unit_out_off(const uint64_t* first, const uint64_t* size_scan, const ResetIndexCut& u) {
    return size_scan[first[u.stream] + u.seg] - size_scan[first[u.stream]];  // (the open segment: seg = E, the stream's closed total)
}

}  // namespace tamp_amd
