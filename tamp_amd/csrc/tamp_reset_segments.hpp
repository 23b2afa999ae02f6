// tamp_reset_segments.hpp -- the segment table of a dictionary-reset call (tamp_amd_compress_resets): how a buffer
// is cut into segments, what a segment's slab holds, what the whole stream can take -- and, for a batch of such buffers
// (tamp_batch_compress_resets), which stream and cut a row of its two segment tables stands for, and the same for the rows a reset
// index claims on the way back (tamp_batch_decompress_resets), and what a byte range of such a stream touches
// (tamp_batch_read_ranges; with segments of any size: tamp_batch_segment_ends, tamp_batch_read_ranges_grid).  Arithmetic only, for the
// host and the device: no HIP type, so that tests/test_reset_segments_host.py, tests/test_batch_resets_host.py,
// tests/test_batch_reset_index_host.py, tests/test_read_ranges_host.py and tests/test_read_ranges_grid_host.py compile it into
// stand-alone host programs.  The kernels that use it: tamp_reset_segments_kernel.hpp, tamp_read_ranges_kernel.hpp,
// tamp_segment_ends_kernel.hpp.
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

// ---- reading byte RANGES of such a batch (tamp_batch_read_ranges) ----
// Every closed segment decodes to exactly N = reset_interval bytes, so decoded byte b of a stream lies in segment b / N and the index
// says where that segment's tokens start.  Range q asks for `len` decoded bytes from `begin` of stream i (E entries, segments 0 .. E,
// the last one open): it touches segments k0 = begin / N through k1 = min((begin + len - 1) / N, E), each one a UNIT that is staged
// behind a copy of the stream's header as a stream of its own and decoded into the range's scratch at j * N for unit j -- the
// range's bytes are then `skip` = begin - k0 * N bytes into that scratch, in one piece.  Here the index is TRUSTED for position
// (a segment's start is no longer token aligned by induction from the header); what is checked is what memory safety and the
// address k * N need.  All of it in 64 bits.
constexpr int32_t kReadGo = 127;  // a range's verdict: no result yet, its units are decoded (every other value is its status)
constexpr int32_t kReadOk = 0, kReadInputExhausted = 2, kReadInvalidConf = -3, kReadBadArgument = -21, kReadBadIndex = -22;
constexpr uint32_t kReadMaxSegment = (1u << 29) - 1 - 512;  // the walk counts a segment's bits in 32 bits (kMaxDecodeIn - 512)
constexpr uint64_t kReadUnitRow = 64;  // bytes of table rows a unit takes in the call's scratch (at least; the budget counts them)

// The header conditions of a stream that may be read by ranges: the reset bit (with it the second header byte, which must be
// zero), no custom dictionary, a window the call accepts.
TAMP_HD inline bool read_header_eligible(const uint8_t* s, uint32_t len, uint32_t max_wbits) {
    if (len < kResetHeaderBytes || max_wbits > 15) return false;
    const uint32_t h0 = s[0];
    return (h0 & 1u) && !((h0 >> 2) & 1u) && s[1] == 0 && ((h0 >> 5) & 7u) + 8 <= max_wbits;
}
// Stream i's rows of reset_first make sense: in order, inside the table, and the table starts at 0.
TAMP_HD inline bool read_index_usable(const uint64_t* first, uint64_t n, uint64_t i) {
    return reset_first_in_order(first, i) && first[i + 1] <= first[n];
}
// Segment k <= E of stream i (E = first[i + 1] - first[i], which may be 0: the whole stream is one open segment): its cut, with the
// range and order check of the entries it uses.  ok = false: an entry out of range or order, or a segment too long to walk.
struct ReadCut {
    uint32_t start, end;
    bool closed, ok;
};
TAMP_HD inline ReadCut read_segment_cut(const uint64_t* first, const uint32_t* off, const uint32_t* in_len, uint64_t i, uint64_t k) {
    const uint64_t f = first[i], E = first[i + 1] - f;
    const bool closed = k < E;
    const uint32_t start = k ? off[f + k - 1] : kResetHeaderBytes, end = closed ? off[f + k] : in_len[i];
    // a closed segment holds its FLUSH, FLUSH at least: it is never empty; the open one may be (a stream that ends with a reset)
    const bool ok = start >= kResetHeaderBytes && end <= in_len[i] && (closed ? start < end : start <= end) && end - start <= kReadMaxSegment;
    return {start, end, closed, ok};
}
TAMP_HD constexpr uint64_t read_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// What a range comes to before anything is decoded.  verdict != kReadGo: the range's status, it has no units.
struct ReadPlan {
    int32_t verdict;
    uint64_t k0;       // its first segment
    uint64_t units;    // segments it touches
    uint64_t scratch;  // decoded bytes its units are given room for: N for every unit but the last, `last_need` for that
    uint64_t staged;   // bytes its units take in the stage: the segments and a header each
    uint32_t last_need;
    uint32_t span_start;  // where its first unit starts in the stream
};
TAMP_HD inline ReadPlan read_range_plan(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint64_t* first,
                                        const uint32_t* off, uint64_t n, uint32_t N, uint32_t max_wbits, uint64_t budget,
                                        uint32_t stream, uint64_t begin, uint32_t len) {
    ReadPlan p = {kReadBadArgument, 0, 0, 0, 0, 0, 0};
    if (stream >= n) return p;
    p.verdict = kReadOk;
    if (len == 0) return p;  // (the stream is not looked at)
    const uint64_t i = stream;
    p.verdict = kReadInvalidConf;
    if (!read_header_eligible(in + in_off[i], in_len[i], max_wbits)) return p;
    p.verdict = kReadBadIndex;
    if (!read_index_usable(first, n, i) || (!off && first[i + 1] != first[i])) return p;  // (entries and no table to hold them)
    const uint64_t E = first[i + 1] - first[i], k0 = begin / N;
    p.k0 = k0;
    p.verdict = kReadInputExhausted;
    if (k0 > E) return p;
    // k1 = min((begin + len - 1) / N, E) without the sum, which 64 bits may not hold, and with ONE 64-bit division: from the first
    // byte of segment k0 the range ends rem + len bytes on, and len - 1 = more * N + r2
    const uint64_t rem = begin - k0 * N;
    const uint32_t more = (len - 1) / N, r2 = (len - 1) % N;
    const bool carry = rem + r2 >= N;
    const uint64_t beyond = (uint64_t)more + (carry ? 1 : 0);  // segments behind k0 that the range reaches into, were there enough
    const bool clipped = beyond > E - k0;                       // ... it runs past the open segment
    const uint64_t units = (clipped ? E - k0 : beyond) + 1, k1 = k0 + units - 1;
    // the span of the touched segments: from the entry in front of the first to the entry behind the last (the units kernel
    // checks every entry between them)
    const ReadCut a = read_segment_cut(first, off, in_len, i, k0), b = read_segment_cut(first, off, in_len, i, k1);
    p.verdict = kReadBadIndex;
    if (!a.ok || !b.ok || b.end < a.start) return p;
    // what is asked of the last unit: up to the range's last byte, or all of it when the range runs on
    const uint32_t last_need = clipped ? N : (uint32_t)(rem + r2 - (carry ? N : 0) + 1);
    const uint64_t scratch = (units - 1) * N + last_need, staged = (uint64_t)(b.end - a.start) + kResetHeaderBytes * units;
    p.verdict = kReadBadArgument;  // the range alone outgrows what the call may take
    if (units > budget / kReadUnitRow || read_sat_add(read_sat_add(scratch, staged), units * kReadUnitRow) > budget) return p;
    p.verdict = kReadGo, p.units = units, p.scratch = scratch, p.staged = staged, p.last_need = last_need, p.span_start = a.start;
    return p;
}
TAMP_HD constexpr uint64_t read_plan_cost(const ReadPlan& p) { return p.scratch + p.staged + p.units * kReadUnitRow; }

// Unit j < units of a range: segment k0 + j.  Its cut must hold up and lie inside the range's span (then its place in the stage
// does, too); place: from the range's first staged byte; room: from the range's first scratch byte.
struct ReadUnit {
    ReadCut cut;
    uint32_t need;     // decoded bytes asked of it
    uint32_t in_len;   // segment + header bytes, 0: no unit (cut.ok false)
    uint64_t place, room;
};
TAMP_HD inline ReadUnit read_range_unit(const uint64_t* first, const uint32_t* off, const uint32_t* in_len, uint32_t N, uint64_t i,
                                        const ReadPlan& p, uint64_t j) {
    ReadUnit u;
    u.cut = read_segment_cut(first, off, in_len, i, p.k0 + j);
    u.need = j + 1 == p.units ? p.last_need : N;
    const uint64_t span = p.staged - kResetHeaderBytes * p.units;  // span_start .. span_start + span
    if (u.cut.ok && (u.cut.start < p.span_start || (uint64_t)u.cut.end - p.span_start > span)) u.cut.ok = false;
    u.in_len = u.cut.ok ? u.cut.end - u.cut.start + kResetHeaderBytes : 0;
    u.place = u.cut.ok ? (uint64_t)(u.cut.start - p.span_start) + kResetHeaderBytes * j : 0;
    u.room = j * N;
    return u;
}
// Bytes a range delivers when its units decoded to `total` bytes in all: what lies behind `skip` = begin - k0 * N, `len` at most.
TAMP_HD constexpr uint64_t read_range_skip(uint64_t begin, uint64_t k0, uint32_t N) { return begin - k0 * N; }
TAMP_HD constexpr uint32_t read_range_delivered(uint64_t total, uint64_t skip, uint32_t len) {
    return total > skip ? (total - skip < len ? (uint32_t)(total - skip) : len) : 0;
}

// ---- the same for segments of ANY size: the table of segment ends (tamp_batch_segment_ends, tamp_batch_read_ranges_grid) ----
// One uint64 entry per SEGMENT of the batch: stream i with E entries in the index has E + 1, at segment_end[first[i] + i + k] for
// k = 0 .. E, entry k the decoded size of its segments 0 .. k (non-decreasing; the last one the stream's decoded size).  Segment k
// covers decoded bytes [B(k), B(k + 1)) with B(0) = 0 and B(k) = entry k - 1; segments of no bytes are legal.  The segment of a byte
// is found by a search where the fixed form divides; everything behind that is the fixed form's.  The table is TRUSTED for position
// and checked on what a range touches; the search reads inside the stream's rows whatever they hold (its bounds come from first).
constexpr uint64_t kSegmentEndSaturated = ~0ull;  // an entry behind a segment of "2^32 - 1 or more" bytes
constexpr uint32_t kSegmentSizeSaturated = 0xFFFFFFFFu;

// Where stream i's rows of the table start (the stream's rows of `first` hold up: read_index_usable).
TAMP_HD inline uint64_t segment_end_row(const uint64_t* first, uint64_t i) { return first[i] + i; }
// Owner of table row p < first[n] + n: the last stream whose first row is not behind p (batch_reset_owner with the key first[i] + i,
// which grows with every stream: no stream is stepped over).
TAMP_HD inline uint64_t segment_end_owner(const uint64_t* first, uint64_t n, uint64_t p) {
    uint64_t lo = 0, hi = n;  // row(lo) <= p < row(hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (segment_end_row(first, mid) <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}
// The running sum the table is made of (tamp_batch_segment_ends), as the operator of a SEGMENTED scan: `head` says that a stream's
// first row lies in the span the value stands for, and then the value counts from that row.  A saturated size makes its entry and
// every later one of its stream kSegmentEndSaturated (true sums stay far below: fewer than 2^32 entries of less than 2^32 each).
struct SegmentEndSum {
    uint64_t v;
    uint32_t head;
};
TAMP_HD constexpr SegmentEndSum segment_end_identity() { return {0, 0}; }
TAMP_HD constexpr uint64_t segment_end_add(uint64_t a, uint64_t b) {
    return a == kSegmentEndSaturated || b == kSegmentEndSaturated ? kSegmentEndSaturated : a + b;
}
TAMP_HD constexpr SegmentEndSum segment_end_combine(const SegmentEndSum& a, const SegmentEndSum& b) {  // (a in front of b)
    return b.head ? b : SegmentEndSum{segment_end_add(a.v, b.v), a.head};
}
// What row p of the table adds: the size of its segment, and whether it is its stream's first.  Reads inside the three tables
// whatever `first` holds (rows that make no sense add nothing).
TAMP_HD inline SegmentEndSum segment_end_term(const uint64_t* first, const uint32_t* closed_size, const uint32_t* open_size, uint64_t n,
                                              uint64_t p) {
    const uint64_t i = segment_end_owner(first, n, p), row = segment_end_row(first, i);
    if (p < row) return segment_end_identity();  // (first[0] != 0)
    const uint64_t k = p - row, E = reset_index_entries(first, n, i);
    uint32_t size = 0;
    if (k < E) size = closed_size[first[i] + k];
    else if (k == E) size = open_size[i];
    return {size == kSegmentSizeSaturated ? kSegmentEndSaturated : size, k == 0 ? 1u : 0u};
}
// The whole table, row by row: what a host-memory call does, and what the kernels' scan comes to.
inline void segment_ends_fill(const uint64_t* first, const uint32_t* closed_size, const uint32_t* open_size, uint64_t* segment_end,
                              uint64_t n) {
    const uint64_t rows = n ? first[n] + n : 0;
    SegmentEndSum sum = segment_end_identity();
    for (uint64_t p = 0; p < rows; p++) {
        sum = segment_end_combine(sum, segment_end_term(first, closed_size, open_size, n, p));
        segment_end[p] = sum.v;
    }
}

// A range of the table form before anything is decoded: ReadPlan with the table's own figures.  `base` = B(k0), `skip` = begin -
// base: where the range's bytes start in its scratch.  The last unit is asked for end - B(k1) bytes, every other one for its whole
// size, and the scratch is end - B(k0): true sizes, the open segment's too.
struct ReadGridPlan {
    ReadPlan p;
    uint64_t base, skip;
};
// Entries k < E of a stream's rows T that are <= b (an upper bound; any contents: the result is in 0 .. E).
TAMP_HD inline uint64_t segment_end_search(const uint64_t* T, uint64_t E, uint64_t b) {
    uint64_t lo = 0, hi = E;  // rows in front of lo are <= b, rows from hi on are not (of a sorted table)
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (T[mid] <= b) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
TAMP_HD inline ReadGridPlan read_grid_plan(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint64_t* first,
                                           const uint32_t* off, const uint64_t* segment_end, uint64_t n, uint32_t max_wbits,
                                           uint64_t budget, uint32_t stream, uint64_t begin, uint32_t len) {
    ReadGridPlan g = {{kReadBadArgument, 0, 0, 0, 0, 0, 0}, 0, 0};
    ReadPlan& p = g.p;
    if (stream >= n) return g;
    p.verdict = kReadOk;
    if (len == 0) return g;  // (the stream is not looked at)
    const uint64_t i = stream;
    p.verdict = kReadInvalidConf;
    if (!read_header_eligible(in + in_off[i], in_len[i], max_wbits)) return g;
    p.verdict = kReadBadIndex;
    if (!read_index_usable(first, n, i) || (!off && first[i + 1] != first[i])) return g;  // (entries and no table to hold them)
    const uint64_t E = first[i + 1] - first[i];
    const uint64_t* const T = segment_end + segment_end_row(first, i);
    const uint64_t total = T[E];
    p.verdict = kReadInputExhausted;
    if (begin >= total) return g;  // (at or behind the stream's end: answered from the table alone)
    const uint64_t sum = read_sat_add(begin, len), end = sum < total ? sum : total;
    const uint64_t k0 = segment_end_search(T, E, begin), k1 = segment_end_search(T, E, end - 1);
    p.k0 = k0;
    // what the search promises of a sorted table, looked at: both ends lie in the segment found for them.  (The units kernel
    // checks every entry between them against the one in front of it, which makes B(k0) <= ... <= T[k1] a chain.)
    const uint64_t b0 = k0 ? T[k0 - 1] : 0, b1 = k1 ? T[k1 - 1] : 0;
    p.verdict = kReadBadIndex;
    if (!(b0 <= begin && begin < T[k0]) || k1 < k0 || !(b1 <= end - 1 && end - 1 < T[k1])) return g;
    if (T[k0] - b0 >= kSegmentSizeSaturated || T[k1] - b1 >= kSegmentSizeSaturated) return g;  // (a segment of 2^32 - 1 bytes or more)
    const uint64_t units = k1 - k0 + 1;
    const ReadCut a = read_segment_cut(first, off, in_len, i, k0), b = read_segment_cut(first, off, in_len, i, k1);
    if (!a.ok || !b.ok || b.end < a.start) return g;
    const uint32_t last_need = (uint32_t)(end - b1);
    const uint64_t scratch = end - b0, staged = (uint64_t)(b.end - a.start) + kResetHeaderBytes * units;
    p.verdict = kReadBadArgument;  // the range alone outgrows what the call may take
    if (units > budget / kReadUnitRow || read_sat_add(read_sat_add(scratch, staged), units * kReadUnitRow) > budget) return g;
    p.verdict = kReadGo, p.units = units, p.scratch = scratch, p.staged = staged, p.last_need = last_need, p.span_start = a.start;
    g.base = b0, g.skip = begin - b0;
    return g;
}
// Unit j < units of such a range: segment k0 + j, read_range_unit with the table's sizes.  `size`: what the table says the segment
// decodes to, which the walk holds it to; a touched entry below the one in front of it, or a size of 2^32 - 1 or more, is no unit.
struct ReadGridUnit {
    ReadUnit u;
    uint32_t size;
};
TAMP_HD inline ReadGridUnit read_grid_unit(const uint64_t* first, const uint32_t* off, const uint32_t* in_len, const uint64_t* segment_end,
                                           uint64_t i, const ReadGridPlan& g, uint64_t j) {
    const ReadPlan& p = g.p;
    const uint64_t* const T = segment_end + segment_end_row(first, i);
    const uint64_t k = p.k0 + j, b = k ? T[k - 1] : 0, e = T[k];
    ReadGridUnit w;
    ReadUnit& u = w.u;
    u.cut = read_segment_cut(first, off, in_len, i, k);
    const uint64_t span = p.staged - kResetHeaderBytes * p.units;  // span_start .. span_start + span
    if (u.cut.ok && (u.cut.start < p.span_start || (uint64_t)u.cut.end - p.span_start > span)) u.cut.ok = false;
    if (e < b || e - b >= kSegmentSizeSaturated || b < g.base) u.cut.ok = false;
    w.size = u.cut.ok ? (uint32_t)(e - b) : 0;
    u.need = !u.cut.ok ? 0 : (j + 1 == p.units ? p.last_need : w.size);
    u.in_len = u.cut.ok ? u.cut.end - u.cut.start + kResetHeaderBytes : 0;
    u.place = u.cut.ok ? (uint64_t)(u.cut.start - p.span_start) + kResetHeaderBytes * j : 0;
    u.room = u.cut.ok ? b - g.base : 0;
    return w;
}

}  // namespace tamp_amd
