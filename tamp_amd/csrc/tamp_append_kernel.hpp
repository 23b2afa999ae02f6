// tamp_append_kernel.hpp -- bytes appended to reset-segmented streams, the closed segments kept at exactly N decoded bytes
// (tamp_batch_append, DESIGN.md 3.13 "Appending"; the arithmetic: tamp_append.hpp).
//
// A stream that receives L > 0 bytes has its OPEN segment decoded (m <= N bytes), the m + L bytes cut at every N into units, every
// unit compressed as a segment of its own and the units placed behind the stream's old bytes in front of the open segment, which
// are not looked at.  The rows of the call's tables are sized from L alone -- ceil(L / N) closed rows and one open row per
// appending stream (append_entry_bound) -- so that nothing waits for the decode; the one closed row that m may leave without a unit
// is compressed as an empty input and dropped.  The steps are kernels of their own on the call's stream; no workgroup waits for
// another, and the only atomics are 64-bit minima into a failing stream's word:
//   tamp_append_order_kernel     one workgroup: which streams' rows of reset_first hold -- in order and behind every usable pair in front,
//                                so that the entries of two streams that hold never overlap
//   tamp_append_plan_kernel      a lane per stream: budget, header, rows of the index, the open segment's cut, whether it is decoded
//   tamp_append_scan_kernel      one workgroup, the shared tile scan: closed rows and open rows in front of every stream, the record
//   tamp_append_rows_kernel      a lane per row of the slice: its owner (binary search in the scans), its staging row and slab; per
//                                open row the range that reads the open segment, delivered to the stream's first closed row
//   (the decode: launch_read_ranges_locked over the open rows' ranges; its walk carries the checks of the open segment)
//   tamp_append_assemble_kernel  a workgroup per row: m, the unit the row holds, its source bytes behind the decoded ones, 16-byte
//                                vectors where source and row are co-aligned, dwords otherwise; the literal width
//   (the compress: launch_compress_locked over the closed rows with the FLUSH token, over the open rows without)
//   tamp_append_splice_kernel    a workgroup per stream: the entries in front, the spans of the new units scanned from the open
//                                segment's old start = the new entries, out_len, status; the stream's entries into a staging table
//   tamp_append_gather_kernel    a workgroup per row and per stream: the units from their slabs, the old prefix in one copy
//   tamp_append_index_kernel     one workgroup: new_reset_first, the scan of the streams' entry counts
//   tamp_append_entries_kernel   a workgroup per stream: its entries from the staging table to new_reset_off
#pragma once
#include "tamp_common.hpp"
#include "tamp_append.hpp"
#include "tamp_write_ranges_kernel.hpp"

namespace tamp_amd {

// The caller's tables (device memory; a host-memory call: its copies).
struct AppendCaller {
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    const uint64_t* first;
    const uint32_t* off;
    uint64_t n;
    uint32_t interval, max_wbits;
    uint32_t header;  // what conf makes of a stream's first header byte (the second one is zero)
    uint32_t literal;
    const uint8_t* src;
    const uint64_t* src_off;
    const uint32_t* src_len;
};

// Per call, in the stream's scratch.
struct AppendTables {
    uint64_t* fail;          // n: write_fail_key of the first rule that fails the stream
    uint64_t* closed_first;  // n + 1: closed rows in front of the stream
    uint64_t* app_first;     // n + 1: open rows (= appending streams) in front of it
    uint64_t* count;         // n: the plan's entry bound, then the stream's entries in the new index
    uint8_t* need;           // n: 0 no rows, 1 appended to without a decode (an empty open segment), 2 the open segment is decoded
    uint8_t* whole;          // n: nothing is appended and the stream fits: it is copied in one piece
    uint8_t* hold;           // n: the stream's rows of reset_first hold (append_rows_hold)
    uint32_t* entries;       // the new entries of stream i from reset_first[i] + closed_first[i] on: old ones, then new ones
    uint64_t entries_cap;
};
struct AppendRecord { uint64_t closed, appends, entries, bound, decodes; };  // what a device-memory call reads back (40 bytes)

// A slice: the streams [i0, i1), their closed rows [c0, c0 + C) and open rows [a0, a0 + A).  Row x < C is a closed row, C + a an open one.
struct AppendSlice {
    uint64_t i0, i1;
    uint64_t c0, C, a0, A;
    uint8_t* region;     // the rows' tables, the staging rows, the slabs
    uint32_t row, slab;  // bytes of a staging row and of a slab
};
// The rows' tables.  Offsets count from the region.  U = C + A.
struct AppendRows {
    uint64_t* row_off;       // U: the staging row: what the compress kernel reads
    uint64_t* slab_off;      // U: where it is compressed to
    uint64_t* range_begin;   // A: the range that reads the open segment: E * N ...
    uint64_t* range_out;     // A: ... into the head of the stream's first closed row
    uint32_t* in_len;        // U: <- the assemble: bytes of the unit; 0: no unit
    uint32_t* cap;           // U
    uint32_t* out_len;       // U: <- the compress
    uint32_t* owner;         // U
    uint32_t* j;             // U: which of the owner's closed rows
    uint32_t* pos;           // U: <- the splice: where the unit starts in the new stream
    uint32_t* range_stream;  // A
    uint32_t* range_len;     // A: N, or 0 where nothing is decoded
    uint32_t* m;             // A: <- the read: decoded bytes of the open segment
    int8_t* status;          // U: <- the compress
    int8_t* read_status;     // A
};
constexpr uint64_t kAppendUnitRow = 80;  // bytes of table rows a unit takes at most (41 per row, 29 per open row); the budget counts them
__host__ __device__ constexpr uint64_t append_rows_bytes(uint64_t U, uint64_t A) { return (41 * U + 29 * A + 255) & ~255ull; }
__host__ __device__ inline AppendRows append_rows_at(uint8_t* base, uint64_t U, uint64_t A) {
    AppendRows r;
    r.row_off = reinterpret_cast<uint64_t*>(base), r.slab_off = r.row_off + U, r.range_begin = r.slab_off + U, r.range_out = r.range_begin + A;
    r.in_len = reinterpret_cast<uint32_t*>(r.range_out + A), r.cap = r.in_len + U, r.out_len = r.cap + U, r.owner = r.out_len + U;
    r.j = r.owner + U, r.pos = r.j + U, r.range_stream = r.pos + U, r.range_len = r.range_stream + A, r.m = r.range_len + A;
    r.status = reinterpret_cast<int8_t*>(r.m + A), r.read_status = r.status + U;
    return r;
}
__host__ __device__ constexpr uint64_t append_stage_at(uint64_t U, uint64_t A) { return append_rows_bytes(U, A); }
// (the slack of 64 bytes: the compress kernel's vector loads may run past a row's last byte)
__host__ __device__ constexpr uint64_t append_slabs_at(uint64_t U, uint64_t A, uint32_t row) { return (append_stage_at(U, A) + U * row + 64 + 255) & ~255ull; }
__host__ __device__ constexpr uint64_t append_region_bytes(uint64_t U, uint64_t A, uint32_t row, uint32_t slab) { return append_slabs_at(U, A, row) + U * slab + 64; }
__host__ __device__ constexpr uint64_t append_unit_cost(uint32_t N, uint32_t slab) { return (uint64_t)write_row_bytes(N) + slab + kAppendUnitRow; }

__device__ __forceinline__ void append_fail(uint64_t* fail, uint64_t i, uint64_t unit, uint32_t rank, int32_t code) {
    atomicMin(reinterpret_cast<unsigned long long*>(fail + i), (unsigned long long)write_fail_key(unit, rank, code));
}
__device__ __forceinline__ bool append_header_ok(const AppendCaller& c, uint64_t i) {
    if (c.in_len[i] < kResetHeaderBytes || c.max_wbits > 15) return false;
    const uint8_t* const s = c.in + c.in_off[i];
    return s[0] == c.header && s[1] == 0 && ((c.header >> 5) & 7u) + 8 <= c.max_wbits;
}
// Stream i's rows of reset_first hold (append_rows_hold: in order, inside the table, behind every usable row pair in front), and
// there is a table for its entries.
__device__ __forceinline__ bool append_index_ok(const AppendCaller& c, const AppendTables& t, uint64_t i) {
    return t.hold[i] && read_index_usable(c.first, c.n, i) && (c.off || c.first[i + 1] == c.first[i]);
}

struct AppendOrderArgs {
    AppendCaller c;
    AppendTables t;
};
// One workgroup: append_rows_hold for every stream.  A thread takes a run of neighbouring streams: the largest usable end of its
// run, the largest of the runs in front, then its streams in order.
__global__ void __launch_bounds__(kResetScanTile) tamp_append_order_kernel(AppendOrderArgs a) {
    __shared__ uint64_t run_end[kResetScanTile];
    const uint64_t n = a.c.n, run = (n + kResetScanTile - 1) / kResetScanTile;
    const uint64_t lo = min((uint64_t)threadIdx.x * run, n), hi = min(lo + run, n);
    uint64_t end = 0;
    for (uint64_t i = lo; i < hi; i++)
        if (read_index_usable(a.c.first, n, i)) end = max(end, a.c.first[i + 1]);
    run_end[threadIdx.x] = end;
    __syncthreads();
    uint64_t before = 0;
    for (uint32_t w = 0; w < threadIdx.x; w++) before = max(before, run_end[w]);
    for (uint64_t i = lo; i < hi; i++) {
        const bool usable = read_index_usable(a.c.first, n, i);
        a.t.hold[i] = usable && a.c.first[i] >= before ? 1 : 0;
        if (usable) before = max(before, a.c.first[i + 1]);
    }
}

struct AppendPlanArgs {
    AppendCaller c;
    AppendTables t;
    uint64_t max_units;  // rows of one stream: what the scratch budget holds
};
__global__ void __launch_bounds__(256) tamp_append_plan_kernel(AppendPlanArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.c.n) return;
    const uint32_t L = a.c.src_len[i];
    const uint64_t B = append_entry_bound(L, a.c.interval);
    uint64_t rows = 0, fail = kWriteNoFail;
    uint8_t need = 0;
    if (L) {  // (nothing appended: the stream is not looked at)
        if (B + 1 > a.max_units) fail = write_fail_key(0, kAppendRankBudget, kBadArgument);
        else if (!append_header_ok(a.c, i)) fail = write_fail_key(0, kAppendRankConf, kInvalidConf);
        else if (!append_index_ok(a.c, a.t, i)) fail = write_fail_key(0, kAppendRankFirst, kReadBadIndex);
        else {
            const ReadCut cut = read_segment_cut(a.c.first, a.c.off, a.c.in_len, i, a.c.first[i + 1] - a.c.first[i]);
            if (!cut.ok) fail = write_fail_key(0, kAppendRankEntries, kReadBadIndex);
            else rows = B, need = cut.end > cut.start ? 2 : 1;
        }
    }
    a.t.fail[i] = fail, a.t.closed_first[i] = rows, a.t.app_first[i] = need ? 1 : 0, a.t.count[i] = B;
    a.t.need[i] = need, a.t.whole[i] = 0;
}

struct AppendScanArgs {
    AppendCaller c;
    AppendTables t;
    AppendRecord* rec;
};
__global__ void __launch_bounds__(kResetScanTile) tamp_append_scan_kernel(AppendScanArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    uint64_t closed = 0, apps = 0, bound = 0, decodes = 0;
    for (uint64_t t0 = 0; t0 < a.c.n; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint64_t i = t0 + threadIdx.x;
        const bool live = i < a.c.n;
        uint64_t tile;
        const uint64_t c_at = closed + reset_tile_scan(live ? a.t.closed_first[i] : 0, wave_sum, tile);
        closed += tile;
        const uint64_t a_at = apps + reset_tile_scan(live ? a.t.app_first[i] : 0, wave_sum, tile);
        apps += tile;
        (void)reset_tile_scan(live ? a.t.count[i] : 0, wave_sum, tile);
        bound += tile;
        (void)reset_tile_scan(live && a.t.need[i] == 2 ? 1 : 0, wave_sum, tile);
        decodes += tile;
        if (live) a.t.closed_first[i] = c_at, a.t.app_first[i] = a_at;
    }
    if (threadIdx.x == 0) {
        a.t.closed_first[a.c.n] = closed, a.t.app_first[a.c.n] = apps;
        a.rec->closed = closed, a.rec->appends = apps, a.rec->entries = a.c.first[a.c.n], a.rec->bound = bound, a.rec->decodes = decodes;
    }
}

struct AppendRowsArgs {
    AppendCaller c;
    AppendTables t;
    AppendSlice s;
};
__global__ void __launch_bounds__(256) tamp_append_rows_kernel(AppendRowsArgs a) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, U = a.s.C + a.s.A;
    if (x >= U) return;
    const bool open = x >= a.s.C;
    const uint64_t* const scan = open ? a.t.app_first : a.t.closed_first;
    const uint64_t g = open ? a.s.a0 + (x - a.s.C) : a.s.c0 + x;
    uint64_t lo = a.s.i0, hi = a.s.i1;  // scan[lo] <= g < scan[hi] (streams without rows are stepped over)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (scan[mid] <= g) lo = mid;
        else hi = mid;
    }
    const uint64_t i = lo;
    const AppendRows w = append_rows_at(a.s.region, U, a.s.A);
    w.row_off[x] = append_stage_at(U, a.s.A) + x * a.s.row;
    w.slab_off[x] = append_slabs_at(U, a.s.A, a.s.row) + x * a.s.slab, w.cap[x] = a.s.slab;
    w.owner[x] = (uint32_t)i, w.j[x] = open ? 0xFFFFFFFFu : (uint32_t)(g - scan[i]);
    if (!open) return;
    const uint64_t r = x - a.s.C;
    const bool ok = append_index_ok(a.c, a.t, i) && a.t.closed_first[i] >= a.s.c0 && a.t.closed_first[i] - a.s.c0 < a.s.C;
    w.range_stream[r] = (uint32_t)i, w.range_len[r] = ok && a.t.need[i] == 2 ? a.c.interval : 0;
    w.range_begin[r] = ok ? (a.c.first[i + 1] - a.c.first[i]) * a.c.interval : 0;
    w.range_out[r] = append_stage_at(U, a.s.A) + (ok ? a.t.closed_first[i] - a.s.c0 : 0) * a.s.row;
}

// What a row of the slice holds once the open segments are decoded.  ok = false: no unit (its stream failed, or the closed row is
// the one that m leaves over).
struct AppendUnit {
    bool ok;
    uint32_t m;
    uint64_t U, j;
    uint64_t first_row;  // the stream's first closed row, where its open segment was decoded to
    int32_t rank, code;  // ok = false and rank != 0: the rule that fails the stream
};
__device__ __forceinline__ AppendUnit append_row_unit(const AppendCaller& c, const AppendTables& t, const AppendSlice& s, const AppendRows& w, uint64_t x) {
    AppendUnit u = {false, 0, 0, 0, 0, 0, 0};
    const uint64_t i = w.owner[x];
    if (i < s.i0 || i >= s.i1 || t.app_first[i] < s.a0 || t.app_first[i] - s.a0 >= s.A || t.closed_first[i] < s.c0) return u;
    const uint64_t r = t.app_first[i] - s.a0;
    u.first_row = t.closed_first[i] - s.c0;
    if (u.first_row >= s.C) return u;
    if (t.need[i] == 2) {
        const int32_t st = w.read_status[r];
        if (st != kOk && st != kInputExhausted) {
            u.code = st;
            u.rank = st == kOob ? kAppendRankOob : (st == kReadBadIndex ? kAppendRankIndex : (st == kBadArgument ? kAppendRankBudget : kAppendRankDecode));
            return u;
        }
        u.m = w.m[r];
        if (u.m > c.interval) {
            u.code = kReadBadIndex, u.rank = kAppendRankIndex;
            return u;
        }
    }
    u.U = append_units(u.m, c.src_len[i], c.interval);
    const bool open = x >= s.C;
    u.j = open ? u.U - 1 : w.j[x];
    u.ok = open || (append_closed_row_used(u.j, u.U) && u.first_row + u.j == x);
    return u;
}

struct AppendAssembleArgs {
    AppendCaller c;
    AppendTables t;
    AppendSlice s;
};
__global__ void __launch_bounds__(256) tamp_append_assemble_kernel(AppendAssembleArgs a) {
    const uint64_t U = a.s.C + a.s.A;
    const AppendRows w = append_rows_at(a.s.region, U, a.s.A);
    const uint32_t N = a.c.interval;
    const uint32_t mask4 = ((0xFFu << a.c.literal) & 0xFFu) * 0x01010101u;
    for (uint64_t x = blockIdx.x; x < U; x += gridDim.x) {
        const AppendUnit u = append_row_unit(a.c, a.t, a.s, w, x);
        const uint64_t i = w.owner[x];
        if (!u.ok) {  // (in_len stays 0: an empty input for the compress kernel)
            if (u.rank && threadIdx.x == 0) append_fail(a.t.fail, i, 0, u.rank, u.code);
            continue;
        }
        const AppendCut cut = append_cut(u.m, a.c.src_len[i], N, u.j);
        if (cut.len > N) continue;
        if (threadIdx.x == 0) w.in_len[x] = cut.len;
        uint8_t* const dst = a.s.region + w.row_off[x];
        // the decoded bytes stand in the stream's first closed row: they are there already, or (one unit in all: the open row) move
        const uint8_t* const old = a.s.region + append_stage_at(U, a.s.A) + u.first_row * a.s.row;
        if (cut.old_len && dst != old) (void)write_copy(dst, old, cut.old_len, 0);
        if (write_copy(dst + cut.old_len, a.c.src + a.c.src_off[i] + cut.src_at, cut.len - cut.old_len, mask4))
            append_fail(a.t.fail, i, 0, kAppendRankExcess, kExcessBits);
    }
}

struct AppendSpliceArgs {
    AppendCaller c;
    AppendTables t;
    AppendSlice s;
    const uint32_t* out_cap;  // the caller's tables
    uint32_t* out_len;
    int8_t* status;
};
__global__ void __launch_bounds__(kResetScanTile) tamp_append_splice_kernel(AppendSpliceArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    __shared__ unsigned long long err_s;
    const uint64_t rows = a.s.C + a.s.A;
    const AppendRows w = append_rows_at(a.s.region, rows, a.s.A);
    for (uint64_t i = a.s.i0 + blockIdx.x; i < a.s.i1; i += gridDim.x) {  // (everything below is uniform over the workgroup)
        const bool usable = append_index_ok(a.c, a.t, i);
        const uint64_t E = usable ? a.c.first[i + 1] - a.c.first[i] : 0, f0 = a.c.first[i], tb = f0 + a.t.closed_first[i];
        const bool room = usable && tb >= f0 && tb + E >= tb && tb + E <= a.t.entries_cap;  // (tables that changed behind the scan: no entries)
        const uint32_t L = a.c.src_len[i];
        if (L == 0) {  // copied as it stands, whatever it holds; its entries with it
            const uint32_t len = a.c.in_len[i];
            const bool fits = len <= a.out_cap[i];
            if (threadIdx.x == 0) a.status[i] = fits ? (int8_t)kOk : (int8_t)kOutputFull, a.out_len[i] = fits ? len : 0, a.t.whole[i] = fits ? 1 : 0, a.t.count[i] = room ? E : 0;
            if (room)
                for (uint64_t k = threadIdx.x; k < E; k += kResetScanTile) a.t.entries[tb + k] = a.c.off[f0 + k];
            continue;
        }
        if (threadIdx.x == 0) err_s = a.t.fail[i];
        __syncthreads();
        // the entries in front of the open segment: range and order alone
        int bad = 0;
        for (uint64_t k0 = 0; k0 < E; k0 += kResetScanTile)
            bad |= __syncthreads_or(k0 + threadIdx.x < E && !read_segment_cut(a.c.first, a.c.off, a.c.in_len, i, k0 + threadIdx.x).ok);
        if (bad && threadIdx.x == 0) atomicMin(&err_s, (unsigned long long)write_fail_key(0, kAppendRankEntries, kReadBadIndex));
        __syncthreads();
        const bool go = err_s == kWriteNoFail && room && a.t.need[i] != 0 && a.t.app_first[i] >= a.s.a0 && a.t.app_first[i] - a.s.a0 < a.s.A;
        uint64_t U = 0, base = 0;
        if (go) {
            const AppendUnit head = append_row_unit(a.c, a.t, a.s, w, a.s.C + (a.t.app_first[i] - a.s.a0));  // (the open row: m and U)
            if (!head.ok) {
                if (threadIdx.x == 0) atomicMin(&err_s, (unsigned long long)write_fail_key(0, head.rank ? head.rank : kAppendRankIndex, head.rank ? head.code : (int32_t)kReadBadIndex));
            } else {
                U = head.U, base = read_segment_cut(a.c.first, a.c.off, a.c.in_len, i, E).start;
                for (uint64_t j0 = 0; j0 < U; j0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
                    const uint64_t j = j0 + threadIdx.x;
                    const bool live = j < U, closed = j + 1 < U;
                    const uint64_t x = closed ? head.first_row + j : a.s.C + (a.t.app_first[i] - a.s.a0);
                    uint32_t len = 0;
                    if (live && (x >= rows || (closed && x >= a.s.C)))
                        atomicMin(&err_s, (unsigned long long)write_fail_key(j, kAppendRankIndex, kReadBadIndex));
                    else if (live && (w.status[x] != kOk || w.out_len[x] < kResetHeaderBytes || w.out_len[x] > a.s.slab))
                        atomicMin(&err_s, (unsigned long long)write_fail_key(j, kAppendRankCompress, w.status[x] != kOk ? w.status[x] : (int32_t)kError));
                    else if (live) len = write_unit_span(w.out_len[x], closed);
                    uint64_t tile;
                    const uint64_t at = base + reset_tile_scan(len, wave_sum, tile);
                    if (live && x < rows) {
                        w.pos[x] = (uint32_t)at;
                        if (closed && tb + E + j < a.t.entries_cap) a.t.entries[tb + E + j] = (uint32_t)(at + len);
                    }
                    base += tile;
                }
            }
        }
        __syncthreads();
        const uint64_t err = err_s;
        const bool done = go && err == kWriteNoFail && U;
        const int32_t st = err != kWriteNoFail ? write_fail_code(err) : (!done ? (int32_t)kReadBadIndex : (append_fits(base, a.out_cap[i]) ? (int32_t)kOk : (int32_t)kOutputFull));
        if (room)  // the old entries in front of the new ones; a failing stream keeps its rows, zeroed
            for (uint64_t k = threadIdx.x; k < E; k += kResetScanTile) a.t.entries[tb + k] = st == kOk ? a.c.off[f0 + k] : 0;
        if (threadIdx.x == 0) a.status[i] = (int8_t)st, a.out_len[i] = st == kOk ? (uint32_t)base : 0, a.t.count[i] = room ? E + (st == kOk ? U - 1 : 0) : 0;
        __syncthreads();  // (the next stream of this workgroup sets the word again)
    }
}

struct AppendGatherArgs {
    AppendCaller c;
    AppendTables t;
    AppendSlice s;
    uint8_t* out;  // the caller's buffer and tables
    const uint64_t* out_off;
    const uint32_t* out_cap;  // nothing is written at or behind out + out_off[i] + out_cap[i]
    const int8_t* status;
    const uint32_t* out_len;
};
// One workgroup per row of the slice, then per stream of the slice (the old bytes: all of them, or those in front of the open
// segment), grid-strided.  Every byte of a new stream has one writer.
__global__ void __launch_bounds__(256) tamp_append_gather_kernel(AppendGatherArgs a) {
    const uint64_t rows = a.s.C + a.s.A;
    const AppendRows w = append_rows_at(a.s.region, rows, a.s.A);
    const uint64_t items = rows + (a.s.i1 - a.s.i0);
    for (uint64_t x = blockIdx.x; x < items; x += gridDim.x) {
        if (x >= rows) {
            const uint64_t i = a.s.i0 + (x - rows);
            if (a.status[i] != kOk) continue;
            uint32_t len = a.c.in_len[i];
            if (!a.t.whole[i]) {
                if (!append_index_ok(a.c, a.t, i) || a.c.src_len[i] == 0) continue;
                const ReadCut cut = read_segment_cut(a.c.first, a.c.off, a.c.in_len, i, a.c.first[i + 1] - a.c.first[i]);
                if (!cut.ok) continue;
                len = cut.start;
            }
            if (len <= a.out_cap[i] && len <= a.out_len[i]) reset_copy(a.out + a.out_off[i], a.c.in + a.c.in_off[i], len, false, 0);
            continue;
        }
        const uint32_t i = w.owner[x];
        if (i < a.s.i0 || i >= a.s.i1 || a.status[i] != kOk || a.t.whole[i]) continue;
        const AppendUnit u = append_row_unit(a.c, a.t, a.s, w, x);
        if (!u.ok) continue;
        const bool closed = u.j + 1 < u.U;
        const uint32_t have = w.out_len[x];
        if (have < kResetHeaderBytes || have > a.s.slab) continue;
        const uint64_t pos = w.pos[x], span = write_unit_span(have, closed);
        if (pos + span > a.out_cap[i] || pos + span > a.out_len[i]) continue;  // (a stream that fits: never)
        uint8_t* const dst = a.out + a.out_off[i] + pos;
        const uint8_t* const slab = a.s.region + w.slab_off[x];
        const uint32_t body = have - kResetHeaderBytes;
        reset_copy(dst, slab + kResetHeaderBytes, body, false, 0);
        // a closed segment ends with the next one's lead, the reset's second FLUSH: the two bytes every slab starts with
        if (closed && threadIdx.x >= 64 && threadIdx.x < 66) dst[body + (threadIdx.x - 64)] = slab[threadIdx.x - 64];
    }
}

struct AppendIndexArgs {
    AppendTables t;
    uint64_t n;
    uint64_t* new_first;  // n + 1
};
__global__ void __launch_bounds__(kResetScanTile) tamp_append_index_kernel(AppendIndexArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    uint64_t base = 0;
    for (uint64_t t0 = 0; t0 < a.n; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint64_t i = t0 + threadIdx.x;
        uint64_t tile;
        const uint64_t at = base + reset_tile_scan(i < a.n ? a.t.count[i] : 0, wave_sum, tile);
        if (i < a.n) a.new_first[i] = at;
        base += tile;
    }
    if (threadIdx.x == 0) a.new_first[a.n] = base;
}

struct AppendEntriesArgs {
    AppendCaller c;
    AppendTables t;
    const uint64_t* new_first;
    uint32_t* new_off;
    uint64_t new_cap;
};
__global__ void __launch_bounds__(256) tamp_append_entries_kernel(AppendEntriesArgs a) {
    for (uint64_t i = blockIdx.x; i < a.c.n; i += gridDim.x) {
        const uint64_t count = a.t.count[i], tb = a.c.first[i] + a.t.closed_first[i], at = a.new_first[i];
        if (!count || tb + count < tb || tb + count > a.t.entries_cap || at + count < at || at + count > a.new_cap) continue;
        for (uint64_t k = threadIdx.x; k < count; k += blockDim.x) a.new_off[at + k] = a.t.entries[tb + k];
    }
}

}  // namespace tamp_amd
