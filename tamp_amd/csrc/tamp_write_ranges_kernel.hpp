// tamp_write_ranges_kernel.hpp -- byte ranges written into reset-segmented streams (tamp_batch_write_ranges, DESIGN.md 3.13
// "Writing ranges"; the arithmetic: tamp_write_ranges.hpp).
//
// A write touches a few segments of one stream.  Every touched segment of the batch is ONE unit, however many writes lie in it:
// decoded into a staging row of N bytes (by tamp_batch_read_ranges' own steps, one range per unit), patched, compressed again as a
// segment of its own, and spliced between the untouched segments, which keep their bytes.  The steps are kernels of their own on the
// call's stream; no workgroup waits for another, and the only atomics are 64-bit minima into a failing stream's word:
//   tamp_write_plan_kernel     a lane per write: order against its predecessor, header, rows of the index, the touched segments
//                              k0 .. k1 in 64 bits, a byte flag per touched segment (plain stores of one value per segment)
//   tamp_write_scan_kernel     one workgroup, the shared tile scan over the flags: the unit of every touched segment, how many of
//                              them are open segments, the 16-byte record of the call
//   tamp_write_streams_kernel  a lane per stream: where its units start in that scan; a stream whose units outgrow the budget
//   tamp_write_rows_kernel     a lane per unit of the slice: its segment (binary search in the scan), its owner, the range that
//                              reads it, its staging row and slab.  Rows stand closed units first, open ones behind them: the
//                              compress launch takes one way of closing its streams
//   (the decode: launch_read_ranges_locked over the rows; its walk carries the checks of the index)
//   tamp_write_patch_kernel    a workgroup per write, piece by piece: source bytes into the rows, 16-byte vectors where source and
//                              row are co-aligned, dwords otherwise; literal width, the write's end against the open segment's size
//   (the compress: launch_compress_locked over the closed rows with the FLUSH token, over the open rows without)
//   tamp_write_splice_kernel   a workgroup per stream: the new length of every segment, their exclusive scan = the new index,
//                              out_len, status
//   tamp_write_gather_kernel   a workgroup per segment of the batch: from the old stream or from the unit's slab to its new place,
//                              the header in front of segment 0; a stream no write touches is one copy
#pragma once
#include "tamp_common.hpp"
#include "tamp_write_ranges.hpp"
#include "tamp_reset_segments_kernel.hpp"

namespace tamp_amd {

constexpr uint32_t kWriteNoOwner = 0xFFFFFFFFu;

// The caller's tables (device memory; a host-memory call: its copies).
struct WriteCaller {
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    const uint64_t* first;
    const uint32_t* off;
    uint64_t n;
    uint32_t interval, max_wbits;
    uint32_t header;   // what conf makes of a stream's first header byte (the second one is zero)
    uint32_t literal;
    const uint32_t* write_stream;
    const uint64_t* write_begin;
    const uint32_t* write_len;
    const uint8_t* src;
    const uint64_t* src_off;
    uint64_t n_writes;
};

// Per call, in the stream's scratch.  S = reset_first[n] + n segments in all; segment k of stream i is g = reset_first[i] + i + k.
struct WriteTables {
    uint64_t S;
    uint64_t* fail;        // n: write_fail_key of the lowest (write, rule) that fails the stream
    uint64_t* fail0;       // n: the same as the plan left it (the patch skips those streams)
    uint64_t* unit_first;  // n + 1: the scan below at each stream's first segment
    uint64_t* open_first;  // n + 1
    uint8_t* flags;        // S: 0 untouched, 1 a touched closed segment, 2 a touched open one
    uint32_t* unit_at;     // S + 1: touched segments in front of g
    uint32_t* open_at;     // S + 1: touched open segments in front of g
    uint32_t* new_pos;     // S: where the segment starts in its new stream
    uint32_t* new_len;     // S
    uint32_t* owner;       // S: the stream the splice placed the segment for
    uint8_t* whole;        // n: no write touches the stream: it is copied in one piece
};
struct WriteRecord { uint64_t units, open_units; };  // what a device-memory call reads back

// A slice: the streams [i0, i1) and their units [u0, u0 + U), Uo of them open segments (o0 open units lie in front of the slice).
struct WriteSlice {
    uint64_t i0, i1;
    uint64_t u0, U, o0, Uo;
    uint8_t* region;  // the units' rows, the staging rows, the slabs
    uint32_t row, slab;  // bytes of a staging row and of a slab
};
// The units' rows.  Offsets count from the region.
struct WriteRows {
    uint64_t* begin;      // the range that reads the unit: k * N
    uint64_t* row_off;    // its staging row: where the range is delivered, what the compress kernel reads
    uint64_t* slab_off;   // where it is compressed to
    uint32_t* stream;     // its owner
    uint32_t* len;        // N; 0: no unit (tables that changed behind the scan)
    uint32_t* size;       // <- the read: decoded bytes
    uint32_t* cap;
    uint32_t* out_len;    // <- the compress
    int8_t* read_status;
    int8_t* status;       // <- the compress
};
static_assert(3 * 8 + 5 * 4 + 2 <= kWriteUnitRow, "a unit's rows stay inside what the budget counts for them");
__host__ __device__ constexpr uint64_t write_rows_bytes(uint64_t U) { return (46 * U + 255) & ~255ull; }
__host__ __device__ inline WriteRows write_rows_at(uint8_t* base, uint64_t U) {
    WriteRows r;
    r.begin = reinterpret_cast<uint64_t*>(base), r.row_off = r.begin + U, r.slab_off = r.row_off + U;
    r.stream = reinterpret_cast<uint32_t*>(r.slab_off + U), r.len = r.stream + U, r.size = r.len + U, r.cap = r.size + U;
    r.out_len = r.cap + U;
    r.read_status = reinterpret_cast<int8_t*>(r.out_len + U), r.status = r.read_status + U;
    return r;
}
__host__ __device__ constexpr uint64_t write_stage_at(uint64_t U) { return write_rows_bytes(U); }
// (the slack of 64 bytes: the compress kernel's vector loads may run past a row's last byte)
__host__ __device__ constexpr uint64_t write_slabs_at(uint64_t U, uint32_t row) { return (write_stage_at(U) + U * row + 64 + 255) & ~255ull; }
__host__ __device__ constexpr uint64_t write_region_bytes(uint64_t U, uint32_t row, uint32_t slab) { return write_slabs_at(U, row) + U * slab + 64; }

// The row of the unit of touched segment g; >= U: none (tables that changed behind the scan).
__device__ __forceinline__ uint64_t write_row_of(const WriteTables& t, const WriteSlice& s, uint64_t g) {
    const uint64_t x = (uint64_t)t.unit_at[g] - s.u0, o = (uint64_t)t.open_at[g] - s.o0;
    return t.flags[g] == 2 ? (s.U - s.Uo) + o : x - o;
}
__device__ __forceinline__ void write_fail(uint64_t* fail, uint64_t i, uint64_t q, uint32_t rank, int32_t code) {
    atomicMin(reinterpret_cast<unsigned long long*>(fail + i), (unsigned long long)write_fail_key(q, rank, code));
}
// Stream i may be written under the call's conf: the reset bit (with it the second header byte, which must be zero), no custom
// dictionary, window, literal and extended as conf says, a window the call accepts.
__device__ __forceinline__ bool write_header_ok(const WriteCaller& c, uint64_t i) {
    if (c.in_len[i] < kResetHeaderBytes || c.max_wbits > 15) return false;
    const uint8_t* const s = c.in + c.in_off[i];
    return s[0] == c.header && s[1] == 0 && ((c.header >> 5) & 7u) + 8 <= c.max_wbits;
}
__device__ __forceinline__ bool write_index_ok(const WriteCaller& c, uint64_t i) {
    return read_index_usable(c.first, c.n, i) && (c.off || c.first[i + 1] == c.first[i]);  // (entries and no table to hold them)
}

struct WritePlanArgs {
    WriteCaller c;
    WriteTables t;
};
__global__ void __launch_bounds__(256) tamp_write_plan_kernel(WritePlanArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.c.n_writes) return;
    const uint32_t i = a.c.write_stream[q];
    if (i >= a.c.n) return;  // (no stream to fail: the write is ignored)
    const uint64_t begin = a.c.write_begin[q];
    const uint32_t len = a.c.write_len[q];
    if (q && !write_in_order(a.c.write_stream[q - 1], a.c.write_begin[q - 1], a.c.write_len[q - 1], i, begin))
        return write_fail(a.t.fail, i, q, kWriteRankOrder, kBadArgument);
    if (len == 0) return;  // (touches nothing: the stream is not looked at)
    if (!write_header_ok(a.c, i)) return write_fail(a.t.fail, i, q, kWriteRankConf, kInvalidConf);
    if (!write_index_ok(a.c, i)) return write_fail(a.t.fail, i, q, kWriteRankFirst, kReadBadIndex);
    const uint64_t E = a.c.first[i + 1] - a.c.first[i], key = a.c.first[i] + i;
    const WriteSpan s = write_span(E, a.c.interval, begin, len);
    if (!s.ok) return write_fail(a.t.fail, i, q, kWriteRankEnd, kInputExhausted);
    // (key + k <= reset_first[i + 1] + i < S: the rows held up.  Two writes in one segment store the same value)
    for (uint64_t k = s.k0; k <= s.k1; k++) a.t.flags[key + k] = k == E ? 2 : 1;
}

struct WriteScanArgs {
    WriteTables t;
    WriteRecord* rec;
};
__global__ void __launch_bounds__(kResetScanTile) tamp_write_scan_kernel(WriteScanArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    uint64_t units = 0, opens = 0;
    for (uint64_t t0 = 0; t0 < a.t.S; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint64_t g = t0 + threadIdx.x;
        const uint32_t f = g < a.t.S ? a.t.flags[g] : 0;
        uint64_t tile;
        const uint64_t u_at = units + reset_tile_scan(f != 0 ? 1 : 0, wave_sum, tile);
        units += tile;
        const uint64_t o_at = opens + reset_tile_scan(f == 2 ? 1 : 0, wave_sum, tile);
        opens += tile;
        // (more than 2^32 - 2 units: the call is refused from the record, nothing is read through the truncated values)
        if (g < a.t.S) a.t.unit_at[g] = (uint32_t)u_at, a.t.open_at[g] = (uint32_t)o_at;
    }
    if (threadIdx.x == 0) {
        a.t.unit_at[a.t.S] = (uint32_t)units, a.t.open_at[a.t.S] = (uint32_t)opens;
        a.rec->units = units, a.rec->open_units = opens;
    }
}

struct WriteStreamsArgs {
    WriteCaller c;
    WriteTables t;
    uint64_t max_units;  // of one stream: what the scratch budget holds
};
__global__ void __launch_bounds__(256) tamp_write_streams_kernel(WriteStreamsArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > a.c.n) return;
    auto at = [&](uint64_t j) {  // stream j's first segment, inside the scan whatever the table holds
        const uint64_t g = a.c.first[j] + j;
        return g < a.c.first[j] || g > a.t.S ? a.t.S : g;
    };
    const uint64_t g0 = at(i);
    a.t.unit_first[i] = a.t.unit_at[g0], a.t.open_first[i] = a.t.open_at[g0];
    if (i == a.c.n) return;
    const uint64_t g1 = at(i + 1);
    if (g1 >= g0 && (uint64_t)a.t.unit_at[g1] - a.t.unit_at[g0] > a.max_units) write_fail(a.t.fail, i, 0, kWriteRankBudget, kBadArgument);
}

struct WriteRowsArgs {
    WriteCaller c;
    WriteTables t;
    WriteSlice s;
};
__global__ void __launch_bounds__(256) tamp_write_rows_kernel(WriteRowsArgs a) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.s.U) return;
    const uint64_t u = a.s.u0 + x;
    uint64_t lo = 0, hi = a.t.S;  // unit_at[lo] <= u < unit_at[hi]: the last segment with u units in front of it is unit u
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.t.unit_at[mid] <= u) lo = mid;
        else hi = mid;
    }
    const uint64_t g = lo;
    if (!a.t.flags[g]) return;  // (the rows are zeroed: no unit)
    const uint64_t r = write_row_of(a.t, a.s, g);
    if (r >= a.s.U) return;
    uint64_t il = 0, ih = a.c.n;  // first[il] + il <= g < first[ih] + ih
    while (ih - il > 1) {
        const uint64_t mid = il + (ih - il) / 2;
        if (a.c.first[mid] + mid <= g) il = mid;
        else ih = mid;
    }
    const uint64_t i = il;
    const WriteRows w = write_rows_at(a.s.region, a.s.U);
    bool mine = i >= a.s.i0 && i < a.s.i1 && write_index_ok(a.c, i) && a.c.first[i] + i <= g;
    const uint64_t k = mine ? g - (a.c.first[i] + i) : 0;
    mine = mine && k <= a.c.first[i + 1] - a.c.first[i];
    w.begin[r] = k * a.c.interval, w.stream[r] = (uint32_t)i, w.len[r] = mine ? a.c.interval : 0;
    w.row_off[r] = write_stage_at(a.s.U) + r * a.s.row;
    w.slab_off[r] = write_slabs_at(a.s.U, a.s.row) + r * a.s.slab, w.cap[r] = a.s.slab;
}

// `len` bytes from src to dst by one workgroup, every byte of dst written once and nothing else of it: 16-byte vectors where source
// and destination are co-aligned, aligned dwords from unaligned loads otherwise, the bytes in front of and behind them as bytes.
// -> the bits of this thread's bytes that `mask4` (a byte mask, four times) selects.
__device__ __forceinline__ uint32_t write_copy(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t mask4) {
    uint32_t seen = 0;
    const bool wide = ((reinterpret_cast<uintptr_t>(dst) ^ reinterpret_cast<uintptr_t>(src)) & 15) == 0;
    const uint32_t unit = wide ? 16 : 4;
    const uint32_t head = min((uint32_t)((unit - (reinterpret_cast<uintptr_t>(dst) & (unit - 1))) & (unit - 1)), len);
    const uint32_t nv = (len - head) / unit, tail0 = head + unit * nv;
    if (wide) {
        for (uint32_t j = threadIdx.x; j < nv; j += blockDim.x) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + head + 16 * j);
            seen |= (v.x | v.y | v.z | v.w) & mask4;
            *reinterpret_cast<uint4*>(dst + head + 16 * j) = v;
        }
    } else {
        for (uint32_t j = threadIdx.x; j < nv; j += blockDim.x) {
            const uint32_t v = reinterpret_cast<const GlobalU32*>(src + head + 4 * j)->v;
            seen |= v & mask4;
            *reinterpret_cast<uint32_t*>(dst + head + 4 * j) = v;
        }
    }
    if (threadIdx.x < 30) {  // at most 15 bytes in front of the first vector and 15 behind the last
        const uint32_t i = threadIdx.x < 15 ? threadIdx.x : tail0 + (threadIdx.x - 15);
        const bool mine = threadIdx.x < 15 ? i < head : i < len;
        if (mine) {
            const uint8_t b = src[i];
            seen |= b & mask4;
            dst[i] = b;
        }
    }
    return seen;
}

struct WritePatchArgs {
    WriteCaller c;
    WriteTables t;
    WriteSlice s;
};
__global__ void __launch_bounds__(256) tamp_write_patch_kernel(WritePatchArgs a) {
    const WriteRows w = write_rows_at(a.s.region, a.s.U);
    const uint32_t N = a.c.interval;
    const uint32_t mask4 = ((0xFFu << a.c.literal) & 0xFFu) * 0x01010101u;
    for (uint64_t q = blockIdx.x; q < a.c.n_writes; q += gridDim.x) {
        const uint32_t i = a.c.write_stream[q], len = a.c.write_len[q];
        if (i < a.s.i0 || i >= a.s.i1 || len == 0 || a.t.fail0[i] != kWriteNoFail) continue;
        const uint64_t E = a.c.first[i + 1] - a.c.first[i], key = a.c.first[i] + i;
        const WriteSpan s = write_span(E, N, a.c.write_begin[q], len);
        if (!s.ok) continue;  // (the plan has failed the stream)
        const uint8_t* const src = a.c.src + a.c.src_off[q];
        for (uint64_t j = 0; j <= s.k1 - s.k0; j++) {
            const uint64_t k = s.k0 + j, r = write_row_of(a.t, a.s, key + k);
            const WritePiece p = write_piece(s, N, j);
            int32_t code = kOk;
            uint32_t rank = 0;
            // the unit of this very segment, decoded; then the write's end against what it decoded to
            if (r >= a.s.U || w.stream[r] != i || w.len[r] == 0 || w.begin[r] != k * N) rank = kWriteRankIndex, code = kReadBadIndex;
            else if (const int32_t st = w.read_status[r]; st != kOk && st != kInputExhausted)
                rank = st == kOob ? kWriteRankOob : (st == kReadBadIndex ? kWriteRankIndex : kWriteRankDecode), code = st;
            else if (p.hi > w.size[r]) rank = kWriteRankEnd, code = kInputExhausted;
            if (rank) {
                if (threadIdx.x == 0) write_fail(a.t.fail, i, q, rank, code);
                continue;
            }
            if (write_copy(a.s.region + w.row_off[r] + p.lo, src + p.skip, p.hi - p.lo, mask4)) write_fail(a.t.fail, i, q, kWriteRankExcess, kExcessBits);
        }
    }
}

struct WriteSpliceArgs {
    WriteCaller c;
    WriteTables t;
    WriteSlice s;
    const uint32_t* out_cap;  // the caller's tables
    uint32_t* out_len;
    int8_t* status;
    uint32_t* new_reset_off;  // may be null
};
__global__ void __launch_bounds__(kResetScanTile) tamp_write_splice_kernel(WriteSpliceArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    __shared__ unsigned long long err_s;
    const WriteRows w = write_rows_at(a.s.region, a.s.U);
    for (uint64_t i = a.s.i0 + blockIdx.x; i < a.s.i1; i += gridDim.x) {  // (everything below is uniform over the workgroup)
        const bool usable = write_index_ok(a.c, i);
        const uint64_t E = usable ? a.c.first[i + 1] - a.c.first[i] : 0, key = a.c.first[i] + i;
        const uint64_t f = a.t.fail[i];
        if (f != kWriteNoFail) {
            if (threadIdx.x == 0) a.status[i] = (int8_t)write_fail_code(f), a.out_len[i] = 0;
            continue;
        }
        int touched = 0;
        if (usable)
            for (uint64_t k0 = 0; k0 <= E; k0 += kResetScanTile) touched |= __syncthreads_or(k0 + threadIdx.x <= E && a.t.flags[key + k0 + threadIdx.x]);
        if (!touched) {  // copied as it stands, whatever it holds; its entries with it
            const uint32_t len = a.c.in_len[i];
            const bool fits = len <= a.out_cap[i];
            if (threadIdx.x == 0) a.status[i] = fits ? (int8_t)kOk : (int8_t)kOutputFull, a.out_len[i] = fits ? len : 0, a.t.whole[i] = fits ? 1 : 0;
            if (a.new_reset_off)
                for (uint64_t k = threadIdx.x; k < E; k += kResetScanTile) a.new_reset_off[a.c.first[i] + k] = a.c.off[a.c.first[i] + k];
            continue;
        }
        if (threadIdx.x == 0) err_s = kWriteNoFail;
        __syncthreads();
        uint64_t base = kResetHeaderBytes;
        for (uint64_t k0 = 0; k0 <= E; k0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
            const uint64_t k = k0 + threadIdx.x, g = key + k;
            const bool live = k <= E;
            uint32_t len = 0;
            if (live && a.t.flags[g]) {
                const uint64_t r = write_row_of(a.t, a.s, g);
                if (r >= a.s.U || w.stream[r] != i || w.len[r] == 0 || w.begin[r] != k * a.c.interval)
                    atomicMin(&err_s, (unsigned long long)write_fail_key(0xFFFFFFFFull, kWriteRankIndex, kReadBadIndex));
                else if (w.status[r] != kOk || w.out_len[r] < kResetHeaderBytes || w.out_len[r] > a.s.slab)
                    atomicMin(&err_s, (unsigned long long)write_fail_key(0xFFFFFFFFull, kWriteRankCompress, w.status[r] != kOk ? w.status[r] : (int32_t)kError));
                else len = write_unit_span(w.out_len[r], k < E);
            } else if (live) {  // trusted for position; what memory safety needs is checked
                const ReadCut cut = read_segment_cut(a.c.first, a.c.off, a.c.in_len, i, k);
                if (!cut.ok) atomicMin(&err_s, (unsigned long long)write_fail_key(0xFFFFFFFFull, kWriteRankIndex, kReadBadIndex));
                else len = cut.end - cut.start;
            }
            uint64_t tile;
            const uint64_t at = base + reset_tile_scan(len, wave_sum, tile);
            if (live) {
                a.t.new_pos[g] = (uint32_t)at, a.t.new_len[g] = len, a.t.owner[g] = (uint32_t)i;
                if (k < E && a.new_reset_off) a.new_reset_off[a.c.first[i] + k] = (uint32_t)(at + len);
            }
            base += tile;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint64_t err = err_s;
            const int32_t st = err != kWriteNoFail ? write_fail_code(err) : (base > a.out_cap[i] ? (int32_t)kOutputFull : (int32_t)kOk);
            a.status[i] = (int8_t)st, a.out_len[i] = st == kOk ? (uint32_t)base : 0, a.t.whole[i] = 0;
        }
        __syncthreads();  // (the next stream of this workgroup sets the word again)
    }
}

struct WriteGatherArgs {
    WriteCaller c;
    WriteTables t;
    WriteSlice s;
    uint8_t* out;  // the caller's buffer and tables
    const uint64_t* out_off;
    const uint32_t* out_cap;  // nothing is written at or behind out + out_off[i] + out_cap[i]
    const int8_t* status;
};
// One workgroup per segment of the batch, then per stream of the slice (the streams that are one copy), grid-strided.  Every byte
// of a new stream has one writer: a segment's workgroup writes [new_pos, new_pos + new_len), segment 0's the header as well.
__global__ void __launch_bounds__(256) tamp_write_gather_kernel(WriteGatherArgs a) {
    const WriteRows w = write_rows_at(a.s.region, a.s.U);
    const uint64_t items = a.t.S + (a.s.i1 - a.s.i0);
    for (uint64_t x = blockIdx.x; x < items; x += gridDim.x) {
        if (x >= a.t.S) {
            const uint64_t i = a.s.i0 + (x - a.t.S);
            if (a.t.whole[i] && a.status[i] == kOk && a.c.in_len[i] <= a.out_cap[i])
                reset_copy(a.out + a.out_off[i], a.c.in + a.c.in_off[i], a.c.in_len[i], false, 0);
            continue;
        }
        const uint64_t g = x;
        const uint32_t i = a.t.owner[g];
        if (i == kWriteNoOwner || i < a.s.i0 || i >= a.s.i1 || a.status[i] != kOk || a.t.whole[i] || !write_index_ok(a.c, i)) continue;
        const uint64_t key = a.c.first[i] + i, E = a.c.first[i + 1] - a.c.first[i];
        if (g < key || g - key > E || a.c.in_len[i] < kResetHeaderBytes) continue;
        const uint64_t k = g - key;
        const uint64_t pos = a.t.new_pos[g];
        const uint32_t len = a.t.new_len[g];
        if (pos + len > a.out_cap[i]) continue;  // (a stream that fits: never)
        uint8_t* const dst = a.out + a.out_off[i] + pos;
        if (k == 0 && threadIdx.x == 128) dst[-2] = a.c.in[a.c.in_off[i]], dst[-1] = 0;  // (pos = 2: the stream's own header)
        if (a.t.flags[g]) {
            const uint64_t r = write_row_of(a.t, a.s, g);
            if (r >= a.s.U) continue;
            const uint32_t have = w.out_len[r];
            if (have < kResetHeaderBytes || have > a.s.slab || write_unit_span(have, k < E) != len) continue;
            const uint8_t* const slab = a.s.region + w.slab_off[r];
            const uint32_t body = have - kResetHeaderBytes;
            reset_copy(dst, slab + kResetHeaderBytes, body, false, 0);
            // a closed segment ends with the next one's lead, the reset's second FLUSH: the two bytes every slab starts with
            if (k < E && threadIdx.x >= 64 && threadIdx.x < 66) dst[body + (threadIdx.x - 64)] = slab[threadIdx.x - 64];
        } else {
            const ReadCut cut = read_segment_cut(a.c.first, a.c.off, a.c.in_len, i, k);
            if (!cut.ok || cut.end - cut.start != len) continue;
            reset_copy(dst, a.c.in + a.c.in_off[i] + cut.start, len, false, 0);
        }
    }
}

}  // namespace tamp_amd
