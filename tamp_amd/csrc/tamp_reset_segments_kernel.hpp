// tamp_reset_segments_kernel.hpp -- one long buffer as a batch of dictionary-reset segments.
//
// A stream whose header has the dictionary_reset bit may hold resets (tamp_compressor_reset_dictionary,
// tamp/_c_src/tamp/compressor.c:847-881): FLUSH, FLUSH padded to 16 bits, and the window is the seeded dictionary again.  What
// lies between two resets is a stream of its own, so a buffer cut every `interval` bytes is a batch: the compress kernel writes
// segment k, opened by the 2-byte append lead (compressor.c:227-234) and closed by a FLUSH token, into slab k of the call's
// scratch, and the three small kernels here turn the slabs into the one stream the reference writes:
//   tamp_reset_rows_kernel    the segments' table rows (input cut, slab)
//   tamp_reset_scan_kernel    exclusive 64-bit scan of the segments' sizes = where each lands, the status of the call
//   tamp_reset_gather_kernel  the slabs packed back to back into the caller's buffer, the header over segment 0's lead
// Plain loads and vector stores only; no atomics: every output byte has one writer.
// A BATCH of such buffers (tamp_batch_compress_resets) runs the segments of all its streams the same way: the tamp_batch_reset_*
// kernels further down (their one atomic: a failing segment's status into its stream's word).
#pragma once
#include "tamp_common.hpp"
#include "tamp_reset_segments.hpp"
#include "tamp_reset_merge.hpp"
#include "tamp_decompress_long_kernel.hpp"

namespace tamp_amd {

constexpr uint32_t kResetScanTile = 1024;  // segments per step of the scan = threads of its one workgroup (TAMP_AMD_RESETS_SCAN_TILE)

struct ResetRowsArgs {
    uint64_t first;     // index of the slice's first segment in the call
    uint32_t count;     // segments of the slice
    uint32_t interval;  // input bytes per segment (the last one of the call: what is left)
    uint64_t total;     // input bytes of the call
    uint32_t slab;      // bytes per slab
    uint64_t* in_off;
    uint32_t* in_len;
    uint64_t* out_off;
    uint32_t* out_cap;
};
__global__ void __launch_bounds__(256) tamp_reset_rows_kernel(ResetRowsArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    a.in_off[i] = reset_segment_start(a.first + i, a.interval), a.in_len[i] = reset_segment_len(a.first + i, a.interval, a.total);
    a.out_off[i] = (uint64_t)i * a.slab, a.out_cap[i] = a.slab;
}

// What the scan carries from slice to slice, in device memory (zeroed in front of the first slice).
struct ResetCarry {
    uint64_t base;          // output bytes of the segments in front
    int32_t lowest, highest;  // of the segments' status codes so far
};

struct ResetScanArgs {
    const uint32_t* seg_len;  // the compress kernel's out_len per segment of the slice
    const int8_t* seg_status;
    uint32_t count;
    uint64_t first;       // index of the slice's first segment in the call
    uint64_t* dst_off;    // -> where each segment lands in the caller's buffer
    uint64_t* reset_off;  // optional: per reset of the call, the offset of the byte behind it (= behind the next segment's lead)
    ResetCarry* carry;
    uint32_t last;        // the call's last slice: the results below are written
    uint64_t out_cap;
    uint64_t* out_len;
    int8_t* status;
};
// One step of a scan by a workgroup of kResetScanTile threads, every one of which calls it (shuffles and two barriers): -> the sum of
// the values of the threads in front, `tile`: of all of them.
__device__ __forceinline__ uint64_t reset_tile_scan(uint64_t v, uint64_t* wave_sum /* LDS, kResetScanTile / kWave */, uint64_t& tile) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint64_t incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t o = __shfl_up(incl, d);
        if ((int)lane >= d) incl += o;
    }
    if (lane == kWave - 1) wave_sum[wave] = incl;
    __syncthreads();
    uint64_t before = 0;
    tile = 0;
    for (uint32_t w = 0; w < kResetScanTile / kWave; w++) {
        const uint64_t ws = wave_sum[w];
        before += w < wave ? ws : 0;
        tile += ws;
    }
    __syncthreads();
    return before + incl - v;
}

__global__ void __launch_bounds__(kResetScanTile) tamp_reset_scan_kernel(ResetScanArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    __shared__ int32_t wave_lo[kResetScanTile / kWave], wave_hi[kResetScanTile / kWave];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    uint64_t base = a.carry->base;
    int32_t lo = 0, hi = 0;
    for (uint32_t t0 = 0; t0 < a.count; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint32_t i = t0 + tid;
        const bool live = i < a.count;
        const uint64_t v = live ? a.seg_len[i] : 0;
        const int32_t s = live ? a.seg_status[i] : 0;
        lo = s < lo ? s : lo, hi = s > hi ? s : hi;
        uint64_t tile;
        const uint64_t at = base + reset_tile_scan(v, wave_sum, tile);
        if (live) {
            a.dst_off[i] = at;
            if (a.reset_off && a.first + i >= 1) a.reset_off[a.first + i - 1] = at + 2;
        }
        base += tile;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int32_t ol = __shfl_xor(lo, d), oh = __shfl_xor(hi, d);
        lo = ol < lo ? ol : lo, hi = oh > hi ? oh : hi;
    }
    if (lane == 0) wave_lo[wave] = lo, wave_hi[wave] = hi;
    __syncthreads();
    if (tid == 0) {
        lo = a.carry->lowest, hi = a.carry->highest;
        for (uint32_t w = 0; w < kResetScanTile / kWave; w++) {
            lo = wave_lo[w] < lo ? wave_lo[w] : lo;
            hi = wave_hi[w] > hi ? wave_hi[w] : hi;
        }
        a.carry->base = base, a.carry->lowest = lo, a.carry->highest = hi;
        if (a.last) {
            // an error of any segment is the call's (TAMP_EXCESS_BITS), then a segment that outgrew its slab or a total that
            // outgrows the caller's room (TAMP_OUTPUT_FULL); out_len = 0 for both
            const int32_t worst = lo < 0 ? lo : (hi > 0 ? hi : (base > a.out_cap ? (int32_t)kOutputFull : (int32_t)kOk));
            *a.status = (int8_t)worst;
            *a.out_len = worst == kOk ? base : 0;
        }
    }
}

// 4 bytes at any address (gfx950 serves misaligned global dword loads in hardware; the compiler emits them for align-1 types).
struct __attribute__((packed, aligned(1))) GlobalU32 { uint32_t v; };

struct ResetGatherArgs {
    const uint8_t* src;     // slab k of the slice at src + k * slab
    uint32_t slab;
    uint32_t count;
    const uint32_t* seg_len;
    const uint64_t* dst_off;
    uint8_t* dst;
    uint64_t dst_cap;       // nothing is written at or behind dst + dst_cap
    uint32_t head_segment;  // segment 0 of the slice is segment 0 of the call: `header` replaces its two lead bytes
    uint32_t header;        // byte 0 in bits 0-7, byte 1 in bits 8-15
};
// `len` bytes from src to dst by one workgroup: the destination is written as aligned dwords strictly inside [dst, dst + len) and the
// up-to-three bytes in front of and behind them as bytes, the source read as unaligned dwords.  `patch`: `header` (byte 0 in bits
// 0-7, byte 1 in bits 8-15) takes the place of the first two bytes.
__device__ __forceinline__ void reset_copy(uint8_t* dst, const uint8_t* src, uint32_t len, bool patch, uint32_t header) {
    const uint32_t head = min((uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3), len);
    const uint32_t ndw = (len - head) >> 2, tail0 = head + 4 * ndw;
    for (uint32_t j = threadIdx.x; j < ndw; j += blockDim.x) {
        const uint32_t i0 = head + 4 * j;
        uint32_t v = reinterpret_cast<const GlobalU32*>(src + i0)->v;
        if (patch && i0 < 2) {  // (the dword that holds a lead byte: at most the first one)
            if (i0 == 0) v = (v & 0xFFFF0000u) | header;
            else v = (v & 0xFFFFFF00u) | (header >> 8);
        }
        *reinterpret_cast<uint32_t*>(dst + i0) = v;
    }
    if (threadIdx.x < 6) {  // the bytes in front of the first aligned dword and behind the last one
        const uint32_t i = threadIdx.x < 3 ? threadIdx.x : tail0 + (threadIdx.x - 3);
        const bool mine = threadIdx.x < 3 ? i < head : i < len;
        if (mine) dst[i] = (patch && i < 2) ? (uint8_t)(header >> (8 * i)) : src[i];
    }
}

// One workgroup per segment, grid-strided: neighbouring workgroups never touch the same dword.
__global__ void __launch_bounds__(256) tamp_reset_gather_kernel(ResetGatherArgs a) {
    for (uint32_t k = blockIdx.x; k < a.count; k += gridDim.x) {
        const uint64_t at = a.dst_off[k];
        if (at >= a.dst_cap) continue;
        const uint64_t room = a.dst_cap - at;
        const uint32_t len = a.seg_len[k] < room ? a.seg_len[k] : (uint32_t)room;
        reset_copy(a.dst + at, a.src + (size_t)k * a.slab, len, a.head_segment && k == 0, a.header);
    }
}

// ---- a BATCH of buffers, each one cut into segments (tamp_batch_compress_resets; the index arithmetic: tamp_reset_segments.hpp) ----
//
// The compress launch takes one way of closing its streams, so the segments of all streams form two dense tables: the CLOSED ones
// (FLUSH token, a reset behind them; S - n of them, in stream order) and the OPEN ones (each stream's last; one per stream).  The
// call walks the closed table in slices, then the open one:
//   tamp_batch_reset_count_kernel   closed segments per stream, their exclusive scan (closed_first[0 .. n], the last entry S - n)
//   tamp_batch_reset_rows_kernel    a lane per segment of the slice: its owner (binary search), input cut and slab
//   tamp_batch_reset_place_kernel   closed slices: the running scan of the segments' sizes; per stream where its first closed
//                                   segment starts and its last one ends in that scan, and the worst status
//   tamp_batch_reset_finish_kernel  open slices: out_len and status of every stream
//   tamp_batch_reset_gather_kernel  a workgroup per segment: its slab to out + out_off[owner] + what the stream's segments in front
//                                   of it took, clipped at out_cap[owner]; the header over the lead of each stream's segment 0;
//                                   on request the RESET INDEX (tamp_batch_compress_resets_index): one store per closed segment
// A device-memory call reads ONE 16-byte record back, once: closed_first[n] and the longest stream behind it, which size the slices,
// the slabs and the scratch -- from the tables themselves, never from the caller's max_in_len hint.

struct BatchResetCountArgs {
    const uint32_t* in_len;
    uint64_t n;
    uint32_t interval;
    uint64_t* closed_first;  // n + 1 entries, and behind them the batch's longest stream: the record a device-memory call reads back
};
__global__ void __launch_bounds__(kResetScanTile) tamp_batch_reset_count_kernel(BatchResetCountArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    __shared__ uint32_t wave_max[kResetScanTile / kWave];
    uint64_t base = 0;
    uint32_t longest = 0;
    for (uint64_t t0 = 0; t0 < a.n; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint64_t i = t0 + threadIdx.x;
        const bool live = i < a.n;
        const uint32_t len = live ? a.in_len[i] : 0;
        const uint64_t v = live ? batch_reset_closed_count(len, a.interval) : 0;
        longest = len > longest ? len : longest;
        uint64_t tile;
        const uint64_t at = base + reset_tile_scan(v, wave_sum, tile);
        if (live) a.closed_first[i] = at;
        base += tile;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(longest, d);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) wave_max[threadIdx.x / kWave] = longest;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 0; w < kResetScanTile / kWave; w++) longest = wave_max[w] > longest ? wave_max[w] : longest;
        a.closed_first[a.n] = base, a.closed_first[a.n + 1] = longest;
    }
}

struct BatchResetRowsArgs {
    const uint64_t* closed_first;
    const uint64_t* in_off;  // the caller's tables
    const uint32_t* in_len;
    uint64_t n;
    uint64_t first;     // the slice's first closed segment / first stream
    uint32_t count;     // rows of the slice
    uint32_t open;      // the slice holds open segments: row r is stream first + r
    uint32_t interval;
    uint32_t slab;
    uint64_t* seg_in_off;  // -> the slice's table
    uint32_t* seg_in_len;
    uint64_t* seg_out_off;
    uint32_t* seg_cap;
    uint32_t* owner;
};
__global__ void __launch_bounds__(256) tamp_batch_reset_rows_kernel(BatchResetRowsArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.count) return;
    const BatchResetRow row = a.open ? batch_reset_open_row(a.closed_first, a.first + r, a.in_len[a.first + r], a.interval)
                                     : batch_reset_closed_row(a.closed_first, a.n, a.first + r, a.interval);
    a.seg_in_off[r] = a.in_off[row.stream] + row.start, a.seg_in_len[r] = row.len;
    a.seg_out_off[r] = (uint64_t)r * a.slab, a.seg_cap[r] = a.slab;
    a.owner[r] = (uint32_t)row.stream;
}

// Per stream, zeroed in front of the first slice.
struct BatchResetStreams {
    uint64_t* start;   // where the stream's first closed segment starts in the scan of all closed segments
    uint64_t* end;     // where its last one ends (end - start: the bytes in front of its open segment)
    int32_t* lowest;   // of its closed segments' status codes
    int32_t* highest;
};

struct BatchResetPlaceArgs {
    const uint32_t* seg_len;  // the compress kernel's out_len per closed segment of the slice
    const int8_t* seg_status;
    const uint32_t* owner;
    uint32_t count;
    uint64_t first;  // the slice's first closed segment
    const uint64_t* closed_first;
    uint64_t* pos;   // -> per segment: where it starts in the scan
    BatchResetStreams s;
    ResetCarry* carry;  // (base only)
};
__global__ void __launch_bounds__(kResetScanTile) tamp_batch_reset_place_kernel(BatchResetPlaceArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    uint64_t base = a.carry->base;
    for (uint32_t t0 = 0; t0 < a.count; t0 += kResetScanTile) {  // (uniform bounds)
        const uint32_t i = t0 + threadIdx.x;
        const bool live = i < a.count;
        const uint64_t v = live ? a.seg_len[i] : 0;
        uint64_t tile;
        const uint64_t at = base + reset_tile_scan(v, wave_sum, tile);
        if (live) {
            const uint32_t o = a.owner[i];
            const uint64_t c = a.first + i;
            a.pos[i] = at;
            if (c == a.closed_first[o]) a.s.start[o] = at;
            if (c + 1 == a.closed_first[o + 1]) a.s.end[o] = at + v;
            const int32_t st = a.seg_status[i];  // (errors are rare: the atomics run for them alone)
            if (st < 0) atomicMin(&a.s.lowest[o], st);
            if (st > 0) atomicMax(&a.s.highest[o], st);
        }
        base += tile;
    }
    if (threadIdx.x == 0) a.carry->base = base;
}

struct BatchResetFinishArgs {
    const uint32_t* seg_len;  // per open segment of the slice
    const int8_t* seg_status;
    uint32_t count;
    uint64_t first;  // the slice's first stream
    BatchResetStreams s;
    const uint32_t* out_cap;  // the caller's tables
    uint32_t* out_len;
    int8_t* status;
};
__global__ void __launch_bounds__(256) tamp_batch_reset_finish_kernel(BatchResetFinishArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.count) return;
    const uint64_t i = a.first + r;
    const int32_t st = a.seg_status[r];
    const int32_t lo = min(a.s.lowest[i], st), hi = max(a.s.highest[i], st);
    const uint64_t total = a.s.end[i] - a.s.start[i] + a.seg_len[r];
    // an error of any segment is the stream's (TAMP_EXCESS_BITS), then a segment that outgrew its slab or a total that outgrows the
    // stream's room (TAMP_OUTPUT_FULL); out_len = 0 for both
    const int32_t worst = lo < 0 ? lo : (hi > 0 ? hi : (total > a.out_cap[i] ? (int32_t)kOutputFull : (int32_t)kOk));
    a.status[i] = (int8_t)worst;
    a.out_len[i] = worst == kOk ? (uint32_t)total : 0;
}

struct BatchResetGatherArgs {
    const uint8_t* src;  // slab k of the slice at src + k * slab
    uint32_t slab;
    uint32_t count;
    uint32_t open;
    uint64_t first;      // the slice's first closed segment (closed slices)
    const uint32_t* seg_len;
    const uint32_t* owner;
    const uint64_t* pos;  // closed slices
    const uint64_t* closed_first;
    BatchResetStreams s;
    uint8_t* dst;             // the caller's buffer and tables
    const uint64_t* out_off;
    const uint32_t* out_cap;  // nothing is written at or behind dst + out_off[i] + out_cap[i]
    uint32_t header;          // byte 0 in bits 0-7, byte 1 in bits 8-15
    uint32_t* reset_off;      // optional, closed slices: the reset index -- entry c for closed segment c of the batch (the streams'
                              // entries stand in stream order, stream i's from closed_first[i] on)
};
__global__ void __launch_bounds__(256) tamp_batch_reset_gather_kernel(BatchResetGatherArgs a) {
    for (uint32_t k = blockIdx.x; k < a.count; k += gridDim.x) {
        const uint32_t o = a.owner[k];
        const uint64_t c0 = a.closed_first[o], from = a.s.start[o];
        const uint64_t at = a.open ? a.s.end[o] - from : a.pos[k] - from;  // in front of it in its stream
        const bool head = a.open ? a.closed_first[o + 1] == c0 : a.first + k == c0;  // the stream's segment 0
        // the byte behind this segment's reset, in its stream: behind the next segment's lead (the reset's last 16 bits).  Of a
        // stream that fails the value means nothing.
        if (!a.open && a.reset_off && threadIdx.x == 0) a.reset_off[a.first + k] = (uint32_t)(at + a.seg_len[k] + 2);
        const uint64_t cap = a.out_cap[o];
        if (at >= cap) continue;
        const uint64_t room = cap - at;
        const uint32_t have = a.seg_len[k] < a.slab ? a.seg_len[k] : a.slab;  // (never read behind the slab)
        const uint32_t len = have < room ? have : (uint32_t)room;
        reset_copy(a.dst + a.out_off[o] + at, a.src + (size_t)k * a.slab, len, head, a.header);
    }
}

// ---- reading such a stream back: where its resets are, and its segments staged as streams of their own ----

// A lane per chunk of the compressed bits walks the tokens that start in the chunk from its settled start (the long-stream decoder's
// front: tamp_long_sync_kernel) and reports what tamp_reset_merge.hpp needs.
struct ResetFindArgs {
    LongArgs a;  // in, n, n_chunks, chunk_bits, wbits, lbits, extended, g
    ResetChunkReport* rep;
};
__global__ void __launch_bounds__(64) tamp_reset_find_kernel(ResetFindArgs x) {
    __shared__ uint8_t lut[128];
    build_prefix_lut(lut);
    __syncthreads();
    const LongArgs& a = x.a;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_chunks) return;
    const uint32_t minp = (uint32_t)min_pattern_size((int)a.wbits, (int)a.lbits);
    const uint32_t end = (i + 1) * a.chunk_bits;
    ResetChunkReport r = {};
    uint32_t t = a.g[i], nt = 0;
    bool prev_flush = false, bad = false;
    while (t != kLongEnd && t < end) {
        uint32_t rec;
        const uint32_t k = long_token(a.in, a.n, t, lut, a.wbits, a.lbits, minp, a.extended != 0, rec, bad);
        if (!k) break;
        t += k;
        const bool flush = rec == 0xFFFFFFFFu;
        if (nt == 0) {
            r.first_end = t >> 3;
            if (flush) r.flags |= kResetChunkFirstFlush;
        } else if (flush && prev_flush) {
            if (r.n_inner < kResetChunkInner) r.inner[r.n_inner] = t >> 3;
            r.n_inner++;
        }
        prev_flush = flush, nt++;
    }
    if (nt) r.flags |= kResetChunkHasTokens | (prev_flush ? kResetChunkLastFlush : 0u);
    x.rep[i] = r;
}

// Segment k of the stream, the stream's two header bytes in front of it, at stage + dst_off[k]: a stream that decodes on its own.
struct ResetStageArgs {
    const uint8_t* in;        // the stream
    const uint32_t* src_off;  // per segment: where it starts in the stream, its bytes
    const uint32_t* src_len;
    const uint64_t* dst_off;  // where its staged stream starts (src_len + 2 bytes)
    uint8_t* stage;
    uint32_t count;
    uint32_t header;          // byte 0 in bits 0-7, byte 1 in bits 8-15
};
__global__ void __launch_bounds__(256) tamp_reset_stage_kernel(ResetStageArgs a) {
    for (uint32_t k = blockIdx.x; k < a.count; k += gridDim.x) {
        uint8_t* const dst = a.stage + a.dst_off[k];
        if (threadIdx.x == 64) dst[0] = (uint8_t)a.header, dst[1] = (uint8_t)(a.header >> 8);
        reset_copy(dst + 2, a.in + a.src_off[k], a.src_len[k], false, 0);
    }
}

// ---- reading a BATCH back with the compressor's reset index (tamp_batch_decompress_resets; the rows: tamp_reset_segments.hpp) ----
//
// The index is a hint, checked here: a stream all of whose claimed segments hold up is SPLIT into units, every other one stays one
// WHOLE unit for the exact decoders.  R = C + n rows (C closed segments, n open ones).  No workgroup waits for another: the steps
// are kernels of their own on the call's stream.
//   tamp_batch_reset_bound_kernel   C and an upper bound of the staged bytes: the 16-byte record a device-memory call reads back
//   tamp_batch_reset_check_kernel   a lane per row: range and order of its entries, then the WALK of its segment, token by token
//                                   (long_token): decoded size, ends at its boundary, last two tokens FLUSH, no offset out of window
//   tamp_batch_reset_sizes_kernel   exclusive scans over the closed rows: decoded sizes, rows that failed
//   tamp_batch_reset_plan_kernel    a lane per stream: split or whole, its size; the scan that places the split streams in the stage
//   tamp_batch_reset_units_kernel   a lane per row: the unit's table row (a row of a whole stream: an empty stream)
//   tamp_batch_reset_stage_kernel   a workgroup per unit: header + segment into the stage (reset_copy)
//   tamp_batch_reset_done_kernel    per split stream out_len / status / in_consumed, then per unit: decoded to the walk's size?

// What a stream must look like to be split: the reset bit (with it the second header byte, which must be zero), no custom
// dictionary, a window the call accepts, a length the 32-bit bit positions of the walk can count.
__device__ __forceinline__ bool reset_split_header(const uint8_t* s, uint32_t len, uint32_t max_wbits) {
    if (len < kResetHeaderBytes || len > kMaxDecodeIn - 512 || max_wbits > 15) return false;
    const uint32_t h0 = s[0];
    const StreamHeader hd = decode_header(h0);
    return hd.dreset && !hd.custom && s[1] == 0 && hd.wbits <= max_wbits;
}

struct BatchResetRecord {  // in device memory; a device-memory call reads the first two words back
    uint64_t closed;        // C = reset_first[n]
    uint64_t staged_bound;  // no verdict can stage more bytes than this
    uint64_t split, units, staged;  // the plan: streams split, their units, the bytes staged (TAMP_AMD_RESETS_DEBUG reads these)
};

struct BatchResetBoundArgs {
    const uint64_t* first;
    const uint32_t* in_len;
    uint64_t n;
    BatchResetRecord* rec;
};
__global__ void __launch_bounds__(kResetScanTile) tamp_batch_reset_bound_kernel(BatchResetBoundArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    uint64_t bound = 0, disorder = 0;
    for (uint64_t t0 = 0; t0 < a.n; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint64_t i = t0 + threadIdx.x;
        const uint64_t E = i < a.n ? reset_index_entries(a.first, a.n, i) : 0;
        uint64_t tile;
        (void)reset_tile_scan(E ? (uint64_t)a.in_len[i] + kResetHeaderBytes * (E + 1) : 0, wave_sum, tile);
        bound += tile;
        (void)reset_tile_scan(i < a.n && !reset_first_in_order(a.first, i) ? 1 : 0, wave_sum, tile);
        disorder += tile;
    }
    // (a table that is no running sum from 0 gives no row one owner: the call then has no index at all)
    if (threadIdx.x == 0) a.rec->closed = disorder ? 0 : a.first[a.n], a.rec->staged_bound = bound;
}

struct BatchResetCheckArgs {
    const uint8_t* in;  // the caller's tables
    const uint64_t* in_off;
    const uint32_t* in_len;
    const uint64_t* first;
    const uint32_t* off;
    uint64_t n, closed;
    uint32_t max_wbits;
    uint32_t* size;   // -> per row: bytes the segment decodes to
    uint8_t* failed;  // -> per row: 0 = the segment holds up
};
__global__ void __launch_bounds__(64) tamp_batch_reset_check_kernel(BatchResetCheckArgs a) {
    __shared__ uint8_t lut[128];
    build_prefix_lut(lut);
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.closed + a.n) return;
    const bool open = r >= a.closed;
    const ResetIndexCut u = open ? reset_index_open_cut(a.first, a.off, a.in_len, a.n, r - a.closed)
                                 : reset_index_closed_cut(a.first, a.off, a.in_len, a.n, r);
    uint64_t bytes = 0;
    bool ok = u.stream != kResetNoOwner;
    if (ok) {
        const uint8_t* const s = a.in + a.in_off[u.stream];
        ok = reset_split_header(s, a.in_len[u.stream], a.max_wbits);
        if (ok) {
            const StreamHeader hd = decode_header(s[0]);
            // the walk: token aligned at u.start by induction from the header, and never a bit read at or behind u.end.  The
            // reference keeps "the last token was a FLUSH" across a reset, so segments behind one start with it set
            const uint32_t end = 8 * u.end;
            uint32_t t = 8 * u.start;
            bool last = u.seg != 0, before = last, bad = false;
            while (t < end) {  // (long_token: at least one bit, or 0)
                uint32_t rec;
                const uint32_t k = long_token(s, u.end, t, lut, hd.wbits, hd.lbits, hd.minp, hd.extended, rec, bad);
                if (!k) break;
                t += k;
                before = last, last = rec == 0xFFFFFFFFu;
                if (!last) bytes += (rec >> 2) & 0xFFu;
            }
            // a closed segment ends exactly at its boundary behind FLUSH, FLUSH; the open one ends as a stream ends: out of tokens
            ok = !bad && bytes <= 0xFFFFFFFFull && (open || (t == end && last && before));
        }
    }
    a.size[r] = ok ? (uint32_t)bytes : 0, a.failed[r] = ok ? 0 : 1;
}

struct BatchResetSizesArgs {
    const uint32_t* size;  // per closed row
    const uint8_t* failed;
    uint64_t closed;
    uint64_t* size_scan;  // -> closed + 1 entries each
    uint64_t* fail_scan;
};
__global__ void __launch_bounds__(kResetScanTile) tamp_batch_reset_sizes_kernel(BatchResetSizesArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    uint64_t bytes = 0, fails = 0;
    for (uint64_t t0 = 0; t0 < a.closed; t0 += kResetScanTile) {  // (uniform bounds)
        const uint64_t c = t0 + threadIdx.x;
        const bool live = c < a.closed;
        uint64_t tile;
        const uint64_t at = bytes + reset_tile_scan(live ? a.size[c] : 0, wave_sum, tile);
        bytes += tile;
        const uint64_t fat = fails + reset_tile_scan(live ? a.failed[c] : 0, wave_sum, tile);
        fails += tile;
        if (live) a.size_scan[c] = at, a.fail_scan[c] = fat;
    }
    if (threadIdx.x == 0) a.size_scan[a.closed] = bytes, a.fail_scan[a.closed] = fails;
}

struct BatchResetPlanArgs {
    const uint8_t* in;  // the caller's tables
    const uint64_t* in_off;
    const uint32_t* in_len;
    const uint32_t* out_cap;
    const uint64_t* first;
    uint64_t n, closed;
    uint32_t max_wbits;
    const uint32_t* size;  // per row
    const uint8_t* failed;
    const uint64_t* size_scan;
    const uint64_t* fail_scan;
    uint64_t budget;       // bytes of the stage: streams are split in stream order until it is full
    uint8_t* split;        // -> per stream
    uint64_t* stage_base;  // -> per split stream: its first staged byte
    uint32_t* total;       // -> per split stream: its decoded size
    uint32_t* whole_len;   // -> per stream: in_len of a whole stream, 0 for a split one (the exact decoders' table)
    BatchResetRecord* rec;
};
__global__ void __launch_bounds__(kResetScanTile) tamp_batch_reset_plan_kernel(BatchResetPlanArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    uint64_t wanted = 0, staged = 0, n_split = 0, units = 0;
    for (uint64_t t0 = 0; t0 < a.n; t0 += kResetScanTile) {  // (uniform bounds)
        const uint64_t i = t0 + threadIdx.x;
        const bool live = i < a.n;
        const uint64_t E = live ? reset_index_entries(a.first, a.n, i) : 0;
        bool ok = E != 0 && !a.failed[a.closed + i] && a.fail_scan[a.first[i + 1]] == a.fail_scan[a.first[i]];
        uint64_t bytes = 0;
        if (ok) {
            // (room that is used up exactly is the exact decoder's to judge)
            bytes = a.size_scan[a.first[i + 1]] - a.size_scan[a.first[i]] + a.size[a.closed + i];
            ok = bytes < a.out_cap[i] && reset_split_header(a.in + a.in_off[i], a.in_len[i], a.max_wbits);
        }
        const uint64_t want = ok ? reset_staged_bytes(a.in_len[i], E) : 0;
        uint64_t tile;
        const uint64_t at = wanted + reset_tile_scan(want, wave_sum, tile);
        wanted += tile;
        ok = ok && at + want <= a.budget;  // (the sums only grow: behind the first stream that does not fit none fits)
        if (ok) staged += want, n_split += 1, units += E + 1;  // (this lane's own streams; summed behind the loop)
        if (live) {
            a.split[i] = ok ? 1 : 0, a.stage_base[i] = at, a.total[i] = (uint32_t)bytes;
            a.whole_len[i] = ok ? 0 : a.in_len[i];
        }
    }
    uint64_t all_staged, all_split, all_units;
    (void)reset_tile_scan(staged, wave_sum, all_staged);
    (void)reset_tile_scan(n_split, wave_sum, all_split);
    (void)reset_tile_scan(units, wave_sum, all_units);
    if (threadIdx.x == 0) a.rec->split = all_split, a.rec->units = all_units, a.rec->staged = all_staged;
}

// The units' table, one row per claimed segment; a row whose stream stays whole is an empty stream (no input, no room).
struct BatchResetUnits {
    uint64_t* in_off;   // where the unit's staged stream starts in the stage
    uint64_t* out_off;  // where it decodes to in the caller's buffer
    uint64_t* src_off;  // where its segment starts in the caller's input
    uint32_t* in_len;   // segment + header bytes (0: no unit)
    uint32_t* out_cap;  // exactly its decoded size
    uint32_t* out_len;  // <- the decode
    uint32_t* owner;    // kResetNoOwner: no unit
    int8_t* status;     // <- the decode
};
struct BatchResetUnitsArgs {
    const uint64_t* in_off;  // the caller's tables
    const uint32_t* in_len;
    const uint64_t* out_off;  // (null: sizes only, no units)
    const uint64_t* first;
    const uint32_t* off;
    uint64_t n, closed;
    const uint32_t* size;
    const uint64_t* size_scan;
    const uint8_t* split;
    const uint64_t* stage_base;
    BatchResetUnits u;
};
__global__ void __launch_bounds__(256) tamp_batch_reset_units_kernel(BatchResetUnitsArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.closed + a.n) return;
    ResetIndexCut u = r >= a.closed ? reset_index_open_cut(a.first, a.off, a.in_len, a.n, r - a.closed)
                                    : reset_index_closed_cut(a.first, a.off, a.in_len, a.n, r);
    if (u.stream != kResetNoOwner && !a.split[u.stream]) u.stream = kResetNoOwner;
    const bool unit = u.stream != kResetNoOwner;
    a.u.owner[r] = u.stream;
    a.u.in_off[r] = unit ? reset_unit_stage_off(a.stage_base[u.stream], u) : 0;
    a.u.in_len[r] = unit ? u.end - u.start + kResetHeaderBytes : 0;
    a.u.src_off[r] = unit ? a.in_off[u.stream] + u.start : 0;
    a.u.out_off[r] = unit ? a.out_off[u.stream] + reset_unit_out_off(a.first, a.size_scan, u) : 0;
    a.u.out_cap[r] = unit ? a.size[r] : 0;
}

struct BatchResetStageArgs {
    const uint8_t* in;  // the caller's input
    const uint64_t* in_off;
    BatchResetUnits u;
    uint8_t* stage;
    uint64_t rows;
};
__global__ void __launch_bounds__(256) tamp_batch_reset_stage_kernel(BatchResetStageArgs a) {
    for (uint64_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const uint32_t o = a.u.owner[r];
        if (o == kResetNoOwner) continue;
        uint8_t* const dst = a.stage + a.u.in_off[r];
        // (the stream's own two header bytes: the second one is zero)
        if (threadIdx.x == 64) dst[0] = a.in[a.in_off[o]], dst[1] = 0;
        reset_copy(dst + kResetHeaderBytes, a.in + a.u.src_off[r], a.u.in_len[r] - kResetHeaderBytes, false, 0);
    }
}

struct BatchResetDoneArgs {
    const uint32_t* in_len;  // the caller's tables
    uint32_t* out_len;
    int8_t* status;
    uint32_t* in_consumed;  // may be null
    uint64_t n, closed;
    const uint8_t* split;
    const uint32_t* total;
    BatchResetUnits u;  // (u.owner null: sizes only, no units were decoded)
    uint32_t units;     // 0: the split streams' results; 1: the units against the walk
};
// Launched twice, one behind the other: a unit that did not decode to the size the walk found makes its stream TAMP_ERROR -- the two
// disagree, which is a defect of the library and not a property of the stream (several units may store that same value).
__global__ void __launch_bounds__(256) tamp_batch_reset_done_kernel(BatchResetDoneArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!a.units) {
        if (r >= a.n || !a.split[r]) return;
        a.out_len[r] = a.total[r], a.status[r] = (int8_t)kInputExhausted;
        if (a.in_consumed) a.in_consumed[r] = a.in_len[r];
        return;
    }
    if (r >= a.closed + a.n) return;
    const uint32_t o = a.u.owner[r];
    if (o == kResetNoOwner) return;
    const int8_t st = a.u.status[r];
    if (a.u.out_len[r] != a.u.out_cap[r] || (st != (int8_t)kInputExhausted && st != (int8_t)kOutputFull)) a.status[o] = (int8_t)kError;
}

}  // namespace tamp_amd
