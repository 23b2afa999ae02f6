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
//                                   of it took, clipped at out_cap[owner]; the header over the lead of each stream's segment 0
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
};
__global__ void __launch_bounds__(256) tamp_batch_reset_gather_kernel(BatchResetGatherArgs a) {
    for (uint32_t k = blockIdx.x; k < a.count; k += gridDim.x) {
        const uint32_t o = a.owner[k];
        const uint64_t c0 = a.closed_first[o], from = a.s.start[o];
        const uint64_t at = a.open ? a.s.end[o] - from : a.pos[k] - from;  // in front of it in its stream
        const bool head = a.open ? a.closed_first[o + 1] == c0 : a.first + k == c0;  // the stream's segment 0
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

}  // namespace tamp_amd
