// tamp_reset_index_kernel.hpp -- the reset index of a batch of streams, found on the device (tamp_batch_index_resets, DESIGN.md 3.13;
// the arithmetic: tamp_reset_index.hpp).  A reset is a FLUSH token whose predecessor is a FLUSH (decompressor.c:501-513), and where
// tokens lie follows from the grammar alone, so the units of work are the chunks of kIndexChunkBits compressed bits of ALL streams,
// numbered through the batch.  Every step is a launch of its own on the call's stream; no workgroup waits for another:
//   tamp_index_chunks_kernel   per stream its status so far and its chunks; their exclusive scan (chunk_first) and the longest stream
//   tamp_index_sync_kernel     tamp_long_sync_kernel's rule, a lane per chunk of the batch: rounds until no start moved
//   tamp_index_find_kernel     a lane per chunk walks its tokens: the report (count pass) or the entries themselves (write pass)
//   tamp_index_merge_kernel    the scan over the chunks' reports in three launches (per tile, over the tiles, per chunk): every chunk's
//                              base in the entry table, whether a FLUSH comes in, the running sum of decoded bytes
//   tamp_index_streams_kernel  a lane per stream: reset_first, status, open_size
//   tamp_index_sizes_kernel    a lane per entry: closed_size from the running counts
// Plain loads and vector stores only; no atomics (several lanes may store the same 1 into a flag).
#pragma once
#include "tamp_common.hpp"
#include "tamp_reset_index.hpp"
#include "tamp_reset_segments_kernel.hpp"

namespace tamp_amd {

static_assert(kIndexMaxStream == kMaxDecodeIn - 512, "the walk's 32-bit bit positions");
static_assert(kIndexHasTokens == kResetChunkHasTokens && kIndexFirstFlush == kResetChunkFirstFlush && kIndexLastFlush == kResetChunkLastFlush,
              "one meaning of the report's flags");

struct IndexCaller {  // the caller's tables
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    uint64_t n;
    uint32_t max_wbits;
};
struct IndexRecord {  // in device memory; the host reads it back
    uint64_t chunks, longest;  // of the batch; of its longest stream
    uint64_t entries;
    uint32_t moved, reserved;  // sync: a start changed in this round
};
struct IndexStreams {  // per stream, the call's scratch
    uint64_t* chunk_first;  // n + 1: the stream's first chunk in the order of the batch
    int8_t* pre;            // the status its first bytes decide (kIndexOk: it has chunks)
    uint8_t* bad;           // an offset out of the window was seen
    IndexRecord* rec;
};

struct IndexChunksArgs {
    IndexCaller c;
    IndexStreams s;
};
__global__ void __launch_bounds__(kResetScanTile) tamp_index_chunks_kernel(IndexChunksArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    __shared__ uint32_t wave_max[kResetScanTile / kWave];
    uint64_t base = 0;
    uint32_t longest = 0;
    for (uint64_t t0 = 0; t0 < a.c.n; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint64_t i = t0 + threadIdx.x;
        const bool live = i < a.c.n;
        IndexStreamPlan p = {kIndexOk, 0, 0};
        if (live) p = index_stream_plan(a.c.in + a.c.in_off[i], a.c.in_len[i], a.c.max_wbits);
        longest = p.chunks > longest ? p.chunks : longest;
        uint64_t tile;
        const uint64_t at = base + reset_tile_scan(p.chunks, wave_sum, tile);
        if (live) a.s.chunk_first[i] = at, a.s.pre[i] = (int8_t)p.status, a.s.bad[i] = 0;
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
        a.s.chunk_first[a.c.n] = base;
        a.s.rec->chunks = base, a.s.rec->longest = longest, a.s.rec->entries = 0, a.s.rec->moved = 0;
    }
}

// A lane's chunk: its stream, where it stands in it, the header's fields.
struct IndexLane {
    const uint8_t* s;
    uint32_t owner, len, k, first_bit, end;
    bool last;  // the stream's last chunk: nothing travels on from it
    StreamHeader hd;
};
__device__ __forceinline__ IndexLane index_lane(const IndexCaller& c, const uint64_t* chunk_first, uint64_t chunk) {
    IndexLane l;
    const uint64_t o = batch_reset_owner(chunk_first, c.n, chunk);
    l.owner = (uint32_t)o, l.s = c.in + c.in_off[o], l.len = c.in_len[o];
    l.k = (uint32_t)(chunk - chunk_first[o]), l.last = chunk + 1 == chunk_first[o + 1];
    const uint32_t h0 = l.s[0];
    l.hd = decode_header(h0), l.first_bit = 8 * (1 + (h0 & 1u)), l.end = (l.k + 1) * kIndexChunkBits;
    return l;
}

struct IndexChunkArgs {
    IndexCaller c;
    IndexStreams s;
    uint32_t chunks;
    uint32_t round0;       // sync: the first round starts from the guesses (the chunks' own first bits), g is not read
    const uint32_t* g;     // chunks + 1 start positions, bits from the stream's first
    uint32_t* g_next;      // sync: the next round's
    IndexChunkReport* rep;  // find, count pass (write = 0)
    uint32_t write;         // find: 1 = the write pass
    const uint64_t* place;  // ... the chunks' places (index_chunk_place) and running byte counts
    const uint64_t* bytes;
    uint32_t* reset_off;    // ... the caller's table
    uint64_t* count;        // ... per entry the running byte count there (null: no closed_size asked for)
};

// tamp_long_sync_kernel with a lane per chunk of the whole batch.  Chunk 0 of every stream starts behind its own header whatever the
// slot in front of it says, and a stream's last chunk hands nothing on: a start never travels from one stream into the next.
__global__ void __launch_bounds__(64) tamp_index_sync_kernel(IndexChunkArgs a) {
    __shared__ uint8_t lut[128];
    __shared__ uint32_t gs[65];
    __shared__ uint32_t moved;
    build_prefix_lut(lut);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < a.chunks;
    IndexLane l = {};
    if (live) l = index_lane(a.c, a.s.chunk_first, i);
    const bool hands_on = live && !l.last;
    const uint32_t next_before = hands_on ? (a.round0 ? l.end : a.g[i + 1]) : kLongEnd;  // the start of chunk i + 1 as the round found it
    // (slot j + 1 behind a stream's last chunk is written by nobody and read by nobody: the next stream's chunk 0 keeps its own)
    if (live) gs[threadIdx.x] = l.k == 0 ? l.first_bit : (a.round0 ? l.k * kIndexChunkBits : a.g[i]);
    if (threadIdx.x == 63) gs[64] = next_before;
    __syncthreads();
    uint32_t seen = 0xFFFFFFFEu, t = 0;  // the start this lane parsed from last time, and where that parse left the chunk
    for (uint32_t inner = 0; inner < 64; inner++) {
        if (threadIdx.x == 0) moved = 0;
        __syncthreads();
        const uint32_t from = live ? gs[threadIdx.x] : kLongEnd;
        if (live && from != seen) {
            seen = from, t = from;
            while (t != kLongEnd && t < l.end) {
                uint32_t rec;
                bool bad = false;
                const uint32_t k = long_token(l.s, l.len, t, lut, l.hd.wbits, l.hd.lbits, l.hd.minp, l.hd.extended, rec, bad);
                t = k ? t + k : kLongEnd;
            }
        }
        __syncthreads();
        if (hands_on && gs[threadIdx.x + 1] != t) {
            gs[threadIdx.x + 1] = t;
            moved = 1;
        }
        __syncthreads();
        if (!moved) break;
    }
    if (live) {
        if (l.k == 0) a.g_next[i] = l.first_bit;  // (every other start is written by the chunk in front of it, possibly in another workgroup)
        if (hands_on) {
            a.g_next[i + 1] = gs[threadIdx.x + 1];
            if (gs[threadIdx.x + 1] != next_before) a.s.rec->moved = 1;
        }
    }
}

// The tokens that START in the chunk, from its settled start.  Count pass: the report.  Write pass: at the chunk's base in the entry
// table every reset's offset in its stream and the running decoded byte count there.  A stream without the reset bit cannot hold
// resets: its FLUSH tokens count as plain ones.
__global__ void __launch_bounds__(64) tamp_index_find_kernel(IndexChunkArgs a) {
    __shared__ uint8_t lut[128];
    build_prefix_lut(lut);
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.chunks) return;
    const IndexLane l = index_lane(a.c, a.s.chunk_first, i);
    uint64_t at = 0, run = 0;
    bool prev = false;  // the token in front is a FLUSH: known to the write pass alone for the chunk's first token
    if (a.write) at = index_place_base(a.place[i]), prev = index_place_flush_in(a.place[i]), run = a.bytes[i];
    uint32_t t = l.k == 0 ? l.first_bit : a.g[i], nt = 0, inner = 0, bytes = 0, first_end = 0;
    bool first_flush = false, bad = false;
    while (t != kLongEnd && t < l.end) {
        uint32_t rec;
        const uint32_t k = long_token(l.s, l.len, t, lut, l.hd.wbits, l.hd.lbits, l.hd.minp, l.hd.extended, rec, bad);
        if (!k) break;
        t += k;
        const bool flush = rec == 0xFFFFFFFFu && l.hd.dreset;
        if (nt == 0) first_end = t >> 3, first_flush = flush;
        if (flush && prev) {
            if (a.write) {
                a.reset_off[at] = t >> 3;
                if (a.count) a.count[at] = run + bytes;
                at++;
            } else {
                inner++;
            }
        }
        if (rec != 0xFFFFFFFFu) bytes += (rec >> 2) & 0xFFu;
        prev = flush, nt++;
    }
    if (a.write) return;
    IndexChunkReport r;
    r.flags = (nt ? kIndexHasTokens : 0u) | (first_flush ? kIndexFirstFlush : 0u) | (nt && prev ? kIndexLastFlush : 0u) | (l.k == 0 ? kIndexHead : 0u);
    r.first_end = first_end, r.inner = inner, r.bytes = bytes;
    a.rep[i] = r;
    if (bad) a.s.bad[l.owner] = 1;
}

// One step of the scan with index_sum_combine by a workgroup of kResetScanTile threads, every one of which calls it: -> the value of
// the threads in front, `tile`: of all of them (reset_tile_scan with the operator in place of the sum).
__device__ __forceinline__ IndexSum index_tile_scan(IndexSum v, IndexSum* wave_sum /* LDS, kResetScanTile / kWave */, IndexSum& tile) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    IndexSum incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const IndexSum o = {__shfl_up(incl.e, d), __shfl_up(incl.b, d)};
        if ((int)lane >= d) incl = index_sum_combine(o, incl);
    }
    IndexSum excl = {__shfl_up(incl.e, 1), __shfl_up(incl.b, 1)};
    if (lane == 0) excl = index_sum_identity();
    if (lane == kWave - 1) wave_sum[wave] = incl;
    __syncthreads();
    IndexSum before = index_sum_identity();
    tile = index_sum_identity();
#pragma unroll 1  // (a chain of sixteen dependent steps either way; unrolled, the sixteen values spill)
    for (uint32_t w = 0; w < kResetScanTile / kWave; w++) {
        const IndexSum ws = wave_sum[w];
        if (w < wave) before = index_sum_combine(before, ws);
        tile = index_sum_combine(tile, ws);
    }
    __syncthreads();
    return index_sum_combine(before, excl);
}

struct IndexMergeArgs {
    const IndexChunkReport* rep;
    uint32_t chunks, tiles;  // tiles = ceil(chunks / kResetScanTile)
    uint32_t step;           // 0: a workgroup per tile -> its value  1: one workgroup -> the value in front of every tile, of all
                             // 2: a workgroup per tile -> its chunks' places and running byte counts
    IndexSum* tile_sum;      // tiles
    IndexSum* tile_before;   // tiles + 1
    uint64_t* place;         // chunks + 1
    uint64_t* bytes;         // chunks + 1
    IndexRecord* rec;
};
__global__ void __launch_bounds__(kResetScanTile) tamp_index_merge_kernel(IndexMergeArgs a) {
    __shared__ IndexSum wave_sum[kResetScanTile / kWave];
    IndexSum tile;
    if (a.step == 1) {
        IndexSum base = index_sum_identity();
        for (uint32_t j0 = 0; j0 < a.tiles; j0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
            const uint32_t j = j0 + threadIdx.x;
            const IndexSum at = index_sum_combine(base, index_tile_scan(j < a.tiles ? a.tile_sum[j] : index_sum_identity(), wave_sum, tile));
            if (j < a.tiles) a.tile_before[j] = at;
            base = index_sum_combine(base, tile);
        }
        if (threadIdx.x == 0) {
            a.tile_before[a.tiles] = base;
            a.place[a.chunks] = index_chunk_place(base, kIndexHead), a.bytes[a.chunks] = base.b, a.rec->entries = base.e >> 3;
        }
        return;
    }
    const uint32_t i = blockIdx.x * kResetScanTile + threadIdx.x;
    const bool live = i < a.chunks;
    IndexChunkReport r = {0, 0, 0, 0};
    if (live) r = a.rep[i];
    const IndexSum own = live ? index_sum_of(r.flags, r.inner, r.bytes) : index_sum_identity();
    const IndexSum in_tile = index_tile_scan(own, wave_sum, tile);
    if (a.step == 0) {
        if (threadIdx.x == 0) a.tile_sum[blockIdx.x] = tile;
        return;
    }
    const IndexSum before = index_sum_combine(a.tile_before[blockIdx.x], in_tile);
    if (live) a.place[i] = index_chunk_place(before, r.flags), a.bytes[i] = before.b;
}

struct IndexStreamsArgs {
    IndexCaller c;
    IndexStreams s;
    const uint32_t* g;
    const uint64_t* place;
    const uint64_t* bytes;
    uint64_t* reset_first;  // the caller's tables
    uint32_t* open_size;    // may be null
    int8_t* status;
};
// reset_first is the entries in front of every stream's first chunk.  The open segment starts at the stream's last reset: the lane
// walks the one chunk that holds it once more for the bytes in front of that reset.
__global__ void __launch_bounds__(256) tamp_index_streams_kernel(IndexStreamsArgs a) {
    __shared__ uint8_t lut[128];
    build_prefix_lut(lut);
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > a.c.n) return;
    const uint64_t c0 = a.s.chunk_first[i];
    a.reset_first[i] = index_place_base(a.place[c0]);
    if (i == a.c.n) return;
    const uint64_t c1 = a.s.chunk_first[i + 1];
    const int32_t pre = a.s.pre[i];
    a.status[i] = (int8_t)(pre != kIndexOk ? pre : (a.s.bad[i] ? kIndexOob : kIndexOk));
    if (!a.open_size) return;
    uint64_t from = a.bytes[c0];
    if (index_place_base(a.place[c1]) != index_place_base(a.place[c0])) {
        const uint64_t ch = index_last_entry_chunk(a.place, c0, c1);
        const IndexLane l = index_lane(a.c, a.s.chunk_first, ch);
        uint32_t t = l.k == 0 ? l.first_bit : a.g[ch], bytes = 0;
        bool prev = index_place_flush_in(a.place[ch]), bad = false;
        from = a.bytes[ch];
        while (t != kLongEnd && t < l.end) {
            uint32_t rec;
            const uint32_t k = long_token(l.s, l.len, t, lut, l.hd.wbits, l.hd.lbits, l.hd.minp, l.hd.extended, rec, bad);
            if (!k) break;
            t += k;
            const bool flush = rec == 0xFFFFFFFFu;
            if (flush && prev) from = a.bytes[ch] + bytes;
            if (!flush) bytes += (rec >> 2) & 0xFFu;
            prev = flush;
        }
    }
    a.open_size[i] = index_size(from, a.bytes[c1]);
}

struct IndexSizesArgs {
    const uint64_t* reset_first;  // the caller's, as tamp_index_streams_kernel wrote it
    uint64_t n, entries;
    const uint64_t* chunk_first;
    const uint64_t* bytes;  // per chunk
    const uint64_t* count;  // per entry
    uint32_t* closed_size;
};
__global__ void __launch_bounds__(256) tamp_index_sizes_kernel(IndexSizesArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.entries) return;
    const uint64_t o = batch_reset_owner(a.reset_first, a.n, e);
    a.closed_size[e] = index_size(e == a.reset_first[o] ? a.bytes[a.chunk_first[o]] : a.count[e - 1], a.count[e]);
}

}  // namespace tamp_amd
