// tamp_pack_kernel.hpp -- tamp_batch_pack: a batch's streams packed back to back on the device (the index arithmetic:
// tamp_pack.hpp).  Three kernels on the call's stream, none of which waits for another workgroup:
//   tamp_pack_sums_kernel     the padded lengths summed per range of streams (one range per workgroup)
//   tamp_pack_offsets_kernel  per workgroup the sum of the ranges in front of its own, then the exclusive 64-bit scan of its range:
//                             dst_off[0 .. n], the last entry the packed size
//   tamp_pack_copy_kernel     a workgroup per run of destination tiles; over capacity is decided from dst_off[n] before any store
// Plain loads and vector stores only; no atomics: every output byte has one writer.
#pragma once
#include "tamp_common.hpp"
#include "tamp_pack.hpp"
#include "tamp_reset_segments_kernel.hpp"

namespace tamp_amd {

constexpr uint32_t kPackCopyThreads = 256;
constexpr uint32_t kPackLinesPerThread = kPackTile / kPackLine / kPackCopyThreads;
static_assert(kPackLinesPerThread * kPackCopyThreads * kPackLine == kPackTile, "a tile is a whole number of lines per thread");

struct PackScanArgs {
    const uint32_t* src_len;
    uint64_t n;
    uint64_t per;    // streams per workgroup, a multiple of kResetScanTile; the grid is ceil(n / per), one workgroup for n = 0
    uint32_t align;
    uint64_t* sums;     // per workgroup (the offsets kernel reads those in front of its own: none when there is one workgroup)
    uint64_t* dst_off;  // n + 1 entries
};
__global__ void __launch_bounds__(kResetScanTile) tamp_pack_sums_kernel(PackScanArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    const uint64_t first = blockIdx.x * a.per, end = a.n - first < a.per ? a.n : first + a.per;
    uint64_t sum = 0;
    for (uint64_t t0 = first; t0 < end; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint64_t i = t0 + threadIdx.x;
        uint64_t tile;
        (void)reset_tile_scan(i < end ? pack_padded(a.src_len[i], a.align) : 0, wave_sum, tile);
        sum += tile;
    }
    if (threadIdx.x == 0) a.sums[blockIdx.x] = sum;
}
__global__ void __launch_bounds__(kResetScanTile) tamp_pack_offsets_kernel(PackScanArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    const uint64_t first = blockIdx.x * a.per, end = a.n - first < a.per ? a.n : first + a.per;
    uint64_t base = 0;
    for (uint32_t j0 = 0; j0 < blockIdx.x; j0 += kResetScanTile) {  // (uniform bounds)
        const uint32_t j = j0 + threadIdx.x;
        uint64_t tile;
        (void)reset_tile_scan(j < blockIdx.x ? a.sums[j] : 0, wave_sum, tile);
        base += tile;
    }
    for (uint64_t t0 = first; t0 < end; t0 += kResetScanTile) {  // (uniform bounds)
        const uint64_t i = t0 + threadIdx.x;
        uint64_t tile;
        const uint64_t at = base + reset_tile_scan(i < end ? pack_padded(a.src_len[i], a.align) : 0, wave_sum, tile);
        if (i < end) a.dst_off[i] = at;
        base += tile;
    }
    if (threadIdx.x == 0 && end == a.n) a.dst_off[a.n] = base;  // (the last range's workgroup: the packed size)
}

// A workgroup takes a run of neighbouring tiles, so that only its first tile searches the whole of dst_off for its first stream.
// Every thread takes kPackLinesPerThread lines of a tile, each kPackCopyThreads lines from the next: a wavefront's loads and stores
// are 1 KiB of neighbouring lines.  No barrier, no shuffle: the loops over streams are each thread's own.
__global__ void __launch_bounds__(kPackCopyThreads)
tamp_pack_copy_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off, const uint32_t* __restrict__ src_len,
                      uint8_t* __restrict__ dst, uint64_t dst_cap, const uint64_t* __restrict__ dst_off, uint64_t n) {
    const uint64_t total = dst_off[n];
    if (total > dst_cap || total == 0) return;  // (over capacity: no byte of dst is written)
    const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & (kPackTile - 1));
    const uint64_t tiles = pack_tile_count(skew, total), run = (tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t t_first = blockIdx.x * run, t_end = tiles - t_first < run ? tiles : t_first + run;
    uint64_t s_hi = 0;
    for (uint64_t t = t_first; t < t_end && t_first < tiles; t++) {
        const PackSpan tile = pack_tile_span(skew, total, t);
        const uint64_t s_lo = t == t_first ? pack_owner(dst_off, 0, n, tile.lo) : pack_owner_from(dst_off, s_hi, n, tile.lo);
        s_hi = pack_owner_from(dst_off, s_lo, n, tile.hi - 1);
        if (s_lo == s_hi && tile.hi - tile.lo == kPackTile && tile.hi <= dst_off[s_lo] + src_len[s_lo]) {
            // the whole tile inside one stream's body: all loads in flight, then all stores
            const uint8_t* const p = src + src_off[s_lo] + (tile.lo - dst_off[s_lo]) + threadIdx.x * kPackLine;
            uint4* const q = reinterpret_cast<uint4*>(dst + tile.lo) + threadIdx.x;
            PackU128 v[kPackLinesPerThread];
#pragma unroll
            for (uint32_t j = 0; j < kPackLinesPerThread; j++) v[j] = *reinterpret_cast<const PackU128*>(p + j * kPackCopyThreads * kPackLine);
#pragma unroll
            for (uint32_t j = 0; j < kPackLinesPerThread; j++) q[j * kPackCopyThreads] = make_uint4(v[j].v[0], v[j].v[1], v[j].v[2], v[j].v[3]);
            continue;
        }
        for (uint32_t line = threadIdx.x; line < kPackTile / kPackLine; line += kPackCopyThreads) {
            const PackSpan s = pack_line_span(skew, total, t, line);
            if (s.hi <= s.lo) continue;  // (in front of dst in the first tile, behind the packed bytes in the last)
            const uint64_t i = pack_owner(dst_off, s_lo, s_hi + 1, s.lo);
            if (pack_line_is_body(dst_off, src_len, i, s)) {
                const PackU128 v = *reinterpret_cast<const PackU128*>(src + src_off[i] + (s.lo - dst_off[i]));
                *reinterpret_cast<uint4*>(dst + s.lo) = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
                continue;
            }
            // where in its line s.lo stands: 0 for every line but the first of a destination that is not 16-byte aligned
            const uint32_t k0 = (uint32_t)((s.lo + skew) & (kPackLine - 1));
            const PackLine x = pack_line_value(src, src_off, src_len, dst_off, i, s_hi + 1, s, k0);
            if (s.hi - s.lo == kPackLine) {
                *reinterpret_cast<uint4*>(dst + s.lo) = make_uint4((uint32_t)x.x0, (uint32_t)(x.x0 >> 32), (uint32_t)x.x1, (uint32_t)(x.x1 >> 32));
            } else {  // the first or the last line of the packed bytes, cut by their ends: at most 15 bytes, twice per call
#pragma clang loop vectorize(disable)  // (byte stores: the bytes around them are not this call's)
                for (uint32_t b = 0; b < (uint32_t)(s.hi - s.lo); b++) {
                    const uint32_t k = k0 + b;
                    dst[s.lo + b] = (uint8_t)((k < 8 ? x.x0 : x.x1) >> (8 * (k & 7)));
                }
            }
        }
    }
}

}  // namespace tamp_amd
