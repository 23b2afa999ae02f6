// tamp_segment_ends_kernel.hpp -- tamp_batch_segment_ends: the table of segment ends from what tamp_batch_index_resets returns
// (DESIGN.md 3.13 "Reading ranges"; the arithmetic: tamp_reset_segments.hpp).  A running sum per stream over the rows of the whole
// batch, a lane per ROW: one stream may have more rows than a scan tile and most have a handful, so no lane loops over a stream.
// The scheme is tamp_batch_pack's (sums per range of rows, then per workgroup the ranges in front of its own and the scan of its
// range), with the stream's base folded into the operator: a SEGMENTED sum (segment_end_combine), whose value starts again at
// every stream's first row -- a base subtracted afterwards would not undo a saturated sum.  A row's stream is found the way
// batch_reset_owner finds owners.  The row count first[n] + n is read on the device: the grid is fixed, nothing is read back.
//   tamp_segment_ends_sums_kernel   a workgroup per range of rows: the range's sum
//   tamp_segment_ends_apply_kernel  the sums in front of its own range, then the scan of its range into segment_end
// Plain loads and vector stores only; no atomics: every entry has one writer.
#pragma once
#include "tamp_common.hpp"
#include "tamp_reset_segments.hpp"
#include "tamp_reset_segments_kernel.hpp"

namespace tamp_amd {

constexpr uint32_t kSegmentEndsMaxGrid = kResetScanTile;  // (the apply kernel sums the ranges in front of its own in one step)

struct SegmentEndsArgs {
    const uint64_t* first;        // n + 1
    const uint32_t* closed_size;  // first[n]
    const uint32_t* open_size;    // n
    uint64_t n;
    SegmentEndSum* sums;    // per workgroup
    uint64_t* segment_end;  // first[n] + n
};
// The rows of workgroup b: [r0, r1), tiles of kResetScanTile from r0 (the same cut in both kernels).
__device__ __forceinline__ void segment_ends_range(const SegmentEndsArgs& a, uint64_t& r0, uint64_t& r1) {
    const uint64_t rows = a.first[a.n] + a.n, steps = (rows + kResetScanTile - 1) / kResetScanTile;
    const uint64_t per = (steps + gridDim.x - 1) / gridDim.x * kResetScanTile;
    r0 = blockIdx.x * per < rows ? blockIdx.x * per : rows;
    r1 = rows - r0 < per ? rows : r0 + per;
}
// One step of the scan with segment_end_combine by a workgroup of kResetScanTile threads, every one of which calls it: -> the value
// of the threads up to and WITH the caller's, `tile`: of all of them (reset_tile_scan with the operator in place of the sum).
__device__ __forceinline__ SegmentEndSum segment_ends_tile_scan(SegmentEndSum v, SegmentEndSum* wave_sum /* LDS, kResetScanTile / kWave */,
                                                                SegmentEndSum& tile) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    SegmentEndSum incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const SegmentEndSum o = {__shfl_up(incl.v, d), __shfl_up(incl.head, d)};
        if ((int)lane >= d) incl = segment_end_combine(o, incl);
    }
    if (lane == kWave - 1) wave_sum[wave] = incl;
    __syncthreads();
    SegmentEndSum before = segment_end_identity();
    tile = segment_end_identity();
    for (uint32_t w = 0; w < kResetScanTile / kWave; w++) {
        const SegmentEndSum ws = wave_sum[w];
        if (w < wave) before = segment_end_combine(before, ws);
        tile = segment_end_combine(tile, ws);
    }
    __syncthreads();
    return segment_end_combine(before, incl);
}

__global__ void __launch_bounds__(kResetScanTile) tamp_segment_ends_sums_kernel(SegmentEndsArgs a) {
    __shared__ SegmentEndSum wave_sum[kResetScanTile / kWave];
    uint64_t r0, r1;
    segment_ends_range(a, r0, r1);
    SegmentEndSum sum = segment_end_identity();
    for (uint64_t t0 = r0; t0 < r1; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint64_t p = t0 + threadIdx.x;
        SegmentEndSum tile;
        (void)segment_ends_tile_scan(p < r1 ? segment_end_term(a.first, a.closed_size, a.open_size, a.n, p) : segment_end_identity(), wave_sum, tile);
        sum = segment_end_combine(sum, tile);
    }
    if (threadIdx.x == 0) a.sums[blockIdx.x] = sum;
}
__global__ void __launch_bounds__(kResetScanTile) tamp_segment_ends_apply_kernel(SegmentEndsArgs a) {
    __shared__ SegmentEndSum wave_sum[kResetScanTile / kWave];
    uint64_t r0, r1;
    segment_ends_range(a, r0, r1);
    if (r0 >= r1) return;  // (the whole workgroup)
    SegmentEndSum base;
    {  // gridDim.x <= kSegmentEndsMaxGrid: one step
        const bool front = threadIdx.x < blockIdx.x;
        (void)segment_ends_tile_scan(front ? a.sums[threadIdx.x] : segment_end_identity(), wave_sum, base);
    }
    for (uint64_t t0 = r0; t0 < r1; t0 += kResetScanTile) {  // (uniform bounds)
        const uint64_t p = t0 + threadIdx.x;
        SegmentEndSum tile;
        const SegmentEndSum at =
            segment_ends_tile_scan(p < r1 ? segment_end_term(a.first, a.closed_size, a.open_size, a.n, p) : segment_end_identity(), wave_sum, tile);
        if (p < r1) a.segment_end[p] = segment_end_combine(base, at).v;
        base = segment_end_combine(base, tile);
    }
}

}  // namespace tamp_amd
