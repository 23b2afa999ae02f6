// tamp_read_ranges_kernel.hpp -- byte ranges of reset-segmented streams, read without decoding the rest (tamp_batch_read_ranges,
// DESIGN.md 3.13 "Reading ranges"; the arithmetic: tamp_reset_segments.hpp).
//
// A range touches a few segments of one stream; each is a UNIT: staged behind a copy of the stream's two header bytes as a stream
// of its own, walked token by token, decoded by the existing launch path into the range's scratch with its room trimmed to the
// last byte asked for, and the range's bytes are one contiguous copy out of that scratch.  The steps are kernels of their own on
// the call's stream; no workgroup waits for another, no atomics but two in LDS:
//   tamp_read_count_kernel   a lane per range, the shared tile scan: units, staged bytes and scratch bytes per range and their
//                            exclusive scans, the range's verdict where it has one already, the 16-byte record of the call
//   tamp_read_units_kernel   a lane per unit: owner range by binary search, the cut with the range and order check of its entries,
//                            what is asked of it, its place in the stage and in the scratch
//   tamp_read_stage_kernel   a workgroup per unit: header + segment into the stage (reset_copy)
//   tamp_read_walk_kernel    a lane per staged unit: decoded size, ends at its boundary behind FLUSH, FLUSH, no offset out of the
//                            window, a closed segment exactly N bytes and the open one N at most; the unit's out_cap
//   (the decode: launch_decompress_locked over the unit rows)
//   tamp_read_gather_kernel  a workgroup per range: its status and length, its bytes from the scratch to the caller's buffer
// A host-memory call makes the first three steps on the host, with the same functions, and uploads the units' rows and the stage.
//
// THE GRID is a policy of the count, units, walk and gather steps: every closed segment N bytes (tamp_batch_read_ranges: the
// ...Args structs, whose instantiations are the code the kernels were before there was a choice), or the table of segment ends
// (tamp_batch_read_ranges_grid: the ...GridArgs structs, which carry a ReadTable behind the same members).  With the table a unit's
// size is its table size, which the walk holds the closed AND the open segment to, and the gather's skip comes from the plan.
#pragma once
#include "tamp_common.hpp"
#include "tamp_reset_segments.hpp"
#include "tamp_reset_segments_kernel.hpp"

namespace tamp_amd {

static_assert(kReadMaxSegment == kMaxDecodeIn - 512, "the walk's 32-bit bit positions");
static_assert(kReadOk == kOk && kReadInputExhausted == kInputExhausted && kReadInvalidConf == kInvalidConf && kReadBadArgument == kBadArgument, "status codes");

constexpr uint8_t kReadUnitClosed = 1, kReadUnitBehindReset = 2;  // a unit's flags
constexpr uint8_t kReadWalkOk = 0, kReadWalkOob = 1, kReadWalkBad = 2;  // a unit's verdict

// The caller's tables (device memory; a host-memory call: its copies).
struct ReadCaller {
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    const uint64_t* first;
    const uint32_t* off;
    uint64_t n;
    uint32_t interval, max_wbits;
    const uint32_t* range_stream;
    const uint64_t* range_begin;
    const uint32_t* range_len;
    uint64_t n_ranges;
};

// Per range of the call, in the stream's scratch: three exclusive scans with one entry more than ranges (a range's cost is the sum
// of its three entries' steps, the units' weighted with kReadUnitRow), the verdict, and whether one of its units has a bad cut.
struct ReadRanges {
    uint64_t* unit_first;
    uint64_t* scratch_first;
    uint64_t* stage_first;
    int8_t* verdict;
    uint8_t* failed;
};
struct ReadRecord { uint64_t units, cost; };  // what a device-memory call reads back: all units, all bytes of scratch they ask for
// The table form's own: the caller's table (null where a step does not read it) and, in the stream's scratch behind the per-range
// tables, where each range's bytes start in its scratch (<- the count).  A unit's table size lies in its `size` row (<- the units
// step), where the walk finds it and leaves what it counted.
struct ReadTable {
    const uint64_t* segment_end;
    uint64_t* skip;
};

// The units' rows of a slice [q0, q1) of the ranges: U = unit_first[q1] - unit_first[q0] rows.  Offsets count from the slice's
// region, which holds the rows, the stage and the scratch, in this order.
struct ReadUnits {
    uint64_t* in_off;   // where the staged unit starts
    uint64_t* out_off;  // where it decodes to
    uint32_t* in_len;   // segment + header bytes; 0: no unit, or one that failed
    uint32_t* need;     // decoded bytes asked of it
    uint32_t* owner;    // its range, counted from q0
    uint8_t* flags;
    uint8_t* verdict;
    // (a host-memory call uploads the rows above)
    uint64_t* src_off;  // where its segment starts in the caller's input
    uint32_t* out_cap;  // min(size, need)
    uint32_t* out_len;  // <- the decode
    uint32_t* size;     // <- the walk
    int8_t* status;     // <- the decode
};
// Bytes of the rows a host-memory call uploads, and of all rows; both multiples of 8.
__host__ __device__ constexpr uint64_t read_units_upload_bytes(uint64_t U) { return (30 * U + 7) & ~7ull; }
__host__ __device__ constexpr uint64_t read_units_bytes(uint64_t U) { return (read_units_upload_bytes(U) + 21 * U + 255) & ~255ull; }
static_assert(30 + 21 <= kReadUnitRow, "a unit's rows stay inside what the budget counts for them");
__host__ __device__ inline ReadUnits read_units_at(uint8_t* base, uint64_t U) {
    ReadUnits u;
    u.in_off = reinterpret_cast<uint64_t*>(base), u.out_off = u.in_off + U;
    u.in_len = reinterpret_cast<uint32_t*>(u.out_off + U), u.need = u.in_len + U, u.owner = u.need + U;
    u.flags = reinterpret_cast<uint8_t*>(u.owner + U), u.verdict = u.flags + U;
    u.src_off = reinterpret_cast<uint64_t*>(base + read_units_upload_bytes(U));
    u.out_cap = reinterpret_cast<uint32_t*>(u.src_off + U), u.out_len = u.out_cap + U, u.size = u.out_len + U;
    u.status = reinterpret_cast<int8_t*>(u.size + U);
    return u;
}
// Where the stage and the scratch of a slice start in its region.
__host__ __device__ constexpr uint64_t read_stage_at(uint64_t U) { return read_units_bytes(U); }
__host__ __device__ constexpr uint64_t read_scratch_at(uint64_t U, uint64_t staged) { return (read_stage_at(U) + staged + 64 + 255) & ~255ull; }
// (the slack of 64 bytes: the decoders' vector loads may run past a unit's last byte)
__host__ __device__ constexpr uint64_t read_region_bytes(uint64_t U, uint64_t staged, uint64_t scratch) { return read_scratch_at(U, staged) + scratch + 64; }

struct ReadCountArgs {
    static constexpr bool kTable = false;
    ReadCaller c;
    uint64_t budget;
    ReadRanges r;
    ReadRecord* rec;
};
struct ReadCountGridArgs {
    static constexpr bool kTable = true;
    ReadCaller c;
    uint64_t budget;
    ReadRanges r;
    ReadRecord* rec;
    ReadTable g;
};
template <class A>
__global__ void __launch_bounds__(kResetScanTile) tamp_read_count_kernel(A a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    // what every range comes to, into the tables (each lane reads back only what it wrote itself) ...
    for (uint64_t q = threadIdx.x; q < a.c.n_ranges; q += kResetScanTile) {
        ReadPlan p;
        if constexpr (A::kTable) {  // (the table form leaves the range's skip for the gather)
            const ReadGridPlan g = read_grid_plan(a.c.in, a.c.in_off, a.c.in_len, a.c.first, a.c.off, a.g.segment_end, a.c.n, a.c.max_wbits,
                                                  a.budget, a.c.range_stream[q], a.c.range_begin[q], a.c.range_len[q]);
            p = g.p, a.g.skip[q] = g.skip;
        } else {
            p = read_range_plan(a.c.in, a.c.in_off, a.c.in_len, a.c.first, a.c.off, a.c.n, a.c.interval, a.c.max_wbits, a.budget,
                                a.c.range_stream[q], a.c.range_begin[q], a.c.range_len[q]);
        }
        a.r.unit_first[q] = p.units, a.r.scratch_first[q] = p.scratch, a.r.stage_first[q] = p.staged;
        a.r.verdict[q] = (int8_t)p.verdict, a.r.failed[q] = 0;
    }
    // ... and the three exclusive scans over them, in place
    uint64_t units = 0, scratch = 0, staged = 0;
    for (uint64_t t0 = 0; t0 < a.c.n_ranges; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint64_t q = t0 + threadIdx.x;
        const bool live = q < a.c.n_ranges;
        uint64_t tile;
        const uint64_t u_at = units + reset_tile_scan(live ? a.r.unit_first[q] : 0, wave_sum, tile);
        units += tile;
        const uint64_t s_at = scratch + reset_tile_scan(live ? a.r.scratch_first[q] : 0, wave_sum, tile);
        scratch += tile;
        const uint64_t g_at = staged + reset_tile_scan(live ? a.r.stage_first[q] : 0, wave_sum, tile);
        staged += tile;
        if (live) a.r.unit_first[q] = u_at, a.r.scratch_first[q] = s_at, a.r.stage_first[q] = g_at;
    }
    if (threadIdx.x == 0) {
        const uint64_t n = a.c.n_ranges;
        a.r.unit_first[n] = units, a.r.scratch_first[n] = scratch, a.r.stage_first[n] = staged;
        a.rec->units = units, a.rec->cost = scratch + staged + kReadUnitRow * units;  // (the sum of read_plan_cost over the ranges)
    }
}

struct ReadSlice {
    uint64_t q0, q1;  // the slice's ranges
    uint64_t U;       // its units: unit_first[q1] - unit_first[q0]
    uint8_t* region;  // rows, stage, scratch
};

struct ReadUnitsArgs {
    static constexpr bool kTable = false;
    ReadCaller c;
    uint64_t budget;
    ReadRanges r;
    ReadSlice s;
};
struct ReadUnitsGridArgs {
    static constexpr bool kTable = true;
    ReadCaller c;
    uint64_t budget;
    ReadRanges r;
    ReadSlice s;
    ReadTable g;
};
template <class A>
__global__ void __launch_bounds__(256) tamp_read_units_kernel(A a) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.s.U) return;
    const ReadUnits u = read_units_at(a.s.region, a.s.U);
    const uint64_t g = a.r.unit_first[a.s.q0] + x;  // the unit, counted through the call
    uint64_t lo = a.s.q0, hi = a.s.q1;  // unit_first[lo] <= g < unit_first[hi] (ranges without units are stepped over)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.r.unit_first[mid] <= g) lo = mid;
        else hi = mid;
    }
    const uint64_t q = lo, j = g - a.r.unit_first[q];
    const uint32_t i = a.c.range_stream[q];
    // (the plan again: the range has units, so the stream and its rows of the index held up)
    ReadPlan p;
    [[maybe_unused]] ReadGridPlan gp;
    if constexpr (A::kTable) {
        gp = read_grid_plan(a.c.in, a.c.in_off, a.c.in_len, a.c.first, a.c.off, a.g.segment_end, a.c.n, a.c.max_wbits, a.budget, i,
                            a.c.range_begin[q], a.c.range_len[q]);
        p = gp.p;
    } else {
        p = read_range_plan(a.c.in, a.c.in_off, a.c.in_len, a.c.first, a.c.off, a.c.n, a.c.interval, a.c.max_wbits, a.budget, i,
                            a.c.range_begin[q], a.c.range_len[q]);
    }
    const uint64_t staged = a.r.stage_first[a.s.q1] - a.r.stage_first[a.s.q0];
    ReadUnit w = {{0, 0, false, false}, 0, 0, 0, 0};  // (stays so only if the tables changed behind the count kernel: nothing is read through them then)
    const bool counted = p.verdict == kReadGo && j < p.units;
    if constexpr (A::kTable) {
        uint32_t size = 0;
        if (counted) {
            const ReadGridUnit gw = read_grid_unit(a.c.first, a.c.off, a.c.in_len, a.g.segment_end, i, gp, j);
            w = gw.u, size = gw.size;
        }
        u.size[x] = size;  // (what the walk holds the unit to)
    } else {
        if (counted) w = read_range_unit(a.c.first, a.c.off, a.c.in_len, a.c.interval, i, p, j);
    }
    u.in_off[x] = read_stage_at(a.s.U) + (a.r.stage_first[q] - a.r.stage_first[a.s.q0]) + w.place;
    u.out_off[x] = read_scratch_at(a.s.U, staged) + (a.r.scratch_first[q] - a.r.scratch_first[a.s.q0]) + w.room;
    u.in_len[x] = w.in_len, u.need[x] = w.need, u.owner[x] = (uint32_t)(q - a.s.q0);
    u.flags[x] = (uint8_t)((w.cut.closed ? kReadUnitClosed : 0) | (p.k0 + j ? kReadUnitBehindReset : 0));
    u.verdict[x] = w.cut.ok ? kReadWalkOk : kReadWalkBad;
    u.src_off[x] = counted ? a.c.in_off[i] + w.cut.start : 0;
    if (!w.cut.ok) a.r.failed[q] = 1;  // (several units may store that same value)
}

struct ReadStageArgs {
    ReadCaller c;
    ReadSlice s;
};
__global__ void __launch_bounds__(256) tamp_read_stage_kernel(ReadStageArgs a) {
    const ReadUnits u = read_units_at(a.s.region, a.s.U);
    for (uint64_t x = blockIdx.x; x < a.s.U; x += gridDim.x) {
        const uint32_t len = u.in_len[x];
        if (!len) continue;
        uint8_t* const dst = a.s.region + u.in_off[x];
        const uint32_t i = a.c.range_stream[a.s.q0 + u.owner[x]];
        // (the stream's own two header bytes: the second one is zero)
        if (threadIdx.x == 64) dst[0] = a.c.in[a.c.in_off[i]], dst[1] = 0;
        reset_copy(dst + kResetHeaderBytes, a.c.in + u.src_off[x], len - kResetHeaderBytes, false, 0);
    }
}

struct ReadWalkArgs {
    static constexpr bool kTable = false;
    ReadSlice s;
    const uint8_t* failed;  // per range of the call
    uint32_t interval;
};
struct ReadWalkGridArgs {
    static constexpr bool kTable = true;
    ReadSlice s;
    const uint8_t* failed;
};
template <class A>
__global__ void __launch_bounds__(64) tamp_read_walk_kernel(A a) {
    __shared__ uint8_t lut[128];
    build_prefix_lut(lut);
    __syncthreads();
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.s.U) return;
    const ReadUnits u = read_units_at(a.s.region, a.s.U);
    uint32_t grid_n;  // fixed grid: the interval; the table: the unit's table size
    if constexpr (A::kTable) grid_n = u.size[x];
    else grid_n = a.interval;
    const uint32_t n = u.in_len[x], N = grid_n;
    uint64_t bytes = 0;
    uint8_t verdict = u.verdict[x];
    if (n && verdict == kReadWalkOk) {
        const uint8_t* const s = a.s.region + u.in_off[x];
        const StreamHeader hd = decode_header(s[0]);
        const bool closed = (u.flags[x] & kReadUnitClosed) != 0;
        // the walk of the staged unit: from behind its header, never a bit read at or behind its end.  The reference keeps "the last
        // token was a FLUSH" across a reset, so segments behind one start with it set
        const uint32_t end = 8 * n;
        uint32_t t = 8 * kResetHeaderBytes;
        bool last = (u.flags[x] & kReadUnitBehindReset) != 0, before = last, bad = false;
        while (t < end) {  // (long_token: at least one bit, or 0; to the end whatever the size: an offset out of the window counts first)
            uint32_t rec;
            const uint32_t k = long_token(s, n, t, lut, hd.wbits, hd.lbits, hd.minp, hd.extended, rec, bad);
            if (!k) break;
            t += k;
            before = last, last = rec == 0xFFFFFFFFu;
            if (!last) bytes += (rec >> 2) & 0xFFu;
        }
        // a closed segment ends exactly at its boundary behind FLUSH, FLUSH and holds exactly N bytes, which is what makes k * N an
        // address; the open one ends as a stream ends, out of tokens, with N bytes at most -- or, with the table, its table size too
        const bool ok = closed ? (t == end && last && before && bytes == N) : (A::kTable ? bytes == N : bytes <= N);
        verdict = bad ? kReadWalkOob : (ok ? kReadWalkOk : kReadWalkBad);
    }
    const bool decode = n && verdict == kReadWalkOk && !a.failed[a.s.q0 + u.owner[x]];
    const uint32_t size = verdict == kReadWalkOk ? (uint32_t)bytes : 0;
    u.verdict[x] = verdict, u.size[x] = size;
    u.out_cap[x] = decode ? min(size, u.need[x]) : 0;
    if (!decode) u.in_len[x] = 0;  // (an empty stream for the decoders)
}

struct ReadGatherArgs {
    static constexpr bool kTable = false;
    ReadCaller c;
    ReadRanges r;
    ReadSlice s;
    uint8_t* out;  // the caller's buffer and tables (a host-memory call: the ranges of the slice packed, out_off counted from q0)
    const uint64_t* out_off;
    uint32_t* out_len;
    int8_t* status;
};
struct ReadGatherGridArgs {
    static constexpr bool kTable = true;
    ReadCaller c;
    ReadRanges r;
    ReadSlice s;
    uint8_t* out;
    const uint64_t* out_off;
    uint32_t* out_len;
    int8_t* status;
    ReadTable g;
};
template <class A>
__global__ void __launch_bounds__(256) tamp_read_gather_kernel(A a) {
    __shared__ unsigned long long total_s;
    __shared__ uint32_t seen_s;
    const ReadUnits u = read_units_at(a.s.region, a.s.U);
    for (uint64_t q = a.s.q0 + blockIdx.x; q < a.s.q1; q += gridDim.x) {
        const int32_t pre = a.r.verdict[q];
        if (pre != kReadGo) {
            if (threadIdx.x == 0) a.status[q] = (int8_t)pre, a.out_len[q] = 0;
            continue;
        }
        if (threadIdx.x == 0) total_s = 0, seen_s = 0;
        __syncthreads();
        const uint64_t x0 = a.r.unit_first[q] - a.r.unit_first[a.s.q0], x1 = a.r.unit_first[q + 1] - a.r.unit_first[a.s.q0];
        uint64_t total = 0;
        uint32_t seen = 0;  // 1: an offset out of the window, 2: a unit that does not hold up, 4: a decode that disagrees with the walk
        for (uint64_t x = x0 + threadIdx.x; x < x1; x += blockDim.x) {
            const uint8_t v = u.verdict[x];
            seen |= v == kReadWalkOob ? 1u : (v == kReadWalkBad ? 2u : 0u);
            const int8_t st = u.status[x];
            if (v == kReadWalkOk && u.in_len[x] && (u.out_len[x] != u.out_cap[x] || (st != (int8_t)kInputExhausted && st != (int8_t)kOutputFull))) seen |= 4u;
            total += u.out_cap[x];
        }
        if (total) atomicAdd(&total_s, (unsigned long long)total);
        if (seen) atomicOr(&seen_s, seen);
        __syncthreads();
        total = total_s, seen = seen_s;
        __syncthreads();  // (the next range of this workgroup zeroes the two words)
        const uint32_t len = a.c.range_len[q];
        int8_t status;
        uint32_t delivered = 0;
        if (seen & 1u) status = (int8_t)kOob;
        else if (seen & 2u) status = (int8_t)kReadBadIndex;
        else if (seen & 4u) status = (int8_t)kError;
        else {
            uint64_t skip;
            if constexpr (A::kTable) skip = a.g.skip[q];
            else skip = read_range_skip(a.c.range_begin[q], a.c.range_begin[q] / a.c.interval, a.c.interval);
            delivered = read_range_delivered(total, skip, len);
            status = delivered == len ? (int8_t)kOk : (int8_t)kInputExhausted;
            // the range's units decoded back to back from its first scratch byte: one contiguous copy
            if (delivered) reset_copy(a.out + a.out_off[q], a.s.region + u.out_off[x0] + skip, delivered, false, 0);
        }
        if (threadIdx.x == 0) a.status[q] = status, a.out_len[q] = delivered;
    }
}

}  // namespace tamp_amd
