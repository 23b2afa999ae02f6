// tamp_reset_segments.hpp -- the segment table of a dictionary-reset call (tamp_amd_compress_resets): how a buffer
// is cut into segments, what a segment's slab holds, what the whole stream can take.  Arithmetic only, for the host and the device:
// no HIP type, so that tests/test_reset_segments_host.py compiles it into a stand-alone host program.  The kernels that use it:
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

}  // namespace tamp_amd
