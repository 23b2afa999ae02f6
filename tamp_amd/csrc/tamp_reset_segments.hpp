// tamp_reset_segments.hpp -- the segment table of a dictionary-reset call (tamp_amd_compress_resets): how a buffer
// is cut into segments, what a segment's slab holds, what the whole stream can take -- and, for a batch of such buffers
// (tamp_batch_compress_resets), which stream and cut a row of its two segment tables stands for.  Arithmetic only, for the host and
// the device: no HIP type, so that tests/test_reset_segments_host.py and tests/test_batch_resets_host.py compile it into stand-alone
// host programs.  The kernels that use it:
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

}  // namespace tamp_amd
