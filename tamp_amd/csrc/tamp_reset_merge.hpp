// tamp_reset_merge.hpp -- where the dictionary resets of a stream are, from what a lane per chunk saw (tamp_reset_find_kernel,
// tamp_reset_segments_kernel.hpp).  A reset is a FLUSH whose predecessor is a FLUSH (decompressor.c:501-513): the
// output is byte aligned behind it and the window is the seeded dictionary again, so the bytes between two resets decode on their
// own.  Host arithmetic only, no HIP type: tests/test_reset_segments_host.py compiles it into a stand-alone host program.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace tamp_amd {

constexpr uint32_t kResetChunkHasTokens = 1, kResetChunkFirstFlush = 2, kResetChunkLastFlush = 4;
constexpr uint32_t kResetChunkInner = 4;  // positions a chunk can report; more of them: the exact decoder takes the stream

// What the tokens that START in one chunk of the compressed bits say about resets.
struct ResetChunkReport {
    uint32_t flags;      // kResetChunk*: the chunk has tokens; its first / its last token is a FLUSH
    uint32_t first_end;  // byte position behind the first token (byte aligned when that is a FLUSH)
    uint32_t n_inner;    // FLUSH tokens of the chunk whose predecessor is a FLUSH of the same chunk ...
    uint32_t inner[kResetChunkInner];  // ... and the byte position behind each of the first four
    uint32_t reserved;
};

// The chunks in stream order -> the byte position behind every reset, ascending.  "The previous token was a FLUSH" rides from a
// chunk to the next one that has tokens.  Three FLUSH tokens in a row are two resets (an empty segment between them).
// -> false: a chunk saw more than kResetChunkInner resets.
inline bool reset_merge(const ResetChunkReport* rep, size_t n_chunks, std::vector<uint32_t>& boundaries) {
    boundaries.clear();
    bool last_was_flush = false;  // (the header is no token)
    for (size_t i = 0; i < n_chunks; i++) {
        const ResetChunkReport& r = rep[i];
        if (!(r.flags & kResetChunkHasTokens)) continue;
        if (last_was_flush && (r.flags & kResetChunkFirstFlush)) boundaries.push_back(r.first_end);
        if (r.n_inner > kResetChunkInner) return false;
        for (uint32_t k = 0; k < r.n_inner; k++) boundaries.push_back(r.inner[k]);
        last_was_flush = (r.flags & kResetChunkLastFlush) != 0;
    }
    return true;
}

// The segments those resets cut a stream of n bytes (header_bytes of header in front) into: byte range [start, start + len) each,
// in order, covering [header_bytes, n) exactly.  -> false: positions that do not ascend inside the stream.
inline bool reset_segments_of(const std::vector<uint32_t>& boundaries, uint32_t header_bytes, uint32_t n, std::vector<uint32_t>& start,
                              std::vector<uint32_t>& len) {
    start.clear(), len.clear();
    uint32_t at = header_bytes;
    if (n < header_bytes) return false;
    for (uint32_t b : boundaries) {
        if (b < at || b > n) return false;
        start.push_back(at), len.push_back(b - at);
        at = b;
    }
    start.push_back(at), len.push_back(n - at);
    return true;
}

}  // namespace tamp_amd
