// tamp_reset_index.hpp -- finding the dictionary resets of a BATCH of streams that came without a reset index
// (tamp_batch_index_resets).  The compressed bits of every stream are cut into chunks of kIndexChunkBits, the chunks
// of all streams are numbered through the batch in stream order, and a lane per chunk reports what the tokens that start in its
// chunk say about resets (tamp_reset_index_kernel.hpp).  Here is what turns those reports into the index: what a stream's first bytes
// decide, the operator of the scan over the chunks, and sizes from running byte counts.  Arithmetic only, for the host and the
// device: no HIP type, so that tests/test_index_resets_host.py compiles it into a stand-alone host program.
#pragma once
#include <stdint.h>

#include "tamp_reset_segments.hpp"

namespace tamp_amd {

constexpr uint32_t kIndexChunkBits = 1024;               // TAMP_AMD_INDEX_RESETS_CHUNK_BITS: 128 compressed bytes per lane
constexpr uint32_t kIndexMaxStream = (1u << 29) - 1 - 512;  // 32-bit bit positions, as the long-stream front (kMaxDecodeIn - 512)
constexpr int32_t kIndexOk = 0, kIndexInputExhausted = 2, kIndexInvalidConf = -3, kIndexOob = -4, kIndexBadArgument = -21;

// What a stream's length and first bytes decide (the first rule that applies): a status that ends it there, or its header bytes and
// its chunks.  A refused stream has no chunks and no entries.  (decompressor.c:276-297; `s` is not read when len is 0.)
struct IndexStreamPlan {
    int32_t status;
    uint32_t header_bytes;
    uint32_t chunks;
};
TAMP_HD inline IndexStreamPlan index_stream_plan(const uint8_t* s, uint32_t len, uint32_t max_wbits) {
    if (len == 0) return {kIndexInputExhausted, 0, 0};
    const uint32_t h0 = s[0], hs = 1 + (h0 & 1u);
    if (len < hs) return {kIndexInputExhausted, 0, 0};
    if ((hs == 2 && s[1] != 0) || ((h0 >> 5) & 7u) + 8 > max_wbits) return {kIndexInvalidConf, 0, 0};
    if (len > kIndexMaxStream) return {kIndexBadArgument, 0, 0};
    return {kIndexOk, hs, (uint32_t)((8ull * len + kIndexChunkBits - 1) / kIndexChunkBits)};
}

// A chunk's report: what the tokens that START in it say.
constexpr uint32_t kIndexHasTokens = 1, kIndexFirstFlush = 2, kIndexLastFlush = 4;  // (tamp_reset_merge.hpp's kResetChunk* values)
constexpr uint32_t kIndexHead = 8;  // the chunk is its stream's chunk 0: "the last token was a FLUSH" restarts as false in front of it
struct IndexChunkReport {
    uint32_t flags;
    uint32_t first_end;  // byte position behind the first token
    uint32_t inner;      // FLUSH tokens whose predecessor is a FLUSH of the same chunk: no cap
    uint32_t bytes;      // decoded bytes of the chunk's tokens (a chunk of 1,024 bits: below 2^15)
};

// The scan's value for a run of chunks: the resets inside the run, the bytes it decodes to, and how "the last token was a FLUSH"
// travels through it.  e = entries << 3 | kIndexSum* bits:
//   Pass  the run has no token and no stream's chunk 0: what comes in goes out (then Take and Last are 0)
//   Take  the run's first token is a FLUSH that the chunks in front can reach: it is a reset when a FLUSH comes in
//   Last  what goes out, for a run that does not pass
constexpr uint64_t kIndexSumPass = 1, kIndexSumTake = 2, kIndexSumLast = 4;
struct IndexSum {
    uint64_t e, b;
};
TAMP_HD constexpr IndexSum index_sum_identity() { return {kIndexSumPass, 0}; }
TAMP_HD constexpr IndexSum index_sum_of(uint32_t flags, uint32_t inner, uint32_t bytes) {
    return {((uint64_t)inner << 3) | ((flags & (kIndexHead | kIndexHasTokens)) == 0 ? kIndexSumPass : 0) |
                ((flags & (kIndexHead | kIndexHasTokens | kIndexFirstFlush)) == (kIndexHasTokens | kIndexFirstFlush) ? kIndexSumTake : 0) |
                ((flags & (kIndexHasTokens | kIndexLastFlush)) == (kIndexHasTokens | kIndexLastFlush) ? kIndexSumLast : 0),
            bytes};
}
// a in front of b.  Associative, not commutative.
TAMP_HD constexpr IndexSum index_sum_combine(const IndexSum& a, const IndexSum& b) {
    return {(((a.e >> 3) + (b.e >> 3) + (((a.e & kIndexSumLast) && (b.e & kIndexSumTake)) ? 1 : 0)) << 3) |
                (a.e & b.e & kIndexSumPass) | (((a.e & kIndexSumPass) ? b.e : a.e) & kIndexSumTake) |
                (((b.e & kIndexSumPass) ? a.e : b.e) & kIndexSumLast),
            a.b + b.b};
}
// A chunk's place from the value of all chunks in front of it (the batch starts with "no FLUSH"): its base in the entry table and
// whether a FLUSH comes in, packed as base << 1 | comes_in.
TAMP_HD constexpr uint64_t index_chunk_place(const IndexSum& before, uint32_t flags) {
    return ((before.e >> 3) << 1) | (!(flags & kIndexHead) && (before.e & kIndexSumLast) ? 1 : 0);
}
TAMP_HD constexpr uint64_t index_place_base(uint64_t place) { return place >> 1; }
TAMP_HD constexpr bool index_place_flush_in(uint64_t place) { return (place & 1) != 0; }

// Decoded bytes between two running counts; a value that does not fit 32 bits saturates.
TAMP_HD constexpr uint32_t index_size(uint64_t from, uint64_t to) { return to - from < 0xFFFFFFFFull ? (uint32_t)(to - from) : 0xFFFFFFFFu; }

// The chunk of stream [c0, c1) that holds the stream's LAST entry, given that it has one: the last chunk whose base lies in front of
// the stream's end of entries.  place: the chunks' packed places, one more entry than chunks.
TAMP_HD inline uint64_t index_last_entry_chunk(const uint64_t* place, uint64_t c0, uint64_t c1) {
    const uint64_t end = index_place_base(place[c1]);
    uint64_t lo = c0, hi = c1;  // base(lo) < end <= base(hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (index_place_base(place[mid]) < end) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Rounds the start search may take for a batch whose longest stream has `longest` chunks: a round carries the right starts over a
// workgroup of 64 chunks at least, a stream of `longest` chunks lies in at most ceil(longest / 64) + 1 workgroups (its chunk 0 need
// not be a workgroup's first), and one more round finds nothing moved.
TAMP_HD constexpr uint64_t index_round_bound(uint64_t longest) { return (longest + 63) / 64 + 2; }

}  // namespace tamp_amd
