// tamp_decoded_size_pieces_kernel.hpp -- the size query for decoder OBJECTS (tamp_batch_decoded_size_pieces): what one call of
// tamp_decompress_resume_kernel would report -- out_len, status, in_consumed -- for an object, a piece of input and an amount of
// output room, without decoding anything.
//
// One lane per row, like the size-only build of the parse (tamp_decompress_split_kernel.hpp, parse_stream<false>), and for the
// same reason: what a token produces follows from its own bits and the out-of-bounds rule from offset + length <= W, so neither
// needs the window.  What differs is where a row starts: not at a header but wherever the object's last call stopped
// (decompressor.c:371-578 entered with a configured object) --
//   * up to 32 bits in the bit buffer: RefReader is seeded with them, and its refill rule gives the consumed count from there;
//   * no header yet, or its first byte stashed by a one-byte call (flags & 2, the byte in skip_bytes);
//   * a token cut short: an RLE run or extended match that has delivered skip_bytes of its bytes (count and offset parked in the
//     state), an extended match whose size is parked and whose offset is still to come, an RLE / extended symbol committed and
//     starved of its payload, a plain match that delivered skip_bytes and still sits in the bit buffer.
// The row reads the object's 16 state bytes and its input, never the window, and writes nothing to the object: any number of
// rows may name the same one.  The token grammar is exact_token / exact_payload (tamp_decode_common.hpp), the reference's own
// loop; the parse's fast loop is not used (DESIGN.md 7 has the measurement).
#pragma once
#include "tamp_decode_common.hpp"
#include "tamp_decompress_resume_kernel.hpp"

namespace tamp_amd {

struct SizePiecesArgs {
    const uint8_t* states;  // object i at states + i * state_stride: its first 16 bytes are read
    uint64_t state_stride;
    const uint32_t* object_index;  // row r acts on object object_index[r]; null: on object r
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    const uint32_t* limit;  // out_cap of the decode call asked about; null: none below 2^32 - 1
    uint32_t* out_len;
    int8_t* status;
    uint32_t* in_consumed;  // may be null
    uint32_t n_rows;
    uint32_t spw;  // rows per wavefront (16, 32 or 64)
    uint32_t max_wbits;
};

__device__ __forceinline__ void size_piece(const SizePiecesArgs& a, const uint32_t row) {
    const uint32_t obj = a.object_index ? a.object_index[row] : row;
    const uint32_t* const sw = reinterpret_cast<const uint32_t*>(a.states + (uint64_t)obj * a.state_stride);
    // state words: tamp_decompress_resume_kernel.hpp
    const uint32_t s0 = sw[0], s1 = sw[1], s2 = sw[2], s3 = sw[3];
    uint32_t ts = s1 >> 24;
    const uint32_t carried = (s1 >> 16) & 0xFFu;
    const uint32_t pend_off = s2 & 0xFFFFu, pend_size = s2 >> 16;
    uint32_t conf = s3 & 0xFFu, skip = (s3 >> 8) & 0xFFu;
    const uint32_t flags = (s3 >> 16) & 0xFFu, bits_max = s3 >> 24;

    const uint8_t* const in = a.in + a.in_off[row];
    const uint32_t n = a.in_len[row] < kMaxDecodeCall ? a.in_len[row] : kMaxDecodeCall;
    const uint32_t cap = a.limit ? a.limit[row] : 0xFFFFFFFFu;
    RefReader r{in, n};
    uint32_t op = 0;
    int res = kInputExhausted;

    do {
        if (bits_max < 8 || bits_max > 15 || bits_max > a.max_wbits) { res = kInvalidConf; break; }
        if (!(flags & kDsConfigured)) {  // decompressor.c:389-429
            uint32_t h0, hs;
            if (n == 0) break;
            if (flags & kDsHeaderStashed) {
                h0 = skip;
                if (in[0]) { res = kInvalidConf; break; }
                hs = 1;
            } else {
                h0 = in[0];
                if ((h0 & 1) && n < 2) { r.ip = 1; break; }
                if ((h0 & 1) && in[1]) { res = kInvalidConf; break; }
                hs = 1 + (h0 & 1);
            }
            r.ip = hs;
            if (decode_header(h0).wbits > bits_max) { res = kInvalidConf; break; }
            conf = h0, skip = 0;
        } else if (carried) {
            r.bb = s0 & (0xFFFFFFFFu << (32 - carried)), r.nb = carried;
        }
        const StreamHeader hd = decode_header(conf);
        const uint32_t W = 1u << hd.wbits;

        for (;;) {  // decompressor.c:431-575
            if (!(r.ip < n || r.nb || ts != kTokNone)) break;
            if (op == cap) { res = kOutputFull; break; }
            r.refill();
            ExactTok t;
            if (ts != kTokNone) {  // the token an earlier call left (decompressor.c:441-460)
                const bool rle = ts == kTokRle;
                if (skip) {
                    t = {rle ? (uint32_t)kExRle : (uint32_t)kExExt, rle ? pend_off : pend_size, pend_off};
                    if (!rle && (pend_off >= W || pend_off + pend_size > W)) t.kind = kExOob;
                } else {
                    t = exact_payload(r, hd, rle, ts == kTokExtHaveSize ? 1 : 0, pend_size);
                }
                ts = kTokNone;
            } else {
                if (r.nb == 0) break;
                t = exact_token(r, hd);
            }
            if (t.kind == kExShort) break;
            if (t.kind == kExOob) { res = kOob; break; }
            if (t.kind == kExFlush) continue;
            // a token picked up again produces what it has not delivered yet (a literal never is: skip_bytes stays for the match)
            const uint32_t len = t.kind == kExLit ? 1u : t.len - skip;
            if (t.kind != kExLit) skip = 0;
            const uint32_t room = cap - op;
            op += len <= room ? len : room;
            if (len > room) { res = kOutputFull; break; }
        }
    } while (false);

    a.out_len[row] = op;
    a.status[row] = (int8_t)res;
    if (a.in_consumed) a.in_consumed[row] = r.ip;
}

// Wavefront w takes rows [w * spw, (w + 1) * spw), then those of w + (waves of the grid), ...: tamp_decode_parse_kernel<false>'s
// walk.  No LDS: the exact loop reads its input through RefReader's dword stage and the prefix code from the packed tables.
__global__ void __launch_bounds__(256) tamp_decoded_size_pieces_kernel(SizePiecesArgs a) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t stride = gridDim.x * (blockDim.x >> 6);
    for (uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; (uint64_t)wave * a.spw < a.n_rows; wave += stride) {
        const uint64_t row = (uint64_t)wave * a.spw + lane;
        if (lane < a.spw && row < a.n_rows) size_piece(a, (uint32_t)row);
    }
}

}  // namespace tamp_amd
