// tamp_decode_common.hpp -- format facts every decoder shares: the stream header, the prefix-code decode, and the
// reference's bit reader (the exact loops of the lane decoder and the split parse) with the split parse's exact token step.
//
// Restated from the reference (tamp/_c_src/tamp/decompressor.c): header :276-297,304-329, bit refill :357-365,
// prefix code :52-104, token loop :431-575 with RLE / extended-match payloads :114-273.
#pragma once
#include "tamp_common.hpp"

namespace tamp_amd {

// The first header byte (decompressor.c:276-297).  Validity checks stay with the callers: the window bound, the second
// header byte and the custom-dictionary length are reported differently by each of them.
struct StreamHeader {
    uint32_t wbits, lbits;
    bool custom, extended, dreset;
    uint32_t table;  // seeded dictionary: literal <= 5, == 6, >= 7 (v1 streams: the last one, decompressor.c:318-319)
    uint32_t minp;   // min_pattern_size
};
__host__ __device__ inline StreamHeader decode_header(uint32_t h0) {
    StreamHeader h;
    h.wbits = ((h0 >> 5) & 7) + 8;
    h.lbits = ((h0 >> 3) & 3) + 5;
    h.custom = (h0 >> 2) & 1;
    h.extended = (h0 >> 1) & 1;
    h.dreset = h0 & 1;
    h.table = (!h.extended || h.lbits >= 7) ? 2u : (h.lbits == 6 ? 1u : 0u);
    h.minp = (uint32_t)min_pattern_size((int)h.wbits, (int)h.lbits);
    return h;
}

// The custom dictionary of stream `s`, whose header asks for one: the call's buffer, or -- with a table (the *_dicts calls) -- the
// W bytes at dict_off[s] of it.  -> kOk and *off, or the stream's status: kBadArgument for a misaligned row, kInvalidConf where
// W bytes are not there (what too short a shared dictionary gets, decompressor.c:304-329).  `have`: a buffer was passed (the
// size query has its length alone).  Nothing is read through a refused row.
__device__ __forceinline__ int custom_dict_offset(bool have, uint64_t dict_len, const uint64_t* dict_off, uint32_t s, uint32_t W, uint64_t* off) {
    const uint64_t o = dict_off ? dict_off[s] : 0;
    *off = o;
    if (!dict_off_aligned(o)) return kBadArgument;  // (a call without a table: o = 0)
    return (have && dict_off_in_bounds(o, W, dict_len)) ? kOk : kInvalidConf;
}

// Prefix-code LUT, 128 bytes: index = the 7 bits after the leading 1 of a code word -> (extra bits << 4) | symbol
// (decompressor.c:52-57 restated from the code table).  Filled by the whole workgroup; the caller synchronises.
__device__ __forceinline__ void build_prefix_lut(uint8_t* lut) {
    for (uint32_t v = threadIdx.x; v < 128; v += blockDim.x) {
        uint32_t entry = 0;
        for (uint32_t s = 1; s < 15; s++) {
            const uint32_t l = tok_nbits(s) - 1u;  // code length without the flag: 2..8
            // code = 1 followed by (l-1) bits; compare those with the top (l-1) bits of v
            if ((tok_code(s) & ((1u << (l - 1)) - 1)) == (v >> (7 - (l - 1)))) entry = ((l - 1) << 4) | s;
        }
        lut[v] = (uint8_t)entry;
    }
}

// Prefix-code reader for the symbol that follows the 0 flag (decompressor.c:52-104).  `b` holds the
// upcoming bits left-aligned; returns the symbol and its code length, or -1 when `avail` is too small.
__device__ __forceinline__ int read_symbol(uint32_t b, uint32_t avail, uint32_t& used) {
    if (avail < 1) return -1;
    if ((b >> 31) == 0) {
        used = 1;
        return 0;
    }
    // code words (without the flag) are 2..8 bits; walk them from the packed tables
    int sym = -1;
    uint32_t nb = 0;
#pragma unroll
    for (uint32_t s = 1; s < 15; s++) {
        const uint32_t l = tok_nbits(s) - 1u;
        if (sym < 0 && (b >> (32 - l)) == tok_code(s)) {
            sym = (int)s;
            nb = l;
        }
    }
    if (avail < nb) return -1;
    used = nb;
    return sym;
}

// The reference's bit reader: `bb`/`nb` behave exactly like its 32-bit buffer (decompressor.c:357-365) -- it decides
// status and consumed count on truncated input; bytes are fetched a dword at a time into `stage` (`ns` of them, the next
// one in the low byte).  `ip` = input bytes pulled into the buffer = the consumed count.  Shared by the exact loops of the
// lane decoder and the split parse.
struct RefReader {
    const uint8_t* in;
    uint32_t n;
    uint32_t ip = 0, bb = 0, nb = 0, stage = 0, ns = 0;

    __device__ __forceinline__ void refill() {
        while (ip < n && nb <= 24) {
            if (ns == 0) {
                const uint8_t* p = in + ip;
                if ((reinterpret_cast<uintptr_t>(p) & 3) == 0 && ip + 4 <= n) {
                    stage = *reinterpret_cast<const uint32_t*>(p);
                    ns = 4;
                } else {
                    stage = *p;
                    ns = 1;
                }
            }
            nb += 8;
            bb |= (stage & 0xFFu) << (32 - nb);
            stage >>= 8;
            ns--;
            ip++;
        }
    }
    // The buffer at a token boundary T (bits from the start of the stream) after a path that tracks bit positions only:
    // everything the reference's most recent refill, at bit position T_mark, pulled in.
    __device__ __forceinline__ void rebuild(uint32_t T, uint32_t T_mark) {
        const uint32_t ip_ref = min(n, ((T_mark + 24) >> 3) + 1);
        bb = 0, nb = 0, stage = 0, ns = 0;
        for (uint32_t b = T >> 3; b < ip_ref; b++) {
            uint32_t byte = in[b], width = 8;
            if (b == (T >> 3)) byte &= 0xFFu >> (T & 7), width = 8 - (T & 7);
            bb |= byte << (32 - nb - width);
            nb += width;
        }
        ip = ip_ref;
    }
};

// What one exact token step decoded.  kExShort: not enough bits (the stream ends here, nothing committed that matters);
// kExOob: a match outside the window.  len = bytes the token produces; arg = the literal byte or the match offset.
enum : uint32_t { kExLit, kExFlush, kExRle, kExExt, kExMatch, kExShort, kExOob };
struct ExactTok {
    uint32_t kind, len, arg;
};

// One token of the reference's loop (decompressor.c:448-572) from a buffer refilled at the top of the token (nb > 0).
// Consumes the token's bits as the reference does -- FLUSH aligns to a byte, RLE / extended payloads refill and retry
// -- and returns it; what to do with it (output room, window, a dictionary reset) is the caller's.  The split parse's
// exact loop; the lane decoder's keeps the same rules inline (tamp_decompress_kernel.hpp says why).
__device__ __forceinline__ ExactTok exact_token(RefReader& r, const StreamHeader& h) {
    const uint32_t W = 1u << h.wbits;
    if (r.bb >> 31) {  // literal, decompressor.c:466-482
        if (r.nb < 1 + h.lbits) return {kExShort, 0, 0};
        const uint32_t c = (r.bb << 1) >> (32 - h.lbits);
        r.bb <<= 1 + h.lbits;
        r.nb -= 1 + h.lbits;
        return {kExLit, 1, c};
    }

    uint32_t b2 = r.bb << 1, n2 = r.nb - 1, used = 0;
    const int sym = read_symbol(b2, n2, used);
    if (sym < 0) return {kExShort, 0, 0};
    b2 <<= used;
    n2 -= used;

    if (sym == kSymFlush) {  // decompressor.c:501-514
        r.bb = b2 << (n2 & 7);
        r.nb = n2 & ~7u;
        return {kExFlush, 0, 0};
    }

    if (h.extended && sym >= kSymRle) {
        r.bb = b2;  // symbol bits are committed before the payload is read (decompressor.c:521-526)
        r.nb = n2;
        const uint32_t trailing = (sym == kSymRle) ? 4u : 3u;
        uint32_t value = 0, match_len = 0, off = 0;
        int got = 0;
        for (;;) {  // decode_rle / decode_extended_match with the loop's refill-and-retry (:114-273,447-456)
            if (got == 0) {
                uint32_t u3 = 0;
                int hsym = (r.nb >= 1 + trailing) ? read_symbol(r.bb, r.nb, u3) : -1;
                if (hsym >= 0 && r.nb - u3 < trailing) hsym = -1;
                if (hsym >= 0) {
                    uint32_t b3 = r.bb << u3;
                    value = ((uint32_t)hsym << trailing) + (b3 >> (32 - trailing));
                    r.bb = b3 << trailing;
                    r.nb -= u3 + trailing;
                    got = (sym == kSymRle) ? 2 : 1;
                    if (sym == kSymExt) match_len = value + h.minp + 12;
                }
            }
            if (got == 1 && r.nb >= h.wbits) {
                off = r.bb >> (32 - h.wbits);
                r.bb <<= h.wbits;
                r.nb -= h.wbits;
                got = 2;
            }
            if (got == 2) break;
            const uint32_t before = r.nb;
            r.refill();
            if (r.nb == before && r.ip == r.n) return {kExShort, 0, 0};  // starved
        }
        if (sym == kSymRle) return {kExRle, value + 2, 0};  // decompressor.c:140-173
        if (off >= W || off + match_len > W) return {kExOob, 0, 0};  // decompressor.c:229-236
        return {kExExt, match_len, off};
    }

    // plain match, decompressor.c:529-572
    if (n2 < h.wbits) return {kExShort, 0, 0};
    const uint32_t match_len = (uint32_t)sym + h.minp;
    const uint32_t off = b2 >> (32 - h.wbits);
    if (off >= W || off + match_len > W) return {kExOob, 0, 0};
    r.bb = b2 << h.wbits;
    r.nb = n2 - h.wbits;
    return {kExMatch, match_len, off};
}

// The payload of an RLE / extended-match symbol whose bits are committed (decode_rle / decode_extended_match with the loop's
// refill-and-retry, decompressor.c:114-273,447-456).  `got` = 0: nothing of it read yet; 1: an extended match whose size
// `match_len` is known and whose offset is still to come (TOKEN_EXT_MATCH parked by an earlier call).  For a decoder that picks a token
// up where an earlier call left it (tamp_decoded_size_pieces_kernel.hpp).  exact_token above keeps these rules inline: called from
// there, this function cost the size-only parse two more spilled SGPRs, and its instruction stream is not to change.
// `parked` (may be null; the decoders that keep the object's state pass it): set where the reference parks the size of an extended
// match because its offset is not in the buffer yet (pending_match_size, decompressor.c:215-222), whatever becomes of the token.
__device__ __forceinline__ ExactTok exact_payload(RefReader& r, const StreamHeader& h, const bool rle, int got, uint32_t match_len,
                                                  uint32_t* parked = nullptr) {
    const uint32_t W = 1u << h.wbits;
    const uint32_t trailing = rle ? 4u : 3u;
    uint32_t value = 0, off = 0;
    for (;;) {
        if (got == 0) {
            uint32_t u3 = 0;
            int hsym = (r.nb >= 1 + trailing) ? read_symbol(r.bb, r.nb, u3) : -1;
            if (hsym >= 0 && r.nb - u3 < trailing) hsym = -1;
            if (hsym >= 0) {
                uint32_t b3 = r.bb << u3;
                value = ((uint32_t)hsym << trailing) + (b3 >> (32 - trailing));
                r.bb = b3 << trailing;
                r.nb -= u3 + trailing;
                got = rle ? 2 : 1;
                if (!rle) match_len = value + h.minp + 12;
            }
        }
        if (got == 1 && r.nb >= h.wbits) {
            off = r.bb >> (32 - h.wbits);
            r.bb <<= h.wbits;
            r.nb -= h.wbits;
            got = 2;
        } else if (got == 1 && parked) {
            *parked = match_len;
        }
        if (got == 2) break;
        const uint32_t before = r.nb;
        r.refill();
        if (r.nb == before && r.ip == r.n) return {kExShort, 0, 0};  // starved
    }
    if (rle) return {kExRle, value + 2, 0};  // decompressor.c:140-173
    if (off >= W || off + match_len > W) return {kExOob, 0, 0};  // decompressor.c:229-236
    return {kExExt, match_len, off};
}

// exact_token for a decoder that keeps the object's state (tamp_seek_kernel.hpp): the same token of the reference's loop from a
// buffer refilled at its top, with the payload of an RLE / extended symbol read by exact_payload, so that `parked` tells what the
// reference left in pending_match_size on the way.  A plain match is consumed here; the reference keeps such a token in its buffer
// until it is delivered, so a caller that needs the buffer of that moment copies bb / nb in front of the call.
__device__ __forceinline__ ExactTok exact_token_state(RefReader& r, const StreamHeader& h, uint32_t* parked) {
    const uint32_t W = 1u << h.wbits;
    if (r.bb >> 31) {  // literal, decompressor.c:466-482
        if (r.nb < 1 + h.lbits) return {kExShort, 0, 0};
        const uint32_t c = (r.bb << 1) >> (32 - h.lbits);
        r.bb <<= 1 + h.lbits;
        r.nb -= 1 + h.lbits;
        return {kExLit, 1, c};
    }
    uint32_t b2 = r.bb << 1, n2 = r.nb - 1, used = 0;
    const int sym = read_symbol(b2, n2, used);
    if (sym < 0) return {kExShort, 0, 0};
    b2 <<= used;
    n2 -= used;
    if (sym == kSymFlush) {  // decompressor.c:501-514
        r.bb = b2 << (n2 & 7);
        r.nb = n2 & ~7u;
        return {kExFlush, 0, 0};
    }
    if (h.extended && sym >= kSymRle) {  // symbol bits are committed before the payload is read (decompressor.c:521-526)
        r.bb = b2;
        r.nb = n2;
        return exact_payload(r, h, sym == kSymRle, 0, 0, parked);
    }
    if (n2 < h.wbits) return {kExShort, 0, 0};  // plain match, decompressor.c:529-572
    const uint32_t match_len = (uint32_t)sym + h.minp;
    const uint32_t off = b2 >> (32 - h.wbits);
    if (off >= W || off + match_len > W) return {kExOob, 0, 0};
    r.bb = b2 << h.wbits;
    r.nb = n2 - h.wbits;
    return {kExMatch, match_len, off};
}

}  // namespace tamp_amd
