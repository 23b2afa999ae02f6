// tamp_seek_kernel.hpp -- a SEEK INDEX for streams that have no dictionary resets (tamp_batch_seek_index,
// tamp_batch_read_ranges_seek; DESIGN.md 3.13 "Reading ranges by checkpoint").
//
// A checkpoint is the reference's decoder object (TampAmdDecoderState + window, the row format of tamp_decompress_resume_kernel.hpp)
// after k calls of tamp_decompressor_decompress with exactly `interval` bytes of room each, next to the input bytes those calls
// consumed.  Its decoded position is exactly k * interval -- inside an RLE run, an extended match or a plain match if that is where
// the room ran out -- so begin / interval is an address.
//   tamp_seek_index_kernel   a wavefront per stream: decodes with the window in LDS and no output at all, and stores a row each time
//                            the decoded count reaches a multiple of the interval with a byte still to come
//   tamp_seek_extend_kernel  the same loop for streams that have GROWN (tamp_batch_seek_index_extend): entered at the stream's
//                            restart row, the last row whose in_pos is smaller than the last row's, and writing the rows behind it
//   tamp_seek_count_kernel   a lane per range, the shared tile scan: the range's verdict and units, their exclusive scan
//   tamp_seek_units_kernel   a lane per unit (range x checkpoint interval): owner by binary search, the checks of the row it
//                            starts at, its 40-byte record
//   tamp_read_seek_kernel    a wavefront per unit: row -> LDS, the pending token picked up, the bytes in front of the range
//                            discarded, the others through the 256-byte stage to their place in the caller's buffer
//   tamp_seek_gather_kernel  a lane per range: out_len and status from what its units added up
// A host-memory read plans on the host with the same two functions (seek_range_plan, seek_range_unit) and uploads the touched rows
// and compressed spans only.
//
// Both decoders are the reference's own loop over RefReader / exact_token_state / exact_payload (tamp_decode_common.hpp): its 32-bit
// buffer is simulated bit for bit, so a row's bit_buffer, bit_buffer_pos and in_pos are read off the reader and not derived.  The
// token loop is wave-uniform; the 64 lanes do the window copies, the row stores and the output.
#pragma once
#include "tamp_decode_common.hpp"
#include "tamp_decompress_resume_kernel.hpp"
#include "tamp_reset_segments_kernel.hpp"

namespace tamp_amd {

constexpr uint32_t kSeekMaxIn = kMaxDecodeIn - 512;  // streams of this many compressed bytes or more: kBadArgument (tamp_batch_read_ranges's bound)
constexpr int32_t kSeekGo = 1;                       // a range's verdict: it has units
constexpr int32_t kSeekBadIndex = -22;               // TAMP_AMD_BAD_INDEX
constexpr uint32_t kSeekFresh = 0xFFFFFFFFu;         // a unit's row: none, it starts at the stream's header
constexpr uint32_t kSeekSawOob = 1, kSeekSawBad = 2; // a range's flags word

__host__ __device__ inline uint32_t seek_wave_lds(uint32_t max_wbits, uint32_t waves) { return waves * ((1u << max_wbits) + kStage); }

// The four state words of a row (layout: tamp_decompress_resume_kernel.hpp).
struct SeekWords { uint32_t w0, w1, w2, w3; };
__host__ __device__ inline SeekWords seek_pack(uint32_t bb, uint32_t nb, uint32_t wp, uint32_t ts, uint32_t pend_off, uint32_t pend_size,
                                               uint32_t conf, uint32_t skip, uint32_t flags, uint32_t bits_max) {
    return {nb ? bb & (0xFFFFFFFFu << (32 - nb)) : 0u, (wp & 0xFFFFu) | (nb << 16) | (ts << 24), (pend_off & 0xFFFFu) | (pend_size << 16),
            (conf & 0xFFu) | ((skip & 0xFFu) << 8) | ((flags & 0xFFu) << 16) | (bits_max << 24)};
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The window side of a token, as the resume kernel applies it (decompressor.c:160-170, 262-270, 568-572).
__device__ __forceinline__ void seek_window_match(uint8_t* win, uint32_t& wp, uint32_t off, uint32_t len, uint32_t mask, uint32_t lane) {
    uint32_t b = 0;  // (len <= 18: one chunk, sources read before the stores: memmove)
    if (lane < len) b = win[off + lane];
    __builtin_amdgcn_wave_barrier();
    if (lane < len) win[(wp + lane) & mask] = (uint8_t)b;
    __builtin_amdgcn_wave_barrier();
    wp = (wp + len) & mask;
}
__device__ __forceinline__ void seek_window_rle(uint8_t* win, uint32_t& wp, uint32_t c, uint32_t count, uint32_t W, uint32_t lane) {
    const uint32_t ww = min(min(count, kRleWindowMax), W - wp);  // first piece only, at most 8 bytes, no wrap
    if (lane < ww) win[wp + lane] = (uint8_t)c;
    __builtin_amdgcn_wave_barrier();
    wp = (wp + ww) & (W - 1);
}
__device__ __forceinline__ void seek_window_ext(uint8_t* win, uint32_t& wp, uint32_t off, uint32_t count, uint32_t W, uint32_t lane) {
    const uint32_t mask = W - 1, ww = min(count, W - wp);  // the complete token only, up to the end of the buffer
    const uint32_t dist = (wp - off) & mask;
    const bool reverse = dist > 0 && dist < ww;
    const uint32_t nchunks = (ww + 63) >> 6;
    for (uint32_t ci = 0; ci < nchunks; ci++) {
        const uint32_t base = (reverse ? nchunks - 1 - ci : ci) << 6;
        uint32_t b = 0;
        if (base + lane < ww) b = win[off + base + lane];
        __builtin_amdgcn_wave_barrier();
        if (base + lane < ww) win[wp + base + lane] = (uint8_t)b;
        __builtin_amdgcn_wave_barrier();
    }
    wp = (wp + ww) & mask;
}
__device__ __forceinline__ void seek_load_window(uint8_t* win, const uint8_t* src, uint32_t W, uint32_t lane) {
    __builtin_amdgcn_wave_barrier();
    if ((reinterpret_cast<uintptr_t>(src) & 3) == 0) {
        for (uint32_t k = lane * 4; k < W; k += 256) *reinterpret_cast<uint32_t*>(win + k) = *reinterpret_cast<const uint32_t*>(src + k);
    } else {
        for (uint32_t k = lane; k < W; k += 64) win[k] = src[k];
    }
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The checks of a row that decoding starts at -- a unit of a read, the restart row of an extension: row `row` of the tables is row r
// of a stream of n compressed bytes whose header has hs bytes, the first of them h0.
__host__ __device__ inline bool seek_row_holds(const uint32_t* ckpt_in, const uint8_t* states, uint64_t stride, uint64_t row, uint64_t r,
                                               uint32_t n, uint32_t hs, uint32_t h0) {
    const uint32_t start = ckpt_in[row];
    if (start < hs || start > n) return false;
    // (the row in front of it, where that one's entry can be one at all: an entry beyond the stream spoils its own row only)
    if (r >= 1 && ckpt_in[row - 1] > start && ckpt_in[row - 1] <= n) return false;
    const uint8_t* const sp = states + row * stride;
    uint32_t w[4];
    for (int b = 0; b < 4; b++) w[b] = (uint32_t)sp[4 * b] | (uint32_t)sp[4 * b + 1] << 8 | (uint32_t)sp[4 * b + 2] << 16 | (uint32_t)sp[4 * b + 3] << 24;
    const uint32_t wp = w[1] & 0xFFFFu, nb = (w[1] >> 16) & 0xFFu, ts = w[1] >> 24;
    const uint32_t pend_off = w[2] & 0xFFFFu, pend_size = w[2] >> 16;
    const uint32_t conf = w[3] & 0xFFu, skip = (w[3] >> 8) & 0xFFu, flags = (w[3] >> 16) & 0xFFu;
    const uint32_t W = 1u << decode_header(h0).wbits;
    if (conf != h0) return false;
    if ((flags & (kDsConfigured | kDsHeaderStashed)) != kDsConfigured) return false;
    if (ts != kTokNone && ts != kTokRle && ts != kTokExtHaveSize) return false;
    if (wp >= W || nb > 32) return false;
    // a token in delivery: what it still holds must lie inside the window and inside itself
    if (ts == kTokRle && skip > pend_off) return false;
    if (ts == kTokExtHaveSize && skip && (pend_off >= W || pend_off + pend_size > W || skip > pend_size)) return false;
    return true;
}

// The RESTART ROW of a stream that holds `have` rows (tamp_batch_seek_index_extend): the last of them whose in_pos is smaller than
// the last row's.  -> how many rows are final (the restart row and those in front of it; 0: restart from the header), or
// kSeekBadRestart when a row between the two lies beyond the stream's n bytes: no index of a prefix of the stream looks so.
constexpr uint32_t kSeekBadRestart = 0xFFFFFFFFu;
__host__ __device__ inline uint32_t seek_restart_rows(const uint32_t* in_pos, uint32_t have, uint32_t n) {
    if (have < 2) return 0;
    const uint32_t last = in_pos[have - 1];
    for (uint32_t r = have - 1; r-- > 0;) {
        if (in_pos[r] < last) return r + 1;
        if (in_pos[r] > n) return kSeekBadRestart;
    }
    return 0;
}

struct SeekIndexArgs {
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    const uint8_t* dict;  // the call's one custom dictionary (null: none)
    uint64_t dict_len;
    const uint8_t* seed_dicts;
    const uint64_t* ckpt_first;  // n + 1: the rows each stream has room for, as a running sum
    uint32_t* ckpt_in;
    uint8_t* ckpt_state;
    uint64_t state_stride;
    uint64_t* decoded_size;
    int8_t* status;
    uint32_t interval, max_wbits, n_streams;
};
// What an extension adds.  A device-memory call gives `have` alone: the rows each stream holds, and the wavefront finds and checks
// its restart row itself.  A host-memory call has done both on the host (restart_state is not null then): have[s] is the number of
// FINAL rows (kSeekBadRestart: the restart row did not hold up), the tables hold the stream's rows BEHIND those, `in` its compressed
// bytes from byte in_base[s] on -- the restart row's in_pos, or 0 -- and row slot[s] of restart_state is the restart row.
struct SeekExtendArgs {
    SeekIndexArgs x;
    const uint32_t* have;
    const uint32_t* in_base;
    const uint32_t* slot;
    const uint8_t* restart_state;
};

// The index loop, a wavefront per stream.  kExtend: entered at the restart row, the way tamp_read_seek_kernel enters its own loop at
// a unit's row; without it `e` is not looked at and every stream starts at its header.
template <bool kExtend>
__device__ __forceinline__ void seek_index_streams(const SeekIndexArgs& a, const SeekExtendArgs* e) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    const uint32_t wave = uni32(threadIdx.x >> 6);
    uint8_t* const win = smem + wave * ((1u << a.max_wbits) + kStage);
    const uint32_t gw = blockIdx.x * nwaves + wave, tw = gridDim.x * nwaves;
    const uint64_t N = a.interval;

    for (uint32_t s = gw; s < a.n_streams; s += tw) {
        const bool staged = kExtend && e->restart_state != nullptr;
        const uint32_t in_base = staged ? uni32(e->in_base[s]) : 0u;  // the stream's bytes in front of `in`
        const uint8_t* const in = a.in + a.in_off[s];
        const uint32_t n = uni32(a.in_len[s]);
        const uint64_t f0 = a.ckpt_first[s], f1 = a.ckpt_first[s + 1];
        uint64_t row_base = 0;                        // the stream's rows in front of its rows of the tables (staged: the final ones)
        uint64_t room = f1 > f0 ? f1 - f0 : 0;        // rows [row_base, room) of the stream may be written
        uint64_t pos = 0, next = N, krow = 0;         // decoded bytes; the next multiple of the interval; rows so far (stored or not)
        int res = kInputExhausted;

        do {
            if (n >= kSeekMaxIn) { res = kBadArgument; break; }
            if (a.max_wbits < 8 || a.max_wbits > 15) { res = kInvalidConf; break; }
            if (n == 0) break;
            uint32_t final_rows = kExtend ? uni32(e->have[s]) : 0u;  // rows [0, final_rows) stand as they are; the last is the restart row
            const uint8_t* restart_row = nullptr;
            uint32_t h0, hs;
            if (in_base == 0) {
                h0 = uni32(in[0]);
                hs = 1 + (h0 & 1);
                if (n < hs) break;
                if (hs == 2 && uni32(in[1])) { res = kInvalidConf; break; }
            } else {  // (the host saw the header; the restart row carries its first byte)
                if (final_rows == 0 || final_rows == kSeekBadRestart || n < in_base) { res = kSeekBadIndex; break; }
                h0 = uni32(e->restart_state[uni32(e->slot[s]) * a.state_stride + 12]);
                hs = 1 + (h0 & 1);
            }
            const StreamHeader hd = decode_header(h0);
            if (hd.wbits > a.max_wbits) { res = kInvalidConf; break; }
            const uint32_t W = 1u << hd.wbits, mask = W - 1;
            const uint8_t* const seed_default = a.seed_dicts + ((size_t)hd.table << 15);
            const uint8_t* seed = seed_default;
            if (hd.custom) {
                if (!a.dict || a.dict_len < W) { res = kInvalidConf; break; }
                seed = a.dict;
            }
            uint32_t start = 0;  // the restart row's in_pos
            if (kExtend && staged) {
                if (final_rows && final_rows != kSeekBadRestart) {
                    restart_row = e->restart_state + uni32(e->slot[s]) * a.state_stride;
                    start = in_base, row_base = final_rows, room += row_base;
                }
            } else if (kExtend && final_rows) {  // the rule, 64 rows a step from the last one down, and the restart row's checks
                uint32_t found = kSeekBadRestart;
                if (final_rows <= room) {
                    const uint32_t* const rows_in = a.ckpt_in + f0;
                    const uint32_t last = uni32(rows_in[final_rows - 1]);
                    uint32_t top = final_rows - 1;  // rows [0, top) are still to be looked at
                    found = 0;
                    while (top && !found) {
                        const bool live = lane < top;
                        const uint32_t v = live ? rows_in[top - 1 - lane] : last;
                        const uint64_t lower = __ballot(live && v < last), other = __ballot(live && v > n);
                        if (other & ((lower & (0 - lower)) - 1)) found = kSeekBadRestart;  // (behind the restart row: none beyond the stream)
                        else if (lower) found = top - (uint32_t)(__ffsll((unsigned long long)lower) - 1);
                        else top = top > 64 ? top - 64 : 0;
                    }
                    found = uni32(found);
                    if (found && found != kSeekBadRestart && !seek_row_holds(a.ckpt_in, a.ckpt_state, a.state_stride, f0 + found - 1, found - 1, n, hs, h0))
                        found = kSeekBadRestart;
                }
                final_rows = found;
                if (final_rows && final_rows != kSeekBadRestart) {
                    restart_row = a.ckpt_state + (f0 + final_rows - 1) * a.state_stride;
                    start = uni32(a.ckpt_in[f0 + final_rows - 1]);
                }
            }
            if (kExtend && final_rows == kSeekBadRestart) { res = kSeekBadIndex; break; }

            RefReader r{in, n - in_base};
            r.ip = hs;
            uint32_t wp = 0, pend_off = 0, pend_size = 0;
            uint32_t row_ts = kTokNone, row_skip = 0;  // the token the restart row lies in
            if (kExtend && restart_row) {
                const uint32_t* const sw = reinterpret_cast<const uint32_t*>(restart_row);
                const uint32_t s0 = uni32(sw[0]), s1 = uni32(sw[1]), s2 = uni32(sw[2]), s3 = uni32(sw[3]);
                const uint32_t carried = min((s1 >> 16) & 0xFFu, 32u);
                wp = s1 & 0xFFFFu & mask, row_ts = s1 >> 24;
                pend_off = s2 & 0xFFFFu, pend_size = s2 >> 16;
                row_skip = (s3 >> 8) & 0xFFu;
                if (carried) r.bb = s0 & (0xFFFFFFFFu << (32 - carried)), r.nb = carried;
                r.ip = start - in_base;
                seek_load_window(win, restart_row + 16, W, lane);
                krow = final_rows, pos = krow * N, next = pos + N;
            } else {
                seek_load_window(win, seed, W, lane);
            }

            bool last_flush = false;
            // a checkpoint at a token boundary waits until a byte behind it is certain: its words, and the window as it stands
            bool waiting = false;
            SeekWords held = {0, 0, 0, 0};
            uint32_t held_in = 0;
            auto store_row = [&](const SeekWords& w, uint32_t in_pos) {
                if (krow < room && (!kExtend || krow >= row_base)) {
                    uint8_t* const row = a.ckpt_state + (f0 + krow - row_base) * a.state_stride;
                    __builtin_amdgcn_wave_barrier();
                    for (uint32_t k = lane * 16; k < W; k += 1024)
                        *reinterpret_cast<uint4*>(row + 16 + k) = *reinterpret_cast<const uint4*>(win + k);
                    if (lane == 0) {
                        *reinterpret_cast<uint4*>(row) = make_uint4(w.w0, w.w1, w.w2, w.w3);
                        a.ckpt_in[f0 + krow - row_base] = in_pos + in_base;
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                krow++;
            };
            auto release = [&]() {
                if (waiting) store_row(held, held_in), waiting = false;
            };
            // bytes [done, len) of the token at hand are delivered from `pos` on; each multiple of the interval INSIDE it is a row
            // What the reference's buffer holds meanwhile: a plain match stays in it until it is delivered (pre_bb / pre_nb: the buffer
            // in front of the token); an RLE run or extended match has left it, and the call that picks the token up refills first
            // (decompressor.c:437), so every row behind the first one inside such a token sees that refill.
            auto inside = [&](uint32_t len, uint32_t done, uint32_t ts, uint32_t pre_bb, uint32_t pre_nb) {
                const bool plain = ts == kTokNone;
                while ((uint64_t)(len - done) > next - pos) {
                    done += (uint32_t)(next - pos);
                    pos = next, next += N;
                    store_row(seek_pack(plain ? pre_bb : r.bb, plain ? pre_nb : r.nb, wp, ts, pend_off, pend_size, h0, done, kDsConfigured, a.max_wbits), r.ip);
                    if (!plain) r.refill();
                }
                pos += len - done;
            };
            // a token that delivers bytes, `done` of them in front of the restart row already (their side of the window with them)
            auto deliver = [&](const ExactTok& t, uint32_t done, uint32_t pre_bb, uint32_t pre_nb) {
                if (t.kind == kExLit) {
                    if (lane == 0) win[wp] = (uint8_t)t.arg;
                    wp = (wp + 1) & mask;
                    pos++;
                } else if (t.kind == kExRle) {
                    if (!done) {
                        const uint32_t c = uni32(win[(wp - 1) & mask]);
                        seek_window_rle(win, wp, c, t.len, W, lane);
                        if ((uint64_t)t.len > next - pos) pend_off = t.len;  // (what a partial run parks, decompressor.c:143-148)
                    }
                    inside(t.len, done, kTokRle, r.bb, r.nb);
                } else if (t.kind == kExExt) {
                    if (!done && (uint64_t)t.len > next - pos) pend_off = t.arg, pend_size = t.len;  // (decompressor.c:243-249)
                    inside(t.len, done, kTokExtHaveSize, r.bb, r.nb);
                    seek_window_ext(win, wp, t.arg, t.len, W, lane);
                } else {
                    inside(t.len, done, kTokNone, pre_bb, pre_nb);  // (the token stays in the buffer until it is delivered, :555-562)
                    seek_window_match(win, wp, t.arg, t.len, mask, lane);
                }
                if (pos == next) {  // a boundary: the object as the call that filled its room left it
                    held = seek_pack(r.bb, r.nb, wp, kTokNone, pend_off, pend_size, h0, 0, kDsConfigured, a.max_wbits);
                    held_in = r.ip, waiting = true;
                    next += N;
                }
            };

            if (kExtend && (row_ts != kTokNone || row_skip)) {  // the token the restart row lies in (decompressor.c:441-460)
                ExactTok t;
                const uint32_t pre_bb = r.bb, pre_nb = r.nb;  // (a plain match: the row's buffer is the one in front of it)
                if (row_ts != kTokNone) {
                    const bool rle = row_ts == kTokRle;
                    r.refill();  // (the call that picks such a token up refills first)
                    if (row_skip) {
                        t = {rle ? (uint32_t)kExRle : (uint32_t)kExExt, rle ? pend_off : pend_size, pend_off};
                        if (!rle && (pend_off >= W || pend_off + pend_size > W)) t.kind = kExOob;
                    } else {
                        uint32_t parked = 0;
                        t = exact_payload(r, hd, rle, row_ts == kTokExtHaveSize ? 1 : 0, pend_size, &parked);
                        if (parked) pend_size = parked;
                    }
                } else {
                    t = exact_token_state(r, hd, nullptr);
                    if (t.kind != kExMatch) t.kind = kExOob;
                }
                // (a row that the checks let through and that no index of this stream holds: the token is not the one it names)
                if (t.kind == kExOob || row_skip > t.len) { res = kSeekBadIndex, pos = 0; break; }
                if (t.kind == kExShort) break;
                deliver(t, row_skip, pre_bb, pre_nb);
            }

            for (;;) {  // decompressor.c:431-575
                if (!(r.ip < r.n || r.nb)) break;
                r.refill();
                if (r.nb == 0) break;
                const uint32_t pre_bb = r.bb, pre_nb = r.nb;
                uint32_t parked = 0;
                const ExactTok t = exact_token_state(r, hd, &parked);
                if (parked) pend_size = parked;
                if (t.kind == kExShort) break;
                if (t.kind == kExOob) { res = kOob; break; }
                if (t.kind == kExFlush) {
                    if (hd.dreset && last_flush) {
                        release();  // (the row's window is the one in front of the reset)
                        wp = 0;
                        seek_load_window(win, seed_default, W, lane);
                    }
                    last_flush = true;
                    continue;
                }
                last_flush = false;
                release();
                deliver(t, 0, pre_bb, pre_nb);
            }
        } while (false);

        if (lane == 0) a.decoded_size[s] = pos, a.status[s] = (int8_t)res;
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ void __launch_bounds__(256) tamp_seek_index_kernel(SeekIndexArgs a) { seek_index_streams<false>(a, nullptr); }

// tamp_batch_seek_index_extend: the same loop from each stream's restart row on.
__global__ void __launch_bounds__(256) tamp_seek_extend_kernel(SeekExtendArgs e) { seek_index_streams<true>(e.x, &e); }

// ---------------------------------------------------------------------------------------------------------------------------------
// Planning a read: host and device run the same two functions.
struct SeekCaller {
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    uint64_t n;
    uint64_t dict_len;  // 0: no custom dictionary with the call
    const uint64_t* first;
    const uint32_t* ckpt_in;
    const uint8_t* states;
    uint64_t stride;
    uint32_t interval, max_wbits;
    const uint32_t* range_stream;
    const uint64_t* range_begin;
    const uint32_t* range_len;
    uint64_t n_ranges;
};

struct SeekPlan {
    int32_t verdict;  // kSeekGo, or the range's status as it stands
    uint64_t k0, units, rows;
    uint32_t hs;
};
__host__ __device__ inline SeekPlan seek_range_plan(const SeekCaller& c, uint64_t q) {
    SeekPlan p = {kBadArgument, 0, 0, 0, 0};
    const uint64_t i = c.range_stream[q];
    if (i >= c.n) return p;
    const uint32_t len = c.range_len[q];
    if (!len) { p.verdict = kOk; return p; }
    const uint32_t n = c.in_len[i];
    if (n >= kSeekMaxIn) return p;
    p.verdict = kInputExhausted;
    if (n == 0) return p;
    const uint8_t* const s = c.in + c.in_off[i];
    p.hs = 1 + (s[0] & 1);
    if (n < p.hs) return p;
    p.verdict = kInvalidConf;
    if (p.hs == 2 && s[1]) return p;
    const StreamHeader hd = decode_header(s[0]);
    if (hd.wbits > c.max_wbits || c.max_wbits > 15) return p;
    if (hd.custom && c.dict_len < (1ull << hd.wbits)) return p;
    p.verdict = kSeekBadIndex;
    const uint64_t f0 = c.first[i], f1 = c.first[i + 1];
    if (f1 < f0 || f1 > c.first[c.n]) return p;
    p.rows = f1 - f0;
    const uint64_t begin = c.range_begin[q], end = begin > ~0ull - len ? ~0ull : begin + len;
    p.k0 = begin / c.interval < p.rows ? begin / c.interval : p.rows;
    const uint64_t k1 = (end - 1) / c.interval < p.rows ? (end - 1) / c.interval : p.rows;
    p.units = k1 - p.k0 + 1;
    p.verdict = kSeekGo;
    return p;
}

// A unit: range q between two checkpoints.  It reads in_n bytes from in + in_at, starts from row `row` (kSeekFresh: at the header),
// drops `front` decoded bytes and writes the `want` behind them at out + out_off[q] + out_rel.
struct SeekUnit {
    uint64_t in_at, out_rel, front;
    uint32_t in_n, row, want, owner;
};
static_assert(sizeof(SeekUnit) == 40, "the unit table's rows");

// -> false: the row the unit starts at does not hold up (TAMP_AMD_BAD_INDEX for its range); nothing of `u` is to be used then.
__host__ __device__ inline bool seek_range_unit(const SeekCaller& c, uint64_t q, const SeekPlan& p, uint64_t j, SeekUnit& u) {
    const uint64_t i = c.range_stream[q], k = p.k0 + j, N = c.interval;
    const uint32_t len = c.range_len[q], n = c.in_len[i];
    const uint64_t begin = c.range_begin[q], end = begin > ~0ull - len ? ~0ull : begin + len;
    const uint64_t f0 = c.first[i], pos0 = k * N;
    const uint64_t lo = begin > pos0 ? begin : pos0, hi = j + 1 == p.units ? end : (k + 1) * N;
    u.front = lo - pos0, u.want = (uint32_t)(hi - lo), u.out_rel = lo - begin, u.owner = (uint32_t)q;
    uint32_t start = 0;
    u.row = kSeekFresh;
    if (k) {
        const uint64_t row = f0 + k - 1;
        start = c.ckpt_in[row];
        if (!seek_row_holds(c.ckpt_in, c.states, c.stride, row, k - 1, n, p.hs, (c.in + c.in_off[i])[0])) return false;
        u.row = (uint32_t)row;
        if (row > 0xFFFFFFFEull) return false;
    }
    // the span ends where the next checkpoint's calls had consumed to; an entry that cannot be that is not used
    uint32_t stop = n;
    if (k < p.rows) {
        const uint32_t e = c.ckpt_in[f0 + k];
        if (e >= start && e <= n) stop = e;
    }
    u.in_at = c.in_off[i] + start, u.in_n = stop - start;
    return true;
}

struct SeekRanges {  // per range of the call, in the stream's scratch
    uint64_t* unit_first;  // n_ranges + 1
    uint32_t* got;         // bytes its units delivered
    uint32_t* flags;       // kSeekSaw...
    int8_t* verdict;
};

struct SeekCountArgs {
    SeekCaller c;
    SeekRanges r;
};
__global__ void __launch_bounds__(kResetScanTile) tamp_seek_count_kernel(SeekCountArgs a) {
    __shared__ uint64_t wave_sum[kResetScanTile / kWave];
    uint64_t units = 0;
    for (uint64_t t0 = 0; t0 < a.c.n_ranges; t0 += kResetScanTile) {  // (uniform bounds: every lane takes part in the shuffles)
        const uint64_t q = t0 + threadIdx.x;
        const bool live = q < a.c.n_ranges;
        SeekPlan p = {kOk, 0, 0, 0, 0};
        if (live) {
            p = seek_range_plan(a.c, q);
            a.r.verdict[q] = (int8_t)p.verdict, a.r.got[q] = 0, a.r.flags[q] = 0;
        }
        uint64_t tile;
        const uint64_t at = units + reset_tile_scan(live && p.verdict == kSeekGo ? p.units : 0, wave_sum, tile);
        units += tile;
        if (live) a.r.unit_first[q] = at;
    }
    if (threadIdx.x == 0) a.r.unit_first[a.c.n_ranges] = units;
}

struct SeekUnitsArgs {
    SeekCaller c;
    SeekRanges r;
    SeekUnit* units;
    uint64_t U;
};
__global__ void __launch_bounds__(256) tamp_seek_units_kernel(SeekUnitsArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.U) return;
    uint64_t lo = 0, hi = a.c.n_ranges;  // unit_first[lo] <= g < unit_first[hi] (ranges without units are stepped over)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.r.unit_first[mid] <= g) lo = mid;
        else hi = mid;
    }
    const uint64_t q = lo, j = g - a.r.unit_first[q];
    const SeekPlan p = seek_range_plan(a.c, q);
    SeekUnit u = {0, 0, 0, 0, kSeekFresh, 0, (uint32_t)q};
    const bool ok = p.verdict == kSeekGo && j < p.units && seek_range_unit(a.c, q, p, j, u);
    if (!ok) {
        u = {0, 0, 0, 0, kSeekFresh, 0, (uint32_t)q};  // (a unit that asks for nothing)
        atomicOr(&a.r.flags[q], kSeekSawBad);
    }
    a.units[g] = u;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct ReadSeekArgs {
    const uint8_t* in;
    const uint8_t* dict;
    uint64_t dict_len;
    const uint8_t* seed_dicts;
    const uint8_t* states;
    uint64_t stride;
    const SeekUnit* units;
    uint64_t U;
    uint32_t* got;
    uint32_t* flags;  // (complete when this kernel starts: the units step ran in front of it)
    uint8_t* out;
    const uint64_t* out_off;
    uint32_t max_wbits;
};

__global__ void __launch_bounds__(256) tamp_read_seek_kernel(ReadSeekArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    const uint32_t wave = uni32(threadIdx.x >> 6);
    uint8_t* const win = smem + wave * ((1u << a.max_wbits) + kStage);
    uint8_t* const stage = win + (1u << a.max_wbits);
    const uint64_t gw = (uint64_t)blockIdx.x * nwaves + wave, tw = (uint64_t)gridDim.x * nwaves;

    for (uint64_t x = gw; x < a.U; x += tw) {
        const SeekUnit* const up = a.units + x;
        const uint32_t want = uni32(up->want), q = uni32(up->owner), n = uni32(up->in_n), rowi = uni32(up->row);
        if (!want || (a.flags[q] & kSeekSawBad)) continue;  // (a range with a bad row writes nothing)
        const uint64_t front = up->front, stop = front + want;
        const uint8_t* const in = a.in + up->in_at;
        uint8_t* const out = a.out + a.out_off[q] + up->out_rel;
        uint32_t op = 0, flushed = 0;  // bytes of the range delivered by this unit: staged, stored
        uint64_t pos = 0;              // bytes decoded since the row
        bool oob = false;

        auto flush_stage = [&](bool all) {
            __builtin_amdgcn_wave_barrier();
            while (op - flushed >= 256 || (all && op > flushed)) {
                const uint32_t nbytes = min(op - flushed, 256u);
                uint8_t* dst = out + flushed;
                if ((reinterpret_cast<uintptr_t>(dst) & 3) == 0 && nbytes == 256) {
                    reinterpret_cast<uint32_t*>(dst)[lane] = *reinterpret_cast<const uint32_t*>(stage + ((flushed + 4 * lane) & (kStage - 1)));
                } else {
                    for (uint32_t k = lane; k < nbytes; k += 64) dst[k] = stage[(flushed + k) & (kStage - 1)];
                }
                flushed += nbytes;
            }
            __builtin_amdgcn_wave_barrier();
        };
        // lanes [0, count) hold the next `count` decoded bytes (count <= 64): those inside [front, stop) are the range's
        auto put = [&](uint32_t b, uint32_t count) {
            const uint64_t p0 = pos, p1 = pos + count;
            pos = p1;
            if (p1 <= front || p0 >= stop) return;
            const uint32_t j0 = p0 < front ? (uint32_t)(front - p0) : 0u, j1 = p1 > stop ? (uint32_t)(stop - p0) : count;
            if (lane >= j0 && lane < j1) stage[(op + lane - j0) & (kStage - 1)] = (uint8_t)b;
            op += j1 - j0;
            if (op - flushed >= 256) flush_stage(false);
        };

        do {
            RefReader r{in, n};
            uint32_t conf, wp = 0, ts = kTokNone, skip = 0, pend_off = 0, pend_size = 0;
            bool last_flush = false;
            const uint8_t* wsrc;
            if (rowi == kSeekFresh) {  // the stream's header: the plan saw it whole
                if (n == 0) break;
                conf = uni32(in[0]);
                r.ip = 1 + (conf & 1);
                if (n < r.ip) break;
                wsrc = nullptr;
            } else {
                const uint8_t* const row = a.states + (uint64_t)rowi * a.stride;
                const uint32_t* const sw = reinterpret_cast<const uint32_t*>(row);
                const uint32_t s0 = uni32(sw[0]), s1 = uni32(sw[1]), s2 = uni32(sw[2]), s3 = uni32(sw[3]);
                const uint32_t carried = min((s1 >> 16) & 0xFFu, 32u);
                wp = s1 & 0xFFFFu, ts = s1 >> 24;
                pend_off = s2 & 0xFFFFu, pend_size = s2 >> 16;
                conf = s3 & 0xFFu, skip = (s3 >> 8) & 0xFFu;
                last_flush = ((s3 >> 16) & kDsLastWasFlush) != 0;
                if (carried) r.bb = s0 & (0xFFFFFFFFu << (32 - carried)), r.nb = carried;
                wsrc = row + 16;
            }
            const StreamHeader hd = decode_header(conf);
            if (hd.wbits > a.max_wbits) break;
            const uint32_t W = 1u << hd.wbits, mask = W - 1;
            const uint8_t* const seed_default = a.seed_dicts + ((size_t)hd.table << 15);
            if (!wsrc) {
                wsrc = seed_default;
                if (hd.custom) {
                    if (!a.dict || a.dict_len < W) break;
                    wsrc = a.dict;
                }
            }
            wp &= mask;
            seek_load_window(win, wsrc, W, lane);

            for (;;) {  // decompressor.c:431-575, entered with a configured object
                if (pos >= stop) break;
                if (!(r.ip < n || r.nb || ts != kTokNone)) break;
                r.refill();
                ExactTok t;
                const uint32_t skip0 = skip;
                if (ts != kTokNone) {  // the token the checkpoint lies in (decompressor.c:441-460)
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
                    t = exact_token_state(r, hd, nullptr);
                }
                if (t.kind == kExShort) break;
                if (t.kind == kExOob) { oob = true; break; }
                if (t.kind == kExFlush) {
                    if (hd.dreset && last_flush) {
                        wp = 0;
                        seek_load_window(win, seed_default, W, lane);
                    }
                    last_flush = true;
                    continue;
                }
                last_flush = false;
                if (t.kind == kExLit) {  // (skip_bytes stays for the match it belongs to)
                    if (lane == 0) win[wp] = (uint8_t)t.arg;
                    wp = (wp + 1) & mask;
                    put(t.arg, 1);
                    continue;
                }
                skip = 0;
                const uint32_t rem = t.len > skip0 ? t.len - skip0 : 0;  // what the token has not delivered yet
                if (t.kind == kExRle) {
                    const uint32_t c = uni32(win[(wp - 1) & mask]);
                    if (skip0 == 0) seek_window_rle(win, wp, c, t.len, W, lane);
                    for (uint32_t base = 0; base < rem && pos < stop; base += 64) put(c, min(rem - base, 64u));
                } else {
                    __builtin_amdgcn_wave_barrier();
                    for (uint32_t base = 0; base < rem && pos < stop; base += 64) {
                        const uint32_t cnt = min(rem - base, 64u);
                        put(lane < cnt ? win[t.arg + skip0 + base + lane] : 0u, cnt);
                    }
                    if (pos < stop) {  // (the unit ends inside the token otherwise: its window is not needed any more)
                        if (t.kind == kExExt) seek_window_ext(win, wp, t.arg, t.len, W, lane);
                        else seek_window_match(win, wp, t.arg, t.len, mask, lane);
                    }
                }
            }
        } while (false);

        flush_stage(true);
        if (lane == 0) {
            if (op) atomicAdd(&a.got[q], op);
            if (oob) atomicOr(&a.flags[q], kSeekSawOob);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

struct SeekGatherArgs {
    SeekRanges r;
    const uint32_t* range_len;
    uint64_t n_ranges;
    uint32_t* out_len;
    int8_t* status;
};
__global__ void __launch_bounds__(256) tamp_seek_gather_kernel(SeekGatherArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.n_ranges) return;
    const int32_t pre = a.r.verdict[q];
    int8_t status = (int8_t)pre;
    uint32_t len = 0;
    if (pre == kSeekGo) {
        const uint32_t f = a.r.flags[q];
        len = a.r.got[q];
        if (f & kSeekSawBad) status = (int8_t)kSeekBadIndex, len = 0;
        else if (f & kSeekSawOob) status = (int8_t)kOob;
        else status = len == a.range_len[q] ? (int8_t)kOk : (int8_t)kInputExhausted;
    }
    a.status[q] = status, a.out_len[q] = len;
}

}  // namespace tamp_amd
