// tamp_pieces_kernel.hpp -- tamp_batch_compress_pieces: the kernels around the compress kernel.
//
// N streaming compressors, each handed one bounded piece, advanced by launches of the batch compress kernel
// (tamp_compress_kernel.hpp, untouched).  That kernel takes per launch ONE lead (none / header / append marker) and ONE end
// (partial / flush / flush + token) and a state row per stream ordinal, so the objects of a call are sorted into classes of
// (lead, end) and every class that occurs is one launch over rows that lie together:
//   tamp_pieces_classify_kernel  one lane per object: the checks of the single piece call, the class, the object's rank in
//                                its class and the place of its input row; the empty piece is finished here.
//   tamp_pieces_stage_kernel     one wavefront per object: the kernel's state row (window + kSlot* fields), the input row
//                                (the bytes a carried run / extended match consumed, the carried ring bytes, the new input)
//                                and the gathered table row.
//   tamp_pieces_unstage_kernel   one wavefront per object: the state row back into the object when the piece completed,
//                                results into the caller's rows.
// Every object is staged as a RESUMED one: a fresh object's row holds the pristine window (seeded, or the object's own window
// bytes as the custom dictionary) with window_pos 0 and no carry, which is what the kernel's fresh path starts from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tamp_common.hpp"
#include "tamp_compress_kernel.hpp"

namespace tamp_amd {

// TampAmdPieceObject (include/tamp_amd.h), by offset: TampAmdLazyCarry first
enum : uint32_t {
    kObjRle = 0, kObjExtCount = 1, kObjExtPos = 2, kObjNbits = 4, kObjTailLen = 5, kObjBits = 8, kObjTail = 12,
    kObjLazyPos = 28, kObjLazyLen = 30, kObjWindowPos = 32, kObjToken = 34, kObjHeader = 48,
};
// the op bits (TAMP_AMD_PIECE_*)
enum : uint32_t { kOpHeader = 1, kOpAppend = 2, kOpResume = 4, kOpFinish = 8, kOpToken = 16, kOpKnown = 31, kOpSkip = 128 };
// class = lead * 3 + end; lead: 0 none, 1 header, 2 append marker; end: 0 partial, 1 flush, 2 flush + token
constexpr uint32_t kPieceClasses = 9;
constexpr uint8_t kPieceDone = 0xFF;   // nothing to launch: SKIP, refused, or the empty piece (finished by the classify kernel)
constexpr uint32_t kPieceRowAlign = 16;  // input rows start at multiples of it

struct PieceRecord {  // what the host waits for
    uint32_t count[kPieceClasses];    // objects per class
    uint32_t longest[kPieceClasses];  // longest staged input row per class
    uint32_t pad[2];
    unsigned long long in_bytes;      // input rows, padded, all classes
};

struct PieceArgs {
    uint8_t* objects;
    uint64_t stride;
    const uint8_t* ops;
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    uint8_t* out;
    const uint64_t* out_off;
    const uint32_t* out_cap;
    uint32_t* out_len;
    int8_t* status;
    uint32_t n, wbits;
    uint32_t lazy, custom_dict;
    const uint8_t* seed;  // the seeded window of the configuration's literal size
    // per object (scratch)
    uint8_t* cls;
    uint32_t* rank;      // in its class; row = base[class] + rank
    uint64_t* row_off;   // of its input row in rows_in
    PieceRecord* rec;
    // per row (scratch): the compress launches' tables, state rows and input rows
    uint64_t* g_in_off;
    uint64_t* g_out_off;
    uint32_t* g_in_len;
    uint32_t* g_out_cap;
    uint32_t* g_out_len;
    int8_t* g_status;
    uint8_t* rows_state;
    uint8_t* rows_in;
    uint32_t base[kPieceClasses];
};

__device__ __forceinline__ uint32_t piece_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

__global__ void __launch_bounds__(256) tamp_pieces_classify_kernel(PieceArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const uint32_t W = 1u << a.wbits;
    uint32_t cls = kPieceDone, total = 0;
    if (i < a.n) {
        const uint32_t op = a.ops[i];
        if (!(op & kOpSkip)) {
            const uint32_t* const h32 = reinterpret_cast<const uint32_t*>(a.objects + (size_t)i * a.stride);
            uint32_t h[9];  // the carry and window_pos
#pragma unroll
            for (int k = 0; k < 9; k++) h[k] = h32[k];
            const uint32_t rle = h[0] & 0xFF, ext = (h[0] >> 8) & 0xFF, ext_pos = h[0] >> 16;
            const uint32_t nbits = h[1] & 0xFF, tail_len = (h[1] >> 8) & 0xFF, bits = h[2];
            const uint32_t lazy_pos = h[7] & 0xFFFF, lazy_len = (h[7] >> 16) & 0xFF;
            const uint32_t n = a.in_len[i], cap = a.out_cap[i];
            const bool resume = op & kOpResume, finish = op & kOpFinish;
            const uint32_t lead = (op & kOpAppend) ? 2u : ((op & kOpHeader) ? 1u : 0u);
            bool bad = (op & ~kOpKnown) != 0 || (op & (kOpHeader | kOpAppend)) == (kOpHeader | kOpAppend) || n > 0xFFFFFF00u;
            // the rules of the single piece call (segment_core), in its words
            if (lazy_len) bad = bad || !resume || !a.lazy || rle || ext || lazy_pos + lazy_len > W || lazy_len > tail_len;
            if (resume) bad = bad || tail_len > 16 || nbits > 31 || (rle && ext) || ext_pos + ext > W || (lead && nbits);
            const uint32_t pre = resume ? rle + ext + tail_len : 0u;
            bad = bad || (uint64_t)pre + n > 0xFFFFFFFFull;  // (32-bit stream lengths)
            if (bad) {
                a.status[i] = kBadArgument, a.out_len[i] = 0;
            } else if (!finish && resume && n == 0 && !lead) {
                // tamp_compressor_compress without input: nothing is sunk and nothing polled; the whole bytes among the
                // pending bits leave (compressor.c:700)
                const uint32_t whole = nbits >> 3;
                if (cap < whole) {
                    a.status[i] = kOutputFull, a.out_len[i] = 0;
                } else {
                    uint8_t* const o = a.out + a.out_off[i];
                    for (uint32_t k = 0; k < whole; k++) o[k] = (uint8_t)(bits >> (24 - 8 * k));
                    uint8_t* const obj = a.objects + (size_t)i * a.stride;
                    if (whole) *reinterpret_cast<uint32_t*>(obj + kObjBits) = bits << (8 * whole);
                    obj[kObjNbits] = (uint8_t)(nbits & 7), obj[kObjToken] = 0;
                    a.status[i] = kOk, a.out_len[i] = whole;
                }
            } else {
                cls = lead * 3 + (finish ? ((op & kOpToken) ? 2u : 1u) : 0u);
                total = pre + n;
            }
        }
    }
    // ranks and places, one atomic per wavefront and class (all lanes arrive here)
    // (in units of the row alignment, with one to spare behind every row: the compress kernel's vector loads may run past a
    // row's last byte.  Up to 2^28 + 1 each, so a wavefront's sum is scanned as two 16-bit halves)
    const uint32_t units = cls == kPieceDone ? 0u : (uint32_t)(((uint64_t)total + kPieceRowAlign - 1) / kPieceRowAlign) + 1u;
    uint32_t rank = 0;
    for (uint32_t c = 0; c < kPieceClasses; c++) {
        const uint64_t same = __ballot(cls == c);
        if (!same) continue;
        const uint32_t longest = wave_max_u32(cls == c ? total : 0u);
        const uint32_t leader = (uint32_t)__builtin_ctzll(same);
        uint32_t first = 0;
        if (lane == leader) {
            first = atomicAdd(&a.rec->count[c], (uint32_t)__builtin_popcountll(same));
            atomicMax(&a.rec->longest[c], longest);
        }
        first = (uint32_t)__builtin_amdgcn_readlane((int)first, (int)leader);
        if (cls == c) rank = first + (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1));
    }
    const uint32_t lo = wave_scan_add(units & 0xFFFFu), hi = wave_scan_add(units >> 16);
    const unsigned long long incl = ((unsigned long long)hi << 16) + lo;
    const unsigned long long sum = (((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)hi, 63)) << 16) +
                                   (uint32_t)__builtin_amdgcn_readlane((int)lo, 63);
    unsigned long long at = 0;
    if (lane == 0 && sum) at = atomicAdd(&a.rec->in_bytes, sum * kPieceRowAlign);
    const uint32_t at_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)at, 0);
    const uint32_t at_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(at >> 32), 0);
    if (i < a.n) {
        a.cls[i] = (uint8_t)cls;
        a.rank[i] = rank;
        a.row_off[i] = (((unsigned long long)at_hi << 32) | at_lo) + (incl - units) * kPieceRowAlign;
    }
}

// dst <- src, n bytes, by one wavefront.  dst is 16-byte aligned; src is anywhere (its 16-byte loads are unaligned ones).
__device__ __forceinline__ void piece_copy_to_aligned(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane) {
    struct __attribute__((packed, aligned(1))) Loose { uint32_t x, y, z, w; };
    const uint32_t nv = n >> 4;
    for (uint32_t k = lane; k < nv; k += kWave) {
        const Loose v = reinterpret_cast<const Loose*>(src)[k];
        reinterpret_cast<uint4*>(dst)[k] = make_uint4(v.x, v.y, v.z, v.w);
    }
    for (uint32_t k = (nv << 4) + lane; k < n; k += kWave) dst[k] = src[k];
}
// (both 8-byte aligned, n a multiple of 8: windows between objects and state rows)
__device__ __forceinline__ void piece_copy_window(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane) {
    for (uint32_t k = lane; k < (n >> 3); k += kWave) reinterpret_cast<uint2*>(dst)[k] = reinterpret_cast<const uint2*>(src)[k];
}

__global__ void __launch_bounds__(256) tamp_pieces_stage_kernel(PieceArgs a) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= a.n) return;
    const uint32_t cls = a.cls[i];
    if (cls == kPieceDone) return;
    const uint32_t W = 1u << a.wbits;
    const uint32_t row = a.base[cls] + a.rank[i];
    const uint8_t* const obj = a.objects + (size_t)i * a.stride;
    const uint8_t* const win = obj + kObjHeader;
    const bool resume = a.ops[i] & kOpResume;
    uint8_t* const st = a.rows_state + (size_t)row * (W + kSegStateExtra);
    piece_copy_window(st, (resume || a.custom_dict) ? win : a.seed, W, lane);
    const uint32_t rle = resume ? obj[kObjRle] : 0u, ext = resume ? obj[kObjExtCount] : 0u;
    const uint32_t ext_pos = resume ? piece_u16(obj + kObjExtPos) : 0u, tail_len = resume ? obj[kObjTailLen] : 0u;
    const uint32_t wp = resume ? piece_u16(obj + kObjWindowPos) & (W - 1) : 0u;
    if (lane < kSegStateExtra) {  // the kSlot* fields, a byte per lane
        const uint32_t k = lane;
        const uint32_t lazy_len = resume ? obj[kObjLazyLen] : 0u;
        uint32_t v = 0;
        if (k < kSlotWindowPos + 2) v = wp >> (8 * (k - kSlotWindowPos));
        else if (k == kSlotRle) v = rle;
        else if (k == kSlotExtCount) v = ext;
        else if (k == kSlotNbits) v = resume ? obj[kObjNbits] : 0u;
        else if (k >= kSlotExtPos && k < kSlotExtPos + 2) v = ext_pos >> (8 * (k - kSlotExtPos));
        else if (k == kSlotLazyLen) v = lazy_len;
        else if (k >= kSlotLazyPos && k < kSlotLazyPos + 2) v = lazy_len ? obj[kObjLazyPos + (k - kSlotLazyPos)] : 0u;
        else if (k >= kSlotBits && k < kSlotBits + 4) v = resume ? obj[kObjBits + (k - kSlotBits)] : 0u;
        st[W + k] = (uint8_t)v;
    }
    // the input row: run bytes (the last byte written), extended-match bytes (window[ext_pos ..)), ring bytes, new input
    const uint64_t off = a.row_off[i];
    uint8_t* const dst = a.rows_in + off;
    const uint32_t pre = rle + ext + tail_len, n = a.in_len[i];
    const uint8_t last = win[(wp - 1) & (W - 1)];
    for (uint32_t k = lane; k < pre; k += kWave)
        dst[k] = k < rle ? last : (k < rle + ext ? win[ext_pos + (k - rle)] : obj[kObjTail + (k - rle - ext)]);
    const uint8_t* src = a.in + a.in_off[i];
    const uint32_t head = min((kPieceRowAlign - (pre & (kPieceRowAlign - 1))) & (kPieceRowAlign - 1), n);
    if (lane < head) dst[pre + lane] = src[lane];
    if (n > head) piece_copy_to_aligned(dst + pre + head, src + head, n - head, lane);
    if (lane == 0) {
        a.g_in_off[row] = off, a.g_in_len[row] = pre + n;
        a.g_out_off[row] = a.out_off[i], a.g_out_cap[row] = a.out_cap[i];
    }
}

__global__ void __launch_bounds__(256) tamp_pieces_unstage_kernel(PieceArgs a) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= a.n) return;
    const uint32_t cls = a.cls[i];
    if (cls == kPieceDone) return;
    const uint32_t W = 1u << a.wbits;
    const uint32_t row = a.base[cls] + a.rank[i];
    const bool finish = cls % 3 != 0;
    int8_t status = a.g_status[row];
    const uint32_t produced = a.g_out_len[row];
    if (status != kOk) {  // the object stays as it came; an unfinished piece that did not complete delivers nothing
        if (lane == 0) a.status[i] = status, a.out_len[i] = finish ? produced : 0u;
        return;
    }
    uint8_t* const obj = a.objects + (size_t)i * a.stride;
    const uint8_t* const st = a.rows_state + (size_t)row * (W + kSegStateExtra);
    const uint8_t* const f = st + W;
    const uint32_t total = a.g_in_len[row];
    const uint32_t parsed = (uint32_t)f[kSlotParsed] | ((uint32_t)f[kSlotParsed + 1] << 8) | ((uint32_t)f[kSlotParsed + 2] << 16) |
                            ((uint32_t)f[kSlotParsed + 3] << 24);
    const uint32_t left = total - parsed;  // <= 16: the ring (full when the call's last poll consumed nothing)
    if (!finish && (parsed > total || left > 16)) {
        if (lane == 0) a.status[i] = kError, a.out_len[i] = 0;
        return;
    }
    piece_copy_window(obj + kObjHeader, st, W, lane);
    if (lane < 12) {  // the object's 48 bytes in front of the window, a dword per lane
        const uint8_t* const tail = a.rows_in + a.row_off[i] + parsed;
        auto tail_byte = [&](uint32_t j) -> uint32_t { return j < left ? tail[j] : 0u; };
        const uint32_t lazy_len = f[kSlotLazyLen];
        uint32_t v = 0;
        if (lane == 8) v = piece_u16(f + kSlotWindowPos) | ((uint32_t)f[kSlotToken] << 16);
        else if (!finish) {
            // (the position only with a count: without one the kernel's field holds whichever match its serial walk took last,
            // which depends on the launch's block size, i.e. on the other objects of the call)
            if (lane == 0) v = (uint32_t)f[kSlotRle] | ((uint32_t)f[kSlotExtCount] << 8) | (f[kSlotExtCount] ? piece_u16(f + kSlotExtPos) << 16 : 0u);
            else if (lane == 1) v = (uint32_t)f[kSlotNbits] | (left << 8);
            else if (lane == 2) v = piece_u16(f + kSlotBits) | (piece_u16(f + kSlotBits + 2) << 16);
            else if (lane < 7) {
                const uint32_t j = (lane - 3) * 4;
                v = tail_byte(j) | (tail_byte(j + 1) << 8) | (tail_byte(j + 2) << 16) | (tail_byte(j + 3) << 24);
            } else if (lane == 7) v = (lazy_len ? piece_u16(f + kSlotLazyPos) : 0u) | (lazy_len << 16);
        }
        reinterpret_cast<uint32_t*>(obj)[lane] = v;
    }
    if (lane == 0) a.status[i] = status, a.out_len[i] = produced;
}

}  // namespace tamp_amd
