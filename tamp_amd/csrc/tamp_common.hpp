// tamp_common.hpp -- constants and small device helpers shared by the gfx950 kernels.
//
// Format facts restated from the reference (paths relative to its repository root):
//   prefix code for match lengths ......... tamp/_c_src/tamp/compressor.c:33-36
//   RLE / extended-match token layout ..... tamp/_c_src/tamp/compressor.c:257-263,342-415
//   tamp_res status numbering ............. tamp/_c_src/tamp/common.h:145-168
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tamp_amd {

constexpr int kWave = 64;          // gfx950 wavefront
constexpr uint32_t kRing = 16;     // the reference's input ring: look-ahead of one parse step
constexpr uint32_t kPendMax = 256; // >= 241 (longest RLE run) and >= 134 (longest extended match)
constexpr uint32_t kRleMax = 241;  // (14 << 4) + 15 + 2
constexpr uint32_t kRleWindowMax = 8;
constexpr uint32_t kExtExtraMax = 120;  // (14 << 3) + 7 + 1
constexpr int kSymRle = 12, kSymExt = 13, kSymFlush = 14;

enum : int8_t {
    kOk = 0,
    kOutputFull = 1,
    kInputExhausted = 2,
    kError = -1,
    kExcessBits = -2,
    kInvalidConf = -3,
    kOob = -4,
    kBadArgument = -21,  // TAMP_AMD_BAD_ARGUMENT (include/tamp_amd.h)
};

// The decoders count input in BITS in 32-bit registers: one call takes less than 2^29 bytes per stream.  The one-shot
// batch call reports longer streams as kBadArgument; the resumable call offers itself kMaxDecodeCall bytes and reports
// them consumed (the caller offers the rest again, as after any TAMP_INPUT_EXHAUSTED).
constexpr uint32_t kMaxDecodeIn = (1u << 29) - 1;
constexpr uint32_t kMaxDecodeCall = 1u << 28;

// Match-length prefix code (compressor.c:33-36): code without the leading 0 flag, length including it.  Packed into
// immediates as well (kCodeLo / kCodeHi / kNbitsPacked): no memory access on the hot paths.
constexpr uint8_t kCodeTab[15] = {0x00, 0x03, 0x08, 0x0b, 0x14, 0x24, 0x26, 0x2b, 0x4b, 0x54, 0x94, 0x95, 0xaa, 0x27, 0xab};
constexpr uint8_t kNbitsTab[15] = {2, 3, 5, 5, 6, 7, 7, 7, 8, 8, 9, 9, 9, 7, 9};  // incl. the flag bit
constexpr uint64_t pack_bytes(const uint8_t* v, int first, int count) {
    uint64_t r = 0;
    for (int i = 0; i < count; i++) r |= (uint64_t)v[first + i] << (8 * i);
    return r;
}
constexpr uint64_t pack_nibbles(const uint8_t* v, int count) {
    uint64_t r = 0;
    for (int i = 0; i < count; i++) r |= (uint64_t)v[i] << (4 * i);
    return r;
}
constexpr uint64_t kCodeLo = pack_bytes(kCodeTab, 0, 8), kCodeHi = pack_bytes(kCodeTab, 8, 7);
constexpr uint64_t kNbitsPacked = pack_nibbles(kNbitsTab, 15);
static_assert(kCodeLo == 0x2b2624140b080300ull && kCodeHi == 0x00ab27aa9594544bull && kNbitsPacked == 0x979998877765532ull,
              "packed prefix code");
__device__ __forceinline__ uint32_t tok_code(uint32_t i) {
    return (uint32_t)((i < 8 ? kCodeLo >> (8 * i) : kCodeHi >> (8 * (i - 8))) & 0xFF);
}
__device__ __forceinline__ uint32_t tok_nbits(uint32_t i) { return (uint32_t)(kNbitsPacked >> (4 * i)) & 15; }

__host__ __device__ constexpr uint32_t align_up(uint32_t x, uint32_t a) { return (x + a - 1) & ~(a - 1); }

// Widest token the compress kernel's emit phase places in ONE step (token_words below takes at most 32 bits):
//   literal                   flag + literal bits
//   match                     prefix code (flag included) + window bits; explicit pieces of the walk are no wider
//   settled RLE token         symbol 12, then the count's prefix code without its flag + 4 trailing bits  (compressor.c:342-359)
//   settled extended match    symbol 13, the size's prefix code without its flag + 3 trailing bits, window bits  (:377-415)
// Settled tokens exist in the PACKED builds only, which take windows up to 2^kPackedMaxWbits: the one constant plan_compress
// (tamp_compress_plan.hpp) and the block-mode test of the one-shot call (tamp_capi.hip) decide `packed` with.
constexpr uint32_t kPackedMaxWbits = 14;
constexpr uint32_t max_code_nbits() {
    uint32_t m = 0;
    for (int i = 0; i < 15; i++) m = kNbitsTab[i] > m ? kNbitsTab[i] : m;
    return m;
}
constexpr uint32_t max_u32(uint32_t a, uint32_t b) { return a > b ? a : b; }
constexpr uint32_t kMaxTokenBits =
    max_u32(max_u32(1 + 8, max_code_nbits() + 15),
            max_u32(kNbitsTab[kSymRle] + max_code_nbits() - 1 + 4, kNbitsTab[kSymExt] + max_code_nbits() - 1 + 3 + kPackedMaxWbits));
static_assert(kMaxTokenBits <= 32, "a token is placed as one 32-bit value: at most two words of the bit buffer");

// Where the nb-bit token v (1 <= nb <= 32, v < 2^nb) lands when it is written MSb-first at bit `bitpos` of a byte stream
// that is kept as 32-bit words in memory order: word *wi gets *w_hi ORed in, word *wi + 1 gets *w_lo when that is non-zero
// (zero whenever the token ends inside word *wi).  The words must be zero where the bits land.
__host__ __device__ __forceinline__ void token_words(uint32_t v, uint32_t nb, uint32_t bitpos, uint32_t* wi, uint32_t* w_hi,
                                                     uint32_t* w_lo) {
    const uint32_t ph = bitpos & 31u;
    const uint64_t x = (uint64_t)v << (64u - ph - nb);  // shift count 1..63
    *wi = bitpos >> 5;
    *w_hi = __builtin_bswap32((uint32_t)(x >> 32));
    *w_lo = __builtin_bswap32((uint32_t)x);
}

// The bucket scan's candidate lengths in BIT units (the fixed-geometry compress builds, kBitLen): a candidate's common prefix
// with the pattern is kept as the bit offset of the first difference, 16..128, and becomes a byte count by one shift.
// A candidate that passed the scan's window test has y = distance << LB | (its bytes 2, 3 ^ the pattern's, LB bits): the XOR of
// byte 2 in bits 0..7 and of the low LB - 8 bits of byte 3 above them.  The first set bit of y therefore classifies it:
//   below LB      a shallow candidate, and that bit | 16 is its first difference counted from the pattern's first bit (bytes 0 and 1
//                 agree: the same bucket and rest): 16..23 -> 2 bytes, 24..16 + LB - 1 -> 3;
//   LB or above   (the distance's bits; all ones for y == 0, the oldest window byte) a deep candidate: the 16-byte compare decides.
// first_set_or_ones is v_ffbl_b32 as the hardware defines it: all ones for a zero operand.
__host__ __device__ __forceinline__ uint32_t first_set_or_ones(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
#else
    return x ? (uint32_t)__builtin_ctz(x) : 0xFFFFFFFFu;
#endif
}
constexpr uint32_t kScanBitsCap = 128;  // a 16-byte hit
template <uint32_t LB>
__host__ __device__ __forceinline__ bool scan_is_deep(uint32_t first_bit_of_y) { return first_bit_of_y > LB - 1; }
__host__ __device__ __forceinline__ uint32_t scan_shallow_bits(uint32_t first_bit_of_y) { return first_bit_of_y | 16u; }
// The 16-byte compare's four difference dwords (candidate ^ pattern, little-endian, in byte order) to the capped bit offset of the
// first difference: 0..128.  `| 32` (64, 96) is exact for 0..31 and keeps all ones; the cap rides in the second three-way minimum.
// (`cap`: kScanBitsCap, which the kernel hands over in a register of its choice -- 128 is no inline constant of the three-operand
// encoding, and left to itself the compiler keeps it in one more scalar register of a kernel that spills those)
__host__ __device__ __forceinline__ uint32_t scan_deep_bits(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3,
                                                            uint32_t cap = kScanBitsCap) {
    const uint32_t t0 = first_set_or_ones(x0), t1 = first_set_or_ones(x1) | 32u, t2 = first_set_or_ones(x2) | 64u,
                   t3 = first_set_or_ones(x3) | 96u;
    const uint32_t m = t0 < t1 ? (t0 < t2 ? t0 : t2) : (t1 < t2 ? t1 : t2);
    const uint32_t m2 = m < t3 ? m : t3;
    return m2 < cap ? m2 : cap;
}
__host__ __device__ __forceinline__ uint32_t scan_bits_len(uint32_t bits) { return bits >> 3; }    // bytes: 2..16 (deep: 0..16)
__host__ __device__ __forceinline__ uint32_t scan_bits_hit16(uint32_t bits) { return bits >> 7; }  // 1 for a 16-byte hit

// Dictionary tables (the *_dicts calls): stream i's dictionary is the W bytes at `off` = dict_off[i] of a buffer of `len`
// bytes.  Offsets are multiples of 16: the decoders seed their windows with 16-byte loads, the compress kernel with dwords.
constexpr uint32_t kDictOffAlign = 16;
__host__ __device__ constexpr bool dict_off_aligned(uint64_t off) { return (off & (kDictOffAlign - 1)) == 0; }
__host__ __device__ constexpr bool dict_off_in_bounds(uint64_t off, uint32_t W, uint64_t len) { return off <= len && W <= len - off; }

__host__ __device__ constexpr int min_pattern_size(int window, int literal) {
    return 2 + (window > 10 + 2 * (literal - 5));
}

// gfx950 LDS serves misaligned ds_read_b32 / _b128 in hardware (the compiler emits them for align-1 types); a
// misaligned access costs the LDS pipe extra passes, so the hot bucket scan keeps aligned dwords + v_alignbyte.
struct __attribute__((packed, aligned(1))) LdsU128 { uint32_t x, y, z, w; };

// 4 bytes at an arbitrary LDS byte offset: two aligned dwords funnel-shifted by the byte phase.
__device__ __forceinline__ uint32_t lds_u32_unaligned(const uint8_t* base, uint32_t off) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(base + (off & ~3u));
    return __builtin_amdgcn_alignbyte(w[1], w[0], off & 3u);
}

// 4 * N consecutive bytes at an arbitrary LDS byte offset, as N dwords: P[j] = lds_u32_unaligned(base, off + 4 * j), from ONE
// aligned base -- N + 1 aligned dwords at immediate offsets and N funnel shifts by the one byte phase, where N separate calls
// compute N addresses and fetch 2 * N dwords (neighbouring pairs overlap).  Reads up to base + (off & ~3) + 4 * N + 3, like
// the last of those calls.
template <int N>
__device__ __forceinline__ void lds_bytes_unaligned(const uint8_t* base, uint32_t off, uint32_t (&P)[N]) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(base + (off & ~3u));
    const uint32_t sh = off & 3u;
    uint32_t d[N + 1];
#pragma unroll
    for (int j = 0; j <= N; j++) d[j] = w[j];
#pragma unroll
    for (int j = 0; j < N; j++) P[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
}

// Inclusive scans over the 64 lanes with DPP row shifts and row broadcasts (six data-parallel-primitive moves instead of
// six ds_bpermute round trips through the LDS pipe with their lane-index arithmetic: __shfl_up compiles to the latter).
// row_shr:n keeps `old` (the identity) where the source lane lies outside the 16-lane row; row_bcast:15 / :31 hand the
// last lane of a row / of the lower half to the rows the row mask selects.
// The DPP controls used below (row_bcast:15 / :31 here, wave_shr:1 in the resolve kernel) exist on the GFX9 family
// (GCN / CDNA, 64-wide wavefronts) only -- which is all this library builds for.  Call sites must be wave-uniform with
// every lane enabled: the row broadcasts read lanes that a partial EXEC mask would leave stale.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "tamp_amd device code is written for gfx9-family wave64 targets (gfx950); its DPP scans have no gfx10+ form"
#endif
template <class Op>
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x, uint32_t identity, Op op) {
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)x, 0x111, 0xF, 0xF, false));  // row_shr:1
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)x, 0x112, 0xF, 0xF, false));  // row_shr:2
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)x, 0x114, 0xF, 0xF, false));  // row_shr:4
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)x, 0x118, 0xF, 0xF, false));  // row_shr:8
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)x, 0x142, 0xA, 0xF, false));  // row_bcast:15 -> rows 1, 3
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)x, 0x143, 0xC, 0xF, false));  // row_bcast:31 -> rows 2, 3
    return x;
}
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t x) {
    return wave_scan_incl(x, 0u, [](uint32_t a, uint32_t b) { return a + b; });
}
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t x) {
    return wave_scan_incl(x, 0u, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        uint32_t o = (uint32_t)__shfl_xor((int)v, off);
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace tamp_amd
