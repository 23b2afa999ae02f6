// tamp_decompress_plan.hpp -- WHICH decoder takes a decompress batch and how it is sized: pre-pass, narrowed window,
// decoder, geometry.  Host arithmetic over the call, the pre-pass result, three device facts and the tuning environment (no HIP call,
// no allocation); launch_decompress, the resume launchers (wave_geometry) and tamp_amd_decompress_plan use it.
#pragma once
#include <algorithm>
#include <cstdlib>
#include "tamp_amd.h"
#include "tamp_decompress_kernel.hpp"
#include "tamp_decompress_split_kernel.hpp"
#include "tamp_decompress_wave_kernel.hpp"

namespace tamp_amd {

// What a call asks for, as far as the plan depends on it.
struct DecodeCall {
    size_t n_streams;
    uint8_t max_wbits;  // as passed: TAMP_AMD_WINDOW_BITS_EXACT still set if the caller set it
    bool has_dict;      // a custom dictionary was passed
    bool exact() const { return (max_wbits & TAMP_AMD_WINDOW_BITS_EXACT) != 0; }
    uint8_t bits() const { return max_wbits & 0x7F; }
};
// The four words of tamp_header_scan_kernel; as constructed: the pre-pass did not run and nothing is known.
struct DecodeScan {
    uint32_t found = 0;                 // largest window bits of the batch's headers, 0 = no valid header at all
    uint32_t longest_in = 0xFFFFFFFFu;  // longest compressed stream
    uint32_t window_units = 0;          // sum of the streams' window sizes in 256-byte units
    uint32_t max_out_cap = 0;           // largest out_cap
};
struct DecodeDevice {
    uint32_t cu_count;
    bool free_known;    // hipMemGetInfo answered ...
    size_t free_bytes;  // ... this
    size_t held_bytes;  // what the stream's split-decoder slab already holds (part of what the call may use)
};

// TAMP_AMD_DECODER = "wave" | "lane" | "global" | "split" (tuning / tests): the first letter decides; nullptr = the plan's own choice.
static inline const char* forced_decoder() { return getenv("TAMP_AMD_DECODER"); }

// The host-only gate in front of the long-stream attempt (tamp_decompress_long_kernel.hpp: a handful of streams, the whole device
// each), with what launch_decompress_long takes from the environment.  All that needs the stream's bytes is that launcher's.
struct DecodeLong {
    bool attempt;
    uint32_t min_len;     // shortest compressed stream it takes (TAMP_AMD_LONGDEC_MIN, from 64)
    bool extended, chain; // TAMP_AMD_LONGDEC_EXT=0 (tests): extended streams to the exact decoders; TAMP_AMD_LONGDEC_CHAIN=0: v1 groups in order
};
static inline DecodeLong decode_wants_long(const DecodeCall& c) {
    const char *const on = getenv("TAMP_AMD_LONGDEC"), *const min_env = getenv("TAMP_AMD_LONGDEC_MIN");
    const char *const ext = getenv("TAMP_AMD_LONGDEC_EXT"), *const chain = getenv("TAMP_AMD_LONGDEC_CHAIN");
    DecodeLong g = {c.n_streams <= 16 && !c.exact() && !(on && atoi(on) == 0) && !forced_decoder(), 256u << 10,
                    !(ext && atoi(ext) == 0), !chain || atoi(chain) != 0};
    if (min_env) { const long v = atol(min_env); if (v >= 64) g.min_len = (uint32_t)v; }
    return g;
}

// The header pre-pass (one tiny kernel and a 16-byte copy that waits for the stream): from 256 streams on when there is anything to
// narrow (limit above 2^8), and whenever the split decoder is forced, which cannot be sized without it.
static inline bool decode_wants_scan(const DecodeCall& c) {
    const char* force = forced_decoder();
    return !c.exact() && c.bits() >= 8 && c.bits() <= 15 && ((c.bits() > 8 && c.n_streams >= 256) || (force && force[0] == 's'));
}

enum class Decoder : uint8_t { kSplit, kWave, kLaneLds, kLaneGlobal };

// One wavefront per stream or object: four per workgroup up to 2^12-byte windows, one above; grid-stride beyond cu_count * 64
// workgroups.  Shared by the wave decoder and both resume kernels; the LDS function and the kernel are the caller's.
struct WaveGeometry { uint32_t waves, groups; };
static inline WaveGeometry wave_geometry(uint32_t bits_max, size_t n, uint32_t cu_count) {
    const uint32_t waves = bits_max <= 12 ? 4 : 1;
    return {waves, (uint32_t)std::min((n + waves - 1) / waves, (size_t)cu_count * 64)};
}

// TAMP_AMD_SPLIT_SPW = 16 | 32 | 64 (tuning / tests): streams per parse wavefront; 0 = the geometry's own choice.
static inline uint32_t forced_split_spw() {
    const char* e = getenv("TAMP_AMD_SPLIT_SPW");
    const int v = e ? atoi(e) : 0;
    return (v == 16 || v == 32 || v == 64) ? (uint32_t)v : 0u;
}

// Streams per parse wavefront for `count` streams (PARSE and its size-only build): enough waves for ~4 per SIMD before lanes are
// filled (tools/dec_split_pmc.sh: the parse runs at one wave's latency)
static inline size_t parse_want_waves(uint32_t cu_count) { return (size_t)cu_count * 16; }
static inline uint32_t parse_spw(size_t count, size_t want_waves, uint32_t forced) {
    return forced ? forced : (count / 16 < want_waves ? 16u : (count / 32 < want_waves ? 32u : 64u));
}

// Split decoder (tamp_decompress_split_kernel.hpp): records, meta word and lag list per stream of a SLICE, a flag byte per stream
// of the batch.  The launcher halves `slice` when the device cannot supply slab_bytes(slice), and asks again.
struct SplitGeometry {
    uint32_t tokcap, maxcap;  // records per stream (whole 64-byte groups), largest out_cap
    size_t slice;             // streams per parse + resolve pair, as the scratch budget allows
    bool wave_resolve;        // RESOLVE: a wavefront per stream, four per workgroup (out_cap up to 2 KiB); else a workgroup per stream
    uint32_t resolve_lds;
    size_t n_streams, want_waves;  // (for the two functions below)
    uint32_t spw_forced;
    size_t b_recs(size_t s) const { return s * tokcap * 4; }
    size_t b_meta(size_t s) const { return s * 4; }
    size_t b_lag(size_t s) const { return s * kSplitMaxLag * 8; }
    size_t slab_bytes(size_t s) const { return b_recs(s) + b_meta(s) + b_lag(s) + n_streams + 64; }
    uint32_t spw(uint32_t count) const { return parse_spw(count, want_waves, spw_forced); }  // for a slice of `count` streams
};
static inline SplitGeometry split_geometry(const DecodeCall& c, const DecodeScan& s, const DecodeDevice& d) {
    SplitGeometry g = {};
    g.maxcap = s.max_out_cap, g.n_streams = c.n_streams;
    g.tokcap = std::max<uint32_t>(16, (uint32_t)std::min<uint64_t>(s.max_out_cap, (uint64_t)s.longest_in * 8 / 6 + 8));
    g.tokcap = (g.tokcap + 15u) & ~15u;
    // Streams per slice: 256 Ki = 4 parse waves per SIMD (measured on configs[3], 1 Mi streams: 2^17 29.4 ms, 2^18 25.4 ms,
    // 2^19 26.4 ms; TAMP_AMD_SPLIT_SLICE_LOG2 overrides), less when the scratch budget says so (records dominate: tokcap x 4 B
    // per stream).
    size_t slice_log2 = 18;
    if (const char* e = getenv("TAMP_AMD_SPLIT_SLICE_LOG2")) { const int v = atoi(e); if (v >= 12 && v <= 22) slice_log2 = (size_t)v; }
    // Scratch budget: a quarter of what the device has free right now, 8 GiB at most (callers that fill HBM with their own batches
    // keep most of it; a slice of 2^18 long streams needs ~3.7 GiB, and configs[3] cut into uneven slices by a 4 GiB budget ran 6.5
    // instead of 5.1 ms).  The slab the stream already holds counts as free: without it the budget -- and with it the slice size,
    // hence the decode time -- of the second call on a shape differed from the first's.  TAMP_AMD_SPLIT_SCRATCH_MB overrides.
    size_t budget = (size_t)8 << 30;
    if (d.free_known) budget = std::min(budget, std::max((d.free_bytes + d.held_bytes) / 4, d.held_bytes));
    if (const char* e = getenv("TAMP_AMD_SPLIT_SCRATCH_MB")) { const long v = atol(e); if (v > 0) budget = (size_t)v << 20; }
    const size_t per = (size_t)g.tokcap * 4 + 4 + kSplitMaxLag * 8;
    g.slice = std::min(std::min<size_t>(c.n_streams, (size_t)1 << slice_log2), std::max<size_t>(budget / per, 4096));
    g.wave_resolve = s.max_out_cap <= kSplitWaveMaxOut;
    if (const char* e = getenv("TAMP_AMD_SPLIT_WAVE_MAX")) {  // (tuning; the one-wavefront RESOLVE covers 4 x 16 x 64 = 4,096 positions)
        const int v = atoi(e);
        g.wave_resolve = s.max_out_cap <= (uint32_t)(v < 0 ? 0 : (v > 4096 ? 4096 : v));
    }
    g.resolve_lds = split_resolve_lds(s.max_out_cap) * (g.wave_resolve ? 4u : 1u);
    g.want_waves = parse_want_waves(d.cu_count);
    g.spw_forced = forced_split_spw();
    return g;
}

// The size query (tamp_batch_decoded_size: the parse's size-only build): streams per wavefront by SplitGeometry::spw's rule --
// enough waves for ~4 per SIMD before lanes are filled, TAMP_AMD_SPLIT_SPW forces 16 / 32 / 64 -- and ONE grid of 256-thread
// workgroups, in strides beyond eight per CU -- about what is resident at 57 VGPRs (seven waves per SIMD) and 68 bytes of LDS per lane.
struct SizeGeometry { uint32_t spw, grid, lds; };
static inline SizeGeometry size_geometry(size_t n_streams, uint32_t cu_count) {
    const uint32_t spw = parse_spw(n_streams, parse_want_waves(cu_count), forced_split_spw());
    const size_t waves = (n_streams + spw - 1) / spw;
    return {spw, (uint32_t)std::max<size_t>(1, std::min((waves + 3) / 4, (size_t)cu_count * 8)), split_size_lds(256)};
}

// The size query for decoder objects (tamp_batch_decoded_size_pieces, tamp_decoded_size_pieces_kernel.hpp): a lane per row by the
// same rule -- rows per wavefront from parse_spw, one grid of 256-thread workgroups in strides beyond eight per CU -- and no LDS: the
// kernel runs the exact loop alone.
static inline SizeGeometry size_pieces_geometry(size_t n_rows, uint32_t cu_count) {
    const SizeGeometry g = size_geometry(n_rows, cu_count);
    return {g.spw, g.grid, 0u};
}

// Lane per stream, windows in LDS: one 64-lane workgroup per 64 streams, one padded row per lane; the bulk build (streams of 512
// compressed bytes and more) adds per-lane staging.  The ONE definition: the capacity estimate and the launch both read it.
struct LaneLdsGeometry { uint32_t lds_row, lds, per_cu, grid; };
static inline LaneLdsGeometry lane_lds_geometry(uint32_t wbits, bool bulk, size_t n_streams, uint32_t cu_count) {
    const uint32_t row = (1u << wbits) + (bulk ? kLaneRowPad : 4u);
    const uint32_t lds = bulk ? lane_decoder_lds(wbits) : kWave * row;
    const uint32_t per_cu = std::min<uint32_t>(160 * 1024 / lds, 16);
    // grid-stride beyond a few waves of workgroups
    return {row, lds, per_cu, (uint32_t)std::min((n_streams + kWave - 1) / kWave, (size_t)cu_count * per_cu * 4)};
}

// Lane per stream, windows in a global scratch slab of one slot per resident lane, 256-thread workgroups.
struct LaneGlobalGeometry {
    uint32_t slot;      // bytes per lane: the window, padded like an LDS row in the bulk build
    bool gbulk;         // bulk path with the windows in the slab
    size_t lanes;       // resident lanes
    uint32_t grid, lds; // workgroups, dynamic LDS (the bulk build's staging)
    size_t slab_bytes;
};
static inline LaneGlobalGeometry lane_global_geometry(uint32_t wbits, bool valid_bits, bool bulk, const DecodeCall& c,
                                                      const DecodeScan& s, uint32_t cu_count) {
    const uint32_t threads = 256;
    const uint32_t slot_bits = valid_bits ? wbits : 8;  // window bits outside 8..15 (every stream fails): non-bulk lanes, 256-byte slots
    LaneGlobalGeometry g = {};
    g.gbulk = valid_bits && bulk;
    g.slot = (1u << slot_bits) + (g.gbulk ? 64 : 0);
    // Resident lanes.  Every step touches the lane's window at random: the kernel runs at the speed of the Infinity Cache (256 MB)
    // as long as the windows in flight fit into it, and of HBM sector traffic beyond.  So: as many lanes as ~144 MB of live windows
    // allow (TAMP_AMD_SCRATCH_MB, tuning), but at least one wave per SIMD (and no more than eight); the slab never above 4 GiB.
    const uint64_t window_bytes = (uint64_t)s.window_units << 8;
    const size_t avg_window = window_bytes ? std::max<size_t>(256, (size_t)(window_bytes / c.n_streams)) : ((size_t)1 << slot_bits);
    size_t fit = ((size_t)144 << 20) / avg_window;
    if (const char* e = getenv("TAMP_AMD_SCRATCH_MB")) fit = ((size_t)atoi(e) << 20) / avg_window;
    g.lanes = std::min((size_t)cu_count * 2048, std::max(fit, (size_t)cu_count * 256));
    g.lanes = std::min(std::min(g.lanes, ((size_t)4 << 30) / g.slot), c.n_streams);
    g.grid = (uint32_t)((g.lanes + threads - 1) / threads);
    g.lds = g.gbulk ? 128 + threads * kLaneStagePad : 0;
    g.slab_bytes = (size_t)g.grid * threads * g.slot;
    return g;
}

struct DecodePlan {  // (in the order plan_decompress decides them; only the chosen decoder's geometry is filled in)
    uint8_t max_wbits;  // narrowed to the largest window the pre-pass found
    bool bulk;          // streams of 512 compressed bytes and more, or of unknown length: the lane decoders' bulk builds
    Decoder decoder;
    SplitGeometry split;
    WaveGeometry wave;  // kWave, and kSplit: what the split decoder flags is decoded by the wave decoder afterwards
    uint32_t wave_lds;
    LaneLdsGeometry lane;
    LaneGlobalGeometry global;
};

// The decisions for one call.  `scan`: the pre-pass's answer, read only when decode_wants_scan(c).  `allow_split` = false: the split
// decoder's scratch was not to be had, the plan for the decoders that need little or none.
static inline DecodePlan plan_decompress(const DecodeCall& c, const DecodeScan& scan, const DecodeDevice& d, bool allow_split = true) {
    const char* const force = forced_decoder();
    const bool scanned = decode_wants_scan(c);
    const DecodeScan s = scanned ? scan : DecodeScan();
    const size_t n = c.n_streams;
    DecodePlan p = {};
    p.max_wbits = c.bits();
    // streams above the limit fail with TAMP_INVALID_CONF under either value; nothing valid exceeds `found`
    if (scanned && s.found >= 8 && s.found < p.max_wbits) p.max_wbits = (uint8_t)s.found;
    if (scanned && s.found == 0) p.max_wbits = 8;
    const uint32_t wbits = p.max_wbits;
    const bool valid_bits = wbits >= 8 && wbits <= 15;
    p.bulk = s.longest_in >= 512;
    const WaveGeometry wave = wave_geometry(wbits, n, d.cu_count);

    // Split decoder: parse one lane per stream without any window, resolve by pointer jumping in LDS.  Needs the pre-pass (longest
    // stream and largest out_cap size its scratch and LDS) and out_cap up to 16 KiB.  Taken from 256 streams on for streams of 512
    // compressed bytes and more, and for short messages unless they are window 2^8 without a custom dictionary: the split decoder
    // has no window to set up, the lane decoders fill one per message (1 Mi x 256 B: custom dictionary at w = 8 1.30 against
    // 2.18 ms, default window 2^10 2.01 against 6.13 ms, 1 Mi x 512 B at w = 9 3.2 against 20.4 ms; w = 8 without a dictionary stays
    // with the LDS lanes, 1.65 against 1.98 ms.  tools/dec_short.py).
    const bool split_fits = valid_bits && s.max_out_cap && s.max_out_cap <= kSplitMaxOut && s.longest_in != 0xFFFFFFFFu;
    const bool short_split = s.longest_in < 512 && (c.has_dict || wbits >= 9);
    const bool want_split = force ? force[0] == 's' : ((s.longest_in >= 512 || short_split) && n >= 256);
    if (allow_split && want_split && split_fits) {
        p.decoder = Decoder::kSplit, p.split = split_geometry(c, s, d), p.wave = wave, p.wave_lds = decode_wave_lds(wbits, wave.waves);
        return p;
    }
    // Three more decoders.  Wave per stream: time follows the total bytes, needs few streams.  Lane per stream with the windows in
    // LDS: rounds of `capacity` streams (the rows limit the resident lanes), a round lasts as long as its longest stream, about
    // twice as fast per byte -- taken when a single round is reasonably full, and for batches of short messages.  Lane per stream
    // with the windows in a global slab: no capacity limit, every wave resident at once and the memory latency hidden by the other
    // waves of the SIMD -- taken for large batches of long streams, whatever their windows (mixed-window batches included).
    bool lds_lanes = false, global_lanes = false;
    LaneLdsGeometry lane = {};
    if (valid_bits && wbits <= kLdsWinBits) lane = lane_lds_geometry(wbits, p.bulk, n, d.cu_count);
    const size_t capacity = (size_t)d.cu_count * lane.per_cu * kWave;  // (0: the windows do not fit LDS)
    if (valid_bits && !p.bulk) {
        const size_t rounds = capacity ? (n + capacity - 1) / capacity : 1;
        lds_lanes = capacity && n * 10 >= rounds * capacity * 2;
    } else if (valid_bits && capacity && wbits <= 9) {
        // small windows: four and more waves of rows fit a CU's LDS, nothing beats that
        const size_t rounds = (n + capacity - 1) / capacity;
        lds_lanes = n * 10 >= rounds * capacity * 6;
    } else if (valid_bits) {
        lds_lanes = capacity && n * 10 >= capacity * 6 && n * 4 <= capacity * 5;
        global_lanes = !lds_lanes && n >= (size_t)d.cu_count * 192;  // ~3/4 wave per SIMD and up
    }
    if (force) lds_lanes = force[0] == 'l', global_lanes = force[0] == 'g';
    // (forced "split" that did not fit is neither of the three letters: no wave decoder for it, LDS lanes up to 2^10 windows and the slab above)
    const bool use_wave = force ? force[0] == 'w' : !(lds_lanes || global_lanes);
    if (valid_bits && use_wave) {
        p.decoder = Decoder::kWave, p.wave = wave, p.wave_lds = decode_wave_lds(wbits, wave.waves);
    } else if (valid_bits && wbits <= kLdsWinBits && !global_lanes) {
        p.decoder = Decoder::kLaneLds, p.lane = lane;  // (forced "lane" above 2^10 windows falls to the slab as well)
    } else {
        p.decoder = Decoder::kLaneGlobal, p.global = lane_global_geometry(wbits, valid_bits, p.bulk, c, s, d.cu_count);
    }
    return p;
}

}  // namespace tamp_amd
