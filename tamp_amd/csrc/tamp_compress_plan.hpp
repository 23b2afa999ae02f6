// tamp_compress_plan.hpp -- HOW a compress batch is launched: build, epoch block, LDS layout, workgroup size, grid.
// plan_compress is host arithmetic over the call and the tuning environment (no HIP call); both launchers and both queries use it.
#pragma once
#include <algorithm>
#include <cstdlib>
#include "tamp_amd.h"
#include "tamp_compress_kernel.hpp"

namespace tamp_amd {

// header byte 0 of a stream from its five fields, compressor.c:236-241 (read back by decompressor.c:276-297)
template <class Conf> static inline uint8_t header_byte(const Conf* c, bool dictionary_reset) {  // (TampAmdConf or TampConf)
    return (uint8_t)(((c->window - 8) << 5) | ((c->literal - 5) << 3) | (!!c->use_custom_dictionary << 2) | (!!c->extended << 1) | dictionary_reset);
}

// What a call asks for, as far as the plan depends on it.  compress_call(): a plain whole-stream batch, opening with the header.
struct CompressCall {
    const TampAmdConf* conf;
    uint32_t max_in_len;  // longest stream of the batch, 0 = unknown
    uint8_t nlead;        // leading bytes 0..2 and (`lead`) what they are, first one in the high byte, as in CompressArgs
    uint16_t lead;        // (a plain call: the header byte, + a zero second byte when dictionary_reset is set)
    uint8_t seg_flags;    // kSegResume | kSegSave | kSegFlushToken | kSegPartial
    uintptr_t dict;       // device address of the custom dictionary, 0 without one (the seeded tables are aligned)
    bool has_state, block_mode;  // a per-stream window state is passed; launch_compress_blocks: a long stream over all workgroups
    bool dict_table = false;     // a *_dicts call: `dict` is the buffer of dictionaries, every stream has a row in dict_off
};
static inline CompressCall compress_call(const TampAmdConf* conf, uint32_t max_in_len, uintptr_t dictionary_address) {
    const bool reset = conf->dictionary_reset != 0;
    return {conf, max_in_len, (uint8_t)(reset ? 2 : 1), (uint16_t)(header_byte(conf, reset) << 8), 0,
            conf->use_custom_dictionary ? dictionary_address : uintptr_t(0), false, false};
}

// Every build of the compress kernel the library launches (the table of DESIGN.md 3.2), and the one place that names them.
enum class CompressBuild : uint8_t { kShortLean, kLeanU16, kLazyPacked, kLazyU16, kRuns, kRuns1024, kFixedExt, kFixedV1,
                                     kBlockLean, kBlockRuns, kBlockRuns1024 };
// `dicts`: the build's twin for a dictionary-table call (the fixed-geometry builds have none: fixed_build_for keeps such calls generic)
static inline auto compress_kernel_of(CompressBuild b, bool dicts = false) -> void (*)(CompressArgs) {
    if (dicts) switch (b) {
        case CompressBuild::kShortLean: return tamp_compress_dict_kernel<true, false, false, 0, 9>;
        case CompressBuild::kLeanU16: return tamp_compress_dict_kernel<false, false, false, 0, kHashBits, true>;
        case CompressBuild::kLazyPacked: return tamp_compress_dict_kernel<true, true, false, 0, kHashBits, true>;
        case CompressBuild::kLazyU16: return tamp_compress_dict_kernel<false, true, false, 0, kHashBits, true>;
        case CompressBuild::kRuns: return tamp_compress_dict_kernel<true, false, true, 0, kHashBits, true>;
        case CompressBuild::kRuns1024: return tamp_compress_dict_kernel<true, false, true, 1024, kHb1024, true>;
        case CompressBuild::kBlockLean: return tamp_compress_dict_kernel<true, false, false, 0, kHashBits, true, true>;
        case CompressBuild::kBlockRuns: return tamp_compress_dict_kernel<true, false, true, 0, kHashBits, true, true>;
        case CompressBuild::kBlockRuns1024: return tamp_compress_dict_kernel<true, false, true, 1024, kHb1024, true, true>;
        case CompressBuild::kFixedExt: case CompressBuild::kFixedV1: return nullptr;
    }
    switch (b) {
        case CompressBuild::kShortLean: return tamp_compress_kernel<true, false, false, 0, 9>;  // (512 buckets, one wavefront)
        case CompressBuild::kLeanU16: return tamp_compress_kernel<false, false, false, 0, kHashBits, true>;
        case CompressBuild::kLazyPacked: return tamp_compress_kernel<true, true, false, 0, kHashBits, true>;
        case CompressBuild::kLazyU16: return tamp_compress_kernel<false, true, false, 0, kHashBits, true>;
        case CompressBuild::kRuns: return tamp_compress_kernel<true, false, true, 0, kHashBits, true>;
        case CompressBuild::kRuns1024: return tamp_compress_kernel<true, false, true, 1024, kHb1024, true>;
        case CompressBuild::kFixedExt: return tamp_compress_fixed::compress_kernel<kFixExt>;
        case CompressBuild::kFixedV1: return tamp_compress_fixed::compress_kernel<kFixV1>;
        case CompressBuild::kBlockLean: return tamp_compress_kernel<true, false, false, 0, kHashBits, true, true>;
        case CompressBuild::kBlockRuns: return tamp_compress_kernel<true, false, true, 0, kHashBits, true, true>;
        case CompressBuild::kBlockRuns1024: return tamp_compress_kernel<true, false, true, 1024, kHb1024, true, true>;
    }
    return nullptr;
}

struct CompressPlan {  // (in the order plan_compress decides them)
    bool packed, lazy, runlist;  // packed: u32 index entries; 2^15 windows fall back to u16 positions
    bool long_streams;           // streams of 1 KiB and more, or of unknown length (= 256-thread workgroups)
    uint32_t hb;               // bucket bits of the LDS layout (the short build scans 512 buckets but keeps the full cursor region)
    uint32_t blk, threads;     // positions matched per epoch, threads per workgroup
    CompressLds lds;
    uint32_t reg_cap, per_cu;  // workgroups per CU: what the build's registers are budgeted for, and the estimate with this layout
    CompressBuild build;       // (tamp_amd_compress_build derives its TAMP_AMD_BUILD_* from it)
    bool persistent;           // as many workgroups as the device holds, claiming streams from a work counter
    uint32_t claim;            // ... this many per fetch
    bool dicts;                // a dictionary-table call: the build's DICTS twin (compress_kernel_of(build, dicts))
};

// Dynamic LDS of a launch of `p`'s kernel (and of the occupancy query about it).  The generic builds take the plan's whole layout
// this way.  The fixed-geometry builds declare the same bytes as a static array (lds_base in tamp_compress_kernel.hpp) and take
// none: handed over a second time they would count twice and halve the workgroups per CU.  What the plan REPORTS is one figure
// for both -- p.lds.total bytes per workgroup, p.per_cu workgroups -- however the bytes reach the kernel.
static inline uint32_t dynamic_lds(const CompressPlan& p) {
    if (p.build == CompressBuild::kFixedExt || p.build == CompressBuild::kFixedV1) return 0;
    return p.lds.total;
}

// Workgroups per CU: what the registers allow (8 for the run-aware builds, 6 lean, 5 lazy), and the estimate for a layout of `lds`
// bytes: 160 KiB per CU, handed out in coarse granules (26,960 B per workgroup measured as five per CU, 25,424 B as six).
static inline uint32_t register_cap(bool lazy, bool runlist) { return lazy ? kLazyPerCu : (runlist ? kWgPerCu : kLeanPerCu); }
static inline uint32_t workgroups_per_cu(uint32_t lds, uint32_t reg_cap) { return std::min(160u * 1024u / align_up(lds, 2048u), reg_cap); }

// Positions matched per epoch (a multiple of 64: the walk chases 64 positions per register; of 256 when it can be: the index is
// scattered in tiles of 256).  The whole stream when it is short; for longer ones the LARGEST block that still allows as many
// workgroups per CU as a 1,024-position block does (at W = 1024 that is 1,024 positions at eight per CU).
static inline uint32_t pick_block(uint32_t W, uint32_t max_in_len, bool packed, bool lazy, bool runlist, uint32_t hb, const char* blk_env) {
    uint32_t blk = max_in_len ? std::min(align_up(max_in_len, 64), 2048u) : 2048u;
    if (blk > 1024) {
        auto per_cu = [&](uint32_t b) { return workgroups_per_cu(CompressLds(W, b, packed, lazy, runlist, hb).total, register_cap(lazy, runlist)); };
        uint32_t best = 1024, want = per_cu(best);
        for (uint32_t b = 1280; b <= 2048; b += 256)
            if (b <= blk && per_cu(b) == want) best = b;
        // (the stream's own length: one epoch instead of two for streams a little over 1 KiB, when that costs no workgroup)
        if (blk > best && blk < 2048 && per_cu(blk) == want) best = blk;
        blk = best;
    }
    if (blk_env) { const uint32_t v = (uint32_t)atoi(blk_env); if (v >= 64 && v <= 2048) blk = align_up(v, 64); }
    if (blk < 64) blk = 64;
    // The cursor region of LDS also serves as the sorted query list (blk x u16) and, in the run-aware builds, as the walk's
    // explicit pieces + the step table (kSlowCap x 8 + blk bytes): a tuning override must not outgrow it.  (Checked here and
    // not by sizing the region from the block: that arithmetic inside the kernel cost the 64-VGPR builds their last register.)
    const uint32_t cur = (hb < kHashBits ? (1u << hb) : kHashBuckets) * 2;
    while (blk > 64 && (blk * 2 > cur || (runlist && kSlowCap * 8 + blk > cur))) blk -= 64;
    while (W + blk + 16 > 65536) blk >>= 1;  // 16-bit buffer positions
    return blk;
}

// Threads per workgroup for a block of `blk` positions: four wavefronts from 1,024 positions on, one below; a TAMP_AMD_BLK override
// that gives LONG streams 512..960 positions keeps the four.  The one definition: plan_compress calls it, the rest takes `threads`.
static inline uint32_t compress_threads(uint32_t blk, bool long_streams, bool blk_overridden) {
    return (blk >= 1024 || (long_streams && blk >= 512 && blk_overridden)) ? 256u : 64u;
}

// The fixed-geometry builds: kFixedExt / kFixedV1 when the call is EXACTLY what they were compiled for; for all
// else, and with TAMP_AMD_FIXED_BUILD=0 (`fixed_env`: A/B runs, parity tests), the generic build plan_compress has put into `p`.
static inline CompressBuild fixed_build_for(const CompressCall& c, const CompressPlan& p, const char* fixed_env) {
    const TampAmdConf* conf = c.conf;
    const bool fits = !c.block_mode && !c.dict_table && !(fixed_env && atoi(fixed_env) == 0) && conf->window == kFixWbits && conf->literal == kFixLbits &&
                      !p.lazy && p.runlist && p.blk == kFixBlk && p.threads == kFixThreads && !c.has_state && c.seg_flags == 0 &&
                      !conf->dictionary_reset && c.nlead == 1 && c.lead == header_byte(conf, false) << 8 && (c.dict & 3) == 0;
    return !fits ? p.build : (conf->extended ? CompressBuild::kFixedExt : CompressBuild::kFixedV1);
}

// The launch decisions for `c`.  The planning overrides are read here and nowhere else.
static inline CompressPlan plan_compress(const CompressCall& c) {
    using B = CompressBuild;
    const char *const blk_env = getenv("TAMP_AMD_BLK"), *const runs_env = getenv("TAMP_AMD_RUNS");
    const char *const fixed_env = getenv("TAMP_AMD_FIXED_BUILD"), *const block_lean_env = getenv("TAMP_AMD_BLOCK_LEAN");
    const TampAmdConf* conf = c.conf;
    const uint32_t W = 1u << conf->window;
    const bool w10 = conf->window == 10, packed = conf->window <= kPackedMaxWbits, lazy = conf->lazy_matching != 0, block = c.block_mode;
    // The run-aware build (u32 entries, default parse only): streams of 1 KiB and more always, so the hint and
    // TAMP_AMD_RUNS (tuning / tests) matter for short messages alone; block mode too (TAMP_AMD_BLOCK_LEAN, tuning: the lean build).
    const bool long_streams = block || c.max_in_len == 0 || align_up(c.max_in_len, 64) >= 1024;
    bool runlist = packed && !lazy && (long_streams || conf->input_hint == TAMP_AMD_HINT_RUNS);
    if (runs_env && !long_streams) runlist = packed && !lazy && atoi(runs_env) != 0;
    if (block && block_lean_env) runlist = false;
    const uint32_t hb = runlist && w10 ? kHb1024 : kHashBits;
    uint32_t blk = pick_block(W, block ? 0 : c.max_in_len, packed, lazy, runlist, hb, blk_env);
    if (block && blk > 1024) blk = 1024;  // (an unknown length's block, but more, smaller ones: block mode's unit of parallelism)
    const uint32_t threads = block ? 256u : compress_threads(blk, long_streams, blk_env != nullptr);
    CompressPlan p = {packed, lazy, runlist, long_streams, hb, blk, threads, CompressLds(W, blk, packed, lazy, runlist, hb)};
    p.reg_cap = register_cap(lazy, runlist), p.per_cu = workgroups_per_cu(p.lds.total, p.reg_cap);
    p.build = block ? (!runlist ? B::kBlockLean : (w10 ? B::kBlockRuns1024 : B::kBlockRuns))  // (v1, default parse, windows <= 2^14)
              : lazy ? (packed ? B::kLazyPacked : B::kLazyU16)
              : !packed ? B::kLeanU16
              : runlist ? (w10 ? B::kRuns1024 : B::kRuns) : B::kShortLean;
    p.build = fixed_build_for(c, p, fixed_env);
    // All but the short-message build run as a PERSISTENT GRID (LOOP in the kernel).  Streams per fetch: one for
    // 256-thread workgroups (1 KiB and more; block mode's blocks), sixteen for one-wavefront ones (lazy / 2^15 / hinted short).
    p.persistent = p.build != B::kShortLean, p.claim = (!p.persistent || p.threads == 256) ? 1u : 16u;
    p.dicts = c.dict_table;
    return p;
}

}  // namespace tamp_amd
