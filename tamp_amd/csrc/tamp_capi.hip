// tamp_capi.hip -- the C ABI of include/tamp_amd.h over the gfx950 kernels.
//
// Thin host shim: argument checks, H2D/D2H staging for host buffers, launch geometry, the seeded
// default dictionaries (tamp/_c_src/tamp/common.c:18-52, computed once per device and kept in HBM),
// and the hipEvent timing hook bench.py reads.  All codec work happens in the kernels; there is no
// CPU code path for it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <functional>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <cstring>

#include "tamp_amd.h"
#include "tamp_compat.h"
#include "tamp_host_stage.hpp"
#include "tamp_compress_kernel.hpp"
#include "tamp_compress_plan.hpp"
#include "tamp_decompress_kernel.hpp"
#include "tamp_decompress_split_kernel.hpp"
#include "tamp_decompress_long_kernel.hpp"
#include "tamp_decompress_wave_kernel.hpp"
#include "tamp_decompress_plan.hpp"
#include "tamp_decompress_resume_kernel.hpp"
#include "tamp_decoded_size_pieces_kernel.hpp"
#include "tamp_compress_resume_kernel.hpp"
#include "tamp_reset_segments_kernel.hpp"
#include "tamp_read_ranges_kernel.hpp"
#include "tamp_segment_ends_kernel.hpp"
#include "tamp_write_ranges_kernel.hpp"
#include "tamp_append_kernel.hpp"
#include "tamp_reset_index_kernel.hpp"
#include "tamp_pack_kernel.hpp"
#include "tamp_pieces_kernel.hpp"
#include "tamp_seek_kernel.hpp"

using namespace tamp_amd;

namespace {

constexpr int kMaxDevices = 64;
constexpr size_t kSeedTable = (size_t)1 << 15;

// A buffer the library keeps between calls and grows on demand (the contents do not survive growth).  Device memory or
// pinned host memory: the two differ in the allocate / free pair only.
template <hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
struct GrowBuf {
    void* p = nullptr;
    size_t bytes = 0;
    // `headroom`: 25 % + 4 KiB on top, so that slowly growing batches do not allocate on every call (off for the decoders'
    // slabs, which are sized from a memory budget)
    hipError_t need(size_t n, bool headroom = true) {
        if (n <= bytes) return hipSuccess;
        release();
        if (headroom) n += n / 4 + 4096;
        hipError_t e = Alloc(&p, n);
        if (e == hipSuccess) bytes = n;
        else p = nullptr;
        return e;
    }
    size_t release() {  // -> the bytes freed
        const size_t n = p ? bytes : 0;
        if (p) (void)Free(p);
        p = nullptr, bytes = 0;
        return n;
    }
};
hipError_t device_alloc(void** p, size_t n) { return hipMalloc(p, n); }
hipError_t pinned_alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
using DeviceBuf = GrowBuf<device_alloc, hipFree>;
using PinnedBuf = GrowBuf<pinned_alloc, hipHostFree>;

// The device scratch kept between calls, one record per HIP stream of the caller: launches on one stream are ordered and
// share its buffers (the next call's kernels find the previous call's done with them), launches on different streams run
// concurrently and do not.
// LOCK RULE.  DeviceCtx::scratch(st) holds the map's mutex for the look-up only.  `mu` is taken at the top of
// launch_compress, launch_compress_resets, launch_compress_batch_resets, launch_decompress, launch_read_ranges,
// launch_write_ranges, launch_append, launch_index_resets, launch_segment_ends, launch_pack and launch_pieces and held to the
// call's last launch: one library call at a time enqueues on a stream and may touch its record.  Under it the members are used
// directly -- no second lock, no pointer that outlives the lock -- and the record is passed down (launch_compress_locked,
// launch_compress_blocks, launch_decompress_long): `mu` is not recursive.
// tamp_amd_trim takes `mu` and drains the stream before it frees, so it can neither free what a call is about to launch
// with nor what a launched kernel still uses.
// A host-memory call (HostCall below) holds the host pipeline's mutex; where it takes a record's `mu` as well, the pipeline's
// comes FIRST and the record's second, never the reverse (read_ranges_host, batch_append).
struct StreamScratch {
    std::mutex mu;
    DeviceBuf slab;        // lane decoder with the windows in global memory: one window slot per resident lane
    DeviceBuf split;       // split decoder: token records, per-stream meta words, lag lists, fallback flags
    DeviceBuf scan;        // header pre-pass: largest window / longest stream / window bytes / largest out_cap (32 bytes, never trimmed)
    DeviceBuf blk;         // block mode (one long v1 stream over all workgroups): tables of pass 1, positions of pass 2, match results
    DeviceBuf lpt;         // expensive-first ordering of a compress batch: scores, order, gathered table rows
    DeviceBuf long_tab;    // one long stream decoded by the whole device: chunk tables, records, group tables
    DeviceBuf long_tails;  // ... the groups' tail maps (groups x window x 2 bytes)
    DeviceBuf long_lags;   // ... extended format: the list of tokens that can lag, the lag lists
    DeviceBuf resets;      // dictionary-reset segments: the slice's table rows and output slabs (launch_compress_resets), a batch's per-stream words in front (launch_compress_batch_resets)
    DeviceBuf pack;        // tamp_batch_pack: the scan's per-workgroup sums (8 KiB, allocated once)
    DeviceBuf ranges;      // tamp_batch_read_ranges: the per-range scans and verdicts (the units, stage and scratch of a slice: `resets`)
    DeviceBuf ends;        // tamp_batch_segment_ends: the scan's per-workgroup sums (16 KiB, allocated once)
    DeviceBuf writes, write_units;  // tamp_batch_write_ranges: its tables per stream and per segment; the rows, staging rows and slabs of a slice's units
    DeviceBuf appends, append_units;  // tamp_batch_append: its tables per stream; the staged entries of the new index, then the rows, staging rows and slabs of a slice's units
    DeviceBuf index_streams, index_chunks, index_entries;  // tamp_batch_index_resets: its tables per stream, per chunk, per entry
    DeviceBuf pieces, piece_rows;  // tamp_batch_compress_pieces: its record and tables per object and per row; the state rows and input rows
    DeviceBuf seek, seek_units;  // tamp_batch_read_ranges_seek: the per-range scan, byte counts, flags and verdicts; the unit table
    // In front of slab.need / split.need: kernels of earlier calls on the stream may still use a buffer that this call has
    // outgrown, so the stream is drained before it is freed.  (The tables of the other members are freed by need() alone:
    // hipFree waits for the device.)
    static hipError_t drain_if_outgrown(DeviceBuf& b, size_t n, hipStream_t st) {
        if (!b.p || n <= b.bytes) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(st);
        if (e == hipSuccess) b.release();
        return e;
    }
    size_t release() {  // -> the bytes freed (tamp_amd_trim, under `mu`, the stream drained)
        size_t n = 0;
        for (DeviceBuf* b : {&slab, &split, &blk, &lpt, &long_tab, &long_tails, &long_lags, &resets, &pack, &ranges, &ends, &writes, &write_units, &appends, &append_units, &index_streams, &index_chunks, &index_entries, &pieces, &piece_rows, &seek, &seek_units}) n += b->release();
        return n;
    }
};

struct DeviceCtx {
    bool ready = false;
    int cu_count = 0;
    size_t lds_per_block = 0;
    uint8_t* seed_dicts = nullptr;  // 3 x 32 KiB: literal<=5, ==6, >=7
    uint32_t* work_counters = nullptr;  // persistent-grid builds: one stream counter per launch, handed out round robin
    std::atomic<uint32_t> next_counter{0};
    static constexpr uint32_t kCounters = 4096;
    std::mutex scratch_mu;  // guards the map below, never a record's fields
    std::map<hipStream_t, StreamScratch> scratch_of;
    StreamScratch& scratch(hipStream_t st) {
        std::lock_guard<std::mutex> lock(scratch_mu);
        return scratch_of[st];  // (map nodes do not move)
    }
    // host-memory batch calls (TAMP_AMD_MEM_HOST): kept staging buffers and the library's own streams, so that a
    // call costs no hipMalloc and a large batch runs as overlapping chunks (copy in / kernel / copy out)
    struct HostPipe {
        static constexpr int kDepth = 3;
        std::mutex mu;  // one host-memory batch call per device at a time
        hipStream_t s[kDepth] = {nullptr, nullptr, nullptr};
        DeviceBuf in[kDepth], out[kDepth], meta[kDepth], state[kDepth], dict;  // (state: the rows of HostBatch::states)
        // pinned host staging for output slabs that do not tile their extent (gaps, padding, permuted offsets): the chunk's
        // extent comes back in ONE transfer and the produced bytes are placed by the host
        PinnedBuf stage[kDepth];
    } pipe;
};

DeviceCtx g_ctx[kMaxDevices];
std::mutex g_mu;

thread_local bool t_timing = false;
thread_local hipEvent_t t_ev0 = nullptr, t_ev1 = nullptr;
thread_local bool t_ev_valid = false;

thread_local char t_last_error[512] = "";
unsigned long long* g_prof = nullptr;  // -DTAMP_PROF builds: device buffer of per-phase cycle sums

#define HIP_OK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) {                                                                           \
            snprintf(t_last_error, sizeof t_last_error, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,     \
                     hipGetErrorString(_e));                                                              \
            return TAMP_AMD_NO_DEVICE;                                                                    \
        }                                                                                                 \
    } while (0)

// One host-memory call on the pipeline's first stream: it holds P.mu (one such call per device at a time) and, behind open(),
// P.s[0] exists.  Every way out of the call drains that stream: the call's copies go to and from its own vectors and the
// caller's arrays, and none of them may still be in flight when those go away -- so a local that an asynchronous copy reads or
// writes is declared IN FRONT of the HostCall and outlives the drain.  (Behind the last wait of a call that completes: nothing.)
struct HostCall {
    DeviceCtx::HostPipe& P;
    std::lock_guard<std::mutex> pipe_lock;
    hipStream_t st = nullptr;
    explicit HostCall(DeviceCtx* ctx) : P(ctx->pipe), pipe_lock(P.mu) {}
    int open() {  // -> TAMP_OK, or TAMP_AMD_NO_DEVICE with the error text set: the call returns it
        if (!P.s[0]) HIP_OK(hipStreamCreateWithFlags(&P.s[0], hipStreamNonBlocking));
        st = P.s[0];
        return TAMP_OK;
    }
    ~HostCall() {
        if (st && hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
    }
};

// The produced bytes of a host-memory call's slabs, back to the caller: row i's len[i] bytes from d_slab + d_off[i] to
// out + out_off[i].  Through ONE pinned transfer of the slabs' extent when that is at most 512 MiB (the rows are placed by the
// host), else -- or with the debugging switch below set, or without the pinned memory -- row by row; nothing when no row
// produced a byte.  The stream is idle when it returns TAMP_OK.
int copy_back_slabs(DeviceCtx::HostPipe& P, hipStream_t st, const uint8_t* d_slab, uint64_t extent, const uint64_t* d_off, uint8_t* out,
                    const uint64_t* out_off, const uint32_t* len, size_t n) {
    uint64_t produced = 0;
    for (size_t i = 0; i < n; i++) produced += len[i];
    if (!produced) return TAMP_OK;
    if (extent <= ((uint64_t)512 << 20) && !getenv("TAMP_AMD_NO_STAGED_COPYBACK") && P.stage[0].need(extent) == hipSuccess) {
        const uint8_t* const stg = static_cast<const uint8_t*>(P.stage[0].p);
        HIP_OK(hipMemcpyAsync(P.stage[0].p, d_slab, extent, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (size_t i = 0; i < n; i++)
            if (len[i]) memcpy(out + out_off[i], stg + d_off[i], len[i]);
        return TAMP_OK;
    }
    (void)hipGetLastError();  // (a failed pinned allocation must not poison later calls)
    for (size_t i = 0; i < n; i++)
        if (len[i]) HIP_OK(hipMemcpyAsync(out + out_off[i], d_slab + d_off[i], len[i], hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return TAMP_OK;
}

void seed_dictionary_host(unsigned char* buf, size_t size, uint8_t literal) {
    // common.c:18-52: xorshift32 from 3758097560, one draw per 8 bytes, nibble selects from a 16-entry table.
    static const char text16[] = " etaoinshrdlcumw";
    static const unsigned char markup16[16] = {' ', 0, '0', 'e', 'i', '>', 't', 'o', '<', 'a', 'n', 's', '\n', 'r', '/', '.'};
    unsigned char table[16];
    for (int k = 0; k < 16; k++)
        table[k] = literal <= 5 ? (unsigned char)(text16[k] & 0x1F)
                                : (literal == 6 ? (unsigned char)(text16[k] & 0x3F) : markup16[k]);
    uint32_t s = 3758097560u, draw = 0;
    for (size_t i = 0; i < size; i++) {
        if ((i & 7) == 0) {
            s ^= s << 13;
            s ^= s >> 17;
            s ^= s << 5;
            draw = s;
        }
        buf[i] = table[draw & 15];
        draw >>= 4;
    }
}

int get_ctx(int device, DeviceCtx** out) {
    if (device < 0 || device >= kMaxDevices) return TAMP_AMD_BAD_ARGUMENT;
    int count = 0;
    HIP_OK(hipGetDeviceCount(&count));
    if (device >= count) {
        snprintf(t_last_error, sizeof t_last_error, "device %d requested, %d visible", device, count);
        return TAMP_AMD_NO_DEVICE;
    }
    HIP_OK(hipSetDevice(device));
    std::lock_guard<std::mutex> lock(g_mu);
    DeviceCtx& c = g_ctx[device];
    if (!c.ready) {
        hipDeviceProp_t prop;
        HIP_OK(hipGetDeviceProperties(&prop, device));
        c.cu_count = prop.multiProcessorCount;
        c.lds_per_block = prop.sharedMemPerBlock;
        std::vector<unsigned char> host(3 * kSeedTable);
        seed_dictionary_host(host.data() + 0 * kSeedTable, kSeedTable, 5);
        seed_dictionary_host(host.data() + 1 * kSeedTable, kSeedTable, 6);
        seed_dictionary_host(host.data() + 2 * kSeedTable, kSeedTable, 8);
        HIP_OK(hipMalloc(&c.seed_dicts, 3 * kSeedTable));
        HIP_OK(hipMemcpy(c.seed_dicts, host.data(), 3 * kSeedTable, hipMemcpyHostToDevice));
        HIP_OK(hipMalloc(&c.work_counters, DeviceCtx::kCounters * sizeof(uint32_t)));
        c.ready = true;
    }
    *out = &c;
    return TAMP_OK;
}

thread_local bool t_timing_outer = false;  // a caller's event pair spans several inner launches (up to sixteen long streams)
void timing_begin(hipStream_t st) {
    if (t_timing_outer) return;
    t_ev_valid = false;
    if (!t_timing) return;
    if (!t_ev0) {
        (void)hipEventCreate(&t_ev0);
        (void)hipEventCreate(&t_ev1);
    }
    (void)hipEventRecord(t_ev0, st);
}
void timing_end(hipStream_t st) {
    if (!t_timing) return;
    (void)hipEventRecord(t_ev1, st);
    t_ev_valid = true;
}

// One event pair around all kernels of a call that makes inner launches (they do not open their own), ended on every way out of it.
struct CallTiming {
    hipStream_t st;
    explicit CallTiming(hipStream_t s) : st(s) { timing_begin(st), t_timing_outer = true; }
    ~CallTiming() { t_timing_outer = false, timing_end(st); }
    CallTiming(const CallTiming&) = delete;
    CallTiming& operator=(const CallTiming&) = delete;
};

struct SegmentSpec {  // streaming Compressor over the engine: how this piece of the stream opens and closes
    uint8_t nlead;
    uint16_t lead;
    uint8_t flags;  // kSegResume | kSegSave | kSegFlushToken | kSegPartial
};

// The per-stream tables of a batch call, from the C entry points down to the kernels' argument blocks: one row per stream, the
// data buffers the offsets point into, the dictionary bytes.  The pointers are the caller's (host or device memory, as the call
// says) or, inside the host pipeline, one chunk's staging buffers.  A column is added here, in rows() and in the *_args functions.
struct BatchTables {
    const uint8_t* in = nullptr;
    const uint64_t* in_off = nullptr;
    const uint32_t* in_len = nullptr;
    uint8_t* out = nullptr;              // null, with out_off: the size query (out_cap holds the limits, may be null)
    const uint64_t* out_off = nullptr;
    const uint32_t* out_cap = nullptr;
    uint32_t* out_len = nullptr;
    int8_t* status = nullptr;
    uint32_t* in_consumed = nullptr;     // may be null
    const uint64_t* dict_off = nullptr;  // the *_dicts calls, else null: stream i's dictionary is dict + dict_off[i], inside dict_len bytes
    const uint8_t* dict = nullptr;
    size_t dict_len = 0;
    size_t n = 0;
    // Rows [i0, i0 + count): every table shifted, null tables stay null, the data pointers stay (offsets are absolute).  The only
    // place where a table pointer is advanced by a stream index.
    BatchTables rows(size_t i0, size_t count) const {
        BatchTables t = *this;
        auto shift = [i0](auto*& p) { if (p) p += i0; };
        shift(t.in_off), shift(t.in_len), shift(t.out_off), shift(t.out_cap), shift(t.out_len), shift(t.status);
        shift(t.in_consumed), shift(t.dict_off);
        t.n = count;
        return t;
    }
};

// Expensive streams first (round 5).  One stream = one workgroup, so a batch cannot finish before its slowest stream does, and
// a batch of only a few rounds of the persistent grid -- 3,052 streams per GPU when BASELINE configs[2] runs on eight -- waits
// for whichever slow stream happened to start last.  What makes a stream slow are its lags and searches, and a
// cheap proxy ranks them well: the number of ALIGNED DWORDS OF FOUR EQUAL BYTES (of the stand-in's 2,304 chunks the slowest
// ones rank 0-7 of 768 by it on prose, 1-57 on Python sources).  Three tiny kernels around the compress launch: score per
// stream, one-workgroup counting sort (descending), the batch's tables gathered in that order -- the compress kernel reads
// row i of the gathered tables, so its claims ARE the order -- and sizes / statuses scattered back afterwards.
__global__ void __launch_bounds__(256) tamp_stream_score_kernel(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                                                 uint32_t n_streams, uint32_t* score) {
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= n_streams) return;
    const uint8_t* p = in + in_off[s];
    const uint32_t n = in_len[s];
    const uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(p) & 3)) & 3);
    uint32_t cnt = 0;
    if (n > head + 4) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p + head);
        const uint32_t nw = (n - head) >> 2;
        for (uint32_t k = lane; k < nw; k += 64) {
            const uint32_t d = w[k];
            cnt += d == (d & 0xFFu) * 0x01010101u;
        }
    }
    cnt = wave_scan_add(cnt);  // (inclusive scan: the last lane holds the sum)
    if (lane == 63) score[s] = cnt;
}
__global__ void __launch_bounds__(1024) tamp_stream_order_kernel(const uint32_t* score, uint32_t n_streams, uint32_t* order) {
    // counting sort by min(score, 1023), descending, one workgroup.  Lanes of a wavefront that hold the same bin go to the LDS
    // counter together (one atomic per distinct bin and wavefront: a batch whose streams all score alike -- synthetic text:
    // zero everywhere -- would otherwise queue 65,536 atomics on one word, 0.11 ms)
    __shared__ uint32_t bins[1024];
    __shared__ uint32_t wsum[16];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    auto grouped_add = [&](uint32_t bin, bool live) -> uint32_t {  // -> this lane's slot in its bin
        uint32_t slot = 0;
        uint64_t todo = __ballot(live);
        while (todo) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
            const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bin, (int)leader);
            const uint64_t same = __ballot(live && bin == b) & todo;
            // (real text: the 64 streams of a wavefront score 30-60 different values, and a round of this loop per value
            // is a dependent LDS atomic each -- 0.18-0.34 ms per 32,768 streams.  Small groups go to the counters one lane
            // each, which the LDS serves in parallel: 0.0x ms)
            if (__builtin_popcountll(same) < 8) break;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&bins[b], (uint32_t)__builtin_popcountll(same));
            base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)leader);
            if (live && bin == b) slot = base + (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1));
            todo &= ~same;
        }
        if ((todo >> lane) & 1ull) slot = atomicAdd(&bins[bin], 1u);
        return slot;
    };
    const uint32_t rounds = (n_streams + 1023) / 1024;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t s = r * 1024 + threadIdx.x;
        const bool live = s < n_streams;
        (void)grouped_add(live ? 1023u - min(score[s], 1023u) : 0u, live);
    }
    __syncthreads();
    const uint32_t v = bins[threadIdx.x];  // exclusive scan of the 1,024 bins: 16 wavefronts
    const uint32_t incl = wave_scan_add(v);
    if (lane == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) base += wsum[w];
    bins[threadIdx.x] = base + incl - v;
    __syncthreads();
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t s = r * 1024 + threadIdx.x;
        const bool live = s < n_streams;
        const uint32_t slot = grouped_add(live ? 1023u - min(score[s], 1023u) : 0u, live);
        if (live) order[slot] = s;
    }
}
// (the dictionary-table column of a *_dicts call, in the same order)
__global__ void tamp_gather_u64_kernel(const uint32_t* order, uint32_t n, const uint64_t* src, uint64_t* dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[order[i]];
}
__global__ void tamp_gather_rows_kernel(const uint32_t* order, uint32_t n, const uint64_t* in_off, const uint32_t* in_len,
                                        const uint64_t* out_off, const uint32_t* out_cap, uint64_t* g_in_off, uint32_t* g_in_len,
                                        uint64_t* g_out_off, uint32_t* g_out_cap) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = order[i];
    g_in_off[i] = in_off[s], g_in_len[i] = in_len[s], g_out_off[i] = out_off[s], g_out_cap[i] = out_cap[s];
}
__global__ void tamp_scatter_results_kernel(const uint32_t* order, uint32_t n, const uint32_t* g_out_len, const int8_t* g_status,
                                            uint32_t* out_len, int8_t* status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = order[i];
    out_len[s] = g_out_len[i], status[s] = g_status[i];
}

// Block mode, pass 2: entry offset and bit position of every block from the tables of pass 1 -- a chain of one dependent
// table look-up per block.  Two levels keep it short: chunks of 512 blocks.  tamp_block_scan_chunks: per chunk, for each of
// the 15 entry offsets (a lane each) where the chain leaves the chunk and the bits it takes.  tamp_block_scan_kernel: per
// chunk, the chain over the CHUNK tables in front of it (a few hundred steps at most for 4 GiB), then the chunk's own 512
// blocks from its true entry.  (One workgroup walking all 97,657 blocks of a 100 MB stream took 4 ms of the call's 11.)
constexpr uint32_t kScanChunk = 512;
__global__ void __launch_bounds__(256) tamp_block_scan_chunks(const uint32_t* table, uint32_t* chunk_table /* n_chunks x 16 x 2 */,
                                                              uint32_t n_blocks) {
    __shared__ uint32_t t[kScanChunk * 16];
    const uint32_t b0 = blockIdx.x * kScanChunk;
    const uint32_t cnt = n_blocks - b0 < kScanChunk ? n_blocks - b0 : kScanChunk;
    for (uint32_t i = threadIdx.x; i < cnt * 16; i += blockDim.x) t[i] = table[(size_t)b0 * 16 + i];
    __syncthreads();
    if (threadIdx.x < 16) {
        uint32_t entry = threadIdx.x;
        unsigned long long bits = 0;
        if (threadIdx.x < 15)
            for (uint32_t i = 0; i < cnt; i++) {
                const uint32_t v = t[i * 16 + entry];
                entry = v & 15u;
                bits += v >> 4;
            }
        // (exit offset | bits << 4 does not fit 32 bits for 512 blocks of 9 Kbit: two words)
        chunk_table[((size_t)blockIdx.x * 16 + threadIdx.x) * 2] = entry;
        chunk_table[((size_t)blockIdx.x * 16 + threadIdx.x) * 2 + 1] = (uint32_t)bits;
    }
}
__global__ void __launch_bounds__(256) tamp_block_scan_kernel(const uint32_t* table, const uint32_t* chunk_table, unsigned long long* info,
                                                              uint32_t n_blocks, uint32_t lead_bits) {
    __shared__ uint32_t t[kScanChunk * 16];
    __shared__ unsigned long long res[kScanChunk];
    const uint32_t b0 = blockIdx.x * kScanChunk;
    const uint32_t cnt = n_blocks - b0 < kScanChunk ? n_blocks - b0 : kScanChunk;
    for (uint32_t i = threadIdx.x; i < cnt * 16; i += blockDim.x) t[i] = table[(size_t)b0 * 16 + i];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long bp = lead_bits;
        uint32_t entry = 0;
        for (uint32_t c = 0; c < blockIdx.x; c++) {  // the chunks in front of this one
            const uint32_t* e = chunk_table + ((size_t)c * 16 + entry) * 2;
            bp += e[1];
            entry = e[0];
        }
        for (uint32_t i = 0; i < cnt; i++) {
            res[i] = (bp << 4) | entry;
            const uint32_t v = t[i * 16 + entry];
            entry = v & 15u;
            bp += v >> 4;
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) info[b0 + i] = res[i];
}

// The kernel's argument block as conf, the call's lead, the dictionary and the batch's tables decide it.  The plan adds the block
// and the claim.  (Value-initialised: no work counter, first stream 0, none of the block-mode tables.)
void set_tables(CompressArgs& a, const BatchTables& t) {
    a.in = t.in, a.in_off = t.in_off, a.in_len = t.in_len, a.n_streams = (uint32_t)t.n;
    a.out = t.out, a.out_off = t.out_off, a.out_cap = t.out_cap, a.out_len = t.out_len, a.status = t.status;
    a.dict_off = t.dict_off, a.dict_len = t.dict_len;
}
CompressArgs fill_compress_args(const DeviceCtx* ctx, const CompressCall& call, const BatchTables& t, uint8_t* d_state) {
    const TampAmdConf* conf = call.conf;
    const uint8_t* const d_dict = t.dict;
    CompressArgs a = {};
    set_tables(a, t);
    a.wbits = conf->window, a.lbits = conf->literal, a.extended = conf->extended != 0;
    a.dict_reset = conf->dictionary_reset != 0, a.lazy = conf->lazy_matching != 0, a.prof = g_prof, a.claim = 1;
    a.nlead = call.nlead, a.lead = call.lead, a.seg_flags = call.seg_flags, a.state = call.has_state ? d_state : nullptr;
    // compressor.c:224-225: non-extended streams always use the literal-8 table
    const int lit = conf->extended ? conf->literal : 8;
    a.dict = conf->use_custom_dictionary ? d_dict : ctx->seed_dicts + (lit <= 5 ? 0 : (lit == 6 ? 1 : 2)) * kSeedTable;
    // epoch cut at long runs (extended format only: the v1 format has no RLE token), tamp_compress_kernel.hpp
    a.cut_run = conf->extended ? 3u : 0u;  // (doubles per stream whenever a cut turns out to be superfluous)
    if (const char* e = getenv("TAMP_AMD_CUT_RUN")) { const int v = atoi(e); a.cut_run = (conf->extended && v >= 2 && v <= 64) ? (uint32_t)v : 0u; }
    a.dbg = getenv("TAMP_AMD_DBG") ? (uint32_t)atoi(getenv("TAMP_AMD_DBG")) : 0;
    return a;
}

// What the two compress launchers do with a plan.  prepare_compress_kernel: the dynamic-LDS attribute of the plan's kernel and, for
// a persistent grid, how many of its workgroups a CU holds (the occupancy query costs ~10 us: once per shape).  launch_on_counter:
// a work-counter slot, zeroed, and the launch over it.  (Two steps: the grid is sized, checked and used between them.)
int prepare_compress_kernel(const CompressPlan& p, int* per_cu) {
    const void* const kernel = reinterpret_cast<const void*>(compress_kernel_of(p.build, p.dicts));
    const uint32_t dyn = dynamic_lds(p);  // (0 for the fixed-geometry builds: their LDS is a static array of the kernel's)
    if (dyn) HIP_OK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    if (!p.persistent) return TAMP_OK;
    static std::mutex occ_mu;
    static std::map<std::pair<const void*, uint64_t>, int> occ;  // (0: not asked yet)
    std::lock_guard<std::mutex> lock(occ_mu);
    int& cached = occ[std::make_pair(kernel, (uint64_t)dyn << 16 | p.threads)];
    if (cached == 0) HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&cached, kernel, (int)p.threads, dyn));
    *per_cu = cached = std::max(cached, 1);
    return TAMP_OK;
}
int launch_on_counter(DeviceCtx* ctx, const CompressPlan& p, uint32_t grid, CompressArgs& a, hipStream_t st) {
    a.work_counter = ctx->work_counters + ctx->next_counter.fetch_add(1) % DeviceCtx::kCounters;
    HIP_OK(hipMemsetAsync(a.work_counter, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(compress_kernel_of(p.build, p.dicts), dim3(grid), dim3(p.threads), dynamic_lds(p), st, a);
    return TAMP_OK;
}

// Block mode (the BLOCKM builds of the compress kernel): ONE long stream of the v1 format, literal 8, default parse, fresh window.
// -> TAMP_OK when the stream was taken this way, 1 when the call does not qualify (the caller goes on with the batch kernel).
// `rec`: the stream's scratch record, locked by the caller.  `a0`: the batch's argument block (its tables are those of `t`).
int launch_compress_blocks(DeviceCtx* ctx, StreamScratch& rec, CompressArgs a0, const BatchTables& t, CompressCall call, hipStream_t st) {
    const TampAmdConf* conf = call.conf;
    const size_t n_streams = t.n;
    uint32_t min_len = 256u << 10;
    if (const char* e = getenv("TAMP_AMD_BLOCK_MIN")) min_len = (uint32_t)atoi(e) > 0 ? (uint32_t)atoi(e) : 0xFFFFFFFFu;  // (tuning / tests; 0 = off)
    if (conf->extended || conf->lazy_matching || conf->literal != 8 || conf->window > 14 || call.has_state || call.seg_flags ||
        call.max_in_len < min_len || n_streams == 0 || n_streams > 64)
        return 1;
    // the streams' table rows: lengths, capacities (the launch geometry and the zero fill depend on them); a handful of LONG
    // streams is taken one after the other, each over all workgroups -- any shorter one among them and the batch kernel takes all
    uint64_t in_off[64], out_off[64], dict_off[64];
    uint32_t in_len[64], out_cap[64];
    if (t.dict_off) HIP_OK(hipMemcpyAsync(dict_off, t.dict_off, 8 * n_streams, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(in_off, t.in_off, 8 * n_streams, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(out_off, t.out_off, 8 * n_streams, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(in_len, t.in_len, 4 * n_streams, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(out_cap, t.out_cap, 4 * n_streams, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    uint32_t n_max = 0;
    for (size_t i = 0; i < n_streams; i++) {
        if (in_len[i] < min_len) return 1;
        // (a dictionary-table row the batch kernel would refuse: the batch kernel refuses it)
        if (t.dict_off && !(dict_off_aligned(dict_off[i]) && dict_off_in_bounds(dict_off[i], 1u << conf->window, t.dict_len))) return 1;
        n_max = std::max(n_max, in_len[i]);
    }
    call.block_mode = true;
    const CompressPlan p = plan_compress(call);
    a0.blk = p.blk, a0.claim = p.claim, a0.cut_run = 0;
    if (p.lds.total > ctx->lds_per_block) return 1;
    int per_cu = 0;
    if (const int rc = prepare_compress_kernel(p, &per_cu)) return rc;
    // scratch for the longest of them
    const uint32_t nb_max = (n_max + a0.blk - 1) / a0.blk, nc_max = (nb_max + kScanChunk - 1) / kScanChunk;
    const size_t table_bytes = ((size_t)nb_max * 16 * 4 + 255) & ~(size_t)255, info_bytes = ((size_t)nb_max * 8 + 255) & ~(size_t)255;
    const size_t chunk_bytes = ((size_t)nc_max * 16 * 8 + 255) & ~(size_t)255;
    // (the match results of pass 1, 3 bytes per input byte, when that stays under 1.5 GiB: pass 3 then does not match again)
    const size_t len_bytes = ((size_t)n_max + 1024 + 255) & ~(size_t)255;
    const bool keep_tables = (size_t)n_max * 3 <= ((size_t)3 << 29) && !getenv("TAMP_AMD_BLOCK_REMATCH");
    HIP_OK(rec.blk.need(table_bytes + info_bytes + chunk_bytes + 256 + (keep_tables ? 3 * len_bytes : 0)));
    uint8_t* const base = static_cast<uint8_t*>(rec.blk.p);
    uint32_t* const chunk_table = reinterpret_cast<uint32_t*>(base + table_bytes + info_bytes);
    uint8_t* const tables = base + table_bytes + info_bytes + chunk_bytes;
    timing_begin(st);
    for (size_t i = 0; i < n_streams; i++) {
        CompressArgs a = a0;
        set_tables(a, t.rows(i, 1));  // (the kernel reads row 0; n_streams: the blocks, below)
        const uint32_t n = in_len[i];
        const uint32_t n_blocks = (n + a.blk - 1) / a.blk;
        const uint32_t n_chunks = (n_blocks + kScanChunk - 1) / kScanChunk;
        a.blk_table = reinterpret_cast<uint32_t*>(base);
        a.blk_info = reinterpret_cast<unsigned long long*>(base + table_bytes);
        a.blk_len = keep_tables ? tables : nullptr;
        a.blk_idx = keep_tables ? reinterpret_cast<uint16_t*>(tables + len_bytes) : nullptr;
        a.n_blocks = n_blocks, a.n_streams = n_blocks;
        const uint32_t g = (uint32_t)std::min<size_t>((size_t)per_cu * (size_t)ctx->cu_count, n_blocks);
        // every byte the emitters may OR into: header + 9 bits per input byte at most (all literals), capped by the caller's room
        const uint64_t bound = (uint64_t)a.nlead + ((uint64_t)n * 9 + 7) / 8 + 8;
        HIP_OK(hipMemsetAsync(a.out + out_off[i], 0, (size_t)std::min<uint64_t>(bound, out_cap[i]), st));
        for (uint32_t pass = 1; pass <= 3; pass++) {
            if (pass == 2) {
                hipLaunchKernelGGL(tamp_block_scan_chunks, dim3(n_chunks), dim3(256), 0, st, a.blk_table, chunk_table, n_blocks);
                hipLaunchKernelGGL(tamp_block_scan_kernel, dim3(n_chunks), dim3(256), 0, st, a.blk_table, chunk_table, a.blk_info, n_blocks, 8u * a.nlead);
                continue;
            }
            a.block_pass = pass;
            if (const int rc = launch_on_counter(ctx, p, g, a, st)) return rc;
        }
    }
    timing_end(st);
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// `t`: device memory.  `seg` / `d_state`: a piece of one stream (segment_core), its state row.
// `rec`: the stream's scratch record, locked by the caller (launch_compress; launch_compress_resets and launch_compress_batch_resets, which hold it over their slices; launch_pieces, over its classes).
int launch_compress_locked(DeviceCtx* ctx, StreamScratch& rec, const TampAmdConf* conf, const BatchTables& t, uint32_t max_in_len,
                           hipStream_t st, const SegmentSpec* seg, uint8_t* d_state) {
    const size_t n_streams = t.n;
    if (n_streams == 0) return TAMP_OK;
    CompressCall call = compress_call(conf, max_in_len, reinterpret_cast<uintptr_t>(t.dict));
    if (seg) call.nlead = seg->nlead, call.lead = seg->lead, call.seg_flags = seg->flags, call.has_state = d_state != nullptr;
    call.dict_table = t.dict_off != nullptr;
    CompressArgs a = fill_compress_args(ctx, call, t, d_state);
    if (n_streams <= 64 && !seg) {  // a handful of LONG v1 streams: each one's blocks over all workgroups (the BLOCKM builds)
        const int rc = launch_compress_blocks(ctx, rec, a, t, call, st);
        if (rc != 1) return rc;
    }
    const CompressPlan p = plan_compress(call);  // (build, block, LDS layout, workgroup, grid: tamp_compress_plan.hpp)
    a.blk = p.blk, a.claim = p.claim;
    if (p.lds.total > ctx->lds_per_block) {
        snprintf(t_last_error, sizeof t_last_error, "LDS %u B > %zu B per block", p.lds.total, ctx->lds_per_block);
        return TAMP_AMD_BAD_ARGUMENT;
    }
    if (!p.persistent && p.threads != 64) {  // (short messages only: long streams are run-aware)
        snprintf(t_last_error, sizeof t_last_error, "no lean build for %u-thread workgroups", p.threads);
        return TAMP_AMD_BAD_ARGUMENT;
    }
    int per_cu = 0;
    if (const int rc = prepare_compress_kernel(p, &per_cu)) return rc;
    if (p.persistent) {
        if (const char* e = getenv("TAMP_AMD_GRID_PER_CU")) {  // (tuning)
            if (atoi(e) > 0) per_cu = atoi(e);
            else fprintf(stderr, "tamp_amd: %d workgroups of %u threads, %u B LDS per CU\n", per_cu, p.threads, p.lds.total);
        }
        const size_t claims = (n_streams + a.claim - 1) / a.claim;
        size_t g = std::min<size_t>((size_t)per_cu * (size_t)ctx->cu_count, claims);
        // TAMP_AMD_STATIC_GRID=1 (tuning): one workgroup per claim instead -- each takes its claim when it starts and finds
        // the counter exhausted afterwards
        if (getenv("TAMP_AMD_STATIC_GRID")) g = claims;
        // (every workgroup fetches one claim beyond the last: the counter ends at (claims + g) * claim)
        if ((claims + g) * a.claim > 0xFFFFFFFFull || g > 0x7FFFFFFFull) {
            snprintf(t_last_error, sizeof t_last_error, "%zu streams: beyond the 32-bit work counter", n_streams);
            return TAMP_AMD_BAD_ARGUMENT;
        }
        // (every argument check lies in front of the event pair: a refused call leaves no half-recorded timing)
        timing_begin(st);
        // expensive streams first, for batches of more than one and at most ~18 rounds of the grid (beyond, the tail is short
        // next to the batch; TAMP_AMD_LPT=0 / =1 force it off / on)
        bool lpt = p.threads == 256 && !seg && n_streams > g && n_streams <= 32768;
        if (const char* e = getenv("TAMP_AMD_LPT")) lpt = atoi(e) != 0 && p.threads == 256 && !seg && n_streams > 1 && n_streams <= (1u << 20);
        uint8_t* lpt_mem = nullptr;
        uint32_t* lpt_order = nullptr;
        uint32_t* lpt_out_len = nullptr;
        int8_t* lpt_status = nullptr;
        if (lpt) {
            const size_t n = n_streams;
            const size_t bytes = n * (4 + 4 + 8 + 4 + 8 + 4 + 4 + 1) + 256 + (a.dict_off ? n * 8 + 8 : 0);
            if (rec.lpt.need(bytes) == hipSuccess) lpt_mem = static_cast<uint8_t*>(rec.lpt.p);
            if (!lpt_mem) {
                (void)hipGetLastError();
                lpt = false;
            } else {
                uint64_t* g_in_off = reinterpret_cast<uint64_t*>(lpt_mem);
                uint64_t* g_out_off = g_in_off + n;
                uint32_t* score = reinterpret_cast<uint32_t*>(g_out_off + n);
                lpt_order = score + n;
                uint32_t* g_in_len = lpt_order + n;
                uint32_t* g_out_cap = g_in_len + n;
                lpt_out_len = g_out_cap + n;
                lpt_status = reinterpret_cast<int8_t*>(lpt_out_len + n);
                hipLaunchKernelGGL(tamp_stream_score_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st, a.in, a.in_off, a.in_len, (uint32_t)n, score);
                hipLaunchKernelGGL(tamp_stream_order_kernel, dim3(1), dim3(1024), 0, st, score, (uint32_t)n, lpt_order);
                hipLaunchKernelGGL(tamp_gather_rows_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, lpt_order, (uint32_t)n, a.in_off,
                                   a.in_len, a.out_off, a.out_cap, g_in_off, g_in_len, g_out_off, g_out_cap);
                a.in_off = g_in_off, a.in_len = g_in_len, a.out_off = g_out_off, a.out_cap = g_out_cap;
                a.out_len = lpt_out_len, a.status = lpt_status;
                if (a.dict_off) {  // (behind the status bytes, at the next multiple of 8)
                    uint64_t* const g_dict_off = reinterpret_cast<uint64_t*>(lpt_mem + ((n * (4 + 4 + 8 + 4 + 8 + 4 + 4 + 1) + 7) & ~(size_t)7));
                    hipLaunchKernelGGL(tamp_gather_u64_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, lpt_order, (uint32_t)n, a.dict_off, g_dict_off);
                    a.dict_off = g_dict_off;
                }
            }
        }
        if (const int rc = launch_on_counter(ctx, p, (uint32_t)g, a, st)) return rc;
        if (lpt) {
            hipLaunchKernelGGL(tamp_scatter_results_kernel, dim3((uint32_t)((n_streams + 255) / 256)), dim3(256), 0, st, lpt_order,
                               (uint32_t)n_streams, lpt_out_len, lpt_status, t.out_len, t.status);
        }
    } else {
        timing_begin(st);
        const size_t launch_step = 1u << 20;
        for (size_t first = 0; first < n_streams; first += launch_step) {  // one stream per workgroup
            a.first_stream = (uint32_t)first;
            const uint32_t g = (uint32_t)std::min<size_t>(launch_step, n_streams - first);
            hipLaunchKernelGGL(compress_kernel_of(p.build, p.dicts), dim3(g), dim3(p.threads), dynamic_lds(p), st, a);
        }
    }
    timing_end(st);
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}
int launch_compress(DeviceCtx* ctx, const TampAmdConf* conf, const BatchTables& t, uint32_t max_in_len, hipStream_t st,
                    const SegmentSpec* seg = nullptr, uint8_t* d_state = nullptr) {
    if (t.n == 0) return TAMP_OK;
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    return launch_compress_locked(ctx, rec, conf, t, max_in_len, st, seg, d_state);
}

// Largest window (bits) any stream header of the batch asks for, among those the caller's limit admits.  LDS rows of the
// decoders are sized from it instead of from the limit: a caller that passes the API default (15) for 1 KiB-window
// streams would otherwise run at a fraction of the occupancy.
__global__ void tamp_header_scan_kernel(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                        const uint32_t* out_cap, uint32_t n, uint32_t limit, uint32_t* result) {
    uint32_t m = 0, longest = 0, wsum = 0;  // wsum: window bytes / 256, summed over the streams within the limit
    uint32_t maxcap = 0;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
        const uint32_t len = in_len[s];
        maxcap = out_cap[s] > maxcap ? out_cap[s] : maxcap;
        if (len == 0) continue;
        longest = len > longest ? len : longest;
        const uint32_t w = 8u + (in[in_off[s]] >> 5);  // header byte, decompressor.c:276-297
        if (w <= limit) {
            m = w > m ? w : m;
            wsum += 1u << (w - 8);
        }
    }
    m = wave_max_u32(m);
    longest = wave_max_u32(longest);
    maxcap = wave_max_u32(maxcap);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wsum += (uint32_t)__shfl_xor((int)wsum, off);
    // one set of atomics per WORKGROUP: with one per wavefront, 16,384 wavefronts of a million-stream batch queued 65,536
    // atomics on four addresses -- 0.39 ms for a pre-pass that reads 13 MB (round 4: block reduction through LDS)
    __shared__ uint32_t red[4][4];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & (kWave - 1)) == 0) red[wave][0] = m, red[wave][1] = longest, red[wave][2] = wsum, red[wave][3] = maxcap;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t nw = blockDim.x >> 6;
        for (uint32_t w = 1; w < nw; w++) {
            m = red[w][0] > m ? red[w][0] : m;
            longest = red[w][1] > longest ? red[w][1] : longest;
            wsum += red[w][2];
            maxcap = red[w][3] > maxcap ? red[w][3] : maxcap;
        }
        if (m) atomicMax(result, m);
        atomicMax(result + 1, longest);
        atomicAdd(result + 2, wsum);
        atomicMax(result + 3, maxcap);
    }
}

// The decoders' argument block from the batch's tables: no scratch, no flagged list, the plan's fields unset.  What a caller passes
// differently (no dictionary for the object calls, a window limit) it says at the call.
DecompressArgs decompress_args(const DeviceCtx* ctx, const BatchTables& t) {
    DecompressArgs a;
    a.in = t.in, a.in_off = t.in_off, a.in_len = t.in_len;
    a.out = t.out, a.out_off = t.out_off, a.out_cap = t.out_cap, a.out_len = t.out_len, a.status = t.status;
    a.in_consumed = t.in_consumed;
    a.dict = t.dict, a.dict_len = t.dict_len, a.dict_off = t.dict_off;
    a.seed_dicts = ctx->seed_dicts;
    a.scratch = nullptr;
    a.only_flagged = nullptr;
    a.flagged_count = nullptr;
    a.n_streams = (uint32_t)t.n;
    a.lds_row = 0;
    a.max_wbits = 0;
    return a;
}

// The front of the long-stream path (tamp_decompress_long_kernel.hpp), shared by the decoder and the size query: header read and
// gates, the tables of the settle rounds and the count pass (with_records: the decoder's records and group tables behind them), the
// tamp_long_sync_kernel rounds, and tamp_long_parse_kernel with write = 0 -- tokens and output bytes per chunk.
struct LongFront {
    uint32_t n, cap;       // compressed bytes; room (the size query: the stream's limit, 0xFFFFFFFF without one)
    uint64_t out_off;      // (decoder only)
    const uint8_t* in;
    StreamHeader hd;
    uint32_t hs, N, chunk_bits, lg;  // header bytes, chunks, bits per chunk, workgroups of the chunk kernels
    const uint8_t* dict0;  // the fresh decoder's window: the custom dictionary, or the seeded table for the stream's literal size
    size_t b_tab;          // bytes of the per-chunk tables at the start of rec.long_tab (records: behind them)
    uint32_t *d_tokbase, *d_rot, *d_specbase, *d_chunk_lag, *d_chunk_o0, *d_chunk_lag0, *d_lagbase;
    LongArgs la;           // as the count pass ran: g = the settled starts, write = 0
    std::vector<uint32_t> ntok, outb;  // per chunk
    bool dbg;              // TAMP_AMD_LONGDEC_DEBUG
};
// A stream behind the length gate that goes to the exact decoders after all: -> 1, and under TAMP_AMD_LONGDEC_DEBUG one line that says why.
static int long_declined(bool dbg, const char* who, const char* why, const char* tag = "long") {
    if (dbg) fprintf(stderr, "[tamp_amd %s %s] declined: %s\n", tag, who, why);
    return 1;
}
// -> 1 when the stream is not one for this path (or anything is off: the exact decoders take it), TAMP_OK with `f` filled in and
// timing begun, an error code otherwise.  `who` names the caller in the debug lines.  `t`: the stream's single row; out_off and
// out_cap may be null.  `has_dict`: a stream with the custom bit has a dictionary (the size query: its length alone, t.dict is null).
int long_decode_front(DeviceCtx* ctx, StreamScratch& rec, const DecodeLong& gate, const BatchTables& t, bool has_dict, uint8_t max_wbits,
                      bool with_records, const char* who, hipStream_t st, LongFront& f, bool resets = false) {
    // `resets` (launch_decompress_resets): the front alone, for a stream WITH the dictionary_reset bit -- the token grammar does not
    // depend on resets -- under its own tag and debug variable; every other caller keeps its gates and its lines
    const char* const tag = resets ? "resets" : "long";
    uint64_t in_off = 0, out_off = 0, dict_off = 0;  // (dict_off: the stream's row of a dictionary table, 0 without one)
    uint32_t n = 0, cap = 0xFFFFFFFFu;
    HIP_OK(hipMemcpyAsync(&n, t.in_len, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    // (the chunk kernels count bits in 32-bit registers: (i + 1) * kLongChunkBits wraps for the last chunk of the top 512 bytes of
    // the accepted range -- those streams stay with the exact decoder)
    if (n < gate.min_len || n > kMaxDecodeIn - 512) return 1;
    const bool dbg = f.dbg = getenv(resets ? "TAMP_AMD_RESETS_DEBUG" : "TAMP_AMD_LONGDEC_DEBUG") != nullptr;
    HIP_OK(hipMemcpyAsync(&in_off, t.in_off, 8, hipMemcpyDeviceToHost, st));
    if (t.out_off) HIP_OK(hipMemcpyAsync(&out_off, t.out_off, 8, hipMemcpyDeviceToHost, st));
    if (t.out_cap) HIP_OK(hipMemcpyAsync(&cap, t.out_cap, 4, hipMemcpyDeviceToHost, st));
    if (t.dict_off) HIP_OK(hipMemcpyAsync(&dict_off, t.dict_off, 8, hipMemcpyDeviceToHost, st));
    uint8_t hdr[2] = {0, 0};
    HIP_OK(hipMemcpyAsync(hdr, t.in + in_off, 2, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const uint8_t* const in = t.in + in_off;
    const StreamHeader hd = decode_header(hdr[0]);
    const uint32_t hs = 1 + (hdr[0] & 1), wbits = hd.wbits, lbits = hd.lbits;
    const bool extended = hd.extended;
    if ((resets ? !hd.dreset || hd.custom : hd.dreset) || (hs == 2 && hdr[1]) || wbits > (uint32_t)(max_wbits & 0x7F) || (max_wbits & 0x7F) > 15)
        return long_declined(dbg, who, "header", tag);
    if (extended && !gate.extended) return long_declined(dbg, who, "extended off", tag);  // (tests: the exact decoder)
    const uint32_t W = 1u << wbits;
    // (its own row's length; a misaligned row is the exact decoders' to report as well)
    if (hd.custom && (!has_dict || !dict_off_aligned(dict_off) || !dict_off_in_bounds(dict_off, W, t.dict_len))) return long_declined(dbg, who, "dictionary", tag);
    f.n = n, f.cap = cap, f.out_off = out_off, f.in = in, f.hd = hd, f.hs = hs;
    f.dict0 = hd.custom ? t.dict + dict_off : ctx->seed_dicts + ((size_t)hd.table << 15);

    const uint64_t total_bits = 8ull * n;
    const uint32_t chunk_bits = extended ? kLongChunkBitsExt : kLongChunkBits;
    const uint32_t N = (uint32_t)((total_bits + chunk_bits - 1) / chunk_bits);
    // scratch: g, g_next (N + 1 each), flags (4), ntok, outb, tokbase, rot (N each), the extended format's seven per-chunk tables,
    // then what the groups need
    const size_t b_tab = ((size_t)(14 * (size_t)N + 16) * 4 + 255) & ~(size_t)255;
    {
        // worst case records: the shortest token is a literal, 1 + literal bits
        const size_t max_tok = (size_t)(total_bits / (1 + lbits)) + 4096;
        const size_t b_groups = ((size_t)(max_tok / 256 + N + 64) * (16 + sizeof(LongGroup) + 4) + 255) & ~(size_t)255;
        const size_t bytes = with_records ? b_tab + max_tok * 4 + b_groups + 4 * (size_t)(1u << 15) + 4096 : b_tab;
        if (rec.long_tab.need(bytes) != hipSuccess) return long_declined(dbg, who, "scratch", tag);
    }
    uint8_t* const tab = static_cast<uint8_t*>(rec.long_tab.p);
    uint32_t* const g0 = reinterpret_cast<uint32_t*>(tab);
    uint32_t* const g1 = g0 + (N + 1);
    uint32_t* const flags = g1 + (N + 1);
    uint32_t* const d_ntok = flags + 8;
    uint32_t* const d_outb = d_ntok + N;
    uint32_t* const d_tokbase = d_outb + N;
    uint32_t* const d_rot = d_tokbase + N;
    uint32_t* const d_nspec = d_rot + N;          // (extended format from here)
    uint32_t* const d_specbase = d_nspec + N;
    uint32_t* const d_chunk_lag = d_specbase + N;  // 2 N
    uint32_t* const d_chunk_o0 = d_chunk_lag + 2 * (size_t)N;
    uint32_t* const d_chunk_lag0 = d_chunk_o0 + N;
    uint32_t* const d_lagbase = d_chunk_lag0 + N;
    f.N = N, f.chunk_bits = chunk_bits, f.b_tab = b_tab;
    f.d_tokbase = d_tokbase, f.d_rot = d_rot, f.d_specbase = d_specbase, f.d_chunk_lag = d_chunk_lag, f.d_chunk_o0 = d_chunk_o0;
    f.d_chunk_lag0 = d_chunk_lag0, f.d_lagbase = d_lagbase;

    timing_begin(st);
    LongArgs& la = f.la;
    memset(&la, 0, sizeof la);
    la.in = in, la.n = n, la.first_bit = 8 * hs, la.n_chunks = N, la.wbits = wbits, la.lbits = lbits;
    la.chunk_bits = chunk_bits, la.extended = extended ? 1u : 0u, la.nspec = d_nspec;
    la.flags = flags, la.ntok = d_ntok, la.outb = d_outb, la.tokbase = d_tokbase, la.rot = d_rot, la.write = 0;
    la.recs = with_records ? reinterpret_cast<uint32_t*>(tab + b_tab) : nullptr;
    // start guesses: the chunk boundaries themselves (chunk 0: behind the header)
    {
        std::vector<uint32_t> init(N + 1);
        for (uint32_t i = 0; i <= N; i++) init[i] = i * chunk_bits;
        init[0] = 8 * hs;
        HIP_OK(hipMemcpyAsync(g0, init.data(), (size_t)(N + 1) * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    const uint32_t lg = (N + 63) / 64;
    f.lg = lg;
    uint32_t* cur = g0;
    uint32_t* nxt = g1;
    bool settled = false;
    int rounds = 0;
    for (int round = 0; round < 512 && !settled; round++, rounds++) {
        HIP_OK(hipMemsetAsync(flags, 0, 8, st));
        la.g = cur, la.g_next = nxt;
        hipLaunchKernelGGL(tamp_long_sync_kernel, dim3(lg), dim3(64), 0, st, la);
        uint32_t changed = 1;
        HIP_OK(hipMemcpyAsync(&changed, flags, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        std::swap(cur, nxt);
        settled = changed == 0;
    }
    if (dbg) fprintf(stderr, "[tamp_amd %s %s] %u bytes, %u chunks, %d sync rounds, settled %d\n", tag, who, n, N, rounds, (int)settled);
    if (!settled) { timing_end(st); return long_declined(dbg, who, "not settled", tag); }
    la.g = cur, la.g_next = nullptr, la.write = 0;
    HIP_OK(hipMemsetAsync(flags, 0, 8, st));
    hipLaunchKernelGGL(tamp_long_parse_kernel, dim3(lg), dim3(64), 0, st, la);
    f.ntok.resize(N), f.outb.resize(N);
    uint32_t fl[2] = {0, 0};
    HIP_OK(hipMemcpyAsync(f.ntok.data(), d_ntok, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(f.outb.data(), d_outb, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(fl, flags, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (fl[1]) { timing_end(st); return long_declined(dbg, who, "offset out of window", tag); }  // an out-of-bounds offset: the exact decoder reports where
    return TAMP_OK;
}

// ONE long v1 stream (tamp_decompress_long_kernel.hpp): start positions settled by rounds of a lane per 512 compressed bytes,
// records per chunk, then the split decoder's RESOLVE over groups of at most kSplitMaxOut output bytes, in order, each with the
// W bytes in front of it as its dictionary.  -> 1 when the call is not one (or anything is off: the exact decoders take it),
// TAMP_OK when the stream has been decoded, an error code otherwise.  Nothing is written before the fall-back decision.
// `t`: the stream's single row.
int launch_decompress_long(DeviceCtx* ctx, StreamScratch& rec, const DecodeLong& gate, const BatchTables& t, uint8_t max_wbits, hipStream_t st) {
    LongFront f;
    if (const int rc = long_decode_front(ctx, rec, gate, t, t.dict != nullptr, max_wbits, true, "decode", st, f); rc != TAMP_OK) return rc;
    const uint32_t n = f.n, cap = f.cap, N = f.N, wbits = f.hd.wbits, W = 1u << wbits, lg = f.lg;
    const uint64_t out_off = f.out_off;
    const bool extended = f.hd.extended, dbg_long = f.dbg;
    uint8_t* const out = t.out + out_off;
    const uint8_t* const dict0 = f.dict0;
    LongArgs& la = f.la;
    uint32_t* const recs = la.recs;
    uint32_t *const d_tokbase = f.d_tokbase, *const d_rot = f.d_rot, *const d_nspec = la.nspec, *const d_specbase = f.d_specbase;
    uint32_t *const d_chunk_lag = f.d_chunk_lag, *const d_chunk_o0 = f.d_chunk_o0, *const d_chunk_lag0 = f.d_chunk_lag0, *const d_lagbase = f.d_lagbase;
    const std::vector<uint32_t>&ntok = f.ntok, &outb = f.outb;
    // Extended format: the tokens that can write fewer bytes to the window than they produce are listed (a second parse), one
    // workgroup walks the list for window_pos at each of them, and what comes back per chunk is the lag behind it and the number
    // of lagging tokens in it (tamp_long_wp_kernel).
    std::vector<uint32_t> chunk_lag;  // per chunk: cumulative lag behind it, lagging tokens in it
    uint32_t* d_lag = nullptr;        // the lag lists
    uint64_t dbg_entries = 0;         // (debug line: list entries, window_pos blocks, most lagging tokens in one chunk)
    size_t dbg_wpblocks = 0;
    uint32_t dbg_maxlag = 0;
    if (extended) {
        std::vector<uint32_t> nspec(N), specbase(N);
        HIP_OK(hipMemcpyAsync(nspec.data(), d_nspec, (size_t)N * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        uint64_t n_entries = 0;
        for (uint32_t i = 0; i < N; i++) specbase[i] = (uint32_t)n_entries, n_entries += (uint64_t)nspec[i] + 1;
        if (n_entries > 0xFFFFFFF0ull) { timing_end(st); return long_declined(dbg_long, "decode", "list too long"); }
        const size_t n_wpblocks = (size_t)((n_entries + kLongWpBlock - 1) / kLongWpBlock);
        // gap, token, bytes written per list entry; behind them the lag lists (at most one entry per listed token) and the
        // window_pos tables of the list's blocks (tamp_long_wp_kernel: 8 bytes per block and start value, 20 per block)
        if (rec.long_lags.need((size_t)n_entries * (3 + 2) * 4 + n_wpblocks * ((size_t)W * 8 + 20) + 256) != hipSuccess) { (void)hipGetLastError(); timing_end(st); return long_declined(dbg_long, "decode", "scratch"); }
        uint32_t* const d_spec = static_cast<uint32_t*>(rec.long_lags.p);
        la.specbase = d_specbase, la.spec_gap = d_spec, la.spec_kl = d_spec + n_entries, la.spec_written = d_spec + 2 * n_entries;
        d_lag = d_spec + 3 * n_entries;
        la.chunk_lag = d_chunk_lag, la.lag = d_lag;
        HIP_OK(hipMemcpyAsync(d_specbase, specbase.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
        la.write = 2;
        hipLaunchKernelGGL(tamp_long_parse_kernel, dim3(lg), dim3(64), 0, st, la);
        {
            LongWpArgs wa;
            wa.a = la, wa.n_entries = (uint32_t)n_entries, wa.n_blocks = (uint32_t)n_wpblocks;
            wa.f_cum = d_spec + 5 * n_entries;
            wa.markers = wa.f_cum + n_wpblocks * (size_t)W;
            wa.state = wa.markers + n_wpblocks;
            wa.f_wp = reinterpret_cast<uint16_t*>(wa.state + 4 * n_wpblocks);
            wa.f_nl = wa.f_wp + n_wpblocks * (size_t)W;
            hipLaunchKernelGGL(tamp_long_wp_kernel<0>, dim3((uint32_t)n_wpblocks), dim3(1024), 0, st, wa);
            hipLaunchKernelGGL(tamp_long_wp_kernel<1>, dim3(1), dim3(64), 0, st, wa);
            hipLaunchKernelGGL(tamp_long_wp_kernel<2>, dim3((uint32_t)n_wpblocks), dim3(256), 0, st, wa);
        }
        chunk_lag.resize(2 * (size_t)N);
        HIP_OK(hipMemcpyAsync(chunk_lag.data(), d_chunk_lag, 2 * (size_t)N * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));  // (also: specbase goes out of scope)
        dbg_entries = n_entries, dbg_wpblocks = n_wpblocks;
        for (uint32_t i = 0; i < N; i++) dbg_maxlag = std::max(dbg_maxlag, chunk_lag[2 * (size_t)i + 1]);
        for (uint32_t i = 0; i < N; i++)
            if (chunk_lag[2 * (size_t)i + 1] > kLongLagCap) { timing_end(st); return long_declined(dbg_long, "decode", "lags per chunk"); }  // (more lagging tokens in one chunk than a group lists)
    }
    // groups of whole chunks: at most kSplitMaxOut output bytes, 2^20 - 1 records and kLongLagCap lagging tokens each
    const bool chain = extended || gate.chain;
    const uint32_t group_out = chain ? kLongGroupOut : kSplitMaxOut;
    struct Group { uint64_t v0; uint32_t tok0, ntok, nout, lag0, nlag; uint64_t lagv0; };  // lagv0: lag of the stream in front of the group
    std::vector<Group> groups;
    std::vector<uint32_t> tokbase(N), rot(N), chunk_o0(N), chunk_lag0(N), lagbase(N);
    uint64_t v = 0, tk = 0, lags = 0, cum = 0;  // output bytes, records, lagging tokens, lag so far
    {
        Group gcur{0, 0, 0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < N; i++) {
            const uint32_t nl = extended ? chunk_lag[2 * (size_t)i + 1] : 0u;
            if (gcur.nout + outb[i] > group_out || gcur.ntok + ntok[i] > 0xFFFFFu || gcur.nlag + nl > kLongLagCap) {
                groups.push_back(gcur);
                gcur = Group{v, (uint32_t)tk, 0, 0, (uint32_t)lags, 0, cum};
            }
            // a group's window cursor starts at (bytes WRITTEN in front of it) mod W: the output position less the lag so far
            tokbase[i] = (uint32_t)tk, rot[i] = (uint32_t)((gcur.v0 - gcur.lagv0) & (W - 1));
            chunk_o0[i] = (uint32_t)(v - gcur.v0), chunk_lag0[i] = (uint32_t)(cum - gcur.lagv0), lagbase[i] = (uint32_t)lags;
            gcur.ntok += ntok[i], gcur.nout += outb[i], gcur.nlag += nl;
            tk += ntok[i], v += outb[i], lags += nl;
            if (extended) cum = chunk_lag[2 * (size_t)i];
        }
        groups.push_back(gcur);
    }
    // (room that is used up -- even exactly -- is TAMP_OUTPUT_FULL in the reference when padding bits are left, decompressor.c:431-436,
    // and a partial last token when it is not enough: the exact decoder's)
    if (v >= cap) { timing_end(st); return long_declined(dbg_long, "decode", "output room"); }
    if (tk > 0xFFFFFFFFull - 4096) { timing_end(st); return long_declined(dbg_long, "decode", "records"); }
    HIP_OK(hipMemcpyAsync(d_tokbase, tokbase.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_rot, rot.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
    if (extended) {
        HIP_OK(hipMemcpyAsync(d_chunk_o0, chunk_o0.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_chunk_lag0, chunk_lag0.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_lagbase, lagbase.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
        la.chunk_o0 = d_chunk_o0, la.chunk_lag0 = d_chunk_lag0, la.lagbase = d_lagbase;
    }
    la.write = 1;
    hipLaunchKernelGGL(tamp_long_parse_kernel, dim3(lg), dim3(64), 0, st, la);
    // per group: meta word, output offset and size, in tables behind the records
    const size_t G = groups.size();
    uint8_t* const gtab = reinterpret_cast<uint8_t*>(recs) + (((size_t)tk + 4096) * 4 + 255 & ~(size_t)255);
    uint64_t* const d_goff = reinterpret_cast<uint64_t*>(gtab);
    uint32_t* const d_glen = reinterpret_cast<uint32_t*>(d_goff + G);
    uint32_t* const d_gmeta = d_glen + G;
    uint8_t* const d_win = reinterpret_cast<uint8_t*>(d_gmeta + G + 16);  // windows of the groups that start inside the first W bytes
    {
        std::vector<uint64_t> goff(G);
        std::vector<uint32_t> glen(G), gmeta(G);
        for (size_t k = 0; k < G; k++) {
            goff[k] = out_off + groups[k].v0, glen[k] = groups[k].nout;
            gmeta[k] = (groups[k].ntok & 0xFFFFFu) | ((wbits - 8) << 20) | (3u << 23);
        }
        HIP_OK(hipMemcpyAsync(d_goff, goff.data(), G * 8, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_glen, glen.data(), G * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_gmeta, gmeta.data(), G * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));  // (the vectors go out of scope)
    }
    if (dbg_long) {
        size_t early = 0;  // groups that start inside the first W bytes (TAMP_AMD_LONGDEC_CHAIN=0: they get a window of their own below)
        for (const Group& gr : groups) early += gr.nout != 0 && gr.v0 < W;
        fprintf(stderr, "[tamp_amd long decode] %zu groups, %llu tokens, %llu bytes out, %llu entries, %zu wp blocks, max lags %u, %zu early groups, %zu scan blocks\n",
                G, (unsigned long long)tk, (unsigned long long)v, (unsigned long long)dbg_entries, dbg_wpblocks, dbg_maxlag, early,
                chain ? (G + kLongScanBlock - 1) / kLongScanBlock : (size_t)0);
    }
    if (chain) {
        // every group by a workgroup of its own, no workgroup waiting for another (tamp_decompress_long_kernel.hpp, step 3):
        // tail maps, their composition by one workgroup, finish.  The group table sits behind the tables above, the maps
        // (G x W x 2 bytes) in a buffer of their own.
        uint8_t* const ctab = d_win + 4 * (size_t)(1u << 15);
        LongGroup* const d_groups = reinterpret_cast<LongGroup*>(ctab);
        const size_t n_blocks = (G + kLongScanBlock - 1) / kLongScanBlock;
        // (behind the groups' maps: the blocks' maps and the window in front of every block)
        // (... and, extended format, in front of every group: with lags the window is not "the last W output bytes")
        if (rec.long_tails.need((G + n_blocks) * (size_t)W * 2 + (n_blocks + (extended ? G : 0)) * (size_t)W + 256) != hipSuccess) { (void)hipGetLastError(); timing_end(st); return long_declined(dbg_long, "decode", "scratch"); }
        uint16_t* const d_maps = static_cast<uint16_t*>(rec.long_tails.p);
        uint16_t* const d_blockmap = d_maps + G * (size_t)W;
        uint8_t* const d_blockwin = reinterpret_cast<uint8_t*>(d_blockmap + n_blocks * (size_t)W);
        uint8_t* const d_groupwin = extended ? d_blockwin + n_blocks * (size_t)W : nullptr;
        {
            std::vector<LongGroup> tabv(G);
            for (size_t k = 0; k < G; k++)
                tabv[k] = LongGroup{groups[k].v0, groups[k].tok0, groups[k].ntok, groups[k].nout, groups[k].lag0, groups[k].nlag, 0};
            HIP_OK(hipMemcpyAsync(d_groups, tabv.data(), G * sizeof(LongGroup), hipMemcpyHostToDevice, st));
            HIP_OK(hipStreamSynchronize(st));
        }
        LongResolveArgs ra;
        ra.recs = recs, ra.groups = d_groups, ra.out = out, ra.dict0 = dict0, ra.tailmap = d_maps, ra.wbits = wbits;
        ra.lag = d_lag, ra.groupwin = d_groupwin;
        ra.n_groups = (uint32_t)G;
        auto k_tails = extended ? tamp_long_resolve_kernel<1, true> : tamp_long_resolve_kernel<1, false>;
        auto k_finish = extended ? tamp_long_resolve_kernel<2, true> : tamp_long_resolve_kernel<2, false>;
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tails), hipFuncAttributeMaxDynamicSharedMemorySize, (int)long_resolve_lds()));
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_finish), hipFuncAttributeMaxDynamicSharedMemorySize, (int)long_resolve_lds()));
        LongScanArgs sc;
        sc.r = ra, sc.blockmap = d_blockmap, sc.blockwin = d_blockwin, sc.n_blocks = (uint32_t)n_blocks;
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(tamp_long_tail_scan_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * W)));
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(tamp_long_tail_scan_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * W)));
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(tamp_long_tail_scan_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * W)));
        hipLaunchKernelGGL(k_tails, dim3((uint32_t)G), dim3(256), long_resolve_lds(), st, ra);
        hipLaunchKernelGGL(tamp_long_tail_scan_kernel<0>, dim3((uint32_t)n_blocks), dim3(kLongScanThreads), 4 * W, st, sc);
        hipLaunchKernelGGL(tamp_long_tail_scan_kernel<1>, dim3(1), dim3(kLongScanThreads), 2 * W, st, sc);
        hipLaunchKernelGGL(tamp_long_tail_scan_kernel<2>, dim3((uint32_t)n_blocks), dim3(kLongScanThreads), 2 * W, st, sc);
        hipLaunchKernelGGL(k_finish, dim3((uint32_t)G), dim3(256), long_resolve_lds(), st, ra);
        hipLaunchKernelGGL(tamp_long_finish_kernel, dim3(1), dim3(1), 0, st, t.out_len, t.status, t.in_consumed, (uint32_t)v, n);
        timing_end(st);
        HIP_OK(hipGetLastError());
        return TAMP_OK;
    }
    SplitArgs sa;
    DecompressArgs& a = sa.d;
    a = decompress_args(ctx, t);  // (per group below: its window as the dictionary, its own output offset and length)
    a.in_consumed = nullptr, a.dict_len = W, a.dict_off = nullptr, a.max_wbits = (uint8_t)wbits;
    sa.lag = nullptr, sa.flagged = nullptr, sa.flagged_count = nullptr, sa.maxcap = kSplitMaxOut, sa.first = 0, sa.count = 1, sa.spw = 64;
    const uint32_t lds = split_resolve_lds(kSplitMaxOut);
    auto resolve_kernel = tamp_decode_resolve_kernel<256, 4>;
    HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(resolve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    uint32_t early = 0;
    for (size_t k = 0; k < G; k++) {
        const Group& gr = groups[k];
        if (gr.nout == 0) continue;
        if (gr.v0 < W) {
            if (early >= 4) { timing_end(st); return TAMP_ERROR; }  // (cannot happen: groups hold >= 11 KiB unless they are the last)
            uint8_t* const wbuf = d_win + (size_t)early * (1u << 15);
            early++;
            hipLaunchKernelGGL(tamp_long_window_kernel, dim3((W + 255) / 256), dim3(256), 0, st, wbuf, out, dict0, (uint32_t)gr.v0, W);
            a.dict = wbuf;
        } else {
            a.dict = out + gr.v0 - W;
        }
        a.out_off = d_goff + k, a.out_len = d_glen + k;
        sa.recs = recs + gr.tok0, sa.meta = d_gmeta + k;
        sa.tokcap = gr.ntok > 2048 ? gr.ntok : 2048;
        hipLaunchKernelGGL(resolve_kernel, dim3(1), dim3(256), lds, st, sa);
    }
    hipLaunchKernelGGL(tamp_long_finish_kernel, dim3(1), dim3(1), 0, st, t.out_len, t.status, t.in_consumed, (uint32_t)v, n);
    timing_end(st);
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// A wavefront-per-stream kernel (the wave decoder -- with a.only_flagged: over the streams the split decoder left -- and the two
// resume kernels) in the geometry of wave_geometry(), with `lds` bytes of dynamic LDS.
template <class Args>
static int launch_waves(void (*kernel)(Args), const Args& a, const WaveGeometry& g, uint32_t lds, hipStream_t st) {
    HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3(g.groups), dim3(g.waves * kWave), lds, st, a);
    return TAMP_OK;
}

// Allocates what `plan` sized and launches its decoder.
int run_decode_plan(DeviceCtx* ctx, StreamScratch& rec, DecompressArgs a, const DecodeCall& call, const DecodeScan& scan,
                    const DecodeDevice& dev, const DecodePlan& plan, hipStream_t st) {
    const size_t n_streams = call.n_streams;
    a.max_wbits = plan.max_wbits;
    switch (plan.decoder) {
        case Decoder::kSplit: {
            // The slab is kept per HIP stream between calls (tamp_amd_trim() releases it).  If the device cannot supply it the
            // slice is halved down to 4,096 streams, and below that the batch goes to the lane / wave decoders, which need
            // little or no scratch: an allocation failure here must not fail a call that another decoder can serve.
            const SplitGeometry& g = plan.split;
            size_t slice = g.slice;
            for (;;) {
                const size_t need = g.slab_bytes(slice);
                if (rec.split.bytes >= need) break;
                HIP_OK(StreamScratch::drain_if_outgrown(rec.split, need, st));
                const bool deny = getenv("TAMP_AMD_SPLIT_FAIL_ABOVE") && need > (size_t)atol(getenv("TAMP_AMD_SPLIT_FAIL_ABOVE"));  // (tests)
                if (!deny && rec.split.need(need, false) == hipSuccess) break;
                (void)hipGetLastError();  // clear the sticky out-of-memory error
                if (slice <= 4096) return run_decode_plan(ctx, rec, a, call, scan, dev, plan_decompress(call, scan, dev, false), st);
                slice = std::max<size_t>(slice / 2, 4096);
            }
            uint8_t* const base = static_cast<uint8_t*>(rec.split.p);
            SplitArgs sa;
            sa.maxcap = g.maxcap, sa.tokcap = g.tokcap;
            sa.recs = reinterpret_cast<uint32_t*>(base);
            sa.meta = reinterpret_cast<uint32_t*>(base + g.b_recs(slice));
            sa.lag = reinterpret_cast<uint32_t*>(base + g.b_recs(slice) + g.b_meta(slice));
            sa.flagged = base + g.b_recs(slice) + g.b_meta(slice) + g.b_lag(slice);
            sa.flagged_count = reinterpret_cast<uint32_t*>(sa.flagged + ((n_streams + 3) & ~(size_t)3));  // (inside the 64 bytes of slack)
            HIP_OK(hipMemsetAsync(sa.flagged_count, 0, 4, st));
            sa.d = a;
            auto resolve_kernel = g.wave_resolve ? tamp_decode_resolve_kernel<64, 4> : tamp_decode_resolve_kernel<256, 4>;
            HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(resolve_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.resolve_lds));
            timing_begin(st);
            for (size_t first = 0; first < n_streams; first += slice) {
                sa.first = (uint32_t)first;
                sa.count = (uint32_t)std::min(slice, n_streams - first);
                sa.spw = g.spw(sa.count);
                const uint32_t pwaves = (sa.count + sa.spw - 1) / sa.spw;
                hipLaunchKernelGGL(tamp_decode_parse_kernel<true>, dim3((pwaves + 3) / 4), dim3(256), split_parse_lds(256), st, sa);
                hipLaunchKernelGGL(resolve_kernel, dim3(g.wave_resolve ? (sa.count + 3) / 4 : sa.count), dim3(256), g.resolve_lds, st, sa);
            }
            // leftovers: the wave decoder over the flagged streams only
            a.only_flagged = sa.flagged;
            a.flagged_count = sa.flagged_count;
            const int rc = launch_waves(tamp_decompress_wave_kernel, a, plan.wave, plan.wave_lds, st);
            timing_end(st);
            if (rc != TAMP_OK) return rc;
            break;
        }
        case Decoder::kWave: {
            timing_begin(st);
            const int rc = launch_waves(tamp_decompress_wave_kernel, a, plan.wave, plan.wave_lds, st);
            timing_end(st);
            if (rc != TAMP_OK) return rc;
            break;
        }
        case Decoder::kLaneLds: {
            a.lds_row = plan.lane.lds_row;
            auto lane_kernel = plan.bulk ? tamp_decompress_kernel<true, true> : tamp_decompress_kernel<true, false>;
            HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(lane_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)plan.lane.lds));
            timing_begin(st);
            hipLaunchKernelGGL(lane_kernel, dim3(plan.lane.grid), dim3(kWave), plan.lane.lds, st, a);
            timing_end(st);
            break;
        }
        case Decoder::kLaneGlobal: {
            const LaneGlobalGeometry& g = plan.global;
            a.lds_row = g.slot;
            HIP_OK(StreamScratch::drain_if_outgrown(rec.slab, g.slab_bytes, st));
            HIP_OK(rec.slab.need(g.slab_bytes, false));
            a.scratch = static_cast<uint8_t*>(rec.slab.p);
            timing_begin(st);
            if (g.gbulk)
                hipLaunchKernelGGL((tamp_decompress_kernel<false, true>), dim3(g.grid), dim3(256), g.lds, st, a);
            else
                hipLaunchKernelGGL((tamp_decompress_kernel<false, false>), dim3(g.grid), dim3(256), 0, st, a);
            timing_end(st);
            break;
        }
    }
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// A handful of long streams, one after the other, each as a single-row record with the whole device (`one`: the long decoder or
// its size query).  One event pair around all of them: kernel_ms of a call with several long streams is the sum, not the last
// stream's.  -> TAMP_OK: all taken; 1: a stream is not one for this path (too short, ...), and the caller's exact path takes the WHOLE
// call, answering for every stream again; an error code otherwise.
template <class One>  // One(const BatchTables& row) -> TAMP_OK, 1 or an error code
int each_long_stream(const BatchTables& t, hipStream_t st, const One& one) {
    timing_begin(st);
    t_timing_outer = true;
    int rc = TAMP_OK;
    for (size_t i = 0; i < t.n && rc == TAMP_OK; i++) rc = one(t.rows(i, 1));
    t_timing_outer = false;
    return rc;
}

// `t`: device memory.  A stream with the custom bit starts from its row of the dictionary table, or from t.dict without one.
// `rec`: the stream's scratch record, locked by the caller (launch_decompress; launch_decompress_resets, which holds it over its steps).
int launch_decompress_locked(DeviceCtx* ctx, StreamScratch& rec, const BatchTables& t, uint8_t max_wbits, hipStream_t st) {
    const size_t n_streams = t.n;
    if (n_streams == 0) return TAMP_OK;
    const DecompressArgs a = decompress_args(ctx, t);
    const DecodeCall call = {n_streams, max_wbits, t.dict != nullptr};
    if (const DecodeLong gate = decode_wants_long(call); gate.attempt) {  // (tamp_decompress_long_kernel.hpp)
        const int rc = each_long_stream(t, st, [&](const BatchTables& row) { return launch_decompress_long(ctx, rec, gate, row, max_wbits, st); });
        if (rc != 1) return rc;
    }
    DecodeScan scan;
    if (decode_wants_scan(call)) {
        HIP_OK(rec.scan.need(32, false));
        uint32_t* const hdr_scan = static_cast<uint32_t*>(rec.scan.p);
        uint32_t words[4] = {0, 0, 0, 0};
        HIP_OK(hipMemsetAsync(hdr_scan, 0, 16, st));
        const uint32_t sg = (uint32_t)std::min<size_t>((n_streams + 255) / 256, (size_t)ctx->cu_count * 4);
        hipLaunchKernelGGL(tamp_header_scan_kernel, dim3(sg), dim3(256), 0, st, t.in, t.in_off, t.in_len, t.out_cap,
                           (uint32_t)n_streams, (uint32_t)call.bits(), hdr_scan);
        HIP_OK(hipMemcpyAsync(words, hdr_scan, 16, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        scan.found = words[0], scan.longest_in = words[1], scan.window_units = words[2], scan.max_out_cap = words[3];
    }
    DecodeDevice dev = {(uint32_t)ctx->cu_count, false, 0, rec.split.bytes};
    DecodePlan plan = plan_decompress(call, scan, dev);
    if (plan.decoder == Decoder::kSplit) {  // its scratch budget: what the device has free right now (asked for this decoder alone)
        size_t total_b = 0;
        dev.free_known = hipMemGetInfo(&dev.free_bytes, &total_b) == hipSuccess;
        if (!dev.free_known) (void)hipGetLastError();
        plan = plan_decompress(call, scan, dev);
    }
    return run_decode_plan(ctx, rec, a, call, scan, dev, plan, st);
}
int launch_decompress(DeviceCtx* ctx, const BatchTables& t, uint8_t max_wbits, hipStream_t st) {
    if (t.n == 0) return TAMP_OK;
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    return launch_decompress_locked(ctx, rec, t, max_wbits, st);
}

// The size of ONE long stream: the long decoder's front counts output bytes per chunk, their sum is the answer (status 2, all of
// the input consumed) as long as it stays below the stream's limit.  -> 1 when the lane kernel has to answer: the stream fails the
// gate, the chunk starts do not settle, an offset is out of bounds, or the sum reaches the limit (TAMP_OUTPUT_FULL, and how much
// of the input that takes, is the exact loop's to say).
// `t`: the stream's single row (out_cap: its limit or null, out_len: the size).
int launch_decoded_size_long(DeviceCtx* ctx, StreamScratch& rec, const DecodeLong& gate, const BatchTables& t, uint8_t max_wbits, hipStream_t st) {
    LongFront f;
    if (const int rc = long_decode_front(ctx, rec, gate, t, true, max_wbits, false, "size query", st, f); rc != TAMP_OK) return rc;
    uint64_t v = 0;
    for (const uint32_t b : f.outb) v += b;
    if (f.dbg) fprintf(stderr, "[tamp_amd long size query] %llu bytes out, limit %u\n", (unsigned long long)v, f.cap);
    if (v >= f.cap) { timing_end(st); return long_declined(f.dbg, "size query", "output room"); }
    hipLaunchKernelGGL(tamp_long_finish_kernel, dim3(1), dim3(1), 0, st, t.out_len, t.status, t.in_consumed, (uint32_t)v, f.n);
    timing_end(st);
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// tamp_batch_decoded_size on device memory: the parse's size-only build (tamp_decompress_split_kernel.hpp), one launch, no scratch,
// no pre-pass, nothing that waits for `st` -- except for a handful of long streams, which the long decoder's front counts with the
// whole device (and waits as the long decoder does).  `t`: device memory, no slab -- out and out_off are null, out_cap holds the
// limits (may be null), out_len takes the sizes; of the dictionary only the length matters (dict is null).
int launch_decoded_size_locked(DeviceCtx* ctx, StreamScratch& rec, const BatchTables& t, uint8_t max_wbits, hipStream_t st) {
    const size_t n_streams = t.n;
    if (n_streams == 0) return TAMP_OK;
    SplitArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.d = decompress_args(ctx, t);
    sa.d.max_wbits = max_wbits & 0x7F;  // (TAMP_AMD_WINDOW_BITS_EXACT: there is no pre-pass to skip)
    if (const DecodeLong gate = decode_wants_long({n_streams, max_wbits, t.dict_len != 0}); gate.attempt) {
        const int rc = each_long_stream(t, st, [&](const BatchTables& row) { return launch_decoded_size_long(ctx, rec, gate, row, max_wbits, st); });
        if (rc != 1) return rc;
    }
    const SizeGeometry g = size_geometry(n_streams, (uint32_t)ctx->cu_count);
    sa.first = 0, sa.count = (uint32_t)n_streams, sa.spw = g.spw;
    timing_begin(st);
    hipLaunchKernelGGL(tamp_decode_parse_kernel<false>, dim3(g.grid), dim3(256), g.lds, st, sa);
    timing_end(st);
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}
int launch_decoded_size(DeviceCtx* ctx, const BatchTables& t, uint8_t max_wbits, hipStream_t st) {
    if (t.n == 0) return TAMP_OK;
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (one library call at a time enqueues on a stream: the lock rule above StreamScratch)
    return launch_decoded_size_locked(ctx, rec, t, max_wbits, st);
}

// Resumable decoding: one wavefront per decoder object (tamp_decompress_resume_kernel.hpp).
// `object_index` (tamp_batch_decompress_pieces, device memory): row r of the tables acts on object object_index[r]; null: on object r.
int launch_decompress_resume(DeviceCtx* ctx, uint8_t* d_states, size_t stride, uint8_t bits_max, const BatchTables& t, hipStream_t st,
                             const uint32_t* object_index = nullptr) {
    const size_t n_streams = t.n;
    if (n_streams == 0) return TAMP_OK;
    ResumeArgs ra;
    DecompressArgs& a = ra.d;
    a = decompress_args(ctx, t);
    a.dict = nullptr, a.dict_len = 0, a.dict_off = nullptr;  // a custom dictionary is the initial content of the object's window
    a.max_wbits = bits_max;
    ra.states = d_states, ra.state_stride = stride, ra.object_index = object_index;
    const WaveGeometry g = wave_geometry(bits_max, n_streams, ctx->cu_count);
    timing_begin(st);
    const int rc = launch_waves(tamp_decompress_resume_kernel, ra, g, decode_wave_lds(bits_max, g.waves), st);
    timing_end(st);
    if (rc != TAMP_OK) return rc;
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// The size query for decoder objects: one lane per row, one launch, nothing allocated and nothing read back
// (tamp_decoded_size_pieces_kernel.hpp).  `t`: device tables -- out_cap holds the limits (may be null), out_len takes the sizes.
int launch_decoded_size_pieces(DeviceCtx* ctx, const uint8_t* d_states, size_t stride, uint8_t bits_max, const uint32_t* object_index,
                               const BatchTables& t, hipStream_t st) {
    if (t.n == 0) return TAMP_OK;
    SizePiecesArgs a;
    a.states = d_states, a.state_stride = stride, a.object_index = object_index;
    a.in = t.in, a.in_off = t.in_off, a.in_len = t.in_len, a.limit = t.out_cap;
    a.out_len = t.out_len, a.status = t.status, a.in_consumed = t.in_consumed;
    a.n_rows = (uint32_t)t.n, a.max_wbits = bits_max;
    const SizeGeometry g = size_pieces_geometry(t.n, (uint32_t)ctx->cu_count);
    a.spw = g.spw;
    timing_begin(st);
    hipLaunchKernelGGL(tamp_decoded_size_pieces_kernel, dim3(g.grid), dim3(256), g.lds, st, a);
    timing_end(st);
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// Compressor objects below flush granularity: one wavefront per object (tamp_compress_resume_kernel.hpp).
int launch_compress_resume(DeviceCtx* ctx, uint8_t* d_states, size_t stride, uint8_t bits_max, int op, int write_token,
                           const BatchTables& t, hipStream_t st) {
    const size_t n = t.n;
    if (n == 0) return TAMP_OK;
    EncodeResumeArgs a;
    a.states = d_states, a.state_stride = stride;
    a.in = t.in, a.in_off = t.in_off, a.in_len = t.in_len;
    a.out = t.out, a.out_off = t.out_off, a.out_cap = t.out_cap, a.out_len = t.out_len, a.status = t.status;
    a.in_consumed = t.in_consumed;
    a.n_objects = (uint32_t)n, a.op = (uint32_t)op, a.write_token = write_token ? 1u : 0u;
    a.max_wbits = bits_max;
    const WaveGeometry g = wave_geometry(bits_max, n, ctx->cu_count);
    timing_begin(st);
    const int rc = launch_waves(tamp_compress_resume_kernel, a, g, encode_resume_lds(bits_max, g.waves), st);
    timing_end(st);
    if (rc != TAMP_OK) return rc;
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

bool conf_valid(const TampAmdConf* c) {
    return c && c->window >= 8 && c->window <= 15 && c->literal >= 5 && c->literal <= 8;  // compressor.c:208-209
}

// ---------------------------------------------------------------------------------------------
// Host-memory batches.  The caller's arrays live in host memory (pageable or pinned); the batch is cut into chunks of
// consecutive streams and each chunk goes copy-in -> kernel -> copy-out on one of three library streams, so the PCIe
// transfers of neighbouring chunks (both directions) overlap the kernels.  A feeder thread issues copy-in + launch,
// the calling thread issues copy-out: with pageable memory hipMemcpyAsync blocks its caller, and two issuers keep
// both directions busy anyway.  Device staging is kept between calls.  The object calls (tamp_batch_*_resume) and the
// piece / segment calls run here too: their objects' state rows travel with the chunks (HostBatch::states).
// ---------------------------------------------------------------------------------------------
struct HostBatch : BatchTables {  // the caller's arrays, in host memory, and what the host path alone needs to know
    uint8_t* states = nullptr;  // optional per-stream state rows of state_stride bytes: in before the launch, out after it
    size_t state_stride = 0;
    const uint8_t* lead = nullptr;  // one-stream batches only: nlead bytes in front of the stream's input, counted in in_len[0]
    size_t nlead = 0;
    bool exact_out = false;    // never the whole-extent copy-back: nothing behind out_len[i] is written (HostChunk)
    bool drop_failed = false;  // (with exact_out) a stream whose status is not TAMP_OK produces nothing: out_len = 0
    // out == nullptr (tamp_batch_decoded_size): no output bytes at all -- out_off is null, out_cap (the limits, may be null) rides
    // along as a table only and takes no part in the chunks' extents; out_len / status / in_consumed come back as always
    uint64_t slab_off(size_t i) const { return out ? out_off[i] : 0; }
    uint64_t slab_cap(size_t i) const { return out ? out_cap[i] : 0; }
};

struct HostChunk {
    size_t i0, i1;
    uint64_t in_lo, in_hi, out_lo, out_hi;
    // Output slabs tile [out_lo, out_hi) exactly, in stream order: the copy-back may be ONE transfer of the whole
    // extent (bytes of a slab behind out_len[i] are unspecified afterwards, include/tamp_amd.h).  Otherwise -- gaps
    // between slabs, permuted or overlapping extents -- only the out_len[i] bytes of each stream are copied, so
    // nothing outside the produced bytes is ever written in the caller's buffer.
    bool out_packed;
};

// Consecutive streams: a chunk closes once it holds `min_streams` streams and `min_bytes` of data (the larger of its
// input and output extents), or earlier at `max_bytes`.  Needs both offset tables ascending and disjoint, the layout
// every packed batch has; otherwise one chunk covers the whole batch.
void plan_host_chunks(const HostBatch& b, size_t min_streams, uint64_t min_bytes, uint64_t max_bytes,
                      std::vector<HostChunk>& chunks) {
    bool ordered = true;
    uint64_t in_end = 0, out_end = 0, in_max = 0, out_max = 0, in_min = ~0ull, out_min = ~0ull;
    for (size_t i = 0; i < b.n; i++) {
        ordered = ordered && b.in_off[i] >= in_end && b.slab_off(i) >= out_end;
        in_end = b.in_off[i] + b.in_len[i], out_end = b.slab_off(i) + b.slab_cap(i);
        in_max = std::max(in_max, in_end), out_max = std::max(out_max, out_end);
        in_min = std::min(in_min, b.in_off[i]), out_min = std::min(out_min, b.slab_off(i));
    }
    if (!ordered) {
        chunks.push_back({0, b.n, in_min, in_max, out_min, out_max, false});
        return;
    }
    size_t i0 = 0;
    while (i0 < b.n) {
        size_t i1 = i0 + 1;
        for (; i1 < b.n; i1++) {
            const uint64_t have = std::max(b.in_off[i1 - 1] + b.in_len[i1 - 1] - b.in_off[i0],
                                           b.slab_off(i1 - 1) + b.slab_cap(i1 - 1) - b.slab_off(i0));
            const uint64_t with = std::max(b.in_off[i1] + b.in_len[i1] - b.in_off[i0],
                                           b.slab_off(i1) + b.slab_cap(i1) - b.slab_off(i0));
            if ((i1 - i0 >= min_streams && have >= min_bytes) || with > max_bytes) break;
        }
        bool packed = !b.exact_out;
        for (size_t i = i0 + 1; i < i1 && packed; i++) packed = b.slab_off(i) == b.slab_off(i - 1) + b.slab_cap(i - 1);
        chunks.push_back({i0, i1, b.in_off[i0], b.in_off[i1 - 1] + b.in_len[i1 - 1], b.slab_off(i0),
                          b.slab_off(i1 - 1) + b.slab_cap(i1 - 1), packed});
        i0 = i1;
    }
    // a short last chunk is a badly filled launch: give it to its neighbour
    if (chunks.size() >= 2 && chunks.back().i1 - chunks.back().i0 < min_streams / 2) {
        const HostChunk last = chunks.back();
        chunks.pop_back();
        HostChunk& prev = chunks.back();
        prev.out_packed = prev.out_packed && last.out_packed && b.slab_off(last.i0) == prev.out_hi;
        prev.i1 = last.i1, prev.in_hi = last.in_hi, prev.out_hi = last.out_hi;
    }
}

// One chunk on the device: its tables (rows of the chunk; offsets stay absolute, the data pointers are shifted instead; dict: the
// staged dictionary or null; a table the caller left out is null here too) and its state rows (row 0 = the chunk's first stream, or null).
using HostLaunch = std::function<int(const BatchTables& d, uint8_t* d_states, hipStream_t)>;

// `dictionary_len`: the bytes of b.dict to stage (b.dict_len is what the kernels are told).
int run_host_batch(DeviceCtx* ctx, int device, const HostBatch& b, const std::vector<HostChunk>& chunks, size_t dictionary_len,
                   const HostLaunch& launch) {
    using Pipe = DeviceCtx::HostPipe;
    Pipe& P = ctx->pipe;
    std::lock_guard<std::mutex> call_lock(P.mu);
    const uint8_t* d_dict = nullptr;
    if (b.dict && dictionary_len) {
        // one dictionary: at most a window of it; a table of them (b.dict_off): all of it, once per call (the buffer is kept and grows)
        const size_t stage = b.dict_off ? dictionary_len : std::min(dictionary_len, kSeedTable);
        HIP_OK(P.dict.need(std::max(stage, kSeedTable)));
        HIP_OK(hipMemcpy(P.dict.p, b.dict, stage, hipMemcpyHostToDevice));
        d_dict = static_cast<const uint8_t*>(P.dict.p);
    }
    size_t max_in = 0, max_out = 0, max_cnt = 0;
    for (const HostChunk& ch : chunks) {
        max_in = std::max<size_t>(max_in, ch.in_hi - ch.in_lo);
        max_out = std::max<size_t>(max_out, ch.out_hi - ch.out_lo);
        max_cnt = std::max(max_cnt, ch.i1 - ch.i0);
    }
    const int depth = (int)std::min<size_t>(Pipe::kDepth, chunks.size());
    const size_t meta_bytes = max_cnt * (8 + 8 + 8 + 4 + 4 + 4 + 4 + 1) + 64;
    for (int j = 0; j < depth; j++) {
        if (!P.s[j]) HIP_OK(hipStreamCreateWithFlags(&P.s[j], hipStreamNonBlocking));
        HIP_OK(P.in[j].need(max_in + 64));  // the kernels' vector loads may run past the last byte
        HIP_OK(P.out[j].need(max_out + 1));
        HIP_OK(P.meta[j].need(meta_bytes));
        if (b.states) HIP_OK(P.state[j].need(max_cnt * b.state_stride));
    }
    auto slot_of = [&](int j, const HostChunk& ch) {  // the device record of a chunk in slot j
        BatchTables s = b;
        uint8_t* m = static_cast<uint8_t*>(P.meta[j].p);
        auto column = [&](auto*& p, size_t width) {  // (every column has its place, a table the caller left out stays null)
            if (p) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(m);
            m += max_cnt * width;
        };
        column(s.in_off, 8), column(s.out_off, 8), column(s.dict_off, 8), column(s.in_len, 4), column(s.out_cap, 4), column(s.out_len, 4);
        column(s.in_consumed, 4), column(s.status, 1);
        s.in = static_cast<const uint8_t*>(P.in[j].p) - ch.in_lo;
        s.out = b.out ? static_cast<uint8_t*>(P.out[j].p) - ch.out_lo : nullptr;
        s.dict = d_dict;
        s.n = ch.i1 - ch.i0;
        return s;
    };
    auto states_of = [&](int j) { return b.states ? static_cast<uint8_t*>(P.state[j].p) : nullptr; };
    auto feed = [&](size_t k) -> int {  // copy-in + launch of chunk k
        const HostChunk& ch = chunks[k];
        const int j = (int)(k % Pipe::kDepth);
        const BatchTables s = slot_of(j, ch), h = b.rows(ch.i0, ch.i1 - ch.i0);  // the chunk's rows: on the device, in the caller's arrays
        const size_t cnt = s.n;
        hipStream_t st = P.s[j];
        uint8_t* const d_in = static_cast<uint8_t*>(P.in[j].p);
        if (b.nlead) HIP_OK(hipMemcpyAsync(d_in, b.lead, b.nlead, hipMemcpyHostToDevice, st));
        if (ch.in_hi > ch.in_lo + b.nlead)
            HIP_OK(hipMemcpyAsync(d_in + b.nlead, b.in + ch.in_lo, ch.in_hi - ch.in_lo - b.nlead, hipMemcpyHostToDevice, st));
        if (b.states)
            HIP_OK(hipMemcpyAsync(states_of(j), b.states + ch.i0 * b.state_stride, cnt * b.state_stride, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(const_cast<uint64_t*>(s.in_off), h.in_off, cnt * 8, hipMemcpyHostToDevice, st));
        if (h.out_off) HIP_OK(hipMemcpyAsync(const_cast<uint64_t*>(s.out_off), h.out_off, cnt * 8, hipMemcpyHostToDevice, st));
        if (h.dict_off) HIP_OK(hipMemcpyAsync(const_cast<uint64_t*>(s.dict_off), h.dict_off, cnt * 8, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(const_cast<uint32_t*>(s.in_len), h.in_len, cnt * 4, hipMemcpyHostToDevice, st));
        if (h.out_cap) HIP_OK(hipMemcpyAsync(const_cast<uint32_t*>(s.out_cap), h.out_cap, cnt * 4, hipMemcpyHostToDevice, st));
        return launch(s, states_of(j), st);
    };
    auto drain = [&](size_t k) -> int {  // copy-out of chunk k, complete on return
        const HostChunk& ch = chunks[k];
        const int j = (int)(k % Pipe::kDepth);
        const BatchTables s = slot_of(j, ch), h = b.rows(ch.i0, ch.i1 - ch.i0);
        const size_t cnt = s.n;
        hipStream_t st = P.s[j];
        // (a handful of streams -- ONE long stream decoded with room for its worst case: tamp.decompress(100 MB) offers 325 MB --
        // first learn what was produced and copy exactly that: the packed path below would move the whole extent)
        const bool out_packed = ch.out_packed && cnt > 16;
        if (out_packed && ch.out_hi > ch.out_lo)
            HIP_OK(hipMemcpyAsync(b.out + ch.out_lo, P.out[j].p, ch.out_hi - ch.out_lo, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h.out_len, s.out_len, cnt * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h.status, s.status, cnt, hipMemcpyDeviceToHost, st));
        if (h.in_consumed) HIP_OK(hipMemcpyAsync(h.in_consumed, s.in_consumed, cnt * 4, hipMemcpyDeviceToHost, st));
        if (b.states)
            HIP_OK(hipMemcpyAsync(b.states + ch.i0 * b.state_stride, states_of(j), cnt * b.state_stride, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (b.drop_failed)
            for (size_t i = ch.i0; i < ch.i1; i++)
                if (b.status[i] != TAMP_OK) b.out_len[i] = 0;
        if (!b.out) return TAMP_OK;  // (tables only)
        // (staging pays when the extent is mostly produced bytes; a sparse or permuted batch can span gigabytes for a few
        // megabytes of output -- those, and extents above 512 MiB of pinned memory per slot, take the merged copies below)
        size_t produced = 0;
        if (!out_packed)
            for (size_t i = ch.i0; i < ch.i1; i++) produced += b.out_len[i];
        const size_t extent = ch.out_hi - ch.out_lo;
        // (... and a handful of streams with room to spare -- one long stream decoded into 8 x its compressed size -- copy their
        // produced bytes directly: the extent of tamp.decompress(100 MB) is 325 MB for 100 MB of output)
        const bool stage_ok = extent <= ((size_t)512 << 20) && extent <= 8 * produced + ((size_t)1 << 20) &&
                              (cnt > 16 || extent <= produced + produced / 4 + ((size_t)1 << 20));
        if (!out_packed && ch.out_hi > ch.out_lo && stage_ok && !getenv("TAMP_AMD_NO_STAGED_COPYBACK") &&
            P.stage[j].need(ch.out_hi - ch.out_lo) == hipSuccess) {
            // One device-to-pinned transfer of the chunk's whole extent, then exactly the produced bytes of every stream
            // placed by the host: bytes between and behind the slabs are never written.  (One hipMemcpyAsync per stream,
            // the form this replaces and the fallback below, is orders of magnitude slower for 10^5+ padded slabs.)
            uint8_t* stg = static_cast<uint8_t*>(P.stage[j].p);
            HIP_OK(hipMemcpyAsync(stg, P.out[j].p, ch.out_hi - ch.out_lo, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            for (size_t i = ch.i0; i < ch.i1; i++)
                if (b.out_len[i]) memcpy(b.out + b.out_off[i], stg + (b.out_off[i] - ch.out_lo), b.out_len[i]);
        } else if (!out_packed) {
            (void)hipGetLastError();  // (a failed pinned allocation must not poison later calls)
            // exactly the produced bytes of every stream, runs of touching full slabs merged into one transfer
            const uint8_t* dev_out = static_cast<const uint8_t*>(P.out[j].p);
            size_t i = ch.i0;
            while (i < ch.i1) {
                const uint64_t lo = b.out_off[i];
                uint64_t hi = lo + b.out_len[i];
                size_t k = i + 1;
                while (k < ch.i1 && b.out_len[k - 1] == b.out_cap[k - 1] && b.out_off[k] == hi) hi += b.out_len[k], k++;
                if (hi > lo) HIP_OK(hipMemcpyAsync(b.out + lo, dev_out + (lo - ch.out_lo), hi - lo, hipMemcpyDeviceToHost, st));
                i = k;
            }
            HIP_OK(hipStreamSynchronize(st));
        }
        return TAMP_OK;
    };
    if (chunks.size() == 1) {
        int rc = feed(0);
        return rc != TAMP_OK ? rc : drain(0);
    }
    std::mutex m;
    std::condition_variable cv;
    size_t fed = 0, drained = 0;
    int feed_rc = TAMP_OK;
    bool stop = false;
    std::string feed_msg;
    std::thread feeder([&] {
        int rc = hipSetDevice(device) == hipSuccess ? TAMP_OK : TAMP_AMD_NO_DEVICE;
        for (size_t k = 0; k < chunks.size() && rc == TAMP_OK; k++) {
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || k < drained + Pipe::kDepth; });  // slot k % kDepth is free again
                if (stop) return;
            }
            rc = feed(k);
            std::lock_guard<std::mutex> lk(m);
            if (rc == TAMP_OK) fed = k + 1;
            else feed_rc = rc, feed_msg = t_last_error;
            cv.notify_all();
        }
        if (rc != TAMP_OK) {
            std::lock_guard<std::mutex> lk(m);
            if (feed_rc == TAMP_OK) feed_rc = rc;
            cv.notify_all();
        }
    });
    int rc = TAMP_OK;
    for (size_t k = 0; k < chunks.size(); k++) {
        {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return fed > k || feed_rc != TAMP_OK; });
            if (fed <= k) {
                rc = feed_rc;
                snprintf(t_last_error, sizeof t_last_error, "%s", feed_msg.c_str());
                break;
            }
        }
        rc = drain(k);
        if (rc != TAMP_OK) break;
        std::lock_guard<std::mutex> lk(m);
        drained = k + 1;
        cv.notify_all();
    }
    {
        std::lock_guard<std::mutex> lk(m);
        stop = true;
        cv.notify_all();
    }
    feeder.join();
    if (rc != TAMP_OK)
        for (int j = 0; j < depth; j++) (void)hipStreamSynchronize(P.s[j]);  // nothing of this call left in flight
    return rc;
}

// tamp_compressor_init (compressor.c:191-244) on a state + a window buffer that may live apart (the reference-named
// object keeps the window in the caller's buffer)
tamp_res encoder_state_fill(TampAmdEncoderState* s, unsigned char* window, const TampAmdConf* conf, int append,
                            uint8_t window_bits_max) {
    TampAmdConf dflt;
    std::memset(&dflt, 0, sizeof dflt);
    dflt.window = 10, dflt.literal = 8, dflt.extended = 1;  // compressor.c:193-203
    if (!conf) conf = &dflt;
    if (!conf_valid(conf) || conf->window > window_bits_max) return TAMP_INVALID_CONF;
    if (append && (!conf->dictionary_reset || conf->use_custom_dictionary)) return TAMP_INVALID_CONF;  // :210
    std::memset(s, 0, sizeof *s);
    s->window = conf->window, s->literal = conf->literal;
    s->flags = (uint8_t)((conf->use_custom_dictionary ? 1 : 0) | (conf->extended ? 2 : 0) | (conf->dictionary_reset ? 4 : 0) |
                         (append ? 8 : 0) | (conf->lazy_matching ? 16 : 0));
    s->cached_match_index = -1;
    if (!conf->use_custom_dictionary)
        seed_dictionary_host(window, (size_t)1 << conf->window, conf->extended ? conf->literal : 8);
    if (append) {  // FLUSH padded to 16 bits: with the previous stream's trailing FLUSH a dictionary reset (:227-235)
        s->bit_buffer = 0xABu << 23, s->bit_buffer_pos = 16, s->last_was_flush = 1;
    } else {  // header byte (+ a zero byte when dictionary_reset), compressor.c:236-241
        const uint32_t header = header_byte(conf, conf->dictionary_reset);
        s->bit_buffer = header << 24, s->bit_buffer_pos = conf->dictionary_reset ? 16 : 8;
    }
    return TAMP_OK;
}

size_t env_or(const char* name, size_t dflt) {  // tuning knobs of the host-memory path
    const char* e = getenv(name);
    const long v = e ? atol(e) : 0;
    return v > 0 ? (size_t)v : dflt;
}

// Chunks of a host-memory decode batch, and of the object calls (tamp_batch_*_resume): the lane-per-stream decoders want
// tens of thousands of streams per launch (launch_decompress)
std::vector<HostChunk> plan_wide_chunks(const DeviceCtx* ctx, const HostBatch& b) {
    std::vector<HostChunk> chunks;
    plan_host_chunks(b, env_or("TAMP_AMD_HOST_CHUNK_STREAMS", (size_t)ctx->cu_count * 128),
                     (uint64_t)env_or("TAMP_AMD_HOST_CHUNK_MB", 32) << 20, 1ull << 30, chunks);
    return chunks;
}

// TAMP_AMD_ALL_DEVICES with host memory: the streams are independent, so the batch is cut into one contiguous range
// per visible device, balanced by input bytes, and each range runs the host-memory path of
// its device on its own host thread.  No data moves between devices; results land in the caller's arrays directly.
int device_fanout_count() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return 0;
    const char* e = getenv("TAMP_AMD_FANOUT");  // tests: more shards than devices (they share device i % count)
    const int forced = e ? atoi(e) : 0;
    return forced > 0 ? forced : count;
}

template <class Call>  // Call(device, the shard's rows) -> library-level return code
int fan_out_over_devices(const BatchTables& t, const Call& call) {
    const uint32_t* const in_len = t.in_len;
    const size_t n_streams = t.n;
    const int shards = device_fanout_count();
    int devices = 0;
    (void)hipGetDeviceCount(&devices);
    if (shards < 1 || devices < 1) {
        snprintf(t_last_error, sizeof t_last_error, "no HIP device visible");
        return TAMP_AMD_NO_DEVICE;
    }
    uint64_t total = 0;
    for (size_t i = 0; i < n_streams; i++) total += in_len[i];
    std::vector<size_t> cut(shards + 1, n_streams);
    cut[0] = 0;
    {
        uint64_t run = 0;
        size_t i = 0;
        for (int r = 1; r < shards; r++) {
            const uint64_t target = total / (uint64_t)shards * (uint64_t)r;
            while (i < n_streams && (total ? run < target : i < n_streams * (size_t)r / (size_t)shards)) run += in_len[i++];
            cut[r] = i;
        }
    }
    std::vector<int> rcs(shards, TAMP_OK);
    std::vector<std::string> msgs(shards);
    std::vector<std::thread> workers;
    for (int r = 0; r < shards; r++) {
        if (cut[r + 1] == cut[r]) continue;
        workers.emplace_back([&, r] {
            rcs[r] = call(r % devices, t.rows(cut[r], cut[r + 1] - cut[r]));
            if (rcs[r] != TAMP_OK) msgs[r] = t_last_error;
        });
    }
    for (std::thread& w : workers) w.join();
    for (int r = 0; r < shards; r++)
        if (rcs[r] != TAMP_OK) {
            snprintf(t_last_error, sizeof t_last_error, "shard %d: %s", r, msgs[r].c_str());
            return rcs[r];
        }
    return TAMP_OK;
}

// What every batch call refuses before it looks for a device (each entry point adds its own in front of or behind this): a missing
// table (`slabs`: the call writes output bytes, so out_off and out_cap are tables it needs), more streams than 32 bits count, a
// memory kind there is none of -- looked at before TAMP_AMD_ALL_DEVICES, which takes host memory (device pointers belong to one device).
int batch_refused(const BatchTables& t, bool slabs, int mem, int device) {
    if (t.n && (!t.in_off || !t.in_len || !t.out_len || !t.status || (slabs && (!t.out_off || !t.out_cap)))) return TAMP_AMD_BAD_ARGUMENT;
    if (t.n > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    if (mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) return TAMP_AMD_BAD_ARGUMENT;
    if (device == TAMP_AMD_ALL_DEVICES && mem != TAMP_AMD_MEM_HOST) return TAMP_AMD_BAD_ARGUMENT;
    return TAMP_OK;
}

// Behind the checks: `one(ctx, device, tables)` on the call's device -- or, for TAMP_AMD_ALL_DEVICES, on every device with its shard.
template <class One>
int on_devices(const BatchTables& t, int device, const One& one) {
    auto on_device = [&](int dev, const BatchTables& shard) {
        DeviceCtx* ctx = nullptr;
        const int rc = get_ctx(dev, &ctx);
        return rc != TAMP_OK ? rc : one(ctx, dev, shard);
    };
    return device == TAMP_AMD_ALL_DEVICES ? fan_out_over_devices(t, on_device) : on_device(device, t);
}

// The batch calls behind their entry points, on the record.  Each *_dicts call is the whole of its plain twin plus a per-stream
// dictionary offset table; the plain call passes none (dict_off = null) and behaves as it always has.
int batch_compress(const TampAmdConf* conf, const BatchTables& t, uint32_t max_in_len, int mem, int device, void* stream) {
    if (!conf) return TAMP_AMD_BAD_ARGUMENT;
    if (const int rc = batch_refused(t, true, mem, device)) return rc;
    // (a table selects among CUSTOM dictionaries: the custom bit sits in the one header byte the launch shares)
    if (t.dict_off && (!conf->use_custom_dictionary || !t.dict)) return TAMP_AMD_BAD_ARGUMENT;
    if (mem == TAMP_AMD_MEM_HOST && !max_in_len) {  // (over the whole call: every shard and chunk takes the same build)
        for (size_t i = 0; i < t.n; i++) max_in_len = std::max(max_in_len, t.in_len[i]);
        if (!max_in_len) max_in_len = 16;
    }
    return on_devices(t, device, [&](DeviceCtx* ctx, int dev, const BatchTables& t) -> int {
        const bool bad_conf = !conf_valid(conf) || (conf->use_custom_dictionary && !t.dict);
        if (mem == TAMP_AMD_MEM_DEVICE) {
            hipStream_t st = static_cast<hipStream_t>(stream);
            if (bad_conf) {  // tamp_compressor_init would have returned TAMP_INVALID_CONF for every stream
                HIP_OK(hipMemsetAsync(t.status, (uint8_t)(int8_t)TAMP_INVALID_CONF, t.n, st));
                HIP_OK(hipMemsetAsync(t.out_len, 0, t.n * sizeof(uint32_t), st));
                return TAMP_OK;
            }
            return launch_compress(ctx, conf, t, max_in_len, st);
        }
        // ---- host memory: stage, run, copy back ----
        if (bad_conf) {
            for (size_t i = 0; i < t.n; i++) t.status[i] = TAMP_INVALID_CONF, t.out_len[i] = 0;
            return TAMP_OK;
        }
        if (t.n == 0) return TAMP_OK;
        HostBatch b{t};
        if (!conf->use_custom_dictionary) b.dict = nullptr;
        std::vector<HostChunk> chunks;
        // a chunk fills the device three times over (256 CUs x 6 workgroups = 1,536 streams at once); measured best for
        // 4 KiB streams (DESIGN_HISTORY.md), and at least 16 MiB so that short messages do not drown in call overhead
        plan_host_chunks(b, env_or("TAMP_AMD_HOST_CHUNK_STREAMS", (size_t)ctx->cu_count * 18),
                         (uint64_t)env_or("TAMP_AMD_HOST_CHUNK_MB", 16) << 20, 1ull << 30, chunks);
        return run_host_batch(ctx, dev, b, chunks, t.dict_off ? t.dict_len : (size_t)1 << conf->window,
                              [&](const BatchTables& d, uint8_t*, hipStream_t cs) { return launch_compress(ctx, conf, d, max_in_len, cs); });
    });
}

// One long buffer as dictionary-reset segments (tamp_amd_compress_resets; kernels and format facts: tamp_reset_segments_kernel.hpp).
// Segment k = input bytes [k * interval, (k + 1) * interval), compressed by the batch kernel as a stream of its own into slab k of
// the stream's scratch: opened by the append lead, closed by a FLUSH token -- all but the call's last one, which a second launch
// of one stream closes without (tamp.compress ends with flush(write_token = False)).  Scan + gather pack the slabs into the
// caller's buffer.  When the slabs outgrow the scratch budget (the split decoder's rule: a quarter of the free memory, what the
// record already holds counting as free, 8 GiB at most) the call runs in slices of at most 2^20 segments; the output base and the
// status so far ride from slice to slice in device memory, so a device-memory call waits for nothing.
// All pointers: device memory.  out_len / status: one element each; reset_off: K - 1 elements or null.
int launch_compress_resets(DeviceCtx* ctx, const TampAmdConf* conf, const uint8_t* d_in, uint64_t in_len, uint32_t interval,
                           uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_len, int8_t* d_status, uint64_t* d_reset_off,
                           hipStream_t st) {
    const uint64_t K = reset_segment_count(in_len, interval);
    const uint32_t slab = reset_slab_bytes(in_len, interval, conf->literal);
    // (what sizes the compress kernel's block: the longest segment, with the floor of 16 the one-stream calls give plan_compress)
    const uint32_t longest = (uint32_t)std::min<uint64_t>(interval, std::max<uint64_t>(in_len, 16));
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    const size_t row_bytes = 8 + 8 + 8 + 4 + 4 + 4 + 1;  // in_off, out_off, dst_off, in_len, out_cap, out_len, status
    size_t budget = (size_t)8 << 30, free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, std::max((free_b + rec.resets.bytes) / 4, rec.resets.bytes));
    else (void)hipGetLastError();
    size_t slice = (size_t)std::min<uint64_t>(K, (uint64_t)1 << 20);
    slice = std::min(slice, std::max<size_t>(budget / ((size_t)slab + row_bytes), 1));
    if (const char* e = getenv("TAMP_AMD_RESETS_SLICE")) { const long v = atol(e); if (v > 0) slice = std::min(slice, (size_t)v); }  // (tuning / tests)
    const size_t tab_bytes = (256 + slice * row_bytes + 64 + 255) & ~(size_t)255;
    HIP_OK(rec.resets.need(tab_bytes + slice * (size_t)slab + 64));
    uint8_t* const base = static_cast<uint8_t*>(rec.resets.p);
    ResetCarry* const carry = reinterpret_cast<ResetCarry*>(base);
    uint64_t* const in_off = reinterpret_cast<uint64_t*>(base + 256);
    uint64_t* const out_off = in_off + slice;
    uint64_t* const dst_off = out_off + slice;
    uint32_t* const seg_in = reinterpret_cast<uint32_t*>(dst_off + slice);
    uint32_t* const seg_cap = seg_in + slice;
    uint32_t* const seg_len = seg_cap + slice;
    int8_t* const seg_status = reinterpret_cast<int8_t*>(seg_len + slice);
    uint8_t* const slabs = base + tab_bytes;
    HIP_OK(hipMemsetAsync(carry, 0, sizeof(ResetCarry), st));
    BatchTables t;
    t.in = in_len ? d_in : base;  // (an empty input: memory of the library's own to point at)
    t.in_off = in_off, t.in_len = seg_in, t.out = slabs, t.out_off = out_off, t.out_cap = seg_cap, t.out_len = seg_len, t.status = seg_status;
    const SegmentSpec with_token = {2, (uint16_t)(0xABu << 7), kSegFlushToken}, without = {2, (uint16_t)(0xABu << 7), 0};
    const uint8_t header = header_byte(conf, true);
    if (getenv("TAMP_AMD_RESETS_DEBUG"))
        fprintf(stderr, "[tamp_amd resets] compress: %llu segments of %u bytes, slab %u, %zu per slice\n", (unsigned long long)K, interval, slab, slice);
    const CallTiming call_timing(st);
    for (uint64_t k0 = 0; k0 < K; k0 += slice) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(slice, K - k0);
        const bool last = k0 + cnt == K;
        const ResetRowsArgs rows = {k0, cnt, interval, in_len, slab, in_off, seg_in, out_off, seg_cap};
        hipLaunchKernelGGL(tamp_reset_rows_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, rows);
        t.n = cnt;
        const uint32_t closed = last ? cnt - 1 : cnt;  // segments that end with a reset
        if (const int rc = launch_compress_locked(ctx, rec, conf, t.rows(0, closed), longest, st, &with_token, nullptr)) return rc;
        if (last)
            if (const int rc = launch_compress_locked(ctx, rec, conf, t.rows(closed, 1), longest, st, &without, nullptr)) return rc;
        const ResetScanArgs scan = {seg_len, seg_status, cnt, k0, dst_off, d_reset_off, carry, last ? 1u : 0u, out_cap, d_out_len, d_status};
        hipLaunchKernelGGL(tamp_reset_scan_kernel, dim3(1), dim3(kResetScanTile), 0, st, scan);
        const ResetGatherArgs gather = {slabs, slab, cnt, seg_len, dst_off, d_out, out_cap, k0 == 0 ? 1u : 0u, (uint32_t)header};
        const uint32_t grid = (uint32_t)std::min<size_t>(cnt, (size_t)ctx->cu_count * 8);
        hipLaunchKernelGGL(tamp_reset_gather_kernel, dim3(grid), dim3(256), 0, st, gather);
    }
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// tamp_amd_compress_resets behind its checks.  Host memory: the input goes to the device in one piece and exactly the produced
// bytes, the results and the reset offsets come back, on the host pipeline's first stream (one host-memory call per device at a time).
int compress_resets(const TampAmdConf* conf, const uint8_t* in, uint64_t in_len, uint32_t interval, uint8_t* out, uint64_t out_cap,
                    uint64_t* out_len, int8_t* status, uint64_t* reset_off, int mem, int device, void* stream) {
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE)
        return launch_compress_resets(ctx, conf, in, in_len, interval, out, out_cap, out_len, status, reset_off, static_cast<hipStream_t>(stream));
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    const uint64_t K = reset_segment_count(in_len, interval);
    const uint64_t room = std::min<uint64_t>(out_cap, tamp_amd_compress_resets_bound(in_len, interval, conf->literal));
    HIP_OK(P.in[0].need(in_len + 64));  // the kernels' vector loads may run past the last byte
    HIP_OK(P.out[0].need(room + 1));
    HIP_OK(P.meta[0].need(16 + (reset_off ? 8 * (size_t)K : 0)));  // (the offsets only when asked for: K can be 2^32 - 1)
    uint8_t* const d_in = static_cast<uint8_t*>(P.in[0].p);
    uint8_t* const d_out = static_cast<uint8_t*>(P.out[0].p);
    uint64_t* const d_len = static_cast<uint64_t*>(P.meta[0].p);
    int8_t* const d_status = reinterpret_cast<int8_t*>(d_len + 1);
    uint64_t* const d_reset = d_len + 2;
    if (in_len) HIP_OK(hipMemcpyAsync(d_in, in, in_len, hipMemcpyHostToDevice, st));
    // (`room` instead of out_cap: a total above the bound does not exist, one above out_cap is above `room` as well)
    if (const int rc = launch_compress_resets(ctx, conf, d_in, in_len, interval, d_out, room, d_len, d_status, reset_off ? d_reset : nullptr, st)) return rc;
    HIP_OK(hipMemcpyAsync(out_len, d_len, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(status, d_status, 1, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (*status != TAMP_OK || *out_len == 0) return TAMP_OK;
    HIP_OK(hipMemcpyAsync(out, d_out, *out_len, hipMemcpyDeviceToHost, st));
    if (reset_off && K > 1) HIP_OK(hipMemcpyAsync(reset_off, d_reset, 8 * (size_t)(K - 1), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return TAMP_OK;
}

// A batch of buffers, every one cut into dictionary-reset segments (tamp_batch_compress_resets; kernels and the two-table order:
// tamp_reset_segments_kernel.hpp).  The segments of ALL streams are the units of work: the closed ones (a reset behind them) run
// first, in slices of the budget rule above, then every stream's open one, each slice as rows -> compress -> place / finish ->
// gather.  What a stream's closed segments took rides per stream in device memory, so a stream may straddle slices.
// `t`: device memory.  `counted`: the closed segments of the batch (sum of K_i - 1) and its longest stream when the caller has them
// from host tables, else null: the one 16-byte record a device-memory call reads back, once, and waits for.  The slabs are sized
// from that longest stream, never from `max_in_len`: the caller's hint sizes the compress kernel's block alone (a stale one costs
// speed, never bytes, as for tamp_batch_compress) -- longest = min(N, max(max_in_len, 16)), the true longest stream standing in
// for a hint of 0 (unknown).
// `index`: the reset index of tamp_batch_compress_resets_index, all of it optional.  first: n + 1 entries, the closed_first table
// (copied from the scratch on the call's stream); off: per closed segment of the batch the offset, in its stream, of the byte behind
// its reset (the gather's store); cap: the entries `off` has room for -- a batch with more closed segments is refused before anything
// is launched that writes to the caller's memory.
struct BatchResetCounted { uint64_t closed, longest; };
struct BatchResetIndex { uint64_t* first; uint32_t* off; uint64_t cap; };
int launch_compress_batch_resets(DeviceCtx* ctx, const TampAmdConf* conf, const BatchTables& t, uint32_t interval, uint32_t max_in_len,
                                 const BatchResetCounted* counted, const BatchResetIndex& index, hipStream_t st) {
    const uint64_t n = t.n;
    if (n == 0) return TAMP_OK;
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    // per stream: closed_first (n + 1) and the longest stream, start, end, lowest, highest, behind the carry
    const size_t streams_bytes = (256 + (n + 2) * 8 + n * (8 + 8 + 4 + 4) + 255) & ~(size_t)255;
    auto count_streams = [&]() -> int {  // the per-stream part of the scratch: zeroed, the closed segments counted and scanned
        uint8_t* const base = static_cast<uint8_t*>(rec.resets.p);
        HIP_OK(hipMemsetAsync(base, 0, streams_bytes, st));
        const BatchResetCountArgs count = {t.in_len, n, interval, reinterpret_cast<uint64_t*>(base + 256)};
        hipLaunchKernelGGL(tamp_batch_reset_count_kernel, dim3(1), dim3(kResetScanTile), 0, st, count);
        return TAMP_OK;
    };
    BatchResetCounted have = counted ? *counted : BatchResetCounted{0, 0};
    if (!counted) {
        HIP_OK(rec.resets.need(streams_bytes + 64));
        if (const int rc = count_streams()) return rc;
        HIP_OK(hipMemcpyAsync(&have, static_cast<uint8_t*>(rec.resets.p) + 256 + n * 8, sizeof have, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    if (index.off && have.closed > index.cap) {
        snprintf(t_last_error, sizeof t_last_error, "reset index: %llu entries, room for %llu", (unsigned long long)have.closed, (unsigned long long)index.cap);
        return TAMP_AMD_BAD_ARGUMENT;
    }
    const uint32_t slab = batch_reset_slab_bytes((uint32_t)std::max<uint64_t>(have.longest, 1), interval, conf->literal);
    const uint32_t longest = (uint32_t)std::min<uint64_t>(interval, std::max<uint64_t>(max_in_len ? max_in_len : have.longest, 16));
    const uint64_t closed = have.closed;
    const size_t row_bytes = 8 + 8 + 8 + 4 + 4 + 4 + 4 + 1;  // in_off, out_off, pos, in_len, out_cap, out_len, owner, status
    size_t budget = (size_t)8 << 30, free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, std::max((free_b + rec.resets.bytes) / 4, rec.resets.bytes));
    else (void)hipGetLastError();
    size_t slice = (size_t)std::min<uint64_t>(std::max<uint64_t>(closed, n), (uint64_t)1 << 20);
    slice = std::min(slice, std::max<size_t>(budget / ((size_t)slab + row_bytes), 1));
    if (const char* e = getenv("TAMP_AMD_RESETS_SLICE")) { const long v = atol(e); if (v > 0) slice = std::min(slice, (size_t)v); }  // (tuning / tests)
    const size_t tab_bytes = (slice * row_bytes + 64 + 255) & ~(size_t)255;
    const size_t all_bytes = streams_bytes + tab_bytes + slice * (size_t)slab + 64;
    // (growth loses the contents: the count is then taken again, a tiny kernel)
    const bool recount = counted || all_bytes > rec.resets.bytes;
    HIP_OK(rec.resets.need(all_bytes));
    if (recount)
        if (const int rc = count_streams()) return rc;
    uint8_t* const base = static_cast<uint8_t*>(rec.resets.p);
    ResetCarry* const carry = reinterpret_cast<ResetCarry*>(base);
    uint64_t* const closed_first = reinterpret_cast<uint64_t*>(base + 256);
    if (index.first) HIP_OK(hipMemcpyAsync(index.first, closed_first, (n + 1) * 8, hipMemcpyDeviceToDevice, st));
    BatchResetStreams per;
    per.start = closed_first + n + 2, per.end = per.start + n;
    per.lowest = reinterpret_cast<int32_t*>(per.end + n), per.highest = per.lowest + n;
    uint8_t* const tab = base + streams_bytes;
    uint64_t* const in_off = reinterpret_cast<uint64_t*>(tab);
    uint64_t* const out_off = in_off + slice;
    uint64_t* const pos = out_off + slice;
    uint32_t* const seg_in = reinterpret_cast<uint32_t*>(pos + slice);
    uint32_t* const seg_cap = seg_in + slice;
    uint32_t* const seg_len = seg_cap + slice;
    uint32_t* const owner = seg_len + slice;
    int8_t* const seg_status = reinterpret_cast<int8_t*>(owner + slice);
    uint8_t* const slabs = tab + tab_bytes;
    BatchTables seg;
    seg.in = t.in ? t.in : base, seg.in_off = in_off, seg.in_len = seg_in;  // (no input at all: memory of the library's own to point at)
    seg.out = slabs, seg.out_off = out_off, seg.out_cap = seg_cap, seg.out_len = seg_len, seg.status = seg_status;
    const SegmentSpec with_token = {2, (uint16_t)(0xABu << 7), kSegFlushToken}, without = {2, (uint16_t)(0xABu << 7), 0};
    const uint32_t header = header_byte(conf, true);
    if (getenv("TAMP_AMD_RESETS_DEBUG"))
        fprintf(stderr, "[tamp_amd resets] batch compress: %llu streams, %llu closed segments of %u bytes, slab %u, %zu per slice, %llu slices\n",
                (unsigned long long)n, (unsigned long long)closed, interval, slab, slice,
                (unsigned long long)((closed + slice - 1) / slice + (n + slice - 1) / slice));
    const CallTiming call_timing(st);
    for (int open = 0; open < 2; open++) {
        const uint64_t rows_total = open ? n : closed;
        for (uint64_t r0 = 0; r0 < rows_total; r0 += slice) {
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(slice, rows_total - r0);
            const BatchResetRowsArgs rows = {closed_first, t.in_off, t.in_len, n, r0, cnt, (uint32_t)open, interval, slab,
                                             in_off, seg_in, out_off, seg_cap, owner};
            hipLaunchKernelGGL(tamp_batch_reset_rows_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, rows);
            seg.n = cnt;
            if (const int rc = launch_compress_locked(ctx, rec, conf, seg, longest, st, open ? &without : &with_token, nullptr)) return rc;
            if (open) {
                const BatchResetFinishArgs finish = {seg_len, seg_status, cnt, r0, per, t.out_cap, t.out_len, t.status};
                hipLaunchKernelGGL(tamp_batch_reset_finish_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, finish);
            } else {
                const BatchResetPlaceArgs place = {seg_len, seg_status, owner, cnt, r0, closed_first, pos, per, carry};
                hipLaunchKernelGGL(tamp_batch_reset_place_kernel, dim3(1), dim3(kResetScanTile), 0, st, place);
            }
            const BatchResetGatherArgs gather = {slabs, slab, cnt, (uint32_t)open, r0, seg_len, owner, pos, closed_first, per,
                                                 t.out, t.out_off, t.out_cap, header, index.off};
            const uint32_t grid = (uint32_t)std::min<size_t>(cnt, (size_t)ctx->cu_count * 8);
            hipLaunchKernelGGL(tamp_batch_reset_gather_kernel, dim3(grid), dim3(256), 0, st, gather);
        }
    }
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// tamp_batch_compress_resets behind its checks.  Host memory, on the host pipeline's kept buffers and first stream (one host-memory
// call per device at a time): the tables and the input's extent go to the device in one piece each; the output slabs lie back to
// back there, each as long as its stream can get or as the caller allows, whichever is less; the two result tables come back, then
// exactly the produced bytes of every stream -- through one pinned transfer of the slabs when that is at most 512 MiB, else stream
// by stream.
int batch_compress_resets(const TampAmdConf* conf, const BatchTables& t, uint32_t interval, uint32_t max_in_len, const BatchResetIndex& index,
                          int mem, int device, void* stream) {
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE) return launch_compress_batch_resets(ctx, conf, t, interval, max_in_len, nullptr, index, static_cast<hipStream_t>(stream));
    const size_t n = t.n;
    if (n == 0) return TAMP_OK;
    uint64_t closed = 0;
    uint32_t longest = 0;
    std::vector<uint64_t> h_out_off(n);
    std::vector<uint32_t> h_cap(n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t len = t.in_len[i];
        longest = std::max(longest, len);
        closed += batch_reset_closed_count(len, interval);
        h_cap[i] = (uint32_t)std::min<uint64_t>(t.out_cap[i], reset_stream_bound(len, interval, conf->literal));
    }
    if (index.off && closed > index.cap) return TAMP_AMD_BAD_ARGUMENT;  // (before anything is written, the device path's rule)
    const HostExtent ext(t.in_off, t.in_len, n);
    const uint64_t room = dense_slabs(h_cap.data(), n, h_out_off.data());
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    HIP_OK(P.in[0].need(ext.bytes() + 64));  // the kernels' vector loads may run past the last byte
    HIP_OK(P.out[0].need(room + 1));
    TableCarver m;
    const auto m_in_off = m.take<uint64_t>(n), m_out_off = m.take<uint64_t>(n);
    const auto m_in_len = m.take<uint32_t>(n), m_cap = m.take<uint32_t>(n), m_out_len = m.take<uint32_t>(n);
    const auto m_status = m.take<int8_t>(n);
    const auto m_reset_off = m.take<uint32_t>(index.off ? closed : 0);  // the reset index, behind the tables
    HIP_OK(P.meta[0].need(m.bytes()));
    void* const mp = P.meta[0].p;
    BatchTables d;
    d.in = static_cast<const uint8_t*>(P.in[0].p), d.in_off = m_in_off.in(mp), d.in_len = m_in_len.in(mp);
    d.out = static_cast<uint8_t*>(P.out[0].p), d.out_off = m_out_off.in(mp), d.out_cap = m_cap.in(mp);
    d.out_len = m_out_len.in(mp), d.status = m_status.in(mp), d.n = n;
    if (ext.bytes()) HIP_OK(hipMemcpyAsync(P.in[0].p, t.in + ext.lo, ext.bytes(), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_in_off.in(mp), ext.off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_out_off.in(mp), h_out_off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_in_len.in(mp), t.in_len, n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_cap.in(mp), h_cap.data(), n * 4, hipMemcpyHostToDevice, st));
    (void)max_in_len;  // (the tables are here: the longest stream is known exactly and stands for the caller's hint)
    const BatchResetCounted counted = {closed, longest};
    uint32_t* const d_reset_off = index.off ? m_reset_off.in(mp) : nullptr;
    // (the first table is the host's own count below; the entries come back with the results)
    if (const int rc = launch_compress_batch_resets(ctx, conf, d, interval, std::max(longest, 1u), &counted, {nullptr, d_reset_off, closed}, st)) return rc;
    HIP_OK(hipMemcpyAsync(t.out_len, d.out_len, n * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(t.status, d.status, n, hipMemcpyDeviceToHost, st));
    if (index.off && closed) HIP_OK(hipMemcpyAsync(index.off, d_reset_off, closed * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (index.first) {
        uint64_t run = 0;
        for (size_t i = 0; i < n; i++) index.first[i] = run, run += batch_reset_closed_count(t.in_len[i], interval);
        index.first[n] = run;
    }
    return copy_back_slabs(P, st, d.out, room, h_out_off.data(), t.out, t.out_off, t.out_len, n);
}

// Reading a stream with dictionary resets back (tamp_amd_decompress_resets): the long-stream decoder's front settles the token
// starts of every chunk, tamp_reset_find_kernel reports the FLUSH pairs, the host merges the reports into the resets' positions
// (tamp_reset_merge.hpp), the segments between them are staged behind the stream's two header bytes as K streams of their own,
// the size build of the split decoder's parse sizes them, and ONE decode call of K streams writes them back to back into the
// caller's buffer.  -> TAMP_OK: done, results in *out_len / *status / *consumed (host memory); 1: declined BEFORE anything was
// written (the caller runs the exact path); an error code (TAMP_ERROR: the batch decode disagreed with the size build).  `rec`: locked by the caller.  d_out == null: the size alone.
int decompress_resets_declined(bool dbg, const char* why) {
    if (dbg) fprintf(stderr, "[tamp_amd resets] declined: %s\n", why);
    return 1;
}
int launch_decompress_resets(DeviceCtx* ctx, StreamScratch& rec, const uint8_t* d_in, uint32_t n, uint8_t* d_out, uint32_t cap,
                             uint8_t max_wbits, hipStream_t st, uint32_t* out_len, int8_t* status, uint32_t* consumed) {
    const bool dbg = getenv("TAMP_AMD_RESETS_DEBUG") != nullptr;
    DecodeLong gate = {true, 256u << 10, true, true};
    if (const char* e = getenv("TAMP_AMD_RESETS_MIN")) { const long v = atol(e); if (v >= 64) gate.min_len = (uint32_t)v; }
    if (n < gate.min_len || n > kMaxDecodeIn - 512) return decompress_resets_declined(dbg, "length");
    // the stream's row for the front, in device memory
    HIP_OK(rec.resets.need(256));
    {
        const uint64_t zero = 0;
        uint8_t* const row = static_cast<uint8_t*>(rec.resets.p);
        HIP_OK(hipMemcpyAsync(row, &zero, 8, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(row + 8, &n, 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(row + 12, &cap, 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));  // (the sources are locals)
    }
    BatchTables row;
    {
        uint8_t* const r = static_cast<uint8_t*>(rec.resets.p);
        row.in = d_in, row.in_off = reinterpret_cast<const uint64_t*>(r), row.in_len = reinterpret_cast<const uint32_t*>(r + 8);
        row.out_cap = reinterpret_cast<const uint32_t*>(r + 12), row.n = 1;
    }
    LongFront f;
    if (const int rc = long_decode_front(ctx, rec, gate, row, false, max_wbits, false, "front", st, f, true); rc != TAMP_OK) return rc;
    timing_end(st);  // (the front began the pair; the steps below make their own)
    // where the resets are
    const uint32_t N = f.N;
    HIP_OK(rec.resets.need((size_t)N * sizeof(ResetChunkReport) + 256));
    ResetChunkReport* const d_rep = static_cast<ResetChunkReport*>(rec.resets.p);
    const ResetFindArgs find = {f.la, d_rep};
    hipLaunchKernelGGL(tamp_reset_find_kernel, dim3(f.lg), dim3(64), 0, st, find);
    std::vector<ResetChunkReport> rep(N);
    HIP_OK(hipMemcpyAsync(rep.data(), d_rep, (size_t)N * sizeof(ResetChunkReport), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    std::vector<uint32_t> boundaries, seg_start, seg_len;
    if (!reset_merge(rep.data(), N, boundaries)) return decompress_resets_declined(dbg, "resets per chunk");
    if (!reset_segments_of(boundaries, f.hs, n, seg_start, seg_len)) return decompress_resets_declined(dbg, "positions");
    const size_t K = seg_start.size();
    // the staged streams and their tables: in_off, out_off (u64), src_off, src_len, in_len, out_cap, size, consumed (u32), status
    std::vector<uint64_t> in_off(K), out_off(K);
    std::vector<uint32_t> in_len(K), size(K), used(K);
    std::vector<int8_t> st8(K);
    uint64_t staged = 0;
    for (size_t k = 0; k < K; k++) in_off[k] = staged, in_len[k] = seg_len[k] + 2, staged += ((uint64_t)seg_len[k] + 2 + 3) & ~3ull;
    const size_t tab_bytes = (K * (8 + 8 + 6 * 4 + 1) + 64 + 255) & ~(size_t)255;
    if (rec.resets.need(tab_bytes + staged + 64) != hipSuccess) { (void)hipGetLastError(); return decompress_resets_declined(dbg, "scratch"); }
    uint8_t* const base = static_cast<uint8_t*>(rec.resets.p);
    uint64_t* const d_in_off = reinterpret_cast<uint64_t*>(base);
    uint64_t* const d_out_off = d_in_off + K;
    uint32_t* const d_src_off = reinterpret_cast<uint32_t*>(d_out_off + K);
    uint32_t* const d_src_len = d_src_off + K;
    uint32_t* const d_in_len = d_src_len + K;
    uint32_t* const d_cap = d_in_len + K;
    uint32_t* const d_size = d_cap + K;
    uint32_t* const d_used = d_size + K;
    int8_t* const d_st = reinterpret_cast<int8_t*>(d_used + K);
    uint8_t* const stage = base + tab_bytes;
    HIP_OK(hipMemcpyAsync(d_in_off, in_off.data(), K * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_src_off, seg_start.data(), K * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_src_len, seg_len.data(), K * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_in_len, in_len.data(), K * 4, hipMemcpyHostToDevice, st));
    const ResetStageArgs sa = {d_in, d_src_off, d_src_len, d_in_off, stage, (uint32_t)K, ((f.hd.wbits - 8) << 5) | ((f.hd.lbits - 5) << 3) | ((uint32_t)f.hd.extended << 1) | 1u}  /* header byte 0; byte 1 is zero */;
    hipLaunchKernelGGL(tamp_reset_stage_kernel, dim3((uint32_t)std::min<size_t>(K, (size_t)ctx->cu_count * 8)), dim3(256), 0, st, sa);
    BatchTables t;
    t.in = stage, t.in_off = d_in_off, t.in_len = d_in_len, t.out_len = d_size, t.status = d_st, t.in_consumed = d_used, t.n = K;
    if (const int rc = launch_decoded_size_locked(ctx, rec, t, max_wbits, st)) return rc;
    HIP_OK(hipMemcpyAsync(size.data(), d_size, K * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(used.data(), d_used, K * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(st8.data(), d_st, K, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    uint64_t total = 0;
    for (size_t k = 0; k < K; k++) {
        if (st8[k] != TAMP_INPUT_EXHAUSTED || used[k] != in_len[k]) return decompress_resets_declined(dbg, "segment");
        out_off[k] = total, total += size[k];
    }
    // (room that is used up exactly is the exact decoder's to judge, as in the long-stream decoder)
    if (total >= cap) return decompress_resets_declined(dbg, "output room");
    if (d_out) {
        HIP_OK(hipMemcpyAsync(d_out_off, out_off.data(), K * 8, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_cap, size.data(), K * 4, hipMemcpyHostToDevice, st));
        t.out = d_out, t.out_off = d_out_off, t.out_cap = d_cap;
        if (const int rc = launch_decompress_locked(ctx, rec, t, max_wbits, st)) return rc;
        std::vector<uint32_t> got(K);
        HIP_OK(hipMemcpyAsync(got.data(), d_size, K * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(st8.data(), d_st, K, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (size_t k = 0; k < K; k++)  // (a segment's room is its exact size: padding bits left read as TAMP_OUTPUT_FULL)
            if (got[k] != size[k] || (st8[k] != TAMP_INPUT_EXHAUSTED && st8[k] != TAMP_OUTPUT_FULL)) {
                if (dbg) fprintf(stderr, "[tamp_amd resets] segment %zu decoded to status %d, %u of %u bytes\n", k, (int)st8[k], got[k], size[k]);
                return TAMP_ERROR;
            }
    }
    if (dbg) fprintf(stderr, "[tamp_amd resets] %s: %zu segments, %llu bytes out\n", d_out ? "decoded" : "sized", K, (unsigned long long)total);
    *out_len = (uint32_t)total, *status = TAMP_INPUT_EXHAUSTED, *consumed = n;
    return TAMP_OK;
}

// The entry point behind its checks: the fast path, or -- declined -- the exact path of tamp_batch_decompress / _decoded_size for
// the one stream, under the same lock.  in / out: device memory; the three results: host memory.
int decompress_resets_device(DeviceCtx* ctx, const uint8_t* d_in, uint32_t n, uint8_t* d_out, uint32_t cap, uint8_t max_wbits,
                             hipStream_t st, uint32_t* out_len, int8_t* status, uint32_t* consumed) {
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    // (TAMP_ERROR: a staged segment did not decode to the size the size build gave it -- the two disagree, which is a defect of the
    // library and not a property of the stream; bytes have been written by then, so it is reported, not handed to the exact path)
    int rc = launch_decompress_resets(ctx, rec, d_in, n, d_out, cap, max_wbits, st, out_len, status, consumed);
    if (rc != 1) return rc;
    HIP_OK(rec.resets.need(256));
    uint8_t* const r = static_cast<uint8_t*>(rec.resets.p);
    const uint64_t zero = 0;
    HIP_OK(hipMemcpyAsync(r, &zero, 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(r + 8, &n, 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(r + 12, &cap, 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    BatchTables t;
    t.in = d_in, t.in_off = reinterpret_cast<const uint64_t*>(r), t.in_len = reinterpret_cast<const uint32_t*>(r + 8);
    t.out_cap = reinterpret_cast<const uint32_t*>(r + 12), t.out_len = reinterpret_cast<uint32_t*>(r + 16);
    t.in_consumed = reinterpret_cast<uint32_t*>(r + 20), t.status = reinterpret_cast<int8_t*>(r + 24), t.n = 1;
    if (d_out) {
        t.out = d_out, t.out_off = reinterpret_cast<const uint64_t*>(r);
        rc = launch_decompress_locked(ctx, rec, t, max_wbits, st);
    } else {
        rc = launch_decoded_size_locked(ctx, rec, t, max_wbits, st);
    }
    if (rc != TAMP_OK) return rc;
    HIP_OK(hipMemcpyAsync(out_len, r + 16, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(consumed, r + 20, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(status, r + 24, 1, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return TAMP_OK;
}

int decompress_resets(uint8_t max_wbits, const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, uint32_t* out_len, int8_t* status,
                      uint32_t* consumed, int mem, int device, void* stream) {
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE)
        return decompress_resets_device(ctx, in, n, out, cap, max_wbits, static_cast<hipStream_t>(stream), out_len, status, consumed);
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    HIP_OK(P.in[0].need((size_t)n + 64));
    if (out) HIP_OK(P.out[0].need((size_t)cap + 1));
    uint8_t* const d_in = static_cast<uint8_t*>(P.in[0].p);
    uint8_t* const d_out = out ? static_cast<uint8_t*>(P.out[0].p) : nullptr;
    if (n) HIP_OK(hipMemcpyAsync(d_in, in, n, hipMemcpyHostToDevice, st));
    if (const int rc = decompress_resets_device(ctx, d_in, n, d_out, cap, max_wbits, st, out_len, status, consumed)) return rc;
    if (out && *out_len) {
        HIP_OK(hipMemcpyAsync(out, d_out, *out_len, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    return TAMP_OK;
}

// Reading a batch back with the compressor's reset index (tamp_batch_decompress_resets; kernels and steps:
// tamp_reset_segments_kernel.hpp).  The index is checked on the device; the segments of the streams that hold up are staged as
// streams of their own in the stream's scratch and decoded as ONE batch by the existing launch path, each into its place in the
// caller's buffer with exactly its decoded size as room; every other stream is decoded as it lies, by a second launch over the
// caller's tables in which the split streams are empty (in_len 0): the stage and the caller's input are two allocations, so the
// two kinds of unit cannot share a launch, and rows that stay in place need no compaction and no scatter.  The walk's sizes stand
// alone -- there is no size build over the staged segments beside it; a unit that decodes to another size is TAMP_ERROR for its
// stream.  `t`, d_first, d_off: device memory; t.out null: the sizes only (nothing is staged).  `counted`: closed = reset_first[n]
// (0 for a table out of order) and the bound of the staged bytes when the caller has them from host tables, else null: the one
// 16-byte record a device-memory call reads back, once, and waits for.
struct BatchResetIndexCounted { uint64_t closed, staged_bound; };
int launch_decompress_batch_resets(DeviceCtx* ctx, const BatchTables& t, const uint64_t* d_first, const uint32_t* d_off, uint8_t max_wbits,
                                   const BatchResetIndexCounted* counted, hipStream_t st) {
    const uint64_t n = t.n;
    if (n == 0) return TAMP_OK;
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    const bool dbg = getenv("TAMP_AMD_RESETS_DEBUG") != nullptr;
    auto exact = [&](const BatchTables& rows) {
        return t.out ? launch_decompress_locked(ctx, rec, rows, max_wbits, st) : launch_decoded_size_locked(ctx, rec, rows, max_wbits, st);
    };
    auto all_whole = [&]() {
        if (dbg) fprintf(stderr, "[tamp_amd resets] batch decode: %llu streams, 0 split into 0 units, %llu whole\n", (unsigned long long)n, (unsigned long long)n);
        return exact(t);
    };
    BatchResetIndexCounted have = counted ? *counted : BatchResetIndexCounted{0, 0};
    if (!counted) {
        HIP_OK(rec.resets.need(256));
        const BatchResetBoundArgs bound = {d_first, t.in_len, n, static_cast<BatchResetRecord*>(rec.resets.p)};
        hipLaunchKernelGGL(tamp_batch_reset_bound_kernel, dim3(1), dim3(kResetScanTile), 0, st, bound);
        HIP_OK(hipMemcpyAsync(&have, rec.resets.p, sizeof have, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    const uint64_t C = have.closed, R = C + n;
    if (C == 0 || R > 0xFFFFFFFFull) return all_whole();  // (no entry anywhere, or more rows than a launch's tables count)
    if (!d_off) return TAMP_AMD_BAD_ARGUMENT;
    size_t budget = (size_t)8 << 30, free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, std::max((free_b + rec.resets.bytes) / 4, rec.resets.bytes));
    else (void)hipGetLastError();
    const size_t stage_bytes = (size_t)std::min<uint64_t>(have.staged_bound, budget);
    const size_t tab_bytes = (256 + 8 * (2 * (C + 1) + n + 3 * R) + 4 * (2 * n + 5 * R) + (2 * R + n) + 255) & ~(size_t)255;
    if (rec.resets.need(tab_bytes + stage_bytes + 64) != hipSuccess) {
        (void)hipGetLastError();
        return all_whole();
    }
    uint8_t* const base = static_cast<uint8_t*>(rec.resets.p);
    BatchResetRecord* const record = reinterpret_cast<BatchResetRecord*>(base);
    uint64_t* const size_scan = reinterpret_cast<uint64_t*>(base + 256);
    uint64_t* const fail_scan = size_scan + C + 1;
    uint64_t* const stage_base = fail_scan + C + 1;
    BatchResetUnits u;
    u.in_off = stage_base + n, u.out_off = u.in_off + R, u.src_off = u.out_off + R;
    uint32_t* const size = reinterpret_cast<uint32_t*>(u.src_off + R);
    uint32_t* const total = size + R;
    uint32_t* const whole_len = total + n;
    u.in_len = whole_len + n, u.out_cap = u.in_len + R, u.out_len = u.out_cap + R, u.owner = u.out_len + R;
    uint8_t* const failed = reinterpret_cast<uint8_t*>(u.owner + R);
    uint8_t* const split = failed + R;
    u.status = reinterpret_cast<int8_t*>(split + n);
    uint8_t* const stage = base + tab_bytes;
    const uint32_t wbits = max_wbits & 0x7F;
    const CallTiming call_timing(st);
    const BatchResetCheckArgs check = {t.in, t.in_off, t.in_len, d_first, d_off, n, C, wbits, size, failed};
    hipLaunchKernelGGL(tamp_batch_reset_check_kernel, dim3((uint32_t)((R + 63) / 64)), dim3(64), 0, st, check);
    const BatchResetSizesArgs sizes = {size, failed, C, size_scan, fail_scan};
    hipLaunchKernelGGL(tamp_batch_reset_sizes_kernel, dim3(1), dim3(kResetScanTile), 0, st, sizes);
    const BatchResetPlanArgs plan = {t.in, t.in_off, t.in_len, t.out_cap, d_first, n, C, wbits, size, failed, size_scan, fail_scan,
                                     stage_bytes, split, stage_base, total, whole_len, record};
    hipLaunchKernelGGL(tamp_batch_reset_plan_kernel, dim3(1), dim3(kResetScanTile), 0, st, plan);
    const uint32_t row_grid = (uint32_t)((R + 255) / 256);
    if (t.out) {
        const BatchResetUnitsArgs units = {t.in_off, t.in_len, t.out_off, d_first, d_off, n, C, size, size_scan, split, stage_base, u};
        hipLaunchKernelGGL(tamp_batch_reset_units_kernel, dim3(row_grid), dim3(256), 0, st, units);
        const BatchResetStageArgs sa = {t.in, t.in_off, u, stage, R};
        hipLaunchKernelGGL(tamp_batch_reset_stage_kernel, dim3((uint32_t)std::min<uint64_t>(R, (uint64_t)ctx->cu_count * 8)), dim3(256), 0, st, sa);
        HIP_OK(hipGetLastError());
        BatchTables ut;
        ut.in = stage, ut.in_off = u.in_off, ut.in_len = u.in_len, ut.out = t.out, ut.out_off = u.out_off, ut.out_cap = u.out_cap;
        ut.out_len = u.out_len, ut.status = u.status, ut.n = R;
        if (const int rc = launch_decompress_locked(ctx, rec, ut, max_wbits, st)) return rc;
    }
    BatchTables wt = t;  // the streams that stay whole, where they lie
    wt.in_len = whole_len;
    if (const int rc = exact(wt)) return rc;
    BatchResetDoneArgs done = {t.in_len, t.out_len, t.status, t.in_consumed, n, C, split, total, u, 0};
    hipLaunchKernelGGL(tamp_batch_reset_done_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, done);
    if (t.out) {
        done.units = 1;
        hipLaunchKernelGGL(tamp_batch_reset_done_kernel, dim3(row_grid), dim3(256), 0, st, done);
    }
    HIP_OK(hipGetLastError());
    if (dbg) {  // (the line waits for the plan's record; a call without the variable does not)
        BatchResetRecord r;
        HIP_OK(hipMemcpyAsync(&r, record, sizeof r, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        fprintf(stderr, "[tamp_amd resets] batch decode: %llu streams, %llu split into %llu units, %llu whole\n", (unsigned long long)n,
                (unsigned long long)r.split, (unsigned long long)r.units, (unsigned long long)(n - r.split));
    }
    return TAMP_OK;
}

// tamp_batch_decompress_resets behind its checks.  Host memory, on the host pipeline's kept buffers and first stream (one host-memory
// call per device at a time): the input's extent, the tables and the index go to the device in one piece each; the output slabs
// lie back to back there; the three result tables come back, then exactly the produced bytes of every stream.
int batch_decompress_resets(const BatchTables& t, const uint64_t* first, const uint32_t* off, uint8_t max_wbits, int mem, int device,
                            void* stream) {
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE) return launch_decompress_batch_resets(ctx, t, first, off, max_wbits, nullptr, static_cast<hipStream_t>(stream));
    const size_t n = t.n;
    if (n == 0) return TAMP_OK;
    BatchResetIndexCounted counted = {first[n], 0};
    for (size_t i = 0; i < n; i++) {
        if (!reset_first_in_order(first, i)) counted.closed = 0;
        if (const uint64_t E = reset_index_entries(first, n, i)) counted.staged_bound += (uint64_t)t.in_len[i] + kResetHeaderBytes * (E + 1);
    }
    const uint64_t C = counted.closed;
    if (C && !off) return TAMP_AMD_BAD_ARGUMENT;
    const HostExtent ext(t.in_off, t.in_len, n);
    std::vector<uint64_t> h_out_off(n, 0);
    const uint64_t room = t.out ? dense_slabs(t.out_cap, n, h_out_off.data()) : 0;
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    HIP_OK(P.in[0].need(ext.bytes() + 64));  // the kernels' vector loads may run past the last byte
    if (t.out) HIP_OK(P.out[0].need(room + 1));
    TableCarver m;
    const auto m_in_off = m.take<uint64_t>(n), m_out_off = m.take<uint64_t>(n);
    const auto m_in_len = m.take<uint32_t>(n), m_cap = m.take<uint32_t>(n), m_out_len = m.take<uint32_t>(n), m_consumed = m.take<uint32_t>(n);
    const auto m_first = m.take<uint64_t>(n + 1);
    const auto m_off = m.take<uint32_t>(C);
    const auto m_status = m.take<int8_t>(n);
    HIP_OK(P.meta[0].need(m.bytes()));
    void* const mp = P.meta[0].p;
    uint64_t* const d_first = m_first.in(mp);
    uint32_t* const d_off = m_off.in(mp);
    BatchTables d;
    d.in = static_cast<const uint8_t*>(P.in[0].p), d.in_off = m_in_off.in(mp), d.in_len = m_in_len.in(mp);
    d.out = t.out ? static_cast<uint8_t*>(P.out[0].p) : nullptr, d.out_off = t.out ? m_out_off.in(mp) : nullptr, d.out_cap = m_cap.in(mp);
    d.out_len = m_out_len.in(mp), d.in_consumed = m_consumed.in(mp), d.status = m_status.in(mp), d.n = n;
    if (ext.bytes()) HIP_OK(hipMemcpyAsync(P.in[0].p, t.in + ext.lo, ext.bytes(), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_in_off.in(mp), ext.off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_out_off.in(mp), h_out_off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_in_len.in(mp), t.in_len, n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_cap.in(mp), t.out_cap, n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_first, first, (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (C) HIP_OK(hipMemcpyAsync(d_off, off, C * 4, hipMemcpyHostToDevice, st));
    if (const int rc = launch_decompress_batch_resets(ctx, d, d_first, d_off, max_wbits, &counted, st)) return rc;
    HIP_OK(hipMemcpyAsync(t.out_len, d.out_len, n * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(t.status, d.status, n, hipMemcpyDeviceToHost, st));
    if (t.in_consumed) HIP_OK(hipMemcpyAsync(t.in_consumed, d.in_consumed, n * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (!t.out) return TAMP_OK;
    return copy_back_slabs(P, st, d.out, room, h_out_off.data(), t.out, t.out_off, t.out_len, n);
}

// Reading byte ranges of reset-segmented streams (tamp_batch_read_ranges; kernels and steps: tamp_read_ranges_kernel.hpp, the
// arithmetic: tamp_reset_segments.hpp).  The ranges are processed in SLICES, in range order, each of which fits the budget with its
// units' rows, stage and scratch (one region of the stream's `resets` buffer); the per-range tables of the whole call lie in `ranges`.
size_t read_ranges_budget(const StreamScratch& rec) {
    size_t budget = (size_t)8 << 30, free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, std::max((free_b + rec.resets.bytes) / 4, (size_t)1 << 20));
    else (void)hipGetLastError();
    if (const char* e = getenv("TAMP_AMD_RANGES_SCRATCH_MB")) { const long v = atol(e); if (v >= 1) budget = (size_t)v << 20; }
    return budget;
}
constexpr size_t kReadRangesHead = 256;  // the record, in front of the per-range tables
size_t read_ranges_bytes(uint64_t nr) { return kReadRangesHead + 24 * (nr + 1) + 2 * nr + 64; }
// (the table form: a skip per range behind them, ReadTable::skip)
size_t read_ranges_grid_bytes(uint64_t nr) { return ((read_ranges_bytes(nr) + 7) & ~(size_t)7) + 8 * nr; }
uint64_t* read_ranges_skip_at(uint8_t* base, uint64_t nr) { return reinterpret_cast<uint64_t*>(base + ((read_ranges_bytes(nr) + 7) & ~(size_t)7)); }
ReadRanges read_ranges_at(uint8_t* base, uint64_t nr) {
    ReadRanges r;
    r.unit_first = reinterpret_cast<uint64_t*>(base + kReadRangesHead), r.scratch_first = r.unit_first + nr + 1;
    r.stage_first = r.scratch_first + nr + 1;
    r.verdict = reinterpret_cast<int8_t*>(r.stage_first + nr + 1), r.failed = reinterpret_cast<uint8_t*>(r.verdict + nr);
    return r;
}
// The slices of a call from the scans of its ranges' costs and units (host copies, nr + 1 entries each): as many ranges as fit the
// budget, one at least (a range that alone outgrows the budget has no units and costs nothing: it was refused when it was counted).
struct ReadSliceSpan { uint64_t q0, q1; };
std::vector<ReadSliceSpan> read_ranges_slices(const uint64_t* cost_first, const uint64_t* unit_first, uint64_t nr, uint64_t budget) {
    std::vector<ReadSliceSpan> slices;
    for (uint64_t q0 = 0; q0 < nr;) {
        uint64_t q1 = q0 + 1;
        while (q1 < nr && cost_first[q1 + 1] - cost_first[q0] <= budget && unit_first[q1 + 1] - unit_first[q0] < 0xFFFFFFFFull) q1++;
        slices.push_back({q0, q1});
        q0 = q1;
    }
    return slices;
}
// The steps of a slice behind its staged units: the walk, the decode of the unit rows by the existing launch path, the gather.
// `c`: what the gather reads of the caller's tables (interval, range_begin, range_len).  `g`: the table form (its skips), or null.
int launch_read_tail(DeviceCtx* ctx, StreamScratch& rec, const ReadCaller& c, const ReadRanges& r, const ReadSlice& s, uint8_t max_wbits,
                     uint8_t* out, const uint64_t* out_off, uint32_t* out_len, int8_t* status, hipStream_t st, const ReadTable* g = nullptr) {
    if (s.U) {
        if (g) {
            const ReadWalkGridArgs walk = {s, r.failed};
            hipLaunchKernelGGL(tamp_read_walk_kernel<ReadWalkGridArgs>, dim3((uint32_t)((s.U + 63) / 64)), dim3(64), 0, st, walk);
        } else {
            const ReadWalkArgs walk = {s, r.failed, c.interval};
            hipLaunchKernelGGL(tamp_read_walk_kernel<ReadWalkArgs>, dim3((uint32_t)((s.U + 63) / 64)), dim3(64), 0, st, walk);
        }
        HIP_OK(hipGetLastError());
        const ReadUnits u = read_units_at(s.region, s.U);
        BatchTables ut;
        ut.in = s.region, ut.in_off = u.in_off, ut.in_len = u.in_len, ut.out = s.region, ut.out_off = u.out_off, ut.out_cap = u.out_cap;
        ut.out_len = u.out_len, ut.status = u.status, ut.n = s.U;
        if (const int rc = launch_decompress_locked(ctx, rec, ut, max_wbits, st)) return rc;
    }
    const dim3 gather_grid((uint32_t)std::min<uint64_t>(s.q1 - s.q0, (uint64_t)ctx->cu_count * 8));
    if (g) {
        const ReadGatherGridArgs gather = {c, r, s, out, out_off, out_len, status, *g};
        hipLaunchKernelGGL(tamp_read_gather_kernel<ReadGatherGridArgs>, gather_grid, dim3(256), 0, st, gather);
    } else {
        const ReadGatherArgs gather = {c, r, s, out, out_off, out_len, status};
        hipLaunchKernelGGL(tamp_read_gather_kernel<ReadGatherArgs>, gather_grid, dim3(256), 0, st, gather);
    }
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}
void read_ranges_debug(uint64_t ranges, uint64_t units, size_t slices, uint64_t staged) {
    fprintf(stderr, "[tamp_amd resets] read ranges: %llu ranges, %llu units, %zu slices, %llu bytes staged\n", (unsigned long long)ranges,
            (unsigned long long)units, slices, (unsigned long long)staged);
}

// Device memory: everything is counted, cut and staged on the device; the call waits once, for the 16-byte record that sizes the
// region -- and, only when the call does not fit ONE slice, for the three scans that say where to cut it.
// `rec`: the stream's scratch record, locked by the caller (launch_read_ranges; launch_write_ranges, whose touched segments are read
// as ranges of their own), who also holds the call's event pair.
// `segment_end`: the table form (tamp_batch_read_ranges_grid; c.interval is not read), or null.
int launch_read_ranges_locked(DeviceCtx* ctx, StreamScratch& rec, const ReadCaller& c, uint8_t max_wbits, uint8_t* out, const uint64_t* out_off,
                              uint32_t* out_len, int8_t* status, bool dbg, hipStream_t st, const uint64_t* segment_end = nullptr) {
    const uint64_t nr = c.n_ranges, budget = read_ranges_budget(rec);
    HIP_OK(rec.ranges.need(segment_end ? read_ranges_grid_bytes(nr) : read_ranges_bytes(nr)));
    uint8_t* const tabs = static_cast<uint8_t*>(rec.ranges.p);
    const ReadRanges r = read_ranges_at(tabs, nr);
    const ReadTable table = {segment_end, read_ranges_skip_at(tabs, nr)};
    const ReadTable* const g = segment_end ? &table : nullptr;
    if (g) {
        const ReadCountGridArgs count = {c, budget, r, reinterpret_cast<ReadRecord*>(tabs), table};
        hipLaunchKernelGGL(tamp_read_count_kernel<ReadCountGridArgs>, dim3(1), dim3(kResetScanTile), 0, st, count);
    } else {
        const ReadCountArgs count = {c, budget, r, reinterpret_cast<ReadRecord*>(tabs)};
        hipLaunchKernelGGL(tamp_read_count_kernel<ReadCountArgs>, dim3(1), dim3(kResetScanTile), 0, st, count);
    }
    HIP_OK(hipGetLastError());
    ReadRecord have = {0, 0};
    HIP_OK(hipMemcpyAsync(&have, tabs, sizeof have, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    std::vector<ReadSliceSpan> slices = {{0, nr}};
    std::vector<uint64_t> cost_first, unit_first;
    if (have.cost > budget || have.units >= 0xFFFFFFFFull) {
        std::vector<uint64_t> scans(3 * (nr + 1));  // (unit_first, scratch_first, stage_first lie one behind the other)
        HIP_OK(hipMemcpyAsync(scans.data(), r.unit_first, scans.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        cost_first.resize(nr + 1), unit_first.assign(scans.begin(), scans.begin() + nr + 1);
        for (uint64_t q = 0; q <= nr; q++) cost_first[q] = scans[nr + 1 + q] + scans[2 * (nr + 1) + q] + kReadUnitRow * scans[q];
        slices = read_ranges_slices(cost_first.data(), unit_first.data(), nr, budget);
    }
    // one region for every slice: the largest.  (A slice's cost counts kReadUnitRow bytes of rows per unit; what it stages and
    // decodes is the rest, and the paddings between the three parts come on top.)
    auto units_of = [&](const ReadSliceSpan& s) { return unit_first.empty() ? have.units : unit_first[s.q1] - unit_first[s.q0]; };
    auto payload_of = [&](const ReadSliceSpan& s) { return (cost_first.empty() ? have.cost : cost_first[s.q1] - cost_first[s.q0]) - kReadUnitRow * units_of(s); };
    size_t region_bytes = 256;
    for (const ReadSliceSpan& s : slices) region_bytes = std::max<size_t>(region_bytes, read_region_bytes(units_of(s), payload_of(s), 0) + 512);
    HIP_OK(rec.resets.need(region_bytes));
    for (const ReadSliceSpan& span : slices) {
        const ReadSlice s = {span.q0, span.q1, units_of(span), static_cast<uint8_t*>(rec.resets.p)};
        if (s.U) {
            if (g) {
                const ReadUnitsGridArgs units = {c, budget, r, s, table};
                hipLaunchKernelGGL(tamp_read_units_kernel<ReadUnitsGridArgs>, dim3((uint32_t)((s.U + 255) / 256)), dim3(256), 0, st, units);
            } else {
                const ReadUnitsArgs units = {c, budget, r, s};
                hipLaunchKernelGGL(tamp_read_units_kernel<ReadUnitsArgs>, dim3((uint32_t)((s.U + 255) / 256)), dim3(256), 0, st, units);
            }
            const ReadStageArgs stage = {c, s};
            hipLaunchKernelGGL(tamp_read_stage_kernel, dim3((uint32_t)std::min<uint64_t>(s.U, (uint64_t)ctx->cu_count * 8)), dim3(256), 0, st, stage);
            HIP_OK(hipGetLastError());
        }
        if (const int rc = launch_read_tail(ctx, rec, c, r, s, max_wbits, out, out_off, out_len, status, st, g)) return rc;
    }
    if (dbg) {  // (the line waits for the count's last entry; a call without the variable does not)
        uint64_t staged = 0;
        HIP_OK(hipMemcpyAsync(&staged, r.stage_first + nr, 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        read_ranges_debug(nr, have.units, slices.size(), staged);
    }
    return TAMP_OK;
}
int launch_read_ranges(DeviceCtx* ctx, const ReadCaller& c, uint8_t max_wbits, uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                       int8_t* status, hipStream_t st, const uint64_t* segment_end) {
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    const CallTiming call_timing(st);
    return launch_read_ranges_locked(ctx, rec, c, max_wbits, out, out_off, out_len, status, getenv("TAMP_AMD_RESETS_DEBUG") != nullptr, st, segment_end);
}

// Host memory, on the host pipeline's first stream (one host-memory call per device at a time): the host counts and cuts with the
// functions the kernels use and copies ONLY the touched segments, a header in front of each, into pinned staging; per slice the
// units' rows and that stage go up, the result tables and the packed ranges come back, and the delivered bytes are placed.
// `segment_end`: the table form (the caller's table, in host memory), or null.
int read_ranges_host(DeviceCtx* ctx, const ReadCaller& c, uint8_t max_wbits, uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                     int8_t* status, const uint64_t* segment_end) {
    const uint64_t nr = c.n_ranges;
    std::vector<ReadPlan> plan(nr);
    std::vector<ReadGridPlan> grid_plan(segment_end ? nr : 0);  // (the table form: plan[q] is grid_plan[q].p)
    std::vector<uint64_t> skip(segment_end ? nr : 0);
    std::vector<uint32_t> unit_size;  // (the table form: the units' table sizes of a slice)
    std::vector<uint64_t> unit_first(nr + 1), cost_first(nr + 1), packed_off(nr);
    std::vector<int8_t> verdict(nr);
    std::vector<uint8_t> failed(nr, 0);
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);
    const bool dbg = getenv("TAMP_AMD_RESETS_DEBUG") != nullptr;
    const uint64_t budget = read_ranges_budget(rec);
    // the count, on the host
    uint64_t units_all = 0, cost_all = 0, staged_all = 0;
    for (uint64_t q = 0; q < nr; q++) {
        if (segment_end) {
            grid_plan[q] = read_grid_plan(c.in, c.in_off, c.in_len, c.first, c.off, segment_end, c.n, c.max_wbits, budget, c.range_stream[q],
                                          c.range_begin[q], c.range_len[q]);
            plan[q] = grid_plan[q].p, skip[q] = grid_plan[q].skip;
        } else {
            plan[q] = read_range_plan(c.in, c.in_off, c.in_len, c.first, c.off, c.n, c.interval, c.max_wbits, budget, c.range_stream[q],
                                      c.range_begin[q], c.range_len[q]);
        }
        unit_first[q] = units_all, cost_first[q] = cost_all, verdict[q] = (int8_t)plan[q].verdict;
        units_all += plan[q].units, cost_all += plan[q].units ? read_plan_cost(plan[q]) : 0;
    }
    unit_first[nr] = units_all, cost_first[nr] = cost_all;
    const std::vector<ReadSliceSpan> slices = read_ranges_slices(cost_first.data(), unit_first.data(), nr, budget);
    // the per-range tables of the device steps: unit_first and the verdicts in `ranges` (the walk's `failed` follows per slice), what
    // the gather reads of the caller's tables and the results in the pipeline's meta buffer
    HIP_OK(rec.ranges.need(segment_end ? read_ranges_grid_bytes(nr) : read_ranges_bytes(nr)));
    const ReadRanges r = read_ranges_at(static_cast<uint8_t*>(rec.ranges.p), nr);
    const ReadTable table = {nullptr, read_ranges_skip_at(static_cast<uint8_t*>(rec.ranges.p), nr)};  // (the device steps read the skips alone)
    const ReadTable* const g = segment_end ? &table : nullptr;
    TableCarver m;
    const auto m_begin = m.take<uint64_t>(nr), m_out_off = m.take<uint64_t>(nr);
    const auto m_len = m.take<uint32_t>(nr), m_out_len = m.take<uint32_t>(nr);
    const auto m_status = m.take<int8_t>(nr);
    HIP_OK(P.meta[0].need(m.bytes()));
    void* const mp = P.meta[0].p;
    uint64_t *const d_begin = m_begin.in(mp), *const d_out_off = m_out_off.in(mp);
    uint32_t *const d_len = m_len.in(mp), *const d_out_len = m_out_len.in(mp);
    int8_t* const d_status = m_status.in(mp);
    ReadCaller d = {};
    d.interval = c.interval, d.max_wbits = c.max_wbits, d.range_begin = d_begin, d.range_len = d_len, d.n_ranges = nr;
    const CallTiming call_timing(st);
    HIP_OK(hipMemcpyAsync(r.unit_first, unit_first.data(), (nr + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(r.verdict, verdict.data(), nr, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_begin, c.range_begin, nr * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_len, c.range_len, nr * 4, hipMemcpyHostToDevice, st));
    if (g && nr) HIP_OK(hipMemcpyAsync(table.skip, skip.data(), nr * 8, hipMemcpyHostToDevice, st));
    for (const ReadSliceSpan& span : slices) {
        const uint64_t U = unit_first[span.q1] - unit_first[span.q0];
        uint64_t staged = 0, scratch = 0, packed = 0;
        for (uint64_t q = span.q0; q < span.q1; q++) {
            // (a range delivers no more than its units are given room for)
            packed_off[q] = packed, packed += std::min<uint64_t>(c.range_len[q], plan[q].scratch);
            staged += plan[q].staged, scratch += plan[q].scratch;
        }
        HIP_OK(rec.resets.need(read_region_bytes(U, staged, scratch)));
        const ReadSlice s = {span.q0, span.q1, U, static_cast<uint8_t*>(rec.resets.p)};
        const uint64_t rows_bytes = read_units_upload_bytes(U);
        if (U) {
            HIP_OK(P.stage[0].need(rows_bytes + staged));
            uint8_t* const h = static_cast<uint8_t*>(P.stage[0].p);
            uint8_t* const h_stage = h + rows_bytes;
            const ReadUnits u = read_units_at(h, U);  // (the uploaded rows alone)
            if (g) unit_size.assign(U, 0);
            uint64_t x = 0, stage_at = 0, scratch_at = 0;
            for (uint64_t q = span.q0; q < span.q1; q++) {
                const uint64_t i = c.range_stream[q];
                for (uint64_t j = 0; j < plan[q].units; j++, x++) {
                    ReadUnit w;
                    if (g) {
                        const ReadGridUnit gw = read_grid_unit(c.first, c.off, c.in_len, segment_end, i, grid_plan[q], j);
                        w = gw.u, unit_size[x] = gw.size;
                    } else {
                        w = read_range_unit(c.first, c.off, c.in_len, c.interval, i, plan[q], j);
                    }
                    u.in_off[x] = read_stage_at(U) + stage_at + w.place, u.out_off[x] = read_scratch_at(U, staged) + scratch_at + w.room;
                    u.in_len[x] = w.in_len, u.need[x] = w.need, u.owner[x] = (uint32_t)(q - span.q0);
                    u.flags[x] = (uint8_t)((w.cut.closed ? kReadUnitClosed : 0) | (plan[q].k0 + j ? kReadUnitBehindReset : 0));
                    u.verdict[x] = w.cut.ok ? kReadWalkOk : kReadWalkBad;
                    if (!w.cut.ok) { failed[q] = 1; continue; }
                    uint8_t* const dst = h_stage + stage_at + w.place;
                    dst[0] = c.in[c.in_off[i]], dst[1] = 0;  // (the stream's own two header bytes: the second one is zero)
                    memcpy(dst + kResetHeaderBytes, c.in + c.in_off[i] + w.cut.start, w.cut.end - w.cut.start);
                    staged_all += w.in_len;
                }
                stage_at += plan[q].staged, scratch_at += plan[q].scratch;
            }
            HIP_OK(hipMemcpyAsync(s.region, h, rows_bytes, hipMemcpyHostToDevice, st));
            if (staged) HIP_OK(hipMemcpyAsync(s.region + read_stage_at(U), h_stage, staged, hipMemcpyHostToDevice, st));
            // (the table form: what the walk holds each unit to, into the row the units kernel of a device-memory call fills;
            // pageable memory: the copy has left `unit_size` when the call returns)
            if (g) HIP_OK(hipMemcpyAsync(read_units_at(s.region, U).size, unit_size.data(), U * 4, hipMemcpyHostToDevice, st));
        }
        const uint64_t nq = span.q1 - span.q0;
        HIP_OK(hipMemcpyAsync(r.failed + span.q0, failed.data() + span.q0, nq, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_out_off + span.q0, packed_off.data() + span.q0, nq * 8, hipMemcpyHostToDevice, st));
        HIP_OK(P.out[0].need(packed + 1));
        uint8_t* const d_out = static_cast<uint8_t*>(P.out[0].p);
        if (const int rc = launch_read_tail(ctx, rec, d, r, s, max_wbits, d_out, d_out_off, d_out_len, d_status, st, g)) return rc;
        HIP_OK(hipMemcpyAsync(out_len + span.q0, d_out_len + span.q0, nq * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(status + span.q0, d_status + span.q0, nq, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        uint64_t extent = 0;  // of the packed ranges: behind the last delivered byte
        for (uint64_t q = span.q0; q < span.q1; q++)
            if (out_len[q]) extent = std::max(extent, packed_off[q] + out_len[q]);
        if (!extent) continue;
        HIP_OK(P.stage[1].need(extent));
        HIP_OK(hipMemcpyAsync(P.stage[1].p, d_out, extent, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        const uint8_t* const back = static_cast<const uint8_t*>(P.stage[1].p);
        for (uint64_t q = span.q0; q < span.q1; q++)
            if (out_len[q]) memcpy(out + out_off[q], back + packed_off[q], out_len[q]);
    }
    if (dbg) read_ranges_debug(nr, units_all, slices.size(), staged_all);
    return TAMP_OK;
}

int batch_read_ranges(const ReadCaller& c, uint8_t max_wbits, uint8_t* out, const uint64_t* out_off, uint32_t* out_len, int8_t* status,
                      int mem, int device, void* stream, const uint64_t* segment_end = nullptr) {
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE)
        return launch_read_ranges(ctx, c, max_wbits, out, out_off, out_len, status, static_cast<hipStream_t>(stream), segment_end);
    if (!c.off && c.n && c.first[c.n] != 0) return TAMP_AMD_BAD_ARGUMENT;  // (entries and no table to hold them)
    return read_ranges_host(ctx, c, max_wbits, out, out_off, out_len, status, segment_end);
}

// The table of segment ends (tamp_batch_segment_ends; kernels: tamp_segment_ends_kernel.hpp).  Device memory: two launches on the
// call's stream, nothing read back, the stream never waited for -- the row count is read on the device, the grid comes from the CU
// count.  Host memory: the same running sum, with the same functions, on the host; no device is looked for.
int launch_segment_ends(DeviceCtx* ctx, const uint64_t* first, const uint32_t* closed_size, const uint32_t* open_size, uint64_t* segment_end,
                        uint64_t n, hipStream_t st) {
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    HIP_OK(rec.ends.need(kSegmentEndsMaxGrid * sizeof(SegmentEndSum), false));
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx->cu_count * 4, kSegmentEndsMaxGrid));
    const SegmentEndsArgs a = {first, closed_size, open_size, n, static_cast<SegmentEndSum*>(rec.ends.p), segment_end};
    if (grid > 1) hipLaunchKernelGGL(tamp_segment_ends_sums_kernel, dim3(grid), dim3(kResetScanTile), 0, st, a);
    hipLaunchKernelGGL(tamp_segment_ends_apply_kernel, dim3(grid), dim3(kResetScanTile), 0, st, a);
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// Writing byte ranges into reset-segmented streams (tamp_batch_write_ranges; kernels and steps: tamp_write_ranges_kernel.hpp, the
// arithmetic: tamp_write_ranges.hpp).  The per-stream and per-segment tables of the whole call lie in `writes`; the units run in
// SLICES of whole streams, each of which fits the budget with its rows, staging rows and slabs (`write_units`).  The decode of a
// slice's units is launch_read_ranges_locked over one range per unit (its own tables: `ranges`, `resets`).
struct WriteOut {
    uint8_t* out;
    const uint64_t* out_off;
    const uint32_t* out_cap;
    uint32_t* out_len;
    int8_t* status;
    uint32_t* new_reset_off;  // may be null
};
struct WriteSliceSpan { uint64_t i0, i1, u0, U, o0, Uo; bool run; };
// All pointers: device memory.  `segments`: reset_first[n] + n when the caller has it from host tables, else null: the call then
// waits for the table's last entry.  It waits for the 16-byte record of the units; a call that does not fit one slice reads two
// tables more to cut it.
int launch_write_ranges(DeviceCtx* ctx, const TampAmdConf* conf, const WriteCaller& c, uint8_t max_wbits, const WriteOut& o,
                        const uint64_t* segments, hipStream_t st) {
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    const bool dbg = getenv("TAMP_AMD_RESETS_DEBUG") != nullptr;
    const uint64_t n = c.n, nw = c.n_writes;
    uint64_t S = 0;
    if (segments) S = *segments;
    else {
        uint64_t entries = 0;
        HIP_OK(hipMemcpyAsync(&entries, c.first + n, 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (entries + n < entries) return TAMP_AMD_BAD_ARGUMENT;
        S = entries + n;
    }
    // the tables: 8-byte ones, 4-byte ones, bytes
    const size_t at_fail = 256, at_fail0 = at_fail + 8 * n, at_ufirst = at_fail0 + 8 * n, at_ofirst = at_ufirst + 8 * (n + 1);
    const size_t at_unit = at_ofirst + 8 * (n + 1), at_open = at_unit + 4 * (S + 1), at_pos = at_open + 4 * (S + 1), at_len = at_pos + 4 * S;
    const size_t at_owner = at_len + 4 * S, at_flags = at_owner + 4 * S, at_whole = at_flags + S, all_bytes = at_whole + n + 64;
    HIP_OK(rec.writes.need(all_bytes));
    uint8_t* const base = static_cast<uint8_t*>(rec.writes.p);
    WriteTables t;
    t.S = S;
    t.fail = reinterpret_cast<uint64_t*>(base + at_fail), t.fail0 = reinterpret_cast<uint64_t*>(base + at_fail0);
    t.unit_first = reinterpret_cast<uint64_t*>(base + at_ufirst), t.open_first = reinterpret_cast<uint64_t*>(base + at_ofirst);
    t.unit_at = reinterpret_cast<uint32_t*>(base + at_unit), t.open_at = reinterpret_cast<uint32_t*>(base + at_open);
    t.new_pos = reinterpret_cast<uint32_t*>(base + at_pos), t.new_len = reinterpret_cast<uint32_t*>(base + at_len);
    t.owner = reinterpret_cast<uint32_t*>(base + at_owner), t.flags = base + at_flags, t.whole = base + at_whole;
    const uint32_t N = c.interval, row = write_row_bytes(N), slab = (uint32_t)reset_segment_bound(N, conf->literal, true);
    const uint64_t budget = read_ranges_budget(rec), max_units = std::max<uint64_t>(budget / write_unit_cost(N, slab), 1);
    const CallTiming call_timing(st);
    HIP_OK(hipMemsetAsync(t.fail, 0xFF, 8 * n, st));
    HIP_OK(hipMemsetAsync(t.owner, 0xFF, 4 * S, st));  // (none)
    HIP_OK(hipMemsetAsync(t.flags, 0, S + n, st));             // (flags and whole, one behind the other)
    if (nw) {
        const WritePlanArgs plan = {c, t};
        hipLaunchKernelGGL(tamp_write_plan_kernel, dim3((uint32_t)((nw + 255) / 256)), dim3(256), 0, st, plan);
    }
    const WriteScanArgs scan = {t, reinterpret_cast<WriteRecord*>(base)};
    hipLaunchKernelGGL(tamp_write_scan_kernel, dim3(1), dim3(kResetScanTile), 0, st, scan);
    const WriteStreamsArgs streams = {c, t, max_units};
    hipLaunchKernelGGL(tamp_write_streams_kernel, dim3((uint32_t)((n + 1 + 255) / 256)), dim3(256), 0, st, streams);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(t.fail0, t.fail, 8 * n, hipMemcpyDeviceToDevice, st));
    WriteRecord have = {0, 0};
    HIP_OK(hipMemcpyAsync(&have, base, sizeof have, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (have.units >= 0xFFFFFFFFull) {
        snprintf(t_last_error, sizeof t_last_error, "write ranges: %llu touched segments", (unsigned long long)have.units);
        return TAMP_AMD_BAD_ARGUMENT;
    }
    std::vector<WriteSliceSpan> slices = {{0, n, 0, have.units, 0, have.open_units, true}};
    if (have.units > max_units) {
        std::vector<uint64_t> firsts(2 * (n + 1));  // (unit_first and open_first lie one behind the other)
        HIP_OK(hipMemcpyAsync(firsts.data(), t.unit_first, firsts.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        uint64_t* const uf = firsts.data();
        uint64_t* const of = uf + n + 1;
        for (uint64_t i = 1; i <= n; i++) uf[i] = std::max(uf[i], uf[i - 1]), of[i] = std::max(of[i], of[i - 1]);  // (any table: in order)
        slices.clear();
        for (uint64_t i0 = 0; i0 < n;) {  // as many whole streams as fit, one at least (its units do not run when it alone is too many)
            uint64_t i1 = i0 + 1;
            while (i1 < n && uf[i1 + 1] - uf[i0] <= max_units) i1++;
            const uint64_t U = uf[i1] - uf[i0];
            slices.push_back({i0, i1, uf[i0], U, of[i0], std::min(of[i1] - of[i0], U), U <= max_units});
            i0 = i1;
        }
    }
    uint64_t most = 0;
    for (const WriteSliceSpan& s : slices) most = std::max(most, s.run ? s.U : 0);
    HIP_OK(rec.write_units.need(write_region_bytes(most, row, slab) + 256));
    uint8_t* const region = static_cast<uint8_t*>(rec.write_units.p);
    const SegmentSpec with_token = {2, (uint16_t)(0xABu << 7), kSegFlushToken}, without = {2, (uint16_t)(0xABu << 7), 0};
    const uint32_t wide = (uint32_t)ctx->cu_count * 8;
    uint64_t staged = 0;
    for (const WriteSliceSpan& span : slices) {
        const uint64_t U = span.run ? span.U : 0, Uo = span.run ? span.Uo : 0;
        const WriteSlice s = {span.i0, span.i1, span.u0, U, span.o0, Uo, region, row, slab};
        if (U) {
            const WriteRows w = write_rows_at(region, U);
            HIP_OK(hipMemsetAsync(region, 0, write_rows_bytes(U), st));
            const WriteRowsArgs rows = {c, t, s};
            hipLaunchKernelGGL(tamp_write_rows_kernel, dim3((uint32_t)((U + 255) / 256)), dim3(256), 0, st, rows);
            HIP_OK(hipGetLastError());
            const ReadCaller rc = {c.in, c.in_off, c.in_len, c.first, c.off, n, N, c.max_wbits, w.stream, w.begin, w.len, U};
            if (const int r = launch_read_ranges_locked(ctx, rec, rc, max_wbits, region, w.row_off, w.size, w.read_status, false, st)) return r;
            if (nw) {
                const WritePatchArgs patch = {c, t, s};
                hipLaunchKernelGGL(tamp_write_patch_kernel, dim3((uint32_t)std::min<uint64_t>(nw, wide)), dim3(256), 0, st, patch);
                HIP_OK(hipGetLastError());
            }
            BatchTables seg;
            seg.in = region, seg.in_off = w.row_off, seg.in_len = w.size, seg.out = region, seg.out_off = w.slab_off, seg.out_cap = w.cap;
            seg.out_len = w.out_len, seg.status = w.status, seg.n = U;
            if (const int r = launch_compress_locked(ctx, rec, conf, seg.rows(0, U - Uo), N, st, &with_token, nullptr)) return r;
            if (const int r = launch_compress_locked(ctx, rec, conf, seg.rows(U - Uo, Uo), N, st, &without, nullptr)) return r;
            if (dbg) {
                std::vector<uint32_t> sizes(U);
                HIP_OK(hipMemcpyAsync(sizes.data(), w.size, 4 * U, hipMemcpyDeviceToHost, st));
                HIP_OK(hipStreamSynchronize(st));
                for (const uint32_t v : sizes) staged += v;
            }
        }
        const WriteSpliceArgs splice = {c, t, s, o.out_cap, o.out_len, o.status, o.new_reset_off};
        hipLaunchKernelGGL(tamp_write_splice_kernel, dim3((uint32_t)std::min<uint64_t>(span.i1 - span.i0, wide)), dim3(kResetScanTile), 0, st, splice);
        const WriteGatherArgs gather = {c, t, s, o.out, o.out_off, o.out_cap, o.status};
        hipLaunchKernelGGL(tamp_write_gather_kernel, dim3((uint32_t)std::min<uint64_t>(S + (span.i1 - span.i0), wide)), dim3(256), 0, st, gather);
        HIP_OK(hipGetLastError());
    }
    if (dbg)
        fprintf(stderr, "[tamp_amd resets] write ranges: %llu writes, %llu units, %zu slices, %llu bytes staged\n", (unsigned long long)nw,
                (unsigned long long)have.units, slices.size(), (unsigned long long)staged);
    return TAMP_OK;
}

// tamp_batch_write_ranges behind its checks.  Host memory, on the host pipeline's kept buffers and first stream (one host-memory
// call per device at a time): the extents of the streams and of the sources and every table go up; the output slabs lie back to back
// on the device, each as long as its stream can get or as the caller allows, whichever is less; the result tables come back, then
// exactly the produced bytes of every stream.
int batch_write_ranges(const TampAmdConf* conf, const WriteCaller& c, uint8_t max_wbits, const WriteOut& o, int mem, int device, void* stream) {
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE) return launch_write_ranges(ctx, conf, c, max_wbits, o, nullptr, static_cast<hipStream_t>(stream));
    const uint64_t n = c.n, nw = c.n_writes, C = c.first[n];
    if (!c.off && C) return TAMP_AMD_BAD_ARGUMENT;  // (entries and no table to hold them)
    if (C + n < C) return TAMP_AMD_BAD_ARGUMENT;
    const uint64_t unit_bound = reset_segment_bound(c.interval, conf->literal, true);
    std::vector<uint64_t> h_out_off(n), grow(n, 0);
    std::vector<uint32_t> h_cap(n);
    const auto lands = [&](size_t q) { return c.write_stream[q] < n; };  // (a write to a stream there is: the others name no source bytes)
    for (uint64_t q = 0; q < nw; q++)  // (what a stream's touched segments can take at most)
        if (lands(q) && c.write_len[q]) grow[c.write_stream[q]] += ((uint64_t)c.write_len[q] / c.interval + 2) * unit_bound;
    for (uint64_t i = 0; i < n; i++)  // the new stream: its untouched bytes, no more than it has, and its touched segments again
        h_cap[i] = (uint32_t)std::min<uint64_t>(o.out_cap[i], std::min<uint64_t>((uint64_t)c.in_len[i] + kResetHeaderBytes + grow[i], 0xFFFFFFFFull));
    const HostExtent ext(c.in_off, c.in_len, n), src(c.src_off, c.write_len, nw, lands);
    const uint64_t room = dense_slabs(h_cap.data(), n, h_out_off.data());
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    HIP_OK(P.in[0].need(ext.bytes() + 64));
    HIP_OK(P.in[1].need(src.bytes() + 64));
    HIP_OK(P.out[0].need(room + 1));
    TableCarver m;
    const auto m_in_off = m.take<uint64_t>(n), m_out_off = m.take<uint64_t>(n), m_first = m.take<uint64_t>(n + 1);
    const auto m_begin = m.take<uint64_t>(nw), m_src_off = m.take<uint64_t>(nw);
    const auto m_in_len = m.take<uint32_t>(n), m_cap = m.take<uint32_t>(n), m_out_len = m.take<uint32_t>(n);
    const auto m_off = m.take<uint32_t>(C), m_new_off = m.take<uint32_t>(C), m_wstream = m.take<uint32_t>(nw), m_wlen = m.take<uint32_t>(nw);
    const auto m_status = m.take<int8_t>(n);
    HIP_OK(P.meta[0].need(m.bytes()));
    void* const mp = P.meta[0].p;
    uint64_t *const d_in_off = m_in_off.in(mp), *const d_out_off = m_out_off.in(mp), *const d_first = m_first.in(mp);
    uint64_t *const d_begin = m_begin.in(mp), *const d_src_off = m_src_off.in(mp);
    uint32_t *const d_in_len = m_in_len.in(mp), *const d_cap = m_cap.in(mp), *const d_out_len = m_out_len.in(mp);
    uint32_t *const d_off = m_off.in(mp), *const d_new_off = m_new_off.in(mp), *const d_wstream = m_wstream.in(mp), *const d_wlen = m_wlen.in(mp);
    int8_t* const d_status = m_status.in(mp);
    if (ext.bytes()) HIP_OK(hipMemcpyAsync(P.in[0].p, c.in + ext.lo, ext.bytes(), hipMemcpyHostToDevice, st));
    if (src.bytes()) HIP_OK(hipMemcpyAsync(P.in[1].p, c.src + src.lo, src.bytes(), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_in_off, ext.off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_out_off, h_out_off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_first, c.first, (n + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_in_len, c.in_len, n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_cap, h_cap.data(), n * 4, hipMemcpyHostToDevice, st));
    if (C) HIP_OK(hipMemcpyAsync(d_off, c.off, C * 4, hipMemcpyHostToDevice, st));
    if (nw) {
        HIP_OK(hipMemcpyAsync(d_begin, c.write_begin, nw * 8, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_src_off, src.off.data(), nw * 8, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_wstream, c.write_stream, nw * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_wlen, c.write_len, nw * 4, hipMemcpyHostToDevice, st));
    }
    WriteCaller d = c;
    d.in = static_cast<const uint8_t*>(P.in[0].p), d.in_off = d_in_off, d.in_len = d_in_len, d.first = d_first, d.off = C ? d_off : nullptr;
    d.write_stream = d_wstream, d.write_begin = d_begin, d.write_len = d_wlen, d.src = static_cast<const uint8_t*>(P.in[1].p), d.src_off = d_src_off;
    uint8_t* const d_out = static_cast<uint8_t*>(P.out[0].p);
    const WriteOut dout = {d_out, d_out_off, d_cap, d_out_len, d_status, o.new_reset_off ? d_new_off : nullptr};
    const uint64_t S = C + n;
    if (const int rc = launch_write_ranges(ctx, conf, d, max_wbits, dout, &S, st)) return rc;
    HIP_OK(hipMemcpyAsync(o.out_len, d_out_len, n * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(o.status, d_status, n, hipMemcpyDeviceToHost, st));
    if (o.new_reset_off && C) HIP_OK(hipMemcpyAsync(o.new_reset_off, d_new_off, C * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return copy_back_slabs(P, st, d_out, room, h_out_off.data(), o.out, o.out_off, o.out_len, n);
}

// Appending to reset-segmented streams (tamp_batch_append; kernels and steps: tamp_append_kernel.hpp, the arithmetic:
// tamp_append.hpp).  The per-stream tables of the whole call lie in `appends`; `append_units` holds the staged entries of the new
// index and, behind them, the region of a slice: the units run in SLICES of whole streams, each of which fits the budget with its
// rows, staging rows and slabs.  The decode of a slice's open segments is launch_read_ranges_locked over one range per appending
// stream (its own tables: `ranges`, `resets`).
struct AppendOut {
    uint8_t* out;
    const uint64_t* out_off;
    const uint32_t* out_cap;
    uint32_t* out_len;
    int8_t* status;
    uint64_t* new_first;
    uint32_t* new_off;  // may be null when new_cap is 0
    uint64_t new_cap;
};
struct AppendSliceSpan { uint64_t i0, i1, c0, C, a0, A; };
// All pointers: device memory.  The call waits for its 40-byte record (rows, entries, the bound that new_reset_off must hold) and,
// where an open segment is decoded, once per slice inside the shared read path; a call that does not fit one slice reads two tables
// more to cut it.  `cap_checked`: the caller has held new_cap against the bound already (host tables).
int launch_append(DeviceCtx* ctx, const TampAmdConf* conf, const AppendCaller& c, uint8_t max_wbits, const AppendOut& o, bool cap_checked,
                  hipStream_t st) {
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    const bool dbg = getenv("TAMP_AMD_RESETS_DEBUG") != nullptr;
    const uint64_t n = c.n;
    // the tables: 8-byte ones, bytes
    const size_t at_fail = 256, at_closed = at_fail + 8 * n, at_app = at_closed + 8 * (n + 1), at_count = at_app + 8 * (n + 1);
    const size_t at_need = at_count + 8 * n, at_whole = at_need + n, at_hold = at_whole + n, all_bytes = at_hold + n + 64;
    HIP_OK(rec.appends.need(all_bytes));
    uint8_t* const base = static_cast<uint8_t*>(rec.appends.p);
    AppendTables t;
    t.fail = reinterpret_cast<uint64_t*>(base + at_fail), t.closed_first = reinterpret_cast<uint64_t*>(base + at_closed);
    t.app_first = reinterpret_cast<uint64_t*>(base + at_app), t.count = reinterpret_cast<uint64_t*>(base + at_count);
    t.need = base + at_need, t.whole = base + at_whole, t.hold = base + at_hold, t.entries = nullptr, t.entries_cap = 0;
    const uint32_t N = c.interval, row = write_row_bytes(N), slab = (uint32_t)reset_segment_bound(N, conf->literal, true);
    const uint64_t budget = read_ranges_budget(rec), max_units = std::max<uint64_t>(budget / append_unit_cost(N, slab), 1);
    const CallTiming call_timing(st);
    const AppendOrderArgs order = {c, t};
    hipLaunchKernelGGL(tamp_append_order_kernel, dim3(1), dim3(kResetScanTile), 0, st, order);
    const AppendPlanArgs plan = {c, t, max_units};
    hipLaunchKernelGGL(tamp_append_plan_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, plan);
    const AppendScanArgs scan = {c, t, reinterpret_cast<AppendRecord*>(base)};
    hipLaunchKernelGGL(tamp_append_scan_kernel, dim3(1), dim3(kResetScanTile), 0, st, scan);
    HIP_OK(hipGetLastError());
    AppendRecord have = {0, 0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(&have, base, sizeof have, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (!cap_checked && (have.entries + have.bound < have.entries || have.entries + have.bound > o.new_cap)) {
        snprintf(t_last_error, sizeof t_last_error, "append: new_reset_cap %llu, %llu entries may be needed", (unsigned long long)o.new_cap,
                 (unsigned long long)(have.entries + have.bound));
        return TAMP_AMD_BAD_ARGUMENT;
    }
    const uint64_t rows_all = have.closed + have.appends;
    if (rows_all >= 0xFFFFFFFFull || have.entries + have.closed < have.entries) {
        snprintf(t_last_error, sizeof t_last_error, "append: %llu rows, %llu entries", (unsigned long long)rows_all, (unsigned long long)have.entries);
        return TAMP_AMD_BAD_ARGUMENT;
    }
    t.entries_cap = have.entries + have.closed;
    std::vector<AppendSliceSpan> slices = {{0, n, 0, have.closed, 0, have.appends}};
    if (rows_all > max_units) {
        std::vector<uint64_t> firsts(2 * (n + 1));  // (closed_first and app_first lie one behind the other)
        HIP_OK(hipMemcpyAsync(firsts.data(), t.closed_first, firsts.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        const uint64_t* const cf = firsts.data();
        const uint64_t* const af = cf + n + 1;
        slices.clear();
        for (uint64_t i0 = 0; i0 < n;) {  // as many whole streams as fit, one at least (a stream that alone is too many has no rows)
            uint64_t i1 = i0 + 1;
            while (i1 < n && (cf[i1 + 1] - cf[i0]) + (af[i1 + 1] - af[i0]) <= max_units) i1++;
            slices.push_back({i0, i1, cf[i0], cf[i1] - cf[i0], af[i0], af[i1] - af[i0]});
            i0 = i1;
        }
    }
    size_t region_bytes = 256;
    for (const AppendSliceSpan& s : slices) region_bytes = std::max<size_t>(region_bytes, append_region_bytes(s.C + s.A, s.A, row, slab));
    const size_t entries_bytes = (4 * t.entries_cap + 255) & ~(size_t)255;
    HIP_OK(rec.append_units.need(entries_bytes + region_bytes + 256));
    t.entries = static_cast<uint32_t*>(rec.append_units.p);
    uint8_t* const region = static_cast<uint8_t*>(rec.append_units.p) + entries_bytes;
    const SegmentSpec with_token = {2, (uint16_t)(0xABu << 7), kSegFlushToken}, without = {2, (uint16_t)(0xABu << 7), 0};
    const uint32_t wide = (uint32_t)ctx->cu_count * 8;
    uint64_t staged = 0;
    for (const AppendSliceSpan& span : slices) {
        const uint64_t U = span.C + span.A;
        const AppendSlice s = {span.i0, span.i1, span.c0, span.C, span.a0, span.A, region, row, slab};
        if (U) {
            const AppendRows w = append_rows_at(region, U, span.A);
            HIP_OK(hipMemsetAsync(region, 0, append_rows_bytes(U, span.A), st));
            const AppendRowsArgs rows = {c, t, s};
            hipLaunchKernelGGL(tamp_append_rows_kernel, dim3((uint32_t)((U + 255) / 256)), dim3(256), 0, st, rows);
            HIP_OK(hipGetLastError());
            if (have.decodes) {
                const ReadCaller rc = {c.in, c.in_off, c.in_len, c.first, c.off, n, N, c.max_wbits, w.range_stream, w.range_begin, w.range_len, span.A};
                if (const int r = launch_read_ranges_locked(ctx, rec, rc, max_wbits, region, w.range_out, w.m, w.read_status, false, st)) return r;
            }
            const AppendAssembleArgs assemble = {c, t, s};
            hipLaunchKernelGGL(tamp_append_assemble_kernel, dim3((uint32_t)std::min<uint64_t>(U, wide)), dim3(256), 0, st, assemble);
            HIP_OK(hipGetLastError());
            BatchTables seg;
            seg.in = region, seg.in_off = w.row_off, seg.in_len = w.in_len, seg.out = region, seg.out_off = w.slab_off, seg.out_cap = w.cap;
            seg.out_len = w.out_len, seg.status = w.status, seg.n = U;
            if (const int r = launch_compress_locked(ctx, rec, conf, seg.rows(0, span.C), N, st, &with_token, nullptr)) return r;
            if (const int r = launch_compress_locked(ctx, rec, conf, seg.rows(span.C, span.A), N, st, &without, nullptr)) return r;
            if (dbg) {
                std::vector<uint32_t> sizes(U);
                HIP_OK(hipMemcpyAsync(sizes.data(), w.in_len, 4 * U, hipMemcpyDeviceToHost, st));
                HIP_OK(hipStreamSynchronize(st));
                for (const uint32_t v : sizes) staged += v;
            }
        }
        const AppendSpliceArgs splice = {c, t, s, o.out_cap, o.out_len, o.status};
        hipLaunchKernelGGL(tamp_append_splice_kernel, dim3((uint32_t)std::min<uint64_t>(span.i1 - span.i0, wide)), dim3(kResetScanTile), 0, st, splice);
        const AppendGatherArgs gather = {c, t, s, o.out, o.out_off, o.out_cap, o.status, o.out_len};
        hipLaunchKernelGGL(tamp_append_gather_kernel, dim3((uint32_t)std::min<uint64_t>(U + (span.i1 - span.i0), wide)), dim3(256), 0, st, gather);
        HIP_OK(hipGetLastError());
    }
    const AppendIndexArgs index = {t, n, o.new_first};
    hipLaunchKernelGGL(tamp_append_index_kernel, dim3(1), dim3(kResetScanTile), 0, st, index);
    if (o.new_off && o.new_cap) {
        const AppendEntriesArgs entries = {c, t, o.new_first, o.new_off, o.new_cap};
        hipLaunchKernelGGL(tamp_append_entries_kernel, dim3((uint32_t)std::min<uint64_t>(n, wide)), dim3(256), 0, st, entries);
    }
    HIP_OK(hipGetLastError());
    if (dbg)
        fprintf(stderr, "[tamp_amd resets] append: %llu appends, %llu units, %zu slices, %llu bytes staged\n", (unsigned long long)have.appends,
                (unsigned long long)rows_all, slices.size(), (unsigned long long)staged);
    return TAMP_OK;
}

// tamp_batch_append behind its checks.  Host memory, on the host pipeline's kept buffers and first stream (one host-memory call per
// device at a time): the host makes the checks of the header, of reset_first and of the entries itself and uploads ONLY the open
// segment of every stream that is appended to, behind a copy of its header as a stream without entries of its own (as
// tamp_batch_read_ranges stages a unit), with the tables and the sources of those streams, packed.  The device call on those streams gives the new tails and
// their entries, counted from the open segment's start; they come back and are spliced onto the old bytes, which never cross the link.
int batch_append(const TampAmdConf* conf, const AppendCaller& c, uint8_t max_wbits, const AppendOut& o, int mem, int device, void* stream) {
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE) return launch_append(ctx, conf, c, max_wbits, o, false, static_cast<hipStream_t>(stream));
    const uint64_t n = c.n;
    std::vector<uint32_t> start(n, 0), h_in_len(n, 0), h_cap(n, 0), h_src_len(n, 0), t_off, t_len(n);
    std::vector<uint64_t> h_in_off(n, 0), h_out_off(n, 0), h_src_off(n, 0), t_first(n + 1);
    std::vector<int8_t> t_status(n);
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    const uint32_t N = c.interval;
    // whose rows of reset_first hold, and have a table for their entries (the device call's append_index_ok)
    std::vector<uint8_t> holds(n);
    append_rows_hold(c.first, n, holds.data());
    for (uint64_t i = 0; i < n; i++)
        if (holds[i] && !c.off && c.first[i + 1] != c.first[i]) holds[i] = 0;
    const uint64_t unit_bound = reset_segment_bound(N, conf->literal, true);
    uint64_t max_units = 1;
    {
        StreamScratch& rec = ctx->scratch(st);
        std::lock_guard<std::mutex> call_lock(rec.mu);
        max_units = std::max<uint64_t>(read_ranges_budget(rec) / append_unit_cost(N, (uint32_t)unit_bound), 1);
    }
    enum : uint8_t { kWhole = 0, kRun = 1, kFailed = 2 };
    std::vector<uint8_t> kind(n, kWhole);
    std::vector<int8_t> pre(n, 0);
    struct Piece { uint64_t from, at, len; };  // of the caller's source buffer: neighbours there stay neighbours and are one copy
    std::vector<Piece> pieces;
    uint64_t staged = 0, src_all = 0, bound_all = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t L = c.src_len[i];
        if (!L) continue;
        const uint64_t B = append_entry_bound(L, N);
        const uint8_t* const s = c.in + c.in_off[i];
        kind[i] = kFailed;
        if (B + 1 > max_units) { pre[i] = (int8_t)TAMP_AMD_BAD_ARGUMENT; continue; }
        if (c.in_len[i] < kResetHeaderBytes || c.max_wbits > 15 || s[0] != c.header || s[1] != 0 || ((c.header >> 5) & 7u) + 8 > c.max_wbits) {
            pre[i] = (int8_t)TAMP_INVALID_CONF;
            continue;
        }
        pre[i] = (int8_t)TAMP_AMD_BAD_INDEX;
        if (!holds[i]) continue;
        const uint64_t E = c.first[i + 1] - c.first[i];
        bool ok = true;
        for (uint64_t k = 0; k <= E && ok; k++) ok = read_segment_cut(c.first, c.off, c.in_len, i, k).ok;
        if (!ok) continue;
        kind[i] = kRun, pre[i] = 0;
        start[i] = read_segment_cut(c.first, c.off, c.in_len, i, E).start;
        h_in_len[i] = kResetHeaderBytes + (c.in_len[i] - start[i]), h_in_off[i] = staged, staged += h_in_len[i];
        const uint64_t moved = start[i] - kResetHeaderBytes;  // bytes of the new stream that the tail does not hold
        const uint64_t tail_room = o.out_cap[i] > moved ? o.out_cap[i] - moved : 0;
        h_cap[i] = (uint32_t)std::min<uint64_t>(tail_room, std::min<uint64_t>(kResetHeaderBytes + (B + 1) * unit_bound, 0xFFFFFFFFull));
        h_src_len[i] = L, bound_all += B;
        // the sources of the streams that run, back to back: nothing between them goes up
        h_src_off[i] = src_all;
        if (!pieces.empty() && pieces.back().from + pieces.back().len == c.src_off[i]) pieces.back().len += L;
        else pieces.push_back({c.src_off[i], src_all, L});
        src_all += L;
    }
    const uint64_t room = dense_slabs(h_cap.data(), n, h_out_off.data());  // (the tails of the streams that run: the others have no room)
    // the open segments, each behind its stream's header, in pinned staging
    HIP_OK(P.stage[0].need(staged + 64));
    uint8_t* const h_stage = static_cast<uint8_t*>(P.stage[0].p);
    for (uint64_t i = 0; i < n; i++) {
        if (kind[i] != kRun) continue;
        uint8_t* const dst = h_stage + h_in_off[i];
        dst[0] = c.in[c.in_off[i]], dst[1] = 0;
        memcpy(dst + kResetHeaderBytes, c.in + c.in_off[i] + start[i], c.in_len[i] - start[i]);
    }
    HIP_OK(P.in[0].need(staged + 64));
    HIP_OK(P.in[1].need(src_all + 64));
    HIP_OK(P.out[0].need(room + 64));
    TableCarver m;
    const auto m_in_off = m.take<uint64_t>(n), m_out_off = m.take<uint64_t>(n), m_first = m.take<uint64_t>(n + 1);
    const auto m_src_off = m.take<uint64_t>(n), m_new_first = m.take<uint64_t>(n + 1);
    const auto m_in_len = m.take<uint32_t>(n), m_cap = m.take<uint32_t>(n), m_out_len = m.take<uint32_t>(n), m_src_len = m.take<uint32_t>(n);
    const auto m_new_off = m.take<uint32_t>(bound_all);
    const auto m_status = m.take<int8_t>(n);
    HIP_OK(P.meta[0].need(m.bytes()));
    void* const mp = P.meta[0].p;
    uint64_t *const d_in_off = m_in_off.in(mp), *const d_out_off = m_out_off.in(mp), *const d_first = m_first.in(mp);
    uint64_t *const d_src_off = m_src_off.in(mp), *const d_new_first = m_new_first.in(mp);
    uint32_t *const d_in_len = m_in_len.in(mp), *const d_cap = m_cap.in(mp), *const d_out_len = m_out_len.in(mp), *const d_src_len = m_src_len.in(mp);
    uint32_t* const d_new_off = m_new_off.in(mp);
    int8_t* const d_status = m_status.in(mp);
    if (staged) HIP_OK(hipMemcpyAsync(P.in[0].p, h_stage, staged, hipMemcpyHostToDevice, st));
    for (const Piece& pc : pieces)
        HIP_OK(hipMemcpyAsync(static_cast<uint8_t*>(P.in[1].p) + pc.at, c.src + pc.from, pc.len, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_in_off, h_in_off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_out_off, h_out_off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_first, 0, (n + 1) * 8, st));  // (the staged streams have no entries)
    HIP_OK(hipMemcpyAsync(d_src_off, h_src_off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_in_len, h_in_len.data(), n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_cap, h_cap.data(), n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_src_len, h_src_len.data(), n * 4, hipMemcpyHostToDevice, st));
    AppendCaller d = c;
    d.in = static_cast<const uint8_t*>(P.in[0].p), d.in_off = d_in_off, d.in_len = d_in_len, d.first = d_first, d.off = nullptr;
    d.src = static_cast<const uint8_t*>(P.in[1].p), d.src_off = d_src_off, d.src_len = d_src_len;
    uint8_t* const d_out = static_cast<uint8_t*>(P.out[0].p);
    const AppendOut dout = {d_out, d_out_off, d_cap, d_out_len, d_status, d_new_first, bound_all ? d_new_off : nullptr, bound_all};
    if (const int rc = launch_append(ctx, conf, d, max_wbits, dout, true, st)) return rc;
    t_off.resize(bound_all);
    HIP_OK(hipMemcpyAsync(t_len.data(), d_out_len, n * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(t_status.data(), d_status, n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(t_first.data(), d_new_first, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (bound_all) HIP_OK(hipMemcpyAsync(t_off.data(), d_new_off, bound_all * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    uint64_t extent = 0;  // of the tails: behind the last produced byte
    for (uint64_t i = 0; i < n; i++)
        if (kind[i] == kRun && t_status[i] == 0 && t_len[i]) extent = std::max(extent, h_out_off[i] + t_len[i]);
    const uint8_t* back = nullptr;
    if (extent) {
        HIP_OK(P.stage[1].need(extent));
        HIP_OK(hipMemcpyAsync(P.stage[1].p, d_out, extent, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        back = static_cast<const uint8_t*>(P.stage[1].p);
    }
    // the splice: old bytes and old entries in front, the tail and its entries (counted from the open segment's start) behind them.
    // Streams that hold have disjoint entries inside the table, so the cursor stays inside new_reset_cap; it is held against it all
    // the same, and a stream whose entries would overrun keeps none
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t E = holds[i] ? c.first[i + 1] - c.first[i] : 0;
        const uint64_t f0 = c.first[i];
        const bool overrun = at + E < at || at + E > o.new_cap;
        if (overrun) E = 0;
        o.new_first[i] = at;
        if (kind[i] == kWhole) {
            const bool fits = c.in_len[i] <= o.out_cap[i];
            o.status[i] = fits ? (int8_t)TAMP_OK : (int8_t)TAMP_OUTPUT_FULL, o.out_len[i] = fits ? c.in_len[i] : 0;
            if (fits && c.in_len[i]) memcpy(o.out + o.out_off[i], c.in + c.in_off[i], c.in_len[i]);
            for (uint64_t k = 0; k < E; k++) o.new_off[at + k] = c.off[f0 + k];
            at += E;
            continue;
        }
        const uint64_t tail_entries = kind[i] == kRun && t_first[i + 1] >= t_first[i] && t_first[i + 1] <= bound_all ? t_first[i + 1] - t_first[i] : 0;
        const bool fits = !overrun && at + E + tail_entries <= o.new_cap;
        const bool ok = kind[i] == kRun && t_status[i] == 0 && t_len[i] >= kResetHeaderBytes && back && fits;
        const uint64_t moved = ok ? start[i] - kResetHeaderBytes : 0, fresh = ok ? tail_entries : 0;
        o.status[i] = kind[i] == kFailed ? pre[i] : (ok ? (int8_t)TAMP_OK : (!fits ? (int8_t)TAMP_AMD_BAD_INDEX : (t_status[i] ? t_status[i] : (int8_t)TAMP_ERROR)));
        o.out_len[i] = ok ? (uint32_t)(moved + t_len[i]) : 0;
        for (uint64_t k = 0; k < E; k++) o.new_off[at + k] = ok ? c.off[f0 + k] : 0;
        at += E;
        if (!ok) continue;
        memcpy(o.out + o.out_off[i], c.in + c.in_off[i], start[i]);
        memcpy(o.out + o.out_off[i] + start[i], back + h_out_off[i] + kResetHeaderBytes, t_len[i] - kResetHeaderBytes);
        for (uint64_t k = 0; k < fresh; k++) o.new_off[at + k] = (uint32_t)(t_off[t_first[i] + k] + moved);
        at += fresh;
    }
    o.new_first[n] = at;
    return TAMP_OK;
}

// The reset index of a batch that came without one (tamp_batch_index_resets; kernels and steps: tamp_reset_index_kernel.hpp, the
// arithmetic: tamp_reset_index.hpp).  All tables in device memory.  The call waits for the 16 bytes that size the chunk tables, for the
// 4-byte changed-flag of every round, and for the entry count that decides whether the entries fit.  -> TAMP_OK, 1 (more entries than
// reset_cap holds: reset_first, open_size and status are complete, reset_off and closed_size untouched) or an error code.
int launch_index_resets(DeviceCtx* ctx, const IndexCaller& c, uint64_t* reset_first, uint32_t* reset_off, uint32_t* closed_size,
                        uint32_t* open_size, uint64_t reset_cap, int8_t* status, hipStream_t st) {
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    const uint64_t n = c.n;
    const size_t first_at = 256, pre_at = first_at + (n + 1) * 8;
    HIP_OK(rec.index_streams.need(pre_at + 2 * n + 64));
    uint8_t* const sb = static_cast<uint8_t*>(rec.index_streams.p);
    IndexStreams s;
    s.rec = reinterpret_cast<IndexRecord*>(sb), s.chunk_first = reinterpret_cast<uint64_t*>(sb + first_at);
    s.pre = reinterpret_cast<int8_t*>(sb + pre_at), s.bad = reinterpret_cast<uint8_t*>(sb + pre_at + n);
    const CallTiming call_timing(st);
    const IndexChunksArgs count = {c, s};
    hipLaunchKernelGGL(tamp_index_chunks_kernel, dim3(1), dim3(kResetScanTile), 0, st, count);
    HIP_OK(hipGetLastError());
    IndexRecord have = {};
    HIP_OK(hipMemcpyAsync(&have, s.rec, 16, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (have.chunks > 0xFFFF0000ull) return TAMP_AMD_BAD_ARGUMENT;  // (the chunks are numbered in 32 bits: 512 GiB of streams)
    const uint32_t C = (uint32_t)have.chunks, tiles = (C + kResetScanTile - 1) / kResetScanTile, lg = (C + 63) / 64;
    // per chunk: two rows of starts, the report, the place and the running byte count; per tile of the scan its value and what lies in front
    const size_t g_bytes = (((size_t)C + 1) * 4 + 15) & ~(size_t)15, sum_bytes = ((size_t)tiles + 1) * sizeof(IndexSum);
    const size_t rep_at = 2 * g_bytes, place_at = rep_at + (size_t)C * sizeof(IndexChunkReport), bytes_at = place_at + ((size_t)C + 1) * 8;
    const size_t sum_at = bytes_at + ((size_t)C + 1) * 8;
    HIP_OK(rec.index_chunks.need(sum_at + 2 * sum_bytes));
    uint8_t* const cb = static_cast<uint8_t*>(rec.index_chunks.p);
    uint32_t* cur = reinterpret_cast<uint32_t*>(cb);
    uint32_t* nxt = reinterpret_cast<uint32_t*>(cb + g_bytes);
    uint64_t* const place = reinterpret_cast<uint64_t*>(cb + place_at);
    uint64_t* const bytes = reinterpret_cast<uint64_t*>(cb + bytes_at);
    uint64_t rounds = 0, entries = 0;
    if (C == 0) {  // (no stream has chunks: an empty index)
        HIP_OK(hipMemsetAsync(place, 0, 8, st));
        HIP_OK(hipMemsetAsync(bytes, 0, 8, st));
    } else {
        IndexChunkArgs ca = {};
        ca.c = c, ca.s = s, ca.chunks = C;
        const uint64_t bound = index_round_bound(have.longest);
        for (bool settled = false; !settled; rounds++) {
            if (rounds == bound) {  // a defect of the library, not a property of the input
                snprintf(t_last_error, sizeof t_last_error, "tamp_batch_index_resets: the starts did not settle in %llu rounds", (unsigned long long)bound);
                return TAMP_ERROR;
            }
            if (rounds) HIP_OK(hipMemsetAsync(&s.rec->moved, 0, 4, st));
            ca.round0 = rounds == 0, ca.g = cur, ca.g_next = nxt;
            hipLaunchKernelGGL(tamp_index_sync_kernel, dim3(lg), dim3(64), 0, st, ca);
            HIP_OK(hipGetLastError());
            uint32_t moved = 1;
            HIP_OK(hipMemcpyAsync(&moved, &s.rec->moved, 4, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            std::swap(cur, nxt);
            settled = moved == 0;
        }
        ca.g = cur, ca.g_next = nullptr, ca.rep = reinterpret_cast<IndexChunkReport*>(cb + rep_at), ca.write = 0;
        hipLaunchKernelGGL(tamp_index_find_kernel, dim3(lg), dim3(64), 0, st, ca);
        IndexMergeArgs m = {ca.rep, C, tiles, 0, reinterpret_cast<IndexSum*>(cb + sum_at), reinterpret_cast<IndexSum*>(cb + sum_at + sum_bytes),
                            place, bytes, s.rec};
        hipLaunchKernelGGL(tamp_index_merge_kernel, dim3(tiles), dim3(kResetScanTile), 0, st, m);
        m.step = 1;
        hipLaunchKernelGGL(tamp_index_merge_kernel, dim3(1), dim3(kResetScanTile), 0, st, m);
        m.step = 2;
        hipLaunchKernelGGL(tamp_index_merge_kernel, dim3(tiles), dim3(kResetScanTile), 0, st, m);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(&entries, &s.rec->entries, 8, hipMemcpyDeviceToHost, st));
    }
    const IndexStreamsArgs sa = {c, s, cur, place, bytes, reset_first, open_size, status};
    hipLaunchKernelGGL(tamp_index_streams_kernel, dim3((uint32_t)((n + 1 + 255) / 256)), dim3(256), 0, st, sa);
    HIP_OK(hipGetLastError());
    if (C) HIP_OK(hipStreamSynchronize(st));  // (the entry count)
    const bool fits = entries <= reset_cap;
    if (fits && entries) {
        if (entries > 0xFFFFFFFFull * 255) return TAMP_AMD_BAD_ARGUMENT;  // (the grid of the lane-per-entry step)
        uint64_t* d_count = nullptr;
        if (closed_size) {
            HIP_OK(rec.index_entries.need(entries * 8));
            d_count = static_cast<uint64_t*>(rec.index_entries.p);
        }
        IndexChunkArgs wa = {};
        wa.c = c, wa.s = s, wa.chunks = C, wa.g = cur, wa.write = 1, wa.place = place, wa.bytes = bytes, wa.reset_off = reset_off, wa.count = d_count;
        hipLaunchKernelGGL(tamp_index_find_kernel, dim3(lg), dim3(64), 0, st, wa);
        if (closed_size) {
            const IndexSizesArgs za = {reset_first, n, entries, s.chunk_first, bytes, d_count, closed_size};
            hipLaunchKernelGGL(tamp_index_sizes_kernel, dim3((uint32_t)((entries + 255) / 256)), dim3(256), 0, st, za);
        }
        HIP_OK(hipGetLastError());
    }
    if (getenv("TAMP_AMD_RESETS_DEBUG"))
        fprintf(stderr, "[tamp_amd resets] index: %llu streams, %llu chunks, %llu rounds, %llu entries\n", (unsigned long long)n,
                (unsigned long long)C, (unsigned long long)rounds, (unsigned long long)entries);
    return fits ? TAMP_OK : 1;
}

// Host memory, on the host pipeline's first stream (one host-memory call per device at a time): the streams go up once, in one
// transfer of their extent, and the tables alone come back.
int index_resets_host(DeviceCtx* ctx, const IndexCaller& c, uint64_t* reset_first, uint32_t* reset_off, uint32_t* closed_size,
                      uint32_t* open_size, uint64_t reset_cap, int8_t* status) {
    const size_t n = c.n;
    const HostExtent ext(c.in_off, c.in_len, n);
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) total += c.in_len[i];
    const uint64_t cap = std::min<uint64_t>(reset_cap, total);  // (every reset ends on a byte of its own)
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    TableCarver m, o;  // the caller's tables in `meta`, the results in `out`
    const auto m_in_off = m.take<uint64_t>(n);
    const auto m_in_len = m.take<uint32_t>(n);
    const auto o_first = o.take<uint64_t>(n + 1);
    const auto o_off = o.take<uint32_t>(cap), o_closed = o.take<uint32_t>(cap), o_open = o.take<uint32_t>(n);
    const auto o_status = o.take<int8_t>(n);
    HIP_OK(P.in[0].need(ext.bytes() + 64));
    HIP_OK(P.meta[0].need(m.bytes()));
    HIP_OK(P.out[0].need(o.bytes()));
    void *const mp = P.meta[0].p, *const op = P.out[0].p;
    uint64_t *const d_in_off = m_in_off.in(mp), *const d_first = o_first.in(op);
    uint32_t *const d_in_len = m_in_len.in(mp), *const d_off = o_off.in(op), *const d_closed = o_closed.in(op), *const d_open = o_open.in(op);
    int8_t* const d_status = o_status.in(op);
    if (ext.bytes()) HIP_OK(hipMemcpyAsync(P.in[0].p, c.in + ext.lo, ext.bytes(), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_in_off, ext.off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_in_len, c.in_len, n * 4, hipMemcpyHostToDevice, st));
    const IndexCaller d = {static_cast<const uint8_t*>(P.in[0].p), d_in_off, d_in_len, c.n, c.max_wbits};
    const int rc = launch_index_resets(ctx, d, d_first, cap ? d_off : nullptr, closed_size && cap ? d_closed : nullptr,
                                       open_size ? d_open : nullptr, cap, d_status, st);
    if (rc != TAMP_OK && rc != 1) return rc;
    HIP_OK(hipMemcpyAsync(reset_first, d_first, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, st));
    if (open_size) HIP_OK(hipMemcpyAsync(open_size, d_open, n * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const uint64_t E = reset_first[n];
    if (rc == TAMP_OK && E) {
        HIP_OK(hipMemcpyAsync(reset_off, d_off, E * 4, hipMemcpyDeviceToHost, st));
        if (closed_size) HIP_OK(hipMemcpyAsync(closed_size, d_closed, E * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    return rc;
}

int batch_index_resets(const IndexCaller& c, uint64_t* reset_first, uint32_t* reset_off, uint32_t* closed_size, uint32_t* open_size,
                       uint64_t reset_cap, int8_t* status, int mem, int device, void* stream) {
    if (c.n == 0 && mem == TAMP_AMD_MEM_HOST) {  // (nothing to look at: the table's one entry)
        reset_first[0] = 0;
        return TAMP_OK;
    }
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE)
        return launch_index_resets(ctx, c, reset_first, reset_off, closed_size, open_size, reset_cap, status, static_cast<hipStream_t>(stream));
    return index_resets_host(ctx, c, reset_first, reset_off, closed_size, open_size, reset_cap, status);
}

int batch_decompress(BatchTables t, uint8_t max_window_bits, int mem, int device, void* stream) {
    if (const int rc = batch_refused(t, true, mem, device)) return rc;
    if (!t.dict) t.dict_len = 0, t.dict_off = nullptr;  // (no buffer: every stream with the custom bit is TAMP_INVALID_CONF, as ever)
    return on_devices(t, device, [&](DeviceCtx* ctx, int dev, const BatchTables& t) -> int {
        if (mem == TAMP_AMD_MEM_DEVICE) return launch_decompress(ctx, t, max_window_bits, static_cast<hipStream_t>(stream));
        if (t.n == 0) return TAMP_OK;
        HostBatch b{t};
        if (!b.dict_off) b.dict_len = std::min(b.dict_len, kSeedTable);  // (one dictionary: no window reads beyond 32 KiB of it)
        return run_host_batch(ctx, dev, b, plan_wide_chunks(ctx, b), b.dict_len, [&](BatchTables d, uint8_t*, hipStream_t cs) {
            if (!d.dict) d.dict_len = 0, d.dict_off = nullptr;  // (nothing staged: a dictionary of no bytes is no dictionary)
            return launch_decompress(ctx, d, max_window_bits, cs);
        });
    });
}

// (no slab: out = out_off = null, the limits travel as the out_cap table; no dictionary bytes either, only their count)
int batch_decoded_size(BatchTables t, uint8_t max_window_bits, int mem, int device, void* stream) {
    if (const int rc = batch_refused(t, false, mem, device)) return rc;
    if (!t.dict_len) t.dict_off = nullptr;  // (as the decode call without a buffer)
    return on_devices(t, device, [&](DeviceCtx* ctx, int dev, const BatchTables& t) -> int {
        if (mem == TAMP_AMD_MEM_DEVICE) return launch_decoded_size(ctx, t, max_window_bits, static_cast<hipStream_t>(stream));
        if (t.n == 0) return TAMP_OK;
        HostBatch b{t};
        return run_host_batch(ctx, dev, b, plan_wide_chunks(ctx, b), 0,
                              [&](const BatchTables& d, uint8_t*, hipStream_t cs) { return launch_decoded_size(ctx, d, max_window_bits, cs); });
    });
}

// What an array of objects is refused for, whatever the call does with it (the object calls below, the size query for decoder objects).
bool object_array_refused(size_t n, const void* states, size_t state_stride, size_t state_size, uint8_t window_bits_max) {
    return (n && !states) || window_bits_max < 8 || window_bits_max > 15 || (state_stride & 15) || state_stride < state_size ||
           (reinterpret_cast<uintptr_t>(states) & 3);
}

// The two object calls behind their entry points (the reference-named objects of include/tamp_compat.h call them with a one-row
// record): what the call alone checks, then device memory or the host pipeline with the state rows travelling with the chunks.
template <class Launch>  // Launch(ctx, d_states, device tables, stream)
int run_object_batch(const BatchTables& t, void* states, size_t state_stride, size_t state_size, uint8_t window_bits_max, int mem,
                     int device, void* stream, const Launch& launch) {
    if (const int rc = batch_refused(t, true, mem, device)) return rc;
    if (object_array_refused(t.n, states, state_stride, state_size, window_bits_max)) return TAMP_AMD_BAD_ARGUMENT;
    DeviceCtx* ctx = nullptr;  // (objects stay on one device: TAMP_AMD_ALL_DEVICES is no device)
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE) return launch(ctx, static_cast<uint8_t*>(states), t, static_cast<hipStream_t>(stream));
    if (t.n == 0) return TAMP_OK;
    HostBatch b{t};
    b.states = static_cast<uint8_t*>(states), b.state_stride = state_stride, b.exact_out = true;
    return run_host_batch(ctx, device, b, plan_wide_chunks(ctx, b), 0,
                          [&](const BatchTables& d, uint8_t* d_states, hipStream_t cs) { return launch(ctx, d_states, d, cs); });
}

int batch_decompress_resume(const BatchTables& t, void* states, size_t state_stride, uint8_t window_bits_max, int mem, int device,
                            void* stream) {
    return run_object_batch(t, states, state_stride, tamp_amd_decoder_state_size(window_bits_max), window_bits_max, mem, device, stream,
                            [&](DeviceCtx* ctx, uint8_t* d_states, const BatchTables& d, hipStream_t st) {
        return launch_decompress_resume(ctx, d_states, state_stride, window_bits_max, d, st);
    });
}

int batch_compress_resume(const BatchTables& t, void* states, size_t state_stride, uint8_t window_bits_max, int op, int write_token,
                          int mem, int device, void* stream) {
    if (op < TAMP_AMD_OP_POLL || op > TAMP_AMD_OP_COMPRESS_AND_FLUSH) return TAMP_AMD_BAD_ARGUMENT;
    return run_object_batch(t, states, state_stride, tamp_amd_encoder_state_size(window_bits_max), window_bits_max, mem, device, stream,
                            [&](DeviceCtx* ctx, uint8_t* d_states, const BatchTables& d, hipStream_t st) {
        return launch_compress_resume(ctx, d_states, state_stride, window_bits_max, op, write_token, d, st);
    });
}

// tamp_batch_pack behind its checks: the scan of the padded lengths (tamp_pack_kernel.hpp), then the copy unless the call only asks
// for the offsets.  Nothing is read back and the stream is never waited for: the grids come from n and the CU count (the copy's is
// cut down by what dst_cap can hold in tiles), and whatever depends on the lengths the kernels take from dst_off.
int launch_pack(DeviceCtx* ctx, const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len, uint8_t* dst, uint64_t dst_cap,
                uint64_t* dst_off, uint64_t n, uint32_t align, hipStream_t st) {
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    constexpr uint32_t kMaxRanges = kResetScanTile;  // (the offsets kernel sums the ranges in front of its own in one step)
    HIP_OK(rec.pack.need(kMaxRanges * sizeof(uint64_t), false));
    const uint64_t steps = (n + kResetScanTile - 1) / kResetScanTile;
    const uint64_t ranges = std::max<uint64_t>(1, std::min<uint64_t>({steps, (uint64_t)ctx->cu_count * 4, kMaxRanges}));
    const uint64_t per = std::max<uint64_t>(1, (steps + ranges - 1) / ranges) * kResetScanTile;
    const uint32_t scan_grid = (uint32_t)std::max<uint64_t>(1, (n + per - 1) / per);
    const PackScanArgs scan = {src_len, n, per, align, static_cast<uint64_t*>(rec.pack.p), dst_off};
    if (scan_grid > 1) hipLaunchKernelGGL(tamp_pack_sums_kernel, dim3(scan_grid), dim3(kResetScanTile), 0, st, scan);
    hipLaunchKernelGGL(tamp_pack_offsets_kernel, dim3(scan_grid), dim3(kResetScanTile), 0, st, scan);
    if (dst && n) {
        const uint64_t most_tiles = dst_cap / kPackTile + 2;  // (a destination at any address: a cut tile at either end)
        const uint32_t grid = (uint32_t)std::min<uint64_t>(most_tiles, (uint64_t)ctx->cu_count * 8);
        hipLaunchKernelGGL(tamp_pack_copy_kernel, dim3(grid), dim3(kPackCopyThreads), 0, st, src, src_off, src_len, dst, dst_cap,
                           (const uint64_t*)dst_off, n);
    }
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// One stream at offset 0 of its buffers, in host memory: the one-row batch of the one-shot, object and piece calls.
struct OneRow {
    uint64_t zero = 0;
    uint32_t ilen, ocap, olen = 0, consumed = 0;
    int8_t status = TAMP_ERROR;
    OneRow(size_t input_size, size_t output_size, size_t most_in = 0xFFFFFFFFu, size_t most_out = 0xFFFFFFFFu)
        : ilen((uint32_t)std::min(input_size, most_in)), ocap((uint32_t)std::min(output_size, most_out)) {}
    BatchTables tables(const uint8_t* in, uint8_t* out) {  // (a null or empty buffer: a byte of the library's own to point at)
        static unsigned char empty = 0;
        BatchTables t;
        t.in = in && ilen ? in : &empty, t.in_off = &zero, t.in_len = &ilen;
        t.out = ocap ? out : &empty, t.out_off = &zero, t.out_cap = &ocap, t.out_len = &olen, t.status = &status;
        t.in_consumed = &consumed, t.n = 1;
        return t;
    }
};

}  // namespace

#include "tamp_pieces.hpp"
#include "tamp_seek.hpp"

extern "C" {

void tamp_initialize_dictionary(unsigned char* buffer, size_t size, uint8_t literal) {
    seed_dictionary_host(buffer, size, literal);
}

int8_t tamp_compute_min_pattern_size(uint8_t window, uint8_t literal) {
    return (int8_t)min_pattern_size(window, literal);
}

// common.h:424 / common.c:58-86: ring[pos..pos+n) (destination wraps) <- ring[off..off+n) (source does not), with the
// result of reading every source byte before any is overwritten.  A host-side buffer utility of the reference's ABI
// (the device decoders have their own copies of this rule); no codec work.
void tamp_window_copy(unsigned char* window, uint16_t* window_pos, uint16_t window_offset, uint8_t match_size,
                      uint16_t window_mask) {
    unsigned char tmp[256];
    for (unsigned i = 0; i < match_size; i++) tmp[i] = window[(size_t)window_offset + i];
    uint16_t p = *window_pos;
    for (unsigned i = 0; i < match_size; i++) {
        window[p] = tmp[i];
        p = (uint16_t)((p + 1) & window_mask);
    }
    *window_pos = p;
}

size_t tamp_amd_compress_bound(size_t n, uint8_t literal, int dictionary_reset) {
    return 1 + (dictionary_reset ? 1 : 0) + (n * ((size_t)literal + 1) + 7) / 8;
}

size_t tamp_amd_compress_resets_bound(size_t n, uint32_t reset_interval, uint8_t literal) {
    if (!reset_interval) return 0;
    return (size_t)reset_stream_bound(n, reset_interval, literal);
}

size_t tamp_amd_compress_resets_slab(size_t n, uint32_t reset_interval, uint8_t literal) {
    return reset_interval ? reset_slab_bytes(n, reset_interval, literal) : 0;
}

int tamp_amd_compress_resets(const TampAmdConf* conf, const uint8_t* in, uint64_t in_len, uint32_t reset_interval, uint8_t* out,
                             uint64_t out_cap, uint64_t* out_len, int8_t* status, uint64_t* reset_off, int mem, int device,
                             void* stream) {
    if (!conf || !out_len || !status || (in_len && !in) || (out_cap && !out)) return TAMP_AMD_BAD_ARGUMENT;
    if (mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) return TAMP_AMD_BAD_ARGUMENT;
    if (!conf_valid(conf) || conf->lazy_matching > 1 || !conf->dictionary_reset || conf->use_custom_dictionary || !reset_interval ||
        in_len > 0xFFFFFFFFull)
        return TAMP_AMD_BAD_ARGUMENT;
    // (a table row's capacity is 32 bits wide: a segment whose worst case does not fit one is not taken)
    if (reset_segment_bound(std::min<uint64_t>(reset_interval, std::max<uint64_t>(in_len, 1)), conf->literal, true) > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    return compress_resets(conf, in, in_len, reset_interval, out, out_cap, out_len, status, reset_off, mem, device, stream);
}

int tamp_amd_decompress_resets(uint8_t max_window_bits, const uint8_t* in, uint32_t in_len, uint8_t* out, uint32_t out_cap,
                               uint32_t* out_len, int8_t* status, uint32_t* in_consumed, int mem, int device, void* stream) {
    if (!out_len || !status || (in_len && !in)) return TAMP_AMD_BAD_ARGUMENT;
    if (mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) return TAMP_AMD_BAD_ARGUMENT;
    uint32_t consumed = 0;
    static const unsigned char empty = 0;
    const int rc = decompress_resets(max_window_bits, in_len ? in : &empty, in_len, out, out_cap, out_len, status, &consumed, in_len ? mem : TAMP_AMD_MEM_HOST, device, stream);
    if (rc == TAMP_OK && in_consumed) *in_consumed = consumed;
    return rc;
}

int tamp_amd_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

const char* tamp_amd_version(void) { return "tamp_amd 0.1 (gfx950)"; }

int tamp_amd_compress_plan(uint8_t window_bits, uint32_t max_in_len, int lazy_matching, uint32_t* block_positions,
                           uint32_t* lds_bytes, uint32_t* threads, uint32_t* workgroups_per_cu) {
    if (window_bits < 8 || window_bits > 15) return TAMP_AMD_BAD_ARGUMENT;
    TampAmdConf conf = {};  // (a plain batch call with TAMP_AMD_HINT_AUTO: the format and the literal width do not move what is reported)
    conf.window = window_bits, conf.literal = 8, conf.lazy_matching = lazy_matching != 0;
    const CompressPlan p = plan_compress(compress_call(&conf, max_in_len, 0));
    if (block_positions) *block_positions = p.blk;
    if (lds_bytes) *lds_bytes = p.lds.total;
    if (threads) *threads = p.threads;
    if (workgroups_per_cu) *workgroups_per_cu = p.per_cu;
    return TAMP_OK;
}

int tamp_amd_compress_build(const TampAmdConf* conf, uint32_t max_in_len, uint32_t call_flags, uintptr_t dictionary_address) {
    if (!conf || conf->window < 8 || conf->window > 15 || conf->literal < 5 || conf->literal > 8) return TAMP_AMD_BAD_ARGUMENT;
    if (call_flags & TAMP_AMD_CALL_BLOCK_MODE) return TAMP_AMD_BUILD_GENERIC;  // (launch_compress_blocks takes the call: its own build)
    CompressCall call = compress_call(conf, max_in_len, dictionary_address);
    if (call_flags & TAMP_AMD_CALL_APPEND) call.nlead = 2, call.lead = 0;  // (FLUSH + padding in front instead of the header: tamp_amd_compress_segment)
    if (call_flags & TAMP_AMD_CALL_RESUME) call.seg_flags |= kSegResume, call.nlead = 0;
    if (call_flags & TAMP_AMD_CALL_SAVE) call.seg_flags |= kSegSave;
    if (call_flags & TAMP_AMD_CALL_FLUSH_TOKEN) call.seg_flags |= kSegFlushToken;
    if (call_flags & TAMP_AMD_CALL_PARTIAL) call.seg_flags |= kSegPartial;
    call.has_state = (call_flags & TAMP_AMD_CALL_STATE) != 0;
    call.dict_table = (call_flags & TAMP_AMD_CALL_DICT_TABLE) != 0;
    const CompressBuild b = plan_compress(call).build;
    return b == CompressBuild::kFixedExt ? TAMP_AMD_BUILD_FIXED_EXT : (b == CompressBuild::kFixedV1 ? TAMP_AMD_BUILD_FIXED_V1 : TAMP_AMD_BUILD_GENERIC);
}

int tamp_amd_decompress_plan(const TampAmdDecodeQuery* q, TampAmdDecodePlan* out) {
    if (!q || !out || q->n_streams == 0) return TAMP_AMD_BAD_ARGUMENT;
    const DecodeCall call = {(size_t)q->n_streams, q->max_window_bits, q->has_dictionary != 0};
    DecodeScan scan;
    scan.found = q->scan_found, scan.longest_in = q->scan_longest_in, scan.window_units = q->scan_window_units, scan.max_out_cap = q->scan_max_out_cap;
    const DecodeDevice dev = {q->cu_count, q->free_known != 0, (size_t)q->free_bytes, (size_t)q->held_bytes};
    const DecodeLong gate = decode_wants_long(call);
    const DecodePlan p = plan_decompress(call, scan, dev, !q->exclude_split);
    *out = {};
    out->long_attempt = gate.attempt, out->long_min_len = gate.min_len, out->long_extended = gate.extended, out->long_chain = gate.chain;
    out->scan = decode_wants_scan(call);
    out->decoder = p.decoder == Decoder::kSplit ? TAMP_AMD_DECODER_SPLIT : p.decoder == Decoder::kWave ? TAMP_AMD_DECODER_WAVE
                   : p.decoder == Decoder::kLaneLds ? TAMP_AMD_DECODER_LANE_LDS : TAMP_AMD_DECODER_LANE_GLOBAL;
    out->max_window_bits = p.max_wbits, out->bulk = p.bulk;
    if (p.decoder == Decoder::kSplit) {
        const SplitGeometry& g = p.split;
        out->split_tokcap = g.tokcap, out->split_maxcap = g.maxcap, out->split_wave_resolve = g.wave_resolve, out->split_resolve_lds = g.resolve_lds;
        out->split_spw = g.spw((uint32_t)g.slice), out->split_slice = g.slice, out->split_slab_bytes = g.slab_bytes(g.slice);
    }
    out->wave_waves = p.wave.waves, out->wave_lds = p.wave_lds, out->wave_groups = p.wave.groups;
    out->lane_lds_row = p.lane.lds_row, out->lane_lds = p.lane.lds, out->lane_per_cu = p.lane.per_cu, out->lane_grid = p.lane.grid;
    out->global_slot = p.global.slot, out->global_grid = p.global.grid, out->global_bulk = p.global.gbulk, out->global_lds = p.global.lds;
    out->global_lanes = p.global.lanes, out->global_slab_bytes = p.global.slab_bytes;
    return TAMP_OK;
}

const char* tamp_amd_last_error(void) { return t_last_error; }

#if defined(TAMP_PROF)
// debug-only: per-phase cycle counters (not part of the public header)
int tamp_amd_prof_read(unsigned long long* out6) {
    if (!g_prof) {
        if (hipMalloc(&g_prof, 128) != hipSuccess) return -1;
        (void)hipMemset(g_prof, 0, 128);
        for (int i = 0; i < 12; i++) out6[i] = 0;
        return 0;
    }
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(out6, g_prof, 128, hipMemcpyDeviceToHost);
    (void)hipMemset(g_prof, 0, 128);
    return 0;
}
#endif

void* tamp_amd_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void tamp_amd_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

void tamp_amd_set_timing(int enabled) { t_timing = enabled != 0; }


// Release the scratch the library keeps between calls on `device`: every HIP stream's record (StreamScratch: decoder
// window slab, split-decoder records, block-mode tables, expensive-first tables, the long-stream decoder's three buffers;
// not the 32 bytes of the header pre-pass) and the staging of the host-memory pipeline (pinned host buffers and device chunk
// buffers).  Every stream that owns a record is synchronised first.  Returns the number of bytes released, or a negative
// TAMP_AMD_* code.
long long tamp_amd_trim(int device) {
    DeviceCtx* ctx = nullptr;
    int rc = get_ctx(device, &ctx);
    if (rc != TAMP_OK) return rc;
    long long freed = 0;
    std::vector<std::pair<hipStream_t, StreamScratch*>> records;
    {
        std::lock_guard<std::mutex> lock(ctx->scratch_mu);
        for (auto& kv : ctx->scratch_of) records.emplace_back(kv.first, &kv.second);  // (map nodes do not move)
    }
    for (auto& sr : records) {
        std::lock_guard<std::mutex> call_lock(sr.second->mu);  // a call in flight on the stream finishes its launches first
        if (hipStreamSynchronize(sr.first) != hipSuccess) (void)hipGetLastError();  // (a stream the caller has destroyed)
        freed += (long long)sr.second->release();
    }
    {   // the host-memory pipeline: pinned staging of non-tiling output slabs (it grows with the largest extent ever staged,
        // possibly gigabytes of pinned RAM), the device-side chunk and state-row buffers, the custom dictionary; all grow
        // again on demand
        DeviceCtx::HostPipe& P = ctx->pipe;
        std::lock_guard<std::mutex> pipe_lock(P.mu);
        for (int i = 0; i < DeviceCtx::HostPipe::kDepth; i++) {
            if (P.s[i] && hipStreamSynchronize(P.s[i]) != hipSuccess) (void)hipGetLastError();
            freed += (long long)P.stage[i].release();
            for (auto* g : {&P.in[i], &P.out[i], &P.meta[i], &P.state[i]}) freed += (long long)g->release();
        }
        freed += (long long)P.dict.release();
    }
    return freed;
}

float tamp_amd_last_kernel_ms(void) {
    if (!t_ev_valid) return -1.0f;
    if (hipEventSynchronize(t_ev1) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, t_ev0, t_ev1) != hipSuccess) return -1.0f;
    return ms;
}

// The batch calls: each entry point puts its tables into one record (BatchTables) and hands it on.
int tamp_batch_compress_dicts(const TampAmdConf* conf, const uint8_t* dictionaries, size_t dictionaries_len, const uint64_t* dict_off,
                              const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                              const uint32_t* out_cap, uint32_t* out_len, int8_t* status, size_t n_streams, uint32_t max_in_len, int mem,
                              int device, void* stream) {
    return batch_compress(conf, {in, in_off, in_len, out, out_off, out_cap, out_len, status, nullptr, dict_off, dictionaries, dictionaries_len, n_streams},
                          max_in_len, mem, device, stream);
}

int tamp_batch_compress(const TampAmdConf* conf, const uint8_t* dictionary, const uint8_t* in, const uint64_t* in_off,
                        const uint32_t* in_len, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                        uint32_t* out_len, int8_t* status, size_t n_streams, uint32_t max_in_len, int mem, int device,
                        void* stream) {
    return tamp_batch_compress_dicts(conf, dictionary, 0, nullptr, in, in_off, in_len, out, out_off, out_cap, out_len, status, n_streams,
                                     max_in_len, mem, device, stream);
}

// (one implementation for both forms: the plain call asks for no index)
int tamp_batch_compress_resets_index(const TampAmdConf* conf, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                     uint32_t reset_interval, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                     uint32_t* out_len, int8_t* status, size_t n_streams, uint32_t max_in_len, int mem, int device,
                                     void* stream, uint64_t* reset_first, uint32_t* reset_off, uint64_t reset_cap) {
    const BatchTables t = {in, in_off, in_len, out, out_off, out_cap, out_len, status, nullptr, nullptr, nullptr, 0, n_streams};
    if (!conf) return TAMP_AMD_BAD_ARGUMENT;
    if (const int rc = batch_refused(t, true, mem, device)) return rc;
    if (!conf_valid(conf) || conf->lazy_matching > 1 || !conf->dictionary_reset || conf->use_custom_dictionary || !reset_interval)
        return TAMP_AMD_BAD_ARGUMENT;
    // (a table row's capacity is 32 bits wide: an interval whose worst case does not fit one is not taken)
    if (reset_segment_bound(reset_interval, conf->literal, true) > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    if (!reset_off && reset_cap) return TAMP_AMD_BAD_ARGUMENT;  // (room for entries and nowhere to put them)
    return batch_compress_resets(conf, t, reset_interval, max_in_len, {reset_first, reset_off, reset_cap}, mem, device, stream);
}

int tamp_batch_compress_resets(const TampAmdConf* conf, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                               uint32_t reset_interval, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                               uint32_t* out_len, int8_t* status, size_t n_streams, uint32_t max_in_len, int mem, int device,
                               void* stream) {
    return tamp_batch_compress_resets_index(conf, in, in_off, in_len, reset_interval, out, out_off, out_cap, out_len, status, n_streams,
                                            max_in_len, mem, device, stream, nullptr, nullptr, 0);
}

int tamp_batch_decompress_resets(uint8_t max_window_bits, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                 const uint64_t* reset_first, const uint32_t* reset_off, uint8_t* out, const uint64_t* out_off,
                                 const uint32_t* out_cap, uint32_t* out_len, int8_t* status, uint32_t* in_consumed, size_t n_streams,
                                 int mem, int device, void* stream) {
    const BatchTables t = {in, in_off, in_len, out, out ? out_off : nullptr, out_cap, out_len, status, in_consumed, nullptr, nullptr, 0, n_streams};
    // (out_cap is read with and without a slab: it is what decides whether a stream's segments may be decoded on their own)
    if (const int rc = batch_refused(t, out != nullptr, mem, device)) return rc;
    if (device == TAMP_AMD_ALL_DEVICES || (n_streams && (!reset_first || !out_cap))) return TAMP_AMD_BAD_ARGUMENT;
    return batch_decompress_resets(t, reset_first, reset_off, max_window_bits, mem, device, stream);
}

int tamp_batch_read_ranges(uint8_t max_window_bits, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                           const uint64_t* reset_first, const uint32_t* reset_off, uint32_t reset_interval, const uint32_t* range_stream,
                           const uint64_t* range_begin, const uint32_t* range_len, uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                           int8_t* status, size_t n_streams, size_t n_ranges, int mem, int device, void* stream) {
    // (refused before a device is looked for)
    if (!in_off || !in_len || !reset_first || !range_stream || !range_begin || !range_len || !out_off || !out_len || !status)
        return TAMP_AMD_BAD_ARGUMENT;
    if ((!in && n_streams) || (!out && n_ranges) || !reset_interval) return TAMP_AMD_BAD_ARGUMENT;
    if ((mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) || device == TAMP_AMD_ALL_DEVICES) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams > 0xFFFFFFFFull || n_ranges > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    if (n_ranges == 0) return TAMP_OK;  // (nothing is touched)
    const ReadCaller c = {in, in_off, in_len, reset_first, reset_off, n_streams, reset_interval, (uint32_t)(max_window_bits & 0x7F),
                          range_stream, range_begin, range_len, n_ranges};
    return batch_read_ranges(c, max_window_bits, out, out_off, out_len, status, mem, device, stream);
}

int tamp_batch_seek_index(const uint8_t* dictionary, size_t dictionary_len, uint8_t max_window_bits, const uint8_t* in, const uint64_t* in_off,
                          const uint32_t* in_len, uint32_t interval, const uint64_t* ckpt_first, uint32_t* ckpt_in, void* ckpt_state,
                          size_t state_stride, uint64_t* decoded_size, int8_t* status, size_t n_streams, int mem, int device, void* stream) {
    // (refused before a device is looked for)
    if (!in_off || !in_len || !ckpt_first || !decoded_size || !status || (!in && n_streams) || !interval) return TAMP_AMD_BAD_ARGUMENT;
    if ((mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) || device == TAMP_AMD_ALL_DEVICES) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams > 0xFFFFFFFFull || max_window_bits < 8 || max_window_bits > 15) return TAMP_AMD_BAD_ARGUMENT;
    if ((state_stride & 15) || state_stride < tamp_amd_decoder_state_size(max_window_bits) || (reinterpret_cast<uintptr_t>(ckpt_state) & 15))
        return TAMP_AMD_BAD_ARGUMENT;
    if (mem == TAMP_AMD_MEM_HOST && n_streams && ckpt_first[n_streams] > ckpt_first[0] && (!ckpt_in || !ckpt_state)) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams == 0) return TAMP_OK;
    const SeekIndexCall c = {dictionary, dictionary_len, max_window_bits, in, in_off, in_len, interval, ckpt_first, ckpt_in,
                             static_cast<uint8_t*>(ckpt_state), state_stride, decoded_size, status, n_streams};
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE) return launch_seek_index(ctx, c, static_cast<hipStream_t>(stream));
    return seek_index_host(ctx, c);
}

int tamp_batch_seek_index_extend(const uint8_t* dictionary, size_t dictionary_len, uint8_t max_window_bits, const uint8_t* in,
                                 const uint64_t* in_off, const uint32_t* in_len, uint32_t interval, const uint64_t* ckpt_first,
                                 const uint32_t* ckpt_have, uint32_t* ckpt_in, void* ckpt_state, size_t state_stride, uint64_t* decoded_size,
                                 int8_t* status, size_t n_streams, int mem, int device, void* stream) {
    // (refused before a device is looked for)
    if (!in_off || !in_len || !ckpt_first || !ckpt_have || !decoded_size || !status || (!in && n_streams) || !interval) return TAMP_AMD_BAD_ARGUMENT;
    if ((mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) || device == TAMP_AMD_ALL_DEVICES) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams > 0xFFFFFFFFull || max_window_bits < 8 || max_window_bits > 15) return TAMP_AMD_BAD_ARGUMENT;
    if ((state_stride & 15) || state_stride < tamp_amd_decoder_state_size(max_window_bits) || (reinterpret_cast<uintptr_t>(ckpt_state) & 15))
        return TAMP_AMD_BAD_ARGUMENT;
    if (mem == TAMP_AMD_MEM_HOST && n_streams && ckpt_first[n_streams] > ckpt_first[0] && (!ckpt_in || !ckpt_state)) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams == 0) return TAMP_OK;
    const SeekIndexCall c = {dictionary, dictionary_len, max_window_bits, in, in_off, in_len, interval, ckpt_first, ckpt_in,
                             static_cast<uint8_t*>(ckpt_state), state_stride, decoded_size, status, n_streams};
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE) return launch_seek_extend(ctx, c, ckpt_have, nullptr, static_cast<hipStream_t>(stream));
    return seek_extend_host(ctx, c, ckpt_have);
}

int tamp_batch_read_ranges_seek(const uint8_t* dictionary, size_t dictionary_len, uint8_t max_window_bits, const uint8_t* in,
                                const uint64_t* in_off, const uint32_t* in_len, uint32_t interval, const uint64_t* ckpt_first,
                                const uint32_t* ckpt_in, const void* ckpt_state, size_t state_stride, const uint32_t* range_stream,
                                const uint64_t* range_begin, const uint32_t* range_len, uint8_t* out, const uint64_t* out_off,
                                uint32_t* out_len, int8_t* status, size_t n_streams, size_t n_ranges, int mem, int device, void* stream) {
    // (refused before a device is looked for)
    if (!in_off || !in_len || !ckpt_first || !range_stream || !range_begin || !range_len || !out_off || !out_len || !status)
        return TAMP_AMD_BAD_ARGUMENT;
    if ((!in && n_streams) || (!out && n_ranges) || !interval) return TAMP_AMD_BAD_ARGUMENT;
    if ((mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) || device == TAMP_AMD_ALL_DEVICES) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams > 0xFFFFFFFFull || n_ranges > 0xFFFFFFFFull || max_window_bits < 8 || max_window_bits > 15) return TAMP_AMD_BAD_ARGUMENT;
    if ((state_stride & 15) || state_stride < tamp_amd_decoder_state_size(max_window_bits) || (reinterpret_cast<uintptr_t>(ckpt_state) & 15))
        return TAMP_AMD_BAD_ARGUMENT;
    if (n_ranges == 0) return TAMP_OK;  // (nothing is touched)
    const SeekCaller c = {in, in_off, in_len, n_streams, dictionary ? dictionary_len : 0, ckpt_first, ckpt_in,
                          static_cast<const uint8_t*>(ckpt_state), state_stride, interval, max_window_bits, range_stream, range_begin,
                          range_len, n_ranges};
    const SeekReadOut o = {out, out_off, out_len, status};
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE) return launch_read_seek(ctx, c, dictionary, o, static_cast<hipStream_t>(stream));
    return read_seek_host(ctx, c, dictionary, o);
}

int tamp_batch_read_ranges_grid(uint8_t max_window_bits, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                const uint64_t* reset_first, const uint32_t* reset_off, const uint64_t* segment_end,
                                const uint32_t* range_stream, const uint64_t* range_begin, const uint32_t* range_len, uint8_t* out,
                                const uint64_t* out_off, uint32_t* out_len, int8_t* status, size_t n_streams, size_t n_ranges, int mem,
                                int device, void* stream) {
    // (refused before a device is looked for)
    if (!in_off || !in_len || !reset_first || !range_stream || !range_begin || !range_len || !out_off || !out_len || !status)
        return TAMP_AMD_BAD_ARGUMENT;
    if ((!in && n_streams) || (!out && n_ranges) || !segment_end) return TAMP_AMD_BAD_ARGUMENT;
    if ((mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) || device == TAMP_AMD_ALL_DEVICES) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams > 0xFFFFFFFFull || n_ranges > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    if (n_ranges == 0) return TAMP_OK;  // (nothing is touched)
    const ReadCaller c = {in, in_off, in_len, reset_first, reset_off, n_streams, 0, (uint32_t)(max_window_bits & 0x7F),
                          range_stream, range_begin, range_len, n_ranges};
    return batch_read_ranges(c, max_window_bits, out, out_off, out_len, status, mem, device, stream, segment_end);
}

int tamp_batch_segment_ends(const uint64_t* reset_first, const uint32_t* closed_size, const uint32_t* open_size, uint64_t* segment_end,
                            size_t n_streams, int mem, int device, void* stream) {
    // (refused before a device is looked for; closed_size may be null only where there is no entry to read through it, which a
    // host-memory call can tell)
    if (!reset_first || !segment_end || (!open_size && n_streams)) return TAMP_AMD_BAD_ARGUMENT;
    if ((mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) || device == TAMP_AMD_ALL_DEVICES) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    if (!closed_size && (mem == TAMP_AMD_MEM_DEVICE ? n_streams != 0 : reset_first[n_streams] != 0)) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams == 0) return TAMP_OK;  // (no rows)
    if (mem == TAMP_AMD_MEM_HOST) {
        segment_ends_fill(reset_first, closed_size, open_size, segment_end, n_streams);
        return TAMP_OK;
    }
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    return launch_segment_ends(ctx, reset_first, closed_size, open_size, segment_end, n_streams, static_cast<hipStream_t>(stream));
}

int tamp_batch_write_ranges(const TampAmdConf* conf, uint8_t max_window_bits, const uint8_t* in, const uint64_t* in_off,
                            const uint32_t* in_len, const uint64_t* reset_first, const uint32_t* reset_off, uint32_t reset_interval,
                            const uint32_t* write_stream, const uint64_t* write_begin, const uint32_t* write_len, const uint8_t* src,
                            const uint64_t* src_off, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len,
                            int8_t* status, uint32_t* new_reset_off, size_t n_streams, size_t n_writes, int mem, int device, void* stream) {
    // (refused before a device is looked for)
    if (!conf || !in_off || !in_len || !reset_first || !out_off || !out_cap || !out_len || !status) return TAMP_AMD_BAD_ARGUMENT;
    if (n_writes && (!write_stream || !write_begin || !write_len || !src || !src_off)) return TAMP_AMD_BAD_ARGUMENT;
    if (((!in || !out) && n_streams) || !reset_interval) return TAMP_AMD_BAD_ARGUMENT;
    if ((mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) || device == TAMP_AMD_ALL_DEVICES) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams > 0xFFFFFFFFull || n_writes > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    if (!conf_valid(conf) || conf->lazy_matching > 1 || !conf->dictionary_reset || conf->use_custom_dictionary) return TAMP_AMD_BAD_ARGUMENT;
    // (a table row's capacity is 32 bits wide: an interval whose worst case does not fit one is not taken)
    if (reset_segment_bound(reset_interval, conf->literal, true) > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams == 0) return TAMP_OK;  // (nothing is done)
    const WriteCaller c = {in, in_off, in_len, reset_first, reset_off, n_streams, reset_interval, (uint32_t)(max_window_bits & 0x7F),
                           (uint32_t)header_byte(conf, true), conf->literal, write_stream, write_begin, write_len, src, src_off, n_writes};
    return batch_write_ranges(conf, c, max_window_bits, {out, out_off, out_cap, out_len, status, new_reset_off}, mem, device, stream);
}

int tamp_batch_append(const TampAmdConf* conf, uint8_t max_window_bits, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                      const uint64_t* reset_first, const uint32_t* reset_off, uint32_t reset_interval, const uint8_t* src,
                      const uint64_t* src_off, const uint32_t* src_len, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                      uint32_t* out_len, int8_t* status, uint64_t* new_reset_first, uint32_t* new_reset_off, uint64_t new_reset_cap,
                      size_t n_streams, int mem, int device, void* stream) {
    // (refused before a device is looked for)
    if (!conf || !in_off || !in_len || !reset_first || !src_off || !src_len || !out_off || !out_cap || !out_len || !status || !new_reset_first)
        return TAMP_AMD_BAD_ARGUMENT;
    if (((!in || !src || !out) && n_streams) || (!new_reset_off && new_reset_cap) || !reset_interval) return TAMP_AMD_BAD_ARGUMENT;
    if ((mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) || device == TAMP_AMD_ALL_DEVICES) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    if (!conf_valid(conf) || conf->lazy_matching > 1 || !conf->dictionary_reset || conf->use_custom_dictionary) return TAMP_AMD_BAD_ARGUMENT;
    // (a table row's capacity is 32 bits wide: an interval whose worst case does not fit one is not taken)
    if (reset_segment_bound(reset_interval, conf->literal, true) > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams == 0) return TAMP_OK;  // (nothing is done)
    // (host tables: the entries new_reset_off must hold are known here; device tables: from the call's record, before anything is written)
    if (mem == TAMP_AMD_MEM_HOST && append_reset_bound(reset_first[n_streams], src_len, n_streams, reset_interval) > new_reset_cap)
        return TAMP_AMD_BAD_ARGUMENT;
    const AppendCaller c = {in, in_off, in_len, reset_first, reset_off, n_streams, reset_interval, (uint32_t)(max_window_bits & 0x7F),
                            (uint32_t)header_byte(conf, true), conf->literal, src, src_off, src_len};
    return batch_append(conf, c, max_window_bits, {out, out_off, out_cap, out_len, status, new_reset_first, new_reset_off, new_reset_cap}, mem,
                        device, stream);
}

int tamp_batch_index_resets(uint8_t max_window_bits, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                            uint64_t* reset_first, uint32_t* reset_off, uint32_t* closed_size, uint32_t* open_size, uint64_t reset_cap,
                            int8_t* status, size_t n_streams, int mem, int device, void* stream) {
    // (refused before a device is looked for)
    if (!in_off || !in_len || !reset_first || !status || (!in && n_streams) || (!reset_off && reset_cap)) return TAMP_AMD_BAD_ARGUMENT;
    if ((mem != TAMP_AMD_MEM_HOST && mem != TAMP_AMD_MEM_DEVICE) || device == TAMP_AMD_ALL_DEVICES) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    const IndexCaller c = {in, in_off, in_len, n_streams, (uint32_t)(max_window_bits & 0x7F)};
    return batch_index_resets(c, reset_first, reset_off, closed_size, open_size, reset_cap, status, mem, device, stream);
}

int tamp_batch_pack(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len, uint8_t* dst, uint64_t dst_cap,
                    uint64_t* dst_off, size_t n_streams, uint32_t align, int device, void* stream) {
    // (refused before a device is looked for, in the manner of batch_refused)
    if (!src_off || !src_len || !dst_off || (!src && n_streams) || (!dst && dst_cap)) return TAMP_AMD_BAD_ARGUMENT;
    if (n_streams > 0xFFFFFFFFull || !pack_align_ok(align)) return TAMP_AMD_BAD_ARGUMENT;
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    return launch_pack(ctx, src, src_off, src_len, dst, dst_cap, dst_off, n_streams, align, static_cast<hipStream_t>(stream));
}

int tamp_batch_decompress_dicts(const uint8_t* dictionaries, size_t dictionaries_len, const uint64_t* dict_off, uint8_t max_window_bits,
                                const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                const uint32_t* out_cap, uint32_t* out_len, int8_t* status, uint32_t* in_consumed, size_t n_streams,
                                int mem, int device, void* stream) {
    return batch_decompress({in, in_off, in_len, out, out_off, out_cap, out_len, status, in_consumed, dict_off, dictionaries, dictionaries_len, n_streams},
                            max_window_bits, mem, device, stream);
}

int tamp_batch_decompress(const uint8_t* dictionary, size_t dictionary_len, uint8_t max_window_bits, const uint8_t* in,
                          const uint64_t* in_off, const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                          const uint32_t* out_cap, uint32_t* out_len, int8_t* status, uint32_t* in_consumed,
                          size_t n_streams, int mem, int device, void* stream) {
    return tamp_batch_decompress_dicts(dictionary, dictionary_len, nullptr, max_window_bits, in, in_off, in_len, out, out_off, out_cap,
                                       out_len, status, in_consumed, n_streams, mem, device, stream);
}

int tamp_batch_decoded_size_dicts(size_t dictionaries_len, const uint64_t* dict_off, uint8_t max_window_bits, const uint8_t* in,
                                  const uint64_t* in_off, const uint32_t* in_len, const uint32_t* limit, uint32_t* decoded_size,
                                  int8_t* status, uint32_t* in_consumed, size_t n_streams, int mem, int device, void* stream) {
    return batch_decoded_size({in, in_off, in_len, nullptr, nullptr, limit, decoded_size, status, in_consumed, dict_off, nullptr, dictionaries_len, n_streams},
                              max_window_bits, mem, device, stream);
}

int tamp_batch_decoded_size(size_t dictionary_len, uint8_t max_window_bits, const uint8_t* in, const uint64_t* in_off,
                            const uint32_t* in_len, const uint32_t* limit, uint32_t* decoded_size, int8_t* status,
                            uint32_t* in_consumed, size_t n_streams, int mem, int device, void* stream) {
    return tamp_batch_decoded_size_dicts(dictionary_len, nullptr, max_window_bits, in, in_off, in_len, limit, decoded_size, status,
                                         in_consumed, n_streams, mem, device, stream);
}

size_t tamp_amd_decoder_state_size(uint8_t window_bits_max) {
    return sizeof(TampAmdDecoderState) + ((size_t)1 << (window_bits_max & 15));
}

tamp_res tamp_amd_decoder_state_init(void* state, const TampAmdConf* conf, uint8_t window_bits_max) {
    if (!state) return TAMP_AMD_BAD_ARGUMENT;
    if (window_bits_max < 8 || window_bits_max > 15) return TAMP_INVALID_CONF;  // decompressor.c:336
    TampAmdDecoderState* s = static_cast<TampAmdDecoderState*>(state);
    std::memset(s, 0, sizeof *s);
    s->window_bits_max = window_bits_max;
    if (!conf) return TAMP_OK;
    // tamp_decompressor_populate_from_conf, decompressor.c:304-329
    if (!conf_valid(conf) || conf->window > window_bits_max) return TAMP_INVALID_CONF;
    if (!conf->use_custom_dictionary)
        seed_dictionary_host(reinterpret_cast<unsigned char*>(s + 1), (size_t)1 << conf->window,
                             conf->extended ? conf->literal : 8);
    s->conf = header_byte(conf, conf->dictionary_reset);
    s->flags = 1;
    return TAMP_OK;
}

int tamp_batch_decompress_resume(void* states, size_t state_stride, uint8_t window_bits_max, const uint8_t* in,
                                 const uint64_t* in_off, const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                 const uint32_t* out_cap, uint32_t* out_len, int8_t* status, uint32_t* in_consumed,
                                 size_t n_streams, int mem, int device, void* stream) {
    return batch_decompress_resume({in, in_off, in_len, out, out_off, out_cap, out_len, status, in_consumed, nullptr, nullptr, 0, n_streams},
                                   states, state_stride, window_bits_max, mem, device, stream);
}

int tamp_batch_decompress_pieces(void* states, size_t state_stride, uint8_t window_bits_max, const uint32_t* object_index,
                                 const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                 const uint32_t* out_cap, uint32_t* out_len, int8_t* status, uint32_t* in_consumed, size_t n_rows,
                                 int device, void* stream) {
    const BatchTables t = {in, in_off, in_len, out, out_off, out_cap, out_len, status, in_consumed, nullptr, nullptr, 0, n_rows};
    return run_object_batch(t, states, state_stride, tamp_amd_decoder_state_size(window_bits_max), window_bits_max, TAMP_AMD_MEM_DEVICE,
                            device, stream, [&](DeviceCtx* ctx, uint8_t* d_states, const BatchTables& d, hipStream_t st) {
        return launch_decompress_resume(ctx, d_states, state_stride, window_bits_max, d, st, object_index);
    });
}

int tamp_batch_decoded_size_pieces(const void* states, size_t state_stride, uint8_t window_bits_max, const uint32_t* object_index,
                                   const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* limit,
                                   uint32_t* decoded_size, int8_t* status, uint32_t* in_consumed, size_t n_rows, int device, void* stream) {
    // (no slab: out = out_off = null, the limits travel as the out_cap table -- which run_object_batch's check would insist on)
    const BatchTables t = {in, in_off, in_len, nullptr, nullptr, limit, decoded_size, status, in_consumed, nullptr, nullptr, 0, n_rows};
    if (const int rc = batch_refused(t, false, TAMP_AMD_MEM_DEVICE, device)) return rc;
    if (object_array_refused(n_rows, states, state_stride, tamp_amd_decoder_state_size(window_bits_max), window_bits_max))
        return TAMP_AMD_BAD_ARGUMENT;
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    return launch_decoded_size_pieces(ctx, static_cast<const uint8_t*>(states), state_stride, window_bits_max, object_index, t,
                                      static_cast<hipStream_t>(stream));
}

size_t tamp_amd_piece_object_size(uint8_t window_bits) {
    return sizeof(TampAmdPieceObject) + ((size_t)1 << window_bits);
}

int tamp_batch_compress_pieces(const TampAmdConf* conf, void* objects, size_t object_stride, const uint8_t* ops, const uint8_t* in,
                               const uint64_t* in_off, const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                               const uint32_t* out_cap, uint32_t* out_len, int8_t* status, size_t n_objects, uint32_t max_in_len, int mem,
                               int device, void* stream) {
    (void)max_in_len;  // (the call measures its pieces itself: the classify kernel's record)
    return batch_compress_pieces(conf, {objects, object_stride, ops, {in, in_off, in_len, out, out_off, out_cap, out_len, status, nullptr, nullptr, nullptr, 0, n_objects}},
                                 mem, device, stream);
}

int tamp_amd_pieces_phase_ms(float* out4) {
    if (!out4) return TAMP_AMD_BAD_ARGUMENT;
    for (int k = 0; k < 4; k++) out4[k] = -1.0f;
    if (!t_piece_ev_valid || hipEventSynchronize(t_piece_ev[4]) != hipSuccess) return TAMP_OK;
    for (int k = 0; k < 4; k++)
        if (hipEventElapsedTime(&out4[k], t_piece_ev[k], t_piece_ev[k + 1]) != hipSuccess) out4[k] = -1.0f;
    return TAMP_OK;
}

size_t tamp_amd_encoder_state_size(uint8_t window_bits_max) {
    return sizeof(TampAmdEncoderState) + ((size_t)1 << (window_bits_max & 15));
}

tamp_res tamp_amd_encoder_state_init(void* state, const TampAmdConf* conf, int append, uint8_t window_bits_max) {
    if (!state) return TAMP_AMD_BAD_ARGUMENT;
    if (window_bits_max > 15) return TAMP_INVALID_CONF;
    TampAmdEncoderState* s = static_cast<TampAmdEncoderState*>(state);
    return encoder_state_fill(s, reinterpret_cast<unsigned char*>(s + 1), conf, append, window_bits_max);
}

int tamp_batch_compress_resume(void* states, size_t state_stride, uint8_t window_bits_max, int op, int write_token,
                               const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                               const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int8_t* status,
                               uint32_t* in_consumed, size_t n_objects, int mem, int device, void* stream) {
    return batch_compress_resume({in, in_off, in_len, out, out_off, out_cap, out_len, status, in_consumed, nullptr, nullptr, 0, n_objects},
                                 states, state_stride, window_bits_max, op, write_token, mem, device, stream);
}

tamp_res tamp_amd_compress(const TampAmdConf* conf, const unsigned char* dictionary, unsigned char* output,
                           size_t output_size, size_t* output_written_size, const unsigned char* input,
                           size_t input_size, int device) {
    if (output_written_size) *output_written_size = 0;
    if (input_size > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    OneRow row(input_size, output_size);
    BatchTables t = row.tables(input, output);
    t.in_consumed = nullptr, t.dict = dictionary;
    const int rc = batch_compress(conf, t, row.ilen, TAMP_AMD_MEM_HOST, device, nullptr);
    if (rc != TAMP_OK) return (tamp_res)rc;
    if (output_written_size) *output_written_size = row.olen;
    return row.status;
}

tamp_res tamp_amd_decompress(const unsigned char* dictionary, size_t dictionary_len, unsigned char* output,
                             size_t output_size, size_t* output_written_size, const unsigned char* input,
                             size_t input_size, size_t* input_consumed_size, int device) {
    if (output_written_size) *output_written_size = 0;
    if (input_consumed_size) *input_consumed_size = 0;
    if (input_size > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;
    OneRow row(input_size, output_size);
    BatchTables t = row.tables(input, output);
    t.dict = dictionary, t.dict_len = dictionary_len;
    const int rc = batch_decompress(t, 15, TAMP_AMD_MEM_HOST, device, nullptr);
    if (rc != TAMP_OK) return (tamp_res)rc;
    if (output_written_size) *output_written_size = row.olen;
    if (input_consumed_size) *input_consumed_size = row.consumed;
    return row.status;
}

tamp_res tamp_amd_read_header(TampAmdConf* conf, const unsigned char* input, size_t input_size,
                              size_t* input_consumed_size) {
    // decompressor.c:276-297
    if (input_consumed_size) *input_consumed_size = 0;
    if (input_size == 0) return TAMP_INPUT_EXHAUSTED;
    const size_t hs = 1 + (input[0] & 1);
    if (input_size < hs) return TAMP_INPUT_EXHAUSTED;
    if (hs >= 2 && input[1]) return TAMP_INVALID_CONF;
    std::memset(conf, 0, sizeof(*conf));
    conf->window = (uint8_t)(((input[0] >> 5) & 7) + 8);
    conf->literal = (uint8_t)(((input[0] >> 3) & 3) + 5);
    conf->use_custom_dictionary = (input[0] >> 2) & 1;
    conf->extended = (input[0] >> 1) & 1;
    conf->dictionary_reset = input[0] & 1;
    if (input_consumed_size) *input_consumed_size = hs;
    return TAMP_OK;
}


// ---------------------------------------------------------------------------------------------
// The reference's own symbol names for the one-shot path (include/tamp_compat.h)
// ---------------------------------------------------------------------------------------------
namespace {
// TampCompressor::private_ (40 bytes) holds a TampAmdEncoderState, TampDecompressor::private_ (16 bytes) a
// TampAmdDecoderState: the same fields the reference keeps in those objects; the windows are the callers' buffers.
static_assert(sizeof(TampAmdEncoderState) == 40, "encoder state layout (tamp_compress_resume_kernel.hpp reads it as 10 dwords)");
static_assert(sizeof(TampConf) == 2, "TampConf must match the reference (common.h:170-182)");
static_assert(sizeof(TampCompressor) == 48, "TampCompressor must match the reference (compressor.h:13-66)");
static_assert(sizeof(TampDecompressor) == 24, "TampDecompressor must match the reference (decompressor.h:13-57)");
static_assert(sizeof(TampAmdDecoderState) == 16, "private state must fit");
int compat_device() {
    const char* e = getenv("TAMP_AMD_DEVICE");
    return e ? atoi(e) : 0;
}
inline TampAmdEncoderState* enc_state(TampCompressor* c) { return reinterpret_cast<TampAmdEncoderState*>(c->private_); }
inline bool enc_ready(const TampAmdEncoderState* s) {
    return s->window >= 8 && s->window <= 15 && s->literal >= 5 && s->literal <= 8;
}

// One of the reference's calls on one object, exact at any granularity: the resumable device kernel
// (tamp_compress_resume_kernel.hpp) on [state | window], both written back.
tamp_res compat_encoder_call(TampCompressor* compressor, int op, bool write_token, unsigned char* output,
                             size_t output_size, size_t* output_written_size, const unsigned char* input,
                             size_t input_size, size_t* input_consumed_size) {
    if (output_written_size) *output_written_size = 0;
    if (input_consumed_size) *input_consumed_size = 0;
    TampAmdEncoderState* s = enc_state(compressor);
    if (!enc_ready(s) || !compressor->window) return TAMP_ERROR;  // not initialised
    const size_t W = (size_t)1 << s->window;
    const size_t stride = (sizeof *s + W + 15) & ~(size_t)15;
    std::vector<unsigned char> slot(stride);
    std::memcpy(slot.data(), s, sizeof *s);
    std::memcpy(slot.data() + sizeof *s, compressor->window, W);
    OneRow row(input_size, output_size);
    const int rc = batch_compress_resume(row.tables(input, output), slot.data(), stride, s->window, op, write_token, TAMP_AMD_MEM_HOST,
                                         compat_device(), nullptr);
    if (rc != TAMP_OK) return (tamp_res)rc;
    std::memcpy(s, slot.data(), sizeof *s);
    std::memcpy(compressor->window, slot.data() + sizeof *s, W);
    if (output_written_size) *output_written_size = row.olen;
    if (input_consumed_size) *input_consumed_size = row.consumed;
    return row.status;
}

// A whole segment on an object that is between segments (ring empty, nothing pending, output bits byte aligned) with
// ample output room: the batch kernel's segment mode instead of token-by-token parsing.  Same bytes, same state after.
constexpr size_t kCompatPiece = (size_t)1 << 30;  // input bytes one object-level device call looks at
bool compat_segment_applies(const TampAmdEncoderState* s, size_t input_size, size_t output_size) {
    if (input_size < 2048 || input_size > 0xFFFFFFFFull) return false;
    if (s->input_size || s->rle_count || s->extended_match_count || s->cached_match_index >= 0) return false;
    if (s->bit_buffer_pos & 7) return false;
    return output_size >= (size_t)(s->bit_buffer_pos >> 3) + tamp_amd_compress_bound(input_size, s->literal, 0) + 2;
}

tamp_res compat_segment(TampCompressor* compressor, unsigned char* output, size_t output_size,
                        size_t* output_written_size, const unsigned char* input, size_t input_size, bool write_token) {
    TampAmdEncoderState* s = enc_state(compressor);
    const size_t lead = s->bit_buffer_pos >> 3;  // header / append marker still waiting in the bit buffer
    for (size_t k = 0; k < lead; k++) output[k] = (unsigned char)(s->bit_buffer >> (24 - 8 * k));
    TampAmdConf c;
    std::memset(&c, 0, sizeof c);
    c.window = s->window, c.literal = s->literal, c.extended = (s->flags >> 1) & 1;
    c.use_custom_dictionary = s->flags & 1, c.dictionary_reset = (s->flags >> 2) & 1, c.lazy_matching = (s->flags >> 4) & 1;
    size_t written = 0;
    int token = 0;
    uint16_t wp = s->window_pos;
    // data is being processed: the FLUSH at the end of this segment is not "consecutive" (compressor.c:548,784)
    tamp_res r = tamp_amd_compress_segment(&c, 0, 0, 1, write_token, compressor->window, &wp, output + lead,
                                           output_size - lead, &written, input, input_size, &token, compat_device());
    if (r != TAMP_OK) return r;
    s->bit_buffer = 0, s->bit_buffer_pos = 0, s->window_pos = wp, s->last_was_flush = token ? 1 : 0;
    if (output_written_size) *output_written_size = lead + written;
    return TAMP_OK;
}
}  // namespace

namespace {
// tamp_compressor_compress on an object, large input, ample output room: ONE piece for the batch kernel
// (tamp_amd_compress_piece_lazy, finish = 0) instead of token-by-token parsing by one wavefront -- the same stream and the
// same object state as far as any later call can tell, except that every whole output byte leaves now (the reference
// would hold the last token's bits back until the next poll: `written` may run up to four bytes ahead of it).
constexpr size_t kCompatPieceMin = 64 << 10;
bool compat_piece_applies(const TampAmdEncoderState* s, size_t input_size, size_t output_size) {
    if (input_size < kCompatPieceMin || input_size > 0xFFFFFF00ull) return false;
    if (s->input_size > 16 || s->bit_buffer_pos > 31) return false;
    // lazy matching: a cached match goes along (TampAmdLazyCarry) in the shape every poll leaves it in -- nothing else pending,
    // its bytes in the ring; any other object state stays with the token-level kernel
    if (s->cached_match_index >= 0 &&
        (!((s->flags >> 4) & 1) || s->rle_count || s->extended_match_count || s->cached_match_size == 0 ||
         s->cached_match_size > s->input_size || (size_t)s->cached_match_index + s->cached_match_size > ((size_t)1 << s->window)))
        return false;
    return output_size >= tamp_amd_compress_bound(input_size + 300, s->literal, 0) + 8;
}

tamp_res compat_piece(TampCompressor* compressor, unsigned char* output, size_t output_size, size_t* written,
                      const unsigned char* input, size_t input_size) {
    TampAmdEncoderState* s = enc_state(compressor);
    TampAmdConf c;
    std::memset(&c, 0, sizeof c);
    c.window = s->window, c.literal = s->literal, c.extended = (s->flags >> 1) & 1;
    c.use_custom_dictionary = s->flags & 1, c.dictionary_reset = (s->flags >> 2) & 1, c.lazy_matching = (s->flags >> 4) & 1;
    TampAmdLazyCarry lz;
    std::memset(&lz, 0, sizeof lz);
    TampAmdCarry& carry = lz.carry;
    // (cached_match_index / _size: -1 means none, a length of 0 on this side)
    if (s->cached_match_index >= 0) lz.cached_pos = (uint16_t)s->cached_match_index, lz.cached_len = s->cached_match_size;
    carry.rle_count = s->rle_count, carry.ext_count = s->extended_match_count, carry.ext_pos = s->extended_match_position;
    carry.bit_count = s->bit_buffer_pos, carry.bits = s->bit_buffer;
    carry.tail_len = s->input_size;
    for (uint32_t k = 0; k < s->input_size; k++) carry.tail[k] = s->input[(s->input_pos + k) & 15];
    uint16_t wp = s->window_pos;
    int token = 0;
    // (resume = 1: the object's window buffer IS the state -- seeded or custom at init, carried since)
    tamp_res r = tamp_amd_compress_piece_lazy(&c, 0, 0, 1, 0, 0, compressor->window, &wp, &lz, output, output_size, written,
                                              input, input_size, &token, compat_device());
    if (r != TAMP_OK) return r;
    s->window_pos = wp;
    s->cached_match_index = lz.cached_len ? (int16_t)lz.cached_pos : (int16_t)-1;
    s->cached_match_size = lz.cached_len;  // (the token-level kernel reads it only behind an index >= 0)
    s->rle_count = carry.rle_count, s->extended_match_count = carry.ext_count, s->extended_match_position = carry.ext_pos;
    s->bit_buffer_pos = carry.bit_count, s->bit_buffer = carry.bit_count ? carry.bits : 0u;
    s->input_pos = 0, s->input_size = carry.tail_len;
    for (uint32_t k = 0; k < 16; k++) s->input[k] = k < carry.tail_len ? carry.tail[k] : 0;
    s->last_was_flush = 0;  // compressor.c:548
    return TAMP_OK;
}
}  // namespace

tamp_res tamp_compressor_init(TampCompressor* compressor, const TampConf* conf, unsigned char* window) {
    TampAmdConf c;
    std::memset(&c, 0, sizeof c);
    c.window = 10, c.literal = 8, c.extended = 1;  // compressor.c:193-203
    int append = 0;
    if (conf) {
        c.window = conf->window, c.literal = conf->literal, c.extended = conf->extended;
        c.use_custom_dictionary = conf->use_custom_dictionary, c.dictionary_reset = conf->dictionary_reset;
        c.lazy_matching = conf->lazy_matching;
        append = conf->append;
    }
    TampAmdEncoderState fresh;
    unsigned char* seed_into = window;
    const tamp_res r = encoder_state_fill(&fresh, seed_into, &c, append, 15);
    if (r != TAMP_OK) return r;  // compressor.c:208-213: nothing touched on an invalid conf
    std::memset(compressor, 0, sizeof *compressor);
    compressor->window = window;
    std::memcpy(compressor->private_, &fresh, sizeof fresh);
    return TAMP_OK;
}

// compressor.c:665-679: bytes into the 16-byte ring.  A buffer copy on the host; no codec work.
void tamp_compressor_sink(TampCompressor* compressor, const unsigned char* input, size_t input_size,
                          size_t* consumed_size) {
    TampAmdEncoderState* s = enc_state(compressor);
    size_t taken = 0;
    while (taken < input_size && s->input_size < 16) {
        s->input[(s->input_pos + s->input_size) & 15] = input[taken++];
        s->input_size++;
    }
    if (consumed_size) *consumed_size = taken;
}

bool tamp_compressor_full(const TampCompressor* compressor) {
    return reinterpret_cast<const TampAmdEncoderState*>(compressor->private_)->input_size == 16;
}

tamp_res tamp_compressor_poll(TampCompressor* compressor, unsigned char* output, size_t output_size,
                              size_t* output_written_size) {
    return compat_encoder_call(compressor, TAMP_AMD_OP_POLL, false, output, output_size, output_written_size, nullptr, 0,
                               nullptr);
}

tamp_res tamp_compressor_compress_cb(TampCompressor* compressor, unsigned char* output, size_t output_size,
                                     size_t* output_written_size, const unsigned char* input, size_t input_size,
                                     size_t* input_consumed_size, tamp_callback_t callback, void* user_data) {
    // One device call takes up to kCompatPiece bytes (32-bit lengths on the device side); longer inputs go piece by
    // piece on the same object -- the reference's own loop does nothing else (compressor.c:700-719) -- and the progress
    // callback (common.h:184-210: (input consumed, total input)) fires after every piece.
    size_t consumed = 0, written = 0;
    tamp_res r = TAMP_OK;
    if (output_written_size) *output_written_size = 0;
    if (input_consumed_size) *input_consumed_size = 0;
    if (!enc_ready(enc_state(compressor)) || !compressor->window) return TAMP_ERROR;
    // with a progress callback the pieces are smaller: it fires -- and may abort -- after each of them
    const size_t piece_max = callback ? std::min<size_t>(kCompatPiece, env_or("TAMP_AMD_PROGRESS_PIECE_MB", 16) << 20) : kCompatPiece;
    do {
        const size_t piece = std::min(input_size - consumed, piece_max);
        size_t c = 0, w = 0;
        if (compat_piece_applies(enc_state(compressor), piece, output_size - written)) {
            r = compat_piece(compressor, output + written, output_size - written, &w, input + consumed, piece);
            if (r == TAMP_OK) c = piece;  // (every byte is taken: parsed, or waiting in the ring)
        } else {
            r = compat_encoder_call(compressor, TAMP_AMD_OP_COMPRESS, false, output + written, output_size - written, &w,
                                    input + consumed, piece, &c);
        }
        consumed += c, written += w;
        if (r == TAMP_OK && callback) {
            int cb = callback(user_data, consumed, input_size);
            if (cb) r = (tamp_res)cb;
        }
        if (c < piece) break;  // output room ran out (TAMP_OUTPUT_FULL) or an error: the caller sees how far it got
    } while (r == TAMP_OK && consumed < input_size);
    if (input_consumed_size) *input_consumed_size = consumed;
    if (output_written_size) *output_written_size = written;
    return r;
}

tamp_res tamp_compressor_compress(TampCompressor* compressor, unsigned char* output, size_t output_size,
                                  size_t* output_written_size, const unsigned char* input, size_t input_size,
                                  size_t* input_consumed_size) {
    return tamp_compressor_compress_cb(compressor, output, output_size, output_written_size, input, input_size,
                                       input_consumed_size, nullptr, nullptr);
}

tamp_res tamp_compressor_compress_and_flush_cb(TampCompressor* compressor, unsigned char* output, size_t output_size,
                                               size_t* output_written_size, const unsigned char* input,
                                               size_t input_size, size_t* input_consumed_size, bool write_token,
                                               tamp_callback_t callback, void* user_data) {
    if (output_written_size) *output_written_size = 0;
    if (input_consumed_size) *input_consumed_size = 0;
    TampAmdEncoderState* s = enc_state(compressor);
    if (!enc_ready(s) || !compressor->window) return TAMP_ERROR;
    tamp_res r;
    if (compat_segment_applies(s, input_size, output_size)) {
        r = compat_segment(compressor, output, output_size, output_written_size, input, input_size, write_token);
        if (r == TAMP_OK && input_consumed_size) *input_consumed_size = input_size;
    } else if (input_size > kCompatPiece) {  // compressor.c:815-845 as it is written there: compress, then flush
        size_t consumed = 0, written = 0, w2 = 0;
        // (the caller's callback rides along: it sees the progress of every piece and a non-zero return aborts the call
        // there, as in the reference, where it runs per poll)
        r = tamp_compressor_compress_cb(compressor, output, output_size, &written, input, input_size, &consumed, callback, user_data);
        if (r == TAMP_OK && consumed == input_size) {
            r = tamp_compressor_flush(compressor, output + written, output_size - written, &w2, write_token);
            written += w2;
        } else if (r == TAMP_OK) {
            r = TAMP_OUTPUT_FULL;
        }
        if (input_consumed_size) *input_consumed_size = consumed;
        if (output_written_size) *output_written_size = written;
    } else {
        r = compat_encoder_call(compressor, TAMP_AMD_OP_COMPRESS_AND_FLUSH, write_token, output, output_size,
                                output_written_size, input, input_size, input_consumed_size);
    }
    if (r == TAMP_OK && callback) {  // final "100 %" callback, compressor.c:836-842
        int cb = callback(user_data, input_size, input_size);
        if (cb) return (tamp_res)cb;
    }
    return r;
}

tamp_res tamp_compressor_flush(TampCompressor* compressor, unsigned char* output, size_t output_size,
                               size_t* output_written_size, bool write_token) {
    return compat_encoder_call(compressor, TAMP_AMD_OP_FLUSH, write_token, output, output_size, output_written_size,
                               nullptr, 0, nullptr);
}

tamp_res tamp_compressor_reset_dictionary(TampCompressor* compressor, unsigned char* output, size_t output_size,
                                          size_t* output_written_size) {  // compressor.c:845-881
    if (output_written_size) *output_written_size = 0;
    TampAmdEncoderState* s = enc_state(compressor);
    if (!enc_ready(s) || !compressor->window) return TAMP_ERROR;
    if (!(s->flags & 4)) return TAMP_INVALID_CONF;
    for (int i = 0; i < 2; i++) {  // two FLUSH tokens in a row on purpose: the suppression flag is cleared before each
        size_t w = 0;
        s->last_was_flush = 0;
        tamp_res r = tamp_compressor_flush(compressor, output, output_size, &w, true);
        if (output_written_size) *output_written_size += w;
        if (r != TAMP_OK) return r;
        output += w, output_size -= w;
    }
    // re-initialise with the same conf minus the custom dictionary; the header that init writes is discarded
    TampAmdConf c;
    std::memset(&c, 0, sizeof c);
    c.window = s->window, c.literal = s->literal, c.extended = (s->flags >> 1) & 1, c.dictionary_reset = 1;
    c.lazy_matching = (s->flags >> 4) & 1;
    const int append = (s->flags >> 3) & 1;
    const tamp_res r = encoder_state_fill(s, compressor->window, &c, append, 15);
    s->bit_buffer = 0, s->bit_buffer_pos = 0;
    return r;
}

tamp_res tamp_compress_stream(TampCompressor* compressor, tamp_read_t read_cb, void* read_handle,
                              tamp_write_t write_cb, void* write_handle, size_t* input_consumed_size,
                              size_t* output_written_size, tamp_callback_t callback, void* user_data) {
    // compressor.c:891-955: pull, compress, push, until EOF; then flush(write_token=false).  The reference pumps a
    // 32-byte work buffer; here the pull fills a host buffer of at most kStreamBuffer bytes (TAMP_AMD_STREAM_BUFFER_MB,
    // default 64 MiB).  An input that ends inside the first fill is ONE segment for the batch kernel (the fast path:
    // same bytes, tamp_compressor_compress_and_flush).  A longer one is fed buffer by buffer to
    // tamp_compressor_compress on the same object -- exact at any cut, memory bounded -- and flushed at EOF.
    if (input_consumed_size) *input_consumed_size = 0;
    if (output_written_size) *output_written_size = 0;
    TampAmdEncoderState* s = enc_state(compressor);
    if (!enc_ready(s) || !compressor->window) return TAMP_ERROR;
    // (TAMP_AMD_STREAM_BUFFER_BYTES, when set, names the buffer in bytes: measurements at the reference's own 32-byte pump size)
    const size_t kStreamBuffer = env_or("TAMP_AMD_STREAM_BUFFER_BYTES", 0) >= 16 ? env_or("TAMP_AMD_STREAM_BUFFER_BYTES", 0)
                                                                                  : env_or("TAMP_AMD_STREAM_BUFFER_MB", 64) << 20;
    constexpr size_t kChunk = 1 << 16;
    std::vector<unsigned char> in, out;
    size_t total_in = 0, total_out = 0;
    auto push = [&](size_t n) -> tamp_res {
        for (size_t at = 0; at < n;) {
            const size_t k = std::min(n - at, kChunk);
            int w = write_cb(write_handle, out.data() + at, k);
            if (w < 0 || (size_t)w != k) return TAMP_WRITE_ERROR;
            at += k, total_out += k;
            if (output_written_size) *output_written_size = total_out;
        }
        return TAMP_OK;
    };
    bool eof = false, first = true;
    for (;;) {
        in.clear();
        while (!eof && in.size() < kStreamBuffer) {
            const size_t at = in.size();
            in.resize(at + kChunk);
            int got = read_cb(read_handle, in.data() + at, kChunk);
            if (got < 0) return TAMP_READ_ERROR;
            in.resize(at + (size_t)got);
            if (got == 0) eof = true;
        }
        total_in += in.size();
        if (input_consumed_size) *input_consumed_size = total_in;
        if (callback && !in.empty()) {  // once per read chunk, total unknown (common.h:198-200)
            int cb = callback(user_data, total_in, 0);
            if (cb) return (tamp_res)cb;
        }
        out.resize(tamp_amd_compress_bound(in.size() + 320, s->literal, 1) + 64);  // (room that lets a buffer go as ONE piece)
        size_t written = 0, consumed = 0;
        if (eof) {  // last (or only) buffer: compress + flush
            tamp_res r = first ? tamp_compressor_compress_and_flush_cb(compressor, out.data(), out.size(), &written, in.data(),
                                                                       in.size(), &consumed, false, nullptr, nullptr)
                               : tamp_compressor_compress(compressor, out.data(), out.size(), &written, in.data(), in.size(), &consumed);
            if (r != TAMP_OK) return r;
            if (consumed != in.size()) return TAMP_ERROR;
            if ((r = push(written)) != TAMP_OK) return r;
            if (!first) {
                r = tamp_compressor_flush(compressor, out.data(), out.size(), &written, false);
                if (r != TAMP_OK) return r;
                if ((r = push(written)) != TAMP_OK) return r;
            }
            return TAMP_OK;
        }
        tamp_res r = tamp_compressor_compress(compressor, out.data(), out.size(), &written, in.data(), in.size(), &consumed);
        if (r != TAMP_OK) return r;
        if (consumed != in.size()) return TAMP_ERROR;
        if ((r = push(written)) != TAMP_OK) return r;
        first = false;
    }
}

tamp_res tamp_decompress_stream(TampDecompressor* decompressor, tamp_read_t read_cb, void* read_handle,
                                tamp_write_t write_cb, void* write_handle, size_t* input_consumed_size,
                                size_t* output_written_size, tamp_callback_t callback, void* user_data) {
    // decompressor.c:585-640: pull a chunk, decode as far as it goes, push, repeat -- the same loop, with work buffers
    // sized for a device call instead of a microcontroller stack.  Memory stays bounded whatever the stream expands to.
    size_t consumed_proxy, written_proxy;
    if (!input_consumed_size) input_consumed_size = &consumed_proxy;
    if (!output_written_size) output_written_size = &written_proxy;
    *input_consumed_size = 0, *output_written_size = 0;
    constexpr size_t kIn = (size_t)1 << 20, kOut = (size_t)8 << 20;
    std::vector<unsigned char> in(kIn), out(kOut);
    size_t pos = 0, avail = 0;
    bool eof = false;
    for (;;) {
        if (avail == 0 && !eof) {
            const int got = read_cb(read_handle, in.data(), (int)std::min<size_t>(kIn, INT_MAX));
            if (got < 0) return TAMP_READ_ERROR;
            eof = got == 0;
            pos = 0, avail = (size_t)got;
            *input_consumed_size += (size_t)got;
        }
        size_t chunk_consumed = 0, chunk_written = 0;
        const tamp_res res = tamp_decompressor_decompress_cb(decompressor, out.data(), kOut, &chunk_written,
                                                             in.data() + pos, avail, &chunk_consumed, nullptr, nullptr);
        if (res < TAMP_OK) return res;
        pos += chunk_consumed, avail -= chunk_consumed;
        for (size_t at = 0; at < chunk_written;) {
            const size_t n = std::min(chunk_written - at, (size_t)1 << 30);
            const int w = write_cb(write_handle, out.data() + at, n);
            if (w < 0 || (size_t)w != n) return TAMP_WRITE_ERROR;
            at += n;
        }
        *output_written_size += chunk_written;
        if (res == TAMP_INPUT_EXHAUSTED && eof) break;
        if (callback) {
            const int cb = callback(user_data, *input_consumed_size, 0);
            if (cb) return (tamp_res)cb;
        }
    }
    return TAMP_OK;
}

// Built-in I/O handlers (common.c:92-132): plain host adaptors, no codec work.
int tamp_stream_mem_read(void* handle, unsigned char* buffer, size_t size) {
    TampMemReader* r = static_cast<TampMemReader*>(handle);
    const size_t n = std::min(std::min(size, r->size - r->pos), (size_t)INT_MAX);
    std::memcpy(buffer, r->data + r->pos, n);
    r->pos += n;
    return (int)n;
}

int tamp_stream_mem_write(void* handle, const unsigned char* buffer, size_t size) {
    TampMemWriter* w = static_cast<TampMemWriter*>(handle);
    if (size > w->capacity - w->pos || size > (size_t)INT_MAX) return -1;
    std::memcpy(w->data + w->pos, buffer, size);
    w->pos += size;
    return (int)size;
}

int tamp_stream_stdio_read(void* handle, unsigned char* buffer, size_t size) {
    FILE* f = static_cast<FILE*>(handle);
    const size_t n = fread(buffer, 1, std::min(size, (size_t)INT_MAX), f);
    return n == 0 && ferror(f) ? -1 : (int)n;
}

int tamp_stream_stdio_write(void* handle, const unsigned char* buffer, size_t size) {
    FILE* f = static_cast<FILE*>(handle);
    const size_t n = fwrite(buffer, 1, size, f);
    return n < size && ferror(f) ? -1 : (int)n;
}

tamp_res tamp_compressor_compress_and_flush(TampCompressor* compressor, unsigned char* output, size_t output_size,
                                            size_t* output_written_size, const unsigned char* input, size_t input_size,
                                            size_t* input_consumed_size, bool write_token) {
    return tamp_compressor_compress_and_flush_cb(compressor, output, output_size, output_written_size, input,
                                                 input_size, input_consumed_size, write_token, nullptr, nullptr);
}

tamp_res tamp_decompressor_read_header(TampConf* conf, const unsigned char* input, size_t input_size,
                                       size_t* input_consumed_size) {
    TampAmdConf c;
    tamp_res r = tamp_amd_read_header(&c, input, input_size, input_consumed_size);
    if (r != TAMP_OK) return r;
    conf->window = c.window, conf->literal = c.literal, conf->use_custom_dictionary = c.use_custom_dictionary;
    conf->extended = c.extended, conf->dictionary_reset = c.dictionary_reset;
    return TAMP_OK;
}

tamp_res tamp_decompressor_init(TampDecompressor* decompressor, const TampConf* conf, unsigned char* window,
                                uint8_t window_bits) {
    if (window_bits < 8 || window_bits > 15) return TAMP_INVALID_CONF;  // decompressor.c:336
    std::memset(decompressor, 0, sizeof *decompressor);
    decompressor->window = window;
    TampAmdDecoderState* s = reinterpret_cast<TampAmdDecoderState*>(decompressor->private_);
    s->window_bits_max = window_bits;
    if (!conf) return TAMP_OK;
    // tamp_decompressor_populate_from_conf, decompressor.c:304-329
    if (conf->window < 8 || conf->window > 15 || conf->literal < 5 || conf->literal > 8) return TAMP_INVALID_CONF;
    if (conf->window > window_bits) return TAMP_INVALID_CONF;
    if (!conf->use_custom_dictionary)
        seed_dictionary_host(window, (size_t)1 << conf->window, conf->extended ? conf->literal : 8);
    s->conf = header_byte(conf, conf->dictionary_reset);
    s->flags = 1;
    return TAMP_OK;
}

tamp_res tamp_decompressor_decompress_cb(TampDecompressor* decompressor, unsigned char* output, size_t output_size,
                                         size_t* output_written_size, const unsigned char* input, size_t input_size,
                                         size_t* input_consumed_size, tamp_callback_t callback, void* user_data) {
    // One call of the reference's (decompressor.c:371-578) = one step of the resumable device decoder on this object:
    // state from private_, window from the caller's buffer, both written back afterwards.
    if (output_written_size) *output_written_size = 0;
    if (input_consumed_size) *input_consumed_size = 0;
    TampAmdDecoderState* s = reinterpret_cast<TampAmdDecoderState*>(decompressor->private_);
    const uint8_t bits_max = s->window_bits_max;
    if (bits_max < 8 || bits_max > 15 || !decompressor->window) return TAMP_ERROR;  // not initialised
    const size_t wcap = (size_t)1 << bits_max;
    // before the header is known the whole buffer may hold a custom dictionary; afterwards 1 << window bytes are live
    const size_t wlive = (s->flags & 1) ? (size_t)1 << (((s->conf >> 5) & 7) + 8) : wcap;
    std::vector<unsigned char> slot(sizeof(TampAmdDecoderState) + wcap);
    std::memcpy(slot.data(), s, sizeof *s);
    std::memcpy(slot.data() + sizeof *s, decompressor->window, wlive);
    size_t written = 0, consumed = 0;
    int8_t st = TAMP_ERROR;
    for (;;) {  // one device step per 256 MiB of input / 1 GiB of output room (the kernel's counters are 32 bits wide)
        OneRow row(input_size - consumed, output_size - written, 0x10000000u, 0x40000000u);
        const int rc = batch_decompress_resume(row.tables(input + consumed, output + written), slot.data(), slot.size(), bits_max,
                                               TAMP_AMD_MEM_HOST, compat_device(), nullptr);
        if (rc != TAMP_OK) return (tamp_res)rc;
        st = row.status;
        written += row.olen, consumed += row.consumed;
        const bool more_in = st == TAMP_INPUT_EXHAUSTED && row.consumed == row.ilen && consumed < input_size;
        const bool more_out = st == TAMP_OUTPUT_FULL && row.olen == row.ocap && written < output_size;
        if (!more_in && !more_out) break;
    }
    std::memcpy(s, slot.data(), sizeof *s);
    const size_t wnow = (s->flags & 1) ? (size_t)1 << (((s->conf >> 5) & 7) + 8) : 0;
    if (wnow) std::memcpy(decompressor->window, slot.data() + sizeof *s, wnow);
    if (output_written_size) *output_written_size = written;
    if (input_consumed_size) *input_consumed_size = consumed;
    if (st >= 0 && callback) {
        const int cb = callback(user_data, consumed, input_size);
        if (cb) return (tamp_res)cb;
    }
    return st;
}

tamp_res tamp_decompressor_decompress(TampDecompressor* decompressor, unsigned char* output, size_t output_size,
                                      size_t* output_written_size, const unsigned char* input, size_t input_size,
                                      size_t* input_consumed_size) {
    return tamp_decompressor_decompress_cb(decompressor, output, output_size, output_written_size, input, input_size,
                                           input_consumed_size, nullptr, nullptr);
}


// ---------------------------------------------------------------------------------------------
// Segment call: one piece of a stream between two flush points, with the window carried in and out.
// This is what tamp.Compressor.write()/flush()/reset_dictionary() need (compressor.c:227-241,728-881).
// ---------------------------------------------------------------------------------------------
namespace {
// One piece of a stream on the batch kernel.  finish = 1: the piece ends with tamp_compressor_flush(flush_token) -- a
// SEGMENT; finish = 0: it ends the way tamp_compressor_compress ends a call (compressor.c:681-722) and `carry` takes what
// the reference's object would still hold.  A carry that comes in is continued from (its run / extended match bytes and
// its unparsed tail are put back in front of the input: tamp_compress_kernel.hpp, kSegStateExtra).
// `cached_pos` / `cached_len` (both or neither): the cached match of lazy matching beside the carry (kSlotLazyPos / kSlotLazyLen).
// Without them an unfinished piece of a lazy configuration is refused: the match would be lost.
tamp_res segment_core(const TampAmdConf* conf, int emit_header, int append_marker, int resume, int finish, int flush_token,
                      unsigned char* window_state, uint16_t* window_pos, TampAmdCarry* carry, unsigned char* output,
                      size_t output_size, size_t* output_written_size, const unsigned char* input, size_t input_size,
                      int* token_written, int device, uint16_t* cached_pos = nullptr, uint8_t* cached_len = nullptr) {
    if (output_written_size) *output_written_size = 0;
    if (token_written) *token_written = 0;
    if (!conf_valid(conf) || conf->lazy_matching > 1 || !window_state || !window_pos) return TAMP_INVALID_CONF;
    if (!finish && (!carry || (conf->lazy_matching && !cached_len))) return TAMP_AMD_BAD_ARGUMENT;  // (lazy: nowhere to leave the cached match)
    if (cached_len && *cached_len) {
        // a cached match belongs to a lazy object in the middle of its input, with no run or extended match pending
        // (compressor.c:563-570), and its bytes are ring bytes: the probe saw nothing else (:588-596)
        if (!carry || !resume || !conf->lazy_matching || carry->rle_count || carry->ext_count ||
            (size_t)*cached_pos + *cached_len > ((size_t)1 << conf->window) || *cached_len > carry->tail_len)
            return TAMP_AMD_BAD_ARGUMENT;
    }
    if (input_size > 0xFFFFFF00ull) return TAMP_AMD_BAD_ARGUMENT;
    DeviceCtx* ctx = nullptr;
    int rc = get_ctx(device, &ctx);
    if (rc != TAMP_OK) return (tamp_res)rc;
    const size_t W = (size_t)1 << conf->window;
    SegmentSpec seg;
    seg.flags = kSegSave | (resume ? kSegResume : 0) | ((finish && flush_token) ? kSegFlushToken : 0) | (finish ? 0 : kSegPartial);
    if (append_marker) {  // compressor.c:227-235: FLUSH (9 bits) padded to 16 bits instead of a header
        seg.nlead = 2, seg.lead = (uint16_t)(0xABu << 7);
    } else if (emit_header) {
        const uint8_t header = header_byte(conf, conf->dictionary_reset);
        seg.nlead = conf->dictionary_reset ? 2 : 1, seg.lead = (uint16_t)(header << 8);
    } else {
        seg.nlead = 0, seg.lead = 0;
    }
    // what leads the input: the bytes a carried run / extended match has consumed (they are window bytes: the last byte
    // written, resp. window[pos .. pos + count)), then the carried tail of the 16-byte ring
    std::vector<unsigned char> prefix;
    std::vector<unsigned char> stbuf(W + kSegStateExtra, 0);  // the kernel's state slot (kSlot* fields behind the window)
    std::memcpy(stbuf.data(), window_state, W);
    auto put = [&](uint32_t field, uint32_t v, int bytes) {
        for (int k = 0; k < bytes; k++) stbuf[W + field + k] = (unsigned char)(v >> (8 * k));
    };
    auto get = [&](uint32_t field, int bytes) {
        uint32_t v = 0;
        for (int k = 0; k < bytes; k++) v |= (uint32_t)stbuf[W + field + k] << (8 * k);
        return v;
    };
    put(kSlotWindowPos, *window_pos, 2);
    if (carry && resume) {
        if (carry->tail_len > 16 || carry->bit_count > 31 || (carry->rle_count && carry->ext_count) ||
            (size_t)carry->ext_pos + carry->ext_count > W || ((emit_header || append_marker) && carry->bit_count))
            return TAMP_AMD_BAD_ARGUMENT;
        const unsigned char last = window_state[(*window_pos - 1) & (W - 1)];
        prefix.insert(prefix.end(), carry->rle_count, last);
        prefix.insert(prefix.end(), window_state + carry->ext_pos, window_state + carry->ext_pos + carry->ext_count);
        prefix.insert(prefix.end(), carry->tail, carry->tail + carry->tail_len);
        put(kSlotRle, carry->rle_count, 1), put(kSlotExtCount, carry->ext_count, 1), put(kSlotNbits, carry->bit_count, 1);
        put(kSlotExtPos, carry->ext_pos, 2), put(kSlotBits, carry->bits, 4);
        if (cached_len && *cached_len) put(kSlotLazyLen, *cached_len, 1), put(kSlotLazyPos, *cached_pos, 2);
    }
    if (!finish && resume && input_size == 0 && !seg.nlead) {
        // tamp_compressor_compress without input: nothing is sunk and nothing polled, even on a full ring
        // (compressor.c:700); the whole bytes among the pending bits leave, as at the end of every piece
        const size_t whole = carry->bit_count >> 3;
        if (output_size < whole) return TAMP_OUTPUT_FULL;
        for (size_t k = 0; k < whole; k++) output[k] = (unsigned char)(carry->bits >> (24 - 8 * k));
        carry->bits = whole ? carry->bits << (8 * whole) : carry->bits;
        carry->bit_count &= 7;
        if (output_written_size) *output_written_size = whole;
        return TAMP_OK;
    }
    if (finish && !flush_token && !resume && emit_header && !append_marker && prefix.empty() && !conf->extended &&
        !conf->lazy_matching && conf->literal == 8 && conf->window <= kPackedMaxWbits && input_size >= ((size_t)256 << 10) &&
        input_size <= 0xFFFFFF00ull) {
        // A whole fresh v1 stream in one finishing call: the batch call takes it as ONE stream and spreads its blocks over
        // all workgroups (launch_compress_blocks).  The object afterwards holds what the reference's would: every consumed
        // byte was written (compressor.c:651-657), so the window is the stream's last W bytes at their ring positions.
        OneRow row(input_size, output_size);
        BatchTables t = row.tables(input, output);
        t.in_consumed = nullptr, t.dict = conf->use_custom_dictionary ? window_state : nullptr;
        rc = batch_compress(conf, t, row.ilen, TAMP_AMD_MEM_HOST, device, nullptr);
        if (rc != TAMP_OK) return (tamp_res)rc;
        if (output_written_size) *output_written_size = row.olen;
        const int8_t st1 = row.status;
        if (st1 == TAMP_OK) {
            const size_t first = input_size > W ? input_size - W : 0;
            for (size_t p2 = first; p2 < input_size; p2++) window_state[p2 & (W - 1)] = input[p2];
            *window_pos = (uint16_t)(input_size & (W - 1));
            if (carry) std::memset(carry, 0, sizeof *carry);
        }
        return st1;
    }
    if ((uint64_t)prefix.size() + (uint64_t)input_size > 0xFFFFFFFFull) return TAMP_AMD_BAD_ARGUMENT;  // (32-bit stream lengths)
    // ONE stream on the host-memory pipeline, the prefix in front of the input, the state slot its state row.  A piece that
    // did not complete leaves window and carry as they came in, so its bytes must not count either: a caller that consumed
    // them and offered the piece again would emit them twice (drop_failed).  (A finishing call keeps the reference's
    // contract -- what fitted is delivered with TAMP_OUTPUT_FULL, compressor.c:65-75.)
    OneRow row(prefix.size() + input_size, output_size);
    const uint32_t ilen = row.ilen;
    HostBatch b{row.tables(input, output)};
    b.in = input, b.out = output;  // (as given: the lead bytes count in in_len[0], the input itself may be empty)
    b.in_consumed = nullptr;
    b.dict = !resume && conf->use_custom_dictionary ? window_state : nullptr;  // (a fresh stream with a custom dictionary: window_state holds it)
    b.states = stbuf.data(), b.state_stride = stbuf.size(), b.lead = prefix.data(), b.nlead = prefix.size();
    b.exact_out = true, b.drop_failed = !finish;
    std::vector<HostChunk> one;
    plan_host_chunks(b, 1, 0, ~0ull, one);
    rc = run_host_batch(ctx, device, b, one, W, [&](const BatchTables& d, uint8_t* d_state, hipStream_t cs) {
        return launch_compress(ctx, conf, d, ilen ? ilen : 16, cs, &seg, d_state);
    });
    if (rc != TAMP_OK) return (tamp_res)rc;
    const uint32_t olen = row.olen;
    const int8_t status = row.status;
    if (output_written_size) *output_written_size = olen;
    if (status == TAMP_OK) {
        std::memcpy(window_state, stbuf.data(), W);
        *window_pos = (uint16_t)get(kSlotWindowPos, 2);
        if (token_written) *token_written = (int)get(kSlotToken, 1);
        if (cached_len) *cached_pos = 0, *cached_len = 0;
        if (carry) {
            std::memset(carry, 0, sizeof *carry);
            if (!finish) {
                if (cached_len) *cached_len = (uint8_t)get(kSlotLazyLen, 1), *cached_pos = (uint16_t)(*cached_len ? get(kSlotLazyPos, 2) : 0);
                carry->rle_count = (uint8_t)get(kSlotRle, 1), carry->ext_count = (uint8_t)get(kSlotExtCount, 1);
                carry->bit_count = (uint8_t)get(kSlotNbits, 1), carry->ext_pos = (uint16_t)get(kSlotExtPos, 2);
                carry->bits = get(kSlotBits, 4);
                const uint32_t parsed = get(kSlotParsed, 4);
                // <= 16.  The ring is full when the call's last poll consumed nothing (a run or an extended match that
                // could not grow emits its token without taking a byte, compressor.c:449-466,505-509): the reference's
                // call ends there all the same (:700-720)
                const uint32_t left = ilen - parsed;
                if (parsed > ilen || left > 16) return TAMP_ERROR;
                carry->tail_len = (uint8_t)left;
                for (uint32_t j = 0; j < left; j++) {
                    const size_t at = (size_t)parsed + j;
                    carry->tail[j] = at < prefix.size() ? prefix[at] : input[at - prefix.size()];
                }
            }
        }
    } else if (!finish && status == TAMP_OUTPUT_FULL) {
        return TAMP_OUTPUT_FULL;  // (the carry is left as it came in: give the piece tamp_amd_compress_bound(input_size + 271) of room)
    }
    return status;
}
}  // namespace

tamp_res tamp_amd_compress_segment(const TampAmdConf* conf, int emit_header, int append_marker, int resume,
                                   int flush_token, unsigned char* window_state, uint16_t* window_pos,
                                   unsigned char* output, size_t output_size, size_t* output_written_size,
                                   const unsigned char* input, size_t input_size, int* token_written, int device) {
    return segment_core(conf, emit_header, append_marker, resume, 1, flush_token, window_state, window_pos, nullptr, output,
                        output_size, output_written_size, input, input_size, token_written, device);
}

tamp_res tamp_amd_compress_piece(const TampAmdConf* conf, int emit_header, int append_marker, int resume, int finish,
                                 int flush_token, unsigned char* window_state, uint16_t* window_pos, TampAmdCarry* carry,
                                 unsigned char* output, size_t output_size, size_t* output_written_size,
                                 const unsigned char* input, size_t input_size, int* token_written, int device) {
    if (!carry) return TAMP_AMD_BAD_ARGUMENT;
    return segment_core(conf, emit_header, append_marker, resume, finish, flush_token, window_state, window_pos, carry, output,
                        output_size, output_written_size, input, input_size, token_written, device);
}

tamp_res tamp_amd_compress_piece_lazy(const TampAmdConf* conf, int emit_header, int append_marker, int resume, int finish,
                                      int flush_token, unsigned char* window_state, uint16_t* window_pos, TampAmdLazyCarry* carry,
                                      unsigned char* output, size_t output_size, size_t* output_written_size,
                                      const unsigned char* input, size_t input_size, int* token_written, int device) {
    if (output_written_size) *output_written_size = 0;
    if (token_written) *token_written = 0;
    if (!carry) return TAMP_AMD_BAD_ARGUMENT;
    return segment_core(conf, emit_header, append_marker, resume, finish, flush_token, window_state, window_pos, &carry->carry,
                        output, output_size, output_written_size, input, input_size, token_written, device, &carry->cached_pos,
                        &carry->cached_len);
}

}  // extern "C"
