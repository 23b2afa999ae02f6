// tamp_seek.hpp -- tamp_batch_seek_index, tamp_batch_seek_index_extend and tamp_batch_read_ranges_seek behind their entry points (included by tamp_capi.hip,
// which owns the device context, the per-stream scratch records and the host pipeline).  The kernels: tamp_seek_kernel.hpp.
//
// The index, device memory: one launch on the caller's stream, nothing allocated, nothing read back.  Host memory: the streams'
// extent, the tables and the dictionary go up on the host pipeline's first stream, and the sizes, the statuses and exactly the rows
// each stream wrote come back.  The extension is the same launch with the table of rows held; from host memory the restart rows are
// found and checked on the host, and only they and the compressed bytes behind them go up.
// The read, device memory, under the stream's scratch record's launch lock:
//   count  ->  ONE wait for the 8-byte unit count  ->  units  ->  decode  ->  gather
// Everything behind the wait is asynchronous.  Host memory: count and units run on the host (the same two functions), and what goes
// up is the unit table, each touched row once and each unit's compressed span -- never a whole stream unless a unit spans it.
#pragma once
#include <unordered_map>

namespace {

struct SeekIndexCall {  // the entry point's arguments
    const uint8_t* dict;
    size_t dict_len;
    uint8_t max_wbits;
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    uint32_t interval;
    const uint64_t* first;
    uint32_t* ckpt_in;
    uint8_t* states;
    size_t stride;
    uint64_t* decoded_size;
    int8_t* status;
    size_t n;
};

SeekIndexArgs seek_index_args(const DeviceCtx* ctx, const SeekIndexCall& c) {
    SeekIndexArgs a;
    a.in = c.in, a.in_off = c.in_off, a.in_len = c.in_len;
    a.dict = c.dict, a.dict_len = c.dict ? c.dict_len : 0, a.seed_dicts = ctx->seed_dicts;
    a.ckpt_first = c.first, a.ckpt_in = c.ckpt_in, a.ckpt_state = c.states, a.state_stride = c.stride;
    a.decoded_size = c.decoded_size, a.status = c.status;
    a.interval = c.interval, a.max_wbits = c.max_wbits, a.n_streams = (uint32_t)c.n;
    return a;
}

int launch_seek_index(DeviceCtx* ctx, const SeekIndexCall& c, hipStream_t st) {
    if (c.n == 0) return TAMP_OK;
    const SeekIndexArgs a = seek_index_args(ctx, c);
    const WaveGeometry g = wave_geometry(c.max_wbits, c.n, ctx->cu_count);
    timing_begin(st);
    const int rc = launch_waves(tamp_seek_index_kernel, a, g, seek_wave_lds(c.max_wbits, g.waves), st);
    timing_end(st);
    if (rc != TAMP_OK) return rc;
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// The extension: the same geometry, the loop entered at each stream's restart row.  `staged`: what a host-memory call adds
// (SeekExtendArgs); null for a device-memory call, whose wavefronts find the restart rows themselves.
struct SeekStaged {
    const uint32_t *in_base, *slot;
    const uint8_t* restart_state;
};
int launch_seek_extend(DeviceCtx* ctx, const SeekIndexCall& c, const uint32_t* have, const SeekStaged* staged, hipStream_t st) {
    if (c.n == 0) return TAMP_OK;
    SeekExtendArgs e;
    e.x = seek_index_args(ctx, c);
    e.have = have;
    e.in_base = staged ? staged->in_base : nullptr, e.slot = staged ? staged->slot : nullptr;
    e.restart_state = staged ? staged->restart_state : nullptr;
    const WaveGeometry g = wave_geometry(c.max_wbits, c.n, ctx->cu_count);
    timing_begin(st);
    const int rc = launch_waves(tamp_seek_extend_kernel, e, g, seek_wave_lds(c.max_wbits, g.waves), st);
    timing_end(st);
    if (rc != TAMP_OK) return rc;
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

int seek_index_host(DeviceCtx* ctx, const SeekIndexCall& c) {
    const size_t n = c.n;
    for (size_t i = 0; i < n; i++)
        if (c.first[i + 1] < c.first[i]) return TAMP_AMD_BAD_ARGUMENT;  // (no running sum: the rows cannot be placed)
    const uint64_t rows = c.first[n] - c.first[0];
    const HostExtent ext(c.in_off, c.in_len, n);
    std::vector<uint64_t> h_first(n + 1);
    for (size_t i = 0; i <= n; i++) h_first[i] = c.first[i] - c.first[0];
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    TableCarver m, o;  // the caller's tables in `meta`, the results in `out`
    const auto m_in_off = m.take<uint64_t>(n), m_first = m.take<uint64_t>(n + 1);
    const auto m_in_len = m.take<uint32_t>(n);
    const auto o_ckpt_in = o.take<uint32_t>(rows);
    const auto o_size = o.take<uint64_t>(n);
    const auto o_status = o.take<int8_t>(n);
    HIP_OK(P.in[0].need(ext.bytes() + 64));
    HIP_OK(P.meta[0].need(m.bytes()));
    HIP_OK(P.out[0].need(o.bytes()));
    HIP_OK(P.state[0].need(rows * c.stride + 64));
    if (c.dict && c.dict_len) HIP_OK(P.dict.need(std::min(c.dict_len, kSeedTable)));
    void *const mp = P.meta[0].p, *const op = P.out[0].p;
    SeekIndexCall d = c;
    d.dict = c.dict && c.dict_len ? static_cast<const uint8_t*>(P.dict.p) : nullptr, d.dict_len = std::min(c.dict_len, kSeedTable);
    d.in = static_cast<const uint8_t*>(P.in[0].p), d.in_off = m_in_off.in(mp), d.first = m_first.in(mp), d.in_len = m_in_len.in(mp);
    d.ckpt_in = o_ckpt_in.in(op), d.states = static_cast<uint8_t*>(P.state[0].p);
    d.decoded_size = o_size.in(op), d.status = o_status.in(op);
    if (ext.bytes()) HIP_OK(hipMemcpyAsync(P.in[0].p, c.in + ext.lo, ext.bytes(), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_in_off.in(mp), ext.off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_first.in(mp), h_first.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_in_len.in(mp), c.in_len, n * 4, hipMemcpyHostToDevice, st));
    if (c.dict && c.dict_len) HIP_OK(hipMemcpyAsync(P.dict.p, c.dict, std::min(c.dict_len, kSeedTable), hipMemcpyHostToDevice, st));
    if (const int rc = launch_seek_index(ctx, d, st)) return rc;
    HIP_OK(hipMemcpyAsync(c.decoded_size, d.decoded_size, n * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(c.status, d.status, n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    // the rows each stream wrote, runs of neighbours in one transfer
    uint64_t run0 = 0, run1 = 0;
    auto flush = [&]() -> int {
        if (run1 > run0) {
            HIP_OK(hipMemcpyAsync(c.states + (c.first[0] + run0) * c.stride, d.states + run0 * c.stride, (run1 - run0) * c.stride, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(c.ckpt_in + c.first[0] + run0, d.ckpt_in + run0, (run1 - run0) * 4, hipMemcpyDeviceToHost, st));
        }
        return TAMP_OK;
    };
    for (size_t i = 0; i < n; i++) {
        const uint64_t S = c.decoded_size[i], C = S ? (S - 1) / c.interval : 0;
        const uint64_t w = std::min(C, h_first[i + 1] - h_first[i]);
        if (!w) continue;
        if (h_first[i] != run1) {
            if (const int frc = flush()) return frc;
            run0 = h_first[i];
        }
        run1 = h_first[i] + w;
    }
    if (const int frc = flush()) return frc;
    HIP_OK(hipStreamSynchronize(st));
    return TAMP_OK;
}

// The extension from host memory.  The rule and the restart row's checks run here (the kernel's own functions), so that what goes
// up is, per stream, its restart row and its compressed bytes from that row's in_pos on -- the whole stream only where it restarts
// from its header -- and what comes back is the rows behind the restart row and the two result tables.
int seek_extend_host(DeviceCtx* ctx, const SeekIndexCall& c, const uint32_t* have) {
    const size_t n = c.n;
    for (size_t i = 0; i < n; i++)
        if (c.first[i + 1] < c.first[i]) return TAMP_AMD_BAD_ARGUMENT;  // (no running sum: the rows cannot be placed)
    std::vector<uint64_t> d_first(n + 1, 0), d_in_off(n, 0);
    std::vector<uint32_t> d_have(n, 0), d_in_base(n, 0), d_slot(n, 0);
    std::vector<uint8_t> spans, restart_rows;
    for (size_t i = 0; i < n; i++) {
        const uint64_t room = c.first[i + 1] - c.first[i];
        const uint32_t len = c.in_len[i];
        const uint8_t* const src = c.in + c.in_off[i];
        const uint32_t hs = len ? 1u + (src[0] & 1u) : 1u;
        uint32_t fin = 0, up = len < kSeekMaxIn ? len : 0;  // final rows; bytes of the stream the kernel may come to read
        if (have[i] > room) {
            fin = kSeekBadRestart;
        } else if (have[i] && len && len < kSeekMaxIn && len >= hs && !(hs == 2 && src[1])) {  // (else: the kernel reports the stream as the build does)
            fin = seek_restart_rows(c.ckpt_in + c.first[i], have[i], len);
            if (fin && fin != kSeekBadRestart && !seek_row_holds(c.ckpt_in, c.states, c.stride, c.first[i] + fin - 1, fin - 1, len, hs, src[0]))
                fin = kSeekBadRestart;
        }
        uint32_t base = 0;
        if (fin == kSeekBadRestart) {
            up = std::min(up, 2u);  // (its header: the stream's other verdicts come first)
        } else if (fin) {
            const uint64_t row = c.first[i] + fin - 1;
            base = c.ckpt_in[row];
            d_slot[i] = (uint32_t)(restart_rows.size() / c.stride);
            restart_rows.insert(restart_rows.end(), c.states + row * c.stride, c.states + (row + 1) * c.stride);
        }
        d_have[i] = fin, d_in_base[i] = base;
        d_in_off[i] = spans.size();
        if (up > base) spans.insert(spans.end(), src + base, src + up);
        spans.resize((spans.size() + 3) & ~(size_t)3);
        d_first[i + 1] = d_first[i] + (fin == kSeekBadRestart ? 0 : room - fin);
    }
    const uint64_t rows = d_first[n];
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    TableCarver m, o;  // the staged tables in `meta`, the results in `out`
    const auto m_in_off = m.take<uint64_t>(n), m_first = m.take<uint64_t>(n + 1);
    const auto m_in_len = m.take<uint32_t>(n), m_have = m.take<uint32_t>(n), m_in_base = m.take<uint32_t>(n), m_slot = m.take<uint32_t>(n);
    const auto o_ckpt_in = o.take<uint32_t>(rows);
    const auto o_size = o.take<uint64_t>(n);
    const auto o_status = o.take<int8_t>(n);
    HIP_OK(P.in[0].need(spans.size() + 64));
    HIP_OK(P.meta[0].need(m.bytes()));
    HIP_OK(P.out[0].need(o.bytes()));
    HIP_OK(P.state[0].need(rows * c.stride + 64));
    HIP_OK(P.state[1].need(restart_rows.size() + c.stride + 64));
    if (c.dict && c.dict_len) HIP_OK(P.dict.need(std::min(c.dict_len, kSeedTable)));
    void *const mp = P.meta[0].p, *const op = P.out[0].p;
    SeekIndexCall d = c;
    d.dict = c.dict && c.dict_len ? static_cast<const uint8_t*>(P.dict.p) : nullptr, d.dict_len = std::min(c.dict_len, kSeedTable);
    d.in = static_cast<const uint8_t*>(P.in[0].p), d.in_off = m_in_off.in(mp), d.first = m_first.in(mp), d.in_len = m_in_len.in(mp);
    d.ckpt_in = o_ckpt_in.in(op), d.states = static_cast<uint8_t*>(P.state[0].p);
    d.decoded_size = o_size.in(op), d.status = o_status.in(op);
    if (!spans.empty()) HIP_OK(hipMemcpyAsync(P.in[0].p, spans.data(), spans.size(), hipMemcpyHostToDevice, st));
    if (!restart_rows.empty()) HIP_OK(hipMemcpyAsync(P.state[1].p, restart_rows.data(), restart_rows.size(), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_in_off.in(mp), d_in_off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_first.in(mp), d_first.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_in_len.in(mp), c.in_len, n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_have.in(mp), d_have.data(), n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_in_base.in(mp), d_in_base.data(), n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_slot.in(mp), d_slot.data(), n * 4, hipMemcpyHostToDevice, st));
    if (c.dict && c.dict_len) HIP_OK(hipMemcpyAsync(P.dict.p, c.dict, std::min(c.dict_len, kSeedTable), hipMemcpyHostToDevice, st));
    const SeekStaged staged = {m_in_base.in(mp), m_slot.in(mp), static_cast<const uint8_t*>(P.state[1].p)};
    if (const int rc = launch_seek_extend(ctx, d, m_have.in(mp), &staged, st)) return rc;
    HIP_OK(hipMemcpyAsync(c.decoded_size, d.decoded_size, n * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(c.status, d.status, n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    // the rows each stream wrote, those behind its restart row: runs of neighbours on the device in one transfer each into a packed
    // staging table, then every stream's rows to their place behind its final ones
    std::vector<uint64_t> wrote(n, 0);
    uint64_t staged_rows = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t fin = d_have[i];
        if (fin == kSeekBadRestart) continue;
        const uint64_t S = c.decoded_size[i], C = S ? (S - 1) / c.interval : 0;
        const uint64_t upto = std::min(C, c.first[i + 1] - c.first[i]);
        if (upto > fin) wrote[i] = upto - fin, staged_rows += wrote[i];
    }
    std::vector<uint8_t> back_state(staged_rows * c.stride);
    std::vector<uint32_t> back_in(staged_rows);
    uint64_t run0 = 0, run1 = 0, stage0 = 0, stage_at = 0;
    auto flush = [&]() -> int {
        if (run1 > run0) {
            HIP_OK(hipMemcpyAsync(back_state.data() + stage0 * c.stride, d.states + run0 * c.stride, (run1 - run0) * c.stride, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(back_in.data() + stage0, d.ckpt_in + run0, (run1 - run0) * 4, hipMemcpyDeviceToHost, st));
        }
        return TAMP_OK;
    };
    for (size_t i = 0; i < n; i++) {
        if (!wrote[i]) continue;
        if (d_first[i] != run1) {
            if (const int frc = flush()) return frc;
            run0 = d_first[i], stage0 = stage_at;
        }
        run1 = d_first[i] + wrote[i], stage_at += wrote[i];
    }
    if (const int frc = flush()) return frc;
    HIP_OK(hipStreamSynchronize(st));
    stage_at = 0;
    for (size_t i = 0; i < n; i++) {
        if (!wrote[i]) continue;
        const uint64_t at = c.first[i] + d_have[i];
        memcpy(c.states + at * c.stride, back_state.data() + stage_at * c.stride, wrote[i] * c.stride);
        memcpy(c.ckpt_in + at, back_in.data() + stage_at, wrote[i] * 4);
        stage_at += wrote[i];
    }
    if (getenv("TAMP_AMD_RESETS_DEBUG"))
        fprintf(stderr, "[tamp_amd seek] extend (host): %llu streams, %llu restart rows and %llu bytes of spans uploaded\n",
                (unsigned long long)n, (unsigned long long)(restart_rows.size() / c.stride), (unsigned long long)spans.size());
    return TAMP_OK;
}

struct SeekReadOut {
    uint8_t* out;
    const uint64_t* out_off;
    uint32_t* out_len;
    int8_t* status;
};

ReadSeekArgs read_seek_args(const DeviceCtx* ctx, const SeekCaller& c, const uint8_t* dict, const SeekUnit* units, uint64_t U,
                            const SeekRanges& r, const SeekReadOut& o) {
    ReadSeekArgs a;
    a.in = c.in, a.dict = dict, a.dict_len = dict ? c.dict_len : 0, a.seed_dicts = ctx->seed_dicts;
    a.states = c.states, a.stride = c.stride, a.units = units, a.U = U, a.got = r.got, a.flags = r.flags;
    a.out = o.out, a.out_off = o.out_off, a.max_wbits = c.max_wbits;
    return a;
}

// Units are claimed by stride over a grid of at most cu_count * 64 workgroups, as the wave-per-stream kernels are launched.
int launch_read_seek_kernel(DeviceCtx* ctx, const ReadSeekArgs& a, hipStream_t st) {
    const WaveGeometry g = wave_geometry(a.max_wbits, a.U, ctx->cu_count);
    return launch_waves(tamp_read_seek_kernel, a, g, seek_wave_lds(a.max_wbits, g.waves), st);
}

int launch_read_seek(DeviceCtx* ctx, const SeekCaller& c, const uint8_t* dict, const SeekReadOut& o, hipStream_t st) {
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    const uint64_t nr = c.n_ranges;
    const size_t got_at = (nr + 1) * 8, flags_at = got_at + nr * 4, verdict_at = flags_at + nr * 4;
    HIP_OK(rec.seek.need(verdict_at + nr + 64));
    uint8_t* const sb = static_cast<uint8_t*>(rec.seek.p);
    const SeekRanges r = {reinterpret_cast<uint64_t*>(sb), reinterpret_cast<uint32_t*>(sb + got_at), reinterpret_cast<uint32_t*>(sb + flags_at),
                          reinterpret_cast<int8_t*>(sb + verdict_at)};
    const CallTiming call_timing(st);
    const SeekCountArgs ca = {c, r};
    hipLaunchKernelGGL(tamp_seek_count_kernel, dim3(1), dim3(kResetScanTile), 0, st, ca);
    HIP_OK(hipGetLastError());
    uint64_t U = 0;
    HIP_OK(hipMemcpyAsync(&U, r.unit_first + nr, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (U > 0xFFFFFFFFull * 255) return TAMP_AMD_BAD_ARGUMENT;  // (the grid of the lane-per-unit step)
    if (U) {
        HIP_OK(rec.seek_units.need(U * sizeof(SeekUnit)));
        SeekUnit* const units = static_cast<SeekUnit*>(rec.seek_units.p);
        const SeekUnitsArgs ua = {c, r, units, U};
        hipLaunchKernelGGL(tamp_seek_units_kernel, dim3((uint32_t)((U + 255) / 256)), dim3(256), 0, st, ua);
        HIP_OK(hipGetLastError());
        if (const int rc = launch_read_seek_kernel(ctx, read_seek_args(ctx, c, dict, units, U, r, o), st)) return rc;
        HIP_OK(hipGetLastError());
    }
    const SeekGatherArgs ga = {r, c.range_len, nr, o.out_len, o.status};
    hipLaunchKernelGGL(tamp_seek_gather_kernel, dim3((uint32_t)((nr + 255) / 256)), dim3(256), 0, st, ga);
    HIP_OK(hipGetLastError());
    if (getenv("TAMP_AMD_RESETS_DEBUG"))
        fprintf(stderr, "[tamp_amd seek] read ranges: %llu ranges, %llu units\n", (unsigned long long)nr, (unsigned long long)U);
    return TAMP_OK;
}

int read_seek_host(DeviceCtx* ctx, const SeekCaller& c, const uint8_t* dict, const SeekReadOut& o) {
    const uint64_t nr = c.n_ranges;
    // count and units, on the host
    std::vector<SeekUnit> units;
    std::vector<uint8_t> spans, rows;
    std::vector<uint64_t> d_out_off(nr, 0);
    std::vector<int32_t> verdict(nr);
    std::unordered_map<uint32_t, uint32_t> row_at;  // a touched row -> its place among the uploaded ones
    uint64_t out_bytes = 0;
    for (uint64_t q = 0; q < nr; q++) {
        const SeekPlan p = seek_range_plan(c, q);
        verdict[q] = p.verdict;
        if (p.verdict != kSeekGo) continue;
        const size_t u0 = units.size();
        bool ok = true;
        for (uint64_t j = 0; ok && j < p.units; j++) {
            SeekUnit u;
            ok = seek_range_unit(c, q, p, j, u);
            if (ok) units.push_back(u);
        }
        if (!ok) {  // (a range with a bad row has no units and writes nothing)
            units.resize(u0);
            verdict[q] = kSeekBadIndex;
            continue;
        }
        d_out_off[q] = out_bytes;
        out_bytes += (c.range_len[q] + 3ull) & ~3ull;
    }
    for (SeekUnit& u : units) {  // the touched rows, once each, and the units' spans
        if (u.row != kSeekFresh) {
            const auto it = row_at.find(u.row);
            if (it != row_at.end()) {
                u.row = it->second;
            } else {
                const uint32_t at = (uint32_t)row_at.size();
                const uint8_t* const src = c.states + (uint64_t)u.row * c.stride;
                rows.insert(rows.end(), src, src + c.stride);
                row_at.emplace(u.row, at);
                u.row = at;
            }
        }
        const uint64_t at = spans.size();
        spans.insert(spans.end(), c.in + u.in_at, c.in + u.in_at + u.in_n);
        spans.resize((spans.size() + 3) & ~(size_t)3);
        u.in_at = at;
    }
    const uint64_t U = units.size();
    std::vector<uint32_t> got(nr, 0), flags(nr, 0);
    std::vector<uint8_t> h_out(out_bytes);
    if (U) {
        HostCall host(ctx);
        if (const int rc = host.open()) return rc;
        DeviceCtx::HostPipe& P = host.P;
        const hipStream_t st = host.st;
        TableCarver m, o;  // the units and where the ranges land in `meta`; the ranges' bytes, then got and flags as one table, in `out`
        const auto m_units = m.take<SeekUnit>(U);
        const auto m_out_off = m.take<uint64_t>(nr);
        const auto o_out = o.take<uint8_t>(out_bytes);
        const auto o_got = o.take<uint32_t>(2 * nr, 8);
        HIP_OK(P.in[0].need(spans.size() + 64));
        HIP_OK(P.state[0].need(rows.size() + 64));
        HIP_OK(P.meta[0].need(m.bytes()));
        HIP_OK(P.out[0].need(o.bytes()));
        const size_t dl = dict && c.dict_len ? std::min<size_t>(c.dict_len, kSeedTable) : 0;
        if (dl) HIP_OK(P.dict.need(dl));
        void *const mp = P.meta[0].p, *const op = P.out[0].p;
        uint32_t *const d_got = o_got.in(op), *const d_flags = d_got + nr;
        if (!spans.empty()) HIP_OK(hipMemcpyAsync(P.in[0].p, spans.data(), spans.size(), hipMemcpyHostToDevice, st));
        if (!rows.empty()) HIP_OK(hipMemcpyAsync(P.state[0].p, rows.data(), rows.size(), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_units.in(mp), units.data(), U * sizeof(SeekUnit), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_out_off.in(mp), d_out_off.data(), nr * 8, hipMemcpyHostToDevice, st));
        if (dl) HIP_OK(hipMemcpyAsync(P.dict.p, dict, dl, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(d_got, 0, nr * 8, st));
        SeekCaller d = c;
        d.in = static_cast<const uint8_t*>(P.in[0].p), d.states = static_cast<const uint8_t*>(P.state[0].p), d.dict_len = dl;
        const SeekRanges r = {nullptr, d_got, d_flags, nullptr};
        const SeekReadOut dout = {o_out.in(op), m_out_off.in(mp), nullptr, nullptr};
        if (const int rc = launch_read_seek_kernel(ctx, read_seek_args(ctx, d, dl ? static_cast<const uint8_t*>(P.dict.p) : nullptr, m_units.in(mp), U, r, dout), st))
            return rc;
        HIP_OK(hipGetLastError());
        if (out_bytes) HIP_OK(hipMemcpyAsync(h_out.data(), o_out.in(op), out_bytes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(got.data(), d_got, nr * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(flags.data(), d_flags, nr * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    for (uint64_t q = 0; q < nr; q++) {  // the gather step
        int32_t status = verdict[q];
        uint32_t len = 0;
        if (status == kSeekGo) {
            len = std::min(got[q], c.range_len[q]);
            status = (flags[q] & kSeekSawOob) ? (int32_t)kOob : (len == c.range_len[q] ? (int32_t)kOk : (int32_t)kInputExhausted);
            if (len) memcpy(o.out + o.out_off[q], h_out.data() + d_out_off[q], len);
        }
        o.status[q] = (int8_t)status, o.out_len[q] = len;
    }
    if (getenv("TAMP_AMD_RESETS_DEBUG"))
        fprintf(stderr, "[tamp_amd seek] read ranges (host): %llu ranges, %llu units, %llu rows and %llu bytes of spans uploaded\n",
                (unsigned long long)nr, (unsigned long long)U, (unsigned long long)row_at.size(), (unsigned long long)spans.size());
    return TAMP_OK;
}

}  // namespace
