// tamp_pieces.hpp -- tamp_batch_compress_pieces behind its entry point (included by tamp_capi.hip, which owns the device
// context, the per-stream scratch records and the compress launcher).  The kernels: tamp_pieces_kernel.hpp.
//
// Device memory, on the caller's stream, under its scratch record's launch lock:
//   classify  ->  ONE wait for the 88-byte record (objects and longest row per class, bytes of input rows)
//             ->  stage  ->  one compress launch per class that occurs  ->  unstage
// Everything behind the wait is asynchronous.  Staging traffic per object and call: the window once each way, the input once.
// Host memory: objects, ops, tables and the input extent go to the host pipeline's kept buffers on its first stream, the
// device path runs there, and the result rows, the objects and exactly out_len[i] bytes per slab come back.
#pragma once

namespace {

constexpr size_t kPieceObjectHeader = sizeof(TampAmdPieceObject);
static_assert(kPieceObjectHeader == 48 && kPieceObjectHeader == kObjHeader, "TampAmdPieceObject: 48 bytes in front of the window");
static_assert(offsetof(TampAmdPieceObject, window_pos) == kObjWindowPos && offsetof(TampAmdPieceObject, token_written) == kObjToken,
              "TampAmdPieceObject: the offsets the kernels use");
static_assert(offsetof(TampAmdLazyCarry, cached_pos) == kObjLazyPos && offsetof(TampAmdLazyCarry, cached_len) == kObjLazyLen &&
              offsetof(TampAmdCarry, bits) == kObjBits && offsetof(TampAmdCarry, tail) == kObjTail &&
              offsetof(TampAmdCarry, bit_count) == kObjNbits && offsetof(TampAmdCarry, tail_len) == kObjTailLen,
              "TampAmdLazyCarry: the offsets the kernels use");
static_assert(TAMP_AMD_PIECE_HEADER == kOpHeader && TAMP_AMD_PIECE_APPEND_MARKER == kOpAppend && TAMP_AMD_PIECE_RESUME == kOpResume &&
              TAMP_AMD_PIECE_FINISH == kOpFinish && TAMP_AMD_PIECE_FLUSH_TOKEN == kOpToken && TAMP_AMD_PIECE_SKIP == kOpSkip,
              "TAMP_AMD_PIECE_*: the bits the kernels test");

// tamp_amd_pieces_phase_ms: with timing on (tamp_amd_set_timing), events of the calling thread's last device-memory call --
// before the classify kernel, behind the wait, behind the stage kernel, behind the last compress launch, behind unstage.
// (Like t_ev0 / t_ev1 of the timing hook: made by the thread's first timed call on the device current then, and kept for the
// thread's life -- five events per thread that ever timed a call, never destroyed.)
thread_local hipEvent_t t_piece_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
thread_local bool t_piece_ev_valid = false;
void piece_mark(int k, hipStream_t st) {
    if (!t_timing) return;
    if (!t_piece_ev[k] && hipEventCreate(&t_piece_ev[k]) != hipSuccess) return;
    (void)hipEventRecord(t_piece_ev[k], st);
    if (k == 4) t_piece_ev_valid = true;
}

struct PieceCall {  // the entry point's arguments; every pointer in device memory by the time launch_pieces sees it
    void* objects;
    size_t stride;
    const uint8_t* ops;
    BatchTables t;
};

int launch_pieces(DeviceCtx* ctx, const TampAmdConf* conf, const PieceCall& c, hipStream_t st) {
    const size_t n = c.t.n;
    if (n == 0) return TAMP_OK;
    StreamScratch& rec = ctx->scratch(st);
    std::lock_guard<std::mutex> call_lock(rec.mu);  // (to the last launch of the call: the lock rule above StreamScratch)
    const size_t W = (size_t)1 << conf->window;
    auto up = [](size_t v, size_t a) { return (v + a - 1) / a * a; };
    // per object: record, row_off (8), rank (4), class (1); per row behind them: in_off, out_off (8), in_len, out_cap, out_len (4), status (1)
    const size_t o_row_off = up(sizeof(PieceRecord), 16), o_rank = o_row_off + n * 8, o_cls = o_rank + n * 4;
    const size_t o_g_in_off = up(o_cls + n, 16), o_g_out_off = o_g_in_off + n * 8, o_g_in_len = o_g_out_off + n * 8;
    const size_t o_g_out_cap = o_g_in_len + n * 4, o_g_out_len = o_g_out_cap + n * 4, o_g_status = o_g_out_len + n * 4;
    HIP_OK(rec.pieces.need(o_g_status + n));
    uint8_t* const m = static_cast<uint8_t*>(rec.pieces.p);
    PieceArgs a = {};
    a.objects = static_cast<uint8_t*>(c.objects), a.stride = c.stride, a.ops = c.ops;
    a.in = c.t.in, a.in_off = c.t.in_off, a.in_len = c.t.in_len;
    a.out = c.t.out, a.out_off = c.t.out_off, a.out_cap = c.t.out_cap, a.out_len = c.t.out_len, a.status = c.t.status;
    a.n = (uint32_t)n, a.wbits = conf->window, a.lazy = conf->lazy_matching != 0, a.custom_dict = conf->use_custom_dictionary != 0;
    const int lit = conf->extended ? conf->literal : 8;  // compressor.c:224-225, as fill_compress_args
    a.seed = ctx->seed_dicts + (lit <= 5 ? 0 : (lit == 6 ? 1 : 2)) * kSeedTable;
    a.rec = reinterpret_cast<PieceRecord*>(m);
    a.row_off = reinterpret_cast<uint64_t*>(m + o_row_off), a.rank = reinterpret_cast<uint32_t*>(m + o_rank), a.cls = m + o_cls;
    a.g_in_off = reinterpret_cast<uint64_t*>(m + o_g_in_off), a.g_out_off = reinterpret_cast<uint64_t*>(m + o_g_out_off);
    a.g_in_len = reinterpret_cast<uint32_t*>(m + o_g_in_len), a.g_out_cap = reinterpret_cast<uint32_t*>(m + o_g_out_cap);
    a.g_out_len = reinterpret_cast<uint32_t*>(m + o_g_out_len), a.g_status = reinterpret_cast<int8_t*>(m + o_g_status);
    CallTiming timed(st);  // (one event pair around the call's kernels; the compress launches inside do not open their own)
    t_piece_ev_valid = false;
    piece_mark(0, st);
    HIP_OK(hipMemsetAsync(a.rec, 0, sizeof(PieceRecord), st));
    hipLaunchKernelGGL(tamp_pieces_classify_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, a);
    PieceRecord got;
    HIP_OK(hipMemcpyAsync(&got, a.rec, sizeof got, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));  // the call's one wait
    piece_mark(1, st);
    size_t rows = 0;
    for (uint32_t k = 0; k < kPieceClasses; k++) a.base[k] = (uint32_t)rows, rows += got.count[k];
    if (rows == 0) return TAMP_OK;  // (SKIPs, refusals and empty pieces only)
    if (rows > n) {
        snprintf(t_last_error, sizeof t_last_error, "piece classes hold %zu rows for %zu objects", rows, n);
        return TAMP_ERROR;
    }
    const size_t state_bytes = up(rows * (W + kSegStateExtra), 64);
    HIP_OK(rec.piece_rows.need(state_bytes + (size_t)got.in_bytes + 64));  // (+ 64: the kernels' vector loads may run past the last byte)
    a.rows_state = static_cast<uint8_t*>(rec.piece_rows.p), a.rows_in = a.rows_state + state_bytes;
    const uint32_t waves = (uint32_t)((n + 3) / 4);
    hipLaunchKernelGGL(tamp_pieces_stage_kernel, dim3(waves), dim3(256), 0, st, a);
    piece_mark(2, st);
    for (uint32_t k = 0; k < kPieceClasses; k++) {
        if (!got.count[k]) continue;
        const uint32_t lead = k / 3, end = k % 3;
        SegmentSpec seg;
        seg.flags = (uint8_t)(kSegSave | kSegResume | (end == 2 ? kSegFlushToken : 0) | (end == 0 ? kSegPartial : 0));
        seg.nlead = 0, seg.lead = 0;
        if (lead == 2) {  // compressor.c:227-235: FLUSH (9 bits) padded to 16 bits instead of a header
            seg.nlead = 2, seg.lead = (uint16_t)(0xABu << 7);
        } else if (lead == 1) {
            seg.nlead = conf->dictionary_reset ? 2 : 1, seg.lead = (uint16_t)(header_byte(conf, conf->dictionary_reset) << 8);
        }
        BatchTables d;
        d.in = a.rows_in, d.in_off = a.g_in_off + a.base[k], d.in_len = a.g_in_len + a.base[k];
        d.out = a.out, d.out_off = a.g_out_off + a.base[k], d.out_cap = a.g_out_cap + a.base[k];
        d.out_len = a.g_out_len + a.base[k], d.status = a.g_status + a.base[k];
        d.n = got.count[k];
        const int rc = launch_compress_locked(ctx, rec, conf, d, got.longest[k] ? got.longest[k] : 16, st, &seg,
                                              a.rows_state + (size_t)a.base[k] * (W + kSegStateExtra));
        if (rc != TAMP_OK) return rc;
    }
    piece_mark(3, st);
    hipLaunchKernelGGL(tamp_pieces_unstage_kernel, dim3(waves), dim3(256), 0, st, a);
    piece_mark(4, st);
    HIP_OK(hipGetLastError());
    return TAMP_OK;
}

// Host memory: one round trip on the host pipeline's first stream and kept buffers.
int run_host_pieces(DeviceCtx* ctx, const TampAmdConf* conf, const PieceCall& c) {
    const BatchTables& h = c.t;
    const size_t n = h.n;
    uint8_t* const objects = static_cast<uint8_t*>(c.objects);
    // The extents the live objects name.  An object the classify kernel refuses for its length (in_len > 0xFFFFFF00) takes no part:
    // it is refused alone, whatever its offsets say, and no byte of its input or slab is staged.  An object whose input or slab
    // would end beyond 2^64 names no bytes either: its staged length becomes 0xFFFFFFFF, so that it is refused the same way.
    std::vector<uint32_t> in_len_d(h.in_len, h.in_len + n);
    uint64_t in_lo = ~0ull, in_hi = 0, out_lo = ~0ull, out_hi = 0;
    for (size_t i = 0; i < n; i++) {
        if (c.ops[i] & TAMP_AMD_PIECE_SKIP) continue;
        if (h.in_off[i] + h.in_len[i] < h.in_off[i] || h.out_off[i] + h.out_cap[i] < h.out_off[i]) in_len_d[i] = 0xFFFFFFFFu;
        if (in_len_d[i] > 0xFFFFFF00u) continue;
        if (h.in_len[i]) in_lo = std::min(in_lo, h.in_off[i]), in_hi = std::max(in_hi, h.in_off[i] + h.in_len[i]);
        if (h.out_cap[i]) out_lo = std::min(out_lo, h.out_off[i]), out_hi = std::max(out_hi, h.out_off[i] + h.out_cap[i]);
    }
    if (in_hi <= in_lo) in_lo = in_hi = 0;
    if (out_hi <= out_lo) out_lo = out_hi = 0;
    if ((in_hi > in_lo && !h.in) || (out_hi > out_lo && !h.out)) return TAMP_AMD_BAD_ARGUMENT;
    std::vector<uint32_t> out_len(n);  // what comes back
    std::vector<int8_t> status(n);
    std::vector<uint8_t> objs(n * c.stride);
    std::vector<uint64_t> slab_at(n, 0);  // where a live object's slab starts on the device
    HostCall host(ctx);
    if (const int rc = host.open()) return rc;
    DeviceCtx::HostPipe& P = host.P;
    const hipStream_t st = host.st;
    TableCarver m;
    const auto m_in_off = m.take<uint64_t>(n), m_out_off = m.take<uint64_t>(n);
    const auto m_in_len = m.take<uint32_t>(n), m_out_cap = m.take<uint32_t>(n), m_out_len = m.take<uint32_t>(n);
    const auto m_status = m.take<int8_t>(n);
    const auto m_ops = m.take<uint8_t>(n, 16);
    HIP_OK(P.meta[0].need(m.bytes()));
    HIP_OK(P.state[0].need(n * c.stride));
    HIP_OK(P.in[0].need((size_t)(in_hi - in_lo) + 64));
    HIP_OK(P.out[0].need((size_t)(out_hi - out_lo) + 1));
    void* const mp = P.meta[0].p;
    uint8_t* const d_out = static_cast<uint8_t*>(P.out[0].p);
    PieceCall d = c;
    d.objects = P.state[0].p, d.ops = m_ops.in(mp);
    d.t.in = static_cast<const uint8_t*>(P.in[0].p) - in_lo, d.t.out = d_out - out_lo;
    d.t.in_off = m_in_off.in(mp), d.t.out_off = m_out_off.in(mp), d.t.in_len = m_in_len.in(mp), d.t.out_cap = m_out_cap.in(mp);
    d.t.out_len = m_out_len.in(mp), d.t.status = m_status.in(mp);
    HIP_OK(hipMemcpyAsync(m_in_off.in(mp), h.in_off, n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_out_off.in(mp), h.out_off, n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_in_len.in(mp), in_len_d.data(), n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_out_cap.in(mp), h.out_cap, n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(m_ops.in(mp), c.ops, n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(P.state[0].p, objects, n * c.stride, hipMemcpyHostToDevice, st));
    if (in_hi > in_lo) HIP_OK(hipMemcpyAsync(P.in[0].p, h.in + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, st));
    if (const int rc = launch_pieces(ctx, conf, d, st)) return rc;
    // back: the result rows and the objects of the live objects, then exactly the produced bytes
    HIP_OK(hipMemcpyAsync(out_len.data(), d.t.out_len, n * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(status.data(), d.t.status, n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(objs.data(), P.state[0].p, n * c.stride, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; i++) {
        if (c.ops[i] & TAMP_AMD_PIECE_SKIP) {
            out_len[i] = 0;  // (a skipped object brings nothing back)
            continue;
        }
        h.out_len[i] = out_len[i], h.status[i] = status[i], slab_at[i] = out_len[i] ? h.out_off[i] - out_lo : 0;
        if (status[i] == TAMP_OK) std::memcpy(objects + i * c.stride, objs.data() + i * c.stride, kPieceObjectHeader + ((size_t)1 << conf->window));
    }
    return copy_back_slabs(P, st, d_out, out_hi - out_lo, slab_at.data(), h.out, h.out_off, out_len.data(), n);
}

int batch_compress_pieces(const TampAmdConf* conf, const PieceCall& c, int mem, int device, void* stream) {
    const BatchTables& t = c.t;
    if (const int rc = batch_refused(t, true, mem, device)) return rc;
    if (device == TAMP_AMD_ALL_DEVICES) return TAMP_AMD_BAD_ARGUMENT;  // (objects stay on one device)
    if (t.n == 0) return TAMP_OK;
    if (!conf || !c.objects || !c.ops) return TAMP_AMD_BAD_ARGUMENT;
    if (!conf_valid(conf) || conf->lazy_matching > 1) return TAMP_INVALID_CONF;
    if ((c.stride & 15) || c.stride < tamp_amd_piece_object_size(conf->window) ||
        (mem == TAMP_AMD_MEM_DEVICE && (reinterpret_cast<uintptr_t>(c.objects) & 15)))
        return TAMP_AMD_BAD_ARGUMENT;
    DeviceCtx* ctx = nullptr;
    if (const int rc = get_ctx(device, &ctx)) return rc;
    if (mem == TAMP_AMD_MEM_DEVICE) return launch_pieces(ctx, conf, c, static_cast<hipStream_t>(stream));
    return run_host_pieces(ctx, conf, c);
}

}  // namespace
