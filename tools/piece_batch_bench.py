"""Batch piece calls against what the library had before them: N streaming compressors advanced per launch
(tamp_batch_compress_pieces) on the two shapes the call is for, next to (a) a loop of the single piece call, (b) the resume
kernel (EncoderBatch) and (c) compress_batch of the same bytes as independent streams -- the ceiling for speed, and the
comparison for size: what streaming buys is the ratio of compressed bytes.

  prose      4,096 objects x 4 KiB per round x 16 rounds, window 2^10, unfinished pieces, frozen prose corpus
  telemetry  65,536 objects x 256 B per round x 16 rounds, window 2^8, every write finished with a FLUSH token

Per shape and round: the new call from device memory (torch events around the call, and where its time goes from the library's
own events: tamp_amd_pieces_phase_ms), the new call from host memory (wall clock around the call, which returns complete),
(a) over a subset of the objects, scaled to all of them, (b) and (c).  One warm-up round of every path on objects of its own;
the timed rounds then run on fresh objects, so every path compresses the same bytes from the same states.
Writes profiles/piece_batch_bench.txt (or argv[1]).  usage: python tools/piece_batch_bench.py [out] [rounds = 16]   (GPU box)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import tamp_amd  # noqa: E402
from tamp_amd import _lib, workloads as wl  # noqa: E402

HEADER, RESUME, FINISH, TOKEN = 1, 4, 8, 16
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "piece_batch_bench.txt")
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 16
lib = _lib.load()
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def shape_prose():
    n, size = 4096, 4096
    prose = np.frombuffer(wl.frozen_corpus("prose"), dtype=np.uint8)
    span = ROUNDS * size
    starts = (np.arange(n, dtype=np.int64) * 7919 * 97) % (len(prose) - span)  # every stream: one contiguous region of the corpus
    rounds = [np.stack([prose[s + r * size : s + (r + 1) * size] for s in starts]) for r in range(ROUNDS)]
    return dict(name="prose", n=n, size=size, window=10, finish=False, rounds=rounds, subset=64)


def shape_telemetry():
    n, size = 65536, 256
    rows = wl.telemetry(n * ROUNDS, size).reshape(n, ROUNDS, size)  # stream i: messages i*ROUNDS .. of the generator, in order
    return dict(name="telemetry", n=n, size=size, window=8, finish=True, rounds=[np.ascontiguousarray(rows[:, r]) for r in range(ROUNDS)], subset=256)


def p(a):
    return C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a.ctypes.data_as(C.c_void_p)


def op_of(shape, r):
    return (HEADER if r == 0 else RESUME) | ((FINISH | TOKEN) if shape["finish"] else 0)


def median(xs):
    return float(np.median(xs)) if len(xs) else float("nan")


def run_new(shape, mem, rounds):
    """-> (ms per round, compressed bytes per round, phase ms per round)"""
    n, size, W = shape["n"], shape["size"], 1 << shape["window"]
    conf = _lib.TampAmdConf(shape["window"], 8, 0, 1, 0, 0)
    stride = 48 + W
    cap = int(lib.tamp_amd_compress_bound(size + 271, 8, 0))
    host = dict(objs=np.zeros((n, stride), np.uint8), in_off=np.arange(n, dtype=np.uint64) * size, in_len=np.full(n, size, np.uint32),
                out=np.zeros(n * cap, np.uint8), out_off=np.arange(n, dtype=np.uint64) * cap, out_cap=np.full(n, cap, np.uint32),
                out_len=np.zeros(n, np.uint32), status=np.zeros(n, np.int8))
    if mem == _lib.MEM_DEVICE:
        t = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else (v.view(np.int32) if v.dtype == np.uint32 else v)).to(dev)
             for k, v in host.items()}
    else:
        t = host
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if mem == _lib.MEM_DEVICE else None
    ms, sizes, phases = [], [], []
    lib.tamp_amd_set_timing(1 if mem == _lib.MEM_DEVICE else 0)
    for r in rounds:
        ops = np.full(n, op_of(shape, r), np.uint8)
        data = shape["rounds"][r].reshape(-1)
        if mem == _lib.MEM_DEVICE:
            ops, data = torch.from_numpy(ops).to(dev), torch.from_numpy(data).to(dev)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        t0 = time.perf_counter()
        rc = lib.tamp_batch_compress_pieces(C.byref(conf), p(t["objs"]), stride, p(ops), p(data), p(t["in_off"]), p(t["in_len"]), p(t["out"]),
                                            p(t["out_off"]), p(t["out_cap"]), p(t["out_len"]), p(t["status"]), n, size, mem, 0, st)
        assert rc == 0, rc
        if mem == _lib.MEM_DEVICE:
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            ph = (C.c_float * 4)()
            lib.tamp_amd_pieces_phase_ms(C.byref(ph))
            phases.append(list(ph))
            status, out_len = t["status"].cpu().numpy(), t["out_len"].cpu().numpy()
        else:
            ms.append((time.perf_counter() - t0) * 1e3)
            status, out_len = t["status"], t["out_len"]
        assert (status == 0).all()
        sizes.append(int(out_len.astype(np.int64).sum()))
    lib.tamp_amd_set_timing(0)
    return ms, sizes, phases


def run_single_loop(shape, rounds):
    """(a): tamp_amd_compress_piece_lazy per object, over a subset; -> ms per round scaled to all objects"""
    n, size, W, k = shape["n"], shape["size"], 1 << shape["window"], shape["subset"]
    conf = _lib.TampAmdConf(shape["window"], 8, 0, 1, 0, 0)
    cap = int(lib.tamp_amd_compress_bound(size + 271, 8, 0))
    wins = [(C.c_ubyte * W)() for _ in range(k)]
    wps = [C.c_uint16(0) for _ in range(k)]
    carries = [_lib.TampAmdLazyCarry() for _ in range(k)]
    out = (C.c_ubyte * cap)()
    written, token = C.c_size_t(0), C.c_int(0)
    ms = []
    for r in rounds:
        op = op_of(shape, r)
        rows = shape["rounds"][r]
        t0 = time.perf_counter()
        for i in range(k):
            res = lib.tamp_amd_compress_piece_lazy(C.byref(conf), int(bool(op & HEADER)), 0, int(bool(op & RESUME)), int(bool(op & FINISH)),
                                                   int(bool(op & TOKEN)), wins[i], C.byref(wps[i]), C.byref(carries[i]), out, cap,
                                                   C.byref(written), p(rows[i]), size, C.byref(token), 0)
            assert res == 0, res
        ms.append((time.perf_counter() - t0) * 1e3 * n / k)
    return ms


def run_encoder_batch(shape, rounds):
    """(b): EncoderBatch.compress / compress_and_flush (host-memory objects, as that class keeps them); -> ms per round, bytes"""
    n, size = shape["n"], shape["size"]
    enc = tamp_amd.EncoderBatch(n, window=shape["window"])
    cap = int(lib.tamp_amd_compress_bound(size + 271, 8, 0))
    ms, sizes = [], []
    for r in rounds:
        chunks = [row.tobytes() for row in shape["rounds"][r]]
        t0 = time.perf_counter()
        if shape["finish"]:
            status, outs, _ = enc.compress_and_flush(chunks, cap, write_token=True)
        else:
            status, outs, _ = enc.compress(chunks, cap)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert (status >= 0).all()
        sizes.append(sum(len(o) for o in outs))
    return ms, sizes


def run_independent(shape, rounds):
    """(c): compress_batch of the same bytes as independent streams, device memory; -> ms per round (call, kernel), bytes"""
    n, size = shape["n"], shape["size"]
    off = torch.arange(n, dtype=torch.int64, device=dev) * size
    length = torch.full((n,), size, dtype=torch.int32, device=dev)
    ms, kernel, sizes = [], [], []
    for r in rounds:
        data = torch.from_numpy(shape["rounds"][r].reshape(-1)).to(dev)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = tamp_amd.compress_batch(data, off, length, window=shape["window"], max_in_len=size, timing=True)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        kernel.append(res.kernel_ms)
        assert (res.status.cpu().numpy() == 0).all()
        sizes.append(int(res.out_len.to(torch.int64).sum().item()))
    return ms, kernel, sizes


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"piece_batch_bench: {torch.cuda.get_device_name(0)}, {ROUNDS} rounds per shape; times in ms per round (median over the timed rounds;")
    say("first / last round beside it where they differ), every path warmed by one round on objects of its own")
    for make in (shape_prose, shape_telemetry):
        shape = make()
        n, size = shape["n"], shape["size"]
        say()
        say(f"== {shape['name']}: {n} objects x {size} B per round, window 2^{shape['window']}, "
            f"{'every write finished with a FLUSH token' if shape['finish'] else 'unfinished pieces'} ==")
        all_rounds = list(range(ROUNDS))
        for mem in (_lib.MEM_DEVICE, _lib.MEM_HOST):
            run_new(shape, mem, [0])
        run_single_loop(shape, [0]), run_independent(shape, [0])
        dev_ms, dev_sizes, phases = run_new(shape, _lib.MEM_DEVICE, all_rounds)
        host_ms, host_sizes, _ = run_new(shape, _lib.MEM_HOST, all_rounds)
        assert dev_sizes == host_sizes
        few = all_rounds[: min(ROUNDS, 4)]
        a_ms = run_single_loop(shape, few)
        run_encoder_batch(shape, [0])
        b_ms, b_sizes = run_encoder_batch(shape, few)
        c_ms, c_kernel, c_sizes = run_independent(shape, all_rounds)
        mb = n * size / 1e6
        row = lambda name, xs, note="": say(f"  {name:<58} {median(xs):10.3f} ms  {mb / median(xs) * 1e3:10.1f} MB/s   first {xs[0]:.3f}  last {xs[-1]:.3f}  {note}")  # noqa: E731
        row("new call, device memory (events around the call)", dev_ms)
        ph = np.array(phases)
        say(f"      of which: classify + the wait {median(ph[:, 0]):.3f}, stage {median(ph[:, 1]):.3f}, compress launches {median(ph[:, 2]):.3f}, "
            f"unstage {median(ph[:, 3]):.3f}  (library events; medians)")
        row("new call, host memory (wall clock, copies included)", host_ms)
        row(f"(a) loop of the single piece call ({shape['subset']} objects, scaled to {n})", a_ms, f"rounds 0..{len(few) - 1}")
        row("(b) EncoderBatch (resume kernel, host-memory objects)", b_ms, f"rounds 0..{len(few) - 1}")
        row("(c) compress_batch, independent streams, device memory", c_ms)
        row("(c) ... its kernel alone (library events)", c_kernel)
        total_in = n * size * ROUNDS
        say(f"  compressed bytes over {ROUNDS} rounds: streaming {sum(dev_sizes)} ({sum(dev_sizes) / total_in:.4f} of the input), "
            f"independent {sum(c_sizes)} ({sum(c_sizes) / total_in:.4f}); streaming / independent = {sum(dev_sizes) / sum(c_sizes):.4f}")
        say(f"  per round, streaming / independent: " + " ".join(f"{s / c:.3f}" for s, c in zip(dev_sizes, c_sizes)))
        if b_sizes[: len(few)] != dev_sizes[: len(few)]:
            say(f"  (EncoderBatch delivers whole tokens per call, the piece call whole bytes: {b_sizes} vs {dev_sizes[:len(few)]} bytes per round)")
        new, a, b, c = median(dev_ms), median(a_ms), median(b_ms), median(c_ms)
        say(f"  new call vs (a): {a / new:.1f}x faster;  vs (b): {b / new:.1f}x {'faster' if b > new else 'SLOWER'};  "
            f"vs (c), the ceiling: {new / c:.2f}x its time ({new - c:+.3f} ms per round)")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
