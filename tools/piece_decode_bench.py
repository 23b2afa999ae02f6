"""Reading back the streams of many streaming compressors: DecompressorBatch (objects on the device, tamp_batch_decoded_size_pieces +
tamp_batch_decompress_pieces) next to DecoderBatch (objects on the host, tamp_batch_decompress_resume through host memory), on the
two shapes of profiles/piece_batch_bench.txt:

  telemetry  65,536 streams x 256 B per round, window 2^8, every write finished with a FLUSH token
  prose      4,096 streams x 4 KiB per round, window 2^10, unfinished pieces, frozen prose corpus

The compressed rounds are made once with tamp_batch_compress_pieces and stay on the device: (out, out_off, out_len) of a round is
what a CompressorBatch result holds.  Every path has decoder objects of its own and decodes the same bytes from the same states.
Per round, wall clock around the call with the device idle before and after (a `read` waits for the slab total itself):

  read           DecompressorBatch.read(out, out_off, out_len): size query, one sync for the total, decode
  read, out_cap  the same with out_cap = message size + 1: one decode launch, nothing read back
  size query     tamp_batch_decoded_size_pieces alone        (events around the call, on the objects of `read, out_cap`)
  decode launch  tamp_batch_decompress_pieces alone          (events around the call, objects of its own)
  5 % active     read() of a round in which one stream in twenty received its next message (objects of their own: stream i takes
                 part in the rounds r with (i + r) % 20 == 0)
  DecoderBatch   DecoderBatch.step on the same bytes as host chunks (making the chunks from the device result is not timed)

A checkout that has no DecompressorBatch (the parent commit of the change that added it) runs the DecoderBatch line alone: the
comparison the committed file records is that run, made in the same session, appended to this one's.
Writes profiles/piece_decode_bench.txt (or argv[1]).  usage: python tools/piece_decode_bench.py [out] [timed rounds = 20]   (GPU box)"""
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
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "piece_decode_bench.txt")
TIMED = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARM = 2
ROUNDS = WARM + TIMED
HAVE = hasattr(tamp_amd, "DecompressorBatch")
lib = _lib.load()
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def p(a):
    return C.c_void_p(a.data_ptr())


def shape_telemetry():
    n, size = 65536, 256
    rows = wl.telemetry(n * ROUNDS, size).reshape(n, ROUNDS, size)  # stream i: messages i*ROUNDS .. of the generator, in order
    return dict(name="telemetry", n=n, size=size, window=8, finish=True, rounds=[np.ascontiguousarray(rows[:, r]) for r in range(ROUNDS)],
                what="every write finished with a FLUSH token")


def shape_prose():
    n, size = 4096, 4096
    prose = np.frombuffer(wl.frozen_corpus("prose"), dtype=np.uint8)
    span = ROUNDS * size
    starts = (np.arange(n, dtype=np.int64) * 7919 * 97) % (len(prose) - span)  # every stream: one contiguous region of the corpus
    rounds = [np.stack([prose[s + r * size : s + (r + 1) * size] for s in starts]) for r in range(ROUNDS)]
    return dict(name="prose", n=n, size=size, window=10, finish=False, rounds=rounds, what="unfinished pieces")


def compress_rounds(shape):
    """-> per round (out uint8, out_len int32) on the device, and the common out_off int64 (slabs of the piece bound)."""
    n, size, W = shape["n"], shape["size"], 1 << shape["window"]
    conf = _lib.TampAmdConf(shape["window"], 8, 0, 1, 0, 0)
    cap = int(lib.tamp_amd_compress_bound(size + 271, 8, 0))
    objs = torch.zeros((n, 48 + W), dtype=torch.uint8, device=dev)
    in_off = torch.arange(n, dtype=torch.int64, device=dev) * size
    in_len = torch.full((n,), size, dtype=torch.int32, device=dev)
    out_off = torch.arange(n, dtype=torch.int64, device=dev) * cap
    out_cap = torch.full((n,), cap, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    made = []
    for r in range(ROUNDS):
        op = (HEADER if r == 0 else RESUME) | ((FINISH | TOKEN) if shape["finish"] else 0)
        ops = torch.full((n,), op, dtype=torch.uint8, device=dev)
        data = torch.from_numpy(shape["rounds"][r].reshape(-1)).to(dev)
        out = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
        out_len = torch.zeros(n, dtype=torch.int32, device=dev)
        rc = lib.tamp_batch_compress_pieces(C.byref(conf), p(objs), 48 + W, p(ops), p(data), p(in_off), p(in_len), p(out), p(out_off), p(out_cap),
                                            p(out_len), p(status), n, size, _lib.MEM_DEVICE, 0, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert not status.any()
        made.append((out, out_len))
    return made, out_off


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def events(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def med(xs):
    xs = xs[WARM:]
    return f"{float(np.median(xs)):9.3f} ms   (min {min(xs):.3f}, max {max(xs):.3f}, {len(xs)} rounds)"


def run_shape(shape):
    n, size, bits = shape["n"], shape["size"], shape["window"]
    made, c_off = compress_rounds(shape)
    comp_bytes = [int(ln.sum().item()) for _, ln in made]
    say(f"== {shape['name']}: {n} streams x {size} B per round, window 2^{bits}, {shape['what']} ==")
    say(f"  compressed bytes per round: first {comp_bytes[0]}, median {int(np.median(comp_bytes))} ({np.median(comp_bytes) / (n * size):.4f} of the plain bytes)")
    plain_total = n * size

    def check(res, r, who):
        # (finished pieces decode to the round's plain bytes; unfinished ones hold back up to a token's worth)
        got = int(res.out_len.sum().item())
        assert bool((res.status == 2).all()), who
        assert got == plain_total if shape["finish"] else abs(got - plain_total) <= n * 300, (who, got)

    if HAVE:
        t = dict(read=[], cap=[], query=[], launch=[], sparse=[], sparse_streams=[])
        d_read, d_cap, d_sparse = (tamp_amd.DecompressorBatch(n, window_bits=bits) for _ in range(3))
        raw = tamp_amd.DecompressorBatch(n, window_bits=bits).objects
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        flat_all = torch.cat([out for out, _ in made])
        base = np.arange(ROUNDS, dtype=np.int64) * int(made[0][0].numel())
        off_h, lens_all = c_off.cpu().numpy(), np.stack([ln.cpu().numpy() for _, ln in made])
        seen = np.zeros(n, dtype=np.int64)  # messages stream i of d_sparse has received
        room = size + 1 if shape["finish"] else size + 300
        l_off = torch.arange(n, dtype=torch.int64, device=dev) * room
        l_cap = torch.full((n,), room, dtype=torch.int32, device=dev)
        l_out = torch.empty(n * room, dtype=torch.uint8, device=dev)
        l_len, l_status, l_used = (torch.zeros(n, dtype=dt, device=dev) for dt in (torch.int32, torch.int8, torch.int32))
        for r, (out, ln) in enumerate(made):
            ms, res = wall(lambda: d_read.read(out, c_off, ln))
            t["read"].append(ms)
            check(res, r, "read")
            ms, rc = events(lambda: lib.tamp_batch_decoded_size_pieces(p(d_cap.objects), d_cap.stride, bits, None, p(out), p(c_off), p(ln), None,
                                                                     p(l_len), p(l_status), p(l_used), n, 0, st))
            assert rc == 0
            t["query"].append(ms)
            ms, res = wall(lambda: d_cap.read(out, c_off, ln, out_cap=room))
            t["cap"].append(ms)
            check(res, r, "read with out_cap")
            ms, rc = events(lambda: lib.tamp_batch_decompress_pieces(p(raw), d_cap.stride, bits, None, p(out), p(c_off), p(ln), p(l_out), p(l_off),
                                                                   p(l_cap), p(l_len), p(l_status), p(l_used), n, 0, st))
            assert rc == 0 and bool((l_status == 2).all())
            t["launch"].append(ms)
            active = (np.arange(n) + r) % 20 == 0
            k = np.minimum(seen, ROUNDS - 1)  # the message each stream receives next
            s_len = np.where(active, lens_all[k, np.arange(n)], 0).astype(np.int32)
            s_off = (base[k] + off_h).astype(np.int64)
            s_len_t, s_off_t = torch.from_numpy(s_len).to(dev), torch.from_numpy(s_off).to(dev)
            ms, res = wall(lambda: d_sparse.read(flat_all, s_off_t, s_len_t))
            t["sparse"].append(ms)
            t["sparse_streams"].append(int(active.sum()))
            assert bool(((res.status == 2) == torch.from_numpy(active).to(dev)).all())
            seen += active
        say(f"  DecompressorBatch.read (size query + sync + decode)   {med(t['read'])}")
        say(f"  DecompressorBatch.read, out_cap given (one launch)    {med(t['cap'])}")
        say(f"  size query alone (events)                             {med(t['query'])}")
        say(f"  decode launch alone (events)                          {med(t['launch'])}")
        say(f"  read, 5 % of the streams active ({int(np.median(t['sparse_streams']))} of {n})           {med(t['sparse'])}")
        q, full = float(np.median(t["query"][WARM:])), float(np.median(t["read"][WARM:]))
        say(f"  the size query is {100 * q / full:.0f} % of a read; a 5 %-active read costs {100 * float(np.median(t['sparse'][WARM:])) / full:.0f} % of a full one")
        del d_read, d_cap, d_sparse, raw, flat_all, l_out
    # DecoderBatch: objects on the host, host chunks
    dec = tamp_amd.DecoderBatch(n, window_bits=bits)
    t_step = []
    room = size + 1 if shape["finish"] else size + 300
    for r, (out, ln) in enumerate(made):
        out_h, len_h, off_h = out.cpu().numpy(), ln.cpu().numpy(), c_off.cpu().numpy()
        chunks = [out_h[int(off_h[i]) : int(off_h[i]) + int(len_h[i])] for i in range(n)]
        t0 = time.perf_counter()
        status, outs, consumed = dec.step(chunks, room)
        t_step.append((time.perf_counter() - t0) * 1e3)
        assert (status == 2).all() and (consumed == len_h).all()
    say(f"  DecoderBatch.step (host objects, host chunks)         {med(t_step)}")
    if HAVE:
        say(f"  DecoderBatch.step / DecompressorBatch.read = {float(np.median(t_step[WARM:])) / full:.1f}x")
    say()


def main():
    say(f"piece_decode_bench: {torch.cuda.get_device_name(0)}, {'DecompressorBatch and DecoderBatch' if HAVE else 'DecoderBatch alone (no DecompressorBatch in this checkout)'};")
    say(f"ms per round, median of {TIMED} rounds after {WARM} warm-up rounds")
    say()
    for make in (shape_telemetry, shape_prose):
        run_shape(make())
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
