"""Byte ranges of streams WITHOUT dictionary resets through a seek index, against the ways there were before: dev tool.

Workload: the ragged 2,000-stream prose batch of tools/batch_resets_bench.py (lengths log-uniform in 8 KiB .. 4 MiB, seed 2026),
compressed at window 10, literal 8, extended format WITHOUT resets.  1,000 random 4 KiB ranges (seed 7), each inside its stream.
Per interval N (16 KiB and 64 KiB):
  build, device          build_seek_index of the resident batch (the size query and the index launch); the index's bytes
  read, device           read_ranges_seek, everything resident: the wait for the unit count is inside the span
  read, host             read_ranges_seek through the host-memory call: planning on the host, touched rows and spans uploaded
  decode + slice         what the parent commit can do: decompress_batch of the WHOLE resident batch, then 1,000 slices (torch)
  read_ranges (resets)   the same data compressed with reset_interval=N and its index: read_ranges, everything resident
Timed with torch events on the current stream around each call and with the wall clock around the same span, the device drained
at both ends; median of the last `--reps - 2` of `--reps` calls (default 7), all in one process.  Every row checks its bytes
against slices of the input (SHA-256 over all ranges).

    python tools/seek_index_bench.py [--out profiles/seek_index_bench.txt] [--streams 2000] [--reps 7]
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
RANGES, RANGE_LEN, RANGE_SEED = 1000, 4 << 10, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--intervals", default="16384,65536")
    args = ap.parse_args()

    import numpy as np
    import torch

    import batch_resets_bench as brb
    import tamp_amd

    assert torch.cuda.is_available(), "a measurement needs the GPU: no fallback"
    brb.STREAMS = args.streams
    flat, in_off, in_len = brb.workload()
    n, total = len(in_len), int(flat.size)
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, reps=args.reps):
        ms, wall, res = [], [], None
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            res = fn()
            e1.record()
            e1.synchronize()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(e0.elapsed_time(e1))
        skip = 2 if reps >= 4 else 0
        med = lambda v: sorted(v[skip:])[(len(v) - skip) // 2]  # noqa: E731
        return med(ms), med(wall), res

    rng = np.random.default_rng(RANGE_SEED)
    r_stream = rng.integers(0, n, RANGES).astype(np.uint32)
    r_begin = np.array([rng.integers(0, max(int(in_len[i]) - RANGE_LEN, 1)) for i in r_stream], dtype=np.uint64)
    r_len = np.minimum(np.full(RANGES, RANGE_LEN, dtype=np.uint64), in_len[r_stream].astype(np.uint64) - r_begin).astype(np.uint32)
    want = hashlib.sha256()
    for i, b, k in zip(r_stream, r_begin, r_len):
        o = int(in_off[i]) + int(b)
        want.update(flat[o : o + int(k)].tobytes())
    want = want.hexdigest()

    def digest(res):
        out = res.out.cpu().numpy() if hasattr(res.out, "cpu") else res.out
        off = res.out_off.cpu().numpy() if hasattr(res.out_off, "cpu") else res.out_off
        got = res.out_len.cpu().numpy() if hasattr(res.out_len, "cpu") else res.out_len
        status = res.status.cpu().numpy() if hasattr(res.status, "cpu") else res.status
        assert (status == 0).all(), status[status != 0][:8]
        h = hashlib.sha256()
        for q in range(RANGES):
            h.update(out[int(off[q]) : int(off[q]) + (int(got[q]) & 0xFFFFFFFF)].tobytes())
        return h.hexdigest()

    t_flat = torch.from_numpy(flat).to(dev)
    t_off, t_len = torch.from_numpy(in_off.view(np.int64)).to(dev), torch.from_numpy(in_len.view(np.int32)).to(dev)
    say(f"# seek index bench: {n} streams, {total} bytes, {RANGES} ranges of {RANGE_LEN} bytes; {torch.cuda.get_device_name(0)}")
    say(f"# median of the last {max(args.reps - 2, 1)} of {args.reps} calls; ms = device events, wall = host clock, same span")

    plain = tamp_amd.compress_batch(t_flat, t_off, t_len, window=10, literal=8, extended=True)
    torch.cuda.synchronize()
    assert (plain.status.cpu().numpy() == 0).all()
    packed = plain.packed()
    c_flat, c_off, c_len = packed.triple()
    torch.cuda.synchronize()
    comp_bytes = int(c_len.to(torch.int64).sum().item())
    host_streams = packed.cpu()
    h_flat, h_off, h_len = host_streams.triple()
    say(f"compressed without resets: {comp_bytes} bytes (ratio {total / comp_bytes:.3f})")

    cap = torch.from_numpy((in_len.astype(np.int64) + 1).astype(np.int32)).to(dev)
    rs_t, rb_t = torch.from_numpy(r_stream.astype(np.int64)).to(dev), torch.from_numpy(r_begin.view(np.int64)).to(dev)

    def decode_and_slice():
        back = tamp_amd.decompress_batch(c_flat, c_off, c_len, out_cap=cap, max_window_bits=10)
        base = back.out_off.to(torch.int64)[rs_t] + rb_t
        idx = base[:, None] + torch.arange(RANGE_LEN, device=dev)[None, :]
        return back, back.out[torch.clamp(idx, max=back.out.numel() - 1)]

    ms, wall, (back, rows) = timed(decode_and_slice)
    h = hashlib.sha256()
    rows = rows.cpu().numpy()
    for q in range(RANGES):
        h.update(rows[q, : int(r_len[q])].tobytes())
    assert h.hexdigest() == want, "decode + slice: other bytes"
    del back
    say(json.dumps(dict(row="decode + slice, device", ms=round(ms, 3), wall_ms=round(wall, 3), decoded_bytes=total)))

    for N in [int(x) for x in args.intervals.split(",")]:
        ms, wall, index = timed(lambda: tamp_amd.build_seek_index(c_flat, c_off, c_len, interval=N, max_window_bits=10), reps=max(args.reps - 2, 3))
        assert (index.size.cpu().numpy() == in_len.astype(np.int64)).all(), "the index: other sizes"
        say(json.dumps(dict(row="build, device", interval=N, ms=round(ms, 3), wall_ms=round(wall, 3), rows=int(index.first[-1].item()),
                            index_bytes=index.nbytes, share_of_decoded=round(index.nbytes / total, 4))))
        ms, wall, res = timed(lambda: tamp_amd.read_ranges_seek(c_flat, c_off, c_len, seek_index=index, stream_index=r_stream, begin=r_begin,
                                                                length=r_len))
        assert digest(res) == want, "read, device: other bytes"
        say(json.dumps(dict(row="read, device", interval=N, ms=round(ms, 3), wall_ms=round(wall, 3))))
        h_index = index.to("cpu")
        ms, wall, res = timed(lambda: tamp_amd.read_ranges_seek(h_flat, h_off, h_len, seek_index=h_index, stream_index=r_stream, begin=r_begin,
                                                                length=r_len))
        assert digest(res) == want, "read, host: other bytes"
        say(json.dumps(dict(row="read, host", interval=N, ms=round(ms, 3), wall_ms=round(wall, 3))))
        del index, h_index
        withr = tamp_amd.compress_batch(t_flat, t_off, t_len, window=10, literal=8, extended=True, dictionary_reset=True, reset_interval=N, reset_index=True)
        torch.cuda.synchronize()
        assert (withr.status.cpu().numpy() == 0).all()
        r_bytes = int(withr.out_len.to(torch.int64).sum().item())
        ms, wall, res = timed(lambda: tamp_amd.read_ranges(withr.out, withr.out_off, withr.out_len, reset_index=withr.reset_index,
                                                           stream_index=r_stream, begin=r_begin, length=r_len, max_window_bits=10))
        assert digest(res) == want, "read_ranges: other bytes"
        say(json.dumps(dict(row="read_ranges (resets), device", interval=N, ms=round(ms, 3), wall_ms=round(wall, 3), compressed_bytes=r_bytes,
                            ratio=round(total / r_bytes, 3))))
        del withr
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
