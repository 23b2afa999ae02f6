"""Extending a seek index when its streams have grown, against building it again: dev tool.

Workload: the ragged 2,000-stream prose batch of tools/batch_resets_bench.py (lengths log-uniform in 8 KiB .. 4 MiB, seed 2026),
written WITHOUT resets by one CompressorBatch connection per stream (window 10, literal 8, extended format) and flushed, so that
what a later write adds continues the same stream: the old bytes are a prefix of the grown ones.  Interval N = 16 KiB.
  case 1   4 KiB of source appended to 1,000 random streams (seed 7)
  case 2   64 KiB appended to all streams (behind case 1)
Per case:
  build, device      build_seek_index of the grown resident batch: the only answer there was
  extend, device     SeekIndex.extend of the index of the batch before the case, everything resident
  sizing, device     of which: the first of its two calls alone (the copy of the rows it works on, the launch with room = have)
  build, host        build_seek_index through the host-memory call (one call, wall clock)
  extend, host       SeekIndex.extend through the host-memory call
and how many rows the extension decoded again (rows behind the restart rows that the index already held) and how many are new.
Timed with torch events on the current stream around each call and with the wall clock around the same span, the device drained
at both ends; median of the last `--reps - 2` of `--reps` calls (default 5), all in one process.  Every extended index is compared
with the build of the same batch, table by table.

    python tools/seek_extend_bench.py [--out profiles/seek_extend_bench.txt] [--streams 2000] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
INTERVAL, WINDOW, PICK_SEED = 16 << 10, 10, 7
CASES = (("4 KiB appended to 1,000 streams", 1000, 4 << 10), ("64 KiB appended to all streams", None, 64 << 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    import batch_resets_bench as brb
    import tamp_amd
    from tamp_amd import _lib
    from tamp_amd.batch import _ptr, pack_streams

    assert torch.cuda.is_available(), "a measurement needs the GPU: no fallback"
    brb.STREAMS = args.streams
    flat, in_off, in_len = brb.workload()
    n, total = len(in_len), int(flat.size)
    dev = torch.device("cuda:0")
    lib = _lib.load()
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

    def host(t):
        return np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t)

    def same(a, b, what):
        for f in ("first", "in_pos", "state", "size", "status"):
            x, y = host(getattr(a, f)), host(getattr(b, f))
            assert x.shape == y.shape and np.array_equal(x.astype(np.int64), y.astype(np.int64)), (what, f)

    say(f"# seek extend bench: {n} streams, {total} source bytes, interval {INTERVAL}, window {WINDOW}; {torch.cuda.get_device_name(0)}")
    say(f"# median of the last {max(args.reps - 2, 1)} of {args.reps} calls; ms = device events, wall = host clock, same span")

    conn = tamp_amd.CompressorBatch(n, window=WINDOW)

    def write(source, off, length):
        """One round of the connection -> the bytes it added to every stream (a write and a flush with its token)."""
        w = conn.write(torch.from_numpy(source).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(length.astype(np.int32)).to(dev))
        f = conn.flush()
        torch.cuda.synchronize()
        parts = []
        for res in (w, f):
            assert (host(res.status) == 0).all()
            out, o, k = host(res.out), host(res.out_off).astype(np.int64), host(res.out_len).astype(np.int64) & 0xFFFFFFFF
            parts.append([out[int(o[i]) : int(o[i]) + int(k[i])].tobytes() for i in range(n)])
        return [a + b for a, b in zip(*parts)]

    streams = write(flat, in_off, in_len)
    sizes = in_len.astype(np.int64)
    say(f"written without resets: {sum(len(s) for s in streams)} bytes (ratio {total / sum(len(s) for s in streams):.3f})")

    def resident(blobs):
        f, o, k = pack_streams(blobs)
        f, o, k = np.array(f), np.array(o), np.array(k)  # (writable copies: torch takes no read-only array)
        return (torch.from_numpy(f).to(dev), torch.from_numpy(o.view(np.int64)).to(dev), torch.from_numpy(k.view(np.int32)).to(dev)), (f, o, k)

    d_now, h_now = resident(streams)
    index = tamp_amd.build_seek_index(*d_now, interval=INTERVAL, max_window_bits=WINDOW)
    torch.cuda.synchronize()
    assert (host(index.size) == sizes).all(), "the index: other sizes"
    h_index = index.to("cpu")

    rng = np.random.default_rng(PICK_SEED)
    for name, count, grow in CASES:
        pick = np.arange(n) if count is None else np.sort(rng.choice(n, min(count, n), replace=False))
        add_len = np.zeros(n, dtype=np.uint32)
        add_len[pick] = grow
        add_off = np.zeros(n, dtype=np.uint64)
        add_off[1:] = np.cumsum(add_len.astype(np.uint64))[:-1]
        source = flat[1000 : 1000 + int(add_len.astype(np.uint64).sum())].copy()  # (prose again, from another place)
        more = write(source, add_off, add_len)
        streams = [a + b for a, b in zip(streams, more)]
        sizes = sizes + add_len.astype(np.int64)
        d_now, h_now = resident(streams)
        say(f"## {name}: {int(add_len.astype(np.uint64).sum())} source bytes, {sum(len(m) for m in more)} compressed bytes added")

        ms, wall, built = timed(lambda: tamp_amd.build_seek_index(*d_now, interval=INTERVAL, max_window_bits=WINDOW), reps=max(args.reps - 2, 3))
        assert (host(built.size) == sizes).all(), "the build: other sizes"
        say(json.dumps(dict(row="build, device", ms=round(ms, 3), wall_ms=round(wall, 3), rows=int(built.first[-1].item()))))
        build_ms = ms
        ms, wall, grown = timed(lambda: index.extend(*d_now))
        same(grown, built, "extend, device")
        say(json.dumps(dict(row="extend, device", ms=round(ms, 3), wall_ms=round(wall, 3), of_build=round(ms / build_ms, 4))))
        extend_ms = ms

        # the sizing call alone, as extend_seek_index makes it
        old_first = index.first.to(torch.int64)
        have = (old_first[1:] - old_first[:-1]).to(torch.int32)
        stride = 16 + (1 << WINDOW)
        size_t, status_t = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int8, device=dev)

        def sizing():
            in_pos1, state1 = index.in_pos.clone(), index.state.clone()
            _lib.check_launch(lib.tamp_batch_seek_index_extend(
                None, 0, WINDOW, _ptr(d_now[0]), _ptr(d_now[1]), _ptr(d_now[2]), INTERVAL, _ptr(old_first), _ptr(have), _ptr(in_pos1),
                _ptr(state1), stride, _ptr(size_t), _ptr(status_t), n, _lib.MEM_DEVICE, 0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            return in_pos1, state1

        ms, wall, _ = timed(sizing)
        assert (host(size_t) == sizes).all(), "the sizing call: other sizes"
        say(json.dumps(dict(row="sizing, device", ms=round(ms, 3), wall_ms=round(wall, 3), share_of_extend=round(ms / extend_ms, 3))))

        t0 = time.perf_counter()
        h_built = tamp_amd.build_seek_index(*h_now, interval=INTERVAL, max_window_bits=WINDOW)
        say(json.dumps(dict(row="build, host", wall_ms=round((time.perf_counter() - t0) * 1e3, 3), calls=1)))
        ms, wall, h_grown = timed(lambda: h_index.extend(*h_now))
        same(h_grown, h_built, "extend, host")
        say(json.dumps(dict(row="extend, host", ms=round(ms, 3), wall_ms=round(wall, 3))))

        # rows decoded again (the index held them, behind the restart rows) and rows that are new
        first0, in_pos0, first1 = host(h_index.first).astype(np.int64), host(h_index.in_pos).astype(np.int64), host(h_grown.first).astype(np.int64)
        again = fresh = from_header = 0
        for i in range(n):
            rows = in_pos0[first0[i] : first0[i + 1]]
            final = 0
            if len(rows) >= 2:
                lower = np.flatnonzero(rows[:-1] < rows[-1])
                final = int(lower[-1]) + 1 if len(lower) else 0
            again += len(rows) - final
            from_header += final == 0
            fresh += int(first1[i + 1] - first1[i]) - len(rows)
        say(json.dumps(dict(row="rows", held=int(first0[-1]), decoded_again=int(again), new=int(fresh), streams_from_their_header=int(from_header))))
        index, h_index = grown, h_grown
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
