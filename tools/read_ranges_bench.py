"""Random 4 KiB reads out of a ragged batch with dictionary resets against decoding all of it: dev tool.

Workload: the batch of tools/batch_resets_bench.py (the frozen prose corpus tiled into 2,000 streams, lengths log-uniform in
8 KiB .. 4 MiB, seed 2026, window 10, literal 8, extended, a reset every 64 KiB), compressed once per process with its reset index.
The load is 1,000 ranges of 4,096 bytes, their first bytes uniformly random over the bytes of the batch (seed 2026; a range that
would leave its stream is moved back inside): 2,000 of the batch's segments at most.
  ranges, device / host   tamp_batch_read_ranges: only the touched segments are staged and decoded
  whole, device / host    tamp_batch_decompress_resets of the whole batch with the same index, then the 1,000 slices (one gather)
hipEvents around each call (torch events on the default stream; host-memory calls are synchronous, so the pair spans them) and the
wall clock around the same span, the device drained at both ends; median of the last ten of twelve calls in a fresh process.  The
SHA-256 over all delivered ranges must be that of the input's slices on every row.

    python tools/read_ranges_bench.py [--out profiles/read_ranges_bench.txt] [--rounds 2]

``--grid`` measures the TABLE form (tamp_batch_read_ranges_grid) instead, into profiles/read_ranges_grid_bench.txt; the rows above are
not run and their file is not touched:
  ranges, device / host      (a) tamp_batch_read_ranges as above -- with ``--parent-lib PATH`` also on a build of the parent commit
  grid, device / host        (b) the table form on the same streams and ranges, the table made by tamp_batch_segment_ends
  ends, device / host        (c) tamp_batch_segment_ends alone
  irregular / irregularwhole     the same data re-cut at record sizes of 1 .. 128 KiB (one of eight sizes per stream, drawn log-uniformly;
                             the streams of one size are compressed by one call and the eight batches merged into one): the table
                             form against tamp_batch_decompress_resets of the merged batch with the merged index, then the slices

    python tools/read_ranges_bench.py --grid [--parent-lib tamp_amd/libtamp_amd_parent.so] [--rounds 2]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
RANGES, LENGTH, SEED, REPS = 1000, 4096, 2026, 12


def child(which, reps):
    import ctypes as C

    import numpy as np
    import torch
    from batch_resets_bench import INTERVAL, LONGEST, workload

    from tamp_amd import _lib

    lib = _lib.load()
    if os.environ.get("TAMP_AMD_BENCH_LIB"):  # (--parent-lib: another build's calls behind this tree's bindings -- it need not have every symbol)
        bound, lib = lib, C.CDLL(os.environ["TAMP_AMD_BENCH_LIB"])
        for name in ("tamp_amd_compress_resets_bound", "tamp_batch_compress_resets_index", "tamp_batch_read_ranges", "tamp_batch_decompress_resets"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = getattr(bound, name).argtypes, getattr(bound, name).restype
    kind, route = which.split("-")
    flat, in_off, in_len = workload()
    n, total = len(in_len), int(flat.size)
    if kind.startswith("irregular"):
        return irregular_child(lib, which, reps, flat, in_off, in_len)
    rng = np.random.default_rng(SEED)
    at = rng.integers(0, total, RANGES).astype(np.uint64)
    r_stream = (np.searchsorted(in_off, at, side="right") - 1).astype(np.uint32)
    r_begin = np.minimum(at - in_off[r_stream], in_len[r_stream].astype(np.uint64) - LENGTH).astype(np.uint64)
    r_len = np.full(RANGES, LENGTH, dtype=np.uint32)
    r_off = (np.arange(RANGES, dtype=np.uint64) * LENGTH).astype(np.uint64)
    source = hashlib.sha256()
    for s, b in zip(r_stream, r_begin):
        source.update(flat[int(in_off[s] + b) : int(in_off[s] + b) + LENGTH].tobytes())
    touched = int(((r_begin + np.uint64(LENGTH - 1)) // np.uint64(INTERVAL) - r_begin // np.uint64(INTERVAL) + np.uint64(1)).sum())
    conf = _lib.TampAmdConf(10, 8, 0, 1, 1, 0)
    cap = np.array([lib.tamp_amd_compress_resets_bound(int(x), INTERVAL, 8) for x in in_len], dtype=np.uint32)
    c_off = np.zeros(n, dtype=np.uint64)
    c_off[1:] = np.cumsum(cap.astype(np.uint64))[:-1]
    entries = int(((np.maximum(in_len.astype(np.uint64), 1) - 1) // INTERVAL).sum())
    room = np.minimum(in_len.astype(np.uint64) + 1, 0xFFFFFFFF).astype(np.uint32)
    d_off = np.zeros(n, dtype=np.uint64)
    d_off[1:] = np.cumsum(room.astype(np.uint64))[:-1]
    dev = torch.device("cuda:0")
    host = route == "host"
    mem = _lib.MEM_HOST if host else _lib.MEM_DEVICE
    whole = kind == "whole"
    # the table form's inputs: every closed segment INTERVAL bytes, the open one what is left
    per = (np.maximum(in_len.astype(np.uint64), 1) - 1) // INTERVAL
    closed = np.full(max(entries, 1), INTERVAL, dtype=np.uint32)
    open_size = (in_len.astype(np.uint64) - per * INTERVAL).astype(np.uint32)
    arrays = dict(closed=closed.view(np.int32), open_size=open_size.view(np.int32), ends=np.zeros(entries + n, np.int64), **dict(flat=flat, in_off=in_off.view(np.int64), in_len=in_len.view(np.int32), comp=np.zeros(int(cap.astype(np.uint64).sum()) + 1, np.uint8),
                  c_off=c_off.view(np.int64), cap=cap.view(np.int32), c_len=np.zeros(n, np.int32), c_status=np.full(n, 99, np.int8),
                  first=np.zeros(n + 1, np.int64), off=np.zeros(max(entries, 1), np.int32),
                  out=np.zeros((int(room.astype(np.uint64).sum()) if whole else RANGES * LENGTH) + 1, np.uint8),
                  d_off=d_off.view(np.int64), room=room.view(np.int32), d_len=np.zeros(n, np.int32), d_status=np.full(n, 99, np.int8),
                  used=np.zeros(n, np.int32), r_stream=r_stream.view(np.int32), r_begin=r_begin.view(np.int64), r_len=r_len.view(np.int32),
                  r_off=r_off.view(np.int64), r_out_len=np.zeros(RANGES, np.int32), r_status=np.full(RANGES, 99, np.int8)))
    held = arrays if host else {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    p = {k: C.c_void_p(v.ctypes.data if host else v.data_ptr()) for k, v in held.items()}
    rc = lib.tamp_batch_compress_resets_index(C.byref(conf), p["flat"], p["in_off"], p["in_len"], INTERVAL, p["comp"], p["c_off"], p["cap"],
                                              p["c_len"], p["c_status"], n, LONGEST, mem, 0, None, p["first"], p["off"], entries)
    torch.cuda.synchronize()
    assert rc == 0, rc
    if kind in ("grid", "ends"):
        rc = lib.tamp_batch_segment_ends(p["first"], p["closed"], p["open_size"], p["ends"], n, mem, 0, None)
        torch.cuda.synchronize()
        assert rc == 0, rc
        want = np.concatenate([np.concatenate([np.arange(1, int(e) + 1, dtype=np.uint64) * np.uint64(INTERVAL), [np.uint64(ln)]]) for e, ln in zip(per, in_len)])
        got_ends = held["ends"] if host else held["ends"].cpu().numpy()
        assert (got_ends.view(np.uint64) == want).all(), "the table is not the running sum"
    # the whole decode's slices: one gather of RANGES x LENGTH bytes out of the decoded slabs
    where = (d_off[r_stream] + r_begin)[:, None] + np.arange(LENGTH, dtype=np.uint64)[None, :]
    where = where.astype(np.int64) if host else torch.from_numpy(where.astype(np.int64)).to(dev)
    ms, wall, got = [], [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        if whole:
            rc = lib.tamp_batch_decompress_resets(15, p["comp"], p["c_off"], p["c_len"], p["first"], p["off"], p["out"], p["d_off"], p["room"],
                                                  p["d_len"], p["d_status"], p["used"], n, mem, 0, None)
            got = held["out"][where]
        elif kind == "grid":
            rc = lib.tamp_batch_read_ranges_grid(15, p["comp"], p["c_off"], p["c_len"], p["first"], p["off"], p["ends"], p["r_stream"], p["r_begin"],
                                                 p["r_len"], p["out"], p["r_off"], p["r_out_len"], p["r_status"], n, RANGES, mem, 0, None)
        elif kind == "ends":
            rc = lib.tamp_batch_segment_ends(p["first"], p["closed"], p["open_size"], p["ends"], n, mem, 0, None)
        else:
            rc = lib.tamp_batch_read_ranges(15, p["comp"], p["c_off"], p["c_len"], p["first"], p["off"], INTERVAL, p["r_stream"], p["r_begin"],
                                            p["r_len"], p["out"], p["r_off"], p["r_out_len"], p["r_status"], n, RANGES, mem, 0, None)
        e1.record()
        e1.synchronize()
        torch.cuda.synchronize()
        assert rc == 0, rc
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))
    as_np = lambda x: x if host else x.cpu().numpy()  # noqa: E731
    if whole:
        assert (as_np(held["d_status"]) == 2).all()
        delivered = as_np(got).tobytes()
    elif kind == "ends":  # (checked against numpy above; the row has no ranges)
        source = hashlib.sha256()
        delivered = b""
    else:
        assert (as_np(held["r_status"]) == 0).all() and (as_np(held["r_out_len"]) == LENGTH).all(), as_np(held["r_status"])[:16]
        delivered = as_np(held["out"])[: RANGES * LENGTH].tobytes()
    assert hashlib.sha256(delivered).hexdigest() == source.hexdigest(), "the delivered ranges are not the input's slices"
    kept, kept_wall = sorted(ms[2:]), sorted(wall[2:])
    med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2  # noqa: E731
    print(json.dumps(dict(which=which, streams=n, bytes=total, segments=entries + n, touched=touched, median_ms=med(kept), min_ms=kept[0],
                          max_ms=kept[-1], wall_ms=med(kept_wall), calls=reps, sha256=source.hexdigest())))


def irregular_child(lib, which, reps, flat, in_off, in_len):
    """The same data re-cut at record sizes of 1 .. 128 KiB: one of eight sizes per stream, the streams of one size compressed by one
    call, the eight batches merged into one (streams in the order of their size) -- a batch no single interval describes."""
    import ctypes as C

    import numpy as np
    import torch
    from batch_resets_bench import LONGEST

    from tamp_amd import _lib

    kind, route = which.split("-")
    host = route == "host"
    mem = _lib.MEM_HOST if host else _lib.MEM_DEVICE
    rng = np.random.default_rng(SEED + 1)
    sizes = np.array([1 << k for k in range(10, 18)], dtype=np.uint64)
    pick = np.sort(rng.integers(0, len(sizes), len(in_len)))  # (sorted: the streams of one size stand together)
    record = sizes[pick]
    n, total = len(in_len), int(flat.size)
    len64 = in_len.astype(np.uint64)
    per = (np.maximum(len64, 1) - 1) // record
    first = np.zeros(n + 1, dtype=np.uint64)
    first[1:] = np.cumsum(per)
    entries = int(first[n])
    closed = np.repeat(record, per.astype(np.int64)).astype(np.uint32)
    open_size = (len64 - per * record).astype(np.uint32)
    rng = np.random.default_rng(SEED)
    at = rng.integers(0, total, RANGES).astype(np.uint64)
    r_stream = (np.searchsorted(in_off, at, side="right") - 1).astype(np.uint32)
    r_begin = np.minimum(at - in_off[r_stream], len64[r_stream] - LENGTH).astype(np.uint64)
    r_len = np.full(RANGES, LENGTH, dtype=np.uint32)
    r_off = (np.arange(RANGES, dtype=np.uint64) * LENGTH).astype(np.uint64)
    source = hashlib.sha256()
    for s, b in zip(r_stream, r_begin):
        source.update(flat[int(in_off[s] + b) : int(in_off[s] + b) + LENGTH].tobytes())
    rec = record[r_stream]
    touched = int(((r_begin + np.uint64(LENGTH - 1)) // rec - r_begin // rec + np.uint64(1)).sum())
    cap = np.array([lib.tamp_amd_compress_resets_bound(int(x), int(r), 8) for x, r in zip(in_len, record)], dtype=np.uint32)
    c_off = np.zeros(n, dtype=np.uint64)
    c_off[1:] = np.cumsum(cap.astype(np.uint64))[:-1]
    room = np.minimum(len64 + 1, 0xFFFFFFFF).astype(np.uint32)
    d_off = np.zeros(n, dtype=np.uint64)
    d_off[1:] = np.cumsum(room.astype(np.uint64))[:-1]
    whole = kind == "irregularwhole"
    dev = torch.device("cuda:0")
    arrays = dict(flat=flat, in_off=in_off.view(np.int64), in_len=in_len.view(np.int32), comp=np.zeros(int(cap.astype(np.uint64).sum()) + 1, np.uint8),
                  c_off=c_off.view(np.int64), cap=cap.view(np.int32), c_len=np.zeros(n, np.int32), c_status=np.full(n, 99, np.int8),
                  first=first.view(np.int64).copy(), group_first=np.zeros(n + len(sizes), np.int64), off=np.zeros(max(entries, 1), np.int32),
                  closed=np.resize(closed, max(entries, 1)).view(np.int32), open_size=open_size.view(np.int32), ends=np.zeros(entries + n, np.int64),
                  out=np.zeros((int(room.astype(np.uint64).sum()) if whole else RANGES * LENGTH) + 1, np.uint8),
                  d_off=d_off.view(np.int64), room=room.view(np.int32), d_len=np.zeros(n, np.int32), d_status=np.full(n, 99, np.int8),
                  used=np.zeros(n, np.int32), r_stream=r_stream.view(np.int32), r_begin=r_begin.view(np.int64), r_len=r_len.view(np.int32),
                  r_off=r_off.view(np.int64), r_out_len=np.zeros(RANGES, np.int32), r_status=np.full(RANGES, 99, np.int8))
    held = arrays if host else {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    at_row = lambda k, i: C.c_void_p((held[k].ctypes.data if host else held[k].data_ptr()) + i * arrays[k].itemsize)  # noqa: E731
    p = {k: at_row(k, 0) for k in held}
    conf = _lib.TampAmdConf(10, 8, 0, 1, 1, 0)
    for g, size in enumerate(sizes):  # one call per record size; its index rows land behind those of the sizes in front
        i0, i1 = int(np.searchsorted(pick, g, side="left")), int(np.searchsorted(pick, g, side="right"))
        if i0 == i1:
            continue
        base, count = int(first[i0]), int(first[i1] - first[i0])
        rc = lib.tamp_batch_compress_resets_index(C.byref(conf), p["flat"], at_row("in_off", i0), at_row("in_len", i0), int(size), p["comp"],
                                                  at_row("c_off", i0), at_row("cap", i0), at_row("c_len", i0), at_row("c_status", i0), i1 - i0, LONGEST,
                                                  mem, 0, None, at_row("group_first", i0 + g), at_row("off", base), count)
        torch.cuda.synchronize()
        assert rc == 0, rc
        mine = (held["group_first"] if host else held["group_first"].cpu().numpy())[i0 + g : i1 + g + 1].view(np.uint64)
        assert (mine + np.uint64(base) == first[i0 : i1 + 1]).all(), "the group's index is not where the merged one expects it"
    assert ((held["c_status"] if host else held["c_status"].cpu().numpy()) == 0).all()
    rc = lib.tamp_batch_segment_ends(p["first"], p["closed"], p["open_size"], p["ends"], n, mem, 0, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    where = (d_off[r_stream] + r_begin)[:, None] + np.arange(LENGTH, dtype=np.uint64)[None, :]
    where = where.astype(np.int64) if host else torch.from_numpy(where.astype(np.int64)).to(dev)
    ms, wall, got = [], [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        if whole:
            rc = lib.tamp_batch_decompress_resets(15, p["comp"], p["c_off"], p["c_len"], p["first"], p["off"], p["out"], p["d_off"], p["room"],
                                                  p["d_len"], p["d_status"], p["used"], n, mem, 0, None)
            got = held["out"][where]
        else:
            rc = lib.tamp_batch_read_ranges_grid(15, p["comp"], p["c_off"], p["c_len"], p["first"], p["off"], p["ends"], p["r_stream"], p["r_begin"],
                                                 p["r_len"], p["out"], p["r_off"], p["r_out_len"], p["r_status"], n, RANGES, mem, 0, None)
        e1.record()
        e1.synchronize()
        torch.cuda.synchronize()
        assert rc == 0, rc
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))
    as_np = lambda x: x if host else x.cpu().numpy()  # noqa: E731
    if whole:
        assert (as_np(held["d_status"]) == 2).all()
        delivered = as_np(got).tobytes()
    else:
        assert (as_np(held["r_status"]) == 0).all() and (as_np(held["r_out_len"]) == LENGTH).all(), as_np(held["r_status"])[:16]
        delivered = as_np(held["out"])[: RANGES * LENGTH].tobytes()
    assert hashlib.sha256(delivered).hexdigest() == source.hexdigest(), "the delivered ranges are not the input's slices"
    kept, kept_wall = sorted(ms[2:]), sorted(wall[2:])
    med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2  # noqa: E731
    print(json.dumps(dict(which=which, streams=n, bytes=total, segments=entries + n, touched=touched, median_ms=med(kept), min_ms=kept[0],
                          max_ms=kept[-1], wall_ms=med(kept_wall), calls=reps, sha256=source.hexdigest())))


def grid_main(args):
    """The rows of ``--grid``, into profiles/read_ranges_grid_bench.txt (after every row: a session that is cut short keeps what it measured)."""
    def run(which, lib=None):
        env = dict(os.environ, TAMP_AMD_BENCH_LIB=os.path.abspath(lib)) if lib else None
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, str(REPS)], capture_output=True, text=True, timeout=1100, env=env)
        if p.returncode != 0:
            raise SystemExit(f"{which}: exit {p.returncode}\n{p.stderr[-2000:]}")
        return json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])

    out = args.out if args.out != os.path.join(ROOT, "profiles", "read_ranges_bench.txt") else os.path.join(ROOT, "profiles", "read_ranges_grid_bench.txt")
    lines = ["# tools/read_ranges_bench.py --grid: the batch of tools/read_ranges_bench.py (2,000 prose streams of 8 KiB .. 4 MiB, a reset every 65,536",
             f"# bytes, window 10, literal 8, extended) and its {RANGES:,} ranges of {LENGTH:,} bytes (seed 2026).  hipEvents around each call, wall clock around",
             "# the same span, the device drained at both ends; median of the last ten of twelve calls in a fresh process (min .. max in brackets).",
             "# ranges = tamp_batch_read_ranges (a): this commit, and `parent` = a build of the parent commit in the same session; grid =",
             "# tamp_batch_read_ranges_grid on the same streams and ranges, the table made by tamp_batch_segment_ends (b); ends = that call alone (c).",
             "# irregular = the same data re-cut at record sizes of 1 .. 128 KiB (one of eight sizes per stream, log-uniform; eight compress calls",
             "# merged into one batch), read through the table; irregularwhole = tamp_batch_decompress_resets of that batch with the merged index,",
             "# then one gather of the slices.  SHA-256 over the delivered ranges equals the input's slices on every row with ranges (asserted).", ""]
    fmt = lambda r: f"{r['median_ms']:10.3f} ms [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]  wall {r['wall_ms']:10.3f} ms"  # noqa: E731
    rows = [(f"{k}-{route}", None) for route in ("device", "host") for k in ("ranges", "grid", "ends")]
    if args.parent_lib:
        rows = [row for route in ("device", "host") for row in ((f"ranges-{route}", args.parent_lib), (f"ranges-{route}", None), (f"grid-{route}", None), (f"ends-{route}", None))]
    rows += [(f"{k}-{route}", None) for route in ("device", "host") for k in ("irregular", "irregularwhole")]
    for rnd in range(args.rounds):
        lines.append(f"run {rnd + 1}")
        for which, lib in rows:
            r = run(which, lib)
            if which.startswith("irregular-") or (rnd == 0 and which == "ranges-device" and lib is None):
                lines.append(f"    ({r['streams']:,} streams, {r['bytes']:,} bytes, {r['segments']:,} segments; the ranges touch {r['touched']:,})")
            lines.append(f"    {which.replace('-', ', '):<24}{' parent' if lib else '       '} {fmt(r)}")
            print(lines[-1], flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_ranges_bench.txt"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", nargs=2, default=None)
    ap.add_argument("--grid", action="store_true", help="the table form's rows, into profiles/read_ranges_grid_bench.txt")
    ap.add_argument("--parent-lib", default=None, help="with --grid: a build of the parent commit for the rows of tamp_batch_read_ranges")
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]))
    if args.grid:
        return grid_main(args)

    def run(which):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, str(REPS)], capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            raise SystemExit(f"{which}: exit {p.returncode}\n{p.stderr[-2000:]}")
        return json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])

    lines = ["# tools/read_ranges_bench.py: the batch of tools/batch_resets_bench.py (2,000 prose streams of 8 KiB .. 4 MiB, a reset every 65,536",
             f"# bytes, window 10, literal 8, extended), compressed once per process with its reset index; {RANGES:,} ranges of {LENGTH:,} bytes, first bytes",
             "# uniform over the batch (seed 2026).  hipEvents around each call, wall clock around the same span, the device drained at both ends;",
             "# median of the last ten of twelve calls in a fresh process (min .. max in brackets).  ranges = tamp_batch_read_ranges; whole =",
             "# tamp_batch_decompress_resets of all streams with the same index, then one gather of the slices.  SHA-256 over the delivered ranges",
             "# equals the input's slices on every row (asserted).  ratio = whole / ranges on the same route.", ""]
    fmt = lambda r: f"{r['median_ms']:10.2f} ms [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  wall {r['wall_ms']:10.2f} ms"  # noqa: E731
    for rnd in range(args.rounds):
        for route in ("device", "host"):
            ranges, whole = run(f"ranges-{route}"), run(f"whole-{route}")
            assert ranges["sha256"] == whole["sha256"]
            if rnd == 0 and route == "device":
                lines.append(f"{ranges['streams']:,} streams, {ranges['bytes']:,} bytes, {ranges['segments']:,} segments; the ranges touch {ranges['touched']:,}")
            if route == "device":
                lines.append(f"run {rnd + 1}")
            lines += [f"    ranges, {route:<7} {fmt(ranges)}   ratio {whole['median_ms'] / ranges['median_ms']:7.1f}",
                      f"    whole, {route:<8} {fmt(whole)}"]
            print("\n".join(lines[-2:]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:  # (after every row pair: a session that is cut short keeps what it measured)
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
