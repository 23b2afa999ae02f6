"""A ragged batch with dictionary resets in ONE call against the routes that existed before: dev tool.

Workload: the frozen prose corpus tiled into 2,000 streams with lengths log-uniform in 8 KiB .. 4 MiB (seed 2026), window 10,
literal 8, extended format, a reset every 64 KiB.  Timed with hipEvents around each call or loop of calls (torch events on the default
stream; host-memory calls are synchronous, so the pair spans them) and with the wall clock around the same span, the device drained
at both ends:
  new, device / host    tamp_batch_compress_resets: the whole batch in one call
  loop, device / host   (a) tamp_amd_compress_resets once per stream: the same bytes (asserted: SHA-256 over all streams)
  plain, device / host  (b) tamp_batch_compress of the same streams WITHOUT resets: one workgroup per stream, other bytes
Median of the last ten of twelve calls in a fresh process; the loop and plain runs make `--old-reps` passes (default twelve) and take
the median of all but the first two (of all but the first below four).  New and old alternate, `--rounds` times (default three).
`--before-root PATH`: a built checkout of the parent commit whose package the loop and plain runs import (without it they run this
tree).

    python tools/batch_resets_bench.py [--out profiles/batch_resets_bench.txt] [--before-root ../parent-checkout]

`--decode`: the way BACK on the same batch, compressed once per process by the call under test's own library (DESIGN.md 3.13,
"Reading a batch back"), every stream with room for its size + 1:
  index, device / host   tamp_batch_decompress_resets with the index of tamp_batch_compress_resets_index
  plain, device / host   tamp_batch_decompress as it stands, on this tree and -- with `--before-root` -- on a build of the parent
  compress, device / host   the `new` rows above, on both builds (the index store and the shared entry point must cost nothing)
Median of the last ten of twelve calls in a fresh process, `--rounds` alternating runs; SHA-256 over all decoded streams must be the
input's on every row.  Written to profiles/batch_reset_decode_bench.txt.

    python tools/batch_resets_bench.py --decode [--before-root ../parent-checkout]

`--index`: the same batch read back WITHOUT its index ("Finding the resets of a batch"):
  find, device / host    (a) tamp_batch_index_resets alone, with the rounds of its start search
  both, device / host    (b) (a) followed by tamp_batch_decompress_resets with the found index
  plain, device / host   (c) tamp_batch_decompress of the same blobs, on this tree and -- with `--before-root` -- on a build of the parent
(d) the found index equals the compressor's and the decoded streams the input (SHA-256, asserted in every find / both process).
Written to profiles/index_resets_bench.txt.

    python tools/batch_resets_bench.py --index [--before-root ../parent-checkout]

`--write`: 1,000 random 4 KiB writes into the same batch, compressed once per process with its index ("Writing ranges"):
  write, device / host   tamp_batch_write_ranges: only the touched segments are decoded, patched and compressed again
  today, device / host   what a caller does without it: tamp_batch_decompress_resets of the whole batch, the patch (one indexed store
                         in torch on the device, in numpy on the host), tamp_batch_compress_resets_index of the whole batch
Median of the last ten of twelve calls in a fresh process, `--rounds` alternating runs; both ways must give the same streams and the
same index (SHA-256).

    python tools/batch_resets_bench.py --write

`--append`: bytes appended to the same batch, compressed once per process with its index ("Appending"); two workloads:
`small` -- 1,000 streams chosen at random get 4 KiB each -- and `all` -- every stream gets 64 KiB:
  append, device / host  tamp_batch_append: only the open segments are decoded; they and the new bytes are compressed, the rest is copied
  today, device / host   what a caller does without it: tamp_batch_decompress_resets of the whole batch into slots with room for the new
                         bytes, the new bytes stored behind the old ones (one indexed store in torch on the device, a copy per stream in
                         numpy on the host), tamp_batch_compress_resets_index of the whole batch
Median of the last ten of twelve calls in a fresh process, `--rounds` alternating runs (two by default); both ways must give the same
streams and the same index (SHA-256), and after every row the result is decoded and compared with old + appended (SHA-256).

    python tools/batch_resets_bench.py --append
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("BATCH_RESETS_BENCH_ROOT") or ROOT)  # (the old runs: --before-root)
STREAMS, SHORTEST, LONGEST, SEED = 2000, 8 << 10, 4 << 20, 2026
INTERVAL = 64 << 10
REPS = 12


def workload():
    """-> (flat uint8 array, in_off uint64, in_len uint32)"""
    import numpy as np

    from tamp_amd import workloads as wl

    raw = wl.frozen_corpus("prose")
    assert raw, "tests/golden/corpus_prose.txt.xz is part of the tree"
    rng = np.random.default_rng(SEED)
    in_len = np.exp(rng.uniform(np.log(SHORTEST), np.log(LONGEST), STREAMS)).astype(np.uint32)
    in_off = np.zeros(STREAMS, dtype=np.uint64)
    in_off[1:] = np.cumsum(in_len.astype(np.uint64))[:-1]
    total = int(in_len.astype(np.uint64).sum())
    one = np.frombuffer(raw, dtype=np.uint8)
    return np.tile(one, total // len(one) + 1)[:total].copy(), in_off, in_len


def child(which, reps):
    import ctypes as C

    import numpy as np
    import torch

    from tamp_amd import _lib

    lib = _lib.load()
    kind, route = which.split("-")
    flat, in_off, in_len = workload()
    n, total = len(in_len), int(flat.size)
    resets = kind != "plain"
    conf = _lib.TampAmdConf(10, 8, 0, 1, int(resets), 0)
    if resets:
        cap = np.array([lib.tamp_amd_compress_resets_bound(int(x), INTERVAL, 8) for x in in_len], dtype=np.uint32)
    else:
        cap = np.array([lib.tamp_amd_compress_bound(int(x), 8, 0) for x in in_len], dtype=np.uint32)
    out_off = np.zeros(n, dtype=np.uint64)
    out_off[1:] = np.cumsum(cap.astype(np.uint64))[:-1]
    room = int(cap.astype(np.uint64).sum())
    ms, wall = [], []

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))

    if route == "device":
        dev = torch.device("cuda:0")
        t_in, t_out = torch.from_numpy(flat).to(dev), torch.empty(room + 1, dtype=torch.uint8, device=dev)
        t_in_off, t_in_len = torch.from_numpy(in_off.view(np.int64)).to(dev), torch.from_numpy(in_len.view(np.int32)).to(dev)
        t_out_off, t_cap = torch.from_numpy(out_off.view(np.int64)).to(dev), torch.from_numpy(cap.view(np.int32)).to(dev)
        t_len = torch.zeros(n, dtype=torch.int64 if kind == "loop" else torch.int32, device=dev)
        t_status = torch.full((n,), 99, dtype=torch.int8, device=dev)
        p_in, p_out, p_len, p_status = t_in.data_ptr(), t_out.data_ptr(), t_len.data_ptr(), t_status.data_ptr()
        tables = [C.c_void_p(t.data_ptr()) for t in (t_in_off, t_in_len)], [C.c_void_p(t.data_ptr()) for t in (t_out_off, t_cap)]
        mem = _lib.MEM_DEVICE
    else:
        out = np.zeros(room + 1, dtype=np.uint8)
        h_len = np.zeros(n, dtype=np.uint64 if kind == "loop" else np.uint32)
        h_status = np.full(n, 99, dtype=np.int8)
        p_in, p_out, p_len, p_status = flat.ctypes.data, out.ctypes.data, h_len.ctypes.data, h_status.ctypes.data
        tables = [C.c_void_p(a.ctypes.data) for a in (in_off, in_len)], [C.c_void_p(a.ctypes.data) for a in (out_off, cap)]
        mem = _lib.MEM_HOST
    vp = C.c_void_p
    if kind == "new":
        def run():
            rc = lib.tamp_batch_compress_resets(C.byref(conf), vp(p_in), *tables[0], INTERVAL, vp(p_out), *tables[1], vp(p_len), vp(p_status),
                                                n, LONGEST, mem, 0, None)
            assert rc == 0, rc
    elif kind == "plain":
        def run():
            rc = lib.tamp_batch_compress(C.byref(conf), None, vp(p_in), *tables[0], vp(p_out), *tables[1], vp(p_len), vp(p_status), n, LONGEST,
                                         mem, 0, None)
            assert rc == 0, rc
    else:
        rows = [(int(in_off[i]), int(in_len[i]), int(out_off[i]), int(cap[i])) for i in range(n)]

        def run():
            for i, (io, il, oo, oc) in enumerate(rows):
                rc = lib.tamp_amd_compress_resets(C.byref(conf), vp(p_in + io), il, INTERVAL, vp(p_out + oo), oc, vp(p_len + 8 * i),
                                                  vp(p_status + i), None, mem, 0, None)
                assert rc == 0, rc
    for _ in range(reps):
        timed(run)
    if route == "device":
        out, h_len, h_status = t_out.cpu().numpy(), t_len.cpu().numpy(), t_status.cpu().numpy()
    assert (h_status == 0).all(), h_status[h_status != 0][:8]
    digest = hashlib.sha256()
    for i in range(n):
        digest.update(out[int(out_off[i]) : int(out_off[i]) + int(h_len[i])].tobytes())
    skip = 2 if reps >= 4 else 1
    kept, kept_wall = sorted(ms[skip:]), sorted(wall[skip:])
    med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2  # noqa: E731
    print(json.dumps(dict(which=which, streams=n, bytes=total, median_ms=med(kept), min_ms=kept[0], max_ms=kept[-1], wall_ms=med(kept_wall),
                          calls=reps, out_len=int(h_len.astype(np.uint64).sum()), sha256=digest.hexdigest(), lib=_lib.LIB_PATH)))


def decode_child(which, reps):
    """One decode row: `index-device`, `index-host`, `plain-device`, `plain-host`."""
    import ctypes as C

    import numpy as np
    import torch

    from tamp_amd import _lib

    lib = _lib.load()
    kind, route = which.split("-")
    flat, in_off, in_len = workload()
    n, total = len(in_len), int(flat.size)
    conf = _lib.TampAmdConf(10, 8, 0, 1, 1, 0)
    cap = np.array([lib.tamp_amd_compress_resets_bound(int(x), INTERVAL, 8) for x in in_len], dtype=np.uint32)
    c_off = np.zeros(n, dtype=np.uint64)
    c_off[1:] = np.cumsum(cap.astype(np.uint64))[:-1]
    entries = int(((np.maximum(in_len.astype(np.uint64), 1) - 1) // INTERVAL).sum())
    room = np.minimum(in_len.astype(np.uint64) + 1, 0xFFFFFFFF).astype(np.uint32)  # (size + 1: a stream that fits ends with status 2)
    d_off = np.zeros(n, dtype=np.uint64)
    d_off[1:] = np.cumsum(room.astype(np.uint64))[:-1]
    dev = torch.device("cuda:0")
    host = route == "host"
    mem = _lib.MEM_HOST if host else _lib.MEM_DEVICE
    arrays = dict(flat=flat, in_off=in_off.view(np.int64), in_len=in_len.view(np.int32), comp=np.zeros(int(cap.astype(np.uint64).sum()) + 1, np.uint8),
                  c_off=c_off.view(np.int64), cap=cap.view(np.int32), c_len=np.zeros(n, np.int32), c_status=np.full(n, 99, np.int8),
                  first=np.zeros(n + 1, np.int64), off=np.zeros(max(entries, 1), np.int32), out=np.zeros(int(room.astype(np.uint64).sum()) + 1, np.uint8),
                  d_off=d_off.view(np.int64), room=room.view(np.int32), d_len=np.zeros(n, np.int32), d_status=np.full(n, 99, np.int8),
                  used=np.zeros(n, np.int32))
    held = arrays if host else {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    p = {k: C.c_void_p(v.ctypes.data if host else v.data_ptr()) for k, v in held.items()}
    if kind == "index":
        rc = lib.tamp_batch_compress_resets_index(C.byref(conf), p["flat"], p["in_off"], p["in_len"], INTERVAL, p["comp"], p["c_off"], p["cap"],
                                                  p["c_len"], p["c_status"], n, LONGEST, mem, 0, None, p["first"], p["off"], entries)
    else:
        rc = lib.tamp_batch_compress_resets(C.byref(conf), p["flat"], p["in_off"], p["in_len"], INTERVAL, p["comp"], p["c_off"], p["cap"],
                                            p["c_len"], p["c_status"], n, LONGEST, mem, 0, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    ms, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        if kind == "index":
            rc = lib.tamp_batch_decompress_resets(15, p["comp"], p["c_off"], p["c_len"], p["first"], p["off"], p["out"], p["d_off"], p["room"],
                                                  p["d_len"], p["d_status"], p["used"], n, mem, 0, None)
        else:
            rc = lib.tamp_batch_decompress(None, 0, 15, p["comp"], p["c_off"], p["c_len"], p["out"], p["d_off"], p["room"], p["d_len"],
                                           p["d_status"], p["used"], n, mem, 0, None)
        e1.record()
        e1.synchronize()
        torch.cuda.synchronize()
        assert rc == 0, rc
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))
    back = held if host else {k: held[k].cpu().numpy() for k in ("out", "d_len", "d_status", "used", "c_len", "c_status")}
    assert (back["c_status"] == 0).all() and (back["d_status"] == 2).all(), back["d_status"][back["d_status"] != 2][:8]
    assert (back["d_len"].view(np.uint32) == in_len).all() and (back["used"] == back["c_len"]).all()
    digest, source = hashlib.sha256(), hashlib.sha256()
    for i in range(n):
        digest.update(back["out"][int(d_off[i]) : int(d_off[i]) + int(in_len[i])].tobytes())
        source.update(flat[int(in_off[i]) : int(in_off[i]) + int(in_len[i])].tobytes())
    assert digest.hexdigest() == source.hexdigest(), "the decoded streams are not the input"
    kept, kept_wall = sorted(ms[2:]), sorted(wall[2:])
    med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2  # noqa: E731
    print(json.dumps(dict(which=which, streams=n, bytes=total, median_ms=med(kept), min_ms=kept[0], max_ms=kept[-1], wall_ms=med(kept_wall),
                          calls=reps, comp_len=int(back["c_len"].astype(np.uint64).sum()), sha256=digest.hexdigest(), lib=_lib.LIB_PATH)))


def decode_main(args):
    me = os.path.abspath(__file__)

    def run(flag, which, parent):
        env = dict(os.environ)
        if parent:
            env["BATCH_RESETS_BENCH_ROOT"] = os.path.abspath(args.before_root)
        p = subprocess.run([sys.executable, me, flag, which, str(REPS)], env=env, capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            raise SystemExit(f"{which}: exit {p.returncode}\n{p.stderr[-2000:]}")
        return json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])

    lines = [f"# tools/batch_resets_bench.py --decode: prose corpus tiled into {STREAMS:,} streams, lengths log-uniform in {SHORTEST:,} .. {LONGEST:,} bytes",
             f"# (seed {SEED}), window 10, literal 8, extended, a reset every 65,536 bytes, compressed once per process; every stream decoded into",
             "# its size + 1 bytes.  hipEvents around each call, wall clock around the same span, the device drained at both ends; median of the",
             "# last ten of twelve calls in a fresh process (min .. max in brackets).  index = tamp_batch_decompress_resets with the compressor's",
             "# reset index; plain = tamp_batch_decompress; compress = tamp_batch_compress_resets.  'parent': a build of the parent commit."
             if args.before_root else "# reset index; plain = tamp_batch_decompress; compress = tamp_batch_compress_resets.",
             "# SHA-256 over all decoded streams equals the input's on every row (asserted).  ratio = plain / index on the same route.", ""]
    fmt = lambda r: (f"{r['median_ms']:10.2f} ms [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  wall {r['wall_ms']:10.2f} ms "  # noqa: E731
                     f"{r['bytes'] / r['median_ms'] / 1e6:8.2f} GB/s")
    sides = [("this tree", False)] + ([("parent", True)] if args.before_root else [])
    for rnd in range(args.rounds):
        lines.append(f"run {rnd + 1}")
        for route in ("device", "host"):
            index = run("--decode-child", f"index-{route}", False)
            lines.append(f"    index, {route:<7} this tree  {fmt(index)}")
            digests = {index["sha256"]}
            for name, parent in sides:
                plain = run("--decode-child", f"plain-{route}", parent)
                digests.add(plain["sha256"])
                lines.append(f"    plain, {route:<7} {name:<9}  {fmt(plain)}   ratio {plain['median_ms'] / index['median_ms']:6.2f}")
            assert len(digests) == 1, digests
            for name, parent in sides:
                lines.append(f"    compress, {route:<4} {name:<9}  {fmt(run('--child', f'new-{route}', parent))}")
        print("\n".join(lines[-(1 + 2 * (1 + 2 * len(sides))):]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # (after every run: a session that is cut short keeps what it measured)
            f.write("\n".join(lines) + "\n")


def index_child(which, reps):
    """One row of --index: `find-device`, `find-host`, `both-device`, `both-host`."""
    import ctypes as C

    import numpy as np
    import torch

    from tamp_amd import _lib

    lib = _lib.load()
    kind, route = which.split("-")
    flat, in_off, in_len = workload()
    n, total = len(in_len), int(flat.size)
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
    E = max(entries, 1)
    arrays = dict(flat=flat, in_off=in_off.view(np.int64), in_len=in_len.view(np.int32), comp=np.zeros(int(cap.astype(np.uint64).sum()) + 1, np.uint8),
                  c_off=c_off.view(np.int64), cap=cap.view(np.int32), c_len=np.zeros(n, np.int32), c_status=np.full(n, 99, np.int8),
                  first=np.zeros(n + 1, np.int64), off=np.zeros(E, np.int32), found_first=np.zeros(n + 1, np.int64), found_off=np.zeros(E, np.int32),
                  closed=np.zeros(E, np.int32), open=np.zeros(n, np.int32), f_status=np.full(n, 99, np.int8),
                  out=np.zeros(int(room.astype(np.uint64).sum()) + 1, np.uint8), d_off=d_off.view(np.int64), room=room.view(np.int32),
                  d_len=np.zeros(n, np.int32), d_status=np.full(n, 99, np.int8), used=np.zeros(n, np.int32))
    held = arrays if host else {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    p = {k: C.c_void_p(v.ctypes.data if host else v.data_ptr()) for k, v in held.items()}
    rc = lib.tamp_batch_compress_resets_index(C.byref(conf), p["flat"], p["in_off"], p["in_len"], INTERVAL, p["comp"], p["c_off"], p["cap"],
                                              p["c_len"], p["c_status"], n, LONGEST, mem, 0, None, p["first"], p["off"], entries)
    torch.cuda.synchronize()
    assert rc == 0, rc
    ms, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        rc = lib.tamp_batch_index_resets(15, p["comp"], p["c_off"], p["c_len"], p["found_first"], p["found_off"], p["closed"], p["open"], entries,
                                         p["f_status"], n, mem, 0, None)
        if kind == "both" and rc == 0:
            rc = lib.tamp_batch_decompress_resets(15, p["comp"], p["c_off"], p["c_len"], p["found_first"], p["found_off"], p["out"], p["d_off"],
                                                  p["room"], p["d_len"], p["d_status"], p["used"], n, mem, 0, None)
        e1.record()
        e1.synchronize()
        torch.cuda.synchronize()
        assert rc == 0, rc
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))
    back = held if host else {k: v.cpu().numpy() for k, v in held.items() if k not in ("flat", "comp")}
    assert (back["c_status"] == 0).all() and (back["f_status"] == 0).all()
    index = hashlib.sha256(back["first"].tobytes() + back["off"][:entries].tobytes()).hexdigest()
    found = hashlib.sha256(back["found_first"].tobytes() + back["found_off"][:entries].tobytes()).hexdigest()
    assert found == index, "the found index is not the compressor's"
    run_sum = np.concatenate([[0], np.cumsum(back["closed"][:entries].view(np.uint32).astype(np.uint64))])
    sizes = run_sum[back["first"][1:]] - run_sum[back["first"][:-1]] + back["open"].view(np.uint32)
    assert (sizes == in_len).all(), "the sizes of the scan are not the inputs'"
    digest = None
    if kind == "both":
        assert (back["d_status"] == 2).all() and (back["d_len"].view(np.uint32) == in_len).all()
        digest, source = hashlib.sha256(), hashlib.sha256()
        for i in range(n):
            digest.update(back["out"][int(d_off[i]) : int(d_off[i]) + int(in_len[i])].tobytes())
            source.update(flat[int(in_off[i]) : int(in_off[i]) + int(in_len[i])].tobytes())
        assert digest.hexdigest() == source.hexdigest(), "the decoded streams are not the input"
        digest = digest.hexdigest()
    kept, kept_wall = sorted(ms[2:]), sorted(wall[2:])
    med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2  # noqa: E731
    print(json.dumps(dict(which=which, streams=n, bytes=total, median_ms=med(kept), min_ms=kept[0], max_ms=kept[-1], wall_ms=med(kept_wall),
                          calls=reps, comp_len=int(back["c_len"].astype(np.uint64).sum()), entries=entries, index_sha256=found, sha256=digest,
                          lib=_lib.LIB_PATH)))


def index_main(args):
    import re

    me = os.path.abspath(__file__)
    line = re.compile(r"index: (\d+) streams, (\d+) chunks, (\d+) rounds, (\d+) entries")

    def run(flag, which, parent):
        env = dict(os.environ, TAMP_AMD_RESETS_DEBUG="1") if flag == "--index-child" else dict(os.environ)
        if parent:
            env["BATCH_RESETS_BENCH_ROOT"] = os.path.abspath(args.before_root)
        p = subprocess.run([sys.executable, me, flag, which, str(REPS)], env=env, capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            raise SystemExit(f"{which}: exit {p.returncode}\n{p.stderr[-2000:]}")
        r = json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])
        m = line.search(p.stderr)
        if m:
            r["chunks"], r["rounds"] = int(m[2]), int(m[3])
        return r

    lines = [f"# tools/batch_resets_bench.py --index: prose corpus tiled into {STREAMS:,} streams, lengths log-uniform in {SHORTEST:,} .. {LONGEST:,} bytes",
             f"# (seed {SEED}), window 10, literal 8, extended, a reset every 65,536 bytes, compressed once per process.  hipEvents around each call or",
             "# pair of calls, wall clock around the same span, the device drained at both ends; median of the last ten of twelve in a fresh process",
             "# (min .. max in brackets).  find = (a) tamp_batch_index_resets alone; both = (b) find, then tamp_batch_decompress_resets with the FOUND",
             "# index; plain = (c) tamp_batch_decompress of the same blobs without an index" + (", 'parent': a build of the parent commit." if args.before_root else "."),
             "# (d) asserted in every find / both process: SHA-256 of the found index equals the compressor's, the scan's sizes are the inputs', and",
             "# (both) SHA-256 over all decoded streams equals the input's.  gain = plain / both on the same route.", ""]
    fmt = lambda r: (f"{r['median_ms']:10.2f} ms [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  wall {r['wall_ms']:10.2f} ms")  # noqa: E731
    sides = [("this tree", False)] + ([("parent", True)] if args.before_root else [])
    for rnd in range(args.rounds):
        lines.append(f"run {rnd + 1}")
        for route in ("device", "host"):
            find = run("--index-child", f"find-{route}", False)
            both = run("--index-child", f"both-{route}", False)
            assert find["index_sha256"] == both["index_sha256"]
            lines.append(f"    find, {route:<7} this tree  {fmt(find)}   {find.get('chunks', 0):,} chunks, {find.get('rounds', 0)} rounds, {find['entries']:,} entries")
            lines.append(f"    both, {route:<7} this tree  {fmt(both)}")
            for name, parent in sides:
                plain = run("--decode-child", f"plain-{route}", parent)
                assert plain["sha256"] == both["sha256"]
                spread = max(both["max_ms"] - both["min_ms"], plain["max_ms"] - plain["min_ms"])
                lines.append(f"    plain, {route:<6} {name:<9}  {fmt(plain)}   gain {plain['median_ms'] / both['median_ms']:5.2f}, plain - both "
                             f"{plain['median_ms'] - both['median_ms']:.2f} ms against a spread of {spread:.2f} ms")
        print("\n".join(lines[-(1 + 2 * (2 + len(sides))):]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # (after every run: a session that is cut short keeps what it measured)
            f.write("\n".join(lines) + "\n")


WRITES, WRITE_BYTES = 1000, 4096


def write_child(which, reps):
    """One row of --write: `write-device`, `write-host`, `today-device`, `today-host`."""
    import ctypes as C

    import numpy as np
    import torch

    from tamp_amd import _lib

    lib = _lib.load()
    kind, route = which.split("-")
    flat, in_off, in_len = workload()
    n, total = len(in_len), int(flat.size)
    conf = _lib.TampAmdConf(10, 8, 0, 1, 1, 0)
    cap = np.array([lib.tamp_amd_compress_resets_bound(int(x), INTERVAL, 8) for x in in_len], dtype=np.uint32)
    c_off = np.zeros(n, dtype=np.uint64)
    c_off[1:] = np.cumsum(cap.astype(np.uint64))[:-1]
    entries = int(((np.maximum(in_len.astype(np.uint64), 1) - 1) // INTERVAL).sum())
    room = np.minimum(in_len.astype(np.uint64) + 1, 0xFFFFFFFF).astype(np.uint32)
    d_off = np.zeros(n, dtype=np.uint64)
    d_off[1:] = np.cumsum(room.astype(np.uint64))[:-1]
    # the writes: disjoint, sorted by (stream, begin); the same ones in every process
    rng = np.random.default_rng(SEED + 1)
    taken, rows = {}, []
    while len(rows) < WRITES:
        i = int(rng.integers(n))
        if in_len[i] < WRITE_BYTES:
            continue
        b = int(rng.integers(int(in_len[i]) - WRITE_BYTES + 1))
        if any(abs(b - o) < WRITE_BYTES for o in taken.get(i, ())):
            continue
        taken.setdefault(i, []).append(b)
        rows.append((i, b))
    rows.sort()
    w_stream = np.array([r[0] for r in rows], dtype=np.uint32)
    w_begin = np.array([r[1] for r in rows], dtype=np.uint64)
    w_len = np.full(WRITES, WRITE_BYTES, dtype=np.uint32)
    src = rng.integers(32, 127, WRITES * WRITE_BYTES, dtype=np.uint8)
    src_off = np.arange(WRITES, dtype=np.uint64) * WRITE_BYTES
    touched = len({(i, k) for i, b in rows for k in range(b // INTERVAL, (b + WRITE_BYTES - 1) // INTERVAL + 1)})
    # where every source byte goes in the decoded batch (the patch of `today`)
    where = (d_off[w_stream] + w_begin)[:, None] + np.arange(WRITE_BYTES, dtype=np.uint64)[None, :]
    dev = torch.device("cuda:0")
    host = route == "host"
    mem = _lib.MEM_HOST if host else _lib.MEM_DEVICE
    comp_room = int(cap.astype(np.uint64).sum()) + 1
    arrays = dict(flat=flat, in_off=in_off.view(np.int64), in_len=in_len.view(np.int32), comp=np.zeros(comp_room, np.uint8),
                  c_off=c_off.view(np.int64), cap=cap.view(np.int32), c_len=np.zeros(n, np.int32), c_status=np.full(n, 99, np.int8),
                  first=np.zeros(n + 1, np.int64), off=np.zeros(max(entries, 1), np.int32), w_stream=w_stream.view(np.int32),
                  w_begin=w_begin.view(np.int64), w_len=w_len.view(np.int32), src=src, src_off=src_off.view(np.int64),
                  comp2=np.zeros(comp_room, np.uint8), c2_len=np.zeros(n, np.int32), c2_status=np.full(n, 99, np.int8),
                  first2=np.zeros(n + 1, np.int64), off2=np.zeros(max(entries, 1), np.int32), where=where.reshape(-1).view(np.int64))
    if kind == "today":
        arrays.update(out=np.zeros(int(room.astype(np.uint64).sum()) + 1, np.uint8), d_off=d_off.view(np.int64), room=room.view(np.int32),
                      d_len=np.zeros(n, np.int32), d_status=np.full(n, 99, np.int8), used=np.zeros(n, np.int32))
    held = arrays if host else {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    p = {k: C.c_void_p(v.ctypes.data if host else v.data_ptr()) for k, v in held.items()}
    rc = lib.tamp_batch_compress_resets_index(C.byref(conf), p["flat"], p["in_off"], p["in_len"], INTERVAL, p["comp"], p["c_off"], p["cap"],
                                              p["c_len"], p["c_status"], n, LONGEST, mem, 0, None, p["first"], p["off"], entries)
    torch.cuda.synchronize()
    assert rc == 0, rc
    ms, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        if kind == "write":
            rc = lib.tamp_batch_write_ranges(C.byref(conf), 15, p["comp"], p["c_off"], p["c_len"], p["first"], p["off"], INTERVAL, p["w_stream"],
                                             p["w_begin"], p["w_len"], p["src"], p["src_off"], p["comp2"], p["c_off"], p["cap"], p["c2_len"],
                                             p["c2_status"], p["off2"], n, WRITES, mem, 0, None)
        else:
            rc = lib.tamp_batch_decompress_resets(15, p["comp"], p["c_off"], p["c_len"], p["first"], p["off"], p["out"], p["d_off"], p["room"],
                                                  p["d_len"], p["d_status"], p["used"], n, mem, 0, None)
            assert rc == 0, rc
            held["out"][held["where"]] = held["src"]
            rc = lib.tamp_batch_compress_resets_index(C.byref(conf), p["out"], p["d_off"], p["in_len"], INTERVAL, p["comp2"], p["c_off"], p["cap"],
                                                      p["c2_len"], p["c2_status"], n, LONGEST, mem, 0, None, p["first2"], p["off2"], entries)
        e1.record()
        e1.synchronize()
        torch.cuda.synchronize()
        assert rc == 0, rc
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))
    back = held if host else {k: held[k].cpu().numpy() for k in ("comp2", "c2_len", "c2_status", "off2")}
    assert (back["c2_status"] == 0).all(), back["c2_status"][back["c2_status"] != 0][:8]
    digest = hashlib.sha256()
    for i in range(n):
        digest.update(back["comp2"][int(c_off[i]) : int(c_off[i]) + int(back["c2_len"][i])].tobytes())
    digest.update(back["off2"][:entries].tobytes())
    kept, kept_wall = sorted(ms[2:]), sorted(wall[2:])
    med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2  # noqa: E731
    print(json.dumps(dict(which=which, streams=n, bytes=total, median_ms=med(kept), min_ms=kept[0], max_ms=kept[-1], wall_ms=med(kept_wall),
                          calls=reps, touched=touched, segments=entries + n, comp_len=int(back["c2_len"].astype(np.uint64).sum()),
                          sha256=digest.hexdigest(), lib=_lib.LIB_PATH)))


def write_main(args):
    me = os.path.abspath(__file__)

    def run(which):
        p = subprocess.run([sys.executable, me, "--write-child", which, str(REPS)], capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            raise SystemExit(f"{which}: exit {p.returncode}\n{p.stderr[-2000:]}")
        return json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])

    lines = [f"# tools/batch_resets_bench.py --write: prose corpus tiled into {STREAMS:,} streams, lengths log-uniform in {SHORTEST:,} .. {LONGEST:,} bytes",
             f"# (seed {SEED}), window 10, literal 8, extended, a reset every 65,536 bytes, compressed once per process with its index; then",
             f"# {WRITES:,} random disjoint writes of {WRITE_BYTES:,} bytes.  write = tamp_batch_write_ranges; today = tamp_batch_decompress_resets of the",
             "# whole batch, the patch as ONE indexed store (torch on the device, numpy on the host), tamp_batch_compress_resets_index of the",
             "# whole batch.  hipEvents around each pass, wall clock around the same span, the device drained at both ends; median of the last ten",
             "# of twelve passes in a fresh process (min .. max in brackets).  Streams and index of both ways are the same bytes (SHA-256,",
             "# asserted).  ratio = today / write on the same route.", ""]
    fmt = lambda r: f"{r['median_ms']:10.2f} ms [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  wall {r['wall_ms']:10.2f} ms"  # noqa: E731
    spread = {}
    for rnd in range(args.rounds):
        got = {w: run(w) for w in ("write-device", "today-device", "write-host", "today-host")}
        assert len({r["sha256"] for r in got.values()}) == 1, got
        first = got["write-device"]
        lines.append(f"{first['streams']:,} streams, {first['bytes']:,} bytes in {first['segments']:,} segments, {first['touched']:,} of them touched  run {rnd + 1}")
        for route in ("device", "host"):
            w, t = got[f"write-{route}"], got[f"today-{route}"]
            spread.setdefault(route, []).append((w["median_ms"], t["median_ms"]))
            lines += [f"    write, {route:<7} {fmt(w)}   ratio {t['median_ms'] / w['median_ms']:7.2f}", f"    today, {route:<7} {fmt(t)}"]
        print("\n".join(lines[-5:]), flush=True)
        tail = [""]
        for route in ("device", "host"):
            ws, ts = [s[0] for s in spread[route]], [s[1] for s in spread[route]]
            tail.append(f"{route}: write medians {min(ws):.2f} .. {max(ws):.2f} ms, today medians {min(ts):.2f} .. {max(ts):.2f} ms over the runs; "
                        f"smallest today / write ratio {min(t / w for w, t in spread[route]):.2f}")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # (after every run: a session that is cut short keeps what it measured)
            f.write("\n".join(lines + tail) + "\n")

APPEND_LOADS = {"small": (1000, 4096), "all": (STREAMS, 64 << 10)}


def append_child(which, reps):
    """One row of --append: `append-device-small`, `append-host-all`, `today-device-small`, ..."""
    import ctypes as C

    import numpy as np
    import torch

    from tamp_amd import _lib

    lib = _lib.load()
    kind, route, load = which.split("-")
    flat, in_off, in_len = workload()
    n, total = len(in_len), int(flat.size)
    conf = _lib.TampAmdConf(10, 8, 0, 1, 1, 0)
    rng = np.random.default_rng(SEED + 2)
    count, piece = APPEND_LOADS[load]
    chosen = np.sort(rng.choice(n, count, replace=False))
    src_len = np.zeros(n, dtype=np.uint32)
    src_len[chosen] = piece
    src_off = np.zeros(n, dtype=np.uint64)
    src_off[1:] = np.cumsum(src_len.astype(np.uint64))[:-1]
    src = rng.integers(32, 127, count * piece, dtype=np.uint8)
    new_len = (in_len.astype(np.uint64) + src_len).astype(np.uint32)
    bound = lambda lens: np.array([lib.tamp_amd_compress_resets_bound(int(x), INTERVAL, 8) for x in lens], dtype=np.uint32)  # noqa: E731
    offsets = lambda sizes: np.concatenate([[0], np.cumsum(sizes.astype(np.uint64))[:-1]]).astype(np.uint64)  # noqa: E731
    cap, cap2 = bound(in_len), bound(new_len)
    c_off, c2_off = offsets(cap), offsets(cap2)
    entries = int(((np.maximum(in_len.astype(np.uint64), 1) - 1) // INTERVAL).sum())
    entries2 = entries + int(((src_len.astype(np.uint64) + INTERVAL - 1) // INTERVAL).sum())  # (the bound tamp_batch_append asks for)
    room2 = np.minimum(new_len.astype(np.uint64) + 1, 0xFFFFFFFF).astype(np.uint32)  # decoded slots with room for the new bytes
    d2_off = offsets(room2)
    where = ((d2_off + in_len)[chosen, None] + np.arange(piece, dtype=np.uint64)[None, :]).reshape(-1)  # (where every new byte goes)
    dev = torch.device("cuda:0")
    host = route == "host"
    mem = _lib.MEM_HOST if host else _lib.MEM_DEVICE
    arrays = dict(flat=flat, in_off=in_off.view(np.int64), in_len=in_len.view(np.int32), comp=np.zeros(int(cap.astype(np.uint64).sum()) + 1, np.uint8),
                  c_off=c_off.view(np.int64), cap=cap.view(np.int32), c_len=np.zeros(n, np.int32), c_status=np.full(n, 99, np.int8),
                  first=np.zeros(n + 1, np.int64), off=np.zeros(max(entries, 1), np.int32), src=src, src_off=src_off.view(np.int64),
                  src_len=src_len.view(np.int32), new_len=new_len.view(np.int32), comp2=np.zeros(int(cap2.astype(np.uint64).sum()) + 1, np.uint8),
                  c2_off=c2_off.view(np.int64), cap2=cap2.view(np.int32), c2_len=np.zeros(n, np.int32), c2_status=np.full(n, 99, np.int8),
                  first2=np.zeros(n + 1, np.int64), off2=np.zeros(max(entries2, 1), np.int32),
                  out=np.zeros(int(room2.astype(np.uint64).sum()) + 1, np.uint8), d2_off=d2_off.view(np.int64), room2=room2.view(np.int32),
                  d_len=np.zeros(n, np.int32), d_status=np.full(n, 99, np.int8), used=np.zeros(n, np.int32), where=where.view(np.int64))
    held = arrays if host else {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    p = {k: C.c_void_p(v.ctypes.data if host else v.data_ptr()) for k, v in held.items()}
    rc = lib.tamp_batch_compress_resets_index(C.byref(conf), p["flat"], p["in_off"], p["in_len"], INTERVAL, p["comp"], p["c_off"], p["cap"],
                                              p["c_len"], p["c_status"], n, LONGEST, mem, 0, None, p["first"], p["off"], entries)
    torch.cuda.synchronize()
    assert rc == 0, rc
    longest2 = int(new_len.max())

    def decode_into_slots(comp, off_, len_, first_, idx_):
        r = lib.tamp_batch_decompress_resets(15, p[comp], p[off_], p[len_], p[first_], p[idx_], p["out"], p["d2_off"], p["room2"], p["d_len"],
                                             p["d_status"], p["used"], n, mem, 0, None)
        assert r == 0, r

    ms, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        if kind == "append":
            rc = lib.tamp_batch_append(C.byref(conf), 15, p["comp"], p["c_off"], p["c_len"], p["first"], p["off"], INTERVAL, p["src"], p["src_off"],
                                       p["src_len"], p["comp2"], p["c2_off"], p["cap2"], p["c2_len"], p["c2_status"], p["first2"], p["off2"], entries2,
                                       n, mem, 0, None)
        else:
            decode_into_slots("comp", "c_off", "c_len", "first", "off")
            if host:
                for i in chosen:
                    at = int(d2_off[i]) + int(in_len[i])
                    held["out"][at : at + piece] = src[int(src_off[i]) : int(src_off[i]) + piece]
            else:
                held["out"][held["where"]] = held["src"]
            rc = lib.tamp_batch_compress_resets_index(C.byref(conf), p["out"], p["d2_off"], p["new_len"], INTERVAL, p["comp2"], p["c2_off"], p["cap2"],
                                                      p["c2_len"], p["c2_status"], n, longest2, mem, 0, None, p["first2"], p["off2"], entries2)
        e1.record()
        e1.synchronize()
        torch.cuda.synchronize()
        assert rc == 0, rc
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))
    # the result, decoded, against old + appended
    if host:
        held["out"][:] = 0
    else:
        held["out"].zero_()
    decode_into_slots("comp2", "c2_off", "c2_len", "first2", "off2")
    torch.cuda.synchronize()
    back = held if host else {k: held[k].cpu().numpy() for k in ("comp2", "c2_len", "c2_status", "first2", "off2", "out", "d_len", "d_status")}
    assert (back["c2_status"] == 0).all(), back["c2_status"][back["c2_status"] != 0][:8]
    assert (back["d_len"].view(np.uint32) == new_len).all()
    got, want = hashlib.sha256(), hashlib.sha256()
    for i in range(n):
        got.update(back["out"][int(d2_off[i]) : int(d2_off[i]) + int(new_len[i])].tobytes())
        want.update(flat[int(in_off[i]) : int(in_off[i]) + int(in_len[i])].tobytes())
        want.update(src[int(src_off[i]) : int(src_off[i]) + int(src_len[i])].tobytes())
    assert got.hexdigest() == want.hexdigest(), "the decoded result is not old + appended"
    digest = hashlib.sha256()
    for i in range(n):
        digest.update(back["comp2"][int(c2_off[i]) : int(c2_off[i]) + int(back["c2_len"][i])].tobytes())
    new_entries = int(back["first2"][n])
    digest.update(back["first2"].tobytes())
    digest.update(back["off2"][:new_entries].tobytes())
    kept, kept_wall = sorted(ms[2:]), sorted(wall[2:])
    med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2  # noqa: E731
    print(json.dumps(dict(which=which, streams=n, bytes=total, appended=int(count) * piece, appends=int(count), median_ms=med(kept), min_ms=kept[0],
                          max_ms=kept[-1], wall_ms=med(kept_wall), calls=reps, segments=entries + n, new_segments=new_entries + n,
                          comp_len=int(back["c2_len"].astype(np.uint64).sum()), sha256=digest.hexdigest(), decoded_sha256=got.hexdigest(),
                          lib=_lib.LIB_PATH)))


def append_main(args):
    me = os.path.abspath(__file__)

    def run(which):
        p = subprocess.run([sys.executable, me, "--append-child", which, str(REPS)], capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            raise SystemExit(f"{which}: exit {p.returncode}\n{p.stderr[-2000:]}")
        return json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])

    lines = [f"# tools/batch_resets_bench.py --append: prose corpus tiled into {STREAMS:,} streams, lengths log-uniform in {SHORTEST:,} .. {LONGEST:,} bytes",
             f"# (seed {SEED}), window 10, literal 8, extended, a reset every 65,536 bytes, compressed once per process with its index; then",
             "# small: 1,000 streams chosen at random receive 4,096 bytes each; all: every stream receives 65,536 bytes.",
             "# append = tamp_batch_append; today = tamp_batch_decompress_resets of the whole batch into slots with room for the new bytes, the new",
             "# bytes stored behind the old ones (ONE indexed store in torch on the device, a copy per stream in numpy on the host),",
             "# tamp_batch_compress_resets_index of the whole batch.  hipEvents around each pass, wall clock around the same span, the device drained",
             "# at both ends; median of the last ten of twelve passes in a fresh process (min .. max in brackets).  Streams and index of both ways",
             "# are the same bytes (SHA-256, asserted), and every row's result decodes to old + appended (SHA-256, asserted in the process).",
             "# ratio = today / append on the same route.", ""]
    fmt = lambda r: f"{r['median_ms']:10.2f} ms [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  wall {r['wall_ms']:10.2f} ms"  # noqa: E731
    spread = {}
    for rnd in range(args.rounds):
        for load in ("small", "all"):
            got = {w: run(f"{w}-{load}") for w in ("append-device", "today-device", "append-host", "today-host")}
            assert len({r["sha256"] for r in got.values()}) == 1, got
            first = got["append-device"]
            lines.append(f"{load}: {first['appends']:,} appends of {first['appended'] // first['appends']:,} bytes to {first['streams']:,} streams, "
                         f"{first['bytes']:,} bytes in {first['segments']:,} segments ({first['new_segments']:,} afterwards)  run {rnd + 1}")
            for route in ("device", "host"):
                a, t = got[f"append-{route}"], got[f"today-{route}"]
                spread.setdefault((load, route), []).append((a["median_ms"], t["median_ms"]))
                lines += [f"    append, {route:<7} {fmt(a)}   ratio {t['median_ms'] / a['median_ms']:7.2f}", f"    today,  {route:<7} {fmt(t)}"]
            print("\n".join(lines[-5:]), flush=True)
            tail = [""]
            for (ld, route), rows in spread.items():
                aps, ts = [r[0] for r in rows], [r[1] for r in rows]
                tail.append(f"{ld}, {route}: append medians {min(aps):.2f} .. {max(aps):.2f} ms, today medians {min(ts):.2f} .. {max(ts):.2f} ms over the runs; "
                            f"smallest today / append ratio {min(t / a for a, t in rows):.2f}")
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:  # (after every row group: a session that is cut short keeps what it measured)
                f.write("\n".join(lines + tail) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_resets_bench.txt"))
    ap.add_argument("--before-root", default=None)
    ap.add_argument("--old-reps", type=int, default=REPS)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", nargs=2, default=None)
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--decode-child", nargs=2, default=None)
    ap.add_argument("--index", action="store_true")
    ap.add_argument("--index-child", nargs=2, default=None)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--write-child", nargs=2, default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--append-child", nargs=2, default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]))
    if args.decode_child:
        return decode_child(args.decode_child[0], int(args.decode_child[1]))
    if args.index_child:
        return index_child(args.index_child[0], int(args.index_child[1]))
    if args.write_child:
        return write_child(args.write_child[0], int(args.write_child[1]))
    if args.append_child:
        return append_child(args.append_child[0], int(args.append_child[1]))
    if args.append:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "append_bench.txt")
        if args.rounds == ap.get_default("rounds"):
            args.rounds = 2
        return append_main(args)
    if args.write:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "write_ranges_bench.txt")
        return write_main(args)
    if args.index:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "index_resets_bench.txt")
        return index_main(args)
    if args.decode:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "batch_reset_decode_bench.txt")
        return decode_main(args)

    def run(which):
        env = dict(os.environ)
        old = not which.startswith("new")
        if old and args.before_root:
            env["BATCH_RESETS_BENCH_ROOT"] = os.path.abspath(args.before_root)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, str(args.old_reps if old else REPS)], env=env,
                           capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            raise SystemExit(f"{which}: exit {p.returncode}\n{p.stderr[-2000:]}")
        return json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])

    old_kept = args.old_reps - (2 if args.old_reps >= 4 else 1)
    lines = [f"# tools/batch_resets_bench.py: prose corpus tiled into {STREAMS:,} streams, lengths log-uniform in {SHORTEST:,} .. {LONGEST:,} bytes (seed {SEED}),",
             "# window 10, literal 8, extended, a reset every 65,536 bytes; hipEvents around each call (loop: around the 2,000 calls), wall clock",
             "# around the same span; new: median of the last ten of twelve calls in a fresh process (min .. max in brackets); loop and plain:",
             f"# median of the last {old_kept} of {args.old_reps} passes, on " + ("a build of the parent commit" if args.before_root else "this tree's library") + ".",
             "# loop = (a) tamp_amd_compress_resets once per stream, the same bytes as new (SHA-256 over all streams); plain = (b) tamp_batch_compress",
             "# without resets, one workgroup per stream, other bytes.  ratio = loop / new on the same route.", ""]
    worst = {}
    spread = {}
    for rnd in range(args.rounds):
        got = {}
        for which in ("new-device", "loop-device", "new-host", "loop-host", "plain-device", "plain-host"):
            got[which] = run(which)
        assert len({got[w]["sha256"] for w in ("new-device", "loop-device", "new-host", "loop-host")}) == 1, got
        fmt = lambda r: (f"{r['median_ms']:10.2f} ms [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  wall {r['wall_ms']:10.2f} ms "  # noqa: E731
                         f"{r['bytes'] / r['median_ms'] / 1e6:8.2f} GB/s")
        first = got["new-device"]
        lines.append(f"{first['streams']:,} streams, {first['bytes']:,} bytes -> {first['out_len']:,} with resets, {got['plain-device']['out_len']:,} without  run {rnd + 1}")
        for route in ("device", "host"):
            r = got[f"loop-{route}"]["median_ms"] / got[f"new-{route}"]["median_ms"]
            worst[route] = min(worst.get(route, r), r)
            spread.setdefault(route, []).append(got[f"loop-{route}"]["median_ms"])
            lines += [f"    new, {route:<7} {fmt(got['new-' + route])}   ratio {r:7.1f}",
                      f"    loop, {route:<6} {fmt(got['loop-' + route])}",
                      f"    plain, {route:<5} {fmt(got['plain-' + route])}"]
        print("\n".join(lines[-7:]), flush=True)
        tail = [""]
        for route in ("device", "host"):
            s = spread[route]
            tail.append(f"{route}: smallest loop / new ratio over all runs {worst[route]:.1f}; the loop's own medians spread {min(s):.2f} .. {max(s):.2f} ms "
                        f"(x{max(s) / min(s):.3f})")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # (after every run: a long session that is cut short keeps what it measured)
            f.write("\n".join(lines + tail) + "\n")
    if any(worst[route] <= max(spread[route]) / min(spread[route]) for route in worst):
        raise SystemExit("the new call did not beat the loop by more than the loop's own spread on every run")


if __name__ == "__main__":
    main()
