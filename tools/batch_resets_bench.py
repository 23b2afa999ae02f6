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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_resets_bench.txt"))
    ap.add_argument("--before-root", default=None)
    ap.add_argument("--old-reps", type=int, default=REPS)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", nargs=2, default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]))

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
