"""One long buffer as dictionary-reset segments against the route to the same bytes that existed before: dev tool.

Workload: the frozen prose corpus tiled to 32,000,000 and 100,000,000 bytes, window 10, literal 8, extended format, a reset every
64 KiB.  Timed with hipEvents around each call (torch events on the default stream; the host-memory calls are synchronous, so the
pair spans them), median of the last ten of twelve:
  new, device   tamp_amd_compress_resets, device memory: kernels only
  new, host     tamp_amd_compress_resets, host memory: staging included -- what compress(..., reset_interval=N) runs
  before        the Compressor object: write(64 KiB) / reset_dictionary() ... flush(False), host memory, one workgroup
and, reading the blob back from host memory (`tamp_amd.decompress(blob)`, size query included):
  decode new    this tree: tamp_amd_decompress_resets, the segments as one batch
  decode before the parent's route for a blob with the reset bit: the decoder object
(`--before-decode-reps R`: the `decode before` runs make R calls and take the median of the last R - 2; default twelve.)
Every run is a fresh process; new and before alternate, three times.  `--before-root PATH`: a built checkout of the parent commit
whose package the `before` runs import (without it they run this tree, whose object path is the same code).  The three blobs of a
size must be the same bytes (SHA-256).

    python tools/resets_bench.py [--out profiles/reset_segments_bench.txt] [--before-root ../parent-checkout]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("RESETS_BENCH_ROOT") or ROOT)  # (the `before` runs: --before-root)
SIZES = (32_000_000, 100_000_000)
INTERVAL = 64 << 10
REPS, KEEP = 12, 10


def corpus(n):
    from tamp_amd import workloads as wl

    raw = wl.frozen_corpus("prose")
    assert raw, "tests/golden/corpus_prose.txt.xz is part of the tree"
    return (raw * (n // len(raw) + 1))[:n]


def child(which, n):
    import ctypes as C
    from io import BytesIO

    import numpy as np
    import torch

    import tamp_amd
    from tamp_amd import _lib

    lib = _lib.load()
    data = corpus(n)
    ms, blob = [], b""
    reps, keep = REPS, KEEP

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        return r

    if which.startswith("decode"):
        packed = open(os.environ["RESETS_BENCH_BLOB"], "rb").read()
        if which == "decode-before":
            reps = int(os.environ.get("RESETS_BENCH_DECODE_REPS", REPS))
            keep = max(reps - 2, 1)
        for _ in range(reps):
            blob = bytes(timed(lambda: tamp_amd.decompress(packed)))
        assert blob == data
    elif which == "before":
        def run():
            with BytesIO() as f:
                c = tamp_amd.Compressor(f, dictionary_reset=True)
                for at in range(0, max(n, 1), INTERVAL):
                    if at:
                        c.reset_dictionary()
                    c.write(data[at : at + INTERVAL])
                c.flush(write_token=False)
                return f.getvalue()
        for _ in range(REPS):
            blob = timed(run)
    else:
        conf = _lib.TampAmdConf(10, 8, 0, 1, 1, 0)
        cap = lib.tamp_amd_compress_resets_bound(n, INTERVAL, 8)
        src = np.frombuffer(data, dtype=np.uint8)
        if which == "new-device":
            dev = torch.device("cuda:0")
            t_src, t_out = torch.from_numpy(src.copy()).to(dev), torch.empty(cap, dtype=torch.uint8, device=dev)
            t_len, t_status = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int8, device=dev)
            for _ in range(REPS):
                rc = timed(lambda: lib.tamp_amd_compress_resets(C.byref(conf), t_src.data_ptr(), n, INTERVAL, t_out.data_ptr(), cap,
                                                                t_len.data_ptr(), t_status.data_ptr(), None, _lib.MEM_DEVICE, 0, None))
                assert rc == 0 and int(t_status.cpu()[0]) == 0
            blob = t_out[: int(t_len.cpu()[0])].cpu().numpy().tobytes()
        else:
            out = np.empty(cap, dtype=np.uint8)
            out_len, status = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int8)
            p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
            for _ in range(REPS):
                rc = timed(lambda: lib.tamp_amd_compress_resets(C.byref(conf), p(src), n, INTERVAL, p(out), cap, p(out_len), p(status),
                                                                None, _lib.MEM_HOST, 0, None))
                assert rc == 0 and int(status[0]) == 0
            blob = out[: int(out_len[0])].tobytes()
    if os.environ.get("RESETS_BENCH_BLOB") and which == "new-host":
        with open(os.environ["RESETS_BENCH_BLOB"], "wb") as fh:
            fh.write(blob)
    kept = sorted(ms[-keep:])
    print(json.dumps(dict(which=which, n=n, median_ms=(kept[(keep - 1) // 2] + kept[keep // 2]) / 2, min_ms=kept[0], max_ms=kept[-1],
                          out_len=len(blob), sha256=hashlib.sha256(blob).hexdigest(), lib=_lib.LIB_PATH)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reset_segments_bench.txt"))
    ap.add_argument("--before-root", default=None)
    ap.add_argument("--before-decode-reps", type=int, default=REPS)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--skip-compress-before", action="store_true", help="decode columns only: the object script is not run")
    ap.add_argument("--child", nargs=2, default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]))

    import tempfile

    blob_path = os.path.join(tempfile.mkdtemp(), "blob.tamp")

    def run(which, n):
        env = dict(os.environ, RESETS_BENCH_BLOB=blob_path, RESETS_BENCH_DECODE_REPS=str(args.before_decode_reps))
        if which in ("before", "decode-before") and args.before_root:
            env["RESETS_BENCH_ROOT"] = os.path.abspath(args.before_root)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, str(n)], env=env, capture_output=True,
                           text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit(f"{which} {n}: exit {p.returncode}\n{p.stderr[-2000:]}")
        return json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])

    lines = ["# tools/resets_bench.py: prose corpus tiled, window 10, literal 8, extended, a reset every 65,536 bytes; hipEvents around each",
             "# call, median of the last ten of twelve calls in a fresh process (min .. max in brackets); `before`: the Compressor object",
             "# script on " + ("a build of the parent commit" if args.before_root else "this tree's library"),
             "# ratio = before / new.  The three blobs of a size are the same bytes.  decode: tamp_amd.decompress(blob) from host memory, size",
             f"# query included, on both trees; `decode before` makes {args.before_decode_reps} calls per process and takes the median of the last {max(args.before_decode_reps - 2, 1)}.", ""]
    worst = worst_dec = None
    for n in args.sizes:
        for rnd in range(3):
            new_d, new_h = run("new-device", n), run("new-host", n)
            old = new_h if args.skip_compress_before else run("before", n)
            assert new_d["sha256"] == new_h["sha256"] == old["sha256"], (new_d, new_h, old)
            dec_new, dec_old = run("decode-new", n), run("decode-before", n)
            assert dec_new["sha256"] == dec_old["sha256"]
            r_dec = dec_old["median_ms"] / dec_new["median_ms"]
            worst_dec = r_dec if worst_dec is None else min(worst_dec, r_dec)
            r_h, r_d = old["median_ms"] / new_h["median_ms"], old["median_ms"] / new_d["median_ms"]
            worst = r_h if worst is None else min(worst, r_h)
            fmt = lambda r: f"{r['median_ms']:10.2f} ms [{r['min_ms']:.2f} .. {r['max_ms']:.2f}] {n / r['median_ms'] / 1e3:8.1f} MB/s"  # noqa: E731
            lines += [f"{n:>11,} bytes -> {old['out_len']:,}  run {rnd + 1}",
                      f"    before      {fmt(old)}",
                      f"    new, host   {fmt(new_h)}   ratio {r_h:7.1f}",
                      f"    new, device {fmt(new_d)}   ratio {r_d:7.1f}",
                      f"    decode before {fmt(dec_old)}   ({args.before_decode_reps} calls)",
                      f"    decode new    {fmt(dec_new)}   ratio {r_dec:7.1f}"]
            if args.skip_compress_before:
                del lines[-5]
            print("\n".join(lines[-6:]), flush=True)
    lines += ["", f"smallest before / new-host ratio over all runs: compress {worst:.1f}, decode {worst_dec:.1f}"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if (worst <= 1.0 and not args.skip_compress_before) or worst_dec <= 1.0:
        raise SystemExit("the new path did not beat the old one on every run")


if __name__ == "__main__":
    main()
