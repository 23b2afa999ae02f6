"""Packing a batch's streams densely on the device (tamp_batch_pack) against a plain copy and against shipping the slabs: dev tool.

Three batches, each compressed once on the device into worst-case slabs:
  configs[1]   65,536 x 4 KiB synthetic text, window 10, literal 8
  telemetry    1,048,576 x 256 B telemetry messages, window 8, literal 7, the shared custom dictionary (configs[4])
  ragged       the batch of tools/batch_resets_bench.py: 2,000 streams of 8 KiB .. 4 MiB of prose, without resets
Per batch, in ONE process, after warm-up, the two sides of every comparison alternating:
  pack         ``BatchResult.packed(out=...)`` (one asynchronous call into a buffer of exactly the packed size), device events
  copy         ``copy_`` of as many contiguous bytes from one device buffer to another, device events
  slabs D2H    the whole slab buffer to pinned host memory: the only bulk way out there was
  packed D2H   ``BatchResult.packed()`` (size query, one ``.item()``, allocation, copy call) and its ``data`` to pinned host memory
  (the last two: wall clock, the device drained at both ends)
and for the first 4,096 streams of configs[1] ``BatchResult.streams()`` (a copy per stream) against ``packed().streams()``.
The bytes a pack must move are counted from the shapes: the packed bytes read and written, 12 bytes of tables read and 8 written per
stream.  The tool fails when, on configs[1], packed D2H does not beat slabs D2H by more than the spread of the two.

    python tools/pack_bench.py [--out profiles/pack_bench.txt] [--reps 10] [--shapes configs1,telemetry,ragged]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def compressed(shape, dev):
    """-> (description, BatchResult on the device)"""
    import numpy as np
    import torch

    import tamp_amd
    from tamp_amd import workloads as wl

    if shape == "configs1":
        n, L = 65536, 4096
        data = torch.from_numpy(wl.synth_text(n, L).reshape(-1)).to(dev)
        off, length = torch.arange(n, dtype=torch.int64, device=dev) * L, torch.full((n,), L, dtype=torch.int32, device=dev)
        return f"configs[1]: {n:,} x {L:,} B synthetic text, w=10 l=8", tamp_amd.compress_batch(data, off, length, max_in_len=L)
    if shape == "telemetry":
        n, L = 1 << 20, 256
        dic = wl.telemetry_dictionary(bytes(tamp_amd.initialize_dictionary(256, literal=7)))
        data = torch.from_numpy(wl.telemetry(n, L).reshape(-1)).to(dev)
        off, length = torch.arange(n, dtype=torch.int64, device=dev) * L, torch.full((n,), L, dtype=torch.int32, device=dev)
        return (f"telemetry: {n:,} x {L} B messages, w=8 l=7, shared custom dictionary",
                tamp_amd.compress_batch(data, off, length, window=8, literal=7, dictionary=dic, max_in_len=L))
    from batch_resets_bench import LONGEST, workload

    flat, in_off, in_len = workload()
    caps = torch.from_numpy(np.array([tamp_amd.compress_bound(int(x)) for x in in_len], dtype=np.int64)).to(dev)
    res = tamp_amd.compress_batch(torch.from_numpy(flat).to(dev), torch.from_numpy(in_off.view(np.int64)).to(dev),
                                  torch.from_numpy(in_len.view(np.int32)).to(dev), out_cap=caps, max_in_len=LONGEST)
    return f"ragged: {len(in_len):,} streams of 8 KiB .. 4 MiB of prose, w=10 l=8, no resets", res


def med(v):
    v = sorted(v)
    return (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2


def measure(shape, reps, lines):
    import torch

    import tamp_amd

    dev = torch.device("cuda:0")
    what, res = compressed(shape, dev)
    torch.cuda.synchronize()
    assert bool((res.status == 0).all().item())
    n, slab = int(res.out_len.numel()), int(res.out.numel())
    first = res.packed()
    total = int(first.off[-1])
    assert first.data.numel() == total == int((res.out_len.to(torch.int64) & 0xFFFFFFFF).sum().item())
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    plain_src = first.data.clone()
    plain_dst = torch.empty_like(plain_src)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    pack_ms, copy_ms = [], []
    for i in range(3 + reps):
        a, b = events(lambda: res.packed(out=out)), events(lambda: plain_dst.copy_(plain_src))
        if i >= 3:
            pack_ms.append(a), copy_ms.append(b)
    assert torch.equal(out, first.data)
    moved = 2 * total + 20 * n
    lines += [what,
              f"    slabs {slab:,} B, packed {total:,} B ({total / n:,.1f} B per stream, {100.0 * total / slab:.1f} % of the slabs)",
              f"    pack         {med(pack_ms):9.3f} ms [{min(pack_ms):.3f} .. {max(pack_ms):.3f}]   {moved:,} B moved (2 x packed + 20 B per stream): {moved / med(pack_ms) / 1e6:8.1f} GB/s",
              f"    copy         {med(copy_ms):9.3f} ms [{min(copy_ms):.3f} .. {max(copy_ms):.3f}]   {2 * total:,} B moved: {2 * total / med(copy_ms) / 1e6:8.1f} GB/s   pack / copy {med(pack_ms) / med(copy_ms):.2f}"]
    del out, plain_src, plain_dst
    pin_slab = torch.empty(slab, dtype=torch.uint8, pin_memory=True)
    pin_packed = torch.empty(total, dtype=torch.uint8, pin_memory=True)

    def ship_packed():
        p = res.packed()
        pin_packed.copy_(p.data, non_blocking=True)

    slab_ms, packed_ms = [], []
    for i in range(2 + reps):
        a, b = wall(lambda: pin_slab.copy_(res.out, non_blocking=True)), wall(ship_packed)
        if i >= 2:
            slab_ms.append(a), packed_ms.append(b)
    assert bytes(pin_packed[:64].numpy()) == bytes(first.data[:64].cpu().numpy())
    gain = med(slab_ms) - med(packed_ms)
    spread = (max(slab_ms) - min(slab_ms)) + (max(packed_ms) - min(packed_ms))
    lines += [f"    slabs D2H    {med(slab_ms):9.3f} ms [{min(slab_ms):.3f} .. {max(slab_ms):.3f}]   {slab / med(slab_ms) / 1e6:8.1f} GB/s over the link",
              f"    packed D2H   {med(packed_ms):9.3f} ms [{min(packed_ms):.3f} .. {max(packed_ms):.3f}]   pack included; {med(slab_ms) / med(packed_ms):.2f} x the slabs' way out; "
              f"gain {gain:.3f} ms, spread of the two {spread:.3f} ms"]
    ok = gain > spread
    if shape == "configs1":
        k = 4096
        part = tamp_amd.BatchResult(res.out, res.out_off[:k], res.out_len[:k], res.status[:k])
        part.streams(), part.packed().streams()
        a, b = wall(part.streams), wall(lambda: part.packed().streams())
        assert part.streams() == part.packed().streams()
        lines.append(f"    {k:,} streams to the host: BatchResult.streams() {a:.1f} ms, packed().streams() {b:.1f} ms")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_bench.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="configs1,telemetry,ragged")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "pack_bench.py measures on a GPU: there is nothing to report without one"
    lines = ["# tools/pack_bench.py: tamp_batch_pack through BatchResult.packed on one MI355X, one process per run, the two sides of every",
             f"# comparison alternating; median of {args.reps} after warm-up (min .. max in brackets).  pack, copy: device events; D2H rows: wall",
             "# clock with the device drained at both ends, pinned destinations.  GB/s = bytes moved (counted from the shapes) / median.", ""]
    failed = []
    for shape in args.shapes.split(","):
        shown = len(lines)
        if not measure(shape, args.reps, lines) and shape == "configs1":
            failed.append(shape)
        print("\n".join(lines[shown:]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # (after every shape: a run that is cut short keeps what it measured)
            f.write("\n".join(lines) + "\n")
        torch.cuda.empty_cache()
    if failed:
        raise SystemExit("configs[1]: packed D2H did not beat slabs D2H by more than the spread of the two")


if __name__ == "__main__":
    main()
