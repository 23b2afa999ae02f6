"""GPU tier: the fixed-geometry compress builds (window 2^10, literal 8, 1,024-position blocks, both formats) against the
generic build (TAMP_AMD_FIXED_BUILD=0) and the reference C / the oracle: status, length and bytes of every stream.

Inputs: the synthetic text, every distinct 4 KiB chunk of the three frozen corpora, one batch of mixed lengths 0..4,096
(below 16 bytes, and lengths that leave the last block short); tight output capacities; a non-default HIP stream.
"""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

L = 4096


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@pytest.fixture(scope="module")
def checker():
    from oracle.checker import Oracle, Ref

    return Ref() if Ref.available() else Oracle()


@contextlib.contextmanager
def generic_build():
    old = os.environ.get("TAMP_AMD_FIXED_BUILD")
    os.environ["TAMP_AMD_FIXED_BUILD"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["TAMP_AMD_FIXED_BUILD"]
        else:
            os.environ["TAMP_AMD_FIXED_BUILD"] = old


def planned_build(extended, max_in_len=L):
    from tamp_amd import _lib

    conf = _lib.TampAmdConf(10, 8, 0, int(extended), 0, 0, 0, 0)
    return _lib.load().tamp_amd_compress_build(ctypes.byref(conf), max_in_len, 0, 0)


def on_device(flat, off, ln):
    import torch

    dev = torch.device("cuda:0")
    return (torch.from_numpy(np.ascontiguousarray(flat)).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
            torch.from_numpy(ln.astype(np.int32)).to(dev))


def both_builds(ta, flat, off, ln, extended, **kw):
    """The same device batch through the fixed and the generic build -> (status, length, slab) of each, on the host."""
    import torch

    data, off_t, len_t = on_device(flat, off, ln)
    torch.cuda.synchronize()  # (the uploads ran on torch's current stream; the call may run on another)
    assert planned_build(extended) == (1 if extended else 2)
    fixed = ta.compress_batch(data, off_t, len_t, window=10, literal=8, extended=extended, max_in_len=L, **kw)
    torch.cuda.synchronize()
    with generic_build():
        assert planned_build(extended) == 0
        generic = ta.compress_batch(data, off_t, len_t, window=10, literal=8, extended=extended, max_in_len=L, **kw)
        torch.cuda.synchronize()
    return fixed, generic


def assert_same_three_ways(fixed, generic, want, n, what):
    fs, gs, ws = fixed.status.cpu().numpy(), generic.status.cpu().numpy(), np.asarray(want.status)
    fl, gl, wl_ = fixed.out_len.cpu().numpy(), generic.out_len.cpu().numpy(), np.asarray(want.out_len)
    assert (fs == gs).all() and (fs == ws).all(), (what, "status")
    assert (fl == gl).all() and (fl.astype(np.int64) == wl_.astype(np.int64)).all(), (what, "length")
    fo, go = fixed.out.cpu().numpy(), generic.out.cpu().numpy()
    foff, goff = fixed.out_off.cpu().numpy(), generic.out_off.cpu().numpy()
    for i in range(n):
        a = fo[int(foff[i]):int(foff[i]) + int(fl[i])].tobytes()
        b = go[int(goff[i]):int(goff[i]) + int(gl[i])].tobytes()
        assert a == b, (what, i, "fixed != generic")
        assert a == want.stream(i), (what, i, "fixed != reference")


@pytest.mark.parametrize("extended", [True, False])
def test_synthetic_text(ta, checker, extended):
    from tamp_amd import workloads as wl

    n = 2048
    rows = wl.synth_text(n, L)
    off, ln = wl.csr_for_fixed(n, L)
    fixed, generic = both_builds(ta, rows.reshape(-1), off, ln, extended)
    want = checker.compress_batch(rows.reshape(-1), off, ln, window=10, literal=8, extended=extended, threads=8)
    assert (np.asarray(want.status) == 0).all()
    assert_same_three_ways(fixed, generic, want, n, ("synth_text", extended))


@pytest.mark.parametrize("extended", [True, False])
@pytest.mark.parametrize("name", ["prose", "markup", "python"])
def test_every_distinct_chunk_of_the_frozen_corpora(ta, checker, name, extended):
    from tamp_amd import workloads as wl

    blob = wl.real_text(name, frozen_only=True)
    assert len(blob) >= 64 * L, "frozen corpus fixture missing"
    chunks = sorted({blob[i:i + L] for i in range(0, len(blob) - L + 1, L)})
    n = len(chunks)
    flat = np.frombuffer(b"".join(chunks), dtype=np.uint8)
    off, ln = wl.csr_for_fixed(n, L)
    fixed, generic = both_builds(ta, flat, off, ln, extended)
    want = checker.compress_batch(flat, off, ln, window=10, literal=8, extended=extended, threads=8)
    assert_same_three_ways(fixed, generic, want, n, (name, extended))


def mixed_streams():
    from tamp_amd import workloads as wl

    prose, py = wl.real_text("prose", frozen_only=True), wl.real_text("python", frozen_only=True)
    synth = wl.synth_text(64, L)
    lens = [0, 1, 2, 3, 4, 5, 7, 8, 9, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 255, 256, 257, 511, 1000, 1023, 1024, 1025, 1039, 1040,
            1041, 1087, 1088, 1500, 2047, 2048, 2049, 2063, 2064, 3000, 3071, 3072, 3073, 3100, 4000, 4079, 4080, 4081, 4095, 4096]
    rng = np.random.default_rng(11)
    lens += [int(x) for x in rng.integers(0, L + 1, 150)]
    out = []
    for i, n in enumerate(lens):
        kind = i % 5
        if kind == 0:
            s = prose[i * 5003:i * 5003 + n]
        elif kind == 1:
            s = py[i * 7001:i * 7001 + n]
        elif kind == 2:
            s = synth[i % 64].tobytes()[:n]
        elif kind == 3:  # long runs, runs that reach the end of the stream
            s = (b"a" * 300 + prose[i * 911:i * 911 + 200] + b" " * 90 + b"xy" * 50 + bytes(400))[:n]
            s = s + b"z" * (n - len(s))
        else:            # periodic data: extended matches that run into the window's end
            s = (py[i * 1301:i * 1301 + 37] * 120)[:n]
        assert len(s) == n
        out.append(s)
    return out


@pytest.mark.parametrize("extended", [True, False])
def test_mixed_lengths(ta, checker, extended):
    from tamp_amd.batch import pack_streams

    streams = mixed_streams()
    flat, off, ln = pack_streams(streams)
    if flat.size == 0:
        flat = np.zeros(1, np.uint8)
    fixed, generic = both_builds(ta, flat, off, ln, extended)
    want = checker.compress_batch(flat, off, ln, window=10, literal=8, extended=extended, threads=8)
    assert_same_three_ways(fixed, generic, want, len(streams), ("mixed", extended))
    # the same batch from host memory (the staging path plans the block from the lengths it sees)
    host = ta.compress_batch(streams, window=10, literal=8, extended=extended)
    for i in range(len(streams)):
        assert int(host.status[i]) == int(want.status[i]) and host.stream(i) == want.stream(i), (i, extended)


@pytest.mark.parametrize("extended", [True, False])
def test_tight_output_capacity(ta, checker, extended):
    """A stream whose output does not fit ends with TAMP_OUTPUT_FULL and the first `capacity` bytes of its stream; one whose
    capacity is exact ends with TAMP_OK.  Nothing is written behind a stream's capacity (the slabs are adjacent)."""
    import torch
    from tamp_amd import workloads as wl

    n = 96
    rows = wl.synth_text(n, L)
    off, ln = wl.csr_for_fixed(n, L)
    full = checker.compress_batch(rows.reshape(-1), off, ln, window=10, literal=8, extended=extended, threads=8)
    flen = np.asarray(full.out_len).astype(np.int64)
    caps = flen + 40
    tight = {0: 0, 1: -1, 2: -5, 7: -(int(flen[7]) // 2), 8: -int(flen[8]), 9: -(int(flen[9]) - 1), 40: -3, 41: 0, 95: -100}
    for i, d in tight.items():
        caps[i] = flen[i] + d
    data, off_t, len_t = on_device(rows.reshape(-1), off, ln)
    cap_t = torch.from_numpy(caps.astype(np.int32)).to(data.device)
    res = {}
    for tag in ("fixed", "generic"):
        with (generic_build() if tag == "generic" else contextlib.nullcontext()):
            r = ta.compress_batch(data, off_t, len_t, window=10, literal=8, extended=extended, max_in_len=L, out_cap=cap_t)
            torch.cuda.synchronize()
        res[tag] = r
    fx, gn = res["fixed"], res["generic"]
    assert bool((fx.status == gn.status).all()) and bool((fx.out_len == gn.out_len).all())
    for i in range(n):
        over = caps[i] < flen[i]
        st, _ = checker.compress(rows[i].tobytes(), window=10, literal=8, extended=extended, cap=int(caps[i]))[:2]
        assert int(fx.status[i]) == st == (1 if over else 0), (i, extended)
        assert int(fx.out_len[i]) == min(int(caps[i]), int(flen[i])), (i, extended)
        assert fx.stream(i) == gn.stream(i) == full.stream(i)[:int(fx.out_len[i])], (i, extended)


@pytest.mark.parametrize("extended", [True, False])
def test_on_a_side_stream(ta, checker, extended):
    import torch
    from tamp_amd import workloads as wl

    n = 1024
    rows = wl.synth_text(n, L, first_index=5000)
    off, ln = wl.csr_for_fixed(n, L)
    side = torch.cuda.Stream()
    fixed, generic = both_builds(ta, rows.reshape(-1), off, ln, extended, stream=side.cuda_stream)
    side.synchronize()
    want = checker.compress_batch(rows.reshape(-1), off, ln, window=10, literal=8, extended=extended, threads=8)
    assert_same_three_ways(fixed, generic, want, n, ("side stream", extended))
