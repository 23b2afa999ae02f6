"""GPU tier: the fixed-geometry compress builds on a STATIC LDS array, with the query sort's lengths counted by the scatter
(DESIGN.md 3.2, 3.3).  Window 2^10, literal 8, both formats, whole-stream batch calls -- the fixed builds' calls, asserted with
tamp_amd_compress_build -- and every stream compared with the reference C (the oracle where that was not built).

* Streams of sixteen lengths around the block and tile sizes in ONE launch, forwards and backwards, on a grid of one workgroup
  per CU: every persistent workgroup takes several streams of different shapes on the same static array.
* Inputs at the edges of the folded count: epochs cut at a run (queries pending behind the lag), brackets of 63 entries and
  more (the clamp, the deferral threshold), brackets of 0 and 1, and the first 64 chunks of each frozen corpus.
* The same batches through the generic build (TAMP_AMD_FIXED_BUILD=0) in a fresh child process: byte-identical.
* 2,048 streams launched twice on one stream into the same slab (``reuse=``): the second result equals the first.
"""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

L = 4096
LENGTHS = [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5000]
REPEATS = 40  # 640 streams over 256 workgroups


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@pytest.fixture(scope="module")
def checker():
    from oracle.checker import Oracle, Ref

    return Ref() if Ref.available() else Oracle()


@contextlib.contextmanager
def environment(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def planned_build(extended, max_in_len):
    from tamp_amd import _lib

    conf = _lib.TampAmdConf(10, 8, 0, int(extended), 0, 0, 0, 0)
    return _lib.load().tamp_amd_compress_build(ctypes.byref(conf), max_in_len, 0, 0)


def on_device(flat, off, ln):
    import torch

    dev = torch.device("cuda:0")
    return (torch.from_numpy(np.ascontiguousarray(flat)).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
            torch.from_numpy(ln.astype(np.int32)).to(dev))


def length_streams():
    """Every length REPEATS times, each time on other text; the lengths cycle, so neighbours in the batch differ in shape."""
    from tamp_amd import workloads as wl

    text = wl.synth_text(REPEATS, 5000 + len(LENGTHS), first_index=900)
    return [text[r].tobytes()[k:k + n] for r in range(REPEATS) for k, n in enumerate(LENGTHS)]


def edge_streams():
    from tamp_amd import workloads as wl

    text = wl.synth_text(2, L, first_index=77)
    t0 = text[0].tobytes()
    out = [b"a" * L,                                       # one byte repeated: every epoch is cut, the rest is pending
           t0[:1500] + b"x" * 60 + t0[1560:],              # a 60-byte run in the second kilobyte: an epoch cut, queries pending behind it
           (b"abc" * (L // 3 + 1))[:L],                    # three bigrams for 4 KiB: brackets far beyond 63 entries
           (b"aab" * (L // 3 + 1))[:L],                    # ... with short runs inside: the deferral threshold
           np.random.default_rng(3).integers(0, 256, L, dtype=np.uint8).tobytes()]  # brackets of 0 and 1
    for name in ("prose", "markup", "python"):
        blob = wl.real_text(name, frozen_only=True)
        assert len(blob) >= 64 * L, "frozen corpus fixture missing"
        out += [blob[i * L:(i + 1) * L] for i in range(64)]
    return out


BATCHES = {"lengths": (length_streams, 5000, {"TAMP_AMD_GRID_PER_CU": "1"}),
           "lengths_reversed": (lambda: length_streams()[::-1], 5000, {"TAMP_AMD_GRID_PER_CU": "1"}),
           "edges": (edge_streams, L, {})}


@pytest.fixture(scope="module")
def batches(checker):
    """name -> (flat, off, len, max_in_len, env, {extended: the checker's result}); computed once, read by every test."""
    from tamp_amd.batch import pack_streams

    out = {}
    for name, (make, max_in_len, env) in BATCHES.items():
        flat, off, ln = pack_streams(make())
        want = {e: checker.compress_batch(flat, off, ln, window=10, literal=8, extended=e, threads=8) for e in (True, False)}
        out[name] = (flat, off, ln, max_in_len, env, want)
    return out


def run_fixed(ta, flat, off, ln, max_in_len, env, extended):
    import torch

    data, off_t, len_t = on_device(flat, off, ln)
    torch.cuda.synchronize()
    assert planned_build(extended, max_in_len) == (1 if extended else 2)
    with environment(**env):
        res = ta.compress_batch(data, off_t, len_t, window=10, literal=8, extended=extended, max_in_len=max_in_len)
        torch.cuda.synchronize()
    return res


def streams_of(res):
    st, ln = res.status.cpu().numpy(), res.out_len.cpu().numpy()
    out, off = res.out.cpu().numpy(), res.out_off.cpu().numpy()
    return st, [out[int(off[i]):int(off[i]) + int(ln[i])].tobytes() for i in range(len(ln))]


@pytest.mark.parametrize("extended", [True, False])
@pytest.mark.parametrize("name", list(BATCHES))
def test_against_the_reference(ta, batches, name, extended):
    flat, off, ln, max_in_len, env, want = batches[name]
    st, got = streams_of(run_fixed(ta, flat, off, ln, max_in_len, env, extended))
    w = want[extended]
    assert (st == np.asarray(w.status)).all(), (name, extended, "status")
    for i in range(len(ln)):
        assert got[i] == w.stream(i), (name, extended, i, int(ln[i]))


CHILD = r"""
import ctypes, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import tamp_amd
from tamp_amd import _lib
z = np.load(sys.argv[2])
dev = torch.device("cuda:0")
out = {}
for name in [k[:-5] for k in z.files if k.endswith("_flat")]:
    data = torch.from_numpy(z[name + "_flat"]).to(dev)
    off_t = torch.from_numpy(z[name + "_off"].astype(np.int64)).to(dev)
    len_t = torch.from_numpy(z[name + "_len"].astype(np.int32)).to(dev)
    m = int(z[name + "_max"])
    for e in (1, 0):
        conf = _lib.TampAmdConf(10, 8, 0, e, 0, 0, 0, 0)
        assert _lib.load().tamp_amd_compress_build(ctypes.byref(conf), m, 0, 0) == 0, "the generic build"
        r = tamp_amd.compress_batch(data, off_t, len_t, window=10, literal=8, extended=bool(e), max_in_len=m)
        torch.cuda.synchronize()
        o, oo, ol = r.out.cpu().numpy(), r.out_off.cpu().numpy(), r.out_len.cpu().numpy()
        out["%s_%d_status" % (name, e)] = r.status.cpu().numpy()
        out["%s_%d_len" % (name, e)] = ol
        out["%s_%d_bytes" % (name, e)] = np.concatenate([o[int(a):int(a) + int(b)] for a, b in zip(oo, ol)] + [np.zeros(0, np.uint8)])
np.savez(sys.argv[3], **out)
"""


def test_generic_build_in_a_fresh_process_is_byte_identical(ta, batches, tmp_path):
    """Also the cross-check that the generic builds did not move: their LDS stays dynamic, their sort is the same code."""
    arrays = {}
    for name, (flat, off, ln, max_in_len, env, want) in batches.items():
        arrays.update({name + "_flat": flat, name + "_off": off, name + "_len": ln, name + "_max": np.int64(max_in_len)})
    np.savez(tmp_path / "in.npz", **arrays)
    env = dict(os.environ, TAMP_AMD_FIXED_BUILD="0")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    generic = np.load(tmp_path / "out.npz")
    for name, (flat, off, ln, max_in_len, env, want) in batches.items():
        for extended in (True, False):
            st, got = streams_of(run_fixed(ta, flat, off, ln, max_in_len, env, extended))
            key = "%s_%d_" % (name, int(extended))
            assert (st == generic[key + "status"]).all(), (name, extended)
            assert ([len(g) for g in got] == generic[key + "len"]).all(), (name, extended)
            assert b"".join(got) == generic[key + "bytes"].tobytes(), (name, extended)


@pytest.mark.parametrize("extended", [True, False])
def test_second_launch_into_the_same_slab(ta, extended):
    import torch
    from tamp_amd import workloads as wl

    n = 2048
    rows = wl.synth_text(n, L, first_index=3000)
    off, ln = wl.csr_for_fixed(n, L)
    data, off_t, len_t = on_device(rows.reshape(-1), off, ln)
    torch.cuda.synchronize()
    assert planned_build(extended, L) == (1 if extended else 2)
    cap = L * 9 // 8 + 16
    first = ta.compress_batch(data, off_t, len_t, window=10, literal=8, extended=extended, max_in_len=L, out_cap=cap)
    torch.cuda.synchronize()
    st1, got1 = streams_of(first)
    assert (st1 == 0).all()
    first.out.zero_()  # (the second launch has to write every byte again)
    second = ta.compress_batch(data, off_t, len_t, window=10, literal=8, extended=extended, max_in_len=L, out_cap=cap, reuse=first)
    torch.cuda.synchronize()
    assert second.out.data_ptr() == first.out.data_ptr(), "the slab was reused"
    st2, got2 = streams_of(second)
    assert (st2 == st1).all() and got2 == got1
