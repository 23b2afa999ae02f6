"""GPU tier: the fixed-geometry compress builds after the changes around their bucket scan -- patterns loaded from one aligned
base, the histogram pass split into full quads and one tail quad with a packed `qstart` store, constant-trip loops as straight-line
stores -- against the reference C (the oracle where that was not built): status, length and bytes of every stream.

The calls are the ones tamp_amd_compress_build names as the fixed builds (window 10, literal 8, default parse, max_in_len 4,096,
both formats), which is asserted.  The inputs are tests/query_setup_input.py's: three texts at 38 lengths (1..9, 1021..1031,
2045..2055, 4090..4096), each stream four times in its batch, once at every batch offset in_off = 0, 1, 2, 3 (mod 4), with
filler bytes in the gaps; the copies must agree with one another and with the checker.  456 streams per format.

Checked on the CPU (tests/test_query_setup_input.py, from the oracle's token trace): the run text gives RLE tokens that write
fewer bytes than they consume in every epoch of 1,024 positions, with the positions behind them at every residue mod 4, and
extended matches; the period-2 text gives matches from the first epoch on (its third token is one); the runs have the stated
lengths and period.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

import query_setup_input as qsi  # noqa: E402

TUNING_ENV = ("TAMP_AMD_BLK", "TAMP_AMD_RUNS", "TAMP_AMD_FIXED_BUILD", "TAMP_AMD_CUT_RUN", "TAMP_AMD_LPT", "TAMP_AMD_STATIC_GRID",
              "TAMP_AMD_BLOCK_MIN", "TAMP_AMD_GRID_PER_CU")


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@pytest.fixture(scope="module")
def checker():
    from oracle.checker import Oracle, Ref

    return Ref() if Ref.available() else Oracle()


@pytest.fixture(autouse=True)
def no_tuning_env(monkeypatch):
    for k in TUNING_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def batch():
    """The one batch both formats compress: (items, flat, in_off, in_len), never modified."""
    its = qsi.items()
    return (its,) + qsi.layout(its)


def planned_build(extended):
    from tamp_amd import _lib

    conf = _lib.TampAmdConf(10, 8, 0, int(extended), 0, 0, 0, 0)
    return _lib.load().tamp_amd_compress_build(ctypes.byref(conf), qsi.L, 0, 0)


@pytest.mark.parametrize("extended", [True, False], ids=["ext", "v1"])
def test_fixed_builds_on_tail_quads_runs_and_offsets(ta, checker, batch, extended):
    import torch
    from tamp_amd.batch import compress_bound

    its, flat, off, ln = batch
    assert len(its) == len(qsi.TEXTS) * len(qsi.LENGTHS) * 4 and sorted(set(int(o) % 4 for o in off)) == [0, 1, 2, 3]
    assert planned_build(extended) == (1 if extended else 2), "the fixed-geometry build"
    want = checker.compress_batch(flat, off, ln, window=10, literal=8, extended=extended, threads=8)
    assert (np.asarray(want.status) == 0).all()

    dev = torch.device("cuda:0")
    data = torch.from_numpy(np.ascontiguousarray(flat)).to(dev)
    off_t, len_t = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev)
    res = ta.compress_batch(data, off_t, len_t, window=10, literal=8, extended=extended, max_in_len=qsi.L,
                            out_cap=compress_bound(qsi.L, 8))
    torch.cuda.synchronize()
    status, out_len = res.status.cpu().numpy(), res.out_len.cpu().numpy()
    out, out_off = res.out.cpu().numpy(), res.out_off.cpu().numpy()
    assert (status == 0).all(), ("status", [(its[i], int(status[i])) for i in np.flatnonzero(status)][:4])
    got = {}
    for i, it in enumerate(its):
        assert int(out_len[i]) == len(want.stream(i)), (it, "length", int(out_len[i]), len(want.stream(i)))
        got[it] = out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes()
        assert got[it] == want.stream(i), (it, "bytes")
    for t, n, r in its:  # the copies of a stream agree, whatever their offset
        assert got[(t, n, r)] == got[(t, n, 0)], (t, n, r, "copies differ")
