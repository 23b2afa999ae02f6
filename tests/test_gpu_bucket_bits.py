"""GPU tier: the fixed-geometry compress builds with their bucket scan's candidate lengths in bit units (a candidate's class read
off the first set bit of its entry's XOR, the 16-byte compare capped at 128 bits, one shared shift) against the reference C (the
oracle where that was not built): status, length and bytes of every stream.

The calls are the ones tamp_amd_compress_build names as the fixed builds (window 10, literal 8, default parse, max_in_len 4,096,
both formats), which is asserted.  The inputs are tests/bucket_bits_input.py's cells -- every common prefix 2..16, the two forms of
3, the oldest window byte, one and two 16-byte hits, the wrap zone at every distance 2..16 in each class, equal lengths at several
window indices -- each with 16 and more bytes of look-ahead and once within its stream's last 15 bytes, every stream four times in
its batch at the batch offsets in_off = 0, 1, 2, 3 (mod 4).  TAMP_AMD_FIXED_BUILD=0 sends the same call through the generic build,
whose scan keeps the byte form: the same bytes.

Checked on the CPU (tests/test_bucket_bits_input.py, from the oracle's token trace): every cell's token at the query position has
the stated kind, length and window index.
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

import bucket_bits_input as bbi  # noqa: E402

L = 4096
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
    """The one batch every test compresses: (cells, flat, in_off, in_len, which), never modified."""
    cells = bbi.cells()
    return (cells,) + bbi.layout([c.data for c in cells])


_want = {}


@pytest.fixture(scope="module")
def want(checker, batch):
    """The checker's streams per format, computed once."""
    def get(extended):
        if extended not in _want:
            cells, flat, off, ln, which = batch
            r = checker.compress_batch(flat, off, ln, window=10, literal=8, extended=extended, threads=8)
            assert (np.asarray(r.status) == 0).all()
            _want[extended] = [r.stream(i) for i in range(len(which))]
        return _want[extended]
    return get


def planned_build(extended):
    from tamp_amd import _lib

    conf = _lib.TampAmdConf(10, 8, 0, int(extended), 0, 0, 0, 0)
    return _lib.load().tamp_amd_compress_build(ctypes.byref(conf), L, 0, 0)


def compress(ta, batch, extended):
    import torch
    from tamp_amd.batch import compress_bound

    cells, flat, off, ln, which = batch
    dev = torch.device("cuda:0")
    data = torch.from_numpy(np.ascontiguousarray(flat)).to(dev)
    off_t, len_t = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev)
    res = ta.compress_batch(data, off_t, len_t, window=10, literal=8, extended=extended, max_in_len=L, out_cap=compress_bound(L, 8))
    torch.cuda.synchronize()
    status, out_len = res.status.cpu().numpy(), res.out_len.cpu().numpy()
    out, out_off = res.out.cpu().numpy(), res.out_off.cpu().numpy()
    return status, [out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(len(which))]


def check(batch, status, got, want):
    cells, flat, off, ln, which = batch
    assert len(which) == 4 * len(cells) and sorted(set(int(o) % 4 for o in off)) == [0, 1, 2, 3]
    assert (status == 0).all(), ("status", [(cells[which[i][0]].name, which[i][1], int(status[i])) for i in np.flatnonzero(status)][:4])
    for i, (k, r) in enumerate(which):
        assert len(got[i]) == len(want[i]), (cells[k].name, r, "length", len(got[i]), len(want[i]))
        assert got[i] == want[i], (cells[k].name, r, "bytes")


@pytest.mark.parametrize("extended", [True, False], ids=["ext", "v1"])
def test_fixed_builds_on_every_cell_at_every_offset(ta, batch, want, extended):
    assert planned_build(extended) == (1 if extended else 2), "the fixed-geometry build"
    status, got = compress(ta, batch, extended)
    check(batch, status, got, want(extended))


@pytest.mark.parametrize("extended", [True, False], ids=["ext", "v1"])
def test_generic_build_gives_the_same_bytes(ta, batch, want, extended, monkeypatch):
    monkeypatch.setenv("TAMP_AMD_FIXED_BUILD", "0")
    assert planned_build(extended) == 0, "a generic build"
    status, got = compress(ta, batch, extended)
    check(batch, status, got, want(extended))
