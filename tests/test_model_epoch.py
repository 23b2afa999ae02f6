"""CPU tier: the scalar model of the kernel's data structures (oracle/tamp_model.c) equals the oracle.

The HIP compressor keeps a linear history + speculative per-block find_best_match + epochs instead of the
reference's ring.  This checks that design, in scalar C, against the oracle for many block
sizes -- including blocks far smaller than the window and inputs that force a re-base after almost every token.
"""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

from oracle.checker import _OracleConf, _p, _u8
from tamp_amd import workloads as wl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from block_draggers import draggers  # noqa: E402


def _model(oracle, data, *, window, literal, extended, dictionary, blk):
    L = oracle.lib
    L.model_compress.restype = C.c_int
    L.model_compress.argtypes = [C.POINTER(_OracleConf), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                 C.POINTER(C.c_size_t), C.c_uint32, C.POINTER(C.c_uint)]
    a = _u8(data)
    conf = _OracleConf(window, literal, int(dictionary is not None), int(extended), 0, 0)
    cap = len(a) * 2 + 64
    out = np.zeros(cap, dtype=np.uint8)
    n, ne = C.c_size_t(0), C.c_uint(0)
    d = _u8(dictionary) if dictionary is not None else None
    r = L.model_compress(C.byref(conf), _p(d) if d is not None else None, _p(a), len(a), _p(out), cap, C.byref(n), blk,
                         C.byref(ne))
    return r, out[: n.value].tobytes(), ne.value


def test_model_equals_oracle(oracle):
    rng = random.Random(11)
    for it in range(400):
        w, lit = rng.randrange(8, 13), rng.randrange(5, 9)
        ext = rng.random() < 0.7
        n = rng.choice([0, 1, 2, 15, 16, 17, 33, 100, 256, 1000, 4096, rng.randrange(1, 6000)])
        kind = rng.randrange(4)
        if kind == 0:
            data = wl.synth_text(1, n, first_index=rng.randrange(1 << 20))[0].tobytes()
        elif kind == 1:
            data = wl.lcg_runs(1, n, first_index=rng.randrange(1 << 20))[0].tobytes()
        elif kind == 2:
            data = wl.stress(1, n, first_index=rng.randrange(1 << 20))[0].tobytes()
        else:
            data = bytes(rng.randrange(256) for _ in range(n))
        if lit < 8 and rng.random() < 0.9:
            data = bytes(b & ((1 << lit) - 1) for b in data)
        d = None
        if rng.random() < 0.3:
            d = (wl.synth_text(1, 1 << w, first_index=it)[0].tobytes())[: 1 << w]
        blk = rng.choice([16, 64, 100, 256, 1024, 2048, 4096])
        want = oracle.compress(data, window=w, literal=lit, extended=ext, dictionary=d)
        got = _model(oracle, data, window=w, literal=lit, extended=ext, dictionary=d, blk=blk)
        assert got[:2] == want, (it, w, lit, ext, n, blk)


def test_epochs_per_stream_on_text(oracle):
    """The speculation rarely breaks on text: about one epoch per block (what the kernel's cost model assumes)."""
    rows = wl.synth_text(32, 4096)
    eps = [_model(oracle, r.tobytes(), window=10, literal=8, extended=True, dictionary=None, blk=2048)[2] for r in rows]
    assert 2 <= np.mean(eps) < 2.6
    eps = [_model(oracle, r.tobytes(), window=10, literal=8, extended=False, dictionary=None, blk=2048)[2] for r in rows]
    assert set(eps) == {2}


@pytest.mark.parametrize("extended", [True, False])
def test_model_equals_oracle_on_the_block_draggers(oracle, extended):
    """The inputs of tests/test_gpu_block_geometry.py (features at periods coprime to 64, 4,625 bytes: more than two of the largest
    blocks) through the model at both ends of the one-wavefront and the four-wavefront block ranges and around 1,024: a
    mismatch the GPU tier reports at these blocks is then the kernel's or the launcher's, not the design's or the inputs'."""
    for name, data in draggers(4625).items():
        want = oracle.compress(data, window=10, literal=8, extended=extended)
        assert want[0] == 0
        for blk in (64, 448, 960, 1024, 1088, 1984, 2048):
            got = _model(oracle, data, window=10, literal=8, extended=extended, dictionary=None, blk=blk)
            assert got[:2] == want, (name, extended, blk)
