"""GPU tier: every build of the compress kernel the library launches (CompressBuild, tamp_amd/csrc/tamp_compress_plan.hpp),
once each, at the smallest shape that reaches it: status, length and bytes of every stream against the reference C / the
oracle, and the batch once through the device decoder.

The launcher picks the build from the window, the parse, the format, the longest stream and three tuning variables; the
host-only queries report the same plan (tests/test_compress_plan_golden.py), and each case first asserts the part of it that
the public calls show: TAMP_AMD_BUILD_* and the threads per workgroup.  Block mode is the launcher's own decision (one v1 stream of
256 KiB and more).

What this file cannot see: no public call reports whether block mode was taken, nor which of the generic instantiations ran,
and another build gives the same bytes.  That a call SELECTS the build named here is covered by the plan alone -- the asserts
on the two queries below and tests/test_compress_plan_golden.py; what is checked here is that every shape that reaches a
build comes back with the reference's bytes.
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

from block_draggers import draggers  # noqa: E402

GENERIC, FIXED_EXT, FIXED_V1 = 0, 1, 2  # include/tamp_amd.h TAMP_AMD_BUILD_*
TUNING_ENV = ("TAMP_AMD_BLK", "TAMP_AMD_RUNS", "TAMP_AMD_FIXED_BUILD", "TAMP_AMD_BLOCK_LEAN", "TAMP_AMD_BLOCK_MIN", "TAMP_AMD_CUT_RUN",
              "TAMP_AMD_LPT", "TAMP_AMD_STATIC_GRID", "TAMP_AMD_GRID_PER_CU")
NAMES = ("text", "prose", "runs67", "repeat131", "period37", "lcg_runs", "stress_runs", "stress_repeats")
N_LONG, N_SHORT, N_BLOCK = 1100, 256, 300000


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


# ---- inputs and expected bytes, computed once and shared (never modified) -------------------------------------------
_streams, _expected = {}, {}


def streams(n):
    if n not in _streams:
        if n == N_BLOCK:  # one long stream: prose, then synthetic text
            from tamp_amd import workloads as wl

            prose = wl.real_text("prose", frozen_only=True)[12345:12345 + 240000]
            _streams[n] = [prose + wl.synth_text(1, n - len(prose))[0].tobytes()]
        else:
            d = draggers(n)
            _streams[n] = [d[k] for k in NAMES]
        assert all(len(s) == n for s in _streams[n])
    return _streams[n]


def expected(checker, n, window, extended, lazy):
    from tamp_amd.batch import pack_streams

    key = (n, window, extended, lazy)
    if key not in _expected:
        flat, off, ln = pack_streams(streams(n))
        want = checker.compress_batch(flat, off, ln, window=window, literal=8, extended=extended, lazy=lazy, threads=8)
        assert (np.asarray(want.status) == 0).all(), (key, "the checker refuses an input")
        _expected[key] = [want.stream(i) for i in range(len(streams(n)))]
    return _expected[key]


def planned(window, extended, lazy, max_in_len):
    """-> (TAMP_AMD_BUILD_*, threads per workgroup) of a plain batch call under the current environment."""
    from tamp_amd import _lib

    lib = _lib.load()
    conf = _lib.TampAmdConf(window, 8, 0, int(extended), 0, int(lazy), 0, 0)
    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert lib.tamp_amd_compress_plan(window, max_in_len, int(lazy), *[ctypes.byref(x) for x in v]) == 0
    return lib.tamp_amd_compress_build(ctypes.byref(conf), max_in_len, 0, 0), v[2].value


def run_batch(ta, checker, n, window, extended, lazy, what):
    """One device batch of streams(n): status 0, length and bytes as the checker's, and the device decoder gives the input back."""
    import torch
    from tamp_amd.batch import compress_bound, pack_streams

    want = expected(checker, n, window, extended, lazy)
    flat, off, ln = pack_streams(streams(n))
    dev = torch.device("cuda:0")
    data = torch.from_numpy(np.ascontiguousarray(flat)).to(dev)
    off_t, len_t = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev)
    res = ta.compress_batch(data, off_t, len_t, window=window, literal=8, extended=extended, lazy_matching=lazy, max_in_len=n,
                            out_cap=compress_bound(n, 8))
    torch.cuda.synchronize()
    status, out_len = res.status.cpu().numpy(), res.out_len.cpu().numpy()
    out, out_off = res.out.cpu().numpy(), res.out_off.cpu().numpy()
    assert (status == 0).all(), (what, "status", status.tolist())
    for i, w in enumerate(want):
        assert int(out_len[i]) == len(w), (what, i, "length", int(out_len[i]), len(w))
        assert out[int(out_off[i]):int(out_off[i]) + len(w)].tobytes() == w, (what, i, "bytes")
    back = ta.decompress_batch(res.out, res.out_off, res.out_len, out_cap=n + 8)
    torch.cuda.synchronize()
    bstatus, blen = back.status.cpu().numpy(), back.out_len.cpu().numpy()
    bout, boff = back.out.cpu().numpy(), back.out_off.cpu().numpy()
    assert (bstatus == 2).all(), (what, "decoder status", bstatus.tolist())
    for i, s in enumerate(streams(n)):
        assert bout[int(boff[i]):int(boff[i]) + int(blen[i])].tobytes() == s, (what, i, "round trip")


# build: (stream length, window, extended, lazy, environment) -> (TAMP_AMD_BUILD_*, threads)
BATCH_BUILDS = {
    "short_lean": ((N_SHORT, 10, True, False, {}), (GENERIC, 64)),
    "lean_u16": ((N_LONG, 15, True, False, {}), (GENERIC, 256)),
    "lazy_packed": ((N_LONG, 10, True, True, {}), (GENERIC, 256)),
    "lazy_u16": ((N_LONG, 15, True, True, {}), (GENERIC, 256)),
    "runs": ((N_LONG, 11, True, False, {}), (GENERIC, 256)),
    "runs_1024": ((N_LONG, 10, True, False, {"TAMP_AMD_FIXED_BUILD": "0"}), (GENERIC, 256)),
    "fixed_ext": ((N_LONG, 10, True, False, {}), (FIXED_EXT, 256)),
    "fixed_v1": ((N_LONG, 10, False, False, {}), (FIXED_V1, 256)),
}


@pytest.mark.parametrize("build", list(BATCH_BUILDS))
def test_batch_build(ta, checker, monkeypatch, build):
    (n, window, extended, lazy, env), want_plan = BATCH_BUILDS[build]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert planned(window, extended, lazy, n) == want_plan, build
    run_batch(ta, checker, n, window, extended, lazy, build)


BLOCK_BUILDS = {
    "block_runs_1024": (10, {}),
    "block_runs": (11, {}),
    "block_lean": (10, {"TAMP_AMD_BLOCK_LEAN": "1"}),
}


@pytest.mark.parametrize("build", list(BLOCK_BUILDS))
def test_block_mode_build(ta, checker, monkeypatch, build):
    """One v1 stream of 300,000 bytes, literal 8: over the 256 KiB threshold, so the launcher spreads its 293 blocks of 1,024
    positions over all workgroups in three passes."""
    window, env = BLOCK_BUILDS[build]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run_batch(ta, checker, N_BLOCK, window, False, False, build)
