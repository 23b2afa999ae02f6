"""GPU tier: the run list of the run-aware compress builds -- the second pass's run-interior candidates and what happens when an
epoch holds more long runs than the list has slots (kRunCap) -- against the reference C (the oracle when the reference library
is not built): status and bytes of every stream, bit-exact.

The inputs are tests/run_list_input.py's; tests/test_run_list_input.py proves from the reference's own tokens that they aim
where they say:
  family A   "one run, one query": the reference's token at the query points INTO the run's interior for more than half of the
             streams, in every branch of the second pass (below cs, cs, above cs), with the candidate at window index 0, in
             the wrap zone, with the first candidate clipped to the oldest window byte and with the length clipped by W - index;
  family B   run fields with more than kRunCap long runs in every epoch: the listing hands its slots out by an LDS atomicAdd, so
             which runs are listed depends on timing; every stream stands four times in its batch and all four must be the
             reference's bytes;
  family C   the same shape with every run listed.
Every batch first asserts, through the two host queries, that the plan picks a run-aware build (the LDS layout with the run list)
and which of TAMP_AMD_BUILD_* it is.  What cannot be seen from here: which runs the device listed.
"""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

import run_list_input as rli  # noqa: E402
from test_compress_plan_golden import compress_lds_total  # noqa: E402

GENERIC, FIXED_EXT, FIXED_V1 = 0, 1, 2  # include/tamp_amd.h TAMP_AMD_BUILD_*
CALL_DICT_TABLE = 128                   # TAMP_AMD_CALL_DICT_TABLE
TUNING_ENV = ("TAMP_AMD_BLK", "TAMP_AMD_RUNS", "TAMP_AMD_FIXED_BUILD", "TAMP_AMD_BLOCK_LEAN", "TAMP_AMD_BLOCK_MIN", "TAMP_AMD_CUT_RUN",
              "TAMP_AMD_LPT", "TAMP_AMD_STATIC_GRID", "TAMP_AMD_GRID_PER_CU")
LAUNCH = 4096  # streams per launch of family A


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


def assert_run_aware(window, literal, extended, max_in_len, want_build, flags=0):
    """The plan of a call under the current environment: the LDS layout with the run list (the lean layout of the same block is
    another size), and the TAMP_AMD_BUILD_* the launcher derives from it."""
    from tamp_amd import _lib

    lib = _lib.load()
    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert lib.tamp_amd_compress_plan(window, max_in_len, 0, *[ctypes.byref(x) for x in v]) == 0
    blk, lds = v[0].value, v[1].value
    hb = 10 if window == 10 else 11
    assert lds == compress_lds_total(1 << window, blk, hb) != compress_lds_total(1 << window, blk, 0), (window, max_in_len, blk, lds)
    conf = _lib.TampAmdConf(window, literal, 0, int(extended), 0, 0, 0, 0)
    assert lib.tamp_amd_compress_build(ctypes.byref(conf), max_in_len, flags, 0) == want_build, (window, literal, extended, max_in_len)
    return blk


_expected = {}


def expected(checker, key, streams, **kw):
    from tamp_amd.batch import pack_streams

    if key not in _expected:
        flat, off, ln = pack_streams(streams)
        want = checker.compress_batch(flat, off, ln, threads=8, **kw)
        assert (np.asarray(want.status) == 0).all(), (key, "the checker refuses an input")
        _expected[key] = [want.stream(i) for i in range(len(streams))]
    return _expected[key]


def compress_and_compare(ta, streams, want, what, **kw):
    """Host-memory batches of at most LAUNCH streams; max_in_len >= 1,024 whatever the streams' lengths (the plan's input)."""
    max_in_len = max(1024, max(len(s) for s in streams))
    wrong = []
    for at in range(0, len(streams), LAUNCH):
        part = streams[at:at + LAUNCH]
        got = ta.compress_batch(list(part), max_in_len=max_in_len, **kw)
        status = np.asarray(got.status)
        for i in range(len(part)):
            if int(status[i]) != 0 or got.stream(i) != want[at + i]:
                wrong.append((at + i, int(status[i])))
    assert not wrong, (what, len(wrong), wrong[:8])


# ---------------------------------------------------------------------------------------------------------------------
# family A
# ---------------------------------------------------------------------------------------------------------------------
# (window, literal, extended, environment) -> TAMP_AMD_BUILD_*
FAMILY_A = {
    "w8_v1": ((8, 8, False, {}), GENERIC),
    "w8_ext": ((8, 8, True, {}), GENERIC),
    "w10_v1_fixed": ((10, 8, False, {}), FIXED_V1),
    "w10_v1_generic": ((10, 8, False, {"TAMP_AMD_FIXED_BUILD": "0"}), GENERIC),
    "w10_ext_fixed": ((10, 8, True, {}), FIXED_EXT),
    "w10_ext_generic": ((10, 8, True, {"TAMP_AMD_FIXED_BUILD": "0"}), GENERIC),
    "w10_v1_literal7": ((10, 7, False, {}), GENERIC),
}


@pytest.mark.parametrize("case", list(FAMILY_A))
def test_family_a_one_run_one_query(ta, checker, monkeypatch, case):
    (window, literal, extended, env), build = FAMILY_A[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    streams = [s.data for s in rli.family_a(window)]
    assert all(max(s) < 128 for s in streams[::101])  # (literal 7 takes them as they are)
    kw = dict(window=window, literal=literal, extended=extended)
    assert_run_aware(window, literal, extended, max(1024, max(len(s) for s in streams)), build)
    compress_and_compare(ta, streams, expected(checker, ("A", window, literal, extended), streams, **kw), case, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# families B and C
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = [(8, {}, None), (10, {}, "fixed"), (10, {"TAMP_AMD_FIXED_BUILD": "0"}, None), (12, {}, None), (14, {}, None)]


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("window,env,fixed", FIELDS, ids=["w8", "w10_fixed", "w10_generic", "w12", "w14"])
def test_run_fields_over_and_under_the_list_capacity(ta, checker, monkeypatch, window, env, fixed, extended):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    streams, names = rli.field_batch(window)
    W = 1 << window
    blk = assert_run_aware(window, 8, extended, max(len(s) for s in streams), (FIXED_EXT if extended else FIXED_V1) if fixed else GENERIC)
    for s, name in zip(streams, names):  # (the input-side predicates again, with the block of THIS plan)
        if name[0] == "B":
            rli.overflow_predicate_v1(s, W, blk, rli.K_RUN_CAP + 1 if window == 8 else rli.K_RUN_CAP * 5 // 4)
            if window >= 11:  # (the predicate that carries over to the extended format)
                rli.overflow_predicate_window(s, W)
        else:
            rli.all_listed_predicate(s, W)
    kw = dict(window=window, literal=8, extended=extended)
    want = expected(checker, ("BC", window, extended), streams, **kw)
    assert len({want[i] for i, nm in enumerate(names) if nm[0] == "B"}) == len(streams) // 5  # (the copies are copies)
    compress_and_compare(ta, list(streams), want, (window, extended, env), **kw)


@pytest.mark.parametrize("window", [10, 12])
def test_block_mode_run_field(ta, checker, window):
    """One v1 run field of 300,000 bytes: over the 256 KiB threshold, so the launcher spreads its blocks of 1,024 positions over
    all workgroups (kBlockRuns1024 at window 2^10, kBlockRuns at 2^12); every block's epoch holds more than 160 long runs."""
    import torch
    from tamp_amd.batch import compress_bound

    data = rli.block_mode_field()
    n = len(data)
    rli.overflow_predicate_v1(data, 1 << window, 1024)
    want = expected(checker, ("block", window), [data], window=window, literal=8, extended=False)[0]
    dev = torch.device("cuda:0")
    res = ta.compress_batch(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev), torch.zeros(1, dtype=torch.int64, device=dev),
                            torch.full((1,), n, dtype=torch.int32, device=dev), window=window, literal=8, extended=False, max_in_len=n,
                            out_cap=compress_bound(n, 8))
    torch.cuda.synchronize()
    assert int(res.status[0]) == 0 and int(res.out_len[0]) == len(want)
    assert res.out.cpu().numpy()[:len(want)].tobytes() == want


@pytest.mark.parametrize("extended", [False, True])
def test_run_fields_through_the_dictionary_table_twin(ta, checker, extended):
    """The DICTS twin of kRuns1024: the family B / C batch of window 2^10 with three custom dictionaries that are run fields
    themselves (the first epoch then holds more than kRunCap long runs as well), one selector per stream."""
    window = 10
    streams, names = rli.field_batch(window)
    dicts = [rli.family_b(1 << window, 10 + k, k != 1) for k in range(3)]
    assert all(rli.runs_in_span(d + s, 0, 1024 + 1024 + 16) > rli.K_RUN_CAP for d in dicts for s, nm in zip(streams, names) if nm[0] == "B")
    sel = [(2 * i + i // 5) % 3 for i in range(len(streams))]
    assert_run_aware(window, 8, extended, max(len(s) for s in streams), GENERIC, flags=CALL_DICT_TABLE)
    got = ta.compress_batch(list(streams), dictionaries=dicts, dictionary_index=sel, window=window, literal=8, extended=extended,
                            max_in_len=max(len(s) for s in streams))
    for i, s in enumerate(streams):
        st, want = checker.compress(s, window=window, literal=8, extended=extended, dictionary=dicts[sel[i]])
        assert st == 0 and int(got.status[i]) == 0 and got.stream(i) == want, (extended, i, names[i], sel[i])


@pytest.mark.parametrize("extended", [False, True])
def test_run_fields_in_pieces(ta, checker, monkeypatch, extended):
    """Two run fields through tamp_amd.Compressor with every write handed over as a piece (PIECE_MIN = 1), in writes of 1..300
    bytes: the second pass under `partial` (no parse step without a full ring, leftq counted to the piece's end).  A piece is a
    short message to the plan, so TAMP_AMD_RUNS=1 asks for the run-aware build; the dense field (runs of 8 or 9 bytes, one
    separator) overflows the list in pieces of about 200 bytes and more."""
    from tamp_amd import _lib

    monkeypatch.setenv("TAMP_AMD_RUNS", "1")
    window = 10
    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert _lib.load().tamp_amd_compress_plan(window, 300, 0, *[ctypes.byref(x) for x in v]) == 0
    assert v[1].value == compress_lds_total(1 << window, v[0].value, 10)  # (the layout with the run list)
    rng = np.random.default_rng(41)
    old_min = ta.Compressor.PIECE_MIN
    ta.Compressor.PIECE_MIN = 1
    try:
        for src in (rli.family_b(4096, 5, True, dense=True), rli.family_b(4096, 6, False)):
            ops, pos = [], 0
            while pos < len(src):
                k = int(rng.choice([1, 2, 15, 16, 17, 40, 100, 200, 250, 300]))
                ops.append(("write", src[pos:pos + k]))
                pos += k
            ops.append(("close",))
            rc, want = checker.stream_script(ops, window=window, literal=8, extended=extended)
            assert rc == 0
            f = io.BytesIO()
            c = ta.Compressor(f, window=window, literal=8, extended=extended)
            for op in ops:
                c.write(op[1]) if op[0] == "write" else c.close()
            assert f.getvalue() == want, (extended, len(src))
    finally:
        ta.Compressor.PIECE_MIN = old_min
