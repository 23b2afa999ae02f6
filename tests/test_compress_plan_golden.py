"""CPU tier: the launch plan of the compress kernel against its characterisation fixture (tests/golden/compress_plan.json).

The fixture holds what tamp_amd_compress_plan and tamp_amd_compress_build answered, over a grid of calls and tuning variables, in
the last commit in which the two queries and the two launchers each wrote the decisions out for themselves (tests/golden/
make_compress_plan.py).  All four now share plan_compress (tamp_amd/csrc/tamp_compress_plan.hpp), which must reproduce every
row.  One answer was allowed to move and has its own test: the plan query honours TAMP_AMD_RUNS as the launcher always did
(plan rows are recorded with the variable unset).
"""
import ctypes
import itertools
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING_ENV = ("TAMP_AMD_BLK", "TAMP_AMD_RUNS", "TAMP_AMD_FIXED_BUILD", "TAMP_AMD_BLOCK_LEAN")


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "compress_plan.json")) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in TUNING_ENV}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def walk(axes):
    """Every grid point of `axes` as a dict, in the fixture's order (itertools.product); the environment is set on the way."""
    env = None
    for point in itertools.product(*[values for _, values in axes]):
        p = dict(zip([name for name, _ in axes], point))
        if p["env"] is not env:  # (the slowest axis)
            env = p["env"]
            for k in TUNING_ENV:
                os.environ.pop(k, None)
            os.environ.update(env)
        yield p


def plan(lib, window, max_in_len, lazy):
    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert lib.tamp_amd_compress_plan(window, max_in_len, lazy, *[ctypes.byref(x) for x in v]) == 0
    return [x.value for x in v]  # block, LDS bytes, threads, workgroups per CU


def test_the_grids_are_the_ones_recorded(golden):
    def axis(section, name):
        return dict(golden[section]["axes"])[name]

    assert axis("plan", "window") == axis("build", "window") == list(range(8, 16))
    assert axis("plan", "max_in_len") == [0, 1, 63, 64, 65, 256, 512, 960, 1023, 1024, 1025, 1088, 1280, 1536, 2047, 2048, 2049, 4096, 65536, 1 << 20]
    assert axis("plan", "lazy") == [0, 1]
    assert axis("plan", "env") == [{}] + [{"TAMP_AMD_BLK": str(b)} for b in (64, 512, 960, 1024, 2048)]
    assert len(golden["plan"]["rows"]) == 6 * 8 * 20 * 2
    assert axis("build", "env") == [{}, {"TAMP_AMD_FIXED_BUILD": "0"}, {"TAMP_AMD_RUNS": "0"}, {"TAMP_AMD_RUNS": "1"}, {"TAMP_AMD_BLK": "512"}]
    assert (axis("build", "literal"), axis("build", "hint"), axis("build", "max_in_len")) == ([5, 8], [0, 1, 2], [0, 256, 960, 1024, 4096, 1 << 20])
    assert axis("build", "flags") == [0, 1, 2, 4, 8, 16, 32, 64, 1 | 2 | 4]  # plain, each TAMP_AMD_CALL_* singly, STATE | RESUME | SAVE
    assert sorted(axis("build", "dictionary")) == [[0, 0x7F0000001000], [0, 0x7F0000001002], [1, 0x7F0000001000], [1, 0x7F0000001002]]
    assert sum(n for _, n in golden["build"]["runs"]) == 5 * 8 * 2 * 2 * 2 * 3 * 2 * 6 * 9 * 4


def test_every_plan_row(lib, golden):
    g = golden["plan"]
    wrong = []
    for p, want in zip(walk(g["axes"]), g["rows"]):
        got = plan(lib, p["window"], p["max_in_len"], p["lazy"])
        if got != g["tuples"][want]:
            wrong.append((p, got, g["tuples"][want]))
    assert not wrong, (len(wrong), wrong[:5])


def test_every_build_row(lib, golden):
    from tamp_amd import _lib

    g = golden["build"]
    want = itertools.chain.from_iterable(itertools.repeat(b, n) for b, n in g["runs"])
    wrong, rows = [], 0
    for p, w in zip(walk(g["axes"]), want):
        custom, address = p["dictionary"]
        conf = _lib.TampAmdConf(p["window"], p["literal"], custom, p["extended"], p["reset"], p["lazy"], p["hint"], 0)
        got = lib.tamp_amd_compress_build(ctypes.byref(conf), p["max_in_len"], p["flags"], address)
        rows += 1
        if got != w:
            wrong.append((p, got, w))
    assert rows == sum(n for _, n in g["runs"])
    assert not wrong, (len(wrong), wrong[:5])


def compress_lds_total(W, blk, hb):
    """CompressLds(W, blk, packed, lazy = false, runlist, hb).total of tamp_compress_kernel.hpp for packed entries: hb = 0 is the lean
    layout (2,048 bucket cursors, no run list), hb = 10 / 11 the run-aware one with that many bucket bits.  A hand copy of the header's
    arithmetic, so it changes with the layout; the test below pins it to three recorded values before relying on it, and its last
    check (the rows recorded under TAMP_AMD_BLK=512) proves the correction without it."""
    def up(x, a):
        return (x + a - 1) // a * a

    ring, pend_max, slow_cap, run_cap = 16, 256, 128, 128  # kRing, kPendMax, kSlowCap, kRunCap
    o = 16 + up(W + blk + ring + pend_max + 32, 16)               # slack, ebuf
    o += (1 << hb if 0 < hb < 11 else 2048) * 2                   # bucket cursors
    tokcap = blk + pend_max + ring + 80
    o += up(max((W + blk + 16) * 4, up(tokcap * 2, 16) + blk * 4 + 16), 16)  # index entries / token list + jump tables
    o += up(blk + 128, 16) + up(blk * 2, 16)                      # blen, bidx
    o += up(max(((blk + pend_max + ring + 64) * 9 + slow_cap * 25) // 32 + 8, 4 + blk // 2) * 4, 16)  # bit buffer
    o += 80 + 64 * 4 + 16                                         # control words, sort bins, prefix codes
    if hb:
        o += run_cap * 4 + run_cap * 4 + 32 + up((W + blk + 96) // 8, 16)  # run list, run bytes, byte set, bitmap
    return o


def test_the_plan_query_honours_the_run_aware_override(lib, golden):
    """TAMP_AMD_RUNS=1 launches short messages with the run-aware build -- at window 2^10 the layout with 1,024 buckets, kHb1024 -- and the
    query now says so: it used to report the lean layout whatever the variable."""
    g = golden["plan"]
    recorded, recorded_blk512 = {}, {}
    for p, row in zip(walk(g["axes"]), g["rows"]):
        if not p["env"] or p["env"] == {"TAMP_AMD_BLK": "512"}:
            (recorded if not p["env"] else recorded_blk512)[(p["window"], p["max_in_len"], p["lazy"])] = g["tuples"][row]
    for k in TUNING_ENV:
        os.environ.pop(k, None)
    blk, lean_lds, threads, _ = recorded[(10, 256, 0)]  # the block comes from the fixture, the layouts from the formula
    assert (blk, threads) == (256, 64)
    assert lean_lds == compress_lds_total(1024, blk, 0)
    assert recorded[(10, 1024, 0)][:2] == [1024, compress_lds_total(1024, 1024, 10)] == [1024, 19616]  # (the formula above is the header's)
    run_aware_lds = compress_lds_total(1024, blk, 10)
    assert run_aware_lds != lean_lds
    assert plan(lib, 10, 256, 0) == recorded[(10, 256, 0)]
    os.environ["TAMP_AMD_RUNS"] = "1"
    got = plan(lib, 10, 256, 0)
    assert got[0] == blk and got[2] == threads
    assert got[1] == run_aware_lds and got[1] != lean_lds
    assert got[3] == min(8, 160 * 1024 // ((run_aware_lds + 2047) // 2048 * 2048))  # eight per CU: the run-aware builds' register budget
    # (and without the formula: 512-byte messages get the layout recorded for long streams under a block override of 512)
    long512 = recorded_blk512[(10, 1024, 0)]
    assert long512[0] == 512 and plan(lib, 10, 512, 0)[:2] == long512[:2] != recorded[(10, 512, 0)][:2]
    os.environ["TAMP_AMD_RUNS"] = "0"
    assert plan(lib, 10, 256, 0) == recorded[(10, 256, 0)]
    assert plan(lib, 10, 1024, 0) == recorded[(10, 1024, 0)]  # (long streams: the variable does not apply)
