"""CPU tier: the decode plan against its characterisation fixture (tests/golden/decompress_plan.json).

The fixture holds what launch_decompress decided, over a grid of calls, pre-pass results, device facts and tuning variables, in
the last commit in which it wrote those decisions out inline (tests/golden/make_decompress_plan.py: recorded through a query
patched into that commit as a copy of the launcher's text).  The launcher and tamp_amd_decompress_plan now share plan_decompress
(tamp_amd/csrc/tamp_decompress_plan.hpp), which must reproduce every row; none was allowed to move.
"""
import base64
import ctypes
import itertools
import json
import os
import struct
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING_ENV = ("TAMP_AMD_DECODER", "TAMP_AMD_SPLIT_SLICE_LOG2", "TAMP_AMD_SPLIT_SCRATCH_MB", "TAMP_AMD_SPLIT_WAVE_MAX",
              "TAMP_AMD_SPLIT_SPW", "TAMP_AMD_SCRATCH_MB", "TAMP_AMD_LONGDEC", "TAMP_AMD_LONGDEC_MIN", "TAMP_AMD_LONGDEC_EXT",
              "TAMP_AMD_LONGDEC_CHAIN")
EXACT, GIB = 0x80, 1 << 30
SPLIT, WAVE, LANE_LDS, LANE_GLOBAL = 0, 1, 2, 3  # include/tamp_amd.h TAMP_AMD_DECODER_*
GROUPS = [
    ["long", ["long_attempt", "long_min_len", "long_extended", "long_chain"]],
    ["choice", ["scan", "decoder", "max_window_bits", "bulk"]],
    ["split", ["split_tokcap", "split_maxcap", "split_wave_resolve", "split_resolve_lds", "split_spw", "split_slice", "split_slab_bytes"]],
    ["wave", ["wave_waves", "wave_lds", "wave_groups"]],
    ["lane", ["lane_lds_row", "lane_lds", "lane_per_cu", "lane_grid"]],
    ["global", ["global_slot", "global_grid", "global_bulk", "global_lds", "global_lanes", "global_slab_bytes"]],
]

# ---- the grid, spelled out (the fixture's own `axes` must say the same) ----
FORCED = [{"TAMP_AMD_DECODER": d} for d in ("split", "lane", "global", "wave")]
LDS_EDGES = ["lds:%d:%d:%s" % (w, bulk, edge) for w in (8, 9, 10) for bulk in (0, 1) for edge in ("lo-1", "lo", "hi", "hi+1")]
N_ALL = [1, 16, 17, 255, 256, 257, 4096, 65536, 1 << 18, (1 << 18) + 1, 1 << 20, "slab-1", "slab"] + LDS_EDGES
LONGEST = [0, 1, 511, 512, 4096, 1 << 20]
OUT_CAP = [0, 1024, 2048, 2049, 4096, 16384, 16385]
SCANS = ([[l, c, "w", "uniform"] for l in LONGEST for c in OUT_CAP] +
         [[l, c, f, u] for l, c in ((511, 1024), (4096, 4096), (4096, 16385)) for f in (0, 8, "w-1", "w") for u in ("uniform", "mixed")
          if (f, u) != ("w", "uniform")])
AXES = {
    "calls": [["env", [{}] + FORCED + [{"TAMP_AMD_LONGDEC": "0"}, {"TAMP_AMD_LONGDEC_MIN": "65536"}]],
              ["cu_count", [256, 8]], ["dictionary", [0, 1]], ["exact", [0, 1]], ["max_wbits", list(range(7, 17))],
              ["free", [None]], ["held", [0]], ["exclude_split", [0]], ["scan", [[4096, 4096, "w", "uniform"]]], ["n_streams", N_ALL]],
    "scans": [["env", [{}] + FORCED], ["cu_count", [256, 8]], ["dictionary", [0, 1]], ["exact", [0]], ["max_wbits", [8, 9, 10, 11, 13, 15]],
              ["free", [None]], ["held", [0]], ["exclude_split", [0]], ["scan", SCANS],
              ["n_streams", [255, 256, 4096, "slab-1", "slab", "lds:10:1:lo-1", "lds:10:1:lo", "lds:10:1:hi", "lds:10:1:hi+1", 1 << 20]]],
    "budget": [["env", [{}, {"TAMP_AMD_DECODER": "split"}, {"TAMP_AMD_SPLIT_SCRATCH_MB": "64"}]], ["cu_count", [256, 8]], ["dictionary", [0]],
               ["exact", [0]], ["max_wbits", [8, 10, 12]], ["free", [None, GIB, 64 * GIB]], ["held", [0, 20 * GIB]], ["exclude_split", [0, 1]],
               ["scan", [[511, 1024, "w", "uniform"], [4096, 4096, "w", "uniform"], [1 << 20, 16384, "w", "uniform"]]],
               ["n_streams", [256, 4096, 65536, 1 << 18, (1 << 18) + 1, 1 << 20]]],
    "tuning": [["env", [{"TAMP_AMD_SPLIT_SLICE_LOG2": "12"}, {"TAMP_AMD_SPLIT_SCRATCH_MB": "64"}, {"TAMP_AMD_SPLIT_WAVE_MAX": "0"},
                        {"TAMP_AMD_SPLIT_WAVE_MAX": "4096"}, {"TAMP_AMD_SPLIT_SPW": "16"}, {"TAMP_AMD_SCRATCH_MB": "16"},
                        {"TAMP_AMD_LONGDEC": "0"}, {"TAMP_AMD_LONGDEC_MIN": "65536"}]],
               ["cu_count", [256, 8]], ["dictionary", [0]], ["exact", [0]], ["max_wbits", [8, 10, 12, 15]], ["free", [None, GIB]], ["held", [0]],
               ["exclude_split", [0]],
               ["scan", [[511, 1024, "w", "uniform"], [4096, 4096, "w", "uniform"], [1 << 20, 16384, "w", "mixed"], [4096, 16385, "w", "uniform"]]],
               ["n_streams", [16, 256, 4096, 65536, (1 << 18) + 1, 1 << 20]]],
}
ROWS = {"calls": 7 * 2 * 2 * 2 * 10 * 37, "scans": 5 * 2 * 2 * 6 * 63 * 10, "budget": 3 * 2 * 3 * 3 * 2 * 2 * 3 * 6, "tuning": 8 * 2 * 4 * 2 * 4 * 6}


def lds_capacity(cu_count, wbits, bulk):
    """Streams one round of the LDS lane decoder holds: 64 per workgroup, as many workgroups per CU as 160 KiB of LDS
    allow, sixteen at most.  A row is the window + 4 bytes; in the bulk build + 36 bytes, next to 128 + 64 x 148 bytes of staging."""
    lds = 128 + 64 * 148 + 64 * ((1 << wbits) + 36) if bulk else 64 * ((1 << wbits) + 4)
    return cu_count * min((160 << 10) // lds, 16) * 64


def n_streams(spec, cu_count):
    if isinstance(spec, int):
        return spec
    if spec.startswith("slab"):  # where the global lanes start: cu_count x 192 streams
        return cu_count * 192 - (spec == "slab-1")
    _, wbits, bulk, edge = spec.split(":")  # either side of 0.6 x and of 1.25 x the LDS lanes' capacity
    cap = lds_capacity(cu_count, int(wbits), int(bulk))
    lo, hi = -(-cap * 6 // 10), cap * 5 // 4
    return {"lo-1": lo - 1, "lo": lo, "hi": hi, "hi+1": hi + 1}[edge]


def scan_words(spec, wbits, n):
    """found, longest_in, window bytes in 256-byte units, max_out_cap.  uniform: every stream at window 2^found; mixed: half at 2^8."""
    longest, cap, found, units = spec
    w = wbits & 0x7F
    f = {"w": w, "w-1": w - 1}.get(found, found)
    per = 0 if f < 8 else ((1 << f) if units == "uniform" else ((1 << f) + 256) // 2)
    return f, longest, n * per // 256, cap


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "decompress_plan.json")) as f:
        doc = json.load(f)
    assert doc["groups"] == GROUPS
    for _, section in doc["sections"]:  # (rows: base64(zlib(little-endian uint16 table indices)), one array per group)
        for g, text in section["rows"].items():
            raw = zlib.decompress(base64.b64decode(text))
            section["rows"][g] = struct.unpack("<%dH" % (len(raw) // 2), raw)
    return doc


@pytest.fixture(autouse=True)
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in TUNING_ENV}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def walk(axes):
    """Every grid point of `axes` as (point, query), in the fixture's order (itertools.product); the environment is set on the way."""
    from tamp_amd import _lib

    env = None
    names = [name for name, _ in axes]
    for point in itertools.product(*[values for _, values in axes]):
        p = dict(zip(names, point))
        if p["env"] is not env:  # (the slowest axis)
            env = p["env"]
            for k in TUNING_ENV:
                os.environ.pop(k, None)
            os.environ.update(env)
        n = n_streams(p["n_streams"], p["cu_count"])
        bits = p["max_wbits"] | (EXACT if p["exact"] else 0)
        yield p, _lib.TampAmdDecodeQuery(n, bits, p["dictionary"], p["exclude_split"], p["free"] is not None, p["cu_count"],
                                         *scan_words(p["scan"], bits, n), p["free"] or 0, p["held"])


def recorded(golden):
    """(section, point, query, {group: recorded tuple}) for every row of the fixture."""
    for name, section in golden["sections"]:
        rows = section["rows"]
        for i, (p, q) in enumerate(walk(section["axes"])):
            yield name, p, q, {g: golden["tables"][g][rows[g][i]] for g, _ in GROUPS}


def test_the_grids_are_the_ones_recorded(golden):
    assert [name for name, _ in golden["sections"]] == list(AXES)
    for name, section in golden["sections"]:
        assert section["axes"] == AXES[name], name
        for g, _ in GROUPS:
            assert len(section["rows"][g]) == ROWS[name], (name, g)
    # the stream counts straddle the thresholds of DESIGN.md 4, at both device sizes
    for cu in (256, 8):
        ns = {n_streams(s, cu) for s in N_ALL}
        assert {cu * 192 - 1, cu * 192} <= ns
        for w in (8, 9, 10):
            for bulk in (0, 1):
                cap = lds_capacity(cu, w, bulk)
                lo, hi = min(n for n in ns if 10 * n >= 6 * cap), max(n for n in ns if 4 * n <= 5 * cap)
                assert {lo - 1, lo, hi, hi + 1} <= ns and 10 * (lo - 1) < 6 * cap and 4 * (hi + 1) > 5 * cap
    assert lds_capacity(256, 10, 1) == 256 * 2 * 64 and lds_capacity(256, 8, 0) == 256 * 9 * 64


def test_every_row(lib, golden):
    from tamp_amd import _lib

    wrong, rows = [], 0
    plan = _lib.TampAmdDecodePlan()
    for name, p, q, want in recorded(golden):
        assert lib.tamp_amd_decompress_plan(ctypes.byref(q), ctypes.byref(plan)) == 0
        got = {g: [getattr(plan, f) for f in fields] for g, fields in GROUPS}
        rows += 1
        if got != want:
            wrong.append((name, p, got, want))
    assert rows == sum(ROWS.values())
    assert not wrong, (len(wrong), wrong[:3])


def test_the_recording_reaches_every_path(golden):
    """A recording that never reaches a path pins nothing: every decoder is chosen UNFORCED somewhere, and the forced quirks are there."""
    unforced = set()
    forced_split_unfit = {}  # window bits -> decoders taken by TAMP_AMD_DECODER=split on a batch the split decoder cannot take
    odd_bits = {}            # window bits outside 8..15 -> (decoder, slot bytes, bulk build)
    no_scratch = set()
    for name, p, q, want in recorded(golden):
        scan, decoder, bits, bulk = want["choice"]
        if "TAMP_AMD_DECODER" not in p["env"] and not p["exclude_split"]:
            unforced.add(decoder)
        if p["env"].get("TAMP_AMD_DECODER") == "split" and decoder != SPLIT and scan and p["max_wbits"] in (10, 12) and bits == p["max_wbits"]:
            forced_split_unfit.setdefault(bits, set()).add(decoder)
        if p["max_wbits"] in (7, 16):
            odd_bits.setdefault(p["max_wbits"], set()).add((decoder, want["global"][0], want["global"][2]))
        if p["exclude_split"]:
            assert decoder != SPLIT
            no_scratch.add(decoder)
    assert unforced == {SPLIT, WAVE, LANE_LDS, LANE_GLOBAL}
    # forced "split" that does not fit never reaches the wave decoder: the LDS lanes up to 2^10 windows, the global slab above
    assert forced_split_unfit == {10: {LANE_LDS}, 12: {LANE_GLOBAL}}
    # window bits outside 8..15, whatever is forced: the global non-bulk lanes with 256-byte slots
    assert odd_bits == {7: {(LANE_GLOBAL, 256, 0)}, 16: {(LANE_GLOBAL, 256, 0)}}
    assert len(no_scratch) >= 2


def test_bad_arguments(lib):
    from tamp_amd import _lib

    q, plan = _lib.TampAmdDecodeQuery(0, 10, 0, 0, 0, 256), _lib.TampAmdDecodePlan()
    assert lib.tamp_amd_decompress_plan(ctypes.byref(q), ctypes.byref(plan)) == _lib.BAD_ARGUMENT
    assert lib.tamp_amd_decompress_plan(None, ctypes.byref(plan)) == _lib.BAD_ARGUMENT
    assert lib.tamp_amd_decompress_plan(ctypes.byref(q), None) == _lib.BAD_ARGUMENT
