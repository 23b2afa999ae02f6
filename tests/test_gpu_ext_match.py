"""GPU tier: the extended-match search decision by decision, on every path that restates it -- Walk::ext_search_rounds with one
wavefront and split over four (Walk::ext_search / Walk::serve), the settled extended matches of the run-aware builds' match
phase (sole_ext) with the walk's shortcut behind them, the fixed-geometry build and the generic ones, the dictionary-table twins,
the lazy builds (where the walk decides, not the match phase) and the carried extended match of the streaming Compressor.
All `-m gpu`, everything bit-exact.

The inputs are tests/ext_match_input.py's: one stream per decision (one candidate, rivals longer by one byte and equally long,
rivals at every lane, round and outer-loop boundary of the search, the cap and one short of it, candidates clipped by the
window's end, first matches that run through window_pos, the stream's last 13..19 bytes, a first match inside a run, runs on
either side, a match that the window's end clips when it is written, and the cap at every distance from an epoch's end);
tests/test_ext_match_input.py proves on the CPU that each takes its decision.  The expected bytes are the oracle's, and each is
first held against the reference's recorded result (status, length, SHA-256) in tests/golden/ext_cells.json, so what is compared
is the reference's own output.  Every batch goes once through decompress_batch.  A failing assertion names configuration, case,
cell and route.
"""
import ctypes
import hashlib
import io
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

import bucket_bits_input as bbi  # noqa: E402
import ext_match_input as emi  # noqa: E402

GENERIC, FIXED_EXT = 0, 1  # include/tamp_amd.h TAMP_AMD_BUILD_*
CALL_DICT_TABLE = 128      # TAMP_AMD_CALL_DICT_TABLE
HINT_AUTO, HINT_RUNS = 0, 2
TUNING_ENV = ("TAMP_AMD_BLK", "TAMP_AMD_RUNS", "TAMP_AMD_FIXED_BUILD", "TAMP_AMD_BLOCK_LEAN", "TAMP_AMD_BLOCK_MIN", "TAMP_AMD_CUT_RUN",
              "TAMP_AMD_LPT", "TAMP_AMD_STATIC_GRID", "TAMP_AMD_GRID_PER_CU")
CONFIG_IDS = [emi.config_id(*c) for c in emi.CONFIGS]
configs = pytest.mark.parametrize("window,literal", emi.CONFIGS, ids=CONFIG_IDS)
parses = pytest.mark.parametrize("lazy", [False, True], ids=["greedy", "lazy"])
CUTS = (1, 15, 16, 17, 19)


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@pytest.fixture(scope="module")
def golden():
    return load_golden("ext_cells.json")["cases"]


@pytest.fixture(autouse=True)
def no_tuning_env(monkeypatch):
    for k in TUNING_ENV:
        monkeypatch.delenv(k, raising=False)


_want = {}


def want(oracle, golden, case, lazy):
    """(status, bytes) of a case: the oracle's, held against the reference's recorded result.  Computed once, never modified."""
    key = (case.window, case.literal, case.name, lazy)
    if key not in _want:
        rc, blob = oracle.compress(case.data, window=case.window, literal=case.literal, extended=True, dictionary=case.dictionary,
                                   lazy_matching=lazy)
        rec = golden[emi.config_id(case.window, case.literal)][case.name][int(lazy)]
        assert [rc, len(blob), hashlib.sha256(blob).hexdigest()] == rec, (key, "the oracle is not the recorded reference")
        _want[key] = (rc, blob)
    return _want[key]


def planned(window, literal, lazy, max_in_len, flags=0, hint=HINT_AUTO, custom=False):
    """-> (TAMP_AMD_BUILD_*, block, threads per workgroup) of a batch call under the current environment."""
    from tamp_amd import _lib

    lib = _lib.load()
    conf = _lib.TampAmdConf(window, literal, int(custom), 1, 0, int(lazy), hint, 0)
    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert lib.tamp_amd_compress_plan(window, max_in_len, int(lazy), *[ctypes.byref(x) for x in v]) == 0
    return lib.tamp_amd_compress_build(ctypes.byref(conf), max_in_len, flags, 4096 if custom else 0), v[0].value, v[2].value


def run_batch(ta, oracle, golden, cases, lazy, route, max_in_len, layout=None, **kw):
    """One device-memory batch of ``cases`` (one configuration): status, length and bytes of every stream as the reference's, and
    the device decoder gives every stream its input back.  ``layout``: (flat, in_off, in_len, which) of bucket_bits_input.layout."""
    import torch
    from tamp_amd.batch import compress_bound, pack_streams

    c0 = cases[0]
    window, literal = c0.window, c0.literal
    if layout is None:
        flat, off, ln = pack_streams([c.data for c in cases])
        which = [(k, 0) for k in range(len(cases))]
    else:
        flat, off, ln, which = layout
    assert len(which) <= 256
    wants = [want(oracle, golden, cases[k], lazy) for k, _ in which]
    dev = torch.device("cuda:0")
    data = torch.from_numpy(np.array(flat, dtype=np.uint8)).to(dev)
    off_t, len_t = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev)
    longest = max(len(c.data) for c in cases)
    dict_kw = {k: v for k, v in kw.items() if k in ("dictionary", "dictionaries", "dictionary_index")}
    res = ta.compress_batch(data, off_t, len_t, window=window, literal=literal, extended=True, lazy_matching=lazy, max_in_len=max_in_len,
                            out_cap=compress_bound(longest, literal), **kw)
    torch.cuda.synchronize()
    status, out_len = res.status.cpu().numpy(), res.out_len.cpu().numpy()
    out, out_off = res.out.cpu().numpy(), res.out_off.cpu().numpy()

    def where(i):
        k, r = which[i]
        return (emi.config_id(window, literal), cases[k].name, cases[k].cell, route + (f", input offset {r} mod 4" if layout else ""))

    for i, (rc, blob) in enumerate(wants):
        assert int(status[i]) == rc, (*where(i), "status", int(status[i]), rc)
        assert int(out_len[i]) == len(blob), (*where(i), "length", int(out_len[i]), len(blob))
        assert out[int(out_off[i]):int(out_off[i]) + len(blob)].tobytes() == blob, (*where(i), "bytes")
    back = ta.decompress_batch(res.out, res.out_off, res.out_len, out_cap=longest + 8, **dict_kw)
    torch.cuda.synchronize()
    bstatus, blen = back.status.cpu().numpy(), back.out_len.cpu().numpy()
    bout, boff = back.out.cpu().numpy(), back.out_off.cpu().numpy()
    for i, (k, _) in enumerate(which):
        assert int(bstatus[i]) == 2, (*where(i), "round trip", int(bstatus[i]))
        assert bout[int(boff[i]):int(boff[i]) + int(blen[i])].tobytes() == cases[k].data, (*where(i), "round trip")


def sized(window, literal, size):
    cases = [c for c in emi.cases(window, literal) if c.size == size]
    assert len(cases) == emi.COUNTS[(window, literal)][size]
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# 1, 4: the led streams, four wavefronts
# ---------------------------------------------------------------------------------------------------------------------
@parses
@configs
def test_led_batch(ta, oracle, golden, monkeypatch, window, literal, lazy):
    """One batch per configuration on the 256-thread builds: window 2^10 with 8-bit literals takes the fixed-geometry build and
    then, under TAMP_AMD_FIXED_BUILD=0, the generic run-aware one; every other configuration, and lazy matching, is generic.
    Without lazy matching the epoch is the one the edge cells were placed against."""
    cases = sized(window, literal, emi.LED)
    max_in_len = max(len(c.data) for c in cases)
    build, blk, threads = planned(window, literal, lazy, max_in_len)
    fixed = (window, literal) == (10, 8) and not lazy
    assert (build, threads) == (FIXED_EXT if fixed else GENERIC, 256), (window, literal, lazy)
    if not lazy:
        assert blk == emi.EDGE_BLOCK[(window, literal)], "the epoch the edge cells were placed against"
        assert {(c.at + int(c.cell[6:])) % blk for c in cases if c.cell.startswith("edge.")} == {0}
    run_batch(ta, oracle, golden, cases, lazy, "led batch" + (", fixed build" if fixed else ""), max_in_len)
    if fixed:
        monkeypatch.setenv("TAMP_AMD_FIXED_BUILD", "0")
        assert planned(window, literal, lazy, max_in_len)[::2] == (GENERIC, 256)
        run_batch(ta, oracle, golden, cases, lazy, "led batch, TAMP_AMD_FIXED_BUILD=0", max_in_len)


# ---------------------------------------------------------------------------------------------------------------------
# 2, 4: the bare streams with their dictionaries, one wavefront
# ---------------------------------------------------------------------------------------------------------------------
@parses
@configs
def test_bare_batch(ta, oracle, golden, window, literal, lazy):
    """The streams under 1 KiB, one call per distinct dictionary, on the one-wavefront build (which runs all four quarters of a
    search by itself); then with run_aware=True, the run-aware build of short messages with its settled extended matches."""
    cases = sized(window, literal, emi.BARE)
    max_in_len = max(len(c.data) for c in cases)
    assert max_in_len < 1024
    dicts = sorted({c.dictionary for c in cases})
    assert len(dicts) >= 20
    for run_aware in (None, True):
        hint = HINT_RUNS if run_aware else HINT_AUTO
        assert planned(window, literal, lazy, max_in_len, hint=hint, custom=True)[::2] == (GENERIC, 64), (window, literal, lazy, run_aware)
        for d in dicts:
            run_batch(ta, oracle, golden, [c for c in cases if c.dictionary == d], lazy, f"bare batch, run_aware={run_aware}", max_in_len,
                      dictionary=d, run_aware=run_aware)


# ---------------------------------------------------------------------------------------------------------------------
# 3: the dictionary table
# ---------------------------------------------------------------------------------------------------------------------
@parses
@pytest.mark.parametrize("window,literal", [(10, 8), (8, 8)], ids=["w10-l8", "w8-l8"])
def test_dictionary_table(ta, oracle, golden, window, literal, lazy):
    """Every bare case with its own dictionary in ONE launch of the table twins (dictionaries=[...], dictionary_index=)."""
    cases = sized(window, literal, emi.BARE)
    max_in_len = max(len(c.data) for c in cases)
    dicts = sorted({c.dictionary for c in cases})
    assert planned(window, literal, lazy, max_in_len, CALL_DICT_TABLE, custom=True)[::2] == (GENERIC, 64)
    run_batch(ta, oracle, golden, cases, lazy, "dictionary table", max_in_len, dictionaries=dicts,
              dictionary_index=[dicts.index(c.dictionary) for c in cases])


# ---------------------------------------------------------------------------------------------------------------------
# 5: input alignment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [True, False], ids=["fixed", "generic"])
def test_input_alignment(ta, oracle, golden, monkeypatch, fixed):
    """Window 2^10: every led stream four times in its batch, at input offsets 0, 1, 2 and 3 mod 4."""
    cases = sized(10, 8, emi.LED)
    max_in_len = max(len(c.data) for c in cases)
    if not fixed:
        monkeypatch.setenv("TAMP_AMD_FIXED_BUILD", "0")
    assert planned(10, 8, False, max_in_len)[::2] == (FIXED_EXT if fixed else GENERIC, 256)
    layout = bbi.layout([c.data for c in cases])
    assert sorted({int(o) % 4 for o in layout[1]}) == [0, 1, 2, 3]
    run_batch(ta, oracle, golden, cases, False, "aligned batch, " + ("fixed build" if fixed else "TAMP_AMD_FIXED_BUILD=0"), max_in_len, layout=layout)


# ---------------------------------------------------------------------------------------------------------------------
# 6: the streaming Compressor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [emi.LED, emi.BARE])
def test_compressor_pieces_carry_the_extended_match(ta, oracle, golden, size):
    """Window 2^10, Compressor with every write handed over as a piece: each rival, cap and clip case in two writes cut 1, 15, 16,
    17 and 19 bytes behind the query -- inside the first match, at its end and inside the bytes the search adds.  The second piece
    starts from the carried position and count and may only move to candidates at or above it: the bytes of the one-shot stream."""
    cases = [c for c in sized(10, 8, size) if c.group in ("rival", "cap", "clip")]
    assert len(cases) == 11
    for c in cases:
        rc, blob = want(oracle, golden, c, False)
        assert rc == 0
        for cut in CUTS:
            f = io.BytesIO()
            comp = ta.Compressor(f, window=10, literal=8, extended=True, dictionary=c.dictionary)
            comp.PIECE_MIN = 1
            comp.write(c.data[:c.at + cut])
            comp.write(c.data[c.at + cut:])
            comp.close()
            assert f.getvalue() == blob, (emi.config_id(10, 8), c.name, c.cell, f"Compressor, pieces cut {cut} behind the query")
