"""CPU tier of the lazy-matching cells (tests/lazy_input.py): every designed input takes the decision it is named for, at the
position it names, as the oracle's decision events (oracle_set_lazy_cb) report it; neighbours of a tuple decide differently and
compress to different bytes; the oracle's bytes are the reference's (live where oracle/_ref is built, and through the recorded
results of tests/golden/lazy_cells.json everywhere).  `pytest -s` prints the census of cells over all configurations.

Nothing here reads the code under test: the conditions are properties of the inputs under the reference's rules, so an input that
misses its cell is a mistake in the design, never a reason to change what is asked of it.
"""
import collections
import ctypes as C
import hashlib
import importlib.util
import os
import sys

import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lazy_input as li  # noqa: E402


def _generator():
    spec = importlib.util.spec_from_file_location("make_lazy_cells", os.path.join(ROOT, "tests", "golden", "make_lazy_cells.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _generator()
CONFIG_IDS = [gen.config_id(*c) for c in gen.CONFIGS]
configs = pytest.mark.parametrize("window,literal,extended", gen.CONFIGS, ids=CONFIG_IDS)
_TOKEN_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_size_t, C.c_uint, C.c_uint)


@pytest.fixture(scope="module")
def golden():
    return load_golden("lazy_cells.json")


_runs = {}


def run(oracle, case):
    """-> (status, bytes, events by position, input position of the first token that is no literal) of one case, computed once."""
    key = (case.window, case.literal, case.extended, case.name)
    if key not in _runs:
        first = []
        cb = _TOKEN_CB(lambda user, kind, pos, length, index: first.append(int(pos)) if kind else None)
        oracle.lib.oracle_set_token_cb.argtypes = [_TOKEN_CB, C.c_void_p]
        oracle.lib.oracle_set_token_cb.restype = None
        oracle.lib.oracle_set_token_cb(cb, None)
        try:
            rc, blob, events = oracle.lazy_events(case.data, window=case.window, literal=case.literal, extended=case.extended,
                                                  dictionary=case.dictionary)
        finally:
            oracle.lib.oracle_set_token_cb(C.cast(None, _TOKEN_CB), None)
        by = collections.defaultdict(list)
        for e in events:
            by[e.pos].append(e)
        _runs[key] = (rc, blob, by, min(first) if first else len(case.data))
    return _runs[key]


def outcome(oracle, case):
    """What was decided at every position the case names: ((event, len, nlen, nidx - wp), ...), or None where it misses."""
    _, _, by, _ = run(oracle, case)
    out = []
    for pos, expect in ((case.at, case.expect), *case.also):
        hit = [e for e in by[pos] if li.matches(e, expect)]
        if not hit:
            return None
        out.append((hit[0].event, hit[0].len, hit[0].nlen, hit[0].nidx - hit[0].wp))
    return tuple(out)


@configs
def test_every_case_reaches_its_cell(oracle, window, literal, extended):
    cases = li.cases(window, literal, extended)
    assert cases
    for c in cases:
        rc, blob, by, first = run(oracle, c)
        what = (gen.config_id(window, literal, extended), c.name)
        assert rc == c.status, (what, rc)
        assert len(c.data) <= 4096, what
        assert len(c.data) < 1024 if c.size == li.BARE else len(c.data) >= 1088, (what, len(c.data))
        for pos, expect in ((c.at, c.expect), *c.also):
            assert any(li.matches(e, expect) for e in by[pos]), (what, c.cell, pos, expect, by[pos])
        if c.size == li.LED and c.at >= 1088:  # window_pos at the cell is the lead's length; the lead is literals only, unless
            # the design has planted the cell's own bytes in it (two copies of the probe's source match each other)
            assert by[c.at][0].wp == c.at % (1 << window), (what, by[c.at][0])
            if not c.cell.startswith(("d.", "g.pattern", "i.")):
                assert first >= c.at - 40, (what, "a match in the lead", first)
        if c.dictionary is not None:
            assert len(c.dictionary) == 1 << window


@configs
def test_neighbours_decide_differently_and_give_different_bytes(oracle, window, literal, extended):
    groups = collections.defaultdict(list)
    for c in li.cases(window, literal, extended):
        groups[(c.group, c.size)].append(c)
    for (group, size), members in groups.items():
        outcomes = [outcome(oracle, c) for c in members]
        blobs = [run(oracle, c)[1] for c in members]
        assert None not in outcomes
        assert len(set(outcomes)) == len(members), (group, size, outcomes)
        assert len(set(blobs)) == len(members), (group, size)


@configs
def test_oracle_bytes_are_the_recorded_reference_bytes(oracle, golden, window, literal, extended):
    rec = golden["cases"][gen.config_id(window, literal, extended)]
    cases = li.cases(window, literal, extended)
    assert sorted(rec) == sorted(c.name for c in cases)
    for c in cases:
        rc, blob, _, _ = run(oracle, c)
        assert [rc, len(blob), hashlib.sha256(blob).hexdigest()] == rec[c.name], (window, literal, extended, c.name)
        # the decision hook changes nothing: the same call without it
        assert oracle.compress(c.data, window=window, literal=literal, extended=extended, dictionary=c.dictionary, lazy_matching=True) == (rc, blob)


@configs
def test_fixture_reproduces_from_the_reference(golden, ref, window, literal, extended):
    """tests/golden/make_lazy_cells.py on the live reference gives the committed results (skipped where oracle/_ref is not built)."""
    cid = gen.config_id(window, literal, extended)
    assert gen.generate_cases(ref, [(window, literal, extended)]) == {cid: golden["cases"][cid]}


def test_census_every_cell_is_reached(oracle):
    census = collections.Counter()
    dropped = 0
    for window, literal, extended in gen.CONFIGS:
        for c in li.cases(window, literal, extended):
            if outcome(oracle, c) is not None:
                census[c.cell] += 1
            dropped += sum(e.event == "dropped_by_rle" for es in run(oracle, c)[2].values() for e in es)
    for cell in li.CELLS:
        print(f"lazy cell {cell:22s} {census[cell]:4d} cases")
    print(f"cached matches dropped by the RLE handler: {dropped}")
    assert sorted(census) == sorted(li.CELLS)
    assert all(census[cell] >= 2 for cell in li.CELLS), census  # (each in more than one size or configuration)
    assert dropped >= 8  # g.run, extended format, every window, both sizes


@pytest.mark.parametrize("extended", [True, False], ids=["ext", "v1"])
@pytest.mark.parametrize("window", [10, 15])
def test_epoch_stream_defers_at_every_lane(oracle, window, extended):
    """j: the defers stand 37 positions apart, so their positions take every residue modulo 64 (the walk's blocks)."""
    for c in li.cases(window, 8, extended):
        if not c.cell.startswith("j."):
            continue
        assert 2300 <= len(c.data) <= 2500
        _, _, by, _ = run(oracle, c)
        named = sorted(pos for pos, ex in ((c.at, c.expect), *c.also) if ex["event"] == "defer" and ex["origin"] == "fresh")
        defers = [pos for pos in named if any(e.event == "defer" and e.origin == "fresh" for e in by[pos])]  # (plants may defer too)
        assert len(defers) == li.J_UNITS and {b - a for a, b in zip(defers, defers[1:])} == {li.J_PERIOD}, c.name
        assert {p % 64 for p in defers} == set(range(64)), c.name
        if c.cell == "j.chain":
            assert all(any(e.event == "defer" and e.origin == "cached" for e in by[p + 1]) for p in defers)


SWEEP_IDS = [f"w{w}-{'ext' if e else 'v1'}" for w, e in gen.SWEEPS]


@pytest.mark.parametrize("window,extended", gen.SWEEPS, ids=SWEEP_IDS)
def test_sweep_stream_keeps_every_cell_and_its_fixture_is_consistent(oracle, golden, window, extended):
    src, marks = li.sweep_source(window, extended)
    rc, whole, events = oracle.lazy_events(src, window=window, literal=8, extended=extended)
    assert rc == 0 and 500 <= len(src) <= 4096
    by = collections.defaultdict(list)
    for e in events:
        by[e.pos].append(e)
    for pos, expect, cell in marks:
        assert any(li.matches(e, expect) for e in by[pos]), (cell, pos, expect, by[pos])
    rec = next(r for r in golden["sweep"] if (r["window"], r["extended"]) == (window, extended))
    assert rec["input_len"] == len(src) and rec["input_sha256"] == hashlib.sha256(src).hexdigest()
    assert rec["whole_len"] == len(whole) and rec["whole_sha256"] == hashlib.sha256(whole).hexdigest()
    assert len(rec["cuts"]) == len(src) + 1
    prev = 0
    for c, (s1, len1, k1, s2, len2, k2) in enumerate(rec["cuts"]):
        assert (s1, s2) == (0, 0) and (k1, k2) == (c, len(src) - c), c
        assert len1 + len2 == len(whole) and prev <= len1, c
        prev = len1


@pytest.mark.parametrize("window,extended", gen.SWEEPS, ids=SWEEP_IDS)
def test_sweep_fixture_reproduces_from_the_reference(golden, ref, window, extended):
    (rec,) = gen.generate_sweeps(ref, [(window, extended)])
    assert rec == next(r for r in golden["sweep"] if (r["window"], r["extended"]) == (window, extended))
