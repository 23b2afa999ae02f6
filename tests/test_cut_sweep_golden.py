"""CPU tier of the cut sweep (tests/cut_sweep_input.py): the input covers what it claims to cover, and the fixture
tests/golden/cut_sweep.json -- the reference object's per-call results for every two-call cut -- is consistent with the
one-shot stream and reproduces from tests/golden/make_cut_sweep.py wherever the reference C is built.

The coverage conditions are NECESSARY conditions read from the oracle's token trace, not from the code under test: if a
change of the recipe misses one, the recipe changes, not the bound.  Measured on the recipe as committed
(cuts inside RLE tokens (< 16 bytes past the start) / inside extended matches (< 16) / tokens ending at the window's end):
w10-ext 308 (68) / 369 (164) / 1, w8-ext 308 (68) / 208 (119) / 3, w15-ext 305 (68) / 325 (134) / none possible,
w10-v1 1, w8-v1 2.
"""
import hashlib
import importlib.util
import os
import sys

import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cut_sweep_input as cs  # noqa: E402

IDS = [cs.case_id(w, e) for w, e in cs.CONFIGS]


@pytest.fixture(scope="module")
def golden():
    return {(r["window"], r["extended"]): r for r in load_golden("cut_sweep.json")}


@pytest.fixture(scope="module")
def traces(oracle):
    return {(w, e): cs.token_trace(oracle, cs.source(w), w, e) for w, e in cs.CONFIGS}


def test_one_input_per_window_of_the_documented_size():
    for w, _ in cs.CONFIGS:
        src = cs.source(w)
        assert 1300 <= len(src) <= 1450, (w, len(src))
        assert len(src) > (1 << w) or w == 15  # passes the end of the window buffer (2^15: the unpacked-index build)
    assert len(cs.source(8)) >= 5 * 256


@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=IDS)
def test_one_shot_stream_is_a_write_and_a_flush(oracle, window, extended):
    """oracle.compress(src) -- the `whole` of every sweep -- is the stream of one write and one flush without a token."""
    src = cs.source(window)
    rc, whole = oracle.compress(src, window=window, literal=cs.LITERAL, extended=extended)
    assert rc == 0
    rc, segs = oracle.stream_script([("write", src), ("flush", False)], window=window, literal=cs.LITERAL, extended=extended)
    assert rc == 0 and segs == whole


@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=IDS)
def test_one_shot_stream_is_the_reference_objects(oracle, ref, window, extended):
    """... and what one reference object emits for them (skipped where oracle/_ref is not built)."""
    src = cs.source(window)
    rc, whole = oracle.compress(src, window=window, literal=cs.LITERAL, extended=extended)
    rc2, want = ref.stream_script([("write", src), ("flush", False)], window=window, literal=cs.LITERAL, extended=extended)
    assert (rc, rc2) == (0, 0) and want == whole


@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=IDS)
def test_cuts_cover_runs_extended_matches_and_the_window_end(traces, window, extended):
    tokens, _ = traces[(window, extended)]
    cov = cs.coverage(tokens, len(cs.source(window)), window)
    print(cs.case_id(window, extended), {k: (len(v) if k == "window_end" else v) for k, v in cov.items()})
    if extended:
        assert cov["rle"] >= 200, cov
        assert cov["rle_near"] >= 50, cov
        assert cov["ext"] >= 100, cov
        assert 241 in cov["rle_lengths"], cov  # the longest RLE token: the 260-byte run is cut in two
        # one extended match that barely is one (16 bytes or fewer) and one that grows over several fills of the ring
        assert min(cov["ext_lengths"]) <= 16 and max(cov["ext_lengths"]) >= 40, cov
        assert cov["ext_near"] >= 50, cov
    else:
        assert cov["rle"] == 0 and cov["ext"] == 0
        assert cov["match"] >= 500, cov
    if window < 15:  # (nothing reaches the end of a 32 KiB window buffer)
        assert len(cov["window_end"]) >= 1, "no match or extended match ends at the end of the window buffer"
        assert any(t[2] >= 3 for t in cov["window_end"])
    # cuts inside a window-end token exist (a token of 2+ bytes has a byte boundary strictly inside)
    for t in cov["window_end"]:
        assert t[3] + t[2] == 1 << window and t[2] >= 2


def test_describe_cut_names_the_token(traces):
    tokens, _ = traces[(10, True)]
    run = next(t for t in tokens if t[0] == 2 and t[2] == 241)
    assert cs.describe_cut(tokens, run[1] + 7) == \
        f"cut {run[1] + 7}: 7 bytes into the rle token of 241 (input {run[1]}, window index 0)"
    assert cs.describe_cut(tokens, run[1]).startswith(f"cut {run[1]}: in front of the rle token of 241")
    assert cs.describe_cut(tokens, len(cs.source(10))).endswith("behind the last token")
    assert cs.inside(run, run[1] + 1) and cs.inside(run, run[1] + 240)
    assert not cs.inside(run, run[1]) and not cs.inside(run, run[1] + 241)


@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=IDS)
def test_fixture_is_consistent_with_the_one_shot_stream(golden, traces, window, extended):
    rec = golden[(window, extended)]
    src = cs.source(window)
    tokens, whole = traces[(window, extended)]
    assert rec["literal"] == cs.LITERAL and rec["cap"] == cs.CAP
    assert rec["input_len"] == len(src) and rec["input_sha256"] == hashlib.sha256(src).hexdigest()
    assert rec["whole_len"] == len(whole) and rec["whole_sha256"] == hashlib.sha256(whole).hexdigest()
    assert len(rec["cuts"]) == len(src) + 1  # every cut 0..len(src)
    prev = 0
    for c, (s1, len1, k1, s2, len2, k2) in enumerate(rec["cuts"]):
        where = cs.describe_cut(tokens, c)
        assert (s1, s2) == (0, 0), where
        assert (k1, k2) == (c, len(src) - c), where        # every byte offered is taken
        assert len1 + len2 == len(whole), where             # the written bytes are the next bytes of the whole stream
        assert prev <= len1 <= len(whole), where            # more input never un-writes a byte
        # the first call holds back at most the 16-byte ring, one growing token and 31 pending bits: what it wrote covers
        # no more than the tokens that end at or before the cut
        assert len1 <= 1 + (9 * c + 7) // 8, where
        prev = len1
    assert rec["cuts"][0][1] == 0  # nothing offered: even the header waits in the bit buffer


def _generator():
    spec = importlib.util.spec_from_file_location("make_cut_sweep", os.path.join(ROOT, "tests", "golden", "make_cut_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=IDS)
def test_fixture_reproduces_from_the_reference(golden, ref, window, extended):
    """tests/golden/make_cut_sweep.py on the live reference object gives the committed fixture (skipped where oracle/_ref
    is not built)."""
    (rec,) = _generator().generate(ref, [(window, extended)])
    assert rec == golden[(window, extended)]
