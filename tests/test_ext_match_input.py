"""CPU tier of the extended-match cells (tests/ext_match_input.py): every designed input takes the decision it is named for.  Per
case and configuration, without and with lazy matching: the oracle's token at the query position (tests/long_stream_writer.py's
reader) is the case's expectation and no token straddles the query; nothing in front of it is an RLE of more than 8 bytes or a
clipped extended match; status, length and SHA-256 are the reference's recorded ones (tests/golden/ext_cells.json), and the
reference's own bytes where oracle/_ref is built.

``rule`` restates the search in plain Python over a window that this file reconstructs itself -- the first match as
find_best_match finds it, then the longest common prefix among the candidates at or above it, capped, ties to the lowest -- and
must agree with every expectation; it also supplies the structural facts the cells claim (16-byte hits, hits that run past the
newest byte, the distance d, the offsets of the kernel's 4-byte filters).  `pytest -s` prints the census.

Nothing here reads the code under test: an input that misses its cell is a mistake in the design.
"""
import collections
import hashlib
import importlib.util
import os
import sys

import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ext_match_input as emi  # noqa: E402
import long_stream_writer as lsw  # noqa: E402


def _generator():
    spec = importlib.util.spec_from_file_location("make_ext_cells", os.path.join(ROOT, "tests", "golden", "make_ext_cells.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _generator()
configs = pytest.mark.parametrize("window,literal", emi.CONFIGS, ids=[emi.config_id(*c) for c in emi.CONFIGS])


@pytest.fixture(scope="module")
def golden():
    return load_golden("ext_cells.json")["cases"]


def said(tk):
    return (tk.kind, tk.produced, tk.off)


def trace(oracle, case, lazy):
    """-> (status, bytes, {input position: token})"""
    rc, blob = oracle.compress(case.data, window=case.window, literal=case.literal, extended=True, dictionary=case.dictionary, lazy_matching=lazy)
    at, pos = {}, 0
    for tk in lsw.read_tokens(blob)[0]:
        if tk.kind != "F":
            at[pos] = tk
            pos += tk.produced
    assert pos == len(case.data), (case.name, "the tokens do not produce the input", pos, len(case.data))
    return rc, blob, at


def window_at(oracle, case):
    """The window at the query, by this file's own account: the dictionary, then the input byte by byte (which holds as long as
    nothing in front of the query is a long RLE or a clipped extended match: ``verify``).  -> (window, window_pos)"""
    W = 1 << case.window
    win = bytearray(case.dictionary if case.dictionary is not None else oracle.initialize_dictionary(W, case.literal))
    for s in range(case.at):
        win[s % W] = case.data[s]
    return win, case.at % W


def lcp(win, c, pat, limit):
    """Common prefix of the window from index c (it ends with the window, it does not wrap) and ``pat``, ``limit`` at most."""
    n, limit = 0, min(limit, len(win) - c, len(pat))
    while n < limit and win[c + n] == pat[n]:
        n += 1
    return n


def starts(win, pat, lo=0):
    """Every window index from ``lo`` on whose two bytes are the pattern's first two, rising."""
    c = win.find(pat[:2], lo)
    while c != -1:
        yield c
        c = win.find(pat[:2], c + 1)


def rule(win, pat, minp):
    """The token at a query whose input is ``pat`` (all that is left of the stream).  -> (token, first match (length, index))"""
    first = (0, 0)
    for c in starts(win, pat):  # find_best_match: the 16-byte ring, min_pattern + 13 at most, longest, ties to the lowest index
        n = lcp(win, c, pat, min(16, minp + 13))
        if n > first[0]:
            first = (n, c)
    n, c = first
    if n < minp:
        return ("L", 1, None), first
    if n <= minp + 11:
        return ("M", n, c), first
    best = first
    for k in starts(win, pat, c):  # candidates at or above the first match: longest, capped, ties to the lowest
        m = lcp(win, k, pat, minp + 131)
        if m > best[0]:
            best = (m, k)
    return ("X",) + best, first


def verify(oracle, case, rec=None, plants=True):
    """Everything the CPU tier asks of one case; raises AssertionError.  ``rec``: the case's line of the fixture; ``plants``: hold
    the window against the design's plants as well."""
    cf = emi.conf(case.window, case.literal)
    win, wp = window_at(oracle, case)
    pat = case.data[case.at:]
    # the window holds every plant where the design put it (a plant of a led stream may run on over the window's end to index 0)
    for index, phrase in case.recipe.plants if plants else ():
        assert bytes(win[(index + j) % cf.W] for j in range(len(phrase))) == phrase, (case.name, "the plant at window index", index)
    by_rule, first = rule(win, pat, cf.minp)
    assert by_rule == case.expect, (case.name, "the rule's token at the query", by_rule, case.expect)
    for k, lazy in enumerate((False, True)):
        rc, blob, at = trace(oracle, case, lazy)
        what = (emi.config_id(case.window, case.literal), case.name, "lazy" if lazy else "greedy")
        assert rc == 0, what
        assert case.at in at, (*what, "a token straddles the query")
        assert said(at[case.at]) == case.expect, (*what, "token at the query", said(at[case.at]), case.expect)
        for pos, tk in case.also:
            assert pos in at and said(at[pos]) == tk, (*what, "token at", pos, pos in at and said(at[pos]), tk)
        for pos, tk in at.items():
            if pos < case.at:
                assert not (tk.kind == "R" and tk.produced > 8) and not (tk.kind == "X" and tk.written < tk.produced), (*what, pos, tk)
                assert tk.wp == pos % cf.W, (*what, pos, tk)
        if rec is not None:
            assert [rc, len(blob), hashlib.sha256(blob).hexdigest()] == rec[k], (*what, "not the recorded reference result")
    return win, wp, first


def hits16(win, pat):
    return [c for c in starts(win, pat) if lcp(win, c, pat, 16) >= 16]


@configs
def test_the_census_is_the_table(window, literal):
    cases = emi.cases(window, literal)
    assert len({c.name for c in cases}) == len(cases)
    for size in (emi.LED, emi.BARE):
        have = {c.cell for c in cases if c.size == size}
        assert len(have) == emi.COUNTS[(window, literal)][size] == sum(c.size == size for c in cases), (size, len(have))
        for cell in emi.CELLS:
            assert (cell in have) != (emi.absent(cell, window, size) is not None), (cell, size, emi.absent(cell, window, size))
        assert have <= set(emi.CELLS)
    for c in cases:
        assert len(c.data) <= emi.MAX_STREAM and (len(c.data) < 1024 if c.size == emi.BARE else c.at >= 1088), c.name
        assert c.dictionary is None if c.size == emi.LED else (len(c.dictionary) == 1 << window and c.at == 8), c.name
    census = collections.Counter(c.cell for c in cases)
    print(f"{emi.config_id(window, literal)}: " + ", ".join(f"{cell} {census[cell]}" for cell in emi.CELLS if census[cell]))


def test_every_cell_exists_somewhere():
    have = {(c.cell, c.size) for cfg in emi.CONFIGS for c in emi.cases(*cfg)}
    assert {cell for cell, _ in have} == set(emi.CELLS)
    both = {cell for cell in emi.CELLS if (cell, emi.LED) in have and (cell, emi.BARE) in have}
    one_size = {"straddle.filter", "run.interior", "written.clip"} | {f"edge.k{k}" for k in emi.EDGE_K}
    assert set(emi.CELLS) - both == one_size | {f"share.d{d}" for d in (2048, 3071, 3072, 16383, 16384, 32000)}  # (those: a dictionary only)


@configs
def test_every_case_takes_its_decision(oracle, golden, window, literal):
    rec = golden[emi.config_id(window, literal)]
    cases = emi.cases(window, literal)
    assert sorted(rec) == sorted(c.name for c in cases)
    cf = emi.conf(window, literal)
    W, s = cf.W, cf.s
    for c in cases:
        win, wp, (n1, first) = verify(oracle, c, rec[c.name])
        pat, hits, (_, length, index) = c.data[c.at:], hits16(win, c.data[c.at:]), c.expect
        what = (c.name, hits, first, wp)
        assert wp == (8 if c.size == emi.BARE else c.at % W), what
        if c.cell.startswith("sole."):
            assert len([k for k in starts(win, pat) if lcp(win, k, pat, 16) >= cf.minp + 12]) == 1 and (index, min(length, cf.minp + 13)) == (first, n1), what
            assert c.cell != "sole.grow" or hits == [first], what
        elif c.cell.startswith(("rival.", "share.")):
            assert len(hits) == (3 if c.cell == "rival.three" else 2) and hits[0] == first, what
            if c.cell.startswith("share."):
                assert hits[1] - hits[0] == int(c.cell[7:]) and index == hits[1], what
        elif c.cell.startswith(("cap.", "edge.")):
            assert len(hits) == (2 if c.cell == "cap.two" else 1) and first == hits[0] == index, what
            assert (length == cf.cap) == (c.cell != "cap.132"), what
            if c.cell.startswith("edge."):
                assert (c.at + int(c.cell[6:])) % emi.EDGE_BLOCK[(window, literal)] == 0, what
        elif c.cell.startswith("clip."):
            high = max(starts(win, pat))
            room = W - high
            assert lcp(win, high, pat, 99) == room == {"clip.win": 20, "clip.tie": 20, "clip.lose": 16, "clip.none": 15}[c.cell] + s, what
            assert (high + n1 + 1 <= W) == (c.cell != "clip.none"), what  # find_extended_match's loop condition (compressor.c:310)
            assert (index + length == W) == (c.cell == "clip.win"), what
        elif c.cell.startswith("straddle"):
            t = (wp - first) % W
            assert 2 <= t < 16 and first + 16 > wp > first, what  # the hit runs past the newest byte
            r0 = (first - wp) % W          # oldest-first offset of the candidate's first byte ...
            r = (r0 + n1 - 3) % W          # ... and of the four bytes around the current end (Walk::ext_search_rounds)
            assert (r > W - 4) == (c.cell == "straddle.filter"), (what, r)
            assert (r0 > W - 4) == (c.cell == "straddle.head"), (what, r0)
            assert (index != first) == (c.cell == "straddle.rival"), what
        elif c.cell.startswith("tail."):
            assert len(pat) == int(c.cell[9:]) + s and len(c.data) == c.at + len(pat), what
        elif c.cell == "run.interior":
            x = cf.sym.x[0]
            assert win[first - 1] == win[first] == win[first + 1] == x and win[first - 18] == x and win[first + 2] != x, what
        elif c.cell == "written.clip":
            assert wp == W - 14 and length == 40 + s, what
        else:
            assert c.cell in ("rle.then.ext", "ext.then.rle"), c.cell


@configs
def test_neighbours_decide_differently(oracle, window, literal):
    groups = collections.defaultdict(list)
    for c in emi.cases(window, literal):
        groups[(c.group, c.size)].append(c)
    for (group, size), members in groups.items():
        if group in ("run", "written"):
            continue  # (cells of their own)
        assert len(members) >= 2, (group, size)
        if group not in ("share", "edge", "rle"):  # (those differ in where the query or the rival stands, not in the token's length)
            assert len({c.expect for c in members}) >= 2, (group, size)
        if size == emi.LED:  # (the plants of a bare stream stand in its dictionary, not in its bytes)
            blobs = [trace(oracle, c, False)[1] for c in members]
            assert len(set(blobs)) == len(members), (group, size)
        assert len({(c.data, c.dictionary) for c in members}) == len(members), (group, size)


def test_a_plant_shortened_by_one_byte_fails_the_check(oracle, golden):
    """The check can fail: every plant of every case at window 2^10, one byte shorter, is refused -- without the fixture too, by the
    window that no longer holds the plant, and in every group of cells some by the tokens alone; so is one deliberately wrong
    expectation."""
    rec = golden[emi.config_id(10, 8)]
    on_token = collections.Counter()
    for c in emi.cases(10, 8):
        for k in range(len(c.recipe.plants)):
            with pytest.raises(AssertionError):
                verify(oracle, emi.shortened(c, k), rec[c.name])
            with pytest.raises(AssertionError, match="the plant at window index"):
                verify(oracle, emi.shortened(c, k))
            try:
                verify(oracle, emi.shortened(c, k), plants=False)
            except AssertionError:
                on_token[c.group] += 1
    print("shortened plants refused by the tokens alone, per group:", dict(on_token))
    assert set(on_token) == {c.group for c in emi.cases(10, 8)}
    c = next(c for c in emi.cases(10, 8) if c.name == "rival.up1-led")
    verify(oracle, c, rec[c.name])
    kind, length, index = c.expect
    with pytest.raises(AssertionError, match="token at the query"):
        verify(oracle, c._replace(expect=(kind, length - 1, index)), rec[c.name])
    with pytest.raises(AssertionError, match="token at the query"):
        verify(oracle, c._replace(expect=(kind, length, c.recipe.plants[0][0])), rec[c.name])


@configs
def test_reference_bytes_are_the_oracles(oracle, ref, window, literal):
    """(skipped where oracle/_ref is not built)"""
    for c in emi.cases(window, literal):
        for lazy in (False, True):
            kw = dict(window=window, literal=literal, extended=True, dictionary=c.dictionary, lazy_matching=lazy)
            assert ref.compress(c.data, **kw) == oracle.compress(c.data, **kw), (c.name, lazy)


@configs
def test_fixture_reproduces_from_the_reference(golden, ref, window, literal):
    """tests/golden/make_ext_cells.py on the live reference gives the committed results (skipped where oracle/_ref is not built)."""
    cid = emi.config_id(window, literal)
    assert gen.generate(ref, [(window, literal)]) == {cid: golden[cid]}
