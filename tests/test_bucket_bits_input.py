"""CPU tier: the inputs of tests/test_gpu_bucket_bits.py aim where they say they aim (tests/bucket_bits_input.py).  Every cell is
read from the oracle's own token trace (tests/long_stream_writer.py's reader): a token starts at the query position, and it has the
stated kind, length and window index, in both formats; neighbours of a group get different tokens; the bytes are the ones recorded
in tests/golden/bucket_bits.json (from the reference C where it is built, which the last test repeats live).

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

import bucket_bits_input as bbi  # noqa: E402
import long_stream_writer as lsw  # noqa: E402

FORMATS = [("ext", True), ("v1", False)]
formats = pytest.mark.parametrize("fmt,extended", FORMATS, ids=[f for f, _ in FORMATS])


def _generator():
    spec = importlib.util.spec_from_file_location("make_bucket_bits", os.path.join(ROOT, "tests", "golden", "make_bucket_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _generator()
_runs = {}


def run(oracle, cell, extended):
    """-> (status, bytes, {input position: token}) of one cell in one format, computed once."""
    key = (cell.name, extended)
    if key not in _runs:
        rc, blob = oracle.compress(cell.data, window=10, literal=8, extended=extended)
        at, pos = {}, 0
        for tk in lsw.read_tokens(blob)[0]:
            at[pos] = tk
            pos += tk.produced
        assert pos == len(cell.data), cell.name
        _runs[key] = (rc, blob, at)
    return _runs[key]


def said(tk):
    return (tk.kind, tk.produced, tk.off)


def test_the_census():
    cells = bbi.cells()
    names = {c.cell for c in cells}
    assert {f"prefix.k{k}" for k in range(2, 17)} <= names
    assert {f"wrap.t{t}" for t in range(2, 17)} | {f"wrap.t{t}.short" for t in range(2, 17)} <= names
    assert {"k3.bit6", "k3.bit7", "oldest.k5", "oldest.k2", "oldest.out", "hit16.two", "hit16.two.rev", "wrap.t2.s3", "wrap.t2.deep",
            "wrap.t3.deep", "tie.low", "tie.index0", "tie.clip", "clip.alone", "clip.longer"} <= names
    assert len(cells) == 2 * len(names) and {c.variant for c in cells} == {"full", "end"}
    for c in cells:
        left = len(c.data) - c.at
        assert len(c.data) < 3072 and (left >= 16 if c.variant == "full" else 2 <= left <= 15), c.name


@formats
def test_every_cell_gets_the_stated_token_at_the_query(oracle, fmt, extended):
    for c in bbi.cells():
        rc, blob, at = run(oracle, c, extended)
        assert rc == 0, c.name
        assert c.at in at, (c.name, fmt, "the parse does not land on the query")
        want = c.expect[fmt]
        got = said(at[c.at])
        print(f"{fmt} {c.name:22s} {got}")
        assert got == want, (c.name, fmt, got, want)
        # nothing but literals and plain matches in front of the query, or an extended match that the window's end does not clip:
        # input position s sits at window index s mod 1,024, as the design assumes
        for pos, tk in at.items():
            if pos < c.at:
                assert tk.kind in "LM" or (tk.kind == "X" and tk.written == tk.produced), (c.name, fmt, pos, tk)
                assert tk.wp == pos % bbi.W, (c.name, fmt, pos, tk)


@formats
def test_the_classes_of_the_scan(oracle, fmt, extended):
    """What the cells are for, restated on the bytes: the index entry of the fixed builds holds a candidate's third byte and the low
    six bits of its fourth, so a candidate is shallow where those differ from the pattern's and deep where they agree."""
    by = {c.name: c for c in bbi.cells()}

    def entry_xor(c, back):
        cand, pat = c.data[c.at - back:c.at - back + 4], c.data[c.at:c.at + 4]
        return (cand[2] ^ pat[2]) | ((cand[3] ^ pat[3]) & 0x3F) << 8

    assert entry_xor(by["prefix.k2-full"], 500) & 0xFF                       # shallow, 2 bytes
    x = entry_xor(by["prefix.k3-full"], 500)
    assert x and not x & 0xFF                                                # shallow, 3 bytes
    for name in ("k3.bit6-full", "k3.bit7-full", "prefix.k4-full", "prefix.k16-full", "oldest.k5-full"):
        assert entry_xor(by[name], 1024 if name.startswith("oldest") else 500) == 0, name  # deep
    assert entry_xor(by["oldest.k2-full"], 1024) & 0xFF
    # the wrap zone: in the kernel's buffer the candidate t bytes in front of the query is followed by the pattern itself
    assert entry_xor(by["wrap.t2-full"], 2) & 0xFF                           # shallow 2 >= t = 2
    x = entry_xor(by["wrap.t3-full"], 3)
    assert x and not x & 0xFF                                                # shallow 3 >= t = 3
    x = entry_xor(by["wrap.t2.s3-full"], 2)
    assert x and not x & 0xFF                                                # shallow 3 >= t = 2
    for name, t in [("wrap.t2.deep-full", 2), ("wrap.t3.deep-full", 3)] + [(f"wrap.t{t}-full", t) for t in range(4, 17)]:
        assert entry_xor(by[name], t) == 0, name                             # deep


@formats
def test_neighbours_decide_differently(oracle, fmt, extended):
    groups = collections.defaultdict(list)
    for c in bbi.cells():
        groups[(c.group, c.variant)].append(c)
    for (group, variant), members in groups.items():
        assert len(members) >= 2, group
        tokens = [said(run(oracle, c, extended)[2][c.at]) for c in members]
        # (the v1 format caps a match at 15 bytes and has no extended match: two 16-byte hits, and the candidate 16 bytes in front
        # of the query with and without its last byte, give it the same token; the extended format tells them apart)
        if variant == "full" and (extended or group not in ("hit16", "wrap.t16")):
            assert len(set(tokens)) >= 2, (group, tokens)
        blobs = [run(oracle, c, extended)[1] for c in members]
        assert len(set(blobs)) == len(members), (group, variant)


@formats
def test_oracle_bytes_are_the_recorded_bytes(oracle, fmt, extended):
    golden = load_golden("bucket_bits.json")
    rec = golden["cases"][fmt]
    assert golden["source"] in ("reference", "oracle")
    assert sorted(rec) == sorted(c.name for c in bbi.cells())
    for c in bbi.cells():
        rc, blob, _ = run(oracle, c, extended)
        assert [rc, len(blob), hashlib.sha256(blob).hexdigest()] == rec[c.name], (fmt, c.name)


def test_fixture_reproduces_from_the_reference(ref):
    """tests/golden/make_bucket_bits.py on the live reference gives the committed results (skipped where oracle/_ref is not built)."""
    assert gen.generate(ref) == load_golden("bucket_bits.json")["cases"]
