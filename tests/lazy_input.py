"""Inputs aimed at the decisions of lazy matching (a plain helper for both test tiers, no fixtures).

lazy_matching=True is about twenty lines of the reference (compressor.c:576-619): take the match at this position (cached at the
previous one, handed over by the RLE arbitration, or searched now); if it is min_pattern..8 bytes long and the ring holds more than
len + 2 bytes, probe the next position; if the probe is longer and its source does not cover window_pos (the slot the literal is
about to overwrite), emit a literal and cache the probe, else take the match.  The library restates that three times (the walk's
state machine, the probe tables with their pointer-doubled vstep table, the resume kernel's object state), so every decision has an
input here that takes it, next to a neighbour that differs by one and decides otherwise.

``cases(window, literal, extended)`` returns ``Case`` records.  Each names the ``cell`` it aims at, the input position ``at`` of the
decision and what the oracle's decision event there (oracle_set_lazy_cb, oracle/tamp_oracle.h) must say (``expect``, and ``also`` for
further positions); ``group`` ties neighbours whose outcomes differ.  tests/test_lazy_input.py proves all of it on the CPU.

Sizes.  ``bare``: under 1 KiB, the one-wavefront lazy launch.  ``led``: behind a lead of at least 1,088 bytes that are all
literals, from an alphabet the cell does not use (the 256-thread launch).  For the decision at input position 0 the lead follows the
cell, there being nothing in front of position 0.  The epoch-edge streams (j) have one size, 2.4 KB.

The designs are written in terms of window_pos.  Nothing here makes an RLE token of more than 8 bytes or a clipped extended match
in front of a decision, so the byte at input position s sits at window index s mod W, and a design that needs bytes AHEAD of
window_pos (d, g.pattern, i.*) takes them from the previous lap of the stream where there is one (window 2^8 bare and led, 2^10
led) and from a custom dictionary otherwise; such cases carry ``dictionary``.  The overlap cells (d) come both ways at every window.

Cells (minimum pattern 2 unless said):
  a.defer a.tie a.lose          nlen = len + 1, len, len - 1
  b.len8 b.len9                 the last length that probes, the first that does not
  b.min b.below                 len = min_pattern probes; len = min_pattern - 1 is a literal without a probe
                                (also at min_pattern 3: window 15 with literal 7, window 11 with literal 5)
  c.ring<len>.probe / .none     len = 2..8 with the stream ending len + 3 / len + 2 bytes behind the match's start: R = len + 3
                                probes and defers (the cached length is the probe's cap R - 1 = the bytes left), R = len + 2 does not
  d.<k>[.copy][.wrap]           the probe's source of 6 bytes at nidx = wp - k, k = -1, 0, 1, 5, 6: defer, overlap, overlap,
                                overlap, defer; .copy adds the same 6 bytes 64 indices further up, clear of wp (the reference keeps
                                the lowest-index candidate and refuses; a search that drops overlapping candidates finds the copy
                                and defers); .wrap: without a dictionary, behind a wrapped window
  e.ext14 e.ext15               a cached match of min_pattern + 12 / + 13 bytes starts an extended match; the first cannot grow,
                                the second grows to 20; in v1 both are plain tokens
  f.chain2 f.chain3             two and three defers in a row; the last cached match (8 bytes or less) is probed again and loses
  g.one                         deferred literal x, then one x: the RLE handler falls through, the cached match is used
  g.pattern                     deferred literal x, then a run of two x that loses the RLE arbitration to a pattern: the CACHED match
                                (5 bytes) is used, not the 6 bytes the arbitration found on the window with the new x in it
  g.run                         deferred literal x, then a run of seven x: longer than the arbitration looks at, the run wins and the
                                cached match is dropped.  Reachable after all: a probe of x only cannot beat the match at the
                                previous position, but "x^7 z" in the window and "x^8 z" in the input give len = 7 (x^7) and
                                nlen = 8 (x^7 z), and a run of seven is emitted without asking the pattern (compressor.c:490)
  h.deferred h.cached h.after   literal 7: the byte that does not fit is the deferred literal itself (TAMP_EXCESS_BITS), the first
                                byte of the cached match (a match token carries it: no error), the literal behind the cached match
  i.end_at_W                    the probe's source ends exactly at W and the pattern goes on at index 0: clipped, nlen = 5
  i.start_at_W-1 i.inside       the only full copy of the probe starts at index W - 1 (no candidate: the probe loses); one lower, it wins
  i.first                       the first decision of the stream is a defer (position 0, cached state at 1), on the initial dictionary
  j.plain j.chain               a defer (a chain of two) every 37 positions over 2.4 KB: 37 is coprime to 64
"""
import functools
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name cell group size data window literal extended dictionary at expect also status")

BARE, LED = "bare", "led"
LEAD = {BARE: 8, LED: 1096}   # 1,096 = 72 mod 256 and mod 1,024: cells of up to 180 bytes stay clear of the window's end
WRAP_LEAD_8 = 264             # window 2^8, bare: one lap and 8 bytes
TAIL = 24                     # literal bytes behind a cell, so that the ring is full at its decisions
EXCESS_BITS = -2

OVERLAP_K = (-1, 0, 1, 5, 6)
RING_LENS = tuple(range(2, 9))
J_UNITS, J_PERIOD = 65, 37


# ---------------------------------------------------------------------------------------------------------------------
# literal filler
# ---------------------------------------------------------------------------------------------------------------------
def initial_dictionary(size, literal):
    """common.c:28-52: xorshift32 from 3758097560, one draw per 8 bytes, a nibble picks from 16 characters."""
    text = b" etaoinshrdlcumw"
    table = bytes(c & 0x1F for c in text) if literal <= 5 else bytes(c & 0x3F for c in text) if literal == 6 else b" \x000ei>to<ans\nr/."
    out, s, draw = bytearray(size), 3758097560, 0
    for i in range(size):
        if i & 7 == 0:
            s ^= (s << 13) & 0xFFFFFFFF
            s ^= s >> 17
            s ^= (s << 5) & 0xFFFFFFFF
            draw = s
        out[i] = table[draw & 15]
        draw >>= 4
    return bytes(out)


def pair_filler(alphabet):
    """Every ordered pair of two different symbols of a prime-sized alphabet exactly once, no symbol next to itself: for each step
    d the cycle 0, d, 2d, ... -- so no two bytes of it repeat and a compressor sees literals only."""
    A = len(alphabet)
    assert A > 2 and all(A % k for k in range(2, A))
    return bytes(alphabet[(i * d) % A] for d in range(1, A) for i in range(A))


def triple_filler(alphabet, n, forbidden):
    """``n`` bytes over ``alphabet`` in which no three bytes repeat, none of ``forbidden`` (a set of 3-byte strings) occurs and no
    symbol stands next to itself (greedy: the successor with the most unused continuations)."""
    used, out = set(forbidden), [alphabet[0], alphabet[1]]

    def free(a, b):
        return [c for c in alphabet if c != b and bytes((a, b, c)) not in used]

    while len(out) < n:
        a, b = out[-2], out[-1]
        c = max(free(a, b), key=lambda c: (len(free(b, c)), -c))
        used.add(bytes((a, b, c)))
        out.append(c)
    return bytes(out)


LEAD_ALPHABET_8 = bytes(range(0x80, 0x80 + 37))
LEAD_ALPHABET_7 = bytes([*range(1, 10), *range(11, 32), *range(33, 40)])  # not in the initial dictionary, no letter or digit
CELL_SYMBOLS_5 = bytes((2, 6, 7, 10, 11, 16, 17, 22, 24))                 # what "ABCDE1234" becomes at literal 5


@functools.lru_cache(maxsize=None)
def filler(window, literal, extended):
    if literal == 8:
        return pair_filler(LEAD_ALPHABET_8)
    if literal == 7:
        return pair_filler(LEAD_ALPHABET_7)
    assert literal == 5 and oracle_min_pattern(window, literal) == 3
    seed = initial_dictionary(1 << window, literal if extended else 8)
    return triple_filler(bytes(c for c in range(32) if c not in CELL_SYMBOLS_5), LEAD[LED] + TAIL + 8,
                         {seed[i:i + 3] for i in range(len(seed) - 2)})


def oracle_min_pattern(window, literal):
    return 2 + (window > 10 + 2 * (literal - 5))


# ---------------------------------------------------------------------------------------------------------------------
# cells: fn(W) -> (cell bytes, offset of the decision, expect, also [(offset, expect)], ahead [(kind, index, bytes)])
# ahead: bytes the window must hold at ("rel": window_pos of the decision + index, "abs": index) when the decision is taken
# ---------------------------------------------------------------------------------------------------------------------
def ev(event, origin=None, **kw):
    d = dict(event=event, **kw)
    if origin:
        d["origin"] = origin
    return d


def cell_a(which):
    plant = {"defer": b"2BCDE3", "tie": b"2BCD3", "lose": b"23"}[which]
    nlen = {"defer": 4, "tie": 3, "lose": 2}[which]

    def fn(W):
        cell = b"ABC1" + plant + b"ABCDE5"
        return cell, 4 + len(plant), ev("defer" if which == "defer" else "tie_or_shorter", "fresh", len=3, nlen=nlen), [], []
    return fn


def cell_b_len(n):
    def fn(W):
        q = b"ABCDEFGHIJK"
        cell = q[:n] + b"1" + b"2" + q[1:] + b"3" + q + b"4"
        return cell, n + 1 + 12, (ev("defer", "fresh", len=8, nlen=10) if n == 8 else ev("no_probe_len", "fresh", len=9)), [], []
    return fn


def cell_b_min(minp, below):
    def fn(W):
        q = b"ABCDE"[:minp + 2]
        first = q[:minp - 1] if below else q[:minp]
        cell = first + b"1" + b"2" + q[1:] + b"3" + q + b"4"
        at = len(first) + 3 + len(q) - 1
        if below:
            return cell, at, ev("no_probe_len", "fresh"), [], []
        return cell, at, ev("defer", "fresh", len=minp, nlen=minp + 1), [(at + 1, ev("tie_or_shorter", "cached", len=minp + 1))], []
    return fn


def cell_c(n, probe):
    def fn(W):
        q = b"ABCDEFGHIJKL"[:n + 3]
        cell = q[:n] + b"1" + b"2" + q[1:] + b"3" + (q if probe else q[:-1])
        at = n + 2 + n + 2 + 1
        if probe:
            return cell, at, ev("defer", "fresh", len=n, nlen=n + 2, ring=n + 3), [(at + 1, ev(None, "cached", len=n + 2, ring=n + 2))], []
        return cell, at, ev("no_probe_ring", "fresh", len=n, ring=n + 2), [], []
    return fn


def cell_d(k, copy):
    def fn(W):
        q = b"ABCDEFG"
        pre = q[1:1 + max(k, 0)]
        cell = b"ABC1" + b"2" + pre + q + b"5"
        ahead = [("rel", 1, q[1:])] if k < 0 else [("rel", 0, q[1 + k:])] if k < 6 else []
        if copy:
            ahead.append(("rel", 64, q[1:]))
        return cell, 5 + len(pre), ev("defer" if k in (-1, 6) else "overlap", "fresh", len=3, nlen=6, rel=-k), [], ahead
    return fn


def cell_e(n, extended):
    def fn(W):
        q = b"ABCDEFGHIJKLMNOPQRSTUV"
        planted = q[1:15] if n == 14 else q[1:21]
        cell = b"ABC1" + b"2" + planted + b"3" + q[:1] + planted + b"4"
        at = 6 + len(planted)
        also = [(at + 1, ev("no_probe_len", "cached", len=n))]
        if extended:
            also.append((at + 1, ev("cached_to_ext", len=n)))
        return cell, at, ev("defer", "fresh", len=3, nlen=n), also, []
    return fn


def cell_f(n):
    def fn(W):
        if n == 2:
            cell, at = b"AB1" + b"2BCD3" + b"4CDEF5" + b"ABCDEF6", 14
        else:
            cell, at = b"AB1" + b"2BCD3" + b"4CDEF5" + b"7DEFGH8" + b"ABCDEFGH9", 21
        also = [(at + k, ev("defer", "cached", len=k + 2, nlen=k + 3)) for k in range(1, n)]
        also.append((at + n, ev("tie_or_shorter", "cached", len=n + 2)))
        return cell, at, ev("defer", "fresh", len=2, nlen=3), also, []
    return fn


def cell_g_one(W):
    return b"1XX2" + b"3XBCD4" + b"5XXBCD6", 11, ev("defer", "fresh", len=2, nlen=4), [(12, ev("tie_or_shorter", "cached", len=4))], []


def cell_g_pattern(extended):
    def fn(W):
        also = [(14, ev("cached_over_rle", len=5, nlen=6))] if extended else []
        also.append((14, ev("tie_or_shorter", "cached", len=5)))
        return b"1XXX2" + b"3XXBCD4" + b"5" + b"XXXBCDE6", 13, ev("defer", "fresh", len=3, nlen=5), also, [("rel", 1, b"XBCDE")]
    return fn


def cell_g_run(extended):
    def fn(W):
        also = [(12, ev("dropped_by_rle", len=8))] if extended else [(12, ev(None, "cached", len=8))]
        return b"1" + b"X" * 7 + b"Z2" + b"3" + b"X" * 8 + b"Z4", 11, ev("defer", "fresh", len=7, nlen=8), also, []
    return fn


def cell_h(which):
    def fn(W):
        if which == "deferred":  # needs the byte in the window already: only a dictionary can hold it
            return b"1" + b"\xC1BCD4", 1, ev("defer", "fresh", len=2, nlen=3), [], [("rel", 100, b"\xC1B1"), ("rel", 120, b"2BCD3")]
        if which == "cached":
            return b"1" + b"A\xC1CD4", 1, ev("defer", "fresh", len=2, nlen=3), [(2, ev(None, "cached", len=3))], \
                [("rel", 100, b"A\xC11"), ("rel", 120, b"2\xC1CD3")]
        return b"ABC1" + b"2BCDE3" + b"ABCDE" + b"\xC1", 10, ev("defer", "fresh", len=3, nlen=4), [(11, ev(None, "cached", len=4))], []
    return fn


def cell_i(which):
    def fn(W):
        if which == "end_at_W":
            return b"ABC1" + b"2" + b"ABCDEFG5", 5, ev("defer", "fresh", len=3, nlen=5, nidx=W - 5), [], [("abs", W - 5, b"BCDEF"), ("abs", 0, b"G")]
        if which == "start_at_W-1":
            return b"ABC1" + b"2" + b"ABCDEF5", 5, ev("tie_or_shorter", "fresh", len=3, nlen=2), [], [("abs", W - 1, b"B"), ("abs", 0, b"CDEF")]
        return b"ABC1" + b"2" + b"ABCDEF5", 5, ev("defer", "fresh", len=3, nlen=5, nidx=W - 6), [], [("abs", W - 6, b"BCDEF")]
    return fn


# ---------------------------------------------------------------------------------------------------------------------
# assembling a stream around a cell
# ---------------------------------------------------------------------------------------------------------------------
def dictionary_fill(W):
    """A custom dictionary that matches nothing: bytes 0xD0..0xFF, which no stream here holds."""
    return bytearray((0xD0 + np.random.default_rng(W).integers(0, 0x30, W)).astype(np.uint8).tobytes())


def assemble(fn, window, literal, extended, lead_len, with_tail=True, dictionary="auto", translate=None):
    """lead | cell | tail with the cell's ``ahead`` bytes put where the window holds them when the decision is taken: in the
    previous lap of the stream, or in a custom dictionary (``dictionary``: "auto" = only when needed, "never" -> None when
    needed, "always").  -> (data, dictionary or None, cell, at, expect, also) or None."""
    W = 1 << window
    fil = filler(window, literal, extended)
    cell, at, expect, also, ahead = fn(W)
    if translate:
        cell = cell.translate(translate)
    lead = bytearray(fil[:lead_len])
    custom = dictionary_fill(W) if dictionary == "always" else None
    p = lead_len + at
    for kind, index, phrase in ahead:
        for j, byte in enumerate(phrase):
            x = (p + index + j) % W if kind == "rel" else index + j
            assert x < W
            s = lead_len - ((lead_len - x) % W or W)  # the last input position in front of the cell that lands on index x
            if s >= 0:
                lead[s] = byte
            elif dictionary == "never":
                return None
            else:
                custom = custom if custom is not None else dictionary_fill(W)
                custom[x] = byte
    data = bytes(lead) + cell + (fil[lead_len:lead_len + TAIL] if with_tail else b"")
    shift = lambda items: [(lead_len + o, e) for o, e in items]  # noqa: E731
    return data, (bytes(custom) if custom is not None else None), lead_len + at, expect, shift(also)


def _best(win, pat, cap):
    """find_best_match on a window that nothing has been written to yet -> (length, index)."""
    W, best = len(win), (0, 0)
    i = win.find(pat[:2])
    while i != -1 and i + 1 < W:
        n = 2
        while n < cap and n < len(pat) and i + n < W and win[i + n] == pat[n]:
            n += 1
        if n > best[0]:
            best = (n, i)
        i = win.find(pat[:2], i + 1)
    return best


@functools.lru_cache(maxsize=None)
def first_decision(window, literal, extended):
    """i.first: b0 | five bytes of the initial dictionary | text.  b0 and the first of the five stand together somewhere in the
    dictionary (a match at position 0), the five stand further up (the probe at position 1 is longer)."""
    seed = initial_dictionary(1 << window, literal if extended else 8)
    for j in range(16, len(seed) - 16):
        s = seed[j:j + 5]
        if any(s[k] == s[k + 1] for k in range(4)):
            continue
        for b0 in sorted(set(seed) - {s[0], seed[-1]}):
            data = bytes([b0]) + s + b"QRSTUVWXYZKLMNOPJ"
            n0, _ = _best(seed, data[:16], 16)
            n1, i1 = _best(seed, data[1:16], 15)
            if 2 <= n0 <= 8 and n1 > n0 and i1 >= 1:
                return data, n0, n1, i1
    raise AssertionError("no first-decision defer on the initial dictionary")


J_FILL = bytes(range(0x80, 0x80 + 53))
J_FIRST = bytes(range(0xB5, 0xB5 + J_UNITS))
J_THIRD = bytes([*range(1, 10), *range(11, 32), *range(33, 46), *range(49, 60), 61, 63, 64, *b"FGIJKLMN"])[:J_UNITS]


@functools.lru_cache(maxsize=None)
def epoch_stream(chain):
    """j: units of 37 bytes, each with its own first byte a (and third byte c), so that no unit finds more than its own plants:
      plain   a B | 30 literals | a B C D E          "aB" is 2 bytes, "BCDE" (planted once, and in every earlier unit) 4: defer
      chain   a B . B c D . c D E H . | 20 literals | a B c D E H     2, then "BcD" 3, then "cDEH" 4: two defers, then "DEH" loses
    -> (data, [(position, expect)])."""
    fil = pair_filler(J_FILL)
    # (28 literals in front of the chain units: none of their plants then lies across a multiple of 256, any window's end)
    out, marks, used = bytearray(fil[-28:] if chain else b"2BCDE3"), [], 0
    for i in range(J_UNITS):
        a, c = J_FIRST[i:i + 1], J_THIRD[i:i + 1]
        if chain:
            unit = a + b"B" + fil[used:used + 1] + b"B" + c + b"D" + fil[used + 1:used + 2] + c + b"DEH" + fil[used + 2:used + 22]
            used += 22
            query = a + b"B" + c + b"DEH"
        else:
            unit = a + b"B" + fil[used:used + 30]
            used += 30
            query = a + b"BCDE"
        out += unit
        p = len(out)
        out += query
        marks.append((p, ev("defer", "fresh", len=2, nlen=3 if chain else 4)))
        if chain:
            marks.append((p + 1, ev("defer", "cached", len=3, nlen=4)))
            marks.append((p + 2, ev("tie_or_shorter", "cached", len=4)))
        else:
            marks.append((p + 1, ev("tie_or_shorter", "cached", len=4)))
    assert len(out) == J_UNITS * J_PERIOD + (28 if chain else 6)
    return bytes(out) + fil[used:used + TAIL], tuple(marks)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of one configuration
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases(window, literal=8, extended=True):
    W, minp = 1 << window, oracle_min_pattern(window, literal)
    out = []

    def add(cell, group, fn, *, sizes=(BARE, LED), with_tail=True, dictionary="auto", lead=None, status=0, suffix="", translate=None):
        for size in sizes:
            lead_len = (lead or {}).get(size, LEAD[size])
            got = assemble(fn, window, literal, extended, lead_len, with_tail, dictionary, translate)
            if got is None:
                continue
            data, custom, at, expect, also = got
            assert len(data) <= 4096 and (len(data) < 1024 if size == BARE else len(data) >= 1088)
            name = f"{cell}{suffix}-{size}"
            out.append(Case(name, cell, group, size, data, window, literal, extended, custom, at, expect, tuple(also), status))

    if literal == 7 and minp == 2:  # h: the excess-bits cells (the lead must not wrap: its bytes fit 7 bits, the dictionary's do not)
        assert W > LEAD[LED] + 256
        add("h.deferred", "h.deferred", cell_h("deferred"), status=EXCESS_BITS)
        add("h.cached", "h.cached", cell_h("cached"))
        add("h.after", "h.after", cell_h("after"), status=EXCESS_BITS, with_tail=False)
        return tuple(out)
    if minp == 3:
        tr = bytes.maketrans(b"ABCDE1234", CELL_SYMBOLS_5) if literal == 5 else None
        add("b.min", "b.min3", cell_b_min(3, False), suffix=".min3", translate=tr)
        add("b.below", "b.min3", cell_b_min(3, True), suffix=".min3", translate=tr)
        return tuple(out)
    assert literal == 8

    # where bytes ahead of window_pos come from: the previous lap (window 2^8: a lead of one lap and 8 bytes; 2^10: the led size), else a dictionary
    lap = {BARE: WRAP_LEAD_8} if window == 8 else None
    for which in ("defer", "tie", "lose"):
        add("a." + which, "a", cell_a(which))
    add("b.len8", "b.len", cell_b_len(8))
    add("b.len9", "b.len", cell_b_len(9))
    add("b.min", "b.min", cell_b_min(2, False))
    add("b.below", "b.min", cell_b_min(2, True))
    for n in RING_LENS:
        add(f"c.ring{n}.probe", f"c.ring{n}", cell_c(n, True), with_tail=False)
        add(f"c.ring{n}.none", f"c.ring{n}", cell_c(n, False), with_tail=False)
    for copy in (False, True):
        tag = ".copy" if copy else ""
        for k in OVERLAP_K:
            add(f"d.{k}{tag}", "d" + tag, cell_d(k, copy), dictionary="always")
            add(f"d.{k}{tag}.wrap", "d.wrap" + tag, cell_d(k, copy), dictionary="never", lead=lap)
    add("e.ext14", "e", cell_e(14, extended))
    add("e.ext15", "e", cell_e(15, extended))
    add("f.chain2", "f", cell_f(2))
    add("f.chain3", "f", cell_f(3))
    add("g.one", "g", cell_g_one)
    add("g.pattern", "g", cell_g_pattern(extended), lead=lap)
    add("g.run", "g", cell_g_run(extended))
    for which in ("end_at_W", "start_at_W-1", "inside"):
        add("i." + which, "i", cell_i(which), lead=lap)

    data, n0, n1, i1 = first_decision(window, literal, extended)
    first = (ev("defer", "fresh", len=n0, nlen=n1, nidx=i1), ((1, ev(None, "cached", len=n1)),))
    fil = filler(window, literal, extended)
    out.append(Case("i.first-bare", "i.first", "i.first", BARE, data, window, literal, extended, None, 0, *first, 0))
    out.append(Case("i.first-led", "i.first", "i.first", LED, data + fil[:LEAD[LED]], window, literal, extended, None, 0, *first, 0))
    for chain in (False, True):
        data, marks = epoch_stream(chain)
        cell = "j.chain" if chain else "j.plain"
        out.append(Case(cell, cell, cell, LED, data, window, literal, extended, None, marks[0][0], marks[0][1], marks[1:], 0))
    return tuple(out)


SWEEP_POOL = bytes(c for c in range(1, 256) if c not in b" \x000ei>to<ans\nr/." and c not in LEAD_ALPHABET_8)


@functools.lru_cache(maxsize=None)
def sweep_source(window, extended):
    """The cells that need no bytes ahead of window_pos, one behind the other in ONE stream of 0.6 KB (for the sweeps that cut a
    stream at every byte, and for dictionary-reset segments): every cell is spelled in symbols of its own, so that it finds its own
    plants only, stands behind 20 literals, and does not lie across a multiple of 256 (any window's end); the ring-gate cell comes
    last, the stream ending where it needs it to.  -> (data, ((position, expect, cell), ...))."""
    fil = pair_filler(LEAD_ALPHABET_8)
    cells = [("a.defer", cell_a("defer")), ("a.tie", cell_a("tie")), ("a.lose", cell_a("lose")), ("b.len8", cell_b_len(8)),
             ("b.len9", cell_b_len(9)), ("b.min", cell_b_min(2, False)), ("b.below", cell_b_min(2, True)), ("f.chain2", cell_f(2)),
             ("f.chain3", cell_f(3)), ("g.one", cell_g_one), ("g.run", cell_g_run(extended)), ("e.ext14", cell_e(14, extended)),
             ("e.ext15", cell_e(15, extended)), ("c.ring5.probe", cell_c(5, True))]
    out, marks, used, taken = bytearray(), [], 0, 0
    for name, fn in cells:
        cell, at, expect, also, ahead = fn(1 << window)
        assert not ahead
        symbols = bytes(sorted(set(cell)))
        cell = cell.translate(bytes.maketrans(symbols, SWEEP_POOL[taken:taken + len(symbols)]))
        taken += len(symbols)
        assert taken <= len(SWEEP_POOL)
        pad = 20
        if (len(out) + pad) % 256 + len(cell) > 256:
            pad += 256 - (len(out) + pad) % 256
        out += fil[used:used + pad]
        used += pad
        marks += [(len(out) + o, e, name) for o, e in [(at, expect), *also]]
        out += cell
    return bytes(out), tuple(marks)


#: every cell some configuration must reach (tests/test_lazy_input.py prints the census)
CELLS = tuple(
    ["a.defer", "a.tie", "a.lose", "b.len8", "b.len9", "b.min", "b.below"]
    + [f"c.ring{n}.{w}" for n in RING_LENS for w in ("probe", "none")]
    + [f"d.{k}{c}{w}" for k in OVERLAP_K for c in ("", ".copy") for w in ("", ".wrap")]
    + ["e.ext14", "e.ext15", "f.chain2", "f.chain3", "g.one", "g.pattern", "g.run", "h.deferred", "h.cached", "h.after",
       "i.end_at_W", "i.start_at_W-1", "i.inside", "i.first", "j.plain", "j.chain"])

#: (window, literal) of the configurations the tests run: the four lazy builds' windows, and the three with other literal widths
CONFIGS_8 = (8, 10, 13, 15)
CONFIGS_OTHER = ((15, 7), (11, 5), (12, 7))


def matches(event, expect):
    """Does a LazyEvent say what ``expect`` asks?  (rel: nidx - wp)"""
    for k, v in expect.items():
        if v is None:
            continue
        got = event.nidx - event.wp if k == "rel" else getattr(event, k)
        if got != v:
            return False
    return True
