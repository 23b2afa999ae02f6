"""Inputs aimed at the decisions of the extended-match search (a plain helper for both test tiers, no fixtures).

In the extended format a first match of min_pattern + 12 bytes or more may grow: the reference searches again on every refill of
its 16-byte ring, each time among the candidates at or above the current one (find_extended_match and the continuation loop of
poll_extended_handling, compressor.c:297-333, 437-468).  Together the searches select "the longest common prefix with the input
among the candidates at or above the first match, capped by the window's end and by min_pattern + 131, ties to the lowest index".
The compress kernel restates that in Walk::ext_search_rounds (one search with the whole look-ahead), in Walk::ext_search /
Walk::serve (the search split over four wavefronts) and in the match phase of the run-aware builds (sole_ext: settled without a
search).  Every decision of the rule has a stream here, next to a neighbour that differs by a byte and decides otherwise.

A stream is ``lead | pattern | tail``; ``cases(window, literal)`` returns ``Case`` records with the cell a stream aims at, the input
position ``at`` of the query, the token the reference must emit there -- ("X", length, window index), ("M", length, index),
("R", count, None) or ("L", 1, None) -- and in ``also`` further (position, token) pairs.  tests/test_ext_match_input.py proves all
of it on the CPU: from the oracle's token trace and from a restatement of the rule over a window it reconstructs itself.

Sizes.  ``led``: the lead is 1,096 bytes or more in which no pair of bytes repeats (lazy_input.pair_filler), so it is literals
only, and the plants overwrite bytes of it: nothing in front of the query is an RLE token of more than 8 bytes or a clipped
extended match, so input position s sits at window index s mod W (the 256-thread builds).  ``bare``: 8 bytes of lead, the plants
in a custom dictionary of W bytes, so window index = dictionary index and window_pos is 8 at the query (under 1 KiB: the
one-wavefront build).  The dictionary's other bytes, the lead's and the pattern's come from disjoint alphabets; a plant ends in a
byte that stands nowhere else in its stream.

Cells (s = min_pattern - 2 is added to every length below; the cap is min_pattern + 131):
  sole.grow sole.k14 sole.k15     one candidate: a common prefix of 20 grows from the 16-byte hit; 14 and 15 cannot grow
  rival.up1 rival.up rival.tie    a higher candidate longer by one byte, by seven, equally long (the lower stays)
  rival.three                     18, 25 and 22 bytes at rising indices: the middle one
  share.d<d>                      a rival longer by one byte d indices above the first match: the lane (64), round (256) and
                                  outer-loop (1,024) boundaries of ext_search_rounds and the quarters of the four wavefronts
  cap.one cap.132 cap.two         a common prefix of 140 gives a token of exactly the cap and a plain match of the other 7; 132
                                  is one short of the cap; two candidates that reach the cap: the lower
  clip.win clip.tie               the higher candidate ends with the window, 20 bytes: it beats 18 (and the token leaves at once,
                                  position + count = W), it does not beat 20
  clip.lose clip.none             the higher candidate is clipped to 16 (a candidate, too short); to 15 (candidate + count + 1 > W:
                                  no candidate)
  straddle straddle.rival         the first match starts t bytes in front of window_pos (t = 10 led, 8 bare) and goes on with the
                                  oldest window bytes; the rival is 3 bytes longer and higher up
  straddle.filter                 t = first match - 1: the four bytes around the current end lie across the write cursor
  straddle.head                   t = 2: the candidate's first four bytes lie across the write cursor
  tail.left<n>                    n = 13..19 bytes from the query to the end of the stream, 18 at a lower index and 40 at a higher:
                                  13 is a plain match, 14..18 stay below with n bytes, 19 moves up
  run.interior                    the window holds x * 20 and a phrase, the pattern is xx + phrase: the first match starts inside
                                  the run
  rle.then.ext ext.then.rle       a run of five in front of the extended match; a run of nine of its last byte behind it
  written.clip                    the query at window_pos W - 14: 14 bytes of a 40-byte match enter the window, so the phrase at
                                  index 0 survives (the next token) and the one at W - 14 does not (literals)
  edge.k<k>                       cap.one with the query k positions in front of a multiple of the launcher's block
``ABSENT`` names the cells a configuration or size cannot have, with the reason; ``COUNTS`` the cases per configuration and size.
"""
import functools
from collections import namedtuple

import numpy as np

import lazy_input as li

Case = namedtuple("Case", "name cell group size data window literal dictionary at expect also recipe")
Recipe = namedtuple("Recipe", "plants pattern tail P pre")  # plants: ((window index, bytes), ...)

BARE, LED = li.BARE, li.LED
CONFIGS = ((10, 8), (8, 8), (12, 8), (15, 8), (15, 7), (11, 5))
P_LED, BARE_LEAD, TAIL = 1096, 8, 24  # 1,096 = 72 mod 256 and mod 1,024
EDGE_K = (1, 2, 15, 16, 17, 132, 133, 134)
#: positions per epoch that tamp_amd_compress_plan gives the led batches, and the multiple of it the edge cells stand in front of
EDGE_BLOCK = {(10, 8): 1024, (8, 8): 1024, (12, 8): 1280, (15, 8): 2048, (15, 7): 2048, (11, 5): 1536}
EDGE_AT = {(10, 8): 2048, (8, 8): 2048, (12, 8): 1280, (15, 8): 2048, (15, 7): 2048, (11, 5): 1536}
SHARE_D = {8: (63, 64, 127, 128, 191, 192), 10: (63, 64, 255, 256, 511, 512, 767, 768), 11: (63, 64, 255, 256, 511, 512, 767, 768),
           12: (63, 64, 255, 256, 511, 512, 767, 768, 1023, 1024, 1025, 2048, 3071, 3072),
           15: (63, 64, 255, 256, 511, 512, 767, 768, 1024, 16383, 16384, 32000)}
TAIL_LEFT = tuple(range(13, 20))
MAX_STREAM = 3584


def config_id(window, literal):
    return f"w{window}-l{literal}"


# ---------------------------------------------------------------------------------------------------------------------
# alphabets
# ---------------------------------------------------------------------------------------------------------------------
Sym = namedtuple("Sym", "long ends dollar sep q x stream bare_stream fill")
_SEED_8 = set(b" \x000ei>to<ans\nr/.")  # the initial dictionary's characters at literal 7 and 8


@functools.lru_cache(maxsize=None)
def symbols(window, literal):
    """long: the phrase every pattern and plant is cut from (no pair of its bytes repeats; literal 5: no three); ends: three bytes
    that end plants; dollar: ends a pattern; sep: stands in front of a pattern; q, x: run bytes; stream: the lead and tail of a led
    stream; bare_stream: of a bare one; fill(W): a dictionary that matches none of these."""
    if literal >= 7:
        letters = bytes(range(65, 89))  # A..X
        pool = bytes(c for c in range(1, 128) if c not in _SEED_8 and c not in letters)
        stream = li.pair_filler(pool[:53])
        rest = np.frombuffer(pool[53:], dtype=np.uint8)

        def fill(W):
            return rest[np.random.default_rng(W).integers(0, len(rest), W)].tobytes()
        return Sym(li.pair_filler(letters[:17])[:170], letters[17:20], letters[20:21], letters[21:22], letters[22:23], letters[23:24],
                   stream, stream[:BARE_LEAD + TAIL], fill)
    assert literal == 5 and li.oracle_min_pattern(window, literal) == 3
    W = 1 << window
    seed = li.initial_dictionary(W, literal)
    own = bytes((2, 6, 7, 10, 11, 16, 17, 22, 24, 25, 26, 27, 28, 29))  # in no initial dictionary of 5-bit literals
    assert not set(own) & set(seed)
    # no three bytes of it repeat, none of the initial dictionary's: literals at minimum pattern 3, as a lead and as a dictionary
    stream = li.triple_filler(bytes(c for c in range(32) if c not in own), W + 320, {seed[i:i + 3] for i in range(len(seed) - 2)})
    # (the straddle cells put the phrase's first t bytes in front of the phrase itself: byte t must not be byte 0 again, or the
    # match of the first copy would run on into the pattern)
    seq = li.triple_filler(own[:7], 200, set())
    k = next(k for k in range(30) if all(seq[k + t] != seq[k] for t in (2, 8, 10, 15)))
    return Sym(seq[k:k + 170], own[7:10], own[10:11], own[11:12], own[12:13], own[13:14],
               stream, stream[W:W + BARE_LEAD + TAIL], lambda n: stream[:n])


Conf = namedtuple("Conf", "window literal W minp s cap sym")


@functools.lru_cache(maxsize=None)
def conf(window, literal):
    minp = li.oracle_min_pattern(window, literal)
    return Conf(window, literal, 1 << window, minp, minp - 2, minp + 131, symbols(window, literal))


# ---------------------------------------------------------------------------------------------------------------------
# assembling a stream
# ---------------------------------------------------------------------------------------------------------------------
def lead_position(P, W, index):
    """The last input position in front of P that lands on window index ``index`` (negative: the lead does not reach it)."""
    return P - ((P - index) % W or W)


def assemble(cf, size, recipe):
    """-> (data, dictionary or None, at).  ``pre``: the bytes right in front of the pattern (default: the separator)."""
    plants, pattern, tail, P, pre = recipe
    sym, W = cf.sym, cf.W
    pre = sym.sep if pre is None else pre
    if size == LED:
        lead = bytearray(sym.stream[:P])
        assert len(lead) == P
        for index, phrase in plants:
            s = lead_position(P, W, index)
            assert 0 <= s and s + len(phrase) <= P - len(pre), (index, s)
            lead[s:s + len(phrase)] = phrase
        lead[P - len(pre):] = pre
        return bytes(lead) + pattern + (sym.stream[P:P + TAIL] if tail else b""), None, P
    custom = bytearray(sym.fill(W))
    assert len(custom) == W
    for index, phrase in plants:
        assert BARE_LEAD <= index and index + len(phrase) <= W, index
        custom[index:index + len(phrase)] = phrase
    lead = bytearray(sym.bare_stream[:BARE_LEAD])
    lead[BARE_LEAD - len(pre):] = pre
    return bytes(lead) + pattern + (sym.bare_stream[BARE_LEAD:] if tail else b""), bytes(custom), BARE_LEAD


def shortened(case, k):
    """``case`` with the phrase of its plant k one byte shorter (the end mark moves up; what it uncovers is the filler again)."""
    plants = list(case.recipe.plants)
    index, phrase = plants[k]
    plants[k] = (index, phrase[:-2] + phrase[-1:])
    data, custom, at = assemble(conf(case.window, case.literal), case.size, case.recipe._replace(plants=tuple(plants)))
    return case._replace(data=data, dictionary=custom, at=at)


# ---------------------------------------------------------------------------------------------------------------------
# the cells of one configuration and size
# ---------------------------------------------------------------------------------------------------------------------
L_TOKEN = ("L", 1, None)


def _designs(cf, size):
    """[(cell, group, plants, pattern, expect, also [(offset from the query, token)], tail, P, pre)]; a cell that the
    configuration cannot have is left out here and named in ABSENT."""
    W, s, cap, sym = cf.W, cf.s, cf.cap, cf.sym
    LONG, (E1, E2, E3), D = sym.long, [bytes([e]) for e in sym.ends], sym.dollar
    led = size == LED
    small = W == 256
    wp = P_LED % W if led else BARE_LEAD
    top = W if (not led or W <= 1024) else P_LED - 1  # one past the highest window index a plant can end at
    i0, i1, i2 = (100, 170, 210) if small else (100, 500, 800)
    out = []

    def add(cell, group, plants, pattern, expect, also=(), tail=True, P=P_LED, pre=None):
        out.append((cell, group, tuple(plants), pattern, expect, tuple(also), tail, P, pre))

    def X(n, index):
        return ("X", n + s, index)

    pat = LONG[:45 + s] + D

    for cell, n in (("sole.grow", 20), ("sole.k14", 14), ("sole.k15", 15)):
        add(cell, "sole", [(i0, LONG[:n + s] + E1)], pat, X(n, i0), [(n + s, L_TOKEN)])

    add("rival.up1", "rival", [(i0, LONG[:20 + s] + E1), (i1, LONG[:21 + s] + E2)], pat, X(21, i1))
    add("rival.up", "rival", [(i0, LONG[:20 + s] + E1), (i1, LONG[:27 + s] + E2)], pat, X(27, i1))
    add("rival.tie", "rival", [(i0, LONG[:20 + s] + E1), (i1, LONG[:20 + s] + E2)], pat, X(20, i0))
    add("rival.three", "rival", [(i0, LONG[:18 + s] + E1), (i1, LONG[:25 + s] + E2), (i2, LONG[:22 + s] + E3)], pat, X(25, i1))

    first = 16 if not led else 100 if W == 1024 else 30 if small else 40
    for d in SHARE_D[cf.window]:
        if first + d + 22 + s <= top:
            add(f"share.d{d}", "share", [(first, LONG[:20 + s] + E1), (first + d, LONG[:21 + s] + E2)], pat, X(21, first + d))

    long_pat = LONG[:140 + s] + D
    add("cap.one", "cap", [(i0, LONG[:140 + s] + E1)], long_pat, ("X", cap, i0), [(cap, ("M", 7, i0 + cap))])
    add("cap.132", "cap", [(i0, LONG[:132 + s] + E1)], long_pat, X(132, i0), [(132 + s, L_TOKEN)])
    if not small:
        add("cap.two", "cap", [(i0, LONG[:140 + s] + E1), (i1, LONG[:140 + s] + E2)], long_pat, ("X", cap, i0))

    if top == W:  # the window's end is within reach of a plant
        low = i0 if small else 300
        hi = W - 20 - s
        clip_pat = LONG[:30 + s] + D
        if led:   # the plant runs on over the window's end: its last 10 bytes stand at index 0
            high, rest, after = [(hi, LONG[:30 + s] + E2)], [], 0
        else:
            high, rest, after = [(hi, LONG[:20 + s])], [(40, LONG[20 + s:30 + s] + E3)], 40
        add("clip.win", "clip", [(low, LONG[:18 + s] + E1)] + high + rest, clip_pat, X(20, hi), [(20 + s, ("M", 10, after))])
        add("clip.tie", "clip", [(low, LONG[:20 + s] + E1)] + high + rest, clip_pat, X(20, low), [(20 + s, ("M", 10, after))])
        for cell, room in (("clip.lose", 16 + s), ("clip.none", 15 + s)):
            add(cell, "clip", [(low, LONG[:18 + s] + E1), (W - room, LONG[:room])], clip_pat, X(18, low))

    if top == W:  # the oldest window bytes are the stream's (or the dictionary's) own
        r_at = 150 if small else 596
        for cell, t, rival in (("straddle", 10 if led else 8, False), ("straddle.rival", 10 if led else 8, True),
                               ("straddle.filter", 14 + s, False), ("straddle.head", 2, False)):
            if t > wp or (not led and t > BARE_LEAD):
                continue
            plants = [(wp, LONG[t:30 + s] + E1)] + ([(r_at, LONG[:33 + s] + E2)] if rival else [])
            add(cell, "straddle", plants, pat, X(33, r_at) if rival else X(30, wp - t), pre=LONG[:t])

    for n in TAIL_LEFT:
        expect = ("M", n + s, i0) if n == 13 else X(n, i0) if n < 19 else X(n, i1)
        add(f"tail.left{n}", "tail", [(i0, LONG[:18 + s] + E1), (i1, LONG[:40] + E2)], LONG[:n + s], expect, tail=False)

    if not led:  # (a run in a stream becomes an RLE token, which writes 8 bytes of it to the window)
        add("run.interior", "run", [(i0, sym.x * 20 + LONG[:20 + s] + E1)], sym.x * 2 + LONG[:20 + s] + D, X(22, i0 + 18))
    add("rle.then.ext", "rle", [(i0, LONG[:20 + s] + E1)], pat, X(20, i0), [(-5, ("R", 5, None))], pre=sym.q * 6)
    add("ext.then.rle", "rle", [(i0, LONG[:20 + s] + E1)], LONG[:20 + s] + LONG[19 + s:20 + s] * 9 + D, X(20, i0), [(20 + s, ("R", 9, None))])

    if led and W <= 2048:
        P = (1088 + 14 + W - 1) // W * W - 14
        plants = [(i0, LONG[:40 + s] + E1), (0, LONG[150:160] + E2)]
        if lead_position(P, W, W - 14) >= 0:
            plants.append((W - 14, LONG[160:170] + E3))
        add("written.clip", "written", plants, LONG[:40 + s] + LONG[150:160] + LONG[160:170] + D, X(40, i0),
            [(40 + s, ("M", 10, 0)), (50 + s, L_TOKEN)], P=P)

    if led:
        for k in EDGE_K:
            P = EDGE_AT[(cf.window, cf.literal)] - k
            # (window 2^8: a plant that holds neither the write cursor nor the separator in front of it)
            room = [i for i in (100, 10) if not any(i <= (P - b) % W < i + 141 + s for b in (0, 1))] if small else [100]
            if room:
                add(f"edge.k{k}", "edge", [(room[0], LONG[:140 + s] + E1)], long_pat, ("X", cap, room[0]), [(cap, ("M", 7, room[0] + cap))], P=P)
    return out


@functools.lru_cache(maxsize=None)
def cases(window, literal):
    cf = conf(window, literal)
    out = []
    for size in (LED, BARE):
        for cell, group, plants, pattern, expect, also, tail, P, pre in _designs(cf, size):
            recipe = Recipe(plants, pattern, tail, P, pre)
            data, custom, at = assemble(cf, size, recipe)
            assert len(data) <= MAX_STREAM and (len(data) < 1024 if size == BARE else at >= 1088), (cell, size, len(data))
            out.append(Case(f"{cell}-{size}", cell, group, size, data, window, literal, custom, at, expect,
                            tuple((at + o, tk) for o, tk in also), recipe))
    return tuple(out)


#: every cell, in the order of the module's docstring
CELLS = tuple(["sole.grow", "sole.k14", "sole.k15", "rival.up1", "rival.up", "rival.tie", "rival.three"]
              + [f"share.d{d}" for d in sorted({d for ds in SHARE_D.values() for d in ds})]
              + ["cap.one", "cap.132", "cap.two", "clip.win", "clip.tie", "clip.lose", "clip.none", "straddle", "straddle.rival",
                 "straddle.filter", "straddle.head"] + [f"tail.left{n}" for n in TAIL_LEFT]
              + ["run.interior", "rle.then.ext", "ext.then.rle", "written.clip"] + [f"edge.k{k}" for k in EDGE_K])

#: cells that a configuration or size cannot have: (cells by prefix, windows, sizes, reason); share.d<d>: see absent()
ABSENT = (
    ("cap.two", (8,), None, "two plants of 141 bytes do not fit 256"),
    ("clip. straddle", (11, 12, 15), (LED,), "the window's end and its oldest bytes hold the initial dictionary: the lead does not reach them"),
    ("straddle.filter", None, (BARE,), "a first match less one is 14 bytes or more in front of window_pos, the lead is 8"),
    ("run.interior", None, (LED,), "a run of 20 in a stream is an RLE token that writes 8 bytes: it never stands in the window"),
    ("written.clip", None, (BARE,), "window_pos is 8 at the query"),
    ("written.clip", (12, 15), (LED,), "window_pos W - 14 lies 4 KB and more into the stream"),
    ("edge.k", None, (BARE,), "one epoch"),
    ("edge.k132 edge.k133 edge.k134", (8,), (LED,), "window_pos 122..124: a plant of 141 bytes in 256 lies across it"),
)

#: cases per configuration and size
COUNTS = {
    (10, 8): {LED: 44, BARE: 35}, (8, 8): {LED: 38, BARE: 32}, (12, 8): {LED: 38, BARE: 41}, (15, 8): {LED: 36, BARE: 39},
    (15, 7): {LED: 36, BARE: 39}, (11, 5): {LED: 36, BARE: 35},
}


def absent(cell, window, size):
    """The reason ``cell`` has no case at this window and size, or None."""
    if cell.startswith("share.d"):
        d, W = int(cell[7:]), 1 << window
        if d not in SHARE_D[window]:
            return "no boundary of the search at this window (SHARE_D)"
        if size == LED and W > 1024 and d > 1024 + 8:
            return "a lead of 1,096 bytes fills window indices 0..1,094 only: the first match at 40, the rival below 1,073"
        return None
    for prefixes, windows, sizes, reason in ABSENT:
        if any(cell.startswith(p) for p in prefixes.split()) and (windows is None or window in windows) and (sizes is None or size in sizes):
            return reason
    return None
