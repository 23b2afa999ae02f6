"""Inputs aimed at the bucket scan's candidate arithmetic (a plain helper for both test tiers, no fixtures).

The fixed-geometry compress builds (window 2^10, literal 8, default parse) read a candidate's class off the first set bit of its
index entry XORed with the query's, and keep its length in bit units (tamp_common.hpp: scan_shallow_bits, scan_deep_bits).  Every
value of that arithmetic that decides something has a stream here, next to a neighbour that decides otherwise.

A stream is ``lead | pattern | tail``: the lead is P = 1,096 bytes in which no pair of bytes repeats (lazy_input.pair_filler), so
it compresses to literals and the greedy parse lands on input position P, the QUERY; the cell's plants overwrite bytes of the
lead.  Nothing in front of the query is an RLE token or a clipped extended match, so input position s sits at window index
s mod 1,024: a plant that starts ``back`` bytes in front of the query is the candidate at window index (P - back) mod 1,024.
The window at the query is the 1,024 bytes in front of it: its oldest byte is input position P - 1,024 = 72, at window_pos.

``cells()`` returns ``Cell`` records: the stream, the query position, and per format ("ext", "v1") what the token at the query
must be -- (kind, length, window index), kind "L" (a literal: no match), "M" (a match) or "X" (an extended match).
tests/test_bucket_bits_input.py proves all of it on the CPU from the oracle's token trace.

Cells (PAT = "ABCDEFGHIJKLMNOPQRST", plants end in a byte no pattern holds):
  prefix.k<k>        k = 2..16: one candidate whose common prefix with the pattern is exactly k (k = 16: it goes on to 20, an
                     extended match in the extended format; 14 and 15 are extended matches that cannot grow)
  k3.bit6 k3.bit7    k = 3 where byte 3 differs from the pattern's in bit 6 / bit 7 only: the entry (which holds its low six bits)
                     agrees, the compare returns 3.  (prefix.k3 differs in the low six bits: the entry decides)
  oldest.k5          the candidate at the oldest window byte, entry in agreement: y == 0
  oldest.k2          ... with byte 2 different: y is the XOR of the low bits alone
  oldest.out         the same plant one byte further back: outside the window, a literal
  hit16.two          two 16-byte hits, 18 bytes at the lower index and 20 at the higher: the extended match moves up to the longer
  hit16.two.rev      the longer at the lower index
  wrap.t<t>          t = 2..16: the candidate t bytes in front of the query agrees up to the newest window byte and goes on with the
                     OLDEST window bytes (one to three more; the total is what the token says)
  wrap.t<t>.short    its neighbour: the last of the t bytes differs, the prefix t - 1 is exact where it stands (t = 2: a literal)
  wrap.t2.s3         t = 2, a pattern "ABA?": in the buffer the candidate's third byte agrees and its fourth does not (low bits)
  wrap.t2.deep       t = 2, a pattern of period 2: in the buffer the candidate is a 16-byte hit
  wrap.t3.deep       t = 3, period 3
  tie.low            6 bytes at window indices 496 and 796: the lower wins
  tie.index0         6 bytes at window indices 0 and 700
  tie.clip           6 bytes from index 1,020 on, clipped to 4 by the window's end, and 4 bytes at index 500: the lower wins
  clip.alone         the clipped one alone
  clip.longer        ... beside 3 bytes at index 500: the clipped 4 win
Every cell comes twice: with 24 literals behind the pattern ("full": 16 bytes and more of look-ahead at the query), and cut
LEFT = 9 bytes behind the query ("end": the stream's last 15 bytes; every length is capped at 9 and ties are decided again).
"""
import functools
from collections import namedtuple

import lazy_input as li

Cell = namedtuple("Cell", "name cell group variant data at expect")  # expect: {"ext": (kind, length, index), "v1": ...}

W = 1024
P = 1096          # the query: window_pos 72
OLDEST = P - W    # input position of the oldest window byte at the query
TAIL = 24
LEFT = 9          # bytes from the query to the end of an "end" stream
MAXP = 15         # min_pattern + 13
PAT = b"ABCDEFGHIJKLMNOPQRST"
END_MARKS = b"#%&*"  # bytes that end a plant: in no pattern, not in the lead, not in the initial dictionary


def _match(length, index, grown=None):
    """What both formats say for a first match of ``length`` (capped at MAXP) at ``index``: the extended format turns a match of
    more than min_pattern + 11 = 13 bytes into an extended match, which goes on to ``grown`` = (length, index) where given."""
    n = min(length, MAXP)
    ext = ("M", n, index) if n <= 13 else ("X",) + (grown or (length, index))
    return {"ext": ext, "v1": ("M", n, index)}


LITERAL = {"ext": ("L", 1, None), "v1": ("L", 1, None)}


def _designs():
    """[(cell, group, plants [(back, bytes)], pattern, expect full, expect end)]"""
    out = []

    def add(cell, group, plants, pattern, full, end):
        out.append((cell, group, plants, pattern, full, end))

    def idx(back):
        return (P - back) % W

    for k in range(2, 17):
        plant = PAT[:k] + b"#" if k < 16 else PAT[:20] + b"#"
        add(f"prefix.k{k}", "prefix", [(500, plant)], PAT + b"$", _match(k, idx(500), (20, idx(500)) if k == 16 else None), _match(min(k, LEFT), idx(500)))
    for bit, byte in ((6, PAT[3] ^ 0x40), (7, PAT[3] ^ 0x80)):
        add(f"k3.bit{bit}", "prefix", [(500, PAT[:3] + bytes([byte]))], PAT + b"$", _match(3, idx(500)), _match(3, idx(500)))

    add("oldest.k5", "oldest", [(W, PAT[:5] + b"#")], PAT + b"$", _match(5, idx(W)), _match(5, idx(W)))
    add("oldest.k2", "oldest", [(W, PAT[:2] + b"#")], PAT + b"$", _match(2, idx(W)), _match(2, idx(W)))
    add("oldest.out", "oldest", [(W + 1, PAT[:5] + b"#")], PAT + b"$", LITERAL, LITERAL)

    add("hit16.two", "hit16", [(700, PAT[:18] + b"#"), (400, PAT[:20] + b"%")], PAT + b"$",
        _match(18, idx(700), (20, idx(400))), _match(LEFT, idx(700)))
    add("hit16.two.rev", "hit16", [(700, PAT[:20] + b"#"), (400, PAT[:18] + b"%")], PAT + b"$",
        _match(20, idx(700), (20, idx(700))), _match(LEFT, idx(700)))

    for t in range(2, 17):
        more = 3 if t <= 10 else 1  # bytes of the pattern at the oldest window bytes: the total stays at 13 or below up to t = 12
        total = t + more
        add(f"wrap.t{t}", f"wrap.t{t}", [(t, PAT[:t]), (W, PAT[t:total] + b"#")], PAT + b"$", _match(total, idx(t)), _match(min(total, LEFT), idx(t)))
        short = LITERAL if t == 2 else _match(t - 1, idx(t))
        short_end = LITERAL if t == 2 else _match(min(t - 1, LEFT), idx(t))
        add(f"wrap.t{t}.short", f"wrap.t{t}", [(t, PAT[:t - 1] + b"#"), (W, PAT[t:total] + b"%")], PAT + b"$", short, short_end)
    add("wrap.t2.s3", "wrap.t2", [(2, b"AB"), (W, b"AZ#")], b"ABAZQRSTUVWXYZKL$", _match(4, idx(2)), _match(4, idx(2)))
    # (one more byte at the oldest window byte: two would be a match for the lead's own "AB" / "ABC", and the parse would not land on the query)
    add("wrap.t2.deep", "wrap.t2", [(2, b"AB"), (W, b"A#")], b"AB" * 10 + b"$", _match(3, idx(2)), _match(3, idx(2)))
    add("wrap.t3.deep", "wrap.t3", [(3, b"ABC"), (W, b"A#")], b"ABC" * 7 + b"$", _match(4, idx(3)), _match(4, idx(3)))

    add("tie.low", "tie", [(600, PAT[:6] + b"#"), (300, PAT[:6] + b"%")], PAT + b"$", _match(6, idx(600)), _match(6, idx(600)))
    add("tie.index0", "tie", [(P - 700, PAT[:6] + b"#"), (P - W, PAT[:6] + b"%")], PAT + b"$", _match(6, 0), _match(6, 0))
    add("tie.clip", "clip", [(P - 500, PAT[:4] + b"#"), (P - 1020, PAT[:6] + b"%")], PAT + b"$", _match(4, 500), _match(4, 500))
    add("clip.alone", "clip", [(P - 1020, PAT[:6] + b"%")], PAT + b"$", _match(4, 1020), _match(4, 1020))
    add("clip.longer", "clip", [(P - 500, PAT[:3] + b"#"), (P - 1020, PAT[:6] + b"%")], PAT + b"$", _match(4, 1020), _match(4, 1020))
    return out


@functools.lru_cache(maxsize=None)
def cells():
    fil = li.pair_filler(li.LEAD_ALPHABET_8)
    assert P + TAIL <= len(fil)
    out = []
    for cell, group, plants, pattern, full, end in _designs():
        lead = bytearray(fil[:P])
        lead[P - 1] = 0xFE  # a byte of its own in front of the pattern: no plant's predecessor repeats it, no match starts there
        for back, phrase in plants:
            s = P - back
            assert OLDEST - 1 <= s and s + len(phrase) <= P, (cell, back)
            lead[s:s + len(phrase)] = phrase
        assert len(pattern) > 16
        whole = bytes(lead) + pattern + fil[P:P + TAIL]
        out.append(Cell(f"{cell}-full", cell, group, "full", whole, P, full))
        out.append(Cell(f"{cell}-end", cell, group, "end", whole[:P + LEFT], P, end))
    assert all(len(c.data) < 3072 for c in out)
    return tuple(out)


RESIDUES = (0, 1, 2, 3)


def layout(streams, fill=0xA5):
    """-> (flat uint8, in_off uint64, in_len uint32, which): every stream four times, copy r at a batch offset in_off = r (mod 4),
    `fill` bytes in the gaps; which[i] = (index into `streams`, r)."""
    import numpy as np

    chunks, offs, lens, which, pos = [], [], [], [], 0
    for k, data in enumerate(streams):
        for r in RESIDUES:
            pad = 1 + (r - (pos + 1)) % 4
            chunks.append(bytes([fill]) * pad)
            pos += pad
            assert pos % 4 == r
            offs.append(pos)
            lens.append(len(data))
            which.append((k, r))
            chunks.append(data)
            pos += len(data)
    chunks.append(bytes([fill]) * 8)
    flat = np.frombuffer(b"".join(chunks), dtype=np.uint8)
    return flat, np.asarray(offs, dtype=np.uint64), np.asarray(lens, dtype=np.uint32), which
