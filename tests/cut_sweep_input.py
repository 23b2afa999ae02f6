"""The cut sweep's input and the classification of its cuts (no GPU import: shared by tests/golden/make_cut_sweep.py,
tests/test_cut_sweep_golden.py and tests/test_gpu_cut_sweep.py).

One stream of about 1.4 KB per window size, written in two (or three) calls cut at EVERY byte.  Between two flush points
the bytes of a stream do not depend on how its input was cut into calls (the reference polls only while its 16-byte ring
is full, compressor.c:700-720), so every cut has the same known answer -- the one-shot stream -- and the sweep is
exhaustive where the randomised piece tests hit a given cut by luck.

The input is the smallest on which the piece-specific code can still go wrong: it passes the end of the window buffer
(once at 2^10, five times at 2^8), holds a run longer than the longest RLE token (241), short runs, extended matches of
15..90 bytes and matches whose source ends at the end of the window buffer.  tests/test_cut_sweep_golden.py asserts
these properties from the oracle's token trace.
"""
from __future__ import annotations

import bisect
import ctypes as C
import functools

#: (window, extended); literal = 8 everywhere.  2^15 is the unpacked-index build of the compress kernel.
CONFIGS = ((10, True), (10, False), (8, True), (8, False), (15, True))
LITERAL = 8
CAP = 4096  # output room of every object call: ample (the whole stream is < 1.5 KB)
KINDS = ("literal", "match", "rle", "extended match")  # oracle/tamp_oracle.h:114

#: Window 2^10, extended format: input position behind the byte that lands on window index W - 1.  Runs put at most 8 of
#: their bytes into the window, so window_pos lags the input position and the repeat around position W makes a match that
#: ends at the window buffer's end in the v1 format only.  A repeat of the 24 bytes in front of THIS position makes one in
#: the extended format (found from the window indices of the token trace; tests/test_cut_sweep_golden.py checks both).
EXT_WINDOW_END_AT = {10: 1296}


def case_id(window: int, extended: bool) -> str:
    return f"w{window}-{'ext' if extended else 'v1'}"


@functools.lru_cache(maxsize=None)
def source(window: int) -> bytes:
    from tamp_amd import workloads as wl

    W = 1 << window
    prose = wl.real_text("prose", frozen_only=True)[50_000:60_000]
    assert len(prose) == 10_000, "tests/golden/corpus_prose.txt.xz missing"
    b = bytearray()
    b += prose[:200]
    b += b"x" * 260                     # a run longer than the longest RLE token (241): two tokens
    b += prose[200:300]
    b += prose[20:110]                  # extended match of 90 bytes
    b += b"aa" + prose[300:306] + b"bbb" + prose[306:312] + b"c" * 9 + prose[312:318] + b"d" * 17 + prose[318:324]
    b += prose[324:500]
    b += b"ab" * 40                     # period 2: a match that overlaps its own output
    b += prose[500:620]
    b += prose[510:600]
    b += bytes(30)
    b += prose[620:700]
    k = len(b) // W                     # the 40 bytes around the last multiple of W: a match cut by the window's end
    b += b[k * W - 24 : k * W + 16] if k else b[len(b) // 2 - 24 : len(b) // 2 + 16]
    b += prose[700:740]
    at = EXT_WINDOW_END_AT.get(window)
    if at is not None:                  # the same for the extended format's (lagging) window position
        b += b[at - 24 : at]
        b += prose[740:780]
    return bytes(b)


_TOKEN_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_size_t, C.c_uint, C.c_uint)


def token_trace(oracle, src: bytes, window: int, extended: bool):
    """Tokens of the one-shot stream as the oracle emits them: [(kind, input position, length, window index)] in input
    order (oracle_set_token_cb, oracle/tamp_oracle.h:114-116), and the stream itself."""
    toks = []
    cb = _TOKEN_CB(lambda user, kind, pos, length, index: toks.append((int(kind), int(pos), int(length), int(index))))
    oracle.lib.oracle_set_token_cb.argtypes = [_TOKEN_CB, C.c_void_p]
    oracle.lib.oracle_set_token_cb.restype = None
    oracle.lib.oracle_set_token_cb(cb, None)
    try:
        rc, whole = oracle.compress(src, window=window, literal=LITERAL, extended=extended)
    finally:
        oracle.lib.oracle_set_token_cb(C.cast(None, _TOKEN_CB), None)
    assert rc == 0
    toks.sort(key=lambda t: t[1])
    pos = 0
    for _, start, length, _ in toks:  # the tokens tile the input
        assert start == pos and length >= 1, (start, pos, length)
        pos += length
    assert pos == len(src)
    return toks, whole


def token_at(tokens, c: int):
    """The token a cut at ``c`` (calls src[:c] and src[c:]) falls into or in front of; None at the end of the input."""
    k = bisect.bisect_right([t[1] for t in tokens], c) - 1
    if k < 0 or c >= tokens[k][1] + tokens[k][2]:
        return None
    return tokens[k]


def inside(token, c: int) -> bool:
    """A cut is inside a token when it lies strictly between the token's first and last byte."""
    return token is not None and token[1] < c < token[1] + token[2]


def describe_cut(tokens, c: int) -> str:
    """'cut 7 bytes into the rle token of 241 (input 201, window index 0)' -- for assertion messages."""
    t = token_at(tokens, c)
    if t is None:
        return f"cut {c}: behind the last token"
    kind, start, length, index = t
    where = f"{c - start} bytes into" if c > start else "in front of"
    return f"cut {c}: {where} the {KINDS[kind]} token of {length} (input {start}, window index {index})"


def coverage(tokens, n: int, window: int) -> dict:
    """Counts of cuts 0..n by the kind of token they are inside, and the tokens that the window buffer's end cut short."""
    W = 1 << window
    out = dict(rle=0, rle_near=0, ext=0, ext_near=0, match=0, rle_lengths=[t[2] for t in tokens if t[0] == 2],
               ext_lengths=[t[2] for t in tokens if t[0] == 3],
               window_end=[t for t in tokens if t[0] in (1, 3) and t[3] + t[2] == W])
    for c in range(n + 1):
        t = token_at(tokens, c)
        if not inside(t, c):
            continue
        key = {1: "match", 2: "rle", 3: "ext"}[t[0]]
        out[key] += 1
        if key != "match" and c - t[1] < 16:
            out[key + "_near"] += 1
    return out
