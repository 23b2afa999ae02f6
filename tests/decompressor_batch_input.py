"""Streams for the DecompressorBatch tests (tests/test_gpu_decompressor_batch.py; no GPU import).

Each stream decodes to 100-400 bytes and compresses to more than 64, so that a batch with one object per cut of it keeps
lanes and wavefronts past the first busy.  Made with the oracle (``Oracle.compress`` / ``Oracle.stream_script``) or by hand.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np


@dataclass(frozen=True)
class Stream:
    name: str
    comp: bytes                 # the `.tamp` stream
    window_bits: int            # capacity of the objects that decode it
    plain: Optional[bytes]      # what it decodes to; None: the stream is in error
    dictionary: Optional[bytes] = None


@functools.lru_cache(maxsize=None)
def prose() -> bytes:
    from tamp_amd import workloads as wl

    text = wl.real_text("prose", frozen_only=True)[50_000:52_000]
    assert len(text) == 2_000, "tests/golden/corpus_prose.txt.xz missing"
    return text


def text() -> bytes:
    """About 300 bytes with plain matches (short repeats) and extended matches (repeats of 40 and 60 bytes)."""
    p = prose()
    return p[:130] + p[20:80] + p[130:190] + p[100:140] + p[190:220]


def run_text() -> bytes:
    """A run of 300 equal bytes inside text: two RLE tokens, of which only 8 bytes each enter the window (the lag case)."""
    p = prose()
    return p[300:340] + b"z" * 300 + p[340:390]


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value: int, n: int):
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def bytes(self) -> bytes:
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(bit << (7 - i) for i, bit in enumerate(b[k : k + 8])) for k in range(0, len(b), 8))


def oob_stream() -> bytes:
    """Window 2^8, literal 8, v1 format: 100 literals, then a match of the shortest length (code word 0) at offset 255 -- offset +
    length leaves the window (TAMP_OOB, -4) -- and literals behind it that are never reached."""
    w = BitWriter().put(0x18, 8)  # header: window 8, literal 8, nothing else
    p = prose()
    for c in p[:100]:
        w.put(1, 1).put(c, 8)
    w.put(0, 1).put(0, 1).put(255, 8)
    for c in p[100:110]:
        w.put(1, 1).put(c, 8)
    return w.bytes()


def streams(oracle):
    """Every stream of the issue's list, in a fixed order."""
    def comp(data, **kw):
        rc, out = oracle.compress(data, **kw)
        assert rc == 0
        return out

    out = []
    t = text()
    for w in (8, 10, 15):
        out.append(Stream(f"text-w{w}", comp(t, window=w), w, t))
    out.append(Stream("run300-w10", comp(run_text(), window=10), 10, run_text()))
    p = prose()
    parts = (p[400:520], p[430:500] + p[520:560], p[560:680])
    rc, two_resets = oracle.stream_script([("write", parts[0]), ("reset",), ("write", parts[1]), ("reset",), ("write", parts[2]),
                                           ("close",)], window=10, dictionary_reset=True)
    assert rc == 0
    out.append(Stream("two-resets-w10", two_resets, 10, b"".join(parts)))
    dictionary = (p[700:1000] * 4)[:1024]
    custom = p[720:780] + p[1000:1180] + p[820:860]
    out.append(Stream("custom-dictionary-w10", comp(custom, window=10, dictionary=dictionary), 10, custom, dictionary))
    seven = bytes(c & 0x7F for c in t)
    out.append(Stream("literal7-w10", comp(seven, window=10, literal=7), 10, seven))
    out.append(Stream("v1-w10", comp(t, window=10, extended=False), 10, t))
    plain10 = out[1].comp
    out.append(Stream("two-byte-header-w10", bytes([plain10[0] | 1, 0]) + plain10[1:], 10, t))
    out.append(Stream("oob-w8", oob_stream(), 8, None))
    out.append(Stream("header-above-window-bits", plain10, 9, None))
    return out


def expected_calls(oracle, s: Stream, pieces_and_caps):
    """The oracle's calls for ONE object of stream ``s`` that is offered, call by call, the unconsumed rest of its stream up to
    ``take`` bytes with ``cap`` bytes of room: [(take, cap), ...] -> [(status, bytes, consumed), ...]."""
    r0, calls = oracle.decode_script(s.comp, pieces_and_caps, window_bits=s.window_bits, dictionary=s.dictionary)
    assert r0 == 0
    return calls


AMPLE = 4096  # room no call of these streams can fill


def two_piece_calls(oracle, s: Stream, cut: int):
    """Stream ``s`` in two pieces, ``comp[:cut]`` and everything the first call left, each decoded into ``size + 1`` bytes of room
    (what ``read(out_cap=None)`` gives it): -> [(status, bytes, consumed)] * 2.  The sizes are the oracle's own, with ample room."""
    n = len(s.comp)
    first = expected_calls(oracle, s, [(cut, AMPLE)])[0]
    sized = expected_calls(oracle, s, [(cut, len(first[1]) + 1)])
    assert sized[0] == first  # (one spare byte is as good as ample room)
    rest = n - first[2]
    second = expected_calls(oracle, s, [(cut, len(first[1]) + 1), (rest, AMPLE)])[1]
    return expected_calls(oracle, s, [(cut, len(first[1]) + 1), (rest, len(second[1]) + 1)])


def c_tables(n):
    """Zeroed host arrays in the shapes of the two C calls' arguments, for calls that must return before they touch any of them
    (window 2^10 objects: 1,040 bytes each)."""
    k = max(n, 1)
    t = dict(states=np.zeros(k * 1040, np.uint8), index=np.zeros(k, np.uint32), data=np.zeros(16, np.uint8), in_off=np.zeros(k, np.uint64),
             in_len=np.zeros(k, np.uint32), out=np.zeros(16, np.uint8), out_off=np.zeros(k, np.uint64), out_cap=np.zeros(k, np.uint32),
             out_len=np.zeros(k, np.uint32), status=np.zeros(k, np.int8), consumed=np.zeros(k, np.uint32))
    return t


def decode_pieces(lib, t, n, stride=1040, bits=10, device=0, **null):
    p = {k: (None if null.get(k) else v.ctypes.data_as(C.c_void_p)) for k, v in t.items()}
    return lib.tamp_batch_decompress_pieces(p["states"], stride, bits, p["index"], p["data"], p["in_off"], p["in_len"], p["out"], p["out_off"],
                                            p["out_cap"], p["out_len"], p["status"], p["consumed"], n, device, None)


def size_pieces(lib, t, n, stride=1040, bits=10, device=0, **null):
    p = {k: (None if null.get(k) else v.ctypes.data_as(C.c_void_p)) for k, v in t.items()}
    return lib.tamp_batch_decoded_size_pieces(p["states"], stride, bits, p["index"], p["data"], p["in_off"], p["in_len"], p["out_cap"],
                                              p["out_len"], p["status"], p["consumed"], n, device, None)
