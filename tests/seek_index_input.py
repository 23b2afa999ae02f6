"""The seek index's expected checkpoints and the ragged batch of its GPU test (no GPU import: shared by
tests/test_seek_index_host.py and tests/test_gpu_seek_index.py).

A checkpoint is defined by the reference's decoder object (include/tamp_amd.h, tamp_batch_seek_index): checkpoint k is the object,
initialised without a configuration, after k calls that were each offered all input not yet consumed and exactly N bytes of room.
``expected_checkpoints`` drives ``oracle_decoder_init`` / ``oracle_decoder_call`` through ctypes exactly so.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import cut_sweep_input as cs

OK, OUTPUT_FULL, INPUT_EXHAUSTED, OOB, INVALID_CONF, BAD_INDEX = 0, 1, 2, -4, -3, -22


class Dec(C.Structure):  # TampAmdDecoderState (include/tamp_amd.h) = OracleDecoder (oracle/tamp_oracle.h): 16 bytes
    _fields_ = [("bit_buffer", C.c_uint32), ("window_pos", C.c_uint16), ("bit_buffer_pos", C.c_uint8),
                ("token_state", C.c_uint8), ("pending_window_offset", C.c_uint16),
                ("pending_match_size", C.c_uint16), ("conf", C.c_uint8), ("skip_bytes", C.c_uint8),
                ("flags", C.c_uint8), ("window_bits_max", C.c_uint8)]


FIELDS = tuple(name for name, _ in Dec._fields_)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _protos(L):
    L.oracle_decoder_init.restype = C.c_int
    L.oracle_decoder_init.argtypes = [C.POINTER(Dec), C.c_void_p, C.c_void_p, C.c_uint8]
    L.oracle_decoder_call.restype = C.c_int
    L.oracle_decoder_call.argtypes = [C.POINTER(Dec), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]


def _fresh(oracle, window_bits, dictionary):
    _protos(oracle.lib)
    d = Dec()
    win = np.zeros(1 << 15, dtype=np.uint8)
    if dictionary is not None:
        dd = np.frombuffer(bytes(dictionary), dtype=np.uint8)[: 1 << 15]
        win[: len(dd)] = dd
    r0 = oracle.lib.oracle_decoder_init(C.byref(d), _p(win), None, window_bits)
    assert r0 == OK
    return d, win


def _call(oracle, d, win, data, cap):
    out = np.zeros(cap + 1, dtype=np.uint8)
    w, k = C.c_size_t(0), C.c_size_t(0)
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    r = oracle.lib.oracle_decoder_call(C.byref(d), _p(win), _p(a) if len(a) else None, len(a), _p(out), cap, C.byref(w), C.byref(k))
    return r, out[: w.value].tobytes(), k.value


def state_dict(d: Dec) -> dict:
    return {f: int(getattr(d, f)) for f in FIELDS}


def expected_checkpoints(oracle, stream: bytes, N: int, *, window_bits: int = 15, dictionary=None):
    """-> (rows, S, statuses, final): rows[k - 1] = {"in_pos", "state" (dict of the 16 bytes' fields), "window" (1 << 15 bytes)}
    for every k >= 1 with k * N < S; S = the bytes the stream decodes to; statuses = what each of those calls returned (all
    OUTPUT_FULL by the definition); final = the status of the call that ended the stream."""
    d, win = _fresh(oracle, window_bits, dictionary)
    pos, S, rows, statuses = 0, 0, [], []
    while True:
        r, got, used = _call(oracle, d, win, stream[pos:], N)
        pos += used
        S += len(got)
        if r != OUTPUT_FULL:
            final = r
            break
        assert len(got) == N
        rows.append({"in_pos": pos, "state": state_dict(d), "window": win.copy()})
        statuses.append(r)
    keep = (S - 1) // N if S else 0  # (a row at k * N == S is no checkpoint: no byte behind it)
    assert keep <= len(rows) <= keep + 1
    return rows[:keep], S, statuses[:keep], final


def restart(oracle, stream: bytes, row_state: dict, window: bytes, in_pos: int, cap: int):
    """The oracle's object set to a checkpoint and run to the end of the stream -> (status, bytes)."""
    _protos(oracle.lib)
    d = Dec()
    for f in FIELDS:
        setattr(d, f, row_state[f])
    win = np.zeros(1 << 15, dtype=np.uint8)
    w = np.frombuffer(bytes(window), dtype=np.uint8)
    win[: len(w)] = w
    r, got, _ = _call(oracle, d, win, stream[in_pos:], cap)
    return r, got


def checkpoint_class(state: dict) -> str:
    if state["token_state"] == 1:
        return "rle"
    if state["token_state"] == 3:
        return "ext"
    return "match" if state["skip_bytes"] else "boundary"


@functools.lru_cache(maxsize=None)
def cut_sweep_stream(oracle, window: int, extended: bool):
    src = cs.source(window)
    rc, stream = oracle.compress(src, window=window, literal=cs.LITERAL, extended=extended)
    assert rc == OK
    return src, stream


def ragged_batch(oracle):
    """The GPU test's batch at N = 100 -> [(name, stream, dictionary or None)]: sizes around the interval, streams that end
    early or badly, three windows, both formats, a custom dictionary, flushes and a dictionary reset."""
    from tamp_amd import workloads as wl

    prose = wl.real_text("prose", frozen_only=True)[20_000:24_000]
    comp = lambda data, **kw: oracle.compress(data, **{"window": 10, "literal": 8, "extended": True, **kw})[1]  # noqa: E731
    batch = []
    for n in (0, 1, 99, 100, 101, 200, 201):
        batch.append((f"len{n}", comp(prose[:n]), None))
    batch.append(("header-only", comp(prose[:300])[:1], None))
    batch.append(("empty", b"", None))
    whole = comp(prose[:900])
    batch.append(("cut-in-token", whole[: len(whole) * 2 // 3], None))
    # a v1 stream at window 8 with three bytes behind its end that the oracle reads as a match out of the window (offset bits
    # all ones): the first such tail, found here and not written down, because it depends on how the stream's last byte is padded
    head = oracle.compress(prose[:150], window=8, extended=False)[1]
    tails = (head + bytes([b, 0xFF, 0xFF]) for b in range(256))
    oob = next(s for s in tails if oracle.decompress(s)[0] == OOB and len(oracle.decompress(s)[1]) >= 150)
    batch.append(("oob", oob, None))
    batch.append(("w8-v1", comp(prose[:700], window=8, extended=False), None))
    batch.append(("w8-ext", comp(prose[100:650], window=8), None))
    batch.append(("w12-v1", comp(prose[:2500], window=12, extended=False), None))
    batch.append(("w12-ext", comp(prose[500:3100] + b"z" * 400, window=12), None))
    dictionary = (prose[3000:4000] * 2)[:1024]
    batch.append(("custom", comp(prose[3200:3900], dictionary=dictionary), dictionary))
    rc, scripted = oracle.stream_script([("write", prose[:250]), ("flush", True), ("write", prose[250:420]), ("reset",),
                                         ("write", prose[100:460]), ("flush", True), ("write", prose[:90]), ("close",)],
                                        window=10, dictionary_reset=True)
    assert rc == OK
    batch.append(("scripted", scripted, None))
    return batch
