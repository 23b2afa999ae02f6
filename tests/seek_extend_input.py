"""Extending a seek index: the rule, stated in Python, and the oracle's rows of cut streams (no GPU import: shared by
tests/test_seek_extend_host.py and tests/test_gpu_seek_extend.py).

A stream has GROWN when its old bytes are a prefix of its new ones.  ``restart_rows`` is the rule of include/tamp_amd.h
(tamp_batch_seek_index_extend) on a stream's old in_pos column; every expectation about rows comes from
``seek_index_input.expected_checkpoints`` on the oracle, of the cut stream for the old rows and of the whole stream for the result.
"""
from __future__ import annotations

import functools

import numpy as np

import seek_index_input as si


def restart_rows(in_pos) -> int:
    """How many of a stream's rows are final: the restart row -- the last one whose in_pos is smaller than the last row's -- and
    those in front of it.  0: none, the stream restarts from its header."""
    in_pos = [int(x) for x in in_pos]
    for r in range(len(in_pos) - 2, -1, -1):
        if in_pos[r] < in_pos[-1]:
            return r + 1
    return 0


def slim(rows, window_bits: int):
    """expected_checkpoints' rows with the window cut to the stream's own size (it returns 32 KiB for every stream)."""
    W = 1 << window_bits
    return [{"in_pos": r["in_pos"], "state": r["state"], "window": r["window"][:W].copy()} for r in rows]


def row_bytes(row) -> bytes:
    """The 16 state bytes of an oracle row, as a table holds them."""
    d = si.Dec()
    for f in si.FIELDS:
        setattr(d, f, row["state"][f])
    return bytes(d)


def place_rows(rows, in_pos, state, at: int) -> None:
    """Oracle rows into the two tables from row ``at`` on."""
    for k, row in enumerate(rows):
        in_pos[at + k] = row["in_pos"]
        state[at + k, :16] = np.frombuffer(row_bytes(row), dtype=np.uint8)
        W = len(row["window"])
        state[at + k, 16 : 16 + W] = row["window"]


def same_row(a, b) -> bool:
    """Two oracle rows, compared the way assert_rows compares a GPU row with one: the buffer's valid bits only, the pending pair
    only where a token is in delivery."""
    sa, sb = a["state"], b["state"]
    if a["in_pos"] != b["in_pos"] or a["window"].tobytes() != b["window"].tobytes():
        return False
    for f in ("window_pos", "token_state", "skip_bytes", "bit_buffer_pos", "conf", "flags", "window_bits_max"):
        if sa[f] != sb[f]:
            return False
    nb = sa["bit_buffer_pos"]
    if nb and (sa["bit_buffer"] >> (32 - nb)) != (sb["bit_buffer"] >> (32 - nb)):
        return False
    if sa["token_state"] or sa["skip_bytes"]:
        return (sa["pending_window_offset"], sa["pending_match_size"]) == (sb["pending_window_offset"], sb["pending_match_size"])
    return True


@functools.lru_cache(maxsize=None)
def whole_rows(oracle, window: int, extended: bool, N: int):
    """-> (src, stream, rows of the whole cut-sweep stream at interval N)."""
    src, stream = si.cut_sweep_stream(oracle, window, extended)
    rows, S, _, _ = si.expected_checkpoints(oracle, stream, N, window_bits=window)
    assert S == len(src)
    return src, stream, slim(rows, window)


@functools.lru_cache(maxsize=None)
def cut_rows(oracle, window: int, extended: bool, N: int, step: int = 1):
    """-> {c: rows of stream[:c]} for c = step, 2 * step, .. up to len(stream) (the last one included whatever the step)."""
    _, stream, _ = whole_rows(oracle, window, extended, N)
    cuts = sorted(set(range(step, len(stream) + 1, step)) | {len(stream)})
    return {c: slim(si.expected_checkpoints(oracle, stream[:c], N, window_bits=window)[0], window) for c in cuts}
