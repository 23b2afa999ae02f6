"""What the tight-output and tight-decode GPU tests share (tests/test_gpu_tight_output.py, tests/test_gpu_tight_decode.py), and
what tests/test_tight_check.py proves can fail: the patterned buffer, the slab layout and the WHOLE-buffer comparison.  A plain
helper: no fixtures, no GPU.
"""
import contextlib
import os

import numpy as np

LEAD, TAIL = 3, 64  # guard bytes in front of the first slab and behind the last


@contextlib.contextmanager
def env(name, value):
    """(set and restored the way tests/test_gpu_fixed_build.py does it)"""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def pattern(n):
    return ((np.arange(n, dtype=np.uint32) * 37 + 11) & 0xFF).astype(np.uint8)


def slab_layout(caps, gap=0):
    """Slabs of ``caps`` bytes ``gap`` bytes apart behind LEAD guard bytes, TAIL guard bytes behind the last.
    -> (out_off, a buffer of pattern())"""
    caps = np.asarray(caps, dtype=np.uint32)
    pitch = caps.astype(np.uint64) + np.uint64(gap)
    out_off = (np.uint64(LEAD) + np.cumsum(pitch) - pitch).astype(np.uint64)
    return out_off, pattern(LEAD + int(pitch.sum()) + TAIL)


def check_call(got, caps, want_status, want_len, want_streams, tag, behind_len_unspecified=False, consumed=None):
    """Per slab: status, length, bytes (``consumed`` = (the call's counts, the expected ones): those too).  Then the whole
    buffer: the expected prefixes in a buffer of pattern() -- guard bytes, gaps and the slab bytes behind out_len untouched
    (``behind_len_unspecified``: all but the latter -- a host-memory call whose slabs tile the buffer brings them back in one
    transfer, and the header leaves those bytes open)."""
    status, out_len, out, out_off = got
    bad = np.flatnonzero((status != want_status) | (out_len != want_len))
    assert bad.size == 0, (tag, "slab", int(bad[0]), "status", int(status[bad[0]]), int(want_status[bad[0]]),
                           "out_len", int(out_len[bad[0]]), int(want_len[bad[0]]))
    if consumed is not None:
        bad = np.flatnonzero(np.asarray(consumed[0]) != np.asarray(consumed[1]))
        assert bad.size == 0, (tag, "slab", int(bad[0]), "consumed", int(consumed[0][bad[0]]), int(consumed[1][bad[0]]))
    expected, care = pattern(out.size), np.ones(out.size, dtype=bool)
    for j, s in enumerate(want_streams):
        o = int(out_off[j])
        assert out[o : o + len(s)].tobytes() == s, (tag, "slab", j, "bytes")
        expected[o : o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        if behind_len_unspecified:
            care[o + len(s) : o + int(caps[j])] = False
    diff = np.flatnonzero((out != expected) & care)
    if diff.size:
        at = int(diff[0])
        j = int(np.searchsorted(out_off, at, side="right")) - 1
        raise AssertionError((tag, "byte", at, "written outside the produced bytes; slab", j, "starts at",
                              int(out_off[max(j, 0)]), "cap", int(caps[max(j, 0)])))
