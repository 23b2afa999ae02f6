"""CPU tier: the inputs of tests/test_gpu_query_setup.py aim where they say they aim (tests/query_setup_input.py), read from the
oracle's own token trace (tests/long_stream_writer.py's reader), the way tests/test_run_list_input.py does for its families.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import long_stream_writer as lsw  # noqa: E402
import query_setup_input as qsi  # noqa: E402


def tokens(oracle, data, extended):
    """[(input position, token)] of the stream the oracle writes for `data` at window 10, literal 8."""
    from tamp_amd.batch import pack_streams

    flat, off, ln = pack_streams([data])
    r = oracle.compress_batch(flat, off, ln, window=10, literal=8, extended=extended, threads=1)
    assert (np.asarray(r.status) == 0).all()
    out, pos = [], 0
    for tk in lsw.read_tokens(r.stream(0))[0]:
        out.append((pos, tk))
        pos += tk.produced
    assert pos == len(data)
    return out


def test_shapes():
    assert set(n % 4 for n in qsi.LENGTHS if n < 10) == {0, 1, 2, 3} and min(qsi.LENGTHS) < 4
    for edge in (1024, 2048, 4096):  # tail quads of 1, 2, 3 positions and a full one at every epoch boundary
        assert {1, 2, 3, 0} <= set(n % 4 for n in qsi.LENGTHS if edge - 6 <= n <= edge + 7)
    assert 1025 in qsi.LENGTHS and 2049 in qsi.LENGTHS  # an epoch of a single position
    its = qsi.items()
    flat, off, ln = qsi.layout(its)
    for (t, n, r), o, k in zip(its, off, ln):
        assert int(o) % 4 == r and int(k) == n and flat[int(o):int(o) + n].tobytes() == qsi.text(t)[:n]
        assert flat[int(o) - 1] == 0xA5 and flat[int(o) + n] == 0xA5  # filler on both sides of every stream


def test_the_run_text_has_the_stated_runs():
    data = qsi.text("runs")
    lengths = set()
    for k, p in enumerate(range(0, qsi.L - qsi.RUN_MAX, qsi.RUN_PERIOD)):
        r = qsi.RUN_MIN + (k * 7) % (qsi.RUN_MAX - qsi.RUN_MIN + 1)
        seen = min(r, qsi.RUN_PERIOD)  # (a longer run ends where the next one starts)
        assert data[p:p + seen] == data[p:p + 1] * seen and data[p + qsi.RUN_PERIOD] != data[p], (k, p, r)
        lengths.add(r)
    assert lengths == set(range(qsi.RUN_MIN, qsi.RUN_MAX + 1))


def test_the_run_text_gives_rle_tokens_and_lags(oracle):
    toks = tokens(oracle, qsi.text("runs"), True)
    lags = [(pos, tk) for pos, tk in toks if tk.kind == "R" and tk.produced > tk.written]
    # RLE tokens that write fewer bytes than they consume, in every epoch of 1,024 positions ...
    # (an epoch holds 27 runs, 13 of them of a byte without an earlier run in the window: at least 8 of those give a lag; the
    # others are mostly taken by matches against an earlier run of the same byte)
    assert all(sum(pos // 1024 == e for pos, _ in lags) >= 8 for e in range(4)), [pos for pos, _ in lags]
    # ... and the walk comes out of them at every residue mod 4 (where the next epoch's buffer starts)
    assert {(pos + tk.produced) % 4 for pos, tk in lags} == {0, 1, 2, 3}
    # extended matches too (the settled-token pass weighs both kinds)
    assert sum(tk.kind == "X" for _, tk in toks) >= 4
    # the v1 format has no RLE token: the same text is matches and literals there
    assert {tk.kind for _, tk in tokens(oracle, qsi.text("runs"), False)} <= {"L", "M", "F"}


@pytest.mark.parametrize("extended", [True, False])
def test_the_period_2_text_matches_from_the_first_epoch_on(oracle, extended):
    toks = tokens(oracle, qsi.text("period2"), extended)
    assert [tk.kind for _, tk in toks[:2]] == ["L", "L"]
    pos, third = toks[2]
    assert pos == 2 and third.kind in "MX"
    # nothing but matches behind the first two bytes, in every epoch
    assert all(tk.kind in "MXF" for _, tk in toks[2:])
    assert {p // 1024 for p, tk in toks[2:] if tk.kind in "MX"} == {0, 1, 2, 3}
