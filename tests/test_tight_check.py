"""CPU tier: the whole-buffer comparison of tests/tight_check.py on synthetic buffers -- the proof that the GPU tests which rely on
it (tests/test_gpu_tight_output.py, tests/test_gpu_tight_decode.py) can fail.  No kernel is broken for it: a correct result is
built by hand and one thing at a time is changed in it."""
import numpy as np
import pytest

from tight_check import LEAD, check_call, slab_layout

N = 37
FULL = bytes((7 * i + 3) & 0xFF for i in range(N))  # a stream's bytes with ample room


def correct(gap):
    """A sweep of capacities 0 .. N + 2 as a correct decoder leaves it -> (got, caps, status, out_len, streams, consumed)"""
    caps = np.arange(N + 3, dtype=np.uint32)
    out_off, out = slab_layout(caps, gap)
    streams = [FULL[: min(int(c), N)] for c in caps]
    for o, s in zip(out_off, streams):
        out[int(o) : int(o) + len(s)] = np.frombuffer(s, dtype=np.uint8)
    status = np.where(caps < N, 1, 2).astype(np.int64)
    out_len = np.minimum(caps, N).astype(np.int64)
    consumed = (out_len // 2 + 1).astype(np.int64)
    return (status.copy(), out_len.copy(), out, out_off), caps, status, out_len, streams, consumed


def check(got, caps, status, out_len, streams, consumed, got_consumed=None, **kw):
    check_call(got, caps, status, out_len, streams, "synthetic", consumed=(consumed if got_consumed is None else got_consumed, consumed), **kw)


@pytest.mark.parametrize("gap", [0, 5])
def test_the_untouched_buffer_passes(gap):
    check(*correct(gap))
    check(*correct(gap), behind_len_unspecified=True)


@pytest.mark.parametrize("gap", [0, 5])
def test_one_byte_behind_a_slabs_end_raises(gap):
    got, caps, *rest = correct(gap)
    j = N + 1  # (cap N + 1, N bytes produced: its last byte is its own, the one behind belongs to the next slab or the gap)
    got[2][int(got[3][j]) + int(caps[j])] ^= 0x10
    for relaxed in (False, True):  # (the relaxed form leaves only a slab's OWN bytes behind out_len open)
        with pytest.raises(AssertionError, match="written outside|bytes"):
            check(got, caps, *rest, behind_len_unspecified=relaxed)


def test_one_byte_behind_the_last_slab_raises():
    got, caps, *rest = correct(0)
    got[2][int(got[3][-1]) + int(caps[-1])] ^= 1
    with pytest.raises(AssertionError, match="written outside"):
        check(got, caps, *rest, behind_len_unspecified=True)


def test_one_byte_in_the_guard_in_front_of_the_first_slab_raises():
    for at in range(LEAD):
        got, *rest = correct(0)
        got[2][at] ^= 0x80
        with pytest.raises(AssertionError, match="written outside"):
            check(got, *rest, behind_len_unspecified=True)


def test_one_byte_behind_out_len_inside_a_slab_raises_unless_the_call_leaves_it_open():
    got, caps, *rest = correct(0)
    j = N + 2  # cap N + 2, N bytes produced: two bytes of its own behind out_len
    got[2][int(got[3][j]) + N] ^= 4
    with pytest.raises(AssertionError, match="written outside"):
        check(got, caps, *rest)
    check(got, caps, *rest, behind_len_unspecified=True)


def test_one_wrong_produced_byte_raises():
    got, *rest = correct(5)
    got[2][int(got[3][20]) + 19] ^= 1
    with pytest.raises(AssertionError, match="bytes"):
        check(got, *rest)


def test_one_wrong_status_raises():
    got, *rest = correct(0)
    got[0][N] = 1
    with pytest.raises(AssertionError, match="status"):
        check(got, *rest)


def test_one_wrong_length_raises():
    got, *rest = correct(0)
    got[1][5] = 4
    with pytest.raises(AssertionError, match="out_len"):
        check(got, *rest)


def test_one_wrong_consumed_count_raises():
    got, caps, status, out_len, streams, consumed = correct(0)
    wrong = consumed.copy()
    wrong[9] += 1
    with pytest.raises(AssertionError, match="consumed"):
        check(got, caps, status, out_len, streams, consumed, got_consumed=wrong)
