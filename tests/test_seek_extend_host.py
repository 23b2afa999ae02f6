"""CPU tier: what a correct extension of a seek index is, pinned on the oracle's decoder object, and the surface of
tamp_batch_seek_index_extend / ``extend_seek_index`` without a device.  The GPU side: tests/test_gpu_seek_extend.py.

The rule (include/tamp_amd.h): a grown stream restarts at the last of its rows whose in_pos is smaller than its last row's; rows up
to that one are final, the others are decoded again.  Here the oracle's rows of every prefix of the cut-sweep streams are compared
with its rows of the whole streams."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cut_sweep_input as cs  # noqa: E402
import seek_extend_input as se  # noqa: E402
import seek_index_input as si  # noqa: E402


@pytest.mark.parametrize("N", (64, 241))
@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=[cs.case_id(*c) for c in cs.CONFIGS])
def test_the_rule_on_the_oracle(oracle, window, extended, N):
    """Every cut of the stream: the rows in front of the old end are the whole stream's, and rows AT the old end are not all --
    continuing from the last row would be wrong."""
    _, stream, whole = se.whole_rows(oracle, window, extended, N)
    differ_at_end = dropped_more_than_one = 0
    for c in range(1, len(stream) + 1):
        rows = se.slim(si.expected_checkpoints(oracle, stream[:c], N, window_bits=window)[0], window)
        assert len(rows) <= len(whole), c
        if not rows:
            continue
        last = rows[-1]["in_pos"]
        assert last <= c
        for k, row in enumerate(rows):
            if row["in_pos"] < last:
                assert se.same_row(row, whole[k]), (c, k)
            else:
                assert row["in_pos"] == c or se.same_row(row, whole[k]), (c, k)  # (only a row AT the old end may differ)
                differ_at_end += not se.same_row(row, whole[k])
        final = se.restart_rows([r["in_pos"] for r in rows])
        assert all(r["in_pos"] < last for r in rows[:final]) and all(r["in_pos"] == last for r in rows[final:]), c
        dropped_more_than_one += len(rows) - final > 1
    assert differ_at_end >= 1
    if (window, extended, N) == (10, True, 64):  # the figures of the issue that asked for the extension
        assert differ_at_end == 31 and dropped_more_than_one == 37


def test_restart_rows():
    assert se.restart_rows([]) == 0 and se.restart_rows([9]) == 0 and se.restart_rows([9, 9, 9]) == 0
    assert se.restart_rows([3, 9]) == 1 and se.restart_rows([3, 5, 9, 9, 9]) == 2 and se.restart_rows([3, 5, 5, 9]) == 3


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    from tamp_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "tamp_batch_seek_index_extend")
    BAD = -21  # TAMP_AMD_BAD_ARGUMENT
    assert BAD == _lib.BAD_ARGUMENT
    w, n = 10, 2
    stride = 16 + (1 << w)
    flat = np.frombuffer(b"\x58abc\x58defg", dtype=np.uint8).copy()
    off, length = np.array([0, 4], np.uint64), np.array([4, 5], np.uint32)
    first, have = np.array([0, 1, 2], np.uint64), np.zeros(n, np.uint32)
    in_pos = np.zeros(2, np.uint32)
    raw = np.zeros(2 * stride + 16, np.uint8)
    at = (-raw.ctypes.data) & 15
    state = raw[at : at + 2 * stride]
    size, status = np.zeros(n, np.uint64), np.zeros(n, np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ok = dict(dictionary=None, dictionary_len=0, w=w, data=p(flat), off=p(off), length=p(length), interval=64, first=p(first), have=p(have),
              in_pos=p(in_pos), state=p(state), stride=stride, size=p(size), status=p(status), n=n, mem=_lib.MEM_HOST, device=0)

    def call(**change):
        a = {**ok, **change}
        return lib.tamp_batch_seek_index_extend(a["dictionary"], a["dictionary_len"], a["w"], a["data"], a["off"], a["length"], a["interval"],
                                                a["first"], a["have"], a["in_pos"], a["state"], a["stride"], a["size"], a["status"], a["n"],
                                                a["mem"], a["device"], None)

    for change in (dict(off=None), dict(length=None), dict(first=None), dict(have=None), dict(size=None), dict(status=None), dict(data=None),
                   dict(interval=0), dict(w=7), dict(w=16), dict(stride=stride + 8), dict(stride=stride - 16),
                   dict(state=C.c_void_p(state.ctypes.data + 4)), dict(mem=7), dict(device=_lib.ALL_DEVICES),
                   dict(n=1 << 32), dict(in_pos=None), dict(state=None)):
        assert call(**change) == BAD, change
    assert call(n=0) == 0  # (nothing to do: no device is looked for either)


def test_the_python_surface_exists_and_checks_before_the_library(monkeypatch):
    import tamp
    import tamp_amd
    from tamp_amd import _lib

    for mod in (tamp_amd, tamp):
        assert callable(mod.extend_seek_index) and callable(mod.SeekIndex.extend)
        assert "extend_seek_index" in mod.__all__

    def no_library():
        raise AssertionError("the library was looked for")

    monkeypatch.setattr(_lib, "load", no_library)
    rng = np.random.default_rng(5)
    w = 8
    index = tamp_amd.SeekIndex(np.array([0, 1, 3], np.uint64), rng.integers(2, 90, 3).astype(np.uint32),
                               rng.integers(0, 256, (3, 16 + (1 << w))).astype(np.uint8), 100, w, np.array([150, 260], np.uint64),
                               np.full(2, 2, np.int8))
    streams = [b"\x58abc", b"\x58defg"]
    with pytest.raises(ValueError):
        tamp_amd.extend_seek_index(streams, seek_index=None)
    with pytest.raises(ValueError):
        tamp_amd.extend_seek_index(streams[:1], seek_index=index)  # fewer streams than the index
    with pytest.raises(ValueError):
        index.extend(streams[:1])
    bad = tamp_amd.SeekIndex(index.first, index.in_pos, index.state[:, :100], 100, w, index.size, index.status)
    with pytest.raises(ValueError):
        bad.extend(streams)
    bad = tamp_amd.SeekIndex(np.array([0, 2, 1], np.uint64), index.in_pos, index.state, 100, w, index.size, index.status)
    with pytest.raises(ValueError):
        bad.extend(streams)
    bad = tamp_amd.SeekIndex(index.first, index.in_pos, index.state, None, w, index.size, index.status)  # the interval is the index's own
    with pytest.raises(ValueError):
        bad.extend(streams)
    torch = pytest.importorskip("torch")
    on_meta = tamp_amd.SeekIndex(*(torch.from_numpy(np.asarray(t).astype(np.int64)) for t in (index.first, index.in_pos, index.state)), 100, w,
                                 index.size, index.status)
    with pytest.raises(ValueError):
        on_meta.extend(streams)  # an index that lives where the data does not
