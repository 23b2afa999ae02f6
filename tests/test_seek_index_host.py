"""CPU tier: the seek index's definition of a checkpoint, checked on the oracle's decoder object (tests/seek_index_input.py), and
the argument checks and file format of the Python layer.  The GPU side: tests/test_gpu_seek_index.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cut_sweep_input as cs  # noqa: E402
import seek_index_input as si  # noqa: E402


@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=[cs.case_id(*c) for c in cs.CONFIGS])
def test_count_rule_and_every_call_output_full(oracle, window, extended):
    src, stream = si.cut_sweep_stream(oracle, window, extended)
    for N in (1, 7, 64):
        rows, S, statuses, final = si.expected_checkpoints(oracle, stream, N)
        assert S == len(src)
        assert len(rows) == (S - 1) // N
        assert all(r == si.OUTPUT_FULL for r in statuses)
        assert final in (si.INPUT_EXHAUSTED, si.OUTPUT_FULL)  # (the last call may fill its room exactly)
        assert [row["in_pos"] for row in rows] == sorted(row["in_pos"] for row in rows)


@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=[cs.case_id(*c) for c in cs.CONFIGS])
def test_restart_from_every_checkpoint(oracle, window, extended):
    src, stream = si.cut_sweep_stream(oracle, window, extended)
    N = 7
    rows, S, _, _ = si.expected_checkpoints(oracle, stream, N)
    for k, row in enumerate(rows, start=1):
        r, got = si.restart(oracle, stream, row["state"], row["window"], row["in_pos"], S + 16)
        assert r == si.INPUT_EXHAUSTED and got == src[k * N:], k


@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=[cs.case_id(*c) for c in cs.CONFIGS])
def test_checkpoint_classes_at_interval_one(oracle, window, extended):
    """A condition on the INPUT: at N = 1 the extended streams have checkpoints at a token boundary, inside a plain match, inside
    an RLE run and inside an extended match, the v1 streams of the first two kinds -- so the GPU test cannot miss a class."""
    _, stream = si.cut_sweep_stream(oracle, window, extended)
    rows, _, _, _ = si.expected_checkpoints(oracle, stream, 1)
    classes = {si.checkpoint_class(row["state"]) for row in rows}
    assert classes == ({"boundary", "match", "rle", "ext"} if extended else {"boundary", "match"})


def _index(n_streams=2, rows=3, w=8):
    from tamp_amd.batch import SeekIndex

    rng = np.random.default_rng(5)
    first = np.array([0, 1, rows][: n_streams + 1], dtype=np.uint64)
    return SeekIndex(first, rng.integers(2, 90, rows).astype(np.uint32), rng.integers(0, 256, (rows, 16 + (1 << w))).astype(np.uint8),
                     100, w, np.array([150, 260][:n_streams], dtype=np.uint64), np.full(n_streams, 2, dtype=np.int8))


def test_save_load_round_trip(tmp_path):
    from tamp_amd import SeekIndex

    a = _index()
    path = str(tmp_path / "index.npz")
    a.save(path)
    assert os.path.exists(path)  # (exactly the path given)
    b = SeekIndex.load(path)
    for f in ("first", "in_pos", "state", "size", "status"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f
    assert (b.interval, b.window_bits) == (100, 8)
    assert b.state.ctypes.data % 16 == 0
    assert a.nbytes == b.nbytes == 3 * 8 + 3 * 4 + 3 * 272 + 2 * 8 + 2
    c = a.to("cpu")
    assert np.array_equal(c.state, a.state) and c.state.ctypes.data % 16 == 0


def test_argument_errors_come_before_the_library(monkeypatch):
    import tamp_amd
    from tamp_amd import _lib

    def no_library():
        raise AssertionError("the library was looked for")

    monkeypatch.setattr(_lib, "load", no_library)
    streams = [b"\x58abc", b"\x58defg"]
    ok = dict(seek_index=_index(), stream_index=[0, 1], begin=[0, 5], length=[4, 4])

    def refused(**change):
        with pytest.raises(ValueError):
            tamp_amd.read_ranges_seek(streams, **{**ok, **change})

    refused(seek_index=None)
    refused(seek_index=tamp_amd.ResetIndex(np.zeros(3, np.uint64), np.zeros(0, np.uint32)))  # (wrong type)
    refused(seek_index=_index(n_streams=1, rows=1))                                           # first not n + 1 long
    for interval in (0, -1, 1 << 32, 2.5, True, None):
        bad = _index()
        bad.interval = interval
        if interval is None:
            continue  # (None is build_seek_index's default, not a value an index holds: checked below)
        refused(seek_index=bad)
    bad = _index()
    bad.window_bits = 16
    refused(seek_index=bad)
    bad = _index()
    bad.in_pos = bad.in_pos[:2]                                                                # tables of unequal length
    refused(seek_index=bad)
    bad = _index()
    bad.state = bad.state[:, :100]
    refused(seek_index=bad)
    bad = _index()
    bad.first = np.array([0, 2, 1], dtype=np.uint64)                                           # no running sum
    refused(seek_index=bad)
    refused(stream_index=[0])                                                                  # tables of unequal length
    refused(begin=[0, -1])
    refused(begin=[0, 1 << 64])
    refused(length=[4, 1 << 32])
    refused(length=[4, -1])
    refused(stream_index=[0, 1 << 32])
    refused(stream_index=np.array([0.5, 1.0]))                                                 # wrong types
    refused(begin=np.array([False, True]))
    torch = pytest.importorskip("torch")
    on_meta = _index()
    on_meta.first, on_meta.in_pos, on_meta.state = (torch.from_numpy(np.asarray(t).astype(np.int64)) for t in
                                                    (on_meta.first, on_meta.in_pos, on_meta.state))
    refused(seek_index=on_meta)                                                                # an index that lives where the data does not
    for interval in (0, -5, 1 << 32, 1.5, "64", True):
        with pytest.raises(ValueError):
            tamp_amd.build_seek_index(streams, interval=interval)
    with pytest.raises(ValueError):
        tamp_amd.build_seek_index(streams, max_window_bits=7)
    with pytest.raises(ValueError):
        tamp_amd.build_seek_index(streams, max_window_bits=16)
