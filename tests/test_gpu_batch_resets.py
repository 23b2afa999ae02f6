"""GPU tier: dictionary-reset segments for every stream of a batch (tamp_batch_compress_resets, the tamp_batch_reset_* kernels of
tamp_reset_segments_kernel.hpp).

Per stream the expected bytes are what ONE compressor object of the checker (the reference C where it is built, else the oracle)
writes for ``write(seg_0) reset write(seg_1) reset ... write(seg_last) flush(False)`` with ``dictionary_reset=True`` -- the script
of tests/test_gpu_reset_segments.py -- and what tamp_amd_compress_resets returns for that stream alone.  Every call lays its
output slabs out by hand, with 0xA5 guard bytes in front of the first, between all and behind the last; the batches are small:
ten streams, 40 intervals at the longest."""
import ctypes as C
import re

import numpy as np
import pytest
from test_gpu_reset_segments import call as one_call
from test_gpu_reset_segments import script

pytestmark = pytest.mark.gpu

OK, OUTPUT_FULL, EXCESS_BITS, BAD_ARGUMENT = 0, 1, -2, -21
GUARD = 0xA5
SLICES = re.compile(r"\[tamp_amd resets\] batch compress: (\d+) streams, (\d+) closed segments of (\d+) bytes, slab \d+, (\d+) per slice, (\d+) slices$", re.M)


@pytest.fixture(scope="module")
def ta():
    import tamp_amd
    from tamp_amd import _lib

    _lib.load()  # raises if the native library is missing: no silent fallback
    return tamp_amd


@pytest.fixture(scope="module")
def checker():
    from oracle.checker import Oracle, Ref

    return Ref() if Ref.available() else Oracle()


@pytest.fixture(scope="module")
def prose():
    from tamp_amd import workloads as wl

    raw = wl.frozen_corpus("prose")
    assert len(raw) >= (1 << 20), "the frozen corpus (tests/golden/corpus_prose.txt.xz) is part of the tree"
    return (np.frombuffer(raw[: 1 << 20], dtype=np.uint8) & 0x7F).tobytes()  # (fits 7-bit literals)


@pytest.fixture(autouse=True)
def no_tuning(monkeypatch):
    for k in ("TAMP_AMD_RESETS_SLICE", "TAMP_AMD_RESETS_DEBUG"):
        monkeypatch.delenv(k, raising=False)


_expected = {}


def expected(checker, data, interval, window=10, literal=8, extended=True, lazy=False):
    """The reference script's bytes (computed once per input and configuration, shared by the tests)."""
    key = (data, interval, window, literal, extended, lazy)
    if key not in _expected:
        res, blob = checker.stream_script(script(data, interval), window=window, literal=literal, extended=extended,
                                          dictionary_reset=True, lazy_matching=lazy)
        assert res == 0
        _expected[key] = blob
    return _expected[key]


def streams_of(prose, lengths, at=0):
    """One stream per length, cut from the corpus one after the other (different text per stream)."""
    out = []
    for n in lengths:
        out.append(prose[at : at + n])
        at += n + 13
    return out


def mixed(interval):
    return [0, 1, interval - 1, interval, interval + 1, 2 * interval, 2 * interval + 1, 40 * interval - 7, 0, interval]


def layout(caps, residues=None):
    """Slabs laid out by hand: at least 8 guard bytes in front of every slab and behind the last; ``residues``: out_off[i] % 4."""
    offs, at = [], 8
    for i, cap in enumerate(caps):
        if residues is not None:
            at += (residues[i] - at) % 4
        offs.append(at)
        at += cap + 8 + (i % 3)
    return np.array(offs, dtype=np.uint64), at


def batch_call(datas, interval, *, window=10, literal=8, extended=True, lazy=False, caps=None, residues=None, mem="host",
               stream=None, dictionary_reset=1, custom=0, max_in_len=0):
    """One tamp_batch_compress_resets call.  -> (rc, status, out_len, the output buffer, out_off, out_cap)"""
    from tamp_amd import _lib
    from tamp_amd.batch import pack_streams

    lib = _lib.load()
    conf = _lib.TampAmdConf(window, literal, custom, int(extended), dictionary_reset, int(lazy))
    n = len(datas)
    flat, in_off, in_len = pack_streams(datas)
    if flat.size == 0:
        flat = np.zeros(1, np.uint8)
    if caps is None:
        caps = [lib.tamp_amd_compress_resets_bound(len(d), max(interval, 1), literal) for d in datas]
    out_cap = np.array(caps, dtype=np.uint32)
    out_off, total = layout(caps, residues)
    out = np.full(total, GUARD, dtype=np.uint8)
    out_len, status = np.full(n, 0xDEAD, dtype=np.uint32), np.full(n, 99, dtype=np.int8)
    if mem == "host":
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = lib.tamp_batch_compress_resets(C.byref(conf), p(flat), p(in_off), p(in_len), interval, p(out), p(out_off), p(out_cap),
                                            p(out_len), p(status), n, max_in_len, _lib.MEM_HOST, 0, None)
        return rc, status, out_len, out, out_off, out_cap
    import torch

    dev = torch.device("cuda:0")
    up = lambda a, view=None: torch.from_numpy(a.copy() if view is None else a.view(view).copy()).to(dev)  # noqa: E731
    t_flat, t_in_off, t_in_len = up(flat), up(in_off, np.int64), up(in_len, np.int32)
    t_out, t_out_off, t_out_cap = up(out), up(out_off, np.int64), up(out_cap, np.int32)
    t_len, t_status = up(out_len, np.int32), up(status)
    torch.cuda.synchronize()
    dp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.tamp_batch_compress_resets(C.byref(conf), dp(t_flat), dp(t_in_off), dp(t_in_len), interval, dp(t_out), dp(t_out_off),
                                        dp(t_out_cap), dp(t_len), dp(t_status), n, max_in_len, _lib.MEM_DEVICE, 0,
                                        C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    return rc, t_status.cpu().numpy(), t_len.cpu().numpy().view(np.uint32), t_out.cpu().numpy(), out_off, out_cap


def guards_intact(out, out_off, out_cap, out_len=None):
    """Every byte outside the slabs is a guard byte still -- and, with ``out_len`` (host-memory calls write exactly the produced
    bytes), every byte of a slab behind the stream's length as well."""
    mask = np.ones(len(out), dtype=bool)
    for i in range(len(out_off)):
        o = int(out_off[i])
        mask[o : o + (int(out_cap[i]) if out_len is None else int(out_len[i]))] = False
    return bool((out[mask] == GUARD).all())


def stream_bytes(out, out_off, out_len, i):
    o = int(out_off[i])
    return out[o : o + int(out_len[i])].tobytes()


def check_batch(res, wants, mem):
    rc, status, out_len, out, out_off, out_cap = res
    assert rc == 0
    assert list(status) == [OK] * len(wants), list(status)
    assert list(out_len) == [len(w) for w in wants]
    for i, w in enumerate(wants):
        assert stream_bytes(out, out_off, out_len, i) == w, i
    assert guards_intact(out, out_off, out_cap, out_len if mem == "host" else None)


CONFIGS = [(w, lit, ext, False) for w in (8, 10, 15) for lit in (8, 7) for ext in (True, False)] + \
          [(10, lit, ext, True) for lit in (8, 7) for ext in (True, False)]


@pytest.mark.parametrize("window,literal,extended,lazy", CONFIGS)
def test_mixed_batch_is_the_reference_script_per_stream(ta, checker, prose, window, literal, extended, lazy):
    for interval in (16, 1000):
        datas = streams_of(prose, mixed(interval), at=3000)
        wants = [expected(checker, d, interval, window, literal, extended, lazy) for d in datas]
        res = batch_call(datas, interval, window=window, literal=literal, extended=extended, lazy=lazy)
        check_batch(res, wants, "host")
        for d, w in zip(datas, wants):  # ... and tamp_amd_compress_resets of that stream alone
            rc, status, out_len, out, guard, _ = one_call(ta, d, interval, window=window, literal=literal, extended=extended, lazy=lazy)
            assert (rc, status) == (0, OK) and out[:out_len] == w


@pytest.mark.parametrize("mem", ["host", "device"])
def test_no_closed_segment_and_one_stream(ta, checker, prose, mem):
    """Every stream with K = 1: the closed launch is empty.  And batches of one stream, with and without closed segments."""
    for interval, lengths in ((16, [0, 5, 16, 1, 15]), (1000, [999, 0, 1000]), (16, [7]), (16, [0]), (16, [3 * 16 + 5]), (1, [1])):
        datas = streams_of(prose, lengths, at=60_000)
        wants = [expected(checker, d, interval) for d in datas]
        check_batch(batch_call(datas, interval, mem=mem), wants, mem)


def test_stream_boundaries_at_the_scan_tiles_edges(ta, checker, prose):
    """N = 1, streams of tile - 1, tile and tile + 1 bytes, each flanked by empty and 1-byte streams: the streams' boundaries fall
    inside a tile of the scans, on its edge and one past it.  The second batch puts the boundaries of the CLOSED table (a stream of
    L bytes has L - 1 closed segments at N = 1) on slots tile - 1, tile and tile + 1 of the scan that places them."""
    from tamp_amd import _lib

    tile = _lib.RESETS_SCAN_TILE
    first = [0, 1, tile - 1, 0, 1, tile, 1, 0, tile + 1, 1, 0]
    second = [tile, 0, 2, 1, 2, 2, 0, tile + 1, 2]
    closed_first = np.cumsum([0] + [max(n, 1) - 1 for n in second])
    assert {tile - 1, tile, tile + 1} <= set(int(x) for x in closed_first)
    for lengths in (first, second):
        datas = streams_of(prose, lengths, at=80_000)
        wants = [expected(checker, d, 1) for d in datas]
        for mem in ("host", "device"):
            check_batch(batch_call(datas, 1, mem=mem), wants, mem)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_slices(ta, checker, prose, mem, monkeypatch, capfd):
    """TAMP_AMD_RESETS_SLICE=7 on the mixed batch: streams straddle slices, slices hold several whole streams -- the same bytes."""
    monkeypatch.setenv("TAMP_AMD_RESETS_DEBUG", "1")
    monkeypatch.setenv("TAMP_AMD_RESETS_SLICE", "7")
    for interval in (16, 1000):
        datas = streams_of(prose, mixed(interval), at=3000)
        wants = [expected(checker, d, interval) for d in datas]
        capfd.readouterr()
        res = batch_call(datas, interval, mem=mem)
        m = SLICES.search(capfd.readouterr().err)
        assert m, "no debug line"
        streams, closed, iv, per_slice, slices = (int(x) for x in m.groups())
        assert (streams, closed, iv, per_slice) == (10, 43, interval, 7) and slices == 7 + 2
        check_batch(res, wants, mem)


@pytest.mark.parametrize("mem", ["host", "device", "device-stream"])
def test_every_slab_alignment_behind_guards(ta, checker, prose, mem):
    """out_off[i] % 4 takes all four values, streams of several segments and of one: every guard byte is intact."""
    import torch

    for interval in (16, 17):
        lengths = [3 * interval + 5, 2, 2 * interval, interval + 3, 0, 5 * interval + 1, 1, 7 * interval]
        residues = [0, 1, 2, 3, 3, 2, 1, 0]
        datas = streams_of(prose, lengths, at=100_000)
        wants = [expected(checker, d, interval) for d in datas]
        # (room to the byte: the slab of a stream ends where its last byte does, the next guard byte right behind it)
        for caps in (None, [len(w) for w in wants]):
            stream = torch.cuda.Stream() if mem == "device-stream" else None
            res = batch_call(datas, interval, residues=residues, caps=caps, mem=mem.split("-")[0], stream=stream)
            assert {int(o) % 4 for o in res[4]} == {0, 1, 2, 3}
            check_batch(res, wants, mem)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_a_failing_stream_fails_alone(ta, checker, prose, mem):
    interval = 16
    datas = streams_of(prose, [5 * interval + 3, 9 * interval + 1, 7 * interval], at=120_000)
    # stream 1 gets one byte less room than its length
    wants = [expected(checker, d, interval) for d in datas]
    caps = [len(wants[0]), len(wants[1]) - 1, len(wants[2])]
    rc, status, out_len, out, out_off, out_cap = batch_call(datas, interval, caps=caps, mem=mem)
    assert rc == 0 and list(status) == [OK, OUTPUT_FULL, OK] and list(out_len) == [len(wants[0]), 0, len(wants[2])]
    assert stream_bytes(out, out_off, out_len, 0) == wants[0] and stream_bytes(out, out_off, out_len, 2) == wants[2]
    assert guards_intact(out, out_off, out_cap, out_len if mem == "host" else None)
    # at literal 7 a byte of 8 bits sits in a MIDDLE segment of stream 2
    bad = bytearray(datas[2])
    bad[3 * interval + 5] = 0x80
    datas7 = [datas[0], datas[1], bytes(bad)]
    wants7 = [expected(checker, d, interval, literal=7) for d in datas7[:2]]
    rc, status, out_len, out, out_off, out_cap = batch_call(datas7, interval, literal=7, mem=mem)
    assert rc == 0 and list(status) == [OK, OK, EXCESS_BITS] and list(out_len) == [len(wants7[0]), len(wants7[1]), 0]
    assert stream_bytes(out, out_off, out_len, 0) == wants7[0] and stream_bytes(out, out_off, out_len, 1) == wants7[1]
    assert guards_intact(out, out_off, out_cap, out_len if mem == "host" else None)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_a_stale_max_in_len_costs_no_bytes(ta, checker, prose, mem):
    """max_in_len is a hint that sizes the compress kernel's block, as for tamp_batch_compress: far too small, far too large or
    unknown (0), every stream is the reference script's bytes -- the slabs are sized from the tables, not from the hint."""
    for interval, lengths in ((1000, mixed(1000)), (65536, [3000, 0, 700, 65536 + 9])):
        datas = streams_of(prose, lengths, at=140_000)
        wants = [expected(checker, d, interval) for d in datas]
        for hint in (100, 1, 16, 1 << 30, 0):
            check_batch(batch_call(datas, interval, mem=mem, max_in_len=hint), wants, mem)


def test_calls_outside_the_contract(ta, prose):
    datas = streams_of(prose, [100, 40], at=0)
    # (the last one: an interval whose one-segment bound does not fit 32 bits)
    for kwargs, interval in ((dict(dictionary_reset=0), 16), (dict(custom=1), 16), ({}, 0), (dict(window=16), 16), ({}, 0xFFFFFFFF)):
        for mem in ("host", "device"):
            rc, status, out_len, out, out_off, out_cap = batch_call(datas, interval, mem=mem, **kwargs)
            assert rc == BAD_ARGUMENT, (kwargs, interval, mem)
            assert (out == GUARD).all() and list(status) == [99, 99] and list(out_len) == [0xDEAD, 0xDEAD]
    # no streams: nothing is done
    rc, status, out_len, out, out_off, out_cap = batch_call([], 16)
    assert rc == 0 and (out == GUARD).all()


def test_python_surface(ta, checker, prose):
    """compress_batch(..., dictionary_reset=True, reset_interval=N) in its three input forms: the bytes of compress() per stream,
    which decompress_batch reads back."""
    import torch

    from tamp_amd.batch import pack_streams

    for interval, kw in ((1000, {}), (16, dict(window=12, extended=False)), (4096, dict(lazy_matching=True))):
        datas = streams_of(prose, mixed(interval)[:8] + [0, 3 * interval + 1], at=200_000)
        wants = [ta.compress(d, dictionary_reset=True, reset_interval=interval, **kw) for d in datas]
        assert wants[5] == expected(checker, datas[5], interval, kw.get("window", 10), 8, kw.get("extended", True), kw.get("lazy_matching", False))
        res = ta.compress_batch(datas, dictionary_reset=True, reset_interval=interval, **kw)
        assert (res.status == OK).all() and res.streams() == wants
        back = ta.decompress_batch(res.streams())
        assert (back.status == 2).all() and back.streams() == datas
        flat, in_off, in_len = pack_streams(datas)
        res = ta.compress_batch(flat, in_off, in_len, dictionary_reset=True, reset_interval=interval, **kw)
        assert (res.status == OK).all() and res.streams() == wants
        dev = torch.device("cuda:0")
        t = ta.compress_batch(torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(in_off.view(np.int64).copy()).to(dev),
                              torch.from_numpy(in_len.view(np.int32).copy()).to(dev), dictionary_reset=True, reset_interval=interval,
                              max_in_len=64, **kw)  # (a stale hint: speed, never bytes)
        torch.cuda.synchronize()
        assert (t.status.cpu().numpy() == OK).all() and t.streams() == wants
        # an explicit capacity for every stream, one byte too few for the longest: that stream alone fails
        longest = max(len(w) for w in wants)
        res = ta.compress_batch(datas, dictionary_reset=True, reset_interval=interval, out_cap=longest - 1, **kw)
        assert [int(s) for s in res.status] == [OUTPUT_FULL if len(w) == longest else OK for w in wants]
