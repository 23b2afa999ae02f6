"""GPU tier: the reset index of a batch (tamp_batch_compress_resets_index) and the batch decode that takes it as a hint
(tamp_batch_decompress_resets, the check / plan / units kernels of tamp_reset_segments_kernel.hpp).

The index is what tamp_amd_compress_resets returns per stream; the decode is, per stream, what tamp_batch_decompress gives on the
same tables (and the checker's decompress), WHATEVER the index holds -- which path a stream took is read from the library's debug
line.  Helpers and the batches (about ten streams cut from the 7-bit prose fixture with ``mixed(interval)``, slabs laid out by hand
behind 0xA5 guards) are those of tests/test_gpu_batch_resets.py."""
import ctypes as C
import random
import re

import numpy as np
import pytest
from long_stream_writer import TokenWriter, read_tokens
from test_gpu_batch_resets import CONFIGS, GUARD, guards_intact, layout, mixed, stream_bytes, streams_of
from test_gpu_batch_resets import batch_call as plain_compress
from test_gpu_batch_resets import expected
from test_gpu_reset_segments import call as one_call

pytestmark = pytest.mark.gpu

OK, OUTPUT_FULL, INPUT_EXHAUSTED, OOB, INVALID_CONF, BAD_ARGUMENT = 0, 1, 2, -4, -3, -21
LINE = re.compile(r"\[tamp_amd resets\] batch decode: (\d+) streams, (\d+) split into (\d+) units, (\d+) whole$", re.M)


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
def debug_line(monkeypatch):
    monkeypatch.delenv("TAMP_AMD_RESETS_SLICE", raising=False)
    monkeypatch.setenv("TAMP_AMD_RESETS_DEBUG", "1")


def segments(n, interval):
    return max(1, -(-n // interval))


def _device(arrays, views):
    import torch

    dev = torch.device("cuda:0")
    return [torch.from_numpy(a.copy() if v is None else a.view(v).copy()).to(dev) for a, v in zip(arrays, views)]


def index_call(datas, interval, *, window=10, literal=8, extended=True, lazy=False, caps=None, mem="host", reset_cap=None,
               want_first=True):
    """One tamp_batch_compress_resets_index call.  -> (rc, status, out_len, out, out_off, out_cap, reset_first, reset_off); the two
    index tables start as 0xEE bytes."""
    from tamp_amd import _lib
    from tamp_amd.batch import pack_streams

    lib = _lib.load()
    conf = _lib.TampAmdConf(window, literal, 0, int(extended), 1, int(lazy))
    n = len(datas)
    flat, in_off, in_len = pack_streams(datas)
    if flat.size == 0:
        flat = np.zeros(1, np.uint8)
    if caps is None:
        caps = [lib.tamp_amd_compress_resets_bound(len(d), interval, literal) for d in datas]
    out_cap = np.array(caps, dtype=np.uint32)
    out_off, total = layout(caps)
    out = np.full(total, GUARD, dtype=np.uint8)
    out_len, status = np.full(n, 0xDEAD, dtype=np.uint32), np.full(n, 99, dtype=np.int8)
    entries = sum(segments(len(d), interval) - 1 for d in datas)
    if reset_cap is None:
        reset_cap = entries
    first = np.full(n + 1, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    off = np.full(max(reset_cap, 1), 0xEEEEEEEE, dtype=np.uint32)
    if mem == "host":
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = lib.tamp_batch_compress_resets_index(C.byref(conf), p(flat), p(in_off), p(in_len), interval, p(out), p(out_off), p(out_cap),
                                                  p(out_len), p(status), n, 0, _lib.MEM_HOST, 0, None, p(first) if want_first else None,
                                                  p(off), reset_cap)
        return rc, status, out_len, out, out_off, out_cap, first, off
    import torch

    t = _device([flat, in_off, in_len, out, out_off, out_cap, out_len, status, first, off],
                [None, np.int64, np.int32, None, np.int64, np.int32, np.int32, None, np.int64, np.int32])
    torch.cuda.synchronize()
    dp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rc = lib.tamp_batch_compress_resets_index(C.byref(conf), dp(t[0]), dp(t[1]), dp(t[2]), interval, dp(t[3]), dp(t[4]), dp(t[5]),
                                              dp(t[6]), dp(t[7]), n, 0, _lib.MEM_DEVICE, 0, None, dp(t[8]) if want_first else None,
                                              dp(t[9]), reset_cap)
    torch.cuda.synchronize()
    return (rc, t[7].cpu().numpy(), t[6].cpu().numpy().view(np.uint32), t[3].cpu().numpy(), out_off, out_cap,
            t[8].cpu().numpy().view(np.uint64), t[9].cpu().numpy().view(np.uint32))


def decode_call(kind, blobs, caps, *, first=None, off=None, residues=None, mem="host", stream=None, max_wbits=15, sizes_only=False):
    """One decode call on hand-laid tables: ``kind`` "resets" (tamp_batch_decompress_resets), "plain" (tamp_batch_decompress) or,
    with ``sizes_only``, tamp_batch_decoded_size.  -> (rc, status, out_len, consumed, out, out_off, out_cap)"""
    from tamp_amd import _lib
    from tamp_amd.batch import pack_streams

    lib = _lib.load()
    n = len(blobs)
    flat, in_off, in_len = pack_streams(blobs)
    if flat.size == 0:
        flat = np.zeros(1, np.uint8)
    out_cap = np.array(caps, dtype=np.uint32)
    out_off, total = layout([int(c) for c in caps], residues)
    out = np.full(total, GUARD, dtype=np.uint8)
    out_len, status, consumed = np.full(n, 0xDEAD, dtype=np.uint32), np.full(n, 99, dtype=np.int8), np.full(n, 0xDEAD, dtype=np.uint32)
    first = np.zeros(n + 1, np.uint64) if first is None else np.ascontiguousarray(first, dtype=np.uint64)
    off = np.zeros(1, np.uint32) if off is None or len(off) == 0 else np.ascontiguousarray(off, dtype=np.uint32)

    def run(p, m, st):
        o, oo = (None, None) if sizes_only else (p(out_t), p(out_off_t))
        if kind == "resets":
            return lib.tamp_batch_decompress_resets(max_wbits, p(flat_t), p(in_off_t), p(in_len_t), p(first_t), p(off_t), o, oo, p(cap_t),
                                                    p(len_t), p(status_t), p(consumed_t), n, m, 0, st)
        if sizes_only:
            return lib.tamp_batch_decoded_size(0, max_wbits, p(flat_t), p(in_off_t), p(in_len_t), p(cap_t), p(len_t), p(status_t),
                                               p(consumed_t), n, m, 0, st)
        return lib.tamp_batch_decompress(None, 0, max_wbits, p(flat_t), p(in_off_t), p(in_len_t), o, oo, p(cap_t), p(len_t),
                                         p(status_t), p(consumed_t), n, m, 0, st)

    if mem == "host":
        flat_t, in_off_t, in_len_t, out_t, out_off_t, cap_t, len_t, status_t, consumed_t, first_t, off_t = (
            flat, in_off, in_len, out, out_off, out_cap, out_len, status, consumed, first, off)
        rc = run(lambda a: a.ctypes.data_as(C.c_void_p), _lib.MEM_HOST, None)
        return rc, status, out_len, consumed, out, out_off, out_cap
    import torch

    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        flat_t, in_off_t, in_len_t, out_t, out_off_t, cap_t, len_t, status_t, consumed_t, first_t, off_t = _device(
            [flat, in_off, in_len, out, out_off, out_cap, out_len, status, consumed, first, off],
            [None, np.int64, np.int32, None, np.int64, np.int32, np.int32, None, np.int32, np.int64, np.int32])
    torch.cuda.synchronize()
    rc = run(lambda x: C.c_void_p(x.data_ptr()), _lib.MEM_DEVICE, C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return (rc, status_t.cpu().numpy(), len_t.cpu().numpy().view(np.uint32), consumed_t.cpu().numpy().view(np.uint32),
            out_t.cpu().numpy(), out_off, out_cap)


def same_as_plain(got, blobs, caps, mem, *, residues=None, checker=None, sizes_only=False, max_wbits=15):
    """``got`` against tamp_batch_decompress (or the size query) on the same tables, stream by stream; optionally the checker too."""
    want = decode_call("plain", blobs, caps, residues=residues, mem=mem, max_wbits=max_wbits, sizes_only=sizes_only)
    assert got[0] == 0 and want[0] == 0
    for i in range(len(blobs)):
        assert (int(got[1][i]), int(got[2][i]), int(got[3][i])) == (int(want[1][i]), int(want[2][i]), int(want[3][i])), i
        if not sizes_only:
            assert stream_bytes(got[4], got[5], got[2], i) == stream_bytes(want[4], want[5], want[2], i), i
        if checker is not None:
            st, data, used = checker.decompress(blobs[i], cap=int(caps[i]), max_window_bits=max_wbits & 0x7F)
            assert (int(got[1][i]), int(got[2][i]), int(got[3][i])) == (st, len(data), used), i
            if not sizes_only:
                assert stream_bytes(got[4], got[5], got[2], i) == data, i
    if sizes_only:
        assert (got[4] == GUARD).all()
    else:
        assert guards_intact(got[4], got[5], got[6], got[2] if mem == "host" else None)


def line_of(capfd):
    m = LINE.findall(capfd.readouterr().err)
    assert m, "no debug line"
    return tuple(int(x) for x in m[-1])  # (streams, split, units, whole)


def true_entries(blob):
    """The byte behind every reset of a stream: behind every FLUSH whose predecessor is a FLUSH (decompressor.c:501-513)."""
    toks = read_tokens(blob)[0]
    return [(b.bit + b.nbits) // 8 for a, b in zip(toks, toks[1:]) if a.kind == "F" and b.kind == "F"]


def index_of(entries_per_stream):
    first = np.cumsum([0] + [len(e) for e in entries_per_stream]).astype(np.uint64)
    off = np.array([x for e in entries_per_stream for x in e], dtype=np.uint32)
    return first, off


_batches = {}


def true_batch(checker, prose, interval, window=10, literal=8, extended=True, lazy=False, lengths=None, at=3000):
    """(datas, blobs, entries per stream) of the mixed batch: the reference script's bytes and where their resets are (computed once)."""
    key = (interval, window, literal, extended, lazy, tuple(lengths) if lengths else None, at)
    if key not in _batches:
        datas = streams_of(prose, lengths or mixed(interval), at=at)
        blobs = [expected(checker, d, interval, window, literal, extended, lazy) for d in datas]
        entries = [true_entries(b) for b in blobs]
        assert [len(e) for e in entries] == [segments(len(d), interval) - 1 for d in datas]
        _batches[key] = (datas, blobs, entries)
    return _batches[key]


def roomy(datas):
    return [len(d) + 1 + (i % 3) for i, d in enumerate(datas)]


# ---- 1. the index ----

@pytest.mark.parametrize("window,literal,extended,lazy", CONFIGS)
def test_index_is_the_one_stream_calls(ta, checker, prose, window, literal, extended, lazy, monkeypatch):
    for interval in (16, 1000):
        datas, blobs, entries = true_batch(checker, prose, interval, window, literal, extended, lazy)
        plain = plain_compress(datas, interval, window=window, literal=literal, extended=extended, lazy=lazy)
        ones = []
        for d in datas:  # tamp_amd_compress_resets of that stream alone
            rc, status, out_len, out, guard, reset_off = one_call(ta, d, interval, window=window, literal=literal, extended=extended, lazy=lazy)
            assert (rc, status) == (0, OK)
            ones.append([int(x) for x in reset_off])
        assert ones == entries
        for mem, slice_env in (("host", None), ("device", None), ("host", "7"), ("device", "7")):
            if slice_env:
                monkeypatch.setenv("TAMP_AMD_RESETS_SLICE", slice_env)  # (streams straddle slices)
            else:
                monkeypatch.delenv("TAMP_AMD_RESETS_SLICE", raising=False)
            rc, status, out_len, out, out_off, out_cap, first, off = index_call(datas, interval, window=window, literal=literal,
                                                                                extended=extended, lazy=lazy, mem=mem)
            assert rc == 0 and list(status) == [OK] * len(datas)
            assert list(out_len) == list(plain[2]) and (out == plain[3]).all() if mem == "host" else True
            for i, b in enumerate(blobs):
                assert stream_bytes(out, out_off, out_len, i) == b, i
            assert guards_intact(out, out_off, out_cap, out_len if mem == "host" else None)
            assert list(first) == list(np.cumsum([0] + [len(e) for e in entries]))
            for i, e in enumerate(entries):
                assert list(off[int(first[i]) : int(first[i + 1])]) == e, i
                for x in e:
                    assert blobs[i][x - 2 : x] == b"\x55\x80"
        monkeypatch.delenv("TAMP_AMD_RESETS_SLICE", raising=False)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_index_room_and_a_failing_stream(ta, checker, prose, mem):
    datas, blobs, entries = true_batch(checker, prose, 16)
    total = sum(len(e) for e in entries)
    # one entry short: refused before anything is written
    rc, status, out_len, out, out_off, out_cap, first, off = index_call(datas, 16, mem=mem, reset_cap=total - 1)
    assert rc == BAD_ARGUMENT
    assert (out == GUARD).all() and list(status) == [99] * len(datas) and list(out_len) == [0xDEAD] * len(datas)
    assert (first == 0xEEEEEEEEEEEEEEEE).all() and (off == 0xEEEEEEEE).all()
    # room to spare, and no reset_first wanted
    rc, status, out_len, out, out_off, out_cap, first, off = index_call(datas, 16, mem=mem, reset_cap=total + 5, want_first=False)
    assert rc == 0 and list(off[:total]) == [x for e in entries for x in e] and (off[total:] == 0xEEEEEEEE).all()
    assert (first == 0xEEEEEEEEEEEEEEEE).all()
    # a stream whose room is one byte short fails alone; the other streams' entries are right
    caps = [len(b) for b in blobs]
    victim = 7
    caps[victim] -= 1
    rc, status, out_len, out, out_off, out_cap, first, off = index_call(datas, 16, mem=mem, caps=caps)
    assert rc == 0 and list(status) == [OUTPUT_FULL if i == victim else OK for i in range(len(datas))]
    assert guards_intact(out, out_off, out_cap, out_len if mem == "host" else None)
    for i, e in enumerate(entries):
        if i != victim:
            assert stream_bytes(out, out_off, out_len, i) == blobs[i] and list(off[int(first[i]) : int(first[i + 1])]) == e, i


# ---- 2. round trip, taken ----

@pytest.mark.parametrize("window,literal,extended,lazy", CONFIGS)
def test_round_trip_takes_the_segments(ta, checker, prose, window, literal, extended, lazy, capfd):
    import torch

    for interval in (16, 1000):
        datas, blobs, entries = true_batch(checker, prose, interval, window, literal, extended, lazy)
        first, off = index_of(entries)
        caps = roomy(datas)
        residues = [i % 4 for i in range(len(datas))]
        split = [len(e) >= 1 for e in entries]
        for mem in ("host", "device", "device-stream"):
            stream = torch.cuda.Stream() if mem == "device-stream" else None
            kind = mem.split("-")[0]
            capfd.readouterr()
            got = decode_call("resets", blobs, caps, first=first, off=off, residues=residues, mem=kind, stream=stream)
            # every stream with K >= 2 is split, u = the sum of their K
            assert line_of(capfd) == (len(datas), sum(split), sum(len(e) + 1 for e in entries if e), len(datas) - sum(split))
            assert {int(o) % 4 for o in got[5]} == {0, 1, 2, 3}
            same_as_plain(got, blobs, caps, kind, residues=residues, checker=checker if mem == "host" else None)
            assert list(got[1]) == [INPUT_EXHAUSTED] * len(datas)
            for i, d in enumerate(datas):
                assert stream_bytes(got[4], got[5], got[2], i) == d, i
        for mem in ("host", "device"):  # the size-only form
            capfd.readouterr()
            got = decode_call("resets", blobs, caps, first=first, off=off, mem=mem, sizes_only=True)
            assert line_of(capfd)[1] == sum(split)
            same_as_plain(got, blobs, caps, mem, sizes_only=True)
            assert [int(x) for x in got[2]] == [len(d) for d in datas]


# ---- 3. room ----

@pytest.mark.parametrize("mem", ["host", "device"])
def test_room(ta, checker, prose, mem, capfd):
    """out_cap = size + 1 is split; the size exactly, size - 1 and 0 are whole: every triple is the existing call's."""
    datas, blobs, entries = true_batch(checker, prose, 16)
    first, off = index_of(entries)
    victims = [i for i, e in enumerate(entries) if e][:3]
    assert len(victims) == 3
    n_split = sum(1 for e in entries if e)
    for delta, whole in ((1, 0), (0, 3), (-1, 3), (None, 3)):
        caps = roomy(datas)
        for v in victims:
            caps[v] = 0 if delta is None else len(datas[v]) + delta
        capfd.readouterr()
        got = decode_call("resets", blobs, caps, first=first, off=off, mem=mem)
        assert line_of(capfd)[1] == n_split - whole, delta
        same_as_plain(got, blobs, caps, mem)
        capfd.readouterr()
        got = decode_call("resets", blobs, caps, first=first, off=off, mem=mem, sizes_only=True)
        assert line_of(capfd)[1] == n_split - whole, delta
        same_as_plain(got, blobs, caps, mem, sizes_only=True)


# ---- 4. an index that lies ----

def lone_flush_stream(extended):
    """A stream with the reset bit whose ONE FLUSH token starts byte aligned: 55 80 stands in front of the byte behind it, and it is
    no reset.  -> (blob, that offset)"""
    rng = random.Random(11)
    w = TokenWriter(window=10, literal=8, extended=extended, more=0)
    w.fill_to(w.bit + 8 * 40 - (w.bit % 8), rng)
    assert w.bit % 8 == 0
    w.flush()
    at = w.bit // 8
    w.fill_to(w.bit + 8 * 30, rng)
    blob = w.blob()
    assert blob[at - 2 : at] == b"\x55\x80" and true_entries(blob) == []
    return blob, at


@pytest.mark.parametrize("mem", ["host", "device"])
def test_an_index_that_lies(ta, checker, prose, mem, capfd):
    """One stream of the batch gets an index that is not true, the others keep theirs: its triple and bytes are the existing call's,
    the line counts it whole and the others split."""
    datas, blobs, entries = true_batch(checker, prose, 16)
    victim = 7  # (40 segments)
    assert len(entries[victim]) >= 5
    n_split = sum(1 for e in entries if e)
    e = entries[victim]
    lone, lone_at = lone_flush_stream(False)
    lone_x, lone_x_at = lone_flush_stream(True)
    lies = {
        "behind a lone FLUSH that starts byte aligned": (lone, [lone_at]),
        "behind a lone FLUSH, extended format": (lone_x, [lone_x_at]),
        "in the middle of a token": (None, e[:3] + [e[3] - 1] + e[4:]),
        "a true entry plus 1": (None, e[:3] + [e[3] + 1] + e[4:]),
        "out of order": (None, e[:2] + [e[3], e[2]] + e[4:]),
        "twice the same": (None, e[:2] + [e[2], e[2]] + e[4:]),
        "beyond in_len": (None, e[:-1] + [len(blobs[victim]) + 1]),
        "far beyond in_len": (None, e[:-1] + [0xFFFFFFFF]),
        "inside the header": (None, [1] + e[1:]),
        "the header's end": (None, [2] + e[1:]),
        "zero": (None, [0] + e[1:]),
    }
    for what, (blob, lie) in lies.items():
        bs, es = list(blobs), [list(x) for x in entries]
        if blob is not None:
            bs[victim] = blob
        es[victim] = lie
        first, off = index_of(es)
        caps = [max(len(b) * 16, 64) for b in bs]
        capfd.readouterr()
        got = decode_call("resets", bs, caps, first=first, off=off, mem=mem)
        assert line_of(capfd) == (len(bs), n_split - 1, sum(len(x) + 1 for i, x in enumerate(entries) if x and i != victim),
                                  len(bs) - n_split + 1), what
        same_as_plain(got, bs, caps, mem, checker=checker)
        capfd.readouterr()
        got = decode_call("resets", bs, caps, first=first, off=off, mem=mem, sizes_only=True)
        assert line_of(capfd)[1] == n_split - 1, what
        same_as_plain(got, bs, caps, mem, sizes_only=True)
    # a reset_first that is no running sum: the call goes without an index
    first, off = index_of(entries)
    for bad in (np.concatenate([first[:3], first[3:4] + 50, first[4:]]), first + np.uint64(1), first[::-1].copy()):
        caps = roomy(datas)
        capfd.readouterr()
        got = decode_call("resets", blobs, caps, first=bad, off=np.concatenate([off, np.zeros(64, np.uint32)]), mem=mem)
        assert line_of(capfd) == (len(blobs), 0, 0, len(blobs))
        same_as_plain(got, blobs, caps, mem)


# ---- 5. an index that is incomplete or odd, yet true ----

@pytest.mark.parametrize("mem", ["host", "device"])
def test_true_but_incomplete_or_odd(ta, checker, prose, mem, capfd):
    datas, blobs, entries = true_batch(checker, prose, 16)
    n_split = sum(1 for e in entries if e)
    # one true entry dropped: the segment holds an inner reset, which its own decode handles
    es = [list(e) for e in entries]
    del es[7][4]
    first, off = index_of(es)
    caps = roomy(datas)
    capfd.readouterr()
    got = decode_call("resets", blobs, caps, first=first, off=off, mem=mem)
    assert line_of(capfd) == (len(blobs), n_split, sum(len(x) + 1 for x in es if x), len(blobs) - n_split)
    same_as_plain(got, blobs, caps, mem, checker=checker)
    # two resets in a row from the checker's object; four FLUSH tokens in a row from the writer
    a, b = prose[500:560], prose[900:990]
    res, twice = checker.stream_script([("write", a), ("reset",), ("reset",), ("write", b), ("flush", False)], dictionary_reset=True)
    assert res == 0 and len(true_entries(twice)) >= 2  # (segments of one FLUSH token between them)
    rng = random.Random(5)
    w = TokenWriter(window=10, literal=8, extended=False, more=0)
    w.fill_to(8 * 30, rng)
    for _ in range(4):
        w.flush()
    w.fill_to(w.bit + 8 * 25, rng)
    four = w.blob()
    assert len(true_entries(four)) == 3
    bs = [twice, blobs[7], four]
    es = [true_entries(x) for x in bs]
    first, off = index_of(es)
    caps = [max(len(x) * 16, 64) for x in bs]
    capfd.readouterr()
    got = decode_call("resets", bs, caps, first=first, off=off, mem=mem)
    assert line_of(capfd) == (3, 3, sum(len(x) + 1 for x in es), 0)
    same_as_plain(got, bs, caps, mem, checker=checker)
    assert stream_bytes(got[4], got[5], got[2], 0) == a + b
    # every stream with K = 1 (an empty index), empty streams, a batch of one stream
    for lengths in ([5, 16, 1, 15], [0, 0, 0], [0], [16 * 3 + 5], [7]):
        datas1, blobs1, entries1 = true_batch(checker, prose, 16, lengths=lengths, at=60_000)
        first, off = index_of(entries1)
        caps = roomy(datas1)
        for bs in (blobs1, [b""] * len(blobs1)):  # (and with no input bytes at all)
            capfd.readouterr()
            got = decode_call("resets", bs, caps, first=first if bs is blobs1 else None, off=off if bs is blobs1 else None, mem=mem)
            split = sum(1 for e in entries1 if e) if bs is blobs1 else 0
            assert line_of(capfd)[:2] == (len(bs), split)
            same_as_plain(got, bs, caps, mem)


# ---- 6. streams that are wrong, with a right index ----

@pytest.mark.parametrize("mem", ["host", "device"])
def test_streams_that_are_wrong(ta, checker, prose, mem, capfd):
    datas, blobs, entries = true_batch(checker, prose, 100, lengths=[150, 300, 40], at=30_000)
    assert len(entries[1]) == 2 and 150 <= len(blobs[1]) <= 400
    first, off = index_of(entries)
    caps = roomy(datas)
    # a three-segment stream cut behind every byte, inside a batch of three
    for cut in range(len(blobs[1])):
        bs = [blobs[0], blobs[1][:cut], blobs[2]]
        got = decode_call("resets", bs, caps, first=first, off=off, mem=mem)
        same_as_plain(got, bs, caps, mem, checker=checker if mem == "host" and cut % 7 == 3 else None)
    capfd.readouterr()
    # an offset out of the window in a middle segment
    w = TokenWriter(window=10, literal=8, extended=False, more=0)
    rng = random.Random(3)
    w.fill_to(8 * 30, rng)
    w.flush(), w.flush()
    w.fill_to(w.bit + 80, rng)
    w.match(1023, 5, check=False)
    w.fill_to(w.bit + 64, rng)
    w.flush(), w.flush()
    w.fill_to(w.bit + 8 * 20, rng)
    oob = w.blob()
    # the custom bit; a window above max_window_bits; no reset bit but a non-empty index
    custom = bytes([blobs[1][0] | 4]) + blobs[1][1:]
    plain_hdr = bytes([blobs[1][0] & ~1]) + blobs[1][2:]
    for what, blob, es, max_wbits, status in (("oob", oob, true_entries(oob), 15, OOB), ("custom", custom, entries[1], 15, INVALID_CONF),
                                              ("window", blobs[1], entries[1], 9, INVALID_CONF),
                                              ("window, exact", blobs[1], entries[1], 9 | 0x80, INVALID_CONF),
                                              ("no reset bit", plain_hdr, [x - 1 for x in entries[1]], 15, None)):
        bs = [blobs[0], blob, blobs[2]]
        f, o = index_of([entries[0], es, entries[2]])
        c = [max(len(x) * 16, 64) for x in bs]
        capfd.readouterr()
        got = decode_call("resets", bs, c, first=f, off=o, mem=mem, max_wbits=max_wbits)
        n, s, u, wh = line_of(capfd)
        assert (n, wh >= 1) == (3, True), what
        if max_wbits == 15:
            assert s == 1  # (stream 0 has one entry, stream 2 none)
        # (the checker as well where it can answer: its reference harness hands every custom-bit stream a window to start from, and
        # it knows no exact-window flag -- for those two the existing call alone is the yardstick)
        same_as_plain(got, bs, c, mem, max_wbits=max_wbits, checker=checker if what != "custom" and max_wbits < 0x80 else None)
        if status is not None:
            assert int(got[1][1]) == status, what


# ---- 7. scan edges ----

def test_stream_boundaries_at_the_scans_edges(ta, checker, prose, capfd):
    """N = 1: streams whose entry counts put the streams' boundaries on slots tile - 1, tile and tile + 1 of the scan over the closed rows."""
    from tamp_amd import _lib

    tile = _lib.RESETS_SCAN_TILE
    lengths = [tile, 0, 2, 1, 2, 2, 0, tile + 1, 2]
    datas, blobs, entries = true_batch(checker, prose, 1, lengths=lengths, at=80_000)
    first, off = index_of(entries)
    assert {tile - 1, tile, tile + 1} <= set(int(x) for x in first)
    caps = roomy(datas)
    for mem in ("host", "device"):
        capfd.readouterr()
        got = decode_call("resets", blobs, caps, first=first, off=off, mem=mem)
        split = sum(1 for e in entries if e)
        assert line_of(capfd) == (len(blobs), split, sum(len(e) + 1 for e in entries if e), len(blobs) - split)
        same_as_plain(got, blobs, caps, mem)
        for i, d in enumerate(datas):
            assert stream_bytes(got[4], got[5], got[2], i) == d, i


# ---- 8. the Python surface ----

def test_python_surface(ta, checker, prose, capfd):
    import torch

    from tamp_amd.batch import pack_streams

    interval = 1000
    datas, blobs, entries = true_batch(checker, prose, interval)
    want_first, want_off = index_of(entries)
    n_split = sum(1 for e in entries if e)
    flat, in_off, in_len = pack_streams(datas)
    dev = torch.device("cuda:0")
    dev_args = (torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(in_off.view(np.int64).copy()).to(dev),
                torch.from_numpy(in_len.view(np.int32).copy()).to(dev))
    for form, args in (("list", (datas,)), ("arrays", (flat, in_off, in_len)), ("tensors", dev_args)):
        res = ta.compress_batch(*args, dictionary_reset=True, reset_interval=interval, reset_index=True)
        torch.cuda.synchronize()
        assert res.streams() == blobs and isinstance(res.reset_index, ta.ResetIndex), form
        idx_first, idx_off = res.reset_index.first, res.reset_index.off
        if form == "tensors":
            assert idx_first.is_cuda and idx_off.is_cuda
            idx_first, idx_off = idx_first.cpu().numpy(), idx_off.cpu().numpy()
        assert list(idx_first) == list(want_first) and list(idx_off) == list(want_off), form
        assert ta.compress_batch(*args, dictionary_reset=True, reset_interval=interval).reset_index is None
        # ... and back, the sizes unknown and with one capacity for all
        for kw in ({}, dict(out_cap=max(len(d) for d in datas) + 1)):
            capfd.readouterr()
            if form == "tensors":
                comp_flat, comp_off, comp_len = pack_streams(res.streams())
                comp = (torch.from_numpy(comp_flat.copy()).to(dev), torch.from_numpy(comp_off.view(np.int64).copy()).to(dev),
                        torch.from_numpy(comp_len.view(np.int32).copy()).to(dev))
                back = ta.decompress_batch(*comp, reset_index=res.reset_index, **kw)
                torch.cuda.synchronize()
                assert back.out.is_cuda and (back.status.cpu().numpy() == INPUT_EXHAUSTED).all()
                assert [int(x) for x in back.in_consumed.cpu()] == [len(b) for b in blobs]
            else:
                back = ta.decompress_batch(res.streams(), reset_index=res.reset_index, **kw)
                assert (back.status == INPUT_EXHAUSTED).all() and [int(x) for x in back.in_consumed] == [len(b) for b in blobs]
            assert back.streams() == datas, (form, kw)
            assert line_of(capfd)[1] == n_split, (form, kw)
    # CUDA tensors end to end on a side stream: the compressor's slab is the decoder's input, tables made on the launch stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = ta.compress_batch(*dev_args, dictionary_reset=True, reset_interval=interval, reset_index=True, stream=side.cuda_stream)
    capfd.readouterr()
    back = ta.decompress_batch(res.out, res.out_off, res.out_len, reset_index=res.reset_index, stream=side.cuda_stream)
    side.synchronize()
    assert line_of(capfd)[1] == n_split
    assert res.streams() == blobs and back.streams() == datas and (back.status.cpu().numpy() == INPUT_EXHAUSTED).all()
    # an index of host arrays with device data, and the other way round
    host_idx = ta.ResetIndex(want_first, want_off)
    back = ta.decompress_batch(res.out, res.out_off, res.out_len, reset_index=host_idx)
    torch.cuda.synchronize()
    assert back.streams() == datas
    back = ta.decompress_batch(blobs, reset_index=res.reset_index)
    assert back.streams() == datas
