"""GPU tier: byte ranges written into reset-segmented streams (tamp_batch_write_ranges, ``write_ranges``; the kernels of
tamp_write_ranges_kernel.hpp, DESIGN.md 3.13 "Writing ranges").

The expectation is always a FRESH compress of the patched input through ``compress_batch(..., reset_interval=N, reset_index=True)``
-- streams and index byte for byte -- and the oracle's decoder on the new streams; where the C call is made by hand, every slab lies at
an odd offset inside a buffer of guard bytes and the whole buffer is compared."""
import ctypes as C
import random
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, OUTPUT_FULL, INPUT_EXHAUSTED, EXCESS_BITS, INVALID_CONF, BAD_ARGUMENT, BAD_INDEX = 0, 1, 2, -2, -3, -21, -22
GUARD = 0xA5
LINE = re.compile(r"\[tamp_amd resets\] write ranges: (\d+) writes, (\d+) units, (\d+) slices, (\d+) bytes staged$", re.M)


@pytest.fixture(scope="module")
def ta():
    import tamp_amd
    from tamp_amd import _lib

    _lib.load()  # raises if the native library is missing: no silent fallback
    return tamp_amd


@pytest.fixture(scope="module")
def prose():
    from tamp_amd import workloads as wl

    raw = wl.frozen_corpus("prose")
    assert len(raw) >= (1 << 20), "the frozen corpus (tests/golden/corpus_prose.txt.xz) is part of the tree"
    return (np.frombuffer(raw[: 1 << 20], dtype=np.uint8) & 0x7F).tobytes()  # (fits 7-bit literals)


@pytest.fixture(autouse=True)
def debug_line(monkeypatch):
    for k in ("TAMP_AMD_RANGES_SCRATCH_MB", "TAMP_AMD_DECODER"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TAMP_AMD_RESETS_DEBUG", "1")


def conf_kw(window=10, literal=8, extended=True, lazy=False):
    return dict(window=window, literal=literal, extended=extended, lazy_matching=lazy)


def streams_for(prose, N, count=64, seed=1):
    """Ragged streams of text-like and run-heavy 7-bit bytes, 0 to about 3 KiB: an empty one, one byte, exactly k N and k N + 1 first."""
    rng = random.Random(seed * 1000 + N)
    lens = [0, 1, 3 * N, 3 * N + 1, N, N - 1] + [rng.randrange(0, 3072) for _ in range(count - 6)]
    datas, at = [], 5000 * seed
    for j, n in enumerate(lens):
        if j % 3 == 2:  # run-heavy: runs of one byte between short pieces of text
            b = bytearray()
            while len(b) < n:
                b += bytes([rng.randrange(32, 127)]) * rng.randrange(1, 60) + prose[at : at + rng.randrange(0, 12)]
                at += 12
            datas.append(bytes(b[:n]))
        else:
            datas.append(prose[at : at + n])
            at += n
    return datas


def random_writes(datas, N, about=200, seed=2, top=0x7F, gap=None):
    """Disjoint writes of 1 .. 3 N bytes, in random order: [(stream, begin, bytes)]."""
    rng = random.Random(seed * 1000 + N)
    writes = []
    order = list(range(len(datas)))
    rng.shuffle(order)
    for i in order:
        pos, n = 0, len(datas[i])
        while len(writes) < about:
            pos += rng.randrange(0, N // 2 + 1 if gap is None else gap)
            ln = rng.randrange(1, 3 * N + 1)
            if pos + ln > n:
                break
            writes.append((i, pos, bytes(rng.randrange(0, top + 1) for _ in range(ln))))
            pos += ln
    rng.shuffle(writes)
    return writes


def patch(datas, writes):
    out = [bytearray(d) for d in datas]
    for i, begin, src in writes:
        assert begin + len(src) <= len(out[i])
        out[i][begin : begin + len(src)] = src
    return [bytes(b) for b in out]


_fresh = {}


def fresh(ta, datas, N, kw):
    """(streams, index) of a fresh compress (computed once per input and configuration, shared by the tests, never changed)."""
    key = (tuple(datas), N, tuple(sorted(kw.items())))
    if key not in _fresh:
        res = ta.compress_batch(list(datas), dictionary_reset=True, reset_interval=N, reset_index=True, **kw)
        assert (res.status == 0).all()
        _fresh[key] = (res.streams(), res.reset_index)
    return _fresh[key]


def np_of(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def write(ta, blobs, index, writes, **more):
    return ta.write_ranges(blobs, reset_index=index, stream_index=[w[0] for w in writes], begin=[w[1] for w in writes],
                           source=[w[2] for w in writes], **more)


def assert_same(ta, res, datas, writes, N, kw, skip=()):
    """The result against a fresh compress of the patched data: status, streams, index."""
    want_streams, want_index = fresh(ta, patch(datas, writes), N, kw)
    status = np_of(res.status)
    got = res.streams()
    off, first = np_of(res.reset_index.off).astype(np.uint32), np_of(res.reset_index.first).astype(np.uint64)
    assert (first == want_index.first).all() and res.reset_index.interval == N
    for i in range(len(datas)):
        if i in skip:
            continue
        assert int(status[i]) == OK, (i, int(status[i]))
        assert got[i] == want_streams[i], i
        a, b = int(first[i]), int(first[i + 1])
        assert (off[a:b] == want_index.off[a:b]).all(), i


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("literal", [7, 8])
@pytest.mark.parametrize("window", [8, 10, 12])
@pytest.mark.parametrize("N", [16, 100, 256])
def test_parity_matrix(ta, oracle, prose, N, window, literal, extended, lazy):
    kw = conf_kw(window, literal, extended, lazy)
    datas = streams_for(prose, N)
    writes = random_writes(datas, N)
    assert len(writes) >= 100  # (200 where the streams have room for them: 64 streams of 3 KiB at most)
    blobs, index = fresh(ta, datas, N, kw)
    res = write(ta, blobs, index, writes, lazy_matching=lazy)
    assert_same(ta, res, datas, writes, N, kw)
    patched = patch(datas, writes)
    for i, blob in enumerate(res.streams()):
        st, back, _ = oracle.decompress(blob, cap=len(patched[i]) + 8)
        assert st in (OK, INPUT_EXHAUSTED) and back == patched[i], i


EDGE_N = 64


def edge_batch(prose):
    return [prose[10_000 : 10_000 + 5 * EDGE_N + 20], prose[20_000 : 20_000 + 7 * EDGE_N], prose[30_000 : 30_000 + 9 * EDGE_N + 1], prose[40_000:40_010]]


@pytest.mark.parametrize("name", ["straddle", "one_closed_segment", "whole_stream", "last_byte_of_open", "first_byte", "five_segments",
                                  "whole_stream_of_full_segments", "open_segment_only"])
def test_edges(ta, prose, name):
    N, kw = EDGE_N, conf_kw()
    datas = edge_batch(prose)
    fill = lambda n: bytes((37 * j + 11) & 0x7F for j in range(n))  # noqa: E731
    writes = {
        "straddle": [(0, 2 * N - 1, b"\x01\x02")],                       # k N - 1 .. k N
        "one_closed_segment": [(0, N, fill(N))],
        "whole_stream": [(0, 0, fill(len(datas[0])))],
        "last_byte_of_open": [(0, len(datas[0]) - 1, b"Z")],
        "first_byte": [(2, 0, b"Q")],
        "five_segments": [(2, N + 5, fill(4 * N - 3))],                  # segments 1 .. 5
        "whole_stream_of_full_segments": [(1, 0, fill(7 * N))],          # the open segment holds exactly N bytes
        "open_segment_only": [(3, 2, b"abc")],                           # a stream without resets
    }[name]
    blobs, index = fresh(ta, datas, N, kw)
    assert_same(ta, write(ta, blobs, index, writes), datas, writes, N, kw)


def test_many_writes_in_one_segment_are_one_unit(ta, prose, capfd):
    N, kw = EDGE_N, conf_kw()
    datas = edge_batch(prose)
    writes = [(0, 2 * N + j, bytes([65 + j % 26])) for j in range(0, N, 2)]  # 32 one-byte writes inside segment 2
    blobs, index = fresh(ta, datas, N, kw)
    capfd.readouterr()
    res = write(ta, blobs, index, writes)
    m = LINE.search(capfd.readouterr().err)
    assert m and (int(m[1]), int(m[2]), int(m[3]), int(m[4])) == (len(writes), 1, 1, N)
    assert_same(ta, res, datas, writes, N, kw)
    # two writes in neighbouring segments and one in another stream: three units
    writes = [(0, N - 1, b"a"), (0, N, b"b"), (1, 0, b"c")]
    capfd.readouterr()
    res = write(ta, blobs, index, writes)
    m = LINE.search(capfd.readouterr().err)
    assert m and (int(m[1]), int(m[2])) == (3, 3)
    assert_same(ta, res, datas, writes, N, kw)


def test_writes_of_no_bytes(ta, prose, capfd):
    """Zero-length writes only, anywhere: the streams equal the inputs and nothing is a unit; and no writes at all."""
    N, kw = EDGE_N, conf_kw()
    datas = edge_batch(prose)
    blobs, index = fresh(ta, datas, N, kw)
    for writes in ([(0, 0, b""), (0, 5, b""), (2, 1 << 40, b""), (3, 3, b"")], []):
        capfd.readouterr()
        res = write(ta, blobs, index, writes)
        m = LINE.search(capfd.readouterr().err)
        assert m and int(m[2]) == 0
        assert (np_of(res.status) == 0).all() and res.streams() == blobs
        assert (np_of(res.reset_index.off) == index.off).all()


def layout(caps):
    """Slabs at odd offsets with guard bytes between them: -> (out_off uint64, total)."""
    off, at = [], 1
    for j, c in enumerate(caps):
        at |= 1
        off.append(at)
        at += int(c) + 3 + j % 5
    return np.array(off, dtype=np.uint64), at + 8


def c_call(blobs, first, off, N, writes, kw, *, out_cap=None, mem="host", max_wbits=15, new_off=True):
    """One tamp_batch_write_ranges call on hand-laid tables, the writes AS GIVEN (no sort): -> (rc, status, out_len, out, out_off,
    out_cap, new_reset_off); poisoned result tables, guard bytes around every slab."""
    from tamp_amd import _lib
    from tamp_amd.batch import _write_bound, pack_streams

    lib = _lib.load()
    n = len(blobs)
    flat, in_off, in_len = pack_streams(blobs)
    if flat.size == 0:
        flat = np.zeros(1, np.uint8)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    off = np.ascontiguousarray(off, dtype=np.uint32)
    if out_cap is None:
        out_cap = np.maximum(_write_bound(first[1:] - first[:-1], N, kw["literal"]), in_len.astype(np.uint64))
    out_cap = np.ascontiguousarray(out_cap, dtype=np.uint32)
    out_off, total = layout(out_cap)
    out = np.full(total, GUARD, dtype=np.uint8)
    out_len, status = np.full(n, 0xDEAD, dtype=np.uint32), np.full(n, 99, dtype=np.int8)
    w_stream = np.array([w[0] for w in writes] or [0], dtype=np.uint32)[: len(writes)]
    w_begin = np.array([w[1] for w in writes] or [0], dtype=np.uint64)[: len(writes)]
    w_len = np.array([len(w[2]) for w in writes] or [0], dtype=np.uint32)[: len(writes)]
    src = np.frombuffer(b"".join(w[2] for w in writes) + b"\0", dtype=np.uint8).copy()
    src_off = (np.cumsum(w_len.astype(np.uint64)) - w_len.astype(np.uint64)).astype(np.uint64)
    new = np.full(max(len(off), 1), 0xDEADBEEF, dtype=np.uint32)
    conf = _lib.TampAmdConf(kw["window"], kw["literal"], 0, int(kw["extended"]), 1, int(kw["lazy_matching"]), 0)
    tables = [flat, in_off, in_len, first, off if len(off) else np.zeros(1, np.uint32), w_stream, w_begin, w_len, src, src_off, out, out_off, out_cap,
              out_len, status, new]
    if mem == "host":
        p = [a.ctypes.data_as(C.c_void_p) for a in tables]
        rc = lib.tamp_batch_write_ranges(C.byref(conf), max_wbits, p[0], p[1], p[2], p[3], p[4] if len(off) else None, N, p[5], p[6], p[7], p[8], p[9],
                                         p[10], p[11], p[12], p[13], p[14], p[15] if new_off and len(off) else None, n, len(writes),
                                         _lib.MEM_HOST, 0, None)
        return rc, status, out_len, out, out_off, out_cap, new[: len(off)]
    import torch

    dev = torch.device("cuda:0")
    views = [None, np.int64, np.int32, np.int64, np.int32, np.int32, np.int64, np.int32, None, np.int64, None, np.int64, np.int32, np.int32, None, np.int32]
    t = [torch.from_numpy(a.copy() if v is None else a.view(v).copy()).to(dev) for a, v in zip(tables, views)]
    torch.cuda.synchronize()
    p = [C.c_void_p(x.data_ptr()) for x in t]
    rc = lib.tamp_batch_write_ranges(C.byref(conf), max_wbits, p[0], p[1], p[2], p[3], p[4] if len(off) else None, N, p[5], p[6], p[7], p[8], p[9],
                                     p[10], p[11], p[12], p[13], p[14], p[15] if new_off and len(off) else None, n, len(writes),
                                     _lib.MEM_DEVICE, 0, None)
    torch.cuda.synchronize()
    return (rc, t[14].cpu().numpy(), t[13].cpu().numpy().view(np.uint32), t[10].cpu().numpy(), out_off, out_cap,
            t[15].cpu().numpy().view(np.uint32)[: len(off)])


def check_c(res, want_streams, want_off, first, *, failing=()):
    """The WHOLE output buffer: every good stream's bytes where they belong, guard bytes everywhere else -- in front of out_off[i], at
    and behind out_off[i] + out_cap[i]; what lies INSIDE a failing stream's slab is its own.  ``failing``: {stream: status}."""
    rc, status, out_len, out, out_off, out_cap, new = res
    assert rc == 0
    expect = np.full(len(out), GUARD, dtype=np.uint8)
    same = np.ones(len(out), dtype=bool)
    for i, blob in enumerate(want_streams):
        o = int(out_off[i])
        if i in failing:
            assert (int(status[i]), int(out_len[i])) == (failing[i], 0), (i, int(status[i]), int(out_len[i]))
            same[o : o + int(out_cap[i])] = False
            continue
        assert (int(status[i]), int(out_len[i])) == (OK, len(blob)), (i, int(status[i]), int(out_len[i]), len(blob))
        expect[o : o + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        a, b = int(first[i]), int(first[i + 1])
        assert (new[a:b] == want_off[a:b]).all(), i
    assert (out[same] == expect[same]).all(), np.flatnonzero(same & (out != expect))[:10]


STATUS_N = 64


def status_batch(ta, prose, kw=None):
    kw = kw or conf_kw()
    datas = [prose[50_000 + 1000 * j : 50_000 + 1000 * j + n] for j, n in enumerate([5 * STATUS_N + 9, 4 * STATUS_N, 0, 3 * STATUS_N + 30, 700, 6 * STATUS_N + 1])]
    blobs, index = fresh(ta, datas, STATUS_N, kw)
    good = [(0, 3, b"abc"), (1, STATUS_N - 2, b"wxyz"), (3, 2 * STATUS_N, b"0123456789"), (4, 100, b"k" * 200), (5, 6 * STATUS_N, b"!")]
    return datas, blobs, index, good


def one_fails(ta, prose, writes, victim, code, *, mem="host", blobs=None, first=None, off=None, kw=None, out_cap=None, N=STATUS_N, max_wbits=15,
              call_kw=None):
    """``writes`` (sorted here unless they are meant not to be) fail stream ``victim`` with ``code``; every other stream succeeds and
    matches a fresh compress of its patched data, behind intact guards."""
    kw = kw or conf_kw()
    datas, b0, index, _ = status_batch(ta, prose, kw)
    blobs = b0 if blobs is None else blobs
    applied = [w for w in writes if w[0] != victim]
    want_streams, want_index = fresh(ta, patch(datas, applied), STATUS_N, kw)
    res = c_call(blobs, index.first if first is None else first, index.off if off is None else off, N, writes, call_kw or kw, out_cap=out_cap, mem=mem,
                 max_wbits=max_wbits)
    check_c(res, want_streams, want_index.off, index.first, failing={victim: code})
    return res


@pytest.mark.parametrize("mem", ["host", "device"])
def test_status_end_of_stream(ta, prose, mem):
    datas, blobs, index, good = status_batch(ta, prose)
    n0 = len(datas[0])
    srt = lambda ws: sorted(ws, key=lambda w: (w[0], w[1]))  # noqa: E731
    one_fails(ta, prose, srt(good + [(0, n0 - 1, b"ab")]), 0, INPUT_EXHAUSTED, mem=mem)                 # one byte past the end
    one_fails(ta, prose, srt(good + [(0, n0, b"a")]), 0, INPUT_EXHAUSTED, mem=mem)                      # begins at the end
    one_fails(ta, prose, srt(good + [(0, n0 + 1000 * STATUS_N, b"a")]), 0, INPUT_EXHAUSTED, mem=mem)    # begins far behind it
    one_fails(ta, prose, srt(good + [(0, (1 << 64) - 1, b"ab")]), 0, INPUT_EXHAUSTED, mem=mem)          # the top of 64 bits
    one_fails(ta, prose, srt(good + [(2, 0, b"a")]), 2, INPUT_EXHAUSTED, mem=mem)                       # into an empty stream
    # a stream of exactly k N bytes: its last byte is written, the byte behind it is not
    datas1 = len(datas[1])
    one_fails(ta, prose, srt([w for w in good if w[0] != 1] + [(1, datas1 - 1, b"ab")]), 1, INPUT_EXHAUSTED, mem=mem)
    res = c_call(blobs, index.first, index.off, STATUS_N, srt(good + [(1, datas1 - 1, b"a")]), conf_kw(), mem=mem)
    want_streams, want_index = fresh(ta, patch(datas, good + [(1, datas1 - 1, b"a")]), STATUS_N, conf_kw())
    check_c(res, want_streams, want_index.off, index.first)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_status_order_and_overlap(ta, prose, mem):
    """Through the C call, which takes the writes as they come: out of order or overlapping is TAMP_AMD_BAD_ARGUMENT for that stream."""
    datas, blobs, index, good = status_batch(ta, prose)
    srt = lambda ws: sorted(ws, key=lambda w: (w[0], w[1]))  # noqa: E731
    base = srt(good)
    assert base[2][0] == 3
    one_fails(ta, prose, base[:3] + [(3, 5, b"abc")] + base[3:], 3, BAD_ARGUMENT, mem=mem)  # a begin in front of the predecessor's
    one_fails(ta, prose, srt(good + [(4, 299, b"xy")]), 4, BAD_ARGUMENT, mem=mem)  # begins on the predecessor's last byte
    # a write of no bytes stands in the order like any other: inside its predecessor it fails the stream
    ws = srt(good)
    at = ws.index((4, 100, b"k" * 200))
    one_fails(ta, prose, ws[: at + 1] + [(4, 150, b"")] + ws[at + 1 :], 4, BAD_ARGUMENT, mem=mem)
    # streams out of order: the write that steps back fails ITS stream
    ws = srt(good)
    one_fails(ta, prose, ws[1:2] + ws[0:1] + ws[2:], 0, BAD_ARGUMENT, mem=mem)
    # touching writes are in order
    ws = srt(good + [(4, 300, b"zz"), (4, 98, b"yy")])
    res = c_call(blobs, index.first, index.off, STATUS_N, ws, conf_kw(), mem=mem)
    want_streams, want_index = fresh(ta, patch(datas, ws), STATUS_N, conf_kw())
    check_c(res, want_streams, want_index.off, index.first)
    # a write for a stream there is none of is ignored, wherever it stands
    res = c_call(blobs, index.first, index.off, STATUS_N, srt(good) + [(len(datas), 0, b"abc"), (77, 5, b"")], conf_kw(), mem=mem)
    want_streams, want_index = fresh(ta, patch(datas, good), STATUS_N, conf_kw())
    check_c(res, want_streams, want_index.off, index.first)


def test_unsorted_cuda_tables(ta, prose):
    """CUDA tables of a CUDA call are passed as they are: the device check answers for them."""
    import torch

    datas, blobs, index, good = status_batch(ta, prose)
    dev = torch.device("cuda:0")
    flat, off, ln = ta.pack_streams(blobs)
    t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev).to(dt)  # noqa: E731
    writes = sorted(good, key=lambda w: (w[0], w[1]))
    writes = writes[1:2] + writes[0:1] + writes[2:]  # stream 1 in front of stream 0
    lens = [len(w[2]) for w in writes]
    res = ta.write_ranges(torch.from_numpy(flat.copy()).to(dev), t(off, torch.int64), t(ln, torch.int32), reset_index=index,
                          stream_index=t([w[0] for w in writes], torch.int32), begin=t([w[1] for w in writes], torch.int64),
                          source=torch.from_numpy(np.frombuffer(b"".join(w[2] for w in writes), dtype=np.uint8).copy()).to(dev),
                          source_off=t(np.cumsum(lens) - np.array(lens), torch.int64), length=t(lens, torch.int32), window=10, literal=8, extended=True)
    torch.cuda.synchronize()
    status = np_of(res.status)
    assert int(status[0]) == BAD_ARGUMENT and int(np_of(res.out_len)[0]) == 0
    assert_same(ta, res, datas, [w for w in good if w[0] != 0], STATUS_N, conf_kw(), skip={0})


@pytest.mark.parametrize("mem", ["host", "device"])
def test_status_conf_and_header(ta, prose, mem):
    datas, blobs, index, good = status_batch(ta, prose)
    srt = lambda ws: sorted(ws, key=lambda w: (w[0], w[1]))  # noqa: E731
    # conf's window or literal differ from the header: every WRITTEN stream fails, the stream no write touches is copied
    for other in (conf_kw(window=11), conf_kw(literal=7), conf_kw(extended=False)):
        res = c_call(blobs, index.first, index.off, STATUS_N, srt(good), other, mem=mem)
        rc, status, out_len, out, out_off, out_cap, new = res
        assert rc == 0 and [int(s) for s in status] == [INVALID_CONF, INVALID_CONF, OK, INVALID_CONF, INVALID_CONF, INVALID_CONF]
        assert int(out_len[2]) == len(blobs[2]) and out[int(out_off[2]) : int(out_off[2]) + len(blobs[2])].tobytes() == blobs[2]
    # a stream without the reset bit (compressed without resets), in the batch's place of stream 3; a second header byte that is not zero
    plain = ta.compress_batch([datas[3]], **conf_kw()).streams()[0]
    for bad in (plain, blobs[3][:1] + b"\x01" + blobs[3][2:], blobs[3][:1], bytes([blobs[3][0] | 4]) + blobs[3][1:]):
        one_fails(ta, prose, srt(good), 3, INVALID_CONF, mem=mem, blobs=blobs[:3] + [bad] + blobs[4:])
    # a window above the call's limit
    res = c_call(blobs, index.first, index.off, STATUS_N, srt(good), conf_kw(), mem=mem, max_wbits=9)
    assert res[0] == 0 and [int(s) for s in res[1]] == [INVALID_CONF, INVALID_CONF, OK, INVALID_CONF, INVALID_CONF, INVALID_CONF]


@pytest.mark.parametrize("mem", ["host", "device"])
def test_status_index(ta, prose, mem):
    datas, blobs, index, good = status_batch(ta, prose)
    srt = lambda ws: sorted(ws, key=lambda w: (w[0], w[1]))  # noqa: E731
    first, off = index.first, index.off
    # stream 0 is written in segment 0 only; its entries 0 (the end of segment 0) and 3 (between the untouched segments 3 and 4)
    a = int(first[0])
    for delta in (1, -1):
        moved = off.copy()
        moved[a] = int(off[a]) + delta
        one_fails(ta, prose, srt(good), 0, BAD_INDEX, mem=mem, off=moved)
    # the same damage on an untouched segment is not noticed: the bytes between the entries are copied as they stand, so the stream is
    # what a fresh compress makes, and the new index carries the displacement
    moved = off.copy()
    moved[a + 3] += np.uint32(1)
    res = c_call(blobs, first, moved, STATUS_N, srt(good), conf_kw(), mem=mem)
    want_streams, want_index = fresh(ta, patch(datas, good), STATUS_N, conf_kw())
    shifted = want_index.off.copy()
    shifted[a + 3] += np.uint32(1)
    check_c(res, want_streams, shifted, first)
    # ... unless the entry leaves the stream or the order: memory safety is checked on every segment
    for value in (0xFFFFFFFF, 0, int(off[a + 2])):
        moved = off.copy()
        moved[a + 3] = value
        one_fails(ta, prose, srt(good), 0, BAD_INDEX, mem=mem, off=moved)
    # the wrong interval: the touched closed segments do not decode to it (streams 2 and 4 have no closed segment to tell by and are
    # written at places both intervals agree on or not at all)
    for wrong in (STATUS_N - 1, STATUS_N - 4, STATUS_N + 1):
        res = c_call(blobs, first, off, wrong, srt([w for w in good if w[0] not in (4, 5)]), conf_kw(), mem=mem)
        assert res[0] == 0 and [int(s) for s in res[1]][:2] == [BAD_INDEX, BAD_INDEX] and int(res[1][3]) == BAD_INDEX, [int(s) for s in res[1]]
        assert [int(s) for s in res[1]][4:] == [OK, OK] and int(res[1][2]) == OK
    # rows of reset_first that are no running sum: the stream's own rows decide
    broken = first.copy()
    broken[4] = first[5] + np.uint64(1)  # stream 3: fine in front; stream 4: decreasing
    res = c_call(blobs, broken, off, STATUS_N, srt(good), conf_kw(), mem=mem)
    assert res[0] == 0 and int(res[1][4]) == BAD_INDEX and int(res[2][4]) == 0


@pytest.mark.parametrize("mem", ["host", "device"])
def test_status_excess_bits_and_room(ta, prose, mem):
    kw7 = conf_kw(literal=7)
    datas, blobs, index, good = status_batch(ta, prose, kw7)
    srt = lambda ws: sorted(ws, key=lambda w: (w[0], w[1]))  # noqa: E731
    for src in (b"\x80", b"ab\xffcd", bytes(40) + b"\x80" + bytes(40)):
        one_fails(ta, prose, srt([w for w in good if w[0] != 3] + [(3, STATUS_N + 7, src)]), 3, EXCESS_BITS, mem=mem, kw=kw7)
    # the first rule that applies: a write behind the end goes before the source's bytes
    one_fails(ta, prose, srt([w for w in good if w[0] != 3] + [(3, len(datas[3]) - 1, b"\x80\x80")]), 3, INPUT_EXHAUSTED, mem=mem, kw=kw7)
    # and of two failing writes the lower one decides
    one_fails(ta, prose, srt([w for w in good if w[0] != 3] + [(3, 0, b"\x80"), (3, len(datas[3]), b"a")]), 3, EXCESS_BITS, mem=mem, kw=kw7)
    one_fails(ta, prose, srt([w for w in good if w[0] != 3] + [(3, 0, b"a"), (3, 9, b"\x80"), (3, len(datas[3]), b"a")]), 3, EXCESS_BITS, mem=mem, kw=kw7)
    # room: one byte short of the new length is TAMP_OUTPUT_FULL, exact room succeeds -- for a written stream and for a copied one
    kw = conf_kw()
    datas, blobs, index, good = status_batch(ta, prose, kw)
    want_streams, want_index = fresh(ta, patch(datas, good), STATUS_N, kw)
    exact = np.array([len(b) for b in want_streams], dtype=np.uint32)
    check_c(c_call(blobs, index.first, index.off, STATUS_N, srt(good), kw, out_cap=exact, mem=mem), want_streams, want_index.off, index.first)
    for victim in (0, 2, 5):
        short = exact.copy()
        short[victim] -= 1
        res = c_call(blobs, index.first, index.off, STATUS_N, srt(good), kw, out_cap=short, mem=mem)
        check_c(res, want_streams, want_index.off, index.first, failing={victim: OUTPUT_FULL})


@pytest.mark.parametrize("mem", ["host", "device"])
def test_untouched_data_stays_untouched(ta, prose, mem):
    """Streams with no write are identical; in written streams every untouched segment's compressed bytes equal the input's, span by
    span through both indexes; nothing is written outside the slabs (check_c compares the whole guard-filled buffer)."""
    N, kw = 100, conf_kw()
    datas = streams_for(prose, N, count=24, seed=3)
    writes = [w for w in random_writes(datas, N, about=60, seed=4, gap=8 * N) if w[0] % 3 != 0]  # every third stream has no write
    writes.sort(key=lambda w: (w[0], w[1]))
    blobs, index = fresh(ta, datas, N, kw)
    res = c_call(blobs, index.first, index.off, N, writes, kw, mem=mem)
    want_streams, want_index = fresh(ta, patch(datas, writes), N, kw)
    check_c(res, want_streams, want_index.off, index.first)
    rc, status, out_len, out, out_off, out_cap, new = res
    touched = {i: set() for i in range(len(datas))}
    for i, begin, src in writes:
        touched[i].update(range(begin // N, (begin + len(src) - 1) // N + 1))
    kept = 0
    for i in range(len(datas)):
        got = out[int(out_off[i]) : int(out_off[i]) + int(out_len[i])].tobytes()
        if not touched[i]:
            assert got == blobs[i], i
            continue
        a, b = int(index.first[i]), int(index.first[i + 1])
        old = [2] + [int(x) for x in index.off[a:b]] + [len(blobs[i])]
        cur = [2] + [int(x) for x in new[a:b]] + [len(got)]
        assert got[:2] == blobs[i][:2]
        for k in range(b - a + 1):
            if k not in touched[i]:
                assert got[cur[k] : cur[k + 1]] == blobs[i][old[k] : old[k + 1]], (i, k)
                kept += 1
    assert kept > 50


def test_memory_kinds_streams_and_found_index(ta, prose):
    """Lists of bytes, the numpy triple and the CUDA-tensor triple give the same result; a side stream works; an index that
    ``index_resets`` found on the blobs works as the compressor's own does."""
    import torch

    N, kw = 100, conf_kw(window=12, literal=7)
    datas = streams_for(prose, N, count=32, seed=5)
    writes = random_writes(datas, N, about=80, seed=6)
    blobs, index = fresh(ta, datas, N, kw)
    lens = np.array([len(w[2]) for w in writes], dtype=np.uint64)
    flat_src = np.frombuffer(b"".join(w[2] for w in writes), dtype=np.uint8).copy()
    tables = dict(stream_index=[w[0] for w in writes], begin=[w[1] for w in writes])
    a = write(ta, blobs, index, writes)
    assert_same(ta, a, datas, writes, N, kw)
    flat, off, ln = ta.pack_streams(blobs)
    b = ta.write_ranges(flat, off, ln, reset_index=index, source=flat_src, source_off=np.cumsum(lens) - lens, length=lens, **tables)
    assert_same(ta, b, datas, writes, N, kw)
    dev = torch.device("cuda:0")
    t = lambda x, dt: torch.from_numpy(np.asarray(x).astype(np.int64)).to(dev).to(dt)  # noqa: E731
    d_flat, d_off, d_len = torch.from_numpy(flat.copy()).to(dev), t(off, torch.int64), t(ln, torch.int32)
    more = dict(window=12, literal=7, extended=True)
    c = ta.write_ranges(d_flat, d_off, d_len, reset_index=index, source=[w[2] for w in writes], **tables, **more)
    torch.cuda.synchronize()
    assert_same(ta, c, datas, writes, N, kw)
    side = torch.cuda.Stream()
    d = ta.write_ranges(d_flat, d_off, d_len, reset_index=index, source=torch.from_numpy(flat_src).to(dev), source_off=np.cumsum(lens) - lens,
                        length=lens, stream=side.cuda_stream, **tables, **more)
    side.synchronize()
    assert_same(ta, d, datas, writes, N, kw)
    with pytest.raises(ValueError, match="required with CUDA tensors"):
        ta.write_ranges(d_flat, d_off, d_len, reset_index=index, source=[w[2] for w in writes], **tables)
    scan = ta.index_resets(blobs)
    e = write(ta, blobs, ta.ResetIndex(scan.index.first, scan.index.off, N), writes)
    assert_same(ta, e, datas, writes, N, kw)


def test_slices(ta, prose, capfd, monkeypatch):
    """A scratch budget of 1 MiB: the same batch takes several slices of whole streams, the result is identical."""
    N, kw = 16, conf_kw()
    datas = streams_for(prose, N, count=160, seed=7)
    datas = [d if len(d) > 1500 else (d + prose[200_000 + 3000 * j : 200_000 + 3000 * j + 2500]) for j, d in enumerate(datas)]
    fill = lambda n, j: bytes((j + 31 * x) & 0x7F for x in range(n))  # noqa: E731
    writes = [(i, 0, fill(len(d), i)) for i, d in enumerate(datas) if i % 5 != 4]  # whole streams: every segment is a unit
    writes += [(i, 7, b"xyz") for i in range(4, len(datas), 5)]
    blobs, index = fresh(ta, datas, N, kw)
    capfd.readouterr()
    one = write(ta, blobs, index, writes)
    m = LINE.search(capfd.readouterr().err)
    assert m and int(m[3]) == 1
    units = int(m[2])
    assert units > 12_000
    monkeypatch.setenv("TAMP_AMD_RANGES_SCRATCH_MB", "1")
    capfd.readouterr()
    res = write(ta, blobs, index, writes)
    m = LINE.search(capfd.readouterr().err)
    assert m and int(m[2]) == units and int(m[3]) >= 2, m and m[0]
    assert res.streams() == one.streams() and (np_of(res.reset_index.off) == np_of(one.reset_index.off)).all()
    assert_same(ta, res, datas, writes, N, kw)
    import torch

    dev = torch.device("cuda:0")
    flat, off, ln = ta.pack_streams(blobs)
    t = lambda x, dt: torch.from_numpy(np.asarray(x).astype(np.int64)).to(dev).to(dt)  # noqa: E731
    capfd.readouterr()
    dres = ta.write_ranges(torch.from_numpy(flat.copy()).to(dev), t(off, torch.int64), t(ln, torch.int32), reset_index=index,
                           stream_index=[w[0] for w in writes], begin=[w[1] for w in writes], source=[w[2] for w in writes], window=10, literal=8,
                           extended=True)
    torch.cuda.synchronize()
    m = LINE.search(capfd.readouterr().err)
    assert m and int(m[3]) >= 2
    assert dres.streams() == one.streams()


def test_round_trip_with_the_sibling_calls(ta, prose):
    N, kw = 100, conf_kw()
    datas = streams_for(prose, N, count=32, seed=8)
    writes = random_writes(datas, N, about=60, seed=9)
    blobs, index = fresh(ta, datas, N, kw)
    res = write(ta, blobs, index, writes)
    assert (np_of(res.status) == 0).all()
    new = res.streams()
    back = ta.read_ranges(new, reset_index=res.reset_index, stream_index=[w[0] for w in writes], begin=[w[1] for w in writes],
                          length=[len(w[2]) for w in writes])
    assert (np_of(back.status) == 0).all() and back.ranges() == [w[2] for w in writes]
    patched = patch(datas, writes)
    whole = ta.decompress_batch(new, out_cap=3200, reset_index=res.reset_index)
    assert [whole.stream(i) for i in range(len(datas))] == patched
    # and a second round of writes on the result, with its index
    again = random_writes(patched, N, about=60, seed=10)
    res2 = write(ta, new, res.reset_index, again)
    assert_same(ta, res2, patched, again, N, kw)
