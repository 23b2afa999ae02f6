"""GPU tier: bytes appended to reset-segmented streams, the grid kept (tamp_batch_append, ``append_batch``; the kernels of
tamp_append_kernel.hpp, DESIGN.md 3.13 "Appending").

The expectation is always a FRESH ``compress_batch(old + appended, dictionary_reset=True, reset_interval=N, reset_index=True)`` --
streams and index byte for byte, entry for entry up to ``first[n]`` -- and the oracle's decoder on every new stream; never the call's
own output.  Where the C call is made by hand, every slab lies at an odd offset inside a buffer of guard bytes and the whole buffer
is compared."""
import ctypes as C
import random
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, OUTPUT_FULL, INPUT_EXHAUSTED, EXCESS_BITS, INVALID_CONF, BAD_ARGUMENT, BAD_INDEX = 0, 1, 2, -2, -3, -21, -22
GUARD = 0xA5
LINE = re.compile(r"\[tamp_amd resets\] append: (\d+) appends, (\d+) units, (\d+) slices, (\d+) bytes staged$", re.M)


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


def masked(b, literal):
    return bytes(np.frombuffer(b, dtype=np.uint8) & ((1 << literal) - 1)) if literal < 7 else b


def streams_for(prose, N, count=64, seed=1, literal=8):
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
    return [masked(d, literal) for d in datas]


def open_size(n, N):
    """Decoded bytes of the open segment of a fresh stream of n bytes: the last of ceil(n / N) segments (N for a full one)."""
    return n - (max(1, -(-n // N)) - 1) * N


def sources_for(prose, datas, N, seed=2, literal=8, at=400_000):
    """What each stream receives: around the open segment's room -- 0, 1, N - m - 1, N - m, N - m + 1, N, 3 N + 1 -- for the first
    42 streams in turn, random lengths up to 3 N behind them."""
    rng = random.Random(seed * 1000 + N)
    out = []
    for i, d in enumerate(datas):
        m = open_size(len(d), N)
        L = [0, 1, N - m - 1, N - m, N - m + 1, N, 3 * N + 1][i % 7] if i < 42 else rng.randrange(0, 3 * N + 1)
        if L < 0:
            L = rng.randrange(0, 3 * N + 1)
        out.append(masked(prose[at : at + L], literal))
        at += L + 3
    return out


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


def on_device(ta, blobs):
    import torch

    dev = torch.device("cuda:0")
    flat, off, ln = ta.pack_streams(blobs)
    t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev).to(dt)  # noqa: E731
    return torch.from_numpy(flat.copy() if flat.size else np.zeros(1, np.uint8)).to(dev), t(off, torch.int64), t(ln, torch.int32)


def assert_same(ta, res, news, N, kw, skip=()):
    """The result against a fresh compress of old + appended: status, streams, the index entry for entry up to first[n]."""
    want_streams, want_index = fresh(ta, news, N, kw)
    status = np_of(res.status)
    got = res.streams()
    off, first = np_of(res.reset_index.off).view(np.uint32), np_of(res.reset_index.first).astype(np.uint64)
    if not skip:
        assert (first == want_index.first).all() and res.reset_index.interval == N
        assert (off[: int(first[-1])] == want_index.off[: int(first[-1])]).all()
    for i in range(len(news)):
        if i in skip:
            continue
        assert int(status[i]) == OK, (i, int(status[i]))
        assert got[i] == want_streams[i], i
        a, b = int(first[i]), int(first[i + 1])
        wa, wb = int(want_index.first[i]), int(want_index.first[i + 1])
        assert (off[a:b] == want_index.off[wa:wb]).all(), i


def oracle_decodes(oracle, blobs, news):
    for i, blob in enumerate(blobs):
        st, back, _ = oracle.decompress(blob, cap=len(news[i]) + 8)
        assert st in (OK, INPUT_EXHAUSTED) and back == news[i], i


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("window,literal,extended,lazy", [(10, 8, True, False), (8, 7, True, False), (10, 8, False, False), (9, 8, True, True),
                                                          (15, 5, True, False)])
@pytest.mark.parametrize("N", [16, 100, 1024])
def test_parity_matrix(ta, oracle, prose, N, window, literal, extended, lazy, mem):
    import torch

    kw = conf_kw(window, literal, extended, lazy)
    datas = streams_for(prose, N, literal=literal)
    srcs = sources_for(prose, datas, N, literal=literal)
    assert {len(s) for s in srcs[:42]} >= {0, 1, N, 3 * N + 1}
    news = [d + s for d, s in zip(datas, srcs)]
    blobs, index = fresh(ta, datas, N, kw)
    if mem == "host":
        res = ta.append_batch(blobs, reset_index=index, source=srcs, lazy_matching=lazy)
    else:
        res = ta.append_batch(*on_device(ta, blobs), reset_index=index, source=srcs, **kw)
        torch.cuda.synchronize()
    assert_same(ta, res, news, N, kw)
    oracle_decodes(oracle, res.streams(), news)


def test_chains_on_the_device(ta, oracle, prose):
    """Three appends in a row on CUDA tensors, each on the previous result's slabs and index as they stand (spare entries behind
    first[n] included); after each the sibling calls take that index."""
    import torch

    N, kw = 100, conf_kw()
    datas = streams_for(prose, N, count=32, seed=3)
    blobs, index = fresh(ta, datas, N, kw)
    data, off, ln = on_device(ta, blobs)
    more = dict(window=10, literal=8, extended=True)
    for step in range(3):
        srcs = sources_for(prose, datas, N, seed=10 + step, at=500_000 + 40_000 * step)
        res = ta.append_batch(data, off, ln, reset_index=index, source=srcs, **more)
        olds, datas = datas, [d + s for d, s in zip(datas, srcs)]
        torch.cuda.synchronize()
        assert_same(ta, res, datas, N, kw)
        oracle_decodes(oracle, res.streams(), datas)
        data, off, ln, index = res.out, res.out_off, res.out_len, res.reset_index
        assert int(np_of(index.off).size) >= int(np_of(index.first)[-1])
        # ranges that straddle the old end
        begin = [max(len(o) - 7, 0) for o in olds]
        back = ta.read_ranges(data, off, ln, reset_index=index, stream_index=list(range(len(datas))), begin=begin, length=[20] * len(datas))
        torch.cuda.synchronize()
        assert back.ranges() == [d[b : b + 20] for d, b in zip(datas, begin)]
        whole = ta.decompress_batch(data, off, ln, out_cap=16_000, reset_index=index)
        torch.cuda.synchronize()
        assert [whole.stream(i) for i in range(len(datas))] == datas
        writes = [(i, len(d) // 2, b"#!#") for i, d in enumerate(datas) if len(d) >= 8]
        w = ta.write_ranges(data, off, ln, reset_index=index, stream_index=[x[0] for x in writes], begin=[x[1] for x in writes],
                            source=[x[2] for x in writes], **more)
        torch.cuda.synchronize()
        patched = [bytearray(d) for d in datas]
        for i, at, src in writes:
            patched[i][at : at + 3] = src
        want_streams, want_index = fresh(ta, [bytes(p) for p in patched], N, kw)
        assert (np_of(w.status) == 0).all() and w.streams() == want_streams
        n_entries = int(want_index.first[-1])
        assert (np_of(w.reset_index.off).view(np.uint32)[:n_entries] == want_index.off[:n_entries]).all()


@pytest.mark.parametrize("mem", ["host", "device"])
def test_streams_that_end_with_a_reset(ta, oracle, prose, mem):
    import torch

    N, kw = 64, conf_kw()
    data = prose[60_000 : 60_000 + 2 * N + 5]
    (blob,), index = fresh(ta, [data], N, kw)
    assert int(index.first[1]) == 2
    cut = blob[: int(index.off[1])]  # E = 2 entries, an empty open segment
    for src in (b"", b"x", prose[70_000 : 70_000 + N], prose[70_000 : 70_000 + 2 * N + 1]):
        args = ([cut, cut],) if mem == "host" else on_device(ta, [cut, cut])
        more = {} if mem == "host" else dict(window=10, literal=8, extended=True)
        twice = ta.ResetIndex(np.array([0, 2, 4], np.uint64), np.concatenate([index.off, index.off]), N)
        res = ta.append_batch(*args, reset_index=twice, source=[src, b""], **more)
        if mem == "device":
            torch.cuda.synchronize()
        assert (np_of(res.status) == 0).all()
        assert res.stream(1) == cut
        if not src:
            assert res.stream(0) == cut and np_of(res.reset_index.first).tolist() == [0, 2, 4]
            continue
        (want,), want_index = fresh(ta, [data[: 2 * N] + src], N, kw)
        assert res.stream(0) == want
        first = np_of(res.reset_index.first)
        assert int(first[1]) == int(want_index.first[1]) and int(first[2]) == int(first[1]) + 2
        assert (np_of(res.reset_index.off).view(np.uint32)[: int(first[1])] == want_index.off).all()
        st, back, _ = oracle.decompress(res.stream(0), cap=len(data) + len(src) + 8)
        assert st in (OK, INPUT_EXHAUSTED) and back == data[: 2 * N] + src


@pytest.mark.parametrize("mem", ["host", "device"])
def test_irregular_closed_segments(ta, oracle, prose, mem):
    """A stream whose closed segment does not hold N bytes (written with a reset at N + 7, as the reference's append mode leaves
    them): only the open segment is brought onto the grid, the bytes in front of it stay."""
    import torch

    N = 64
    a, b = prose[80_000 : 80_000 + N + 7], prose[81_000:81_010]
    res, blob = oracle.stream_script([("write", a), ("reset",), ("write", b), ("close",)], window=10, literal=8, dictionary_reset=True)
    assert res == 0
    scan = ta.index_resets([blob])
    assert int(scan.index.first[1]) == 1
    start = int(scan.index.off[0])
    for src in (prose[82_000 : 82_000 + 5], prose[82_000 : 82_000 + 3 * N + 1]):
        args = ([blob],) if mem == "host" else on_device(ta, [blob])
        more = {} if mem == "host" else dict(window=10, literal=8, extended=True)
        out = ta.append_batch(*args, reset_index=scan.index, reset_interval=N, source=[src], **more)
        if mem == "device":
            torch.cuda.synchronize()
        assert int(np_of(out.status)[0]) == OK
        new = out.stream(0)
        assert new[:start] == blob[:start]
        st, back, _ = oracle.decompress(new, cap=len(a + b + src) + 8)
        assert st in (OK, INPUT_EXHAUSTED) and back == a + b + src
        first, off = np_of(out.reset_index.first), np_of(out.reset_index.off).view(np.uint32)
        assert int(first[1]) == 1 + (len(b) + len(src) - 1) // N and int(off[0]) == start
        # behind the old entry the stream is on the grid: what a fresh compress makes of b + src, behind its header
        (tail,), tail_index = fresh(ta, [b + src], N, conf_kw())
        assert new[start:] == tail[2:]
        assert (off[1 : int(first[1])] == tail_index.off + np.uint32(start - 2)).all()


FAIL_N = 64


def failing_batch(ta, oracle, prose):
    """Ten streams at literal 7; each victim fails by one rule, the others are appended to as usual.
    -> (blobs, first, off, sources, out_cap, {victim: code}, datas)."""
    N, kw = FAIL_N, conf_kw(literal=7)
    lens = [3 * N + 40, 2 * N, 5 * N + 9, N + 1, 700, 2 * N + 30, 90, 4 * N + 3, 3 * N + 5, 2 * N + 17]
    datas = [prose[100_000 + 1000 * j : 100_000 + 1000 * j + n] for j, n in enumerate(lens)]
    srcs = [prose[120_000 + 500 * j : 120_000 + 500 * j + n] for j, n in enumerate([N, 3, 2 * N + 1, N - 1, 40, 7, 130, 2 * N, 0, 50])]
    blobs, index = fresh(ta, datas, N, kw)
    blobs, first, off = list(blobs), index.first.copy(), index.off.copy()
    failing = {}
    # 0: its last entry moved by one byte: the open segment no longer parses to N bytes at most from there (the oracle says so)
    last = int(first[1]) - 1
    st, back, _ = oracle.decompress(blobs[0][:2] + blobs[0][int(off[last]) + 1 :], cap=4096)
    assert st in (OK, INPUT_EXHAUSTED) and len(back) > N, "the moved entry must be told by the size alone: choose other data"
    off[last] += np.uint32(1)
    failing[0] = BAD_INDEX
    # 1: an open segment of 2 N bytes under the call's interval N (compressed with 2 N: no entries)
    (blobs[1],), _ = fresh(ta, [datas[1]], 2 * N, kw)
    assert int(first[2]) - int(first[1]) == 1
    off = np.delete(off, int(first[1]))
    first[2:] -= np.uint64(1)
    failing[1] = BAD_INDEX
    # 2: a header of another window
    (other,), other_index = fresh(ta, [datas[2]], N, conf_kw(window=11, literal=7))
    assert len(other_index.off) == int(first[3]) - int(first[2])
    blobs[2] = other
    off[int(first[2]) : int(first[3])] = other_index.off
    failing[2] = INVALID_CONF
    # 3: a source byte of 0x80
    srcs[3] = srcs[3][:20] + b"\x80" + srcs[3][21:]
    failing[3] = EXCESS_BITS
    # 4: out_cap one byte short (below)
    failing[4] = OUTPUT_FULL
    # 9: rows of reset_first out of order; stream 8 in front of it receives nothing and is copied
    first[9] = first[10] + np.uint64(1)
    failing[9] = BAD_INDEX
    news = [d + s for d, s in zip(datas, srcs)]
    want_streams, _ = fresh(ta, [news[i] if i not in (3,) else datas[i] for i in range(len(datas))], N, kw)
    from tamp_amd.batch import _append_closed_bound

    out_cap = np.array([len(b) + (-(-len(s) // N) + 1) * _append_closed_bound(N, 7) for b, s in zip(blobs, srcs)], dtype=np.uint32)
    out_cap[4] = len(want_streams[4]) - 1
    return blobs, first, off, srcs, out_cap, failing, datas


@pytest.mark.parametrize("mem", ["host", "device"])
def test_failing_alone(ta, oracle, prose, mem):
    import torch

    N, kw = FAIL_N, conf_kw(literal=7)
    blobs, first, off, srcs, out_cap, failing, datas = failing_batch(ta, oracle, prose)
    index = ta.ResetIndex(first, off, N)
    if mem == "host":
        res = ta.append_batch(blobs, reset_index=index, source=srcs, out_cap=out_cap)
    else:
        res = ta.append_batch(*on_device(ta, blobs), reset_index=index, source=srcs, out_cap=torch.from_numpy(out_cap.astype(np.int64)).cuda(),
                              window=10, literal=7, extended=True)
        torch.cuda.synchronize()
    status, out_len = np_of(res.status), np_of(res.out_len)
    for i, code in failing.items():
        assert (int(status[i]), int(out_len[i])) == (code, 0), (i, int(status[i]), int(out_len[i]))
    good = [i for i in range(len(datas)) if i not in failing]
    want_streams, want_index = fresh(ta, [datas[i] + srcs[i] for i in good], N, kw)
    new_first, new_off = np_of(res.reset_index.first), np_of(res.reset_index.off).view(np.uint32)
    for at, i in enumerate(good):
        assert int(status[i]) == OK and res.stream(i) == want_streams[at], i
        if i == 8:  # (its rows of reset_first do not hold: it is copied without entries)
            continue
        a, b = int(new_first[i]), int(new_first[i + 1])
        assert (new_off[a:b] == want_index.off[int(want_index.first[at]) : int(want_index.first[at + 1])]).all(), i
    # a failing stream keeps its E rows, zeroed
    for i in (0, 2, 3, 4):
        a, b = int(new_first[i]), int(new_first[i + 1])
        assert b - a == int(first[i + 1]) - int(first[i]) and (new_off[a:b] == 0).all(), i


def layout(caps):
    """Slabs at odd offsets with guard bytes between them: -> (out_off uint64, total)."""
    off, at = [], 1
    for j, c in enumerate(caps):
        at |= 1
        off.append(at)
        at += int(c) + 3 + j % 5
    return np.array(off, dtype=np.uint64), at + 8


def c_call(blobs, first, off, N, srcs, kw, *, mem, new_cap, src_shift=0, pad=0, no_off=False):
    """One tamp_batch_append call on hand-laid tables: poisoned result tables, guard bytes around every slab; source i starts
    ``src_shift + i`` bytes (odd and even) behind a 16-byte boundary of its own; ``pad`` poisoned entries lie behind the
    ``new_cap`` that the call is told of; ``no_off``: reset_off is NULL.  -> (rc, status, out_len, out, out_off, out_cap, new_first,
    new_off with its pad)."""
    from tamp_amd import _lib
    from tamp_amd.batch import _append_closed_bound, pack_streams

    lib = _lib.load()
    n = len(blobs)
    flat, in_off, in_len = pack_streams(blobs)
    out_cap = np.array([len(b) + (-(-len(s) // N) + 1) * _append_closed_bound(N, kw["literal"]) for b, s in zip(blobs, srcs)], dtype=np.uint32)
    out_off, total = layout(out_cap)
    out = np.full(total, GUARD, dtype=np.uint8)
    out_len, status = np.full(n, 0xDEAD, dtype=np.uint32), np.full(n, 99, dtype=np.int8)
    src_off, at = [], 0
    for i, s in enumerate(srcs):
        at = (at + 15) // 16 * 16 + (src_shift + i) % 16
        src_off.append(at)
        at += len(s)
    src = np.zeros(at + 16, dtype=np.uint8)
    for o, s in zip(src_off, srcs):
        src[o : o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    src_off, src_len = np.array(src_off, dtype=np.uint64), np.array([len(s) for s in srcs], dtype=np.uint32)
    new_first, new_off = np.full(n + 1, 0xDEAD, dtype=np.uint64), np.full(max(new_cap, 1) + pad, 0xDEADBEEF, dtype=np.uint32)
    first, off = np.ascontiguousarray(first, dtype=np.uint64), np.ascontiguousarray(off, dtype=np.uint32)
    conf = _lib.TampAmdConf(kw["window"], kw["literal"], 0, int(kw["extended"]), 1, int(kw["lazy_matching"]), 0)
    tables = [flat, in_off, in_len, first, off if len(off) else np.zeros(1, np.uint32), src, src_off, src_len, out, out_off, out_cap, out_len, status,
              new_first, new_off]
    if mem == "host":
        t = tables
        p = [a.ctypes.data_as(C.c_void_p) for a in tables]
    else:
        import torch

        dev = torch.device("cuda:0")
        views = [None, np.int64, np.int32, np.int64, np.int32, None, np.int64, np.int32, None, np.int64, np.int32, np.int32, None, np.int64, np.int32]
        t = [torch.from_numpy(a.copy() if v is None else a.view(v).copy()).to(dev) for a, v in zip(tables, views)]
        torch.cuda.synchronize()
        p = [C.c_void_p(x.data_ptr()) for x in t]
    rc = lib.tamp_batch_append(C.byref(conf), 15, p[0], p[1], p[2], p[3], p[4] if len(off) and not no_off else None, N, p[5], p[6], p[7], p[8], p[9], p[10],
                               p[11], p[12], p[13], p[14], new_cap, n, _lib.MEM_HOST if mem == "host" else _lib.MEM_DEVICE, 0, None)
    if mem != "host":
        import torch

        torch.cuda.synchronize()
        t = [x.cpu().numpy() for x in t]
    return rc, t[12], t[11].view(np.uint32), t[8], out_off, out_cap, t[13].view(np.uint64), t[14].view(np.uint32)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_the_c_call_by_hand(ta, prose, mem):
    N, kw = 100, conf_kw()
    datas = streams_for(prose, N, count=24, seed=5)
    srcs = sources_for(prose, datas, N, seed=6)
    news = [d + s for d, s in zip(datas, srcs)]
    blobs, index = fresh(ta, datas, N, kw)
    want_streams, want_index = fresh(ta, news, N, kw)
    bound = int(index.first[-1]) + sum(-(-len(s) // N) for s in srcs)
    for shift in (0, 1):
        rc, status, out_len, out, out_off, out_cap, new_first, new_off = c_call(blobs, index.first, index.off, N, srcs, kw, mem=mem, new_cap=bound,
                                                                                src_shift=shift)
        assert rc == 0 and (status == 0).all()
        expect = np.full(len(out), GUARD, dtype=np.uint8)
        for i, blob in enumerate(want_streams):
            assert int(out_len[i]) == len(blob), i
            expect[int(out_off[i]) : int(out_off[i]) + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        assert (out == expect).all(), np.flatnonzero(out != expect)[:10]
        assert (new_first == want_index.first).all()
        entries = int(new_first[-1])
        assert (new_off[:entries] == want_index.off).all() and (new_off[entries:] == 0xDEADBEEF).all()
    # one entry less than the bound: refused, nothing written
    rc, status, out_len, out, out_off, out_cap, new_first, new_off = c_call(blobs, index.first, index.off, N, srcs, kw, mem=mem, new_cap=bound - 1)
    assert rc == BAD_ARGUMENT
    assert (out == GUARD).all() and (status == 99).all() and (out_len == 0xDEAD).all()
    assert (new_first == 0xDEAD).all() and (new_off == 0xDEADBEEF).all()


@pytest.mark.parametrize("mem", ["host", "device"])
def test_rows_that_overlap_fail_alone(ta, prose, mem):
    """Rows of reset_first that are each in order but claim the same entries ({0, 5, 3, 8, 10}: streams 0 and 2): the later one does
    not hold.  It fails alone, or is copied without entries when nothing is appended; the streams that hold get their own entries, and
    nothing is stored behind new_reset_cap, which is exactly the bound."""
    N, kw = 64, conf_kw()
    datas = [prose[130_000 + 1000 * j : 130_000 + 1000 * j + n] for j, n in enumerate([5 * N + 9, 2 * N + 3, 5 * N + 20, 2 * N + 30])]
    blobs, index = fresh(ta, datas, N, kw)
    assert index.first.tolist() == [0, 5, 7, 12, 14]
    first = np.array([0, 5, 3, 8, 10], dtype=np.uint64)  # stream 1: decreasing; stream 2: into stream 0's entries; stream 3: behind both
    off = np.concatenate([index.off[0:5], np.array([7, 7, 7], np.uint32), index.off[12:14]])
    some = [prose[140_000 : 140_000 + N + 5], prose[141_000 : 141_000 + 9], prose[142_000 : 142_000 + 2 * N], prose[143_000 : 143_000 + 3 * N + 1]]
    for srcs in ([b"", b"", b"", b""], some):
        bound = 10 + sum(-(-len(s) // N) for s in srcs)
        rc, status, out_len, out, out_off, out_cap, new_first, new_off = c_call(blobs, first, off, N, srcs, kw, mem=mem, new_cap=bound, pad=16)
        assert rc == 0
        expect = np.full(len(out), GUARD, dtype=np.uint8)
        same = np.ones(len(out), dtype=bool)
        if not srcs[0]:
            assert (status == 0).all()
            for i, blob in enumerate(blobs):
                assert int(out_len[i]) == len(blob)
                expect[int(out_off[i]) : int(out_off[i]) + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
            assert new_first.tolist() == [0, 5, 5, 5, 7]
            assert (new_off[:5] == index.off[0:5]).all() and (new_off[5:7] == index.off[12:14]).all()
        else:
            assert [int(x) for x in status] == [OK, BAD_INDEX, BAD_INDEX, OK] and int(out_len[1]) == int(out_len[2]) == 0
            want_streams, want_index = fresh(ta, [datas[0] + srcs[0], datas[3] + srcs[3]], N, kw)
            for at, i in enumerate((0, 3)):
                assert int(out_len[i]) == len(want_streams[at]), i
                expect[int(out_off[i]) : int(out_off[i]) + len(want_streams[at])] = np.frombuffer(want_streams[at], dtype=np.uint8)
                a, b = int(new_first[i]), int(new_first[i + 1])
                assert (new_off[a:b] == want_index.off[int(want_index.first[at]) : int(want_index.first[at + 1])]).all(), i
            for i in (1, 2):  # (what lies inside a failing stream's slab is its own)
                same[int(out_off[i]) : int(out_off[i]) + int(out_cap[i])] = False
            assert int(new_first[1]) == int(new_first[2]) == int(new_first[3]) and int(new_first[4]) == int(want_index.first[2])
        assert (out[same] == expect[same]).all(), np.flatnonzero(same & (out != expect))[:10]
        assert int(new_first[-1]) <= bound and (new_off[int(new_first[-1]) :] == 0xDEADBEEF).all()


@pytest.mark.parametrize("mem", ["host", "device"])
def test_entries_and_no_table_for_them(ta, prose, mem):
    """reset_off == NULL: a stream with entries fails alone with TAMP_AMD_BAD_INDEX, one without entries is appended to, in both
    memory kinds alike."""
    N, kw = 64, conf_kw()
    datas = [prose[150_000 : 150_000 + 2 * N + 5], prose[151_000 : 151_000 + 10]]
    srcs = [prose[152_000 : 152_000 + 7], prose[153_000 : 153_000 + N + 60]]
    blobs, index = fresh(ta, datas, N, kw)
    assert index.first.tolist() == [0, 2, 2]
    rc, status, out_len, out, out_off, out_cap, new_first, new_off = c_call(blobs, index.first, index.off, N, srcs, kw, mem=mem, new_cap=2 + 1 + 2,
                                                                            no_off=True)
    assert rc == 0 and [int(x) for x in status] == [BAD_INDEX, OK] and int(out_len[0]) == 0
    (want,), want_index = fresh(ta, [datas[1] + srcs[1]], N, kw)
    assert out[int(out_off[1]) : int(out_off[1]) + int(out_len[1])].tobytes() == want
    assert len(want_index.off) == 2  # (10 + 124 bytes: three segments)
    assert new_first.tolist() == [0, 0, 2] and (new_off[:2] == want_index.off).all()


def test_slices(ta, prose, capfd, monkeypatch):
    """A scratch budget of 1 MiB at N = 1024: the batch takes three slices or more of whole streams and gives the same result; a
    stream whose rows alone outgrow the budget fails alone."""
    import torch

    N, kw = 1024, conf_kw()
    datas = streams_for(prose, N, count=64, seed=7)
    srcs = [prose[(17_000 * i) % 900_000 : (17_000 * i) % 900_000 + 16 * N + 13 * i] for i in range(64)]
    news = [d + s for d, s in zip(datas, srcs)]
    blobs, index = fresh(ta, datas, N, kw)
    capfd.readouterr()
    one = ta.append_batch(blobs, reset_index=index, source=srcs)
    m = LINE.search(capfd.readouterr().err)
    assert m and (int(m[1]), int(m[3])) == (64, 1)
    units = int(m[2])
    assert units > 2 * 464  # (1 MiB holds 464 rows of 1024 + 1156 + 80 bytes)
    assert int(m[4]) == sum(len(s) + open_size(len(d), N) for d, s in zip(datas, srcs))
    assert_same(ta, one, news, N, kw)
    monkeypatch.setenv("TAMP_AMD_RANGES_SCRATCH_MB", "1")
    capfd.readouterr()
    res = ta.append_batch(blobs, reset_index=index, source=srcs)
    m = LINE.search(capfd.readouterr().err)
    assert m and int(m[2]) == units and int(m[3]) >= 3, m and m[0]
    assert res.streams() == one.streams() and (np_of(res.reset_index.off) == np_of(one.reset_index.off)).all()
    capfd.readouterr()
    dres = ta.append_batch(*on_device(ta, blobs), reset_index=index, source=srcs, window=10, literal=8, extended=True)
    torch.cuda.synchronize()
    m = LINE.search(capfd.readouterr().err)
    assert m and int(m[3]) >= 3
    assert dres.streams() == one.streams()
    # one stream receives more than the budget holds rows for
    big = list(srcs)
    big[5] = (prose * 2)[: 480 * N]
    for args, more in (((blobs,), {}), (on_device(ta, blobs), dict(window=10, literal=8, extended=True))):
        res = ta.append_batch(*args, reset_index=index, source=big, **more)
        torch.cuda.synchronize()
        status = np_of(res.status)
        assert int(status[5]) == BAD_ARGUMENT and int(np_of(res.out_len)[5]) == 0
        assert all(int(s) == OK for i, s in enumerate(status) if i != 5)
        got = res.streams()
        assert all(got[i] == one.stream(i) for i in range(64) if i != 5)


def test_stream_argument(ta, prose):
    """``stream=`` on a side stream, next to a compress_batch on the current one: the same bytes."""
    import torch

    N, kw = 100, conf_kw()
    datas = streams_for(prose, N, count=32, seed=8)
    srcs = sources_for(prose, datas, N, seed=9)
    news = [d + s for d, s in zip(datas, srcs)]
    blobs, index = fresh(ta, datas, N, kw)
    data, off, ln = on_device(ta, blobs)
    busy = on_device(ta, [prose[i * 4096 : (i + 1) * 4096] for i in range(128)])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    other = ta.compress_batch(*busy, window=10, literal=8, extended=True, max_in_len=4096)
    res = ta.append_batch(data, off, ln, reset_index=index, source=srcs, stream=side.cuda_stream, window=10, literal=8, extended=True)
    side.synchronize()
    torch.cuda.synchronize()
    assert (np_of(other.status) == 0).all()
    assert_same(ta, res, news, N, kw)
    with pytest.raises(ValueError, match="required with CUDA tensors"):
        ta.append_batch(data, off, ln, reset_index=index, source=srcs)


def test_command_line(ta, prose, tmp_path):
    """``python -m tamp_amd append STREAM INPUT``: the file is rewritten (or ``-o`` written) as a fresh compress of old + appended;
    a stream without a closed segment needs ``--reset-interval``."""
    from tamp_amd import cli

    N = 256
    old, more = prose[90_000 : 90_000 + 3 * N + 17], prose[95_000 : 95_000 + 2 * N + 40]
    stream, extra, out = tmp_path / "log.tamp", tmp_path / "more.bin", tmp_path / "new.tamp"
    stream.write_bytes(bytes(ta.compress(old, dictionary_reset=True, reset_interval=N)))
    extra.write_bytes(more)
    want = bytes(ta.compress(old + more, dictionary_reset=True, reset_interval=N))
    assert cli.main(["append", str(stream), str(extra), "-o", str(out)]) == 0
    assert out.read_bytes() == want and stream.read_bytes() != want
    assert cli.main(["append", str(stream), str(extra), "--reset-interval", str(N + 1)]) == 1  # (not the stream's interval)
    assert cli.main(["append", str(stream), str(extra)]) == 0
    assert stream.read_bytes() == want and sorted(p.name for p in tmp_path.iterdir()) == ["log.tamp", "more.bin", "new.tamp"]
    short = tmp_path / "short.tamp"
    short.write_bytes(bytes(ta.compress(old[:100], dictionary_reset=True, reset_interval=N)))
    assert cli.main(["append", str(short), str(extra)]) == 1  # (nothing to tell the interval by)
    assert cli.main(["append", str(short), str(extra), "--reset-interval", str(N)]) == 0
    assert short.read_bytes() == bytes(ta.compress(old[:100] + more, dictionary_reset=True, reset_interval=N))
