"""GPU tier: byte ranges of reset-segmented streams read without decoding the rest (tamp_batch_read_ranges, ``read_ranges``; the
kernels of tamp_read_ranges_kernel.hpp, DESIGN.md 3.13 "Reading ranges").

The streams are cut from the 7-bit prose fixture and compressed through tamp_batch_compress_resets_index; the expectation is always
the slice of the ORIGINAL input, never a GPU result.  Every range's room is laid out by hand behind 0xA5 guards at all four
residues mod 4, the result tables are poisoned before the call, and afterwards the whole buffer is compared."""
import ctypes as C
import random
import re

import numpy as np
import pytest
from long_stream_writer import TokenWriter
from test_gpu_batch_reset_index import index_call
from test_gpu_batch_resets import CONFIGS, GUARD, layout, mixed, streams_of

pytestmark = pytest.mark.gpu

OK, INPUT_EXHAUSTED, ERROR, INVALID_CONF, OOB, BAD_ARGUMENT, BAD_INDEX = 0, 2, -1, -3, -4, -21, -22
TABLE = {OK, INPUT_EXHAUSTED, ERROR, INVALID_CONF, OOB, BAD_ARGUMENT, BAD_INDEX}  # every status the call's table knows
LINE = re.compile(r"\[tamp_amd resets\] read ranges: (\d+) ranges, (\d+) units, (\d+) slices, (\d+) bytes staged$", re.M)
WEAK = "weak"  # a range of which only the table's rules are asserted: a status of the table, out_len <= length, guards intact


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


def entries_of(n, interval):
    return max(1, -(-n // interval)) - 1


_batches = {}


def batch(prose, interval, window=10, literal=8, extended=True, lazy=False, lengths=None, at=3000):
    """(datas, blobs, reset_first, reset_off) of a batch compressed once through tamp_batch_compress_resets_index."""
    key = (interval, window, literal, extended, lazy, tuple(lengths) if lengths is not None else None, at)
    if key not in _batches:
        datas = streams_of(prose, mixed(interval) if lengths is None else lengths, at=at)
        rc, status, out_len, out, out_off, _, first, off = index_call(datas, interval, window=window, literal=literal, extended=extended, lazy=lazy)
        assert rc == 0 and (status == 0).all()
        blobs = [out[int(o) : int(o) + int(n)].tobytes() for o, n in zip(out_off, out_len)]
        assert [int(first[i + 1] - first[i]) for i in range(len(datas))] == [entries_of(len(d), interval) for d in datas]
        _batches[key] = (datas, blobs, first.copy(), off[: int(first[-1])].copy())
    return _batches[key]


def ranges_call(blobs, first, off, interval, ranges, *, mem="host", stream=None, max_wbits=15):
    """One tamp_batch_read_ranges call on hand-laid tables; ``ranges``: (stream, begin, length) each.
    -> (rc, status, out_len, the output buffer, out_off)"""
    from tamp_amd import _lib
    from tamp_amd.batch import pack_streams

    lib = _lib.load()
    flat, in_off, in_len = pack_streams(blobs)
    if flat.size == 0:
        flat = np.zeros(1, np.uint8)
    nr = len(ranges)
    r_stream = np.array([r[0] for r in ranges], dtype=np.uint32)
    r_begin = np.array([r[1] for r in ranges], dtype=np.uint64)
    r_len = np.array([r[2] for r in ranges], dtype=np.uint32)
    out_off, total = layout([r[2] for r in ranges], [q % 4 for q in range(nr)])
    out = np.full(total, GUARD, dtype=np.uint8)
    out_len, status = np.full(nr, 0xDEAD, dtype=np.uint32), np.full(nr, 99, dtype=np.int8)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    no_off = off is None  # (a null reset_off: for an index without entries)
    off = np.zeros(1, np.uint32) if off is None or len(off) == 0 else np.ascontiguousarray(off, dtype=np.uint32)
    tables = [flat, in_off, in_len, first, off, r_stream, r_begin, r_len, out, out_off, out_len, status]
    if mem == "host":
        p = [a.ctypes.data_as(C.c_void_p) for a in tables]
        p[4] = None if no_off else p[4]
        rc = lib.tamp_batch_read_ranges(max_wbits, p[0], p[1], p[2], p[3], p[4], interval, p[5], p[6], p[7], p[8], p[9], p[10], p[11],
                                        len(blobs), nr, _lib.MEM_HOST, 0, None)
        return rc, status, out_len, out, out_off
    import torch

    dev = torch.device("cuda:0")
    views = [None, np.int64, np.int32, np.int64, np.int32, np.int32, np.int64, np.int32, None, np.int64, np.int32, None]
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        t = [torch.from_numpy(a.copy() if v is None else a.view(v).copy()).to(dev) for a, v in zip(tables, views)]
    torch.cuda.synchronize()
    p = [C.c_void_p(x.data_ptr()) for x in t]
    p[4] = None if no_off else p[4]
    rc = lib.tamp_batch_read_ranges(max_wbits, p[0], p[1], p[2], p[3], p[4], interval, p[5], p[6], p[7], p[8], p[9], p[10], p[11],
                                    len(blobs), nr, _lib.MEM_DEVICE, 0, C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return rc, t[11].cpu().numpy(), t[10].cpu().numpy().view(np.uint32), t[8].cpu().numpy(), out_off


def rule(datas, interval, r):
    """The table of the call for a true index: (status, bytes) of range ``r`` from the ORIGINAL input."""
    s, begin, length = r
    if s >= len(datas):
        return BAD_ARGUMENT, b""
    if length == 0:
        return OK, b""
    if begin // interval > entries_of(len(datas[s]), interval):
        return INPUT_EXHAUSTED, b""
    piece = datas[s][begin : begin + length]
    return (OK if len(piece) == length else INPUT_EXHAUSTED), piece


def check(res, ranges, wants):
    """Status, length and the WHOLE buffer; ``wants[q]``: (status, bytes), or WEAK."""
    rc, status, out_len, out, out_off = res
    assert rc == 0
    expect = np.full(len(out), GUARD, dtype=np.uint8)
    same = np.ones(len(out), dtype=bool)
    for q, (r, w) in enumerate(zip(ranges, wants)):
        o = int(out_off[q])
        if w == WEAK:
            assert int(status[q]) in TABLE and int(out_len[q]) <= r[2], (q, r, int(status[q]), int(out_len[q]))
            same[o : o + int(out_len[q])] = False  # (what it delivered is its own; everything around it is compared)
            continue
        assert (int(status[q]), int(out_len[q])) == (w[0], len(w[1])), (q, r, int(status[q]), int(out_len[q]), w[0], len(w[1]))
        expect[o : o + len(w[1])] = np.frombuffer(w[1], dtype=np.uint8)
    bad = np.flatnonzero((out != expect) & same)
    assert bad.size == 0, ("bytes differ, or a guard was written", bad[:8].tolist())


def touched(r, interval, E):
    """The segments range ``r`` touches in a stream with E entries."""
    _, begin, length = r
    if length == 0 or begin // interval > E:
        return set()
    return set(range(begin // interval, min((begin + length - 1) // interval, E) + 1))


def sweep(datas, interval):
    """Every boundary of every stream: begins and lengths around the segments' edges, the stream's end and the last segment."""
    N, ranges = interval, []
    for s, d in enumerate(datas):
        L, E = len(d), entries_of(len(d), interval)
        begins = {0, 1, L - 1, L, L + 1, (E + 1) * N, (E + 2) * N}
        for k in {1, max(E, 1), max(E // 2, 1)}:
            begins |= {k * N - 1, k * N, k * N + 1}
        lens = {0, 1, N - 1, N, N + 1, 2 * N, 3 * N + 1, L, L + 5}
        ranges += [(s, b, n) for b in sorted(x for x in begins if x >= 0) for n in sorted(lens)]
    return ranges


def stream1():
    import torch

    return torch.cuda.Stream()


# ---- every boundary, on every configuration, from host and device memory ----

@pytest.mark.parametrize("window,literal,extended,lazy", CONFIGS)
def test_every_boundary(ta, prose, window, literal, extended, lazy, capfd):
    for interval in (16, 1000):
        datas, blobs, first, off = batch(prose, interval, window, literal, extended, lazy)
        ranges = sweep(datas, interval)
        wants = [rule(datas, interval, r) for r in ranges]
        assert {w[0] for w in wants} == {OK, INPUT_EXHAUSTED} and any(w[0] == INPUT_EXHAUSTED and w[1] for w in wants)
        check(ranges_call(blobs, first, off, interval, ranges), ranges, wants)
        line = LINE.findall(capfd.readouterr().err)[-1]  # only the touched segments are units
        assert (int(line[0]), int(line[1])) == (len(ranges), sum(len(touched(r, interval, entries_of(len(datas[r[0]]), interval))) for r in ranges))
        check(ranges_call(blobs, first, off, interval, ranges, mem="device", stream=stream1() if lazy or window == 15 else None), ranges, wants)


@pytest.mark.parametrize("forced", ["split", "wave", "lane", "global"])
def test_every_decoder(ta, prose, forced, monkeypatch):
    """The decode step is the existing launch path, so TAMP_AMD_DECODER keeps forcing it: a unit whose room is trimmed to the last
    byte asked for (need < size) comes back with exactly that many bytes from each of them."""
    monkeypatch.setenv("TAMP_AMD_DECODER", forced)
    for interval in (16, 1000):
        datas, blobs, first, off = batch(prose, interval)
        ranges = sweep(datas, interval)
        wants = [rule(datas, interval, r) for r in ranges]
        assert any(w[0] == OK and (r[1] + r[2]) % interval and r[1] + r[2] < len(datas[r[0]]) for r, w in zip(ranges, wants))  # trimmed units
        for mem in ("host", "device"):
            check(ranges_call(blobs, first, off, interval, ranges, mem=mem), ranges, wants)


# ---- shapes ----

@pytest.mark.parametrize("mem", ["host", "device"])
def test_shapes(ta, prose, mem):
    interval = 16
    datas, blobs, first, off = batch(prose, interval)
    long = max(range(len(datas)), key=lambda s: len(datas[s]))
    L = len(datas[long])
    shapes = {
        "the same range twice": [(long, 40, 50), (long, 40, 50)],
        "two ranges on one segment, and overlapping ones": [(long, 33, 3), (long, 37, 9), (long, 30, 100), (long, 90, 100)],
        "reverse stream order": [(s, 1, 20) for s in reversed(range(len(datas)))],
        "300 ranges on one stream": [(long, (7 * q) % L, 1 + q % 45) for q in range(300)],
        "the empty stream and streams without entries": [(s, b, n) for s, d in enumerate(datas) if len(d) <= interval
                                                         for b in (0, 1, interval) for n in (1, interval, 3 * interval)],
        "no stream of that number among good ones": [(0, 0, 0), (len(datas), 0, 4), (long, 5, 4), (0xFFFFFFFF, 0, 0), (long, 0, 1)],
    }
    for what, ranges in shapes.items():
        wants = [rule(datas, interval, r) for r in ranges]
        check(ranges_call(blobs, first, off, interval, ranges, mem=mem), ranges, wants)
    assert [len(d) for d in datas].count(0) == 2 and wants[1][0] == BAD_ARGUMENT
    # one range on each of 300 streams (short ones: most have no entry at all)
    lengths = [(11 * i) % 50 for i in range(300)]
    datas, blobs, first, off = batch(prose, interval, lengths=lengths, at=100)
    ranges = [(s, (3 * s) % 40, 1 + s % 30) for s in range(300)]
    check(ranges_call(blobs, first, off, interval, ranges, mem=mem), ranges, [rule(datas, interval, r) for r in ranges])
    # no entries anywhere: reset_off may be null
    datas, blobs, first, off = batch(prose, interval, lengths=[5, 0, 16], at=100)
    assert int(first[-1]) == 0
    ranges = [(0, 0, 5), (0, 2, 9), (1, 0, 1), (2, 15, 2), (2, 16, 1)]
    check(ranges_call(blobs, first, None, interval, ranges, mem=mem), ranges, [rule(datas, interval, r) for r in ranges])


# ---- a damaged index ----

def damaged(datas, interval, ranges, stream, bad, weak=()):
    """The rule with the segments ``bad`` of ``stream`` refused; ranges that touch only good ones and ``weak`` ones: WEAK."""
    wants = []
    for r in ranges:
        w = rule(datas, interval, r)
        if r[0] == stream:
            t = touched(r, interval, entries_of(len(datas[stream]), interval))
            if t & set(bad):
                w = (BAD_INDEX, b"")
            elif t & set(weak):
                w = WEAK
        wants.append(w)
    return wants


@pytest.mark.parametrize("mem", ["host", "device"])
def test_a_damaged_index(ta, prose, mem):
    interval = 16
    datas, blobs, first, off = batch(prose, interval)
    long = max(range(len(datas)), key=lambda s: len(datas[s]))
    E, f = entries_of(len(datas[long]), interval), int(first[long])
    assert E == 39
    ranges = [r for r in sweep(datas, interval) if r[0] != long]
    ranges += [(long, b, n) for b in range(0, 9 * interval, 5) for n in (1, 7, interval, 2 * interval + 3)] + [(long, 0, len(datas[long]))]

    def run(first_, off_, bad, weak=(), stream=long):
        wants = damaged(datas, interval, ranges, stream, bad, weak)
        assert any(w != WEAK and w[0] == BAD_INDEX for w in wants) and any(w != WEAK and w[0] == OK and w[1] for w in wants)
        check(ranges_call(blobs, first_, off_, interval, ranges, mem=mem), ranges, wants)

    def with_entry(j, value):
        o = off.copy()
        o[f + j] = value
        return o

    run(first, with_entry(3, len(blobs[long]) + 1), bad=(3, 4))             # an entry beyond in_len
    run(first, with_entry(3, 0xFFFFFFFF), bad=(3, 4))
    run(first, with_entry(4, off[f + 3]), bad=(4, 5))                       # two equal entries: an empty segment, and one of 2 N bytes
    o = off.copy()
    o[f + 3], o[f + 4] = off[f + 4], off[f + 3]
    run(first, o, bad=(3, 4, 5))                                            # swapped
    run(first, with_entry(0, 1), bad=(0, 1))                                # inside the header
    run(first, with_entry(0, 0), bad=(0, 1))
    # an entry shifted by one: the segment that ENDS at it loses its second FLUSH, or ends in front of eight bits that are no FLUSH at
    # any literal width; what the one BEHIND it comes to is not said
    run(first, with_entry(3, off[f + 3] - 1), bad=(3,), weak=(4,))
    run(first, with_entry(3, off[f + 3] + 1), bad=(3,), weak=(4,))
    # a reset_first that decreases: the stream whose rows are out of order; the one behind it has other entries than its own
    fd = first.copy()
    fd[long + 1] = first[long] - 1
    wants = damaged(datas, interval, ranges, long, bad=range(E + 1))
    wants = [WEAK if r[0] == long + 1 and r[2] else w for r, w in zip(ranges, wants)]
    check(ranges_call(blobs, fd, off, interval, ranges, mem=mem), ranges, wants)
    # the wrong interval: every range that touches a closed segment
    for wrong in (interval + 1, 2 * interval):
        wants = []
        for r in ranges:
            En = entries_of(len(datas[r[0]]), interval)
            t = touched(r, wrong, En)
            wants.append(rule(datas, interval, r) if not r[2] else (BAD_INDEX, b"") if any(k < En for k in t)
                         else (INPUT_EXHAUSTED, b"") if not t else WEAK)
        assert sum(w != WEAK and w[0] == BAD_INDEX for w in wants) > 100
        check(ranges_call(blobs, first, off, wrong, ranges, mem=mem), ranges, wants)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_streams_that_are_refused(ta, prose, mem):
    interval = 16
    datas, blobs, first, off = batch(prose, interval)
    long = max(range(len(datas)), key=lambda s: len(datas[s]))
    ranges = sweep(datas, interval)
    for h0 in (blobs[long][0] & 0xFE, blobs[long][0] | 4):  # no reset bit; the custom bit
        changed = list(blobs)
        changed[long] = bytes([h0]) + blobs[long][1:]
        wants = [(INVALID_CONF, b"") if r[0] == long and r[2] else rule(datas, interval, r) for r in ranges]
        check(ranges_call(changed, first, off, interval, ranges, mem=mem), ranges, wants)
    changed = list(blobs)
    changed[long] = blobs[long][:1] + b"\x01" + blobs[long][2:]  # a second header byte that is not zero
    wants = [(INVALID_CONF, b"") if r[0] == long and r[2] else rule(datas, interval, r) for r in ranges]
    check(ranges_call(changed, first, off, interval, ranges, mem=mem), ranges, wants)
    # window 11 with max_window_bits = 10
    datas, blobs, first, off = batch(prose, interval, window=11)
    ranges = sweep(datas, interval) + [(len(datas), 0, 3)]
    wants = [(BAD_ARGUMENT, b"") if r[0] >= len(datas) else (INVALID_CONF, b"") if r[2] else (OK, b"") for r in ranges]
    check(ranges_call(blobs, first, off, interval, ranges, mem=mem, max_wbits=10), ranges, wants)
    check(ranges_call(blobs, first, off, interval, ranges, mem=mem, max_wbits=11), ranges, [rule(datas, interval, r) for r in ranges])


@pytest.mark.parametrize("mem", ["host", "device"])
def test_an_offset_out_of_the_window(ta, prose, mem):
    """A hand-built stream of three segments of 16 bytes, the middle one with a match that runs out of the window: TAMP_OOB for every
    range that touches it, the ranges of the segments around it and of the stream next to it are delivered."""
    interval, rng = 16, random.Random(5)
    w = TokenWriter(window=10, literal=8, extended=False, more=0)
    plain, entries = bytearray(), []
    for seg in range(3):
        for _ in range(13 if seg == 1 else interval):
            b = rng.randrange(32, 127)
            w.lit(b)
            plain.append(b)
        if seg == 1:
            w.match(w.W - 1, 3, check=False)  # offset + length beyond the window's end
            plain += b"???"
        if seg < 2:
            w.flush(), w.flush()
            assert w.bit % 8 == 0
            entries.append(w.bit // 8)
    hand = w.blob()
    datas, blobs, first, off = batch(prose, interval, lengths=[100], at=100)
    blobs2 = [hand, blobs[0]]
    first2 = np.array([0, 2, 2 + int(first[1])], dtype=np.uint64)
    off2 = np.concatenate([np.array(entries, dtype=np.uint32), off])
    datas2 = [bytes(plain), datas[0]]
    ranges = [(0, b, n) for b in range(0, 3 * interval + 2, 3) for n in (1, 5, interval, 40)] + [(1, 0, 100), (1, 17, 30)]
    wants = [(OOB, b"") if r[0] == 0 and 1 in touched(r, interval, 2) else rule(datas2, interval, r) for r in ranges]
    assert sum(w[0] == OOB for w in wants) > 10 and sum(w[0] == OK for w in wants) > 10
    check(ranges_call(blobs2, first2, off2, interval, ranges, mem=mem), ranges, wants)


# ---- slices ----

@pytest.mark.parametrize("mem", ["host", "device"])
def test_slices(ta, prose, mem, monkeypatch, capfd):
    interval = 1000
    datas, blobs, first, off = batch(prose, interval)
    long = max(range(len(datas)), key=lambda s: len(datas[s]))
    L = len(datas[long])
    ranges = [(long, q % 7, L) for q in range(80)] + [(s, 0, 10) for s in range(len(datas))]  # about 3.2 MB of scratch
    wants = [rule(datas, interval, r) for r in ranges]
    check(ranges_call(blobs, first, off, interval, ranges, mem=mem), ranges, wants)
    assert int(LINE.findall(capfd.readouterr().err)[-1][2]) == 1
    monkeypatch.setenv("TAMP_AMD_RANGES_SCRATCH_MB", "1")
    check(ranges_call(blobs, first, off, interval, ranges, mem=mem), ranges, wants)
    line = LINE.findall(capfd.readouterr().err)[-1]
    assert int(line[0]) == len(ranges) and int(line[2]) >= 3
    # one range that alone outgrows the budget is refused alone
    datas, blobs, first, off = batch(prose, interval, lengths=[5000, 1_000_000], at=0)
    ranges = [(0, 10, 2000), (1, 0, 1_000_000), (1, 999_000, 3000), (1, 1_000_000 - 10, 100), (0, 4990, 100)]
    wants = [rule(datas, interval, r) for r in ranges]
    wants[1] = (BAD_ARGUMENT, b"")
    check(ranges_call(blobs, first, off, interval, ranges, mem=mem), ranges, wants)


# ---- the Python surface ----

def test_python_surface(ta, prose, capfd):
    import torch

    interval = 1000
    datas = streams_of(prose, mixed(interval), at=3000)
    res = ta.compress_batch(datas, literal=7, dictionary_reset=True, reset_interval=interval, reset_index=True)
    assert (res.status == 0).all() and res.reset_index.interval == interval
    rng = random.Random(11)
    ranges = [(s, rng.randrange(0, len(datas[s]) + 50), rng.randrange(0, 2500)) for s in rng.choices(range(len(datas)), k=60)]
    stream_index, begin, length = ([r[k] for r in ranges] for k in range(3))
    want = [rule(datas, interval, r) for r in ranges]
    capfd.readouterr()
    r = ta.read_ranges(res.streams(), reset_index=res.reset_index, stream_index=stream_index, begin=begin, length=length)
    assert isinstance(r, ta.RangeResult) and r.ranges() == [w[1] for w in want] and r.status.tolist() == [w[0] for w in want]
    assert r.out_off.tolist() == np.concatenate([[0], np.cumsum(length)[:-1]]).tolist() and r.range(3) == want[3][1]
    # the host-memory call uploads the touched segments and a header each, nothing else of the streams
    staged, idx = 0, res.reset_index
    for s, b, n in ranges:
        E, f = entries_of(len(datas[s]), interval), int(idx.first[s])
        for k in touched((s, b, n), interval, E):
            start = 2 if k == 0 else int(idx.off[f + k - 1])
            staged += (int(idx.off[f + k]) if k < E else int(res.out_len[s])) - start + 2
    line = LINE.findall(capfd.readouterr().err)[-1]
    assert int(line[3]) == staged
    # numpy tables on the packed batch, and an interval that overrides the index's
    r2 = ta.read_ranges(res.out, res.out_off, res.out_len, reset_index=ta.ResetIndex(idx.first, idx.off, 77), reset_interval=interval,
                        stream_index=np.array(stream_index, np.uint32), begin=np.array(begin, np.uint64), length=np.array(length, np.uint32))
    assert r2.ranges() == r.ranges() and (r2.status == r.status).all()
    # CUDA tensors, asynchronous on a stream of the caller's
    dev = torch.device("cuda:0")
    flat, in_off, in_len = ta.pack_streams(res.streams())
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = [torch.from_numpy(a).to(dev) for a in (flat, in_off.view(np.int64), in_len.view(np.int32))]
        tr = [torch.tensor(x, dtype=dt, device=dev) for x, dt in ((stream_index, torch.int32), (begin, torch.int64), (length, torch.int32))]
    st.synchronize()
    r3 = ta.read_ranges(t[0], t[1], t[2], reset_index=idx, stream_index=tr[0], begin=tr[1], length=tr[2], stream=st.cuda_stream, timing=True)
    st.synchronize()
    assert r3.out.is_cuda and r3.ranges() == r.ranges() and r3.status.cpu().tolist() == r.status.tolist() and r3.kernel_ms > 0
    r4 = ta.read_ranges(t[0], t[1], t[2], reset_index=idx, stream_index=stream_index, begin=begin, length=length)
    torch.cuda.synchronize()
    assert r4.ranges() == r.ranges()
    assert ta.read_ranges(res.streams(), reset_index=idx, stream_index=[], begin=[], length=[]).ranges() == []
