"""GPU tier: byte ranges of streams whose reset segments differ in size (tamp_batch_segment_ends, tamp_batch_read_ranges_grid,
``ResetScan.segment_ends``, ``read_ranges(..., segment_ends=)``; the table policy of tamp_read_ranges_kernel.hpp and the kernels of
tamp_segment_ends_kernel.hpp, DESIGN.md 3.13 "Reading ranges").

The streams are made on the CPU by the checker's ``stream_script`` over the 7-bit prose fixture, with resets at places of their own;
the expectation is always the slice of the ORIGINAL input, never a GPU result.  Every range's room is laid out by hand behind 0xA5
guards at all four residues mod 4, the result tables are poisoned before the call, and afterwards the whole buffer is compared."""
import bisect
import ctypes as C

import numpy as np
import pytest
from test_gpu_batch_resets import CONFIGS, GUARD, layout
from test_gpu_read_ranges import BAD_ARGUMENT, BAD_INDEX, INPUT_EXHAUSTED, OK, check, ranges_call

pytestmark = pytest.mark.gpu

SATURATED = (1 << 64) - 1
TILE = 1024  # kResetScanTile


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
    for k in ("TAMP_AMD_RANGES_SCRATCH_MB", "TAMP_AMD_DECODER", "TAMP_AMD_RESETS_DEBUG"):
        monkeypatch.delenv(k, raising=False)


# Five streams of 0, 1, 2, 3 and 9 resets: the bytes written between them (two and three resets in a row, a reset first, a reset last).
SIZES = [[517], [0, 233], [700, 1, 0], [64, 0, 0, 399], [300, 0, 0, 41, 700, 3, 128, 64, 5, 57]]

_irregular = {}


def irregular(checker, prose, window=10, literal=8, extended=True, lazy=False):
    """(datas, blobs, the sizes written) of the five streams, made once per configuration by the checker."""
    key = (window, literal, extended, lazy)
    if key not in _irregular:
        datas, blobs, at = [], [], 7000
        for sizes in SIZES:
            ops = []
            for k, n in enumerate(sizes):
                ops += ([("reset",)] if k else []) + [("write", prose[at : at + n])]
                at += n + 11
            res, blob = checker.stream_script(ops + [("close",)], window=window, literal=literal, extended=extended, dictionary_reset=True,
                                              lazy_matching=lazy)
            assert res == 0
            datas.append(b"".join(op[1] for op in ops if op[0] == "write"))
            blobs.append(blob)
        _irregular[key] = (datas, blobs)
    return _irregular[key]


def geometry(scan, i):
    """B(0 .. K) of stream i from the scan's own sizes: B[k] the first decoded byte of segment k, B[K] the stream's size."""
    a, b = int(scan.index.first[i]), int(scan.index.first[i + 1])
    sizes = [int(x) for x in scan.closed_size[a:b]] + [int(scan.open_size[i])]
    return [0] + list(np.cumsum(sizes))


def checked_scan(ta, datas, blobs, written=None):
    """index_resets of the blobs, held against what was written: the sizes between resets, and the table of segment ends."""
    scan = ta.index_resets(blobs)
    assert (scan.status == 0).all()
    ends = scan.segment_ends()
    assert ends.dtype == np.uint64 and len(ends) == len(scan.index.off) + len(blobs) and scan.segment_ends() is ends
    for i, d in enumerate(datas):
        B = geometry(scan, i)
        row = int(scan.index.first[i]) + i
        assert B[-1] == len(d) and [int(x) for x in ends[row : row + len(B) - 1]] == B[1:]
        if written is not None:  # (a reset right behind a reset closes an empty segment)
            assert [s for s in np.diff(B) if s] == [s for s in written[i] if s], i
            assert len(B) - 1 >= len(written[i])
    return scan, ends


def grid_call(blobs, first, off, ends, ranges, *, mem="host", stream=None, max_wbits=15):
    """One tamp_batch_read_ranges_grid call on hand-laid tables; ``ranges``: (stream, begin, length) each.
    -> (rc, status, out_len, the output buffer, out_off)"""
    from tamp_amd import _lib
    from tamp_amd.batch import pack_streams

    lib = _lib.load()
    flat, in_off, in_len = pack_streams(blobs)
    nr = len(ranges)
    r_stream = np.array([r[0] for r in ranges], dtype=np.uint32)
    r_begin = np.array([r[1] for r in ranges], dtype=np.uint64)
    r_len = np.array([r[2] for r in ranges], dtype=np.uint32)
    out_off, total = layout([r[2] for r in ranges], [q % 4 for q in range(nr)])
    out = np.full(total, GUARD, dtype=np.uint8)
    out_len, status = np.full(nr, 0xDEAD, dtype=np.uint32), np.full(nr, 99, dtype=np.int8)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    no_off = len(off) == 0  # (a null reset_off: for an index without entries)
    off = np.zeros(1, np.uint32) if no_off else np.ascontiguousarray(off, dtype=np.uint32)
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    assert len(ends) == int(first[-1]) + len(blobs)
    tables = [flat, in_off, in_len, first, off, ends, r_stream, r_begin, r_len, out, out_off, out_len, status]
    if mem == "host":
        p = [a.ctypes.data_as(C.c_void_p) for a in tables]
        p[4] = None if no_off else p[4]
        rc = lib.tamp_batch_read_ranges_grid(max_wbits, *p, len(blobs), nr, _lib.MEM_HOST, 0, None)
        return rc, status, out_len, out, out_off
    import torch

    dev = torch.device("cuda:0")
    views = [None, np.int64, np.int32, np.int64, np.int32, np.int64, np.int32, np.int64, np.int32, None, np.int64, np.int32, None]
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        t = [torch.from_numpy(a.copy() if v is None else a.view(v).copy()).to(dev) for a, v in zip(tables, views)]
    torch.cuda.synchronize()
    p = [C.c_void_p(x.data_ptr()) for x in t]
    p[4] = None if no_off else p[4]
    rc = lib.tamp_batch_read_ranges_grid(max_wbits, *p, len(blobs), nr, _lib.MEM_DEVICE, 0,
                                         C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return rc, t[12].cpu().numpy(), t[11].cpu().numpy().view(np.uint32), t[9].cpu().numpy(), out_off


def rule(datas, r):
    """The table of the call for a true table: (status, bytes) of range ``r`` from the ORIGINAL input."""
    s, begin, length = r
    if s >= len(datas):
        return BAD_ARGUMENT, b""
    if length == 0:
        return OK, b""
    piece = datas[s][begin : begin + length]  # (begin >= total: no bytes, TAMP_INPUT_EXHAUSTED)
    return (OK if len(piece) == length else INPUT_EXHAUSTED), piece


def sweep(datas, scan):
    """Every boundary of every stream: begins at every B(k) - 1, B(k), B(k) + 1; one byte, all bytes, across 1, 2 and all segments, to
    the last byte and one past it, begin == total, len == 0; ranges that repeat and overlap."""
    ranges = []
    for s, d in enumerate(datas):
        B, L = geometry(scan, s), len(d)
        for k, b in enumerate(B):
            for begin in (b - 1, b, b + 1):
                if begin < 0:
                    continue
                lens = {1, 2}
                for ahead in (1, 2):  # to the end of this segment and of the next, exactly, one short and one past
                    e = B[min(k + ahead, len(B) - 1)]
                    lens |= {e - begin - 1, e - begin, e - begin + 1}
                lens |= {L - begin, L - begin + 1}
                ranges += [(s, begin, n) for n in sorted(x for x in lens if x > 0)]
        ranges += [(s, 0, L), (s, 0, L + 1), (s, 0, 1), (s, max(L - 1, 0), 1), (s, max(L - 1, 0), 2), (s, L, 1), (s, L, 0), (s, L + 5, 3), (s, 3, 0),
                   (s, 1 << 40, 7), (s, SATURATED, 1), (s, SATURATED - 1, 9)]
    ranges += ranges[5:25] + [(len(datas), 0, 1), (len(datas), 0, 0), (4, 290, 500), (4, 300, 400), (4, 200, 900), (4, 290, 500)]
    return ranges


def stream1():
    import torch

    return torch.cuda.Stream()


# ---- irregular streams: every boundary, on every configuration, from host and device memory ----

@pytest.mark.parametrize("window,literal,extended,lazy", [c for c in CONFIGS if c[0] in (8, 10)])
def test_irregular_streams(ta, checker, prose, window, literal, extended, lazy):
    datas, blobs = irregular(checker, prose, window, literal, extended, lazy)
    scan, ends = checked_scan(ta, datas, blobs, SIZES)
    assert scan.index.interval is None
    assert [int(scan.index.first[i + 1] - scan.index.first[i]) >= len(SIZES[i]) - 1 for i in range(5)] == [True] * 5
    with pytest.raises(ValueError, match="not given and not in the index"):  # (what the caller was left with)
        ta.read_ranges(blobs, reset_index=scan.index, stream_index=[0], begin=[0], length=[1])
    ranges = sweep(datas, scan)
    wants = [rule(datas, r) for r in ranges]
    assert {w[0] for w in wants} == {OK, INPUT_EXHAUSTED, BAD_ARGUMENT} and any(w[0] == INPUT_EXHAUSTED and w[1] for w in wants)
    check(grid_call(blobs, scan.index.first, scan.index.off, ends, ranges), ranges, wants)
    check(grid_call(blobs, scan.index.first, scan.index.off, ends, ranges, mem="device", stream=stream1() if lazy or literal == 7 else None),
          ranges, wants)


def test_python_surface_host_and_device(ta, checker, prose):
    """``read_ranges(..., segment_ends=)`` on lists, numpy tables and CUDA tensors (index -> table -> ranges on the device, on a side
    stream too), an interval that is given being ignored; the memory-kind refusal."""
    import torch

    datas, blobs = irregular(checker, prose)
    scan, ends = checked_scan(ta, datas, blobs, SIZES)
    ranges = [r for r in sweep(datas, scan) if r[0] < len(datas)][::7]
    wants = [rule(datas, r) for r in ranges]
    args = dict(stream_index=[r[0] for r in ranges], begin=[r[1] for r in ranges], length=[r[2] for r in ranges])

    def held(res):
        assert [int(x) for x in res.status] == [w[0] for w in wants]
        assert res.ranges() == [w[1] for w in wants]

    held(ta.read_ranges(blobs, reset_index=scan.index, segment_ends=ends, **args))
    held(ta.read_ranges(blobs, reset_index=scan.index, segment_ends=[int(x) for x in ends], reset_interval=1, **args))
    flat, in_off, in_len = ta.pack_streams(blobs)
    held(ta.read_ranges(flat, in_off, in_len, reset_index=scan.index, segment_ends=ends, **args))
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(flat).to(dev), torch.from_numpy(in_off.view(np.int64)).to(dev), torch.from_numpy(in_len.view(np.int32)).to(dev)]
    with pytest.raises(ValueError, match="another memory kind"):
        ta.read_ranges(*t, reset_index=scan.index, segment_ends=ends, **args)
    with pytest.raises(ValueError, match="another memory kind"):
        ta.read_ranges(flat, in_off, in_len, reset_index=scan.index, segment_ends=torch.from_numpy(ends.view(np.int64)).to(dev), **args)
    for side in (None, stream1()):
        st = side.cuda_stream if side is not None else None
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())
        dscan = ta.index_resets(*t, stream=st)
        dends = dscan.segment_ends(stream=st)
        assert dends.is_cuda and dends.dtype == torch.int64 and dscan.segment_ends() is dends
        res = ta.read_ranges(*t, reset_index=dscan.index, segment_ends=dends, stream=st, **args)
        torch.cuda.synchronize()
        assert dends.cpu().numpy().view(np.uint64).tolist() == ends.tolist()
        held(res)
    import tamp

    assert tamp.segment_ends(scan.index.first, scan.closed_size, scan.open_size).tolist() == ends.tolist()


def test_reference_made_append_mode_file(ta, checker, prose):
    """A log a reference compressor wrote: one session that made the file, three more written with ``append=True`` and concatenated.
    Every session is readable by range, alone and across the session boundaries."""
    sessions = [prose[20000 + 900 * j : 20000 + 900 * j + n] for j, n in enumerate((400, 650, 1, 333))]
    res, blob = checker.stream_script([("write", sessions[0]), ("close",)], window=10, literal=7, dictionary_reset=True)
    assert res == 0
    for s in sessions[1:]:
        res, more = checker.stream_script([("write", s), ("close",)], window=10, literal=7, dictionary_reset=True, append=True)
        assert res == 0
        blob += more
    data = b"".join(sessions)
    res, plain = checker.stream_script([("write", prose[:100]), ("close",)], window=10, literal=7)
    assert res == 0
    scan, ends = checked_scan(ta, [data], [blob], [[len(s) for s in sessions]])
    starts = [0] + list(np.cumsum([len(s) for s in sessions]))
    ranges = [(0, starts[j], len(s)) for j, s in enumerate(sessions)]  # every session, whole
    ranges += [(0, starts[j] + len(s) // 2, 40) for j, s in enumerate(sessions)] + [(0, starts[j] - 3, 9) for j in (1, 2, 3)]
    ranges += [(0, 0, len(data)), (0, 5, len(data)), (0, len(data) - 1, 1), (0, len(data), 1), (0, starts[2] - 1, len(sessions[2]) + 2)]
    wants = [rule([data], r) for r in ranges]
    assert [w[1] for w in wants[:4]] == sessions
    for mem in ("host", "device"):
        check(grid_call([blob], scan.index.first, scan.index.off, ends, ranges, mem=mem), ranges, wants)
    # next to a stream without the reset bit: that one is refused alone
    scan2 = ta.index_resets([plain, blob])
    res = ta.read_ranges([plain, blob], reset_index=scan2.index, segment_ends=scan2.segment_ends(), stream_index=[0, 1], begin=[0, starts[3]],
                         length=[10, len(sessions[3])])
    assert [int(x) for x in res.status] == [-3, OK] and res.ranges() == [b"", sessions[3]]


def test_cli_read(ta, checker, prose, tmp_path):
    from tamp_amd import cli

    datas, blobs = irregular(checker, prose)
    f, out = tmp_path / "log.tamp", tmp_path / "piece.bin"
    f.write_bytes(blobs[4])
    assert cli.main(["read", str(f), "--begin", "290", "--length", "800", "-o", str(out)]) == 0
    assert out.read_bytes() == datas[4][290:1090]
    assert cli.main(["read", str(f), "--begin", str(len(datas[4]) - 5), "--length", "800", "-o", str(out)]) == 0
    assert out.read_bytes() == datas[4][-5:]
    assert cli.main(["read", str(f), "--begin", str(len(datas[4])), "--length", "1", "-o", str(out)]) == 0 and out.read_bytes() == b""


# ---- mixed intervals: two regular batches merged into one call ----

def regular_ends(datas, first, interval):
    """The table of a batch compressed with one interval, from its index and lengths."""
    ends = []
    for i, d in enumerate(datas):
        E = int(first[i + 1] - first[i])
        ends += [(k + 1) * interval for k in range(E)] + [len(d)]
    return np.array(ends, dtype=np.uint64)


def test_mixed_intervals(ta, prose):
    lengths = ([0, 1, 511, 512, 513, 1024, 1025, 5000, 0, 512], [0, 1, 767, 768, 769, 1536, 1537, 5000, 768, 3])
    parts = []
    for interval, lens in zip((512, 768), lengths):
        datas = [prose[40000 + 6000 * j : 40000 + 6000 * j + n] for j, n in enumerate(lens)]
        res = ta.compress_batch(datas, dictionary_reset=True, reset_interval=interval, reset_index=True, literal=7)
        assert (res.status == 0).all() and res.reset_index.interval == interval
        parts.append((interval, datas, res.streams(), np.asarray(res.reset_index.first, np.uint64), np.asarray(res.reset_index.off, np.uint32)))
    (n0, d0, b0, f0, o0), (n1, d1, b1, f1, o1) = parts
    first = np.concatenate([f0, f1[1:] + f0[-1]])
    off = np.concatenate([o0, o1])
    ends = np.concatenate([regular_ends(d0, f0, n0), regular_ends(d1, f1, n1)])
    assert ta.segment_ends(f0, np.full(len(o0), n0, np.uint32), np.array([len(d) - n0 * int(f0[i + 1] - f0[i]) for i, d in enumerate(d0)], np.uint32)
                           ).tolist() == regular_ends(d0, f0, n0).tolist()
    alone, merged = [], []
    for base, (interval, datas, blobs, f, o) in zip((0, len(d0)), parts):
        ranges = []
        for s, d in enumerate(datas):
            L, E = len(d), int(f[s + 1] - f[s])
            begins = {0, 1, L - 1, L, L + 1, (E + 1) * interval, (E + 2) * interval} | {k * interval + x for k in (1, max(E, 1)) for x in (-1, 0, 1)}
            ranges += [(s, b, n) for b in sorted(x for x in begins if x >= 0) for n in (0, 1, interval - 1, interval, interval + 1, 2 * interval + 1, L + 5)]
        got = ranges_call(blobs, f, o, interval, ranges)  # what tamp_batch_read_ranges gives the batch alone ...
        check(got, ranges, [rule(datas, r) for r in ranges])  # (... which is the slice of the input)
        alone.append((ranges, got))
        merged += [(s + base, b, n) for s, b, n in ranges]
    for mem in ("host", "device"):
        rc, status, out_len, out, out_off = grid_call(b0 + b1, first, off, ends, merged, mem=mem)
        assert rc == 0
        q = 0
        for ranges, (_, a_status, a_len, a_out, a_off) in alone:
            for j, r in enumerate(ranges):
                assert (int(status[q]), int(out_len[q])) == (int(a_status[j]), int(a_len[j])), (mem, q, r)
                o, ao, n = int(out_off[q]), int(a_off[j]), int(a_len[j])
                assert out[o : o + n].tobytes() == a_out[ao : ao + n].tobytes(), (mem, q, r)
                q += 1
        check((rc, status, out_len, out, out_off), merged, [rule(d0 + d1, r) for r in merged])


# ---- the scan: tamp_batch_segment_ends against numpy ----

def ends_of(first, closed, opens):
    want = []
    for i in range(len(opens)):
        run, dead = 0, False
        for s in [int(x) for x in closed[int(first[i]) : int(first[i + 1])]] + [int(opens[i])]:
            dead |= s == 0xFFFFFFFF
            run += s
            want.append(SATURATED if dead else run)
    return want


def ends_call(first, closed, opens, mem):
    """One tamp_batch_segment_ends call with the table behind guard words.  -> (rc, the table with its guards)"""
    from tamp_amd import _lib

    lib = _lib.load()
    n, rows = len(opens), len(closed) + len(opens)
    room = np.full(rows + 16, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    closed_or_one = closed if len(closed) else np.zeros(1, np.uint32)
    if mem == "host":
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = lib.tamp_batch_segment_ends(p(first), p(closed) if len(closed) else None, p(opens), p(room[8:]), n, _lib.MEM_HOST, 0, None)
        return rc, room
    import torch

    dev = torch.device("cuda:0")
    t = [torch.from_numpy(a.view(v).copy()).to(dev) for a, v in ((first, np.int64), (closed_or_one, np.int32), (opens, np.int32), (room, np.int64))]
    torch.cuda.synchronize()
    rc = lib.tamp_batch_segment_ends(C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()), C.c_void_p(t[2].data_ptr()),
                                     C.c_void_p(t[3].data_ptr() + 64), n, _lib.MEM_DEVICE, 0, None)
    torch.cuda.synchronize()
    return rc, t[3].cpu().numpy().view(np.uint64)


def scan_batches():
    rng = np.random.default_rng(11)
    out = {}
    for name, counts in (("1 stream", [3]), ("1 stream, no entries", [0]), ("3,000 streams", rng.integers(0, 6, 3000)),
                         ("1,025 entries", [1025]), ("2,500 entries", [2500]),
                         # a long stream that starts inside a tile, ends at a tile's last row, or starts at a tile's first row
                         ("inside", [2, 0, 5] + [1025] + [1, 0]), ("to a tile's end", [4, 2 * TILE - 6, 0, 3]),
                         ("from a tile's start", [TILE - 1, 2500, 0, 0, 2]), ("no stream has entries", [0] * 40)):
        counts = np.asarray(counts, dtype=np.int64)
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        closed = rng.integers(0, 701, int(first[-1])).astype(np.uint32)
        opens = rng.integers(0, 701, len(counts)).astype(np.uint32)
        out[name] = (first, closed, opens)
    first, closed, opens = (a.copy() for a in out["inside"])
    closed[int(first[3]) + 700] = 0xFFFFFFFF  # (saturated from inside the long stream to its end, across a tile; the next stream starts anew)
    opens[0] = 0xFFFFFFFF
    out["saturated"] = (first, closed, opens)
    return out


@pytest.mark.parametrize("name", list(scan_batches()))
def test_segment_ends_against_numpy(ta, name):
    first, closed, opens = scan_batches()[name]
    want = ends_of(first, closed, opens)
    if name == "to a tile's end":
        assert int(first[2]) + 2 == 2 * TILE  # (the long stream's open row is a tile's last)
    if name == "from a tile's start":
        assert int(first[1]) + 1 == TILE
    if name == "saturated":
        assert want.count(SATURATED) == 1 + (1025 - 700 + 1) and want[-1] != SATURATED
    for mem in ("host", "device"):
        rc, room = ends_call(first, closed, opens, mem)
        assert rc == 0
        assert [int(x) for x in room[8 : 8 + len(want)]] == want, (name, mem)
        assert (room[:8] == 0xA5A5A5A5A5A5A5A5).all() and (room[8 + len(want) :] == 0xA5A5A5A5A5A5A5A5).all(), (name, mem)


# ---- the count kernel's tile: more ranges than one step of its scan ----

def test_more_ranges_than_a_scan_tile(ta, checker, prose):
    datas, blobs = irregular(checker, prose)
    scan, ends = checked_scan(ta, datas, blobs, SIZES)
    rng = np.random.default_rng(5)
    ranges = []
    for q in range(TILE + 1):
        s = int(rng.integers(0, 5))
        ranges.append((s, int(rng.integers(0, len(datas[s]) + 2)), int(rng.integers(0, 300))))
    wants = [rule(datas, r) for r in ranges]
    for mem in ("host", "device"):
        check(grid_call(blobs, scan.index.first, scan.index.off, ends, ranges, mem=mem), ranges, wants)


# ---- forged tables ----

def touches(B, r, segments):
    """Range ``r`` of a stream with the TRUE geometry B touches one of ``segments`` (empty segments between its ends count)."""
    _, begin, length = r
    if length == 0 or begin >= B[-1]:
        return False
    end = min(begin + length, B[-1])
    k0, k1 = bisect.bisect_right(B, begin) - 1, bisect.bisect_right(B, end - 1) - 1
    return any(k0 <= k <= k1 for k in segments)


def test_forged_tables(ta, checker, prose):
    """The table is verified on what is touched: a forged entry refuses exactly the ranges that touch its segments; every other
    range of the call is delivered in full, and nothing is written outside a delivered range."""
    datas, blobs = irregular(checker, prose)
    scan, ends = checked_scan(ta, datas, blobs, SIZES)
    s = 4
    B = geometry(scan, s)
    K, row = len(B) - 1, int(scan.index.first[s]) + s
    sizes = list(np.diff(B))
    k = sizes.index(128)  # segments 3, 128, 64, 5 lie around it: entry k ends the segment of 128 bytes
    assert sizes[k - 1 : k + 3] == [3, 128, 64, 5] and K - 1 > k + 2 and sizes[-1] == 57 and sizes[-2] == 5  # (the open segment: 57 bytes)
    ranges = [r for r in sweep(datas, scan) if r[0] < 5 and r[2]]
    truth = [rule(datas, r) for r in ranges]

    def forged(change, bad_segments, total=None):
        t = ends.copy()
        change(t)
        wants, refused = [], 0
        for r, w in zip(ranges, truth):
            if r[0] != s:
                wants.append(w)
            elif total is not None and r[1] >= total:  # (answered from the table alone)
                wants.append((INPUT_EXHAUSTED, b""))
            elif touches(B[:-1] + [max(B[-1], total or 0)], r, bad_segments):
                wants.append((BAD_INDEX, b"")), (refused := refused + 1)
            else:
                wants.append(w)
        assert refused and any(w[0] == OK and w[1] for r, w in zip(ranges, wants) if r[0] == s)
        for mem in ("host", "device"):
            check(grid_call(blobs, scan.index.first, scan.index.off, t, ranges, mem=mem), ranges, wants)

    def set_entry(j, v):
        return lambda t: t.__setitem__(row + j, v)

    forged(set_entry(k, B[k + 1] + 1), {k, k + 1})  # one entry off by one, up: its segment grows, the next one shrinks
    forged(set_entry(k, B[k + 1] - 1), {k, k + 1})  # ... and down

    def swap(t):
        t[row + k], t[row + k + 1] = t[row + k + 1], t[row + k]

    forged(swap, {k, k + 1, k + 2})  # two entries swapped: the table is not sorted there
    forged(set_entry(K - 1, B[K] + 1), {K - 1}, total=B[K] + 1)  # the open segment's end too large
    forged(set_entry(K - 1, B[K] - 1), {K - 1}, total=B[K] - 1)  # ... and too small
    forged(set_entry(K - 2, SATURATED), {K - 2, K - 1})  # an entry of 2^64 - 1: its segment, and the one that starts there
