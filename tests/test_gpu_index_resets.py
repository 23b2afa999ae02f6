"""GPU tier: the reset index of streams that came without one (tamp_batch_index_resets, ``index_resets``; the kernels of
tamp_reset_index_kernel.hpp, DESIGN.md 3.13 "Finding the resets of a batch").

The expectation is always the CPU token reader's (``read_tokens`` of long_stream_writer.py): a reset is an F token that follows an
F, its offset is (bit + nbits) >> 3, sizes are sums of ``produced``.  The input tables are laid out by hand, streams at every residue
mod 4 of the flat buffer; the four result tables sit in 0xEE fill between guard words that must survive."""
import ctypes as C
import random
import re

import numpy as np
import pytest
from long_stream_writer import TokenWriter, mixed, oob, read_tokens

pytestmark = pytest.mark.gpu

OK, INPUT_EXHAUSTED, INVALID_CONF, OOB, BAD_ARGUMENT = 0, 2, -3, -4, -21
CB = 1024  # TAMP_AMD_INDEX_RESETS_CHUNK_BITS (asserted against the binding below)
FILL, GUARD_WORDS = 0xEE, 4
LINE = re.compile(r"\[tamp_amd resets\] index: (\d+) streams, (\d+) chunks, (\d+) rounds, (\d+) entries$", re.M)
DECODE = re.compile(r"\[tamp_amd resets\] batch decode: (\d+) streams, (\d+) split into (\d+) units, (\d+) whole$", re.M)


@pytest.fixture(scope="module")
def ta():
    import tamp_amd
    from tamp_amd import _lib

    _lib.load()  # raises if the native library is missing: no silent fallback
    assert _lib.INDEX_RESETS_CHUNK_BITS == CB
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
    monkeypatch.delenv("TAMP_AMD_DECODER", raising=False)
    monkeypatch.setenv("TAMP_AMD_RESETS_DEBUG", "1")


def truth(blob, max_wbits=15):
    """(status, reset offsets, closed sizes, open size) of one stream from the CPU token reader and the call's table of rules."""
    n = len(blob)
    if n == 0 or n < 1 + (blob[0] & 1):
        return INPUT_EXHAUSTED, [], [], 0
    if (blob[0] & 1 and blob[1]) or ((blob[0] >> 5) & 7) + 8 > max_wbits:
        return INVALID_CONF, [], [], 0
    toks, window = read_tokens(blob)[:2]
    offs, closed, seg, prev = [], [], 0, False
    for tk in toks:
        flush = tk.kind == "F" and bool(blob[0] & 1)  # (no reset bit: no resets)
        if flush and prev:
            offs.append((tk.bit + tk.nbits) >> 3)
            closed.append(seg)
            seg = 0
        seg, prev = seg + tk.produced, flush
    return (OOB if any(oob(tk, window) for tk in toks) else OK), offs, closed, seg


def guarded(count, dtype):
    """A table of ``count`` entries in 0xEE fill between guard words of 0x5A bytes -> (the whole array, the table's view)."""
    size = np.dtype(dtype).itemsize
    whole = np.frombuffer(bytes([0x5A]) * (GUARD_WORDS * size) + bytes([FILL]) * (count * size) + bytes([0x5A]) * (GUARD_WORDS * size), dtype=dtype).copy()
    return whole, whole[GUARD_WORDS : GUARD_WORDS + count]


def guards_intact(whole, count):
    g = whole[0]
    return bool((whole[:GUARD_WORDS] == g).all() and (whole[GUARD_WORDS + count:] == g).all())


def index_call(blobs, *, cap, mem="host", stream=None, max_wbits=15, null_off=False, with_sizes=True):
    """One tamp_batch_index_resets call on hand-laid tables.  -> (rc, reset_first, reset_off, closed_size, open_size, status), the
    entry tables ``cap`` long; the guard words around every table are asserted here."""
    from tamp_amd import _lib

    lib = _lib.load()
    n = len(blobs)
    in_off, in_len, at = np.zeros(n, np.uint64), np.zeros(n, np.uint32), 5
    for i, b in enumerate(blobs):  # streams at every residue mod 4, a few bytes of another value between them
        at += (i - at) % 4
        in_off[i], in_len[i] = at, len(b)
        at += len(b) + 3
    flat = np.full(at + 8, 0xC3, dtype=np.uint8)
    for i, b in enumerate(blobs):
        flat[int(in_off[i]) : int(in_off[i]) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    assert n < 4 or {int(o) % 4 for o in in_off} == {0, 1, 2, 3}
    wholes, views = zip(guarded(n + 1, np.uint64), guarded(cap, np.uint32), guarded(cap, np.uint32), guarded(n, np.uint32), guarded(n, np.int8))
    counts = (n + 1, cap, cap, n, n)
    use = [True, not null_off, with_sizes and not null_off, with_sizes, True]
    if mem == "host":
        p = [w[GUARD_WORDS:].ctypes.data_as(C.c_void_p) if u else None for w, u in zip(wholes, use)]
        rc = lib.tamp_batch_index_resets(max_wbits, flat.ctypes.data_as(C.c_void_p), in_off.ctypes.data_as(C.c_void_p),
                                         in_len.ctypes.data_as(C.c_void_p), p[0], p[1], p[2], p[3], 0 if null_off else cap, p[4], n,
                                         _lib.MEM_HOST, 0, None)
        got = wholes
    else:
        import torch

        dev = torch.device("cuda:0")
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
            t_in = [torch.from_numpy(a).to(dev) for a in (flat, in_off.view(np.int64), in_len.view(np.int32))]
            t = [torch.from_numpy(w.view(np.uint8).copy()).to(dev) for w in wholes]
        torch.cuda.synchronize()
        p = [C.c_void_p(x.data_ptr() + GUARD_WORDS * w.dtype.itemsize) if u else None for x, w, u in zip(t, wholes, use)]
        rc = lib.tamp_batch_index_resets(max_wbits, C.c_void_p(t_in[0].data_ptr()), C.c_void_p(t_in[1].data_ptr()), C.c_void_p(t_in[2].data_ptr()),
                                         p[0], p[1], p[2], p[3], 0 if null_off else cap, p[4], n, _lib.MEM_DEVICE, 0,
                                         C.c_void_p(stream.cuda_stream) if stream is not None else None)
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize()
        got = [x.cpu().numpy().view(w.dtype) for x, w in zip(t, wholes)]
    for w, count in zip(got, counts):
        assert guards_intact(w, count), "a guard word was written"
    return (rc,) + tuple(w[GUARD_WORDS : GUARD_WORDS + count] for w, count in zip(got, counts))


def check(res, blobs, max_wbits=15):
    """All five tables against the CPU truth; what lies behind the entries stays 0xEE."""
    rc, first, off, closed, open_size, status = res
    want = [truth(b, max_wbits) for b in blobs]
    assert rc == 0
    assert status.tolist() == [w[0] for w in want], [(i, int(s), w[0]) for i, (s, w) in enumerate(zip(status, want)) if int(s) != w[0]]
    assert first.tolist() == np.concatenate([[0], np.cumsum([len(w[1]) for w in want])]).tolist()
    for i, w in enumerate(want):
        a, b = int(first[i]), int(first[i + 1])
        assert off[a:b].tolist() == w[1], ("offsets of stream", i)
        assert closed[a:b].tolist() == w[2], ("closed sizes of stream", i)
        assert int(open_size[i]) == w[3], ("open size of stream", i, int(open_size[i]), w[3])
    E = int(first[-1])
    assert (off[E:].view(np.uint8) == FILL).all() and (closed[E:].view(np.uint8) == FILL).all()
    return want


def entries(blobs, max_wbits=15):
    return sum(len(truth(b, max_wbits)[1]) for b in blobs)


MODES = [("host", False), ("device", False), ("device", True)]


def run_modes(blobs, max_wbits=15, slack=3):
    import torch

    out = []
    for mem, own_stream in MODES:
        st = torch.cuda.Stream() if own_stream else None
        out.append(check(index_call(blobs, cap=entries(blobs, max_wbits) + slack, mem=mem, stream=st, max_wbits=max_wbits), blobs, max_wbits))
    return out[0]


def spliced(w, rng, chunks):
    """``mixed`` tokens with resets spliced in at random, ending in chunk ``chunks`` - 1: a stream of exactly ``chunks`` chunks."""
    while w.bit < chunks * CB - 400:
        mixed(w, rng, min(w.bit + rng.randrange(100, 4000), chunks * CB - 400))
        for _ in range(rng.choice((2, 2, 2, 3))):
            w.flush()
    w.plain_until(chunks * CB - 60, rng)
    blob = w.blob()
    assert (8 * len(blob) + CB - 1) // CB == chunks
    return blob


def hand_built():
    """(name, blob) of every designed stream of test 1, all at windows <= 11."""
    rng = random.Random(41)
    new = lambda window=10, literal=8, extended=True, **kw: TokenWriter(window, literal, extended, more=0, **kw)  # noqa: E731
    out = []
    w = new()  # stream 0: its chunks are the batch's, so its chunk 63|64 is a workgroup's edge
    w.fill_to(5 * CB - 16, rng)
    w.flush()
    assert w.bit == 5 * CB
    w.flush()  # the first token of chunk 5: a reset across a chunk boundary
    w.fill_to(64 * CB - 16, rng)
    w.flush()
    assert w.bit == 64 * CB
    w.flush()  # ... across a workgroup's
    w.plain_until(66 * CB, rng)
    out.append(("boundaries", w.blob()))
    w = new(11, 7, False)
    w.plain_until(700, rng)
    for _ in range(3):
        w.flush()
    w.plain_until(2000, rng)
    out.append(("three in a row", w.blob()))
    w = new(9)
    w.fill_to(2 * CB, rng)
    for _ in range(41):
        w.flush()
    assert w.bit == 2 * CB + 41 * 16 < 3 * CB
    w.plain_until(3 * CB + 100, rng)
    out.append(("40 resets in one chunk", w.blob()))
    w = new()
    w.fill_to(800, rng)
    w.flush()
    w.plain_until(1500, rng)
    out.append(("a lone FLUSH", w.blob()))
    w = new(8, 6)
    w.plain_until(300, rng)
    w.flush()
    w.lit(65)
    w.flush()
    w.plain_until(900, rng)
    out.append(("FLUSH, plain, FLUSH", w.blob()))
    for chunks in (63, 64, 65, 129):
        out.append(("%d chunks" % chunks, spliced(new(10, 8, chunks % 2 == 1), rng, chunks)))
    w = new()
    w.plain_until(1200, rng)
    w.flush(), w.flush()
    w.plain_until(2000, rng)
    w.match(17, 9)
    blob = w.blob()
    cut = blob[: (w.tokens[-1].bit + 10) // 8]
    assert len(read_tokens(cut)[0]) == len(w.tokens) - 1
    out.append(("cut inside its last token", cut))
    out.append(("a header and nothing else", new().blob()))
    out.append(("one byte", new().blob()[:1]))
    out.append(("no byte", b""))

    def flushes(w):
        w.plain_until(w.bit + 300, random.Random(7), literals=True)
        w.flush(), w.flush(), w.flush()
        w.plain_until(w.bit + 300, random.Random(8), literals=True)
        return w.blob()

    with_bit, without = flushes(new()), flushes(TokenWriter(10, 8, True))
    assert without[0] == with_bit[0] & 0xFE and len(truth(with_bit)[1]) == 2
    out.append(("FLUSH FLUSH without the reset bit", without))
    out.append(("the custom bit", flushes(new(custom=True))))
    out.append(("window 12", flushes(new(12))))
    out.append(("a second header byte", flushes(TokenWriter(10, 8, True, more=1))))
    w = new()
    w.plain_until(500, rng)
    w.flush(), w.flush()
    w.match(w.W + 1 - 5, 5, check=False)
    w.plain_until(1400, rng)
    w.flush(), w.flush()
    w.plain_until(1800, rng)
    out.append(("an offset out of the window", w.blob()))
    return out


def test_hand_built_streams_in_one_batch(ta):
    """Every designed stream in ONE batch at max_window_bits = 11, through the host-memory call, the device-memory call and a
    stream of the caller's: offsets, closed and open sizes and status equal the token reader's."""
    named = hand_built()
    blobs = [b for _, b in named]
    want = dict(zip([k for k, _ in named], run_modes(blobs, max_wbits=11)))
    assert len(want["boundaries"][1]) == 2 and want["boundaries"][1] == [5 * CB // 8 + 2, 64 * CB // 8 + 2]
    assert len(want["three in a row"][1]) == 2 and want["three in a row"][2][1] == 0
    assert len(want["40 resets in one chunk"][1]) == 40 and len(want["a lone FLUSH"][1]) == 0 and len(want["FLUSH, plain, FLUSH"][1]) == 0
    assert all(len(want["%d chunks" % c][1]) >= 5 for c in (63, 64, 65, 129))
    assert want["cut inside its last token"][0] == OK and len(want["cut inside its last token"][1]) == 1
    assert want["a header and nothing else"] == (OK, [], [], 0)
    assert want["one byte"][0] == want["no byte"][0] == INPUT_EXHAUSTED
    assert want["FLUSH FLUSH without the reset bit"][:3] == (OK, [], []) and want["FLUSH FLUSH without the reset bit"][3] > 0
    assert want["the custom bit"][0] == OK and len(want["the custom bit"][1]) == 2
    assert want["window 12"][0] == want["a second header byte"][0] == INVALID_CONF
    assert want["an offset out of the window"][0] == OOB and len(want["an offset out of the window"][1]) == 2


def test_periodic_stream_settles_within_the_bound(ta, capfd):
    """One token repeated over 200 chunks, then a reset: a parse from a wrong phase never falls back into step, so the right starts
    travel a workgroup per round.  The bound as implemented: for a longest stream of c chunks at most ceil(c / 64) + 1 rounds until
    every start is right (the stream's chunk 0 need not be a workgroup's first), plus the one round that finds nothing moved."""
    rng = random.Random(42)
    blobs = []
    for extended in (True, False):
        w = TokenWriter(10, 8, extended, more=0)
        while w.bit < 200 * CB - 24:
            w.match(0, 13 if extended else 15)
        w.flush(), w.flush()
        w.plain_until(w.bit + 700, rng)
        blobs.append(w.blob())
    for blob in blobs:
        capfd.readouterr()
        want = check(index_call([b"\x59\x00" + bytes(37), blob], cap=5), [b"\x59\x00" + bytes(37), blob])
        m = LINE.search(capfd.readouterr().err)
        chunks = (8 * len(blob) + CB - 1) // CB
        assert m and int(m[1]) == 2 and int(m[2]) == chunks + 1 and int(m[4]) == 1 == len(want[1][1])
        assert chunks >= 200 and 2 <= int(m[3]) <= -(-chunks // 64) + 1 + 1
    run_modes(blobs)


def test_every_configuration(ta):
    """Windows 8..15, literals 5..8, both formats: 64 short streams of at most 3 chunks with two or three resets each."""
    blobs = []
    for window in range(8, 16):
        for literal in range(5, 9):
            for extended in (False, True):
                rng = random.Random(1000 * window + 10 * literal + extended)
                w = TokenWriter(window, literal, extended, more=0)
                for _ in range(rng.choice((2, 3))):
                    mixed(w, rng, w.bit + rng.randrange(40, 600))
                    w.flush(), w.flush()
                mixed(w, rng, w.bit + rng.randrange(0, 300))
                assert 8 * len(w.blob()) <= 3 * CB
                blobs.append(w.blob())
    want = run_modes(blobs)
    assert all(s == OK and len(o) >= 2 for s, o, _, _ in want)


def test_capacity(ta):
    """One entry of room too few, and no room at all: 1, the per-stream tables complete, no byte of the entry tables written."""
    rng = random.Random(43)
    blobs = [b for _, b in hand_built()[1:6]] + [spliced(TokenWriter(10, 8, True, more=0), rng, 9)]
    E = entries(blobs)
    assert E > 45
    full = check(index_call(blobs, cap=E), blobs)
    for mem, own in MODES:
        import torch

        for kw in (dict(cap=E - 1), dict(cap=E, null_off=True), dict(cap=1)):
            rc, first, off, closed, open_size, status = index_call(blobs, mem=mem, stream=torch.cuda.Stream() if own else None, **kw)
            assert rc == 1
            assert first.tolist() == np.concatenate([[0], np.cumsum([len(w[1]) for w in full])]).tolist()
            assert status.tolist() == [w[0] for w in full] and open_size.tolist() == [w[3] for w in full]
            assert (off.view(np.uint8) == FILL).all() and (closed.view(np.uint8) == FILL).all()
        # only the offsets asked for: the size tables stay as they were
        rc, first, off, closed, open_size, status = index_call(blobs, cap=E, mem=mem, with_sizes=False)
        assert rc == 0 and off.tolist() == [o for w in full for o in w[1]]
        assert (closed.view(np.uint8) == FILL).all() and (open_size.view(np.uint8) == FILL).all()


def test_the_wrapper_calls_again_with_the_exact_count(ta, capfd):
    """300 resets back to back in about 1 KiB: more than the first call's max(n, total_bytes >> 12) entries of room."""
    w = TokenWriter(10, 8, True, more=0)
    w.lit(66)
    for _ in range(301):
        w.flush()
    w.lit(67)
    blobs = [w.blob(), b"\x59\x00"]
    assert len(blobs[0]) < 1024 and entries(blobs) == 300 > max(len(blobs), sum(map(len, blobs)) >> 12)
    capfd.readouterr()
    scan = ta.index_resets(blobs)
    lines = LINE.findall(capfd.readouterr().err)
    assert len(lines) == 2 and all(int(x[3]) == 300 for x in lines)
    want = truth(blobs[0])
    assert scan.index.first.tolist() == [0, 300, 300] and scan.index.off.tolist() == want[1] and scan.closed_size.tolist() == want[2]
    assert scan.status.tolist() == [OK, OK] and scan.size(0) == 2 and scan.size(1) == 0 and scan.index.interval is None


N = 4096


@pytest.mark.parametrize("conf", [dict(window=10, literal=8, extended=True), dict(window=12, literal=7, extended=False)],
                         ids=["w10 l8 ext", "w12 l7 v1"])
def test_against_the_compressor(ta, prose, capfd, conf):
    """Streams compressed with reset_interval = N: the found index is the compressor's, the sizes are the inputs', and read_ranges
    and decompress_batch take the result as it stands."""
    import torch

    lengths = [0, 1, N - 1, N, N + 1, 3 * N, 2 * N + 77, 5 * N - 1, 33, 7 * N + 1234]
    datas, at = [], 2000
    for n in lengths:
        datas.append(prose[at : at + n])
        at += n + 13
    res = ta.compress_batch(datas, dictionary_reset=True, reset_interval=N, reset_index=True, **conf)
    assert (res.status == 0).all()
    streams = res.streams()
    scan = ta.index_resets(streams)
    assert isinstance(scan, ta.ResetScan) and scan.status.tolist() == [OK] * len(datas)
    assert scan.index.first.tolist() == res.reset_index.first.tolist()
    assert scan.index.off.tolist() == res.reset_index.off[: int(res.reset_index.first[-1])].tolist()
    assert scan.index.interval == N
    assert [scan.size(i) for i in range(len(datas))] == lengths
    assert [truth(s)[1] for s in streams] == [scan.index.off[int(a) : int(b)].tolist() for a, b in zip(scan.index.first, scan.index.first[1:])]
    # ranges: inside a segment, across one and two segment edges, in the open segment, behind the end
    ranges = [(5, 100, 50), (5, N - 10, 20), (5, N - 1, N + 2), (9, 7 * N + 5, 1000), (6, 2 * N + 70, 50), (3, 0, N), (4, N, 1), (7, 3 * N - 3, 9)]
    r = ta.read_ranges(streams, reset_index=scan.index, stream_index=[q[0] for q in ranges], begin=[q[1] for q in ranges],
                       length=[q[2] for q in ranges])
    assert r.ranges() == [datas[s][b : b + n] for s, b, n in ranges]
    assert r.status.tolist() == [OK if len(datas[s][b : b + n]) == n else INPUT_EXHAUSTED for s, b, n in ranges]
    capfd.readouterr()
    back = ta.decompress_batch(streams, reset_index=scan.index)
    m = DECODE.search(capfd.readouterr().err)
    assert [back.stream(i) for i in range(len(datas))] == datas
    assert m and int(m[2]) == sum(1 for n in lengths if n > N) and int(m[3]) > int(m[2])
    # the other two input forms
    flat, in_off, in_len = ta.pack_streams(streams)
    scan2 = ta.index_resets(flat, in_off, in_len)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = [torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(in_off.view(np.int64)).to(dev), torch.from_numpy(in_len.view(np.int32)).to(dev)]
    st.synchronize()
    scan3 = ta.index_resets(t[0], t[1], t[2], stream=st.cuda_stream, timing=True)
    st.synchronize()
    scan4 = ta.index_resets(t[0], t[1], t[2])
    torch.cuda.synchronize()
    for other in (scan2, scan3, scan4):
        cpu = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else x  # noqa: E731
        assert cpu(other.index.first).tolist() == scan.index.first.tolist() and cpu(other.index.off).tolist() == scan.index.off.tolist()
        assert cpu(other.closed_size).tolist() == scan.closed_size.tolist() and cpu(other.open_size).tolist() == scan.open_size.tolist()
        assert other.index.interval == N and [other.size(i) for i in range(len(datas))] == lengths
    assert scan3.index.first.is_cuda and scan3.kernel_ms > 0
    assert ta.read_ranges(t[0], t[1], t[2], reset_index=scan3.index, stream_index=[5], begin=[N - 10], length=[20]).ranges() == [datas[5][N - 10 : N + 10]]
    import tamp

    assert tamp.index_resets(streams).index.off.tolist() == scan.index.off.tolist()
    # no closed segment: no interval
    short = ta.index_resets([streams[2]])
    assert short.index.interval is None and short.index.first.tolist() == [0, 0] and short.size(0) == N - 1


def test_streams_this_library_did_not_write(ta, checker, prose):
    """A reference compressor object with reset_dictionary() calls at places of its own; one stream continued in append mode."""
    pieces = [prose[9000 : 9000 + n] for n in (1, 17, 300, 5000)]
    scripts = {
        "between writes": [("write", pieces[0]), ("reset",), ("write", pieces[1]), ("reset",), ("write", pieces[2]), ("reset",),
                           ("write", pieces[3]), ("close",)],
        "two in a row": [("write", pieces[2]), ("reset",), ("reset",), ("write", pieces[1]), ("close",)],
        "first": [("reset",), ("write", pieces[3]), ("reset",), ("write", pieces[0]), ("close",)],
        "a flush that is none": [("write", pieces[1]), ("flush", True), ("write", pieces[2]), ("reset",), ("write", pieces[3]), ("flush", False)],
    }
    blobs, datas, segments = [], [], []
    for ops in scripts.values():
        res, blob = checker.stream_script(ops, window=10, literal=7, dictionary_reset=True)
        assert res == 0
        blobs.append(blob)
        datas.append(b"".join(op[1] for op in ops if op[0] == "write"))
        seg, cur = [], 0
        for op in ops:
            if op[0] == "write":
                cur += len(op[1])
            elif op[0] == "reset":
                seg.append(cur)
                cur = 0
        segments.append(seg)
    # a base stream and a session appended to it: the session opens with a reset
    res, more = checker.stream_script([("write", pieces[2]), ("close",)], window=10, literal=7, dictionary_reset=True, append=True)
    assert res == 0
    blobs.append(blobs[0] + more)
    datas.append(datas[0] + pieces[2])
    want = run_modes(blobs)
    # closed sizes are the bytes written between resets (a reset right behind a reset closes an empty segment)
    for i, seg in enumerate(segments + [segments[0] + [len(pieces[3])]]):
        assert want[i][0] == OK and [c for c in want[i][2] if c] == [c for c in seg if c], i
        assert len(want[i][1]) >= len(seg) and sum(want[i][2]) + want[i][3] == len(datas[i])
    assert want[1][2].count(0) >= 1 and want[4][3] == len(pieces[2])
    scan = ta.index_resets(blobs)
    assert scan.index.interval is None
    assert [scan.size(i) for i in range(len(blobs))] == [len(d) for d in datas]
    for i, w in enumerate(want):
        assert scan.index.off[int(scan.index.first[i]) : int(scan.index.first[i + 1])].tolist() == w[1]
    back = ta.decompress_batch(blobs, reset_index=scan.index)
    assert [back.stream(i) for i in range(len(blobs))] == datas
