"""GPU tier: one long buffer as dictionary-reset segments (tamp_amd_compress_resets, tamp_reset_segments_kernel.hpp).

The expected bytes are what ONE compressor object of the checker (the reference C where it is built, else the oracle) writes for
``write(seg_0) reset write(seg_1) reset ... write(seg_last) flush(False)`` with ``dictionary_reset=True``.  The calls are small:
a few hundred to a few thousand input bytes, up to 1,025 segments."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, OUTPUT_FULL, EXCESS_BITS, BAD_ARGUMENT = 0, 1, -2, -21
GUARD = 64


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


def script(data, interval):
    ops = []
    for at in range(0, max(len(data), 1), interval):
        if at:
            ops.append(("reset",))
        ops.append(("write", data[at : at + interval]))
    return ops + [("flush", False)]


def expected(checker, data, interval, window, literal, extended, lazy):
    res, blob = checker.stream_script(script(data, interval), window=window, literal=literal, extended=extended,
                                      dictionary_reset=True, lazy_matching=lazy)
    assert res == 0
    return blob


def segments(n, interval):
    return max(1, -(-n // interval))


def call(ta, data, interval, *, window=10, literal=8, extended=True, lazy=False, cap=None, mem="host", stream=None,
         dictionary_reset=1, custom=0):
    """One tamp_amd_compress_resets call with GUARD bytes of 0xA5 behind out_cap.
    -> (rc, status, out_len, the out_cap bytes, the guard bytes, reset_off)"""
    from tamp_amd import _lib

    lib = _lib.load()
    conf = _lib.TampAmdConf(window, literal, custom, int(extended), dictionary_reset, int(lazy))
    n, K = len(data), segments(len(data), interval)
    if cap is None:
        cap = lib.tamp_amd_compress_resets_bound(n, interval, literal)
    src = np.frombuffer(bytes(data), dtype=np.uint8) if n else np.zeros(1, np.uint8)
    out = np.full(cap + GUARD, 0xA5, dtype=np.uint8)
    out_len, status = np.full(1, 0xDEAD, dtype=np.uint64), np.full(1, 99, dtype=np.int8)
    reset_off = np.zeros(max(K - 1, 1), dtype=np.uint64)
    if mem == "host":
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = lib.tamp_amd_compress_resets(C.byref(conf), p(src), n, interval, p(out), cap, p(out_len), p(status), p(reset_off),
                                          _lib.MEM_HOST, 0, None)
        return rc, int(status[0]), int(out_len[0]), out[:cap].tobytes(), out[cap:].tobytes(), reset_off[: K - 1]
    import torch

    dev = torch.device("cuda:0")
    t_src, t_out = torch.from_numpy(src.copy()).to(dev), torch.from_numpy(out).to(dev)
    t_len, t_status = torch.from_numpy(out_len.view(np.int64)).to(dev), torch.from_numpy(status).to(dev)
    t_reset = torch.from_numpy(reset_off.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    rc = lib.tamp_amd_compress_resets(C.byref(conf), t_src.data_ptr(), n, interval, t_out.data_ptr(), cap, t_len.data_ptr(),
                                      t_status.data_ptr(), t_reset.data_ptr(), _lib.MEM_DEVICE, 0,
                                      C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    got = t_out.cpu().numpy()
    return (rc, int(t_status.cpu()[0]), int(t_len.cpu().numpy().view(np.uint64)[0]), got[:cap].tobytes(), got[cap:].tobytes(),
            t_reset.cpu().numpy().view(np.uint64)[: K - 1])


def check_offsets(blob, reset_off):
    """Every offset is the byte behind a reset: FLUSH + padding to 16 bits (0x55 0x80) lies in front of it."""
    for off in reset_off:
        assert blob[int(off) - 2 : int(off)] == b"\x55\x80", int(off)
    assert list(reset_off) == sorted(set(int(x) for x in reset_off))


#: (interval, input length): K = 1, 2, 3 and 40, the scan tile - 1 / tile / tile + 1, multiples of the interval and not, empty
def cases():
    from tamp_amd import _lib

    tile = _lib.RESETS_SCAN_TILE
    out = [(1, 0), (1, 1), (1, 2), (1, 3), (1, 40), (1, tile - 1), (1, tile), (1, tile + 1)]
    for iv in (15, 16, 17):
        out += [(iv, 40 * iv), (iv, 40 * iv - 7), (iv, 2 * iv + 1), (iv, iv)]
    out += [(1000, 999), (1000, 2000), (1000, 2500), (1000, 40_000 - 3), (4096, 100), (4096, 3 * 4096), (4096, 2 * 4096 + 100)]
    return out


CONFIGS = [(w, lit, ext, lazy) for w in (8, 10, 15) for lit in (8, 7) for ext in (True, False) for lazy in (False, True)]


@pytest.mark.parametrize("window,literal,extended,lazy", CONFIGS)
def test_bytes_are_the_reference_script(ta, checker, prose, window, literal, extended, lazy):
    ks = set()
    for j, (interval, n) in enumerate(cases()):
        data = prose[1000 * j + 17 : 1000 * j + 17 + n]
        want = expected(checker, data, interval, window, literal, extended, lazy)
        rc, status, out_len, out, guard, reset_off = call(ta, data, interval, window=window, literal=literal, extended=extended, lazy=lazy)
        assert (rc, status, out_len) == (0, OK, len(want)), (interval, n)
        assert out[:out_len] == want, (interval, n)
        assert guard == b"\xA5" * GUARD
        assert len(reset_off) == segments(n, interval) - 1
        check_offsets(want, reset_off)
        ks.add(segments(n, interval))
    from tamp_amd import _lib

    tile = _lib.RESETS_SCAN_TILE
    assert {1, 2, 3, 40, tile - 1, tile, tile + 1} <= ks


@pytest.mark.parametrize("extended", [True, False])
def test_device_memory_and_a_stream_of_the_callers(ta, checker, prose, extended):
    import torch

    side = torch.cuda.Stream()
    for interval, n in ((1, 0), (17, 40 * 17 - 7), (1, 1025), (1000, 2500), (4096, 3 * 4096)):
        data = prose[5000 : 5000 + n]
        want = expected(checker, data, interval, 10, 8, extended, False)
        for stream in (None, side):
            rc, status, out_len, out, guard, reset_off = call(ta, data, interval, extended=extended, mem="device", stream=stream)
            assert (rc, status, out_len) == (0, OK, len(want)), (interval, n)
            assert out[:out_len] == want and guard == b"\xA5" * GUARD
            check_offsets(want, reset_off)


def test_slices_carry_the_output_base(ta, checker, prose, monkeypatch, capfd):
    """TAMP_AMD_RESETS_SLICE: 40 segments in slices of 7 and 1,025 in slices of 100 -- the same bytes and offsets."""
    monkeypatch.setenv("TAMP_AMD_RESETS_DEBUG", "1")
    for slice_, interval, n in ((7, 17, 40 * 17 - 7), (100, 1, 1025), (1, 1000, 2500), (39, 16, 640)):
        monkeypatch.setenv("TAMP_AMD_RESETS_SLICE", str(slice_))
        data = prose[9000 : 9000 + n]
        want = expected(checker, data, interval, 10, 8, True, False)
        for mem in ("host", "device"):
            capfd.readouterr()
            rc, status, out_len, out, guard, reset_off = call(ta, data, interval, mem=mem)
            assert f"{slice_} per slice" in capfd.readouterr().err
            assert (rc, status, out_len) == (0, OK, len(want))
            assert out[:out_len] == want and guard == b"\xA5" * GUARD
            check_offsets(want, reset_off)


def test_gather_meets_every_alignment(ta, checker, prose):
    """The gather reads slab k at k * slab of a 256-byte aligned buffer and writes it where the scan says, in a 256-byte aligned
    buffer (device memory: torch's allocation): all four residues mod 4 must have occurred on both sides."""
    from tamp_amd import _lib

    lib = _lib.load()
    src_res, dst_res = set(), set()
    for interval, n in ((17, 40 * 17), (1, 40), (15, 600)):
        data = prose[20_000 : 20_000 + n]
        want = expected(checker, data, interval, 10, 8, True, False)
        rc, status, out_len, out, guard, reset_off = call(ta, data, interval, mem="device")
        assert (rc, status, out[:out_len]) == (0, OK, want)
        slab = lib.tamp_amd_compress_resets_slab(n, interval, 8)
        starts = [0] + [int(x) - 2 for x in reset_off]  # (a segment starts with its 2-byte lead)
        src_res |= {(k * slab) % 4 for k in range(len(starts))}
        dst_res |= {s % 4 for s in starts}
    assert src_res == {0, 1, 2, 3} and dst_res == {0, 1, 2, 3}, (src_res, dst_res)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_output_room(ta, checker, prose, mem):
    """out_cap == out_len succeeds; one byte fewer is TAMP_OUTPUT_FULL with out_len = 0 and nothing behind out_cap written."""
    for interval, n in ((17, 40 * 17 - 7), (1000, 2500), (1, 3)):
        data = prose[30_000 : 30_000 + n]
        want = expected(checker, data, interval, 10, 8, True, False)
        rc, status, out_len, out, guard, _ = call(ta, data, interval, cap=len(want), mem=mem)
        assert (rc, status, out_len, out) == (0, OK, len(want), want) and guard == b"\xA5" * GUARD
        rc, status, out_len, out, guard, _ = call(ta, data, interval, cap=len(want) - 1, mem=mem)
        assert (rc, status, out_len) == (0, OUTPUT_FULL, 0) and guard == b"\xA5" * GUARD


@pytest.mark.parametrize("mem", ["host", "device"])
def test_excess_bits_in_a_middle_segment(ta, prose, mem):
    data = bytearray(prose[40_000 : 40_000 + 40 * 17])
    data[20 * 17 + 5] = 0x80
    rc, status, out_len, out, guard, _ = call(ta, bytes(data), 17, literal=7, mem=mem)
    assert (rc, status, out_len) == (0, EXCESS_BITS, 0) and guard == b"\xA5" * GUARD
    data[20 * 17 + 5] = 0x7F
    rc, status, out_len, out, guard, _ = call(ta, bytes(data), 17, literal=7, mem=mem)
    assert (rc, status) == (0, OK) and out_len > 0


def test_calls_outside_the_contract(ta, prose):
    data = prose[:100]
    assert call(ta, data, 17, dictionary_reset=0)[0] == BAD_ARGUMENT
    assert call(ta, data, 17, custom=1)[0] == BAD_ARGUMENT
    assert call(ta, data, 17, window=16)[0] == BAD_ARGUMENT
    from tamp_amd import _lib

    lib = _lib.load()
    conf = _lib.TampAmdConf(10, 8, 0, 1, 1, 0)
    n, st = C.c_uint64(7), C.c_int8(7)
    buf = (C.c_ubyte * 256)()
    assert lib.tamp_amd_compress_resets(C.byref(conf), buf, 100, 0, buf, 256, C.byref(n), C.byref(st), None, 0, 0, None) == BAD_ARGUMENT
    assert lib.tamp_amd_compress_resets(C.byref(conf), buf, 1 << 32, 4096, buf, 256, C.byref(n), C.byref(st), None, 0, 0, None) == BAD_ARGUMENT
    assert (n.value, st.value) == (7, 7)


def test_bound_holds_on_random_bytes(ta):
    from tamp_amd import _lib

    lib = _lib.load()
    rng = random.Random(5)
    for interval in range(1, 18):
        for literal in (8, 7):
            n = 40 * interval - (interval // 2)
            data = bytes(rng.randrange(1 << literal) for _ in range(n))
            bound = lib.tamp_amd_compress_resets_bound(n, interval, literal)
            rc, status, out_len, out, guard, _ = call(ta, data, interval, literal=literal, cap=bound)
            assert (rc, status) == (0, OK) and 0 < out_len <= bound, (interval, literal, out_len, bound)


def test_python_surface_round_trip(ta, checker, prose):
    """compress(..., reset_interval=N): the script's bytes; this package and the checker decode them to the input."""
    for interval, n, kw in ((4096, 50_000, {}), (1000, 2500, dict(window=12, extended=False)), (17, 673, dict(lazy_matching=True)),
                            (64 << 10, 300_000, {})):
        data = prose[100_000 : 100_000 + n]
        blob = ta.compress(data, dictionary_reset=True, reset_interval=interval, **kw)
        want = expected(checker, data, interval, kw.get("window", 10), 8, kw.get("extended", True), kw.get("lazy_matching", False))
        assert blob == want
        assert bytes(ta.decompress(blob)) == data
        res, back, consumed = checker.decompress(blob, cap=n + 64)
        assert (res, back, consumed) == (2, data, len(blob))
    # calls the batch does not take run the same script on the object: the same bytes
    data = prose[200_000:203_000]
    want = expected(checker, data, 1000, 10, 8, True, False)
    assert ta.compress(data.decode(), dictionary_reset=True, reset_interval=1000) == want


# ---- reading such a stream back: tamp_amd_decompress_resets ----

import re  # noqa: E402

import long_stream_writer as lsw  # noqa: E402

TAKEN = re.compile(r"\[tamp_amd resets\] (decoded|sized): (\d+) segments, (\d+) bytes out$", re.M)


@pytest.fixture
def resets_debug(monkeypatch):
    monkeypatch.setenv("TAMP_AMD_RESETS_MIN", "64")
    monkeypatch.setenv("TAMP_AMD_RESETS_DEBUG", "1")
    for k in ("TAMP_AMD_DECODER", "TAMP_AMD_LONGDEC", "TAMP_AMD_LONGDEC_MIN", "TAMP_AMD_LONGDEC_DEBUG"):
        monkeypatch.delenv(k, raising=False)


def decode_call(blob, cap, *, mem="host", max_window_bits=15, size_only=False):
    """-> (rc, (status, bytes or size, consumed))"""
    from tamp_amd import _lib

    lib = _lib.load()
    src = np.frombuffer(bytes(blob), dtype=np.uint8) if len(blob) else np.zeros(1, np.uint8)
    out = np.full(cap + GUARD, 0xA5, dtype=np.uint8)
    out_len, consumed, status = np.full(1, 77, np.uint32), np.full(1, 77, np.uint32), np.full(1, 77, np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    if mem == "host":
        rc = lib.tamp_amd_decompress_resets(max_window_bits, p(src), len(blob), None if size_only else p(out), cap, p(out_len),
                                            p(status), p(consumed), _lib.MEM_HOST, 0, None)
        got = out
    else:
        import torch

        dev = torch.device("cuda:0")
        t_src, t_out = torch.from_numpy(src.copy()).to(dev), torch.from_numpy(out).to(dev)
        torch.cuda.synchronize()
        rc = lib.tamp_amd_decompress_resets(max_window_bits, t_src.data_ptr(), len(blob), None if size_only else t_out.data_ptr(), cap,
                                            p(out_len), p(status), p(consumed), _lib.MEM_DEVICE, 0, None)
        torch.cuda.synchronize()
        got = t_out.cpu().numpy()
    assert got[cap:].tobytes() == b"\xA5" * GUARD
    n = int(out_len[0])
    return rc, (int(status[0]), n if size_only else got[:n].tobytes(), int(consumed[0]))


def check_decode(checker, capfd, blob, cap, *, must_take, segments=None, mem="host", max_window_bits=15, want=None):
    """The call's triple is the checker's, for the decode and for the size alone; the debug line says which path ran."""
    if want is None:
        want = checker.decompress(blob, cap=cap, max_window_bits=max_window_bits)
    for size_only in (False, True):
        capfd.readouterr()
        rc, got = decode_call(blob, cap, mem=mem, max_window_bits=max_window_bits, size_only=size_only)
        err = capfd.readouterr().err
        assert rc == 0, err
        assert got == ((want[0], len(want[1]), want[2]) if size_only else want), err
        m = TAKEN.search(err)
        if must_take:
            assert m and "declined" not in err, err
            assert m[1] == ("sized" if size_only else "decoded") and int(m[3]) == len(want[1])
            if segments is not None:
                assert int(m[2]) == segments
        else:
            assert m or "[tamp_amd resets" in err and "declined: " in err, err
    return err


@pytest.mark.parametrize("window,extended", [(8, True), (10, True), (15, True), (8, False), (10, False), (15, False)])
def test_decode_clean_streams_are_taken(ta, checker, prose, capfd, resets_debug, window, extended):
    """K = 1 and K = 40 (resets wherever the data puts them: in the middle of chunks), host and device memory."""
    for interval, n, K in ((4096, 3000, 1), (1000, 40_000 - 3, 40)):
        data = prose[50_000 : 50_000 + n]
        blob = expected(checker, data, interval, window, 8, extended, False)
        want = checker.decompress(blob, cap=n + 64)
        assert want == (2, data, len(blob))
        for mem in ("host", "device"):
            check_decode(checker, capfd, blob, n + 64, must_take=True, segments=K, mem=mem, want=want)


def flush_pair_across_a_chunk_boundary(extended, window=10):
    """Chunk 2's last token is a FLUSH that ends exactly on the chunk boundary; chunk 3's first token is the FLUSH that resets."""
    rng = random.Random(3)
    w = lsw.TokenWriter(window, 8, extended, more=0)
    cb = w.chunk_bits
    w.fill_to(3 * cb - 9, rng)
    w.flush()
    assert w.bit == 3 * cb
    w.flush()
    w.plain_until(5 * cb + 100, rng)
    w.flush(), w.flush()  # ... and a pair in the middle of chunk 5
    w.plain_until(7 * cb, rng)
    assert [t.bit // cb for t in w.tokens if t.kind == "F"][:2] == [2, 3]
    return w


@pytest.mark.parametrize("extended", [True, False])
def test_decode_flush_pair_split_across_chunks(ta, checker, capfd, resets_debug, extended):
    w = flush_pair_across_a_chunk_boundary(extended)
    check_decode(checker, capfd, w.blob(), w.out + 64, must_take=True, segments=3)


@pytest.mark.parametrize("extended", [True, False])
def test_decode_empty_segments(ta, checker, prose, capfd, resets_debug, extended):
    """Two reset ops in a row on the checker's object, and four FLUSH tokens in a row from the token writer (three resets)."""
    a, b = prose[60_000:61_000], prose[61_000:61_700]
    res, blob = checker.stream_script([("write", a), ("reset",), ("reset",), ("write", b), ("flush", False)], extended=extended,
                                      dictionary_reset=True)
    assert res == 0
    check_decode(checker, capfd, blob, len(a) + len(b) + 64, must_take=True)
    rng = random.Random(4)
    w = lsw.TokenWriter(10, 8, extended, more=0)
    w.plain_until(700, rng)
    for _ in range(4):
        w.flush()
    w.plain_until(3 * w.chunk_bits, rng)
    check_decode(checker, capfd, w.blob(), w.out + 64, must_take=True, segments=4)


def test_decode_either_way_cases(ta, checker, prose, capfd, resets_debug):
    rng = random.Random(6)
    # more than four resets inside one chunk
    w = lsw.TokenWriter(10, 8, False, more=0)
    w.plain_until(300, rng)
    for _ in range(7):
        w.flush()
    w.plain_until(2 * w.chunk_bits, rng)
    err = check_decode(checker, capfd, w.blob(), w.out + 64, must_take=False)
    assert "declined: resets per chunk" in err
    # an offset out of the window in segment 2
    w = lsw.TokenWriter(10, 8, False, more=0)
    w.plain_until(1000, rng)
    w.flush(), w.flush()
    w.plain_until(3000, rng)
    w.match(w.W - 2, 5, check=False)
    w.plain_until(2 * w.chunk_bits, rng)
    assert checker.decompress(w.blob(), cap=w.out + 64)[0] == -4
    check_decode(checker, capfd, w.blob(), w.out + 64, must_take=False)
    # the custom bit (no dictionary can be passed), and a window above max_window_bits
    from oracle.checker import Oracle

    w = lsw.TokenWriter(10, 8, True, custom=True, more=0)
    w.plain_until(2 * w.chunk_bits, rng)
    want = Oracle().decompress(w.blob(), cap=w.out + 64)  # (the library's rule; the reference's C leaves the window to its caller)
    assert want[0] == -3
    check_decode(checker, capfd, w.blob(), w.out + 64, must_take=False, want=want)
    w = lsw.TokenWriter(12, 8, True, more=0)
    w.plain_until(2 * w.chunk_bits, rng)
    check_decode(checker, capfd, w.blob(), w.out + 64, must_take=False, max_window_bits=10)
    # room equal to the size, and one byte fewer
    data = prose[70_000:72_500]
    blob = expected(checker, data, 1000, 10, 8, True, False)
    for cap in (len(data), len(data) - 1):
        check_decode(checker, capfd, blob, cap, must_take=False)
    # without the reset bit, and below the threshold
    res, plain = checker.compress(data)
    check_decode(checker, capfd, plain, len(data) + 64, must_take=False)


def test_decode_cut_at_every_byte(ta, checker, prose, capfd, resets_debug):
    """A three-segment stream of ~300 bytes cut behind every byte: the checker's triple every time."""
    data = prose[80_000:80_450]
    blob = expected(checker, data, 150, 10, 8, True, False)
    assert 200 <= len(blob) <= 400
    for n in range(len(blob) + 1):
        want = checker.decompress(blob[:n], cap=len(data) + 64)
        rc, got = decode_call(blob[:n], len(data) + 64)
        assert rc == 0 and got == want, n
    capfd.readouterr()


def test_python_decompress_takes_the_reset_path(ta, checker, prose, capfd, resets_debug):
    data = prose[100_000:160_000]
    blob = ta.compress(data, dictionary_reset=True, reset_interval=4096)
    capfd.readouterr()
    assert bytes(ta.decompress(blob)) == data
    err = capfd.readouterr().err
    assert [m[1] for m in TAKEN.finditer(err)] == ["sized", "decoded"] and "declined" not in err, err
    assert checker.decompress(blob, cap=len(data) + 64) == (2, data, len(blob))
