"""GPU tier (-m gpu): every codec path at all 64 header settings (window 2^8..2^15 x literal 5..8 x both formats).

Three things follow from the header in every path -- the minimum match length (3 for nine (window, literal) pairs), the
seeded dictionary (one per literal width in the extended format, the literal-8 one in v1) and the literal width of the
bit readers and writers.  Every result here is compared with the oracle (oracle/libtamp_oracle.so, pinned against the
reference on the CPU tier) or with tests/golden/config_matrix.json (recorded from the reference): status, bytes, and
the consumed count where the call reports one.  Each expectation is computed once and shared by every path that must
produce it.
"""
import ctypes as C
import hashlib
import io
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
from conftest import load_golden, unb64, workload_rows

pytestmark = pytest.mark.gpu

WINDOWS, LITERALS = range(8, 16), range(5, 9)
SETTINGS = [(w, lit, ext) for w in WINDOWS for lit in LITERALS for ext in (True, False)]
MINP3 = [(w, lit) for w in WINDOWS for lit in LITERALS if 2 + (w > 10 + 2 * (lit - 5)) == 3]
DECODERS = (None, "wave", "lane", "global", "split")


@pytest.fixture(scope="module")
def ta():
    import tamp_amd
    from tamp_amd import _lib

    lib = _lib.load()  # raises if the native library is missing: no silent fallback
    assert lib.tamp_amd_device_count() >= 1, "no HIP device visible"
    return tamp_amd


def _pmap(fn, jobs):
    """The oracle's C calls release the GIL: expectations are computed on 16 threads."""
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda j: fn(*j), jobs))


def _rows(kind, literal, n, row):
    mask = f"&{(1 << literal) - 1}" if literal < 8 else ""
    return workload_rows(f"{kind}{mask}:{n}")(row + 1)[row].tobytes()


def _matrix_bytes(spec):
    """A source / dictionary record of tests/golden/config_matrix.json -> its bytes (see tests/test_oracle_golden.py)."""
    if spec is None:
        return None
    data = bytearray(b"".join(workload_rows(name)(row + 1)[row].tobytes() for name, row in spec["pieces"]))
    if spec.get("patch"):
        data[spec["patch"][0]] = spec["patch"][1]
    assert hashlib.sha256(data).hexdigest() == spec["sha256"], ("generator drifted", spec["pieces"])
    return bytes(data)


def _excess(data, literal, pos):
    """`data` with a byte of 2^literal (one bit above the literal width) at `pos`: EXCESS_BITS there."""
    b = bytearray(data)
    b[pos] = 1 << literal if literal < 8 else b[pos]
    return bytes(b)


def _short_inputs(w, lit):
    """< 1 KiB each: text, short and long runs, long repeats, random bytes, tiny streams, an offending byte at 123."""
    k = w * 4 + lit
    runs = b"".join(bytes([(i * 7) & ((1 << lit) - 1)]) * n for i, n in enumerate((1, 2, 3, 4, 5, 9, 17, 40, 250, 400)))
    rep = _rows("synth_text", lit, 180, k % 7)
    out = [_rows("synth_text", lit, 900, k % 5), _rows("stress", lit, 600, 1), _rows("stress", lit, 950, 2),
           _rows("stress", lit, 500, 0), _rows("lcg_runs", lit, 700, k % 3), runs[:960], (rep * 6)[:960],
           b"", _rows("synth_text", lit, 1, 0), _rows("synth_text", lit, 3, 1), _rows("synth_text", lit, 17, 2)]
    if lit < 8:
        out.append(_excess(_rows("synth_text", lit, 400, 3), lit, 123))
    return out


def _long_inputs(w, lit):
    """>= 1 KiB: text, runs, long repeats (extended matches at their cap), random bytes, a repeat from the window's far
    end, an offending byte at 1500."""
    k = w * 4 + lit
    b = min(400, 1 << (w - 2))
    blk = _rows("synth_text", lit, b, 9)
    edge = blk + _rows("stress", lit, (1 << w) - b - 2, 3) + blk + blk[:150] * 3  # (random filler: nothing matches)
    out = [_rows("synth_text", lit, 4000, k % 5), _rows("stress", lit, 3000, 4), _rows("stress", lit, 5000, 5),
           _rows("stress", lit, 1500, 0), edge * (1 + 2048 // len(edge)), _rows("synth_text", lit, 200, 9) * 40]
    if lit < 8:
        out.append(_excess(_rows("synth_text", lit, 2000, 4), lit, 1500))
    return out


def _custom_dictionary(w, lit):
    return _rows("synth_text", lit, 1 << w, 11)


def _check_batch(res, want, inputs, tag):
    for j, (st, comp) in enumerate(want):
        assert int(res.status[j]) == st, (tag, j, len(inputs[j]))
        assert res.stream(j) == comp, (tag, j, len(inputs[j]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. batch compress: every build x every (window, literal, format), seeded and custom dictionary
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_compress_every_build_at_every_setting(ta, oracle):
    """Short messages: lean one-wavefront build (default hint) and the run-aware build; streams of 1 KiB and more: the
    run-aware generic build, the 2^10 build, the lean u16 build at 2^15; lazy matching: the lazy u32 and u16 builds.  One
    call per (build, setting, dictionary); inputs with runs, capped extended matches, repeats from the far end of the
    window, random bytes and one byte above the literal width."""
    jobs = []
    for w, lit, ext in SETTINGS:
        short, long_ = _short_inputs(w, lit), _long_inputs(w, lit)
        for d in (None, _custom_dictionary(w, lit)):
            jobs.append((w, lit, ext, d, short, long_))
    want = {}

    def expect(i, w, lit, ext, d, short, long_):
        kw = dict(window=w, literal=lit, extended=ext, dictionary=d)
        return i, ([oracle.compress(x, **kw) for x in short], [oracle.compress(x, **kw) for x in long_],
                   [oracle.compress(x, lazy_matching=True, **kw) for x in short + long_])

    for i, exp in _pmap(expect, [(i,) + j for i, j in enumerate(jobs)]):
        want[i] = exp
    statuses = set()
    for i, (w, lit, ext, d, short, long_) in enumerate(jobs):
        w_short, w_long, w_lazy = want[i]
        kw = dict(window=w, literal=lit, extended=ext, dictionary=d)
        tag = (w, lit, ext, d is not None)
        max_short = max(len(x) for x in short)
        assert max_short < 1024 and min(len(x) for x in long_) >= 1024
        _check_batch(ta.compress_batch(short, max_in_len=max_short, **kw), w_short, short, tag + ("lean",))
        _check_batch(ta.compress_batch(short, max_in_len=max_short, run_aware=True, **kw), w_short, short, tag + ("runs",))
        _check_batch(ta.compress_batch(long_, **kw), w_long, long_, tag + ("long",))
        _check_batch(ta.compress_batch(short + long_, lazy_matching=True, **kw), w_lazy, short + long_, tag + ("lazy",))
        statuses |= {st for st, _ in w_short + w_long}
    assert statuses == {0, -2}


# ---------------------------------------------------------------------------------------------------------------------
# 2. every batch decoder on mixed batches (each stream carries its own header)
# ---------------------------------------------------------------------------------------------------------------------
def _decode_cases(oracle):
    """-> (small, large): lists of (compressed, plain, window).  `small` has plain streams below 2 KiB - 64 (every cap of
    it fits the one-wavefront RESOLVE), `large` adds streams of 2..16 KiB.  Every header setting, seeded dictionaries,
    compressed streams of 512 bytes and more, truncated copies and copies with one bit flipped."""
    rng = random.Random(20261016)
    jobs = []
    for w, lit, ext in SETTINGS:
        k = w * 8 + lit * 2 + ext
        small = [_rows("synth_text", lit, 1900, k % 6), _rows("stress", lit, 800, 0), _rows("stress", lit, 1500, 1),
                 _rows("stress", lit, 1200, 2)]
        large = [_rows("synth_text", lit, 9000, k % 4), _rows("stress", lit, 5000, 5)]
        for x in small:
            jobs.append((x, w, lit, ext, "small"))
        for x in large:
            jobs.append((x, w, lit, ext, "large"))
    comps = _pmap(lambda x, w, lit, ext, _: oracle.compress(x, window=w, literal=lit, extended=ext), jobs)
    small, large = [], []
    for (x, w, lit, ext, kind), (st, comp) in zip(jobs, comps):
        assert st == 0
        (small if kind == "small" else large).append((comp, x, w))
    assert sum(len(c) >= 512 for c, _, _ in small) >= 100
    for group in (small, large):
        extra = []
        for comp, x, w in group[::2]:
            extra.append((comp[: rng.randrange(1, len(comp))], x, w))
            bad = bytearray(comp)
            bad[rng.randrange(1, len(bad))] ^= 1 << rng.randrange(8)
            extra.append((bytes(bad), x, w))
        group.extend(extra)
    return small, small + large


def _with_caps(cases):
    """Each stream at caps ample, exact, exact - 1, 0 and 1 -> (streams, caps, windows)."""
    streams, caps, wins = [], [], []
    for comp, x, w in cases:
        for cap in (len(x) + 64, len(x), max(len(x) - 1, 0), 0, 1):
            streams.append(comp), caps.append(cap), wins.append(w)
    return streams, caps, wins


def _decode_expect(oracle, streams, caps, max_window_bits=15, dictionary=None):
    return _pmap(lambda s, cap: oracle.decompress(s, cap=cap, max_window_bits=max_window_bits, dictionary=dictionary),
                 list(zip(streams, caps)))


def _check_decode(res, want, tag):
    for j, (st, out, consumed) in enumerate(want):
        got = (int(res.status[j]), res.stream(j), int(res.in_consumed[j]))
        assert got == (st, out, consumed), (tag, j, got[0], st, len(got[1]), len(out), got[2], consumed)


def test_every_batch_decoder_on_mixed_header_batches(ta, oracle, monkeypatch):
    """Batch A: every header setting in one call (>= 256 streams: header pre-pass; the unforced choice takes the split
    decoder), caps ample / exact / exact - 1 / 0 / 1, once all <= 2 KiB (one-wavefront RESOLVE) and once with caps up to
    16 KiB (workgroup RESOLVE).  Batch B: its streams at windows <= 2^10 with max_window_bits = 10 (the LDS lane decoders).
    Each batch unforced and under TAMP_AMD_DECODER = wave / lane / global / split."""
    small, large = _decode_cases(oracle)
    for cases in (small, large):
        streams, caps, wins = _with_caps(cases)
        want = _decode_expect(oracle, streams, caps)
        assert len(streams) >= 5 * 256 and len({s[0] for s in streams}) >= 64
        sub = [j for j, w in enumerate(wins) if w <= 10]
        b_streams, b_caps, b_want = [streams[j] for j in sub], [caps[j] for j in sub], [want[j] for j in sub]
        assert len(b_streams) >= 256
        for mode in DECODERS:
            if mode is None:
                monkeypatch.delenv("TAMP_AMD_DECODER", raising=False)
            else:
                monkeypatch.setenv("TAMP_AMD_DECODER", mode)
            res = ta.decompress_batch(streams, out_cap=np.array(caps, np.uint32))
            _check_decode(res, want, ("A", mode, max(caps)))
            res = ta.decompress_batch(b_streams, out_cap=np.array(b_caps, np.uint32), max_window_bits=10)
            _check_decode(res, b_want, ("B", mode, max(caps)))
    monkeypatch.delenv("TAMP_AMD_DECODER", raising=False)
    # window limits below the batch's largest header, and no header pre-pass
    streams, caps, _ = _with_caps(large)
    for limit in (12, 9):
        want = _decode_expect(oracle, streams, caps, max_window_bits=limit)
        assert sum(st == -3 for st, _, _ in want) >= 256
        _check_decode(ta.decompress_batch(streams, out_cap=np.array(caps, np.uint32), max_window_bits=limit), want,
                      ("limit", limit))
    want = _decode_expect(oracle, streams, caps)
    _check_decode(ta.decompress_batch(streams, out_cap=np.array(caps, np.uint32), scan_headers=False), want, "no scan")


def test_every_batch_decoder_with_custom_dictionaries(ta, oracle, monkeypatch):
    """Custom-dictionary streams of every literal width and both formats, one call per window (the dictionary is the
    batch's), under every decoder."""
    rng = random.Random(5)
    for w in WINDOWS:
        cases = []
        d = _custom_dictionary(w, 8)  # one dictionary per call (bytes above 5..7 bits in it are fine: it is the window)
        for lit in LITERALS:
            dm = bytes(b & ((1 << lit) - 1) for b in d)
            for ext in (True, False):
                for x in (_rows("synth_text", lit, 1500, lit) + dm[100:600], _rows("stress", lit, 1200, 2)):
                    st, comp = oracle.compress(x, window=w, literal=lit, extended=ext, dictionary=d)
                    assert st == 0
                    cases.append((comp, x, w))
                    cases.append((comp[: rng.randrange(1, len(comp))], x, w))
        streams, caps, _ = _with_caps(cases)
        limit = max(w, 10)
        want = _decode_expect(oracle, streams, caps, max_window_bits=limit, dictionary=d)
        for mode in DECODERS:
            if mode is None:
                monkeypatch.delenv("TAMP_AMD_DECODER", raising=False)
            else:
                monkeypatch.setenv("TAMP_AMD_DECODER", mode)
            res = ta.decompress_batch(streams, out_cap=np.array(caps, np.uint32), dictionary=d, max_window_bits=limit)
            _check_decode(res, want, ("custom", w, mode))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the long-stream decoder at every (window, literal) pair with a 3-byte minimum match
# ---------------------------------------------------------------------------------------------------------------------
def test_long_stream_decoder_at_every_three_byte_minimum_match(ta, oracle, monkeypatch):
    """Streams of 100-400 KB compressed, both formats, one with a custom dictionary: whole, cut short by 1, 2, 3 and 7
    bytes, and with one of three bits flipped -- through the long-stream decoder (TAMP_AMD_LONGDEC_MIN = 65536) and again
    through the exact decoders (TAMP_AMD_LONGDEC = 0)."""
    rng = random.Random(99)
    jobs = []
    for i, (w, lit) in enumerate(MINP3):
        for ext in (True, False):
            x = _rows("synth_text", lit, 250_000, i % 4) + _rows("stress", lit, 40_000, 3 * (i % 3)) + \
                _rows("stress", lit, 20_000, 1) + _rows("stress", lit, 30_000, 2)
            d = _custom_dictionary(w, lit) if (w, lit, ext) == (13, 5, False) else None
            jobs.append((x, w, lit, ext, d))
    comps = _pmap(lambda x, w, lit, ext, d: oracle.compress(x, window=w, literal=lit, extended=ext, dictionary=d), jobs)
    cases = []
    for (x, w, lit, ext, d), (st, comp) in zip(jobs, comps):
        assert st == 0 and 100_000 <= len(comp) <= 400_000, (w, lit, ext, len(comp))
        variants = [comp] + [comp[:-k] for k in (1, 2, 3, 7)]
        for _ in range(3):
            bad = bytearray(comp)
            bad[rng.randrange(2, len(bad))] ^= 1 << rng.randrange(8)
            variants.append(bytes(bad))
        cap = len(x) + 64
        want = _pmap(lambda s: oracle.decompress(s, cap=cap, dictionary=d), [(s,) for s in variants])
        cases.append(((w, lit, ext), variants, cap, d, want))
    monkeypatch.delenv("TAMP_AMD_DECODER", raising=False)
    monkeypatch.setenv("TAMP_AMD_LONGDEC_MIN", "65536")
    for longdec in ("1", "0"):
        monkeypatch.setenv("TAMP_AMD_LONGDEC", longdec)
        for tag, variants, cap, d, want in cases:
            res = ta.decompress_batch(variants, out_cap=cap, dictionary=d)
            _check_decode(res, want, ("long", longdec) + tag)


# ---------------------------------------------------------------------------------------------------------------------
# 4. Compressor streams: segments and pieces
# ---------------------------------------------------------------------------------------------------------------------
def _replay_compressor(ta, conf, dictionary, ops):
    f = io.BytesIO()
    c = ta.Compressor(f, dictionary=dictionary, **conf)
    for op in ops:
        if op[0] == "write":
            c.write(op[1])
        elif op[0] == "flush":
            c.flush(op[1])
        elif op[0] == "reset":
            c.reset_dictionary()
        else:
            c.close()
    return f.getvalue()


def test_compressor_replays_the_matrix_scripts_as_segments_and_pieces(ta, oracle):
    """tests/golden/config_matrix.json's scripts on tamp_amd.Compressor, with the default PIECE_MIN (a segment per flush
    point) and with PIECE_MIN = 1 (a piece per write, run / match / bit state carried between them), then seeded scripts
    of the same settings against Oracle.stream_script."""
    recs = load_golden("config_matrix.json")["streams"]
    scripts = []
    for rec in recs:
        src, d = _matrix_bytes(rec["source"]), _matrix_bytes(rec["dictionary"])
        ops = [("write", src[op[1] : op[2]]) if op[0] == "write" else tuple(op) for op in rec["ops"]]
        st, want = oracle.stream_script(ops, dictionary=d, **rec["conf"])
        assert (st, len(want), hashlib.sha256(want).hexdigest()) == (
            rec["status"], rec["expected_len"], rec["expected_sha256"]), rec["name"]
        scripts.append((rec["name"], rec["conf"], d, ops, want))
    rng = random.Random(31)
    for w, lit in MINP3 + [(8, 5), (8, 6), (10, 6), (14, 7)]:
        for ext in (True, False):
            src = _rows("synth_text", lit, 6000, w) + _rows("stress", lit, 2000, 1) + _rows("stress", lit, 3000, 2)
            conf = dict(window=w, literal=lit, extended=ext, dictionary_reset=rng.random() < 0.3)
            ops, pos = [], 0
            while pos < len(src):
                m = rng.choice([1, 2, 15, 16, 17, 33, 400, 2000])
                ops.append(("write", src[pos : pos + m]))
                pos += m
                if rng.random() < 0.1:
                    ops.append(("flush", rng.random() < 0.8))
                elif conf["dictionary_reset"] and rng.random() < 0.05:
                    ops.append(("reset",))
            ops.append(("close",))
            st, want = oracle.stream_script(ops, **conf)
            assert st == 0
            scripts.append((f"seeded_{w}_{lit}_{ext}", conf, None, ops, want))
    old_min = ta.Compressor.PIECE_MIN
    try:
        for piece_min in (old_min, 1):
            ta.Compressor.PIECE_MIN = piece_min
            for name, conf, d, ops, want in scripts:
                assert _replay_compressor(ta, conf, d, ops) == want, (name, piece_min)
    finally:
        ta.Compressor.PIECE_MIN = old_min


def test_pieces_raise_excess_bits_at_five_and_six_bit_literals(ta, oracle):
    """An offending byte in the middle of a later piece: ExcessBitsError from the write that hands it over (pieces) or
    from the flush (segments), as in the reference's write; what reached the file before it (nothing from the failed
    piece) is the start of the stream without the offending byte."""
    old_min = ta.Compressor.PIECE_MIN
    try:
        for piece_min in (1, old_min):
            ta.Compressor.PIECE_MIN = piece_min
            for w, lit in ((11, 5), (8, 5), (13, 6), (10, 6), (15, 6)):
                good = _rows("synth_text", lit, 6000, w)
                bad = _excess(good, lit, 4000)
                f = io.BytesIO()
                c = ta.Compressor(f, window=w, literal=lit)
                c.write(bad[:1500])
                c.write(bad[1500:3000])
                with pytest.raises(ta.ExcessBitsError):
                    c.write(bad[3000:])
                    c.flush()
                # what left before the offending piece is the start of the stream without it
                st, want = oracle.compress(good, window=w, literal=lit)
                assert st == 0 and want.startswith(f.getvalue()), (w, lit, piece_min)
    finally:
        ta.Compressor.PIECE_MIN = old_min


# ---------------------------------------------------------------------------------------------------------------------
# 5. reference-named objects: the segment and piece shortcuts of TampCompressor, TampDecompressor with a conf
# ---------------------------------------------------------------------------------------------------------------------
class _TampConf(C.Structure):
    _fields_ = [("window", C.c_uint16, 4), ("literal", C.c_uint16, 4), ("use_custom_dictionary", C.c_uint16, 1),
                ("extended", C.c_uint16, 1), ("dictionary_reset", C.c_uint16, 1), ("append", C.c_uint16, 1),
                ("lazy_matching", C.c_uint16, 1)]


def test_reference_named_objects_at_five_and_six_bit_literals(ta, oracle):
    """One TampCompressor per setting driven through token-level calls, compat_segment (compress_and_flush of >= 2 KiB on
    an object between segments) and compat_piece (compress of >= 64 KiB): the bytes are the oracle's stream; then a
    TampDecompressor initialised with the conf decodes them (input after the header)."""
    from tamp_amd import _lib

    lib = _lib.load()
    sz = C.POINTER(C.c_size_t)
    lib.tamp_compressor_init.restype = C.c_int8
    lib.tamp_compressor_init.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tamp_compressor_compress.restype = C.c_int8
    lib.tamp_compressor_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, sz, C.c_char_p, C.c_size_t, sz]
    lib.tamp_compressor_compress_and_flush.restype = C.c_int8
    lib.tamp_compressor_compress_and_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, sz, C.c_char_p, C.c_size_t, sz,
                                                       C.c_bool]
    lib.tamp_decompressor_init.restype = C.c_int8
    lib.tamp_decompressor_init.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint8]
    lib.tamp_decompressor_decompress.restype = C.c_int8
    lib.tamp_decompressor_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, sz, C.c_void_p, C.c_size_t, sz]
    for w in (13, 14, 15):
        for lit in (5, 6):
            for ext in (1, 0):
                custom = (w, lit, ext) == (14, 5, 1)
                text = _rows("synth_text", lit, 200_000, w + lit)
                runs = _rows("stress", lit, 9000, 1) + _rows("stress", lit, 9000, 2)
                dic = _custom_dictionary(w, lit) if custom else None
                tc = _TampConf(window=w, literal=lit, extended=ext, use_custom_dictionary=int(custom))
                obj, window = (C.c_ubyte * 48)(), (C.c_ubyte * (1 << w))()
                if custom:
                    C.memmove(window, dic, 1 << w)
                assert lib.tamp_compressor_init(obj, C.byref(tc), window) == 0
                out = (C.c_ubyte * 400_000)()
                emitted = bytearray()

                def call(fn, data, *extra):
                    nw, nc = C.c_size_t(0), C.c_size_t(0)
                    assert fn(obj, out, len(out), C.byref(nw), data, len(data), C.byref(nc), *extra) == 0
                    assert nc.value == len(data)
                    emitted.extend(bytes(out[: nw.value]))

                pieces = [text[:37], text[37:700], runs[:5000], text[700:9000], text[9000:90_000], text[90_000:90_011],
                          runs[5000:] + text[90_011:170_000], text[170_000:170_500]]
                call(lib.tamp_compressor_compress, pieces[0])                   # token level, ring half full
                call(lib.tamp_compressor_compress_and_flush, pieces[1], True)   # token level
                call(lib.tamp_compressor_compress_and_flush, pieces[2], True)   # compat_segment
                call(lib.tamp_compressor_compress_and_flush, pieces[3], True)   # compat_segment
                call(lib.tamp_compressor_compress, pieces[4])                   # compat_piece
                call(lib.tamp_compressor_compress, pieces[5])                   # token level
                call(lib.tamp_compressor_compress, pieces[6])                   # compat_piece, 11 bytes in the ring
                call(lib.tamp_compressor_compress_and_flush, pieces[7], False)  # token level: the ring is not empty
                ops = [("write", pieces[0]), ("write", pieces[1]), ("flush", True), ("write", pieces[2]), ("flush", True),
                       ("write", pieces[3]), ("flush", True), ("write", pieces[4]), ("write", pieces[5]),
                       ("write", pieces[6]), ("write", pieces[7]), ("flush", False)]
                st, want = oracle.stream_script(ops, window=w, literal=lit, extended=bool(ext), dictionary=dic)
                tag = (w, lit, ext, custom)
                assert st == 0 and bytes(emitted) == want, tag + (len(emitted), len(want))
                # the conf handed to init, the input starting after the header (the window buffer was compressed into:
                # a custom dictionary is put back first)
                if custom:
                    C.memmove(window, dic, 1 << w)
                plain = b"".join(pieces)
                d = (C.c_ubyte * 24)()
                assert lib.tamp_decompressor_init(d, C.byref(tc), window, w) == 0, tag
                back = (C.c_ubyte * (len(plain) + 64))()
                cbuf = (C.c_ubyte * (len(want) - 1)).from_buffer_copy(want[1:])
                nw, nc = C.c_size_t(0), C.c_size_t(0)
                r = lib.tamp_decompressor_decompress(d, back, len(back), C.byref(nw), cbuf, len(want) - 1, C.byref(nc))
                assert (r, bytes(back[: nw.value]), nc.value) == (2, plain, len(want) - 1), tag


# ---------------------------------------------------------------------------------------------------------------------
# 6. encoder objects
# ---------------------------------------------------------------------------------------------------------------------
def test_encoder_objects_replay_the_matrix_call_scripts(ta):
    """tests/golden/config_matrix.json's call scripts on EncoderBatch objects (the resume kernel): every call's status,
    bytes and consumed count as the reference object returned them -- literal 5-8, windows up to 2^15, the 3-byte
    minimum matches, a custom dictionary, lazy matching, dictionary_reset and EXCESS_BITS in the middle of a piece."""
    recs = load_golden("config_matrix.json")["encoders"]
    for rec in recs:
        src, d = _matrix_bytes(rec["source"]), _matrix_bytes(rec["dictionary"])
        ops = [[op[0], src[op[1] : op[2]]] + op[3:] if op[0] in ("compress", "sink", "compress_and_flush") else op
               for op in rec["ops"]]
        emitted, want, pos = unb64(rec["emitted"]), [], 0
        for r, n, k in rec["calls"]:  # each call's bytes are the next slice of what the script emitted
            want.append((r, emitted[pos : pos + n], k))
            pos += n
        enc = ta.EncoderBatch(1, dictionary=d, **rec["conf"])
        got = []
        for op in ops:
            if op[0] == "sink":
                got.append((0, b"", int(enc.sink([op[1]])[0])))
                continue
            if op[0] == "poll":
                st, outs, cons = enc.poll([op[1]])
            elif op[0] == "flush":
                st, outs, cons = enc.flush([op[2]], bool(op[1]))
            elif op[0] == "compress":
                st, outs, cons = enc.compress([op[1]], [op[2]])
            else:
                st, outs, cons = enc.compress_and_flush([op[1]], [op[3]], bool(op[2]))
            got.append((int(st[0]), outs[0], int(cons[0])))
        for k, (g, wnt) in enumerate(zip(got, want)):
            assert g == wnt, (rec["name"], k, ops[k][0])
        assert len(got) == len(want)
