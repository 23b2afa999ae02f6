"""Round 5, GPU tier: ONE long v1 stream decoded by the whole device (tamp_decompress_long_kernel.hpp: chunk starts settled by
speculative parses, records per chunk, the split decoder's RESOLVE over groups in order) against the reference C / the
oracle -- bytes, status, consumed count -- and against the exact decoders the launcher falls back to
(reference: tamp/_c_src/tamp/decompressor.c:371-578)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@pytest.fixture(scope="module")
def checker():
    from oracle.checker import Oracle, Ref

    return Ref() if Ref.available() else Oracle()


def _corpus(kind, n):
    from tamp_amd import workloads as wl

    blob = wl.real_text(kind)
    return (blob * (n // len(blob) + 1))[:n]


def _long_path_lines(capfd):
    """The long-stream decoder's debug lines since the last look (TAMP_AMD_LONGDEC_DEBUG): -> (decoded, reasons it declined for).
    Without them a long path that hands every stream to the exact decoders returns the same bytes and nobody notices."""
    import re

    err = capfd.readouterr().err
    return bool(re.search(r"\[tamp_amd long decode\] \d+ groups, ", err)), re.findall(r"\[tamp_amd long decode\] declined: (.+)", err)


def _same_as_checker(ta, checker, blob, cap, dictionary=None):
    r = ta.decompress_batch([blob], out_cap=cap, dictionary=dictionary)
    st, out, used = checker.decompress(blob, cap=cap, dictionary=dictionary)
    assert int(r.status[0]) == st
    assert bytes(r.stream(0)) == out
    if r.in_consumed is not None:
        assert int(r.in_consumed[0]) == used
    return st, out


CASES = [
    ("prose_w10", dict(), "prose", 3_000_000),
    ("python_w8", dict(window=8), "python", 1_500_000),
    ("python_w12", dict(window=12), "python", 1_500_000),
    ("markup_w15", dict(window=15), "markup", 1_500_000),
    ("prose_literal7", dict(literal=7), "prose7", 1_200_000),
    ("zeros", dict(), "zeros", 2_000_000),          # one token repeated: chunk starts settle a chunk at a time
    ("random", dict(), "random", 600_000),            # all literals
    ("period_1000", dict(), "period", 3_500_000),    # matches only
]


def _data(kind, n):
    if kind == "zeros":
        return bytes(n)
    if kind == "random":
        return np.random.default_rng(11).integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "period":
        unit = np.random.default_rng(12).integers(97, 123, 1000, dtype=np.uint8).tobytes()
        return (unit * (n // 1000 + 1))[:n]
    if kind == "prose7":
        return bytes(b & 127 for b in _corpus("prose", n))
    return _corpus(kind, n)


@pytest.mark.parametrize("name,conf,kind,n", CASES, ids=[c[0] for c in CASES])
def test_one_long_v1_stream_decodes_like_the_reference(ta, checker, name, conf, kind, n, monkeypatch, capfd):
    data = _data(kind, n)
    blob = ta.compress(data, extended=False, **conf)
    assert len(blob) >= 256 << 10 or kind in ("zeros",)  # (long enough for the long-stream decoder; zeros compress to 280 KB)
    assert bytes(ta.decompress(blob)) == data
    monkeypatch.setenv("TAMP_AMD_LONGDEC_DEBUG", "1")
    capfd.readouterr()
    st, out = _same_as_checker(ta, checker, blob, n + 100)
    assert st == 2 and out == data
    assert _long_path_lines(capfd) == (True, [])  # decoded by the long path, not handed on
    # groups through RESOLVE one launch after the other: the same bytes
    monkeypatch.setenv("TAMP_AMD_LONGDEC_CHAIN", "0")
    r = ta.decompress_batch([blob], out_cap=n + 100)
    assert int(r.status[0]) == 2 and bytes(r.stream(0)) == data
    # the exact decoders give the same answer (the path the launcher falls back to)
    monkeypatch.setenv("TAMP_AMD_LONGDEC", "0")
    r = ta.decompress_batch([blob], out_cap=n + 100)
    assert int(r.status[0]) == 2 and bytes(r.stream(0)) == data


EXT_CASES = [
    ("prose_w10", dict(), "prose", 3_000_000),
    ("python_w8", dict(window=8), "python", 1_500_000),      # runs of blanks: an RLE lag every few hundred bytes
    ("python_w10", dict(), "python", 2_500_000),
    ("python_w12", dict(window=12), "python", 1_500_000),
    ("markup_w15", dict(window=15), "markup", 1_500_000),
    ("prose_literal7", dict(literal=7), "prose7", 1_200_000),
    ("prose_literal6", dict(literal=6), "prose6", 1_200_000),  # the seeded dictionary of 6-bit literals (decompressor.c:318-319)
    # nothing but 241-byte RLE tokens, every one lagging: 9 + 8 + 4 = 21 bits each, so 48 or 49 start in a 1,024-bit chunk -- below
    # the 63 a group lists, every group is ONE chunk (two would pass 63), and the long path takes the stream: what the case
    # measures is the long path with 320,000 one-chunk groups, not the fall-back ("lags per chunk" would be 64 and more)
    ("zeros", dict(), "zeros", 40_000_000),
    ("random", dict(), "random", 600_000),
    ("period_1000", dict(), "period", 3_500_000),    # extended matches of 130+ bytes, clipped at the ring's end
    ("runs_mixed", dict(), "runs", 2_000_000),       # runs of 2..300 bytes between words
]


@pytest.mark.parametrize("name,conf,kind,n", EXT_CASES, ids=[c[0] for c in EXT_CASES])
def test_one_long_extended_stream_decodes_like_the_reference(ta, checker, name, conf, kind, n, monkeypatch, capfd):
    """Round 6: the library's default format.  RLE / extended-match tokens write fewer bytes to the window than they produce
    (decompressor.c:162-170,266-268); window_pos at those tokens comes from one pass over them (tamp_long_wp_kernel), the
    groups' lag lists from there."""
    if kind == "prose6":
        data = bytes(b & 63 for b in _corpus("prose", n))
    elif kind == "runs":
        rng = np.random.default_rng(21)
        words = _corpus("prose", 400_000).split()
        parts, size = [], 0
        while size < n:
            w = words[int(rng.integers(len(words)))]
            run = bytes([int(rng.integers(32, 127))]) * int(rng.integers(2, 300))
            parts += [w, run]
            size += len(w) + len(run)
        data = b"".join(parts)[:n]
    else:
        data = _data(kind, n)
    blob = ta.compress(data, **conf)  # extended = the default
    assert blob[0] & 2
    monkeypatch.setenv("TAMP_AMD_LONGDEC_MIN", "65536")  # (the long-stream decoder from 64 KiB of compressed bytes on)
    assert len(blob) >= 64 << 10
    monkeypatch.setenv("TAMP_AMD_LONGDEC_DEBUG", "1")
    capfd.readouterr()
    st, out = _same_as_checker(ta, checker, blob, len(data) + 100)
    assert st == 2 and out == data
    assert _long_path_lines(capfd) == (True, [])  # decoded by the long path, not handed on
    assert bytes(ta.decompress(blob)) == data
    # the exact decoders give the same answer (the path the launcher falls back to)
    monkeypatch.setenv("TAMP_AMD_LONGDEC_EXT", "0")
    r = ta.decompress_batch([blob], out_cap=len(data) + 100)
    assert int(r.status[0]) == 2 and bytes(r.stream(0)) == data
    monkeypatch.delenv("TAMP_AMD_LONGDEC_EXT")
    # cut near the end and corrupted in the middle: whatever the reference makes of it
    for cut in (1, 2, 3, 7):
        _same_as_checker(ta, checker, blob[: len(blob) - cut], len(data) + 100)
    rng = np.random.default_rng(6)
    for _ in range(3):
        bad = bytearray(blob)
        bad[int(rng.integers(1000, len(bad)))] ^= 1 << int(rng.integers(8))
        _same_as_checker(ta, checker, bytes(bad), len(data) + 4096)


def test_long_stream_with_custom_dictionary_flush_tokens_and_a_tail(ta, checker):
    import io

    data = _corpus("prose", 1_600_000)
    dic = data[70_000:71_024]
    blob = ta.compress(data, extended=False, dictionary=dic)
    assert bytes(ta.decompress(blob, dictionary=dic)) == data
    _same_as_checker(ta, checker, blob, len(data) + 64, dictionary=dic)
    # FLUSH tokens inside the stream (decompressor.c:501-514: pad to the byte boundary), pieces of odd sizes
    f = io.BytesIO()
    with ta.Compressor(f, extended=False) as c:
        pos = 0
        for k, step in enumerate((300_001, 17, 250_000, 1, 400_000, 123_457, 526_524)):
            c.write(data[pos : pos + step])
            pos += step
            if k % 2 == 0:
                c.flush(write_token=True)
    blob = f.getvalue()
    assert pos == len(data) and len(blob) >= 256 << 10
    st, out = _same_as_checker(ta, checker, blob, len(data) + 64)
    assert st == 2 and out == data
    # cut anywhere near the end: partial tokens, status and consumed count as the reference's
    for cut in (1, 2, 3, 5, 9):
        _same_as_checker(ta, checker, blob[: len(blob) - cut], len(data) + 64)


def test_what_the_long_stream_decoder_declines_goes_to_the_exact_decoders(ta, checker):
    data = _corpus("python", 1_200_000)
    blob = bytearray(ta.compress(data, extended=False))
    # output room too small: TAMP_OUTPUT_FULL with the partial last token, like the reference
    _same_as_checker(ta, checker, bytes(blob), 500_000)
    _same_as_checker(ta, checker, bytes(blob), len(data))  # exactly enough
    # a corrupted byte in the middle: whatever the reference makes of it (an out-of-bounds offset, or other bytes)
    rng = np.random.default_rng(5)
    for _ in range(6):
        bad = bytearray(blob)
        bad[int(rng.integers(1000, len(bad)))] ^= 1 << int(rng.integers(8))
        _same_as_checker(ta, checker, bytes(bad), len(data) + 4096)
    # extended-format and dictionary-reset streams are not its business
    ext = ta.compress(data, extended=True)
    _same_as_checker(ta, checker, ext, len(data) + 64)


def test_long_stream_decode_rate(ta):
    """32 MB of prose, v1: the stream came back at 7.3 MB/s through one wavefront; the bar here is 150 MB/s end to end
    through the host-memory call (measured: ~500; groups resolved one launch after the other: ~250)."""
    import time

    data = _corpus("prose", 32_000_000)
    blob = ta.compress(data, extended=False)
    ta.decompress(blob[: 300_000] + b"")  # (warm-up: scratch, code objects)
    t0 = time.time()
    out = ta.decompress(blob)
    dt = time.time() - t0
    assert bytes(out) == data
    assert len(data) / dt > 150e6, dt


def test_a_handful_of_long_streams_in_one_call(ta, checker):
    """Up to sixteen long v1 streams in one decode call take the long-stream decoder one after the other; a batch with a short or an
    extended-format stream among them goes to the exact decoders whole.  Same bytes, statuses and consumed counts either way."""
    datas = [_corpus("prose", 700_000), _corpus("python", 900_000), _corpus("markup", 650_000)]
    blobs = [ta.compress(d, extended=False) for d in datas]
    r = ta.decompress_batch(blobs, out_cap=1_000_000)
    for i, (b, d) in enumerate(zip(blobs, datas)):
        st, out, used = checker.decompress(b, cap=1_000_000)
        assert (int(r.status[i]), bytes(r.stream(i))) == (st, out) and out == d
        if r.in_consumed is not None:
            assert int(r.in_consumed[i]) == used
    mixed = blobs + [ta.compress(datas[0][:5000], extended=False), ta.compress(datas[1], extended=True)]
    r = ta.decompress_batch(mixed, out_cap=1_000_000)
    for i, b in enumerate(mixed):
        st, out, used = checker.decompress(b, cap=1_000_000)
        assert (int(r.status[i]), bytes(r.stream(i))) == (st, out)
