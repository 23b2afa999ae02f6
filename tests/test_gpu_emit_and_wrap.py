"""GPU tier: the emit phase's direct token placement (token_words: every token ORed to its place in the bit buffer) and the
wrapped compare (prefix_len_wrapped16) at each of its call sites, against the reference C (the oracle when the
reference library is not built): status and bytes of every stream.  At window 2^10 / literal 8 the fixed-geometry build is
compared with the generic build (TAMP_AMD_FIXED_BUILD=0) as well.

What the inputs aim at:
  bit phases     near-incompressible streams -- nine bits per byte, so the bit phase walks through all 32 values and tokens
                 cross words at every offset -- at lengths around every block boundary;
  wide tokens    small and large windows x every literal width (the literal / match token widths 6..24), streams that end
                 with EXCESS_BITS, and periodic data at window 2^14, whose settled extended-match tokens reach 32 bits;
  K > 4          the one-wavefront build on messages with more than 4 x 64 tokens (the emit's uncached token loop);
  carry / lags   4 KiB streams with long runs and 37-byte periodic text: several flushes, carried bits, re-based epochs;
  wrap zone      candidates within 15 bytes of the newest window byte (periodic data of period 1..16), at the first block
                 boundary, at the first positions of the first epoch (the second 16-byte read starts in front of the
                 buffer), from the interior of listed runs (second pass), and under lazy matching (the probe);
  block mode     one long v1 stream whose blocks OR their bits into the output.
"""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

FORMATS = [True, False]


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@pytest.fixture(scope="module")
def checker():
    from oracle.checker import Oracle, Ref

    return Ref() if Ref.available() else Oracle()


@contextlib.contextmanager
def generic_build():
    old = os.environ.get("TAMP_AMD_FIXED_BUILD")
    os.environ["TAMP_AMD_FIXED_BUILD"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["TAMP_AMD_FIXED_BUILD"]
        else:
            os.environ["TAMP_AMD_FIXED_BUILD"] = old


def expected(checker, streams, **kw):
    from tamp_amd.batch import pack_streams

    flat, off, ln = pack_streams(streams)
    kw.pop("max_in_len", None)  # (a launch hint, nothing of the format)
    if "lazy_matching" in kw:
        kw["lazy"] = kw.pop("lazy_matching")  # (the checker's name for it)
    return checker.compress_batch(flat if flat.size else np.zeros(1, np.uint8), off, ln, threads=8, **kw)


def assert_equal(got, want, streams, tag):
    for i in range(len(streams)):
        assert int(got.status[i]) == int(want.status[i]), (tag, i, len(streams[i]), "status")
        assert got.stream(i) == want.stream(i), (tag, i, len(streams[i]), "bytes")


def check(ta, checker, streams, tag, both_builds=False, **kw):
    """One batch (<= 256 streams) against the checker; both_builds: window 2^10 / literal 8, the fixed and the generic build."""
    assert len(streams) <= 256
    want = expected(checker, streams, **kw)
    assert_equal(ta.compress_batch(streams, **kw), want, streams, tag)
    if both_builds:
        assert kw.get("window", 10) == 10 and kw.get("literal", 8) == 8
        with generic_build():
            assert_equal(ta.compress_batch(streams, **kw), want, streams, tag + ("generic",))
    return want


def text(n, row=0):
    from tamp_amd import workloads as wl

    return wl.synth_text(row + 1, n)[row].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# every bit phase and word crossing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", FORMATS)
def test_every_bit_phase_and_word_crossing(ta, checker, extended):
    rng = np.random.default_rng(20261018)
    lens = list(range(1, 71)) + [255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096]
    streams = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    want = check(ta, checker, streams, ("phases", extended), both_builds=True, window=10, literal=8, extended=extended)
    # nearly nothing matches: nine bits per byte behind the header, so every phase 0..31 occurs as a token's first bit
    assert int(want.out_len[-1]) > 4096
    short = [s for s in streams if len(s) <= 257]  # (a batch of short messages: the one-wavefront build)
    check(ta, checker, short, ("phases, short", extended), window=10, literal=8, extended=extended)


# ---------------------------------------------------------------------------------------------------------------------
# wide tokens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", FORMATS)
def test_token_widths_at_small_and_large_windows(ta, checker, extended):
    rng = np.random.default_rng(7)
    statuses = set()
    for window in (8, 9, 12, 14):
        for literal in (5, 6, 7, 8):
            mask = np.uint8((1 << literal) - 1)
            t = np.frombuffer(text(3000, window + literal), dtype=np.uint8) & mask
            noise = rng.integers(0, 256, 1500, dtype=np.uint8) & mask
            runs = np.concatenate([np.full(n, (7 * i + 1) & int(mask), np.uint8) for i, n in enumerate((1, 2, 3, 9, 17, 40, 250, 400))])
            streams = [t.tobytes(), noise.tobytes(), runs.tobytes(), (t[:180].tobytes() * 12), t[:700].tobytes(), noise[:333].tobytes()]
            if literal < 8:  # one byte above the literal width: the stream ends there with EXCESS_BITS
                for src, pos in ((t, 1500), (noise, 77), (t[:700], 699)):
                    bad = src.copy()
                    bad[pos] = 1 << literal
                    streams.append(bad.tobytes())
            want = check(ta, checker, streams, ("widths", window, literal, extended), window=window, literal=literal, extended=extended)
            statuses |= {int(s) for s in want.status}
            short = [s for s in streams if len(s) < 960]
            check(ta, checker, short, ("widths, short", window, literal, extended), window=window, literal=literal, extended=extended)
    assert statuses == {0, -2}


CODE = (0x00, 0x03, 0x08, 0x0b, 0x14, 0x24, 0x26, 0x2b, 0x4b, 0x54, 0x94, 0x95, 0xaa, 0x27, 0xab)  # compressor.c:33-36
NBITS = (2, 3, 5, 5, 6, 7, 7, 7, 8, 8, 9, 9, 9, 7, 9)


def token_widths(comp, n_in, window, literal, minp):
    """Bit widths of the tokens of an extended-format stream that decodes to n_in bytes -> (all widths, extended-match sizes)."""
    bits = "".join(format(b, "08b") for b in comp)
    table = {format(c, "0%db" % (n - 1)): i for i, (c, n) in enumerate(zip(CODE, NBITS))}

    def symbol(p):
        k = ""
        while k not in table:
            k += bits[p]
            p += 1
        return table[k], p

    p, done, widths, sizes = 8, 0, [], []
    while done < n_in:
        s = p
        if bits[p] == "1":
            p += 1 + literal
            done += 1
        else:
            sym, p = symbol(p + 1)
            if sym == 12:    # RLE: count - 2 = code << 4 | 4 bits
                ci, p = symbol(p)
                done += ((ci << 4) | int(bits[p:p + 4], 2)) + 2
                p += 4
            elif sym == 13:  # extended match: size - min - 12 = code << 3 | 3 bits, then the window index
                ci, p = symbol(p)
                sizes.append(((ci << 3) | int(bits[p:p + 3], 2)) + minp + 12)
                done += sizes[-1]
                p += 3 + window
            else:
                assert sym < 12
                done += sym + minp
                p += window
        widths.append(p - s)
    assert done == n_in
    return widths, sizes


def test_settled_extended_match_tokens_of_32_bits(ta, checker):
    """Periodic data at window 2^14, extended format: extended matches of 14 .. 133 bytes; symbol 13 (7 bits), a size code of
    8 + 3 bits (sizes 94 .. 117 and 126 .. 133) and 14 window bits are one 32-bit token, the widest the emit places.  The
    expected streams are parsed here: they hold such tokens, and none wider.  Streams of two periods and a bit have ONE
    earlier copy of every pattern, which is when the match phase settles the token itself (no rival); whether it did is
    not visible in the bytes."""
    rng = np.random.default_rng(14)
    streams = []
    for period in (150, 151, 233, 377, 512, 600):
        block = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
        streams.append((block * (9000 // period + 1))[:9000])
        streams.append(text(700, period) + (block * 20)[:5000 + period])
        for extra in (94, 117, 133, 2 * 133 + 100, period - 3):  # one earlier copy only
            streams.append(block + block[:extra] + text(60, extra))
    want = check(ta, checker, streams, ("ext32",), window=14, literal=8, extended=True)
    wide = 0
    for i, s in enumerate(streams):
        widths, sizes = token_widths(want.stream(i), len(s), 14, 8, 2)
        assert max(widths) <= 32 and all(14 <= z <= 133 for z in sizes), (i, max(widths))
        wide += sum(w == 32 for w in widths)
        if len(s) == 9000:
            assert 32 in widths, i
    assert wide >= 100, wide


# ---------------------------------------------------------------------------------------------------------------------
# more than four tokens per thread: the emit's uncached loop
# ---------------------------------------------------------------------------------------------------------------------
def test_uncached_token_loop_of_the_short_message_build(ta, checker):
    from tamp_amd import workloads as wl

    rng = np.random.default_rng(900)
    for extended in FORMATS:
        msgs = [rng.integers(0, 256, 900, dtype=np.uint8).tobytes() for _ in range(64)]  # ~900 tokens on 64 threads
        check(ta, checker, msgs, ("random 900", extended), window=8, literal=8, extended=extended, max_in_len=900)
    dic = wl.telemetry_dictionary(bytes(ta.initialize_dictionary(256, literal=7)))
    rows = wl.telemetry(256, 256)
    msgs = [rows[i].tobytes() for i in range(256)]
    for extended in FORMATS:
        check(ta, checker, msgs, ("telemetry", extended), window=8, literal=7, extended=extended, dictionary=dic, max_in_len=256)


# ---------------------------------------------------------------------------------------------------------------------
# carried bits and lags across epochs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", FORMATS)
def test_carry_and_lags_across_epochs(ta, checker, extended):
    from tamp_amd import workloads as wl

    prose, py = wl.real_text("prose", frozen_only=True), wl.real_text("python", frozen_only=True)
    n = 4096
    streams = []
    for i in range(24):
        if i % 2 == 0:  # long runs, runs that reach the end of the stream
            s = (b"a" * 300 + prose[i * 911:i * 911 + 200] + b" " * 90 + b"xy" * 50 + bytes(400))[:n]
            s = s + b"z" * (n - len(s))
        else:           # periodic data: extended matches that run into the window's end
            s = (py[i * 1301:i * 1301 + 37] * 120)[:n]
        assert len(s) == n
        streams.append(s)
    check(ta, checker, streams, ("carry", extended), both_builds=True, window=10, literal=8, extended=extended)


# ---------------------------------------------------------------------------------------------------------------------
# wrap zone
# ---------------------------------------------------------------------------------------------------------------------
def periodic_inputs():
    rng = np.random.default_rng(15)
    out = []
    for period in range(1, 17):  # (16: a 16-byte hit exactly 16 bytes in front of the newest byte takes the wrapped compare too)
        pat = bytes(rng.choice(np.arange(33, 127), period, replace=False).astype(np.uint8))
        for n in (40, 700, 1100, 2100):
            out.append((period, (pat * (n // period + 1))[:n]))
    return out


@pytest.mark.parametrize("extended", FORMATS)
def test_wrap_zone_periodic(ta, checker, extended):
    streams = [s for _, s in periodic_inputs()]
    check(ta, checker, streams, ("periodic", extended), both_builds=True, window=10, literal=8, extended=extended)


@pytest.mark.parametrize("extended", FORMATS)
def test_wrap_zone_across_the_first_block_boundary(ta, checker, extended):
    """The periodic inputs behind 1,017 .. 1,031 bytes of text: their wrap candidates straddle position 1,024."""
    streams = [text(1016 + period, period) + s for period, s in periodic_inputs()]
    assert {len(s) - len(t) for (_, t), s in zip(periodic_inputs(), streams)} >= set(range(1017, 1032))
    check(ta, checker, streams, ("boundary", extended), both_builds=True, window=10, literal=8, extended=extended)


@pytest.mark.parametrize("extended", FORMATS)
def test_wrap_zone_at_the_first_positions_of_the_first_epoch(ta, checker, extended):
    """Inputs that repeat the newest bytes of the seeded dictionary: wrap candidates for positions 0, 1, .. of the first
    epoch, where the compare's second read starts up to 15 bytes in front of the buffer."""
    tail = bytes(ta.initialize_dictionary(1024))[-8:]
    streams = [tail * 200, tail * 5 + text(300), tail + text(2000, 1), tail[:2] * 3 + tail * 2 + text(50, 2)]
    for m in range(1, 9):
        streams.append(tail[-m:] * 20)
        streams.append(tail[-m:] + tail[-m:][:1] * 3 + text(1100, m))
    for m in range(9, 16):  # the dictionary's last m bytes, then its OLDEST bytes: the ring's continuation
        d = bytes(ta.initialize_dictionary(1024))
        streams.append(d[-m:] + d[:16 - m] + text(40, m))
    check(ta, checker, streams, ("first positions", extended), both_builds=True, window=10, literal=8, extended=extended)


@pytest.mark.parametrize("extended", FORMATS)
def test_wrap_zone_candidates_inside_listed_runs(ta, checker, extended):
    """A run of 8+ equal bytes x that ends d = 1..15 bytes before a pattern starting with x x: the run's interior is not in
    the index, the second pass finds those candidates, and for d <= 13 they run past the newest window byte (a candidate that
    starts with x x lies t >= d + 2 bytes in front of the pattern; the second pass takes t = 2..15 through the wrapped compare,
    so at d = 14, 15 the same candidates take its ordinary one).  The pattern goes on with
    the bytes the ring continues with (what was written 1,024 bytes earlier), so the wrapped part matches too; a second
    variant goes on with unrelated text."""
    rng = np.random.default_rng(8)
    streams = []
    for d in range(1, 16):
        for runlen in (8, 40):
            for r in (2, 3):
                x = 0x41 + d
                pre = bytes(rng.integers(97, 123, 1100 + 7 * d, dtype=np.uint8))
                filler = bytes(rng.integers(48, 58, d, dtype=np.uint8))
                head = pre + bytes([x]) * runlen + filler
                q = len(head)
                ring = head[q - 1024:q - 1024 + 10]
                streams.append(head + bytes([x]) * r + filler + ring + text(300, d))
                streams.append(head + bytes([x]) * r + text(300, d + 1))
    for i in range(0, len(streams), 128):
        check(ta, checker, streams[i:i + 128], ("runs", extended, i), both_builds=True, window=10, literal=8, extended=extended)


@pytest.mark.parametrize("extended", FORMATS)
def test_wrap_zone_under_lazy_matching(ta, checker, extended):
    streams = [s for _, s in periodic_inputs()]
    streams += [text(1016 + period, period) + s for period, s in periodic_inputs()[::4]]
    check(ta, checker, streams, ("lazy", extended), window=10, literal=8, extended=extended, lazy_matching=True)


# ---------------------------------------------------------------------------------------------------------------------
# block mode
# ---------------------------------------------------------------------------------------------------------------------
def test_block_mode_stream_and_one_byte_short(ta, checker):
    from tamp_amd import workloads as wl

    n = 262144 + 7
    data = wl.real_text("prose", frozen_only=True)[:n]
    assert len(data) == n
    want = expected(checker, [data], window=10, literal=8, extended=False)
    assert int(want.status[0]) == 0
    full = want.stream(0)
    got = ta.compress_batch([data], window=10, literal=8, extended=False)
    assert int(got.status[0]) == 0 and got.stream(0) == full
    cap = len(full) - 1
    flat = np.frombuffer(data, dtype=np.uint8)
    tight = checker.compress_batch(flat, np.zeros(1, np.uint64), np.array([n], np.uint32), out_cap=np.array([cap], np.uint32),
                                   window=10, literal=8, extended=False)
    assert int(tight.status[0]) == 1  # TAMP_OUTPUT_FULL
    short = ta.compress_batch([data], window=10, literal=8, extended=False, out_cap=cap)
    assert int(short.status[0]) == 1 and short.stream(0) == full[:cap]  # ... with the exact prefix (compressor.c:65-75)
