"""GPU tier: lazy matching in bounded pieces -- the cached match of compressor.c:576-619 carried between calls of the batch kernel
(tamp_amd_compress_piece_lazy, TampAmdLazyCarry; kSlotLazyLen / kSlotLazyPos of the kernel's state slot).  All `-m gpu`, bit-exact.

Inputs and expectations are those of tests/test_gpu_lazy.py: tests/lazy_input.py's sweep stream (611 bytes, 13 defers per
configuration) cut at every byte and its decision cells cut around the deciding poll, the oracle's bytes held against the
reference's recorded results in tests/golden/lazy_cells.json, and for every cut of the sweep stream the reference object's
(status, written, consumed) of both calls.  What a piece leaves in its carry is held against the object of the token-level resume
kernel that took the same call (EncoderBatch(lazy_matching=True), pinned to the reference by test_resume_kernel_every_cut).

  1  every cut on the piece path, and the carry after the first piece
  2  hand-over both ways between the resume kernel's object and the piece's carry, at the cuts that hold a cached match
  3  three pieces, the middle one 1 or 17 bytes
  4  every decision cell with the deciding poll as the first piece's last, and one byte to either side
  5  too little output room for an unfinished piece that starts from a cached match
  6  refusals of a cached match that cannot be
  7  Compressor(lazy_matching=True) against live reference objects, per-call counts; bounded memory at the default thresholds
  8  the reference-named objects: large calls of a lazy object on the piece path
"""
import ctypes as C
import hashlib
import io
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

import lazy_input as li  # noqa: E402
import test_gpu_lazy as tgl  # noqa: E402  (want, describe, CONFIGS, SWEEPS: the same expectations, computed once)
from test_gpu_cut_sweep import STATE_BYTES, EncoderState, _ring  # noqa: E402

SWEEP_IDS = [f"w{w}-{'ext' if e else 'v1'}" for w, e in tgl.SWEEPS]
sweeps = pytest.mark.parametrize("window,extended", tgl.SWEEPS, ids=SWEEP_IDS)
EXCESS_BITS, OUTPUT_FULL = -2, 1


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@pytest.fixture(scope="module")
def golden():
    return tgl.load_golden("lazy_cells.json")


@pytest.fixture(autouse=True)
def no_tuning_env(monkeypatch):
    for k in tgl.TUNING_ENV:
        monkeypatch.delenv(k, raising=False)


def show(lz) -> str:
    c = lz.carry
    return (f"carry(cached={lz.cached_len}@{lz.cached_pos} rle={c.rle_count} ext={c.ext_count}@{c.ext_pos} bits={c.bit_count}:{c.bits:#010x} "
            f"tail={bytes(c.tail[: min(c.tail_len, 16)])!r})")


class Pieces:
    """Piece calls through the C ABI (as tamp_amd/codec.py makes them), and per sweep configuration the first piece and the resume
    kernel's object of every cut -- each computed once, whichever test asks first, and never modified."""

    def __init__(self, ta, oracle, golden):
        from tamp_amd import _lib

        self.ta, self.oracle, self.golden, self._lib, self.lib = ta, oracle, golden, _lib, _lib.load()
        self._sweep = {}

    def conf(self, window, literal, extended, lazy=True, custom=False):
        return self._lib.TampAmdConf(window, literal, int(custom), int(extended), 0, int(lazy))

    def piece(self, conf, win, wp, lz, data, *, first, resume, finish, cap=None):
        n = len(data)
        if cap is None:
            cap = self.lib.tamp_amd_compress_bound(n + 272, conf.literal, 0) + 8
        out = (C.c_ubyte * (cap + 1))()
        written, token = C.c_size_t(0), C.c_int(0)
        src = (C.c_ubyte * max(n, 1)).from_buffer_copy(data if n else b"\0")
        res = self.lib.tamp_amd_compress_piece_lazy(C.byref(conf), int(first), 0, int(resume), int(finish), 0, win, C.byref(wp),
                                                    C.byref(lz), out, cap, C.byref(written), src, n, C.byref(token), 0)
        assert written.value <= cap
        return res, C.string_at(out, written.value)

    def fresh(self, window, dictionary=None):
        W = 1 << window
        win = (C.c_ubyte * W).from_buffer_copy(dictionary) if dictionary is not None else (C.c_ubyte * W)()
        return win, C.c_uint16(0), self._lib.TampAmdLazyCarry()

    def copies(self, window, first):
        """Fresh copies of what a first piece left: (window buffer, window_pos, carry)."""
        _, lz, win, wp = first
        return (C.c_ubyte * (1 << window)).from_buffer_copy(win), C.c_uint16(wp), self._lib.TampAmdLazyCarry.from_buffer_copy(lz)

    def sweep(self, window, extended):
        key = (window, extended)
        if key not in self._sweep:
            src, marks = li.sweep_source(window, extended)
            rec = next(r for r in self.golden["sweep"] if (r["window"], r["extended"]) == key)
            rc, whole = self.oracle.compress(src, window=window, literal=8, extended=extended, lazy_matching=True)
            assert rc == 0 and rec["input_sha256"] == hashlib.sha256(src).hexdigest() and rec["whole_sha256"] == hashlib.sha256(whole).hexdigest()
            n, W = len(src), 1 << window
            assert len(rec["cuts"]) == n + 1 and rec["cap"] == tgl.CAP
            t0 = time.perf_counter()
            enc = self.ta.EncoderBatch(n + 1, window=window, literal=8, extended=extended, lazy_matching=True)
            st1, out1_a, k1 = enc.compress([src[:c] for c in range(n + 1)], tgl.CAP)
            states1 = enc.states.copy()
            firsts = []
            for c in range(n + 1):
                win, wp, lz = self.fresh(window)
                res, out1 = self.piece(self.conf(window, 8, extended), win, wp, lz, src[:c], first=True, resume=False, finish=False)
                assert res == 0, (SWEEP_IDS[tgl.SWEEPS.index(key)], tgl.describe(marks, c), "first piece returned", res)
                firsts.append((out1, self._lib.TampAmdLazyCarry.from_buffer_copy(lz), C.string_at(win, W), wp.value))
            print(f"lazy pieces {SWEEP_IDS[tgl.SWEEPS.index(key)]}: {n + 1} objects in one launch, {n + 1} first pieces, {time.perf_counter() - t0:.2f} s")
            held = [c for c, f in enumerate(firsts) if f[1].cached_len]
            near = sorted({x for c in held for x in (c - 1, c, c + 1) if 0 <= x <= n})
            self._sweep[key] = dict(src=src, marks=marks, rec=rec, whole=whole, states1=states1, out1_a=out1_a, firsts=firsts, held=held,
                                    near=near, name=SWEEP_IDS[tgl.SWEEPS.index(key)])
        return self._sweep[key]

    def state_of(self, s, c) -> EncoderState:
        return EncoderState.from_buffer_copy(s["states1"][c, :STATE_BYTES].tobytes())


@pytest.fixture(scope="module")
def pieces(ta, oracle, golden):
    return Pieces(ta, oracle, golden)


# ---------------------------------------------------------------------------------------------------------------------
# 1: every cut, piece path
# ---------------------------------------------------------------------------------------------------------------------
@sweeps
def test_piece_path_every_cut_and_its_carry(pieces, window, extended):
    """src[:c] as an unfinished piece on a fresh object, src[c:] as the finishing one: both return 0, the first is a prefix of the
    one-shot stream and runs at most four bytes ahead of the reference object's first call (the object sits on its last token's
    bits until the next poll, compressor.c:549-551; a piece hands every whole byte over at once), and the two together are the
    one-shot stream.  What the first piece leaves is, field by field, the state of the resume kernel's object after the same call:
    cached match, run, extended match, ring, window, window position, pending bits."""
    s = pieces.sweep(window, extended)
    src, marks, whole, W = s["src"], s["marks"], s["whole"], 1 << window
    t0 = time.perf_counter()
    for c, first in enumerate(s["firsts"]):
        out1, lz, win, wp = first
        carry, st = lz.carry, pieces.state_of(s, c)
        where = f"{s['name']}: {tgl.describe(marks, c)}, {show(lz)}"
        wl1 = s["rec"]["cuts"][c][1]
        assert out1 == whole[: len(out1)], (where, "bytes of the first piece")
        assert 0 <= len(out1) - wl1 <= 4, (where, f"{len(out1)} bytes against the reference object's {wl1}")
        assert lz.reserved2 == 0 and carry.reserved == 0 and carry.bit_count <= 7 and carry.tail_len <= 16, where
        if st.cached_match_index >= 0:
            assert (lz.cached_pos, lz.cached_len) == (st.cached_match_index, st.cached_match_size), \
                (where, f"object holds index {st.cached_match_index} size {st.cached_match_size}")
            assert carry.rle_count == 0 and carry.ext_count == 0 and lz.cached_len <= carry.tail_len, where
        else:
            assert (lz.cached_pos, lz.cached_len) == (0, 0), (where, "the object holds no cached match")
        assert carry.rle_count == st.rle_count, (where, f"object rle_count {st.rle_count}")
        assert carry.ext_count == st.extended_match_count, (where, f"object count {st.extended_match_count}")
        if carry.ext_count:
            assert carry.ext_pos == st.extended_match_position, (where, f"object position {st.extended_match_position}")
        assert bytes(carry.tail[: carry.tail_len]) == _ring(st), (where, f"object ring {_ring(st)!r}")
        assert wp == st.window_pos, (where, f"window_pos {wp} vs object {st.window_pos}")
        assert win == s["states1"][c, STATE_BYTES : STATE_BYTES + W].tobytes(), (where, "window bytes")
        # pending bits: as many bits have been produced either way; the piece's < 8 are the object's last ones
        assert 8 * len(out1) + carry.bit_count == 8 * len(s["out1_a"][c]) + st.bit_buffer_pos, \
            (where, f"{len(out1)} bytes + {carry.bit_count} bits vs object {len(s['out1_a'][c])} bytes + {st.bit_buffer_pos} bits")
        if carry.bit_count:
            pending = (st.bit_buffer >> (32 - st.bit_buffer_pos)) & ((1 << carry.bit_count) - 1)
            assert carry.bits >> (32 - carry.bit_count) == pending, (where, f"object bits {st.bit_buffer:#010x}/{st.bit_buffer_pos}")
        win2, wp2, lz2 = pieces.copies(window, first)
        res, out2 = pieces.piece(pieces.conf(window, 8, extended), win2, wp2, lz2, src[c:], first=False, resume=True, finish=True)
        assert res == 0, (where, f"finishing piece returned {res}")
        assert out1 + out2 == whole, (where, "first piece + finishing piece")
        assert bytes(lz2) == bytes(32), (where, f"a finishing piece left {show(lz2)}")
    assert len(s["held"]) >= 5, f"{s['name']}: only {len(s['held'])} cuts left a cached match in the carry"
    print(f"lazy pieces {s['name']}: {len(s['firsts'])} finishing pieces, {len(s['held'])} cuts held a cached match, {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------------------------------
# 2: hand-over both ways
# ---------------------------------------------------------------------------------------------------------------------
@sweeps
def test_resume_kernel_state_finished_by_a_piece(pieces, window, extended):
    """The resume kernel's object after src[:c], turned into a carry the way the reference-named objects do it (cached_match_index
    -1 = no cached match; bit_count is the object's bit_buffer_pos, up to 31 on entry), finished by ONE finishing piece."""
    s = pieces.sweep(window, extended)
    src, W = s["src"], 1 << window
    assert s["near"]
    for c in s["near"]:
        st = pieces.state_of(s, c)
        lz = pieces._lib.TampAmdLazyCarry()
        carry = lz.carry
        if st.cached_match_index >= 0:
            lz.cached_pos, lz.cached_len = st.cached_match_index, st.cached_match_size
        carry.rle_count, carry.ext_count, carry.ext_pos = st.rle_count, st.extended_match_count, st.extended_match_position
        carry.bit_count, carry.bits, carry.tail_len = st.bit_buffer_pos, st.bit_buffer, st.input_size
        for k, byte in enumerate(_ring(st)):
            carry.tail[k] = byte
        where = f"{s['name']}: {tgl.describe(s['marks'], c)}, object state as {show(lz)}"
        win = (C.c_ubyte * W).from_buffer_copy(s["states1"][c, STATE_BYTES : STATE_BYTES + W].tobytes())
        wp = C.c_uint16(st.window_pos)
        res, out = pieces.piece(pieces.conf(window, 8, extended), win, wp, lz, src[c:], first=False, resume=True, finish=True)
        assert res == 0, (where, f"finishing piece returned {res}")
        assert s["out1_a"][c] + out == s["whole"], (where, "object bytes + finishing piece")
    assert sum(pieces.state_of(s, c).cached_match_index >= 0 for c in s["near"]) >= 5


@sweeps
def test_piece_carry_finished_by_the_resume_kernel(pieces, window, extended):
    """What the first piece left, written into encoder objects the way the reference-named objects take a piece's carry back, the
    cuts finished in ONE compress_and_flush launch of the resume kernel."""
    s = pieces.sweep(window, extended)
    src, W, cuts = s["src"], 1 << window, s["near"]
    enc = pieces.ta.EncoderBatch(len(cuts), window=window, literal=8, extended=extended, lazy_matching=True)
    for k, c in enumerate(cuts):
        _, lz, win, wp = s["firsts"][c]
        carry = lz.carry
        st = EncoderState.from_buffer_copy(enc.states[k, :STATE_BYTES].tobytes())  # (conf fields as initialised)
        st.window_pos = wp
        st.cached_match_index, st.cached_match_size = (lz.cached_pos, lz.cached_len) if lz.cached_len else (-1, 0)
        st.rle_count, st.extended_match_count, st.extended_match_position = carry.rle_count, carry.ext_count, carry.ext_pos
        st.bit_buffer_pos, st.bit_buffer = carry.bit_count, (carry.bits if carry.bit_count else 0)
        st.input_pos, st.input_size = 0, carry.tail_len
        for j in range(16):
            st.input[j] = carry.tail[j] if j < carry.tail_len else 0
        st.last_was_flush = 0
        enc.states[k, :STATE_BYTES] = np.frombuffer(bytes(st), dtype=np.uint8)
        enc.states[k, STATE_BYTES : STATE_BYTES + W] = np.frombuffer(win, dtype=np.uint8)
    status, outs, consumed = enc.compress_and_flush([src[c:] for c in cuts], tgl.CAP, write_token=False)
    for k, c in enumerate(cuts):
        out1, lz, _, _ = s["firsts"][c]
        where = f"{s['name']}: {tgl.describe(s['marks'], c)}, {show(lz)}"
        assert (int(status[k]), int(consumed[k])) == (0, len(src) - c), where
        assert out1 + outs[k] == s["whole"], (where, "first piece + resume kernel")


# ---------------------------------------------------------------------------------------------------------------------
# 3: three pieces
# ---------------------------------------------------------------------------------------------------------------------
@sweeps
@pytest.mark.parametrize("middle", [1, 17])
def test_three_pieces(pieces, window, extended, middle):
    """src[:c], src[c:c+m], src[c+m:]: a middle byte that cannot fill the ring runs no poll and hands the cached match on as it
    came; 17 bytes run the poll that uses it."""
    s = pieces.sweep(window, extended)
    src, whole = s["src"], s["whole"]
    for c in s["near"]:
        first = s["firsts"][c]
        out1, lz1, win1, wp1 = first
        win, wp, lz = pieces.copies(window, first)
        mid = src[c : c + middle]
        where = f"{s['name']}: {tgl.describe(s['marks'], c)}, middle piece of {len(mid)} on {show(lz1)}"
        res, out2 = pieces.piece(pieces.conf(window, 8, extended), win, wp, lz, mid, first=False, resume=True, finish=False)
        assert res == 0, (where, f"returned {res}")
        assert out1 + out2 == whole[: len(out1) + len(out2)], (where, "bytes of the middle piece")
        if lz1.carry.tail_len + len(mid) < 16:  # the ring does not fill: no poll (compressor.c:700-720)
            assert out2 == b"" and (lz.cached_pos, lz.cached_len) == (lz1.cached_pos, lz1.cached_len), (where, f"-> {show(lz)}")
            assert bytes(lz.carry.tail[: lz.carry.tail_len]) == bytes(lz1.carry.tail[: lz1.carry.tail_len]) + mid, (where, f"-> {show(lz)}")
            assert wp.value == wp1 and C.string_at(win, 1 << window) == win1, (where, "window changed without a poll")
        res, out3 = pieces.piece(pieces.conf(window, 8, extended), win, wp, lz, src[c + middle :], first=False, resume=True, finish=True)
        assert res == 0, (where, f"finishing piece returned {res}")
        assert out1 + out2 + out3 == whole, (where, "three pieces")


# ---------------------------------------------------------------------------------------------------------------------
# 4: every decision cell
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,literal,extended", tgl.CONFIGS, ids=[tgl.config_id(*c) for c in tgl.CONFIGS])
def test_every_decision_cell(pieces, oracle, golden, window, literal, extended):
    """Every case of the configuration cut so that the deciding poll is the first piece's last one (decision position + 16), and
    one byte to either side: the joined bytes are the case's.  Cases without a dictionary, and one with (a fresh first piece from
    the custom dictionary, then a resumed one).  The excess-bits cells: the call that contains the offending poll -- the first
    piece when 16 bytes from the offending one on are in it, else the finishing one -- returns TAMP_EXCESS_BITS."""
    every = li.cases(window, literal, extended)
    with_dict = [c for c in every if c.dictionary is not None and c.status == 0]
    chosen = [c for c in every if c.dictionary is None or c.status != 0] + with_dict[:1]
    assert chosen and (not with_dict or chosen[-1].dictionary is not None)
    t0, calls, excess = time.perf_counter(), 0, 0
    for case in chosen:
        rc, blob = tgl.want(oracle, golden, case)
        assert rc == case.status
        custom = case.dictionary is not None
        for cut in sorted({min(max(case.at + 16 + d, 0), len(case.data)) for d in (-1, 0, 1)}):
            where = (tgl.config_id(window, literal, extended), case.name, case.cell, f"decision at {case.at}, cut at {cut} of {len(case.data)}")
            conf = pieces.conf(window, literal, extended, custom=custom)
            win, wp, lz = pieces.fresh(window, case.dictionary)
            res1, out1 = pieces.piece(conf, win, wp, lz, case.data[:cut], first=True, resume=False, finish=False)
            calls += 1
            if rc == EXCESS_BITS:
                bad = next(k for k, b in enumerate(case.data) if b >> literal)
                assert res1 == (EXCESS_BITS if bad + 16 <= cut else 0), (*where, f"offending byte at {bad}: first piece returned {res1}")
                if res1 == 0:
                    res2, _ = pieces.piece(conf, win, wp, lz, case.data[cut:], first=False, resume=True, finish=True)
                    calls += 1
                    assert res2 == EXCESS_BITS, (*where, f"offending byte at {bad}: finishing piece returned {res2}")
                excess += 1
                continue
            assert res1 == 0, (*where, f"first piece returned {res1}")
            res2, out2 = pieces.piece(conf, win, wp, lz, case.data[cut:], first=False, resume=True, finish=True)
            calls += 1
            assert res2 == 0, (*where, f"finishing piece returned {res2} after {show(lz)}")
            assert out1 + out2 == blob, (*where, "joined bytes")
    if literal == 7 and li.oracle_min_pattern(window, literal) == 2:
        assert excess >= 2
    print(f"lazy pieces {tgl.config_id(window, literal, extended)}: {len(chosen)} cases, {calls} piece calls, {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------------------------------
# 5: output room
# ---------------------------------------------------------------------------------------------------------------------
@sweeps
def test_unfinished_piece_without_room_leaves_the_cached_match(pieces, window, extended):
    """At a cut that holds a cached match, a second unfinished piece with one byte less room than it needs: TAMP_OUTPUT_FULL, no
    byte written, window, window_pos and the 32 bytes of the carry as they came; with exact room it completes."""
    s = pieces.sweep(window, extended)
    src, whole, W = s["src"], s["whole"], 1 << window
    c = next(c for c in s["held"] if c + 200 <= len(src))
    first = s["firsts"][c]
    out1, lz1, win1, wp1 = first
    where = f"{s['name']}: {tgl.describe(s['marks'], c)}, {show(lz1)}"
    conf = pieces.conf(window, 8, extended)
    mid = src[c : c + 200]
    win, wp, lz = pieces.copies(window, first)
    res, ample = pieces.piece(conf, win, wp, lz, mid, first=False, resume=True, finish=False)
    assert res == 0 and len(ample) >= 2, (where, res, len(ample))
    win, wp, lz = pieces.copies(window, first)
    res, out = pieces.piece(conf, win, wp, lz, mid, first=False, resume=True, finish=False, cap=len(ample) - 1)
    assert (res, out) == (OUTPUT_FULL, b""), (where, f"one byte short: {res}, {len(out)} bytes")
    assert bytes(lz) == bytes(lz1) and lz.cached_len, (where, f"-> {show(lz)}")
    assert wp.value == wp1 and C.string_at(win, W) == win1, (where, "window changed")
    res, out2 = pieces.piece(conf, win, wp, lz, mid, first=False, resume=True, finish=False, cap=len(ample))
    assert res == 0 and out2 == ample, (where, f"exact room: {res}")
    res, out3 = pieces.piece(conf, win, wp, lz, src[c + 200 :], first=False, resume=True, finish=True)
    assert res == 0 and out1 + out2 + out3 == whole, (where, "after the refused piece")


# ---------------------------------------------------------------------------------------------------------------------
# 6: refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_of_a_cached_match(pieces):
    """A carry with cached_len != 0 is TAMP_AMD_BAD_ARGUMENT, and nothing is written or changed, with a configuration without lazy
    matching, with resume = 0, beside a pending run, beyond the window's end and when it is longer than the tail."""
    from tamp_amd import _lib

    window, extended = 10, True
    s = pieces.sweep(window, extended)
    W = 1 << window
    c = s["held"][0]
    first = s["firsts"][c]
    _, lz1, win1, wp1 = first
    assert 0 < lz1.cached_len <= lz1.carry.tail_len
    rest = s["src"][c:]

    def attempt(what, *, lazy=True, resume=True, change=None, finish=False):
        win, wp, lz = pieces.copies(window, first)
        if change:
            change(lz)
        before = bytes(lz)
        res, out = pieces.piece(pieces.conf(window, 8, extended, lazy=lazy), win, wp, lz, rest, first=False, resume=resume, finish=finish)
        assert (res, out) == (_lib.BAD_ARGUMENT, b""), (what, res, len(out))
        assert bytes(lz) == before and wp.value == wp1 and C.string_at(win, W) == win1, (what, "something changed")

    for finish in (False, True):
        attempt("a configuration without lazy matching", lazy=False, finish=finish)
        attempt("resume = 0", resume=False, finish=finish)
        attempt("rle_count = 1", change=lambda lz: setattr(lz.carry, "rle_count", 1), finish=finish)
        attempt("cached_pos + cached_len > W", change=lambda lz: setattr(lz, "cached_pos", W - lz.cached_len + 1), finish=finish)
        attempt("cached_len > tail_len", change=lambda lz: setattr(lz.carry, "tail_len", lz.cached_len - 1), finish=finish)
    # (the carry as it came is served)
    win, wp, lz = pieces.copies(window, first)
    res, out = pieces.piece(pieces.conf(window, 8, extended), win, wp, lz, rest, first=False, resume=True, finish=True)
    assert res == 0 and first[0] + out == s["whole"]


# ---------------------------------------------------------------------------------------------------------------------
# 7: Compressor, per-call counts against live reference objects
# ---------------------------------------------------------------------------------------------------------------------
def test_lazy_compressor_write_streams_like_the_reference_object(ta, oracle):
    """tests/test_gpu_round3.py::test_compressor_write_streams_like_the_reference_object with lazy_matching=True on both sides:
    every write handed over as a piece (PIECE_MIN = 1), the bytes the reference object's, the counts the reference's up to the
    bits its object holds back until the next poll (0..4 bytes at a write, equal at every flush point).  Then the default
    thresholds: a large write leaves during the call."""
    from oracle.checker import Ref
    from tamp_amd import workloads as wl

    if not Ref.available():
        pytest.skip("oracle/_ref (the reference C built in place) is the only checker with object-level calls")
    ref = Ref()
    rng = np.random.default_rng(611)
    prose = wl.real_text("prose", frozen_only=True)
    assert len(prose) >= 300_000
    old_min = ta.Compressor.PIECE_MIN
    ta.Compressor.PIECE_MIN = 1
    try:
        for ext in (True, False):
            for si, src in enumerate((li.sweep_source(10, ext)[0], prose[:20_000])):
                for trial in range(2):
                    ops, pos = [], 0
                    while pos < len(src):
                        k = int(rng.choice([1, 3, 15, 16, 17, 40, 300, 5000]))
                        ops.append(("write", src[pos : pos + k]))
                        pos += k
                        if rng.random() < 0.08:
                            ops.append(("flush", bool(rng.integers(0, 2))))
                    ops.append(("close",))
                    want_counts = []
                    rc, want = ref.stream_script(ops, window=10, literal=8, extended=ext, lazy_matching=True, counts=want_counts)
                    assert rc == 0
                    f = io.BytesIO()
                    c = ta.Compressor(f, window=10, literal=8, extended=ext, lazy_matching=True)
                    got_counts = []
                    for op in ops:
                        if op[0] == "write":
                            got_counts.append(c.write(op[1]))
                        elif op[0] == "flush":
                            got_counts.append(c.flush(op[1]))
                        else:
                            got_counts.append(c.close())
                    assert f.getvalue() == want, (si, ext, trial)
                    gc, wc = np.cumsum(got_counts), np.cumsum(want_counts)
                    for k, op in enumerate(ops):
                        if op[0] == "write":
                            assert 0 <= gc[k] - wc[k] <= 4, (si, ext, trial, k, got_counts[k], want_counts[k])
                        else:
                            assert gc[k] == wc[k], (si, ext, trial, k)
    finally:
        ta.Compressor.PIECE_MIN = old_min
    # the default thresholds: a large write leaves in bounded pieces during the call, and nothing of it waits for the flush
    rc, want = oracle.compress(prose[:300_000], window=10, literal=8, extended=True, lazy_matching=True)
    assert rc == 0
    f = io.BytesIO()
    c = ta.Compressor(f, lazy_matching=True)
    n1 = c.write(prose[:300_000])
    assert n1 > 0 and len(f.getvalue()) == n1 and len(c._pending) == 0
    n2 = c.close()
    assert f.getvalue() == want and n1 + n2 == len(want)


# ---------------------------------------------------------------------------------------------------------------------
# 8: reference-named objects
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", [True, False], ids=["ext", "v1"])
def test_reference_named_lazy_object_takes_the_piece_path(ta, extended):
    """tamp_compressor_init(lazy_matching = 1), two tamp_compressor_compress calls of 70,000 bytes (the piece path from 64 KiB on),
    tamp_compressor_flush: bytes and per-call (status, written, consumed) against the reference object -- a piece hands whole
    bytes over up to four bytes earlier, equal again at the flush -- and the object's cached match after the first call is the
    resume kernel's for the same call."""
    from oracle.checker import Ref
    from tamp_amd import _lib
    from tamp_amd import workloads as wl

    if not Ref.available():
        pytest.skip("needs oracle/_ref")
    ref = Ref()
    lib = _lib.load()

    class TampConf(C.Structure):
        _fields_ = [("window", C.c_uint16, 4), ("literal", C.c_uint16, 4), ("use_custom_dictionary", C.c_uint16, 1),
                    ("extended", C.c_uint16, 1), ("dictionary_reset", C.c_uint16, 1), ("append", C.c_uint16, 1),
                    ("lazy_matching", C.c_uint16, 1)]

    sz = C.POINTER(C.c_size_t)
    lib.tamp_compressor_init.restype = C.c_int8
    lib.tamp_compressor_init.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tamp_compressor_compress.restype = C.c_int8
    lib.tamp_compressor_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, sz, C.c_void_p, C.c_size_t, sz]
    lib.tamp_compressor_flush.restype = C.c_int8
    lib.tamp_compressor_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, sz, C.c_bool]
    prose = wl.real_text("prose", frozen_only=True)
    parts = [prose[100_000:170_000], prose[170_000:240_000]]
    cap = 2 * 70_000 + 4096
    rc, want = ref.encode_script([("compress", parts[0], cap), ("compress", parts[1], cap), ("flush", False, cap)], window=10, literal=8,
                                 extended=extended, lazy_matching=True)
    assert rc == 0 and [w[0] for w in want] == [0, 0, 0]
    conf = TampConf(window=10, literal=8, extended=int(extended), lazy_matching=1)
    window, comp = (C.c_ubyte * 1024)(), (C.c_ubyte * 48)()
    assert lib.tamp_compressor_init(comp, C.byref(conf), window) == 0
    got, after_first = [], None
    for part in parts:
        out, buf = (C.c_ubyte * cap)(), (C.c_ubyte * len(part)).from_buffer_copy(part)
        w, k = C.c_size_t(0), C.c_size_t(0)
        res = lib.tamp_compressor_compress(comp, out, cap, C.byref(w), buf, len(part), C.byref(k))
        got.append((res, bytes(out[: w.value]), k.value))
        if after_first is None:
            after_first = EncoderState.from_buffer_copy(bytes(comp)[8:48])
    out, w = (C.c_ubyte * 64)(), C.c_size_t(0)
    res = lib.tamp_compressor_flush(comp, out, 64, C.byref(w), False)
    got.append((res, bytes(out[: w.value]), 0))
    assert b"".join(g[1] for g in got) == b"".join(w[1] for w in want)
    gc, wc = np.cumsum([len(g[1]) for g in got]), np.cumsum([len(w[1]) for w in want])
    for k in range(2):
        assert (got[k][0], got[k][2]) == (want[k][0], want[k][2]), (k, got[k][0], got[k][2])
        assert 0 <= gc[k] - wc[k] <= 4, (k, int(gc[k]), int(wc[k]))
    assert got[2][0] == 0 and gc[2] == wc[2]
    enc = ta.EncoderBatch(1, window=10, literal=8, extended=extended, lazy_matching=True)
    st, outs, used = enc.compress([parts[0]], cap)
    assert (int(st[0]), outs[0], int(used[0])) == want[0]  # (the resume kernel's call is the reference's)
    obj = EncoderState.from_buffer_copy(enc.states[0, :STATE_BYTES].tobytes())
    assert after_first.cached_match_index == obj.cached_match_index, (after_first.cached_match_index, obj.cached_match_index)
    if obj.cached_match_index >= 0:
        assert after_first.cached_match_size == obj.cached_match_size
    assert _ring(after_first) == _ring(obj) and after_first.window_pos == obj.window_pos
