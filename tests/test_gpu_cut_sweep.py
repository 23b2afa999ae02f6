"""GPU tier of the cut sweep: one 1.4 KB stream (tests/cut_sweep_input.py) cut at EVERY byte on each code path that
carries compressor or decoder state from one call to the next.  All `-m gpu`, everything bit-exact.

Between two flush points the bytes of a stream do not depend on how its input was cut into calls, so every cut has the
same known answer, `whole` = the oracle's one-shot stream (pinned to the reference object by
tests/test_cut_sweep_golden.py), and the reference object's per-call results for every cut are the fixture
tests/golden/cut_sweep.json.  Routes, per configuration (window 2^10 / 2^8 in both formats, 2^15 extended):

  A   token-level resume kernel (tamp_batch_compress_resume, EncoderBatch): all cuts in one launch per step
  B   piece path of the batch kernel (tamp_amd_compress_piece through the C ABI): two calls per cut, and the carry
      after the first against A's object state (the mapping the reference-named objects' hand-over relies on)
  C   hand-over both ways: A's state finished by one piece call, B's carry finished by the resume kernel
  D   three pieces, the middle one 1 or 17 bytes
  E   decoder objects (tamp_batch_decompress_resume, DecoderBatch): input cut at every byte, room cut at every byte
  F   the guard that pieces are not offered with lazy matching

A failing assertion names the configuration, the cut and the oracle token the cut falls into.  Each route prints the
cuts and calls it ran and the time it took (pytest -s).
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

import cut_sweep_input as cs  # noqa: E402

IDS = [cs.case_id(w, e) for w, e in cs.CONFIGS]
sweep_configs = pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=IDS)


class EncoderState(C.Structure):
    """include/tamp_amd.h TampAmdEncoderState (the window follows at byte 40 of an object)."""
    _fields_ = [("bit_buffer", C.c_uint32), ("window_pos", C.c_uint16), ("bit_buffer_pos", C.c_uint8),
                ("input_size", C.c_uint8), ("input_pos", C.c_uint8), ("window", C.c_uint8), ("literal", C.c_uint8),
                ("flags", C.c_uint8), ("input", C.c_uint8 * 16), ("cached_match_index", C.c_int16),
                ("extended_match_position", C.c_uint16), ("cached_match_size", C.c_uint8), ("rle_count", C.c_uint8),
                ("extended_match_count", C.c_uint8), ("last_was_flush", C.c_uint8), ("reserved", C.c_uint32)]


STATE_BYTES = 40
assert C.sizeof(EncoderState) == STATE_BYTES


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


def _ring(st: EncoderState) -> bytes:
    """The unparsed bytes of an object's 16-byte ring, oldest first."""
    return bytes(st.input[(st.input_pos + k) & 15] for k in range(st.input_size))


class Sweep:
    """Per configuration: the input, the oracle's stream and token trace, and the results of routes A and B, which the
    later routes start from (each computed once, whichever test asks first)."""

    def __init__(self, ta, oracle):
        from tamp_amd import _lib

        self.ta, self.oracle, self._lib, self.lib = ta, oracle, _lib, _lib.load()
        self.golden = {(r["window"], r["extended"]): r for r in load_golden("cut_sweep.json")}
        self._case, self._a, self._b = {}, {}, {}

    # ---- input and expectations ----
    def case(self, window, extended):
        key = (window, extended)
        if key not in self._case:
            src = cs.source(window)
            tokens, whole = cs.token_trace(self.oracle, src, window, extended)
            name = cs.case_id(window, extended)
            self._case[key] = (src, tokens, whole, lambda c, what="": f"{name}: {cs.describe_cut(tokens, c)}{': ' if what else ''}{what}")
        return self._case[key]

    def conf(self, window, extended, lazy=False):
        return self._lib.TampAmdConf(window, cs.LITERAL, 0, int(extended), 0, int(lazy))

    # ---- one piece call through the C ABI (as tamp_amd/codec.py does) ----
    def piece(self, conf, window_buf, wp, carry, data, *, first, resume, finish):
        n = len(data)
        cap = self.lib.tamp_amd_compress_bound(n + 272, cs.LITERAL, 0) + 8
        out = (C.c_ubyte * cap)()
        written, token = C.c_size_t(0), C.c_int(0)
        src = (C.c_ubyte * max(n, 1)).from_buffer_copy(data if n else b"\0")
        res = self.lib.tamp_amd_compress_piece(C.byref(conf), int(first), 0, int(resume), int(finish), 0, window_buf,
                                               C.byref(wp), C.byref(carry), out, cap, C.byref(written), src, n,
                                               C.byref(token), 0)
        assert written.value <= cap
        return res, C.string_at(out, written.value)

    def carry_ok(self, carry) -> bool:
        """include/tamp_amd.h TampAmdCarry, what a piece leaves behind.  The ring holds 15 bytes at most unless the call's
        last poll took none of its 16 (tamp_compressor_compress returns with a full ring where a run or an extended match
        that could not grow emitted its token on the ring that took the call's last byte, compressor.c:449-466,505-509,
        700-720) -- and then nothing is growing any more.  Route B holds every carry against the reference-pinned object
        of route A, so a full ring passes only where the reference object's ring is full."""
        if carry.tail_len == 16 and (carry.rle_count or carry.ext_count):
            return False
        return (carry.bit_count <= 7 and carry.tail_len <= 16 and not (carry.rle_count and carry.ext_count)
                and carry.reserved == 0)

    def show(self, carry) -> str:
        return (f"carry(rle={carry.rle_count} ext={carry.ext_count}@{carry.ext_pos} bits={carry.bit_count}:{carry.bits:#010x} "
                f"tail={bytes(carry.tail[: min(carry.tail_len, 16)])!r} reserved={carry.reserved})")

    # ---- route A: resume kernel, every cut one object ----
    def route_a(self, window, extended):
        key = (window, extended)
        if key not in self._a:
            src, _, _, _ = self.case(window, extended)
            n = len(src)
            t0 = time.perf_counter()
            enc = self.ta.EncoderBatch(n + 1, window=window, literal=cs.LITERAL, extended=extended)
            st1, out1, k1 = enc.compress([src[:c] for c in range(n + 1)], cs.CAP)
            states1 = enc.states.copy()
            st2, out2, k2 = enc.compress_and_flush([src[c:] for c in range(n + 1)], cs.CAP, write_token=False)
            print(f"cut-sweep {cs.case_id(window, extended)} route A: {n + 1} cuts, 2 launches, {time.perf_counter() - t0:.2f} s")
            self._a[key] = dict(states1=states1, call1=(st1, out1, k1), call2=(st2, out2, k2))
        return self._a[key]

    def state_of(self, window, extended, c) -> EncoderState:
        return EncoderState.from_buffer_copy(self.route_a(window, extended)["states1"][c, :STATE_BYTES].tobytes())

    # ---- route B: first piece of every cut (carry, window, bytes); the second piece is the test's ----
    def route_b(self, window, extended):
        key = (window, extended)
        if key not in self._b:
            src, _, _, where = self.case(window, extended)
            W = 1 << window
            t0 = time.perf_counter()
            firsts = []
            for c in range(len(src) + 1):
                win, wp, carry = (C.c_ubyte * W)(), C.c_uint16(0), self._lib.TampAmdCarry()
                res, out1 = self.piece(self.conf(window, extended), win, wp, carry, src[:c], first=True, resume=False, finish=False)
                assert res == 0, where(c, f"first piece returned {res}")
                firsts.append((out1, self._lib.TampAmdCarry.from_buffer_copy(carry), C.string_at(win, W), wp.value))
            print(f"cut-sweep {cs.case_id(window, extended)} route B, first pieces: {len(firsts)} cuts, {len(firsts)} piece calls, "
                  f"{time.perf_counter() - t0:.2f} s")
            self._b[key] = firsts
        return self._b[key]

    def resume_from(self, window, first):
        """Fresh copies of what a first piece left: (window buffer, window_pos, carry)."""
        _, carry, win, wp = first
        W = 1 << window
        return (C.c_ubyte * W).from_buffer_copy(win), C.c_uint16(wp), self._lib.TampAmdCarry.from_buffer_copy(carry)


@pytest.fixture(scope="module")
def sweep(ta, oracle):
    return Sweep(ta, oracle)


@sweep_configs
def test_a_resume_kernel_every_cut_in_one_launch(sweep, window, extended):
    """A: object c compresses src[:c], then compresses src[c:] and flushes: per call and per object the reference object's
    (status, bytes written, consumed) of the fixture, and the bytes are the corresponding slice of the one-shot stream."""
    src, _, whole, where = sweep.case(window, extended)
    rec = sweep.golden[(window, extended)]
    assert rec["input_len"] == len(src) and len(rec["cuts"]) == len(src) + 1 and rec["whole_len"] == len(whole)
    a = sweep.route_a(window, extended)
    (st1, out1, k1), (st2, out2, k2) = a["call1"], a["call2"]
    for c, (ws1, wl1, wk1, ws2, wl2, wk2) in enumerate(rec["cuts"]):
        assert (int(st1[c]), len(out1[c]), int(k1[c])) == (ws1, wl1, wk1), where(c, "first call")
        assert out1[c] == whole[:wl1], where(c, "bytes of the first call")
        assert (int(st2[c]), len(out2[c]), int(k2[c])) == (ws2, wl2, wk2), where(c, "second call")
        assert out2[c] == whole[wl1:], where(c, "bytes of the second call")


@sweep_configs
def test_b_piece_path_every_cut_and_its_carry(sweep, window, extended):
    """B: src[:c] as an unfinished piece on a fresh window, src[c:] as the finishing one: the two outputs are the one-shot
    stream, and what the first piece leaves behind (include/tamp_amd.h:424-434) is, field by field, what object c of route A
    holds after its first call -- run, extended match, ring, window, window position, pending bits (the object keeps whole
    bytes of its last token back that the piece has already delivered)."""
    src, _, whole, where = sweep.case(window, extended)
    W = 1 << window
    firsts = sweep.route_b(window, extended)
    a = sweep.route_a(window, extended)
    len1_a = [len(o) for o in a["call1"][1]]
    t0 = time.perf_counter()
    full_rings = 0
    for c, first in enumerate(firsts):
        out1, carry, win, wp = first
        assert sweep.carry_ok(carry), where(c, sweep.show(carry))
        st = sweep.state_of(window, extended, c)
        assert carry.rle_count == st.rle_count, where(c, f"{sweep.show(carry)} vs object rle_count {st.rle_count}")
        assert carry.ext_count == st.extended_match_count, where(c, f"{sweep.show(carry)} vs object count {st.extended_match_count}")
        if carry.ext_count:
            assert carry.ext_pos == st.extended_match_position, where(c, f"{sweep.show(carry)} vs object position {st.extended_match_position}")
        assert bytes(carry.tail[: carry.tail_len]) == _ring(st), where(c, f"{sweep.show(carry)} vs object ring {_ring(st)!r}")
        full_rings += carry.tail_len == 16
        assert wp == st.window_pos, where(c, f"window_pos {wp} vs object {st.window_pos}")
        assert win == a["states1"][c, STATE_BYTES : STATE_BYTES + W].tobytes(), where(c, "window bytes")
        # pending bits: as many bits have been produced either way; the piece's < 8 are the object's last ones
        assert 8 * len(out1) + carry.bit_count == 8 * len1_a[c] + st.bit_buffer_pos, \
            where(c, f"{len(out1)} bytes + {carry.bit_count} bits vs object {len1_a[c]} bytes + {st.bit_buffer_pos} bits")
        assert out1 == whole[: len(out1)], where(c, "bytes of the first piece")
        if carry.bit_count:
            assert carry.bit_count <= st.bit_buffer_pos
            pending = (st.bit_buffer >> (32 - st.bit_buffer_pos)) & ((1 << carry.bit_count) - 1)
            assert carry.bits >> (32 - carry.bit_count) == pending, where(c, f"{sweep.show(carry)} vs object bits {st.bit_buffer:#010x}/{st.bit_buffer_pos}")
        if carry.tail_len == 16:  # a call without input polls nothing, full ring or not (compressor.c:700)
            win0, wp0, carry0 = sweep.resume_from(window, first)
            res, out0 = sweep.piece(sweep.conf(window, extended), win0, wp0, carry0, b"", first=False, resume=True, finish=False)
            assert (res, out0) == (0, b""), where(c, f"an empty piece on a full ring returned {res} and {out0!r}")
            assert bytes(carry0) == bytes(carry) and wp0.value == wp and C.string_at(win0, W) == win, \
                where(c, f"an empty piece on a full ring: {sweep.show(carry)} -> {sweep.show(carry0)}")
        win2, wp2, carry2 = sweep.resume_from(window, first)
        res, out2 = sweep.piece(sweep.conf(window, extended), win2, wp2, carry2, src[c:], first=False, resume=True, finish=True)
        assert res == 0, where(c, f"finishing piece returned {res}")
        assert out1 + out2 == whole, where(c, "first piece + finishing piece")
    if not extended:
        assert full_rings == 0  # (every v1 poll takes a byte)
    print(f"cut-sweep {cs.case_id(window, extended)} route B, finishing pieces and carries: {len(firsts)} cuts, {len(firsts)} piece calls, "
          f"{full_rings} calls ended on a full ring, {time.perf_counter() - t0:.2f} s")


@sweep_configs
def test_c_resume_kernel_state_finished_by_a_piece(sweep, window, extended):
    """C, resume to piece: object c of route A after its first call, turned into a carry the way the reference-named objects
    do it (bit_count is the object's bit_buffer_pos: up to 31 on entry), finished by ONE piece call."""
    from tamp_amd import _lib

    src, _, whole, where = sweep.case(window, extended)
    W = 1 << window
    a = sweep.route_a(window, extended)
    out1_a = a["call1"][1]
    t0 = time.perf_counter()
    most_bits = 0
    for c in range(len(src) + 1):
        st = sweep.state_of(window, extended, c)
        carry = _lib.TampAmdCarry()
        carry.rle_count, carry.ext_count, carry.ext_pos = st.rle_count, st.extended_match_count, st.extended_match_position
        carry.bit_count, carry.bits = st.bit_buffer_pos, st.bit_buffer
        carry.tail_len = st.input_size
        for k, byte in enumerate(_ring(st)):
            carry.tail[k] = byte
        assert carry.bit_count <= 31 and carry.tail_len <= 16, where(c, sweep.show(carry))
        most_bits = max(most_bits, carry.bit_count)
        win = (C.c_ubyte * W).from_buffer_copy(a["states1"][c, STATE_BYTES : STATE_BYTES + W].tobytes())
        wp = C.c_uint16(st.window_pos)
        res, out = sweep.piece(sweep.conf(window, extended), win, wp, carry, src[c:], first=False, resume=True, finish=True)
        assert res == 0, where(c, f"finishing piece returned {res}")
        assert out1_a[c] + out == whole, where(c, f"object bytes + finishing piece, entered with {st.bit_buffer_pos} pending bits")
    assert most_bits >= 8, "no object sat on a whole byte of its last token: the entry with 8..31 pending bits was not reached"
    print(f"cut-sweep {cs.case_id(window, extended)} route C, resume to piece: {len(src) + 1} cuts, {len(src) + 1} piece calls, "
          f"most pending bits on entry {most_bits}, {time.perf_counter() - t0:.2f} s")


@sweep_configs
def test_c_piece_carry_finished_by_the_resume_kernel(sweep, window, extended):
    """C, piece to resume: what the first piece of route B left, written into encoder objects the way the reference-named
    objects take a piece's carry back, all cuts finished in ONE compress_and_flush launch of the resume kernel."""
    src, _, whole, where = sweep.case(window, extended)
    W, n = 1 << window, len(src)
    firsts = sweep.route_b(window, extended)
    t0 = time.perf_counter()
    enc = sweep.ta.EncoderBatch(n + 1, window=window, literal=cs.LITERAL, extended=extended)
    for c, (_, carry, win, wp) in enumerate(firsts):
        st = EncoderState.from_buffer_copy(enc.states[c, :STATE_BYTES].tobytes())  # (conf fields as initialised)
        st.window_pos = wp
        st.rle_count, st.extended_match_count, st.extended_match_position = carry.rle_count, carry.ext_count, carry.ext_pos
        st.bit_buffer_pos, st.bit_buffer = carry.bit_count, (carry.bits if carry.bit_count else 0)
        st.input_pos, st.input_size = 0, carry.tail_len
        for k in range(16):
            st.input[k] = carry.tail[k] if k < carry.tail_len else 0
        st.last_was_flush = 0
        enc.states[c, :STATE_BYTES] = np.frombuffer(bytes(st), dtype=np.uint8)
        enc.states[c, STATE_BYTES : STATE_BYTES + W] = np.frombuffer(win, dtype=np.uint8)
    status, outs, consumed = enc.compress_and_flush([src[c:] for c in range(n + 1)], cs.CAP, write_token=False)
    for c, (out1, carry, _, _) in enumerate(firsts):
        assert (int(status[c]), int(consumed[c])) == (0, n - c), where(c, sweep.show(carry))
        assert out1 + outs[c] == whole, where(c, f"first piece + resume kernel from {sweep.show(carry)}")
    print(f"cut-sweep {cs.case_id(window, extended)} route C, piece to resume: {n + 1} cuts, 1 launch, {time.perf_counter() - t0:.2f} s")


@sweep_configs
@pytest.mark.parametrize("middle", [1, 17])
def test_d_three_pieces(sweep, window, extended, middle):
    """D: src[:c], src[c:c+m], src[c+m:] as pieces (the first is route B's first piece: same call, same arguments).  The
    carry after the middle piece obeys the same rules; a middle byte that cannot fill the 16-byte ring runs no parse step:
    no bytes leave and the carry has only grown by that byte."""
    src, _, whole, where = sweep.case(window, extended)
    firsts = sweep.route_b(window, extended)
    t0 = time.perf_counter()
    idle = 0
    for c, first in enumerate(firsts):
        out1, carry1, win1, wp1 = first
        win, wp, carry = sweep.resume_from(window, first)
        mid = src[c : c + middle]
        res, out2 = sweep.piece(sweep.conf(window, extended), win, wp, carry, mid, first=False, resume=True, finish=False)
        assert res == 0, where(c, f"middle piece of {len(mid)} returned {res}")
        assert sweep.carry_ok(carry), where(c, f"after a middle piece of {len(mid)}: {sweep.show(carry)}")
        assert out1 + out2 == whole[: len(out1) + len(out2)], where(c, f"bytes of the middle piece of {len(mid)}")
        if carry1.tail_len + len(mid) < 16:  # the ring does not fill: no poll (compressor.c:700-720)
            idle += 1
            assert out2 == b"", where(c, f"a middle piece of {len(mid)} on {sweep.show(carry1)} wrote {out2!r}")
            assert bytes(carry.tail[: carry.tail_len]) == bytes(carry1.tail[: carry1.tail_len]) + mid, \
                where(c, f"{sweep.show(carry1)} + {mid!r} -> {sweep.show(carry)}")
            assert (carry.rle_count, carry.ext_count, carry.bit_count) == (carry1.rle_count, carry1.ext_count, carry1.bit_count), \
                where(c, f"{sweep.show(carry1)} -> {sweep.show(carry)}")
            if carry.ext_count:
                assert carry.ext_pos == carry1.ext_pos, where(c, f"{sweep.show(carry1)} -> {sweep.show(carry)}")
            if carry.bit_count:
                assert carry.bits >> (32 - carry.bit_count) == carry1.bits >> (32 - carry.bit_count), \
                    where(c, f"{sweep.show(carry1)} -> {sweep.show(carry)}")
            assert wp.value == wp1 and C.string_at(win, 1 << window) == win1, where(c, "window changed without a parse step")
        res, out3 = sweep.piece(sweep.conf(window, extended), win, wp, carry, src[c + middle :], first=False, resume=True, finish=True)
        assert res == 0, where(c, f"finishing piece returned {res}")
        assert out1 + out2 + out3 == whole, where(c, f"three pieces, the middle one {len(mid)} bytes")
    if middle == 1:
        assert idle >= len(firsts) // 2  # (15 of 16 ring fills cannot be completed by one byte)
    print(f"cut-sweep {cs.case_id(window, extended)} route D, middle {middle}: {len(firsts)} cuts, {2 * len(firsts)} piece calls, "
          f"{idle} middle pieces without a parse step, {time.perf_counter() - t0:.2f} s")


def _decode_sweep(sweep, window, blob, scripts, where):
    """One decoder object per script [(take, cap), (take, cap)], advanced in one launch per step; every call against the
    oracle's resumable decoder on the same script.  -> the outputs of each object joined."""
    batch = sweep.ta.DecoderBatch(len(scripts), window_bits=window)
    pos = [0] * len(scripts)
    got = [[] for _ in scripts]
    for step in range(2):
        chunks = [blob[pos[i] : pos[i] + s[step][0]] for i, s in enumerate(scripts)]
        caps = np.array([s[step][1] for s in scripts], dtype=np.uint32)
        status, outs, consumed = batch.step(chunks, caps)
        for i in range(len(scripts)):
            got[i].append((int(status[i]), outs[i], int(consumed[i])))
            pos[i] += int(consumed[i])
    joined = []
    for i, script in enumerate(scripts):
        r0, want = sweep.oracle.decode_script(blob, script, window_bits=window)
        assert r0 == 0
        for k in range(2):
            assert got[i][k] == want[k], where(i, k, got[i][k], want[k])
        joined.append(b"".join(o for _, o, _ in got[i]))
    return joined


@sweep_configs
def test_e_decoder_objects_input_cut_at_every_byte(sweep, window, extended):
    """E: decoder object c is offered blob[:c], then everything it has not consumed, with ample room: status, bytes and
    consumed count of both calls as the oracle's resumable decoder returns them; together the input of the sweep."""
    src, _, whole, _ = sweep.case(window, extended)
    room = len(src) + 64
    t0 = time.perf_counter()
    scripts = [[(c, room), (len(whole), room)] for c in range(len(whole) + 1)]
    name = cs.case_id(window, extended)
    joined = _decode_sweep(sweep, window, whole, scripts,
                           lambda c, k, got, want: f"{name}: stream cut at byte {c} of {len(whole)}, call {k + 1}: status/consumed "
                                                   f"{got[0]}/{got[2]} vs {want[0]}/{want[2]}, {len(got[1])} vs {len(want[1])} bytes")
    for c, back in enumerate(joined):
        assert back == src, f"{name}: stream cut at byte {c}: {len(back)} bytes decoded"
    print(f"cut-sweep {name} route E, input cuts: {len(scripts)} cuts, 2 launches, {time.perf_counter() - t0:.2f} s")


@sweep_configs
def test_e_decoder_objects_room_cut_at_every_byte(sweep, window, extended):
    """E: decoder object c is offered the whole stream with room for c bytes, then what it has not consumed with ample
    room."""
    src, tokens, whole, _ = sweep.case(window, extended)
    room = len(src) + 64
    t0 = time.perf_counter()
    scripts = [[(len(whole), c), (len(whole), room)] for c in range(len(src) + 1)]
    name = cs.case_id(window, extended)
    joined = _decode_sweep(sweep, window, whole, scripts,
                           lambda c, k, got, want: f"{name}: room of {c} bytes, {cs.describe_cut(tokens, c)}, call {k + 1}: "
                                                   f"status/consumed {got[0]}/{got[2]} vs {want[0]}/{want[2]}, "
                                                   f"{len(got[1])} vs {len(want[1])} bytes")
    for c, back in enumerate(joined):
        assert back == src, f"{name}: room of {c} bytes, {cs.describe_cut(tokens, c)}: {len(back)} bytes decoded"
    print(f"cut-sweep {name} route E, room cuts: {len(scripts)} cuts, 2 launches, {time.perf_counter() - t0:.2f} s")


def test_f_unfinished_pieces_are_not_offered_with_lazy_matching(sweep):
    """F: the cached match of lazy matching is not carried between pieces, so a piece that does not finish its segment is
    refused (TAMP_AMD_BAD_ARGUMENT) and leaves everything as it was; the finishing call of the same stream is served."""
    from tamp_amd import _lib

    src = cs.source(10)[:300]
    win, wp, carry = (C.c_ubyte * 1024)(), C.c_uint16(0), _lib.TampAmdCarry()
    res, out = sweep.piece(sweep.conf(10, True, lazy=True), win, wp, carry, src, first=True, resume=False, finish=False)
    assert res == _lib.BAD_ARGUMENT and out == b""
    assert wp.value == 0 and bytes(win) == bytes(1024) and bytes(carry) == bytes(C.sizeof(carry))
    res, out = sweep.piece(sweep.conf(10, True, lazy=True), win, wp, carry, src, first=True, resume=False, finish=True)
    rc, want = sweep.oracle.compress(src, window=10, literal=cs.LITERAL, extended=True, lazy_matching=True)
    assert (res, rc) == (0, 0) and out == want
