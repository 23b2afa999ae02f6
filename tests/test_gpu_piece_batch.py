"""GPU tier of the batch piece calls: many streaming compressors advanced per launch (tamp_batch_compress_pieces,
``CompressorBatch``).  All `-m gpu`, every comparison bit-exact.

Two independent yardsticks: the oracle's one-shot stream for whole inputs, and the single-object call for the same arguments
(tamp_amd_compress_piece_lazy, which tests/test_gpu_cut_sweep.py, tests/test_gpu_lazy.py and the piece fuzzers pin to the
reference) for status, bytes and the object a call leaves -- window, window_pos, the 32 carry bytes, token_written (with one
field of no meaning set apart: `state_diff`).

Every batch call of this file runs behind guard bytes: the slabs lie apart in a buffer filled with a pattern, result rows start
from a sentinel, and `Harness.batch` checks after every call that nothing outside the slabs was written (host memory: nothing
behind out_len[i] either) and that a SKIP object, its slab and its rows are as they were.
"""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

import cut_sweep_input as cs  # noqa: E402
import lazy_input as li  # noqa: E402

HEADER, APPEND, RESUME, FINISH, TOKEN, SKIP = 1, 2, 4, 8, 16, 128
OK, OUTPUT_FULL, EXCESS_BITS, BAD_ARGUMENT = 0, 1, -2, -21
MEM_HOST, MEM_DEVICE = 0, 1
HDR = 48          # bytes of an object in front of its window
GUARD = 0xA5      # the pattern of the output buffer
GAP = 24          # guard bytes in front of, between and behind the slabs (not a multiple of 16: slabs at odd alignments)
ROW_OUT_LEN, ROW_STATUS = 0x7E7E7E7E, 0x5A


class Harness:
    def __init__(self):
        import torch

        from tamp_amd import _lib

        self._lib, self.lib, self.torch = _lib, _lib.load(), torch
        self.dev = torch.device("cuda:0")

    def conf(self, window=10, extended=True, *, lazy=False, literal=8, dictionary_reset=False, custom=False):
        return self._lib.TampAmdConf(window, literal, int(custom), int(extended), int(dictionary_reset), int(lazy))

    def room(self, conf, n):
        return int(self.lib.tamp_amd_compress_bound(n + 271, conf.literal, int(conf.dictionary_reset)))

    def fresh(self, conf, n=1, dictionary=None):
        objs = np.zeros((n, HDR + (1 << conf.window)), dtype=np.uint8)
        if dictionary is not None:
            objs[:, HDR:] = np.frombuffer(dictionary, dtype=np.uint8)
        return objs

    # ---- the yardstick: ONE object through the single call, flags from the op ----
    def single(self, conf, obj, op, data, cap=None):
        """-> (status, bytes, the object afterwards); `obj` (uint8[48 + W]) is not changed."""
        W = 1 << conf.window
        data = bytes(data)
        cap = self.room(conf, len(data)) if cap is None else int(cap)
        po = self._lib.TampAmdPieceObject.from_buffer_copy(obj[:HDR].tobytes())
        carry = self._lib.TampAmdLazyCarry.from_buffer_copy(bytes(po.carry))
        win = (C.c_ubyte * W).from_buffer_copy(obj[HDR : HDR + W].tobytes())
        wp, written, token = C.c_uint16(po.window_pos), C.c_size_t(0), C.c_int(0)
        out = (C.c_ubyte * max(cap, 1))()
        src = (C.c_ubyte * max(len(data), 1)).from_buffer_copy(data if data else b"\0")
        res = self.lib.tamp_amd_compress_piece_lazy(C.byref(conf), int(bool(op & HEADER)), int(bool(op & APPEND)), int(bool(op & RESUME)),
                                                    int(bool(op & FINISH)), int(bool(op & TOKEN)), win, C.byref(wp), C.byref(carry), out, cap,
                                                    C.byref(written), src, len(data), C.byref(token), 0)
        assert written.value <= cap
        after = obj.copy()
        if res == OK:
            after[:32] = np.frombuffer(bytes(carry), dtype=np.uint8)
            after[32:34] = np.frombuffer(np.uint16(wp.value).tobytes(), dtype=np.uint8)
            after[34] = token.value
            after[HDR : HDR + W] = np.frombuffer(bytes(win), dtype=np.uint8)
        else:  # (the single call leaves a failed piece's window and carry as they came)
            assert bytes(carry) == obj[:32].tobytes() and bytes(win) == obj[HDR : HDR + W].tobytes() and wp.value == po.window_pos
        return int(res), C.string_at(out, written.value), after

    # ---- the call under test ----
    def batch(self, conf, objs, ops, chunks, caps=None, mem=MEM_DEVICE, claimed_len=None, claimed_off=None):
        """One tamp_batch_compress_pieces call.  -> (status int8[n], out_len uint32[n], [bytes], objects afterwards).  `objs` is
        not changed.  SKIP objects get a pattern in their rows and must come back untouched.  `claimed_len`: {object: in_len the
        table claims for it} -- lengths the call must refuse without reading a byte (the buffer holds `chunks` only); `claimed_off`:
        the same for in_off (host memory only: device pointers beyond the buffer are the caller's to avoid)."""
        torch, n = self.torch, len(ops)
        ops = np.asarray(ops, dtype=np.uint8)
        chunks = [bytes(c) for c in chunks]
        caps = np.array([self.room(conf, len(c)) for c in chunks] if caps is None else caps, dtype=np.uint32)
        in_len = np.array([len(c) for c in chunks], dtype=np.uint32)
        in_off = np.zeros(n, dtype=np.uint64)
        in_off[1:] = np.cumsum(in_len[:-1].astype(np.uint64) + 3)  # (three bytes between the inputs: odd alignments)
        flat = np.full(int(in_off[-1] + in_len[-1]) + 3, 0xEE, dtype=np.uint8)
        for c, o in zip(chunks, in_off):
            flat[int(o) : int(o) + len(c)] = np.frombuffer(c, dtype=np.uint8)
        out_off = np.zeros(n, dtype=np.uint64)
        out_off[0] = GAP
        out_off[1:] = GAP + np.cumsum(caps[:-1].astype(np.uint64) + GAP)
        out = np.full(int(out_off[-1] + caps[-1]) + GAP, GUARD, dtype=np.uint8)
        out_len, status = np.full(n, ROW_OUT_LEN, dtype=np.uint32), np.full(n, ROW_STATUS, dtype=np.int8)
        for i, claim in (claimed_len or {}).items():
            in_len[i] = claim
        assert not claimed_off or mem == MEM_HOST
        for i, claim in (claimed_off or {}).items():
            in_off[i] = claim
        before = np.ascontiguousarray(objs)
        held = dict(objs=before.copy(), ops=ops, flat=flat, in_off=in_off, in_len=in_len, out=out, out_off=out_off, caps=caps,
                    out_len=out_len, status=status)
        if mem == MEM_DEVICE:
            t = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else (v.view(np.int32) if v.dtype == np.uint32 else v)).to(self.dev)
                 for k, v in held.items()}
            p = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}
            stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        else:
            p = {k: v.ctypes.data_as(C.c_void_p) for k, v in held.items()}
            stream = None
        rc = self.lib.tamp_batch_compress_pieces(C.byref(conf), p["objs"], before.shape[1], p["ops"], p["flat"], p["in_off"], p["in_len"],
                                                 p["out"], p["out_off"], p["caps"], p["out_len"], p["status"], n, 0, mem, 0, stream)
        assert rc == OK, (rc, self.lib.tamp_amd_last_error())
        if mem == MEM_DEVICE:
            torch.cuda.synchronize()
            after, out = t["objs"].cpu().numpy(), t["out"].cpu().numpy()
            out_len, status = t["out_len"].cpu().numpy().view(np.uint32), t["status"].cpu().numpy()
            for k in ("ops", "flat", "in_off", "in_len", "out_off", "caps"):  # (inputs stay inputs)
                assert (t[k].cpu().numpy() == (held[k].view(np.int64) if held[k].dtype == np.uint64 else
                                              (held[k].view(np.int32) if held[k].dtype == np.uint32 else held[k]))).all(), k
        else:
            after = held["objs"]
        skip = (ops & SKIP) != 0
        assert (out_len[skip] == ROW_OUT_LEN).all() and (status[skip] == ROW_STATUS).all(), "rows of SKIP objects were written"
        assert (out_len[~skip] <= caps[~skip]).all()
        assert (after[skip] == before[skip]).all(), "SKIP objects were written"
        keep = np.ones(len(out), dtype=bool)  # the bytes no call may write
        for i in range(n):
            if not skip[i]:
                keep[int(out_off[i]) : int(out_off[i]) + (int(out_len[i]) if mem == MEM_HOST else int(caps[i]))] = False
        assert (out[keep] == GUARD).all(), "bytes outside the slabs%s were written" % (" or behind out_len" if mem == MEM_HOST else "")
        outs = [b"" if skip[i] else out[int(out_off[i]) : int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
        return status, out_len, outs, after

    def expect(self, conf, objs, ops, chunks, caps=None):
        """The single call for every object of a batch call that is not SKIP.  -> [(status, bytes, object afterwards)]"""
        return [None if ops[i] & SKIP else self.single(conf, objs[i], ops[i], chunks[i], None if caps is None else caps[i])
                for i in range(len(ops))]

    def same(self, got, want, ops, what):
        status, out_len, outs, after = got
        for i, w in enumerate(want):
            if w is None:
                continue
            assert (int(status[i]), outs[i]) == (w[0], w[1]), f"{what}: object {i} (op {ops[i]:#x}): status / bytes, want status {w[0]} and {len(w[1])} bytes"
            assert int(out_len[i]) == len(w[1])
            diff = state_diff(after[i], w[2])
            assert diff.size == 0, f"{what}: object {i} (op {ops[i]:#x}): the object differs at bytes {diff[:8]}"


@pytest.fixture(scope="module")
def hx():
    return Harness()


def state_diff(got, want):
    """Byte positions at which the object a batch call left differs from the single call's.  All of them count but one field:
    carry.ext_pos where carry.ext_count is 0.  The single call leaves there the window position of whichever extended match
    its kernel's serial walk took last -- a by-product of the launch's block size, which follows the piece's length, and no
    state (tests/test_gpu_cut_sweep.py reads the field only beside a count, too).  The batch call writes 0 there when a piece
    completes, so that no object depends on the other objects of its call (test_cut_sweep_one_call_per_step asserts the 0), and
    leaves an object that came with such a position as it was when the piece fails or has no input."""
    got, want = got.copy(), want.copy()
    if want[1] == 0:
        got[2:4] = want[2:4] = 0
    return np.flatnonzero(got != want)


def show(obj):
    return (f"object(rle={obj[0]} ext={obj[1]}@{int(obj[2]) | int(obj[3]) << 8} bits={obj[4]} tail={obj[5]} cached={obj[30]}@"
            f"{int(obj[28]) | int(obj[29]) << 8} window_pos={int(obj[32]) | int(obj[33]) << 8} token={obj[34]})")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the cut sweep, one launch sequence per step
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=[cs.case_id(w, e) for w, e in cs.CONFIGS])
def test_cut_sweep_one_call_per_step(hx, oracle, window, extended):
    src = cs.source(window)
    tokens, whole = cs.token_trace(oracle, src, window, extended)
    n = len(src)
    conf = hx.conf(window, extended)
    where = lambda c, what: f"{cs.case_id(window, extended)}: {cs.describe_cut(tokens, c)}: {what}"  # noqa: E731
    objs0 = hx.fresh(conf, n + 1)
    ops1 = [HEADER] * (n + 1)
    st1, _, out1, objs1 = hx.batch(conf, objs0, ops1, [src[:c] for c in range(n + 1)])  # (cut 0: a header and no input)
    assert (st1 == OK).all()
    ops2 = [RESUME | FINISH] * (n + 1)
    st2, _, out2, objs2 = hx.batch(conf, objs1, ops2, [src[c:] for c in range(n + 1)])  # (cut n: the empty finishing piece)
    assert (st2 == OK).all()
    for c in range(n + 1):
        assert out1[c] + out2[c] == whole, where(c, "first piece + finishing piece")
        assert out1[c] == whole[: len(out1[c])]
    # the object after step 1 against the single call's: inside RLE / extended-match tokens, on a full ring, every 8th other cut
    inside = [c for c in range(n + 1) if (t := cs.token_at(tokens, c)) is not None and t[0] in (2, 3) and cs.inside(t, c)]
    full = [c for c in range(n + 1) if objs1[c, 5] == 16]
    rest = [c for c in range(n + 1) if c not in set(inside) | set(full)][::8]
    if extended:
        assert inside and full, "the sweep must cut RLE / extended-match tokens and end calls on a full ring"
    for c in sorted(set(inside) | set(full) | set(rest)):
        res, bytes1, want = hx.single(conf, objs0[c], HEADER, src[:c])
        assert (res, bytes1) == (OK, out1[c]), where(c, "bytes of the first piece")
        diff = state_diff(objs1[c], want)
        assert diff.size == 0, where(c, f"{show(objs1[c])} vs the single call's {show(want)}, bytes {diff[:8]}")
    assert not objs1[objs1[:, 1] == 0][:, 2:4].any(), "an extended-match position without a count"
    # after the finish nothing is carried, and a piece without input writes nothing and changes nothing
    assert not objs2[:, :32].any() and not objs2[:, 34].any()
    st3, len3, _, objs3 = hx.batch(conf, objs2, [RESUME] * (n + 1), [b""] * (n + 1))
    assert (st3 == OK).all() and (len3 == 0).all() and (objs3 == objs2).all()
    print(f"piece-batch {cs.case_id(window, extended)}: {n + 1} cuts in 3 calls, {len(inside)} cuts inside RLE / extended tokens, "
          f"{len(full)} on a full ring, {len(rest)} others held against the single call")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. every class in ONE call (and 7.: the same from host memory)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", (MEM_DEVICE, MEM_HOST), ids=("device", "host"))
def test_every_class_in_one_call(hx, mem):
    from tamp_amd import workloads as wl

    prose = wl.frozen_corpus("prose")
    conf = hx.conf(10, True, dictionary_reset=True)
    src = cs.source(10)
    objs, ops, chunks = [], [], []

    def resumed(k, first_op=HEADER):
        """An object in the middle of its stream: `k` bytes of the sweep source taken by the single call."""
        res, _, obj = hx.single(conf, hx.fresh(conf)[0], first_op, src[:k])
        assert res == OK
        return obj

    def add(obj, op, data):
        objs.append(obj), ops.append(op), chunks.append(data)

    kinds = []
    for rep, k in enumerate((211, 700, 1203)):  # three of each kind, at different states, interleaved by class
        text = prose[5000 * rep : 5000 * rep + 900 + 37 * rep]
        broken = resumed(k)
        broken[5] = 17  # tail_len
        both = resumed(k)
        skipped = np.full(HDR + 1024, 0xC3, dtype=np.uint8)
        group = [("fresh+header", hx.fresh(conf)[0], HEADER, text),
                 ("resumed+finish+token", resumed(k), RESUME | FINISH | TOKEN, src[k:]),
                 ("fresh+append marker", hx.fresh(conf)[0], APPEND, text[::-1]),
                 ("broken carry", broken, RESUME, text),
                 ("resumed+unfinished", resumed(k), RESUME, src[k : k + 300]),
                 ("skip", skipped, SKIP | HEADER, text),
                 ("resumed+finish", resumed(k), RESUME | FINISH, src[k:]),
                 ("resumed, no input", resumed(k), RESUME, b""),
                 ("header and append marker", both, HEADER | APPEND | RESUME, text),
                 ("fresh+header+finish", hx.fresh(conf)[0], HEADER | FINISH, text),
                 ("resumed append+finish+token", resumed(k, APPEND), RESUME | FINISH | TOKEN, src[k : k + 100]),
                 ("fresh+header, no input", hx.fresh(conf)[0], HEADER, b""),
                 ("unknown op bit", resumed(k), RESUME | 64, text),
                 ("too long", resumed(k), RESUME | FINISH, text),
                 ("input beyond 2^64", resumed(k), RESUME | FINISH, text)]
        group = group[rep:] + group[:rep]
        for name, obj, op, data in group:
            kinds.append(name)
            add(obj, op, data)
    objs = np.stack(objs)
    # in_len above 0xFFFFFF00: refused for that object alone, and not a byte of the 4 GiB it claims is read
    too_long = dict(zip([i for i, name in enumerate(kinds) if name == "too long"], (0xFFFFFFFF, 0xFFFFFF01, 0xFFFFFFFF)))
    assert len(too_long) == 3
    # host memory: an input that would end beyond 2^64 is refused the same way (device memory: an ordinary finishing piece here)
    beyond = {i: 2**64 - 8 for i, name in enumerate(kinds) if name == "input beyond 2^64"} if mem == MEM_HOST else {}
    got = hx.batch(conf, objs, ops, chunks, mem=mem, claimed_len=too_long, claimed_off=beyond)
    # (the single call has no op byte: what only the batch call can refuse is held against the contract below instead)
    only_batch = ("header and append marker", "unknown op bit", "too long") + (("input beyond 2^64",) if beyond else ())
    want = hx.expect(conf, objs, [SKIP if kinds[i] in only_batch else op for i, op in enumerate(ops)], chunks)
    hx.same(got, want, ops, "every class in one call")
    status = got[0]
    for i, name in enumerate(kinds):
        if name in ("broken carry", "header and append marker", "unknown op bit", "too long") or i in beyond:
            assert status[i] == BAD_ARGUMENT and got[1][i] == 0 and (got[3][i] == objs[i]).all(), name
        elif name != "skip":
            assert status[i] == OK, name
    tokens = [int(got[3][i][34]) for i, name in enumerate(kinds) if "token" in name]
    assert tokens and all(tokens), "a stream that allows resets writes its FLUSH token"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. lazy matching: three pieces, the middle one 1 and 17 bytes
# ---------------------------------------------------------------------------------------------------------------------------
def test_lazy_matching_three_pieces(hx, oracle):
    src, _ = li.sweep_source(10, True)
    n = len(src)
    conf = hx.conf(10, True, lazy=True)
    rc, whole = oracle.compress(src, window=10, literal=8, extended=True, lazy_matching=True)
    assert rc == 0
    fresh = hx.fresh(conf)[0]
    first = [hx.single(conf, fresh, HEADER, src[:c]) for c in range(n + 1)]  # the single call at every cut
    cached = [c for c in range(n + 1) if first[c][2][30] != 0]
    assert cached, "no cut of the sweep source leaves a cached match"
    cuts = sorted(set(range(0, n + 1, 8)) | set(cached))
    cases = [(c, m) for c in cuts for m in (1, 17)]
    objs0 = hx.fresh(conf, len(cases))
    ops1, ops2, ops3 = [HEADER] * len(cases), [RESUME] * len(cases), [RESUME | FINISH] * len(cases)
    in1, in2, in3 = [src[:c] for c, _ in cases], [src[c : c + m] for c, m in cases], [src[c + m :] for c, m in cases]
    got1 = hx.batch(conf, objs0, ops1, in1)
    hx.same(got1, [first[c] for c, _ in cases], ops1, "lazy, first piece")
    assert sum(1 for c, _ in cases if got1[3][cases.index((c, 1))][30]) >= len(cached)
    got2 = hx.batch(conf, got1[3], ops2, in2)
    hx.same(got2, hx.expect(conf, got1[3], ops2, in2), ops2, "lazy, middle piece")
    got3 = hx.batch(conf, got2[3], ops3, in3)
    hx.same(got3, hx.expect(conf, got2[3], ops3, in3), ops3, "lazy, finishing piece")
    for k, (c, m) in enumerate(cases):
        assert got1[2][k] + got2[2][k] + got3[2][k] == whole, f"lazy: cut {c}, middle piece {m}"
    print(f"piece-batch lazy: {len(cases)} objects, {len(cached)} cuts leave a cached match: {cached[:12]}")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. too little room (and 7.: the same from host memory)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", (MEM_DEVICE, MEM_HOST), ids=("device", "host"))
def test_too_little_room(hx, mem):
    src = cs.source(10)
    conf = hx.conf(10, True)
    objs, ops, chunks, caps = [], [], [], []
    for c in (300, 777, 1250):
        res, first_bytes, mid = hx.single(conf, hx.fresh(conf)[0], HEADER, src[:c])
        assert res == OK
        for obj, op, data in ((hx.fresh(conf)[0], HEADER, src[:c]), (mid, RESUME | FINISH, src[c:])):
            res, ample, _ = hx.single(conf, obj, op, data)
            T = len(ample)
            assert res == OK and T > 1
            for cap in (0, T - 1, T, T + 1):
                objs.append(obj), ops.append(op), chunks.append(data), caps.append(cap)
    objs = np.stack(objs)
    got = hx.batch(conf, objs, ops, chunks, caps, mem=mem)
    want = hx.expect(conf, objs, ops, chunks, caps)
    hx.same(got, want, ops, "too little room")
    status, out_len, _, after = got
    for i in range(len(ops)):
        short = i % 4 < 2
        assert status[i] == (OUTPUT_FULL if short else OK), (i, caps[i])
        if short:
            assert (after[i] == objs[i]).all(), f"object {i}: changed by a piece that did not fit"
            assert out_len[i] == (caps[i] if ops[i] & FINISH else 0)  # (a finishing piece delivers what fitted)
    # TAMP_EXCESS_BITS: 7-bit literals and one byte >= 0x80 in the second piece
    conf7 = hx.conf(10, True, literal=7)
    text = bytes(b & 0x7F for b in src)
    res, _, mid = hx.single(conf7, hx.fresh(conf7)[0], HEADER, text[:500])
    assert res == OK
    bad = text[500:640] + b"\x80" + text[641:900]
    objs7 = np.stack([mid, mid, mid, mid])
    ops7 = [RESUME, RESUME | FINISH, RESUME, RESUME | FINISH | TOKEN]
    chunks7 = [bad, bad, text[500:900], text[500:900]]
    got7 = hx.batch(conf7, objs7, ops7, chunks7, mem=mem)
    hx.same(got7, hx.expect(conf7, objs7, ops7, chunks7), ops7, "excess bits")
    assert list(got7[0]) == [EXCESS_BITS, EXCESS_BITS, OK, OK]
    assert (got7[3][:2] == objs7[:2]).all() and got7[1][0] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 5. steady state over rounds
# ---------------------------------------------------------------------------------------------------------------------------
STREAMS, ROUNDS = 64, 6


def steady_inputs():
    """64 streams of up to 6 x 600 bytes from the frozen prose corpus, each with a 300-byte run and a repeated 200-byte block
    spliced in at seeded places (carried runs and extended matches cross round boundaries), and seeded piece lengths 0..600."""
    from tamp_amd import workloads as wl

    prose = wl.frozen_corpus("prose")
    assert len(prose) >= STREAMS * 4096
    rng = np.random.default_rng(20240917)
    lens = rng.integers(0, 601, size=(ROUNDS, STREAMS))
    lens[0, 3] = lens[2, 5] = lens[5, 7] = 0  # (a first write, a middle one and the last one without input)
    streams = []
    for i in range(STREAMS):
        b = bytearray(prose[4096 * i : 4096 * (i + 1)])
        total = int(lens[:, i].sum())
        at = int(rng.integers(0, max(total - 300, 1)))
        b[at : at + 300] = bytes([b[at]]) * 300
        at = int(rng.integers(250, max(total - 200, 251)))
        b[at : at + 200] = b[at - 230 : at - 30]
        streams.append(bytes(b[:total]))
    pieces = []
    for r in range(ROUNDS):
        starts = lens[:r].sum(axis=0)
        pieces.append([streams[i][int(starts[i]) : int(starts[i]) + int(lens[r, i])] for i in range(STREAMS)])
    return streams, pieces


STEADY = ((8, True), (10, True), (10, False), (15, True))
steady_configs = pytest.mark.parametrize("window,extended", STEADY, ids=[cs.case_id(w, e) for w, e in STEADY])


@pytest.fixture(scope="module")
def steady(oracle):
    streams, pieces = steady_inputs()
    whole = {}

    def want(window, extended):
        if (window, extended) not in whole:
            r = [oracle.compress(s, window=window, literal=8, extended=extended) for s in streams]
            assert all(rc == 0 for rc, _ in r)
            whole[(window, extended)] = [b for _, b in r]
        return whole[(window, extended)]

    return streams, pieces, want


@steady_configs
def test_steady_state_rounds_c_call(hx, steady, window, extended):
    streams, pieces, want = steady
    conf = hx.conf(window, extended)
    objs = hx.fresh(conf, STREAMS)
    got = [b""] * STREAMS
    for r in range(ROUNDS):
        st, _, outs, objs = hx.batch(conf, objs, [HEADER if r == 0 else RESUME] * STREAMS, pieces[r])
        assert (st == OK).all(), f"round {r}"
        got = [g + o for g, o in zip(got, outs)]
    st, _, outs, objs = hx.batch(conf, objs, [RESUME | FINISH] * STREAMS, [b""] * STREAMS)
    assert (st == OK).all() and not objs[:, :32].any()
    got = [g + o for g, o in zip(got, outs)]
    for i, w in enumerate(want(window, extended)):
        assert got[i] == w, f"stream {i} of {len(streams[i])} bytes"


@steady_configs
def test_steady_state_rounds_compressor_batch(steady, window, extended):
    import tamp_amd

    streams, pieces, want = steady
    batch = tamp_amd.CompressorBatch(STREAMS, window=window, extended=extended)
    got = [b""] * STREAMS
    for r in range(ROUNDS):
        res = batch.write(pieces[r] if r % 2 else [p or None for p in pieces[r]])  # (None and b"" both mean: nothing for this stream)
        assert (res.status.cpu().numpy() == OK).all()
        got = [g + o for g, o in zip(got, res.streams())]
    res = batch.close()
    got = [g + o for g, o in zip(got, res.streams())]
    for i, w in enumerate(want(window, extended)):
        assert got[i] == w, f"stream {i} of {len(streams[i])} bytes"
    assert all(batch.close().out_len.cpu().numpy() == 0)  # (closed and byte aligned: nothing more to write)


@steady_configs
def test_steady_state_flush_every_round(steady, window, extended):
    """flush(write_token=True) after every round: the streams of 64 single ``tamp_amd.Compressor`` objects fed the same calls,
    and they decode back."""
    import tamp_amd

    streams, pieces, _ = steady
    batch = tamp_amd.CompressorBatch(STREAMS, window=window, extended=extended)
    files = [io.BytesIO() for _ in range(STREAMS)]
    singles = [tamp_amd.Compressor(f, window=window, extended=extended) for f in files]
    got = [b""] * STREAMS
    for r in range(ROUNDS):
        for res in (batch.write(pieces[r]), batch.flush(write_token=True)):
            got = [g + o for g, o in zip(got, res.streams())]
        for c, p in zip(singles, pieces[r]):
            c.write(p)
            c.flush(write_token=True)
    got = [g + o for g, o in zip(got, batch.close().streams())]
    for c in singles:
        c.close()
    for i, f in enumerate(files):
        assert got[i] == f.getvalue(), f"stream {i}"
    back = tamp_amd.decompress_batch(got, out_cap=4096 + 64)
    for i in range(STREAMS):
        assert back.stream(i) == streams[i], f"stream {i} does not decode back"


def test_compressor_batch_device_input_and_which(steady):
    """``write`` from CUDA tensors, ``flush`` of some streams only."""
    import torch

    import tamp_amd

    streams, pieces, _ = steady
    dev = torch.device("cuda:0")
    batch = tamp_amd.CompressorBatch(STREAMS)
    files = [io.BytesIO() for _ in range(STREAMS)]
    singles = [tamp_amd.Compressor(f) for f in files]
    got = [b""] * STREAMS
    some = list(range(0, STREAMS, 3))
    for r in range(3):
        flat, off, length = tamp_amd.pack_streams(pieces[r])
        res = batch.write(torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                          torch.from_numpy(length.astype(np.int32)).to(dev))
        for res in (res, batch.flush(which=some)):
            got = [g + o for g, o in zip(got, res.streams())]
        for i, (c, p) in enumerate(zip(singles, pieces[r])):
            c.write(p)
            if i in some:
                c.flush()
    got = [g + o for g, o in zip(got, batch.close().streams())]
    for i, (c, f) in enumerate(zip(singles, files)):
        c.close()
        assert got[i] == f.getvalue(), f"stream {i}"


# ---------------------------------------------------------------------------------------------------------------------------
# 6. custom dictionary and reset_dictionary
# ---------------------------------------------------------------------------------------------------------------------------
def test_custom_dictionary_and_reset(steady):
    import tamp_amd

    streams, _, _ = steady
    dictionary = bytes(streams[9][:200] + streams[10][:56])
    assert len(dictionary) == 1 << 8
    kw = dict(window=8, dictionary=dictionary, dictionary_reset=True)
    batch = tamp_amd.CompressorBatch(8, **kw)
    files = [io.BytesIO() for _ in range(8)]
    singles = [tamp_amd.Compressor(f, **kw) for f in files]
    first = [streams[i][:500 + 13 * i] for i in range(8)]
    second = [streams[i][500 + 13 * i : 1400] for i in range(8)]
    got = [b""] * 8
    for res in (batch.write(first), batch.reset_dictionary(which=[1, 5]), batch.write(second), batch.close()):
        assert (res.status.cpu().numpy() == OK).all()
        got = [g + o for g, o in zip(got, res.streams())]
    for i, c in enumerate(singles):
        c.write(first[i])
        if i in (1, 5):
            c.reset_dictionary()
        c.write(second[i])
        c.close()
        assert got[i] == files[i].getvalue(), f"stream {i}"
    assert got[1] != got[0] and len({len(g) for g in got}) > 1


def test_append_mode_and_reset_of_some_streams(steady):
    """``append=True`` (a FLUSH padded to 16 bits instead of a header) and ``reset_dictionary`` on seeded windows: the bytes of single
    ``tamp_amd.Compressor`` objects given the same calls, and the appended streams decode behind a stream of the same kind."""
    import tamp_amd

    streams, _, _ = steady
    kw = dict(window=10, dictionary_reset=True, append=True)
    batch = tamp_amd.CompressorBatch(6, **kw)
    files = [io.BytesIO() for _ in range(6)]
    singles = [tamp_amd.Compressor(f, **kw) for f in files]
    got = [b""] * 6
    parts = [[streams[20 + i][a:b] for i in range(6)] for a, b in ((0, 700), (700, 701), (701, 1500))]
    calls = (lambda: batch.write(parts[0]), lambda: batch.flush(which=[0, 2]), lambda: batch.write(parts[1]),
             lambda: batch.reset_dictionary(which=[2, 3]), lambda: batch.flush(), lambda: batch.write(parts[2]), batch.close)
    for call in calls:
        res = call()
        assert (res.status.cpu().numpy() == OK).all()
        got = [g + o for g, o in zip(got, res.streams())]
    for i, c in enumerate(singles):
        c.write(parts[0][i])
        if i in (0, 2):
            c.flush()
        c.write(parts[1][i])
        if i in (2, 3):
            c.reset_dictionary()
        c.flush()
        c.write(parts[2][i])
        c.close()
        assert got[i] == files[i].getvalue(), f"stream {i}"
    front = io.BytesIO()  # (closed with its FLUSH token: with the appended stream's marker that is a dictionary reset)
    with tamp_amd.Compressor(front, window=10, dictionary_reset=True) as c:
        c.write(b"in front")
    head = front.getvalue()
    for i in range(6):
        assert bytes(tamp_amd.decompress(head + got[i])) == b"in front" + streams[20 + i][:1500], f"stream {i}"


def test_a_failed_piece_ends_its_streams_write(steady):
    """7-bit literals, a ``write`` cut into several pieces (``PIECE_MAX`` lowered for the test): the stream whose second piece holds
    a byte >= 0x80 reports TAMP_EXCESS_BITS, delivers the bytes of its first piece only and stays where that piece left it --
    its later pieces are not sent -- and the other streams are those of single ``tamp_amd.Compressor`` objects."""
    import tamp_amd

    streams, _, _ = steady
    text = [bytes(b & 0x7F for b in streams[30 + i][:1000]) for i in range(4)]
    text[2] = text[2][:300] + b"\x80" + text[2][301:]
    batch = tamp_amd.CompressorBatch(4, literal=7)
    batch._piece_max = 256
    res = batch.write(text)
    status = res.status.cpu().numpy()
    assert list(status) == [OK, OK, EXCESS_BITS, OK]
    first_only = tamp_amd.CompressorBatch(1, literal=7)
    want = first_only.write([text[2][:256]])
    assert res.stream(2) == want.stream(0)
    assert (batch.objects[2].cpu().numpy() == first_only.objects[0].cpu().numpy()).all(), "the failed stream's object moved on"
    closing = batch.close()
    for i in (0, 1, 3):
        f = io.BytesIO()
        with tamp_amd.Compressor(f, literal=7) as c:
            c.write(text[i])
        assert res.stream(i) + closing.stream(i) == f.getvalue(), f"stream {i}"
