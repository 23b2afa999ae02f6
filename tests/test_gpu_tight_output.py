"""GPU tier (-m gpu): compress with too little output room, on every build of the compress kernel.

The rule (include/tamp_amd.h, tamp_batch_compress): with T = the stream's length with ample room and S = its status there, a slab
of ``cap`` bytes gets (TAMP_OUTPUT_FULL, the first ``cap`` bytes) when ``cap < T`` and (S, all T bytes) otherwise, and nothing is
written at or behind the slab's end.  Every build shares the code that decides this (the end of the emit phase in
tamp_compress_kernel.hpp); each build reaches it with its own epochs, flush boundaries and store alignments.

One SWEEP is one batch call: the same input once per capacity, slab ``j`` with ``cap = j`` for ``j = 0 .. T + 2``, the slabs laid
back to back -- so neighbouring slabs start at every byte alignment, and a store at or behind a slab's end lands in a neighbour
whose bytes are known, or in the guard bytes around the slabs.  The output buffer is filled with a pattern before the call and
compared WHOLE afterwards: the expected prefixes where they belong, the pattern everywhere else.  Every expectation is the
oracle's (oracle/libtamp_oracle.so at the same capacity; pinned against the reference, capacity by capacity, by
tests/test_oracle_vs_reference.py), never a result of the GPU's own.  Inputs: tests/tight_output_input.py.
"""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tight_output_input as toi  # noqa: E402
from tight_check import LEAD, TAIL, check_call, env, pattern, slab_layout  # noqa: E402,F401

pytestmark = pytest.mark.gpu

OK, OUTPUT_FULL, EXCESS_BITS = toi.OK, toi.OUTPUT_FULL, toi.EXCESS_BITS
MEM_HOST, MEM_DEVICE = 0, 1
BUILD_GENERIC, BUILD_FIXED_EXT, BUILD_FIXED_V1 = 0, 1, 2
CALL_DICT_TABLE = 128  # include/tamp_amd.h TAMP_AMD_CALL_DICT_TABLE
HINT_AUTO, HINT_RUNS = 0, 2


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    lib = _lib.load()  # raises if the native library is missing: no silent fallback
    assert lib.tamp_amd_device_count() >= 1, "no HIP device visible"
    return lib


def make_conf(window, literal, extended, lazy=False, custom=False, hint=HINT_AUTO):
    from tamp_amd import _lib

    return _lib.TampAmdConf(window, literal, int(custom), int(extended), 0, int(lazy), hint, 0)


def custom_dictionary(window, literal, seed):
    return toi._mask(toi.text(1 << window, seed), literal)


# ---------------------------------------------------------------------------------------------------------------------
# expectations: one oracle sweep per (configuration, input, dictionary), shared by every test that runs it
# ---------------------------------------------------------------------------------------------------------------------
class Sweep:
    """``x`` once per capacity 0 .. T + 2 and what the oracle gives each slab."""

    def __init__(self, oracle, x, window, literal, extended, lazy, dictionary, n_caps=None):
        kw = dict(window=window, literal=literal, extended=extended, dictionary=dictionary)
        self.S, self.full = oracle.compress(x, lazy_matching=lazy, **kw)
        assert self.S in (OK, EXCESS_BITS)
        self.x, self.T = x, len(self.full)
        n = self.T + 3 if n_caps is None else n_caps
        self.caps = np.arange(n, dtype=np.uint32)
        flat = np.frombuffer(x * n, dtype=np.uint8)
        want = oracle.compress_batch(flat, np.arange(n, dtype=np.uint64) * len(x), np.full(n, len(x), np.uint32),
                                     out_cap=self.caps, lazy=lazy, threads=16, **kw)
        self.status, self.out_len = np.asarray(want.status).astype(np.int64), np.asarray(want.out_len).astype(np.int64)
        self.streams = [want.stream(j) for j in range(n)]
        # (the oracle states the rule: a sweep is the stream's ample-room bytes cut at every capacity)
        for j in range(n):
            assert (int(self.status[j]), self.streams[j]) == toi.rule(self.S, self.full, j), ("oracle off the rule", j)


_sweeps = {}


def sweep_of(oracle, x, window, literal, extended, lazy=False, dictionary=None, n_caps=None):
    key = (x, window, literal, extended, lazy, dictionary, n_caps)
    if key not in _sweeps:
        _sweeps[key] = Sweep(oracle, x, window, literal, extended, lazy, dictionary, n_caps)
    return _sweeps[key]


def inputs_of(kind, literal):
    """The inputs of a case: the clean one and, below 8-bit literals, one with the offending byte first, one with it in the
    middle (long input: just behind the first epoch boundary) and one with it last."""
    if kind == "short":
        x = toi.short_input(literal)
        return toi.with_offenders(x, literal, (0, len(x) // 2, len(x) - 1))
    x = toi.long_input(literal)
    return toi.with_offenders(x, literal, (0, toi.BEHIND_BOUNDARY, len(x) - 1))


# ---------------------------------------------------------------------------------------------------------------------
# one batch call on a patterned buffer, and its comparison with the expectation
# ---------------------------------------------------------------------------------------------------------------------
def batch_call(lib, mem, conf, streams, caps, max_in_len, gap=0, dictionary=None, table=None):
    """tamp_batch_compress (``table`` = (dictionaries, selectors): tamp_batch_compress_dicts) on slabs ``gap`` bytes apart in
    a buffer filled with pattern().  -> (status, out_len, the whole buffer, out_off), on the host."""
    from tamp_amd.batch import pack_streams

    flat, in_off, in_len = pack_streams(streams)
    caps = np.asarray(caps, dtype=np.uint32)
    n = len(caps)
    out_off, out = slab_layout(caps, gap)
    out_len, status = np.full(n, 0x7FFFFFFF, np.uint32), np.full(n, 99, np.int8)
    dict_buf = dict_off = None
    if table is not None:
        dicts, sel = table
        dict_buf = np.frombuffer(b"".join(dicts), dtype=np.uint8)
        dict_off = np.asarray(sel, dtype=np.uint64) * np.uint64(len(dicts[0]))
    elif dictionary is not None:
        dict_buf = np.frombuffer(dictionary, dtype=np.uint8)
    host = [flat, in_off, in_len, out, out_off, caps, out_len, status, dict_buf, dict_off]
    if mem == MEM_DEVICE:
        import torch

        dev = torch.device("cuda:0")
        as_signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
        held = [None if a is None else torch.from_numpy(a.view(as_signed.get(a.dtype, a.dtype)).copy()).to(dev) for a in host]
        ptr = [None if t is None else C.c_void_p(t.data_ptr()) for t in held]
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    else:
        held = host
        ptr = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in host]
        stream = None
    p_in, p_in_off, p_in_len, p_out, p_out_off, p_cap, p_len, p_status, p_dict, p_dict_off = ptr
    if table is not None:
        rc = lib.tamp_batch_compress_dicts(C.byref(conf), p_dict, int(dict_buf.size), p_dict_off, p_in, p_in_off, p_in_len, p_out,
                                           p_out_off, p_cap, p_len, p_status, n, max_in_len, mem, 0, stream)
    else:
        rc = lib.tamp_batch_compress(C.byref(conf), p_dict, p_in, p_in_off, p_in_len, p_out, p_out_off, p_cap, p_len, p_status,
                                     n, max_in_len, mem, 0, stream)
    assert rc == 0, rc
    if mem == MEM_DEVICE:
        torch.cuda.synchronize()
        out, out_len, status = held[3].cpu().numpy(), held[6].cpu().numpy().view(np.uint32), held[7].cpu().numpy()
    return status.astype(np.int64), out_len.astype(np.int64), out, out_off


def run_sweep(lib, mem, conf, sw, max_in_len, tag, gap=0, dictionary=None):
    got = batch_call(lib, mem, conf, [sw.x] * len(sw.caps), sw.caps, max_in_len, gap=gap, dictionary=dictionary)
    check_call(got, sw.caps, sw.status, sw.out_len, sw.streams, tag, behind_len_unspecified=(mem == MEM_HOST and gap == 0))
    return set(int(s) for s in sw.status)


def planned(lib, window, max_in_len, lazy=False):
    """-> (block, LDS bytes, threads, workgroups per CU) of tamp_amd_compress_plan"""
    v = [C.c_uint32(0) for _ in range(4)]
    assert lib.tamp_amd_compress_plan(window, max_in_len, int(lazy), *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the sweeps, one case per build
# ---------------------------------------------------------------------------------------------------------------------
# (id, window, literal, extended, lazy, run-aware hint, input, TAMP_AMD_FIXED_BUILD, shared custom dictionary,
#  what tamp_amd_compress_build names, threads per workgroup of tamp_amd_compress_plan)
CASES = [
    ("lean_w10", 10, 8, True, False, False, "short", None, False, BUILD_GENERIC, 64),
    ("lean_w9_l5", 9, 5, True, False, False, "short", None, False, BUILD_GENERIC, 64),
    ("short_runs_w10_l7", 10, 7, True, False, True, "short", None, False, BUILD_GENERIC, 64),
    ("lean_w10_stale_bound", 10, 8, True, False, False, "long, short bound", None, False, BUILD_GENERIC, 64),
    ("runs_w8_v1", 8, 8, False, False, False, "long", None, False, BUILD_GENERIC, 256),
    ("runs_w12_l7", 12, 7, True, False, False, "long", None, False, BUILD_GENERIC, 256),
    ("u16_index_w15", 15, 8, True, False, False, "long", None, False, BUILD_GENERIC, 256),
    ("fixed_ext", 10, 8, True, False, False, "long", None, False, BUILD_FIXED_EXT, 256),
    ("fixed_v1", 10, 8, False, False, False, "long", None, False, BUILD_FIXED_V1, 256),
    ("generic_w10", 10, 8, True, False, False, "long", "0", False, BUILD_GENERIC, 256),
    ("lazy_w10_l7", 10, 7, True, True, False, "long", None, False, BUILD_GENERIC, 256),
    ("lazy_w15", 15, 8, True, True, False, "long", None, False, BUILD_GENERIC, 256),
    ("shared_dictionary_w10", 10, 8, True, False, False, "long", None, True, BUILD_FIXED_EXT, 256),
]


def case_geometry(kind):
    """max_in_len of a case's calls: the short input's own length (below 1 KiB: one-wavefront workgroups), 1,024 for the long
    one -- epochs of 1,024 positions, so its 2,560 bytes are two and a half of them.  "long, short bound": the long input under
    the short one's bound, which only sizes the block -- the one-wavefront build takes it in eight epochs of 320 positions."""
    return toi.BLOCK if kind == "long" else len(toi.short_input())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sweep_on_every_build(lib, oracle, case):
    _, window, literal, extended, lazy, runs, kind, fixed_env, shared, build, threads = case
    max_in_len = case_geometry(kind)
    conf = make_conf(window, literal, extended, lazy, custom=shared, hint=HINT_RUNS if runs else HINT_AUTO)
    dictionary = custom_dictionary(window, literal, 21) if shared else None
    seen = set()
    with (env("TAMP_AMD_FIXED_BUILD", fixed_env) if fixed_env is not None else contextlib.nullcontext()):
        assert lib.tamp_amd_compress_build(C.byref(conf), max_in_len, 0, 0) == build
        blk, _, plan_threads, _ = planned(lib, window, max_in_len, lazy)
        assert plan_threads == threads and blk == (toi.BLOCK if kind == "long" else 320), (blk, plan_threads)
        for k, x in enumerate(inputs_of(kind, literal)):
            sw = sweep_of(oracle, x, window, literal, extended, lazy, dictionary)
            # (long input: two and a half epochs, each emitting hundreds of bytes -- capacities inside every one of them)
            assert kind == "short" or (len(x) == toi.LONG_LEN and (sw.S != OK or sw.T > 700))
            seen |= run_sweep(lib, MEM_DEVICE, conf, sw, max_in_len, (case[0], "input", k), dictionary=dictionary)
    assert seen == ({OK, OUTPUT_FULL} if literal == 8 else {OK, OUTPUT_FULL, EXCESS_BITS})


def test_sweep_on_a_dictionary_table_with_two_dictionaries(lib, oracle):
    """tamp_batch_compress_dicts: slab j is compressed under dictionary j % 2, so neighbouring slabs hold different streams."""
    window, literal, extended = 10, 8, True
    x = toi.long_input(literal)
    dicts = [custom_dictionary(window, literal, 31), toi.long_input(literal)[300 : 300 + (1 << window)]]
    n = max(len(oracle.compress(x, window=window, dictionary=d)[1]) for d in dicts) + 3
    per_dict = [sweep_of(oracle, x, window, literal, extended, dictionary=d, n_caps=n) for d in dicts]
    assert per_dict[0].full != per_dict[1].full
    sel = [j % 2 for j in range(n)]
    want_status = np.array([per_dict[k].status[j] for j, k in enumerate(sel)])
    want_len = np.array([per_dict[k].out_len[j] for j, k in enumerate(sel)])
    want_streams = [per_dict[k].streams[j] for j, k in enumerate(sel)]
    conf = make_conf(window, literal, extended, custom=True)
    assert lib.tamp_amd_compress_build(C.byref(conf), toi.BLOCK, CALL_DICT_TABLE, 0) == BUILD_GENERIC
    caps = np.arange(n, dtype=np.uint32)
    for mem in (MEM_DEVICE, MEM_HOST):
        got = batch_call(lib, mem, conf, [x] * n, caps, toi.BLOCK, table=(dicts, sel))
        check_call(got, caps, want_status, want_len, want_streams, ("dictionary table", mem), behind_len_unspecified=mem == MEM_HOST)
    assert set(int(s) for s in want_status) == {OK, OUTPUT_FULL}


def test_sweep_through_the_expensive_first_permutation(lib, oracle):
    """TAMP_AMD_LPT=1: the streams are compressed in another order and their results scattered back.  One call with the clean
    input and two offending ones, capacity by capacity: all three statuses, each at its own row."""
    window, literal, extended = 12, 7, True
    xs = inputs_of("long", literal)
    sweeps = [sweep_of(oracle, x, window, literal, extended) for x in (xs[0], xs[2], xs[3])]
    streams = [sw.x for sw in sweeps for _ in sw.caps]
    caps = np.concatenate([sw.caps for sw in sweeps])
    want_status, want_len = np.concatenate([sw.status for sw in sweeps]), np.concatenate([sw.out_len for sw in sweeps])
    conf = make_conf(window, literal, extended)
    assert planned(lib, window, toi.BLOCK)[2] == 256  # (the ordering is for four-wavefront workgroups)
    with env("TAMP_AMD_LPT", "1"):
        got = batch_call(lib, MEM_DEVICE, conf, streams, caps, toi.BLOCK)
    check_call(got, caps, want_status, want_len, [s for sw in sweeps for s in sw.streams], "expensive first")
    assert set(int(s) for s in want_status) == {OK, OUTPUT_FULL, EXCESS_BITS}


HOST_CASES = [c for c in CASES if c[0] in ("lean_w10", "fixed_ext", "runs_w12_l7")]


@pytest.mark.parametrize("gap", [0, 5], ids=["tiled", "gapped"])
@pytest.mark.parametrize("case", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_sweep_from_host_memory(lib, oracle, case, gap):
    """The host-memory call: tiled slabs come back in one transfer (slab bytes behind out_len are unspecified, everything
    else is checked), slabs with gaps get exactly their produced bytes."""
    _, window, literal, extended, lazy, _, kind, _, _, _, _ = case
    conf = make_conf(window, literal, extended, lazy)
    xs = inputs_of(kind, literal)
    seen = set()
    for k, x in enumerate(xs if gap == 0 else xs[-2:]):
        sw = sweep_of(oracle, x, window, literal, extended, lazy)
        seen |= run_sweep(lib, MEM_HOST, conf, sw, case_geometry(kind), (case[0], "host", gap, k), gap=gap)
    assert seen >= {OUTPUT_FULL, OK if literal == 8 else EXCESS_BITS}


# ---------------------------------------------------------------------------------------------------------------------
# 2. the one-stream calls
# ---------------------------------------------------------------------------------------------------------------------
def guarded(size):
    """A buffer of ``size`` bytes of room with TAIL guard bytes behind it."""
    return pattern(size + TAIL)


def assert_guard(buf, size, written, tag):
    assert written <= size, tag
    assert np.array_equal(buf[written:], pattern(size + TAIL)[written:]), tag + ("written behind the produced bytes",)


ONE_STREAM = [("w10_short", 10, 8, True, "short", None), ("w10_long", 10, 8, False, "long", None),
              ("w12_l6_offending", 12, 6, True, "long", 1500), ("w9_l5_offending_last", 9, 5, True, "short", 299)]


@pytest.mark.parametrize("case", ONE_STREAM, ids=[c[0] for c in ONE_STREAM])
def test_one_stream_compress_with_short_output_size(lib, oracle, case):
    """tamp_amd_compress with output_size in {0, 1, T - 1, T, T + 1}: the oracle's status and bytes at that capacity."""
    _, window, literal, extended, kind, bad = case
    x = toi.short_input(literal) if kind == "short" else toi.long_input(literal)
    if bad is not None:
        x = toi.offending(x, literal, bad)
    S, full = oracle.compress(x, window=window, literal=literal, extended=extended)
    T = len(full)
    assert S == (OK if bad is None else EXCESS_BITS) and T > 3
    conf = make_conf(window, literal, extended)
    src = np.frombuffer(x, dtype=np.uint8)
    seen = set()
    for size in (0, 1, T - 1, T, T + 1):
        want = oracle.compress(x, window=window, literal=literal, extended=extended, cap=size)
        assert want == toi.rule(S, full, size)
        buf, written = guarded(size), C.c_size_t(12345)
        st = lib.tamp_amd_compress(C.byref(conf), None, buf.ctypes.data_as(C.c_void_p), size, C.byref(written),
                                   src.ctypes.data_as(C.c_void_p), len(x), 0)
        assert (st, buf[: written.value].tobytes()) == want, (case[0], size, st, written.value)
        assert_guard(buf, size, written.value, (case[0], size))
        seen.add(st)
    assert seen == {OUTPUT_FULL, S}


class HostObject:
    """A compressor object as the segment and piece calls see it: window bytes, window position, carry."""

    def __init__(self, window):
        from tamp_amd import _lib

        self.window_state = pattern(1 << window)  # (a fresh stream without a custom dictionary ignores it on input)
        self.window_pos = C.c_uint16(7)
        self.carry = _lib.TampAmdCarry()

    def snapshot(self):
        return self.window_state.tobytes(), self.window_pos.value, bytes(self.carry)

    def restore(self, snap):
        self.window_state[:] = np.frombuffer(snap[0], dtype=np.uint8)
        self.window_pos.value = snap[1]
        C.memmove(C.byref(self.carry), snap[2], len(snap[2]))


def segment_call(lib, conf, obj, data, size, *, first, flush_token, piece=None):
    """tamp_amd_compress_segment, or with ``piece`` = finish: tamp_amd_compress_piece.  -> (status, bytes written)"""
    src = np.frombuffer(data, dtype=np.uint8)
    buf, written, token = guarded(size), C.c_size_t(12345), C.c_int(0)
    head = (C.byref(conf), int(first), 0, int(not first))
    tail = (buf.ctypes.data_as(C.c_void_p), size, C.byref(written), src.ctypes.data_as(C.c_void_p), len(data), C.byref(token), 0)
    ws = obj.window_state.ctypes.data_as(C.c_void_p)
    if piece is None:
        st = lib.tamp_amd_compress_segment(*head, int(flush_token), ws, C.byref(obj.window_pos), *tail)
    else:
        st = lib.tamp_amd_compress_piece(*head, int(piece), int(flush_token), ws, C.byref(obj.window_pos), C.byref(obj.carry), *tail)
    assert_guard(buf, size, written.value, ("segment call", size))
    return st, buf[: written.value].tobytes()


SEGMENT_CONFS = [(10, 8, True), (12, 6, True), (9, 8, False)]


@pytest.mark.parametrize("conf3", SEGMENT_CONFS, ids=["w10", "w12_l6", "w9_v1"])
def test_segment_with_too_little_room_leaves_the_object_alone(lib, oracle, conf3):
    """Two segments of one stream (write, flush with a token, write, close).  Each first with no room and with one byte too
    few: TAMP_OUTPUT_FULL, what fitted is the start of the segment, window_state and *window_pos byte-identical to what they
    were; then with exactly enough: the bytes of the uninterrupted script."""
    window, literal, extended = conf3
    x = toi.long_input(literal)
    parts = (x[:1300], x[1300:])
    kw = dict(window=window, literal=literal, extended=extended)
    st, want = oracle.stream_script([("write", parts[0]), ("flush", True), ("write", parts[1]), ("close",)], **kw)
    st1, want1 = oracle.stream_script([("write", parts[0]), ("flush", True)], **kw)
    assert st == st1 == OK and want.startswith(want1)
    segments = (want1, want[len(want1):])
    conf, obj, emitted = make_conf(window, literal, extended), HostObject(window), b""
    for k, (data, seg) in enumerate(zip(parts, segments)):
        before = obj.snapshot()
        for size in (0, len(seg) - 1):
            got = segment_call(lib, conf, obj, data, size, first=k == 0, flush_token=k == 0)
            assert got == (OUTPUT_FULL, seg[:size]), (conf3, k, size, got[0], len(got[1]))
            assert obj.snapshot() == before, (conf3, k, size, "the object changed")
        got = segment_call(lib, conf, obj, data, len(seg), first=k == 0, flush_token=k == 0)
        assert got == (OK, seg), (conf3, k, got[0], len(got[1]))
        emitted += got[1]
    assert emitted == want


@pytest.mark.parametrize("conf3", SEGMENT_CONFS, ids=["w10", "w12_l6", "w9_v1"])
def test_piece_with_too_little_room_leaves_the_object_alone(lib, oracle, conf3):
    """Three pieces of one stream, the last one finishing it.  A piece that does not finish and does not fit delivers NOTHING
    (its bytes would be emitted twice when it is offered again) and leaves window_state, *window_pos and *carry
    byte-identical; the finishing piece delivers what fitted, as a segment does.  How many bytes a middle piece needs is not
    the oracle's to say (it has no pieces): the call is made once with ample room to learn it, put back, made with one byte
    too few, and made again with exactly enough -- same bytes, same object as with ample room.  The oracle judges the sum:
    the pieces together are the uninterrupted stream."""
    window, literal, extended = conf3
    x = toi.long_input(literal)
    parts = (x[:900], x[900:2000], x[2000:])
    st, want = oracle.compress(x, window=window, literal=literal, extended=extended)
    assert st == OK
    conf, obj, emitted = make_conf(window, literal, extended), HostObject(window), b""
    for k, data in enumerate(parts):
        finish = k == len(parts) - 1
        call = dict(first=k == 0, flush_token=False, piece=finish)
        before = obj.snapshot()
        if finish:
            need, ample = len(want) - len(emitted), None
        else:
            ample = segment_call(lib, conf, obj, data, int(lib.tamp_amd_compress_bound(len(data) + 271, literal, 0)), **call)
            assert ample[0] == OK and want.startswith(emitted + ample[1]), (conf3, k, ample[0])
            need, after_ample = len(ample[1]), obj.snapshot()
            obj.restore(before)
        assert need > 1
        for size in (0, need - 1):
            got = segment_call(lib, conf, obj, data, size, **call)
            assert got == (OUTPUT_FULL, want[len(emitted):len(emitted) + size] if finish else b""), (conf3, k, size, got[0], len(got[1]))
            assert obj.snapshot() == before, (conf3, k, size, "the object changed")
        got = segment_call(lib, conf, obj, data, need, **call)
        assert got[0] == OK and (finish or (got == ample and obj.snapshot() == after_ample)), (conf3, k, got[0], len(got[1]))
        emitted += got[1]
    assert emitted == want
