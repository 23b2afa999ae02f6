"""GPU tier: the seek index of streams without dictionary resets (tamp_batch_seek_index, tamp_batch_read_ranges_seek,
``build_seek_index`` / ``read_ranges_seek``; the kernels of tamp_seek_kernel.hpp, DESIGN.md 3.13 "Reading ranges by checkpoint").

Every expectation comes from the oracle's decoder object driven as the header defines a checkpoint (tests/seek_index_input.py) or
is a slice of the ORIGINAL input, never a GPU result.  The C entry points are called directly where the test lays out the buffers
itself: rows behind 0xEE, output room behind 0xA5 guards, result tables poisoned before the call."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cut_sweep_input as cs  # noqa: E402
import seek_index_input as si  # noqa: E402
from seek_index_input import BAD_INDEX, INPUT_EXHAUSTED, OK, OOB  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, ROW_FILL, GAP = 0xA5, 0xEE, 5
MEMS = ("host", "device")


@pytest.fixture(scope="module")
def ta():
    import tamp_amd
    from tamp_amd import _lib

    _lib.load()  # raises if the native library is missing: no silent fallback
    return tamp_amd


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pack(blobs):
    from tamp_amd.batch import pack_streams

    flat, off, length = pack_streams(blobs)
    return (flat if flat.size else np.zeros(1, np.uint8)), off, length


class _Mem:
    """Arrays of a call where `mem` says: numpy as they are, or copied to the device and back."""

    def __init__(self, mem):
        self.mem, self.pairs = mem, []

    def __call__(self, a):
        if a is None:
            return None
        if self.mem == "host":
            return _p(a)
        import torch

        t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda")
        if a.flags.writeable:  # (what the call may write comes back; the streams are read-only on both sides)
            self.pairs.append((a, t))
        else:
            self.keep = getattr(self, "keep", []) + [t]
        return C.c_void_p(t.data_ptr())

    def back(self):
        if self.mem == "device":
            import torch

            torch.cuda.synchronize()
            for a, t in self.pairs:
                if a.size:
                    a.view(np.uint8).reshape(-1)[:] = t.cpu().numpy()

    @property
    def kind(self):
        from tamp_amd import _lib

        return _lib.MEM_HOST if self.mem == "host" else _lib.MEM_DEVICE


def aligned_rows(rows, stride, fill=ROW_FILL):
    from tamp_amd.batch import _aligned_rows

    a = _aligned_rows(max(rows, 1), stride)
    a[...] = fill
    return a


def index_call(blobs, N, w, room, *, mem="host", dictionary=None):
    """tamp_batch_seek_index with `room[i]` rows for stream i -> (rc, size, status, first, in_pos, state): rows behind ROW_FILL."""
    from tamp_amd import _lib

    lib = _lib.load()
    flat, off, length = _pack(blobs)
    n = len(blobs)
    first = np.zeros(n + 1, dtype=np.uint64)
    first[1:] = np.cumsum(np.asarray(room, dtype=np.uint64))
    total, stride = int(first[-1]), 16 + (1 << w)
    in_pos = np.full(max(total, 1), 0xEEEEEEEE, dtype=np.uint32)
    state = aligned_rows(total, stride)
    size = np.full(n, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    status = np.full(n, 0x77, dtype=np.int8)
    d = None if dictionary is None else np.frombuffer(bytes(dictionary), dtype=np.uint8).copy()
    m = _Mem(mem)
    rc = lib.tamp_batch_seek_index(m(d), 0 if d is None else len(d), w, m(flat), m(off), m(length), N, m(first), m(in_pos), m(state), stride,
                                   m(size), m(status), n, m.kind, 0, None)
    m.back()
    return rc, size, status, first, in_pos[:total], state[:total]


def read_call(blobs, N, w, first, in_pos, state, ranges, *, mem="host", dictionary=None):
    """tamp_batch_read_ranges_seek, every range's room laid out behind guards -> (rc, out_len, status, [bytes in the room], clean):
    clean = every byte of the buffer outside the delivered ones still holds the guard."""
    from tamp_amd import _lib

    lib = _lib.load()
    flat, off, length = _pack(blobs)
    nr = len(ranges)
    r_stream = np.array([r[0] for r in ranges], dtype=np.uint32)
    r_begin = np.array([r[1] for r in ranges], dtype=np.uint64)
    r_len = np.array([r[2] for r in ranges], dtype=np.uint32)
    out_off = np.zeros(nr, dtype=np.uint64)
    at = GAP
    for q in range(nr):
        out_off[q] = at
        at += int(r_len[q]) + GAP + (q % 4)  # (all four residues mod 4)
    out = np.full(at + 16, GUARD, dtype=np.uint8)
    out_len = np.full(nr, 0xEEEEEEEE, dtype=np.uint32)
    status = np.full(nr, 0x77, dtype=np.int8)
    d = None if dictionary is None else np.frombuffer(bytes(dictionary), dtype=np.uint8).copy()
    stride = 16 + (1 << w)
    st = state if len(state) else aligned_rows(0, stride)
    ip = in_pos if len(in_pos) else np.zeros(1, np.uint32)
    m = _Mem(mem)
    rc = lib.tamp_batch_read_ranges_seek(m(d), 0 if d is None else len(d), w, m(flat), m(off), m(length), N, m(np.ascontiguousarray(first)),
                                         m(np.ascontiguousarray(ip)), m(st), stride, m(r_stream), m(r_begin), m(r_len), m(out), m(out_off),
                                         m(out_len), m(status), len(blobs), nr, m.kind, 0, None)
    m.back()
    got, mask = [], np.ones(len(out), dtype=bool)
    for q in range(nr):
        o, k = int(out_off[q]), min(int(out_len[q]), int(r_len[q]))
        got.append(out[o : o + k].tobytes())
        mask[o : o + k] = False
    clean = bool((out[mask] == GUARD).all()) and bool((out_len <= r_len).all())
    return rc, out_len, status, got, clean


def full_index(oracle, blobs, N, w, *, mem="host", dictionary=None):
    sizes = [len(oracle.decompress(b, dictionary=dictionary, max_window_bits=w)[1]) if len(b) else 0 for b in blobs]
    room = [(s - 1) // N if s else 0 for s in sizes]
    return index_call(blobs, N, w, room, mem=mem, dictionary=dictionary), sizes, room


def assert_rows(oracle, stream, rows, in_pos, state, w, *, restart_with=None):
    """The GPU's rows of one stream against the oracle's, field by field."""
    assert len(rows) == len(in_pos) == len(state)
    W = 1 << (((stream[0] >> 5) & 7) + 8)
    for k, row in enumerate(rows):
        g = si.Dec.from_buffer_copy(state[k, :16].tobytes())
        e = row["state"]
        where = f"row {k}"
        assert int(in_pos[k]) == row["in_pos"], where
        assert state[k, 16 : 16 + W].tobytes() == row["window"][:W].tobytes(), where
        for f in ("window_pos", "token_state", "skip_bytes", "bit_buffer_pos", "conf", "flags", "window_bits_max"):
            assert int(getattr(g, f)) == e[f], (where, f)
        nb = e["bit_buffer_pos"]
        assert (g.bit_buffer >> (32 - nb) if nb else 0) == (e["bit_buffer"] >> (32 - nb) if nb else 0), where
        if e["token_state"] or e["skip_bytes"]:
            assert (g.pending_window_offset, g.pending_match_size) == (e["pending_window_offset"], e["pending_match_size"]), where
        if restart_with is not None:
            src, N = restart_with
            r, rest = si.restart(oracle, stream, si.state_dict(g), state[k, 16 : 16 + W].tobytes(), int(in_pos[k]), len(src) + 16)
            assert r == INPUT_EXHAUSTED and rest == src[(k + 1) * N :], where


# ---- 1. checkpoints against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=[cs.case_id(*c) for c in cs.CONFIGS])
def test_checkpoints_equal_the_oracles(ta, oracle, window, extended, mem):
    src, stream = si.cut_sweep_stream(oracle, window, extended)
    classes = set()
    for N in (64, 1000) if window == 15 else (1, 3, 64, 241, 1000, 4096):
        rows, S, _, _ = si.expected_checkpoints(oracle, stream, N, window_bits=window)
        (rc, size, status, first, in_pos, state), sizes, room = full_index(oracle, [stream], N, window, mem=mem)
        assert rc == 0 and int(size[0]) == S == len(src) and int(status[0]) == INPUT_EXHAUSTED
        assert room[0] == len(rows)
        assert_rows(oracle, stream, rows, in_pos, state, window, restart_with=(src, N))
        classes |= {si.checkpoint_class(si.state_dict(si.Dec.from_buffer_copy(state[k, :16].tobytes()))) for k in range(len(rows))}
    if window != 15:
        assert classes == ({"boundary", "match", "rle", "ext"} if extended else {"boundary", "match"})


# ---- 2. every begin, in one call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,mem", [(64, "host"), (64, "device"), (1, "device")])
@pytest.mark.parametrize("window,extended", cs.CONFIGS, ids=[cs.case_id(*c) for c in cs.CONFIGS])
def test_every_begin_in_one_call(ta, oracle, window, extended, N, mem):
    src, stream = si.cut_sweep_stream(oracle, window, extended)
    S = len(src)
    (rc, size, status, first, in_pos, state), _, _ = full_index(oracle, [stream], N, window, mem="device")
    assert rc == 0 and int(size[0]) == S
    ranges = [(0, b, n) for b in range(S + 3) for n in (0, 1, 5, 63, 64, 65, 200, S)]
    rc, out_len, st, got, clean = read_call([stream], N, window, first, in_pos, state, ranges, mem=mem)
    assert rc == 0 and clean
    for q, (_, b, n) in enumerate(ranges):
        want = src[b : b + n]
        assert got[q] == want and int(out_len[q]) == len(want), (b, n)
        assert int(st[q]) == (OK if len(want) == n else INPUT_EXHAUSTED), (b, n)


# ---- 3. the ragged batch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS)
def test_ragged_batch(ta, oracle, mem):
    N, w = 100, 12
    batch = si.ragged_batch(oracle)
    names = [b[0] for b in batch]
    blobs = [b[1] for b in batch]
    dictionary = next(b[2] for b in batch if b[2] is not None)
    decoded = []
    for name, blob, d in batch:
        r, data, _ = oracle.decompress(blob, dictionary=d, max_window_bits=w) if len(blob) else (INPUT_EXHAUSTED, b"", 0)
        decoded.append((r, data))
    assert decoded[names.index("oob")][0] == OOB and decoded[names.index("cut-in-token")][0] == INPUT_EXHAUSTED
    assert {len(decoded[names.index(f"len{n}")][1]) for n in (0, 1, 99, 100, 101, 200, 201)} == {0, 1, 99, 100, 101, 200, 201}
    room = [(len(d) - 1) // N if len(d) else 0 for _, d in decoded]
    rc, size, status, first, in_pos, state = index_call(blobs, N, w, room, mem=mem, dictionary=dictionary)
    assert rc == 0
    for i, (r, data) in enumerate(decoded):
        assert (int(size[i]), int(status[i])) == (len(data), r), names[i]
        rows, S, _, _ = si.expected_checkpoints(oracle, blobs[i], N, window_bits=w, dictionary=batch[i][2]) if len(blobs[i]) else ([], 0, 0, 0)
        assert S == len(data) and len(rows) == room[i], names[i]
        f0, f1 = int(first[i]), int(first[i + 1])
        if rows:
            assert_rows(oracle, blobs[i], rows, in_pos[f0:f1], state[f0:f1], w)
    ranges = []
    for i, (r, data) in enumerate(decoded):
        ranges.append((i, 0, len(data) + 4))
        for k in range(room[i] + 2):
            ranges += [(i, max(k * N - 3, 0), 7), (i, k * N, N), (i, k * N + 1, 2 * N)]
    rc, out_len, st, got, clean = read_call(blobs, N, w, first, in_pos, state, ranges, mem=mem, dictionary=dictionary)
    assert rc == 0 and clean
    for q, (i, b, n) in enumerate(ranges):
        r, data = decoded[i]
        want = data[b : b + n]
        assert got[q] == want, (names[i], b, n)
        if len(want) == n:
            assert int(st[q]) == OK, (names[i], b, n)
        else:  # the stream ended first: as it ends -- an offset out of the window stays TAMP_OOB, behind the bytes in front of it
            assert int(st[q]) == (OOB if r == OOB else INPUT_EXHAUSTED), (names[i], b, n)


# ---- 4. short room -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS)
def test_short_room_then_a_second_call(ta, oracle, mem):
    N, w = 64, 10
    pairs = [si.cut_sweep_stream(oracle, 10, True), si.cut_sweep_stream(oracle, 8, False), si.cut_sweep_stream(oracle, 10, False)]
    blobs = [p[1] for p in pairs]
    expect = [si.expected_checkpoints(oracle, b, N, window_bits=w)[0] for b in blobs]
    C_ = [len(e) for e in expect]
    room = [C_[0] - 2, 0, C_[2] + 3]  # too little, none, more than there are
    rc, size, status, first, in_pos, state = index_call(blobs, N, w, room, mem=mem)
    assert rc == 0
    for i in range(3):
        S = int(size[i])
        assert S == len(pairs[i][0]) and (S - 1) // N == C_[i] and int(status[i]) == INPUT_EXHAUSTED  # (the size still tells C)
        f0, wrote = int(first[i]), min(room[i], C_[i])
        assert_rows(oracle, blobs[i], expect[i][:wrote], in_pos[f0 : f0 + wrote], state[f0 : f0 + wrote], w)
        f1 = int(first[i + 1])
        assert (state[f0 + wrote : f1] == ROW_FILL).all() and (in_pos[f0 + wrote : f1] == 0xEEEEEEEE).all(), i  # only the rows given
    room2 = [(int(s) - 1) // N for s in size]
    rc, size2, status2, first2, in_pos2, state2 = index_call(blobs, N, w, room2, mem=mem)
    assert rc == 0 and (size2 == size).all()
    for i in range(3):
        f0, f1 = int(first2[i]), int(first2[i + 1])
        assert_rows(oracle, blobs[i], expect[i], in_pos2[f0:f1], state2[f0:f1], w)
    # and a short index still reads: the last row serves what lies behind it
    ranges = [(0, b, 90) for b in range(0, len(pairs[0][0]), 37)] + [(1, 5, 2000)]
    rc, out_len, st, got, clean = read_call(blobs, N, w, first, in_pos, state, ranges, mem=mem)
    assert rc == 0 and clean
    for q, (i, b, n) in enumerate(ranges):
        assert got[q] == pairs[i][0][b : b + n], (i, b)


# ---- 5. forged rows -------------------------------------------------------------------------------------------------------------
FORGERIES = ("conf", "flag", "token_state", "window_pos", "in_pos beyond", "in_pos below")


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("forgery", FORGERIES)
def test_forged_rows(ta, oracle, forgery, mem):
    N, w = 64, 10
    pairs = [si.cut_sweep_stream(oracle, 10, True), si.cut_sweep_stream(oracle, 10, False), si.cut_sweep_stream(oracle, 8, True)]
    blobs = [p[1] for p in pairs]
    (rc, size, status, first, in_pos, state), _, room = full_index(oracle, blobs, N, w, mem="device")
    assert rc == 0
    victim, r = 1, 5  # row 5 of stream 1 = its checkpoint 6
    row = int(first[victim]) + r
    in_pos, state = in_pos.copy(), state.copy()
    g = si.Dec.from_buffer_copy(state[row, :16].tobytes())
    if forgery == "conf":
        g.conf ^= 0x20
    elif forgery == "flag":
        g.flags &= ~1
    elif forgery == "token_state":
        g.token_state = 7
    elif forgery == "window_pos":
        g.window_pos = 1 << 10
    elif forgery == "in_pos beyond":
        in_pos[row] = len(blobs[victim]) + 1
    else:
        in_pos[row] = in_pos[row - 1] - 1
    state[row, :16] = np.frombuffer(bytes(g), dtype=np.uint8)
    ranges = []
    for i, (src, _) in enumerate(pairs):
        for k in range(room[i] + 1):
            ranges += [(i, k * N + 3, 10), (i, max(k * N - 5, 0), 10), (i, k * N + 60, N + 10)]
        ranges.append((i, 0, len(src)))
    rc, out_len, st, got, clean = read_call(blobs, N, w, first, in_pos, state, ranges, mem=mem)
    assert rc == 0 and clean  # (nothing is written outside out_len)
    touched = 0
    for q, (i, b, n) in enumerate(ranges):
        src = pairs[i][0]
        end = min(b + n, len(src))
        units = range(b // N, (end - 1) // N + 1)
        if i == victim and (r + 1) in units:  # a unit of the range starts at the forged row
            assert (int(st[q]), int(out_len[q])) == (BAD_INDEX, 0), (b, n)
            touched += 1
        else:
            assert got[q] == src[b : b + n] and int(st[q]) == (OK if b + n <= len(src) else INPUT_EXHAUSTED), (i, b, n)
    assert touched >= 4


# ---- 6. long ranges and real text -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prose300():
    from tamp_amd import workloads as wl

    raw = wl.frozen_corpus("prose")
    assert len(raw) >= 400_000, "the frozen corpus (tests/golden/corpus_prose.txt.xz) is part of the tree"
    return raw[50_000:350_000]


@pytest.mark.parametrize("window,N", [(10, 4096), (12, 65536)])
def test_long_ranges_and_real_text(ta, oracle, prose300, window, N, tmp_path):
    import torch

    data = prose300
    rc, stream = oracle.compress(data, window=window)
    assert rc == OK
    rng = random.Random(window)
    ranges = [(rng.randrange(len(data)), rng.randint(1, 20_000)) for _ in range(200)] + [(0, len(data))]
    begin, length = [r[0] for r in ranges], [r[1] for r in ranges]

    def check(res):
        out_len = np.asarray(res.out_len.cpu() if hasattr(res.out_len, "cpu") else res.out_len).astype(np.int64) & 0xFFFFFFFF
        status = np.asarray(res.status.cpu() if hasattr(res.status, "cpu") else res.status)
        for q, (b, n) in enumerate(ranges):
            want = data[b : b + n]
            assert res.range(q) == want and int(out_len[q]) == len(want), (b, n)
            assert int(status[q]) == (OK if len(want) == n else INPUT_EXHAUSTED), (b, n)

    flat = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    in_off, in_len = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.tensor([len(stream)], dtype=torch.int32, device="cuda")
    index = ta.build_seek_index(flat, in_off, in_len, interval=N, max_window_bits=window)
    assert int(index.size[0]) == len(data) and len(index.in_pos) == (len(data) - 1) // N
    check(ta.read_ranges_seek(flat, in_off, in_len, seek_index=index, stream_index=[0] * len(ranges), begin=begin, length=length))
    # through a file, and through the host-memory call
    path = str(tmp_path / "index.npz")
    index.save(path)
    loaded = ta.SeekIndex.load(path)
    assert loaded.nbytes == index.nbytes and (loaded.interval, loaded.window_bits) == (N, window)
    check(ta.read_ranges_seek([stream], seek_index=loaded, stream_index=[0] * len(ranges), begin=begin, length=length))
    host = ta.build_seek_index([stream], interval=N)
    assert host.window_bits == window and np.array_equal(host.in_pos, loaded.in_pos) and np.array_equal(host.state, loaded.state)
    check(ta.read_ranges_seek(flat, in_off, in_len, seek_index=loaded.to("cuda"), stream_index=[0] * len(ranges), begin=begin, length=length))
