"""GPU tier: extending a seek index when its streams have grown (tamp_batch_seek_index_extend, ``extend_seek_index`` /
``SeekIndex.extend``; tamp_seek_extend_kernel of tamp_seek_kernel.hpp).

Every expectation comes from the oracle's decoder object (tests/seek_index_input.py's ``expected_checkpoints``: of the old bytes for
the rows a stream holds, of the grown stream for the result) or is a slice of the ORIGINAL input, never a GPU result.  The C entry
is called directly, from both memory kinds, with the tables behind 0xEE fill as in tests/test_gpu_seek_index.py."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seek_extend_input as se  # noqa: E402
import seek_index_input as si  # noqa: E402
from seek_index_input import BAD_INDEX, INPUT_EXHAUSTED, OK, OOB  # noqa: E402
from test_gpu_seek_index import FORGERIES, MEMS, ROW_FILL, _Mem, _pack, aligned_rows, assert_rows, read_call  # noqa: E402

pytestmark = pytest.mark.gpu

IN_FILL = 0xEEEEEEEE


@pytest.fixture(scope="module")
def ta():
    import tamp_amd
    from tamp_amd import _lib

    _lib.load()  # raises if the native library is missing: no silent fallback
    return tamp_amd


def tables(room, w):
    """-> (first, in_pos, state) for `room[i]` rows per stream, all fill."""
    first = np.zeros(len(room) + 1, dtype=np.uint64)
    first[1:] = np.cumsum(np.asarray(room, dtype=np.uint64))
    total = int(first[-1])
    return first, np.full(max(total, 1), IN_FILL, dtype=np.uint32), aligned_rows(total, 16 + (1 << w))


def extend_call(blobs, N, w, first, have, in_pos, state, *, mem="host", dictionary=None):
    """tamp_batch_seek_index_extend on tables the test filled -> (rc, size, status); in_pos and state hold the result."""
    from tamp_amd import _lib

    lib = _lib.load()
    flat, off, length = _pack(blobs)
    n = len(blobs)
    size = np.full(n, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    status = np.full(n, 0x77, dtype=np.int8)
    have = np.asarray(have, dtype=np.uint32)
    d = None if dictionary is None else np.frombuffer(bytes(dictionary), dtype=np.uint8).copy()
    first = np.ascontiguousarray(first)
    first.flags.writeable = have.flags.writeable = False  # (only read: not copied back)
    m = _Mem(mem)
    rc = lib.tamp_batch_seek_index_extend(m(d), 0 if d is None else len(d), w, m(flat), m(off), m(length), N, m(first), m(have), m(in_pos),
                                          m(state), 16 + (1 << w), m(size), m(status), n, m.kind, 0, None)
    m.back()
    return rc, size, status


def fill_intact(in_pos, state, a, b):
    return bool((state[a:b] == ROW_FILL).all()) and bool((in_pos[a:b] == IN_FILL).all())


# ---- 1. the cut sweep as one batch ---------------------------------------------------------------------------------------------
SWEEPS = [(10, True, 64, 1), (10, True, 241, 1), (10, False, 64, 1), (10, False, 241, 1), (8, True, 64, 1), (8, True, 241, 1),
          (8, False, 64, 1), (8, False, 241, 1), (15, True, 64, 10), (8, True, 1, 13)]


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("window,extended,N,step", SWEEPS, ids=[f"w{w}-{'ext' if e else 'v1'}-N{N}" for w, e, N, _ in SWEEPS])
def test_cut_sweep_as_one_batch(ta, oracle, window, extended, N, step, mem):
    """Stream i of the old batch is whole[:c]; every slot of the grown batch is `whole`.  One call must leave the whole stream's
    rows in every slot, whatever row the stream had to restart at."""
    src, whole, want = se.whole_rows(oracle, window, extended, N)
    cuts = se.cut_rows(oracle, window, extended, N, step)
    cs_ = sorted(cuts)
    n, C_ = len(cs_), len(want)
    assert n <= 691 and C_ == (len(src) - 1) // N
    room = [C_ + (i % 2) for i in range(n)]  # (every other stream: a row of room behind its last one)
    first, in_pos, state = tables(room, window)
    have, classes, dropped = [], set(), []
    for i, c in enumerate(cs_):
        rows = cuts[c]
        se.place_rows(rows, in_pos, state, int(first[i]))
        have.append(len(rows))
        final = se.restart_rows([r["in_pos"] for r in rows])
        dropped.append(len(rows) - final)
        if final:
            classes.add(si.checkpoint_class(rows[final - 1]["state"]))
    rc, size, status = extend_call([whole] * n, N, window, first, have, in_pos, state, mem=mem)
    assert rc == 0
    f0 = int(first[0])
    assert_rows(oracle, whole, want, in_pos[f0 : f0 + C_], state[f0 : f0 + C_], window)
    same_in, same_state = in_pos[f0 : f0 + C_].copy(), state[f0 : f0 + C_].copy()
    for i, c in enumerate(cs_):
        f0, f1 = int(first[i]), int(first[i + 1])
        assert (int(size[i]), int(status[i])) == (len(src), INPUT_EXHAUSTED), c
        if not (np.array_equal(in_pos[f0 : f0 + C_], same_in) and np.array_equal(state[f0 : f0 + C_], same_state)):  # (else: checked above)
            assert_rows(oracle, whole, want, in_pos[f0 : f0 + C_], state[f0 : f0 + C_], window)
        assert fill_intact(in_pos, state, f0 + C_, f1), c
    if N == 64 and step == 1:  # the restart rows actually used, and cuts that cost more than the last row
        assert classes == ({"boundary", "match", "rle", "ext"} if extended else {"boundary", "match"})
        # (from the oracle, tests/test_seek_extend_host.py: the v1 streams never lose more than their last row)
        assert (max(dropped), sum(d > 1 for d in dropped)) == {(10, True): (3, 37), (8, True): (3, 35)}.get((window, extended), (1, 0))
    if N == 1:
        assert max(dropped) == 258  # (the rows of a run share one in_pos)


# ---- 2. the ragged batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS)
def test_ragged_batch(ta, oracle, mem):
    N, w = 100, 12
    batch = si.ragged_batch(oracle)
    # (the stream with the custom dictionary and the unchanged one first: old streams, entered at a restart row)
    batch.sort(key=lambda b: b[0] not in ("custom", "w12-v1"))
    names = [b[0] for b in batch]
    blobs = [b[1] for b in batch]
    dictionary = next(b[2] for b in batch if b[2] is not None)
    n, n_old = len(batch), len(batch) - 3  # the last three streams are new
    assert names[n_old:] == ["w8-ext", "w12-ext", "scripted"] and {"oob", "cut-in-token", "custom"} <= set(names[:n_old])
    old = [blob[: len(blob) * 2 // 3] for blob in blobs[:n_old]]
    old[names.index("w12-v1")] = blobs[names.index("w12-v1")]  # unchanged
    old[names.index("len101")] = blobs[names.index("len101")][:1]  # from its header alone
    old[names.index("len100")] = b""  # from nothing
    decoded, want = [], []
    for name, blob, d in batch:
        r, data, _ = oracle.decompress(blob, dictionary=d, max_window_bits=w) if len(blob) else (INPUT_EXHAUSTED, b"", 0)
        decoded.append((r, data))
        want.append(se.slim(si.expected_checkpoints(oracle, blob, N, window_bits=w, dictionary=d)[0], 15) if len(blob) else [])
    room = [len(rows) for rows in want]
    assert room == [(len(d) - 1) // N if len(d) else 0 for _, d in decoded]
    first, in_pos, state = tables(room, w)
    have = [0] * n
    for i in range(n_old):
        rows = se.slim(si.expected_checkpoints(oracle, old[i], N, window_bits=w, dictionary=batch[i][2])[0], w) if len(old[i]) else []
        se.place_rows(rows, in_pos, state, int(first[i]))
        have[i] = len(rows)
    assert sum(1 for h in have if h) >= 5 and have[names.index("w12-v1")] == room[names.index("w12-v1")] > 0
    custom = names.index("custom")
    assert have[custom] >= 2 and se.restart_rows(in_pos[int(first[custom]) : int(first[custom]) + have[custom]]) >= 1
    rc, size, status = extend_call(blobs, N, w, first, have, in_pos, state, mem=mem, dictionary=dictionary)
    assert rc == 0
    for i, (r, data) in enumerate(decoded):
        assert (int(size[i]), int(status[i])) == (len(data), r), names[i]
        f0, f1 = int(first[i]), int(first[i + 1])
        if want[i]:
            assert_rows(oracle, blobs[i], want[i], in_pos[f0:f1], state[f0:f1], w)
    ranges = []
    for i, (r, data) in enumerate(decoded):
        ranges.append((i, 0, len(data) + 4))
        for k in range(room[i] + 2):
            ranges += [(i, max(k * N - 3, 0), 7), (i, k * N + 1, 2 * N)]
    total = int(first[-1])
    rc, out_len, st, got, clean = read_call(blobs, N, w, first, in_pos[:total], state[:total], ranges, mem=mem, dictionary=dictionary)
    assert rc == 0 and clean
    for q, (i, b, k) in enumerate(ranges):
        r, data = decoded[i]
        assert got[q] == data[b : b + k], (names[i], b, k)
        assert int(st[q]) == (OK if len(data[b : b + k]) == k else (OOB if r == OOB else INPUT_EXHAUSTED)), (names[i], b, k)


# ---- 3. room -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS)
def test_room_then_a_second_call(ta, oracle, mem):
    N, w = 64, 10
    configs = [(10, True), (8, False), (10, False)]
    whole = [se.whole_rows(oracle, *c, N) for c in configs]
    blobs = [x[1] for x in whole]
    want = [se.slim(si.expected_checkpoints(oracle, b, N, window_bits=w)[0], 15) for b in blobs]  # (rows of the call's window size)
    old = [se.slim(si.expected_checkpoints(oracle, b[: len(b) // 2], N, window_bits=w)[0], w) for b in blobs]
    C_, have = [len(x) for x in want], [len(x) for x in old]
    assert all(2 <= h < c - 3 for h, c in zip(have, C_))
    room = [C_[0] - 2, have[1], C_[2] + 3]  # too little, exactly the rows it holds, more than there are
    first, in_pos, state = tables(room, w)
    for i in range(3):
        se.place_rows(old[i], in_pos, state, int(first[i]))
    rc, size, status = extend_call(blobs, N, w, first, have, in_pos, state, mem=mem)
    assert rc == 0
    for i in range(3):
        S = int(size[i])
        assert S == len(whole[i][0]) and (S - 1) // N == C_[i] and int(status[i]) == INPUT_EXHAUSTED  # (the size still tells C)
        f0, f1, wrote = int(first[i]), int(first[i + 1]), min(room[i], C_[i])
        assert_rows(oracle, blobs[i], want[i][:wrote], in_pos[f0 : f0 + wrote], state[f0 : f0 + wrote], w)
        assert fill_intact(in_pos, state, f0 + wrote, f1), i  # only the rows given
    # sized from decoded_size, with the rows the first call left
    room2 = [(int(s) - 1) // N for s in size]
    have2 = [min(r, c) for r, c in zip(room, C_)]
    first2, in_pos2, state2 = tables(room2, w)
    for i in range(3):
        a, b = int(first[i]), int(first2[i])
        in_pos2[b : b + have2[i]], state2[b : b + have2[i]] = in_pos[a : a + have2[i]], state[a : a + have2[i]]
    rc, size2, status2 = extend_call(blobs, N, w, first2, have2, in_pos2, state2, mem=mem)
    assert rc == 0 and (size2 == size).all() and (status2 == status).all()
    for i in range(3):
        f0, f1 = int(first2[i]), int(first2[i + 1])
        assert_rows(oracle, blobs[i], want[i], in_pos2[f0:f1], state2[f0:f1], w)


# ---- 4. a forged restart row ------------------------------------------------------------------------------------------------------
def _forge(forgery, in_pos, state, row, beyond):
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
        in_pos[row] = beyond
    else:
        in_pos[row] = in_pos[row - 1] - 1
    state[row, :16] = np.frombuffer(bytes(g), dtype=np.uint8)


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("which", ("restart row", "last row"))
@pytest.mark.parametrize("forgery", FORGERIES)
def test_forged_restart_row(ta, oracle, forgery, which, mem):
    N, w = 64, 10
    configs = [(10, True), (10, False), (8, True)]
    whole = [se.whole_rows(oracle, *c, N) for c in configs]
    blobs = [x[1] for x in whole]
    want = [se.slim(si.expected_checkpoints(oracle, b, N, window_bits=w)[0], 15) for b in blobs]
    victim = 1
    # the victim's old bytes: the first cut behind the middle that costs exactly its last row, with two final rows at least
    cuts = se.cut_rows(oracle, *configs[victim], N)
    c = next(c for c in sorted(cuts) if c > len(blobs[victim]) // 2 and len(cuts[c]) >= 3
             and se.restart_rows([r["in_pos"] for r in cuts[c]]) == len(cuts[c]) - 1)
    cut = [len(blobs[0]) // 2, c, len(blobs[2]) * 2 // 3]
    old = [se.slim(si.expected_checkpoints(oracle, b[:k], N, window_bits=w)[0], w) for b, k in zip(blobs, cut)]
    have, room = [len(x) for x in old], [len(x) for x in want]
    first, in_pos, state = tables(room, w)
    for i in range(3):
        se.place_rows(old[i], in_pos, state, int(first[i]))
    final = se.restart_rows([r["in_pos"] for r in old[victim]])
    assert final == have[victim] - 1 >= 2
    row = int(first[victim]) + (final - 1 if which == "restart row" else have[victim] - 1)
    _forge(forgery, in_pos, state, row, len(blobs[victim]) + 1)
    f0, f1 = int(first[victim]), int(first[victim + 1])
    before_in, before_state = in_pos[f0:f1].copy(), state[f0:f1].copy()
    rc, size, status = extend_call(blobs, N, w, first, have, in_pos, state, mem=mem)
    assert rc == 0
    for i in range(3):
        a, b = int(first[i]), int(first[i + 1])
        if i == victim and which == "restart row":
            assert (int(status[i]), int(size[i])) == (BAD_INDEX, 0)
            assert np.array_equal(in_pos[a:b], before_in) and np.array_equal(state[a:b], before_state)  # untouched, byte for byte
        else:  # (a forged last row is not the restart row: it is decoded again)
            assert (int(size[i]), int(status[i])) == (len(whole[i][0]), INPUT_EXHAUSTED), i
            assert_rows(oracle, blobs[i], want[i], in_pos[a:b], state[a:b], w)


# ---- 5. the Python surface ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prose300():
    from tamp_amd import workloads as wl

    raw = wl.frozen_corpus("prose")
    assert len(raw) >= 400_000, "the frozen corpus (tests/golden/corpus_prose.txt.xz) is part of the tree"
    return raw[50_000:350_000]


def _same_index(a, b):
    """Two indexes on either memory kind: every table equal."""
    assert (a.interval, a.window_bits) == (b.interval, b.window_bits)
    for f in ("first", "in_pos", "state", "size", "status"):
        x, y = (np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t) for t in (getattr(a, f), getattr(b, f)))
        assert x.shape == y.shape and np.array_equal(x.astype(np.int64), y.astype(np.int64)), f


@pytest.mark.parametrize("window,N", [(10, 4096), (12, 65536)])
def test_python_surface(ta, oracle, prose300, window, N, tmp_path):
    import torch

    data = prose300
    rc, stream = oracle.compress(data, window=window)
    assert rc == OK
    # the stream as three messages of a connection would leave it: a prefix of the bytes at each step
    steps = [stream[: len(stream) // 3], stream[: len(stream) * 2 // 3], stream]
    rng = random.Random(window)
    ranges = [(rng.randrange(len(data)), rng.randint(1, 20_000)) for _ in range(200)]
    begin, length = [r[0] for r in ranges], [r[1] for r in ranges]

    def cuda(blob):
        flat = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        return flat, torch.zeros(1, dtype=torch.int64, device="cuda"), torch.tensor([len(blob)], dtype=torch.int32, device="cuda")

    def check_ranges(res):
        for q, (b, k) in enumerate(ranges):
            assert res.range(q) == data[b : b + k], (b, k)

    # CUDA tensors, against the device build
    index = ta.build_seek_index(*cuda(steps[0]), interval=N, max_window_bits=window)
    kept = [np.asarray(t.cpu().numpy()).copy() for t in (index.first, index.in_pos, index.state)]
    grown = index.extend(*cuda(steps[1]))
    for t, k in zip((index.first, index.in_pos, index.state), kept):
        assert np.array_equal(t.cpu().numpy(), k)  # the old index is not modified
    grown = ta.extend_seek_index(*cuda(steps[2]), seek_index=grown)
    _same_index(grown, ta.build_seek_index(*cuda(stream), interval=N, max_window_bits=window))
    check_ranges(ta.read_ranges_seek(*cuda(stream), seek_index=grown, stream_index=[0] * len(ranges), begin=begin, length=length))
    # host lists, once through a file, against the host build
    index = ta.build_seek_index([steps[0]], interval=N)
    assert index.window_bits == window
    kept = [np.array(t) for t in (index.first, index.in_pos, index.state)]
    path = str(tmp_path / "index.npz")
    index.extend([steps[1]]).save(path)
    for t, k in zip((index.first, index.in_pos, index.state), kept):
        assert np.array_equal(t, k)
    grown = ta.SeekIndex.load(path).extend([stream])
    _same_index(grown, ta.build_seek_index([stream], interval=N))
    check_ranges(ta.read_ranges_seek([stream], seek_index=grown, stream_index=[0] * len(ranges), begin=begin, length=length))
    # more streams than the index holds: the new one is built from its header
    two = grown.extend([stream, steps[1]])
    _same_index(two, ta.build_seek_index([stream, steps[1]], interval=N, max_window_bits=window))


# ---- 6. a live connection ------------------------------------------------------------------------------------------------------------
def test_live_connection(ta, prose300):
    n, window, rounds, N = 8, 10, 5, 512
    comp = ta.CompressorBatch(n, window=window)
    streams, sources = [b""] * n, [b""] * n
    index = None
    at = 0
    for rnd in range(rounds):
        messages = []
        for i in range(n):
            k = 900 + 37 * i + 11 * rnd  # about 1 KB each
            messages.append(prose300[at : at + k])
            at += k
        written, flushed = comp.write(messages), comp.flush()
        previous = [len(s) for s in sources]
        streams = [s + written.stream(i) + flushed.stream(i) for i, s in enumerate(streams)]
        sources = [s + m for s, m in zip(sources, messages)]
        index = ta.build_seek_index(streams, interval=N) if index is None else index.extend(streams)
        ranges = [(i, max(previous[i] - 300, 0), 700) for i in range(n)] + [(i, previous[i], 64) for i in range(n)]
        res = ta.read_ranges_seek(streams, seek_index=index, stream_index=[r[0] for r in ranges], begin=[r[1] for r in ranges],
                                  length=[r[2] for r in ranges])
        for q, (i, b, k) in enumerate(ranges):  # ranges that straddle the previous end
            assert res.range(q) == sources[i][b : b + k], (rnd, i)
    _same_index(index, ta.build_seek_index(streams, interval=N))
    assert all(int(s) == len(src) for s, src in zip(index.size, sources))
