"""GPU tier (-m gpu) of the streaming decoders that stay on the device: ``tamp_amd.DecompressorBatch``,
``tamp_batch_decompress_pieces`` and ``tamp_batch_decoded_size_pieces``.  Every comparison is bit-exact.

Two yardsticks, neither of them the code under test: the oracle's decoder object call by call (``Oracle.decode_script`` ->
status, bytes, consumed per call), and ``tamp_batch_decompress_resume`` on device memory for the 16 + W bytes an object holds
after a call (tests/test_gpu_parity.py and tests/test_gpu_cut_sweep.py pin that call to the reference).
"""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

import decompressor_batch_input as di  # noqa: E402

NAMES = ("text-w8", "text-w10", "text-w15", "run300-w10", "two-resets-w10", "custom-dictionary-w10", "literal7-w10", "v1-w10",
         "two-byte-header-w10", "oob-w8", "header-above-window-bits")
OK, OUTPUT_FULL, INPUT_EXHAUSTED = 0, 1, 2
GUARD, GAP = 0xA5, 24


@pytest.fixture(scope="module")
def all_streams(oracle):
    streams = di.streams(oracle)
    assert tuple(s.name for s in streams) == NAMES
    for s in streams:
        assert len(s.comp) > 64 and (s.plain is None or 100 <= len(s.plain) <= 400), s.name
    return {s.name: s for s in streams}


class Harness:
    def __init__(self):
        import torch

        import tamp_amd
        from tamp_amd import _lib

        self.torch, self.tamp, self._lib, self.lib = torch, tamp_amd, _lib, _lib.load()
        self.dev = torch.device("cuda:0")

    def up(self, a):
        return self.torch.from_numpy(np.array(a)).to(self.dev)  # (a copy: packed chunks are read-only views of a bytes object)

    def pieces(self, chunks):
        """-> (flat, in_off, in_len) on the device."""
        flat, off, ln = self.tamp.pack_streams(chunks)
        return self.up(flat if flat.size else np.zeros(16, np.uint8)), self.up(off.astype(np.int64)), self.up(ln.astype(np.int32))

    def resume(self, objects, bits, chunks, caps):
        """The yardstick: tamp_batch_decompress_resume on device memory, object r <- chunks[r] with caps[r] bytes of room.  `objects`
        (CUDA uint8 (n, stride)) is advanced in place.  -> (status, [bytes], consumed) on the host."""
        torch = self.torch
        n, stride = objects.shape
        assert objects.is_contiguous() and len(chunks) == n and len(caps) == n
        data, off, ln = self.pieces(chunks)
        cap = np.asarray(caps, dtype=np.int64)
        o_off = np.cumsum(cap) - cap
        out = torch.zeros(int(cap.sum()) + 1, dtype=torch.uint8, device=self.dev)
        out_len = torch.zeros(n, dtype=torch.int32, device=self.dev)
        status = torch.zeros(n, dtype=torch.int8, device=self.dev)
        consumed = torch.zeros(n, dtype=torch.int32, device=self.dev)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        cap_t, off_t = self.up(cap.astype(np.uint32).view(np.int32)), self.up(o_off)
        rc = self.lib.tamp_batch_decompress_resume(p(objects), stride, bits, p(data), p(off), p(ln), p(out), p(off_t), p(cap_t), p(out_len),
                                                   p(status), p(consumed), n, self._lib.MEM_DEVICE, 0, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        out_h, len_h = out.cpu().numpy(), out_len.cpu().numpy()
        return (status.cpu().numpy(), [out_h[int(o_off[r]) : int(o_off[r]) + int(len_h[r])].tobytes() for r in range(n)],
                consumed.cpu().numpy().astype(np.int64))

    def result(self, res):
        """A BatchResult's rows on the host: (status, [bytes], consumed)."""
        self.torch.cuda.synchronize()
        return res.status.cpu().numpy(), res.streams(), res.in_consumed.cpu().numpy().astype(np.int64)


@pytest.fixture(scope="module")
def h():
    return Harness()


def assert_rows(got, want, what):
    """got: (status, [bytes], consumed) arrays; want: [(status, bytes, consumed)] of the oracle."""
    status, outs, consumed = got
    assert len(outs) == len(want)
    for r, (ws, wb, wk) in enumerate(want):
        assert (int(status[r]), outs[r], int(consumed[r])) == (ws, wb, wk), f"{what}: row {r}"


# ---- 1. every cut -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_cut(name, h, oracle, all_streams):
    """One object per cut of the stream, all in one batch: ``read`` piece 1, then ``read`` what it left, sizes found by the query."""
    s = all_streams[name]
    n = len(s.comp) + 1
    want = [di.two_piece_calls(oracle, s, c) for c in range(n)]
    d = h.tamp.DecompressorBatch(n, window_bits=s.window_bits, dictionary=s.dictionary)
    assert tuple(d.objects.shape) == (n, d.stride) and d.objects.is_cuda
    shadow = d.objects.clone()
    offered = [0] * n
    for call in range(2):
        chunks = [s.comp[offered[c] : c] if call == 0 else s.comp[offered[c] :] for c in range(n)]
        res = d.read(chunks)
        got = h.result(res)
        assert_rows(got, [w[call] for w in want], f"{name}, call {call + 1}")
        assert len(res.out_len) == n
        # the object a call leaves: tamp_batch_decompress_resume with the same input and the room `read` gave it (size + 1)
        ref = h.resume(shadow, s.window_bits, chunks, [len(b) + 1 for b in got[1]])
        assert (ref[0] == got[0]).all() and ref[1] == got[1] and (ref[2] == got[2]).all()
        assert h.torch.equal(shadow, d.objects), f"{name}, call {call + 1}: objects differ"
        offered = [offered[c] + int(got[2][c]) for c in range(n)]
    if s.plain is not None:
        assert all(w[0][1] + w[1][1] == s.plain for w in want)


# ---- 2. the size query against the decode, at every limit -----------------------------------------------------------------------
CLASSES = {
    "fresh object": lambda st: st["flags"] == 0,
    "first header byte stashed": lambda st: (st["flags"] & 2) != 0,
    "no carried bits": lambda st: (st["flags"] & 1) and st["nbits"] == 0 and st["ts"] == 0 and st["skip"] == 0 and st["consumed"] > 2,
    "1..7 carried bits": lambda st: st["ts"] == 0 and st["skip"] == 0 and 1 <= st["nbits"] <= 7,
    # (a call that ends for lack of input holds less than one token; only a full output leaves the buffer as a refill filled it)
    "more than 24 carried bits": lambda st: st["nbits"] > 24,
    "RLE run partly delivered": lambda st: st["ts"] == 1 and st["skip"] > 0,
    "extended match partly delivered": lambda st: st["ts"] == 3 and st["skip"] > 0,
    "extended match: size parked, offset to come": lambda st: st["ts"] == 3 and st["skip"] == 0,
    "RLE symbol starved of its payload": lambda st: st["ts"] == 1 and st["skip"] == 0,
    "extended-match symbol starved of its payload": lambda st: st["ts"] == 2 and st["skip"] == 0,
    "plain match partly delivered": lambda st: st["ts"] == 0 and st["skip"] > 0 and (st["flags"] & 1),
}


def test_size_query_equals_decode_at_every_limit(h, oracle, all_streams):
    torch, bits = h.torch, 10
    pool = [all_streams[k] for k in ("text-w10", "run300-w10", "two-resets-w10", "literal7-w10", "v1-w10", "two-byte-header-w10")]
    five = bytes(c & 0x1F for c in di.text())  # 6-bit literals: a token can leave 26 of 32 buffered bits
    rc, comp5 = oracle.compress(five, window=10, literal=5)
    assert rc == 0
    pool.append(di.Stream("literal5-w10", comp5, 10, five))
    # piece 1 of every stream at every cut, with ample room and with room that cuts a token short: one launch
    cands = [(s, c, cap) for s in pool for c in range(len(s.comp) + 1) for cap in (di.AMPLE, 1, 3, 20, 50, 100, 150)]
    objs = h.tamp.DecompressorBatch(len(cands), window_bits=bits).objects.clone()
    stride = objs.shape[1]
    _, _, consumed1 = h.resume(objs, bits, [s.comp[:c] for s, c, _ in cands], [cap for _, _, cap in cands])
    head = objs[:, :16].cpu().numpy()
    chosen = {}
    for i in range(len(cands)):
        st = dict(nbits=int(head[i, 6]), ts=int(head[i, 7]), skip=int(head[i, 13]), flags=int(head[i, 14]), consumed=int(consumed1[i]))
        for what, test in CLASSES.items():
            if what not in chosen and test(st):
                chosen[what] = i
    assert sorted(chosen) == sorted(CLASSES), f"no piece leaves: {sorted(set(CLASSES) - set(chosen))}"

    picks = list(chosen.values())
    sel = objs[torch.tensor(picks, device=h.dev)].clone()  # the objects mid-stream, one per class
    rest = [cands[i][0].comp[int(consumed1[i]) :] for i in picks]
    _, ample, _ = h.resume(sel.clone(), bits, rest, [di.AMPLE] * len(picks))
    rows = [(j, limit) for j in range(len(picks)) for limit in range(len(ample[j]) + 2)]  # limit = 0 .. size + 1
    assert len(rows) > 64
    row_obj = np.array([j for j, _ in rows], dtype=np.int32)
    limits = [limit for _, limit in rows]
    # the yardstick: every row on a copy of its object
    want = h.resume(sel[torch.from_numpy(row_obj.astype(np.int64)).to(h.dev)].clone(), bits, [rest[j] for j, _ in rows], limits)

    data, off, ln = h.pieces([rest[j] for j, _ in rows])
    R = len(rows)
    size = torch.full((R,), -1, dtype=torch.int32, device=h.dev)
    status = torch.full((R,), 0x5A, dtype=torch.int8, device=h.dev)
    consumed = torch.full((R,), -1, dtype=torch.int32, device=h.dev)
    before = sel.clone()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    index_t, limit_t = h.up(row_obj), h.up(np.array(limits, np.int32))  # (named: the launch is asynchronous)
    rc = h.lib.tamp_batch_decoded_size_pieces(p(sel), stride, bits, p(index_t), p(data), p(off), p(ln), p(limit_t), p(size), p(status),
                                              p(consumed), R, 0, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(sel, before), "the query wrote to an object"
    got = (status.cpu().numpy(), size.cpu().numpy(), consumed.cpu().numpy())
    names = list(chosen)
    for r, (j, limit) in enumerate(rows):
        assert (int(got[0][r]), int(got[1][r]), int(got[2][r])) == (int(want[0][r]), len(want[1][r]), int(want[2][r])), \
            f"{names[j]} (piece 1 = {cands[picks[j]][0].name}[:{cands[picks[j]][1]}] into {cands[picks[j]][2]}), limit {limit}"
    # no limit table, no index table, no consumed table: row r is object r with ample room
    data, off, ln = h.pieces(rest)
    rc = h.lib.tamp_batch_decoded_size_pieces(p(sel), stride, bits, None, p(data), p(off), p(ln), None, p(size), p(status), None,
                                              len(picks), 0, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert size.cpu().numpy()[: len(picks)].tolist() == [len(b) for b in ample]


# ---- 3. selection ---------------------------------------------------------------------------------------------------------------
def test_selected_objects_advance_and_the_others_are_untouched(h, oracle, all_streams):
    torch, bits, n = h.torch, 10, 70
    s = all_streams["text-w10"]
    rng = random.Random(7)
    named = rng.sample(range(n), 23)  # shuffled: rows and objects in different orders
    others = sorted(set(range(n)) - set(named))
    cuts = [5 + 8 * r for r in range(23)]
    want = [di.two_piece_calls(oracle, s, c) for c in cuts]
    objs = h.tamp.DecompressorBatch(n, window_bits=bits).objects.clone()
    stride = objs.shape[1]
    pattern = torch.arange(stride, device=h.dev).mul(37).add(11).to(torch.uint8)
    objs[torch.tensor(others, device=h.dev)] = pattern  # state AND window: an object no row names is not even read
    idx_t = torch.tensor(named, device=h.dev)
    index = h.up(np.array(named, dtype=np.int32))
    shadow = objs[idx_t].clone()
    G = 8  # guard rows in front of and behind the result rows
    offered = [0] * 23
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for call in range(2):
        chunks = [s.comp[: cuts[r]] if call == 0 else s.comp[offered[r] :] for r in range(23)]
        caps = [len(w[call][1]) + 1 for w in want]
        data, off, ln = h.pieces(chunks)
        o_off = np.cumsum([GAP + c for c in caps]) - np.array(caps)  # slab r behind GAP guard bytes
        total = int(o_off[-1]) + caps[-1] + GAP
        out = torch.full((total,), GUARD, dtype=torch.uint8, device=h.dev)
        out_len = torch.full((23 + 2 * G,), 0x7E7E7E7E, dtype=torch.int32, device=h.dev)
        status = torch.full((23 + 2 * G,), 0x5A, dtype=torch.int8, device=h.dev)
        consumed = torch.full((23 + 2 * G,), 0x7E7E7E7E, dtype=torch.int32, device=h.dev)
        off_t, cap_t = h.up(o_off.astype(np.int64)), h.up(np.array(caps, np.int32))  # (named: the launch is asynchronous)
        rc = h.lib.tamp_batch_decompress_pieces(p(objs), stride, bits, p(index), p(data), p(off), p(ln), p(out), p(off_t), p(cap_t),
                                                p(out_len[G:]), p(status[G:]), p(consumed[G:]), 23, 0, None)
        assert rc == 0
        torch.cuda.synchronize()
        out_h, len_h = out.cpu().numpy(), out_len.cpu().numpy()
        got = (status.cpu().numpy()[G : G + 23], [out_h[int(o_off[r]) : int(o_off[r]) + int(len_h[G + r])].tobytes() for r in range(23)],
               consumed.cpu().numpy()[G : G + 23].astype(np.int64))
        assert_rows(got, [w[call] for w in want], f"call {call + 1}")
        # guards: the rows around the tables, every byte outside the bytes written
        for t, v in ((out_len, 0x7E7E7E7E), (status, 0x5A), (consumed, 0x7E7E7E7E)):
            th = t.cpu().numpy()
            assert (th[:G] == v).all() and (th[G + 23 :] == v).all()
        mask = np.ones(total, dtype=bool)
        for r in range(23):
            mask[int(o_off[r]) : int(o_off[r]) + int(len_h[G + r])] = False
        assert (out_h[mask] == GUARD).all(), "bytes outside the slabs' written part"
        # the named objects: as tamp_batch_decompress_resume leaves them; the others: as they were
        ref = h.resume(shadow, bits, chunks, caps)
        assert ref[1] == got[1]
        assert torch.equal(objs[idx_t], shadow)
        assert bool((objs[torch.tensor(others, device=h.dev)] == pattern).all())
        offered = [offered[r] + int(got[2][r]) for r in range(23)]
    assert all(w[0][1] + w[1][1] == s.plain for w in want)


def test_none_chunks_take_no_part(h, oracle, all_streams):
    torch, n = h.torch, 70
    s = all_streams["run300-w10"]
    d = h.tamp.DecompressorBatch(n, window_bits=10)
    fresh = d.objects.clone()
    part = sorted(random.Random(3).sample(range(n), 23))
    cut = {i: 3 + 3 * k for k, i in enumerate(part)}
    want = {i: di.two_piece_calls(oracle, s, cut[i]) for i in part}
    res = d.read([s.comp[: cut[i]] if i in cut else None for i in range(n)])
    st, outs, consumed = h.result(res)
    off = res.out_off.cpu().numpy()
    for i in range(n):
        if i in cut:
            assert (int(st[i]), outs[i], int(consumed[i])) == want[i][0], i
        else:
            assert (int(st[i]), outs[i], int(consumed[i]), int(off[i])) == (0, b"", 0, 0), i
    idle = torch.tensor([i for i in range(n) if i not in cut], device=h.dev)
    assert torch.equal(d.objects[idle], fresh[idle])
    # nobody takes part: no launch, n rows of zeros
    res = d.read([None] * n)
    st, outs, consumed = h.result(res)
    assert not st.any() and not consumed.any() and outs == [b""] * n
    # the second piece, as CUDA tensors: in_len == 0 takes no part either, unless `which` names the stream
    rest = [s.comp[want[i][0][2] :] if i in cut else b"" for i in range(n)]
    data, off_t, len_t = h.pieces(rest)
    empty = part[0]
    assert cut[empty] == 3
    res = d.read(data, off_t, len_t * (torch.arange(n, device=h.dev) != empty), which=[empty])
    st, outs, consumed = h.result(res)
    for i in part:
        if i == empty:  # took part with no input: nothing to decode, nothing consumed
            assert (int(st[i]), outs[i], int(consumed[i])) == (INPUT_EXHAUSTED, b"", 0)
        else:
            assert (int(st[i]), outs[i], int(consumed[i])) == want[i][1], i
    assert torch.equal(d.objects[idle], fresh[idle])
    with pytest.raises(ValueError):
        d.read(data, off_t, len_t, which=[empty, empty])


# ---- 4. output cut short ----------------------------------------------------------------------------------------------------------
def test_output_cut_short_then_drained(h, oracle, all_streams):
    p = di.prose()
    tail_plain = p[1200:1240] + b"q" * 200  # the stream ends in an RLE token: a full output leaves it pending with all input consumed
    rc, tail_comp = oracle.compress(tail_plain, window=10)
    assert rc == 0
    tail = di.Stream("tail-run-w10", tail_comp, 10, tail_plain)
    jobs = []  # (stream, room of the first call)
    for s in [all_streams[k] for k in ("text-w10", "run300-w10", "two-resets-w10", "v1-w10")]:
        jobs += [(s, cap) for cap in (0, 1, 7, len(s.plain) - 1)]
    jobs += [(tail, 100), (tail, 239)]
    n = len(jobs)
    want = []
    for s, cap in jobs:
        first = di.expected_calls(oracle, s, [(len(s.comp), cap)])[0]
        rest = len(s.comp) - first[2]
        size2 = len(di.expected_calls(oracle, s, [(len(s.comp), cap), (rest, di.AMPLE)])[1][1])
        want.append(di.expected_calls(oracle, s, [(len(s.comp), cap), (rest, size2 + 1)]))
    assert all(w[0][0] == OUTPUT_FULL for w in want)
    assert want[-2][0][2] == len(tail.comp) and want[-1][0][2] == len(tail.comp)  # (what the tail stream is for)
    d = h.tamp.DecompressorBatch(n, window_bits=10)
    r1 = h.result(d.read([s.comp for s, _ in jobs], out_cap=[cap for _, cap in jobs]))
    assert_rows(r1, [w[0] for w in want], "first call")
    chunks = [s.comp[int(r1[2][i]) :] for i, (s, _) in enumerate(jobs)]
    assert chunks[-1] == b"" and chunks[-2] == b""
    r2 = h.result(d.read(chunks))
    assert_rows(r2, [w[1] for w in want], "second call")
    for i, (s, _) in enumerate(jobs):
        assert r1[1][i] + r2[1][i] == s.plain, i
    # out_cap as one int for every stream, and max_out: a stream above it stops there and is continued by a later read
    d = h.tamp.DecompressorBatch(n, window_bits=10)
    r1 = h.result(d.read([s.comp for s, _ in jobs], out_cap=50))
    d2 = h.tamp.DecompressorBatch(n, window_bits=10)
    r1b = h.result(d2.read([s.comp for s, _ in jobs], max_out=50))
    assert (r1[0] == r1b[0]).all() and r1[1] == r1b[1] and (r1[2] == r1b[2]).all() and (r1[0] == OUTPUT_FULL).all()
    assert h.torch.equal(d.objects, d2.objects)
    for i, (s, _) in enumerate(jobs):
        assert r1[1][i] == s.plain[:50]
    r2 = h.result(d2.read([s.comp[int(r1b[2][i]) :] for i, (s, _) in enumerate(jobs)]))
    for i, (s, _) in enumerate(jobs):
        assert r1b[1][i] + r2[1][i] == s.plain and int(r2[0][i]) == INPUT_EXHAUSTED, i


# ---- 5. round trip with CompressorBatch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dictionary_reset", (False, True))
def test_round_trip_with_compressor_batch(dictionary_reset, h):
    n = 70
    rng = random.Random(11 + dictionary_reset)
    p = di.prose()
    cb = h.tamp.CompressorBatch(n, window=10, dictionary_reset=dictionary_reset)
    d = h.tamp.DecompressorBatch(n, window_bits=10)
    sent, received = [b""] * n, [b""] * n

    def deliver(res):
        back = d.read(res.out, res.out_off, res.out_len)  # the compressor's CUDA tensors as they are
        st, outs, consumed = h.result(back)
        lens = res.out_len.cpu().numpy()
        for i in range(n):
            if lens[i]:
                assert int(st[i]) == INPUT_EXHAUSTED and int(consumed[i]) == int(lens[i]), i
            else:
                assert (int(st[i]), outs[i], int(consumed[i])) == (0, b"", 0), i
            received[i] += outs[i]

    for rnd in range(3):
        msgs = []
        for i in range(n):
            if rng.random() < 0.2:
                msgs.append(None)
            else:
                a = rng.randrange(0, len(p) - 300)
                msgs.append(p[a : a + rng.randrange(40, 301)])
                sent[i] += msgs[-1]
        deliver(cb.write(msgs))
        deliver(cb.flush())
        assert received == sent, f"round {rnd}"
        if dictionary_reset and rnd < 2:
            deliver(cb.reset_dictionary(which=rng.sample(range(n), 20)))
    assert all(len(x) > 0 for x in sent)


# ---- 6. refusals of the two C calls ---------------------------------------------------------------------------------------------
def test_c_calls_refuse_without_a_launch(h):
    bad = h._lib.BAD_ARGUMENT
    t = di.c_tables(3)  # host arrays: a launch that read or wrote them as device memory would fault, a refusal never looks
    for call, tables in ((di.decode_pieces, ("states", "in_off", "in_len", "out_off", "out_cap", "out_len", "status")),
                         (di.size_pieces, ("states", "in_off", "in_len", "out_len", "status"))):
        for name in tables:
            assert call(h.lib, t, 3, **{name: True}) == bad, (call.__name__, name)
        assert call(h.lib, t, 3, stride=1048) == bad and call(h.lib, t, 3, stride=1024) == bad
        assert call(h.lib, t, 3, bits=7) == bad and call(h.lib, t, 3, bits=16) == bad
        assert call(h.lib, t, 0) == OK  # nothing to do: TAMP_OK, and no launch either
        assert call(h.lib, t, 0, states=True, in_off=True, in_len=True, out_len=True, status=True, out_off=True, out_cap=True) == OK
    assert all(not v.any() for v in t.values())
