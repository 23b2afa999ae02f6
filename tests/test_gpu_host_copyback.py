"""GPU tier: how the four host-memory calls with dense output slabs on the device bring their bytes back (copy_back_slabs in
tamp_capi.hip) -- tamp_batch_compress_resets, tamp_batch_decompress_resets, tamp_batch_write_ranges, tamp_batch_compress_pieces.

Each call runs from host memory twice, through the one pinned transfer (``TAMP_AMD_NO_STAGED_COPYBACK`` unset) and row by row (set;
the variable is read at call time), on four streams of a few hundred bytes: one empty, one with too little room (TAMP_OUTPUT_FULL and
no bytes), the slabs in permuted order with gaps between them inside a buffer of guard bytes.  Both runs give the lengths, the
statuses and the bytes of the device-memory call on the same rows, and leave every byte outside [out_off[i], out_off[i] + out_len[i])
as it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, OUTPUT_FULL, INPUT_EXHAUSTED = 0, 1, 2
MEM_HOST, MEM_DEVICE = 0, 1
GUARD = 0xA5
N = 64            # the reset interval
VICTIM = 2        # the stream whose slab is too small
ORDER = [2, 0, 3, 1]  # the slabs' order in the output buffer
KW = dict(window=10, literal=8, extended=True, lazy_matching=False)
SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
PIECE_HEADER, PIECE_FINISH = 1, 8


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    return _lib.load()  # raises if the native library is missing: no silent fallback


@pytest.fixture(scope="module")
def batch():
    """(datas, blobs, reset_first, reset_off): the four inputs, and their streams with a reset every N bytes (computed once)."""
    import tamp_amd as ta
    from tamp_amd import workloads as wl

    prose = wl.frozen_corpus("prose")
    datas = [prose[1000:1300], b"", prose[5000:5417], prose[9000:9230]]
    res = ta.compress_batch(datas, dictionary_reset=True, reset_interval=N, reset_index=True, **KW)
    assert (res.status == 0).all()
    first, off = np.array(res.reset_index.first, dtype=np.uint64), np.array(res.reset_index.off, dtype=np.uint32)
    assert first.tolist() == [0, 4, 4, 10, 13]
    return datas, res.streams(), first, off


def layout(caps):
    """The slabs in ORDER, 5 + j guard bytes in front of the j-th: -> (out_off uint64, the buffer of guard bytes)."""
    off, at = np.zeros(len(caps), dtype=np.uint64), 0
    for j, i in enumerate(ORDER):
        at += 5 + j
        off[i] = at
        at += int(caps[i])
    return off, np.full(at + 9, GUARD, dtype=np.uint8)


def invoke(fn, args, mem):
    """One C call; numpy arrays among ``args`` are its tables -- host memory: passed as they are; device memory: copied to the
    device and, after the call, back over themselves -- everything else is passed on.  -> rc"""
    if mem == MEM_HOST:
        return fn(*[a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in args])
    import torch

    tables = [a for a in args if isinstance(a, np.ndarray)]
    tensors = [torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype))).cuda() for a in tables]
    torch.cuda.synchronize()
    it = iter(tensors)
    rc = fn(*[C.c_void_p(next(it).data_ptr()) if isinstance(a, np.ndarray) else a for a in args])
    torch.cuda.synchronize()
    for a, t in zip(tables, tensors):
        a.view(SIGNED.get(a.dtype, a.dtype))[...] = t.cpu().numpy()
    return rc


def flat_of(chunks):
    """The inputs with three bytes between them: -> (bytes, in_off, in_len)."""
    in_len = np.array([len(c) for c in chunks], dtype=np.uint32)
    in_off = (np.cumsum(in_len.astype(np.uint64) + 3) - in_len - 3 + 1).astype(np.uint64)
    flat = np.full(int(in_off[-1]) + int(in_len[-1]) + 3, 0xEE, dtype=np.uint8)
    for c, o in zip(chunks, in_off):
        flat[int(o) : int(o) + len(c)] = np.frombuffer(c, dtype=np.uint8)
    return flat, in_off, in_len


def three_ways(monkeypatch, run, caps, good=OK):
    """``run(mem, out, out_off, out_cap, out_len, status) -> (rc, more results)`` from device memory, then from host memory with the
    staged copy-back and without; ``good``: the status of a stream that has room.  -> the results of the device-memory call: (out_len, status, [bytes per stream], more)."""
    caps = np.array(caps, dtype=np.uint32)
    got = []
    for mem, switch in ((MEM_DEVICE, None), (MEM_HOST, None), (MEM_HOST, "1")):
        if switch is None:
            monkeypatch.delenv("TAMP_AMD_NO_STAGED_COPYBACK", raising=False)
        else:
            monkeypatch.setenv("TAMP_AMD_NO_STAGED_COPYBACK", switch)
        out_off, out = layout(caps)
        out_len, status = np.full(len(caps), 0xDEAD, dtype=np.uint32), np.full(len(caps), 99, dtype=np.int8)
        rc, more = run(mem, out, out_off, caps.copy(), out_len, status)
        assert rc == 0, (mem, switch, rc)
        assert (out_len <= caps).all()
        rows = [out[int(o) : int(o) + int(n)].tobytes() for o, n in zip(out_off, out_len)]
        print(mem, switch, out_len.tolist(), status.tolist())
        if mem == MEM_HOST:  # the gaps, the tail of every slab and the whole slab of the stream that failed
            untouched = np.ones(len(out), dtype=bool)
            for o, n in zip(out_off, out_len):
                untouched[int(o) : int(o) + int(n)] = False
            assert (out[untouched] == GUARD).all(), (switch, np.flatnonzero(untouched & (out != GUARD))[:10])
        got.append((out_len.tolist(), status.tolist(), rows, more))
    assert got[1] == got[0], "host memory, staged copy-back, against device memory"
    assert got[2] == got[0], "host memory, row by row, against device memory"
    out_len, status = got[0][0], got[0][1]
    assert status[VICTIM] == OUTPUT_FULL and out_len[VICTIM] == 0
    assert [s for i, s in enumerate(status) if i != VICTIM] == [good] * 3 and sum(1 for n in out_len if n) >= 2
    return got[0]


def test_compress_resets(lib, batch, monkeypatch):
    from tamp_amd import _lib

    datas, blobs, _, _ = batch
    conf = _lib.TampAmdConf(KW["window"], KW["literal"], 0, 1, 1, 0)
    flat, in_off, in_len = flat_of(datas)
    caps = [lib.tamp_amd_compress_resets_bound(len(d), N, KW["literal"]) for d in datas]
    caps[VICTIM] = 5

    def run(mem, out, out_off, out_cap, out_len, status):
        return invoke(lib.tamp_batch_compress_resets, [C.byref(conf), flat, in_off, in_len, N, out, out_off, out_cap, out_len, status,
                                                       len(datas), 0, mem, 0, None], mem), None

    _, _, rows, _ = three_ways(monkeypatch, run, caps)
    assert [r for i, r in enumerate(rows) if i != VICTIM] == [b for i, b in enumerate(blobs) if i != VICTIM]


def test_decompress_resets(lib, batch, monkeypatch):
    datas, blobs, first, off = batch
    flat, in_off, in_len = flat_of(blobs)
    caps = [len(d) + 3 for d in datas]
    caps[VICTIM] = 0

    def run(mem, out, out_off, out_cap, out_len, status):
        consumed = np.full(len(blobs), 0xDEAD, dtype=np.uint32)
        rc = invoke(lib.tamp_batch_decompress_resets, [15, flat, in_off, in_len, first, off, out, out_off, out_cap, out_len, status, consumed,
                                                       len(blobs), mem, 0, None], mem)
        return rc, consumed.tolist()

    # (a decoder that has room ends on the last byte of its input: TAMP_INPUT_EXHAUSTED)
    _, _, rows, _ = three_ways(monkeypatch, run, caps, good=INPUT_EXHAUSTED)
    assert [r for i, r in enumerate(rows) if i != VICTIM] == [d for i, d in enumerate(datas) if i != VICTIM]


def test_write_ranges(lib, batch, monkeypatch):
    from tamp_amd import _lib
    from tamp_amd.batch import _write_bound

    datas, blobs, first, off = batch
    conf = _lib.TampAmdConf(KW["window"], KW["literal"], 0, 1, 1, 0)
    flat, in_off, in_len = flat_of(blobs)
    # (the C call takes the writes as they come: in order of stream and begin)
    writes = [(0, 10, b"y" * 20), (0, 100, b"the quick brown fox jumps over the lazy dog, and over the next reset"), (VICTIM, 5, b"x" * 30),
              (3, 60, b"0123456789")]
    w_stream = np.array([w[0] for w in writes], dtype=np.uint32)
    w_begin = np.array([w[1] for w in writes], dtype=np.uint64)
    src, src_off, w_len = flat_of([w[2] for w in writes])
    caps = np.maximum(_write_bound(first[1:] - first[:-1], N, KW["literal"]), in_len.astype(np.uint64)).tolist()
    caps[VICTIM] = 5

    def run(mem, out, out_off, out_cap, out_len, status):
        new_off = np.full(len(off), 0xDEADBEEF, dtype=np.uint32)
        rc = invoke(lib.tamp_batch_write_ranges, [C.byref(conf), 15, flat, in_off, in_len, first, off, N, w_stream, w_begin, w_len, src, src_off,
                                                  out, out_off, out_cap, out_len, status, new_off, len(blobs), len(writes), mem, 0, None], mem)
        # (the new entries of the streams that were written; a failed stream's are not specified)
        return rc, [new_off[int(first[i]) : int(first[i + 1])].tolist() for i in range(len(blobs)) if status[i] == OK]

    _, _, rows, _ = three_ways(monkeypatch, run, caps)
    assert rows[1] == blobs[1] and rows[0] != blobs[0] and rows[3] != blobs[3]  # (the untouched stream as it was, the written ones anew)


def test_compress_pieces(lib, batch, monkeypatch):
    """One piece per object: header, input, finish."""
    from tamp_amd import _lib

    datas = batch[0]
    conf = _lib.TampAmdConf(KW["window"], KW["literal"], 0, 1, 0, 0)
    flat, in_off, in_len = flat_of(datas)
    ops = np.full(len(datas), PIECE_HEADER | PIECE_FINISH, dtype=np.uint8)
    caps = [int(lib.tamp_amd_compress_bound(len(d) + 271, KW["literal"], 0)) for d in datas]
    caps[VICTIM] = 0
    stride = 48 + (1 << KW["window"])

    def run(mem, out, out_off, out_cap, out_len, status):
        objs = np.zeros((len(datas), stride), dtype=np.uint8)
        rc = invoke(lib.tamp_batch_compress_pieces, [C.byref(conf), objs, stride, ops, flat, in_off, in_len, out, out_off, out_cap, out_len,
                                                     status, len(datas), 0, mem, 0, None], mem)
        return rc, objs.tobytes()

    import tamp_amd as ta

    _, _, rows, _ = three_ways(monkeypatch, run, caps)
    want = ta.compress_batch(list(datas), **KW).streams()  # (a whole stream in one piece is the stream of the batch call)
    assert rows[0] == want[0] and rows[3] == want[3]
