"""GPU tier: every per-stream table of a batch call -- the dictionary selector with them -- across host chunks and fan-out shards.

600 streams of 4,096 bytes (tests/dict_table_input.py; extended format, window 10, the window-10 custom dictionaries), the selector
cycling through every row so that each chunk and each shard starts on another row.  TAMP_AMD_HOST_CHUNK_STREAMS=64 and
TAMP_AMD_HOST_CHUNK_MB=1 cut a host-memory call into three chunks (256 / 256 / 88 streams where a stream's extent is 4,096 bytes);
TAMP_AMD_FANOUT=3 cuts an ALL_DEVICES call into three shards in front of that.  Every stream is compared bit-exact with the checker
under ITS dictionary, every status, length and consumed count with it.  The object calls (DecoderBatch.step, EncoderBatch.compress)
take the same three-chunk split with 600 objects and 64-byte pieces: their state rows travel with the chunks.
"""
import contextlib
import ctypes as C
import faulthandler
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dict_table_input as dti  # noqa: E402

pytestmark = pytest.mark.gpu

N, LEN, WINDOW, CAP = 600, 4096, 10, 4096
MODES = ("host", "fanout", "device")


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@contextlib.contextmanager
def time_limit(seconds):
    """A case that hangs ends the run (with every thread's stack) instead of waiting for the caller's patience."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


@pytest.fixture
def chunked(monkeypatch):
    monkeypatch.setenv("TAMP_AMD_HOST_CHUNK_STREAMS", "64")
    monkeypatch.setenv("TAMP_AMD_HOST_CHUNK_MB", "1")
    monkeypatch.setenv("TAMP_AMD_FANOUT", "3")  # (read by ALL_DEVICES calls only)


@pytest.fixture(scope="module")
def batch(oracle):
    """The inputs and what the checker makes of each stream under its own dictionary (computed once, never changed)."""
    dicts = dti.dictionaries(WINDOW)
    sel = [i % dti.K for i in range(N)]
    streams = [dti.stream(k, LEN, 2000 + i) for i, k in enumerate(sel)]
    comp = [oracle.compress(s, window=WINDOW, extended=True, dictionary=dicts[k]) for s, k in zip(streams, sel)]
    assert all(st == 0 for st, _ in comp)
    blobs = [b for _, b in comp]
    # (a neighbour's dictionary gives other bytes: a selector shifted by a row fails the comparisons)
    assert all(oracle.compress(streams[i], window=WINDOW, extended=True, dictionary=dicts[(sel[i] + 1) % dti.K])[1] != blobs[i] for i in range(0, N, 37))
    tight = [oracle.decompress(b, dictionary=dicts[k], cap=CAP) for b, k in zip(blobs, sel)]
    roomy = [oracle.decompress(b, dictionary=dicts[k], cap=LEN + 1) for b, k in zip(blobs, sel)]
    assert all(r == (2, s, len(b)) for r, s, b in zip(roomy, streams, blobs))
    assert all(len(out) == CAP for _, out, _ in tight)
    return dict(dicts=dicts, sel=sel, streams=streams, comp=comp, blobs=blobs, tight=tight, roomy=roomy)


def _inputs(ta, mode, items, dicts, sel):
    """-> (positional arguments, keywords, dictionaries, dictionary_index) of a batch call on ``items`` in this mode"""
    from tamp_amd import _lib

    if mode != "device":
        return (items,), dict(device=_lib.ALL_DEVICES if mode == "fanout" else 0), dicts, sel
    import torch

    dev = torch.device("cuda:0")
    flat, off, ln = ta.pack_streams(items)
    table = torch.from_numpy(np.frombuffer(b"".join(dicts), dtype=np.uint8).reshape(len(dicts), -1).copy()).to(dev)
    args = (torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev))
    return args, {}, table, torch.tensor(sel, dtype=torch.int32, device=dev)


def _sync(mode):
    if mode == "device":
        import torch

        torch.cuda.synchronize()


@pytest.mark.parametrize("mode", MODES)
def test_compress_every_stream_under_its_own_dictionary(ta, batch, chunked, mode):
    args, kw, d, s = _inputs(ta, mode, batch["streams"], batch["dicts"], batch["sel"])
    with time_limit(120):
        r = ta.compress_batch(*args, window=WINDOW, extended=True, dictionaries=d, dictionary_index=s, max_in_len=LEN, **kw)
        _sync(mode)
    for i, (st, want) in enumerate(batch["comp"]):
        assert (int(r.status[i]), int(r.out_len[i])) == (st, len(want)) and r.stream(i) == want, (mode, i, batch["sel"][i])


def _decoded(r, mode, i):
    return (int(r.status[i]), r.stream(i), int(r.in_consumed[i]))


@pytest.mark.parametrize("mode", MODES)
def test_decompress_with_and_without_out_cap(ta, batch, chunked, mode):
    args, kw, d, s = _inputs(ta, mode, batch["blobs"], batch["dicts"], batch["sel"])
    with time_limit(120):
        tight = ta.decompress_batch(*args, out_cap=CAP, dictionaries=d, dictionary_index=s, **kw)
        sized = ta.decompress_batch(*args, dictionaries=d, dictionary_index=s, **kw)
        _sync(mode)
    for i in range(N):
        assert _decoded(tight, mode, i) == batch["tight"][i], (mode, "out_cap", i, batch["sel"][i])
        assert int(tight.out_len[i]) == len(batch["tight"][i][1])
        assert _decoded(sized, mode, i) == batch["roomy"][i], (mode, "sized", i, batch["sel"][i])
        assert int(sized.out_len[i]) == LEN


@pytest.mark.parametrize("mode", ["host", "fanout"])
def test_decompress_without_a_consumed_table(ta, batch, chunked, mode):
    """tamp_batch_decompress_dicts with in_consumed = null (the Python calls always pass one): statuses, lengths and bytes as ever."""
    from tamp_amd import _lib

    lib = _lib.load()
    flat, in_off, in_len = ta.pack_streams(batch["blobs"])
    table, dict_off = ta.DictionaryTable(batch["dicts"], batch["sel"]).on_host(N)
    cap = np.full(N, LEN + 1, np.uint32)
    out_off = (np.cumsum(cap, dtype=np.uint64) - cap).astype(np.uint64)
    out, out_len, status = np.zeros(int(cap.sum()) + 1, np.uint8), np.full(N, 0xDDDDDDDD, np.uint32), np.full(N, 77, np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    with time_limit(120):
        rc = lib.tamp_batch_decompress_dicts(p(table), table.size, p(dict_off), 15, p(flat), p(in_off), p(in_len), p(out), p(out_off), p(cap),
                                             p(out_len), p(status), None, N, _lib.MEM_HOST, _lib.ALL_DEVICES if mode == "fanout" else 0, None)
    assert rc == 0
    for i, s in enumerate(batch["streams"]):
        o = int(out_off[i])
        assert (int(status[i]), int(out_len[i]), out[o:o + LEN].tobytes()) == (2, LEN, s), (mode, i)


@pytest.mark.parametrize("mode", MODES)
def test_decoded_size_with_and_without_limit(ta, batch, chunked, mode):
    args, kw, d, s = _inputs(ta, mode, batch["blobs"], batch["dicts"], batch["sel"])
    with time_limit(120):
        limited = ta.decoded_size_batch(*args, limit=CAP, dictionary=ta.DictionaryTable(d, s), **kw)
        free = ta.decoded_size_batch(*args, dictionary=ta.DictionaryTable(d, s), **kw)
        _sync(mode)
    for i in range(N):
        st, out, used = batch["tight"][i]
        assert (int(limited.size[i]), int(limited.status[i]), int(limited.in_consumed[i])) == (len(out), st, used), (mode, "limit", i)
        assert (int(free.size[i]), int(free.status[i]), int(free.in_consumed[i])) == (LEN, 2, len(batch["blobs"][i])), (mode, "no limit", i)


PIECE, OBJ_LEN = 64, 1024  # the object calls: 64-byte pieces of the first KiB of every stream, 4,096 bytes of room per object and call


def test_decoder_objects_in_three_chunks(ta, oracle, batch, chunked):
    plain = [s[:OBJ_LEN] for s in batch["streams"]]
    blobs = [oracle.compress(s, window=WINDOW)[1] for s in plain]
    steps = (max(len(b) for b in blobs) + PIECE - 1) // PIECE + 1  # (one more: every object sees the end of its input)
    want = [oracle.decode_script(b, [(PIECE, CAP)] * steps, window_bits=WINDOW) for b in blobs]
    assert all(r0 == 0 and b"".join(out for _, out, _ in calls) == s for (r0, calls), s in zip(want, plain))
    with time_limit(120):
        dec = ta.DecoderBatch(N, window_bits=WINDOW)
        pos = [0] * N
        for step in range(steps):
            status, outs, consumed = dec.step([b[pos[i]:pos[i] + PIECE] for i, b in enumerate(blobs)], CAP)
            for i in range(N):
                assert (int(status[i]), outs[i], int(consumed[i])) == want[i][1][step], (step, i)
                pos[i] += int(consumed[i])


def test_encoder_objects_in_three_chunks(ta, oracle, batch, chunked):
    plain = [s[:OBJ_LEN] for s in batch["streams"]]
    want = [oracle.compress(s, window=WINDOW, extended=True) for s in plain]
    got = [bytearray() for _ in plain]
    with time_limit(120):
        enc = ta.EncoderBatch(N, window=WINDOW, extended=True)
        for at in range(0, OBJ_LEN, PIECE):
            status, outs, consumed = enc.compress([s[at:at + PIECE] for s in plain], CAP)
            assert (np.asarray(status) == 0).all() and (np.asarray(consumed) == PIECE).all(), at
            for g, o in zip(got, outs):
                g += o
        status, outs, _ = enc.flush(CAP, write_token=False)
        assert (np.asarray(status) == 0).all()
    for i, (g, o) in enumerate(zip(got, outs)):
        assert (0, bytes(g + o)) == want[i], i
