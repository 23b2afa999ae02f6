"""GPU tier of the dictionary-table calls: one launch, one custom dictionary per stream (tamp_batch_*_dicts; ``dictionaries=`` /
``dictionary_index=`` in Python), against the oracle -- and the reference C where it is built -- called per stream with THAT
stream's dictionary.  The inputs (tests/dict_table_input.py) compress to other bytes under any other dictionary, so a selector
that is ignored, shifted or applied to a neighbour fails the byte comparisons.

Covered: every compress build a batch call reaches (fixed geometry, generic, run-aware, lean one-wavefront, lazy, u16 index,
block mode, the expensive-first permutation), device and host memory, the four decoders, the size query, the long-stream
decoder, and rows the calls must refuse without touching anything.
"""
import contextlib
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dict_table_input as dti  # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, INVALID_CONF = -21, -3


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@pytest.fixture(scope="module")
def checkers(oracle):
    from oracle.checker import Ref

    return [oracle] + ([Ref()] if Ref.available() else [])


@contextlib.contextmanager
def env(name, value):
    """(set and restored the way tests/test_gpu_fixed_build.py does it)"""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


_expected = {}


def expected(checkers, window, literal, extended, lazy, max_len):
    """The 160-stream batch of a configuration and what the checkers make of every stream under ITS dictionary (computed once)."""
    key = (window, literal, extended, lazy, max_len)
    if key not in _expected:
        dicts, sel, streams = dti.batch(window, literal, max_len)
        want = []
        for k, s in zip(sel, streams):
            got = [c.compress(s, window=window, literal=literal, extended=extended, lazy_matching=lazy, dictionary=dicts[k]) for c in checkers]
            assert all(g == got[0] for g in got) and got[0][0] == 0
            want.append(got[0][1])
        _expected[key] = (dicts, sel, streams, want)
    return _expected[key]


def compress_with_table(ta, streams, dicts, sel, mem, **kw):
    """-> [(status, bytes)] of one table call, at device or at host memory."""
    import torch

    from tamp_amd.batch import pack_streams

    if mem == "host":
        r = ta.compress_batch(streams, dictionaries=dicts, dictionary_index=sel, **kw)
    else:
        dev = torch.device("cuda:0")
        flat, off, ln = pack_streams(streams)
        flat = flat if flat.size else np.zeros(1, np.uint8)
        table = torch.from_numpy(np.frombuffer(b"".join(dicts), dtype=np.uint8).reshape(len(dicts), -1).copy()).to(dev)
        r = ta.compress_batch(torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                              torch.from_numpy(ln.astype(np.int32)).to(dev), dictionaries=table,
                              dictionary_index=torch.tensor(sel, dtype=torch.int32, device=dev), **kw)
        torch.cuda.synchronize()
    return [(int(r.status[i]), r.stream(i)) for i in range(len(streams))]


CALL_DICT_TABLE = 128  # include/tamp_amd.h TAMP_AMD_CALL_DICT_TABLE


def planned_build(window, literal, extended, lazy, max_in_len, flags=0):
    from tamp_amd import _lib

    conf = _lib.TampAmdConf(window, literal, 1, int(extended), 0, int(lazy), 0, 0)
    return _lib.load().tamp_amd_compress_build(ctypes.byref(conf), max_in_len, flags, 0)


def planned(window, max_in_len, lazy=False):
    """-> (block, LDS bytes, threads, workgroups per CU) of tamp_amd_compress_plan"""
    from tamp_amd import _lib

    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert _lib.load().tamp_amd_compress_plan(window, max_in_len, int(lazy), *[ctypes.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


# ---------------------------------------------------------------- 1. compress

# (id, window, literal, extended, lazy, max_len, TAMP_AMD_FIXED_BUILD, the build tamp_amd_compress_build names for the long PLAIN
# call -- the null-table comparison of each case; the table call itself always takes a generic build, its table twin)
COMPRESS_CASES = [
    ("w10_fixed_ext", 10, 8, True, False, None, None, 1),
    ("w10_generic_ext", 10, 8, True, False, None, "0", 0),
    ("w10_fixed_v1", 10, 8, False, False, None, None, 2),
    ("w10_generic_v1", 10, 8, False, False, None, "0", 0),
    ("w8_l7_messages", 8, 7, True, False, 256, None, 0),
    ("w15_u16_index", 15, 8, True, False, None, None, 0),
    ("w10_lazy", 10, 8, True, True, None, None, 0),
]


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("case", COMPRESS_CASES, ids=[c[0] for c in COMPRESS_CASES])
def test_compress_every_stream_under_its_own_dictionary(ta, checkers, case, mem):
    _, window, literal, extended, lazy, max_len, fixed_env, build = case
    dicts, sel, streams, want = expected(checkers, window, literal, extended, lazy, max_len)
    kw = dict(window=window, literal=literal, extended=extended, lazy_matching=lazy)
    longest = max(len(s) for s in streams)
    short = [i for i, s in enumerate(streams) if len(s) <= 300]  # (a call of its own: one-wavefront workgroups below 1 KiB)
    assert {len(streams[i]) for i in short} >= {0, 1, 15, 16, 17} and len({sel[i] for i in short}) == dti.K
    with (env("TAMP_AMD_FIXED_BUILD", fixed_env) if fixed_env is not None else contextlib.nullcontext()):
        assert planned_build(window, literal, extended, lazy, longest) == build
        assert planned_build(window, literal, extended, lazy, longest, CALL_DICT_TABLE) == 0
        if longest >= 1024:  # (four wavefronts per workgroup for the long call, one for the short one)
            assert planned(window, longest, lazy)[2] == 256 and planned(window, 300, lazy)[2] == 64
        got = compress_with_table(ta, streams, dicts, sel, mem, max_in_len=longest, **kw)
        got_short = compress_with_table(ta, [streams[i] for i in short], dicts, [sel[i] for i in short], mem, max_in_len=300, **kw)
        # the null-table path of the same build: the streams of selector 0 under dictionary=dictionaries[0]
        zero = [i for i, k in enumerate(sel) if k == 0]
        plain = ta.compress_batch([streams[i] for i in zero], dictionary=dicts[0], max_in_len=longest, **kw)
    for i, (st, out) in enumerate(got):
        assert st == 0 and len(out) == len(want[i]) and out == want[i], (case[0], mem, i, sel[i], len(streams[i]))
    for j, i in enumerate(short):
        assert got_short[j] == (0, want[i]), (case[0], mem, "short call", i, sel[i], len(streams[i]))
    for j, i in enumerate(zero):
        assert (int(plain.status[j]), plain.stream(j)) == got[i], (case[0], mem, "dictionary= against the table", i)


def test_compress_a_batch_the_expensive_first_order_permutes(ta, checkers):
    """More streams than the persistent grid has workgroups: the launcher orders the streams by cost, gathers the table rows
    -- the selector with them -- and scatters the results back."""
    import torch

    blk, _, threads, per_cu = planned(10, 1024)
    assert threads == 256
    n = per_cu * torch.cuda.get_device_properties(0).multi_processor_count + 1  # the smallest batch that is ordered
    dicts = dti.dictionaries(10)
    sel = [(i * 7 + i // 11) % dti.K for i in range(n)]
    # (costs differ: noisy streams match less)
    streams = [dti.stream(k, 1024 if i % 3 else 700, i % 97, noise=(0.02, 0.3, 0.7)[i % 3]) for i, k in enumerate(sel)]
    with env("TAMP_AMD_LPT", "1"):  # (ordered whatever the grid turns out to hold; without it, from n streams on)
        got = compress_with_table(ta, streams, dicts, sel, "device", window=10, literal=8, max_in_len=1024)
    default = compress_with_table(ta, streams, dicts, sel, "device", window=10, literal=8, max_in_len=1024)
    assert default == got
    zero = [i for i, k in enumerate(sel) if k == 0]  # the null-table path: dictionary=dictionaries[0]
    plain = ta.compress_batch([streams[i] for i in zero], window=10, literal=8, dictionary=dicts[0], max_in_len=1024)
    assert [(int(plain.status[j]), plain.stream(j)) for j in range(len(zero))] == [got[i] for i in zero]
    oracle = checkers[0]
    memo = {}
    for i, (k, s) in enumerate(zip(sel, streams)):
        if (k, s) not in memo:
            memo[(k, s)] = oracle.compress(s, window=10, literal=8, dictionary=dicts[k])
        assert got[i] == memo[(k, s)], (i, k)


# ---------------------------------------------------------------- 2. block mode

def test_block_mode_two_streams_two_dictionaries(ta, checkers):
    dicts = dti.dictionaries(10)
    sel = [4, 1]
    streams = [dti.stream(k, 262144 + 4096, 500 + k, noise=0.3) for k in sel]
    kw = dict(window=10, literal=8, extended=False, max_in_len=262144 + 4096)
    want = []
    for k, s in zip(sel, streams):
        got = [c.compress(s, window=10, literal=8, extended=False, dictionary=dicts[k]) for c in checkers]
        assert all(g == got[0] for g in got)
        want.append(got[0])
    assert want[0] != checkers[0].compress(streams[0], window=10, literal=8, extended=False, dictionary=dicts[1])
    assert compress_with_table(ta, streams, dicts, sel, "device", **kw) == want
    with env("TAMP_AMD_BLOCK_MIN", "0"):  # (the batch kernel instead)
        assert compress_with_table(ta, streams, dicts, sel, "device", **kw) == want


# ---------------------------------------------------------------- 3. decode

def decode_expected(checkers, blobs, dicts, sel, cap):
    want = []
    for k, b in zip(sel, blobs):
        got = [c.decompress(b, dictionary=dicts[k] if k is not None else None, cap=cap) for c in checkers]
        assert all(g == got[0] for g in got)
        want.append(got[0])
    return want


def assert_decodes(r, want, what):
    for i, (st, out, used) in enumerate(want):
        assert (int(r.status[i]), r.stream(i), int(r.in_consumed[i])) == (st, out, used), (what, i)


@pytest.mark.parametrize("decoder", ["split", "lane", "global", "wave"])
@pytest.mark.parametrize("case", [COMPRESS_CASES[0], COMPRESS_CASES[2], COMPRESS_CASES[4], COMPRESS_CASES[5]], ids=lambda c: c[0])
def test_decode_with_the_table_on_every_decoder(ta, checkers, case, decoder, monkeypatch):
    import torch

    from tamp_amd.batch import pack_streams

    _, window, literal, extended, lazy, max_len, _, _ = case
    dicts, sel, streams, blobs = expected(checkers, window, literal, extended, lazy, max_len)
    cap = 9000 + 8
    monkeypatch.setenv("TAMP_AMD_DECODER", decoder)
    host = ta.decompress_batch(blobs, out_cap=cap, dictionaries=dicts, dictionary_index=sel)
    dev = torch.device("cuda:0")
    flat, off, ln = pack_streams(blobs)
    table = torch.from_numpy(np.frombuffer(b"".join(dicts), dtype=np.uint8).reshape(dti.K, -1).copy()).to(dev)
    args = (torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev))
    device = ta.decompress_batch(*args, out_cap=cap, dictionaries=table, dictionary_index=torch.tensor(sel, device=dev))
    sizes = ta.decoded_size_batch(*args, limit=cap, dictionary=ta.DictionaryTable(table, torch.tensor(sel, device=dev)))
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        for r in (host, device):
            assert (int(r.status[i]), r.stream(i), int(r.in_consumed[i])) == (2, s, len(blobs[i])), (case[0], decoder, i, sel[i])
        assert (int(sizes.size[i]), int(sizes.status[i]), int(sizes.in_consumed[i])) == (len(s), 2, len(blobs[i])), (case[0], decoder, i)


def test_decode_a_mixed_batch_over_one_table(ta, checkers):
    """Streams with the custom bit at windows 8, 10 and 12 and streams without it, over a table of D = 4,096: each custom stream
    reads the first ``1 << its window`` bytes of its row, one without the bit ignores its row."""
    oracle = checkers[0]
    d12 = dti.dictionaries(12)
    sel, blobs, plain, custom = [], [], [], []
    for i in range(60):
        k = (i * 3) % dti.K
        s = dti.stream(k, (40, 256, 1500, 4096)[i % 4], 300 + i)
        window = (8, 10, 12)[i % 3]
        use = i % 5 != 4
        st, b = oracle.compress(s, window=window, extended=bool(i % 2), dictionary=d12[k][: 1 << window] if use else None)
        assert st == 0 and bool(b[0] & 4) == use
        sel.append(k), blobs.append(b), plain.append(s), custom.append(use)
    assert not all(custom) and any(custom)
    want = decode_expected(checkers, blobs, d12, sel, 4200)
    assert all(w[:2] == (2, s) for w, s in zip(want, plain))
    # (the rows matter: under the row of another dictionary a custom stream decodes to other bytes)
    assert all(oracle.decompress(b, dictionary=d12[(k + 1) % dti.K], cap=4200)[1] != s for b, k, s, c in zip(blobs, sel, plain, custom) if c)
    r = ta.decompress_batch(blobs, out_cap=4200, dictionaries=d12, dictionary_index=sel)
    assert_decodes(r, want, "mixed")
    q = ta.decoded_size_batch(blobs, limit=4200, dictionary=ta.DictionaryTable(d12, sel))
    for i in range(len(blobs)):
        assert (int(q.size[i]), int(q.status[i]), int(q.in_consumed[i])) == (int(r.out_len[i]), int(r.status[i]), int(r.in_consumed[i])), i
    # a tight limit: the size query answers what the decode answers with out_cap = limit
    r = ta.decompress_batch(blobs, out_cap=200, dictionaries=d12, dictionary_index=sel)
    assert_decodes(r, decode_expected(checkers, blobs, d12, sel, 200), "mixed, 200 bytes of room")
    q = ta.decoded_size_batch(blobs, limit=200, dictionary=ta.DictionaryTable(d12, sel))
    for i in range(len(blobs)):
        assert (int(q.size[i]), int(q.status[i]), int(q.in_consumed[i])) == (int(r.out_len[i]), int(r.status[i]), int(r.in_consumed[i])), i


@pytest.mark.parametrize("mem", ["device", "host"])
def test_decode_without_out_cap_round_trips(ta, checkers, mem):
    import torch

    from tamp_amd.batch import pack_streams

    dicts, sel, streams, blobs = expected(checkers, 10, 8, True, False, None)
    if mem == "host":
        r = ta.decompress_batch(blobs, dictionaries=dicts, dictionary_index=np.array(sel))
    else:
        dev = torch.device("cuda:0")
        flat, off, ln = pack_streams(blobs)
        r = ta.decompress_batch(torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                                torch.from_numpy(ln.astype(np.int32)).to(dev), dictionaries=np.stack([np.frombuffer(d, np.uint8) for d in dicts]),
                                dictionary_index=torch.tensor(sel, device=dev))
        torch.cuda.synchronize()
    for i, s in enumerate(streams):
        assert (int(r.status[i]), r.stream(i)) == (2, s), (mem, i)


# ---------------------------------------------------------------- 4. the long-stream decoder

def test_long_decoder_takes_each_stream_with_its_own_dictionary(ta, checkers, monkeypatch, capfd):
    oracle = checkers[0]
    dicts = dti.dictionaries(10)
    sel = [2, 4, 1]
    plain = [dti.stream(k, 300_000, 700 + k, noise=0.6) for k in sel]
    blobs = [oracle.compress(s, window=10, extended=ext, dictionary=dicts[k])[1] for s, k, ext in zip(plain, sel, (False, False, True))]
    assert all(len(b) >= 65536 and b[0] & 4 for b in blobs), [len(b) for b in blobs]
    want = decode_expected(checkers, blobs, dicts, sel, 300_100)
    assert [w[:2] for w in want] == [(2, s) for s in plain]
    monkeypatch.setenv("TAMP_AMD_LONGDEC_MIN", "65536")
    monkeypatch.setenv("TAMP_AMD_LONGDEC_DEBUG", "1")
    # the two v1 streams in a call of their own: one stream declined would send a WHOLE call to the exact decoders, which write
    # every stream again, and a long path that ignored the table would go unnoticed
    capfd.readouterr()
    r = ta.decompress_batch(blobs[:2], out_cap=300_100, dictionaries=dicts, dictionary_index=sel[:2])
    err = capfd.readouterr().err
    print(err)
    assert_decodes(r, want[:2], "long, v1")
    taken = re.findall(r"\[tamp_amd long decode\] \d+ groups, ", err)
    declined = re.findall(r"\[tamp_amd long decode\] declined: (.+)", err)
    assert len(taken) == 2 and declined == [], (taken, declined)
    # ... and with the extended stream behind them (taken or declined, the line says which; never for its dictionary)
    r = ta.decompress_batch(blobs, out_cap=300_100, dictionaries=dicts, dictionary_index=sel)
    err = capfd.readouterr().err
    print(err)
    assert_decodes(r, want, "long")
    taken = re.findall(r"\[tamp_amd long decode\] \d+ groups, ", err)
    declined = re.findall(r"\[tamp_amd long decode\] declined: (.+)", err)
    assert len(taken) >= 2 and len(taken) + len(declined) == 3 and "dictionary" not in declined, (taken, declined)
    # a row whose window ends beyond the table: the long path declines, the exact decoders report it
    capfd.readouterr()
    table = b"".join(dicts)
    r = _raw_decompress(ta, table[: 4 * 1024 + 1008], [k * 1024 for k in sel], blobs, [300_100] * 3, "host")
    assert "declined: dictionary" in capfd.readouterr().err
    assert [(st, n) for st, n, _ in r] == [(2, 300_000), (INVALID_CONF, 0), (2, 300_000)]
    q = ta.decoded_size_batch(blobs, dictionary=ta.DictionaryTable(dicts, sel))
    assert [(int(q.size[i]), int(q.status[i]), int(q.in_consumed[i])) for i in range(3)] == [(300_000, 2, len(b)) for b in blobs]


# ---------------------------------------------------------------- 5. rows the calls refuse

GUARD, GAP = 0xA5, 32


def _tables(streams, caps):
    from tamp_amd.batch import pack_streams

    flat, in_off, in_len = pack_streams(streams)
    flat = flat if flat.size else np.zeros(1, np.uint8)
    caps = np.asarray(caps, dtype=np.uint32)
    out_off = (np.cumsum(caps.astype(np.uint64) + GAP) - caps + 0).astype(np.uint64)  # GAP guard bytes in front of every slab
    out = np.full(int(out_off[-1] + caps[-1] + GAP), GUARD, dtype=np.uint8)
    return flat, in_off, in_len, out, out_off, caps


def _raw(ta, call, table, dict_off, streams, caps, mem):
    """One *_dicts call through the C ABI with the offsets as given (Python forms index * D and cannot misalign a row).
    -> [(status, out_len, slab)] with the whole slab, and asserts the guard bytes around every slab."""
    import torch

    from tamp_amd import _lib

    lib = _lib.load()
    flat, in_off, in_len, out, out_off, caps = _tables(streams, caps)
    n = len(streams)
    arrays = dict(table=np.frombuffer(table, dtype=np.uint8).copy(), dict_off=np.asarray(dict_off, dtype=np.uint64), flat=flat, in_off=in_off,
                  in_len=in_len, out=out, out_off=out_off, caps=caps, out_len=np.full(n, 0xDDDDDDDD, np.uint32),
                  status=np.full(n, 77, np.int8), consumed=np.zeros(n, np.uint32))
    if mem == "device":
        dev = torch.device("cuda:0")
        held = {k: torch.from_numpy(np.array(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v)).to(dev)
                for k, v in arrays.items()}
        p = {k: ctypes.c_void_p(t.data_ptr()) for k, t in held.items()}
        torch.cuda.synchronize()
    else:
        p = {k: v.ctypes.data_as(ctypes.c_void_p) for k, v in arrays.items()}
    m = _lib.MEM_DEVICE if mem == "device" else _lib.MEM_HOST
    rc = call(lib, p, len(table), n, m)
    assert rc == 0
    if mem == "device":
        torch.cuda.synchronize()
        for k in ("out", "out_len", "status", "consumed"):
            arrays[k] = held[k].cpu().numpy().view(arrays[k].dtype)
    out = arrays["out"]
    res, at = [], 0
    for i in range(n):
        o, c = int(out_off[i]), int(caps[i])
        assert (out[at:o] == GUARD).all(), ("guard bytes in front of slab", i)
        at = o + c
        res.append((int(arrays["status"][i]), int(arrays["out_len"][i]), out[o:o + c].tobytes()))
    assert (out[at:] == GUARD).all(), "guard bytes behind the last slab"
    return res, arrays


def _raw_compress(ta, conf, table, dict_off, streams, caps, mem, max_in_len=0):
    def call(lib, p, table_len, n, m):
        return lib.tamp_batch_compress_dicts(ctypes.byref(conf), p["table"], table_len, p["dict_off"], p["flat"], p["in_off"], p["in_len"],
                                             p["out"], p["out_off"], p["caps"], p["out_len"], p["status"], n, max_in_len, m, 0, None)
    return _raw(ta, call, table, dict_off, streams, caps, mem)[0]


def _raw_decompress(ta, table, dict_off, blobs, caps, mem):
    """-> [(status, out_len, in_consumed)]; asserts that the size query answers the same."""
    def call(lib, p, table_len, n, m):
        return lib.tamp_batch_decompress_dicts(p["table"], table_len, p["dict_off"], 15, p["flat"], p["in_off"], p["in_len"], p["out"],
                                               p["out_off"], p["caps"], p["out_len"], p["status"], p["consumed"], n, m, 0, None)

    def size_call(lib, p, table_len, n, m):
        return lib.tamp_batch_decoded_size_dicts(table_len, p["dict_off"], 15, p["flat"], p["in_off"], p["in_len"], p["caps"],
                                                 p["out_len"], p["status"], p["consumed"], n, m, 0, None)
    res, arrays = _raw(ta, call, table, dict_off, blobs, caps, mem)
    got = [(st, n, int(arrays["consumed"][i])) for i, (st, n, _) in enumerate(res)]
    for i, (st, n, slab) in enumerate(res):
        if st < 0:
            assert n == 0 and slab == bytes([GUARD]) * len(slab), ("a refused stream writes nothing", i)
    sres, sarrays = _raw(ta, size_call, table, dict_off, blobs, caps, mem)
    assert [(st, n, int(sarrays["consumed"][i])) for i, (st, n, _) in enumerate(sres)] == got, "size query != decode"
    return got


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("case", [COMPRESS_CASES[0], COMPRESS_CASES[1], COMPRESS_CASES[4], COMPRESS_CASES[6]], ids=lambda c: c[0])
def test_compress_refuses_a_bad_row_and_nothing_else(ta, checkers, case, mem):
    from tamp_amd import _lib

    _, window, literal, extended, lazy, max_len, fixed_env, _ = case
    oracle = checkers[0]
    W = 1 << window
    dicts = dti.dictionaries(window)
    table = b"".join(dicts) + bytes(range(40))  # (a tail: the last whole window ends 40 bytes in front of the end)
    n_len = 256 if max_len else 1500
    sel = [1, 2, 3, 4, 0, 1, 2, 3, 4, 0]
    streams = [dti.stream(k, n_len - 7 * i, 900 + i, literal=literal) for i, k in enumerate(sel)]
    off = [k * W for k in sel]
    assert len(table) == 5 * W + 40
    off[2] = 4 * W + 48              # a multiple of 16 whose window would end 8 bytes past the table
    off[4] = 2 * W + 8               # inside the table, not a multiple of 16
    off[6] = 1 << 40                 # far outside
    off[7] = 4 * W + 24              # the last bytes of the table, not a multiple of 16
    off[9] = 4 * W + 32              # the last row there is: in bounds by 8 bytes
    bad = {2, 4, 6, 7}
    conf = _lib.TampAmdConf(window, literal, 1, int(extended), 0, int(lazy), 0, 0)
    caps = [2000] * len(sel)
    with (env("TAMP_AMD_FIXED_BUILD", fixed_env) if fixed_env is not None else contextlib.nullcontext()):
        got = _raw_compress(ta, conf, table, off, streams, caps, mem, max_in_len=n_len)
    for i, (st, n, slab) in enumerate(got):
        if i in bad:
            assert (st, n) == (BAD_ARGUMENT, 0) and slab == bytes([GUARD]) * len(slab), (case[0], mem, i, st, n)
        else:
            want = oracle.compress(streams[i], window=window, literal=literal, extended=extended, lazy_matching=lazy,
                                   dictionary=table[off[i]:off[i] + W])
            assert (st, slab[:n]) == want, (case[0], mem, i)


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("decoder", ["split", "lane", "global", "wave"])
def test_decode_refuses_a_bad_row_and_nothing_else(ta, checkers, decoder, mem, monkeypatch):
    oracle = checkers[0]
    W = 1024
    dicts = dti.dictionaries(10)
    table = b"".join(dicts) + bytes(range(40))
    sel = [1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2]
    plain = [dti.stream(k, 1200 - 31 * i, 950 + i) for i, k in enumerate(sel)]
    off = [k * W for k in sel]
    off[2] = 4 * W + 48              # ends 8 bytes past the table: TAMP_INVALID_CONF, what too short a shared dictionary gets
    off[4] = 2 * W + 8               # not a multiple of 16: TAMP_AMD_BAD_ARGUMENT
    off[6] = 1 << 40
    off[7] = 4 * W + 24              # not a multiple of 16, in bounds
    off[10] = (1 << 40) + 3          # a stream WITHOUT the custom bit ignores its row, whatever it holds
    off[11] = 4 * W + 32             # the last row there is: in bounds by 8 bytes
    status = {2: INVALID_CONF, 4: BAD_ARGUMENT, 6: INVALID_CONF, 7: BAD_ARGUMENT}
    blobs = [oracle.compress(s, window=10, extended=bool(i % 2),
                             dictionary=None if i == 10 else dicts[k] if i in status else table[off[i]:off[i] + W])[1]
             for i, (k, s) in enumerate(zip(sel, plain))]
    monkeypatch.setenv("TAMP_AMD_DECODER", decoder)
    got = _raw_decompress(ta, table, off, blobs, [1300] * len(sel), mem)
    for i, (st, n, used) in enumerate(got):
        if i in status:
            assert (st, n) == (status[i], 0), (decoder, mem, i, st, n)
        else:
            assert (st, n, used) == (2, len(plain[i]), len(blobs[i])), (decoder, mem, i)
    # the bytes of the good streams
    def call(lib, p, table_len, n, m):
        return lib.tamp_batch_decompress_dicts(p["table"], table_len, p["dict_off"], 15, p["flat"], p["in_off"], p["in_len"], p["out"],
                                               p["out_off"], p["caps"], p["out_len"], p["status"], p["consumed"], n, m, 0, None)
    res, _ = _raw(ta, call, table, off, blobs, [1300] * len(sel), mem)
    for i, (st, n, slab) in enumerate(res):
        if i not in status:
            assert slab[:n] == plain[i], (decoder, mem, i)


def test_python_device_selector_out_of_range_is_the_streams_own_error(ta, checkers):
    """A device selector is not checked on the host (that would take a sync): the row lands outside the table and the stream
    alone is refused."""
    import torch

    from tamp_amd.batch import pack_streams

    dev = torch.device("cuda:0")
    dicts = dti.dictionaries(10)
    sel = [0, 1, 7, 3, -1, 4]
    streams = [dti.stream(k % dti.K, 600, 990 + i) for i, k in enumerate(sel)]
    flat, off, ln = pack_streams(streams)
    r = ta.compress_batch(torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                          torch.from_numpy(ln.astype(np.int32)).to(dev), window=10, dictionaries=dicts,
                          dictionary_index=torch.tensor(sel, device=dev), max_in_len=600)
    torch.cuda.synchronize()
    for i, k in enumerate(sel):
        if 0 <= k < dti.K:
            assert (int(r.status[i]), r.stream(i)) == checkers[0].compress(streams[i], window=10, dictionary=dicts[k]), i
        else:
            assert (int(r.status[i]), int(r.out_len[i])) == (BAD_ARGUMENT, 0), i
