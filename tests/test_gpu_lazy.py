"""GPU tier: lazy matching decision by decision, on every path that restates it -- the walk's state machine and the probe tables
of the lazy compress builds (kLazyPacked, kLazyU16 and their dictionary-table twins, with one wavefront and with four), whole
segments with state, and the resume kernel's cached match between calls.  All `-m gpu`, everything bit-exact.

The inputs are tests/lazy_input.py's: one stream per decision (defer / tie / lose, the length and ring gates, the overlap rule at
both of its ends, cached matches into extended matches, chains, the RLE handler meeting a cached match, excess bits at a deferred
literal, the window's end, the stream's first position, and a defer at every distance from an epoch's end); tests/test_lazy_input.py
proves on the CPU that each takes its decision.  The expected bytes are the oracle's, and each is first held against the reference's
recorded result (status, length, SHA-256) in tests/golden/lazy_cells.json, so what is compared is the reference's own output.
Every batch goes once through decompress_batch.  A failing assertion names configuration, case (cell and size) and route.

The reference harness does not show its object's cached_match_index / cached_match_size, so for the resume kernel bytes and
per-call results (status, written, consumed) are what is held; a wrong cached state shows in the second call's bytes.
"""
import ctypes
import hashlib
import io
import os
import sys
import time

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

import lazy_input as li  # noqa: E402

GENERIC = 0            # include/tamp_amd.h TAMP_AMD_BUILD_GENERIC
CALL_DICT_TABLE = 128  # TAMP_AMD_CALL_DICT_TABLE
TUNING_ENV = ("TAMP_AMD_BLK", "TAMP_AMD_RUNS", "TAMP_AMD_FIXED_BUILD", "TAMP_AMD_BLOCK_LEAN", "TAMP_AMD_BLOCK_MIN", "TAMP_AMD_CUT_RUN",
              "TAMP_AMD_LPT", "TAMP_AMD_STATIC_GRID", "TAMP_AMD_GRID_PER_CU")
CONFIGS = tuple((w, 8, e) for w in li.CONFIGS_8 for e in (True, False)) + tuple((w, l, e) for w, l in li.CONFIGS_OTHER for e in (True, False))
SWEEPS = ((8, True), (8, False), (10, True), (10, False))
CAP = 4096


def config_id(window, literal, extended):
    return f"w{window}-l{literal}-{'ext' if extended else 'v1'}"


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@pytest.fixture(scope="module")
def golden():
    return load_golden("lazy_cells.json")


@pytest.fixture(autouse=True)
def no_tuning_env(monkeypatch):
    for k in TUNING_ENV:
        monkeypatch.delenv(k, raising=False)


_want = {}


def want(oracle, golden, case):
    """(status, bytes) of a case: the oracle's, held against the reference's recorded result.  Computed once, never modified."""
    key = (case.window, case.literal, case.extended, case.name)
    if key not in _want:
        rc, blob = oracle.compress(case.data, window=case.window, literal=case.literal, extended=case.extended, dictionary=case.dictionary,
                                   lazy_matching=True)
        rec = golden["cases"][config_id(case.window, case.literal, case.extended)][case.name]
        assert [rc, len(blob), hashlib.sha256(blob).hexdigest()] == rec, (key, "the oracle is not the recorded reference")
        _want[key] = (rc, blob)
    return _want[key]


def planned(window, literal, extended, max_in_len, flags=0):
    """-> (TAMP_AMD_BUILD_*, block, threads per workgroup) of a lazy batch call under the current environment."""
    from tamp_amd import _lib

    lib = _lib.load()
    conf = _lib.TampAmdConf(window, literal, 0, int(extended), 0, 1, 0, 0)
    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert lib.tamp_amd_compress_plan(window, max_in_len, 1, *[ctypes.byref(x) for x in v]) == 0
    return lib.tamp_amd_compress_build(ctypes.byref(conf), max_in_len, flags, 0), v[0].value, v[2].value


def run_batch(ta, oracle, golden, cases, route, max_in_len, **dict_kw):
    """One device-memory batch of ``cases`` (one configuration): status, length and bytes of every stream as the reference's, and the
    device decoder gives the streams that were served their input back."""
    import torch
    from tamp_amd.batch import compress_bound, pack_streams

    c0 = cases[0]
    window, literal, extended = c0.window, c0.literal, c0.extended
    wants = [want(oracle, golden, c) for c in cases]
    flat, off, ln = pack_streams([c.data for c in cases])
    dev = torch.device("cuda:0")
    data = torch.from_numpy(np.array(flat, dtype=np.uint8)).to(dev)
    off_t, len_t = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev)
    longest = max(len(c.data) for c in cases)
    res = ta.compress_batch(data, off_t, len_t, window=window, literal=literal, extended=extended, lazy_matching=True, max_in_len=max_in_len,
                            out_cap=compress_bound(longest, literal), **dict_kw)
    torch.cuda.synchronize()
    status, out_len = res.status.cpu().numpy(), res.out_len.cpu().numpy()
    out, out_off = res.out.cpu().numpy(), res.out_off.cpu().numpy()
    for i, (c, (rc, blob)) in enumerate(zip(cases, wants)):
        where = (config_id(window, literal, extended), c.name, c.cell, route)
        assert int(status[i]) == rc, (*where, "status", int(status[i]), rc)
        assert int(out_len[i]) == len(blob), (*where, "length", int(out_len[i]), len(blob))
        assert out[int(out_off[i]):int(out_off[i]) + len(blob)].tobytes() == blob, (*where, "bytes")
    back = ta.decompress_batch(res.out, res.out_off, res.out_len, out_cap=longest + 8, **dict_kw)
    torch.cuda.synchronize()
    bstatus, blen = back.status.cpu().numpy(), back.out_len.cpu().numpy()
    bout, boff = back.out.cpu().numpy(), back.out_off.cpu().numpy()
    for i, (c, (rc, _)) in enumerate(zip(cases, wants)):
        if rc == 0:
            where = (config_id(window, literal, extended), c.name, c.cell, route, "round trip")
            assert int(bstatus[i]) == 2, (*where, int(bstatus[i]))
            assert bout[int(boff[i]):int(boff[i]) + int(blen[i])].tobytes() == c.data, where


# ---------------------------------------------------------------------------------------------------------------------
# batch builds: every case without a dictionary, one batch per configuration and size
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [li.BARE, li.LED])
@pytest.mark.parametrize("window,literal,extended", CONFIGS, ids=[config_id(*c) for c in CONFIGS])
def test_batch_builds(ta, oracle, golden, window, literal, extended, size):
    """kLazyPacked (windows up to 2^14) and kLazyU16 (2^15): the bare sizes with max_in_len under 1 KiB, one wavefront; the led sizes
    (and the epoch-edge streams) with four."""
    cases = [c for c in li.cases(window, literal, extended) if c.dictionary is None and c.size == size]
    assert cases
    max_in_len = max(len(c.data) for c in cases)
    assert max_in_len < 1024 if size == li.BARE else min(len(c.data) for c in cases) >= 1088
    build, _, threads = planned(window, literal, extended, max_in_len)
    assert (build, threads) == (GENERIC, 64 if size == li.BARE else 256), (window, literal, extended, size)
    run_batch(ta, oracle, golden, cases, f"batch {size}", max_in_len)


# ---------------------------------------------------------------------------------------------------------------------
# dictionaries: the cases that carry one, with a shared dictionary and through the dictionary table
# ---------------------------------------------------------------------------------------------------------------------
DICT_CONFIGS = tuple(c for c in CONFIGS if c[1] == 8 or c[:2] == (12, 7))


@pytest.mark.parametrize("size", [li.BARE, li.LED])
@pytest.mark.parametrize("window,literal,extended", DICT_CONFIGS, ids=[config_id(*c) for c in DICT_CONFIGS])
def test_dictionary_cases(ta, oracle, golden, window, literal, extended, size):
    """The overlap cells (d) and whatever else needs bytes ahead of window_pos: once through dictionaries=[...] / dictionary_index=
    with every distinct dictionary in ONE launch (the table twins), once per distinct dictionary as dictionary= (every case of (d) with
    the dictionary it shares with nothing that could hide its decision)."""
    every = [c for c in li.cases(window, literal, extended) if c.dictionary is not None]
    cases = [c for c in every if c.size == size]
    assert cases and (literal == 7 or sum(c.cell.startswith("d.") for c in cases) == 2 * len(li.OVERLAP_K))
    dicts = sorted({c.dictionary for c in cases})
    if len(dicts) < 3 and literal == 8:  # a lead that laps the window leaves nothing of the dictionary to differ in: the bare cases ride along
        assert size == li.LED and window <= 10
        cases, dicts = every, sorted({c.dictionary for c in every})
    assert len(dicts) >= 3 or literal == 7
    max_in_len = max(len(c.data) for c in cases)
    build, _, threads = planned(window, literal, extended, max_in_len, CALL_DICT_TABLE)
    assert (build, threads) == (GENERIC, 64 if size == li.BARE else 256)
    run_batch(ta, oracle, golden, cases, f"dictionary table {size}", max_in_len, dictionaries=dicts,
              dictionary_index=[dicts.index(c.dictionary) for c in cases])
    for d in dicts:
        run_batch(ta, oracle, golden, [c for c in cases if c.dictionary == d], f"shared dictionary {size}", max_in_len, dictionary=d)


# ---------------------------------------------------------------------------------------------------------------------
# epoch edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", [64, 128, 192, 512, None])
@pytest.mark.parametrize("extended", [True, False], ids=["ext", "v1"])
@pytest.mark.parametrize("window", [10, 15])
def test_epoch_edges(ta, oracle, golden, monkeypatch, window, extended, blk):
    """j: a defer (and a chain of two) every 37 positions, under epochs of 64, 128 and 192 positions (one wavefront), 512 (four) and
    the launcher's own choice: cached states at every lane of the walk's blocks and every distance to an epoch's end."""
    if blk is not None:
        monkeypatch.setenv("TAMP_AMD_BLK", str(blk))
    cases = [c for c in li.cases(window, 8, extended) if c.cell.startswith("j.")]
    assert len(cases) == 2
    max_in_len = max(len(c.data) for c in cases)
    build, got_blk, threads = planned(window, 8, extended, max_in_len)
    assert build == GENERIC and threads == (64 if blk in (64, 128, 192) else 256), (blk, got_blk, threads)
    if blk is not None:
        assert got_blk == blk
    run_batch(ta, oracle, golden, cases, f"TAMP_AMD_BLK={blk}", max_in_len)


# ---------------------------------------------------------------------------------------------------------------------
# whole segments with state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", [True, False], ids=["ext", "v1"])
@pytest.mark.parametrize("window", [8, 10, 15])
def test_compressor_object_segments(ta, oracle, window, extended):
    """Compressor(lazy_matching=True): write, flush(write_token=True), write, close -- the flush falls between a deferred literal and
    its cached match, so the first segment ends on the literal and the second starts without a cached state."""
    src, marks = li.sweep_source(window, extended)
    for cell in ("a.defer", "f.chain3", "g.run", "e.ext15"):
        at = next(pos for pos, _, name in marks if name == cell)
        for cut in (at, at + 1, at + 2):
            ops = [("write", src[:cut]), ("flush", True), ("write", src[cut:]), ("close",)]
            rc, blob = oracle.stream_script(ops, window=window, literal=8, extended=extended, lazy_matching=True)
            assert rc == 0
            f = io.BytesIO()
            c = ta.Compressor(f, window=window, literal=8, extended=extended, lazy_matching=True)
            c.write(src[:cut])
            c.flush(write_token=True)
            c.write(src[cut:])
            c.close()
            assert f.getvalue() == blob, (config_id(window, 8, extended), cell, "Compressor, flush at", cut)


def reset_script(data, interval):
    ops = []
    for at in range(0, max(len(data), 1), interval):
        if at:
            ops.append(("reset",))
        ops.append(("write", data[at:at + interval]))
    return ops + [("flush", False)]


@pytest.mark.parametrize("extended", [True, False], ids=["ext", "v1"])
@pytest.mark.parametrize("window", [8, 10, 15])
def test_dictionary_reset_segments(ta, oracle, window, extended):
    """compress_batch(dictionary_reset=True, reset_interval=N, lazy_matching=True) on the sweep stream, N chosen so that a cut falls
    one byte behind a defer (and, by the other segments, anywhere in other cells): the oracle's script, segment by segment."""
    src, marks = li.sweep_source(window, extended)
    intervals = [next(pos for pos, _, name in marks if name == cell) + 1 for cell in ("a.defer", "b.len8", "f.chain2")]
    defers = {pos for pos, e, _ in marks if e.get("event") == "defer"}
    assert all(n - 1 in defers for n in intervals)  # the first segment ends on a deferred literal
    res = [ta.compress_batch([src], window=window, literal=8, extended=extended, dictionary_reset=True, reset_interval=n, lazy_matching=True,
                             max_in_len=len(src)) for n in intervals]
    kw = dict(window=window, literal=8, extended=extended, dictionary_reset=True, lazy_matching=True)
    for n, r in zip(intervals, res):
        ops = reset_script(src, n)
        rc, blob = oracle.stream_script(ops, **kw)
        assert rc == 0 and int(r.status[0]) == 0
        got, at = r.stream(0), 0
        for seg, end in enumerate([k + 1 for k, op in enumerate(ops) if op[0] == "reset"]):  # the script up to each reset
            rc, part = oracle.stream_script(ops[:end], **kw)
            assert rc == 0 and blob.startswith(part) and len(part) > at
            assert got[at:len(part)] == part[at:], (config_id(window, 8, extended), "reset_interval", n, "segment", seg)
            at = len(part)
        assert got == blob


# ---------------------------------------------------------------------------------------------------------------------
# the resume kernel, cut at every byte
# ---------------------------------------------------------------------------------------------------------------------
def describe(marks, c):
    near = [(pos, name) for pos, _, name in marks if pos - 1 <= c <= pos + 16]
    return f"cut {c}" + (f" ({', '.join(f'{name} decides at {pos}' for pos, name in near[:2])})" if near else "")


@pytest.mark.parametrize("window,extended", SWEEPS, ids=[f"w{w}-{'ext' if e else 'v1'}" for w, e in SWEEPS])
def test_resume_kernel_every_cut(ta, oracle, golden, window, extended):
    """EncoderBatch(lazy_matching=True): object c compresses src[:c], then compresses src[c:] and flushes -- one object per cut, two
    launches.  Per call and per object the reference object's (status, bytes written, consumed) of the fixture; the joined bytes
    are the one-shot stream, whose cached matches therefore survived every cut in the object's state."""
    src, marks = li.sweep_source(window, extended)
    rec = next(r for r in golden["sweep"] if (r["window"], r["extended"]) == (window, extended))
    rc, whole = oracle.compress(src, window=window, literal=8, extended=extended, lazy_matching=True)
    assert rc == 0 and rec["input_sha256"] == hashlib.sha256(src).hexdigest() and rec["whole_sha256"] == hashlib.sha256(whole).hexdigest()
    n = len(src)
    assert len(rec["cuts"]) == n + 1 and rec["cap"] == CAP
    t0 = time.perf_counter()
    enc = ta.EncoderBatch(n + 1, window=window, literal=8, extended=extended, lazy_matching=True)
    st1, out1, k1 = enc.compress([src[:c] for c in range(n + 1)], CAP)
    cached = enc.states[:, 28:34].copy()  # cached_match_index (int16) .. cached_match_size (byte 32), for the message
    st2, out2, k2 = enc.compress_and_flush([src[c:] for c in range(n + 1)], CAP, write_token=False)
    print(f"lazy cut sweep w{window}-{'ext' if extended else 'v1'}: {n + 1} cuts, 2 launches, {time.perf_counter() - t0:.2f} s")
    name = f"w{window}-{'ext' if extended else 'v1'}"
    for c, (ws1, wl1, wk1, ws2, wl2, wk2) in enumerate(rec["cuts"]):
        state = f"cached match index {int(cached[c, :2].view(np.int16)[0])} size {int(cached[c, 4])}"
        where = f"{name}: {describe(marks, c)}, {state}"
        assert (int(st1[c]), len(out1[c]), int(k1[c])) == (ws1, wl1, wk1), (where, "first call")
        assert out1[c] == whole[:wl1], (where, "bytes of the first call")
        assert (int(st2[c]), len(out2[c]), int(k2[c])) == (ws2, wl2, wk2), (where, "second call")
        assert out2[c] == whole[wl1:], (where, "bytes of the second call")
    held = (np.ascontiguousarray(cached[:, :2]).view(np.int16)[:, 0] >= 0) & (cached[:, 4] > 0)
    assert held.sum() >= 5, "no object was cut while it held a cached match"
