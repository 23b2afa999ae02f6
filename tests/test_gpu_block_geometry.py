"""GPU tier: the compress kernel's bytes at every block size the launcher can pick (block size and epoch cuts
are policy, "about cost and never about bytes").

Everything in the kernel is sized from the epoch block -- the LDS layout, the index tiles and a part-filled last one, the
64-position jump-table blocks, the token list, the bit buffer, the rebase test -- and the launcher derives the block from
max_in_len, the window and the build.  Three sweeps, every stream against the reference C / the oracle (status, length,
bytes) and once through the device decoder:
  a) TAMP_AMD_BLK, the launcher's own block override, at every multiple of 64 a configuration admits: an epoch boundary at
     every multiple of 64 of a 4.6 KB stream, under inputs whose features recur at periods coprime to 64 (block_draggers);
  b) no environment: max_in_len in {64k, 64k + 1} for k = 1..32, every window, both parses, both formats -- every block a
     window can reach, and the lengths that leave a second epoch of one position;
  c) max_in_len far below the streams' lengths (include/tamp_amd.h: the bound only sizes the block).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

from block_draggers import CUT_NAMES, cut_lengths, draggers, masked  # noqa: E402

N_LONG, N_SHORT = 4625, 960  # (4,625: more than two of the largest blocks plus the look-ahead)
TUNING_ENV = ("TAMP_AMD_BLK", "TAMP_AMD_RUNS", "TAMP_AMD_FIXED_BUILD", "TAMP_AMD_CUT_RUN", "TAMP_AMD_LPT", "TAMP_AMD_STATIC_GRID",
              "TAMP_AMD_BLOCK_MIN", "TAMP_AMD_GRID_PER_CU")


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


@pytest.fixture(scope="module")
def checker():
    from oracle.checker import Oracle, Ref

    return Ref() if Ref.available() else Oracle()


@pytest.fixture(autouse=True)
def no_tuning_env(monkeypatch):
    for k in TUNING_ENV:
        monkeypatch.delenv(k, raising=False)


def plan(window, max_in_len, lazy):
    """-> (block, LDS bytes, threads, workgroups per CU) as the launcher would choose them under the current environment."""
    from tamp_amd import _lib

    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert _lib.load().tamp_amd_compress_plan(window, max_in_len, int(lazy), *[ctypes.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


# ---- inputs and expected bytes, computed once and shared (never modified) -------------------------------------------
_sources, _expected, _dicts = {}, {}, {}


def source(name, literal):
    """Dragger `name` at the longest length any test uses, masked to `literal` bits; tests take prefixes of it."""
    if literal not in _sources:
        _sources[literal] = {k: masked(v, literal) for k, v in draggers(N_LONG).items()}
    return _sources[literal][name]


def prose_dictionary(window):
    if window not in _dicts:
        from tamp_amd import workloads as wl

        _dicts[window] = wl.real_text("prose", frozen_only=True)[50021:50021 + (1 << window)]
        assert len(_dicts[window]) == 1 << window
    return _dicts[window]


def conf_key(conf):
    return (conf["window"], conf.get("literal", 8), bool(conf["extended"]), bool(conf.get("lazy_matching")), bool(conf.get("custom")))


def expected(checker, conf, items):
    """{(name, length): bytes} for `items` under `conf`: what is missing goes to the checker in ONE batch."""
    from tamp_amd.batch import pack_streams

    window, literal, extended, lazy, custom = key = conf_key(conf)
    have = _expected.setdefault(key, {})
    todo = sorted({it for it in items if it not in have})
    if todo:
        flat, off, ln = pack_streams([source(name, literal)[:n] for name, n in todo])
        want = checker.compress_batch(flat, off, ln, window=window, literal=literal, extended=extended, lazy=lazy,
                                      dictionary=prose_dictionary(window) if custom else None, threads=8)
        assert (np.asarray(want.status) == 0).all(), (key, "the checker refuses an input")
        for i, it in enumerate(todo):
            have[it] = want.stream(i)
    return have


def run_batch(ta, conf, items, want, max_in_len, what, run_aware=None):
    """One device batch of `items` = [(name, length)]: status 0, length and bytes as `want`, and the device decoder gives
    the input back.  -> number of streams compared."""
    import torch
    from tamp_amd.batch import compress_bound, pack_streams

    window, literal, extended, lazy, custom = conf_key(conf)
    streams = [source(name, literal)[:n] for name, n in items]
    longest = max(len(s) for s in streams)
    flat, off, ln = pack_streams(streams)
    dev = torch.device("cuda:0")
    data = torch.from_numpy(np.ascontiguousarray(flat)).to(dev)
    off_t, len_t = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev)
    dictionary = prose_dictionary(window) if custom else None
    res = ta.compress_batch(data, off_t, len_t, window=window, literal=literal, extended=extended, lazy_matching=lazy,
                            dictionary=dictionary, max_in_len=max_in_len, out_cap=compress_bound(longest, literal),
                            run_aware=run_aware)
    torch.cuda.synchronize()
    status, out_len = res.status.cpu().numpy(), res.out_len.cpu().numpy()
    out, out_off = res.out.cpu().numpy(), res.out_off.cpu().numpy()
    assert (status == 0).all(), (what, "status", [(items[i], int(status[i])) for i in np.flatnonzero(status)][:4])
    for i, it in enumerate(items):
        assert int(out_len[i]) == len(want[it]), (what, it, "length", int(out_len[i]), len(want[it]))
        got = out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes()
        assert got == want[it], (what, it, "bytes")
    back = ta.decompress_batch(res.out, res.out_off, res.out_len, out_cap=longest + 8, dictionary=dictionary)
    torch.cuda.synchronize()
    bstatus, blen = back.status.cpu().numpy(), back.out_len.cpu().numpy()
    bout, boff = back.out.cpu().numpy(), back.out_off.cpu().numpy()
    assert (bstatus == 2).all(), (what, "decoder status")
    for i, s in enumerate(streams):
        assert bout[int(boff[i]):int(boff[i]) + int(blen[i])].tobytes() == s, (what, items[i], "round trip")
    return len(items)


# ---- a) the block override: bytes do not depend on the block ---------------------------------------------------------
def _cfg(tag, parts=1, min_blocks=30, **conf):
    return [pytest.param(conf, part, parts, min_blocks, id="%s-%s%s" % (tag, "ext" if conf["extended"] else "v1",
                                                                         "-%d" % part if parts > 1 else "")) for part in range(parts)]


def _both(tag, **kw):
    return _cfg(tag, extended=True, **kw) + _cfg(tag, extended=False, **kw)


# (the 2^15 window costs the checker several seconds per sweep: its blocks are swept in four parts)
LONG = (_both("w8-runs", window=8)                       # block far larger than the window: ring-end cuts
        + _both("w10-runs", window=10, min_blocks=16)    # 1,024 buckets: pick_block caps the block at 1,024, where the fixed build takes over
        + _both("w12-runs", window=12)                   # window larger than the block
        + _cfg("w12-lit5", window=12, literal=5, extended=True)            # minimum match 3, inputs masked
        + _cfg("w10-dict", window=10, custom=True, extended=True, min_blocks=16)  # (run-aware with 1,024 buckets as well)
        + _both("w15-lean", window=15, parts=4)          # u16 index entries
        + _both("w10-lazy", window=10, lazy_matching=True) + _both("w12-lazy", window=12, lazy_matching=True)
        + _cfg("w15-lazy", window=15, lazy_matching=True, extended=True, parts=4))


def sweep_override(ta, checker, monkeypatch, conf, n, m, envs, part, parts, min_blocks, run_aware=None, two_blocks_up_to=2048):
    window, literal, extended, lazy, custom = conf_key(conf)
    eff = {}  # effective block -> the override that gives it
    for v in envs:
        monkeypatch.setenv("TAMP_AMD_BLK", str(v))
        eff.setdefault(plan(window, n, lazy)[0], v)
    assert len(eff) >= min_blocks, (sorted(eff), "the override does not reach enough blocks")
    assert all(b % 64 == 0 and 64 <= b <= 2048 for b in eff)
    names = list(draggers(64))
    mine = sorted(eff)[part::parts]
    batches = {b: [(k, n) for k in names] + [(k, c) for k in CUT_NAMES for c in cut_lengths(b, m, n)] for b in mine}
    want = expected(checker, conf, [it for items in batches.values() for it in items])
    compared = 0
    for b, items in batches.items():
        if b <= two_blocks_up_to:
            assert max(c for _, c in items) > 2 * b, (b, "no stream longer than two blocks")
        monkeypatch.setenv("TAMP_AMD_BLK", str(eff[b]))
        assert plan(window, n, lazy)[0] == b
        compared += run_batch(ta, conf, items, want, n, (conf, "TAMP_AMD_BLK", eff[b], "block", b), run_aware=run_aware)
    print("override sweep %s: %d blocks, %d streams compared" % (conf, len(mine), compared))


@pytest.mark.parametrize("conf,part,parts,min_blocks", LONG)
def test_override_sweep_long_streams(ta, checker, monkeypatch, conf, part, parts, min_blocks):
    sweep_override(ta, checker, monkeypatch, conf, N_LONG, 2, range(64, 2049, 64), part, parts, min_blocks)


SHORT = [pytest.param(dict(window=w, literal=lit, extended=ext, lazy_matching=lazy), ra,
                      id="w%d-lit%d-%s-%s" % (w, lit, "lazy" if lazy else ("runs" if ra else "lean"), "ext" if ext else "v1"))
         for (w, lit, lazy, ra) in ((10, 8, False, None), (8, 7, False, None), (10, 8, False, True), (8, 7, False, True), (10, 8, True, None))
         for ext in (True, False)]


@pytest.mark.parametrize("conf,run_aware", SHORT)
def test_override_sweep_short_messages(ta, checker, monkeypatch, conf, run_aware):
    """max_in_len = 960: one-wavefront workgroups (the short-message kernel, which is no persistent grid; its run-aware and lazy
    siblings) through several blocks per message -- without the override only a lag makes them start a second epoch."""
    sweep_override(ta, checker, monkeypatch, conf, N_SHORT, 1, range(64, 961, 64), 0, 1, 15, run_aware=run_aware, two_blocks_up_to=448)


def test_short_message_build_refuses_a_256_thread_block(ta, monkeypatch):
    """The lean short-message build exists for one wavefront only: a block override of 1,024 positions is refused, nothing is launched."""
    import torch
    from tamp_amd import _lib
    from tamp_amd.batch import pack_streams

    flat, off, ln = pack_streams([source(k, 8)[:N_SHORT] for k in ("text", "runs67", "random")])
    dev = torch.device("cuda:0")
    args = (torch.from_numpy(np.ascontiguousarray(flat)).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
            torch.from_numpy(ln.astype(np.int32)).to(dev))
    monkeypatch.setenv("TAMP_AMD_BLK", "1024")
    assert plan(10, N_SHORT, False)[0] == 1024 and plan(10, N_SHORT, False)[2] == 256
    with pytest.raises(ValueError):
        ta.compress_batch(*args, window=10, max_in_len=N_SHORT)
    assert b"no lean build for 256-thread workgroups" in _lib.load().tamp_amd_last_error()
    monkeypatch.delenv("TAMP_AMD_BLK")
    ok = ta.compress_batch(*args, window=10, max_in_len=N_SHORT)
    torch.cuda.synchronize()
    assert (ok.status.cpu().numpy() == 0).all()


# ---- b) the launcher's own choices -------------------------------------------------------------------------------------
AUTO_LENS = [n for k in range(1, 33) for n in (64 * k, 64 * k + 1)]
ENUMERATION = list(range(0, 4200)) + [4625, 8192, 65536, 1 << 20]


def _auto_params():
    out = []
    for lazy in (False, True):
        for window in range(8, 16):
            parts = 4 if window >= 14 else 1  # (the large windows cost the checker most)
            for ext in (True, False):
                for part in range(parts):
                    out.append(pytest.param(window, lazy, ext, part, parts, id="w%d-%s-%s%s" % (
                        window, "lazy" if lazy else "default", "ext" if ext else "v1", "-%d" % part if parts > 1 else "")))
    return out


@pytest.mark.parametrize("window,lazy,extended,part,parts", _auto_params())
def test_blocks_the_launcher_picks(ta, checker, window, lazy, extended, part, parts):
    assert "TAMP_AMD_BLK" not in os.environ
    reachable = {plan(window, n, lazy)[0] for n in ENUMERATION}
    picked = {n: plan(window, n, lazy)[0] for n in AUTO_LENS}
    assert len(set(picked.values())) >= len(reachable) and set(picked.values()) <= reachable, (sorted(reachable), sorted(set(picked.values())))
    conf = dict(window=window, extended=extended, lazy_matching=lazy)
    names = list(draggers(64))
    mine = AUTO_LENS[part::parts]
    batches = {n: [(k, n) for k in names] + [("text", n - d) for d in (1, 15, 16, 17)] for n in mine}
    want = expected(checker, conf, [it for items in batches.values() for it in items])
    compared = 0
    for n, items in batches.items():
        compared += run_batch(ta, conf, items, want, n, (conf, "max_in_len", n, "block", picked[n]))
        if n <= 960 and not lazy:
            compared += run_batch(ta, conf, items, want, n, (conf, "max_in_len", n, "run_aware"), run_aware=True)
    print("launcher's choice %s: %d blocks of %d reachable, %d streams compared" % (conf, len({picked[n] for n in mine}), len(reachable), compared))


# ---- c) an understated bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", [True, False])
def test_understated_max_in_len(ta, checker, extended):
    """max_in_len is an upper bound the library cannot check for device memory: it sizes the block and picks the build, nothing
    else.  4,625-byte streams under bounds of 100 (lean one-wavefront build, 128-position blocks), 1,000 and 1,500 bytes (run-aware
    build, 1,024-position blocks) give the reference's bytes."""
    conf = dict(window=10, extended=extended)
    items = [(k, N_LONG) for k in draggers(64)]
    want = expected(checker, conf, items)
    for bound in (100, 1000, 1500):
        run_batch(ta, conf, items, want, bound, (conf, "understated max_in_len", bound))
