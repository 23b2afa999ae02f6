"""GPU tier: the fixed-geometry compress builds, whose wavefronts take the match phase's sorted query groups from a counter in LDS
(kClaim in tamp_compress_kernel.hpp), against the reference C (the oracle where that was not built): status, length and bytes of
every stream.  TAMP_AMD_FIXED_BUILD=0 sends the same calls through the generic build, which keeps the strided loop: the same bytes.

What a query computes does not depend on which wavefront runs it, so the output is bit for bit what it was; what can go wrong is
the hand-out itself -- a group taken twice or not at all, a partial last group, a counter that is not back at zero for the next
epoch or the next stream of a persistent workgroup, the second pass over listed runs reading a first-pass result that another
wavefront has not stored yet.  The batches therefore mix, a few hundred streams each:

  lengths   1, 2, 17, 63, 64, 65, 255, 256, 257, 1,023, 1,024, 1,025, 1,088, 2,047, 2,048, 4,095, 4,096 (up to max_in_len): epochs
            with fewer queries than one group of 64, exactly one group, one more, a partial last group, and with 1,024-position
            blocks, epochs that start with pending positions of the one before;
  contents  the benchmark's synthetic text; one bigram every third position (a third of the brackets at the cap of 63: the first
            groups dwarf the rest); bytes without a repeated bigram (every group is done at once); long runs of one byte between
            text (the run list, the second pass and its barrier, the epoch cut); runs of 2..6 of one byte between other bytes (a
            crowded bucket: deferred positions).

Each batch also runs with one workgroup per CU (TAMP_AMD_GRID_PER_CU=1), so that a persistent workgroup goes through several streams
and many epochs on the same two counter words.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1088, 2047, 2048, 4095, 4096)
KINDS = ("text", "bigram", "unique", "long_runs", "short_runs")
TUNING_ENV = ("TAMP_AMD_BLK", "TAMP_AMD_RUNS", "TAMP_AMD_FIXED_BUILD", "TAMP_AMD_CUT_RUN", "TAMP_AMD_LPT", "TAMP_AMD_STATIC_GRID",
              "TAMP_AMD_BLOCK_MIN", "TAMP_AMD_GRID_PER_CU")


def unique_bigrams(n):
    """n <= 4,096 bytes in which no bigram occurs twice: for d = 2..9 the pairs (a, a + d), a = 0..255, follow each other, so the
    bigrams are (a, a + d) and (a + d, a + 1): byte differences d and 1 - d, each first byte once per difference."""
    a = np.arange(256, dtype=np.uint32)
    s = np.concatenate([np.stack([a, a + d], axis=1).reshape(-1) for d in range(2, 10)]).astype(np.uint8)
    pairs = s[:-1].astype(np.uint32) * 256 + s[1:]
    assert len(np.unique(pairs)) == len(pairs)
    return s[:n]


def content(kind, n, seed, text):
    rng = np.random.default_rng(1000 + seed)
    if kind == "text":
        return text[seed % len(text)][:n].copy()
    if kind == "bigram":  # "qz" and one byte that varies
        s = np.empty(3 * ((n + 2) // 3), dtype=np.uint8)
        s[0::3], s[1::3], s[2::3] = ord("q"), ord("z"), rng.integers(32, 127, size=len(s) // 3)
        return s[:n]
    if kind == "unique":
        return np.roll(unique_bigrams(4096), 512 * (seed % 8))[:n].copy()
    out = []
    total = 0
    while total < n:
        if kind == "long_runs":  # 20..400 equal bytes, then 10..200 bytes of text
            k = int(rng.integers(10, 200))
            o = int(rng.integers(0, 4096 - k))
            piece = [np.full(int(rng.integers(20, 400)), rng.choice([ord(" "), ord("x"), 0]), dtype=np.uint8), text[(seed + total) % len(text)][o:o + k]]
        else:  # runs of 2..6 of one byte, one or two other bytes between them
            piece = [np.full(int(rng.integers(2, 7)), ord("e"), dtype=np.uint8), rng.integers(97, 123, size=int(rng.integers(1, 3))).astype(np.uint8)]
        out += piece
        total += sum(len(p) for p in piece)
    return np.concatenate(out)[:n]


_batches = {}


def batch_for(max_in_len):
    """(flat, in_off, in_len) of the one batch per max_in_len, made once and never modified."""
    if max_in_len not in _batches:
        from tamp_amd import workloads as wl

        text = wl.synth_text(8, 4096)
        lengths = [n for n in LENGTHS if n <= max_in_len]
        reps = 6 if max_in_len == 4096 else 8
        streams = [content(kind, n, r, text) for r in range(reps) for n in lengths for kind in KINDS]
        order = np.random.default_rng(max_in_len).permutation(len(streams))
        streams = [streams[i] for i in order]
        ln = np.array([len(s) for s in streams], dtype=np.int64)
        assert sorted(set(ln.tolist())) == lengths and 300 <= len(streams) <= 600
        off = np.concatenate([[0], np.cumsum(ln)[:-1]])
        _batches[max_in_len] = (np.concatenate(streams), off, ln)
    return _batches[max_in_len]


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


_want = {}


@pytest.fixture(scope="module")
def want(checker):
    """The checker's streams per (max_in_len, format), computed once."""
    def get(max_in_len, extended):
        if (max_in_len, extended) not in _want:
            flat, off, ln = batch_for(max_in_len)
            r = checker.compress_batch(flat, off, ln, window=10, literal=8, extended=extended, threads=8)
            assert (np.asarray(r.status) == 0).all()
            _want[(max_in_len, extended)] = [r.stream(i) for i in range(len(ln))]
        return _want[(max_in_len, extended)]
    return get


def planned_build(extended, max_in_len):
    from tamp_amd import _lib

    conf = _lib.TampAmdConf(10, 8, 0, int(extended), 0, 0, 0, 0)
    return _lib.load().tamp_amd_compress_build(ctypes.byref(conf), max_in_len, 0, 0)


def compress(ta, max_in_len, extended):
    import torch
    from tamp_amd.batch import compress_bound

    flat, off, ln = batch_for(max_in_len)
    dev = torch.device("cuda:0")
    data = torch.from_numpy(np.ascontiguousarray(flat)).to(dev)
    off_t, len_t = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev)
    res = ta.compress_batch(data, off_t, len_t, window=10, literal=8, extended=extended, max_in_len=max_in_len,
                            out_cap=compress_bound(max_in_len, 8))
    torch.cuda.synchronize()
    status, out_len = res.status.cpu().numpy(), res.out_len.cpu().numpy()
    out, out_off = res.out.cpu().numpy(), res.out_off.cpu().numpy()
    return status, [out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(len(ln))]


def check(max_in_len, status, got, want):
    ln = batch_for(max_in_len)[2]
    assert (status == 0).all(), ("status", [(int(i), int(ln[i]), int(status[i])) for i in np.flatnonzero(status)][:4])
    bad = [(i, int(ln[i]), len(got[i]), len(want[i])) for i in range(len(ln)) if got[i] != want[i]]
    assert not bad, ("streams that differ (index, input length, length, reference length)", len(bad), bad[:6])


CASES = [(L, e) for L in (1024, 4096) for e in (True, False)]
IDS = ["%d-%s" % (L, "ext" if e else "v1") for L, e in CASES]


@pytest.mark.parametrize("max_in_len,extended", CASES, ids=IDS)
def test_fixed_builds_give_the_reference_bytes(ta, want, max_in_len, extended):
    assert planned_build(extended, max_in_len) == (1 if extended else 2), "the fixed-geometry build"
    status, got = compress(ta, max_in_len, extended)
    check(max_in_len, status, got, want(max_in_len, extended))


@pytest.mark.parametrize("max_in_len,extended", CASES, ids=IDS)
def test_one_workgroup_per_cu_runs_several_streams_on_its_counters(ta, want, max_in_len, extended, monkeypatch):
    monkeypatch.setenv("TAMP_AMD_GRID_PER_CU", "1")
    assert planned_build(extended, max_in_len) == (1 if extended else 2), "the fixed-geometry build"
    status, got = compress(ta, max_in_len, extended)
    check(max_in_len, status, got, want(max_in_len, extended))


@pytest.mark.parametrize("max_in_len,extended", CASES, ids=IDS)
def test_generic_build_gives_the_same_bytes(ta, want, max_in_len, extended, monkeypatch):
    monkeypatch.setenv("TAMP_AMD_FIXED_BUILD", "0")
    assert planned_build(extended, max_in_len) == 0, "a generic build"
    status, got = compress(ta, max_in_len, extended)
    check(max_in_len, status, got, want(max_in_len, extended))
