"""GPU tier (-m gpu): decode with too little output room, on every build of every batch decoder.

The rule (include/tamp_amd.h, tamp_batch_decompress; tests/tight_decode_input.rule): with (S, X, K) = a stream's status, bytes
and consumed count with ample room and N = len(X), a slab of ``cap`` bytes gets (TAMP_OUTPUT_FULL, X[:cap]) when ``cap < N``,
exactly (S, X, K) when ``cap > N``, and all of X with S or TAMP_OUTPUT_FULL when ``cap == N``; nothing is written in front of a
slab, behind its ``out_len`` produced bytes, or at or behind its end.  Every build has a fast path gated on the remaining room
and a hand-over to the reference-exact loop where room runs short, and stores in wide units whose shape follows the slab's address.

One SWEEP is one tamp_batch_decompress call through ctypes: the same compressed stream once per capacity, slab ``j`` with
``cap = j`` for ``j = 0 .. N + 2``, the slabs back to back behind 3 guard bytes (slab starts are triangular numbers: every
residue mod 16), 64 guard bytes behind the last.  The output buffer holds a position-dependent pattern and the three tables
poison values before the call; afterwards status, length and consumed count are compared per slab and the buffer WHOLE: the
expected prefixes where they belong, the pattern everywhere else (tests/tight_check.py; tests/test_tight_check.py proves that
comparison can fail).  Every expectation is the oracle's at that capacity (pinned to the reference at every capacity by
tests/test_oracle_vs_reference.py), never a result of the GPU's own.  Each case forces its decoder and then asks
tamp_amd_decompress_plan, with the batch's own facts, whether the call reached the build the case is named for.
Inputs: tests/tight_decode_input.py (their properties: tests/test_tight_decode_input.py).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tight_decode_input as tdi  # noqa: E402
from tight_check import check_call, slab_layout  # noqa: E402

pytestmark = pytest.mark.gpu

MEM_HOST, MEM_DEVICE = 0, 1
SPLIT, WAVE, LANE_LDS, LANE_GLOBAL = 0, 1, 2, 3  # include/tamp_amd.h TAMP_AMD_DECODER_*
TUNING_ENV = ("TAMP_AMD_DECODER", "TAMP_AMD_SPLIT_SLICE_LOG2", "TAMP_AMD_SPLIT_SCRATCH_MB", "TAMP_AMD_SPLIT_WAVE_MAX",
              "TAMP_AMD_SPLIT_SPW", "TAMP_AMD_SCRATCH_MB", "TAMP_AMD_LONGDEC", "TAMP_AMD_LONGDEC_MIN", "TAMP_AMD_SPLIT_FAIL_ABOVE")
MIN_STREAMS = 256  # from here on a call runs the header pre-pass, and the split decoder is within reach
POISON_LEN, POISON_STATUS, POISON_CONSUMED = 0x7FFFFFFF, 99, 0x7FFFFFFE


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    lib = _lib.load()  # raises if the native library is missing: no silent fallback
    assert lib.tamp_amd_device_count() >= 1, "no HIP device visible"
    return lib


@pytest.fixture(autouse=True)
def unforced(monkeypatch):
    for k in TUNING_ENV:
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------------------------------------------------------------
# expectations: one oracle sweep per stream, shared by every test that runs it
# ---------------------------------------------------------------------------------------------------------------------
class Sweep:
    """A stream once per capacity 0 .. N + 2 (then copies with ample room up to MIN_STREAMS) and the oracle's result per slab."""

    def __init__(self, oracle, case):
        self.case = case
        self.full = oracle.decompress(case.blob, dictionary=case.dictionary, cap=1 << 16)
        self.N = N = len(self.full[1])
        caps = list(range(N + 3)) + [N + 8] * max(0, MIN_STREAMS - (N + 3))
        self.caps = np.array(caps, dtype=np.uint32)
        want = [oracle.decompress(case.blob, dictionary=case.dictionary, cap=c) for c in caps]
        self.status = np.array([w[0] for w in want], dtype=np.int64)
        self.streams = [w[1] for w in want]
        self.out_len = np.array([len(s) for s in self.streams], dtype=np.int64)
        self.consumed = np.array([w[2] for w in want], dtype=np.int64)
        for c, w in zip(caps, want):  # (the oracle states the rule; the CPU tier holds the reference to the same)
            assert tdi.obeys(self.full, c, w), ("oracle off the rule", case.name, c)
        self.pairs = len(caps)


_sweeps = {}


def sweep_of(oracle, name):
    if name not in _sweeps:
        _sweeps[name] = Sweep(oracle, tdi.cases(oracle)[name])
    return _sweeps[name]


class Batch:
    """The slabs of one call: blobs, capacities and the expectation per slab (one sweep, or several interleaved)."""

    def __init__(self, sweeps, interleave=False):
        order = [(s, j) for s in sweeps for j in range(s.pairs)]
        if interleave:  # round-robin: neighbouring lanes of a wavefront hold different streams
            order.sort(key=lambda sj: (sj[1], sweeps.index(sj[0])))
        self.blobs = [s.case.blob for s, _ in order]
        self.caps = np.array([s.caps[j] for s, j in order], dtype=np.uint32)
        self.status = np.array([s.status[j] for s, j in order], dtype=np.int64)
        self.out_len = np.array([s.out_len[j] for s, j in order], dtype=np.int64)
        self.consumed = np.array([s.consumed[j] for s, j in order], dtype=np.int64)
        self.streams = [s.streams[j] for s, j in order]
        dictionaries = {s.case.dictionary for s in sweeps} - {None}
        assert len(dictionaries) <= 1
        self.dictionary = dictionaries.pop() if dictionaries else None
        self.windows = [s.case.window for s, _ in order]


# ---------------------------------------------------------------------------------------------------------------------
# one call on a patterned buffer, its comparison with the expectation, and the plan the launcher had for it
# ---------------------------------------------------------------------------------------------------------------------
def decode_call(lib, mem, batch, gap=0, with_consumed=True, sizes_only=False):
    """tamp_batch_decompress (``sizes_only``: tamp_batch_decoded_size with limit = the capacities) on slabs ``gap`` bytes apart in
    a buffer of pattern().  -> ((status, out_len, the whole buffer, out_off), consumed or None), on the host."""
    from tamp_amd.batch import pack_streams

    flat, in_off, in_len = pack_streams(batch.blobs)
    caps, n = batch.caps, len(batch.caps)
    out_off, out = slab_layout(caps, gap)
    out_len, status = np.full(n, POISON_LEN, np.uint32), np.full(n, POISON_STATUS, np.int8)
    consumed = np.full(n, POISON_CONSUMED, np.uint32) if with_consumed else None
    dict_buf = None if batch.dictionary is None else np.frombuffer(batch.dictionary, dtype=np.uint8)
    host = [flat, in_off, in_len, out, out_off, caps, out_len, status, consumed, dict_buf]
    if mem == MEM_DEVICE:
        import torch

        dev = torch.device("cuda:0")
        as_signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
        held = [None if a is None else torch.from_numpy(a.view(as_signed.get(a.dtype, a.dtype)).copy()).to(dev) for a in host]
        ptr = [None if t is None else C.c_void_p(t.data_ptr()) for t in held]
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
    else:
        held = host
        ptr = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in host]
        stream = None
    p_in, p_in_off, p_in_len, p_out, p_out_off, p_cap, p_len, p_status, p_consumed, p_dict = ptr
    dict_len = 0 if dict_buf is None else int(dict_buf.size)
    if sizes_only:
        rc = lib.tamp_batch_decoded_size(dict_len, 15, p_in, p_in_off, p_in_len, p_cap, p_len, p_status, p_consumed, n, mem, 0, stream)
    else:
        rc = lib.tamp_batch_decompress(p_dict, dict_len, 15, p_in, p_in_off, p_in_len, p_out, p_out_off, p_cap, p_len, p_status,
                                       p_consumed, n, mem, 0, stream)
    assert rc == 0, rc
    if mem == MEM_DEVICE:
        torch.cuda.synchronize()
        out, out_len, status = held[3].cpu().numpy(), held[6].cpu().numpy().view(np.uint32), held[7].cpu().numpy()
        consumed = held[8].cpu().numpy().view(np.uint32) if with_consumed else None
    return (status.astype(np.int64), out_len.astype(np.int64), out, out_off), None if consumed is None else consumed.astype(np.int64)


def check_decode(got, consumed, batch, tag, behind_len_unspecified=False):
    check_call(got, batch.caps, batch.status, batch.out_len, batch.streams, tag, behind_len_unspecified=behind_len_unspecified,
               consumed=None if consumed is None else (consumed, batch.consumed))


def planned(lib, batch):
    """tamp_amd_decompress_plan for the call just made: the batch's own facts, as the header pre-pass finds them."""
    import torch

    from tamp_amd import _lib

    q = _lib.TampAmdDecodeQuery(len(batch.caps), 15, batch.dictionary is not None, 0, 0,
                                torch.cuda.get_device_properties(0).multi_processor_count, max(batch.windows),
                                max(len(b) for b in batch.blobs), sum(1 << w for w in batch.windows) // 256, int(batch.caps.max()))
    plan = _lib.TampAmdDecodePlan()
    assert lib.tamp_amd_decompress_plan(C.byref(q), C.byref(plan)) == 0
    return plan


def assert_planned(lib, batch, facts, tag):
    plan = planned(lib, batch)
    assert plan.scan == 1 and plan.long_attempt == 0, tag
    for field, value in facts.items():
        assert getattr(plan, field) == value, (tag, "the call did not reach its build:", field, getattr(plan, field), value)
    return plan


def run(lib, oracle, monkeypatch, forced, spw, names, facts, tag, mem=MEM_DEVICE, gap=0, interleave=False):
    """Every stream of ``names`` as a sweep of its own (``interleave``: all in one call) under TAMP_AMD_DECODER = ``forced``."""
    if forced is not None:
        monkeypatch.setenv("TAMP_AMD_DECODER", forced)
    if spw is not None:
        monkeypatch.setenv("TAMP_AMD_SPLIT_SPW", str(spw))
    sweeps = [sweep_of(oracle, name) for name in names]
    batches = [Batch(sweeps, interleave=True)] if interleave else [Batch([s]) for s in sweeps]
    seen, pairs = set(), 0
    for k, batch in enumerate(batches):
        t = (tag, "all of " + ", ".join(names) if interleave else names[k], "host" if mem == MEM_HOST else "device", "gap", gap)
        assert len(batch.caps) >= MIN_STREAMS
        got, consumed = decode_call(lib, mem, batch, gap=gap)
        assert_planned(lib, batch, facts, t)
        check_decode(got, consumed, batch, t, behind_len_unspecified=(mem == MEM_HOST and gap == 0))
        seen |= set(int(s) for s in batch.status)
        pairs += len(batch.caps)
    print("%s: %d (stream, capacity) pairs in %d calls" % (tag, pairs, len(batches)))
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# 1. the sweeps, one case per build
# ---------------------------------------------------------------------------------------------------------------------
LONG_W10 = ("long text w10 ext", "long text w10 v1")
# id: (TAMP_AMD_DECODER, TAMP_AMD_SPLIT_SPW, streams, what tamp_amd_decompress_plan must say, the statuses of the sweeps)
CASES = {
    "wave, 4 waves per workgroup": ("wave", None, LONG_W10 + ("tokens", "oob", "cut", "reset"), dict(decoder=WAVE, wave_waves=4), {1, 2, -4}),
    "wave, 1 wave per workgroup": ("wave", None, ("long text w15",), dict(decoder=WAVE, wave_waves=1, max_window_bits=15), {1, 2}),
    "LDS lanes, lean": ("lane", None, ("short text w10 ext", "short text w10 v1", "short text w9 l5", "short_tokens"),
                        dict(decoder=LANE_LDS, bulk=0), {1, 2}),
    "LDS lanes, bulk": ("lane", None, LONG_W10 + ("tokens", "reset", "oob", "custom"), dict(decoder=LANE_LDS, bulk=1), {1, 2, -4}),
    "slab lanes, lean": ("global", None, ("short text w10 ext", "short text w9 l5", "short text w15"),
                         dict(decoder=LANE_GLOBAL, bulk=0, global_bulk=0), {1, 2}),
    "slab lanes, bulk": ("global", None, ("long text w15", "tokens", "reset"), dict(decoder=LANE_GLOBAL, bulk=1, global_bulk=1), {1, 2}),
    "split, one-wavefront RESOLVE": ("split", None, ("short text w10 ext", "short text w10 v1", "short text w9 l5", "short text w15",
                                                     "short_tokens"), dict(decoder=SPLIT, split_wave_resolve=1), {1, 2}),
    "split, workgroup RESOLVE": ("split", None, LONG_W10 + ("long text w15", "tokens", "oob", "cut", "custom"),
                                 dict(decoder=SPLIT, split_wave_resolve=0, bulk=1), {1, 2, -4}),
    "split, 16 streams per parse wave": ("split", 16, LONG_W10, dict(decoder=SPLIT, split_spw=16), {1, 2}),
    "split, 32 streams per parse wave": ("split", 32, LONG_W10, dict(decoder=SPLIT, split_spw=32), {1, 2}),
    "split, 64 streams per parse wave": ("split", 64, LONG_W10, dict(decoder=SPLIT, split_spw=64), {1, 2}),
    "split, handed back": ("split", None, ("lag", "reset"), dict(decoder=SPLIT), {1, 2}),
    # nothing forced: 256 and more streams of 512 and more compressed bytes with at most 16 KiB of room are the split decoder's
    # (tests/test_gpu_decode_plan.py "256 streams"), above 2 KiB of room with a workgroup per stream in RESOLVE
    "unforced": (None, None, ("long text w10 ext", "tokens"), dict(decoder=SPLIT, bulk=1, split_wave_resolve=0, max_window_bits=10), {1, 2}),
}
HOST_CASES = ("wave, 4 waves per workgroup", "LDS lanes, bulk", "split, workgroup RESOLVE")


@pytest.mark.parametrize("case", list(CASES))
def test_sweep_on_every_decoder_build(lib, oracle, monkeypatch, case):
    forced, spw, names, facts, statuses = CASES[case]
    assert run(lib, oracle, monkeypatch, forced, spw, names, facts, case) == statuses


def test_lag_and_reset_sweeps_straddle_the_hand_back(oracle):
    """The split decoder flags a stream at its 49th lagging token and at a dictionary reset, as far as ``cap`` lets the parse run:
    the sweeps hold capacities on both sides of each (from the writer's bookkeeping, tests/tight_decode_input.py)."""
    lag, reset = sweep_of(oracle, "lag"), sweep_of(oracle, "reset")
    at = tdi.lag_starts(lag.case)[tdi.LAG_LIMIT]
    assert lag.N == tdi.n_out(lag.case) and int(lag.caps[0]) == 0 and 64 < at < lag.N - 64 and lag.N + 2 in lag.caps
    assert (lag.caps < at).sum() > 64 and (lag.caps > at + 9).sum() > 64
    first = tdi.reset_starts(reset.case)[0]
    assert reset.N == tdi.n_out(reset.case) and (reset.caps < first).sum() > 64 and (reset.caps > first).sum() > 64


@pytest.mark.parametrize("forced,facts", [("lane", dict(decoder=LANE_LDS, bulk=1)), ("global", dict(decoder=LANE_GLOBAL, global_bulk=1)),
                                          ("split", dict(decoder=SPLIT, split_wave_resolve=0))], ids=["lane", "global", "split"])
def test_interleaved_sweeps_of_three_streams(lib, oracle, monkeypatch, forced, facts):
    """One call whose slabs alternate between the sweeps of three streams: neighbouring lanes of a wavefront hold different
    streams, at different capacities, and leave their fast paths at different steps."""
    seen = run(lib, oracle, monkeypatch, forced, None, ("long text w10 ext", "tokens", "oob"), facts, "interleaved, " + forced,
               interleave=True)
    assert seen == {1, 2, -4}


@pytest.mark.parametrize("gap", [0, 5], ids=["tiled", "gapped"])
@pytest.mark.parametrize("case", HOST_CASES)
def test_sweep_from_host_memory(lib, oracle, monkeypatch, case, gap):
    """The host-memory call: tiled slabs come back in one transfer (slab bytes behind out_len are unspecified, everything else is
    checked), slabs 5 bytes apart get exactly their produced bytes and nothing else in the caller's buffer."""
    forced, spw, names, facts, statuses = CASES[case]
    assert run(lib, oracle, monkeypatch, forced, spw, names, facts, case + ", host", mem=MEM_HOST, gap=gap) == statuses


def test_sweep_without_a_consumed_table(lib, oracle):
    """in_consumed = NULL in a device call: statuses, lengths and the whole buffer as ever."""
    batch = Batch([sweep_of(oracle, "tokens")])
    got, consumed = decode_call(lib, MEM_DEVICE, batch, with_consumed=False)
    assert consumed is None
    check_decode(got, None, batch, "no consumed table")


@pytest.mark.parametrize("name", ["long text w10 ext", "tokens"])
@pytest.mark.parametrize("mem", [MEM_DEVICE, MEM_HOST], ids=["device", "host"])
def test_size_query_at_every_limit(lib, oracle, name, mem):
    """tamp_batch_decoded_size with limit = the capacities of a sweep: the size, status and consumed count of the decode, and not
    a byte of output."""
    batch = Batch([sweep_of(oracle, name)])
    (status, size, out, _), consumed = decode_call(lib, mem, batch, sizes_only=True)
    bad = np.flatnonzero((status != batch.status) | (size != batch.out_len) | (consumed != batch.consumed))
    assert bad.size == 0, (name, "limit", int(batch.caps[bad[0]]), int(status[bad[0]]), int(size[bad[0]]), int(consumed[bad[0]]))
    assert np.array_equal(out, slab_layout(batch.caps)[1])
