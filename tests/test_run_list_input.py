"""CPU tier: the inputs of tests/test_gpu_run_list.py aim where they say they aim (tests/run_list_input.py).

The GPU tier compares bytes with the reference and nothing else, so it only tests the second pass of the run-aware builds
(tamp_compress_kernel.hpp, `if (nruns)`) where the reference's own choice depends on it.  This tier proves that from the
reference side alone:

  * ``second_pass_key`` -- the three branches and their shortcuts, restated -- finds what a byte-by-byte scan of every
    interior position finds, on the random buffers of test_run_candidates_model.py and at every family A query;
  * the token the reference writes at each family A query is mapped back to an input position; the streams whose token
    points INTO the run's interior are counted per (branch, flag), the counts the issue asks for are asserted, and the
    restatement names the same position, cell and length for every one of them;
  * three deliberately wrong copies of the restatement (no cz candidate below cs; rq + 1 read as rq; the limit W - index
    ignored) each disagree with the scan on family A: the inputs can tell;
  * family B holds more long runs per epoch than the run list has slots, family C fewer, by the raw bytes;
  * the oracle and the reference C agree on all three families.

What it cannot show: which runs the device listed.  That more than kRunCap runs are found per epoch is a property of the
inputs and of the listing as the kernel's code reads; that the output is the same whichever are listed is the GPU tier's.
"""
import collections
import ctypes
import functools
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import long_stream_writer as lsw  # noqa: E402
import run_list_input as rli  # noqa: E402
from test_run_candidates_model import run_heavy_buffers  # noqa: E402

WINDOWS_A = (8, 10)
WINDOWS_BC = (8, 10, 12, 14)
BC_SIZES = rli.BC_SIZES


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


def planned_block(lib, window, max_in_len):
    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert lib.tamp_amd_compress_plan(window, max_in_len, 0, *[ctypes.byref(x) for x in v]) == 0
    return v[0].value


def test_the_constants_are_the_headers():
    with open(os.path.join(ROOT, "tamp_amd", "csrc", "tamp_compress_kernel.hpp")) as f:
        src = f.read()
    assert int(re.search(r"constexpr uint32_t kRunCap = (\d+);", src).group(1)) == rli.K_RUN_CAP
    assert int(re.search(r"constexpr uint32_t kLongRun = (\d+);", src).group(1)) == rli.K_LONG_RUN


def test_restatement_on_random_buffers():
    rng = random.Random(5)
    checked = won_in = 0
    for it, W, blk, buf, wp_e, runs in run_heavy_buffers(rng):
        for q in range(blk):
            cap_len = rng.choice([16, 16, 16, rng.randrange(2, 17)])
            got, won = rli.second_pass_key(buf, q, W, wp_e, cap_len, runs)
            want, at = rli.exhaustive_key(buf, q, W, wp_e, cap_len, runs)
            assert got == want and (won is None or won.c == at), (it, W, q, wp_e, cap_len, got, want, won, at)
            checked += buf[W + q] == buf[W + q + 1]
            won_in += won is not None
    assert checked > 5000 and won_in > 2000


# ---------------------------------------------------------------------------------------------------------------------
# family A
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_a_views(window, blk, dictionary):
    return [rli.epoch_view(s.data, s.pq, 1 << window, blk, dictionary) for s in rli.family_a(window)]


def compressed(checker, streams, window, extended=False):
    from tamp_amd.batch import pack_streams

    flat, off, ln = pack_streams(streams)
    r = checker.compress_batch(flat, off, ln, window=window, literal=8, extended=extended, threads=8)
    assert (np.asarray(r.status) == 0).all()
    return [r.stream(i) for i in range(len(streams))]


@pytest.mark.parametrize("window", WINDOWS_A)
def test_family_a_restatement_against_an_exhaustive_scan(lib, oracle, window):
    W = 1 << window
    fam = rli.family_a(window)
    views = family_a_views(window, planned_block(lib, window, 2048), oracle.initialize_dictionary(W))
    interior = 0
    for s, (buf, q, wp_e, cap_len, runs, base) in zip(fam, views):
        assert (s.a - base, s.b - base) in runs or s.a - base < 0, (s.aim, s.a, s.b)
        got, won = rli.second_pass_key(buf, q, W, wp_e, cap_len, runs)
        want, at = rli.exhaustive_key(buf, q, W, wp_e, cap_len, runs)
        assert got == want and (won is None or won.c == at), (s.aim, s.a, s.b, s.pq, s.rq, s.agree, got, want, won, at)
        interior += won is not None
    assert interior > len(fam) // 2


@pytest.mark.parametrize("weaken", ["no_cz", "rq_plus_1", "no_lim"])
@pytest.mark.parametrize("window", WINDOWS_A)
def test_family_a_catches_a_weakened_restatement(lib, oracle, window, weaken):
    """The inputs, not the kernel: a second pass without the cz candidate below cs, one that reads rq + 1 as rq, one that
    ignores the limit W - index -- each must differ from the byte-by-byte scan on family A, on at least 100 streams."""
    W = 1 << window
    views = family_a_views(window, planned_block(lib, window, 2048), oracle.initialize_dictionary(W))
    caught = sum(rli.second_pass_key(buf, q, W, wp_e, cap_len, runs, weaken=weaken)[0] != rli.exhaustive_key(buf, q, W, wp_e, cap_len, runs)[0]
                 for buf, q, wp_e, cap_len, runs, _ in views)
    print("weakened restatement %s, window %d: differs from the scan on %d of %d streams" % (weaken, window, caught, len(views)))
    assert caught >= 100, (weaken, window, caught)


def cell_table(lib, oracle, window):
    """-> (Counter over (branch, flag) with flag in "*", "idx0", "wrap", "lo", "lim"; streams; interior streams), asserting on the
    way that the restatement names the position, cell and length of every token that points into the run's interior."""
    W = 1 << window
    fam = rli.family_a(window)
    views = family_a_views(window, planned_block(lib, window, 2048), oracle.initialize_dictionary(W))
    blobs = compressed(oracle, [s.data for s in fam], window)
    table, how, hits = collections.Counter(), collections.Counter(), 0
    for s, blob, (buf, q, wp_e, cap_len, runs, base) in zip(fam, blobs, views):
        bit = rli.v1_token_at(blob, s.pq)
        assert bit is not None, ("no token starts at the query", s.aim, s.pq)
        tk = lsw.read_tokens(blob, start=bit, stop=bit + 1)[0][0]
        cell = rli.token_cell(s, W, tk.off, tk.produced) if tk.kind == "M" else None
        key, won = rli.second_pass_key(buf, q, W, wp_e, cap_len, runs)
        if cell is None:
            continue
        hits += 1
        p, branch, flags = cell
        assert won is not None and (won.c + base, won.branch, won.flags, key >> 16) == (p, branch, flags, tk.produced), \
            (s.aim, s.a, s.b, s.pq, s.rq, s.agree, cell, tk, won, key >> 16)
        table[(branch, "*")] += 1
        for f in flags:
            table[(branch, f)] += 1
        how[(branch, won.how)] += 1
    return table, how, len(fam), hits


@pytest.mark.parametrize("window", WINDOWS_A)
def test_family_a_cell_table_from_the_references_tokens(lib, oracle, window):
    table, how, n, hits = cell_table(lib, oracle, window)
    print("family A, window %d: %d streams, %d decided by a run-interior candidate" % (window, n, hits))
    for branch in (rli.BELOW, rli.CS, rli.ABOVE):
        print("  %-5s %s" % (branch, "  ".join("%s %d" % (f, table[(branch, f)]) for f in ("*", "idx0", "wrap", "lo", "lim"))),
              "| " + "  ".join("%s %d" % (h, c) for (b, h), c in sorted(how.items()) if b == branch))
    for branch in (rli.BELOW, rli.CS, rli.ABOVE):
        assert table[(branch, "*")] >= 200, (branch, table)
        assert table[(branch, "idx0")] >= 8 and table[(branch, "wrap")] >= 8, (branch, table)
    assert sum(table[(b, "lo")] for b in (rli.BELOW, rli.CS, rli.ABOVE)) >= 8
    assert sum(table[(b, "lim")] for b in (rli.BELOW, rli.CS, rli.ABOVE)) >= 8
    assert {h for _, h in how} >= {"rq", "rq+1", "cmp", "rc", "wrapped"}  # every shortcut of the second pass decided some token


def test_the_lean_token_walker_is_the_projects_reader(oracle):
    for window, s in [(8, s) for s in rli.family_a(8)[::997]] + [(10, s) for s in rli.family_a(10)[::1499]]:
        blob = compressed(oracle, [s.data], window)[0]
        pos = 0
        for tk in lsw.read_tokens(blob)[0]:
            if tk.kind != "F":
                assert rli.v1_token_at(blob, pos) == tk.bit, (window, pos)
                if tk.produced > 1:
                    assert rli.v1_token_at(blob, pos + 1) is None
            pos += tk.produced
        assert pos == len(s.data)


# ---------------------------------------------------------------------------------------------------------------------
# families B and C
# ---------------------------------------------------------------------------------------------------------------------
def interior_matches(oracle, data, window):
    """Match tokens of the v1 stream of ``data`` whose source lies in the interior a+1 .. b-4 of a long run -> (count, matches)."""
    W = 1 << window
    starts, ends = rli.long_runs(data)
    pos = inside = matches = 0
    for tk in lsw.read_tokens(compressed(oracle, [data], window)[0])[0]:
        if tk.kind == "M":
            matches += 1
            p = pos - ((pos - tk.off) % W or W)
            j = int(np.searchsorted(starts, p, side="right")) - 1
            inside += p >= 0 and j >= 0 and starts[j] + 1 <= p <= ends[j] - 4
        pos += tk.produced
    assert pos == len(data)
    return inside, matches


@pytest.mark.parametrize("same_byte", [True, False])
@pytest.mark.parametrize("window", WINDOWS_BC)
def test_family_b_and_c_predicates(lib, oracle, window, same_byte):
    """Window 2^8: an epoch's span is 256 + 1,024 + 16 = 1,296 bytes, which holds 144 runs of 8 bytes at the very most; the dense
    variant (runs of 8 or 9 bytes, one separator) is asked for MORE than kRunCap there, every other window for 1.25 x kRunCap."""
    W = 1 << window
    for n, seed in BC_SIZES:
        blk = planned_block(lib, window, n)
        b = rli.family_b(n, seed, same_byte, dense=window == 8)
        counts = rli.overflow_predicate_v1(b, W, blk, at_least=rli.K_RUN_CAP + 1 if window == 8 else rli.K_RUN_CAP * 5 // 4)
        if window >= 11:
            rli.overflow_predicate_window(b, W)
        inside, matches = interior_matches(oracle, b, window)
        assert inside >= 10, (window, n, inside, matches)
        c = rli.family_c(window, n, seed, same_byte)
        listed = rli.all_listed_predicate(c, W)
        assert len(rli.long_runs(c)[0]) >= 16
        print("window %2d %s %5d B: family B long runs per epoch (block %d) %d..%d, %d of %d v1 matches point into a run's interior; "
              "family C at most %d per largest epoch buffer" % (window, "one byte  " if same_byte else "many bytes", n, blk, min(counts),
                                                                  max(counts), inside, matches, max(listed)))


def test_the_batches_of_the_gpu_tier():
    """tests/test_gpu_run_list.py's batches are these streams: four copies of every family B stream, and the block-mode field holds
    at least 1.25 x kRunCap long runs in the span of every block of 1,024 positions, at both of its windows."""
    for window in WINDOWS_BC:
        streams, names = rli.field_batch(window)
        for n, seed in BC_SIZES:
            for same_byte in (True, False):
                b = rli.family_b(n, seed, same_byte, dense=window == 8)
                assert sorted(nm for s, nm in zip(streams, names) if s == b) == [("B", n, same_byte, k) for k in range(rli.COPIES)]
                assert rli.family_c(window, n, seed, same_byte) in streams
        where = [i for i, nm in enumerate(names) if nm[:3] == ("B", 4096, True)]
        assert max(where) - min(where) >= 10  # (scattered over the batch)
    for window in (10, 12):
        counts = rli.overflow_predicate_v1(rli.block_mode_field(), 1 << window, 1024)
        print("block-mode field, window %d: long runs per block span %d..%d" % (window, min(counts), max(counts)))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle and the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", [False, True])
def test_oracle_and_reference_agree_on_the_three_families(oracle, ref, extended):
    for window in WINDOWS_A:
        streams = [s.data for s in rli.family_a(window)]
        assert compressed(oracle, streams, window, extended) == compressed(ref, streams, window, extended), ("A", window)
    for window in WINDOWS_BC:
        streams = []
        for n, seed in BC_SIZES:
            for same_byte in (True, False):
                streams += [rli.family_b(n, seed, same_byte, dense=window == 8), rli.family_c(window, n, seed, same_byte)]
        assert compressed(oracle, streams, window, extended) == compressed(ref, streams, window, extended), ("B, C", window)
