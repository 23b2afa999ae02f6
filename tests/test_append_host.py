"""CPU tier: appending to reset-segmented streams (tamp_batch_append, ``append_batch``) as far as no device is needed -- the symbol
and its binding, the Python names, the keyword refusals of ``append_batch``, what the C call refuses before it looks for a device
(a new_reset_cap below the bound included), the unit, cut and splice arithmetic of tamp_append.hpp compiled for the HOST into a
stand-alone program (with the address and undefined-behaviour sanitizers when the compiler has their runtimes; nothing loaded into
python is sanitised) against a restatement in Python, and the slab bound of ``out_cap=None`` against the oracle's compressor."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARGUMENTS = "tamp_batch_append", 23
BAD_ARGUMENT = -21


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_symbol_and_binding(lib):
    from tamp_amd import _lib

    header = open(os.path.join(ROOT, "include", "tamp_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\);" % NAME, code)
    assert m and len(m[1].split(",")) == ARGUMENTS
    assert NAME in _lib.SYMBOLS and hasattr(C.CDLL(_lib.LIB_PATH), NAME)
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == ARGUMENTS and fn.restype is C.c_int
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T %s$" % NAME, out, flags=re.M)


def test_python_names():
    import tamp
    import tamp_amd

    for pkg in (tamp_amd, tamp):
        assert "append_batch" in pkg.__all__ and pkg.append_batch is tamp_amd.append_batch


def test_keyword_refusals_come_before_the_library(monkeypatch):
    """Every refusal is a ValueError raised before the native library is looked for."""
    import tamp_amd
    from tamp_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded before the keywords were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    data = [bytes([0x59, 0, 1, 2]), bytes([0x59, 0, 3])]
    flat, in_off, in_len = tamp_amd.pack_streams(data)
    idx = tamp_amd.ResetIndex(np.zeros(3, np.uint64), np.zeros(0, np.uint32), 16)
    good = dict(reset_index=idx, source=[b"a", b"b"])
    flat_source = dict(source=np.frombuffer(b"ab", dtype=np.uint8), source_off=[0, 1], length=[1, 1])

    def refused(match, **change):
        for args in ((data,), (flat, in_off, in_len)):
            with pytest.raises(ValueError, match=match):
                tamp_amd.append_batch(*args, **{**good, **change})

    refused("a ResetIndex expected", reset_index=(idx.first, idx.off))
    refused("a ResetIndex expected", reset_index=None)
    for entries in (0, 2, 4):
        refused("one entry per stream and one more", reset_index=tamp_amd.ResetIndex(np.zeros(entries, np.uint64), idx.off, 16))
    refused("not given and not in the index", reset_index=tamp_amd.ResetIndex(idx.first, idx.off))  # a missing interval
    for bad in (0, -1, 1 << 32, 1.5, "16", True):
        refused("a positive integer that fits 32 bits", reset_interval=bad)
        refused("a positive integer that fits 32 bits", reset_index=tamp_amd.ResetIndex(idx.first, idx.off, bad))
    refused("one per stream, or one per entry of stream_index", source=[b"a"])
    refused("one per stream, or one per entry of stream_index", source=[b"a", b"b", b"c"])
    refused("one per stream, or one per entry of stream_index", source=[b"a", b"b"], stream_index=[0])
    refused("one per stream, or one per entry of stream_index", **{**flat_source, "length": [1]})
    refused("one per stream, or one per entry of stream_index", **{**flat_source, "source_off": [0, 1, 2]})
    refused("a sequence of bytes-likes", source=b"ab")
    refused("derived from a sequence", source_off=[0, 1])
    refused("derived from a sequence", length=[1, 1])
    refused("needs source_off and length", source=flat_source["source"])
    refused("needs source_off and length", source=flat_source["source"], source_off=[0, 1])
    refused("length: does not fit 32 bits", **{**flat_source, "length": [1, 1 << 32]})
    refused("length: negative", **{**flat_source, "length": [1, -1]})
    refused("source_off: negative", **{**flat_source, "source_off": [0, -1]})
    refused("stream_index: out of range", source=[b"a"], stream_index=[2])
    refused("stream_index: negative", source=[b"a"], stream_index=[-1])
    refused("named twice", source=[b"a", b"b"], stream_index=[1, 1])
    refused("window must be in 8..15", window=16)
    refused("literal must be in 5..8", literal=4)
    refused("out_cap: one entry per stream", out_cap=[8])
    refused("out_cap: does not fit 32 bits", out_cap=1 << 32)
    refused("does not fit 32 bits: pass out_cap", source=[b"a", b"b"], reset_interval=0xFFFFFFFF)  # (the default room of one full segment)
    # what is fine gets as far as the library: nothing appended, None for nothing, named streams in any order, a flat source
    for change in (dict(), dict(source=[b"", None]), dict(source=[b"xyz"], stream_index=[1]), dict(source=[b"x", b"y"], stream_index=[1, 0]),
                   dict(source=[], stream_index=[]), flat_source, dict(reset_index=tamp_amd.ResetIndex(idx.first, idx.off, 0), reset_interval=16)):
        with pytest.raises(AssertionError, match="the library was loaded"):
            tamp_amd.append_batch(data, **{**good, **change})


def test_front_end_tables():
    """Named streams become one row per stream; ``out_cap=None`` is the stream's length and ceil(L / N) + 1 full closed segments."""
    import tamp_amd
    from tamp_amd import _lib

    seen = {}

    class Stop(Exception):
        pass

    class Lib:
        def tamp_amd_set_timing(self, on):
            pass

        def tamp_batch_append(self, *a):
            addr = lambda p: C.cast(p, C.c_void_p).value  # noqa: E731
            n = a[19]
            seen["src_off"] = np.ctypeslib.as_array(C.cast(addr(a[9]), C.POINTER(C.c_uint64)), (n,)).tolist()
            seen["src_len"] = np.ctypeslib.as_array(C.cast(addr(a[10]), C.POINTER(C.c_uint32)), (n,)).tolist()
            seen["src"] = bytes(np.ctypeslib.as_array(C.cast(addr(a[8]), C.POINTER(C.c_uint8)), (6,)))
            seen["conf"] = (a[0]._obj.window, a[0]._obj.literal, a[0]._obj.extended, a[0]._obj.dictionary_reset, a[0]._obj.lazy_matching)
            seen["cap"] = np.ctypeslib.as_array(C.cast(addr(a[13]), C.POINTER(C.c_uint32)), (n,)).tolist()
            seen["new_cap"], seen["interval"], seen["mem"] = a[18], a[7], a[20]
            raise Stop()

    real = _lib.load
    _lib.load = lambda: Lib()
    try:
        idx = tamp_amd.ResetIndex(np.array([0, 2, 2, 2], np.uint64), np.array([9, 20], np.uint32), 16)
        with pytest.raises(Stop):
            tamp_amd.append_batch([bytes([0x33, 0]) + bytes(30), bytes([0x33, 0, 9]), bytes([0x33, 0])], reset_index=idx, stream_index=[2, 0],
                                  source=[b"z" * 33, b"abcde"], lazy_matching=True)
    finally:
        _lib.load = real
    assert seen["src_len"] == [5, 0, 33] and seen["src_off"] == [33, 0, 0] and seen["src"] == b"zzzzzz"
    assert seen["conf"] == (9, 7, 1, 1, 1)  # 0x33: window 9, literal 7, extended, the reset bit
    closed = 2 + (16 * 8 + 16) // 8
    assert seen["cap"] == [32 + 2 * closed, 3 + closed, 2 + 4 * closed]
    assert seen["new_cap"] == 2 + 1 + 0 + 3 and seen["interval"] == 16 and seen["mem"] == _lib.MEM_HOST


TABLES = ("in_off", "in_len", "reset_first", "src_off", "src_len", "out_off", "out_cap", "out_len", "status", "new_reset_first")


def _arrays(src_len=1, entries=0):
    a = dict(data=np.array([0x59, 0, 0, 0], dtype=np.uint8), in_off=np.zeros(1, np.uint64), in_len=np.full(1, 4, np.uint32),
             reset_first=np.array([0, entries], np.uint64), reset_off=np.full(4, 2, np.uint32), src=np.zeros(64, np.uint8),
             src_off=np.zeros(1, np.uint64), src_len=np.full(1, src_len, np.uint32), out=np.full(256, 0xA5, np.uint8),
             out_off=np.zeros(1, np.uint64), out_cap=np.full(1, 256, np.uint32), out_len=np.full(1, 0xDEAD, np.uint32),
             status=np.full(1, 99, np.int8), new_reset_first=np.full(2, 0xDEAD, np.uint64), new_reset_off=np.full(8, 0xDEAD, np.uint32))
    return a, {k: v.ctypes.data_as(C.c_void_p) for k, v in a.items()}


def _call(lib, *, missing=(), n=1, interval=16, mem=None, device=0, conf=None, no_conf=False, new_cap=8, src_len=1, entries=0):
    from tamp_amd import _lib

    held, p = _arrays(src_len, entries)
    for k in missing:
        p[k] = None
    conf = conf or _lib.TampAmdConf(10, 8, 0, 1, 1, 0, 0)
    rc = lib.tamp_batch_append(None if no_conf else C.byref(conf), 15, p["data"], p["in_off"], p["in_len"], p["reset_first"], p["reset_off"],
                               interval, p["src"], p["src_off"], p["src_len"], p["out"], p["out_off"], p["out_cap"], p["out_len"], p["status"],
                               p["new_reset_first"], p["new_reset_off"], new_cap, n, _lib.MEM_HOST if mem is None else mem, device, None)
    return rc, held


def test_call_level_refusals(lib):
    """Before a device is looked for: TAMP_AMD_BAD_ARGUMENT on a machine with and without one, for both memory kinds."""
    from tamp_amd import _lib

    call = lambda **kw: _call(lib, **kw)[0]  # noqa: E731
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        for table in TABLES + ("data", "src", "out"):
            assert call(missing=(table,), mem=mem) == BAD_ARGUMENT, table
        assert call(missing=("new_reset_off",), mem=mem) == BAD_ARGUMENT  # (a capacity and no table)
        assert call(no_conf=True, mem=mem) == BAD_ARGUMENT
        assert call(interval=0, mem=mem) == BAD_ARGUMENT
        assert call(interval=0xFFFFFFFF, mem=mem) == BAD_ARGUMENT  # (a worst-case segment that does not fit 32 bits)
        assert call(device=_lib.ALL_DEVICES, mem=mem) == BAD_ARGUMENT
        assert call(n=1 << 32, mem=mem) == BAD_ARGUMENT
        # conf: the reset bit is required, a custom dictionary is not taken, the fields must be in range
        for conf in (_lib.TampAmdConf(10, 8, 0, 1, 0, 0, 0), _lib.TampAmdConf(10, 8, 1, 1, 1, 0, 0), _lib.TampAmdConf(7, 8, 0, 1, 1, 0, 0),
                     _lib.TampAmdConf(10, 9, 0, 1, 1, 0, 0), _lib.TampAmdConf(10, 8, 0, 1, 1, 2, 0)):
            assert call(conf=conf, mem=mem) == BAD_ARGUMENT
        assert call(n=0, missing=("data", "src", "out", "reset_off", "new_reset_off"), new_cap=0, mem=mem) == 0  # nothing is done
    for mem in (2, -1, 7):
        assert call(mem=mem) == BAD_ARGUMENT
    # host tables: a new_reset_cap below reset_first[n] + sum ceil(src_len / N) is refused with nothing written
    for src_len, entries, need in ((1, 0, 1), (16, 0, 1), (17, 0, 2), (33, 2, 5), (0, 3, 3)):
        rc, held = _call(lib, src_len=src_len, entries=entries, new_cap=need - 1, missing=("new_reset_off",) if need == 1 else ())
        assert rc == BAD_ARGUMENT, (src_len, entries)
        assert (held["out"] == 0xA5).all() and int(held["out_len"][0]) == 0xDEAD and int(held["status"][0]) == 99
        assert (held["new_reset_first"] == 0xDEAD).all() and (held["new_reset_off"] == 0xDEAD).all()


PROGRAM = r"""
#include "tamp_append.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace tamp_amd;
typedef unsigned long long ull;

// Reads cases, one per line, and answers each with one line; the caller holds the restatement.
//   units m L N               -> U bound, then per unit j < min(U, 6) and for the last one: len old_len src_at, and whether closed row j holds a unit
//   splice start cap U len..  -> total fits, then the U - 1 entries (len: the slab length of unit j, lead included)
//   bound entries N n len..   -> the entries new_reset_off must hold
//   hold n first..            -> per stream: its rows of reset_first hold (n + 1 values)
int main() {
    char what[16];
    long cases = 0;
    while (scanf("%15s", what) == 1) {
        cases++;
        if (!strcmp(what, "units")) {
            ull m, L, N;
            if (scanf("%llu %llu %llu", &m, &L, &N) != 3) return 2;
            const uint64_t U = append_units((uint32_t)m, (uint32_t)L, (uint32_t)N);
            printf("%llu %llu", (ull)U, (ull)append_entry_bound((uint32_t)L, (uint32_t)N));
            for (uint64_t x = 0; x < 7; x++) {
                const uint64_t j = x < 6 ? x : U - 1;
                if (j >= U) continue;
                const AppendCut c = append_cut((uint32_t)m, (uint32_t)L, (uint32_t)N, j);
                printf(" %u %u %llu %d", c.len, c.old_len, (ull)c.src_at, append_closed_row_used(j, U) ? 1 : 0);
            }
            const AppendCut past = append_cut((uint32_t)m, (uint32_t)L, (uint32_t)N, U);
            printf(" %u\n", past.len);
        } else if (!strcmp(what, "splice")) {
            ull start, cap, U;
            if (scanf("%llu %llu %llu", &start, &cap, &U) != 3) return 2;
            std::vector<uint32_t> len(U);
            for (ull j = 0; j < U; j++) {
                ull v;
                if (scanf("%llu", &v) != 1) return 2;
                len[j] = (uint32_t)v;
            }
            std::vector<uint64_t> entry(U);
            const uint64_t total = append_splice((uint32_t)start, len.data(), U, entry.data());
            printf("%llu %d", (ull)total, append_fits(total, (uint32_t)cap) ? 1 : 0);
            for (ull j = 0; j + 1 < U; j++) printf(" %llu", (ull)entry[j]);
            printf("\n");
        } else if (!strcmp(what, "bound")) {
            ull entries, N, n;
            if (scanf("%llu %llu %llu", &entries, &N, &n) != 3) return 2;
            std::vector<uint32_t> len(n);
            for (ull i = 0; i < n; i++) {
                ull v;
                if (scanf("%llu", &v) != 1) return 2;
                len[i] = (uint32_t)v;
            }
            printf("%llu\n", (ull)append_reset_bound(entries, len.data(), n, (uint32_t)N));
        } else if (!strcmp(what, "hold")) {
            ull n;
            if (scanf("%llu", &n) != 1) return 2;
            std::vector<uint64_t> first(n + 1);
            for (ull i = 0; i <= n; i++) {
                ull v;
                if (scanf("%llu", &v) != 1) return 2;
                first[i] = v;
            }
            std::vector<uint8_t> hold(n + 1);
            append_rows_hold(first.data(), n, hold.data());
            for (ull i = 0; i < n; i++) printf("%d ", hold[i]);
            printf("\n");
        } else return 3;
    }
    static_assert(write_fail_key(0, kAppendRankBudget, -21) < write_fail_key(0, kAppendRankConf, -3), "the first rule first");
    static_assert(write_fail_key(0, kAppendRankEntries, -22) < write_fail_key(0, kAppendRankOob, -4), "entries in front of the open segment");
    static_assert(write_fail_key(0, kAppendRankExcess, -2) < write_fail_key(0, kAppendRankCompress, 1), "the source in front of the units");
    static_assert(write_fail_key(0xFFFFFFFFull, kAppendRankCompress, -1) < kWriteNoFail, "every key lies below 'none'");
    static_assert(append_units(0, 0, 5) == 1 && append_units(5, 0, 5) == 1 && append_units(5, 1, 5) == 2, "units");
    fprintf(stderr, "%ld cases\n", cases);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("append")
    (d / "append.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), str(d / "append.cpp"), "-o", str(d / "append")]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizers' runtimes)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "append"), sanitized


def units_py(m, L, N):
    """(U, bound, cut): cut(j) = (len, old_len, src_at, closed row j holds a unit) of unit j, in Python integers."""
    total = m + L
    U = max(1, -(-total // N))

    def cut(j):
        lo, hi = j * N, min((j + 1) * N, total)
        return (hi - lo, min(m, hi) if j == 0 else 0, lo - m if j else 0, int(j + 1 < U))

    return U, -(-L // N), cut


def walk_py(m, L, N):
    """The same by a plain walk over the bytes: old bytes are ('o', k), appended ones ('s', k); cut at every N."""
    both = [("o", k) for k in range(m)] + [("s", k) for k in range(L)]
    units = [both[at : at + N] for at in range(0, len(both), N)] or [[]]
    out = []
    for j, u in enumerate(units):
        old = sum(1 for b in u if b[0] == "o")
        firsts = [b[1] for b in u if b[0] == "s"]
        assert old == 0 or j == 0
        out.append((len(u), old, firsts[0] if firsts and j else 0, int(j + 1 < len(units))))
    return out


def test_append_arithmetic(program):
    """Unit counts and cuts for every (m, L, N) with N in 1..9, m <= N, L <= 4 N + 1, and around 2^32 - 1 for L and N; the splice
    (new entries, new length, overflow past 32 bits); the bound of new_reset_off: against the restatement above."""
    exe, sanitized = program
    rng = random.Random(20241020)
    lines, wants = [], []
    top = (1 << 32) - 1
    cases = [(m, L, N) for N in range(1, 10) for m in range(N + 1) for L in range(4 * N + 2)]
    for N in (1, 2, 7, 1 << 16, top - 1, top):
        for L in (top, top - 1, top - 2, N, max(N - 1, 0), min(N + 1, top), 0, 1):
            for m in {0, 1, N // 2, max(N - 1, 0), N}:
                cases.append((m, L, N))
    for m, L, N in cases:
        U, bound, cut = units_py(m, L, N)
        assert U - 1 <= bound <= U  # what sizes the rows: the closed rows are the bound, at most one stays unused
        if L <= 4 * N + 1 and N < 10:
            walked = walk_py(m, L, N)
            assert len(walked) == U
            for j, w in enumerate(walked):  # (a unit without source bytes has no first one: src_at is not looked at)
                assert w == cut(j) or (w[0] == w[1] and w[:2] == cut(j)[:2] and w[3] == cut(j)[3]), (m, L, N, j)
        lines.append("units %d %d %d" % (m, L, N))
        want = [U, bound]
        for x in range(7):
            j = x if x < 6 else U - 1
            if j < U:
                want += list(cut(j))
        wants.append(want + [0])
    for _ in range(800):
        U = rng.randrange(1, 12)
        start = rng.choice((2, 2, 9, 1000, top - 40, top - 2))
        lens = [rng.randrange(2, 90) for _ in range(U)]  # slab lengths, lead included
        cap = rng.choice((top, 0, start, start + sum(lens)))
        at, entries = start, []
        for j, v in enumerate(lens):
            at += v if j + 1 < U else v - 2  # a closed unit: - lead + the next lead; the open one: - lead
            if j + 1 < U:
                entries.append(at)
        lines.append("splice %d %d %d %s" % (start, cap, U, " ".join(map(str, lens))))
        wants.append([at, int(at <= cap and at <= top)] + entries)
    for _ in range(300):
        N = rng.choice((1, 3, 16, 1 << 16, top))
        lens = [rng.choice((0, 1, N - 1, N, N + 1, 3 * N + 1, top)) % (top + 1) for _ in range(rng.randrange(0, 9))]
        entries = rng.choice((0, 5, 1 << 40))
        lines.append("bound %d %d %d %s" % (entries, N, len(lens), " ".join(map(str, lens))))
        wants.append([entries + sum(-(-v // N) for v in lens)])
    # rows of reset_first that hold: each pair in order inside the table, and behind every such pair in front; the entries of
    # the streams that hold are then disjoint and their sum is first[n] at most, which is what makes the bound a bound
    tables = [[0, 5, 3, 8], [0, 5, 3, 8, 10], [0, 0, 0], [1, 2, 3], [0, 9, 2, 4, 9], [0, 3, 3, 2, 7, 7]]
    for _ in range(400):
        n = rng.randrange(1, 9)
        t = sorted(rng.randrange(0, 12) for _ in range(n + 1)) if rng.random() < 0.3 else [rng.randrange(0, 12) for _ in range(n + 1)]
        if rng.random() < 0.7:
            t[0] = 0
        tables.append(t)
    for t in tables:
        n = len(t) - 1
        usable = [t[i] <= t[i + 1] <= t[n] and (i != 0 or t[0] == 0) for i in range(n)]
        hold = [int(usable[i] and all(t[i] >= t[j + 1] for j in range(i) if usable[j])) for i in range(n)]
        claimed = [k for i in range(n) if hold[i] for k in range(t[i], t[i + 1])]
        assert len(claimed) == len(set(claimed)) and len(claimed) <= t[n] and claimed == sorted(claimed)
        if t == sorted(t) and t[0] == 0:
            assert all(hold)  # (a running sum from 0: every stream holds)
        lines.append("hold %d %s" % (n, " ".join(map(str, t))))
        wants.append(hold)
    assert wants[-len(tables)] == [1, 0, 0]  # {0, 5, 3, 8}: stream 0 holds; stream 1 is out of order, stream 2 claims stream 0's entries
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    print(p.stderr[-500:], "(host ASan + UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    got = [[int(x) for x in row.split()] for row in p.stdout.strip().split("\n")]
    assert len(got) == len(wants) == len(lines)
    for line, g, w in zip(lines, got, wants):
        assert g == w, (line, g, w)
    assert "%d cases" % len(lines) in p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


@pytest.mark.parametrize("literal", [5, 6, 7, 8])
def test_default_room_never_undercuts(oracle, literal):
    """``out_cap=None``: the old length plus ceil(L / N) + 1 full closed segments is at least what the oracle's compressor makes of
    old + appended when both are random bytes of the literal width -- the worst case, (nearly) every byte a literal."""
    from tamp_amd.batch import _append_closed_bound

    rng = random.Random(literal)
    for interval in (1, 16, 100, 256):
        closed = _append_closed_bound(interval, literal)
        assert closed == 2 + (interval * (literal + 1) + 9 + 7) // 8
        for n in (0, 1, interval - 1, interval, interval + 1, 3 * interval, 3 * interval + 1):
            for L in (0, 1, interval - n % interval, interval, 3 * interval + 1, rng.randrange(1, 4 * interval + 2)):
                data = bytes(rng.randrange(1 << literal) for _ in range(n + L))

                def blob_of(k):
                    ops = []
                    for at in range(0, max(k, 1), interval):
                        ops += ([("reset",)] if at else []) + [("write", data[at : min(at + interval, k)])]
                    res, blob = oracle.stream_script(ops + [("flush", False)], window=8, literal=literal, dictionary_reset=True)
                    assert res == 0
                    return blob

                old, new = blob_of(n), blob_of(n + L)
                bound = len(old) + (-(-L // interval) + 1) * closed
                assert len(new) <= bound, (interval, n, L, len(old), len(new), bound)
