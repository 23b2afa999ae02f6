"""CPU tier: writing byte ranges into reset-segmented streams (tamp_batch_write_ranges, ``write_ranges``) as far as no device is
needed -- the symbol and its binding, the Python names, the keyword refusals of ``write_ranges``, the front end's sort and derived
tables, what the C call refuses before it looks for a device, the write and splice arithmetic of tamp_write_ranges.hpp compiled for
the HOST into a stand-alone program (with the address and undefined-behaviour sanitizers when the compiler has their runtimes;
nothing loaded into python is sanitised) against a restatement in Python, and the slab bound of ``out_cap=None`` against the
oracle's compressor."""
import ctypes as C
import dataclasses
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARGUMENTS = "tamp_batch_write_ranges", 24
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
        assert "write_ranges" in pkg.__all__ and pkg.write_ranges is tamp_amd.write_ranges
    # the call brings no new field: the result is a BatchResult, its index a ResetIndex
    assert [f.name for f in dataclasses.fields(tamp_amd.ResetIndex)] == ["first", "off", "interval"]
    assert [f.name for f in dataclasses.fields(tamp_amd.BatchResult)][-1] == "reset_index"


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
    good = dict(reset_index=idx, stream_index=[0, 1], begin=[0, 0], source=[b"a", b"b"])
    flat_source = dict(source=np.frombuffer(b"ab", dtype=np.uint8), source_off=[0, 1], length=[1, 1])

    def refused(match, **change):
        for args in ((data,), (flat, in_off, in_len)):
            with pytest.raises(ValueError, match=match):
                tamp_amd.write_ranges(*args, **{**good, **change})

    refused("a ResetIndex expected", reset_index=(idx.first, idx.off))
    refused("a ResetIndex expected", reset_index=None)
    for entries in (0, 2, 4):
        refused("one entry per stream and one more", reset_index=tamp_amd.ResetIndex(np.zeros(entries, np.uint64), idx.off, 16))
    refused("not given and not in the index", reset_index=tamp_amd.ResetIndex(idx.first, idx.off))  # a missing interval
    for bad in (0, -1, 1 << 32, 1.5, "16", True):
        refused("a positive integer that fits 32 bits", reset_interval=bad)
        refused("a positive integer that fits 32 bits", reset_index=tamp_amd.ResetIndex(idx.first, idx.off, bad))
    refused("one entry per write each", stream_index=[0])
    refused("one entry per write each", begin=[0, 0, 0])
    refused("one entry per write each", source=[b"a"])
    refused("one entry per write each", **{**flat_source, "length": [1]})
    refused("one entry per write each", **{**flat_source, "source_off": [0, 1, 2]})
    refused("a sequence of bytes-likes", source=b"ab")
    refused("derived from a sequence", source_off=[0, 1])
    refused("derived from a sequence", length=[1, 1])
    refused("needs source_off and length", source=flat_source["source"])
    refused("needs source_off and length", source=flat_source["source"], source_off=[0, 1])
    refused("begin: negative", begin=[0, -1])
    refused("stream_index: negative", stream_index=[-1, 0])
    refused("length: does not fit 32 bits", **{**flat_source, "length": [1, 1 << 32]})
    refused("source_off: negative", **{**flat_source, "source_off": [0, -1]})
    refused("stream_index: out of range", stream_index=[0, 2])
    refused("overlap", stream_index=[0, 0], begin=[0, 1], source=[b"ab", b"c"])
    refused("overlap", stream_index=[0, 0], begin=[1, 0], source=[b"c", b"ab"])  # (whichever order they come in)
    refused("overlap", stream_index=[1, 1], begin=[(1 << 64) - 1, (1 << 64) - 1], source=[b"ab", b"c"])  # (a sum 64 bits do not hold)
    refused("window must be in 8..15", window=16)
    refused("literal must be in 5..8", literal=4)
    refused("out_cap: one entry per stream", out_cap=[8])
    refused("out_cap: does not fit 32 bits", out_cap=1 << 32)
    # what is fine gets as far as the library: writes that touch, in any order, and writes of no bytes anywhere
    for change in (dict(), dict(stream_index=[1, 0]), dict(stream_index=[0, 0], begin=[1, 0]), dict(stream_index=[0, 0], begin=[0, 0], source=[b"", b"a"]),
                   flat_source, dict(reset_index=tamp_amd.ResetIndex(idx.first, idx.off, 0), reset_interval=16)):
        with pytest.raises(AssertionError, match="the library was loaded"):
            tamp_amd.write_ranges(data, **{**good, **change})


def test_front_end_tables():
    """The sort is stable by (stream, begin), and what a sequence of sources derives is its running sum."""
    from tamp_amd.batch import _write_tables

    # (stream, begin, length, tag): the tags ride in source_off
    rows = [(2, 10, 0, 0), (0, 7, 3, 1), (2, 10, 0, 2), (1, 0, 0, 3), (0, 0, 7, 4), (2, 10, 5, 5), (2, 3, 7, 6), (1, 0, 0, 7), (1, 0, 2, 8)]
    s, b, n, tag = _write_tables([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], 3)
    assert (s.dtype, b.dtype, n.dtype, tag.dtype) == (np.uint32, np.uint64, np.uint32, np.uint64)
    assert tag.tolist() == [4, 1, 3, 7, 8, 6, 0, 2, 5]  # equal keys keep the order they came in
    assert s.tolist() == [0, 0, 1, 1, 1, 2, 2, 2, 2] and b.tolist() == [0, 7, 0, 0, 0, 3, 10, 10, 10]
    assert n.tolist() == [7, 3, 0, 0, 2, 7, 0, 0, 5]
    # a write of no bytes goes in front of one that begins where it stands; strictly inside another it is an overlap
    s, b, n, tag = _write_tables([0, 0, 0], [5, 5, 7], [2, 0, 0], [0, 1, 2], 1)
    assert tag.tolist() == [1, 0, 2] and n.tolist() == [0, 2, 0]
    with pytest.raises(ValueError, match="overlap"):
        _write_tables([0, 0], [5, 6], [2, 0], [0, 1], 1)
    s, b, n, tag = _write_tables(np.zeros(0, np.uint32), [], np.zeros(0, np.int64), [], 0)
    assert len(s) == len(b) == len(n) == len(tag) == 0
    s, b, n, tag = _write_tables([0, 0], [(1 << 64) - 1, 5], [0, 2], [0, 0], 1)  # (a begin at the very end, of no bytes)
    assert b.tolist() == [5, (1 << 64) - 1]

    # the derived tables, seen by the library's stand-in
    import tamp_amd
    from tamp_amd import _lib

    seen = {}

    class Stop(Exception):
        pass

    class Lib:
        def tamp_amd_set_timing(self, on):
            pass

        def tamp_batch_write_ranges(self, *a):
            addr = lambda p: C.cast(p, C.c_void_p).value  # noqa: E731
            nw = a[20]
            seen["stream"] = np.ctypeslib.as_array(C.cast(addr(a[8]), C.POINTER(C.c_uint32)), (nw,)).tolist()
            seen["begin"] = np.ctypeslib.as_array(C.cast(addr(a[9]), C.POINTER(C.c_uint64)), (nw,)).tolist()
            seen["length"] = np.ctypeslib.as_array(C.cast(addr(a[10]), C.POINTER(C.c_uint32)), (nw,)).tolist()
            seen["src_off"] = np.ctypeslib.as_array(C.cast(addr(a[12]), C.POINTER(C.c_uint64)), (nw,)).tolist()
            seen["src"] = bytes(np.ctypeslib.as_array(C.cast(addr(a[11]), C.POINTER(C.c_uint8)), (6,)))
            seen["conf"] = (a[0]._obj.window, a[0]._obj.literal, a[0]._obj.extended, a[0]._obj.dictionary_reset, a[0]._obj.lazy_matching)
            seen["cap"] = np.ctypeslib.as_array(C.cast(addr(a[15]), C.POINTER(C.c_uint32)), (2,)).tolist()
            raise Stop()

    real = _lib.load
    _lib.load = lambda: Lib()
    try:
        idx = tamp_amd.ResetIndex(np.array([0, 2, 2], np.uint64), np.array([9, 20], np.uint32), 16)
        with pytest.raises(Stop):
            tamp_amd.write_ranges([bytes([0x33, 0]) + bytes(30), bytes([0x33, 0, 9])], reset_index=idx, stream_index=[1, 0, 0], begin=[0, 40, 3],
                                  source=[b"z", b"abc", b"de"], lazy_matching=True)
    finally:
        _lib.load = real
    assert seen["stream"] == [0, 0, 1] and seen["begin"] == [3, 40, 0] and seen["length"] == [2, 3, 1]
    assert seen["src_off"] == [4, 1, 0] and seen["src"] == b"zabcde"
    assert seen["conf"] == (9, 7, 1, 1, 1)  # 0x33: window 9, literal 7, extended, the reset bit
    # out_cap=None: E + 1 full segments at literal 7, and never less than the stream has
    assert seen["cap"] == [2 * (2 + (16 * 8 + 16) // 8) + 2 + (16 * 8 + 7) // 8, 2 + (16 * 8 + 7) // 8]


TABLES = ("in_off", "in_len", "reset_first", "out_off", "out_cap", "out_len", "status")
WRITE_TABLES = ("write_stream", "write_begin", "write_len", "src", "src_off")


def _arrays():
    a = dict(data=np.array([0x59, 0, 0, 0], dtype=np.uint8), in_off=np.zeros(1, np.uint64), in_len=np.full(1, 4, np.uint32),
             reset_first=np.zeros(2, np.uint64), reset_off=np.zeros(4, np.uint32), write_stream=np.zeros(1, np.uint32),
             write_begin=np.zeros(1, np.uint64), write_len=np.full(1, 1, np.uint32), src=np.zeros(8, np.uint8), src_off=np.zeros(1, np.uint64),
             out=np.zeros(64, np.uint8), out_off=np.zeros(1, np.uint64), out_cap=np.full(1, 64, np.uint32), out_len=np.zeros(1, np.uint32),
             status=np.zeros(1, np.int8), new_reset_off=np.zeros(4, np.uint32))
    return a, {k: v.ctypes.data_as(C.c_void_p) for k, v in a.items()}


def _call(lib, *, missing=(), n=1, n_writes=1, interval=16, mem=None, device=0, conf=None, no_conf=False):
    from tamp_amd import _lib

    held, p = _arrays()
    for k in missing:
        p[k] = None
    conf = conf or _lib.TampAmdConf(10, 8, 0, 1, 1, 0, 0)
    rc = lib.tamp_batch_write_ranges(None if no_conf else C.byref(conf), 15, p["data"], p["in_off"], p["in_len"], p["reset_first"], p["reset_off"],
                                     interval, p["write_stream"], p["write_begin"], p["write_len"], p["src"], p["src_off"], p["out"],
                                     p["out_off"], p["out_cap"], p["out_len"], p["status"], p["new_reset_off"], n, n_writes,
                                     _lib.MEM_HOST if mem is None else mem, device, None)
    del held
    return rc


def test_call_level_refusals(lib):
    """Before a device is looked for: TAMP_AMD_BAD_ARGUMENT on a machine with and without one, for both memory kinds."""
    from tamp_amd import _lib

    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        for table in TABLES:
            assert _call(lib, missing=(table,), mem=mem) == BAD_ARGUMENT, table
            assert _call(lib, missing=(table,), mem=mem, n_writes=0) == BAD_ARGUMENT, table
        for table in WRITE_TABLES:
            assert _call(lib, missing=(table,), mem=mem) == BAD_ARGUMENT, table
        assert _call(lib, missing=("data",), mem=mem) == BAD_ARGUMENT
        assert _call(lib, missing=("out",), mem=mem) == BAD_ARGUMENT
        assert _call(lib, no_conf=True, mem=mem) == BAD_ARGUMENT
        assert _call(lib, interval=0, mem=mem) == BAD_ARGUMENT
        assert _call(lib, interval=0xFFFFFFFF, mem=mem) == BAD_ARGUMENT  # (a worst-case segment that does not fit 32 bits)
        assert _call(lib, device=_lib.ALL_DEVICES, mem=mem) == BAD_ARGUMENT
        assert _call(lib, n=1 << 32, mem=mem) == BAD_ARGUMENT
        assert _call(lib, n_writes=1 << 32, mem=mem) == BAD_ARGUMENT
        # conf: the reset bit is required, a custom dictionary is not taken, the fields must be in range
        for conf in (_lib.TampAmdConf(10, 8, 0, 1, 0, 0, 0), _lib.TampAmdConf(10, 8, 1, 1, 1, 0, 0), _lib.TampAmdConf(7, 8, 0, 1, 1, 0, 0),
                     _lib.TampAmdConf(10, 9, 0, 1, 1, 0, 0), _lib.TampAmdConf(10, 8, 0, 1, 1, 2, 0)):
            assert _call(lib, conf=conf, mem=mem) == BAD_ARGUMENT
        assert _call(lib, n=0, missing=("data", "out", "reset_off", "new_reset_off") + WRITE_TABLES, n_writes=0, mem=mem) == 0  # nothing is done
    for mem in (2, -1, 7):
        assert _call(lib, mem=mem) == BAD_ARGUMENT


PROGRAM = r"""
#include "tamp_write_ranges.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace tamp_amd;
typedef unsigned long long ull;

// Reads cases, one per line, and answers each with one line; the caller holds the restatement.
//   span E N begin len        -> ok k0 k1 lo hi, then per piece: lo hi skip
//   order ps pb pl s b        -> 0 / 1
//   splice E closed.. len..   -> total, then per segment its start, then the E entries (len: the slab length of a touched segment when
//                                its flag is 1 or 2 -- 2: the open one --, the old span when it is 0)
int main() {
    char what[16];
    long cases = 0;
    while (scanf("%15s", what) == 1) {
        cases++;
        if (!strcmp(what, "span")) {
            ull E, N, begin, len;
            if (scanf("%llu %llu %llu %llu", &E, &N, &begin, &len) != 4) return 2;
            const WriteSpan s = write_span(E, (uint32_t)N, begin, (uint32_t)len);
            printf("%d %llu %llu %u %u", s.ok ? 1 : 0, (ull)s.k0, (ull)s.k1, s.lo, s.hi);
            if (s.ok)
                for (uint64_t j = 0; j <= s.k1 - s.k0 && j < 8; j++) {
                    const WritePiece p = write_piece(s, (uint32_t)N, j);
                    printf(" %u %u %llu", p.lo, p.hi, (ull)p.skip);
                }
            printf("\n");
        } else if (!strcmp(what, "order")) {
            ull ps, pb, pl, s, b;
            if (scanf("%llu %llu %llu %llu %llu", &ps, &pb, &pl, &s, &b) != 5) return 2;
            printf("%d\n", write_in_order((uint32_t)ps, pb, (uint32_t)pl, (uint32_t)s, b) ? 1 : 0);
        } else if (!strcmp(what, "splice")) {
            ull E;
            if (scanf("%llu", &E) != 1) return 2;
            std::vector<uint32_t> len(E + 1);
            for (ull k = 0; k <= E; k++) {
                ull flag, v;
                if (scanf("%llu %llu", &flag, &v) != 2) return 2;
                len[k] = flag ? write_unit_span((uint32_t)v, flag == 1) : (uint32_t)v;
            }
            std::vector<uint64_t> start(E + 1), entry(E + 1);
            const uint64_t total = write_splice(len.data(), E, start.data(), entry.data());
            printf("%llu", (ull)total);
            for (ull k = 0; k <= E; k++) printf(" %llu", (ull)start[k]);
            for (ull k = 0; k < E; k++) printf(" %llu", (ull)entry[k]);
            printf("\n");
        } else return 3;
    }
    static_assert(write_fail_key(3, kWriteRankEnd, 2) < write_fail_key(3, kWriteRankOob, -4), "of one write's rules the first");
    static_assert(write_fail_key(2, kWriteRankExcess, -2) < write_fail_key(3, kWriteRankOrder, -21), "the lowest write first");
    static_assert(write_fail_key(0xFFFFFFFFull, kWriteRankCompress, -1) < kWriteNoFail, "every key lies below 'none'");
    static_assert(write_fail_code(write_fail_key(7, kWriteRankIndex, -22)) == -22 && write_fail_code(write_fail_key(7, kWriteRankEnd, 2)) == 2, "the code rides along");
    static_assert(write_row_bytes(1) == 16 && write_row_bytes(16) == 16 && write_row_bytes(17) == 32 && write_row_bytes(0xFFFFFFF0u) == 0xFFFFFFF0u, "rows");
    fprintf(stderr, "%ld cases\n", cases);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("write_ranges")
    (d / "writes.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), str(d / "writes.cpp"), "-o", str(d / "writes")]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizers' runtimes)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "writes"), sanitized


def span_py(E, N, begin, length):
    """A write against a plain walk over the bytes' segments: (ok, k0, k1, lo, hi, pieces)."""
    k0 = begin // N
    if length == 0 or k0 > E:
        return (0, k0, 0, 0, 0, [])
    last = begin + length - 1  # (Python integers: no overflow)
    k1 = last // N
    if k1 > E:
        return (0, k0, 0, 0, 0, [])
    pieces = []
    for k in range(k0, k1 + 1):
        lo, hi = max(begin, k * N), min(begin + length, (k + 1) * N)
        pieces.append((lo - k * N, hi - k * N, lo - begin))
    return (1, k0, k1, begin - k0 * N, last - k1 * N + 1, pieces)


def test_write_and_splice_arithmetic(program):
    """Random writes at intervals 1, 7 and 64 -- among them writes that end exactly on a segment boundary, writes of one whole segment,
    and begins around 2^32 and at the top of 64 bits --, the order rule, and random splices: against the restatement above."""
    exe, sanitized = program
    rng = random.Random(20240607)
    lines, wants = [], []
    for N in (1, 7, 64):
        for _ in range(1500):
            E = rng.choice((0, 1, 2, 5, 40, (1 << 32) // N + 3, (1 << 40)))
            shape = rng.randrange(6)
            if shape == 0:  # ends exactly on a boundary
                k = rng.randrange(0, min(E, 50) + 1)
                length = rng.randrange(1, 3 * N + 1)
                begin = max((k + 1) * N - length, 0)
                length = (k + 1) * N - begin
            elif shape == 1:  # exactly one segment
                begin, length = rng.randrange(0, min(E, 50) + 1) * N, N
            elif shape == 2:  # around 2^32
                begin, length = (1 << 32) + rng.randrange(-3 * N - 2, 3 * N + 3), rng.randrange(0, 3 * N + 2)
            elif shape == 3:  # around the open segment's end
                begin, length = max((E + 1) * N + rng.randrange(-2 * N - 1, 2), 0), rng.randrange(0, 2 * N + 2)
            elif shape == 4:  # the top of 64 bits and of 32
                begin, length = (1 << 64) - 1 - rng.randrange(0, 3), rng.choice((0, 1, 2, (1 << 32) - 1))
            else:
                begin, length = rng.randrange(0, (min(E, 50) + 2) * N), rng.randrange(0, 3 * N + 2)
            lines.append("span %d %d %d %d" % (E, N, begin, length))
            ok, k0, k1, lo, hi, pieces = span_py(E, N, begin, length)
            want = [ok, k0, k1, lo, hi] if ok else [0, k0, 0, 0, 0]
            for p in pieces[:8]:
                want += list(p)
            wants.append(want)
    for _ in range(600):
        ps, s = rng.randrange(0, 4), rng.randrange(0, 4)
        pb = rng.choice((0, 5, (1 << 32) - 1, (1 << 64) - 2))
        pl = rng.choice((0, 1, 3, (1 << 32) - 1))
        b = rng.choice((0, 4, 5, 6, 8, pb, (pb + pl) % (1 << 64), max(pb + pl - 1, 0) % (1 << 64), (1 << 64) - 1))
        lines.append("order %d %d %d %d %d" % (ps, pb, pl, s, b))
        wants.append([int(s > ps or (s == ps and pb + pl < (1 << 64) and b >= pb + pl))])
    for _ in range(600):
        E = rng.randrange(0, 12)
        segs = [(rng.randrange(0, 2), rng.randrange(2, 90)) for _ in range(E + 1)]  # (touched?, slab length / old span)
        words, new_len = [], []
        for k, (touched, v) in enumerate(segs):
            flag = 0 if not touched else (1 if k < E else 2)
            words += [flag, v]
            new_len.append(v if flag == 0 else (v if flag == 1 else v - 2))  # a closed unit: - lead + the next lead; the open one: - lead
        lines.append("splice %d %s" % (E, " ".join(map(str, words))))
        starts, at = [], 2
        for v in new_len:
            starts.append(at)
            at += v
        wants.append([at] + starts + [starts[k] + new_len[k] for k in range(E)])
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
    """``out_cap=None``: the bound of E + 1 full segments is at least what the oracle's compressor makes of random PATCHED data of a
    stream with E resets, whatever its open segment holds -- random bytes of the literal width are the worst case, (nearly) every
    byte a literal."""
    from tamp_amd.batch import _write_bound, compress_resets_bound

    rng = random.Random(literal)
    for interval in (1, 16, 100, 256):
        for n in (0, 1, interval, interval + 1, 3 * interval, 3 * interval + 1, rng.randrange(1, 6 * interval + 2)):
            data = bytearray(rng.randrange(1 << literal) for _ in range(n))
            for _ in range(3):  # patched: random writes of random bytes
                if n:
                    at = rng.randrange(n)
                    ln = rng.randrange(0, n - at + 1)
                    data[at : at + ln] = bytes(rng.randrange(1 << literal) for _ in range(ln))
            data = bytes(data)
            E = max(1, -(-n // interval)) - 1
            bound = int(_write_bound(np.array([E], dtype=np.uint64), interval, literal)[0])
            assert bound == compress_resets_bound((E + 1) * interval, interval, literal) >= compress_resets_bound(n, interval, literal)
            ops = []
            for at in range(0, max(n, 1), interval):
                ops += ([("reset",)] if at else []) + [("write", data[at : at + interval])]
            res, blob = oracle.stream_script(ops + [("flush", False)], window=8, literal=literal, dictionary_reset=True)
            assert res == 0 and len(blob) <= bound, (interval, n, len(blob), bound)
