"""CPU tier: byte ranges of streams whose reset segments differ in size (tamp_batch_segment_ends, tamp_batch_read_ranges_grid,
``ResetScan.segment_ends``, ``read_ranges(..., segment_ends=)``) as far as no device is needed -- the two symbols and their bindings,
the Python names, the new keyword refusals of ``read_ranges``, what the C calls refuse before they look for a device, the host-memory
form of the ends call against numpy, the ``read`` command's parser, and the table arithmetic of tamp_reset_segments.hpp compiled for
the HOST into a stand-alone program with the address and undefined-behaviour sanitizers when the compiler has their runtimes
(nothing loaded into python is sanitised)."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ, READ_ARGUMENTS = "tamp_batch_read_ranges_grid", 19
ENDS, ENDS_ARGUMENTS = "tamp_batch_segment_ends", 8
BAD_ARGUMENT = -21
SATURATED = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_symbols_and_bindings(lib):
    from tamp_amd import _lib

    header = open(os.path.join(ROOT, "include", "tamp_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    nm = shutil.which("nm")
    exported = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout if nm else None
    for name, arguments in ((READ, READ_ARGUMENTS), (ENDS, ENDS_ARGUMENTS)):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m and len(m[1].split(",")) == arguments, name
        assert name in _lib.SYMBOLS and hasattr(C.CDLL(_lib.LIB_PATH), name)
        fn = getattr(lib, name)
        assert len(fn.argtypes) == arguments and fn.restype is C.c_int
        if exported is not None:
            assert re.search(r" T %s$" % name, exported, flags=re.M)
    # the table stands where the interval stood: the same parameters around it
    fixed = re.search(r"\btamp_batch_read_ranges\s*\(([^;]*)\)\s*;", code)[1]
    grid = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % READ, code)[1]
    squeeze = lambda text: [" ".join(p.split()) for p in text.split(",")]  # noqa: E731
    assert squeeze(grid) == [p if p != "uint32_t reset_interval" else "const uint64_t *segment_end" for p in squeeze(fixed)]
    assert "const uint64_t *segment_end" in squeeze(grid)


def test_python_names():
    import tamp
    import tamp_amd

    for pkg in (tamp_amd, tamp):
        for name in ("segment_ends", "read_ranges", "ResetScan", "index_resets"):
            assert name in pkg.__all__ and getattr(pkg, name) is getattr(tamp_amd, name)
    # neither dataclass moved: the first five fields of ResetScan, interval as the last of ResetIndex
    assert [f.name for f in dataclasses.fields(tamp_amd.ResetScan)][:5] == ["index", "status", "closed_size", "open_size", "kernel_ms"]
    assert [f.name for f in dataclasses.fields(tamp_amd.ResetScan)][-1] == "_keep"
    assert [f.name for f in dataclasses.fields(tamp_amd.ResetIndex)][-1] == "interval"
    assert callable(tamp_amd.ResetScan.segment_ends)
    import inspect

    assert "segment_ends" in inspect.signature(tamp_amd.read_ranges).parameters


def test_segment_ends_host_memory(lib):
    """The host-memory form needs no device: against numpy, streams without entries, a saturated size, the table cached."""
    import tamp_amd

    rng = np.random.default_rng(7)
    for n in (1, 2, 17, 300):
        counts = rng.integers(0, 6, n)
        if n == 17:
            counts[3] = 1500  # (more rows than a scan tile, for what the host form cares)
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        closed = rng.integers(0, 701, int(first[n])).astype(np.uint32)
        opens = rng.integers(0, 701, n).astype(np.uint32)
        if n == 300:
            closed[int(first[5]) + 1 if counts[5] > 1 else 0] = 0xFFFFFFFF
        want = []
        for i in range(n):
            sizes = [int(x) for x in closed[int(first[i]):int(first[i + 1])]] + [int(opens[i])]
            run, dead = 0, False
            for s in sizes:
                dead |= s == 0xFFFFFFFF
                run += s
                want.append(SATURATED if dead else run)
        scan = tamp_amd.ResetScan(tamp_amd.ResetIndex(first, np.zeros(int(first[n]), np.uint32)), np.zeros(n, np.int8), closed, opens)
        got = scan.segment_ends()
        assert got.dtype == np.uint64 and len(got) == int(first[n]) + n
        assert [int(x) for x in got] == want
        assert scan.segment_ends() is got
        if not np.any(closed == 0xFFFFFFFF):
            assert [scan.size(i) for i in range(n)] == [int(got[int(first[i + 1]) + i]) for i in range(n)]
    # behind guard words, through the C entry
    first, closed, opens = np.array([0, 0, 2, 2], np.uint64), np.array([5, 0], np.uint32), np.array([3, 0, 9], np.uint32)
    room = np.full(5 + 4, 0xAB, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.tamp_batch_segment_ends(p(first), p(closed), p(opens), p(room[2:]), 3, 0, 0, None) == 0
    assert list(room) == [0xAB, 0xAB, 3, 5, 5, 5, 9, 0xAB, 0xAB]
    assert lib.tamp_batch_segment_ends(p(first[:1]), None, None, p(room), 0, 0, 0, None) == 0 and room[0] == 0xAB


def test_keyword_refusals_come_before_the_library(monkeypatch):
    """Every new refusal is a ValueError raised before the native library is looked for; an interval is not needed and not looked at."""
    import tamp_amd
    from tamp_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded before the keywords were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    data = [b"abc", b"defg"]
    flat, in_off, in_len = tamp_amd.pack_streams(data)
    idx = tamp_amd.ResetIndex(np.array([0, 1, 3], np.uint64), np.array([2, 2, 3], np.uint32))
    good = dict(reset_index=idx, stream_index=[0, 1], begin=[0, 0], length=[1, 1], segment_ends=np.zeros(5, np.uint64))

    def refused(match, **change):
        for args in ((data,), (flat, in_off, in_len)):
            with pytest.raises(ValueError, match=match):
                tamp_amd.read_ranges(*args, **{**good, **change})

    for entries in (0, 3, 4, 6):
        refused("one entry per segment", segment_ends=np.zeros(entries, np.uint64))
    refused("one entry per segment", segment_ends=[1, 2, 3])
    refused("1-D table of integers", segment_ends=np.zeros((5, 1), np.uint64))
    refused("1-D table of integers", segment_ends=np.zeros(5, np.float64))
    refused("1-D table of integers", segment_ends=np.zeros(5, bool))
    refused("does not fit 64 bits", segment_ends=[0, 1, 2, 3, 1 << 64])
    refused("does not fit 64 bits", segment_ends=np.array([0, 1, -2, 3, 4], np.int64))
    import torch

    refused("1-D table of integers", segment_ends=torch.zeros(5, dtype=torch.float32))
    refused("one entry per segment", segment_ends=torch.zeros(4, dtype=torch.int64))
    # what the fixed form refuses it still refuses, with and without the table
    refused("a ResetIndex expected", reset_index=None)
    refused("one entry per range each", stream_index=[0])
    with pytest.raises(ValueError, match="not given and not in the index"):
        tamp_amd.read_ranges(data, **{**good, "segment_ends": None})
    # what is fine gets as far as the library: no interval, an interval that would be refused, sequences and host tensors
    for change in ({}, {"reset_interval": 0}, {"reset_interval": "x"}, {"segment_ends": [3, 3, 4, 5, SATURATED]},
                   {"segment_ends": torch.zeros(5, dtype=torch.int64)}, {"segment_ends": np.zeros(5, np.int32)},
                   {"reset_index": tamp_amd.ResetIndex(idx.first, idx.off, 16)}):
        with pytest.raises(AssertionError, match="the library was loaded"):
            tamp_amd.read_ranges(data, **{**good, **change})


TABLES = ("in_off", "in_len", "reset_first", "range_stream", "range_begin", "range_len", "out_off", "out_len", "status")


def _read_call(lib, *, missing=(), n=1, n_ranges=1, mem=0, device=0):
    a = dict(data=np.array([0x59, 0, 0, 0], dtype=np.uint8), in_off=np.zeros(1, np.uint64), in_len=np.full(1, 4, np.uint32),
             reset_first=np.zeros(2, np.uint64), reset_off=np.zeros(4, np.uint32), segment_end=np.zeros(1, np.uint64),
             range_stream=np.zeros(1, np.uint32), range_begin=np.zeros(1, np.uint64), range_len=np.full(1, 8, np.uint32),
             out=np.zeros(64, np.uint8), out_off=np.zeros(1, np.uint64), out_len=np.zeros(1, np.uint32), status=np.zeros(1, np.int8))
    p = {k: (None if k in missing else v.ctypes.data_as(C.c_void_p)) for k, v in a.items()}
    return lib.tamp_batch_read_ranges_grid(15, p["data"], p["in_off"], p["in_len"], p["reset_first"], p["reset_off"], p["segment_end"],
                                           p["range_stream"], p["range_begin"], p["range_len"], p["out"], p["out_off"], p["out_len"],
                                           p["status"], n, n_ranges, mem, device, None)


def _ends_call(lib, *, missing=(), n=1, mem=0, device=0, entries=0):
    a = dict(reset_first=np.array([0, entries], np.uint64), closed_size=np.zeros(max(entries, 1), np.uint32), open_size=np.zeros(1, np.uint32),
             segment_end=np.zeros(entries + 1, np.uint64))
    p = {k: (None if k in missing else v.ctypes.data_as(C.c_void_p)) for k, v in a.items()}
    return lib.tamp_batch_segment_ends(p["reset_first"], p["closed_size"], p["open_size"], p["segment_end"], n, mem, device, None)


def test_call_level_refusals(lib):
    """Before a device is looked for: TAMP_AMD_BAD_ARGUMENT on a machine with and without one, for both memory kinds."""
    from tamp_amd import _lib

    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        for table in TABLES:
            assert _read_call(lib, missing=(table,), mem=mem) == BAD_ARGUMENT, table
            assert _read_call(lib, missing=(table,), mem=mem, n_ranges=0) == BAD_ARGUMENT, table
            assert _read_call(lib, missing=(table, "reset_off"), mem=mem) == BAD_ARGUMENT, table
        assert _read_call(lib, missing=("data",), mem=mem) == BAD_ARGUMENT
        assert _read_call(lib, missing=("out",), mem=mem) == BAD_ARGUMENT
        assert _read_call(lib, missing=("segment_end",), mem=mem) == BAD_ARGUMENT
        assert _read_call(lib, missing=("segment_end",), mem=mem, n_ranges=0) == BAD_ARGUMENT
        assert _read_call(lib, device=_lib.ALL_DEVICES, mem=mem) == BAD_ARGUMENT
        assert _read_call(lib, n=1 << 32, mem=mem) == BAD_ARGUMENT
        assert _read_call(lib, n_ranges=1 << 32, mem=mem) == BAD_ARGUMENT
        assert _read_call(lib, n_ranges=0, mem=mem) in (0, -20)
        for table in ("reset_first", "segment_end", "open_size"):
            assert _ends_call(lib, missing=(table,), mem=mem) == BAD_ARGUMENT, table
        assert _ends_call(lib, missing=("reset_first",), mem=mem, n=0) == BAD_ARGUMENT
        assert _ends_call(lib, missing=("segment_end",), mem=mem, n=0) == BAD_ARGUMENT
        assert _ends_call(lib, missing=("closed_size",), mem=mem, entries=1) == BAD_ARGUMENT
        assert _ends_call(lib, device=_lib.ALL_DEVICES, mem=mem) == BAD_ARGUMENT
        assert _ends_call(lib, n=1 << 32, mem=mem) == BAD_ARGUMENT
        assert _ends_call(lib, missing=("open_size", "closed_size"), mem=mem, n=0) == 0  # (no streams: nothing is done)
    assert _ends_call(lib, missing=("closed_size",), mem=_lib.MEM_HOST) == 0  # (host memory: no entry to read through it)
    for mem in (2, -1, 7):
        assert _read_call(lib, mem=mem) == BAD_ARGUMENT
        assert _read_call(lib, mem=mem, device=_lib.ALL_DEVICES) == BAD_ARGUMENT
        assert _ends_call(lib, mem=mem) == BAD_ARGUMENT


def test_cli_parser_accepts_read():
    from tamp_amd import cli

    ap = cli.build_parser()
    a = ap.parse_args(["read", "log.tamp", "--begin", "100", "--length", "7"])
    assert (a.command, a.file, a.begin, a.length, a.output) == ("read", "log.tamp", 100, 7, None)
    a = ap.parse_args(["read", "log.tamp", "--begin", str((1 << 64) - 1), "--length", str((1 << 32) - 1), "-o", "out.bin"])
    assert (a.begin, a.length, a.output) == ((1 << 64) - 1, (1 << 32) - 1, "out.bin")
    for bad in (["read", "log.tamp", "--begin", "0"], ["read", "--begin", "0", "--length", "1"],
                ["read", "log.tamp", "--begin", "-1", "--length", "1"], ["read", "log.tamp", "--begin", "0", "--length", str(1 << 32)]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_cli_read_refuses_a_stream_without_the_reset_bit(tmp_path, capsys, monkeypatch):
    """The message comes from the header byte alone: before the library is looked for."""
    from tamp_amd import _lib, cli

    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    f = tmp_path / "plain.tamp"
    f.write_bytes(bytes([0x58, 0xB3, 0x04]))
    assert cli.main(["read", str(f), "--begin", "0", "--length", "1"]) == 1
    assert "no dictionary resets" in capsys.readouterr().err
    assert cli.main(["read", str(tmp_path / "none.tamp"), "--begin", "0", "--length", "1"]) == 1


PROGRAM = r"""
#include "tamp_reset_segments.hpp"
#include <cstdio>
#include <vector>
using namespace tamp_amd;

static int failures = 0;
static long checked = 0, streams = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGUMENTS__); printf("\n"); } } } while (0)
typedef unsigned long long ull;

// One stream of K segments of the given decoded sizes (the last one open) among two others, all tables sized exactly (an entry read
// behind a table is an address error).
struct Batch {
    uint64_t n = 3, i = 1, E;
    std::vector<uint64_t> first, in_off, ends;
    std::vector<uint32_t> off, in_len, clen;
    std::vector<uint8_t> in;
    Batch(const std::vector<uint32_t>& size) {
        const uint32_t K = (uint32_t)size.size();
        E = K - 1;
        first = {0, 2, 2 + E, 3 + E};
        off.assign(3 + E, 0), in_len = {30, 0, 9}, clen.assign(K, 0);
        off[0] = 7, off[1] = 19, off[2 + E] = 5;
        uint32_t at = kResetHeaderBytes;
        for (uint32_t k = 0; k < K; k++) {  // (compressed bytes: a closed segment holds its FLUSH, FLUSH at least, the open one may be empty)
            clen[k] = k < E ? 3 + (k * 5 + size[k]) % 4 : (size[k] ? 1 + size[k] % 3 : 0);
            at += clen[k];
            if (k < E) off[2 + k] = at;
        }
        in_len[i] = at;
        in_off = {0, 30, 30 + (uint64_t)at};
        in.assign(30 + at + 9, 0xCC);
        for (uint64_t s = 0; s < n; s++) in[in_off[s]] = 0x59, in[in_off[s] + 1] = 0;  // window 10, literal 8, the reset bit
        // the table through the function that makes it: 3 + 1 segments in front, 1 + 1 behind
        std::vector<uint32_t> closed = {11, 12}, open = {13, size[E], 21};
        for (uint32_t k = 0; k < E; k++) closed.push_back(size[k]);
        closed.push_back(20);
        ends.assign(first[n] + n, 0);
        segment_ends_fill(first.data(), closed.data(), open.data(), ends.data(), n);
    }
    ReadGridPlan plan(uint64_t begin, uint32_t len, uint32_t stream = 1, uint64_t budget = 1ull << 40) const {
        return read_grid_plan(in.data(), in_off.data(), in_len.data(), first.data(), off.data(), ends.data(), n, 15, budget, stream, begin, len);
    }
    ReadGridUnit unit(const ReadGridPlan& g, uint64_t j, uint32_t stream = 1) const {
        return read_grid_unit(first.data(), off.data(), in_len.data(), ends.data(), stream, g, j);
    }
};

// Every range of such a stream against a plain walk over its segments.
static void stream(const std::vector<uint32_t>& size) {
    const Batch t(size);
    const uint32_t K = (uint32_t)size.size();
    const uint64_t E = t.E;
    streams++;
    std::vector<uint64_t> B(K + 1, 0);
    for (uint32_t k = 0; k < K; k++) B[k + 1] = B[k] + size[k];
    const uint64_t total = B[K];
    CHECK(t.ends[0] == 11 && t.ends[2] == 36 && t.ends[t.first[2] + 2] == 20 && t.ends[t.first[2] + 3] == 41, "the neighbours' rows");
    for (uint32_t k = 0; k < K; k++) CHECK(t.ends[segment_end_row(t.first.data(), 1) + k] == B[k + 1], "row %u of the table", k);
    std::vector<uint64_t> begins, lens;
    for (uint64_t b = 0; b <= total + 2; b++) begins.push_back(b);
    for (uint64_t l = 0; l <= total + 2; l++) lens.push_back(l);
    for (uint64_t big : {(1ull << 32) - 2, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 1, ~0ull - 1, ~0ull}) {
        begins.push_back(big);
        if (big <= 0xFFFFFFFFull) lens.push_back(big);
    }
    for (uint64_t begin : begins)
        for (uint64_t len64 : lens) {
            const uint32_t len = (uint32_t)len64;
            const ReadGridPlan g = t.plan(begin, len);
            const ReadPlan& p = g.p;
            checked++;
            if (len == 0) {
                CHECK(p.verdict == kReadOk && p.units == 0, "an empty range");
                continue;
            }
            if (begin >= total) {
                CHECK(p.verdict == kReadInputExhausted && p.units == 0, "begin %llu len %u: at or behind the end", (ull)begin, len);
                continue;
            }
            const uint64_t sum = begin + len < begin ? ~0ull : begin + len, end = sum < total ? sum : total;
            // the walk: the segment that holds `begin`, the one that holds the last byte, everything between them (empty ones too)
            uint64_t k0 = 0, k1 = 0;
            for (uint32_t k = 0; k < K; k++) {
                if (B[k] <= begin && begin < B[k + 1]) k0 = k;
                if (B[k] <= end - 1 && end - 1 < B[k + 1]) k1 = k;
            }
            const uint64_t units = k1 - k0 + 1;
            CHECK(p.verdict == kReadGo && p.k0 == k0 && p.units == units && k0 <= E, "begin %llu len %u: verdict %d k0 %llu units %llu (want %llu, %llu)",
                  (ull)begin, len, p.verdict, (ull)p.k0, (ull)p.units, (ull)k0, (ull)units);
            if (p.verdict != kReadGo || p.units != units || p.k0 != k0) continue;
            uint32_t cut0 = kResetHeaderBytes;
            for (uint64_t k = 0; k < k0; k++) cut0 += t.clen[k];
            uint64_t staged = 0;
            for (uint64_t k = k0; k <= k1; k++) staged += t.clen[k] + kResetHeaderBytes;
            CHECK(p.scratch == end - B[k0] && p.staged == staged && p.span_start == cut0 && p.last_need == end - B[k1], "begin %llu len %u: scratch %llu staged %llu",
                  (ull)begin, len, (ull)p.scratch, (ull)p.staged);
            CHECK(g.base == B[k0] && g.skip == begin - B[k0] && g.skip < size[k0], "begin %llu len %u: the gather offset %llu", (ull)begin, len, (ull)g.skip);
            CHECK(read_plan_cost(p) == p.scratch + staged + units * kReadUnitRow, "the cost");
            uint64_t place = 0, sum_need = 0, decoded = 0;
            uint32_t cut = cut0;
            for (uint64_t j = 0; j < units; j++) {
                const uint64_t k = k0 + j;
                const ReadGridUnit w = t.unit(g, j);
                const ReadUnit& u = w.u;
                CHECK(u.cut.ok && u.cut.start == cut && u.cut.end == cut + t.clen[k] && u.cut.closed == (k < E), "begin %llu len %u unit %llu: cut %u..%u",
                      (ull)begin, len, (ull)j, u.cut.start, u.cut.end);
                const uint64_t need = k == k1 ? end - B[k1] : size[k];
                CHECK(w.size == size[k] && u.need == need && u.room == B[k] - B[k0], "begin %llu len %u unit %llu: size %u need %u room %llu", (ull)begin, len,
                      (ull)j, w.size, u.need, (ull)u.room);
                CHECK(u.place == place && u.in_len == t.clen[k] + kResetHeaderBytes, "begin %llu len %u unit %llu: place %llu", (ull)begin, len, (ull)j, (ull)u.place);
                CHECK(u.room + u.need <= p.scratch && u.place + u.in_len <= p.staged, "unit %llu stays inside the range's scratch and stage", (ull)j);
                place += u.in_len, sum_need += u.need, cut += t.clen[k];
                decoded += size[k] < u.need ? size[k] : u.need;  // (what the unit decodes to: min(its size, need))
            }
            CHECK(sum_need == p.scratch, "the scratch against the sum over the units");
            uint64_t delivered = 0;
            if (len <= 64) { for (uint64_t b = begin; b - begin < len; b++) delivered += b < total; }
            else delivered = total - begin < len ? total - begin : len;
            CHECK(delivered == end - begin && read_range_delivered(decoded, g.skip, len) == delivered, "begin %llu len %u: delivered %u (want %llu)", (ull)begin, len,
                  read_range_delivered(decoded, g.skip, len), (ull)delivered);
        }
    // the neighbours are not disturbed by this one's rows
    CHECK(t.plan(0, 1, 0).p.verdict == kReadGo && t.plan(0, 1, 0).p.staged == 7 - 2 + 2 && t.plan(36, 1, 0).p.verdict == kReadInputExhausted, "stream 0");
    CHECK(t.plan(20, 5, 2).p.verdict == kReadGo && t.plan(20, 5, 2).p.staged == 9 - 5 + 2 && t.plan(20, 5, 2).p.k0 == 1 && t.plan(41, 1, 2).p.verdict == kReadInputExhausted, "stream 2");
    CHECK(t.plan(0, 1, 3).p.verdict == kReadBadArgument && t.plan(0, 0, 3).p.verdict == kReadBadArgument, "a stream there is none of");
}

// Equal sizes: the same plan and units as the fixed form with that N, wherever the range ends inside the stream.
static void against_fixed(uint32_t K, uint32_t N, uint32_t open) {
    std::vector<uint32_t> size(K, N);
    size[K - 1] = open;
    const Batch t(size);
    const uint64_t total = (uint64_t)(K - 1) * N + open;
    for (uint64_t begin = 0; begin < total; begin++)
        for (uint64_t len = 1; begin + len <= total; len++) {
            const ReadPlan f = read_range_plan(t.in.data(), t.in_off.data(), t.in_len.data(), t.first.data(), t.off.data(), t.n, N, 15, 1ull << 40, 1, begin, (uint32_t)len);
            const ReadGridPlan g = t.plan(begin, (uint32_t)len);
            checked++;
            CHECK(f.verdict == kReadGo && g.p.verdict == f.verdict && g.p.k0 == f.k0 && g.p.units == f.units && g.p.scratch == f.scratch && g.p.staged == f.staged &&
                  g.p.last_need == f.last_need && g.p.span_start == f.span_start, "K %u N %u begin %llu len %llu: the plans differ", K, N, (ull)begin, (ull)len);
            CHECK(g.skip == read_range_skip(begin, f.k0, N), "the skip");
            for (uint64_t j = 0; j < f.units && j < g.p.units; j++) {
                const ReadUnit a = read_range_unit(t.first.data(), t.off.data(), t.in_len.data(), N, 1, f, j), b = t.unit(g, j).u;
                CHECK(a.cut.ok && b.cut.ok && a.cut.start == b.cut.start && a.cut.end == b.cut.end && a.cut.closed == b.cut.closed && a.need == b.need &&
                      a.in_len == b.in_len && a.place == b.place && a.room == b.room, "K %u N %u begin %llu len %llu unit %llu: the units differ", K, N, (ull)begin, (ull)len, (ull)j);
            }
        }
}

// true: the range is refused as TAMP_AMD_BAD_INDEX -- by its plan, or by one of its units
static bool refused(const Batch& t, uint64_t begin, uint32_t len) {
    const ReadGridPlan g = t.plan(begin, len);
    if (g.p.verdict == kReadBadIndex) return true;
    if (g.p.verdict != kReadGo) return false;
    bool bad = false;
    for (uint64_t j = 0; j < g.p.units; j++) {
        const ReadGridUnit w = t.unit(g, j);
        bad |= !w.u.cut.ok;
        if (!w.u.cut.ok) CHECK(w.u.in_len == 0 && w.u.need == 0 && w.u.room == 0 && w.size == 0, "a unit without a cut has no bytes and no room");
    }
    return bad;
}

// Hand-made tables: five segments of 4 bytes, rows 4 8 12 16 20 at r .. r + 4.
static void bad_tables() {
    const Batch good(std::vector<uint32_t>(5, 4));
    const uint64_t r = segment_end_row(good.first.data(), 1);
    for (uint64_t k = 0; k < 5; k++) CHECK(good.ends[r + k] == 4 * (k + 1) && !refused(good, 4 * k + 1, 2), "the good table");
    CHECK(!refused(good, 0, 20) && good.plan(0, 20).p.units == 5, "the whole stream");
    {   // a decreasing entry INSIDE the touched span
        Batch t = good;
        t.ends[r + 2] = 7;
        CHECK(refused(t, 5, 10), "a decreasing entry inside the span");
        CHECK(refused(t, 0, 20), "... and in the range of the whole stream");
        // (byte 9 lies in the span the forged entry opened for segment 3, 7 .. 16: a size the WALK will not find in that segment)
        CHECK(!refused(t, 9, 1) && t.plan(9, 1).p.k0 == 3 && t.unit(t.plan(9, 1), 0).size == 9, "a range the forged entry sends to its neighbour");
        CHECK(!refused(t, 1, 2) && t.plan(1, 2).p.verdict == kReadGo, "segment 0 is not touched by it");
        CHECK(!refused(t, 17, 3) && t.plan(17, 3).p.verdict == kReadGo && t.plan(17, 3).p.k0 == 4, "segment 4 is not touched by it");
    }
    {   // ... IN FRONT of it: the touched segments hold up, the range goes
        Batch t = good;
        t.ends[r + 0] = 9;
        const ReadGridPlan g = t.plan(13, 2), w = good.plan(13, 2);
        CHECK(g.p.verdict == kReadGo && g.p.k0 == w.p.k0 && g.p.units == 1 && g.skip == w.skip && !refused(t, 13, 2), "a decreasing entry in front of the span");
        CHECK(refused(t, 2, 11), "... which a range across it meets");
        CHECK(!refused(t, 2, 4) && t.unit(t.plan(2, 4), 0).size == 9, "(segment 0 alone: a size the walk will not find)");
    }
    {   // ... BEHIND it
        Batch t = good;
        t.ends[r + 3] = 21;
        const ReadGridPlan g = t.plan(1, 5), w = good.plan(1, 5);
        CHECK(g.p.verdict == kReadGo && g.p.k0 == 0 && g.p.units == 2 && g.skip == w.skip && g.p.scratch == w.p.scratch && !refused(t, 1, 5), "a decreasing entry behind the span");
        CHECK(!refused(t, 17, 2) && t.unit(t.plan(17, 2), 0).size == 9, "(the segment in front of it: a size the walk will not find)");
    }
    {   // an entry of 2^64 - 1: its segment and every one behind it
        Batch t = good;
        t.ends[r + 1] = kSegmentEndSaturated;
        CHECK(!refused(t, 0, 2) && t.plan(0, 2).p.verdict == kReadGo, "the segment in front of a saturated entry");
        CHECK(refused(t, 5, 1) && refused(t, 3, 3), "the segment of a saturated entry");
        CHECK(refused(t, 9, 1), "the segment behind a saturated entry");
        for (uint64_t k = 1; k < 5; k++) t.ends[r + k] = kSegmentEndSaturated;  // (what tamp_batch_segment_ends makes of a size of 0xFFFFFFFF)
        CHECK(!refused(t, 0, 4) && refused(t, 0, 5) && refused(t, 4, 1) && refused(t, 1ull << 40, 1) && refused(t, ~0ull - 1, 9), "a stream saturated from its second segment on");
    }
    {   // a size of 2^32 - 1, and the largest one that is taken
        Batch t = good;
        for (uint64_t k = 1; k < 5; k++) t.ends[r + k] = good.ends[r + k] + 0xFFFFFFFFull - 4;
        CHECK(refused(t, 5, 1) && refused(t, 2, 4) && !refused(t, 2, 2), "a segment of 2^32 - 1 bytes");
        CHECK(!refused(t, 0xFFFFFFFFull + 4, 1) && t.plan(0xFFFFFFFFull + 4, 1).p.k0 == 2, "the segment behind it, from its table position");
        for (uint64_t k = 1; k < 5; k++) t.ends[r + k] -= 1;
        const ReadGridPlan g = t.plan(5, 1);
        CHECK(g.p.verdict == kReadGo && t.unit(g, 0).size == 0xFFFFFFFEu && t.unit(g, 0).u.need == 2, "a segment of 2^32 - 2 bytes");
    }
    {   // the budget, the window, the header, entries without a table -- as in the fixed form
        CHECK(good.plan(0, 20, 1, 200).p.verdict == kReadBadArgument && good.plan(0, 4, 1, 200).p.verdict == kReadGo, "a range that alone outgrows the budget");
        CHECK(read_grid_plan(good.in.data(), good.in_off.data(), good.in_len.data(), good.first.data(), good.off.data(), good.ends.data(), 3, 9, 1ull << 40, 1, 0, 1).p.verdict == kReadInvalidConf, "a window above the call's");
        CHECK(read_grid_plan(good.in.data(), good.in_off.data(), good.in_len.data(), good.first.data(), nullptr, good.ends.data(), 3, 15, 1ull << 40, 1, 0, 1).p.verdict == kReadBadIndex, "entries and no table to hold them");
        Batch t = good;
        t.in[t.in_off[1]] = 0x58;
        CHECK(t.plan(0, 1).p.verdict == kReadInvalidConf && t.plan(0, 1, 0).p.verdict == kReadGo, "no reset bit");
        Batch d = good;
        d.first[2] = 1;
        CHECK(d.plan(0, 1).p.verdict == kReadBadIndex, "rows of reset_first that decrease");
    }
}

// The running sum of tamp_batch_segment_ends: streams without entries, a saturated size, rows of reset_first that make no sense.
static void running_sum() {
    {
        const uint64_t first[6] = {0, 0, 3, 3, 3, 5};
        const uint32_t closed[5] = {5, 0, 0, 0xFFFFFFFFu, 1}, open[5] = {9, 2, 0, 7, 3};
        uint64_t ends[10];
        segment_ends_fill(first, closed, open, ends, 5);
        const uint64_t want[10] = {9, 5, 5, 5, 7, 0, 7, ~0ull, ~0ull, ~0ull};
        for (int p = 0; p < 10; p++) CHECK(ends[p] == want[p], "row %d: %llu", p, (ull)ends[p]);
        for (uint64_t p = 0; p < 10; p++) CHECK(segment_end_owner(first, 5, p) == (p < 1 ? 0u : p < 5 ? 1u : p < 6 ? 2u : p < 7 ? 3u : 4u), "the owner of row %llu", (ull)p);
        segment_ends_fill(first, closed, open, ends, 0);  // (no streams: nothing is read)
    }
    {   // the operator: associative over every cut of a sequence with heads and a saturated term
        const SegmentEndSum seq[7] = {{3, 1}, {4, 0}, {kSegmentEndSaturated, 0}, {2, 0}, {5, 1}, {0, 0}, {6, 0}};
        SegmentEndSum left = segment_end_identity();
        for (int a = 0; a < 7; a++) left = segment_end_combine(left, seq[a]);
        for (int cut = 0; cut <= 7; cut++) {
            SegmentEndSum x = segment_end_identity(), y = segment_end_identity();
            for (int a = 0; a < cut; a++) x = segment_end_combine(x, seq[a]);
            for (int a = cut; a < 7; a++) y = segment_end_combine(y, seq[a]);
            const SegmentEndSum z = segment_end_combine(x, y);
            CHECK(z.v == left.v && z.head == left.head && z.v == 11, "cut %d: %llu", cut, (ull)z.v);
        }
        CHECK(segment_end_add(kSegmentEndSaturated, 5) == kSegmentEndSaturated && segment_end_add(5, kSegmentEndSaturated) == kSegmentEndSaturated && segment_end_add(2, 3) == 5, "the sum");
    }
    {   // rows of reset_first that are no running sum add nothing, and nothing is read outside the tables
        const uint64_t first[4] = {0, 3, 1, 2};
        const uint32_t closed[2] = {5, 6}, open[3] = {1, 2, 3};
        uint64_t ends[5];
        segment_ends_fill(first, closed, open, ends, 3);
        checked++;
    }
}

int main() {
    const uint32_t sizes[4] = {0, 1, 4, 7};
    for (uint32_t K : {1u, 2u, 3u, 5u}) {
        uint32_t combos = 1;
        for (uint32_t k = 0; k < K; k++) combos *= 4;
        for (uint32_t c = 0; c < combos; c++) {  // every choice of sizes: empty segments in a row, in front, open
            std::vector<uint32_t> size(K);
            for (uint32_t k = 0, r = c; k < K; k++, r /= 4) size[k] = sizes[r % 4];
            stream(size);
        }
    }
    for (uint32_t K : {1u, 2u, 3u, 5u})
        for (uint32_t N : {1u, 4u, 7u})
            for (uint32_t open : {1u, N}) against_fixed(K, N, open);
    bad_tables();
    running_sum();
    printf("%s: %ld streams, %ld ranges, %d failures\n", failures ? "FAILED" : "ok", streams, checked, failures);
    return failures ? 1 : 0;
}
""".replace("__VA_ARGUMENTS__", "__VA_ARGS__")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("read_ranges_grid")
    (d / "grid.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), str(d / "grid.cpp"), "-o", str(d / "grid")]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizers' runtimes)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "grid"), sanitized


def test_table_arithmetic(program):
    """Every stream of K in {1, 2, 3, 5} segments with sizes drawn from {0, 1, 4, 7} -- all choices, so two and three empty segments
    in a row, an empty first and an empty open segment are among them -- between two other streams, every range with begin and len
    <= total + 2 and begins and lengths around 2^32 and 2^64: first segment, unit count, each unit's cut, size, need, place and room,
    the gather offset and the bytes delivered against a plain walk; equal sizes against the fixed form; hand-made bad tables; the
    running sum of the ends call."""
    exe, sanitized = program
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr, "(host ASan + UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    m = re.match(r"ok: (\d+) streams, (\d+) ranges, 0 failures", p.stdout)
    assert m and int(m[1]) == 4 + 16 + 64 + 1024 and int(m[2]) > 500000, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
