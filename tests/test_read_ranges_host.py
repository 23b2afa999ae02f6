"""CPU tier: reading byte ranges of reset-segmented streams (tamp_batch_read_ranges, ``read_ranges``) as far as no device is
needed -- the symbol and its binding, the Python names, the keyword refusals of ``read_ranges``, what the C call refuses before it
looks for a device, and the range arithmetic of tamp_reset_segments.hpp compiled for the HOST into a stand-alone program with the
address and undefined-behaviour sanitizers when the compiler has their runtimes (nothing loaded into python is sanitised)."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARGUMENTS = "tamp_batch_read_ranges", 19
BAD_ARGUMENT, BAD_INDEX = -21, -22


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
    assert re.search(r"\b%s\s*\(" % NAME, code)
    m = re.search(r"TAMP_AMD_BAD_INDEX\s*=\s*(-?\d+)", code)
    assert m and int(m[1]) == BAD_INDEX == _lib.BAD_INDEX
    assert code.index("TAMP_AMD_BAD_ARGUMENT") < code.index("TAMP_AMD_BAD_INDEX")
    assert NAME in _lib.SYMBOLS and hasattr(C.CDLL(_lib.LIB_PATH), NAME)
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == ARGUMENTS and fn.restype is C.c_int
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T %s$" % NAME, out, flags=re.M)
    with pytest.raises(ValueError, match="reset index"):
        _lib.check_launch(BAD_INDEX)


def test_python_names():
    import tamp
    import tamp_amd

    for pkg in (tamp_amd, tamp):
        for name in ("read_ranges", "RangeResult"):
            assert name in pkg.__all__ and getattr(pkg, name) is getattr(tamp_amd, name)
    idx = tamp_amd.ResetIndex(np.zeros(3, np.uint64), np.zeros(0, np.uint32))
    assert len(idx.first) == 3 and len(idx.off) == 0 and idx.interval is None
    assert [f.name for f in dataclasses.fields(tamp_amd.ResetIndex)][-1] == "interval"
    assert tamp_amd.ResetIndex(idx.first, idx.off, 64).interval == 64
    assert [f.name for f in dataclasses.fields(tamp_amd.BatchResult)][-1] == "reset_index"
    r = tamp_amd.RangeResult(np.arange(6, dtype=np.uint8), np.array([0, 4], np.uint64), np.array([3, 2], np.uint32), np.zeros(2, np.int8))
    assert r.range(0) == bytes([0, 1, 2]) and r.ranges() == [bytes([0, 1, 2]), bytes([4, 5])] and r.kernel_ms == -1.0


def test_keyword_refusals_come_before_the_library(monkeypatch):
    """Every refusal is a ValueError raised before the native library is looked for."""
    import tamp_amd
    from tamp_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded before the keywords were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    data = [b"abc", b"defg"]
    flat, in_off, in_len = tamp_amd.pack_streams(data)
    idx = tamp_amd.ResetIndex(np.zeros(3, np.uint64), np.zeros(0, np.uint32), 16)
    good = dict(reset_index=idx, stream_index=[0, 1], begin=[0, 0], length=[1, 1])

    def refused(match, **change):
        for args in ((data,), (flat, in_off, in_len)):
            with pytest.raises(ValueError, match=match):
                tamp_amd.read_ranges(*args, **{**good, **change})

    refused("a ResetIndex expected", reset_index=(idx.first, idx.off))
    refused("a ResetIndex expected", reset_index=None)
    for entries in (0, 2, 4):
        refused("one entry per stream and one more", reset_index=tamp_amd.ResetIndex(np.zeros(entries, np.uint64), idx.off, 16))
    refused("one entry per range each", stream_index=[0])
    refused("one entry per range each", begin=[0, 0, 0])
    refused("one entry per range each", length=np.zeros(1, np.uint32))
    refused("not given and not in the index", reset_index=tamp_amd.ResetIndex(idx.first, idx.off))
    for bad in (0, -1, 1 << 32, 1.5, "16", True):
        refused("a positive integer that fits 32 bits", reset_interval=bad)
        refused("a positive integer that fits 32 bits", reset_index=tamp_amd.ResetIndex(idx.first, idx.off, bad))
    refused("begin: negative", begin=[0, -1])
    refused("begin: negative", begin=np.array([-5, 0], np.int64))
    refused("length: does not fit 32 bits", length=[1, 1 << 32])
    refused("length: does not fit 32 bits", length=[-1, 1])
    # the interval of the call goes before the index's; what is fine gets as far as the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        tamp_amd.read_ranges(data, **{**good, "reset_index": tamp_amd.ResetIndex(idx.first, idx.off, 0), "reset_interval": 16})
    with pytest.raises(AssertionError, match="the library was loaded"):
        tamp_amd.read_ranges(data, **{**good, "begin": [0, (1 << 64) - 1], "length": [0, (1 << 32) - 1]})


TABLES = ("in_off", "in_len", "reset_first", "range_stream", "range_begin", "range_len", "out_off", "out_len", "status")


def _arrays():
    a = dict(data=np.array([0x59, 0, 0, 0], dtype=np.uint8), in_off=np.zeros(1, np.uint64), in_len=np.full(1, 4, np.uint32),
             reset_first=np.zeros(2, np.uint64), reset_off=np.zeros(4, np.uint32), range_stream=np.zeros(1, np.uint32),
             range_begin=np.zeros(1, np.uint64), range_len=np.full(1, 8, np.uint32), out=np.zeros(64, np.uint8),
             out_off=np.zeros(1, np.uint64), out_len=np.zeros(1, np.uint32), status=np.zeros(1, np.int8))
    return a, {k: v.ctypes.data_as(C.c_void_p) for k, v in a.items()}


def _call(lib, *, missing=(), n=1, n_ranges=1, interval=16, mem=None, device=0):
    from tamp_amd import _lib

    held, p = _arrays()
    for k in missing:
        p[k] = None
    rc = lib.tamp_batch_read_ranges(15, p["data"], p["in_off"], p["in_len"], p["reset_first"], p["reset_off"], interval, p["range_stream"],
                                    p["range_begin"], p["range_len"], p["out"], p["out_off"], p["out_len"], p["status"], n, n_ranges,
                                    _lib.MEM_HOST if mem is None else mem, device, None)
    del held
    return rc


def test_call_level_refusals(lib):
    """Before a device is looked for: TAMP_AMD_BAD_ARGUMENT on a machine with and without one, for both memory kinds."""
    from tamp_amd import _lib

    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        for table in TABLES:
            assert _call(lib, missing=(table,), mem=mem) == BAD_ARGUMENT, table
            assert _call(lib, missing=(table,), mem=mem, n_ranges=0) == BAD_ARGUMENT, table
            assert _call(lib, missing=(table, "reset_off"), mem=mem) == BAD_ARGUMENT, table
        assert _call(lib, missing=("data",), mem=mem) == BAD_ARGUMENT
        assert _call(lib, missing=("out",), mem=mem) == BAD_ARGUMENT
        assert _call(lib, interval=0, mem=mem) == BAD_ARGUMENT
        assert _call(lib, device=_lib.ALL_DEVICES, mem=mem) == BAD_ARGUMENT
        assert _call(lib, n=1 << 32, mem=mem) == BAD_ARGUMENT
        assert _call(lib, n_ranges=1 << 32, mem=mem) == BAD_ARGUMENT
    for mem in (2, -1, 7):
        assert _call(lib, mem=mem) == BAD_ARGUMENT
        assert _call(lib, mem=mem, device=_lib.ALL_DEVICES) == BAD_ARGUMENT


def test_no_ranges(lib):
    """n_ranges == 0: nothing is refused that the tables do not refuse, nothing is touched (TAMP_OK; TAMP_AMD_NO_DEVICE is allowed on a
    machine without a device)."""
    from tamp_amd import _lib

    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        assert _call(lib, n_ranges=0, mem=mem) in (0, -20)
        assert _call(lib, n_ranges=0, n=0, missing=("data", "out", "reset_off"), mem=mem) in (0, -20)


PROGRAM = r"""
#include "tamp_reset_segments.hpp"
#include <cstdio>
#include <vector>
using namespace tamp_amd;

static int failures = 0;
static long checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)
typedef unsigned long long ull;

// One stream of K segments -- K - 1 closed ones of N decoded bytes, the open one of `open` -- among two others, tables sized exactly
// (an entry read behind a table is an address error): every range of it against a plain walk over its segments.
static void stream(uint32_t K, uint32_t N, uint32_t open) {
    const uint64_t n = 3, i = 1, E = K - 1;
    std::vector<uint64_t> first = {0, 2, 2 + E, 3 + E};
    std::vector<uint32_t> off(3 + E), in_len = {30, 0, 9};
    off[0] = 7, off[1] = 19, off[2 + E] = 5;
    std::vector<uint32_t> clen(K);
    uint32_t at = kResetHeaderBytes;
    for (uint32_t k = 0; k < K; k++) {
        clen[k] = k < E ? 3 + (k * 5 + N) % 4 : (open ? 1 + open % 3 : 0);  // (compressed bytes; the open segment may be empty)
        at += clen[k];
        if (k < E) off[2 + k] = at;
    }
    in_len[i] = at;
    std::vector<uint64_t> in_off = {0, 30, 30 + (uint64_t)at};
    std::vector<uint8_t> in(30 + at + 9, 0xCC);
    for (uint64_t s = 0; s < n; s++) in[in_off[s]] = 0x59, in[in_off[s] + 1] = 0;  // window 10, literal 8, the reset bit
    const uint64_t total = (uint64_t)E * N + open, budget = 1ull << 40;
    std::vector<uint64_t> begins, lens;
    for (uint64_t b = 0; b <= (uint64_t)K * N + 2; b++) begins.push_back(b);
    for (uint64_t l = 0; l <= 3ull * N + 2; l++) lens.push_back(l);
    for (uint64_t big : {(1ull << 32) - 2, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 1, (1ull << 40) - 1, 1ull << 40, (1ull << 40) + 1, ~0ull - 1, ~0ull}) {
        begins.push_back(big);
        if (big <= 0xFFFFFFFFull) lens.push_back(big);
    }
    for (uint64_t begin : begins)
        for (uint64_t len64 : lens) {
            const uint32_t len = (uint32_t)len64;
            const ReadPlan p = read_range_plan(in.data(), in_off.data(), in_len.data(), first.data(), off.data(), n, N, 15, budget, (uint32_t)i, begin, len);
            checked++;
            if (len == 0) {
                CHECK(p.verdict == kReadOk && p.units == 0, "an empty range");
                continue;
            }
            // the walk: segment k stands for the decoded bytes [k N, (k + 1) N), whatever the open one holds of them
            const uint64_t end = begin + len < begin ? ~0ull : begin + len;  // (exclusive; saturated, as the last byte asked for is)
            uint64_t seg_start = 0, units = 0, k0 = 0, scratch = 0, staged = 0;
            uint32_t cut = kResetHeaderBytes;
            std::vector<uint32_t> want_start, want_end, want_need;
            std::vector<uint64_t> want_room;
            for (uint32_t k = 0; k < K; k++) {
                const bool touched = begin - seg_start < N && begin >= seg_start ? true : (seg_start > begin && seg_start < end);
                if (touched) {
                    if (!units) k0 = k;
                    const uint64_t left = end - seg_start;
                    want_start.push_back(cut), want_end.push_back(cut + clen[k]), want_need.push_back(left < N ? (uint32_t)left : N);
                    want_room.push_back(scratch);
                    scratch += want_need.back(), staged += clen[k] + kResetHeaderBytes, units++;
                }
                cut += clen[k], seg_start += N;
            }
            if (!units) {
                CHECK(p.verdict == kReadInputExhausted && p.units == 0, "begin %llu len %u: behind the last segment", (ull)begin, len);
                continue;
            }
            CHECK(p.verdict == kReadGo && p.k0 == k0 && p.units == units, "begin %llu len %u: k0 %llu units %llu (want %llu, %llu)", (ull)begin, len,
                  (ull)p.k0, (ull)p.units, (ull)k0, (ull)units);
            if (p.verdict != kReadGo || p.units != units) continue;
            CHECK(p.scratch == scratch && p.staged == staged, "begin %llu len %u: scratch %llu staged %llu (want %llu, %llu)", (ull)begin, len,
                  (ull)p.scratch, (ull)p.staged, (ull)scratch, (ull)staged);
            CHECK(read_plan_cost(p) == scratch + staged + units * kReadUnitRow, "the cost");
            uint64_t place = 0, sum_need = 0, sum_staged = 0;
            for (uint64_t j = 0; j < units; j++) {
                const ReadUnit u = read_range_unit(first.data(), off.data(), in_len.data(), N, i, p, j);
                CHECK(u.cut.ok && u.cut.start == want_start[j] && u.cut.end == want_end[j] && u.cut.closed == (k0 + j < E), "begin %llu len %u unit %llu: cut %u..%u",
                      (ull)begin, len, (ull)j, u.cut.start, u.cut.end);
                CHECK(u.need == want_need[j] && u.room == want_room[j] && (j + 1 == units || u.need == N), "begin %llu len %u unit %llu: need %u room %llu", (ull)begin, len,
                      (ull)j, u.need, (ull)u.room);
                CHECK(u.place == place && u.in_len == want_end[j] - want_start[j] + kResetHeaderBytes, "begin %llu len %u unit %llu: place %llu", (ull)begin, len, (ull)j, (ull)u.place);
                place += u.in_len, sum_need += u.need, sum_staged += u.in_len;
            }
            CHECK(sum_need == p.scratch && sum_staged == p.staged, "the totals against the sum over the units");
            // what is delivered when every unit decodes to min(its size, need): byte by byte where the range is small
            uint64_t decoded = 0;
            for (uint64_t j = 0; j < units; j++) {
                const uint64_t size = k0 + j < E ? N : open;
                decoded += size < want_need[j] ? size : want_need[j];
            }
            const uint64_t skip = read_range_skip(begin, p.k0, N);
            CHECK(skip == begin - k0 * N && skip < N, "the gather offset");
            uint64_t delivered = 0;
            if (len <= 64) { for (uint64_t b = begin; b - begin < len; b++) delivered += b < total; }
            else delivered = begin < total ? (total - begin < len ? total - begin : len) : 0;
            CHECK(read_range_delivered(decoded, skip, len) == delivered, "begin %llu len %u: delivered %u (want %llu)", (ull)begin, len,
                  read_range_delivered(decoded, skip, len), (ull)delivered);
        }
    // the other two streams are not disturbed by this one's entries
    CHECK(read_range_plan(in.data(), in_off.data(), in_len.data(), first.data(), off.data(), n, N, 15, budget, 0, 0, 1).staged == 7 - 2 + 2, "stream 0");
    CHECK(read_range_plan(in.data(), in_off.data(), in_len.data(), first.data(), off.data(), n, N, 15, budget, 2, N, 1).staged == 9 - 5 + 2, "stream 2");
}

static int verdict(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint64_t* first, const uint32_t* off, uint64_t n, uint32_t N,
                   uint32_t stream, uint64_t begin, uint32_t len, uint32_t max_wbits = 15, uint64_t budget = 1ull << 40) {
    return read_range_plan(in, in_off, in_len, first, off, n, N, max_wbits, budget, stream, begin, len).verdict;
}

// Hand-made tables that must be refused.
static void bad_tables() {
    uint8_t in[80];
    for (int b = 0; b < 80; b++) in[b] = 0xCC;
    in[0] = 0x59, in[1] = 0, in[40] = 0x59, in[41] = 0;
    const uint64_t in_off[2] = {0, 40};
    const uint32_t in_len[2] = {40, 30};
    const uint32_t N = 8;
    const uint64_t first[3] = {0, 3, 4};
    {   // the good tables to start from: stream 0 with entries 10, 20, 40 (it ends with a reset), stream 1 with 5
        const uint32_t off[4] = {10, 20, 40, 5};
        for (uint64_t k = 0; k < 4; k++) CHECK(verdict(in, in_off, in_len, first, off, 2, N, 0, k * N, N) == kReadGo, "good segment %llu", (ull)k);
        const ReadCut c = read_segment_cut(first, off, in_len, 0, 3);
        CHECK(c.ok && !c.closed && c.start == 40 && c.end == 40, "an empty open segment");
        CHECK(verdict(in, in_off, in_len, first, off, 2, N, 0, 4 * N, 1) == kReadInputExhausted, "behind the open segment");
        CHECK(verdict(in, in_off, in_len, first, off, 2, N, 2, 0, 1) == kReadBadArgument, "a stream there is none of");
        CHECK(verdict(in, in_off, in_len, first, off, 2, N, 2, 0, 0) == kReadBadArgument, "... which goes before the empty range");
        CHECK(verdict(in, in_off, in_len, first, off, 2, N, 1, 1ull << 50, 0) == kReadOk, "an empty range anywhere");
        CHECK(verdict(in, in_off, in_len, first, off, 2, N, 0, 0, 4 * N, 15, 200) == kReadBadArgument, "a range that alone outgrows the budget");
        CHECK(verdict(in, in_off, in_len, first, off, 2, N, 0, 0, N, 15, 200) == kReadGo, "... and one that does not");
        CHECK(verdict(in, in_off, in_len, first, nullptr, 2, N, 0, 0, 1) == kReadBadIndex, "entries and no table to hold them");
        CHECK(verdict(in, in_off, in_len, first, off, 2, N, 0, 0, 1, 9) == kReadInvalidConf, "a window above the call's");
        CHECK(verdict(in, in_off, in_len, first, off, 2, N, 0, 0, 1, 10) == kReadGo && verdict(in, in_off, in_len, first, off, 2, N, 0, 0, 1, 16) == kReadInvalidConf, "the window's limits");
    }
    for (int h = 0; h < 4; h++) {  // the header: no reset bit, the custom bit, a second byte that is not zero, a stream shorter than it
        uint8_t other[80];
        for (int b = 0; b < 80; b++) other[b] = in[b];
        uint32_t len2[2] = {40, 30};
        if (h == 0) other[0] = 0x58;
        if (h == 1) other[0] = 0x5D;
        if (h == 2) other[1] = 1;
        if (h == 3) len2[0] = 1;
        const uint32_t off[4] = {10, 20, 40, 5};
        CHECK(verdict(other, in_off, len2, first, off, 2, N, 0, 0, 1) == kReadInvalidConf, "header case %d", h);
        CHECK(verdict(other, in_off, len2, first, off, 2, N, 1, 0, 1) == kReadGo, "header case %d: the other stream", h);
    }
    struct { uint32_t off[4]; int bad[4]; const char* what; } rows[] = {   // bad[k]: a one-byte range in segment k of stream 0 is refused
        {{10, 10, 40, 5}, {0, 1, 0, 0}, "two equal entries"},
        {{20, 10, 40, 5}, {0, 1, 0, 0}, "entries out of order"},
        {{10, 20, 41, 5}, {0, 0, 1, 1}, "an entry beyond in_len"},
        {{2, 20, 40, 5}, {1, 0, 0, 0}, "an entry at the header's end: an empty first segment"},
        {{1, 20, 40, 5}, {1, 1, 0, 0}, "an entry inside the header (and the segment that starts there)"},
        {{0, 20, 40, 5}, {1, 1, 0, 0}, "an entry of zero (and the segment that starts there)"},
        {{10, 20, 0xFFFFFFFFu, 5}, {0, 0, 1, 1}, "the largest value"},
    };
    for (const auto& row : rows) {
        for (uint64_t k = 0; k < 4; k++) {
            CHECK((verdict(in, in_off, in_len, first, row.off, 2, N, 0, k * N + 3, 1) == kReadBadIndex) == (row.bad[k] != 0), "%s: segment %llu", row.what, (ull)k);
            CHECK(read_segment_cut(first, row.off, in_len, 0, k).ok == !row.bad[k], "%s: cut %llu", row.what, (ull)k);
        }
        CHECK(verdict(in, in_off, in_len, first, row.off, 2, N, 1, 0, 2 * N) == kReadGo, "%s: the other stream", row.what);
    }
    {   // a bad entry BETWEEN the first and the last touched segment: the range has units, the one with the bad cut says so -- and a
        // cut that leaves the range's span is refused although its own entries are in order
        const uint32_t off[4] = {30, 20, 40, 5};
        const ReadPlan p = read_range_plan(in, in_off, in_len, first, off, 2, N, 15, 1ull << 40, 0, 0, 4 * N);
        CHECK(p.verdict == kReadGo && p.units == 4, "the span of a range with a bad inner entry");
        int ok = 0;
        for (uint64_t j = 0; j < 4; j++) {
            const ReadUnit u = read_range_unit(first, off, in_len, N, 0, p, j);
            ok += u.cut.ok;
            if (u.cut.ok) CHECK(u.place + u.in_len <= p.staged, "unit %llu stays inside the range's stage", (ull)j);
            else CHECK(u.in_len == 0, "a unit without a cut has no bytes");
        }
        CHECK(ok == 3, "entries 30, 20: segment 1 is refused (%d hold up)", ok);
        const uint32_t in_len3[1] = {60};
        const uint64_t first3[2] = {0, 4};
        const uint32_t off3[4] = {20, 50, 10, 30};  // segments 20..50 and 10..30 hold up on their own; the span of segments 1..3 is 20..30
        const ReadPlan q = read_range_plan(in, in_off, in_len3, first3, off3, 1, N, 15, 1ull << 40, 0, N, 3 * N);
        CHECK(q.verdict == kReadGo && q.units == 3 && q.staged == 10 + 6, "a span between entries out of order");
        CHECK(read_segment_cut(first3, off3, in_len3, 0, 1).ok && read_segment_cut(first3, off3, in_len3, 0, 3).ok, "the two cuts on their own");
        for (uint64_t j = 0; j < 3; j++) CHECK(!read_range_unit(first3, off3, in_len3, N, 0, q, j).cut.ok, "cut %llu leaves the span (or is out of order)", (ull)j);
    }
    {   // E = 0: the whole stream is one open segment
        const uint64_t none[3] = {0, 0, 0};
        uint32_t len1[2] = {40, 30};
        ReadCut c = read_segment_cut(none, nullptr, len1, 0, 0);
        CHECK(c.ok && !c.closed && c.start == 2 && c.end == 40, "the cut of a stream without entries");
        CHECK(verdict(in, in_off, len1, none, nullptr, 2, N, 0, 3, 100) == kReadGo && verdict(in, in_off, len1, none, nullptr, 2, N, 0, N, 1) == kReadInputExhausted, "E = 0");
        len1[0] = 2;
        CHECK(read_segment_cut(none, nullptr, len1, 0, 0).ok && verdict(in, in_off, len1, none, nullptr, 2, N, 0, 0, 1) == kReadGo, "a header and nothing else");
        len1[0] = 1;
        CHECK(!read_segment_cut(none, nullptr, len1, 0, 0).ok, "E = 0 and a stream shorter than its header");
        len1[0] = 0;
        CHECK(!read_segment_cut(none, nullptr, len1, 0, 0).ok, "E = 0 and an empty stream");
        len1[0] = kResetHeaderBytes + kReadMaxSegment;
        CHECK(read_segment_cut(none, nullptr, len1, 0, 0).ok, "the longest segment the walk counts");
        len1[0] = kResetHeaderBytes + kReadMaxSegment + 1;
        CHECK(!read_segment_cut(none, nullptr, len1, 0, 0).ok, "a segment too long for 32-bit bit positions");
    }
    {   // tables that are no running sum from 0
        const uint32_t off[6] = {10, 20, 25, 5, 6, 7};
        const uint64_t down[3] = {0, 3, 2}, up[3] = {1, 3, 4}, over[3] = {0, 5, 4};
        CHECK(verdict(in, in_off, in_len, down, off, 2, N, 0, 0, 1) == kReadBadIndex && verdict(in, in_off, in_len, down, off, 2, N, 1, 0, 1) == kReadBadIndex, "a table that decreases");
        CHECK(verdict(in, in_off, in_len, up, off, 2, N, 0, 0, 1) == kReadBadIndex && verdict(in, in_off, in_len, up, off, 2, N, 1, 0, 1) == kReadGo, "a table that does not start at 0");
        CHECK(verdict(in, in_off, in_len, over, off, 2, N, 0, 0, 1) == kReadBadIndex, "entries beyond the table's last");
    }
}

int main() {
    const uint32_t Ks[4] = {1, 2, 3, 5}, Ns[3] = {1, 4, 7};
    long streams = 0;
    for (uint32_t K : Ks)
        for (uint32_t N : Ns) {
            std::vector<uint32_t> opens = {0, 1, N - 1, N};
            for (size_t a = 0; a < opens.size(); a++) {
                bool seen = false;
                for (size_t b = 0; b < a; b++) seen |= opens[b] == opens[a];
                if (!seen) stream(K, N, opens[a]), streams++;
            }
        }
    bad_tables();
    static_assert(read_range_delivered(10, 3, 4) == 4 && read_range_delivered(10, 3, 9) == 7 && read_range_delivered(3, 3, 9) == 0, "delivered");
    static_assert(read_sat_add(~0ull, 1) == ~0ull && read_sat_add(1, 2) == 3, "saturating sum");
    printf("%s: %ld streams, %ld ranges, %d failures\n", failures ? "FAILED" : "ok", streams, checked, failures);
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("read_ranges")
    (d / "ranges.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), str(d / "ranges.cpp"), "-o", str(d / "ranges")]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizers' runtimes)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "ranges"), sanitized


def test_range_arithmetic(program):
    """Every stream of K in {1, 2, 3, 5} segments of N in {1, 4, 7} bytes with an open segment of 0, 1, N - 1 or N bytes, every range
    with begin <= K N + 2 and len <= 3 N + 2 and begins and lengths around 2^32, 2^40 and 2^64: first segment, unit count, each unit's
    cut, need, place in the stage and in the scratch, the gather offset and the bytes delivered against a plain walk; the totals
    against the sums over the units; hand-made bad entries, also in the cut of a stream without entries."""
    exe, sanitized = program
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr, "(host ASan + UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    m = re.match(r"ok: (\d+) streams, (\d+) ranges, 0 failures", p.stdout)
    want = 0
    for K in (1, 2, 3, 5):
        for N in (1, 4, 7):
            want += len({0, 1, N - 1, N}) * (K * N + 3 + 9) * (3 * N + 3 + 2)
    assert m and int(m[1]) == 4 * (2 + 4 + 4) and int(m[2]) == want, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
