"""CPU tier: the reset index of a batch (tamp_batch_compress_resets_index) and the batch decode that takes it as a hint
(tamp_batch_decompress_resets) as far as no device is needed -- the two symbols and their bindings, the keyword refusals of
``compress_batch`` / ``decompress_batch``, what the two C calls refuse before they look for a device, and the index arithmetic of
tamp_reset_segments.hpp compiled for the HOST into a stand-alone program with the address and undefined-behaviour sanitizers when
the compiler has their runtimes (nothing loaded into python is sanitised)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tamp_batch_compress_resets_index": 18, "tamp_batch_decompress_resets": 16}  # name -> arguments
BAD_ARGUMENT = -21


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


@pytest.mark.parametrize("name", list(NAMES))
def test_symbol_and_binding(lib, name):
    from tamp_amd import _lib

    header = open(os.path.join(ROOT, "include", "tamp_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\b%s\s*\(" % name, code)
    assert name in _lib.SYMBOLS and hasattr(C.CDLL(_lib.LIB_PATH), name)
    fn = getattr(lib, name)
    assert len(fn.argtypes) == NAMES[name] and fn.restype is C.c_int
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T %s$" % name, out, flags=re.M)


def test_python_names():
    import tamp
    import tamp_amd

    for pkg in (tamp_amd, tamp):
        assert "ResetIndex" in pkg.__all__ and pkg.ResetIndex is tamp_amd.ResetIndex
    idx = tamp_amd.ResetIndex(np.zeros(3, np.uint64), np.zeros(0, np.uint32))
    assert len(idx.first) == 3 and len(idx.off) == 0
    # a new LAST field with a default: positional constructions keep working
    res = tamp_amd.BatchResult(None, None, None, None)
    assert res.reset_index is None
    import dataclasses

    assert [f.name for f in dataclasses.fields(tamp_amd.BatchResult)][-1] == "reset_index"


def test_keyword_refusals_come_before_the_library(monkeypatch):
    """Every refusal is a ValueError raised before the native library is looked for."""
    import tamp_amd
    from tamp_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded before the keywords were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    data = [b"abc", b"defg"]
    for kwargs in ({}, dict(dictionary_reset=True), dict(dictionary_reset=False)):
        with pytest.raises(ValueError, match="reset_index needs reset_interval"):
            tamp_amd.compress_batch(data, reset_index=True, **kwargs)
    idx = tamp_amd.ResetIndex(np.zeros(3, np.uint64), np.zeros(0, np.uint32))
    dicts = [bytes(1024), bytes(1024)]
    for kwargs in (dict(dictionary=bytes(1024)), dict(dictionaries=dicts, dictionary_index=[0, 1]), dict(dictionaries=dicts),
                   dict(dictionary_index=[0, 1]), dict(dictionary=tamp_amd.DictionaryTable(dicts, [0, 1]))):
        with pytest.raises(ValueError, match="reset_index excludes dictionaries"):
            tamp_amd.decompress_batch(data, reset_index=idx, **kwargs)
    for entries in (0, 2, 4):
        bad = tamp_amd.ResetIndex(np.zeros(entries, np.uint64), np.zeros(0, np.uint32))
        with pytest.raises(ValueError, match="one entry per stream and one more"):
            tamp_amd.decompress_batch(data, reset_index=bad)
        flat, in_off, in_len = tamp_amd.pack_streams(data)
        with pytest.raises(ValueError, match="one entry per stream and one more"):
            tamp_amd.decompress_batch(flat, in_off, in_len, reset_index=bad, out_cap=16)
    with pytest.raises(ValueError, match="a ResetIndex expected"):
        tamp_amd.decompress_batch(data, reset_index=(np.zeros(3, np.uint64), np.zeros(0, np.uint32)))


def _arrays():
    a = dict(data=np.array([0x59, 0, 0, 0], dtype=np.uint8), in_off=np.zeros(1, np.uint64), in_len=np.full(1, 4, np.uint32),
             out=np.zeros(64, np.uint8), out_off=np.zeros(1, np.uint64), out_cap=np.full(1, 64, np.uint32),
             out_len=np.zeros(1, np.uint32), status=np.zeros(1, np.int8), consumed=np.zeros(1, np.uint32),
             reset_first=np.zeros(2, np.uint64), reset_off=np.zeros(4, np.uint32))
    return a, {k: v.ctypes.data_as(C.c_void_p) for k, v in a.items()}


def _compress_index(lib, conf, p, n, mem, dev):
    return lib.tamp_batch_compress_resets_index(C.byref(conf), p["data"], p["in_off"], p["in_len"], 16, p["out"], p["out_off"], p["out_cap"],
                                                p["out_len"], p["status"], n, 0, mem, dev, None, p["reset_first"], p["reset_off"], 4)


def _decompress_resets(lib, conf, p, n, mem, dev):
    return lib.tamp_batch_decompress_resets(15, p["data"], p["in_off"], p["in_len"], p["reset_first"], p["reset_off"], p["out"],
                                            p["out_off"], p["out_cap"], p["out_len"], p["status"], p["consumed"], n, mem, dev, None)


SLABS = ("in_off", "in_len", "out_off", "out_cap", "out_len", "status")
CALLS = {
    "tamp_batch_compress_resets_index": (SLABS, _compress_index),
    "tamp_batch_decompress_resets": (SLABS + ("reset_first",), _decompress_resets),
}


def _call(lib, name, *, missing=(), n=1, mem=None, device=0):
    from tamp_amd import _lib

    held, p = _arrays()
    for k in missing:
        p[k] = None
    conf = _lib.TampAmdConf(10, 8, 0, 1, 1, 0, 0, 0)
    rc = CALLS[name][1](lib, conf, p, n, _lib.MEM_HOST if mem is None else mem, device)
    del held
    return rc


@pytest.mark.parametrize("name", list(CALLS))
def test_each_required_table_null_in_turn(lib, name):
    for table in CALLS[name][0]:
        assert _call(lib, name, missing=(table,)) == BAD_ARGUMENT, table
        if "decompress" in name:  # (in_consumed may be null: the refusal is the table's)
            assert _call(lib, name, missing=(table, "consumed")) == BAD_ARGUMENT, table


@pytest.mark.parametrize("name", list(CALLS))
def test_memory_kind_all_devices_and_stream_count(lib, name):
    from tamp_amd import _lib

    assert _call(lib, name, mem=2) == BAD_ARGUMENT
    assert _call(lib, name, mem=-1) == BAD_ARGUMENT
    assert _call(lib, name, device=_lib.ALL_DEVICES) == BAD_ARGUMENT
    assert _call(lib, name, mem=_lib.MEM_DEVICE, device=_lib.ALL_DEVICES) == BAD_ARGUMENT
    assert _call(lib, name, mem=7, device=_lib.ALL_DEVICES) == BAD_ARGUMENT
    assert _call(lib, name, n=1 << 32) == BAD_ARGUMENT
    assert _call(lib, name, n=1 << 32, mem=_lib.MEM_DEVICE) == BAD_ARGUMENT


def test_more_refusals_and_no_streams(lib):
    from tamp_amd import _lib

    held, p = _arrays()
    conf = _lib.TampAmdConf(10, 8, 0, 1, 1, 0, 0, 0)
    args = (p["data"], p["in_off"], p["in_len"], 16, p["out"], p["out_off"], p["out_cap"], p["out_len"], p["status"])
    # a null conf; room for entries and nowhere to put them; the sizes-only form of the decode still needs the limits
    assert lib.tamp_batch_compress_resets_index(None, *args, 1, 0, _lib.MEM_HOST, 0, None, p["reset_first"], p["reset_off"], 4) == BAD_ARGUMENT
    assert lib.tamp_batch_compress_resets_index(C.byref(conf), *args, 1, 0, _lib.MEM_HOST, 0, None, p["reset_first"], None, 4) == BAD_ARGUMENT
    assert lib.tamp_batch_decompress_resets(15, p["data"], p["in_off"], p["in_len"], p["reset_first"], p["reset_off"], None, None, None,
                                            p["out_len"], p["status"], None, 1, _lib.MEM_HOST, 0, None) == BAD_ARGUMENT
    # no streams: nothing is refused and nothing is read (TAMP_OK; TAMP_AMD_NO_DEVICE on a machine without one)
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        assert lib.tamp_batch_compress_resets_index(C.byref(conf), *([None] * 3), 16, *([None] * 5), 0, 0, mem, 0, None, None, None, 0) in (0, -20)
        assert lib.tamp_batch_decompress_resets(15, *([None] * 11), 0, mem, 0, None) in (0, -20)
    del held


PROGRAM = r"""
#include "tamp_reset_segments.hpp"
#include <cstdio>
#include <vector>
using namespace tamp_amd;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// One batch with K[i] segments per stream and a verdict per stream: the tables built the way the kernels build them (reset_first as a
// running sum, the scan of the closed rows' sizes, the scan that places the split streams in the stage), every row's unit against a
// plain walk over streams and segments.
static long batch(const std::vector<uint32_t>& K, unsigned verdicts) {
    const uint64_t n = K.size();
    std::vector<uint64_t> first(n + 1);  // (sized exactly: an entry behind a table is an address error)
    std::vector<uint32_t> in_len(n);
    std::vector<std::vector<uint32_t>> seg_len(n), seg_size(n);
    for (uint64_t i = 0, run = 0; i < n; i++) {
        first[i] = run, run += K[i] - 1, first[i + 1] = run;
        uint32_t len = kResetHeaderBytes;
        for (uint32_t j = 0; j < K[i]; j++) {
            seg_len[i].push_back(j + 1 == K[i] ? (i + j) % 3 : 2 + (3 * i + j) % 5);  // (the last segment may be empty)
            seg_size[i].push_back(7 * (uint32_t)i + 11 * j + (j & 1 ? 0 : 300));
            len += seg_len[i][j];
        }
        in_len[i] = len;
    }
    const uint64_t C = first[n];
    std::vector<uint32_t> off(C), size(C + n);
    for (uint64_t i = 0; i < n; i++) {
        uint32_t at = kResetHeaderBytes;
        for (uint32_t j = 0; j + 1 < K[i]; j++) at += seg_len[i][j], off[first[i] + j] = at, size[first[i] + j] = seg_size[i][j];
        size[C + i] = seg_size[i][K[i] - 1];
    }
    std::vector<uint64_t> size_scan(C + 1), stage_base(n);
    for (uint64_t c = 0, run = 0; c <= C; c++) { size_scan[c] = run; if (c < C) run += size[c]; }
    std::vector<uint8_t> split(n);
    uint64_t staged = 0, units = 0;
    for (uint64_t i = 0; i < n; i++) {
        CHECK(reset_first_in_order(first.data(), i), "order of stream %llu", (unsigned long long)i);
        const uint64_t E = reset_index_entries(first.data(), n, i);
        CHECK(E == K[i] - 1, "entries of stream %llu", (unsigned long long)i);
        split[i] = E && ((verdicts >> i) & 1);
        stage_base[i] = staged;
        if (split[i]) staged += reset_staged_bytes(in_len[i], E), units += E + 1;
    }
    // every row against the walk
    std::vector<uint8_t> staged_once(staged, 0);
    uint64_t seen_units = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t start = kResetHeaderBytes;
        uint64_t out = 0, stage = stage_base[i];
        for (uint32_t j = 0; j < K[i]; j++) {
            const bool open = j + 1 == K[i];
            const uint64_t r = open ? C + i : first[i] + j;
            const ResetIndexCut u = open ? reset_index_open_cut(first.data(), off.data(), in_len.data(), n, i)
                                         : reset_index_closed_cut(first.data(), off.data(), in_len.data(), n, r);
            if (K[i] == 1) {
                CHECK(u.stream == kResetNoOwner, "a stream without entries claims no row");
                continue;
            }
            CHECK(u.stream == i && u.seg == j && u.start == start && u.end == start + seg_len[i][j], "row %llu: stream %u segment %u cut %u..%u",
                  (unsigned long long)r, u.stream, u.seg, u.start, u.end);
            if (u.stream != i) continue;
            if (split[i]) {
                CHECK(reset_unit_stage_off(stage_base[i], u) == stage, "stage offset of row %llu", (unsigned long long)r);
                CHECK(reset_unit_out_off(first.data(), size_scan.data(), u) == out, "output offset of row %llu", (unsigned long long)r);
                const uint64_t at = reset_unit_stage_off(stage_base[i], u), len = (uint64_t)(u.end - u.start) + kResetHeaderBytes;
                CHECK(at + len <= staged, "row %llu staged inside the stage", (unsigned long long)r);
                for (uint64_t b = at; b < at + len && b < staged; b++) staged_once[b]++;
                seen_units++;
            }
            start += seg_len[i][j], out += size[r], stage += seg_len[i][j] + kResetHeaderBytes;
        }
        if (split[i]) CHECK(stage == stage_base[i] + reset_staged_bytes(in_len[i], K[i] - 1), "staged bytes of stream %llu", (unsigned long long)i);
    }
    CHECK(seen_units == units, "%llu units", (unsigned long long)seen_units);
    for (uint64_t b = 0; b < staged; b++) CHECK(staged_once[b] == 1, "stage byte %llu written %u times", (unsigned long long)b, staged_once[b]);
    return 1;
}

// Hand-made rows that must be refused: the range and order check of the entries, and tables that are no running sum.
static void bad_rows() {
    const uint32_t in_len[2] = {40, 30};
    {   // one good batch to start from: stream 0 with entries 10, 20, 40 (the last: the stream ends with a reset), stream 1 with 5
        const uint64_t first[3] = {0, 3, 4};
        const uint32_t off[4] = {10, 20, 40, 5};
        for (uint64_t c = 0; c < 4; c++) CHECK(reset_index_closed_cut(first, off, in_len, 2, c).stream == (c < 3 ? 0u : 1u), "good row %llu", (unsigned long long)c);
        const ResetIndexCut o0 = reset_index_open_cut(first, off, in_len, 2, 0), o1 = reset_index_open_cut(first, off, in_len, 2, 1);
        CHECK(o0.stream == 0 && o0.seg == 3 && o0.start == 40 && o0.end == 40, "an empty open segment");
        CHECK(o1.stream == 1 && o1.seg == 1 && o1.start == 5 && o1.end == 30, "open segment of stream 1");
    }
    const uint64_t first[3] = {0, 3, 4};
    struct { uint32_t off[4]; int bad_closed[4]; int bad_open[2]; const char* what; } rows[] = {
        {{10, 10, 40, 5}, {0, 1, 0, 0}, {0, 0}, "two equal entries"},
        {{20, 10, 40, 5}, {0, 1, 0, 0}, {0, 0}, "entries out of order"},
        {{10, 20, 41, 5}, {0, 0, 1, 0}, {1, 0}, "an entry beyond in_len"},
        {{2, 20, 40, 5}, {1, 0, 0, 0}, {0, 0}, "an entry at the header's end: an empty first segment"},
        {{1, 20, 40, 5}, {1, 1, 0, 0}, {0, 0}, "an entry inside the header (and the row that starts there)"},
        {{0, 20, 40, 5}, {1, 1, 0, 0}, {0, 0}, "an entry of zero (and the row that starts there)"},
        {{10, 20, 40, 1}, {0, 0, 0, 1}, {0, 1}, "stream 1: inside the header"},
        {{10, 20, 40, 31}, {0, 0, 0, 1}, {0, 1}, "stream 1: beyond in_len"},
        {{10, 20, 0xFFFFFFFFu, 5}, {0, 0, 1, 0}, {1, 0}, "the largest value"},
    };
    for (const auto& row : rows) {
        for (uint64_t c = 0; c < 4; c++)
            CHECK((reset_index_closed_cut(first, row.off, in_len, 2, c).stream == kResetNoOwner) == (row.bad_closed[c] != 0), "%s: closed row %llu", row.what, (unsigned long long)c);
        for (uint64_t i = 0; i < 2; i++)
            CHECK((reset_index_open_cut(first, row.off, in_len, 2, i).stream == kResetNoOwner) == (row.bad_open[i] != 0), "%s: open row %llu", row.what, (unsigned long long)i);
    }
    {   // tables that are no running sum from 0
        const uint32_t off[6] = {10, 20, 25, 5, 6, 7};
        const uint64_t down[3] = {0, 3, 2}, up[3] = {1, 3, 4}, over[3] = {0, 5, 4};
        CHECK(reset_first_in_order(down, 0) && !reset_first_in_order(down, 1), "a table that decreases");
        CHECK(!reset_first_in_order(up, 0) && reset_first_in_order(up, 1), "a table that does not start at 0");
        CHECK(reset_index_entries(down, 2, 0) == 0 && reset_index_entries(down, 2, 1) == 0, "entries of a decreasing table");
        CHECK(reset_index_entries(over, 2, 0) == 0, "entries beyond the table's last");
        CHECK(reset_index_open_cut(down, off, in_len, 2, 1).stream == kResetNoOwner, "open row of a decreasing table");
        for (uint64_t c = 0; c < 2; c++) CHECK(reset_index_closed_cut(down, off, in_len, 2, c).stream == kResetNoOwner, "closed row %llu of a decreasing table", (unsigned long long)c);
    }
}

int main() {
    long batches = 0;
    const uint32_t Ks[4] = {1, 2, 3, 5};
    for (int n = 1; n <= 4; n++) {
        int total = 1;
        for (int j = 0; j < n; j++) total *= 4;
        for (int code = 0; code < total; code++) {
            std::vector<uint32_t> K(n);
            for (int j = 0, c = code; j < n; j++, c /= 4) K[j] = Ks[c % 4];
            for (unsigned verdicts = 0; verdicts < (1u << n); verdicts++) batches += batch(K, verdicts);
        }
    }
    bad_rows();
    static_assert(reset_staged_bytes(2, 1) == 4 && reset_staged_bytes(100, 3) == 98 + 8, "staged bytes");
    printf("%s: %ld batches, %d failures\n", failures ? "FAILED" : "ok", batches, failures);
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("batch_reset_index")
    (d / "index.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), str(d / "index.cpp"), "-o", str(d / "index")]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizers' runtimes)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "index"), sanitized


def test_index_arithmetic(program):
    """Every batch of up to 4 streams with K_i in {1, 2, 3, 5} and every verdict pattern: the unit count, each unit's owner, segment
    number, input cut, place in the stage and output offset against a plain walk; the staged units tile the stage exactly; and the
    range and order check of the entries on hand-made bad rows."""
    exe, sanitized = program
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr, "(host ASan + UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    m = re.match(r"ok: (\d+) batches, 0 failures", p.stdout)
    assert m and int(m[1]) == 4 * 2 + 16 * 4 + 64 * 8 + 256 * 16, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
