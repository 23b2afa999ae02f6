"""CPU tier: dictionary-reset segments for every stream of a batch (tamp_batch_compress_resets) as far as no device is needed -- the
symbol and its binding, the ``reset_interval`` keyword's refusals in ``compress_batch``, the Python bound against the library's, and
the stream / segment mapping of tamp_reset_segments.hpp compiled for the HOST into a stand-alone program with the address and
undefined-behaviour sanitizers when the compiler has their runtimes (nothing loaded into python is sanitised)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tamp_batch_compress_resets"


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
    assert NAME in _lib.SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == 15 and fn.restype is ctypes.c_int
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T %s$" % NAME, out, flags=re.M)


def test_keyword_refusals_come_before_the_library(monkeypatch):
    """Every refusal is a ValueError raised before the native library is looked for."""
    import tamp_amd
    from tamp_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded before the keywords were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    data = [b"abc", b"defg"]
    for bad in (0, -1, 1.5, "4096", True):
        with pytest.raises(ValueError, match="reset_interval must be a positive integer"):
            tamp_amd.compress_batch(data, dictionary_reset=True, reset_interval=bad)
    for kwargs in ({}, dict(dictionary_reset=False), dict(window=12)):
        with pytest.raises(ValueError, match="reset_interval needs dictionary_reset=True"):
            tamp_amd.compress_batch(data, reset_interval=4096, **kwargs)
    dicts = [bytes(1024), bytes(1024)]
    for kwargs in (dict(dictionary=bytes(1024)), dict(dictionaries=dicts, dictionary_index=[0, 1]), dict(dictionaries=dicts),
                   dict(dictionary_index=[0, 1]), dict(dictionary=tamp_amd.DictionaryTable(dicts, [0, 1])),
                   dict(reuse=tamp_amd.BatchResult(None, None, None, None))):
        with pytest.raises(ValueError, match="reset_interval excludes"):
            tamp_amd.compress_batch(data, dictionary_reset=True, reset_interval=16, **kwargs)
    with pytest.raises(ValueError):
        tamp_amd.compress_batch(data, dictionary_reset=True, reset_interval=1 << 32)
    with pytest.raises(ValueError):
        tamp_amd.compress_batch(data, dictionary_reset=True, reset_interval=16, window=16)
    with pytest.raises(ValueError):
        tamp_amd.compress_batch(data, dictionary_reset=True, reset_interval=16, literal=9)


def test_python_bound_is_the_librarys(lib):
    from tamp_amd import batch

    for interval in (1, 15, 16, 17, 1000, 65536):
        for literal in (5, 7, 8):
            lens = [0, 1, interval - 1, interval, interval + 1, 2 * interval, 2 * interval + 1, 40 * interval - 7, 4 << 20]
            want = [lib.tamp_amd_compress_resets_bound(n, interval, literal) for n in lens]
            assert [batch.compress_resets_bound(n, interval, literal) for n in lens] == want
            assert [int(x) for x in batch.compress_resets_bound(np.array(lens, dtype=np.uint32), interval, literal)] == want


PROGRAM = r"""
#include "tamp_reset_segments.hpp"
#include <cstdio>
#include <vector>
using namespace tamp_amd;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// One batch: the tables built the way the count kernel and the rows kernel build them, against a plain walk over streams and segments.
static void batch(const std::vector<uint32_t>& len, uint32_t interval) {
    const uint64_t n = len.size();
    std::vector<uint64_t> closed_first(n + 1);  // (sized exactly: an entry behind the table is an address error)
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; i++) closed_first[i] = run, run += batch_reset_closed_count(len[i], interval);
    closed_first[n] = run;
    const uint64_t closed = run;
    uint64_t S = 0;
    for (uint64_t i = 0; i < n; i++) S += reset_segment_count(len[i], interval);
    CHECK(closed + n == S, "%llu closed + %llu open, %llu segments", (unsigned long long)closed, (unsigned long long)n, (unsigned long long)S);
    std::vector<std::vector<uint8_t>> covered(n);
    for (uint64_t i = 0; i < n; i++) covered[i].assign(len[i], 0);
    auto cover = [&](const BatchResetRow& r) {
        CHECK(r.stream < n && r.start + r.len <= len[r.stream], "cut %llu+%u of stream %llu", (unsigned long long)r.start, r.len, (unsigned long long)r.stream);
        if (r.stream < n && r.start + r.len <= len[r.stream])
            for (uint32_t b = 0; b < r.len; b++) covered[r.stream][r.start + b]++;
    };
    // the walk: segment s of the batch is segment k of stream i; closed slot s - i, or open slot i
    uint64_t s = 0, closed_seen = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t K = reset_segment_count(len[i], interval);
        CHECK(closed_first[i] + i == s, "seg_first of stream %llu", (unsigned long long)i);
        for (uint64_t k = 0; k < K; k++, s++) {
            const uint64_t start = k * (uint64_t)interval;
            const uint32_t cut = (uint32_t)(len[i] - start < interval ? len[i] - start : interval);
            if (k + 1 < K) {
                const uint64_t c = s - i;
                CHECK(c == closed_seen && c < closed, "closed slot %llu", (unsigned long long)c);
                CHECK(batch_reset_owner(closed_first.data(), n, c) == i, "owner of %llu", (unsigned long long)c);
                const BatchResetRow r = batch_reset_closed_row(closed_first.data(), n, c, interval);
                CHECK(r.stream == i && r.k == k && r.start == start && r.len == cut && cut == interval, "closed row %llu", (unsigned long long)c);
                cover(r);
                closed_seen++;
            } else {
                const BatchResetRow r = batch_reset_open_row(closed_first.data(), i, len[i], interval);
                CHECK(r.stream == i && r.k == k && r.start == start && r.len == cut, "open row %llu", (unsigned long long)i);
                CHECK(len[i] == 0 || cut >= 1, "an empty open segment of a stream with bytes");
                cover(r);
            }
        }
    }
    CHECK(s == S && closed_seen == closed, "%llu segments walked", (unsigned long long)s);
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t b = 0; b < len[i]; b++) CHECK(covered[i][b] == 1, "byte %u of stream %llu covered %u times", b, (unsigned long long)i, covered[i][b]);
}

int main() {
    long batches = 0;
    for (uint32_t N : {1u, 16u}) {
        const uint32_t lens[7] = {0, 1, N - 1, N, N + 1, 2 * N, 2 * N + 1};
        for (int n = 1; n <= 4; n++) {
            int total = 1;
            for (int j = 0; j < n; j++) total *= 7;
            for (int code = 0; code < total; code++) {
                std::vector<uint32_t> len(n);
                for (int j = 0, c = code; j < n; j++, c /= 7) len[j] = lens[c % 7];
                batch(len, N);
                batches++;
            }
        }
    }
    // the ends of the 32-bit range: arithmetic only (no bytes)
    {
        const uint64_t cf[4] = {0, 1, 1, 2};  // lengths 2^32 - 1, 0, 2^32 - 1 at an interval of 2^31
        const BatchResetRow a = batch_reset_closed_row(cf, 3, 1, 0x80000000u), b = batch_reset_open_row(cf, 2, 0xFFFFFFFFu, 0x80000000u);
        CHECK(a.stream == 2 && a.k == 0 && a.start == 0 && a.len == 0x80000000u, "closed row at the end of the range");
        CHECK(b.stream == 2 && b.k == 1 && b.start == 0x80000000ull && b.len == 0x7FFFFFFFu, "open row at the end of the range");
        CHECK(batch_reset_open_row(cf, 1, 0, 0x80000000u).len == 0, "empty stream");
    }
    static_assert(batch_reset_closed_count(0, 16) == 0 && batch_reset_closed_count(16, 16) == 0 && batch_reset_closed_count(17, 16) == 1, "count");
    static_assert(batch_reset_closed_count(0xFFFFFFFFu, 1) == 0xFFFFFFFEull, "count at the end of the range");
    static_assert(batch_reset_slab_bytes(0, 65536, 8) == reset_slab_bytes(65536, 65536, 8) && batch_reset_slab_bytes(100, 65536, 8) == reset_slab_bytes(100, 65536, 8), "slab");
    printf("%s: %ld batches, %d failures\n", failures ? "FAILED" : "ok", batches, failures);
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("batch_resets")
    (d / "mapping.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), str(d / "mapping.cpp"), "-o", str(d / "mapping")]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizers' runtimes)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "mapping"), sanitized


def test_stream_segment_mapping(program):
    """Lengths from {0, 1, N-1, N, N+1, 2N, 2N+1}, every batch of up to 4 streams, N in {1, 16}: every segment maps to the right
    stream, cut and closed / open table slot, and S - n closed plus n open segments cover each input byte once."""
    exe, sanitized = program
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr, "(host ASan + UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    m = re.match(r"ok: (\d+) batches, 0 failures", p.stdout)
    assert m and int(m[1]) == 2 * (7 + 49 + 343 + 2401), p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
