"""CPU tier: finding the resets of a batch (tamp_batch_index_resets, ``index_resets``) as far as no device is needed -- the symbol
and its binding, the chunk size in the header and beside the kernels, the Python names, the keyword refusals of ``index_resets``,
what the C call refuses before it looks for a device, and the scan and merge arithmetic of tamp_reset_index.hpp compiled for the
HOST into a stand-alone program with the address and undefined-behaviour sanitizers when the compiler has their runtimes (nothing
loaded into python is sanitised)."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARGUMENTS = "tamp_batch_index_resets", 14
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
    assert re.search(r"\b%s\s*\(" % NAME, code)
    assert NAME in _lib.SYMBOLS and hasattr(C.CDLL(_lib.LIB_PATH), NAME)
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == ARGUMENTS and fn.restype is C.c_int
    assert fn.argtypes[8] is C.c_uint64 and fn.argtypes[10] is C.c_size_t  # reset_cap, n_streams
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T %s$" % NAME, out, flags=re.M)


def test_chunk_size_is_one_number():
    from tamp_amd import _lib

    header = open(os.path.join(ROOT, "include", "tamp_amd.h")).read()
    arith = open(os.path.join(ROOT, "tamp_amd", "csrc", "tamp_reset_index.hpp")).read()
    kernels = open(os.path.join(ROOT, "tamp_amd", "csrc", "tamp_reset_index_kernel.hpp")).read()
    h = re.search(r"#define\s+TAMP_AMD_INDEX_RESETS_CHUNK_BITS\s+(\d+)", header)
    k = re.search(r"constexpr uint32_t kIndexChunkBits = (\d+);", arith)
    assert h and k and int(h[1]) == int(k[1]) == _lib.INDEX_RESETS_CHUNK_BITS == 1024
    assert '#include "tamp_reset_index.hpp"' in kernels and "kIndexChunkBits" in kernels
    assert not re.search(r"\b1024\b", re.sub(r"//.*", "", kernels)), "the kernels take the chunk size from the arithmetic header"


def test_python_names():
    import tamp
    import tamp_amd

    for pkg in (tamp_amd, tamp):
        for name in ("index_resets", "ResetScan"):
            assert name in pkg.__all__ and getattr(pkg, name) is getattr(tamp_amd, name)
    assert [f.name for f in dataclasses.fields(tamp_amd.ResetScan)][:5] == ["index", "status", "closed_size", "open_size", "kernel_ms"]
    assert [f.name for f in dataclasses.fields(tamp_amd.ResetIndex)][-1] == "interval"
    assert [f.name for f in dataclasses.fields(tamp_amd.BatchResult)][-1] == "reset_index"
    idx = tamp_amd.ResetIndex(np.array([0, 2, 2, 3], np.uint64), np.array([9, 20, 7], np.uint32))
    scan = tamp_amd.ResetScan(idx, np.zeros(3, np.int8), np.array([5, 0xFFFFFFFF, 1], np.uint32), np.array([4, 6, 0], np.uint32))
    assert (scan.size(0), scan.size(1), scan.size(2)) == (5 + 0xFFFFFFFF + 4, 6, 1) and scan.kernel_ms == -1.0
    assert all(isinstance(scan.size(i), int) for i in range(3))


def test_command_line_takes_files():
    from tamp_amd import cli

    args = cli.build_parser().parse_args(["index", "a.tamp", "b.tamp"])
    assert args.command == "index" and args.files == ["a.tamp", "b.tamp"]
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["index"])


def test_interval_detection():
    from tamp_amd.batch import _detect_interval

    first = np.array([0, 2, 2, 3], np.uint64)

    def found(closed, open_size, status=(0, 0, 0)):
        return _detect_interval(first, np.array(closed, np.uint32), np.array(open_size, np.uint32), np.array(status, np.int8))

    assert found([64, 64, 64], [3, 64, 0]) == 64
    assert found([64, 64, 64], [3, 65, 0]) is None  # an open segment larger than the closed ones
    assert found([64, 63, 64], [3, 3, 0]) is None
    assert found([64, 64, 9], [3, 3, 0], (0, 0, -4)) == 64  # (the closed segments of streams that are not TAMP_OK do not count)
    assert found([64, 64, 9], [3, 3, 0], (-4, 0, -4)) is None  # no closed segment left
    assert _detect_interval(np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.array([5, 5], np.uint32), np.zeros(2, np.int8)) is None


def test_keyword_refusals_come_before_the_library(monkeypatch):
    """Every refusal is a ValueError raised before the native library is looked for."""
    import tamp_amd
    from tamp_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded before the keywords were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    data = [b"abc", b"defg"]
    flat, in_off, in_len = tamp_amd.pack_streams(data)
    for args in ((data,), (flat, in_off, in_len)):
        for bad in (7, 16, 0, -1, 1.5, "15", True, None):
            with pytest.raises(ValueError, match="max_window_bits"):
                tamp_amd.index_resets(*args, max_window_bits=bad)
        with pytest.raises(AssertionError, match="the library was loaded"):  # what is fine gets as far as the library
            tamp_amd.index_resets(*args, max_window_bits=8)
    with pytest.raises(ValueError, match="one entry per stream each"):
        tamp_amd.index_resets(flat, in_off, in_len[:1])
    with pytest.raises(ValueError, match="one entry per stream each"):
        tamp_amd.index_resets(flat, np.zeros(3, np.uint64), in_len)
    with pytest.raises(ValueError, match="both or neither"):
        tamp_amd.index_resets(flat, in_off)


TABLES = ("in_off", "in_len", "reset_first", "status")


def _call(lib, *, missing=(), n=1, cap=4, mem=None, device=0):
    from tamp_amd import _lib

    a = dict(data=np.array([0x59, 0, 0, 0], dtype=np.uint8), in_off=np.zeros(1, np.uint64), in_len=np.full(1, 4, np.uint32),
             reset_first=np.full(2, 77, np.uint64), reset_off=np.zeros(4, np.uint32), closed_size=np.zeros(4, np.uint32),
             open_size=np.zeros(1, np.uint32), status=np.zeros(1, np.int8))
    p = {k: (None if k in missing else v.ctypes.data_as(C.c_void_p)) for k, v in a.items()}
    rc = lib.tamp_batch_index_resets(15, p["data"], p["in_off"], p["in_len"], p["reset_first"], p["reset_off"], p["closed_size"],
                                     p["open_size"], cap, p["status"], n, _lib.MEM_HOST if mem is None else mem, device, None)
    return rc, a


def test_call_level_refusals(lib):
    """Before a device is looked for: TAMP_AMD_BAD_ARGUMENT on a machine with and without one, for both memory kinds."""
    from tamp_amd import _lib

    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        for table in TABLES:
            assert _call(lib, missing=(table,), mem=mem)[0] == BAD_ARGUMENT, table
            assert _call(lib, missing=(table,), mem=mem, n=0)[0] == BAD_ARGUMENT, table
        assert _call(lib, missing=("data",), mem=mem)[0] == BAD_ARGUMENT
        assert _call(lib, missing=("reset_off",), mem=mem)[0] == BAD_ARGUMENT
        assert _call(lib, missing=("reset_off", "closed_size"), mem=mem, cap=1)[0] == BAD_ARGUMENT
        assert _call(lib, device=_lib.ALL_DEVICES, mem=mem)[0] == BAD_ARGUMENT
        assert _call(lib, n=1 << 32, mem=mem)[0] == BAD_ARGUMENT
    for mem in (2, -1, 7):
        assert _call(lib, mem=mem)[0] == BAD_ARGUMENT
        assert _call(lib, mem=mem, device=_lib.ALL_DEVICES)[0] == BAD_ARGUMENT


def test_no_streams(lib):
    """n == 0: TAMP_OK and reset_first[0] = 0 (TAMP_AMD_NO_DEVICE is allowed on a machine without a device)."""
    from tamp_amd import _lib

    rc, a = _call(lib, n=0, missing=("data", "reset_off", "closed_size", "open_size"), cap=0)
    assert rc in (0, -20)
    if rc == 0:
        assert list(a["reset_first"]) == [0, 77]
    assert _call(lib, n=0, mem=_lib.MEM_DEVICE)[0] in (0, -20)


PROGRAM = r"""
#include "tamp_reset_index.hpp"
#include "tamp_reset_merge.hpp"
#include <cstdio>
#include <vector>
using namespace tamp_amd;

static int failures = 0;
static long batches = 0, chunks_seen = 0, merged = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)
typedef unsigned long long ull;

static uint32_t rng_state = 12345;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) % n; }

struct Token { bool flush; uint32_t end; uint32_t bytes; };  // end: the byte position behind it
struct Chunk { std::vector<Token> t; };
typedef std::vector<Chunk> Stream;

// A chunk whose report is (tokens or none, first token a FLUSH, last token a FLUSH, `inner` FLUSH-after-FLUSH pairs).
static Chunk make_chunk(bool any, bool ff, bool lf, uint32_t inner, uint32_t& pos, bool big) {
    Chunk c;
    if (!any) return c;
    auto put = [&](bool flush) {
        uint32_t bytes = flush ? 0 : rnd(300);
        if (!flush && big) bytes = 0x7FFFFFF0u + rnd(32), big = false;  // (one per chunk: a chunk's bytes are a 32-bit sum)
        pos += 1 + rnd(3);
        c.t.push_back({flush, pos, bytes});
    };
    if (inner == 0 && ff == lf && rnd(2)) { put(ff); return c; }  // a chunk of one token
    put(ff);
    put(false);
    if (inner) {
        for (uint32_t k = 0; k <= inner; k++) put(true);
        put(false);
    }
    put(lf);
    return c;
}

static IndexChunkReport report_of(const Chunk& c, bool head) {
    IndexChunkReport r = {head ? kIndexHead : 0u, 0, 0, 0};
    bool prev = false;
    for (size_t k = 0; k < c.t.size(); k++) {
        if (k == 0) r.first_end = c.t[k].end, r.flags |= kIndexHasTokens | (c.t[k].flush ? kIndexFirstFlush : 0u);
        else if (c.t[k].flush && prev) r.inner++;
        r.bytes += c.t[k].bytes, prev = c.t[k].flush;
    }
    if (!c.t.empty() && prev) r.flags |= kIndexLastFlush;
    return r;
}

// The scan as the device runs it: tiles of `tile` chunks, each folded, the tiles' values scanned, every chunk from its tile's base.
static void scan(const std::vector<IndexChunkReport>& rep, size_t tile, std::vector<uint64_t>& place, std::vector<uint64_t>& bytes) {
    const size_t C = rep.size(), T = (C + tile - 1) / tile;
    std::vector<IndexSum> sum(T, index_sum_identity()), before(T + 1, index_sum_identity());
    for (size_t c = 0; c < C; c++) sum[c / tile] = index_sum_combine(sum[c / tile], index_sum_of(rep[c].flags, rep[c].inner, rep[c].bytes));
    for (size_t t = 0; t < T; t++) before[t + 1] = index_sum_combine(before[t], sum[t]);
    place.assign(C + 1, 0), bytes.assign(C + 1, 0);
    IndexSum at = index_sum_identity();
    for (size_t c = 0; c < C; c++) {
        if (c % tile == 0) at = before[c / tile];
        place[c] = index_chunk_place(at, rep[c].flags), bytes[c] = at.b;
        at = index_sum_combine(at, index_sum_of(rep[c].flags, rep[c].inner, rep[c].bytes));
    }
    place[C] = index_chunk_place(before[T], kIndexHead), bytes[C] = before[T].b;
}

static void batch(const std::vector<Stream>& streams) {
    batches++;
    // the plain walk, stream by stream
    std::vector<std::vector<uint32_t>> want_off(streams.size()), want_closed(streams.size());
    std::vector<uint32_t> want_open(streams.size());
    for (size_t s = 0; s < streams.size(); s++) {
        bool prev = false;
        uint64_t seg = 0;
        for (const Chunk& c : streams[s])
            for (const Token& t : c.t) {
                if (t.flush && prev) want_off[s].push_back(t.end), want_closed[s].push_back(seg < 0xFFFFFFFFull ? (uint32_t)seg : 0xFFFFFFFFu), seg = 0;
                seg += t.bytes, prev = t.flush;
            }
        want_open[s] = seg < 0xFFFFFFFFull ? (uint32_t)seg : 0xFFFFFFFFu;
    }
    // the reports and the chunk table
    std::vector<IndexChunkReport> rep;
    std::vector<const Chunk*> chunk;
    std::vector<uint64_t> chunk_first(streams.size() + 1, 0);
    for (size_t s = 0; s < streams.size(); s++) {
        for (size_t k = 0; k < streams[s].size(); k++) rep.push_back(report_of(streams[s][k], k == 0)), chunk.push_back(&streams[s][k]);
        chunk_first[s + 1] = rep.size();
    }
    chunks_seen += rep.size();
    for (size_t c = 0; c < rep.size(); c++) {
        const uint64_t o = batch_reset_owner(chunk_first.data(), streams.size(), c);
        CHECK(chunk_first[o] <= c && c < chunk_first[o + 1], "owner of chunk %zu", c);
    }
    for (size_t tile : {(size_t)1, (size_t)2, (size_t)3, (size_t)64}) {
        std::vector<uint64_t> place, bytes;
        scan(rep, tile, place, bytes);
        const uint64_t E = index_place_base(place[rep.size()]);
        std::vector<uint32_t> off(E, 0xEEEEEEEEu), closed(E);
        std::vector<uint64_t> count(E), first(streams.size() + 1);
        for (size_t c = 0; c < rep.size(); c++) {  // the write pass
            uint64_t at = index_place_base(place[c]), run = 0;
            bool prev = index_place_flush_in(place[c]);
            for (const Token& t : chunk[c]->t) {
                if (t.flush && prev) {
                    CHECK(at < E, "an entry behind the table");
                    if (at < E) off[at] = t.end, count[at] = bytes[c] + run;
                    at++;
                }
                run += t.bytes, prev = t.flush;
            }
            CHECK(at == index_place_base(place[c + 1]), "chunk %zu ends where the next one begins", c);
        }
        for (size_t s = 0; s <= streams.size(); s++) first[s] = index_place_base(place[chunk_first[s]]);
        CHECK(first[0] == 0, "the table starts at 0");
        for (size_t s = 0; s < streams.size(); s++) {
            CHECK(first[s + 1] - first[s] == want_off[s].size(), "stream %zu: %llu entries, %zu wanted (tile %zu)", s, (ull)(first[s + 1] - first[s]), want_off[s].size(), tile);
            if (first[s + 1] - first[s] != want_off[s].size()) continue;
            for (uint64_t e = first[s]; e < first[s + 1]; e++) {
                const uint64_t o = batch_reset_owner(first.data(), streams.size(), e);
                CHECK(o == s, "owner of entry");
                closed[e] = index_size(e == first[o] ? bytes[chunk_first[o]] : count[e - 1], count[e]);
                CHECK(off[e] == want_off[s][e - first[s]] && closed[e] == want_closed[s][e - first[s]], "stream %zu entry %llu", s, (ull)(e - first[s]));
            }
            uint64_t from = bytes[chunk_first[s]];
            if (first[s + 1] != first[s]) {  // the open segment, as the lane per stream finds it
                const uint64_t ch = index_last_entry_chunk(place.data(), chunk_first[s], chunk_first[s + 1]);
                CHECK(index_place_base(place[ch]) < first[s + 1] && index_place_base(place[ch + 1]) == first[s + 1], "the chunk of the last entry");
                bool prev = index_place_flush_in(place[ch]);
                uint64_t run = 0;
                for (const Token& t : chunk[ch]->t) {
                    if (t.flush && prev) from = bytes[ch] + run;
                    run += t.bytes, prev = t.flush;
                }
            }
            CHECK(index_size(from, bytes[chunk_first[s + 1]]) == want_open[s], "stream %zu open size", s);
        }
    }
    // the host merge of the one-stream call, where a chunk has no more resets than it reports
    for (size_t s = 0; s < streams.size(); s++) {
        std::vector<ResetChunkReport> old;
        bool fits = true;
        for (const Chunk& c : streams[s]) {
            const IndexChunkReport r = report_of(c, false);
            ResetChunkReport o = {r.flags & 7u, r.first_end, r.inner, {0, 0, 0, 0}, 0};
            bool prev = false;
            uint32_t n = 0;
            for (size_t k = 0; k < c.t.size(); k++) {
                if (k && c.t[k].flush && prev && n < kResetChunkInner) o.inner[n++] = c.t[k].end;
                prev = c.t[k].flush;
            }
            fits = fits && r.inner <= kResetChunkInner;
            old.push_back(o);
        }
        std::vector<uint32_t> b;
        const bool ok = reset_merge(old.data(), old.size(), b);
        CHECK(ok == fits, "reset_merge's limit");
        if (ok) {
            merged++;
            CHECK(b == want_off[s], "stream %zu against reset_merge", s);
        }
    }
}

int main() {
    const uint32_t inners[5] = {0, 1, 4, 5, 40};
    // every report sequence of one stream of 0 to 3 chunks
    for (uint32_t n = 0; n <= 3; n++) {
        std::vector<uint32_t> pick(n, 0);
        for (;;) {
            Stream s;
            uint32_t pos = 2;
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t v = pick[k];
                s.push_back(v == 20 ? make_chunk(false, false, false, 0, pos, false) : make_chunk(true, v & 1, (v >> 1) & 1, inners[v >> 2], pos, false));
            }
            batch({s});
            uint32_t k = 0;
            while (k < n && ++pick[k] == 21) pick[k++] = 0;
            if (k == n) break;
        }
    }
    // batches of 1 to 3 streams of 0 to 5 chunks, drawn: the carry at every stream's first chunk, running sums around 2^32
    for (uint32_t round = 0; round < 60000; round++) {
        std::vector<Stream> b(1 + rnd(3));
        for (Stream& s : b) {
            uint32_t pos = 2;
            const uint32_t n = rnd(6);
            for (uint32_t k = 0; k < n; k++) {
                const bool flushy = rnd(3) != 0;  // (mostly FLUSH at the edges: that is where the carry matters)
                s.push_back(rnd(5) == 0 ? make_chunk(false, false, false, 0, pos, false)
                                        : make_chunk(true, flushy || rnd(2), flushy || rnd(2), inners[rnd(5)], pos, rnd(4) == 0));
            }
        }
        batch(b);
    }
    // the operator: associative on drawn values, the identity on both sides
    for (uint32_t round = 0; round < 200000; round++) {
        IndexSum v[3];
        for (IndexSum& x : v) {
            x = index_sum_of(rnd(16), rnd(3), rnd(1000));
            if (rnd(2)) x = index_sum_combine(x, index_sum_of(rnd(16), rnd(3), rnd(1000)));
        }
        const IndexSum l = index_sum_combine(index_sum_combine(v[0], v[1]), v[2]), r = index_sum_combine(v[0], index_sum_combine(v[1], v[2]));
        CHECK(l.e == r.e && l.b == r.b, "associative");
        const IndexSum a = index_sum_combine(index_sum_identity(), v[0]), z = index_sum_combine(v[0], index_sum_identity());
        CHECK(a.e == v[0].e && z.e == v[0].e && a.b == v[0].b && z.b == v[0].b, "identity");
    }
    // what a stream's first bytes decide
    const uint8_t plain[3] = {0x58, 0xFF, 0}, reset[3] = {0x59, 0, 0}, more[3] = {0x59, 1, 0}, wide[3] = {0xF9, 0, 0}, custom[3] = {0x5D, 0, 0};
    CHECK(index_stream_plan(nullptr, 0, 15).status == kIndexInputExhausted, "no bytes");
    CHECK(index_stream_plan(reset, 1, 15).status == kIndexInputExhausted && index_stream_plan(plain, 1, 15).status == kIndexOk, "one byte");
    CHECK(index_stream_plan(plain, 1, 15).header_bytes == 1 && index_stream_plan(plain, 1, 15).chunks == 1, "a one-byte header alone");
    CHECK(index_stream_plan(reset, 2, 15).status == kIndexOk && index_stream_plan(reset, 2, 15).header_bytes == 2, "a header and nothing else");
    CHECK(index_stream_plan(more, 3, 15).status == kIndexInvalidConf, "second header byte");
    CHECK(index_stream_plan(wide, 3, 14).status == kIndexInvalidConf && index_stream_plan(wide, 3, 15).status == kIndexOk, "window");
    CHECK(index_stream_plan(custom, 3, 15).status == kIndexOk, "the custom bit");
    CHECK(index_stream_plan(reset, kIndexMaxStream + 1, 15).status == kIndexBadArgument && index_stream_plan(reset, kIndexMaxStream, 15).status == kIndexOk, "length");
    CHECK(index_stream_plan(more, kIndexMaxStream + 1, 15).status == kIndexInvalidConf, "the first rule that applies");
    CHECK(index_stream_plan(reset, 128, 15).chunks == 1 && index_stream_plan(reset, 129, 15).chunks == 2, "chunks");
    CHECK(index_stream_plan(reset, kIndexMaxStream, 15).chunks == (kIndexMaxStream + 127) / 128, "chunks of the longest stream");
    static_assert(index_size(5, 9) == 4 && index_size(0, 0xFFFFFFFEull) == 0xFFFFFFFEu && index_size(0, 0xFFFFFFFFull) == 0xFFFFFFFFu &&
                  index_size(7, (1ull << 33) + 7) == 0xFFFFFFFFu, "sizes saturate");
    static_assert(index_round_bound(1) == 3 && index_round_bound(64) == 3 && index_round_bound(65) == 4 && index_round_bound(200) == 6, "rounds");
    printf("%s: %ld batches, %ld chunks, %ld streams against reset_merge, %d failures\n", failures ? "FAILED" : "ok", batches, chunks_seen, merged, failures);
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("index_resets")
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


def test_scan_and_merge_arithmetic(program):
    """Every report sequence of one stream of 0 to 3 chunks (a chunk without tokens, or with every combination of first-FLUSH and
    last-FLUSH and 0, 1, 4, 5 or 40 inner resets) and 60,000 drawn batches of 1 to 3 streams of 0 to 5 chunks, some with 2^31 decoded
    bytes in a chunk: entries, offsets, closed and open sizes through the scan in tiles of 1, 2, 3 and 64 chunks against a plain walk
    over the tokens, and against reset_merge where no chunk passes its limit of four; the operator's associativity; the header rules."""
    exe, sanitized = program
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr, "(host ASan + UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    m = re.match(r"ok: (\d+) batches, (\d+) chunks, (\d+) streams against reset_merge, 0 failures", p.stdout)
    assert m and int(m[1]) == 1 + 21 + 21 ** 2 + 21 ** 3 + 60000 and int(m[2]) > 100000 and int(m[3]) > 10000, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
