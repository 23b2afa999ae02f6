"""CPU tier: packing a batch's streams densely (tamp_batch_pack, ``pack_batch``, ``BatchResult.packed``) as far as no device is
needed -- the symbol and its binding, what the C call refuses before it looks for a device, the keyword refusals of ``pack_batch``,
the numpy path (the model the GPU tests compare with) against a three-line loop, ``PackedBatch``'s accessors, and the tile / line
arithmetic of tamp_pack.hpp compiled for the HOST into a stand-alone program with the address and undefined-behaviour sanitizers when
the compiler has their runtimes (nothing loaded into python is sanitised)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tamp_batch_pack"
NO_DEVICE, BAD_ARGUMENT = -20, -21
TILE = 16384  # kPackTile of tamp_pack.hpp (the program below asserts it)


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
    assert len(fn.argtypes) == 10 and fn.restype is C.c_int
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T %s$" % NAME, out, flags=re.M)


def test_python_names():
    import tamp
    import tamp_amd

    for pkg in (tamp_amd, tamp):
        for name in ("PackedBatch", "pack_batch"):
            assert name in pkg.__all__ and getattr(pkg, name) is getattr(tamp_amd, name)
    assert callable(tamp_amd.BatchResult.packed)


def _arrays():
    a = dict(src=np.arange(64, dtype=np.uint8), src_off=np.array([0, 32], np.uint64), src_len=np.array([5, 7], np.uint32),
             dst=np.zeros(64, np.uint8), dst_off=np.zeros(3, np.uint64))
    return a, {k: v.ctypes.data_as(C.c_void_p) for k, v in a.items()}


def _call(lib, *, missing=(), n=2, cap=64, align=1, device=0):
    held, p = _arrays()
    for k in missing:
        p[k] = None
    rc = lib.tamp_batch_pack(p["src"], p["src_off"], p["src_len"], p["dst"], cap, p["dst_off"], n, align, device, None)
    assert (held["dst"] == 0).all() and (held["dst_off"] == 0).all()  # (host arrays: no call here may write them)
    return rc


def test_refusals_come_before_the_device(lib):
    for table in ("src_off", "src_len", "dst_off"):
        assert _call(lib, missing=(table,)) == BAD_ARGUMENT, table
        assert _call(lib, missing=(table,), n=0) == BAD_ARGUMENT, table
        assert _call(lib, missing=(table, "dst"), cap=0) == BAD_ARGUMENT, table
    assert _call(lib, missing=("src",)) == BAD_ARGUMENT       # no source and streams to read
    assert _call(lib, missing=("dst",), cap=1) == BAD_ARGUMENT  # room and nowhere to put it
    assert _call(lib, n=1 << 32) == BAD_ARGUMENT
    for align in (0, 3, 6, 12, 4097, 8192, 1 << 31, 0xFFFFFFFF):
        assert _call(lib, align=align) == BAD_ARGUMENT, align
    # every one of them is decided before the device: the same answers for a device there is none of
    assert _call(lib, missing=("src_off",), device=63) == BAD_ARGUMENT
    assert _call(lib, align=3, device=-7) == BAD_ARGUMENT


def test_a_well_formed_call_needs_a_device(lib):
    """Host arrays stand in for device memory here, so the call is only made where no device can take it."""
    if lib.tamp_amd_device_count() > 0:
        assert _call(lib, device=63) in (NO_DEVICE, BAD_ARGUMENT)  # (a device ordinal that is not there: nothing is launched)
        return
    for kwargs in ({}, dict(align=16), dict(align=4096), dict(n=0), dict(missing=("dst",), cap=0), dict(missing=("src",), n=0)):
        assert _call(lib, **kwargs) == NO_DEVICE, kwargs


def test_keyword_refusals_come_before_the_library(monkeypatch):
    """Every refusal is a ValueError raised before the native library is looked for."""
    import tamp_amd
    from tamp_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded before the keywords were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    data, off, length = np.arange(32, dtype=np.uint8), np.array([0, 8], np.uint64), np.array([8, 8], np.uint32)
    for bad in (0, 3, 24, 8192, -4, 2.0, "16", True, None):
        with pytest.raises(ValueError, match="align must be a power of two in 1..4096"):
            tamp_amd.pack_batch(data, off, length, align=bad)
        with pytest.raises(ValueError, match="align must be a power of two in 1..4096"):
            tamp_amd.BatchResult(data, off, length, None).packed(align=bad)
    with pytest.raises(ValueError, match="out= needs CUDA tensors"):
        tamp_amd.pack_batch(data, off, length, out=np.zeros(16, np.uint8))
    with pytest.raises(ValueError, match="out= needs CUDA tensors"):
        tamp_amd.BatchResult(data, off, length, None).packed(out=np.zeros(16, np.uint8))
    for o, l in ((off[:1], length), (off, length[:1]), (np.zeros(3, np.uint64), length)):
        with pytest.raises(ValueError, match="one offset and one length per stream"):
            tamp_amd.pack_batch(data, o, l)
    with pytest.raises(ValueError, match="ends behind the data"):
        tamp_amd.pack_batch(data, np.array([0, 30], np.uint64), length)
    # the host path needs no library at all
    p = tamp_amd.pack_batch(data, off, length)
    assert p.data.tobytes() == bytes(range(16))


def _model(data, off, length, align):
    """The three-line loop: every stream at the running sum of the padded lengths, zero between them."""
    out, at = bytearray(), []
    for o, n in zip(off, length):
        at.append(len(out))
        out += bytes(data[int(o) : int(o) + int(n)]) + bytes(-int(n) % align)
    return bytes(out), at + [len(out)]


@pytest.mark.parametrize("align", [1, 4, 16, 4096])
def test_numpy_pack_against_the_loop(align):
    import tamp_amd

    rng = np.random.default_rng(align)
    lens = np.array([0, 1, 15, 16, 17, 0, 0, 255, 4095, 4096, 4097, 33, 5000, 0], dtype=np.uint32)
    caps = lens.astype(np.uint64) + rng.integers(0, 9, len(lens)).astype(np.uint64)  # gaps between the streams
    starts = np.cumsum(caps) - caps
    data = rng.integers(0, 256, int(caps.sum()) + 3, dtype=np.uint8)
    for order in (np.arange(len(lens)), rng.permutation(len(lens)), np.array([3, 3, 9, 3], dtype=np.int64), np.zeros(0, np.int64)):
        off, length = starts[order], lens[order]
        p = tamp_amd.pack_batch(data, off, length, align=align)
        want, at = _model(data, off, length, align)
        assert p.data.dtype == np.uint8 and p.off.dtype == np.uint64 and p.len.dtype == np.uint32
        assert p.data.tobytes() == want and p.off.tolist() == at and p.len.tolist() == length.tolist()
        assert all(int(x) % align == 0 for x in p.off)
    # other integer types and a bytes object for the data
    p = tamp_amd.pack_batch(data.tobytes(), starts.astype(np.int64), lens.astype(np.int32), align=align)
    assert p.data.tobytes() == _model(data, starts, lens, align)[0]


def test_packed_batch_accessors_agree():
    import tamp_amd

    streams = [b"", b"a", b"hello world", bytes(range(200)), b"", b"xyz"]
    flat, off, length = tamp_amd.pack_streams(streams)
    slabs = tamp_amd.BatchResult(np.concatenate([flat, np.zeros(8, np.uint8)]), off, length, np.zeros(len(streams), np.int8))
    for align in (1, 16):
        p = slabs.packed(align=align)
        assert isinstance(p, tamp_amd.PackedBatch) and p.cpu() is p
        assert p.streams() == streams == [p.stream(i) for i in range(len(streams))] == slabs.streams()
        data, in_off, in_len = p.triple()
        assert data is p.data and len(in_off) == len(in_len) == len(streams) and in_off.tolist() == p.off[:-1].tolist()
        assert [data[int(o) : int(o) + int(n)].tobytes() for o, n in zip(in_off, in_len)] == streams
        assert int(p.off[-1]) == len(p.data) == sum(-(-len(s) // align) * align for s in streams)
    empty = tamp_amd.pack_batch(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert empty.streams() == [] and empty.off.tolist() == [0] and len(empty.data) == 0 and len(empty.triple()[1]) == 0


PROGRAM = r"""
#include "tamp_pack.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace tamp_amd;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)
typedef unsigned long long ull;

// Stream i holds kStreamLen bytes at most, a stretch of one table of bytes that are never 0 (padding is); neighbouring streams and
// neighbouring positions differ.  (Whole lines are filled, claimed and compared sixteen bytes at a time: the program walks 0.7 GB.)
constexpr uint32_t kStreamLen = 2 * kPackTile + 1, kStreamShift = 131;
static std::vector<uint8_t> table;
static const uint8_t* content(uint64_t stream) { return table.data() + kStreamShift * (stream % 32); }

// One batch, packed by the walk the copy kernel makes -- its tiles, its lines, its owner searches and the line values of
// tamp_pack.hpp -- every stored byte claimed.  The source holds the streams back to back in REVERSE order and is sized
// exactly: a load outside a stream's bytes is an address error at the buffer's ends and a wrong byte elsewhere.
static void batch(const std::vector<uint32_t>& len, uint32_t align, uint32_t skew) {
    const uint64_t n = len.size();
    std::vector<uint64_t> src_off(n), dst_off(n + 1);
    uint64_t bytes = 0;
    for (uint64_t i = n; i-- > 0;) src_off[i] = bytes, bytes += len[i];
    std::vector<uint8_t> src(bytes);
    for (uint64_t i = 0; i < n; i++)
        if (len[i]) memcpy(&src[src_off[i]], content(i), len[i]);
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; i++) dst_off[i] = run, run += pack_padded(len[i], align);
    const uint64_t total = dst_off[n] = run;
    std::vector<uint8_t> want(total, 0), got(total, 0xEE), claims(total, 0);
    for (uint64_t i = 0; i < n; i++)
        if (len[i]) memcpy(&want[dst_off[i]], content(i), len[i]);
    const uint64_t tiles = pack_tile_count(skew, total);
    CHECK(tiles == (total ? (skew + total + kPackTile - 1) / kPackTile : 0), "%llu tiles for %llu bytes at skew %u", (ull)tiles, (ull)total, skew);
    uint64_t s_hi = 0, covered = 0;
    for (uint64_t t = 0; t < tiles; t++) {
        const PackSpan tile = pack_tile_span(skew, total, t);
        CHECK(tile.lo == covered && tile.hi > tile.lo && tile.hi <= total && tile.hi - tile.lo <= kPackTile, "tile %llu: [%llu, %llu)", (ull)t, (ull)tile.lo, (ull)tile.hi);
        covered = tile.hi;
        const uint64_t s_lo = t == 0 ? pack_owner(dst_off.data(), 0, n, tile.lo) : pack_owner_from(dst_off.data(), s_hi, n, tile.lo);
        s_hi = pack_owner_from(dst_off.data(), s_lo, n, tile.hi - 1);
        CHECK(dst_off[s_lo] <= tile.lo && tile.lo < dst_off[s_lo + 1] && dst_off[s_hi] <= tile.hi - 1 && tile.hi - 1 < dst_off[s_hi + 1], "owners of tile %llu", (ull)t);
        CHECK(s_lo == pack_owner(dst_off.data(), 0, n, tile.lo) && s_hi == pack_owner(dst_off.data(), 0, n, tile.hi - 1), "the two searches agree");
        const bool whole = s_lo == s_hi && tile.hi - tile.lo == kPackTile && tile.hi <= dst_off[s_lo] + len[s_lo];  // (the kernel's short cut)
        for (uint32_t line = 0; line < kPackTile / kPackLine; line++) {
            const PackSpan s = pack_line_span(skew, total, t, line);
            if (s.hi <= s.lo) continue;
            CHECK(s.lo >= tile.lo && s.hi <= tile.hi && s.hi - s.lo <= kPackLine, "line %u of tile %llu", line, (ull)t);
            const uint32_t k0 = (uint32_t)((s.lo + skew) & (kPackLine - 1));
            CHECK(k0 + (s.hi - s.lo) <= kPackLine && (s.hi - s.lo == kPackLine ? k0 == 0 : (s.lo == 0 || s.hi == total)), "line [%llu, %llu) at byte %u", (ull)s.lo, (ull)s.hi, k0);
            const uint64_t i = pack_owner(dst_off.data(), s_lo, s_hi + 1, s.lo);
            CHECK(dst_off[i] <= s.lo && s.lo < dst_off[i + 1], "owner of %llu", (ull)s.lo);
            const bool body = pack_line_is_body(dst_off.data(), len.data(), i, s);
            CHECK(!whole || (body && i == s_lo), "a whole tile holds body lines of its one stream only");
            const PackLine x = body ? pack_load16(src.data() + src_off[i] + (s.lo - dst_off[i]))
                                    : pack_line_value(src.data(), src_off.data(), len.data(), dst_off.data(), i, s_hi + 1, s, k0);
            if (s.hi - s.lo == kPackLine) {
                uint64_t c[2];
                memcpy(c, &claims[s.lo], 16);
                CHECK(c[0] == 0 && c[1] == 0, "line at %llu claimed before", (ull)s.lo);
                memset(&claims[s.lo], 1, 16), memcpy(&got[s.lo], &x.x0, 8), memcpy(&got[s.lo + 8], &x.x1, 8);
            } else {
                for (uint64_t b = 0; b < s.hi - s.lo; b++) {
                    const uint32_t k = k0 + (uint32_t)b;
                    claims[s.lo + b]++, got[s.lo + b] = (uint8_t)((k < 8 ? x.x0 : x.x1) >> (8 * (k & 7)));
                }
            }
            // (what the line holds above its claimed bytes is never stored, but it must be zero: nothing of another stream is loaded)
            if (!body && k0 == 0 && s.hi - s.lo < kPackLine) {
                const uint64_t w = s.hi - s.lo, above = w >= 8 ? x.x1 >> (8 * (w - 8)) : (x.x1 | x.x0 >> (8 * w));
                CHECK(above == 0, "bytes above the last line's %llu", (ull)w);
            }
        }
    }
    CHECK(covered == total, "tiles cover %llu of %llu bytes", (ull)covered, (ull)total);
    const std::vector<uint8_t> once(total, 1);
    if (total && (memcmp(claims.data(), once.data(), total) || memcmp(got.data(), want.data(), total)))
        for (uint64_t b = 0; b < total; b++) {
            if (claims[b] != 1) { CHECK(claims[b] == 1, "byte %llu claimed %u times", (ull)b, claims[b]); break; }
            if (got[b] != want[b]) { CHECK(got[b] == want[b], "byte %llu is %u, not %u", (ull)b, got[b], want[b]); break; }
        }
}

int main() {
    static_assert(kPackTile == TILE && kPackLine == 16 && kPackTile % kPackLine == 0, "the geometry the tests are written for");
    const uint32_t T = kPackTile;
    table.resize(kStreamLen + 31 * kStreamShift);
    for (size_t j = 0; j < table.size(); j++) table[j] = (uint8_t)(1 + (j * 7 + (j >> 8) * 3) % 255);
    const uint32_t lens[9] = {0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 1};
    long batches = 0;
    for (uint32_t align : {1u, 16u})
        for (int n = 1; n <= 4; n++) {
            int count = 1;
            for (int j = 0; j < n; j++) count *= 9;
            for (int code = 0; code < count; code++) {
                std::vector<uint32_t> len(n);
                for (int j = 0, c = code; j < n; j++, c /= 9) len[j] = lens[c % 9];
                batch(len, align, 0);
                // a destination that is not tile aligned, not even line aligned (the smaller batches: the cuts move, the walk is the same)
                if (n <= 2) for (uint32_t skew : {1u, 15u, 16u, T - 17, T - 1}) batch(len, align, skew);
                batches++;
            }
        }
    // other alignments, a run of empty streams inside a line, many streams in one tile
    for (uint32_t align : {2u, 256u, 4096u}) batch({5, 0, 0, 0, 0, 0, 0, 3, 4097, 0, 1}, align, 9);
    {
        std::vector<uint32_t> len(3000);
        for (size_t i = 0; i < len.size(); i++) len[i] = (uint32_t)(i * 7 % 41);
        batch(len, 1, 3), batch(len, 4, 0);
    }
    // the ends of the range: arithmetic only (no bytes)
    static_assert(pack_align_ok(1) && pack_align_ok(4096) && !pack_align_ok(0) && !pack_align_ok(3) && !pack_align_ok(8192) && !pack_align_ok(0x80000000u), "align");
    static_assert(pack_padded(0, 4096) == 0 && pack_padded(1, 4096) == 4096 && pack_padded(0xFFFFFFFFu, 1) == 0xFFFFFFFFull, "padded");
    static_assert(pack_padded(0xFFFFFFFFu, 4096) == 0x100000000ull && pack_padded(0xFFFFF001u, 4096) == 0x100000000ull, "padded beyond 32 bits");
    {
        const uint64_t M = 0xFFFFFFFFull;
        uint64_t off[6] = {0, M, 2 * M, 2 * M, 3 * M, 4 * M};  // lengths 2^32 - 1 (and an empty stream)
        CHECK(pack_owner(off, 0, 5, M - 1) == 0 && pack_owner(off, 0, 5, M) == 1 && pack_owner(off, 0, 5, 2 * M) == 3 && pack_owner(off, 0, 5, 4 * M - 1) == 4, "owners beyond 2^32");
        CHECK(pack_owner_from(off, 0, 5, 4 * M - 1) == 4 && pack_owner_from(off, 1, 5, 2 * M - 1) == 1 && pack_owner_from(off, 1, 5, 2 * M) == 3, "owners beyond 2^32, from a stream in front");
        const uint64_t total = 4 * M;
        CHECK(pack_tile_count(0, total) == (total + T - 1) / T && pack_tile_count(T - 1, total) == (total + 2 * T - 2) / T, "tiles beyond 2^32");
        const uint64_t t = (1ull << 33) / T;  // the tile that starts at packed byte 2^33 - skew
        const PackSpan a = pack_tile_span(5, total, t), b = pack_line_span(5, total, t, 1), z = pack_tile_span(5, total, pack_tile_count(5, total) - 1);
        CHECK(a.lo == (1ull << 33) - 5 && a.hi == a.lo + T && b.lo == a.lo + 16 && b.hi == b.lo + 16 && z.hi == total && z.lo < z.hi, "spans beyond 2^32");
        std::vector<uint32_t> len = {0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 0xFFFFFFFFu};
        uint64_t pieces = 0;
        pack_walk(off, len.data(), 0, 5, M - 3, M + 4, [&](uint64_t s, uint64_t at, uint64_t pos, uint32_t m) {
            CHECK((pieces == 0 && s == 0 && at == M - 3 && pos == M - 3 && m == 3) || (pieces == 1 && s == 1 && at == 0 && pos == M && m == 4), "piece %llu", (ull)pieces);
            pieces++;
        });
        CHECK(pieces == 2, "%llu pieces", (ull)pieces);
        // the largest batch there is: 2^32 - 1 streams of 2^32 - 1 bytes, padded to 4096, still counts in 64 bits
        CHECK(M * pack_padded(0xFFFFFFFFu, 4096) / M == 0x100000000ull && pack_tile_count(T - 1, M * 0x100000000ull) == (M << 32) / T + 1, "the largest batch");
    }
    printf("%s: %ld batches, %d failures\n", failures ? "FAILED" : "ok", batches, failures);
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("pack")
    (d / "walk.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "c++", "-O2", "-g", "-std=c++17", "-DTILE=%d" % TILE, "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), str(d / "walk.cpp"), "-o", str(d / "walk")]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizers' runtimes)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "walk"), sanitized


def test_every_packed_byte_has_one_writer(program):
    """Lengths from {0, 1, 15, 16, 17, T-1, T, T+1, 2T+1}, every batch of up to 4 streams, align in {1, 16}: walking all tiles and
    lines the way the copy kernel does, every destination byte below the total is claimed exactly once, as the right byte of the right
    stream or as zero padding, and none at or beyond the total; then the arithmetic with lengths of 2^32 - 1 and offsets beyond 2^32."""
    exe, sanitized = program
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr, "(host ASan + UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    m = re.match(r"ok: (\d+) batches, 0 failures", p.stdout)
    assert m and int(m[1]) == 2 * (9 + 81 + 729 + 6561), p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
