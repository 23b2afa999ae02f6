"""CPU tier: dictionary-reset segments (tamp_amd_compress_resets) as far as no device is needed -- the ``reset_interval`` keyword's
rules, the command line's option, the symbols, the bound against the checker's sizes, and the segment table's arithmetic
(tamp_reset_segments.hpp) compiled for the HOST into a stand-alone program with the address and undefined-behaviour
sanitizers when the compiler has their runtimes (nothing loaded into python is sanitised)."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tamp_amd_compress_resets", "tamp_amd_compress_resets_bound", "tamp_amd_compress_resets_slab",
               "tamp_amd_decompress_resets")


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_keyword_rules():
    """reset_interval without dictionary_reset=True is a ValueError, as reset_dictionary() on such an object; so is an interval
    that is no positive integer.  (Both are decided before the native library is looked for.)"""
    import tamp_amd

    for kwargs in ({}, dict(dictionary_reset=False), dict(window=12)):
        with pytest.raises(ValueError):
            tamp_amd.compress(b"abc", reset_interval=4096, **kwargs)
    for bad in (0, -1, 1.5, "4096", True):
        with pytest.raises(ValueError):
            tamp_amd.compress(b"abc", dictionary_reset=True, reset_interval=bad)
    with pytest.raises(ValueError):
        tamp_amd.compress(b"abc", dictionary_reset=True, reset_interval=16, window=16)


def test_command_line_option():
    from tamp_amd import cli

    args = cli.build_parser().parse_args(["compress", "--reset-interval", "65536", "-i", "x"])
    assert args.reset_interval == 65536
    assert cli.build_parser().parse_args(["compress", "-i", "x"]).reset_interval is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["decompress", "--reset-interval", "4096"])


def test_symbols_and_binding(lib):
    from tamp_amd import _lib

    header = open(os.path.join(ROOT, "include", "tamp_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(raw, name)
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in NEW_SYMBOLS:
            assert re.search(r" T %s$" % name, out, flags=re.M), name
    m = re.search(r"#define TAMP_AMD_RESETS_SCAN_TILE (\d+)", header)
    kernel = open(os.path.join(ROOT, "tamp_amd", "csrc", "tamp_reset_segments_kernel.hpp")).read()
    k = re.search(r"constexpr uint32_t kResetScanTile = (\d+);", kernel)
    assert m and k and int(m[1]) == int(k[1]) == _lib.RESETS_SCAN_TILE


def test_bound_against_the_checkers_sizes(lib, oracle):
    """The bound holds for what the checker's object writes on random bytes at intervals 1..17 (and 1000, 4096), and is exact for
    the empty input.  Without the reference build the oracle's object stands in."""
    from oracle.checker import Ref

    checker = Ref() if Ref.available() else oracle
    rng = random.Random(11)
    assert lib.tamp_amd_compress_resets_bound(0, 4096, 8) == 2
    assert lib.tamp_amd_compress_resets_bound(100, 0, 8) == 0 and lib.tamp_amd_compress_resets_slab(100, 0, 8) == 0
    for interval in list(range(1, 18)) + [1000, 4096]:
        for literal in (8, 7, 5):
            for n in (0, 1, interval, 3 * interval, 7 * interval + interval // 2 + 1):
                data = bytes(rng.randrange(1 << literal) for _ in range(n))
                ops = []
                for at in range(0, max(n, 1), interval):
                    ops += ([("reset",)] if at else []) + [("write", data[at : at + interval])]
                res, blob = checker.stream_script(ops + [("flush", False)], literal=literal, dictionary_reset=True)
                assert res == 0
                bound = lib.tamp_amd_compress_resets_bound(n, interval, literal)
                assert len(blob) <= bound, (interval, literal, n)
                assert lib.tamp_amd_compress_resets_slab(n, interval, literal) == 2 + (min(interval, max(n, 1)) * (literal + 1) + 16) // 8


PROGRAM = r"""
#include "tamp_reset_segments.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace tamp_amd;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// one call's table, built the way the launcher builds it: slices of `slice` segments, rows by the rows kernel's arithmetic
static void table(uint64_t total, uint32_t interval, uint32_t literal, uint64_t slice) {
    const uint64_t K = reset_segment_count(total, interval);
    const uint32_t slab = reset_slab_bytes(total, interval, literal);
    CHECK(K >= 1 && (total == 0 ? K == 1 : (K - 1) * (uint64_t)interval < total && total <= K * (uint64_t)interval), "K %llu", (unsigned long long)K);
    uint64_t covered = 0, bound = 0, rows = 0;
    for (uint64_t k0 = 0; k0 < K; k0 += slice) {
        const uint64_t cnt = K - k0 < slice ? K - k0 : slice;
        std::vector<uint64_t> in_off(cnt), out_off(cnt);  // (sized exactly: a row behind the slice is an address error)
        std::vector<uint32_t> in_len(cnt), out_cap(cnt);
        for (uint64_t i = 0; i < cnt; i++) {
            in_off[i] = reset_segment_start(k0 + i, interval), in_len[i] = reset_segment_len(k0 + i, interval, total);
            out_off[i] = i * slab, out_cap[i] = slab;
        }
        for (uint64_t i = 0; i < cnt; i++, rows++) {
            const bool last = k0 + i == K - 1;
            CHECK(in_off[i] == covered, "segment %llu starts at %llu, %llu covered", (unsigned long long)(k0 + i), (unsigned long long)in_off[i], (unsigned long long)covered);
            CHECK(in_len[i] <= interval && (last || in_len[i] == interval) && (total == 0 || in_len[i] >= 1), "segment %llu: %u bytes", (unsigned long long)(k0 + i), in_len[i]);
            const uint64_t need = reset_segment_bound(in_len[i], literal, !last);
            CHECK(need <= out_cap[i] || out_cap[i] == 0xFFFFFFFFu, "segment %llu: bound %llu, slab %u", (unsigned long long)(k0 + i), (unsigned long long)need, out_cap[i]);
            CHECK(i == 0 || out_off[i] == out_off[i - 1] + out_cap[i - 1], "slabs do not tile");
            covered += in_len[i], bound += need;
        }
    }
    CHECK(rows == K && covered == total, "%llu rows, %llu bytes", (unsigned long long)rows, (unsigned long long)covered);
    CHECK(bound == reset_stream_bound(total, interval, literal), "bound %llu", (unsigned long long)bound);
}

int main() {
    long tables = 0;
    const uint32_t intervals[] = {1, 2, 15, 16, 17, 100, 1000, 4096, 65536};
    for (uint32_t interval : intervals)
        for (uint32_t literal = 5; literal <= 8; literal++)
            for (uint64_t total : {0ull, 1ull, 2ull, 15ull, 16ull, 17ull, 1023ull, 1024ull, 1025ull, 4095ull, 4096ull, 4097ull, 70000ull})
                for (uint64_t slice : {1ull, 7ull, 1024ull, 1ull << 20}) {
                    if (total / interval > 5000) continue;
                    table(total, interval, literal, slice);
                    tables++;
                }
    // the ends of the 32-bit range: arithmetic only (no rows)
    static_assert(reset_segment_count(0xFFFFFFFFull, 1) == 0xFFFFFFFFull && reset_segment_count(0xFFFFFFFFull, 0xFFFFFFFFu) == 1, "count");
    static_assert(reset_segment_len(0xFFFFFFFEull, 1, 0xFFFFFFFFull) == 1 && reset_segment_len(0, 0xFFFFFFFFu, 0xFFFFFFFFull) == 0xFFFFFFFFu, "len");
    static_assert(reset_slab_bytes(0xFFFFFFFFull, 0xFFFFFFFFu, 8) == 0xFFFFFFFFu, "a slab is capped at what a table row can say");
    static_assert(reset_slab_bytes(0xFFFFFFFFull, 65536, 8) == 2 + (65536 * 9 + 16) / 8 && reset_slab_bytes(0, 65536, 8) == 2 + 25 / 8, "slab");
    static_assert(reset_stream_bound(0, 4096, 8) == 2 && reset_stream_bound(0xFFFFFFFFull, 1, 8) == 0xFFFFFFFEull * 5 + 4, "bound");
    table(0xFFFFFFFFull, 0xFFFFFFFFu, 8, 1), table(0xFFFFFFFFull, 0x80000000u, 5, 1ull << 20), tables += 2;
    printf("%s: %ld tables, %d failures\n", failures ? "FAILED" : "ok", tables, failures);
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("reset_segments")
    (d / "segments.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), str(d / "segments.cpp"), "-o", str(d / "segments")]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizers' runtimes)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "segments"), sanitized


def test_segment_table_arithmetic(program):
    exe, sanitized = program
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr, "(host ASan + UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert re.match(r"ok: \d+ tables, 0 failures", p.stdout), p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


# ---- the host merge of the reset finder's chunk reports (tamp_reset_merge.hpp) ----

MERGE_PROGRAM = r"""
#include "tamp_reset_merge.hpp"
#include <cstdio>
#include <vector>
using namespace tamp_amd;

// stdin: cases; per case "n header_bytes chunks", then per chunk "flags first_end n_inner i0 i1 i2 i3"
// stdout: per case "decline", or "ok" + the boundaries, and "segments" + start:len pairs
int main() {
    unsigned cases = 0;
    if (scanf("%u", &cases) != 1) return 2;
    for (unsigned c = 0; c < cases; c++) {
        unsigned n, hs, chunks;
        if (scanf("%u %u %u", &n, &hs, &chunks) != 3) return 2;
        std::vector<ResetChunkReport> rep(chunks);  // (sized exactly: a report behind the last chunk is an address error)
        for (unsigned i = 0; i < chunks; i++) {
            ResetChunkReport& r = rep[i];
            if (scanf("%u %u %u %u %u %u %u", &r.flags, &r.first_end, &r.n_inner, &r.inner[0], &r.inner[1], &r.inner[2], &r.inner[3]) != 7) return 2;
            r.reserved = 0;
        }
        std::vector<uint32_t> b, start, len;
        if (!reset_merge(rep.data(), rep.size(), b)) { printf("decline\n"); continue; }
        printf("ok");
        for (uint32_t x : b) printf(" %u", x);
        printf("\n");
        if (!reset_segments_of(b, hs, n, start, len)) { printf("bad positions\n"); continue; }
        printf("segments");
        for (size_t k = 0; k < start.size(); k++) printf(" %u:%u", start[k], len[k]);
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def merge_program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("reset_merge")
    (d / "merge.cpp").write_text(MERGE_PROGRAM)
    base = [hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"), str(d / "merge.cpp"),
            "-o", str(d / "merge")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizers' runtimes)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "merge"), sanitized


def chunk_reports(blob):
    """What tamp_reset_find_kernel reports for ``blob``, from the token writer's reader: per chunk of the compressed bits the
    tokens that START in it.  -> (header bytes, report rows, the boundaries a walk over ALL tokens in order finds)"""
    import long_stream_writer as lsw

    extended = bool(blob[0] & 2)
    cb = lsw.CHUNK_BITS_EXT if extended else lsw.CHUNK_BITS_V1
    tokens = lsw.read_tokens(blob)[0]
    chunks = (8 * len(blob) + cb - 1) // cb
    rows = [[0, 0, 0, 0, 0, 0, 0] for _ in range(chunks)]
    seen = [None] * chunks  # kind of the chunk's previous token
    boundaries, prev = [], None
    for tk in tokens:
        i, end, flush = tk.bit // cb, (tk.bit + tk.nbits) // 8, tk.kind == "F"
        if flush and prev == "F":
            boundaries.append(end)
        prev = tk.kind
        r = rows[i]
        if not r[0] & 1:
            r[0] |= 1 | (2 if flush else 0)
            r[1] = end
        elif flush and seen[i] == "F":
            if r[2] < 4:
                r[3 + r[2]] = end
            r[2] += 1
        seen[i] = tk.kind
        r[0] = (r[0] & ~4) | (4 if flush else 0)
    return 1 + (blob[0] & 1), rows, boundaries


def test_host_merge_of_chunk_reports(merge_program, oracle):
    """Reports generated from the checker's blobs (resets every 1 .. 4096 bytes, two resets in a row, both formats) and from
    token-writer streams (a FLUSH pair split across a chunk boundary, four and seven FLUSH tokens in a row): the boundaries are those
    of a walk over all tokens in order, the segments tile the stream, and every segment behind the header decodes alone to its
    share of the plain text."""
    import random as rnd

    import long_stream_writer as lsw
    from oracle.checker import Ref

    from tamp_amd import workloads as wl

    checker = Ref() if Ref.available() else oracle
    prose = wl.frozen_corpus("prose")
    blobs = []
    for extended in (True, False):
        for interval, n in ((1, 40), (17, 680), (150, 450), (1000, 39_997), (4096, 3000)):
            data = prose[7000 : 7000 + n]
            ops = []
            for at in range(0, max(n, 1), interval):
                ops += ([("reset",)] if at else []) + [("write", data[at : at + interval])]
            res, blob = checker.stream_script(ops + [("flush", False)], extended=extended, dictionary_reset=True)
            assert res == 0
            blobs.append(blob)
        res, blob = checker.stream_script([("write", prose[:900]), ("reset",), ("reset",), ("write", prose[900:1500]), ("flush", False)],
                                          extended=extended, dictionary_reset=True)
        blobs.append(blob)
        for flushes in (2, 4, 7):
            w = lsw.TokenWriter(10, 8, extended, more=0)
            rng = rnd.Random(flushes)
            w.fill_to(3 * w.chunk_bits - 9, rng)  # (the first FLUSH ends chunk 2 exactly, the next one starts chunk 3)
            for _ in range(flushes):
                w.flush()
            w.plain_until(5 * w.chunk_bits, rng)
            blobs.append(w.blob())
    cases = [chunk_reports(b) for b in blobs]
    text = [str(len(cases))]
    for blob, (hs, rows, _) in zip(blobs, cases):
        text.append(f"{len(blob)} {hs} {len(rows)}")
        text += [" ".join(map(str, r)) for r in rows]
    exe, sanitized = merge_program
    p = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
    print(p.stderr, "(host ASan + UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    lines = iter(p.stdout.splitlines())
    declined = 0
    for blob, (hs, rows, boundaries) in zip(blobs, cases):
        head = next(lines).split()
        if max(r[2] for r in rows) > 4:
            assert head == ["decline"]
            declined += 1
            continue
        assert head[0] == "ok" and [int(x) for x in head[1:]] == boundaries
        segs = [tuple(map(int, s.split(":"))) for s in next(lines).split()[1:]]
        assert len(segs) == len(boundaries) + 1 and segs[0][0] == hs and segs[-1][0] + segs[-1][1] == len(blob)
        assert all(a[0] + a[1] == b[0] for a, b in zip(segs, segs[1:]))
        whole = checker.decompress(blob, cap=64 + 256 * len(blob))
        parts = [checker.decompress(blob[:hs] + blob[s : s + ln], cap=64 + 256 * len(blob)) for s, ln in segs]
        assert whole[0] == 2 and all(r[0] == 2 and r[2] == hs + ln for r, (s, ln) in zip(parts, segs))
        assert b"".join(r[1] for r in parts) == whole[1]
    # (a reset every byte or every 17 bytes puts more than four into one chunk as well)
    assert declined == sum(max(r[2] for r in rows) > 4 for _, rows, _ in cases) and 2 <= declined <= len(cases) - 8
