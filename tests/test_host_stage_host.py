"""CPU tier: the staging arithmetic of the host-memory calls (tamp_host_stage.hpp) -- the table carver on the nine layouts the calls
take from it, the extent of a batch's rows with rebased offsets, and the running sum of dense output slabs -- compiled for the HOST
into a stand-alone program with the address and undefined-behaviour sanitizers when the compiler has their runtimes (nothing loaded
into python is sanitised)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "tamp_host_stage.hpp"
#include <cstdio>
#include <cstring>
using namespace tamp_amd;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)
typedef unsigned long long ull;

struct Unit40 {  // (the unit row of tamp_batch_read_ranges_seek: three 8-byte and four 4-byte fields)
    uint64_t a, b, c;
    uint32_t d, e, f, g;
};
static_assert(sizeof(Unit40) == 40 && alignof(Unit40) == 8, "the unit row");

// One layout: its takes in order, each checked as it is taken, then all of them against each other and against bytes(), then
// every table written through its pointer into a buffer of exactly bytes() (a store outside it is an address error).
struct Layout {
    const char* name;
    TableCarver c;
    struct Span { size_t at, bytes; };
    std::vector<Span> spans;
    explicit Layout(const char* n) : name(n) {}
    template <class T>
    void take(size_t count, size_t align = alignof(T)) {
        const size_t before = c.used;
        const Carved<T> t = c.take<T>(count, align);
        CHECK(t.at % alignof(T) == 0 && t.at % align == 0, "%s: table %zu at %zu", name, spans.size(), t.at);
        CHECK(t.at >= before && t.at < before + align, "%s: table %zu at %zu behind %zu", name, spans.size(), t.at, before);
        CHECK(c.used == (count ? t.at + count * sizeof(T) : before), "%s: table %zu of %zu elements leaves %zu used", name, spans.size(), count, c.used);
        spans.push_back({t.at, count * sizeof(T)});
    }
    void done() {
        CHECK(c.bytes() == c.used + 64, "%s: %zu bytes for %zu used", name, c.bytes(), c.used);
        for (size_t i = 0; i < spans.size(); i++) {
            // (in front of the slack; a table of no elements may point into it, and is never read)
            CHECK(spans[i].at + spans[i].bytes <= (spans[i].bytes ? c.used : c.bytes()), "%s: table %zu ends at %zu of %zu", name, i, spans[i].at + spans[i].bytes, c.bytes());
            for (size_t j = 0; j < i; j++)
                CHECK(!spans[i].bytes || !spans[j].bytes || spans[j].at + spans[j].bytes <= spans[i].at, "%s: tables %zu and %zu overlap", name, j, i);
        }
        std::vector<uint8_t> buf(c.bytes(), 0);
        for (size_t i = 0; i < spans.size(); i++)
            if (spans[i].bytes) memset(Carved<uint8_t>{spans[i].at}.in(buf.data()), (int)(i + 1), spans[i].bytes);
        for (size_t i = 0; i < spans.size(); i++)
            for (size_t b = 0; b < spans[i].bytes; b++)
                if (buf[spans[i].at + b] != i + 1) { CHECK(false, "%s: byte %zu of table %zu overwritten", name, b, i); break; }
    }
};

// The nine layouts, as the calls take them (n streams or objects, nw writes or ranges or units, C index entries).
static int layouts(size_t n, size_t nw, size_t C) {
    int count = 0;
    for (int with_index = 0; with_index < 2; with_index++) {  // batch_compress_resets: meta
        Layout l("compress_resets");
        l.take<uint64_t>(n), l.take<uint64_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<int8_t>(n);
        l.take<uint32_t>(with_index ? C : 0);
        l.done(), count++;
    }
    {  // batch_decompress_resets: meta
        Layout l("decompress_resets");
        l.take<uint64_t>(n), l.take<uint64_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(n);
        l.take<uint64_t>(n + 1), l.take<uint32_t>(C), l.take<int8_t>(n);
        l.done(), count++;
    }
    {  // read_ranges_host: meta (nw ranges)
        Layout l("read_ranges");
        l.take<uint64_t>(nw), l.take<uint64_t>(nw), l.take<uint32_t>(nw), l.take<uint32_t>(nw), l.take<int8_t>(nw);
        l.done(), count++;
    }
    {  // batch_write_ranges: meta
        Layout l("write_ranges");
        l.take<uint64_t>(n), l.take<uint64_t>(n), l.take<uint64_t>(n + 1), l.take<uint64_t>(nw), l.take<uint64_t>(nw);
        l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(C), l.take<uint32_t>(C), l.take<uint32_t>(nw), l.take<uint32_t>(nw);
        l.take<int8_t>(n);
        l.done(), count++;
    }
    {  // batch_append: meta (C: the bound of the new entries)
        Layout l("append");
        l.take<uint64_t>(n), l.take<uint64_t>(n), l.take<uint64_t>(n + 1), l.take<uint64_t>(n), l.take<uint64_t>(n + 1);
        l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(C), l.take<int8_t>(n);
        l.done(), count++;
    }
    {  // index_resets_host: meta, out (C: the entries there is room for)
        Layout m("index_resets meta"), o("index_resets out");
        m.take<uint64_t>(n), m.take<uint32_t>(n);
        o.take<uint64_t>(n + 1), o.take<uint32_t>(C), o.take<uint32_t>(C), o.take<uint32_t>(n), o.take<int8_t>(n);
        m.done(), o.done(), count++;
    }
    {  // seek_index_host: meta, out (C rows of checkpoints)
        Layout m("seek_index meta"), o("seek_index out");
        m.take<uint64_t>(n), m.take<uint64_t>(n + 1), m.take<uint32_t>(n);
        o.take<uint32_t>(C), o.take<uint64_t>(n), o.take<int8_t>(n);
        m.done(), o.done(), count++;
    }
    for (size_t out_bytes : {(size_t)0, 4 * C, 4 * C + 4}) {  // read_seek_host: meta, out (nw units, n ranges, the ranges' padded bytes)
        Layout m("read_seek meta"), o("read_seek out");
        m.take<Unit40>(nw), m.take<uint64_t>(n);
        o.take<uint8_t>(out_bytes), o.take<uint32_t>(2 * n, 8);
        m.done(), o.done(), count++;
    }
    {  // run_host_pieces: meta (the ops rounded to 16)
        Layout l("pieces");
        l.take<uint64_t>(n), l.take<uint64_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<uint32_t>(n), l.take<int8_t>(n);
        l.take<uint8_t>(n, 16);
        l.done(), count++;
    }
    return count;
}

static void extent(const char* name, std::vector<uint64_t> off, std::vector<uint32_t> len, uint64_t lo, uint64_t hi, std::vector<uint64_t> want) {
    const HostExtent e(off.data(), len.data(), off.size());
    CHECK(e.lo == lo && e.hi == hi && e.bytes() == hi - lo, "%s: [%llu, %llu)", name, (ull)e.lo, (ull)e.hi);
    CHECK(e.off == want, "%s: the rebased offsets", name);
}

int main() {
    int count = 0;
    for (size_t n : {0, 1, 3})
        for (size_t nw : {0, 1, 3})
            for (size_t C : {0, 1, 3}) count += layouts(n, nw, C);
    {  // a table of no elements between two others: no room, and the next one aligned all the same
        TableCarver c;
        const auto a = c.take<int8_t>(3);
        const auto z = c.take<uint64_t>(0);
        CHECK(c.used == 3 && z.at % 8 == 0, "an empty table: %zu used, at %zu", c.used, z.at);
        const auto b = c.take<uint32_t>(2);
        CHECK(a.at == 0 && b.at == 4 && c.used == 12 && c.bytes() == 76, "behind it: at %zu, %zu used", b.at, c.used);
        uint32_t words[4] = {0, 0, 0, 0};
        CHECK(b.in(words) == words + 1, "the pointer of a table");
    }
    extent("reverse order", {200, 100, 0}, {10, 20, 30}, 0, 210, {200, 100, 0});
    extent("reverse order, from 50", {250, 150, 50}, {10, 20, 30}, 50, 260, {200, 100, 0});
    extent("an empty row between two", {40, 1000, 60}, {8, 0, 4}, 40, 64, {0, 0, 20});
    extent("an empty row in front of the others", {7, 40, 60}, {0, 8, 4}, 40, 64, {0, 0, 20});
    extent("all rows empty", {5, 900, 17}, {0, 0, 0}, 0, 0, {0, 0, 0});
    extent("no rows", {}, {}, 0, 0, {});
    extent("one row at a large offset", {0xFFFFFFFF00000000ull}, {0xFFFFFFFFu}, 0xFFFFFFFF00000000ull, 0xFFFFFFFFFFFFFFFFull, {0});
    extent("two rows beyond 2^32", {0x300000000ull, 0x100000000ull}, {16, 1}, 0x100000000ull, 0x300000010ull, {0x200000000ull, 0});
    {  // the form tamp_batch_write_ranges uses: the writes that land in a stream there is, and have bytes
        const uint64_t n = 2;
        const std::vector<uint32_t> stream = {0, 7, 1, 1, 2};
        const std::vector<uint64_t> src_off = {500, 3, 300, 900, 100};
        const std::vector<uint32_t> len = {10, 99, 5, 0, 50};
        const HostExtent e(src_off.data(), len.data(), len.size(), [&](size_t q) { return stream[q] < n; });
        CHECK(e.lo == 300 && e.hi == 510, "the kept writes: [%llu, %llu)", (ull)e.lo, (ull)e.hi);
        CHECK(e.off == (std::vector<uint64_t>{200, 0, 0, 0, 0}), "the kept writes' offsets");
        const HostExtent none(src_off.data(), len.data(), len.size(), [](size_t) { return false; });
        CHECK(none.lo == 0 && none.hi == 0 && none.off == std::vector<uint64_t>(5, 0), "no write kept");
    }
    {  // dense slabs: the running sum; a slab of no room takes none
        const std::vector<uint32_t> cap = {5, 0, 0, 7, 0xFFFFFFFFu, 0xFFFFFFFFu, 1};
        std::vector<uint64_t> off(cap.size(), 99);
        const uint64_t room = dense_slabs(cap.data(), cap.size(), off.data());
        CHECK(off == (std::vector<uint64_t>{0, 5, 5, 5, 12, 12 + 0xFFFFFFFFull, 12 + 2 * 0xFFFFFFFFull}), "the running sum");
        CHECK(room == 13 + 2 * 0xFFFFFFFFull, "%llu bytes of room", (ull)room);
        CHECK(dense_slabs(nullptr, 0, nullptr) == 0, "no slabs");
    }
    printf("%s: %d layouts, %d failures\n", failures ? "FAILED" : "ok", count, failures);
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("host_stage")
    (d / "stage.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "c++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            str(d / "stage.cpp"), "-o", str(d / "stage")]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizers' runtimes)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "stage"), sanitized


def test_staging_arithmetic(program):
    """The carver on the takes of all nine layouts for n, nw, C in {0, 1, 3}: every table aligned to its element type (and to what the
    caller asked for), no two overlapping, the last one ending inside bytes(), a table of no elements taking no room and leaving the
    next one aligned, every table writable through its pointer; HostExtent on rows in reverse order, an empty row between two others,
    empty rows alone, a row at a large offset and the predicate form of tamp_batch_write_ranges; dense slabs as the running sum."""
    exe, sanitized = program
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr, "(host ASan + UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    m = re.match(r"ok: (\d+) layouts, 0 failures", p.stdout)
    assert m and int(m[1]) == 27 * 12, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_header_has_no_hip_in_it():
    """It compiles with a plain host compiler: no HIP header, type or qualifier; and the extent is defined there alone."""
    csrc = os.path.join(ROOT, "tamp_amd", "csrc")
    text = open(os.path.join(csrc, "tamp_host_stage.hpp")).read()
    code = re.sub(r"//.*", "", text)
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", code)
    holders = [f for f in sorted(os.listdir(csrc)) if re.search(r"\bstruct HostExtent\b", open(os.path.join(csrc, f)).read())]
    assert holders == ["tamp_host_stage.hpp"]
