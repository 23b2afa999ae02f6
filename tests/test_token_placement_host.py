"""CPU tier: token_words of tamp_amd/csrc/tamp_common.hpp, compiled for the HOST into a stand-alone program (its own main,
no GPU call) and checked there against a bit-by-bit MSb-first writer.

The emit phase of the compress kernel ORs every token straight to its place with token_words: one 64-bit shift by
64 - phase - bits, which must stay in 1..63 for every phase 0..31 and every width 1..32.  The program is built with the
host's undefined-behaviour sanitizer when the compiler has its runtime (a shift count out of range aborts the run) and
without it otherwise; the comparisons are the same.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "tamp_common.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace tamp_amd;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the reference's bit sink, one bit at a time: bit k of the stream is bit 7 - (k & 7) of byte k >> 3
static void write_bits(std::vector<uint8_t>& buf, uint64_t bitpos, uint32_t v, uint32_t nb) {
    for (uint32_t i = nb; i-- > 0; bitpos++)
        if ((v >> i) & 1u) buf[bitpos >> 3] |= (uint8_t)(0x80u >> (bitpos & 7));
}
static void place(std::vector<uint32_t>& words, uint32_t bitpos, uint32_t v, uint32_t nb) {
    uint32_t wi, w_hi, w_lo;
    token_words(v, nb, bitpos, &wi, &w_hi, &w_lo);
    const uint32_t ph = bitpos & 31u;
    CHECK(wi == bitpos >> 5, "bitpos %u", bitpos);
    CHECK((w_lo != 0) <= (ph + nb > 32), "ph %u nb %u v %08x: second word without a crossing", ph, nb, v);
    words[wi] |= w_hi;
    if (w_lo) words[wi + 1] |= w_lo;
}
static bool same(const std::vector<uint32_t>& words, const std::vector<uint8_t>& bytes) {
    return words.size() * 4 == bytes.size() && memcmp(words.data(), bytes.data(), bytes.size()) == 0;
}
static uint64_t rng_state;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

int main() {
    // every phase x every width x four bit patterns, one token behind a guard word and in front of two
    long singles = 0;
    for (uint32_t ph = 0; ph < 32; ph++)
        for (uint32_t nb = 1; nb <= 32; nb++) {
            const uint32_t ones = nb == 32 ? 0xFFFFFFFFu : (1u << nb) - 1u;
            const uint32_t vals[4] = {ones, 1u << (nb - 1), 1u, 0xAAAAAAAAu & ones};
            for (uint32_t v : vals) {
                std::vector<uint32_t> words(4, 0u);
                std::vector<uint8_t> bytes(16, 0);
                place(words, 32 + ph, v, nb);
                write_bits(bytes, 32 + ph, v, nb);
                CHECK(same(words, bytes), "ph %u nb %u v %08x", ph, nb, v);
                singles++;
            }
        }
    // seeded sequences into a zeroed buffer with guard words on both sides
    long tokens = 0;
    for (uint32_t seed = 1; seed <= 20; seed++) {
        rng_state = 0x9E3779B97F4A7C15ull * seed;
        const uint32_t guard = 2, nwords = guard + 1 + 1000 + guard;  // 1,000 tokens of <= 32 bits behind a phase of <= 31
        std::vector<uint32_t> words(nwords, 0u);
        std::vector<uint8_t> bytes(nwords * 4, 0);
        uint32_t bitpos = 32 * guard + rnd() % 32;
        const uint32_t first = bitpos;
        for (int k = 0; k < 1000; k++) {
            const uint32_t nb = 1 + rnd() % 32;
            const uint32_t v = rnd() & (nb == 32 ? 0xFFFFFFFFu : (1u << nb) - 1u);
            place(words, bitpos, v, nb);
            write_bits(bytes, bitpos, v, nb);
            bitpos += nb;
            tokens++;
        }
        CHECK(same(words, bytes), "seed %u", seed);
        for (uint32_t w = 0; w < nwords; w++)
            if (w < (first >> 5) || w > ((bitpos - 1) >> 5)) CHECK(words[w] == 0, "seed %u: word %u outside the written range", seed, w);
    }
    static_assert(kMaxTokenBits == 32, "7 + 11 + 14: the settled extended-match token at window 2^14");
    printf("%s: %ld single tokens, %ld tokens in sequences, %d failures\n", failures ? "FAILED" : "ok", singles, tokens, failures);
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("placement")
    (d / "placement.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), str(d / "placement.cpp"), "-o", str(d / "placement")]
    sanitize = ["-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizer's runtime)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "placement"), sanitized


def test_token_words_against_a_bitwise_writer(program):
    exe, sanitized = program
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr, "(host UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.startswith("ok: 4096 single tokens, 20000 tokens in sequences, 0 failures"), p.stdout
    assert "runtime error" not in p.stderr
