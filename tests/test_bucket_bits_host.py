"""CPU tier: the bucket scan's candidate arithmetic in bit units (tamp_amd/csrc/tamp_common.hpp: first_set_or_ones, scan_is_deep,
scan_shallow_bits, scan_deep_bits, scan_bits_len, scan_bits_hit16), compiled for the HOST into a stand-alone program (its own main,
no GPU call) and checked there against the byte-wise rules it replaces in the fixed-geometry compress builds:

  shallow   exhaustive over the 2^14 values of the entry's low bits (byte 2's XOR in bits 0..7, six bits of byte 3's above), under
            four distances: a candidate is deep iff they are all zero, else 2 bytes long iff byte 2 differs, else 3; no 16-byte hit;
  deep      every first difference -- byte 0..15 at each of its 8 bits, and none -- with nothing, everything and seeded noise
            behind it: the capped bit offset is 8 * byte + bit (128 for none), the length the byte, a 16-byte hit iff none.

Built with the host's undefined-behaviour sanitizer when the compiler has its runtime, and without it otherwise.
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
using namespace tamp_amd;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

int main() {
    constexpr uint32_t LB = 14;
    CHECK(first_set_or_ones(0) == 0xFFFFFFFFu && first_set_or_ones(1) == 0 && first_set_or_ones(0x80000000u) == 31, "first set bit");
    long shallow = 0, deep_entries = 0;
    const uint32_t dists[4] = {0u, 1u, 0x155u, 1022u};
    for (uint32_t d : dists)
        for (uint32_t low = 0; low < (1u << LB); low++) {
            const uint32_t y = (d << LB) | low;
            const uint32_t fb = first_set_or_ones(y);
            CHECK(scan_is_deep<LB>(fb) == (low == 0), "d %u low %04x", d, low);
            if (low == 0) { deep_entries++; continue; }
            const uint32_t bits = scan_shallow_bits(fb);
            CHECK(bits >= 16 && bits < 16 + LB, "d %u low %04x bits %u", d, low, bits);
            CHECK(scan_bits_len(bits) == ((low & 0xFFu) ? 2u : 3u), "d %u low %04x len %u", d, low, scan_bits_len(bits));
            CHECK(scan_bits_hit16(bits) == 0, "d %u low %04x", d, low);
            shallow++;
        }
    // the byte-wise compare of 16 candidate bytes against 16 pattern bytes
    long deep = 0;
    for (uint32_t byte = 0; byte <= 16; byte++)
        for (uint32_t bit = 0; bit < 8; bit++)
            for (int noise = 0; noise < 6; noise++) {  // behind the first difference: nothing, everything, seeded noise
                uint8_t pat[16], cand[16];
                for (int k = 0; k < 16; k++) pat[k] = (uint8_t)rnd(), cand[k] = pat[k];
                if (byte < 16) {
                    const uint8_t above = (uint8_t)(0xFFu << bit << 1);
                    cand[byte] ^= (uint8_t)((1u << bit) | (noise == 0 ? 0u : noise == 1 ? above : (rnd() & above)));
                    for (uint32_t k = byte + 1; k < 16; k++) cand[k] ^= (uint8_t)(noise == 0 ? 0u : noise == 1 ? 0xFFu : rnd());
                }
                uint32_t n = 0;
                while (n < 16 && cand[n] == pat[n]) n++;
                CHECK(n == byte, "the design: byte %u", byte);
                uint32_t p[4], c[4];
                memcpy(p, pat, 16), memcpy(c, cand, 16);  // little-endian dwords, as the kernel loads them
                const uint32_t bits = scan_deep_bits(c[0] ^ p[0], c[1] ^ p[1], c[2] ^ p[2], c[3] ^ p[3]);
                CHECK(bits == (byte < 16 ? 8 * byte + bit : kScanBitsCap), "byte %u bit %u noise %d: bits %u", byte, bit, noise, bits);
                CHECK(bits == scan_deep_bits(c[0] ^ p[0], c[1] ^ p[1], c[2] ^ p[2], c[3] ^ p[3], kScanBitsCap), "the cap handed over");
                CHECK(scan_bits_len(bits) == n, "byte %u bit %u noise %d: len %u", byte, bit, noise, scan_bits_len(bits));
                CHECK(scan_bits_hit16(bits) == (n == 16 ? 1u : 0u), "byte %u bit %u noise %d", byte, bit, noise);
                deep++;
            }
    printf("%s: %ld shallow values, %ld deep entries, %ld compares, %d failures\n", failures ? "FAILED" : "ok", shallow, deep_entries, deep, failures);
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("bucket_bits")
    (d / "bits.cpp").write_text(PROGRAM)
    base = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "tamp_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), str(d / "bits.cpp"), "-o", str(d / "bits")]
    sanitize = ["-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + sanitize, capture_output=True, text=True, timeout=600)
    sanitized = p.returncode == 0
    if not sanitized:  # (a toolchain without the sanitizer's runtime)
        p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(d / "bits"), sanitized


def test_scan_bits_against_the_bytewise_rules(program):
    exe, sanitized = program
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr, "(host UBSan: %s)" % ("on" if sanitized else "off"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.startswith("ok: %d shallow values, 4 deep entries, %d compares, 0 failures" % (4 * (2 ** 14 - 1), 17 * 8 * 6)), p.stdout
    assert "runtime error" not in p.stderr
