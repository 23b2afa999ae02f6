"""CPU tier: static figures of the fixed-geometry compress builds after the work on the code around their bucket scan (pattern
loads from one aligned base, the histogram pass by full quads, constant-trip loops as straight-line stores), from a cross-compile
of the device code the way tests/test_fixed_build_static.py makes one (plus line tables, which change no instruction).

The parent's figures are those of profiles/query_setup_static.txt, rows "parent": vector ALU instructions as tools/isa_classes.py
counts them (everything starting v_ except v_readlane / v_writelane, fast + slow) and spilled SGPRs.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_HPP = os.path.join(ROOT, "tamp_amd", "csrc", "tamp_compress_kernel.hpp")

# profiles/query_setup_static.txt, the parent commit's build: (VALU, spilled SGPRs) of the extended and the v1 kernel
PARENT = {"ext": (2704, 22), "v1": (1888, 6)}


@pytest.fixture(scope="module")
def device_code(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("qsetup") / "dev.s"
    flags = None
    for line in open(os.path.join(ROOT, "tamp_amd", "csrc", "Makefile")):
        m = re.match(r"HIPFLAGS \?= (.*)", line)
        if m:
            flags = m.group(1).replace("$(ARCH)", "gfx950").split()
    assert flags, "HIPFLAGS of the library's Makefile"
    p = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-gline-tables-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                                          "tamp_capi.hip", "-o", str(out)],
                       cwd=os.path.join(ROOT, "tamp_amd", "csrc"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    remarks = {}
    for b in re.split(r"remark: Function Name: ", p.stderr)[1:]:
        name = b.split()[0]
        remarks[name] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", b)}
    asm = out.read_text()
    files = {int(n): os.path.basename(f) for n, f in re.findall(r'\n\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]*)"', asm)}
    parts = re.split(r"\n(_ZN[^\n:]*):[^\n]*\n", asm)
    bodies = {parts[i]: parts[i + 1].split(".end_amdhsa_kernel")[0] for i in range(1, len(parts) - 1, 2)}
    names = sorted(n for n in bodies if "tamp_compress_fixed" in n)
    assert len(names) == 2 and names == sorted(n for n in remarks if "tamp_compress_fixed" in n), names
    return remarks, bodies, files, dict(zip(("ext", "v1"), names))  # FIX = 1 (extended format), FIX = 2 (v1)


def located(body, files):
    """[(source file, line, instruction)] of a kernel body: every instruction with the last .loc in front of it."""
    out, cur = [], (None, 0)
    for ln in body.split("\n"):
        s = ln.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            cur = (files.get(int(m.group(1))), int(m.group(2)))
        elif ln.startswith("\t") and s and s[0] not in ".;":
            out.append((cur[0], cur[1], s.split(";")[0].strip()))
    return out


def valu(ins):
    return sum(i.startswith("v_") and not i.startswith(("v_readlane", "v_writelane")) for _, _, i in ins)


@pytest.mark.parametrize("which", ["ext", "v1"])
def test_fewer_vector_instructions_than_the_parent(device_code, which):
    remarks, bodies, files, names = device_code
    ins = located(bodies[names[which]], files)
    got = valu(ins)
    print("fixed %s kernel: %d VALU instructions (parent %d), %d in all" % (which, got, PARENT[which][0], len(ins)))
    assert got < PARENT[which][0]


@pytest.mark.parametrize("which", ["ext", "v1"])
def test_registers_spills_occupancy(device_code, which):
    remarks, bodies, files, names = device_code
    r = remarks[names[which]]
    assert r["VGPRs"] <= 64 and r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["Occupancy"] == 8, r
    assert r["SGPRs Spill"] <= PARENT[which][1], r
    assert not any(i.startswith(("flat_", "scratch_")) for _, _, i in located(bodies[names[which]], files))


LDS_DWORDS = {"ds_read_b32": 1, "ds_read2_b32": 2, "ds_read_b64": 2, "ds_read2_b64": 4, "ds_read_b96": 3, "ds_read_b128": 4}


def test_the_query_setup_loads_its_pattern_as_five_dwords(device_code):
    """Between the query's number (`q = sorted[j]`, the match phase's first line) and the byte in front of the pattern (`prevb`)
    the extended kernel reads the 16 pattern bytes, and nothing else, through the helpers of tamp_common.hpp: five dwords at the
    most (one aligned base), where four separate unaligned loads read eight."""
    remarks, bodies, files, names = device_code
    src = open(KERNEL_HPP).read().split("\n")
    first = next(i + 1 for i, ln in enumerate(src) if "const uint32_t q = sorted[j];" in ln)
    last = next(i + 1 for i, ln in enumerate(src) if i + 1 > first and "const uint32_t prevb = ebuf[W + q - 1];" in ln)
    ins = located(bodies[names["ext"]], files)
    at = [k for k, (f, ln, _) in enumerate(ins) if f == "tamp_compress_kernel.hpp" and ln == first]
    assert at, "the match loop's first line has instructions of its own"
    end = next(k for k, (f, ln, i) in enumerate(ins) if k > at[0] and f == "tamp_compress_kernel.hpp" and ln == last and i.startswith("ds_read_u8"))
    reads = [(f, i) for f, _, i in ins[at[0]:end] if i.split()[0] in LDS_DWORDS]
    assert all(f == "tamp_common.hpp" for f, _ in reads), reads
    dwords = sum(LDS_DWORDS[i.split()[0]] for _, i in reads)
    print("pattern load of the query set-up:", [i for _, i in reads])
    assert 4 <= dwords <= 5, reads
