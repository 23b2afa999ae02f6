"""CPU tier: static figures of the fixed-geometry compress builds' bucket scan after its candidate lengths moved to bit units
(kBitLen), from a cross-compile of the device code the way tests/test_query_setup_static.py makes one.

The parent's figures are those of profiles/bucket_bits_static.txt, rows "parent": vector ALU instructions as tools/isa_classes.py
counts them (everything starting v_ except v_readlane / v_writelane), of the whole kernel and of the scan loop, and spilled SGPRs.
The scan loop: the block of instructions from the first to the last one attributed to the lines of the `while (pe < pe_end)` loop of
the kEntV2 scan, helpers inlined between them included (the 16-byte compare, the bit arithmetic of tamp_common.hpp, min / max), the
query set-up and the code behind the loop that the scheduler moves between them (lines from `q = sorted[j]` up to the loop, and
lines behind it) left out: one lock-step iteration, the loop's entry test and the two instructions of its wrap-zone branch.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "tamp_compress_kernel.hpp"
KERNEL_HPP = os.path.join(ROOT, "tamp_amd", "csrc", KERNEL)

# profiles/bucket_bits_static.txt, the parent commit's build: (whole-kernel VALU, scan-loop VALU) of the extended and the v1 kernel
PARENT = {"ext": (2666, 40), "v1": (1853, 40)}
SPILLED_SGPRS = {"ext": 20, "v1": 4}


@pytest.fixture(scope="module")
def device_code(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("bucket_loop") / "dev.s"
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


def is_valu(i):
    return i.startswith("v_") and not i.startswith(("v_readlane", "v_writelane"))


def scan_loop(ins):
    """The scan loop's instructions (see the module's docstring)."""
    src = open(KERNEL_HPP).read().split("\n")
    setup = next(i + 1 for i, ln in enumerate(src) if "const uint32_t q = sorted[j];" in ln)
    first = next(i + 1 for i, ln in enumerate(src) if "while (pe < pe_end) {" in ln)
    last = next(i + 1 for i, ln in enumerate(src) if i + 1 > first and "}  // TAMP_REPEAT" in ln) - 1
    at = [k for k, (f, ln, _) in enumerate(ins) if f == KERNEL and first <= ln <= last]
    assert at, "the loop's lines have instructions of their own"
    return [(f, ln, i) for f, ln, i in ins[at[0]:at[-1] + 1] if not (f == KERNEL and (setup <= ln < first or ln > last))]


@pytest.mark.parametrize("which", ["ext", "v1"])
def test_the_scan_loop_issues_fewer_vector_instructions(device_code, which):
    remarks, bodies, files, names = device_code
    ins = located(bodies[names[which]], files)
    loop = scan_loop(ins)
    got, whole = sum(is_valu(i) for _, _, i in loop), sum(is_valu(i) for _, _, i in ins)
    print("fixed %s kernel: scan loop %d VALU (parent %d), whole kernel %d (parent %d)" % (which, got, PARENT[which][1], whole, PARENT[which][0]))
    assert got <= PARENT[which][1] - 2
    assert whole < PARENT[which][0]
    # the class from one first-set-bit of y, the cap inside the second three-way minimum, no sub-dword compare and no select
    ops = [i.split()[0] for _, _, i in loop]
    assert ops.count("v_ffbl_b32") == 5 and ops.count("v_min3_u32") == 3, ops
    assert not any(o.endswith("_sdwa") or o.startswith("v_cndmask") for o in ops), ops


@pytest.mark.parametrize("which", ["ext", "v1"])
def test_registers_spills_occupancy(device_code, which):
    remarks, bodies, files, names = device_code
    r = remarks[names[which]]
    assert r["VGPRs"] <= 64 and r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["Occupancy"] == 8, r
    assert r["SGPRs Spill"] <= SPILLED_SGPRS[which], r
    assert not any(i.startswith(("flat_", "scratch_")) for _, _, i in located(bodies[names[which]], files))
