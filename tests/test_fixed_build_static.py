"""CPU tier: static properties of the fixed-geometry compress builds (tamp_compress_fixed::compress_kernel<FIX>), from a
cross-compile of the device code (hipcc needs no GPU): registers, spills, occupancy, and what must not be in their ISA.

The bounds are those of the generic headline build they replace (profiles/r6_kernel_resource_usage.txt, profiles/
r6_bucket_loop_isa_classes.txt): 64 VGPRs at eight waves per SIMD with nothing in scratch, fewer than its 135 spilled SGPRs
and fewer than its 360 v_readlane / v_writelane.  profiles/fixed_build_static.txt has the figures of the build as committed.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def device_code(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("fixed") / "dev.s"
    flags = None
    for line in open(os.path.join(ROOT, "tamp_amd", "csrc", "Makefile")):
        m = re.match(r"HIPFLAGS \?= (.*)", line)
        if m:
            flags = m.group(1).replace("$(ARCH)", "gfx950").split()
    assert flags, "HIPFLAGS of the library's Makefile"
    p = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", "tamp_capi.hip", "-o", str(out)],
                       cwd=os.path.join(ROOT, "tamp_amd", "csrc"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    remarks = {}
    for b in re.split(r"remark: Function Name: ", p.stderr)[1:]:
        name = b.split()[0]
        remarks[name] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", b)}
    asm = out.read_text()
    parts = re.split(r"\n(_ZN[^\n:]*):[^\n]*\n", asm)
    bodies = {parts[i]: parts[i + 1].split(".end_amdhsa_kernel")[0] for i in range(1, len(parts) - 1, 2)}
    return remarks, bodies


def fixed_names(table):
    names = sorted(n for n in table if "tamp_compress_fixed" in n)
    assert len(names) == 2, names  # FIX = 1 (extended format), FIX = 2 (v1)
    return names


def instructions(body):
    return [ln.strip() for ln in body.split("\n") if ln.startswith("\t") and ln.strip() and ln.strip()[0] not in ".;"]


def test_registers_spills_occupancy(device_code):
    remarks, _ = device_code
    for name in fixed_names(remarks):
        r = remarks[name]
        assert r["VGPRs"] <= 64 and r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
        assert r["Occupancy"] == 8, (name, r)
        assert r["SGPRs Spill"] < 135, (name, r)


def test_isa(device_code):
    _, bodies = device_code
    ext_name, v1_name = fixed_names(bodies)
    counts = {}
    for name in (ext_name, v1_name):
        ins = instructions(bodies[name])
        counts[name] = len(ins)
        assert not any(i.startswith(("flat_", "scratch_")) for i in ins), name
        assert all(f"s_setprio {k}" in bodies[name] for k in (0, 2, 3)), name  # the wavefront priorities of DESIGN.md 3.14
        assert sum(i.startswith(("v_readlane", "v_writelane")) for i in ins) < 360, name
        # LDS region bases are immediates: (nearly) every LDS access carries an offset, and the dynamic allocation's size
        # is not needed for any address
        ds = [i for i in ins if i.startswith("ds_")]
        assert sum("offset" in i for i in ds) >= 0.8 * len(ds), name
    # the v1 build carries nothing of the extended format: no settled-token pass, no RLE / extended-match state machine
    assert counts[v1_name] < 0.75 * counts[ext_name], counts
    # both are smaller than the generic build they stand in for
    generic = [n for n in bodies if n.startswith("_ZN8tamp_amd20tamp_compress_kernelILb1ELb0ELb1ELj1024ELj10ELb1ELb0E")]
    assert len(generic) == 1, generic
    assert counts[ext_name] < len(instructions(bodies[generic[0]])), counts
