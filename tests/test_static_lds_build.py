"""CPU tier: the fixed-geometry compress builds take their LDS from a static array, every other build from the
dynamic allocation.  From a cross-compile of the device code with the library's own flags (hipcc needs no GPU):

* both fixed kernels reserve kLdsFixed.total = 19,616 bytes of LDS in their descriptors; the generic headline build and the
  one-wavefront build reserve none (their dynamic base stays 0, their total what the launcher plans);
* no LDS address of a fixed kernel is made by adding the literal 0 to a register (the base of a dynamic allocation, which the
  compiler folds too late to drop the add: 115 such adds in the extended build before the static array);
* their VALU instruction counts -- vector ALU including v_readlane / v_writelane, as tools/isa_classes.py classes them -- are below
  those of the builds on dynamic LDS, 2,927 (extended) and 2,021 (v1): profiles/static_lds_static.txt, same toolchain.

And on the host: `ffbl | k` is the saturating add the 16-byte compare's tail used to make, for every value v_ffbl_b32 returns.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_FIXED = 19616  # kLdsFixed.total (tamp_compress_kernel.hpp pins it with a static_assert; tests/golden/compress_plan.json reports it)
VALU_DYNAMIC_LDS = {"ext": 2927, "v1": 2021}  # profiles/static_lds_static.txt, column "parent"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("static_lds") / "dev.s"
    flags = None
    for line in open(os.path.join(ROOT, "tamp_amd", "csrc", "Makefile")):
        m = re.match(r"HIPFLAGS \?= (.*)", line)
        if m:
            flags = m.group(1).replace("$(ARCH)", "gfx950").split()
    assert flags, "HIPFLAGS of the library's Makefile"
    p = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "tamp_capi.hip", "-o", str(out)],
                       cwd=os.path.join(ROOT, "tamp_amd", "csrc"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    parts = re.split(r"\n(_ZN[^\n:]*):[^\n]*\n", out.read_text())
    table = {}
    for i in range(1, len(parts) - 1, 2):
        body = parts[i + 1].split(".end_amdhsa_kernel")[0]
        m = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body)
        if m:
            code = body.split(".amdhsa_kernel")[0]
            ins = [ln.strip() for ln in code.split("\n") if ln.startswith("\t") and ln.strip() and ln.strip()[0] not in ".;"]
            table[parts[i]] = (int(m.group(1)), ins)
    return table


def fixed_names(table):
    names = sorted(n for n in table if "tamp_compress_fixed" in n)
    assert len(names) == 2, names  # FIX = 1 (extended format), FIX = 2 (v1)
    return dict(zip(("ext", "v1"), names))


def test_static_lds_only_in_the_fixed_builds(kernels):
    for name in fixed_names(kernels).values():
        assert kernels[name][0] == LDS_FIXED, (name, kernels[name][0])
    # the generic headline build (PACKED, RUNS, WSCAN 1024, 1,024 buckets, LOOP) and the one-wavefront build (512 buckets, no LOOP)
    for prefix in ("_ZN8tamp_amd20tamp_compress_kernelILb1ELb0ELb1ELj1024ELj10ELb1ELb0E", "_ZN8tamp_amd20tamp_compress_kernelILb1ELb0ELb0ELj0ELj9ELb0ELb0E"):
        names = [n for n in kernels if n.startswith(prefix)]
        assert len(names) == 1, (prefix, names)
        assert kernels[names[0]][0] == 0, (names[0], kernels[names[0]][0])
    # ... and so does every other build of the compress kernel
    for name, (lds, _) in kernels.items():
        if "tamp_compress_kernel" in name or "tamp_compress_dict_kernel" in name:
            assert lds == 0, (name, lds)


def test_no_add_of_zero_and_fewer_valu_instructions(kernels):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from isa_classes import classify
    finally:
        sys.path.pop(0)
    for tag, name in fixed_names(kernels).items():
        ins = kernels[name][1]
        zero_adds = [i for i in ins if re.match(r"v_add_u32_e32\s+v\d+,\s*0,\s*v\d+", i)]
        assert not zero_adds, (name, len(zero_adds))
        valu = 0
        for i in ins:
            op, operands = (i.split(None, 1) + [""])[:2]
            valu += classify(op, operands.split(";")[0]) in ("fast", "slow", "lane")
        print(tag, "VALU instructions:", valu, "of", VALU_DYNAMIC_LDS[tag], "on dynamic LDS")
        assert valu < VALU_DYNAMIC_LDS[tag], (name, valu)


def test_or_is_the_saturating_add_for_every_first_set_bit():
    """v_ffbl_b32 returns 0..31, or all ones for a zero operand: for these 33 values `| k` equals the unsigned saturating `+ k`
    with k = 32, 64, 96 (the bits of k lie above bit 4; all ones stays all ones either way)."""
    for f in list(range(32)) + [0xFFFFFFFF]:
        for k in (32, 64, 96):
            assert (f | k) == min(f + k, 0xFFFFFFFF), (f, k)
