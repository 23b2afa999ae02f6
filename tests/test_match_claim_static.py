"""CPU tier: the match phase's hand-out of sorted query groups (kClaim in tamp_compress_kernel.hpp), from a cross-compile of the
device code the way tests/test_bucket_loop_static.py makes one.

  * Both fixed-geometry kernels hold the claim: one LDS atomic with return on the claim's control word, inside the match phase, its
    result read by v_readfirstlane_b32.
  * Nobody waits for anybody in that phase: between the phase's first and last instruction there is no s_sleep, and no loop reads an
    LDS word again at an address the loop does not change unless a barrier or an LDS atomic stands in the loop (a loop is the span
    from a label to a later branch back to it; an address it "does not change" is a ds_read whose address register no instruction
    of the span writes).
  * The generic build of the same geometry (W = 2^10, run-aware, persistent) has no such atomic: its loop is the strided one.

The match phase of a kernel: from the first to the last instruction attributed to the source lines between the phase's banner
comment and the priority change behind its closing barrier.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "tamp_compress_kernel.hpp"
KERNEL_HPP = os.path.join(ROOT, "tamp_amd", "csrc", KERNEL)
GENERIC_1024 = "tamp_compress_kernelILb1ELb0ELb1ELj1024ELj10ELb1ELb0EE"  # <PACKED, !LAZY, RUNS, 1024, 10 bucket bits, LOOP, !BLOCKM>
ATOMIC = re.compile(r"ds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)(_rtn)?_[uif]\d+")


@pytest.fixture(scope="module")
def device_code(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("match_claim") / "dev.s"
    flags = None
    for line in open(os.path.join(ROOT, "tamp_amd", "csrc", "Makefile")):
        m = re.match(r"HIPFLAGS \?= (.*)", line)
        if m:
            flags = m.group(1).replace("$(ARCH)", "gfx950").split()
    assert flags, "HIPFLAGS of the library's Makefile"
    p = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-gline-tables-only", "-S", "tamp_capi.hip", "-o", str(out)],
                       cwd=os.path.join(ROOT, "tamp_amd", "csrc"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    asm = out.read_text()
    files = {int(n): os.path.basename(f) for n, f in re.findall(r'\n\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]*)"', asm)}
    parts = re.split(r"\n(_ZN[^\n:]*):[^\n]*\n", asm)
    bodies = {parts[i]: parts[i + 1].split(".end_amdhsa_kernel")[0] for i in range(1, len(parts) - 1, 2)}
    fixed = sorted(n for n in bodies if "tamp_compress_fixed" in n)
    generic = [n for n in bodies if GENERIC_1024 in n]
    assert len(fixed) == 2 and len(generic) == 1, (fixed, generic)
    return bodies, files, {"ext": fixed[0], "v1": fixed[1], "generic": generic[0]}  # FIX = 1 (extended format), FIX = 2 (v1)


def located(body, files):
    """[(source file, line, text)] of a kernel body: every instruction and every label, with the last .loc in front of it."""
    out, cur = [], (None, 0)
    for ln in body.split("\n"):
        s = ln.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            cur = (files.get(int(m.group(1))), int(m.group(2)))
        elif re.match(r"\.LBB\w+:", s):
            out.append((cur[0], cur[1], s.split(":")[0] + ":"))
        elif ln.startswith("\t") and s and s[0] not in ".;":
            out.append((cur[0], cur[1], s.split(";")[0].strip()))
    return out


def match_phase(ins):
    src = open(KERNEL_HPP).read().split("\n")
    first = next(i + 1 for i, ln in enumerate(src) if "---------------- match: find_best_match" in ln)
    last = next(i + 1 for i, ln in enumerate(src) if i + 1 > first and "__builtin_amdgcn_s_setprio(kPrioShort);" in ln)
    at = [k for k, (f, ln, _) in enumerate(ins) if f == KERNEL and first <= ln <= last]
    assert at, "the phase's lines have instructions of their own"
    return [t for _, _, t in ins[at[0]:at[-1] + 1]]


def regs(operand):
    """The registers an operand names: v5 -> {v5}, v[4:7] -> {v4..v7}."""
    m = re.fullmatch(r"([vs])\[(\d+):(\d+)\]", operand)
    if m:
        return {m.group(1) + str(k) for k in range(int(m.group(2)), int(m.group(3)) + 1)}
    return {operand} if re.fullmatch(r"[vs]\d+|vcc|exec", operand) else set()


def loops(phase):
    """[(first, last)] instruction spans from a label to a later branch back to it."""
    labels = {t[:-1]: k for k, t in enumerate(phase) if t.endswith(":")}
    out = []
    for k, t in enumerate(phase):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", t)
        if m and m.group(1) in labels and labels[m.group(1)] < k:
            out.append((labels[m.group(1)], k))
    return out


def waiting_loops(phase):
    """Loops that read an LDS word at an address they do not change, with no barrier and no LDS atomic in them."""
    bad = []
    for a, b in loops(phase):
        span = [t for t in phase[a:b + 1] if not t.endswith(":")]
        if any(t.startswith("s_barrier") or ATOMIC.match(t) for t in span):
            continue
        written = set()
        for t in span:
            ops = [o.strip() for o in t.split(None, 1)[1].split(",")] if " " in t else []
            if ops and not t.startswith(("ds_write", "s_cmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop")):
                written |= regs(ops[0])  # (the destination comes first)
        for t in span:
            if t.startswith("ds_read"):
                ops = [o.strip().split()[0] for o in t.split(None, 1)[1].split(",")]
                if not (regs(ops[1]) & written):
                    bad.append((phase[a], t))
    return bad


@pytest.mark.parametrize("which", ["ext", "v1"])
def test_fixed_kernels_claim_their_groups_in_the_match_phase(device_code, which):
    bodies, files, names = device_code
    ins = located(bodies[names[which]], files)
    phase = match_phase(ins)
    whole = [t for _, _, t in ins if t.startswith("ds_inc_rtn_u32")]
    claims = [k for k, t in enumerate(phase) if t.startswith("ds_inc_rtn_u32")]
    assert len(whole) == 1 and len(claims) == 1, (whole, claims)
    dst = phase[claims[0]].split()[1].rstrip(",")
    behind = phase[claims[0] + 1:claims[0] + 8]
    assert any(t.startswith("v_readfirstlane_b32") and t.endswith(dst) for t in behind), behind
    # the claim is inside a loop: taken again whenever a group is done
    assert any(a < claims[0] < b for a, b in loops(phase))


@pytest.mark.parametrize("which", ["ext", "v1"])
def test_nobody_waits_in_the_match_phase(device_code, which):
    bodies, files, names = device_code
    phase = match_phase(located(bodies[names[which]], files))
    assert len(loops(phase)) >= 3, "the claim loop, the bucket scan, the wrap zone"
    assert not any(t.startswith("s_sleep") for t in phase)
    assert waiting_loops(phase) == []


def test_the_check_sees_a_waiting_loop():
    spin = [".LBB0_1:", "ds_read_b32 v1, v2 offset:72", "s_waitcnt lgkmcnt(0)", "v_cmp_eq_u32_e32 vcc, 0, v1", "s_cbranch_vccnz .LBB0_1"]
    assert waiting_loops(spin) == [(".LBB0_1:", "ds_read_b32 v1, v2 offset:72")]
    assert waiting_loops(spin[:1] + ["v_add_u32_e32 v2, 4, v2"] + spin[1:]) == []
    assert waiting_loops(spin[:1] + ["s_barrier"] + spin[1:]) == []


def test_generic_build_keeps_the_strided_loop(device_code):
    bodies, files, names = device_code
    ins = [t for _, _, t in located(bodies[names["generic"]], files)]
    assert not any(t.startswith("ds_inc_rtn_u32") for t in ins)
