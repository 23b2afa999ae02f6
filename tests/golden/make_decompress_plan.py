#!/usr/bin/env python3
"""Regenerate tests/golden/decompress_plan.json: what the decode launcher decides over a grid of calls, pre-pass results, device
facts and tuning variables.

    python tests/golden/make_decompress_plan.py <commit>          (from the repository root; needs git, make and hipcc)

The fixture is a CHARACTERISATION of launch_decompress as it stood in commit a88a792, the last one in which the launcher wrote
its decisions out inline, between allocations and launches -- and NOT of plan_decompress (tamp_amd/csrc/tamp_decompress_plan.hpp),
which tests/test_decompress_plan_golden.py holds to these rows.  That commit has no query to ask, so the recipe is:

  1. `git archive <commit>` into a temporary directory;
  2. apply tests/golden/decompress_plan_parent_query.patch: it adds tamp_amd_decompress_plan to that tree's tamp_capi.hip as a
     line-for-line copy of the launcher's inline decisions, allocations and launches left out.  Its only substitutions are the
     reads of ctx->cu_count, hipMemGetInfo, rec.split.bytes and the pre-pass result, which become query fields, and the allocation
     loop giving up, which becomes the query's exclude_split.  Review it against the launcher's text of that commit;
  3. build that tree's library (make -C tamp_amd/csrc);
  4. walk the grid below with it.

Regenerate only when a change is MEANT to move a decision: from the commit before that change (with the patch rebased onto it)
plus a review of every row that differs.  Everything is host arithmetic: no GPU is needed.

Encoding.  An answer is cut into the six groups of GROUPS; `tables` holds the distinct tuples of each group, and every section
holds, per group, the table index of every row of its grid in itertools.product order (the last axis varies fastest).  A hundred
thousand rows of six indices are kept as base64(zlib(little-endian uint16 array)) -- pack_rows() / unpack_rows() -- which keeps the
file in the tens of kilobytes; the tables stay plain.  Axis values that depend on another axis are symbols, resolved by
n_streams() and scan_words() below.
"""
import base64
import struct
import zlib
import ctypes
import itertools
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

PATH = os.path.join(HERE, "decompress_plan.json")
PATCH = os.path.join(HERE, "decompress_plan_parent_query.patch")
TUNING_ENV = ("TAMP_AMD_DECODER", "TAMP_AMD_SPLIT_SLICE_LOG2", "TAMP_AMD_SPLIT_SCRATCH_MB", "TAMP_AMD_SPLIT_WAVE_MAX",
              "TAMP_AMD_SPLIT_SPW", "TAMP_AMD_SCRATCH_MB", "TAMP_AMD_LONGDEC", "TAMP_AMD_LONGDEC_MIN", "TAMP_AMD_LONGDEC_EXT",
              "TAMP_AMD_LONGDEC_CHAIN")
EXACT = 0x80  # include/tamp_amd.h TAMP_AMD_WINDOW_BITS_EXACT
GIB = 1 << 30


class Query(ctypes.Structure):  # include/tamp_amd.h TampAmdDecodeQuery
    _fields_ = [("n_streams", ctypes.c_uint64), ("max_window_bits", ctypes.c_uint8), ("has_dictionary", ctypes.c_uint8),
                ("exclude_split", ctypes.c_uint8), ("free_known", ctypes.c_uint8), ("cu_count", ctypes.c_uint32),
                ("scan_found", ctypes.c_uint32), ("scan_longest_in", ctypes.c_uint32), ("scan_window_units", ctypes.c_uint32),
                ("scan_max_out_cap", ctypes.c_uint32), ("free_bytes", ctypes.c_uint64), ("held_bytes", ctypes.c_uint64)]


GROUPS = [  # include/tamp_amd.h TampAmdDecodePlan, in its order
    ["long", ["long_attempt", "long_min_len", "long_extended", "long_chain"]],
    ["choice", ["scan", "decoder", "max_window_bits", "bulk"]],
    ["split", ["split_tokcap", "split_maxcap", "split_wave_resolve", "split_resolve_lds", "split_spw", "split_slice", "split_slab_bytes"]],
    ["wave", ["wave_waves", "wave_lds", "wave_groups"]],
    ["lane", ["lane_lds_row", "lane_lds", "lane_per_cu", "lane_grid"]],
    ["global", ["global_slot", "global_grid", "global_bulk", "global_lds", "global_lanes", "global_slab_bytes"]],
]
U64 = ("split_slice", "split_slab_bytes", "global_lanes", "global_slab_bytes")


class Plan(ctypes.Structure):
    _fields_ = ([(f, ctypes.c_uint32) for _, fs in GROUPS for f in fs if f not in U64] + [(f, ctypes.c_uint64) for f in U64])


FORCED = [{"TAMP_AMD_DECODER": d} for d in ("split", "lane", "global", "wave")]
LDS_EDGES = ["lds:%d:%d:%s" % (w, bulk, edge) for w in (8, 9, 10) for bulk in (0, 1) for edge in ("lo-1", "lo", "hi", "hi+1")]
N_ALL = [1, 16, 17, 255, 256, 257, 4096, 65536, 1 << 18, (1 << 18) + 1, 1 << 20, "slab-1", "slab"] + LDS_EDGES
# [longest_in, max_out_cap, found, window units]: found 0 | 8 | "w-1" | "w" (the call's window bits), units "uniform" | "mixed"
SCAN_TYPICAL = [4096, 4096, "w", "uniform"]
LONGEST = [0, 1, 511, 512, 4096, 1 << 20]
OUT_CAP = [0, 1024, 2048, 2049, 4096, 16384, 16385]
SCANS = ([[l, c, "w", "uniform"] for l in LONGEST for c in OUT_CAP] +
         [[l, c, f, u] for l, c in ((511, 1024), (4096, 4096), (4096, 16385)) for f in (0, 8, "w-1", "w") for u in ("uniform", "mixed")
          if (f, u) != ("w", "uniform")])
SECTIONS = [
    # every call shape under every forced decoder and the long-stream gates, with a typical pre-pass result where one is read
    ["calls", [["env", [{}] + FORCED + [{"TAMP_AMD_LONGDEC": "0"}, {"TAMP_AMD_LONGDEC_MIN": "65536"}]],
               ["cu_count", [256, 8]], ["dictionary", [0, 1]], ["exact", [0, 1]], ["max_wbits", list(range(7, 17))],
               ["free", [None]], ["held", [0]], ["exclude_split", [0]], ["scan", [SCAN_TYPICAL]], ["n_streams", N_ALL]]],
    # every pre-pass result, where the pre-pass runs
    ["scans", [["env", [{}] + FORCED], ["cu_count", [256, 8]], ["dictionary", [0, 1]], ["exact", [0]], ["max_wbits", [8, 9, 10, 11, 13, 15]],
               ["free", [None]], ["held", [0]], ["exclude_split", [0]], ["scan", SCANS],
               ["n_streams", [255, 256, 4096, "slab-1", "slab", "lds:10:1:lo-1", "lds:10:1:lo", "lds:10:1:hi", "lds:10:1:hi+1", 1 << 20]]]],
    # the split decoder's scratch budget, and what the launcher takes when no scratch is to be had
    ["budget", [["env", [{}, {"TAMP_AMD_DECODER": "split"}, {"TAMP_AMD_SPLIT_SCRATCH_MB": "64"}]], ["cu_count", [256, 8]], ["dictionary", [0]],
                ["exact", [0]], ["max_wbits", [8, 10, 12]], ["free", [None, GIB, 64 * GIB]], ["held", [0, 20 * GIB]], ["exclude_split", [0, 1]],
                ["scan", [[511, 1024, "w", "uniform"], [4096, 4096, "w", "uniform"], [1 << 20, 16384, "w", "uniform"]]],
                ["n_streams", [256, 4096, 65536, 1 << 18, (1 << 18) + 1, 1 << 20]]]],
    # the other tuning variables, on a reduced grid
    ["tuning", [["env", [{"TAMP_AMD_SPLIT_SLICE_LOG2": "12"}, {"TAMP_AMD_SPLIT_SCRATCH_MB": "64"}, {"TAMP_AMD_SPLIT_WAVE_MAX": "0"},
                         {"TAMP_AMD_SPLIT_WAVE_MAX": "4096"}, {"TAMP_AMD_SPLIT_SPW": "16"}, {"TAMP_AMD_SCRATCH_MB": "16"},
                         {"TAMP_AMD_LONGDEC": "0"}, {"TAMP_AMD_LONGDEC_MIN": "65536"}]],
                ["cu_count", [256, 8]], ["dictionary", [0]], ["exact", [0]], ["max_wbits", [8, 10, 12, 15]], ["free", [None, GIB]], ["held", [0]],
                ["exclude_split", [0]],
                ["scan", [[511, 1024, "w", "uniform"], [4096, 4096, "w", "uniform"], [1 << 20, 16384, "w", "mixed"], [4096, 16385, "w", "uniform"]]],
                ["n_streams", [16, 256, 4096, 65536, (1 << 18) + 1, 1 << 20]]]],
]


def lds_capacity(cu_count, wbits, bulk):
    """Streams one round of the LDS lane decoder holds: 64 per workgroup, as many workgroups per CU as 160 KiB of
    LDS allow, sixteen at most.  A row is the window + 4 bytes, in the bulk build + 36 bytes next to 128 + 64 x 148 bytes."""
    lds = 128 + 64 * 148 + 64 * ((1 << wbits) + 36) if bulk else 64 * ((1 << wbits) + 4)
    return cu_count * min((160 << 10) // lds, 16) * 64


def n_streams(spec, cu_count):
    """"slab": where the global lanes start (cu_count x 192 streams); "lds:<wbits>:<bulk>:<edge>": either side of 0.6 x and
    1.25 x the LDS lanes' capacity."""
    if isinstance(spec, int):
        return spec
    if spec.startswith("slab"):
        return cu_count * 192 - (spec == "slab-1")
    _, wbits, bulk, edge = spec.split(":")
    cap = lds_capacity(cu_count, int(wbits), int(bulk))
    lo, hi = -(-cap * 6 // 10), cap * 5 // 4  # first n with 10 n >= 6 cap, last with 4 n <= 5 cap
    return {"lo-1": lo - 1, "lo": lo, "hi": hi, "hi+1": hi + 1}[edge]


def scan_words(spec, wbits, n):
    """found, longest_in, window bytes in 256-byte units, max_out_cap.  uniform: every stream at window 2^found; mixed: half of
    them at 2^8."""
    longest, cap, found, units = spec
    w = wbits & 0x7F
    f = {"w": w, "w-1": w - 1}.get(found, found)
    per = 0 if f < 8 else ((1 << f) if units == "uniform" else ((1 << f) + 256) // 2)
    return f, longest, n * per // 256, cap


def pack_rows(indices):
    return base64.b64encode(zlib.compress(struct.pack("<%dH" % len(indices), *indices), 9)).decode()


def unpack_rows(text):
    raw = zlib.decompress(base64.b64decode(text))
    return struct.unpack("<%dH" % (len(raw) // 2), raw)


def walk(axes):
    """Every grid point of `axes` as a Query, in itertools.product order; the environment is set on the way."""
    env = None
    names = [name for name, _ in axes]
    for point in itertools.product(*[values for _, values in axes]):
        p = dict(zip(names, point))
        if p["env"] is not env:  # (the slowest axis)
            env = p["env"]
            for k in TUNING_ENV:
                os.environ.pop(k, None)
            os.environ.update(env)
        n = n_streams(p["n_streams"], p["cu_count"])
        bits = p["max_wbits"] | (EXACT if p["exact"] else 0)
        yield p, Query(n, bits, p["dictionary"], p["exclude_split"], p["free"] is not None, p["cu_count"],
                       *scan_words(p["scan"], bits, n), p["free"] or 0, p["held"])
    for k in TUNING_ENV:
        os.environ.pop(k, None)


def answer(lib, q):
    """The query's answer as one tuple per group of GROUPS."""
    plan = Plan()
    assert lib.tamp_amd_decompress_plan(ctypes.byref(q), ctypes.byref(plan)) == 0
    return [[getattr(plan, f) for f in fields] for _, fields in GROUPS]


def build_parent(commit, tmp):
    subprocess.run("git archive %s | tar -x -C %s" % (commit, tmp), shell=True, check=True, cwd=ROOT)
    subprocess.check_call(["patch", "-p1", "-s", "-i", PATCH], cwd=tmp)
    subprocess.check_call(["make", "-C", os.path.join(tmp, "tamp_amd", "csrc"), "../libtamp_amd.so"])
    return os.path.join(tmp, "tamp_amd", "libtamp_amd.so")


def main():
    assert len(sys.argv) == 2, __doc__
    with tempfile.TemporaryDirectory() as tmp:
        # (TAMP_AMD_PLAN_LIB: a library already built by steps 1 to 3)
        lib = ctypes.CDLL(os.environ.get("TAMP_AMD_PLAN_LIB") or build_parent(sys.argv[1], tmp))
        tables = {g: [] for g, _ in GROUPS}
        index = {g: {} for g, _ in GROUPS}
        sections, total = [], 0
        for name, axes in SECTIONS:
            rows = {g: [] for g, _ in GROUPS}
            for _, q in walk(axes):
                total += 1
                for (g, _), t in zip(GROUPS, answer(lib, q)):
                    i = index[g].setdefault(tuple(t), len(tables[g]))
                    if i == len(tables[g]):
                        tables[g].append(t)
                    rows[g].append(i)
            sections.append([name, {"axes": axes, "rows": {g: pack_rows(r) for g, r in rows.items()}}])
    doc = {"recorded_from": sys.argv[1], "groups": GROUPS, "tables": tables, "sections": sections}
    with open(PATH, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d rows, %s distinct tuples, %d bytes" % (PATH, total, {g: len(t) for g, t in tables.items()}, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
