#!/usr/bin/env python3
"""Regenerate tests/golden/compress_plan.json: what the two host-only launch queries answer over a grid of calls.

    TAMP_AMD_LIB=<libtamp_amd.so of the commit to record> python tests/golden/make_compress_plan.py <commit>

The fixture is a CHARACTERISATION of the launcher's decisions, recorded from the library of commit ee4e9e4 -- the last one
in which tamp_amd_compress_plan, tamp_amd_compress_build and the two launchers each wrote those decisions out for themselves --
and NOT from the library that shares one plan_compress (tamp_amd/csrc/tamp_compress_plan.hpp): tests/
test_compress_plan_golden.py holds the shared plan to these rows.  Regenerate it only when a change is MEANT to move a
decision, from the library of the commit before that change plus a review of every row that differs.  Both queries are host
arithmetic: no GPU is needed.

  plan   tamp_amd_compress_plan over window x max_in_len x lazy x environment.  Recorded with TAMP_AMD_RUNS unset only: the
         query honours that variable since it shares the launcher's plan, the one place where its answer was allowed to move.
         `tuples` are the distinct (block, LDS bytes, threads, workgroups per CU) answers, `rows` index them in grid order.
  build  tamp_amd_compress_build over the axes in `axes`, in itertools.product order (the last axis varies fastest), as
         run lengths [TAMP_AMD_BUILD_*, count]: nearly every call takes the generic build.
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, "compress_plan.json")
TUNING_ENV = ("TAMP_AMD_BLK", "TAMP_AMD_RUNS", "TAMP_AMD_FIXED_BUILD", "TAMP_AMD_BLOCK_LEAN")

STATE, RESUME, SAVE, FLUSH_TOKEN, PARTIAL, APPEND, BLOCK_MODE = 1, 2, 4, 8, 16, 32, 64  # include/tamp_amd.h TAMP_AMD_CALL_*
ALIGNED, MISALIGNED = 0x7F0000001000, 0x7F0000001002

PLAN_AXES = [
    ["env", [{}] + [{"TAMP_AMD_BLK": str(b)} for b in (64, 512, 960, 1024, 2048)]],
    ["window", list(range(8, 16))],
    ["max_in_len", [0, 1, 63, 64, 65, 256, 512, 960, 1023, 1024, 1025, 1088, 1280, 1536, 2047, 2048, 2049, 4096, 65536, 1 << 20]],
    ["lazy", [0, 1]],
]
BUILD_AXES = [
    ["env", [{}, {"TAMP_AMD_FIXED_BUILD": "0"}, {"TAMP_AMD_RUNS": "0"}, {"TAMP_AMD_RUNS": "1"}, {"TAMP_AMD_BLK": "512"}]],
    ["window", list(range(8, 16))],
    ["literal", [5, 8]],
    ["extended", [0, 1]],
    ["lazy", [0, 1]],
    ["hint", [0, 1, 2]],
    ["reset", [0, 1]],
    ["max_in_len", [0, 256, 960, 1024, 4096, 1 << 20]],
    ["flags", [0, STATE, RESUME, SAVE, FLUSH_TOKEN, PARTIAL, APPEND, BLOCK_MODE, STATE | RESUME | SAVE]],
    ["dictionary", [[0, ALIGNED], [0, MISALIGNED], [1, ALIGNED], [1, MISALIGNED]]],  # [use_custom_dictionary, address]
]


def walk(axes):
    """Every grid point of `axes` as a dict, in itertools.product order; the environment is set on the way."""
    env = None
    for point in itertools.product(*[values for _, values in axes]):
        p = dict(zip([name for name, _ in axes], point))
        if p["env"] is not env:  # (the slowest axis)
            env = p["env"]
            for k in TUNING_ENV:
                os.environ.pop(k, None)
            os.environ.update(env)
        yield p
    for k in TUNING_ENV:
        os.environ.pop(k, None)


def plan_row(lib, p):
    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert lib.tamp_amd_compress_plan(p["window"], p["max_in_len"], p["lazy"], *[ctypes.byref(x) for x in v]) == 0
    return [x.value for x in v]


def build_row(lib, p):
    from tamp_amd import _lib

    custom, address = p["dictionary"]
    conf = _lib.TampAmdConf(p["window"], p["literal"], custom, p["extended"], p["reset"], p["lazy"], p["hint"], 0)
    return lib.tamp_amd_compress_build(ctypes.byref(conf), p["max_in_len"], p["flags"], address)


def main():
    from tamp_amd import _lib

    assert len(sys.argv) == 2 and os.environ.get("TAMP_AMD_LIB"), __doc__
    lib = _lib.load()
    tuples, rows = [], []
    for p in walk(PLAN_AXES):
        t = plan_row(lib, p)
        if t not in tuples:
            tuples.append(t)
        rows.append(tuples.index(t))
    runs = []
    for p in walk(BUILD_AXES):
        b = build_row(lib, p)
        assert b in (0, 1, 2), (p, b)
        if runs and runs[-1][0] == b:
            runs[-1][1] += 1
        else:
            runs.append([b, 1])
    doc = {"recorded_from": sys.argv[1],
           "plan": {"axes": PLAN_AXES, "tuples": tuples, "rows": rows},
           "build": {"axes": BUILD_AXES, "runs": runs}}
    with open(PATH, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d plan rows (%d distinct), %d build rows in %d runs, %d bytes" % (
        PATH, len(rows), len(tuples), sum(n for _, n in runs), len(runs), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
