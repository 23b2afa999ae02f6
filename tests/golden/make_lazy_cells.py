#!/usr/bin/env python3
"""tests/golden/lazy_cells.json: what the reference C returns for the designed lazy-matching inputs of tests/lazy_input.py.

    python tests/golden/make_lazy_cells.py

"cases": per configuration (window, literal, format) and case the reference's one-shot result with lazy_matching on -- status,
bytes written and their SHA-256 (the bytes themselves are the oracle's, which the CPU tier holds against these three).
"sweep": per configuration what ONE reference TampCompressor object with lazy matching returns when the sweep stream
(lazy_input.sweep_source) reaches it in two calls cut at every byte: tamp_compressor_compress(src[:c]), then
tamp_compressor_compress_and_flush(src[c:], write_token=false), 4,096 bytes of room each; per call status, bytes written, bytes
consumed.  Recorded results only; needs the reference C built in place (oracle/_ref; build container only).
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lazy_input as li  # noqa: E402

PATH = os.path.join(HERE, "lazy_cells.json")
CAP = 4096
CONFIGS = tuple((w, 8, e) for w in li.CONFIGS_8 for e in (True, False)) + tuple((w, l, e) for w, l in li.CONFIGS_OTHER for e in (True, False))
SWEEPS = ((8, True), (8, False), (10, True), (10, False))


def config_id(window, literal, extended):
    return f"w{window}-l{literal}-{'ext' if extended else 'v1'}"


def generate_cases(ref, configs=CONFIGS):
    out = {}
    for window, literal, extended in configs:
        rec = {}
        for c in li.cases(window, literal, extended):
            rc, blob = ref.compress(c.data, window=window, literal=literal, extended=extended, dictionary=c.dictionary, lazy_matching=True)
            rec[c.name] = [rc, len(blob), hashlib.sha256(blob).hexdigest()]
        out[config_id(window, literal, extended)] = rec
    return out


def generate_sweeps(ref, configs=SWEEPS):
    recs = []
    for window, extended in configs:
        src, _ = li.sweep_source(window, extended)
        kw = dict(window=window, literal=8, extended=extended, lazy_matching=True)
        rc, whole = ref.compress(src, **kw)
        assert rc == 0
        cuts = []
        for c in range(len(src) + 1):
            r0, calls = ref.encode_script([("compress", src[:c], CAP), ("compress_and_flush", src[c:], False, CAP)], **kw)
            assert r0 == 0 and len(calls) == 2
            (s1, o1, k1), (s2, o2, k2) = calls
            assert o1 + o2 == whole, (window, extended, c)  # the stream does not depend on the cut
            cuts.append([s1, len(o1), k1, s2, len(o2), k2])
        recs.append(dict(window=window, extended=extended, cap=CAP, input_len=len(src), input_sha256=hashlib.sha256(src).hexdigest(),
                         whole_len=len(whole), whole_sha256=hashlib.sha256(whole).hexdigest(), cuts=cuts))
    return recs


def main():
    from oracle.checker import Ref

    ref = Ref()
    cases, sweeps = generate_cases(ref), generate_sweeps(ref)
    with open(PATH, "w") as f:  # one line per case and per sweep keeps diffs readable
        f.write('{"cases": {\n')
        for i, (cid, rec) in enumerate(cases.items()):
            f.write(f' "{cid}": {{\n')
            f.write(",\n".join(f'  {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in rec.items()))
            f.write("\n }" + (",\n" if i + 1 < len(cases) else "\n"))
        f.write('},\n"sweep": [\n')
        f.write(",\n".join(" " + json.dumps(r, separators=(",", ":")) for r in sweeps))
        f.write("\n]}\n")
    print(f"{sum(len(r) for r in cases.values())} cases in {len(cases)} configurations, {sum(len(r['cuts']) for r in sweeps)} cuts -> {PATH}")


if __name__ == "__main__":
    main()
