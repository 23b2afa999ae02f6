#!/usr/bin/env python3
"""tests/golden/cut_sweep.json: what ONE reference TampCompressor object returns when the cut sweep's input
(tests/cut_sweep_input.py) reaches it in two calls cut at every byte.

    python tests/golden/make_cut_sweep.py

For every configuration and every cut c in 0..len(src): tamp_compressor_compress(src[:c]) then
tamp_compressor_compress_and_flush(src[c:], write_token=false), 4,096 bytes of room each, on the reference C built in
place (oracle/_ref; build container only).  Per call three integers are kept -- status, bytes written, bytes consumed:
the written bytes are always the next bytes of the one-shot stream, which the tests take from the oracle.
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
import cut_sweep_input as cs  # noqa: E402

PATH = os.path.join(HERE, "cut_sweep.json")


def generate(ref, configs=cs.CONFIGS):
    """The fixture's content from a live reference object (oracle.checker.Ref)."""
    recs = []
    for window, extended in configs:
        src = cs.source(window)
        rc, whole = ref.compress(src, window=window, literal=cs.LITERAL, extended=extended)
        assert rc == 0
        cuts = []
        for c in range(len(src) + 1):
            r0, calls = ref.encode_script([("compress", src[:c], cs.CAP), ("compress_and_flush", src[c:], False, cs.CAP)],
                                          window=window, literal=cs.LITERAL, extended=extended)
            assert r0 == 0 and len(calls) == 2
            (s1, o1, k1), (s2, o2, k2) = calls
            assert o1 + o2 == whole, (window, extended, c)  # the stream does not depend on the cut
            cuts.append([s1, len(o1), k1, s2, len(o2), k2])
        recs.append(dict(window=window, extended=extended, literal=cs.LITERAL, cap=cs.CAP, input_len=len(src),
                         input_sha256=hashlib.sha256(src).hexdigest(), whole_len=len(whole),
                         whole_sha256=hashlib.sha256(whole).hexdigest(), cuts=cuts))
    return recs


def main():
    from oracle.checker import Ref

    recs = generate(Ref())
    with open(PATH, "w") as f:  # one line per cut keeps diffs readable
        f.write("[\n")
        for i, r in enumerate(recs):
            head = {k: v for k, v in r.items() if k != "cuts"}
            f.write(json.dumps(head)[:-1] + ', "cuts": [\n')
            f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in r["cuts"]))
            f.write("\n]}" + (",\n" if i + 1 < len(recs) else "\n"))
        f.write("]\n")
    print(f"{sum(len(r['cuts']) for r in recs)} cuts in {len(recs)} configurations -> {PATH}")


if __name__ == "__main__":
    main()
