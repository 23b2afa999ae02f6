#!/usr/bin/env python3
"""tests/golden/bucket_bits.json: status, length and SHA-256 of the stream that the reference C writes for every designed input of
tests/bucket_bits_input.py (window 2^10, literal 8, default parse), in both formats.

    python tests/golden/make_bucket_bits.py

Recorded from the reference C where it is built in place (oracle/_ref), else from the oracle, which the CPU tier holds against the
reference (tests/test_oracle_vs_reference.py); "source" says which.  Recorded results only.
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
import bucket_bits_input as bbi  # noqa: E402

PATH = os.path.join(HERE, "bucket_bits.json")
FORMATS = (("ext", True), ("v1", False))


def generate(codec):
    out = {}
    for fmt, extended in FORMATS:
        rec = {}
        for c in bbi.cells():
            rc, blob = codec.compress(c.data, window=10, literal=8, extended=extended)
            rec[c.name] = [rc, len(blob), hashlib.sha256(blob).hexdigest()]
        out[fmt] = rec
    return out


def main():
    from oracle.checker import Oracle, Ref

    live = Ref.available()
    cases = generate(Ref() if live else Oracle())
    with open(PATH, "w") as f:  # one line per case keeps diffs readable
        f.write('{"source": %s,\n"cases": {\n' % json.dumps("reference" if live else "oracle"))
        for i, (fmt, rec) in enumerate(cases.items()):
            f.write(f' "{fmt}": {{\n')
            f.write(",\n".join(f'  {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in rec.items()))
            f.write("\n }" + (",\n" if i + 1 < len(cases) else "\n"))
        f.write("}}\n")
    print(f"{sum(len(r) for r in cases.values())} cases -> {PATH}")


if __name__ == "__main__":
    main()
