#!/usr/bin/env python3
"""tests/golden/ext_cells.json: what the reference C returns for the designed extended-match inputs of tests/ext_match_input.py.

    python tests/golden/make_ext_cells.py

Per configuration (window, literal; extended format) and case the reference's one-shot result without and with lazy matching --
status, bytes written and their SHA-256 each (the bytes themselves are the oracle's, which the CPU tier holds against these).
Recorded results only; needs the reference C built in place (oracle/_ref; build container only).
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
import ext_match_input as emi  # noqa: E402

PATH = os.path.join(HERE, "ext_cells.json")
CONFIGS = emi.CONFIGS
config_id = emi.config_id


def record(checker, case, lazy):
    rc, blob = checker.compress(case.data, window=case.window, literal=case.literal, extended=True, dictionary=case.dictionary,
                                lazy_matching=lazy)
    return [rc, len(blob), hashlib.sha256(blob).hexdigest()]


def generate(ref, configs=CONFIGS):
    return {config_id(window, literal): {c.name: [record(ref, c, False), record(ref, c, True)] for c in emi.cases(window, literal)}
            for window, literal in configs}


def main():
    from oracle.checker import Ref

    cases = generate(Ref())
    with open(PATH, "w") as f:  # one line per case keeps diffs readable
        f.write('{"cases": {\n')
        for i, (cid, rec) in enumerate(cases.items()):
            f.write(f' "{cid}": {{\n')
            f.write(",\n".join(f'  {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in rec.items()))
            f.write("\n }" + (",\n" if i + 1 < len(cases) else "\n"))
        f.write("}}\n")
    print(f"{sum(len(r) for r in cases.values())} cases in {len(cases)} configurations -> {PATH}")


if __name__ == "__main__":
    main()
