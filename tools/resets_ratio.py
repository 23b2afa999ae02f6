"""What the resets cost in compression ratio: the three frozen corpora (3 MiB each) compressed by the checker on the CPU (the
reference C where it is built, else the oracle) as ONE stream, and with a dictionary reset every 4 / 16 / 64 / 256 KiB -- the bytes
tamp_amd.compress(..., dictionary_reset=True, reset_interval=N) returns.  Window 10, literal 8, extended format.  No GPU.  Dev tool.

    python tools/resets_ratio.py [--out profiles/reset_segments_ratio.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from oracle.checker import Oracle, Ref
    from tamp_amd import workloads as wl

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reset_segments_ratio.txt"))
    args = ap.parse_args()
    checker = Ref() if Ref.available() else Oracle()
    lines = ["# tools/resets_ratio.py: compressed size with a dictionary reset every N bytes against the un-segmented stream",
             f"# ({type(checker).__name__} on the CPU; window 10, literal 8, extended format; frozen corpora of tests/golden, 3 MiB each)",
             f"{'corpus':8s} {'plain':>10s} {'one stream':>11s} " + " ".join(f"{f'{k} KiB':>18s}" for k in (4, 16, 64, 256))]
    for name in ("prose", "python", "markup"):
        data = wl.frozen_corpus(name)
        res, whole = checker.compress(data, dictionary_reset=True)
        assert res == 0
        cols = []
        for kib in (4, 16, 64, 256):
            step = kib << 10
            ops = []
            for at in range(0, len(data), step):
                ops += ([("reset",)] if at else []) + [("write", data[at : at + step])]
            res, blob = checker.stream_script(ops + [("flush", False)], dictionary_reset=True)
            assert res == 0 and checker.decompress(blob, cap=len(data) + 64)[1] == data
            cols.append(f"{len(blob):>9,} {100.0 * (len(blob) - len(whole)) / len(whole):+7.2f}%")
        lines.append(f"{name:8s} {len(data):>10,} {len(whole):>11,} " + " ".join(cols))
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
