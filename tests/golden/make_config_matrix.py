#!/usr/bin/env python3
"""Regenerate tests/golden/config_matrix.json from the REFERENCE, in the build container only.

    python tests/golden/make_config_matrix.py

The header of a stream picks one of 64 settings (window 2^8..2^15 x literal 5..8 x extended on/off), and three things
in every codec path follow from it: the minimum match length (3 instead of 2 for nine (window, literal) pairs,
common.c:54-56), the seeded dictionary (one table per literal width in the extended format, the literal-8 table in v1)
and the literal width of every bit reader and writer.  This fixture records what one reference object does at those
settings:

* ``streams`` -- op scripts (write / flush(write_token) / reset_dictionary / close) replayed on ONE reference compressor
  object (the shape of streaming.json), with the length and SHA-256 of the bytes it emitted;
* ``encoders`` -- call scripts below flush granularity (sink / poll / compress / flush / compress_and_flush with small
  output rooms) on ONE reference compressor object (the shape of encoder_resume.json), with each call's status, byte
  count and consumed count, and the bytes of all calls together (each call's bytes are the next slice of them).

Coverage: every literal width at windows 2^8, 2^10, 2^13, 2^14 and 2^15, every (window, literal) pair whose minimum match
is 3, both formats, and on subsets a custom dictionary, ``dictionary_reset`` and ``lazy_matching``.  Inputs are
tamp_amd.workloads rows masked to the literal width, recorded as ``[workload, row]`` pieces (the names
tests/conftest.py:workload_rows reads) with the SHA-256 of their concatenation; script ops index that source, so the
file holds no input bytes.
"""
import base64
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from conftest import workload_rows  # noqa: E402
from oracle.checker import Ref  # noqa: E402

PATH = os.path.join(HERE, "config_matrix.json")


def min_pattern_size(window, literal):
    return 2 + (window > 10 + 2 * (literal - 5))  # common.c:54-56


# every literal width at five windows, plus the pairs whose minimum match is 3 (literal 5 at 2^11..2^15, literal 6 at
# 2^13..2^15, literal 7 at 2^15)
MINP3 = [(w, lit) for w in range(8, 16) for lit in range(5, 9) if min_pattern_size(w, lit) == 3]
PAIRS = sorted({(w, lit) for w in (8, 10, 13, 14, 15) for lit in (5, 6, 7, 8)} | set(MINP3))


def b64(b: bytes) -> str:
    return base64.b64encode(b).decode()


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def _name(kind, literal, n):
    return f"{kind}&{(1 << literal) - 1}:{n}" if literal < 8 else f"{kind}:{n}"


def source(pieces) -> bytes:
    """[[workload, row], ...] -> the rows' bytes, concatenated (also used by the tests)."""
    return b"".join(workload_rows(name)(row + 1)[row].tobytes() for name, row in pieces)


def source_pieces(literal, k):
    """Text, long runs (stress row 1), long repeats (stress row 2), short runs, random bytes (stress row 0), more text."""
    return [[_name("synth_text", literal, 1500), k % 5], [_name("stress", literal, 700), 1 + 3 * (k % 2)],
            [_name("stress", literal, 1800), 2 + 3 * (k % 2)], [_name("lcg_runs", literal, 500), k % 4],
            [_name("stress", literal, 300), 3 * (k % 2)], [_name("synth_text", literal, 1000), 5 + k % 5]]


def dictionary_pieces(window, literal, k):
    return [[_name("synth_text", literal, 1 << window), 10 + k % 3]]


def stream_scripts():
    """(name, conf, dictionary pieces or None, source pieces, ops) -- ops index the source: ["write", start, end].
    Every pair in both formats; one script in four adds a custom dictionary, dictionary_reset or lazy matching."""
    out = []
    rng = random.Random(20261016)
    for k, (w, lit) in enumerate(PAIRS):
        for ext in (True, False):
            tag = ("plain", "dict", "reset", "lazy")[(k + 2 * (not ext)) % 4]
            conf = dict(window=w, literal=lit, extended=ext)
            if tag == "reset":
                conf["dictionary_reset"] = True
            if tag == "lazy":
                conf["lazy_matching"] = True
            pieces = source_pieces(lit, k + int(ext))
            n = len(source(pieces))
            ops, pos = [], 0
            while pos < n:
                x = rng.random()
                if x < 0.8:
                    m = rng.choice([1, 17, 300, 700, 1500, 2500])
                    ops.append(["write", pos, min(n, pos + m)])
                    pos = min(n, pos + m)
                elif x < 0.93 or tag != "reset":
                    ops.append(["flush", rng.random() < 0.85])
                else:
                    ops.append(["reset"])
            ops.append(["close"] if rng.random() < 0.5 else ["flush", False])
            dpieces = dictionary_pieces(w, lit, k) if tag == "dict" else None
            out.append((f"w{w}_l{lit}_{'ext' if ext else 'v1'}_{tag}", conf, dpieces, pieces, ops))
    return out


def encoder_scripts():
    """(name, conf, dictionary pieces or None, source pieces, patch, ops) -- ops index the source (["compress", start,
    end, cap], ["sink", start, end], ["compress_and_flush", start, end, write_token, cap], ["poll", cap], ["flush",
    write_token, cap]); `patch` = [position, byte] puts a byte above the literal width into the source, or None."""
    out = []
    rng = random.Random(4712)
    pairs = MINP3 + [(8, 5), (8, 6), (10, 6), (10, 7), (13, 7), (13, 8), (14, 7), (14, 8), (8, 8), (10, 8)]
    for k, (w, lit) in enumerate(pairs):
        conf = dict(window=w, literal=lit, extended=k % 3 != 2)
        if k % 5 == 1:
            conf["lazy_matching"] = True
        if k % 4 == 3:
            conf["dictionary_reset"] = True
        pieces = source_pieces(lit, k)
        n = len(source(pieces))
        p_token = 0.7 if k % 3 == 0 else 1.0  # (a flush without its token pads mid-stream: most scripts stay decodable)
        ops, pos = [], rng.randrange(0, 400)
        for _ in range(rng.randrange(15, 30)):
            kind = rng.choice(["compress", "compress", "compress", "compress", "poll", "sink", "flush", "compress_and_flush"])
            cap = rng.choice([0, 1, 2, 3, 5, 6, 8, 20]) if rng.random() < 0.35 else rng.choice([64, 300])
            m = rng.choice([1, 3, 15, 16, 17, 40, 100])
            rg = [pos, pos + m]
            pos = (pos + m) % (n - 400)
            if kind == "compress":
                ops.append(["compress"] + rg + [cap])
            elif kind == "poll":
                ops.append(["poll", cap])
            elif kind == "sink":
                ops.append(["sink"] + rg)
            elif kind == "flush":
                ops.append(["flush", rng.random() < p_token, cap])
            else:
                ops.append(["compress_and_flush"] + rg + [rng.random() < p_token, cap])
        ops.append(["flush", True, 400])
        out.append((f"w{w}_l{lit}_{'ext' if conf['extended'] else 'v1'}_{k}", conf, None, pieces, None, ops))
    # a custom dictionary at a minimum match of 3, and a byte above the literal width in the middle of a piece
    for w, lit, ext in ((13, 5, True), (15, 6, False)):
        ops = [["compress", i, i + 300, 64] for i in range(0, 1800, 300)] + [["flush", True, 64]]
        out.append((f"w{w}_l{lit}_custom_dictionary", dict(window=w, literal=lit, extended=ext),
                    dictionary_pieces(w, lit, w), source_pieces(lit, w), None, ops))
    for w, lit in ((11, 5), (10, 5), (14, 6), (8, 6)):
        ops = [["compress", 0, 700, 64], ["compress", 700, 1000, 64], ["compress", 1000, 1100, 64], ["flush", False, 64]]
        out.append((f"w{w}_l{lit}_excess_bits", dict(window=w, literal=lit, extended=w % 2 == 1), None,
                    source_pieces(lit, w), [1037, 1 << lit], ops))
    return out


def patched(src, patch):
    if patch is None:
        return src
    b = bytearray(src)
    b[patch[0]] = patch[1]
    return bytes(b)


def encoder_op(op, src):
    """A script op with its source range replaced by the bytes (the form Ref.encode_script takes)."""
    if op[0] in ("compress", "sink", "compress_and_flush"):
        return (op[0], src[op[1] : op[2]]) + tuple(op[3:])
    return tuple(op)


def main():
    ref = Ref()
    assert ref.sizes() == (2, 48, 24), ref.sizes()
    streams, encoders = [], []
    for name, conf, dpieces, pieces, ops in stream_scripts():
        src = source(pieces)
        d = source(dpieces) if dpieces else None
        st, got = ref.stream_script([("write", src[op[1] : op[2]]) if op[0] == "write" else tuple(op) for op in ops],
                                    dictionary=d, **conf)
        assert st == 0, (name, st)
        plain = b"".join(src[op[1] : op[2]] for op in ops if op[0] == "write")
        # a FLUSH without its token pads mid-stream: only scripts without one decode back to their writes
        decodes = not any(op == ["flush", False] for op in ops[:-1])
        if decodes:
            dst, back, _ = ref.decompress(got, dictionary=d, cap=len(plain) + 64)
            assert dst == 2 and back == plain, name
        streams.append(dict(name=name, conf=conf, source=dict(pieces=pieces, sha256=sha(src)),
                            dictionary=dict(pieces=dpieces, sha256=sha(d)) if dpieces else None, ops=ops, status=st,
                            expected_len=len(got), expected_sha256=sha(got), decodes=decodes))
    for name, conf, dpieces, pieces, patch, ops in encoder_scripts():
        src = patched(source(pieces), patch)
        d = source(dpieces) if dpieces else None
        r0, calls = ref.encode_script([encoder_op(op, src) for op in ops], dictionary=d, **conf)
        assert r0 == 0, name
        encoders.append(dict(name=name, conf=conf, source=dict(pieces=pieces, patch=patch, sha256=sha(src)),
                             dictionary=dict(pieces=dpieces, sha256=sha(d)) if dpieces else None, ops=ops, init=r0,
                             emitted=b64(b"".join(out for _, out, _ in calls)),
                             calls=[[r, len(out), k] for r, out, k in calls]))
    assert any(c[0] == -2 for rec in encoders for c in rec["calls"])
    with open(PATH, "w") as f:  # one record per line
        f.write('{"note": "outputs of oracle/_ref/libtamp_ref.so (reference C, -O3, TAMP_LAZY_MATCHING=1); '
                'tests/golden/make_config_matrix.py",\n')
        for key, recs in (("streams", streams), ("encoders", encoders)):
            f.write(f'"{key}": [\n' + ",\n".join(json.dumps(r, sort_keys=True) for r in recs) + "\n]")
            f.write(",\n" if key == "streams" else "\n}\n")
    print(os.path.basename(PATH), os.path.getsize(PATH), len(streams), "stream scripts,", len(encoders), "encoder scripts")


if __name__ == "__main__":
    main()
