"""Inputs of the tight-output tests (tests/test_oracle_vs_reference.py, tests/test_gpu_tight_output.py), built in code from a
seed and a word list, and the rule both tiers check.

THE RULE (include/tamp_amd.h, tamp_batch_compress).  T = the stream's length with ample room (for a stream that ends with
TAMP_EXCESS_BITS: the whole bytes in front of the offending literal), S = its status with ample room.  With ``cap`` bytes of room
the stream ends with (TAMP_OUTPUT_FULL, its first ``cap`` bytes) when ``cap < T`` and with (S, all T bytes) otherwise.

Every input mixes words, runs of one byte and repeats of earlier text that are long enough for an extended match, so that RLE
and extended-match tokens straddle the capacities of a sweep; ``tail`` says what the stream ends in (a run and a repeat are still
pending when the input ends: the drain emits them).  All bytes are masked to ``literal`` bits; ``offending`` puts one byte of
``1 << literal`` back in.
"""
import functools
import random

OK, OUTPUT_FULL, EXCESS_BITS = 0, 1, -2

WORDS = ("sensor valve depth north queue stage pixel frame delta gamma orbit laser motor probe relay timer "
         "a of to in it is on at by we").split()

BLOCK = 1024                  # positions per epoch of every long-stream build at max_in_len = 1024 (tamp_amd_compress_plan)
LONG_LEN = 5 * BLOCK // 2     # "2.5 blocks": two full epochs and a half one
BEHIND_BOUNDARY = BLOCK + 1   # an offending byte just behind the first epoch boundary


@functools.lru_cache(maxsize=None)
def text(n, seed):
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += rng.choice(WORDS).encode() + (b" " if rng.random() < 0.8 else b", ")
    return bytes(out[:n])


def _mask(data, literal):
    return bytes(b & ((1 << literal) - 1) for b in data)


def rule(status, full, cap):
    """What ``cap`` bytes of room give a stream whose ample-room result is (status, full)."""
    return (OUTPUT_FULL, full[:cap]) if cap < len(full) else (status, full)


def offending(data, literal, pos):
    """``data`` with a byte one bit above the literal width at ``pos``: TAMP_EXCESS_BITS there."""
    assert literal < 8 and 0 <= pos < len(data)
    b = bytearray(data)
    b[pos] = 1 << literal
    return bytes(b)


def sample(n, literal=8, tail="run"):
    """``n`` bytes: words, a run, a repeat of the words at the front, and ``tail`` ("run" | "repeat" | "text") at the end."""
    if n <= 2:
        return _mask(text(n, 3), literal)
    n_text, n_run, n_tail = (2 * n + 4) // 5, n // 6, max(2, n // 8)
    n_rep = n - n_text - n_run - n_tail
    front = text(n_text, 5)
    rep = (front * 2)[n_text // 5 : n_text // 5 + n_rep]
    end = {"run": b"z" * n_tail, "repeat": (front * 2)[1 : 1 + n_tail], "text": text(n_tail, 7)}[tail]
    out = front + b"r" * n_run + rep + end
    assert len(out) == n
    return _mask(out, literal)


def short_input(literal=8):
    """300 bytes: words, a run of 40, words, a 60-byte repeat of the front (an extended match), a trailing run of 20."""
    t = text(120, 1)
    out = t[:100] + b"r" * 40 + t[100:] + text(60, 2) + t[20:80] + b"z" * 20
    assert len(out) == 300
    return _mask(out, literal)


def long_input(literal=8):
    """LONG_LEN bytes = 2.5 blocks of 1,024 positions: a run across the first block boundary, a repeat across the second, a
    300-byte repeat of the front (extended matches at their cap), a run of 100, and a trailing run of 20."""
    a = text(700, 11)
    out = bytearray(a)                      # [0, 700)
    out += b"a" * 60 + text(200, 12)        # [700, 960)
    out += a[100:160]                       # [960, 1020)
    out += b"b" * 30                        # [1020, 1050): across 1,024
    mid = text(500, 13)
    out += mid                              # [1050, 1550)
    out += a[:300] + text(150, 14)          # [1550, 2000)
    out += mid[:100]                        # [2000, 2100): across 2,048
    out += text(300, 15) + b"c" * 100       # [2100, 2500)
    out += text(40, 16) + b"z" * 20
    assert len(out) == LONG_LEN
    return _mask(bytes(out), literal)


def with_offenders(data, literal, positions):
    """[data] for literal 8, else data and one copy per position with the offending byte there."""
    if literal == 8:
        return [data]
    return [data] + [offending(data, literal, p) for p in sorted({p for p in positions if 0 <= p < len(data)})]


# Lengths of the CPU tier and what each ends in.  120 is there for the reference's widest margin: with the offending byte last it
# ends in a 14-byte repeat, the shortest extended match (19 bits at window 2^8, two whole bytes), for which the reference wants
# six bytes of room.
CPU_SAMPLES = ((0, "text"), (1, "text"), (2, "text"), (16, "run"), (17, "repeat"), (40, "run"), (120, "repeat"), (300, None),
               (701, "repeat"))


def cpu_inputs(literal):
    out = []
    for n, tail in CPU_SAMPLES:
        data = short_input(literal) if tail is None else sample(n, literal, tail)
        out += with_offenders(data, literal, (0, n // 2, n - 1))
    return out
