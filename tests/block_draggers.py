"""Inputs that drag every kind of token across every epoch boundary (a plain helper for both test tiers, no fixtures).

The compress kernel matches one block of positions per epoch; with blocks that are multiples of 64, features that recur at
periods coprime to 64 meet a block's last positions, its 16-byte look-ahead and the stream's tail at every offset within
a few KB: plain matches, RLE runs on both sides of kLongRun = 8, kRleWindowMax = 8 and kRleMax = 241, extended matches
around min + 11 and min + 131 bytes, periodic data whose matches run into the window's end, all literals, and short runs
so dense that one block holds more slow positions than the walk lists in one segment.
"""
import numpy as np

from tamp_amd import workloads as wl

RUN_LENGTHS = (2, 3, 7, 8, 9, 10, 12, 13, 16, 17, 30, 64, 240, 241, 242, 243, 300)
COPY_LENGTHS = (14, 15, 16, 17, 18, 19, 20, 40, 133, 134, 135, 136, 150)
PERIODS = (1, 2, 3, 37, 255, 257)
CUT_DELTAS = (-17, -16, -15, -1, 0, 1, 15, 16, 17)
CUT_NAMES = ("text", "runs67", "repeat131")


def _text(n, row):
    return wl.synth_text(1, max(n, 1), first_index=row, threads=1)[0].tobytes()[:n]


def _runs67(n, seed):
    src = _text(n + 128, 1000 + seed)
    out, k, p = bytearray(), 0, 0
    while len(out) < n:
        r = RUN_LENGTHS[k % len(RUN_LENGTHS)]
        plain = max(67, r + 29) - r
        out += src[p:p + plain]
        p += plain
        out += bytes([b"-= *_#x"[k % 7]]) * r
        k += 1
    return bytes(out[:n])


def _repeat131(n, seed):
    out = bytearray(_text(200, 2000 + seed))
    fresh = _text(n + 64, 3000 + seed)
    k, p = 0, 0
    while len(out) < n:
        m = COPY_LENGTHS[k % len(COPY_LENGTHS)]
        dist = 1 + (131 * k) % min(len(out) - 1, 900)
        for _ in range(m):  # (byte by byte: a copy may overlap itself)
            out.append(out[len(out) - dist])
        f = 3 + k % 7
        out += fresh[p:p + f]
        p += f
        k += 1
    return bytes(out[:n])


def draggers(n, seed=0):
    """-> {name: bytes of length n}, the same for the same (n, seed)."""
    rng = np.random.default_rng(1000003 * seed + 17)
    prose = wl.real_text("prose", frozen_only=True)
    assert len(prose) >= (1 << 20), "frozen prose corpus fixture missing"
    at = 4099 * (seed + 1)
    stress = wl.stress(3, max(n, 1), first_index=3 * seed, threads=1)
    out = {
        "text": _text(n, seed),
        "prose": prose[at:at + n],
        "runs67": _runs67(n, seed),
        "repeat131": _repeat131(n, seed) if n > 200 else _text(n, 2000 + seed),
    }
    for p in PERIODS:
        phrase = prose[at + 7001:at + 7001 + p]
        out["period%d" % p] = (phrase * (n // p + 1))[:n]
    out["random"] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    out["lcg_runs"] = wl.lcg_runs(1, max(n, 1), first_index=seed, threads=1)[0].tobytes()[:n]
    out["pairs"] = np.repeat(rng.integers(97, 123, n // 2 + 1, dtype=np.uint8), 2).tobytes()[:n]
    out["triples"] = np.repeat(rng.integers(97, 101, n // 3 + 1, dtype=np.uint8), 3).tobytes()[:n]
    # (the workload generator's own long runs and long repeats: rows 1 and 2 of its three shapes)
    out["stress_runs"] = stress[1].tobytes()[:n]
    out["stress_repeats"] = stress[2].tobytes()[:n]
    assert all(len(v) == n for v in out.values())
    return out


def masked(data, literal):
    """`data` with every byte cut to `literal` bits (a wider byte is TAMP_EXCESS_BITS, which is not what these inputs test)."""
    if literal >= 8:
        return data
    return (np.frombuffer(data, dtype=np.uint8) & np.uint8((1 << literal) - 1)).tobytes()


def cut_lengths(blk, m, n):
    """The lengths around m blocks that put the stream's tail and the 16-byte look-ahead on both sides of a block's end."""
    return [m * blk + d for d in CUT_DELTAS if 0 < m * blk + d <= n]
