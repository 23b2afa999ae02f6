#!/usr/bin/env python3
"""Host-side replay of the fixed-geometry compress build's match phase: how evenly the sorted query groups load the four wavefronts.

The brackets are replayed as tools/hash_search.py replays them (tile-ordered buckets, 1,024 buckets, the W = 2^10 build's
multiplier, 256-position tiles, the default dictionary as the first window) on epochs cut from the benchmark's synthetic text.  A
query scans min(bracket, 63) entries; the queries of an epoch are sorted by that length, longest first, and run in groups of 64
whose lanes loop in lock step: a group costs its longest bracket.  Per epoch the script sums the groups each of the four
wavefronts runs under three orders --

  straight   wavefront w runs groups w, w + 4, w + 8, ...  (the strided loop)
  snake      odd rows of four groups reversed
  on demand  a wavefront that is done takes the next group (kClaim)

-- and prints the four sums of the straight order, their mean, and the longest wavefront of each order: the workgroup waits for
that one at the barrier behind the phase.  It also prints where the scanned entries come from (window and bucket, same bigram,
the query's own entry, tile slack) and the entries scanned with smaller tiles.  CPU only.
usage: wave_balance.py [streams]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tamp_amd  # noqa: E402
from tamp_amd import workloads as wl  # noqa: E402

W, BLK, HB, M, CAP, WAVES = 1024, 1024, 10, 5455, 63, 4
DICT = np.frombuffer(bytes(tamp_amd.initialize_dictionary(W)), dtype=np.uint8)


def epochs(rows):
    """(bigram of every buffer position, positions matched) per epoch: the window, then the block."""
    out = []
    for r in rows:
        hist = np.concatenate([DICT, r]).astype(np.uint32)
        for e0 in range(0, len(r), BLK):
            nv = min(BLK, len(r) - e0)
            buf = hist[e0:e0 + W + nv + 1]
            buf = np.concatenate([buf, np.zeros(W + nv + 1 - len(buf), dtype=np.uint32)])
            out.append((buf[:W + nv] | (buf[1:W + nv + 1] << 8), nv))
    return out


def brackets(big, nv, tile):
    """Entries between a query's two cursor snapshots: its bucket's entries from the tile of its oldest window byte to its own."""
    NE = W + nv
    h = ((big * M) & 0xFFFF) >> (16 - HB)
    t = np.arange(NE) // tile
    nt = (NE + tile - 1) // tile
    C = np.bincount(h * (nt + 1) + t + 1, minlength=(1 << HB) * (nt + 1)).reshape(1 << HB, nt + 1)
    P = np.cumsum(C, axis=1)  # P[b, t] = entries of bucket b in tiles < t
    q = np.arange(nv)
    bq = h[W + q]
    return P[bq, (W + q) // tile + 1] - P[bq, q // tile], h


def orders(groups):
    """Per-wavefront sums of the straight order, and the longest wavefront of the straight, snake and on-demand orders."""
    pad = (-len(groups)) % WAVES
    rows = np.concatenate([groups, np.zeros(pad, dtype=groups.dtype)]).reshape(-1, WAVES)
    straight = rows.sum(axis=0)
    snake = rows.copy()
    snake[1::2] = snake[1::2, ::-1]
    free = np.zeros(WAVES, dtype=np.int64)
    for g in groups:  # (ties: the lowest wavefront; any rule gives the same longest sum within one group's cost)
        free[np.argmin(free)] += g
    return straight, snake.sum(axis=0).max(), free.max()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    eps = epochs(wl.synth_text(n, 4096))
    per_wave = np.zeros(WAVES)
    first = snake = demand = 0.0
    scanned = in_win = same = nq = 0
    for big, nv in eps:
        L, h = brackets(big, nv, 256)
        s = np.sort(np.minimum(L, CAP))[::-1]
        s = np.concatenate([s, np.zeros((-len(s)) % 64, dtype=s.dtype)]).reshape(-1, 64)
        groups = s.max(axis=1)
        st, sn, dm = orders(groups)
        per_wave += st
        first += groups[0]
        snake += sn
        demand += dm
        scanned += int(L.sum())
        nq += nv
        for q in range(nv):  # the window's index positions q .. q + W - 2, and the query's own entry
            win = slice(q, q + W - 1)
            hit = h[win] == h[W + q]
            in_win += int(hit.sum())
            same += int((hit & (big[win] == big[W + q])).sum())
    ne = len(eps)
    print(f"{n} streams, {ne} epochs, {scanned / nq:.2f} entries scanned per query")
    print("lock-step iterations per epoch, straight order, wavefronts 0..3: " + " / ".join(f"{v / ne:.1f}" for v in per_wave))
    print(f"  mean of the four {per_wave.sum() / ne / WAVES:.1f}, the first group alone {first / ne:.1f}")
    print(f"  longest wavefront: straight {per_wave.max() / ne:.1f}, snake {snake / ne:.1f}, on demand {demand / ne:.1f}")
    print(f"of the {scanned / nq:.2f}: {in_win / nq:.2f} in the window and the bucket ({same / nq:.2f} with the query's bigram), "
          f"1.00 the query's own entry, {scanned / nq - in_win / nq - 1:.2f} tile slack")
    for tile in (128, 64):
        sc = lock = 0
        for big, nv in eps:
            L, _ = brackets(big, nv, tile)
            s = np.sort(L)[::-1]
            s = np.concatenate([s, np.zeros((-len(s)) % 64, dtype=s.dtype)]).reshape(-1, 64)
            sc, lock = sc + int(L.sum()), lock + int(s.max(axis=1).sum())
        print(f"{tile}-position tiles: {sc / nq:.2f} entries scanned per query, {lock * 64 / nq:.2f} lock-step iterations per 64 queries")


if __name__ == "__main__":
    main()
