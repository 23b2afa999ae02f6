"""Inputs of tests/test_gpu_query_setup.py (what they aim at is checked on the CPU by tests/test_query_setup_input.py).

The fixed-geometry compress builds (window 2^10, literal 8, 1,024-position blocks) load their patterns from one aligned base,
count full quads of the histogram pass apart from the partial quad a range ends with, and run their constant-trip loops as
straight-line stores.  Three texts, each cut at the lengths below:

  text     workloads.synth_text: the headline's input;
  period2  "abab...": two buckets hold every position, the brackets saturate at 63, the cursors cross the 16-bit halves of the
           packed counters, and every position behind the first two has a match;
  runs     a run of 9..40 equal bytes starts every 37 positions of the synthetic text (a run of 37 and more ends where the next
           one, of another byte, starts; every other run is of a byte the window holds no run of): RLE tokens that write fewer bytes than they consume, so epochs start at every residue
           mod 4 behind them, the run cut ends blocks inside them, and the run-list second pass and the settled-token pass
           load their patterns.

Lengths: 1..9 (a stream shorter than a quad, an only epoch with a tail quad of 1, 2, 3), 1021..1031 and 2045..2055 (tail quads
and epochs of a single position at the first and a middle epoch boundary), 4090..4096 (the last epoch).
"""
import numpy as np

L = 4096
LENGTHS = tuple(range(1, 10)) + tuple(range(1021, 1032)) + tuple(range(2045, 2056)) + tuple(range(4090, 4097))
TEXTS = ("text", "period2", "runs")
RESIDUES = (0, 1, 2, 3)
RUN_PERIOD, RUN_MIN, RUN_MAX = 37, 9, 40

_cache = {}


def text(name):
    """The L bytes of text `name`; streams are prefixes of it."""
    if name not in _cache:
        from tamp_amd import workloads as wl

        base = wl.synth_text(1, L)[0].tobytes()
        if name == "text":
            data = base
        elif name == "period2":
            data = b"ab" * (L // 2)
        elif name == "runs":
            buf = bytearray(base)
            for k, p in enumerate(range(0, L, RUN_PERIOD)):
                r = RUN_MIN + (k * 7) % (RUN_MAX - RUN_MIN + 1)
                # (every other run of a byte the window has no run of: that one has no match to lose against)
                buf[p:p + r] = bytes([b"xyzq-_"[k % 6] if k % 2 == 0 else 0x80 + k % 64]) * r
            data = bytes(buf[:L])
        else:
            raise KeyError(name)
        assert len(data) == L
        _cache[name] = data
    return _cache[name]


def items():
    """[(text, length, residue)]: every text at every length, once at each batch offset in_off = residue (mod 4)."""
    return [(t, n, r) for t in TEXTS for n in LENGTHS for r in RESIDUES]


def layout(its, fill=0xA5):
    """-> (flat uint8, in_off uint64, in_len uint32): stream i at an offset with in_off[i] % 4 == its residue, `fill` bytes in the
    gaps (1..7 of them, and 8 behind the last stream)."""
    chunks, offs, pos = [], [], 0
    for t, n, r in its:
        pad = 1 + (r - (pos + 1)) % 4
        chunks.append(bytes([fill]) * pad)
        pos += pad
        assert pos % 4 == r
        offs.append(pos)
        chunks.append(text(t)[:n])
        pos += n
    chunks.append(bytes([fill]) * 8)
    flat = np.frombuffer(b"".join(chunks), dtype=np.uint8)
    return flat, np.asarray(offs, dtype=np.uint64), np.asarray([n for _, n, _ in its], dtype=np.uint32)
