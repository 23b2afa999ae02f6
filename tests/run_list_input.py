"""Inputs aimed at the run list of the run-aware compress builds (a plain helper for both test tiers, no fixtures).

The run-aware builds take the interior a+1 .. b-4 of every LISTED run [a, b) of kLongRun and more equal bytes out of the
bigram index; the second pass of the match phase (tamp_compress_kernel.hpp, the `if (nruns)` block behind the bucket scan)
puts the candidates back by arithmetic on the run record, in three branches around cs = b - rq.  At most kRunCap runs are
listed per epoch, in the order an LDS atomicAdd hands the slots out; further runs stay fully indexed.

``second_pass_key``  the second pass restated as the kernel writes it, returning which branch and shortcut won;
``exhaustive_key``   the same question answered by comparing bytes at every interior position;
``family_a``         v1 streams "one run, one query", each aimed at one cell of the second pass;
``family_b``         run fields dense enough that every epoch sees more than kRunCap long runs;
``family_c``         the same shape, sparse enough that every run is listed;
``*_predicate``      what the inputs must be for those claims to hold, from the raw bytes alone.

v1 (extended = False) writes every consumed byte to the window, so input position p has window index p mod W there and the
geometry below is exact.  In the extended format an RLE token writes at most 8 bytes and an extended match may be clipped at
the ring end, so only the predicate "more than kRunCap long runs in every W consecutive bytes" carries over (a run of 8 and
more still leaves 8 or 9 equal bytes in the window).
"""
import functools
from collections import namedtuple

import numpy as np

K_RUN_CAP, K_LONG_RUN = 128, 8  # kRunCap, kLongRun of tamp_compress_kernel.hpp (tests/test_run_list_input.py reads the header)
RING = 16                       # kRing: the look-ahead, and the longest compare
LENGTHS = (8, 9, 12, 16, 17, 24, 40)
RQS = tuple(range(2, 18))
BELOW, CS, ABOVE = "below", "cs", "above"
RUN_BYTES = b"#%@=~_"           # never in the synthetic text, the initial dictionary, the tails or the marker
TAIL, OTHER, MARK = b"QZ", b"KV", b"J"


# ---------------------------------------------------------------------------------------------------------------------
# the second pass, restated
# ---------------------------------------------------------------------------------------------------------------------
def lcp(buf, c, qpos, cap=RING):
    n = 0
    while n < cap and buf[c + n] == buf[qpos + n]:
        n += 1
    return n


def lcp_wrapped(buf, c, t, W, qpos):
    """prefix_len_wrapped16: candidate byte k is buf[c + k] in front of the newest window byte (k < t), then the OLDEST ones."""
    n = 0
    while n < RING and buf[c + n if n < t else c - W + n] == buf[qpos + n]:
        n += 1
    return n


def listed_runs(buf, NE):
    """The runs the kernel's listing finds in an epoch buffer that indexes positions 0 .. NE-1: heads in front of NE, ends capped at
    NE + 16, kLongRun bytes and more -> [(a, b)].  (All of them: which kRunCap of them get a slot is the device's business.)"""
    a = np.frombuffer(bytes(buf[:NE + RING]), dtype=np.uint8)
    if a.size == 0:
        return []
    heads = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
    ends = np.concatenate((heads[1:], [a.size]))
    keep = (ends - heads >= K_LONG_RUN) & (heads < NE)
    return [(int(h), int(e)) for h, e in zip(heads[keep], ends[keep])]


Won = namedtuple("Won", "c branch flags how run")  # flags: subset of {"idx0", "wrap", "lo", "lim"}; how: "rq" "rq+1" "cmp" "rc" "wrapped"


def _flags(**kw):
    return frozenset(k for k, v in kw.items() if v)


def second_pass_key(buf, q, W, wp_e, cap_len, runs, weaken=None):
    """The kernel's second pass for the query at buffer position W + q (window = buf[q : q + W], window index of buffer position
    c = (c + wp_e) mod W), over the listed ``runs`` [(a, b)], starting from "no match".  -> (key, Won or None) with
    key = length << 16 | (W - index), as the match phase reduces it.  ``weaken``: None, or one of "no_cz", "rq_plus_1", "no_lim" --
    a deliberately wrong copy, for the test that the inputs can tell (never anything the kernel does)."""
    mask, qpos = W - 1, W + q
    x = buf[qpos]
    if buf[qpos + 1] != x:
        return 0, None
    rq = lcp(buf, qpos, qpos + 1, RING - 1) + 1  # the pattern's own leading run, 2..16
    key, won = 0, None
    left_out = set()
    for a, b in runs:
        left_out.update(range(a + 1, b - 3))

    def clip_of(c):  # "may not run past index W-1"
        return W if weaken == "no_lim" else W - ((c + wp_e) & mask)

    # wrap zone: the left-out positions t = 2..15 bytes in front of the window's end that hold x
    for t in range(2, RING):
        c = q + W - t
        if c not in left_out or buf[c] != x:
            continue
        i = (c + wp_e) & mask
        if i == mask:
            continue
        lw = lcp_wrapped(buf, c, t, W, qpos)
        ln = min(lw, cap_len, clip_of(c))
        k = (ln << 16) | (W - i)
        if ln >= 2 and k > key:
            run = next(r for r in runs if r[0] < c < r[1])
            cs = run[1] - rq
            key = k
            won = Won(c, BELOW if c < cs else (CS if c == cs else ABOVE),
                      _flags(wrap=True, idx0=i == 0, lim=W - i < min(lw, cap_len)), "wrapped", run)
    cz = q + ((-wp_e - q) & mask)  # the window position with index 0
    qhi = q + W - RING
    pb2 = (buf[qpos + rq], buf[qpos + rq + 1]) if rq < RING else None  # the pattern's two bytes behind ITS run
    for a, b in runs:
        lo, hi = max(a + 1, q), min(b - 4, qhi)
        if buf[a] != x or lo > hi:
            continue
        cs = b - rq
        cz_in = lo <= cz <= hi
        cands = []  # (candidate, branch, length before the limits, how)
        hiA = min(hi, cs - 1)
        if lo <= hiA:  # below cs: exactly rq bytes wherever it starts, the lowest index decides
            c = cz if (cz_in and cz <= hiA and weaken != "no_cz") else lo
            cands.append((c, BELOW, rq, "rq"))
        if lo <= cs <= hi:  # cs itself: goes on behind the run; the two bytes kept with the run record decide whether to look
            ln, how = rq, "rq"
            if rq < RING and buf[b] == pb2[0]:
                if buf[b + 1] != pb2[1]:
                    ln, how = (rq if weaken == "rq_plus_1" else rq + 1), "rq+1"
                else:
                    ln, how = lcp(buf, cs, qpos), "cmp"
            cands.append((cs, CS, ln, how))
        c1 = max(lo, cs + 1)
        if c1 <= hi:  # above cs: the run remainder, shrinking; the first one, or index 0 behind it
            cands.append((c1, ABOVE, b - c1, "rc"))
            if cz_in and cz > c1:
                cands.append((cz, ABOVE, b - cz, "rc"))
        for c, branch, ln, how in cands:
            lim_i = W - ((c + wp_e) & mask)
            k = (min(ln, cap_len, clip_of(c)) << 16) | lim_i
            if k > key:
                key = k
                won = Won(c, branch, _flags(idx0=c == cz, lo=c == lo and q > a + 1, lim=lim_i < min(ln, cap_len)), how, (a, b))
    if key >> 16 < 2:
        return 0, None
    return key, won


def exhaustive_key(buf, q, W, wp_e, cap_len, runs):
    """The best key over EVERY interior position of the listed runs of the pattern's byte inside the window, bytes compared one
    by one (the newest window byte itself, t = 1, is the first pass's) -> (key, position)."""
    mask, qpos = W - 1, W + q
    x = buf[qpos]
    if buf[qpos + 1] != x:
        return 0, None
    best, at = 0, None
    for a, b in runs:
        if buf[a] != x:
            continue
        for c in range(max(a + 1, q), min(b - 4, q + W - 2) + 1):
            t = q + W - c
            i = (c + wp_e) & mask
            ln = min(lcp(buf, c, qpos) if t >= RING else lcp_wrapped(buf, c, t, W, qpos), cap_len, W - i)
            k = (ln << 16) | (W - i)
            if ln >= 2 and k > best:
                best, at = k, c
    return best, at


def epoch_view(data, p, W, blk, dictionary):
    """The epoch buffer in which the kernel answers the query at input position ``p`` of a v1 stream: blocks of ``blk`` positions,
    each behind the W window bytes in front of it (the dictionary first) -> (buf, q, wp_e, cap_len, runs, base) with buffer
    position c = input position c + base.  cap_len for literal 8, windows up to 2^14: min 2, so 15 bytes at most."""
    n = len(data)
    k = p // blk
    nvalid = min(blk, n - k * blk)
    full = bytes(dictionary) + bytes(data) + bytes(2 * RING + 16)
    buf = full[k * blk:k * blk + W + nvalid + 2 * RING + 16]
    return buf, p - k * blk, (k * blk) & (W - 1), min(n - p, 15), listed_runs(buf, W + nvalid), k * blk - W


# ---------------------------------------------------------------------------------------------------------------------
# family A: one run, one query
# ---------------------------------------------------------------------------------------------------------------------
OneRun = namedtuple("OneRun", "data a b pq rq agree aim")  # the run is data[a:b], the query starts at pq


@functools.lru_cache(maxsize=None)
def _text(row, n=6000):
    from tamp_amd import workloads as wl

    return wl.synth_text(1, n, first_index=7000 + row, threads=1)[0].tobytes()


def one_run(W, L, rq, agree, P, F, aim, k=0, tail=40):
    """prefix of P text bytes | x^L | two tail bytes | F filler bytes (the last one a byte that occurs nowhere else) | x^rq |
    two bytes that agree with the run's tail in ``agree`` positions | text.  agree = 3: both, and the bytes behind them repeat
    the filler and then the OLDEST window bytes, so that a candidate in the wrap zone goes on around the ring."""
    x = RUN_BYTES[k % len(RUN_BYTES):][:1]
    pre, fill, post = _text(k % 7)[:P], _text(7 + k % 5)[:max(F - 1, 0)] + (MARK if F else b""), _text(12 + k % 3)[:tail]
    a, b = P, P + L
    pq = b + 2 + F
    behind = (TAIL, TAIL[:1] + OTHER[1:], OTHER, TAIL)[agree]
    data = pre + x * L + TAIL + fill + x * rq + behind
    if agree == 3:
        oldest = data[pq - W:pq - W + 8] if pq >= W else b""
        post = (fill + oldest + post)[:max(tail, 0)]
    data += post
    assert len(pre) == P and len(fill) == F and data[pq:pq + rq] == x * rq and data[pq - 1:pq] != x
    return OneRun(data, a, b, pq, rq, agree, aim)


@functools.lru_cache(maxsize=None)
def family_a(window):
    """The streams of family A at this window, each aimed (``aim``) at a cell of the second pass:
      idx0   the run lies wholly inside the window and window index 0 falls z bytes into it -- below, on and above cs, on the head, in
             the indexed tail, behind the run: the candidates in front of index 0 are clipped by W - index, index 0 itself is cz;
      wrap   the run ends within 15 bytes of the query; index 0 outside the run, or on one of its wrap-zone candidates;
      lo     the run begins in front of the oldest window byte, which is s bytes into it (lo clipped to q);
      tail   the stream ends 0..3 bytes behind the query's two bytes (the look-ahead cap).
    """
    W = 1 << window
    out, k = [], 0

    def add(*a, **kw):
        nonlocal k
        out.append(one_run(W, *a, k=k, **kw))
        k += 1

    for L in LENGTHS:
        for rq in RQS:
            near_cs = {L - rq + d for d in (-2, -1, 0, 1, 2, 3)}
            for z in range(-2, L + 3):  # index 0 at run offset z
                edge = z <= 1 or z >= L - 5
                for agree in (0, 1, 2):
                    if edge or z in near_cs or (z + agree) % 3 == 0:
                        add(L, rq, agree, W - z, 40, "idx0")
    for F in range(0, 10):
        for j in range(4, 14 - F):  # index 0 on the wrap-zone candidate b - j (t = j + 2 + F)
            for L in (12, 40):
                if L < j + 1:
                    continue
                for rq in sorted({j - 2, j - 1, j, j + 1, j + 3} & set(RQS)):
                    for agree in (0, 2, 3):
                        add(L, rq, agree, W - (L - j), F, "wrap")
        for L in (12, 17, 40):
            for rq in RQS:
                for agree in (0, 2, 3):
                    add(L, rq, agree, W - 150 if window > 8 else W + 70, F, "wrap")
    for L in LENGTHS:
        for s in range(1, L - 2):  # the oldest window byte is run offset s
            rem = L - s
            for rq in sorted({rem - 2, rem - 1, rem, rem + 1, rem + 2, 2, 16, 17} & set(RQS)):
                for agree in (0, 1, 2):
                    add(L, rq, agree, 100 + (rq * 7 + s) % 23, W + s - L - 2, "lo")
    for L in (9, 16, 40):
        for rq in (2, 5, 12, 16):
            for tail in (0, 1, 3):
                for z in (L - rq, 2, -2):
                    add(L, rq, 2, W - z, 40, "tail", tail=tail)
    return tuple(out)


def token_cell(s, W, off, length):
    """The cell of a family A stream whose reference token at the query is a match of ``length`` bytes at window offset ``off`` ->
    (input position, branch, flags), or None when the position is not interior to the run."""
    d = (s.pq - off) % W or W
    p = s.pq - d
    if not s.a + 1 <= p <= s.b - 4:
        return None
    cs = s.b - min(s.rq, RING)
    natural = lcp(s.data + bytes(RING), p, s.pq, min(15, len(s.data) - s.pq)) if d >= RING else None  # (a wrap-zone token: not judged here)
    flags = _flags(idx0=p % W == 0, wrap=d < RING, lo=d == W and p > s.a + 1,
                   lim=length == W - p % W and (natural is None or length < natural))
    return p, BELOW if p < cs else (CS if p == cs else ABOVE), flags


_V1_CODES = {}


def v1_token_at(blob, position):
    """Walk the tokens of a v1 stream (literal 8 .. 5 from the header) up to input ``position`` -> (bit at which the token that starts
    there begins, or None when a token straddles the position).  A lean walker: the token itself is then read by
    long_stream_writer.read_tokens, and the two are compared whole on a few streams by the CPU tier."""
    import long_stream_writer as lsw

    if not _V1_CODES:
        for s in range(14):
            nb = lsw.NBITS[s] - 1
            for rest in range(1 << (8 - nb)):
                _V1_CODES[(lsw.CODE[s] << (8 - nb)) | rest] = (s, nb)
    h0 = blob[0]
    window, literal = ((h0 >> 5) & 7) + 8, ((h0 >> 3) & 3) + 5
    assert not h0 & 3, "a plain v1 stream"
    minp = lsw.min_pattern(window, literal)
    total = 8 * (len(blob) + 2)
    v = int.from_bytes(bytes(blob) + b"\0\0", "big")
    t, pos = 8, 0
    while pos < position and t < total - 16:
        if (v >> (total - 1 - t)) & 1:
            t, pos = t + 1 + literal, pos + 1
        else:
            code = _V1_CODES.get((v >> (total - 9 - t)) & 0xFF)
            if code is None:  # (FLUSH: not in front of a query)
                return None
            t, pos = t + 1 + code[1] + window, pos + code[0] + minp
    return t if pos == position else None


# ---------------------------------------------------------------------------------------------------------------------
# families B and C: run fields
# ---------------------------------------------------------------------------------------------------------------------
def run_field(n, seed, same_byte, lengths=(8, 12), gaps=(1, 3), gap_of=None):
    """``n`` bytes of runs of lengths[0]..lengths[1] equal bytes, separated by gaps[0]..gaps[1] other bytes (or ``gap_of(k)``).
    same_byte: every run is of '=' (listed and unlisted runs of one byte compete for every pattern); else the run bytes
    cycle through 41 values.  The separators are lower-case text, never a run byte, never equal to their neighbours' run byte."""
    rng = np.random.default_rng(77003 * seed + 5)
    sep = _text(15 + seed % 4, max(n, 64))
    many = bytes(range(0x21, 0x21 + 41))  # '!' .. 'I': no lower-case letter
    out, k, p = bytearray(), 0, 0
    while len(out) < n:
        g = int(rng.integers(gaps[0], gaps[1] + 1)) if gap_of is None else gap_of(k)
        out += sep[p:p + g]
        p = (p + g) % (len(sep) - 512)
        x = 0x3D if same_byte else many[(k * 7) % len(many)]
        out += bytes([x]) * int(rng.integers(lengths[0], lengths[1] + 1))
        k += 1
    return bytes(out[:n])


def family_b(n, seed, same_byte, dense=False):
    """dense: runs of 8 or 9 bytes, one separator -- for window 2^8, whose epochs (256 + 1,024 + 16 bytes) cannot hold 160 runs."""
    return run_field(n, seed, same_byte, (8, 9), (1, 1)) if dense else run_field(n, seed, same_byte)


def family_c(window, n, seed, same_byte):
    """Runs of 8..40 bytes, spaced so that no W + 2,048 + 16 bytes hold more than about 80 of them."""
    period = max(48, ((1 << window) + 2064) // 80 + 1)
    return run_field(n, seed, same_byte, (8, 40), gap_of=lambda k: period - 40 + (k * 5) % 9)


def long_runs(data):
    """Maximal runs of kLongRun and more bytes of ``data`` -> (starts, ends) as arrays."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    if a.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    heads = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
    ends = np.concatenate((heads[1:], [a.size]))
    keep = ends - heads >= K_LONG_RUN
    return heads[keep], ends[keep]


def runs_in_span(data, lo, hi):
    """Long runs of data[lo:hi] taken on its own (a run cut by the span's edge counts by what is left of it)."""
    return len(long_runs(data[max(lo, 0):hi])[0])


def epoch_run_counts(data, W, blk):
    """Long runs in the span [k*blk - W, (k+1)*blk + 16) of every epoch but the first (v1: the bytes the kernel's epoch buffer holds)."""
    return [runs_in_span(data, k * blk - W, (k + 1) * blk + RING) for k in range(1, (len(data) + blk - 1) // blk)]


def window_run_counts(data, W, step=64):
    """Long runs in spans of W consecutive input bytes, every ``step`` bytes (and the last one)."""
    starts = list(range(0, max(len(data) - W, 0) + 1, step)) + [max(len(data) - W, 0)]
    return [runs_in_span(data, s, s + W) for s in starts]


def overflow_predicate_v1(data, W, blk, at_least=160):
    """Family B, v1: every epoch but the first sees at least 1.25 x kRunCap long runs -> the counts."""
    counts = epoch_run_counts(data, W, blk)
    assert counts and min(counts) >= at_least, (W, blk, counts)
    return counts


def overflow_predicate_window(data, W):
    """Family B, windows of 2^11 and more, either format: every W consecutive input bytes hold more than kRunCap long runs."""
    counts = window_run_counts(data, W)
    assert min(counts) > K_RUN_CAP, (W, min(counts))
    return counts


def all_listed_predicate(data, W, at_most=100):
    """Family C: no span of W + 2,048 + 16 bytes (the largest epoch buffer) holds more than 100 long runs."""
    span = W + 2048 + RING
    counts = [runs_in_span(data, s, s + span) for s in range(0, max(len(data) - span, 0) + 1, 64)]
    assert max(counts) <= at_most, (W, max(counts))
    return counts


BC_SIZES = ((4096, 1), (12288, 2))  # (bytes, seed) of the run fields both tiers use
COPIES = 4


@functools.lru_cache(maxsize=None)
def field_batch(window):
    """The batch of families B and C at this window -> (streams, names): every family B stream stands COPIES times, at scattered
    indices (which kRunCap runs an epoch lists depends on timing, the bytes must not), family C streams in between."""
    named = []
    for n, seed in BC_SIZES:
        for same_byte in (True, False):
            named += [(("B", n, same_byte, k), family_b(n, seed, same_byte, dense=window == 8)) for k in range(COPIES)]
            named.append((("C", n, same_byte, 0), family_c(window, n, seed, same_byte)))
    order = [(7 * i + 3) % len(named) for i in range(len(named))]  # (len = 20: 7 is coprime to it)
    assert sorted(order) == list(range(len(named)))
    return tuple(named[i][1] for i in order), tuple(named[i][0] for i in order)


@functools.lru_cache(maxsize=None)
def block_mode_field(n=300000):
    """One family B stream (every run the same byte) long enough for block mode: blocks of 1,024 positions over all workgroups."""
    return family_b(n, 3, True)
