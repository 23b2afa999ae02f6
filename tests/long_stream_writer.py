"""Token streams built bit by bit for the long-stream decoder (a plain helper for both test tiers, no fixtures).

``TokenWriter`` writes the ``.tamp`` token grammar as ``long_token()`` of tamp_decompress_long_kernel.hpp reads it -- header
byte, literal, match, RLE, extended match, FLUSH with its padding; windows 8..15, literals 5..8, both formats -- and keeps, per
token, the bit it starts at, the bytes it produces, the bytes it writes to the window and ``window_pos`` in front of it.
``read_tokens`` reads a blob back into the same records (streams that were cut or had bytes appended).  ``chunk_table`` and
``group_cuts`` derive what the launcher derives: tokens, bytes, special and lagging tokens of the tokens that START in each
chunk of 4,096 (v1) or 1,024 (extended) bits, and the groups (launch_decompress_long's three conditions: output bytes,
records, lagging tokens).  Nothing here computes decoded BYTES: the expected output is always the checker's.

``DESIGNED`` names streams that sit on one boundary of the long-stream decoder each; every entry returns a ``Stream`` whose
``props`` are asserted from the bookkeeping by tests/test_long_stream_writer.py -- the guarantee that the GPU tests of
tests/test_gpu_long_decode_edges.py aim where they say they aim.
"""
import random
from collections import namedtuple

CODE = (0x00, 0x03, 0x08, 0x0B, 0x14, 0x24, 0x26, 0x2B, 0x4B, 0x54, 0x94, 0x95, 0xAA, 0x27, 0xAB)  # tests/test_host_logic.py
NBITS = (2, 3, 5, 5, 6, 7, 7, 7, 8, 8, 9, 9, 9, 7, 9)  # flag bit included
SYM_RLE, SYM_EXT, SYM_FLUSH = 12, 13, 14
CHUNK_BITS_V1, CHUNK_BITS_EXT = 4096, 1024
GROUP_OUT, SPLIT_MAX_OUT, LAG_CAP, WP_BLOCK, SCAN_BLOCK = 32768, 16384, 63, 2048, 64
_DECODE = {}  # bits after the flag -> symbol
for _s in range(15):
    _DECODE[format(CODE[_s], "0%db" % (NBITS[_s] - 1))] = _s

def oob(tk, window):
    """An offset that runs out of the window (TAMP_OOB)."""
    return tk.off is not None and tk.off + tk.produced > 1 << window


Tok = namedtuple("Tok", "bit nbits kind produced written wp off")  # kind: L M R X F; off: window offset of M / X, else None


def min_pattern(window, literal):
    return 2 + (window > 10 + 2 * (literal - 5))


def header_byte(window, literal, extended, custom=False, more=False):
    return (window - 8) << 5 | (literal - 5) << 3 | int(custom) << 2 | int(extended) << 1 | int(more)


class TokenWriter:
    def __init__(self, window=10, literal=8, extended=False, custom=False, more=None):
        """``more``: None, or the value of a second header byte (the first then has its lowest bit set)."""
        self.window, self.literal, self.extended = window, literal, bool(extended)
        self.W, self.minp = 1 << window, min_pattern(window, literal)
        self.buf = bytearray([header_byte(window, literal, extended, custom, more is not None)])
        if more is not None:
            self.buf.append(more)
        self.header_bits = 8 * len(self.buf)
        self._acc = self._n = 0
        self.tokens, self.wp, self.out = [], 0, 0
        self.max_plain = self.minp + (11 if extended else 13)
        self.max_ext = self.minp + 131

    @property
    def bit(self):
        return 8 * len(self.buf) + self._n

    @property
    def chunk_bits(self):
        return CHUNK_BITS_EXT if self.extended else CHUNK_BITS_V1

    def _put(self, v, nb):
        assert 0 <= v < 1 << nb
        self._acc, self._n = self._acc << nb | v, self._n + nb
        while self._n >= 8:
            self._n -= 8
            self.buf.append(self._acc >> self._n)
            self._acc &= (1 << self._n) - 1

    def _tok(self, start, kind, produced, written, off=None):
        self.tokens.append(Tok(start, self.bit - start, kind, produced, written, self.wp, off))
        self.wp, self.out = (self.wp + written) & (self.W - 1), self.out + produced

    def lit(self, b):
        t = self.bit
        self._put(1 << self.literal | (b & ((1 << self.literal) - 1)), 1 + self.literal)
        self._tok(t, "L", 1, 1)

    def match(self, off, ln, check=True):
        sym, t = ln - self.minp, self.bit
        assert 0 <= sym <= (11 if self.extended else 13) and 0 <= off < self.W
        assert not check or off + ln <= self.W
        self._put(CODE[sym], NBITS[sym])
        self._put(off, self.window)
        self._tok(t, "M", ln, ln, off)

    def _second(self, value, trailing):
        h = value >> trailing
        assert 0 <= h <= 14
        self._put(CODE[h], NBITS[h] - 1)
        self._put(value & ((1 << trailing) - 1), trailing)

    def rle(self, count):
        assert self.extended and 2 <= count <= 241
        t = self.bit
        self._put(CODE[SYM_RLE], NBITS[SYM_RLE])
        self._second(count - 2, 4)
        self._tok(t, "R", count, min(count, 8, self.W - self.wp))

    def ext(self, off, ln, check=True):
        assert self.extended and self.minp + 12 <= ln <= self.max_ext and 0 <= off < self.W
        assert not check or off + ln <= self.W
        t = self.bit
        self._put(CODE[SYM_EXT], NBITS[SYM_EXT])
        self._second(ln - self.minp - 12, 3)
        self._put(off, self.window)
        self._tok(t, "X", ln, min(ln, self.W - self.wp), off)

    def flush(self):
        t = self.bit
        self._put(CODE[SYM_FLUSH], NBITS[SYM_FLUSH])
        self._put(0, -self.bit % 8)
        self._tok(t, "F", 0, 0)

    # ---- bit sizes, and fillers of plain tokens ----
    def match_bits(self, ln):
        return NBITS[ln - self.minp] + self.window

    def rle_bits(self, count):
        return NBITS[SYM_RLE] + NBITS[(count - 2) >> 4] - 1 + 4

    def ext_bits(self, ln):
        return NBITS[SYM_EXT] + NBITS[(ln - self.minp - 12) >> 3] - 1 + 3 + self.window

    def plain(self, rng, max_bits=None):
        """One random plain token (a literal or a match inside the window) of at most ``max_bits`` bits."""
        ln = rng.randrange(self.minp, self.max_plain + 1)
        if rng.random() < 0.4 or (max_bits is not None and self.match_bits(ln) > max_bits):
            self.lit(rng.randrange(256))
        else:
            self.match(rng.randrange(0, self.W - ln + 1), ln)

    def plain_until(self, bit, rng, literals=False):
        """Plain tokens until the next token would start at or behind ``bit``: every one of them starts in front of it."""
        while self.bit < bit:
            self.lit(rng.randrange(256)) if literals else self.plain(rng)

    def fill_to(self, bit, rng):
        """Plain tokens that end EXACTLY at ``bit`` (random ones, then a combination of token sizes that fits)."""
        sizes = {1 + self.literal: None}
        for ln in range(self.minp, self.max_plain + 1):
            sizes.setdefault(self.match_bits(ln), ln)
        big = max(sizes)
        while bit - self.bit > 12 * big:
            self.plain(rng)
        need = bit - self.bit
        assert need >= 0
        how = [None] * (need + 1)  # how[k]: the size of one token of a combination that sums to k
        how[0] = 0
        for k in range(1, need + 1):
            for s in sizes:
                if s <= k and how[k - s] is not None:
                    how[k] = s
                    break
        assert how[need] is not None, ("no combination of plain tokens fills", need)
        while need:
            s = how[need]
            ln = sizes[s]
            self.lit(rng.randrange(256)) if ln is None else self.match(rng.randrange(0, self.W - ln + 1), ln)
            need -= s
        assert self.bit == bit

    def blob(self):
        return bytes(self.buf) + (bytes([self._acc << (8 - self._n)]) if self._n else b"")


def read_tokens(blob, start=None, stop=None):
    """The tokens of ``blob`` as long_token() reads them, with the writer's bookkeeping: up to the first token that the
    bytes do not complete.  ``start`` / ``stop``: from that bit on (window_pos then counts from there), up to the first token
    that starts at or behind ``stop``.  -> (tokens, window, literal, extended, header bits)"""
    h0 = blob[0]
    window, literal, extended = ((h0 >> 5) & 7) + 8, ((h0 >> 3) & 3) + 5, bool(h0 & 2)
    W, minp, n = 1 << window, min_pattern(window, literal), 8 * len(blob)

    def bits(t, k):  # k <= 15 bits from bit t, or None behind the end
        if t + k > n:
            return None
        v = int.from_bytes(blob[t >> 3 : (t >> 3) + 3].ljust(3, b"\0"), "big")
        return (v >> (24 - (t & 7) - k)) & ((1 << k) - 1)

    def symbol(t):  # a prefix code word WITHOUT its flag bit at t -> (symbol, bits), or None
        for k in range(1, 9):
            v = bits(t, k)
            if v is None:
                return None
            s = _DECODE.get(format(v, "0%db" % k))
            if s is not None:
                return s, k
        raise AssertionError("not a complete prefix code")

    toks, t, wp = [], 8 * (1 + (h0 & 1)) if start is None else start, 0
    while stop is None or t < stop:
        flag = bits(t, 1)
        if flag is None:
            break
        if flag:
            if bits(t, 1 + literal) is None:
                break
            tok = Tok(t, 1 + literal, "L", 1, 1, wp, None)
        else:
            sk = symbol(t + 1)
            if sk is None:
                break
            sym, used = sk[0], 1 + sk[1]
            if sym == SYM_FLUSH:
                tok = Tok(t, used + -(t + used) % 8, "F", 0, 0, wp, None)
            elif extended and sym >= SYM_RLE:
                hk = symbol(t + used)
                trailing = 4 if sym == SYM_RLE else 3
                if hk is None or bits(t + used + hk[1], trailing) is None:
                    break
                v = (hk[0] << trailing) + bits(t + used + hk[1], trailing)
                used += hk[1] + trailing
                if sym == SYM_RLE:
                    tok = Tok(t, used, "R", v + 2, min(v + 2, 8, W - wp), wp, None)
                else:
                    off = bits(t + used, window)
                    if off is None:
                        break
                    ln = v + minp + 12
                    tok = Tok(t, used + window, "X", ln, min(ln, W - wp), wp, off)
            else:
                off = bits(t + used, window)
                if off is None:
                    break
                tok = Tok(t, used + window, "M", sym + minp, sym + minp, wp, off)
        toks.append(tok)
        t, wp = t + tok.nbits, (wp + tok.written) & (W - 1)
    return toks, window, literal, extended, 8 * (1 + (h0 & 1))


ChunkTable = namedtuple("ChunkTable", "n_chunks ntok outb nspec nlag nflush")
Group = namedtuple("Group", "v0 first_chunk ntok nout nlag")


def chunk_table(tokens, n_bytes, extended):
    """Per chunk, over the tokens that START in it and that ``n_bytes`` of the stream complete."""
    cb = CHUNK_BITS_EXT if extended else CHUNK_BITS_V1
    N = (8 * n_bytes + cb - 1) // cb
    ntok, outb, nspec, nlag, nflush = ([0] * N for _ in range(5))
    for tk in tokens:
        if tk.bit + tk.nbits > 8 * n_bytes:
            break
        i = tk.bit // cb
        if tk.kind == "F":
            nflush[i] += 1
            continue
        ntok[i] += 1
        outb[i] += tk.produced
        nspec[i] += tk.kind in "RX"
        nlag[i] += tk.written < tk.produced
    return ChunkTable(N, ntok, outb, nspec, nlag, nflush)


def group_cuts(ct, extended, chain=True):
    """The launcher's groups of whole chunks (tamp_capi.hip, launch_decompress_long): a chunk opens a new group when the
    open one would pass its output bytes, 2^20 - 1 records or 63 lagging tokens with it."""
    group_out = GROUP_OUT if (extended or chain) else SPLIT_MAX_OUT
    groups, v = [], 0
    cur = [0, 0, 0, 0, 0]
    for i in range(ct.n_chunks):
        nl = ct.nlag[i] if extended else 0
        if cur[3] + ct.outb[i] > group_out or cur[2] + ct.ntok[i] > 0xFFFFF or cur[4] + nl > LAG_CAP:
            groups.append(Group(*cur))
            cur = [v, i, 0, 0, 0]
        cur[2] += ct.ntok[i]
        cur[3] += ct.outb[i]
        cur[4] += nl
        v += ct.outb[i]
    groups.append(Group(*cur))
    return groups


Numbers = namedtuple("Numbers", "n_bytes chunks groups tokens out entries wp_blocks max_lags early scan_blocks oob group_list table")


def numbers(tokens, n_bytes, window, extended, chain=True):
    """What the decoder's debug lines report for a stream of ``n_bytes`` that holds ``tokens``."""
    ct = chunk_table(tokens, n_bytes, extended)
    gl = group_cuts(ct, extended, chain)
    entries = sum(ct.nspec) + ct.n_chunks if extended else 0
    chained = extended or chain
    return Numbers(n_bytes, ct.n_chunks, len(gl), sum(ct.ntok), sum(ct.outb), entries, (entries + WP_BLOCK - 1) // WP_BLOCK,
                   max(ct.nlag) if extended else 0, sum(1 for g in gl if g.nout and g.v0 < (1 << window)),
                   (len(gl) + SCAN_BLOCK - 1) // SCAN_BLOCK if chained else 0,
                   any(oob(tk, window) for tk in tokens if tk.bit + tk.nbits <= 8 * n_bytes), gl, ct)


class Stream:
    """A designed stream: the blob, the writer's tokens, its configuration and the properties it was built for."""

    def __init__(self, w, props=None, dictionary=None, blob=None):
        self.blob = w.blob() if blob is None else blob
        self.tokens, self.window, self.literal, self.extended = w.tokens, w.window, w.literal, w.extended
        self.dictionary, self.props = dictionary, dict(props or {})

    def numbers(self, n_bytes=None, chain=True):
        return numbers(self.tokens, len(self.blob) if n_bytes is None else n_bytes, self.window, self.extended, chain)

    @property
    def produced(self):
        return sum(tk.produced for tk in self.tokens)


def mixed(w, rng, until_bit):
    """Random tokens of every kind the format has (FLUSH too) until ``until_bit`` is reached or passed."""
    while w.bit < until_bit:
        u = rng.random()
        if u < 0.02:
            w.flush()
        elif w.extended and u < 0.10:
            w.rle(rng.choice((2, 3, 7, 8, 9, 10, 17, 18, 40, 241)))
        elif w.extended and u < 0.18:
            ln = rng.randrange(w.minp + 12, w.max_ext + 1)
            w.ext(rng.randrange(0, w.W - ln + 1), ln)
        else:
            w.plain(rng)


def random_token_list(seed):
    """A short random stream over all windows, literal sizes and both formats (the CPU tier's seeded sweep)."""
    rng = random.Random(seed)
    w = TokenWriter(rng.randrange(8, 16), rng.randrange(5, 9), rng.random() < 0.5)
    mixed(w, rng, w.bit + rng.choice((40, 300, 2500, 9000)))
    return Stream(w)


# ---------------------------------------------------------------------------------------------------------------
# designed streams
# ---------------------------------------------------------------------------------------------------------------
def one_token_repeated(extended, kind, chunks=70):
    """Literal-only / match-only streams whose token size is coprime to the chunk: a token starts at every bit phase in front
    of a boundary -- it ends exactly on one, one bit in front of one and one bit behind one."""
    w = TokenWriter(10, 8, extended)
    rng = random.Random(3)
    while w.bit < chunks * w.chunk_bits - 16:
        w.lit(rng.randrange(256)) if kind == "L" else w.match(rng.randrange(0, w.W - 3), 3)  # 9 and 13 bits
    s = Stream(w)
    size = 9 if kind == "L" else 13
    s.props = dict(kinds={kind}, phases=set(range(size)), chunks=chunks)
    return s


def flush_edges(extended):
    """FLUSH tokens whose padding ends on a chunk boundary, for each of the 8 pad lengths (each the last token of its chunk);
    a FLUSH as the first token of a chunk; a chunk of FLUSH tokens only."""
    w = TokenWriter(10, 8, extended)
    rng = random.Random(4)
    cb = w.chunk_bits
    for pad in range(8):
        w.fill_to((2 + 3 * pad) * cb - 9 - pad, rng)
        w.flush()
        assert w.bit == (2 + 3 * pad) * cb
    w.fill_to(30 * cb, rng)
    w.flush()  # first token of chunk 30
    w.fill_to(40 * cb, rng)
    while w.bit < 41 * cb:  # chunk 40: nothing but FLUSH tokens (9 bits + 7 of padding each)
        w.flush()
    assert w.bit == 41 * cb
    mixed(w, rng, 70 * cb - 40)
    return Stream(w, dict(pads=set(range(8)), flush_first=30, flush_only=40, chunks=70))


def periodic(extended):
    """One token repeated over 200 chunks: a parse from a wrong phase of a periodic bit stream never falls back into step,
    the right starts travel a workgroup of 64 chunks per round."""
    w = TokenWriter(10, 8, extended)
    while w.bit < 200 * w.chunk_bits - 24:
        w.match(0, 13 if extended else 15)
    return Stream(w, dict(chunks=200))


def chunk_cut_lengths(s, counts=(63, 64, 65, 128, 129)):
    return [c * (CHUNK_BITS_EXT if s.extended else CHUNK_BITS_V1) // 8 for c in counts]


def mixed_70(extended, window=10, seed=5):
    w = TokenWriter(window, 8, extended)
    rng = random.Random(seed)
    mixed(w, rng, 70 * w.chunk_bits - 600)
    w.fill_to(70 * w.chunk_bits - 3, rng)  # (the last byte: five token bits and three of padding)
    return Stream(w, dict(chunks=70))


def end_cuts(s):
    """Every byte length of the last two chunks plus 8 bytes."""
    cbytes = (CHUNK_BITS_EXT if s.extended else CHUNK_BITS_V1) // 8
    return list(range(len(s.blob) - 2 * cbytes - 8, len(s.blob)))


def group_cut(target, twin):
    """v1, window 2^10: the chunks up to some chunk k produce exactly ``target`` output bytes (``twin``: one more), the last
    token of chunk k tuned for it.  With ``target`` = the group's room, group 0 ends with chunk k; the twin's would pass
    the room by one byte and closes a chunk earlier."""
    w = TokenWriter(10, 8, False)
    rng = random.Random(6)
    cb, goal = w.chunk_bits, target + int(twin)
    done = False
    while not done:
        end = (w.bit // cb + 1) * cb
        r, t = goal - w.out, w.bit
        plan = None
        for a in range(0, min(r // 15, (end - t) // 17) + 1):  # a matches of 15 bytes (17 bits), b literals, one match of f bytes
            for f in range(2, 16):
                b = r - 15 * a - f
                if b < 0:
                    continue
                last = t + 17 * a + 9 * b
                if last < end <= last + w.match_bits(f):
                    plan = (a, b, f)
                    break
            if plan:
                break
        if plan:
            a, b, f = plan
            order = ["M"] * a + ["L"] * b
            rng.shuffle(order)
            for k in order:
                w.match(rng.randrange(0, w.W - 15), 15) if k == "M" else w.lit(rng.randrange(256))
            w.match(rng.randrange(0, w.W - f), f)
            done = True
            assert w.out == goal and w.tokens[-1].bit < end <= w.bit
        elif r > 3615 + 460:
            while w.bit < end:
                w.match(rng.randrange(0, w.W - 15), 15)
        else:
            w.plain_until(end, rng, literals=True)
    cut_chunk = w.tokens[-1].bit // cb + 1  # the first chunk behind the cut
    mixed(w, rng, (cut_chunk + 6) * cb)
    return Stream(w, dict(cut_chunk=cut_chunk, cut_out=goal, twin=twin))


def _source_tokens(w, rng, wp0):
    for _ in range(5):
        w.lit(rng.randrange(256))
    w.match(wp0 - 3, 8)      # three bytes of the window in front of the group, five of the group's own
    w.match(w.wp - 3, 10)    # off < window_pos < off + len
    w.match(w.wp - 2, 2)     # the two bytes just written
    w.match(w.wp - 1, 2)     # the byte just written and the one under the cursor


def sources_v1():
    """v1, window 2^10: 31 KB of output, then a chunk of 2 KB and more that group 0 has no room for -- it opens group 1 with
    five literals and matches whose source straddles the group's first byte, straddles the write cursor, is the byte just
    written."""
    w = TokenWriter(10, 8, False)
    rng = random.Random(14)
    cb = w.chunk_bits
    while w.out < 30000:
        w.match(rng.randrange(0, w.W - 15), 15)
    while True:
        w.plain_until((w.bit // cb + 1) * cb, rng, literals=True)
        if w.out > 30800 and 8 <= w.wp <= w.W - 40:
            break
    assert w.out <= GROUP_OUT
    chunk, v0 = w.tokens[-1].bit // cb + 1, w.out
    _source_tokens(w, rng, w.wp)
    while w.bit < (chunk + 1) * cb:
        w.match(rng.randrange(0, w.W - 15), 15)
    mixed(w, rng, (chunk + 5) * cb)
    return Stream(w, dict(group_chunk=chunk, v0=v0))


def densest_w15():
    """v1, window 2^15: every chunk full of the longest match (15 bytes in 22 bits, 186 or 187 to a chunk), the most a chunk can
    produce at this window: with TAMP_AMD_LONGDEC_CHAIN=0 groups are five chunks of 2.8 KB, and three of them start inside the
    first W = 32,768 bytes."""
    w = TokenWriter(15, 8, False)
    rng = random.Random(7)
    while w.bit < 24 * w.chunk_bits - 24:
        w.match(rng.randrange(0, w.W - 15), 15)
    return Stream(w, dict(early_unchained=3))


def lag_chunks(window, lags, chunks=70, extra=None, back=(), seed=8):
    """Extended format: every chunk holds exactly ``lags`` lagging RLE tokens (9 bytes produced, 8 written) and a few plain
    tokens; ``extra`` = (chunk, lags) gives one chunk another count.  With 63 every group is one chunk.  ``back``: group
    distances -- each chunk's last tokens copy bytes that the chunk so many chunks earlier wrote, and bytes of the initial
    dictionary that nothing has overwritten yet (plain matches, placed by the writer's window_pos bookkeeping)."""
    w = TokenWriter(window, 8, True)
    rng = random.Random(seed)
    cb = w.chunk_bits
    starts, copies = [], []  # window_pos and bytes written so far at each chunk's first token
    for c in range(chunks):
        end = (c + 1) * cb
        starts.append((w.wp, sum(t.written for t in w.tokens)))
        n = extra[1] if extra and extra[0] == c else lags
        w.lit(rng.randrange(256)) if c else w.rle(9)  # (the stream's first token: an RLE of the dictionary's last byte)
        for _ in range(n - (0 if c else 1)):
            w.rle(9)
        total = starts[-1][1]
        for d in back:
            if c - d >= 0:
                off, wr = starts[c - d]
                ln = rng.randrange(w.minp, w.max_plain + 1)
                if total - wr + 600 < w.W and off + ln <= w.W:  # still in the window when this chunk ends
                    w.match(off, ln)
                    copies.append((c, d))
        if back:
            wr_end = total + 8 * n + 80  # bytes written when this chunk is over, at most
            if wr_end + 16 < w.W:
                w.match(rng.randrange(wr_end, w.W - 14), rng.randrange(w.minp, w.max_plain + 1))
                copies.append((c, "dictionary"))
        w.fill_to(end, rng) if end - w.bit >= 100 else w.plain_until(end, rng, literals=True)
    props = dict(lags=lags, chunks=chunks, extra=extra, copies=copies)
    return Stream(w, props)


def wp_blocks(window, seed=9):
    """Extended format: about 4,200 entries in the list of RLE / extended-match tokens and chunk markers -- three blocks of the
    window_pos chain; a chunk marker is entry 2,047, RLE and extended-match tokens sit on both sides of entries 2,048 and
    4,096; tokens clipped at the ring's end: RLE at window_pos W - 1 and W - 3, an extended match that ends exactly at W
    (not clipped), one that starts at window_pos 0, and every wrap of the ring clips one."""
    w = TokenWriter(window, 8, True)
    rng = random.Random(seed)
    cb, W = w.chunk_bits, w.W
    big = w.ext_bits(w.max_ext)
    stunt = 0

    def entries():  # list entries in front of the next token
        return sum(1 for t in w.tokens if t.kind in "RX") + w.bit // cb

    def special(end, stunts):
        nonlocal stunt
        room = W - w.wp
        if stunts and room <= w.max_ext and w.bit + 400 < end:  # the ring's end is near: one of four ways over it
            how = stunt % 4
            stunt += 1
            if how < 2:  # an RLE at window_pos W - 1 / W - 3, plain tokens up to there
                want = 1 if how == 0 else 3
                while W - w.wp > want:
                    ln = min(W - w.wp - want, w.max_plain)
                    w.lit(rng.randrange(256)) if ln < w.minp else w.match(rng.randrange(0, W - ln + 1), ln)
                w.rle(5)
            elif how == 2 and room >= w.minp + 12:  # an extended match that ends exactly at W: not clipped
                w.ext(rng.randrange(0, W - room + 1), room)
            else:  # clipped
                ln = max(w.minp + 12, min(w.max_ext, room + rng.randrange(1, 30)))
                w.ext(rng.randrange(0, W - ln + 1), ln)
        elif w.wp == 0 or rng.random() < 0.45:
            ln = rng.randrange(w.minp + 12, min(w.minp + 50, w.max_ext) + 1)
            w.ext(rng.randrange(0, W - ln + 1), ln)
        else:
            w.rle(rng.choice((2, 3, 4, 5, 6, 7, 8, 8, 8, 9, 12, 30)))

    marker_done = False
    while entries() < 4200:
        c = w.bit // cb
        end = (c + 1) * cb
        need = 2047 - entries()  # specials this chunk needs for its marker to be entry 2,047
        k = 34
        if not marker_done and 0 <= need <= 60:
            k = need if need <= 34 else need - 20
        n = 0
        while n < k and w.bit + big + 8 * 9 < end:
            before = len(w.tokens)
            special(end, marker_done or need > 100)
            n += sum(1 for t in w.tokens[before:] if t.kind in "RX")
        if not marker_done and n == need:
            marker_done = True
        w.plain_until(end, rng, literals=True)
    assert marker_done
    return Stream(w, dict(entries_min=4200, blocks=3))


def sources(window=10):
    """Extended format, 63 lagging RLE tokens in each of chunks 0..2 (so chunk 1 and chunk 2 each open a group): an RLE as the
    stream's first token and as a group's first token; matches whose source straddles the group's first byte, straddles
    the write cursor, is the byte just written; an extended match of the maximum length from offset W - len."""
    w = TokenWriter(window, 8, True)
    rng = random.Random(10)
    cb = w.chunk_bits
    for c in range(3):
        for _ in range(63):
            w.rle(9)
        if c < 2:
            w.plain_until((c + 1) * cb, rng, literals=True)
    # chunk 2 opened a group with an RLE; now, in the same group:
    first = next(t for t in w.tokens if t.bit >= 2 * cb)
    wp0 = first.wp
    assert wp0 >= 3
    _source_tokens(w, rng, wp0)
    w.ext(w.W - w.max_ext, w.max_ext)
    mixed(w, rng, 8 * cb)
    return Stream(w, dict(group_chunks=(1, 2)))


def fresh_window(extended, dictionary=True):
    """Window 2^15 and a custom dictionary: about 31,000 literals (group 0), then a chunk that does not fit group 0 any more
    and whose tokens copy dictionary bytes at ring indices nothing has written yet, then tokens that copy group 0's bytes."""
    w = TokenWriter(15, 8, extended, custom=dictionary)
    rng = random.Random(11)
    cb = w.chunk_bits
    while w.out < 31000:
        w.lit(rng.randrange(256))
    w.plain_until((w.bit // cb + 1) * cb, rng, literals=True)
    v0, fresh = w.out, []
    end = (w.tokens[-1].bit // cb + 2) * cb  # one whole chunk behind the literals
    while w.bit < end:
        ln = w.max_ext if extended else w.max_plain
        lo = w.wp + ln + 1  # ring indices from here to W have not been written: window_pos has not wrapped yet
        if w.out < w.W - 2 * ln and lo + ln < w.W:
            off = rng.randrange(lo, w.W - ln)
            fresh.append(len(w.tokens))
        else:
            off = rng.randrange(0, 30000)
        w.ext(off, ln) if extended else w.match(off, ln)
    for _ in range(200):
        ln = rng.randrange(w.minp, w.max_plain + 1)
        w.match(rng.randrange(0, 30000), ln)
    mixed(w, rng, w.bit + 4 * cb)
    dic = bytes(random.Random(12).randrange(256) for _ in range(1 << 15)) if dictionary else None
    return Stream(w, dict(v0=v0, fresh=fresh), dictionary=dic)


def bad_offset(extended=False):
    """Mixed tokens, and in chunk 40 a match with off + len = W + 1."""
    w = TokenWriter(10, 8, extended)
    rng = random.Random(13)
    mixed(w, rng, 40 * w.chunk_bits + 100)
    w.match(w.W + 1 - 5, 5, check=False)
    mixed(w, rng, 70 * w.chunk_bits - 20)
    return Stream(w, dict(bad_chunk=40))


DESIGNED = {
    "literals v1": lambda: one_token_repeated(False, "L"),
    "literals ext": lambda: one_token_repeated(True, "L"),
    "matches v1": lambda: one_token_repeated(False, "M"),
    "matches ext": lambda: one_token_repeated(True, "M"),
    "flush v1": lambda: flush_edges(False),
    "flush ext": lambda: flush_edges(True),
    "periodic v1": lambda: periodic(False),
    "periodic ext": lambda: periodic(True),
    "mixed v1": lambda: mixed_70(False),
    "mixed ext": lambda: mixed_70(True),
    "group 32768": lambda: group_cut(GROUP_OUT, False),
    "group 32769": lambda: group_cut(GROUP_OUT, True),
    "group 16384": lambda: group_cut(SPLIT_MAX_OUT, False),
    "group 16385": lambda: group_cut(SPLIT_MAX_OUT, True),
    "densest w15": densest_w15,
    "lags 63 w10": lambda: lag_chunks(10, 63),
    "lags 63 w15": lambda: lag_chunks(15, 63),
    "lags 64 in one chunk": lambda: lag_chunks(10, 63, extra=(35, 64)),
    "lags 20": lambda: lag_chunks(10, 20),
    "groups 64": lambda: lag_chunks(15, 63, chunks=64, back=(3, 17, 60)),
    "groups 65": lambda: lag_chunks(15, 63, chunks=65, back=(3, 17, 60)),
    "groups 128": lambda: lag_chunks(15, 63, chunks=128, back=(3, 17, 60)),
    "groups 129": lambda: lag_chunks(15, 63, chunks=129, back=(3, 17, 60)),
    "wp blocks w8": lambda: wp_blocks(8),
    "wp blocks w10": lambda: wp_blocks(10),
    "sources": sources,
    "sources v1": sources_v1,
    "fresh v1": lambda: fresh_window(False),
    "fresh ext": lambda: fresh_window(True),
    "bad offset": bad_offset,
}
_cache = {}


def designed(name):
    """The designed stream ``name`` (built once per process; treat it as read-only)."""
    if name not in _cache:
        _cache[name] = DESIGNED[name]()
    return _cache[name]
