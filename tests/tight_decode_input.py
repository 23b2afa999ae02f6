"""Inputs of the tight-decode tests (tests/test_tight_decode_input.py, tests/test_oracle_vs_reference.py,
tests/test_gpu_tight_decode.py): a small named set of compressed streams, and the rule all tiers check.  A plain helper: no
fixtures, no GPU.

THE RULE (include/tamp_amd.h, tamp_batch_decompress).  (S, X, K) = a stream's status, bytes and consumed count with ample room,
N = len(X).  With ``cap`` bytes of room:
    cap <  N:  TAMP_OUTPUT_FULL, out_len = cap, the slab holds X[:cap]
    cap >  N:  exactly (S, X, K)
    cap == N:  all of X, status S or TAMP_OUTPUT_FULL (the reference asks ``op == cap`` before it looks at the next token: a
               stream that ends in TAMP_OOB, or a clean one with pad bits left, reports TAMP_OUTPUT_FULL here)
and in_consumed never decreases as ``cap`` grows.

TEXT streams are the oracle's compression of tight_output_input.short_input / long_input (300 and 2,560 plain bytes: under 512
and from 512 compressed bytes on -- the lean and the bulk builds, the one-wavefront and the workgroup RESOLVE).  DESIGNED streams
are written token by token with long_stream_writer.TokenWriter; what each was built for is in ``props`` and is asserted from
the writer's bookkeeping (bit positions, bytes produced and written, window_pos -- never decoded bytes) by
tests/test_tight_decode_input.py.
"""
import random

import long_stream_writer as lsw
import tight_output_input as toi

OUTPUT_FULL, INPUT_EXHAUSTED, OOB = 1, 2, -4
RLE_COUNTS = (2, 8, 9, 16, 17, 241)
LAG_LIMIT = 48  # tamp_decompress_split_kernel.hpp kSplitMaxLag: the 49th lagging token flags a stream


def rule(full, cap):
    """What ``cap`` bytes of room give a stream whose ample-room result is ``full`` = (S, X, K).
    -> (the statuses allowed, the bytes, the consumed count or None where only "never decreases" binds it)"""
    S, X, K = full
    if cap < len(X):
        return (OUTPUT_FULL,), X[:cap], None
    if cap > len(X):
        return (S,), X, K
    return (S, OUTPUT_FULL), X, None


def obeys(full, cap, got):
    statuses, data, consumed = rule(full, cap)
    return got[0] in statuses and got[1] == data and (consumed is None or got[2] == consumed) and got[2] <= full[2]


class Case:
    """One compressed stream: configuration, blob, optional dictionary, the writer's tokens (designed streams) and ``props``."""

    def __init__(self, name, window, literal, extended, blob, dictionary=None, tokens=None, props=None):
        self.name, self.window, self.literal, self.extended = name, window, literal, bool(extended)
        self.blob, self.dictionary, self.tokens, self.props = blob, dictionary, tokens, dict(props or {})

    def __repr__(self):
        return "Case(%r)" % self.name


# ---------------------------------------------------------------------------------------------------------------------
# text streams
# ---------------------------------------------------------------------------------------------------------------------
TEXT_CONFS = (("w10 ext", 10, 8, True), ("w10 v1", 10, 8, False), ("w9 l5", 9, 5, False), ("w15", 15, 8, True))


def text_cases(oracle):
    out = []
    for kind, make in (("short", toi.short_input), ("long", toi.long_input)):
        for tag, window, literal, extended in TEXT_CONFS:
            x = make(literal)
            st, blob = oracle.compress(x, window=window, literal=literal, extended=extended)
            assert st == 0
            out.append(Case("%s text %s" % (kind, tag), window, literal, extended, blob, props=dict(plain=len(x), kind=kind)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# designed streams
# ---------------------------------------------------------------------------------------------------------------------
def _place(w, ln, back=0, stunts=()):
    """Plain matches until a token of ``ln`` bytes at window_pos stays inside the ring with ``back`` bytes in front of it.
    ``stunts``: a list of (room, token) -- where the ring has to be wrapped for it, the next of them does that: plain tokens up
    to window_pos W - room, then the token, which is clipped at the ring's end."""
    assert back + ln <= w.W
    while w.wp + ln > w.W or w.wp < back:
        if stunts and w.wp + ln > w.W and w.wp <= w.W - stunts[0][0]:
            room, token = stunts.pop(0)
            _goto(w, w.W - room)
            token()
        else:
            w.match(0, w.max_plain)


def _goto(w, pos):
    """Plain tokens until window_pos is exactly ``pos``."""
    while w.wp != pos:
        step = min((pos - w.wp) % w.W, w.max_plain)
        w.lit(0x41) if step < w.minp else w.match(0, step)


def _to_phase(w, rng, phase):
    """Plain tokens until the next token starts at bit ``phase`` of a byte."""
    odd = [ln for ln in range(w.minp, w.max_plain + 1) if w.match_bits(ln) % 2]
    while w.bit % 8 != phase:
        if (1 + w.literal) % 2 or (phase - w.bit) % 2 == 0:
            w.lit(rng.randrange(256))
        else:
            w.match(0, odd[0])


def _filler(w, rng, min_bytes, min_out, max_out, literals=0.6):
    """Literals and plain matches inside the window until the blob has ``min_bytes`` and more than ``min_out`` bytes come out."""
    while (len(w.buf) < min_bytes or w.out <= min_out) and w.out + w.max_plain <= max_out:
        if rng.random() < literals:
            w.lit(rng.randrange(256))
        else:
            ln = rng.randrange(w.minp, w.max_plain + 1)
            w.match(rng.randrange(0, w.W - ln + 1), ln)


def _ext_distances(ln, few=False):
    return sorted(d for d in ({1, 16, ln} if few else {1, 2, 3, 4, 8, 15, 16, 17, ln - 1, ln}) if 1 <= d <= ln)


def _every_token(w, rng, plain_lengths, ext_lengths, phases, few=False):
    """Every token kind; matches whose source overlaps their destination; the RLE counts; extended matches at both ends of
    their range; tokens clipped at the ring's end (each time the ring wraps: an RLE at window_pos W - 1, an extended match
    that starts 5 bytes in front of the end, an RLE at W - 3); FLUSH at the bit phases ``phases``."""
    for _ in range(12):
        w.lit(rng.randrange(256))
    overlaps = set()
    stunts = [(1, lambda: w.rle(5)), (5, lambda: w.ext(7, w.minp + 20)), (3, lambda: w.rle(8))]
    for ln in plain_lengths:  # plain matches at every distance 1 .. length
        for d in range(1, ln + 1):
            _place(w, ln, d, stunts)
            w.match(w.wp - d, ln)
            overlaps.add(("M", ln, d))
    for count in RLE_COUNTS:  # away from the ring's end: min(count, 8) bytes enter the window
        _place(w, 8, 0, stunts)
        w.rle(count)
        w.lit(rng.randrange(256))
    for ln in ext_lengths:
        _place(w, ln, 0, stunts)
        w.ext(rng.randrange(0, w.W - ln + 1), ln)  # somewhere in the window
        for d in _ext_distances(ln, few and ln > 40):
            _place(w, ln, d, stunts)
            w.ext(w.wp - d, ln)
            overlaps.add(("X", ln, d))
    while stunts:  # (those the ring did not wrap for: a lap of plain tokens each)
        room, token = stunts.pop(0)
        _goto(w, w.W - room)
        token()
    for p in phases:
        _to_phase(w, rng, p)
        w.flush()
    return overlaps


def tokens_case(short=False):
    if short:
        w = lsw.TokenWriter(9, 5, True)
        plain, ext, phases = (2, w.max_plain), (w.minp + 12, w.max_ext), (4, 1, 6)
    else:
        w = lsw.TokenWriter(10, 8, True)
        plain, ext, phases = (2, 3, w.max_plain), (w.minp + 12, w.max_ext), (0, 1, 2, 3, 4, 5, 6, 7)
    rng = random.Random(41 + short)
    overlaps = _every_token(w, rng, plain, ext, phases, few=short)
    if short:
        _filler(w, rng, 300, 1500, 1990)
    else:
        _filler(w, rng, 600, 2048, 4000, literals=0.85)
    w.fill_to((w.bit + 150) // 8 * 8, rng)  # the last token ends on a byte: no pad bits, so exact room reports the end status
    return Case("short_tokens" if short else "tokens", w.window, w.literal, True, w.blob(), tokens=w.tokens,
                props=dict(overlaps=overlaps, plain_lengths=plain, ext_lengths=ext, phases=set(phases), status=INPUT_EXHAUSTED))


def lag_case():
    """64 RLE tokens of 9 bytes (8 enter the window: a lagging token each) with a match and a literal between them."""
    w = lsw.TokenWriter(10, 8, True)
    rng = random.Random(43)
    for _ in range(64):
        w.rle(9)
        ln = w.max_plain
        w.match(rng.randrange(0, w.W - ln + 1), ln)
        w.lit(rng.randrange(256))
    _filler(w, rng, 600, 2048, 4000)
    return Case("lag", 10, 8, True, w.blob(), tokens=w.tokens, props=dict(status=INPUT_EXHAUSTED))


def lag_starts(case):
    """Output offsets at which the lagging tokens (written < produced) of a designed stream start."""
    out, at = [], 0
    for tk in case.tokens:
        if tk.written < tk.produced:
            out.append(at)
        at += tk.produced
    return out


def reset_case():
    """v1, 5-bit literals, a second header byte of 0 and three dictionary resets (FLUSH, FLUSH)."""
    w = lsw.TokenWriter(10, 5, False, more=0)
    rng = random.Random(44)
    for k, until in enumerate((900, 1500, 2000, 2300)):
        _filler(w, rng, 0, until, 4000)
        if k < 3:
            _to_phase(w, rng, (3, 0, 6)[k])
            w.flush()
            w.flush()
            w.wp = 0  # (the decoder starts over on the seeded dictionary)
    _filler(w, rng, 600, 2048, 4000)
    return Case("reset", 10, 5, False, w.blob(), tokens=w.tokens, props=dict(status=INPUT_EXHAUSTED))


def reset_starts(case):
    """Output offsets of the dictionary resets: a FLUSH token directly behind a FLUSH token."""
    out, at, last = [], 0, False
    for tk in case.tokens:
        if tk.kind == "F" and last:
            out.append(at)
        last = tk.kind == "F"
        at += tk.produced
    return out


def oob_case():
    """v1, window 2^8: plain tokens, then a match with off + len = W + 1, then tokens nobody decodes."""
    w = lsw.TokenWriter(8, 8, False)
    rng = random.Random(45)
    _filler(w, rng, 600, 2048, 4000)
    n_out, n_tokens = w.out, len(w.tokens)
    w.match(w.W + 1 - 6, 6, check=False)
    for _ in range(20):
        w.plain(rng)
    return Case("oob", 8, 8, False, w.blob(), tokens=w.tokens, props=dict(status=OOB, n_out=n_out, bad_token=n_tokens))


def cut_case():
    """Window 2^12: mixed tokens, the last one an extended match; the blob ends inside that token's offset field."""
    w = lsw.TokenWriter(12, 8, True)
    rng = random.Random(46)
    lsw.mixed(w, rng, 2400)
    _filler(w, rng, 600, 2048, 3900)
    _place(w, 60)
    n_out = w.out
    w.ext(rng.randrange(0, w.W - 60), 60)
    last = w.tokens[-1]
    n_bytes = (last.bit + last.nbits - 6) // 8
    assert last.bit < 8 * n_bytes < last.bit + last.nbits
    return Case("cut", 12, 8, True, w.blob()[:n_bytes], tokens=w.tokens, props=dict(status=INPUT_EXHAUSTED, n_out=n_out))


def custom_dictionary(window, literal, seed):
    return toi._mask(toi.text(1 << window, seed), literal)


def custom_case():
    """Custom bit set: mixed tokens, and matches from dictionary bytes at ring indices nothing has overwritten yet."""
    w = lsw.TokenWriter(10, 8, True, custom=True)
    rng = random.Random(47)
    fresh = 0
    while w.wp + 200 < w.W and w.out == w.wp:  # (window_pos has not wrapped: everything from window_pos on is dictionary)
        ln = rng.randrange(w.minp, w.max_plain + 1)
        w.match(rng.randrange(w.wp + ln, w.W - ln + 1), ln)
        w.lit(rng.randrange(256))
        fresh += 1
    w.ext(w.W - w.max_ext, w.max_ext)
    lsw.mixed(w, rng, w.bit + 1500)
    _filler(w, rng, 600, 2048, 4000)
    return Case("custom", 10, 8, True, w.blob(), dictionary=custom_dictionary(10, 8, 51), tokens=w.tokens,
                props=dict(status=INPUT_EXHAUSTED, fresh=fresh))


DESIGNED = {"tokens": tokens_case, "short_tokens": lambda: tokens_case(short=True), "lag": lag_case, "reset": reset_case,
            "oob": oob_case, "cut": cut_case, "custom": custom_case}
_cache = {}


def designed(name):
    """The designed stream ``name`` (built once per process; treat it as read-only)."""
    if name not in _cache:
        _cache[name] = DESIGNED[name]()
    return _cache[name]


def cases(oracle):
    """name -> Case, every stream of the set (built once per process)."""
    if "text" not in _cache:
        _cache["text"] = text_cases(oracle)
    out = {c.name: c for c in _cache["text"]}
    out.update((name, designed(name)) for name in DESIGNED)
    return out


def n_out(case):
    """Bytes a designed stream produces with ample room, from the bookkeeping."""
    return case.props.get("n_out", sum(tk.produced for tk in case.tokens))
