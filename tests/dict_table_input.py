"""Inputs of the dictionary-table tests (tests/test_dict_table_host.py, tests/test_gpu_dict_table.py), built in code from seeds
and small strings.

K = 5 dictionaries of ``1 << window`` bytes, each filled with its own small vocabulary (five disjoint word lists, repeated to
length), and streams drawn mostly from ONE dictionary's vocabulary plus a few noise bytes.  A stream therefore compresses to
other bytes under its own dictionary than under any foreign one -- ``assert_inputs_detect_an_ignored_selector`` below (run by
tests/test_dict_table_host.py) proves with the oracle alone that every stream whose selector is not 0 differs from what
dictionary 0 would give, so a launch that ignored the selector (or applied a neighbour's) cannot pass the byte comparisons of
the GPU tier.

A stream of 0 or 1 bytes is the same bytes under every dictionary (a header; a header and one literal): ``selectors_and_lengths``
gives those two lengths to streams of selector 0 only.
"""
import functools

import numpy as np

K = 5
# five disjoint word lists (ASCII below 128: literal 7 takes them too); short words first so that a 256-byte dictionary holds many
VOCAB = (
    "volt amp ohm watt phase grid relay fuse meter surge load trip feeder breaker busbar".split(),
    "temp hum dew wind gust rain hail fog baro cloud frost storm drizzle sleet squall".split(),
    "lat lon alt fix sat hdop knot bear head track yaw pitch roll drift geoid".split(),
    "rpm oil cam rod gear cog pump valve boost knock idle choke piston gasket clutch".split(),
    "ack nak syn fin rst ttl mtu crc seq hop port peer route frame jitter".split(),
)
assert len({w for v in VOCAB for w in v}) == sum(len(v) for v in VOCAB), "the vocabularies share no word"

LONG_LENGTHS = (15, 16, 17, 300, 1023, 1024, 4096, 9000)  # with 0 and 1 (selector 0 only): the lengths of the GPU tier


def dictionaries(window):
    """-> K dictionaries of ``1 << window`` bytes: dictionary k is vocabulary k as ``word=`` fields, repeated to length."""
    size = 1 << window
    out = []
    for k in range(K):
        unit = "".join(f"{w}={(7 * i + k) % 10};" for i, w in enumerate(VOCAB[k])).encode()
        out.append((unit * (size // len(unit) + 1))[:size])
    return out


@functools.lru_cache(maxsize=None)
def stream(k, n, seed, noise=0.04, literal=8):
    """``n`` bytes of ``word=digit;`` fields from vocabulary ``k`` with a noise byte now and then (below ``1 << literal``)."""
    rng = np.random.default_rng(1000 * seed + k)
    out = bytearray()
    while len(out) < n:
        if rng.random() < noise:
            out.append(int(rng.integers(0, 1 << min(literal, 8))))
        w = VOCAB[k][int(rng.integers(0, len(VOCAB[k])))]
        out += f"{w}={int(rng.integers(0, 10))};".encode()
    return bytes(out[:n])


def selectors_and_lengths(max_len=None):
    """160 (selector, length) pairs: 80 streams with selector ``i % 5``, a block of 40 with selector 3, 40 with ``4 - i % 5`` --
    runs of equal and of alternating selectors both occur.  The lengths cycle through LONG_LENGTHS (capped at ``max_len``); in
    the first and the last part the first two streams of selector 0 are 0 and 1 bytes long instead."""
    sel = [i % K for i in range(80)] + [3] * 40 + [K - 1 - i % K for i in range(40)]
    lens = [LONG_LENGTHS[i % len(LONG_LENGTHS)] for i in range(len(sel))]
    for lo, hi in ((0, 80), (120, 160)):
        zeros = [i for i in range(lo, hi) if sel[i] == 0]
        lens[zeros[0]], lens[zeros[1]] = 0, 1
    if max_len is not None:
        lens = [min(n, max_len) for n in lens]
    return sel, lens


def batch(window, literal=8, max_len=None):
    """-> (dictionaries, selectors, streams) of the 160-stream batch at this window."""
    sel, lens = selectors_and_lengths(max_len)
    return dictionaries(window), sel, [stream(k, n, i, literal=literal) for i, (k, n) in enumerate(zip(sel, lens))]


# (window, literal, extended, lazy, max_len): the configurations the GPU tier compresses
CONFIGS = ((10, 8, True, False, None), (10, 8, False, False, None), (8, 7, True, False, 256), (15, 8, True, False, None),
           (10, 8, True, True, None))


def assert_inputs_detect_an_ignored_selector(oracle):
    for window, literal, extended, lazy, max_len in CONFIGS:
        dicts, sel, streams = batch(window, literal, max_len)
        assert {0, 1} <= {len(s) for s in streams} and all(k == 0 for k, s in zip(sel, streams) if len(s) < 2)
        for i, (k, s) in enumerate(zip(sel, streams)):
            kw = dict(window=window, literal=literal, extended=extended, lazy_matching=lazy)
            st_own, own = oracle.compress(s, dictionary=dicts[k], **kw)
            assert st_own == 0, (window, i)
            if k != 0:
                st_0, under_0 = oracle.compress(s, dictionary=dicts[0], **kw)
                assert st_0 == 0 and own != under_0, (window, literal, extended, i, k, len(s))
            # and it decodes under its own dictionary alone
            assert oracle.decompress(own, dictionary=dicts[k])[:2] == (2, s) or len(s) == 0, (window, i)
