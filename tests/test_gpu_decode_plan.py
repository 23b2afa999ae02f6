"""GPU tier (-m gpu): the decoder the launcher picks when NOTHING is forced, on small batches that sit on the choice boundaries of
DESIGN.md section 4.  Every batch is decoded through a device-memory call (the launcher sees the batch as it is) and compared
with the oracle's decoder -- bytes, sizes, status, consumed counts; then tamp_amd_decompress_plan, asked with the batch's own
facts computed on the host and the device's CU count, must name the decoder the design promises for that row.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPLIT, WAVE, LANE_LDS, LANE_GLOBAL = 0, 1, 2, 3  # include/tamp_amd.h TAMP_AMD_DECODER_*
TUNING_ENV = ("TAMP_AMD_DECODER", "TAMP_AMD_SPLIT_SLICE_LOG2", "TAMP_AMD_SPLIT_SCRATCH_MB", "TAMP_AMD_SPLIT_WAVE_MAX",
              "TAMP_AMD_SPLIT_SPW", "TAMP_AMD_SCRATCH_MB", "TAMP_AMD_LONGDEC", "TAMP_AMD_LONGDEC_MIN", "TAMP_AMD_SPLIT_FAIL_ABOVE")

# name: (messages, streams, out_cap, max_window_bits, header pre-pass allowed) -> decoder, and what else the plan must say.
# `messages` names a set of 256 compressed messages of the fixture below; more streams than that tile it.
ROWS = {
    # below 256 streams there is no pre-pass and nothing but the wave decoder
    "255 streams":            (("text4k", 255, 4104, 15, True), WAVE, dict(scan=0, max_window_bits=15)),
    # 256 streams of 512+ compressed bytes, capacity at most 16 KiB: split
    "256 streams":            (("text4k", 256, 4104, 15, True), SPLIT, dict(scan=1, max_window_bits=10, bulk=1, split_wave_resolve=0)),
    # the longest stream one byte under / at 512 compressed bytes: short messages at window 2^10 are split-decoder batches too,
    # but only streams of 512 bytes and more count as bulk
    "longest 511":            (("upto511", 256, 2048, 15, True), SPLIT, dict(scan=1, bulk=0, split_wave_resolve=1)),
    "longest 512":            (("upto512", 256, 2048, 15, True), SPLIT, dict(scan=1, bulk=1, split_wave_resolve=1)),
    # RESOLVE: a wavefront per stream up to 2 KiB of capacity, a workgroup above
    "out_cap 2048":           (("text4k", 256, 2048, 15, True), SPLIT, dict(split_wave_resolve=1, split_maxcap=2048)),
    "out_cap 2049":           (("text4k", 256, 2049, 15, True), SPLIT, dict(split_wave_resolve=0, split_maxcap=2049)),
    # capacity above 16 KiB is not a split-decoder batch; 256 long streams fill neither kind of lanes
    "out_cap 16384":          (("text4k", 256, 16384, 15, True), SPLIT, dict(split_maxcap=16384)),
    "out_cap 16385":          (("text4k", 256, 16385, 15, True), WAVE, dict(scan=1, max_window_bits=10)),
    # window 2^8, short messages: split with a custom dictionary, not without (and 256 of them do not fill the LDS lanes)
    "window 8, dictionary":   (("short8d", 256, 264, 15, True), SPLIT, dict(max_window_bits=8, bulk=0)),
    "window 8":               (("short8", 256, 264, 15, True), WAVE, dict(max_window_bits=8, bulk=0)),
    # limit 15 over window-2^10 streams: only the narrowed window fits LDS rows (8,192 short messages are a quarter of a round)
    "narrowed to 10":         (("short10", 8192, 16385, 15, True), LANE_LDS, dict(scan=1, max_window_bits=10, bulk=0, lane_lds_row=1028)),
    "not narrowed":           (("short10", 8192, 16385, 15, False), WAVE, dict(scan=0, max_window_bits=15, bulk=1)),
}


@pytest.fixture(scope="module")
def ta():
    import tamp_amd
    from tamp_amd import _lib

    lib = _lib.load()  # raises if the native library is missing: no silent fallback
    assert lib.tamp_amd_device_count() >= 1, "no HIP device visible"
    return tamp_amd


@pytest.fixture(autouse=True)
def unforced(monkeypatch):
    for k in TUNING_ENV:
        monkeypatch.delenv(k, raising=False)


def text_with_compressed_size(ta, text, target):
    """A piece of `text` that the library compresses (window 2^10) to exactly `target` bytes.  (A byte more of text can cost nine
    bits and so two bytes, and a longer match can save some: one run of prefixes skips sizes, eight starting points do not.)"""
    pieces = [text[start : start + n] for start in range(0, 16000, 2000) for n in range(600, 1200)]
    res = ta.compress_batch(pieces, window=10)
    sizes = [int(x) for x in res.out_len]
    assert target in sizes, (target, min(sizes), max(sizes))
    return pieces[sizes.index(target)]


@pytest.fixture(scope="module")
def messages(ta, oracle):
    """name -> (256 compressed streams, dictionary, {out_cap: the oracle's (status, bytes, consumed) per stream}); text from the
    frozen prose corpus, compressed by the library once."""
    from tamp_amd import workloads as wl

    blob = wl.real_text("prose", 3 << 20, frozen_only=True)
    assert len(blob) >= (2 << 20), "the frozen corpus (tests/golden/corpus_prose.txt.xz) is part of the tree"
    d8 = blob[-256:]

    def compress(msgs, **kw):
        res = ta.compress_batch(msgs, **kw)
        assert (np.asarray(res.status) == 0).all()
        return res.streams()

    text4k = [blob[i * 4096 : (i + 1) * 4096] for i in range(256)]
    short = [blob[(1 << 20) + i * 300 : (1 << 20) + i * 300 + 200 + i % 57] for i in range(256)]
    sets = {
        "text4k": (compress(text4k, window=10), None),
        "short10": (compress(short, window=10), None),
        "short8": (compress(short, window=8), None),
        "short8d": (compress(short, window=8, dictionary=d8), d8),
    }
    for target in (511, 512):  # 255 short messages and one whose compressed size is the target
        longest = compress([text_with_compressed_size(ta, blob[1 << 21 :], target)], window=10)
        assert len(longest[0]) == target and max(len(s) for s in sets["short10"][0]) < 511
        sets["upto%d" % target] = (sets["short10"][0][:100] + longest + sets["short10"][0][101:], None)
    assert min(len(s) for s in sets["text4k"][0]) >= 512
    return {name: (streams, d, {}) for name, (streams, d) in sets.items()}


def expected(oracle, messages, name, cap):
    streams, d, by_cap = messages[name]
    if cap not in by_cap:
        by_cap[cap] = [oracle.decompress(s, dictionary=d, cap=cap, max_window_bits=15) for s in streams]
    return by_cap[cap]


@pytest.mark.parametrize("row", list(ROWS))
def test_unforced_choice(ta, oracle, messages, row):
    import torch

    from tamp_amd import _lib
    from tamp_amd.batch import pack_streams

    (name, n, cap, limit, scan_headers), decoder, facts = ROWS[row]
    streams, d, _ = messages[name]
    want = expected(oracle, messages, name, cap)
    batch = [streams[i % 256] for i in range(n)]
    flat, off, ln = pack_streams(batch)
    dev = torch.device("cuda:0")
    res = ta.decompress_batch(torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                              torch.from_numpy(ln.astype(np.int32)).to(dev), out_cap=cap, dictionary=d, max_window_bits=limit,
                              scan_headers=scan_headers)
    torch.cuda.synchronize()
    out, out_len = res.out.cpu().numpy(), res.out_len.cpu().numpy()
    status, consumed = res.status.cpu().numpy(), res.in_consumed.cpu().numpy()
    bad = [i for i in range(n)
           if (int(status[i]), out[i * cap : i * cap + int(out_len[i])].tobytes(), int(consumed[i])) != tuple(want[i % 256])]
    assert not bad, (row, bad[:10])

    # the batch's own facts, as the header pre-pass finds them
    wbits = [8 + (s[0] >> 5) for s in batch]
    q = _lib.TampAmdDecodeQuery(n, limit | (0 if scan_headers else _lib.WINDOW_BITS_EXACT), d is not None, 0, 0,
                                torch.cuda.get_device_properties(0).multi_processor_count,
                                max(wbits), int(ln.max()), sum(1 << w for w in wbits) // 256, cap)
    plan = _lib.TampAmdDecodePlan()
    assert _lib.load().tamp_amd_decompress_plan(ctypes.byref(q), ctypes.byref(plan)) == 0
    assert plan.decoder == decoder, (row, plan.decoder)
    assert plan.long_attempt == 0  # (more than sixteen streams)
    for field, value in facts.items():
        assert getattr(plan, field) == value, (row, field, getattr(plan, field))
