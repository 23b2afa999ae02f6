"""GPU tier (-m gpu): the decoded-size query (tamp_batch_decoded_size / tamp_amd.decoded_size_batch) and what is built on it.

The contract: per stream exactly the out_len, status and in_consumed that tamp_batch_decompress returns for the same call with
out_cap[i] = limit[i] (no limit: 0xFFFFFFFF), and no output bytes.  The checker is the oracle's decoder
(oracle.decompress -> (status, bytes, consumed)); where a test compares with a decode call instead, it says so.
"""
import io
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
from conftest import load_golden, unb64

pytestmark = pytest.mark.gpu

BIG = 1 << 20


@pytest.fixture(scope="module")
def ta():
    import tamp_amd
    from tamp_amd import _lib

    assert _lib.load().tamp_amd_device_count() >= 1, "no HIP device visible"
    return tamp_amd


def _triples(q, n=None):
    size, status, used = (np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x) for x in (q.size, q.status, q.in_consumed))
    size, used = size.view(np.uint32), used.view(np.uint32)
    return [(int(size[i]), int(status[i]), int(used[i])) for i in range(len(status) if n is None else n)]


def _want(oracle, blob, cap=BIG, dictionary=None):
    st, out, used = oracle.decompress(blob, dictionary=dictionary, cap=cap)
    return (len(out), st, used)


# ---------------------------------------------------------------------------------------------------------------
# 1. fixtures
# ---------------------------------------------------------------------------------------------------------------
def test_known_answers_and_device_vectors(ta, oracle):
    ka = load_golden("known_answers.json")["decompress"]
    seen = set()
    for c in ka:
        blob, d = bytes.fromhex(c["compressed"]), unb64(c["dictionary"])
        for dictionary in ([d, None] if d is not None else [None]):
            got = _triples(ta.decoded_size_batch([blob], dictionary=dictionary))[0]
            assert got == _want(oracle, blob, dictionary=dictionary), (c["name"], dictionary is not None)
            seen.add(got[1])
        if d is not None:  # only the dictionary's length matters: any bytes of that length give the same answer
            got = _triples(ta.decoded_size_batch([blob], dictionary=bytes(len(d))))[0]
            assert got == _want(oracle, blob, dictionary=d), c["name"]
        assert _triples(ta.decoded_size_batch([blob], dictionary=d))[0][1] == c["status"], c["name"]
    vs = load_golden("device_vectors.json")
    blobs = [unb64(v["data"]) for v in vs]
    got = _triples(ta.decoded_size_batch(blobs))
    for j, v in enumerate(vs):
        assert got[j] == _want(oracle, blobs[j]), v["name"]
        assert got[j] == (len(unb64(v["output"])), v["status"], v["consumed"]), v["name"]
        seen.add(got[j][1])
    assert {2, -3, -4} <= seen


# ---------------------------------------------------------------------------------------------------------------
# 2. limits inside tokens
# ---------------------------------------------------------------------------------------------------------------
def _every_limit(ta, oracle, blob, plain_len, dictionary, name):
    limits = list(range(0, plain_len + 2))
    q = ta.decoded_size_batch([blob] * len(limits), limit=np.array(limits, dtype=np.uint32), dictionary=dictionary)
    got = _triples(q)
    statuses = set()
    for j, cap in enumerate(limits):
        assert got[j] == _want(oracle, blob, cap=cap, dictionary=dictionary), (name, cap)
        statuses.add(got[j][1])
    return statuses


def test_limits_inside_tokens(ta, oracle):
    for c in load_golden("known_answers.json")["decompress"]:
        if c["status"] != 2:
            continue
        statuses = _every_limit(ta, oracle, bytes.fromhex(c["compressed"]), len(unb64(c["expected"])), unb64(c["dictionary"]), c["name"])
        assert statuses == {1, 2}, c["name"]
    # an RLE token (100 equal bytes) and an extended match (a 40-byte phrase again: longer than any plain match) with text around them
    rng = random.Random(5)
    phrase = bytes(rng.randrange(97, 123) for _ in range(40))
    for name, plain in (("rle", b"ab" + b"x" * 100 + b"cd"), ("extended_match", phrase + b"--" + phrase + b"!")):
        st, blob = oracle.compress(plain, extended=True)
        assert st == 0 and len(blob) < len(plain) - 30, name  # (the run / the repeat took a few bytes)
        assert oracle.decompress(blob, cap=BIG)[1] == plain
        assert _every_limit(ta, oracle, blob, len(plain), None, name) == {1, 2}
    # an int limit is every stream's limit; 0xFFFFFFFF is "none"
    st, blob = oracle.compress(b"ab" + b"x" * 100 + b"cd")
    assert _triples(ta.decoded_size_batch([blob, blob], limit=50)) == [_want(oracle, blob, cap=50)] * 2
    assert _triples(ta.decoded_size_batch([blob], limit=0xFFFFFFFF)) == [(104, 2, len(blob))]


# ---------------------------------------------------------------------------------------------------------------
# 3. ragged differential
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(oracle):
    """~2,000 streams of every configuration, a tenth truncated, a tenth with a flipped bit, and compressed lengths pinned on the
    thresholds of the kernel's two loops; with the oracle's (size, status, consumed) at cap 2^20, computed once."""
    from tamp_amd import workloads as wl

    rng = random.Random(20261018)
    nprng = np.random.default_rng(20261018)
    corpora = [wl.frozen_corpus(k) for k in ("prose", "python", "markup")]
    jobs = []
    for i in range(1700):
        kind = rng.randrange(6)
        if kind < 3:
            n = rng.randrange(0, 6001)
            at = rng.randrange(0, len(corpora[kind]) - n)
            plain = corpora[kind][at : at + n]
        elif kind < 5:
            plain = nprng.integers(0, 256, rng.randrange(0, 6001) if kind == 3 else rng.randrange(0, 300), dtype=np.uint8).tobytes()
        else:
            plain = bytes([rng.randrange(256)]) * rng.randrange(2, 701)
        window, literal = 8 + i % 8, 5 + (i // 8) % 4
        extended, dreset = bool((i // 32) % 2), bool((i // 64) % 2)
        plain = (np.frombuffer(plain, dtype=np.uint8) & np.uint8((1 << literal) - 1)).tobytes()
        jobs.append((plain, dict(window=window, literal=literal, extended=extended, dictionary_reset=dreset)))
    # (the oracle's encoder searches the whole window per position: the calls run side by side, ctypes releases the GIL)
    with ThreadPoolExecutor(max_workers=8) as pool:
        compressed = list(pool.map(lambda j: oracle.compress(j[0], **j[1]), jobs))
    streams, long_ones = [], {}
    for (plain, conf), (st, blob) in zip(jobs, compressed):
        extended, dreset = conf["extended"], conf["dictionary_reset"]
        assert st == 0
        if len(blob) >= 1100 and len(long_ones.setdefault((extended, dreset), [])) < 6:
            long_ones[(extended, dreset)].append(blob)
        r = rng.random()
        if r < 0.1 and len(blob) > 1:
            blob = blob[: rng.randrange(0, len(blob))]
        elif r < 0.2 and blob:
            b = bytearray(blob)
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            blob = bytes(b)
        streams.append(blob)
    assert sorted(long_ones) == [(False, False), (False, True), (True, False), (True, True)]
    assert all(len(v) == 6 for v in long_ones.values())
    for blob in sum(long_ones.values(), []):  # (hs: 1 header byte, 2 with dictionary_reset)
        hs = 1 + (blob[0] & 1)
        for n in (0, 1, 2, hs + 7, hs + 8, 63, 64, 65, hs + 159, hs + 160, hs + 161, 1023, 1024, 1025):
            streams.append(blob[:n])
        streams.append(bytes([blob[0] | 1, 1]))              # a second header byte that is not zero
        streams.append(bytes([blob[0] | 1, 1]) + blob[2:200])
        streams.append(bytes([blob[0] | 1]))                 # ... and one that is missing
    oob = bytes.fromhex(next(c["compressed"] for c in load_golden("known_answers.json")["decompress"] if c["status"] == -4))
    streams += [oob, streams[0][:40] + oob[1:], oob + streams[1][:40]]
    order = list(range(len(streams)))
    rng.shuffle(order)
    streams = [streams[i] for i in order]
    want = [_want(oracle, s) for s in streams]
    assert {w[1] for w in want} >= {2, -3, -4} and len({w[0] for w in want}) > 500
    return streams, want


@pytest.mark.parametrize("spw", [None, 16, 32, 64])
def test_ragged_batch_equals_the_oracle(ta, ragged, monkeypatch, spw):
    streams, want = ragged
    if spw is None:
        monkeypatch.delenv("TAMP_AMD_SPLIT_SPW", raising=False)
    else:
        monkeypatch.setenv("TAMP_AMD_SPLIT_SPW", str(spw))
    got = _triples(ta.decoded_size_batch(streams))
    bad = [(i, len(streams[i]), got[i], want[i]) for i in range(len(streams)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])
    for n in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257):
        assert _triples(ta.decoded_size_batch(streams[:n])) == want[:n], n


# ---------------------------------------------------------------------------------------------------------------
# 4. a dictionary reset inside the stream changes nothing
# ---------------------------------------------------------------------------------------------------------------
def test_dictionary_reset_inside_the_stream(ta, oracle):
    from tamp_amd import workloads as wl

    text = wl.frozen_corpus("prose")
    blobs, plains = [], []
    for k, (window, extended) in enumerate(((8, True), (10, False), (12, True), (15, False))):
        parts = [text[10_000 * k + 700 * j : 10_000 * k + 700 * j + 300 + 90 * j] for j in range(4)]
        ops = []
        for p in parts:
            ops += [("write", p), ("reset",)]
        ops += [("write", b"tail"), ("close",)]
        st, blob = oracle.stream_script(ops, window=window, extended=extended, dictionary_reset=True)
        assert st == 0
        blobs.append(blob), plains.append(b"".join(parts) + b"tail")
    with io.BytesIO() as f:
        c = ta.Compressor(f, dictionary_reset=True)
        c.write(text[:500]), c.reset_dictionary(), c.write(text[500:1500]), c.reset_dictionary(), c.write(text[:40]), c.close()
        blobs.append(f.getvalue()), plains.append(text[:500] + text[500:1500] + text[:40])
    got = _triples(ta.decoded_size_batch(blobs))
    for j, blob in enumerate(blobs):
        assert got[j][:2] == (len(plains[j]), 2), j
        assert got[j] == _want(oracle, blob), j
        assert oracle.decompress(blob, cap=BIG)[1] == plains[j]


# ---------------------------------------------------------------------------------------------------------------
# 5. a big grid
# ---------------------------------------------------------------------------------------------------------------
def test_big_grid_of_telemetry_messages(ta, monkeypatch):
    import torch

    from tamp_amd import workloads as wl

    n = 131_073
    dev = torch.device("cuda:0")
    d8 = wl.telemetry_dictionary(bytes(ta.initialize_dictionary(256, literal=7)))
    rows = wl.telemetry(n, 256)
    in_off, in_len = wl.csr_for_fixed(n, 256)
    comp = ta.compress_batch(torch.from_numpy(rows.reshape(-1)).to(dev), torch.from_numpy(in_off.astype(np.int64)).to(dev),
                             torch.from_numpy(in_len.astype(np.int32)).to(dev), window=8, literal=7, dictionary=d8, max_in_len=256)
    assert bool((comp.status == 0).all())
    for spw in (None, 16):  # (16 streams per wavefront: more workgroups than one grid holds, the kernel strides)
        if spw:
            monkeypatch.setenv("TAMP_AMD_SPLIT_SPW", str(spw))
        q = ta.decoded_size_batch(comp.out, comp.out_off, comp.out_len, dictionary=d8)
        assert bool((q.size == 256).all()) and bool((q.status == 2).all()), spw
        assert bool((q.in_consumed == comp.out_len).all()), spw
        q = ta.decoded_size_batch(comp.out, comp.out_off, comp.out_len)  # dictionary_len = 0
        assert bool((q.status == -3).all()) and bool((q.size == 0).all()), spw


# ---------------------------------------------------------------------------------------------------------------
# 6. forms and paths agree
# ---------------------------------------------------------------------------------------------------------------
def test_forms_and_paths_agree(ta, ragged, monkeypatch):
    import torch

    streams, want = ragged
    assert _triples(ta.decoded_size_batch(streams)) == want
    flat, in_off, in_len = ta.pack_streams(streams)
    assert _triples(ta.decoded_size_batch(flat, in_off, in_len)) == want
    limits = np.array([(7 * i) % 900 for i in range(len(streams))], dtype=np.uint32)
    limited = _triples(ta.decoded_size_batch(flat, in_off, in_len, limit=limits))
    assert {t[1] for t in limited} >= {1, 2}
    dev = torch.device("cuda:0")
    t_flat, t_off, t_len = (torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(in_off.astype(np.int64)).to(dev),
                            torch.from_numpy(in_len.astype(np.int32)).to(dev))
    assert _triples(ta.decoded_size_batch(t_flat, t_off, t_len)) == want
    assert _triples(ta.decoded_size_batch(t_flat, t_off, t_len, limit=torch.from_numpy(limits.astype(np.int64)).to(dev))) == limited
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    q = ta.decoded_size_batch(t_flat, t_off, t_len, stream=side.cuda_stream)
    side.synchronize()
    assert _triples(q) == want
    q = ta.decoded_size_batch(t_flat, t_off, t_len, limit=17, stream=side.cuda_stream, timing=True)
    side.synchronize()
    assert _triples(q) == _triples(ta.decoded_size_batch(streams, limit=17)) and q.kernel_ms > 0
    monkeypatch.setenv("TAMP_AMD_FANOUT", "3")
    assert _triples(ta.decoded_size_batch(streams, device=-1)) == want
    assert _triples(ta.decoded_size_batch(flat, in_off, in_len, limit=limits, device=-1)) == limited


# ---------------------------------------------------------------------------------------------------------------
# 7. decompress_batch(out_cap=None)
# ---------------------------------------------------------------------------------------------------------------
def _decoded(res, n):
    out_off, out_len, status, used = (np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
                                      for x in (res.out_off, res.out_len, res.status, res.in_consumed))
    out = res.out.cpu().numpy() if hasattr(res.out, "cpu") else res.out
    return [(int(status[i]), out[int(out_off[i]) : int(out_off[i]) + int(out_len.view(np.uint32)[i])].tobytes(),
             int(used.view(np.uint32)[i])) for i in range(n)]


def test_decompress_batch_without_out_cap(ta, ragged, oracle):
    import torch

    streams, want = ragged
    n = len(streams)
    flat, in_off, in_len = ta.pack_streams(streams)
    dev = torch.device("cuda:0")
    t_flat, t_off, t_len = (torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(in_off.astype(np.int64)).to(dev),
                            torch.from_numpy(in_len.astype(np.int32)).to(dev))
    # the reference: the explicit capacity (slabs of 2^20 bytes in device memory; only the produced bytes come back)
    ref = ta.decompress_batch(t_flat, t_off, t_len, out_cap=BIG)
    r_off, r_len, r_st, r_used = (x.cpu().numpy() for x in (ref.out_off, ref.out_len, ref.status, ref.in_consumed))
    full = [(int(r_st[i]), ref.out[int(r_off[i]) : int(r_off[i]) + int(r_len[i])].cpu().numpy().tobytes(), int(r_used[i])) for i in range(n)]
    del ref
    assert [(len(b), s, u) for s, b, u in full] == want
    total = sum(w[0] + 1 for w in want)
    host = ta.decompress_batch(streams)
    assert _decoded(host, n) == full
    assert total <= host.out.size <= total + 1
    dev_res = ta.decompress_batch(t_flat, t_off, t_len)
    assert _decoded(dev_res, n) == full
    assert dev_res.out.numel() == total
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    dev_res = ta.decompress_batch(t_flat, t_off, t_len, stream=side.cuda_stream)
    side.synchronize()
    assert _decoded(dev_res, n) == full
    # max_out: the explicit capacity of 100, in slabs of min(size + 1, 100)
    capped = _decoded(ta.decompress_batch(streams, out_cap=100), n)
    assert {c[0] for c in capped} >= {1, 2}
    total = sum(min(_want(oracle, s, cap=100)[0] + 1, 100) for s in streams)
    host = ta.decompress_batch(streams, max_out=100)
    assert _decoded(host, n) == capped and total <= host.out.size <= total + 1
    dev_res = ta.decompress_batch(t_flat, t_off, t_len, max_out=100)
    assert _decoded(dev_res, n) == capped and dev_res.out.numel() == total


# ---------------------------------------------------------------------------------------------------------------
# 8. one long stream: the chunk counts of the long decoder's front
# ---------------------------------------------------------------------------------------------------------------
def _text(kind, n):
    from tamp_amd import workloads as wl

    return wl.frozen_corpus(kind)[:n]


@pytest.mark.parametrize("kind", ["prose", "python"])
@pytest.mark.parametrize("extended", [False, True], ids=["v1", "extended"])
@pytest.mark.parametrize("window", [8, 12])
def test_long_stream_is_counted_by_chunks(ta, oracle, monkeypatch, capfd, kind, extended, window):
    plain = _text(kind, 200_000)
    blob = bytes(ta.compress(plain, window=window, extended=extended))
    assert len(blob) > 4096 and oracle.decompress(blob, cap=BIG)[1] == plain
    monkeypatch.setenv("TAMP_AMD_LONGDEC_MIN", "4096")
    monkeypatch.setenv("TAMP_AMD_LONGDEC_DEBUG", "1")
    capfd.readouterr()
    got = _triples(ta.decoded_size_batch([blob]))[0]
    err = capfd.readouterr().err
    assert got == (len(plain), 2, len(blob))
    assert "[tamp_amd long size query]" in err and "settled 1" in err, err
    # a limit below the size (and exactly the size): the lane kernel's answer, the oracle's triple at that cap
    for limit in (len(plain), len(plain) - 1, 70_001, 0):
        assert _triples(ta.decoded_size_batch([blob], limit=limit))[0] == _want(oracle, blob, cap=limit), limit
    assert _triples(ta.decoded_size_batch([blob], limit=len(plain) + 1))[0] == (len(plain), 2, len(blob))
    capfd.readouterr()
    monkeypatch.setenv("TAMP_AMD_LONGDEC", "0")
    assert _triples(ta.decoded_size_batch([blob]))[0] == got
    assert "[tamp_amd long" not in capfd.readouterr().err
    # two long streams and a short one in a call: whatever path answers, the same tables
    monkeypatch.delenv("TAMP_AMD_LONGDEC")
    assert _triples(ta.decoded_size_batch([blob, blob[:5000], blob])) == [got, _want(oracle, blob[:5000]), got]


def test_long_stream_of_rle_tokens_only(ta, monkeypatch, capfd):
    n = 2_000_000
    blob = bytes(ta.compress(bytes(n), extended=True))
    monkeypatch.setenv("TAMP_AMD_LONGDEC_MIN", "4096")
    monkeypatch.setenv("TAMP_AMD_LONGDEC_DEBUG", "1")
    assert len(blob) > 4096
    capfd.readouterr()
    assert _triples(ta.decoded_size_batch([blob]))[0] == (n, 2, len(blob))
    assert "[tamp_amd long size query]" in capfd.readouterr().err
    monkeypatch.setenv("TAMP_AMD_LONGDEC", "0")
    assert _triples(ta.decoded_size_batch([blob]))[0] == (n, 2, len(blob))
    assert _triples(ta.decoded_size_batch([blob], limit=1_000_000))[0][:2] == (1_000_000, 1)


@pytest.mark.parametrize("extended", [False, True], ids=["v1", "extended"])
def test_one_shot_decompress_sizes_the_blob_first(ta, extended):
    import inspect

    from tamp_amd import codec

    plain = (_text("prose", 700_000) + bytes(300_000)) if extended else _text("python", 900_000)
    blob = bytes(ta.compress(plain, extended=extended))
    assert len(blob) >= 256 << 10
    assert bytes(ta.decompress(blob)) == plain
    src = inspect.getsource(codec.decompress)
    assert "decoded_size_batch" in src and "factor" not in src and "64 x" not in src  # the 8 x / 64 x retry loop is gone
