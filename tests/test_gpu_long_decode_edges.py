"""GPU tier: the long-stream decoder (tamp_decompress_long_kernel.hpp, long_decode_front / launch_decompress_long in tamp_capi.hip)
on token streams BUILT at its boundaries (tests/long_stream_writer.py; tests/test_long_stream_writer.py asserts that every stream
has the property it is named for).  Every stream goes through ``decompress_batch`` with TAMP_AMD_LONGDEC_MIN=64 and
TAMP_AMD_LONGDEC_DEBUG=1: status, bytes and consumed count are the checker's (the reference C where it is built, else the oracle),
bit for bit; the debug lines say whether the long path decoded the stream or declined it -- and its chunks, groups, tokens, list
entries, window_pos blocks and scan blocks are the writer's numbers.  Then once more with TAMP_AMD_LONGDEC=0: the same triple and not
a line.  The streams are a few KB to 100 KB; up to sixteen share a call."""
import re

import numpy as np
import pytest

import long_stream_writer as lsw
from long_stream_writer import designed

pytestmark = pytest.mark.gpu

TUNING_ENV = ("TAMP_AMD_DECODER", "TAMP_AMD_SPLIT_SLICE_LOG2", "TAMP_AMD_SPLIT_SCRATCH_MB", "TAMP_AMD_SPLIT_WAVE_MAX",
              "TAMP_AMD_SPLIT_SPW", "TAMP_AMD_SCRATCH_MB", "TAMP_AMD_LONGDEC", "TAMP_AMD_LONGDEC_MIN", "TAMP_AMD_SPLIT_FAIL_ABOVE",
              "TAMP_AMD_LONGDEC_EXT", "TAMP_AMD_LONGDEC_CHAIN")

FRONT = re.compile(r"\[tamp_amd long (decode|size query)\] (\d+) bytes, (\d+) chunks, (\d+) sync rounds, settled (\d)$")
DECODE = re.compile(r"\[tamp_amd long decode\] (\d+) groups, (\d+) tokens, (\d+) bytes out, (\d+) entries, (\d+) wp blocks, "
                    r"max lags (\d+), (\d+) early groups, (\d+) scan blocks$")
SIZED = re.compile(r"\[tamp_amd long size query\] (\d+) bytes out, limit (\d+)$")
DECLINED = re.compile(r"\[tamp_amd long (decode|size query)\] declined: (.+)$")


@pytest.fixture(scope="module")
def ta():
    import tamp_amd
    from tamp_amd import _lib

    _lib.load()  # raises if the native library is missing: no silent fallback
    return tamp_amd


@pytest.fixture(scope="module")
def checker():
    from oracle.checker import Oracle, Ref

    return Ref() if Ref.available() else Oracle()


@pytest.fixture(autouse=True)
def long_path_with_debug_lines(monkeypatch):
    for k in TUNING_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TAMP_AMD_LONGDEC_MIN", "64")
    monkeypatch.setenv("TAMP_AMD_LONGDEC_DEBUG", "1")


def reports(err):
    """The debug lines of one call, a dict per stream the long path looked at."""
    out, cur = [], None
    for line in err.splitlines():
        if "[tamp_amd long" not in line:
            continue
        if m := FRONT.search(line):
            cur = dict(bytes=int(m[2]), chunks=int(m[3]), rounds=int(m[4]), settled=int(m[5]))
            out.append(cur)
        elif m := DECODE.search(line):
            assert cur is not None and "taken" not in cur and "declined" not in cur, err
            cur.update(taken=True, groups=int(m[1]), tokens=int(m[2]), out=int(m[3]), entries=int(m[4]), wp_blocks=int(m[5]),
                       max_lags=int(m[6]), early=int(m[7]), scan_blocks=int(m[8]))
        elif m := SIZED.search(line):
            cur.update(sized=int(m[1]))
        elif m := DECLINED.search(line):
            if cur is None or "taken" in cur or "declined" in cur:  # (header, format and dictionary gates: in front of the first line)
                cur = {}
                out.append(cur)
            cur["declined"] = m[2]
        else:
            raise AssertionError("an unknown debug line: " + line)
    return out


def decode(ta, checker, capfd, monkeypatch, blobs, caps, dictionary=None, max_window_bits=15, want=None):
    """One call through the long path and one with it switched off: both the checker's triples.  -> the first call's reports."""
    if want is None:
        want = [checker.decompress(b, cap=c, dictionary=dictionary, max_window_bits=max_window_bits) for b, c in zip(blobs, caps)]
    capfd.readouterr()
    r = ta.decompress_batch(blobs, out_cap=np.asarray(caps, dtype=np.uint32), dictionary=dictionary, max_window_bits=max_window_bits)
    err = capfd.readouterr().err
    for i, w in enumerate(want):
        assert (int(r.status[i]), int(r.in_consumed[i])) == (w[0], w[2]), (i, err)
        assert bytes(r.stream(i)) == w[1], i
    monkeypatch.setenv("TAMP_AMD_LONGDEC", "0")
    r = ta.decompress_batch(blobs, out_cap=np.asarray(caps, dtype=np.uint32), dictionary=dictionary, max_window_bits=max_window_bits)
    off = capfd.readouterr().err
    monkeypatch.delenv("TAMP_AMD_LONGDEC")
    assert "[tamp_amd long" not in off
    for i, w in enumerate(want):
        assert (int(r.status[i]), bytes(r.stream(i)), int(r.in_consumed[i])) == w, i
    return reports(err)


def assert_taken(rep, nb, record=None, name=""):
    """The long path decoded the stream, and counted what the writer counted."""
    assert rep.get("taken") and rep["settled"] == 1, rep
    got = {k: rep[k] for k in ("bytes", "chunks", "groups", "tokens", "out", "entries", "wp_blocks", "max_lags", "early", "scan_blocks")}
    want = dict(bytes=nb.n_bytes, chunks=nb.chunks, groups=nb.groups, tokens=nb.tokens, out=nb.out, entries=nb.entries,
                wp_blocks=nb.wp_blocks, max_lags=nb.max_lags, early=nb.early, scan_blocks=nb.scan_blocks)
    if record is not None:
        record(name, " ".join(f"{k}={v}" for k, v in got.items()) + f" rounds={rep['rounds']}")
    assert got == want, name


def run_designed(ta, checker, capfd, monkeypatch, record, names, chain=True):
    streams = [designed(n) for n in names]
    reps = decode(ta, checker, capfd, monkeypatch, [s.blob for s in streams], [s.produced + 64 for s in streams])
    assert len(reps) == len(names), reps
    for n, s, rep in zip(names, streams, reps):
        assert_taken(rep, s.numbers(chain=chain), record, n + ("" if chain else " (CHAIN=0)"))
    return reps


@pytest.fixture
def record(record_property):
    return lambda name, text: record_property(name, text)


@pytest.mark.parametrize("fmt", ["v1", "ext"])
def test_chunk_edges(ta, checker, capfd, monkeypatch, record, fmt):
    """Literal-only and match-only streams with a token start at every bit phase of a chunk boundary; FLUSH tokens whose padding
    ends on a boundary (all eight pad lengths), as a chunk's first and last token, and a chunk of FLUSH tokens only."""
    run_designed(ta, checker, capfd, monkeypatch, record, [f"literals {fmt}", f"matches {fmt}", f"flush {fmt}"])


@pytest.mark.parametrize("fmt", ["v1", "ext"])
def test_sync_across_workgroups(ta, checker, capfd, monkeypatch, record, fmt):
    """One token repeated over 200 chunks: the starts settle a workgroup of 64 chunks per round.  The same blob cut to 63, 64, 65, 128
    and 129 chunks: the last chunk and lane 63 of tamp_long_sync_kernel each write the start behind them."""
    s = designed(f"periodic {fmt}")
    lens = [len(s.blob)] + lsw.chunk_cut_lengths(s)
    reps = decode(ta, checker, capfd, monkeypatch, [s.blob[:n] for n in lens], [s.produced + 64] * len(lens))
    assert len(reps) == len(lens)
    for n, rep in zip(lens, reps):
        assert_taken(rep, s.numbers(n), record, f"periodic {fmt} {n} bytes")
    assert reps[0]["rounds"] >= 3 and [r["chunks"] for r in reps] == [200, 63, 64, 65, 128, 129]


def _prefix_counts(s):
    ends, ntok, nout = [], [0], [0]
    for tk in s.tokens:
        ends.append(tk.bit + tk.nbits)
        ntok.append(ntok[-1] + (tk.kind != "F"))
        nout.append(nout[-1] + tk.produced)
    return np.asarray(ends), ntok, nout


@pytest.mark.parametrize("fmt", ["v1", "ext"])
def test_end_of_stream_cuts(ta, checker, capfd, monkeypatch, record, fmt):
    """70 chunks of mixed tokens cut at every byte of the last two chunks plus 8 bytes (a multiple of the chunk's bytes, one more,
    one fewer among them), sixteen cuts per call; 1..5 zero bytes and 1..5 0xFF bytes appended (the reference says what they mean);
    the size query on the uncut stream and sixteen cuts.  (v1: 1,032 cuts in 65 calls.)"""
    s = designed(f"mixed {fmt}")
    cb = lsw.CHUNK_BITS_EXT if s.extended else lsw.CHUNK_BITS_V1
    ends, ntok, nout = _prefix_counts(s)
    cuts = lsw.end_cuts(s)
    cap = s.produced + 64
    for at in range(0, len(cuts), 16):
        lens = cuts[at : at + 16]
        reps = decode(ta, checker, capfd, monkeypatch, [s.blob[:n] for n in lens], [cap] * len(lens))
        assert len(reps) == len(lens)
        for k, (n, rep) in enumerate(zip(lens, reps)):
            if k == 0:  # one cut per call against all of the writer's numbers, every cut against chunks, tokens and bytes
                assert_taken(rep, s.numbers(n))
            done = int(np.searchsorted(ends, 8 * n, side="right"))  # tokens the cut completes
            assert rep.get("taken") and (rep["bytes"], rep["chunks"], rep["tokens"], rep["out"]) == (n, (8 * n + cb - 1) // cb, ntok[done], nout[done]), n
    tails = [s.blob + t * k for t in (b"\0", b"\xff") for k in range(1, 6)]
    reps = decode(ta, checker, capfd, monkeypatch, tails, [cap + 64] * len(tails))
    assert len(reps) == len(tails)
    for blob, rep in zip(tails, reps):
        toks = lsw.read_tokens(blob)[0]
        assert_taken(rep, lsw.numbers(toks, len(blob), s.window, s.extended), record, f"mixed {fmt} + {len(blob) - len(s.blob)} x {blob[-1]:#x}")
    # the size query through the same front
    lens = [len(s.blob)] + cuts[5 :: len(cuts) // 16][:16]
    assert len(lens) == 17
    want = [checker.decompress(s.blob[:n], cap=cap) for n in lens]
    capfd.readouterr()
    got = []
    for at in (0, 16):
        q = ta.decoded_size_batch([s.blob[:n] for n in lens[at : at + 16]])
        got += [(int(q.status[i]), int(q.size[i]), int(q.in_consumed[i])) for i in range(len(q.size))]
    reps = reports(capfd.readouterr().err)
    assert got == [(w[0], len(w[1]), w[2]) for w in want]
    assert [(r.get("sized"), r["settled"]) for r in reps] == [(len(w[1]), 1) for w in want]


def test_group_cuts(ta, checker, capfd, monkeypatch, record):
    """Group 0 ends at exactly 32,768 output bytes; the twin would reach 32,769 and closes a chunk earlier.  With
    TAMP_AMD_LONGDEC_CHAIN=0 the same at 16,384 / 16,385 (kSplitMaxOut), and window 2^15 with every chunk full of the longest match:
    groups as small as the rule allows, three of them start inside the first W bytes (tamp_long_window_kernel for each)."""
    reps = run_designed(ta, checker, capfd, monkeypatch, record, ["group 32768", "group 32769"])
    assert [r["groups"] for r in reps] == [2, 2]
    monkeypatch.setenv("TAMP_AMD_LONGDEC_CHAIN", "0")
    reps = run_designed(ta, checker, capfd, monkeypatch, record, ["group 16384", "group 16385", "densest w15", "group 32768"], chain=False)
    assert reps[2]["early"] == 3 and reps[2]["scan_blocks"] == 0


def test_lag_cap(ta, checker, capfd, monkeypatch, record):
    """Extended format.  63 lagging RLE tokens in every one of 70 chunks: taken, every group one chunk, 70 groups (at window 2^15 all far
    shorter than W: the tail maps pass the window on through many groups); 64 in one chunk: declined; 20 per chunk: groups of three
    chunks, closed by the lag cap."""
    reps = run_designed(ta, checker, capfd, monkeypatch, record, ["lags 63 w10", "lags 63 w15", "lags 20"])
    assert [(r["groups"], r["max_lags"]) for r in reps] == [(70, 63), (70, 63), (24, 20)]
    s = designed("lags 64 in one chunk")
    reps = decode(ta, checker, capfd, monkeypatch, [s.blob], [s.produced + 64])
    assert len(reps) == 1 and reps[0]["declined"] == "lags per chunk" and (reps[0]["chunks"], reps[0]["settled"]) == (70, 1), reps


def test_scan_blocks(ta, checker, capfd, monkeypatch, record):
    """Exactly 64, 65, 128 and 129 groups (one, two, two and three blocks of the tail-map scan), every group's last tokens copying
    bytes written 3, 17 and 60 groups earlier and bytes of the initial dictionary that nothing has overwritten."""
    reps = run_designed(ta, checker, capfd, monkeypatch, record, ["groups 64", "groups 65", "groups 128", "groups 129"])
    assert [(r["groups"], r["scan_blocks"]) for r in reps] == [(64, 1), (65, 2), (128, 2), (129, 3)]


def test_window_pos_blocks(ta, checker, capfd, monkeypatch, record):
    """Extended format, windows 2^8 and 2^10: 4,200 list entries in three blocks of the window_pos chain, a chunk marker as a block's
    last entry, tokens clipped at the ring's end."""
    reps = run_designed(ta, checker, capfd, monkeypatch, record, ["wp blocks w8", "wp blocks w10"])
    assert [r["wp_blocks"] for r in reps] == [3, 3]


def test_sources(ta, checker, capfd, monkeypatch, record):
    """Matches whose source straddles the write cursor, the group's first byte, or is the byte just written; an RLE as the first token
    of the stream and of a group; an extended match of the maximum length from offset W - len."""
    run_designed(ta, checker, capfd, monkeypatch, record, ["sources", "sources v1"])
    monkeypatch.setenv("TAMP_AMD_LONGDEC_CHAIN", "0")
    run_designed(ta, checker, capfd, monkeypatch, record, ["sources v1"], chain=False)


@pytest.mark.parametrize("fmt", ["v1", "ext"])
def test_fresh_window(ta, checker, capfd, monkeypatch, record, fmt):
    """Window 2^15 with a custom dictionary: a group that starts inside the first W bytes copies dictionary bytes at ring indices not
    yet written, then group 0's bytes.  Without the dictionary argument: declined, and TAMP_INVALID_CONF from the exact decoders."""
    from oracle.checker import Oracle

    s = designed(f"fresh {fmt}")
    for chain in (True, False) if fmt == "v1" else (True,):
        if not chain:
            monkeypatch.setenv("TAMP_AMD_LONGDEC_CHAIN", "0")
        reps = decode(ta, checker, capfd, monkeypatch, [s.blob], [s.produced + 64], dictionary=s.dictionary)
        assert len(reps) == 1
        assert_taken(reps[0], s.numbers(chain=chain), record, f"fresh {fmt}" + ("" if chain else " (CHAIN=0)"))
        assert reps[0]["early"] == (2 if chain else 3)
    monkeypatch.delenv("TAMP_AMD_LONGDEC_CHAIN", raising=False)
    want = [Oracle().decompress(s.blob, cap=s.produced + 64)]  # (the library's rule; the reference's C leaves the window to its caller)
    assert want[0][0] == -3
    reps = decode(ta, checker, capfd, monkeypatch, [s.blob], [s.produced + 64], want=want)
    assert reps == [dict(declined="dictionary")]


def test_declines(ta, checker, capfd, monkeypatch):
    """One stream per reason the long path hands a stream to the exact decoders; the triple is the checker's every time."""
    import random

    s = designed("bad offset")
    reps = decode(ta, checker, capfd, monkeypatch, [s.blob], [s.produced + 64])
    assert len(reps) == 1 and reps[0]["declined"] == "offset out of window" and reps[0]["settled"] == 1, reps
    assert checker.decompress(s.blob, cap=s.produced + 64)[0] == -4
    s = designed("mixed v1")
    for cap in (s.produced, s.produced - 1):
        reps = decode(ta, checker, capfd, monkeypatch, [s.blob], [cap])
        assert len(reps) == 1 and reps[0]["declined"] == "output room", reps
    w = lsw.TokenWriter(10, 8, False, more=0)  # the dictionary-reset bit, and the second header byte it announces
    lsw.mixed(w, random.Random(1), 20 * w.chunk_bits)
    assert decode(ta, checker, capfd, monkeypatch, [w.blob()], [w.out + 64]) == [dict(declined="header")]
    w = lsw.TokenWriter(12, 8, True)
    lsw.mixed(w, random.Random(2), 20 * w.chunk_bits)
    assert decode(ta, checker, capfd, monkeypatch, [w.blob()], [w.out + 64], max_window_bits=10) == [dict(declined="header")]
    s = designed("mixed ext")
    monkeypatch.setenv("TAMP_AMD_LONGDEC_EXT", "0")
    assert decode(ta, checker, capfd, monkeypatch, [s.blob], [s.produced + 64]) == [dict(declined="extended off")]


SIXTEEN = ["literals v1", "matches ext", "flush v1", "flush ext", "mixed v1", "mixed ext", "group 32768", "lags 63 w10", "lags 63 w15",
           "lags 20", "groups 65", "wp blocks w8", "sources", "sources v1", "densest w15", "periodic ext"]


def test_sixteen_streams_in_one_call(ta, checker, capfd, monkeypatch, record):
    """Sixteen different designed streams, both formats, in one call -- from host memory and as device tensors: sixteen decode lines,
    each stream its own triple."""
    import torch

    run_designed(ta, checker, capfd, monkeypatch, record, SIXTEEN)
    streams = [designed(n) for n in SIXTEEN]
    flat, off, ln = ta.batch.pack_streams([s.blob for s in streams])
    dev = torch.device("cuda:0")
    caps = np.asarray([s.produced + 64 for s in streams], dtype=np.int64)
    capfd.readouterr()
    r = ta.decompress_batch(torch.from_numpy(flat).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                            torch.from_numpy(ln.astype(np.int32)).to(dev), out_cap=torch.from_numpy(caps).to(dev))
    torch.cuda.synchronize()
    reps = reports(capfd.readouterr().err)
    assert len(reps) == 16
    status, consumed = r.status.cpu().numpy(), r.in_consumed.cpu().numpy()
    for i, (n, s, rep) in enumerate(zip(SIXTEEN, streams, reps)):
        assert_taken(rep, s.numbers(), None, n)
        assert (int(status[i]), bytes(r.stream(i)), int(consumed[i])) == checker.decompress(s.blob, cap=s.produced + 64), n
