"""CPU tier: the token writer of tests/long_stream_writer.py against the decoders' checkers, and every designed stream against
the property it was designed for -- asserted from the writer's bookkeeping (bit positions, bytes produced and written,
window_pos), never from decoded bytes.  tests/test_gpu_long_decode_edges.py aims the long-stream decoder
(tamp_decompress_long_kernel.hpp) with these streams; this file is the guarantee that it aims where it says."""
import pytest

import long_stream_writer as lsw
from long_stream_writer import designed


@pytest.fixture(scope="module")
def ref():
    from oracle.checker import Ref

    return Ref() if Ref.available() else None


def _decodes(oracle, ref, s, blob=None):
    blob = s.blob if blob is None else blob
    want = oracle.decompress(blob, cap=s.produced + 64, dictionary=s.dictionary)
    if ref is not None:
        assert ref.decompress(blob, cap=s.produced + 64, dictionary=s.dictionary) == want
    return want


@pytest.mark.parametrize("name", [n for n in lsw.DESIGNED if n != "bad offset"])
def test_designed_stream_decodes_whole_and_reads_back(oracle, ref, name):
    s = designed(name)
    st, out, used = _decodes(oracle, ref, s)
    assert (st, used, len(out)) == (2, len(s.blob), s.produced)
    assert lsw.read_tokens(s.blob)[0] == s.tokens
    assert len(s.blob) <= 110 << 10 and s.produced <= 1 << 20


def test_seeded_random_token_lists(oracle, ref):
    kinds, confs = set(), set()
    for seed in range(3000):
        s = lsw.random_token_list(seed)
        st, out, used = _decodes(oracle, ref, s)
        assert (st, used, len(out)) == (2, len(s.blob), s.produced), seed
        toks, window, literal, extended, hbits = lsw.read_tokens(s.blob)
        assert (toks, window, literal, extended, hbits) == (s.tokens, s.window, s.literal, s.extended, 8), seed
        for tk in s.tokens:  # what a token writes to the window (decompressor.c:162-170, 266-268)
            room = (1 << s.window) - tk.wp
            assert tk.written == {"L": 1, "M": tk.produced, "F": 0, "R": min(tk.produced, 8, room), "X": min(tk.produced, room)}[tk.kind]
        kinds |= {tk.kind for tk in s.tokens}
        confs.add((s.window, s.literal, s.extended))
    assert kinds == set("LMRXF") and len(confs) == 8 * 4 * 2


def _boundary_phases(s):
    """boundary - first bit, for the token that covers each chunk boundary's bit (0: it starts there)."""
    cb = lsw.CHUNK_BITS_EXT if s.extended else lsw.CHUNK_BITS_V1
    out = {}
    for tk in s.tokens:
        b = (tk.bit + tk.nbits - 1) // cb * cb
        if tk.bit <= b and b > 0:
            out[b] = (tk.kind, b - tk.bit, tk.nbits)
    return out


@pytest.mark.parametrize("name", ["literals v1", "literals ext", "matches v1", "matches ext"])
def test_chunk_edges_every_phase(name):
    s = designed(name)
    assert {tk.kind for tk in s.tokens} == s.props["kinds"] and s.numbers().chunks == 70
    ph = _boundary_phases(s)
    size = s.tokens[0].nbits
    assert len(ph) >= 69 and {p for _, p, _ in ph.values()} == set(range(size))
    # phase 0: a token ends exactly on the boundary; 1: the covering token starts one bit in front (the one before it ends 1 bit
    # before the boundary); size - 1: the covering token ends one bit behind it
    assert {0, 1, size - 1} <= s.props["phases"]


@pytest.mark.parametrize("name", ["flush v1", "flush ext"])
def test_flush_edges(name):
    s = designed(name)
    cb = lsw.CHUNK_BITS_EXT if s.extended else lsw.CHUNK_BITS_V1
    ends = {tk.nbits - 9 for tk in s.tokens if tk.kind == "F" and (tk.bit + tk.nbits) % cb == 0 and tk.bit % cb}
    assert ends == set(range(8))  # every pad length, padding ends on a boundary, the FLUSH is its chunk's last token
    assert any(tk.kind == "F" and tk.bit == s.props["flush_first"] * cb for tk in s.tokens)
    ct = s.numbers().table
    c = s.props["flush_only"]
    assert (ct.ntok[c], ct.outb[c], ct.nflush[c]) == (0, 0, cb // 16) and ct.n_chunks == 70


@pytest.mark.parametrize("name", ["periodic v1", "periodic ext"])
def test_periodic_stream_and_its_cuts(oracle, ref, name):
    s = designed(name)
    assert len({(tk.kind, tk.nbits, tk.produced) for tk in s.tokens}) == 1 and s.numbers().chunks == 200
    assert s.tokens[0].nbits % 2 and (lsw.CHUNK_BITS_V1 % s.tokens[0].nbits)  # no chunk boundary is in phase with the tokens for long
    for n, chunks in zip(lsw.chunk_cut_lengths(s), (63, 64, 65, 128, 129)):
        assert s.numbers(n).chunks == chunks
        assert _decodes(oracle, ref, s, s.blob[:n])[0] == 2


@pytest.mark.parametrize("name", ["mixed v1", "mixed ext"])
def test_end_of_stream_cuts(oracle, ref, name):
    s = designed(name)
    cbytes = (lsw.CHUNK_BITS_EXT if s.extended else lsw.CHUNK_BITS_V1) // 8
    cuts = lsw.end_cuts(s)
    assert len(s.blob) == 70 * cbytes and len(cuts) == 2 * cbytes + 8 and cuts[-1] == len(s.blob) - 1
    assert {68 * cbytes - 1, 68 * cbytes, 68 * cbytes + 1, 69 * cbytes - 1, 69 * cbytes, 69 * cbytes + 1} <= set(cuts)
    assert {tk.kind for tk in s.tokens} == set("LMRXF" if s.extended else "LMF")
    for n in cuts[::37]:
        st, out, used = _decodes(oracle, ref, s, s.blob[:n])
        nb = s.numbers(n)
        assert st == 2 and len(out) == nb.out  # (the tokens the cut completes: what the bookkeeping counts)
    for tail in (b"\0", b"\xff"):
        for k in range(1, 6):
            blob = s.blob + tail * k
            toks = lsw.read_tokens(blob)[0]
            st, out, used = _decodes(oracle, ref, s, blob)
            if not any(lsw.oob(tk, s.window) for tk in toks):
                assert st == 2 and len(out) == sum(tk.produced for tk in toks)


def test_group_cuts():
    for target, chain in ((lsw.GROUP_OUT, True), (lsw.SPLIT_MAX_OUT, False)):
        a, b = designed("group %d" % target), designed("group %d" % (target + 1))
        for s, twin in ((a, False), (b, True)):
            nb = s.numbers(chain=chain)
            k = s.props["cut_chunk"]
            assert sum(nb.table.outb[:k]) == target + twin
            g0 = nb.group_list[0]
            if not twin:
                assert g0.nout == target and nb.group_list[1].first_chunk == k  # the room used up to the byte
            else:
                assert g0.nout + nb.table.outb[k - 1] == target + 1 and nb.group_list[1].first_chunk == k - 1


def test_densest_chunks_unchained():
    s = designed("densest w15")
    nb = s.numbers(chain=False)
    assert {tk.produced for tk in s.tokens} == {15} and min(nb.table.outb[:-1]) >= 186 * 15
    assert nb.early == 3 and nb.scan_blocks == 0 and all(g.nout <= lsw.SPLIT_MAX_OUT for g in nb.group_list)
    assert [g.first_chunk for g in nb.group_list[:4]] == [0, 5, 10, 15]  # as small as the rule allows: five chunks of 2.8 KB


def test_lag_cap_streams():
    for name, window in (("lags 63 w10", 10), ("lags 63 w15", 15)):
        nb = designed(name).numbers()
        assert nb.table.nlag == [63] * 70 and nb.groups == 70 and nb.scan_blocks == 2
        assert [g.first_chunk for g in nb.group_list] == list(range(70)) and max(g.nout for g in nb.group_list) < 1 << window
    nb = designed("lags 64 in one chunk").numbers()
    assert nb.table.nlag == [63] * 35 + [64] + [63] * 34 and nb.max_lags == 64
    nb = designed("lags 20").numbers()
    assert nb.table.nlag == [20] * 70 and [g.first_chunk for g in nb.group_list] == list(range(0, 70, 3))
    assert all(g.nlag == 60 for g in nb.group_list[:-1])  # closed by the lag cap, not by room or records


@pytest.mark.parametrize("groups", [64, 65, 128, 129])
def test_scan_block_streams(groups):
    s = designed("groups %d" % groups)
    nb = s.numbers()
    assert nb.groups == groups and nb.scan_blocks == (groups + 63) // 64 and nb.max_lags == 63
    assert len(s.blob) <= 17 << 10
    copies = s.props["copies"]
    # 32,768 bytes of window and 504 bytes and more written per group: the window reaches back 60 groups, not 100
    assert {d for _, d in copies} == {3, 17, 60, "dictionary"}
    assert sum(1 for _, d in copies if d == 60) >= 3 and sum(1 for _, d in copies if d == "dictionary") >= 20
    # the sources lie in front of the group by construction: the chunk (= group) that wrote them is `d` chunks back and
    # fewer than W bytes have been written since
    starts = {}
    for tk in s.tokens:
        starts.setdefault(tk.bit // lsw.CHUNK_BITS_EXT, tk.wp)
    assert len(starts) >= groups


@pytest.mark.parametrize("window", [8, 10])
def test_window_pos_block_streams(window):
    s = designed("wp blocks w%d" % window)
    nb = s.numbers()
    W = 1 << window
    assert 4200 <= nb.entries < 4300 and nb.wp_blocks == 3 and nb.max_lags <= lsw.LAG_CAP
    # the list: per chunk its RLE / extended-match tokens, then a marker
    entries, chunk = [], 0
    for tk in s.tokens:
        while tk.bit // lsw.CHUNK_BITS_EXT > chunk:
            entries.append(None)
            chunk += 1
        if tk.kind in "RX":
            entries.append(tk)
    assert entries[2047] is None  # a chunk marker is the last entry of block 0
    for edge in (2048, 4096):
        near = [e.kind for e in entries[edge - 12 : edge + 12] if e is not None]
        assert {"R", "X"} <= set(near[: len(near) // 2]) and {"R", "X"} <= set(near[len(near) // 2 :])
    clipped = [tk for tk in s.tokens if tk.kind in "RX" and W - tk.wp < min(tk.produced, 8 if tk.kind == "R" else tk.produced)]
    assert len(clipped) >= 50
    assert any(tk.kind == "R" and tk.wp == W - 1 for tk in clipped) and any(tk.kind == "R" and tk.wp == W - 3 for tk in clipped)
    assert any(tk.kind == "X" and tk.wp == 0 for tk in s.tokens)
    assert any(tk.kind == "X" and tk.wp + tk.produced == W for tk in s.tokens)


def test_source_stream():
    s = designed("sources")
    nb = s.numbers()
    assert nb.max_lags == 63 and [g.first_chunk for g in nb.group_list[:3]] == [0, 1, 2]
    assert s.tokens[0].kind == "R"  # the stream's first token: its byte is the dictionary's
    i = next(i for i, tk in enumerate(s.tokens) if tk.bit >= 2 * lsw.CHUNK_BITS_EXT)
    assert s.tokens[i].kind == "R"  # a group's first token: its byte is external
    assert [tk.kind for tk in s.tokens[i + 63 : i + 73]] == list("LLLLLMMMMX")
    x = s.tokens[i + 72]
    assert x.produced == lsw.min_pattern(10, 8) + 131
    _source_matches(s.tokens, i + 68, s.tokens[i].wp)


def _source_matches(tokens, i, wp0):
    """tokens[i:i + 4]: the four matches of long_stream_writer._source_tokens; ``wp0`` = window_pos at the group's first token."""
    a, b, c, d = tokens[i : i + 4]
    assert a.off < wp0 < a.off + a.produced <= a.wp  # partly the window in front of the group, partly bytes the group has written
    assert b.off < b.wp < b.off + b.produced         # straddles the write cursor
    assert c.off + c.produced == c.wp                # the bytes just written
    assert d.off == d.wp - 1                         # the byte just written, and the one under the cursor


def test_source_stream_v1():
    s = designed("sources v1")
    nb = s.numbers()
    g1 = nb.group_list[1]
    assert g1.first_chunk == s.props["group_chunk"] and g1.v0 == s.props["v0"]
    i = next(i for i, tk in enumerate(s.tokens) if tk.bit >= g1.first_chunk * lsw.CHUNK_BITS_V1)
    assert [tk.kind for tk in s.tokens[i : i + 9]] == list("LLLLLMMMM") and 3 <= s.tokens[i].wp
    _source_matches(s.tokens, i + 5, s.tokens[i].wp)


@pytest.mark.parametrize("name", ["fresh v1", "fresh ext"])
def test_fresh_window_streams(oracle, ref, name):
    s = designed(name)
    assert len(s.dictionary) == 1 << 15 and s.blob[0] & 4
    for chain in (True, False) if not s.extended else (True,):
        nb = s.numbers(chain=chain)
        g1 = next(g for g in nb.group_list if g.v0 >= 31000)
        assert 31000 <= g1.v0 < 1 << 15 and g1.v0 == s.props["v0"]  # a group that starts inside the first W bytes, behind the literals
        assert nb.early == (2 if chain else 3)
    # tokens of that group whose source is a ring index that nothing has written: window_pos has not wrapped, the offset is ahead of it
    assert len(s.props["fresh"]) >= 8
    for i in s.props["fresh"]:
        assert sum(tk.written for tk in s.tokens[:i]) < 1 << 15 and s.tokens[i].kind in "MX"
    # without the dictionary argument the library's rule is TAMP_INVALID_CONF (the oracle restates it; the reference's C leaves
    # the window's contents to its caller), and the long-stream decoder says "declined: dictionary"
    assert oracle.decompress(s.blob, cap=s.produced + 64) == (-3, b"", 1)


def test_bad_offset_stream(oracle, ref):
    s = designed("bad offset")
    bad = [tk for tk in s.tokens if lsw.oob(tk, s.window)]
    assert len(bad) == 1 and bad[0].bit // lsw.CHUNK_BITS_V1 == 40 and s.numbers().oob
    st, out, used = _decodes(oracle, ref, s)
    assert st == -4 and len(out) == sum(tk.produced for tk in s.tokens[: s.tokens.index(bad[0])])
