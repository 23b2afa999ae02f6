"""CPU tier: every stream of tests/tight_decode_input.py against the property it was built for -- asserted from the token
writer's bookkeeping (bit positions, bytes produced and written, window_pos), never from decoded bytes -- and the sizes that decide
which build of a decoder tests/test_gpu_tight_decode.py reaches with it.  This file is the guarantee that the GPU cases aim where
they say."""
import pytest

import long_stream_writer as lsw
import tight_decode_input as tdi


def _overlap(tk):
    """Distance destination - source of a match whose source runs into its destination, else None."""
    d = tk.wp - tk.off if tk.off is not None else 0
    return d if 1 <= d <= tk.produced else None


def test_text_streams_sit_on_their_side_of_512_compressed_bytes(oracle):
    cases = tdi.cases(oracle)
    names = [n for n in cases if " text " in n]
    assert len(names) == 8
    for name in names:
        c = cases[name]
        st, x, used = oracle.decompress(c.blob, cap=c.props["plain"] + 8)
        assert (st, len(x), used) == (tdi.INPUT_EXHAUSTED, c.props["plain"], len(c.blob)), name
        assert c.blob[0] == lsw.header_byte(c.window, c.literal, c.extended)
        if c.props["kind"] == "short":
            assert len(x) == 300 and len(c.blob) < 512, (name, len(c.blob))  # lean builds, one-wavefront RESOLVE
        else:
            assert len(x) == 2560 > 2048 and 512 <= len(c.blob) <= 1100, (name, len(c.blob))  # bulk builds, workgroup RESOLVE
    assert {(cases[n].window, cases[n].literal, cases[n].extended) for n in names} == {(10, 8, True), (10, 8, False), (9, 5, False),
                                                                                      (15, 8, True)}


@pytest.mark.parametrize("name", list(tdi.DESIGNED))
def test_designed_stream_sizes_and_the_writer_against_the_checker(oracle, name):
    c = tdi.designed(name)
    n = tdi.n_out(c)
    if name == "short_tokens":
        assert len(c.blob) < 512 and n <= 2040, (len(c.blob), n)
    else:
        assert 560 <= len(c.blob) <= 800 and 2048 < n <= 4096, (len(c.blob), n)
    # the bookkeeping is the stream's: the checker produces as many bytes and ends as the design says
    st, x, used = oracle.decompress(c.blob, dictionary=c.dictionary, cap=n + 8)
    assert (st, len(x)) == (c.props["status"], n), (name, st, len(x), n)
    toks = lsw.read_tokens(c.blob)[0]
    if name == "cut":
        assert toks == c.tokens[:-1] and used == len(c.blob)  # (the bytes do not complete the last token)
    elif name != "reset":  # (read_tokens does not start window_pos over at a reset)
        assert toks[: len(c.tokens)] == c.tokens
    for tk in c.tokens:  # what a token writes to the window (decompressor.c:162-170, 266-268)
        room = (1 << c.window) - tk.wp
        assert tk.written == {"L": 1, "M": tk.produced, "F": 0, "R": min(tk.produced, 8, room), "X": min(tk.produced, room)}[tk.kind]


def test_configurations_across_the_designed_set():
    confs = {(c.literal, c.extended) for c in map(tdi.designed, tdi.DESIGNED)}
    assert {lit for lit, _ in confs} == {5, 8} and {ext for _, ext in confs} == {True, False}
    assert all(tdi.designed(n).window <= 10 for n in ("tokens", "short_tokens", "reset", "oob", "custom", "lag"))  # LDS rows
    assert tdi.designed("cut").window <= 12  # (four wavefronts per workgroup in the wave decoder)


@pytest.mark.parametrize("name", ["tokens", "short_tokens"])
def test_tokens_streams_hold_every_kind_overlap_count_and_phase(name):
    c = tdi.designed(name)
    W = 1 << c.window
    w = lsw.TokenWriter(c.window, c.literal, c.extended)
    assert {tk.kind for tk in c.tokens} == set("LMRXF")
    # matches whose source overlaps their destination: plain ones at every distance 1 .. length, extended ones at the listed ones
    seen = {(tk.kind, tk.produced, _overlap(tk)) for tk in c.tokens if tk.kind in "MX" and _overlap(tk)}
    assert c.props["overlaps"] <= seen
    for ln in c.props["plain_lengths"]:
        assert {d for k, n, d in c.props["overlaps"] if (k, n) == ("M", ln)} == set(range(1, ln + 1))
    assert {2, w.max_plain} <= set(c.props["plain_lengths"])
    for ln in c.props["ext_lengths"]:
        assert {1, ln} <= {d for k, n, d in c.props["overlaps"] if (k, n) == ("X", ln)}
    assert {w.minp + 12, w.max_ext} <= set(c.props["ext_lengths"])  # extended matches at minimum and maximum length
    # RLE counts, each at least once with room for its 8 window bytes
    assert set(tdi.RLE_COUNTS) <= {tk.produced for tk in c.tokens if tk.kind == "R" and tk.wp + 8 <= W}
    # tokens clipped at the end of the window: an RLE at W - 1, an extended match
    clipped = [tk for tk in c.tokens if tk.kind in "RX" and tk.wp + min(tk.produced, 8 if tk.kind == "R" else tk.produced) > W]
    assert all(tk.written == W - tk.wp < tk.produced for tk in clipped)
    assert {"R", "X"} <= {tk.kind for tk in clipped} and any(tk.kind == "R" and tk.wp == W - 1 for tk in clipped)
    # FLUSH at several bit phases; none directly behind another
    phases = {tk.bit % 8 for tk in c.tokens if tk.kind == "F"}
    assert phases == c.props["phases"] and len(phases) >= 3
    assert not any(a.kind == b.kind == "F" for a, b in zip(c.tokens, c.tokens[1:]))
    # the last token ends on a byte: exact room reports the end status, not TAMP_OUTPUT_FULL
    last = c.tokens[-1]
    assert (last.bit + last.nbits) % 8 == 0 and last.produced and len(c.blob) * 8 == last.bit + last.nbits


def test_lag_stream_crosses_the_limit_in_the_middle_third():
    c = tdi.designed("lag")
    starts, n = tdi.lag_starts(c), tdi.n_out(c)
    assert len(starts) >= 60
    assert n / 3 < starts[tdi.LAG_LIMIT] < 2 * n / 3  # the 49th lagging token
    assert not any(tk.kind == "F" for tk in c.tokens) and c.blob[0] & 1 == 0  # (nothing else hands the stream back)


def test_reset_stream_has_a_second_header_byte_and_three_resets():
    c = tdi.designed("reset")
    assert c.blob[0] & 1 and c.blob[1] == 0
    resets, n = tdi.reset_starts(c), tdi.n_out(c)
    assert len(resets) >= 2 and resets[0] >= n / 4 and resets[-1] < n
    for k, tk in enumerate(c.tokens):  # window_pos starts over behind every reset
        if tk.kind == "F" and k and c.tokens[k - 1].kind == "F" and k + 1 < len(c.tokens):
            assert c.tokens[k + 1].wp == 0


def test_oob_stream_runs_out_of_the_window_behind_its_output():
    c = tdi.designed("oob")
    bad = c.tokens[c.props["bad_token"]]
    assert lsw.oob(bad, c.window) and not any(lsw.oob(tk, c.window) for tk in c.tokens[: c.props["bad_token"]])
    assert sum(tk.produced for tk in c.tokens[: c.props["bad_token"]]) == c.props["n_out"]
    assert c.props["status"] == tdi.OOB and bad.bit + bad.nbits <= 8 * len(c.blob)
    assert c.props["n_out"] > 2048  # (behind ALL of the output: nothing is produced once the token has been met)


def test_cut_stream_ends_inside_its_last_token():
    c = tdi.designed("cut")
    last = c.tokens[-1]
    assert last.kind == "X" and last.bit < 8 * len(c.blob) < last.bit + last.nbits
    assert not any(lsw.oob(tk, c.window) for tk in c.tokens)


def test_custom_stream_reads_dictionary_bytes(oracle):
    c = tdi.designed("custom")
    assert c.blob[0] & 4 and len(c.dictionary) == 1 << c.window
    fresh = [tk for tk in c.tokens[: 2 * c.props["fresh"]] if tk.kind == "M"]
    assert len(fresh) == c.props["fresh"] >= 20 and all(tk.off >= tk.wp + tk.produced for tk in fresh)  # (no wrap yet: dictionary)
    st, x, _ = oracle.decompress(c.blob, dictionary=c.dictionary, cap=8192)
    other = oracle.decompress(c.blob, dictionary=bytes(1 << c.window), cap=8192)
    assert st == tdi.INPUT_EXHAUSTED and other[1] != x  # (the dictionary's bytes reach the output)
