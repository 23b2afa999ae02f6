"""CPU tier, build container only: differential check oracle <-> the reference C library itself.

Skipped wherever oracle/_ref/libtamp_ref.so was not built (it needs /root/reference at build
time).  Mirrors the reference's own differential pattern (fuzz/esp32_host/differential.cpp,
fuzz/fuzz_round_trip.c:14-90): random configuration, assert identical bytes and round trip.
"""
import random

from tamp_amd import workloads as wl


def _inputs(rng, n):
    kind = rng.randrange(5)
    if kind == 0:
        return wl.synth_text(1, n, first_index=rng.randrange(1 << 20))[0].tobytes()
    if kind == 1:
        return bytes(rng.randrange(256) for _ in range(n))
    if kind == 2:
        return wl.lcg_runs(1, n, first_index=rng.randrange(1 << 20))[0].tobytes()
    if kind == 3:
        return wl.stress(1, n, first_index=rng.randrange(1 << 20))[0].tobytes()
    return bytes([rng.randrange(256)]) * n


def test_differential_compress_decompress(oracle, ref):
    rng = random.Random(20260928)
    for it in range(1500):
        w, lit = rng.randrange(8, 16), rng.randrange(5, 9)
        ext, lazy = rng.random() < 0.6, rng.random() < 0.25
        n = rng.choice([0, 1, 2, 15, 16, 17, 33, 100, 256, 1000, 4096, rng.randrange(1, 6000)])
        data = _inputs(rng, n)
        if lit < 8 and rng.random() < 0.9:
            data = bytes(b & ((1 << lit) - 1) for b in data)
        d = None
        if rng.random() < 0.3:
            d = (_inputs(rng, 1 << w) + bytes(1 << w))[: 1 << w]
        kw = dict(window=w, literal=lit, extended=ext, dictionary=d, lazy_matching=lazy)
        a, b = oracle.compress(data, **kw), ref.compress(data, **kw)
        assert a == b, (it, w, lit, ext, lazy, n)
        if a[0] != 0:
            continue
        for cap in (n + 8, n, max(0, n - 1), n // 2):
            da = oracle.decompress(a[1], dictionary=d, cap=cap)
            db = ref.decompress(a[1], dictionary=d, cap=cap)
            assert da == db, (it, "decode", cap)
        assert oracle.decompress(a[1], dictionary=d, cap=n + 8)[1] == data
        if len(a[1]) > 2:
            bad = bytearray(a[1])
            for _ in range(2):
                bad[rng.randrange(1, len(bad))] ^= 1 << rng.randrange(8)
            bad = bytes(bad[: rng.randrange(2, len(bad) + 1)])
            assert oracle.decompress(bad, dictionary=d, cap=n + 300) == ref.decompress(bad, dictionary=d, cap=n + 300)


def test_compress_with_too_little_room_is_the_rule_and_the_reference_stays_inside_it(oracle, ref):
    """Every capacity 0..T+8 of every stream of tests/tight_output_input.cpu_inputs at windows 8/10/12/15 x literals 5..8 x both
    formats x lazy on/off.  The rule (include/tamp_amd.h; T and S from the REFERENCE's ample-room result): cap < T gives
    (OUTPUT_FULL, first cap bytes), otherwise (S, all T bytes).
      (a) the oracle is the rule, exactly;
      (b) the rule says OUTPUT_FULL => the reference says OUTPUT_FULL;
      (c) the reference's bytes are a prefix of the rule's;
      (d) the reference's status is the rule's or OUTPUT_FULL.
    Measured slack of the reference (INTEGRATION.md quotes the pair): `agree_from` = the smallest k with the reference equal to
    the rule at every cap >= T + k, `shortfall` = the most bytes it delivers fewer than min(cap, T).  Both at most 8: the
    reference holds back at most its 32-bit bit buffer and one further token of at most 32 bits.  Measured: 4 and 5."""
    import tight_output_input as toi
    from concurrent.futures import ThreadPoolExecutor

    jobs = [(dict(window=w, literal=lit, extended=ext, lazy_matching=lazy), x)
            for w in (8, 10, 12, 15) for lit in (5, 6, 7, 8) for ext in (True, False) for lazy in (False, True)
            for x in toi.cpu_inputs(lit)]

    def sweep(kw, x):
        status, full = ref.compress(x, **kw)
        assert status in (toi.OK, toi.EXCESS_BITS), (kw, len(x), status)
        T, agree_from, shortfall, statuses = len(full), 0, 0, set()
        for cap in range(T + 9):
            want = toi.rule(status, full, cap)
            got, r = oracle.compress(x, cap=cap, **kw), ref.compress(x, cap=cap, **kw)
            tag = (kw, len(x), status, T, cap)
            assert got == want, tag + ("oracle", got[0], len(got[1]))                           # (a)
            assert want[0] != toi.OUTPUT_FULL or r[0] == toi.OUTPUT_FULL, tag + ("ref", r[0])   # (b)
            assert want[1].startswith(r[1]), tag + ("ref bytes", len(r[1]))                     # (c)
            assert r[0] in (want[0], toi.OUTPUT_FULL), tag + ("ref", r[0])                      # (d)
            if r != want and cap >= T:
                agree_from = cap - T + 1
            shortfall = max(shortfall, min(cap, T) - len(r[1]))
            statuses.add(want[0])
        return agree_from, shortfall, statuses, status, T

    with ThreadPoolExecutor(16) as ex:  # (both libraries' calls release the GIL)
        results = list(ex.map(lambda j: sweep(*j), jobs))
    agree_from, shortfall = max(r[0] for r in results), max(r[1] for r in results)
    print(f"reference vs rule over {sum(r[4] + 9 for r in results)} cases: agrees from T + {agree_from}, "
          f"delivers up to {shortfall} bytes fewer")
    assert set().union(*(r[2] for r in results)) == {toi.OK, toi.OUTPUT_FULL, toi.EXCESS_BITS}
    assert sum(r[3] == toi.EXCESS_BITS and r[4] > 1 for r in results) >= 100  # (streams that fail behind some output)
    assert agree_from <= 8 and shortfall <= 8, (agree_from, shortfall)


def test_decode_with_too_little_room_is_the_rule_at_every_capacity(oracle, ref):
    """Every stream of tests/tight_decode_input.py at every capacity 0..N+8 (N = its output with ample room): the oracle and the
    reference agree on (status, bytes, consumed), the result obeys tight_decode_input.rule -- cap < N: (OUTPUT_FULL, X[:cap]);
    cap > N: the ample-room result; cap == N: all of X with the end status or OUTPUT_FULL -- and the consumed count never
    decreases as the capacity grows.  tests/test_gpu_tight_decode.py expects the oracle's result of every decoder, capacity by
    capacity; this test pins that expectation to the reference."""
    import tight_decode_input as tdi
    from concurrent.futures import ThreadPoolExecutor

    def sweep(c):
        full = ref.decompress(c.blob, dictionary=c.dictionary, cap=1 << 16)
        N = len(full[1])
        statuses, exact, last = set(), None, 0
        for cap in range(N + 9):
            got = oracle.decompress(c.blob, dictionary=c.dictionary, cap=cap)
            r = ref.decompress(c.blob, dictionary=c.dictionary, cap=cap)
            tag = (c.name, cap, N)
            assert got == r, tag + (got[0], r[0], len(got[1]), len(r[1]), got[2], r[2])
            assert tdi.obeys(full, cap, got), tag + (got[0], len(got[1]), got[2])
            assert got[2] >= last, tag + ("consumed", got[2], last)
            last = got[2]
            statuses.add(got[0])
            if cap == N:
                exact = got[0] == full[0]
        return N + 9, statuses, exact

    with ThreadPoolExecutor(16) as ex:  # (both libraries' calls release the GIL)
        results = list(ex.map(sweep, tdi.cases(oracle).values()))
    print(f"decode, oracle vs reference vs rule: {sum(r[0] for r in results)} (stream, capacity) pairs over {len(results)} streams")
    assert set().union(*(r[1] for r in results)) >= {tdi.OUTPUT_FULL, tdi.INPUT_EXHAUSTED, tdi.OOB}
    assert {r[2] for r in results} == {True, False}  # exact room: the end status on some streams, OUTPUT_FULL on others


def test_struct_sizes(ref):
    # sizeof(TampConf)=2, TampCompressor=48, TampDecompressor=24 on x86-64
    assert ref.sizes() == (2, 48, 24)
