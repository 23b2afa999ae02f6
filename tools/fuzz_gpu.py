"""Randomised differential run on the GPU box: compress (all modes) and decompress (both decoders) against the oracle.
   usage: python tools/fuzz_gpu.py [seconds]   -- prints a summary line; exits 1 on the first mismatch.
          python tools/fuzz_gpu.py [seconds] index   -- random token streams with resets through tamp_amd.index_resets against the
                                                        CPU token reader (tests/long_stream_writer.py) instead.
          python tools/fuzz_gpu.py [seconds] write   -- random batches compressed with resets, random disjoint writes through
                                                        tamp_amd.write_ranges against a fresh compress of the patched data.
          python tools/fuzz_gpu.py [seconds] append  -- random batches compressed with resets, random chains of appends through
                                                        tamp_amd.append_batch against a fresh compress of old + appended."""
import os, random, sys, time
sys.path.insert(0, os.environ.get('GRAFT_REPO_ROOT', '/root/repo'))
import numpy as np
import tamp_amd
from tamp_amd import workloads as wl
from oracle.checker import Oracle

o = Oracle()
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = random.Random(int(os.environ.get('FUZZ_SEED', '1')))
t0 = time.time()
rounds = streams = 0


def index_mode():
    """Batches of random token streams (every window, literal width and format; resets spliced in; some cut anywhere) ->
    offsets, closed and open sizes and status of index_resets against read_tokens."""
    global rounds, streams
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tests'))
    from long_stream_writer import TokenWriter, mixed, oob, read_tokens

    def truth(blob):
        if len(blob) < 2:
            return 2, [], [], 0
        toks, window = read_tokens(blob)[:2]
        offs, closed, seg, prev = [], [], 0, False
        for tk in toks:
            flush = tk.kind == 'F'
            if flush and prev:
                offs.append((tk.bit + tk.nbits) >> 3), closed.append(seg)
                seg = 0
            seg, prev = seg + tk.produced, flush
        return (-4 if any(oob(tk, window) for tk in toks) else 0), offs, closed, seg

    while time.time() - t0 < budget:
        blobs = []
        for _ in range(rng.choice([1, 5, 70, 300])):
            w = TokenWriter(rng.randrange(8, 16), rng.randrange(5, 9), rng.random() < 0.5, more=0)
            end = w.bit + rng.choice([0, 50, 900, 1100, 5000, 70000, 140000])
            while w.bit < end:
                mixed(w, rng, min(end, w.bit + rng.randrange(1, 3000)))
                for _ in range(rng.choice([0, 1, 2, 2, 3, 50])):
                    w.flush()
                if rng.random() < 0.02:
                    w.match(w.W - 1, w.minp, check=False)
            blob = w.blob()
            blobs.append(blob[: rng.randrange(len(blob) + 1)] if rng.random() < 0.2 else blob)
        scan = tamp_amd.index_resets(blobs)
        for i, blob in enumerate(blobs):
            a, b = int(scan.index.first[i]), int(scan.index.first[i + 1])
            got = (int(scan.status[i]), scan.index.off[a:b].tolist(), scan.closed_size[a:b].tolist(), int(scan.open_size[i]))
            if got != truth(blob):
                print('INDEX MISMATCH', i, len(blob), blob[:1].hex(), got[0], truth(blob)[0], len(got[1]), len(truth(blob)[1]))
                open('fuzz_index_fail.bin', 'wb').write(blob)  # (the stream that differs, into the working directory)
                sys.exit(1)
        rounds += 1
        streams += len(blobs)
    print(f"index fuzz ok: {rounds} rounds, {streams} streams, {time.time() - t0:.0f} s")
    sys.exit(0)


def write_mode():
    """Random batches (every window, literal width and format, lazy or not, any interval), random disjoint writes in random order,
    host and device memory -> streams, index and status of write_ranges against compress_batch of the patched data."""
    global rounds, streams
    import torch

    while time.time() - t0 < budget:
        window, literal, ext, lazy = rng.randrange(8, 16), rng.randrange(5, 9), rng.random() < 0.5, rng.random() < 0.3
        N = rng.choice([1, 7, 16, 100, 256, 1000, 4096])
        n = rng.choice([1, 5, 70, 300])
        top = (1 << literal) - 1
        datas = []
        for _ in range(n):
            L = rng.choice([0, 1, N, N + 1, 3 * N, rng.randrange(0, 6000)])
            style = rng.randrange(3)
            if style == 0:
                datas.append(bytes(rng.randrange(top + 1) for _ in range(L)))
            elif style == 1:
                datas.append(bytes((wl.synth_text(1, max(L, 1), first_index=rng.randrange(1000))[0][:L]) & top))
            else:
                datas.append((bytes([rng.randrange(top + 1)]) * rng.randrange(1, 300) * (L // 2 + 1))[:L])
        kw = dict(window=window, literal=literal, extended=ext, lazy_matching=lazy)
        base = tamp_amd.compress_batch(datas, dictionary_reset=True, reset_interval=N, reset_index=True, **kw)
        if (base.status != 0).any():  # (random bytes of a narrow literal width can outgrow the default slab: not this call's business)
            continue
        writes, patched = [], [bytearray(d) for d in datas]
        for i, d in enumerate(datas):
            pos = 0
            while rng.random() < 0.7:
                pos += rng.randrange(0, 4 * N + 2)
                ln = rng.randrange(0, 3 * N + 2)
                if pos + ln > len(d):
                    break
                src = bytes(rng.randrange(top + 1) for _ in range(ln))
                writes.append((i, pos, src))
                patched[i][pos : pos + ln] = src
                pos += ln
        rng.shuffle(writes)
        want = tamp_amd.compress_batch([bytes(b) for b in patched], dictionary_reset=True, reset_interval=N, reset_index=True, **kw)
        tables = dict(reset_index=base.reset_index, stream_index=[w[0] for w in writes], begin=[w[1] for w in writes], source=[w[2] for w in writes],
                      lazy_matching=lazy)
        host = rng.random() < 0.5
        if host:
            res = tamp_amd.write_ranges(base.streams(), **tables)
        else:
            dev = torch.device('cuda:0')
            flat, off, ln = tamp_amd.pack_streams(base.streams())
            t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev).to(dt)
            res = tamp_amd.write_ranges(torch.from_numpy(np.concatenate([flat, np.zeros(1, np.uint8)])).to(dev), t(off, torch.int64), t(ln, torch.int32),
                                        window=window, literal=literal, extended=ext, **tables)
            torch.cuda.synchronize()
        status = np.asarray(res.status.cpu() if hasattr(res.status, 'cpu') else res.status)
        got_off = np.asarray(res.reset_index.off.cpu() if hasattr(res.reset_index.off, 'cpu') else res.reset_index.off).astype(np.uint32)
        # (a patched segment that outgrows its slab fails both ways alike: the status is compared, not asked to be 0)
        ok = np.asarray(want.status) == 0
        firsts = np.asarray(want.reset_index.first).astype(np.int64)
        same_index = all((got_off[firsts[i] : firsts[i + 1]] == want.reset_index.off[firsts[i] : firsts[i + 1]]).all() for i in np.flatnonzero(ok))
        if (status != want.status).any() or res.streams() != want.streams() or not same_index:
            bad = [i for i in range(n) if status[i] != want.status[i] or res.stream(i) != want.stream(i)] or ['index']
            print('WRITE MISMATCH', 'host' if host else 'device', window, literal, ext, lazy, N, n, len(writes), bad[:8], [int(status[i]) for i in bad[:8]])
            for i in bad[:3]:  # per stream: decoded bytes, old and wanted compressed bytes, its room, its writes
                print('  stream', i, len(datas[i]), len(base.stream(i)), len(want.stream(i)), int(want.status[i]), int(res._keep[-1][i]) if not host else '-',
                      sorted((w[1], len(w[2])) for w in writes if w[0] == i))
            sys.exit(1)
        rounds += 1
        streams += n
    print(f"write fuzz ok: {rounds} rounds, {streams} streams, {time.time() - t0:.0f} s")
    sys.exit(0)


def append_mode():
    """Random batches (every window, literal width and format, lazy or not, any interval), chains of one to four appends of random
    lengths around the open segment's room, host memory or device memory (there each call on the previous result's slabs and index as
    they stand) -> streams, index and status of append_batch after every link against compress_batch of old + appended."""
    global rounds, streams
    import torch

    def piece(L, top):
        style = rng.randrange(3)
        if style == 0:
            return bytes(rng.randrange(top + 1) for _ in range(L))
        if style == 1:
            return bytes((wl.synth_text(1, max(L, 1), first_index=rng.randrange(1000))[0][:L]) & top)
        return (bytes([rng.randrange(top + 1)]) * rng.randrange(1, 300) * (L // 2 + 1))[:L]

    links = 0
    while time.time() - t0 < budget:
        window, literal, ext, lazy = rng.randrange(8, 16), rng.randrange(5, 9), rng.random() < 0.5, rng.random() < 0.3
        N = rng.choice([1, 7, 16, 100, 256, 1000, 4096])
        n = rng.choice([1, 5, 70, 300])
        top = (1 << literal) - 1
        datas = [piece(rng.choice([0, 1, N, N + 1, 3 * N, rng.randrange(0, 6000)]), top) for _ in range(n)]
        kw = dict(window=window, literal=literal, extended=ext, lazy_matching=lazy)
        base = tamp_amd.compress_batch(datas, dictionary_reset=True, reset_interval=N, reset_index=True, **kw)
        if (base.status != 0).any():  # (random bytes of a narrow literal width can outgrow the default slab: not this call's business)
            continue
        host = rng.random() < 0.5
        index = base.reset_index
        if host:
            args = (base.streams(),)
        else:
            dev = torch.device('cuda:0')
            flat, off, ln = tamp_amd.pack_streams(base.streams())
            t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev).to(dt)
            args = (torch.from_numpy(np.concatenate([flat, np.zeros(1, np.uint8)])).to(dev), t(off, torch.int64), t(ln, torch.int32))
        for _ in range(rng.randrange(1, 5)):
            srcs = []
            for d in datas:
                m = len(d) - (max(1, -(-len(d) // N)) - 1) * N
                L = rng.choice([0, 0, 1, max(N - m - 1, 0), N - m, N - m + 1, N, 3 * N + 1, rng.randrange(0, 3 * N + 2)])
                srcs.append(piece(L, top) if rng.random() < 0.8 else None)
            datas = [d + (s or b'') for d, s in zip(datas, srcs)]
            want = tamp_amd.compress_batch(datas, dictionary_reset=True, reset_interval=N, reset_index=True, **kw)
            if (want.status != 0).any():
                break
            if host:
                res = tamp_amd.append_batch(*args, reset_index=index, source=srcs, lazy_matching=lazy)
                args, index = (res.streams(),), res.reset_index
            else:
                res = tamp_amd.append_batch(*args, reset_index=index, source=srcs, **kw)
                torch.cuda.synchronize()
                args, index = (res.out, res.out_off, res.out_len), res.reset_index
            as_np = lambda x: np.asarray(x.cpu() if hasattr(x, 'cpu') else x)
            status, got_first = as_np(res.status), as_np(index.first).astype(np.uint64)
            entries = int(want.reset_index.first[-1])
            got_off = as_np(index.off).view(np.uint32)[:entries]
            if (status != 0).any() or res.streams() != want.streams() or (got_first != want.reset_index.first).any() or (got_off != want.reset_index.off).any():
                bad = [i for i in range(n) if status[i] != 0 or res.stream(i) != want.stream(i)] or ['index']
                print('APPEND MISMATCH', 'host' if host else 'device', window, literal, ext, lazy, N, n, bad[:8], [int(status[i]) for i in bad[:8] if i != 'index'])
                for i in [b for b in bad[:3] if b != 'index']:
                    print('  stream', i, 'old + new bytes', len(datas[i]), 'appended', len(srcs[i] or b''), 'got', len(res.stream(i)), 'want', len(want.stream(i)))
                sys.exit(1)
            links += 1
        rounds += 1
        streams += n
    print(f"append fuzz ok: {rounds} rounds, {links} appends, {streams} streams, {time.time() - t0:.0f} s")
    sys.exit(0)


if len(sys.argv) > 2 and sys.argv[2] == 'index':
    index_mode()
if len(sys.argv) > 2 and sys.argv[2] == 'append':
    append_mode()
if len(sys.argv) > 2 and sys.argv[2] == 'write':
    write_mode()
gens = [lambda n, L, k: wl.synth_text(n, L, first_index=k), lambda n, L, k: wl.lcg_runs(n, L, first_index=k),
        lambda n, L, k: wl.stress(n, L, first_index=k), lambda n, L, k: wl.telemetry(n, L, first_index=k),
        lambda n, L, k: np.random.default_rng(k).integers(0, 256, (n, L), dtype=np.uint8),
        lambda n, L, k: (np.random.default_rng(k).integers(0, 4, (n, L), dtype=np.uint8) * 37 + 65).astype(np.uint8),
        lambda n, L, k: np.repeat(np.random.default_rng(k).integers(0, 256, (n, (L + 6) // 7), dtype=np.uint8), 7, axis=1)[:, :L].copy()]
def long_repeats(n, L, k):
    # text-like bytes with long back-references (20-300 bytes copied from up to 1200 bytes back): long extended matches
    r = np.random.default_rng(k)
    rows = np.empty((n, L), dtype=np.uint8)
    for i in range(n):
        buf = bytearray(r.integers(97, 97 + int(r.integers(2, 20)), min(L, 64), dtype=np.uint8).tobytes())
        while len(buf) < L:
            if r.random() < 0.6 and len(buf) > 30:
                d = int(r.integers(1, min(len(buf), 1200) + 1)); m = int(r.integers(14, 300))
                for _ in range(m): buf.append(buf[-d])
            else:
                buf += r.integers(97, 123, int(r.integers(1, 12)), dtype=np.uint8).tobytes()
        rows[i] = np.frombuffer(bytes(buf[:L]), dtype=np.uint8)
    return rows
gens.append(long_repeats)
gens.append(long_repeats)
while time.time() - t0 < budget:
    n = rng.choice([1, 3, 64, 200, 700])
    L = rng.choice([1, 2, 17, 100, 333, 1024, 3000, 4096, 9000])
    window = rng.choice([8, 9, 10, 10, 10, 11, 12, 13, 14, 15])
    literal = rng.choice([8, 8, 7, 6, 5])
    ext = rng.random() < 0.6
    lazy = rng.random() < 0.3
    rows = rng.choice(gens)(n, L, rng.randrange(1 << 20))
    if literal < 8:
        rows = rows & np.uint8((1 << literal) - 1)
    d = None
    if rng.random() < 0.25:
        d = np.random.default_rng(rng.randrange(1 << 20)).integers(0, 1 << min(literal, 7), 1 << window, dtype=np.uint8).tobytes()
    kw = dict(window=window, literal=literal, extended=ext, lazy_matching=lazy, dictionary=d)
    flat = np.ascontiguousarray(rows).reshape(-1)
    off, ln = wl.csr_for_fixed(n, L)
    got = tamp_amd.compress_batch(flat, off, ln, max_in_len=L, run_aware=rng.choice([None, False, True, True]), **kw)
    want = o.compress_batch(flat, off, ln, threads=16, **{('lazy' if k == 'lazy_matching' else k): v for k, v in kw.items()})
    comp = []
    for i in range(n):
        a, b = got.stream(i), want.stream(i)
        if int(got.status[i]) != int(want.status[i]) or a != b:
            print('COMPRESS MISMATCH', kw if d is None else {**kw, 'dictionary': 'custom'}, n, L, i, int(got.status[i]), int(want.status[i]), len(a), len(b))
            outdir = os.path.join(os.environ.get('GRAFT_REPO_ROOT', '/root/repo'), 'gpurun_out')
            os.makedirs(outdir, exist_ok=True)
            np.save(os.path.join(outdir, 'fuzz_fail_input.npy'), np.asarray(rows[i]))
            open(os.path.join(outdir, 'fuzz_fail_got.bin'), 'wb').write(a)
            open(os.path.join(outdir, 'fuzz_fail_want.bin'), 'wb').write(b)
            if d is not None: open(os.path.join(outdir, 'fuzz_fail_dict.bin'), 'wb').write(d)
            sys.exit(1)
        comp.append(b)
    cap = rng.choice([L + 8, L, max(1, L // 2), L + 300])
    trunc = rng.random() < 0.3
    if trunc:
        comp = [c[: rng.randrange(0, len(c) + 1)] for c in comp]
    for mode in ('wave', 'lane', 'global', 'split'):
        os.environ['TAMP_AMD_DECODER'] = mode
        res = tamp_amd.decompress_batch(comp, out_cap=cap, dictionary=d, max_window_bits=rng.choice([window, 15]))
        for i in range(n):
            st, out, cons = o.decompress(comp[i], dictionary=d, cap=cap, max_window_bits=15)
            if (int(res.status[i]), res.stream(i), int(res.in_consumed[i])) != (st, out, cons):
                print('DECOMPRESS MISMATCH', mode, window, literal, ext, n, L, i, cap, trunc, int(res.status[i]), st, int(res.out_len[i]), len(out), int(res.in_consumed[i]), cons)
                sys.exit(1)
    del os.environ['TAMP_AMD_DECODER']
    rounds += 1
    streams += n
print(f"fuzz ok: {rounds} rounds, {streams} streams, {time.time() - t0:.0f} s")
