"""GPU tier: a batch's streams packed densely on the device (tamp_batch_pack, the kernels of tamp_pack_kernel.hpp)
through ``pack_batch`` / ``BatchResult.packed``.

The model is ``pack_batch`` on numpy arrays (tests/test_pack_host.py checks it against a three-line loop).  Sources are filled with
0xA5 between their streams; the destination is a view into a larger tensor pre-filled with 0x5A, GUARD bytes in front of it and as
many behind, so that a byte written outside the packed bytes shows on either side.  T is the copy's tile (kPackTile), S the scan's
(TAMP_AMD_RESETS_SCAN_TILE).  Comparisons run on the device and come back as one flag per call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, S = 16384, 1024
GUARD = 256
EDGE_LENS = list(range(0, 71)) + [255, 256, 257, 4095, 4096, 4097, T - 1, T, T + 1, 3 * T + 5]
ALIGNS = (1, 2, 16, 256)


@pytest.fixture(scope="module")
def ta():
    import tamp_amd
    from tamp_amd import _lib

    _lib.load()  # raises if the native library is missing: no silent fallback
    return tamp_amd


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def source(streams, starts, size):
    """The streams at ``starts`` in a buffer of ``size`` bytes that holds 0xA5 wherever no stream lies."""
    data = np.full(size, 0xA5, dtype=np.uint8)
    for s, at in zip(streams, starts):
        data[at : at + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return data


def random_streams(lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]


def to_device(dev, data, off, length):
    import torch

    return (torch.from_numpy(np.array(data, dtype=np.uint8)).to(dev), torch.from_numpy(np.array(off, dtype=np.int64)).to(dev),
            torch.from_numpy(np.asarray(length, dtype=np.uint32).view(np.int32).copy()).to(dev))


class Guarded:
    """A destination of ``cap`` bytes at ``residue`` mod 16 (the allocation is 256-byte aligned) between two guards of 0x5A."""

    def __init__(self, dev, cap, residue=0):
        import torch

        self.big = torch.full((GUARD + 16 + cap + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
        assert self.big.data_ptr() % 256 == 0
        self.lo, self.cap = GUARD + residue, cap
        self.out = self.big[self.lo : self.lo + cap]

    def guards_intact(self, written):
        """A device flag: every byte in front of the view and from ``written`` bytes into it on is still 0x5A."""
        return (self.big[: self.lo] == 0x5A).all() & (self.big[self.lo + written :] == 0x5A).all()


def check(ta, dev, data, off, length, align, *, residue=0, stream=None):
    """One packed call into an exactly sized guarded view, against the numpy model; -> the result."""
    import torch

    want = ta.pack_batch(data, off, length, align=align)
    d = to_device(dev, data, off, length)
    g = Guarded(dev, len(want.data), residue)
    p = ta.pack_batch(*d, align=align, out=g.out, stream=stream)
    torch.cuda.synchronize()
    assert p.off.cpu().numpy().astype(np.uint64).tolist() == want.off.tolist()
    assert bytes(g.out.cpu().numpy()) == want.data.tobytes()
    assert bool(g.guards_intact(len(want.data)))
    assert p.streams() == want.streams() and p.len.cpu().numpy().view(np.uint32).tolist() == want.len.tolist()
    return p


@pytest.fixture(scope="module")
def edges(ta, dev):
    """The edge batch: its streams, the numpy model per alignment (computed once), and its sources on the device -- ``literal[k]``
    the slabs back to back with capacities len + k, ``at[r]`` every slab starting at residue r mod 16."""
    import torch

    streams = random_streams(EDGE_LENS, 7)
    lens = np.array(EDGE_LENS, dtype=np.uint32)
    flat, off, _ = ta.pack_streams(streams)
    want = {}
    for align in ALIGNS:
        w = ta.pack_batch(flat, off, lens, align=align)
        want[align] = (torch.from_numpy(w.data).to(dev), torch.from_numpy(w.off.astype(np.int64)).to(dev), len(w.data))
    literal, at = [], []
    for k in range(16):
        caps = lens.astype(np.int64) + k
        starts = np.cumsum(caps) - caps
        literal.append(to_device(dev, source(streams, starts, int(caps.sum()) + 1), starts, lens))
        slots = (lens.astype(np.int64) + 15 + 16) // 16 * 16  # a 16-byte slot grid with a gap behind every stream
        starts = np.cumsum(slots) - slots + k
        at.append(to_device(dev, source(streams, starts, int(slots.sum()) + 16), starts, lens))
    assert all(d[0].data_ptr() % 256 == 0 for d in literal + at)
    assert {int(s) % 16 for s in literal[1][1].tolist()} == set(range(16))  # (capacities len + 1 alone reach every residue)
    return want, literal, at


@pytest.mark.parametrize("align", ALIGNS)
def test_edges_at_every_source_and_destination_residue(ta, dev, edges, align):
    """One stream per length in {0..70, 255..257, 4095..4097, T-1, T, T+1, 3T+5}; the source slabs at every residue mod 16 (both
    layouts of the fixture), the destination view at every residue mod 16: bytes, zero padding, offsets and both guards."""
    import torch

    want, literal, at = edges
    w_data, w_off, total = want[align]
    flags, calls = [], []
    for layout, sources in (("len+k", literal), ("residue", at)):
        for k, d in enumerate(sources):
            for residue in range(16):
                g = Guarded(dev, total, residue)
                assert g.out.data_ptr() % 16 == residue
                p = ta.pack_batch(*d, align=align, out=g.out)
                flags.append(torch.equal(p.off, w_off) & torch.equal(g.out, w_data) & g.guards_intact(total))
                calls.append((layout, k, residue))
    failed = [c for c, ok in zip(calls, torch.stack([torch.as_tensor(f, device=dev) for f in flags]).cpu().tolist()) if not ok]
    assert not failed, failed[:10]
    assert len(calls) == 2 * 16 * 16


def test_permuted_gapped_and_shared_sources(ta, dev):
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 300, 300).astype(np.uint32)
    streams = random_streams(lens, 12)
    caps = lens.astype(np.int64) + rng.integers(0, 40, len(lens))
    starts = np.cumsum(caps) - caps
    data = source(streams, starts, int(caps.sum()) + 5)
    order = rng.permutation(len(lens))
    for align in (1, 16):
        check(ta, dev, data, starts[order], lens[order], align, residue=3)
    # two streams reading the same source bytes, and one that overlaps them
    off = np.array([starts[40], starts[7], starts[40], starts[40] + 1], dtype=np.int64)
    length = np.array([lens[40], lens[7], lens[40], max(int(lens[40]), 1) - 1], dtype=np.uint32)
    p = check(ta, dev, data, off, length, 4)
    assert p.stream(0) == p.stream(2) == streams[40]


@pytest.mark.parametrize("n", [1, 255, 256, 257, S - 1, S, S + 1, 2 * S + 1, S * S + 1])
def test_scan_levels(ta, dev, n):
    """Stream counts around the scan's step (S streams per step of a workgroup, one range of steps per workgroup, at most S ranges):
    above S * S streams a workgroup takes more than one step and the sums of S ranges are scanned."""
    import torch

    rng = np.random.default_rng(n)
    lens = rng.integers(0, 41, n).astype(np.uint32)
    off = np.cumsum(lens.astype(np.int64)) - lens
    data = rng.integers(0, 256, int(lens.sum()) + 1, dtype=np.uint8)
    want = ta.pack_batch(data, off, lens, align=2)
    g = Guarded(dev, len(want.data), 5)
    p = ta.pack_batch(*to_device(dev, data, off, lens), align=2, out=g.out)
    ok = torch.equal(p.off, torch.from_numpy(want.off.astype(np.int64)).to(dev)) & torch.equal(g.out, torch.from_numpy(want.data).to(dev))
    assert bool(ok) and bool(g.guards_intact(len(want.data)))
    assert int(p.off[-1]) == int(want.off[-1]) == len(want.data)


def test_one_long_stream_among_a_thousand_short_ones(ta, dev):
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 41, 1001).astype(np.uint32)
    lens[500] = 3 * T + 5
    streams = random_streams(lens, 6)
    flat, off, _ = ta.pack_streams(streams)
    for align, residue in ((1, 0), (1, 9), (16, 0), (4096, 1)):
        check(ta, dev, np.concatenate([flat, np.full(3, 0xA5, np.uint8)]), off, lens, align, residue=residue)


def test_capacity_decides_before_any_store(ta, dev):
    import torch

    lens = np.array([5, 0, T + 3, 17, 4000], dtype=np.uint32)
    streams = random_streams(lens, 3)
    flat, off, _ = ta.pack_streams(streams)
    want = ta.pack_batch(flat, off, lens, align=16)
    total = len(want.data)
    d = to_device(dev, flat, off, lens)
    w_off = torch.from_numpy(want.off.astype(np.int64)).to(dev)
    for residue in (0, 7):
        # one byte short: the offsets are written, the destination is untouched, every guard is intact
        g = Guarded(dev, total - 1, residue)
        p = ta.pack_batch(*d, align=16, out=g.out)
        assert torch.equal(p.off, w_off) and int(p.off[-1]) == total > g.out.numel()
        assert bool((g.big == 0x5A).all())
        # exactly enough
        g = Guarded(dev, total, residue)
        p = ta.pack_batch(*d, align=16, out=g.out)
        assert torch.equal(p.off, w_off) and bytes(g.out.cpu().numpy()) == want.data.tobytes() and bool(g.guards_intact(total))
        # more than enough: nothing at or behind the packed bytes is written
        g = Guarded(dev, total + 100, residue)
        p = ta.pack_batch(*d, align=16, out=g.out)
        assert bytes(g.out[:total].cpu().numpy()) == want.data.tobytes() and bool(g.guards_intact(total))
    # dst = NULL, dst_cap = 0: the offsets only
    p = ta.pack_batch(*d, align=16, out=torch.empty(0, dtype=torch.uint8, device=dev))
    assert torch.equal(p.off, w_off) and p.data.numel() == 0
    # ... and without out= the two calls allocate exactly the packed size
    p = ta.pack_batch(*d, align=16)
    assert p.data.numel() == total and p.streams() == streams and torch.equal(p.off, w_off)


def test_no_streams_and_empty_streams(ta, dev):
    import torch

    none = to_device(dev, np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.uint32))
    for out in (None, Guarded(dev, 64, 3).out):
        p = ta.pack_batch(*none, out=out)
        assert p.off.cpu().tolist() == [0] and p.streams() == [] and p.len.numel() == 0
        assert out is None or bool((out == 0x5A).all())
    for data in (np.zeros(0, np.uint8), np.full(40, 0xA5, np.uint8)):
        empties = to_device(dev, data, np.array([0, 0, len(data), 0, 0], np.int64), np.zeros(5, np.uint32))
        for align in (1, 4096):
            g = Guarded(dev, 32, 1)
            p = ta.pack_batch(*empties, align=align, out=g.out)
            assert p.off.cpu().tolist() == [0] * 6 and p.streams() == [b""] * 5 and bool((g.big == 0x5A).all())
            assert ta.pack_batch(*empties, align=align).data.numel() == 0


def test_on_a_stream_of_the_callers(ta, dev):
    import torch

    rng = np.random.default_rng(21)
    lens = rng.integers(0, 9000, 200).astype(np.uint32)
    streams = random_streams(lens, 22)
    flat, off, _ = ta.pack_streams(streams)
    want = ta.pack_batch(flat, off, lens, align=16)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        d = to_device(dev, flat, off, lens)
        g = Guarded(dev, len(want.data), 2)
    side.synchronize()
    for out in (g.out, None):
        p = ta.pack_batch(*d, align=16, out=out, stream=side.cuda_stream)
        side.synchronize()
        assert p.off.cpu().numpy().astype(np.uint64).tolist() == want.off.tolist()
        assert bytes(p.data.cpu().numpy()) == want.data.tobytes() and p.streams() == streams
    assert bool(g.guards_intact(len(want.data)))


@pytest.fixture(scope="module")
def compressed(ta, dev):
    """300 streams of 0..5,000 bytes of synthetic text and one of 300 KB, compressed on the device into worst-case slabs."""
    import torch
    from tamp_amd import workloads as wl

    rng = np.random.default_rng(31)
    text = wl.synth_text(1, 400 * 1024).reshape(-1)
    lens = np.append(rng.integers(0, 5001, 300), 300 * 1024).astype(np.uint32)
    starts = rng.integers(0, len(text) - 300 * 1024, len(lens))
    inputs = [text[s : s + n].tobytes() for s, n in zip(starts, lens)]
    flat, off, _ = ta.pack_streams(inputs)
    res = ta.compress_batch(*to_device(dev, flat if flat.size else np.zeros(1, np.uint8), off, lens))
    torch.cuda.synchronize()
    assert (res.status.cpu().numpy() == 0).all()
    return inputs, lens, res


@pytest.mark.parametrize("how", ["packed", "align16", "out"])
def test_compress_pack_decompress(ta, dev, compressed, how):
    import torch

    inputs, lens, res = compressed
    if how == "out":
        room = torch.full((int(res.out.numel()),), 0x5A, dtype=torch.uint8, device=dev)
        p = res.packed(out=room)
        assert p.data is room and int(p.off[-1]) <= room.numel() and bool((room[int(p.off[-1]) :] == 0x5A).all())
    else:
        p = res.packed(align=16) if how == "align16" else res.packed()
        assert p.data.numel() == int(p.off[-1])
    assert int(p.off[-1]) < res.out.numel() * 0.75  # (the point of the call: far less than the slabs)
    out_off, out_len = res.out_off.cpu().tolist(), res.out_len.cpu().tolist()
    slabs = res.out.cpu().numpy().tobytes()
    assert p.streams() == [slabs[o : o + n] for o, n in zip(out_off, out_len)]
    for i in (0, 1, 150, 299, 300):
        assert p.stream(i) == res.stream(i)
    if how == "align16":
        assert all(o % 16 == 0 for o in p.off.cpu().tolist())
    sizes = ta.decoded_size_batch(*p.triple())
    assert sizes.size.cpu().numpy().view(np.uint32).tolist() == lens.tolist() and (sizes.status.cpu().numpy() == 2).all()
    back = ta.decompress_batch(*p.triple(), out_cap=torch.from_numpy(lens.astype(np.int64) + 1).to(dev))
    assert (back.status.cpu().numpy() == 2).all()
    assert back.streams() == inputs
