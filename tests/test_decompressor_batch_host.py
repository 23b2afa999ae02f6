"""CPU tier: what ``tamp_amd.DecompressorBatch`` and its two C calls decide on the host, before any device is looked for --
constructor and ``read`` refusals, which streams take part, the slab arithmetic of ``read(out_cap=None)``, and the refusals of
``tamp_batch_decompress_pieces`` / ``tamp_batch_decoded_size_pieces``.  The decoding itself: tests/test_gpu_decompressor_batch.py.
"""
import os
import sys

import numpy as np
import pytest

import tamp_amd
from tamp_amd import _lib
from tamp_amd.batch import _read_participants, _read_slabs, _read_which

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decompressor_batch_input import c_tables as _tables, decode_pieces as _decode, size_pieces as _size  # noqa: E402

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libtamp_amd.so not built")


def test_exported_and_aliased():
    assert "DecompressorBatch" in tamp_amd.__all__
    assert tamp_amd.DecompressorBatch is tamp_amd.batch.DecompressorBatch
    for name in ("tamp_batch_decompress_pieces", "tamp_batch_decoded_size_pieces"):
        assert name in _lib.SYMBOLS


def test_constructor_needs_no_device_and_refuses_bad_arguments():
    d = tamp_amd.DecompressorBatch(5, window_bits=10)
    assert (d.n, d.window_bits, d.stride) == (5, 10, 16 + 1024)
    assert tamp_amd.DecompressorBatch(3).stride == 16 + (1 << 15)  # DecoderBatch's default
    for bad_n in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError):
            tamp_amd.DecompressorBatch(bad_n)
    for bits in (7, 16):
        with pytest.raises(ValueError):
            tamp_amd.DecompressorBatch(1, window_bits=bits)
    plain = _lib.TampAmdConf(10, 8, 0, 1, 0, 0, 0)
    custom = _lib.TampAmdConf(10, 8, 1, 1, 0, 0, 0)
    with pytest.raises(ValueError, match="use_custom_dictionary"):  # a dictionary the conf does not ask for
        tamp_amd.DecompressorBatch(1, window_bits=10, conf=plain, dictionary=bytes(1024))
    with pytest.raises(ValueError, match="custom dictionary expected"):  # DecoderBatch's own refusal
        tamp_amd.DecompressorBatch(1, window_bits=10, conf=custom)
    tamp_amd.DecompressorBatch(1, window_bits=10, conf=custom, dictionary=bytes(1024))
    tamp_amd.DecompressorBatch(1, window_bits=10, dictionary=bytes(1024))  # conf=None: the streams' headers decide


def test_read_refusals_come_before_any_launch():
    """Every one of these raises ValueError although no device exists here: the checks run before the library is loaded."""
    d = tamp_amd.DecompressorBatch(4, window_bits=10)
    with pytest.raises(ValueError, match="3 chunks for 4 streams"):
        d.read([b"a", None, b""])
    with pytest.raises(ValueError, match="5 chunks"):
        d.read([None] * 5)
    with pytest.raises(ValueError, match="named twice"):
        d.read([None] * 4, which=[1, 2, 1])
    for bad in ([4], [-1], [0, 7]):
        with pytest.raises(ValueError, match="0..3"):
            d.read([None] * 4, which=bad)
    with pytest.raises(ValueError, match="max_out"):
        d.read([None] * 4, max_out=1 << 32)
    with pytest.raises(ValueError, match="out_cap needs 4"):
        d.read([b"x"] * 4, out_cap=[1, 2, 3])
    with pytest.raises(ValueError, match="32 bits"):
        d.read([b"x"] * 4, out_cap=[1, 2, 3, 1 << 32])
    assert d._objects is None  # nothing was made


def test_none_takes_no_part_and_empty_bytes_does():
    none = np.zeros(6, dtype=bool)
    chunks = [b"ab", None, b"", bytearray(), None, memoryview(b"c")]
    assert _read_participants(chunks, none).tolist() == [True, False, True, True, False, True]
    assert _read_participants([None] * 6, none).tolist() == [False] * 6
    # `which` adds streams whose chunk is None (tensors: whose in_len is 0) ...
    assert _read_participants(chunks, _read_which([4], 6)).tolist() == [True, False, True, True, True, True]
    # ... and is a mask of its own
    assert _read_which(None, 3).tolist() == [False] * 3
    assert _read_which([2, 0], 3).tolist() == [True, False, True]
    assert _read_which(np.array([1], dtype=np.int64), 3).tolist() == [False, True, False]
    assert _read_which([], 0).tolist() == []


def test_slabs_are_size_plus_one_at_the_running_sum():
    size = np.array([0, 5, 0, 241, 1, 4000], dtype=np.uint32)
    cap, off = _read_slabs(size, 0xFFFFFFFF)
    assert cap.tolist() == [1, 6, 1, 242, 2, 4001]
    assert off.tolist() == [0, 1, 7, 8, 250, 252]
    assert int(cap.sum()) == 4253 and cap.dtype == np.int64
    # max_out bounds the room, never the spare byte on top of it
    cap, off = _read_slabs(size, 241)
    assert cap.tolist() == [1, 6, 1, 241, 2, 241]
    assert off.tolist() == [0, 1, 7, 8, 249, 251]
    cap, off = _read_slabs(size, 0)
    assert cap.tolist() == [0] * 6 and off.tolist() == [0] * 6
    # sizes are uint32 values whatever the storage: int32 tables come back from the device
    wrapped = np.array([-1, 7], dtype=np.int32)
    cap, off = _read_slabs(wrapped, 0xFFFFFFFF)
    assert cap.tolist() == [0xFFFFFFFF, 8] and off.tolist() == [0, 0xFFFFFFFF]
    cap, off = _read_slabs(np.zeros(0, dtype=np.uint32), 100)
    assert cap.size == 0 and off.size == 0


def test_slabs_on_torch_tensors_match_numpy():
    torch = pytest.importorskip("torch")
    size = np.array([0, 5, 0, 241, 1, 4000, -1], dtype=np.int32)
    for max_out in (0xFFFFFFFF, 241, 1, 0):
        want_cap, want_off = _read_slabs(size, max_out)
        cap, off = _read_slabs(torch.from_numpy(size), max_out)
        assert cap.dtype == torch.int64 and cap.tolist() == want_cap.tolist() and off.tolist() == want_off.tolist()


@needs_lib
def test_c_calls_refuse_before_a_device_is_looked_for():
    """TAMP_AMD_BAD_ARGUMENT, not TAMP_AMD_NO_DEVICE, on a machine without a GPU -- and with one, no launch: the host arrays passed as
    "device memory" here are never touched."""
    lib = _lib.load()
    bad = _lib.BAD_ARGUMENT
    t = _tables(3)
    for call, tables in ((_decode, ("states", "in_off", "in_len", "out_off", "out_cap", "out_len", "status")),
                         (_size, ("states", "in_off", "in_len", "out_len", "status"))):
        for name in tables:
            assert call(lib, t, 3, **{name: True}) == bad, (call.__name__, name)
        for stride in (1041, 1048, 1024, 16):  # not a multiple of 16; below 16 + (1 << 10)
            assert call(lib, t, 3, stride=stride) == bad, (call.__name__, stride)
        for bits in (7, 16, 0, 255):
            assert call(lib, t, 3, bits=bits) == bad, (call.__name__, bits)
        assert call(lib, t, 3, device=_lib.ALL_DEVICES) == bad  # objects stay on one device
        assert call(lib, t, 0, bits=7) == bad and call(lib, t, 0, stride=8) == bad  # n_rows == 0 excuses the tables alone
    assert all(not v.any() for v in t.values())
