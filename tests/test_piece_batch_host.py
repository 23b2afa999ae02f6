"""CPU tier: batch piece calls (tamp_batch_compress_pieces, ``CompressorBatch``) as far as no device is needed -- the symbols and
their bindings, the object's layout, everything the C call refuses before it looks for a device, and the keyword refusals of
``CompressorBatch``, which come before the native library is looked for."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tamp_batch_compress_pieces", "tamp_amd_piece_object_size", "tamp_amd_pieces_phase_ms")
OK, INVALID_CONF, NO_DEVICE, BAD_ARGUMENT = 0, -3, -20, -21
MEM_HOST, MEM_DEVICE, ALL_DEVICES = 0, 1, -1


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_symbols_and_bindings(lib):
    from tamp_amd import _lib

    header = open(os.path.join(ROOT, "include", "tamp_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(raw, name), name
    assert len(lib.tamp_batch_compress_pieces.argtypes) == 17 and lib.tamp_batch_compress_pieces.restype is C.c_int
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(r" T %s$" % name, out, flags=re.M), name


def test_object_layout(lib):
    from tamp_amd import _lib

    assert C.sizeof(_lib.TampAmdPieceObject) == 48
    assert C.sizeof(_lib.TampAmdLazyCarry) == 32
    assert _lib.TampAmdPieceObject.window_pos.offset == 32 and _lib.TampAmdPieceObject.token_written.offset == 34
    header = open(os.path.join(ROOT, "include", "tamp_amd.h")).read()
    assert re.search(r"typedef struct TampAmdPieceObject\s*\{[^}]*TampAmdLazyCarry carry;[^}]*uint16_t window_pos;[^}]*"
                     r"uint8_t token_written;[^}]*uint8_t reserved\[13\];[^}]*\}", header)
    for bits in range(8, 16):
        assert lib.tamp_amd_piece_object_size(bits) == 48 + (1 << bits)
        assert lib.tamp_amd_piece_object_size(bits) % 16 == 0  # (the smallest stride is a valid one)
    for name, value in (("HEADER", 1), ("APPEND_MARKER", 2), ("RESUME", 4), ("FINISH", 8), ("FLUSH_TOKEN", 16), ("SKIP", 128)):
        assert getattr(_lib, "PIECE_" + name) == value
        assert re.search(r"TAMP_AMD_PIECE_%s = %d\b" % (name, value), header)


def _call(lib, *, missing=(), n=2, window=10, stride=None, mem=MEM_HOST, device=0, conf=True, lazy=0):
    from tamp_amd import _lib

    stride = 48 + (1 << window) if stride is None else stride
    held = dict(objects=np.zeros(2 * max(stride, 48 + (1 << 15)) + 16, np.uint8), ops=np.zeros(2, np.uint8), inp=np.zeros(16, np.uint8),
                in_off=np.zeros(2, np.uint64), in_len=np.array([4, 4], np.uint32), out=np.zeros(1024, np.uint8),
                out_off=np.array([0, 512], np.uint64), out_cap=np.array([512, 512], np.uint32), out_len=np.full(2, 77, np.uint32),
                status=np.full(2, 55, np.int8))
    p = {k: v.ctypes.data_as(C.c_void_p) for k, v in held.items()}
    for k in missing:
        p[k] = None
    c = _lib.TampAmdConf(window, 8, 0, 1, 0, lazy)
    rc = lib.tamp_batch_compress_pieces(C.byref(c) if conf else None, p["objects"], stride, p["ops"], p["inp"], p["in_off"], p["in_len"],
                                        p["out"], p["out_off"], p["out_cap"], p["out_len"], p["status"], n, 0, mem, device, None)
    if rc != OK or n == 0:  # (no refused call writes anything)
        assert (held["out_len"] == 77).all() and (held["status"] == 55).all() and not held["out"].any() and not held["objects"].any()
    return rc


def test_refusals_come_before_the_device(lib):
    for device in (0, 63, -7):  # the same answers for a device there is none of
        for table in ("objects", "ops", "in_off", "in_len", "out_off", "out_cap", "out_len", "status"):
            assert _call(lib, missing=(table,), device=device) == BAD_ARGUMENT, table
        assert _call(lib, conf=False, device=device) == BAD_ARGUMENT
        for window in (8, 10, 15):
            size = 48 + (1 << window)
            for stride in (0, 48, size - 16, size + 8, size + 4, size + 1):
                assert _call(lib, window=window, stride=stride, device=device) == BAD_ARGUMENT, (window, stride)
        for mem in (2, -1, 7):
            assert _call(lib, mem=mem, device=device) == BAD_ARGUMENT, mem
        assert _call(lib, n=1 << 32, device=device) == BAD_ARGUMENT
        assert _call(lib, n=0, device=device) == OK  # nothing to do, and nothing is done
        assert _call(lib, n=0, device=device, missing=("objects", "ops", "in_off", "status")) == OK
    for mem in (MEM_HOST, MEM_DEVICE):
        assert _call(lib, mem=mem, device=ALL_DEVICES) == BAD_ARGUMENT
        assert _call(lib, mem=mem, device=ALL_DEVICES, n=0) == BAD_ARGUMENT
    # device-memory objects are 16-byte aligned (host arrays stand in: the refusal comes before anything is read)
    held = np.zeros(4096, np.uint8)
    base = held.ctypes.data
    odd = C.c_void_p(base + (16 - base % 16) % 16 + 8)
    from tamp_amd import _lib

    c = _lib.TampAmdConf(8, 8, 0, 1, 0, 0)
    z = np.zeros(2, np.uint64)
    q = z.ctypes.data_as(C.c_void_p)
    assert lib.tamp_batch_compress_pieces(C.byref(c), odd, 48 + 256, q, q, q, q, q, q, q, q, q, 1, 0, MEM_DEVICE, 0, None) == BAD_ARGUMENT


def test_phase_times_without_a_call(lib):
    ms = (C.c_float * 4)(7, 7, 7, 7)
    assert lib.tamp_amd_pieces_phase_ms(C.byref(ms)) == OK and list(ms) == [-1.0] * 4  # nothing recorded
    assert lib.tamp_amd_pieces_phase_ms(None) == BAD_ARGUMENT


def test_invalid_conf(lib):
    for window in (7, 16):
        assert _call(lib, window=window, stride=48 + (1 << 15)) == INVALID_CONF, window
    assert _call(lib, lazy=2) == INVALID_CONF


def test_a_well_formed_call_needs_a_device(lib):
    if lib.tamp_amd_device_count() > 0:
        assert _call(lib, device=63) in (NO_DEVICE, BAD_ARGUMENT)  # (a device ordinal that is not there: nothing is launched)
        return
    assert _call(lib) == NO_DEVICE
    assert _call(lib, stride=48 + 1024 + 16) == NO_DEVICE


def test_python_names():
    import tamp
    import tamp_amd

    for pkg in (tamp_amd, tamp):
        assert "CompressorBatch" in pkg.__all__ and pkg.CompressorBatch is tamp_amd.CompressorBatch
    for method in ("write", "flush", "reset_dictionary", "close"):
        assert callable(getattr(tamp_amd.CompressorBatch, method))


def test_keyword_refusals_come_before_the_library(monkeypatch):
    import tamp_amd
    from tamp_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(ValueError, match="Dictionary-window size mismatch"):
        tamp_amd.CompressorBatch(4, window=10, dictionary=bytes(512))
    with pytest.raises(ValueError):
        tamp_amd.CompressorBatch(4, append=True)  # (without dictionary_reset)
    with pytest.raises(ValueError):
        tamp_amd.CompressorBatch(4, window=8, append=True, dictionary_reset=True, dictionary=bytes(256))
    for kwargs in (dict(window=7), dict(window=16), dict(literal=4), dict(literal=9)):
        with pytest.raises(ValueError):
            tamp_amd.CompressorBatch(4, **kwargs)
    for n in (-1, 2.0, True, "4"):
        with pytest.raises(ValueError):
            tamp_amd.CompressorBatch(n)
    batch = tamp_amd.CompressorBatch(4, dictionary_reset=True)  # (constructing needs neither the library nor a device)
    for chunks in ([b"a"] * 3, [b"a"] * 5, []):
        with pytest.raises(ValueError, match="chunks for 4 streams"):
            batch.write(chunks)
    for which in ([4], [-1], [0, 1, 99]):
        for call in (lambda w: batch.flush(which=w), lambda w: batch.flush(False, w), batch.reset_dictionary):
            with pytest.raises(ValueError, match="which"):
                call(which)
    with pytest.raises(ValueError, match="dictionary_reset"):
        tamp_amd.CompressorBatch(4).reset_dictionary()
