"""CPU tier: the decoded-size query's boundary -- the symbol, its argument errors (reported before any device is touched, in
the order tamp_batch_decompress uses) and the Python surface that goes with it.  No compute calls."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_header_declares_and_library_exports_the_call(lib):
    from tamp_amd import _lib

    text = open(os.path.join(ROOT, "include", "tamp_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+tamp_batch_decoded_size\s*\(", text)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "tamp_batch_decoded_size")
    assert "tamp_batch_decoded_size" in _lib.SYMBOLS


def _call(lib, *, in_off=True, in_len=True, size=True, status=True, limit=False, n=1, mem=None, device=0):
    from tamp_amd import _lib

    data = np.array([0x58, 0, 0, 0], dtype=np.uint8)
    tables = dict(in_off=np.zeros(1, np.uint64), in_len=np.full(1, 4, np.uint32), size=np.zeros(1, np.uint32),
                  status=np.zeros(1, np.int8), limit=np.full(1, 7, np.uint32))
    want = dict(in_off=in_off, in_len=in_len, size=size, status=status, limit=limit)
    p = {k: (tables[k].ctypes.data_as(C.c_void_p) if want[k] else None) for k in tables}
    return lib.tamp_batch_decoded_size(0, 15, data.ctypes.data_as(C.c_void_p), p["in_off"], p["in_len"], p["limit"], p["size"],
                                       p["status"], None, n, _lib.MEM_HOST if mem is None else mem, device, None)


@pytest.mark.parametrize("missing", ["in_off", "in_len", "size", "status"])
def test_a_null_table_is_a_bad_argument(lib, missing):
    assert _call(lib, **{missing: False}) == -21
    assert _call(lib, limit=True, **{missing: False}) == -21


def test_bad_mem_and_all_devices_with_device_memory_are_bad_arguments(lib):
    from tamp_amd import _lib

    assert _call(lib, mem=2) == -21
    assert _call(lib, mem=-1) == -21
    assert _call(lib, mem=_lib.MEM_DEVICE, device=_lib.ALL_DEVICES) == -21
    assert _call(lib, mem=7, device=_lib.ALL_DEVICES) == -21  # (the memory kind is looked at first)
    assert _call(lib, n=1 << 32) == -21


def test_python_surface():
    import tamp
    import tamp_amd

    sig = inspect.signature(tamp_amd.decompress_batch)
    assert sig.parameters["out_cap"].default is None
    assert sig.parameters["max_out"].default == 0xFFFFFFFF
    for pkg in (tamp_amd, tamp):
        assert callable(pkg.decoded_size_batch) and "decoded_size_batch" in pkg.__all__
    sig = inspect.signature(tamp_amd.decoded_size_batch)
    assert list(sig.parameters) == ["data", "in_off", "in_len", "limit", "dictionary", "max_window_bits", "device", "stream", "timing"]
    assert sig.parameters["limit"].default is None and sig.parameters["max_window_bits"].default == 15
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[3:])
