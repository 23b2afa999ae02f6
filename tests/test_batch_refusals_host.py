"""CPU tier: what the batch calls refuse before any device is looked for -- the five entry points that take the per-stream tables
(tamp_batch_compress_dicts, tamp_batch_decompress_dicts, tamp_batch_decoded_size_dicts, tamp_batch_decompress_resume,
tamp_batch_compress_resume) and the three plain twins.  Every refusal is TAMP_AMD_BAD_ARGUMENT (-21); a call that got as far as a
device would answer TAMP_AMD_NO_DEVICE (-20) on a machine without one.  No compute calls (modelled on tests/test_decoded_size_host.py)."""
import ctypes as C

import numpy as np
import pytest

BAD_ARGUMENT = -21


@pytest.fixture(scope="module")
def lib():
    from tamp_amd import _lib

    try:
        return _lib.load()
    except _lib.NativeLibraryError:
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")


def _arrays():
    a = dict(data=np.array([0x58, 0, 0, 0], dtype=np.uint8), in_off=np.zeros(1, np.uint64), in_len=np.full(1, 4, np.uint32),
             out=np.zeros(64, np.uint8), out_off=np.zeros(1, np.uint64), out_cap=np.full(1, 64, np.uint32),
             out_len=np.zeros(1, np.uint32), status=np.zeros(1, np.int8), consumed=np.zeros(1, np.uint32),
             dict=np.zeros(1024, np.uint8), dict_off=np.zeros(1, np.uint64), states=np.zeros(4096, np.uint8))
    return a, {k: v.ctypes.data_as(C.c_void_p) for k, v in a.items()}


# name -> (the tables the call refuses to take as null, how it is called).  `p`: the pointers (a missing one is None), `x`: what the
# resume calls take on top (stride, window_bits_max, op).
def _compress_dicts(lib, conf, p, x, n, mem, dev):
    return lib.tamp_batch_compress_dicts(C.byref(conf), p["dict"], 1024, p["dict_off"], p["data"], p["in_off"], p["in_len"], p["out"],
                                         p["out_off"], p["out_cap"], p["out_len"], p["status"], n, 0, mem, dev, None)


def _compress(lib, conf, p, x, n, mem, dev):
    return lib.tamp_batch_compress(C.byref(conf), p["dict"], p["data"], p["in_off"], p["in_len"], p["out"], p["out_off"], p["out_cap"],
                                   p["out_len"], p["status"], n, 0, mem, dev, None)


def _decompress_dicts(lib, conf, p, x, n, mem, dev):
    return lib.tamp_batch_decompress_dicts(p["dict"], 1024, p["dict_off"], 15, p["data"], p["in_off"], p["in_len"], p["out"], p["out_off"],
                                           p["out_cap"], p["out_len"], p["status"], p["consumed"], n, mem, dev, None)


def _decompress(lib, conf, p, x, n, mem, dev):
    return lib.tamp_batch_decompress(p["dict"], 1024, 15, p["data"], p["in_off"], p["in_len"], p["out"], p["out_off"], p["out_cap"],
                                     p["out_len"], p["status"], p["consumed"], n, mem, dev, None)


def _decoded_size_dicts(lib, conf, p, x, n, mem, dev):
    return lib.tamp_batch_decoded_size_dicts(1024, p["dict_off"], 15, p["data"], p["in_off"], p["in_len"], p["out_cap"], p["out_len"],
                                             p["status"], p["consumed"], n, mem, dev, None)


def _decoded_size(lib, conf, p, x, n, mem, dev):
    return lib.tamp_batch_decoded_size(1024, 15, p["data"], p["in_off"], p["in_len"], p["out_cap"], p["out_len"], p["status"],
                                       p["consumed"], n, mem, dev, None)


def _decompress_resume(lib, conf, p, x, n, mem, dev):
    return lib.tamp_batch_decompress_resume(p["states"], x["stride"], x["bits"], p["data"], p["in_off"], p["in_len"], p["out"], p["out_off"],
                                            p["out_cap"], p["out_len"], p["status"], p["consumed"], n, mem, dev, None)


def _compress_resume(lib, conf, p, x, n, mem, dev):
    return lib.tamp_batch_compress_resume(p["states"], x["stride"], x["bits"], x["op"], 0, p["data"], p["in_off"], p["in_len"], p["out"],
                                          p["out_off"], p["out_cap"], p["out_len"], p["status"], p["consumed"], n, mem, dev, None)


SLABS = ("in_off", "in_len", "out_off", "out_cap", "out_len", "status")
CALLS = {
    "tamp_batch_compress_dicts": (SLABS, _compress_dicts),
    "tamp_batch_compress": (SLABS, _compress),
    "tamp_batch_decompress_dicts": (SLABS, _decompress_dicts),
    "tamp_batch_decompress": (SLABS, _decompress),
    "tamp_batch_decoded_size_dicts": (("in_off", "in_len", "out_len", "status"), _decoded_size_dicts),
    "tamp_batch_decoded_size": (("in_off", "in_len", "out_len", "status"), _decoded_size),
    "tamp_batch_decompress_resume": (("states",) + SLABS, _decompress_resume),
    "tamp_batch_compress_resume": (("states",) + SLABS, _compress_resume),
}
RESUME = ("tamp_batch_decompress_resume", "tamp_batch_compress_resume")


def _call(lib, name, *, missing=(), n=1, mem=None, device=0, **extra):
    from tamp_amd import _lib

    held, p = _arrays()
    for k in missing:
        p[k] = None
    x = dict(stride=2048, bits=10, op=_lib.OP_COMPRESS)  # (2,048: a multiple of 16 above both state sizes at window 10)
    x.update(extra)
    conf = _lib.TampAmdConf(10, 8, 1, 1, 0, 0, 0, 0)
    rc = CALLS[name][1](lib, conf, p, x, n, _lib.MEM_HOST if mem is None else mem, device)
    del held
    return rc


@pytest.mark.parametrize("name", list(CALLS))
def test_each_required_table_null_in_turn(lib, name):
    for table in CALLS[name][0]:
        assert _call(lib, name, missing=(table,)) == BAD_ARGUMENT, table
        assert _call(lib, name, missing=(table, "consumed")) == BAD_ARGUMENT, table


@pytest.mark.parametrize("name", list(CALLS))
def test_memory_kind_all_devices_and_stream_count(lib, name):
    from tamp_amd import _lib

    assert _call(lib, name, mem=2) == BAD_ARGUMENT
    assert _call(lib, name, mem=-1) == BAD_ARGUMENT
    assert _call(lib, name, mem=_lib.MEM_DEVICE, device=_lib.ALL_DEVICES) == BAD_ARGUMENT
    assert _call(lib, name, mem=7, device=_lib.ALL_DEVICES) == BAD_ARGUMENT  # (the memory kind is looked at first)
    assert _call(lib, name, n=1 << 32) == BAD_ARGUMENT
    assert _call(lib, name, n=1 << 32, mem=_lib.MEM_DEVICE) == BAD_ARGUMENT


def test_compress_refuses_a_null_conf(lib):
    from tamp_amd import _lib

    _, p = _arrays()
    for fn, lead in ((lib.tamp_batch_compress_dicts, (None, p["dict"], 1024, p["dict_off"])), (lib.tamp_batch_compress, (None, p["dict"]))):
        assert fn(*lead, p["data"], p["in_off"], p["in_len"], p["out"], p["out_off"], p["out_cap"], p["out_len"], p["status"], 1, 0,
                  _lib.MEM_HOST, 0, None) == BAD_ARGUMENT


@pytest.mark.parametrize("name", RESUME)
def test_resume_calls_refuse_stride_window_and_op(lib, name):
    from tamp_amd import _lib

    size = (lib.tamp_amd_decoder_state_size if "decompress" in name else lib.tamp_amd_encoder_state_size)(10)
    assert size <= 2048
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        assert _call(lib, name, mem=mem, stride=2048 + 8) == BAD_ARGUMENT          # not a multiple of 16
        assert _call(lib, name, mem=mem, stride=(size - 1) & ~15) == BAD_ARGUMENT  # a multiple of 16 below the state's size
        assert _call(lib, name, mem=mem, stride=0) == BAD_ARGUMENT
        assert _call(lib, name, mem=mem, bits=7) == BAD_ARGUMENT
        assert _call(lib, name, mem=mem, bits=16) == BAD_ARGUMENT
        assert _call(lib, name, mem=mem, bits=12) == BAD_ARGUMENT                  # (2,048 bytes hold no 4 KiB window)
        if name == "tamp_batch_compress_resume":
            assert _call(lib, name, mem=mem, op=_lib.OP_POLL - 1) == BAD_ARGUMENT
            assert _call(lib, name, mem=mem, op=_lib.OP_COMPRESS_AND_FLUSH + 1) == BAD_ARGUMENT
    # (the states' address: a multiple of 4)
    held, p = _arrays()
    odd = C.c_void_p(held["states"].ctypes.data + 1)
    lead = (odd, 2048, 10) if "decompress" in name else (odd, 2048, 10, _lib.OP_COMPRESS, 0)
    assert getattr(lib, name)(*lead, p["data"], p["in_off"], p["in_len"], p["out"], p["out_off"], p["out_cap"], p["out_len"], p["status"],
                              p["consumed"], 1, _lib.MEM_HOST, 0, None) == BAD_ARGUMENT
