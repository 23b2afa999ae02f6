"""CPU tier of the dictionary-table calls (tamp_batch_*_dicts; ``dictionaries=`` / ``dictionary_index=`` in Python): the symbols,
the argument errors that need no device, and the proof that the GPU tier's inputs can tell one dictionary from another."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dict_table_input as dti  # noqa: E402

NEW = ("tamp_batch_compress_dicts", "tamp_batch_decompress_dicts", "tamp_batch_decoded_size_dicts")
OLD = ("tamp_batch_compress", "tamp_batch_decompress", "tamp_batch_decoded_size", "tamp_amd_compress", "tamp_amd_decompress",
       "tamp_amd_compress_build", "tamp_amd_compress_plan", "tamp_amd_decompress_plan", "tamp_amd_trim",
       "tamp_compressor_init", "tamp_compressor_compress_and_flush", "tamp_decompressor_init", "tamp_decompressor_decompress")


def test_the_three_calls_are_exported_next_to_the_old_ones():
    import subprocess

    from tamp_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "libtamp_amd.so not built (run __graft_entry__.build())"
    exported = {line.split()[-1] for line in subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode().splitlines()
                if line.split()[-2:-1] == ["T"]}
    lib = ctypes.CDLL(_lib.LIB_PATH)  # loading needs libamdhip64 but no GPU
    for name in NEW + OLD:
        assert name in exported and hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "tamp_amd.h")).read()
    for name in NEW:
        assert name + "(" in header, name


def test_inputs_detect_an_ignored_selector(oracle):
    dti.assert_inputs_detect_an_ignored_selector(oracle)


def test_input_shape():
    sel, lens = dti.selectors_and_lengths()
    assert len(sel) == 160 and sel[:10] == [0, 1, 2, 3, 4] * 2 and set(sel[80:120]) == {3} and sel[120:125] == [4, 3, 2, 1, 0]
    assert set(lens) == {0, 1} | set(dti.LONG_LENGTHS)
    for w in (8, 10, 12, 15):
        d = dti.dictionaries(w)
        assert len(d) == dti.K and all(len(x) == 1 << w for x in d) and len(set(d)) == dti.K


@pytest.fixture(scope="module")
def ta():
    import tamp_amd

    return tamp_amd


def _calls(ta):
    """The three calls in the keyword form -> fn(streams, dictionary, dictionaries, dictionary_index).  ``decoded_size_batch`` keeps
    its parameter list: it takes the pair as ``dictionary=DictionaryTable(dictionaries, dictionary_index)``."""
    def size_query(streams, dictionaries=None, dictionary_index=None):
        return ta.decoded_size_batch(streams, dictionary=ta.DictionaryTable(dictionaries, dictionary_index))

    def keywords(fn, **more):
        return lambda streams, **kw: fn(streams, **kw, **more)
    return (keywords(ta.compress_batch, window=10), keywords(ta.decompress_batch, out_cap=64), keywords(ta.decompress_batch), size_query)


def test_argument_errors_need_no_device(ta):
    d10 = dti.dictionaries(10)
    streams = [b"volt=1;amp=2;", b"temp=3;"]
    for fn in _calls(ta):
        if fn.__name__ != "size_query":
            with pytest.raises(ValueError, match="exclude each other"):
                fn(streams, dictionary=d10[0], dictionaries=d10, dictionary_index=[0, 1])
            with pytest.raises(ValueError, match="exclude each other"):
                fn(streams, dictionary=ta.DictionaryTable(d10, [0, 1]), dictionaries=d10, dictionary_index=[0, 1])
            with pytest.raises(ValueError, match="needs dictionaries"):
                fn(streams, dictionary_index=[0, 1])
        with pytest.raises(ValueError, match="needs a dictionary_index"):
            fn(streams, dictionaries=d10)
        for bad in ([0, 5], [-1, 0], np.array([0, dti.K], dtype=np.int64)):
            with pytest.raises(ValueError, match="out of range"):
                fn(streams, dictionaries=d10, dictionary_index=bad)
        with pytest.raises(ValueError, match="integer"):
            fn(streams, dictionaries=d10, dictionary_index=[0.0, 1.0])
        with pytest.raises(ValueError, match="equal length"):
            fn(streams, dictionaries=[d10[0], d10[1][:512]], dictionary_index=[0, 1])
        with pytest.raises(ValueError, match="multiple of 16"):
            fn(streams, dictionaries=[x[:1000] for x in d10], dictionary_index=[0, 1])
        with pytest.raises(ValueError, match=r"\(K, D\)"):
            fn(streams, dictionaries=np.zeros(1024, np.uint8), dictionary_index=[0, 0])
    # compress: D is the window itself
    for wrong in (9, 11):
        with pytest.raises(ValueError, match="Dictionary-window size mismatch"):
            ta.compress_batch(streams, window=wrong, dictionaries=d10, dictionary_index=[0, 1])
        with pytest.raises(ValueError, match="Dictionary-window size mismatch"):
            ta.compress_batch(streams, window=wrong, dictionary=ta.DictionaryTable(d10, [0, 1]))
    with pytest.raises(ValueError, match="Dictionary-window size mismatch"):
        ta.compress_batch(streams, window=10, dictionaries=np.zeros((3, 2048), np.uint8), dictionary_index=[0, 1])


def test_the_size_query_keeps_its_parameter_list(ta):
    """(tests/test_decoded_size_host.py pins it; the table goes in as ``dictionary=``)"""
    import inspect

    assert "dictionaries" not in inspect.signature(ta.decoded_size_batch).parameters
    for fn in (ta.compress_batch, ta.decompress_batch):
        assert {"dictionaries", "dictionary_index"} <= set(inspect.signature(fn).parameters)
    assert "DictionaryTable" in ta.__all__
    t = ta.DictionaryTable(dti.dictionaries(8), np.array([4, 0, 2], dtype=np.uint8))
    assert (t.count, t.size, len(t)) == (dti.K, 256, dti.K * 256)
    assert t.on_host(3)[1].tolist() == [1024, 0, 512] and t.on_host(3)[1].dtype == np.uint64


def test_one_selector_per_stream(ta):
    """(raised after the library has loaded: the streams are counted there)"""
    d10 = dti.dictionaries(10)
    for fn in _calls(ta):
        try:
            with pytest.raises(ValueError, match="per stream"):
                fn([b"volt=1;", b"amp=2;", b"ohm=3;"], dictionaries=d10, dictionary_index=[0, 1])
        except ta.NativeLibraryError:
            pytest.skip("libtamp_amd.so not built")


def test_c_abi_refuses_a_table_without_the_custom_bit():
    """tamp_batch_compress_dicts: the custom bit sits in the one header byte the launch shares -- checked before any device is
    looked for."""
    from tamp_amd import _lib

    try:
        lib = _lib.load()
    except _lib.NativeLibraryError:
        pytest.skip("libtamp_amd.so not built")
    conf = _lib.TampAmdConf(10, 8, 0, 1, 0, 0, 0, 0)
    z8, z4, z1 = np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.int8)
    buf = np.zeros(1024, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.tamp_batch_compress_dicts(ctypes.byref(conf), p(buf), 1024, p(z8), p(buf), p(z8), p(z4), p(buf), p(z8), p(z4), p(z4), p(z1),
                                       1, 0, _lib.MEM_HOST, 0, None)
    assert rc == _lib.BAD_ARGUMENT
    conf.use_custom_dictionary = 1  # ... nor one without a buffer
    rc = lib.tamp_batch_compress_dicts(ctypes.byref(conf), None, 0, p(z8), p(buf), p(z8), p(z4), p(buf), p(z8), p(z4), p(z4), p(z1),
                                       1, 0, _lib.MEM_HOST, 0, None)
    assert rc == _lib.BAD_ARGUMENT
