"""CPU tier: which compress build a batch call takes (tamp_amd_compress_build, the launcher's own predicate).

The fixed-geometry builds (tamp_compress_fixed::compress_kernel<FIX>) are compiled for ONE configuration: window 2^10,
literal 8, default parse, 1,024-position blocks, whole streams (no saved state, no segment flags, the plain header byte in
front, a dword-aligned dictionary).  They are taken for exactly that and refused for every single deviation; the generic
build stays reachable through TAMP_AMD_FIXED_BUILD=0.
"""
import ctypes
import os

import pytest

GENERIC, FIXED_EXT, FIXED_V1 = 0, 1, 2
STATE, RESUME, SAVE, FLUSH_TOKEN, PARTIAL, APPEND, BLOCK_MODE = 1, 2, 4, 8, 16, 32, 64


@pytest.fixture(scope="module")
def build():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    lib = _lib.load()

    def query(window=10, literal=8, extended=1, custom=0, reset=0, lazy=0, hint=0, max_in_len=4096, flags=0, dict_addr=0):
        conf = _lib.TampAmdConf(window, literal, custom, extended, reset, lazy, hint, 0)
        return lib.tamp_amd_compress_build(ctypes.byref(conf), max_in_len, flags, dict_addr)

    return query


@pytest.fixture(autouse=True)
def clean_env():
    names = ("TAMP_AMD_FIXED_BUILD", "TAMP_AMD_BLK", "TAMP_AMD_RUNS")
    saved = {k: os.environ.pop(k, None) for k in names}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def test_taken_for_exactly_the_flagship_configuration(build):
    assert build(extended=1) == FIXED_EXT
    assert build(extended=0) == FIXED_V1
    # stream length: anything that plans 1,024-position blocks of 256 threads -- 1 KiB and more, or unknown
    for n in (0, 1024, 1025, 4096, 65536, 1 << 20):
        assert build(max_in_len=n) == FIXED_EXT and build(extended=0, max_in_len=n) == FIXED_V1, n
    # a custom dictionary at a dword-aligned address (its header bit rides in the lead byte: still the plain header)
    assert build(custom=1, dict_addr=0x7F0000001000) == FIXED_EXT
    assert build(custom=1, extended=0, dict_addr=0x7F0000001004) == FIXED_V1
    # the hint only picks the build of SHORT messages
    assert build(hint=1) == FIXED_EXT and build(hint=2) == FIXED_EXT


def test_the_layout_is_the_generic_builds(build):
    from tamp_amd import _lib

    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert _lib.load().tamp_amd_compress_plan(10, 4096, 0, *[ctypes.byref(x) for x in v]) == 0
    assert tuple(x.value for x in v) == (1024, 19616, 256, 8)  # block, LDS bytes, threads, workgroups per CU


@pytest.mark.parametrize("window", [8, 9, 11, 12, 13, 14, 15])
def test_refused_for_another_window(build, window):
    assert build(window=window) == GENERIC and build(window=window, extended=0) == GENERIC


@pytest.mark.parametrize("literal", [5, 6, 7])
def test_refused_for_another_literal_width(build, literal):
    assert build(literal=literal) == GENERIC and build(literal=literal, extended=0) == GENERIC


@pytest.mark.parametrize("blk", ["64", "256", "512", "960"])
def test_refused_for_a_block_override(build, blk):
    os.environ["TAMP_AMD_BLK"] = blk
    assert build() == GENERIC and build(extended=0) == GENERIC


def test_a_block_override_that_changes_nothing_changes_nothing(build):
    os.environ["TAMP_AMD_BLK"] = "1024"
    assert build() == FIXED_EXT


def test_refused_for_short_messages(build):
    for n in (1, 64, 256, 512, 960):
        assert build(max_in_len=n) == GENERIC and build(max_in_len=n, hint=2) == GENERIC, n


@pytest.mark.parametrize("flags", [STATE, RESUME, SAVE, FLUSH_TOKEN, PARTIAL, STATE | RESUME, STATE | SAVE, STATE | RESUME | SAVE | FLUSH_TOKEN,
                                   STATE | SAVE | PARTIAL])
def test_refused_for_a_state_pointer_and_each_segment_flag(build, flags):
    assert build(flags=flags) == GENERIC and build(extended=0, flags=flags) == GENERIC


def test_refused_for_dictionary_reset(build):
    assert build(reset=1) == GENERIC and build(reset=1, extended=0) == GENERIC


@pytest.mark.parametrize("addr", [0x7F0000001001, 0x7F0000001002, 0x7F0000001003])
def test_refused_for_a_misaligned_dictionary(build, addr):
    assert build(custom=1, dict_addr=addr) == GENERIC and build(custom=1, extended=0, dict_addr=addr) == GENERIC
    assert build(custom=0, dict_addr=addr) == FIXED_EXT  # (no custom dictionary: the address is not looked at)


def test_refused_for_an_appended_lead(build):
    assert build(flags=APPEND) == GENERIC and build(extended=0, flags=APPEND) == GENERIC


def test_refused_for_block_mode(build):
    assert build(extended=0, max_in_len=1 << 20, flags=BLOCK_MODE) == GENERIC
    assert build(extended=0, max_in_len=1 << 20) == FIXED_V1


def test_refused_for_the_lazy_parse(build):
    assert build(lazy=1) == GENERIC and build(lazy=1, extended=0) == GENERIC


def test_the_switch_forces_the_generic_build(build):
    os.environ["TAMP_AMD_FIXED_BUILD"] = "0"
    assert build() == GENERIC and build(extended=0) == GENERIC
    os.environ["TAMP_AMD_FIXED_BUILD"] = "1"
    assert build() == FIXED_EXT and build(extended=0) == FIXED_V1
    assert build(window=11) == GENERIC  # (the switch forces nothing the other way)


def test_bad_arguments(build):
    from tamp_amd import _lib

    assert build(window=7) < 0 and build(window=16) < 0 and build(literal=4) < 0 and build(literal=9) < 0
    assert _lib.load().tamp_amd_compress_build(None, 4096, 0, 0) < 0
