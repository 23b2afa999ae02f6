"""CPU tier: the entry point and the carry of lazy matching in bounded pieces (include/tamp_amd.h tamp_amd_compress_piece_lazy,
TampAmdLazyCarry) -- exported, and laid out the same for a C caller and for tamp_amd._lib.  No compute calls."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_lazy_piece_call():
    from tamp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtamp_amd.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "tamp_amd_compress_piece_lazy") and hasattr(lib, "tamp_amd_compress_piece")
    assert hasattr(lib, "tamp_amd_compress_segment")
    assert "tamp_amd_compress_piece_lazy" in _lib.SYMBOLS


def test_carry_layout_in_python():
    from tamp_amd import _lib

    assert ctypes.sizeof(_lib.TampAmdCarry) == 28
    assert ctypes.sizeof(_lib.TampAmdLazyCarry) == 32
    assert _lib.TampAmdLazyCarry.carry.offset == 0 and _lib.TampAmdLazyCarry.carry.size == 28
    assert (_lib.TampAmdLazyCarry.cached_pos.offset, _lib.TampAmdLazyCarry.cached_len.offset,
            _lib.TampAmdLazyCarry.reserved2.offset) == (28, 30, 31)
    assert bytes(_lib.TampAmdLazyCarry()) == bytes(32)  # a fresh object: nothing cached


def test_carry_layout_for_a_c_caller(tmp_path):
    """A plain C translation unit against include/tamp_amd.h prints the sizes and offsets tamp_amd._lib declares."""
    from tamp_amd import _lib

    if not shutil.which("gcc"):
        pytest.skip("gcc missing")
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "tamp_amd.h"\n'
        "int main(void) {\n"
        "  TampAmdLazyCarry z = {0};\n"
        '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(TampAmdCarry), sizeof(TampAmdLazyCarry),\n'
        "         offsetof(TampAmdLazyCarry, carry), offsetof(TampAmdLazyCarry, cached_pos), offsetof(TampAmdLazyCarry, cached_len),\n"
        "         offsetof(TampAmdLazyCarry, reserved2), offsetof(TampAmdCarry, bit_count), offsetof(TampAmdCarry, bits),\n"
        "         offsetof(TampAmdCarry, tail), (int)z.cached_len);\n"
        "  (void)tamp_amd_compress_piece_lazy; (void)tamp_amd_compress_piece;\n"
        "  return 0;\n}\n"
    )
    exe = tmp_path / "layout"
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    if os.path.exists(_lib.LIB_PATH):  # (the function names are only referenced when there is a library to link)
        libdir = os.path.dirname(_lib.LIB_PATH)
        cmd += ["-L", libdir, "-ltamp_amd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    else:
        src.write_text(src.read_text().replace("  (void)tamp_amd_compress_piece_lazy; (void)tamp_amd_compress_piece;\n", ""))
    subprocess.check_call(cmd)
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    C = _lib.TampAmdCarry
    assert out == [ctypes.sizeof(C), ctypes.sizeof(_lib.TampAmdLazyCarry), _lib.TampAmdLazyCarry.carry.offset,
                   _lib.TampAmdLazyCarry.cached_pos.offset, _lib.TampAmdLazyCarry.cached_len.offset,
                   _lib.TampAmdLazyCarry.reserved2.offset, C.bit_count.offset, C.bits.offset, C.tail.offset, 0]
    assert out[:6] == [28, 32, 0, 28, 30, 31]
