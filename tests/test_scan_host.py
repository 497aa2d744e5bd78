"""CPU test of the scan by key prefix's shared text (csrc/bcw_scan.h: the argument check of bcw_index_scan*, the match /
list / count rule, the `fits` rule, the tile arithmetic): tools/scan_check.cpp checks every refusal the call makes and
the accepted edge cases (n_prefix == 0, a duplicate prefix, a 64-byte prefix, a prefix longer than the key), and the
rule against a byte-wise memcmp model over a few thousand (key, prefix set, off, flags) cases. The program stands alone
(no device, no library) and includes the header the host and the scan kernels compile, so the same source is what a
sanitizer build runs (its header says how)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_host_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/scan_check.cpp")
    exe = str(tmp_path / "scan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "scan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.startswith("scan_check ok")


def test_scan_binding_matches_header():
    """the ctypes structs have the sizes scan_check.cpp asserts of the header's, and the flag its value"""
    import ctypes as C

    from bitcaskdb_amd import _lib as L
    assert [C.sizeof(t) for t in (L.ScanParams, L.ScanGroup, L.ScanOut, L.ScanResult)] == [24, 32, 72, 48]
    assert L.SCAN_SOFT_DELETED == 1
    text = open(L.HEADER_PATH).read()
    assert "#define BCW_SCAN_SOFT_DELETED 1u" in text and "#define BCW_ABI_VERSION 2" in text
