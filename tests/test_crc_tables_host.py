"""CPU test of the CRC-32C constant tables every context uploads (csrc/bcw_crc_tables.h: initc, enc_ops, pow2 and the
stream verify's LDS image): tools/crc_tables_check.cpp checks each against a bit-at-a-time CRC-32C restated in it, the
known answers of CRC-32C, and the hashes of the tables as they were built before the header existed -- the program
stands alone (no device, no library), so the same source is what a sanitizer build runs (its header says how)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_crc_tables_host_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/crc_tables_check.cpp")
    exe = str(tmp_path / "crc_tables_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "crc_tables_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.splitlines()[-1] == "crc_tables_check ok"
