"""CPU test of the index's hash as the kernels and the library compile it (csrc/bcw_murmur.h): tools/murmur_check.cpp
feeds it every key length 0..80 block by block and through a byte pointer, against a byte-at-a-time restatement and
the known answers of test_index_oracle.py -- the program stands alone (no device, no library), so the same source is
what a sanitizer build runs (its header says how)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_murmur_host_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/murmur_check.cpp")
    exe = str(tmp_path / "murmur_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "murmur_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    assert out.startswith("murmur_check ok")
