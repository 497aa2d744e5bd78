"""CPU test of the host's device-memory types and layouts (csrc/bcw_devmem.h): tools/devmem_check.cpp
runs the six device layouts through the carver's two passes (measured total == end of the carve, alignment, no
overlap, a take past the end refused), the record table's column list and its helpers, and the owning handle's
reserve / move / free logic against stand-ins for the HIP calls -- the program stands alone (no device, no library),
so the same source is what a sanitizer build runs (its header says how)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devmem_host_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/devmem_check.cpp")
    exe = str(tmp_path / "devmem_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "devmem_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    assert out.startswith("devmem_check ok")
