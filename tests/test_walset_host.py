"""CPU test of the resident WAL set's host side (csrc/bcw_walset.h: sorted insert, replace, remove, hand-back of
owned images): tools/walset_check.cpp replays 20 000 random operations against a std::map model. The program stands
alone (no device, no library), so the same source is what a sanitizer build runs (its header says how)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walset_host_table_matches_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/walset_check.cpp")
    exe = str(tmp_path / "walset_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "walset_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.startswith("walset_check ok")
