"""CPU test of the compaction filter rules' shared text (csrc/bcw_rules.h: validation of a bcw_compact_rules, the
packed prefix table, the chunked prefix match, the rule order): tools/rules_check.cpp checks every refusal
bcw_index_set_compact_rules makes and the accepted edge cases, and the chunked match against a byte-wise memcmp model
over a few thousand (key, prefix) pairs. The program stands alone (no device, no library) and includes the header the
filter kernel compiles, so the same source is what a sanitizer build runs (its header says how)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rules_host_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/rules_check.cpp")
    exe = str(tmp_path / "rules_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "rules_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.startswith("rules_check ok")
