"""CPU test of the payload parsers' host-and-device text: tools/parse_check.cpp runs uvarint and parse_record
(csrc/bcw_parse.h, the text the decode, the point reads, the Get and the scrub compile) over a plain array and over a
fragment list, against a model written from the reference's own loops, on the payload families of tests/_payloads.py
at every NsSize of the GPU tests -- the program stands alone (no device, no library), so the same source is what a
sanitizer build runs (its header says how)."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_host_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/parse_check.cpp")
    exe = str(tmp_path / "parse_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "parse_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    assert out.startswith("parse_check ok")
    n = {k: int(v) for k, v in re.findall(r"(ok|invalid|panic) (\d+)", out.split("status", 1)[1])}
    assert min(n.values()) > 1000  # every class, many times over
