"""CPU test of the writer's host-and-device text: tools/frame_check.cpp checks the framing rules, varints, CRC mask
and Record.Encode header that the host and the writer kernels compile (csrc/bcw_frame.h) against models written from
the reference's own loops -- the program stands alone (no device, no library), so the same source is what a sanitizer
build runs (its header says how)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_host_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/frame_check.cpp")
    exe = str(tmp_path / "frame_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "frame_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    assert out.startswith("frame_check ok")
