"""CPU tests of the host text behind bcw_index_verify* (csrc/bcw_verify.h): tools/verify_check.cpp checks the class
decision, the untrusted-span pre-check and the `fits` rule the scrub kernels compile against brute-force models -- the
program stands alone (no device, no library), so the same source is what a sanitizer build runs (its header says
how); the constants against the header; and the class decision restated in Python, the model the GPU tests
(test_gpu_verify.py) build their expectation on, against a table of cases."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VFY_OK, VFY_NO_WAL, VFY_READ, VFY_RECORD, VFY_KEY = range(5)


def test_verify_host_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/verify_check.cpp")
    exe = str(tmp_path / "verify_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "verify_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    assert out.startswith("verify_check ok")


def test_constants_and_layouts_match_the_header():
    from bitcaskdb_amd import _lib as L
    assert (L.VFY_OK, L.VFY_NO_WAL, L.VFY_READ, L.VFY_RECORD, L.VFY_KEY) == (0, 1, 2, 3, 4)
    with open(os.path.join(ROOT, "include", "bcw.h")) as fh:
        text = fh.read()
    for name, val in (("OK", 0), ("NO_WAL", 1), ("READ", 2), ("RECORD", 3), ("KEY", 4)):
        assert re.search(r"#define BCW_VFY_%s %d\b" % (name, val), text), name
    assert "#define BCW_ABI_VERSION 2" in text
    # the layouts the header states: 48-byte list entries, and the result's fields where C puts them
    assert C.sizeof(L.VerifyBad) == 48 and L.VerifyBad.key_len.offset == 40 and L.VerifyBad.cls.offset == 44
    assert C.sizeof(L.VerifyOut) == 48 and L.VerifyOut.rows_cap.offset == 40
    r = L.VerifyResult
    assert (r.by_class.offset, r.by_rd.offset, r.n_bad.offset, r.per_fid.offset) == (16, 56, 120, 136)
    assert r.fits.offset == 136 + C.sizeof(L.UsageResult) and C.sizeof(r) == r.fits.offset + 8


# bcw_verify.h restated ----------------------------------------------------------------------------------------
def classify(wal_found: bool, rd_status: int, rec_status: int, key_equal: bool) -> int:
    if not wal_found:
        return VFY_NO_WAL
    if rd_status != 0:
        return VFY_READ
    if rec_status != 0:
        return VFY_RECORD
    return VFY_OK if key_equal else VFY_KEY


def span_untrusted(off: int, size: int, seg_len: int) -> bool:
    return size > seg_len or off < 40 or off > seg_len


def fits(n_bad, bad_cap, key_bytes, keys_cap, n_fids, rows_cap, overflow=False) -> bool:
    return n_bad <= bad_cap and key_bytes <= keys_cap and n_fids <= rows_cap and not overflow


CASES = [  # (wal found, rd_status, rec_status, key equal) -> class: Get's order, then the key
    ((True, 0, 0, True), VFY_OK),
    ((True, 0, 0, False), VFY_KEY),
    ((True, 0, 1, True), VFY_RECORD),
    ((True, 0, 2, False), VFY_RECORD),       # a record that does not parse has no key to compare
    ((True, 1, 0, True), VFY_READ),
    ((True, 3, 2, False), VFY_READ),         # a read error hides what the bytes would parse to
    ((True, 7, 0, True), VFY_READ),
    ((False, 0, 0, True), VFY_NO_WAL),
    ((False, 3, 1, False), VFY_NO_WAL),      # no WAL: nothing else is looked at
]


@pytest.mark.parametrize("args,cls", CASES)
def test_class_decision(args, cls):
    assert classify(*args) == cls


def test_every_combination_has_one_class_in_gets_order():
    for wal in (False, True):
        for rd in range(8):
            for rec in range(4):
                for eq in (False, True):
                    c = classify(wal, rd, rec, eq)
                    first = 1 if not wal else 2 if rd else 3 if rec else 4 if not eq else 0
                    assert c == first


def test_span_pre_check_and_fits_edges():
    assert [span_untrusted(o, 11, 1000) for o in (0, 17, 39, 40, 1000, 1001)] == [True, True, True, False, False, True]
    assert [span_untrusted(40, z, 1000) for z in (0, 1000, 1001, 2 ** 64 - 1)] == [False, False, True, True]
    assert fits(0, 0, 0, 0, 0, 0) and fits(3, 3, 30, 30, 2, 2)
    assert not fits(3, 2, 30, 30, 2, 2) and not fits(3, 3, 30, 29, 2, 2) and not fits(3, 3, 30, 30, 2, 1)
    assert not fits(0, 0, 0, 0, 0, 0, overflow=True)
