"""CPU tests of the space accounting's host text: tools/usage_check.cpp checks the closed form of WalRecordSize the
index's accounting pass compiles (csrc/bcw_usage.h) against the reference's loop and, at sizes no loop can walk,
against the same formula in 128-bit arithmetic -- the program stands alone (no device, no library), so the same
source is what a sanitizer build runs (its header says how); and the picker helper against a restatement of
DefaultCompactionPicker (db.go:200-224)."""
from __future__ import annotations

import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_usage_host_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/usage_check.cpp")
    exe = str(tmp_path / "usage_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "usage_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    assert out.startswith("usage_check ok")


def test_closed_form_matches_the_library_loop():
    """the same closed form restated in Python against bcw_wal_record_size (the loop, oracle-tested in test_capi)"""
    from bitcaskdb_amd import _lib as L

    def closed(off, size):
        if size == 0:
            return 0
        lo = 32768 - (off - 40) % 32768
        total = 0
        if lo < 7:
            total, lo = lo, 32768
        first = min(size, lo - 7)
        total += 7 + first
        rem = size - first
        if rem:
            total += (rem // 32761) * 32768 + ((7 + rem % 32761) if rem % 32761 else 0)
        return total

    rnd = random.Random(5)
    for _ in range(3000):
        off, size = 40 + rnd.randrange(1 << 30), rnd.randrange(1 << rnd.randrange(1, 21))
        assert closed(off, size) == L.lib.bcw_wal_record_size(off, size)


def _picker_model(infos, ratio):
    """db.go:200-224 line by line; the unstable sort made total by the fid"""
    wals = [tuple(w) for w in infos]
    wals.sort(key=lambda w: w[0])
    wals.sort(key=lambda w: w[2], reverse=True)  # stable: equal FreeBytes stay in ascending fid order
    res = []
    for fid, size, free in wals:
        q = float("inf") if size == 0 and free else float("nan") if size == 0 else free / size
        if q < ratio:
            break
        res.append(fid)
        if len(res) >= 2:
            break
    return res


def test_default_compaction_picker():
    from bitcaskdb_amd import PickerWalInfo, default_compaction_picker as pick
    assert pick([], 0.3) == []
    assert pick([(1, 1000, 100)], 0.3) == []
    assert pick([(1, 1000, 300)], 0.3) == [1]
    assert pick([(1, 1000, 299)], 0.3) == []
    # descending FreeBytes, at most two
    assert pick([(1, 1000, 500), (2, 1000, 900), (3, 1000, 700)], 0.3) == [2, 3]
    # the walk stops at the first WAL below the ratio, though a later one is above it (a smaller file)
    assert pick([(1, 10000, 500), (2, 1000, 900), (3, 1000, 400)], 0.3) == [2]
    # a tie in FreeBytes: ascending fid, whatever the input order
    assert pick([(9, 1000, 500), (4, 1000, 500), (7, 1000, 500)], 0.3) == [4, 7]
    assert pick([(4, 1000, 500), (7, 1000, 500), (9, 1000, 500)], 0.3) == [4, 7]
    assert pick([PickerWalInfo(5, 100, 90), PickerWalInfo(3, 100, 90)], 0.5) == [3, 5]
    assert pick([(1, 0, 0), (2, 0, 5)], 0.3) == [2, 1]  # Go's float division by zero: never below the ratio
    rnd = random.Random(11)
    for _ in range(300):
        infos = [(fid, rnd.choice([0, 100, 1000, 1 << 30]), rnd.choice([0, 10, 50, 400, 999, 1 << 29]))
                 for fid in rnd.sample(range(50), rnd.randrange(0, 9))]
        ratio = rnd.choice([0.0, 0.1, 0.3, 0.5, 1.0])
        assert pick(infos, ratio) == _picker_model(infos, ratio)
