"""CPU tests of the host text behind bcw_index_drop_fids* (csrc/bcw_drop.h): tools/drop_check.cpp checks the
membership test, the selection predicate and the list normalisation the drop kernel and the export kernels compile
against a std::set model -- the program stands alone (no device, no library), so the same source is what a
sanitizer build runs (its header says how); and the predicate restated in Python, the model the GPU tests
(test_gpu_index_drop.py) build their dict model on, against a set model of its own."""
from __future__ import annotations

import bisect
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP_IN, DROP_NOT_IN = 0, 1
MAX_FIDS = 4096
U64 = 2 ** 64 - 1


def test_drop_host_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tools/drop_check.cpp")
    exe = str(tmp_path / "drop_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "bitcaskdb_amd", "csrc"),
                    os.path.join(ROOT, "tools", "drop_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    assert out.startswith("drop_check ok")


def test_constants_match_the_header():
    from bitcaskdb_amd import _lib as L
    assert (L.DROP_IN, L.DROP_NOT_IN, L.USAGE_MAX_FIDS) == (DROP_IN, DROP_NOT_IN, MAX_FIDS)
    with open(os.path.join(ROOT, "include", "bcw.h")) as fh:
        text = fh.read()
    assert "#define BCW_DROP_IN      0" in text and "#define BCW_DROP_NOT_IN  1" in text


# bcw_drop.h restated ------------------------------------------------------------------------------------------
def normalise(mode, fids):
    """the list as the kernel reads it (ascending, distinct), or None where the library answers BCW_E_INVAL"""
    if mode not in (DROP_IN, DROP_NOT_IN) or fids is None:
        return None
    out = sorted(set(fids))
    return None if len(out) > MAX_FIDS else out


def fid_in_range(norm, f):
    if not norm or f < norm[0] or f > norm[-1]:
        return False
    i = bisect.bisect_left(norm, f)
    return i < len(norm) and norm[i] == f


def selected(mode, live, off, member):
    return bool(live) and off != 0 and member == (mode == DROP_IN)


def _model(mode, live, off, fidset, f):
    if not live or off == 0:
        return False
    return (f in fidset) if mode == DROP_IN else (f not in fidset)


def _lists():
    rng = random.Random(21)
    yield []
    for f in (0, 1, 9, U64 - 1, U64):
        yield [f]
    yield [0, U64]
    yield [5, 5, 5, 9, 9, 3]  # duplicates, unsorted
    yield [U64, 0, U64, 0]
    yield [U64 - 3 * i for i in range(MAX_FIDS)]  # the cap itself
    big = list(range(1, MAX_FIDS + 1))
    yield big + [rng.choice(big) for _ in range(904)]  # 5000 entries, 4096 distinct
    for _ in range(40):
        n = rng.randrange(0, 300)
        yield [rng.choice([rng.randrange(0, 400), rng.randrange(0, 2 ** 64)]) for _ in range(n)]


@pytest.mark.parametrize("mode", [DROP_IN, DROP_NOT_IN])
def test_predicate_against_a_set_model(mode):
    rng = random.Random(22 + mode)
    for raw in _lists():
        norm = normalise(mode, raw)
        assert norm == sorted(set(raw))
        s = set(raw)
        probes = [0, 1, U64, U64 - 1] + [rng.randrange(0, 2 ** 64) for _ in range(20)]
        for f in rng.sample(norm, min(len(norm), 50)):
            probes += [f, (f + 1) & U64, (f - 1) & U64]
        for f in probes:
            assert fid_in_range(norm, f) == (f in s)
            for off in (0, 1, 39, 40):
                for live in (False, True):
                    assert selected(mode, live, off, fid_in_range(norm, f)) == _model(mode, live, off, s, f)


def test_empty_lists_and_the_soft_delete_exemption():
    assert not any(selected(DROP_IN, True, off, fid_in_range([], 7)) for off in (0, 1, 39, 40))
    assert [selected(DROP_NOT_IN, True, off, fid_in_range([], 7)) for off in (0, 1, 39, 40)] == [False, True, True, True]
    # a soft-deleted entry (fid 0, off 0) stays even when fid 0 is named, in either mode
    assert not selected(DROP_IN, True, 0, fid_in_range([0], 0))
    assert not selected(DROP_NOT_IN, True, 0, fid_in_range([5], 0))
    # a dead entry is never selected
    assert not selected(DROP_IN, False, 40, True) and not selected(DROP_NOT_IN, False, 40, False)


def test_refusals():
    assert normalise(2, [1]) is None and normalise(-1, [1]) is None
    assert normalise(DROP_IN, None) is None
    assert normalise(DROP_IN, list(range(MAX_FIDS + 1))) is None
    assert len(normalise(DROP_NOT_IN, list(range(MAX_FIDS)) * 2)) == MAX_FIDS
