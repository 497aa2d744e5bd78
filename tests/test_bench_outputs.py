"""bench.py's result line and --dump-outputs: a plain run times exactly --steps steps and runs none of the --full
legs, and the dumped record table of its last timed step equals the oracle's decode of the same synthetic segment."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE = 1_700_000_000
COLS = ("foff", "size", "expire", "key_len", "val_len", "meta_len", "first_frag", "emit_frag", "hdr_size", "flags",
        "etag_off", "status")


def _fake_outputs(n, cap):
    """a record table and result on the host, as bench.py holds them on the device"""
    import torch
    from bitcaskdb_amd import _lib as L
    tdt = {"u8": torch.int64, "u4": torch.int32, "u1": torch.uint8}
    cols = {}
    for i, (name, dt) in enumerate(L.TABLE_COLUMNS):
        if name in ("aux0", "aux1"):
            continue
        cols[name] = ((torch.arange(cap, dtype=torch.int64) * (i + 3)) % 251).to(tdt[dt])
    res = L.DecodeResult(n_records=n, n_records_total=n, n_frags=n + 5, first_bad_record=-1, generation=77)
    d_res = torch.from_numpy(np.frombuffer(bytes(res), dtype=np.uint8).copy())
    return L, cols, d_res


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    n, cap = 1000, 1064
    L, cols, d_res = _fake_outputs(n, cap)
    whole = tmp_path / "whole"
    bench.dump_outputs(str(whole), L, cols, d_res)
    assert sorted(os.listdir(whole)) == sorted([c + ".npy" for c in COLS] + ["result.npy"])
    res = np.load(whole / "result.npy")
    assert res.dtype == np.float64 and len(res) == len(bench.RESULT_FIELDS)
    assert res[bench.RESULT_FIELDS.index("n_records")] == n and res[bench.RESULT_FIELDS.index("first_bad_record")] == -1
    for c in COLS:
        a = np.load(whole / (c + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape == (n,)
        assert (a == cols[c][:n].numpy().astype(np.float64)).all(), c
    # above the budget: the same seeded rows of every column, identical from call to call
    row_bytes = sum(np.load(whole / (c + ".npy")).dtype.itemsize for c in COLS)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 100 * (row_bytes + 8))
    s1, s2 = tmp_path / "s1", tmp_path / "s2"
    bench.dump_outputs(str(s1), L, cols, d_res)
    bench.dump_outputs(str(s2), L, cols, d_res)
    rows = np.load(s1 / "sample_rows.npy")
    assert rows.dtype == np.float64 and len(rows) == 100 and (np.diff(rows) > 0).all() and rows[-1] < n
    total = 0
    for f in os.listdir(s1):
        a = np.load(s1 / f)
        total += a.nbytes
        assert (a == np.load(s2 / f)).all(), f
    assert total <= 100 * (row_bytes + 8) + 8 * len(bench.RESULT_FIELDS)
    for c in COLS:
        assert (np.load(s1 / (c + ".npy")) == np.load(whole / (c + ".npy"))[rows.astype(np.int64)]).all(), c


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    steps, seg = 3, 6 << 20
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", "1", "--seg-bytes", str(seg), "--dump-outputs", str(tmp_path / "out")],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    ln = lines[0]
    assert ln["steps"] == steps and ln["ms_per_step"] > 0 and ln["unit"] == "GiB/s" and ln["higher_is_better"] is True
    assert ln["dtype"] == "u8" and ln["full"] is False
    assert abs(ln["value"] - ln["config"]["seg_bytes"] / 2 ** 30 / (ln["ms_per_step"] * 1e-3)) <= 0.02 * ln["value"]
    # the roofline's k_crc samples come from inside the timed steps (event pairs on every 4th launch)
    assert 1 <= ln["roofline"]["kernel_launches_timed"] <= steps
    # none of the --full legs ran
    assert ln["cpu_baseline"] is None and ln["pcie_inclusive_GiBs"] is None and ln["roofline"]["kernel_ms_all"] is None
    assert not {"pipelined", "config_c", "encode_e", "e2e", "cpu_all_cores", "cpu_config_a_pread"} & set(ln)
    # the dumped table is the oracle's decode of the oracle's own synthetic segment (same generator, seed 42)
    seg_bytes = O.synth(seg, 0, 42, value_mode=0)
    assert len(seg_bytes) == ln["config"]["seg_bytes"]
    ref = O.decode(seg_bytes, 40, BASE, 20, 20, want_bytes=False)
    n = len(ref.recs)
    assert n == ln["config"]["records"] > 1000 and ref.err_class == 0
    res = np.load(tmp_path / "out" / "result.npy")
    assert res[0] == n and res[2] == len(ref.frags) == ln["config"]["fragments"] and res[5] == 0
    total = res.nbytes
    for c in COLS:
        a = np.load(tmp_path / "out" / (c + ".npy"))
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64) and a.shape == (n,), c
        assert (a == ref.recs[c].astype(np.float64)).all(), c
    assert total <= 64 << 20
