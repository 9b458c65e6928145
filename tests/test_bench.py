"""GPU: bench.py's contract on a small batch.  A plain run times exactly --steps encode steps and prints the
headline line alone; --dump-outputs writes what the last timed step returned (the oracle's streams, the same
files from run to run); --full adds the decode pass, per-kernel times, roofline, secondary figures and the CPU
baseline.  The benchmark runs as a fresh interpreter with a timeout, as it is run for every change."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BLOCKS, BLOCK, WB = 8, 32768, 15
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("decode_MBps", "decode_ms_per_step", "kernels_ms", "roofline", "secondary", "cpu_baseline")
DUMPED = ("out_sample", "out_sample_pos", "out_bytes", "out_off", "err")


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--blocks", str(N_BLOCKS),
           "--block-bytes", str(BLOCK), "--win-bits", str(WB), *args]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {name: np.load(os.path.join(d, name + ".npy")) for name in DUMPED}


def test_plain_run_dumps_the_last_step_and_full_adds_the_rest(tmp_path):
    plain = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"))
    assert all(k in plain for k in HEADLINE)
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert plain["unit"] == "MB/s" and plain["higher_is_better"] is True and plain["dtype"] == "u8"
    assert not [k for k in FULL_ONLY if k in plain]

    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(name + ".npy" for name in DUMPED)
    assert sum(os.path.getsize(tmp_path / "plain" / f) for f in files) <= 64 << 20
    got = _load(tmp_path / "plain")
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert not got["err"].any()
    for b in range(N_BLOCKS):
        want = np.frombuffer(O.encode(O.zipf_block(b, BLOCK), WB, header=False), np.uint8)
        assert got["out_bytes"][b] == want.size, f"block {b}"
        assert np.array_equal(got["out_sample"][b], want[got["out_sample_pos"][b].astype(np.int64)]), f"block {b}"

    full = _bench("--full", "--steps", "2", "--warmup", "1", "--cpu-blocks", "1",
                  "--dump-outputs", str(tmp_path / "full"))
    assert full["steps"] == 2 and all(k in full for k in HEADLINE + FULL_ONLY)
    assert full["compressed_ratio"] == plain["compressed_ratio"]
    again = _load(tmp_path / "full")
    for name in DUMPED:
        assert np.array_equal(again[name], got[name]), name
