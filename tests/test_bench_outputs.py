"""bench.py --dump-outputs: the arrays written after the timed steps are the transforms of the bench's seeded input (checked
against the CPU oracle), whole when small and a seeded sample of rows when larger than the 64 MB cap; a plain run's line
carries none of the --full measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT_SEED = 0x5EED0003   # bench.py's fillRandom seed of the input


def _bench(workload, out_dir, steps=3):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", workload, "--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0
    assert "cpu_baseline" not in d and "attainable" not in d["roofline"] and "per_kernel" not in d["roofline"]
    return d, np.load(os.path.join(out_dir, "output.npy"))


@pytest.mark.gpu
def test_dump_outputs_whole(tmp_path, oracle):
    n, batch = 4096, 64
    d, got = _bench(f"c2c_2p12_b{batch}", tmp_path)
    assert got.dtype == np.float32 and got.shape == (batch, 2 * n)
    assert d["outputs"]["sample"] == "all"
    x = oracle.random_complex_batch(n, batch, INPUT_SEED).reshape(-1)
    want = oracle.c2c_ref_batch(x, [n], batch, "forward", "none")
    assert oracle.rel_l2(got.reshape(-1), want) <= 1e-5 and oracle.rel_max(got.reshape(-1), want) <= 1e-5


@pytest.mark.gpu
def test_dump_outputs_sampled_rows(tmp_path, oracle):
    n, batch = 1 << 20, 16
    d, got = _bench(f"c2c_2p20_b{batch}", tmp_path)
    assert got.nbytes < 64e6 and got.dtype == np.float32
    keep = got.shape[0]
    assert 1 <= keep < batch and got.shape[1] == 2 * n
    rows = sorted(int(i) for i in np.random.default_rng(0x5EED00D0).choice(batch, keep, replace=False))
    for k, b in enumerate(rows):
        x = oracle.random_complex_batch(n, 1, INPUT_SEED, b).reshape(-1)
        want = oracle.c2c_ref_batch(x, [n], 1, "forward", "none")
        assert oracle.rel_l2(got[k], want) <= 1e-5 and oracle.rel_max(got[k], want) <= 1e-5, f"row {b}"
