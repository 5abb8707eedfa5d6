"""bench.py on an MI355X: a plain run prints the headline line and nothing it does not need; --full adds the untimed passes
and the checks against the CPU oracle, and leaves the timed window's outputs as they were."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = ['--gpus', '1', '--steps', '20', '--warmup', '5']


def bench_line(argv, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'DCLR_BENCH_CHILD')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + argv, env=env, capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs(tmp_path):
    plain = bench_line(WINDOW + ['--dump-outputs', str(tmp_path / 'plain')])
    assert plain['unit'] == 'scan-pairs/s' and plain['higher_is_better'] is True and plain['steps'] == 20
    assert plain['value'] > 0 and abs(plain['value'] * plain['ms_per_step'] - 8e3) < 1e-6 * 8e3       # 8 pairs per step
    for key in ('secondary', 'cpu_baseline', 'pose_delta_vs_oracle', 'latency_ms_per_batch'):
        assert key not in plain, key
    assert plain['kernels_us'] and plain['roofline']['avg_us'] > 0 and plain['roofline']['alone_us'] is None

    full = bench_line(WINDOW + ['--full', '--no-secondary', '--no-cpu-leg', '--pose-pairs', '2',
                                '--dump-outputs', str(tmp_path / 'full')])
    assert full['pose_delta_pairs'] == 2 and full['pose_delta_max'] < 1e-4
    assert full['roofline']['alone_us'] > 0 and full['latency_ms_per_batch']['batches'] > 0
    assert 'cpu_baseline' not in full and 'secondary' not in full
    y_plain, y_full = np.load(str(tmp_path / 'plain' / 'y.npy')), np.load(str(tmp_path / 'full' / 'y.npy'))
    assert y_plain.shape == (8, 8) and np.isfinite(y_plain).all() and np.array_equal(y_plain, y_full)


@pytest.mark.gpu
def test_plain_and_full_latency_runs():
    argv = ['--gpus', '1', '--latency', '--steps', '10', '--warmup', '2']
    plain = bench_line(argv)
    assert list(plain['latency_ms']) == ['pairwise'] and plain['ms_per_step'] == plain['latency_ms']['pairwise']['median_ms']
    assert plain['kernels_us'] is None and plain['back_to_back_pairs_per_s'] is None and 'pose_delta_vs_oracle' not in plain
    full = bench_line(argv + ['--full', '--no-cpu-leg'])
    assert set(full['latency_ms']) == {'pairwise', 'sequential'} and full['kernels_us'] and full['back_to_back_pairs_per_s'] > 0
    assert full['pose_delta_vs_oracle'] < 1e-4 and 'cpu_baseline' not in full
