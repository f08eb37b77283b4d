"""-m gpu: bench.py --dump-outputs, run in fresh child processes: what the timed train() call computed in its last step, as
float32 / float64 .npy files within 64 MB, and the same bits from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('theta', 'w', 'episode_reward', 'pi_last', 'pi_traj', 'reward', 'delta', 'g')


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1', '--no-configs',
           '--no-cpu-baseline', '--no-roofline', '--dump-outputs', str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, MFG_BENCH_HEAT='5'), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith('{')][-1])


def test_dump_outputs_are_the_last_step_and_repeat_bit_for_bit(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    z = _bench(tmp_path / 'a', 3)
    assert z['steps'] == 3 and z['ms_per_step'] > 0
    a = {n: np.load(tmp_path / 'a' / (n + '.npy')) for n in NAMES}
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(n + '.npy' for n in NAMES)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')) <= 64_000_000
    d, T, F = 21, 15, 21 * 22 // 2 + 21 + 1
    n = a['pi_last'].shape[0]
    assert 0 < n < 65536                                   # the default batch is sampled down to the budget
    assert a['theta'].shape == (1,) and a['theta'][0] == z['theta_end'] and a['w'].shape == (F,)
    assert a['episode_reward'].shape == (3,)               # one entry per timed step
    assert a['pi_traj'].shape == (n, T + 1, d) and a['reward'].shape == (n, T) and a['delta'].shape == a['g'].shape == (n, T)
    assert np.array_equal(a['pi_traj'][:, -1], a['pi_last'])
    _bench(tmp_path / 'b', 3)
    for name in NAMES:
        assert np.array_equal(np.load(tmp_path / 'b' / (name + '.npy')), a[name]), name
