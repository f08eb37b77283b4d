"""-m gpu: a plain bench.py run (no --full) in a fresh child process does the headline and nothing else: the JSON line keeps its
contract, and the legs that moved behind --full (roofline and fused-kernel probes, other configurations, CPU baseline, the N > 1
loop / collective / scaling legs) leave no trace in it."""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_headline_only():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '8192']
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, MFG_BENCH_HEAT='5'), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    z = json.loads(lines[0])
    assert z['metric'] == 'env-steps/sec for batched d-bin population rollouts' and z['unit'] == 'env-steps/s'
    assert z['higher_is_better'] is True and z['dtype'] == 'f32 (f64 accumulate)'
    assert z['n_gpus'] == 1 and z['steps'] == 3 and z['warmup'] == 1 and z['config']['global_batch'] == 8192
    assert z['value'] > 0 and abs(z['value'] - 8192 * 15 * 3 / (z['ms_per_step'] * 3e-3)) <= 1e-6 * z['value']
    assert z['roofline'] is None and z['fused_kernel'] is None and z['cpu_baseline'] is None
    assert not {'configs', 'collective', 'loops', 'other_scaling', 'c5_strong'} & set(z)
