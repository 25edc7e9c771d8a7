"""bench.py --dump-outputs and --full: the dump of the state the last timed step left (dtypes, the seeded env sample that keeps
it under its budget) on CPU tensors, and a small plain run on the GPU (no legs, identical outputs from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Sim:
    """The attributes of KilobotSim that dump_outputs reads, on the CPU (velocity drive, no objects, no sleep state)."""

    def __init__(self, E, N):
        g = torch.Generator().manual_seed(7)
        self.num_envs, self.device = E, torch.device('cpu')
        self.x, self.y, self.theta, self.v, self.w = (torch.randn(E, N, generator=g) for _ in range(5))
        self.status = torch.randint(0, 1 << 20, (E,), generator=g, dtype=torch.int32)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False and bench.parse_args([]).dump_outputs is None
    a = bench.parse_args(['--full', '--dump-outputs', 'out', '--steps', '7'])
    assert a.full and a.dump_outputs == 'out' and a.steps == 7


def test_dump_writes_every_state_field_of_every_env(tmp_path):
    s = _Sim(6, 16)
    bench.dump_outputs(s, str(tmp_path))
    d = _load(str(tmp_path))
    assert sorted(d) == ['status', 'theta', 'v', 'w', 'x', 'y']
    for f in ('x', 'y', 'theta', 'v', 'w'):
        assert d[f].dtype == np.float32 and np.array_equal(d[f], getattr(s, f).numpy())
    assert d['status'].dtype == np.float64 and np.array_equal(d['status'], s.status.numpy().astype(np.float64))


def test_dump_samples_envs_to_stay_within_the_budget(tmp_path, monkeypatch):
    E, N = 50, 32
    per_env = 5 * N * 4 + 8
    monkeypatch.setattr(bench, 'DUMP_BUDGET', 12 * per_env + 5)
    s = _Sim(E, N)
    bench.dump_outputs(s, str(tmp_path / 'a'))
    bench.dump_outputs(s, str(tmp_path / 'b'))
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    idx = a['env_index'].astype(np.int64)
    assert a['env_index'].dtype == np.float64 and len(idx) == 12 and np.all(np.diff(idx) > 0) and idx[-1] < E
    assert sum(v.nbytes for k, v in a.items() if k != 'env_index') <= bench.DUMP_BUDGET
    for f in ('x', 'y', 'theta', 'v', 'w', 'status'):
        assert np.array_equal(a[f], getattr(s, f).numpy()[idx].astype(a[f].dtype)), f
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)      # the sample is fixed


def _bench(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--envs', '16', '--bots', '64', '--steps', '4',
                        '--warmup', '2', '--dump-outputs', out_dir], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_identical_outputs(tmp_path):
    d1 = _bench(str(tmp_path / 'a'))
    d2 = _bench(str(tmp_path / 'b'))
    for d in (d1, d2):
        assert d['metric'] == 'kilobot-steps/sec' and d['unit'] == 'kilobot-steps/s' and d['higher_is_better'] is True
        assert d['dtype'] == 'f32' and d['steps'] == 4 and d['status_flags'] == 0
        assert abs(d['value'] - 16 * 64 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
        assert 'cpu_baseline' not in d and 'audit_pass' not in d['roofline']
        assert all(d[k] is None for k in ('fused_env_step', 'with_sleep_state', 'jammed_swarm', 'cfg2', 'cfg4'))
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    assert sorted(a) == ['status', 'theta', 'v', 'w', 'x', 'y'] and a['x'].shape == (16, 64)
    assert all(np.array_equal(a[k], b[k]) for k in a)
