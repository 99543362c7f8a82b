"""bench.py's command line and --dump-outputs writer, on the host (the timed path itself needs an MI355X)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
    return bench.parse()


def test_plain_run_is_lean_by_default(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, '--full', '--dump-outputs', 'd')
    assert a.full and a.dump_outputs == 'd'


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, '--steps', '0')


def _trainer(groups):
    opt = lambda ps: types.SimpleNamespace(param_groups=[{'params': ps}])  # noqa: E731
    return types.SimpleNamespace(optimizers_dict={k: opt(v) for k, v in groups.items()})


def test_dump_outputs_writes_losses_and_parameters(tmp_path):
    g = torch.Generator().manual_seed(1)
    back = [torch.randn(64, 32, 3, 3, generator=g), torch.randn(64, generator=g)]
    front = [torch.randn(1000, generator=g)]
    out = ({'semseg_sensor_a_loss': torch.tensor(1.25), 'cycle_loss': torch.tensor(0.5)}, {}, torch.tensor(1.75))
    names = bench.dump_outputs(str(tmp_path), _trainer({'optimizer_back': back, 'optimizer_front_sensor_a': front}), out)
    assert sorted(os.listdir(tmp_path)) == sorted(n + '.npy' for n in names)
    assert np.load(tmp_path / 'final_loss.npy') == np.float32(1.75)
    assert np.load(tmp_path / 'loss_semseg_sensor_a_loss.npy') == np.float32(1.25)
    p = np.load(tmp_path / 'params_optimizer_back.npy')
    assert p.dtype == np.float32
    np.testing.assert_array_equal(p, torch.cat([t.reshape(-1) for t in back]).numpy())
    np.testing.assert_array_equal(np.load(tmp_path / 'params_optimizer_front_sensor_a.npy'), front[0].numpy())


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 40_000)
    big = [torch.arange(50_000, dtype=torch.float32)]
    out = ({'loss': torch.tensor(2.0)}, {}, torch.tensor(2.0))
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), _trainer({'optimizer_back': big}), out)
    a, b = np.load(tmp_path / 'a' / 'params_optimizer_back.npy'), np.load(tmp_path / 'b' / 'params_optimizer_back.npy')
    assert sum(f.stat().st_size - 128 for f in (tmp_path / 'a').iterdir()) <= 40_000
    np.testing.assert_array_equal(a, b)  # the same fixed sample every time
    assert a.size < 50_000 and np.all(np.diff(a) > 0) and np.all(a == np.round(a))  # sorted indices into the full vector
