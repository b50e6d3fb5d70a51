"""bench.py --dump-outputs on the host: what dump_outputs writes for a model and the losses of a step, in full and as the fixed
sample it falls back to above its size budget."""
import os

import numpy as np
import torch

import bench


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.BatchNorm1d(32))


def test_dump_writes_the_losses_and_the_whole_state_as_float_arrays(tmp_path):
    m = _model()
    bench.dump_outputs(str(tmp_path), {"cls": torch.tensor(0.5)}, m)
    assert sorted(os.listdir(tmp_path)) == ["loss.cls.npy", "state.0.bias.npy", "state.0.weight.npy", "state.1.bias.npy",
                                            "state.1.running_mean.npy", "state.1.running_var.npy", "state.1.weight.npy"]
    loss = np.load(tmp_path / "loss.cls.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [0.5]
    w = np.load(tmp_path / "state.0.weight.npy")
    assert w.dtype == np.float32 and np.array_equal(w, m[0].weight.detach().numpy().reshape(-1))


def test_dump_above_the_budget_keeps_the_same_sample_every_run(tmp_path, monkeypatch):
    m = _model()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2048)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), {"cls": 0.5}, m)
    bench.dump_outputs(str(b), {"cls": 0.5}, m)
    assert sum(np.load(a / f).nbytes for f in os.listdir(a)) <= 2048
    w = np.load(a / "state.0.weight.npy")
    assert 0 < w.size < 64 * 32 and np.array_equal(w, np.load(b / "state.0.weight.npy"))
    assert np.isin(w, m[0].weight.detach().numpy()).all()
