"""druglamp_amd/checkpoint.py alone — pack / write / read / compare_signatures on small CPU tensors — and the scheduler's
state() / load_state() round trip.  No device, no trainer: the trainer's side is tests/test_checkpoint_gpu.py."""
import os

import pytest
import torch

from druglamp_amd import checkpoint as ck


def _signature(**over):
    sig = {"model": "DrugLAMP",
           "params": [["a.weight", [3, 4], 0], ["a.bias", [3], 12], ["b.weight", [5, 3], 16]],
           "compute_dtype": "bfloat16", "world": 1, "optimisers": ["opt", "opt_ssl"],
           "ema": {"on": True, "decay": 0.99, "warmup": True},
           "guard": {"on": False, "max_grad_norm": None, "skip_nonfinite": False},
           "freeze_bn": False, "cls_loss": None,
           "param_groups": [["a.weight", "default", False], ["a.bias", "no_decay", False], ["b.weight", "frozen", True]],
           "graph_steps": False, "fixed_caps": None}
    sig.update(over)
    return sig


def _blob(seed=0, extra=None):
    g = torch.Generator().manual_seed(seed)
    sd = {"a.weight": torch.randn(3, 4, generator=g), "a.bias": torch.randn(3, generator=g), "b.weight": torch.randn(5, 3, generator=g),
          "bn.num_batches_tracked": torch.tensor(7)}
    trainer = {"optimisers": {"opt": {"exp_avg": torch.randn(32, generator=g), "exp_avg_sq": torch.rand(32, generator=g),
                                      "steps": [3, 3, 0], "lr": 1e-3}},
               "cm_weight": 10.0, "ema": None, "fixed_caps": (128, None),
               "rng": {"cpu": [torch.get_rng_state()], "seed_offset": [5]}}
    return ck.pack(sd, trainer, _signature(), extra)


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and (a == b or (a != a and b != b))


def test_checkpoint_py_file_reads_back_with_weights_only(tmp_path):
    path = tmp_path / "c.pt"
    blob = _blob(extra={"epoch": 3, "history": [{"ausum": float("nan"), "loss": 0.5, "weights": "ema"}], "best": {"arena": torch.arange(4.0)}})
    ck.write(blob, path)
    raw = torch.load(path, map_location="cpu", weights_only=True)          # the plain reader, without the module
    assert raw["format"] == 1 and set(raw) == set(ck.KEYS)
    got = ck.read(path)
    assert _same(got, blob)
    assert got["trainer"]["fixed_caps"] == [128, None]                     # (tuples are stored as lists)
    assert got["extra"]["history"][0]["ausum"] != got["extra"]["history"][0]["ausum"]


def test_checkpoint_py_pack_refuses_what_weights_only_cannot_read():
    with pytest.raises(TypeError, match="extra"):
        ck.pack({}, {}, _signature(), extra={"fn": len})
    with pytest.raises(TypeError, match="extra must be a dict"):
        ck.pack({}, {}, _signature(), extra=[1, 2])


def test_checkpoint_py_write_is_atomic(tmp_path, monkeypatch):
    path = tmp_path / "c.pt"
    ck.write(_blob(seed=1), path)
    before = path.read_bytes()

    def broken_save(obj, f, *a, **kw):
        f.write(b"half a file")
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", broken_save)
    with pytest.raises(OSError, match="disk full"):
        ck.write(_blob(seed=2), path)
    monkeypatch.undo()
    assert path.read_bytes() == before                                     # the earlier file: byte-identical
    assert os.listdir(tmp_path) == ["c.pt"]                                # and no temporary file left behind
    assert _same(ck.read(path), _blob(seed=1))
    # a failed FIRST write leaves nothing at all
    monkeypatch.setattr(torch, "save", broken_save)
    with pytest.raises(OSError):
        ck.write(_blob(), tmp_path / "d.pt")
    assert os.listdir(tmp_path) == ["c.pt"]


def test_checkpoint_py_read_refuses_unknown_formats_and_broken_files(tmp_path):
    path = tmp_path / "c.pt"
    blob = _blob()
    blob["format"] = 2
    ck.write(blob, path)
    with pytest.raises(RuntimeError, match="format 2"):
        ck.read(path)
    torch.save({"state_dict": {}}, path)
    with pytest.raises(RuntimeError, match="not a trainer checkpoint"):
        ck.read(path)
    ck.write(_blob(), path)
    data = path.read_bytes()
    path.write_bytes(data[:len(data) // 2])
    with pytest.raises(RuntimeError, match="cannot be read"):
        ck.read(path)


def test_scheduler_state_round_trip_gives_the_same_next_learning_rates():
    from druglamp_amd.trainer import CosineAnnealingWarmupRestarts
    a = CosineAnnealingWarmupRestarts(10, 1e-3, 1e-8, 2)
    for _ in range(7):
        a.step()
    blob = ck.pack({}, {"schedulers": {"opt": a.state()}}, _signature())
    b = CosineAnnealingWarmupRestarts(10, 1e-3, 1e-8, 2)
    b.load_state(blob["trainer"]["schedulers"]["opt"])
    assert (b.step_in_cycle, b.cycle, b.lr) == (a.step_in_cycle, a.cycle, a.lr) == (7, 0, a.lr)
    nxt_a, nxt_b = [a.step() for _ in range(5)], [b.step() for _ in range(5)]          # (crosses the restart at step 10)
    assert nxt_a == nxt_b and a.cycle == b.cycle == 1 and len(set(nxt_a)) == 5


def test_checkpoint_py_signature_comparison_names_the_first_differing_field():
    saved = _signature()
    assert ck.compare_signatures(saved, _signature()) == (None, [])
    # a signature that went through a file holds lists where the trainer's may hold tuples
    assert ck.compare_signatures(saved, _signature(fixed_caps=None, optimisers=("opt", "opt_ssl"))) == (None, [])

    renamed = _signature()
    renamed["params"][1][0] = "a.offset"
    err, _ = ck.compare_signatures(saved, renamed)
    assert "parameter 1 is named 'a.bias' in the file and 'a.offset' here" in err

    reshaped = _signature()
    reshaped["params"][2][1] = [5, 4]
    err, _ = ck.compare_signatures(saved, reshaped)
    assert "parameter 'b.weight' has shape (5, 3) in the file and (5, 4) here" in err

    moved = _signature()
    moved["params"][2][2] = 20
    err, _ = ck.compare_signatures(saved, moved)
    assert "'b.weight' sits at arena offset 16 in the file and 20 here" in err

    err, _ = ck.compare_signatures(saved, _signature(world=2))
    assert "world size is 1 in the file and 2 here" in err

    # the FIRST difference in the order of MUST_MATCH: the model's class comes before the parameters and the world size
    both = _signature(world=2, model="DrugLAMPwoLLM")
    both["params"][0][0] = "x"
    err, _ = ck.compare_signatures(saved, both)
    assert "the file holds a DrugLAMP, the trainer a DrugLAMPwoLLM" in err and "world" not in err

    err, _ = ck.compare_signatures(saved, _signature(ema={"on": False, "decay": None, "warmup": None}))
    assert "weight EMA is on in the file and off here" in err
    regrouped = _signature()
    regrouped["param_groups"][1][1] = "default"
    err, _ = ck.compare_signatures(saved, regrouped)
    assert "parameter-group assignment: entry 1" in err and "no_decay" in err
    err, _ = ck.compare_signatures(saved, _signature(param_groups=None))
    assert "parameter groups are on in the file and off here" in err

    with pytest.raises(RuntimeError, match="world size is 1 in the file and 2 here"):
        ck.validate({"signature": saved}, _signature(world=2))


def test_checkpoint_py_graph_steps_and_fixed_caps_only_warn():
    saved = _signature()
    err, notes = ck.compare_signatures(saved, _signature(graph_steps=True, fixed_caps=[128, 4096]))
    assert err is None and len(notes) == 2
    assert any("graph_steps is False in the file and True here" in n for n in notes)
    assert any("fixed_caps" in n for n in notes)
    assert ck.validate({"signature": saved}, _signature(graph_steps=True)) == ["graph_steps is False in the file and True here"]
