"""Parameter groups in the training step (Trainer(param_groups=...)): the default trainer untouched, a neutral group bit-equal to
it, real groups (no decay for vectors, encoders at a tenth of the learning rate, a frozen adaptor) pinned per parameter against
the ungrouped optimiser entry points, eager against hipGraph-replayed steps, a runtime change, and freezing's effect on the
rest of the model.  Small-model pattern of tests/test_cls_loss_step_gpu.py: make_batch(8), PMMA dropout off, trainers from one
seed.

The per-parameter reference: for every parameter that received a gradient, ops.adamw_step / ops.adamw_step_guarded on clones
of its (arena, flat.grads, exp_avg, exp_avg_sq) slices from BEFORE the step, with lr = float32(optimiser lr) * float32(lr_scale)
and the weight decay of the parameter's group — bit for bit what the one grouped launch per run must leave (the kernel's bit
contract, tests/test_adamw_groups_gpu.py), so no tolerance appears."""
import numpy as np
import pytest
import torch

from tests import grad_guard_ref as gr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ADAPTOR = "p_adaptor_wo_skip_connect."


def _groups():
    """The frozen adaptor comes first: the first matching group wins, and its biases / norm weights are frozen with it."""
    from druglamp_amd.param_groups import ParamGroup
    return [ParamGroup("adaptor", match=(ADAPTOR + "*",), frozen=True),
            ParamGroup("no_decay", max_ndim=1, weight_decay=0.0),
            ParamGroup("encoders", match=("drug_extractor.*", "protein_extractor.*"), lr_scale=0.1)]


def _make(dtype, graph=False, seed=4321, pre=None, **kw):
    from druglamp_amd import ops
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.trainer import Trainer
    torch.manual_seed(seed)
    ops.manual_seed(77)
    ops.seed_offset_tensor(DEV).zero_()
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    model = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    model.pmma.p_drop = 0.0
    model.pmma.embeddings.p_drop = 0.0
    if pre is not None:
        pre(model)
    tr = Trainer(model, cfg, device=DEV, compute_dtype=dtype, graph_steps=graph, **kw)
    tr.set_lrs(1e-3, 2e-3, 3e-3)
    return tr


def _batch(dtype, seed=7, n=8):
    from druglamp_amd.synthetic import make_batch
    return make_batch(n, DEV, seed=seed, with_graph=True, llm_dtype=dtype)


def _bits(t):
    return t.view(torch.int32)


def _state(tr):
    return tr.flat.arena.clone(), tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone()


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _span(tr, i):
    s = tr.flat.offsets[i]
    return s, s + (tr.flat.params[i].numel() + 3) // 4 * 4


def _live(tr):
    return [i for i, p in enumerate(tr.flat.params) if p.grad is not None]


def _snapshot(tr, opts):
    return tr.flat.arena.clone(), {name: (getattr(tr, name).exp_avg.clone(), getattr(tr, name).exp_avg_sq.clone()) for name in opts}


def _reference(tr, snap, opts, guard=None):
    """Advances the snapshot (taken before the step) in place by per-parameter ungrouped optimiser calls, the step's optimisers
    in the step's order; returns (arena, {optimiser: (exp_avg, exp_avg_sq)}) to compare with the trainer's state after it."""
    from druglamp_amd import ops
    arena, moments = snap
    values = [tr.param_groups.values(g) for g, _, _ in tr.param_group_table()]
    for name in opts:
        opt = getattr(tr, name)
        m, v = moments[name]
        for i in _live(tr):
            s, e = _span(tr, i)
            scale, wd = values[i]
            kw = dict(lr=float(np.float32(opt.lr) * np.float32(scale)), beta1=opt.betas[0], beta2=opt.betas[1], eps=opt.eps,
                      weight_decay=wd, step=opt.steps[i], grad_scale=1.0)
            if guard is None:
                ops.adamw_step(arena[s:e], tr.flat.grads[s:e], m[s:e], v[s:e], **kw)
            else:
                ops.adamw_step_guarded(arena[s:e], tr.flat.grads[s:e], m[s:e], v[s:e], guard, **kw)
    return arena, moments


def _assert_matches(tr, ref, opts, what):
    arena, moments = ref
    assert torch.equal(_bits(arena), _bits(tr.flat.arena)), (what, "arena")
    for name in opts:
        opt = getattr(tr, name)
        assert torch.equal(_bits(moments[name][0]), _bits(opt.exp_avg)), (what, name, "exp_avg")
        assert torch.equal(_bits(moments[name][1]), _bits(opt.exp_avg_sq)), (what, name, "exp_avg_sq")


def _count(monkeypatch, names):
    from druglamp_amd import ops
    calls = []
    for name in names:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    return calls


def test_off_means_untouched(monkeypatch):
    from druglamp_amd import ops
    calls = _count(monkeypatch, ["adamw_step_groups", "adamw_step"])
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        for kw in ({}, {"param_groups": None}, {"param_groups": []}):
            tr = _make(dtype, **kw)
            for _ in range(3):
                tr.training_step(batch, meta=meta, cur_epoch=1)
            tr.check_device_flags()
            assert tr.param_groups is None and tr.opt.groups is None
            with pytest.raises(RuntimeError, match="parameter groups are off"):
                tr.param_group_table()
            with pytest.raises(RuntimeError, match="parameter groups are off"):
                tr.set_param_group("default", lr_scale=0.5)
        assert "adamw_step_groups" not in calls and calls.count("adamw_step") >= 9
        del calls[:]
        tr = _make(dtype, param_groups=_groups())            # the probe works: the feature, when on, goes through the new entry point
        tr.training_step(batch, meta=meta, cur_epoch=1)
        tr.check_device_flags()
        assert "adamw_step" not in calls and calls.count("adamw_step_groups") >= 1
    finally:
        ops.use_seed_offset(False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_neutral_group_changes_no_bit(dtype):
    from druglamp_amd import ops
    from druglamp_amd.param_groups import ParamGroup
    batch, meta = _batch(dtype)
    res = []
    try:
        for kw in ({}, {"param_groups": [ParamGroup("all", match=("*",), weight_decay=1e-2)]}):
            tr = _make(dtype, **kw)
            for _ in range(3):
                tr.training_step(batch, meta=meta, cur_epoch=1)
            tr.check_device_flags()
            res.append(_state(tr))
        assert {g for g, _, _ in tr.param_group_table()} == {"all"}
    finally:
        ops.use_seed_offset(False)
    assert _same(res[0], res[1])
    assert all(bool(torch.isfinite(t).all()) for t in res[1]) and float(res[1][1].abs().max()) > 0


def _freeze_adaptor(model):
    for n, p in model.named_parameters():
        if n.startswith(ADAPTOR):
            p.requires_grad_(False)


def test_real_groups_with_a_clipping_guard_per_parameter(monkeypatch):
    from druglamp_amd import ops
    calls = _count(monkeypatch, ["adamw_step_groups", "adamw_step_guarded"])
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, param_groups=_groups(), max_grad_norm=1e-3, ema_decay=0.9)
        names = [n for n, _ in tr.model.named_parameters()]
        table = tr.param_group_table()
        assert [n for _, n, _ in table] == names
        frozen = [i for i, (g, _, _) in enumerate(table) if g == "adaptor"]
        assert [names[i] for i in frozen] == [n for n in names if n.startswith(ADAPTOR)] and len(frozen) == 6
        assert all(not tr.flat.params[i].requires_grad for i in frozen)
        assert sum(p.requires_grad for p in tr.flat.params) == len(names) - 6
        by = dict((n, g) for g, n, _ in table)
        assert by["protein_extractor.conv1.weight"] == "encoders" and by["protein_extractor.conv1.bias"] == "no_decay"
        assert by["mlp_classifier.fc1.weight"] == "default"
        start = _state(tr)
        shadow0 = tr.ema.shadow.clone()
        for i in frozen:                                     # what a norm over the WHOLE buffer would pick up
            s, e = _span(tr, i)
            tr.flat.grads[s:e] = 1e3
        per_step = []
        for k in (1, 2, 3):
            snap = _snapshot(tr, ["opt"])
            del calls[:]
            out = tr.training_step(batch, meta=meta, cur_epoch=1)
            per_step.append(list(calls))
            live = _live(tr)
            assert live and not (set(live) & set(frozen)) and all(tr.flat.params[i].grad is None for i in frozen)
            assert all(tr.opt.steps[i] == k for i in live) and all(tr.opt.steps[i] == 0 for i in frozen)
            guard = tr.grad_guard.guard.clone()
            ref = _reference(tr, snap, ["opt"], guard)
            _assert_matches(tr, ref, ["opt"], "step %d" % k)
            want = np.sqrt(gr.sqnorm(torch.cat([tr.flat.grads[slice(*_span(tr, i))] for i in live])))
            got = float(out["grad_norm"])
            print("step", k, "grad_norm", got, "fp64 over the live gradient", want)
            assert abs(got - want) <= float(gr.ulp32(want))
            st = tr.grad_guard_stats()
            assert 0.0 < st["coef"] < 1.0 and st["clipped"] == k and st["skipped"] == 0
        tr.check_device_flags()
        end = _state(tr)
        for i in frozen:
            s, e = _span(tr, i)
            for a, b, what in zip(start, end, ("arena", "exp_avg", "exp_avg_sq")):
                assert torch.equal(_bits(a[s:e]), _bits(b[s:e])), (names[i], what)
            assert torch.equal(_bits(shadow0[s:e]), _bits(tr.ema.shadow[s:e])), (names[i], "EMA shadow")
            assert float(end[1][s:e].abs().max()) == 0.0 and float(end[2][s:e].abs().max()) == 0.0
        moved = [i for i in _live(tr) if not torch.equal(start[0][slice(*_span(tr, i))], end[0][slice(*_span(tr, i))])]
        assert len(moved) > 0.9 * len(_live(tr))           # (a vector without decay whose gradient is exactly zero stays put)
        assert not torch.equal(shadow0, tr.ema.shadow)
        # the launch count: an ungrouped trainer whose adaptor was frozen by hand forms the same runs
        plain = _make(dtype, pre=_freeze_adaptor, max_grad_norm=1e-3, ema_decay=0.9)
        plain_steps = []
        for k in (1, 2, 3):
            del calls[:]
            plain.training_step(batch, meta=meta, cur_epoch=1)
            plain_steps.append(list(calls))
        assert _live(plain) == _live(tr)
    finally:
        ops.use_seed_offset(False)
    for a, b in zip(per_step, plain_steps):
        assert set(a) == {"adamw_step_groups"} and set(b) == {"adamw_step_guarded"} and len(a) == len(b) >= 1
    print("optimiser launches per step:", [len(a) for a in per_step])


def test_an_ssl_epoch_step_and_eager_against_replayed_steps():
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    res = {}
    try:
        tr = _make(dtype, param_groups=_groups(), max_grad_norm=1e-3)
        assert tr.use_ssl and 5 % tr.ssl_epoch_step == 0
        opts = ["opt", "opt_ssl"] + (["opt_cm"] if (tr.use_cm and 5 >= tr.cm_init_epoch) else [])
        snap = _snapshot(tr, opts)
        out = tr.training_step(batch, meta=meta, cur_epoch=5)
        assert "ssl" in out and ("cm" in out) == ("opt_cm" in opts)
        assert tr.opt_ssl.groups is tr.opt.groups and tr.opt.groups is tr.param_groups      # one table for the optimisers
        ref = _reference(tr, snap, opts, tr.grad_guard.guard.clone())
        _assert_matches(tr, ref, opts, "SSL-epoch step")
        assert float(tr.opt_ssl.exp_avg.abs().max()) > 0
        tr.check_device_flags()
        for graph in (False, True):
            tr = _make(dtype, graph=graph, param_groups=_groups(), max_grad_norm=1e-3)
            tr.fixed_caps = tr.fixed_caps_for([(batch, meta)])
            states = []
            for _ in range(4):                               # 2 eager warm-up steps, then the capture and 2 replays
                tr.training_step(batch, meta=meta, cur_epoch=1)
                states.append(_state(tr))
            tr.check_device_flags()
            res[graph] = (states, sum(g_.replays for g_ in tr._graphs.values()), tr.grad_guard_stats())
    finally:
        ops.use_seed_offset(False)
    assert res[True][1] == 2 and res[False][1] == 0
    for k, (a, b) in enumerate(zip(res[False][0], res[True][0])):
        assert _same(a, b), "state after step %d" % (k + 1)
    assert res[False][2] == res[True][2]
    assert not torch.equal(res[True][0][2][0], res[True][0][3][0])


def test_a_runtime_change_takes_effect_on_the_next_step():
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, param_groups=_groups())
        twin = _make(dtype, param_groups=_groups())
        for t in (tr, twin):
            t.training_step(batch, meta=meta, cur_epoch=1)
        assert _same(_state(tr), _state(twin))
        tr.set_param_group("encoders", lr_scale=0.5, weight_decay=0.05)
        tr.set_param_group("default", weight_decay=0.0)
        assert tr.param_groups.values("encoders") == (0.5, 0.05) and tr.param_groups.values("default") == (1.0, 0.0)
        assert tr.param_groups.group_tab.tolist()[3] == [0.5, float(np.float32(0.05))]
        snap = _snapshot(tr, ["opt"])
        for t in (tr, twin):
            t.training_step(batch, meta=meta, cur_epoch=1)
        _assert_matches(tr, _reference(tr, snap, ["opt"]), ["opt"], "the step after set_param_group")
        assert not torch.equal(tr.flat.arena, twin.flat.arena)          # ... and it differs from the unchanged twin
        tr.check_device_flags()
        keep = tr.param_groups.group_tab.clone()
        with pytest.raises(ValueError, match="no group named 'encoder'"):
            tr.set_param_group("encoder", lr_scale=0.5)
        for bad in (-0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite number >= 0"):
                tr.set_param_group("encoders", lr_scale=bad)
            with pytest.raises(ValueError, match="finite number >= 0"):
                tr.set_param_group("encoders", weight_decay=bad)
        assert torch.equal(keep, tr.param_groups.group_tab)
    finally:
        ops.use_seed_offset(False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_freezing_does_not_disturb_the_gradients_of_the_rest(dtype):
    """First step from one seed: every trainable parameter's gradient is torch.equal between a trainer with the frozen adaptor
    and one without groups.  Measured on the MI355X at fp32 and bf16: no parameter differs (the frozen adaptor's inputs carry no
    gradient, so its whole backward drops out and no grouped weight-gradient launch loses a member) — the assertion is the
    strict one, no launch is named and no margin is granted."""
    from druglamp_amd import ops
    batch, meta = _batch(dtype)
    grads = []
    try:
        for kw in ({"param_groups": _groups()}, {}):
            tr = _make(dtype, **kw)
            tr.fixed_caps = tr.fixed_caps_for([(batch, meta)])
            tr.training_step(batch, meta=meta, cur_epoch=1)
            tr.check_device_flags()
            grads.append({n: (None if p.grad is None else p.grad.clone()) for n, p in tr.model.named_parameters()})
    finally:
        ops.use_seed_offset(False)
    fr, un = grads
    assert all(fr[n] is None and un[n] is not None for n in fr if n.startswith(ADAPTOR))
    live = [n for n in fr if fr[n] is not None]
    assert live == [n for n in un if un[n] is not None and not n.startswith(ADAPTOR)] and len(live) > 100
    differ = [n for n in live if not torch.equal(fr[n], un[n])]
    for n in differ:
        print("differs:", n, float((fr[n].double() - un[n].double()).norm() / un[n].double().norm()))
    assert differ == []
