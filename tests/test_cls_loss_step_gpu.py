"""The classification loss in the step (Trainer(cls_loss=...), cls_loss.classification_loss): the gradients it sends through the
model against the same formula in torch fp32 ops on one forward graph, eager against hipGraph-replayed steps with per-sample
weights that change every step, the default trainer untouched, and bad weights / labels.
Small-model pattern of tests/test_trainer_ema_gpu.py: make_batch(8), PMMA dropout off, two trainers from one seed.

The gradient comparison runs at compute dtype fp32.  Its bar is relative to the distance between two torch formulations of
the neutral loss, which differ by a few fp32 roundings of d loss / d score; at compute dtype bf16 the score's gradient is
rounded to bf16 on either side, a tie that falls the other way is one bf16 ulp (2^-8) of an element, and no bar derived from
fp32 roundings means anything there (the bf16 store is pinned element by element in tests/test_cls_loss_paths_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U_F = 2.0 ** -24


def _make(dtype, n_class=1, graph=False, seed=4321, **kw):
    from druglamp_amd import ops
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.trainer import Trainer
    torch.manual_seed(seed)
    ops.manual_seed(77)
    ops.seed_offset_tensor(DEV).zero_()
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    cfg["DECODER"]["BINARY"] = n_class
    model = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    model.pmma.p_drop = 0.0
    model.pmma.embeddings.p_drop = 0.0
    tr = Trainer(model, cfg, device=DEV, compute_dtype=dtype, graph_steps=graph, **kw)
    tr.set_lrs(1e-3, 1e-3, 1e-3)
    return tr


def _batch(dtype, seed=7, n=8):
    from druglamp_amd.synthetic import make_batch
    return make_batch(n, DEV, seed=seed, with_graph=True, llm_dtype=dtype)


def _with_weights(meta, ws):
    return [dict(m_, Weight=float(w)) for m_, w in zip(meta, ws)]


def _bits(t):
    return t.view(torch.int32)


def _state(tr):
    return tr.flat.arena.clone(), tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone()


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _torch_formula(score, labels, spec, w):
    """The issue's formula in torch fp32 ops on the classifier's score."""
    s = score.float()
    z = s[:, 0] if s.shape[1] == 1 else s[:, 1] - s[:, 0]
    y = labels.reshape(-1).float()
    p, q = torch.sigmoid(z), torch.sigmoid(-z)
    d = (y * q - (1 - y) * p).abs()
    m = d ** spec.gamma if spec.gamma != 0 else torch.ones_like(d)
    B = spec.pos_weight * y * F.softplus(-z) + spec.neg_weight * (1 - y) * F.softplus(z)
    ww = torch.ones_like(z) if w is None else w
    return (ww * m * B).sum() / (ww.sum() if w is not None else z.numel())


def _flat_grad(loss, params):
    gs = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
    return torch.cat([g.reshape(-1).double() for g in gs if g is not None]), [g is not None for g in gs]


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("n_class", [1, 2])
def test_gradients_through_the_model_against_the_torch_formula_on_one_graph(n_class):
    from druglamp_amd import ops
    from druglamp_amd.cls_loss import ClsLoss, classification_loss
    from druglamp_amd.model.basic_model import binary_cross_entropy, cross_entropy_logits
    dtype = torch.float32
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, n_class=n_class)
        m = tr.model
        m.train()
        feat_d, feat_p, labels, llm_d, llm_p = batch
        _, _, _, _, score = m(feat_d, feat_p, llm_d, llm_p, hints=tr.hints_of(meta, batch))      # ONE forward: same activations, same masks
        assert score.shape == (8, n_class)
        params = [p for p in m.parameters() if p.requires_grad]
        # the yardstick: two torch formulations of the neutral loss on this graph
        z = score.float().squeeze(1) if n_class == 1 else score.float()[:, 1] - score.float()[:, 0]
        _, default = binary_cross_entropy(score, labels) if n_class == 1 else cross_entropy_logits(score, labels)
        ga, used_a = _flat_grad(default, params)
        gb, used_b = _flat_grad(F.binary_cross_entropy_with_logits(z, labels.float().reshape(-1)), params)
        assert used_a == used_b and ga.numel() > 1_000_000
        r0 = _rel(ga, gb)
        bar = 8.0 * max(r0, U_F)
        w = torch.tensor([0.5, 2.0, 1.0, 0.0, 3.0, 1.5, 0.25, 1.0], dtype=torch.float32, device=DEV)
        for name, spec, ww in (("neutral", ClsLoss(), None), ("pos_weight=3", ClsLoss(pos_weight=3.0), None),
                               ("focal(0.25, 2) weighted", ClsLoss.focal(0.25, 2.0), w)):
            _, lk = classification_loss(score, labels, spec, ww)
            lt = _torch_formula(score, labels, spec, ww)
            gk, used_k = _flat_grad(lk, params)
            gt, used_t = _flat_grad(lt, params)
            assert used_k == used_t == used_a
            measure = _rel(gk, gt)
            print("n_class %d  %-24s rel L2 of the flat gradient %.3e   r0 %.3e   bar %.3e   |loss kernel - torch| %.3e"
                  % (n_class, name, measure, r0, bar, abs(float(lk.detach()) - float(lt.detach()))))
            assert bool(torch.isfinite(gk).all()) and float(gt.norm()) > 0
            assert measure <= bar, (name, measure, r0)
        ops.check_guard_flags(DEV)
    finally:
        ops.use_seed_offset(False)


def test_replayed_steps_with_changing_weights_equal_eager_ones_bit_for_bit():
    from druglamp_amd import ops
    from druglamp_amd.cls_loss import ClsLoss
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    g = torch.Generator().manual_seed(3)
    metas = [_with_weights(meta, (torch.rand(8, generator=g) * 3).tolist()) for _ in range(5)]
    res = {}
    try:
        for graph in (False, True):
            tr = _make(dtype, graph=graph, cls_loss=ClsLoss.focal(0.25, 2.0))
            tr.fixed_caps = tr.fixed_caps_for([(batch, meta)])
            arenas, losses = [], []
            for mt in metas:                                     # 2 eager warm-up steps, then the capture and 3 replays
                out = tr.training_step(batch, meta=mt, cur_epoch=1)
                arenas.append(tr.flat.arena.clone())
                losses.append(out["cls"].clone())
            tr.check_device_flags()
            res[graph] = (arenas, losses, sum(g_.replays for g_ in tr._graphs.values()), _state(tr))
    finally:
        ops.use_seed_offset(False)
    assert res[True][2] == 3 and res[False][2] == 0
    for k, (a, b) in enumerate(zip(res[False][0], res[True][0])):
        assert torch.equal(_bits(a), _bits(b)), "arena after step %d" % (k + 1)
    for k, (a, b) in enumerate(zip(res[False][1], res[True][1])):
        assert torch.equal(_bits(a.reshape(1)), _bits(b.reshape(1))) and bool(torch.isfinite(a)), "loss of step %d" % (k + 1)
    assert _same(res[False][3], res[True][3])
    assert len({float(l) for l in res[True][1][2:]}) == 3         # the replays saw three different weight vectors


def test_graphs_with_and_without_weights_are_keyed_apart():
    from druglamp_amd import ops
    from druglamp_amd.cls_loss import ClsLoss
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    mw = _with_weights(meta, [1.0, 2.0, 0.5, 1.0, 0.0, 3.0, 1.0, 1.0])
    try:
        tr = _make(dtype, graph=True, cls_loss=ClsLoss(pos_weight=3.0))
        tr.fixed_caps = tr.fixed_caps_for([(batch, meta)])
        for _ in range(3):
            tr.training_step(batch, meta=mw, cur_epoch=1)
        assert tr.graph_captures == 1 and next(iter(tr._graphs.values())).weights is not None
        tr.training_step(batch, meta=meta, cur_epoch=1)          # no weights: not the captured body — an eager step of another key
        assert tr.graph_captures == 1 and sum(g_.replays for g_ in tr._graphs.values()) == 1
        tr.check_device_flags()
    finally:
        ops.use_seed_offset(False)


def test_the_default_trainer_is_untouched(monkeypatch):
    from druglamp_amd import ops
    from druglamp_amd.cls_loss import ClsLoss
    calls = []
    real_fwd, real_bwd = ops.cls_loss_fwd, ops.cls_loss_bwd
    monkeypatch.setattr(ops, "cls_loss_fwd", lambda *a, **k: (calls.append("fwd"), real_fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "cls_loss_bwd", lambda *a, **k: (calls.append("bwd"), real_bwd(*a, **k))[1])
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    mw = _with_weights(meta, [2.0] * 8)                          # weights in meta mean nothing to a trainer without cls_loss
    res = []
    try:
        for kw, mt, graph in (({}, meta, False), ({"cls_loss": None}, mw, False), ({}, mw, True)):
            tr = _make(dtype, graph=graph, **kw)
            tr.fixed_caps = tr.fixed_caps_for([(batch, meta)])
            for _ in range(4):
                tr.training_step(batch, meta=mt, cur_epoch=1)
            tr.check_device_flags()
            assert tr.cls_loss is None and all(g_.weights is None for g_ in tr._graphs.values())
            res.append(_state(tr))
        assert calls == []                                       # no dl_cls_loss_* call, eager or captured
        assert _same(res[0], res[1]) and _same(res[0], res[2])
        tr = _make(dtype, cls_loss=ClsLoss())                    # the probe works: the feature, when on, goes through both entry points
        tr.training_step(batch, meta=meta, cur_epoch=1)
        tr.check_device_flags()
        assert calls == ["fwd", "bwd"]
    finally:
        ops.use_seed_offset(False)


def test_a_negative_weight_in_meta_surfaces_through_check_device_flags():
    from druglamp_amd import ops
    from druglamp_amd.cls_loss import ClsLoss
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, cls_loss=ClsLoss.focal(0.25, 2.0))
        out = tr.training_step(batch, meta=_with_weights(meta, [1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0, 1.0]), cur_epoch=1)
        assert bool(torch.isnan(out["cls"]))
        with pytest.raises(RuntimeError, match="classification loss guard tripped — FLAG_CLS_LABEL"):
            tr.check_device_flags()
        tr.check_device_flags()                                  # cleared
    finally:
        ops.guard_flags(DEV).zero_()
        ops.cls_loss_flags(DEV).zero_()
        ops.use_seed_offset(False)


def test_a_bad_label_on_a_skipping_trainer_is_reported_by_the_next_steps_poll():
    """skip_nonfinite skips the poisoned step (parameters keep their bits); the guard word still tells: not silent."""
    from druglamp_amd import ops
    from druglamp_amd.cls_loss import ClsLoss
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, cls_loss=ClsLoss(pos_weight=3.0), skip_nonfinite=True)
        before = tr.flat.arena.clone()
        labels = batch[2].clone()
        labels[2] = 2.0
        out = tr.training_step(batch[:2] + (labels,) + batch[3:], meta=meta, cur_epoch=1)
        torch.cuda.synchronize()                                 # (the posted copy of the words has landed)
        assert bool(torch.isnan(out["cls"])) and torch.equal(_bits(before), _bits(tr.flat.arena))
        with pytest.raises(RuntimeError, match="classification loss guard tripped in an earlier step — FLAG_CLS_LABEL"):
            tr.training_step(batch, meta=meta, cur_epoch=1)
        tr.training_step(batch, meta=meta, cur_epoch=1)          # cleared: training goes on
        tr.check_device_flags()
    finally:
        ops.guard_flags(DEV).zero_()
        ops.cls_loss_flags(DEV).zero_()
        ops.use_seed_offset(False)


def test_weights_on_only_some_entries_raise_before_anything_runs():
    from druglamp_amd import ops
    from druglamp_amd.cls_loss import ClsLoss
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    some = [dict(m_, Weight=1.0) if k % 2 else dict(m_) for k, m_ in enumerate(meta)]
    try:
        tr = _make(dtype, cls_loss=ClsLoss(pos_weight=3.0))
        before = _state(tr)
        with pytest.raises(ValueError, match="all of them or none"):
            tr.training_step(batch, meta=some, cur_epoch=1)
        with pytest.raises(ValueError, match="weights for a batch"):
            tr.training_step(batch, meta=_with_weights(meta, [1.0] * 8)[:5], cur_epoch=1)
        assert _same(before, _state(tr))
    finally:
        ops.use_seed_offset(False)
