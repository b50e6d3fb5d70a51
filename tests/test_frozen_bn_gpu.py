"""Frozen-BatchNorm fine-tuning and input gradients of a deployed model: the eval-mode BatchNorm backward (dl_bn_eval_bwd)
through BatchNormRowsFn, ProteinCNNFn, MolecularGCN, the whole model, Trainer(freeze_bn=True) and model.eval() + backward,
against torch fp64 autograd of the oracle with bn_training=False.

Measures and bounds (from tests/test_parity_gpu.py, not new): outputs by helpers.relerr at F32_TOL = 1e-4; fp32 gradients by
the relative L2 error per parameter, ||got - ref|| <= 10 F32_TOL max(||ref||, 1e-4) — the bound check_gradnorms puts on the
NORMS there, here on the difference itself (which bounds the difference of the norms); parameters whose gradient is
analytically zero (key-projection biases, the MHLA gate bias: softmax shift invariance) against the largest norm, as there.
bf16: the cosine of the whole gradient vector >= 0.98 (the floor of the bf16 whole-model leg, tests/test_model_gpu.py).
The oracle's whole-model pass (fp64 autograd on the host, batch 4) is computed once and shared.  ReLU kink: as in
tests/test_norm_paths_gpu.py a ReLU whose fp64 pre-activation is within 64 u_f of zero (relative to its terms) may open on one
side only; in the whole-model reference those ProteinCNN elements follow the kernels' side (_protein_cnn_agreed).
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import load, model_inputs, relerr
from tests.test_parity_gpu import BF16_TOL, F32_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16_COS = 0.98


def rel_l2(got, ref, scale=None):
    got, ref = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    return float((got - ref).norm()) / max(float(ref.norm()) if scale is None else scale, 1e-4)


def _zero_grad_param(k):
    return k.endswith(("key.bias", "key_mol.bias", "lin2.bias", "in_proj_bias"))


# ---- BatchNormRowsFn ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
def test_batch_norm_rows_eval_mode_backward_against_fp64_autograd(relu):
    """Fails on the parent commit: 'eval-mode backward is not implemented'."""
    from druglamp_amd.functional import BatchNormRowsFn
    g = torch.Generator().manual_seed(11)
    R, C = 37, 128
    x = torch.randn(R, C, generator=g).to(DEV).requires_grad_(True)
    gamma = (1.0 + 0.5 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    beta = (0.5 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    rmean, rvar = (0.3 * torch.randn(C, generator=g)).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV)
    cot = torch.randn(R, C, generator=g).to(DEV)
    rm0, rv0 = rmean.clone(), rvar.clone()
    y, _, _ = BatchNormRowsFn.apply(x, gamma, beta, rmean, rvar, False, 1e-5, None, relu)
    (y * cot).sum().backward()
    xr, gr, br = (t.detach().double().requires_grad_(True) for t in (x, gamma, beta))
    yr = F.batch_norm(xr, rmean.double(), rvar.double(), gr, br, False, 0.1, 1e-5)
    if relu:
        yr = F.relu(yr)
    (yr * cot.double()).sum().backward()
    assert relerr(y, yr) <= F32_TOL
    for name, a, b in (("x", x, xr), ("gamma", gamma, gr), ("beta", beta, br)):
        assert rel_l2(a.grad, b.grad) <= 10 * F32_TOL, (name, rel_l2(a.grad, b.grad))
    assert torch.equal(rmean, rm0) and torch.equal(rvar, rv0)
    # all parameters frozen: the dx pass alone
    x2 = x.detach().clone().requires_grad_(True)
    y2, _, _ = BatchNormRowsFn.apply(x2, gamma.detach(), beta.detach(), rmean, rvar, False, 1e-5, None, relu)
    (y2 * cot).sum().backward()
    assert torch.equal(x2.grad, x.grad)


# ---- ProteinCNN --------------------------------------------------------------------------------------------------------------
def _protein_cnn():
    from druglamp_amd.model.basic_model import ProteinCNN
    torch.manual_seed(2)
    m = ProteinCNN(128, [128] * 3, [3, 6, 9]).to(DEV)
    with torch.no_grad():
        for bn in (m.bn1, m.bn2, m.bn3):
            bn.running_mean.normal_(0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.normal_(1.0, 0.3)
            bn.bias.normal_(0.0, 0.3)
    m.compute_dtype = torch.float32
    return m


def _freeze(m):
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.eval()
    return m


def test_protein_cnn_with_frozen_batchnorm_against_the_fp64_oracle():
    """Fails on the parent commit (the module passes its own training flag; the backward raises 'only implemented for
    training-mode BatchNorm' once the mode is taken from the BatchNorm modules)."""
    from oracle import druglamp_oracle as O
    from tests.test_protein_cnn_compact_gpu import _plan_dev, _tiled
    S, lengths = 2304, [98, 1022, 511]
    B = len(lengths)
    ids, fill = _tiled(B, S, lengths, seed=4)
    full = _freeze(_protein_cnn())
    comp = copy.deepcopy(full)
    proj = torch.randn(B, S // 9, 128, generator=torch.Generator().manual_seed(3)).to(DEV)
    bufs0 = {k: v.clone() for k, v in full.state_dict().items() if "running" in k or "num_batches" in k}
    outs = []
    for m, plan in ((full, None), (comp, _plan_dev(lengths, S))):
        z = m(ids, fill, site_pool=9, plan=plan)
        (z.float() * proj).sum().backward()
        outs.append(z.float())
        for k, v in bufs0.items():
            assert torch.equal(m.state_dict()[k], v), k                      # running statistics and counters: bitwise unchanged
    from druglamp_amd import ops
    ops.check_guard_flags(DEV)
    sd = {"p." + k: (v.detach().double().cpu().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.detach().cpu().double())
          for k, v in full.state_dict().items()}
    zr = O.protein_cnn(sd, "p", ids.cpu(), fill.double().cpu(), False)
    zr = zr.view(-1, 9, S // 9, zr.shape[-1]).mean(dim=1)
    (zr * proj.double().cpu()).sum().backward()
    assert relerr(outs[0], zr) <= F32_TOL and relerr(outs[1], zr) <= F32_TOL
    for (k, a), (_, b) in zip(full.named_parameters(), comp.named_parameters()):
        ref = sd["p." + k].grad
        assert rel_l2(a.grad, ref) <= 10 * F32_TOL, ("full", k, rel_l2(a.grad, ref))
        assert rel_l2(b.grad, ref) <= 10 * F32_TOL, ("compact", k, rel_l2(b.grad, ref))
        assert rel_l2(b.grad, a.grad) <= 10 * F32_TOL, ("compact vs full", k, rel_l2(b.grad, a.grad))


def test_protein_cnn_refuses_batchnorm_modules_in_different_modes():
    from tests.test_protein_cnn_compact_gpu import _tiled
    m = _protein_cnn().train()
    m.bn2.eval()
    ids, fill = _tiled(1, 2304, [98])
    with pytest.raises(ValueError, match="must all be in training mode or all in eval mode"):
        m(ids, fill, site_pool=9)


# ---- MolecularGCN ------------------------------------------------------------------------------------------------------------
def test_gcn_frozen_compact_padding_equals_the_512_row_computation():
    """The compact padding form needs no multiplicities with fixed statistics: same outputs and gradients as all 512 rows, at
    the fp32 tolerances of tests/test_model_gpu.py::test_gcn_compact_padding_equals_the_512_row_computation (2e-5, gradients
    20 x)."""
    from druglamp_amd.model.basic_model import MolecularGCN
    from druglamp_amd.synthetic import make_batch
    tol = 2e-5
    torch.manual_seed(1)
    ref = MolecularGCN(75, 128, True, [128] * 3).to(DEV)
    with torch.no_grad():
        for mod in ref.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_(0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
    ref.compute_dtype = torch.float32
    _freeze(ref)
    cmp_ = copy.deepcopy(ref)
    ref.compact_padding, cmp_.compact_padding = False, True
    cmp_.compact_min_rows = 0
    (feat_d, *_), _ = make_batch(6, DEV, seed=9, with_graph=True)
    h, adj = feat_d
    cot = torch.randn(6, 512, 128, generator=torch.Generator().manual_seed(5)).to(DEV)
    bufs0 = {k: v.clone() for k, v in ref.named_buffers()}
    outs = []
    for m in (ref, cmp_):
        o = m((h, adj))
        (o.float() * cot).sum().backward()
        outs.append(o)
        for k, v in m.named_buffers():
            assert torch.equal(v, bufs0[k]), k
    assert getattr(outs[1], "_dl_tail", None) is not None, "the compact form was not taken"
    assert relerr(outs[1].float(), outs[0].float()) <= tol
    for (n, a), (_, b) in zip(ref.named_parameters(), cmp_.named_parameters()):
        assert relerr(b.grad, a.grad) <= 20 * tol, n


# ---- the whole model ---------------------------------------------------------------------------------------------------------
KIND, BATCH = "DrugLAMP", 4


def _inputs():
    return model_inputs("modeltrain." + KIND, BATCH)


def _model(dtype=torch.float32):
    from tests.test_model_gpu import build
    return build(KIND, load("model_" + KIND), dtype=dtype)


KINK = 64 * 2.0 ** -24                       # the ReLU kink band of tests/test_norm_paths_gpu.py: |pre| <= 64 u_f (sum of |terms|)
KINK_CAP = 1e-3                              # at most 1 element in 1000 per tensor may sit in it (asserted), as there
agreed_kinks = []                            # per ProteinCNN layer of the last _oracle() run: elements taken from the kernels' side


def _protein_cnn_agreed(open_sets):
    """oracle.protein_cnn restated with ONE difference: a ReLU whose fp64 pre-activation lies in the kink band — where fp32
    cannot tell its sign (measured on this fixture: 4 of 1.18 M elements of layer 3 at |pre| / magnitude <= 2.7e-8 open on one
    side only, each worth 1 / sqrt(9216) of its channel's gradient: 4e-3 of conv3's, against 7e-5 with none) — takes the
    side the kernels took (open_sets: per layer the (B, C, S) set y > 0 of the GPU forward).  Both sides are correct
    evaluations of a function that is not differentiable there; everywhere else the fp64 sign holds, and a kernel that opened
    a ReLU wrongly outside the band would still be compared with the fp64 sign.  open_sets = None: the oracle's function
    itself (asserted equal in _oracle)."""
    def protein_cnn(sd, p, ids, fill, bn_training):
        from oracle.druglamp_oracle import _bn
        del agreed_kinks[:]
        v = F.embedding(ids.long(), sd[p + ".embedding.weight"], padding_idx=0)
        v = torch.cat((v, fill.unsqueeze(-1).to(v.dtype)), dim=-1).transpose(2, 1)
        for i in (1, 2, 3):
            w, b = sd["%s.conv%d.weight" % (p, i)], sd["%s.conv%d.bias" % (p, i)]
            pre = F.conv1d(v, w, b, padding="same")
            mask = pre > 0
            if open_sets is not None:
                with torch.no_grad():
                    mag = F.conv1d(v.abs(), w.abs(), b.abs(), padding="same")
                    band = pre.abs() <= KINK * mag
                    assert float(band.double().mean()) <= KINK_CAP, "layer %d: %g of the elements at the ReLU kink" % (i, float(band.double().mean()))
                    agreed_kinks.append(int((band & (mask != open_sets[i - 1])).sum()))
                    mask = torch.where(band, open_sets[i - 1], mask)
            v = _bn(sd, "%s.bn%d" % (p, i), pre * mask, bn_training)
        return v.reshape(v.size(0), v.size(2), -1)
    return protein_cnn


def _gpu_open_sets():
    """The sets y > 0 of the three ProteinCNN ReLUs in the GPU's fp32 forward of the shared inputs, as (B, C, S) host tensors."""
    from druglamp_amd import ops
    m, _ = _model()
    m.eval()
    rec, orig = [], ops.bn_apply_fwd

    def spy(y, *a, **k):
        rec.append(y)
        return orig(y, *a, **k)

    vd, vp, xd, xp, _y = (t.to(DEV) for t in _inputs())
    ops.bn_apply_fwd = spy
    try:
        with torch.no_grad():
            m(vd, vp, xd, xp)
    finally:
        ops.bn_apply_fwd = orig
    B, S = vp.shape
    ys = [t for t in rec if t.dim() == 2 and t.shape[0] == B * (S + 8)]
    assert len(ys) == 3, [tuple(t.shape) for t in rec]
    return [(t.reshape(B, S + 8, -1)[:, 4:4 + S].transpose(1, 2) > 0).cpu() for t in ys]


@functools.lru_cache(maxsize=None)
def _oracle():
    """fp64 autograd of the oracle's model_forward(..., bn_training=False) + BCE on the shared inputs: (loss, score, {parameter:
    gradient}, gradient of the protein LLM embedding).  With dropout off this is the frozen training forward AND the eval
    forward.  The ProteinCNN's ReLUs inside the kink band open as the kernels opened them (_protein_cnn_agreed)."""
    from oracle import druglamp_oracle as O
    m, _ = _model()
    vd, vp, xd, xp, y = _inputs()
    sd = {}
    for k, v in m.state_dict().items():
        v = v.detach().cpu()
        sd[k] = v.double().requires_grad_(True) if (v.dtype.is_floating_point and "running" not in k) else (v.double() if v.dtype.is_floating_point else v)
    for k in list(sd):                                         # one ProteinCNN under two names: one leaf
        if k.startswith("ssl_model.extractor."):
            sd[k] = sd["protein_extractor." + k[len("ssl_model.extractor."):]]
    with torch.no_grad():                                      # the restatement IS the oracle's function
        fill = O._fill_bit(xp.double())
        assert torch.equal(_protein_cnn_agreed(None)(sd, "protein_extractor", vp, fill, False), O.protein_cnn(sd, "protein_extractor", vp, fill, False))
    xp64 = xp.double().requires_grad_(True)
    own = O.protein_cnn
    O.protein_cnn = _protein_cnn_agreed(_gpu_open_sets())
    try:
        out = O.model_forward(sd, KIND, vd.double(), vp, xd.double(), xp64, bn_training=False)
    finally:
        O.protein_cnn = own
    assert len(agreed_kinks) == 3 and sum(agreed_kinks) <= 16, agreed_kinks
    print("ProteinCNN ReLUs taken from the kernels' side inside the kink band, per layer:", agreed_kinks)
    _, loss = O.bce_loss(out["score"], y.double())
    loss.backward()
    grads = {k: v.grad for k, v in sd.items() if torch.is_tensor(v) and v.requires_grad and v.grad is not None}
    return float(loss.detach()), out["score"].detach(), grads, xp64.grad


def _check_grads_fp32(m, grads):
    named = dict(m.named_parameters())
    scale = max(float(g.norm()) for g in grads.values())
    seen = 0
    for k, ref in grads.items():
        if k not in named or named[k].grad is None:
            continue
        seen += 1
        err = rel_l2(named[k].grad, ref, scale if _zero_grad_param(k) else None)
        assert err <= 10 * F32_TOL, (k, err)
    assert seen >= 100, seen
    for k in ("protein_extractor.bn1.weight", "protein_extractor.bn3.bias", "mlp_classifier.bn2.weight", "protein_extractor.conv1.weight"):
        assert k in grads and named[k].grad is not None, k


def test_whole_model_frozen_batchnorm_cls_backward_against_the_fp64_oracle():
    from druglamp_amd.model.basic_model import binary_cross_entropy
    loss_ref, score_ref, grads, _ = _oracle()
    m, _ = _model()
    m.freeze_batchnorm()
    m.train()
    assert m.training and not any(mod.training for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm1d))
    bufs0 = {k: v.clone() for k, v in m.named_buffers()}
    vd, vp, xd, xp, y = (t.to(DEV) for t in _inputs())
    m.zero_grad()
    out = m(vd, vp, xd, xp)
    _, loss = binary_cross_entropy(out[4], y)
    loss.backward()
    assert relerr(out[4], score_ref) <= F32_TOL
    assert abs(float(loss.detach()) - loss_ref) <= 1e-4
    _check_grads_fp32(m, grads)
    for k, v in m.named_buffers():
        assert torch.equal(v, bufs0[k]), k


def test_whole_model_frozen_batchnorm_bf16_gradient_direction():
    from druglamp_amd.model.basic_model import binary_cross_entropy
    loss_ref, score_ref, grads, _ = _oracle()
    m, _ = _model(torch.bfloat16)
    m.freeze_batchnorm()
    m.train()
    vd, vp, xd, xp, y = (t.to(DEV) for t in _inputs())
    m.zero_grad()
    out = m(vd, vp, xd.bfloat16(), xp.bfloat16())
    _, loss = binary_cross_entropy(out[4], y)
    loss.backward()
    assert relerr(out[4], score_ref) <= BF16_TOL
    named = dict(m.named_parameters())
    keys = [k for k in grads if k in named and named[k].grad is not None]
    got = torch.cat([named[k].grad.detach().double().cpu().flatten() for k in keys])
    ref = torch.cat([grads[k].flatten() for k in keys])
    cos = float(torch.dot(got, ref) / (got.norm() * ref.norm()))
    assert cos >= BF16_COS, cos


@pytest.mark.parametrize("compact", [False, True])
def test_input_gradient_of_a_deployed_model(compact):
    """model.eval(), a protein LLM embedding that asks for a gradient, backward: the gradient is finite and the oracle's, with
    the ProteinCNN on all rows and on the distinct rows of the plan."""
    from druglamp_amd import ops
    from druglamp_amd.model.basic_model import binary_cross_entropy
    from druglamp_amd.protein_plan import BatchHints, lengths_from_codes
    from tests.test_protein_cnn_compact_gpu import _plan_dev
    _, score_ref, grads, xp_grad = _oracle()
    m, _ = _model()
    m.eval()
    vd, vp, xd, xp, y = (t.to(DEV) for t in _inputs())
    xp.requires_grad_(True)
    hints = BatchHints(0, _plan_dev(lengths_from_codes(vp), vp.shape[1])) if compact else None
    out = m(vd, vp, xd, xp, hints=hints)
    _, loss = binary_cross_entropy(out[4], y)
    loss.backward()
    ops.check_guard_flags(DEV)
    assert relerr(out[4], score_ref) <= F32_TOL
    assert xp.grad is not None and bool(torch.isfinite(xp.grad).all()) and float(xp.grad.abs().max()) > 0
    assert rel_l2(xp.grad, xp_grad) <= 10 * F32_TOL, rel_l2(xp.grad, xp_grad)
    k = "protein_extractor.conv1.weight"                      # the ProteinCNN's eval-mode backward ran too (its parameters ask for gradients)
    assert rel_l2(dict(m.named_parameters())[k].grad, grads[k]) <= 10 * F32_TOL


# ---- the trainer -------------------------------------------------------------------------------------------------------------
def _trainer(graph, freeze, seed=4321):
    from druglamp_amd import ops
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.trainer import Trainer
    torch.manual_seed(seed)
    ops.manual_seed(77)
    ops.seed_offset_tensor(torch.device(DEV)).zero_()
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    cfg["RS"]["SSL"], cfg["RS"]["CM"] = False, False
    model = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    model.pmma.p_drop = 0.0
    model.pmma.embeddings.p_drop = 0.0
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_(0.1, 0.1)
                mod.running_var.uniform_(0.7, 1.3)
    tr = Trainer(model, cfg, device=torch.device(DEV), compute_dtype=torch.bfloat16, graph_steps=graph, freeze_bn=freeze)
    tr.set_lrs(1e-3, 1e-3, 1e-3)
    return tr


ON_PATH = ("protein_extractor.", "drug_extractor.", "mlp_classifier.")      # where the cls step's nine BatchNorm layers live


def _bn_state(model):
    bufs = {k: v.clone() for k, v in model.named_buffers() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    affine = {k: v.detach().clone() for k, v in model.named_parameters()
              if k.rsplit(".", 1)[0] in {n for n, mod in model.named_modules() if isinstance(mod, torch.nn.BatchNorm1d)}}
    return bufs, affine


def test_trainer_with_frozen_batchnorm_eager_and_graph_replayed():
    from druglamp_amd import ops
    from druglamp_amd.synthetic import make_batch
    batch, meta = make_batch(8, DEV, seed=7, with_graph=True, llm_dtype=torch.bfloat16)
    seq = [(batch, meta)] * 3
    losses = {}
    try:
        for graph in (False, True):
            tr = _trainer(graph, True)
            m = tr.model
            tr.fixed_caps = tr.fixed_caps_for(seq)
            bufs0, affine0 = _bn_state(m)
            assert sum(k.startswith(ON_PATH) for k in bufs0) == 27    # nine BatchNorm layers under the cls step
            arena0 = tr.flat.arena.clone()
            losses[graph] = [float(tr.training_step(b, meta=mt, cur_epoch=1)["cls"]) for b, mt in seq]
            tr.check_device_flags()
            bufs1, affine1 = _bn_state(m)
            for k, v in bufs0.items():
                assert torch.equal(bufs1[k], v), k                   # running statistics and step counters: bitwise unchanged
            moved = [k for k, v in affine0.items() if not torch.equal(affine1[k], v)]
            on_path = [k for k in affine0 if k.startswith(ON_PATH)]
            assert set(on_path) <= set(moved), sorted(set(on_path) - set(moved))
            assert not torch.equal(tr.flat.arena, arena0)
            if graph:
                assert len(tr._graphs) == 1 and sum(g.replays for g in tr._graphs.values()) >= 1
                assert all("frozen_bn" in g.base for g in tr._graphs.values())
            else:
                m.eval()
                m.train()                                            # a later train() leaves BatchNorm frozen
                assert m.training and m.pmma.training
                assert not any(mod.training for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm1d))
                sd_keys = set(m.state_dict())
                m.freeze_batchnorm(False)
                assert all(mod.training for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm1d))
                assert set(m.state_dict()) == sd_keys
    finally:
        ops.use_seed_offset(False)
    # (dropout off, equal capacities: a replay is the eager step bit for bit, as in tests/test_graph_step_gpu.py)
    assert losses[False] == losses[True], (losses[False], losses[True])


def test_trainer_refuses_frozen_batchnorm_with_the_ssl_or_cm_heads():
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.trainer import Trainer
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    assert cfg["RS"]["SSL"]
    model = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    with pytest.raises(ValueError, match="cls steps only"):
        Trainer(model, cfg, device=torch.device(DEV), freeze_bn=True)


def test_without_the_switch_batchnorm_trains_as_before():
    """Guards the rewiring of ProteinCNN.forward to its BatchNorm modules' mode: a model that never called freeze_batchnorm
    runs ProteinCNNFn with training statistics and every running statistic moves."""
    from druglamp_amd import functional as Fn
    from druglamp_amd.synthetic import make_batch
    seen = []
    orig = Fn.ProteinCNNFn.apply

    def spy(x, training, *rest):
        seen.append(bool(training))
        return orig(x, training, *rest)

    tr = _trainer(False, False)
    batch, meta = make_batch(8, DEV, seed=7, with_graph=True, llm_dtype=torch.bfloat16)
    bufs0, _ = _bn_state(tr.model)
    Fn.ProteinCNNFn.apply = spy
    try:
        tr.training_step(batch, meta=meta, cur_epoch=1)
    finally:
        del Fn.ProteinCNNFn.apply                                    # (back to the inherited classmethod)
    assert seen == [True], seen
    bufs1, _ = _bn_state(tr.model)
    still = [k for k, v in bufs0.items() if k.startswith(ON_PATH) and torch.equal(bufs1[k], v)]
    assert not still, still
