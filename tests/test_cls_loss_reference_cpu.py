"""No GPU: the fp64 reference of the classification loss (tests/cls_loss_ref.py) against the reference's FocalLossV1 (the
golden tests/golden/focal_v1.npz), torch's binary_cross_entropy_with_logits and cross_entropy in fp64; ClsLoss validation;
the meta weight parsing; the guard texts and the C ABI's host checks; and the data conditions of every GPU case of
tests/test_cls_loss_paths_gpu.py."""
import dataclasses
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cls_loss_ref as R

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(n, seed, zmax=12.0):
    g = torch.Generator().manual_seed(seed)
    z = (torch.rand(n, generator=g, dtype=F64) * 2 - 1) * zmax
    y = (torch.rand(n, generator=g) < 0.4).double()
    w = torch.rand(n, generator=g, dtype=F64) * 3
    w[::4] = 0.0
    return z, y, w


# ---- the formula ---------------------------------------------------------------------------------------------------------------
def test_reference_equals_the_recorded_focal_loss_of_the_original():
    g = np.load(os.path.join(ROOT, "tests", "golden", "focal_v1.npz"))
    z, y = torch.from_numpy(g["z"]), torch.from_numpy(g["y"])
    assert z.shape == (257,) and float(z.abs().max()) == 20.0 and bool(((y > 0) & (y < 1)).any())
    assert [tuple(s) for s in g["settings"]] == [(0.25, 2.0), (0.5, 1.0), (0.75, 3.0)]
    for k, (alpha, gamma) in enumerate(g["settings"]):
        r = R.cls_loss(z.unsqueeze(1), y, None, float(alpha), float(1 - alpha), float(gamma))
        assert abs(r["loss"] - float(g["loss_%d" % k])) <= 1e-15 * abs(float(g["loss_%d" % k]))
        want = torch.from_numpy(g["grad_%d" % k])
        assert float((r["grad"] - want).abs().max()) <= 1e-16, k
        # the closed form is autograd's derivative (terms reach |z| = 20 and carry a dozen fp64 roundings on either side)
        assert float((r["dz"] - r["dz_autograd"]).abs().max()) <= 24 * 2.0 ** -53 * 20.0, k


@pytest.mark.parametrize("pw", [1.0, 3.0, 0.25])
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_equals_bce_with_logits_with_pos_weight(pw, weighted):
    z, y, w = _rand(300, 11)
    zz = z.clone().requires_grad_(True)
    per = F.binary_cross_entropy_with_logits(zz, y, weight=w if weighted else None, pos_weight=torch.tensor(pw, dtype=F64), reduction="sum")
    want = per / (w.sum() if weighted else 300.0)
    want.backward()
    r = R.cls_loss(z.unsqueeze(1), y, w if weighted else None, pw, 1.0, 0.0)
    assert abs(r["loss"] - float(want.detach())) <= 1e-14 * float(want.detach())
    assert float((r["grad"] - zz.grad).abs().max()) <= 1e-16
    assert float((r["probs"] - torch.sigmoid(z)).abs().max()) <= 1e-16
    assert r["den"] == (float(w.sum()) if weighted else 300.0)


def test_reference_on_two_outputs_with_the_neutral_spec_equals_cross_entropy():
    g = torch.Generator().manual_seed(5)
    s = torch.randn(200, 2, generator=g, dtype=F64) * 6
    y = (torch.rand(200, generator=g) < 0.5).long()
    ss = s.clone().requires_grad_(True)
    want = F.cross_entropy(ss, y)
    want.backward()
    r = R.cls_loss(s, y.double(), None, 1.0, 1.0, 0.0)
    assert abs(r["loss"] - float(want.detach())) <= 1e-14 * float(want.detach())
    assert float((torch.stack((-r["grad"], r["grad"]), 1) - ss.grad).abs().max()) <= 1e-16
    assert float((r["probs"] - torch.softmax(s, 1)[:, 1]).abs().max()) <= 1e-15


def test_gamma_zero_is_exactly_one_and_sign_zero_is_zero():
    z = torch.tensor([0.0, 0.0, 3.0], dtype=F64)
    y = torch.tensor([0.5, 0.5, 1.0], dtype=F64)
    r0 = R.cls_loss(z.unsqueeze(1), y, None, 1.0, 1.0, 0.0)
    assert float(r0["terms"][0]) == math.log(2.0)                                # m = 1 also at d = 0
    r1 = R.cls_loss(z.unsqueeze(1), y, None, 1.0, 1.0, 1.0)
    assert float(r1["d"][0]) == 0.0 and float(r1["terms"][0]) == 0.0 and float(r1["dz"][0]) == 0.0


def test_reference_poisons_bad_rows_and_keeps_the_others():
    for b in R.BAD_CASES:
        score, y, w, gout = R.bad_data(b, 300, torch.float32, 1)
        r = R.cls_loss(score, y, w, 0.25, 0.75, 2.0, gout)
        assert math.isnan(r["loss"]) and math.isfinite(r["loss_clean"]) and r["den"] > 0, b.name
        assert r["poisoned"].nonzero().flatten().tolist() == [b.row], b.name          # exactly the row the case names
        assert r["flagged"].nonzero().flatten().tolist() == ([b.row] if b.flagged else []), b.name
        assert bool(torch.isfinite(r["grad"]).all())
        if b.what == "z":
            want = {"nan": float("nan"), "inf": 1.0, "-inf": 0.0}[str(b.value)]
            got = float(r["probs"][b.row])
            assert got == want or (got != got and want != want), b.name


# ---- the GPU cases' data ---------------------------------------------------------------------------------------------------------
def test_case_table_crosses_every_axis_with_both_forms():
    assert R.SIZES == (1, 63, 64, 65, 255, 256, 257, R.ONE_WG, R.ONE_WG + 1, 70001)
    assert {c.N for c in R.CASES} == set(R.SIZES) and len({c.name for c in R.CASES}) == len(R.CASES)
    for single in (True, False):
        cs = [c for c in R.CASES if (c.N <= R.ONE_WG) == single]
        assert {c.dt for c in cs} == {torch.float32, torch.bfloat16} and {c.n_out for c in cs} == {1, 2}
        assert {c.ld == c.n_out for c in cs} == {True, False} and {c.ld for c in cs} <= {1, 2, 8}
        assert {c.weights for c in cs} == {True, False}
        assert {c.gamma for c in cs} == set(R.GAMMAS) == {0.0, 1.0, 2.0, 1.5}
        assert {c.a for c in cs} == set(R.ALPHAS) == {(1.0, 1.0), (3.0, 1.0), (0.25, 0.75), (0.0, 1.0)}
        assert {c.data for c in cs} == {"hard", "soft", "yp"}
    hdr = open(os.path.join(ROOT, "druglamp_amd", "csrc", "cls_loss.hip")).read()
    assert re.search(r"CLS_ONE_WG_ROWS\s*=\s*%d\b" % R.ONE_WG, hdr)
    assert (70001 + 255) // 256 > 256                                           # the final kernel's strided pass takes a second round


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_case_data_conditions(c):
    score, y, w, gout = R.case_data(c)
    assert score.shape == (c.N, c.n_out) and score.dtype == c.dt and (w is not None) == c.weights
    r = R.cls_loss(score, y, w, c.a[0], c.a[1], c.gamma, gout)
    R.conditions(c, r, y)
    if c.weights and c.N >= 5:
        assert bool((w == 0).any()) and bool((w > 0).any())
    if c.data == "hard":
        assert bool(((y == 0) | (y == 1)).all())
        if c.N > 2:
            assert float(r["z"].abs().max()) >= 88.0
    assert float(r["dz"].sub(r["dz_autograd"]).abs().max()) <= 1e-12 * max(1.0, float(r["dz"].abs().max()))
    for v in (c.a[0], c.a[1], c.gamma, gout):                                  # the kernel's fp32 arguments are exact
        assert float(torch.tensor(v, dtype=torch.float32)) == v


# ---- ClsLoss ---------------------------------------------------------------------------------------------------------------------
def test_cls_loss_spec_is_validated_and_immutable():
    from druglamp_amd.cls_loss import ClsLoss
    s = ClsLoss()
    assert (s.pos_weight, s.neg_weight, s.gamma) == (1.0, 1.0, 0.0)
    assert dataclasses.astuple(ClsLoss(3, 1, 2)) == (3.0, 1.0, 2.0) and ClsLoss(0.0, 1.0) and ClsLoss(1.0, 0.0, 8.0) and ClsLoss(gamma=1.0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.gamma = 2.0
    nan, inf = float("nan"), float("inf")
    for kw in ({"pos_weight": -1.0}, {"pos_weight": nan}, {"pos_weight": inf}, {"neg_weight": -0.5}, {"neg_weight": nan},
               {"neg_weight": inf}, {"pos_weight": 0.0, "neg_weight": 0.0}, {"gamma": -1.0}, {"gamma": 0.5}, {"gamma": 0.999},
               {"gamma": 8.5}, {"gamma": nan}, {"gamma": inf}, {"gamma": "2"}, {"pos_weight": None}, {"neg_weight": True},
               {"pos_weight": torch.tensor(1.0)}):
        with pytest.raises(ValueError):
            ClsLoss(**kw)
    f = ClsLoss.focal(0.25, 2)
    assert dataclasses.astuple(f) == (0.25, 0.75, 2.0) and dataclasses.astuple(ClsLoss.focal()) == (0.25, 0.75, 2.0)
    assert ClsLoss.focal(0.0, 1.0).pos_weight == 0.0 and ClsLoss.focal(1.0, 0.0).neg_weight == 0.0
    for a, g in ((-0.1, 2.0), (1.1, 2.0), (nan, 2.0), (0.25, 0.5), (0.25, 9.0), ("a", 2.0)):
        with pytest.raises(ValueError):
            ClsLoss.focal(a, g)


def test_trainer_refuses_what_is_not_a_cls_loss():
    import inspect
    from druglamp_amd.trainer import Trainer
    assert inspect.signature(Trainer.__init__).parameters["cls_loss"].default is None
    with pytest.raises(ValueError, match="ClsLoss"):
        Trainer(None, None, cls_loss=(1.0, 1.0, 0.0))
    with pytest.raises(TypeError):
        from druglamp_amd.cls_loss import classification_loss
        classification_loss(torch.zeros(2, 1), torch.zeros(2), (1.0, 1.0, 0.0))


def test_meta_weights_all_none_some():
    from druglamp_amd.cls_loss import meta_weights
    assert meta_weights(None) is None and meta_weights([]) is None
    assert meta_weights([{"Y": 1.0}, {"Y": 0.0}]) is None
    w = meta_weights([{"Y": 1.0, "Weight": 2}, {"Y": 0.0, "Weight": 0.5}, {"Weight": -1.0}])      # (a bad value is the device guard's business)
    assert w.dtype == torch.float32 and w.tolist() == [2.0, 0.5, -1.0] and w.device.type == "cpu"
    for meta in ([{"Weight": 1.0}, {"Y": 0.0}], [{"Y": 0.0}, {"Y": 1.0}, {"Weight": 1.0}]):
        with pytest.raises(ValueError, match="all of them or none"):
            meta_weights(meta)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_signatures_build_flag_and_guard_texts():
    from druglamp_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, "include", "druglamp_hip.h")).read()
    assert ops.FLAG_CLS_LABEL == 1 and set(ops.CLS_FLAG_TEXT) == {ops.FLAG_CLS_LABEL}
    text = ops.guard_message(0, ops.FLAG_CLS_LABEL)
    assert "classification loss guard tripped — FLAG_CLS_LABEL" in text and "Weight" in text and "label" in text and "padding" not in text
    both = ops.guard_message(_lib.FLAG_GCN_NODE_PAD, ops.FLAG_CLS_LABEL, " in an earlier step")
    assert "padding guard tripped in an earlier step — " + ops.FLAG_TEXT[_lib.FLAG_GCN_NODE_PAD] in both and "FLAG_CLS_LABEL" in both
    assert ops.guard_message(_lib.FLAG_GCN_NODE_PAD) == "druglamp_amd: padding guard tripped — " + ops.FLAG_TEXT[_lib.FLAG_GCN_NODE_PAD]
    assert "unknown" in ops.guard_message(0, 2)
    assert build.FILE_FLAGS["cls_loss.hip"] == ["-fno-slp-vectorize"]
    for fn in ("dl_cls_loss_fwd", "dl_cls_loss_bwd", "dl_cls_loss_workspace_bytes"):
        assert fn in _lib.SIGNATURES and re.search(r"\b%s\(" % fn, hdr)


def test_host_checks_refuse_bad_arguments_before_any_launch():
    """The entry points validate on the host and return before touching the device: callable without a GPU."""
    from druglamp_amd import _lib
    L = _lib.lib()
    assert L.dl_cls_loss_workspace_bytes(R.ONE_WG) == 0 and L.dl_cls_loss_workspace_bytes(R.ONE_WG + 1) == 17 * 8
    assert L.dl_cls_loss_workspace_bytes(70001) == 274 * 8
    p = 4096                                                                   # (a non-null address that is never dereferenced)

    def fwd(ld=1, n_out=1, dt=0, N=8, a=(1.0, 1.0), gamma=0.0, score=p, labels=p, out2=p, ws=None, nws=0, flags=None):
        return L.dl_cls_loss_fwd(score, ld, n_out, dt, labels, None, N, a[0], a[1], gamma, None, out2, ws, nws, 1, flags, None)

    def bwd(ld=1, n_out=1, dt=0, N=8, a=(1.0, 1.0), gamma=0.0, out2=p, gout=p, ds=p, ldd=1):
        return L.dl_cls_loss_bwd(p, ld, n_out, dt, p, None, N, a[0], a[1], gamma, out2, gout, ds, ldd, None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(score=None), dict(labels=None), dict(N=0), dict(N=-3), dict(n_out=0), dict(n_out=3), dict(n_out=2, ld=1), dict(dt=2),
           dict(a=(-1.0, 1.0)), dict(a=(1.0, nan)), dict(a=(inf, 1.0)), dict(a=(0.0, 0.0)), dict(gamma=0.5), dict(gamma=-1.0),
           dict(gamma=8.5), dict(gamma=nan)]
    for kw in bad:
        assert fwd(**kw) != 0, kw
        assert b"dl_cls_loss_fwd" in L.dl_last_error(), kw
        if "score" not in kw and "labels" not in kw:
            assert bwd(**kw) != 0 and b"dl_cls_loss_bwd" in L.dl_last_error(), kw
    assert fwd(out2=None) != 0 and fwd(flags=2) != 0
    assert fwd(N=R.ONE_WG + 1) != 0 and b"workspace" in L.dl_last_error()       # the two-stage form needs its workspace
    assert fwd(N=R.ONE_WG + 1, ws=p, nws=17 * 8 - 1) != 0 and b"workspace" in L.dl_last_error()
    assert bwd(out2=None) != 0 and bwd(gout=None) != 0 and bwd(ds=None) != 0 and bwd(n_out=2, ld=2, ldd=1) != 0
