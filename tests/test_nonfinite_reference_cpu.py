"""What tests/test_nonfinite_paths_gpu.py rests on, without a GPU:

  * the torch semantics the contract ("Non-finite values") is written from, asserted in fp64;
  * every case of the GPU table built on the CPU and classified from the fp64 references alone: no plant is vacuous (at least
    one poisoned and one untouched output element), every clean reference is finite, and the case takes the launch form it
    names (the existing mirrors of the host dispatch: gemm_ref.select, _is16 / _bn_forms, norm_adj_form, gate_bwd_form);
  * the checker catches planted errors: a ReLU that swallows NaN, a softmax whose maximum and sum drop NaN, an untouched
    element that differs by one ulp; the reference itself passes.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import nonfinite_ref as NF
from tests import test_nonfinite_paths_gpu as T

F64 = torch.float64
NAN, INF = float("nan"), float("inf")


# ---- torch semantics ---------------------------------------------------------------------------------------------------------
def test_relu_and_clamp_keep_nan():
    x = torch.tensor([NAN, -1.0, 2.0, -INF, INF], dtype=F64)
    r = torch.relu(x)
    assert math.isnan(float(r[0])) and r[1:].tolist() == [0.0, 2.0, 0.0, INF]
    assert math.isnan(float(torch.clamp(x, min=1.0)[0])) and math.isnan(float(x.clamp_min(0.0)[0]))
    assert math.isnan(float(torch.tensor([NAN], dtype=F64).clamp_min(1.0).rsqrt()))


def test_gelu_of_infinities():
    g = F.gelu(torch.tensor([-INF, INF, NAN], dtype=F64))
    assert math.isnan(float(g[0])) and float(g[1]) == INF and math.isnan(float(g[2]))       # -inf x Phi(-inf) = -inf x 0


def test_minus_inf_logit_is_a_masked_class():
    x = torch.tensor([[0.5, -INF, 1.5], [0.5, INF, 1.5], [0.5, NAN, 1.5]], dtype=F64)
    p = torch.softmax(x, 1)
    assert float(p[0, 1]) == 0.0 and abs(float(p[0].sum()) - 1.0) < 1e-15
    assert bool(torch.isnan(p[1]).all()) and bool(torch.isnan(p[2]).all())
    ce = F.cross_entropy(x, torch.tensor([0, 0, 0]), reduction="none")
    two = F.cross_entropy(x[:1, [0, 2]], torch.tensor([0]), reduction="none")
    assert abs(float(ce[0]) - float(two[0])) < 1e-15 and math.isnan(float(ce[1])) and math.isnan(float(ce[2]))
    # an ignored row full of NaN leaves the mean alone
    y = torch.tensor([0, -100, 2])
    xx = torch.tensor([[0.5, 0.1, 1.5], [NAN, NAN, NAN], [0.3, 0.2, 0.1]], dtype=F64, requires_grad=True)
    loss = F.cross_entropy(xx, y, ignore_index=-100)
    clean = F.cross_entropy(xx.detach()[[0, 2]], y[[0, 2]])
    assert float(loss.detach()) == float(clean)
    # (torch's own backward multiplies the ignored row's softmax by 0 and returns NaN for that row's logits; here an ignored
    # row contributes nothing, forward and backward: DESIGN.md "Non-finite values", selects are selects, and loss_ref.ce_rows_bwd)
    loss.backward()
    assert bool(torch.isfinite(xx.grad[[0, 2]]).all()) and bool(torch.isnan(xx.grad[1]).all())     # the recorded divergence, pinned


def test_norms_of_a_column_holding_inf_are_nan():
    x = torch.randn(6, 3, dtype=F64)
    for v in (INF, -INF, NAN):
        x[2, 1] = v
        bn = F.batch_norm(x, None, None, training=True)
        assert bool(torch.isnan(bn[:, 1]).all()) and bool(torch.isfinite(bn[:, [0, 2]]).all())
        ln = F.layer_norm(x, (3,))
        assert bool(torch.isnan(ln[2]).all()) and bool(torch.isfinite(ln[[0, 1, 3, 4, 5]]).all())


def test_relu_backward_is_a_select():
    x = torch.tensor([-1.0, 2.0], dtype=F64, requires_grad=True)
    torch.relu(x).backward(torch.tensor([NAN, NAN], dtype=F64))
    assert float(x.grad[0]) == 0.0 and math.isnan(float(x.grad[1]))


def test_adamw_with_an_inf_gradient_gives_nan():
    for v in (INF, NAN):
        p = torch.nn.Parameter(torch.ones(3, dtype=F64))
        opt = torch.optim.AdamW([p], lr=1e-3)
        p.grad = torch.tensor([0.1, v, -0.2], dtype=F64)
        opt.step()
        q = p.detach()
        assert math.isnan(float(q[1])) and math.isfinite(float(q[0])) and math.isfinite(float(q[2]))


# ---- every case of the GPU table, from the references ------------------------------------------------------------------------
def test_case_names_are_unique():
    names = [c.name for c in T.ALL_CASES]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", T.ALL_CASES, ids=[c.name for c in T.ALL_CASES])
def test_case_is_not_vacuous_and_names_its_form(case):
    side = case.make("cpu")
    assert T.expected_form(case, side) == case.form, "%s names another launch form" % case.name
    clean, plants = T.classify_case(case, side)
    assert len(plants) >= 2
    again = side.ref()                                     # the plants were removed
    for k in clean:
        assert torch.equal(NF.bits(again[k]), NF.bits(clean[k])), k
    kinds = {pl.value for pl, _, _ in plants}
    assert "nan" in kinds


def test_gemm_table_covers_every_epilogue_and_tile_family():
    forms = " ; ".join(c.form for c in T.GEMM_CASES)
    for need in ("epi0", "epi2", "epi3", "epi4", "epi5", "epi1", "big256 epi5", "lat128 epi5", "reduce<", "tt2", "group", "pair", " cs "):
        assert need in forms, need
    acts = {(s.c.act, "epi1" in c.form) for c in T.GEMM_CASES for s in [c.make("cpu")] if s.c.kind == "gemm"}
    assert (1, True) in acts and (2, True) in acts         # the general epilogue with act 1 and act 2
    ops = {pl.operand for c in T.GEMM_CASES for pl in c.plants}
    assert ops == {"X", "W", "bias", "res", "old"}
    epi4 = [c for c in T.GEMM_CASES if "epi4" in c.form]
    assert epi4 and all({pl.operand for pl in c.plants} == {"X", "W"} for c in epi4)      # through the incoming gradient only


# ---- the checker catches planted errors ------------------------------------------------------------------------------------------
def _relu_case():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, 9, generator=g, dtype=F64)
    xp = x.clone()
    xp[2, 3] = NAN
    xp[4, 5] = -INF                                        # relu(-inf) = 0: a moved element
    return x, xp


def test_checker_passes_the_reference_and_fails_a_swallowing_relu():
    x, xp = _relu_case()
    ref = lambda t: t.clamp_min(0.0)
    swallow = lambda t: torch.where(t > 0, t, torch.zeros_like(t))
    p, u, m = NF.classify(ref(x), ref(xp))
    assert int(p.sum()) == 1 and int(u.sum()) >= 60
    NF.check_nonfinite("relu", "ref", "y", ref(x), ref(xp), ref(x), ref(xp), lambda moved: 0.0)
    with pytest.raises(AssertionError, match="came out finite"):
        NF.check_nonfinite("relu", "where", "y", swallow(x), swallow(xp), ref(x), ref(xp))


def test_checker_fails_a_softmax_whose_maximum_and_sum_drop_nan():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(5, 8, generator=g, dtype=F64)
    xp = x.clone()
    xp[1, 2] = NAN

    def dropping(t):                                       # fmaxf-style maximum and a sum that skips NaN terms
        m = torch.nan_to_num(t, nan=-INF).amax(1, keepdim=True)
        e = torch.exp(t - m)
        return e / torch.nan_to_num(e, nan=0.0).sum(1, keepdim=True)
    ref = lambda t: torch.softmax(t, 1)
    NF.check_nonfinite("softmax", "ref", "p", ref(x), ref(xp), ref(x), ref(xp))
    assert int(torch.isnan(dropping(xp)).sum()) == 1       # only the planted element: the rest of the row came out finite
    with pytest.raises(AssertionError, match="came out finite"):
        NF.check_nonfinite("softmax", "dropping", "p", dropping(x), dropping(xp), ref(x), ref(xp))


def test_checker_fails_one_ulp_in_an_untouched_element_and_the_other_infinity():
    x, xp = _relu_case()
    ref = lambda t: t.clamp_min(0.0)
    got = ref(xp).float()
    leak = got.clone()
    leak[6, 8] = torch.nextafter(leak[6, 8], torch.tensor(INF))
    with pytest.raises(AssertionError, match="do not depend on the plant"):
        NF.check_nonfinite("relu", "ulp", "y", ref(x).float(), leak, ref(x), ref(xp))
    y, yp = x.clone(), x.clone()
    yp[0, 0] = INF
    wrong = yp.clone()
    wrong[0, 0] = -INF
    with pytest.raises(AssertionError, match="other infinity"):
        NF.check_nonfinite("copy", "sign", "y", y, wrong, y, yp)
    nan_for_inf = yp.clone()
    nan_for_inf[0, 0] = NAN
    rec = NF.check_nonfinite("copy", "nan", "y", y, nan_for_inf, y, yp)
    assert rec["inf_as_nan"] == 1 and rec["nan_as_inf"] == 0
    moved_bad = ref(xp).clone()
    moved_bad[4, 5] = 1e-3                                 # relu(-inf) must be an exact zero under the bound 0
    with pytest.raises(AssertionError, match="exceeds its bound"):
        NF.check_nonfinite("relu", "moved", "y", ref(x), moved_bad, ref(x), ref(xp), lambda moved: 0.0)


def test_vacuous_cases_are_refused():
    x = torch.randn(4, 4, dtype=F64)
    with pytest.raises(AssertionError, match="poisons nothing"):
        NF.assert_not_vacuous("c", "p", [(x, x.clone())])
    with pytest.raises(AssertionError, match="no output that is independent"):
        NF.assert_not_vacuous("c", "p", [(x, torch.full_like(x, NAN))])


def test_log_lines(tmp_path, monkeypatch):
    import json
    path = tmp_path / "nf.jsonl"
    monkeypatch.setenv("DL_NONFINITE_LOG", str(path))
    x, xp = _relu_case()
    ref = lambda t: t.clamp_min(0.0)
    NF.check_nonfinite("relu", "ref", "y", ref(x), ref(xp), ref(x), ref(xp), None, "x@2,3=nan")
    rec = json.loads(path.read_text().strip())
    assert rec["case"] == "relu" and rec["plant"] == "x@2,3=nan" and rec["poisoned"] == 1 and rec["moved"] == 1 and rec["swallowed"] == 0
