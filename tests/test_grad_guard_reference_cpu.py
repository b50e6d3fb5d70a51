"""The gradient guard without a GPU: the fp64 restatement of tests/grad_guard_ref.py pinned against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, and the host logic of the three entry points and of the Trainer's
arguments (validation happens before any launch)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import grad_guard_ref as gr

LR, B1, B2, EPS, WD = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8, 1e-2))   # the fp32 values the C ABI receives
SHAPES = [(5,), (3, 4), (7, 2), (1,), (2, 3, 3)]
MAX_NORM = 0.75
POISON_STEP = 3                                  # 1-based; not the first (torch creates its state in the first step)


def _grads(step, poison):
    g = torch.Generator().manual_seed(100 + step)
    out = [torch.randn(s, generator=g, dtype=torch.float32) * (0.2 + 0.4 * step) for s in SHAPES]
    if poison:
        out[2].view(-1)[5] = float("inf")
    return out


def _torch_run(steps, skip_nonfinite):
    """fp64 torch: clip_grad_norm_ + AdamW; a non-finite step is 'opt.step() not taken, count advanced'."""
    g0 = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter(torch.randn(s, generator=g0, dtype=torch.float32).double()) for s in SHAPES]
    opt = torch.optim.AdamW(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    coefs = []
    for step in range(1, steps + 1):
        grads = _grads(step, step == POISON_STEP)
        for p, g in zip(params, grads):
            p.grad = g.double().clone()
        before = [p.grad.clone() for p in params]
        total = torch.nn.utils.clip_grad_norm_(params, MAX_NORM, error_if_nonfinite=False)
        k = max(range(len(params)), key=lambda i: float(before[i].abs().max()) if torch.isfinite(before[i]).all() else -1.0)
        j = int(before[k].abs().argmax())
        coefs.append(float(params[k].grad.view(-1)[j] / before[k].view(-1)[j]))
        if skip_nonfinite and not math.isfinite(float(total)):
            for p in params:
                opt.state[p]["step"] += 1
            continue
        opt.step()
    return params, opt, coefs


def _ref_run(steps, skip_nonfinite):
    g0 = torch.Generator().manual_seed(7)
    p = torch.cat([torch.randn(s, generator=g0, dtype=torch.float32).view(-1) for s in SHAPES]).double()
    m, v, mag = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    guards = []
    for step in range(1, steps + 1):
        g = torch.cat([t.view(-1) for t in _grads(step, step == POISON_STEP)])
        d = gr.finalize(gr.sqnorm(g), 1.0, MAX_NORM, skip_nonfinite)
        guards.append(d)
        p, m, v = gr.adamw_guarded(p, g, m, v, (d["coef"], d["norm"], d["skip"]), LR, B1, B2, EPS, WD, step, 1.0)
        if not d["skip"] and math.isfinite(d["norm"]):
            mag = B1 * mag + (1 - B1) * (g.double() * d["coef"]).abs()       # the sum of the absolute terms of exp_avg
    return p, m, v, guards, mag


def test_reference_equals_torch_clipping_and_adamw_over_four_steps():
    steps = 4
    params, opt, coefs = _torch_run(steps, skip_nonfinite=True)
    p, m, v, guards, mag = _ref_run(steps, skip_nonfinite=True)
    tp = torch.cat([q.detach().view(-1) for q in params])
    tm = torch.cat([opt.state[q]["exp_avg"].view(-1) for q in params])
    tv = torch.cat([opt.state[q]["exp_avg_sq"].view(-1) for q in params])
    u = 2.0 ** -24
    for step, (d, c) in enumerate(zip(guards, coefs), 1):
        if step == POISON_STEP:
            assert d["skip"] == 1.0 and d["coef"] == 0.0 and not math.isfinite(d["norm"]) and d["clipped"] == 0
            continue
        # the clipped coefficient: torch's fp64 value, rounded once to fp32 by the guard
        assert d["skip"] == 0.0 and d["clipped"] == 1 and 0 < d["coef"] < 1
        assert abs(d["coef"] - c) <= u * c, (step, d["coef"], c)
    assert all(int(opt.state[q]["step"]) == steps for q in params)            # count advanced on the skipped step too
    # The reference's gradient scale carries two fp32 roundings (the coefficient, its product with grad_scale): 2^-23
    # relative on the gradient, so on every term of exp_avg (whose terms may cancel: measured against their absolute sum);
    # twice that on exp_avg_sq (positive terms); the update m / (sqrt(v) + eps) moves by at most 2^-23 + 2^-23 of itself per
    # step, the parameter by the sum over the steps.  A factor 2 of slack each.
    assert float(((m - tm).abs() / mag).max()) <= 2 * 2 * u
    assert float(((v - tv).abs() / tv.abs().clamp_min(1e-30)).max()) <= 2 * 4 * u
    upd_bound = LR / (1 - B1)                         # |m_hat / sqrt(v_hat)| <= 1 / (1 - b1) at these step counts (loose)
    assert float((p - tp).abs().max()) <= 2 * 4 * u * steps * upd_bound
    assert torch.isfinite(p).all() and torch.isfinite(tp).all()


def test_reference_without_skip_lets_the_nonfinite_step_through_like_torch():
    """skip_nonfinite off: the coefficient is what the torch formula gives for an infinite norm (0), and the infinite
    element times 0 is NaN — in torch and in the restatement."""
    params, opt, coefs = _torch_run(POISON_STEP, skip_nonfinite=False)
    p, m, v, guards, _ = _ref_run(POISON_STEP, skip_nonfinite=False)
    d = guards[-1]
    assert d["skip"] == 0.0 and d["coef"] == 0.0 and d["norm"] == float("inf") and d["clipped"] == 1
    tp = torch.cat([q.detach().view(-1) for q in params])
    assert torch.equal(torch.isnan(p), torch.isnan(tp)) and int(torch.isnan(p).sum()) == 1


def test_finalize_restatement_edge_cases():
    assert gr.finalize(4.0, 1.0, 0.0)["coef"] == 1.0 and gr.finalize(4.0, 1.0, -1.0)["coef"] == 1.0
    d = gr.finalize(4.0, 0.5, 2.0)                    # norm 1 <= max_norm: clamp to exactly 1, not counted as clipped
    assert d["coef"] == 1.0 and d["norm"] == 1.0 and d["clipped"] == 0
    d = gr.finalize(float("nan"), 1.0, 2.0, skip_nonfinite=False)
    assert d["coef"] != d["coef"] and d["skip"] == 0.0 and d["clipped"] == 0
    big = gr.sqnorm(np.full(1000, 3e38, np.float32))                 # finite in fp64 although every square overflows fp32
    d = gr.finalize(big, 1.0, 1.0, skip_nonfinite=True)
    assert math.isfinite(big) and d["skip"] == 0.0 and d["norm"] == float("inf") and 0 < d["coef"] < 1e-30
    assert gr.finalize(gr.sqnorm(np.full(1000, 1e-30, np.float32)), 1.0, 1.0)["norm"] > 0


def test_entry_points_validate_their_arguments_before_any_launch():
    from druglamp_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    p16 = (C.addressof(buf) + 15) // 16 * 16
    adam = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
    cases = [
        ("dl_grad_sqnorm", lambda: L.dl_grad_sqnorm(None, 16, p16, 0, p16, 64, None)),
        ("dl_grad_sqnorm", lambda: L.dl_grad_sqnorm(p16, 16, None, 0, p16, 64, None)),
        ("dl_grad_sqnorm", lambda: L.dl_grad_sqnorm(p16, 16, p16, 0, None, 64, None)),
        ("dl_grad_sqnorm", lambda: L.dl_grad_sqnorm(p16, 0, p16, 0, p16, 64, None)),
        ("dl_grad_sqnorm", lambda: L.dl_grad_sqnorm(p16 + 4, 16, p16, 0, p16, 64, None)),             # misaligned g
        ("dl_grad_sqnorm", lambda: L.dl_grad_sqnorm(p16, 3 * 4096, p16, 0, p16, 16, None)),           # needs 24 bytes
        ("dl_grad_guard_finalize", lambda: L.dl_grad_guard_finalize(None, 1.0, 1.0, 1, p16, p16, None)),
        ("dl_grad_guard_finalize", lambda: L.dl_grad_guard_finalize(p16, 1.0, 1.0, 1, None, p16, None)),
        ("dl_grad_guard_finalize", lambda: L.dl_grad_guard_finalize(p16, 1.0, 1.0, 1, p16, None, None)),
        ("dl_adamw_step_guarded", lambda: L.dl_adamw_step_guarded(None, p16, p16, p16, 16, *adam, 1, 1.0, None, 0, p16, None)),
        ("dl_adamw_step_guarded", lambda: L.dl_adamw_step_guarded(p16, p16, p16, p16, 16, *adam, 1, 1.0, None, 0, None, None)),
        ("dl_adamw_step_guarded", lambda: L.dl_adamw_step_guarded(p16, p16, p16, p16, 0, *adam, 1, 1.0, None, 0, p16, None)),
        ("dl_adamw_step_guarded", lambda: L.dl_adamw_step_guarded(p16, p16, p16, p16, 16, *adam, 0, 1.0, None, 0, p16, None)),
    ]
    for name, call in cases:
        assert call() == -1, name
        assert name.encode() in L.dl_last_error(), (name, L.dl_last_error())
    assert b"workspace" in (L.dl_grad_sqnorm(p16, 3 * 4096, p16, 0, p16, 16, None), L.dl_last_error())[1]


def test_workspace_formula_of_the_wrapper_is_the_headers():
    from druglamp_amd import ops
    assert [ops.grad_sqnorm_workspace_bytes(n) for n in (1, 4096, 4097, 2048 * 4096, 2048 * 4096 + 1, 1 << 40)] == \
        [8, 8, 16, 8 * 2048, 8 * 2048, 8 * 2048]


@pytest.mark.parametrize("bad", [0, 0.0, -1, float("nan"), float("inf")])
def test_trainer_rejects_a_max_grad_norm_that_is_not_positive_and_finite(bad):
    from druglamp_amd.trainer import Trainer
    with pytest.raises(ValueError, match="max_grad_norm"):
        Trainer(None, None, max_grad_norm=bad)
