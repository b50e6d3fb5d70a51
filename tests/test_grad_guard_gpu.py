"""The gradient-guard kernels (csrc/grad_guard.hip; dl_adamw_step_guarded: csrc/optim.hip) through druglamp_amd.ops, against tests/grad_guard_ref.py.

  * dl_grad_sqnorm: the fp64 sum of the exactly squared fp32 data to a relative n 2^-53 (the bound of ANY summation order in
    fp64 for positive terms — derived, not measured), bitwise repeatable, at sizes that take every path of the launch shape:
    below one 16-byte chunk, a scalar tail, several workgroups, more than one grid pass ((1 << 23) + 5: 2049 block-passes of
    4096 elements over a grid capped at 2048 workgroups), and accumulation over three runs;
  * magnitudes an fp32 accumulator gets wrong (3e38: squares overflow fp32; 1e-30: squares underflow it);
  * NaN / +inf / -inf planted first, last (in the scalar tail) and in the middle, with and without skip_nonfinite;
  * dl_grad_guard_finalize: coefficient, norm, skip flag, counters;
  * dl_adamw_step_guarded: bitwise dl_adamw_step at the effective scale; nothing written on a skipped step."""
import math

import numpy as np
import pytest
import torch

from tests import grad_guard_ref as gr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U64 = 2.0 ** -53


def _state(n):
    from druglamp_amd import ops
    acc = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.full((ops.grad_sqnorm_workspace_bytes(n) // 8,), float("nan"), dtype=torch.float64, device=DEV)   # needs no initialisation
    guard = torch.full((4,), -7.0, dtype=torch.float32, device=DEV)
    counters = torch.zeros(2, dtype=torch.int64, device=DEV)
    return acc, ws, guard, counters


def _data(n, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g, dtype=torch.float32) * scale).to(DEV)


def _ulps(got, want):
    return abs(float(got) - float(want)) / float(gr.ulp32(want))


@pytest.mark.parametrize("n", [1, 3, 4, 1003, 1028, (1 << 20) + 5, (1 << 23) + 5])
def test_sqnorm_against_the_fp64_sum_of_exact_squares(n):
    from druglamp_amd import ops
    g = _data(n, seed=n % 97)
    acc, ws, guard, counters = _state(n)
    ops.grad_sqnorm(g, acc, ws)
    first = acc.clone()
    ops.grad_guard_finalize(acc, guard, counters)
    ws.fill_(float("nan"))
    ops.grad_sqnorm(g, acc, ws)
    want = gr.sqnorm(g)
    got = float(first)
    print("n", n, "relative error / 2^-53:", abs(got - want) / want / U64)
    assert abs(got - want) <= n * U64 * want
    assert torch.equal(first.view(torch.int64), acc.view(torch.int64)), "two calls on the same data differ"
    ref = gr.finalize(want)
    gd = guard.tolist()
    assert _ulps(gd[1], ref["norm64"]) <= 1.0
    assert gd[0] == 1.0 and gd[2] == 0.0 and gd[3] == 0.0 and counters.tolist() == [0, 0]


def test_sqnorm_accumulates_over_three_runs():
    from druglamp_amd import ops
    parts = [_data(1003, 1), _data(4, 2), _data(1028, 3)]
    acc, ws, _, _ = _state(1028)
    acc.fill_(123.0)                                    # the first run overwrites
    for k, g in enumerate(parts):
        ops.grad_sqnorm(g, acc, ws, accumulate=k > 0)
    n = sum(p.numel() for p in parts)
    want = gr.sqnorm(torch.cat(parts))
    assert abs(float(acc) - want) <= n * U64 * want
    ops.grad_sqnorm(parts[0], acc, ws, accumulate=True)
    want2 = want + gr.sqnorm(parts[0])
    assert abs(float(acc) - want2) <= (n + 1003) * U64 * want2


@pytest.mark.parametrize("value", [3e38, 1e-30])
@pytest.mark.parametrize("n", [1003, 70001])
def test_magnitudes_an_fp32_accumulator_gets_wrong(value, n):
    from druglamp_amd import ops
    g = torch.full((n,), value, dtype=torch.float32, device=DEV)
    acc, ws, guard, counters = _state(n)
    ops.grad_sqnorm(g, acc, ws)
    ops.grad_guard_finalize(acc, guard, counters, pre_scale=1.0, max_norm=1.0, skip_nonfinite=True)
    want = gr.sqnorm(g)
    ref = gr.finalize(want, 1.0, 1.0, True)
    gd = guard.tolist()
    assert math.isfinite(float(acc)) and abs(float(acc) - want) <= n * U64 * want
    assert gd[2] == 0.0 and counters.tolist()[0] == 0              # a finite gradient never reads as non-finite
    if value > 1:
        assert gd[1] == float("inf") == ref["norm"]                # the norm saturates in fp32, the coefficient does not
        assert 0.0 < gd[0] < 1e-30 and math.isfinite(gd[0]) and _ulps(gd[0], ref["coef64"]) <= 1.0
        assert counters.tolist()[1] == 1
    else:
        assert gd[1] > 0.0 and _ulps(gd[1], ref["norm64"]) <= 1.0
        assert gd[0] == 1.0 and counters.tolist()[1] == 0


@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_nonfinite_element_anywhere_is_seen(bad, where):
    from druglamp_amd import ops
    n = 1003                                            # n % 4 == 3: the last element is in the scalar tail
    g = _data(n, 5)
    g[{"first": 0, "last": n - 1, "middle": 501}[where]] = bad
    acc, ws, guard, counters = _state(n)
    for call in (1, 2):                                 # skip_nonfinite = 1: {0, nonfinite norm, 1}, counted once per call
        ops.grad_sqnorm(g, acc, ws)
        ops.grad_guard_finalize(acc, guard, counters, pre_scale=1.0, max_norm=1.0, skip_nonfinite=True)
        gd = guard.tolist()
        assert gd[0] == 0.0 and gd[2] == 1.0
        assert (gd[1] != gd[1]) if bad != bad else gd[1] == float("inf")
        assert counters.tolist() == [call, 0]
    ops.grad_guard_finalize(acc, guard, counters, pre_scale=1.0, max_norm=1.0, skip_nonfinite=False)
    ref = gr.finalize(gr.sqnorm(g), 1.0, 1.0, False)
    gd = guard.tolist()
    assert gd[2] == 0.0                                 # not skipped: the coefficient is what the torch formula yields
    assert (gd[0] != gd[0] and ref["coef"] != ref["coef"]) if bad != bad else (gd[0] == 0.0 == ref["coef"])
    assert counters.tolist() == [2, ref["clipped"]]


def test_finalize_coefficient_norm_and_counters():
    from druglamp_amd import ops
    acc, _, guard, counters = _state(4)
    want_clipped = 0
    #        acc    pre_scale  max_norm
    cases = [(4.0, 1.0, 0.0), (4.0, 1.0, -3.0), (4.0, 1.0, 3.0), (4.0, 1.0, 1.0), (4.0, 0.5, 0.75), (1e6, 0.5, 1e-3),
             (2.0, 1.0, 1.4142135), (0.0, 1.0, 1.0), (1e300, 1.0, 5.0), (1e-300, 1.0, 5.0)]
    for a, ps, mx in cases:
        acc.fill_(a)
        ops.grad_guard_finalize(acc, guard, counters, pre_scale=ps, max_norm=mx, skip_nonfinite=True)
        ref = gr.finalize(a, ps, mx, True)
        gd = guard.tolist()
        want_clipped += ref["clipped"]
        if mx <= 0 or ref["coef64"] == 1.0:
            assert gd[0] == 1.0, (a, ps, mx, gd)
        else:
            assert _ulps(gd[0], ref["coef64"]) <= 1.0 and gd[0] < 1.0, (a, ps, mx, gd, ref)
        assert (gd[1] == ref["norm"]) if math.isinf(ref["norm"]) else (_ulps(gd[1], ref["norm64"]) <= 1.0), (a, ps, mx, gd, ref)
        assert gd[2] == 0.0 and counters.tolist() == [0, want_clipped]
    assert want_clipped == 5
    acc.fill_(float("inf"))                             # a skipped step is not a clipped one
    ops.grad_guard_finalize(acc, guard, counters, pre_scale=1.0, max_norm=1.0, skip_nonfinite=True)
    assert guard.tolist()[:3] == [0.0, float("inf"), 1.0] and counters.tolist() == [1, want_clipped]


def _adam_operands(n, lowp, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(DEV)
    grad = (torch.randn(n, generator=g) * 3).to(DEV)
    m = (torch.randn(n, generator=g) * 0.1).to(DEV)
    v = (torch.rand(n, generator=g) * 0.01).to(DEV)
    lp = None if lowp is None else torch.full((n,), 5.0, dtype=lowp, device=DEV)
    return p, grad, m, v, lp


KW = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, step=3)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("lowp", [None, torch.float32, torch.bfloat16], ids=["nolowp", "lowp32", "lowp16"])
@pytest.mark.parametrize("n", [1, 4, 1003, 1028])
def test_guarded_adamw_is_adamw_at_the_effective_scale_and_writes_nothing_when_skipped(n, lowp):
    from druglamp_amd import ops
    for coef, gscale in ((1.0, 0.5), (0.37, 0.5), (1e-3, 1.0)):
        guard = torch.tensor([coef, 123.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
        eff = float(np.float32(gscale) * np.float32(coef))
        a = _adam_operands(n, lowp, seed=n)
        b = _adam_operands(n, lowp, seed=n)
        ops.adamw_step(a[0], a[1], a[2], a[3], grad_scale=eff, lowp=a[4], **KW)
        ops.adamw_step_guarded(b[0], b[1], b[2], b[3], guard, grad_scale=gscale, lowp=b[4], **KW)
        for x, y, name in zip(a, b, ("param", "grad", "exp_avg", "exp_avg_sq", "lowp")):
            if x is not None:
                assert torch.equal(_bits(x), _bits(y)), (name, coef)
        assert not torch.equal(a[0], _adam_operands(n, lowp, seed=n)[0])          # (the step did move the parameters)
    guard = torch.tensor([0.0, float("nan"), 1.0, 0.0], dtype=torch.float32, device=DEV)
    for poison in (False, True):
        b = _adam_operands(n, lowp, seed=n)
        if poison:
            b[1].fill_(float("nan"))
        keep = [None if t is None else t.clone() for t in b]
        ops.adamw_step_guarded(b[0], b[1], b[2], b[3], guard, grad_scale=0.5, lowp=b[4], **KW)
        for x, y, name in zip(keep, b, ("param", "grad", "exp_avg", "exp_avg_sq", "lowp")):
            if x is not None:
                assert torch.equal(_bits(x), _bits(y)), (name, "skipped step wrote")
