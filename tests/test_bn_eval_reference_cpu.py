"""The fp64 reference of dl_bn_eval_bwd (tests/bn_eval_ref.py) against torch autograd of F.batch_norm(training=False), and the
element-wise checker of tests/test_bn_eval_bwd_gpu.py on a CPU emulation of the kernel's result and on planted errors.  Also
the kink share of every GPU case's seed (the GPU test asserts the cap; a seed that broke it would be found here first)."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_eval_ref as ber
from tests import norm_ref as nr
from tests import test_bn_eval_bwd_gpu as tb
from tests.test_norm_paths_gpu import BF, F32, F64, KINK, KINK_CAP

EPS = 1e-5


@pytest.mark.parametrize("relu_in,relu_out", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("rule", ["none", "win", "rw"])
def test_reference_equals_autograd_of_eval_mode_batch_norm(relu_in, relu_out, rule):
    g = torch.Generator().manual_seed(5)
    R, C = 80, 12
    pre = torch.randn(R, C, generator=g, dtype=F64).requires_grad_(True)       # what feeds the ReLU in front (or the BatchNorm itself)
    rmean, rvar = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.5
    gamma = (1.0 + 0.5 * torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    beta = (0.5 * torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    dz = torch.randn(R, C, generator=g, dtype=F64)
    if rule == "none":
        w = torch.ones(R, dtype=F64)
    elif rule == "win":
        w = nr.window_weights(R, 20, 3, 15)
    else:
        w = torch.tensor([-1.0, 0.0, 1.0, 3.0], dtype=F64)[torch.randint(0, 4, (R,), generator=g)]
    keep = w >= 0
    y = F.relu(pre) if relu_in else pre
    z = F.batch_norm(y[keep], rmean, rvar, gamma, beta, False, 0.1, EPS)
    if relu_out:
        z = F.relu(z)
    # (excluded rows take no part; a row with w > 1 is ONE row whose dz already is the sum over its copies)
    (z * dz[keep]).sum().backward()
    rstd = 1.0 / torch.sqrt(rvar + EPS)
    dx, sums, m = ber.bn_eval_bwd(dz, y.detach(), w, rmean, rstd, gamma.detach(), beta.detach(), relu_in, relu_out)
    want = torch.zeros(R, C, dtype=F64)
    want[keep] = pre.grad[keep]
    assert torch.allclose(dx, want, rtol=1e-12, atol=1e-13)
    assert bool((dx[~keep] == 0).all())
    assert torch.allclose(sums[:C], beta.grad, rtol=1e-12, atol=1e-13) and torch.allclose(sums[C:], gamma.grad, rtol=1e-12, atol=1e-13)
    assert torch.equal(m["dx"], dx.abs()) and bool((m["s0"] >= sums[:C].abs() - 1e-12).all()) and bool((m["s1"] >= sums[C:].abs() - 1e-12).all())


def test_weights_drop_out_of_the_compact_form():
    """The argument the kernel rests on: a row that stands for m identical rows, fed the SUM of their gradients, gives the
    expanded matrix's sums, and its dx is the sum of the copies' dx."""
    g = torch.Generator().manual_seed(6)
    R, C = 9, 8
    y, dzs = torch.randn(R, C, generator=g, dtype=F64), torch.randn(3, R, C, generator=g, dtype=F64)
    mult = torch.tensor([1, 3, 1, 2, 1, 1, 3, 1, 2])
    mean, rstd, gamma, beta = (torch.randn(C, generator=g, dtype=F64) for _ in range(4))
    idx = torch.repeat_interleave(torch.arange(R), mult)
    copy = torch.cat([torch.arange(int(k)) for k in mult])
    dz_e = dzs[copy, idx]                                                        # every copy has its own gradient
    dz_c = torch.zeros(R, C, dtype=F64).index_add_(0, idx, dz_e)
    for relu_in, relu_out in ((False, False), (True, False), (False, True)):
        dx_e, s_e, _ = ber.bn_eval_bwd(dz_e, y[idx], torch.ones(len(idx), dtype=F64), mean, rstd, gamma, beta, relu_in, relu_out)
        dx_c, s_c, _ = ber.bn_eval_bwd(dz_c, y, mult.double(), mean, rstd, gamma, beta, relu_in, relu_out)
        assert torch.allclose(s_c, s_e, rtol=1e-12, atol=1e-13)
        assert torch.allclose(dx_c, torch.zeros(R, C, dtype=F64).index_add_(0, idx, dx_e), rtol=1e-12, atol=1e-13)


def _emulate(c, relu_in, relu_out):
    """The case's host data and a result with the kernel's roundings: fp32 arithmetic, the output dtype's store."""
    w, rw, _win, y, dz, mean, rstd, gamma, beta = tb.case_data(c)
    y[w < 0], dz[w < 0] = float("nan"), float("nan")
    keep = w >= 0
    xh = (y[keep] - mean) * rstd
    gg = dz[keep] * ((xh * gamma + beta > 0) if relu_out else 1.0)
    v = gg * (gamma * rstd)
    if relu_in:
        v = v * (y[keep] > 0)
    dx = torch.zeros(c.R, c.C)
    dx[keep] = v
    sums = torch.cat([gg.double().sum(0), (gg * xh).double().sum(0)]).float()
    return (w, y, dz, mean, rstd, gamma, beta), dx.to(c.dt), sums


SMALL = [c for c in tb.CASES if c.R <= 400]


@pytest.mark.parametrize("c", SMALL, ids=[c.name for c in SMALL])
def test_checker_accepts_an_emulation_of_the_kernel(c):
    for relu_in, relu_out in tb.MASKS:
        (w, y, dz, mean, rstd, gamma, beta), dx, sums = _emulate(c, relu_in, relu_out)
        tb.check_bn_eval(c.name, c.dt, dz, y, w, mean, rstd, gamma, beta, relu_in, relu_out, dx, sums)
        tb.check_bn_eval(c.name, c.dt, dz, y, w, mean, rstd, gamma, beta, relu_in, relu_out, dx, None)


def _case(name):
    return next(c for c in tb.CASES if c.name == name)


@pytest.mark.parametrize("name", ["wide128_rw_r100", "f32_c256_rw_r100", "wide128_win", "f32_c64_win"])
@pytest.mark.parametrize("relu_in,relu_out", tb.MASKS)
def test_checker_catches_planted_errors(name, relu_in, relu_out):
    c = _case(name)
    (w, y, dz, mean, rstd, gamma, beta), dx, sums = _emulate(c, relu_in, relu_out)
    args = (c.name, c.dt, dz, y, w, mean, rstd, gamma, beta, relu_in, relu_out)
    tb.check_bn_eval(*args, dx, sums)
    ref, rsums, m = ber.bn_eval_bwd(dz, y, w, mean, rstd, gamma, beta, relu_in, relu_out)
    kink = nr.kink(m["pre"], m["pre_mag"], KINK) if relu_out else torch.zeros_like(ref, dtype=torch.bool)
    live = (ref != 0) & ~kink
    # one wrong element of dx: off by 1 % (bf16: two units in the last place would be inside the bound)
    r, col = [int(v) for v in live.nonzero()[len(live.nonzero()) // 2]]
    bad = dx.clone()
    bad[r, col] = float(bad[r, col]) * (1.03 if c.dt == BF else 1.0 + 1e-5)
    with pytest.raises(AssertionError, match="exceeds its rounding bound"):
        tb.check_bn_eval(*args, bad, sums)
    # the weight applied to a row that stands for several
    if c.rule[0] == "rw":
        rows = ((w > 1) & live.any(1)).nonzero().flatten()
        bad = dx.float().clone()
        bad[rows[0]] *= float(w[rows[0]])
        with pytest.raises(AssertionError, match="exceeds its rounding bound"):
            tb.check_bn_eval(*args, bad.to(c.dt), sums)
    # an excluded / halo row read (NaN reaches dx) or written with anything but +0
    ex = int((w < 0).nonzero()[0])
    bad = dx.clone()
    bad[ex] = (dz[ex] * y[ex]).to(c.dt)              # NaN: what a read of that row yields
    with pytest.raises(AssertionError, match="non-finite addressed elements|non-zero excluded row"):
        tb.check_bn_eval(*args, bad, sums)
    bad = dx.clone()
    bad[ex, 3] = -0.0
    with pytest.raises(AssertionError, match="non-zero excluded row"):
        tb.check_bn_eval(*args, bad, sums)
    # d gamma short of one row's term
    keep = w >= 0
    xh = torch.zeros(c.R, c.C, dtype=F64)
    xh[keep] = (y[keep].double() - mean.double()) * rstd.double()
    gfull = torch.zeros(c.R, c.C, dtype=F64)
    gfull[keep] = dz[keep].double() * ((m["pre"][keep] > 0) if relu_out else 1.0)
    term = (gfull * xh)[r]
    bad_s = sums.clone()
    bad_s[c.C:] -= term.float()
    assert float(term.abs().max()) > 0
    with pytest.raises(AssertionError, match="exceeds its rounding bound"):
        tb.check_bn_eval(*args, dx, bad_s)


@pytest.mark.parametrize("c", tb.CASES, ids=[c.name for c in tb.CASES])
def test_case_seeds_stay_under_the_kink_cap(c):
    w, _rw, _win, y, dz, mean, rstd, gamma, beta = tb.case_data(c)
    _, _, m = ber.bn_eval_bwd(dz, y, w, mean, rstd, gamma, beta, False, True)
    share = float((nr.kink(m["pre"], m["pre_mag"], KINK) & (w >= 0)[:, None]).double().mean())
    assert share <= KINK_CAP / 10, share
