"""The fp64 normalisation reference of tests/norm_ref.py against torch (layer_norm, batch_norm and fp64 autograd through the
expanded matrix of the weighted forms), and the bounds of tests/test_norm_paths_gpu.py shown to be neither too tight nor
too loose: an emulation of every kernel's arithmetic (fp32 statistics, bf16 loads and stores, the expression order of the
kernel source) passes its checker, and each planted error fails it.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as nr
from tests import test_norm_paths_gpu as G

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS, MOM = G.EPS, G.MOMENTUM


def _close(a, b, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-12), (what, float((a - b).abs().max()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the reference against torch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D,share,with_dres", [(5, 8, 1, True), (12, 36, 3, False), (14, 260, 7, True)])
def test_layernorm_reference_equals_torch(M, D, share, with_dres):
    g = _gen(M * D)
    x = (torch.randn(M, D, generator=g, dtype=F64) + 3.0).requires_grad_(True)
    gamma, beta = (torch.randn(D, generator=g, dtype=F64).requires_grad_(True) for _ in range(2))
    dy = torch.randn(M // share, D, generator=g, dtype=F64)
    dres = torch.randn(M, D, generator=g, dtype=F64) if with_dres else None
    y = F.layer_norm(x, (D,), gamma, beta, EPS)
    (y * dy.repeat_interleave(share, 0)).sum().backward()
    ry, mean, rstd, m = nr.ln_fwd(x.detach(), gamma.detach(), beta.detach(), EPS)
    _close(ry, y.detach(), "y")
    _close(mean, x.detach().mean(1), "mean")
    _close(rstd, 1.0 / torch.sqrt(x.detach().var(1, unbiased=False) + EPS), "rstd")
    dx, dg, db, mb = nr.ln_bwd(dy, x.detach(), gamma.detach(), dres, share, mean=mean, rstd=rstd)
    _close(dx, x.grad + (dres if with_dres else 0.0), "dx")
    _close(dg, gamma.grad, "dgamma")
    _close(db, beta.grad, "dbeta")
    dx2, _, _, _ = nr.ln_bwd(dy, x.detach(), gamma.detach(), dres, share, eps=EPS)          # statistics of x by default
    _close(dx2, dx, "dx (default statistics)")
    assert (ry.abs() <= m["y"] * (1 + 1e-12)).all() and (dx.abs() <= mb["dx"] * (1 + 1e-12) + 1e-300).all()
    assert (dg.abs() <= mb["dgamma"] * (1 + 1e-12)).all() and (db.abs() <= mb["dbeta"] * (1 + 1e-12)).all()


def test_batchnorm_reference_equals_torch_batch_norm():
    R, C = 37, 12
    g = _gen(1)
    x = (torch.randn(R, C, generator=g, dtype=F64) * 2 + 1).requires_grad_(True)
    gamma, beta = (torch.randn(C, generator=g, dtype=F64).requires_grad_(True) for _ in range(2))
    rm, rv = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.5
    dz = torch.randn(R, C, generator=g, dtype=F64)
    trm, trv = rm.clone(), rv.clone()
    z = F.batch_norm(x, trm, trv, gamma, beta, True, MOM, EPS)
    (z * dz).sum().backward()
    w = nr.window_weights(R, 0, 0, 0)
    xd, gd, bd = x.detach(), gamma.detach(), beta.detach()
    s0, s1, _ = nr.bn_sums(xd, w)
    mean, var, rstd, rm1, rv1 = nr.bn_finalize(s0, s1, R, EPS, MOM, rm, rv)
    _close(rm1, trm, "running_mean")
    _close(rv1, trv, "running_var")
    rz, m = nr.bn_apply(xd, w, mean, rstd, gd, bd)
    _close(rz, z.detach(), "z")
    b0, b1, _ = nr.bn_bwd_sums(dz, xd, w, mean, rstd)
    dy, md = nr.bn_bwd_apply(dz, xd, w, mean, rstd, gd, b0, b1, 1.0 / R)
    _close(dy, x.grad, "dx")
    _close(b1, gamma.grad, "dgamma")
    _close(b0, beta.grad, "dbeta")
    assert (rz.abs() <= m["z"] * (1 + 1e-12)).all() and (m["z"] <= m["folded"] * (1 + 1e-12)).all()
    assert (dy.abs() <= md["dy"] * (1 + 1e-12)).all()


@pytest.mark.parametrize("relu", [False, True])
def test_weighted_batchnorm_reference_equals_autograd_through_the_expanded_matrix(relu):
    """Rows repeated m times, excluded rows dropped, context rows computed with the statistics of the others; the gradients
    of the copies are summed back."""
    R, C = 23, 6
    g = _gen(2)
    w = torch.tensor([-1, -1, 1, 3, 0, 1, 2, -1, 0, 3, 1, 1, 0, -1, 2, 1, 1, 3, 0, 1, -1, -1, -1], dtype=F64)
    x = torch.randn(R, C, generator=g, dtype=F64) + 0.5
    gamma, beta = (torch.randn(C, generator=g, dtype=F64) for _ in range(2))
    dz = torch.randn(R, C, generator=g, dtype=F64)          # a row's dz: the sum over its copies
    n = int(w.clamp_min(0).sum())
    X, Gm, Bt = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    stat_idx = torch.cat([torch.full((int(m),), r) for r, m in enumerate(w.tolist()) if m > 0])
    Xe = X[stat_idx]
    mean_t, var_t = Xe.mean(0), Xe.var(0, unbiased=False)
    # every copy of a row takes dz / m; a context row is one row outside the statistics
    rows = torch.cat([stat_idx, torch.nonzero(w == 0).flatten()])
    dze = torch.cat([(dz / w.clamp_min(1)[:, None])[stat_idx], dz[w == 0]])
    Z = (X[rows] - mean_t) / torch.sqrt(var_t + EPS) * Gm + Bt
    if relu:
        Z = Z.clamp_min(0.0)
    (Z * dze).sum().backward()
    s0, s1, _ = nr.bn_sums(x, w)
    mean, var, rstd, _, _ = nr.bn_finalize(s0, s1, n, EPS)
    _close(mean, mean_t.detach(), "mean")
    _close(var, var_t.detach(), "var")
    z, _ = nr.bn_apply(x, w, mean, rstd, gamma, beta, relu=relu)
    ze = torch.zeros_like(z)
    ze[rows] = Z.detach()
    _close(z, ze, "z")
    assert (z[w < 0] == 0).all()
    if relu:
        dy, b0, b1, _ = nr.bn_relu_bwd(dz, x, mean, rstd, gamma, beta, 1.0 / n, w)
    else:
        b0, b1, _ = nr.bn_bwd_sums(dz, x, w, mean, rstd)
        dy, _ = nr.bn_bwd_apply(dz, x, w, mean, rstd, gamma, b0, b1, 1.0 / n)
    _close(dy, X.grad, "dx")
    assert (dy[w < 0] == 0).all()
    _close(b1, Gm.grad, "dgamma")
    _close(b0, Bt.grad, "dbeta")


def test_tail_expansion_and_relu_mask():
    x = torch.arange(2 * 5 * 3, dtype=F64).reshape(10, 3)
    xe, idx = nr.bn_tail_expand(x, 5, 3, 2)
    assert idx.tolist() == [0, 1, 2, 3, 4, 3, 4, 5, 6, 7, 8, 9, 8, 9] and torch.equal(xe, x[idx])
    assert nr.tail_weights(10, 5, 3, 2).tolist() == [1, 1, 1, 2, 2] * 2
    assert nr.window_weights(8, 4, 1, 2).tolist() == [-1, 1, 1, -1] * 2
    # relu_mask: the gradient of max(0, .) in front of the BatchNorm (y is that ReLU's output)
    g = _gen(3)
    pre = torch.randn(9, 4, generator=g, dtype=F64).requires_grad_(True)
    gamma, dz = torch.randn(4, generator=g, dtype=F64), torch.randn(9, 4, generator=g, dtype=F64)
    y = pre.clamp_min(0.0)
    mean, var = y.mean(0), y.var(0, unbiased=False)
    (((y - mean) / torch.sqrt(var + EPS) * gamma) * dz).sum().backward()
    w = nr.window_weights(9, 0, 0, 0)
    yd = y.detach()
    rstd = 1.0 / torch.sqrt(var.detach() + EPS)
    b0, b1, _ = nr.bn_bwd_sums(dz, yd, w, mean.detach(), rstd)
    dy, _ = nr.bn_bwd_apply(dz, yd, w, mean.detach(), rstd, gamma, b0, b1, 1.0 / 9, relu_mask=True)
    _close(dy, pre.grad, "relu_mask")


# ---- emulations of the kernels' arithmetic ------------------------------------------------------------------------------------
def emu_ln_fwd(x, gamma, beta, eps, denom=None):
    v = x.float()
    D = v.shape[1]
    mean = v.sum(1) / D
    d = v - mean[:, None]
    var = (d * d).sum(1) / (denom or D)
    rstd = torch.rsqrt(var + eps)
    return (d * rstd[:, None] * gamma + beta).to(x.dtype), mean, rstd


def emu_ln_bwd(dy, x, mean, rstd, gamma, dres, share, modulo=False):
    M, D = x.shape
    r = torch.arange(M)
    dv = dy.float()[r % share if modulo else r // share]
    xh = (x.float() - mean[:, None]) * rstd[:, None]
    gg = dv * gamma
    c1 = gg.sum(1, keepdim=True) / D
    c2 = (gg * xh).sum(1, keepdim=True) / D
    o = rstd[:, None] * (gg - c1 - xh * c2)
    if dres is not None:
        o = o + dres.float()
    return o.to(x.dtype), (dv * xh).sum(0), dv.sum(0)


def emu_bn_sums(y, w):
    sel = w > 0
    v, ws = y[sel].float(), w[sel].float()[:, None]
    t = v * ws
    return torch.cat([t.sum(0), (t * v).sum(0)])


def emu_bn_finalize(sums, n, eps, mom, rm, rv):
    C = sums.numel() // 2
    inv_n = G.f32(1.0 / n)
    m = sums[:C] * inv_n
    v = (sums[C:] * inv_n - m * m).clamp_min(0.0)
    unbias = G.f32(n / (n - 1.0)) if n > 1 else 1.0
    return m, v, torch.rsqrt(v + eps), (1.0 - mom) * rm + mom * m, (1.0 - mom) * rv + mom * (v * unbias)


def emu_bn_apply(y, w, mean, rstd, gamma, beta, wide, relu=False):
    keep = (w >= 0)[:, None]
    v = torch.where(keep, y.float(), torch.zeros((), dtype=F32))
    if wide:
        a = rstd * gamma
        o = v * a + (beta - mean * a)
    else:
        o = (v - mean) * rstd * gamma + beta
    if relu:
        o = o.clamp_min(0.0)
    return torch.where(keep, o, torch.zeros((), dtype=F32)).to(y.dtype)


def emu_bn_bwd_sums(dz, y, w, mean, rstd, gamma=None, beta=None):
    keep = w >= 0
    d, yh = dz[keep].float(), (y[keep].float() - mean) * rstd
    if gamma is not None:
        d = torch.where(yh * gamma + beta > 0, d, torch.zeros((), dtype=F32))
    return torch.cat([d.sum(0), (d * yh).sum(0)])


def emu_bn_bwd_apply(dz, y, w, mean, rstd, gamma, sums, inv_n, relu_mask, weighted, beta=None):
    C = y.shape[1]
    keep = (w >= 0)[:, None]
    d = torch.where(keep, dz.float(), torch.zeros((), dtype=F32))
    yv = torch.where(keep, y.float(), torch.zeros((), dtype=F32))
    yh = (yv - mean) * rstd
    if beta is not None:
        d = torch.where(yh * gamma + beta > 0, d, torch.zeros((), dtype=F32))
    s0, s1 = sums[:C], sums[C:]
    if weighted:
        o = gamma * rstd * (d - (s0 * inv_n + yh * (s1 * inv_n)) * w.float()[:, None])
    else:
        o = gamma * rstd * (d - s0 * inv_n - yh * (s1 * inv_n))
    if relu_mask:
        o = torch.where(yv > 0, o, torch.zeros((), dtype=F32))
    return torch.where(keep, o, torch.zeros((), dtype=F32)).to(y.dtype)


def emu_tail_fix(dy, y, mean, rstd, gamma, sums, inv_n, wmul, LP, lead):
    C = y.shape[1]
    tail = (torch.arange(y.shape[0]) % LP) >= lead
    xh = (y.float() - mean) * rstd
    fixed = dy.float() - (wmul - 1.0) * gamma * rstd * (sums[:C] * inv_n + xh * sums[C:] * inv_n)
    return torch.where(tail[:, None], fixed.to(dy.dtype), dy)


def _ln_operands(dt, M, D, data, seed, share=1, with_dres=True):
    g = _gen(seed)
    xv, const = G.ln_data(data, M, D, g)
    x = xv.to(dt)
    gamma, beta = 1.0 + 0.5 * torch.randn(D, generator=g), 0.5 * torch.randn(D, generator=g)
    dy = torch.randn(M // share, D, generator=g).to(dt)
    dres = (0.5 * torch.randn(M, D, generator=g)).to(dt) if with_dres else None
    return x, gamma, beta, dy, dres, const


@pytest.mark.parametrize("dt,M,D,data,share", [(BF, 33, 256, "randn", 1), (BF, 17, 512, "const", 1), (BF, 9, 2048, "offset", 1),
                                              (BF, 63, 264, "spike", 7), (BF, 12, 36, "tiny", 1), (F32, 7, 2048, "offset", 1),
                                              (F32, 9, 260, "const", 1), (F32, 60, 1024, "spike", 12), (F32, 130, 4, "tiny", 1),
                                              (F32, 31, 512, "randn", 1)])
def test_layernorm_emulation_passes(dt, M, D, data, share):
    x, gamma, beta, dy, dres, const = _ln_operands(dt, M, D, data, M + D, share)
    y, mean, rstd = emu_ln_fwd(x, gamma, beta, EPS)
    G.check_ln_fwd("emu", dt, x, gamma, beta, EPS, y, mean, rstd, const)
    _, rmean, rrstd, _ = nr.ln_fwd(x, gamma, beta, EPS)
    m32, r32 = rmean.float(), rrstd.float()
    dx, dg, db = emu_ln_bwd(dy, x, m32, r32, gamma, dres, share)
    assert torch.isfinite(dx.float()).all()
    G.check_ln_bwd("emu", dt, dy, x, m32, r32, gamma, dres, share, dx, dg, db)


def _bn_operands(dt, R, C, data, seed):
    g = _gen(seed)
    y = G.bn_data(data, R, C, g).to(dt)
    dz = torch.randn(R, C, generator=g).to(dt)
    gamma, beta = 1.0 + 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return y, dz, gamma, beta, rm, rv


def _rw(R, seed):
    w = torch.tensor([-1.0, 0.0, 1.0, 3.0])[torch.randint(0, 4, (R,), generator=_gen(seed))]
    w[:5], w[-7:] = -1.0, -1.0
    w[5:8] = torch.tensor([3.0, 0.0, 1.0])
    return w.double()


BN_EMU = [(BF, 64, "none", 40000, "relu"), (BF, 128, "none", 33, "offset"), (BF, 96, "none", 31, "const"), (BF, 64, "none", 3000, "relu"), (BF, 72, (40, 4, 32, 5), None, "randn"),
          (BF, 256, (37, 3, 31, 7), None, "spike"), (BF, 128, "rw", 100, "relu"), (BF, 260, "rw", 77, "tiny"), (F32, 4, "none", 33, "offset"),
          (F32, 260, "rw", 50, "spike"), (F32, 128, (136, 128, 8, 4), None, "const"), (F32, 128, "none", 1, "randn")]


@pytest.mark.parametrize("dt,C,rule,R,data", BN_EMU)
def test_batchnorm_emulation_passes(dt, C, rule, R, data):
    if isinstance(rule, tuple):
        R = rule[0] * rule[3]
        w = nr.window_weights(R, *rule[:3])
    else:
        w = _rw(R, C) if rule == "rw" else torch.ones(R, dtype=F64)
    weighted = rule == "rw"
    wide = dt == BF and C in (64, 128, 256)
    y, dz, gamma, beta, rm, rv = _bn_operands(dt, R, C, data, R + C)
    y[w < 0] = float("nan")
    dz[w < 0] = float("nan")
    n = int(w.clamp_min(0).sum())
    sums = emu_bn_sums(y, w)
    G.check_bn_sums("emu", "stats", y, w, sums)
    mean, var, rstd, rm1, rv1 = emu_bn_finalize(sums, n, EPS, MOM, rm, rv)
    G.check_bn_finalize("emu", "finalize", n, EPS, MOM, rm, rv, mean, var, rstd, rm1, rv1, sums=sums)
    G.check_bn_finalize("emu", "stats_finalize", n, EPS, MOM, rm, rv, mean, var, rstd, rm1, rv1, y=y, w=w, sums_out=sums)
    z = emu_bn_apply(y, w, mean, rstd, gamma, beta, wide)
    G.check_bn_apply("emu", "apply", dt, wide, y, w, mean, rstd, gamma, beta, z)
    bs = emu_bn_bwd_sums(dz, y, w, mean, rstd)
    G.check_bn_bwd_sums("emu", "bwd_reduce", dz, y, w, mean, rstd, bs)
    inv_n = G.f32(1.0 / n)
    for relu_mask in (0, 1):
        dy = emu_bn_bwd_apply(dz, y, w, mean, rstd, gamma, bs, inv_n, relu_mask, weighted)
        assert torch.isfinite(dy.float()).all()
        G.check_bn_bwd_apply("emu", "bwd_apply", dt, dz, y, w, mean, rstd, gamma, bs, inv_n, relu_mask, dy)


@pytest.mark.parametrize("dt,C,R,data", [(BF, 512, 200, "randn"), (BF, 128, 33, "offset"), (F32, 260, 31, "tiny"), (F32, 4, 1000, "spike"),
                                         (BF, 72, 3000, "relu")])
def test_batchnorm_relu_emulation_passes(dt, C, R, data):
    y, dz, gamma, beta, _, _ = _bn_operands(dt, R, C, data, R * C)
    w = torch.ones(R, dtype=F64)
    s0, s1, _ = nr.bn_sums(y, w)
    mean, _, rstd, _, _ = nr.bn_finalize(s0, s1, R, EPS)
    mean, rstd = mean.float(), rstd.float()
    z = emu_bn_apply(y, w, mean, rstd, gamma, beta, False, relu=True)
    G.check_bn_apply("emu", "apply_relu", dt, False, y, w, mean, rstd, gamma, beta, z, relu=True)
    sums = emu_bn_bwd_sums(dz, y, w, mean, rstd, gamma, beta)
    sb = G.check_bn_bwd_sums("emu", "relu_bwd", dz, y, w, mean, rstd, sums, gamma, beta)
    inv_n = G.f32(1.0 / R)
    dy = emu_bn_bwd_apply(dz, y, w, mean, rstd, gamma, sums, inv_n, 0, False, beta=beta)
    r0, r1, _ = nr.bn_bwd_sums(dz, y, w, mean, rstd, gamma, beta)
    G.check_bn_bwd_apply("emu", "relu_bwd dy", dt, dz, y, w, mean, rstd, gamma, torch.cat([r0, r1]), inv_n, 0, dy, beta=beta, sums_bound=sb)


def _tail_operands(dt, C, B, LP, lead, wmul, data, seed):
    R = B * LP
    y, dz, gamma, beta, rm, rv = _bn_operands(dt, R, C, data, seed)
    w = nr.tail_weights(R, LP, lead, wmul)
    n = int(w.sum())
    s0, s1, _ = nr.bn_sums(y, w)
    mean, _, rstd, _, _ = nr.bn_finalize(s0, s1, n, EPS)
    mean, rstd = mean.float(), rstd.float()
    sums = emu_bn_bwd_sums(dz, y, torch.ones(R, dtype=F64), mean, rstd)
    return y, dz, gamma, w, n, mean, rstd, sums


@pytest.mark.parametrize("dt,C,B,LP,lead,wmul,data", [(BF, 128, 4, 136, 128, 48, "relu"), (BF, 72, 3, 21, 16, 5, "offset"), (F32, 260, 3, 21, 16, 1, "randn"),
                                                      (BF, 72, 3, 21, 16, 1, "randn")])
def test_tail_fix_emulation_passes(dt, C, B, LP, lead, wmul, data):
    y, dz, gamma, w, n, mean, rstd, sums = _tail_operands(dt, C, B, LP, lead, wmul, data, C + wmul)
    inv_n = G.f32(1.0 / n)
    once = emu_bn_bwd_apply(dz, y, torch.ones_like(w), mean, rstd, gamma, sums, inv_n, 0, False)
    dy = emu_tail_fix(once, y, mean, rstd, gamma, sums, inv_n, wmul, LP, lead)
    G.check_bn_bwd_apply("emu", "tail_fix", dt, dz, y, w, mean, rstd, gamma, sums, inv_n, 0, dy, stores=2)


def _emu_function(x, gamma, beta, dz, LP, lead, wmul, relu, rm, rv, wide):
    """BatchNormRowsFn (wmul = 1) / BatchNormWeightedTailFn on the emulated kernels."""
    R, C = x.shape
    w = nr.tail_weights(R, LP, lead, wmul)
    n = int(w.sum())
    q = torch.arange(R) % LP
    if wmul == 1:
        sums = emu_bn_sums(x, w)
    else:
        sums = emu_bn_sums(x[q < lead], torch.ones(int((q < lead).sum()), dtype=F64)) + float(wmul) * emu_bn_sums(
            x[q >= lead], torch.ones(int((q >= lead).sum()), dtype=F64))
    mean, var, rstd, rm1, rv1 = emu_bn_finalize(sums, n, EPS, MOM, rm, rv)
    ones = torch.ones(R, dtype=F64)
    y = emu_bn_apply(x, ones, mean, rstd, gamma, beta, wide and not relu, relu=relu)
    inv_n = G.f32(1.0 / n)
    bs = emu_bn_bwd_sums(dz, x, ones, mean, rstd, gamma if relu else None, beta if relu else None)
    dx = emu_bn_bwd_apply(dz, x, ones, mean, rstd, gamma, bs, inv_n, 0, False, beta=beta if relu else None)
    if wmul != 1 or LP != lead:
        dx = emu_tail_fix(dx, x, mean, rstd, gamma, bs, inv_n, wmul, LP, lead)
    return dict(y=y, dx=dx, dgamma=bs[C:], dbeta=bs[:C], mean=mean, var=var, rmean=rm1, rvar=rv1)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dt,C,B,LP,lead,wmul,data", [(BF, 128, 1, 200, 200, 1, "relu"), (BF, 96, 1, 33, 33, 1, "offset"), (F32, 260, 1, 50, 50, 1, "randn"),
                                                      (BF, 128, 4, 136, 128, 48, "relu"), (BF, 72, 3, 21, 16, 5, "randn"), (F32, 132, 3, 21, 16, 5, "offset")])
def test_end_to_end_emulation_passes(dt, C, B, LP, lead, wmul, data, relu):
    x, dz, gamma, beta, rm, rv = _bn_operands(dt, B * LP, C, data, C + wmul)
    wide = dt == BF and C in (64, 128, 256)
    got = _emu_function(x, gamma, beta, dz, LP, lead, wmul, relu, rm, rv, wide)
    tail = LP != lead
    G.check_e2e("emu", dt, wide and not relu, x, gamma, beta, dz, LP, lead, wmul, relu, EPS, MOM, rm, rv, got,
                extra_tau=3 * G.U_F if tail else 0.0, stores=2 if tail else 1)


def test_end_to_end_reference_equals_norm_ref():
    """The autograd reference of the end-to-end test and the formulas of norm_ref agree (weighted tail, ReLU)."""
    B, LP, lead, wmul, C = 3, 7, 4, 5, 6
    x, dz, gamma, beta, _, _ = (t.double() for t in _bn_operands(F32, B * LP, C, "randn", 5))
    ry, rdx, rdg, rdb, rmean, rvar = G.e2e_reference(x, gamma, beta, dz, LP, lead, wmul, True, EPS)
    w = nr.tail_weights(B * LP, LP, lead, wmul)
    n = int(w.sum())
    s0, s1, _ = nr.bn_sums(x, w)
    mean, var, rstd, _, _ = nr.bn_finalize(s0, s1, n, EPS)
    _close(mean, rmean)
    _close(var, rvar)
    _close(nr.bn_apply(x, w, mean, rstd, gamma, beta, relu=True)[0], ry)
    dy, b0, b1, _ = nr.bn_relu_bwd(dz, x, mean, rstd, gamma, beta, 1.0 / n, w)
    _close(dy, rdx)
    _close(b1, rdg)
    _close(b0, rdb)


# ---- planted errors: each must fail its checker ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,C", [(BF, 128), (BF, 72), (F32, 4)])
def test_a_window_shifted_by_one_row_fails(dt, C):
    win, halo, valid, nwin = 40, 4, 32, 5
    R = win * nwin
    y, dz, gamma, beta, rm, rv = _bn_operands(dt, R, C, "randn", C)        # halo rows hold finite values here: the rule alone is wrong
    w = nr.window_weights(R, win, halo, valid)
    shifted = nr.window_weights(R, win, halo + 1, valid)
    wide = dt == BF and C in (64, 128, 256)
    G.check_bn_sums("ok", "stats", y, w, emu_bn_sums(y, w))
    with pytest.raises(AssertionError, match="rounding bound"):
        G.check_bn_sums("shifted", "stats", y, w, emu_bn_sums(y, shifted))
    s0, s1, _ = nr.bn_sums(y, w)
    mean, _, rstd, _, _ = nr.bn_finalize(s0, s1, valid * nwin, EPS)
    mean, rstd = mean.float(), rstd.float()
    with pytest.raises(AssertionError):
        G.check_bn_apply("shifted", "apply", dt, wide, y, w, mean, rstd, gamma, beta, emu_bn_apply(y, shifted, mean, rstd, gamma, beta, wide))
    bs = emu_bn_bwd_sums(dz, y, w, mean, rstd)
    with pytest.raises(AssertionError, match="rounding bound"):
        G.check_bn_bwd_sums("shifted", "bwd_reduce", dz, y, w, mean, rstd, emu_bn_bwd_sums(dz, y, shifted, mean, rstd))
    with pytest.raises(AssertionError):
        G.check_bn_bwd_apply("shifted", "bwd_apply", dt, dz, y, w, mean, rstd, gamma, bs, G.f32(1.0 / (valid * nwin)), 0,
                             emu_bn_bwd_apply(dz, y, shifted, mean, rstd, gamma, bs, G.f32(1.0 / (valid * nwin)), 0, False))


@pytest.mark.parametrize("dt,C,B,LP,lead,wmul", [(BF, 128, 4, 136, 128, 48), (BF, 72, 3, 21, 16, 5), (F32, 260, 3, 21, 16, 5)])
def test_tail_rows_taking_the_mean_terms_once_fail(dt, C, B, LP, lead, wmul):
    y, dz, gamma, w, n, mean, rstd, sums = _tail_operands(dt, C, B, LP, lead, wmul, "randn", C)
    inv_n = G.f32(1.0 / n)
    once = emu_bn_bwd_apply(dz, y, torch.ones_like(w), mean, rstd, gamma, sums, inv_n, 0, False)
    with pytest.raises(AssertionError, match="rounding bound"):
        G.check_bn_bwd_apply("once", "tail_fix", dt, dz, y, w, mean, rstd, gamma, sums, inv_n, 0, once, stores=2)


@pytest.mark.parametrize("dt,M,D", [(BF, 33, 256), (BF, 9, 2048), (F32, 7, 260)])
def test_variance_over_d_minus_one_fails(dt, M, D):
    x, gamma, beta, _, _, _ = _ln_operands(dt, M, D, "randn", D)
    y, mean, rstd = emu_ln_fwd(x, gamma, beta, EPS, denom=D - 1)
    with pytest.raises(AssertionError, match="rstd exceeds"):
        G.check_ln_fwd("dm1", dt, x, gamma, beta, EPS, y, mean, rstd)
    # with the statistics taken as right, the output alone gives it away (fp32: element-wise; bf16: the scale bias).  At
    # D = 2048 the error of rstd (1 / 2D) is below what M D bf16 roundings average out to: there rstd is the witness.
    if D > 260:
        return
    _, good_mean, good_rstd = emu_ln_fwd(x, gamma, beta, EPS)
    with pytest.raises(AssertionError, match="y (exceeds|carries a scale error)"):
        G.check_ln_fwd("dm1", dt, x, gamma, beta, EPS, y, good_mean, good_rstd)


@pytest.mark.parametrize("dt,M,D,share", [(BF, 63, 256, 7), (F32, 56, 260, 7)])
def test_dy_share_modulo_instead_of_division_fails(dt, M, D, share):
    x, gamma, beta, dy, dres, _ = _ln_operands(dt, M, D, "randn", M, share)
    _, rmean, rrstd, _ = nr.ln_fwd(x, gamma, beta, EPS)
    dx, dg, db = emu_ln_bwd(dy, x, rmean.float(), rrstd.float(), gamma, dres, share, modulo=True)
    with pytest.raises(AssertionError, match="dx exceeds"):
        G.check_ln_bwd("mod", dt, dy, x, rmean.float(), rrstd.float(), gamma, dres, share, dx, dg, db)


def _two_ulps(t, ref, mag):
    """Move one bf16 element by two ulps away from the reference: the first element that is no cancellation (|ref| >= mag / 2)
    and sits in the lower quarter of its binade (where two ulps are the largest fraction of the value).  This is the bound at its
    tightest and the only place where a two-ulp move is certain to be caught: with MARGIN = 2 the bound is 2 u_b mag = 2^-7
    mag, two ulps of a value v in [2^e, 2^(e+1)) are 2^(e-6), so near the top of a binade, or where v is a cancellation of
    larger terms (mag > |v|), a two-ulp error sits at or inside the bound by the rounding model's own terms."""
    flat = t.reshape(-1).clone()
    r, m = ref.reshape(-1), mag.reshape(-1)
    mant = r.abs() / torch.exp2(torch.floor(torch.log2(r.abs().clamp_min(1e-300))))
    i = int(torch.nonzero((r.abs() >= 0.5 * m) & (mant < 1.25) & (r.abs() > 1e-3))[0])
    bits = flat.view(torch.int16)
    up = (flat[i].double() >= r[i]) == (flat[i] > 0)           # growing the magnitude moves away from the reference
    bits[i] += 2 if up else -2
    return flat.reshape(t.shape), i


def test_one_element_moved_by_two_bf16_ulps_fails():
    x, gamma, beta, dy, dres, _ = _ln_operands(BF, 33, 256, "randn", 7)
    y, mean, rstd = emu_ln_fwd(x, gamma, beta, EPS)
    ry, _, _, m = nr.ln_fwd(x, gamma, beta, EPS)
    G.check_ln_fwd("ok", BF, x, gamma, beta, EPS, y, mean, rstd)
    y2, _ = _two_ulps(y, ry, m["y"])
    with pytest.raises(AssertionError, match="y exceeds"):
        G.check_ln_fwd("ulp", BF, x, gamma, beta, EPS, y2, mean, rstd)
    # BatchNorm apply (wide form) and backward apply
    R, C = 77, 128
    yb, dz, gamma, beta, _, _ = _bn_operands(BF, R, C, "randn", 9)
    w = torch.ones(R, dtype=F64)
    s0, s1, _ = nr.bn_sums(yb, w)
    mean, _, rstd, _, _ = nr.bn_finalize(s0, s1, R, EPS)
    mean, rstd = mean.float(), rstd.float()
    z = emu_bn_apply(yb, w, mean, rstd, gamma, beta, True)
    rz, mz = nr.bn_apply(yb, w, mean, rstd, gamma, beta)
    z2, _ = _two_ulps(z, rz, mz["z"])
    with pytest.raises(AssertionError, match="rounding bound"):
        G.check_bn_apply("ulp", "apply", BF, True, yb, w, mean, rstd, gamma, beta, z2)
    bs = emu_bn_bwd_sums(dz, yb, w, mean, rstd)
    inv_n = G.f32(1.0 / R)
    d = emu_bn_bwd_apply(dz, yb, w, mean, rstd, gamma, bs, inv_n, 0, False)
    rd, md = nr.bn_bwd_apply(dz, yb, w, mean, rstd, gamma, bs[:C], bs[C:], inv_n)
    d2, _ = _two_ulps(d, rd, md["dy"])
    with pytest.raises(AssertionError, match="rounding bound"):
        G.check_bn_bwd_apply("ulp", "bwd_apply", BF, dz, yb, w, mean, rstd, gamma, bs, inv_n, 0, d2)


@pytest.mark.parametrize("value", [1e-30, -0.0])
def test_a_halo_row_left_non_zero_fails(value):
    win, halo, valid, nwin, C = 37, 3, 31, 7, 72
    R = win * nwin
    y, dz, gamma, beta, _, _ = _bn_operands(BF, R, C, "randn", 4)
    w = nr.window_weights(R, win, halo, valid)
    s0, s1, _ = nr.bn_sums(y, w)
    mean, _, rstd, _, _ = nr.bn_finalize(s0, s1, valid * nwin, EPS)
    mean, rstd = mean.float(), rstd.float()
    z = emu_bn_apply(y, w, mean, rstd, gamma, beta, False)
    G.check_bn_apply("ok", "apply", BF, False, y, w, mean, rstd, gamma, beta, z)
    z[win + 1, 5] = value                                       # a halo row of the second window
    with pytest.raises(AssertionError, match="non-zero excluded row|rounding bound"):
        G.check_bn_apply("halo", "apply", BF, False, y, w, mean, rstd, gamma, beta, z)


# ---- the ReLU kink exclusion stays under its cap (reference alone) -------------------------------------------------------------
@pytest.mark.parametrize("data", ["randn", "offset", "relu", "spike", "tiny"])
@pytest.mark.parametrize("dt", [BF, F32])
def test_kink_exclusion_share_is_under_its_cap(data, dt):
    R, C = 4096, 256
    y, _, gamma, beta, _, _ = _bn_operands(dt, R, C, data, 11)
    w = torch.ones(R, dtype=F64)
    s0, s1, _ = nr.bn_sums(y, w)
    mean, _, rstd, _, _ = nr.bn_finalize(s0, s1, R, EPS)
    _, m = nr.bn_apply(y, w, mean.float(), rstd.float(), gamma, beta, relu=True)
    share = float(nr.kink(m["pre"], m["pre_mag"], G.KINK).double().mean())
    assert share <= G.KINK_CAP, share
    # the density of the pre-activation near zero (~0.4) times the band (~8e-6): a few elements in a million
    assert share <= 1e-4, share
