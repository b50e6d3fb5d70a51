"""fp64 reference of the classification loss of druglamp_amd/csrc/cls_loss.hip, the case table of
tests/test_cls_loss_paths_gpu.py and its data (no GPU needed: tests/test_cls_loss_reference_cpu.py pins all three).

Row i: z = score[i, 0] (one output) or score[i, 1] - score[i, 0] (two), y = labels[i], w = weights[i] (1 without weights),
    p = sigmoid(z), q = sigmoid(-z), s = y q - (1 - y) p (= y - p), d = |s|, m = d^gamma (gamma = 0: 1),
    B = a_pos y softplus(-z) + a_neg (1 - y) softplus(z),   l = w m B,   loss = sum l / den,
    den = N without weights, the sum of the VALID weights with (a negative or non-finite weight counts 0),
    d l / d z = w (dm B + m dB),  dm = -gamma d^(gamma - 1) sgn(s) p q (sgn(0) = 0),  dB = a_neg (1 - y) p - a_pos y q.
A row is `poisoned` when z is not finite, y is outside [0, 1] or not finite, or w is negative or not finite: its term and
its gradient are NaN (so the loss is NaN); `terms`, `dz` and the magnitudes hold 0 there and `loss_clean` is the loss of the
other rows over the same den, so that everything else can still be compared.  `flagged`: the rows with a bad label or weight
(the bad values that are host or label data, as opposed to a non-finite score).

Magnitudes (what a first-order rounding bound multiplies; see tests/test_cls_loss_paths_gpu.py):
    mag_s  = y q + (1 - y) p                         the terms of s (= d for hard labels: no cancellation)
    mag_l  = w B (m + gamma d^(gamma - 1) mag_s)     a relative error of m, B or w, and an absolute error of d through m
    mag_dB = a_pos y q + a_neg (1 - y) p
    mag_dz = w [gamma p q B (d^(gamma - 1) + (gamma - 1) d^(gamma - 2) mag_s) + mag_dB (m + gamma d^(gamma - 1) mag_s)]
    sens_l, sens_dz, sens_p = |z| |d l / d z|, |z| |d^2 l / d z^2|, |z| p q: what a relative error of z moves (the fp32
        difference of two outputs)
"""
import collections
import math

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
ONE_WG = 4096                    # csrc/cls_loss.hip CLS_ONE_WG_ROWS: the one-workgroup form's limit


def _softplus(t):
    """max(t, 0) + log1p(exp(-|t|)) in a form that autograd differentiates at t = 0 too (the max / abs form has a kink there)."""
    return torch.logaddexp(torch.zeros_like(t), t)


def _sigmoid_pair(z):
    """(sigmoid(z), sigmoid(-z)): both formed directly, neither as 1 - the other."""
    return torch.sigmoid(z), torch.sigmoid(-z)


def _pow(d, g):
    """d^g with 0^0 = 1, 0^positive = 0, and d^negative at d = 0 -> inf (only ever multiplied into a bound)."""
    if g == 0:
        return torch.ones_like(d)
    return torch.where(d > 0, d.clamp(min=1e-300) ** g, torch.full_like(d, 0.0 if g > 0 else float("inf")))


def z_of(score):
    s = score.to(F64)
    return s[:, 0] if s.shape[1] == 1 else s[:, 1] - s[:, 0]


def cls_loss(score, labels, weights, a_pos, a_neg, gamma, gout=1.0):
    """score (N, 1 | 2) in any dtype (read exactly), labels (N,), weights (N,) or None; a_pos, a_neg, gamma, gout python floats
    (the kernel's fp32 arguments: pass values that fp32 holds).  Everything in fp64."""
    z, y = z_of(score), labels.to(F64)
    N = z.shape[0]
    w = torch.ones(N, dtype=F64) if weights is None else weights.to(F64)
    bad_w = ~(torch.isfinite(w) & (w >= 0))
    bad_y = ~(torch.isfinite(y) & (y >= 0) & (y <= 1))
    bad_z = ~torch.isfinite(z)
    poisoned = bad_w | bad_y | bad_z
    ok = ~poisoned
    zz, yy, ww = torch.where(ok, z, torch.zeros_like(z)), torch.where(ok, y, torch.zeros_like(y)), torch.where(ok, w, torch.zeros_like(w))
    den = float(torch.where(bad_w, torch.zeros_like(w), w).sum()) if weights is not None else float(N)

    zz = zz.clone().requires_grad_(True)
    p, q = _sigmoid_pair(zz)
    sp_pos, sp_neg = _softplus(zz), _softplus(-zz)
    s = yy * q - (1 - yy) * p
    d = s.abs()
    pm1 = _pow(d, gamma - 1) if gamma != 0 else torch.zeros_like(d)
    m = pm1 * d if gamma != 0 else torch.ones_like(d)
    B = a_pos * yy * sp_neg + a_neg * (1 - yy) * sp_pos
    dB = a_neg * (1 - yy) * p - a_pos * yy * q
    dm = -gamma * pm1 * torch.sign(s) * p * q
    terms = ww * m * B
    dz = ww * (dm * B + m * dB)                                     # the closed form
    auto = torch.autograd.grad(terms.sum(), zz, retain_graph=True)[0]  # ... and autograd of the terms (compared in the CPU test)
    d2 = torch.autograd.grad(dz.sum(), zz, allow_unused=True)[0]
    d2 = torch.zeros_like(z) if d2 is None else d2
    with torch.no_grad():
        mag_s = yy * q + (1 - yy) * p
        pm2 = (gamma - 1) * _pow(d, gamma - 2) if gamma > 1 else torch.zeros_like(d)
        mterm = m + gamma * pm1 * mag_s
        mag_l = ww * B * mterm
        mag_dB = a_pos * yy * q + a_neg * (1 - yy) * p
        mag_dz = ww * (gamma * p * q * B * (pm1 + pm2 * mag_s) + mag_dB * mterm)
        gs = gout / den if den != 0 else float("nan")
        pz, qz = _sigmoid_pair(z)                                   # probs: sigmoid(z) by IEEE rules, poisoned rows included
        clean = float(terms.sum()) / den if den != 0 else float("nan")
        out = {
            "z": z, "den": den, "terms": terms.detach(), "loss_clean": clean,
            "loss": float("nan") if bool(poisoned.any()) else clean,
            "probs": pz, "dz": dz.detach(), "dz_autograd": auto, "grad": gs * dz.detach(),
            "poisoned": poisoned, "flagged": bad_w | bad_y,
            "d": d.detach(), "mag_s": mag_s, "mag_l": mag_l, "mag_dz": mag_dz, "mag_grad": abs(gs) * mag_dz, "gs": gs,
            "sens_l": z.abs().where(ok, torch.zeros_like(z)) * dz.detach().abs(), "sens_dz": zz.detach().abs() * d2.abs(),
            "sens_p": zz.detach().abs() * (p * q).detach(),
        }
    return out


# =================================================================================================================================
# The case table of tests/test_cls_loss_paths_gpu.py
# =================================================================================================================================
Case = collections.namedtuple("Case", "name N dt n_out ld weights gamma a data seed")
SIZES = (1, 63, 64, 65, 255, 256, 257, ONE_WG, ONE_WG + 1, 70001)     # wave, block, form and second-stage (> 256 partials) boundaries
GAMMAS = (0.0, 1.0, 2.0, 1.5)
ALPHAS = ((1.0, 1.0), (3.0, 1.0), (0.25, 0.75), (0.0, 1.0))


def _cases():
    cs, i = [], 0
    for N in SIZES:                      # every size with both dtypes and output counts; the other axes rotate, and ...
        for dt in (F32, BF):
            for n_out in (1, 2):
                cs.append(Case("n%d_%s_o%d" % (N, "bf16" if dt == BF else "f32", n_out), N, dt, n_out, n_out if i % 2 == 0 else 8,
                               (i // 2) % 2 == 1, GAMMAS[i % 4], ALPHAS[(i // 4 + i) % 4], "hard", 500 + i))
                i += 1
    # ... every value of every axis meets BOTH forms explicitly: the one-workgroup form at 257 rows, the two-stage form at 4097
    for N in (257, ONE_WG + 1):
        for k, (g, a) in enumerate((g, a) for g in GAMMAS for a in ALPHAS):
            dt, n_out = (F32, BF)[k % 2], 1 + (k // 2) % 2
            cs.append(Case("n%d_g%g_a%g_%g" % (N, g, a[0], a[1]), N, dt, n_out, (n_out, 8)[(k // 4) % 2], (k // 3) % 2 == 0, g, a,
                           "hard", 700 + 31 * k + N))
        cs.append(Case("n%d_soft" % N, N, F32, 1, 1, True, 2.0, (0.25, 0.75), "soft", 801 + N))
        cs.append(Case("n%d_soft_bf16_o2" % N, N, BF, 2, 8, False, 1.5, (3.0, 1.0), "soft", 803 + N))
        cs.append(Case("n%d_y_equals_p" % N, N, F32, 1, 8, True, 1.0, (1.0, 1.0), "yp", 805 + N))
        cs.append(Case("n%d_y_equals_p_bf16_o2" % N, N, BF, 2, 2, False, 1.0, (0.25, 0.75), "yp", 807 + N))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
YP_ROW = 3                               # the row with z = 0, y = 0.5 of the `yp` cases


def case_data(c):
    """(score (N, n_out) in c.dt, labels fp32 (N,), weights fp32 (N,) | None, gout) on the CPU.
    hard: z uniform over [-90, 90] with the extremes planted, labels 0 / 1;  soft: |z| <= 8, labels uniform in [0, 1] kept away
    from p (the sign of y - p must be the kernel's);  yp: hard rows plus one row with z = 0, y = 0.5 (y == p exactly).
    weights: uniform in [0, 4) with every fifth zero."""
    g = torch.Generator().manual_seed(c.seed)
    N = c.N
    zmax = 8.0 if c.data == "soft" else 90.0
    z = (torch.rand(N, generator=g, dtype=F64) * 2 - 1) * zmax
    if c.data != "soft":
        z[0] = zmax
        if N > 1:
            z[1] = -zmax
    if c.n_out == 1:
        score = z.unsqueeze(1)
    else:
        base = torch.randn(N, generator=g, dtype=F64) * 3
        score = torch.stack((base - z / 2, base + z / 2), 1)
    score = score.to(c.dt)
    y = (torch.rand(N, generator=g) < 0.3).to(F32)
    if N > 2:
        y[0], y[1] = 1.0, 0.0                                     # the confident-and-right tails: d underflows
    if c.data == "soft":
        y = torch.rand(N, generator=g).to(F32)
        p = torch.sigmoid(z_of(score)).to(F32)
        near = (y - p).abs() < 1e-3
        y = torch.where(near, (p + 0.25).clamp(max=1.0), y)
        y = torch.where(((y - p).abs() < 1e-3), (p - 0.25).clamp(min=0.0), y)
    if c.data == "yp" and N > YP_ROW:
        score[YP_ROW] = 0.0 if c.n_out == 1 else score[YP_ROW, 0]
        y[YP_ROW] = 0.5
    w = None
    if c.weights:
        w = (torch.rand(N, generator=g) * 4).to(F32)
        w[::5] = 0.0
        if N == 1:
            w[0] = 1.5
    gout = 0.75 + (c.seed % 7) * 0.125
    return score, y, w, gout


def conditions(c, r, y):
    """What the GPU test assumes of a case's data (asserted on the CPU): den > 0, no poisoned row, finite bounds, and the
    sign of y - p is decided far outside the rounding of s (or s is exactly 0)."""
    assert r["den"] > 0 and not bool(r["poisoned"].any()), c.name
    for k in ("mag_l", "mag_dz", "sens_l", "sens_dz"):
        assert bool(torch.isfinite(r[k]).all()), (c.name, k)
    d, ms = r["d"], r["mag_s"]
    assert bool(((d == 0) | (d > 256 * 2.0 ** -24 * ms) | (ms < 2.0 ** -100)).all()), c.name
    if c.data == "yp" and c.N > YP_ROW:
        assert float(d[YP_ROW]) == 0.0 and float(y[YP_ROW]) == 0.5, c.name
    if c.data == "soft":
        assert bool(((y > 0) & (y < 1)).any()) and float(d.min()) > 1e-4, c.name


# ---- bad inputs (tests/test_cls_loss_paths_gpu.py, second half) -------------------------------------------------------------------
BadCase = collections.namedtuple("BadCase", "name what value row flagged")
BAD_ROW = 5
BAD_CASES = [BadCase("z_nan", "z", float("nan"), BAD_ROW, False), BadCase("z_pinf", "z", float("inf"), BAD_ROW, False),
             BadCase("z_ninf", "z", float("-inf"), BAD_ROW, False),
             BadCase("label_m1", "y", -1.0, BAD_ROW, True), BadCase("label_2", "y", 2.0, BAD_ROW, True),
             BadCase("label_nan", "y", float("nan"), BAD_ROW, True),
             BadCase("weight_m1", "w", -1.0, BAD_ROW, True), BadCase("weight_inf", "w", float("inf"), BAD_ROW, True)]
BAD_SHAPES = ((300, F32, 1), (300, BF, 2), (ONE_WG + 1, F32, 2))          # both forms


def bad_data(b, N, dt, n_out):
    base = Case("bad", N, dt, n_out, n_out, True, 2.0, (0.25, 0.75), "hard", 900 + N)
    score, y, w, gout = case_data(base)
    if b.what == "z":
        score[b.row, n_out - 1] = b.value
    elif b.what == "y":
        y[b.row] = b.value
    else:
        w[b.row] = b.value
    return score, y, w, gout
