"""Every launch form of the LayerNorm kernels (norm.hip: dl_layernorm_fwd / dl_layernorm_bwd) and of the BatchNorm kernels
(bn.hip: bn_reduce<0/1>, bn_apply_fwd_run, bn_bwd_apply_run, dl_bn_tail_fix, dl_bn_finalize, dl_bn_stats_finalize,
dl_bn_apply_relu_fwd, dl_bn_relu_bwd) element-wise against the fp64 reference of tests/norm_ref.py:

    |got - ref| <= tau * mag          for every addressed element of every output,

with `mag` the sum of the absolute terms of the output's own expression (norm_ref returns it) and tau from the rounding
model below.  The kernels run through the C ABI (druglamp_amd._lib) exactly as the ops wrappers call it, on buffers this
test owns: everything outside the addressed rows and columns is NaN beforehand, inputs (pitch padding, the other column
slices of a wider tensor, rows past M, excluded / halo rows of y and dz: a stray read poisons the result) and outputs (an
addressed element must be overwritten, everything else bitwise unchanged; halo / excluded output rows exactly zero).
Every backward runs twice and must be bitwise repeatable.  The checkers (check_*) take plain tensors on any device:
tests/test_norm_reference_cpu.py runs them on CPU emulations of the kernels' arithmetic and on planted errors.

DL_NORM_BOUND_LOG=<file>: every check appends one JSON line (case, output, dtype, worst |err| / bound).

Forms (host dispatch of norm.hip / bn.hip)
  dl_layernorm_fwd   bf16, D in {256, 512}, ldx, ldy % 8 == 0, x, y, gamma, beta 16-byte aligned -> ln_fwd16_kernel<D>
                     (32 / 16 rows per workgroup: 2 / 1 rows per wave pass, 4 passes, 4 waves); else ln_fwd_kernel<T, NV>
                     with NV = 1, 2, 4, 8 for D <= 256, 512, 1024, 2048 (8 rows per workgroup).
  dl_layernorm_bwd   same test over dy, x, dx, dres (lds % 8, 16-byte bases) and gamma -> ln_bwd16_kernel<D>; else
                     ln_bwd_kernel<T, NV>; 32 rows per workgroup, partials [nb][2][D] -> dl_reduce_partials_kernel: one
                     launch for adjacent dgamma | dbeta, one each otherwise, none when both are null; with a dl_reduce_item
                     the partials are handed back and dl_reduce_batch reduces them.
  bn_reduce<MODE>    bf16, C in {64, 128, 256}, 16-byte bases -> bn_partial_wide_kernel<MODE>; else
                     bn_partial_kernel<T, MODE>; then dl_reduce_partials_kernel (its four-way loop runs beyond 192 chunks).
                     MODE 0: dl_bn_stats(_rw) and the first launch of dl_bn_stats_finalize (second: bn_reduce_finalize_kernel);
                     MODE 1: dl_bn_bwd_reduce(_rw).
  bn_apply_fwd_run   wide -> bn_apply_fwd_wide_kernel<C> (z = y a + b folded per column); else bn_apply_fwd_kernel<T>.
  bn_bwd_apply_run   wide -> bn_bwd_apply_wide_kernel<C>; else bn_bwd_apply_kernel<T>.
  dl_bn_apply_relu_fwd / dl_bn_relu_bwd   always the generic kernels (bn_apply_fwd_kernel<T, true>; bn_partial_kernel<T, 1>
                     with the ReLU's open set + dl_reduce_partials_kernel + bn_bwd_apply_kernel<T> with prelu_b).
  dl_bn_tail_fix     bn_tail_fix_kernel<T>, in place over dy.

Rounding model (first order; u_b = 2^-8 bf16 round to nearest, u_f = 2^-24 fp32; u_st = the output dtype's).  The reference
reads the kernel's own bf16 / fp32 operands, so inputs are exact; the apply and backward kernels take the fp32 mean, rstd
and sums the test passes in as exact operands, the statistics kernels are checked on their own.
  fp32 sum of N terms: relative (N + c) u_f of the sum of the absolute terms, N = D columns (LayerNorm) or the case's row
      count R (BatchNorm column sums and LayerNorm dgamma / dbeta over M rows), c the roundings of one term.
  LayerNorm forward: e_mean = (D + 2) u_f sum|x| / D.  var = sum (x - mean)^2 / D: (D + 4) u_f var + e_mean^2 (the mean's
      error moves every deviation alike; the cross term vanishes; the square is kept because it is all that is left on a
      constant row).  rstd: the interval rsqrt(var -+ e_var + eps) around the reference + 3 u_f.  y = xhat gamma + beta:
      (u_st + 4 u_f)(|xhat gamma| + |beta|) + |xhat gamma| e_rstd / rstd + rstd |gamma| e_mean.
  LayerNorm backward (mean, rstd given): dx = rstd (g - c1 - xhat c2) + dres, g = dy gamma, c1 = sum g / D, c2 = sum g xhat / D:
      (u_st + (D + 8) u_f) mag_dx.  dgamma = sum_r dy xhat, dbeta = sum_r dy: (M + 6) u_f of the absolute sums.
  BatchNorm sums (w y, w y^2; dz, dz yhat): (R + 6) u_f of the absolute sums.
  BatchNorm finalize: mean = s0 / n: tau_s + 2 u_f of E1 = sum w|y| / n (tau_s = the relative error of the sums it reads: 0 for
      dl_bn_finalize, whose sums are operands).  The batch variance is the one-pass E[y^2] - mean^2 in fp32, so its error is
      relative to the SECOND MOMENT E2 = sum w y^2 / n, not to the variance: (tau_s + 3 u_f) E2 + 2 |mean| e_mean + 3 u_f
      mean^2 (the `offset` data families keep a large mean / std so that this is what is tested).  rstd: the interval as
      above.  Running statistics: 3 / 4 u_f of (1 - m)|r| + m |new| plus m times the new value's error.
  BatchNorm apply: (u_st) (|yhat gamma| + |beta|) + 4 u_f x the terms of the form's own expression: the same for the generic
      form ((y - mean) rstd gamma + beta), (|y| + |mean|) |rstd gamma| + |beta| for the wide form (fma(y, a, beta - mean a)).
  BatchNorm backward apply: (u_st + 10 u_f) mag_dy; dl_bn_tail_fix re-rounds a stored dy in place: 2 u_st + 14 u_f.
  dl_bn_relu_bwd computes its sums itself: their error, times |gamma rstd| (1 + |yhat|) / n, is added to dy's bound.
tau = MARGIN x the first-order sum: the margin covers the second-order terms, and a recorded worst |err| / bound at or below
1 / MARGIN says a form stays inside the first-order model itself (profiles/norm_bound_margins.txt).
Scale bias: bf16 roundings are zero-mean, only the fp32-level part of a bound (`coherent`) can move an output coherently.
The least-squares scale s = sum (got - ref) ref / sum ref^2 must stay within sum coherent |ref| / sum ref^2 plus six
standard deviations of zero-mean errors of the remaining size (uniform over +-bound: variance bound^2 / 3).  The roundings
must be independent for that: the BatchNorm forward outputs, a function of (y, column) alone, are taken once per distinct y
of a column (half of a post-ReLU column is the one value 0, and 40000 bf16 rows hold each value many times over).
ReLU kink: an element whose fp64 pre-activation satisfies |yhat gamma + beta| <= 64 u_f (|yhat gamma| + |beta|) may open on
one side only; it is left out of the element-wise checks of the ReLU outputs and their gradients (its |dz| terms are added
to the bounds of the sums), and at most 1 element in 1000 may be left out per tensor (asserted).  End to end the
pre-activation is computed from the kernels' own statistics, so the band is widened by |gamma| times the error of yhat.
"""
import collections
import ctypes
import json
import math
import os

import pytest
import torch

from tests import norm_ref as nr

DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U_B, U_F, MARGIN = 2.0 ** -8, 2.0 ** -24, 2.0
KINK, KINK_CAP = 64 * U_F, 1e-3
EPS = float(torch.tensor(1e-5, dtype=F32))             # the fp32 value the C ABI receives
MOMENTUM = float(torch.tensor(0.1, dtype=F32))


def u_st(dt):
    return U_B if dt == BF else U_F


def f32(v):
    return float(torch.tensor(v, dtype=F32))


# ---- the check ---------------------------------------------------------------------------------------------------------------
def _log(case, what, dt, ratio):
    path = os.environ.get("DL_NORM_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "output": what, "dtype": str(dt).split(".")[1], "ratio": ratio}) + "\n")


def check(case, what, dt, got, ref, bound, coherent=None, skip=None, distinct=None):
    """|got - ref| <= bound element by element (skip: the kink elements left out, their share capped); coherent: the fp32-level
    part of `bound`, given where the scale-bias check applies; distinct: the elements that check runs over (one of every
    group of elements computed from identical operands, whose roundings are copies of each other, not independent)."""
    got = got.double()
    assert got.shape == ref.shape, "%s: %s has shape %s, reference %s" % (case, what, tuple(got.shape), tuple(ref.shape))
    if skip is not None:
        share = float(skip.double().mean()) if skip.numel() else 0.0
        _log(case, what + " kink share", dt, share)
        assert share <= KINK_CAP, "%s: %s leaves out %.3g of its elements at the ReLU kink" % (case, what, share)
        keep = ~skip
        got, ref, bound = got[keep], ref[keep], bound[keep]
        coherent = None if coherent is None else coherent[keep]
        distinct = None if distinct is None else distinct[keep]
    assert torch.isfinite(got).all(), "%s: %s has non-finite addressed elements" % (case, what)
    if got.numel() == 0:
        return
    err = got - ref
    ratio = float((err.abs() / (bound + 1e-300)).max())
    _log(case, what, dt, ratio)
    assert ratio <= 1.0, "%s: %s exceeds its rounding bound by x%.3g" % (case, what, ratio)
    if distinct is not None:
        err, ref, bound = err[distinct], ref[distinct], bound[distinct]
        coherent = None if coherent is None else coherent[distinct]
    den = float((ref * ref).sum())
    if coherent is not None and den > 0:
        s = float((err * ref).sum()) / den
        lim = (float((coherent * ref.abs()).sum()) + 6.0 * float((((bound - coherent) * ref) ** 2).sum().sqrt()) / math.sqrt(3.0)) / den
        _log(case, what + " bias", dt, abs(s) / lim)
        assert abs(s) <= lim, "%s: %s carries a scale error of %.3g (allowed %.3g)" % (case, what, s, lim)


def check_zero_rows(case, what, got, rows):
    """Halo / excluded output rows are exactly (+)zero."""
    z = got[rows]
    bits = z.contiguous().view(torch.int16 if z.dtype == BF else torch.int32)
    assert bool((bits == 0).all()), "%s: %s has a non-zero excluded row" % (case, what)


def _interval_rstd(var, rstd, e_var, eps):
    lo = 1.0 / torch.sqrt((var - e_var).clamp_min(0.0) + eps)
    hi = 1.0 / torch.sqrt(var + e_var + eps)
    return torch.maximum((lo - rstd).abs(), (hi - rstd).abs()) + MARGIN * 3 * U_F * rstd


# ---- LayerNorm checkers ------------------------------------------------------------------------------------------------------
def check_ln_fwd(case, dt, x, gamma, beta, eps, y, mean, rstd, const_rows=None):
    D = x.shape[1]
    ry, rmean, rrstd, m = nr.ln_fwd(x, gamma, beta, eps)
    e_mean = MARGIN * (D + 2) * U_F * m["mean"]
    e_var = MARGIN * (D + 4) * U_F * m["var"] + e_mean ** 2
    e_rstd = _interval_rstd(m["var"], rrstd, e_var, eps)
    coh = MARGIN * 4 * U_F * m["y"] + m["xg"] * (e_rstd / rrstd)[:, None] + m["carry"] * e_mean[:, None]
    check(case, "mean", F32, mean, rmean, e_mean)
    check(case, "rstd", F32, rstd, rrstd, e_rstd)
    check(case, "y", dt, y, ry, coh + MARGIN * u_st(dt) * m["y"], coh)
    if const_rows is not None and len(const_rows):
        # constant rows whose sums are exact in fp32 (values of a few bits): var = 0, rstd = eps^-1/2, y = beta to rounding.
        # This holds as long as the kernel's mean of such a row is the constant itself: the generic kernels divide the exact
        # sum by (float)D (correctly rounded), the 16-byte forms multiply by 1.0f / D with D a power of two.  A kernel that
        # multiplied by a rounded reciprocal (D = 36, 260) would need the rstd |gamma| e_mean term of the main bound here.
        b = beta.double().expand(len(const_rows), D)
        check(case, "rstd[const rows]", F32, rstd[const_rows], torch.full((len(const_rows),), eps ** -0.5, dtype=F64, device=x.device),
              MARGIN * 3 * U_F * rrstd[const_rows])
        check(case, "y[const rows]", dt, y[const_rows], b, MARGIN * (u_st(dt) + 4 * U_F) * b.abs())


def check_ln_bwd(case, dt, dy, x, mean, rstd, gamma, dres, share, dx, dgamma, dbeta):
    M, D = x.shape
    rdx, rdg, rdb, m = nr.ln_bwd(dy, x, gamma, dres, share, mean=mean, rstd=rstd)
    coh = MARGIN * (D + 8) * U_F * m["dx"]
    check(case, "dx", dt, dx, rdx, coh + MARGIN * u_st(dt) * m["dx"], coh)
    if dgamma is not None:
        check(case, "dgamma", F32, dgamma, rdg, MARGIN * (M + 6) * U_F * m["dgamma"])
        check(case, "dbeta", F32, dbeta, rdb, MARGIN * (M + 6) * U_F * m["dbeta"])


# ---- BatchNorm checkers ------------------------------------------------------------------------------------------------------
def tau_sum(R):
    return (R + 6) * U_F


def check_bn_sums(case, what, y, w, sums):
    R, C = y.shape
    s0, s1, m = nr.bn_sums(y, w)
    check(case, what + " s0", F32, sums[:C], s0, MARGIN * tau_sum(R) * m["s0"])
    check(case, what + " s1", F32, sums[C:], s1, MARGIN * tau_sum(R) * m["s1"])


def finalize_bounds(mean, var, rstd, E1, E2, tau_s, eps, n, momentum, rm0, rv0):
    """Bounds (MARGIN included) of mean / var / rstd / running statistics computed from sums of relative error tau_s."""
    e_mean = MARGIN * (tau_s + 2 * U_F) * E1
    e_var = MARGIN * ((tau_s + 3 * U_F) * E2 + 3 * U_F * mean * mean) + 2 * mean.abs() * e_mean
    out = {"mean": e_mean, "var": e_var, "rstd": _interval_rstd(var, rstd, e_var, eps)}
    unbias = n / (n - 1.0) if n > 1 else 1.0
    if rm0 is not None:
        out["rmean"] = MARGIN * 3 * U_F * ((1 - momentum) * rm0.double().abs() + momentum * mean.abs()) + momentum * e_mean
        out["rvar"] = MARGIN * 4 * U_F * ((1 - momentum) * rv0.double().abs() + momentum * var * unbias) + momentum * unbias * e_var
    return out


def check_bn_finalize(case, what, n, eps, momentum, rm0, rv0, mean, var, rstd, rm1, rv1, sums=None, y=None, w=None, sums_out=None,
                      extra_tau=0.0):
    """dl_bn_finalize (sums: the fp32 operands) or dl_bn_stats_finalize (y, w: the statistics come from the data)."""
    if sums is not None:
        C = sums.numel() // 2
        s0, s1 = sums[:C].double(), sums[C:].double()
        E1, E2, tau = s0.abs() / n, s1.abs() / n, 0.0
    else:
        C = y.shape[1]
        s0, s1, m = nr.bn_sums(y, w)
        E1, E2, tau = m["s0"] / n, m["s1"] / n, tau_sum(y.shape[0]) + extra_tau
        if sums_out is not None:
            check(case, what + " s0", F32, sums_out[:C], s0, MARGIN * tau * m["s0"])
            check(case, what + " s1", F32, sums_out[C:], s1, MARGIN * tau * m["s1"])
    rmean, rvar, rrstd, rrm, rrv = nr.bn_finalize(s0, s1, n, eps, momentum, rm0, rv0)
    b = finalize_bounds(rmean, rvar, rrstd, E1, E2, tau, eps, n, momentum, rm0, rv0)
    check(case, what + " mean", F32, mean, rmean, b["mean"])
    check(case, what + " var", F32, var, rvar, b["var"])
    if rstd is not None:
        check(case, what + " rstd", F32, rstd, rrstd, b["rstd"])
        _log(case, what + " rstd relative error", F32, float(((rstd.double() - rrstd).abs() / rrstd).max()))
    if rm0 is not None:
        check(case, what + " running_mean", F32, rm1, rrm, b["rmean"])
        check(case, what + " running_var", F32, rv1, rrv, b["rvar"])
    return rmean, rvar, rrstd, b


def distinct_per_column(y):
    """True at the first occurrence of every value of a column: z is a function of (y, column) alone, so the roundings of
    equal y (the zeros behind a ReLU, the few thousand bf16 values a long column draws from) are one rounding, not many."""
    ys, idx = y.float().sort(dim=0, stable=True)
    first = torch.ones_like(ys, dtype=torch.bool)
    first[1:] = ys[1:] != ys[:-1]
    return torch.zeros_like(first).scatter_(0, idx, first)


def check_bn_apply(case, what, dt, wide, y, w, mean, rstd, gamma, beta, z, relu=False):
    rz, m = nr.bn_apply(y, w, mean, rstd, gamma, beta, relu=relu)
    coh = MARGIN * 4 * U_F * (m["folded"] if wide else m["z"])
    skip = nr.kink(m["pre"], m["pre_mag"], KINK) & (w >= 0)[:, None] if relu else None
    check(case, what, dt, z, rz, coh + MARGIN * u_st(dt) * m["z"], coh, skip, distinct_per_column(y))
    check_zero_rows(case, what, z, w < 0)


def check_bn_bwd_sums(case, what, dz, y, w, mean, rstd, sums, gamma=None, beta=None):
    R, C = y.shape
    s0, s1, m = nr.bn_bwd_sums(dz, y, w, mean, rstd, gamma, beta)
    b0, b1 = MARGIN * tau_sum(R) * m["s0"], MARGIN * tau_sum(R) * m["s1"]
    if gamma is not None:                   # the |dz| of the kink elements: they may count or not
        keep = w >= 0
        _, ma = nr.bn_apply(y, w, mean, rstd, gamma, beta)
        k = nr.kink(ma["pre"], ma["pre_mag"], KINK)[keep]
        d, yh = dz[keep].double().abs(), ((y[keep].double() - mean.double()) * rstd.double()).abs()
        b0, b1 = b0 + (d * k).sum(0), b1 + (d * yh * k).sum(0)
    check(case, what + " s0", F32, sums[:C], s0, b0)
    check(case, what + " s1", F32, sums[C:], s1, b1)
    return b0, b1


def check_bn_bwd_apply(case, what, dt, dz, y, w, mean, rstd, gamma, sums, inv_n, relu_mask, dy, stores=1, beta=None, sums_bound=None):
    """sums: the fp32 operands of the apply pass.  sums_bound: (b0, b1) when the kernel computed the sums itself
    (dl_bn_relu_bwd): `sums` are then the reference's and their error is carried into dy's bound."""
    C = y.shape[1]
    rdy, m = nr.bn_bwd_apply(dz, y, w, mean, rstd, gamma, sums[:C], sums[C:], inv_n, relu_mask, beta)
    coh = MARGIN * (10 + 4 * (stores - 1)) * U_F * m["dy"]
    skip = None
    if sums_bound is not None:
        yh = ((y.double() - mean.double()) * rstd.double()).abs()
        yh = torch.where(torch.isfinite(yh), yh, torch.zeros_like(yh))
        coh = coh + (gamma.double() * rstd.double()).abs() * w.clamp_min(0)[:, None] * (sums_bound[0] + yh * sums_bound[1]) * inv_n
    if beta is not None:
        _, ma = nr.bn_apply(y, w, mean, rstd, gamma, beta)
        skip = nr.kink(ma["pre"], ma["pre_mag"], KINK) & (w >= 0)[:, None]
    check(case, what, dt, dy, rdy, coh + MARGIN * stores * u_st(dt) * m["dy"], coh, skip)
    check_zero_rows(case, what, dy, w < 0)


# ---- buffers the test owns ------------------------------------------------------------------------------------------------------
class Guarded:
    """A flat NaN-filled buffer with a guard band on both sides; `view` hands out an as_strided view of the addressed
    elements and records them in `mask`."""
    G = 256

    def __init__(self, n, dt, dev=None):
        dev = dev or DEV
        self.t = torch.full((n + 2 * self.G,), float("nan"), device=dev, dtype=dt)
        self.mask = torch.zeros(n + 2 * self.G, dtype=torch.bool, device=dev)

    def view(self, shape, strides=None, off=0):
        if strides is None:
            strides = tuple(int(math.prod(shape[i + 1:])) for i in range(len(shape)))
        torch.as_strided(self.mask, shape, strides, self.G + off).fill_(True)
        return torch.as_strided(self.t, shape, strides, self.G + off)

    def bits(self):
        return self.t.view(torch.int16 if self.t.dtype == BF else torch.int32).clone()

    def untouched(self, case, before):
        outside = ~self.mask
        assert torch.equal(self.bits()[outside], before[outside]), "%s: a store outside the addressed elements" % case


def _filled(values, dt):
    """A guarded contiguous copy of `values` (any shape)."""
    g = Guarded(values.numel(), dt)
    v = g.view(tuple(values.shape))
    v.copy_(values)
    return v


def _out(shape, dt):
    g = Guarded(int(math.prod(shape)), dt)
    return g, g.view(tuple(shape))


def _lib():
    from druglamp_amd import _lib as lib_mod, ops
    return lib_mod.lib(), lib_mod.check, ops._stream(), ops._DT, lib_mod


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- data families -------------------------------------------------------------------------------------------------------------
def ln_data(kind, M, D, g):
    """[M][D] float32 rows (rounded to the case's dtype by the caller) and the rows that are constant."""
    x = torch.randn(M, D, generator=g)
    const = []
    if kind == "offset":
        x = x + 30.0
    elif kind == "const":                         # even rows constant (a few bits: every fp32 sum is exact), odd rows randn
        const = list(range(0, M, 2))
        x[const] = (torch.randint(-40, 41, (len(const), 1), generator=g).float() / 8.0).expand(len(const), D)
    elif kind == "spike":
        x[torch.arange(M), torch.randint(0, D, (M,), generator=g)] *= 64.0
    elif kind == "tiny":
        x = x * 1e-3
    return x, const


def bn_data(kind, R, C, g):
    y = torch.randn(R, C, generator=g)
    if kind == "offset":
        y = y + 8.0
    elif kind == "relu":
        y = y.clamp_min(0.0)
    elif kind == "const":
        y = (torch.randint(-40, 41, (1, C), generator=g).float() / 8.0).expand(R, C).contiguous()
    elif kind == "spike":
        y[torch.randint(0, R, (C,), generator=g), torch.arange(C)] *= 64.0
    elif kind == "tiny":
        y = y * 1e-3
    return y


# ---- LayerNorm cases -------------------------------------------------------------------------------------------------------------
Lay = collections.namedtuple("Lay", "ld off shift")        # row pitch, first column, elements the base is shifted by


def contig(D):
    return Lay(D, 0, 0)


LnCase = collections.namedtuple("LnCase", "name fwd bwd dt D M lay data dres pg out share")


def _ln(name, fwd, bwd, dt, D, M, lay=None, data="randn", dres=True, pg=True, out=None, share=1):
    lay = lay or contig(D)
    return LnCase(name, fwd, bwd, dt, D, M, lay, data, dres, pg, out or lay, share)


F16_256, B16_256, F16_512, B16_512 = "ln_fwd16<256>", "ln_bwd16<256>", "ln_fwd16<512>", "ln_bwd16<512>"


def _gen(dt, D):
    nv = 1 if D <= 256 else 2 if D <= 512 else 4 if D <= 1024 else 8
    t = "bf16" if dt == BF else "float"
    return "ln_fwd<%s,%d>" % (t, nv), "ln_bwd<%s,%d>" % (t, nv)


def _g(name, fwd, bwd, dt, D, M, **kw):
    return _ln(name, fwd, bwd, dt, D, M, **kw)


LN_CASES = [
    # 16-byte forms at D = 256: two rows share a wave (seg_sum<32>); M odd leaves the partner row past M
    _ln("v16_256_m1", F16_256, B16_256, BF, 256, 1, data="randn", dres=False),
    _ln("v16_256_m33_slice_of_768", F16_256, B16_256, BF, 256, 33, Lay(768, 256, 0), "offset"),
    _ln("v16_256_m95_pitch264", F16_256, B16_256, BF, 256, 95, Lay(264, 0, 0), "spike"),
    # 16-byte forms at D = 512: one row per wave pass, 16 rows per forward workgroup
    _ln("v16_512_m17_const", F16_512, B16_512, BF, 512, 17, data="const"),
    _ln("v16_512_m47_pitch520", F16_512, B16_512, BF, 512, 47, Lay(520, 0, 0), "randn", dres=False),
    _ln("v16_512_m64_tiny", F16_512, B16_512, BF, 512, 64, data="tiny"),
    # fallbacks from the 16-byte form (gamma / beta stay 16-byte aligned)
    _g("fallback_256_ld260", "ln_fwd<bf16,1>", "ln_bwd<bf16,1>", BF, 256, 33, lay=Lay(260, 0, 0), data="offset"),
    _g("fallback_512_base_8byte", "ln_fwd<bf16,2>", "ln_bwd<bf16,2>", BF, 512, 17, lay=Lay(512, 0, 4), data="randn"),
    # generic bf16
    _g("bf16_d36_m7", "ln_fwd<bf16,1>", "ln_bwd<bf16,1>", BF, 36, 7, data="const"),
    _g("bf16_d264_m9", "ln_fwd<bf16,2>", "ln_bwd<bf16,2>", BF, 264, 9, lay=Lay(272, 4, 0), data="spike"),
    _g("bf16_d1000_m1", "ln_fwd<bf16,4>", "ln_bwd<bf16,4>", BF, 1000, 1, data="randn", dres=False),
    _g("bf16_d1028_m130", "ln_fwd<bf16,8>", "ln_bwd<bf16,8>", BF, 1028, 130, data="offset"),
    _g("bf16_d2048_m9", "ln_fwd<bf16,8>", "ln_bwd<bf16,8>", BF, 2048, 9, lay=Lay(2052, 0, 0), data="tiny"),
    # generic fp32
    _g("f32_d4_m130", "ln_fwd<float,1>", "ln_bwd<float,1>", F32, 4, 130, data="randn"),
    _g("f32_d256_m7", "ln_fwd<float,1>", "ln_bwd<float,1>", F32, 256, 7, lay=Lay(260, 0, 0), data="offset"),
    _g("f32_d260_m9", "ln_fwd<float,2>", "ln_bwd<float,2>", F32, 260, 9, data="const", dres=False),
    _g("f32_d512_m1", "ln_fwd<float,2>", "ln_bwd<float,2>", F32, 512, 1, data="spike"),
    _g("f32_d1024_m9", "ln_fwd<float,4>", "ln_bwd<float,4>", F32, 1024, 9, lay=Lay(2048, 1024, 0), data="tiny"),
    _g("f32_d2048_m7", "ln_fwd<float,8>", "ln_bwd<float,8>", F32, 2048, 7, data="offset"),
    # backward: row tails of the 32-row workgroup, dres, need_param_grads=False, out= a strided slice, dy_share
    _ln("bwd16_m5_no_dres", F16_256, B16_256, BF, 256, 5, dres=False),
    _ln("bwd16_m31_no_param_grads", F16_512, B16_512, BF, 512, 31, pg=False),
    _ln("bwd16_m33_out_slice", F16_256, B16_256, BF, 256, 33, out=Lay(768, 512, 0)),
    _ln("bwd16_m100_deferred_reduction", F16_512, B16_512, BF, 512, 100, data="offset", pg="deferred"),
    _ln("bwd16_share7_m63", F16_256, B16_256, BF, 256, 63, share=7),
    _ln("bwd16_share12_m60", F16_512, B16_512, BF, 512, 60, share=12),
    _g("bwd_m5_no_dres", "ln_fwd<bf16,2>", "ln_bwd<bf16,2>", BF, 264, 5, dres=False),
    _g("bwd_m31_no_param_grads", "ln_fwd<float,2>", "ln_bwd<float,2>", F32, 260, 31, pg=False),
    _g("bwd_m33_out_slice", "ln_fwd<bf16,4>", "ln_bwd<bf16,4>", BF, 1000, 33, out=Lay(3000, 1000, 0)),
    _g("bwd_m100_split_param_grads", "ln_fwd<float,2>", "ln_bwd<float,2>", F32, 512, 100, data="offset", pg="split"),
    _g("bwd_share7_m63", "ln_fwd<bf16,2>", "ln_bwd<bf16,2>", BF, 264, 63, share=7),
    _g("bwd_share12_m60", "ln_fwd<float,4>", "ln_bwd<float,4>", F32, 1024, 60, share=12),
]


def _ln_view(lay, M, D, dt, values=None):
    """A guarded [M][D] view with the case's pitch, column offset and base shift; three more rows behind it stay NaN."""
    g = Guarded((M + 3) * lay.ld + lay.shift, dt)
    v = g.view((M, D), (lay.ld, 1), lay.shift + lay.off)
    if values is not None:
        v.copy_(values)
    return g, v


def _is16(dt, D, views, params):
    return (dt == BF and D in (256, 512) and all(v.stride(0) % 8 == 0 and v.data_ptr() % 16 == 0 for v in views)
            and all(p.data_ptr() % 16 == 0 for p in params))


@pytest.mark.gpu
@pytest.mark.parametrize("c", LN_CASES, ids=[c.name for c in LN_CASES])
def test_layernorm_form_against_fp64(c):
    L, ok, stream, DT, lib_mod = _lib()
    dt, D, M = c.dt, c.D, c.M
    g = torch.Generator().manual_seed(sum(map(ord, c.name)))
    xv, const = ln_data(c.data, M, D, g)
    _, x = _ln_view(c.lay, M, D, dt, xv)
    gamma = _filled(1.0 + 0.5 * torch.randn(D, generator=g), F32)
    beta = _filled(0.5 * torch.randn(D, generator=g), F32)
    yg, y = _ln_view(c.lay, M, D, dt)
    mg, mean = _out((M,), F32)
    rg, rstd = _out((M,), F32)
    gen = _gen(dt, D)
    assert c.fwd == (("ln_fwd16<%d>" % D) if _is16(dt, D, (x, y), (gamma, beta)) else gen[0]), "the case names another forward form"
    before = [b.bits() for b in (yg, mg, rg)]
    ok(L.dl_layernorm_fwd(x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), y.stride(0), mean.data_ptr(),
                          rstd.data_ptr(), M, D, EPS, DT[dt], stream), "dl_layernorm_fwd")
    check_ln_fwd(c.name, dt, x, gamma, beta, EPS, y, mean, rstd, const)
    for b, bb in zip((yg, mg, rg), before):
        b.untouched(c.name, bb)

    # ---- backward (twice: bitwise repeatable); mean / rstd: the fp64 statistics rounded to fp32, exact operands ----
    _, rmean, rrstd, _ = nr.ln_fwd(x, gamma, beta, EPS)
    mean_in, rstd_in = _filled(rmean.float(), F32), _filled(rrstd.float(), F32)
    Mdy = M // c.share
    _, dy = _ln_view(c.lay, Mdy, D, dt, torch.randn(Mdy, D, generator=g))
    dres = _ln_view(c.lay, M, D, dt, 0.5 * torch.randn(M, D, generator=g))[1] if c.dres else None
    dxg, dx = _ln_view(c.out, M, D, dt)
    # parameter gradients: adjacent [2][D] (one final-reduction launch), "split" (two buffers: one launch each), "deferred"
    # (the partials are handed back as a dl_reduce_item and reduced by dl_reduce_batch), False (none)
    if c.pg == "split":
        (gg, dgam), (bg, dbet) = _out((D,), F32), _out((D,), F32)
        grads = [gg, bg]
    else:
        gbg, gb = _out((2, D), F32)
        dgam, dbet, grads = gb[0], gb[1], [gbg]
    views = [dy, x, dx] + ([dres] if c.dres else [])
    assert c.bwd == (("ln_bwd16<%d>" % D) if _is16(dt, D, views, (gamma,)) else gen[1]), "the case names another backward form"
    nbytes = L.dl_layernorm_bwd_workspace_bytes(M, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    outs = []
    for rep in range(2):
        for b in [dxg] + grads:
            b.t.fill_(float("nan"))
        before = [b.bits() for b in [dxg] + grads]
        item = lib_mod.ReduceItem() if c.pg == "deferred" else None
        ok(L.dl_layernorm_bwd(dy.data_ptr(), dy.stride(0), c.share, x.data_ptr(), x.stride(0), mean_in.data_ptr(), rstd_in.data_ptr(),
                              gamma.data_ptr(), _ptr(dres), 0 if dres is None else dres.stride(0), dx.data_ptr(), dx.stride(0),
                              dgam.data_ptr() if c.pg else None, dbet.data_ptr() if c.pg else None, 0, M, D, DT[dt],
                              ws.data_ptr(), ws.numel(), None if item is None else ctypes.pointer(item), stream), "dl_layernorm_bwd")
        if item is not None:
            assert item.kind != 0, "%s: the final reduction was not handed back" % c.name
            ok(L.dl_reduce_batch((lib_mod.ReduceItem * 1)(item), 1, stream), "dl_reduce_batch")
        torch.cuda.synchronize()
        outs.append([b.bits() for b in [dxg] + grads])
        dxg.untouched(c.name, before[0])
        for b, bb in zip(grads, before[1:]):
            if c.pg:
                b.untouched(c.name, bb)
            else:
                assert torch.equal(b.bits(), bb), "%s: parameter gradients written although not asked for" % c.name
    assert all(torch.equal(a, b) for a, b in zip(*outs)), "%s: backward not bitwise repeatable" % c.name
    check_ln_bwd(c.name, dt, dy, x, mean_in, rstd_in, gamma, dres, c.share, dx, dgam if c.pg else None, dbet if c.pg else None)


# ---- BatchNorm cases -------------------------------------------------------------------------------------------------------------
BnCase = collections.namedtuple("BnCase", "name forms dt C rule R data")
WIDE = ("bn_partial_wide<0/1>", "bn_apply_fwd_wide", "bn_bwd_apply_wide")
GEN_BF = ("bn_partial<bf16,0/1>", "bn_apply_fwd<bf16>", "bn_bwd_apply<bf16>")
GEN_F32 = ("bn_partial<float,0/1>", "bn_apply_fwd<float>", "bn_bwd_apply<float>")


def _bn_forms(dt, C, tensors):
    """The host test of bn_reduce / bn_apply_fwd_run / bn_bwd_apply_run, restated."""
    if dt == BF and C in (64, 128, 256) and all(t.data_ptr() % 16 == 0 for t in tensors):
        return WIDE
    return GEN_BF if dt == BF else GEN_F32


def _bn(name, forms, dt, C, rule, R=None, data="randn"):
    if rule[0] == "win":
        R = rule[1] * rule[4]
    return BnCase(name, forms, dt, C, rule, R, data)


NONE = ("none",)


def _win(win, halo, valid, n):
    return ("win", win, halo, valid, n)


BN_CASES = [
    # no row rule
    _bn("wide64_r1", WIDE, BF, 64, NONE, 1), _bn("wide128_r31_offset", WIDE, BF, 128, NONE, 31, "offset"),
    _bn("wide256_r33_relu", WIDE, BF, 256, NONE, 33, "relu"), _bn("bf16_c72_r1", GEN_BF, BF, 72, NONE, 1),
    _bn("bf16_c96_r31_const", GEN_BF, BF, 96, NONE, 31, "const"), _bn("bf16_c260_r33_spike", GEN_BF, BF, 260, NONE, 33, "spike"),
    _bn("bf16_c512_r33_tiny", GEN_BF, BF, 512, NONE, 33, "tiny"), _bn("f32_c4_r33_offset", GEN_F32, F32, 4, NONE, 33, "offset"),
    _bn("f32_c128_r31", GEN_F32, F32, 128, NONE, 31), _bn("f32_c260_r1", GEN_F32, F32, 260, NONE, 1),
    _bn("wide128_r33_const", WIDE, BF, 128, NONE, 33, "const"), _bn("f32_c128_r33_relu", GEN_F32, F32, 128, NONE, 33, "relu"),
    # more than 256 partial chunks (the four-way loops of the second reduction stage); 40 rows per block at C = 64
    _bn("wide64_r40000_relu", WIDE, BF, 64, NONE, 40000, "relu"), _bn("wide128_r9000", WIDE, BF, 128, NONE, 9000),
    _bn("bf16_c96_r9000_relu", GEN_BF, BF, 96, NONE, 9000, "relu"), _bn("f32_c260_r9000_offset", GEN_F32, F32, 260, NONE, 9000, "offset"),
    # windows
    _bn("wide64_win40_4_32x5", WIDE, BF, 64, _win(40, 4, 32, 5), data="relu"), _bn("bf16_c72_win40_4_32x5", GEN_BF, BF, 72, _win(40, 4, 32, 5)),
    _bn("wide256_win37_3_31x7", WIDE, BF, 256, _win(37, 3, 31, 7), data="offset"), _bn("bf16_c260_win37_3_31x7", GEN_BF, BF, 260, _win(37, 3, 31, 7), data="relu"),
    _bn("f32_c4_win37_3_31x7", GEN_F32, F32, 4, _win(37, 3, 31, 7)),
    _bn("wide128_tail_win136_128_8x4", WIDE, BF, 128, _win(136, 128, 8, 4)), _bn("wide128_lead_win136_0_128x4", WIDE, BF, 128, _win(136, 0, 128, 4)),
    _bn("bf16_c96_tail_win136_128_8x4", GEN_BF, BF, 96, _win(136, 128, 8, 4), data="relu"), _bn("bf16_c96_lead_win136_0_128x4", GEN_BF, BF, 96, _win(136, 0, 128, 4), data="offset"),
    _bn("wide128_model_win2312x2", WIDE, BF, 128, _win(2312, 4, 2304, 2), data="relu"), _bn("bf16_c512_model_win2312x2", GEN_BF, BF, 512, _win(2312, 4, 2304, 2)),
    _bn("f32_c128_model_win2312x2", GEN_F32, F32, 128, _win(2312, 4, 2304, 2), data="offset"),
    # row weights from {-1, 0, 1, 3} with runs of excluded rows at both ends
    _bn("wide64_rw_r100", WIDE, BF, 64, ("rw",), 100, "relu"), _bn("wide256_rw_r333", WIDE, BF, 256, ("rw",), 333, "offset"),
    _bn("wide128_rw_r9000", WIDE, BF, 128, ("rw",), 9000), _bn("bf16_c72_rw_r100", GEN_BF, BF, 72, ("rw",), 100),
    _bn("bf16_c512_rw_r77", GEN_BF, BF, 512, ("rw",), 77, "relu"), _bn("f32_c128_rw_r100", GEN_F32, F32, 128, ("rw",), 100, "offset"),
    _bn("f32_c260_rw_r50", GEN_F32, F32, 260, ("rw",), 50, "spike"),
]


def _row_weights(c, g):
    if c.rule[0] == "none":
        return torch.ones(c.R, dtype=F64), None, (0, 0, 0)
    if c.rule[0] == "win":
        _, win, halo, valid, _n = c.rule
        return nr.window_weights(c.R, win, halo, valid), None, (win, halo, valid)
    w = torch.tensor([-1.0, 0.0, 1.0, 3.0])[torch.randint(0, 4, (c.R,), generator=g)]
    w[:5] = -1.0
    w[-7:] = -1.0
    w[5:8] = torch.tensor([3.0, 0.0, 1.0])
    return w.double(), w.float(), (0, 0, 0)


def _params(C, g, n):
    return [_filled(t, F32) for t in ([1.0 + 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)] +
                                      [torch.randn(C, generator=g) for _ in range(n)])]


@pytest.mark.gpu
@pytest.mark.parametrize("c", BN_CASES, ids=[c.name for c in BN_CASES])
def test_batchnorm_form_against_fp64(c):
    L, ok, stream, DT, _ = _lib()
    dt, C, R, name = c.dt, c.C, c.R, c.name
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    w64, rw, (win, halo, valid) = _row_weights(c, g)
    w = w64.to(DEV)
    rw = None if rw is None else _filled(rw, F32)
    n = int(w64.clamp_min(0).sum())
    y = _filled(bn_data(c.data, R, C, g), dt)
    dz = _filled(torch.randn(R, C, generator=g), dt)
    y[w < 0] = float("nan")                          # excluded / halo rows are never read
    dz[w < 0] = float("nan")
    gamma, beta, rm0, = _params(C, g, 1)
    rv0 = _filled(torch.rand(C, generator=g) + 0.5, F32)
    wide = c.forms is WIDE
    assert c.forms == _bn_forms(dt, C, (y, dz)), "the case names other forms"
    ws = torch.empty(L.dl_bn_workspace_bytes(R, C), dtype=torch.uint8, device=DEV)
    wsa = (ws.data_ptr(), ws.numel(), stream)

    def guarded_call(outs, fn):
        before = [b.bits() for b, _ in outs]
        fn()
        torch.cuda.synchronize()
        for (b, _), bb in zip(outs, before):
            b.untouched(name, bb)

    # ---- bn_reduce<0>: dl_bn_stats / dl_bn_stats_rw ----
    sg, sums = _out((2 * C,), F32)
    if rw is not None:
        guarded_call([(sg, sums)], lambda: ok(L.dl_bn_stats_rw(y.data_ptr(), R, C, rw.data_ptr(), DT[dt], sums.data_ptr(), *wsa), "dl_bn_stats_rw"))
    else:
        guarded_call([(sg, sums)], lambda: ok(L.dl_bn_stats(y.data_ptr(), R, C, win, halo, valid, DT[dt], sums.data_ptr(), *wsa), "dl_bn_stats"))
    check_bn_sums(name, "stats", y, w, sums)

    # ---- dl_bn_stats_finalize (momentum 0.1 against given running statistics) ----
    outs = [_out((2 * C,), F32)] + [_out((C,), F32) for _ in range(3)]
    rm1, rv1 = _filled(rm0, F32), _filled(rv0, F32)
    (_, sums2), (_, mean2), (_, var2), (_, rstd2) = outs
    guarded_call(outs, lambda: ok(L.dl_bn_stats_finalize(y.data_ptr(), R, C, win, halo, valid, _ptr(rw), DT[dt], n, EPS, MOMENTUM, sums2.data_ptr(),
                                                         mean2.data_ptr(), var2.data_ptr(), rstd2.data_ptr(), rm1.data_ptr(), rv1.data_ptr(), *wsa),
                                  "dl_bn_stats_finalize"))
    check_bn_finalize(name, "stats_finalize", n, EPS, MOMENTUM, rm0, rv0, mean2, var2, rstd2, rm1, rv1, y=y, w=w, sums_out=sums2)

    # ---- dl_bn_finalize on the sums of dl_bn_stats (operands) ----
    outs = [_out((C,), F32) for _ in range(3)]
    rm1, rv1 = _filled(rm0, F32), _filled(rv0, F32)
    (_, mean), (_, var), (_, rstd) = outs
    guarded_call(outs, lambda: ok(L.dl_bn_finalize(sums.data_ptr(), n, EPS, MOMENTUM, mean.data_ptr(), var.data_ptr(), rstd.data_ptr(), rm1.data_ptr(),
                                                   rv1.data_ptr(), C, stream), "dl_bn_finalize"))
    check_bn_finalize(name, "finalize", n, EPS, MOMENTUM, rm0, rv0, mean, var, rstd, rm1, rv1, sums=sums)

    # ---- bn_apply_fwd_run ----
    zg, z = _out((R, C), dt)
    if rw is not None:
        guarded_call([(zg, z)], lambda: ok(L.dl_bn_apply_fwd_rw(y.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                                 beta.data_ptr(), R, C, rw.data_ptr(), DT[dt], stream), "dl_bn_apply_fwd_rw"))
    else:
        guarded_call([(zg, z)], lambda: ok(L.dl_bn_apply_fwd(y.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                              beta.data_ptr(), R, C, win, halo, valid, DT[dt], stream), "dl_bn_apply_fwd"))
    check_bn_apply(name, "apply_fwd", dt, wide, y, w, mean, rstd, gamma, beta, z)

    # ---- bn_reduce<1> and bn_bwd_apply_run, twice ----
    inv_n = f32(1.0 / n)
    reps = []
    for rep in range(2):
        bg, bs = _out((2 * C,), F32)
        if rw is not None:
            guarded_call([(bg, bs)], lambda: ok(L.dl_bn_bwd_reduce_rw(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, C, rw.data_ptr(),
                                                                       DT[dt], bs.data_ptr(), *wsa), "dl_bn_bwd_reduce_rw"))
        else:
            guarded_call([(bg, bs)], lambda: ok(L.dl_bn_bwd_reduce(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, C, win, halo, valid,
                                                                    DT[dt], bs.data_ptr(), *wsa), "dl_bn_bwd_reduce"))
        dys = []
        for relu_mask in (0, 1):
            dg, dy = _out((R, C), dt)
            if rw is not None:
                guarded_call([(dg, dy)], lambda: ok(L.dl_bn_bwd_apply_rw(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                                          bs.data_ptr(), inv_n, relu_mask, dy.data_ptr(), R, C, rw.data_ptr(), DT[dt], stream),
                                                    "dl_bn_bwd_apply_rw"))
            else:
                guarded_call([(dg, dy)], lambda: ok(L.dl_bn_bwd_apply(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                                       bs.data_ptr(), inv_n, relu_mask, dy.data_ptr(), R, C, win, halo, valid, DT[dt], stream),
                                                    "dl_bn_bwd_apply"))
            dys.append((dg, dy))
        reps.append((bg, bs, dys))
    for a, b in zip([reps[0][0]] + [d for d, _ in reps[0][2]], [reps[1][0]] + [d for d, _ in reps[1][2]]):
        assert torch.equal(a.bits(), b.bits()), "%s: backward not bitwise repeatable" % name
    _, bs, dys = reps[0]
    check_bn_bwd_sums(name, "bwd_reduce", dz, y, w, mean, rstd, bs)
    for relu_mask in (0, 1):
        check_bn_bwd_apply(name, "bwd_apply[relu_mask=%d]" % relu_mask, dt, dz, y, w, mean, rstd, gamma, bs, inv_n, relu_mask, dys[relu_mask][1])


# ---- BatchNorm -> ReLU (always the generic kernels; no `const` data: every element would sit on the kink) -------------------------
ReluCase = collections.namedtuple("ReluCase", "name forms dt C R data")
RELU_FORMS = ("bn_apply_fwd<T,relu>", "bn_partial<T,1,prelu>", "bn_bwd_apply<T,prelu_b>")
RELU_CASES = [
    ReluCase("relu_bf16_c512_r200", RELU_FORMS, BF, 512, 200, "randn"), ReluCase("relu_bf16_c128_r33_offset", RELU_FORMS, BF, 128, 33, "offset"),
    ReluCase("relu_bf16_c72_r9000_relu", RELU_FORMS, BF, 72, 9000, "relu"), ReluCase("relu_f32_c260_r31_tiny", RELU_FORMS, F32, 260, 31, "tiny"),
    ReluCase("relu_f32_c4_r1000_spike", RELU_FORMS, F32, 4, 1000, "spike"),
]


def _stats32(y, w, n):
    """The fp64 statistics of y rounded to fp32 (operands of the apply and backward kernels)."""
    s0, s1, _ = nr.bn_sums(y, w)
    mean, _var, rstd, _, _ = nr.bn_finalize(s0, s1, n, EPS)
    return _filled(mean.float(), F32), _filled(rstd.float(), F32)


@pytest.mark.gpu
@pytest.mark.parametrize("c", RELU_CASES, ids=[c.name for c in RELU_CASES])
def test_batchnorm_relu_form_against_fp64(c):
    L, ok, stream, DT, _ = _lib()
    dt, C, R, name = c.dt, c.C, c.R, c.name
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    w = torch.ones(R, dtype=F64, device=DEV)
    y = _filled(bn_data(c.data, R, C, g), dt)
    dz = _filled(torch.randn(R, C, generator=g), dt)
    gamma, beta = _params(C, g, 0)
    mean, rstd = _stats32(y, w, R)
    zg, z = _out((R, C), dt)
    before = zg.bits()
    ok(L.dl_bn_apply_relu_fwd(y.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), R, C, DT[dt], stream),
       "dl_bn_apply_relu_fwd")
    zg.untouched(name, before)
    check_bn_apply(name, "apply_relu_fwd", dt, False, y, w, mean, rstd, gamma, beta, z, relu=True)
    ws = torch.empty(L.dl_bn_workspace_bytes(R, C), dtype=torch.uint8, device=DEV)
    inv_n = f32(1.0 / R)
    reps = []
    for rep in range(2):
        (dg, dy), (sg, sums) = _out((R, C), dt), _out((2 * C,), F32)
        before = (dg.bits(), sg.bits())
        ok(L.dl_bn_relu_bwd(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), inv_n, dy.data_ptr(),
                            sums.data_ptr(), R, C, DT[dt], ws.data_ptr(), ws.numel(), stream), "dl_bn_relu_bwd")
        torch.cuda.synchronize()
        dg.untouched(name, before[0])
        sg.untouched(name, before[1])
        reps.append((dg, dy, sg, sums))
    assert torch.equal(reps[0][0].bits(), reps[1][0].bits()) and torch.equal(reps[0][2].bits(), reps[1][2].bits()), \
        "%s: backward not bitwise repeatable" % name
    _, dy, _, sums = reps[0]
    sb = check_bn_bwd_sums(name, "relu_bwd", dz, y, w, mean, rstd, sums, gamma, beta)
    rs0, rs1, _ = nr.bn_bwd_sums(dz, y, w, mean, rstd, gamma, beta)
    check_bn_bwd_apply(name, "relu_bwd dy", dt, dz, y, w, mean, rstd, gamma, torch.cat([rs0, rs1]), inv_n, 0, dy, beta=beta, sums_bound=sb)


# ---- dl_bn_tail_fix behind dl_bn_bwd_apply (two stores of dy) ----------------------------------------------------------------------
TailCase = collections.namedtuple("TailCase", "name forms dt C B LP lead w data")
TAIL_CASES = [TailCase("tail_%s_c%d_lp%d_lead%d_w%d" % ("bf16" if dt == BF else "f32", C, LP, lead, w), ("bn_tail_fix<%s>" % ("bf16" if dt == BF else "float"),),
                       dt, C, B, LP, lead, w, data)
              for (dt, C, B, LP, lead, data) in ((BF, 128, 4, 136, 128, "relu"), (BF, 72, 3, 21, 16, "offset"), (F32, 260, 3, 21, 16, "randn"))
              for w in (1, 5, 48)]


@pytest.mark.gpu
@pytest.mark.parametrize("c", TAIL_CASES, ids=[c.name for c in TAIL_CASES])
def test_batchnorm_tail_fix_against_fp64(c):
    L, ok, stream, DT, _ = _lib()
    dt, C, name = c.dt, c.C, c.name
    R = c.B * c.LP
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    w = nr.tail_weights(R, c.LP, c.lead, c.w, DEV)
    n = int(w.sum())
    y = _filled(bn_data(c.data, R, C, g), dt)
    dz = _filled(torch.randn(R, C, generator=g), dt)
    gamma, beta = _params(C, g, 0)
    mean, rstd = _stats32(y, w, n)
    ones = torch.ones(R, dtype=F64, device=DEV)
    s0, s1, _ = nr.bn_bwd_sums(dz, y, ones, mean, rstd)
    sums = _filled(torch.cat([s0, s1]).float(), F32)
    inv_n = f32(1.0 / n)
    reps = []
    for rep in range(2):
        dg, dy = _out((R, C), dt)
        before = dg.bits()
        ok(L.dl_bn_bwd_apply(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), sums.data_ptr(), inv_n, 0, dy.data_ptr(),
                             R, C, 0, 0, 0, DT[dt], stream), "dl_bn_bwd_apply")
        torch.cuda.synchronize()
        once = dy.clone()
        ok(L.dl_bn_tail_fix(dy.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), sums.data_ptr(), inv_n, c.w, R, C,
                            c.LP, c.lead, DT[dt], stream), "dl_bn_tail_fix")
        torch.cuda.synchronize()
        dg.untouched(name, before)
        reps.append((dg, dy))
    assert torch.equal(reps[0][0].bits(), reps[1][0].bits()), "%s: not bitwise repeatable" % name
    dy = reps[0][1]
    lead_rows = (torch.arange(R, device=DEV) % c.LP) < c.lead
    assert torch.equal(dy[lead_rows], once[lead_rows]), "%s: dl_bn_tail_fix touched a lead row" % name
    check_bn_bwd_apply(name, "bwd_apply+tail_fix", dt, dz, y, w, mean, rstd, gamma, sums, inv_n, 0, dy, stores=2)


# ---- end to end against fp64 autograd ----------------------------------------------------------------------------------------------
E2eCase = collections.namedtuple("E2eCase", "name fn dt C B LP lead w relu data")
E2E_CASES = [E2eCase("%s_%s_c%d_r%d%s" % (fn, "bf16" if dt == BF else "f32", C, B * LP, "_relu" if relu else ""), fn, dt, C, B, LP, lead, w, relu, data)
             for (fn, dt, C, B, LP, lead, w, data) in (("rows", BF, 128, 1, 200, 200, 1, "relu"), ("rows", BF, 96, 1, 33, 33, 1, "offset"),
                                                       ("rows", F32, 260, 1, 50, 50, 1, "randn"), ("tail", BF, 128, 4, 136, 128, 48, "relu"),
                                                       ("tail", BF, 72, 3, 21, 16, 5, "randn"), ("tail", F32, 132, 3, 21, 16, 5, "offset"))
             for relu in (False, True)]


def e2e_reference(x, gamma, beta, dz, LP, lead, wmul, relu, eps):
    """fp64 autograd through the expanded matrix of bn_tail_expand (wmul = 1: the matrix itself): y on the compact rows, the
    gradients with those of the copies summed back, the batch mean and biased variance."""
    X, G_, B_ = (t.double().clone().requires_grad_(True) for t in (x, gamma, beta))
    Xe, idx = nr.bn_tail_expand(X, LP, lead, wmul)
    mean = Xe.mean(0)
    var = ((Xe - mean) ** 2).mean(0)
    Ze = (Xe - mean) / torch.sqrt(var + eps) * G_ + B_
    if relu:
        Ze = Ze.clamp_min(0.0)
    mult = nr.tail_weights(x.shape[0], LP, lead, wmul, x.device)
    (Ze * (dz.double() / mult[:, None])[idx]).sum().backward()
    first = torch.zeros(x.shape[0], dtype=torch.long, device=x.device)
    first[idx.flip(0)] = torch.arange(idx.numel(), device=x.device).flip(0)
    return Ze.detach()[first], X.grad, G_.grad, B_.grad, mean.detach(), var.detach()


def check_e2e(case, dt, wide_apply, x, gamma, beta, dz, LP, lead, wmul, relu, eps, momentum, rm0, rv0, got, extra_tau=0.0, stores=1):
    """got: dict(y, dx, dgamma, dbeta, mean, var, rmean, rvar) of the autograd Function."""
    R, C = x.shape
    w = nr.tail_weights(R, LP, lead, wmul, x.device)
    n = int(w.sum())
    ry, rdx, rdg, rdb, rmean, rvar = e2e_reference(x, gamma, beta, dz, LP, lead, wmul, relu, eps)
    _, _, rrstd, fb = check_bn_finalize(case, "e2e", n, eps, momentum, rm0, rv0, got["mean"], got["var"], None, got["rmean"], got["rvar"], y=x, w=w,
                                        extra_tau=extra_tau)
    g, rs = gamma.double(), rrstd
    _, ma = nr.bn_apply(x, w, rmean, rrstd, gamma, beta, relu=relu)
    yh = (x.double() - rmean) * rs
    e_rr = fb["rstd"] / rrstd
    e_yh = rs * fb["mean"] + yh.abs() * (e_rr + 2 * U_F)
    skip = nr.kink(ma["pre"], ma["pre_mag"] + g.abs() * e_yh / KINK, KINK) if relu else None
    coh = MARGIN * 4 * U_F * (ma["folded"] if wide_apply else ma["z"]) + g.abs() * e_yh
    check(case, "y", dt, got["y"], ry, coh + MARGIN * u_st(dt) * ma["z"], coh, skip)
    # backward: sums from the kernels' own yhat, then dx
    inv_n = 1.0 / n
    d = dz.double() * ((ma["pre"] > 0) if relu else 1.0)
    k = skip.double() if relu else torch.zeros_like(d)
    dabs = dz.double().abs()
    m0, m1 = d.abs().sum(0), (d * yh).abs().sum(0)
    b0 = MARGIN * tau_sum(R) * m0 + (dabs * k).sum(0)
    b1 = MARGIN * tau_sum(R) * m1 + (d.abs() * e_yh).sum(0) + (dabs * yh.abs() * k).sum(0)
    check(case, "dbeta", F32, got["dbeta"], rdb, b0)
    check(case, "dgamma", F32, got["dgamma"], rdg, b1)
    s0, s1 = d.sum(0), (d * yh).sum(0)
    _, md = nr.bn_bwd_apply(d, x, w, rmean, rrstd, gamma, s0, s1, inv_n)
    gr = (g * rs).abs()
    coh = (MARGIN * (10 + 4 * (stores - 1)) * U_F + e_rr) * md["dy"] + gr * w[:, None] * ((b0 + yh.abs() * b1) * inv_n + s1.abs() * inv_n * e_yh)
    check(case, "dx", dt, got["dx"], rdx, coh + MARGIN * stores * u_st(dt) * md["dy"], coh, skip)


@pytest.mark.gpu
@pytest.mark.parametrize("c", E2E_CASES, ids=[c.name for c in E2E_CASES])
def test_batchnorm_functions_against_fp64_autograd(c):
    from druglamp_amd import functional as Fn
    dt, C = c.dt, c.C
    R = c.B * c.LP
    g = torch.Generator().manual_seed(sum(map(ord, c.name)))
    x = bn_data(c.data, R, C, g).to(DEV, dt).requires_grad_(True)
    gamma = (1.0 + 0.5 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    beta = (0.5 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    rm0, rv0 = torch.randn(C, generator=g).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV)
    dz = torch.randn(R, C, generator=g).to(DEV, dt)
    outs = []
    for rep in range(2):
        rm, rv = rm0.clone(), rv0.clone()
        x.grad = gamma.grad = beta.grad = None
        if c.fn == "rows":
            y, mean, var = Fn.BatchNormRowsFn.apply(x, gamma, beta, rm, rv, True, EPS, MOMENTUM, c.relu)
        else:
            y, mean, var = Fn.BatchNormWeightedTailFn.apply(x, gamma, beta, rm, rv, EPS, MOMENTUM, c.LP, c.lead, c.w, c.relu)
        y.backward(dz)
        outs.append(dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, mean=mean, var=var, rmean=rm, rvar=rv))
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), "%s: %s not bitwise repeatable" % (c.name, k)
    tail = c.fn == "tail"
    wide = dt == BF and C in (64, 128, 256) and not c.relu
    check_e2e(c.name, dt, wide, x.detach(), gamma.detach(), beta.detach(), dz, c.LP, c.lead, c.w, c.relu, EPS, MOMENTUM, rm0, rv0, outs[0],
              extra_tau=3 * U_F if tail else 0.0, stores=2 if tail else 1)
