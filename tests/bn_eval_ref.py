"""fp64 reference of dl_bn_eval_bwd (bn_eval.hip): the backward of a BatchNorm that ran on FIXED statistics, written from
the definition in plain torch (no library call), on whatever device the operands live; in the style of tests/norm_ref.py.

Rows take part where the row weight w[r] >= 0 (norm_ref.window_weights turns the window rule into such weights); the weight
is otherwise NOT applied: a row that stands for m identical rows already carries the sum of their gradients in dz, and xhat
is the same for all of them, so the plain sum over the compact rows is the sum over the expanded ones.

    xhat = (y - mean) rstd
    g    = dz * [relu_out ? (xhat gamma + beta > 0) : 1]
    sums = (sum_r g | sum_r g xhat)                      (d beta | d gamma)
    dx   = g gamma rstd * [relu_in ? (y > 0) : 1]        zero on the rows that take no part (never read)
"""
import torch

from tests.norm_ref import window_weights          # noqa: F401  (re-exported: the window rule as row weights)

F64 = torch.float64


def _d(t):
    return None if t is None else t.to(F64)


def bn_eval_bwd(dz, y, w, mean, rstd, gamma, beta=None, relu_in=False, relu_out=False):
    """(dx [R][C], sums [2C], mags).  w [R]: row weights (only the sign is used).  mags: the tensors a rounding bound
    multiplies — dx = |dx|, s0 = sum |g|, s1 = sum |g xhat| — and, for the ReLU kink of relu_out, pre = xhat gamma + beta
    with pre_mag = |xhat gamma| + |beta| (zero rows where w < 0) and xhat_abs = |xhat|."""
    keep = w >= 0
    R, C = y.shape
    mu, rs, gm = _d(mean), _d(rstd), _d(gamma)
    d, yk = _d(dz[keep]), _d(y[keep])
    xh = (yk - mu) * rs
    pre = torch.zeros((R, C), dtype=F64, device=y.device)
    pre_mag = torch.zeros_like(pre)
    xhat_abs = torch.zeros_like(pre)
    xhat_abs[keep] = xh.abs()
    g = d
    if relu_out:
        bt = _d(beta)
        p = xh * gm + bt
        pre[keep], pre_mag[keep] = p, (xh * gm).abs() + bt.abs()
        g = torch.where(p > 0, d, torch.zeros_like(d))        # a select: a closed element's dz is not read
    s0, s1 = g.sum(0), (g * xh).sum(0)
    v = g * gm * rs
    if relu_in:
        v = torch.where(yk > 0, v, torch.zeros_like(v))
    dx = torch.zeros((R, C), dtype=F64, device=y.device)
    dx[keep] = v
    mags = {"dx": dx.abs(), "s0": g.abs().sum(0), "s1": (g * xh).abs().sum(0), "pre": pre, "pre_mag": pre_mag, "xhat_abs": xhat_abs}
    return dx, torch.cat([s0, s1]), mags
