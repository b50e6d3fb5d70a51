"""fp64 references of the LayerNorm and BatchNorm operations of norm.hip / bn.hip, written from the definitions in plain
torch (no library call), on whatever device the operands live.  Every function returns its values and, under `mags`, the
tensors an element-wise rounding bound multiplies: the sum of the absolute values of the terms of its own expression.

BatchNorm is defined over an explicit row-weight vector w[r]: w < 0 excluded (outputs are zero, the row is never read),
w = 0 a context row (computed, no part in the statistics), w = m >= 1 a row that stands for m identical rows (it counts m
times in the statistics; its incoming gradient is the sum over the m copies, so it takes the mean terms m times).
"""
import torch

F64 = torch.float64


def _d(t):
    return None if t is None else t.to(F64)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------
def ln_fwd(x, gamma, beta, eps):
    """x [M][D] -> (y, mean, rstd, mags).  mags: mean = sum |x| / D, var, xg = |xhat gamma|, y = |xhat gamma| + |beta|,
    carry = rstd |gamma| (what an error of the mean is multiplied by on its way into y)."""
    x, g, b = _d(x), _d(gamma), _d(beta)
    D = x.shape[1]
    mean = x.sum(1) / D
    d = x - mean[:, None]
    var = (d * d).sum(1) / D
    rstd = 1.0 / torch.sqrt(var + eps)
    xg = d * rstd[:, None] * g
    y = xg + b
    mags = {"mean": x.abs().sum(1) / D, "var": var, "xg": xg.abs(), "y": xg.abs() + b.abs(),
            "carry": rstd[:, None] * g.abs().expand_as(x)}
    return y, mean, rstd, mags


def ln_bwd(dy, x, gamma, dres=None, dy_share=1, mean=None, rstd=None, eps=1e-5):
    """(dx, dgamma, dbeta, mags) of y = LayerNorm(x) gamma + beta (+ the residual branch's gradient dres added to dx).
    dy has M / dy_share rows; row i of it is the gradient of rows i dy_share .. (i + 1) dy_share - 1 (the literal expansion).
    mean / rstd: the statistics the forward saved, taken as exact operands (default: those of x)."""
    dy, x, g, dres = _d(dy), _d(x), _d(gamma), _d(dres)
    if dy_share != 1:
        dy = dy.repeat_interleave(dy_share, 0)
    D = x.shape[1]
    if mean is None:
        mean = x.sum(1) / D
        rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).sum(1) / D + eps)
    xh = (x - _d(mean)[:, None]) * _d(rstd)[:, None]
    rs = _d(rstd)[:, None]
    gg = dy * g
    c1 = gg.sum(1, keepdim=True) / D
    c2 = (gg * xh).sum(1, keepdim=True) / D
    dx = rs * (gg - c1 - xh * c2)
    mag = rs.abs() * (gg.abs() + gg.abs().sum(1, keepdim=True) / D + xh.abs() * (gg * xh).abs().sum(1, keepdim=True) / D)
    if dres is not None:
        dx = dx + dres
        mag = mag + dres.abs()
    mags = {"dx": mag, "dgamma": (dy * xh).abs().sum(0), "dbeta": dy.abs().sum(0)}
    return dx, (dy * xh).sum(0), dy.sum(0), mags


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------
def window_weights(R, win, halo, valid, device="cpu"):
    """The window rule as row weights: inside every window of `win` rows the rows [halo, halo + valid) are valid (1), the
    others excluded (-1); win = 0: every row is valid."""
    if win == 0:
        return torch.ones(R, dtype=F64, device=device)
    q = torch.arange(R, device=device) % win
    return torch.where((q >= halo) & (q < halo + valid), 1.0, -1.0).to(F64)


def bn_sums(y, w):
    """(s0, s1, mags): s0 = sum_r w_r y_r, s1 = sum_r w_r y_r^2 over the rows with w > 0; mags: s0 = sum w |y|, s1 = s1."""
    sel = w > 0
    ys, ws = _d(y[sel]), _d(w[sel])[:, None]
    s0, s1 = (ws * ys).sum(0), (ws * ys * ys).sum(0)
    return s0, s1, {"s0": (ws * ys.abs()).sum(0), "s1": s1.clone()}


def bn_finalize(s0, s1, n, eps, momentum=0.0, running_mean=None, running_var=None):
    """(mean, biased var, rstd, running_mean', running_var') from the sums over n rows; the running variance takes the
    unbiased n / (n - 1) variance."""
    s0, s1 = _d(s0), _d(s1)
    mean = s0 / n
    var = (s1 / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    unbias = n / (n - 1.0) if n > 1 else 1.0
    rm = None if running_mean is None else (1.0 - momentum) * _d(running_mean) + momentum * mean
    rv = None if running_var is None else (1.0 - momentum) * _d(running_var) + momentum * var * unbias
    return mean, var, rstd, rm, rv


def _yhat(y, mean, rstd):
    return (_d(y) - _d(mean)) * _d(rstd)


def bn_apply(y, w, mean, rstd, gamma, beta, relu=False):
    """z = yhat gamma + beta on the rows with w >= 0, zero elsewhere (relu: max(0, .) behind it).  mags: z = |yhat gamma| +
    |beta|, folded = (|y| + |mean|) |rstd gamma| + |beta| (the terms of z = y a + (beta - mean a)), pre / pre_mag: the
    pre-activation and its magnitude (for the ReLU kink)."""
    keep = w >= 0
    R, C = y.shape
    g, b, mu, rs = _d(gamma), _d(beta), _d(mean), _d(rstd)
    z = torch.zeros((R, C), dtype=F64, device=y.device)
    mag, fold, pre = torch.zeros_like(z), torch.zeros_like(z), torch.zeros_like(z)
    yk = _d(y[keep])
    yg = (yk - mu) * rs * g
    pre[keep] = yg + b
    z[keep] = (yg + b).clamp_min(0.0) if relu else yg + b
    mag[keep] = yg.abs() + b.abs()
    fold[keep] = (yk.abs() + mu.abs()) * (rs * g).abs() + b.abs()
    return z, {"z": mag, "folded": fold, "pre": pre, "pre_mag": mag}


def bn_relu_apply(y, mean, rstd, gamma, beta):
    return bn_apply(y, torch.ones(y.shape[0], dtype=F64, device=y.device), mean, rstd, gamma, beta, relu=True)


def _open(y, mean, rstd, gamma, beta):
    return _yhat(y, mean, rstd) * _d(gamma) + _d(beta) > 0


def bn_bwd_sums(dz, y, w, mean, rstd, gamma=None, beta=None):
    """(s0, s1, mags) = (sum dz, sum dz yhat) over the rows with w >= 0 (a row's dz is already the sum over its copies).
    gamma / beta given: a ReLU follows, dz counts where yhat gamma + beta > 0.  mags: s0 = sum |dz|, s1 = sum |dz yhat|."""
    keep = w >= 0
    d, yh = _d(dz[keep]), _yhat(y[keep], mean, rstd)
    if gamma is not None:
        d = torch.where(_open(y[keep], mean, rstd, gamma, beta), d, torch.zeros_like(d))     # a select: a closed element's dz is not read
    return d.sum(0), (d * yh).sum(0), {"s0": d.abs().sum(0), "s1": (d * yh).abs().sum(0)}


def bn_bwd_apply(dz, y, w, mean, rstd, gamma, s0, s1, inv_n, relu_mask=False, beta=None):
    """dy = gamma rstd (dz - w_r (s0 / n + yhat s1 / n)) on the rows with w >= 0, zero elsewhere; relu_mask: zero where
    y <= 0 (the ReLU that produced y); beta given: a ReLU follows the BatchNorm, dz counts where yhat gamma + beta > 0.
    mags: dy = the sum of the absolute terms."""
    keep = w >= 0
    R, C = y.shape
    g, rs, s0, s1 = _d(gamma), _d(rstd), _d(s0), _d(s1)
    d, yk, wk = _d(dz[keep]), _d(y[keep]), _d(w[keep])[:, None]
    yh = (yk - _d(mean)) * rs
    if beta is not None:
        d = torch.where(_open(y[keep], mean, rstd, gamma, beta), d, torch.zeros_like(d))
    v = g * rs * (d - wk * (s0 * inv_n + yh * (s1 * inv_n)))
    m = (g * rs).abs() * (d.abs() + wk * (s0.abs() * inv_n + yh.abs() * (s1.abs() * inv_n)))
    if relu_mask:
        v, m = torch.where(yk > 0, v, torch.zeros_like(v)), torch.where(yk > 0, m, torch.zeros_like(m))
    dy = torch.zeros((R, C), dtype=F64, device=y.device)
    mag = torch.zeros_like(dy)
    dy[keep], mag[keep] = v, m
    return dy, {"dy": mag}


def bn_relu_bwd(dz, y, mean, rstd, gamma, beta, inv_n, w=None):
    """Backward of z = max(0, BN(y)): (dy, s0, s1, mags); w: row weights for the mean terms (default: all ones)."""
    if w is None:
        w = torch.ones(y.shape[0], dtype=F64, device=y.device)
    s0, s1, ms = bn_bwd_sums(dz, y, w, mean, rstd, gamma, beta)
    dy, md = bn_bwd_apply(dz, y, w, mean, rstd, gamma, s0, s1, inv_n, beta=beta)
    return dy, s0, s1, {"dy": md["dy"], "s0": ms["s0"], "s1": ms["s1"]}


def tail_weights(R, LP, lead, w, device="cpu"):
    """Row weights of the compact padding form: inside every window of LP rows the first `lead` rows count once, the rest
    w times."""
    q = torch.arange(R, device=device) % LP
    return torch.where(q < lead, 1.0, float(w)).to(F64)


def bn_tail_expand(x, LP, lead, w):
    """x [B LP][C] -> (the expanded matrix of B (lead + w tail) rows, the row of x every expanded row copies)."""
    R = x.shape[0]
    B, tail = R // LP, LP - lead
    base = torch.arange(B, device=x.device)[:, None] * LP
    idx = torch.cat([base + torch.arange(lead, device=x.device)[None]] +
                    [base + lead + torch.arange(tail, device=x.device)[None]] * w, 1).reshape(-1)
    return x[idx], idx


def kink(pre, pre_mag, width):
    """Elements whose pre-activation is within `width` x its magnitude of zero: a ReLU there may open on one side only."""
    return pre.abs() <= width * pre_mag
