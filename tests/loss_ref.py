"""float64 references of the loss kernels (ntxent.hip, losses.hip), written from the definitions in plain torch (no
F.cross_entropy, F.normalize, logsumexp or cosine_similarity), plus the magnitudes (`mag*`: sums of the absolute values
of the terms of each output's own expression) the rounding bounds of tests/test_loss_paths_gpu.py multiply.  Every
function reads the kernel's own operands (bf16-rounded or fp32) and runs on the device they live on.

NT-Xent (header comment of ntxent.hip): a side is [q rows; k rows], n rows per half.  Row r of a side's q half has the
global id off + r, of its k half n_global + off + r.  The positive of global id g is g +- n_global; a resident row's own
column is excluded when the streamed side holds it; row_loss = lse - [positive present] logit(positive).
"""
import torch

F64 = torch.float64
NORM_EPS = float(torch.tensor(1e-12, dtype=torch.float32))     # losses.hip NORM_EPS as the fp32 value the kernels compare with
COS_EPS = float(torch.tensor(1e-8, dtype=torch.float32))       # losses.hip COS_EPS


# ---- NT-Xent -----------------------------------------------------------------------------------------------------------------
def _gids(n, off, ng, dev):
    r = torch.arange(n, device=dev)
    return torch.cat((off + r, ng + off + r))


def _b_index(gid, nb, off_b, ng):
    """Row of the streamed side with this global id, or -1."""
    first = gid < ng
    r = torch.where(first, gid, gid - ng) - off_b
    return torch.where((r >= 0) & (r < nb), torch.where(first, r, nb + r), torch.full_like(r, -1))


def _ntx_chunks(aq, ak, bq, bk, off_a, off_b, ng, T, chunk):
    """Yields (rows lo:hi, s = logits / T, lam = logits with absolute values / T, own-column mask, jpos) per row chunk."""
    A = torch.cat((aq, ak)).to(F64)
    B = torch.cat((bq, bk)).to(F64)
    Aa, Ba = A.abs(), B.abs()
    na, nb, dev = aq.shape[0], bq.shape[0], A.device
    ga = _gids(na, off_a, ng, dev)
    jself = _b_index(ga, nb, off_b, ng)
    jpos = _b_index(torch.where(ga < ng, ga + ng, ga - ng), nb, off_b, ng)
    cols = torch.arange(2 * nb, device=dev)
    for lo in range(0, 2 * na, chunk):
        hi = min(lo + chunk, 2 * na)
        s = (A[lo:hi] @ B.t()) / T
        lam = (Aa[lo:hi] @ Ba.t()) / T
        own = cols.unsqueeze(0) == jself[lo:hi].unsqueeze(1)
        yield lo, hi, B, Ba, s, lam, own, jpos[lo:hi]


def ntx_fwd(aq, ak, bq, bk, off_a, off_b, n_global, T, chunk=1024):
    """lse and row_loss of the 2 n_a resident rows.  Returns a dict with them and lam (per row: the largest logit with
    absolute values over T, which bounds |logit| / T and scales the logit rounding), has_pos, colw (per streamed column:
    the largest softmax weight it carries in any resident row; 0 for a column that is only ever an own column)."""
    na, nb, dev = aq.shape[0], bq.shape[0], aq.device
    lse = torch.empty(2 * na, dtype=F64, device=dev)
    loss, lamx = torch.empty_like(lse), torch.empty_like(lse)
    has_pos = torch.empty(2 * na, dtype=torch.bool, device=dev)
    colw = torch.zeros(2 * nb, dtype=F64, device=dev)
    for lo, hi, B, Ba, s, lam, own, jpos in _ntx_chunks(aq, ak, bq, bk, off_a, off_b, n_global, T, chunk):
        sm = s.masked_fill(own, float("-inf"))
        m = sm.amax(1, keepdim=True)
        e = torch.exp(sm - m)
        l = m.squeeze(1) + torch.log(e.sum(1))
        hp = jpos >= 0
        pl = torch.where(hp, s.gather(1, jpos.clamp(min=0).unsqueeze(1)).squeeze(1), torch.zeros_like(l))
        lse[lo:hi], loss[lo:hi], has_pos[lo:hi] = l, l - pl, hp
        lamx[lo:hi] = lam.amax(1)
        colw = torch.maximum(colw, torch.exp(sm - l.unsqueeze(1)).amax(0))
    return {"lse": lse, "row_loss": loss, "lam": lamx, "has_pos": has_pos, "colw": colw}


def ntx_bwd(aq, ak, bq, bk, off_a, off_b, n_global, T, lse_a, lse_b, gscale, chunk=1024):
    """dA_i = gscale / T sum_j w_ij B_j, w_ij = [lse_a] exp(s_ij - lse_a[i]) + [lse_b] exp(s_ij - lse_b[j]) - (#given) [j = pos_i],
    w_ij = 0 on the own column; the lse vectors are exact operands.  Returns dq, dk (n_a x d each), mag (same shapes:
    gscale / T sum_j (|exp terms| + (#given) [j = pos_i]) |B_jd|) and lam (2 n_a)."""
    na, d, dev = aq.shape[0], aq.shape[1], aq.device
    npos = (lse_a is not None) + (lse_b is not None)
    assert npos > 0
    dA = torch.empty(2 * na, d, dtype=F64, device=dev)
    mag, lamx = torch.empty_like(dA), torch.empty(2 * na, dtype=F64, device=dev)
    la = lse_a.to(F64) if lse_a is not None else None
    lb = lse_b.to(F64) if lse_b is not None else None
    for lo, hi, B, Ba, s, lam, own, jpos in _ntx_chunks(aq, ak, bq, bk, off_a, off_b, n_global, T, chunk):
        e = torch.zeros_like(s)
        if la is not None:
            e += torch.exp(s - la[lo:hi].unsqueeze(1))
        if lb is not None:
            e += torch.exp(s - lb.unsqueeze(0))
        pos = torch.zeros_like(s)
        hp = jpos >= 0
        pos[torch.nonzero(hp).squeeze(1), jpos[hp]] = float(npos)
        w = (e - pos).masked_fill(own, 0.0)
        wa = (e + pos).masked_fill(own, 0.0)
        dA[lo:hi] = (gscale / T) * (w @ B)
        mag[lo:hi] = abs(gscale / T) * (wa @ Ba)
        lamx[lo:hi] = lam.amax(1)
    return {"dq": dA[:na], "dk": dA[na:], "mag_dq": mag[:na], "mag_dk": mag[na:], "lam": lamx}


# ---- cosine row loss ---------------------------------------------------------------------------------------------------------
def _cos_parts(x, y):
    x, y = x.to(F64), y.to(F64)
    nx, ny = (x * x).sum(1).sqrt(), (y * y).sum(1).sqrt()
    dx, dy = nx.clamp(min=NORM_EPS), ny.clamp(min=NORM_EPS)
    return x, y, nx, dx, dy, (x * y).sum(1), (x * y).abs().sum(1)


def cos_rows(x, y):
    """2 - 2 <x / max(|x|, eps), y / max(|y|, eps)> per row.  mags: cos and mdot = sum_d |x_d y_d| / (dx dy)."""
    x, y, nx, dx, dy, dot, adot = _cos_parts(x, y)
    cos = dot / (dx * dy)
    return {"row_loss": 2.0 - 2.0 * cos, "cos": cos, "mdot": adot / (dx * dy)}


def cos_rows_bwd(x, y, gscale):
    """gscale d(row_loss) / dx = a1 y + a2 x, a1 = -2 g / (dx dy), a2 = 2 g dot / (dx^3 dy) where |x| > eps and 0 where the
    clamp holds.  mags: t1 = |a1 y|, t2 = |a2 x|, t3 = 2 |g| sum|x y| / (dx^3 dy) |x| (what an error of the dot moves)."""
    x, y, nx, dx, dy, dot, adot = _cos_parts(x, y)
    live = (nx > NORM_EPS).to(F64)
    a1 = -2.0 * gscale / (dx * dy)
    a2 = live * 2.0 * gscale * dot / (dx ** 3 * dy)
    a3 = live * 2.0 * abs(gscale) * adot / (dx ** 3 * dy)
    return {"dx": a1.unsqueeze(1) * y + a2.unsqueeze(1) * x, "t1": (a1.unsqueeze(1) * y).abs(), "t2": (a2.unsqueeze(1) * x).abs(),
            "t3": a3.unsqueeze(1) * x.abs()}


# ---- cross entropy over rows ---------------------------------------------------------------------------------------------------
def ce_rows(logits, labels, C, ignore):
    """logits (N, >= C): lse (N,), mean loss over the counted rows, their count.  A label that is not `ignore` counts; outside
    [0, C) it makes the mean NaN; no counted row gives NaN (0 / 0).  mags: mag_lse = |m| + |log sum| + sum_c p_c |x_c - m|,
    row_loss and mag_loss = |lse| + |x_y| per counted valid row (0 elsewhere)."""
    x = logits[:, :C].to(F64)
    m = x.amax(1)
    e = torch.exp(x - m.unsqueeze(1))
    ssum = e.sum(1)
    lse = m + torch.log(ssum)
    counted = labels != ignore
    valid = counted & (labels >= 0) & (labels < C)
    xy = x.gather(1, labels.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    row = torch.where(valid, lse - xy, torch.zeros_like(lse))
    cnt = int(counted.sum())
    bad = bool((counted & ~valid).any())
    mean = float("nan") if (cnt == 0 or bad) else float(row.sum()) / cnt
    p = e / ssum.unsqueeze(1)
    return {"lse": lse, "mean": mean, "count": cnt, "row_loss": row, "valid": valid,
            "mag_lse": m.abs() + torch.log(ssum).abs() + (p * (x - m.unsqueeze(1)).abs()).sum(1),
            "mag_loss": torch.where(valid, lse.abs() + xy.abs(), torch.zeros_like(lse))}


def ce_rows_bwd(logits, labels, C, ignore, lse, count, gout, Cp):
    """dlogits (N, Cp) = gout / count (exp(x - lse) - [c == label]) for valid counted rows while count > 0, zero elsewhere
    (ignored rows, rows with a label outside [0, C), the columns [C, Cp)).  lse, count, gout are exact operands.
    mags: mag = |g| (p + [c == label]); xl = |x - lse| (the exponent the fast exp rounds)."""
    x = logits[:, :C].to(F64)
    N = x.shape[0]
    valid = (labels != ignore) & (labels >= 0) & (labels < C) & (count > 0)
    g = float(gout) / float(count) if count > 0 else 0.0
    p = torch.exp(x - lse.to(F64).unsqueeze(1))
    hot = torch.zeros_like(x)
    hot[torch.arange(N, device=x.device), labels.clamp(0, C - 1)] = 1.0
    on = valid.unsqueeze(1)
    d = torch.zeros(N, Cp, dtype=F64, device=x.device)
    mag, xl = torch.zeros_like(d), torch.zeros_like(d)
    d[:, :C] = torch.where(on, g * (p - hot), torch.zeros_like(p))            # a select: an uncounted row's logits are not read
    mag[:, :C] = torch.where(on, abs(g) * (p + hot), torch.zeros_like(p))
    xl[:, :C] = (x - lse.to(F64).unsqueeze(1)).abs()
    return {"dlogits": d, "mag": mag, "xl": xl}


# ---- triplet loss with distance 1 - sigmoid(cos) -----------------------------------------------------------------------------
def triplet(p, d, gt, margin):
    """gt (n_p, n_d) int8: 1 positive, 0 negative, -1 ignored.  Anchor i with positives and negatives: every (positive,
    negative) pair is a triplet with hinge argument dist(i, pos) - dist(i, neg) + margin; with negatives only: the anchor
    is its own positive (dist(i, i)); without negatives: none.  loss = sum of hinges / max(n_tri, 1).  Each norm is clamped
    at 1e-8.  Returns dist, cos, mdot (sum_c |p_c d_c| / (|p| |d|)), selfd, loss, n_tri, dp, dd (gradients of the loss),
    hv (1-d: every triplet's hinge argument), hinge_sum, and the gradient magnitudes mag_dp / mag_dd =
    sum |G| (|other_c| / (|p| |d|) + mdot |own_c| / |own|^2)."""
    p, d = p.to(F64), d.to(F64)
    n_p, n_d = gt.shape
    pn = (p * p).sum(1).sqrt().clamp(min=COS_EPS)
    dn = (d * d).sum(1).sqrt().clamp(min=COS_EPS)
    den = pn.unsqueeze(1) * dn.unsqueeze(0)
    cos = (p @ d.t()) / den
    mdot = (p.abs() @ d.abs().t()) / den
    dist = 1.0 - 1.0 / (1.0 + torch.exp(-cos))
    selfd = 1.0 - 1.0 / (1.0 + torch.exp(-(p * p).sum(1) / (pn * pn)))
    coef = torch.zeros_like(dist)
    hvs, total, n_tri = [], 0.0, 0
    for i in range(n_p):
        pos = torch.nonzero(gt[i] == 1).squeeze(1)
        neg = torch.nonzero(gt[i] == 0).squeeze(1)
        if len(neg) == 0:
            continue
        if len(pos) > 0:
            hv = dist[i, pos].unsqueeze(1) - dist[i, neg].unsqueeze(0) + margin
            act = (hv > 0).to(F64)
            coef[i, pos] += act.sum(1)
            coef[i, neg] -= act.sum(0)
        else:
            hv = selfd[i] - dist[i, neg] + margin
            act = (hv > 0).to(F64)
            coef[i, neg] -= act
        total += float((hv * act).sum())
        n_tri += hv.numel()
        hvs.append(hv.reshape(-1))
    nt = max(n_tri, 1)
    sg = 1.0 - dist
    G = -sg * (1.0 - sg) * coef / nt                               # d loss / d cos
    Ga = G.abs()
    dp = (G / den) @ d - (G * cos).sum(1, keepdim=True) * p / (pn * pn).unsqueeze(1)
    dd = (G / den).t() @ p - (G * cos).sum(0).unsqueeze(1) * d / (dn * dn).unsqueeze(1)
    mag_dp = (Ga / den) @ d.abs() + (Ga * mdot).sum(1, keepdim=True) * p.abs() / (pn * pn).unsqueeze(1)
    mag_dd = (Ga / den).t() @ p.abs() + (Ga * mdot).sum(0).unsqueeze(1) * d.abs() / (dn * dn).unsqueeze(1)
    hv = torch.cat(hvs) if hvs else torch.zeros(0, dtype=F64, device=p.device)
    return {"dist": dist, "cos": cos, "mdot": mdot, "selfd": selfd, "loss": total / nt, "n_tri": n_tri, "dp": dp, "dd": dd,
            "hv": hv, "hinge_sum": total, "mag_dp": mag_dp, "mag_dd": mag_dd, "coef": coef}

