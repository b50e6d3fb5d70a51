"""fp64 reference of the hit attributions (dl_pgca_pairs_attr / dl_pgca_pairs_ragged_attr, include/druglamp_hip.h) and their
element bounds.

The quantity, for one pair: q (Lq, hd) queries, K | V (Lk, hd) the drug's stored rows, wk (Lk,) the multiplicity of a stored key
(1 in front of the tail, w on the last t rows), dO (Lq, hd) the gradient of the target w.r.t. the attention output, and
optionally sites / dL (Lq, left) the left half of the concat and its gradient:
    s = scale q K^T      p = exp(s) / sum_c wk exp(s)      g = dO V^T      D = sum_c wk p g      ds = p (g - D)
    key [c] = sum_r (ds s + p g)        one copy's value of stored key c  = (<dK_c, K_c> + <dV_c, V_c>) / wk_c
    site[r] = sum_c wk ds s  (+ <dL_r, sites_r>)                          = <dq_r, q_r> (+ <dsites_r, sites_r>)
and the identity  sum over the EXPANDED columns of key = sum_r sum_c wk ds s + sum_r D[r],  D[r] = <dO_r, O_r>.

The bound.  No fitted tolerance: it is put together from
    bp[r, c]   the element bound of one copy's probability, tests/test_pgca_pairs_probs_gpu._drug_map's
               b = 2 p ((hd + 2) u_f (lam + mag_lse) + (F + 8) u_f) + 2^-120   (MARGIN = 2 inside);
    es, eg     the fp32 dot products:  MARGIN (hd + 2) u_f scale sum_i |q_i K_i|  and  MARGIN (hd + 2) u_f sum_i |dO_i V_i|
               (hd products and additions, the scale multiply and one spare rounding);
    fp32 sums  of n terms:  MARGIN (n + 8) u_f sum |terms|,  over the Lk stored keys or the Lq rows, as the siblings write them;
and propagated to first order (MARGIN covers the products of two errors) through the formulas.  The outputs are signed and
cancel, so every step is bounded relative to the sum of ABSOLUTE values it handles and the result is an absolute bound:
    D     eD   = sum_c wk (bp |g| + p eg) + MARGIN (Lk + 8) u_f sum_c wk p |g|
               (the kernel's sweep-1 weights e / l are an evaluation of p under the same model as bp: fp32 scores, exp2, an fp32
                sum of the keys)
    ds    a_ds = p (|g| + |D|) >= |ds|,   e_ds = bp (|g| + |D|) + p (eg + eD) + 3 MARGIN u_f a_ds      (subtract, multiply, wk)
    T = ds s + p g:   a_T = a_ds |s| + p |g|,   e_T = e_ds |s| + a_ds es + bp |g| + p eg + 3 MARGIN u_f a_T
    key [c]:  sum_r e_T + MARGIN (Lq + 8) u_f sum_r a_T + 2^-120
    site[r]:  sum_c wk (e_ds |s| + a_ds es) + MARGIN (Lk + 11) u_f sum_c wk a_ds |s|
              + MARGIN (left + 2) u_f sum_i |dL_i sites_i| + 2^-120                                     (the left half's fp32 dot)
"""
import torch

U_F, MARGIN, FLOOR = 2.0 ** -24, 2.0, 2.0 ** -120


def key_weights(Lk, t, w, device=None):
    wk = torch.ones(Lk, dtype=torch.float64, device=device)
    if t:
        wk[Lk - t:] = float(w)
    return wk


def closed_form(q, K, V, dO, t, w, scale, sites=None, dL=None):
    """The fp64 closed form of one pair (operands of any dtype; they are taken as given and promoted).  Returns a dict with key
    (Lk,), site (Lq,), the intermediates the bounds need, and the two sides' ingredients of the identity."""
    q, K, V, dO = q.double(), K.double(), V.double(), dO.double()
    wk = key_weights(K.shape[0], t, w, q.device)
    s = scale * (q @ K.t())
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    p = e / (wk * e).sum(-1, keepdim=True)
    g = dO @ V.t()
    D = (wk * p * g).sum(-1, keepdim=True)
    ds = p * (g - D)
    core = (wk * ds * s).sum(-1)
    left = (dL.double() * sites.double()).sum(-1) if sites is not None else torch.zeros_like(core)
    return dict(s=s, p=p, g=g, D=D, ds=ds, wk=wk, key=(ds * s + p * g).sum(0), site=core + left, core=core,
                abs_qk=scale * (q.abs() @ K.abs().t()), abs_gv=dO.abs() @ V.abs().t(),
                abs_left=(dL.double() * sites.double()).abs().sum(-1) if sites is not None else torch.zeros_like(core),
                left_cols=0 if sites is None else sites.shape[-1])


def bounds(r, bp, hd=128):
    """(bound of key (Lk,), bound of site (Lq,)) of closed_form's result r, with bp (Lq, Lk) the element bound of p."""
    s, p, g, D, wk = r["s"].abs(), r["p"], r["g"].abs(), r["D"].abs(), r["wk"]
    Lq, Lk = p.shape
    es, eg = MARGIN * (hd + 2) * U_F * r["abs_qk"], MARGIN * (hd + 2) * U_F * r["abs_gv"]
    eD = (wk * (bp * g + p * eg)).sum(-1, keepdim=True) + MARGIN * (Lk + 8) * U_F * (wk * p * g).sum(-1, keepdim=True)
    a_ds = p * (g + D)
    e_ds = bp * (g + D) + p * (eg + eD) + 3 * MARGIN * U_F * a_ds
    a_T = a_ds * s + p * g
    e_T = e_ds * s + a_ds * es + bp * g + p * eg + 3 * MARGIN * U_F * a_T
    key_b = e_T.sum(0) + MARGIN * (Lq + 8) * U_F * a_T.sum(0) + FLOOR
    site_b = ((wk * (e_ds * s + a_ds * es)).sum(-1) + MARGIN * (Lk + 11) * U_F * (wk * a_ds * s).sum(-1)
              + MARGIN * (r["left_cols"] + 2) * U_F * r["abs_left"] + FLOOR)
    return key_b, site_b


def expand(v, t, w, cols):
    """A per-stored-key vector (Lk,) in the columns of the drug's full key set (copy i of tail key j at lead + i t + j), zeros
    from the drug's own count up to cols."""
    lead = v.shape[0] - t
    full = torch.cat([v[:lead], v[lead:].repeat(int(w))]) if t else v
    out = torch.zeros(cols, dtype=v.dtype, device=v.device)
    out[:full.shape[0]] = full
    return out


def autograd_form(q, K, V, dO, t, w, scale, sites=None, dL=None):
    """The same two outputs as torch fp64 autograd gradient x value on the leaves q, sites, K, V, the forward written out with
    the tail keys physically expanded: (key (Lk,) per copy, site (Lq,), O (Lq, hd))."""
    q, K, V = (x.double().clone().requires_grad_(True) for x in (q, K, V))
    lead, copies = K.shape[0] - t, int(w) if t else 1
    Kf = torch.cat([K[:lead], K[lead:].repeat(copies, 1)]) if t else K
    Vf = torch.cat([V[:lead], V[lead:].repeat(copies, 1)]) if t else V
    O = torch.softmax(scale * (q @ Kf.t()), -1) @ Vf
    target = (dO.double() * O).sum()
    leaves = [q, K, V]
    if sites is not None:
        sl = sites.double().clone().requires_grad_(True)
        target = target + (dL.double() * sl).sum()           # the concat's left half IS sites: d target / d sites = dL
        leaves.append(sl)
    grads = torch.autograd.grad(target, leaves)
    site = (grads[0] * q).sum(-1)
    if sites is not None:
        site = site + (grads[3] * sl).sum(-1)
    key = ((grads[1] * K).sum(-1) + (grads[2] * V).sum(-1)) / key_weights(K.shape[0], t, w, K.device)
    return key.detach(), site.detach(), O.detach()


def case_reference(s, extra, with_sites):
    """The reference of a whole case of tests/test_pgca_pairs_probs_gpu._setup (s; expanded) with the gradients of `extra`
    (dict: d_out (n, Lq, hd), d_sites (n, Lq, hd), sites (n_q, Lq, hd)): key (n, cols), its bound, site (n, Lq), its bound, and
    per pair the identity's ingredients core_sum = sum_r sum_c wk ds s and d_sum = sum_r D[r]."""
    c = s["c"]
    E = s["q"].shape[-1]
    n = s["n"]
    dev = s["q"].device
    key = torch.zeros(n, c.cols, dtype=torch.float64, device=dev)
    key_b = torch.zeros_like(key)
    site = torch.zeros(n, c.Lq, dtype=torch.float64, device=dev)
    site_b = torch.zeros_like(site)
    core_sum = torch.zeros(n, dtype=torch.float64, device=dev)
    d_sum = torch.zeros_like(core_sum)
    pi, di = s["pi"].tolist(), s["di"].tolist()
    row0 = s["row0"].tolist()
    for i in range(n):
        Lk, w = c.drugs[di[i]]
        rows = s["rows"][row0[di[i]]:row0[di[i]] + Lk]
        r = closed_form(s["q"][pi[i]], rows[:, :E], rows[:, E:], extra["d_out"][i], c.tail_rows, w, s["scale"],
                        extra["sites"][pi[i]] if with_sites else None, extra["d_sites"][i] if with_sites else None)
        kb, sb = bounds(r, s["bound"][i, :, :Lk], E)
        key[i], key_b[i] = expand(r["key"], c.tail_rows, w, c.cols), expand(kb, c.tail_rows, w, c.cols)
        site[i], site_b[i] = r["site"], sb
        core_sum[i], d_sum[i] = r["core"].sum(), r["D"].sum()
    return dict(key=key, key_b=key_b, site=site, site_b=site_b, core_sum=core_sum, d_sum=d_sum)
