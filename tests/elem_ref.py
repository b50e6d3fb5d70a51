"""fp64 / integer references of the elementwise (elementwise.hip), row-table (compact.hip) and graph (graph.hip) kernels,
one function per operation, written from the contracts in the kernels' header comments and the reference model's
formulas.  Plain torch on whatever device the operands live on (no GPU needed); arithmetic outputs come with `mag`, the
sum of the absolute terms of the output's own expression.  The references read the kernels' own (bf16 / fp32) operands.
"""
import math

import numpy as np
import torch

F64 = torch.float64


# ---- round to nearest even, fp32 -> bf16, on the bit patterns -------------------------------------------------------------------
def bf16_rne_bits(x):
    """The 16-bit pattern (int64 tensor, 0..65535) of fp32 `x` rounded to bf16 to nearest, ties to even: add 0x7fff plus the
    lowest kept bit to the 32-bit pattern, keep the upper half.  Infinities stay, finite values beyond the largest bf16
    round to infinity, fp32 subnormals round like any other value (to +-0 or the smallest bf16 subnormals).  No NaN."""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16) & 0xffff


def bf16_trunc_bits(x):
    """The same by truncation (the planted error of the CPU test)."""
    return ((x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff) >> 16) & 0xffff


def bits_to_bf16(bits):
    b = bits.to(torch.int64)
    return (b - ((b & 0x8000) << 1)).to(torch.int16).view(torch.bfloat16)


def bits16(t):
    """bf16 tensor -> its bit patterns as int64 in 0..65535."""
    return t.contiguous().view(torch.int16).to(torch.int64) & 0xffff


def cast(src, ddt):
    """dl_cast: the value of src in ddt, round to nearest even where ddt is narrower."""
    if src.dtype == ddt:
        return src.clone()
    if ddt == torch.float32:
        return src.float()                                   # bf16 -> fp32 is exact
    return bits_to_bf16(bf16_rne_bits(src)).reshape(src.shape)


# ---- dropout mask: the contract of common.cuh ---------------------------------------------------------------------------------
# This replica is the SPECIFICATION of the mask, not a copy of one kernel: the standalone dropout kernels and every GEMM
# epilogue must draw the same bits from (seed, group index), because forward and backward of one dropout site run in
# different kernels and regenerate the mask instead of storing it.
#   group g = (row * ncols + col) >> 2 serves elements 4g .. 4g + 3 of the logical [rows][ncols] tensor,
#   bits64 = splitmix(seed, g), element j of the group takes bits 16 j .. 16 j + 15, keep = bits16 >= thr16,
#   thr16 = clamp(floor(fl(fl(p) * 65536 + 0.5)), 0, 65535); kept elements are scaled by fl(1 / (1 - p)).
#   thr16 == 0 (p == 0 or p < 2^-17) is no dropout at all: nothing dropped, nothing scaled.
_M32 = np.uint64(0xffffffff)


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & _M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & _M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & _M32
    h ^= h >> np.uint64(16)
    return h


def splitmix(seed, idx):
    """64 bits per (seed, group index); numpy uint64 arithmetic, 32-bit lanes masked by hand."""
    seed = np.uint64(int(seed) & 0xffffffffffffffff)
    idx = np.asarray(idx, dtype=np.uint64)
    x = ((idx & _M32) + (seed & _M32)) & _M32
    hi = ((idx >> np.uint64(32)) ^ (seed >> np.uint64(32))) & _M32
    a = fmix32(x ^ hi)
    rot = ((hi << np.uint64(13)) | (hi >> np.uint64(19))) & _M32
    b = fmix32(((x + np.uint64(0x9E3779B9)) & _M32) ^ rot ^ np.uint64(0x7F4A7C15))
    return (a << np.uint64(32)) | b


def dropout_thr16(p):
    t = np.float32(np.float32(p) * np.float32(65536.0)) + np.float32(0.5)
    return 0 if t <= 0 else (65535 if t >= 65535 else int(t))


def keep_mask(seed, rows, ncols, thr16):
    """[rows][ncols] bool numpy array: True where the element is kept."""
    e = np.arange(rows * ncols, dtype=np.uint64)
    bits = splitmix(seed, e >> np.uint64(2))
    b16 = (bits >> (np.uint64(16) * (e & np.uint64(3)))) & np.uint64(0xffff)
    return (b16 >= np.uint64(thr16)).reshape(rows, ncols)


def inv_keep(p):
    """The fp32 scale of the kept elements; 1 where p rounds to thr16 == 0 (no dropout)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if dropout_thr16(p) else 1.0


def dropout(x, keep, p):
    """y = keep ? x fl(1 / (1 - p)) : 0 in fp64; x may already hold a sum (positional add)."""
    y = torch.where(keep, x.double() * inv_keep(p), torch.zeros((), dtype=F64, device=x.device))
    return y, y.abs()


def add_rowmod(x, pe, L):
    """x[r] + pe[r mod L] in fp64 and its magnitude."""
    x = x.double()
    if pe is None:
        return x, x.abs()
    idx = torch.arange(x.shape[0], device=x.device) % L
    p = pe.double()[idx]
    return x + p, x.abs() + p.abs()


# ---- MHLA token gate ----------------------------------------------------------------------------------------------------------
def gate_softmax(logits):
    """gate[b][j][l] = softmax_l(logits[b][l][j]); also d[b][j][l] = max_l' x - x (the exponent a fast exp sees)."""
    x = logits.double()
    d = x.max(dim=1, keepdim=True).values - x
    e = torch.exp(-d)
    g = e / e.sum(dim=1, keepdim=True)
    return g.permute(0, 2, 1).contiguous(), d.permute(0, 2, 1).contiguous()


def gate_flat_index(L, D, H, device):
    """For the flat element f of a sample's [L][D] block: (j, l) with gate_flat[f / hd] = gate[j][l], the reference model's
    reinterpretation of the [H][L] gate block as L*H consecutive values, by index."""
    hd = D // H
    k = torch.arange(L * D, device=device) // hd
    return k // L, k % L


def token_gate_fwd(v, logits, H, res):
    B, L, D = v.shape
    gate, d = gate_softmax(logits)
    j, l = gate_flat_index(L, D, H, v.device)
    gf = gate[:, j, l]                                       # [B][L * D]
    vv = v.double().reshape(B, L * D)
    out = vv * (gf + res)
    return gate, d, out.reshape(B, L, D), {"out": (vv.abs() * (gf + res)).reshape(B, L, D), "vg": (vv.abs() * gf).reshape(B, L, D),
                                           "j": j, "l": l}


def token_gate_bwd(dout, v, gate, H, res):
    """dv = dout (g + res); dgate[b][j][l] = sum_c dout v over the hd elements of flat row (j L + l); dlogits[b][l][j] =
    g (dgate - sum_l g dgate)."""
    B, L, D = v.shape
    hd = D // H
    do, vv, g = dout.double().reshape(B, H, L, hd), v.double().reshape(B, H, L, hd), gate.double()
    dv = do * (g[..., None] + res)
    dg = (do * vv).sum(-1)
    A = (do * vv).abs().sum(-1)
    dot = (g * dg).sum(-1, keepdim=True)
    Dabs = (g * A).sum(-1, keepdim=True)
    dl = g * (dg - dot)
    return dv.reshape(B, L, D), dl.permute(0, 2, 1).contiguous(), {"dv": dv.abs().reshape(B, L, D),
                                                                     "dlogits": (g * (A + Dabs)).permute(0, 2, 1).contiguous()}


# ---- GELU derivative ----------------------------------------------------------------------------------------------------------
def gelu_grad(x):
    """Phi(x) + x phi(x) in fp64 (Phi through erfc: no cancellation in the lower tail) and Phi + |x| phi."""
    x = x.double()
    cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return cdf + x * pdf, cdf + x.abs() * pdf


def gelu_bwd(dy, pre):
    g, _ = gelu_grad(pre)
    dx = dy.double() * g
    return dx, dx.abs()


def gate_dpre(dl, w2, pre):
    """dpre[r][c] = gelu'(pre[r][c]) sum_h dl[r][h] w2[h][c]; returns dpre, acc, S = sum_h |dl||w2|, gelu'."""
    acc = dl.double() @ w2.double()
    S = dl.double().abs() @ w2.double().abs()
    g, _ = gelu_grad(pre)
    return acc * g, acc, S, g


def gelu_grad_rational_f32(x):
    """gelu_grad_fast2 of common.cuh in fp32 numpy arithmetic (the documented rational fit; fused multiply-adds emulated in
    fp64 and rounded once, the reciprocal correctly rounded)."""
    f = np.float32
    x = np.clip(np.asarray(x, dtype=f), f(-5.5), f(5.5))
    x2 = (x * x).astype(f)

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(f)
    p = fma(np.full_like(x, f(1.6454146817e-04)), x2, f(1.4818409354e-02))
    p = fma(p, x2, f(-2.9252399590e-02))
    p = fma(p, x2, f(7.9844805043e-01))
    q = fma(np.full_like(x, f(5.5159476634e-03)), x2, f(3.8876839848e-02))
    q = fma(q, x2, f(3.0011850475e-01))
    q = fma(q, x2, f(1.0))
    r = (f(1.0) / q).astype(f)
    return fma((x * p).astype(f), r, f(0.5))


# ---- LLM feature ingest ---------------------------------------------------------------------------------------------------------
def fill_pool(x, site_len):
    """x [B][S][F] -> fill [B][S] (1 where the row sums to zero), pooled [B][n_site][Fp] = mean over the site_len rows
    c n_site + j of xcat = [x | fill], zero in columns F + 1 .. Fp - 1; mag likewise; rowsum / rowabs for the data condition."""
    B, S, F = x.shape
    n_site, Fp = S // site_len, (F + 1 + 7) // 8 * 8
    xd = x.double()
    rowsum, rowabs = xd.sum(-1), xd.abs().sum(-1)
    fill = (rowsum == 0).double()
    xcat = torch.cat((xd, fill[..., None]), -1).reshape(B, site_len, n_site, F + 1)
    pooled = torch.zeros(B, n_site, Fp, dtype=F64, device=x.device)
    mag = torch.zeros_like(pooled)
    pooled[..., :F + 1] = xcat.sum(1) / site_len
    mag[..., :F + 1] = xcat.abs().sum(1) / site_len
    return fill, pooled, mag, rowsum, rowabs


def rowmod_sum(x, L, old=None):
    """out[l][d] = (old +) sum_b x[b L + l][d]."""
    M, D = x.shape
    xd = x.double().reshape(M // L, L, D)
    out, mag = xd.sum(0), xd.abs().sum(0)
    if old is not None:
        out, mag = out + old.double(), mag + old.double().abs()
    return out, mag


# ---- AdamW ----------------------------------------------------------------------------------------------------------------------
def adamw(p, g, m, v, lr, b1, b2, eps, wd, step, gscale):
    """Decoupled decay; the scalars are the fp32 values the C ABI receives, everything else fp64.  Returns p', m', v' and the
    pieces the bound needs."""
    f = lambda s: float(np.float32(s))                       # noqa: E731
    lr, b1, b2, eps, wd, gscale = map(f, (lr, b1, b2, eps, wd, gscale))
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    grad = g * gscale
    m1 = b1 * m + (1 - b1) * grad
    v1 = b2 * v + (1 - b2) * grad * grad
    den = v1.sqrt() / bc2s + eps
    u = (lr / bc1) * (m1 / den)
    x = p * (1 - lr * wd)
    return x - u, m1, v1, {"m": (b1 * m).abs() + ((1 - b1) * grad).abs(), "v": v1, "u": u.abs(), "x": x.abs(), "den": den,
                           "sqrt_v": v1.sqrt(), "step_scale": lr / bc1, "eps": eps,
                           "amp1": b1 ** step / bc1, "amp2": b2 ** step / (bc2s * bc2s)}


# ---- MolecularGCN ---------------------------------------------------------------------------------------------------------------
def norm_adjacency(adj):
    """ahat[b][i][j] = din[i] adj[b][j][i] dout[j]; dout[j] = clamp(sum_i adj[j][i], 1)^-1/2, din[i] = clamp(sum_j adj[j][i], 1)^-1/2.
    Also the raw degree sums (for the data condition at the clamp)."""
    a = adj.double()
    so, si = a.sum(2), a.sum(1)
    dout, din = so.clamp_min(1.0).rsqrt(), si.clamp_min(1.0).rsqrt()
    ahat = din[:, :, None] * a.transpose(1, 2) * dout[:, None, :]
    return ahat, ahat.abs(), so, si


def graph_aggregate(ahat, feat, n, transpose):
    """out[b][i] = sum_j A'[b][i][j] feat[b][j] for i < n (A' = ahat or its transpose), feat[b][i] for n <= i < N."""
    a, f = ahat.double(), feat.double()
    if transpose:
        a = a.transpose(1, 2)
    out, mag = f.clone(), f.abs()
    out[:, :n] = a @ f[:, :n]
    mag[:, :n] = a.abs() @ f[:, :n].abs()
    return out, mag


# ---- pure data movers (by index; bit-exact) ---------------------------------------------------------------------------------------
def gather_pad(store, offsets, lengths, S, repeat):
    """out[b][s] = store[offsets[b] + (s mod len_b)] for s < reps_b len_b, zero afterwards; repeat: reps_b = S / len_b
    (len_b > S: all zero), else reps_b = 1 and at most S rows; len_b <= 0: all zero."""
    B, F = len(lengths), store.shape[1]
    out = torch.zeros(B, S, F, dtype=store.dtype, device=store.device)
    for b in range(B):
        ln, off = int(lengths[b]), int(offsets[b])
        filled = 0 if ln <= 0 else ((S // ln) * ln if repeat else min(ln, S))
        if filled:
            s = torch.arange(filled, device=store.device)
            out[b, :filled] = store[off + (s % ln if repeat else s)]
    return out


def embed_pad(ids, weight, fill, D, halo):
    """out[b][halo + l] = [weight[clamp(ids[b][l], 0, V - 1)][:D] | fill[b][l]], halo rows zero.  weight [V][D + 1] (last
    column unused)."""
    B, L = ids.shape
    V = weight.shape[0]
    out = torch.zeros(B, L + 2 * halo, D + 1, dtype=weight.dtype, device=weight.device)
    out[:, halo:halo + L, :D] = weight[ids.clamp(0, V - 1)][..., :D]
    out[:, halo:halo + L, D] = fill
    return out


def embed_rows(ids, weight, fill, src, D):
    """out[r] = [weight[clamp(ids[src[r]])][:D] | fill[src[r]]], zero rows where src[r] < 0 (ids, fill flat)."""
    V = weight.shape[0]
    s = src.long().clamp_min(0)
    out = torch.zeros(src.numel(), D + 1, dtype=weight.dtype, device=weight.device)
    out[:, :D] = weight[ids.reshape(-1)[s].clamp(0, V - 1)][:, :D]
    out[:, D] = fill.reshape(-1)[s]
    out[src < 0] = 0
    return out


def rows_gather(src, index):
    out = src[index.long().clamp_min(0)].clone()
    out[index < 0] = 0
    return out


def rows_sum_strided(x, rep):
    """out[r] = sum_{k < count_r} x[first_r + k stride_r] in fp64, and the sum of the absolute terms."""
    R, C = rep.shape[0], x.shape[1]
    out = torch.zeros(R, C, dtype=F64, device=x.device)
    mag = torch.zeros_like(out)
    xd = x.double()
    first, stride, count = (rep[:, i].long() for i in range(3))
    for k in range(int(count.max()) if R else 0):
        live = count > k
        rows = (first + k * stride)[live]
        out[live] += xd[rows]
        mag[live] += xd[rows].abs()
    return out, mag


def interleave_streams(split, inverse_of=None):
    """split [S][R][row] -> [R][S * row] (forward); `inverse_of` [R][S * row] -> [S][R][row]."""
    if inverse_of is None:
        S, R, W = split.shape
        return split.permute(1, 0, 2).reshape(R, S * W).clone()
    R, S, W = inverse_of
    return split.reshape(R, S, W).permute(1, 0, 2).clone()


def concat2(a, b):
    return torch.cat((a, b), 1)


def weight_prep_item(image, src, ld, row0, mode, cs=0):
    """Write one item into the flat image `image` (values of the image's dtype, rounded to nearest even): plain (0)
    image[(row0 + r) ld + c], transposed (1) image[c ld + row0 + r], strided (2) image[row0 + r ld + c cs] = src[r][c]."""
    rows, cols = src.shape
    r = torch.arange(rows, device=src.device)[:, None]
    c = torch.arange(cols, device=src.device)[None, :]
    idx = (row0 + r) * ld + c if mode == 0 else (c * ld + row0 + r if mode == 1 else row0 + r * ld + c * cs)
    image[idx.reshape(-1)] = cast(src.float(), image.dtype).reshape(-1)
    return idx.reshape(-1)


# ---- ProteinCNN tail ------------------------------------------------------------------------------------------------------------
def sitepool_index(L, C, S, device):
    """For output o = n_site q + r of a sample (q < C, r < n_site) and s < S: (body row, channel) of the contribution,
    row = n_site ((s C + q) % S) + r, channel = (s C + q) / S."""
    n_site = L // S
    o = torch.arange(n_site * C, device=device)
    q, r = o // n_site, o % n_site
    s = torch.arange(S, device=device)[:, None]
    t = s * C + q[None, :]
    return n_site * (t % S) + r[None, :], t // S            # [S][n_site * C] each


def sitepool_fwd(zbody, S):
    """zbody [B][L][C] (the L body rows of every sample, halo removed or gathered through row_of) -> pooled [B][n_site * C]."""
    B, L, C = zbody.shape
    row, ch = sitepool_index(L, C, S, zbody.device)
    t = zbody.double()[:, row, ch]                           # [B][S][n_site * C]
    return t.sum(1) / S, t.abs().sum(1) / S


def sitepool_bwd(dpooled, L, C, S):
    """dz body [B][L][C]: every z element feeds exactly one output, dz = dpooled[that output] / S."""
    B = dpooled.shape[0]
    row, ch = sitepool_index(L, C, S, dpooled.device)
    dz = torch.zeros(B, L, C, dtype=F64, device=dpooled.device)
    cnt = torch.zeros(L, C, dtype=torch.int64, device=dpooled.device)
    d = dpooled.double().reshape(B, -1)
    for s in range(S):
        dz[:, row[s], ch[s]] += d / S
        cnt[row[s], ch[s]] += 1
    assert bool((cnt == 1).all()), "the site-pooling index map is a bijection"
    return dz, dz.abs()
