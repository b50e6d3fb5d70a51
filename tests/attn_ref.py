"""float64 reference of dl_attn_fwd / dl_attn_bwd (include/druglamp_hip.h), described the way the C ABI describes a problem,
plus the per-element magnitudes the rounding bounds of tests/test_attention_paths_gpu.py are stated against.

Everything is gathered out of the strided buffers with torch.as_strided (element strides of (problem, head, row); the head
dim is contiguous), so the reference reads exactly the elements the ABI says the kernels read.  Shapes of the results:
O [S][P][H][Lq][hd], LSE [S][P][H][Lq], raw [P][H][Lq][Lk] (segment 0), dQ [P][H][Lq][hd], dK / dV [P][H][Lk][hd].

Semantics (header): segment 0 of problem p queries with Q(p), segment 1 with Q(partner(p)), partner(p) = (p + shift) % P.
Key multiplicities (rows, w): the last `rows` keys each stand for w identical keys, i.e. log(w) is added to their logits;
the raw logits of a tail key therefore carry the + log(w) too (softmax over a raw row = the weights the output uses;
documented at ops.attn_fwd).
dQ(p) is the sum of its segment-0 share (attention p) and its segment-1 share (attention p - shift); dK / dV of an attention
sum over its segments, and those of a tail key are the sums over the keys it stands for.  The backward's Delta is
rowsum(dO * O) over the O it is GIVEN (the ABI takes O as an input): pass the kernel's O as `o` to reference_bwd.
"""
import math

import torch


def gather(buf, strides, P, H, L, hd, offset=0):
    """[P][H][L][hd] float64 view-copy of the rows the ABI addresses: buf + offset + p*ps + h*hs + r*rs + (0..hd-1)."""
    ps, hs, rs = strides
    return torch.as_strided(buf, (P, H, L, hd), (ps, hs, rs, 1), buf.storage_offset() + offset).double()


def _logw(Lk, key_tail, dev):
    lw = torch.zeros(Lk, dtype=torch.float64, device=dev)
    if key_tail is not None and key_tail[0] > 0:
        lw[Lk - int(key_tail[0]):] = math.log(float(key_tail[1]))
    return lw


def reference_fwd(q, k, v, *, n_problems, n_heads, n_segments, partner_shift, Lq, Lk, head_dim, scale,
                  q_strides, k_strides, v_strides, key_tail=None):
    """fp64 forward.  Returns a dict: O, LSE, raw and their magnitudes mag_O = sum_k P_ik |V_kd|, mag_lse = max_k lam_ik and
    mag_raw = lam, lam_ik = scale sum_d |q_id||k_kd| + log w_k (the logit with absolute values), plus what the backward
    reference needs (P per segment, the gathered operands)."""
    P, H, S, hd = n_problems, n_heads, n_segments, head_dim
    Q = gather(q, q_strides, P, H, Lq, hd)
    K = gather(k, k_strides, P, H, Lk, hd)
    V = gather(v, v_strides, P, H, Lk, hd)
    lw = _logw(Lk, key_tail, Q.device)
    perm = (torch.arange(P, device=Q.device) + partner_shift) % P     # segment 1 of problem p uses Q(partner(p))
    Qs = [Q] + ([Q[perm]] if S == 2 else [])
    out = {"Q": Q, "K": K, "V": V, "perm": perm, "Qs": Qs, "Pm": [], "lam": []}
    O, LSE, mO, mL = [], [], [], []
    for Qx in Qs:
        s = scale * (Qx @ K.transpose(-1, -2)) + lw
        lam = scale * (Qx.abs() @ K.abs().transpose(-1, -2)) + lw
        lse = torch.logsumexp(s, -1)
        pm = torch.exp(s - lse.unsqueeze(-1))
        O.append(pm @ V)
        mO.append(pm @ V.abs())
        LSE.append(lse)
        mL.append(lam.amax(-1))
        out["Pm"].append(pm)
        out["lam"].append(lam)
        if len(O) == 1:
            out["raw"], out["mag_raw"] = s, lam
    out.update(O=torch.stack(O), LSE=torch.stack(LSE), mag_O=torch.stack(mO), mag_lse=torch.stack(mL))
    return out


def reference_bwd(fwd, do, *, do_strides, do_ss, scale, o=None, o_strides=None, o_ss=0):
    """fp64 backward of the attention `fwd` (reference_fwd's dict) for the output gradient dO (addressed like O).  o: the O
    the backward is given (Delta = rowsum(dO * O) over it); None = the reference's own O.  Returns dQ, dK, dV and
    mag_dQ = scale sum_j P_ij (|dP_ij| + |Delta_i|) |K_jd|, mag_dK = scale sum_i P_ij (|dP_ij| + |Delta_i|) |Q_id|,
    mag_dV = sum_i P_ij |dO_id| (both segments summed as the values are)."""
    Q, K, V, perm = fwd["Q"], fwd["K"], fwd["V"], fwd["perm"]
    P, H, Lq, hd = Q.shape
    dQ, mdQ = torch.zeros_like(Q), torch.zeros_like(Q)
    dK, mdK, dV, mdV = (torch.zeros_like(K) for _ in range(4))
    for seg, (Qx, pm) in enumerate(zip(fwd["Qs"], fwd["Pm"])):
        dO = gather(do, do_strides, P, H, Lq, hd, seg * do_ss)
        Og = fwd["O"][seg] if o is None else gather(o, o_strides, P, H, Lq, hd, seg * o_ss)
        dP = dO @ V.transpose(-1, -2)
        delta = (dO * Og).sum(-1, keepdim=True)
        dS = pm * (dP - delta)
        A = pm * (dP.abs() + delta.abs())
        gq, mq = scale * (dS @ K), scale * (A @ K.abs())
        if seg == 0:
            dQ += gq
            mdQ += mq
        else:                                          # attention a's segment 1 used Q(partner(a)): its share goes there
            dQ.index_add_(0, perm, gq)
            mdQ.index_add_(0, perm, mq)
        dK += scale * (dS.transpose(-1, -2) @ Qx)
        mdK += scale * (A.transpose(-1, -2) @ Qx.abs())
        dV += pm.transpose(-1, -2) @ dO
        mdV += pm.transpose(-1, -2) @ dO.abs()
    return {"dQ": dQ, "dK": dK, "dV": dV, "mag_dQ": mdQ, "mag_dK": mdK, "mag_dV": mdV}
