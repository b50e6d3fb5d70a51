"""Every launch form of dl_attn_fwd / dl_attn_bwd (attention.hip: launch_fwd / launch_bwd) element-wise against the fp64
reference of tests/attn_ref.py, with one bound per dtype and output taken from the rounding model below.

Each case of CASES names the kernel forms its shape, dtype, head dim, algo and key multiplicities select.  Every case runs the
forward and the backward with all outputs checked element by element (O, LSE, raw logits where asked for, dQ, dK, dV), in
buffers whose every element outside the addressed rows and columns is NaN beforehand: inputs (a stray read poisons the
result) and outputs (an addressed element must be overwritten, an element outside must be bitwise unchanged).  The
backward runs twice and must be bitwise repeatable.

DL_ATTN_BOUND_LOG=<file>: every check appends one JSON line (case, output, dtype, worst |err| / bound).
"""
import collections
import json
import math
import os

import pytest
import torch

from tests.attn_ref import reference_bwd, reference_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AUTO, STREAM, TWO_PASS, ONE_PASS = 0, 1, 2, 3

# ---- rounding model ------------------------------------------------------------------------------------------------------
# u_b = 2^-8 (bf16 round to nearest: 8 significant bits), u_f = 2^-24 (fp32).  Inputs are exact in the fp64 reference (it
# reads the kernel's own bf16 / fp32 operands), so every error is the kernels' rounding.  The table's cases keep the
# absolute logits lam = scale sum_d |q_d||k_d| + log w at or below LAM (asserted per case), head_dim <= HD and every summed
# length (keys, or query rows of both segments) at or below LEN.
#   logits S = Q K^T: bf16 products are exact in fp32, fp32 products round; fp32 accumulation over hd terms ->
#       |dS| <= (HD + 2) u_f lam <= E_S, which is also the relative error of every exp(S - m).
#   LSE = m scale + log(l): the logit error, l summed in fp32 over <= LEN terms each <= 1 (relative LEN u_f), log and the
#       final add (a few u_f of |LSE|) -> |dLSE| <= (HD + 3) u_f mag_lse + (LEN + 4) u_f (the only absolute floor).
#   raw logits: the logit error alone -> (HD + 2) u_f mag_raw.
#   O: P relative error E_S + E_LSE (online rescaling, normalisation), P rounded to bf16 before the PV product (u_b, bf16
#       only), fp32 accumulation over <= LEN keys, the bf16 store (u_b): |dO| <= tau_O sum_k P_k |V_kd| = tau_O mag_O.
#   dV = P^T dO, dK / dQ = scale dS^T Q / dS K with dS = P (dP - Delta): P recomputed from the stored LSE (relative error
#       E_S + E_LSE), dP and Delta in fp32 (relative LEN u_f of |dP| + |Delta| for dO not cancelling below 2^-8 of its
#       absolute sums), P or dS rounded to bf16 before the last product (u_b), fp32 accumulation (LEN u_f), bf16 store (u_b).
# tau = MARGIN x the first-order sum above: the margin covers the second-order terms the sum leaves out, and a measured
# worst |err| / bound at or below 1 / MARGIN says the kernels stay inside the first-order model itself.
# Scale bias: the bf16 roundings are round-to-nearest, i.e. zero-mean; only the fp32-level terms (E_S + E_LSE) can move a
# whole output coherently.  A least-squares scale s = sum (got - ref) ref / sum ref^2 must stay within those plus six
# standard deviations of what zero-mean errors of the bounded size give (each at most uniform over +-bound: variance
# bound^2 / 3) — the per-element bound alone cannot see a systematic error below one bf16 rounding.
U_B, U_F = 2.0 ** -8, 2.0 ** -24
LAM, HD, LEN, MARGIN = 96.0, 128, 2048, 2.0
E_S = (HD + 2) * U_F * LAM
E_LSE = E_S + (LEN + 4) * U_F
TAU = {
    torch.bfloat16: {"O": MARGIN * (2 * U_B + E_S + E_LSE + LEN * U_F), "d": MARGIN * (2 * U_B + E_S + E_LSE + 2 * LEN * U_F)},
    torch.float32: {"O": MARGIN * (E_S + E_LSE + (LEN + 2) * U_F), "d": MARGIN * (E_S + E_LSE + (2 * LEN + 4) * U_F)},
}
TAU_LSE, LSE_FLOOR, TAU_RAW = MARGIN * (HD + 3) * U_F, MARGIN * (LEN + 4) * U_F, MARGIN * (HD + 2) * U_F
BIAS = E_S + E_LSE

Case = collections.namedtuple("Case", "name forms dt hd P H S shift Lq Lk fwd bwd raw tail layout data")
BF, F32 = torch.bfloat16, torch.float32
R64, F1, F128, FG, FG128 = ("fwd_res<bf16,64,2,4>", "fwd<bf16,64,1,64,4>", "fwd<bf16,64,2,128>", "fwd<bf16,64,2>",
                            "fwd<bf16,128,2>")
B1, B2, B3, B4, B5 = ("bwd_fused<bf16,64>", "bwd_dq/dkv<bf16,64,2,true>", "bwd_dq/dkv<bf16,64,2,false>",
                      "bwd_dq/dkv_ring<bf16,128,2,true>", "bwd_dq/dkv_ring<bf16,128,2,false>")
CASES = [
    # K/V-resident forward, LDS-resident backward pair (AUTO with a small grid, TWO_PASS, ONE_PASS on an ineligible shape)
    Case("res_raw_lq1", (R64, B2), BF, 64, 2, 2, 1, 0, 1, 17, AUTO, AUTO, True, None, "pitch", "randn"),
    Case("res_lq1_lk1", (R64, B2), BF, 64, 3, 1, 1, 0, 1, 1, AUTO, AUTO, True, None, "strided", "randn"),
    Case("res_lk1_lq65", (R64, B2), BF, 64, 2, 2, 1, 0, 65, 1, AUTO, TWO_PASS, False, None, "fused", "randn"),
    Case("res_paired_p3_shift1_onepass_falls_back", (R64, B2), BF, 64, 3, 2, 2, 1, 65, 63, AUTO, ONE_PASS, False, None,
         "fused", "randn"),
    Case("res_paired_two_pass", (R64, B2), BF, 64, 4, 2, 2, 2, 256, 256, AUTO, TWO_PASS, True, None, "pitch", "randn"),
    Case("res_big_logits", (R64, B2), BF, 64, 2, 2, 1, 0, 129, 255, AUTO, AUTO, True, None, "strided", "big"),
    Case("res_dominant_key", (R64, B2), BF, 64, 2, 2, 1, 0, 64, 200, AUTO, AUTO, False, None, "pitch", "dominant"),
    Case("res_equal_logits", (R64, B2), BF, 64, 2, 2, 2, 1, 63, 64, AUTO, TWO_PASS, False, None, "fused", "equal"),
    # one-pass backward: forced (one segment, paired with 2 shift = P, Lq > 256) and chosen by AUTO (H * (P or shift) >= 256)
    Case("onepass_single_forced", (R64, B1), BF, 64, 3, 2, 1, 0, 17, 129, AUTO, ONE_PASS, True, None, "pitch", "randn"),
    Case("onepass_paired_forced_lq300", (R64, B1), BF, 64, 4, 1, 2, 2, 300, 256, AUTO, ONE_PASS, False, None, "strided",
         "randn"),
    Case("onepass_paired_big_logits", (R64, B1), BF, 64, 2, 2, 2, 1, 64, 65, AUTO, ONE_PASS, False, None, "fused", "big"),
    Case("auto_onepass_single", (R64, B1), BF, 64, 64, 4, 1, 0, 100, 256, AUTO, AUTO, False, None, "fused", "randn"),
    Case("auto_onepass_paired", (R64, B1), BF, 64, 128, 4, 2, 64, 64, 64, AUTO, AUTO, False, None, "fused", "randn"),
    # streaming forward with one 16-row query tile per wave (Lq <= 64, no raw logits)
    Case("small_q_stream", (F1, B3), BF, 64, 2, 3, 1, 0, 64, 129, STREAM, STREAM, False, None, "pitch", "randn"),
    Case("small_q_long_keys_paired", (F1, B3), BF, 64, 2, 2, 2, 1, 17, 257, AUTO, AUTO, False, None, "fused", "randn"),
    Case("small_q_tail_mid_tile", (F1, B3), BF, 64, 3, 2, 1, 0, 63, 100, AUTO, AUTO, False, (37, 3.0), "strided",
         "randn"),
    Case("small_q_tail_one_row_lq1", (F1, B3), BF, 64, 2, 2, 1, 0, 1, 65, AUTO, AUTO, False, (1, 2.5), "pitch", "randn"),
    Case("small_q_dominant_long", (F1, B3), BF, 64, 2, 1, 1, 0, 17, 300, AUTO, AUTO, False, None, "pitch", "dominant"),
    # 128-key tiles for long key sequences
    Case("long_keys_1024", (F128, B3), BF, 64, 2, 2, 1, 0, 129, 1024, AUTO, AUTO, False, None, "fused", "randn"),
    Case("long_keys_1025_tail1", (F128, B3), BF, 64, 2, 1, 1, 0, 65, 1025, AUTO, AUTO, False, (1, 7.0), "pitch", "randn"),
    Case("long_keys_1023", (FG, B3), BF, 64, 2, 1, 1, 0, 257, 1023, AUTO, AUTO, False, None, "strided", "big"),
    # the generic streaming forward at head_dim 64: raw logits with long or tailed keys, STREAM, Lq > 256
    Case("generic_raw_long", (FG, B3), BF, 64, 2, 2, 1, 0, 129, 300, AUTO, AUTO, True, None, "pitch", "randn"),
    Case("generic_raw_tail_all_rows", (FG, B3), BF, 64, 2, 2, 1, 0, 80, 160, AUTO, AUTO, True, (160, 3.0), "fused",
         "randn"),
    Case("generic_raw_tail_w1", (FG, B3), BF, 64, 2, 1, 1, 0, 65, 64, AUTO, AUTO, True, (8, 1.0), "strided", "randn"),
    Case("generic_stream_lq255", (FG, B3), BF, 64, 3, 2, 2, 1, 255, 64, STREAM, STREAM, False, None, "pitch", "randn"),
    Case("generic_lq257_lk17", (R64, B3), BF, 64, 2, 2, 1, 0, 257, 17, AUTO, AUTO, False, None, "fused", "randn"),
    Case("generic_paired_p3_long", (FG, B3), BF, 64, 3, 2, 2, 1, 100, 300, AUTO, AUTO, False, None, "strided", "randn"),
    # head_dim 128 in bf16
    Case("hd128_raw_lq257", (FG128, B5), BF, 128, 2, 2, 1, 0, 257, 129, AUTO, AUTO, True, None, "pitch", "randn"),
    Case("hd128_paired_half", (FG128, B5), BF, 128, 4, 1, 2, 2, 40, 40, AUTO, AUTO, False, None, "fused", "randn"),
    Case("hd128_paired_p3_shift1", (FG128, B5), BF, 128, 3, 2, 2, 1, 1, 65, AUTO, AUTO, False, None, "strided", "big"),
    Case("hd128_tail_pgca", (FG128, B4), BF, 128, 3, 1, 1, 0, 100, 136, AUTO, AUTO, False, (8, 48.0), "fused", "randn"),
    Case("hd128_tail_all_rows_lq1", (FG128, B4), BF, 128, 2, 2, 1, 0, 1, 63, AUTO, AUTO, True, (63, 2.5), "pitch",
         "dominant"),
    Case("hd128_equal_logits", (FG128, B5), BF, 128, 2, 1, 1, 0, 64, 256, STREAM, STREAM, False, None, "strided", "equal"),
    # fp32 pipelines: the Delta launch + the generic dQ / dK-dV pair
    Case("f32_hd64_paired_p3", ("fwd<float,64,1>", "delta+bwd<float,64>"), F32, 64, 3, 2, 2, 1, 17, 65, AUTO, AUTO,
         False, None, "fused", "randn"),
    Case("f32_hd64_tail", ("fwd<float,64,1>", "delta+bwd<float,64>"), F32, 64, 2, 2, 1, 0, 64, 129, AUTO, AUTO, True,
         (1, 7.0), "strided", "big"),
    Case("f32_hd128_raw", ("fwd<float,128,1>", "delta+bwd<float,128>"), F32, 128, 3, 1, 1, 0, 129, 63, AUTO, AUTO, True,
         None, "pitch", "dominant"),
    Case("f32_hd128_tail_all_rows", ("fwd<float,128,1>", "delta+bwd<float,128>"), F32, 128, 2, 1, 1, 0, 65, 256, AUTO,
         AUTO, False, (256, 2.5), "fused", "randn"),
]


class Store:
    """A flat NaN-filled buffer with a guard band on both sides; `region` hands out as_strided views of the addressed
    elements and records them in `mask`."""
    G = 256

    def __init__(self, n, dt):
        self.t = torch.full((n + 2 * self.G,), float("nan"), device=DEV, dtype=dt)
        self.mask = torch.zeros(n + 2 * self.G, dtype=torch.bool, device=DEV)
        self.base = self.t[self.G:]

    def region(self, strides, P, H, L, hd, off=0):
        ps, hs, rs = strides
        shape, st = (P, H, L, hd), (ps, hs, rs, 1)
        torch.as_strided(self.mask, shape, st, self.G + off).fill_(True)
        return torch.as_strided(self.t, shape, st, self.G + off)

    def bits(self):
        return self.t.view(torch.int16 if self.t.dtype == torch.bfloat16 else torch.int32).clone()


def _layout(kind, P, H, S, Lq, Lk, hd):
    """{operand: (store name, strides, offset)}, store sizes, o_ss.  Strides are multiples of 16 bytes in both dtypes."""
    d = H * hd
    if kind == "fused":                          # the model's [P][L][3d] projection output, [P][Lq][S d] with o_ss = d
        L = max(Lq, Lk)
        st = (L * 3 * d, hd, 3 * d)
        ost = (Lq * S * d, hd, S * d)
        ops = {"q": ("qkv", st, 0), "k": ("qkv", st, d), "v": ("qkv", st, 2 * d), "o": ("o", ost, 0), "do": ("do", ost, 0),
               "dq": ("dqkv", st, 0), "dk": ("dqkv", st, d), "dv": ("dqkv", st, 2 * d)}
        return ops, {"qkv": P * L * 3 * d, "dqkv": P * L * 3 * d, "o": P * Lq * S * d, "do": P * Lq * S * d}, d
    if kind == "pitch":                          # separate buffers, rows wider than H*hd, segments a whole buffer apart
        pq, pk, po = d + 16, d + 24, d + 40
        qs, ks, os_ = (Lq * pq, hd, pq), (Lk * pk, hd, pk), (Lq * po, hd, po)
        ops = {"q": ("q", qs, 0), "k": ("k", ks, 0), "v": ("v", ks, 0), "o": ("o", os_, 0), "do": ("do", os_, 0),
               "dq": ("dq", qs, 0), "dk": ("dk", ks, 0), "dv": ("dv", ks, 0)}
        n = {"q": P * Lq * pq, "k": P * Lk * pk, "v": P * Lk * pk, "o": S * P * Lq * po, "do": S * P * Lq * po}
        n.update(dq=n["q"], dk=n["k"], dv=n["v"])
        return ops, n, P * Lq * po
    # "strided": head-major Q / K / O ([H][P][L][hd + 8]: problem stride < head stride), V row-interleaved ([Lk][P][H][hd])
    r = hd + 8
    qs, ks, vs, os_ = (Lq * r, P * Lq * r, r), (Lk * r, P * Lk * r, r), (d, hd, P * d), (Lq * r, P * Lq * r, r)
    ops = {"q": ("q", qs, 0), "k": ("k", ks, 0), "v": ("v", vs, 0), "o": ("o", os_, 0), "do": ("do", os_, 0),
           "dq": ("dq", qs, 0), "dk": ("dk", ks, 0), "dv": ("dv", vs, 0)}
    n = {"q": H * P * Lq * r, "k": H * P * Lk * r, "v": Lk * P * d, "o": S * H * P * Lq * r, "do": S * H * P * Lq * r}
    n.update(dq=n["q"], dk=n["k"], dv=n["v"])
    return ops, n, H * P * Lq * r


def _data(c, g, scale):
    """q [P][H][Lq][hd], k / v [P][H][Lk][hd] (float32, to be rounded to the case's dtype)."""
    P, H, Lq, Lk, hd = c.P, c.H, c.Lq, c.Lk, c.hd
    if c.data == "big":                          # logits of tens: most exp terms underflow
        sig = (45.0 / (scale * hd * 0.64)) ** 0.5      # mean |logit| sum 45, std ~7: the largest stay below LAM
        q = torch.randn(P, H, Lq, hd, generator=g) * sig
        k = torch.randn(P, H, Lk, hd, generator=g) * sig
    else:
        q = torch.randn(P, H, Lq, hd, generator=g) * 0.7
        k = torch.randn(P, H, Lk, hd, generator=g) * 0.7
    if c.data == "dominant":                     # every query row has one key with a logit of 40 (the rest are small)
        j = torch.randint(0, Lk, (P, H, Lq), generator=g)
        kj = torch.gather(k, 2, j.unsqueeze(-1).expand(P, H, Lq, hd))
        q = kj * (40.0 / scale) / (kj * kj).sum(-1, keepdim=True) + 0.05 * torch.randn(P, H, Lq, hd, generator=g)
    if c.data == "equal":                        # all keys of a (problem, head) identical: every row's logits are equal
        k = k[:, :, :1].expand(P, H, Lk, hd).contiguous()
    v = torch.randn(P, H, Lk, hd, generator=g)
    return q, k, v


def _log(case, what, dt, ratio):
    path = os.environ.get("DL_ATTN_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "output": what, "dtype": str(dt).split(".")[1], "ratio": ratio}) + "\n")


def _check(case, what, dt, got, ref, bound, bias=None):
    got = got.double()
    assert torch.isfinite(got).all(), "%s: %s has non-finite addressed elements" % (case, what)
    err = got - ref
    ratio = float((err.abs() / bound).max())
    _log(case, what, dt, ratio)
    assert ratio <= 1.0, "%s: %s exceeds its rounding bound by x%.3g" % (case, what, ratio)
    den = float((ref * ref).sum())
    if bias is not None and den > 0:
        s = float((err * ref).sum()) / den
        lim = bias + 6.0 * float(((bound * ref) ** 2).sum().sqrt()) / den / math.sqrt(3.0)
        _log(case, what + " bias", dt, abs(s) / lim)
        assert abs(s) <= lim, "%s: %s carries a scale error of %.3g (allowed %.3g)" % (case, what, s, lim)


def _untouched(case, store, before):
    outside = ~store.mask
    assert torch.equal(store.bits()[outside], before[outside]), "%s: a store outside the addressed rows" % case


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_attention_form_against_fp64(c):
    from druglamp_amd import ops
    dt, P, H, S, Lq, Lk, hd = c.dt, c.P, c.H, c.S, c.Lq, c.Lk, c.hd
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(sum(map(ord, c.name)))
    layout, sizes, o_ss = _layout(c.layout, P, H, S, Lq, Lk, hd)
    stores = {name: Store(n, dt) for name, n in sizes.items()}

    def region(op, seg=0):
        sname, st, off = layout[op]
        return stores[sname].region(st, P, H, Lq if op in ("q", "o", "do", "dq") else Lk, hd, off + seg * (o_ss if op in ("o", "do") else 0))

    def base(op):
        sname, st, off = layout[op]
        return stores[sname].base[off:], st

    q, k, v = _data(c, g, scale)
    region("q").copy_(q)
    region("k").copy_(k)
    region("v").copy_(v)
    for s in range(S):
        region("do", s).copy_(torch.randn(P, H, Lq, hd, generator=g) * 0.5)
    for s in range(S):
        region("o", s)                                   # addressed: marks the mask (values stay NaN until the kernel writes)
    for op in ("dq", "dk", "dv"):
        region(op)
    (qb, qs), (kb, ks), (vb, vs), (ob, os_), (dob, dos) = (base(x) for x in ("q", "k", "v", "o", "do"))
    common = dict(n_problems=P, n_heads=H, n_segments=S, partner_shift=c.shift, Lq=Lq, Lk=Lk, head_dim=hd, scale=scale,
                  q_strides=qs, k_strides=ks, v_strides=vs, key_tail=c.tail)

    # ---- forward ----
    raw = Store(P * H * Lq * Lk, torch.float32) if c.raw else None
    raw_t = raw.region((H * Lq * Lk, Lq * Lk, Lk), P, H, Lq, Lk) if c.raw else None
    o_before = stores[layout["o"][0]].bits()
    lse = ops.attn_fwd(qb, kb, vb, out=ob, o_strides=os_, o_ss=o_ss, raw_logits=raw.base if c.raw else None,
                       algo=c.fwd, **common)
    ref = reference_fwd(qb, kb, vb, **common)
    assert float(max(l.max() for l in ref["lam"])) <= LAM, "%s: logits beyond the range the bounds assume" % c.name
    for s in range(S):
        _check(c.name, "O[seg%d]" % s, dt, region("o", s), ref["O"][s], TAU[dt]["O"] * ref["mag_O"][s] + 1e-300, BIAS)
    _check(c.name, "LSE", dt, lse, ref["LSE"], TAU_LSE * ref["mag_lse"] + LSE_FLOOR)
    if c.raw:
        _check(c.name, "raw", dt, raw_t, ref["raw"], TAU_RAW * ref["mag_raw"] + 1e-300)
        _untouched(c.name, raw, torch.full_like(raw.t, float("nan")).view(torch.int32))
    _untouched(c.name, stores[layout["o"][0]], o_before)

    # ---- backward (twice: bitwise repeatable) ----
    outs = []
    for rep in range(2):
        for op in ("dq", "dk", "dv"):
            stores[layout[op][0]].t.fill_(float("nan"))
        before = {layout[op][0]: stores[layout[op][0]].bits() for op in ("dq", "dk", "dv")}
        (dqb, dqs), (dkb, dks), (dvb, dvs) = (base(x) for x in ("dq", "dk", "dv"))
        ops.attn_bwd(qb, kb, vb, ob, dob, lse, o_strides=os_, o_ss=o_ss, do_strides=dos, do_ss=o_ss, dq=dqb, dq_strides=dqs,
                     dk=dkb, dk_strides=dks, dv=dvb, dv_strides=dvs, algo=c.bwd, **common)
        outs.append({name: stores[name].bits() for name in before})
        for name, b in before.items():
            _untouched(c.name, stores[name], b)
    for name in outs[0]:
        assert torch.equal(outs[0][name], outs[1][name]), "%s: backward not bitwise repeatable (%s)" % (c.name, name)
    bref = reference_bwd(ref, dob, do_strides=dos, do_ss=o_ss, scale=scale, o=ob, o_strides=os_, o_ss=o_ss)
    for op, name in (("dq", "dQ"), ("dk", "dK"), ("dv", "dV")):
        _check(c.name, name, dt, region(op), bref[name], TAU[dt]["d"] * bref["mag_" + name] + 1e-300, BIAS)


def test_key_multiplicities_with_two_segments_are_rejected():
    from druglamp_amd import ops
    P, H, L, hd = 2, 1, 16, 64
    x = torch.zeros(P * L, H * hd, device=DEV, dtype=torch.bfloat16)
    st = (L * H * hd, hd, H * hd)
    o = torch.zeros(2, P * L, H * hd, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="one segment only"):
        ops.attn_fwd(x, x, x, n_problems=P, n_heads=H, n_segments=2, partner_shift=1, Lq=L, Lk=L, head_dim=hd, scale=0.125,
                     q_strides=st, k_strides=st, v_strides=st, out=o, o_strides=st, o_ss=P * L * H * hd, key_tail=(4, 2.0))
