"""dl_attn_probs (attn_probs.hip: attn_lse_kernel + attn_probs_kernel) element-wise against the fp64 reference of
tests/attn_ref.py: per-head maps, head means, paired segments, key multiplicities unexpanded and expanded.

Buffers as in tests/test_attention_paths_gpu.py: inputs sit in NaN-filled strided stores (a stray read poisons the result),
the output sits in a NaN-filled store with a guard band and a row pitch out_ld > the column count — every addressed element
must be overwritten, every other element bitwise unchanged.  Every case runs with the LSE of ops.attn_fwd and with lse=None
(the statistics kernel), each twice: the two runs must agree bitwise.

Rounding model (that file's: u_f = 2^-24, MARGIN = 2; lam and mag_lse from attn_ref).  P = exp(s - lse): the logit error
(hd + 2) u_f lam_qk and the LSE's logit error (hd + 2) u_f mag_lse_q are each relative in P; the sum l, the log and the exp2
add (Lk_full + 8) u_f; results below 2^-126 may be flushed by v_exp_f32 (floor 2^-120):
    |got - ref| <= MARGIN ref ((hd + 2) u_f (lam_qk + mag_lse_q) + (Lk_full + 8) u_f) + 2^-120
A head mean is bounded by the mean over heads of the per-head bounds plus u_f ref (the fp32 sum over heads).  A row of a full
or expanded map sums to 1 within (Lk_full + 8) u_f plus the row's summed bounds.

DL_ATTN_BOUND_LOG=<file>: every check appends one JSON line (case, output, worst |err| / bound).
"""
import collections
import json
import math
import os

import pytest
import torch

from tests.attn_ref import reference_fwd
# The NaN-filled stores, the operand layouts and the data recipes are that file's, so that both files test the same buffers:
# _data reads only P, H, Lq, Lk, hd and data of a case, which the Case below carries under the same names.
from tests.test_attention_paths_gpu import Store, _data, _layout

pytestmark = pytest.mark.gpu
U_F, MARGIN, LAM, FLOOR = 2.0 ** -24, 2.0, 96.0, 2.0 ** -120
BF, F32 = torch.bfloat16, torch.float32

# vec: out_ld a multiple of 4 (16-byte stores; the store is 16-byte aligned) or not (4-byte stores throughout)
Case = collections.namedtuple("Case", "name dt hd P H S shift Lq Lk mean tail expand vec layout data")
CASES = [
    Case("lq1_lk1", BF, 64, 2, 2, 1, 0, 1, 1, False, None, False, True, "pitch", "randn"),
    Case("lq1_lk17_scalar_stores", BF, 64, 2, 2, 1, 0, 1, 17, False, None, False, False, "strided", "randn"),
    Case("paired_p3_head_mean", BF, 64, 3, 4, 2, 1, 65, 63, True, None, False, True, "fused", "randn"),
    Case("paired_key_crosses_tile_big", BF, 64, 2, 4, 2, 1, 64, 65, False, None, False, True, "pitch", "big"),
    Case("dominant_underflow", BF, 64, 2, 1, 1, 0, 17, 300, False, None, False, False, "pitch", "dominant"),
    Case("equal_uniform_rows", BF, 64, 2, 1, 1, 0, 17, 257, False, None, False, True, "strided", "equal"),
    Case("pgca_tail_expanded_512", BF, 128, 3, 1, 1, 0, 100, 136, False, (8, 48.0), True, True, "fused", "randn"),
    Case("pgca_tail_unexpanded_w2.5", BF, 128, 3, 1, 1, 0, 100, 136, False, (8, 2.5), False, True, "fused", "randn"),
    Case("tail_mid_tile_expanded_head_mean", BF, 64, 2, 2, 1, 0, 63, 100, True, (37, 3.0), True, False, "strided", "randn"),
    Case("tail_one_row_on_tile_edge", BF, 64, 2, 2, 1, 0, 1, 65, False, (1, 7.0), True, True, "pitch", "randn"),
    Case("tail_every_key", BF, 128, 2, 2, 1, 0, 33, 63, False, (63, 2.0), True, True, "pitch", "randn"),
    Case("f32_paired_head_mean", F32, 64, 3, 2, 2, 1, 17, 65, True, None, False, False, "fused", "randn"),
    Case("f32_hd128_tail_expanded", F32, 128, 2, 1, 1, 0, 129, 63, False, (8, 3.0), True, True, "strided", "randn"),
    # several workgroups per CU at once: a key tile whose LDS-DMA is read before it has landed shows only under load
    Case("pgca_many_workgroups", BF, 128, 256, 1, 1, 0, 256, 136, False, (8, 47.0), True, True, "fused", "randn"),
]


def _log(case, what, ratio):
    path = os.environ.get("DL_ATTN_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "output": what, "ratio": ratio}) + "\n")


def _expected(c, ref):
    """fp64 map and per-element bound in the layout the call writes: [S][P][H or 1][Lq][cols]."""
    hd, Lk = c.hd, c.Lk
    t, w = (int(c.tail[0]), float(c.tail[1])) if c.tail else (0, 1.0)
    lead = Lk - t
    lk_full = int(math.ceil(lead + t * w))
    pm, lam = torch.stack(ref["Pm"]), torch.stack(ref["lam"])                       # [S][P][H][Lq][Lk]
    rel = (hd + 2) * U_F * (lam + ref["mag_lse"].unsqueeze(-1)) + (lk_full + 8) * U_F
    if c.expand and t:
        copies = int(w)
        assert copies == w
        reps = (1, 1, 1, 1, copies)                                                  # column lead + i t + j <- tail key j
        pm = torch.cat([pm[..., :lead], (pm[..., lead:] / w).repeat(reps)], -1)
        rel = torch.cat([rel[..., :lead], rel[..., lead:].repeat(reps)], -1)
    bound = MARGIN * pm * rel + FLOOR
    if c.mean:
        pm = pm.mean(2, keepdim=True)
        bound = bound.mean(2, keepdim=True) + U_F * pm
    return pm, bound, lk_full


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_probability_map_against_fp64(c):
    from druglamp_amd import ops
    dt, P, H, S, Lq, Lk, hd = c.dt, c.P, c.H, c.S, c.Lq, c.Lk, c.hd
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(sum(map(ord, c.name)))
    layout, sizes, o_ss = _layout(c.layout, P, H, S, Lq, Lk, hd)
    stores = {name: Store(n, dt) for name, n in sizes.items() if name in {layout[op][0] for op in ("q", "k", "v", "o")}}

    def region(op, seg=0):
        sname, st, off = layout[op]
        return stores[sname].region(st, P, H, Lq if op in ("q", "o") else Lk, hd, off + seg * (o_ss if op == "o" else 0))

    def base(op):
        sname, st, off = layout[op]
        return stores[sname].base[off:], st

    q, k, v = _data(c, g, scale)
    region("q").copy_(q)
    region("k").copy_(k)
    region("v").copy_(v)
    for s in range(S):
        region("o", s)
    (qb, qs), (kb, ks), (vb, vs), (ob, os_) = (base(x) for x in ("q", "k", "v", "o"))
    common = dict(n_problems=P, n_heads=H, n_segments=S, partner_shift=c.shift, Lq=Lq, Lk=Lk, head_dim=hd, scale=scale,
                  q_strides=qs, k_strides=ks, key_tail=c.tail)
    ref = reference_fwd(qb, kb, vb, v_strides=vs, **common)
    assert float(max(l.max() for l in ref["lam"])) <= LAM, "%s: logits beyond the range the bounds assume" % c.name
    want, bound, lk_full = _expected(c, ref)
    cols = want.shape[-1]
    assert cols == (Lk - int(c.tail[0]) + int(c.tail[0]) * int(c.tail[1]) if (c.tail and c.expand) else Lk)
    lse_fwd = ops.attn_fwd(qb, kb, vb, out=ob, o_strides=os_, o_ss=o_ss, v_strides=vs, **common)

    out_ld = cols + 4 + (-cols) % 4 if c.vec else cols + (3 if (cols + 3) % 4 else 5)
    assert (out_ld % 4 == 0) == c.vec and out_ld > cols
    HO = 1 if c.mean else H
    out = Store(S * P * HO * Lq * out_ld, torch.float32)
    view = out.region((HO * Lq * out_ld, Lq * out_ld, out_ld), S * P, HO, Lq, cols).view(S, P, HO, Lq, cols)
    blank = torch.full_like(out.t, float("nan")).view(torch.int32)
    runs = {}
    for mode in ("lse_of_attn_fwd", "lse_none"):
        for rep in range(2):
            out.t.fill_(float("nan"))
            ops.attn_probs(qb, kb, lse=lse_fwd if mode == "lse_of_attn_fwd" else None, head_mean=c.mean, expand_tail=c.expand,
                           out=out.base, out_ld=out_ld, **common)
            bits = out.bits()
            assert torch.equal(bits[~out.mask], blank[~out.mask]), "%s/%s: a store outside the addressed columns" % (c.name, mode)
            if rep:
                assert torch.equal(bits, runs[mode]), "%s/%s: not bitwise repeatable" % (c.name, mode)
            runs[mode] = bits
        got = view.double()
        assert torch.isfinite(got).all(), "%s/%s: addressed elements left unwritten or non-finite" % (c.name, mode)
        ratio = float(((got - want).abs() / bound).max())
        print("%s/%s: worst |err| / bound = %.4g" % (c.name, mode, ratio))
        _log(c.name, mode, ratio)
        assert ratio <= 1.0, "%s/%s: exceeds its rounding bound by x%.3g" % (c.name, mode, ratio)
        if c.tail is None or c.expand:                  # a full or expanded map: rows sum to 1
            dev = (got.sum(-1) - 1.0).abs()
            lim = (lk_full + 8) * U_F + bound.sum(-1)
            rs = float((dev / lim).max())
            print("%s/%s: worst |row sum - 1| / limit = %.4g" % (c.name, mode, rs))
            _log(c.name, mode + " row sums", rs)
            assert rs <= 1.0, "%s/%s: a row sums to 1 +- %.3g (allowed x%.3g)" % (c.name, mode, float(dev.max()), rs)
