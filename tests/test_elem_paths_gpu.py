"""Every launch form of the elementwise kernels (elementwise.hip), the row-table kernels (compact.hip: dl_embed_rows,
dl_rows_gather, dl_rows_sum_strided) and the graph kernels (dl_norm_adjacency, graph.hip: dl_graph_aggregate) through the
C ABI, element-wise against the fp64 / integer references of tests/elem_ref.py:

    |got - ref| <= bound = MARGIN x (first-order rounding sum) x mag      for every addressed element of every output,

with the constants, the `check` and the `Guarded` buffers of tests/test_norm_paths_gpu.py (imported, not restated; MARGIN = 2,
u_f = 2^-24, u_b = 2^-8, u_st the output dtype's).  Pure data movers and casts are compared bit for bit: no tolerance.
Buffers: every operand sits in the middle of a larger NaN-filled buffer (integer tables: -7, which the contracts read as "no
row", ids: far beyond the vocabulary), every output in a NaN-filled buffer: an addressed element must be overwritten,
everything else (pitch padding, elements past n, the other items' parts of a shared weight image, the unused last column of
the padded embedding table is NaN and must reach no output) stays bitwise unchanged.  Every launch runs twice and must
repeat bitwise.  The checkers (check_*) take plain tensors on any device and the case data is built on the host:
tests/test_elem_reference_cpu.py checks the data conditions and the dispatch arithmetic of every case and runs the
checkers on planted errors without a GPU.

DL_ELEM_BOUND_LOG=<file>: every check appends one JSON line (case, form, output, dtype, worst |err| / bound; bit-exact
checks log 0); tools/elem_bound_margins.py reduces it to profiles/elem_bound_margins.txt.

Forms (host dispatch -> kernel instantiation): the FORMS table below; every case names the instantiation it selects and
tests/test_elem_reference_cpu.py asserts that table and case lists agree.

Rounding model (first order; the references read the kernels' own operands)
  fp32 sum of N terms: N u_f of the sum of the absolute terms (any order), plus the roundings of one term.
  fast exp (__expf = exp2(x log2 e)), as in the loss suite: relative (2 |x| + 2) u_f.
  gate = e_l / sum e: (2 d_l + 2) u_f [e_l, d = max - x] + sum_l g_l (2 d_l + 2) u_f + L u_f [the sum] + 4 u_f [x - max, 1 / sum,
      the product], relative to g.  out = v (g + res): (u_st + 2 u_f) |v| (g + res) + |v| e_gate.
  gate backward: dv = dout (g + res): (u_st + 2 u_f) |dv|.  dgate_l = sum_c dout v over hd terms: (hd + 1) u_f A_l, A_l = sum_c |dout v|;
      dot = sum_l g_l dgate_l: (L + 2) u_f Dabs + sum_l g_l e_dgate_l <= (L + hd + 3) u_f Dabs, Dabs = sum_l g_l A_l;
      dlogits = g (dgate - dot): the subtraction, the product and the store on top: (u_st + (L + hd + 5) u_f) g_l (A_l + Dabs).
  positional add + dropout: y = (x + pe) fl(1 / (1 - p)): (u_st + 2 u_f) |y| (the reference multiplies by the same fp32 scale);
      dropout apply: (u_st + u_f) |y|, i.e. one store rounding of x / (1 - p) up to the fp32 product; dropped elements are +0
      exactly and the mask equals the integer replica (elem_ref.keep_mask: the contract of common.cuh) exactly.  A p that
      rounds to thr16 == 0 (p < 2^-17) is no dropout: the output is the plain sum / a bit-exact copy, unscaled, in both
      kernels; test_gemm_leaves_a_thr16_zero_site_alone pins the same for the GEMM epilogues, whose backward is dl_dropout_apply.
  gelu'(x) = Phi + x phi through erff and the fast exp: absolute e_g = 8 u_f, the constant of the GEMM suite (the cancellation
      in 1 + erf is absolute, of the order u_f).  dl_gelu_bwd: (u_st + u_f) |dx| + |dy| e_g.
  dl_gate_dpre: acc = 8 fused multiply-adds: 9 u_f S, S = sum_h |dl||w2|; out = acc gelu': (u_st + u_f) |out| + 9 u_f S |gelu'| +
      |acc| e_g; bf16 takes gelu_grad_fast2, the rational fit of common.cuh: e_g = 8 u_f + 1.0e-4.  MEASURED, not derived: the
      fit's worst error in fp32 arithmetic on a dense grid over [-12, 12] is 1.013e-4 at |x| = 0.282
      (tests/test_elem_reference_cpu.py::test_gelu_grad_rational_fit, profiles/elem_bound_margins.txt); the comment in
      common.cuh used to claim 1.0e-4 and now states the measured figure.  The bound's term is DELIBERATELY kept at the old
      1.0e-4, 1.3 % below what was measured, so that it is not widened to fit the code: MARGIN has to cover the difference,
      and the recorded ratio shows that it does.
  dl_fill_pool: the fill bit is exact (the data keeps |row sum| >= 2^-10 sum |x| or the row entirely zero, so no summation
      order can change it); pooled: site_len terms, 1 / site_len rounded, the product: (u_st + (site_len + 2) u_f) mag.
  dl_rowmod_sum: nb terms (+ the old value): (nb + 2) u_f mag, fp32 output.
  dl_adamw_step (scalars: the fp32 values the ABI receives; bc1 = 1 - b1^t and bc2s = sqrt(1 - b2^t) come from the HOST's powf /
      sqrtf: 2 u_f for powf, amplified by b^t / (1 - b^t) through the subtraction: e_bc1 = (2 amp1 + 1) u_f, e_bc2s = (amp2 + 2) u_f):
      m' = b1 m + (1 - b1) g gscale: 4 u_f mag_m;  v' likewise (positive terms): 5 u_f v';  den = sqrt(v') / bc2s + eps (sqrtf and
      the division correctly rounded: hipcc's default): tau_den = (2.5 + 1 + 1 + 1) u_f + e_bc2s;  u = (lr / bc1) (m' / den):
      e_u = (lr / bc1) e_m' / den + |u| (tau_den + 3 u_f + e_bc1);  p' = p (1 - lr wd) - u: 4 u_f (|p| + |u|) + e_u.
      lowp == the stored p' rounded to nearest even, bit for bit.
  dl_norm_adjacency: degree sums of n terms (exact for a 0/1 adjacency), rsqrtf at 2 ulp (stated, not documented for this
      use; the recorded ratio shows what was needed): each degree 4 u_f + n u_f / 2, two products, the store:
      (u_st + (n + 10) u_f) |ahat| weighted, (u_st + 10 u_f) |ahat| for 0/1.
  dl_graph_aggregate: the GEMM suite's accumulation term, (n + 2) 2 u_f S, S = sum_j |a||f|, + u_st |out|; the any-size kernel
      (two roundings per term) stays inside the same term.  Virtual nodes are copied: bit-exact.
  dl_rows_sum_strided: (count + 1) u_f S + u_st |out|; count 0 is exactly zero.
  dl_cnn_sitepool_fwd: (u_st + (S + 2) u_f) mag; _bwd: one product and the store: (u_st + 2 u_f) |dz|; halo rows exactly zero.
  dl_cnn_sitepool_rows_fwd: the same sums on rows gathered through row_of.  _rows_bwd: a compact row sums the gradients of the
      `count` positions it stands for, then 1 / S: (count + 2) u_f mag + u_st |dz|; halo, context and bucket padding rows exactly zero.
"""
import collections
import json
import math
import os
import struct

import numpy as np
import pytest
import torch

from tests import elem_ref as er
from tests.test_norm_paths_gpu import BF, DEV, F32, MARGIN, U_B, U_F, Guarded, _lib, _ptr, check, u_st

pytestmark = pytest.mark.gpu

E_G = 8 * U_F                       # gelu' through erff / fast exp, absolute (the GEMM suite's constant)
E_G_FAST = 1.0e-4                   # gelu_grad_fast2: deliberately the fit's ORIGINAL claim, below the measured 1.013e-4 (see above)
DTN = {BF: "bf16", F32: "f32", torch.bool: "bool"}

# kernel instantiation -> the host dispatch condition that selects it
FORMS = collections.OrderedDict([
    ("gate_softmax_kernel<T> + gate_apply_kernel<T>", "dl_token_gate_fwd, always (T = the dtype)"),
    ("gate_bwd_rows_kernel<T>", "dl_token_gate_bwd, hd / 4 a power of two in 1..64"),
    ("gate_bwd_kernel<T>", "dl_token_gate_bwd, any other hd"),
    ("add_rowmod_dropout_kernel<T>", "dl_add_rowmod_dropout, always"),
    ("dropout_apply_kernel<T>", "dl_dropout_apply, always"),
    ("gelu_bwd_kernel<T>", "dl_gelu_bwd, always"),
    ("gate_dpre_kernel<T, 8>", "dl_gate_dpre, always; cpr = dd / 8 threads per row, rpb = 256 / cpr rows per pass"),
    ("fill_pool_kernel<T, TO>", "dl_fill_pool, the four (in, out) dtype pairs"),
    ("rowmod_sum_kernel<T>", "dl_rowmod_sum, always; the 16-way loop runs from nb = 13"),
    ("adamw_kernel<TL>", "dl_adamw_step: TL = bf16 with a bf16 image, float otherwise (fp32 image or none)"),
    ("cast_kernel<TS, TD>", "dl_cast, the four dtype pairs; n % 4 elements take the scalar tail"),
    ("norm_adj_kernel<TO>", "dl_norm_adjacency, (n (n + 1) + 2 n) 4 bytes <= 150 KiB (n <= 194); attribute call above 64 KiB (n >= 127)"),
    ("norm_adj_any_kernel<TO>", "dl_norm_adjacency, n >= 195"),
    ("graph_aggregate_kernel<T, 128>", "dl_graph_aggregate, n <= 128"),
    ("graph_aggregate_any_kernel<T, 128>", "dl_graph_aggregate, n > 128"),
    ("gather_pad_kernel<T>", "dl_gather_pad, always; grid (min(chunks / 256, 64), B)"),
    ("embed_pad_kernel<T>", "dl_embed_pad, always; grid (min(chunks / 256, 16), B)"),
    ("embed_rows_kernel<T>", "dl_embed_rows, always; min(chunks / 2048, 2048) gather workgroups"),
    ("rows_gather_kernel", "dl_rows_gather, always; min(chunks / 1024, 16384) workgroups"),
    ("interleave_streams_kernel", "dl_interleave_streams, always; min(chunks / 256, 8192) workgroups"),
    ("concat2_kernel", "dl_concat2, always; min(chunks / 256, 8192) workgroups"),
    ("rows_sum_wide_kernel<CPR>", "dl_rows_sum_strided, bf16, C in {64, 128, 256, 512}, x and out 16-byte aligned; CPR = C / 8; min(R / 4, 4096) workgroups"),
    ("rows_sum_kernel<T>", "dl_rows_sum_strided, otherwise"),
    ("cnn_sitepool_fwd_kernel<bf16>", "dl_cnn_sitepool_fwd, unless the transpose form applies"),
    ("cnn_sitepool_bwd_kernel<bf16>", "dl_cnn_sitepool_bwd, unless the transpose form applies"),
    ("transpose_view_kernel", "dl_cnn_sitepool_fwd / _bwd, site_len 1, L % 64 == 0, C % 64 == 0, 16-byte bases"),
    ("weight_prep_kernel<TD>", "dl_weight_prep, both image dtypes; items plain / transposed / strided"),
    ("cnn_sitepool_fwd_kernel<bf16> through row_of", "dl_cnn_sitepool_rows_fwd, always"),
    ("cnn_sitepool_rows_bwd_kernel<128, 256>", "dl_cnn_sitepool_rows_bwd, C == 128 and L / site_len == 256; 16 / 8 / 4 slices for B < 32 / < 128 / >= 128"),
    ("cnn_sitepool_rows_bwd_kernel<0, 0>", "dl_cnn_sitepool_rows_bwd, any other shape; the same slices"),
])


# ---- logging check -------------------------------------------------------------------------------------------------------------
def _elog(case, form, what, dt, ratio):
    path = os.environ.get("DL_ELEM_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "form": form, "output": what, "dtype": DTN.get(dt, str(dt)), "ratio": ratio}) + "\n")


def echeck(case, form, what, dt, got, ref, bound):
    """`check` of the norm suite, with the form in the log line."""
    g = got.double()
    if g.shape == ref.shape and g.numel() and bool(torch.isfinite(g).all()):
        _elog(case, form, what, dt, float(((g - ref).abs() / (bound + 1e-300)).max()))
    check(case, what, dt, got, ref, bound)


def _bits(t):
    t = t.contiguous()
    return t.to(torch.uint8) if t.dtype == torch.bool else t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def exact(case, form, what, got, ref):
    """Bit for bit (data movers, casts, masks, zero rows)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, "%s: %s has shape / dtype %s %s, reference %s %s" % (
        case, what, tuple(got.shape), got.dtype, tuple(ref.shape), ref.dtype)
    bad = _bits(got) != _bits(ref)
    assert not bool(bad.any()), "%s: %s differs from the reference in %d elements (first at flat index %d)" % (
        case, what, int(bad.sum()), int(bad.reshape(-1).nonzero()[0]))
    _elog(case, form, what, got.dtype, 0.0)


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
class Out:
    """An output inside a NaN-filled guarded buffer: `v` the addressed view; done(): nothing else changed."""

    def __init__(self, shape, dt, strides=None, off=0, n=None, dev=None):
        n = n if n is not None else int(math.prod(shape))
        self.g = Guarded(n + off, dt, dev)
        self.v = self.g.view(tuple(shape), strides, off)
        self.before = self.g.bits()

    def done(self, case):
        self.g.untouched(case, self.before)
        return self


def placed(values, dt=None, off=0, strides=None, n=None, dev=None):
    """A guarded copy of `values` (cast to dt), `off` elements behind an aligned address, optionally strided."""
    dt = dt or values.dtype
    shape = tuple(values.shape)
    n = n if n is not None else int(math.prod(shape))
    g = Guarded(n + off, dt, dev)
    v = g.view(shape, strides, off)
    v.copy_(values)
    return v


def table(values, fill=-7, dt=torch.int32, dev=None):
    """An integer table in the middle of a buffer of `fill` (out of range for every contract here)."""
    n = values.numel()
    t = torch.full((n + 128,), fill, dtype=dt, device=dev or DEV)
    v = t[64:64 + n].view(values.shape)
    v.copy_(values)
    return v


def same_bits(case, a, b):
    for x, y in zip(a, b):
        assert torch.equal(x.g.bits(), y.g.bits()), "%s: not bitwise repeatable" % case


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31))


# =================================================================================================================================
# token gate
# =================================================================================================================================
GateF = collections.namedtuple("GateF", "name form dt B L H hd res spread")
GATE_FWD = [GateF("gatef_%s_L%d_H%d_hd%d_res%d%s" % (DTN[dt], L, H, hd, res, "_spread80" if sp else ""),
                  "gate_softmax_kernel<T> + gate_apply_kernel<T>", dt, 3, L, H, hd, res, sp)
            for dt in (F32, BF)
            for (L, H, hd, res, sp) in ((1, 3, 4, 0, 0), (40, 8, 8, 1, 0), (64, 3, 12, 1, 0), (65, 8, 4, 0, 0), (200, 8, 16, 1, 0),
                                        (65, 3, 8, 1, 1), (200, 3, 4, 0, 1))]


def gate_fwd_data(c):
    g = _gen(c.name)
    D = c.H * c.hd
    v = torch.randn(c.B, c.L, D, generator=g).to(c.dt)
    lg = torch.randn(c.B, c.L, c.H, generator=g) * 1.5
    if c.spread and c.L > 1:                                # a spread of about 80: without the max subtraction exp overflows / underflows
        lg[:, 0, :] = 40.0
        lg[:, c.L // 2, :] = -40.0
    return v, lg.to(c.dt)


def gate_bound(gate, d, L):
    """Relative bound of the gate, [B][H][L] (MARGIN included)."""
    t = 2 * d + 2
    return MARGIN * U_F * (t + (gate * t).sum(-1, keepdim=True) + L + 4)


def check_gate_fwd(c, v, logits, gate, out):
    rg, d, rout, m = er.token_gate_fwd(v, logits, c.H, float(c.res))
    tau = gate_bound(rg, d, c.L)
    echeck(c.name, "gate_softmax_kernel<%s>" % DTN[c.dt], "gate", F32, gate, rg, tau * rg)
    eg = (tau * rg)[:, m["j"], m["l"]].reshape(rout.shape)
    echeck(c.name, "gate_apply_kernel<%s>" % DTN[c.dt], "out", c.dt, out, rout,
           MARGIN * (u_st(c.dt) + 2 * U_F) * m["out"] + v.double().abs() * eg)


@pytest.mark.parametrize("c", GATE_FWD, ids=[c.name for c in GATE_FWD])
def test_token_gate_fwd(c):
    L, ok, stream, DT, _ = _lib()
    v, lg = gate_fwd_data(c)
    v, lg = placed(v.to(DEV)), placed(lg.to(DEV))
    D = c.H * c.hd

    def launch():
        out, gate = Out((c.B, c.L, D), c.dt), Out((c.B, c.H, c.L), F32)
        ok(L.dl_token_gate_fwd(v.data_ptr(), lg.data_ptr(), out.v.data_ptr(), gate.v.data_ptr(), c.B, c.L, D, c.H, c.res, DT[c.dt], stream),
           "dl_token_gate_fwd")
        torch.cuda.synchronize()
        return out.done(c.name), gate.done(c.name)

    a, b = launch(), launch()
    same_bits(c.name, a, b)
    check_gate_fwd(c, v, lg, a[1].v, a[0].v)


GateB = collections.namedtuple("GateB", "name form dt B L H hd res")
GATE_BWD = [GateB("gateb_%s_L%d_H%d_hd%d_res%d" % (DTN[dt], L, H, hd, res), form, dt, 2, L, H, hd, res)
            for dt in (F32, BF)
            for (form, L, H, hd, res) in (("gate_bwd_rows_kernel<T>", 65, 3, 4, 1), ("gate_bwd_rows_kernel<T>", 40, 8, 8, 1),
                                          ("gate_bwd_rows_kernel<T>", 13, 3, 32, 0), ("gate_bwd_rows_kernel<T>", 5, 3, 256, 1),
                                          ("gate_bwd_rows_kernel<T>", 1, 8, 8, 0), ("gate_bwd_kernel<T>", 70, 3, 12, 1),
                                          ("gate_bwd_kernel<T>", 1, 3, 24, 0), ("gate_bwd_kernel<T>", 3, 2, 512, 1),
                                          ("gate_bwd_kernel<T>", 130, 3, 24, 0))]


def gate_bwd_form(hd):
    lpr = hd // 4
    return "gate_bwd_rows_kernel<T>" if 1 <= lpr <= 64 and (lpr & (lpr - 1)) == 0 else "gate_bwd_kernel<T>"


def gate_bwd_data(c):
    g = _gen(c.name)
    D = c.H * c.hd
    dout = torch.randn(c.B, c.L, D, generator=g).to(c.dt)
    v = torch.randn(c.B, c.L, D, generator=g).to(c.dt)
    gate = torch.softmax(torch.randn(c.B, c.H, c.L, generator=g) * 1.5, -1)            # fp32 operand of the kernel
    return dout, v, gate


def check_gate_bwd(c, dout, v, gate, dv, dlogits):
    rdv, rdl, m = er.token_gate_bwd(dout, v, gate, c.H, float(c.res))
    form = c.form.replace("<T>", "<%s>" % DTN[c.dt])
    echeck(c.name, form, "dv", c.dt, dv, rdv, MARGIN * (u_st(c.dt) + 2 * U_F) * m["dv"])
    echeck(c.name, form, "dlogits", c.dt, dlogits, rdl, MARGIN * (u_st(c.dt) + (c.L + c.hd + 5) * U_F) * m["dlogits"])


@pytest.mark.parametrize("c", GATE_BWD, ids=[c.name for c in GATE_BWD])
def test_token_gate_bwd(c):
    L, ok, stream, DT, _ = _lib()
    dout, v, gate = (placed(t.to(DEV)) for t in gate_bwd_data(c))
    D = c.H * c.hd

    def launch():
        dv, dl = Out((c.B, c.L, D), c.dt), Out((c.B, c.L, c.H), c.dt)
        ok(L.dl_token_gate_bwd(dout.data_ptr(), v.data_ptr(), gate.data_ptr(), dv.v.data_ptr(), dl.v.data_ptr(), c.B, c.L, D, c.H, c.res,
                               DT[c.dt], stream), "dl_token_gate_bwd")
        torch.cuda.synchronize()
        return dv.done(c.name), dl.done(c.name)

    a, b = launch(), launch()
    same_bits(c.name, a, b)
    check_gate_bwd(c, dout, v, gate, a[0].v, a[1].v)


# =================================================================================================================================
# positional add + dropout, dropout apply
# =================================================================================================================================
def find_seed(rows, D, thr, start):
    """The first seed from `start` on whose mask has a kept and a dropped element in every row (the CPU test asserts it)."""
    s = start
    while True:
        k = er.keep_mask(s, rows, D, thr)
        if k.any(1).all() and (~k).any(1).all():
            return s
        s += 1


Drop = collections.namedtuple("Drop", "name form dt M D L pe p seed off")


def _drop(dt, M, D, L, pe, p, start, off=0):
    thr = er.dropout_thr16(p) if p > 0 else 0
    seed = find_seed(M, D, thr, start) - off if thr else start
    return Drop("rowmod_%s_M%d_D%d_L%d_pe%d_p%g_off%d" % (DTN[dt], M, D, L, pe, p, off), "add_rowmod_dropout_kernel<T>", dt, M, D, L, pe, p,
                seed, off)


ROWMOD = [_drop(dt, M, D, L, pe, p, start, off) for dt in (F32, BF) for (M, D, L, pe, p, start, off) in (
    (50, 32, 16, 1, 0.0, 11, 0), (50, 32, 16, 0, 0.0, 12, 0), (50, 32, 16, 1, 0.1, 0x1234567800000000, 0), (50, 32, 16, 0, 0.5, 77, 5),
    (7, 4, 5, 1, 0.5, 1000, 0), (300, 8, 7, 1, 0.5, 2 ** 63 + 9, 3),
    (50, 32, 16, 1, 2.0 ** -18, 5, 0))]                     # thr16 == 0: no dropout, the plain sum (no 1 / (1 - p))


def drop_data(c):
    g = _gen(c.name)
    x = torch.randn(c.M, c.D, generator=g)
    x = (x + 0.5 * torch.sign(x)).to(c.dt)                  # |x| >= 0.5 > |pe|: no sum is zero, the mask can be read off the output
    pe = ((torch.rand(c.L, c.D, generator=g) - 0.5) * 0.8).to(c.dt) if c.pe else None
    return x, pe


def check_dropout(c, form, x, pe, L, y, what="y", roundings=2):
    """y against keep ? (x + pe) fl(1 / (1 - p)) : +0 with the replica's mask; the mask itself exactly; the kept share."""
    M, D = x.shape
    s, mag = er.add_rowmod(x, pe, L)
    thr = er.dropout_thr16(c.p) if c.p > 0 else 0
    if thr == 0:                                            # p == 0 or p < 2^-17: no dropout, no scaling; without pe a bit-exact copy
        echeck(c.name, form, what, c.dt, y, s, MARGIN * (u_st(c.dt) + U_F) * mag if pe is not None else 0 * mag)
        return
    keep = torch.from_numpy(er.keep_mask(c.seed + c.off, M, D, thr)).to(x.device)
    ref, rmag = er.dropout(s, keep, c.p)
    assert bool((s != 0).all()), "%s: the data has a zero sum: the mask cannot be read off the output" % c.name
    exact(c.name, form, what + " mask", (y != 0), keep)
    exact(c.name, form, what + " dropped", y[~keep], torch.zeros_like(y[~keep]))
    echeck(c.name, form, what, c.dt, y, ref, MARGIN * (u_st(c.dt) + roundings * U_F) * rmag)
    q, n = 1 - thr / 65536.0, M * D
    share = float(keep.double().mean())
    assert abs(share - q) <= 6 * math.sqrt(q * (1 - q) / n), "%s: kept share %.4f, expected %.4f" % (c.name, share, q)


@pytest.mark.parametrize("c", ROWMOD, ids=[c.name for c in ROWMOD])
def test_add_rowmod_dropout(c):
    L, ok, stream, DT, _ = _lib()
    x, pe = drop_data(c)
    x = placed(x.to(DEV))
    pe = None if pe is None else placed(pe.to(DEV))
    off = torch.tensor([c.off], dtype=torch.int64, device=DEV) if c.off else None

    def launch(seed, off):
        y = Out((c.M, c.D), c.dt)
        ok(L.dl_add_rowmod_dropout(x.data_ptr(), _ptr(pe), y.v.data_ptr(), c.M, c.D, c.L, c.p, seed % 2 ** 64, _ptr(off), DT[c.dt], stream),
           "dl_add_rowmod_dropout")
        torch.cuda.synchronize()
        return (y.done(c.name),)

    a, b = launch(c.seed, off), launch(c.seed, off)
    same_bits(c.name, a, b)
    check_dropout(c, "add_rowmod_dropout_kernel<%s>" % DTN[c.dt], x, pe, c.L, a[0].v)
    if c.off:                                               # the device offset == the same amount added to the by-value seed
        same_bits(c.name + " (offset by value)", a, launch(c.seed + c.off, None))


DropA = collections.namedtuple("DropA", "name form dt M D ldx ldy p seed off")


def _dropa(dt, M, D, ldx, ldy, p, start, off):
    seed = find_seed(M, D, er.dropout_thr16(p), start) - off if er.dropout_thr16(p) else start
    return DropA("dropapply_%s_M%d_D%d_ldx%d_ldy%d_p%g_off%d" % (DTN[dt], M, D, ldx, ldy, p, off), "dropout_apply_kernel<T>", dt, M, D, ldx, ldy,
                 p, seed, off)


DROP_APPLY = [_dropa(dt, *r) for dt in (F32, BF) for r in ((40, 32, 32, 32, 0.1, 100, 0), (40, 32, 40, 36, 0.5, 200, 0),
                                                          (300, 8, 12, 8, 0.5, 300, 7), (9, 4, 8, 12, 0.5, 2 ** 40, 2 ** 33),
                                                          (40, 32, 32, 32, 2.0 ** -18, 5, 0))]        # thr16 == 0, as in ROWMOD


def dropa_data(c):
    x = torch.randn(c.M, c.D, generator=_gen(c.name))
    return (x + 0.5 * torch.sign(x)).to(c.dt)


@pytest.mark.parametrize("c", DROP_APPLY, ids=[c.name for c in DROP_APPLY])
def test_dropout_apply(c):
    L, ok, stream, DT, _ = _lib()
    x = placed(dropa_data(c).to(DEV), strides=(c.ldx, 1), n=c.M * c.ldx)
    off = torch.tensor([c.off], dtype=torch.int64, device=DEV) if c.off else None

    def launch(seed, off):
        y = Out((c.M, c.D), c.dt, strides=(c.ldy, 1), n=c.M * c.ldy)
        ok(L.dl_dropout_apply(x.data_ptr(), y.v.data_ptr(), c.M, c.D, c.ldx, c.ldy, c.p, seed % 2 ** 64, _ptr(off), DT[c.dt], stream),
           "dl_dropout_apply")
        torch.cuda.synchronize()
        return (y.done(c.name),)

    a, b = launch(c.seed, off), launch(c.seed, off)
    same_bits(c.name, a, b)
    check_dropout(c, "dropout_apply_kernel<%s>" % DTN[c.dt], x, None, 1, a[0].v, roundings=1)
    if c.off:
        same_bits(c.name + " (offset by value)", a, launch(c.seed + c.off, None))


def test_gemm_leaves_a_thr16_zero_site_alone():
    """The third party to the thr16 == 0 contract: dl_gemm with 0 < dropout_p < 2^-17 runs no dropout epilogue, so its output
    equals the dropout_p = 0 launch bit for bit (LinearFn replays such a site through dl_dropout_apply, which then copies)."""
    from druglamp_amd import ops
    g = torch.Generator().manual_seed(18)
    for dt in (F32, BF):
        x, w = torch.randn(70, 64, generator=g).to(dt).to(DEV), torch.randn(48, 64, generator=g).to(dt).to(DEV)
        bias = torch.randn(48, generator=g).to(DEV)
        kw = dict(M=70, N=48, K=64, bias=bias)
        plain = ops.gemm(x, w, **kw)
        tiny = ops.gemm(x, w, dropout_p=2.0 ** -18, seed=5, **kw)
        torch.cuda.synchronize()
        exact("gemm_thr16_zero_%s" % DTN[dt], "dl_gemm epilogue", "out", tiny, plain)
        dropped = ops.gemm(x, w, dropout_p=0.5, seed=5, **kw)
        assert bool((dropped == 0).any()) and not torch.equal(dropped, plain)            # (the argument does reach the epilogue)


# =================================================================================================================================
# GELU derivative, gate_dpre
# =================================================================================================================================
Gelu = collections.namedtuple("Gelu", "name form dt n")
GELU = [Gelu("gelubwd_%s_n%d" % (DTN[dt], n), "gelu_bwd_kernel<T>", dt, n) for dt in (F32, BF) for n in (4, 1028)]


def gelu_data(c):
    g = _gen(c.name)
    pre = torch.cat((torch.tensor([-0.0, 0.0]), torch.linspace(-12.0, 12.0, c.n - 2)))
    dy = torch.randn(c.n, generator=g) + 0.25
    return dy.to(c.dt), pre.to(c.dt)


def check_gelu_bwd(c, dy, pre, dx):
    ref, mag = er.gelu_bwd(dy, pre)
    echeck(c.name, "gelu_bwd_kernel<%s>" % DTN[c.dt], "dx", c.dt, dx, ref, MARGIN * ((u_st(c.dt) + U_F) * mag + dy.double().abs() * E_G))


@pytest.mark.parametrize("c", GELU, ids=[c.name for c in GELU])
def test_gelu_bwd(c):
    L, ok, stream, DT, _ = _lib()
    dy, pre = (placed(t.to(DEV)) for t in gelu_data(c))

    def launch():
        dx = Out((c.n,), c.dt)
        ok(L.dl_gelu_bwd(dy.data_ptr(), pre.data_ptr(), dx.v.data_ptr(), c.n, DT[c.dt], stream), "dl_gelu_bwd")
        torch.cuda.synchronize()
        return (dx.done(c.name),)

    a, b = launch(), launch()
    same_bits(c.name, a, b)
    check_gelu_bwd(c, dy, pre, a[0].v)


Dpre = collections.namedtuple("Dpre", "name form dt M dd")
DPRE = [Dpre("dpre_%s_M%d_dd%d" % (DTN[dt], M, dd), "gate_dpre_kernel<T, 8>", dt, M, dd) for dt in (F32, BF)
        for (M, dd) in ((2049, 8), (1, 8), (681, 24), (3000, 24), (257, 64), (81, 200), (1, 200), (9, 2048), (2500, 64))]


def dpre_plan(M, dd):
    """(cpr, rpb, blocks, idle threads per block) of the host dispatch."""
    cpr = dd // 8
    rpb = 256 // cpr
    blocks = max(1, min(8192, (M + rpb * 8 - 1) // (rpb * 8)))
    return cpr, rpb, blocks, 256 - cpr * rpb


def dpre_data(c):
    g = _gen(c.name)
    return (torch.randn(c.M, 8, generator=g).to(c.dt), (torch.randn(8, c.dd, generator=g) * 0.3).to(c.dt),
            (torch.randn(c.M, c.dd, generator=g) * 2.0).to(c.dt))


def check_gate_dpre(c, dl, w2, pre, out):
    ref, acc, S, g = er.gate_dpre(dl, w2, pre)
    e_g = E_G + (E_G_FAST if c.dt == BF else 0.0)
    echeck(c.name, "gate_dpre_kernel<%s, 8>" % DTN[c.dt], "dpre", c.dt, out, ref,
           MARGIN * ((u_st(c.dt) + U_F) * ref.abs() + 9 * U_F * S * g.abs() + acc.abs() * e_g))


@pytest.mark.parametrize("c", DPRE, ids=[c.name for c in DPRE])
def test_gate_dpre(c):
    L, ok, stream, DT, _ = _lib()
    dl, w2, pre = (placed(t.to(DEV)) for t in dpre_data(c))

    def launch():
        out = Out((c.M, c.dd), c.dt)
        ok(L.dl_gate_dpre(dl.data_ptr(), w2.data_ptr(), pre.data_ptr(), out.v.data_ptr(), c.M, c.dd, 8, DT[c.dt], stream), "dl_gate_dpre")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    a, b = launch(), launch()
    same_bits(c.name, a, b)
    check_gate_dpre(c, dl, w2, pre, a[0].v)


# =================================================================================================================================
# fill_pool, rowmod_sum
# =================================================================================================================================
FillPool = collections.namedtuple("FillPool", "name form dti dto B n_site site_len F")
FILL_POOL = [FillPool("fillpool_%s_%s_B%d_ns%d_sl%d_F%d" % (DTN[a], DTN[b], B, ns, sl, F), "fill_pool_kernel<T, TO>", a, b, B, ns, sl, F)
             for a in (F32, BF) for b in (F32, BF) for (B, ns, sl, F) in ((3, 5, 1, 8), (3, 3, 3, 520), (1, 2, 9, 1024), (5, 1, 3, 8))]


def fill_pool_data(c):
    """x [B][S][F]: rows that are all +0, all -0, and rows with a sum well away from zero (mean 0.5)."""
    g = _gen(c.name)
    S = c.n_site * c.site_len
    x = (torch.randn(c.B, S, c.F, generator=g) + 0.5).to(c.dti).float()
    flat = x.view(c.B * S, c.F)
    flat[0::4] = 0.0
    flat[2::8] = -0.0
    if flat.shape[0] > 1:
        flat[1] = (torch.randn(c.F, generator=g) + 0.5).to(c.dti).float()
    return x.to(c.dti)


def check_fill_pool(c, x, fill, pooled):
    form = "fill_pool_kernel<%s, %s>" % (DTN[c.dti], DTN[c.dto])
    rfill, rp, mag, _, _ = er.fill_pool(x, c.site_len)
    exact(c.name, form, "fill", fill, rfill.to(c.dti))
    echeck(c.name, form, "pooled", c.dto, pooled, rp, MARGIN * (u_st(c.dto) + (c.site_len + 2) * U_F) * mag)
    exact(c.name, form, "pooled zero columns", pooled[..., c.F + 1:], torch.zeros_like(pooled[..., c.F + 1:]))


@pytest.mark.parametrize("c", FILL_POOL, ids=[c.name for c in FILL_POOL])
def test_fill_pool(c):
    L, ok, stream, DT, _ = _lib()
    x = placed(fill_pool_data(c).to(DEV))
    S, Fp = c.n_site * c.site_len, (c.F + 1 + 7) // 8 * 8

    def launch():
        fill, pooled = Out((c.B, S), c.dti), Out((c.B, c.n_site, Fp), c.dto)
        ok(L.dl_fill_pool(x.data_ptr(), fill.v.data_ptr(), pooled.v.data_ptr(), c.B, S, c.F, c.site_len, DT[c.dti], DT[c.dto], stream), "dl_fill_pool")
        torch.cuda.synchronize()
        return fill.done(c.name), pooled.done(c.name)

    a, b = launch(), launch()
    same_bits(c.name, a, b)
    check_fill_pool(c, x, a[0].v, a[1].v)


RowSum = collections.namedtuple("RowSum", "name form dt nb L D acc")
ROWMOD_SUM = [RowSum("rowmodsum_%s_nb%d_L%d_D%d_acc%d" % (DTN[dt], nb, L, D, acc), "rowmod_sum_kernel<T>", dt, nb, L, D, acc)
              for dt in (F32, BF) for i, nb in enumerate((1, 3, 4, 5, 16, 17, 29, 33))
              for (L, D, acc) in (((3, 4), (4, 64), (5, 52))[i % 3] + (i % 2,), ((3, 4), (4, 64), (5, 52))[(i + 1) % 3] + (1 - i % 2,))]


def rowmod_sum_data(c):
    g = _gen(c.name)
    return (torch.randn(c.nb * c.L, c.D, generator=g) + 0.25).to(c.dt), torch.randn(c.L, c.D, generator=g)


def check_rowmod_sum(c, x, old, out):
    ref, mag = er.rowmod_sum(x, c.L, old if c.acc else None)
    echeck(c.name, "rowmod_sum_kernel<%s>" % DTN[c.dt], "out", F32, out, ref, MARGIN * (c.nb + 2) * U_F * mag)


@pytest.mark.parametrize("c", ROWMOD_SUM, ids=[c.name for c in ROWMOD_SUM])
def test_rowmod_sum(c):
    L, ok, stream, DT, _ = _lib()
    x, old = rowmod_sum_data(c)
    x, old = placed(x.to(DEV)), old.to(DEV)

    def launch():
        out = Out((c.L, c.D), F32)
        if c.acc:
            out.v.copy_(old)
            out.before = out.g.bits()
        ok(L.dl_rowmod_sum(x.data_ptr(), out.v.data_ptr(), c.nb * c.L, c.D, c.L, c.acc, DT[c.dt], stream), "dl_rowmod_sum")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    a, b = launch(), launch()
    same_bits(c.name, a, b)
    check_rowmod_sum(c, x, old, a[0].v)


# =================================================================================================================================
# AdamW
# =================================================================================================================================
Adam = collections.namedtuple("Adam", "name form lowp n")
ADAMW = [Adam("adamw_lowp%s_n%d" % (DTN.get(lp, "none"), n), "adamw_kernel<TL>", lp, n) for lp in (None, F32, BF) for n in (1, 4, 1003, 1028)]
ADAM_HYPER = ((1, 1.0, 0.0), (1000, 1.0 / 128, 1e-2), (1, 1.0 / 128, 1e-2), (1000, 1.0, 0.0))       # (step, grad_scale, weight_decay)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8


def adamw_data(c, hyper):
    g = _gen(c.name + str(hyper))
    n = c.n
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) / hyper[1]
    m, v = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 1e-2 + 1e-4
    zero = torch.arange(n) % 5 == 3                         # elements with g = m = v = 0: the denominator is eps itself
    if n == 1:
        zero[:] = hyper[0] == 1000
    gr[zero], m[zero], v[zero] = 0.0, 0.0, 0.0
    return p, gr, m, v


def check_adamw(c, hyper, p0, g, m0, v0, p1, m1, v1, lowp):
    step, gscale, wd = hyper
    rp, rm, rv, k = er.adamw(p0, g, m0, v0, ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, wd, step, gscale)
    form = "adamw_kernel<%s>" % ("bf16" if c.lowp == BF else "float")
    name = "%s step%d gs%g wd%g" % (c.name, step, gscale, wd)
    e_bc1, e_bc2s = (2 * k["amp1"] + 1) * U_F, (k["amp2"] + 2) * U_F
    e_m = 4 * U_F * k["m"]
    tau_den = 5.5 * U_F + e_bc2s
    e_u = k["step_scale"] * e_m / k["den"] + k["u"] * (tau_den + 3 * U_F + e_bc1)
    echeck(name, form, "exp_avg", F32, m1, rm, MARGIN * e_m)
    echeck(name, form, "exp_avg_sq", F32, v1, rv, MARGIN * 5 * U_F * k["v"])
    echeck(name, form, "param", F32, p1, rp, MARGIN * (4 * U_F * (k["x"] + k["u"]) + e_u))
    if c.lowp is not None:
        exact(name, form, "lowp", lowp, er.cast(p1, c.lowp))


@pytest.mark.parametrize("c", ADAMW, ids=[c.name for c in ADAMW])
def test_adamw_step(c):
    L, ok, stream, DT, _ = _lib()
    for hyper in ADAM_HYPER:
        step, gscale, wd = hyper
        p0, g, m0, v0 = (t.to(DEV) for t in adamw_data(c, hyper))
        gp = placed(g)

        def launch():
            outs = [Out((c.n,), F32) for _ in range(3)] + ([Out((c.n,), c.lowp)] if c.lowp is not None else [])
            for o, src in zip(outs, (p0, m0, v0)):
                o.v.copy_(src)
                o.before = o.g.bits()
            ok(L.dl_adamw_step(outs[0].v.data_ptr(), gp.data_ptr(), outs[1].v.data_ptr(), outs[2].v.data_ptr(), c.n, ADAM_LR, ADAM_B1, ADAM_B2,
                               ADAM_EPS, wd, step, gscale, outs[3].v.data_ptr() if c.lowp is not None else None,
                               DT[c.lowp] if c.lowp is not None else 0, stream), "dl_adamw_step")
            torch.cuda.synchronize()
            return [o.done(c.name) for o in outs]

        a, b = launch(), launch()
        same_bits(c.name, a, b)
        check_adamw(c, hyper, p0, g, m0, v0, a[0].v, a[1].v, a[2].v, a[3].v if c.lowp is not None else None)


# =================================================================================================================================
# cast
# =================================================================================================================================
Cast = collections.namedtuple("Cast", "name form sdt ddt n")
CAST = [Cast("cast_%s_%s_n%d" % (DTN[a], DTN[b], n), "cast_kernel<TS, TD>", a, b, n) for a in (F32, BF) for b in (F32, BF) for n in (1, 3, 4, 5, 1027)]


def _f32_from_bits(bits):
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


CAST_SPECIALS = _f32_from_bits([
    0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,         # exact ties: to even downwards, to even upwards, both signs
    0x3f808001, 0x3f807fff, 0x3f80ffff,                     # just past / just short of a tie; carries into the next binade: 0x3fffffff below
    0x3fffffff, 0x00000000, 0x80000000, 0x7f800000, 0xff800000,
    0x7f7fffff, 0xff7fffff, 0x7f7f0000, 0x7f7f7fff,         # the largest finite fp32 (rounds to inf), the largest bf16, just below the tie to inf
    0x00000001, 0x80000001, 0x007fffff, 0x00008000, 0x00018000, 0x00010000, 0x0000ffff, 0x00400000])   # fp32 subnormals


def cast_data(c):
    g = _gen(c.name)
    x = torch.randn(c.n, generator=g) * 3
    if c.sdt == F32:
        x[:1] = CAST_SPECIALS[0]
        if c.n >= CAST_SPECIALS.numel():
            x[:CAST_SPECIALS.numel()] = CAST_SPECIALS
            x[-3:] = CAST_SPECIALS[1:4]                      # ties in the scalar tail too
    return x.to(c.sdt) if c.sdt == BF else x


def check_cast(c, src, dst):
    exact(c.name, "cast_kernel<%s, %s>" % (DTN[c.sdt], DTN[c.ddt]), "dst", dst, er.cast(src, c.ddt))


@pytest.mark.parametrize("c", CAST, ids=[c.name for c in CAST])
def test_cast(c):
    L, ok, stream, DT, _ = _lib()
    src = placed(cast_data(c).to(DEV))

    def launch():
        dst = Out((c.n,), c.ddt)
        ok(L.dl_cast(src.data_ptr(), DT[c.sdt], dst.v.data_ptr(), DT[c.ddt], c.n, stream), "dl_cast")
        torch.cuda.synchronize()
        return (dst.done(c.name),)

    a, b = launch(), launch()
    same_bits(c.name, a, b)
    check_cast(c, src, a[0].v)


# =================================================================================================================================
# MolecularGCN: adjacency normalisation, aggregation
# =================================================================================================================================
NormAdj = collections.namedtuple("NormAdj", "name form dto n")


def norm_adj_form(n):
    lds = (n * (n + 1) + 2 * n) * 4
    return ("norm_adj_any_kernel<TO>" if lds > 150 * 1024 else "norm_adj_kernel<TO>"), lds > 64 * 1024


NORM_ADJ = [NormAdj("normadj_%s_n%d" % (DTN[dt], n), norm_adj_form(n)[0], dt, n) for dt in (F32, BF) for n in (1, 5, 126, 127, 128, 194, 195, 300)]


def norm_adj_data(c):
    """[2][n][n] fp32: sample 0 a 0/1 adjacency with isolated nodes (and self loops on some), sample 1 weighted (weights in
    [0.5, 1.5]); the CPU test asserts that no degree sum lies within 2^-10 of the clamp at 1."""
    g = _gen(c.name)
    n = c.n
    a = (torch.rand(2, n, n, generator=g) < min(1.0, 4.0 / max(n, 1) + 0.05)).float()
    a[:, n // 2, :] = 0.0
    a[:, :, n // 2] = 0.0                                   # an isolated node
    a[1] = a[1] * (0.5 + torch.rand(n, n, generator=g))
    return a


def check_norm_adj(c, adj, ahat):
    ref, mag, _, _ = er.norm_adjacency(adj)
    form = c.form.replace("TO", DTN[c.dto])
    echeck(c.name, form, "ahat[0/1]", c.dto, ahat[0], ref[0], MARGIN * (u_st(c.dto) + 10 * U_F) * mag[0])
    echeck(c.name, form, "ahat[weighted]", c.dto, ahat[1], ref[1], MARGIN * (u_st(c.dto) + (c.n + 10) * U_F) * mag[1])


@pytest.mark.parametrize("c", NORM_ADJ, ids=[c.name for c in NORM_ADJ])
def test_norm_adjacency(c):
    L, ok, stream, DT, _ = _lib()
    adj = placed(norm_adj_data(c).to(DEV))

    def launch():
        out = Out((2, c.n, c.n), c.dto)
        ok(L.dl_norm_adjacency(adj.data_ptr(), out.v.data_ptr(), 2, c.n, DT[c.dto], stream), "dl_norm_adjacency")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    a, b = launch(), launch()
    same_bits(c.name, a, b)
    check_norm_adj(c, adj, a[0].v)


Agg = collections.namedtuple("Agg", "name form dt n")
AGG = [Agg("aggregate_%s_n%d" % (DTN[dt], n), "graph_aggregate_kernel<T, 128>" if n <= 128 else "graph_aggregate_any_kernel<T, 128>", dt, n)
       for dt in (F32, BF) for n in (1, 5, 16, 17, 77, 124, 128, 129, 160, 333)]
AGG_B, AGG_C = 3, 128


def agg_data(c, N):
    g = _gen(c.name + str(N))
    ahat = (torch.randn(AGG_B, c.n, c.n, generator=g) / math.sqrt(c.n)).to(c.dt)
    feat = torch.randn(AGG_B, N, AGG_C, generator=g).to(c.dt)
    return ahat, feat


def check_aggregate(c, tag, ahat, feat, transpose, out):
    n = c.n
    ref, mag = er.graph_aggregate(ahat, feat, n, transpose)
    form = c.form.replace("<T", "<" + DTN[c.dt])
    echeck(c.name + tag, form, "out", c.dt, out[:, :n], ref[:, :n], MARGIN * ((n + 2) * 2 * U_F * mag[:, :n] + u_st(c.dt) * ref[:, :n].abs()))
    if out.shape[1] > n:
        exact(c.name + tag, form, "virtual nodes", out[:, n:], feat[:, n:])


@pytest.mark.parametrize("c", AGG, ids=[c.name for c in AGG])
def test_graph_aggregate(c):
    L, ok, stream, DT, _ = _lib()
    for N in (c.n, c.n + 3):
        ahat, feat = (placed(t.to(DEV)) for t in agg_data(c, N))
        if c.n % 2 and c.dt == F32:                         # odd n: the samples' adjacency blocks alternate in 16-byte alignment
            assert len({(ahat.data_ptr() + b * c.n * c.n * 4) % 16 for b in range(AGG_B)}) > 1
        for tr in (0, 1):
            def launch():
                out = Out((AGG_B, N, AGG_C), c.dt)
                ok(L.dl_graph_aggregate(ahat.data_ptr(), feat.data_ptr(), out.v.data_ptr(), AGG_B, c.n, N, AGG_C, tr, DT[c.dt], stream),
                   "dl_graph_aggregate")
                torch.cuda.synchronize()
                return (out.done(c.name),)

            a, b = launch(), launch()
            same_bits(c.name, a, b)
            check_aggregate(c, "[N=%d,transpose=%d]" % (N, tr), ahat, feat, tr, a[0].v)


# =================================================================================================================================
# data movers
# =================================================================================================================================
Gather = collections.namedtuple("Gather", "name form dt S F lengths repeat")
GATHER = [Gather("gatherpad_%s_S%d_F%d_rep%d" % (DTN[dt], S, F, rep), "gather_pad_kernel<T>", dt, S, F, lens, rep)
          for rep in (0, 1) for (dt, S, F, lens) in ((BF, 12, 8, (-1, 0, 1, 11, 12, 13, 4, 7)), (F32, 12, 4, (13, 4, 12, 0, 11, -1, 1, 6)),
                                                     (BF, 4100, 32, (4100, 7, 5000, 2050)), (F32, 6, 260, (6, 2, 5)))]


def gather_plan(c):
    """(chunks per sample, workgroups along x) of the host dispatch: the grid-stride loop runs from 64 * 256 chunks."""
    per = c.S * (c.F * (2 if c.dt == BF else 4) // 16)
    return per, min(64, (per + 255) // 256)


def gather_data(c):
    g = _gen(c.name)
    need = [max(0, ln) if c.repeat else max(0, min(ln, c.S)) for ln in c.lengths]
    need = [0 if (c.repeat and ln > c.S) else nd for ln, nd in zip(c.lengths, need)]
    rows = sum(need) + 5
    store = torch.randn(rows, c.F, generator=g).to(c.dt)
    order = torch.randperm(len(need), generator=g).tolist()           # non-monotone offsets
    offs, pos = [0] * len(need), 2
    for i in order:
        offs[i] = pos
        pos += need[i]
    return store, torch.tensor(offs, dtype=torch.int64), torch.tensor(c.lengths, dtype=torch.int32)


def check_gather_pad(c, store, offsets, lengths, out):
    exact(c.name, "gather_pad_kernel<%s>" % DTN[c.dt], "out", out, er.gather_pad(store, offsets.tolist(), lengths.tolist(), c.S, c.repeat))


@pytest.mark.parametrize("c", GATHER, ids=[c.name for c in GATHER])
def test_gather_pad(c):
    L, ok, stream, DT, _ = _lib()
    store, offs, lens = gather_data(c)
    store, offs, lens = placed(store.to(DEV)), table(offs, -7, torch.int64), table(lens)
    B = len(c.lengths)

    def launch():
        out = Out((B, c.S, c.F), c.dt)
        ok(L.dl_gather_pad(store.data_ptr(), offs.data_ptr(), lens.data_ptr(), out.v.data_ptr(), B, c.S, c.F, c.repeat, DT[c.dt], stream),
           "dl_gather_pad")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    a, b = launch(), launch()
    same_bits(c.name, a, b)
    check_gather_pad(c, store, offs, lens, a[0].v)


Embed = collections.namedtuple("Embed", "name form dt B L V D halo")
EMBED = [Embed("embed_%s_B%d_L%d_V%d_D%d_halo%d" % (DTN[dt], B, L, V, D, halo), "embed_pad_kernel<T> | embed_rows_kernel<T>", dt, B, L, V, D, halo)
         for dt in (F32, BF) for (B, L, V, D, halo) in ((3, 9, 26, 7, 0), (3, 9, 26, 7, 4), (2, 33, 26, 127, 4), (2, 300, 128, 127, 0),
                                                        (2, 4100, 5, 7, 4))]


def embed_plan(c):
    """chunks per sample and workgroups along x of dl_embed_pad: the grid-stride loop runs from 16 * 256 chunks."""
    per = (c.L + 2 * c.halo) * ((c.D + 1) // 8)
    return per, min(16, (per + 255) // 256)


def embed_data(c):
    """ids with -3, 0, V - 1, V + 5 among them; the padded table's last column is NaN (never read into an output)."""
    g = _gen(c.name)
    ids = torch.randint(0, c.V, (c.B, c.L), generator=g)
    ids[0, :4] = torch.tensor([-3, 0, c.V - 1, c.V + 5])
    ids[-1, -2:] = torch.tensor([c.V + 5, -3])
    weight = torch.randn(c.V, c.D + 1, generator=g).to(c.dt)
    weight[:, c.D] = float("nan")
    fill = (torch.rand(c.B, c.L, generator=g) < 0.3).to(c.dt)
    # row table of the compact form: every position once in a scrambled order, "no row" entries (src < 0) in between
    src = torch.randperm(c.B * c.L, generator=g).to(torch.int32)
    src = torch.cat((src[:5], torch.tensor([-1, -1], dtype=torch.int32), src[5:], torch.tensor([-1], dtype=torch.int32), src[:3]))
    return ids, weight, fill, src


def check_embed(c, what, ids, weight, fill, src, out):
    dn = DTN[c.dt]
    if what == "pad":
        exact(c.name, "embed_pad_kernel<%s>" % dn, "out", out, er.embed_pad(ids, weight, fill, c.D, c.halo))
    else:
        exact(c.name, "embed_rows_kernel<%s>" % dn, "out", out, er.embed_rows(ids, weight, fill, src, c.D))


@pytest.mark.parametrize("c", EMBED, ids=[c.name for c in EMBED])
def test_embed_pad_and_rows(c):
    L, ok, stream, DT, _ = _lib()
    ids, weight, fill, src = embed_data(c)
    ids, src = table(ids, c.V + 1000, torch.int64), table(src)
    weight, fill = placed(weight.to(DEV)), placed(fill.to(DEV))
    R = src.numel()

    def launch_pad():
        out = Out((c.B, c.L + 2 * c.halo, c.D + 1), c.dt)
        ok(L.dl_embed_pad(ids.data_ptr(), weight.data_ptr(), fill.data_ptr(), out.v.data_ptr(), c.B, c.L, c.V, c.D, c.halo, DT[c.dt], stream),
           "dl_embed_pad")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    def launch_rows():
        out = Out((R, c.D + 1), c.dt)
        ok(L.dl_embed_rows(ids.data_ptr(), weight.data_ptr(), fill.data_ptr(), src.data_ptr(), out.v.data_ptr(), R, c.V, c.D, None, 0, 0, None,
                           DT[c.dt], stream), "dl_embed_rows")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    a, b = launch_pad(), launch_pad()
    same_bits(c.name, a, b)
    check_embed(c, "pad", ids, weight, fill, src, a[0].v)
    a, b = launch_rows(), launch_rows()
    same_bits(c.name, a, b)
    check_embed(c, "rows", ids, weight, fill, src, a[0].v)


# The rows_gather cap is 16384 workgroups of 1024 chunks, so the case past it needs 16.8 M rows of 16 bytes: a 268 MB output,
# and with the guard's bit copies, the mask, the int32 index and the reference about 2 GB of device memory for the case's
# lifetime; both launches and all compares together take about 0.05 s on an MI355X (the largest interleave / concat2 cases:
# 34 / 42 MB outputs).  It is by far the heaviest case of this file.
Mover = collections.namedtuple("Mover", "name form op R row_bytes S")
MOVERS = ([Mover("rowsgather_R%d_row%d" % (R, rb), "rows_gather_kernel", "gather", R, rb, 0)
           for (R, rb) in ((37, 16), (300, 256), (16384 * 1024 + 5, 16))] +
          [Mover("interleave_R%d_row%d_S%d" % (R, rb, S), "interleave_streams_kernel", "interleave", R, rb, S)
           for (R, rb, S) in ((37, 16, 1), (37, 16, 2), (5, 256, 3), (8192 * 128 + 3, 16, 2))] +
          [Mover("concat2_R%d_row%d" % (R, rb), "concat2_kernel", "concat", R, rb, 0) for (R, rb) in ((37, 16), (9, 256), (8192 * 64 + 1, 16))])


def mover_plan(c):
    """(16-byte chunks, workgroups, the cap) of the host dispatch; concat: b's rows are 3 chunks (12 words) wider than a's."""
    cpr = c.row_bytes // 16
    if c.op == "gather":
        total = c.R * cpr
        return total, min(16384, (total + 1023) // 1024), 16384
    total = c.R * c.S * cpr if c.op == "interleave" else c.R * (cpr + cpr + 3)
    return total, min(8192, (total + 255) // 256), 8192


@pytest.mark.parametrize("c", MOVERS, ids=[c.name for c in MOVERS])
def test_row_movers(c):
    L, ok, stream, DT, _ = _lib()
    g = torch.Generator(device=DEV).manual_seed(len(c.name) + c.R)
    w = c.row_bytes // 4                                    # rows as fp32 words

    def run(call, shape):
        def launch():
            out = Out(shape, F32)
            ok(call(out.v), "dl_" + c.op)
            torch.cuda.synchronize()
            return (out.done(c.name),)
        a, b = launch(), launch()
        same_bits(c.name, a, b)
        return a[0].v

    if c.op == "gather":
        nsrc = 1000
        src = placed(torch.randn(nsrc, w, generator=g, device=DEV))
        index = torch.randint(-1, nsrc, (c.R,), generator=g, device=DEV, dtype=torch.int32)
        index[:2] = torch.tensor([-1, nsrc - 1], dtype=torch.int32)
        index = table(index)
        got = run(lambda o: L.dl_rows_gather(src.data_ptr(), index.data_ptr(), o.data_ptr(), c.R, c.row_bytes, stream), (c.R, w))
        exact(c.name, c.form, "out", got, er.rows_gather(src, index))
    elif c.op == "interleave":
        split = placed(torch.randn(c.S, c.R, w, generator=g, device=DEV))
        got = run(lambda o: L.dl_interleave_streams(split.data_ptr(), o.data_ptr(), c.R, c.row_bytes, c.S, 0, stream), (c.R, c.S * w))
        ref = er.interleave_streams(split)
        exact(c.name, c.form, "interleaved", got, ref)
        joined = placed(ref)
        back = run(lambda o: L.dl_interleave_streams(joined.data_ptr(), o.data_ptr(), c.R, c.row_bytes, c.S, 1, stream), (c.S, c.R, w))
        exact(c.name, c.form, "split (inverse)", back, er.interleave_streams(joined, (c.R, c.S, w)))
    else:
        wb = w + 12
        a_, b_ = placed(torch.randn(c.R, w, generator=g, device=DEV)), placed(torch.randn(c.R, wb, generator=g, device=DEV))
        got = run(lambda o: L.dl_concat2(a_.data_ptr(), b_.data_ptr(), o.data_ptr(), c.R, c.row_bytes, wb * 4, 0, stream), (c.R, w + wb))
        exact(c.name, c.form, "cat", got, er.concat2(a_, b_))
        cat = placed(er.concat2(a_, b_))

        def inv():
            oa, ob = Out((c.R, w), F32), Out((c.R, wb), F32)
            ok(L.dl_concat2(oa.v.data_ptr(), ob.v.data_ptr(), cat.data_ptr(), c.R, c.row_bytes, wb * 4, 1, stream), "dl_concat2")
            torch.cuda.synchronize()
            return oa.done(c.name), ob.done(c.name)
        x, y = inv(), inv()
        same_bits(c.name, x, y)
        exact(c.name, c.form, "a (inverse)", x[0].v, a_)
        exact(c.name, c.form, "b (inverse)", x[1].v, b_)


RSum = collections.namedtuple("RSum", "name form dt C R off")
ROWS_SUM = [RSum("rowssum_%s_C%d_R%d_off%d" % (DTN[dt], C, R, off), form, dt, C, R, off) for (form, dt, C, R, off) in (
    ("rows_sum_wide_kernel<CPR>", BF, 64, 16391, 0), ("rows_sum_wide_kernel<CPR>", BF, 128, 23, 0), ("rows_sum_wide_kernel<CPR>", BF, 256, 23, 0),
    ("rows_sum_wide_kernel<CPR>", BF, 512, 23, 0), ("rows_sum_kernel<T>", BF, 32, 23, 0), ("rows_sum_kernel<T>", BF, 192, 23, 0),
    ("rows_sum_kernel<T>", BF, 128, 23, 4), ("rows_sum_kernel<T>", F32, 128, 23, 0), ("rows_sum_kernel<T>", F32, 4, 70, 0))]


def rows_sum_form(c, x_ptr, out_ptr):
    wide = c.dt == BF and c.C in (64, 128, 256, 512) and (x_ptr | out_ptr) % 16 == 0
    return "rows_sum_wide_kernel<CPR>" if wide else "rows_sum_kernel<T>"


def rows_sum_data(c):
    """x [600][C] and rep [R][3] = (first, stride, count): counts 0, 1, 3, 4 G, 4 G + 1, 200 (G = the wide form's k-groups),
    stride 1 and larger."""
    g = _gen(c.name)
    nx = 600
    x = (torch.randn(nx, c.C, generator=g) + 0.25).to(c.dt)
    G4 = 4 * (64 // (c.C // 8)) if c.C in (64, 128, 256, 512) else 8
    counts = torch.tensor([0, 1, 3, G4, G4 + 1, 200])[torch.arange(c.R) % 6]
    stride = torch.tensor([1, 2, 1, 3])[torch.arange(c.R) % 4]
    first = torch.randint(0, nx, (c.R,), generator=g)
    first = torch.minimum(first, nx - 1 - (counts - 1).clamp_min(0) * stride)
    return x, torch.stack((first, stride, counts), 1).to(torch.int32)


def check_rows_sum(c, form, x, rep, out):
    ref, mag = er.rows_sum_strided(x, rep)
    cnt = rep[:, 2].double()[:, None]
    echeck(c.name, form, "out", c.dt, out, ref, MARGIN * ((cnt + 1) * U_F * mag + u_st(c.dt) * ref.abs()))
    exact(c.name, form, "count 0 rows", out[rep[:, 2] == 0], torch.zeros_like(out[rep[:, 2] == 0]))


@pytest.mark.parametrize("c", ROWS_SUM, ids=[c.name for c in ROWS_SUM])
def test_rows_sum_strided(c):
    L, ok, stream, DT, _ = _lib()
    x, rep = rows_sum_data(c)
    x, rep = placed(x.to(DEV), off=c.off), table(rep)

    def launch():
        out = Out((c.R, c.C), c.dt, off=c.off)
        assert rows_sum_form(c, x.data_ptr(), out.v.data_ptr()) == c.form, "%s: the case names the other form" % c.name
        ok(L.dl_rows_sum_strided(x.data_ptr(), rep.data_ptr(), out.v.data_ptr(), c.R, c.C, DT[c.dt], stream), "dl_rows_sum_strided")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    a, b = launch(), launch()
    same_bits(c.name, a, b)
    form = "rows_sum_wide_kernel<%d>" % (c.C // 8) if c.form.startswith("rows_sum_wide") else "rows_sum_kernel<%s>" % DTN[c.dt]
    check_rows_sum(c, form, x, rep, a[0].v)


# =================================================================================================================================
# weight images
# =================================================================================================================================
# (image, rows, cols, ld, row0, mode, cs); images A..E; B and D are shared by two items through row0
WPREP_ITEMS = (("A", 63, 130, 134, 0, 0, 0), ("B", 65, 64, 64, 0, 0, 0), ("B", 1, 64, 64, 66, 0, 0), ("C", 130, 63, 68, 3, 0, 0),
               ("D", 130, 65, 200, 4, 1, 0), ("D", 63, 1, 200, 134, 1, 0), ("E", 64, 63, 65, 62, 2, -1), ("F", 1, 1, 1, 0, 1, 0),
               ("G", 64, 64, 64, 0, 1, 0))
WPREP_SIZE = {"A": 63 * 134, "B": 67 * 64, "C": 133 * 68, "D": 65 * 200, "E": 64 * 65, "F": 1, "G": 64 * 64}
WPREP = [collections.namedtuple("WPrep", "name form dt")("weightprep_%s" % DTN[dt], "weight_prep_kernel<TD>", dt) for dt in (F32, BF)]


def wprep_sources():
    g = _gen("weight_prep")
    return [torch.randn(r, cl, generator=g) for (_, r, cl, _, _, _, _) in WPREP_ITEMS]


def wprep_reference(dt, srcs, dev):
    """image name -> (expected flat image with NaN where no item writes, addressed mask)."""
    out = {}
    for name, size in WPREP_SIZE.items():
        out[name] = [torch.full((size,), float("nan"), dtype=dt, device=dev), torch.zeros(size, dtype=torch.bool, device=dev)]
    for (name, r, cl, ld, row0, mode, cs), s in zip(WPREP_ITEMS, srcs):
        idx = er.weight_prep_item(out[name][0], s.to(dev), ld, row0, mode, cs)
        assert not bool(out[name][1][idx].any()), "items overlap in image %s" % name
        out[name][1][idx] = True
    return out


@pytest.mark.parametrize("c", WPREP, ids=[c.name for c in WPREP])
def test_weight_prep(c):
    L, ok, stream, DT, _ = _lib()
    srcs = wprep_sources()
    dsrc = [placed(s.to(DEV)) for s in srcs]
    ref = wprep_reference(c.dt, srcs, DEV)
    form = "weight_prep_kernel<%s>" % DTN[c.dt]

    def launch():
        imgs = {k: Guarded(n, c.dt) for k, n in WPREP_SIZE.items()}
        before = {k: g.bits() for k, g in imgs.items()}
        items, bmap = b"", []
        for i, ((name, r, cl, ld, row0, mode, cs), s) in enumerate(zip(WPREP_ITEMS, dsrc)):
            base = imgs[name].t.data_ptr() + Guarded.G * imgs[name].t.element_size()
            items += struct.pack("<QQqiiiiq", s.data_ptr(), base, ld, r, cl, row0, mode, cs)
            bmap += [(i, t) for t in range(((r + 63) // 64) * ((cl + 63) // 64))]
        bmap = bmap[::-1]                                   # any order of the workgroups
        items_dev = torch.frombuffer(bytearray(items), dtype=torch.uint8).to(DEV)
        bmap_dev = table(torch.tensor(bmap, dtype=torch.int32).reshape(-1))
        ok(L.dl_weight_prep(items_dev.data_ptr(), bmap_dev.data_ptr(), len(bmap), DT[c.dt], stream), "dl_weight_prep")
        torch.cuda.synchronize()
        for k, g in imgs.items():
            g.mask[Guarded.G:Guarded.G + WPREP_SIZE[k]] = ref[k][1]
            g.untouched(c.name + " image " + k, before[k])
        return imgs

    a, b = launch(), launch()
    for k in a:
        assert torch.equal(a[k].bits(), b[k].bits()), "%s: not bitwise repeatable" % c.name
        got = a[k].t[Guarded.G:Guarded.G + WPREP_SIZE[k]]
        exact(c.name, form, "image " + k, got[ref[k][1]], ref[k][0][ref[k][1]])


# =================================================================================================================================
# ProteinCNN tail: site pooling on the dense layout
# =================================================================================================================================
Pool = collections.namedtuple("Pool", "name form B n_site site_len C halo")


def sitepool_form(n_site, site_len, C):
    L = n_site * site_len
    return "transpose_view_kernel" if site_len == 1 and L % 64 == 0 and C % 64 == 0 else "general"


SITEPOOL = [Pool("sitepool_ns%d_sl%d_C%d_halo%d" % (ns, sl, C, halo),
                 "transpose_view_kernel" if sitepool_form(ns, sl, C) != "general" else "cnn_sitepool_fwd_kernel<bf16> | cnn_sitepool_bwd_kernel<bf16>",
                 2, ns, sl, C, halo)
            for (ns, sl, C, halo) in ((1, 3, 8, 0), (31, 5, 64, 4), (32, 9, 128, 0), (33, 3, 128, 4), (256, 3, 64, 4), (256, 5, 8, 0),
                                      (96, 1, 64, 4), (64, 1, 64, 0), (128, 1, 128, 4), (64, 1, 192, 4), (33, 1, 8, 0))]


def sitepool_data(c):
    g = _gen(c.name)
    L = c.n_site * c.site_len
    return (torch.randn(c.B, L, c.C, generator=g) + 0.25).to(BF), (torch.randn(c.B, c.n_site * c.C, generator=g) + 0.25).to(BF)


def check_sitepool_fwd(c, form, zbody, pooled):
    ref, mag = er.sitepool_fwd(zbody, c.site_len)
    if c.site_len == 1:
        exact(c.name, form, "pooled", pooled.reshape(ref.shape), zbody.permute(0, 2, 1).reshape(ref.shape).contiguous())
    echeck(c.name, form, "pooled", BF, pooled.reshape(ref.shape), ref, MARGIN * (U_B + (c.site_len + 2) * U_F) * mag)


def check_sitepool_bwd(c, form, dpooled, dz):
    """dz [B][L + 2 halo][C]: the body against the reference, the halo rows exactly zero (halo 0: there are none)."""
    L = c.n_site * c.site_len
    ref, mag = er.sitepool_bwd(dpooled, L, c.C, c.site_len)
    echeck(c.name, form, "dz", BF, dz[:, c.halo:c.halo + L], ref, MARGIN * (U_B + 2 * U_F) * mag)
    if c.halo:
        h = torch.cat((dz[:, :c.halo], dz[:, c.halo + L:]), 1)
        exact(c.name, form, "dz halo rows", h, torch.zeros_like(h))


@pytest.mark.parametrize("c", SITEPOOL, ids=[c.name for c in SITEPOOL])
def test_cnn_sitepool(c):
    Lb, ok, stream, DT, _ = _lib()
    zb, dp = sitepool_data(c)
    L = c.n_site * c.site_len
    z = torch.full((c.B, L + 2 * c.halo, c.C), float("nan"), dtype=BF)                  # halo rows are never read by the forward
    z[:, c.halo:c.halo + L] = zb
    z, dp = placed(z.to(DEV)), placed(dp.to(DEV))
    tv = c.form == "transpose_view_kernel"

    def fwd():
        out = Out((c.B, c.n_site * c.C), BF)
        ok(Lb.dl_cnn_sitepool_fwd(z.data_ptr(), out.v.data_ptr(), c.B, L, c.C, c.halo, c.site_len, DT[BF], stream), "dl_cnn_sitepool_fwd")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    def bwd():
        out = Out((c.B, L + 2 * c.halo, c.C), BF)
        ok(Lb.dl_cnn_sitepool_bwd(dp.data_ptr(), out.v.data_ptr(), c.B, L, c.C, c.halo, c.site_len, DT[BF], stream), "dl_cnn_sitepool_bwd")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    a, b = fwd(), fwd()
    same_bits(c.name, a, b)
    check_sitepool_fwd(c, "transpose_view_kernel" if tv else "cnn_sitepool_fwd_kernel<bf16>", z[:, c.halo:c.halo + L], a[0].v)
    a, b = bwd(), bwd()
    same_bits(c.name, a, b)
    check_sitepool_bwd(c, "transpose_view_kernel" if tv else "cnn_sitepool_bwd_kernel<bf16>", dp, a[0].v)


# ---- site pooling through the row tables of the compact layout (host tables of druglamp_amd.protein_plan) ------------------------
RowsPool = collections.namedtuple("RowsPool", "name form lengths L site_len C")
ROWS_BUCKET = 256


def _rows_form(C, n_site):
    return "cnn_sitepool_fwd_kernel<bf16> through row_of | cnn_sitepool_rows_bwd_kernel<%s>" % ("128, 256" if C == 128 and n_site == 256 else "0, 0")


ROWSPOOL = [RowsPool("rowspool_B%d_L%d_sl%d_C%d" % (len(ln), L, sl, C), _rows_form(C, L // sl), ln, L, sl, C) for (ln, L, sl, C) in (
    ((100, 300, 700), 768, 3, 128),                          # <128, 256>, 16 slices; deep tails of 39 and 149 positions, one plain sample
    (tuple((88, 98, 48, 200, 30, 120)[i % 6] for i in range(128)), 256, 1, 128),          # <128, 256>, B = 128: 4 slices
    (tuple((88, 98, 48, 200, 30, 60)[i % 6] for i in range(32)), 256, 1, 8),              # <0, 0>, B = 32: 8 slices
    ((68, 58, 150), 192, 3, 64))]                            # <0, 0>, 16 slices


def rows_slices(B):
    return 4 if B >= 128 else (8 if B >= 32 else 16)


def rowspool_plan(c):
    from druglamp_amd.protein_plan import ProteinPlan
    return ProteinPlan(c.lengths, c.L, bucket=ROWS_BUCKET)


def rowspool_data(c, plan):
    """z [R][C] compact rows (NaN in every row no position maps to: halo, context and padding rows are never read) and
    dpooled [B][n_site C]."""
    g = _gen(c.name)
    z = (torch.randn(plan.rows, c.C, generator=g) + 0.25).to(BF)
    used = torch.zeros(plan.rows, dtype=torch.bool)
    used[torch.from_numpy(plan.row_of).long()] = True
    z[~used] = float("nan")
    return z, (torch.randn(len(c.lengths), (c.L // c.site_len) * c.C, generator=g) + 0.25).to(BF)


def check_rowspool_fwd(c, z, row_of, pooled):
    B = len(c.lengths)
    body = z[row_of.long()].reshape(B, c.L, c.C)
    ref, mag = er.sitepool_fwd(body, c.site_len)
    echeck(c.name, "cnn_sitepool_fwd_kernel<bf16> through row_of", "pooled", BF, pooled, ref, MARGIN * (U_B + (c.site_len + 2) * U_F) * mag)


def check_rowspool_bwd(c, dpooled, rep, dz):
    B = len(c.lengths)
    body, _ = er.sitepool_bwd(dpooled, c.L, c.C, c.site_len)
    ref, mag = er.rows_sum_strided(body.reshape(B * c.L, c.C), rep)
    cnt = rep[:, 2].double()[:, None]
    form = c.form.split(" | ")[1]
    echeck(c.name, form, "dz", BF, dz, ref, MARGIN * ((cnt + 2) * U_F * mag + U_B * ref.abs()))
    exact(c.name, form, "dz rows of count 0", dz[rep[:, 2] == 0], torch.zeros_like(dz[rep[:, 2] == 0]))


@pytest.mark.parametrize("c", ROWSPOOL, ids=[c.name for c in ROWSPOOL])
def test_cnn_sitepool_rows(c):
    Lb, ok, stream, DT, _ = _lib()
    plan = rowspool_plan(c)
    z, dp = rowspool_data(c, plan)
    z, dp = placed(z.to(DEV)), placed(dp.to(DEV))
    row_of, rep = table(torch.from_numpy(plan.row_of)), table(torch.from_numpy(plan.rep))
    B, R = len(c.lengths), plan.rows

    def fwd():
        out = Out((B, (c.L // c.site_len) * c.C), BF)
        ok(Lb.dl_cnn_sitepool_rows_fwd(z.data_ptr(), row_of.data_ptr(), out.v.data_ptr(), B, c.L, c.C, c.site_len, DT[BF], stream),
           "dl_cnn_sitepool_rows_fwd")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    def bwd():
        out = Out((R, c.C), BF)
        ok(Lb.dl_cnn_sitepool_rows_bwd(dp.data_ptr(), rep.data_ptr(), row_of.data_ptr(), out.v.data_ptr(), B, c.L, c.C, R, c.site_len, DT[BF],
                                       stream), "dl_cnn_sitepool_rows_bwd")
        torch.cuda.synchronize()
        return (out.done(c.name),)

    a, b = fwd(), fwd()
    same_bits(c.name, a, b)
    check_rowspool_fwd(c, z, row_of, a[0].v)
    a, b = bwd(), bwd()
    same_bits(c.name, a, b)
    check_rowspool_bwd(c, dp, rep, a[0].v)


ALL_CASES = (GATE_FWD + GATE_BWD + ROWMOD + DROP_APPLY + GELU + DPRE + FILL_POOL + ROWMOD_SUM + ADAMW + CAST + NORM_ADJ + AGG + GATHER +
             EMBED + MOVERS + ROWS_SUM + WPREP + SITEPOOL + ROWSPOOL)
