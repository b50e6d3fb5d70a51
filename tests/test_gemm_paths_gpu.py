"""Every launch form of dl_gemm / dl_gemm_pair / dl_gemm_group / dl_colsum (csrc/gemm.hip, csrc/gemm_big.cuh) element-wise
against the fp64 reference of tests/gemm_ref.py:

    |got - ref| <= bound     for every element of C, pre_out and x_colsum (no sampling),

one parametrised case per row of CASES (dl_colsum: COLSUM_CASES).  Every row names the launch form it selects in the short
text of gemm_ref.select(), the Python mirror of the host dispatch; tests/test_gemm_reference_cpu.py asserts that the text
is what the dispatch rules give, asserts the mirror against the library where the library answers on the host, and checks
the data conditions below without a GPU.  The table is ordered by kernel family.

Buffers.  Every operand (X, W, bias, residual, dact_pre) lies inside a larger NaN-filled allocation: guard bands before and
after, NaN in every pitch gap (ldx > K, ldw > K, ldr > N, lddp > N) — a stray read poisons the result instead of faulting.
Every output is a row slice of a larger pitched buffer (ldc > N, rows before and after) filled with NaN: everything outside
[M, N] must be bitwise unchanged, everything inside overwritten (finite; `accumulate` starts from finite old values).
Every case runs twice and must be bitwise repeatable.  Dropout cases compare with the integer-exact mask of
gemm_ref.keep_mask, so one wrong keep decision is an error of the size of the element.

Form text
  k128 <in>><out> X<xs>W<ws> dma|reg epi<E> [sp<S> tw<T> [cs] reduce<out>]
                      gemm_kernel<T, TO, XS, WS, SPLIT, DMA, EPI, TW, CS>: 128 x 128 tiles (TW 4) or 64 x 64 (TW 2), LDS-DMA staging
                      when K is whole 128-byte steps, register staging otherwise (register staging keeps EPI 0 and 1 only);
                      split-K slabs + splitk_reduce_kernel<TO>; cs = x_colsum rides along
  big256 epi<E>       gemm_big_kernel<8, 2, 4, 128, 2, E>: 256 x 256 tiles, persistent, one workgroup per CU
  lat128 epi<E>       gemm_big_kernel<4, 2, 2, 128, 4, E>: 128 x 128 tiles, four-stage ring (few-tile form)
  tt2 bm<B> sp<S> [cs] gemm_big_tt2_kernel, 256- or 128-row tiles, slabs + splitk_reduce_kernel
  group bm<B>         dl_gemm_group: gemm_big_tt2_kernel<..., GROUP> over several weight gradients, one dl_reduce_batch
  pair ...            dl_gemm_pair sharing one gemm_kernel launch (nprob = 2)

Rounding bound (first order; U_F = 2^-24, U_B = 2^-8, round to nearest; one ulp = 2 U).  The reference reads the kernel's own
operands, so every error is the kernel's rounding.  S = sum_k |X||W| per output element.
  accumulation   e = (K + splits + 2) 2 U_F S.  bf16 products are exact in fp32, fp32 products round once; every add is counted
                 at one whole ulp because MFMA-internal adds need not round to nearest; `splits` adds for the slab reduction.
  bias           + U_F |pre|.  pre_out: e + U_st |pre| (U_st = U_B for bf16 storage, U_F for fp32).
  activation     ReLU: Lipschitz 1, the maximum is exact for numbers, and it KEEPS a NaN or +inf of the pre-activation (max_keep_nan,
                 common.cuh; -inf gives 0): tests/test_nonfinite_paths_gpu.py.  GELU: Lipschitz 1.13, so e <- 1.13 e, plus 4 U_F |gelu| for the erff forms
                 (the cancellation in 1 + erf for negative arguments costs at most U_F |pre| <= U_F (S + |bias|), which the
                 accumulation term holds several times over), plus the documented absolute 7.1e-5 of gelu_fast2 in the bf16
                 specialised epilogues (|pre| <= 12, asserted on the data).
  gelu'          v = act g: e <- e |g| + |act| e_g + U_F |v|, e_g = 8 U_F (erff / expf forms) plus the documented 1.0e-4 of
                 gelu_grad_fast2 in the bf16 specialised epilogue (|dact_pre| <= 5.5, asserted).
  residual, old C  + U_F (|v| + |added|) each.
  dropout        the mask is exact; the scale 1 / (1 - p) is the reference's own fp32 value: e <- e / (1 - p) + U_F |v|.
  store          + U_st |C|.
  x_colsum       (K + splits + 2) 2 U_F sum_k |X|.     dl_colsum: (rows per lane + 4 + chunks + 1) 2 U_F sum_m |X| from its plan.
Long contractions.  The accumulation term grows with K S while |acc| grows with sqrt(K): at K = 262147 the bound is several times
|acc| and would pass a missing slab or a misread tail step.  The weight-gradient tile kernels (tt2, group) therefore run on
integer operands in [-2, 2]: every product and every partial sum is an integer below S <= 4 K < 2^24, so fp32 accumulation is
exact in any order and under any rounding mode, and besides the bound the outputs must EQUAL the reference (rounded once to the
output type).  Their operands' guard rows reach one k-step (64 rows) past the last row: a tail step that is not fed from the
zero page reads NaN.
bound = MARGIN x the sum, MARGIN = 2: a recorded worst ratio at or below 1 / MARGIN says a form stays inside the first-order
model.  The two polynomial constants are the kernels' own documented errors: the test holds the kernels to them.
Scale bias, per output: bf16 store roundings are zero-mean, only the fp32-level part of the bound (`coherent`) can move an
output coherently: the least-squares scale s = sum (got - ref) ref / sum ref^2 must stay within sum coherent |ref| / sum ref^2
plus six standard deviations of zero-mean errors of the remaining size.
Floors.  The two polynomial constants are absolute, so where |C| is tiny they are the whole bound and the case would say nothing
about the relative terms.  GELU has such outputs by nature (against the bf16 store term U_B |C| the 7.1e-5 wins where
|gelu| < 7.1e-5 / U_B = 0.018: pre-activations next to zero or below about -2.7), so the condition cannot be "none", and dropped
elements (bound and floor both zero) count as not dominated.  conditions() calls an output
floor-dominated when the polynomial's term is more than half of its bound, i.e. larger than all rounding terms together, and
requires fewer than a quarter of a case's outputs to be so: at least three quarters of every case are then judged mainly by the
rounding terms, and the pre_out / epi0 / epi3 / epi5 outputs, which have no floor, always are.

DL_GEMM_BOUND_LOG=<file>: every check appends one JSON line (case, form, output, worst |err| / bound, MARGIN);
tools/gemm_bound_margins.py reduces the log to profiles/gemm_bound_margins.txt.
"""
import ctypes as C
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U_B, U_F, MARGIN = 2.0 ** -8, 2.0 ** -24, 2.0
GELU_POLY, GRAD_POLY = 7.1e-5, 1.0e-4        # documented at gelu_fast2 / gelu_grad_fast2 (csrc/common.cuh)
PRE_MAX, DPRE_MAX = 12.0, 5.5                # the intervals those two figures are documented for
SEED_OFFSET = 0x1234567


# ---- the table ----------------------------------------------------------------------------------------------------------------
def G(name, form, M, N, K, **kw):
    """One product.  bf_in / bf_out: bf16 operands / output; xs / ws: K-slow X / W; ldx / ldw: pitches (None: the natural one
    + 8); bias, pre (pre_out), dact (dact_pre): presence; act; res: None | 'after' | 'before'; rmod: res_row_mod; p: dropout;
    acc: accumulate; split: split_k; cs: x_colsum; algo; dyn: dynamic tile tickets; soff: device seed offset on; deferred: run
    inside deferred_reductions(); exact: integer operands in [-2, 2] (see the header: long contractions)."""
    c = types.SimpleNamespace(name=name, form=form, M=M, N=N, K=K, bf_in=True, bf_out=None, xs=0, ws=0, ldx=None, ldw=None,
                              bias=False, act=0, pre=False, dact=False, res=None, rmod=0, p=0.0, acc=False, split=-1, cs=False,
                              algo=0, dyn=False, soff=False, deferred=False, exact=False, kind="gemm", seed=0)
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    if c.bf_out is None:
        c.bf_out = c.bf_in
    if c.ldx is None:
        c.ldx = (M if c.xs else K) + 8
    if c.ldw is None:
        c.ldw = (N if c.ws else K) + 8
    return c


def _epi_kw(epi, p=0.0):
    return {0: dict(bias=True), 2: dict(bias=True, act=1, pre=True, p=p), 3: dict(bias=True, res="after", p=p),
            4: dict(dact=True, p=p), 5: dict(bias=True, act=2)}[epi]


def _cases():
    cs = []
    f32 = dict(bf_in=False)
    # ---- gemm_kernel, not split, LDS-DMA staging ---------------------------------------------------------------------------
    cs.append(G("k_bf_epi0_one_tile", "k128 bf16>bf16 X0W0 dma epi0", 128, 128, 64, bias=True))
    cs.append(G("k_bf_epi2_m1", "k128 bf16>bf16 X0W0 dma epi2", 1, 136, 64, **_epi_kw(2, 0.1)))
    cs.append(G("k_bf_epi0_nobias", "k128 bf16>bf16 X0W0 dma epi0", 200, 136, 64))
    cs.append(G("k_bf_epi2", "k128 bf16>bf16 X0W0 dma epi2", 200, 136, 64, **_epi_kw(2, 0.1)))
    cs.append(G("k_bf_epi3", "k128 bf16>bf16 X0W0 dma epi3", 130, 264, 192, **_epi_kw(3, 0.37)))
    cs.append(G("k_bf_epi4", "k128 bf16>bf16 X0W0 dma epi4", 200, 136, 64, **_epi_kw(4, 0.1)))
    cs.append(G("k_bf_epi5", "k128 bf16>bf16 X0W0 dma epi5", 130, 264, 192, **_epi_kw(5)))
    cs.append(G("k_bf_f32out_epi0", "k128 bf16>f32 X0W0 dma epi0", 200, 136, 64, bias=True, bf_out=False))
    cs.append(G("k_f32_epi0", "k128 f32>f32 X0W0 dma epi0", 200, 136, 64, bias=True, **f32))
    cs.append(G("k_f32_epi2", "k128 f32>f32 X0W0 dma epi2", 130, 264, 192, **_epi_kw(2, 0.1), **f32))
    cs.append(G("k_f32_epi3", "k128 f32>f32 X0W0 dma epi3", 200, 136, 64, **_epi_kw(3, 0.37), **f32))
    cs.append(G("k_f32_epi4", "k128 f32>f32 X0W0 dma epi4", 130, 264, 192, **_epi_kw(4, 0.1), **f32))
    cs.append(G("k_f32_epi5", "k128 f32>f32 X0W0 dma epi5", 200, 136, 64, **_epi_kw(5), **f32))
    # EPI 1 by each trigger
    cs.append(G("k_bf_epi1_n36", "k128 bf16>bf16 X0W0 dma epi1", 200, 36, 64, bias=True, act=1, pre=True))
    cs.append(G("k_f32_epi1_n130", "k128 f32>f32 X0W0 dma epi1", 130, 130, 64, bias=True, res="after", **f32))
    cs.append(G("k_bf_epi1_accumulate", "k128 bf16>f32 X0W0 dma epi1", 200, 136, 64, bias=True, acc=True, bf_out=False))
    cs.append(G("k_bf_epi1_rowmod", "k128 bf16>bf16 X0W0 dma epi1", 200, 136, 64, res="after", rmod=50, p=0.1))
    cs.append(G("k_f32_epi1_res_before", "k128 f32>f32 X0W0 dma epi1", 130, 264, 192, bias=True, res="before", p=0.37, **f32))
    cs.append(G("k_bf_epi1_relu_res", "k128 bf16>bf16 X0W0 dma epi1", 200, 136, 64, bias=True, act=2, res="after"))
    cs.append(G("k_bf_epi1_gelu_dact", "k128 bf16>bf16 X0W0 dma epi1", 130, 136, 64, bias=True, act=1, dact=True, p=0.1))
    # layouts
    cs.append(G("k_bf_x0w1_epi4", "k128 bf16>bf16 X0W1 dma epi4", 200, 136, 64, ws=1, **_epi_kw(4, 0.1)))
    cs.append(G("k_bf_x1w1_epi0", "k128 bf16>f32 X1W1 dma epi0", 200, 136, 64, xs=1, ws=1, bf_out=False))
    cs.append(G("k_f32_x0w1_epi0", "k128 f32>f32 X0W1 dma epi0", 130, 264, 96, ws=1, bias=True, **f32))
    cs.append(G("k_f32_x1w1_epi1", "k128 f32>f32 X1W1 dma epi1", 132, 136, 64, xs=1, ws=1, acc=True, **f32))
    # 58 x 9 = 522 tiles on 512 workgroups: ten workgroups walk a second tile (next-tile prefetch, the LDS aliasing barrier)
    cs.append(G("k_bf_epi3_two_rounds", "k128 bf16>bf16 X0W0 dma epi3", 7300, 1032, 64, **_epi_kw(3, 0.1)))
    # ---- gemm_kernel, register staging (K is not whole steps) --------------------------------------------------------------
    cs.append(G("r_bf_x0w0_epi0", "k128 bf16>bf16 X0W0 reg epi0", 200, 136, 72, bias=True))
    cs.append(G("r_bf_x0w0_epi1", "k128 bf16>bf16 X0W0 reg epi1", 130, 264, 200, **_epi_kw(2, 0.1)))
    cs.append(G("r_bf_x0w1_epi1", "k128 bf16>bf16 X0W1 reg epi1", 200, 136, 72, ws=1, **_epi_kw(4, 0.37)))
    cs.append(G("r_bf_x1w1_epi0", "k128 bf16>f32 X1W1 reg epi0", 136, 264, 200, xs=1, ws=1, bf_out=False))
    cs.append(G("r_f32_x0w0_epi1", "k128 f32>f32 X0W0 reg epi1", 130, 130, 36, bias=True, act=2, **f32))
    cs.append(G("r_f32_x0w1_epi0", "k128 f32>f32 X0W1 reg epi0", 200, 136, 36, ws=1, bias=True, **f32))
    cs.append(G("r_f32_x1w1_epi1", "k128 f32>f32 X1W1 reg epi1", 132, 136, 36, xs=1, ws=1, acc=True, **f32))
    # ---- the operand layouts of the model ----------------------------------------------------------------------------------
    cs.append(G("conv_dma_ldx64_k192", "k128 bf16>bf16 X0W0 dma epi5", 200, 136, 192, ldx=64, **_epi_kw(5)))
    cs.append(G("conv_reg_ldx40_k120", "k128 bf16>bf16 X0W0 reg epi1", 200, 136, 120, ldx=40, **_epi_kw(5)))
    cs.append(G("inproj_ldw_3e", "k128 bf16>bf16 X0W0 dma epi0", 200, 136, 64, ldw=192, bias=True))
    cs.append(G("dgrad_w1_ldw_3e", "k128 bf16>bf16 X0W1 reg epi0", 130, 64, 200, ws=1, ldw=192))
    # ---- split-K slabs -----------------------------------------------------------------------------------------------------
    cs.append(G("s_f32_split3", "k128 f32>f32 X0W0 dma epi1 sp3 tw4 reduce<f32>", 130, 136, 224, split=3, **f32))
    cs.append(G("s_bf_trim8to3", "k128 bf16>f32 X0W0 dma epi1 sp3 tw4 reduce<f32>", 130, 136, 192, split=8, bf_out=False))
    cs.append(G("s_bf_bf16out_split2", "k128 bf16>f32 X0W0 dma epi1 sp2 tw4 reduce<bf16>", 130, 136, 256, split=2))
    cs.append(G("s_bf_auto_tw2", "k128 bf16>f32 X1W1 dma epi1 sp4 tw2 reduce<f32>", 64, 128, 1024, xs=1, ws=1, split=0, bf_out=False))
    cs.append(G("s_bf_auto_tw2_cs", "k128 bf16>f32 X1W1 dma epi1 sp4 tw2 cs reduce<f32>", 72, 136, 1024, xs=1, ws=1, split=0, cs=True,
                bf_out=False))
    cs.append(G("s_bf_auto_tw4_cs_tail", "k128 bf16>f32 X1W1 reg epi1 sp4 tw4 cs reduce<f32>", 200, 136, 1000, xs=1, ws=1, split=0,
                cs=True, bf_out=False))
    cs.append(G("s_f32_reg_accumulate", "k128 f32>f32 X1W1 reg epi1 sp4 tw4 reduce<f32>", 132, 136, 100, xs=1, ws=1, split=4, acc=True,
                **f32))
    cs.append(G("s_f32_auto_tw2", "k128 f32>f32 X1W1 dma epi1 sp4 tw2 reduce<f32>", 64, 68, 512, xs=1, ws=1, split=0, **f32))
    cs.append(G("s_bf_deferred_cs", "k128 bf16>f32 X1W1 dma epi1 sp4 tw2 cs reduce<f32>", 72, 136, 1024, xs=1, ws=1, split=0, cs=True,
                bf_out=False, deferred=True))
    # ---- gemm_big_kernel, 256 x 256 ----------------------------------------------------------------------------------------
    for epi, p in ((0, 0.0), (2, 0.1), (3, 0.37), (4, 0.1), (5, 0.0)):
        # 192 x 1 tiles: the fewest that are eligible; one k-step; last row tile 1 row, column tile 136 wide
        cs.append(G("big_epi%d_192tiles" % epi, "big256 epi%d" % epi, 48897, 136, 64, **_epi_kw(epi, p)))
    for epi, p in ((0, 0.0), (2, 0.37), (3, 0.1), (4, 0.37), (5, 0.0)):
        # 130 x 2 = 260 tiles on 256 workgroups: four take a second tile; last column tile 8 wide
        cs.append(G("big_epi%d_260tiles" % epi, "big256 epi%d" % epi, 33032, 264, 192, **_epi_kw(epi, p)))
    cs.append(G("big_epi3_tickets_seed_offset", "big256 epi3", 33032, 264, 192, dyn=True, soff=True, **_epi_kw(3, 0.1)))
    # ---- gemm_big_kernel, few-tile 128 x 128 deep ring ---------------------------------------------------------------------
    for epi, p in ((0, 0.0), (2, 0.1), (3, 0.37), (4, 0.1), (5, 0.0)):
        cs.append(G("lat_epi%d_8x128" % epi, "lat128 epi%d" % epi, 8, 128, 512, **_epi_kw(epi, p)))
        cs.append(G("lat_epi%d_130x136" % epi, "lat128 epi%d" % epi, 130, 136, 576, **_epi_kw(epi, p)))
    # ---- gemm_big_tt2_kernel -----------------------------------------------------------------------------------------------
    tt = dict(xs=1, ws=1, split=0, exact=True)
    cs.append(G("tt256_f32", "tt2 bm256 sp13 reduce<f32>", 1280, 512, 4100, bf_out=False, **tt))
    cs.append(G("tt256_bf16out_cs", "tt2 bm256 sp13 cs reduce<bf16>", 1280, 512, 4100, cs=True, **tt))
    cs.append(G("tt128_f32_cs", "tt2 bm128 sp84 cs reduce<f32>", 96, 640, 262147, cs=True, bf_out=False, **tt))
    cs.append(G("tt128_bf16out", "tt2 bm128 sp84 reduce<bf16>", 96, 640, 262147, **tt))
    # ---- dl_gemm_group through ops.flush_wgrads ----------------------------------------------------------------------------
    m = lambda n, M, N, K, cs_: G(n, "group", M, N, K, xs=1, ws=1, split=0, cs=cs_, bf_out=False, exact=True)
    cs.append(types.SimpleNamespace(name="group_bm128_mixed", form="group bm128 sp2,2,2", kind="group", members=[
        m("g0", 128, 136, 1000, True), m("g1", 64, 256, 1024, False), m("g2", 200, 72, 2048, True)]))
    cs.append(types.SimpleNamespace(name="group_bm256", form="group bm256 sp22,22", kind="group", members=[
        m("g0", 1280, 512, 16384, False), m("g1", 256, 256, 16392, True)]))
    # ---- dl_gemm_pair, one shared launch -----------------------------------------------------------------------------------
    cs.append(types.SimpleNamespace(name="pair_f32_epi1", form="pair k128 f32>f32 X0W0 dma epi1", kind="pair", members=[
        G("p%d" % i, "", 130, 136, 64, bias=True, res="before", p=0.1, **f32) for i in range(2)]))
    cs.append(types.SimpleNamespace(name="pair_bf_epi2", form="pair k128 bf16>bf16 X0W0 dma epi2", kind="pair", members=[
        G("p%d" % i, "", 200, 136, 64, **_epi_kw(2, 0.37)) for i in range(2)]))
    k = 0
    for c in cs:
        for q in getattr(c, "members", [c]):
            q.seed = 1000 + k
            k += 1
    return cs


CASES = _cases()
# dl_colsum: (name, bf16, M, N, ldx, accumulate)
COLSUM_CASES = [("cs_f32_m1", False, 1, 136, 144, False), ("cs_bf_m1_acc", True, 1, 64, 72, True),
                ("cs_f32_scalar_ld41", False, 130, 37, 41, False), ("cs_bf_scalar_ld41_acc", True, 200, 37, 41, True),
                ("cs_f32_thousands_acc", False, 5000, 264, 272, True), ("cs_bf_thousands", True, 7300, 520, 528, False)]


# ---- data (no GPU needed: tests/test_gemm_reference_cpu.py checks the conditions on it) ----------------------------------------
BIG_OPERAND = 1 << 24


def gen(c, big_dev=None):
    """The logical operands of case c in their storage dtype, on the CPU.  X / W: storage-shaped 2-D [rows][cols], or 1-D
    where the rows overlap (pitch < row length).  Operands of more than BIG_OPERAND elements (plain weight-gradient
    products only: no condition depends on their values) are drawn on `big_dev` when one is given."""
    g = torch.Generator().manual_seed(c.seed)
    dt = BF if c.bf_in else F32

    def mat(rows, cols, ld, scale):
        n = (rows, cols) if ld >= cols else ((rows - 1) * ld + cols,)
        gg, dev = g, "cpu"
        if big_dev is not None and rows * cols > BIG_OPERAND:
            assert R.plain(c)
            gg, dev = torch.Generator(device=big_dev).manual_seed(c.seed + (1 << 20) * cols), big_dev
        if c.exact:
            return torch.randint(-2, 3, n, generator=gg, device=dev).to(dt)
        return (torch.randn(*n, generator=gg, device=dev) * scale).to(dt)

    d = {"X": mat(*((c.K, c.M) if c.xs else (c.M, c.K)), c.ldx, 1.0),
         "W": mat(*((c.K, c.N) if c.ws else (c.N, c.K)), c.ldw, 1.2 / math.sqrt(c.K))}
    if c.bias:
        d["bias"] = torch.randn(c.N, generator=g) * 0.5
    if c.res:
        d["res"] = torch.randn(c.rmod or c.M, c.N, generator=g).to(dt)
    if c.dact:
        d["dact"] = (torch.randn(c.M, c.N, generator=g) * 1.5).clamp_(-5.0, 5.0).to(dt)
    if c.acc:
        d["old"] = torch.randn(c.M, c.N, generator=g).to(BF if c.bf_out else F32)
    return d


def storage_span(rows, cols, ld):
    return rows * ld if ld >= cols else (rows - 1) * ld + cols


def reference(c, flat_x, flat_w, d, dev, seed_offset=0):
    """gemm_ref.reference for case c: flat_x / flat_w are the storages from the base pointers, d the logical tensors."""
    X = R.operand(flat_x, c.M, c.K, c.ldx, c.xs)
    W = R.operand(flat_w, c.N, c.K, c.ldw, c.ws)
    f = lambda k: d[k].to(dev).to(F64) if k in d else None
    keep = torch.from_numpy(R.keep_mask(c.seed, seed_offset, c.M, c.N, c.p)).to(dev) if c.p > 0 else None
    return R.reference(X, W, bias=f("bias"), act=c.act, dact_pre=f("dact"), residual=f("res"), res_row_mod=c.rmod,
                       res_before_dropout=c.res == "before", keep=keep, keep_scale=R.inv_keep(c.p) if c.p > 0 else 1.0,
                       old_c=f("old"), want_colsum=c.cs), keep


def poly_form(c, form):
    """The bf16 specialised epilogues evaluate GELU / gelu' by polynomial."""
    return c.bf_in and ("epi2" in form or "epi4" in form)


def bounds(c, r, splits, poly, keep):
    """{output: (bound, coherent part)} from the header's first-order model."""
    st_in, st_out = (U_B if c.bf_in else U_F), (U_B if c.bf_out else U_F)
    out = {}
    e = (c.K + splits + 2) * 2 * U_F * r["S"]
    floor = torch.zeros_like(e)
    if c.bias:
        e = e + U_F * r["pre"].abs()
    if c.pre:
        out["pre_out"] = (MARGIN * (e + st_in * r["pre"].abs()), MARGIN * e)
    v = r["act"]
    if c.act == 1:
        floor = floor + (GELU_POLY if poly else 0.0)
        e = 1.13 * e + 4 * U_F * v.abs() + floor
    if c.dact:
        eg = 8 * U_F + (GRAD_POLY if poly else 0.0)
        floor = floor * r["g"].abs()
        e = e * r["g"].abs() + v.abs() * eg + U_F * (v * r["g"]).abs()
        v = v * r["g"]
    if c.res == "before":
        e = e + U_F * (v.abs() + r["res"].abs())
    if keep is not None:
        s = R.inv_keep(c.p)
        e = torch.where(keep, e * s + U_F * r["dropped"].abs(), torch.zeros_like(e))
        floor = torch.where(keep, floor * s, torch.zeros_like(e))
    if c.res == "after":
        e = e + U_F * (r["dropped"].abs() + r["res"].abs())
    if c.acc:
        e = e + U_F * (r["before_acc"].abs() + (r["C"] - r["before_acc"]).abs())
    out["C"] = (MARGIN * (e + st_out * r["C"].abs()), MARGIN * e)
    out["floor"] = MARGIN * floor
    if c.cs:
        b = MARGIN * (c.K + splits + 2) * 2 * U_F * r["x_colsum_mag"]
        out["x_colsum"] = (b, b)
    return out


def conditions(c, r, form, keep, d):
    """What the bound assumes about the data of case c; raises AssertionError."""
    poly = poly_form(c, form)
    if c.act == 1 and poly:
        assert float(r["pre"].abs().max()) <= PRE_MAX, "%s: |pre| leaves the interval of the documented GELU error" % c.name
    if c.dact and poly:
        assert float(d["dact"].abs().max()) <= DPRE_MAX, "%s: |dact_pre| leaves the interval of the documented gelu' error" % c.name
    b = bounds(c, r, 1, poly, keep)
    dom = (b["floor"] > 0.5 * b["C"][0]).double().mean()
    assert float(dom) < 0.25, "%s: the absolute term of the polynomial dominates the bound of %.0f %% of the outputs" % (c.name, 100 * float(dom))


# ---- device buffers -------------------------------------------------------------------------------------------------------------
GUARD = 256            # elements on both sides: a multiple of 16 bytes in every dtype
GUARD_ROWS = 64        # operands: plus this many whole NaN rows of the pitch before and after (one k-step of the deepest tile)


class Buf:
    """[rows_total][ld] elements between two guard bands, filled with NaN; `inner` is the addressed [M][N] at row0."""

    @staticmethod
    def out_lead(row0, ld):
        """Elements from the allocation's start to an output's first addressed element."""
        return GUARD + row0 * ld

    @staticmethod
    def operand_lead(ld):
        """Elements from the allocation's start to an operand's base pointer."""
        return GUARD + GUARD_ROWS * ld

    def __init__(self, rows, cols, ld, dt, row0=0, extra_rows=0, dev=DEV):
        self.span = (rows + extra_rows) * ld
        self.t = torch.full((self.span + 2 * GUARD,), float("nan"), dtype=dt, device=dev)
        self.off = self.out_lead(row0, ld)
        self.inner = torch.as_strided(self.t, (rows, cols), (ld, 1), self.off)
        self.mask = torch.zeros_like(self.t, dtype=torch.bool)
        torch.as_strided(self.mask, (rows, cols), (ld, 1), self.off).fill_(True)
        self.ld, self.old = ld, None

    @classmethod
    def operand(cls, t, rows, cols, ld, dev=DEV):
        """Storage-shaped t ([rows][cols], or 1-D for overlapping rows) placed at pitch ld."""
        b = cls.__new__(cls)
        b.span = storage_span(rows, cols, ld)
        lead = cls.operand_lead(ld)
        b.t = torch.full((b.span + 2 * lead,), float("nan"), dtype=t.dtype, device=dev)
        if t.dim() == 1:
            b.t[lead:lead + b.span] = t.to(dev)
        else:
            torch.as_strided(b.t, (rows, cols), (ld, 1), lead).copy_(t.to(dev))
        b.flat = b.t[lead:]
        return b

    def refill(self):
        self.t.fill_(float("nan"))
        if self.old is not None:
            self.inner.copy_(self.old)

    def bits(self):
        return self.t.view({2: torch.int16, 4: torch.int32}[self.t.element_size()]).clone()

    def untouched(self, what):
        fresh = torch.full((1,), float("nan"), dtype=self.t.dtype, device=self.t.device).view(self.bits().dtype)
        assert bool((self.bits()[~self.mask] == fresh).all()), "%s was written outside its addressed elements" % what


def _log(case, form, what, ratio):
    path = os.environ.get("DL_GEMM_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "form": form, "output": what, "ratio": ratio, "margin": MARGIN}) + "\n")


def check(case, form, what, got, ref, bound, coherent):
    got = got.to(F64)
    assert got.shape == ref.shape
    assert bool(torch.isfinite(got).all()), "%s: %s has elements that were not written, or NaN from a stray read" % (case, what)
    err = got - ref
    ratio = float((err.abs() / (bound + 1e-300)).max())
    _log(case, form, what, ratio)
    print("%s [%s] %s: worst |err| / bound = %.4f" % (case, form, what, ratio))
    assert ratio <= 1.0, "%s [%s]: %s exceeds its rounding bound by x%.3g" % (case, form, what, ratio)
    den = float((ref * ref).sum())
    if den > 0:
        s = float((err * ref).sum()) / den
        lim = (float((coherent * ref.abs()).sum()) + 6.0 * float((((bound - coherent) * ref) ** 2).sum().sqrt()) / math.sqrt(3.0)) / den
        _log(case, form, what + " bias", abs(s) / lim)
        assert abs(s) <= lim, "%s [%s]: %s carries a scale error of %.3g (allowed %.3g)" % (case, form, what, s, lim)


class Prob:
    """The device side of one product: guarded operands, guarded outputs, the dl_gemm_args keywords."""

    def __init__(self, c):
        from druglamp_amd import ops
        self.c, self.d = c, gen(c, DEV)
        d, dt = self.d, (BF if c.bf_in else F32)
        self.X = Buf.operand(d["X"], *((c.K, c.M) if c.xs else (c.M, c.K)), c.ldx)
        self.W = Buf.operand(d["W"], *((c.K, c.N) if c.ws else (c.N, c.K)), c.ldw)
        pad = 8 if c.N % 4 == 0 else 5              # pitches keep the alignment the entry point asks for at this N, no more
        self.keep = []
        mk = lambda t, ld: Buf.operand(t, t.shape[0], t.shape[1], ld)
        self.kw = dict(M=c.M, N=c.N, K=c.K, x_kslow=bool(c.xs), w_kslow=bool(c.ws), ldx=c.ldx, ldw=c.ldw, act=c.act,
                       res_row_mod=c.rmod, res_before_dropout=c.res == "before", dropout_p=c.p, seed=c.seed, accumulate=c.acc,
                       split_k=c.split, algo=c.algo)
        if c.bias:
            b = Buf.operand(d["bias"][None, :], 1, c.N, c.N)
            self.keep.append(b)
            self.kw["bias"] = b.flat[:c.N]
        if c.res:
            b = mk(d["res"], c.N + pad)
            self.keep.append(b)
            self.kw["residual"] = torch.as_strided(b.flat, tuple(d["res"].shape), (c.N + pad, 1))
        self.lddp = c.N + pad
        if c.dact:
            b = mk(d["dact"], self.lddp)
            self.keep.append(b)
            self.kw["dact_pre"] = b.flat
        self.outs = {"C": Buf(c.M, c.N, c.N + pad, BF if c.bf_out else F32, row0=2, extra_rows=5)}
        if c.acc:
            self.outs["C"].old = d["old"].to(DEV)
        self.kw["out"] = self.outs["C"].inner
        if c.pre:
            self.outs["pre_out"] = Buf(c.M, c.N, c.N + pad, dt, row0=1, extra_rows=3)
            self.kw["pre_out"] = self.outs["pre_out"].inner
        if c.cs:
            self.outs["x_colsum"] = Buf(1, c.M, c.M, F32)
            self.kw["x_colsum"] = self.outs["x_colsum"].inner[0]
        self.x, self.w = self.X.flat, self.W.flat
        self.ops = ops

    def args(self):
        a, out = self.ops._gemm_args(self.x, self.w, **self.kw)
        a.ldp, a.lddp = (self.outs["pre_out"].ld if "pre_out" in self.outs else self.c.N), self.lddp
        return a, out

    def launch(self):
        a, out = self.args()
        self.ops._gemm_launch(a, out, self.x, self.c.acc, self.kw.get("x_colsum"))

    def verify(self, case, form, splits, seed_offset=0):
        c = self.c
        r, keep = reference(c, self.x, self.w, self.d, DEV, seed_offset)
        conditions(c, r, form, keep, self.d)
        b = bounds(c, r, splits, poly_form(c, form), keep)
        for what, buf in self.outs.items():
            ref = {"C": r["C"], "pre_out": r["pre"], "x_colsum": r["x_colsum"][None, :] if c.cs else None}[what]
            bd, co = b[what]
            check(case, form, what, buf.inner, ref, bd.reshape(ref.shape), co.reshape(ref.shape))
            if c.exact:
                assert float(r["S"].max()) < 2.0 ** 24 and R.plain(c)
                want = ref.to(buf.inner.dtype)
                assert torch.equal(buf.inner, want), "%s: %s differs from the exact result in %d elements" % (case, what, int((buf.inner != want).sum()))


def _twice(case, probs, launch):
    snaps = []
    for _ in range(2):
        for p in probs:
            for b in p.outs.values():
                b.refill()
        launch()
        torch.cuda.synchronize()
        for p in probs:
            for what, b in p.outs.items():
                b.untouched("%s: %s" % (case, what))
        snaps.append([b.bits() for p in probs for b in p.outs.values()])
    for x, y in zip(*snaps):
        assert torch.equal(x, y), "%s is not bitwise repeatable" % case


PAIR_EQUAL = ("M", "N", "K", "ldx", "ldw", "ldc", "x_kslow", "w_kslow", "in_dtype", "out_dtype", "ldr", "res_row_mod", "res_before_dropout",
              "act", "ldp", "lddp", "dropout_p", "accumulate", "split_k", "algo", "dropout_seed_offset", "tile_tickets")
PAIR_POINTERS = ("X", "W", "C", "bias", "residual", "pre_out", "dact_pre")


def assert_twin(a, b):
    """dl_gemm_pair's own condition for sharing one launch, on the argument blocks it is given.  When it does not hold the
    entry point quietly runs two single launches, whose outputs are just as right: the pair cases would then pin nothing new."""
    for f in PAIR_EQUAL:
        assert getattr(a, f) == getattr(b, f), "pair members differ in %s" % f
    for f in PAIR_POINTERS:
        assert (getattr(a, f) is None) == (getattr(b, f) is None), "pair members differ in the presence of %s" % f
        assert (getattr(b, f) or 0) & 15 == 0, "the second member's %s is not 16-byte aligned" % f
    assert not a.x_colsum and not b.x_colsum and not a.deferred and not b.deferred


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_gemm_form(c):
    from druglamp_amd import _lib, ops
    members = getattr(c, "members", [c])
    probs = [Prob(q) for q in members]
    seed_offset = 0
    try:
        if c.kind == "gemm":
            p = probs[0]
            ops.dynamic_tiles(c.dyn)
            if c.soff:
                seed_offset = SEED_OFFSET
                ops.use_seed_offset(True)
                ops.seed_offset_tensor(torch.device(DEV)).fill_(seed_offset)
            if c.deferred:
                def launch():
                    with ops.deferred_reductions():
                        ops.gemm(p.x, p.w, **p.kw)
            else:
                launch = p.launch
            _twice(c.name, probs, launch)
            if c.dyn:
                torch.cuda.synchronize()
                assert int(ops._tickets[("cuda", 0)].abs().sum()) == 0, "the ticket words are not zero after the launch"
            p.verify(c.name, c.form, R.resolve_split(c), seed_offset)
        elif c.kind == "pair":
            def launch():
                (a0, _), (a1, _) = probs[0].args(), probs[1].args()
                assert_twin(a0, a1)
                _lib.check(_lib.lib().dl_gemm_pair(C.byref(a0), C.byref(a1), ops._stream()), "dl_gemm_pair")
            _twice(c.name, probs, launch)
            for p in probs:
                p.verify(c.name + "/" + p.c.name, c.form, 1)
        else:
            def launch():
                with ops.deferred_reductions():
                    for p in probs:
                        ops.gemm(p.x, p.w, **p.kw)
                    assert len(ops._wgroup) == len(probs), "the products did not queue up as a weight-gradient group"
            _twice(c.name, probs, launch)
            _, sp = R.group_plan([(q.M, q.N, q.K) for q in members])
            for p, s in zip(probs, sp):
                p.verify(c.name + "/" + p.c.name, c.form, s)
    finally:
        ops.dynamic_tiles(False)
        if seed_offset:
            ops.seed_offset_tensor(torch.device(DEV)).fill_(0)
        ops.use_seed_offset(False)


@pytest.mark.parametrize("case", COLSUM_CASES, ids=lambda t: t[0])
def test_colsum_form(case):
    from druglamp_amd import ops
    name, bf, M, N, ldx, acc = case
    g = torch.Generator().manual_seed(500 + [t[0] for t in COLSUM_CASES].index(name))
    x = torch.randn(M, N, generator=g).to(BF if bf else F32)
    old = torch.randn(N, generator=g)
    X = Buf.operand(x, M, N, ldx)
    out = Buf(1, N, N, F32)
    if acc:
        out.old = old.to(DEV)[None, :]
    prob = types.SimpleNamespace(outs={"out": out})
    xv = torch.as_strided(X.flat, (M, N), (ldx, 1))
    _twice(name, [prob], lambda: ops.colsum(xv, out=out.inner[0], accumulate=acc))
    ref, mag = R.colsum(xv.to(F64), old.to(DEV).to(F64) if acc else None)
    rows, chunks = R.colsum_plan(M, N)
    b = MARGIN * (rows // 4 + 4 + chunks + 1) * 2 * U_F * mag
    form = "colsum_partial<%s>%s" % ("bf16" if bf else "f32", " scalar" if N % 4 else "")
    check(name, form, "out", out.inner[0], ref, b, b)
