"""Every launch form of dl_bn_eval_bwd (bn_eval.hip: the backward of a BatchNorm on fixed statistics) through the C ABI,
element-wise against the fp64 reference of tests/bn_eval_ref.py:

    |got - ref| <= tau * mag          for every addressed element of dx and of the sums,

with the rounding model, the constants and the buffer discipline of tests/test_norm_paths_gpu.py (its `check`, `Guarded`
buffers, U_F / U_B, MARGIN = 2, KINK = 64 u_f, KINK_CAP = 1e-3 are imported, not restated):
  dx = g gamma rstd: the store's rounding and at most four fp32 roundings (xhat is not in it; gamma rstd, the product, the
      mask):                                                            (u_st + 4 u_f) |dx|
  sums = (sum g | sum g xhat) over R rows in fp32:                      (R + 6) u_f of the absolute sums
  relu_out: an element with |xhat gamma + beta| <= 64 u_f (|xhat gamma| + |beta|) may open on one side only; it is left out
      of dx's check and its |dz| (|dz xhat|) is added to the bounds of the sums; at most 1 element in 1000 per tensor.
      relu_in reads the operand y itself (y > 0): no kink.
Buffers: NaN everywhere outside the addressed elements, excluded / halo rows of dz and y included (a stray read poisons the
result); an addressed output element must be overwritten, everything else stay bitwise unchanged; excluded rows of dx are
exactly +0; every launch runs twice and must repeat bitwise.

Forms (host dispatch of dl_bn_eval_bwd)
  bf16, C in {64, 128, 256}, dz / y / dy 16-byte aligned -> bn_eval_bwd_wide_kernel<SUMS, RELU_OUT>; else
  bn_eval_bwd_kernel<T, SUMS>; 32 rows per workgroup at these sizes, partials [chunks][2][C] -> dl_reduce_partials_kernel
  (its four-way loop runs beyond 192 chunks: the r9000 cases).  sums == NULL: the dx pass alone, no workspace.
The cases and their data are built on the host (case_data) so that tests/test_bn_eval_reference_cpu.py can check the kink
share of every seed and run the checker on planted errors without a GPU.
"""
import collections

import pytest
import torch

from tests import bn_eval_ref as ber
from tests import norm_ref as nr
from tests.test_norm_paths_gpu import (BF, DEV, F32, F64, KINK, MARGIN, U_F, Guarded, _lib, _out, _ptr, check, check_zero_rows,
                                       tau_sum, u_st)

MASKS = ((0, 0), (1, 0), (0, 1))                   # (relu_in, relu_out): no mask, ProteinCNN's order, the SimSiam MLPs' order


# ---- the checker (plain tensors on any device) -----------------------------------------------------------------------------
def check_bn_eval(case, dt, dz, y, w, mean, rstd, gamma, beta, relu_in, relu_out, dx, sums):
    """dx [R][C] and sums [2C] (or None) of one launch against the fp64 reference."""
    R, C = y.shape
    rdx, rsums, m = ber.bn_eval_bwd(dz, y, w, mean, rstd, gamma, beta, relu_in, relu_out)
    b0, b1 = MARGIN * tau_sum(R) * m["s0"], MARGIN * tau_sum(R) * m["s1"]
    skip = None
    if relu_out:
        keep = w >= 0
        skip = nr.kink(m["pre"], m["pre_mag"], KINK) & keep[:, None]
        d, k = dz[keep].double().abs(), skip[keep]                 # the |dz| of the kink elements: they may count or not
        b0, b1 = b0 + (d * k).sum(0), b1 + (d * m["xhat_abs"][keep] * k).sum(0)
    coh = MARGIN * 4 * U_F * m["dx"]
    check(case, "dx", dt, dx, rdx, coh + MARGIN * u_st(dt) * m["dx"], coh, skip)
    check_zero_rows(case, "dx", dx, w < 0)
    if sums is not None:
        check(case, "sums s0", F32, sums[:C], rsums[:C], b0)
        check(case, "sums s1", F32, sums[C:], rsums[C:], b1)


# ---- cases -------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name wide dt C R rule off")


def _c(name, wide, dt, C, R=None, rule=("none",), off=0):
    if rule[0] == "win":
        R = rule[1] * rule[4]
    return Case(name, wide, dt, C, R, rule, off)


WIN = ("win", 40, 4, 30, 5)                        # windows of 40 rows: 4 halo rows, 30 valid, 6 excluded behind them; 5 windows
RW = ("rw",)                                       # row weights from {-1, 0, 1, 3}
CASES = [
    # wide form: R = 1, one short of / one past a workgroup's 32-row block, several partials, > 192 partials
    _c("wide128_r1", True, BF, 128, 1), _c("wide128_r31", True, BF, 128, 31), _c("wide128_r33", True, BF, 128, 33),
    _c("wide64_r100", True, BF, 64, 100), _c("wide256_r100", True, BF, 256, 100), _c("wide128_r9000", True, BF, 128, 9000),
    _c("wide128_win", True, BF, 128, rule=WIN), _c("wide64_win", True, BF, 64, rule=WIN), _c("wide256_rw_r333", True, BF, 256, 333, RW),
    _c("wide128_rw_r100", True, BF, 128, 100, RW),
    # generic form: another C, a base that is 8-byte but not 16-byte aligned, fp32
    _c("bf16_c40_r1", False, BF, 40, 1), _c("bf16_c40_r33", False, BF, 40, 33), _c("bf16_c40_win", False, BF, 40, rule=WIN),
    _c("bf16_c40_rw_r100", False, BF, 40, 100, RW), _c("bf16_c128_misaligned_r100", False, BF, 128, 100, off=4),
    _c("bf16_c128_misaligned_win", False, BF, 128, rule=WIN, off=4), _c("bf16_c260_r9000", False, BF, 260, 9000),
    _c("f32_c128_r31", False, F32, 128, 31), _c("f32_c128_r33", False, F32, 128, 33), _c("f32_c40_r1", False, F32, 40, 1),
    _c("f32_c64_win", False, F32, 64, rule=WIN), _c("f32_c256_rw_r100", False, F32, 256, 100, RW), _c("f32_c128_r9000", False, F32, 128, 9000),
]


def case_data(c):
    """Host tensors of a case, seeded by its name: (w [R] fp64 row weights, rw [R] fp32 or None, (win, halo, valid), y, dz
    [R][C] rounded to the case's dtype, mean, rstd, gamma, beta [C] fp32).  y, gamma, beta are continuous draws and beta is
    not tied to mean rstd gamma, so a pre-activation lands in the kink band with probability ~ 64 u_f."""
    g = torch.Generator().manual_seed(sum(map(ord, c.name)))
    R, C = c.R, c.C
    rw, win = None, (0, 0, 0)
    if c.rule[0] == "none":
        w = torch.ones(R, dtype=F64)
    elif c.rule[0] == "win":
        win = tuple(c.rule[1:4])
        w = nr.window_weights(R, *win)
    else:
        rw = torch.tensor([-1.0, 0.0, 1.0, 3.0])[torch.randint(0, 4, (R,), generator=g)]
        rw[:5], rw[-7:] = -1.0, -1.0
        rw[5:8] = torch.tensor([3.0, 0.0, 1.0])
        w = rw.double()
    y = (0.3 + 1.5 * torch.randn(R, C, generator=g)).to(c.dt).float()
    dz = torch.randn(R, C, generator=g).to(c.dt).float()
    mean = 0.3 + 0.5 * torch.randn(C, generator=g)
    rstd = torch.rsqrt(torch.rand(C, generator=g) * 2.0 + 0.25)
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    return w, rw, win, y, dz, mean, rstd, gamma, beta


def _placed(values, dt, off=0):
    """A guarded copy of `values` whose first element lies `off` elements behind a 16-byte aligned address."""
    gd = Guarded(values.numel() + off, dt)
    v = gd.view(tuple(values.shape), off=off)
    v.copy_(values)
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_bn_eval_bwd_form_against_fp64(c):
    L, ok, stream, DT, _ = _lib()
    dt, C, R, name = c.dt, c.C, c.R, c.name
    w64, rw, (win, halo, valid), y, dz, mean, rstd, gamma, beta = case_data(c)
    w = w64.to(DEV)
    y, dz = _placed(y, dt, c.off), _placed(dz, dt, c.off)
    y[w < 0] = float("nan")                         # excluded / halo rows are never read
    dz[w < 0] = float("nan")
    mean, rstd, gamma, beta = (_placed(t, F32) for t in (mean, rstd, gamma, beta))
    rw = None if rw is None else _placed(rw, F32)
    ws = torch.empty(L.dl_bn_workspace_bytes(R, C), dtype=torch.uint8, device=DEV)

    def launch(relu_in, relu_out, with_sums):
        gd = Guarded(R * C + c.off, dt)
        dx = gd.view((R, C), off=c.off)
        sg, sums = _out((2 * C,), F32)
        wide = dt == BF and C in (64, 128, 256) and all(t.data_ptr() % 16 == 0 for t in (dz, y, dx))
        assert wide == c.wide, "%s: the case names the other form" % name
        before = (gd.bits(), sg.bits())
        ok(L.dl_bn_eval_bwd(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                            beta.data_ptr() if relu_out else None, relu_in, relu_out, dx.data_ptr(), sums.data_ptr() if with_sums else None,
                            R, C, win, halo, valid, _ptr(rw), DT[dt], ws.data_ptr() if with_sums else None, ws.numel() if with_sums else 0,
                            stream), "dl_bn_eval_bwd")
        torch.cuda.synchronize()
        gd.untouched(name, before[0])
        if with_sums:
            sg.untouched(name, before[1])
        else:
            assert torch.equal(sg.bits(), before[1]), "%s: sums written although not asked for" % name
        return gd, dx, sg, sums

    for relu_in, relu_out in MASKS:
        tag = "%s[relu_in=%d,relu_out=%d]" % (name, relu_in, relu_out)
        a, b = launch(relu_in, relu_out, True), launch(relu_in, relu_out, True)
        assert torch.equal(a[0].bits(), b[0].bits()) and torch.equal(a[2].bits(), b[2].bits()), "%s: not bitwise repeatable" % tag
        check_bn_eval(tag, dt, dz, y, w, mean, rstd, gamma, beta, relu_in, relu_out, a[1], a[3])
        n = launch(relu_in, relu_out, False)                                   # sums == NULL: the dx pass alone
        check_bn_eval(tag + "[no sums]", dt, dz, y, w, mean, rstd, gamma, beta, relu_in, relu_out, n[1], None)
        assert torch.equal(n[0].bits(), a[0].bits()), "%s: dx differs between the launches with and without sums" % tag


@pytest.mark.gpu
def test_bn_eval_bwd_refuses_bad_arguments():
    L, _, stream, DT, lib_mod = _lib()
    R, C = 8, 64
    t = torch.zeros(R, C, device=DEV)
    o = torch.empty(R, C, device=DEV)
    p = torch.ones(C, device=DEV)
    s = torch.empty(2 * C, device=DEV)
    ws = torch.empty(L.dl_bn_workspace_bytes(R, C), dtype=torch.uint8, device=DEV)

    def call(dz=t, dy=o, beta=None, relu_out=0, sums=s, ws_bytes=ws.numel()):
        return L.dl_bn_eval_bwd(dz.data_ptr(), t.data_ptr(), p.data_ptr(), p.data_ptr(), p.data_ptr(), _ptr(beta), 0, relu_out, dy.data_ptr(),
                                _ptr(sums), R, C, 0, 0, 0, None, DT[F32], ws.data_ptr(), ws_bytes, stream)

    assert call() == 0
    assert call(dy=t) != 0                          # dy aliases dz
    assert call(relu_out=1) != 0                    # relu_out without beta
    assert call(ws_bytes=16) != 0                   # sums asked for, workspace too small
    assert call(sums=None, ws_bytes=0) == 0         # no sums: no workspace needed
    torch.cuda.synchronize()
