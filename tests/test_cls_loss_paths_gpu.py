"""Every launch form of the classification-loss kernels (csrc/cls_loss.hip: dl_cls_loss_fwd / dl_cls_loss_bwd) element-wise
against the fp64 reference of tests/cls_loss_ref.py, in the manner of tests/test_loss_paths_gpu.py:

    |got - ref| <= MARGIN x (first-order rounding sum) x mag + floor     for every addressed element of every output,

operands in the middle of NaN-filled buffers, outputs in NaN-filled buffers with nothing outside the addressed elements
changed, every launch twice and bitwise repeatable.  The cases (tests/cls_loss_ref.py: CASES) cross N, dtype, n_out, ld,
weights, gamma and (a_pos, a_neg) with both forms; their data conditions are asserted without a GPU in
tests/test_cls_loss_reference_cpu.py.  Then the bad inputs: a non-finite z, a bad label, a bad weight.

Forms (host rule cls_single(N): N <= 4096)
  forward   one workgroup: cls_loss_fwd_kernel<T> on a grid of 1, each of 256 threads walks rows t, t + 256, ... (R = ceil(N / 256)
            <= 16 serial adds), wave tree (6 levels) + 4 LDS words (2 levels), the division.
            two-stage: cls_loss_fwd_kernel<T> on ceil(N / 256) workgroups (one row per thread, the same tree), then
            cls_loss_final_kernel: 256 threads stride over the nb partial pairs (ceil(nb / 256) serial adds), the tree, the division.
  backward  cls_loss_bwd_kernel<T>, one thread per row, in both.

Rounding model (first order; u_f = 2^-24, u_b = 2^-8 for a bf16 store; the units below are u_f).  Per row, in the order of
cls_row():
  e = expf(-|z|) (1 ulp: 2), l1 = log1pf(e) (2 ulp: 4, + e's 2 -> 6), hi = 1 / (1 + e) (the sum 1, e's share <= 1, the quotient
  <= 2.5 ulp: 5 -> 7), lo = e hi (2 + 7 + 1 = 10): p and q carry E_s = 10.  softplus = max(+-z, 0) + l1: E_sp = 7.
  s = y q - (1 - y) p: (1 - y) 1, each product 1, the difference 1: |ds| <= (E_s + 4) mag_s = 14 mag_s =: E_d mag_s, mag_s = y q +
  (1 - y) p (for hard labels mag_s = d: no cancellation, which is why d is formed this way).
  pm1 = d^(gamma - 1), m = pm1 d: whole gamma by <= 7 multiplies, otherwise powf (OpenCL bound 16 ulp: 32; gamma - 1 is exact):
  E_pow = 32 relative, plus the absolute error of d: |dm| <= gamma pm1 E_d mag_s + m E_pow.
  B = a_pos y softplus(-z) + a_neg (1 - y) softplus(z), non-negative terms: E_B = E_sp + 4 = 11.
  l = (w m) B: two products ->  |dl| <= 45 mag_l,  mag_l = w B (m + gamma pm1 mag_s)                     (K_L = E_pow + E_B + 2)
  dB = a_neg (1 - y) p - a_pos y q: (E_s + 4) mag_dB.   dm = -(gamma pm1) sgn(s) p q: relative E_pow + 2 E_s + 3 = 55 in pm1's
  relative part and (gamma - 1) d^(gamma - 2) E_d mag_s in d's absolute part; times B: + E_B + 1 = 67.  m dB: (E_pow + E_s + 4) = 46.
  dl = w (dm B + m dB): the sum and w 2 more; g = (gout / den) dl: the quotient 5, den's own error D (below), the product 1:
      |dg| <= (76 + D) mag_grad + u_st |g|,   mag_grad = |gout / den| mag_dz (cls_loss_ref).                   (K_G = 76 + D)
  The sign of s is the reference's: the cases keep d = 0 exactly or d > 256 u_f mag_s (conditions()).
  Two outputs: z = fl(score[1] - score[0]) carries u_f |z|, which moves l, g and p by the sensitivities sens_* of cls_loss_ref.
Sums: den and the loss numerator are sums of non-negative / same-order terms through D roundings, D = R + 8 in the
  one-workgroup form and 17 + ceil(nb / 256) in the two-stage form:
      |d den| <= D den,   |d loss| <= (K_L + 2 D + 2) sum mag_l / den.
Underflow: fp32 and bf16 share the exponent range; below 2^-126 a term (sigmoid(-90) = 8e-40, its softplus, their products)
  may be flushed or keep only absolute precision.  Every such quantity is multiplied by factors of at most
  (1 + w)(1 + a_pos + a_neg)(2 + gamma)(1 + |z|) (and 1 + |gout / den| in the gradient): that times 2^-126 is the floor.

DL_CLS_LOSS_BOUND_LOG=<file>: every check appends one JSON line; `python -m tests.test_cls_loss_paths_gpu <log> <out>` reduces
it to profiles/cls_loss_bound_margins.txt (worst ratio per form, output and dtype).
"""
import collections
import json
import math
import os
import sys

import pytest
import torch

from tests import cls_loss_ref as R
from tests.test_loss_paths_gpu import Buf, MARGIN, U_B, U_F, _rc, _twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TINY = 2.0 ** -126
E_S, K_L, K_G0 = 10.0, 45.0, 76.0
CODE = 4                         # what the raw launches ask dl_cls_loss_fwd to OR into their private flag word


def _dtn(dt):
    return "bf16" if dt == BF else "f32"


def _form(N):
    return "one-workgroup" if N <= R.ONE_WG else "two-stage"


def _depth(N):
    nb = (N + 255) // 256
    return (nb + 8) if N <= R.ONE_WG else 17 + (nb + 255) // 256


def check(case, form, what, dt, got, ref, bound):
    got, ref, bound = got.double().cpu(), ref.double().cpu(), torch.as_tensor(bound, dtype=F64).cpu()
    assert got.shape == ref.shape, "%s: %s has shape %s, reference %s" % (case, what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "%s: %s has non-finite addressed elements" % (case, what)
    ratio = float(((got - ref).abs() / (bound + 1e-300)).max())
    path = os.environ.get("DL_CLS_LOSS_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "form": form, "output": what, "dtype": _dtn(dt), "ratio": ratio}) + "\n")
    assert ratio <= 1.0, "%s [%s]: %s exceeds its rounding bound by x%.3g" % (case, form, what, ratio)


def _floor(r, w, a, gamma):
    ww = torch.ones_like(r["z"]) if w is None else w.double().clamp(min=0).nan_to_num(0.0, 0.0, 0.0)
    z = r["z"].abs().nan_to_num(0.0, 0.0, 0.0)
    return TINY * (1 + ww) * (1 + a[0] + a[1]) * (2 + gamma) * (1 + z)


class Run:
    """One case on the device: operands inside NaN-filled buffers, one forward (twice) and one backward (twice)."""

    def __init__(self, name, score, y, w, a, gamma, gout, ld):
        from druglamp_amd import _lib, ops
        self.name, self.a, self.gamma, self.gout = name, a, gamma, gout
        N, n_out = score.shape
        self.N, self.n_out, self.dt, self.ld = N, n_out, score.dtype, ld
        L = _lib.lib()
        sb = Buf((N - 1) * ld + n_out, score.dtype)
        sb.view((N, n_out), (ld, 1)).copy_(score.to(DEV))
        yb = Buf(N, F32)
        yb.view((N,)).copy_(y.to(DEV))
        wb = None
        if w is not None:
            wb = Buf(N, F32)
            wb.view((N,)).copy_(w.to(DEV))
        nws = L.dl_cls_loss_workspace_bytes(N)
        assert (nws == 0) == (N <= R.ONE_WG)
        self.probs_b, self.out2_b, self.ws_b = Buf(N, F32), Buf(2, F32), Buf(max(nws // 4, 1), F32)
        self.probs, self.out2 = self.probs_b.view((N,)), self.out2_b.view((2,))
        if nws:
            self.ws_b.view((nws // 4,))
        self.flags = torch.zeros(1, dtype=torch.int32, device=DEV)
        g = torch.tensor([gout], dtype=F32, device=DEV)
        self.ds_b = Buf((N - 1) * ld + n_out, score.dtype)
        self.ds = self.ds_b.view((N, n_out), (ld, 1))
        dtc = ops._dt(score)
        wp = None if wb is None else wb.ptr()
        _twice(name, "forward", [self.probs_b, self.out2_b] + ([self.ws_b] if nws else []),
               lambda: _rc(L.dl_cls_loss_fwd(sb.ptr(), ld, n_out, dtc, yb.ptr(), wp, N, a[0], a[1], gamma, self.probs_b.ptr(), self.out2_b.ptr(),
                                             self.ws_b.ptr() if nws else None, nws, CODE, self.flags.data_ptr(), ops._stream()), "dl_cls_loss_fwd"))
        if not nws:
            self.ws_b.untouched(name, "the unused workspace")
        _twice(name, "backward", [self.ds_b],
               lambda: _rc(L.dl_cls_loss_bwd(sb.ptr(), ld, n_out, dtc, yb.ptr(), wp, N, a[0], a[1], gamma, self.out2_b.ptr(), g.data_ptr(),
                                             self.ds_b.ptr(), ld, ops._stream()), "dl_cls_loss_bwd"))

    def check_rows(self, r, w, rows=None):
        """probs and dscore of `rows` (default: all) against the reference r."""
        name, form, dt = self.name, _form(self.N), self.dt
        two = 1.0 if self.n_out == 2 else 0.0
        D = _depth(self.N)
        fl = _floor(r, w, self.a, self.gamma)
        sel = slice(None) if rows is None else rows
        pb = MARGIN * U_F * (E_S * r["probs"].abs() + two * r["sens_p"]) + MARGIN * TINY
        check(name, form, "probs", dt, self.probs.cpu()[sel], r["probs"][sel], pb[sel])
        u_st = U_B if dt == BF else 0.0
        gs = abs(r["gs"])
        gb = MARGIN * (((K_G0 + D) * U_F + u_st) * r["mag_grad"] + u_st * r["grad"].abs() + two * U_F * gs * r["sens_dz"]) + MARGIN * fl * (1 + gs)
        ds = self.ds.cpu()
        if self.n_out == 2:
            check(name, form + " bwd", "dscore[:, 0]", dt, ds[sel, 0], -r["grad"][sel], gb[sel])
            check(name, form + " bwd", "dscore[:, 1]", dt, ds[sel, 1], r["grad"][sel], gb[sel])
        else:
            check(name, form + " bwd", "dscore", dt, ds[sel, 0], r["grad"][sel], gb[sel])

    def check_den(self, r):
        D = _depth(self.N)
        check(self.name, _form(self.N), "den", self.dt, self.out2.cpu()[1:], torch.tensor([r["den"]], dtype=F64), MARGIN * D * U_F * r["den"])


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_cls_loss_form_against_fp64(c):
    score, y, w, gout = R.case_data(c)
    r = R.cls_loss(score, y, w, c.a[0], c.a[1], c.gamma, gout)
    R.conditions(c, r, y)
    run = Run(c.name, score, y, w, c.a, c.gamma, gout, c.ld)
    assert int(run.flags.item()) == 0, "%s: the flag word was raised on clean data" % c.name
    run.check_rows(r, w)
    run.check_den(r)
    D = _depth(c.N)
    two = 1.0 if c.n_out == 2 else 0.0
    lb = MARGIN * (U_F * ((K_L + 2 * D + 2) * float(r["mag_l"].sum()) + two * float(r["sens_l"].sum())) + float(_floor(r, w, c.a, c.gamma).sum())) / r["den"]
    check(c.name, _form(c.N), "loss", c.dt, run.out2.cpu()[:1], torch.tensor([r["loss"]], dtype=F64), lb)
    if c.data == "yp" and c.N > R.YP_ROW:                          # y == p exactly: d = 0, m = 0, sgn(0) = 0 -> a zero gradient, bit for bit
        assert float(run.ds[R.YP_ROW].float().abs().max()) == 0.0 and float(run.probs[R.YP_ROW]) == 0.5


BAD = [(b, s) for b in R.BAD_CASES for s in R.BAD_SHAPES]


@pytest.mark.parametrize("b,shape", BAD, ids=["%s_n%d_%s_o%d" % (b.name, s[0], _dtn(s[1]), s[2]) for b, s in BAD])
def test_bad_input_poisons_its_row_only(b, shape):
    N, dt, n_out = shape
    score, y, w, gout = R.bad_data(b, N, dt, n_out)
    r = R.cls_loss(score, y, w, 0.25, 0.75, 2.0, gout)
    assert r["poisoned"].nonzero().flatten().tolist() == [b.row] and r["den"] > 0
    run = Run("%s_n%d" % (b.name, N), score, y, w, (0.25, 0.75), 2.0, gout, n_out)
    torch.cuda.synchronize()                                        # the process survives: no device assert
    assert int(run.flags.item()) == (CODE if b.flagged else 0), (b.name, int(run.flags.item()))
    assert math.isnan(float(run.out2[0])), "%s: the loss is %r, not NaN" % (b.name, float(run.out2[0]))
    assert bool(torch.isnan(run.ds[b.row].float()).all()), "%s: the bad row's gradient is not NaN" % b.name
    others = torch.arange(N) != b.row
    run.check_rows(r, w, others)                                    # the reference computed without the bad row
    run.check_den(r)
    if b.what == "z":                                               # sigmoid(z) by IEEE rules
        got, want = float(run.probs[b.row]), float(r["probs"][b.row])
        assert got == want or (got != got and want != want), (b.name, got, want)


def test_bad_label_and_weight_surface_through_check_guard_flags():
    from druglamp_amd import ops
    ops.guard_flags(DEV).zero_()
    ops.cls_loss_flags(DEV).zero_()
    score, y, w, _ = R.bad_data(R.BAD_CASES[0], 64, F32, 1)        # (the NaN score: poisons, but is no label / weight error)
    out2, _ = ops.cls_loss_fwd(score.to(DEV), y.to(DEV), w.to(DEV), 1.0, 1.0, 0.0)
    assert math.isnan(float(out2[0]))
    ops.check_guard_flags(DEV)                                      # nothing raised
    for b in R.BAD_CASES:
        if not b.flagged:
            continue
        score, y, w, _ = R.bad_data(b, 64, BF, 2)
        out2, probs = ops.cls_loss_fwd(score.to(DEV), y.to(DEV), w.to(DEV), 3.0, 1.0, 1.0)
        assert math.isnan(float(out2[0])) and probs.shape == (64,), b.name
        assert int(ops.guard_flags(DEV).item()) == 0                # the padding guards' word is not touched
        with pytest.raises(RuntimeError, match="FLAG_CLS_LABEL"):
            ops.check_guard_flags(DEV)
        assert int(ops.cls_loss_flags(DEV).item()) == 0             # cleared by the check
        ops.check_guard_flags(DEV)


def test_autograd_function_returns_loss_and_probs_and_the_kernel_gradient():
    from druglamp_amd.cls_loss import ClsLoss, classification_loss
    c = R.BY_NAME["n257_soft"]
    score, y, w, _ = R.case_data(c)
    r = R.cls_loss(score, y, w, 0.25, 0.75, 2.0, 1.0)
    s = score.to(DEV).requires_grad_(True)
    n, loss = classification_loss(s, y.to(DEV).unsqueeze(1), ClsLoss.focal(0.25, 2.0), w.to(DEV))
    assert n.shape == (c.N,) and n.dtype == F32 and not n.requires_grad and loss.dim() == 0
    (loss * 1.0).backward()
    D = _depth(c.N)
    check(c.name + " fn", "ClsLossFn", "grad", F32, s.grad.cpu()[:, 0], r["grad"], MARGIN * (K_G0 + D) * U_F * r["mag_grad"] + MARGIN * TINY)
    check(c.name + " fn", "ClsLossFn", "n", F32, n.cpu(), r["probs"], MARGIN * E_S * U_F * r["probs"] + MARGIN * TINY)
    assert abs(float(loss.detach()) - r["loss"]) <= MARGIN * U_F * (K_L + 2 * D + 2) * float(r["mag_l"].sum()) / r["den"]


if __name__ == "__main__":       # python -m tests.test_cls_loss_paths_gpu <DL_CLS_LOSS_BOUND_LOG file> <profiles/cls_loss_bound_margins.txt>
    worst = collections.OrderedDict()
    for line in open(sys.argv[1]):
        e = json.loads(line)
        k = (e["form"], e["output"], e["dtype"])
        if k not in worst or e["ratio"] > worst[k][0]:
            worst[k] = (e["ratio"], e["case"])
    out = ["Worst |err| / bound of tests/test_cls_loss_paths_gpu.py on an MI355X (gfx950), per launch form, output and dtype",
           "(bounds carry MARGIN = %g: a ratio at or below %.2f stays inside the first-order rounding model itself)." % (MARGIN, 1 / MARGIN),
           "", "%-22s %-14s %-6s %9s  %s" % ("form", "output", "dtype", "worst", "case")]
    for (form, what, dt), (ratio, case) in sorted(worst.items()):
        out.append("%-22s %-14s %-6s %9.4f  %s%s" % (form, what, dt, ratio, case, "   >1/MARGIN" if ratio > 1 / MARGIN else ""))
    open(sys.argv[2], "w").write("\n".join(out) + "\n")
    print("\n".join(out))
