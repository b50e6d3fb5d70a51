"""Every launch form of the loss kernels (ntxent.hip: ntx_launch; losses.hip: dl_cos_rowloss_*, dl_ce_rows_*,
dl_triplet_sigcos_*) element-wise against the fp64 references of tests/loss_ref.py:

    |got - ref| <= bound = MARGIN x (first-order rounding sum) x mag     for every addressed element of every output,

with `mag` the sum of the absolute terms of the output's own expression (loss_ref returns it).  One table of cases per
family; every case names the kernel instantiations it selects.  Every operand lies in the middle of a larger buffer whose
other elements are NaN (labels: an out-of-range class, label matrices: positives), every output in a NaN-filled buffer:
addressed elements must be overwritten (finite), everything else bitwise unchanged, including the triplet scratch past
dl_triplet_sigcos_buffer_floats and dlogits columns >= Cp.  Every launch runs twice and must be bitwise repeatable.
The data generators and the conditions on the references (`ntx_conditions`, `triplet_conditions`) take no GPU:
tests/test_loss_reference_cpu.py asserts the conditions for every case but the 65536 x 65536 one.

DL_LOSS_BOUND_LOG=<file>: every check appends one JSON line (case, kernel form, output, dtype, worst |err| / bound);
tools/loss_bound_margins.py reduces it to profiles/loss_bound_margins.txt.

Forms (host dispatch)
  ntx_launch         ntxent_kernel<T, HD, RT, BWD>: T = float -> RT 1; T = bf16 -> RT 2 once the resident side has 2 n >= 65536
                     rows, else RT 1; HD = d in {64, 128}; 6 instantiations x forward / backward.  The LDS ring has 4 slots
                     while a 64-row tile is <= 16 KiB and 3 for <float, 128>.  The backward picks one of three weight loops by
                     which log-sum-exp vectors it is given (wmode 0: both, 1: resident only, 2: streamed only), each in a
                     fast copy and a `slow` copy (tiles holding an own / positive column, the streamed tail or an invalid
                     resident row).  dl_ntxent_fwd_ex adds ntx_vec_sum_kernel when `loss` is given.
  dl_cos_rowloss_*   cos_rowloss_fwd_kernel (+ vec_sum_kernel when loss_sum is given), cos_rowloss_bwd_kernel; fp32.
  dl_ce_rows_fwd     bf16, ld == 32, C <= 32, 16-byte base -> ce_rows32_fwd_kernel; else ce_rows_fwd_kernel<T>; then
                     ce_rows_final_kernel.
  dl_ce_rows_bwd     bf16, ld == ldd == Cp == 32, C <= 32, 16-byte bases -> ce_rows32_bwd_kernel; else ce_rows_bwd_kernel<T>.
  dl_triplet_sigcos  fwd: row_norm x 2, sigcos_dist, triplet_reduce (no coefficients), triplet_final; bwd: triplet_reduce
                     (coefficients by atomic +-1), triplet_bwd_p, triplet_bwd_d.  n_d <= 8192 (LDS index lists).

Rounding model (first order; u_f = 2^-24 fp32, u_b = 2^-8 bf16 round to nearest).  The references read the kernels' own
operands, so every error is the kernels' rounding.  A fp32 sum of N terms in the order the code performs it has a
relative error of at most N u_f of the sum of the absolute terms.  exp(x) is evaluated as exp2(x log2 e): rounding the
argument contributes |x| u_f relative, the unit 2 u_f.
  NT-Xent logits: bf16 products are exact in fp32 (fp32 products round once), fp32 accumulation over d terms:
      |ds| / T <= (d + 2) u_f lam, lam_i = max_j sum_d |a_id||b_jd| / T (loss_ref: `lam`, per resident row).
  NT-Xent forward: a term is exp2(fma(s, c, -fl(m c))), c = fl(fl(1 / T) log2 e): the logit error plus four roundings of
      an argument of size <= lam log2 e -> relative (d + 6) u_f lam + 2 u_f.  A lane sums one quarter of the streamed
      columns (2 n_b / 4 terms) and rescales its running sum once per tile at most: the multiply, the add and exp2's unit
      are 4 u_f per tile, and the rescale exponents telescope up to the rounding of fl(m c), u_f lam per change of the
      running maximum, at most one per tile -> nt lam u_f with nt = ceil(2 n_b / 64) tiles.  The 4-way combine evaluates
      exp2((m - m_all) c) without fma: 4 u_f lam and 8 u_f.  lse = m / T + log(l): logf 2 u_f of |log l| <= log(2 n_b),
      the product and the add 2 u_f of |lse| <= lam + log(2 n_b):
          |d lse_i| <= u_f [(d + 14 + nt) lam_i + 2 n_b / 4 + 4 nt + 12 + 4 log(2 n_b)].
      row_loss = lse - s_pos / T adds the positive logit's error and the subtraction: (d + 7) u_f lam_i.
      loss (ntx_vec_sum_kernel): against the fp64 mean of the kernel's own row_loss, 2 n_a u_f of mean |row_loss|.
  NT-Xent backward: an exp term of w is exp2(fma(s, c, -fl(lse log2 e))): relative E_w = u_f [(d + 6) lam_i + |lse| + 2]
      with |lse| the largest given log-sum-exp the row meets.  w (after the fp32 subtraction of the positive's count) is
      rounded to bf16 before the second product (u_b of |w|, bf16 rows only; fp32 rows keep fp32 weights), the product
      accumulates in fp32 over the 2 n_b streamed columns and is scaled by fl(gscale fl(1 / T)) (3 u_f):
          |d dA_id| <= [u_b + E_w + (2 n_b + 5) u_f] mag_id,  mag_id = gscale / T sum_j (exp terms + count [j = pos_i]) |B_jd|.
  cosine rows: dot, |x|^2, |y|^2 are lane sums of D / 64 terms plus a 6-level wave tree: L = D / 64 + 7.
      |d row_loss| <= u_f [2 (L + 1) mdot + 2 |cos| (L + 8) + 2 + 2 |cos|], mdot = sum |x y| / (dx dy) (the norm errors drop
      out where the eps clamp holds; the bound keeps them).  dx = a1 y + a2 x: u_f [(L + 12) |a1 y| + (2 L + 14) |a2 x| +
      (L + 1) t3], t3 = what an error of the dot moves (loss_ref).  loss_sum: n u_f sum |row_loss| against the fp64 sum of
      the kernel's own rows.
  cross entropy: lse = m + log(sum exp(x - m)) with fast exp / log: sum_c p_c (2 |x_c - m| + 2) u_f + C u_f for the sum,
      2 u_f |log sum| + u_f |lse| -> u_f [C + 6 + 4 mag_lse].  Row loss lse - x_y: u_f (|lse| + |x_y|) more.  The mean is a
      wave tree per 256 rows, a strided pass and a second tree: depth 20 + nb / 256 (nb = blocks) over sum |row loss| / count.
      dlogits = g (exp(x - lse) - [c = y]), g = gout / count: relative u_st + (8 + 2 |x - lse|) u_f of |g| (p + [c = y]),
      u_st the store's rounding (u_b for bf16).  Underflow: fp32 and bf16 share the exponent range; below the smallest
      normal 2^-126 an exp term or the product g p may be flushed to zero or keep only absolute precision (the `big`
      rows have exp(-160) ~ 3e-70 and g exp(-80) ~ 5e-38), so dlogits carries an absolute floor of (1 + |g|) 2^-126.
  triplet: norms and dots are lane sums of dim / 64 terms plus the tree: L = dim / 64 + 7.  cos: u_f [L mdot + (L + 6) |cos|],
      dist = 1 - sigmoid(cos) has slope <= 1 / 4 and its own few roundings: |d dist| <= u_f [(L mdot + (L + 6) |cos| + 2) / 4 + 3].
      Hinges: the references' hinge arguments stay further than 4 x that from zero (asserted), so the active set and
      n_tri are exact and the coefficient matrix (atomic +-1) is exact.  loss: active hinges each carry two distance errors
      and 3 u_f; the sum is 256 strided partial sums, a tree and a serial pass over the anchors: (T_max / 256 + 12 + n_p) u_f
      of the hinge sum, T_max the largest triplet count of an anchor.  dp (dd): serial over the n_d (n_p) columns, each
      term ~10 roundings and twice the cos error: (n + 3 L + 20) u_f mag.
bound = MARGIN x the sums above; a recorded worst ratio at or below 1 / MARGIN says a form stays inside the first-order model.
Scale bias (NT-Xent and cross entropy gradients): bf16 roundings are zero-mean, only the fp32-level part (`coherent`) can
move an output coherently; the least-squares scale s = sum (got - ref) ref / sum ref^2 must stay within
sum coherent |ref| / sum ref^2 plus six standard deviations of zero-mean errors of the remaining size.  The roundings must
be independent for that: the `equal` NT-Xent cases (all rows identical, so every gradient row is one scalar times the same
vector and the exact gradient cancels to zero) are left out of the scale check and keep the element-wise one.
"""
import collections
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U_B, U_F, MARGIN, LAM = 2.0 ** -8, 2.0 ** -24, 2.0, 96.0
LP = 18.0            # `spread` data: the logit / T every row has with its positive (and a planted column with its row)
COLW = 0.05


def _dtname(dt):
    return str(dt).split(".")[1]


# ---- the check ---------------------------------------------------------------------------------------------------------------
def _log(case, form, what, dt, ratio):
    path = os.environ.get("DL_LOSS_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "form": form, "output": what, "dtype": _dtname(dt), "ratio": ratio}) + "\n")


def check(case, form, what, dt, got, ref, bound, coherent=None):
    """|got - ref| <= bound element by element; coherent: the fp32-level part of `bound`, given where the scale-bias check
    applies."""
    got = torch.as_tensor(got, dtype=F64, device=ref.device) if not torch.is_tensor(got) else got.double()
    assert got.shape == ref.shape, "%s: %s has shape %s, reference %s" % (case, what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "%s: %s has non-finite addressed elements" % (case, what)
    err = got - ref
    ratio = float((err.abs() / (bound + 1e-300)).max())
    _log(case, form, what, dt, ratio)
    assert ratio <= 1.0, "%s [%s]: %s exceeds its rounding bound by x%.3g" % (case, form, what, ratio)
    den = float((ref * ref).sum())
    if coherent is not None and den > 0:
        s = float((err * ref).sum()) / den
        lim = (float((coherent * ref.abs()).sum()) + 6.0 * float((((bound - coherent) * ref) ** 2).sum().sqrt()) / math.sqrt(3.0)) / den
        _log(case, form, what + " bias", dt, abs(s) / lim)
        assert abs(s) <= lim, "%s [%s]: %s carries a scale error of %.3g (allowed %.3g)" % (case, form, what, s, lim)


class Buf:
    """A flat buffer of n elements with a guard band on both sides, filled with `fill` (NaN); `view` hands out as_strided
    views of the addressed elements and records them in `mask`."""
    G = 64                                               # elements: a multiple of 16 bytes in every dtype used

    def __init__(self, n, dt=F32, fill=float("nan"), dev=DEV):
        self.fill, self.n = fill, n
        self.t = torch.full((n + 2 * self.G,), fill, device=dev, dtype=dt)
        self.mask = torch.zeros(n + 2 * self.G, dtype=torch.bool, device=dev)

    def view(self, shape, strides=None, off=0):
        if strides is None:
            strides, acc = [], 1
            for s in reversed(shape):
                strides.insert(0, acc)
                acc *= s
        torch.as_strided(self.mask, shape, strides, self.G + off).fill_(True)
        return torch.as_strided(self.t, shape, strides, self.G + off)

    def ptr(self, off=0):
        return self.t.data_ptr() + (self.G + off) * self.t.element_size()

    def bits(self):
        it = {2: torch.int16, 4: torch.int32}.get(self.t.element_size()) if self.t.is_floating_point() else None
        return (self.t.view(it) if it is not None else self.t).clone()

    def refill(self):
        self.t.fill_(self.fill)

    def untouched(self, case, what):
        """Everything outside the addressed elements still holds the fill pattern, bit for bit."""
        fresh = Buf(0, self.t.dtype, self.fill, self.t.device).bits()[0]
        out = self.bits()[~self.mask]
        assert bool((out == fresh).all()), "%s: %s was written outside its addressed elements" % (case, what)


def guard(t, fill=float("nan")):
    """A copy of t in the middle of a larger buffer of `fill`; contiguous, 16-byte aligned when the allocation is."""
    b = Buf(t.numel(), t.dtype, fill, DEV)
    v = b.view(tuple(t.shape))
    v.copy_(t)
    return v


def out(shape, dt=F32):
    b = Buf(int(np.prod(shape)), dt)
    return b, b.view(tuple(shape))


def _rc(rc, what):
    from druglamp_amd import _lib
    _lib.check(rc, what)


def _twice(case, what, bufs, launch):
    """Run `launch` twice into refilled output buffers: bitwise equal results, nothing written outside."""
    snaps = []
    for rep in range(2):
        for b in bufs:
            b.refill()
        launch()
        torch.cuda.synchronize()
        for i, b in enumerate(bufs):
            b.untouched(case, "%s output %d" % (what, i))
        snaps.append([b.bits() for b in bufs])
    for x, y in zip(*snaps):
        assert torch.equal(x, y), "%s: %s is not bitwise repeatable" % (case, what)


# ==== NT-Xent =================================================================================================================
# A case is a global batch (q, k of n_global rows) and launches (a_off, n_a, b_off, n_b, wmodes): resident rows
# [a_off, a_off + n_a) of both halves scored against streamed rows [b_off, b_off + n_b); the forward always runs, then one
# backward per wmode (0 needs equal sides: both log-sum-exp vectors are the forward's; 2 takes the streamed side's
# log-sum-exp from the kernel run with the sides swapped: an operand, exact to the reference).
NtxCase = collections.namedtuple("NtxCase", "name forms dt d T kind ng launches seed plant entry")


def _nform(dt, d, rt, nst):
    t = "bf16" if dt == BF else "float"
    return ("ntxent<%s,%d,%d,fwd> ring%d" % (t, d, rt, nst), "ntxent<%s,%d,%d,bwd> ring%d" % (t, d, rt, nst))


def _nst(dt, d):
    return 4 if 64 * d * (2 if dt == BF else 4) <= 16384 else 3


def _ntx_cases():
    cs, i = [], 0
    kinds = ("spread", "big", "equal")
    for n in (1, 8, 37, 64, 200):                       # last tile with 2, 16, 10, 64 (full) and 16 valid columns of 2 n
        for dt in (F32, BF):
            for d in (64, 128):
                kind, T = kinds[(i + i // 4) % 3], (0.1, 0.5)[(i + i // 4) % 2]
                cs.append(NtxCase("sym_n%d_%s_d%d_%s_T%g" % (n, _dtname(dt), d, kind, T), _nform(dt, d, 1, _nst(dt, d)), dt, d, T, kind,
                                  n, ((0, n, 0, n, (0,)),), 100 + i, None, "ex"))
                i += 1
    for dt in (F32, BF):                                # streamed sides that wrap the ring; both one-sided weight loops
        w3 = tuple((r * 40, 40, 0, 120, (1,)) for r in range(3)) + tuple((0, 120, r * 40, 40, (2,)) for r in range(3))
        cs.append(NtxCase("ring_world3_%s" % _dtname(dt), _nform(dt, 128, 1, _nst(dt, 128)), dt, 128, 0.1, "spread", 120, w3, 131, None, "ex"))
        cs.append(NtxCase("ring_330_%s" % _dtname(dt), _nform(dt, 128, 1, _nst(dt, 128)), dt, 128, 0.5, "spread", 330,
                          ((145, 40, 0, 330, (1,)), (0, 330, 145, 40, (2,))), 137, (145, 40), "ex"))
        cs.append(NtxCase("ring_330_big_%s" % _dtname(dt), _nform(dt, 128, 1, _nst(dt, 128)), dt, 128, 0.1, "big", 330,
                          ((290, 40, 0, 330, (1,)), (0, 330, 0, 40, (2,))), 139, None, "ex"))
    # two 16-row tiles per wave: streamed rows at the start, the middle and the end of the global batch
    for n, nb, d, kind, T in ((32768, 100, 64, "spread", 0.1), (32805, 321, 64, "big", 0.5), (32768, 321, 128, "spread", 0.5),
                              (32805, 100, 128, "spread", 0.1)):
        ls = tuple((0, n, off, nb, (1, 2)) for off in (0, (n - nb) // 2 + 1, n - nb))
        cs.append(NtxCase("rt2_n%d_nb%d_d%d_%s" % (n, nb, d, kind), _nform(BF, d, 2, 4), BF, d, T, kind, n, ls, 151 + d + nb, None, "ex"))
    cs.append(NtxCase("rt2_product_n32768_d128", _nform(BF, 128, 2, 4), BF, 128, 0.1, "spread", 32768, ((0, 32768, 0, 32768, (0,)),),
                      171, None, "ex"))
    cs.append(NtxCase("rt_boundary_n32767_nb64_d64", _nform(BF, 64, 1, 4), BF, 64, 0.1, "spread", 32767, ((0, 32767, 16000, 64, (1, 2)),),
                      173, None, "ex"))
    cs.append(NtxCase("legacy_entry_n37_f32_d64", _nform(F32, 64, 1, 4), F32, 64, 0.5, "spread", 37, ((0, 37, 0, 37, (0,)),), 175, None,
                      "legacy"))
    cs.append(NtxCase("autograd_fn_n200_bf16_d128", _nform(BF, 128, 1, 4), BF, 128, 0.1, "spread", 200, ((0, 200, 0, 200, (0,)),), 177,
                      None, "fn"))
    return cs


NTX_CASES = _ntx_cases()
NTX_BIG = ("rt2_product_n32768_d128",)               # 65536 resident x 65536 streamed rows: conditions asserted on the GPU only


def ntx_batch(c):
    """The global batch (q, k) of a case on the CPU, rounded to the case's dtype.
    spread: logits / T of standard deviation ~4; every row has logit / T = LP with its positive, and where `plant` names a
            small resident range every streamed row outside it has logit / T = LP with one resident row (round robin), so
            that every streamed column carries weight in some resident row;
    big:    |logit| / T of tens, up to LAM;   equal: all rows identical."""
    g = torch.Generator().manual_seed(c.seed)
    d, T, ng = c.d, c.T, c.ng
    if c.kind == "equal":
        v = torch.randn(d, generator=g, dtype=F64) * math.sqrt(8.0 * T / d)
        q = v.expand(ng, d).clone()
        return q.to(c.dt), q.clone().to(c.dt)
    sig = math.sqrt(36.0 * T / (0.64 * d)) if c.kind == "big" else math.sqrt(4.0 * T / math.sqrt(d))
    q, k = (torch.randn(ng, d, generator=g, dtype=F64) for _ in range(2))
    q, k = (x / (x * x).sum(1, keepdim=True).sqrt() * (sig * math.sqrt(d)) for x in (q, k))     # equal row norms: no outlier rows
    if c.kind == "spread":
        k += ((T * LP - (q * k).sum(1)) / (q * q).sum(1)).unsqueeze(1) * q
        if c.plant is not None:
            a0, na = c.plant
            A = torch.cat((q[a0:a0 + na], k[a0:a0 + na]))
            rows = torch.cat((torch.arange(0, a0), torch.arange(a0 + na, ng)))
            for h, x in enumerate((q, k)):
                tgt = A[(torch.arange(len(rows)) * 2 + h) % (2 * na)]
                x[rows] += ((T * LP - (x[rows] * tgt).sum(1)) / (tgt * tgt).sum(1)).unsqueeze(1) * tgt
    return q.to(c.dt), k.to(c.dt)


def ntx_sides(q, k, launch):
    a0, na, b0, nb, _ = launch
    return q[a0:a0 + na], k[a0:a0 + na], q[b0:b0 + nb], k[b0:b0 + nb]


def ntx_conditions(c, fwd_refs):
    """The conditions on the references alone: fwd_refs = [(launch, loss_ref.ntx_fwd result)] of every launch of the case."""
    for launch, r in fwd_refs:
        assert float(r["lam"].max()) <= LAM, "%s: |logit| / T beyond the range the bounds assume (%.3g)" % (c.name, float(r["lam"].max()))
    if c.kind == "spread":
        by_side = collections.OrderedDict()
        for (a0, na, b0, nb, _), r in fwd_refs:
            if nb <= 1024:
                cw = by_side.get((b0, nb))
                by_side[(b0, nb)] = r["colw"] if cw is None else torch.maximum(cw, r["colw"])
        for side, cw in by_side.items():
            assert float(cw.min()) >= COLW, "%s: streamed column %d of side %s carries weight %.3g only" % (
                c.name, int(cw.argmin()), side, float(cw.min()))


def ntx_bound_fwd(r, d, nb):
    nb2 = 2 * nb
    nt = (nb2 + 63) // 64
    b_lse = MARGIN * U_F * ((d + 14 + nt) * r["lam"] + nb2 / 4 + 4 * nt + 12 + 4 * math.log(nb2))
    return b_lse, b_lse + MARGIN * U_F * (d + 7) * r["lam"]


def ntx_bound_bwd(r, dt, d, nb, lse_a, lse_b, extra=0.0):
    """(bound, coherent part) of dq / dk stacked as [2 n_a][d]; extra: a further relative fp32-level error of every weight."""
    lmax = torch.zeros_like(r["lam"])
    if lse_a is not None:
        lmax = torch.maximum(lmax, lse_a.double().abs())
    if lse_b is not None:
        lmax = torch.maximum(lmax, lse_b.double().abs().max().expand_as(lmax))
    mag = torch.cat((r["mag_dq"], r["mag_dk"]))
    coh = MARGIN * (U_F * ((d + 6) * r["lam"] + lmax + 2 + (2 * nb + 5)) + extra).unsqueeze(1) * mag
    return coh + MARGIN * (U_B if dt == BF else 0.0) * mag, coh


def _ntx_launch(c, qg, kg, launch):
    from druglamp_amd import _lib, ops
    L = _lib.lib()
    a0, na, b0, nb, wmodes = launch
    tag = "%s a%d+%d b%d+%d" % (c.name, a0, na, b0, nb)
    sym = (a0, na) == (b0, nb)
    aq, ak, bq, bk = (guard(x) for x in ntx_sides(qg, kg, launch))
    if sym:                                             # the single-process launch passes the same rows as both sides
        bq, bk = aq, ak
    # ---- forward ----
    (lse_b_, lse), (rl_b_, rl), (ls_b_, ls) = out((2 * na,)), out((2 * na,)), out((1,))
    fa = ops._ntx_args(aq, ak, bq, bk, a0, b0, c.ng, c.T)
    _twice(tag, "forward", (lse_b_, rl_b_, ls_b_),
           lambda: _rc(L.dl_ntxent_fwd_ex(fa, lse_b_.ptr(), rl_b_.ptr(), ls_b_.ptr(), ops._stream()), "dl_ntxent_fwd_ex"))
    r = R.ntx_fwd(aq, ak, bq, bk, a0, b0, c.ng, c.T)
    b_lse, b_loss = ntx_bound_fwd(r, c.d, nb)
    check(tag, c.forms[0], "lse", c.dt, lse, r["lse"], b_lse)
    check(tag, c.forms[0], "row_loss", c.dt, rl, r["row_loss"], b_loss)
    own = rl.double()
    check(tag, "ntx_vec_sum", "loss", c.dt, ls, own.mean().reshape(1), MARGIN * 2 * na * U_F * own.abs().mean().reshape(1))
    # ---- backward, one launch per weight loop ----
    for wm in wmodes:
        assert wm != 0 or sym
        la = lse if wm in (0, 1) else None
        lb = None
        if wm == 0:
            lb = lse
        elif wm == 2:
            lb = guard(ops.ntxent_fwd_ex(bq, bk, aq, ak, b0, a0, c.ng, c.T)[1])
        gscale = 1.0 / (2 * nb if wm == 2 else 2 * na)
        ba = ops._ntx_args(aq, ak, bq, bk, a0, b0, c.ng, c.T, la, lb)
        (dq_b, dq), (dk_b, dk) = out((na, c.d)), out((na, c.d))
        _twice(tag, "backward wmode %d" % wm, (dq_b, dk_b),
               lambda: _rc(L.dl_ntxent_bwd_ex(ba, gscale, dq_b.ptr(), dk_b.ptr(), ops._stream()), "dl_ntxent_bwd_ex"))
        rb = R.ntx_bwd(aq, ak, bq, bk, a0, b0, c.ng, c.T, la, lb, gscale)
        bound, coh = ntx_bound_bwd(rb, c.dt, c.d, nb, la, lb)
        check(tag, c.forms[1] + " wmode%d" % wm, "dA", c.dt, torch.cat((dq, dk)), torch.cat((rb["dq"], rb["dk"])), bound,
              None if c.kind == "equal" else coh)
    return launch, r


def _ntx_legacy(c, qg, kg):
    """dl_ntxent_fwd / dl_ntxent_bwd (fp32 rows, one process) through ops."""
    from druglamp_amd import ops
    n = c.ng
    q, k = guard(qg), guard(kg)
    outs = [ops.ntxent_fwd(q, k, c.T) for _ in range(2)]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*outs)), "%s: forward not repeatable" % c.name
    loss, lse = outs[0]
    r = R.ntx_fwd(q, k, q, k, 0, 0, n, c.T)
    b_lse, b_loss = ntx_bound_fwd(r, c.d, n)
    check(c.name, c.forms[0], "lse", c.dt, lse, r["lse"], b_lse)
    check(c.name, c.forms[0] + " + ntx_vec_sum", "loss", c.dt, loss, r["row_loss"].mean().reshape(1),
          (b_loss.mean() + MARGIN * 2 * n * U_F * r["row_loss"].abs().mean()).reshape(1))
    gout = 0.75
    gs = [ops.ntxent_bwd(q, k, c.T, lse, gout) for _ in range(2)]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*gs)), "%s: backward not repeatable" % c.name
    gscale = float(torch.tensor(gout / (2 * n), dtype=F32))
    rb = R.ntx_bwd(q, k, q, k, 0, 0, n, c.T, lse, lse, gscale)
    bound, coh = ntx_bound_bwd(rb, c.dt, c.d, n, lse, lse)
    check(c.name, c.forms[1] + " wmode0", "dA", c.dt, torch.cat(gs[0]), torch.cat((rb["dq"], rb["dk"])), bound, coh)
    return (0, n, 0, n, (0,)), r


def _ntx_fn(c, qg, kg):
    """NTXentFn: bf16 rows in, bf16 gradients out; the reference's own log-sum-exp stands in for the kernel's (its bound
    joins the weights' error), the upstream gradient multiplies in fp32 and the result is rounded to bf16."""
    from druglamp_amd import functional as Fn
    n, up = c.ng, 0.625
    q, k = guard(qg).requires_grad_(True), guard(kg).requires_grad_(True)
    loss = Fn.NTXentFn.apply(q, k, c.T)
    (loss * up).backward()
    r = R.ntx_fwd(q.detach(), k.detach(), q.detach(), k.detach(), 0, 0, n, c.T)
    b_lse, b_loss = ntx_bound_fwd(r, c.d, n)
    check(c.name, c.forms[0] + " + ntx_vec_sum", "loss", c.dt, loss.detach().reshape(1), r["row_loss"].mean().reshape(1),
          (b_loss.mean() + MARGIN * 2 * n * U_F * r["row_loss"].abs().mean()).reshape(1))
    gscale = up / (2 * n)
    rb = R.ntx_bwd(q.detach(), k.detach(), q.detach(), k.detach(), 0, 0, n, c.T, r["lse"], r["lse"], gscale)
    bound, coh = ntx_bound_bwd(rb, c.dt, c.d, n, r["lse"], r["lse"], extra=float(b_lse.max()) / MARGIN + 2 * U_F)
    ref = torch.cat((rb["dq"], rb["dk"]))
    check(c.name, c.forms[1] + " wmode0", "dA (bf16)", c.dt, torch.cat((q.grad, k.grad)), ref, bound + MARGIN * U_B * ref.abs(), coh)
    assert q.grad.dtype == BF and k.grad.dtype == BF
    return (0, n, 0, n, (0,)), r


@pytest.mark.parametrize("c", NTX_CASES, ids=[c.name for c in NTX_CASES])
def test_ntxent_form_against_fp64(c):
    qc, kc = ntx_batch(c)
    qg, kg = qc.to(DEV), kc.to(DEV)
    if c.entry == "legacy":
        refs = [_ntx_legacy(c, qg, kg)]
    elif c.entry == "fn":
        refs = [_ntx_fn(c, qg, kg)]
    else:
        refs = [_ntx_launch(c, qg, kg, launch) for launch in c.launches]
    ntx_conditions(c, refs)


# ==== cosine row loss =========================================================================================================
COS_CASES = [(1, 4), (5, 260), (300, 128), (1027, 64)]
COS_FORMS = ("cos_rowloss_fwd", "cos_rowloss_fwd + vec_sum", "cos_rowloss_bwd")


def cos_data(n, D):
    """x, y (n, D) fp32 on the CPU; where there are rows to spare: a zero x row, a zero y row and an x row of norm 1e-20."""
    g = torch.Generator().manual_seed(7 * n + D)
    x = torch.randn(n, D, generator=g) * 0.8
    y = torch.randn(n, D, generator=g) * 1.3 + 0.2 * x
    if n >= 5:
        x[1] = 0.0
        y[2] = 0.0
        x[3] = x[3] * (1e-20 / float(x[3].double().norm()))
        x[4] = 0.0
        y[4] = 0.0
    return x, y


def cos_bounds(D, rf, rb):
    Ls = D / 64 + 7
    b_row = MARGIN * U_F * (2 * (Ls + 1) * rf["mdot"] + 2 * rf["cos"].abs() * (Ls + 8) + 2 + 2 * rf["cos"].abs())
    b_dx = MARGIN * U_F * ((Ls + 12) * rb["t1"] + (2 * Ls + 14) * rb["t2"] + (Ls + 1) * rb["t3"])
    return b_row, b_dx


@pytest.mark.parametrize("n,D", COS_CASES, ids=["%dx%d" % s for s in COS_CASES])
def test_cos_rowloss_forms_against_fp64(n, D):
    from druglamp_amd import _lib, ops
    L = _lib.lib()
    name = "cos_%dx%d" % (n, D)
    xc, yc = cos_data(n, D)
    x, y = guard(xc.to(DEV)), guard(yc.to(DEV))
    gscale = 1.0 / n
    rf, rb = R.cos_rows(x, y), R.cos_rows_bwd(x, y, gscale)
    b_row, b_dx = cos_bounds(D, rf, rb)
    for with_sum in (False, True):
        (row_b, row), (sum_b, tot) = out((n,)), out((1,))
        _twice(name, "forward", (row_b, sum_b),
               lambda: _rc(L.dl_cos_rowloss_fwd(x.data_ptr(), y.data_ptr(), row_b.ptr(), sum_b.ptr() if with_sum else None, n, D,
                                                ops._stream()), "dl_cos_rowloss_fwd"))
        check(name, COS_FORMS[1 if with_sum else 0], "row_loss", F32, row, rf["row_loss"], b_row)
        if n >= 5:                                      # the eps branches: a zero row on either side gives exactly 2
            assert float(row[1]) == 2.0 and float(row[2]) == 2.0 and float(row[4]) == 2.0
        if with_sum:
            own = row.double()
            check(name, COS_FORMS[1], "loss_sum", F32, tot, own.sum().reshape(1), (n * U_F * own.abs().sum()).reshape(1))
        else:
            sum_b.mask.zero_()
            sum_b.untouched(name, "loss_sum (not asked for)")
    dx_b, dx = out((n, D))
    _twice(name, "backward", (dx_b,),
           lambda: _rc(L.dl_cos_rowloss_bwd(x.data_ptr(), y.data_ptr(), gscale, dx_b.ptr(), n, D, ops._stream()), "dl_cos_rowloss_bwd"))
    check(name, COS_FORMS[2], "dx", F32, dx, rb["dx"], b_dx)


def test_cos_rowloss_fn_with_a_row_gradient_against_fp64():
    """CosRowLossFn under a non-uniform upstream gradient: the kernel runs with scale 1, the rows are scaled in fp32."""
    from druglamp_amd import functional as Fn
    n, D = 300, 128
    xc, yc = cos_data(n, D)
    x, y = guard(xc.to(DEV)).requires_grad_(True), guard(yc.to(DEV))
    wt = (torch.arange(n, device=DEV, dtype=F32) % 7 - 3.0) * 0.37
    rows = Fn.CosRowLossFn.apply(x, y)
    (rows * wt).sum().backward()
    rf, rb = R.cos_rows(x.detach(), y), R.cos_rows_bwd(x.detach(), y, 1.0)
    b_row, b_dx = cos_bounds(D, rf, rb)
    check("cos_fn_300x128", COS_FORMS[0], "row_loss", F32, rows.detach(), rf["row_loss"], b_row)
    ref = rb["dx"] * wt.double().unsqueeze(1)
    check("cos_fn_300x128", COS_FORMS[2], "dx (row gradient)", F32, x.grad, ref, b_dx * wt.double().abs().unsqueeze(1) + MARGIN * U_F * ref.abs())


# ==== cross entropy over rows =================================================================================================
CeCase = collections.namedtuple("CeCase", "name forms dt ld C Cp ldd off N ignore kind labels")
CE32, CEB, CEF = ("ce_rows32_fwd", "ce_rows32_bwd"), ("ce_rows_fwd<bf16>", "ce_rows_bwd<bf16>"), ("ce_rows_fwd<float>", "ce_rows_bwd<float>")
CE_CASES = [
    CeCase("fast_c27_n1000_ign0", CE32, BF, 32, 27, 32, 32, 0, 1000, 0, "x3", "rand"),
    CeCase("fast_c32_n256_ign-100", CE32, BF, 32, 32, 32, 32, 0, 256, -100, "x3", "rand"),
    CeCase("fast_c1_n257_ign-100", CE32, BF, 32, 1, 32, 32, 0, 257, -100, "x3", "rand"),
    CeCase("fast_c27_n256_big", CE32, BF, 32, 27, 32, 32, 0, 256, 0, "big", "rand"),
    CeCase("fast_c27_n1_ign-100", CE32, BF, 32, 27, 32, 32, 0, 1, -100, "x3", "rand"),
    CeCase("misaligned_c27_n255_falls_back", CEB, BF, 32, 27, 32, 32, 4, 255, 0, "x3", "rand"),
    CeCase("bf16_ld48_c40_n257", CEB, BF, 48, 40, 48, 48, 0, 257, -100, "x3", "rand"),
    CeCase("bf16_ld32_ldd40_c27_n255", (CE32[0], CEB[1]), BF, 32, 27, 32, 40, 0, 255, 0, "x3", "rand"),
    CeCase("f32_ld5_c5_n1", CEF, F32, 5, 5, 5, 5, 0, 1, -100, "x3", "rand"),
    CeCase("f32_ld5_c5_n257_ign0", CEF, F32, 5, 5, 5, 5, 0, 257, 0, "x3", "rand"),
    CeCase("f32_ld40_c27_cp32_ldd40_n1000_big", CEF, F32, 40, 27, 32, 40, 0, 1000, 0, "big", "rand"),
    CeCase("fast_all_ignored_n255", CE32, BF, 32, 27, 32, 32, 0, 255, 0, "x3", "all_ignored"),
    CeCase("f32_label_out_of_range_n257", CEF, F32, 40, 27, 32, 40, 0, 257, -100, "x3", "one_bad"),
    CeCase("fast_label_out_of_range_n256", CE32, BF, 32, 27, 32, 32, 0, 256, 0, "x3", "one_bad"),
]


def ce_data(c):
    g = torch.Generator().manual_seed(sum(map(ord, c.name)))
    x = torch.randn(c.N, c.C, generator=g) * 3.0
    if c.kind == "big" and c.C >= 2:                    # one +80 and one -80 entry per row
        hi = torch.randint(0, c.C, (c.N,), generator=g)
        lo = (hi + 1 + torch.randint(0, c.C - 1, (c.N,), generator=g)) % c.C
        x[torch.arange(c.N), hi] = 80.0
        x[torch.arange(c.N), lo] = -80.0
    y = torch.randint(0, c.C, (c.N,), generator=g)
    if c.labels == "all_ignored":
        y[:] = c.ignore
    elif c.labels == "one_bad":
        y[c.N // 2] = c.C if c.ignore != c.C else c.C + 1
    elif c.ignore < 0 and c.N > 3:
        y[::3] = c.ignore
    return x.to(c.dt), y


@pytest.mark.parametrize("c", CE_CASES, ids=[c.name for c in CE_CASES])
def test_ce_rows_form_against_fp64(c):
    from druglamp_amd import _lib, ops
    L = _lib.lib()
    dtc = _lib.DL_BF16 if c.dt == BF else _lib.DL_F32
    xc, yc = ce_data(c)
    N, C = c.N, c.C
    lg = Buf(N * c.ld + c.off, c.dt)
    x = lg.view((N, C), (c.ld, 1), c.off)               # the columns [C, ld) stay NaN: a pad column that is used poisons
    x.copy_(xc.to(DEV))
    y = guard(yc.to(DEV), fill=C + 5)
    nws = L.dl_ce_rows_workspace_bytes(N)
    (lse_b, lse), (o2_b, o2), (ws_b, _ws) = out((N,)), out((2,)), out((nws // 4,))
    _twice(c.name, "forward", (lse_b, o2_b, ws_b),
           lambda: _rc(L.dl_ce_rows_fwd(lg.ptr(c.off), c.ld, y.data_ptr(), N, C, c.ignore, dtc, lse_b.ptr(), o2_b.ptr(), ws_b.ptr(), nws,
                                        ops._stream()), "dl_ce_rows_fwd"))
    r = R.ce_rows(x, y, C, c.ignore)
    b_lse = MARGIN * U_F * (C + 6 + 4 * r["mag_lse"])
    check(c.name, c.forms[0], "lse", c.dt, lse, r["lse"], b_lse)
    assert float(o2[1]) == r["count"], "%s: counted rows %g, reference %d" % (c.name, float(o2[1]), r["count"])
    if math.isnan(r["mean"]):
        assert math.isnan(float(o2[0])), "%s: the mean must be NaN (all ignored / a label out of range)" % c.name
    else:
        nb = (N + 255) // 256
        b_mean = MARGIN * ((b_lse / MARGIN + U_F * r["mag_loss"])[r["valid"]].sum() + (20 + nb / 256) * U_F * r["row_loss"].abs().sum()) / r["count"]
        check(c.name, c.forms[0] + " + ce_rows_final", "mean", c.dt, o2[:1], torch.tensor([r["mean"]], dtype=F64, device=DEV), b_mean.reshape(1))
    # ---- backward ----
    gout = guard(torch.tensor([0.625], device=DEV))
    dl = Buf(N * c.ldd + c.off, c.dt)
    d = dl.view((N, c.Cp), (c.ldd, 1), c.off)
    _twice(c.name, "backward", (dl,),
           lambda: _rc(L.dl_ce_rows_bwd(lg.ptr(c.off), c.ld, y.data_ptr(), N, C, c.ignore, dtc, lse_b.ptr(), o2_b.ptr(), gout.data_ptr(),
                                        dl.ptr(c.off), c.ldd, c.Cp, ops._stream()), "dl_ce_rows_bwd"))
    rb = R.ce_rows_bwd(x, y, C, c.ignore, lse, r["count"], float(gout), c.Cp)
    coh = MARGIN * U_F * (8 + 2 * rb["xl"]) * rb["mag"]
    floor = (1.0 + abs(float(gout)) / max(r["count"], 1)) * 2.0 ** -126
    check(c.name, c.forms[1], "dlogits", c.dt, d, rb["dlogits"], coh + MARGIN * (U_B if c.dt == BF else 0.0) * rb["mag"] + floor, coh)
    zero = rb["mag"] == 0                               # ignored rows, rows with a bad label, the columns [C, Cp): exactly +0
    zb = d[zero].contiguous().view(torch.int16 if c.dt == BF else torch.int32)
    assert bool((zb == 0).all()), "%s: a dlogits element that must be zero is not" % c.name


# ==== triplet loss ============================================================================================================
TriCase = collections.namedtuple("TriCase", "name n_p n_d dim margin seed")
TRI_FORMS = ("row_norm + sigcos_dist", "triplet_reduce + triplet_final", "triplet_reduce(coef) + triplet_bwd_p", "triplet_reduce(coef) + triplet_bwd_d")
TRI_CASES = [
    TriCase("tri_1x5_dim4", 1, 5, 4, 0.25, 0),
    TriCase("tri_7x33_dim256", 7, 33, 256, 0.3, 0),
    TriCase("tri_5x64_dim70", 5, 64, 70, 0.25, 0),
    TriCase("tri_3x300_dim64", 3, 300, 64, 0.3, 0),
    TriCase("tri_2x8192_dim8", 2, 8192, 8, 0.25, 0),
]


def tri_data(c):
    """p, d (fp32) and the label matrix (int8) on the CPU.  Rows share a 3-dimensional latent so that the cosines spread over
    (-1, 1) and hinges fall on both sides of zero.  Anchor 0 has no positive (anchor-as-positive branch); with five or more
    anchors, anchor 1 has no negative and anchor 2 is all ignored; with three, anchor 0 is a regular one (more than 256
    triplets), anchor 1 has no positive and anchor 2 no negative; the 8192-column case has three positives in anchor 0 and
    none in anchor 1."""
    g = torch.Generator().manual_seed(1000 * c.n_p + c.n_d + 17 * c.seed)
    W = torch.randn(3, c.dim, generator=g)
    p = torch.randn(c.n_p, 3, generator=g) @ W + 0.3 * torch.randn(c.n_p, c.dim, generator=g)
    d = torch.randn(c.n_d, 3, generator=g) @ W + 0.3 * torch.randn(c.n_d, c.dim, generator=g)
    u = torch.rand(c.n_p, c.n_d, generator=g)
    gt = torch.where(u < 0.3, -1, torch.where(u < 0.7, 0, 1)).to(torch.int8)
    if c.n_d == 8192:
        gt[:] = 0
        gt[0, [5, 4100, 8191]] = 1
    elif c.n_p == 3:                                    # anchor 0 keeps positives and negatives: > 256 triplets
        gt[1][gt[1] == 1] = 0
        gt[2][gt[2] == 0] = 1
    else:
        gt[0][gt[0] == 1] = 0
        if c.n_p >= 5:
            gt[1][gt[1] == 0] = 1
            gt[2] = -1
    return p, d, gt


def tri_bounds(c, r):
    Ls = c.dim / 64 + 7
    b_dist = MARGIN * U_F * ((Ls * r["mdot"] + (Ls + 6) * r["cos"].abs() + 2) / 4 + 3)
    return Ls, b_dist


def triplet_conditions(c, r):
    """No hinge argument within 4 x the distance bound of zero: the kernels' active set is the reference's."""
    Ls, b_dist = tri_bounds(c, r)
    if r["hv"].numel():
        lo = float(r["hv"].abs().min())
        assert lo > 4 * float(b_dist.max()), "%s: a hinge argument of %.3g is ambiguous (distance bound %.3g)" % (c.name, lo, float(b_dist.max()))
        assert bool((r["hv"] > 0).any())
    return Ls, b_dist


@pytest.mark.parametrize("c", TRI_CASES, ids=[c.name for c in TRI_CASES])
def test_triplet_sigcos_against_fp64(c):
    from druglamp_amd import _lib, ops
    L = _lib.lib()
    pc, dc, gtc = tri_data(c)
    n_p, n_d, dim = c.n_p, c.n_d, c.dim
    p, d, gt = guard(pc.to(DEV)), guard(dc.to(DEV)), guard(gtc.to(DEV), fill=1)
    r = R.triplet(p, d, gt, c.margin)
    Ls, b_dist = triplet_conditions(c, r)
    nf = L.dl_triplet_sigcos_buffer_floats(n_p, n_d)
    assert nf == 3 * n_p * n_d + 4 * n_p + n_d
    (buf_b, buf), (loss_b, loss), (nt_b, ntri) = out((nf,)), out((1,)), out((1,))
    _twice(c.name, "forward", (buf_b, loss_b, nt_b),
           lambda: _rc(L.dl_triplet_sigcos_fwd(p.data_ptr(), d.data_ptr(), gt.data_ptr(), n_p, n_d, dim, c.margin, buf_b.ptr(), loss_b.ptr(),
                                               nt_b.ptr(), ops._stream()), "dl_triplet_sigcos_fwd"))
    check(c.name, TRI_FORMS[0], "dist", F32, buf[:n_p * n_d].reshape(n_p, n_d), r["dist"], b_dist)
    assert float(ntri) == max(r["n_tri"], 1), "%s: %g triplets, reference %d" % (c.name, float(ntri), r["n_tri"])
    pos, neg = (gt == 1).sum(1), (gt == 0).sum(1)
    t_max = int(torch.where(pos > 0, pos * neg, neg).max())
    n_act = int((r["hv"] > 0).sum())
    b_loss = MARGIN * ((t_max / 256 + 12 + n_p) * U_F * r["hinge_sum"] + n_act * (2 * float(b_dist.max()) / MARGIN + 3 * U_F)) / max(r["n_tri"], 1)
    check(c.name, TRI_FORMS[1], "loss", F32, loss, torch.tensor([r["loss"]], dtype=F64, device=DEV), torch.tensor([b_loss], dtype=F64, device=DEV))
    # ---- backward: reuses the forward's scratch (norms, cosines, distances) and rewrites the coefficients ----
    (dp_b, dp), (dd_b, dd) = out((n_p, dim)), out((n_d, dim))
    gout = 0.75

    def bwd():
        _rc(L.dl_triplet_sigcos_bwd(p.data_ptr(), d.data_ptr(), gt.data_ptr(), buf_b.ptr(), n_p, n_d, dim, c.margin, nt_b.ptr(), gout,
                                    dp_b.ptr(), dd_b.ptr(), ops._stream()), "dl_triplet_sigcos_bwd")
    _twice(c.name, "backward", (dp_b, dd_b), bwd)
    buf_b.untouched(c.name, "scratch after the backward")
    coef = buf[2 * n_p * n_d + 3 * n_p: 3 * n_p * n_d + 3 * n_p].reshape(n_p, n_d).double()
    assert torch.equal(coef, r["coef"]), "%s: the hinge coefficients differ from the reference's active set" % c.name
    check(c.name, TRI_FORMS[2], "dp", F32, dp, gout * r["dp"], MARGIN * (n_d + 3 * Ls + 20) * U_F * gout * r["mag_dp"])
    check(c.name, TRI_FORMS[3], "dd", F32, dd, gout * r["dd"], MARGIN * (n_p + 3 * Ls + 20) * U_F * gout * r["mag_dd"])
