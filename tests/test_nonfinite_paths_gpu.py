"""How NaN and +-inf pass through the kernels: the contract of DESIGN.md ("Non-finite values"),

    a non-finite value is never turned into a finite one on the way from a kernel's inputs to its outputs,
    and it never leaks into outputs that do not depend on it,

one parametrised case per launch form, on the smallest case of that form of the existing fp64 suites (the same data, the same
guarded buffers, the same launch through the C ABI), checked by tests/nonfinite_ref.py against the repository's own fp64
references.  A case runs clean once, then once per plant: ONE element of ONE floating-point operand replaced by NaN (or by
+-inf where the value has a meaning: activation pre-activations through X or the bias, logits, normalisation inputs, AdamW
gradients).  Integer operands, by-value arguments and saved forward tensors (pre-activations, ReLU mask sources, saved
log-sum-exp, saved mean / rstd) are never planted: a non-finite value there means the forward already carried it to the loss.

Every case object is built by make(device): tests/test_nonfinite_reference_cpu.py builds the same operands on the CPU and
asserts from the references alone that no case is vacuous (at least one poisoned and one untouched output element) and that
each case takes the launch form it names.

Families here: GEMM (every epilogue and tile family), LayerNorm, BatchNorm (training statistics, apply, fused ReLU, backward),
attention forward and backward, the pair-indexed PGCA forward, the cosine row loss and cross entropy, the token gate, GELU backward, AdamW, cast, adjacency normalisation, graph
aggregation, and end to end the training step and library screening.

`moved` elements (finite in the planted reference, but changed).  profiles/nonfinite_sites.txt lists them per form; they arise in
five places only, and each Side states its bound in bound():
  gemm      behind a ReLU of -inf (an exact zero): the roundings of the dropout scale, the residual, old C and the store
  ce        a -inf logit is a masked class: the loss suite's own bounds of lse, the mean and dlogits on the planted reference
  gate      a -inf logit is a masked token: the elem suite's relative gate bound without the masked token's infinite exponent;
            `out` = v (gate + res): finite only (its bound multiplies the gate's, whose masked term is 0 x inf)
  fill_pool a NaN in an all-zero row clears its fill bit: exactly 0
  triplet   a NaN hinge is a closed ReLU in the backward, so the other drugs' gradients lose its coefficient: finite only (the
            suite's bound multiplies mag_dd, whose terms with the NaN cosine are not numbers)
Everywhere else (LayerNorm, BatchNorm, AdamW, attention with +inf in V, the movers) a +-inf plant moves nothing: inf - inf and
inf / inf make the whole row, channel or element NaN in the reference, and the table shows moved = 0 for those rows.

DL_NONFINITE_LOG=<file>: one JSON line per check; tools/nonfinite_sites.py reduces it to profiles/nonfinite_sites.txt.
"""
import collections
import contextlib
import ctypes as C
import functools
import math
import struct

import pytest
import torch

from tests import elem_ref as er
from tests import gemm_ref as GR
from tests import loss_ref as LR
from tests import nonfinite_ref as NF
from tests import norm_ref as nr
from tests import test_attention_paths_gpu as A
from tests import test_attention_probs_gpu as AP
from tests import test_elem_paths_gpu as E
from tests import test_gemm_paths_gpu as G
from tests import test_loss_paths_gpu as LS
from tests import test_norm_paths_gpu as N
from tests import bn_eval_ref as ber
from tests import test_bn_eval_bwd_gpu as BE
from tests import attr_ref
from tests import test_pgca_pairs_attr_gpu as AT
from tests import test_pgca_pairs_gpu as PG
from tests import test_pgca_pairs_probs_gpu as PP
from tests import test_pgca_pairs_profile_gpu as PF
from tests import test_pgca_ragged_gpu as RG
from tests.profile_ref import profile_ref

DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U_B, U_F, MARGIN = 2.0 ** -8, 2.0 ** -24, 2.0
NAN, PINF, NINF = "nan", "+inf", "-inf"

Case = collections.namedtuple("Case", "name family form make plants")
Plant = collections.namedtuple("Plant", "operand index value")


def u_st(dt):
    return U_B if dt == BF else U_F


@contextlib.contextmanager
def planted(tensors, index, value):
    """The same element of every tensor of `tensors` (a device operand and, where the reference reads one, its host mirror)
    replaced by `value`; put back afterwards."""
    saved = [NF.plant(t, index, value) for t in tensors]
    try:
        yield
    finally:
        for t, old in zip(tensors, saved):
            t[index] = old


def _gpu(dev):
    return torch.device(dev).type == "cuda"


def _lib():
    return N._lib()


class Side:
    """One case's operands on one device.  operands: {name: [tensors the plant goes into]}; run(): the kernels' outputs
    (clones of the addressed elements; GPU only); ref(): the fp64 references of the same outputs from the operands as they are
    now; bound(what, ref_planted): the bound of moved elements or None."""
    operands = {}
    everything_depends = False      # True: every output depends on every planted element (no untouched element can exist)
    nan_as_inf = None               # a reason (text): this case may return an infinity where the reference has NaN; None: a failure

    def bound(self, what, refs):
        return None


# ==== driver ======================================================================================================================
def _tag(pl):
    f = lambda i: ":" if isinstance(i, slice) else ("+".join(map(str, i)) if isinstance(i, (list, tuple)) else str(i))
    return "%s@%s=%s" % (pl.operand, ",".join(f(i) for i in pl.index), pl.value)


def classify_case(case, side):
    """CPU and GPU: per plant, the references of every output, clean and planted; asserts that the plant is not vacuous."""
    clean = side.ref()
    out = []
    for pl in case.plants:
        with planted(side.operands[pl.operand], pl.index, pl.value):
            refs = side.ref()
        tag = _tag(pl)
        NF.assert_not_vacuous(case.name, tag, [(clean[k], refs[k]) for k in clean], masking=pl.value == NINF,
                              need_untouched=not side.everything_depends)
        out.append((pl, tag, refs))
    return clean, out


def drive(case):
    side = case.make(DEV)
    got_clean = side.run()
    ref_clean = side.ref()
    assert set(got_clean) == set(ref_clean)
    for pl in case.plants:
        tag = _tag(pl)
        with planted(side.operands[pl.operand], pl.index, pl.value):
            got, refs = side.run(), side.ref()
            NF.assert_not_vacuous(case.name, tag, [(ref_clean[k], refs[k]) for k in ref_clean], masking=pl.value == NINF,
                                  need_untouched=not side.everything_depends)
            for what in ref_clean:
                b = side.bound(what, refs)
                NF.check_nonfinite(case.name, case.form, what, got_clean[what], got[what], ref_clean[what], refs[what],
                                   (lambda moved, b=b: b) if b is not None else None, tag, allow_nan_as_inf=side.nan_as_inf is not None)
    again = side.run()                                     # the operands are back: the clean result, bit for bit
    for what in got_clean:
        assert torch.equal(NF.bits(again[what]), NF.bits(got_clean[what])), "%s: %s differs after the plants were removed" % (case.name, what)


# ==== GEMM ========================================================================================================================
GEMM_BY_NAME = {c.name: c for c in G.CASES}
# (case of tests/test_gemm_paths_gpu.py, what it is here for)
GEMM_PICK = [
    ("k_f32_epi0", "epi0"), ("k_bf_epi2", "epi2, polynomial GELU, dropout"), ("k_f32_epi2", "epi2, erf GELU"), ("k_f32_epi3", "epi3 residual"),
    ("k_bf_epi4", "epi4: planted through the incoming gradient only"), ("k_bf_epi5", "epi5 ReLU"), ("k_f32_epi5", "epi5 ReLU fp32"),
    ("k_bf_epi1_n36", "general epilogue, act 1"), ("k_bf_epi1_relu_res", "general epilogue, act 2 + residual"),
    ("r_f32_x0w0_epi1", "general epilogue, act 2, register staging"), ("k_bf_epi1_accumulate", "old C"),
    ("k_f32_epi1_res_before", "residual before dropout"), ("big_epi5_192tiles", "big256 epi5"), ("lat_epi5_130x136", "lat128 epi5"),
    ("s_f32_split3", "split-K + reduce"), ("s_bf_auto_tw2_cs", "split-K tw2 + x_colsum"), ("tt256_bf16out_cs", "tt2 + x_colsum"),
    ("group_bm128_mixed", "group"), ("pair_bf_epi2", "pair"),
]


def _gemm_flat(t, ld, dev):
    """The storage of a logical operand at its pitch (gaps zero: the reference never reads them)."""
    if t.dim() == 1:
        return t.to(dev)
    f = torch.zeros(G.storage_span(t.shape[0], t.shape[1], ld), dtype=t.dtype, device=dev)
    torch.as_strided(f, tuple(t.shape), (ld, 1)).copy_(t)
    return f


def gemm_plants(c):
    """Plants of one product (member index 0 of a group / pair): interior of a full tile, the last addressed row / column /
    k, every floating-point operand in turn; +-inf through X and the bias where an activation follows."""
    M, N_, K = c.M, c.N, c.K
    xi = lambda i, k: (k * c.ldx + i,) if c.xs else (i * c.ldx + k,)
    wi = lambda j, k: (k * c.ldw + j,) if c.ws else (j * c.ldw + k,)
    ps = [Plant("X", xi(min(5, M - 1), min(7, K - 1)), NAN), Plant("X", xi(M - 1, K - 1), NAN), Plant("W", wi(N_ - 1, K - 1), NAN)]
    if c.exact:                                            # integer operands with zeros: inf x 0 would be NaN on both sides; NaN only
        return ps
    if c.bias:
        ps.append(Plant("bias", (N_ - 1,), NAN))
    if c.res:
        col = N_ - 1
        if c.res == "before" and c.p > 0:                  # a residual added before the dropout is dropped with its element: a kept one
            keep = GR.keep_mask(c.seed, 0, M, N_, c.p)
            col = int(keep[M - 1].nonzero()[0][-1])
        ps.append(Plant("res", ((c.rmod or M) - 1, col), NAN))
    if c.acc:
        ps.append(Plant("old", (min(5, M - 1), min(9, N_ - 1)), NAN))
    if c.act:
        ps += [Plant("X", xi(M - 2, 1), PINF), Plant("X", xi(min(3, M - 1), K - 1), NINF)]
        if c.bias:
            ps += [Plant("bias", (3,), PINF), Plant("bias", (N_ - 2,), NINF)]
    return ps


class GemmSide(Side):
    def __init__(self, c, dev):
        self.c, self.members = c, getattr(c, "members", [c])
        self.gpu = _gpu(dev)
        self.dev = dev
        if self.gpu:
            self.probs = [G.Prob(q) for q in self.members]
            self.fx, self.fw, self.d = [p.x for p in self.probs], [p.w for p in self.probs], [p.d for p in self.probs]
        else:
            self.d = [G.gen(q) for q in self.members]
            self.fx = [_gemm_flat(d["X"], q.ldx, dev) for d, q in zip(self.d, self.members)]
            self.fw = [_gemm_flat(d["W"], q.ldw, dev) for d, q in zip(self.d, self.members)]
        d0 = self.d[0]
        self.operands = {"X": [self.fx[0]], "W": [self.fw[0]]}
        for key in ("bias", "res", "old"):
            if key in d0:
                self.operands[key] = [d0[key]]
        if self.gpu:
            p = self.probs[0]
            if "bias" in d0:
                self.operands["bias"].append(p.kw["bias"])
            if "res" in d0:
                self.operands["res"].append(p.kw["residual"])
            if "old" in d0:
                self.operands["old"].append(p.outs["C"].old)
        self._r = None
        if any(q.act == 1 and q.bf_in for q in self.members):
            self.nan_as_inf = "polynomial GELU of the bf16 epilogues: -inf x Phi(-4.3) = -inf x 8e-6 = -inf where erf gives -inf x 0 = NaN"

    def _key(self, i, what):
        return what if len(self.members) == 1 else "%s/%s" % (self.members[i].name, what)

    def ref(self):
        out, self._r = {}, []
        for i, q in enumerate(self.members):
            r, _ = G.reference(q, self.fx[i], self.fw[i], self.d[i], self.dev)
            self._r.append(r)
            out[self._key(i, "C")] = r["C"]
            if q.pre:
                out[self._key(i, "pre_out")] = r["pre"]
            if q.cs:
                out[self._key(i, "x_colsum")] = r["x_colsum"][None, :]
        return out

    def bound(self, what, refs):
        """Moved elements arise behind a ReLU of -inf: an exact zero, then the dropout scale, the residual and old C, one
        rounding each, and the store."""
        if not what.endswith("C"):
            return None
        i = 0 if len(self.members) == 1 else [q.name for q in self.members].index(what.split("/")[0])
        q, r = self.members[i], self._r[i]
        z = lambda t: torch.nan_to_num(t.abs(), nan=0.0, posinf=0.0, neginf=0.0)
        mag = z(r["dropped"]) + z(r["C"]) + (z(r["res"]) if "res" in r else 0.0) + (z(self.d[i]["old"].to(self.dev).double()) if q.acc else 0.0)
        return MARGIN * (U_F * mag + u_st(BF if q.bf_out else F32) * z(r["C"]))

    def run(self):
        from druglamp_amd import _lib, ops
        c, probs = self.c, self.probs
        if c.kind == "gemm":
            launch = probs[0].launch
        elif c.kind == "pair":
            def launch():
                (a0, _), (a1, _) = probs[0].args(), probs[1].args()
                G.assert_twin(a0, a1)
                _lib.check(_lib.lib().dl_gemm_pair(C.byref(a0), C.byref(a1), ops._stream()), "dl_gemm_pair")
        else:
            def launch():
                with ops.deferred_reductions():
                    for p in probs:
                        ops.gemm(p.x, p.w, **p.kw)
                    assert len(ops._wgroup) == len(probs), "the products did not queue up as a weight-gradient group"
        G._twice(c.name, probs, launch)                    # refill, launch, nothing outside [M, N] written, bitwise repeatable
        return {self._key(i, what): b.inner.clone() for i, p in enumerate(probs) for what, b in p.outs.items()}


def _gemm_case(name, why):
    c = GEMM_BY_NAME[name]
    return Case("gemm/" + name, "gemm", c.form, functools.partial(GemmSide, c), gemm_plants(getattr(c, "members", [c])[0]))


GEMM_CASES = [_gemm_case(n, w) for n, w in GEMM_PICK]


# ==== LayerNorm ===================================================================================================================
LN_BY_NAME = {c.name: c for c in N.LN_CASES}
LN_PICK = ["v16_256_m33_slice_of_768", "v16_512_m47_pitch520", "bf16_d36_m7", "bf16_d264_m9", "bwd_m33_out_slice", "bf16_d1028_m130",
           "f32_d4_m130", "f32_d260_m9", "f32_d1024_m9", "f32_d2048_m7", "bwd16_share7_m63"]


def _guarded_view(lay, M, D, dt, dev, values=None):
    g = N.Guarded((M + 3) * lay.ld + lay.shift, dt, dev)
    v = g.view((M, D), (lay.ld, 1), lay.shift + lay.off)
    if values is not None:
        v.copy_(values)
    return g, v


def _place(values, dt, dev):
    g = N.Guarded(values.numel(), dt, dev)
    v = g.view(tuple(values.shape))
    v.copy_(values)
    return v


def _outbuf(shape, dt, dev):
    g = N.Guarded(int(math.prod(shape)), dt, dev)
    return g, g.view(tuple(shape))


class LnSide(Side):
    """dl_layernorm_fwd on x, then dl_layernorm_bwd on (dy, x, dres) with the CLEAN statistics as saved operands."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        dt, D, M = c.dt, c.D, c.M
        g = torch.Generator().manual_seed(sum(map(ord, c.name)))
        xv, _ = N.ln_data(c.data, M, D, g)
        _, self.x = _guarded_view(c.lay, M, D, dt, dev, xv)
        self.gamma = _place(1.0 + 0.5 * torch.randn(D, generator=g), F32, dev)
        self.beta = _place(0.5 * torch.randn(D, generator=g), F32, dev)
        _, rmean, rrstd, _ = nr.ln_fwd(self.x, self.gamma, self.beta, N.EPS)
        self.mean_in, self.rstd_in = _place(rmean.float(), F32, dev), _place(rrstd.float(), F32, dev)
        Mdy = M // c.share
        _, self.dy = _guarded_view(c.lay, Mdy, D, dt, dev, torch.randn(Mdy, D, generator=g))
        self.dres = _guarded_view(c.lay, M, D, dt, dev, 0.5 * torch.randn(M, D, generator=g))[1] if c.dres else None
        self.operands = {"x": [self.x], "dy": [self.dy]}
        if c.dres:
            self.operands["dres"] = [self.dres]

    def forms(self):
        c, gen = self.c, N._gen(self.c.dt, self.c.D)
        _, y = _guarded_view(c.lay, c.M, c.D, c.dt, self.dev)
        _, dx = _guarded_view(c.out, c.M, c.D, c.dt, self.dev)
        f16 = N._is16(c.dt, c.D, (self.x, y), (self.gamma, self.beta))
        b16 = N._is16(c.dt, c.D, [self.dy, self.x, dx] + ([self.dres] if c.dres else []), (self.gamma,))
        return ("ln_fwd16<%d>" % c.D) if f16 else gen[0], ("ln_bwd16<%d>" % c.D) if b16 else gen[1]

    def ref(self):
        c = self.c
        y, mean, rstd, _ = nr.ln_fwd(self.x, self.gamma, self.beta, N.EPS)
        dx, dg, db, _ = nr.ln_bwd(self.dy, self.x, self.gamma, self.dres, c.share, mean=self.mean_in, rstd=self.rstd_in)
        return {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dgamma": dg, "dbeta": db}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c, dev = self.c, self.dev
        dt, D, M = c.dt, c.D, c.M
        x, dy, dres = self.x, self.dy, self.dres
        yg, y = _guarded_view(c.lay, M, D, dt, dev)
        (mg, mean), (rg, rstd) = _outbuf((M,), F32, dev), _outbuf((M,), F32, dev)
        dxg, dx = _guarded_view(c.out, M, D, dt, dev)
        gbg, gb = _outbuf((2, D), F32, dev)
        bufs = (yg, mg, rg, dxg, gbg)
        before = [b.bits() for b in bufs]
        ok(L.dl_layernorm_fwd(x.data_ptr(), x.stride(0), self.gamma.data_ptr(), self.beta.data_ptr(), y.data_ptr(), y.stride(0), mean.data_ptr(),
                              rstd.data_ptr(), M, D, N.EPS, DT[dt], stream), "dl_layernorm_fwd")
        ws = torch.empty(L.dl_layernorm_bwd_workspace_bytes(M, D), dtype=torch.uint8, device=dev)
        ok(L.dl_layernorm_bwd(dy.data_ptr(), dy.stride(0), c.share, x.data_ptr(), x.stride(0), self.mean_in.data_ptr(), self.rstd_in.data_ptr(),
                              self.gamma.data_ptr(), N._ptr(dres), 0 if dres is None else dres.stride(0), dx.data_ptr(), dx.stride(0),
                              gb[0].data_ptr(), gb[1].data_ptr(), 0, M, D, DT[dt], ws.data_ptr(), ws.numel(), None, stream), "dl_layernorm_bwd")
        torch.cuda.synchronize()
        for b, bb in zip(bufs, before):
            b.untouched(c.name, bb)
        return {"y": y.clone(), "mean": mean.clone(), "rstd": rstd.clone(), "dx": dx.clone(), "dgamma": gb[0].clone(), "dbeta": gb[1].clone()}


def _ln_case(name):
    c = LN_BY_NAME[name]
    M, D = c.M, c.D
    Mdy = M // c.share
    ps = [Plant("x", (min(3, M - 1), min(5, D - 1)), NAN), Plant("x", (M - 1, D - 1), NAN), Plant("x", (M // 2, D // 2), PINF),
          Plant("x", (M - 1, 0), NINF), Plant("dy", (min(2, Mdy - 1), min(6, D - 1)), NAN), Plant("dy", (Mdy - 1, D - 1), NAN)]
    if c.dres:
        ps.append(Plant("dres", (M - 1, D - 1), NAN))
    return Case("ln/" + name, "layernorm", "%s + %s" % (c.fwd, c.bwd), functools.partial(LnSide, c), ps)


LN_NF_CASES = [_ln_case(n) for n in LN_PICK]


# ==== BatchNorm ===================================================================================================================
BN_BY_NAME = {c.name: c for c in N.BN_CASES}
BN_PICK = ["wide128_r31_offset", "wide256_r33_relu", "bf16_c260_r33_spike", "f32_c128_r31", "f32_c4_r33_offset", "bf16_c72_win40_4_32x5",
           "wide64_rw_r100", "f32_c128_rw_r100"]


class BnSide(Side):
    """Training BatchNorm as the model chains it: dl_bn_stats_finalize on y (sums, mean, biased variance, rstd, the running
    statistics), dl_bn_finalize on those sums, the apply pass with the kernels' own statistics (plain and, without a row rule,
    dl_bn_apply_relu_fwd), and the backward on dz with the CLEAN statistics as saved operands: dl_bn_bwd_reduce, dl_bn_bwd_apply
    (relu_mask 0 / 1) and, without a row rule, dl_bn_relu_bwd."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        dt, Cc, R = c.dt, c.C, c.R
        g = torch.Generator().manual_seed(sum(map(ord, c.name)))
        w64, rw, self.rule = N._row_weights(c, g)
        self.w = w64.to(dev)
        self.rw = None if rw is None else _place(rw, F32, dev)
        self.n = int(w64.clamp_min(0).sum())
        self.y = _place(N.bn_data(c.data, R, Cc, g), dt, dev)
        self.dz = _place(torch.randn(R, Cc, generator=g), dt, dev)
        live = self.w >= 0
        self.y[~live] = float("nan")                       # excluded / halo rows are never read (as in the norm suite)
        self.dz[~live] = float("nan")
        self.gamma = _place(1.0 + 0.5 * torch.randn(Cc, generator=g), F32, dev)
        self.beta = _place(0.5 * torch.randn(Cc, generator=g), F32, dev)
        self.rm0 = _place(torch.randn(Cc, generator=g), F32, dev)
        self.rv0 = _place(torch.rand(Cc, generator=g) + 0.5, F32, dev)
        s0, s1, _ = nr.bn_sums(self.y, self.w)
        mean, _, rstd, _, _ = nr.bn_finalize(s0, s1, self.n, N.EPS)
        self.mean_s, self.rstd_s = _place(mean.float(), F32, dev), _place(rstd.float(), F32, dev)
        self.plain = c.rule[0] == "none"
        self.inv_n = N.f32(1.0 / self.n)
        self.operands = {"y": [self.y], "dz": [self.dz]}
        self.live_rows = [int(i) for i in live.nonzero().flatten()]

    def forms(self):
        return N._bn_forms(self.c.dt, self.c.C, (self.y, self.dz))

    def ref(self):
        y, dz, w = self.y, self.dz, self.w
        s0, s1, _ = nr.bn_sums(y, w)
        mean, var, rstd, rm, rv = nr.bn_finalize(s0, s1, self.n, N.EPS, N.MOMENTUM, self.rm0, self.rv0)
        out = {"sums": torch.cat([s0, s1]), "mean": mean, "var": var, "rstd": rstd, "running_mean": rm, "running_var": rv}
        out.update({"finalize " + k: out[k] for k in ("mean", "var", "rstd", "running_mean", "running_var")})
        out["z"], _ = nr.bn_apply(y, w, mean, rstd, self.gamma, self.beta)
        b0, b1, _ = nr.bn_bwd_sums(dz, y, w, self.mean_s, self.rstd_s)
        out["bwd sums"] = torch.cat([b0, b1])
        for rm_ in (0, 1):
            out["dy[relu_mask=%d]" % rm_], _ = nr.bn_bwd_apply(dz, y, w, self.mean_s, self.rstd_s, self.gamma, b0, b1, self.inv_n, bool(rm_))
        if self.plain:
            out["z relu"], _ = nr.bn_apply(y, w, mean, rstd, self.gamma, self.beta, relu=True)
            dy, r0, r1, _ = nr.bn_relu_bwd(dz, y, self.mean_s, self.rstd_s, self.gamma, self.beta, self.inv_n)
            out["relu_bwd dy"], out["relu_bwd sums"] = dy, torch.cat([r0, r1])
        return out

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c, dev = self.c, self.dev
        dt, Cc, R, n = c.dt, c.C, c.R, self.n
        win, halo, valid = self.rule
        y, dz, rw = self.y, self.dz, self.rw
        ws = torch.empty(L.dl_bn_workspace_bytes(R, Cc), dtype=torch.uint8, device=dev)
        wsa = (ws.data_ptr(), ws.numel(), stream)
        o = lambda shape, d=F32: _outbuf(shape, d, dev)
        B = {"sums": o((2 * Cc,)), "mean": o((Cc,)), "var": o((Cc,)), "rstd": o((Cc,)), "finalize mean": o((Cc,)), "finalize var": o((Cc,)),
             "finalize rstd": o((Cc,)), "z": o((R, Cc), dt), "bwd sums": o((2 * Cc,)), "dy[relu_mask=0]": o((R, Cc), dt), "dy[relu_mask=1]": o((R, Cc), dt)}
        if self.plain:
            B.update({"z relu": o((R, Cc), dt), "relu_bwd dy": o((R, Cc), dt), "relu_bwd sums": o((2 * Cc,))})
        run_stats = {k: _place(v, F32, dev) for k, v in (("running_mean", self.rm0), ("running_var", self.rv0), ("finalize running_mean", self.rm0),
                                                          ("finalize running_var", self.rv0))}
        before = {k: g.bits() for k, (g, _) in B.items()}
        P = {k: v.data_ptr() for k, (_, v) in B.items()}
        P.update({k: v.data_ptr() for k, v in run_stats.items()})
        ok(L.dl_bn_stats_finalize(y.data_ptr(), R, Cc, win, halo, valid, N._ptr(rw), DT[dt], n, N.EPS, N.MOMENTUM, P["sums"], P["mean"], P["var"],
                                  P["rstd"], P["running_mean"], P["running_var"], *wsa), "dl_bn_stats_finalize")
        ok(L.dl_bn_finalize(P["sums"], n, N.EPS, N.MOMENTUM, P["finalize mean"], P["finalize var"], P["finalize rstd"], P["finalize running_mean"],
                            P["finalize running_var"], Cc, stream), "dl_bn_finalize")
        g_, b_ = self.gamma.data_ptr(), self.beta.data_ptr()
        ms, rs = self.mean_s.data_ptr(), self.rstd_s.data_ptr()
        if rw is not None:
            ok(L.dl_bn_apply_fwd_rw(y.data_ptr(), P["z"], P["mean"], P["rstd"], g_, b_, R, Cc, rw.data_ptr(), DT[dt], stream), "dl_bn_apply_fwd_rw")
            ok(L.dl_bn_bwd_reduce_rw(dz.data_ptr(), y.data_ptr(), ms, rs, R, Cc, rw.data_ptr(), DT[dt], P["bwd sums"], *wsa), "dl_bn_bwd_reduce_rw")
            for m_ in (0, 1):
                ok(L.dl_bn_bwd_apply_rw(dz.data_ptr(), y.data_ptr(), ms, rs, g_, P["bwd sums"], self.inv_n, m_, P["dy[relu_mask=%d]" % m_], R, Cc,
                                        rw.data_ptr(), DT[dt], stream), "dl_bn_bwd_apply_rw")
        else:
            ok(L.dl_bn_apply_fwd(y.data_ptr(), P["z"], P["mean"], P["rstd"], g_, b_, R, Cc, win, halo, valid, DT[dt], stream), "dl_bn_apply_fwd")
            ok(L.dl_bn_bwd_reduce(dz.data_ptr(), y.data_ptr(), ms, rs, R, Cc, win, halo, valid, DT[dt], P["bwd sums"], *wsa), "dl_bn_bwd_reduce")
            for m_ in (0, 1):
                ok(L.dl_bn_bwd_apply(dz.data_ptr(), y.data_ptr(), ms, rs, g_, P["bwd sums"], self.inv_n, m_, P["dy[relu_mask=%d]" % m_], R, Cc, win, halo,
                                     valid, DT[dt], stream), "dl_bn_bwd_apply")
        if self.plain:
            ok(L.dl_bn_apply_relu_fwd(y.data_ptr(), P["z relu"], P["mean"], P["rstd"], g_, b_, R, Cc, DT[dt], stream), "dl_bn_apply_relu_fwd")
            ok(L.dl_bn_relu_bwd(dz.data_ptr(), y.data_ptr(), ms, rs, g_, b_, self.inv_n, P["relu_bwd dy"], P["relu_bwd sums"], R, Cc, DT[dt],
                                ws.data_ptr(), ws.numel(), stream), "dl_bn_relu_bwd")
        torch.cuda.synchronize()
        for k, (g, _) in B.items():
            g.untouched(c.name, before[k])
        out = {k: v.clone() for k, (_, v) in B.items()}
        out.update({k: v.clone() for k, v in run_stats.items()})
        return out


def _bn_case(name):
    c = BN_BY_NAME[name]
    g = torch.Generator().manual_seed(sum(map(ord, c.name)))
    w64, _, _ = N._row_weights(c, g)
    live = [int(i) for i in (w64 > 0).nonzero().flatten()]             # rows that take part in the statistics
    r0, r1 = live[min(2, len(live) - 1)], live[-1]
    Cc = c.C
    ps = [Plant("y", (r0, min(5, Cc - 1)), NAN), Plant("y", (r1, Cc - 1), NAN), Plant("y", (r0, 1), PINF), Plant("y", (r1, Cc - 2), NINF),
          Plant("dz", (r0, min(6, Cc - 1)), NAN), Plant("dz", (r1, Cc - 1), NAN)]
    return Case("bn/" + name, "batchnorm", " | ".join(c.forms) + (" | " + " | ".join(N.RELU_FORMS) if c.rule[0] == "none" else ""),
                functools.partial(BnSide, c), ps)


BN_NF_CASES = [_bn_case(n) for n in BN_PICK]


# ==== losses: cosine rows, cross entropy ==========================================================================================
class CosSide(Side):
    def __init__(self, n, D, dev):
        self.n, self.D, self.dev = n, D, dev
        xc, yc = LS.cos_data(n, D)
        self.x, self.y = _place(xc, F32, dev), _place(yc, F32, dev)
        self.operands = {"x": [self.x], "y": [self.y]}
        self.gscale = 1.0 / n

    def ref(self):
        rf, rb = LR.cos_rows(self.x, self.y), LR.cos_rows_bwd(self.x, self.y, self.gscale)
        return {"row_loss": rf["row_loss"], "loss_sum": rf["row_loss"].sum().reshape(1), "dx": rb["dx"]}

    def run(self):
        from druglamp_amd import _lib, ops
        L, n, D = _lib.lib(), self.n, self.D
        (row_b, row), (sum_b, tot), (dx_b, dx) = LS.out((n,)), LS.out((1,)), LS.out((n, D))
        LS._twice("cos", "forward", (row_b, sum_b), lambda: LS._rc(L.dl_cos_rowloss_fwd(self.x.data_ptr(), self.y.data_ptr(), row_b.ptr(), sum_b.ptr(),
                                                                                          n, D, ops._stream()), "dl_cos_rowloss_fwd"))
        LS._twice("cos", "backward", (dx_b,), lambda: LS._rc(L.dl_cos_rowloss_bwd(self.x.data_ptr(), self.y.data_ptr(), self.gscale, dx_b.ptr(), n, D,
                                                                                   ops._stream()), "dl_cos_rowloss_bwd"))
        return {"row_loss": row.clone(), "loss_sum": tot.clone(), "dx": dx.clone()}


COS_NF_CASES = [Case("cos/%dx%d" % (n, D), "loss", " | ".join(LS.COS_FORMS), functools.partial(CosSide, n, D),
                     [Plant("x", (n - 1, D - 1), NAN), Plant("y", (min(6, n - 1), min(3, D - 1)), NAN), Plant("x", (n // 2, 1), PINF)])
                for (n, D) in ((5, 260), (300, 128))]

CE_BY_NAME = {c.name: c for c in LS.CE_CASES}
CE_PICK = ["fast_c27_n1000_ign0", "fast_c32_n256_ign-100", "bf16_ld48_c40_n257", "f32_ld5_c5_n257_ign0", "f32_ld40_c27_cp32_ldd40_n1000_big"]


class CeSide(Side):
    """dl_ce_rows_fwd (lse per row, [mean, count]) and dl_ce_rows_bwd on the forward's own lse and count."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        xc, yc = LS.ce_data(c)
        self.lg = LS.Buf(c.N * c.ld + c.off, c.dt, dev=dev)
        self.x = self.lg.view((c.N, c.C), (c.ld, 1), c.off)
        self.x.copy_(xc)
        self.labels = yc.to(dev)
        self.operands = {"logits": [self.x]}
        self.gout = 0.625

    def ref(self):
        c = self.c
        r = LR.ce_rows(self.x, self.labels, c.C, c.ignore)
        rb = LR.ce_rows_bwd(self.x, self.labels, c.C, c.ignore, r["lse"], r["count"], self.gout, c.Cp)
        self._r, self._rb = r, rb
        return {"lse": r["lse"], "mean": torch.tensor([r["mean"]], dtype=F64, device=self.dev), "count": torch.tensor([float(r["count"])], dtype=F64, device=self.dev),
                "dlogits": rb["dlogits"]}

    def bound(self, what, refs):
        """The loss suite's bounds on the planted reference (a -inf logit is a masked class: the row's lse, the mean and the
        row's dlogits move), with the masked class's own terms p |x - m| = 0 x inf and |x - lse| = inf left out."""
        c, r, rb = self.c, self._r, self._rb
        z = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)
        x = self.x.double()
        m = x.amax(1, keepdim=True)
        e = torch.exp(x - m)
        ssum = e.sum(1, keepdim=True)
        mag_lse = z(m.abs().squeeze(1) + torch.log(ssum).abs().squeeze(1) + z(e / ssum * (x - m).abs()).sum(1))
        b_lse = MARGIN * U_F * (c.C + 6 + 4 * mag_lse)
        if what == "lse":
            return b_lse
        if what == "mean":
            nb = (c.N + 255) // 256
            return (MARGIN * ((b_lse / MARGIN + U_F * z(r["mag_loss"]))[r["valid"]].sum() + (20 + nb / 256) * U_F * z(r["row_loss"]).abs().sum())
                    / max(r["count"], 1)).reshape(1)
        if what == "dlogits":
            mag = z(rb["mag"])
            coh = MARGIN * U_F * (8 + 2 * z(rb["xl"])) * mag + mag * b_lse.unsqueeze(1)        # (the kernel reads its own fp32 lse)
            floor = (1.0 + abs(self.gout) / max(r["count"], 1)) * 2.0 ** -126
            return coh + MARGIN * (U_B if c.dt == BF else 0.0) * mag + floor
        return None

    def run(self):
        from druglamp_amd import _lib, ops
        c, L = self.c, _lib.lib()
        dtc = _lib.DL_BF16 if c.dt == BF else _lib.DL_F32
        N_, Cc = c.N, c.C
        y = LS.guard(self.labels, fill=Cc + 5)
        nws = L.dl_ce_rows_workspace_bytes(N_)
        (lse_b, lse), (o2_b, o2), (ws_b, _ws) = LS.out((N_,)), LS.out((2,)), LS.out((nws // 4,))
        LS._twice(c.name, "forward", (lse_b, o2_b, ws_b),
                  lambda: LS._rc(L.dl_ce_rows_fwd(self.lg.ptr(c.off), c.ld, y.data_ptr(), N_, Cc, c.ignore, dtc, lse_b.ptr(), o2_b.ptr(), ws_b.ptr(), nws,
                                                  ops._stream()), "dl_ce_rows_fwd"))
        gout = LS.guard(torch.tensor([self.gout], device=self.dev))
        dl = LS.Buf(N_ * c.ldd + c.off, c.dt)
        d = dl.view((N_, c.Cp), (c.ldd, 1), c.off)
        LS._twice(c.name, "backward", (dl,),
                  lambda: LS._rc(L.dl_ce_rows_bwd(self.lg.ptr(c.off), c.ld, y.data_ptr(), N_, Cc, c.ignore, dtc, lse_b.ptr(), o2_b.ptr(), gout.data_ptr(),
                                                  dl.ptr(c.off), c.ldd, c.Cp, ops._stream()), "dl_ce_rows_bwd"))
        return {"lse": lse.clone(), "mean": o2[:1].clone(), "count": o2[1:].clone(), "dlogits": d.clone()}


def _ce_case(name):
    c = CE_BY_NAME[name]
    _, y = LS.ce_data(c)
    counted = [int(i) for i in (y != c.ignore).nonzero().flatten()]
    ignored = [int(i) for i in (y == c.ignore).nonzero().flatten()]
    r0, r1 = counted[min(3, len(counted) - 1)], counted[-1]
    off = lambda r: (int(y[r]) + 1) % c.C                              # a class that is not the row's label
    ps = [Plant("logits", (r0, off(r0)), NAN), Plant("logits", (r1, c.C - 1), NAN), Plant("logits", (r0, off(r0)), NINF), Plant("logits", (r1, off(r1)), PINF)]
    if ignored:                                            # an ignored row FULL of NaN contributes nothing: the lse of that row only;
        ps.append(Plant("logits", (ignored[-1], slice(None)), NAN))        # the mean, the count and every other row bitwise unchanged
    return Case("ce/" + name, "loss", " | ".join(c.forms), functools.partial(CeSide, c), ps)


CE_NF_CASES = [_ce_case(n) for n in CE_PICK]


class TripletSide(Side):
    """dl_triplet_sigcos_fwd (distances, loss, triplet count) and dl_triplet_sigcos_bwd on the forward's scratch.  relu(NaN) is
    NaN: a NaN hinge poisons the loss, and its gradient is a closed ReLU's; a pair whose cosine is NaN poisons the gradients of
    its anchor and its drug even without a hinge coefficient (0 x NaN, as autograd's backward of the sigmoid gives)."""
    GOUT = 0.75

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        pc, dc, gtc = LS.tri_data(c)
        self.p, self.d, self.gt = _place(pc, F32, dev), _place(dc, F32, dev), gtc.to(dev)
        self.operands = {"p": [self.p], "d": [self.d]}

    def ref(self):
        r = LR.triplet(self.p, self.d, self.gt, self.c.margin)
        t = lambda v: torch.tensor([float(v)], dtype=F64, device=self.dev)
        return {"dist": r["dist"], "loss": t(r["loss"]), "n_tri": t(max(r["n_tri"], 1)), "dp": self.GOUT * r["dp"], "dd": self.GOUT * r["dd"]}

    def run(self):
        from druglamp_amd import _lib, ops
        c, L = self.c, _lib.lib()
        n_p, n_d, dim = c.n_p, c.n_d, c.dim
        gt = LS.guard(self.gt, fill=1)
        nf = L.dl_triplet_sigcos_buffer_floats(n_p, n_d)
        (buf_b, buf), (loss_b, loss), (nt_b, ntri) = LS.out((nf,)), LS.out((1,)), LS.out((1,))
        LS._twice(c.name, "forward", (buf_b, loss_b, nt_b),
                  lambda: LS._rc(L.dl_triplet_sigcos_fwd(self.p.data_ptr(), self.d.data_ptr(), gt.data_ptr(), n_p, n_d, dim, c.margin, buf_b.ptr(),
                                                         loss_b.ptr(), nt_b.ptr(), ops._stream()), "dl_triplet_sigcos_fwd"))
        dist = buf[:n_p * n_d].reshape(n_p, n_d).clone()
        (dp_b, dp), (dd_b, dd) = LS.out((n_p, dim)), LS.out((n_d, dim))
        LS._twice(c.name, "backward", (dp_b, dd_b),
                  lambda: LS._rc(L.dl_triplet_sigcos_bwd(self.p.data_ptr(), self.d.data_ptr(), gt.data_ptr(), buf_b.ptr(), n_p, n_d, dim, c.margin,
                                                         nt_b.ptr(), self.GOUT, dp_b.ptr(), dd_b.ptr(), ops._stream()), "dl_triplet_sigcos_bwd"))
        buf_b.untouched(c.name, "scratch after the backward")
        return {"dist": dist, "loss": loss.clone(), "n_tri": ntri.clone(), "dp": dp.clone(), "dd": dd.clone()}


def _tri_case(name):
    c = {t.name: t for t in LS.TRI_CASES}[name]
    _, _, gt = LS.tri_data(c)
    i_reg = int(((gt == 1).any(1) & (gt == 0).any(1)).nonzero()[0])                    # an anchor with positives and negatives
    j_neg, j_pos = int((gt[i_reg] == 0).nonzero()[0]), int((gt[i_reg] == 1).nonzero()[-1])
    ps = [Plant("d", (j_neg, 3), NAN), Plant("d", (j_pos, c.dim - 1), NAN), Plant("p", (i_reg, 1), NAN), Plant("p", (0, c.dim - 1), NAN),
          Plant("d", (c.n_d - 1, 0), PINF)]
    return Case("triplet/" + name, "loss", " | ".join(LS.TRI_FORMS), functools.partial(TripletSide, c), ps)


TRI_NF_CASES = [_tri_case(n) for n in ("tri_7x33_dim256", "tri_5x64_dim70")]


class NtxSide(Side):
    """One launch of an NT-Xent case: dl_ntxent_fwd_ex (lse, row_loss, the mean through ntx_vec_sum) and one dl_ntxent_bwd_ex per
    weight mode, on the forward's own log-sum-exp (mode 2: the streamed side's, from the kernel run with the sides swapped).
    One-sided launches keep resident and streamed rows in separate buffers: a NaN in resident row i poisons row i alone, a NaN
    in streamed row j every resident row EXCEPT the one whose own column j is (the kernel overwrites the own column).  In the
    symmetric launch (mode 0) the same rows are both sides and every row sees every other: everything is poisoned."""

    def __init__(self, c, li, dev):
        self.c, self.dev, self.launch = c, dev, c.launches[li]
        a0, na, b0, nb, self.wmodes = self.launch
        qc, kc = LS.ntx_batch(c)
        self.sym = (a0, na) == (b0, nb)
        self.everything_depends = self.sym
        self.nan_as_inf = ("a resident row whose EVERY logit is NaN keeps the running maximum at its initial -inf (fmaxf drops NaN), and "
                           "its lse / row_loss (and the mean over the rows) come out as an infinity; rows with some finite logit give NaN")
        self.aq, self.ak, bq, bk = (_place(x, c.dt, dev) for x in LS.ntx_sides(qc, kc, self.launch))
        self.bq, self.bk = (self.aq, self.ak) if self.sym else (bq, bk)
        self.operands = {"aq": [self.aq], "ak": [self.ak]}
        if not self.sym:
            self.operands.update(bq=[self.bq], bk=[self.bk])

    def ref(self):
        c = self.c
        a0, na, b0, nb, _ = self.launch
        r = LR.ntx_fwd(self.aq, self.ak, self.bq, self.bk, a0, b0, c.ng, c.T)
        out = {"lse": r["lse"], "row_loss": r["row_loss"], "loss": r["row_loss"].mean().reshape(1)}
        for wm in self.wmodes:
            la = r["lse"] if wm in (0, 1) else None
            lb = r["lse"] if wm == 0 else (LR.ntx_fwd(self.bq, self.bk, self.aq, self.ak, b0, a0, c.ng, c.T)["lse"] if wm == 2 else None)
            rb = LR.ntx_bwd(self.aq, self.ak, self.bq, self.bk, a0, b0, c.ng, c.T, la, lb, 1.0 / (2 * nb if wm == 2 else 2 * na))
            out["dA[wmode %d]" % wm] = torch.cat((rb["dq"], rb["dk"]))
        return out

    def run(self):
        from druglamp_amd import _lib, ops
        c, L = self.c, _lib.lib()
        a0, na, b0, nb, _ = self.launch
        aq, ak, bq, bk = self.aq, self.ak, self.bq, self.bk
        (lse_b_, lse), (rl_b_, rl), (ls_b_, ls) = LS.out((2 * na,)), LS.out((2 * na,)), LS.out((1,))
        fa = ops._ntx_args(aq, ak, bq, bk, a0, b0, c.ng, c.T)
        LS._twice(c.name, "forward", (lse_b_, rl_b_, ls_b_),
                  lambda: LS._rc(L.dl_ntxent_fwd_ex(fa, lse_b_.ptr(), rl_b_.ptr(), ls_b_.ptr(), ops._stream()), "dl_ntxent_fwd_ex"))
        out = {"lse": lse.clone(), "row_loss": rl.clone(), "loss": ls.clone()}
        for wm in self.wmodes:
            la = lse if wm in (0, 1) else None
            lb = lse if wm == 0 else (LS.guard(ops.ntxent_fwd_ex(bq, bk, aq, ak, b0, a0, c.ng, c.T)[1]) if wm == 2 else None)
            ba = ops._ntx_args(aq, ak, bq, bk, a0, b0, c.ng, c.T, la, lb)
            (dq_b, dq), (dk_b, dk) = LS.out((na, c.d)), LS.out((na, c.d))
            gscale = 1.0 / (2 * nb if wm == 2 else 2 * na)
            LS._twice(c.name, "backward wmode %d" % wm, (dq_b, dk_b),
                      lambda: LS._rc(L.dl_ntxent_bwd_ex(ba, gscale, dq_b.ptr(), dk_b.ptr(), ops._stream()), "dl_ntxent_bwd_ex"))
            out["dA[wmode %d]" % wm] = torch.cat((dq, dk))
        return out


def _ntx_cases():
    cs = []
    for c in LS.NTX_CASES:
        if not (c.name.startswith("sym_n37_") or c.name.startswith("ring_330_") and "big" not in c.name):
            continue
        for li, (a0, na, b0, nb, wm) in enumerate(c.launches):
            ps = [Plant("aq", (min(5, na - 1), 3), NAN), Plant("ak", (na - 1, c.d - 1), NAN)]
            if (a0, na) != (b0, nb):
                own = a0 - b0 + 7 if b0 <= a0 + 7 < b0 + nb else None               # the streamed row that is resident row 7's own column
                ps += [Plant("bq", (own if own is not None else 3, 1), NAN), Plant("bk", (a0 - b0 + na - 1 if b0 <= a0 + na - 1 < b0 + nb else nb - 1, c.d - 1), NAN)]      # (own column of the last resident row)
            cs.append(Case("ntxent/%s/launch%d" % (c.name, li), "loss", "%s | %s wmode %s | ntx_vec_sum" % (c.forms[0], c.forms[1], ",".join(map(str, wm))),
                           functools.partial(NtxSide, c, li), ps))
    return cs


NTX_NF_CASES = _ntx_cases()


# ==== elementwise, graph ==========================================================================================================
def _by_name(cases):
    return {c.name: c for c in cases}


class GateFwdSide(Side):
    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        v, lg = E.gate_fwd_data(c)
        self.v, self.lg = E.placed(v.to(dev), dev=dev), E.placed(lg.to(dev), dev=dev)
        self.operands = {"v": [self.v], "logits": [self.lg]}

    def ref(self):
        rg, d, rout, m = er.token_gate_fwd(self.v, self.lg, self.c.H, float(self.c.res))
        self._rg, self._d = rg, d
        return {"gate": rg, "out": rout}

    def bound(self, what, refs):
        if what != "gate":
            return None
        d = torch.nan_to_num(self._d, nan=0.0, posinf=0.0)            # the masked token's own exponent: its gate is an exact zero
        return torch.nan_to_num(E.gate_bound(torch.nan_to_num(self._rg, nan=0.0), d, self.c.L) * self._rg, nan=0.0)

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        D = c.H * c.hd
        out, gate = E.Out((c.B, c.L, D), c.dt), E.Out((c.B, c.H, c.L), F32)
        ok(L.dl_token_gate_fwd(self.v.data_ptr(), self.lg.data_ptr(), out.v.data_ptr(), gate.v.data_ptr(), c.B, c.L, D, c.H, c.res, DT[c.dt], stream),
           "dl_token_gate_fwd")
        torch.cuda.synchronize()
        out.done(c.name), gate.done(c.name)
        return {"gate": gate.v.clone(), "out": out.v.clone()}


class GateBwdSide(Side):
    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.dout, self.v, self.gate = (E.placed(t.to(dev), dev=dev) for t in E.gate_bwd_data(c))
        self.operands = {"dout": [self.dout], "v": [self.v]}

    def ref(self):
        rdv, rdl, _ = er.token_gate_bwd(self.dout, self.v, self.gate, self.c.H, float(self.c.res))
        return {"dv": rdv, "dlogits": rdl}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        D = c.H * c.hd
        dv, dl = E.Out((c.B, c.L, D), c.dt), E.Out((c.B, c.L, c.H), c.dt)
        ok(L.dl_token_gate_bwd(self.dout.data_ptr(), self.v.data_ptr(), self.gate.data_ptr(), dv.v.data_ptr(), dl.v.data_ptr(), c.B, c.L, D, c.H, c.res,
                               DT[c.dt], stream), "dl_token_gate_bwd")
        torch.cuda.synchronize()
        dv.done(c.name), dl.done(c.name)
        return {"dv": dv.v.clone(), "dlogits": dl.v.clone()}


class GeluBwdSide(Side):
    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.dy, self.pre = (E.placed(t.to(dev), dev=dev) for t in E.gelu_data(c))
        self.operands = {"dy": [self.dy]}

    def ref(self):
        return {"dx": er.gelu_bwd(self.dy, self.pre)[0]}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        dx = E.Out((c.n,), c.dt)
        ok(L.dl_gelu_bwd(self.dy.data_ptr(), self.pre.data_ptr(), dx.v.data_ptr(), c.n, DT[c.dt], stream), "dl_gelu_bwd")
        torch.cuda.synchronize()
        return {"dx": dx.done(c.name).v.clone()}


class AdamSide(Side):
    HYPER = E.ADAM_HYPER[1]                                # step 1000, grad_scale 1 / 128, weight decay 1e-2

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.p0, g, self.m0, self.v0 = (t.to(dev) for t in E.adamw_data(c, self.HYPER))
        self.g = E.placed(g, dev=dev)
        self.operands = {"grad": [self.g]}

    def ref(self):
        step, gscale, wd = self.HYPER
        rp, rm, rv, _ = er.adamw(self.p0, self.g, self.m0, self.v0, E.ADAM_LR, E.ADAM_B1, E.ADAM_B2, E.ADAM_EPS, wd, step, gscale)
        out = {"param": rp, "exp_avg": rm, "exp_avg_sq": rv}
        if self.c.lowp is not None:
            out["lowp"] = rp.clone()                       # the low-precision image carries the same value (classification only)
        return out

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        step, gscale, wd = self.HYPER
        outs = [E.Out((c.n,), F32) for _ in range(3)] + ([E.Out((c.n,), c.lowp)] if c.lowp is not None else [])
        for o, src in zip(outs, (self.p0, self.m0, self.v0)):
            o.v.copy_(src)
            o.before = o.g.bits()
        ok(L.dl_adamw_step(outs[0].v.data_ptr(), self.g.data_ptr(), outs[1].v.data_ptr(), outs[2].v.data_ptr(), c.n, E.ADAM_LR, E.ADAM_B1, E.ADAM_B2,
                           E.ADAM_EPS, wd, step, gscale, outs[3].v.data_ptr() if c.lowp is not None else None,
                           DT[c.lowp] if c.lowp is not None else 0, stream), "dl_adamw_step")
        torch.cuda.synchronize()
        for o in outs:
            o.done(c.name)
        out = {"param": outs[0].v.clone(), "exp_avg": outs[1].v.clone(), "exp_avg_sq": outs[2].v.clone()}
        if c.lowp is not None:
            out["lowp"] = outs[3].v.clone()
        return out


class CastSide(Side):
    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.src = E.placed(E.cast_data(c).to(dev), dev=dev)
        self.operands = {"src": [self.src]}

    def ref(self):
        return {"dst": er.cast(self.src, self.c.ddt).double()}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        dst = E.Out((c.n,), c.ddt)
        ok(L.dl_cast(self.src.data_ptr(), DT[c.sdt], dst.v.data_ptr(), DT[c.ddt], c.n, stream), "dl_cast")
        torch.cuda.synchronize()
        return {"dst": dst.done(c.name).v.clone()}


class NormAdjSide(Side):
    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.adj = E.placed(E.norm_adj_data(c).to(dev), dev=dev)
        self.operands = {"adj": [self.adj]}

    def ref(self):
        return {"ahat": er.norm_adjacency(self.adj)[0]}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        out = E.Out((2, c.n, c.n), c.dto)
        ok(L.dl_norm_adjacency(self.adj.data_ptr(), out.v.data_ptr(), 2, c.n, DT[c.dto], stream), "dl_norm_adjacency")
        torch.cuda.synchronize()
        return {"ahat": out.done(c.name).v.clone()}


class AggSide(Side):
    def __init__(self, c, dev):
        self.c, self.dev, self.N = c, dev, c.n + 3
        self.ahat, self.feat = (E.placed(t.to(dev), dev=dev) for t in E.agg_data(c, self.N))
        self.operands = {"ahat": [self.ahat], "feat": [self.feat]}

    def ref(self):
        return {"out[transpose=%d]" % tr: er.graph_aggregate(self.ahat, self.feat, self.c.n, tr)[0] for tr in (0, 1)}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c, res = self.c, {}
        for tr in (0, 1):
            out = E.Out((E.AGG_B, self.N, E.AGG_C), c.dt)
            ok(L.dl_graph_aggregate(self.ahat.data_ptr(), self.feat.data_ptr(), out.v.data_ptr(), E.AGG_B, c.n, self.N, E.AGG_C, tr, DT[c.dt], stream),
               "dl_graph_aggregate")
            torch.cuda.synchronize()
            res["out[transpose=%d]" % tr] = out.done(c.name).v.clone()
        return res


class DropSide(Side):
    """dl_add_rowmod_dropout (pe: the positional table, or none) and dl_dropout_apply: a dropped element is +0 whatever it held."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.apply = hasattr(c, "ldx")
        if self.apply:
            self.x = E.placed(E.dropa_data(c).to(dev), strides=(c.ldx, 1), n=c.M * c.ldx, dev=dev)
            self.pe, self.L = None, 1
        else:
            x, pe = E.drop_data(c)
            self.x, self.pe, self.L = E.placed(x.to(dev), dev=dev), (None if pe is None else E.placed(pe.to(dev), dev=dev)), c.L
        self.operands = {"x": [self.x]}
        if self.pe is not None:
            self.operands["pe"] = [self.pe]
        thr = er.dropout_thr16(c.p) if c.p > 0 else 0
        self.keep = torch.from_numpy(er.keep_mask(c.seed + c.off, c.M, c.D, thr)).to(dev) if thr else None

    def ref(self):
        s, _ = er.add_rowmod(self.x, self.pe, self.L)
        return {"y": er.dropout(s, self.keep, self.c.p)[0] if self.keep is not None else s}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        off = torch.tensor([c.off], dtype=torch.int64, device=self.dev) if c.off else None
        if self.apply:
            y = E.Out((c.M, c.D), c.dt, strides=(c.ldy, 1), n=c.M * c.ldy)
            ok(L.dl_dropout_apply(self.x.data_ptr(), y.v.data_ptr(), c.M, c.D, c.ldx, c.ldy, c.p, c.seed % 2 ** 64, N._ptr(off), DT[c.dt], stream),
               "dl_dropout_apply")
        else:
            y = E.Out((c.M, c.D), c.dt)
            ok(L.dl_add_rowmod_dropout(self.x.data_ptr(), N._ptr(self.pe), y.v.data_ptr(), c.M, c.D, c.L, c.p, c.seed % 2 ** 64, N._ptr(off), DT[c.dt],
                                       stream), "dl_add_rowmod_dropout")
        torch.cuda.synchronize()
        return {"y": y.done(c.name).v.clone()}


class DpreSide(Side):
    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.dl, self.w2, self.pre = (E.placed(t.to(dev), dev=dev) for t in E.dpre_data(c))
        self.operands = {"dl": [self.dl], "w2": [self.w2]}

    def ref(self):
        return {"dpre": er.gate_dpre(self.dl, self.w2, self.pre)[0]}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        out = E.Out((c.M, c.dd), c.dt)
        ok(L.dl_gate_dpre(self.dl.data_ptr(), self.w2.data_ptr(), self.pre.data_ptr(), out.v.data_ptr(), c.M, c.dd, 8, DT[c.dt], stream), "dl_gate_dpre")
        torch.cuda.synchronize()
        return {"dpre": out.done(c.name).v.clone()}


class FillPoolSide(Side):
    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.x = E.placed(E.fill_pool_data(c).to(dev), dev=dev)
        self.operands = {"x": [self.x]}

    def ref(self):
        fill, pooled, _, _, _ = er.fill_pool(self.x, self.c.site_len)
        return {"fill": fill, "pooled": pooled}

    def bound(self, what, refs):
        """A NaN in an all-zero row moves its fill bit from 1 to 0 (the row no longer sums to zero): an exact value."""
        return torch.zeros_like(refs["fill"]) if what == "fill" else None

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        S, Fp = c.n_site * c.site_len, (c.F + 1 + 7) // 8 * 8
        fill, pooled = E.Out((c.B, S), c.dti), E.Out((c.B, c.n_site, Fp), c.dto)
        ok(L.dl_fill_pool(self.x.data_ptr(), fill.v.data_ptr(), pooled.v.data_ptr(), c.B, S, c.F, c.site_len, DT[c.dti], DT[c.dto], stream), "dl_fill_pool")
        torch.cuda.synchronize()
        return {"fill": fill.done(c.name).v.clone(), "pooled": pooled.done(c.name).v.clone()}


class RowmodSumSide(Side):
    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        x, old = E.rowmod_sum_data(c)
        self.x, self.old = E.placed(x.to(dev), dev=dev), old.to(dev)
        self.operands = {"x": [self.x]}
        if c.acc:
            self.operands["old"] = [self.old]

    def ref(self):
        return {"out": er.rowmod_sum(self.x, self.c.L, self.old if self.c.acc else None)[0]}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        out = E.Out((c.L, c.D), F32)
        if c.acc:
            out.v.copy_(self.old)
            out.before = out.g.bits()
        ok(L.dl_rowmod_sum(self.x.data_ptr(), out.v.data_ptr(), c.nb * c.L, c.D, c.L, c.acc, DT[c.dt], stream), "dl_rowmod_sum")
        torch.cuda.synchronize()
        return {"out": out.done(c.name).v.clone()}


class GatherSide(Side):
    """dl_rows_gather: a mover, NaN and infinities are bit patterns like any other; a row with index < 0 is zero."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        g = torch.Generator().manual_seed(len(c.name) + c.R)
        self.w = c.row_bytes // 4
        self.src = E.placed(torch.randn(1000, self.w, generator=g).to(dev), dev=dev)
        index = torch.randint(-1, 1000, (c.R,), generator=g, dtype=torch.int32)
        index[:4] = torch.tensor([-1, 999, 5, 5], dtype=torch.int32)
        self.index = E.table(index.to(dev), dev=dev)
        self.operands = {"src": [self.src]}

    def ref(self):
        return {"out": er.rows_gather(self.src, self.index).double()}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        out = E.Out((c.R, self.w), F32)
        ok(L.dl_rows_gather(self.src.data_ptr(), self.index.data_ptr(), out.v.data_ptr(), c.R, c.row_bytes, stream), "dl_rows_gather")
        torch.cuda.synchronize()
        return {"out": out.done(c.name).v.clone()}


class GatherPadSide(Side):
    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        store, offs, lens = E.gather_data(c)
        self.store = E.placed(store.to(dev), dev=dev)
        self.offs, self.lens = E.table(offs.to(dev), -7, torch.int64, dev), E.table(lens.to(dev), dev=dev)
        self.operands = {"store": [self.store]}

    def ref(self):
        return {"out": er.gather_pad(self.store, self.offs.tolist(), self.lens.tolist(), self.c.S, self.c.repeat).double()}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c, B = self.c, len(self.c.lengths)
        out = E.Out((B, c.S, c.F), c.dt)
        ok(L.dl_gather_pad(self.store.data_ptr(), self.offs.data_ptr(), self.lens.data_ptr(), out.v.data_ptr(), B, c.S, c.F, c.repeat, DT[c.dt], stream),
           "dl_gather_pad")
        torch.cuda.synchronize()
        return {"out": out.done(c.name).v.clone()}


class EmbedSide(Side):
    """dl_embed_pad and dl_embed_rows: the embedding table and the fill bits are the floating-point operands."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        ids, weight, fill, src = E.embed_data(c)
        self.ids, self.src = E.table(ids.to(dev), c.V + 1000, torch.int64, dev), E.table(src.to(dev), dev=dev)
        self.weight, self.fill = E.placed(weight.to(dev), dev=dev), E.placed(fill.to(dev), dev=dev)
        self.operands = {"weight": [self.weight], "fill": [self.fill]}

    def ref(self):
        c = self.c
        return {"pad": er.embed_pad(self.ids, self.weight, self.fill, c.D, c.halo).double(),
                "rows": er.embed_rows(self.ids, self.weight, self.fill, self.src, c.D).double()}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c, R = self.c, self.src.numel()
        pad, rows = E.Out((c.B, c.L + 2 * c.halo, c.D + 1), c.dt), E.Out((R, c.D + 1), c.dt)
        ok(L.dl_embed_pad(self.ids.data_ptr(), self.weight.data_ptr(), self.fill.data_ptr(), pad.v.data_ptr(), c.B, c.L, c.V, c.D, c.halo, DT[c.dt],
                          stream), "dl_embed_pad")
        ok(L.dl_embed_rows(self.ids.data_ptr(), self.weight.data_ptr(), self.fill.data_ptr(), self.src.data_ptr(), rows.v.data_ptr(), R, c.V, c.D,
                           None, 0, 0, None, DT[c.dt], stream), "dl_embed_rows")
        torch.cuda.synchronize()
        return {"pad": pad.done(c.name).v.clone(), "rows": rows.done(c.name).v.clone()}


class RowsSumSide(Side):
    """dl_rows_sum_strided: fp32 sums of `count` rows behind a (first, stride, count) table; a row of count 0 is zero."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        x, rep = E.rows_sum_data(c)
        self.x, self.rep = E.placed(x.to(dev), off=c.off, dev=dev), E.table(rep.to(dev), dev=dev)
        self.operands = {"x": [self.x]}

    def form(self):
        out = E.Out((self.c.R, self.c.C), self.c.dt, off=self.c.off, dev=self.dev)
        return E.rows_sum_form(self.c, self.x.data_ptr(), out.v.data_ptr())

    def ref(self):
        return {"out": er.rows_sum_strided(self.x, self.rep)[0]}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        out = E.Out((c.R, c.C), c.dt, off=c.off)
        assert E.rows_sum_form(c, self.x.data_ptr(), out.v.data_ptr()) == c.form, "%s: the case names the other form" % c.name
        ok(L.dl_rows_sum_strided(self.x.data_ptr(), self.rep.data_ptr(), out.v.data_ptr(), c.R, c.C, DT[c.dt], stream), "dl_rows_sum_strided")
        torch.cuda.synchronize()
        return {"out": out.done(c.name).v.clone()}


class SitePoolSide(Side):
    """dl_cnn_sitepool_fwd on z (the halo rows hold NaN and are never read) and dl_cnn_sitepool_bwd on dpooled."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        zb, dp = E.sitepool_data(c)
        self.L = c.n_site * c.site_len
        z = torch.full((c.B, self.L + 2 * c.halo, c.C), float("nan"), dtype=BF)
        z[:, c.halo:c.halo + self.L] = zb
        self.z, self.dp = E.placed(z.to(dev), dev=dev), E.placed(dp.to(dev), dev=dev)
        self.operands = {"z": [self.z], "dpooled": [self.dp]}

    def ref(self):
        c = self.c
        body = er.sitepool_bwd(self.dp, self.L, c.C, c.site_len)[0]
        dz = torch.zeros(c.B, self.L + 2 * c.halo, c.C, dtype=F64, device=self.dev)
        dz[:, c.halo:c.halo + self.L] = body
        return {"pooled": er.sitepool_fwd(self.z[:, c.halo:c.halo + self.L], c.site_len)[0].reshape(c.B, c.n_site * c.C), "dz": dz}

    def run(self):
        Lb, ok, stream, DT, _ = _lib()
        c = self.c
        pooled, dz = E.Out((c.B, c.n_site * c.C), BF), E.Out((c.B, self.L + 2 * c.halo, c.C), BF)
        ok(Lb.dl_cnn_sitepool_fwd(self.z.data_ptr(), pooled.v.data_ptr(), c.B, self.L, c.C, c.halo, c.site_len, DT[BF], stream), "dl_cnn_sitepool_fwd")
        ok(Lb.dl_cnn_sitepool_bwd(self.dp.data_ptr(), dz.v.data_ptr(), c.B, self.L, c.C, c.halo, c.site_len, DT[BF], stream), "dl_cnn_sitepool_bwd")
        torch.cuda.synchronize()
        return {"pooled": pooled.done(c.name).v.clone(), "dz": dz.done(c.name).v.clone()}


class RowsPoolSide(Side):
    """dl_cnn_sitepool_rows_fwd / _bwd through the row tables of the compact layout (rows no position maps to hold NaN)."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.plan = plan = E.rowspool_plan(c)
        z, dp = E.rowspool_data(c, plan)
        self.z, self.dp = E.placed(z.to(dev), dev=dev), E.placed(dp.to(dev), dev=dev)
        self.row_of, self.rep = E.table(torch.from_numpy(plan.row_of).to(dev), dev=dev), E.table(torch.from_numpy(plan.rep).to(dev), dev=dev)
        self.operands = {"z": [self.z], "dpooled": [self.dp]}

    def ref(self):
        c, B = self.c, len(self.c.lengths)
        body = self.z[self.row_of.long()].reshape(B, c.L, c.C)
        dbody = er.sitepool_bwd(self.dp, c.L, c.C, c.site_len)[0]
        return {"pooled": er.sitepool_fwd(body, c.site_len)[0].reshape(B, -1), "dz": er.rows_sum_strided(dbody.reshape(B * c.L, c.C), self.rep)[0]}

    def run(self):
        Lb, ok, stream, DT, _ = _lib()
        c, B, R = self.c, len(self.c.lengths), self.plan.rows
        pooled, dz = E.Out((B, (c.L // c.site_len) * c.C), BF), E.Out((R, c.C), BF)
        ok(Lb.dl_cnn_sitepool_rows_fwd(self.z.data_ptr(), self.row_of.data_ptr(), pooled.v.data_ptr(), B, c.L, c.C, c.site_len, DT[BF], stream),
           "dl_cnn_sitepool_rows_fwd")
        ok(Lb.dl_cnn_sitepool_rows_bwd(self.dp.data_ptr(), self.rep.data_ptr(), self.row_of.data_ptr(), dz.v.data_ptr(), B, c.L, c.C, R, c.site_len,
                                       DT[BF], stream), "dl_cnn_sitepool_rows_bwd")
        torch.cuda.synchronize()
        return {"pooled": pooled.done(c.name).v.clone(), "dz": dz.done(c.name).v.clone()}


class MoverSide(Side):
    """dl_interleave_streams and dl_concat2 (forward direction): bit movers."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        g = torch.Generator().manual_seed(len(c.name) + c.R)
        self.w = w = c.row_bytes // 4
        if c.op == "interleave":
            self.a, self.b = E.placed(torch.randn(c.S, c.R, w, generator=g).to(dev), dev=dev), None
            self.operands = {"a": [self.a]}
        else:
            self.a, self.b = E.placed(torch.randn(c.R, w, generator=g).to(dev), dev=dev), E.placed(torch.randn(c.R, w + 12, generator=g).to(dev), dev=dev)
            self.operands = {"a": [self.a], "b": [self.b]}

    def ref(self):
        return {"out": (er.interleave_streams(self.a) if self.c.op == "interleave" else er.concat2(self.a, self.b)).double()}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c, w = self.c, self.w
        if c.op == "interleave":
            out = E.Out((c.R, c.S * w), F32)
            ok(L.dl_interleave_streams(self.a.data_ptr(), out.v.data_ptr(), c.R, c.row_bytes, c.S, 0, stream), "dl_interleave_streams")
        else:
            out = E.Out((c.R, 2 * w + 12), F32)
            ok(L.dl_concat2(self.a.data_ptr(), self.b.data_ptr(), out.v.data_ptr(), c.R, c.row_bytes, (w + 12) * 4, 0, stream), "dl_concat2")
        torch.cuda.synchronize()
        return {"out": out.done(c.name).v.clone()}


class WprepSide(Side):
    """dl_weight_prep: the parameter tensors written into the weight images (plain, transposed, strided items; cast to the image
    dtype).  Outputs: per image, the elements some item addresses."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.src = [E.placed(t.to(dev), dev=dev) for t in E.wprep_sources()]
        self.operands = {"A": [self.src[0]], "D": [self.src[4]], "E": [self.src[6]]}

    def ref(self):
        r = E.wprep_reference(self.c.dt, self.src, self.dev)
        self._mask = {k: v[1] for k, v in r.items()}
        return {"image " + k: v[0][v[1]].double() for k, v in r.items()}

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c = self.c
        imgs = {k: N.Guarded(n, c.dt, self.dev) for k, n in E.WPREP_SIZE.items()}
        before = {k: g.bits() for k, g in imgs.items()}
        items, bmap = b"", []
        for i, ((name, r, cl, ld, row0, mode, cs_), t) in enumerate(zip(E.WPREP_ITEMS, self.src)):
            base = imgs[name].t.data_ptr() + N.Guarded.G * imgs[name].t.element_size()
            items += struct.pack("<QQqiiiiq", t.data_ptr(), base, ld, r, cl, row0, mode, cs_)
            bmap += [(i, b) for b in range(((r + 63) // 64) * ((cl + 63) // 64))]
        items_dev = torch.frombuffer(bytearray(items), dtype=torch.uint8).to(self.dev)
        bmap_dev = E.table(torch.tensor(bmap[::-1], dtype=torch.int32).reshape(-1).to(self.dev), dev=self.dev)
        ok(L.dl_weight_prep(items_dev.data_ptr(), bmap_dev.data_ptr(), len(bmap), DT[c.dt], stream), "dl_weight_prep")
        torch.cuda.synchronize()
        self.ref()
        out = {}
        for k, g in imgs.items():
            g.mask[N.Guarded.G:N.Guarded.G + E.WPREP_SIZE[k]] = self._mask[k]
            g.untouched(c.name + " image " + k, before[k])
            out["image " + k] = g.t[N.Guarded.G:N.Guarded.G + E.WPREP_SIZE[k]][self._mask[k]].clone()
        return out


def _table_cases():
    cs = []
    for c in E.WPREP:
        cs.append(Case("elem/" + c.name, "elem", c.form, functools.partial(WprepSide, c), [
            Plant("A", (5, 7), NAN), Plant("A", (62, 129), NAN), Plant("D", (129, 64), NAN), Plant("E", (63, 62), NAN), Plant("A", (0, 0), PINF)]))
    for name in ("gatherpad_bf16_S12_F8_rep0", "gatherpad_f32_S12_F4_rep1"):
        c = _by_name(E.GATHER)[name]
        store, offs, lens = E.gather_data(c)
        used = [(int(o), min(int(n), c.S)) for o, n in zip(offs, lens) if 0 < int(n) <= (c.S if c.repeat else 10 ** 9)]
        first, last = used[0], used[-1]
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(GatherPadSide, c), [
            Plant("store", (first[0], 1), NAN), Plant("store", (last[0] + last[1] - 1, c.F - 1), NAN), Plant("store", (first[0], 0), PINF)]))
    for name in ("embed_f32_B3_L9_V26_D7_halo4", "embed_bf16_B2_L33_V26_D127_halo4"):
        c = _by_name(E.EMBED)[name]
        ids = E.embed_data(c)[0]
        v = int(ids[1, 2])                                  # an id that is in range
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(EmbedSide, c), [
            Plant("weight", (v, 1), NAN), Plant("weight", (v, c.D - 1), NAN), Plant("fill", (c.B - 1, c.L - 1), NAN), Plant("fill", (0, 5), PINF)]))
    for name in ("rowssum_bf16_C128_R23_off0", "rowssum_bf16_C512_R23_off0", "rowssum_bf16_C192_R23_off0", "rowssum_f32_C4_R70_off0"):
        c = _by_name(E.ROWS_SUM)[name]
        rep = E.rows_sum_data(c)[1]
        r1, r5 = rep[1], rep[5]                             # rows of count 1 and of count 200
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(RowsSumSide, c), [
            Plant("x", (int(r1[0]), 1), NAN), Plant("x", (int(r5[0]) + 199 * int(r5[1]), c.C - 1), NAN), Plant("x", (int(r5[0]), 0), PINF)]))
    for name in ("sitepool_ns31_sl5_C64_halo4", "sitepool_ns64_sl1_C64_halo0"):
        c = _by_name(E.SITEPOOL)[name]
        L_ = c.n_site * c.site_len
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(SitePoolSide, c), [
            Plant("z", (0, c.halo + 3, 5), NAN), Plant("z", (c.B - 1, c.halo + L_ - 1, c.C - 1), NAN), Plant("dpooled", (0, 7), NAN),
            Plant("dpooled", (c.B - 1, c.n_site * c.C - 1), NAN)]))
    for name in ("rowspool_B3_L192_sl3_C64", "rowspool_B3_L768_sl3_C128"):
        c = _by_name(E.ROWSPOOL)[name]
        row_of = E.rowspool_plan(c).row_of
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(RowsPoolSide, c), [
            Plant("z", (int(row_of[3]), 5), NAN), Plant("z", (int(row_of[-1]), c.C - 1), NAN), Plant("dpooled", (0, 7), NAN),
            Plant("dpooled", (len(c.lengths) - 1, (c.L // c.site_len) * c.C - 1), NAN)]))
    for name in ("interleave_R37_row16_S2", "concat2_R37_row16"):
        c = _by_name(E.MOVERS)[name]
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(MoverSide, c), [
            Plant("a", (0, 5, 1) if c.op == "interleave" else (5, 1), NAN), Plant("a", (1, c.R - 1, 3) if c.op == "interleave" else (c.R - 1, 3), PINF)]))
    return cs


def _kept(c):
    """(first kept, last kept, a pair: the last kept AND the last dropped element together) of the case's dropout mask.  A
    dropped element is +0 whatever it held, so the pair plant poisons the kept element alone and the dropped one must stay the
    bit pattern of +0: a dropout written as a product with a 0 / 1 mask would turn it into NaN.  Without dropout: the second
    and the last element, no pair."""
    thr = er.dropout_thr16(c.p) if c.p > 0 else 0
    if not thr:
        return (0, 1), (c.M - 1, c.D - 1), None
    keep = torch.from_numpy(er.keep_mask(c.seed + c.off, c.M, c.D, thr))
    k, d = keep.nonzero(), (~keep).nonzero()
    last = (int(k[-1][0]), int(k[-1][1]))
    return (int(k[0][0]), int(k[0][1])), last, ([last[0], int(d[-1][0])], [last[1], int(d[-1][1])])


def _elem_cases():
    cs = []
    for table_, names in ((E.ROWMOD, ("rowmod_f32_M50_D32_L16_pe1_p0.1_off0", "rowmod_bf16_M300_D8_L7_pe1_p0.5_off3", "rowmod_bf16_M50_D32_L16_pe0_p0_off0")),
                          (E.DROP_APPLY, ("dropapply_f32_M40_D32_ldx40_ldy36_p0.5_off0", "dropapply_bf16_M300_D8_ldx12_ldy8_p0.5_off7"))):
        for name in names:
            c = _by_name(table_)[name]
            first, last, pair = _kept(c)
            ps = [Plant("x", first, NAN), Plant("x", last, NAN), Plant("x", last, PINF)] + ([Plant("x", pair, NAN)] if pair else [])
            if getattr(c, "pe", 0):
                ps.append(Plant("pe", (c.L - 1, c.D - 1), NAN))
            cs.append(Case("elem/" + name, "elem", c.form, functools.partial(DropSide, c), ps))
    for name in ("dpre_f32_M81_dd200", "dpre_bf16_M257_dd64"):
        c = _by_name(E.DPRE)[name]
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(DpreSide, c), [
            Plant("dl", (3, 5), NAN), Plant("dl", (c.M - 1, 7), NAN), Plant("w2", (7, c.dd - 1), NAN)]))
    for name in ("fillpool_f32_bf16_B3_ns3_sl3_F520", "fillpool_bf16_f32_B3_ns5_sl1_F8"):
        c = _by_name(E.FILL_POOL)[name]
        S = c.n_site * c.site_len
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(FillPoolSide, c), [
            Plant("x", (1, 1, 3), NAN), Plant("x", (c.B - 1, S - 1, c.F - 1), NAN), Plant("x", (0, 0, 0), NAN)]))
    for name in [n for n in _by_name(E.ROWMOD_SUM) if n.startswith(("rowmodsum_f32_nb5_", "rowmodsum_bf16_nb17_"))]:
        c = _by_name(E.ROWMOD_SUM)[name]
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(RowmodSumSide, c), [
            Plant("x", (1, 2), NAN), Plant("x", (c.nb * c.L - 1, c.D - 1), NAN)] + ([Plant("old", (c.L - 1, 0), NAN)] if c.acc else [])))
    c = _by_name(E.MOVERS)["rowsgather_R37_row16"]
    cs.append(Case("elem/" + c.name, "elem", c.form, functools.partial(GatherSide, c), [
        Plant("src", (5, 1), NAN), Plant("src", (999, 3), NAN), Plant("src", (5, 0), PINF)]))
    gf, gb, ge, ad, ca, na, ag = map(_by_name, (E.GATE_FWD, E.GATE_BWD, E.GELU, E.ADAMW, E.CAST, E.NORM_ADJ, E.AGG))
    for name in ("gatef_f32_L65_H8_hd4_res0", "gatef_bf16_L65_H8_hd4_res0"):
        c = gf[name]
        D = c.H * c.hd
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(GateFwdSide, c), [
            Plant("logits", (1, 5, 2), NAN), Plant("logits", (c.B - 1, c.L - 1, c.H - 1), NAN), Plant("v", (0, c.L - 1, D - 1), NAN),
            Plant("logits", (1, 64, 3), NINF), Plant("logits", (0, 7, 1), PINF)]))
    for name in ("gateb_f32_L65_H3_hd4_res1", "gateb_bf16_L70_H3_hd12_res1"):
        c = gb[name]
        D = c.H * c.hd
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(GateBwdSide, c), [
            Plant("dout", (0, 3, 5), NAN), Plant("dout", (c.B - 1, c.L - 1, D - 1), NAN), Plant("v", (1, c.L - 1, 0), NAN)]))
    for name in ("gelubwd_f32_n1028", "gelubwd_bf16_n1028"):
        c = ge[name]
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(GeluBwdSide, c), [Plant("dy", (600,), NAN), Plant("dy", (c.n - 1,), NAN)]))
    for name in ("adamw_lowpnone_n1003", "adamw_lowpbf16_n1003", "adamw_lowpf32_n1028"):
        c = ad[name]
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(AdamSide, c), [
            Plant("grad", (600,), NAN), Plant("grad", (c.n - 1,), NAN), Plant("grad", (5,), PINF), Plant("grad", (c.n - 2,), NINF)]))
    for name in ("cast_f32_bf16_n1027", "cast_bf16_f32_n1027", "cast_f32_f32_n5"):
        c = ca[name]
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(CastSide, c), [
            Plant("src", (c.n // 2,), NAN), Plant("src", (c.n - 1,), NAN), Plant("src", (c.n - 2,), PINF), Plant("src", (c.n - 1,), NINF)]))
    for name in ("normadj_f32_n5", "normadj_bf16_n5", "normadj_f32_n195", "normadj_bf16_n195"):
        c = na[name]
        n = c.n
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(NormAdjSide, c), [
            Plant("adj", (0, 1, 3), NAN), Plant("adj", (1, n - 1, n - 1), NAN), Plant("adj", (0, n // 2, n // 2), NAN)]))
    for name in ("aggregate_f32_n5", "aggregate_bf16_n17", "aggregate_f32_n129", "aggregate_bf16_n160"):
        c = ag[name]
        n = c.n
        cs.append(Case("elem/" + name, "elem", c.form, functools.partial(AggSide, c), [
            Plant("ahat", (1, 2, 3), NAN), Plant("ahat", (E.AGG_B - 1, n - 1, n - 1), NAN), Plant("feat", (0, n - 1, E.AGG_C - 1), NAN),
            Plant("feat", (1, n + 1, 7), NAN)]))
    return cs


ELEM_NF_CASES = _elem_cases() + _table_cases()


# ==== attention forward and backward ==============================================================================================
ATTN_BY_NAME = {c.name: c for c in A.CASES}
ATTN_PICK = ["res_paired_p3_shift1_onepass_falls_back", "onepass_single_forced", "small_q_tail_mid_tile", "long_keys_1025_tail1",
             "generic_raw_tail_w1", "hd128_paired_half", "hd128_tail_pgca", "f32_hd64_paired_p3", "f32_hd128_raw"]


class _Store(A.Store):
    """tests/test_attention_paths_gpu.Store on a chosen device."""

    def __init__(self, n, dt, dev):
        self.t = torch.full((n + 2 * self.G,), float("nan"), device=dev, dtype=dt)
        self.mask = torch.zeros(n + 2 * self.G, dtype=torch.bool, device=dev)
        self.base = self.t[self.G:]


class AttnSide(Side):
    """dl_attn_fwd, then dl_attn_bwd on the forward's own O and LSE (the chain the model runs), in the buffers and layouts of
    the attention suite.  The reference's backward takes the reference's own O."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        dt, P, H, S, Lq, Lk, hd = c.dt, c.P, c.H, c.S, c.Lq, c.Lk, c.hd
        self.scale = hd ** -0.5
        g = torch.Generator().manual_seed(sum(map(ord, c.name)))
        self.layout, sizes, self.o_ss = A._layout(c.layout, P, H, S, Lq, Lk, hd)
        self.stores = {name: _Store(n, dt, dev) for name, n in sizes.items()}
        q, k, v = A._data(c, g, self.scale)
        self.region("q").copy_(q)
        self.region("k").copy_(k)
        self.region("v").copy_(v)
        for s in range(S):
            self.region("do", s).copy_(torch.randn(P, H, Lq, hd, generator=g) * 0.5)
            self.region("o", s)
        for op in ("dq", "dk", "dv"):
            self.region(op)
        (qb, qs), (kb, ks), (vb, vs) = (self.base(x) for x in ("q", "k", "v"))
        self.common = dict(n_problems=P, n_heads=H, n_segments=S, partner_shift=c.shift, Lq=Lq, Lk=Lk, head_dim=hd, scale=self.scale,
                           q_strides=qs, k_strides=ks, v_strides=vs, key_tail=c.tail)
        self.operands = {"q": [self.region("q")], "k": [self.region("k")], "v": [self.region("v")], "do": [self.region("do", 0)]}

    def region(self, op, seg=0):
        c = self.c
        sname, st, off = self.layout[op]
        return self.stores[sname].region(st, c.P, c.H, c.Lq if op in ("q", "o", "do", "dq") else c.Lk, c.hd,
                                         off + seg * (self.o_ss if op in ("o", "do") else 0))

    def base(self, op):
        sname, st, off = self.layout[op]
        return self.stores[sname].base[off:], st

    def ref(self):
        (qb, _), (kb, _), (vb, _), (dob, dos) = (self.base(x) for x in ("q", "k", "v", "do"))
        r = A.reference_fwd(qb, kb, vb, **self.common)
        b = A.reference_bwd(r, dob, do_strides=dos, do_ss=self.o_ss, scale=self.scale)
        out = {"O": r["O"], "LSE": r["LSE"], "dQ": b["dQ"], "dK": b["dK"], "dV": b["dV"]}
        if self.c.raw:
            out["raw"] = r["raw"]
        return out

    def run(self):
        from druglamp_amd import ops
        c = self.c
        P, H, S, Lq, Lk = c.P, c.H, c.S, c.Lq, c.Lk
        (qb, _), (kb, _), (vb, _), (ob, os_), (dob, dos) = (self.base(x) for x in ("q", "k", "v", "o", "do"))
        outs = sorted({self.layout[op][0] for op in ("o", "dq", "dk", "dv")} - {self.layout[op][0] for op in ("q", "k", "v", "do")})
        for name in outs:
            self.stores[name].t.fill_(float("nan"))
        before = {name: self.stores[name].bits() for name in outs}
        raw = _Store(P * H * Lq * Lk, F32, self.dev) if c.raw else None
        raw_t = raw.region((H * Lq * Lk, Lq * Lk, Lk), P, H, Lq, Lk) if c.raw else None
        lse = ops.attn_fwd(qb, kb, vb, out=ob, o_strides=os_, o_ss=self.o_ss, raw_logits=raw.base if c.raw else None, algo=c.fwd, **self.common)
        (dqb, dqs), (dkb, dks), (dvb, dvs) = (self.base(x) for x in ("dq", "dk", "dv"))
        ops.attn_bwd(qb, kb, vb, ob, dob, lse, o_strides=os_, o_ss=self.o_ss, do_strides=dos, do_ss=self.o_ss, dq=dqb, dq_strides=dqs,
                     dk=dkb, dk_strides=dks, dv=dvb, dv_strides=dvs, algo=c.bwd, **self.common)
        torch.cuda.synchronize()
        for name, b in before.items():
            A._untouched(c.name, self.stores[name], b)
        out = {"O": torch.stack([self.region("o", s) for s in range(S)]), "LSE": lse.clone(), "dQ": self.region("dq").clone(),
               "dK": self.region("dk").clone(), "dV": self.region("dv").clone()}
        if c.raw:
            A._untouched(c.name, raw, torch.full_like(raw.t, float("nan")).view(torch.int32))
            out["raw"] = raw_t.clone()
        return out


def _attn_case(name):
    c = ATTN_BY_NAME[name]
    P, H, Lq, Lk, hd = c.P, c.H, c.Lq, c.Lk, c.hd
    ps = [Plant("q", (0, 0, min(5, Lq - 1), 3), NAN), Plant("q", (P - 1, H - 1, Lq - 1, hd - 1), NAN),
          Plant("k", (0, H - 1, min(20, Lk - 2), 7), NAN), Plant("k", (P - 1, 0, Lk - 1, hd - 1), NAN),
          Plant("v", (P - 1, H - 1, min(9, Lk - 1), 5), NAN), Plant("v", (0, 0, Lk - 1, hd - 1), NAN),
          Plant("do", (0, 0, min(4, Lq - 1), 2), NAN), Plant("do", (P - 1, H - 1, Lq - 1, hd - 1), NAN)]
    if name in ("small_q_tail_mid_tile", "f32_hd64_paired_p3"):
        ps.append(Plant("v", (1, 0, Lk - 2, 1), PINF))
    return Case("attn/" + name, "attention", " + ".join(c.forms), functools.partial(AttnSide, c), ps)


ATTN_NF_CASES = [_attn_case(n) for n in ATTN_PICK]


class ProbsSide(AttnSide):
    """dl_attn_probs on the cases of tests/test_attention_probs_gpu.py: the probability map per head or as the head mean, with
    the tail keys expanded or not, once from the log-sum-exp of dl_attn_fwd on the same (planted) operands and once with
    lse=None.  A NaN in Q row i poisons row i of the map, one in K row j every row of that problem and head."""

    def ref(self):
        (qb, _), (kb, _), (vb, _) = (self.base(x) for x in ("q", "k", "v"))
        want = AP._expected(self.c, A.reference_fwd(qb, kb, vb, **self.common))[0]
        return {"map[lse of attn_fwd]": want, "map[lse=None]": want}

    def run(self):
        from druglamp_amd import ops
        c = self.c
        P, H, S, Lq, Lk = c.P, c.H, c.S, c.Lq, c.Lk
        (qb, _), (kb, _), (vb, vs), (ob, os_) = (self.base(x) for x in ("q", "k", "v", "o"))
        common = {k: v for k, v in self.common.items() if k != "v_strides"}
        lse_fwd = ops.attn_fwd(qb, kb, vb, out=ob, o_strides=os_, o_ss=self.o_ss, v_strides=vs, **common)
        t, w = (int(c.tail[0]), int(c.tail[1])) if (c.tail and c.expand) else (0, 1)
        cols = Lk - t + t * w
        out_ld = cols + 4 + (-cols) % 4 if c.vec else cols + (3 if (cols + 3) % 4 else 5)
        HO = 1 if c.mean else H
        out = _Store(S * P * HO * Lq * out_ld, F32, self.dev)
        view = out.region((HO * Lq * out_ld, Lq * out_ld, out_ld), S * P, HO, Lq, cols).view(S, P, HO, Lq, cols)
        blank = torch.full_like(out.t, float("nan")).view(torch.int32)
        res = {}
        for what, lse in (("map[lse of attn_fwd]", lse_fwd), ("map[lse=None]", None)):
            out.t.fill_(float("nan"))
            ops.attn_probs(qb, kb, lse=lse, head_mean=c.mean, expand_tail=c.expand, out=out.base, out_ld=out_ld, **common)
            torch.cuda.synchronize()
            assert torch.equal(out.bits()[~out.mask], blank[~out.mask]), "%s: a store outside the addressed columns" % c.name
            res[what] = view.clone()
        return res


def _probs_case(name):
    c = {t.name: t for t in AP.CASES}[name]
    P, H, Lq, Lk, hd = c.P, c.H, c.Lq, c.Lk, c.hd
    ps = [Plant("q", (0, 0, min(5, Lq - 1), 3), NAN), Plant("q", (P - 1, H - 1, Lq - 1, hd - 1), NAN),
          Plant("k", (0, H - 1, min(9, Lk - 2), 7), NAN), Plant("k", (P - 1, 0, Lk - 1, hd - 1), NAN)]
    form = "attn_probs<%s,%d>%s%s" % (E.DTN[c.dt], hd, " head mean" if c.mean else " per head", " expanded tail" if (c.tail and c.expand) else "")
    return Case("probs/" + name, "attention", form, functools.partial(ProbsSide, c), ps)


PROBS_NF_CASES = [_probs_case(n) for n in ("lq1_lk17_scalar_stores", "paired_p3_head_mean", "pgca_tail_expanded_512", "pgca_tail_unexpanded_w2.5",
                                           "tail_mid_tile_expanded_head_mean", "f32_paired_head_mean", "f32_hd128_tail_expanded")]


# ==== pair-indexed PGCA forward ===================================================================================================
class PairSide(Side):
    """dl_pgca_pairs_fwd through ops.pgca_pairs on the cases of tests/test_pgca_pairs_gpu.py: protein codes q (n_q, Lq, E), drug
    codes kv (n_kv, Lk, 2E), pairs (pi, di) with repeated and permuted indices, the left copy, the bias.  A NaN in one drug's
    code rows poisons exactly the pairs naming that drug, one in a protein's rows exactly that protein's pairs (and there the
    query row alone); the left copy moves bit patterns."""

    def __init__(self, c, dt, dev):
        self.c, self.dt, self.dev = c, dt, dev
        g = torch.Generator().manual_seed(sum(map(ord, c.name)))
        E_ = PG.E
        self.scale = E_ ** -0.5
        self.q = _place(torch.randn(c.n_q, c.Lq, E_, generator=g) * 0.7, dt, dev)
        self.kv = _place(torch.cat([torch.randn(c.n_kv, c.Lk, E_, generator=g) * 0.7, torch.randn(c.n_kv, c.Lk, E_, generator=g)], dim=2), dt, dev)
        self.left = _place(torch.randn(c.n_q, c.Lq, c.left_cols, generator=g), dt, dev) if c.left_cols else None
        self.bias = (torch.randn(E_, generator=g) * 0.5).to(dev) if c.bias else None
        self.pi = torch.tensor(c.pi, dtype=torch.int32, device=dev)
        self.di = torch.tensor(c.di, dtype=torch.int32, device=dev)
        self.operands = {"q": [self.q], "kv": [self.kv]}
        if self.left is not None:
            self.operands["left"] = [self.left]

    def ref(self):
        c, E_, n = self.c, PG.E, len(self.c.pi)
        pi, di = self.pi.long(), self.di.long()
        Qg, Kg, Vg = self.q[pi].contiguous(), self.kv[di, :, :E_].contiguous(), self.kv[di, :, E_:].contiguous()
        r = A.reference_fwd(Qg, Kg, Vg, n_problems=n, n_heads=1, n_segments=1, partner_shift=0, Lq=c.Lq, Lk=c.Lk, head_dim=E_, scale=self.scale,
                            q_strides=(c.Lq * E_, E_, E_), k_strides=(c.Lk * E_, E_, E_), v_strides=(c.Lk * E_, E_, E_), key_tail=c.tail)
        O = r["O"][0, :, 0]
        if self.bias is not None:
            O = O + self.bias.double()
        out = {"O": O}
        if self.left is not None:
            out["left copy"] = self.left[pi].double()
        return out

    def run(self):
        from druglamp_amd import ops
        c, n = self.c, len(self.c.pi)
        cols = c.left_cols + PG.E
        g = N.Guarded(n * c.Lq * c.pitch, self.dt, self.dev)
        out = g.view((n, c.Lq, cols), (c.Lq * c.pitch, c.pitch, 1))
        before = g.bits()
        got = ops.pgca_pairs(self.q, self.kv, self.pi, self.di, scale=self.scale, left=self.left, bias=self.bias, key_tail=c.tail, out=out)
        assert got is out
        torch.cuda.synchronize()
        g.untouched(c.name, before)
        res = {"O": out[:, :, c.left_cols:].clone()}
        if self.left is not None:
            res["left copy"] = out[:, :, :c.left_cols].clone()
        return res


def _pair_case(name, dt):
    c = PG.CASES[name]
    ps = [Plant("kv", (c.di[min(1, len(c.di) - 1)], min(5, c.Lk - 1), 3), NAN), Plant("kv", (c.di[0], c.Lk - 1, 2 * PG.E - 1), NAN),
          Plant("kv", (c.di[-1], c.Lk - 1, PG.E - 1), NAN), Plant("q", (c.pi[0], c.Lq - 1, PG.E - 1), NAN), Plant("q", (c.pi[-1], min(7, c.Lq - 1), 0), NAN)]
    if c.left_cols:
        ps.append(Plant("left", (c.pi[0], c.Lq - 1, c.left_cols - 1), NAN))
    return Case("pairs/%s-%s" % (name, E.DTN[dt]), "pairs", "pgca_pairs_fwd<%s>" % E.DTN[dt], functools.partial(PairSide, c, dt), ps)


PAIR_NF_CASES = [_pair_case(n, dt) for n, dt in (("a_compact", BF), ("a_compact", F32), ("c_partial_tiles", BF), ("d_tail_bias_padded", BF))]


class RaggedSide(Side):
    """dl_pgca_pairs_ragged_fwd through ops.pgca_pairs_ragged on the row store, the key table and the pairs of
    tests/test_pgca_ragged_gpu.py (a fresh copy of its buffers: the suite's own are shared and never modified)."""

    def __init__(self, name, dt, dev):
        self.s = s = RG.build(name, dt, dev)
        self.c, self.dev = s["c"], dev
        self.row0 = [int(r) for r in s["row0"][:s["n_kv"]]]
        self.operands = {"q": [s["q"]], "rows": [s["rows"]]}
        if s["left"] is not None:
            self.operands["left"] = [s["left"]]

    def ref(self):
        s, c, E_ = self.s, self.c, RG.E
        O = torch.zeros(s["n"], c.Lq, E_, dtype=F64, device=self.dev)
        for d, (Lk, w) in enumerate(c.drugs):
            sel = (s["di"] == d).nonzero().flatten()
            Qg = s["q"][s["pi"][sel].long()].contiguous()
            r0 = self.row0[d]
            Kd, Vd = s["rows"][r0:r0 + Lk, :E_].contiguous(), s["rows"][r0:r0 + Lk, E_:].contiguous()
            r = A.reference_fwd(Qg, Kd, Vd, n_problems=sel.numel(), n_heads=1, n_segments=1, partner_shift=0, Lq=c.Lq, Lk=Lk, head_dim=E_,
                                scale=s["scale"], q_strides=(c.Lq * E_, E_, E_), k_strides=(0, E_, E_), v_strides=(0, E_, E_),
                                key_tail=(c.tail_rows, w) if c.tail_rows else None)
            O[sel] = r["O"][0, :, 0]
        if s["bias"] is not None:
            O = O + s["bias"].double()
        out = {"O": O}
        if s["left"] is not None:
            out["left copy"] = s["left"][s["pi"].long()].double()
        return out

    def run(self):
        c = self.c
        flat, out, mask, before = RG._run(self.s)
        assert torch.equal(RG._bits(flat)[~mask], before[~mask]), "%s: a store outside the addressed elements" % c.name
        res = {"O": out[:, :, c.left_cols:].clone()}
        if c.left_cols:
            res["left copy"] = out[:, :, :c.left_cols].clone()
        return res


def _ragged_case(name, dt):
    c = RG.CASES[name]
    row0, r = [], 0
    for d, (Lk, _) in enumerate(c.drugs):
        if d == len(c.drugs) // 2:
            r += RG.GAP
        row0.append(r)
        r += Lk
    last = len(c.drugs) - 1
    ps = [Plant("rows", (row0[1] + min(3, c.drugs[1][0] - 1), 3), NAN), Plant("rows", (row0[last] + c.drugs[last][0] - 1, RG.E - 1), NAN),
          Plant("rows", (row0[0] + c.drugs[0][0] - 1, 2 * RG.E - 1), NAN), Plant("q", (c.pi[0], c.Lq - 1, RG.E - 1), NAN), Plant("q", (c.pi[-1], min(7, c.Lq - 1), 0), NAN)]
    if c.left_cols:
        ps.append(Plant("left", (c.pi[0], c.Lq - 1, c.left_cols - 1), NAN))
    return Case("ragged/%s-%s" % (name, E.DTN[dt]), "pairs", "pgca_pairs_ragged_fwd<%s>" % E.DTN[dt], functools.partial(RaggedSide, name, dt), ps)


class PairMapSide(Side):
    """dl_pgca_pairs_ragged_probs (the probability maps of the pairs, tail keys expanded or not) and, profile=True,
    dl_pgca_pairs_ragged_profile (key_mass: the mean of a pair's map over its query rows; site_peak: the row maxima; the integer
    site_key is not compared) on a fresh copy of the buffers of tests/test_pgca_pairs_probs_gpu.py."""

    def __init__(self, name, dt, expand, profile, dev):
        self.s = s = PP.build(name, dt, expand, dev)
        self.c, self.dev, self.profile = s["c"], dev, profile
        self.row0 = [int(r) for r in s["row0"][:s["n_kv"]]]
        self.operands = {"q": [s["q"]], "rows": [s["rows"]]}

    def ref(self):
        s, c = self.s, self.c
        want = torch.zeros(s["n"], c.Lq, c.cols, dtype=F64, device=self.dev)
        for d, (Lk, w) in enumerate(c.drugs):
            r0 = self.row0[d]
            pm = PP._drug_map(s["q"].contiguous(), s["rows"][r0:r0 + Lk, :PP.E].contiguous(), c.tail_rows, w, s["expand"], s["scale"])[0]
            sel = (s["di"] == d).nonzero().flatten()
            want[sel, :, :pm.shape[-1]] = pm[s["pi"][sel].long()]
        if not self.profile:
            return {"map": want}
        km, _, peak, _, _ = profile_ref(want, torch.zeros_like(want))
        return {"key_mass": km, "site_peak": peak}

    def run(self):
        s = self.s
        if not self.profile:
            flat, out, mask, before = PP._run(s)
            assert torch.equal(PP._bits(flat)[~mask], before[~mask]), "%s: a store outside the addressed elements" % self.c.name
            return {"map": out.clone()}
        res = PF._run(s)
        for flat, _, mask, before in res:
            assert torch.equal(PP._bits(flat)[~mask], before[~mask]), "%s: a store outside the addressed elements" % self.c.name
        return {"key_mass": res[0][1].clone(), "site_peak": res[1][1].clone()}


def _pairmap_case(name, dt, expand, profile):
    c = PP.CASES[(name, expand)]
    row0, r = [], 0
    for d, (Lk, _) in enumerate(c.drugs):
        if d == len(c.drugs) // 2:
            r += PP.GAP
        row0.append(r)
        r += Lk
    last = len(c.drugs) - 1
    ps = [Plant("rows", (row0[1] + min(3, c.drugs[1][0] - 1), 3), NAN), Plant("rows", (row0[last] + c.drugs[last][0] - 1, PP.E - 1), NAN),
          Plant("q", (c.pi[0], c.Lq - 1, PP.E - 1), NAN), Plant("q", (c.pi[-1], min(7, c.Lq - 1), 0), NAN)]
    kern = "pgca_pairs_ragged_profile" if profile else "pgca_pairs_ragged_probs"
    return Case("%s/%s-%s%s" % ("profile" if profile else "pairprobs", name, E.DTN[dt], "-expanded" if expand else ""), "pairs",
                "%s<%s>%s" % (kern, E.DTN[dt], " expanded" if expand else ""), functools.partial(PairMapSide, name, dt, expand, profile), ps)


PAIRMAP_NF_CASES = ([_pairmap_case(n, dt, e, False) for n, dt, e in (("a_six_layouts", BF, False), ("a_six_layouts", BF, True), ("a_six_layouts", F32, True),
                                                                     ("b_no_tail", F32, True))] +
                    [_pairmap_case(n, dt, True, True) for n, dt in (("a_six_layouts", BF), ("a_six_layouts", F32), ("b_no_tail", BF))])


class AttrSide(Side):
    """dl_pgca_pairs_ragged_attr (gradient x code per drug key and per protein site) with the left half: planted through the
    incoming gradients d_out / d_sites and through the codes it re-reads (q, the drug rows, the site codes)."""

    def __init__(self, name, dt, dev):
        self.s = s = PP.build(name, dt, True, dev)
        self.c, self.dev = s["c"], dev
        c = self.c
        g = torch.Generator().manual_seed(4242)
        grad = PP._nan_view(s["n"], c.Lq, 2 * PP.E, dt, 0.05 * torch.randn(s["n"], c.Lq, 2 * PP.E, generator=g), dev)
        sites = PP._nan_view(c.n_q, c.Lq, PP.E, dt, 0.7 * torch.randn(c.n_q, c.Lq, PP.E, generator=g), dev)
        self.x = dict(d_out=grad[..., PP.E:], d_sites=grad[..., :PP.E], sites=sites)
        self.operands = {"d_out": [self.x["d_out"]], "d_sites": [self.x["d_sites"]], "sites": [sites], "q": [s["q"]], "rows": [s["rows"]]}

    def ref(self):
        r = attr_ref.case_reference(self.s, self.x, True)
        return {"key_attr": r["key"], "site_attr": r["site"]}

    def run(self):
        res = AT._run(self.s, self.x, True)
        for flat, _, mask, before in res:
            assert torch.equal(PP._bits(flat)[~mask], before[~mask]), "%s: a store outside the addressed elements" % self.c.name
        return {"key_attr": res[0][1].clone(), "site_attr": res[1][1].clone()}


def _attr_case(name, dt):
    c = PP.CASES[(name, True)]
    n = len(c.pi)
    ps = [Plant("d_out", (1, min(5, c.Lq - 1), 3), NAN), Plant("d_out", (n - 1, c.Lq - 1, PP.E - 1), NAN), Plant("d_sites", (0, c.Lq - 1, 2), NAN),
          Plant("sites", (c.pi[1], 3, 1), NAN), Plant("q", (c.pi[0], c.Lq - 1, PP.E - 1), NAN), Plant("rows", (min(3, c.drugs[0][0] - 1), 3), NAN)]
    return Case("attr/%s-%s" % (name, E.DTN[dt]), "pairs", "pgca_pairs_ragged_attr<%s> sites" % E.DTN[dt], functools.partial(AttrSide, name, dt), ps)


ATTR_NF_CASES = [_attr_case(n, dt) for n, dt in (("a_six_layouts", BF), ("a_six_layouts", F32), ("b_no_tail", BF))]


RAGGED_NF_CASES = [_ragged_case(n, dt) for n, dt in (("a_six_layouts", BF), ("a_six_layouts", F32), ("b_no_tail", BF))]


# ==== eval-mode / frozen BatchNorm backward =======================================================================================
BE_BY_NAME = {c.name: c for c in BE.CASES}
BE_PICK = ["wide128_r33", "wide64_win", "wide256_rw_r333", "bf16_c40_r33", "bf16_c128_misaligned_win", "f32_c128_r33", "f32_c256_rw_r100"]


class BnEvalSide(Side):
    """dl_bn_eval_bwd (the backward of a BatchNorm on fixed statistics: eval mode and frozen fine-tuning) with sums, under the
    three ReLU masks of the suite; planted through the incoming gradient dz only (y, mean and rstd are saved tensors)."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        w64, rw, self.win, y, dz, mean, rstd, gamma, beta = BE.case_data(c)
        self.w = w64.to(dev)
        pl = lambda v, dt, off=0: N.Guarded(v.numel() + off, dt, dev).view(tuple(v.shape), off=off).copy_(v)
        self.y, self.dz = pl(y, c.dt, c.off), pl(dz, c.dt, c.off)
        self.y[self.w < 0] = float("nan")
        self.dz[self.w < 0] = float("nan")
        self.mean, self.rstd, self.gamma, self.beta = (pl(t, F32) for t in (mean, rstd, gamma, beta))
        self.rw = None if rw is None else pl(rw, F32)
        self.operands = {"dz": [self.dz]}

    def ref(self):
        out = {}
        for ri, ro in BE.MASKS:
            dx, sums, _ = ber.bn_eval_bwd(self.dz, self.y, self.w, self.mean, self.rstd, self.gamma, self.beta, ri, ro)
            out["dx[relu_in=%d,relu_out=%d]" % (ri, ro)], out["sums[relu_in=%d,relu_out=%d]" % (ri, ro)] = dx, sums
        return out

    def run(self):
        L, ok, stream, DT, _ = _lib()
        c, dev = self.c, self.dev
        R, Cc, dt = c.R, c.C, c.dt
        win, halo, valid = self.win
        ws = torch.empty(L.dl_bn_workspace_bytes(R, Cc), dtype=torch.uint8, device=dev)
        out = {}
        for ri, ro in BE.MASKS:
            gd = N.Guarded(R * Cc + c.off, dt, dev)
            dx = gd.view((R, Cc), off=c.off)
            sg, sums = _outbuf((2 * Cc,), F32, dev)
            wide = dt == BF and Cc in (64, 128, 256) and all(t.data_ptr() % 16 == 0 for t in (self.dz, self.y, dx))
            assert wide == c.wide, "%s: the case names the other form" % c.name
            before = (gd.bits(), sg.bits())
            ok(L.dl_bn_eval_bwd(self.dz.data_ptr(), self.y.data_ptr(), self.mean.data_ptr(), self.rstd.data_ptr(), self.gamma.data_ptr(),
                                self.beta.data_ptr() if ro else None, ri, ro, dx.data_ptr(), sums.data_ptr(), R, Cc, win, halo, valid, N._ptr(self.rw),
                                DT[dt], ws.data_ptr(), ws.numel(), stream), "dl_bn_eval_bwd")
            torch.cuda.synchronize()
            gd.untouched(c.name, before[0])
            sg.untouched(c.name, before[1])
            out["dx[relu_in=%d,relu_out=%d]" % (ri, ro)], out["sums[relu_in=%d,relu_out=%d]" % (ri, ro)] = dx.clone(), sums.clone()
        return out


def _bn_eval_case(name):
    c = BE_BY_NAME[name]
    w64 = BE.case_data(c)[0]
    live = [int(i) for i in (w64 >= 0).nonzero().flatten()]
    ps = [Plant("dz", (live[min(2, len(live) - 1)], min(5, c.C - 1)), NAN), Plant("dz", (live[-1], c.C - 1), NAN)]
    form = "bn_eval_bwd_wide_kernel<SUMS, RELU_OUT>" if c.wide else "bn_eval_bwd_kernel<%s, SUMS>" % ("bf16" if c.dt == BF else "float")
    return Case("bn_eval/" + name, "batchnorm", form, functools.partial(BnEvalSide, c), ps)


BN_EVAL_NF_CASES = [_bn_eval_case(n) for n in BE_PICK]

ALL_CASES = GEMM_CASES + LN_NF_CASES + BN_NF_CASES + COS_NF_CASES + CE_NF_CASES + TRI_NF_CASES + NTX_NF_CASES + ELEM_NF_CASES + ATTN_NF_CASES + PROBS_NF_CASES + PAIR_NF_CASES + RAGGED_NF_CASES + PAIRMAP_NF_CASES + ATTR_NF_CASES + BN_EVAL_NF_CASES


def expected_form(case, side):
    """The launch form(s) the host dispatch gives the case's operands, from the suites' own mirrors (CPU test)."""
    fam = case.name.split("/")[0]
    if fam == "gemm":
        c = side.c
        if c.kind == "gemm":
            return GR.select(c)
        if c.kind == "pair":
            return "pair " + GR.select(c.members[0], pair=True)
        return case.form                                   # group: tests/test_gemm_reference_cpu.py pins the plan against the library
    if fam == "ln":
        return "%s + %s" % side.forms()
    if fam == "bn":
        return " | ".join(side.forms()) + (" | " + " | ".join(N.RELU_FORMS) if side.plain else "")
    c = side.c if hasattr(side, "c") else None
    if case.name.startswith("elem/normadj"):
        return E.norm_adj_form(c.n)[0]
    if case.name.startswith("elem/gateb"):
        return E.gate_bwd_form(c.hd)
    if case.name.startswith("elem/rowssum"):
        return side.form()
    if case.name.startswith("elem/aggregate"):
        return "graph_aggregate_kernel<T, 128>" if c.n <= 128 else "graph_aggregate_any_kernel<T, 128>"
    return case.form


# ==== the kernel tests ============================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_nonfinite_values_pass_through(case):
    drive(case)


# ==== end to end ==================================================================================================================
def _trainer(dtype, seed=0):
    from druglamp_amd import ops
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.trainer import Trainer
    torch.manual_seed(seed)
    ops.manual_seed(seed + 1)
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    model = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    tr = Trainer(model, cfg, device=torch.device(DEV), compute_dtype=dtype)
    tr.set_lrs(1e-4)
    return model, tr


@functools.lru_cache(maxsize=None)
def _train_batch(graph=False):
    """(batch, meta) of 8 pairs: pre-extracted drug features, or (graph=True) dense molecular graphs through the MolecularGCN."""
    from druglamp_amd.synthetic import make_batch
    return make_batch(8, torch.device(DEV), seed=7, with_graph=graph)


def _plant_batch(batch, plant):
    """The batch with one NaN: `xp` one protein-LLM element, `vd` one pre-extracted drug feature element, `graph` one node
    feature of one real atom of a molecular graph (its way to the loss goes through the ReLU epilogues and the BatchNorm of the
    MolecularGCN).  Works on any device."""
    feat_d, vp, y, xd, xp = batch
    xp, xd = xp.clone(), xd.clone()
    if plant == "xp":
        xp[(3,) + _first_real(xp, 3)] = float("nan")
    elif plant == "vd":
        feat_d = feat_d.clone()
        feat_d[(5,) + _first_real(feat_d, 5)] = float("nan")
    elif plant == "graph":
        h, adj = feat_d[0].clone(), feat_d[1].clone()
        h[5, 2, 7] = float("nan")                          # (every molecule of make_batch has at least 10 atoms)
        feat_d = (h, adj)
    elif isinstance(feat_d, tuple):
        feat_d = (feat_d[0].clone(), feat_d[1].clone())
    return feat_d, vp, y, xd, xp


def _first_real(t, sample):
    """(row, column) of a non-zero element of sample `sample` of a (B, rows, C) feature tensor (zero rows are padding)."""
    nz = (t[sample] != 0).nonzero()
    return int(nz[len(nz) // 2][0]), int(nz[len(nz) // 2][1])


@functools.lru_cache(maxsize=None)
def _oracle_cls(plant, graph):
    """The fp64 oracle's cls loss of the batch-8 training-mode forward on the seed-0 weights, with the plant."""
    from oracle import druglamp_oracle as O
    model, _ = _trainer(torch.float32)
    cpu = lambda t: tuple(cpu(u) for u in t) if isinstance(t, tuple) else t.detach().cpu()
    feat_d, vp, y, xd, xp = _plant_batch(tuple(cpu(t) for t in _train_batch(graph)[0]), plant)
    xd, xp = xd.double(), xp.double()
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    with torch.no_grad():
        vd = O.molecular_gcn(sd, "drug_extractor", feat_d[0].double(), feat_d[1].double(), True) if graph else feat_d.double()
        score = O.model_forward(sd, "DrugLAMP", vd, vp, xd, xp, bn_training=True)["score"]
        n, yy = torch.sigmoid(score).squeeze(1), y.double()                # (F.binary_cross_entropy refuses a NaN input on the CPU:
        return float(-(yy * torch.log(n) + (1 - yy) * torch.log(1 - n)).mean())   # the mean BCE of oracle.bce_loss from its definition)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("plant", ["xp", "vd", "graph"])
def test_training_step_loss_shows_a_nan_input(dtype, plant):
    """One NaN in one protein-LLM element / one pre-extracted drug feature element / one node feature of a molecular graph of a
    batch of 8: the cls loss of the step is not finite, as the fp64 oracle gives on the same batch.  The graph plant reaches
    the loss only through the ReLU epilogues and the training BatchNorm of the MolecularGCN; the other two through GELU,
    LayerNorm and attention, and all three through binary_cross_entropy, whose device kernel asserts on a NaN."""
    graph = plant == "graph"
    assert math.isfinite(_oracle_cls("none", graph)) and math.isnan(_oracle_cls(plant, graph)), "the oracle does not carry the NaN to the loss"
    batch, meta = _train_batch(graph)
    _, tr = _trainer(dtype)
    clean = float(tr.training_step(_plant_batch(batch, "none"), meta=meta if graph else None, cur_epoch=1)["cls"])
    assert math.isfinite(clean), clean
    _, tr = _trainer(dtype)
    got = float(tr.training_step(_plant_batch(batch, plant), meta=meta if graph else None, cur_epoch=1)["cls"])
    print("cls loss: clean %.6f, with a NaN in %s: %r" % (clean, plant, got))
    assert not math.isfinite(got), "a NaN in %s left the cls loss finite (%r)" % (plant, got)
    arena = tr.flat.arena.detach()
    assert not bool(torch.isfinite(arena).all()), "the step's parameter update is finite although the loss is not"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_screening_scores_show_a_nan_entity_and_only_it(dtype):
    """A drug whose features hold one NaN scores NaN against every protein and every other score of the library is bitwise
    what the clean library gives; the same for a protein."""
    from tests import test_drug_library_gpu as DL
    from druglamp_amd.trainer import Trainer
    m, cfg = DL._model("DrugLAMP", dtype)
    tr = Trainer(m, cfg, device=DL.DEV, compute_dtype=dtype)
    m.eval()
    vd, vp, _, xd, xp = DL._data()
    vd, xd, xp = vd.clone(), xd.to(dtype).clone(), xp.to(dtype).clone()
    vp, xp = vp[:2], xp[:2]

    def scores():
        lib = tr.build_library([(vd[:2], xd[:2]), (vd[2:], xd[2:])], hints=[DL._hints(), None])
        return tr.screen_library([(vp[:1], xp[:1]), (vp[1:], xp[1:])], lib, pair_batch=5).clone()

    clean = scores()
    assert clean.shape == (2, DL.ND) and bool(torch.isfinite(clean).all())
    for what, t, ent in (("drug v", vd, 1), ("drug x", xd, 2), ("protein x", xp, 1)):
        idx = (ent,) + _first_real(t, ent)
        with planted([t], idx, NAN):
            got = scores()
        hit = torch.zeros_like(clean, dtype=torch.bool)
        if what.startswith("drug"):
            hit[:, ent] = True
        else:
            hit[ent, :] = True
        print("%s %d: scores %s" % (what, ent, got.tolist()))
        assert bool(torch.isnan(got[hit]).all()), "a NaN in %s %d left one of its scores finite: %s" % (what, ent, got.tolist())
        assert torch.equal(NF.bits(got)[~hit], NF.bits(clean)[~hit]), "a NaN in %s %d changed another entity's score" % (what, ent)
    assert torch.equal(NF.bits(scores()), NF.bits(clean))
