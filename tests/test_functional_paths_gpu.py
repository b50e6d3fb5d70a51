"""Every autograd Function of druglamp_amd/functional.py (the layer above the kernels: fixed sequences of launches with
hand-written backward passes) element by element against fp64 autograd of the plain formulations in tests/fn_ref.py.

Every output and every returned gradient of every case is compared:

    |got_i - ref64_i| <= K x E_r,   E_r = max over row r (last dimension) of |plain_i - ref64_i|, floored by the median of E_r,

where `plain` is the same formulation evaluated in plain torch on the CPU at the compute dtype (fp32, or bf16 with every op
rounded to bf16) from the same operands and masks: the bound is measured against the reference, never against the code under
test.  K = 4 for bf16 (the kernels round only stores and accumulate in fp32), K = 8 for fp32 (fast exp, the gelu' fit,
another summation order).  Pure data movers and casts are bit-exact.
Terms added to single tensors' bounds (fn_ref.extra_bound), all in ProteinCNNFn, where the contraction of a weight gradient
runs over the R = B S = 600 to 900 rows of the batch and a row of the returned (C, C, k) gradient has only k = 3, 6 or 9
elements: with the envelope alone, 1 or 2 of the 49152 elements of grad:conv0.w missed K x E_r by a factor of 1.03 to 1.32 in
five fp32 cases and one bf16 case, and one of 128 batch variances (out:var1, fp32) by 1.07, all with correct wiring (every
other tensor of those cases, and the same tensors in the other cases, inside).  The plain evaluation sums these rows blocked
on the CPU, the kernels one after another in fp32 slabs.  The accumulation model of tests/test_gemm_paths_gpu.py is added with
independent roundings (a random walk over the R terms, as fn_ref.cnn_relu_tol takes it): 8 sqrt(R) u_f l2 with
l2 = sqrt(sum (dpre x)^2) for grad:conv<i>.w and the same for the column sum behind the training-mode out:var<i>; about as
large as K x E_r itself in fp32.  In the compact layouts in bf16 a representative row's dpre is stored (rounded to bf16) once
and counts with its multiplicity m, so its rounding enters the weight gradient coherently where the expanded plain evaluation
rounds every copy separately (one element of cnn_train_compact_pool_bf16 missed by 1.22): 5 x 2^-9 sqrt(m_max / 3) l2 of the
same store model is added there.  K is unchanged.

Each case runs forward and backward twice on fresh leaves and must repeat bitwise; the upstream gradient is random; every
Function has at least one case whose upstream gradient is non-contiguous (the leading columns of a wider buffer, or a
transposed view).  Dropout masks are those of the integer replica (tests/elem_ref.keep_mask) under the seeds
ops.manual_seed / ops.next_seed hand out, replayed on the CPU.  ReLU: an element is open by the sign of the reference's own
fp64 pre-activation, except within the rounding of that pre-activation, where the kernel's choice (y > 0) is taken; the share
resolved that way is capped (tests/test_functional_reference_cpu.py asserts the cap from the reference alone).

Uninitialised memory: the Functions that allocate with torch.empty run once, the caching allocator's free blocks are filled
with NaN patterns, and the second run must give bitwise the same outputs and gradients.

FORMS (tests/fn_ref.py) maps every Function branch to the condition that selects it; the CPU test asserts that the cases
here, the tests named in fn_ref.ELSEWHERE and the branches listed in fn_ref.OPEN cover it exactly.
DL_FN_BOUND_LOG=<file>: every comparison appends one JSON line; tools/functional_bound_margins.py reduces one run to
profiles/functional_bound_margins.txt.
"""
import collections

import pytest
import torch

from tests import elem_ref as er
from tests import fn_ref as R
from tests.fn_ref import BF, F32, Case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CAST_CASES = [Case("cast_%s_%s_to_%s" % (lay, R.DTN[src], R.DTN[dst]), "cast", src, ("CastFn " + form,), dict(src=src, dst=dst, layout=lay))
              for (lay, form) in (("contig", "contiguous"), ("permuted", "permuted-dense"), ("sliced", "non-dense"))
              for (src, dst) in ((F32, BF), (BF, F32))]


# ---- running a case on the device ----------------------------------------------------------------------------------------------------
def _layout(t, mode):
    """The upstream gradient as the device sees it: same values, the layout the case asks for."""
    if mode == "slice":
        big = torch.full(t.shape[:-1] + (t.shape[-1] + 8,), 3.0, dtype=t.dtype, device=t.device)
        big[..., :t.shape[-1]] = t
        return big[..., :t.shape[-1]]
    if mode == "perm":
        return t.transpose(0, 1).contiguous().transpose(0, 1)
    return t.contiguous()


def _fn():
    from druglamp_amd import functional
    return functional


def hip_block(c, D):
    k = c.cfg
    S = 2 if k["paired"] else 1
    params = [D[n] for s in range(S) for n in R.block_param_names(k["paired"], s)]
    return dict(y=_fn().transformer_block(D["x"], k["paired"], k["H"], k.get("p", 0.0), True, 1e-6, params))


def hip_linear(c, D):
    return dict(y=_fn().LinearFn.apply(D["x"], D["weight"], D.get("bias"), D.get("pe"), c.cfg.get("p", 0.0), True))


def hip_addpe(c, D):
    return dict(y=_fn().AddPeDropoutFn.apply(D["x"], D["pe"], c.cfg.get("p", 0.0), True))


def hip_layernorm(c, D):
    y = _fn().layer_norm(D["x"], D["ln.w"], D["ln.b"], 1e-5)
    return dict(y=y, m=_fn().TokenMeanFn.apply(y)) if c.cfg["mode"] in ("mean", "L1") else dict(y=y)


def hip_pgca(c, D):
    k = c.cfg
    # seq-first views of batch-first tensors, as the callers pass them
    y, second = _fn().GuidedCrossAttentionFn.apply(D["q"].permute(1, 0, 2), D["k"].permute(1, 0, 2), D["in_w"], D.get("in_b"), D["out_w"],
                                                   D.get("out_b"), k["H"], k["second"] == "raw", k.get("tail"), k["second"] == "probs")
    assert (second is None) == (k["second"] is None)
    return dict(y=y) if second is None else {"y": y, k["second"]: second}


def hip_gate(c, D):
    return dict(y=_fn().TokenGateFn.apply(D["v"], D["lin1.w"], D["lin1.b"], D["lin2.w"], D["lin2.b"], c.cfg["H"], c.cfg["res"]))


def hip_dense(c, D):
    k = c.cfg
    return dict(y=_fn().dense(D["x"], D["weight"], D.get("bias"), D.get("residual"), k.get("act", False), bool(k.get("weight_t"))))


def hip_fillpool(c, D):
    fill, pooled = _fn().FillPoolFn.apply(D["x"], c.cfg["site_len"], c.cfg["out_dt"])
    return dict(fill=fill, pooled=pooled)


_SIDE = {}            # case name -> the kernel's own ReLU choices (y > 0), read from what the Function saved for its backward


def hip_cnn(c, D):
    from druglamp_amd.protein_plan import ProteinPlan
    Fn, k = _fn(), c.cfg
    B, S, C, lay, training = k["B"], k["S"], k["C"], k["layout"], k["training"]
    params = [D["%s%d.%s" % (m, i, n)] for i in range(3) for m, n in (("conv", "w"), ("conv", "b"), ("bn", "w"), ("bn", "b"), ("bn", "rm"), ("bn", "rv"))]
    momenta = (0.1, 0.1, 0.1) if training else None
    row_of = None
    if lay in ("plain", "pooled"):
        x = torch.nn.functional.pad(D["x"], (0, 0, 4, 4))
        outs = Fn.ProteinCNNFn.apply(x, training, R.CNN_EPS, k["site_len"] if lay == "pooled" else 0, momenta, False, None, 0, *params)
    elif lay == "raw_dx":
        x = Fn.EmbedPadFn.apply(D["ids"], D["emb"], D["fill"], 0)
        outs = Fn.ProteinCNNFn.apply(x, training, R.CNN_EPS, 0, momenta, True, None, 0, *params)
    else:
        plan = ProteinPlan(k["lengths"][:B], S, bucket=8)
        assert plan.rows < B * S and all(p > 0 for p in plan.period), "the lengths give no compact plan"
        src, w, rep, row_of = (torch.from_numpy(a).to(DEV) for a in (plan.src, plan.w, plan.rep, plan.row_of))
        x = Fn.EmbedRowsFn.apply(D["ids"], D["emb"], D["fill"], 0, src, None)
        outs = Fn.ProteinCNNFn.apply(x, training, R.CNN_EPS, 0, momenta, True, w, plan.n, *params)
    z = outs[0]
    sv = z.grad_fn.saved_tensors
    side = {}
    for i in range(3):
        y = sv[i * 5 + 1]
        body = y[row_of.long()].view(B, S, C) if row_of is not None else y.view(B, S + 8, C)[:, 4:-4]
        side["y%d" % i] = (body.transpose(1, 2) > 0).cpu()
    _SIDE[c.name] = side
    if lay == "compact":
        z = Fn.ExpandRowsFn.apply(z, row_of, rep)
    elif lay == "compact_pool":
        z = Fn.SitePoolRowsFn.apply(z, row_of, rep, B, S, k["site_len"])
    res = collections.OrderedDict(y=z)
    for i in range(3):
        res["mean%d" % i], res["var%d" % i] = outs[1 + 2 * i], outs[2 + 2 * i]
    return res


def hip_mlp(c, D):
    """run_mlp over an nn.Sequential whose parameters are the case's leaves; the fused BatchNorm -> ReLU output is recorded on
    the way (the kernel's own choice of the ReLU side)."""
    import torch.nn as nn
    Fn, k = _fn(), c.cfg
    seq = nn.Sequential(nn.Linear(k["K"], k["N1"]), nn.BatchNorm1d(k["N1"]), nn.ReLU(), nn.Linear(k["N1"], k["N2"], bias=False), nn.BatchNorm1d(k["N2"])).to(DEV)

    def put(mod, name, t):
        mod._parameters.pop(name, None)
        mod._buffers.pop(name, None)
        object.__setattr__(mod, name, t)
    put(seq[0], "weight", D["l0.w"]), put(seq[0], "bias", D["l0.b"]), put(seq[3], "weight", D["l1.w"])
    for i, m in ((0, seq[1]), (1, seq[4])):
        put(m, "weight", D["bn%d.w" % i]), put(m, "bias", D["bn%d.b" % i]), put(m, "running_mean", D["bn%d.rm" % i]), put(m, "running_var", D["bn%d.rv" % i])
    seq.train(k["training"])
    side, orig = {}, (Fn.batch_norm_rows, Fn.batch_norm_rows_weighted_tail)

    def rec(f):
        def g(bn, x2d, *a, **kw):
            y = f(bn, x2d, *a, **kw)
            if kw.get("relu"):
                side["y0"] = (y.detach() > 0).cpu()
            return y
        return g
    Fn.batch_norm_rows, Fn.batch_norm_rows_weighted_tail = rec(orig[0]), rec(orig[1])
    try:
        y = Fn.run_mlp(seq, D["x"], tail=k.get("tail") if k.get("tail") else None)
    finally:
        Fn.batch_norm_rows, Fn.batch_norm_rows_weighted_tail = orig
    assert "y0" in side and y.shape[1] == k["N2"]
    _SIDE[c.name] = side
    return dict(y=y)


HIP = {"mlp": hip_mlp, "cnn": hip_cnn,
       "expandrows": lambda c, D: dict(y=_fn().ExpandRowsFn.apply(D["z"], D["row_of"], D["rep"])),
       "sitepoolrows": lambda c, D: dict(y=_fn().SitePoolRowsFn.apply(D["z"], D["row_of"], D["rep"], len(c.cfg["lengths"]), c.cfg["S"], c.cfg["site_len"])), "block": hip_block, "linear": hip_linear, "addpe": hip_addpe, "layernorm": hip_layernorm, "pgca": hip_pgca, "gate": hip_gate,
       "dense": hip_dense, "fillpool": hip_fillpool,
       "concat2": lambda c, D: dict(y=_fn().Concat2Fn.apply(D["a"], D["b"])),
       "tokenmean": lambda c, D: dict(y=_fn().TokenMeanFn.apply(D["x"])),
       "expandtail": lambda c, D: dict(y=_fn().ExpandTailFn.apply(D["x"], c.cfg["lead"], c.cfg["w"])),
       "sitepool": lambda c, D: dict(y=_fn().SitePoolFn.apply(D["x"], c.cfg["site_len"])),
       "graphagg": lambda c, D: dict(y=_fn().GraphAggregateFn.apply(D["ahat"], D["feat"])),
       "embedding": lambda c, D: dict(y=_fn().EmbeddingFn.apply(D["ids"], D["weight"], c.cfg.get("padding_idx"))),
       "embedrows": lambda c, D: dict(y=_fn().EmbedRowsFn.apply(D["ids"], D["emb"], D["fill"], c.cfg.get("padding_idx"), D["src"], None)),
       "embedpad": lambda c, D: dict(y=_fn().EmbedPadFn.apply(D["ids"], D["weight"], D["fill"], c.cfg.get("padding_idx")))}


def run_hip(c, data):
    """One forward + backward on fresh leaves: 'out:<name>' / 'grad:<leaf>' -> CPU tensors."""
    from druglamp_amd import ops
    ops.manual_seed(R.SEED0)
    D = collections.OrderedDict()
    for name, (t, role, want) in data.leaf.items():
        D[name] = t.to(DEV) if role == "int" else t.to(DEV).detach().clone().requires_grad_(want)
    try:
        outs = HIP[c.kind](c, D)
        names = [n for n in outs if n in data.dy]
        assert names == list(data.dy), (names, list(data.dy))
        torch.autograd.backward([outs[n] for n in names], [_layout(data.dy[n][0].to(DEV), data.dy[n][1]) for n in names])
        torch.cuda.synchronize()
    except RuntimeError as e:
        if any(w in str(e) for w in ("illegal memory access", "HIP error", "hipError")):
            pytest.exit("%s: the device reported %s; nothing more runs on it in this process" % (c.name, e), returncode=3)
        raise
    finally:
        ops.manual_seed(0x5EED)
    res = collections.OrderedDict(("out:" + n, o.detach().cpu()) for n, o in outs.items())
    for name, (t, role, want) in data.leaf.items():
        if want:
            assert D[name].grad is not None, "%s: no gradient reached %s" % (c.name, name)
            res["grad:" + name] = D[name].grad.detach().cpu()
    return res


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(c, a, b, what):
    assert list(a) == list(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and torch.equal(_bits(a[key]), _bits(b[key])), \
            "%s: %s %s (%d elements differ)" % (c.name, key, what, int((_bits(a[key]) != _bits(b[key])).sum()))


_DATA = {}


def data_of(c):
    if c.name not in _DATA:
        _DATA[c.name] = R.build(c)
    return _DATA[c.name]


# ---- the cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_function_against_fp64_autograd(c):
    data = data_of(c)
    got = run_hip(c, data)
    again = run_hip(c, data)
    same_bits(c, got, again, "does not repeat bitwise")
    k = c.cfg
    kernel = None
    if c.kind == "dense" and k.get("act") == "relu":
        kernel = {"y": got["out:y"][..., :k["N"]] > 0}
    if c.kind in ("cnn", "mlp"):
        kernel = dict(_SIDE[c.name])
    ref, plain, ctx = R.reference(c, data, kernel)
    for name, share in ctx.share.items():
        assert share <= R.RELU_CAP[c.dt], "%s: %.3g of %s resolved by the kernel's own choice" % (c.name, share, name)
    # dtypes: activations and their gradients in the compute dtype, parameter gradients in fp32
    for name, (t, role, want) in data.leaf.items():
        if want:
            assert got["grad:" + name].dtype == t.dtype, "%s: grad:%s is %s" % (c.name, name, got["grad:" + name].dtype)
    R.check_case(c, got, ref, plain, ctx)
    if c.kind == "dense" and "residual" not in data.leaf:
        pad = got["out:y"][..., k["N"]:]
        assert not bool((_bits(pad) != 0).any()), "%s: padded output columns are not exactly +0" % c.name
    if c.kind in ("embedding", "embedpad", "embedrows") and k.get("padding_idx") is not None:
        assert not bool((_bits(got["grad:emb" if c.kind == "embedrows" else "grad:weight"][k["padding_idx"]]) != 0).any()), "%s: the padding_idx row of dw is not exactly zero" % c.name
    if c.kind == "linear" and "x" in k.get("want", ("x",)) and k.get("p", 0) > 0:
        # the mask itself: exactly the replica's dropped elements are +0 in the output
        keep = torch.from_numpy(er.keep_mask(R.seeds(R.SEED0, 1)[0], k["B"] * k["L"], k["N"], er.dropout_thr16(k["p"]))).reshape(got["out:y"].shape)
        assert not bool((_bits(got["out:y"])[~keep] != 0).any()) and bool((got["out:y"][keep] != 0).any()), c.name + ": dropped elements"


@pytest.mark.parametrize("c", CAST_CASES, ids=lambda c: c.name)
def test_cast_function_layouts_bit_for_bit(c):
    Fn = _fn()
    k = c.cfg
    g = R._gen(c.name)
    base = (torch.randn((5, 33, 48), generator=g) * 3).to(k["src"]).to(DEV).requires_grad_(True)

    def view(t):
        t = t.clone()
        return t if k["layout"] == "contig" else (t.permute(1, 0, 2) if k["layout"] == "permuted" else t[:, :, :40])
    runs = []
    for _ in range(2):
        x = view(base)
        y = Fn.cast(x, k["dst"])
        dyb = (torch.randn((5, 33, 48), generator=R._gen(c.name + "dy")) * 3).to(k["dst"]).to(DEV)
        dy = view(dyb)
        dx, = torch.autograd.grad(y, x, dy)
        runs.append((y.detach(), dx))
        assert y.dtype == k["dst"] and dx.dtype == k["src"]
        assert torch.equal(_bits(y.detach().cpu()), _bits(er.cast(x.detach().cpu(), k["dst"]))), c.name + ": forward values"
        assert torch.equal(_bits(dx.cpu()), _bits(er.cast(dy.cpu(), k["src"]))), c.name + ": gradient values"
        if k["layout"] == "sliced":
            assert y.is_contiguous() and dx.is_contiguous()
        else:
            assert y.stride() == x.stride() and dx.stride() == dy.stride(), "%s: strides %s / %s, input %s" % (c.name, y.stride(), dx.stride(), x.stride())
            assert y.is_contiguous() == (k["layout"] == "contig")
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    R._blog(c, "out:y", c.dt, 0.0)
    R._blog(c, "grad:x", c.dt, 0.0)


# ---- uninitialised memory -------------------------------------------------------------------------------------------------------------
def poison_free_blocks():
    """Fill every free block of the caching allocator (up to 64 MiB each) with 0xFF bytes: NaN in bf16 and in fp32."""
    torch.cuda.synchronize()
    sizes = sorted((b["size"] for seg in torch.cuda.memory_snapshot() for b in seg["blocks"] if b["state"] == "inactive" and b["size"] <= (64 << 20)),
                   reverse=True)
    held = [torch.empty(s, dtype=torch.uint8, device=DEV).fill_(0xFF) for s in sizes]
    torch.cuda.synchronize()
    n = len(held)
    del held
    return n


@pytest.mark.parametrize("name", ["pgca_raw_h1_bf16", "pgca_tail_w5_f32", "block_paired_drop_bf16", "block_self_f32", "expandtail_bf16",
                                  "dense_k641_n100_gelu_bf16", "dense_residual_gelu_n36_f32", "cnn_train_raw_dx_bf16", "cnn_train_plain_f32",
                                  "cnn_train_compact_f32", "cnn_eval_frozen_raw_dx_bf16", "mlp_tail_train_bf16", "mlp_eval_f32", "mlp_eval_frozen_bf16"])
def test_no_unwritten_torch_empty_memory_reaches_a_result(name):
    """GuidedCrossAttentionFn (o, raw, dqp, dkv, din_w, din_b), TransformerBlockFn (qkv, a, out, pre, da, dqkv, dx), ExpandTailFn
    (out, dy), DenseFn with `pre` and ProteinCNNFn (y, dprev: the GEMMs write only rows [pl, pl + Mg), the halo rows of the
    backward's buffers hold junk by the Function's own comment) allocate with torch.empty and rely on their launches to write every element that is read."""
    c = R.BY_NAME[name]
    data = data_of(c)
    first = run_hip(c, data)
    assert poison_free_blocks() > 0
    probe = torch.empty(first["out:y"].shape, dtype=first["out:y"].dtype, device=DEV)
    vacuous = not bool(torch.isnan(probe).all())
    del probe
    assert not vacuous, "%s: a torch.empty of the output's size does not come back holding the NaN pattern: the test would prove nothing" % name
    second = run_hip(c, data)
    same_bits(c, first, second, "changes when the allocator's free blocks hold NaN")
