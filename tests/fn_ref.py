"""fp64 references of the autograd Functions of druglamp_amd/functional.py, their cases, and the element-wise checker.

Every reference is a plain-torch formulation of the Function's docstring contract (taken from oracle/druglamp_oracle.py where
it has one: pmma_attention_*, _mlp, mhla_forward, pgca_forward, protein_cnn's view) differentiated by torch autograd.  One
formulation serves twice: evaluated in fp64 it is the reference, evaluated at the compute dtype (fp32, or bf16 with every
op rounded to bf16) it is the "plain" computation whose own distance from the reference gives the bound (see `envelope`).
Both read the operands the Function reads: inputs already rounded to the compute dtype, fp32 master weights rounded as
functional.lowp rounds them (to nearest even).  Biases, LayerNorm / BatchNorm parameters and running statistics, which the
Functions read in fp32, are exact in the fp64 reference; the plain bf16 evaluation rounds them to bf16 like every other
operand of an op ("every op rounded to bf16") and returns their gradients in bf16, so the bf16 envelope behind such a
parameter holds that 2^-9 too and is somewhat wider than the kernels' own rounding.  Dropout masks come from the integer
replica tests/elem_ref.keep_mask with the seeds that ops.manual_seed / ops.next_seed hand out (`seeds` replays the generator),
in the order the forward draws them.  Compact forms (key_tail, ExpandTailFn, and the ProteinPlan layouts of EmbedRowsFn ->
ProteinCNNFn -> ExpandRowsFn / SitePoolRowsFn) are referenced by the expanded computation on every row, so that the expected
gradient of a representative row is the sum over the rows it stands for.  ReLU: Ctx.relu, dense_relu_tol, cnn_relu_tol.

Nothing here needs a GPU: tests/test_functional_reference_cpu.py pins the references, the data conditions, the FORMS table
and the checker; tests/test_functional_paths_gpu.py runs the Functions.
"""
import collections
import json
import math
import os

import torch
import torch.nn.functional as F

from tests import elem_ref as er

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
DTN = {BF: "bf16", F32: "f32"}
K_BOUND = {BF: 4.0, F32: 8.0}               # |got - ref64| <= K x E_r (the issue's constants)
RELU_CAP = {BF: 1e-2, F32: 1e-4}            # largest share of a tensor whose ReLU side may be read from the kernel's output
U_F = 2.0 ** -24

# =================================================================================================================================
# Function branch -> the condition that selects it.  Every case names the branches it takes; branches that another suite
# already compares element-wise are named in ELSEWHERE; a branch that no test compares element-wise would have to be listed in
# OPEN with the reason (empty now; tests/test_functional_reference_cpu.py asserts that the three together cover FORMS exactly).
# =================================================================================================================================
FORMS = collections.OrderedDict([
    ("TransformerBlockFn paired", "paired=True: S = 2 streams, n_segments = 2, the fc layer; 18 parameters per stream"),
    ("TransformerBlockFn self", "paired=False: S = 1, 16 parameters"),
    ("TransformerBlockFn dropout", "training and p_drop > 0: two seeds per stream, masks in both FFN GEMM epilogues, dropout_apply + the "
                                   "dact epilogue's mask in the backward"),
    ("TransformerBlockFn no dropout", "p_eff == 0: seeds (0, 0)"),
    ("LinearFn plain", "pe is None"),
    ("LinearFn pe_drop", "pe given: positional rows added before the dropout (res_row_mod); backward dropout_apply + rowmod_sum"),
    ("LinearFn wT", "bf16, x wants a gradient and N % 8 == 0: the transposed weight image"),
    ("LinearFn kslow", "fp32, or N % 8 != 0: the data gradient through the K-slow forward image"),
    ("LinearFn no bias", "bias is None"),
    ("LinearFn x only", "needs_input_grad = x"),
    ("LinearFn weight only", "needs_input_grad = weight (no dx GEMM, no bias column sums)"),
    ("LinearFn bias only", "needs_input_grad = bias with the weight frozen: ops.colsum"),
    ("LinearFn pe frozen", "pe given and needs_input_grad[3] false: no rowmod_sum"),
    ("AddPeDropoutFn p=0", "p_eff == 0"),
    ("AddPeDropoutFn p>0", "p_eff > 0: mask in the forward, dropout_apply in the backward"),
    ("AddPeDropoutFn pe frozen", "needs_input_grad[1] false"),
    ("LayerNormFn plain", "any dy that is not a stride-0 token expansion (made contiguous)"),
    ("LayerNormFn sliced dy", "plain route with a non-contiguous dy"),
    ("LayerNormFn dy_share", "3-d dy with stride(1) == 0, stride(2) == 1, shape[1] > 1: TokenMeanFn's expansion"),
    ("LayerNormFn L=1", "TokenMeanFn behind it with one token: shape[1] == 1 takes the plain route"),
    ("GuidedCrossAttentionFn need_raw", "raw logits as second output"),
    ("GuidedCrossAttentionFn need_probs", "head-averaged softmax map as second output (dl_attn_probs)"),
    ("GuidedCrossAttentionFn neither", "second output None"),
    ("GuidedCrossAttentionFn key_tail", "key_tail = (rows, weight > 1): log(weight) on the tail keys' logits"),
    ("GuidedCrossAttentionFn key_tail probs", "need_probs with key_tail: the map expanded in ExpandTailFn's order"),
    ("GuidedCrossAttentionFn no biases", "in_b / out_b None"),
    ("GuidedCrossAttentionFn H=1", "one head"),
    ("GuidedCrossAttentionFn H>1", "several heads"),
    ("GuidedCrossAttentionFn wT", "bf16: transposed images for the three data gradients"),
    ("GuidedCrossAttentionFn kslow", "fp32: K-slow forward images"),
    ("TokenGateFn gate_dpre", "H == 8, dd % 8 == 0, dd <= 2048: dl_gate_dpre"),
    ("TokenGateFn padded image", "bf16, H != 8, H <= 64: zero-padded 64-deep GEMM with the padded W2^T image"),
    ("TokenGateFn kslow", "fp32, H != 8: K-slow GEMM with the dact epilogue"),
    ("TokenGateFn padded H", "H no whole 16-byte chunk (H % 8 in bf16, H % 4 in fp32): dlogits zero-padded for lin2's weight gradient"),
    ("TokenGateFn residual", "add_residual=True"),
    ("TokenGateFn no residual", "add_residual=False"),
    ("CastFn contiguous", "_cast_keep_layout: x.is_contiguous()"),
    ("CastFn permuted-dense", "_cast_keep_layout: a permutation of a contiguous tensor keeps its strides"),
    ("CastFn non-dense", "_cast_keep_layout: anything else is made contiguous"),
    ("DenseFn weight_t square", "weight_t=True, 128 x 128: dw[:N, :K].t()"),
    ("DenseFn weight_t", "weight_t=True, K != N"),
    ("DenseFn padded K", "x wider than in_features (641 -> 648)"),
    ("DenseFn padded N", "out_features % 8 != 0: padded weight image, padded bias, zero output columns"),
    ("DenseFn direct bias", "N % 8 == 0 and an fp32 bias: read in place"),
    ("DenseFn residual", "residual given: dres = dy"),
    ("DenseFn act False", "no activation"),
    ("DenseFn act gelu", "act=True: pre-activation saved (torch.empty `pre`), dl_gelu_bwd"),
    ("DenseFn act relu", "act='relu': the mask read off the output"),
    ("DenseFn x only", "needs_input_grad = x"),
    ("DenseFn weight only", "needs_input_grad = weight"),
    ("DenseFn bias only", "needs_input_grad = bias with the weight frozen: ops.colsum"),
    ("DenseFn wT", "bf16 and x wants a gradient"),
    ("DenseFn kslow", "fp32"),
    ("Concat2Fn", "always"),
    ("TokenMeanFn", "always"),
    ("ExpandTailFn", "always"),
    ("SitePoolFn", "always (bf16: the kernels take no fp32)"),
    ("FillPoolFn", "x wants a gradient"),
    ("GraphAggregateFn n<=128", "the MFMA kernel; backward = the transpose launch"),
    ("GraphAggregateFn n>128", "the vector-ALU kernel; backward = the transpose launch"),
    ("EmbeddingFn padded", "D % 8 != 0: dy copied into a zero-padded buffer"),
    ("EmbeddingFn direct", "D % 8 == 0, contiguous dy of the compute dtype"),
    ("EmbeddingFn non-contiguous dy", "dy sliced out of a wider buffer"),
    ("EmbeddingFn padding_idx", "padding_idx given: that row of dw zeroed"),
    ("EmbedPadFn", "always; halo rows of dy are ignored"),
    ("EmbedRowsFn", "always; rows with src < 0 are ignored"),
    ("ExpandRowsFn", "always"),
    ("SitePoolRowsFn", "always"),
    ("ProteinCNNFn training", "training=True: batch statistics, bn_bwd_reduce + bn_bwd_apply"),
    ("ProteinCNNFn plain", "rw None, no pooling, raw_dx False: the body rows as a view, dx copied into a zeroed buffer"),
    ("ProteinCNNFn pooled", "pool_site_len > 0 (bf16): cnn_sitepool_fwd / _bwd on the padded buffer"),
    ("ProteinCNNFn raw_dx", "raw_dx=True behind EmbedPadFn: dx with its halo rows as they are, the unwritten ones zeroed"),
    ("ProteinCNNFn compact", "rw from a ProteinPlan between EmbedRowsFn and ExpandRowsFn / SitePoolRowsFn"),
    ("ProteinCNNFn eval", "training=False: running statistics, bn_eval_bwd with the sums"),
    ("ProteinCNNFn eval frozen", "training=False and no BatchNorm parameter wants a gradient: bn_eval_bwd without the sums"),
    ("ProteinCNNFn no input gradient", "needs_input_grad[0] false"),
    ("BatchNormRowsFn train", "run_mlp without tail, training: batch statistics; relu fused behind the first BatchNorm, not behind the last"),
    ("BatchNormRowsFn eval", "run_mlp in eval mode (with or without tail: eval is row-wise): bn_eval_bwd with the sums"),
    ("BatchNormRowsFn eval frozen", "eval mode and no BatchNorm parameter wants a gradient: bn_eval_bwd without the sums"),
    ("BatchNormWeightedTailFn", "run_mlp with tail = (LP, lead, w) in training: weighted statistics, bn_tail_fix"),
    ("run_mlp", "Linear -> BatchNorm1d -> ReLU -> Linear -> BatchNorm1d: DenseFn's padded output sliced to num_features, the fusion, the tail dispatch"),
    ("CosRowLossFn", "always"), ("CrossEntropyRowsFn", "always"), ("NTXentFn", "world == 1"), ("TripletSigCosFn", "always"),
])

ELSEWHERE = {
    "CosRowLossFn": ["tests.test_loss_paths_gpu::test_cos_rowloss_fn_with_a_row_gradient_against_fp64"],
    "CrossEntropyRowsFn": ["tests.test_loss_paths_gpu::test_ce_rows_form_against_fp64"],
    "NTXentFn": ["tests.test_loss_paths_gpu::test_ntxent_form_against_fp64"],
    "TripletSigCosFn": ["tests.test_loss_paths_gpu::test_triplet_sigcos_against_fp64"],
}

OPEN = collections.OrderedDict()


# =================================================================================================================================
# seeds and masks
# =================================================================================================================================
def seeds(seed0, n):
    """The first n values ops.next_seed() returns after ops.manual_seed(seed0): a CPU torch.Generator, randint(0, 2^62)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed0))
    return [int(torch.randint(0, 2 ** 62, (1,), generator=g).item()) for _ in range(n)]


def drop_mask(seed, rows, cols, p):
    """Multiplicative fp64 mask of one dropout site over a logical [rows][cols] tensor: 0 or fl32(1 / (1 - p))."""
    return torch.from_numpy(er.keep_mask(seed, rows, cols, er.dropout_thr16(p))).double() * er.inv_keep(p)


class Ctx:
    """One evaluation of a formulation at dtype dt.  masks: ReLU open sets decided by an earlier (fp64) evaluation, which the
    plain evaluation reuses; kernel: name -> bool tensor, the kernel's own choice (y > 0), taken where the reference's
    pre-activation lies within `tol` of zero."""

    def __init__(self, dt, masks=None, kernel=None):
        self.dt, self.masks, self.kernel = dt, masks, kernel or {}
        self.open, self.share, self.keep = {}, {}, {}

    def drop(self, x, mask):
        wide = F32 if self.dt == BF else self.dt            # the fp32 scale is applied before the store rounding
        return (x.to(wide) * mask.to(wide)).to(self.dt)

    def relu(self, name, pre, tol):
        if self.masks is not None:
            op = self.masks[name]
        else:
            op = pre.detach() > 0
            amb = pre.detach().abs() <= tol
            self.share[name] = float(amb.double().mean())
            if name in self.kernel:
                op = torch.where(amb, self.kernel[name], op)
            self.open[name] = op
        return pre * op.to(pre.dtype)


# =================================================================================================================================
# cases
# =================================================================================================================================
Case = collections.namedtuple("Case", "name kind dt forms cfg")
SEED0 = 0x5EED5


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31))


class Data:
    """leaf: name -> (CPU tensor, role, wants a gradient); role 'act' (compute dtype as stored), 'w' (fp32 master that the
    Function reads through lowp: rounded to the compute dtype), 'f32' (fp32 parameter read as it is), 'int' (index table).
    dy: output name -> (upstream gradient in the output's dtype, layout of the device copy: 'c' contiguous, 'slice' the leading
    columns of a wider buffer, 'perm' a transpose(0, 1) view, 'expand' produced by the Function chained behind)."""

    def __init__(self):
        self.leaf, self.dy = collections.OrderedDict(), collections.OrderedDict()

    def add(self, name, t, role, grad=True):
        self.leaf[name] = (t, role, grad and role != "int")

    def up(self, name, t, layout="c"):
        self.dy[name] = (t, layout)


def _rn(g, shape, dt, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dt)


def _lin_params(d, g, prefix, n_out, n_in, bias=True, grad=True):
    d.add(prefix + ".w", _rn(g, (n_out, n_in), F32, n_in ** -0.5), "w", grad)
    if bias:
        d.add(prefix + ".b", _rn(g, (n_out,), F32, 0.1), "f32", grad)


def _ln_params(d, g, prefix, n):
    d.add(prefix + ".w", 1.0 + _rn(g, (n,), F32, 0.1), "f32")
    d.add(prefix + ".b", _rn(g, (n,), F32, 0.1), "f32")


BLOCK_PARAMS = {True: ("ln1", "q", "k", "v", "fc", "out", "ln2", "fc1", "fc2"), False: ("ln1", "q", "k", "v", "out", "ln2", "fc1", "fc2")}


def block_param_names(paired, s):
    return ["s%d.%s.%s" % (s, p, wb) for p in BLOCK_PARAMS[paired] for wb in ("w", "b")]


def build(c):
    g, d, k, dt = _gen(c.name + str(c.cfg.get("salt", ""))), Data(), c.cfg, c.dt     # salt: another draw of the same case
    if c.kind == "block":
        S, B, L, dm = (2 if k["paired"] else 1), k["B"], k["L"], k["d"]
        d.add("x", _rn(g, (S, B, L, dm), dt), "act")
        for s in range(S):
            for p in BLOCK_PARAMS[k["paired"]]:
                if p.startswith("ln"):
                    _ln_params(d, g, "s%d.%s" % (s, p), dm)
                else:
                    n_out, n_in = {"fc": (dm, 2 * dm), "fc1": (4 * dm, dm), "fc2": (dm, 4 * dm)}.get(p, (dm, dm))
                    _lin_params(d, g, "s%d.%s" % (s, p), n_out, n_in)
        d.up("y", _rn(g, (S, B, L, dm), dt), k.get("dy", "c"))
    elif c.kind == "linear":
        B, L, K, N = k["B"], k["L"], k["K"], k["N"]
        want = k.get("want", ("x", "weight", "bias", "pe"))
        d.add("x", _rn(g, (B, L, K), dt), "act", "x" in want)
        d.add("weight", _rn(g, (N, K), F32, K ** -0.5), "w", "weight" in want)
        if k.get("bias", True):
            d.add("bias", _rn(g, (N,), F32, 0.1), "f32", "bias" in want)
        if k.get("pe"):
            d.add("pe", _rn(g, (1, L, N), F32, 0.5), "w", "pe" in want)
        d.up("y", _rn(g, (B, L, N), dt), k.get("dy", "c"))
    elif c.kind == "addpe":
        B, L, D = k["B"], k["L"], k["D"]
        d.add("x", _rn(g, (B, L, D), dt), "act")
        d.add("pe", _rn(g, (1, L, D), F32, 0.5), "w", k.get("pe_grad", True))
        d.up("y", _rn(g, (B, L, D), dt), k.get("dy", "c"))
    elif c.kind == "layernorm":
        B, L, D = k["B"], k["L"], k["D"]
        d.add("x", _rn(g, (B, L, D), dt) + 0.5, "act")
        _ln_params(d, g, "ln", D)
        if k["mode"] in ("mean", "L1"):
            d.up("m", _rn(g, (B, D), F32), "c")
        else:
            d.up("y", _rn(g, (B, L, D), dt), "slice" if k["mode"] == "sliced" else "c")
    elif c.kind == "pgca":
        B, Lq, Lk, E = k["B"], k["Lq"], k["Lk"], k["E"]
        d.add("q", _rn(g, (B, Lq, E), dt), "act")
        d.add("k", _rn(g, (B, Lk, E), dt), "act")
        d.add("in_w", _rn(g, (3 * E, E), F32, 1.5 * E ** -0.5), "w")
        if k.get("biases", True):
            d.add("in_b", _rn(g, (3 * E,), F32, 0.1), "f32")
        d.add("out_w", _rn(g, (E, E), F32, E ** -0.5), "w")
        if k.get("biases", True):
            d.add("out_b", _rn(g, (E,), F32, 0.1), "f32")
        d.up("y", _rn(g, (Lq, B, E), dt), k.get("dy", "perm"))
    elif c.kind == "gate":
        B, L, D, H, dd = k["B"], k["L"], k["D"], k["H"], k["dd"]
        d.add("v", _rn(g, (B, L, D), dt), "act")
        _lin_params(d, g, "lin1", dd, D)
        _lin_params(d, g, "lin2", H, dd)
        d.up("y", _rn(g, (B, L, D), dt), k.get("dy", "c"))
    elif c.kind == "dense":
        B, L, K, Kp, N = k["B"], k["L"], k["K"], k["Kp"], k["N"]
        Np = (N + 7) // 8 * 8
        want = k.get("want", ("x", "weight", "bias", "residual"))
        x = _rn(g, (B, L, Kp), dt)
        x[..., K:] = 0
        d.add("x", x, "act", "x" in want)
        d.add("weight", _rn(g, (K, N) if k.get("weight_t") else (N, K), F32, K ** -0.5), "w", "weight" in want)
        if k.get("bias", True):
            d.add("bias", _rn(g, (N,), F32, 0.1), "f32", "bias" in want)
        if k.get("residual"):
            d.add("residual", _rn(g, (B, L, Np), dt), "act", "residual" in want)
        d.up("y", _rn(g, (B, L, Np), dt), k.get("dy", "c"))
    elif c.kind == "concat2":
        d.add("a", _rn(g, (k["B"], k["L"], k["wa"]), dt), "act")
        d.add("b", _rn(g, (k["B"], k["L"], k["wb"]), dt), "act")
        d.up("y", _rn(g, (k["B"], k["L"], k["wa"] + k["wb"]), dt), k.get("dy", "c"))
    elif c.kind == "tokenmean":
        d.add("x", _rn(g, (k["B"], k["L"], k["C"]), dt), "act")
        d.up("y", _rn(g, (k["B"], k["C"]), F32), k.get("dy", "c"))
    elif c.kind == "expandtail":
        B, lead, tail, w, C = k["B"], k["lead"], k["tail"], k["w"], k["C"]
        d.add("x", _rn(g, (B, lead + tail, C), dt), "act")
        d.up("y", _rn(g, (B, lead + w * tail, C), dt), k.get("dy", "c"))
    elif c.kind == "sitepool":
        B, L, C, S = k["B"], k["L"], k["C"], k["site_len"]
        d.add("x", _rn(g, (B, L, C), dt), "act")
        d.up("y", _rn(g, (B, L // S, C), dt), k.get("dy", "c"))
    elif c.kind == "fillpool":
        B, S, Fw, sl = k["B"], k["S"], k["F"], k["site_len"]
        x = _rn(g, (B, S, Fw), dt)
        x[:, -3:] = 0                                    # whole rows of zeros: the fill bit is 1 there
        d.add("x", x, "act")
        d.up("pooled", _rn(g, (B, S // sl, (Fw + 1 + 7) // 8 * 8), k["out_dt"]), k.get("dy", "c"))
    elif c.kind == "graphagg":
        B, n, N = k["B"], k["n"], k["N"]
        adj = (torch.rand((B, n, n), generator=g) < 0.15).float()
        adj = ((adj + adj.transpose(1, 2) + 2 * torch.eye(n)) > 0).float() + torch.eye(n)
        d.add("ahat", er.norm_adjacency(adj)[0].to(dt), "act", False)
        d.add("feat", _rn(g, (B, N, 128), dt), "act")
        d.up("y", _rn(g, (B, N, 128), dt), k.get("dy", "c"))
    elif c.kind == "embedding":
        V, D, B, L = k["V"], k["D"], k["B"], k["L"]
        ids = torch.randint(0, V, (B, L), generator=g)
        ids[0, :5] = 0
        ids[1, -4:] = 3
        d.add("ids", ids, "int")
        d.add("weight", _rn(g, (V, D), k["wdt"]), "act")
        d.up("y", _rn(g, (B, L, D), k["wdt"]), k.get("dy", "c"))
    elif c.kind == "embedpad":
        V, D, B, L = k["V"], k["D"], k["B"], k["L"]
        ids = torch.randint(0, V, (B, L), generator=g)
        ids[0, -6:] = 0
        d.add("ids", ids, "int")
        d.add("fill", (ids == 0).to(dt), "act", False)
        d.add("weight", _rn(g, (V, D), dt), "act")
        dy = _rn(g, (B, L + 8, D + 1), dt)
        dy[:, :4] = 1e30                                 # the halo rows: NaN-free junk that must not reach dw
        dy[:, -4:] = -1e30
        d.up("y", dy, k.get("dy", "c"))
    elif c.kind == "mlp":
        M, K, N1, N2 = k["B"] * k["LP"], k["K"], k["N1"], k["N2"]
        d.add("x", _rn(g, (M, K), dt), "act")
        _lin_params(d, g, "l0", N1, K)
        _lin_params(d, g, "l1", N2, N1, bias=False)
        for i, n in enumerate((N1, N2)):
            d.add("bn%d.w" % i, 1.0 + _rn(g, (n,), F32, 0.1), "f32", not k.get("frozen"))
            d.add("bn%d.b" % i, _rn(g, (n,), F32, 0.3), "f32", not k.get("frozen"))
            d.add("bn%d.rm" % i, _rn(g, (n,), F32, 0.2), "f32", False)
            d.add("bn%d.rv" % i, 0.5 + torch.rand((n,), generator=g), "f32", False)
        d.up("y", _rn(g, (M, N2), dt), k.get("dy", "c"))
    elif c.kind in ("expandrows", "sitepoolrows"):
        from druglamp_amd.protein_plan import ProteinPlan
        plan = ProteinPlan(k["lengths"], k["S"], bucket=8)
        B, S, C = len(k["lengths"]), k["S"], k["C"]
        d.add("row_of", torch.from_numpy(plan.row_of), "int")
        d.add("rep", torch.from_numpy(plan.rep), "int")
        d.add("z", _rn(g, (plan.rows, C), dt), "act")
        d.up("y", _rn(g, (B * S, C) if c.kind == "expandrows" else (B, S // k["site_len"], C), dt), k.get("dy", "c"))
    elif c.kind == "embedrows":
        from druglamp_amd.protein_plan import ProteinPlan
        B, S, D = k["B"], k["S"], k["D"]
        ids = torch.zeros((B, S), dtype=torch.int64)
        for b, L in enumerate(k["lengths"]):
            one = torch.cat((torch.zeros(1, dtype=torch.int64), torch.randint(1, 27, (L,), generator=g), torch.zeros(1, dtype=torch.int64)))
            ids[b, :(S // (L + 2)) * (L + 2)] = one.repeat(S // (L + 2))
        src = torch.from_numpy(ProteinPlan(k["lengths"], S, bucket=8).src)
        d.add("ids", ids, "int")
        d.add("src", src, "int")
        d.add("fill", (ids == 0).to(dt), "act", False)
        d.add("emb", _rn(g, (27, D), dt), "act")
        dy = _rn(g, (src.numel(), D + 1), dt)
        dy[src < 0] = 1e30                               # halo and bucket-padding rows: NaN-free junk that must not reach dw
        dy[(src < 0) & (torch.arange(src.numel()) % 2 == 1)] = -1e30
        d.up("y", dy, k.get("dy", "c"))
    elif c.kind == "cnn":
        B, S, C, lay = k["B"], k["S"], k["C"], k["layout"]
        if lay in ("plain", "pooled"):
            d.add("x", _rn(g, (B, S, C), dt), "act", k.get("want_x", True))
        else:
            # tiled residue codes: period P = L + 2 with the CLS / SEP slots coded 0, zeros behind the last whole period
            ids = torch.zeros((B, S), dtype=torch.int64)
            for b, L in enumerate(k["lengths"][:B]):
                P = L + 2
                one = torch.cat((torch.zeros(1, dtype=torch.int64), torch.randint(1, 27, (L,), generator=g), torch.zeros(1, dtype=torch.int64)))
                ids[b, :(S // P) * P] = one.repeat(S // P)
            d.add("ids", ids, "int")
            d.add("fill", (ids == 0).to(dt), "act", False)
            d.add("emb", _rn(g, (27, C - 1), dt), "act")
        for i, ks in enumerate(CNN_KERNELS):
            # unit-variance pre-activations; behind the first layer they are centred at +1.2 sigma (an eighth of the elements stays
            # closed), which halves the density at zero: at 5 sigma of the propagated bf16 rounding (cnn_relu_tol) the share of
            # a layer that is the kernel's to choose would otherwise pass the 1 % cap at the third layer
            d.add("conv%d.w" % i, _rn(g, (C, C, ks), F32, (ks * C) ** -0.5), "w")
            d.add("conv%d.b" % i, _rn(g, (C,), F32, 0.2) + (1.2 if i else 0.0), "f32")
            d.add("bn%d.w" % i, 1.0 + _rn(g, (C,), F32, 0.1), "f32", not k.get("frozen"))
            d.add("bn%d.b" % i, _rn(g, (C,), F32, 0.1), "f32", not k.get("frozen"))
            d.add("bn%d.rm" % i, 0.3 + _rn(g, (C,), F32, 0.1), "f32", False)
            d.add("bn%d.rv" % i, 0.5 + torch.rand((C,), generator=g), "f32", False)
        sl = k.get("site_len", 1)
        shape = {"plain": (B, S, C), "raw_dx": (B, S, C), "compact": (B * S, C)}.get(lay, (B, S // sl, C))
        d.up("y", _rn(g, shape, dt), k.get("dy", "c"))
    else:
        raise KeyError(c.kind)
    return d


# =================================================================================================================================
# the formulations (run at fp64 = reference, at the compute dtype = plain)
# =================================================================================================================================
def _heads(x, H):
    B, L, D = x.shape
    return x.view(B, L, H, D // H).permute(0, 2, 1, 3)


def _sdpa(q, k, v):
    a = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(q.shape[-1]), dim=-1)
    o = torch.matmul(a, v).permute(0, 2, 1, 3)
    return o.reshape(o.shape[0], o.shape[1], -1)


def ref_block(c, T, ctx):
    """block.py:33-62 as the oracle's pmma_forward states it, one block: stream s attends over its own keys / values with its
    own queries and (paired) with the other stream's queries; fc over the concatenation; out; residual; LN; Mlp with the two
    dropout sites; residual."""
    k = c.cfg
    paired, H, p = k["paired"], k["H"], k.get("p", 0.0)
    S, B, L, d = T["x"].shape
    sd = seeds(SEED0, 2 * S) if p > 0 else None
    P = lambda s, n: T["s%d.%s" % (s, n)]                                                  # noqa: E731
    lin = lambda s, n, x: F.linear(x, P(s, n + ".w"), P(s, n + ".b"))                      # noqa: E731
    xn = [F.layer_norm(T["x"][s], (d,), P(s, "ln1.w"), P(s, "ln1.b"), 1e-6) for s in range(S)]
    q, kk, v = ([_heads(lin(s, n, xn[s]), H) for s in range(S)] for n in ("q", "k", "v"))
    ys = []
    for s in range(S):
        a = _sdpa(q[s], kk[s], v[s])
        if paired:
            a = lin(s, "fc", torch.cat((a, _sdpa(q[1 - s], kk[s], v[s])), dim=-1))
        x1 = lin(s, "out", a) + T["x"][s]
        h = F.gelu(lin(s, "fc1", F.layer_norm(x1, (d,), P(s, "ln2.w"), P(s, "ln2.b"), 1e-6)))
        if p > 0:
            h = ctx.drop(h, drop_mask(sd[2 * s], B * L, 4 * d, p).reshape(B, L, 4 * d))
        y = lin(s, "fc2", h)
        if p > 0:
            y = ctx.drop(y, drop_mask(sd[2 * s + 1], B * L, d, p).reshape(B, L, d))
        ys.append(y + x1)
    return collections.OrderedDict(y=torch.stack(ys))


def ref_linear(c, T, ctx):
    k = c.cfg
    y = F.linear(T["x"], T["weight"], T.get("bias"))
    if "pe" in T:
        y = y + T["pe"]                                   # (1, L, N) over (B, L, N): row r takes pe[r % L]
        if k.get("p", 0.0) > 0:
            y = ctx.drop(y, drop_mask(seeds(SEED0, 1)[0], k["B"] * k["L"], k["N"], k["p"]).reshape(y.shape))
    return collections.OrderedDict(y=y)


def ref_addpe(c, T, ctx):
    k = c.cfg
    y = T["x"] + T["pe"]
    if k.get("p", 0.0) > 0:
        y = ctx.drop(y, drop_mask(seeds(SEED0, 1)[0], k["B"] * k["L"], k["D"], k["p"]).reshape(y.shape))
    return collections.OrderedDict(y=y)


def ref_layernorm(c, T, ctx):
    y = F.layer_norm(T["x"], (c.cfg["D"],), T["ln.w"], T["ln.b"], 1e-5)
    out = collections.OrderedDict(y=y)
    if c.cfg["mode"] in ("mean", "L1"):
        out["m"] = y.mean(dim=1)
    return out


def ref_pgca(c, T, ctx):
    """oracle pgca_forward on seq-first views; key_tail by the expansion of ExpandTailFn (tail rows repeated `weight` times)."""
    k = c.cfg
    H, E, B, Lq = k["H"], k["E"], k["B"], k["Lq"]
    query, key = T["q"].permute(1, 0, 2), T["k"].permute(1, 0, 2)
    if k.get("tail"):
        rows, w = k["tail"]
        lead = key.shape[0] - rows
        key = torch.cat((key[:lead], key[lead:].repeat(w, 1, 1)), dim=0)
    Lk, hd = key.shape[0], E // H
    W, b = T["in_w"], T.get("in_b")
    qp = F.linear(query, W[:E], None if b is None else b[:E]) * (float(hd) ** -0.5)
    kv = F.linear(key, W[E:], None if b is None else b[E:])
    kp, vp = kv.chunk(2, dim=-1)
    qp = qp.contiguous().view(Lq, B * H, hd).transpose(0, 1)
    kp = kp.contiguous().view(Lk, B * H, hd).transpose(0, 1)
    vp = vp.contiguous().view(Lk, B * H, hd).transpose(0, 1)
    raw = torch.bmm(qp, kp.transpose(1, 2))
    pr = torch.softmax(raw, dim=-1)
    o = torch.bmm(pr, vp).transpose(0, 1).contiguous().view(Lq, B, E)
    out = collections.OrderedDict(y=F.linear(o, T["out_w"], T.get("out_b")))
    if k["second"] == "raw":
        out["raw"] = raw.view(B, H, Lq, Lk)
    elif k["second"] == "probs":
        out["probs"] = pr.view(B, H, Lq, Lk).mean(dim=1)
    return out


def ref_gate(c, T, ctx):
    """oracle mhla_forward (+ v): softmax over the tokens, the flat reinterpretation of the contiguous (B, L, D) buffer."""
    k = c.cfg
    v, H = T["v"], k["H"]
    B, L, D = v.shape
    g = F.linear(F.gelu(F.linear(v, T["lin1.w"], T["lin1.b"])), T["lin2.w"], T["lin2.b"])
    g = torch.softmax(g, dim=1).transpose(1, 2).contiguous()
    out = (g.view(B * H, L, 1) * v.contiguous().view(B * H, L, D // H)).view(B, L, D)
    return collections.OrderedDict(y=out + v if k["res"] else out)


def dense_relu_tol(c, T):
    """The rounding of DenseFn's pre-activation itself: an fp32 accumulation of K products and the bias (the GEMM suite's
    (K + 2) u_f of the sum of the absolute terms); the operands are read exactly."""
    k = c.cfg
    W = T["weight"].t() if k.get("weight_t") else T["weight"]
    mag = T["x"][..., :k["K"]].detach().abs().double() @ W.detach().abs().double().t()
    if "bias" in T:
        mag = mag + T["bias"].detach().abs().double()
    return (k["K"] + 2) * U_F * mag


def ref_dense(c, T, ctx):
    k = c.cfg
    K, N = k["K"], k["N"]
    W = T["weight"].t() if k.get("weight_t") else T["weight"]
    pre = F.linear(T["x"][..., :K], W, T.get("bias"))
    if k.get("act") == "relu":
        y = ctx.relu("y", pre, dense_relu_tol(c, T))
    else:
        y = F.gelu(pre) if k.get("act") else pre
    y = F.pad(y, (0, (N + 7) // 8 * 8 - N))
    return collections.OrderedDict(y=y + T["residual"] if "residual" in T else y)


def ref_concat2(c, T, ctx):
    return collections.OrderedDict(y=torch.cat((T["a"], T["b"]), dim=-1))


def ref_tokenmean(c, T, ctx):
    return collections.OrderedDict(y=T["x"].mean(dim=1))


def ref_expandtail(c, T, ctx):
    lead, w = c.cfg["lead"], c.cfg["w"]
    x = T["x"]
    return collections.OrderedDict(y=torch.cat((x[:, :lead], x[:, lead:].repeat(1, w, 1)), dim=1))


def ref_sitepool(c, T, ctx):
    """basic_model.py:179 + DrugLAMP.py:35-37: the (B, C, L) activation viewed as (B, L, C), then the mean over the site_len
    strided groups (oracle protein_cnn's last line and model_forward's pooling)."""
    x, S = T["x"], c.cfg["site_len"]
    B, L, C = x.shape
    v = x.transpose(1, 2).contiguous().reshape(B, L, C)
    return collections.OrderedDict(y=v.view(B, S, L // S, C).mean(dim=1))


def ref_fillpool(c, T, ctx):
    x, sl = T["x"], c.cfg["site_len"]
    B, S, Fw = x.shape
    fill = (x.detach().sum(dim=-1) == 0).to(x.dtype)
    pooled = torch.cat((x, fill.unsqueeze(-1)), dim=-1).view(B, sl, S // sl, Fw + 1).mean(dim=1)
    if x.dtype != F64:
        pooled = pooled.to(c.cfg["out_dt"])                # the plain evaluation stores what the Function stores
    return collections.OrderedDict(fill=fill, pooled=F.pad(pooled, (0, (Fw + 1 + 7) // 8 * 8 - Fw - 1)))


def ref_graphagg(c, T, ctx):
    n = c.cfg["n"]
    f = T["feat"]
    return collections.OrderedDict(y=torch.cat((torch.bmm(T["ahat"], f[:, :n]), f[:, n:]), dim=1))


def ref_embedding(c, T, ctx):
    return collections.OrderedDict(y=F.embedding(T["ids"], T["weight"], padding_idx=c.cfg.get("padding_idx")))


def ref_embedpad(c, T, ctx):
    e = F.embedding(T["ids"], T["weight"], padding_idx=c.cfg.get("padding_idx"))
    return collections.OrderedDict(y=F.pad(torch.cat((e, T["fill"].unsqueeze(-1)), dim=-1), (0, 0, 4, 4)))


CNN_KERNELS = (3, 6, 9)
CNN_EPS = 1e-5


def cnn_relu_tol(i, dt, v, w, var_in):
    """How far the kernel's pre-activation of layer i can lie from the reference's, so that the side of the ReLU is the
    kernel's to choose.  K = k C terms per element, l2 = sqrt(sum (w z)^2).
    The accumulation itself is fp32 in both dtypes (bf16 products are exact in fp32): K roundings, independent, a random
    walk with sigma <= sqrt(K) u_f l2; 8 sigma, and 16 sqrt(K) u_f l2 behind the first layer, whose fp32 inputs carry a few
    u_f each.  In bf16 the layers behind the first read what the kernels STORED: y = relu(pre) rounded to bf16, then
    z = a (y - mean) + beta (a = gamma rstd) rounded to bf16, each store a relative error of at most 2^-9, uniform: variance
    (2^-9 v)^2 / 3 per stored value (an overestimate: the mean over a binade is about half of it).  To first order
        var(y_k - y_ref) = [open] var(pre_k - pre_ref) + (2^-9 y)^2 / 3,     var(z_k - z_ref) = a^2 var(y) + (2^-9 z)^2 / 3,
        var(pre_k - pre_ref) of the next layer = sum w^2 var(z)   (independent terms; batch statistics average the errors out),
    carried from layer to layer in `var_in`; the tolerance is 5 sigma.  Measured on an MI355X with the one-layer model at 6.9
    sigma of the z rounding alone: no side disagreed beyond it at the second layer, 21 elements in four cases at the third, up to
    1.41 x beyond, which is what the propagated variance of the second layer's own disagreement accounts for.  The worst-case
    sums (K u_f sum |w z|, 2^-9 sum |w z|) would hand several per cent of a layer to the kernel."""
    K = w.shape[1] * w.shape[2]
    w2 = w.detach().double() ** 2
    tol = (8 if i == 0 else 16) * math.sqrt(K) * U_F * F.conv1d(v.detach().double() ** 2, w2, None, padding="same").sqrt()
    sig2 = F.conv1d(var_in, w2, None, padding="same") if dt == BF else torch.zeros_like(tol)
    return tol + 5 * sig2.sqrt(), sig2


def ref_cnn(c, T, ctx):
    """oracle protein_cnn (basic_model.py:172-180): embedding + fill bit, three Conv1d('same') -> ReLU -> BatchNorm1d on the
    whole (B, S) batch, every position computed; the outputs of the compact layouts are those rows, their gradients the sums."""
    k = c.cfg
    B, S, C, lay, training = k["B"], k["S"], k["C"], k["layout"], k["training"]
    if "x" in T:
        v = T["x"]
    else:
        v = torch.cat((F.embedding(T["ids"], T["emb"], padding_idx=0), T["fill"].unsqueeze(-1)), dim=-1)
    v = v.transpose(1, 2)
    out = collections.OrderedDict()
    var_in = torch.zeros(v.shape, dtype=F64)
    for i in range(3):
        w, b = T["conv%d.w" % i], T["conv%d.b" % i]
        pre = F.conv1d(v, w, b, padding="same")
        tol, sig2 = cnn_relu_tol(i, c.dt, v, w, var_in) if ctx.masks is None else (None, None)
        if ctx.masks is None:                                 # for extra_bound: the two factors of the weight gradient's terms
            pre.retain_grad()
            ctx.keep["pre%d" % i], ctx.keep["in%d" % i] = pre, v.detach()
        y = ctx.relu("y%d" % i, pre, tol)
        rm, rv = T["bn%d.rm" % i].detach().clone(), T["bn%d.rv" % i].detach().clone()
        mean = y.detach().mean(dim=(0, 2)) if training else rm
        var = y.detach().var(dim=(0, 2), unbiased=False) if training else rv
        out["mean%d" % i], out["var%d" % i] = mean, var
        if ctx.masks is None:
            ctx.keep["y4sum%d" % i] = (y.detach().double() ** 4).sum(dim=(0, 2))
        v = F.batch_norm(y, rm, rv, T["bn%d.w" % i], T["bn%d.b" % i], training, 0.1, CNN_EPS)
        if ctx.masks is None and c.dt == BF:
            a2 = (T["bn%d.w" % i].detach().double() ** 2 / (var.double() + CNN_EPS))[None, :, None]
            var_y = sig2 * (y.detach() > 0) + (2.0 ** -9 * y.detach().double()) ** 2 / 3
            var_in = a2 * var_y + (2.0 ** -9 * v.detach().double()) ** 2 / 3
    z = v.transpose(1, 2)                                     # (B, S, C) channel-last
    if lay in ("pooled", "compact_pool"):
        sl = k["site_len"]
        z = v.contiguous().reshape(B, S, C).view(B, sl, S // sl, C).mean(dim=1)      # the (B, C, S) buffer viewed as (B, S, C), pooled
    elif lay == "compact":
        z = z.reshape(B * S, C)
    res = collections.OrderedDict(y=z)
    res.update(out)
    return res


def mlp_rows(c):
    """(idx, mult): the rows of the expanded matrix as indices into the compact one, and every compact row's multiplicity."""
    k = c.cfg
    B, LP = k["B"], k["LP"]
    if not k.get("tail"):
        return torch.arange(B * LP), torch.ones(B * LP, dtype=F64)
    _, lead, w = k["tail"]
    one = torch.cat((torch.arange(lead), torch.arange(lead, LP).repeat(w)))
    idx = torch.cat([one + b * LP for b in range(B)])
    mult = torch.ones(LP, dtype=F64)
    mult[lead:] = w
    return idx, mult.repeat(B)


def ref_mlp(c, T, ctx):
    """run_mlp's contract on the EXPANDED rows (a tail row repeated w times): Linear -> BatchNorm1d -> ReLU -> Linear ->
    BatchNorm1d as torch.nn computes them; the output of a compact row is that of its copies (their mean, so that the upstream
    gradient of a compact row is shared out over its copies and its input gradient is the sum over them).
    ReLU: the pre-activation is z = a (h - mean) + beta, a = gamma rstd, h the stored Linear output.  The kernels' h differs
    from the reference's by the fp32 accumulation (random walk, 16 sqrt(K) u_f l2 as in cnn_relu_tol) and in bf16 by its store
    rounding, sigma = 2^-9 |h| / sqrt(3), 5 sigma taken; the BatchNorm itself adds a few u_f of its terms."""
    k = c.cfg
    training = k["training"]
    idx, mult = mlp_rows(c)
    xe = T["x"][idx]
    h = F.linear(xe, T["l0.w"], T["l0.b"])
    rm, rv = T["bn0.rm"].detach().clone(), T["bn0.rv"].detach().clone()
    z = F.batch_norm(h, rm, rv, T["bn0.w"], T["bn0.b"], training, 0.1, CNN_EPS)
    tol = None
    if ctx.masks is None:
        hd = h.detach().double()
        mean, var = (hd.mean(0), hd.var(0, unbiased=False)) if training else (T["bn0.rm"].detach().double(), T["bn0.rv"].detach().double())
        a = T["bn0.w"].detach().double().abs() / torch.sqrt(var + CNN_EPS)
        l2 = ((xe.detach().double() ** 2) @ (T["l0.w"].detach().double() ** 2).t()).sqrt()
        tol = a * 16 * math.sqrt(k["K"]) * U_F * l2 + 8 * U_F * (a * (hd.abs() + mean.abs()) + T["bn0.b"].detach().double().abs())
        if c.dt == BF:
            tol = tol + 5 * a * 2.0 ** -9 * hd.abs() / math.sqrt(3)
        if "y0" in ctx.kernel and ctx.kernel["y0"].shape[0] != idx.numel():
            ctx.kernel["y0"] = ctx.kernel["y0"][idx]
    y = ctx.relu("y0", z, tol)
    h2 = F.linear(y, T["l1.w"])
    oe = F.batch_norm(h2, T["bn1.rm"].detach().clone(), T["bn1.rv"].detach().clone(), T["bn1.w"], T["bn1.b"], training, 0.1, CNN_EPS)
    wide = F64 if oe.dtype == F64 else F32
    out = torch.zeros((mult.numel(), oe.shape[1]), dtype=wide).index_add(0, idx, oe.to(wide)) / mult.to(wide)[:, None]
    return collections.OrderedDict(y=out.to(oe.dtype))


def ref_expandrows(c, T, ctx):
    """out[i] = z[row_of[i]]; a compact row's gradient is the sum over the positions it stands for."""
    return collections.OrderedDict(y=T["z"][T["row_of"].long()])


def ref_sitepoolrows(c, T, ctx):
    k = c.cfg
    B, S, C, sl = len(k["lengths"]), k["S"], k["C"], k["site_len"]
    v = T["z"][T["row_of"].long()].view(B, S, C).transpose(1, 2).contiguous().reshape(B, S, C)
    return collections.OrderedDict(y=v.view(B, sl, S // sl, C).mean(dim=1))


def ref_embedrows(c, T, ctx):
    """out[r] = [emb[ids[src[r]]] | fill[src[r]]] (ids, fill flat), zero rows where src[r] < 0."""
    src = T["src"].long()
    s0 = src.clamp_min(0)
    e = F.embedding(T["ids"].reshape(-1)[s0], T["emb"], padding_idx=c.cfg.get("padding_idx"))
    rows = torch.cat((e, T["fill"].reshape(-1)[s0].unsqueeze(-1)), dim=-1)
    return collections.OrderedDict(y=rows * (src >= 0).unsqueeze(-1).to(rows.dtype))


REFS = {"mlp": ref_mlp, "expandrows": ref_expandrows, "sitepoolrows": ref_sitepoolrows, "embedrows": ref_embedrows, "cnn": ref_cnn, "block": ref_block, "linear": ref_linear, "addpe": ref_addpe, "layernorm": ref_layernorm, "pgca": ref_pgca, "gate": ref_gate,
        "dense": ref_dense, "concat2": ref_concat2, "tokenmean": ref_tokenmean, "expandtail": ref_expandtail, "sitepool": ref_sitepool,
        "fillpool": ref_fillpool, "graphagg": ref_graphagg, "embedding": ref_embedding, "embedpad": ref_embedpad}

# results that are pure data movement: compared bit for bit (every value of the compute dtype is exact in fp64)
EXACT = {"concat2": ("out:y", "grad:a", "grad:b"), "expandtail": ("out:y",), "embedding": ("out:y",), "embedpad": ("out:y",), "embedrows": ("out:y",), "expandrows": ("out:y",),
         "fillpool": ("out:fill",)}
EXACT_CNN_EVAL = tuple("out:%s%d" % (n, i) for n in ("mean", "var") for i in range(3))       # eval mode hands the running statistics back


def leaves_at(data, dt, cdt):
    T = collections.OrderedDict()
    for name, (t, role, want) in data.leaf.items():
        if role == "int":
            T[name] = t
            continue
        v = t.to(cdt) if role == "w" else t                # lowp: the master rounded to the compute dtype
        T[name] = v.to(dt).detach().clone().requires_grad_(want)
    return T


def evaluate(c, data, dt, masks=None, kernel=None):
    """Outputs ('out:<name>') and gradients of every leaf that wants one ('grad:<name>') of the formulation at dtype dt."""
    ctx = Ctx(dt, masks, kernel)
    T = leaves_at(data, dt, c.dt)
    outs = REFS[c.kind](c, T, ctx)
    names = [n for n in outs if n in data.dy]
    torch.autograd.backward([outs[n] for n in names], [data.dy[n][0].to(outs[n].dtype) for n in names])
    res = collections.OrderedDict(("out:" + n, o.detach()) for n, o in outs.items())
    for name, (t, role, want) in data.leaf.items():
        if want:
            res["grad:" + name] = T[name].grad if T[name].grad is not None else torch.zeros_like(T[name])
    return res, ctx


def reference(c, data, kernel=None):
    """(fp64 reference, plain evaluation at the compute dtype with the reference's ReLU sets, the fp64 Ctx)."""
    ref, ctx = evaluate(c, data, F64, kernel=kernel)
    plain, _ = evaluate(c, data, c.dt, masks=ctx.open)
    return ref, plain, ctx


# =================================================================================================================================
# the bound and the checker
# =================================================================================================================================
def envelope(plain, ref64):
    """E_r = max_i |plain_i - ref64_i| per row (last dimension; a 0-d or 1-d tensor is one row), floored by the median of E_r
    over the tensor's rows, broadcast back to the tensor's shape."""
    e = (plain.double() - ref64).abs()
    rows = e.reshape(-1, e.shape[-1]) if e.dim() >= 1 and e.numel() else e.reshape(1, -1)
    rmax = rows.max(dim=1).values if rows.numel() else rows.sum(1)
    rmax = torch.maximum(rmax, rmax.median()) if rmax.numel() else rmax
    return rmax.reshape(-1, 1).expand(rows.shape).reshape(e.shape)


def extra_bound(c, key, ctx):
    """Terms added to single tensors' bounds (see the header of tests/test_functional_paths_gpu.py for why): None for every
    other tensor.  The model is the accumulation / store model of tests/test_gemm_paths_gpu.py with independent roundings: a sum of
    R fp32 terms t_r is a random walk, sigma <= sqrt(R) u_f l2, l2 = sqrt(sum t_r^2) (as cnn_relu_tol takes it); 8 sigma.
      ProteinCNNFn grad:conv<i>.w   R = B S rows, t = dpre x: 8 sqrt(R) u_f l2.
                                    compact layouts in bf16: a representative row's dpre is rounded to bf16 ONCE and enters the sum
                                    with its multiplicity m (the same input row for every copy), so its store rounding adds up
                                    coherently over m <= S / P periods where the expanded plain evaluation rounds every copy on its
                                    own: sigma <= 2^-9 sqrt(m_max / 3) l2; 5 sigma.
      ProteinCNNFn out:var<i>       (training) the column sum behind E[y^2]: t = y^2 / R: 8 sqrt(R) u_f sqrt(sum y^4) / R."""
    if c.kind != "cnn" or ctx is None:
        return None
    k = c.cfg
    R_ = k["B"] * k["S"]
    if key.startswith("grad:conv") and key.endswith(".w"):
        i = int(key[len("grad:conv")])
        pre, vin = ctx.keep["pre%d" % i], ctx.keep["in%d" % i]
        w0 = torch.zeros(c.cfg["C"], c.cfg["C"], CNN_KERNELS[i], dtype=F64, requires_grad=True)
        S2, = torch.autograd.grad((F.conv1d(vin ** 2, w0, None, padding="same") * pre.grad ** 2).sum(), w0)
        l2 = S2.sqrt()
        e = 8 * math.sqrt(R_) * U_F * l2
        if c.dt == BF and k["layout"].startswith("compact"):
            m_max = max(k["S"] // (L + 2) for L in k["lengths"][:k["B"]])
            e = e + 5 * 2.0 ** -9 * math.sqrt(m_max / 3.0) * l2
        return e
    if key.startswith("out:var") and k["training"]:
        i = int(key[len("out:var")])
        return 8 * math.sqrt(R_) * U_F * ctx.keep["y4sum%d" % i].sqrt() / R_
    return None


def _blog(case, key, dt, ratio):
    path = os.environ.get("DL_FN_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case.name, "kind": case.kind, "tensor": key, "dtype": DTN[dt], "ratio": ratio,
                                "forms": list(case.forms)}) + "\n")


def check_case(c, got, ref, plain, ctx=None):
    """Every output and gradient of `got` (name -> tensor on any device) element by element: bit-exact for the data movers,
    |got - ref64| <= K x E_r otherwise.  Raises AssertionError naming every tensor that misses."""
    assert set(got) == set(ref), "%s: results %s, reference %s" % (c.name, sorted(got), sorted(ref))
    K, bad = K_BOUND[c.dt], []
    for key, r in ref.items():
        g = got[key].detach().cpu()
        if tuple(g.shape) != tuple(r.shape):
            bad.append("%s: shape %s, reference %s" % (key, tuple(g.shape), tuple(r.shape)))
            continue
        g = g.double()
        if not bool(torch.isfinite(g).all()):
            bad.append("%s: %d non-finite elements" % (key, int((~torch.isfinite(g)).sum())))
            continue
        err = (g - r).abs()
        if key in EXACT.get(c.kind, ()) or (c.kind == "cnn" and not c.cfg["training"] and key in EXACT_CNN_EVAL):
            n = int((err != 0).sum())
            _blog(c, key, c.dt, 0.0 if n == 0 else float("inf"))
            if n:
                bad.append("%s: a data mover differs in %d elements (first at flat index %d)" % (key, n, int((err != 0).reshape(-1).nonzero()[0])))
            continue
        bound = K * envelope(plain[key], r)
        extra = extra_bound(c, key, ctx)
        if extra is not None:
            bound = bound + extra
        ratio = float((err / (bound + 1e-300)).max()) if err.numel() else 0.0
        _blog(c, key, c.dt, ratio)
        miss = err > bound
        if bool(miss.any()):
            i = int((err / (bound + 1e-300)).reshape(-1).argmax())
            bad.append("%s: %d of %d elements beyond %g x envelope, worst |err| / bound %.3g at flat index %d (got %.6g, ref %.6g, bound %.3g)"
                       % (key, int(miss.sum()), err.numel(), K, ratio, i, float(g.reshape(-1)[i]), float(r.reshape(-1)[i]),
                          float(bound.reshape(-1)[i])))
    assert not bad, "%s [%s]:\n  " % (c.name, ", ".join(c.forms)) + "\n  ".join(bad)


# =================================================================================================================================
# the case lists
# =================================================================================================================================
def _both(name, kind, forms_of, cfg, dts=(F32, BF)):
    """One case per compute dtype; forms_of(dt) -> the FORMS keys the case takes."""
    return [Case("%s_%s" % (name, DTN[dt]), kind, dt, tuple(forms_of(dt) if callable(forms_of) else forms_of), dict(cfg)) for dt in dts]


def _route(fn, dt, wt_ok=True):
    return "%s %s" % (fn, "wT" if (dt == BF and wt_ok) else "kslow")


CASES = []
# ---- TransformerBlockFn: the attention kernels take head_dim 64 and 128 only, so d = 128 with H = 2 or 1 and d = 256 with H = 4;
#      B L = 3 x 24 = 72 or 2 x 40 = 80 rows (no multiple of 64) ----------------------------------------------------------------
CASES += _both("block_paired", "block", ("TransformerBlockFn paired", "TransformerBlockFn no dropout"), dict(paired=True, B=3, L=24, d=128, H=2))
CASES += _both("block_paired_drop", "block", ("TransformerBlockFn paired", "TransformerBlockFn dropout"),
               dict(paired=True, B=3, L=24, d=128, H=2, p=0.1, dy="perm"))
CASES += _both("block_self", "block", ("TransformerBlockFn self", "TransformerBlockFn no dropout"), dict(paired=False, B=3, L=24, d=128, H=1, dy="slice"))
CASES += _both("block_self_drop", "block", ("TransformerBlockFn self", "TransformerBlockFn dropout"), dict(paired=False, B=2, L=40, d=256, H=4, p=0.1))
# ---- LinearFn ------------------------------------------------------------------------------------------------------------------
CASES += _both("linear_plain", "linear", lambda dt: ("LinearFn plain", _route("LinearFn", dt)), dict(B=3, L=33, K=72, N=64, dy="slice"))
CASES += _both("linear_plain_n36_nobias", "linear", lambda dt: ("LinearFn plain", "LinearFn kslow", "LinearFn no bias"),
               dict(B=3, L=33, K=72, N=36, bias=False))
CASES += [Case("linear_plain_n38_f32", "linear", F32, ("LinearFn plain", "LinearFn kslow"), dict(B=3, L=33, K=72, N=38))]
CASES += _both("linear_pe_drop", "linear", lambda dt: ("LinearFn pe_drop", _route("LinearFn", dt)), dict(B=3, L=24, K=40, N=64, pe=True, p=0.1))
CASES += _both("linear_pe_p0_frozen_pe", "linear", lambda dt: ("LinearFn pe_drop", "LinearFn pe frozen", _route("LinearFn", dt)),
               dict(B=3, L=24, K=40, N=64, pe=True, p=0.0, want=("x", "weight", "bias")))
CASES += _both("linear_x_only", "linear", lambda dt: ("LinearFn plain", "LinearFn x only", _route("LinearFn", dt)), dict(B=3, L=33, K=72, N=64, want=("x",)))
CASES += _both("linear_weight_only", "linear", ("LinearFn plain", "LinearFn weight only"), dict(B=3, L=33, K=72, N=64, want=("weight",)))
CASES += _both("linear_bias_only", "linear", ("LinearFn pe_drop", "LinearFn bias only"), dict(B=3, L=24, K=40, N=64, pe=True, p=0.1, want=("bias", "pe")))
# ---- AddPeDropoutFn ------------------------------------------------------------------------------------------------------------
CASES += _both("addpe_p0", "addpe", ("AddPeDropoutFn p=0",), dict(B=3, L=24, D=72, p=0.0, dy="slice"))
CASES += _both("addpe_drop", "addpe", ("AddPeDropoutFn p>0",), dict(B=3, L=24, D=72, p=0.1))
CASES += _both("addpe_drop_frozen_pe", "addpe", ("AddPeDropoutFn p>0", "AddPeDropoutFn pe frozen"), dict(B=2, L=33, D=64, p=0.1, pe_grad=False))
# ---- LayerNormFn ---------------------------------------------------------------------------------------------------------------
CASES += _both("ln_contig", "layernorm", ("LayerNormFn plain",), dict(B=3, L=33, D=128, mode="contig"))
CASES += _both("ln_sliced_dy", "layernorm", ("LayerNormFn plain", "LayerNormFn sliced dy"), dict(B=3, L=33, D=72, mode="sliced"))
CASES += _both("ln_token_mean", "layernorm", ("LayerNormFn dy_share", "TokenMeanFn"), dict(B=3, L=33, D=128, mode="mean"))
CASES += _both("ln_token_mean_L1", "layernorm", ("LayerNormFn L=1", "TokenMeanFn"), dict(B=5, L=1, D=128, mode="L1"))
# ---- GuidedCrossAttentionFn ----------------------------------------------------------------------------------------------------
CASES += _both("pgca_raw_h1", "pgca", lambda dt: ("GuidedCrossAttentionFn need_raw", "GuidedCrossAttentionFn H=1", _route("GuidedCrossAttentionFn", dt)),
               dict(B=3, Lq=24, Lk=40, E=64, H=1, second="raw"))
CASES += _both("pgca_probs_h4", "pgca", lambda dt: ("GuidedCrossAttentionFn need_probs", "GuidedCrossAttentionFn H>1", _route("GuidedCrossAttentionFn", dt)),
               dict(B=2, Lq=33, Lk=40, E=256, H=4, second="probs", dy="c"))
CASES += _both("pgca_none_nobias_h2", "pgca", lambda dt: ("GuidedCrossAttentionFn neither", "GuidedCrossAttentionFn no biases", "GuidedCrossAttentionFn H>1",
                                                          _route("GuidedCrossAttentionFn", dt)),
               dict(B=3, Lq=24, Lk=33, E=128, H=2, second=None, biases=False))
CASES += _both("pgca_tail_w5", "pgca", lambda dt: ("GuidedCrossAttentionFn key_tail", "GuidedCrossAttentionFn neither", "GuidedCrossAttentionFn H=1",
                                                   _route("GuidedCrossAttentionFn", dt)),
               dict(B=3, Lq=24, Lk=48, E=128, H=1, second=None, tail=(8, 5)))
CASES += _both("pgca_tail_w5_probs_h2", "pgca", lambda dt: ("GuidedCrossAttentionFn key_tail", "GuidedCrossAttentionFn key_tail probs",
                                                            "GuidedCrossAttentionFn need_probs", "GuidedCrossAttentionFn H>1", _route("GuidedCrossAttentionFn", dt)),
               dict(B=2, Lq=24, Lk=48, E=128, H=2, second="probs", tail=(8, 5)))
# ---- TokenGateFn ---------------------------------------------------------------------------------------------------------------
CASES += _both("gate_h8_res", "gate", ("TokenGateFn gate_dpre", "TokenGateFn residual"), dict(B=3, L=24, D=64, H=8, dd=32, res=True))
CASES += _both("gate_h8_nores", "gate", ("TokenGateFn gate_dpre", "TokenGateFn no residual"), dict(B=2, L=33, D=128, H=8, dd=64, res=False, dy="slice"))
# (the weight gradient of lin2 is a GEMM whose X row pitch is H: other H run on a zero-padded dlogits, see gate_h4_res_bf16 / gate_h2_nores_f32)
CASES += _both("gate_h16_res", "gate", lambda dt: ("TokenGateFn padded image" if dt == BF else "TokenGateFn kslow", "TokenGateFn residual"),
               dict(B=3, L=24, D=64, H=16, dd=32, res=True))
CASES += _both("gate_h24_nores", "gate", lambda dt: ("TokenGateFn padded image" if dt == BF else "TokenGateFn kslow", "TokenGateFn no residual"),
               dict(B=3, L=24, D=96, H=24, dd=40, res=False))
CASES += _both("gate_h4_nores", "gate", ("TokenGateFn kslow", "TokenGateFn no residual"), dict(B=3, L=24, D=64, H=4, dd=40, res=False), dts=(F32,))
# ---- DenseFn -------------------------------------------------------------------------------------------------------------------
CASES += _both("dense_t_sq128_relu", "dense", lambda dt: ("DenseFn weight_t square", "DenseFn act relu", "DenseFn direct bias", _route("DenseFn", dt)),
               dict(B=3, L=33, K=128, Kp=128, N=128, weight_t=True, act="relu"))
CASES += _both("dense_t_72x40", "dense", lambda dt: ("DenseFn weight_t", "DenseFn act False", "DenseFn direct bias", _route("DenseFn", dt)),
               dict(B=3, L=33, K=72, Kp=72, N=40, weight_t=True, act=False, dy="slice"))
CASES += _both("dense_k641_n100_gelu", "dense", lambda dt: ("DenseFn padded K", "DenseFn padded N", "DenseFn act gelu", _route("DenseFn", dt)),
               dict(B=3, L=24, K=641, Kp=648, N=100, act=True))
CASES += _both("dense_t_k385_n36", "dense", lambda dt: ("DenseFn weight_t", "DenseFn padded K", "DenseFn padded N", "DenseFn act False", _route("DenseFn", dt)),
               dict(B=2, L=33, K=385, Kp=392, N=36, weight_t=True, act=False))
CASES += _both("dense_residual", "dense", lambda dt: ("DenseFn residual", "DenseFn act False", "DenseFn direct bias", _route("DenseFn", dt)),
               dict(B=3, L=33, K=64, Kp=64, N=64, residual=True, act=False))
CASES += _both("dense_residual_gelu_n36", "dense", lambda dt: ("DenseFn residual", "DenseFn act gelu", "DenseFn padded N", _route("DenseFn", dt)),
               dict(B=3, L=33, K=64, Kp=64, N=36, residual=True, act=True))
CASES += _both("dense_x_only", "dense", lambda dt: ("DenseFn x only", "DenseFn padded N", "DenseFn act relu", _route("DenseFn", dt)),
               dict(B=3, L=33, K=64, Kp=64, N=36, act="relu", want=("x",), salt=1))
CASES += _both("dense_weight_only", "dense", ("DenseFn weight only", "DenseFn padded N", "DenseFn act False"),
               dict(B=3, L=33, K=64, Kp=64, N=36, act=False, want=("weight",)))
CASES += _both("dense_bias_only", "dense", ("DenseFn bias only", "DenseFn padded N", "DenseFn act gelu"),
               dict(B=3, L=33, K=64, Kp=64, N=36, act=True, want=("bias",)))
# ---- movers and pools ------------------------------------------------------------------------------------------------------------
CASES += _both("concat2", "concat2", ("Concat2Fn",), dict(B=3, L=33, wa=72, wb=40, dy="slice"))
CASES += _both("tokenmean", "tokenmean", ("TokenMeanFn",), dict(B=3, L=33, C=72, dy="slice"))
CASES += _both("expandtail", "expandtail", ("ExpandTailFn",), dict(B=3, lead=19, tail=8, w=5, C=72, dy="slice"))
CASES += _both("sitepool", "sitepool", ("SitePoolFn",), dict(B=3, L=36, C=72, site_len=9, dy="slice"), dts=(BF,))
CASES += _both("fillpool_to_bf16", "fillpool", ("FillPoolFn",), dict(B=3, S=36, F=40, site_len=9, out_dt=BF, dy="slice"))
CASES += _both("fillpool_to_f32", "fillpool", ("FillPoolFn",), dict(B=2, S=24, F=72, site_len=3, out_dt=F32), dts=(F32,))
CASES += _both("graphagg_n24", "graphagg", ("GraphAggregateFn n<=128",), dict(B=3, n=24, N=40, dy="slice"))
CASES += _both("graphagg_n130", "graphagg", ("GraphAggregateFn n>128",), dict(B=2, n=130, N=141))
# ---- embeddings ------------------------------------------------------------------------------------------------------------------
CASES += [Case("embedding_d127_f32", "embedding", F32, ("EmbeddingFn padded", "EmbeddingFn padding_idx"), dict(V=27, D=127, B=3, L=33, wdt=F32, padding_idx=0)),
          Case("embedding_d127_bf16", "embedding", BF, ("EmbeddingFn padded", "EmbeddingFn padding_idx"), dict(V=27, D=127, B=3, L=33, wdt=BF, padding_idx=0)),
          Case("embedding_d64_bf16", "embedding", BF, ("EmbeddingFn direct",), dict(V=27, D=64, B=3, L=33, wdt=BF, padding_idx=None)),
          Case("embedding_d64_f32_sliced_dy", "embedding", F32, ("EmbeddingFn non-contiguous dy", "EmbeddingFn padding_idx"),
               dict(V=27, D=64, B=3, L=33, wdt=F32, padding_idx=3, dy="slice"))]
CASES += _both("embedpad_junk_halo", "embedpad", ("EmbedPadFn",), dict(V=27, D=127, B=3, L=40, padding_idx=0))
CASES += _both("embedpad_junk_halo_sliced_dy", "embedpad", ("EmbedPadFn",), dict(V=27, D=63, B=2, L=33, padding_idx=None, dy="slice"))

CASES += [Case("linear_bias_only_n38_f32", "linear", F32, ("LinearFn plain", "LinearFn bias only"), dict(B=3, L=33, K=72, N=38, want=("bias",))),
          Case("linear_pe_n36_frozen_weight_bf16", "linear", BF, ("LinearFn pe_drop", "LinearFn kslow", "LinearFn bias only"),
               dict(B=3, L=24, K=40, N=36, pe=True, p=0.0, want=("x", "bias", "pe")))]
CASES += [Case("gate_h4_res_bf16", "gate", BF, ("TokenGateFn padded image", "TokenGateFn residual", "TokenGateFn padded H"), dict(B=3, L=24, D=64, H=4, dd=32, res=True)),
          Case("gate_h2_nores_f32", "gate", F32, ("TokenGateFn kslow", "TokenGateFn no residual", "TokenGateFn padded H"), dict(B=3, L=24, D=64, H=2, dd=40, res=False))]
_MLP = dict(B=3, LP=27, K=72, N1=96, N2=36)
CASES += _both("mlp_train", "mlp", ("run_mlp", "BatchNormRowsFn train"), dict(_MLP, training=True))
CASES += _both("mlp_tail_train", "mlp", ("run_mlp", "BatchNormWeightedTailFn"), dict(_MLP, training=True, tail=(27, 19, 5), dy="slice"))
CASES += _both("mlp_eval", "mlp", ("run_mlp", "BatchNormRowsFn eval"), dict(_MLP, training=False, dy="slice"))
CASES += _both("mlp_tail_eval", "mlp", ("run_mlp", "BatchNormRowsFn eval"), dict(_MLP, training=False, tail=(27, 19, 5)))
CASES += _both("mlp_eval_frozen", "mlp", ("run_mlp", "BatchNormRowsFn eval", "BatchNormRowsFn eval frozen"), dict(_MLP, training=False, frozen=True, salt=1))
CASES += [Case("expandrows_bf16", "expandrows", BF, ("ExpandRowsFn",), dict(S=300, C=128, lengths=(40, 71, 100), dy="slice")),
          Case("expandrows_f32", "expandrows", F32, ("ExpandRowsFn",), dict(S=300, C=72, lengths=(33, 120))),
          Case("sitepoolrows_bf16", "sitepoolrows", BF, ("SitePoolRowsFn",), dict(S=288, C=128, lengths=(40, 71, 100), site_len=9, dy="slice"))]
CASES += _both("embedrows_junk_rows", "embedrows", ("EmbedRowsFn",), dict(B=3, S=300, D=127, lengths=(40, 71, 100), padding_idx=0))
CASES += _both("embedrows_junk_rows_sliced_dy", "embedrows", ("EmbedRowsFn",), dict(B=2, S=300, D=63, lengths=(33, 120), padding_idx=None, dy="slice"))
# ---- ProteinCNNFn: S = 300 (288 where the pooling through the row map needs S / site_len % 8 == 0), C = 128, k = 3 / 6 / 9 ------------
_CNN = dict(B=3, S=300, C=128, lengths=(40, 71, 100))
CASES += _both("cnn_train_plain", "cnn", ("ProteinCNNFn training", "ProteinCNNFn plain"), dict(_CNN, layout="plain", training=True, dy="slice"))
CASES += _both("cnn_train_plain_no_dx", "cnn", ("ProteinCNNFn training", "ProteinCNNFn plain", "ProteinCNNFn no input gradient"),
               dict(_CNN, B=2, layout="plain", training=True, want_x=False))
CASES += _both("cnn_train_pooled", "cnn", ("ProteinCNNFn training", "ProteinCNNFn pooled"), dict(_CNN, layout="pooled", site_len=6, training=True), dts=(BF,))
CASES += _both("cnn_train_raw_dx", "cnn", ("ProteinCNNFn training", "ProteinCNNFn raw_dx", "EmbedPadFn"), dict(_CNN, layout="raw_dx", training=True))
CASES += _both("cnn_train_compact", "cnn", ("ProteinCNNFn training", "ProteinCNNFn compact", "EmbedRowsFn", "ExpandRowsFn"),
               dict(_CNN, layout="compact", training=True, dy="slice"))
CASES += _both("cnn_train_compact_pool", "cnn", ("ProteinCNNFn training", "ProteinCNNFn compact", "EmbedRowsFn", "SitePoolRowsFn"),
               dict(_CNN, S=288, layout="compact_pool", site_len=9, training=True, dy="slice"), dts=(BF,))
CASES += _both("cnn_eval_plain", "cnn", ("ProteinCNNFn eval", "ProteinCNNFn plain"), dict(_CNN, B=2, layout="plain", training=False))
CASES += _both("cnn_eval_compact", "cnn", ("ProteinCNNFn eval", "ProteinCNNFn compact", "EmbedRowsFn", "ExpandRowsFn"),
               dict(_CNN, layout="compact", training=False))
CASES += _both("cnn_eval_frozen_raw_dx", "cnn", ("ProteinCNNFn eval", "ProteinCNNFn eval frozen", "ProteinCNNFn raw_dx", "EmbedPadFn"),
               dict(_CNN, B=2, layout="raw_dx", training=False, frozen=True))
CASES += _both("cnn_eval_frozen_no_dx", "cnn", ("ProteinCNNFn eval", "ProteinCNNFn eval frozen", "ProteinCNNFn plain", "ProteinCNNFn no input gradient"),
               dict(_CNN, B=2, layout="plain", training=False, frozen=True, want_x=False))

BY_NAME = collections.OrderedDict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES)
