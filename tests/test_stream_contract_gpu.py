"""The stream contract of the native entry points: every launch of every ops.* wrapper goes to torch's CURRENT stream.

Every dl_* entry point takes a dl_stream and every wrapper passes ops._stream().  Only the training step ever runs under graph
capture — the one place where an off-stream launch fails loudly; the screening and inference kernels (pgca_pairs*, attn_probs,
bn_eval_bwd, embed_rows, rows_*) never do.  Here each wrapper is called once on a fresh side stream that is held back
(stream_ref.skew), behind copies that only then put the real inputs in place of a DECOY set:

    reference     call(real inputs) on the default stream
    test run      inputs hold the decoy; on stream S: delay, inputs <- real, call(inputs)

The outputs must agree bit for bit.  Any launch a wrapper sends to another stream — a helper, a second-stage reduction, a cached
buffer's first touch — runs during the delay: it reads decoy inputs or partial results nobody has written yet, or its output is
overwritten by the late copies.  The decoy is a second, equally valid draw (same index, label, length and table tensors, other
floating-point payloads), so a stray launch computes a wrong VALUE and never touches memory it should not.

CASES holds one small entry per launching wrapper, at the smallest shape that takes the family's multi-launch form where there
is one.  `reaches` declares the stream-taking symbols an entry calls; the GPU test records the symbols actually called and
compares, the CPU test checks that the declarations cover every stream-taking symbol of the signature table."""
import collections
import ctypes
import types

import pytest
import torch

from tests import stream_ref as S

DEV = S.DEV
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
I32, I64 = torch.int32, torch.int64

Case = collections.namedtuple("Case", "name make call reaches decoy")
CASES = []
# Stream-taking symbols that no entry reaches: profiling hooks and workspace-size queries only (none of those takes a stream
# today, so this is empty; a new one goes here with a one-line reason).
EXEMPT = {}


def case(name, reaches, decoy=None):
    def deco(fn):
        make, call = fn()
        CASES.append(Case(name, make, call, tuple(reaches), decoy))
        return fn
    return deco


def stream_symbols():
    """Every symbol of _lib's signature table whose last argument is the stream (void*, after an int status)."""
    from druglamp_amd import _lib
    return sorted(n for n, (res, args) in _lib.SIGNATURES.items() if res is _lib.c_i32 and args and args[-1] is _lib.c_vp)


def R(g, *shape, dt=F32, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(dt).to(DEV)


def U(g, *shape, lo=0.5, hi=1.5):
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).to(DEV)


def fixed(seed=99):
    """The generator of everything that is NOT payload (indices, labels, lengths, tables): the same in both draws."""
    return torch.Generator().manual_seed(seed)


def _ops():
    from druglamp_amd import ops
    return ops


# ---- GEMM family ------------------------------------------------------------------------------------------------------------
@case("cast", ["dl_cast"])
def _cast():
    return (lambda g: {"x": R(g, 1000)}), (lambda t: (_ops().cast(t["x"], BF16),))


@case("gemm", ["dl_gemm"])
def _gemm():
    M, N, K = 130, 136, 64
    return (lambda g: {"x": R(g, M, K), "w": R(g, N, K)}), (lambda t: (_ops().gemm(t["x"], t["w"], M=M, N=N, K=K),))


def _wgrad(t, x, w, M, N, K):
    return _ops().gemm(t[x], t[w], M=M, N=N, K=K, x_kslow=True, w_kslow=True, out_dtype=F32, split_k=0)


@case("gemm_split_k", ["dl_gemm"])                   # slabs + the reduction launch, scratch from ops._ws
def _gemm_split():
    M, N, K = 64, 128, 1024
    return (lambda g: {"x": R(g, K, M, dt=BF16), "w": R(g, K, N, dt=BF16)}), (lambda t: (_wgrad(t, "x", "w", M, N, K),))


@case("gemm_deferred_reduction", ["dl_gemm", "dl_reduce_batch"])
def _gemm_deferred():
    M, N, K = 64, 128, 1024

    def call(t):
        with _ops().deferred_reductions():
            out = _wgrad(t, "x", "w", M, N, K)
        return (out,)
    return (lambda g: {"x": R(g, K, M, dt=BF16), "w": R(g, K, N, dt=BF16)}), call


@case("gemm_group", ["dl_gemm_group", "dl_reduce_batch"])       # the grouped weight gradients of a block's backward
def _gemm_group():
    shapes = ((128, 136, 1000), (64, 256, 1024))

    def make(g):
        t = {}
        for i, (M, N, K) in enumerate(shapes):
            t["x%d" % i], t["w%d" % i] = R(g, K, M, dt=BF16), R(g, K, N, dt=BF16)
        return t

    def call(t):
        with _ops().deferred_reductions():
            outs = tuple(_wgrad(t, "x%d" % i, "w%d" % i, M, N, K) for i, (M, N, K) in enumerate(shapes))
        return outs
    return make, call


@case("gemm_pair", ["dl_gemm_pair"])
def _gemm_pair():
    M, N, K = 130, 136, 64
    make = lambda g: {"x0": R(g, M, K), "w0": R(g, N, K), "x1": R(g, M, K), "w1": R(g, N, K)}       # noqa: E731
    return make, (lambda t: tuple(_ops().gemm_pair((t["x0"], t["x1"]), (t["w0"], t["w1"]), M=M, N=N, K=K)))


@case("colsum", ["dl_colsum"])                       # thousands of rows: partial sums + the final launch
def _colsum():
    return (lambda g: {"x": R(g, 5000, 264)}), (lambda t: (_ops().colsum(t["x"]),))


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------
def _ln_make(g, M=1000, D=256):
    t = {"x": R(g, M, D, dt=BF16), "gamma": U(g, D), "beta": R(g, D, scale=0.1)}
    _, t["mean"], t["rstd"] = _ops().layernorm_fwd(t["x"], t["gamma"], t["beta"], 1e-5)
    t["dy"] = R(g, M, D, dt=BF16)
    return t


@case("layernorm_fwd", ["dl_layernorm_fwd"])
def _ln_fwd():
    return (lambda g: {k: v for k, v in _ln_make(g).items() if k in ("x", "gamma", "beta")}), \
        (lambda t: tuple(_ops().layernorm_fwd(t["x"], t["gamma"], t["beta"], 1e-5)))


@case("layernorm_bwd_param_grads", ["dl_layernorm_bwd"])
def _ln_bwd():
    return _ln_make, (lambda t: tuple(_ops().layernorm_bwd(t["dy"], t["x"], t["mean"], t["rstd"], t["gamma"])))


@case("layernorm_bwd_deferred", ["dl_layernorm_bwd", "dl_reduce_batch"])
def _ln_bwd_deferred():
    def call(t):
        with _ops().deferred_reductions():
            out = _ops().layernorm_bwd(t["dy"], t["x"], t["mean"], t["rstd"], t["gamma"])
        return tuple(out)
    return _ln_make, call


# ---- attention --------------------------------------------------------------------------------------------------------------
_AT = dict(P=2, H=2, Lq=65, Lk=63, hd=64)


def _attn_kw():
    P, H, Lq, Lk, hd = (_AT[k] for k in ("P", "H", "Lq", "Lk", "hd"))
    qs, ks = (H * Lq * hd, Lq * hd, hd), (H * Lk * hd, Lk * hd, hd)
    return dict(n_problems=P, n_heads=H, n_segments=1, partner_shift=0, Lq=Lq, Lk=Lk, head_dim=hd, scale=hd ** -0.5,
                q_strides=qs, k_strides=ks), qs, ks


def _attn_fwd(t):
    kw, qs, ks = _attn_kw()
    out = torch.empty_like(t["q"])
    lse = _ops().attn_fwd(t["q"], t["k"], t["v"], out=out, v_strides=ks, o_strides=qs, o_ss=out.numel(), **kw)
    return out, lse


def _attn_make(g, bwd=False):
    P, H, Lq, Lk, hd = (_AT[k] for k in ("P", "H", "Lq", "Lk", "hd"))
    t = {"q": R(g, P, H, Lq, hd, dt=BF16, scale=0.7), "k": R(g, P, H, Lk, hd, dt=BF16, scale=0.7), "v": R(g, P, H, Lk, hd, dt=BF16)}
    if bwd:
        t["o"], t["lse"] = _attn_fwd(t)
        t["do"] = R(g, P, H, Lq, hd, dt=BF16, scale=0.5)
    return t


@case("attn_fwd", ["dl_attn_fwd"])
def _c_attn_fwd():
    return _attn_make, _attn_fwd


@case("attn_bwd", ["dl_attn_bwd"])
def _c_attn_bwd():
    def call(t):
        kw, qs, ks = _attn_kw()
        dq, dk, dv = torch.empty_like(t["q"]), torch.empty_like(t["k"]), torch.empty_like(t["v"])
        _ops().attn_bwd(t["q"], t["k"], t["v"], t["o"], t["do"], t["lse"], v_strides=ks, o_strides=qs, o_ss=t["o"].numel(),
                        do_strides=qs, do_ss=t["o"].numel(), dq=dq, dq_strides=qs, dk=dk, dk_strides=ks, dv=dv, dv_strides=ks, **kw)
        return dq, dk, dv
    return (lambda g: _attn_make(g, bwd=True)), call


@case("attn_probs_own_lse", ["dl_attn_probs"])       # lse=None: the LSE launch into ops._ws, then the map
def _c_attn_probs():
    def call(t):
        kw, _, _ = _attn_kw()
        return (_ops().attn_probs(t["q"], t["k"], head_mean=True, **kw),)
    return (lambda g: {k: v for k, v in _attn_make(g).items() if k != "v"}), call


# ---- pair-indexed PGCA (screening) ------------------------------------------------------------------------------------------
_PG = dict(n_q=2, Lq=40, E=128, tail=8, pi=(1, 0, 1, 0, 1), di=(0, 1, 1, 0, 1))


def _pairs_make(g, ragged, grad=False):
    n_q, Lq, E, tail = _PG["n_q"], _PG["Lq"], _PG["E"], _PG["tail"]
    t = {"q": R(g, n_q, Lq, E, dt=BF16, scale=0.7), "left": R(g, n_q, Lq, E, dt=BF16), "bias": R(g, E, scale=0.5),
         "pi": torch.tensor(_PG["pi"], dtype=I32, device=DEV), "di": torch.tensor(_PG["di"], dtype=I32, device=DEV)}
    if ragged:                                       # two drugs of 16 and 24 stored keys, the last 8 standing for 3 / 2 keys each
        t["rows"] = torch.cat((R(g, 40, E, dt=BF16, scale=0.7), R(g, 40, E, dt=BF16)), dim=1)
        t["row0"] = torch.tensor([0, 16], dtype=I64, device=DEV)
        t["keys"] = torch.tensor([16, 24], dtype=I32, device=DEV)
        t["w"] = torch.tensor([3.0, 2.0], dtype=F32, device=DEV)
    else:                                            # two drugs of 24 stored keys, the last 8 standing for 3 keys each
        t["kv"] = torch.cat((R(g, 2, 24, E, dt=BF16, scale=0.7), R(g, 2, 24, E, dt=BF16)), dim=2)
    if grad:
        t["d_out"] = R(g, len(_PG["pi"]), Lq, E, dt=BF16, scale=0.5)
        t["d_sites"] = R(g, len(_PG["pi"]), Lq, E, dt=BF16, scale=0.5)
    return t


_SC = 128 ** -0.5


@case("pgca_pairs", ["dl_pgca_pairs_fwd"])
def _c_pairs():
    return (lambda g: _pairs_make(g, False)), \
        (lambda t: (_ops().pgca_pairs(t["q"], t["kv"], t["pi"], t["di"], scale=_SC, left=t["left"], bias=t["bias"], key_tail=(8, 3.0)),))


@case("pgca_pairs_ragged", ["dl_pgca_pairs_ragged_fwd"])
def _c_pairs_ragged():
    return (lambda g: _pairs_make(g, True)), \
        (lambda t: (_ops().pgca_pairs_ragged(t["q"], t["rows"], t["row0"], t["keys"], t["w"], t["pi"], t["di"], scale=_SC, key_tail_rows=8,
                                             left=t["left"], bias=t["bias"]),))


@case("pgca_pairs_probs", ["dl_pgca_pairs_probs"])
def _c_pairs_probs():
    return (lambda g: _pairs_make(g, False)), \
        (lambda t: (_ops().pgca_pairs_probs(t["q"], t["kv"], t["pi"], t["di"], scale=_SC, key_tail=(8, 3.0), expand_tail=True),))


@case("pgca_pairs_ragged_probs", ["dl_pgca_pairs_ragged_probs"])
def _c_pairs_ragged_probs():
    return (lambda g: _pairs_make(g, True)), \
        (lambda t: (_ops().pgca_pairs_ragged_probs(t["q"], t["rows"], t["row0"], t["keys"], t["w"], t["pi"], t["di"], scale=_SC,
                                                   key_tail_rows=8, cols=32, expand_tail=True),))


@case("pgca_pairs_profile", ["dl_pgca_pairs_profile"])
def _c_pairs_profile():
    return (lambda g: _pairs_make(g, False)), \
        (lambda t: tuple(_ops().pgca_pairs_profile(t["q"], t["kv"], t["pi"], t["di"], scale=_SC, key_tail=(8, 3.0))))


@case("pgca_pairs_ragged_profile", ["dl_pgca_pairs_ragged_profile"])
def _c_pairs_ragged_profile():
    return (lambda g: _pairs_make(g, True)), \
        (lambda t: tuple(_ops().pgca_pairs_ragged_profile(t["q"], t["rows"], t["row0"], t["keys"], t["w"], t["pi"], t["di"], scale=_SC,
                                                          key_tail_rows=8, cols=32)))


@case("pgca_pairs_attr", ["dl_pgca_pairs_attr"])
def _c_pairs_attr():
    return (lambda g: _pairs_make(g, False, grad=True)), \
        (lambda t: tuple(_ops().pgca_pairs_attr(t["q"], t["kv"], t["d_out"], t["pi"], t["di"], scale=_SC, key_tail=(8, 3.0),
                                                sites=t["left"], d_sites=t["d_sites"])))


@case("pgca_pairs_ragged_attr", ["dl_pgca_pairs_ragged_attr"])
def _c_pairs_ragged_attr():
    return (lambda g: _pairs_make(g, True, grad=True)), \
        (lambda t: tuple(_ops().pgca_pairs_ragged_attr(t["q"], t["rows"], t["row0"], t["keys"], t["w"], t["d_out"], t["pi"], t["di"],
                                                       scale=_SC, key_tail_rows=8, cols=32, sites=t["left"], d_sites=t["d_sites"])))


# ---- MHLA gate, elementwise, ingest -----------------------------------------------------------------------------------------
def _gate_make(g, bwd=False):
    B, L, D, H = 2, 16, 64, 8
    t = {"v": R(g, B, L, D, dt=BF16), "logits": R(g, B, L, H, dt=BF16)}
    if bwd:
        _, t["gate"] = _ops().token_gate_fwd(t["v"], t["logits"], H, True)
        del t["logits"]
        t["dout"] = R(g, B, L, D, dt=BF16)
    return t


@case("token_gate_fwd", ["dl_token_gate_fwd"])
def _c_gate_fwd():
    return _gate_make, (lambda t: tuple(_ops().token_gate_fwd(t["v"], t["logits"], 8, True)))


@case("token_gate_bwd", ["dl_token_gate_bwd"])
def _c_gate_bwd():
    return (lambda g: _gate_make(g, bwd=True)), (lambda t: tuple(_ops().token_gate_bwd(t["dout"], t["v"], t["gate"], 8, True)))


@case("gate_dpre", ["dl_gate_dpre"])
def _c_gate_dpre():
    return (lambda g: {"dl": R(g, 32, 8, dt=BF16), "w2": R(g, 8, 64, dt=BF16), "pre": R(g, 32, 64, dt=BF16)}), \
        (lambda t: (_ops().gate_dpre(t["dl"], t["w2"], t["pre"]),))


@case("add_rowmod_dropout", ["dl_add_rowmod_dropout"])
def _c_add_rowmod():
    return (lambda g: {"x": R(g, 64, 32, dt=BF16), "pe": R(g, 16, 32, dt=BF16)}), \
        (lambda t: (_ops().add_rowmod_dropout(t["x"], t["pe"], 0.1, 3),))


@case("dropout_apply", ["dl_dropout_apply"])
def _c_dropout():
    return (lambda g: {"x": R(g, 64, 32, dt=BF16)}), (lambda t: (_ops().dropout_apply(t["x"], 0.1, 5),))


@case("rowmod_sum", ["dl_rowmod_sum"])
def _c_rowmod_sum():
    return (lambda g: {"x": R(g, 64, 32, dt=BF16)}), (lambda t: (_ops().rowmod_sum(t["x"], 16),))


@case("gelu_bwd", ["dl_gelu_bwd"])
def _c_gelu_bwd():
    return (lambda g: {"dy": R(g, 32, 64, dt=BF16), "pre": R(g, 32, 64, dt=BF16)}), (lambda t: (_ops().gelu_bwd(t["dy"], t["pre"]),))


@case("fill_pool", ["dl_fill_pool"])
def _c_fill_pool():
    def make(g):
        x = R(g, 2, 36, 40, dt=BF16)
        x[:, 30:] = 0                                # zero rows: the fill bit (the same rows in both draws)
        return {"x": x}
    return make, (lambda t: tuple(_ops().fill_pool(t["x"], 9, BF16)))


@case("interleave_streams", ["dl_interleave_streams"])
def _c_interleave():
    return (lambda g: {"x": R(g, 2, 3, 7, 64, dt=BF16)}), (lambda t: (_ops().interleave_streams(t["x"]),))


@case("concat2", ["dl_concat2"])
def _c_concat2():
    return (lambda g: {"a": R(g, 10, 128, dt=BF16), "b": R(g, 10, 128, dt=BF16)}), (lambda t: (_ops().concat2(t["a"], t["b"]),))


@case("gather_pad", ["dl_gather_pad"])
def _c_gather_pad():
    def make(g):
        return {"store": R(g, 50, 8), "offsets": torch.tensor([0, 20], dtype=I64, device=DEV),
                "lengths": torch.tensor([7, 11], dtype=I32, device=DEV)}
    return make, (lambda t: (_ops().gather_pad(t["store"], t["offsets"], t["lengths"], 32, True),))


def _ids(B, L, V=27):
    return torch.randint(1, V, (B, L), generator=fixed()).to(DEV)


@case("embed_pad", ["dl_embed_pad"])
def _c_embed_pad():
    def make(g):
        return {"ids": _ids(2, 24), "weight": R(g, 27, 15), "fill": (torch.rand(2, 24, generator=fixed(3)) < 0.2).float().to(DEV)}
    return make, (lambda t: (_ops().embed_pad(t["ids"], t["weight"], t["fill"], 4),))


@case("weight_prep", ["dl_weight_prep"])
def _c_weight_prep():
    import numpy as np
    item_t = np.dtype([("src", "<u8"), ("dst", "<u8"), ("ld", "<i8"), ("rows", "<i4"), ("cols", "<i4"),
                       ("row0", "<i4"), ("transpose", "<i4"), ("cs", "<i8")])       # dl_wprep_item, as functional._refresh_all_images packs it
    r, c = 70, 130

    def call(t):
        image = torch.empty((r, c), dtype=BF16, device=DEV)
        items = np.array([(t["master"].data_ptr(), image.data_ptr(), c, r, c, 0, 0, 0)], dtype=item_t)
        ntile = ((r + 63) // 64) * ((c + 63) // 64)
        items_dev = torch.from_numpy(items.view(np.uint8).copy()).to(DEV, non_blocking=False)
        bmap_dev = torch.tensor([(0, k) for k in range(ntile)], dtype=I32).reshape(-1).to(DEV)
        _ops().weight_prep(items_dev, bmap_dev, ntile, BF16)
        t["_keep"] = (items_dev, bmap_dev)           # (alive until the caller has synchronised)
        return (image,)
    return (lambda g: {"master": R(g, r, c)}), call


# ---- graph kernels ----------------------------------------------------------------------------------------------------------
def _adj(g, B=2, n=20):
    a = (torch.rand(B, n, n, generator=g) < 0.2).float()
    a = ((a + a.transpose(1, 2)) > 0).float()
    idx = torch.arange(n)
    a[:, idx, idx] = 2.0
    return a.to(DEV)


@case("norm_adjacency", ["dl_norm_adjacency"])
def _c_norm_adj():
    return (lambda g: {"adj": _adj(g)}), (lambda t: (_ops().norm_adjacency(t["adj"], F32),))


@case("graph_aggregate", ["dl_graph_aggregate"])
def _c_graph_agg():
    return (lambda g: {"ahat": R(g, 2, 20, 20, dt=BF16, scale=0.2), "feat": R(g, 2, 32, 128, dt=BF16)}), \
        (lambda t: (_ops().graph_aggregate(t["ahat"], t["feat"]),))


# ---- ProteinCNN: pooling, the distinct-row tables ---------------------------------------------------------------------------
@case("cnn_sitepool_fwd", ["dl_cnn_sitepool_fwd"])
def _c_sitepool_fwd():
    return (lambda g: {"z": R(g, 2, 96 + 8, 64, dt=BF16)}), (lambda t: (_ops().cnn_sitepool_fwd(t["z"], 96, 4, 3),))


@case("cnn_sitepool_bwd", ["dl_cnn_sitepool_bwd"])
def _c_sitepool_bwd():
    return (lambda g: {"d": R(g, 2, 32, 64, dt=BF16)}), (lambda t: (_ops().cnn_sitepool_bwd(t["d"], 96, 4, 3),))


_PLAN = dict(S=1152, lengths=[98, 398, 511], site_len=9, C=64)
_plan_dev = []


def _pd():
    """The device row tables of the three-protein plan (tests/test_protein_cnn_compact_gpu.py), built once."""
    if not _plan_dev:
        from druglamp_amd.protein_plan import PlanDev, ProteinPlan
        _plan_dev.append(PlanDev(ProteinPlan(_PLAN["lengths"], _PLAN["S"], 64), DEV))
        torch.cuda.synchronize()
    return _plan_dev[0]


def _tiled_ids():
    import numpy as np
    from druglamp_amd.data import repeat_integer_label
    rs = np.random.RandomState(0)
    S_, lengths = _PLAN["S"], _PLAN["lengths"]
    ids, fill = torch.zeros(len(lengths), S_, dtype=F64), torch.zeros(len(lengths), S_)
    for b, L in enumerate(lengths):
        ids[b] = torch.from_numpy(repeat_integer_label(rs.randint(1, 26, L), S_))
        fill[b, (S_ // (L + 2)) * (L + 2):] = 1.0
    return ids.long().to(DEV), fill.to(DEV)


@case("embed_rows", ["dl_embed_rows"])
def _c_embed_rows():
    def make(g):
        pd = _pd()
        ids, fill = _tiled_ids()
        return {"ids": ids, "fill": fill, "weight": R(g, 27, 63), "src": pd.src.clone(), "period": pd.period.clone()}
    return make, (lambda t: (_ops().embed_rows(t["ids"], t["weight"], t["fill"], t["src"], t["period"]),))


@case("rows_gather", ["dl_rows_gather"])
def _c_rows_gather():
    return (lambda g: {"z": R(g, _pd().rows, 64, dt=BF16), "row_of": _pd().row_of.clone()}), \
        (lambda t: (_ops().rows_gather(t["z"], t["row_of"]),))


@case("rows_sum_strided", ["dl_rows_sum_strided"])
def _c_rows_sum():
    return (lambda g: {"x": R(g, len(_PLAN["lengths"]) * _PLAN["S"], 64, dt=BF16), "rep": _pd().rep.clone()}), \
        (lambda t: (_ops().rows_sum_strided(t["x"], t["rep"]),))


@case("cnn_sitepool_rows_fwd", ["dl_cnn_sitepool_rows_fwd"])
def _c_sitepool_rows_fwd():
    return (lambda g: {"z": R(g, _pd().rows, _PLAN["C"], dt=BF16), "row_of": _pd().row_of.clone()}), \
        (lambda t: (_ops().cnn_sitepool_rows_fwd(t["z"], t["row_of"], len(_PLAN["lengths"]), _PLAN["S"], _PLAN["site_len"]),))


@case("cnn_sitepool_rows_bwd", ["dl_cnn_sitepool_rows_bwd"])
def _c_sitepool_rows_bwd():
    def make(g):
        pd = _pd()
        return {"d": R(g, len(_PLAN["lengths"]), _PLAN["S"] // _PLAN["site_len"], _PLAN["C"], dt=BF16), "rep": pd.rep.clone(),
                "row_of": pd.row_of.clone()}
    return make, (lambda t: (_ops().cnn_sitepool_rows_bwd(t["d"], t["rep"], t["row_of"], _PLAN["S"], _PLAN["site_len"]),))


@case("protein_plan_build", ["dl_protein_plan_build"])          # integer inputs only: the tables it writes are the payload
def _c_plan_build():
    def make(g):
        pd = _pd()
        return {"len": pd.len_dev.clone(), "tables": torch.full((pd._off[4],), 0x5a, dtype=torch.uint8, device=DEV)}

    def call(t):
        pd = _pd()
        o_w, o_rep, o_map, o_per, o_len = pd._off
        buf = t["tables"]
        view = types.SimpleNamespace(buf=buf, len_dev=t["len"], B=pd.B, S=pd.S, rows=pd.rows, src=buf[:o_w].view(I32),
                                     w=buf[o_w:o_rep].view(F32), rep=buf[o_rep:o_map].view(I32), row_of=buf[o_map:o_per].view(I32),
                                     period=buf[o_per:o_len].view(I32))
        _ops().protein_plan_build(view)
        return (buf,)
    return make, call


def _eq_rows(g, equal):
    x = R(g, 3, 24, 16, dt=BF16)
    if equal:
        x[:, 16:] = x[0, 16]
    return {"x": x}


# the output is one guard bit: the real draw violates the rule (the bit must come up), the decoy keeps it (an early launch
# would leave the word at zero)
@case("rows_equal_check", ["dl_rows_equal_check"], decoy=lambda g: _eq_rows(g, True))
def _c_rows_equal():
    def call(t):
        _ops().rows_equal_check(t["x"], 16, 2)
        return (_ops().guard_flags(DEV),)
    return (lambda g: _eq_rows(g, False)), call


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------
_BN = dict(R=200, C=64, win=40, halo=4, valid=32, n=160)


def _bn_make(g, rw=False, dt=BF16):
    Rr, C = _BN["R"], _BN["C"]
    t = {"y": R(g, Rr, C, dt=dt), "dz": R(g, Rr, C, dt=dt), "mean": R(g, C, scale=0.1), "rstd": U(g, C), "gamma": U(g, C),
         "beta": R(g, C, scale=0.1), "sums": R(g, 2 * C)}
    if rw:                                           # a table: halo rows, context rows, multiplicities
        w = torch.tensor([-1.0, 0.0, 1.0, 1.0, 3.0], dtype=F32).repeat(Rr // 5)
        t["rw"] = w.to(DEV)
    return t


def _bn_rule(t):
    return (0, 0, 0, t["rw"]) if "rw" in t else (_BN["win"], _BN["halo"], _BN["valid"])


def _bn_cases(suffix, rw):
    sym = lambda base: [base + ("_rw" if rw else "")]                                       # noqa: E731
    make = lambda g: _bn_make(g, rw)                                                        # noqa: E731

    @case("bn_stats" + suffix, sym("dl_bn_stats"))
    def _a():
        return make, (lambda t: (_ops().bn_stats(t["y"], *_bn_rule(t)),))

    @case("bn_apply_fwd" + suffix, sym("dl_bn_apply_fwd"))
    def _b():
        return make, (lambda t: (_ops().bn_apply_fwd(t["y"], t["mean"], t["rstd"], t["gamma"], t["beta"], *_bn_rule(t)),))

    @case("bn_bwd_reduce" + suffix, sym("dl_bn_bwd_reduce"))
    def _c():
        return make, (lambda t: (_ops().bn_bwd_reduce(t["dz"], t["y"], t["mean"], t["rstd"], *_bn_rule(t)),))

    @case("bn_bwd_apply" + suffix, sym("dl_bn_bwd_apply"))
    def _d():
        return make, (lambda t: (_ops().bn_bwd_apply(t["dz"], t["y"], t["mean"], t["rstd"], t["gamma"], t["sums"], 1.0 / _BN["n"], True,
                                                      *_bn_rule(t)),))


_bn_cases("", False)
_bn_cases("_rw", True)


@case("bn_stats_finalize", ["dl_bn_stats_finalize"])            # partial sums + the second stage; running statistics in place
def _c_bn_stats_finalize():
    def make(g):
        t = _bn_make(g)
        t["rm"], t["rv"] = R(g, _BN["C"], scale=0.1), U(g, _BN["C"])
        return t

    def call(t):
        out = _ops().bn_stats_finalize(t["y"], _BN["win"], _BN["halo"], _BN["valid"], _BN["n"], 1e-5, 0.1, t["rm"], t["rv"])
        return tuple(out) + (t["rm"], t["rv"])
    return make, call


@case("bn_finalize", ["dl_bn_finalize"])
def _c_bn_finalize():
    def make(g):
        C = _BN["C"]
        return {"sums": torch.cat((R(g, C, scale=3.0), U(g, C, lo=200.0, hi=300.0))), "rm": R(g, C, scale=0.1), "rv": U(g, C)}

    def call(t):
        return tuple(_ops().bn_finalize(t["sums"], _BN["n"], 1e-5, 0.1, t["rm"], t["rv"])) + (t["rm"], t["rv"])
    return make, call


@case("bn_tail_fix", ["dl_bn_tail_fix"])             # in place on dy
def _c_bn_tail_fix():
    def make(g):
        t = _bn_make(g)
        t["dy"] = R(g, _BN["R"], _BN["C"], dt=BF16)
        return t
    return make, (lambda t: (_ops().bn_tail_fix(t["dy"], t["y"], t["mean"], t["rstd"], t["gamma"], t["sums"], 1.0 / 400, 4, 40, 32),))


@case("bn_apply_relu_fwd", ["dl_bn_apply_relu_fwd"])
def _c_bn_relu_fwd():
    return _bn_make, (lambda t: (_ops().bn_apply_relu_fwd(t["y"], t["mean"], t["rstd"], t["gamma"], t["beta"]),))


@case("bn_relu_bwd", ["dl_bn_relu_bwd"])
def _c_bn_relu_bwd():
    return _bn_make, (lambda t: tuple(_ops().bn_relu_bwd(t["dz"], t["y"], t["mean"], t["rstd"], t["gamma"], t["beta"], 1.0 / _BN["R"])))


@case("bn_eval_bwd", ["dl_bn_eval_bwd"])
def _c_bn_eval_bwd():
    return _bn_make, (lambda t: tuple(_ops().bn_eval_bwd(t["dz"], t["y"], t["mean"], t["rstd"], t["gamma"], t["beta"], relu_out=True,
                                                         win=_BN["win"], halo=_BN["halo"], valid=_BN["valid"])))


# ---- losses -----------------------------------------------------------------------------------------------------------------
@case("cos_rowloss_fwd", ["dl_cos_rowloss_fwd"])
def _c_cos_fwd():
    return (lambda g: {"x": R(g, 20, 64), "y": R(g, 20, 64)}), (lambda t: (_ops().cos_rowloss_fwd(t["x"], t["y"]),))


@case("cos_rowloss_bwd", ["dl_cos_rowloss_bwd"])
def _c_cos_bwd():
    return (lambda g: {"x": R(g, 20, 64), "y": R(g, 20, 64)}), (lambda t: (_ops().cos_rowloss_bwd(t["x"], t["y"], 0.05),))


def _ntx_make(g, bwd=None):
    t = {"q": R(g, 40, 64), "k": R(g, 40, 64)}
    if bwd == "plain":
        _, t["lse"] = _ops().ntxent_fwd(t["q"], t["k"], 0.5)
    elif bwd == "ex":
        _, t["lse"], _ = _ops().ntxent_fwd_ex(t["q"], t["k"], t["q"], t["k"], 0, 0, 40, 0.5)
    return t


@case("ntxent_fwd", ["dl_ntxent_fwd"])               # streamed tiles into ops._ws, then the final reduction
def _c_ntx_fwd():
    return _ntx_make, (lambda t: tuple(_ops().ntxent_fwd(t["q"], t["k"], 0.5)))


@case("ntxent_bwd", ["dl_ntxent_bwd"])
def _c_ntx_bwd():
    return (lambda g: _ntx_make(g, "plain")), (lambda t: tuple(_ops().ntxent_bwd(t["q"], t["k"], 0.5, t["lse"], 1.0)))


@case("ntxent_fwd_ex", ["dl_ntxent_fwd_ex"])
def _c_ntx_fwd_ex():
    return _ntx_make, (lambda t: tuple(_ops().ntxent_fwd_ex(t["q"], t["k"], t["q"], t["k"], 0, 0, 40, 0.5)))


@case("ntxent_bwd_ex", ["dl_ntxent_bwd_ex"])
def _c_ntx_bwd_ex():
    return (lambda g: _ntx_make(g, "ex")), \
        (lambda t: tuple(_ops().ntxent_bwd_ex(t["q"], t["k"], t["q"], t["k"], 0, 0, 40, 0.5, t["lse"], t["lse"], 1.0 / 80)))


def _tri_make(g, bwd=False):
    t = {"p": R(g, 6, 32), "d": R(g, 7, 32), "gt": torch.randint(-1, 2, (6, 7), generator=fixed()).to(torch.int8).to(DEV)}
    if bwd:
        _, t["ntri"], t["buf"] = _ops().triplet_sigcos_fwd(t["p"], t["d"], t["gt"], 0.25)
    return t


@case("triplet_sigcos_fwd", ["dl_triplet_sigcos_fwd"])
def _c_tri_fwd():
    def call(t):
        loss, ntri, buf = _ops().triplet_sigcos_fwd(t["p"], t["d"], t["gt"], 0.25)
        return loss, ntri, buf[:6 * 7]               # the distance matrix; behind it scratch the forward only partly writes
    return _tri_make, call


@case("triplet_sigcos_bwd", ["dl_triplet_sigcos_bwd"])
def _c_tri_bwd():
    return (lambda g: _tri_make(g, True)), \
        (lambda t: tuple(_ops().triplet_sigcos_bwd(t["p"], t["d"], t["gt"], 0.25, t["buf"], t["ntri"], 1.0)))


def _ce_make(g, bwd=False):
    N = 5000
    t = {"logits": R(g, N, 32, dt=BF16), "labels": torch.randint(0, 27, (N,), generator=fixed()).to(DEV)}
    if bwd:
        t["out2"], t["lse"] = _ops().ce_rows_fwd(t["logits"], t["labels"], 27, -100)
        t["go"] = U(g, 1)
    return t


@case("ce_rows_fwd", ["dl_ce_rows_fwd"])             # thousands of rows: per-workgroup partials + the final launch
def _c_ce_fwd():
    return _ce_make, (lambda t: tuple(_ops().ce_rows_fwd(t["logits"], t["labels"], 27, -100)))


@case("ce_rows_bwd", ["dl_ce_rows_bwd"])
def _c_ce_bwd():
    return (lambda g: _ce_make(g, True)), \
        (lambda t: (_ops().ce_rows_bwd(t["logits"], t["labels"], 27, -100, t["lse"], t["out2"], t["go"]),))


def _cls_make(g, bwd=False):
    N = 5000                                         # above 4096 rows: the partial-sum form with its final launch
    t = {"score": R(g, N, 1), "labels": (torch.rand(N, generator=fixed()) < 0.3).float().to(DEV)}
    if bwd:
        t["out2"], _ = _ops().cls_loss_fwd(t["score"], t["labels"], None, 2.0, 1.0, 2.0)
        t["go"] = U(g, 1)
    return t


@case("cls_loss_fwd", ["dl_cls_loss_fwd"])
def _c_cls_fwd():
    return _cls_make, (lambda t: tuple(_ops().cls_loss_fwd(t["score"], t["labels"], None, 2.0, 1.0, 2.0)))


@case("cls_loss_bwd", ["dl_cls_loss_bwd"])
def _c_cls_bwd():
    return (lambda g: _cls_make(g, True)), \
        (lambda t: (_ops().cls_loss_bwd(t["score"], t["labels"], None, 2.0, 1.0, 2.0, t["out2"], t["go"]),))


# ---- optimiser phase: in place, the mutated tensors are the outputs ----------------------------------------------------------
def _opt_make(g, n=5000):
    return {"param": R(g, n), "grad": R(g, n, scale=0.1), "m": R(g, n, scale=0.01), "v": U(g, n, lo=1e-4, hi=1e-3),
            "lowp": R(g, n, dt=BF16)}


def _opt_out(t):
    return t["param"], t["m"], t["v"], t["lowp"]


@case("adamw_step", ["dl_adamw_step"])
def _c_adamw():
    def call(t):
        _ops().adamw_step(t["param"], t["grad"], t["m"], t["v"], lr=1e-3, step=3, lowp=t["lowp"])
        return _opt_out(t)
    return _opt_make, call


@case("adamw_step_guarded", ["dl_adamw_step_guarded"])
def _c_adamw_guarded():
    def make(g):
        t = _opt_make(g)
        t["guard"] = torch.tensor([0.5, 2.0, 0.0, 0.0], dtype=F32, device=DEV)
        return t

    def call(t):
        _ops().adamw_step_guarded(t["param"], t["grad"], t["m"], t["v"], t["guard"], lr=1e-3, step=3, lowp=t["lowp"])
        return _opt_out(t)
    return make, call


@case("adamw_step_groups", ["dl_adamw_step_groups"])
def _c_adamw_groups():
    def make(g):
        t = _opt_make(g)
        t["quad"] = (torch.arange(1250) // 500).to(torch.uint8).to(DEV)
        t["tab"] = torch.tensor([[1.0, 0.01], [0.5, 0.0], [2.0, 0.1]], dtype=F32, device=DEV)
        return t

    def call(t):
        _ops().adamw_step_groups(t["param"], t["grad"], t["m"], t["v"], t["quad"], t["tab"], lr=1e-3, step=3, lowp=t["lowp"])
        return _opt_out(t)
    return make, call


@case("grad_guard", ["dl_grad_sqnorm", "dl_grad_guard_finalize"])     # per-workgroup partials, the fp64 sum, the decision
def _c_grad_guard():
    n = 10000

    def make(g):
        return {"g": R(g, n), "acc": torch.zeros(1, dtype=F64, device=DEV), "guard": torch.zeros(4, dtype=F32, device=DEV),
                "counters": torch.zeros(2, dtype=I64, device=DEV)}

    def call(t):
        ops = _ops()
        ws = torch.empty(ops.grad_sqnorm_workspace_bytes(n) // 8, dtype=F64, device=DEV)
        ops.grad_sqnorm(t["g"], t["acc"], ws)
        ops.grad_guard_finalize(t["acc"], t["guard"], t["counters"], max_norm=1.0)
        return t["acc"], t["guard"], t["counters"]
    return make, call


@case("ema_update", ["dl_ema_update"])
def _c_ema():
    def call(t):
        _ops().ema_update(t["ema"], t["param"], 0.1)
        return (t["ema"],)
    return (lambda g: {"ema": R(g, 5000), "param": R(g, 5000)}), call


# ---- the procedure ----------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the loaded library while a case runs: hands every symbol on and notes its name."""

    def __init__(self, real):
        self._real, self.seen = real, set()

    def __getattr__(self, name):
        self.seen.add(name)
        return getattr(self._real, name)


def _clone(t):
    return {k: v.clone() for k, v in t.items()}


def _out_bits(outs):
    assert isinstance(outs, tuple) and outs and all(torch.is_tensor(o) for o in outs), "a case returns a tuple of tensors"
    return [S.bits(o).clone() for o in outs]


def _reset_guard_words():
    ops = _ops()
    ops.guard_flags(DEV).zero_()
    if ops.cls_loss_flags(DEV, create=False) is not None:
        ops.cls_loss_flags(DEV).zero_()


def run_procedure(make, call, decoy=None, record=None):
    """(reference bits, test-run bits, delay in ms) of one entry; record: a set that receives the dl_* symbols `call` reached."""
    from druglamp_amd import _lib
    real = make(torch.Generator().manual_seed(1))
    fake = (decoy or make)(torch.Generator().manual_seed(2))
    assert set(real) == set(fake)
    for k in real:
        assert real[k].shape == fake[k].shape and real[k].dtype == fake[k].dtype, k
        if not real[k].is_floating_point():
            assert torch.equal(real[k], fake[k]), "%s: index / label / length / table tensors are the same in both draws" % k
    assert any(real[k].is_floating_point() and not torch.equal(real[k], fake[k]) for k in real) or \
        all(not v.is_floating_point() for v in real.values()), "the decoy differs in no payload"
    torch.cuda.synchronize()
    # reference: the default stream
    _reset_guard_words()
    ref_out = call(_clone(real))
    torch.cuda.synchronize()
    ref = _out_bits(ref_out)
    plain_ms = S.measure_ms(lambda: call(_clone(real)))
    d = S.delay_for(plain_ms)
    # test run: a fresh stream held back by d; the real inputs arrive behind the delay
    _reset_guard_words()
    work = _clone(fake)
    torch.cuda.synchronize()
    side = S.side_streams(1)[0]                      # a fresh stream that runs beside the default one
    real_lib = _lib.lib()
    rec = _Recorder(real_lib)
    try:
        if record is not None:
            _lib._lib = rec
        with torch.cuda.stream(side):
            S.skew(side, d)
            for k in work:
                work[k].copy_(real[k])
            got_out = call(work)
    finally:
        _lib._lib = real_lib
    torch.cuda.synchronize()
    if record is not None:
        record.update(rec.seen)
    got = _out_bits(got_out)
    del ref_out
    _reset_guard_words()
    return ref, got, d


def _equal(ref, got):
    return len(ref) == len(got) and all(a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(ref, got))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_wrapper_launches_only_on_the_current_stream(c):
    seen = set()
    ref, got, d = run_procedure(c.make, c.call, c.decoy, record=seen)
    reached = seen & set(stream_symbols())
    assert reached == set(c.reaches), "%s reaches %s, declared %s" % (c.name, sorted(reached), sorted(c.reaches))
    bad = [i for i, (a, b) in enumerate(zip(ref, got)) if not torch.equal(a, b)]
    assert _equal(ref, got), ("%s: outputs %s differ from the default-stream run when the call is made on a side stream held back "
                              "by %.1f ms behind the copies of its inputs: a launch went to another stream" % (c.name, bad, d))


@pytest.mark.gpu
def test_the_procedure_detects_an_off_stream_launch():
    """The harness's own detection power: a "wrapper" that computes y = 2 x on the DEFAULT stream, whatever the current one,
    must come out unequal — and the same computation on the current stream equal."""
    make = lambda g: {"x": R(g, 4096)}                                                      # noqa: E731

    def off_stream(t):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return (t["x"] * 2,)
    ref, got, _ = run_procedure(make, off_stream)
    assert not _equal(ref, got)
    ref, got, _ = run_procedure(make, lambda t: (t["x"] * 2,))
    assert _equal(ref, got)


@pytest.mark.gpu
def test_scratch_is_per_device_and_stream_and_private_under_capture():
    ops = _ops()
    n = 4096
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a, a2 = ops._ws.get(n, DEV), ops._ws.get(n, DEV)
    with torch.cuda.stream(s2):
        b = ops._ws.get(n, DEV)
    assert a.data_ptr() == a2.data_ptr() and a.untyped_storage().data_ptr() == a2.untyped_storage().data_ptr()
    assert a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()
    assert ops._ws.get(n, DEV).untyped_storage().data_ptr() not in (a.untyped_storage().data_ptr(), b.untyped_storage().data_ptr())
    # under capture: a fresh tensor from the graph's own pool, never the shared buffer (a minimal capture of one ops.cast)
    x = torch.randn(1000, device=DEV)
    ops.cast(x, BF16)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    taken = []
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        assert torch.cuda.is_current_stream_capturing()
        taken.append(ops._ws.get(n, DEV))
        taken.append(ops._ws.get(n, DEV))
        y = ops.cast(x, BF16)
    shared = {buf.untyped_storage().data_ptr() for buf in ops._ws.bufs.values()}
    assert taken[0].data_ptr() != taken[1].data_ptr()
    assert taken[0].data_ptr() not in shared and taken[1].data_ptr() not in shared
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, x.to(BF16))


def test_every_stream_taking_symbol_is_reached_by_an_entry():
    """No GPU needed: the static `reaches` declarations (which the GPU test checks against the calls it records) cover every
    stream-taking symbol of the signature table; EXEMPT is for profiling hooks and workspace-size queries only."""
    from druglamp_amd import _lib
    syms = set(stream_symbols())
    assert len(syms) >= 75 and "dl_gemm" in syms and "dl_version" not in syms and "dl_gemm_workspace_bytes" not in syms
    assert all(isinstance(_lib.SIGNATURES[n][1][-1], type) and _lib.SIGNATURES[n][1][-1] is ctypes.c_void_p for n in syms)
    declared = set()
    for c in CASES:
        assert c.reaches and set(c.reaches) <= syms, "%s declares %s: not stream-taking symbols" % (c.name, sorted(set(c.reaches) - syms))
        declared |= set(c.reaches)
    assert len({c.name for c in CASES}) == len(CASES)
    for name, why in EXEMPT.items():
        assert name in syms and name not in declared and isinstance(why, str) and why
        assert name.startswith("dl_prof_") or name.endswith("_bytes") or name.endswith("_floats"), "%s: only hooks and size queries" % name
    missing = sorted(syms - declared - set(EXEMPT))
    assert not missing, "stream-taking symbols no CASES entry reaches: %s" % missing
