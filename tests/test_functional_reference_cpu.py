"""No GPU: the fp64 formulations of tests/fn_ref.py against torch.nn modules and the oracle (1e-12 in fp64), the data
conditions of every case of tests/test_functional_paths_gpu.py (dropout replica, ReLU near zero, zero padding columns), the
FORMS table against the case lists, and the checker on planted wiring errors."""
import collections
import importlib
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import druglamp_oracle as O
from tests import elem_ref as er
from tests import fn_ref as R

F64 = torch.float64
TOL = 1e-12


@pytest.fixture(scope="module")
def refs():
    """name -> (data, fp64 reference, plain evaluation, fp64 Ctx), computed once for every case."""
    out = collections.OrderedDict()
    for c in R.CASES:
        d = R.build(c)
        out[c.name] = (d,) + R.reference(c, d)
    return out


def _close(a, b, what):
    a, b = a.detach(), b.detach()
    err = float((a.double() - b.double()).abs().max())
    assert a.shape == b.shape and err <= TOL * max(1.0, float(b.abs().max())), "%s: %g" % (what, err)


# ---- the formulations against torch.nn / the oracle ----------------------------------------------------------------------------
def _block_sd(T, paired):
    """The oracle's key names for one block: stream 0 is the protein stream, stream 1 the molecule stream."""
    sd = {}
    for s, suf in ((0, ""), (1, "_mol")) if paired else ((0, ""),):
        names = {"ln1": "attention_norm" if s == 0 else "att_norm_mol", "q": "attn.query" + suf, "k": "attn.key" + suf, "v": "attn.value" + suf,
                 "fc": "attn.fc" + suf, "out": "attn.out" + suf, "ln2": "ffn_norm" + suf, "fc1": "ffn%s.fc1" % suf, "fc2": "ffn%s.fc2" % suf}
        for p in R.BLOCK_PARAMS[paired]:
            sd["L.%s.weight" % names[p]] = T["s%d.%s.w" % (s, p)]
            sd["L.%s.bias" % names[p]] = T["s%d.%s.b" % (s, p)]
    return sd


@pytest.mark.parametrize("name", ["block_paired_f32", "block_paired_drop_bf16", "block_self_f32", "block_self_drop_f32"])
def test_block_formulation_is_the_oracles_block(name):
    c = R.BY_NAME[name]
    d = R.build(c)
    T = R.leaves_at(d, F64, c.dt)
    got = R.ref_block(c, T, R.Ctx(F64))["y"]
    k = c.cfg
    S, B, L, dm = T["x"].shape
    sd = _block_sd(T, k["paired"])
    p = k.get("p", 0.0)
    m = [R.drop_mask(s_, B * L, w, p).reshape(B, L, w) for s_, w in zip(R.seeds(R.SEED0, 2 * S), (4 * dm, dm) * S)] if p > 0 else [None] * (2 * S)
    if k["paired"]:
        prot, mol = T["x"][0], T["x"][1]
        ap, am, _, _ = O.pmma_attention_paired(sd, "L.attn", O._ln(sd, "L.attention_norm", prot, 1e-6), O._ln(sd, "L.att_norm_mol", mol, 1e-6), k["H"])
        prot, mol = ap + prot, am + mol
        prot = O._mlp(sd, "L.ffn", O._ln(sd, "L.ffn_norm", prot, 1e-6), m[0], m[1]) + prot
        mol = O._mlp(sd, "L.ffn_mol", O._ln(sd, "L.ffn_norm_mol", mol, 1e-6), m[2], m[3]) + mol
        want = torch.stack((prot, mol))
    else:
        x = T["x"][0]
        a, _ = O.pmma_attention_self(sd, "L.attn", O._ln(sd, "L.attention_norm", x, 1e-6), k["H"])
        x = a + x
        want = (O._mlp(sd, "L.ffn", O._ln(sd, "L.ffn_norm", x, 1e-6), m[0], m[1]) + x)[None]
    _close(got, want, name)


@pytest.mark.parametrize("name", ["pgca_raw_h1_f32", "pgca_probs_h4_bf16", "pgca_tail_w5_f32", "pgca_tail_w5_probs_h2_bf16"])
def test_pgca_formulation_is_the_oracles_and_a_tail_row_sums_its_copies(name):
    c = R.BY_NAME[name]
    d = R.build(c)
    T = R.leaves_at(d, F64, c.dt)
    out = R.ref_pgca(c, T, R.Ctx(F64))
    k = c.cfg
    key = T["k"].detach()
    if k.get("tail"):
        rows, w = k["tail"]
        key = torch.cat((key[:, :-rows], key[:, -rows:].repeat(1, w, 1)), dim=1).requires_grad_(True)
    sd = {"p.in_proj_weight": T["in_w"], "p.in_proj_bias": T["in_b"], "p.out_proj.weight": T["out_w"], "p.out_proj.bias": T["out_b"]}
    y, raw = O.pgca_forward(sd, "p", T["q"].permute(1, 0, 2), key.permute(1, 0, 2), k["H"])
    _close(out["y"], y, name + " y")
    if k["second"] == "raw":
        _close(out["raw"], raw, name + " raw")
    if k["second"] == "probs":
        _close(out["probs"], torch.softmax(raw, -1).mean(1), name + " probs")
    if k.get("tail"):
        dy = d.dy["y"][0].double()
        gk, = torch.autograd.grad(out["y"], T["k"], dy, retain_graph=True)
        gfull, = torch.autograd.grad(y, key, dy)
        lead = T["k"].shape[1] - rows
        _close(gk[:, :lead], gfull[:, :lead], name + " lead rows")
        _close(gk[:, lead:], gfull[:, lead:].reshape(k["B"], w, rows, -1).sum(1), name + " tail rows = sums over their copies")


def test_gate_formulation_is_the_oracles_mhla():
    for name in ("gate_h8_res_f32", "gate_h24_nores_bf16"):
        c = R.BY_NAME[name]
        T = R.leaves_at(R.build(c), F64, c.dt)
        sd = {"m.lin1.weight": T["lin1.w"], "m.lin1.bias": T["lin1.b"], "m.lin2.weight": T["lin2.w"], "m.lin2.bias": T["lin2.b"]}
        want = O.mhla_forward(sd, "m", T["v"], c.cfg["H"])
        _close(R.ref_gate(c, T, R.Ctx(F64))["y"], want + T["v"] if c.cfg["res"] else want, name)


def test_small_formulations_against_torch_nn_and_the_kernel_references():
    c = R.BY_NAME["sitepool_bf16"]
    T = R.leaves_at(R.build(c), F64, c.dt)
    _close(R.ref_sitepool(c, T, None)["y"].reshape(3, -1), er.sitepool_fwd(T["x"].detach(), 9)[0], "sitepool against the index form")
    c = R.BY_NAME["fillpool_to_bf16_f32"]
    T = R.leaves_at(R.build(c), F64, c.dt)
    fill, pooled, _, _, _ = er.fill_pool(T["x"].detach(), 9)
    out = R.ref_fillpool(c, T, None)
    _close(out["fill"], fill, "fill")
    _close(out["pooled"], pooled, "pooled")
    assert float(fill.sum()) == 3 * 3
    c = R.BY_NAME["graphagg_n130_f32"]
    T = R.leaves_at(R.build(c), F64, c.dt)
    _close(R.ref_graphagg(c, T, None)["y"], er.graph_aggregate(T["ahat"], T["feat"].detach(), 130, False)[0], "graph aggregate")
    c = R.BY_NAME["dense_k641_n100_gelu_f32"]
    T = R.leaves_at(R.build(c), F64, c.dt)
    lin = torch.nn.Linear(641, 100).double()
    with torch.no_grad():
        lin.weight.copy_(T["weight"])
        lin.bias.copy_(T["bias"])
    y = R.ref_dense(c, T, R.Ctx(F64))["y"]
    _close(y[..., :100], torch.nn.GELU()(lin(T["x"][..., :641])), "dense")
    assert y.shape[-1] == 104 and float(y[..., 100:].detach().abs().max()) == 0
    c = R.BY_NAME["ln_token_mean_f32"]
    T = R.leaves_at(R.build(c), F64, c.dt)
    ln = torch.nn.LayerNorm(128, eps=1e-5).double()
    with torch.no_grad():
        ln.weight.copy_(T["ln.w"])
        ln.bias.copy_(T["ln.b"])
    _close(R.ref_layernorm(c, T, None)["m"], ln(T["x"]).mean(1), "layer norm + token mean")
    c = R.BY_NAME["expandtail_f32"]
    T = R.leaves_at(R.build(c), F64, c.dt)
    y = R.ref_expandtail(c, T, None)["y"]
    for j in range(5 * 8):                                   # ExpandTailFn's contract: row lead + j is tail row j % tail
        assert torch.equal(y[:, 19 + j], T["x"][:, 19 + j % 8])


@pytest.mark.parametrize("name", ["cnn_train_raw_dx_f32", "cnn_eval_compact_bf16", "cnn_train_pooled_bf16", "cnn_train_compact_pool_bf16"])
def test_cnn_formulation_is_the_oracles_protein_cnn(name):
    from druglamp_amd.protein_plan import ProteinPlan
    c = R.BY_NAME[name]
    T = R.leaves_at(R.build(c), F64, c.dt)
    k = c.cfg
    B, S, C = k["B"], k["S"], k["C"]
    out = R.ref_cnn(c, T, R.Ctx(F64))
    sd = {"p.embedding.weight": T["emb"]} if "emb" in T else {}
    for i in range(3):
        sd.update({"p.conv%d.weight" % (i + 1): T["conv%d.w" % i], "p.conv%d.bias" % (i + 1): T["conv%d.b" % i], "p.bn%d.weight" % (i + 1): T["bn%d.w" % i],
                   "p.bn%d.bias" % (i + 1): T["bn%d.b" % i], "p.bn%d.running_mean" % (i + 1): T["bn%d.rm" % i], "p.bn%d.running_var" % (i + 1): T["bn%d.rv" % i]})
    if "emb" in T:
        assert float(T["emb"][0].detach().abs().max()) > 0             # (the oracle's F.embedding(padding_idx=0) reads row 0 like any other)
        want = O.protein_cnn(sd, "p", T["ids"], T["fill"], k["training"])          # the (B, C, S) buffer viewed as (B, S, C)
    else:
        v = T["x"].transpose(1, 2)
        for i in (1, 2, 3):
            v = O._bn(sd, "p.bn%d" % i, F.relu(F.conv1d(v, sd["p.conv%d.weight" % i], sd["p.conv%d.bias" % i], padding="same")), k["training"])
        want = v.reshape(B, S, C)
    if k["layout"] in ("pooled", "compact_pool"):
        sl = k["site_len"]
        _close(out["y"], want.view(B, sl, S // sl, C).mean(dim=1), name)                  # model_forward's pooling (DrugLAMP.py:35-37)
    else:
        _close(out["y"].reshape(B, S, C), want.reshape(B, C, S).transpose(1, 2), name)
    if "ids" in T:                                          # the data is what the compact plan claims: periodic, zeros behind
        plan = ProteinPlan(k["lengths"][:B], S, bucket=8)
        assert plan.rows < B * S and all(p > 0 for p in plan.period)        # every sample takes the segment layout
        ids = T["ids"]
        for b, L in enumerate(k["lengths"][:B]):
            P, E = L + 2, (S // (L + 2)) * (L + 2)
            assert torch.equal(ids[b, P:E], ids[b, :E - P]) and int(ids[b, E:].abs().sum()) == 0 and E < S


@pytest.mark.parametrize("name", ["mlp_train_f32", "mlp_tail_train_bf16", "mlp_tail_eval_f32", "mlp_eval_frozen_bf16"])
def test_mlp_formulation_is_torch_nn_on_the_expanded_rows(name):
    import torch.nn as nn
    c = R.BY_NAME[name]
    k = c.cfg
    T = R.leaves_at(R.build(c), F64, c.dt)
    seq = nn.Sequential(nn.Linear(k["K"], k["N1"]), nn.BatchNorm1d(k["N1"]), nn.ReLU(), nn.Linear(k["N1"], k["N2"], bias=False), nn.BatchNorm1d(k["N2"])).double()
    with torch.no_grad():
        seq[0].weight.copy_(T["l0.w"]), seq[0].bias.copy_(T["l0.b"]), seq[3].weight.copy_(T["l1.w"])
        for i, m in ((0, seq[1]), (1, seq[4])):
            m.weight.copy_(T["bn%d.w" % i]), m.bias.copy_(T["bn%d.b" % i]), m.running_mean.copy_(T["bn%d.rm" % i]), m.running_var.copy_(T["bn%d.rv" % i])
    seq.train(k["training"])
    idx, mult = R.mlp_rows(c)
    assert int(mult.sum()) == idx.numel() and torch.equal(torch.bincount(idx).double(), mult)
    want = seq(T["x"].detach()[idx])
    got = R.ref_mlp(c, T, R.Ctx(F64))["y"]
    _close(got[idx], want, name)                             # every copy carries its representative's output
    if k.get("tail"):
        assert idx.numel() == k["B"] * (19 + 5 * 8) and k["N2"] % 8 != 0


def test_seed_replica_is_the_generator_of_ops():
    from druglamp_amd import ops
    ops.manual_seed(R.SEED0)
    assert [ops.next_seed() for _ in range(4)] == R.seeds(R.SEED0, 4)
    ops.manual_seed(0x5EED)


# ---- data conditions ----------------------------------------------------------------------------------------------------------
def test_data_conditions_of_every_case(refs):
    for c in R.CASES:
        d, ref, plain, ctx = refs[c.name]
        k = c.cfg
        for name, share in ctx.share.items():               # ReLU near zero: the share resolved by the kernel's own choice is capped
            assert share <= R.RELU_CAP[c.dt], "%s: %.3g of %s within rounding of zero" % (c.name, share, name)
        assert (k.get("act") == "relu" or c.kind in ("cnn", "mlp")) == bool(ctx.share), c.name
        for key, t in ref.items():
            assert bool(torch.isfinite(t).all()) and t.dtype == F64, (c.name, key)
            assert tuple(plain[key].shape) == tuple(t.shape), (c.name, key)
            if key.startswith("grad:") and key not in ("grad:s0.k.b", "grad:s1.k.b"):
                assert float(t.abs().max()) > 0, "%s: %s is identically zero: the case does not reach it" % (c.name, key)
        if c.kind == "dense":
            assert float(d.leaf["x"][0][..., k["K"]:].abs().sum()) == 0
            Np = (k["N"] + 7) // 8 * 8
            if "residual" not in d.leaf:
                assert float(ref["out:y"][..., k["N"]:].abs().sum()) == 0 and ref["out:y"].shape[-1] == Np
        if k.get("p", 0) > 0:                              # the masks drop about p of the elements, and not the same ones at both sites
            m = R.drop_mask(R.seeds(R.SEED0, 2)[0], 72, 64, k["p"])
            m2 = R.drop_mask(R.seeds(R.SEED0, 2)[1], 72, 64, k["p"])
            assert 0.05 < float((m == 0).double().mean()) < 0.15 and not torch.equal(m, m2)
            assert abs(float(m.max()) - 1 / (1 - k["p"])) < 1e-6
        if c.kind == "embedpad":
            dy = d.dy["y"][0].float()
            assert float(dy[:, :4].min()) >= 1e29 and float(dy[:, -4:].max()) <= -1e29 and float(ref["grad:weight"].abs().max()) < 1e3
        if c.kind == "embedrows":
            src, dy = d.leaf["src"][0], d.dy["y"][0].float()
            assert int((src < 0).sum()) >= 8 * k["B"] and float(dy[src < 0].abs().min()) >= 1e29 and float(ref["grad:emb"].abs().max()) < 1e3
            assert float(ref["out:y"][src < 0].abs().max()) == 0
        if c.kind in ("embedding", "embedpad") and k.get("padding_idx") is not None:
            assert float(ref["grad:weight"][k["padding_idx"]].abs().max()) == 0 and bool((d.leaf["ids"][0] == k["padding_idx"]).any())
        if c.kind == "embedding":
            assert d.leaf["ids"][0].unique().numel() < d.leaf["ids"][0].numel()      # repeated ids


def test_analytically_zero_gradients_are_noise_in_both_evaluations(refs):
    """The key-projection bias of a softmax attention has no gradient: the reference gives ~1e-17, the plain evaluation its
    own rounding noise — the envelope of such a tensor is that noise, no special rule."""
    d, ref, plain, _ = refs["block_paired_f32"]
    assert float(ref["grad:s0.k.b"].abs().max()) < 1e-12 * float(ref["grad:s0.v.b"].abs().max())
    assert float(R.envelope(plain["grad:s0.k.b"], ref["grad:s0.k.b"]).max()) > 0


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_forms_table_and_case_lists_agree():
    from tests import test_functional_paths_gpu as G
    named = set()
    for c in list(R.CASES) + list(G.CAST_CASES):
        assert c.forms, c.name
        for f in c.forms:
            assert f in R.FORMS, "%s names the unknown form %r" % (c.name, f)
            named.add(f)
    assert not named & set(R.ELSEWHERE) and not named & set(R.OPEN) and not set(R.ELSEWHERE) & set(R.OPEN)
    assert named | set(R.ELSEWHERE) | set(R.OPEN) == set(R.FORMS), (named | set(R.ELSEWHERE) | set(R.OPEN)) ^ set(R.FORMS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for form, tests in R.ELSEWHERE.items():
        for t in tests:
            mod, fn = t.split("::")
            src = open(os.path.join(root, mod.replace(".", os.sep) + ".py")).read()
            assert re.search(r"^def %s\(" % re.escape(fn), src, re.M), "%s: %s does not exist" % (form, t)
    # every Function class of functional.py appears in the table
    Fn = importlib.import_module("druglamp_amd.functional")
    for name, obj in vars(Fn).items():
        if isinstance(obj, type) and issubclass(obj, torch.autograd.Function) and obj is not torch.autograd.Function:
            assert any(f == name or f.startswith(name + " ") for f in R.FORMS), name
    # the branch a case claims is the one its shape selects
    for c in R.CASES:
        k = c.cfg
        if c.kind == "linear" and k.get("want", ("x",)).count("x"):
            assert ("LinearFn wT" in c.forms) == (c.dt == R.BF and k["N"] % 8 == 0), c.name
        if c.kind == "gate":
            assert ("TokenGateFn gate_dpre" in c.forms) == (k["H"] == 8 and k["dd"] % 8 == 0)
            assert ("TokenGateFn padded image" in c.forms) == (k["H"] != 8 and c.dt == R.BF and k["dd"] % 8 == 0)
        if c.kind == "dense":
            assert ("DenseFn padded N" in c.forms) == (k["N"] % 8 != 0) and ("DenseFn padded K" in c.forms) == (k["Kp"] != k["K"])
        if c.kind == "graphagg":
            assert ("GraphAggregateFn n<=128" in c.forms) == (k["n"] <= 128)
        if c.kind == "embedding":
            assert ("EmbeddingFn padded" in c.forms) == (k["D"] % 8 != 0)
        if c.kind == "layernorm":
            assert ("LayerNormFn dy_share" in c.forms) == (k["mode"] == "mean" and k["L"] > 1)
    per_fn = collections.defaultdict(set)
    for c in R.CASES:
        lay = c.cfg.get("dy", "perm" if c.kind == "pgca" else "c")
        per_fn[c.kind].add("sliced" if c.cfg.get("mode") == "sliced" else lay)
    for kind, lays in per_fn.items():                       # at least one variant per Function takes a non-contiguous dy
        assert lays - {"c"}, "%s: no case with a non-contiguous dy" % kind


# ---- the checker on planted errors ------------------------------------------------------------------------------------------------
def _as_got(c, plain):
    return collections.OrderedDict((k, v.clone()) for k, v in plain.items())


def test_checker_passes_the_plain_evaluation_and_fails_planted_wiring_errors(refs):
    for name in ("dense_t_sq128_relu_bf16", "block_paired_bf16", "block_paired_f32", "pgca_tail_w5_bf16", "concat2_f32"):
        d, ref, plain, _ = refs[name]
        R.check_case(R.BY_NAME[name], _as_got(R.BY_NAME[name], plain), ref, plain)          # an untouched copy passes
    # 1. a square weight gradient without its transpose: same norm, same values
    c = R.BY_NAME["dense_t_sq128_relu_bf16"]
    d, ref, plain, _ = refs[c.name]
    got = _as_got(c, plain)
    got["grad:weight"] = got["grad:weight"].t().contiguous()
    with pytest.raises(AssertionError, match="grad:weight"):
        R.check_case(c, got, ref, plain)
    # 2. the k and v slices of the fused qkv bias gradient swapped
    for name in ("block_paired_bf16", "block_paired_f32"):
        c = R.BY_NAME[name]
        d, ref, plain, _ = refs[name]
        got = _as_got(c, plain)
        got["grad:s1.k.b"], got["grad:s1.v.b"] = got["grad:s1.v.b"], got["grad:s1.k.b"]
        with pytest.raises(AssertionError, match=r"grad:s1\.k\.b"):
            R.check_case(c, got, ref, plain)
    # 3. one wrong tail row: the last representative row's gradient not summed over its 5 copies
    c = R.BY_NAME["pgca_tail_w5_bf16"]
    d, ref, plain, _ = refs[c.name]
    got = _as_got(c, plain)
    got["grad:k"][-1, -1] = (got["grad:k"][-1, -1].float() / 5).to(got["grad:k"].dtype)
    with pytest.raises(AssertionError, match="grad:k: "):
        R.check_case(c, got, ref, plain)
    # 4. a data mover off by one bf16 ulp in one element
    c = R.BY_NAME["concat2_f32"]
    d, ref, plain, _ = refs[c.name]
    got = _as_got(c, plain)
    got["out:y"][1, 2, 3] *= 1 + 2.0 ** -23
    with pytest.raises(AssertionError, match="data mover"):
        R.check_case(c, got, ref, plain)


def test_envelope_rows_and_floor():
    ref = torch.zeros(4, 3, dtype=F64)
    plain = torch.tensor([[1.0, 0, 0], [0, 0, 0], [0, 2.0, 0], [0, 0, 4.0]])
    E = R.envelope(plain, ref)
    assert E.shape == ref.shape and E[0].tolist() == [1, 1, 1] and E[3].tolist() == [4, 4, 4]
    assert E[1].tolist() == [1, 1, 1]                      # the lucky row is floored by the (lower) median of the row maxima
    assert R.envelope(torch.tensor([1.0, 3.0]), torch.zeros(2, dtype=F64)).tolist() == [3, 3]      # a 1-d tensor is one row
