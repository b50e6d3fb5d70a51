"""Parameter groups without a GPU: the fp64 oracle of the grouped AdamW kernel (tests/param_groups_ref.py) against
torch.optim.AdamW in fp64 with real param_groups, and the host logic of druglamp_amd.param_groups on the real DrugLAMP model.

The oracle comparison: both sides are fp64 and receive the same fp32-rounded scalars; they differ in operation order only
(torch: lerp, addcmul, addcdiv).  The bar is 1e-12 relative to the tensor's largest magnitude: an element of exp_avg is a sum of
two terms of either sign, and relative to ITSELF an element that cancels to 1e-4 of its terms is at 1e-16 / 1e-4 already."""
import numpy as np
import pytest
import torch

from tests import param_groups_ref as pr


def _model():
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    torch.manual_seed(11)
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    return MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640)


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.mark.parametrize("guard", [None, (0.37, 5.0, 0.0, 0.0)], ids=["noguard", "guard"])
def test_the_oracle_agrees_with_torch_adamw_in_fp64_with_real_param_groups(guard):
    n = 1003
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    tab = [(1.0, 1e-2), (0.1, 0.0), (0.0, 1e-2), (3.0, 0.5)]
    quads = [(c % 4) if c < 64 else (1 if c < 128 else (3 if c < 200 else 0)) for c in range((n + 3) // 4)]
    lr, b1, b2, eps, gscale = 1e-3, 0.9, 0.999, 1e-8, 0.5
    segs = pr.segments(quads, n)
    vals = pr.group_values(tab, lr)
    eff = float(np.float32(gscale) * np.float32(guard[0])) if guard is not None else pr.f32(gscale)
    tp = [torch.nn.Parameter(p0[s:e].clone()) for s, e, _ in segs]
    opt = torch.optim.AdamW([{"params": [q], "lr": vals[k][0], "weight_decay": vals[k][1]} for q, (_, _, k) in zip(tp, segs)],
                            lr=1.0, betas=(pr.f32(b1), pr.f32(b2)), eps=pr.f32(eps), weight_decay=7.0)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * 3
        p, m, v = pr.adamw_groups(p, g, m, v, quads, tab, lr, b1, b2, eps, step, gscale, guard)
        for q, (s, e, _) in zip(tp, segs):
            q.grad = g[s:e] * eff
        opt.step()
        tm = torch.cat([opt.state[q]["exp_avg"] for q in tp])
        tv = torch.cat([opt.state[q]["exp_avg_sq"] for q in tp])
        for name, a, b in (("param", p, torch.cat([q.detach() for q in tp])), ("exp_avg", m, tm), ("exp_avg_sq", v, tv)):
            err = float((a - b).abs().max() / b.abs().max())
            print("step %d %-10s max |oracle - torch| / max |torch| = %.3e" % (step, name, err))
            assert err <= 1e-12, (step, name, err)
    assert float((p - p0).abs().max()) > 1e-4                 # (the steps moved the parameters)


def test_the_oracle_leaves_out_of_range_chunks_and_skipped_steps_alone():
    n = 10
    p = torch.arange(1.0, n + 1, dtype=torch.float64)
    g, m, v = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    q, _, _ = pr.adamw_groups(p, g, m, v, [0, 5, 0], [(1.0, 0.0)], 1e-2, 0.9, 0.999, 1e-8, 1, 1.0)
    assert torch.equal(q[4:8], p[4:8]) and bool((q[:4] != p[:4]).all()) and bool((q[8:] != p[8:]).all())
    q, m1, v1 = pr.adamw_groups(p, g, m, v, [0, 0, 0], [(1.0, 0.0)], 1e-2, 0.9, 0.999, 1e-8, 1, 1.0, guard=(0.0, float("nan"), 1.0, 0.0))
    assert torch.equal(q, p) and torch.equal(m1, m) and torch.equal(v1, v)


def _groups():
    from druglamp_amd.param_groups import ParamGroup
    return [ParamGroup("pcnn_convs", match=("protein_extractor.conv*.weight",), lr_scale=0.5),
            ParamGroup("no_decay", max_ndim=1, weight_decay=0.0),
            ParamGroup("encoders", match=("drug_extractor.*", "protein_extractor.*"), lr_scale=0.1),
            ParamGroup("adaptor", match=("p_adaptor_wo_skip_connect.lin?.weight",), frozen=True)]


def test_first_match_wins_and_max_ndim_selects_exactly_the_vectors(model):
    from druglamp_amd.param_groups import ParamGroup, ParamGroups
    pg = ParamGroups(model, _groups(), default_weight_decay=1e-2)
    named = dict(model.named_parameters())
    tab = pg.table()
    assert [n for _, n, _ in tab] == list(named) and all(num == named[n].numel() for _, n, num in tab)
    by = {n: g for g, n, _ in tab}
    # first match wins: the conv weights match "pcnn_convs" and "encoders" -> the earlier one; the encoders' biases and norm
    # weights match "no_decay" and "encoders" -> "no_decay"
    assert by["protein_extractor.conv1.weight"] == by["protein_extractor.conv3.weight"] == "pcnn_convs"
    assert by["protein_extractor.conv1.bias"] == by["protein_extractor.bn1.weight"] == by["drug_extractor.gnn.gnn_layers.0.bn_layer.bias"] == "no_decay"
    assert by["protein_extractor.embedding.weight"] == by["drug_extractor.init_transform.weight"] == "encoders"
    assert by["p_adaptor_wo_skip_connect.lin1.weight"] == "adaptor" and by["p_adaptor_wo_skip_connect.lin1.bias"] == "no_decay"
    assert by["mlp_classifier.fc1.weight"] == by["pmma.embeddings.pe_prot"] == "default"
    assert {n for n, g in by.items() if g == "no_decay"} == {n for n, p in named.items() if p.ndim <= 1}
    assert pg.rows == [(1.0, 1e-2), (0.5, 1e-2), (1.0, 0.0), (0.1, 1e-2), (1.0, 1e-2)] and pg.names[0] == "default"
    # the deduplicated names: the ProteinCNN the SSL head shares is matched as protein_extractor.*, and only so
    assert not any(n.startswith("ssl_model.extractor") for n in named)
    only = ParamGroups(model, [ParamGroup("pcnn", match=("protein_extractor.*",))], default_weight_decay=1e-2)
    assert {n for g, n, _ in only.table() if g == "pcnn"} == {n for n in named if n.startswith("protein_extractor.")}
    assert len([1 for g, _, _ in only.table() if g == "pcnn"]) == 13
    with pytest.raises(ValueError, match="no parameter ends up"):
        ParamGroups(model, [ParamGroup("shared", match=("ssl_model.extractor.*",))], default_weight_decay=1e-2)


def test_every_chunk_of_every_parameter_carries_its_group_padding_included():
    from druglamp_amd.param_groups import ParamGroups
    from druglamp_amd.trainer import FlatParams
    model = _model()                                     # (FlatParams rebinds the parameters' storage: a model of its own)
    pg = ParamGroups(model, _groups(), default_weight_decay=1e-2)
    pg.freeze()
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert frozen == ["p_adaptor_wo_skip_connect.lin1.weight", "p_adaptor_wo_skip_connect.lin2.weight"]
    flat = FlatParams(list(model.parameters()))
    pg.build(flat)
    assert pg.quad_group.dtype == torch.uint8 and pg.quad_group.numel() == flat.numel // 4 and flat.numel % 4 == 0
    assert pg.group_tab.dtype == torch.float32 and tuple(pg.group_tab.shape) == (5, 2)
    assert pg.group_tab.tolist() == torch.tensor(pg.rows, dtype=torch.float32).tolist()
    by = {n: pg.names.index(g) for g, n, _ in pg.table()}
    padded = 0
    for (name, p), off in zip(model.named_parameters(), flat.offsets):
        chunks = (p.numel() + 3) // 4
        padded += p.numel() % 4 != 0
        got = pg.quad_group[off // 4:off // 4 + chunks]
        assert bool((got == by[name]).all()), name
    assert padded >= 3                                   # (75-, 127-, 641- and 385-wide matrices and the 1- and 27-element vectors)
    ends = [off + (p.numel() + 3) // 4 * 4 for p, off in zip(flat.params, flat.offsets)]
    assert ends[:-1] == flat.offsets[1:] and ends[-1] == flat.numel       # the chunks above cover the whole table
    # a runtime change rewrites one row, host and device
    pg.set("encoders", lr_scale=0.25)
    pg.set("default", weight_decay=0.0)
    assert pg.group_tab.tolist()[3] == [0.25, float(np.float32(1e-2))] and pg.group_tab.tolist()[0] == [1.0, 0.0]
    assert pg.values("encoders") == (0.25, 1e-2)
    with pytest.raises(ValueError, match="no group named"):
        pg.set("encoder", lr_scale=0.25)
    for bad in (-1.0, float("nan"), float("inf"), "0.1", True):
        with pytest.raises(ValueError, match="finite number >= 0"):
            pg.set("encoders", lr_scale=bad)
        with pytest.raises(ValueError, match="finite number >= 0"):
            pg.set("encoders", weight_decay=bad)
    assert pg.values("encoders") == (0.25, 1e-2)


def test_every_listed_value_error_is_raised(model):
    from druglamp_amd.param_groups import ParamGroup, ParamGroups
    ok = ParamGroup("a", match=("lin_d1.*",))
    cases = {
        "duplicate name": ([ok, ParamGroup("a", match=("lin_d2.*",))], "used twice"),
        "empty name": ([ParamGroup("", match=("lin_d1.*",))], "non-empty name"),
        "the name default": ([ParamGroup("default", match=("lin_d1.*",))], "reserved"),
        "negative lr_scale": ([ParamGroup("b", match=("lin_d1.*",), lr_scale=-0.5)], "lr_scale"),
        "nan lr_scale": ([ParamGroup("b", match=("lin_d1.*",), lr_scale=float("nan"))], "lr_scale"),
        "inf lr_scale": ([ParamGroup("b", match=("lin_d1.*",), lr_scale=float("inf"))], "lr_scale"),
        "negative weight_decay": ([ParamGroup("b", match=("lin_d1.*",), weight_decay=-1e-2)], "weight_decay"),
        "nan weight_decay": ([ParamGroup("b", match=("lin_d1.*",), weight_decay=float("nan"))], "weight_decay"),
        "inf weight_decay": ([ParamGroup("b", match=("lin_d1.*",), weight_decay=float("inf"))], "weight_decay"),
        "64 groups": ([ParamGroup("g%d" % i, match=("lin_d1.*",)) for i in range(64)], "at most 63"),
        "a typo": ([ok, ParamGroup("typo", match=("lin_dd1.*",))], "no parameter ends up in group\\(s\\) 'typo'"),
        "shadowed": ([ok, ParamGroup("late", match=("lin_d1.weight",))], "no parameter ends up in group\\(s\\) 'late'"),
        "selects nothing": ([ParamGroup("none")], "neither match patterns nor max_ndim"),
    }
    for what, (groups, msg) in cases.items():
        with pytest.raises(ValueError, match=msg):
            ParamGroups(model, groups, default_weight_decay=1e-2)
            pytest.fail(what)
    with pytest.raises(ValueError, match="default_weight_decay"):
        ParamGroups(model, [ok], default_weight_decay=-1.0)
    # 63 groups are fine (with "default": the 64 rows the kernel takes)
    names = [n for n, _ in model.named_parameters()][:63]
    pg = ParamGroups(model, [ParamGroup("g%d" % i, match=(n,)) for i, n in enumerate(names)], default_weight_decay=1e-2)
    assert len(pg.names) == 64
