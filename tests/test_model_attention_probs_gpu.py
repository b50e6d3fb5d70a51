"""Whole model with keep_attention_probs: both PGCA blocks hand back their softmax weights (B, 256, 512) instead of the raw
logits — from the full-key call without hints, from the compact-key call (block + 8 distinct drug rows, map expanded to the
512 rows) with the hints that enable the compact drug forms.  fp32 DrugLAMP in eval, the golden model of test_model_gpu.py."""
import pytest
import torch

from tests.helpers import load, relerr
from tests.test_model_gpu import DEV, build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs():
    """One model, one batch, three eval forwards: default, with the maps, with the maps and the compact-form hints."""
    import druglamp_amd.ops as ops_mod
    from druglamp_amd.protein_plan import BatchHints
    from druglamp_amd.synthetic import make_batch
    from druglamp_amd.trainer import Trainer
    m, _ = build("DrugLAMP", load("model_DrugLAMP"))
    m.eval()
    batch, meta = make_batch(4, DEV, seed=11, with_graph=True, llm_dtype=torch.float32)
    feat_d, feat_p, _labels, llm_d, llm_p = batch
    hints = Trainer.padding_hints_of(meta, batch)
    out = {"m": m, "B": 4}
    real = ops_mod.attn_probs

    def forward(name, h):
        seen = []
        ops_mod.attn_probs = lambda *a, **k: (seen.append((k["Lk"], k.get("key_tail"), k.get("head_mean"))), real(*a, **k))[1]
        try:
            with torch.no_grad():
                score = m(feat_d, feat_p, llm_d, llm_p, hints=h)[-1]
        finally:
            ops_mod.attn_probs = real
        out[name] = {"score": score.clone(), "calls": seen,
                     "A": (m.A_v_gca, m.A_x_gca), "P_raw": (m.P_v_gca, m.P_x_gca),
                     "P": None if m.P_v_gca is None else (m.get_cross_attn_prob("v"), m.get_cross_attn_prob("x"))}

    forward("default", None)
    m.keep_attention_probs = True
    forward("probs", None)
    m.drug_extractor.compact_min_rows = 0             # (a batch of 4: take the compact MolecularGCN form anyway)
    forward("probs_hints", BatchHints(**hints))
    out["blk"] = hints["drug_tokens"]
    return out


def test_default_keeps_the_raw_logits_and_no_map(runs):
    d = runs["default"]
    assert d["P_raw"] == (None, None) and d["calls"] == []
    assert all(a is not None and tuple(a.shape) == (runs["B"], 1, 256, 512) for a in d["A"])
    with pytest.raises(RuntimeError):
        m = runs["m"]
        keep, m.P_v_gca = m.P_v_gca, None
        try:
            m.get_cross_attn_prob("v")
        finally:
            m.P_v_gca = keep


def test_maps_without_hints(runs):
    d, p = runs["default"], runs["probs"]
    assert p["A"] == (None, None)
    assert p["calls"] == [(512, None, True), (512, None, True)]
    assert torch.equal(p["score"], d["score"])
    for got, raw in zip(p["P"], d["A"]):
        assert tuple(got.shape) == (runs["B"], 256, 512) and got.device.type == "cpu" and got.dtype == torch.float32
        assert float((got.double().sum(-1) - 1).abs().max()) <= 1e-5
        assert relerr(got, torch.softmax(raw.double(), -1)[:, 0]) <= 1e-4


def test_maps_from_the_compact_key_forms(runs):
    p, c = runs["probs"], runs["probs_hints"]
    assert c["A"] == (None, None)
    blk = runs["blk"]
    assert sorted(c["calls"]) == sorted([(128 + 8, (8, 48), True), (blk + 8, (8, (512 - blk) // 8), True)]), c["calls"]
    for got, full in zip(c["P"], p["P"]):
        assert tuple(got.shape) == (runs["B"], 256, 512)
        assert float((got.double().sum(-1) - 1).abs().max()) <= 1e-5
        assert relerr(got, full) <= 1e-4
    assert relerr(c["score"], p["score"]) <= 1e-4
