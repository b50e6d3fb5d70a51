"""Shortlisted screening end to end: the cached cross-modality latents (encode_proteins / encode_drugs of DrugLAMP2C2P, the
library's resident copy) and Trainer.shortlist / screen_library(shortlist=) / shortlist_recall.

Seed-0 DrugLAMP2C2P, make_batch(8, seed=31, with_graph=False): 3 proteins x 8 drugs, the drugs encoded as two batches of
different key layouts (one under BatchHints(drug_tokens=128): its x branch is compact, so its latent comes from the compact
token mean).  Tolerances are the project's: fp32 1e-4 against the oracle, bf16 2e-2 against the model's own eval forward."""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NP, ND = 3, 8
KIND = "DrugLAMP2C2P"


def _model(kind, dtype, seed=0):
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    torch.manual_seed(seed)
    cfg = load_yaml_into(get_cfg_defaults(), kind)
    m = MInterface(kind, cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    m.set_compute_dtype(dtype)
    m.eval()
    return m, cfg


@functools.lru_cache(maxsize=None)
def _data():
    from druglamp_amd.synthetic import make_batch
    (vd, vp, y, xd, xp), _ = make_batch(ND, DEV, seed=31, with_graph=False)
    return vd, vp, y, xd, xp


def _hints():
    from druglamp_amd.protein_plan import BatchHints
    return BatchHints(drug_tokens=128, raw_attention=False)      # every molecule of make_batch has at most 128 tokens


def _batches(dt=torch.float32):
    vd, vp, _, xd, xp = _data()
    xd, xp = xd.to(dt), xp.to(dt)
    prots = [(vp[:2], xp[:2]), (vp[2:NP], xp[2:NP])]
    drugs = [(vd[:3], xd[:3]), (vd[3:], xd[3:])]
    return prots, drugs


def _codes(m, dt):
    prots, drugs = _batches(dt)
    from druglamp_amd.screening import ProteinCode
    pcode = ProteinCode.cat([m.encode_proteins(*b) for b in prots])
    return pcode, [m.encode_drugs(*drugs[0], _hints()), m.encode_drugs(*drugs[1])]


def _pairs():
    """Eight (drug i, protein i % 3) rows and id records in which every row is its own protein and its own drug."""
    di, pi = torch.arange(ND), torch.arange(ND) % NP
    meta = [{"Prot_ID": "p%d" % i, "Drug_ID": "d%d" % i, "Y": 1} for i in range(ND)]
    return di, pi, meta


@functools.lru_cache(maxsize=None)
def _setup():
    """fp32 trainer, library, protein / drug batches and the dense screen: built once, read only."""
    from druglamp_amd.trainer import Trainer
    m, cfg = _model(KIND, torch.float32)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=torch.float32)
    m.eval()
    prots, drugs = _batches()
    lib = tr.build_library(drugs, hints=[_hints(), None])
    dense = tr.screen_library(prots, lib, pair_batch=5)
    return m, tr, prots, lib, dense


def test_fp32_latents_equal_the_oracles():
    from oracle import druglamp_oracle as O
    m, _ = _model(KIND, torch.float32)
    vd, vp, _, xd, xp = _data()
    pcode, dcodes = _codes(m, torch.float32)
    assert dcodes[0].layout("x") == (136, 8, 48) and dcodes[1].layout("x") == (512, 0, 1)       # the two forms of the token mean
    plat, dlat = pcode.latent, torch.cat([c.latent for c in dcodes])
    assert plat.shape == (NP, 256) and dlat.shape == (ND, 256) and plat.dtype == dlat.dtype == torch.float32
    di, pi, meta = _pairs()
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        cm = O.model_forward(sd, KIND, vd[di].float().cpu(), vp[pi].cpu(), xd[di].float().cpu(), xp[pi].float().cpu())["cm"]
        _, pl, dl, _ = O.cm_forward(sd, "cm_model", cm["prot"], cm["aug_prot"], cm["drug"], cm["aug_drug"], meta, 0.5,
                                    bn_training=False, return_latents=True)
    ep, ed = float((plat.cpu() - pl[:NP]).abs().max()), float((dlat.cpu() - dl).abs().max())
    print("fp32 latents: max |protein - oracle| = %.3g, max |drug - oracle| = %.3g (tolerance 1e-4)" % (ep, ed))
    assert float((pl.norm(dim=1) - 1).abs().max()) < 1e-5 and float((dl[0] - dl[1]).abs().max()) > 1e-3     # unit rows, drugs differ
    assert ep <= 1e-4 and ed <= 1e-4


def test_bf16_latents_equal_the_models_eval_forward():
    from druglamp_amd.model.cross_modality import CMLabels
    m, _ = _model(KIND, torch.bfloat16)
    vd, vp, _, xd, xp = _data()
    pcode, dcodes = _codes(m, torch.bfloat16)
    di, pi, meta = _pairs()
    with torch.no_grad():
        _, _, _, cp, _ = m(vd[di], vp[pi], xd[di].bfloat16(), xp[pi].bfloat16())
        means = [cp[k].float().mean(dim=1) for k in ("prot", "aug_prot", "drug", "aug_drug")]
        pl, dl = m.cm_model.latents_from_means(*means, CMLabels(ND, DEV).fill(meta))
    plat, dlat = pcode.latent, torch.cat([c.latent for c in dcodes])
    assert plat.dtype == torch.float32 and dlat.dtype == torch.float32
    ep, ed = float((plat - pl[:NP].float()).abs().max()), float((dlat - dl.float()).abs().max())
    print("bf16 latents: max |protein - eval forward| = %.3g, max |drug - eval forward| = %.3g (tolerance 2e-2)" % (ep, ed))
    assert ep <= 2e-2 and ed <= 2e-2


def test_library_holds_the_latents_and_shortlist_is_latent_topk():
    from druglamp_amd import ops
    m, tr, prots, lib, _ = _setup()
    pcode, dcodes = _codes(m, torch.float32)
    assert lib.latent.shape == (ND, 256) and lib.latent.dtype == torch.float32 and lib.latent.is_cuda
    assert torch.equal(lib.latent, torch.cat([c.latent for c in dcodes]))
    sims, idx = tr.shortlist(prots, lib, 4)
    assert sims.shape == idx.shape == (NP, 4) and sims.dtype == torch.float32 and idx.dtype == torch.int64
    v, i = ops.latent_topk(pcode.latent, lib.latent, 4)
    assert torch.equal(sims, v) and torch.equal(idx, i)
    cos = pcode.latent.double() @ lib.latent.double().t()
    assert float((sims.double() - cos.gather(1, idx)).abs().max()) <= 2e-5
    assert torch.equal(idx, torch.topk(cos, 4, dim=1).indices) or float(torch.diff(torch.sort(cos, dim=1).values, dim=1).min()) <= 4e-5


def test_shortlist_of_the_whole_library_is_the_plain_top_k():
    """shortlist=D returns the indices of plain top_k, values within 1e-4.  First the premise that makes equal indices a
    fair demand beside a 1e-4 value tolerance: the neighbouring probabilities that decide the returned indices — a protein's
    ranks 1 .. k + 1, the cut included — differ by more than 2e-4.
    k = 1: the seed-0 weights are untrained and put a protein's eight probabilities within 1.4e-3 of each other (measured on the
    MI355X: 0.4909457 0.4902231 0.4901896 ... for protein 0; rank 1 leads rank 2 by 7.2e-4, 5.9e-4 and 5.7e-4, while further
    down fifteen of the 21 neighbouring gaps are below 2e-4, the smallest 2.53e-06), so only the best hit is determined beyond
    the tolerance.  An earlier form of this test demanded the premise of all eight ranks, also for k = 1, and failed there
    on data that the dense path of before this change produces.  Larger k: the next test, which needs no premise."""
    m, tr, prots, lib, dense = _setup()
    sv = torch.sort(dense, dim=1, descending=True).values
    print("dense screen: sorted probabilities per protein:\n%s" % "\n".join(" ".join("%.7f" % x for x in row) for row in sv.tolist()))
    k = 1
    gap = float((sv[:, :k] - sv[:, 1:k + 1]).min())
    print("dense screen: smallest gap between neighbouring probabilities among ranks 1 .. %d = %.3g" % (k + 1, gap))
    assert gap > 2e-4, "the ranking is ambiguous on this data"
    pv, pi = tr.screen_library(prots, lib, pair_batch=5, top_k=k)
    for pair_batch in (5, 256):
        v, i = tr.screen_library(prots, lib, pair_batch=pair_batch, top_k=k, shortlist=ND)
        assert v.shape == (NP, k) and i.dtype == torch.int64 and v.dtype == torch.float32
        assert torch.equal(i, pi), pair_batch
        err = float((v - pv).abs().max())
        assert err <= 1e-4, (pair_batch, err)


def test_shortlist_of_the_whole_library_agrees_with_the_plain_top_k_up_to_near_ties():
    """shortlist=D against plain top_k without the distinctness premise: with every drug on the shortlist the two paths score
    the same 24 pairs (in other chunks), so per protein the k values agree within 1e-4 rank by rank, every returned index
    carries a dense probability within 1e-4 of the value returned for it, and a drug whose dense probability is more than
    2e-4 above the k-th value cannot be missing (1e-4 for each path)."""
    m, tr, prots, lib, dense = _setup()
    for k in (1, 3, ND):
        pv, _ = tr.screen_library(prots, lib, pair_batch=5, top_k=k)
        for pair_batch in (5, 256):
            v, i = tr.screen_library(prots, lib, pair_batch=pair_batch, top_k=k, shortlist=ND)
            assert v.shape == (NP, k) and i.dtype == torch.int64 and v.dtype == torch.float32
            assert bool((v[:, :-1] >= v[:, 1:]).all())
            assert all(len(set(row)) == k for row in i.tolist())
            assert float((v - pv).abs().max()) <= 1e-4, (k, pair_batch)
            assert float((dense.gather(1, i) - v).abs().max()) <= 1e-4, (k, pair_batch)
            kept = torch.zeros_like(dense, dtype=torch.bool).scatter_(1, i, True)
            assert not bool(((dense > v[:, -1:] + 2e-4) & ~kept).any()), (k, pair_batch)


def test_shortlist_4_top_2_is_topk_of_the_dense_result_on_the_shortlist():
    m, tr, prots, lib, dense = _setup()
    _, cand = tr.shortlist(prots, lib, 4)
    tv, sel = torch.topk(dense.gather(1, cand), 2, dim=1)
    ti = cand.gather(1, sel)
    v, i = tr.screen_library(prots, lib, pair_batch=5, top_k=2, shortlist=4)
    assert torch.equal(i, ti) and float((v - tv).abs().max()) <= 1e-4
    assert bool((v[:, 0] >= v[:, 1]).all())


def test_shortlist_recall():
    m, tr, prots, lib, dense = _setup()
    r = tr.shortlist_recall(prots, lib, top_k=2, shortlist=ND)
    assert r["recall"] == 1.0 and torch.equal(r["per_protein"].cpu(), torch.ones(NP))
    r = tr.shortlist_recall(prots, lib, top_k=2, shortlist=4)
    full = tr.screen_library(prots, lib, top_k=2)[1]
    short = tr.screen_library(prots, lib, top_k=2, shortlist=4)[1]
    want = torch.tensor([len(set(full[p].tolist()) & set(short[p].tolist())) / 2.0 for p in range(NP)])
    assert r["per_protein"].shape == (NP,) and torch.equal(r["per_protein"].cpu(), want)
    assert 0.0 <= r["recall"] <= 1.0 and abs(r["recall"] - float(want.mean())) < 1e-6


def test_errors():
    from druglamp_amd.screening import DrugLibrary
    m, tr, prots, lib, _ = _setup()
    with pytest.raises(ValueError, match="top_k"):
        tr.screen_library(prots, lib, shortlist=4)
    with pytest.raises(ValueError, match="smaller than top_k"):
        tr.screen_library(prots, lib, top_k=5, shortlist=4)
    with pytest.raises(ValueError, match="shortlist"):
        tr.screen_library(prots, lib, top_k=2, shortlist=ND + 1)
    with pytest.raises(ValueError, match="shortlist"):
        tr.shortlist(prots, lib, ND + 1)
    with pytest.raises(ValueError, match="shortlist"):
        tr.shortlist(prots, lib, 0)
    big = types.SimpleNamespace(n=5000, latent=lib.latent)                  # only its size is looked at before the limit is
    with pytest.raises(ValueError, match="1024"):
        tr.screen_library(prots, big, top_k=2, shortlist=1025)
    with pytest.raises(ValueError, match="1024"):
        tr.shortlist(prots, big, 1025)
    bare = DrugLibrary(lib.branches, lib.dtype, lib.epoch, lib.fingerprint)
    with pytest.raises(RuntimeError, match="no latents"):
        tr.screen_library(prots, bare, top_k=2, shortlist=4)
    with pytest.raises(RuntimeError, match="no latents"):
        tr.shortlist(prots, bare, 4)


def test_a_saved_and_reloaded_library_gives_bit_equal_shortlists(tmp_path):
    from druglamp_amd.screening import DrugLibrary
    m, tr, prots, lib, _ = _setup()
    lib.save(tmp_path / "lib.pt")
    back = DrugLibrary.load(tmp_path / "lib.pt", m, DEV)
    assert torch.equal(back.latent, lib.latent) and back.latent.is_cuda
    a, b = tr.shortlist(prots, lib, 5), tr.shortlist(prots, back, 5)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    va, ia = tr.screen_library(prots, lib, top_k=2, shortlist=5)
    vb, ib = tr.screen_library(prots, back, top_k=2, shortlist=5)
    assert torch.equal(va, vb) and torch.equal(ia, ib)


def test_bf16_library_latents_are_rounded_once_and_shortlists_run():
    from druglamp_amd import ops
    from druglamp_amd.trainer import Trainer
    m, cfg = _model(KIND, torch.bfloat16)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=torch.bfloat16)
    m.eval()
    prots, drugs = _batches(torch.bfloat16)
    lib = tr.build_library(drugs, hints=[_hints(), None])
    pcode, dcodes = _codes(m, torch.bfloat16)
    assert lib.latent.dtype == torch.bfloat16 and torch.equal(lib.latent, torch.cat([c.latent for c in dcodes]).bfloat16())
    sims, idx = tr.shortlist(prots, lib, 4)
    v, i = ops.latent_topk(pcode.latent.bfloat16(), lib.latent, 4)
    assert torch.equal(sims, v) and torch.equal(idx, i)
    vals, hits = tr.screen_library(prots, lib, top_k=2, shortlist=4)
    assert vals.shape == (NP, 2) and bool(((hits.unsqueeze(2) == idx.unsqueeze(1)).any(dim=2)).all())


@pytest.mark.parametrize("kind", ["DrugLAMP", "DrugLAMPwoLLM"])
def test_other_models_have_no_latents_and_refuse_a_shortlist(kind):
    from druglamp_amd.trainer import Trainer
    m, cfg = _model(kind, torch.float32)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=torch.float32)
    m.eval()
    vd, vp, _, xd, xp = _data()
    llm = None if kind == "DrugLAMPwoLLM" else xd[:4]
    assert m.encode_proteins(vp[:NP], xp[:NP]).latent is None and m.encode_drugs(vd[:4], llm).latent is None
    lib = tr.build_library([(vd[:4], llm)])
    assert lib.latent is None
    prots = [(vp[:NP], xp[:NP])]
    with pytest.raises(RuntimeError, match="two_c2p"):
        tr.screen_library(prots, lib, top_k=2, shortlist=3)
    with pytest.raises(RuntimeError, match="two_c2p"):
        tr.shortlist(prots, lib, 3)
