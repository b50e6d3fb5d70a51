"""Hit profiles at the model and trainer level (DrugLAMPBase.cross_attn_profile_codes / cross_attn_profile_library,
Trainer.hit_profiles) on the small synthetic setup of tests/test_library_maps_gpu.py, rebuilt here: seed-0 DrugLAMP and
DrugLAMPwoLLM, make_batch(4, seed=31, with_graph=False), 3 proteins x 4 drugs, the drugs encoded as two batches of different key
layouts (one under the drug_tokens = 128 hint) and a library built from the mixed codes.

The model methods are the kernel wrappers on the codes' own operands (bitwise); Trainer.hit_profiles is the model method whatever
the chunking (bitwise for pair_batch 1, 3 and 256); and a profile agrees with the reductions of Trainer.hit_maps on the same hits
within TWICE the bounds of tests/profile_ref.py — two kernels, each within b of the fp64 reference that is computed here from the
codes' own q and rows (tests/test_pgca_pairs_probs_gpu._drug_map): no model-to-model tolerance."""
import functools

import pytest
import torch

from tests.profile_ref import profile_ref
from tests.test_pgca_pairs_probs_gpu import LAM, _drug_map

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NP, ND = 3, 4
BF, F32 = torch.bfloat16, torch.float32


def _model(kind, dtype):
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    torch.manual_seed(0)
    cfg = load_yaml_into(get_cfg_defaults(), kind)
    m = MInterface(kind, cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    m.set_compute_dtype(dtype)
    m.eval()
    return m, cfg


@functools.lru_cache(maxsize=None)
def _data():
    from druglamp_amd.synthetic import make_batch
    (vd, vp, _, xd, xp), _ = make_batch(4, DEV, seed=31, with_graph=False)
    return vd, vp[:NP], xd, xp[:NP]


def _hints():
    from druglamp_amd.protein_plan import BatchHints
    return BatchHints(drug_tokens=128, raw_attention=False)      # every molecule of make_batch has at most 128 tokens


def _codes(m, dt):
    """(protein code, library of drugs 0-1 encoded under the hint and drugs 2-3 without, the two drug codes)"""
    from druglamp_amd.screening import DrugLibrary
    vd, vp, xd, xp = _data()
    xd, xp = xd.to(dt), xp.to(dt)
    codes = [m.encode_drugs(vd[:2], xd[:2], _hints()), m.encode_drugs(vd[2:], xd[2:])]
    return m.encode_proteins(vp, xp), DrugLibrary.from_codes(codes, m), codes


def _same(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b)) and len(a) == len(b) == 3


@pytest.mark.parametrize("kind,dt", [("DrugLAMP", BF), ("DrugLAMP", F32), ("DrugLAMPwoLLM", BF)],
                         ids=["DrugLAMP-bfloat16", "DrugLAMP-float32", "DrugLAMPwoLLM-bfloat16"])
def test_model_methods_are_the_kernel_wrappers_on_the_codes_operands(kind, dt):
    from druglamp_amd import ops
    from druglamp_amd.screening import LIB_TAIL_ROWS
    m, _ = _model(kind, dt)
    pcode, lib, codes = _codes(m, dt)
    pi, di = torch.arange(NP).repeat_interleave(ND), torch.arange(ND).repeat(NP)
    pi_d, di_d = pi.to(DEV, torch.int32), di.to(DEV, torch.int32)
    assert sorted(lib.branches) == (["v", "x"] if kind == "DrugLAMP" else ["v"])
    for b in lib.branches:
        q, lb = pcode.branches[b][1], lib.branches[b]
        got = m.cross_attn_profile_library(pcode, lib, pi, di, branch=b)
        want = ops.pgca_pairs_ragged_profile(q, lb.rows, lb.row0, lb.n_keys, lb.tail_weight, pi_d, di_d, scale=128 ** -0.5,
                                             key_tail_rows=LIB_TAIL_ROWS, cols=512)
        assert _same(got, want) and all(t.is_cuda for t in got)
        mass, peak, key = got
        assert mass.shape == (NP * ND, 512) and peak.shape == key.shape == (NP * ND, 256) and key.dtype == torch.int32
        assert float((mass.double().sum(-1) - 1).abs().max()) <= 1e-5
        assert bool((key >= 0).all()) and bool((key < lib.keys(b)[di].to(DEV).view(-1, 1)).all())      # an index into the STORED keys
        wide = m.cross_attn_profile_library(pcode, lib, pi, di, branch=b, cols=520)
        assert wide[0].shape == (NP * ND, 520) and bool((wide[0][:, 512:] == 0).all()) and _same((wide[0][:, :512], wide[1], wide[2]), got)
        # the codes of one layout as they are (the x branch of the hinted batch is compact: 136 keys, tail (8, 48))
        d = codes[0].branches[b]
        sel = di < 2
        got_c = m.cross_attn_profile_codes(pcode, codes[0], pi[sel], di[sel], branch=b)
        want_c = ops.pgca_pairs_profile(q, d.kv, pi_d[sel.to(DEV)], di_d[sel.to(DEV)], scale=128 ** -0.5, key_tail=d.key_tail)
        assert _same(got_c, want_c) and got_c[0].shape == (NP * 2, 512) and int(got_c[2].max()) < d.kv.shape[1]
    if kind == "DrugLAMP":
        assert codes[0].layout("x") == (136, 8, 48)
    empty = m.cross_attn_profile_library(pcode, lib, [], [])
    assert empty[0].shape == (0, 0) and empty[1].shape == empty[2].shape == (0, 256)
    with pytest.raises(ValueError, match="cross_attn_profile_library: unknown branch 'w'"):
        m.cross_attn_profile_library(pcode, lib, [0], [0], branch="w")
    if kind == "DrugLAMPwoLLM":
        with pytest.raises(ValueError, match="unknown branch 'x'"):
            m.cross_attn_profile_codes(pcode, codes[0], [0], [0], branch="x")
    with pytest.raises(IndexError, match="drug index out of range"):
        m.cross_attn_profile_library(pcode, lib, [0], [ND])


@pytest.mark.parametrize("dt", [BF, F32], ids=["bfloat16", "float32"])
def test_hit_profiles_of_a_screen(dt):
    from druglamp_amd.screening import LIB_TAIL_ROWS
    from druglamp_amd.trainer import HitProfiles, Trainer
    m, cfg = _model("DrugLAMP", dt)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=dt)
    m.eval()
    vd, vp, xd, xp = _data()
    xd, xp = xd.to(dt), xp.to(dt)
    prots = [(vp[:2], xp[:2]), (vp[2:], xp[2:])]
    lib = tr.build_library([(vd[:2], xd[:2]), (vd[2:], xd[2:])], hints=[_hints(), None])
    _, idx = tr.screen_library(prots, lib, pair_batch=5, top_k=2)
    idx = idx.cpu()
    pcode = m.encode_proteins(vp, xp)
    pi = torch.arange(NP).repeat_interleave(2)
    for b in ("v", "x"):
        want = m.cross_attn_profile_library(pcode, lib, pi, idx.reshape(-1), branch=b)
        for pair_batch in (1, 3, 256):                                      # (chunks of 3 pairs: a chunk ends inside a protein)
            prof = tr.hit_profiles(prots, lib, idx, branch=b, pair_batch=pair_batch)
            assert isinstance(prof, HitProfiles) and not any(t.is_cuda for t in prof)
            assert prof.key_mass.shape == (NP, 2, 512) and prof.site_peak.shape == prof.site_key.shape == (NP, 2, 256)
            assert _same([t.reshape(NP * 2, -1) for t in prof], want), (b, pair_batch)
        # against the reductions of the maps of the same hits: two kernels, each within b of the fp64 reference on the codes
        maps = tr.hit_maps(prots, lib, idx, branch=b, pair_batch=3).double()                    # (NP, 2, 256, 512)
        q, lb = pcode.branches[b][1], lib.branches[b]
        worst = [0.0, 0.0]
        for p in range(NP):
            for j in range(2):
                d = int(idx[p, j])
                r0, n, w = int(lb.row0[d]), int(lb.n_keys[d]), float(lb.tail_weight[d])
                pm, bd, lk_full, lam = _drug_map(q[p:p + 1].contiguous(), lb.rows[r0:r0 + n, :128].contiguous(), LIB_TAIL_ROWS, w, True, 128 ** -0.5)
                assert lam <= LAM and lk_full == 512
                _, km_b, _, peak_b, _ = profile_ref(pm[0], bd[0])
                km_b, peak_b, bd = km_b.cpu(), peak_b.cpu(), bd[0].cpu()
                mp = maps[p, j]
                worst[0] = max(worst[0], float(((prof.key_mass[p, j].double() - mp.mean(0)).abs() / (2 * km_b)).max()))
                peak, arg = mp.max(-1)
                worst[1] = max(worst[1], float(((prof.site_peak[p, j].double() - peak).abs() / (2 * peak_b)).max()))
                key = prof.site_key[p, j].long().unsqueeze(-1)
                assert bool((key >= 0).all()) and bool((key < n).all())
                floor = peak - 2 * bd.gather(-1, key).squeeze(-1) - 2 * bd.gather(-1, arg.unsqueeze(-1)).squeeze(-1)
                assert bool((mp.gather(-1, key).squeeze(-1) >= floor).all()), (b, p, j)
        print("hit_profiles %s %s against the reductions of hit_maps: worst |diff| / (2 bound): key_mass %.4g, site_peak %.4g"
              % (str(dt).split(".")[1], b, worst[0], worst[1]))
        assert worst[0] <= 1.0 and worst[1] <= 1.0
    assert _same(tr.hit_profiles(prots, lib, idx), tr.hit_profiles(prots, lib, idx.numpy(), pair_batch=64))
    # refusals: hit_maps' checks and texts
    with pytest.raises(ValueError, match="hit_profiles: unknown branch 'w'"):
        tr.hit_profiles(prots, lib, idx, branch="w")
    with pytest.raises(ValueError, match="hit_profiles: indices has 2 rows, the protein batches yield more proteins"):
        tr.hit_profiles(prots, lib, idx[:2])
    with pytest.raises(ValueError, match=r"hit_profiles: indices must be \(P, k\)"):
        tr.hit_profiles(prots, lib, idx.reshape(-1))
    with pytest.raises(IndexError, match="hit_profiles: drug index out of range"):
        tr.hit_profiles(prots, lib, idx + ND)
    with pytest.raises(ValueError, match="hit_profiles: indices has 3 rows, the protein batches yielded 2 proteins"):
        tr.hit_profiles(prots[:1], lib, idx)
