"""Library screening (druglamp_amd/screening.py, DrugLAMPBase.encode_proteins / encode_drugs / score_codes, Trainer.screen):
cached entity codes + the pair-indexed PGCA kernel against the CPU oracle and against the model's own eval forward on the
explicit pairs.

Tolerances are the project's: fp32 1e-4 * max(1, |ref|), bf16 3e-2 against the oracle and 2e-2 against the model's own eval
forward (tests/test_eval_path_gpu.py)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NP, ND = 3, 4                     # proteins x drugs of the oracle comparison


def _model(kind, dtype, seed=0):
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    torch.manual_seed(seed)
    cfg = load_yaml_into(get_cfg_defaults(), kind)
    m = MInterface(kind, cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    m.set_compute_dtype(dtype)
    m.eval()
    return m, cfg


def _grid(P, D):
    """All pairs, protein-major: pair p * D + d."""
    pi = torch.arange(P).repeat_interleave(D)
    di = torch.arange(D).repeat(P)
    return pi, di


@functools.lru_cache(maxsize=None)
def _data():
    from druglamp_amd.synthetic import make_batch
    (vd, vp, y, xd, xp), _ = make_batch(4, DEV, seed=31, with_graph=False)
    return vd, vp[:NP], y, xd, xp[:NP]


@functools.lru_cache(maxsize=None)
def _oracle(kind):
    """The oracle's (NP, ND) score matrix for the seed-0 weights of `kind` on the 12 explicit pairs (computed once)."""
    from oracle import druglamp_oracle as O
    m, _ = _model(kind, torch.float32)
    vd, vp, _, xd, xp = _data()
    pi, di = _grid(NP, ND)
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = O.model_forward(sd, kind, vd[di].float().cpu(), vp[pi].cpu(), None if kind == "DrugLAMPwoLLM" else xd[di].float().cpu(),
                              xp[pi].float().cpu())["score"]
    assert ref.shape == (NP * ND, 1)
    return ref.view(NP, ND)


def _screen_scores(m, vd, vp, xd, xp, pi, di, hints=None):
    pcode = m.encode_proteins(vp, xp, hints)
    dcode = m.encode_drugs(vd, xd, hints)
    return m.score_codes(pcode, dcode, pi, di).cpu(), pcode, dcode


@pytest.mark.parametrize("kind", ["DrugLAMP", "DrugLAMPwoLLM"])
def test_fp32_codes_score_like_the_oracle_on_the_explicit_pairs(kind):
    ref = _oracle(kind)
    tol = 1e-4 * max(1.0, float(ref.abs().max()))
    # power: any two proteins and any two drugs differ by more than 3 tolerances somewhere — a swapped index cannot pass
    for a in range(NP):
        for b in range(a + 1, NP):
            assert float((ref[a] - ref[b]).abs().max()) > 3 * tol, (a, b)
    for a in range(ND):
        for b in range(a + 1, ND):
            assert float((ref[:, a] - ref[:, b]).abs().max()) > 3 * tol, (a, b)
    m, _ = _model(kind, torch.float32)
    vd, vp, _, xd, xp = _data()
    pi, di = _grid(NP, ND)
    got, pcode, dcode = _screen_scores(m, vd, vp, xd, xp, pi, di)
    assert got.shape == (NP * ND, 1) and got.dtype == torch.float32
    assert set(pcode.branches) == set(dcode.branches) == ({"v"} if kind == "DrugLAMPwoLLM" else {"v", "x"})
    err = float((got.view(NP, ND) - ref).abs().max())
    print("%s fp32: max |score - oracle| = %.3g (tolerance %.3g)" % (kind, err, tol))
    assert err <= tol


@pytest.mark.parametrize("kind", ["DrugLAMP", "DrugLAMPwoLLM"])
def test_bf16_codes_score_like_the_oracle_and_the_eval_forward(kind):
    """The scores of this data span less than the bf16 tolerance, so this leg cannot see an index mix-up: index correctness
    in bf16 rests on tests/test_pgca_pairs_gpu.py (the kernel against fp64 with permuted and repeated indices) and on the
    fp32 leg above, which runs the same host code."""
    ref = _oracle(kind)
    m, _ = _model(kind, torch.bfloat16)
    vd, vp, _, xd, xp = _data()
    xd, xp = xd.bfloat16(), xp.bfloat16()
    pi, di = _grid(NP, ND)
    got, _, _ = _screen_scores(m, vd, vp, xd, xp, pi, di)
    with torch.no_grad():
        own = m(vd[di], vp[pi], xd[di], xp[pi])[4].float().cpu()
    e_ref, e_own = float((got.view(NP, ND) - ref).abs().max()), float((got - own).abs().max())
    print("%s bf16: max |score - oracle| = %.3g, max |score - eval forward| = %.3g" % (kind, e_ref, e_own))
    assert e_ref <= 3e-2 * max(1.0, float(ref.abs().max()))
    assert e_own <= 2e-2


def test_compact_key_codes_score_like_the_512_key_forward():
    from druglamp_amd.protein_plan import BatchHints
    from druglamp_amd.screening import DrugCode
    from druglamp_amd.synthetic import make_batch
    from druglamp_amd.trainer import Trainer
    P, D = 2, 12
    m, _ = _model("DrugLAMP", torch.float32)
    batch, meta = make_batch(D, DEV, seed=5, with_graph=True)
    (h, adj), vp, _, xd, xp = batch
    vp, xp = vp[:P], xp[:P]
    hints = BatchHints(drug_tokens=Trainer.padding_hints_of(meta, batch)["drug_tokens"], raw_attention=False)
    pi, di = _grid(P, D)
    with torch.no_grad():                                # hints=None: raw logits are kept, the PGCA blocks run over all 512 keys
        ref = m((h[di], adj[di]), vp[pi], xd[di], xp[pi])[4].float().cpu()
    tol = 1e-4 * max(1.0, float(ref.abs().max()))
    got, _, dcode = _screen_scores(m, (h, adj), vp, xd, xp, pi, di, hints)
    assert dcode.layout("v") == (136, 8, 48) and dcode.layout("x") == (136, 8, 48)
    e_compact = float((got - ref).abs().max())
    m.compact_keys = False
    full, _, dfull = _screen_scores(m, (h, adj), vp, xd, xp, pi, di, hints)
    assert dfull.layout("v") == (512, 0, 1) and dfull.layout("x") == (512, 0, 1)
    e_full = float((full - ref).abs().max())
    # one compact and one full batch: cat brings both to the 512-key form (a row gather in ExpandTailFn's order)
    half_full = m.encode_drugs((h[6:], adj[6:]), xd[6:], hints)
    m.compact_keys = True
    m.drug_extractor.compact_min_rows = 0                # six molecules: MolecularGCN would keep its plain form
    half_compact = m.encode_drugs((h[:6], adj[:6]), xd[:6], hints)
    assert half_compact.layout("v") == (136, 8, 48) and half_full.layout("v") == (512, 0, 1)
    mixed = DrugCode.cat([half_compact, half_full])
    assert mixed.layout("v") == (512, 0, 1) and mixed.layout("x") == (512, 0, 1) and mixed.n == D
    e_mixed = float((m.score_codes(m.encode_proteins(vp, xp), mixed, pi, di).cpu() - full).abs().max())
    print("compact keys: max |score - forward| compact %.3g, full %.3g; mixed cat against the all-full code %.3g (tolerance %.3g)"
          % (e_compact, e_full, e_mixed, tol))
    assert e_compact <= tol and e_full <= tol and e_mixed <= tol


def test_contract_of_the_codes_and_trainer_screen():
    from druglamp_amd import functional as Fn
    from druglamp_amd.screening import DrugCode
    from druglamp_amd.trainer import Trainer
    m, cfg = _model("DrugLAMP", torch.float32)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=torch.float32)
    m.eval()
    vd, vp, y, xd, xp = _data()
    pi, di = _grid(NP, ND)
    got, pcode, dcode = _screen_scores(m, vd, vp, xd, xp, pi, di)
    # training mode: codes would depend on the batch through BatchNorm
    m.train()
    for call in (lambda: m.encode_proteins(vp, xp), lambda: m.encode_drugs(vd, xd), lambda: m.score_codes(pcode, dcode, pi, di)):
        with pytest.raises(RuntimeError, match="eval mode only"):
            call()
    m.eval()
    # host indices are range-checked before anything is launched
    for bad_pi, bad_di in (([0, NP], [0, 0]), ([0, 0], [0, ND]), ([-1], [0]), ([0], [-1])):
        with pytest.raises(IndexError):
            m.score_codes(pcode, dcode, bad_pi, bad_di)
    assert m.score_codes(pcode, dcode, [], []).shape == (0, 1)
    # codes built in two drug batches and concatenated: bitwise the scores of one batch
    two = DrugCode.cat([m.encode_drugs(vd[:2], xd[:2]), m.encode_drugs(vd[2:], xd[2:])])
    assert torch.equal(m.score_codes(pcode, two, pi, di).cpu(), got)
    # Trainer.screen over two protein and two drug batches: (P, D) probabilities = sigmoid of score_codes on the full grid
    # (the same kernels on the same operands; only the row counts of the launches differ: 1e-6 is a few fp32 roundings of
    # values of order one), and = predict's on the explicit pairs at the fp32 tolerance
    prob = tr.screen([(vp[:2], xp[:2]), (vp[2:], xp[2:])], [(vd[:1], xd[:1]), (vd[1:], xd[1:])], pair_batch=5)
    assert prob.shape == (NP, ND) and prob.dtype == torch.float32
    assert float((prob.cpu() - torch.sigmoid(got).view(NP, ND)).abs().max()) <= 1e-6
    dd, pp = di.to(DEV), pi.to(DEV)
    p_ref = tr.predict([(vd[dd], vp[pp], y[dd], xd[dd], xp[pp])])[0].cpu().view(NP, ND)
    err = float((prob.cpu() - p_ref).abs().max())
    print("Trainer.screen fp32: max |p - predict| = %.3g" % err)
    assert err <= 1e-4
    # a code from before the parameters changed is refused
    Fn.bump_param_epoch()
    with pytest.raises(RuntimeError, match="parameter epoch"):
        m.score_codes(pcode, dcode, pi, di)
