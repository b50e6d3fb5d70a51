"""Training steps at capacities ABOVE what the batch needs ("Capacities, not exact sizes": "a larger block only
computes more rows explicitly; unused table rows are padding rows").  A step runs at a capacity pair — a drug-token block of
128 / 256 / 384 and a ProteinCNN row-table size off the ladder of protein_plan.row_class — and with varying lengths most steps
of a run execute at a pair larger than their batch needs (Trainer._find_graph replays the tightest graph that HOLDS the batch,
Trainer._capture_caps never shrinks).  Every other test runs at the tightest pair; this file runs above it:

  A  one step of every kind with a cached single-step reference (tests/step_ref.py single_reference), fp32 pipeline, with
     Trainer.fixed_caps at six pairs, per parameter against the fp64 oracle at the plain bounds of step_ref.TOL — the control
     pair (128, 6144) is the trainer's own tight pair and has 1880 padding rows itself; one bf16 step at (384, 12288);
  B  the two mechanisms on their own: the ProteinCNN module and the site pooling through the row map at three table sizes (the
     compact module against the full one AND, in fp32, against an fp64 run of the same layers in plain torch on the CPU;
     padding rows of the pooled gradient exactly zero in a NaN-filled buffer), the drug LLM adaptor, the cross-attention over
     block + 8 keys and SimSiam on the distinct drug rows at blocks 128 / 256 / 384, for a batch whose molecules have at most 128
     tokens and for one with a 200-token molecule — bounds and dtypes of the tight-capacity tests they restate, each cited;
  C  the lookup itself: a small batch replayed on the graph captured for a larger one, bit for bit against an eager trainer
     pinned to that graph's capacities (arena, AdamW moments and step counts, BatchNorm buffers).

An enlarged capacity changes summation order only, so no assertion here has a bound of its own.  Measured margins, the replay
counts of C and which of these tests two arithmetic-only mutations turn red: profiles/capacity_invariance.txt."""
import copy
import functools
import gc

import pytest
import torch
import torch.nn.functional as F

from tests import step_ref as S
from tests.helpers import relerr
from tests.test_step_kinds_gpu import _setup

pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("ignore:Using padding='same' with even kernel"),
              pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad=True to a scalar")]
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _collect_behind_every_test():
    """Trainers with captured graphs are reference cycles (GraphedStep.tr, Trainer._graphs): left to the cyclic collector, a
    trainer of this file would die at an arbitrary later moment, inside another file's test — and tests there count kernel
    launches (tests/test_checkpoint_gpu.py::test_off_means_off), which the weight-image tables rebuilt behind a dead model add
    to.  Nothing of this file outlives its test."""
    yield
    gc.collect()


# ---- A: whole steps ---------------------------------------------------------------------------------------------------------------
NEED = 4264                       # compact rows of the batch of step_ref.build_case (batch 8, seed 33)
TIGHT = (128, 6144)
CAPS = [TIGHT,                    # the control: the trainer's own pair (1880 of its 6144 rows are padding rows already)
        (256, 6144), (384, 6144),             # the block alone, up to its maximum (block <= 512 - 128)
        (128, 8192), (128, 12288),            # the rows alone: one class up, and the last class at which the compact form pays
        (384, 12288)]                         # both
KINDS = ("llm_cls", "llm_ssl_only", "2c2p_cm", "2c2p_ssl_cm", "wollm_ssl")
STEP_CASES = [(k, c) for k in KINDS for c in CAPS if k != "wollm_ssl" or c[0] == 128]       # (no drug LLM branch: rows only)


@functools.lru_cache(maxsize=None)
def _oracle_run(kind):
    """The fp64 OracleRun of a kind at the initial weights with a checkpoint in front of its step — what
    step_ref.resolve_relu_sides needs and step_ref.single_reference does not keep.  Built only if a step misses a bound, once
    per kind; every use starts with restore()."""
    model_kind, ssl, cm, _ = S.SINGLE[kind]
    m, cfg, batch, meta, _ = S.build_case(S._CASE_OF[(model_kind, cm)])
    run = S.OracleRun(S.oracle_state(m, torch.float64), model_kind, use_ssl=ssl, use_cm=cm, lrs=S.LRS, batch=batch, meta=meta,
                      masks=S.draw_masks(1))
    run.checkpoint()
    return run


def _step_at(kind, caps, dtype=torch.float32):
    """One recorded step of `kind` from the initial weights with Trainer.fixed_caps = caps; the capacities are asserted on
    the hints the step runs with."""
    model_kind, ssl, cm, ep = S.SINGLE[kind]
    m, cfg, tr, rec, dev_batch, batch, meta, masks = _setup(S._CASE_OF[(model_kind, cm)], dtype)
    tight = tr.fixed_caps_for([(dev_batch, meta)])
    assert tight == TIGHT, tight
    spec = tr.protein_plan_of(meta, dev_batch, must_pay=False)
    assert spec.need == NEED and spec.pays(12288) and not spec.pays(14336)
    tr.fixed_caps = caps
    compute_ssl, compute_cm = tr.use_ssl and ep % tr.ssl_epoch_step == 0, tr.use_cm and ep >= tr.cm_init_epoch
    assert (compute_ssl, compute_cm) == (ssl and ep % 5 == 0, cm and ep >= 5)
    h = tr.hints_of(meta, dev_batch, kind="cm" if compute_cm else "ssl" if compute_ssl else "cls")
    assert h.drug_tokens == caps[0] and h.protein_plan is not None and h.protein_plan.rows == caps[1], (h.key(), caps)
    assert h.protein_plan.w.numel() == caps[1]
    got = rec.step(dev_batch, meta, ep, masks[0] if compute_ssl else None)          # (ends with tr.check_device_flags())
    assert len(tr._plan_devs) == 1 and next(iter(tr._plan_devs.values())) is h.protein_plan      # the step ran on these tables
    return got, ep


@pytest.mark.parametrize("kind,caps", STEP_CASES, ids=["%s-%d-%d" % (k, c[0], c[1]) for k, c in STEP_CASES])
def test_step_at_capacity(kind, caps):
    """The assertions of tests/test_step_kinds_gpu.py (compare_step: losses, live set, every gradient, moments, stillness,
    update) at the plain bounds of step_ref.TOL, with that file's resolve_relu_sides fallback, at each capacity pair."""
    got, ep = _step_at(kind, caps)
    sr = S.single_reference(kind)
    ref, tag = sr["ref"], "%s at block %d rows %d" % (kind, caps[0], caps[1])
    failures, flips = [], []
    rows = S.compare_step(got, ref, yard=sr["yard"], tag=tag, failures=failures)
    if failures:
        # the reference of a step is a set (step_ref.OracleRun._protein_cnn): the fp64 oracle with the ProteinCNN ReLUs that
        # lie within fp32 rounding noise of zero on either side
        print(_line(kind, caps, rows, got, ref, 0), "| %d checks failed" % len(failures))
        run = _oracle_run(kind)
        run.restore()
        log = []
        ref, flips = S.resolve_relu_sides(run, ep, got, run.step(ep), log)
        print("\n".join("capacity_invariance %s: %s" % (tag, ln) for ln in log))
        if flips:
            failures = []
            rows = S.compare_step(got, ref, yard=sr["yard"], tag=tag, failures=failures)
    print(_line(kind, caps, rows, got, ref, len(flips)))
    assert not failures, "%d checks failed:\n  " % len(failures) + "\n  ".join(failures[:40])


def _line(kind, caps, rows, got, ref, flips):
    s = S.summary(rows)
    ratio, key, val, bound = max((r["value"] / r["bound"], r["key"], r["value"], r["bound"]) for r in rows if r["check"] == "A3")
    losses = " ".join("%s %.6f / %.6f" % (k, float(got["losses"].get(k, 0.0)), ref["losses"][k]) for k in ("cls", "ssl", "cm")
                      if ref["losses"][k] != 0.0)
    return ("capacity_invariance %-12s block %3d rows %5d: live %3d checked %3d | gradient worst %.3f of its bound (%.1e of %.1e, %s) "
            "median %.1e | exp_avg worst %.1e exp_avg_sq worst %.1e | losses got / fp64 %s (worst error %.1e) | update cos %.6f "
            "share %.4f | ReLU groups on the other side %d" % (kind, caps[0], caps[1], s["live"], s["checked"], ratio, val, bound, key,
                                                              s["grad_median"], s["m_worst"], s["v_worst"], losses, s["loss_worst"],
                                                              s["cos"], s["share"], flips))


def test_bf16_step_at_capacity():
    """The bf16 pipeline's SSL-consumed step of DrugLAMP at (384, 12288) against the fp64 oracle at step_ref.BF16_TOL."""
    kind, caps = "llm_ssl_only", (384, 12288)
    got, ep = _step_at(kind, caps, torch.bfloat16)
    failures = []
    out = S.compare_step_bf16(got, S.single_reference(kind)["ref"], tag="%s epoch %d at %s" % (kind, ep, caps), failures=failures)
    print("capacity_invariance bf16 %-12s block %3d rows %5d: loss errors %s | cosine of the whole gradient %.5f | lowest cosine among "
          "the %d largest parameters %.5f (%s)" % (kind, caps[0], caps[1], {k: "%.1e" % v for k, v in out["losses"].items()},
                                                   out["cos_all"], out["big"], out["cos_min"], out["cos_min_key"]))
    assert not failures, failures


# ---- B: ProteinCNN on distinct rows at three table sizes ---------------------------------------------------------------------------
# B = 4, one short protein and one at the longest the collate keeps: need 3370 rows -> 4096 (the 2048-row bucket), 6144 (the
# next class), 8192 (twice the need, rounded to a class): 18 %, 45 % and 59 % of the table are padding rows
CNN_S, CNN_LENGTHS, CNN_SITE = 2304, (100, 1022, 1000, 900), 9
ROWS = ("tight", "next class", "twice the need")


def _cnn_rows(which):
    from druglamp_amd.protein_plan import PlanSpec, row_class
    spec = PlanSpec(CNN_LENGTHS, CNN_S)
    caps = (spec.rows(), row_class(spec.rows() + 1), row_class(2 * spec.need))
    assert spec.need == 3370 and caps == (4096, 6144, 8192), (spec.need, caps)
    return spec, caps[ROWS.index(which)]


def _cnn_plain(m, ids, fill, site_len):
    """ProteinCNN.forward of the reference (basic_model.py:172-180 with the view-not-transpose, then the caller's site pooling,
    DrugLAMP.py:39-40) on the module's own layers in plain torch: any device, any dtype."""
    v = m.embedding(ids.long())
    v = torch.cat((v, fill.unsqueeze(-1).to(v.dtype)), dim=-1).transpose(2, 1)
    for conv, bn in ((m.conv1, m.bn1), (m.conv2, m.bn2), (m.conv3, m.bn3)):
        v = bn(F.relu(conv(v)))
    B, C, L = v.shape
    return v.reshape(B, L, C).view(B, site_len, L // site_len, C).mean(dim=1)


def _cnn_inputs():
    from druglamp_amd.model.basic_model import ProteinCNN
    from tests.test_protein_cnn_compact_gpu import _tiled
    torch.manual_seed(1)
    m = ProteinCNN(128, [128] * 3, [3, 6, 9]).train()
    proj = torch.randn(len(CNN_LENGTHS), CNN_S // CNN_SITE, 128, generator=torch.Generator().manual_seed(4))
    ids, fill = _tiled(len(CNN_LENGTHS), CNN_S, CNN_LENGTHS, seed=3)
    return m, ids, fill, proj


@functools.lru_cache(maxsize=None)
def _cnn_fp64():
    """(output, {parameter: gradient}, {buffer: value}) of the full module in fp64 on the CPU: once per process."""
    m, ids, fill, proj = _cnn_inputs()
    m = m.double()
    z = _cnn_plain(m, ids.cpu(), fill.cpu().double(), CNN_SITE)
    (z * proj.double()).sum().backward()
    return z.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}, {n: b.detach().clone() for n, b in m.named_buffers()}


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dt,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_compact_protein_cnn_module_at_capacity(dt, tol, rows):
    """test_compact_protein_cnn_module_equals_the_full_one (tests/test_protein_cnn_compact_gpu.py) with tables larger than the
    batch needs, its bounds: output tol = 2e-5 / 3e-2, gradients 20 x tol (fp32) or cosine >= 0.995 (bf16), BatchNorm buffers
    1e-4 / 2e-2 — compact against full, and in fp32 both against the fp64 CPU run at the same bounds."""
    from druglamp_amd import ops
    from druglamp_amd.protein_plan import PlanDev
    spec, cap = _cnn_rows(rows)
    pd = PlanDev(spec, DEV, rows=cap)
    assert pd.rows == cap and pd.w.numel() == cap and bool((pd.w[spec.need:] == -1).all()) and bool((pd.src[spec.need:] == -1).all())
    m, ids, fill, proj = _cnn_inputs()
    full = m.to(DEV)
    full.compute_dtype = dt
    comp = copy.deepcopy(full)
    proj = proj.to(DEV)
    outs = []
    for mod, plan in ((full, None), (comp, pd)):
        z = mod(ids, fill.to(dt), site_pool=CNN_SITE, plan=plan)
        (z.float() * proj).sum().backward()
        outs.append(z.float())
    ops.check_guard_flags(DEV)
    bt = 1e-4 if dt == torch.float32 else 2e-2
    errs = {"out": relerr(outs[1], outs[0])}
    assert errs["out"] <= tol
    for (n, a), (_, b) in zip(full.named_parameters(), comp.named_parameters()):
        if dt == torch.float32:
            errs[n] = relerr(b.grad, a.grad)
            assert errs[n] <= 20 * tol, n
        else:
            x, y = b.grad.double().flatten(), a.grad.double().flatten()
            assert float(torch.dot(x, y) / (x.norm() * y.norm() + 1e-30)) >= 0.995, n
    for (n, a), (_, b) in zip(full.named_buffers(), comp.named_buffers()):
        assert relerr(b, a) <= bt, n
    if dt == torch.float32:
        z64, g64, b64 = _cnn_fp64()
        for name, mod, out in (("full", full, outs[0]), ("compact", comp, outs[1])):
            e = {"out": relerr(out, z64)}
            e.update({n: relerr(p.grad, g64[n]) for n, p in mod.named_parameters()})
            eb = {n: relerr(b, b64[n]) for n, b in mod.named_buffers()}
            print("capacity_invariance ProteinCNN %-7s rows %5d against fp64: output %.1e | gradients worst %.1e (%s) | buffers worst %.1e"
                  % (name, cap, e["out"], max(v for k, v in e.items() if k != "out"), max(e, key=lambda k: e[k] if k != "out" else -1),
                     max(eb.values())))
            assert e["out"] <= tol, name
            assert all(v <= 20 * tol for k, v in e.items() if k != "out"), (name, {k: v for k, v in e.items() if v > 20 * tol})
            assert all(v <= bt for v in eb.values()), (name, eb)


@pytest.mark.parametrize("rows", ROWS)
def test_site_pooling_through_the_row_map_at_capacity(rows):
    """dl_cnn_sitepool_rows_fwd / _bwd with tables larger than the batch needs, against the fp64 restatement of
    test_site_pooling_through_the_row_map at its bounds (forward 1e-2, backward 5e-3: one bf16 rounding of an fp32 sum).
    The rows no position maps to hold NaN in the forward's input; the gradient is written into a NaN-filled buffer between
    guard bands: real rows against fp64, padding rows exactly zero, nothing outside the buffer."""
    from druglamp_amd import ops
    from druglamp_amd.protein_plan import PlanDev
    from tests.test_norm_paths_gpu import Guarded, _lib
    Lb, ok, stream, DT, _ = _lib()
    spec, cap = _cnn_rows(rows)
    pd = PlanDev(spec, DEV, rows=cap)
    B, S, C, need = len(CNN_LENGTHS), CNN_S, 128, spec.need
    g = torch.Generator().manual_seed(1)
    z = torch.randn(cap, C, generator=g).bfloat16().to(DEV)
    used = torch.zeros(cap, dtype=torch.bool, device=DEV)
    used[pd.row_of.long()] = True
    assert not bool(used[need:].any())
    z[~used] = float("nan")
    out = ops.cnn_sitepool_rows_fwd(z, pd.row_of, B, S, CNN_SITE)
    zd = z.double().requires_grad_(True)
    full = zd[pd.row_of.long()].view(B, S, C).transpose(1, 2).contiguous().view(B, S, C)
    want = full.view(B, CNN_SITE, S // CNN_SITE, C).mean(dim=1)
    assert bool(torch.isfinite(out.float()).all()) and relerr(out, want) <= 1e-2
    gp = torch.randn(B, S // CNN_SITE, C, generator=g).bfloat16().to(DEV)
    buf = Guarded(cap * C, torch.bfloat16)
    dz = buf.view((cap, C))
    before = buf.bits()
    ok(Lb.dl_cnn_sitepool_rows_bwd(gp.data_ptr(), pd.rep.data_ptr(), pd.row_of.data_ptr(), dz.data_ptr(), B, S, C, cap, CNN_SITE,
                                   DT[torch.bfloat16], stream), "dl_cnn_sitepool_rows_bwd")
    torch.cuda.synchronize()
    buf.untouched("dl_cnn_sitepool_rows_bwd rows %d" % cap, before)
    want.backward(gp.double())
    assert bool((dz[need:].view(torch.int16) == 0).all()), "padding rows of the compact gradient are not +0"
    assert bool((dz[~used].view(torch.int16) == 0).all()), "a row no position maps to received a gradient"
    assert relerr(dz[:need], zd.grad[:need]) <= 5e-3
    ops.check_guard_flags(DEV)


# ---- B: the drug branch at blocks 128 / 256 / 384 --------------------------------------------------------------------------------
# "short": make_batch as it is (at most 128 tokens: 128 is the tight block); "long": one molecule raised to 200 tokens (256 is)
DRUG_CASES = [("short", 128), ("short", 256), ("short", 384), ("long", 256), ("long", 384)]
DRUG_IDS = ["%s-%d" % c for c in DRUG_CASES]


def raise_tokens(batch, meta, b, n_tok):
    """The batch with molecule b's ChemBERTa rows refilled up to n_tok tokens (rows behind them stay zero) and its Drug_Tokens
    record set to match: make_batch never draws more than 128."""
    feat_d, vp, y, xd, xp = batch
    old = int(meta[b]["Drug_Tokens"])
    assert old < n_tok <= xd.shape[1]
    xd = xd.clone()
    xd[b, old:n_tok] = torch.randn(n_tok - old, xd.shape[2], generator=torch.Generator().manual_seed(900 + b)).to(xd)
    meta = [dict(mt) for mt in meta]
    meta[b]["Drug_Tokens"] = n_tok
    return (feat_d, vp, y, xd, xp), meta


def _drug_batch(which, B, dt):
    from druglamp_amd.synthetic import make_batch
    from druglamp_amd.trainer import Trainer
    batch, meta = make_batch(B, DEV, seed=11, with_graph=True, llm_dtype=dt)
    if which == "long":
        batch, meta = raise_tokens(batch, meta, 1, 200)
    assert Trainer.padding_hints_of(meta, batch) == {"drug_tokens": 128 if which == "short" else 256}
    return batch, meta


def _drug_model(dt):
    from druglamp_amd import ops
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    torch.manual_seed(3)
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    ref = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV).train()
    ref.pmma.p_drop = 0.0
    ref.pmma.embeddings.p_drop = 0.0
    ref.set_compute_dtype(dt)
    ops.guard_flags(DEV).zero_()                  # (the sticky guard word may carry a bit an earlier test provoked on purpose)
    return ref


def _running_stats_equal(ref, cmp_, bound):
    """BatchNorm running statistics are forward quantities: the bound of the test's output, never below the 1e-4 that
    test_simsiam_on_the_distinct_drug_rows_equals_all_rows gives them."""
    n_seen = 0
    for (n, a), (_, b) in zip(ref.named_buffers(), cmp_.named_buffers()):
        if "running" in n:
            assert relerr(b, a) <= max(bound, 1e-4), n
            n_seen += 1
        elif "num_batches_tracked" in n:
            assert torch.equal(a, b), n
    assert n_seen >= 10


@pytest.mark.parametrize("which,blk", DRUG_CASES, ids=DRUG_IDS)
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-5), (torch.bfloat16, 2e-2)])
def test_drug_llm_adaptor_at_block(dt, tol, which, blk):
    """test_drug_llm_adaptor_compact_padding_equals_the_full_computation (tests/test_model_gpu.py) at every block that holds the
    batch, its bounds: whole model with BatchHints(drug_tokens=blk) against the four-argument call that computes all 512 rows;
    scores tol = 1e-5 / 2e-2, gradients 50 x tol (fp32) or cosine >= 0.98 (bf16)."""
    from druglamp_amd import ops
    from druglamp_amd.protein_plan import BatchHints
    ref = _drug_model(dt)
    batch, meta = _drug_batch(which, 4, dt)
    cmp_ = copy.deepcopy(ref)
    cmp_.check_padding = True
    feat_d, feat_p, labels, llm_d, llm_p = batch
    outs = []
    for m, h in ((ref, None), (cmp_, BatchHints(drug_tokens=blk))):
        score = m(feat_d, feat_p, llm_d, llm_p, hints=h)[-1]
        score.float().sum().backward()
        outs.append(score.float())
    assert relerr(outs[1], outs[0]) <= tol
    for (n, a), (_, b) in zip(ref.named_parameters(), cmp_.named_parameters()):
        if a.grad is None:
            assert b.grad is None, n
            continue
        if dt == torch.float32:
            assert relerr(b.grad, a.grad) <= 50 * tol, n
        else:
            x, y = b.grad.double().flatten(), a.grad.double().flatten()
            assert float(torch.dot(x, y) / (x.norm() * y.norm() + 1e-30)) >= 0.98, n
    _running_stats_equal(ref, cmp_, tol)
    ops.check_guard_flags(DEV)                       # dl_rows_equal_check stays quiet: every block here holds the batch


@pytest.mark.parametrize("which,blk", DRUG_CASES, ids=DRUG_IDS)
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-4), (torch.bfloat16, 2e-2)])
def test_cross_attention_over_the_drug_rows_at_block(dt, tol, which, blk):
    """test_cross_attention_over_the_distinct_drug_rows_whole_model (tests/test_model_gpu.py) at every block that holds the
    batch, its bounds and batch sizes (4 in fp32, 16 in bf16): PGCA over block + 8 keys with tail weight (512 - block) / 8
    (spied on ops.attn_fwd) against PGCA over the 512 expanded rows."""
    import druglamp_amd.ops as ops_mod
    from druglamp_amd.protein_plan import BatchHints
    ref = _drug_model(dt)
    ref.drug_extractor.compact_min_rows = 0           # (a batch of 4: take the compact MolecularGCN form anyway)
    B = 4 if dt == torch.float32 else 16
    batch, meta = _drug_batch(which, B, dt)
    cmp_ = copy.deepcopy(ref)
    ref.compact_keys, cmp_.compact_keys = False, True
    feat_d, feat_p, labels, llm_d, llm_p = batch
    outs, calls = [], []
    real = ops_mod.attn_fwd
    for m in (ref, cmp_):
        seen = []
        ops_mod.attn_fwd = lambda *a, **k: (seen.append((k["Lk"], k.get("key_tail"))), real(*a, **k))[1]
        try:
            score = m(feat_d, feat_p, llm_d, llm_p, hints=BatchHints(drug_tokens=blk, raw_attention=False))[-1]
        finally:
            ops_mod.attn_fwd = real
        (score.float().view(-1) * torch.tensor([1.0, -2.0, 0.5, 3.0], device=DEV).repeat(B // 4)).sum().backward()
        outs.append(score.float())
        calls.append([c for c in seen if c[0] != 256])                  # the two PGCA launches (PMMA's have Lk = 256)
    assert calls[0] == [(512, None), (512, None)]
    assert sorted(calls[1]) == sorted([(128 + 8, (8, 48)), (blk + 8, (8, (512 - blk) // 8))]), calls[1]
    assert relerr(outs[1], outs[0]) <= (tol if dt == torch.float32 else 3 * tol)
    pa = [(n, a.grad, b.grad) for (n, a), (_, b) in zip(ref.named_parameters(), cmp_.named_parameters()) if a.grad is not None]
    assert all(b is not None for _, _, b in pa) and len(pa) >= 150
    top = max(float(a.abs().max()) for _, a, _ in pa)
    if dt == torch.float32:
        for n, a, b in pa:
            assert float((a - b).abs().max()) <= 20 * tol * max(float(a.abs().max()), 1e-3 * top), n
    else:
        va, vb = torch.cat([a.double().flatten() for _, a, _ in pa]), torch.cat([b.double().flatten() for _, _, b in pa])
        assert float(torch.dot(va, vb) / (va.norm() * vb.norm())) >= 0.997
        for n, a, b in sorted(pa, key=lambda t: -float(t[1].norm()))[:40]:
            x, y = b.double().flatten(), a.double().flatten()
            assert float(torch.dot(x, y) / (x.norm() * y.norm() + 1e-30)) >= 0.88, n
    _running_stats_equal(ref, cmp_, tol if dt == torch.float32 else 3 * tol)
    ops_mod.check_guard_flags(DEV)


@pytest.mark.parametrize("which,lead", DRUG_CASES, ids=DRUG_IDS)
@pytest.mark.parametrize("dt,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_simsiam_on_the_drug_rows_at_block(dt, tol, which, lead):
    """test_simsiam_on_the_distinct_drug_rows_equals_all_rows (tests/test_model_gpu.py) with SSL.drug_simsiam(drug_rows=lead) at
    every block that holds the molecules (GCN rows identical from row 128 on, token rows from each molecule's count on), its
    bounds: loss tol = 2e-5 / 3e-2, input gradient 50 x tol / 0.1, parameter gradients 50 x tol on the scale of the head's
    largest (fp32) or cosine >= 0.98 (bf16), running statistics max(tol, 1e-4)."""
    from druglamp_amd.model.self_supervised_learning import SSL
    torch.manual_seed(2)
    B, N = 6, 512
    n_tok = [100, 200 if which == "long" else 128, 37, 64, 90, 12]
    assert max(n_tok) <= lead
    a = SSL(torch.nn.Identity(), 640, drug_ssl_type="simsiam").to(DEV).train()
    a.compute_dtype = dt
    a.build_projectors(128, 385, DEV)
    b = copy.deepcopy(a)
    g = torch.Generator().manual_seed(3)
    vd0 = torch.randn(B, N, 128, generator=g)
    vd0[:, 128:] = vd0[:, 128:129]                                          # identical padding rows (per molecule, as the GCN gives them)
    xd0 = torch.randn(B, N, 392, generator=g)
    xd0[:, :, 385:] = 0
    for i, n in enumerate(n_tok):
        xd0[i, n:] = xd0[0, N - 1]                                          # the same zero + fill-bit row everywhere
    res = {}
    for name, m, rows in (("all", a, None), ("distinct", b, lead)):
        vd = vd0.to(DEV, dt).requires_grad_(True)
        loss = m.drug_simsiam(vd, (xd0.to(DEV, dt), 385), rows)
        loss.backward()
        gv = vd.grad.float()
        gv_c = torch.cat([gv[:, :lead], gv[:, lead:].reshape(B, -1, 8, 128).sum(1)], 1)       # what reaches the compact rows
        res[name] = (float(loss), gv_c, {n: p.grad.float() for n, p in m.named_parameters() if p.grad is not None},
                     {n: t.float().clone() for n, t in m.named_buffers() if "running" in n})
    assert abs(res["all"][0] - res["distinct"][0]) <= tol * abs(res["all"][0])
    rel = lambda x, y: float((x - y).abs().max() / (y.abs().max() + 1e-30))                 # noqa: E731
    assert rel(res["distinct"][1], res["all"][1]) <= (50 * tol if dt == torch.float32 else 0.1)
    assert set(res["all"][2]) == set(res["distinct"][2]) and len(res["all"][2]) >= 10
    top = max(float(ga.abs().max()) for ga in res["all"][2].values())
    for n, ga in res["all"][2].items():
        gb = res["distinct"][2][n]
        if dt == torch.float32:
            assert float((gb - ga).abs().max()) <= 50 * tol * max(float(ga.abs().max()), 1e-3 * top), n
        elif float(ga.norm()) >= 1e-2 * max(float(t.norm()) for t in res["all"][2].values()):
            assert float(torch.dot(gb.flatten(), ga.flatten()) / (gb.norm() * ga.norm() + 1e-30)) >= 0.98, n
    for n, ra in res["all"][3].items():
        assert rel(res["distinct"][3][n], ra) <= max(tol, 1e-4), n


# ---- C: a small batch replayed on the graph of a larger one ----------------------------------------------------------------------
def _state(tr):
    st = {"arena": tr.flat.arena.clone()}
    for n in ("opt", "opt_ssl", "opt_cm"):
        o = getattr(tr, n)
        if o is not None:
            st[n + ".exp_avg"], st[n + ".exp_avg_sq"], st[n + ".steps"] = o.exp_avg.clone(), o.exp_avg_sq.clone(), list(o.steps)
    for n, b in tr.model.named_buffers():
        st["buffer." + n] = b.clone()
    return st


@pytest.mark.parametrize("ssl_step", [False, True], ids=["cls", "ssl"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_small_batch_replays_the_larger_graph_bit_for_bit(dt, ssl_step):
    """Trainer(graph_steps=True), fixed_caps unset: warm-up and capture on a batch of (256, 6144), then a batch of (128, 4096),
    the large one again (cls, or the SSL-consumed step of epoch 5, which this trainer runs eagerly at the same capacities), the
    small one again.  The small batch's steps are replays of the one captured graph (its tables refilled), and the whole state
    equals, bit for bit, that of an eager trainer with fixed_caps = the graph's capacities."""
    from druglamp_amd.protein_plan import PlanSpec, row_class
    from druglamp_amd.synthetic import make_batch
    from druglamp_amd.trainer import Trainer
    from tests.test_protein_cnn_compact_gpu import _trainer
    large = raise_tokens(*make_batch(8, DEV, seed=41, with_graph=False, llm_dtype=dt, max_prot_len=1022), 0, 200)
    small = make_batch(8, DEV, seed=42, with_graph=False, llm_dtype=dt, max_prot_len=300)
    pairs = [(Trainer.padding_hints_of(mt, bt)["drug_tokens"], row_class(PlanSpec([r["Prot_Len"] for r in mt], 2304).need))
             for bt, mt in (large, small)]
    assert pairs == [(256, 6144), (128, 4096)], pairs
    seq = [(large, 1)] * 3 + [(small, 1), (large, 5 if ssl_step else 1), (small, 1)]
    states, caps = {}, None
    for name in ("graph", "eager"):
        tr = _trainer(name == "graph", True, dt=dt)
        if name == "eager":
            tr.fixed_caps = caps
        counts = []
        for (batch, meta), ep in seq:
            tr.training_step(batch, meta=meta, cur_epoch=ep)
            counts.append((tr.graph_captures, len(tr._graphs), sum(g.replays for g in tr._graphs.values())))
        tr.check_device_flags()
        states[name] = _state(tr)
        if name == "graph":
            (g,) = tr._graphs.values()
            caps = (g.block, g.rows_cap)
            assert caps == pairs[0] and tr.fixed_caps is None
            want = [(0, 0, 0), (0, 0, 0), (1, 1, 1), (1, 1, 2), (1, 1, 2) if ssl_step else (1, 1, 3), (1, 1, 3) if ssl_step else (1, 1, 4)]
            print("capacity_invariance replay %s %s: (captures, graphs, replays) after each step %s"
                  % ("ssl" if ssl_step else "cls", str(dt).split(".")[1], counts))
            assert counts == want, counts
        else:
            assert counts == [(0, 0, 0)] * len(seq)
    a, b = states["graph"], states["eager"]
    assert set(a) == set(b)
    for k in a:
        assert (a[k] == b[k]) if isinstance(a[k], list) else torch.equal(a[k], b[k]), k
    assert a["opt.steps"] and max(a["opt.steps"]) >= 5
