"""The reference side of tests/test_step_kinds_gpu.py, checked without a GPU (tests/step_ref.py):
  * the reference stays inside the caps: one step of every kind from the initial weights, fp32 oracle against fp64 oracle,
    passes the losses / gradients / update assertions at the plain bounds; the live and checked tensor counts are pinned;
  * a sequence cls -> ssl -> cls of the fp32 oracle against the fp64 oracle that adopts its parameters between the steps
    (run_oracle's `sync`) passes ALL six assertions at the plain bounds — the mechanics the GPU test relies on;
  * the ProteinCNN alias matters: without it the oracle optimises two copies and an SSL step ends elsewhere;
  * the comparison bites: compare_step fails on copies of the oracle's own record that are wrong in one place."""
import pytest
import torch

from tests import step_ref as S

pytestmark = [pytest.mark.filterwarnings("ignore:Using padding='same' with even kernel"),
              pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad=True to a scalar")]

# measured with batch 8 of seed 33 and the weights of manual_seed(0): (live, checked) tensors of one step from the initial
# weights; the fp32 oracle's worst relative L2 error is printed next to it (5e-5 ... 9e-5; DrugLAMPwoLLM's cls step 1.8e-4 on
# pmma.encoder.encoder_norm.bias, the one tensor whose bound in the GPU test rises above 5e-4: to 4 x that)
COUNTS = {
    "2c2p_cls": (175, 162), "2c2p_ssl_only": (23, 22), "2c2p_cm": (49, 44), "2c2p_ssl_cm": (49, 44), "2c2p_ssl_cm_start": (49, 44),
    "wollm_cls": (147, 137), "wollm_ssl": (15, 15), "llm_cls": (175, 162), "llm_ssl_only": (23, 22),
}


@pytest.mark.parametrize("name", sorted(S.SINGLE))
def test_fp32_oracle_stays_inside_the_caps(name):
    r = S.single_reference(name)                 # (raises if the fp32 oracle misses a bound against the fp64 oracle)
    ys, rec = r["yard_summary"], r["ref"]
    print(S.summary_line(name, 0, rec["epoch"], ys), "| losses", rec["losses"], "cm_weight", rec["cm_weight"])
    assert (len(rec["live"]), ys["checked"]) == COUNTS[name]
    assert ys["grad_worst"] <= S.TOL["grad"], ys
    kind, ssl, cm, ep = S.SINGLE[name]
    ssl_live = [k for k in rec["live"] if k.startswith("ssl_model.") or k.startswith(S.ALIAS_TO)]
    if ssl and ep % 5 == 0 and not (cm and ep >= 5):
        assert len(ssl_live) == len(rec["live"])           # an SSL-consumed step: the SSL head and the shared ProteinCNN only
        assert rec["losses"]["ssl"] > 0 and rec["losses"]["cm"] == 0.0
    if cm and ep >= 5:
        assert rec["losses"]["cm"] > 0                      # the batch's repeated ids yield triplets
    assert rec["cm_weight"] == 1.0                          # (cm and cls losses of this batch are within a factor 10)


def test_sequence_with_adopted_parameters_passes_every_assertion():
    name = "ssl_only_llm"
    c = S.CASES[name]
    m, cfg, batch, meta, masks = S.build_case(name)
    kw = dict(use_ssl=c["ssl"], use_cm=c["cm"], lrs=S.LRS, batch=batch, meta=meta, masks=masks)
    steps = (4, 5, 6)
    r32 = S.run_oracle(S.oracle_state(m, torch.float32), c["kind"], steps, **kw)
    ref = S.run_oracle(S.oracle_state(m, torch.float64), c["kind"], steps, sync=lambda i: r32[i - 1]["after"], **kw)
    noisy = set()
    for i, (a, b) in enumerate(zip(r32, ref)):
        rows = S.compare_step(a, b, noisy=noisy, tag="step %d" % i)
        print(S.summary_line(name, i, b["epoch"], S.summary(rows)))
        assert len(b["live"]) == (23 if b["epoch"] % 5 == 0 else 175)
    # step counts after cls, ssl, cls: opt stepped every live parameter, opt_ssl only the 23 of the SSL step
    last = ref[-1]["opt"]
    assert last["opt"]["step"]["protein_extractor.conv1.weight"] == 3 and last["opt"]["step"]["ssl_model.to_logits.weight"] == 1
    assert last["opt"]["step"]["mlp_classifier.fc1.weight"] == 2 and last["opt_ssl"]["step"]["mlp_classifier.fc1.weight"] == 0
    assert last["opt_ssl"]["step"]["protein_extractor.conv1.weight"] == 1 and "opt_cm" not in last


def test_the_protein_cnn_alias_matters():
    name = "ssl_only_wollm"
    c = S.CASES[name]
    m, cfg, batch, meta, masks = S.build_case(name)
    kw = dict(use_ssl=True, use_cm=False, lrs=S.LRS, batch=batch, meta=meta, masks=masks)
    sd = S.oracle_state(m)
    assert sd["ssl_model.extractor.conv1.weight"] is sd["protein_extractor.conv1.weight"]
    split = S.oracle_state(m, alias=False)
    assert split["ssl_model.extractor.conv1.weight"] is not split["protein_extractor.conv1.weight"]
    S.run_oracle(sd, c["kind"], (5,), **kw)
    S.run_oracle(split, c["kind"], (5,), **kw)
    w0 = m.state_dict()["protein_extractor.conv1.weight"].double()
    moved = float((sd["protein_extractor.conv1.weight"].detach() - w0).abs().max())
    assert moved > 0.5 * (S.LRS[0] + S.LRS[1])             # opt and opt_ssl both stepped the shared ProteinCNN on the SSL gradient
    # two copies: the SSL head's copy trains, the model's own ProteinCNN never sees the SSL gradient
    assert torch.equal(split["protein_extractor.conv1.weight"].detach(), w0)
    assert not torch.equal(split["ssl_model.extractor.conv1.weight"].detach(), w0)


def test_relu_sides_are_listed_switched_and_found():
    """OracleRun's ProteinCNN (relu written as a mask) equals the oracle's own bit for bit; a step taken with one near-zero ReLU
    on the other side has other ProteinCNN gradients, and resolve_relu_sides finds exactly that switch again."""
    from oracle import druglamp_oracle as O
    name = "ssl_only_wollm"
    c = S.CASES[name]
    m, cfg, batch, meta, masks = S.build_case(name)
    kw = dict(use_ssl=True, use_cm=False, lrs=S.LRS, batch=batch, meta=meta, masks=masks)
    run = S.OracleRun(S.oracle_state(m), c["kind"], **kw)
    run.checkpoint()
    ref = run.step(5)
    # the oracle as it stands, without OracleRun
    sd = S.oracle_state(m)
    ot = O.OracleTrainer(sd, c["kind"], lr=S.LRS[0], ssl_lr=S.LRS[1], cm_lr=S.LRS[2], use_ssl=True, use_cm=False)
    vd, vp, y, xd, xp = batch
    r = ot.step(vd.double(), vp, None, xp.double(), y.double(), meta=meta, cur_epoch=5, mask=masks[0][0], replace=masks[0][1])
    assert float(r["ssl"]) == ref["losses"]["ssl"]
    assert torch.equal(sd["protein_extractor.conv1.weight"].grad, ref["grad"]["protein_extractor.conv1.weight"])
    assert torch.equal(sd["protein_extractor.conv1.weight"].detach(), ref["after"]["protein_extractor.conv1.weight"])
    # a switch: the groups are listed nearest to zero first, in units of the layer's tolerance
    groups = run.groups()
    assert 1 <= len(groups) <= 2000 and all(0.0 <= g[0] <= 1.0 for g in groups) and groups == sorted(groups), len(groups)
    print("groups of ReLUs within the tolerance of zero: %d; nearest %s" % (len(groups), [(g[0], g[1], g[2], len(g[3])) for g in groups[:3]]))
    pick = next(g for g in groups if g[1] == 1)            # (call 1: the masked-LM pass, whose gradient the step consumes)
    flips = [(pick[1], pick[2], ix) for ix in pick[3]]
    run.restore()
    other = run.step(5, flips)
    k = "protein_extractor.conv%d.bias" % pick[2]
    assert not torch.equal(other["grad"][k], ref["grad"][k])
    run.restore()
    again = run.step(5)
    assert torch.equal(again["grad"][k], ref["grad"][k]) and torch.equal(again["after"][k], ref["after"][k])      # restore restores
    found, kept = S.resolve_relu_sides(run, 5, other, again, max_groups=3, stop_at=0.0)
    assert kept == [pick] and found["relu_flips"] == tuple(flips) and torch.equal(found["grad"][k], other["grad"][k])
    S.compare_step(other, found)


def _broken(rec, what):
    lr, wd = S.LRS[0], 1e-2
    bad = S.copy_record(rec)
    dead = next(k for k in sorted(rec["before"]) if k not in rec["live"] and k.endswith(".weight") and not k.startswith("drug_extractor."))
    if what == "negated gradient":
        k = "ssl_model.to_logits.weight" if "ssl_model.to_logits.weight" in rec["live"] else "v_gca.out_proj.weight"
        bad["grad"][k] = -rec["grad"][k]
    elif what == "transposed gradient":
        k = next(k for k in sorted(rec["live"]) if rec["grad"][k].dim() == 2 and rec["grad"][k].shape[0] == rec["grad"][k].shape[1])
        bad["grad"][k] = rec["grad"][k].t().contiguous()
    elif what == "weight decay on a dead parameter":
        bad["after"][dead] = rec["after"][dead] * (1 - lr * wd)
    elif what == "step count of a dead parameter":
        bad["opt"]["opt"]["step"][dead] = rec["opt"]["opt"]["step"][dead] + 1
    elif what == "opt_ssl moments on a cls step":
        k = "protein_extractor.conv1.weight"
        bad["opt"]["opt_ssl"]["m"][k] = 0.1 * rec["grad"][k]
    return bad


@pytest.mark.parametrize("what,caught_by", [
    ("negated gradient", "A3"), ("transposed gradient", "A3"), ("weight decay on a dead parameter", "A5"),
    ("step count of a dead parameter", "A4"), ("opt_ssl moments on a cls step", "A4"),
])
def test_the_comparison_bites(what, caught_by):
    # an SSL-consumed step has dead parameters (everything but the 23 live ones); the opt_ssl case needs a cls step,
    # the transposed one a square weight (the SSL heads have none)
    rec = S.single_reference("llm_cls" if "cls step" in what or "transposed" in what else "2c2p_ssl_only")["ref"]
    S.compare_step(S.copy_record(rec), rec)                     # the untouched copy passes
    failures = []
    S.compare_step(_broken(rec, what), rec, failures=failures)
    assert failures and all(f.startswith(("A4", "A5") if caught_by == "A4" else caught_by) for f in failures), failures
    assert any(f.startswith(caught_by) for f in failures), failures
    with pytest.raises(AssertionError, match=caught_by):
        S.compare_step(_broken(rec, what), rec)
