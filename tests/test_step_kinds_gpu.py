"""Training steps of every kind — cls, SSL-consumed, CM-consumed, SSL + CM — of trainer.Trainer in the fp32 pipeline against
oracle.druglamp_oracle.OracleTrainer in fp64, per parameter (tests/step_ref.py holds the reference side and the comparison):
losses and cm_weight, the set of parameters the optimisers consumed a gradient for, every gradient by relative L2 error,
the step counts and moments of the three fused AdamW instances over the one arena, bitwise stillness of everything the step
left without a gradient (arena padding included), and the parameter update over all elements.  Sequences return to a cls
step behind SSL / CM steps, so step counts (and with them bias corrections and FlatParams.runs) differ between parameters.

The oracle keeps its own optimiser state and adopts the trainer's parameter VALUES between the steps (step_ref.run_oracle
says why: one near-zero-gradient element that an AdamW step moves the other way changes the ProteinCNN gradients of the
next step by several 1e-3 in ANY second arithmetic, the oracle's own fp32 included).  Where a step misses a bound, the ProteinCNN
ReLUs whose fp64 pre-activation lies within fp32 rounding noise of zero may sit on the other side in the reference
(step_ref.resolve_relu_sides: the second SSL step of ssl_only_llm needs ONE, |pre| = 5e-8).  The bound of a gradient is 5e-4, raised
to 4 x the fp32 CPU oracle's own error against fp64 for that parameter only where that error exceeds 1.25e-4.
Measured margins: profiles/step_kinds_margins.txt."""
import pytest
import torch

from tests import step_ref as S

pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("ignore:Using padding='same' with even kernel"),
              pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad=True to a scalar")]
DEV = torch.device("cuda", 0)


class Recorder:
    """Records the trainer's steps in step_ref's layout.  The indices a step consumed are observed by wrapping
    FlatParams.pack_grads; slices of the arena and of the moments run to the next parameter's offset (padding included)."""

    def __init__(self, tr, model):
        names = {id(p): S.canon(n) for n, p in model.named_parameters()}
        fl = tr.flat
        self.tr = tr
        self.keys = [names[id(p)] for p in fl.params]
        assert len(set(self.keys)) == len(self.keys)
        self.numel = {k: p.numel() for k, p in zip(self.keys, fl.params)}
        self.span = [(off, off + (p.numel() + 3) // 4 * 4) for p, off in zip(fl.params, fl.offsets)]
        assert self.span[-1][1] == fl.numel and all(a[1] == b[0] for a, b in zip(self.span, self.span[1:]))
        self.opts = {n: getattr(tr, n) for n in ("opt", "opt_ssl", "opt_cm") if getattr(tr, n) is not None}
        self.consumed = None
        pack = fl.pack_grads

        def observed():
            idx = pack()
            self.consumed = list(idx)
            return idx
        fl.pack_grads = observed
        self.state = self._snap()

    def _cut(self, t):
        t = t.detach().cpu()
        return {k: t[s:e] for k, (s, e) in zip(self.keys, self.span)}

    def _snap(self):
        return {"p": self._cut(self.tr.flat.arena),
                "o": {n: (self._cut(o.exp_avg), self._cut(o.exp_avg_sq), dict(zip(self.keys, o.steps))) for n, o in self.opts.items()}}

    def step(self, batch, meta, ep, masks):
        tr, before = self.tr, self.state
        self.consumed = None
        out = tr.training_step(batch, meta=meta, cur_epoch=ep, ssl_masks=masks)
        tr.check_device_flags()
        after = self.state = self._snap()
        idx = self.consumed
        assert idx is not None, "the step did not pack its gradients through FlatParams.pack_grads"
        rec = {"epoch": ep, "losses": {k: float(v) for k, v in out.items() if k in ("cls", "ssl", "cm")}, "cm_weight": tr.cm_weight,
               "numel": self.numel, "live": frozenset(self.keys[i] for i in idx),
               "grad": {self.keys[i]: tr.flat.grad_views[i].detach().cpu().clone() for i in idx},
               "before": before["p"], "after": after["p"], "opt": {}}
        for n in self.opts:
            rec["opt"][n] = {"step": after["o"][n][2], "m_before": before["o"][n][0], "m": after["o"][n][0],
                             "v_before": before["o"][n][1], "v": after["o"][n][1]}
        return rec


def _setup(name, dtype=torch.float32):
    from druglamp_amd.trainer import Trainer
    S.cap_threads()
    m, cfg, batch, meta, masks = S.build_case(name)
    m = m.to(DEV)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=dtype)
    tr.set_lrs(*S.LRS)                                   # constant learning rates, the oracle's
    assert not tr.run_dead_backward and not tr.graph_steps and tr.world == 1
    vd, vp, y, xd, xp = (t.to(DEV) for t in batch)
    if dtype == torch.bfloat16:
        xd, xp = xd.bfloat16(), xp.bfloat16()
    masks = [(a.to(DEV), b.to(DEV)) for a, b in masks]
    rec = Recorder(tr, m)
    extra = set(rec.keys) - set(S.canon(k) for k in m.state_dict())
    assert not extra, extra
    return m, cfg, tr, rec, (vd, vp, y, xd, xp), batch, meta, masks


def _forms(tr, meta, batch, hints):
    """Which compact forms a step of this batch runs: the ProteinCNN distinct-row plan and / or the drug-token block."""
    plan = tr.protein_plan_of(meta, batch)
    blk = tr.padding_hints_of(meta, batch).get("drug_tokens", 0)
    if hints:
        # batch 8 of seed 33: both pay (no fixed_caps needed) — the ProteinCNN runs on its distinct rows, the drug LLM adaptor,
        # the key side of the cross-attention and SimSiam on one 128-token block per molecule
        assert plan is not None and blk == 128, (plan, blk)
        h = tr.hints_of(meta, batch, kind="ssl")
        assert h.protein_plan is not None and h.drug_tokens == 128
    else:
        assert plan is None and blk == 0
        h = tr.hints_of(meta, batch, kind="ssl")
        assert h.protein_plan is None and h.drug_tokens == 0
    return "ProteinCNN plan %s, drug-token block %d" % ("on (%d rows)" % plan.need if plan is not None else "off", blk)


def _run_case(name):
    c = S.CASES[name]
    m, cfg, tr, rec, dev_batch, batch, meta, masks = _setup(name)
    print("step_kinds %s: %s" % (name, _forms(tr, meta, dev_batch, c["hints"])))
    kw = dict(use_ssl=c["ssl"], use_cm=c["cm"], lrs=S.LRS, batch=batch, meta=meta, masks=S.draw_masks(len(masks)))
    o64 = S.OracleRun(S.oracle_state(m, torch.float64), c["kind"], **kw)
    o32 = S.OracleRun(S.oracle_state(m, torch.float32), c["kind"], **kw)
    assert set(o64.keys) == set(k for k in rec.keys if ".projector." not in k)
    noisy, noisy32, mi = set(), set(), 0
    for i, ep in enumerate(c["epochs"]):
        if i:
            o64.load(rec.state["p"])
            o32.load(rec.state["p"])
        sm = None
        if c["ssl"] and ep % 5 == 0:
            sm = masks[mi]
            mi += 1
        got = rec.step(dev_batch, meta, ep, sm)
        o64.checkpoint()
        ref = o64.step(ep)
        yard, ysum = S.yardstick(o32.step(ep), ref, noisy=noisy32, tag="%s step %d" % (name, i), strict=False)
        failures, tag, seen = [], "%s step %d (epoch %d)" % (name, i, ep), set(noisy)
        rows = S.compare_step(got, ref, yard=yard, noisy=noisy, tag=tag, failures=failures)
        if failures:
            # the reference of a step is a set (step_ref.OracleRun._protein_cnn): the fp64 oracle with the ProteinCNN ReLUs that
            # lie within fp32 rounding noise of zero on either side
            print(S.summary_line(name, i, ep, S.summary(rows), ysum), "| %d checks failed" % len(failures))
            log = []
            ref, flips = S.resolve_relu_sides(o64, ep, got, ref, log)
            print("\n".join("step_kinds %s: %s" % (tag, ln) for ln in log))
            print("step_kinds %s: other side taken at %d group(s) of ReLUs within rounding noise of zero: %s" % (
                tag, len(flips), [(call, layer, len(ixs), "%.3f of the tolerance" % t) for t, call, layer, ixs in flips]))
            if flips:
                noisy.clear()
                noisy.update(seen)
                failures = []
                rows = S.compare_step(got, ref, yard=yard, noisy=noisy, tag=tag, failures=failures)
        print(S.summary_line(name, i, ep, S.summary(rows), ysum))
        assert not failures, "%d checks failed:\n  " % len(failures) + "\n  ".join(failures[:40])
    return rec


def test_ssl_only_llm():
    """DrugLAMP as shipped (RS.SSL, no CM), epochs 4, 5, 5, 6, 6: cls, two SSL-consumed steps (opt and opt_ssl both step the
    23 tensors of the SSL head and the shared ProteinCNN on the SSL gradient), back to cls twice (opt_ssl idle)."""
    rec = _run_case("ssl_only_llm")
    st = rec.state["o"]
    assert st["opt"][2]["protein_extractor.conv1.weight"] == 5 and st["opt"][2]["mlp_classifier.fc1.weight"] == 3
    assert st["opt"][2]["ssl_model.to_logits.weight"] == 2 and st["opt_ssl"][2]["ssl_model.to_logits.weight"] == 2
    assert st["opt_ssl"][2]["mlp_classifier.fc1.weight"] == 0


def test_ssl_only_wollm():
    """DrugLAMPwoLLM as shipped, epochs 4, 5, 6: the masked-LM-only SSL head (no SimSiam: xd is None), 15 live tensors."""
    _run_case("ssl_only_wollm")


def test_cm_start():
    """DrugLAMP2C2P, epochs 4, 5, 6: cls, the ssl + cm step of INIT_EPOCH with the host-side cm_weight auto-scale, a cm step."""
    rec = _run_case("cm_start")
    assert rec.state["o"]["opt_cm"][2]["cm_model.to_prot_latent.weight"] == 2


def test_cm_steady():
    """DrugLAMP2C2P, epochs 6, 10: a cm step without the auto-scale, then ssl + cm past INIT_EPOCH."""
    _run_case("cm_steady")


def test_ssl_only_2c2p():
    """DrugLAMP2C2P with RS.CM off, epoch 5: SimSiam + masked-LM gradients consumed in the 2C2P wiring."""
    _run_case("ssl_only_2c2p")


def test_no_hints():
    """The SSL-consumed step of DrugLAMP without the collate's Drug_Tokens / Prot_Len records: the full forms."""
    _run_case("no_hints")


@pytest.mark.parametrize("name,single", [("ssl_only_llm", "llm_ssl_only"), ("cm_steady", "2c2p_cm")])
def test_bf16_step(name, single):
    """The bf16 pipeline (LLM features cast to bf16) on the SSL-consumed step of DrugLAMP (epoch 5)
    and the cm step of DrugLAMP2C2P (epoch 6), each from the initial weights, against the fp64 oracle."""
    ep = S.SINGLE[single][3]
    m, cfg, tr, rec, dev_batch, batch, meta, masks = _setup(name, torch.bfloat16)
    ref = S.single_reference(single)["ref"]
    got = rec.step(dev_batch, meta, ep, masks[0] if ep % 5 == 0 else None)
    failures = []
    out = S.compare_step_bf16(got, ref, tag="%s epoch %d" % (name, ep), failures=failures)
    print("step_kinds bf16 %-14s epoch %2d: loss errors %s | cosine of the whole gradient %.5f | lowest cosine among the %d largest "
          "parameters %.5f (%s)" % (name, ep, {k: "%.1e" % v for k, v in out["losses"].items()}, out["cos_all"], out["big"],
                                    out["cos_min"], out["cos_min_key"]))
    assert not failures, failures
