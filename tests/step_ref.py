"""Reference side of the step-kind tests (tests/test_step_kinds_gpu.py, tests/test_step_reference_cpu.py): no GPU needed.

A training step of every kind (cls, ssl, cm, ssl + cm) is run by oracle.druglamp_oracle.OracleTrainer in fp64 and RECORDED —
losses, per-parameter gradients (None kept as None), parameters before / after, and the torch AdamW state of each of the three
optimisers — in the layout `compare_step` reads.  The trainer under test is recorded in the same layout by the GPU test, so the
very same comparison runs on (fp32 pipeline, fp64 oracle), on (fp32 oracle, fp64 oracle) — the yardstick the bounds come
from — and on deliberately broken copies of the oracle's own record (the comparison must bite).

A record (one per step) is a dict:
    epoch, losses {cls, ssl, cm} (0.0 = not computed), cm_weight,
    live    frozenset of parameter keys the optimisers consumed a gradient for,
    grad    {key: tensor} for the live keys,
    numel   {key: int};  before / after {key: tensor} — flat or shaped, at least numel elements (the trainer's slices carry
            the arena's 16-byte padding behind them),
    opt     {"opt" | "opt_ssl" | "opt_cm": {"step": {key: int}, "m_before", "m", "v_before", "v": {key: tensor or None}}}
            (None = torch holds no state for the parameter: counts as step 0 and zero moments).
Keys are parameter names with `ssl_model.extractor.*` mapped onto `protein_extractor.*` (one shared ProteinCNN).

Two properties of the reference that a step-level comparison has to respect (both measured, profiles/step_kinds_margins.txt):
  * in a sequence the oracle adopts the compared run's parameter VALUES between the steps and keeps its own optimiser state
    (`run_oracle` sync=, `OracleRun.load`);
  * the reference of a step is a set: the ProteinCNN ReLUs whose fp64 pre-activation is zero to fp32 rounding may sit on
    either side (`OracleRun.groups`, `resolve_relu_sides`)."""
import contextlib
import copy
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import relerr

ALIAS_FROM, ALIAS_TO = "ssl_model.extractor.", "protein_extractor."
LRS = (1e-4, 3e-5, 3e-5)
BATCH, SEED, SEQ = 8, 33, 2304

# case -> model kind, RS switches, cur_epoch sequence, whether the collate's Drug_Tokens / Prot_Len records stay in meta
CASES = {
    "ssl_only_llm": dict(kind="DrugLAMP", ssl=True, cm=False, epochs=(4, 5, 5, 6, 6), hints=True),
    "ssl_only_wollm": dict(kind="DrugLAMPwoLLM", ssl=True, cm=False, epochs=(4, 5, 6), hints=True),
    "cm_start": dict(kind="DrugLAMP2C2P", ssl=True, cm=True, epochs=(4, 5, 6), hints=True),
    "cm_steady": dict(kind="DrugLAMP2C2P", ssl=True, cm=True, epochs=(6, 10), hints=True),
    "ssl_only_2c2p": dict(kind="DrugLAMP2C2P", ssl=True, cm=False, epochs=(5,), hints=True),
    "no_hints": dict(kind="DrugLAMP", ssl=True, cm=False, epochs=(5,), hints=False),
}

# the bounds of the issue (fp32 pipeline against the fp64 oracle)
TOL = dict(cls=1e-4, ssl=1e-4, cm=1e-3, grad=5e-4, grad_floor=1e-4, noise=1e-3, yard_factor=4.0, yard_min=1.25e-4,
           cos=0.999, share=0.99, share_tol=2e-2)


U_F32 = 2.0 ** -24          # unit roundoff of fp32
RELU_SIGMAS = (8.0, 16.0, 16.0)      # per ProteinCNN layer: see OracleRun.groups
RELU_MAX_GROUPS = 12


def canon(key):
    return ALIAS_TO + key[len(ALIAS_FROM):] if key.startswith(ALIAS_FROM) else key


def cap_threads():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


def oracle_state(model, dtype=torch.float64, alias=True):
    """The oracle's state dict from a model's: floating tensors cloned to `dtype` on the CPU, and the reference's ONE
    ProteinCNN under both `protein_extractor.*` and `ssl_model.extractor.*` restored (state_dict() hands out two keys, a clone
    of each would make the oracle optimise two copies).  alias=False leaves the two copies (tests only: shows it matters)."""
    sd = {}
    for k, v in model.state_dict().items():
        v = v.detach().cpu()
        sd[k] = v.to(dtype).clone() if v.is_floating_point() else v.clone()
    if alias:
        for k in list(sd):
            if k.startswith(ALIAS_FROM):
                sd[k] = sd[ALIAS_TO + k[len(ALIAS_FROM):]]
    return sd


def draw_masks(n_ssl_steps, seed=SEED, batch=BATCH, seq=SEQ):
    """One (mask, replace) pair of (B, 2304) bool per SSL step from a seeded CPU generator: rates 0.15 and 0.1."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return [(torch.rand(batch, seq, generator=g) < 0.15, torch.rand(batch, seq, generator=g) < 0.1) for _ in range(n_ssl_steps)]


def build_case(name):
    """(model on the CPU, cfg, batch on the CPU, meta, masks) of a case: weights from manual_seed(0), SimSiam projectors built
    and frozen (the reference creates them after its optimisers: they are in none), dropout 0, batch 8 of seed 33."""
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.synthetic import make_batch
    c = CASES[name]
    torch.manual_seed(0)
    cfg = load_yaml_into(get_cfg_defaults(), c["kind"])
    cfg["RS"]["SSL"], cfg["RS"]["CM"] = c["ssl"], c["cm"]
    m = MInterface(c["kind"], cfg).load_model(n_drug_feature=384, n_prot_feature=640)
    m.ssl_model.build_projectors(128, 385)
    for n, p in m.named_parameters():
        if ".projector." in n:
            p.requires_grad_(False)
    m.pmma.p_drop = 0.0
    m.pmma.embeddings.p_drop = 0.0
    batch, meta = make_batch(BATCH, "cpu", seed=SEED, with_graph=False)
    if not c["hints"]:
        meta = [{k: v for k, v in mt.items() if k not in ("Drug_Tokens", "Prot_Len")} for mt in meta]
    masks = draw_masks(sum(1 for e in c["epochs"] if c["ssl"] and e % 5 == 0))
    return m, cfg, batch, meta, masks


def _share(cur, prev):
    """Snapshot {key: tensor or None}: a tensor whose bits did not change since `prev` is the SAME object as there (a step
    touches a few dozen of the ~220 tensors), everything else is cloned."""
    out = {}
    for k, t in cur.items():
        if t is None:
            out[k] = None
        elif prev is not None and prev.get(k) is not None and prev[k].shape == t.shape and torch.equal(prev[k], t):
            out[k] = prev[k]
        else:
            out[k] = t.detach().clone()
    return out


class OracleRun:
    """OracleTrainer on the state dict `sd` (its dtype is the run's), one recorded step at a time.
    batch = (vd, vp, y, xd, xp) as the trainer takes it; masks: one (mask, replace) per SSL step, in order."""

    def __init__(self, sd, kind, *, use_ssl, use_cm, lrs, batch, meta, masks):
        from oracle import druglamp_oracle as O
        cap_threads()
        self.dt = dt = next(v.dtype for v in sd.values() if v.is_floating_point())
        vd, vp, y, xd, xp = (t.detach().cpu() for t in batch)
        self.inputs = (vd.to(dt), vp, None if kind == "DrugLAMPwoLLM" else xd.to(dt), xp.to(dt), y.to(dt))
        self.meta, self.masks, self.mi, self.use_ssl = meta, list(masks), 0, use_ssl
        self.ot = ot = O.OracleTrainer(sd, kind, lr=lrs[0], ssl_lr=lrs[1], cm_lr=lrs[2], use_ssl=use_ssl, use_cm=use_cm)
        ids = {id(p) for p in ot.params}
        name = {}
        for k, v in sd.items():
            if id(v) in ids and id(v) not in name:
                name[id(v)] = canon(k) if canon(k) not in name.values() else k      # (two copies, oracle_state(alias=False): own names)
        self.keys = [name[id(p)] for p in ot.params]
        assert len(set(self.keys)) == len(self.keys)
        self.numel = {k: p.numel() for k, p in zip(self.keys, ot.params)}
        self.opts = {n: o for n, o in (("opt", ot.opt), ("opt_ssl", ot.opt_ssl), ("opt_cm", ot.opt_cm)) if o is not None}
        self.prev_p = _share(self._params(), None)
        self.prev_o = {n: (_share(self._moments(o, "exp_avg"), None), _share(self._moments(o, "exp_avg_sq"), None))
                       for n, o in self.opts.items()}
        self.cands, self._flips, self._calls, self._ck = [], (), 0, None

    # -- the ReLUs of the ProteinCNN whose side rounding decides ---------------------------------------------------------------
    # relu(pre) is not differentiable at 0: where a pre-activation lies within the rounding noise of its K-term fp32 sum, WHICH
    # side an arithmetic lands on is not wrong either way (tests/fn_ref.py cnn_relu_tol: "the side of the ReLU is the kernel's
    # to choose"), but the gradient jumps — one such element of conv3 (|pre| = 5.0e-8 in fp64 where the layer's rms is 0.5)
    # moved every ProteinCNN gradient of an SSL-consumed step by 5e-4 - 1.4e-3 of its norm on the MI355X, and putting that one
    # ReLU on the other side in the fp64 oracle brought all of them back to <= 4.1e-5 (profiles/step_kinds_margins.txt).
    # So the reference of a step is a SET: the fp64 oracle with any of the ReLUs whose pre-activation lies within the tolerance
    # of zero on either side.  The tolerance is the one tests/fn_ref.py already holds the ProteinCNN Function to
    # (cnn_relu_tol): 8 standard deviations of the K-term fp32 random-walk rounding error, sqrt(K) u l2, in the first layer and
    # 16 behind it (whose inputs carry rounding of their own) — with the layer's rms pre-activation for l2, the per-element
    # sqrt(sum (w z)^2) it estimates.  The sequences are tiled, so a pre-activation occurs several times as the very same
    # number (and the compact layout computes it once): such ReLUs switch together, as one group.  `groups()` lists the groups
    # after a step; step(ep, flips) takes the other side at the listed ReLUs; `resolve_relu_sides` searches the set.
    def groups(self):
        """[(|pre| / tolerance, call, layer, [flat indices])] of the last step, nearest to zero first."""
        g = {}
        for t, call, layer, ix in self.cands:
            g.setdefault((t, call, layer), []).append(ix)
        return sorted((t, call, layer, sorted(ixs)) for (t, call, layer), ixs in g.items())

    def _protein_cnn(self, sd, p, ids, fill, bn_training):
        """oracle.druglamp_oracle.protein_cnn, token for token, with relu(v) written as v * [v > 0] so that sides can be listed
        and switched (tests/test_step_reference_cpu.py pins that it is bit-identical without switches)."""
        from oracle import druglamp_oracle as O
        call, self._calls = self._calls, self._calls + 1
        v = F.embedding(ids.long(), sd[p + ".embedding.weight"], padding_idx=0)
        v = torch.cat((v, fill.unsqueeze(-1).to(v.dtype)), dim=-1).transpose(2, 1)
        for i in (1, 2, 3):
            w = sd["%s.conv%d.weight" % (p, i)]
            pre = F.conv1d(v, w, sd["%s.conv%d.bias" % (p, i)], padding="same")
            a = pre.detach().abs().reshape(-1)
            tau = RELU_SIGMAS[i - 1] * math.sqrt(w.shape[1] * w.shape[2]) * U_F32 * float(pre.detach().double().pow(2).mean().sqrt())
            self.cands += [(float(a[ix]) / tau, call, i, int(ix)) for ix in (a <= tau).nonzero().flatten().tolist()]
            open_ = pre.detach() > 0
            for c_, l_, ix in self._flips:
                if (c_, l_) == (call, i):
                    open_.view(-1)[ix] = ~open_.view(-1)[ix]
            v = O._bn(sd, "%s.bn%d" % (p, i), torch.where(open_, pre, torch.zeros_like(pre)), bn_training)
        return v.reshape(v.size(0), v.size(2), -1)

    @contextlib.contextmanager
    def _patched(self, flips):
        from oracle import druglamp_oracle as O
        orig, self.cands, self._flips, self._calls = O.protein_cnn, [], tuple(flips), 0
        O.protein_cnn = self._protein_cnn
        try:
            yield
        finally:
            O.protein_cnn = orig

    def checkpoint(self):
        """Remember parameters, optimiser state and bookkeeping: `restore` puts them back (a step can then be taken again)."""
        self._ck = ([p.detach().clone() for p in self.ot.params], {n: copy.deepcopy(o.state_dict()) for n, o in self.opts.items()},
                    self.mi, self.ot.cm_weight, self.prev_p, self.prev_o)

    def restore(self):
        ps, sds, self.mi, self.ot.cm_weight, self.prev_p, prev_o = self._ck
        self.prev_o = dict(prev_o)
        with torch.no_grad():
            for p, q in zip(self.ot.params, ps):
                p.copy_(q)
        for n, o in self.opts.items():
            o.load_state_dict(copy.deepcopy(sds[n]))

    def _params(self):
        return {k: p.detach() for k, p in zip(self.keys, self.ot.params)}

    def _moments(self, o, which):
        return {k: (o.state[p][which] if p in o.state else None) for k, p in zip(self.keys, self.ot.params)}

    def load(self, values):
        """Overwrite the parameter VALUES (not the optimisers' state) with `values` {key: tensor of at least numel elements}:
        the next step then starts from exactly the parameters of the run it is compared with (see `run_oracle`)."""
        with torch.no_grad():
            for k, p in zip(self.keys, self.ot.params):
                p.copy_(values[k].detach().reshape(-1)[:p.numel()].view_as(p).to(p.dtype))
        self.prev_p = _share(self._params(), self.prev_p)

    def step(self, ep, flips=()):
        """flips: (CNN call of the step — 0 the model's forward, 1 the masked-LM pass —, layer 1..3, flat index into the (B, C, L)
        pre-activation) of the ReLUs to put on the other side."""
        ot = self.ot
        mask = replace = None
        if self.use_ssl and ep % ot.epoch_step == 0:
            mask, replace = self.masks[self.mi]
            self.mi += 1
        vd, vp, xd, xp, y = self.inputs
        with self._patched(flips):
            r = ot.step(vd, vp, xd, xp, y, meta=self.meta, cur_epoch=ep, mask=mask, replace=replace)
        pairs = list(zip(self.keys, ot.params))
        rec = {"epoch": ep, "losses": {k: float(r[k]) for k in ("cls", "ssl", "cm")}, "cm_weight": r["cm_weight"], "numel": self.numel}
        rec["grad"] = {k: p.grad.detach().clone() for k, p in pairs if p.grad is not None}
        rec["live"] = frozenset(rec["grad"])
        rec["before"], rec["after"] = self.prev_p, _share(self._params(), self.prev_p)
        rec["opt"] = {}
        for n, o in self.opts.items():
            m, v = _share(self._moments(o, "exp_avg"), self.prev_o[n][0]), _share(self._moments(o, "exp_avg_sq"), self.prev_o[n][1])
            rec["opt"][n] = {"step": {k: (int(o.state[p]["step"]) if p in o.state else 0) for k, p in pairs},
                             "m_before": self.prev_o[n][0], "m": m, "v_before": self.prev_o[n][1], "v": v}
            self.prev_o[n] = (m, v)
        self.prev_p = rec["after"]
        rec["relu_flips"] = tuple(flips)
        return rec


def run_oracle(sd, kind, steps, *, use_ssl, use_cm, lrs, batch, meta, masks, sync=None):
    """OracleTrainer.step for each cur_epoch in `steps`; one record per step.

    sync(i) (optional, called before step i > 0) returns the parameter values {key: tensor} of the run under comparison after
    ITS step i - 1, and the oracle continues from those.  Why: an AdamW step from (nearly) zero moments moves every element by
    ~lr * sign(g), so the one or two elements per tensor whose gradient is smaller than the run's rounding noise move the
    other way in another arithmetic — and the ProteinCNN's gradient, whose BatchNorm backward cancels most of its input
    (DESIGN section 5), turns ONE such element of conv1.weight (2 lr = 2e-4 apart) into a 3e-3 - 6e-3 relative change of every
    ProteinCNN gradient of the NEXT step.  Measured here with the oracle alone: fp32 against fp64 at the SSL step behind a cls
    step, 6.2e-3 when each run follows its own parameters, 8.7e-5 when both start the step from the same ones.  Left alone,
    that chaos — not the arithmetic under test — would set the bound of every step but the first.  The oracle keeps its OWN
    optimiser state (step counts, moments: they are linear in the gradients and do not amplify), so the bookkeeping is still
    compared between two independent runs, and every step's update is checked before the oracle adopts its result."""
    run = OracleRun(sd, kind, use_ssl=use_ssl, use_cm=use_cm, lrs=lrs, batch=batch, meta=meta, masks=masks)
    out = []
    for i, ep in enumerate(steps):
        if sync is not None and i > 0:
            run.load(sync(i))
        out.append(run.step(ep))
    return out


def resolve_relu_sides(run, ep, got, ref, log=None, max_groups=None, stop_at=1e-4):
    """`ref` = run.step(ep) just failed against `got`, and run.checkpoint() was taken in front of it.  Searches the step's
    reference set (OracleRun.groups) greedily: each of the RELU_MAX_GROUPS groups of ReLUs nearest to zero (in units of their
    layer's tolerance; of the ProteinCNN pass whose gradient the step consumes) is put on the other side, alone on top of those already taken, and kept if that brings the ProteinCNN
    gradients of the oracle closer to those of `got` (L2 over all of them, by at least a tenth: a switch the kernel did not
    make moves them apart).  The oracle ends in the state behind the step with the kept switches; returns (its record,
    the kept groups).  A handful of binary choices against ~190 000 gradient elements: a wrong kernel is not fitted by
    them, and every assertion of the step is then made against the result."""
    cnn = [k for k in ref["live"] if k.startswith(ALIAS_TO) and k in got["grad"]]
    if not cnn:
        return ref, []

    def dist(r):
        return math.sqrt(sum(float((_flat(got["grad"][k], r["numel"][k]) - _flat(r["grad"][k], r["numel"][k])).norm()) ** 2 for k in cnn))
    # the pass whose gradient the step consumes: the masked-LM pass (call 1) on an SSL-consumed step, else the model's forward
    call_live = 1 if all(k.startswith(("ssl_model.", ALIAS_TO)) for k in ref["live"]) else 0
    groups = [g for g in run.groups() if g[1] == call_live][:max_groups or RELU_MAX_GROUPS]
    scale = math.sqrt(sum(float(ref["grad"][k].norm()) ** 2 for k in cnn))
    best, flips, kept = dist(ref), [], []
    for t, call, layer, ixs in groups:
        if best <= stop_at * scale:            # (1e-4: already five times inside the plain bound, nothing left to explain)
            break
        run.restore()
        r = run.step(ep, flips + [(call, layer, ix) for ix in ixs])
        d = dist(r)
        if log is not None:
            log.append("call %d layer %d, %d ReLU(s) at %.3f of the tolerance: distance %.3e -> %.3e" % (call, layer, len(ixs), t, best, d))
        if d < 0.9 * best:
            best, ref = d, r
            flips += [(call, layer, ix) for ix in ixs]
            kept.append((t, call, layer, ixs))
    if ref["relu_flips"] != tuple(flips) or run.prev_p is not ref["after"]:
        run.restore()
        ref = run.step(ep, flips)
    return ref, kept


def copy_record(rec):
    """A copy whose dicts are its own and whose tensors are shared: change it by REPLACING entries, never in place."""
    out = dict(rec)
    for f in ("losses", "grad", "before", "after", "numel"):
        out[f] = dict(rec[f])
    out["opt"] = {n: {f: dict(d) for f, d in o.items()} for n, o in rec["opt"].items()}
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------------------
def _flat(t, n):
    return t.detach().reshape(-1)[:n].double().cpu()


def _rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def _same_bits(a, b):
    if a is None or b is None:
        return (a is None or not bool(a.count_nonzero())) and (b is None or not bool(b.count_nonzero()))
    return a is b or torch.equal(a, b)


def grad_bound(key, tol, yard=None):
    """5e-4, raised to 4 x the fp32 oracle's own error against fp64 for this parameter only where that error exceeds 1.25e-4."""
    e = (yard or {}).get(key, 0.0)
    return max(tol["grad"], tol["yard_factor"] * e) if e > tol["yard_min"] else tol["grad"]


def compare_step(got, ref, tol=None, yard=None, noisy=None, tag="", failures=None):
    """The six assertions of a step, `got` against `ref` (records).  yard {key: fp32-oracle relative L2 error of the gradient}
    feeds `grad_bound`; noisy: keys whose gradient an EARLIER step of the sequence excluded as rounding noise (their moments
    carry that noise and are not compared; it is extended in place).  Every failure of the step is collected and raised in
    one AssertionError, each line starting with its assertion's number ("A3 ..."); returns the rows it checked as dicts
    {check, key, value, bound}."""
    tol = dict(TOL, **(tol or {}))
    noisy = set() if noisy is None else noisy
    rows, bad = [], []

    def row(check, key, value, bound, ok):
        rows.append({"check": check, "key": key, "value": value, "bound": bound})
        if not ok:
            bad.append("%s %s %s: %.3e against %.3e" % (check, tag, key, value, bound))

    # 1. losses, cm_weight
    for k in ("cls", "ssl", "cm"):
        r, g = ref["losses"][k], float(got["losses"].get(k, 0.0))
        e = abs(g - r) / max(abs(r), 1e-6) if r != 0.0 else abs(g)
        if r != 0.0:
            relerr(torch.tensor([g], dtype=torch.float64), torch.tensor([r], dtype=torch.float64))
        row("A1", "loss." + k, e, tol[k], e <= tol[k])
    if got["cm_weight"] != ref["cm_weight"]:
        bad.append("A1 %s cm_weight: %r against %r" % (tag, got["cm_weight"], ref["cm_weight"]))
    # 2. the live set
    if set(got["live"]) != set(ref["live"]):
        extra, missing = sorted(set(got["live"]) - set(ref["live"])), sorted(set(ref["live"]) - set(got["live"]))
        bad.append("A2 %s live set: %d extra %s, %d missing %s" % (tag, len(extra), extra[:4], len(missing), missing[:4]))
    live = sorted(set(got["live"]) & set(ref["live"]))
    numel = ref["numel"]
    # 3. gradients per parameter
    gref = {k: _flat(ref["grad"][k], numel[k]) for k in live}
    gmax = max(float(v.norm()) for v in gref.values()) if gref else 0.0
    checked = []
    for k in live:
        if tuple(got["grad"][k].shape) != tuple(ref["grad"][k].shape):
            bad.append("A3 %s %s: shape %s against %s" % (tag, k, tuple(got["grad"][k].shape), tuple(ref["grad"][k].shape)))
            continue
        g = _flat(got["grad"][k], numel[k])
        if float(gref[k].norm()) >= tol["grad_floor"] * gmax:
            relerr(g, gref[k])
            e, b = _rel_l2(g, gref[k]), grad_bound(k, tol, yard)
            row("A3", k, e, b, e <= b)
            checked.append(k)
        else:
            row("A3.noise", k, float(g.norm()), tol["noise"] * gmax, float(g.norm()) <= tol["noise"] * gmax)
            noisy.add(k)
    # 4. optimiser state
    if set(got["opt"]) != set(ref["opt"]):
        bad.append("A4 %s optimisers: %s against %s" % (tag, sorted(got["opt"]), sorted(ref["opt"])))
    for name in sorted(set(got["opt"]) & set(ref["opt"])):
        go, ro = got["opt"][name], ref["opt"][name]
        for k in numel:
            if int(go["step"][k]) != int(ro["step"][k]):
                bad.append("A4 %s %s.step %s: %d against %d" % (tag, name, k, go["step"][k], ro["step"][k]))
            if ro["m"][k] is None:                           # torch holds no state: the moments here are still zero
                if not (_same_bits(go["m"][k], None) and _same_bits(go["v"][k], None)):
                    bad.append("A4 %s %s %s: moments without a step" % (tag, name, k))
        if not any(int(ro["step"][k]) for k in live):
            continue
        for k in checked:
            if k in noisy or ro["m"][k] is None or go["m"][k] is None:
                continue
            b = grad_bound(k, tol, yard)
            e = _rel_l2(_flat(go["m"][k], numel[k]), _flat(ro["m"][k], numel[k]))
            row("A4.m." + name, k, e, b, e <= b)
            e = _rel_l2(_flat(go["v"][k], numel[k]), _flat(ro["v"][k], numel[k]))
            row("A4.v." + name, k, e, 2 * b, e <= 2 * b)
    # 5. untouched means untouched: bitwise, on both sides, padding included
    for side, rec in (("got", got), ("ref", ref)):
        for k in rec["before"]:
            n = rec["numel"].get(k, rec["before"][k].numel())
            dead = k not in rec["live"]
            a, b = rec["before"][k].reshape(-1), rec["after"][k].reshape(-1)
            if not (_same_bits(a, b) if dead else _same_bits(a[n:], b[n:])):
                bad.append("A5 %s %s parameter %s: %s changed" % (tag, side, k, "bits of a parameter without a gradient" if dead else "padding"))
            if not dead:
                continue
            for name, o in rec["opt"].items():
                if not (_same_bits(o["m_before"][k], o["m"][k]) and _same_bits(o["v_before"][k], o["v"][k])):
                    bad.append("A5 %s %s %s %s: moments of a parameter without a gradient changed" % (tag, side, name, k))
    # 6. the update over all elements of the live parameters
    if live:
        dg = torch.cat([_flat(got["after"][k], numel[k]) - _flat(got["before"][k], numel[k]) for k in live])
        dr = torch.cat([_flat(ref["after"][k], numel[k]) - _flat(ref["before"][k], numel[k]) for k in live])
        cos = float(torch.dot(dg, dr) / (dg.norm() * dr.norm() + 1e-300))
        share = float(((dg - dr).abs() <= tol["share_tol"] * dr.abs().max()).double().mean())
        row("A6.cos", "update", cos, tol["cos"], cos >= tol["cos"])
        row("A6.share", "update", share, tol["share"], share >= tol["share"])
    if failures is not None:
        failures.extend(bad)
    elif bad:
        raise AssertionError("%d checks failed:\n  " % len(bad) + "\n  ".join(bad[:40]))
    return rows


def summary(rows):
    """Worst and median of a step's rows, for the printed line and profiles/step_kinds_margins.txt."""
    g = sorted((r["value"], r["key"]) for r in rows if r["check"] == "A3")
    m = [r["value"] for r in rows if r["check"].startswith("A4.m.")]
    v = [r["value"] for r in rows if r["check"].startswith("A4.v.")]
    one = {r["check"]: r["value"] for r in rows if r["check"].startswith("A6")}
    loss = max((r["value"] for r in rows if r["check"] == "A1"), default=0.0)
    return {"live": len([r for r in rows if r["check"] in ("A3", "A3.noise")]), "checked": len(g),
            "grad_worst": g[-1][0] if g else 0.0, "grad_worst_key": g[-1][1] if g else "-",
            "grad_median": float(np.median([x for x, _ in g])) if g else 0.0,
            "m_worst": max(m, default=0.0), "v_worst": max(v, default=0.0), "loss_worst": loss,
            "cos": one.get("A6.cos", 1.0), "share": one.get("A6.share", 1.0)}


def summary_line(case, i, ep, s, y=None):
    t = "step_kinds %-14s step %d epoch %2d: live %3d checked %3d | grad rel-L2 worst %.1e (%s) median %.1e" % (
        case, i, ep, s["live"], s["checked"], s["grad_worst"], s["grad_worst_key"], s["grad_median"])
    t += " | exp_avg worst %.1e exp_avg_sq worst %.1e | loss worst %.1e | update cos %.6f share %.4f" % (
        s["m_worst"], s["v_worst"], s["loss_worst"], s["cos"], s["share"])
    if y is not None:
        t += " | fp32-oracle yardstick: grad worst %.1e median %.1e, cos %.6f share %.4f" % (
            y["grad_worst"], y["grad_median"], y["cos"], y["share"])
    return t


# one step of each kind from the initial weights: (model kind, RS.SSL, RS.CM, cur_epoch)
SINGLE = {
    "2c2p_cls": ("DrugLAMP2C2P", True, True, 4),
    "2c2p_ssl_only": ("DrugLAMP2C2P", True, False, 5),
    "2c2p_cm": ("DrugLAMP2C2P", True, True, 6),
    "2c2p_ssl_cm": ("DrugLAMP2C2P", True, True, 10),
    "2c2p_ssl_cm_start": ("DrugLAMP2C2P", True, True, 5),
    "wollm_cls": ("DrugLAMPwoLLM", True, False, 4),
    "wollm_ssl": ("DrugLAMPwoLLM", True, False, 5),
    "llm_cls": ("DrugLAMP", True, False, 4),
    "llm_ssl_only": ("DrugLAMP", True, False, 5),
}
_CASE_OF = {("DrugLAMP2C2P", True): "cm_start", ("DrugLAMP2C2P", False): "ssl_only_2c2p", ("DrugLAMPwoLLM", False): "ssl_only_wollm",
            ("DrugLAMP", False): "ssl_only_llm"}


def yardstick(rec32, ref, noisy=None, tag="", strict=True):
    """The fp32 oracle's step against the fp64 oracle's by `compare_step` at the plain bounds; returns ({key: gradient error},
    summary).  strict: losses, gradients and update (assertions 1, 3, 6) must pass — the reference stays inside the caps.
    (Not the moments: in a sequence the two oracles may hold different sides of a near-zero ReLU, OracleRun._protein_cnn.)
    The GPU test runs it with strict=False: there the figures only feed `grad_bound`, and a CPU whose fp32 sums land a ReLU on
    the other side must not fail a test of the kernels."""
    failures = []
    rows = compare_step(rec32, ref, noisy=noisy, tag="fp32 oracle " + tag, failures=failures)
    hard = [f for f in failures if f.startswith(("A1", "A3", "A6"))]
    if strict and hard:
        raise AssertionError("%d checks failed:\n  " % len(hard) + "\n  ".join(hard[:40]))
    return {r["key"]: r["value"] for r in rows if r["check"] == "A3"}, summary(rows)


@functools.lru_cache(maxsize=None)
def single_reference(name):
    """The fp64 oracle's record of ONE step of a kind from the initial weights, with the fp32 oracle's yardstick: computed
    once per process, shared by every test that needs it, never modified (copy_record first).
    Returns {"ref": record, "yard": {key: error}, "yard_summary": summary}."""
    kind, ssl, cm, ep = SINGLE[name]
    m, cfg, batch, meta, _ = build_case(_CASE_OF[(kind, cm)])
    kw = dict(use_ssl=ssl, use_cm=cm, lrs=LRS, batch=batch, meta=meta, masks=draw_masks(1))
    ref = run_oracle(oracle_state(m, torch.float64), kind, (ep,), **kw)[0]
    r32 = run_oracle(oracle_state(m, torch.float32), kind, (ep,), **kw)[0]
    yard, ysum = yardstick(r32, ref, tag=name)
    return {"ref": ref, "yard": yard, "yard_summary": ysum}


BF16_TOL = dict(loss=3e-2, cos_all=0.995, cos_each=0.98, big=0.05)


def compare_step_bf16(got, ref, tag="", failures=None):
    """The bf16 pipeline's step against the fp64 oracle's, with the figures of the batch-256 test: losses within 3e-2 (of
    max(1, |ref|)), cosine of the concatenated live gradient (the parameters above the noise floor) >= 0.995, and >= 0.98 for
    every parameter whose reference gradient norm is >= 0.05 of the largest.  Returns {losses, cos_all, cos_min, cos_min_key, big}."""
    bad, out = [], {"losses": {}}
    for k in ("cls", "ssl", "cm"):
        r, g = ref["losses"][k], float(got["losses"].get(k, 0.0))
        e = abs(g - r) / max(1.0, abs(r))
        out["losses"][k] = e
        if e > BF16_TOL["loss"]:
            bad.append("B1 %s loss.%s: %.3e against %.3e" % (tag, k, e, BF16_TOL["loss"]))
    if set(got["live"]) != set(ref["live"]):
        bad.append("B2 %s live set: %d against %d tensors" % (tag, len(got["live"]), len(ref["live"])))
    live = sorted(set(got["live"]) & set(ref["live"]))
    n = ref["numel"]
    gref = {k: _flat(ref["grad"][k], n[k]) for k in live}
    gmax = max(float(v.norm()) for v in gref.values())
    keys = [k for k in live if float(gref[k].norm()) >= TOL["grad_floor"] * gmax]
    ggot = {k: _flat(got["grad"][k], n[k]) for k in keys}
    a, b = torch.cat([ggot[k] for k in keys]), torch.cat([gref[k] for k in keys])
    out["cos_all"] = float(torch.dot(a, b) / (a.norm() * b.norm()))
    big = [k for k in keys if float(gref[k].norm()) >= BF16_TOL["big"] * gmax]
    each = sorted((float(torch.dot(ggot[k], gref[k]) / (ggot[k].norm() * gref[k].norm())), k) for k in big)
    out["cos_min"], out["cos_min_key"], out["big"], out["each"] = each[0][0], each[0][1], len(big), each
    if out["cos_all"] < BF16_TOL["cos_all"]:
        bad.append("B3 %s cosine of the whole gradient: %.5f against %.3f" % (tag, out["cos_all"], BF16_TOL["cos_all"]))
    bad += ["B3 %s cosine of %s: %.5f against %.2f" % (tag, k, c, BF16_TOL["cos_each"]) for c, k in each if c < BF16_TOL["cos_each"]]
    if failures is not None:
        failures.extend(bad)
    elif bad:
        raise AssertionError("%d checks failed:\n  " % len(bad) + "\n  ".join(bad[:40]))
    return out
