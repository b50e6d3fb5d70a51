"""The gradient guard at trainer level (Trainer(max_grad_norm=..., skip_nonfinite=...)): eager and hipGraph-replayed steps,
an SSL-epoch step (two optimisers, one decision) and two data-parallel ranks.  Small-model pattern of
tests/test_graph_step_gpu.py: make_batch(8), PMMA dropout off, so that two trainers started from one seed compute the same
bits.  A non-finite gradient is planted through a tensor hook on mlp_classifier.fc4.bias that multiplies the gradient by a
DEVICE scalar (1.0 or nan): the multiplication is a kernel of the backward pass, so it is captured with the step and a replay
reads whatever the scalar holds then."""
import functools
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import grad_guard_ref as gr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]


def _make(dtype, graph=False, seed=4321, dev=DEV, **guard):
    from druglamp_amd import ops
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.trainer import Trainer
    torch.manual_seed(seed)
    ops.manual_seed(77)
    ops.seed_offset_tensor(dev).zero_()
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    model = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(dev)
    model.pmma.p_drop = 0.0
    model.pmma.embeddings.p_drop = 0.0
    tr = Trainer(model, cfg, device=dev, compute_dtype=dtype, graph_steps=graph, **guard)
    tr.set_lrs(1e-3, 1e-3, 1e-3)
    tr.poison = torch.ones((), dtype=torch.float32, device=dev)
    model.mlp_classifier.fc4.bias.register_hook(lambda g, t=tr: g * t.poison)
    return tr


def _batch(dtype, seed=7, dev=DEV):
    from druglamp_amd.synthetic import make_batch
    return make_batch(8, dev, seed=seed, with_graph=True, llm_dtype=dtype)


def _state(tr):
    return tr.flat.arena.clone(), tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone()


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _bits(x):
    return int(np.float32(x).view(np.int32))


def _step_sqnorm(tr):
    """fp64 sum of squares of flat.grads over the runs of the parameters that hold a gradient (the step's idx)."""
    idx = [i for i, p in enumerate(tr.flat.params) if p.grad is not None]
    assert idx
    return gr.sqnorm(torch.cat([tr.flat.grads[s:e] for s, e, _ in tr.flat.runs(idx, lambda i: 0)]))


@functools.lru_cache(maxsize=None)
def _neutral(dtype):
    """Three steps without the guard and three with a guard that never acts (max_grad_norm 1e30), from one seed.  Computed
    once per dtype and left unchanged: the clip test compares against the state after step 1."""
    from druglamp_amd import ops
    batch, meta = _batch(dtype)
    res = {}
    try:
        for on in (False, True):
            tr = _make(dtype, **({"max_grad_norm": 1e30} if on else {}))
            outs, after1 = [], None
            for k in range(3):
                outs.append(tr.training_step(batch, meta=meta, cur_epoch=1))
                if k == 0:
                    after1 = _state(tr)
                    if on:
                        res["norm1"] = float(outs[0]["grad_norm"])
                        res["sqnorm1"] = _step_sqnorm(tr)
            tr.check_device_flags()
            res[on] = {"keys": [sorted(o) for o in outs], "after1": after1, "final": _state(tr),
                       "stats": tr.grad_guard_stats() if on else None, "guard_obj": tr.grad_guard}
    finally:
        ops.use_seed_offset(False)
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_guard_that_never_acts_changes_no_bit(dtype):
    res = _neutral(dtype)
    assert res[False]["guard_obj"] is None                     # guard off: no state allocated
    assert res[False]["keys"] == [["cls"]] * 3 and res[True]["keys"] == [["cls", "grad_norm"]] * 3
    assert _same(res[False]["after1"], res[True]["after1"]) and _same(res[False]["final"], res[True]["final"])
    st = res[True]["stats"]
    assert (st["skipped"], st["clipped"]) == (0, 0) and st["coef"] == 1.0 and st["norm"] > 0
    assert all(bool(torch.isfinite(t).all()) for t in res[True]["final"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_reported_norm_is_the_fp64_norm_of_the_flat_gradient(dtype):
    res = _neutral(dtype)
    want = np.sqrt(res["sqnorm1"])                             # world size 1: pre_scale 1
    print("grad_norm", res["norm1"], "fp64", want)
    assert abs(res["norm1"] - want) <= float(gr.ulp32(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_clipping_scales_the_first_moments_by_the_coefficient(dtype):
    """AdamW's first update is invariant to the gradient's scale, so the parameters barely differ; the moments carry the
    coefficient: from zero moments exp_avg = fl((1 - b1) fl(g c)) against fl((1 - b1) g) c — three roundings of at most half
    an ulp between them; exp_avg_sq = fl(fl((1 - b2) gc) gc), gc = fl(g c), against fl(fl((1 - b2) g) g) c^2.  4 ulp on
    elements above the smallest normal."""
    from druglamp_amd import ops
    res = _neutral(dtype)
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, max_grad_norm=0.5 * res["norm1"])
        tr.training_step(batch, meta=meta, cur_epoch=1)
        st = tr.grad_guard_stats()
    finally:
        ops.use_seed_offset(False)
    c = st["coef"]
    assert st["clipped"] == 1 and st["skipped"] == 0 and _bits(st["norm"]) == _bits(res["norm1"])
    want_c = 0.5 * res["norm1"] / (np.sqrt(res["sqnorm1"]) + 1e-6)
    assert abs(c - want_c) <= 2 * float(gr.ulp32(want_c)) and 0.49 < c < 0.51     # (norm1 is itself rounded: one more ulp)
    tiny = float(np.finfo(np.float32).tiny)
    for name, power, got, base in (("exp_avg", 1, tr.opt.exp_avg, res[True]["after1"][1]),
                                   ("exp_avg_sq", 2, tr.opt.exp_avg_sq, res[True]["after1"][2])):
        want = base.double() * (float(c) ** power)
        ulp = torch.from_numpy(gr.ulp32(want.abs().float().cpu().numpy())).to(want.device)
        big = want.abs() > tiny
        err = ((got.double() - want).abs() / ulp)[big]
        print(name, "elements", int(big.sum()), "max error / ulp", float(err.max()))
        assert int(big.sum()) > 1_000_000 and float(err.max()) <= 4.0, name
        assert bool(torch.isfinite(got).all())


def _skip_sequence(tr, batch, meta, poison_at, steps):
    """Runs `steps` steps, the (1-based) step poison_at with poison = nan; returns the state after every step and the step's
    host values (read at once: a replayed step returns the graph's static tensors, grad_norm is a view of the guard)."""
    states, outs = [], []
    for k in range(1, steps + 1):
        tr.poison.fill_(float("nan") if k == poison_at else 1.0)
        out = tr.training_step(batch, meta=meta, cur_epoch=1)
        outs.append({key: float(v) for key, v in out.items()})
        states.append(_state(tr))
    return states, outs


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_nonfinite_step_is_skipped_and_training_goes_on(dtype):
    from druglamp_amd import ops
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, skip_nonfinite=True)
        states, outs = _skip_sequence(tr, batch, meta, poison_at=2, steps=3)
        norms = [o["grad_norm"] for o in outs]
        st = tr.grad_guard_stats()
        steps_host = set(tr.opt.steps[i] for i, p in enumerate(tr.flat.params) if p.grad is not None)
        bad = _make(dtype, max_grad_norm=1e30, skip_nonfinite=False)     # the same plant without the skip
        bad_states, _ = _skip_sequence(bad, batch, meta, poison_at=2, steps=2)
        bad_st = bad.grad_guard_stats()
        idx = [i for i, p in enumerate(bad.flat.params) if p.grad is not None]           # the parameters the step updated
        bad_nan = all(bool(torch.isnan(bad.flat.arena[s:e]).all()) for s, e, _ in bad.flat.runs(idx, lambda i: 0))
    finally:
        ops.use_seed_offset(False)
    assert _same(states[0], states[1]), "the poisoned step wrote parameters or moments"
    assert not torch.equal(states[1][0], states[2][0]), "the step after the skipped one did not move the parameters"
    assert all(bool(torch.isfinite(t).all()) for t in states[2])
    assert (st["skipped"], st["clipped"]) == (1, 0) and st["coef"] == 1.0 and np.isfinite(st["norm"])
    assert np.isfinite(norms[0]) and norms[1] != norms[1] and np.isfinite(norms[2]) and _bits(norms[2]) == _bits(st["norm"])
    assert steps_host == {3}                                    # the host's step counts include the skipped step
    assert bool(torch.isfinite(bad_states[0][0]).all())
    assert bad_nan, "without the skip the poisoned step should have made every updated parameter NaN"
    assert bad_st["skipped"] == 0 and bad_st["norm"] != bad_st["norm"]


def test_replayed_steps_clip_and_skip_bit_identically_to_eager_ones():
    """graph_steps=True, past the two eager warm-up steps: a clipped replay, a poisoned replay (skipped), a clean one —
    against the eager guarded trainer at equal capacities."""
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    norm1 = _neutral(dtype)["norm1"]
    res = {}
    try:
        for graph in (False, True):
            tr = _make(dtype, graph=graph, max_grad_norm=0.5 * norm1, skip_nonfinite=True)
            tr.fixed_caps = tr.fixed_caps_for([(batch, meta)])
            states, outs = _skip_sequence(tr, batch, meta, poison_at=4, steps=5)
            tr.check_device_flags()
            res[graph] = (states, tr.grad_guard_stats(), sum(g.replays for g in tr._graphs.values()),
                          [(o["cls"], _bits(o["grad_norm"])) for o in outs])
    finally:
        ops.use_seed_offset(False)
    assert res[True][2] == 3 and res[False][2] == 0             # steps 3, 4, 5 were replays
    for graph in (False, True):
        states, st, _, _ = res[graph]
        assert _same(states[2], states[3]), "the poisoned step wrote parameters or moments (graph=%s)" % graph
        assert not torch.equal(states[3][0], states[4][0])
        assert st["skipped"] == 1 and st["clipped"] >= 1 and all(bool(torch.isfinite(t).all()) for t in states[4])
    assert res[False][1] == res[True][1]                         # norm, coefficient and counters agree bit for bit
    assert res[False][3] == res[True][3]
    for a, b in zip(res[False][0], res[True][0]):
        assert _same(a, b)


def test_an_ssl_epoch_step_takes_one_decision_for_both_optimisers():
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, max_grad_norm=1e-4)
        assert tr.use_ssl and 5 % tr.ssl_epoch_step == 0
        out = tr.training_step(batch, meta=meta, cur_epoch=5)
        st = tr.grad_guard_stats()
    finally:
        ops.use_seed_offset(False)
    assert "ssl" in out and "grad_norm" in out
    assert (st["skipped"], st["clipped"]) == (0, 1) and 0 < st["coef"] < 1     # two optimiser steps, ONE finalize
    assert abs(st["coef"] - 1e-4 / (st["norm"] + 1e-6)) <= 4 * float(gr.ulp32(st["coef"]))
    # from zero moments and equal betas both optimisers hold the same moments iff they applied the same coefficient
    assert float(tr.opt.exp_avg.abs().max()) > 0
    assert torch.equal(tr.opt.exp_avg, tr.opt_ssl.exp_avg) and torch.equal(tr.opt.exp_avg_sq, tr.opt_ssl.exp_avg_sq)


def test_fit_records_the_epochs_skipped_and_clipped_counts():
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    from druglamp_amd.synthetic import make_batch
    val, _ = make_batch(32, DEV, seed=2, with_graph=True, llm_dtype=dtype)     # (32 pairs: both classes present, the AUROC exists)
    try:
        tr = _make(dtype, max_grad_norm=1e-4, skip_nonfinite=True)
        epoch = [0]

        def train_batches():                                     # epoch 1: a clean step, a poisoned one; epoch 2: two clean steps
            epoch[0] += 1
            for k in range(2):
                tr.poison.fill_(float("nan") if (epoch[0] == 1 and k == 1) else 1.0)
                yield batch, meta
        res = tr.fit(train_batches, lambda: [val], epochs=2)
    finally:
        ops.use_seed_offset(False)
    h = res["history"]
    assert len(h) == 2 and (h[0]["grad_skipped"], h[0]["grad_clipped"]) == (1, 1) and (h[1]["grad_skipped"], h[1]["grad_clipped"]) == (0, 2)
    assert np.isfinite(h[1]["train_loss"]) and bool(torch.isfinite(tr.flat.arena).all())
    assert tr.grad_guard_stats()["skipped"] == 1


# ---- two data-parallel ranks (gloo rendezvous, both on cuda:0) -------------------------------------------------------------------
STEPS2, POISON2 = 5, 4


def _worker(rank, world, port, q):
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    from druglamp_amd import ops
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    tr = _make(dtype, graph=True, seed=1234, dev=dev, max_grad_norm=1e-4, skip_nonfinite=True)
    batch, meta = _batch(dtype, seed=100 + rank, dev=dev)         # different data per rank
    norm_bits, same_after_poison = [], None
    for k in range(1, STEPS2 + 1):
        tr.poison.fill_(float("nan") if (k == POISON2 and rank == 1) else 1.0)     # the plant on rank 1 ONLY
        before = _state(tr)
        out = tr.training_step(batch, meta=meta, cur_epoch=1)
        norm_bits.append(_bits(float(out["grad_norm"])))
        if k == POISON2:
            same_after_poison = _same(before, _state(tr))
    torch.cuda.synchronize()
    st = tr.grad_guard_stats()
    replays = sum(g.replays for g in tr._graphs.values())
    q.put((rank, norm_bits, same_after_poison, st, replays, tr.replicas_in_sync(), bool(torch.isfinite(tr.flat.arena).all())))
    ops.use_seed_offset(False)
    dist.destroy_process_group()


def test_two_ranks_take_the_same_decision_without_another_collective():
    """The norm is that of the all-reduced buffer, identical on every rank: both report the same grad_norm bits, both skip
    the step in which ONLY rank 1's gradient is poisoned, and the replicas are in sync at the end."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
    (_, bits0, same0, st0, rep0, sync0, fin0), (_, bits1, same1, st1, rep1, sync1, fin1) = res
    assert bits0 == bits1                                          # the same grad_norm bits, step by step
    nan_step = np.array(bits0[POISON2 - 1], dtype=np.int32).view(np.float32)
    assert np.isnan(nan_step) and all(np.isfinite(np.array(b, dtype=np.int32).view(np.float32)) for k, b in enumerate(bits0) if k != POISON2 - 1)
    assert same0 and same1                                         # both skipped the poisoned step
    assert st0 == st1 or (st0["norm"] != st0["norm"])              # (dict equality fails only on a NaN norm; not the last step here)
    assert st0["skipped"] == st1["skipped"] == 1 and st0["clipped"] == st1["clipped"] == STEPS2 - 1
    assert rep0 == rep1 == STEPS2 - 2 and sync0 and sync1 and fin0 and fin1
