"""The weight EMA at trainer level (Trainer(ema_decay=..., ema_warmup=...), WeightEMA, ema_weights, adopt_ema, fit): eager and
hipGraph-replayed steps, a skipped step, an SSL-epoch step (two optimisers, one update), the swap and two data-parallel ranks.
Small-model pattern of tests/test_trainer_grad_guard_gpu.py: make_batch(8), PMMA dropout off, so that two trainers started
from one seed compute the same bits; a non-finite gradient is planted through the `poison` hook on mlp_classifier.fc4.bias."""
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import ema_ref as er

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]


def _make(dtype, graph=False, seed=4321, dev=DEV, **kw):
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
    tr = Trainer(model, cfg, device=dev, compute_dtype=dtype, graph_steps=graph, **kw)
    tr.set_lrs(1e-3, 1e-3, 1e-3)
    tr.poison = torch.ones((), dtype=torch.float32, device=dev)
    model.mlp_classifier.fc4.bias.register_hook(lambda g, t=tr: g * t.poison)
    return tr


def _batch(dtype, seed=7, dev=DEV, n=8):
    from druglamp_amd.synthetic import make_batch
    return make_batch(n, dev, seed=seed, with_graph=True, llm_dtype=dtype)


def _state(tr):
    return tr.flat.arena.clone(), tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone()


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_off_is_off():
    from druglamp_amd import ops
    try:
        tr = _make(torch.bfloat16)
    finally:
        ops.use_seed_offset(False)
    assert tr.ema is None and tr._ema_spare is None
    with pytest.raises(RuntimeError, match="EMA is off"):
        with tr.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="EMA is off"):
        tr.adopt_ema()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_average_never_touches_the_live_state(dtype):
    from druglamp_amd import ops
    batch, meta = _batch(dtype)
    res = {}
    try:
        for on in (False, True):
            tr = _make(dtype, **({"ema_decay": 0.99} if on else {}))
            keys = [sorted(tr.training_step(batch, meta=meta, cur_epoch=1)) for _ in range(3)]
            tr.check_device_flags()
            res[on] = (_state(tr), keys, tr.ema)
    finally:
        ops.use_seed_offset(False)
    assert res[False][2] is None and res[True][2].updates == 3
    assert res[False][1] == res[True][1] == [["cls"]] * 3
    assert _same(res[False][0], res[True][0])
    assert not torch.equal(res[True][2].shadow, res[True][0][0]) and bool(torch.isfinite(res[True][2].shadow).all())


@pytest.mark.parametrize("warmup", [False, True], ids=["constant", "warmup"])
def test_the_shadow_follows_the_fp64_recurrence_over_the_arena_snapshots(warmup):
    """Four updates: each within 2^-22 max(|e|, |p|) of the exact one (ema_ref.bound), an earlier error is carried with
    factor 1 - w <= 1, and every shadow lies in the hull of the initial arena and the snapshots: 4 * 2^-22 * the largest
    magnitude among those, per element."""
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, ema_decay=0.99, ema_warmup=warmup)
        init = tr.ema.shadow.clone()
        assert torch.equal(_bits(init), _bits(tr.flat.arena)) and init.data_ptr() != tr.flat.arena.data_ptr()
        snaps = []
        for _ in range(4):
            tr.training_step(batch, meta=meta, cur_epoch=1)
            snaps.append(tr.flat.arena.clone())
        tr.check_device_flags()
        shadow = tr.ema.shadow.clone()
    finally:
        ops.use_seed_offset(False)
    assert tr.ema.updates == 4
    want = er.run(init, snaps, 0.99, warmup)
    big = torch.stack([init.abs()] + [s.abs() for s in snaps]).max(dim=0).values.cpu().numpy().astype(np.float64)
    err = np.abs(shadow.cpu().numpy().astype(np.float64) - want)
    lim = 4 * 2.0 ** -22 * big
    moved = int((shadow != init).sum())
    print("warmup", warmup, "moved elements", moved, "worst error / bound", float((err[big > 0] / lim[big > 0]).max()))
    assert bool((err <= lim).all())
    assert moved > 1_000_000
    if warmup:                                                   # 0.9, 9/11, 0.75, 9/13 instead of four times 0.01
        const = er.run(init, snaps, 0.99, False)
        assert float(np.abs(want - const).max()) > 100 * float(lim.max())     # the bound tells the two schedules apart


def test_replayed_steps_update_the_shadow_bit_identically_to_eager_ones():
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    res = {}
    try:
        for graph in (False, True):
            tr = _make(dtype, graph=graph, ema_decay=0.99, ema_warmup=True)
            tr.fixed_caps = tr.fixed_caps_for([(batch, meta)])
            shadows = []
            for _ in range(5):
                tr.training_step(batch, meta=meta, cur_epoch=1)
                shadows.append(tr.ema.shadow.clone())
            tr.check_device_flags()
            res[graph] = (shadows, sum(g.replays for g in tr._graphs.values()), tr.ema.updates)
    finally:
        ops.use_seed_offset(False)
    assert res[True][1] == 3 and res[False][1] == 0             # steps 3, 4, 5 were replays
    assert res[True][2] == res[False][2] == 5
    for k, (a, b) in enumerate(zip(res[False][0], res[True][0])):
        assert torch.equal(_bits(a), _bits(b)), "shadow after step %d" % (k + 1)
    assert not torch.equal(res[True][0][3], res[True][0][4])


def test_a_skipped_step_leaves_the_shadow_alone_but_is_counted():
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, skip_nonfinite=True, ema_decay=0.9)
        shadows = []
        for k in (1, 2, 3):
            tr.poison.fill_(float("nan") if k == 2 else 1.0)
            tr.training_step(batch, meta=meta, cur_epoch=1)
            shadows.append(tr.ema.shadow.clone())
        st = tr.grad_guard_stats()
    finally:
        ops.use_seed_offset(False)
    assert st["skipped"] == 1
    assert torch.equal(_bits(shadows[0]), _bits(shadows[1])), "the skipped step moved the shadow"
    assert not torch.equal(shadows[1], shadows[2]) and bool(torch.isfinite(shadows[2]).all())
    assert tr.ema.updates == 3                                   # the host's count includes the skipped step


def test_an_ssl_epoch_step_updates_the_shadow_once():
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, ema_decay=0.9)
        assert tr.use_ssl and 5 % tr.ssl_epoch_step == 0
        init = tr.ema.shadow.clone()
        out = tr.training_step(batch, meta=meta, cur_epoch=5)
        tr.check_device_flags()
    finally:
        ops.use_seed_offset(False)
    assert "ssl" in out and tr.ema.updates == 1
    assert float(tr.opt_ssl.exp_avg.abs().max()) > 0             # both optimisers stepped
    want = er.update(init, tr.flat.arena, er.weight(0.9, 0))
    err = np.abs(tr.ema.shadow.cpu().numpy().astype(np.float64) - want)
    assert bool((err <= er.bound(init, tr.flat.arena)).all())
    moved, stepped = tr.ema.shadow != init, tr.flat.arena != init
    assert int(moved.sum()) > 100_000 and not bool((moved & ~stepped).any())   # (the SSL backward reaches part of the model)


def test_swapping_the_average_in_and_out():
    from druglamp_amd import functional as Fn
    from druglamp_amd import ops
    from druglamp_amd.synthetic import make_batch
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    (vd, vp, _, xd, xp), _ = make_batch(4, DEV, seed=31, with_graph=False, llm_dtype=dtype)
    try:
        twin = _make(dtype, ema_decay=0.5)                      # never enters the context
        for _ in range(3):
            twin.training_step(batch, meta=meta, cur_epoch=1)
        twin_state, twin_shadow = _state(twin), twin.ema.shadow.clone()
        tr = _make(dtype, ema_decay=0.5)
        for _ in range(2):
            tr.training_step(batch, meta=meta, cur_epoch=1)
        live, shadow = tr.flat.arena.clone(), tr.ema.shadow.clone()
        assert not torch.equal(live, shadow)
        epoch0 = Fn._param_epoch
        with tr.ema_weights() as inside:
            assert inside is tr and Fn._param_epoch > epoch0
            assert torch.equal(_bits(tr.flat.arena), _bits(shadow))
            pred_in = tr.predict([batch])[0].clone()
            lib_in = tr.build_library([(vd, xd)])
            probs_in = tr.screen_library([(vp, xp)], lib_in)
            with pytest.raises(RuntimeError, match="already inside"):
                with tr.ema_weights():
                    pass
            with pytest.raises(RuntimeError, match="inside ema_weights"):
                tr.training_step(batch, meta=meta, cur_epoch=1)
            with pytest.raises(RuntimeError, match="inside ema_weights"):
                tr.adopt_ema()
            assert torch.equal(_bits(tr.flat.arena), _bits(shadow))            # the refusals changed nothing
            epoch_in = Fn._param_epoch
        assert Fn._param_epoch > epoch_in
        assert torch.equal(_bits(tr.flat.arena), _bits(live)) and torch.equal(_bits(tr.ema.shadow), _bits(shadow))
        with pytest.raises(RuntimeError, match="parameter epoch"):
            tr.screen_library([(vp, xp)], lib_in)
        lib_out = tr.build_library([(vd, xd)])
        pred_out = tr.predict([batch])[0].clone()
        with pytest.raises(ZeroDivisionError):                  # an exception inside the context: the live bits come back too
            with tr.ema_weights():
                1 / 0
        assert torch.equal(_bits(tr.flat.arena), _bits(live))
        tr.training_step(batch, meta=meta, cur_epoch=1)
        tr.check_device_flags()
        tr_state, tr_shadow = _state(tr), tr.ema.shadow.clone()
    finally:
        ops.use_seed_offset(False)
    assert _same(twin_state, tr_state) and torch.equal(_bits(twin_shadow), _bits(tr_shadow))     # the next step: as if never entered
    assert bool(torch.isfinite(probs_in).all()) and probs_in.shape == (4, 4)
    assert lib_in.fingerprint != lib_out.fingerprint             # a library built inside is stamped with the averaged weights
    assert not torch.equal(pred_in, pred_out)


def test_predict_inside_the_context_is_predict_of_a_model_holding_the_average():
    """predict inside ema_weights() against a second trainer whose arena was loaded with the shadow's values and whose
    buffers are the first trainer's at that moment (eval-mode BatchNorm reads them)."""
    from druglamp_amd import functional as Fn
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, ema_decay=0.5)
        for _ in range(2):
            tr.training_step(batch, meta=meta, cur_epoch=1)
        with tr.ema_weights():
            pred_in = tr.predict([batch])[0].clone()
        other = _make(dtype)
        with torch.no_grad():
            other.flat.arena.copy_(tr.ema.shadow)
            for dst, src in zip(other.model.buffers(), tr.model.buffers()):
                dst.copy_(src)
        Fn.bump_param_epoch()
        pred_other = other.predict([batch])[0].clone()
        pred_live = tr.predict([batch])[0].clone()
    finally:
        ops.use_seed_offset(False)
    assert torch.equal(_bits(pred_in), _bits(pred_other))
    assert not torch.equal(pred_in, pred_live)


def test_adopt_ema_makes_the_average_the_live_weights():
    from druglamp_amd import functional as Fn
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    try:
        tr = _make(dtype, ema_decay=0.5)
        for _ in range(2):
            tr.training_step(batch, meta=meta, cur_epoch=1)
        shadow = tr.ema.shadow.clone()
        assert not torch.equal(tr.flat.arena, shadow)
        epoch0 = Fn._param_epoch
        tr.adopt_ema()
        sd = tr.model.state_dict()
    finally:
        ops.use_seed_offset(False)
    assert Fn._param_epoch > epoch0
    assert torch.equal(_bits(tr.flat.arena), _bits(shadow)) and torch.equal(_bits(tr.ema.shadow), _bits(shadow))
    name, p = next(iter(tr.model.named_parameters()))
    assert torch.equal(sd[name].reshape(-1), shadow[:p.numel()])                # state_dict holds the averaged weights


def test_fit_validates_selects_and_reloads_on_the_average():
    from druglamp_amd import ops
    dtype = torch.bfloat16
    batch, meta = _batch(dtype)
    val, _ = _batch(dtype, seed=2, n=32)                          # (32 pairs: both classes present, the AUROC exists)
    seen = []
    try:
        tr = _make(dtype, ema_decay=0.5)

        def on_epoch(ep, got):                                   # after the epoch's validation, outside its context
            with tr.ema_weights():
                again = tr.evaluate([val])
            seen.append((ep, dict(got), again, tr.flat.arena.clone(), tr.ema.shadow.clone()))
        res = tr.fit(lambda: [(batch, meta)] * 2, lambda: [val], epochs=2, on_epoch=on_epoch)
    finally:
        ops.use_seed_offset(False)
    h = res["history"]
    assert len(h) == len(seen) == 2 and all(e["weights"] == "ema" for e in h)
    for ep, got, again, _, _ in seen:
        for key, v in again.items():
            assert got[key] == v or (v != v and got[key] != got[key]), (ep, key, got[key], v)
    assert not torch.equal(seen[0][4], seen[1][4]) and tr.ema.updates == 4
    best = seen[res["best_epoch"] - 1]
    assert res["best_epoch"] in (1, 2)
    assert torch.equal(_bits(tr.flat.arena), _bits(best[3])) and torch.equal(_bits(tr.ema.shadow), _bits(best[4]))


# ---- two data-parallel ranks (gloo rendezvous, both on cuda:0) -------------------------------------------------------------------
STEPS2, POISON2 = 5, 4


def _worker(rank, world, port, q):
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    from druglamp_amd import ops
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    tr = _make(dtype, graph=True, seed=1234 + rank, dev=dev, skip_nonfinite=True, ema_decay=0.9)   # (seeded apart: the constructor syncs)
    start_sync = tr.replicas_in_sync() and bool(torch.equal(_bits(tr.ema.shadow), _bits(tr.flat.arena)))
    batch, meta = _batch(dtype, seed=100 + rank, dev=dev)         # different data per rank
    moved = []
    for k in range(1, STEPS2 + 1):
        tr.poison.fill_(float("nan") if (k == POISON2 and rank == 1) else 1.0)     # the plant on rank 1 ONLY
        before = tr.ema.shadow.clone()
        tr.training_step(batch, meta=meta, cur_epoch=1)
        moved.append(not torch.equal(_bits(before), _bits(tr.ema.shadow)))
    torch.cuda.synchronize()
    in_sync = tr.replicas_in_sync()
    if rank == 1:                                                 # the checksum covers the shadow: one element apart is seen
        tr.ema.shadow[12345] += 1.0
    apart = tr.replicas_in_sync()
    q.put((rank, moved, start_sync, in_sync, apart, tr.ema.updates, tr.grad_guard_stats()["skipped"],
           bool(torch.isfinite(tr.ema.shadow).all())))
    ops.use_seed_offset(False)
    dist.destroy_process_group()


def test_two_ranks_keep_bit_identical_shadows_without_another_collective():
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
    for rank, moved, start_sync, in_sync, apart, updates, skipped, finite in res:
        assert moved == [k != POISON2 for k in range(1, STEPS2 + 1)], (rank, moved)     # neither rank's shadow moved at step 4
        assert start_sync and in_sync and not apart, rank
        assert updates == STEPS2 and skipped == 1 and finite, rank
