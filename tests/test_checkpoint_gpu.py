"""Trainer checkpoints (Trainer.save_checkpoint / load_checkpoint / fit(checkpoint_dir=..., resume=...)) on the device: the round
trip, resumed runs against uninterrupted ones bit for bit, prediction after a load, refusals, and "off means off".

Setup of tests/test_graph_step_gpu.py: make_batch(8) batches, bf16 compute, lr 1e-3.  A "fresh" trainer is a new model built
under a DIFFERENT torch.manual_seed with a differently seeded dropout generator; before it loads it also draws from
ops.next_seed() and torch's device generator, so a load that forgets one of the generators is caught.  Nothing here has a
tolerance: every comparison is torch.equal or equality of floats."""
import gc
import os
import shutil
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ADAPTOR = "p_adaptor_wo_skip_connect."


def _make(p_drop=0.0, graph=False, seed=4321, kind="DrugLAMP", gen_seed=77, **kw):
    from druglamp_amd import ops
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.trainer import Trainer
    torch.manual_seed(seed)
    ops.manual_seed(gen_seed)
    ops.seed_offset_tensor(DEV).zero_()
    cfg = load_yaml_into(get_cfg_defaults(), kind)
    model = MInterface(kind, cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    model.pmma.p_drop = p_drop
    model.pmma.embeddings.p_drop = p_drop
    tr = Trainer(model, cfg, device=DEV, compute_dtype=torch.bfloat16, graph_steps=graph, **kw)
    tr.set_lrs(1e-3, 1e-3, 1e-3)
    return tr


def _fresh(p_drop=0.0, graph=False, seed=999, **kw):
    """A trainer that shares nothing with the saving one: other initial weights, other generator positions."""
    from druglamp_amd import ops
    tr = _make(p_drop, graph, seed=seed, gen_seed=4242, **kw)
    ops.next_seed()
    torch.rand(5, device=DEV)
    torch.rand(5)
    return tr


def _batches(seeds=(7, 8, 9)):
    from druglamp_amd.synthetic import make_batch
    return [make_batch(8, DEV, seed=s, with_graph=True, llm_dtype=torch.bfloat16) for s in seeds]


def _state(tr):
    """Every tensor a step leaves behind: arena, the moments of every optimiser, all buffers, shadow, guard counters."""
    out = {"arena": tr.flat.arena.clone()}
    for name, o, _ in tr._opt_schd():
        out[name + ".exp_avg"], out[name + ".exp_avg_sq"] = o.exp_avg.clone(), o.exp_avg_sq.clone()
    for k, b in tr.model.named_buffers():
        out["buffer " + k] = b.detach().clone()
    if tr.ema is not None:
        out["shadow"] = tr.ema.shadow.clone()
    if tr.grad_guard is not None:
        out["guard counters"] = tr.grad_guard.counters.clone()
    return out


def _counts(tr):
    """Every host-side count and value a checkpoint carries."""
    cm = getattr(tr.model, "cm_model", None)
    return {"steps": {n: list(o.steps) for n, o, _ in tr._opt_schd()}, "lr": {n: o.lr for n, o, _ in tr._opt_schd()},
            "schedulers": {n: (s.step_in_cycle, s.cycle, s.lr) for n, _, s in tr._opt_schd()},
            "ema.updates": None if tr.ema is None else tr.ema.updates, "cm_weight": tr.cm_weight,
            "margin": None if cm is None else (cm.m_sch_loss_fn._step, cm.m_sch_loss_fn.m_cur),
            "groups": None if tr.param_groups is None else (tr.param_group_table(), list(tr.param_groups.rows))}


def _assert_same(a: dict, b: dict):
    assert list(a) == list(b), (sorted(set(a) ^ set(b)))
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def _floats(out):
    return {k: float(v) for k, v in out.items()}


@pytest.fixture
def ckdir(tmp_path):
    yield tmp_path
    shutil.rmtree(tmp_path, ignore_errors=True)          # (a checkpoint of the default model is a few hundred MB)


@pytest.fixture(autouse=True)
def _collect_trainers():
    """A trainer is a reference cycle (its captured graphs point back at it): collect the four to eight of a test here, so that
    their device memory — some of it used on side streams — is not released in the middle of whatever test runs later."""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _groups():
    from druglamp_amd.param_groups import ParamGroup
    return [ParamGroup("adaptor", match=(ADAPTOR + "*",), frozen=True),
            ParamGroup("no_decay", max_ndim=1, weight_decay=0.0),
            ParamGroup("encoders", match=("drug_extractor.*", "protein_extractor.*"), lr_scale=0.1)]


def _everything():
    from druglamp_amd.cls_loss import ClsLoss
    return dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.99, ema_warmup=True, cls_loss=ClsLoss(pos_weight=2.0, gamma=2.0),
                param_groups=_groups())


def test_round_trip_with_everything_on(ckdir):
    from druglamp_amd import ops
    from druglamp_amd.model import MInterface, load_reference_checkpoint
    path = ckdir / "all.pt"
    try:
        a = _make(**_everything())
        a.set_param_group("encoders", lr_scale=0.05, weight_decay=0.02)
        for b, mt in _batches():
            a.training_step(b, meta=mt, cur_epoch=1)
        a.on_train_epoch_end(1)
        a.save_checkpoint(path, extra={"note": "three steps", "ids": [1, 2, 3]})
        b_ = _fresh(**_everything())
        assert not torch.equal(a.flat.arena, b_.flat.arena)
        extra = b_.load_checkpoint(path)
    finally:
        ops.use_seed_offset(False)
    assert extra == {"note": "three steps", "ids": [1, 2, 3]}
    _assert_same(_state(a), _state(b_))
    assert _counts(a) == _counts(b_)
    assert a.opt.steps != [0] * len(a.opt.steps) and a.ema.updates == 3 and a.schd.step_in_cycle == 1
    assert b_.param_groups.values("encoders") == (0.05, 0.02)
    assert torch.equal(a.param_groups.group_tab, b_.param_groups.group_tab)                 # the device table was rewritten
    frozen = [p for (g, n, _), p in zip(b_.param_group_table(), b_.flat.params) if g == "adaptor"]
    assert frozen and not any(p.requires_grad for p in frozen)
    assert a.grad_guard_stats() == b_.grad_guard_stats()
    # the file is a weight file too: the reference loader takes it as it stands
    torch.manual_seed(5)
    m = MInterface("DrugLAMP", a.cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    res = load_reference_checkpoint(m, str(path), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, x), (k2, y) in zip(a.model.state_dict().items(), m.state_dict().items()):
        assert k == k2 and torch.equal(x, y), k


def _run(tr, seq, epochs):
    return [_floats(tr.training_step(b, meta=mt, cur_epoch=ep)) for (b, mt), ep in zip(seq, epochs)]


def test_eager_resume_with_dropout_equals_the_uninterrupted_run(ckdir):
    from druglamp_amd import ops
    bs = _batches()
    seq, eps = bs + bs, [1] * 6
    kw = dict(ema_decay=0.9)
    try:
        u = _make(0.1, **kw)
        lu = _run(u, seq, eps)
        r = _make(0.1, **kw)
        lr_ = _run(r, seq[:3], eps[:3])
        r.save_checkpoint(ckdir / "k3.pt")
        f = _fresh(0.1, **kw)
        f.load_checkpoint(ckdir / "k3.pt")
        lf = _run(f, seq[3:], eps[3:])
        f.check_device_flags()
    finally:
        ops.use_seed_offset(False)
    assert lr_ == lu[:3]
    assert lf == lu[3:], (lf, lu[3:])
    assert len({l["cls"] for l in lu}) == 6
    _assert_same(_state(u), _state(f))
    assert _counts(u) == _counts(f)


def test_resume_across_ssl_and_cm_steps_and_an_epoch_end(ckdir):
    """DrugLAMP2C2P: epoch 5 is the SSL epoch in which the CM head starts (cm_weight auto-scale, the SimSiam projectors are
    created, the MLM mask is drawn from torch's device generator), epochs 6 and 7 have the CM head, epoch 10 both again.  The
    epoch ends step the three schedulers and the head's margin schedule.  The save falls behind the first epoch end."""
    from druglamp_amd import ops
    bs = _batches()
    seq, eps = bs + bs, [1, 5, 6, 7, 10, 10]

    def first(tr):
        out = _run(tr, seq[:3], eps[:3])
        tr.on_train_epoch_end(6)
        return out

    def second(tr):
        out = _run(tr, seq[3:4], eps[3:4])
        tr.on_train_epoch_end(7)
        return out + _run(tr, seq[4:], eps[4:])

    def projectors(tr):
        return {k: v.detach().clone() for k, v in tr.model.state_dict().items() if ".projector." in k}
    try:
        u = _make(0.1, kind="DrugLAMP2C2P")
        lu = first(u) + second(u)
        r = _make(0.1, kind="DrugLAMP2C2P")
        first(r)
        r.save_checkpoint(ckdir / "k3.pt")
        f = _fresh(0.1, kind="DrugLAMP2C2P")
        assert not projectors(f)                                  # created lazily: the load builds them from the file
        f.load_checkpoint(ckdir / "k3.pt")
        _assert_same(projectors(r), projectors(f))
        lf = second(f)
        f.check_device_flags()
    finally:
        ops.use_seed_offset(False)
    assert [sorted(l) for l in lu] == [["cls"], ["cls", "cm", "ssl"], ["cls", "cm"], ["cls", "cm"], ["cls", "cm", "ssl"], ["cls", "cm", "ssl"]]
    assert lf == lu[3:], (lf, lu[3:])
    assert u.opt_ssl is not None and u.opt_cm is not None
    _assert_same(_state(u), _state(f))                            # (the moments of opt_ssl and opt_cm are part of _state)
    assert _counts(u) == _counts(f)
    assert len(projectors(u)) > 0
    _assert_same(projectors(u), projectors(f))


def test_graph_resume_without_dropout_equals_the_uninterrupted_run(ckdir):
    """Graph equals eager at pinned capacities (tests/test_graph_step_gpu.py), so the resumed trainer — two eager warm-up steps,
    then replays of a new capture — leaves the bits of the run that replayed throughout."""
    from druglamp_amd import ops
    bs = _batches()
    seq = (bs + bs + bs)[:8]
    eps = [1] * 8
    try:
        u = _make(0.0, True)
        caps = u.fixed_caps_for(seq)
        u.fixed_caps = caps
        lu = _run(u, seq, eps)
        r = _make(0.0, True)
        r.fixed_caps = caps
        _run(r, seq[:4], eps[:4])
        r.save_checkpoint(ckdir / "k4.pt")
        f = _fresh(0.0, True)
        f.fixed_caps = caps
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message="Trainer.load_checkpoint")     # same graph_steps, same fixed_caps: no warning
            f.load_checkpoint(ckdir / "k4.pt")
        lf = _run(f, seq[4:], eps[4:])
        f.check_device_flags()
        replays = sum(g.replays for g in f._graphs.values())
    finally:
        ops.use_seed_offset(False)
    assert sum(g.replays for g in u._graphs.values()) >= 6 and replays >= 2
    assert lf == lu[4:], (lf, lu[4:])
    _assert_same(_state(u), _state(f))
    assert _counts(u) == _counts(f)


def test_graph_resume_with_dropout_is_deterministic_given_the_file(ckdir):
    """With dropout on, a captured graph bakes the site seeds drawn when it was captured, and a trainer that loads captures anew:
    the resumed run is a correct continuation but NOT the bits of the uninterrupted run, so this test does not compare with
    one.  What holds: the round trip, and that the file determines what follows — two loads, the same steps, the same bits."""
    from druglamp_amd import ops
    bs = _batches()
    seq = (bs + bs + bs)[:8]
    eps = [1] * 8
    try:
        r = _make(0.1, True)
        _run(r, seq[:4], eps[:4])
        assert sum(g.replays for g in r._graphs.values()) == 2
        r.save_checkpoint(ckdir / "k4.pt")
        offset = int(ops.seed_offset_tensor(DEV))
        res = []
        for seed in (999, 555):
            f = _fresh(0.1, True, seed=seed)
            f.load_checkpoint(ckdir / "k4.pt")
            assert not f._graphs and not f._eager_seen and int(ops.seed_offset_tensor(DEV)) == offset > 0
            _assert_same(_state(r), _state(f))
            assert _counts(r) == _counts(f)
            losses = _run(f, seq[4:], eps[4:])
            assert sum(g.replays for g in f._graphs.values()) == 2
            res.append((losses, _state(f), _counts(f)))
    finally:
        ops.use_seed_offset(False)
    assert res[0][0] == res[1][0] and all(l["cls"] == l["cls"] for l in res[0][0])
    _assert_same(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]


def test_predicting_after_a_load_uses_the_loaded_weights(ckdir):
    """The low-precision weight images are cached per parameter epoch: a load that did not bump it would predict with the
    images of the weights it replaced.  A library built before the load is stale afterwards."""
    from druglamp_amd import ops
    from druglamp_amd.synthetic import make_batch
    bs = _batches()
    (vd, vp, _, xd, xp), _ = make_batch(4, DEV, seed=31, with_graph=False, llm_dtype=torch.bfloat16)
    try:
        a = _make(0.1)
        _run(a, bs, [1] * 3)
        pa = a.predict([bs[0][0]])[0].clone()
        a.save_checkpoint(ckdir / "a.pt")
        b = _fresh(0.1)
        pb0 = b.predict([bs[0][0]])[0].clone()                   # B's weight images exist and are current
        lib = b.build_library([(vd, xd)])
        assert b.screen_library([(vp, xp)], lib).shape == (4, 4)
        b.load_checkpoint(ckdir / "a.pt")
        pb = b.predict([bs[0][0]])[0]
        with pytest.raises(RuntimeError, match="parameter epoch"):
            b.screen_library([(vp, xp)], lib)
    finally:
        ops.use_seed_offset(False)
    assert not torch.equal(pb0, pa)
    assert torch.equal(pb, pa)


def test_refused_files_leave_the_trainer_untouched(ckdir):
    from druglamp_amd import ops
    from druglamp_amd.param_groups import ParamGroup
    b0, m0 = _batches((7,))[0]

    def saved(name, step=True, **kw):
        tr = _make(**kw)
        if step:
            tr.training_step(b0, meta=m0, cur_epoch=1)
        tr.save_checkpoint(ckdir / name)
        return ckdir / name

    def refused(tr, path, match):
        before, counts = _state(tr), _counts(tr)
        with pytest.raises(RuntimeError, match=match):
            tr.load_checkpoint(path)
        _assert_same(before, _state(tr))
        assert counts == _counts(tr)
    try:
        plain = saved("plain.pt")
        t = _fresh()
        t.training_step(b0, meta=m0, cur_epoch=1)                # (moments and step counts that a wrong write would change)
        refused(t, saved("ema.pt", ema_decay=0.9), "weight EMA is on in the file and off here")
        refused(t, saved("wollm.pt", step=False, kind="DrugLAMPwoLLM"),"the file holds a DrugLAMPwoLLM, the trainer a DrugLAMP")
        blob = torch.load(plain, map_location="cpu", weights_only=True)
        blob["format"] = 2
        torch.save(blob, ckdir / "format2.pt")
        refused(t, ckdir / "format2.pt", "format 2")
        data = plain.read_bytes()
        (ckdir / "half.pt").write_bytes(data[:len(data) // 2])
        refused(t, ckdir / "half.pt", "cannot be read")
        groups = [ParamGroup("no_decay", max_ndim=1, weight_decay=0.0)]
        g = _fresh(param_groups=[ParamGroup("no_decay", max_ndim=2, weight_decay=0.0)])
        refused(g, saved("groups.pt", param_groups=groups), "parameter-group assignment: entry")
        # an eager trainer's file in a graph-replaying trainer: the same state, a warning
        gt = _fresh(graph=True)
        with pytest.warns(UserWarning, match="graph_steps is False in the file and True here"):
            gt.load_checkpoint(plain)
        _assert_same(_state(_load_into_eager(plain)), _state(gt))
    finally:
        ops.use_seed_offset(False)


def _load_into_eager(path):
    tr = _fresh()
    tr.load_checkpoint(path)
    return tr


def _same_history(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y)
        for k in x:
            assert x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]), (k, x[k], y[k])


def test_fit_resumed_equals_fit_uninterrupted(ckdir):
    from druglamp_amd import ops
    from druglamp_amd.model import MInterface, load_reference_checkpoint
    from druglamp_amd.synthetic import make_batch
    train = _batches((7, 8))
    val, _ = make_batch(16, DEV, seed=2, with_graph=True, llm_dtype=torch.bfloat16)
    assert 0 < float(val[2].sum()) < 16                         # both labels present: the AUROC exists

    class Crash(Exception):
        pass

    def crash(ep, _val):
        if ep == 2:
            raise Crash()
    try:
        f = _make(0.1)
        rf = f.fit(lambda: train, lambda: [val], epochs=4, checkpoint_dir=ckdir / "f")
        g = _make(0.1)
        with pytest.raises(Crash):
            g.fit(lambda: train, lambda: [val], epochs=4, on_epoch=crash, checkpoint_dir=ckdir / "g")
        assert os.path.exists(ckdir / "g" / "last.pt")
        h = _fresh(0.1)
        rh = h.fit(lambda: train, lambda: [val], epochs=4, checkpoint_dir=ckdir / "g", resume=True)
    finally:
        ops.use_seed_offset(False)
    assert rf["epochs_run"] >= 2
    _same_history(rf["history"], rh["history"])
    assert (rf["best_epoch"], rf["epochs_run"]) == (rh["best_epoch"], rh["epochs_run"])
    assert rf["best_val_ausum"] == rh["best_val_ausum"]
    assert torch.equal(f.flat.arena, h.flat.arena)              # after the final reload of the best snapshot
    for name in ("f", "g"):
        torch.manual_seed(11)
        m = MInterface("DrugLAMP", f.cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
        assert not load_reference_checkpoint(m, str(ckdir / name / "best.pt"), strict=True).missing_keys
        p0 = next(iter(m.parameters()))
        assert torch.equal(p0, next(iter(f.model.parameters())))      # best.pt holds the best parameters: the ones fit reloaded
    assert torch.load(ckdir / "f" / "best.pt", map_location="cpu", weights_only=True)["extra"]["epoch"] == rf["best_epoch"]


def _kernel_launches(fn):
    """Device kernels launched by fn() (library and torch kernels alike; copies and memsets are not kernels)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sum(1 for n in names if not n.lower().startswith(("memcpy", "memset")))


def test_off_means_off(ckdir):
    """fit without checkpoint_dir writes nothing, and a trainer that saved launches what one that never did launches: the save
    leaves no hook, stream or flag behind."""
    from druglamp_amd import ops
    bs = _batches()
    val = bs[2][0]
    cwd = os.getcwd()
    try:
        os.chdir(ckdir)
        t = _make(0.1)
        t.fit(lambda: bs[:1], lambda: [val], epochs=1)
        assert os.listdir(ckdir) == []
        os.chdir(cwd)
        counts = []
        for save in (False, True):
            tr = _make(0.1, ema_decay=0.9, max_grad_norm=1.0)
            _run(tr, bs[:2], [1, 1])
            if save:
                tr.save_checkpoint(ckdir / "s.pt")
            torch.cuda.synchronize()
            counts.append(_kernel_launches(lambda: _run(tr, bs, [1] * 3)))
    finally:
        os.chdir(cwd)
        ops.use_seed_offset(False)
    assert counts[0] == counts[1] and counts[0] > 300, counts
