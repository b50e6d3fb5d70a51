"""A malformed batch must RAISE: the device-side padding guards (csrc/compact.hip) end to end — from the model's forward at
its default switches into the sticky device word, and from there through the trainer: the poll at the head of the next step,
check_device_flags at an epoch boundary, graph replays, and the closing checks of evaluate / screen / build_library.

Every malformed batch is malformed as data only: one padding node, one token row beyond the hinted block, one residue of a
later period, a residue count that is off by one.  Shapes, indices and tables are those of the clean batch.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32, BF = torch.float32, torch.bfloat16

T_PERIOD = "not tiled with the period"
T_TOKEN = "token rows beyond the hinted block"
T_NODE = "not identical virtual padding nodes"


def _trainer(graph, dt):
    from druglamp_amd import ops
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.trainer import Trainer
    torch.manual_seed(5)
    ops.manual_seed(77)
    ops.seed_offset_tensor(DEV).zero_()
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    m = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    m.pmma.p_drop = 0.0
    m.pmma.embeddings.p_drop = 0.0
    m.drug_extractor.compact_min_rows = 0          # (a batch of 8: take the compact MolecularGCN form — and its guard — anyway)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=dt, graph_steps=graph)
    tr.set_lrs(1e-4, 3e-5, 1e-5)
    ops.guard_flags(DEV).zero_()                   # (the sticky word may carry a bit an earlier test provoked on purpose)
    return tr


def _batch(dt, seed=7):
    from druglamp_amd.synthetic import make_batch
    batch, meta = make_batch(8, DEV, seed=seed, with_graph=True, llm_dtype=dt)
    assert max(m_["Drug_Tokens"] for m_ in meta) <= 128 and max(m_["Drug_Tokens"] for m_ in meta) > 64
    return batch, meta


def bad_node(batch):
    (h, adj), vp, y, xd, xp = batch
    h = h.clone()
    assert adj.shape[1] == 128 and float(h[2, 300, 5]) == 0.0
    h[2, 300, 5] = 1                               # a padding node (beyond the 128-node adjacency block) that is no virtual node
    return ((h, adj), vp, y, xd, xp)


def bad_token(batch):
    (h, adj), vp, y, xd, xp = batch
    xd = xd.clone()
    assert float(xd[3, 400].abs().sum()) == 0.0
    xd[3, 400, 7] = 1                              # a token row beyond the hinted block of 128
    return ((h, adj), vp, y, xd, xp)


def bad_residue(batch, meta):
    (h, adj), vp, y, xd, xp = batch
    vp = vp.clone()
    t = meta[1]["Prot_Len"] + 2 + 3                # residue 2 of the SECOND period
    assert 2 * (meta[1]["Prot_Len"] + 2) <= vp.shape[1] and float(vp[1, t]) == float(vp[1, 3])
    vp[1, t] = 25 if float(vp[1, t]) != 25 else 24
    return ((h, adj), vp, y, xd, xp)


def bad_length(meta):
    meta = copy.deepcopy(meta)
    meta[1]["Prot_Len"] += 1                        # a wrong length record: the tables are built for another period
    return meta


def _word():
    from druglamp_amd import ops
    return int(ops.guard_flags(DEV).item())


def _replays(tr):
    return sum(g.replays for g in tr._graphs.values())


# ---- the model's forward at its default switches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_each_guard_trips_with_its_own_bit_and_text(dt):
    from druglamp_amd import _lib, ops
    tr = _trainer(False, dt)
    m = tr.model
    assert m.guard_padding and m.drug_extractor.guard_padding and not m.check_padding and not m.drug_extractor.check_padding
    batch, meta = _batch(dt)

    def forward(b, mt):
        hints = tr.hints_of(mt, b)
        assert hints.drug_tokens == 128 and hints.protein_plan is not None
        with torch.no_grad():
            m(b[0], b[1], b[3], b[4], hints=hints)

    forward(batch, meta)
    assert _word() == 0                                               # the clean batch is quiet
    ops.check_guard_flags(DEV)
    launches = 3
    for bad, mt, bit, text in ((bad_node(batch), meta, _lib.FLAG_GCN_NODE_PAD, T_NODE),
                               (bad_token(batch), meta, _lib.FLAG_DRUG_TOKEN_PAD, T_TOKEN),
                               (bad_residue(batch, meta), meta, _lib.FLAG_PROT_PERIOD, T_PERIOD),
                               (batch, bad_length(meta), _lib.FLAG_PROT_PERIOD, T_PERIOD)):
        forward(bad, mt)
        launches += 3
        assert _word() == bit, (text, _word())                        # exactly that bit, before it is cleared
        with pytest.raises(RuntimeError, match="padding guard tripped — .*" + text) as e:
            ops.check_guard_flags(DEV)
        assert sum(t in str(e.value) for t in (T_NODE, T_TOKEN, T_PERIOD)) == 1
        assert _word() == 0                                           # cleared by the raise
    # sticky across forwards: a clean forward in between clears nothing, a second trip adds its bit
    forward(bad_node(batch), meta)
    forward(batch, meta)
    assert _word() == _lib.FLAG_GCN_NODE_PAD
    forward(bad_token(batch), meta)
    assert _word() == _lib.FLAG_GCN_NODE_PAD | _lib.FLAG_DRUG_TOKEN_PAD
    with pytest.raises(RuntimeError, match=T_TOKEN + ".*" + T_NODE):
        ops.check_guard_flags(DEV)
    assert _word() == 0
    # guard_padding = False: the drug guards are quiet on the same input (the period guard has no switch of its own)
    m.guard_padding = m.drug_extractor.guard_padding = False
    forward(bad_node(batch), meta)
    forward(bad_token(batch), meta)
    assert _word() == 0
    forward(bad_residue(batch, meta), meta)
    assert _word() == _lib.FLAG_PROT_PERIOD
    ops.guard_flags(DEV).zero_()
    print("model forward %s: %d guard launches" % (dt, launches + 9 + 1))


# ---- the trainer, eager ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_eager_steps_deliver_a_trip_at_the_next_step_and_at_the_epoch_end(dt):
    tr = _trainer(False, dt)
    batch, meta = _batch(dt)
    tr.training_step(batch, meta=meta, cur_epoch=1)
    for bad, mt, text in ((bad_node(batch), meta, T_NODE), (bad_token(batch), meta, T_TOKEN),
                          (bad_residue(batch, meta), meta, T_PERIOD), (batch, bad_length(meta), T_PERIOD)):
        # (synchronise first: the poll at the head of the bad step then consumes the previous step's copy of the word, and the
        #  bad step posts its own — one copy is in flight at a time)
        torch.cuda.synchronize()
        out = tr.training_step(bad, meta=mt, cur_epoch=1)              # the malformed step itself does not raise
        assert torch.is_tensor(out["cls"])
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="tripped in an earlier step — .*" + text):
            tr.training_step(batch, meta=meta, cur_epoch=1)
        assert _word() == 0
        tr.training_step(batch, meta=meta, cur_epoch=1)                # the step after that runs clean
        tr.check_device_flags()
    # the last step of an epoch is the bad one: the epoch boundary raises
    torch.cuda.synchronize()
    tr.training_step(bad_node(batch), meta=meta, cur_epoch=1)
    with pytest.raises(RuntimeError, match="padding guard tripped — .*" + T_NODE):
        tr.on_train_epoch_end(1)
    assert _word() == 0
    # ... once: the copy of the word that the bad step posted for the next poll was delivered by that raise
    tr.training_step(batch, meta=meta, cur_epoch=1)
    torch.cuda.synchronize()
    tr.training_step(batch, meta=meta, cur_epoch=1)
    tr.check_device_flags()


# ---- the trainer, captured -------------------------------------------------------------------------------------------------------
def test_a_graph_replay_on_a_malformed_batch_trips_the_guards():
    from druglamp_amd import ops
    batch, meta = _batch(BF)
    bad = bad_residue(bad_token(bad_node(batch)), meta)                # same shapes, same meta: the same graph key
    try:
        tr = _trainer(True, BF)
        for _ in range(tr.graph_warmup + 2):
            tr.training_step(batch, meta=meta, cur_epoch=1)
        tr.check_device_flags()
        caps, reps = tr.graph_captures, _replays(tr)
        assert caps == 1 and len(tr._graphs) == 1 and reps >= 1
        tr.training_step(bad, meta=meta, cur_epoch=1)
        assert (tr.graph_captures, _replays(tr)) == (caps, reps + 1)   # a replay, no new capture
        with pytest.raises(RuntimeError, match="padding guard tripped — .*" + T_PERIOD + ".*" + T_TOKEN + ".*" + T_NODE):
            tr.check_device_flags()
        assert _word() == 0
        # ... and through the next step's poll
        tr.training_step(batch, meta=meta, cur_epoch=1)
        torch.cuda.synchronize()
        tr.training_step(bad, meta=meta, cur_epoch=1)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="tripped in an earlier step — .*" + T_PERIOD + ".*" + T_TOKEN + ".*" + T_NODE):
            tr.training_step(batch, meta=meta, cur_epoch=1)
        assert _word() == 0
        tr.training_step(batch, meta=meta, cur_epoch=1)
        tr.check_device_flags()
        assert tr.graph_captures == caps and _replays(tr) == reps + 4
    finally:
        ops.use_seed_offset(False)


# ---- the no-grad paths -----------------------------------------------------------------------------------------------------------
def test_evaluate_screen_and_build_library_raise_at_their_closing_check():
    from druglamp_amd.protein_plan import BatchHints
    tr = _trainer(False, BF)
    batch, meta = _batch(BF)
    (h, adj), vp, y, xd, xp = batch
    (hb, _), _, _, _, _ = bad_node(batch)
    assert 0 < float(y.sum()) < y.numel()
    with pytest.raises(RuntimeError, match="padding guard tripped — .*" + T_NODE):
        tr.evaluate([bad_node(batch)])
    assert _word() == 0
    assert "loss" in tr.evaluate([batch])                             # a clean call afterwards succeeds
    with pytest.raises(RuntimeError, match="padding guard tripped — .*" + T_NODE):
        tr.screen([(vp, xp)], [((hb, adj), xd)])
    assert _word() == 0
    assert tuple(tr.screen([(vp, xp)], [((h, adj), xd)]).shape) == (8, 8)
    # a hint that claims a drug-token block smaller than a molecule's token count
    with pytest.raises(RuntimeError, match="padding guard tripped — .*" + T_TOKEN):
        tr.build_library([((h, adj), xd)], hints=BatchHints(drug_tokens=64))
    assert _word() == 0
    assert tr.build_library([((h, adj), xd)], hints=BatchHints(drug_tokens=128)).n == 8
    tr.check_device_flags()
