"""Trainer checkpoints on two data-parallel ranks (gloo rendezvous, both on cuda:0, fresh child processes — the mould of
tests/test_graph_step_world2_gpu.py): every rank calls save_checkpoint and rank 0 writes; both ranks load the one file into
fresh trainers that were seeded differently per rank, find their own random state in it, and go on to the bits of a two-rank
run that was never interrupted.  The ranks see different data and, with dropout on, draw different masks: a load that gave
both ranks rank 0's generators would leave the uninterrupted run's bits.  A world-1 trainer refuses the file."""
import gc
import queue
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
STEPS, CUT = 4, 2


def _trainer(rank, seed):
    from druglamp_amd import ops
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    torch.manual_seed(seed + 17 * rank)                   # different initial weights per rank
    ops.manual_seed(seed + rank)                          # ... and different dropout site seeds
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    model = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(dev)
    model.pmma.p_drop = 0.1
    model.pmma.embeddings.p_drop = 0.1
    tr = Trainer(model, cfg, device=dev, compute_dtype=torch.bfloat16, graph_steps=False, ema_decay=0.9)
    tr.set_lrs(1e-3, 1e-3, 1e-3)
    return tr


def _steps(rank, dev, seq, path):
    """STEPS steps of a seed-1234 trainer; with a path the run is cut after CUT steps: save, fresh trainer, load, go on."""
    from druglamp_amd import ops
    tr = _trainer(rank, 1234)
    losses = []
    for k, (b, mt) in enumerate(seq):
        if path is not None and k == CUT:
            tr.save_checkpoint(path)                      # every rank calls; rank 0 writes; all leave once the file exists
            saved = tr.flat.arena.clone()
            del tr
            tr = _trainer(rank, 777)                      # fresh: other weights (synchronised to ITS rank 0's), other generators
            ops.next_seed()
            torch.rand(3 + rank, device=dev)
            assert not torch.equal(saved, tr.flat.arena)
            tr.load_checkpoint(path)
            assert torch.equal(saved, tr.flat.arena) and tr.replicas_in_sync()
        losses.append(float(tr.training_step(b, meta=mt, cur_epoch=1)["cls"]))
    torch.cuda.synchronize()
    return tr.flat.arena.detach().cpu().numpy(), tr.ema.shadow.detach().cpu().numpy(), losses, tr.replicas_in_sync()


def _worker(rank, world, port, path, q):
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    from druglamp_amd.synthetic import make_batch
    dev = torch.device("cuda:0")
    data = [make_batch(8, dev, seed=100 + 10 * k + rank, with_graph=True, llm_dtype=torch.bfloat16) for k in range(2)]
    seq = (data + data)[:STEPS]
    whole = _steps(rank, dev, seq, None)                  # (both runs start from the same seeds: _trainer sets every generator)
    resumed = _steps(rank, dev, seq, path)
    q.put((rank, whole, resumed))
    dist.destroy_process_group()


def _run(path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, path, q)) for r in range(2)]
    for p in procs:
        p.start()
    res, deadline = [], time.monotonic() + 300            # (the pair of ranks under its own time limit)
    try:
        while len(res) < 2:
            try:
                res.append(q.get(timeout=2))
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                if dead or time.monotonic() > deadline:
                    raise RuntimeError("the ranks did not finish (exit codes %s)" % [p.exitcode for p in procs])
        res.sort(key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(60 if p.exitcode is None else 1)
            if p.is_alive():
                p.kill()
    return res


def test_two_ranks_resume_from_one_file_to_the_bits_of_the_uninterrupted_run(tmp_path):
    path = str(tmp_path / "w2.pt")
    try:
        ranks = _run(path)
        whole, resumed = [r[1] for r in ranks], [r[2] for r in ranks]
        for res in (whole, resumed):
            assert res[0][3] and res[1][3]                                                     # replicas_in_sync
            assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
            assert res[0][2] != res[1][2]                                                      # the ranks saw different data
        for rank in range(2):
            assert whole[rank][2] == resumed[rank][2], (rank, whole[rank][2], resumed[rank][2])    # each rank's own masks came back
            assert np.array_equal(whole[rank][0], resumed[rank][0]) and np.array_equal(whole[rank][1], resumed[rank][1])
        assert np.isfinite(whole[0][0]).all()
        # a world-1 trainer refuses the file, before anything is written
        tr = _trainer(0, 4321)
        before = tr.flat.arena.clone()
        with pytest.raises(RuntimeError, match="world size is 2 in the file and 1 here"):
            tr.load_checkpoint(path)
        assert torch.equal(before, tr.flat.arena)
    finally:
        from druglamp_amd import ops
        ops.use_seed_offset(False)
        (tmp_path / "w2.pt").unlink(missing_ok=True)
        tr = None
        gc.collect()                                      # (the trainer's device memory goes now, not in the middle of a later test)
