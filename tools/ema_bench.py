"""Cost of the weight EMA on the MI355X (method of tools/grad_guard_bench.py: back-to-back launches, wall clock per call).

  1. kernels on the trainer's own arena (14 026 568 fp32 for the DrugLAMP config): ops.ema_update (12 B per element: reads the
     shadow and the arena, writes the shadow) and ops.adamw_step (28 B per element), timed ALTERNATING in one process — blocks
     of 50 launches of one, then of the other, five rounds — so that the two are measured in the same run;
  2. the training step at batch 32, bf16, graph-replayed: EMA off against ema_decay=0.999, same process.
"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from druglamp_amd import ops
from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
from druglamp_amd.model import MInterface
from druglamp_amd.synthetic import make_batch
from druglamp_amd.trainer import Trainer
dev = torch.device("cuda:0")
def t(f, n=50):
    for _ in range(5): f()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n * 1e6
def trainer(**kw):
    torch.manual_seed(0); ops.manual_seed(1)
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    model = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(dev)
    tr = Trainer(model, cfg, device=dev, compute_dtype=torch.bfloat16, graph_steps=True, **kw)
    tr.set_lrs(1e-4, 1e-4, 1e-4)
    return tr
tr = trainer(ema_decay=0.999)
N = tr.flat.numel
arena, shadow, grads = tr.flat.arena, tr.ema.shadow, torch.randn_like(tr.flat.arena) * 1e-3
m1, m2 = tr.opt.exp_avg, tr.opt.exp_avg_sq
guard = torch.tensor([1.0, 1.0, 0.0, 0.0], device=dev)
skip = torch.tensor([0.0, 1.0, 1.0, 0.0], device=dev)
te, ta = [], []
for _ in range(5):
    te.append(t(lambda: ops.ema_update(shadow, arena, 1e-3)))
    ta.append(t(lambda: ops.adamw_step(arena, grads, m1, m2, lr=1e-6, step=3)))
tg = t(lambda: ops.ema_update(shadow, arena, 1e-3, guard))
ts_ = t(lambda: ops.ema_update(shadow, arena, 1e-3, skip))
me, ma = sorted(te)[2], sorted(ta)[2]
print("arena %d fp32" % N, flush=True)
print("ema_update  %s us  (median %.1f us, 12 B/element: %.2f TB/s)" % (" ".join("%.1f" % v for v in te), me, 12 * N / me / 1e6), flush=True)
print("adamw_step  %s us  (median %.1f us, 28 B/element: %.2f TB/s)" % (" ".join("%.1f" % v for v in ta), ma, 28 * N / ma / 1e6), flush=True)
print("ema_update with a guard %.1f us, on a skipped step %.1f us" % (tg, ts_), flush=True)
print("ema pass / one adamw launch = %.3f (bytes: 12 / 28 = %.3f)" % (me / ma, 12 / 28), flush=True)
del tr, arena, shadow, grads, m1, m2
if "--no-step" not in sys.argv:
    batch, meta = make_batch(32, dev, seed=100, with_graph=True, llm_dtype=torch.bfloat16)
    for kw in ({}, {"ema_decay": 0.999}):
        tr = trainer(**kw)
        for _ in range(8): tr.training_step(batch, meta=meta, cur_epoch=1)
        ts, th = [], []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(100): tr.training_step(batch, meta=meta, cur_epoch=1)
            t1 = time.perf_counter()                    # (the host has enqueued everything: below the step time = the GPU is the bound)
            torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) / 100 * 1e3); th.append((t1 - t0) / 100 * 1e3)
        print("step batch 32 bf16 graph-replayed, EMA %s: %s ms, host enqueue %s ms (replays %d)" % (
            "on " if kw else "off", " ".join("%.3f" % v for v in ts), " ".join("%.3f" % v for v in th), sum(g.replays for g in tr._graphs.values())), flush=True)
        del tr
