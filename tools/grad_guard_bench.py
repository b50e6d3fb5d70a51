"""Cost of the gradient guard on the MI355X (method of tools/ln_bench.py: back-to-back launches, wall clock per call).

  1. kernels on an arena of the model's size (14 026 568 fp32): ops.grad_sqnorm + ops.grad_guard_finalize (reads 4 B per
     element) next to ops.adamw_step and ops.adamw_step_guarded (28 B per element);
  2. the training step at batch 32, bf16, graph-replayed: guard off against max_grad_norm + skip_nonfinite, same process.
"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from druglamp_amd import ops
dev = torch.device("cuda:0")
def t(f, n=50):
    for _ in range(5): f()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n * 1e6
N = 14_026_568
xf = torch.randn(N, device=dev); gf = torch.randn_like(xf); m1 = torch.zeros_like(xf); m2 = torch.zeros_like(xf)
gg = ops.GradGuard(N, dev, max_norm=1.0, skip_nonfinite=True)
tsq = t(lambda: ops.grad_sqnorm(gf, gg.acc, gg.workspace))
tdec = t(lambda: gg.decide([gf]))
tad = t(lambda: ops.adamw_step(xf, gf, m1, m2, lr=1e-4, step=3))
tag = t(lambda: ops.adamw_step_guarded(xf, gf, m1, m2, gg.guard, lr=1e-4, step=3))
print("grad_sqnorm %d: %.1f us (%.2f TB/s)   sqnorm + finalize %.1f us   adamw %.1f us (%.2f TB/s)   adamw_guarded %.1f us (%.2f TB/s)" % (
    N, tsq, 4 * N / tsq / 1e6, tdec, tad, 28 * N / tad / 1e6, tag, 28 * N / tag / 1e6), flush=True)
print("guard pass / one adamw launch = %.3f (bytes: 4 / 28 = %.3f)" % (tdec / tad, 4 / 28), flush=True)
if "--no-step" not in sys.argv:
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.synthetic import make_batch
    from druglamp_amd.trainer import Trainer
    batch, meta = make_batch(32, dev, seed=100, with_graph=True, llm_dtype=torch.bfloat16)
    for kw in ({}, {"max_grad_norm": 1.0, "skip_nonfinite": True}):
        torch.manual_seed(0); ops.manual_seed(1)
        cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
        model = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(dev)
        tr = Trainer(model, cfg, device=dev, compute_dtype=torch.bfloat16, graph_steps=True, **kw)
        tr.set_lrs(1e-4, 1e-4, 1e-4)
        for _ in range(8): tr.training_step(batch, meta=meta, cur_epoch=1)
        ts, th = [], []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(100): tr.training_step(batch, meta=meta, cur_epoch=1)
            t1 = time.perf_counter()                    # (the host has enqueued everything: below the step time = the GPU is the bound)
            torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) / 100 * 1e3); th.append((t1 - t0) / 100 * 1e3)
        print("step batch 32 bf16 graph-replayed, guard %s: %s ms, host enqueue %s ms (replays %d)%s" % (
            "on " if kw else "off", " ".join("%.3f" % v for v in ts), " ".join("%.3f" % v for v in th), sum(g.replays for g in tr._graphs.values()),
            "  " + str(tr.grad_guard_stats()) if kw else ""), flush=True)
        del tr, model
