"""Library screening: Trainer.screen against Trainer.predict over the same pairs.

    python tools/screen_bench.py [--out profiles/screen_bench.txt] [--proteins 16] [--drugs 256] [--drug-batch 64] [--repeats 5]

Workload: bf16 DrugLAMP, P proteins x D drugs from synthetic.make_batch (drug graphs, LLM embeddings), every pair scored.
screen    Trainer.screen: protein codes once, drug batches of --drug-batch streamed, 256 pairs per chunk
predict   Trainer.predict over the same P * D explicit pairs in batches of 256, inputs gathered and resident beforehand (the
          whole forward per pair: the path every pair took before)
Protocol: both legs run in one process on the same weights; one warm-up each, then `repeats` rounds with the legs alternating;
a leg's time is a host clock around a call that ends in a device synchronise (both end with check_device_flags).  Medians are
reported with min / max, the ratio, and the largest difference between the two legs' probabilities.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = torch.device("cuda", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--proteins", type=int, default=16)
    ap.add_argument("--drugs", type=int, default=256)
    ap.add_argument("--drug-batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("screen_bench: needs the GPU (a timing taken elsewhere says nothing)")
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.synthetic import make_batch
    from druglamp_amd.trainer import Trainer
    P, D, PB = a.proteins, a.drugs, 256
    torch.manual_seed(0)
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    m = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    m.set_compute_dtype(torch.bfloat16)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=torch.bfloat16)
    (_, vp, _, _, xp), _ = make_batch(P, DEV, seed=1, with_graph=True, llm_dtype=torch.bfloat16)
    ((h, adj), _, _, xd, _), _ = make_batch(D, DEV, seed=2, with_graph=True, llm_dtype=torch.bfloat16)
    prot_batches = [(vp, xp)]
    drug_batches = [((h[s:s + a.drug_batch], adj[s:s + a.drug_batch]), xd[s:s + a.drug_batch]) for s in range(0, D, a.drug_batch)]
    # the explicit pairs in Trainer.screen's order (drug-major), gathered once and resident
    di = torch.arange(D, device=DEV).repeat_interleave(P)
    pi = torch.arange(P, device=DEV).repeat(D)
    y = torch.zeros(P * D, device=DEV)
    pairs = []
    for s in range(0, P * D, PB):
        d_, p_ = di[s:s + PB], pi[s:s + PB]
        pairs.append(((h[d_], adj[d_]), vp[p_], y[s:s + PB], xd[d_], xp[p_]))

    def screen():
        return tr.screen(prot_batches, drug_batches, pair_batch=PB)

    def predict():
        return tr.predict(pairs)[0].view(D, P).t()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    legs = [("screen", screen), ("predict", predict)]
    outs = {name: timed(fn)[1] for name, fn in legs}                   # warm-up + the outputs that are compared
    diff = float((outs["screen"] - outs["predict"]).abs().max())
    times = {name: [] for name, _ in legs}
    for _ in range(a.repeats):
        for name, fn in legs:
            times[name].append(timed(fn)[0])
    med = {k: statistics.median(v) for k, v in times.items()}
    text = ["library screening: Trainer.screen vs Trainer.predict, bf16 DrugLAMP, %d proteins x %d drugs = %d pairs, %s"
            % (P, D, P * D, torch.cuda.get_device_name(0)),
            "drug batches of %d, %d pairs per chunk / per predict batch; %d rounds, legs alternating, one warm-up each"
            % (a.drug_batch, PB, a.repeats)]
    for name, _ in legs:
        t = times[name]
        text.append("  %-8s %9.1f ms  (min %9.1f, max %9.1f)   %8.0f pairs/s" % (name, med[name], min(t), max(t), P * D / med[name] * 1e3))
    text.append("predict / screen = %.2fx;  max |p_screen - p_predict| = %.2e (bf16 pipeline)" % (med["predict"] / med["screen"], diff))
    out = "\n".join(text) + "\n"
    print(out, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
