"""Timing of the shortlist prefilter (dl_latent_topk) and of a shortlisted screen.  Needs the MI355X.

    python tools/latent_topk_bench.py [--out profiles/latent_topk.txt] [--reps 7] [--skip-screen]

1. Kernel: ops.latent_topk at P = 1024, D = 2^20, M in {64, 1024}, bf16 and fp32, against a torch baseline on the same box:
   torch.topk(q @ L_chunk.T) over column chunks that fit memory, the chunks' lists merged with torch.topk (torch only, none of
   the code under test).  The two are run alternately, each call between a device event pair; the medians and their ratio are
   reported, with the kernel's share of the HBM roofline: bytes = one read of the library per 64-row query tile + the outputs,
   over the peak bandwidth, over the measured time.  (That is the bound the issue names; the launch is in fact closer to the
   matrix pipe's bound, which is printed beside it.)
2. End to end: Trainer.screen_library(top_k=10) exhaustive against shortlist=256 on one synthetic library (seed-0
   DrugLAMP2C2P, bf16; 256 synthetic drugs encoded once and stored 8 times over: 2048 library entries — the cost of a screen
   depends on the entry count and the key counts, not on the entries being different molecules).
No recall is reported: on untrained weights it means nothing (Trainer.shortlist_recall measures it on a trained model)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = torch.device("cuda", 0)
HBM_PEAK = 8.0e12            # bytes / s (MI355X, HBM3E)
MFMA_PEAK = {torch.bfloat16: 2.5e15, torch.float32: 157.3e12}     # dense FLOP / s of the matrix pipe per operand type


def unit_rows(n, dtype, seed, chunk=1 << 16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = torch.empty(n, 256, dtype=dtype, device=DEV)
    for r0 in range(0, n, chunk):
        x = torch.randn(min(chunk, n - r0), 256, generator=g, device=DEV)
        out[r0:r0 + x.shape[0]] = torch.nn.functional.normalize(x, dim=1).to(dtype)
    return out


def torch_topk(q, lib, M, chunk=1 << 16):
    best_v = best_i = None
    for c0 in range(0, lib.shape[0], chunk):
        s = (q @ lib[c0:c0 + chunk].t()).float()
        v, i = torch.topk(s, min(M, s.shape[1]), dim=1)
        i = i + c0
        if best_v is not None:
            v, i = torch.cat([best_v, v], dim=1), torch.cat([best_i, i], dim=1)
            v, sel = torch.topk(v, min(M, v.shape[1]), dim=1)
            i = torch.gather(i, 1, sel)
        best_v, best_i = v, i
    return best_v, best_i


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(a, b, reps):
    """Medians (ms) of a() and b() run alternately `reps` times after one warm-up each, and their last outputs."""
    a(), b()
    ta, tb = [], []
    for _ in range(reps):
        t, oa = timed(a)
        ta.append(t)
        t, ob = timed(b)
        tb.append(t)
    return statistics.median(ta), statistics.median(tb), min(ta), max(ta), min(tb), max(tb), oa, ob


def kernel_part(lines, reps):
    from druglamp_amd import ops
    P, D = 1024, 1 << 20
    lines.append("kernel: ops.latent_topk vs torch.topk(q @ L_chunk.T) merged over 65536-column chunks; P = %d, D = %d; median of %d "
                 "alternating runs (min .. max), device events" % (P, D, reps))
    for dtype in (torch.bfloat16, torch.float32):
        q, lib = unit_rows(P, dtype, 1), unit_rows(D, dtype, 2)
        es = q.element_size()
        for M in (64, 1024):
            tk, tt, k0, k1, t0, t1, (kv, ki), (tv, ti) = alternate(lambda: ops.latent_topk(q, lib, M), lambda: torch_topk(q, lib, M), reps)
            dv = float((kv - tv).abs().max())
            same = float((ki == ti).float().mean())
            nbytes = -(-P // 64) * D * 256 * es + P * M * 8
            flops = 2.0 * P * D * 256
            t_hbm, t_mfma = nbytes / HBM_PEAK * 1e3, flops / MFMA_PEAK[dtype] * 1e3
            lines.append("  %-8s M %4d: kernel %8.3f ms (%.3f .. %.3f)   torch %8.3f ms (%.3f .. %.3f)   torch / kernel = %.2f   "
                         "HBM bound %.3f ms = %.1f %% of the kernel time (%.1f GB; matrix-pipe bound %.3f ms = %.1f %%)   "
                         "max |value - torch| = %.2g, equal indices %.4f"
                         % (str(dtype).split(".")[1], M, tk, k0, k1, tt, t0, t1, tt / tk, t_hbm, 100 * t_hbm / tk, nbytes / 1e9,
                            t_mfma, 100 * t_mfma / tk, dv, same))
            print(lines[-1], flush=True)
        del q, lib
        torch.cuda.empty_cache()


def screen_part(lines, reps):
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.protein_plan import BatchHints
    from druglamp_amd.screening import DrugLibrary
    from druglamp_amd.synthetic import make_batch
    from druglamp_amd.trainer import Trainer
    torch.manual_seed(0)
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP2C2P")
    m = MInterface("DrugLAMP2C2P", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=torch.bfloat16)
    m.eval()
    hints = BatchHints(drug_tokens=128, raw_attention=False)
    codes, prots = [], None
    for b in range(4):
        (vd, vp, _, xd, xp), _ = make_batch(64, DEV, seed=100 + b, with_graph=False, llm_dtype=torch.bfloat16)
        codes.append(m.encode_drugs(vd, xd, hints))
        if prots is None:
            prots = [(vp[:8].clone(), xp[:8].clone())]
        del vd, vp, xd, xp
    lib = DrugLibrary.from_codes(codes * 8, m)
    D, k, M = lib.n, 10, 256
    ta, tb, a0, a1, b0, b1, _, _ = alternate(lambda: tr.screen_library(prots, lib, top_k=k), lambda: tr.screen_library(prots, lib, top_k=k, shortlist=M),
                                             max(5, reps - 2))
    lines.append("screen: Trainer.screen_library(top_k=%d), 8 proteins x %d library entries (%.1f MB resident), bf16, pair_batch 256: "
                 "exhaustive %.1f ms (%.1f .. %.1f)   shortlist=%d %.1f ms (%.1f .. %.1f)   exhaustive / shortlisted = %.2f"
                 % (k, D, lib.nbytes / 1e6, ta, a0, a1, M, tb, b0, b1, ta / tb))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-screen", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("latent_topk_bench: needs the GPU (a CPU run measures nothing)")
    if a.reps < 5:
        sys.exit("latent_topk_bench: at least five repetitions")
    lines = []
    kernel_part(lines, a.reps)
    if not a.skip_screen:
        screen_part(lines, a.reps)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
