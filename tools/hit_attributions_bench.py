"""Hit attributions: one dl_pgca_pairs_ragged_attr launch against one dl_pgca_pairs_ragged_profile launch on the same pairs (the
attribution kernel does twice the MFMA work and reads twice the row bytes), and the wall time of Trainer.hit_attributions
against Trainer.hit_profiles for the same 256 hits (what the tail backward costs).

    python tools/hit_attributions_bench.py [--out profiles/hit_attributions.txt] [--launches 50] [--rounds 7] [--calls 5]

Launch shape (tools/hit_profiles_bench.py's): 256 pairs (16 proteins x 16 drugs of a library of 64, drug-major), Lq 256, library
drugs of 136 keys whose last 8 stand for 48 each (512 columns), bf16 codes filled with N(0, 0.7^2) values; d_out / d_sites the
halves of a (256, 256, 256) bf16 gradient of N(0, 0.05^2).  Device-resident index vectors, preallocated outputs.
Protocol: both legs in ONE process; warm-up of both, then `launches` calls between two device events per round, the legs
alternating, `rounds` rounds; a leg's figure is the median of its rounds (min / max printed).
Trainer legs: seed-0 DrugLAMP in bf16, make_batch(16, seed=31): 16 proteins (two batches of 8) x 16 hits (every drug of a
16-drug library), host wall time of a whole call (synchronised), the legs alternating, median of `calls` calls after one warm-up."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
N_P, N_D, PAIRS_P, PAIRS_D, LQ, LK, T, W, E = 16, 64, 16, 16, 256, 136, 8, 48, 128


def _time(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches          # us per call


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3              # ms


def _launch_legs(a, text):
    from druglamp_amd import ops
    g = torch.Generator(device=DEV).manual_seed(1)
    cols = LK - T + T * W
    n = PAIRS_P * PAIRS_D
    q = (torch.randn(N_P, LQ, E, device=DEV, generator=g) * 0.7).bfloat16()
    sites = (torch.randn(N_P, LQ, E, device=DEV, generator=g) * 0.7).bfloat16()
    rows = (torch.randn(N_D * LK, 2 * E, device=DEV, generator=g) * 0.7).bfloat16()
    grad = (torch.randn(n, LQ, 2 * E, device=DEV, generator=g) * 0.05).bfloat16()
    row0 = torch.arange(N_D, dtype=torch.int64, device=DEV) * LK
    n_keys = torch.full((N_D,), LK, dtype=torch.int32, device=DEV)
    tw = torch.full((N_D,), float(W), dtype=torch.float32, device=DEV)
    di = torch.arange(0, N_D, N_D // PAIRS_D).repeat_interleave(PAIRS_P).to(DEV, torch.int32)
    pi = torch.arange(PAIRS_P).repeat(PAIRS_D).to(DEV, torch.int32)
    p_out = (torch.empty((n, cols), device=DEV), torch.empty((n, LQ), device=DEV), torch.empty((n, LQ), device=DEV, dtype=torch.int32))
    a_out = (torch.empty((n, cols), device=DEV), torch.empty((n, LQ), device=DEV))

    def profile_launch():
        ops.pgca_pairs_ragged_profile(q, rows, row0, n_keys, tw, pi, di, scale=E ** -0.5, key_tail_rows=T, cols=cols, out=p_out)

    def attr_launch():
        ops.pgca_pairs_ragged_attr(q, rows, row0, n_keys, tw, grad[..., E:], pi, di, scale=E ** -0.5, key_tail_rows=T, cols=cols,
                                   sites=sites, d_sites=grad[..., :E], out=a_out)
    legs = [("profile launch", profile_launch), ("attr launch", attr_launch)]
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ops.check_guard_flags(torch.device(DEV))
    times = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            times[name].append(_time(fn, a.launches))
    text.append("%d pairs (%d proteins x %d drugs of a library of %d, drug-major), Lq %d, %d keys tail (%d, %d) -> %d columns, bf16; "
                "%d launches x %d rounds, legs alternating in one process (device events)" % (n, PAIRS_P, PAIRS_D, N_D, LQ, LK, T, W, cols, a.launches, a.rounds))
    med = {}
    for name, _ in legs:
        t = times[name]
        med[name] = statistics.median(t)
        text.append("  %-16s %8.1f us  (min %8.1f, max %8.1f)" % (name, med[name], min(t), max(t)))
    text.append("attr launch / profile launch = %.2fx" % (med["attr launch"] / med["profile launch"]))


def _trainer_legs(a, text):
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.synthetic import make_batch
    from druglamp_amd.trainer import Trainer
    dev = torch.device(DEV)
    torch.manual_seed(0)
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    m = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(dev)
    tr = Trainer(m, cfg, device=dev, compute_dtype=torch.bfloat16)
    m.eval()
    (vd, vp, _, xd, xp), _ = make_batch(16, dev, seed=31, with_graph=False)
    xd, xp = xd.bfloat16(), xp.bfloat16()
    prots = [(vp[:8], xp[:8]), (vp[8:], xp[8:])]
    lib = tr.build_library([(vd, xd)])
    idx = torch.arange(16).repeat(16, 1)
    legs = [("hit_profiles (v, pair_batch 256)", lambda: tr.hit_profiles(prots, lib, idx, branch="v")),
            ("hit_attributions (v + x, pair_batch 64)", lambda: tr.hit_attributions(prots, lib, idx)),
            ("hit_attributions (v + x, pair_batch 128)", lambda: tr.hit_attributions(prots, lib, idx, pair_batch=128))]
    for _, fn in legs:
        fn()
    times = {name: [] for name, _ in legs}
    for _ in range(a.calls):
        for name, fn in legs:
            times[name].append(_wall(fn))
    text.append("Trainer, 16 proteins (2 batches) x 16 hits = 256 hits, bf16, host wall time of a call incl. the protein encode; %d calls, legs alternating" % a.calls)
    med = {}
    for name, _ in legs:
        t = times[name]
        med[name] = statistics.median(t)
        text.append("  %-42s %8.1f ms  (min %8.1f, max %8.1f)" % (name, med[name], min(t), max(t)))
    text.append("hit_attributions (pair_batch 64) / hit_profiles = %.2fx" % (med[legs[1][0]] / med[legs[0][0]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hit_attributions_bench: needs the GPU (a timing taken elsewhere says nothing)")
    text = ["Hit attributions: dl_pgca_pairs_ragged_attr vs dl_pgca_pairs_ragged_profile, Trainer.hit_attributions vs hit_profiles, %s"
            % torch.cuda.get_device_name(0)]
    _launch_legs(a, text)
    _trainer_legs(a, text)
    out = "\n".join(text) + "\n"
    print(out, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
