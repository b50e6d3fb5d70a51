"""Hit profiles of (protein, drug) pairs from cached codes: model.cross_attn_profile_library (one dl_pgca_pairs_ragged_profile launch,
no map written) against the only route that existed before it — model.cross_attn_prob_library (the (N, n_site, 512) fp32 maps)
followed by mean(1) and max(-1) in torch on the device.

    python tools/hit_profiles_bench.py [--out profiles/hit_profiles.txt] [--launches 50] [--rounds 7]

Shape (the model's): 256 pairs (16 proteins x 16 drugs of a library of 64, drug-major), Lq 256, library drugs of 136 keys whose
last 8 stand for 48 each (512 columns), bf16 codes.  Both routes go through the model methods' checks (a stand-in model object:
the methods need its eval flag, compute dtype, branch set and head_dim only) on codes filled with N(0, 0.7^2) values, so that no
encoder runs.
Protocol: both legs in ONE process on the same pairs; warm-up of both, then `launches` calls between two device events per
round, the legs alternating, `rounds` rounds; the figure of a leg is the median of its rounds (min / max printed).  The two
route legs include the model methods' host work (checks, index upload, allocation), as a caller sees them; two further legs
time the two launches alone, on device-resident index vectors and preallocated outputs.  The map leg
rotates over output-sized allocations through torch's caching allocator as it does in use.
"""
import argparse
import os
import statistics
import sys
import types

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hit_profiles_bench: needs the GPU (a timing taken elsewhere says nothing)")
    from druglamp_amd import screening
    from druglamp_amd.model.basic_model import DrugLAMPBase
    g = torch.Generator(device=DEV).manual_seed(1)
    cols = LK - T + T * W
    n = PAIRS_P * PAIRS_D
    q = (torch.randn(N_P, LQ, E, device=DEV, generator=g) * 0.7).bfloat16()
    rows = (torch.randn(N_D * LK, 2 * E, device=DEV, generator=g) * 0.7).bfloat16()
    branch = types.SimpleNamespace(rows=rows, row0=torch.arange(N_D, dtype=torch.int64, device=DEV) * LK,
                                   n_keys=torch.full((N_D,), LK, dtype=torch.int32, device=DEV),
                                   tail_weight=torch.full((N_D,), float(W), dtype=torch.float32, device=DEV))
    epoch = screening.param_epoch()
    lib = types.SimpleNamespace(branches={"v": branch}, n=N_D, dtype=torch.bfloat16, epoch=epoch,
                                full_keys=lambda b: torch.full((N_D,), cols, dtype=torch.int64))
    pcode = types.SimpleNamespace(branches={"v": (None, q)}, n=N_P, dtype=torch.bfloat16, epoch=epoch)
    model = types.SimpleNamespace(compute_dtype=torch.bfloat16, llm_branch=False, v_gca=types.SimpleNamespace(head_dim=E),
                                  _need_eval=lambda who: None)
    for name in ("_check_pairs", "_pair_maps"):
        setattr(model, name, types.MethodType(getattr(DrugLAMPBase, name), model))
    model._no_profiles = DrugLAMPBase._no_profiles
    profile_fn = types.MethodType(DrugLAMPBase.cross_attn_profile_library.__wrapped__, model)
    maps_fn = types.MethodType(DrugLAMPBase.cross_attn_prob_library.__wrapped__, model)
    drugs = torch.arange(0, N_D, N_D // PAIRS_D)                                  # 16 drugs spread over the library
    di = drugs.repeat_interleave(PAIRS_P)                                         # drug-major, as screen_library orders a chunk
    pi = torch.arange(PAIRS_P).repeat(PAIRS_D)

    def profile():
        return profile_fn(pcode, lib, pi, di, cols=cols)

    def maps_then_reduce():
        m = maps_fn(pcode, lib, pi, di, cols=cols)
        peak, key = m.max(-1)
        return m.mean(1), peak, key

    # the two launches alone (index vectors already on the device, outputs preallocated): what the routes' kernels take
    from druglamp_amd import ops
    pi_d, di_d = pi.to(DEV, torch.int32), di.to(DEV, torch.int32)
    p_out = (torch.empty((n, cols), device=DEV), torch.empty((n, LQ), device=DEV), torch.empty((n, LQ), device=DEV, dtype=torch.int32))
    m_out = torch.empty((n, LQ, cols), device=DEV)
    tab = (rows, branch.row0, branch.n_keys, branch.tail_weight, pi_d, di_d)

    def profile_launch():
        ops.pgca_pairs_ragged_profile(q, *tab, scale=E ** -0.5, key_tail_rows=T, cols=cols, out=p_out)

    def maps_launch():
        ops.pgca_pairs_ragged_probs(q, *tab, scale=E ** -0.5, key_tail_rows=T, cols=cols, expand_tail=True, out=m_out)

    legs = [("profile", profile), ("maps+torch", maps_then_reduce)]
    launches_only = [("profile launch", profile_launch), ("maps launch", maps_launch)]
    with torch.no_grad():
        kept = {}
        for name, fn in legs:
            for _ in range(3):
                kept[name] = fn()
            torch.cuda.synchronize()
        d_mass = float((kept["profile"][0] - kept["maps+torch"][0]).abs().max())
        d_peak = float((kept["profile"][1] - kept["maps+torch"][1]).abs().max())
        # the parent route names a COLUMN (possibly a further copy of a tail key); the profile names the stored key
        col = kept["maps+torch"][2]
        stored = torch.where(col >= LK - T, LK - T + (col - (LK - T)) % T, col)
        same_key = float((stored == kept["profile"][2].long()).double().mean())
        del kept
        for _, fn in launches_only:
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in legs + launches_only}
        for _ in range(a.rounds):
            for name, fn in legs + launches_only:
                times[name].append(_time(fn, a.launches))
    prof_bytes = n * (cols + 2 * LQ) * 4
    map_bytes = n * LQ * cols * 4
    text = ["Hit profiles from cached codes: cross_attn_profile_library vs cross_attn_prob_library + mean(1) / max(-1) in torch, bf16 codes, %s"
            % torch.cuda.get_device_name(0),
            "%d pairs (%d proteins x %d drugs of a library of %d, drug-major), Lq %d, %d keys tail (%d, %d) -> %d columns; profiles %.2f MB "
            "written, maps %.1f MB written and read back twice; %d launches x %d rounds, legs alternating in one process (device events)"
            % (n, PAIRS_P, PAIRS_D, N_D, LQ, LK, T, W, cols, prof_bytes / 1e6, map_bytes / 1e6, a.launches, a.rounds)]
    med = {}
    for name, _ in legs + launches_only:
        t = times[name]
        med[name] = statistics.median(t)
        text.append("  %-14s %8.1f us  (min %8.1f, max %8.1f)" % (name, med[name], min(t), max(t)))
    text.append("maps+torch / profile = %.2fx; profile %s the parent route's median" % (
        med["maps+torch"] / med["profile"], "is below" if med["profile"] <= med["maps+torch"] else "EXCEEDS"))
    text.append("the launches alone (ONE output buffer each, so the maps launch writes into the last-level cache: not pair_maps_bench's "
                "rotating-buffer figure): maps launch / profile launch = %.2fx" % (med["maps launch"] / med["profile launch"]))
    text.append("max |key_mass diff| %.2e, max |site_peak diff| %.2e, site_key equal to the stored key of torch's argmax column on %.4f of the rows"
                % (d_mass, d_peak, same_key))
    out = "\n".join(text) + "\n"
    print(out, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
