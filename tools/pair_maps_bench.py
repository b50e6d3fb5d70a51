"""PGCA attention maps of (protein, drug) pairs from cached codes: dl_pgca_pairs_ragged_probs against the only route from codes
that existed before it, and against the floor its algorithmic bytes set.

    python tools/pair_maps_bench.py [--out profiles/pair_maps.txt] [--launches 20] [--repeats 7]

pair maps  ops.pgca_pairs_ragged_probs(expand_tail=True): one launch, operands read in place through the index vectors
gather     the route without it: q[pi] and the drugs' key rows gathered into dense tensors (torch.index_select), then
           ops.attn_probs(lse=None, expand_tail=True) on them (statistics kernel + map kernel) — possible only because every
           drug of this library has the same layout; the gathers are part of the route and are timed with it
floor      (the fp32 map written + every distinct protein's q and every distinct drug's keys read once) / the HBM peak

Shape (the model's): 256 pairs (16 proteins x 16 drugs of a library of 64, drug-major), Lq 256, library drugs of 136 keys whose
last 8 stand for 48 each, expanded to 512 columns, bf16 operands.
Protocol: every variant runs over ROTATING output buffers that together exceed the 256 MB last-level cache; warm-up launches
of every variant on every buffer, then `launches` launches between two device events, `repeats` times with the variants
alternating; the median is reported with min / max and the map's store bytes over it.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
HBM_PEAK, HBM_MEASURED = 8.0e12, 6.29e12      # bytes / s: the spec peak and the measured float4 copy rate (MI355X)
N_P, N_D, PAIRS_P, PAIRS_D, LQ, LK, T, W, E = 16, 64, 16, 16, 256, 136, 8, 48, 128


def _time(fn, nsets, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(launches):
        fn(i % nsets)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pair_maps_bench: needs the GPU (a timing taken elsewhere says nothing)")
    from druglamp_amd import ops
    g = torch.Generator(device=DEV).manual_seed(1)
    scale = E ** -0.5
    cols = LK - T + T * W
    n = PAIRS_P * PAIRS_D
    q = (torch.randn(N_P, LQ, E, device=DEV, generator=g) * 0.7).bfloat16()
    rows = (torch.randn(N_D * LK, 2 * E, device=DEV, generator=g) * 0.7).bfloat16()
    row0 = torch.arange(N_D, dtype=torch.int64, device=DEV) * LK
    n_keys = torch.full((N_D,), LK, dtype=torch.int32, device=DEV)
    tw = torch.full((N_D,), float(W), dtype=torch.float32, device=DEV)
    drugs = torch.arange(0, N_D, N_D // PAIRS_D)                                  # 16 drugs spread over the library
    di = drugs.repeat_interleave(PAIRS_P).to(DEV, torch.int32)                    # drug-major, as screen_library orders a chunk
    pi = torch.arange(PAIRS_P).repeat(PAIRS_D).to(DEV, torch.int32)
    pi_rows = pi.long()
    key_rows = (row0[di.long()].view(-1, 1) + torch.arange(LK, device=DEV)).reshape(-1)
    map_bytes = n * LQ * cols * 4
    read_bytes = PAIRS_P * LQ * E * 2 + PAIRS_D * LK * E * 2
    nsets = max(2, -(-3 * (256 << 20) // (2 * map_bytes)))                        # outputs of all sets: at least 1.5 x the last-level cache
    outs = [torch.empty((n, LQ, cols), dtype=torch.float32, device=DEV) for _ in range(nsets)]

    def pair_maps(i):
        ops.pgca_pairs_ragged_probs(q, rows, row0, n_keys, tw, pi, di, scale=scale, key_tail_rows=T, cols=cols, expand_tail=True, out=outs[i])

    def gather(i):
        qg = q.index_select(0, pi_rows)
        kg = rows.index_select(0, key_rows)                                       # (n * LK, 256): [K | V'] rows as stored
        ops.attn_probs(qg, kg, n_problems=n, n_heads=1, n_segments=1, partner_shift=0, Lq=LQ, Lk=LK, head_dim=E, scale=scale,
                       q_strides=(LQ * E, E, E), k_strides=(LK * 2 * E, E, 2 * E), lse=None, head_mean=True, key_tail=(T, float(W)),
                       expand_tail=True, out=outs[i].view(1, n, LQ, cols), out_ld=cols)

    variants = [("pair maps", pair_maps), ("gather", gather)]
    kept = {}
    for vname, fn in variants:                                                    # warm-up (every buffer) + agreement on buffer 0
        for i in range(nsets):
            fn(i)
        torch.cuda.synchronize()
        kept[vname] = outs[0].clone()
    diff = float((kept["pair maps"] - kept["gather"]).abs().max())
    rowsum = float((kept["pair maps"].double().sum(-1) - 1).abs().max())
    del kept
    times = {v: [] for v, _ in variants}
    for _ in range(a.repeats):
        for vname, fn in variants:
            times[vname].append(_time(fn, nsets, a.launches))
    floor_us = (map_bytes + read_bytes) / HBM_PEAK * 1e6
    text = ["PGCA pair maps from cached codes: dl_pgca_pairs_ragged_probs vs gather + dl_attn_probs, bf16 operands, %s" % torch.cuda.get_device_name(0),
            "%d pairs (%d proteins x %d drugs of a library of %d, drug-major), Lq %d, %d keys tail (%d, %d) -> %d columns; map %.1f MB, "
            "operands read once %.2f MB, %d output buffers, %d launches x %d repeats (device events, medians)"
            % (n, PAIRS_P, PAIRS_D, N_D, LQ, LK, T, W, cols, map_bytes / 1e6, read_bytes / 1e6, nsets, a.launches, a.repeats)]
    med = {}
    for vname, _ in variants:
        t = times[vname]
        med[vname] = statistics.median(t)
        text.append("  %-10s %8.1f us  (min %8.1f, max %8.1f)   map stores %.2f TB/s   floor / this = %.2f"
                    % (vname, med[vname], min(t), max(t), map_bytes / med[vname] / 1e6, floor_us / med[vname]))
    text.append("  %-10s %8.1f us  = (%.1f MB written + %.2f MB read) / %.1f TB/s HBM peak (%.1f us at the measured %.2f TB/s copy rate)"
                % ("floor", floor_us, map_bytes / 1e6, read_bytes / 1e6, HBM_PEAK / 1e12, (map_bytes + read_bytes) / HBM_MEASURED * 1e6,
                   HBM_MEASURED / 1e12))
    text.append("gather / pair maps = %.2fx; bound: the map's stores (%.1f%% of the algorithmic bytes); max |pair maps - gather| %.2e, "
                "worst |row sum - 1| %.2e" % (med["gather"] / med["pair maps"], 100.0 * map_bytes / (map_bytes + read_bytes), diff, rowsum))
    out = "\n".join(text) + "\n"
    print(out, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
