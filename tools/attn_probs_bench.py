"""Attention probability maps: dl_attn_probs against the composition it replaces.

    python tools/attn_probs_bench.py [--out profiles/attn_probs_bench.txt] [--launches 20] [--repeats 7]

baseline   ops.attn_fwd(..., raw_logits=raw, need_lse=False) into a scratch O, then torch.softmax(raw, -1): the forward
           writes the fp32 logits, the softmax reads them and writes the map (three passes over the map, plus P.V and O)
probs      ops.attn_probs(lse=None): statistics kernel + one pass that writes the map
probs+lse  ops.attn_probs(lse=<the LSE of an attn_fwd call>): the map pass alone (what GuidedCrossAttentionFn issues)

Shapes: PGCA (B 256, 1 head of 128, Lq 256, Lk 512, head mean = the one head), the same map through compact keys (Lk 136,
tail (8, 47), expanded to 512 columns; its baseline is the 512-key composition, which is what a map cost before), and one
PMMA map (B 256, 4 heads of 64, L 256, per head).  bf16 operands.
Protocol: every variant runs over ROTATING buffer sets whose outputs together exceed the 256 MB last-level cache; warm-up
launches, then `launches` launches between two events, `repeats` times with the variants alternating; the median is reported
with min / max, the map's store bytes and the TB/s they imply, and the largest element difference between the variants' maps.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
SHAPES = [
    # name, B, H, hd, Lq, Lk (distinct keys), key_tail, head_mean
    ("pgca 256x512", 256, 1, 128, 256, 512, None, True),
    ("pgca compact 136 -> 512", 256, 1, 128, 256, 136, (8, 47), True),
    ("pmma 4 heads 256x256", 256, 4, 64, 256, 256, None, False),
]


def _time(fn, nsets, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(launches):
        fn(i % nsets)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches          # us per call


def bench_shape(name, B, H, hd, Lq, Lk, tail, mean, launches, repeats):
    from druglamp_amd import functional as Fn
    from druglamp_amd import ops
    d = H * hd
    scale = hd ** -0.5
    cols = Lk if tail is None else Lk - tail[0] + tail[0] * tail[1]
    map_bytes = B * (1 if mean else H) * Lq * cols * 4
    nsets = max(2, -(-3 * (256 << 20) // (2 * map_bytes)))     # outputs of all sets: at least 1.5 x the last-level cache
    g = torch.Generator(device=DEV).manual_seed(1)
    sets = []
    for _ in range(nsets):
        q = (torch.randn(B * Lq, d, device=DEV, generator=g) * 0.7).bfloat16()
        kv = (torch.randn(B, Lk, 2 * d, device=DEV, generator=g) * 0.7).bfloat16()
        kv_full = kv if tail is None else Fn.ExpandTailFn.apply(kv, Lk - tail[0], tail[1])
        s = {"q": q, "kv": kv.view(B * Lk, 2 * d), "kv_full": kv_full.reshape(B * cols, 2 * d),
             "raw": torch.empty((B, H, Lq, cols), dtype=torch.float32, device=DEV),
             "o": torch.empty((B * Lq, d), dtype=torch.bfloat16, device=DEV),
             "out": torch.empty((1, B, Lq, cols) if mean else (1, B, H, Lq, cols), dtype=torch.float32, device=DEV)}
        sets.append(s)
    qs = (Lq * d, hd, d)
    common = dict(n_problems=B, n_heads=H, n_segments=1, partner_shift=0, Lq=Lq, head_dim=hd, scale=scale, q_strides=qs)

    def fwd(s, keys, n, **kw):
        ks = (n * 2 * d, hd, 2 * d)
        return ops.attn_fwd(s["q"], keys, keys[:, d:], Lk=n, k_strides=ks, v_strides=ks, out=s["o"], o_strides=qs, o_ss=0,
                            **common, **kw)

    def baseline(i):
        s = sets[i]
        fwd(s, s["kv_full"], cols, need_lse=False, raw_logits=s["raw"])
        s["ref"] = torch.softmax(s["raw"], -1)

    def probs(i, lse=None):
        s = sets[i]
        ops.attn_probs(s["q"], s["kv"], Lk=Lk, k_strides=(Lk * 2 * d, hd, 2 * d), lse=lse, head_mean=mean, key_tail=tail,
                       expand_tail=tail is not None, out=s["out"], out_ld=cols, **common)

    for s in sets:
        s["lse"] = fwd(s, s["kv"], Lk, need_lse=True, key_tail=tail)
    variants = [("baseline", baseline), ("probs", probs), ("probs+lse", lambda i: probs(i, sets[i]["lse"]))]
    diffs = {}
    for vname, fn in variants:                                  # warm-up (every set) + agreement of the maps on set 0
        for i in range(nsets):
            fn(i)
        torch.cuda.synchronize()
        if vname != "baseline":
            diffs[vname] = float((sets[0]["out"].view(-1) - sets[0]["ref"].view(-1)).abs().max())
    times = {v: [] for v, _ in variants}
    for _ in range(repeats):
        for vname, fn in variants:
            times[vname].append(_time(fn, nsets, launches))
    lines = ["%s: B %d, H %d, head_dim %d, Lq %d, Lk %d%s -> %d columns, %s; map %.1f MB, %d buffer sets, %d launches x %d repeats"
             % (name, B, H, hd, Lq, Lk, "" if tail is None else " tail (%d, %d)" % tail, cols, "head mean" if mean else "per head",
                map_bytes / 1e6, nsets, launches, repeats)]
    base = statistics.median(times["baseline"])
    for vname, _ in variants:
        t = times[vname]
        med = statistics.median(t)
        lines.append("  %-10s %8.1f us  (min %8.1f, max %8.1f)   map stores %.2f TB/s   baseline / this = %.2fx%s"
                     % (vname, med, min(t), max(t), map_bytes / med / 1e6, base / med,
                        "" if vname == "baseline" else "   max |diff to baseline map| %.2e" % diffs[vname]))
    return lines, {v: statistics.median(t) for v, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_probs_bench: needs the GPU (a timing taken elsewhere says nothing)")
    text = ["attention probability maps: dl_attn_probs vs attn_fwd(raw_logits) + torch.softmax, bf16 operands, %s"
            % torch.cuda.get_device_name(0)]
    slower = []
    for shp in SHAPES:
        lines, med = bench_shape(*shp, a.launches, a.repeats)
        text += lines
        slower += ["%s/%s" % (shp[0], v) for v in ("probs", "probs+lse") if med[v] > med["baseline"]]
    text.append("slower than the baseline: %s" % (", ".join(slower) if slower else "none"))
    out = "\n".join(text) + "\n"
    print(out, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
