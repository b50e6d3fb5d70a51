"""Resident drug library: model.score_library (per-drug trimmed keys, dl_pgca_pairs_ragged_fwd) against model.score_codes on
DrugCode.cat of the same codes (one uniform layout, dl_pgca_pairs_fwd) over the same pairs, and the library's memory.

    python tools/library_bench.py --library [--out profiles/library_bench.txt] [--proteins 16] [--drugs 256] [--drug-batch 64] [--repeats 7]

Workload: bf16 DrugLAMP, the synthetic library of tools/screen_bench.py (make_batch seeds 1 and 2: drug graphs, LLM embeddings),
P proteins x D drugs, every pair scored drug-major in chunks of 256 pairs.  The drug batches are encoded under their
`drug_tokens` hint, so every code has the compact (136, 8, 48) layout: the baseline leg is the uniform path at its best.
--library  times the two legs (without it only the memory figures are printed).
Protocol: both legs run in one process on the same codes; one warm-up each, then `repeats` rounds with the legs alternating; a
leg's time is a host clock around the chunk loop, which ends in a device synchronise.  Medians are reported with min / max
(the run-to-run spread), the ratio, and the largest difference between the two legs' scores.
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
    ap.add_argument("--library", action="store_true", help="time score_library against score_codes")
    ap.add_argument("--out", default="")
    ap.add_argument("--proteins", type=int, default=16)
    ap.add_argument("--drugs", type=int, default=256)
    ap.add_argument("--drug-batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("library_bench: needs the GPU (a timing taken elsewhere says nothing)")
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.protein_plan import BatchHints
    from druglamp_amd.screening import DrugCode, DrugLibrary
    from druglamp_amd.synthetic import make_batch
    from druglamp_amd.trainer import Trainer
    P, D, PB = a.proteins, a.drugs, 256
    torch.manual_seed(0)
    cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
    m = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(DEV)
    m.set_compute_dtype(torch.bfloat16)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=torch.bfloat16)
    m.eval()
    (_, vp, _, _, xp), _ = make_batch(P, DEV, seed=1, with_graph=True, llm_dtype=torch.bfloat16)
    batch, meta = make_batch(D, DEV, seed=2, with_graph=True, llm_dtype=torch.bfloat16)
    (h, adj), _, _, xd, _ = batch
    hints = BatchHints(drug_tokens=Trainer.padding_hints_of(meta, batch).get("drug_tokens", 0), raw_attention=False)
    pcode = m.encode_proteins(vp, xp)
    codes = [m.encode_drugs((h[s:s + a.drug_batch], adj[s:s + a.drug_batch]), xd[s:s + a.drug_batch], hints) for s in range(0, D, a.drug_batch)]
    cat = DrugCode.cat(codes)
    lib = DrugLibrary.from_codes(codes, m)
    tr.check_device_flags()
    di = torch.arange(D).repeat_interleave(P)                             # drug-major, as Trainer.screen / screen_library
    pi = torch.arange(P).repeat(D)

    def chunks(score, code):
        return torch.cat([score(pcode, code, pi[s:s + PB], di[s:s + PB]) for s in range(0, P * D, PB)])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    text = ["resident drug library, bf16 DrugLAMP, %d drugs in batches of %d, %s" % (D, a.drug_batch, torch.cuda.get_device_name(0))]
    for k in sorted(lib.branches):
        nk = lib.keys(k).double()
        b = lib.branches[k]
        full = D * 512 * 256 * b.rows.element_size()
        own = sum(t.numel() * t.element_size() for t in (b.rows, b.row0, b.n_keys, b.tail_weight, b.bias))
        text.append("  branch %s: uniform layout %s; library keys per drug min %d / mean %.1f / max %d; %d bytes against %d at 512 keys "
                    "(%.2fx) and %d in the uniform layout (%.2fx)"
                    % (k, cat.layout(k), int(nk.min()), float(nk.mean()), int(nk.max()), own, full, full / own,
                       cat.branches[k].kv.numel() * b.rows.element_size(), cat.branches[k].kv.numel() * b.rows.element_size() / own))
    text.append("  lib.nbytes = %d; D x 512 x 512 B per branch = %d" % (lib.nbytes, len(lib.branches) * D * 512 * 512))
    if a.library:
        legs = [("library", lambda: chunks(m.score_library, lib)), ("codes", lambda: chunks(m.score_codes, cat))]
        outs = {name: timed(fn)[1] for name, fn in legs}                 # warm-up + the outputs that are compared
        diff = float((outs["library"] - outs["codes"]).abs().max())
        times = {name: [] for name, _ in legs}
        for _ in range(a.repeats):
            for name, fn in legs:
                times[name].append(timed(fn)[0])
        tr.check_device_flags()
        med = {k: statistics.median(v) for k, v in times.items()}
        text.append("score_library vs score_codes on DrugCode.cat, %d proteins x %d drugs = %d pairs, %d pairs per chunk; %d rounds, legs "
                    "alternating, one warm-up each" % (P, D, P * D, PB, a.repeats))
        for name, _ in legs:
            t = times[name]
            text.append("  %-8s %9.2f ms  (min %9.2f, max %9.2f)   %8.0f pairs/s" % (name, med[name], min(t), max(t), P * D / med[name] * 1e3))
        text.append("codes / library = %.3fx;  max |score_library - score_codes| = %.2e (bf16 pipeline)" % (med["codes"] / med["library"], diff))
    out = "\n".join(text) + "\n"
    print(out, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
