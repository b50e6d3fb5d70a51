"""Reduce a DL_NORM_BOUND_LOG file of tests/test_norm_paths_gpu.py to profiles/norm_bound_margins.txt: the worst |err| / bound
per kernel form, output and dtype, the ReLU kink shares and the rstd errors of the one-pass variance.

    DL_NORM_BOUND_LOG=log.jsonl pytest -m gpu tests/test_norm_paths_gpu.py
    python tools/norm_bound_margins.py log.jsonl profiles/norm_bound_margins.txt
"""
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_norm_paths_gpu as G  # noqa: E402

MARGIN = G.MARGIN
form = {}
for c in G.LN_CASES:
    form[c.name] = ("LayerNorm", c.fwd, c.bwd)
for c in G.BN_CASES:
    form[c.name] = ("BatchNorm",) + tuple(c.forms)
for c in G.RELU_CASES:
    form[c.name] = ("BatchNorm->ReLU",) + tuple(c.forms)
for c in G.TAIL_CASES:
    form[c.name] = ("tail fix",) + tuple(c.forms)
for c in G.E2E_CASES:
    form[c.name] = ("end to end", "BatchNormRowsFn" if c.fn == "rows" else "BatchNormWeightedTailFn")


def kernel(fam, forms, out):
    if fam == "LayerNorm":
        return forms[0] if out.split()[0] in ("y", "mean", "rstd", "y[const", "rstd[const") else forms[1]
    if fam == "BatchNorm":
        if out.startswith("stats_finalize"):
            return forms[0].replace("0/1", "0") + " + bn_reduce_finalize"
        if out.startswith("stats"):
            return forms[0].replace("0/1", "0") + " + reduce_partials"
        if out.startswith("finalize"):
            return "bn_finalize"
        if out.startswith("apply_fwd"):
            return forms[1]
        if out.startswith("bwd_reduce"):
            return forms[0].replace("0/1", "1") + " + reduce_partials"
        return forms[2]
    if fam == "BatchNorm->ReLU":
        return forms[0] if out.startswith("apply") else forms[2] if "dy" in out else forms[1]
    return forms[0]


worst = collections.OrderedDict()
kinks = collections.OrderedDict()
rel = collections.OrderedDict()
for line in open(sys.argv[1]):
    r = json.loads(line)
    fam, *forms = form[r["case"]]
    if r["output"].endswith("rstd relative error"):
        rel[(r["case"], r["output"])] = r["ratio"]
        continue
    if r["output"].endswith("kink share"):
        k = (fam, r["case"], r["output"])
        kinks[k] = max(kinks.get(k, 0.0), r["ratio"])
        continue
    k = (fam, kernel(fam, forms, r["output"]), r["output"], r["dtype"])
    if k not in worst or r["ratio"] > worst[k][0]:
        worst[k] = (r["ratio"], r["case"])

out = ["Worst |err| / bound of tests/test_norm_paths_gpu.py on an MI355X (gfx950), per kernel form, output and dtype",
       "(DL_NORM_BOUND_LOG of one run of `pytest -m gpu tests/test_norm_paths_gpu.py`; bounds carry MARGIN = %g, so a ratio at" % MARGIN,
       "or below %.2f stays inside the first-order rounding model itself; ratios above that pass and are marked '>1/MARGIN')." % (1 / MARGIN),
       "`<output> bias` rows are the scale-bias check (|s| / allowed).  Reduced from the log by tools/norm_bound_margins.py.", ""]
fam0 = None
for (fam, kern, what, dt), (ratio, case) in sorted(worst.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2], kv[0][3])):
    if fam != fam0:
        out += ["", "== %s ==" % fam, "%-52s %-34s %-8s %9s  %s" % ("form", "output", "dtype", "worst", "case")]
        fam0 = fam
    out.append("%-52s %-34s %-8s %9.4f  %s%s" % (kern, what, dt, ratio, case, "   >1/MARGIN" if ratio > 1 / MARGIN else ""))
above = [k for k, (r, _) in worst.items() if r > 1 / MARGIN]
out += ["", "Ratios between 1/MARGIN and 1: %s" % ("none: every form stays inside the first-order model" if not above else
                                                     "; ".join("%s %s %s" % (k[1], k[2], k[3]) for k in above))]
out += ["", "== ReLU kink: share of elements left out (cap %g) ==" % G.KINK_CAP]
nz = [(k, v) for k, v in kinks.items() if v > 0]
out.append("%d tensors checked, %d with any element left out, largest share %.3g" % (len(kinks), len(nz), max(kinks.values()) if kinks else 0.0))
for (fam, case, what), v in nz:
    out.append("%-40s %-34s %.3g" % (case, what, v))
out += ["", "End to end the band is 64 u_f (|yhat gamma| + |beta|) + |gamma| x (the bound of the error of the kernels' own yhat); shares there:"]
for (fam, case, what), v in kinks.items():
    if fam == "end to end":
        out.append("%-40s %-34s %.3g" % (case, what, v))
out += ["", "== one-pass variance E[y^2] - mean^2 in fp32: worst relative error of rstd itself, `offset` columns (8 + randn, mean / std ~ 8) ==",
        "(bounded relative to the second moment; post-ReLU conv outputs have mean / std ~ 1, the `relu` rows below)"]
for (case, what), v in rel.items():
    if "offset" in case or "relu" in case:
        out.append("%-40s %-38s %.3g" % (case, what, v))
open(sys.argv[2], "w").write("\n".join(out) + "\n")
print("\n".join(out))
