"""Reduce a DL_LOSS_BOUND_LOG file of tests/test_loss_paths_gpu.py to profiles/loss_bound_margins.txt: the worst |err| / bound
per kernel form, output and dtype, and the cases that name each form.

    DL_LOSS_BOUND_LOG=log.jsonl pytest -m gpu tests/test_loss_paths_gpu.py
    python tools/loss_bound_margins.py log.jsonl profiles/loss_bound_margins.txt
"""
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_loss_paths_gpu as G  # noqa: E402

MARGIN = G.MARGIN


def family(form):
    return ("NT-Xent" if form.startswith("ntx") else "cosine row loss" if form.startswith("cos") else
            "cross entropy rows" if form.startswith("ce_") else "triplet sig-cos")


worst = collections.OrderedDict()
cases = collections.OrderedDict()
for line in open(sys.argv[1]):
    r = json.loads(line)
    k = (family(r["form"]), r["form"], r["output"], r["dtype"])
    if k not in worst or r["ratio"] > worst[k][0]:
        worst[k] = (r["ratio"], r["case"])
    cases.setdefault((k[0], r["form"]), collections.OrderedDict())[r["case"].split(" ")[0]] = True

out = ["Worst |err| / bound of tests/test_loss_paths_gpu.py on an MI355X (gfx950), per kernel form, output and dtype",
       "(DL_LOSS_BOUND_LOG of one run of `pytest -m gpu tests/test_loss_paths_gpu.py`; bounds carry MARGIN = %g, so a ratio at" % MARGIN,
       "or below %.2f stays inside the first-order rounding model itself; ratios above that pass and are marked '>1/MARGIN')." % (1 / MARGIN),
       "`<output> bias` rows are the scale-bias check (|s| / allowed).  Reduced from the log by tools/loss_bound_margins.py."]
fam0 = None
for (fam, form, what, dt), (ratio, case) in sorted(worst.items(), key=lambda kv: kv[0]):
    if fam != fam0:
        out += ["", "== %s ==" % fam, "%-44s %-20s %-9s %9s  %s" % ("form", "output", "dtype", "worst", "case")]
        fam0 = fam
    out.append("%-44s %-20s %-9s %9.4f  %s%s" % (form, what, dt, ratio, case, "   >1/MARGIN" if ratio > 1 / MARGIN else ""))
above = [k for k, (r, _) in worst.items() if r > 1 / MARGIN]
out += ["", "Ratios between 1/MARGIN and 1: %s" % ("none: every form stays inside the first-order model" if not above else
                                                     "; ".join("%s %s %s" % (k[1], k[2], k[3]) for k in above))]
out += ["", "== form -> cases =="]
for (fam, form), cs in sorted(cases.items()):
    out.append("%-44s %s" % (form, " ".join(cs)))
open(sys.argv[2], "w").write("\n".join(out) + "\n")
print("\n".join(out))
