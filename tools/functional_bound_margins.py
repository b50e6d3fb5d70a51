"""Reduce a DL_FN_BOUND_LOG file of tests/test_functional_paths_gpu.py to profiles/functional_bound_margins.txt: the FORMS
table (every autograd Function branch, the condition that selects it, the cases or the tests of other suites that pin it, the
worst |err| / bound among its cases) and, per case, the tensor that came closest to its bound (bit-exact comparisons log 0).

    DL_FN_BOUND_LOG=log.jsonl pytest -m gpu tests/test_functional_paths_gpu.py
    python tools/functional_bound_margins.py log.jsonl profiles/functional_bound_margins.txt
"""
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import fn_ref as R  # noqa: E402

worst = collections.OrderedDict()          # case -> (ratio, tensor, n tensors, dtype)
by_form = collections.OrderedDict()        # form -> {case: worst ratio}
for line in open(sys.argv[1]):
    r = json.loads(line)
    w = worst.get(r["case"])
    worst[r["case"]] = (max(r["ratio"], w[0]) if w else r["ratio"], r["tensor"] if (not w or r["ratio"] > w[0]) else w[1], (w[2] if w else 0) + 1,
                        r["dtype"])
    for f in r["forms"]:
        d = by_form.setdefault(f, collections.OrderedDict())
        d[r["case"]] = max(d.get(r["case"], 0.0), r["ratio"])

out = ["Worst |err| / bound of tests/test_functional_paths_gpu.py on an MI355X (gfx950): bound = K x row envelope of the plain",
       "compute-dtype evaluation against the fp64 reference (K = %g bf16, %g fp32; tests/fn_ref.py), so a ratio of 1 / K is the plain" % (R.K_BOUND[R.BF], R.K_BOUND[R.F32]),
       "evaluation's own distance; 0.0000 rows are bit-exact comparisons only.  DL_FN_BOUND_LOG of one run, reduced by",
       "tools/functional_bound_margins.py.", "", "== FORMS: Function branch, worst ratio, condition, cases =="]
for form, cond in R.FORMS.items():
    if form in by_form:
        cs = by_form[form]
        out.append("%-40s %7.4f  %s" % (form, max(cs.values()), cond))
        out.append("%-40s          cases: %s" % ("", " ".join(cs)))
    elif form in R.ELSEWHERE:
        out.append("%-40s       -  %s" % (form, cond))
        out.append("%-40s          pinned by: %s" % ("", " ".join(R.ELSEWHERE[form])))
    else:
        out.append("%-40s       -  %s" % (form, cond))
        out.append("%-40s          NOT COMPARED: %s" % ("", R.OPEN.get(form, "no case in this log")))
out += ["", "== cases: worst tensor ==", "%-40s %-6s %8s  %-24s %s" % ("case", "dtype", "worst", "tensor", "tensors compared")]
for case, (ratio, tensor, n, dt) in worst.items():
    out.append("%-40s %-6s %8.4f  %-24s %d" % (case, dt, ratio, tensor, n))
top = max(worst.items(), key=lambda kv: kv[1][0])
out += ["", "Largest ratio: %.4f (%s, %s); %d cases, %d comparisons." % (top[1][0], top[0], top[1][1], len(worst), sum(v[2] for v in worst.values()))]
open(sys.argv[2], "w").write("\n".join(out) + "\n")
print("\n".join(out))
