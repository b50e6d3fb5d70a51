"""Reduce a DL_ELEM_BOUND_LOG file of tests/test_elem_paths_gpu.py to profiles/elem_bound_margins.txt: the worst |err| / bound
per kernel form, output and dtype (bit-exact checks log 0), the cases that name each form, and the measured error of the
rational GELU' fit (tests/test_elem_reference_cpu.py measures it on the CPU).

    DL_ELEM_BOUND_LOG=log.jsonl pytest -m gpu tests/test_elem_paths_gpu.py
    python tools/elem_bound_margins.py log.jsonl profiles/elem_bound_margins.txt
"""
import collections
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import elem_ref as er  # noqa: E402
from tests import test_elem_paths_gpu as G  # noqa: E402

MARGIN = G.MARGIN

worst = collections.OrderedDict()
cases = collections.OrderedDict()
for line in open(sys.argv[1]):
    r = json.loads(line)
    k = (r["form"], r["output"], r["dtype"])
    if k not in worst or r["ratio"] > worst[k][0]:
        worst[k] = (r["ratio"], r["case"])
    cases.setdefault(r["form"], collections.OrderedDict())[r["case"].split(" ")[0].split("[")[0]] = True

out = ["Worst |err| / bound of tests/test_elem_paths_gpu.py on an MI355X (gfx950), per kernel form, output and dtype",
       "(DL_ELEM_BOUND_LOG of one run of `pytest -m gpu tests/test_elem_paths_gpu.py`; bounds carry MARGIN = %g, so a ratio at" % MARGIN,
       "or below %.2f stays inside the first-order rounding model itself; ratios above that pass and are marked '>1/MARGIN';" % (1 / MARGIN),
       "0.0000 rows are bit-exact comparisons).  Reduced from the log by tools/elem_bound_margins.py.", "",
       "%-48s %-22s %-6s %9s  %s" % ("form", "output", "dtype", "worst", "case")]
for (form, what, dt), (ratio, case) in sorted(worst.items(), key=lambda kv: kv[0]):
    out.append("%-48s %-22s %-6s %9.4f  %s%s" % (form, what, dt, ratio, case, "   >1/MARGIN" if ratio > 1 / MARGIN else ""))
above = [k for k, (r, _) in worst.items() if r > 1 / MARGIN]
out += ["", "Ratios between 1/MARGIN and 1: %s" % ("none: every form stays inside the first-order model" if not above else
                                                     "; ".join("%s %s %s" % k for k in above))]
x = np.linspace(-12.0, 12.0, 2400001)
err = np.abs(er.gelu_grad_rational_f32(x).astype(np.float64) - er.gelu_grad(torch.from_numpy(x))[0].numpy())
out += ["", "== measured constant ==",
        "gelu_grad_fast2 (rational GELU' of the bf16 pipelines) in fp32 arithmetic against fp64 GELU', 2400001 points over [-12, 12]:",
        "worst |error| %.4e at |x| = %.3f (the bound's absolute term is %.1e; tests/test_elem_reference_cpu.py asserts the measurement)"
        % (float(err.max()), float(abs(x[err.argmax()])), G.E_G_FAST)]
out += ["", "== form -> cases =="]
for form, cs in sorted(cases.items()):
    out.append("%-48s %s" % (form, " ".join(cs)))
open(sys.argv[2], "w").write("\n".join(out) + "\n")
print("\n".join(out))
