"""Reduce a DL_NONFINITE_LOG file of tests/test_nonfinite_paths_gpu.py to profiles/nonfinite_sites.txt: per launch form and
plant kind (nan / +inf / -inf) the cases that ran it, the number of planted runs, and the class counts of their outputs
(poisoned / untouched / moved by the fp64 reference), how many poisoned elements the kernel returned as the other kind of
non-finite value (NaN where the reference has an infinity and the reverse; both are non-finite and pass), and how many it
swallowed or leaked (both fail the test: a committed table has zeros there).  Only what the log holds.

    DL_NONFINITE_LOG=log.jsonl pytest -m gpu tests/test_nonfinite_paths_gpu.py
    python tools/nonfinite_sites.py log.jsonl profiles/nonfinite_sites.txt
"""
import collections
import json
import sys

rows = collections.OrderedDict()
for line in open(sys.argv[1]):
    r = json.loads(line)
    kind = r["plant"].rsplit("=", 1)[-1]
    k = (r["case"].split("/")[0], r["form"], kind)
    t = rows.setdefault(k, {"cases": collections.OrderedDict(), "plants": set(), "poisoned": 0, "untouched": 0, "moved": 0, "nan_as_inf": 0,
                            "inf_as_nan": 0, "swallowed": 0, "leaked": 0, "bounded": 0})
    t["cases"][r["case"].split("/", 1)[1]] = True
    t["plants"].add((r["case"], r["plant"]))
    for f in ("poisoned", "untouched", "moved", "nan_as_inf", "inf_as_nan", "swallowed", "leaked"):
        t[f] += r[f]
    t["bounded"] += int(bool(r["bounded"]) and r["moved"] > 0)

out = ["How NaN and +-inf pass through every launch form: tests/test_nonfinite_paths_gpu.py on an MI355X (gfx950), one row per family,",
       "form and plant kind (DL_NONFINITE_LOG of one run of `pytest -m gpu tests/test_nonfinite_paths_gpu.py`).  Element counts are sums",
       "over the outputs of all planted runs of the row; classes by the fp64 reference (poisoned: not finite, untouched: bitwise the clean",
       "value, moved: finite but changed).  NaN>inf / inf>NaN: poisoned elements the kernel returned as the other non-finite kind (pass).",
       "swallowed / leaked fail the test.  Reduced from the log by tools/nonfinite_sites.py.", "",
       "%-10s %-5s %6s %10s %11s %8s %8s %8s %9s %7s  %s" % ("family", "plant", "runs", "poisoned", "untouched", "moved", "NaN>inf", "inf>NaN",
                                                              "swallowed", "leaked", "form  <-  cases")]
for (fam, form, kind), t in rows.items():
    out.append("%-10s %-5s %6d %10d %11d %8d %8d %8d %9d %7d  %s  <-  %s" % (
        fam, kind, len(t["plants"]), t["poisoned"], t["untouched"], t["moved"], t["nan_as_inf"], t["inf_as_nan"], t["swallowed"], t["leaked"],
        form, " ".join(t["cases"])))
bad = [k for k, t in rows.items() if t["swallowed"] or t["leaked"]]
vac = [k for k, t in rows.items() if k[2] != "-inf" and t["poisoned"] == 0]
out += ["", "Rows with swallowed or leaked elements: %s" % ("none" if not bad else "; ".join("%s %s %s" % k for k in bad)),
        "NaN / +inf rows without a poisoned element: %s" % ("none" if not vac else "; ".join("%s %s %s" % k for k in vac)),
        "", "The sites that were fixed and the ones left alone: DESIGN.md, \"Non-finite values\"."]
open(sys.argv[2], "w").write("\n".join(out) + "\n")
print("\n".join(out))
