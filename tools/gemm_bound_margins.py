"""Reduce a DL_GEMM_BOUND_LOG file of tests/test_gemm_paths_gpu.py to profiles/gemm_bound_margins.txt: the worst |err| / bound
per launch form and output, and the cases that run each form.

    DL_GEMM_BOUND_LOG=log.jsonl pytest -m gpu tests/test_gemm_paths_gpu.py
    python tools/gemm_bound_margins.py log.jsonl profiles/gemm_bound_margins.txt

Everything from the line `== notes ==` of an existing output file on is hand-written (the explanation of the ratios, the
mutation check) and is kept as it is; only the tables above it are rewritten.
"""
import collections
import json
import os
import sys

NOTES = "== notes =="
FAMILIES = [("k128", "gemm_kernel (128 x 128 / 64 x 64 tiles), split-K slabs included"), ("big256", "gemm_big_kernel 256 x 256"),
            ("lat128", "gemm_big_kernel few-tile 128 x 128 deep ring"), ("tt2", "gemm_big_tt2_kernel"), ("group", "dl_gemm_group"),
            ("pair", "dl_gemm_pair shared launch"), ("colsum", "dl_colsum")]


def family(form):
    return next(i for i, (k, _) in enumerate(FAMILIES) if form.startswith(k))


def reduce_log(lines):
    worst, cases, margin = {}, {}, None
    for line in lines:
        r = json.loads(line)
        assert margin in (None, r["margin"]), "the log mixes runs with different MARGIN"
        margin = r["margin"]
        k = (family(r["form"]), r["form"], r["output"])
        if k not in worst or r["ratio"] > worst[k][0]:
            worst[k] = (r["ratio"], r["case"])
        cases.setdefault((k[0], r["form"]), collections.OrderedDict())[r["case"].split("/")[0]] = True
    return worst, cases, margin


def render(worst, cases, margin):
    out = ["Worst |err| / bound of tests/test_gemm_paths_gpu.py on an MI355X (gfx950), per launch form and output",
           "(DL_GEMM_BOUND_LOG of one run of `pytest -m gpu tests/test_gemm_paths_gpu.py`; bounds carry MARGIN = %g, so a ratio at" % margin,
           "or below %.2f stays inside the first-order rounding model itself; ratios above that pass and are marked '>1/MARGIN')." % (1 / margin),
           "`<output> bias` rows are the scale-bias check (|s| / allowed).  The form text is that of gemm_ref.select() (see the header of",
           "the test file).  Reduced from the log by tools/gemm_bound_margins.py."]
    fam0 = None
    for (fam, form, what), (ratio, case) in sorted(worst.items()):
        if fam != fam0:
            out += ["", "== %s ==" % FAMILIES[fam][1], "%-52s %-14s %9s  %s" % ("form", "output", "worst", "case")]
            fam0 = fam
        out.append("%-52s %-14s %9.4f  %s%s" % (form, what, ratio, case, "   >1/MARGIN" if ratio > 1 / margin else ""))
    above = ["%s %s" % (k[1], k[2]) for k, (r, _) in sorted(worst.items()) if r > 1 / margin]
    out += ["", "Ratios between 1/MARGIN and 1: %s" % ("; ".join(above) or "none: every form stays inside the first-order model")]
    out += ["", "== form -> cases =="]
    for (fam, form), cs in sorted(cases.items()):
        out.append("%-52s %s" % (form, " ".join(cs)))
    return out


def main(log, dst):
    out = render(*reduce_log(open(log)))
    if os.path.exists(dst):
        old = open(dst).read().split("\n")
        if NOTES in old:
            out += [""] + old[old.index(NOTES):]
    text = "\n".join(out).rstrip("\n") + "\n"
    open(dst, "w").write(text)
    print(text, end="")


if __name__ == "__main__":
    main(*sys.argv[1:3])
