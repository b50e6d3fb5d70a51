"""How NaN and +-inf pass through a kernel: the planting helper and the checker of tests/test_nonfinite_paths_gpu.py.
Plain torch, no GPU import: tests/test_nonfinite_reference_cpu.py runs everything here on the CPU.

The contract ("Non-finite values"): a non-finite value is never turned into a finite one on the way from a
kernel's inputs to its outputs, and it never leaks into outputs that do not depend on it.  A case runs an operation twice,
on clean operands and on the same operands with ONE element replaced (the plant), through the kernel and through the
repository's fp64 reference of the operation.  classify() sorts every output element by what the REFERENCE does:

    poisoned    the planted reference is not finite (and differs from the clean one)
    untouched   the planted reference equals the clean reference bit for bit
    moved       finite but different (only +-inf plants: a -inf logit becomes probability 0, an inf variance gives rstd 0)

and check_nonfinite() asserts, element by element,

    poisoned  => the kernel's planted output is not finite.  Where the reference is +-inf the kernel must give the same
                 infinity or NaN (never the other infinity; `inf_as_nan` counts the NaN).  Where the reference is NaN the
                 kernel must give NaN, unless the CASE allows an infinity and says why (allow_nan_as_inf: the polynomial
                 GELU of the bf16 epilogues gives -inf x 8e-6 = -inf where erf gives -inf x 0 = NaN; an NT-Xent row whose
                 every logit is NaN gives lse = -inf); such elements are counted (`nan_as_inf`) and recorded.
    untouched => the planted output equals the clean output BIT FOR BIT (every kernel here repeats bitwise, so no tolerance).
    moved     => finite, and within `bound_fn(moved mask)` of the planted reference where the case gives a bound (the family's
                 existing rounding bound without the planted operand's own magnitude terms); finite only where it cannot.

A case must not be vacuous: at least one poisoned and one untouched element over its outputs (assert_not_vacuous), decided
from the references alone.

DL_NONFINITE_LOG=<file>: every check appends one JSON line; tools/nonfinite_sites.py reduces the log to
profiles/nonfinite_sites.txt.
"""
import json
import os

import torch

F64 = torch.float64
NAN, INF = float("nan"), float("inf")
PLANT_NAMES = {"nan": NAN, "+inf": INF, "-inf": -INF}
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """The elements of t as integers of the same width (bitwise comparison: NaN == NaN, +0 != -0)."""
    t = t.contiguous()
    return t.view(_INT[t.element_size()])


def plant(t, index, value):
    """t[index] = value in place (index: a tuple into t, or a flat int); returns the value that was there."""
    if isinstance(value, str):
        value = PLANT_NAMES[value]
    if isinstance(index, int):
        index = tuple(int(i) for i in torch.unravel_index(torch.tensor(index), t.shape)) if t.dim() != 1 else (index,)
    old = t[index].clone()
    t[index] = value
    return old


def classify(ref_clean, ref_planted):
    """(poisoned, untouched, moved): boolean masks over the output, from the two references alone."""
    assert ref_clean.shape == ref_planted.shape and ref_clean.dtype == ref_planted.dtype
    untouched = (bits(ref_planted) == bits(ref_clean)).reshape(ref_clean.shape)       # (an infinity the clean data already holds, as in the
    poisoned = ~torch.isfinite(ref_planted) & ~untouched                               #  cast cases, is untouched data like any other)
    moved = ~poisoned & ~untouched
    return poisoned, untouched, moved


def counts(ref_clean, ref_planted):
    p, u, m = classify(ref_clean, ref_planted)
    return {"poisoned": int(p.sum()), "untouched": int(u.sum()), "moved": int(m.sum())}


def assert_not_vacuous(case, plant_name, pairs, masking=False, need_untouched=True):
    """pairs: (ref_clean, ref_planted) of every output of the case (for BatchNorm statistics and the scalar losses the
    untouched elements are in the OTHER channels / rows / outputs, so the requirement is over all outputs together).
    masking: a -inf plant that the operation reads as a mask (a masked class or token, a closed ReLU) poisons nothing by
    definition; it must move something instead, and the case's other plants carry the poisoned elements."""
    tot = {"poisoned": 0, "untouched": 0, "moved": 0}
    for a, b in pairs:
        for k, v in counts(a, b).items():
            tot[k] += v
    if masking:
        assert tot["poisoned"] + tot["moved"] > 0, "%s [%s]: vacuous, the plant changes nothing in the reference" % (case, plant_name)
    else:
        assert tot["poisoned"] > 0, "%s [%s]: vacuous, the plant poisons nothing in the reference" % (case, plant_name)
    # need_untouched=False: only where the case states that every output depends on every planted element (symmetric NT-Xent)
    assert tot["untouched"] > 0 or not need_untouched, "%s [%s]: vacuous, the reference has no output that is independent of the plant" % (case, plant_name)
    return tot


def _log(rec):
    path = os.environ.get("DL_NONFINITE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def check_nonfinite(case, form, what, got_clean, got_planted, ref_clean, ref_planted, bound_fn=None, plant_name="nan", allow_nan_as_inf=False):
    """See the header.  got_*: the kernel's output in its storage dtype; ref_*: fp64.  bound_fn(moved) -> the bound of the
    moved elements (a tensor of ref's shape, or a float), or None: moved elements are required to be finite only."""
    assert got_clean.shape == got_planted.shape == ref_clean.shape, "%s: %s shapes differ" % (case, what)
    assert got_clean.dtype == got_planted.dtype
    ref_clean, ref_planted = ref_clean.to(F64), ref_planted.to(F64)
    poisoned, untouched, moved = classify(ref_clean, ref_planted)
    g = got_planted.to(F64)
    tag = "%s [%s] %s, plant %s" % (case, form, what, plant_name)
    rec = {"case": case, "form": form, "output": what, "plant": plant_name, "poisoned": int(poisoned.sum()),
           "untouched": int(untouched.sum()), "moved": int(moved.sum()), "bounded": bound_fn is not None}
    ref_nan, ref_inf = poisoned & torch.isnan(ref_planted), poisoned & torch.isinf(ref_planted)
    rec["nan_as_inf"] = int((ref_nan & torch.isinf(g)).sum())
    rec["inf_as_nan"] = int((ref_inf & torch.isnan(g)).sum())
    swallowed = poisoned & torch.isfinite(g)
    wrong_inf = ref_inf & torch.isinf(g) & (g != ref_planted)
    leaked = untouched & (bits(got_planted) != bits(got_clean)).reshape(untouched.shape)
    bad_moved = moved & ~torch.isfinite(g)
    rec.update(swallowed=int(swallowed.sum()), leaked=int(leaked.sum()))
    _log(rec)
    print("%s: %d poisoned, %d untouched, %d moved; NaN as inf %d, inf as NaN %d" % (
        tag, rec["poisoned"], rec["untouched"], rec["moved"], rec["nan_as_inf"], rec["inf_as_nan"]))

    def first(mask):
        return tuple(int(i) for i in mask.nonzero()[0]) if mask.dim() else ()
    if bool(swallowed.any()):
        i = first(swallowed)
        raise AssertionError("%s: %d of %d poisoned elements came out finite (first at %s: reference %s, kernel %r)" % (
            tag, int(swallowed.sum()), rec["poisoned"], i, float(ref_planted[i]), float(g[i])))
    assert not bool(wrong_inf.any()), "%s: %d elements carry the other infinity" % (tag, int(wrong_inf.sum()))
    assert allow_nan_as_inf or rec["nan_as_inf"] == 0, "%s: %d elements are an infinity where the reference is NaN (the case does not allow it)" % (
        tag, rec["nan_as_inf"])
    if bool(leaked.any()):
        i = first(leaked)
        raise AssertionError("%s: %d of %d elements that do not depend on the plant changed (first at %s: clean %r, planted %r)" % (
            tag, int(leaked.sum()), rec["untouched"], i, float(got_clean[i]), float(g[i])))
    assert not bool(bad_moved.any()), "%s: %d moved elements are not finite where the reference is" % (tag, int(bad_moved.sum()))
    if bound_fn is not None and bool(moved.any()):
        b = bound_fn(moved)
        b = b if torch.is_tensor(b) else torch.full_like(ref_planted, float(b))
        err = (g - ref_planted).abs()[moved]
        ratio = float((err / (b.to(F64)[moved] + 1e-300)).max())
        assert ratio <= 1.0, "%s: a moved element exceeds its bound by x%.3g" % (tag, ratio)
    return rec
