"""fp64 restatement of the gradient guard (csrc/grad_guard.hip, the guarded AdamW step of csrc/optim.hip; contract in include/druglamp_hip.h): the sum of squares, the
finalize decision and the guarded AdamW step.  numpy / torch on the CPU; the scalars are the fp32 values the C ABI receives.
"""
import math

import numpy as np
import torch

from tests import elem_ref as er

F32_MAX = float(np.finfo(np.float32).max)


def sqnorm(g):
    """Sum of the EXACT squares of fp32 data in fp64 (an fp32 product has 48 significand bits: exact in fp64).  Up to 2^16
    elements the sum is correctly rounded (math.fsum); beyond, numpy's pairwise fp64 sum (error ~ log2(n) 2^-53 relative).
    A NaN or an infinity in the data gives a non-finite result (nan or inf)."""
    a = np.asarray(g.detach().cpu().numpy() if torch.is_tensor(g) else g, dtype=np.float32).reshape(-1).astype(np.float64)
    sq = a * a
    if not np.isfinite(sq).all():
        return float("nan") if np.isnan(sq).any() else float("inf")
    return math.fsum(sq.tolist()) if sq.size <= (1 << 16) else float(np.sum(sq))


def f32(x):
    """x rounded to fp32 (overflow to inf, as a C cast does), as a Python float."""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(x))


def finalize(acc, pre_scale=1.0, max_norm=0.0, skip_nonfinite=False):
    """acc (the fp64 sum) -> dict(coef, norm, skip, clipped, coef64, norm64): coef / norm / skip are guard[0..2] as fp32 values,
    coef64 / norm64 the doubles they were rounded from, clipped what counters[1] is incremented by."""
    pre_scale, max_norm = f32(pre_scale), f32(max_norm)
    nonfinite = not math.isfinite(acc)
    norm = pre_scale * math.sqrt(acc) if acc == acc and acc >= 0 else float("nan")
    coef = 1.0
    if max_norm > 0:
        c = max_norm / (norm + 1e-6)             # torch.nn.utils.clip_grad_norm_
        coef = 1.0 if c > 1.0 else c             # clamp(max=1): a NaN stays
    skip = bool(nonfinite and skip_nonfinite)
    return {"coef": 0.0 if skip else f32(coef), "norm": f32(norm), "skip": 1.0 if skip else 0.0,
            "clipped": int(coef < 1.0 and not skip), "coef64": coef, "norm64": norm}


def adamw_guarded(p, g, m, v, guard, lr, b1, b2, eps, wd, step, gscale):
    """guard = (coef, norm, skip): er.adamw with the fp32 gradient scale fl(gscale * coef); a skipped step returns p, m, v
    unchanged (in fp64)."""
    if guard[2] != 0:
        return p.double(), m.double(), v.double()
    eff = float(np.float32(gscale) * np.float32(guard[0]))
    return er.adamw(p, g, m, v, lr, b1, b2, eps, wd, step, eff)[:3]


def ulp32(x):
    """The spacing of fp32 numbers at |x| (numpy array or scalar); the smallest subnormal at 0."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)
