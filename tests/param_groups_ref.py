"""fp64 restatement of dl_adamw_step_groups (csrc/optim.hip) for the tests: tests/elem_ref.adamw with a learning rate and
a weight decay per 16-byte chunk.  As there, the scalars are first rounded to the fp32 values the C ABI receives; the group's
learning rate is the fp32 PRODUCT float32(lr) * float32(lr_scale) (the kernel's one fp32 multiply), the guarded gradient scale
the fp32 product float32(gscale) * float32(guard[0]); everything else is fp64."""
import math

import numpy as np
import torch


def f32(x) -> float:
    return float(np.float32(x))


def group_values(tab, lr):
    """Per group: (lr_k, wd_k) as Python floats holding fp32 values."""
    return [(float(np.float32(lr) * np.float32(row[0])), f32(row[1])) for row in np.asarray(tab, dtype=np.float64).reshape(-1, 2)]


def segments(quad_group, n):
    """Maximal segments of equal group id over n elements: [(start_elem, end_elem, id)]."""
    q = [int(k) for k in quad_group]
    assert len(q) == (n + 3) // 4
    out = []
    for c, k in enumerate(q):
        s, e = 4 * c, min(4 * c + 4, n)
        if out and out[-1][2] == k:
            out[-1] = (out[-1][0], e, k)
        else:
            out.append((s, e, k))
    return out


def adamw_groups(p, g, m, v, quad_group, tab, lr, b1, b2, eps, step, gscale, guard=None):
    """Returns p', m', v' (fp64).  quad_group: ceil(n / 4) ids; tab: (G, 2) {lr_scale, weight_decay}; guard: None or the 4 values
    {coef, norm, skip, 0}.  Chunks whose id is >= G, and everything on a skipped step, come back unchanged."""
    p, g, m, v = (t.detach().cpu().double().clone() for t in (p, g, m, v))
    n = p.numel()
    if guard is not None:
        gd = [f32(x) for x in guard]
        if gd[2] != 0.0:
            return p, m, v
        gscale = float(np.float32(gscale) * np.float32(gd[0]))
    else:
        gscale = f32(gscale)
    b1, b2, eps = f32(b1), f32(b2), f32(eps)
    vals = group_values(tab, lr)
    ids = torch.as_tensor([int(k) for k in quad_group], dtype=torch.int64).repeat_interleave(4)[:n]
    live = ids < len(vals)
    safe = ids.clamp(max=len(vals) - 1)
    lr_e = torch.tensor([a for a, _ in vals], dtype=torch.float64)[safe]
    wd_e = torch.tensor([b for _, b in vals], dtype=torch.float64)[safe]
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    grad = g * gscale
    m1 = b1 * m + (1 - b1) * grad
    v1 = b2 * v + (1 - b2) * grad * grad
    den = v1.sqrt() / bc2s + eps
    x = p * (1 - lr_e * wd_e) - (lr_e / bc1) * (m1 / den)
    return torch.where(live, x, p), torch.where(live, m1, m), torch.where(live, v1, v)
