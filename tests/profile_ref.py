"""fp64 reference of the hit profiles (dl_pgca_pairs_profile / dl_pgca_pairs_ragged_profile, include/druglamp_hip.h) and their
bounds, as reductions of an fp64 probability map and of its element bound.

The map `pm` (..., Lq, cols) is the expanded map of tests/attn_ref.reference_fwd (as tests/test_pgca_pairs_probs_gpu._drug_map lays
it out: copy i of tail key j at column lead + i t + j, zeros behind a drug's own F columns) and `b` its element bound
    b[r, c] = 2 ref ((hd + 2) u_f (lam + mag_lse) + (F + 8) u_f) + 2^-120,     u_f = 2^-24
(0 in the zero-fill columns).  No new tolerance:
    key_mass [c] = (1 / Lq) sum_r pm[r, c]     |got - ref| <= (1 / Lq) sum_r b[r, c] + (Lq + 8) u_f ref + 2^-120
                   (a mean of bounded errors plus an fp32 sum of Lq non-negative terms and one division)
    site_peak[r] = max_c pm[r, c]              |got - ref| <= max_c b[r, c]
                   (|max x - max y| <= max |x - y|)
    site_key [r]   in [0, n_keys) and  pm[r, site_key] >= site_peak[r] - b[r, site_key] - b[r, argmax_ref]:
                   the kernel maximises computed values g with |g - pm| <= b, so g[key] >= g[argmax_ref] gives exactly this; ties
                   and near-ties need no exclusion.  site_key names a STORED key, whose copy 0 sits at the column of that number.
"""
import torch

U_F, FLOOR = 2.0 ** -24, 2.0 ** -120


def profile_ref(pm, b):
    """(key_mass, its bound, site_peak, its bound, argmax) of an fp64 map pm (..., Lq, cols) with element bound b."""
    Lq = pm.shape[-2]
    km = pm.sum(-2) / Lq
    km_b = b.sum(-2) / Lq + (Lq + 8) * U_F * km + FLOOR
    peak, arg = pm.max(-1)
    return km, km_b, peak, b.amax(-1), arg


def site_key_slack(pm, b, site_key, n_keys):
    """Per row, pm[r, site_key] - (site_peak[r] - b[r, site_key] - b[r, argmax]) (>= 0 is what the kernel guarantees) and
    whether site_key is in [0, n_keys); n_keys broadcasts against site_key (..., Lq)."""
    peak, arg = pm.max(-1)
    in_range = (site_key >= 0) & (site_key < n_keys)
    k = site_key.long().clamp(0, pm.shape[-1] - 1).unsqueeze(-1)
    at = pm.gather(-1, k).squeeze(-1)
    slack = at - (peak - b.gather(-1, k).squeeze(-1) - b.gather(-1, arg.unsqueeze(-1)).squeeze(-1))
    return slack, in_range
