"""fp64 reference of dl_latent_topk (include/druglamp_hip.h): the similarities in float64 from the STORED operands (already
rounded to their dtype) and the top-M in the specified order — value descending, equal values by ascending index, a NaN above
every number (NaNs by ascending index).  No test functions here."""
import numpy as np
import torch


def sims64(q: torch.Tensor, lib: torch.Tensor) -> np.ndarray:
    """(P, D) float64 dot products of the rows of q (P, 256) and lib (D, 256) as stored."""
    return q.detach().cpu().double().numpy() @ lib.detach().cpu().double().numpy().T


def topm(s: np.ndarray, M: int):
    """(values (P, M) float64, indices (P, M) int64) of the score matrix s (P, D)."""
    P, D = s.shape
    assert 1 <= M <= D
    idx = np.arange(D)
    vals, inds = np.empty((P, M)), np.empty((P, M), dtype=np.int64)
    for p in range(P):
        nan = np.isnan(s[p])
        clean = np.where(nan, 0.0, s[p])
        order = np.lexsort((idx, -clean, ~nan))[:M]          # NaN first, then value descending, then index ascending
        vals[p], inds[p] = s[p][order], order
    return vals, inds


def unit_rows(n: int, seed: int, dtype: torch.dtype) -> torch.Tensor:
    """n unit-norm random rows of 256, rounded to dtype (the rounding comes last: these are the stored operands)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 256, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).to(dtype)


def int_rows(n: int, seed: int, dtype: torch.dtype, distinct: int = 0) -> torch.Tensor:
    """n rows of 256 small integers (-2 .. 2): every dot product (|s| <= 1024) is exact in fp32 whatever the order of the
    sum.  distinct > 0: only that many different rows, row i = base[i % distinct] — many exact ties."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(-2, 3, (distinct or n, 256), generator=g).to(dtype)
    return base[torch.arange(n) % (distinct or n)].contiguous()
