"""Entity codes of the screening path: what a DrugLAMP forward computes per protein and per drug, cached so that a
P x D screen pays it P + D times and only the pair stage P * D times.

In eval mode everything in front of the PGCA attention core is per entity (MolecularGCN, ProteinCNN, fill / site pooling,
the LLM adaptors; BatchNorm uses its running statistics), and the drug enters the pair stage only as key and value of the
two PGCA blocks (reference model/DrugLAMP.py:55-71).  PGCA's in-projection of the query depends on the protein alone, that
of key / value on the drug alone (guided_cross_attention_model.py:138-162), and the out-projection is linear behind the
softmax (:290-314):  softmax(Q K^T) V W_o^T = softmax(Q K^T) (V W_o^T).  So

  ProteinCode, per branch ('v'; 'x' where the model has an LLM branch):
      sites (P, n_site, 128)   the protein sites (`vpc` / `xpc` of the forward), compute dtype
      q     (P, n_site, 128)   their query in-projection
  DrugCode, per branch:
      kv    (D, Lk, 256)       [K | V'] — the key / value in-projection of the drug rows with V' = V W_o^T folded in
      bias  (128,) fp32        the out-projection bias (added by the kernel in fp32: folding it into V' would lean on
                               rounded probabilities summing to one)
      layout (Lk, key_tail_rows, key_tail_weight)
                               the encoders' compact forms hand over block + 8 distinct rows whose last 8 stand for
                               key_tail_weight identical padding rows each (MolecularGCN, the drug LLM adaptor under a
                               `drug_tokens` hint): the code is built from those rows and the multiplicity becomes the key
                               tail of the attention; otherwise all 512 rows, no tail.

model.score_codes (model/basic_model.py) runs the pair stage from these with one ops.pgca_pairs launch per branch.
Codes record the compute dtype and the parameter epoch (functional.bump_param_epoch) they were built at.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import functional as Fn
from . import ops


def param_epoch() -> int:
    """The optimiser epoch functional.bump_param_epoch advances (weight images and entity codes are valid for one)."""
    return Fn._param_epoch


def _in_proj(gca, cdt):
    E = gca.embed_dim
    if gca.num_heads != 1 or E != 128:
        raise NotImplementedError("screening: PGCA with one head of 128 only (got %d heads, embed_dim %d)" % (gca.num_heads, E))
    w = Fn.lowp((gca.in_proj_weight,), cdt)
    b = None if gca.in_proj_bias is None else gca.in_proj_bias.detach()
    return E, w, b


@torch.no_grad()
def protein_branch(gca, sites: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sites, q) of one PGCA block: sites (P, n_site, E) -> q = sites W_q^T + b_q, as GuidedCrossAttentionFn projects it."""
    cdt = gca.compute_dtype
    E, w, b = _in_proj(gca, cdt)
    sites = Fn.cast(sites, cdt).contiguous()
    P, L, _ = sites.shape
    q = ops.gemm(sites.view(P * L, E), w[:E], M=P * L, N=E, K=E, bias=None if b is None else b[:E])
    return sites, q.view(P, L, E)


class DrugBranch:
    __slots__ = ("kv", "bias", "layout")

    def __init__(self, kv: torch.Tensor, bias: Optional[torch.Tensor], layout: Tuple[int, int, int]):
        self.kv, self.bias, self.layout = kv, bias, (int(layout[0]), int(layout[1]), int(layout[2]))

    @property
    def key_tail(self):
        return (self.layout[1], float(self.layout[2])) if self.layout[1] else None

    def full(self) -> "DrugBranch":
        """The same code over the full key set: tail row j copied to rows lead + i * tail + j (i < weight) — ExpandTailFn's
        order.  K and V' are row-wise functions of the drug rows, so the gather is exact."""
        Lk, t, w = self.layout
        if not t:
            return self
        lead = Lk - t
        idx = torch.cat([torch.arange(lead), lead + torch.arange(t * w) % t]).to(self.kv.device)
        return DrugBranch(self.kv.index_select(1, idx), self.bias, (lead + t * w, 0, 1))


@torch.no_grad()
def drug_branch(gca, rows: torch.Tensor, tail: Optional[Tuple[int, int]] = None) -> DrugBranch:
    """[K | V'] of one PGCA block from the drug rows (D, Lk, E); tail = (rows, weight) of a compact form or None."""
    cdt = gca.compute_dtype
    E, w, b = _in_proj(gca, cdt)
    rows = Fn.cast(rows, cdt).contiguous()
    D, Lk, _ = rows.shape
    M = D * Lk
    kv = ops.gemm(rows.view(M, E), w[E:], M=M, N=2 * E, K=E, bias=None if b is None else b[E:])      # `kv` of GuidedCrossAttentionFn
    code = torch.empty_like(kv)
    code[:, :E].copy_(kv[:, :E])
    ops.gemm(kv[:, E:], Fn.lowp((gca.out_proj.weight,), cdt), M=M, N=E, K=E, ldx=2 * E, out=code[:, E:])   # V' = V W_o^T
    ob = gca.out_proj.bias
    bias = None if ob is None else ob.detach().float().clone()
    t, wt = (int(tail[0]), int(tail[1])) if tail is not None else (0, 1)
    return DrugBranch(code.view(D, Lk, 2 * E), bias, (Lk, t, wt))


class _Code:
    def __init__(self, branches: Dict[str, object], dtype: torch.dtype, epoch: int):
        self.branches, self.dtype, self.epoch = dict(branches), dtype, int(epoch)

    @staticmethod
    def _same(codes: Sequence["_Code"], what: str):
        if not codes:
            raise ValueError("%s.cat: nothing to concatenate" % what)
        c0 = codes[0]
        for c in codes[1:]:
            if c.dtype != c0.dtype or c.epoch != c0.epoch or set(c.branches) != set(c0.branches):
                raise ValueError("%s.cat: codes of different compute dtypes, parameter epochs or branches" % what)
        return c0


class ProteinCode(_Code):
    """branches[name] = (sites, q), both (P, n_site, 128) in the compute dtype."""

    @property
    def n(self) -> int:
        return int(next(iter(self.branches.values()))[0].shape[0])

    @classmethod
    def cat(cls, codes: List["ProteinCode"]) -> "ProteinCode":
        c0 = cls._same(codes, "ProteinCode")
        if len(codes) == 1:
            return c0
        return cls({k: tuple(torch.cat([c.branches[k][i] for c in codes]) for i in range(2)) for k in c0.branches}, c0.dtype, c0.epoch)


class DrugCode(_Code):
    """branches[name] = DrugBranch(kv (D, Lk, 256), bias fp32 (128,), layout (Lk, key_tail_rows, key_tail_weight))."""

    @property
    def n(self) -> int:
        return int(next(iter(self.branches.values())).kv.shape[0])

    def layout(self, branch: str = "v") -> Tuple[int, int, int]:
        return self.branches[branch].layout

    @classmethod
    def cat(cls, codes: List["DrugCode"]) -> "DrugCode":
        """Codes of one key layout are concatenated as they are; mixed layouts are first brought to the full key set."""
        c0 = cls._same(codes, "DrugCode")
        if len(codes) == 1:
            return c0
        out = {}
        for k in c0.branches:
            bs = [c.branches[k] for c in codes]
            if len({b.layout for b in bs}) > 1:
                bs = [b.full() for b in bs]
                if len({b.layout for b in bs}) > 1:
                    raise ValueError("DrugCode.cat: branch %s has %s keys in full form" % (k, sorted({b.layout[0] for b in bs})))
            out[k] = DrugBranch(torch.cat([b.kv for b in bs]), bs[0].bias, bs[0].layout)
        return cls(out, c0.dtype, c0.epoch)
