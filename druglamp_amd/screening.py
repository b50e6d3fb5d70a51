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

  DrugLibrary, per branch: the resident form of many DrugCodes of ANY layouts — one packed row store with a per-drug table
      rows (R, 256)  row0 (D,) int64  n_keys (D,) int32  tail_weight (D,) fp32  bias (128,) fp32
                               drug d owns rows row0[d] .. row0[d] + n_keys[d] - 1; each of its last 8 rows stands for
                               tail_weight[d] identical keys.  A drug is trimmed to its own rows: roundup8(rows in front
                               of its trailing run of padding rows) + 8 keys instead of the batch's block + 8 or 512.
model.score_library runs the pair stage from it with one ops.pgca_pairs_ragged launch per branch.

Attention maps of pairs come from the same codes: the PGCA weights softmax(scale q K_d^T + log w) need only a ProteinCode's q and
the first 128 columns of a drug's rows, so model.cross_attn_prob_codes / cross_attn_prob_library (one ops.pgca_pairs_probs /
pgca_pairs_ragged_probs launch) give what get_cross_attn_prob gives after an eval forward on those pairs, without one.
"""
from __future__ import annotations

import hashlib
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from . import functional as Fn
from . import ops


LIB_TAIL_ROWS = 8                  # key_tail_rows of every library launch; the tail rows of every compact form


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


def token_mean(rows: torch.Tensor, tail=None) -> torch.Tensor:
    """The fp32 mean over an entity's full row set, (n, C).  rows (n, L, C); tail = (distinct rows (n, block + 8, C), w) of an
    encoder's compact form (`_dl_tail`): each of its last 8 rows stands for w identical rows, so the mean over the
    block + 8 w rows is (sum(lead rows) + w sum(tail rows)) / (block + 8 w) — nothing is expanded."""
    if tail is None:
        return rows.float().mean(dim=1)
    y, w = tail
    lead, w = y.shape[1] - LIB_TAIL_ROWS, int(w)
    y = y.float()
    return (y[:, :lead].sum(dim=1) + w * y[:, lead:].sum(dim=1)) / float(lead + LIB_TAIL_ROWS * w)


def _cat_latents(codes, what: str):
    have = [c.latent is not None for c in codes]
    if not any(have):
        return None
    if not all(have):
        raise ValueError("%s: codes with and without latents" % what)
    return torch.cat([c.latent for c in codes])


class _Code:
    """latent: (n, 256) fp32 l2-normalised cross-modality latents of the entities (two_c2p models with an LLM branch), or None."""

    def __init__(self, branches: Dict[str, object], dtype: torch.dtype, epoch: int, *, latent: Optional[torch.Tensor] = None):
        self.branches, self.dtype, self.epoch, self.latent = dict(branches), dtype, int(epoch), latent

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
        return cls({k: tuple(torch.cat([c.branches[k][i] for c in codes]) for i in range(2)) for k in c0.branches}, c0.dtype, c0.epoch,
                   latent=_cat_latents(codes, "ProteinCode.cat"))


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
        return cls(out, c0.dtype, c0.epoch, latent=_cat_latents(codes, "DrugCode.cat"))




def fingerprint(model: torch.nn.Module, dtype: torch.dtype) -> str:
    """sha1 over the model's state_dict (names and tensor bytes in key order, computed on the CPU) and the compute dtype: what
    a saved library is valid for (the parameter epoch is a per-process counter and means nothing in a file)."""
    h = hashlib.sha1()
    for k, v in model.state_dict().items():
        t = v.detach().cpu().contiguous().reshape(-1)
        h.update(k.encode() + b"\0" + str(t.dtype).encode() + b"\0")
        h.update(t.view(torch.uint8).numpy().tobytes())
    h.update(str(dtype).encode())
    return h.hexdigest()


class LibraryBranch:
    __slots__ = ("rows", "row0", "n_keys", "tail_weight", "bias")

    def __init__(self, rows, row0, n_keys, tail_weight, bias):
        self.rows, self.row0, self.n_keys, self.tail_weight, self.bias = rows, row0, n_keys, tail_weight, bias


def _trim_branch(b: DrugBranch):
    """(rows (R, 256), n_keys (D,) int64, tail_weight (D,) fp32) of one code's branch, every drug trimmed to its own rows.

    Drug d's last row x is its padding row; rows equal to x BY VALUE (torch.eq: -0.0 == +0.0 — the GCN's in-block virtual
    nodes pass through the aggregation product, which can turn one into the other; NaN != NaN, so such a drug is kept whole)
    at the end of the drug are the trailing run.  lead = the rows in front of it rounded up to a multiple of 8; the code stood
    for count = (Lk - t) + t * w keys (Lk without a tail); with count - lead a multiple of 8 and >= 16 the drug becomes
    kv[:lead] followed by 8 copies of x, weight (count - lead) / 8.  Otherwise (and where the code's t tail rows are not all
    equal to x) its rows are stored unchanged with the code's own weight.  Equal rows have equal scores and equal values, so
    the softmax over lead + 8 * weight = count keys is the one over the code's keys."""
    Lk, t, w = b.layout
    T = LIB_TAIL_ROWS
    if t not in (0, T):
        raise ValueError("DrugLibrary: a code with %d tail rows (the library's kernel launches take %d or none)" % (t, T))
    if Lk < T:
        raise ValueError("DrugLibrary: a code of %d keys (at least %d are needed)" % (Lk, T))
    kv = b.kv
    D = kv.shape[0]
    dev = kv.device
    count = (Lk - t) + t * w if t else Lk
    eq = (kv == kv[:, -1:, :]).all(dim=2)                                     # (D, Lk): row equals the drug's last row
    pos = torch.arange(1, Lk + 1, device=dev)
    front = (pos * (~eq)).amax(dim=1)                                         # rows in front of the trailing run of equal rows
    lead = (front + 7) // 8 * 8
    rest = count - lead
    trim = (rest >= 2 * T) & (rest % T == 0)
    if t:
        trim &= eq[:, Lk - t:].all(dim=1)
    n_keys = torch.where(trim, lead + T, torch.full_like(lead, Lk))
    weight = torch.where(trim, rest // T, torch.full_like(lead, w if t else 1)).to(torch.float32)
    start = torch.cumsum(n_keys, 0) - n_keys
    drug = torch.repeat_interleave(torch.arange(D, device=dev), n_keys)      # (a host sync for the row count: a one-time build step)
    r = torch.arange(drug.numel(), device=dev) - start[drug]
    src = torch.where(trim[drug] & (r >= lead[drug]), torch.full_like(r, Lk - 1), r)
    rows = kv.reshape(D * Lk, kv.shape[2]).index_select(0, drug * Lk + src)
    return rows, n_keys, weight


class DrugLibrary:
    """A resident drug library: per branch a LibraryBranch (see the module text), plus the compute dtype, the parameter epoch
    and — when built or loaded with the model — the parameter fingerprint that a saved file carries.  latent: the drugs'
    cross-modality latents (D, 256) in the compute dtype (bf16: rounded once, when the library is built), the resident side
    of ops.latent_topk / Trainer.shortlist; None where the codes carry none."""

    def __init__(self, branches: Dict[str, LibraryBranch], dtype: torch.dtype, epoch: int, fingerprint_: Optional[str] = None,
                 latent: Optional[torch.Tensor] = None):
        self.branches, self.dtype, self.epoch, self.fingerprint = dict(branches), dtype, int(epoch), fingerprint_
        self.latent = latent
        self._count_full_keys()

    def _count_full_keys(self) -> None:
        """Per branch the full key count of every drug, (D,) int64 on the host: taken once here (from_codes, load) and after
        append, so that a map launch sizes its columns without a device sync."""
        T = LIB_TAIL_ROWS
        self._full_keys = {k: (b.n_keys.to(torch.int64) - T + T * b.tail_weight.to(torch.int64)).cpu() for k, b in self.branches.items()}

    # ---- building -------------------------------------------------------------------------------------------------------
    @classmethod
    def from_codes(cls, codes: Iterable[DrugCode], model: Optional[torch.nn.Module] = None) -> "DrugLibrary":
        """The library of the drugs of `codes` (DrugCodes of any layouts, in order; an iterator is consumed code by code, so
        that only the trimmed rows of earlier codes stay alive).  No code is expanded to its full key set.  Plain torch ops:
        runs on CPU tensors too.  model: stamps the library with the fingerprint `save` needs."""
        c0, parts, lats = None, {}, []
        for c in codes:
            if c0 is None:
                c0 = c
            elif c.dtype != c0.dtype or c.epoch != c0.epoch or set(c.branches) != set(c0.branches) or (c.latent is None) != (c0.latent is None):
                raise ValueError("DrugLibrary: codes of different compute dtypes, parameter epochs or branches")
            if c.latent is not None:
                lats.append(c.latent.to(c.dtype))
            for k, b in c.branches.items():
                parts.setdefault(k, []).append(_trim_branch(b) + (b.bias,))
        if c0 is None:
            raise ValueError("DrugLibrary.from_codes: no codes")
        branches = {}
        for k, ps in parts.items():
            n_keys = torch.cat([p[1] for p in ps])
            branches[k] = LibraryBranch(torch.cat([p[0] for p in ps]), torch.cumsum(n_keys, 0) - n_keys, n_keys.to(torch.int32),
                                        torch.cat([p[2] for p in ps]), ps[0][3])
        return cls(branches, c0.dtype, c0.epoch, None if model is None else fingerprint(model, c0.dtype),
                   latent=torch.cat(lats).contiguous() if lats else None)

    def append(self, dcode: DrugCode) -> "DrugLibrary":
        """Adds the drugs of one more code behind the library's (in place; returns self).  Copies the row store once: build a
        large library with from_codes over all its codes."""
        if dcode.dtype != self.dtype or dcode.epoch != self.epoch or set(dcode.branches) != set(self.branches):
            raise ValueError("DrugLibrary.append: the code's compute dtype, parameter epoch or branches differ from the library's")
        if (dcode.latent is None) != (self.latent is None):
            raise ValueError("DrugLibrary.append: the code and the library do not both carry latents")
        if self.latent is not None:
            self.latent = torch.cat([self.latent, dcode.latent.to(self.dtype)]).contiguous()
        for k, b in dcode.branches.items():
            rows, n_keys, weight = _trim_branch(b)
            lb = self.branches[k]
            row0 = lb.rows.shape[0] + torch.cumsum(n_keys, 0) - n_keys
            self.branches[k] = LibraryBranch(torch.cat([lb.rows, rows]), torch.cat([lb.row0, row0]), torch.cat([lb.n_keys, n_keys.to(torch.int32)]),
                                             torch.cat([lb.tail_weight, weight]), lb.bias)
        self._count_full_keys()
        return self

    # ---- what it holds --------------------------------------------------------------------------------------------------
    @property
    def n(self) -> int:
        return int(next(iter(self.branches.values())).n_keys.numel())

    @property
    def nbytes(self) -> int:
        lat = 0 if self.latent is None else self.latent.numel() * self.latent.element_size()
        return lat + sum(t.numel() * t.element_size() for b in self.branches.values()
                         for t in (b.rows, b.row0, b.n_keys, b.tail_weight, b.bias) if t is not None)

    def keys(self, branch: str = "v") -> torch.Tensor:
        """The stored key count of every drug, (D,) int32."""
        return self.branches[branch].n_keys

    def full_keys(self, branch: str = "v") -> torch.Tensor:
        """The full key count n_keys - 8 + 8 * tail_weight of every drug, (D,) int64 on the host: the columns of its expanded
        attention map (512 on the model's path)."""
        return self._full_keys[branch]

    def expand(self, branch: str, i: int) -> torch.Tensor:
        """Drug i's code over its full key set (lead + 8 * weight rows, 512 on the model's path) in ExpandTailFn's order: tail row
        j at rows lead + m * 8 + j (m < weight).  For tests and debugging."""
        b = self.branches[branch]
        r0, n, w = int(b.row0[i]), int(b.n_keys[i]), int(b.tail_weight[i])
        T = LIB_TAIL_ROWS
        idx = torch.cat([torch.arange(n - T), n - T + torch.arange(T * w) % T]).to(b.rows.device)
        return b.rows[r0:r0 + n].index_select(0, idx)

    # ---- persistence ----------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """One torch.save of a dict of tensors and plain scalars (readable with weights_only=True)."""
        if self.fingerprint is None:
            raise RuntimeError("DrugLibrary.save: the library has no parameter fingerprint (build it with from_codes(codes, model) "
                               "or Trainer.build_library)")
        blob = {"format": 1, "dtype": str(self.dtype).split(".")[1], "fingerprint": self.fingerprint, "branches": sorted(self.branches)}
        for k, b in self.branches.items():
            for f in LibraryBranch.__slots__:
                t = getattr(b, f)
                if t is not None:
                    blob["%s.%s" % (k, f)] = t.detach().cpu()
        if self.latent is not None:          # (a library without latents writes exactly the keys above)
            blob["latent"] = self.latent.detach().cpu()
        torch.save(blob, path)

    @classmethod
    def load(cls, path, model: torch.nn.Module, device=None) -> "DrugLibrary":
        """Reads a saved library for `model`: the file's fingerprint must be that of the model's parameters now (RuntimeError
        otherwise); the library is stamped with the current parameter epoch."""
        blob = torch.load(path, map_location="cpu", weights_only=True)
        if blob.get("format") != 1 or blob.get("dtype") not in ("float32", "bfloat16"):
            raise RuntimeError("DrugLibrary.load: %s is not a saved drug library" % (path,))
        dtype = getattr(torch, blob["dtype"])
        now = fingerprint(model, dtype)
        if blob["fingerprint"] != now:
            raise RuntimeError("DrugLibrary.load: the library was built with other parameters or another compute dtype "
                               "(fingerprint %s, the model's is %s); build it again" % (blob["fingerprint"], now))
        branches = {}
        for k in blob["branches"]:
            ts = [blob.get("%s.%s" % (k, f)) for f in LibraryBranch.__slots__]
            branches[k] = LibraryBranch(*[t if t is None or device is None else t.to(device) for t in ts])
        lat = blob.get("latent")
        return cls(branches, dtype, param_epoch(), now, latent=lat if lat is None or device is None else lat.to(device))
