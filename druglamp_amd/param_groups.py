"""Parameter groups for the fused AdamW (Trainer(param_groups=...)): a learning-rate scale and a weight decay per group of
parameters, and freezing.

The optimiser keeps its one launch per contiguous run of parameters: the group of every 16-byte chunk of the flat arena is a
byte of a device table (`quad_group`), the groups' values are rows of a second one (`group_tab`), and dl_adamw_step_groups
(csrc/optim.hip) looks both up per chunk.  A host-side split of the runs at every group boundary would turn the one to
three launches of an optimiser into a couple of hundred: biases and norm weights interleave with matrices.

    groups = [ParamGroup("no_decay", max_ndim=1, weight_decay=0.0),
              ParamGroup("encoders", match=("drug_extractor.*", "protein_extractor.*"), lr_scale=0.1),
              ParamGroup("adaptor", match=("drug_llm_adaptor.*",), frozen=True)]
    trainer = Trainer(model, cfg, param_groups=groups)

Names are those of model.named_parameters() (deduplicated: the ProteinCNN the SSL head shares appears as
`protein_extractor.*` only).  The first matching group wins; what no group matches is group 0, "default".
"""
from __future__ import annotations

import dataclasses
import fnmatch
import math
from typing import List, Optional, Sequence, Tuple

import torch

MAX_GROUPS = 64          # rows of the device table (dl_adamw_step_groups: n_groups in [1, 64]); "default" is one of them


@dataclasses.dataclass(frozen=True)
class ParamGroup:
    """One group: the parameters whose name matches any fnmatch pattern of `match`, or whose ndim is <= `max_ndim`
    (max_ndim=1: biases and norm weights).  lr_scale multiplies every optimiser's scheduled learning rate (one fp32 multiply on
    the device); weight_decay=None means the optimiser's own value.  frozen=True: the trainer switches requires_grad off for
    the group's parameters before anything else is built (it cannot be changed afterwards)."""
    name: str
    match: Tuple[str, ...] = ()
    max_ndim: Optional[int] = None
    lr_scale: float = 1.0
    weight_decay: Optional[float] = None
    frozen: bool = False

    def selects(self, pname: str, p) -> bool:
        if self.max_ndim is not None and p.ndim <= self.max_ndim:
            return True
        return any(fnmatch.fnmatchcase(pname, pat) for pat in self.match)


def _value(what: str, v) -> float:
    ok = isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(float(v)) and float(v) >= 0.0
    if not ok:
        raise ValueError("%s = %r: must be a finite number >= 0" % (what, v))
    return float(v)


class ParamGroups:
    """The assignment of a model's parameters to groups (host, at construction), and after build(flat) the two device tables
    the optimiser kernel reads:
        quad_group  uint8, flat.numel / 4 entries: the group of every 16-byte chunk, a parameter's padding chunk included
        group_tab   fp32 (G, 2): {lr_scale, weight_decay} per group, row 0 = "default"
    Raises ValueError for an empty or duplicate group name or the name "default", a negative or non-finite lr_scale /
    weight_decay, more than 63 groups, a group with neither `match` nor `max_ndim`, and a group that ends up with no parameter
    (a typo in a pattern must not pass silently)."""

    def __init__(self, model: torch.nn.Module, groups: Sequence[ParamGroup], default_weight_decay: float):
        groups = list(groups)
        wd0 = _value("ParamGroups: default_weight_decay", default_weight_decay)
        if len(groups) > MAX_GROUPS - 1:
            raise ValueError("ParamGroups: %d groups; at most %d (and \"default\")" % (len(groups), MAX_GROUPS - 1))
        seen = {"default"}
        rows = [(1.0, wd0)]
        for g in groups:
            if not isinstance(g, ParamGroup):
                raise ValueError("ParamGroups: %r is not a ParamGroup" % (g,))
            if not isinstance(g.name, str) or not g.name:
                raise ValueError("ParamGroups: a group needs a non-empty name (got %r)" % (g.name,))
            if g.name in seen:
                raise ValueError("ParamGroups: the group name %r is %s" % (g.name, "reserved" if g.name == "default" else "used twice"))
            seen.add(g.name)
            if isinstance(g.match, str):
                raise ValueError("ParamGroups: group %r: match must be a sequence of patterns, not one string" % g.name)
            if not tuple(g.match) and g.max_ndim is None:
                raise ValueError("ParamGroups: group %r selects nothing: it has neither match patterns nor max_ndim" % g.name)
            rows.append((_value("ParamGroups: group %r: lr_scale" % g.name, g.lr_scale),
                         wd0 if g.weight_decay is None else _value("ParamGroups: group %r: weight_decay" % g.name, g.weight_decay)))
        self.names: List[str] = ["default"] + [g.name for g in groups]
        self.frozen: List[bool] = [False] + [bool(g.frozen) for g in groups]
        self.rows: List[Tuple[float, float]] = rows
        self._params = []                        # (parameter name, parameter, group index), in model.named_parameters() order
        count = [0] * len(self.names)
        for pname, p in model.named_parameters():
            k = next((j + 1 for j, g in enumerate(groups) if g.selects(pname, p)), 0)
            self._params.append((pname, p, k))
            count[k] += 1
        empty = [self.names[k] for k in range(1, len(self.names)) if count[k] == 0]
        if empty:
            raise ValueError("ParamGroups: no parameter ends up in group(s) %s (a pattern that matches nothing, or earlier groups "
                             "took every match: the first matching group wins)" % ", ".join(repr(n) for n in empty))
        self.quad_group: Optional[torch.Tensor] = None
        self.group_tab: Optional[torch.Tensor] = None

    def freeze(self):
        """requires_grad_(False) on every parameter of a frozen group."""
        for _, p, k in self._params:
            if self.frozen[k]:
                p.requires_grad_(False)

    def group_of(self, pname: str) -> str:
        for n, _, k in self._params:
            if n == pname:
                return self.names[k]
        raise KeyError(pname)

    def build(self, flat) -> "ParamGroups":
        """The device tables for `flat` (a trainer.FlatParams over this model's parameters), on the arena's device."""
        by_id = {id(p): k for _, p, k in self._params}
        if len(flat.params) != len(self._params) or any(id(p) not in by_id for p in flat.params):
            raise ValueError("ParamGroups.build: the FlatParams does not hold this model's parameters")
        quads = torch.empty(flat.numel // 4, dtype=torch.uint8)
        for p, off in zip(flat.params, flat.offsets):
            quads[off // 4:off // 4 + (p.numel() + 3) // 4] = by_id[id(p)]
        self.quad_group = quads.to(flat.arena.device)
        self.group_tab = torch.tensor(self.rows, dtype=torch.float32).reshape(len(self.rows), 2).to(flat.arena.device)
        return self

    def table(self) -> List[Tuple[str, str, int]]:
        """[(group name, parameter name, numel)] in parameter order, for logging."""
        return [(self.names[k], n, p.numel()) for n, p, k in self._params]

    def assignment(self) -> List[list]:
        """[[parameter name, group name, frozen]] in parameter order: what a checkpoint's signature records."""
        return [[n, self.names[k], bool(self.frozen[k])] for n, _, k in self._params]

    def state(self) -> dict:
        """The groups' current values, set_param_group's changes included: {"names": [...], "rows": [[lr_scale, weight_decay]]}."""
        return {"names": list(self.names), "rows": [[float(s), float(w)] for s, w in self.rows]}

    def check_state(self, state: dict) -> None:
        """ValueError unless `state` is a state() of these groups with valid values (nothing is written)."""
        if list(state.get("names", ())) != self.names or len(state.get("rows", ())) != len(self.names):
            raise ValueError("ParamGroups: the saved groups %s are not this trainer's %s" % (list(state.get("names", ())), self.names))
        for n, row in zip(self.names, state["rows"]):
            _value("ParamGroups: saved group %r: lr_scale" % n, row[0])
            _value("ParamGroups: saved group %r: weight_decay" % n, row[1])

    def load_state(self, state: dict) -> None:
        """Take every group's values from a state() and rewrite the device table (one small copy, between steps)."""
        self.check_state(state)
        self.rows = [(float(s), float(w)) for s, w in state["rows"]]
        if self.group_tab is not None:
            self.group_tab.copy_(torch.tensor(self.rows, dtype=torch.float32).reshape(len(self.rows), 2))

    def values(self, name: str) -> Tuple[float, float]:
        """(lr_scale, weight_decay) of a group as the host knows them."""
        if name not in self.names:
            raise ValueError("ParamGroups: no group named %r (groups: %s)" % (name, ", ".join(self.names)))
        return self.rows[self.names.index(name)]

    def set(self, name: str, lr_scale: Optional[float] = None, weight_decay: Optional[float] = None):
        """Rewrite one group's row (a small host-to-device copy between steps; never during a capture — the optimisers run
        outside the captured graph).  Takes effect with the next optimiser launch.  Whether a group is frozen cannot change."""
        if name not in self.names:
            raise ValueError("ParamGroups.set: no group named %r (groups: %s)" % (name, ", ".join(self.names)))
        k = self.names.index(name)
        s, w = self.rows[k]
        if lr_scale is not None:
            s = _value("ParamGroups.set: group %r: lr_scale" % name, lr_scale)
        if weight_decay is not None:
            w = _value("ParamGroups.set: group %r: weight_decay" % name, weight_decay)
        self.rows[k] = (s, w)
        if self.group_tab is not None:
            self.group_tab[k].copy_(torch.tensor([s, w], dtype=torch.float32))
