"""Data-parallel training loop (reference: trainer.py:39-292 + main.py:155-168), one process per GPU.

What is restated from the reference, in its order (trainer.py:179-231):
    forward -> opt.zero_grad -> cls backward -> [opt_ssl.zero_grad -> ssl forward/backward]
            -> [opt_cm.zero_grad -> cm forward (+ one-time weight auto-scale) -> backward]
            -> opt.step -> [opt_ssl.step] -> [opt_cm.step]
All three AdamW instances own the SAME parameter list (main.py:158-160), so every zero_grad wipes the
previous loss's gradients and each optimiser steps on whatever gradient is present last — kept as is.
Parameters whose gradient is None are skipped by torch.optim.AdamW; here too (per-parameter step
counts, contiguous "runs" of parameters with gradients).

What is new (MI355X-native):
  * parameters live in ONE flat fp32 arena; gradients are packed into a flat buffer by a single
    multi-tensor copy; each optimiser step is a handful of fused dl_adamw_step launches over
    contiguous runs instead of ~250 per-tensor updates;
  * gradient all-reduce = RCCL all-reduce (sum; the 1/world factor is folded into the AdamW kernel's
    grad_scale) on the flat buffer after backward, or (DL_GRAD_OVERLAP=1) on 8 MB buckets started from
    inside backward as soon as a bucket's gradients exist (GradOverlap), instead of Lightning's DDP wrapper.  Unlike the reference's DDP
    (which only reduces the cls backward that ran under the wrapper), the gradients the optimisers
    consume are reduced whichever loss produced them, so replicas never drift;
  * a backward pass whose gradients the next zero_grad wipes before any optimiser steps (cls on SSL / CM
    steps, ssl on CM steps) is not run: the parameters after the step are the same, the step is shorter;
  * optional gradient guard (Trainer(max_grad_norm=..., skip_nonfinite=...)): global-norm clipping and the skip of a step with
    a non-finite gradient, decided on the device from one fp64 pass over the flat gradient — no host round trip;
  * optional weight EMA (Trainer(ema_decay=...), WeightEMA): an averaged copy of the arena, one dl_ema_update pass per step behind
    the last optimiser, swapped in for evaluation and screening (Trainer.ema_weights) or for good (Trainer.adopt_ema);
  * optional imbalance-aware classification loss (Trainer(cls_loss=ClsLoss(...)), cls_loss.py): pos_weight, per-sample weights
    (meta "Weight") and the focal term as one dl_cls_loss_fwd / dl_cls_loss_bwd launch pair in place of the torch loss tail;
  * optional parameter groups (Trainer(param_groups=[ParamGroup(...)]), param_groups.py): a learning-rate scale and a weight decay
    per group and frozen parts, with the group looked up per 16-byte chunk inside the optimiser kernel (dl_adamw_step_groups) —
    the launches per optimiser stay the one to three of its runs;
  * checkpoints (Trainer.save_checkpoint / load_checkpoint, fit(checkpoint_dir=..., resume=True); the file: checkpoint.py):
    everything a step reads or writes outside the model — moments, step counts, schedules, EMA, guard counters, group values,
    the random generators of every rank — in one file beside the state_dict, so that a run resumes bit for bit; no kernel,
    and nothing changes for a trainer that never saves or loads.
"""
from __future__ import annotations

import collections
import contextlib
import dataclasses
import math
import os
import warnings
from typing import Dict, List, Optional, Sequence

import torch
import torch.distributed as dist

from . import checkpoint as ckpt
from . import functional as Fn
from . import ops
from .checkpoint import check_tensor
from .cls_loss import ClsLoss, classification_loss, meta_weights
from .param_groups import ParamGroup, ParamGroups
from .model.basic_model import binary_cross_entropy, cross_entropy_logits

# Trainer.hit_profiles: key_mass (P, k, cols) fp32, site_peak (P, k, n_site) fp32, site_key (P, k, n_site) int32, on the CPU
HitProfiles = collections.namedtuple("HitProfiles", "key_mass site_peak site_key")
# Trainer.hit_attributions: logit (P, k) fp32, key_attr {branch: (P, k, cols_b)} fp32, site_attr {branch: (P, k, n_site)} fp32, on the CPU
HitAttributions = collections.namedtuple("HitAttributions", "logit key_attr site_attr")


class CosineAnnealingWarmupRestarts:
    """scheduler/cosine_annealing_warmup.py:5-88 as plain arithmetic (cycle_mult = 1, gamma = 1): lr starts
    at min_lr; the k-th step() gives linear warm-up for k < warmup_steps, then half-cosine to min_lr."""

    def __init__(self, first_cycle_steps: int, max_lr: float, min_lr: float = 1e-8, warmup_steps: int = 0):
        assert warmup_steps < first_cycle_steps
        self.first_cycle_steps, self.max_lr, self.min_lr, self.warmup_steps = first_cycle_steps, max_lr, min_lr, warmup_steps
        self.step_in_cycle = 0
        self.cycle = 0
        self.lr = min_lr

    def step(self) -> float:
        self.step_in_cycle += 1
        if self.step_in_cycle >= self.first_cycle_steps:
            self.cycle += 1
            self.step_in_cycle -= self.first_cycle_steps
        s = self.step_in_cycle
        if s < self.warmup_steps:
            self.lr = (self.max_lr - self.min_lr) * s / self.warmup_steps + self.min_lr
        else:
            self.lr = self.min_lr + (self.max_lr - self.min_lr) * (
                1 + math.cos(math.pi * (s - self.warmup_steps) / (self.first_cycle_steps - self.warmup_steps))) / 2
        return self.lr

    def state(self) -> dict:
        """Where the schedule stands, for a checkpoint."""
        return {"step_in_cycle": int(self.step_in_cycle), "cycle": int(self.cycle), "lr": float(self.lr)}

    def load_state(self, state: dict) -> None:
        self.step_in_cycle, self.cycle, self.lr = int(state["step_in_cycle"]), int(state["cycle"]), float(state["lr"])


class FlatParams:
    """All optimised parameters as views into one fp32 arena (+ a same-layout gradient buffer)."""

    def __init__(self, params: Sequence[torch.nn.Parameter]):
        self.params = list(params)
        dev = self.params[0].device
        self.offsets, n = [], 0
        for p in self.params:
            self.offsets.append(n)
            n += (p.numel() + 3) // 4 * 4          # keep every tensor 16-byte aligned
        self.numel = n
        self.arena = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(n, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, off in zip(self.params, self.offsets):
                view = self.arena[off:off + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
        self.grad_views = [self.grads[off:off + p.numel()].view(p.shape) for p, off in zip(self.params, self.offsets)]

    def pack_grads(self) -> List[int]:
        """Copy the present .grad tensors into the flat buffer; returns the indices that had one."""
        idx = [i for i, p in enumerate(self.params) if p.grad is not None]
        if idx:
            torch._foreach_copy_([self.grad_views[i] for i in idx], [self.params[i].grad for i in idx])
        return idx

    def runs(self, idx: List[int], key) -> List[tuple]:
        """Merge adjacent parameter indices with equal key(i) into (start_elem, end_elem, first_index)."""
        out = []
        for i in idx:
            s, e = self.offsets[i], self.offsets[i] + (self.params[i].numel() + 3) // 4 * 4
            if out and out[-1][1] == s and key(out[-1][2]) == key(i) and out[-1][3] + 1 == i:
                out[-1] = (out[-1][0], e, out[-1][2], i)
            else:
                out.append((s, e, i, i))
        return [(s, e, first) for s, e, first, _ in out]


class GradOverlap:
    """Gradient all-reduce overlapped with the backward pass that produces the gradients (world > 1).

    The flat gradient buffer is cut into buckets of consecutive parameters, last parameter first (the
    order backward roughly finishes them in).  A post-accumulate hook on every parameter counts its
    bucket down; a complete bucket is packed into the flat buffer (one multi-tensor copy) and an
    asynchronous all-reduce (sum) is started on each of its contiguous runs.  Buckets go out in strict
    index order (a complete bucket waits for its predecessors), and `finish()` sends the rest after
    backward, so every rank issues the same collectives in the same order whatever the timing.

    Which parameters a backward pass of a `kind` ("cls" / "ssl" / "cm") reaches is agreed on by all
    ranks during the first pass of that kind (one small all-reduce of a presence mask, the only host
    sync; that pass reduces after backward).  Later passes reduce exactly the agreed set: a parameter
    of the set without a local gradient contributes zeros, a gradient outside the set is an error."""

    def __init__(self, flat: FlatParams, bucket_bytes: int = 8 << 20):
        self.flat = flat
        self.bucket_elems = max(bucket_bytes // 4, 1)
        self.expected: Dict[str, frozenset] = {}
        self.armed: Optional[str] = None
        self.bucket_of: Dict[int, int] = {}
        self.buckets: List[List[int]] = []
        self.pending: List[int] = []
        self.ready: set = set()
        self.next_bucket = 0
        self.works: list = []
        self.reduced: set = set()          # parameter indices whose all-reduce has been started
        self.index = {id(p): i for i, p in enumerate(flat.params)}
        self.handles = [p.register_post_accumulate_grad_hook(self._hook) for p in flat.params if p.requires_grad]

    def _plan(self, kind: str):
        exp = sorted(self.expected[kind], reverse=True)
        self.buckets, self.bucket_of, cur, n = [], {}, [], 0
        for i in exp:
            cur.append(i)
            n += self.flat.params[i].numel()
            if n >= self.bucket_elems:
                self.buckets.append(sorted(cur))
                cur, n = [], 0
        if cur:
            self.buckets.append(sorted(cur))
        for b, idx in enumerate(self.buckets):
            for i in idx:
                self.bucket_of[i] = b
        self.pending = [len(b) for b in self.buckets]

    def arm(self, kind: str):
        """Call right before the backward pass whose gradients the optimisers will consume."""
        self.works, self.reduced, self.ready, self.next_bucket, self.armed = [], set(), set(), 0, kind
        if kind in self.expected:
            self._plan(kind)
        else:
            self.buckets, self.bucket_of, self.pending = [], {}, []

    def _hook(self, p):
        if self.armed is None:
            return
        b = self.bucket_of.get(self.index[id(p)])
        if b is None:
            return
        self.pending[b] -= 1
        if self.pending[b] == 0:
            self.ready.add(b)
            while self.next_bucket in self.ready:
                self._launch(self.buckets[self.next_bucket])
                self.next_bucket += 1

    def _launch(self, idx: List[int]):
        fl = self.flat
        local = [i for i in idx if fl.params[i].grad is not None]
        absent = [i for i in idx if fl.params[i].grad is None]
        if local:
            torch._foreach_copy_([fl.grad_views[i] for i in local], [fl.params[i].grad for i in local])
        if absent:
            torch._foreach_zero_([fl.grad_views[i] for i in absent])
        for s, e, _ in fl.runs(idx, lambda i: 0):
            self.works.append(dist.all_reduce(fl.grads[s:e], op=dist.ReduceOp.SUM, async_op=True))
        self.reduced.update(idx)

    def _agree(self, have: List[int]) -> frozenset:
        """Union over ranks of the parameters that received a gradient."""
        mask = torch.zeros(len(self.flat.params), dtype=torch.int32)
        mask[have] = 1
        mask = mask.to(self.flat.grads.device)
        dist.all_reduce(mask, op=dist.ReduceOp.MAX)
        return frozenset(mask.cpu().nonzero().flatten().tolist())

    def finish(self) -> List[int]:
        """After backward: send the buckets the hooks did not, wait for everything; returns the indices the
        optimisers step (the agreed set)."""
        kind, self.armed = self.armed, None
        have = [i for i, p in enumerate(self.flat.params) if p.grad is not None]
        if kind not in self.expected:
            self.expected[kind] = self._agree(have)
            self._plan(kind)
            self.next_bucket = 0
        else:
            extra = set(have) - self.expected[kind]
            if extra:
                raise RuntimeError("GradOverlap: %d parameters outside the set agreed for '%s' backward passes received a "
                                   "gradient (first: index %d); the graph changed between steps" % (len(extra), kind, min(extra)))
        for b in range(self.next_bucket, len(self.buckets)):
            self._launch(self.buckets[b])
        self.next_bucket = len(self.buckets)
        for w in self.works:
            w.wait()
        self.works = []
        return sorted(self.expected[kind])


class FusedAdamW:
    """torch.optim.AdamW semantics (lr, betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2) on a FlatParams.
    groups (a built param_groups.ParamGroups, or None): every run is ONE dl_adamw_step_groups launch in place of the
    dl_adamw_step / dl_adamw_step_guarded one — the runs are still formed by step counts alone; the kernel resolves the group
    of each 16-byte chunk from groups.quad_group[s / 4 : e / 4] and multiplies this optimiser's lr by the group's scale."""
    WEIGHT_DECAY = 1e-2

    def __init__(self, flat: FlatParams, lr: float, betas=(0.9, 0.999), eps=1e-8, weight_decay=WEIGHT_DECAY, groups=None):
        self.flat, self.lr, self.betas, self.eps, self.wd = flat, lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros_like(flat.arena)
        self.exp_avg_sq = torch.zeros_like(flat.arena)
        self.steps = [0] * len(flat.params)
        self.groups = groups

    def step(self, idx: List[int], grad_scale: float = 1.0, guard: Optional[torch.Tensor] = None):
        """guard (ops.GradGuard.guard, a device tensor): the guarded kernel scales the gradient by grad_scale * guard[0] and
        writes nothing when guard[2] != 0.  The per-parameter step counts advance either way: the host does not know the
        device's decision."""
        gr = self.groups
        for s, e, first in self.flat.runs(idx, lambda i: self.steps[i]):
            run = (self.flat.arena[s:e], self.flat.grads[s:e], self.exp_avg[s:e], self.exp_avg_sq[s:e])
            kw = dict(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, step=self.steps[first] + 1,
                      grad_scale=grad_scale)
            # one launch per run, through the public name of its form (the three differ in their signatures alone)
            if gr is not None:
                ops.adamw_step_groups(*run, gr.quad_group[s // 4:e // 4], gr.group_tab, guard=guard, **kw)
            elif guard is not None:
                ops.adamw_step_guarded(*run, guard, weight_decay=self.wd, **kw)
            else:
                ops.adamw_step(*run, weight_decay=self.wd, **kw)
        for i in idx:
            self.steps[i] += 1

    def state(self) -> dict:
        """Both moments (copied to the CPU), the per-parameter step counts and the learning rate, for a checkpoint."""
        return {"exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu(), "steps": list(self.steps),
                "lr": float(self.lr)}

    def check_state(self, state: dict, what: str = "optimiser") -> None:
        """RuntimeError unless `state` is a state() of an optimiser over this arena (nothing is written)."""
        for k in ("exp_avg", "exp_avg_sq"):
            check_tensor("%s.%s" % (what, k), state.get(k), self.exp_avg.shape, torch.float32)
        steps = state.get("steps")
        if not isinstance(steps, list) or len(steps) != len(self.steps) or any(not isinstance(s, int) or s < 0 for s in steps):
            raise RuntimeError("checkpoint: %s.steps must be %d step counts" % (what, len(self.steps)))
        float(state["lr"])

    def load_state(self, state: dict) -> None:
        self.exp_avg.copy_(state["exp_avg"])
        self.exp_avg_sq.copy_(state["exp_avg_sq"])
        self.steps = [int(s) for s in state["steps"]]
        self.lr = float(state["lr"])


class WeightEMA:
    """An exponential moving average of the parameters on a FlatParams: `shadow`, an fp32 clone of the arena taken at
    construction (timm's ModelEmaV2; torch's AveragedModel after its first update_parameters), moved towards the arena by ONE
    dl_ema_update launch over the WHOLE arena per training step — parameters that received no gradient this step are averaged
    too (towards their unchanged value), as standard EMA does, and equal values (those, and the arena's padding) keep their bits.
    Weight of the update after t earlier ones: 1 - decay, or with warmup 1 - min(decay, (1 + t) / (10 + t)) — without it a
    short fine-tune never leaves its initial weights; the kernel receives the weight rounded to fp32.
    `updates` is a host count.  Like FusedAdamW's step counts it advances on a step the gradient guard skipped (the kernel
    writes nothing then, but the host does not know the device's decision), so the warmup schedule counts skipped steps."""

    def __init__(self, flat: FlatParams, decay: float, warmup: bool = False):
        self.flat, self.decay, self.warmup = flat, float(decay), bool(warmup)
        self.shadow = flat.arena.clone()
        self.updates = 0

    def weight(self, t: Optional[int] = None) -> float:
        """The weight of the update that follows t earlier ones (default: the next one), before its rounding to fp32."""
        t = self.updates if t is None else t
        return 1.0 - (min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay)

    def update(self, guard: Optional[torch.Tensor] = None):
        """guard (ops.GradGuard.guard): nothing is written when guard[2] != 0; `updates` advances either way."""
        ops.ema_update(self.shadow, self.flat.arena, self.weight(), guard)
        self.updates += 1

    def state(self) -> dict:
        """The shadow (copied to the CPU) and the update count, for a checkpoint."""
        return {"shadow": self.shadow.detach().cpu(), "updates": int(self.updates)}

    def load_state(self, state: dict) -> None:
        self.shadow.copy_(state["shadow"])
        self.updates = int(state["updates"])


class GraphedStep:
    """The cls-only part of a training step — forward, BCE, backward, gradient packing — captured ONCE per batch shape
    into a hipGraph (torch.cuda.CUDAGraph drives hipStreamBeginCapture on a side stream; every libdruglamp_hip launch
    goes to torch's current stream, so the whole launch sequence — ~260 library launches + ~100 torch launches — lands
    in the graph) and replayed with one host call per step.  At 32-64 pairs per GPU the eager step is bound by the
    7-9 ms the host needs to enqueue it; the replay costs the host < 1 ms.

    What stays outside the graph, on purpose: the gradient all-reduce (RCCL), the fused AdamW launches (their step
    counts and learning rates are by-value arguments that change from step to step) and the weight-EMA pass behind them (its
    weight is one too).
    What makes a replay a NEW step although every launch argument is frozen:
      * inputs are copied into the graph's static input tensors (skipped when the caller hands over those very
        tensors, Trainer.static_batch — a loader can assemble the next batch in place);
      * dropout masks are keyed by (site seed + *device offset*): the first node of the graph bumps the offset
        (ops.seed_offset_tensor), forward and backward of one replay read the same value;
      * the weight images are refreshed from the fp32 masters by the dl_weight_prep launch at the head of the graph;
      * BatchNorm running statistics are updated by the in-graph dl_bn_finalize launches (none with frozen BatchNorm: the
        flag is part of the trainer's graph key)."""

    def __init__(self, trainer: "Trainer", batch, kind: str = "cls", meta=None, caps=None):
        """Capture only records (nothing executes): the caller has already run eager steps of this shape AND kind, so lazy
        allocations (the SimSiam projectors of the first SSL forward), weight-image tables and workspaces exist.
        kind "ssl" (round 3): a step of an SSL epoch without the CM head — forward, BCE (logged only: its backward is dead,
        the next zero_grad wipes it, trainer.py:196-212 of the reference), SSL heads, their backward, gradient packing.  The
        MLM mask draw (rand / topk / scatter on the device) is captured with the step: torch's device generator is
        graph-safe (its Philox offset is advanced per replay), so every replay draws fresh masks.
        kinds "cm" / "sslcm" (round 3): a step with the cross-modality head (and, on SSL epochs, the SSL forward whose loss
        is logged and whose backward is dead).  The head is shape-static (model/cross_modality.py: unique-row blocks padded
        to the batch, masked BatchNorm statistics, (B, B) label matrix with ignored padding); the batch's label matrix is
        built on the host and copied into this graph's CMLabels before every replay.  The margin of the triplet loss and
        Trainer.cm_weight are by-value arguments of the capture: the trainer keys its graphs by them."""
        self.kind = kind
        self.tr = trainer
        dev = trainer.device
        self.static = self._clone(batch)
        # this graph's own device tables (refilled per replay) at the CAPACITIES the capture is made for: caps = (drug-token
        # block, ProteinCNN table rows), by-value knowledge of the capture — any batch that needs at most that much replays it
        self.hints = trainer.hints_of(meta, batch, own_tables=True, kind=kind, caps=caps)
        self.block = self.hints.drug_tokens                    # 0 = every drug-token row computed (serves any batch)
        self.rows_cap = None if self.hints.protein_plan is None else self.hints.protein_plan.rows
        self.base = None                                        # (set by the trainer: kind + batch signature + by-value scalars)
        self.byval = ()
        self.labels = None
        # Trainer(cls_loss=...) with per-sample weights (meta "Weight"): this graph's static weight tensor, refilled in run()
        # beside the labels; whether there are weights is part of the trainer's graph key
        w = meta_weights(meta) if trainer.cls_loss is not None else None
        self.weights = None if w is None else w.to(dev)
        if "cm" in kind:
            from .model.cross_modality import CMCodes, CMLabels
            if trainer.model.cm_model.global_batch and trainer.world > 1:
                # global-batch form: the step gathers integer id codes and builds the label matrix on the device
                self.labels = CMCodes(int(batch[2].shape[0]), dev).fill(meta)
            else:
                self.labels = CMLabels(int(batch[2].shape[0]), dev).fill(meta, trainer.model.cm_model.use_cm)
        # The weight-image refresh (dl_weight_prep) must be a node of the graph whatever ran last: an eager forward with no
        # optimiser step behind it (evaluate() between the warm-up steps and this capture, a validate-every-N loop) leaves
        # the images current, lowp() would skip the refresh during capture, and every replay would then compute with the
        # images frozen at capture time while AdamW keeps moving the fp32 masters.  Making the epoch stale puts the
        # refresh (and the derived-layout rebuilds) at the head of the captured forward; counted below.
        # (the item tables of the refresh are rebuilt — a host-to-device copy, illegal during capture — whenever the set of
        #  live images changed, e.g. an earlier model's images were garbage-collected: do that eagerly first)
        Fn.bump_param_epoch()
        Fn.refresh_images()
        Fn.bump_param_epoch()
        before = ops.weight_prep_launches()
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        from . import _lib as _L
        if _L.AUDIT:
            _L.lib()
            _L.audit_begin()
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.out, self.idx = self._body()
        if _L.AUDIT:
            self.audit = self._audit_pointers(_L.audit_end())
        if ops.weight_prep_launches() == before and Fn.planned_image_count() > 0:
            raise RuntimeError("GraphedStep: no dl_weight_prep launch was captured; replays would use stale weight images")
        self.replays = 0

    def _pinned_ranges(self):
        """(address, bytes) of every buffer that lives as long as the trainer / process: what a captured launch may point at
        besides memory of the graph's own pool."""
        tr = self.tr
        ts = [tr.flat.arena, tr.flat.grads] + [t for o in (tr.opt, tr.opt_ssl, tr.opt_cm) if o is not None for t in (o.exp_avg, o.exp_avg_sq)]
        ts += [b for b in tr.model.buffers()] + [p_ for p_ in tr.model.parameters()]
        ts += [t for b in self.static for t in (b if isinstance(b, (tuple, list)) else (b,))]
        if self.labels is not None:
            ts += [self.labels.buf if hasattr(self.labels, "buf") else self.labels.dev]
        if self.hints.protein_plan is not None:
            ts += [self.hints.protein_plan.buf]
        if self.weights is not None:
            ts += [self.weights]
        ts += list(ops._guard_flags.values()) + list(ops._cls_flags.values())
        ts += list(ops._seed_offsets.values()) + list(ops._tickets.values())
        ts += [e.image for e in Fn._lowp_cache.values() if torch.is_tensor(e.image)]
        for tab in list(Fn._lowp_tables.values()) + [t for t in Fn._lowp_retired if isinstance(t, tuple) and len(t) == 4]:
            ts += [tab[1], tab[2]]
        out = []
        for t in ts:
            if torch.is_tensor(t) and t.is_cuda:
                st = t.untyped_storage()
                out.append((st.data_ptr(), st.nbytes()))
        return out

    def _audit_pointers(self, log):
        """DL_GRAPH_PTR_AUDIT=1: every device pointer a captured library launch received lies in the graph's private pool or
        in a pinned buffer; anything else could be freed and re-used under the graph (the two use-after-free classes of
        round 2 were exactly that).  Raises with the offending entry points; returns (pointers checked, in pool, pinned)."""
        segs = [(s["address"], s["address"] + s["total_size"], tuple(s.get("segment_pool_id", (0, 0)))) for s in torch.cuda.memory_snapshot()]
        pinned = self._pinned_ranges()
        n_pool = n_pin = 0
        bad = []
        for fn, what, ptr in log:
            seg = next((s for s in segs if s[0] <= ptr < s[1]), None)
            if seg is not None and seg[2] != (0, 0):
                n_pool += 1
            elif any(a <= ptr < a + n for a, n in pinned):
                n_pin += 1
            elif seg is None:
                pass        # not device memory of the caching allocator (e.g. a module-scope constant of the library)
            else:
                bad.append((fn, what, hex(ptr)))
        if bad:
            raise RuntimeError("GraphedStep: %d pointers of captured launches lie in neither the graph's pool nor a pinned buffer "
                               "(first: %s)" % (len(bad), bad[:6]))
        return len(log), n_pool, n_pin

    @staticmethod
    def _clone(batch):
        return tuple(tuple(t.clone() for t in b) if isinstance(b, (tuple, list)) else b.clone() for b in batch)

    def _is_static(self, batch) -> bool:
        flat = lambda bt: [t for b in bt for t in (b if isinstance(b, (tuple, list)) else (b,))]   # noqa: E731
        return all(a is b for a, b in zip(flat(batch), flat(self.static)))

    @staticmethod
    def signature(batch):
        return tuple(tuple((tuple(t.shape), t.dtype) for t in b) if isinstance(b, (tuple, list)) else (tuple(b.shape), b.dtype)
                     for b in batch)

    def _body(self):
        tr = self.tr
        ops.seed_offset_tensor(tr.device).add_(1)
        # (hints: by-value knowledge of the capture — the block sizes are part of the graph key, the table CONTENTS are refilled)
        out, _ = tr._forward_backward(self.static, "ssl" in self.kind, "cm" in self.kind, hints=self.hints, weights=self.weights,
                                      cm_labels={"labels": self.labels})
        idx = tr.flat.pack_grads()
        self.reduced = False
        if tr.graph_allreduce and (tr.world > 1 or tr.graph_allreduce == "force"):
            # the gradient all-reduce as nodes of the graph (RCCL collectives can be captured: tools/graph_allreduce_probe.py):
            # no host launch between backward and the collective.  The agreed parameter set must be cached already (the
            # eager warm-up steps of this shape did that): agreeing needs a host sync, which capture forbids.
            if tr.world > 1:
                if self.last not in (tr._agreed_sets or {}):
                    raise RuntimeError("GraphedStep: the agreed gradient set of %s steps must exist before capture" % self.last)
                idx = tr._agreed(self.last, idx)
            tr._all_reduce_runs(idx)
            self.reduced = True
        return out, idx

    @property
    def last(self) -> str:
        """The backward pass the optimisers consume (the key of the agreed gradient set)."""
        return "cm" if "cm" in self.kind else self.kind

    def run(self, batch, meta=None, weights=None):
        """weights: this step's meta_weights(meta), where the trainer has them already."""
        if self.hints.protein_plan is not None:    # this batch's residue counts -> the graph's static tables (built on the device)
            spec = self.tr.protein_plan_of(meta, batch, must_pay=False)
            if spec is None or spec.need > self.hints.protein_plan.rows:
                raise RuntimeError("GraphedStep: the batch's ProteinCNN row tables do not fit the captured capacity")
            self.hints.protein_plan.fill(spec)
        if self.labels is not None:                # host label matrix / id codes -> the graph's static tensors
            if hasattr(self.labels, "buf"):
                self.labels.fill(meta, self.tr.model.cm_model.use_cm)
            else:
                self.labels.fill(meta)
        if self.weights is not None:               # this step's sample weights -> the graph's static weight tensor
            w = weights if weights is not None else meta_weights(meta)
            if w is None or w.numel() != self.weights.numel():
                raise RuntimeError("GraphedStep: the graph was captured with per-sample weights; this step's meta has none for the batch")
            self.weights.copy_(w)
        if not self._is_static(batch):                  # copy into the static inputs (device-to-device)
            for dst, src in zip(self.static, batch):
                if isinstance(dst, tuple):
                    for d, s_ in zip(dst, src):
                        d.copy_(s_)
                else:
                    dst.copy_(src)
        self.graph.replay()
        self.replays += 1
        return self.out, self.idx


class Trainer:
    """ExpModule restated (trainer.py:39-292).  `cfg` is the merged config tree.
    graph_steps=True: cls, SSL-epoch and CM steps run as hipGraph replays (GraphedStep); the first steps of every new
    (batch shape, step kind), the epoch the CM head starts in and the global-batch CM form stay eager.
    graph_steps="auto" (round 5): a replay where it was measured to pay (`wants_graph`): every kind at per-GPU batches <= 128
    (the eager step is host-enqueue bound there) and, at any batch, the kinds with the cross-modality head (600+ launches per
    step, many of them 3 us: eager 9.2-10.4 / 12.5-14.8 ms against 8.76 / 11.5 ms replayed at batch 256, same box); the cls and
    SSL-epoch steps at batch 256 stay eager (12.4 / 10.6 ms against 12.6 / 11.0 replayed)."""
    overlap = None
    # (drug-token block, ProteinCNN table rows) used for EVERY step, eager or captured, instead of per-batch capacities.
    # Reductions over rows (BatchNorm statistics, split-K weight gradients) associate by the row count, so an eager trainer
    # matches a graph-replaying one BIT FOR BIT only at equal capacities: the graph-vs-eager tests pin this on both trainers
    # when their batches differ (`fixed_caps_for`).  Eager steps otherwise round the needed rows up to 2048, captures use the
    # geometric classes of protein_plan.row_class (identical up to 16 k rows).
    fixed_caps = None
    _agreed_sets = None
    grad_bf16 = False
    graph_allreduce = False
    ema = None
    cls_loss = None
    param_groups = None
    _ema_spare = None
    _ema_swapped = False

    def __init__(self, model, cfg, device=None, compute_dtype=torch.float32, graph_steps: bool = False, freeze_bn: bool = False,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, ema_decay: Optional[float] = None,
                 ema_warmup: bool = False, cls_loss: Optional[ClsLoss] = None, param_groups: Optional[Sequence[ParamGroup]] = None):
        """freeze_bn=True: fine-tuning with frozen BatchNorm (model.freeze_batchnorm()): every BatchNorm1d normalises with its
        running statistics, which the steps leave bitwise unchanged; its weight / bias train.  cls steps only (eager or
        replayed): with the SSL or the CM head switched on (RS.SSL / RS.CM) construction raises.

        param_groups: a sequence of param_groups.ParamGroup (None or empty: off — nothing is allocated and a step calls exactly
        what it calls without them).  On, every parameter belongs to the first group that selects it (fnmatch patterns over
        model.named_parameters() names, or max_ndim; the rest is group "default": scale 1, the optimiser's weight decay), and
        every optimiser launch of a step is a dl_adamw_step_groups launch over the same run, eager and replayed steps alike
        (the optimisers run outside the captured graph): the group of each 16-byte chunk is read on the device from ONE chunk
        table that opt, opt_ssl and opt_cm share, each multiplies its own scheduled lr by the group's lr_scale (one fp32
        multiply) and uses the group's weight_decay.  The launch count of a step does not change.  set_param_group rewrites a
        group's values between steps; param_group_table lists the assignment.
        A group with frozen=True: requires_grad is switched off for its parameters first thing here, before the arena, the
        overlap hooks and any capture exist.  The parameters stay in the arena (the EMA, checkpoints and sync_replicas see
        them) but never receive a gradient, so they are in no optimiser run, not in the gradient guard's norm and not in the
        all-reduce; their arena values, both moments and their EMA shadow keep their bits.
          * BatchNorm running statistics are buffers, not parameters: a frozen module's BatchNorm still updates them in
            training mode unless freeze_bn is on as well.
          * lr_scale=0 is NOT freezing: the moments still move, and a -0.0 parameter can become +0.0.

        max_grad_norm / skip_nonfinite: the gradient guard (off unless one of them is set; off = the launches of a step are
        exactly those without it and no state is allocated).  On, every step — eager or replayed — measures the global L2 norm
        of the AVERAGED gradient (the all-reduced flat buffer times 1 / world: the same bits on every rank, so replicas take
        the same decision without another collective) with one fp64 pass over the gradient runs, decides ONCE on the
        device, and all optimisers of the step (opt, opt_ssl, opt_cm read the same gradient) apply that decision:
          * max_grad_norm (positive, finite): the gradient is scaled by min(1, max_grad_norm / (norm + 1e-6)), the formula
            of torch.nn.utils.clip_grad_norm_;
          * skip_nonfinite=True: a step whose gradient holds a NaN or an infinity is skipped — parameters, exp_avg and
            exp_avg_sq keep their bits.  The host never learns of the skip (the step does not synchronise), so the
            per-parameter step counts advance all the same and the bias correction of later steps counts the skipped
            ones — unlike torch.cuda.amp.GradScaler, which does not count a skipped step; the price of a step that never
            waits for the device.  BatchNorm running statistics are updated by the forward pass and are outside the
            guard's reach: a forward that produced non-finite activations has already written them.
        The step's result gains "grad_norm" (a device scalar); grad_guard_stats() reads the counters.

        ema_decay / ema_warmup: the weight EMA (off unless ema_decay is set: `ema` is None, nothing is allocated and a step
        launches exactly what it launches without it).  ema_decay: a float in [0, 1).  On, `ema` is a WeightEMA whose shadow
        starts as a clone of the arena (after the replicas were synchronised) and every training step — eager or replayed —
        ends with one dl_ema_update over the whole arena behind its last optimiser, outside the captured graph, reading the
        step's guard when the gradient guard is on: a skipped step leaves the shadow's bits alone.  As with the
        per-parameter step counts above, `ema.updates` advances on a skipped step all the same, and with ema_warmup the
        weight schedule counts it.  The shadow is a function of bit-identical parameters and a bit-identical guard decision
        on every rank: replicas hold the same shadow without another collective.  ema_weights() / adopt_ema() put the
        average to use; fit() validates and selects on it.  Buffers (BatchNorm running statistics) are shared, not averaged.

        cls_loss: the imbalance-aware classification loss (cls_loss.ClsLoss: pos_weight / neg_weight / focal gamma; off unless
        given: a step then calls what it calls without it and nothing is allocated).  On, the eager step and the captured
        body take the step's classification loss from cls_loss.classification_loss (one dl_cls_loss_fwd and one
        dl_cls_loss_bwd launch at the step's batch sizes, for one- and two-output classifiers alike); everything behind the
        loss — gradient guard, optimisers, EMA, all-reduce — is untouched.  Per-sample weights arrive through meta: when
        every entry of a step's meta has a "Weight" key, the step weights its samples with them (a (B,) fp32 device tensor;
        a captured step refills its own static copy before every replay, and whether a step has weights is part of the graph
        key); weights on only some entries raise ValueError.  The weights are a Python list turned into B floats and copied
        from pageable host memory, so a step WITH weights waits for that small copy; a step without them never synchronises.
        A negative or non-finite weight, like a label outside [0, 1], makes the loss and that sample's gradient NaN and raises
        FLAG_CLS_LABEL in the loss's own device guard word, which the step's polling and check_device_flags report beside the
        padding guards (with skip_nonfinite such a step is skipped, not silent).  predict / evaluate keep reporting the
        unweighted loss, so validation losses stay comparable across settings; fit is unchanged.  At world > 1 the loss and
        its normaliser (the batch size, or the sum of the weights) are rank-local, like every other mean of the step: the
        all-reduce averages the ranks' gradients of their own normalised losses."""
        if cls_loss is not None and not isinstance(cls_loss, ClsLoss):
            raise ValueError("Trainer(cls_loss=%r): must be None or a ClsLoss" % (cls_loss,))
        if param_groups:         # (first thing: frozen parameters lose requires_grad before FlatParams, GradOverlap and any capture)
            self.param_groups = ParamGroups(model, param_groups, default_weight_decay=FusedAdamW.WEIGHT_DECAY)
            self.param_groups.freeze()
        self.cls_loss = cls_loss
        if ema_decay is not None:
            ok = isinstance(ema_decay, (int, float)) and not isinstance(ema_decay, bool) and 0.0 <= float(ema_decay) < 1.0
            if not ok:
                raise ValueError("Trainer(ema_decay=%r): must be None or a float in [0, 1)" % (ema_decay,))
        if max_grad_norm is not None:
            mg = float(max_grad_norm)
            if not (mg > 0.0 and math.isfinite(mg)):
                raise ValueError("Trainer(max_grad_norm=%r): must be None or a positive finite number" % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.model = model
        self.cfg = cfg
        self.compute_dtype, self.freeze_bn = compute_dtype, bool(freeze_bn)     # (recorded in a checkpoint's signature)
        if freeze_bn:
            if bool(cfg["RS"]["SSL"]) or bool(cfg["RS"]["CM"]):
                raise ValueError("Trainer(freeze_bn=True) runs cls steps only: the SSL and CM step kinds are not supported with "
                                 "frozen BatchNorm (set RS.SSL and RS.CM to False)")
            model.freeze_batchnorm()
        self.device = device or next(model.parameters()).device
        self.n_class = cfg["DECODER"]["BINARY"]
        self.epochs = cfg["SOLVER"]["MAX_EPOCH"]
        self.use_ssl = bool(cfg["RS"]["SSL"])
        self.use_cm = bool(cfg["RS"]["CM"])
        self.ssl_epoch_step = cfg["RS"]["EPOCH_STEP"]
        self.cm_init_epoch = cfg["RS"]["INIT_EPOCH"]
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        model.set_compute_dtype(compute_dtype)
        # main.py:158-160: three AdamW over model.parameters() built BEFORE any SSL forward (the lazily
        # created SimSiam projectors are therefore in none of them)
        self.flat = FlatParams([p for p in model.parameters()])
        if self.world > 1:
            # what the reference's DDP wrapper does at wrap time (trainer.py:143-148 -> torch DDP): every replica starts
            # from rank 0's parameters and buffers (BatchNorm running statistics, step counters), whatever each rank's
            # own initialisation drew.  Without it replicas that were seeded differently drift silently: the all-reduce
            # averages gradients, never weights.
            self.sync_replicas()
        Fn.bump_param_epoch()
        warm = int(self.epochs * 0.2)
        pg = self.param_groups.build(self.flat) if self.param_groups is not None else None   # one table for the three optimisers
        self.opt = FusedAdamW(self.flat, cfg["SOLVER"]["LR"], groups=pg)
        self.opt_ssl = FusedAdamW(self.flat, cfg["SOLVER"]["SSL_LR"], groups=pg) if self.use_ssl else None
        self.opt_cm = FusedAdamW(self.flat, cfg["SOLVER"]["CM_LR"], groups=pg) if self.use_cm else None
        self.grad_guard = None
        self._guard_runs = None
        if self.max_grad_norm is not None or self.skip_nonfinite:
            self.grad_guard = ops.GradGuard(self.flat.numel, self.flat.grads.device, max_norm=self.max_grad_norm or 0.0,
                                            skip_nonfinite=self.skip_nonfinite)
        if ema_decay is not None:
            self.ema = WeightEMA(self.flat, float(ema_decay), warmup=ema_warmup)
        self.schd =CosineAnnealingWarmupRestarts(self.epochs, cfg["SOLVER"]["LR"], 1e-8, warm)
        self.schd_ssl = CosineAnnealingWarmupRestarts(self.epochs, cfg["SOLVER"]["SSL_LR"], 1e-8, warm) if self.use_ssl else None
        self.schd_cm = CosineAnnealingWarmupRestarts(self.epochs, cfg["SOLVER"]["CM_LR"], 1e-8, warm) if self.use_cm else None
        self.opt.lr = self.schd.lr
        if self.opt_ssl:
            self.opt_ssl.lr = self.schd_ssl.lr
        if self.opt_cm:
            self.opt_cm.lr = self.schd_cm.lr
        self.cm_weight = 1.0
        # the reference wipes the cls (and ssl) gradients with the next zero_grad before any optimiser steps
        # (header); a backward pass whose gradients nobody consumes is skipped unless asked for
        self.run_dead_backward = os.environ.get("DL_DEAD_BACKWARD", "0") == "1"
        # Gradient all-reduce at world > 1.  "1": bucketed all-reduce from inside backward (GradOverlap) for
        # eagerly run steps; the persistent large-tile GEMMs then hand their tiles out dynamically (ops.dynamic_tiles):
        # a CU that an RCCL channel workgroup occupies for a while takes fewer tiles instead of forcing a second round —
        # the reason overlap was off by default in round 1.  "0" (DEFAULT until a multi-GPU RCCL run of the overlapped form
        # is on record under profiles/): one reduction after backward.  "force": overlap also at
        # world size 1 (RCCL sanity runs).  hipGraph-replayed steps (graph_steps) always reduce after the replay: hooks
        # cannot launch collectives from inside a replay, and at the small per-GPU batches where graphs are used the
        # 5 ms saved on launches outweigh the <= 0.6 ms all-reduce they leave exposed.  UNMEASURED on RCCL with N > 1
        # (no multi-GPU box was available; two ranks sharing one GPU over gloo: tests/test_grad_overlap_gpu.py).
        self.grad_bf16 = os.environ.get("DL_GRAD_BF16", "0") == "1"     # bf16 gradient all-reduce (see _all_reduce_runs)
        # DL_GRAPH_ALLREDUCE=1: graph-replayed steps capture their gradient all-reduce (RCCL) instead of issuing it after
        # the replay; "force": also at world size 1 (single-GPU check of the capture path).  Off by default until a
        # multi-GPU run of it is on record.
        ga = os.environ.get("DL_GRAPH_ALLREDUCE", "0")
        self.graph_allreduce = "force" if ga == "force" else (ga == "1")
        ov = os.environ.get("DL_GRAD_OVERLAP", "0")
        grouped = dist.is_available() and dist.is_initialized()
        want_overlap = ((self.world > 1 and ov not in ("0", "")) or (ov == "force" and grouped)) and not graph_steps
        self.overlap = GradOverlap(self.flat) if want_overlap else None
        if self.overlap is not None:
            ops.dynamic_tiles(True)      # persistent GEMMs hand their tiles out dynamically while collectives share the CUs
            ops.reset_tickets()
            # (bucket all-reduces are issued from backward hooks: hints_of keeps the forward on one stream then)
        # hook-driven collectives cannot be launched from inside a graph replay: graphed steps reduce after the replay
        self.graph_steps = ("auto" if graph_steps == "auto" else bool(graph_steps)) if self.overlap is None else False
        self._graphs: Dict[tuple, GraphedStep] = {}
        self._agreed_sets: Dict[str, frozenset] = {}
        self._eager_seen: Dict[tuple, int] = {}
        self._graph_caps: Dict[tuple, tuple] = {}   # per (kind, batch signature, by-value scalars): the largest capacities asked for
        self.graph_captures = 0                     # captures made so far (tests / bench: bounded under varying lengths)
        self.graph_warmup = 2            # eager (real) steps of a batch shape before its graph is captured
        self.graph_cache_max = max(1, int(os.environ.get("DL_GRAPH_CACHE_MAX", "6")))     # live GraphedSteps (LRU)
        # A device synchronisation every `graph_sync_every` replays (0 = never).  Round 5 saw ONE hardware exception after
        # ~300 replays that no host call separated (an experimental head, since removed); every shipped step
        # kind soaks clean for 2000+ unsynchronised replays (tools/graph_nosync_soak.py), but the mechanism was never found,
        # so the replay queue is bounded: one stream synchronise per 256 steps costs < 0.1 % of a training loop that does not
        # read its losses (one that does synchronises every step anyway).
        self.graph_sync_every = max(0, int(os.environ.get("DL_GRAPH_SYNC_EVERY", "256")))
        self._replays_since_sync = 0
        self._plan_devs: Dict[tuple, object] = {}           # ProteinCNN row tables of eager steps, one set per shape
        # DL_FIXED_CAPS="<drug-token block>,<ProteinCNN table rows | none>": one capacity for every step of this trainer (the
        # deterministic mode: row reductions associate by capacity, so bits otherwise depend on which graph / bucket serves a
        # batch — INTEGRATION.md "Reproducibility"); the attribute `fixed_caps` is the programmatic form.
        fc = os.environ.get("DL_FIXED_CAPS", "")
        if fc:
            a, b = (fc.split(",") + ["none"])[:2]
            self.fixed_caps = (int(a), None if b.strip().lower() in ("", "none") else int(b))
        on_gpu = torch.device(self.device).type == "cuda"
        self._guard_pin = torch.zeros(1, dtype=torch.int32).pin_memory() if on_gpu else None
        self._guard_event = None
        # (the classification loss's own guard word and its pinned copy exist only with cls_loss: created here, before any capture)
        self._cls_pin = torch.zeros(1, dtype=torch.int32).pin_memory() if (on_gpu and cls_loss is not None) else None
        if self._cls_pin is not None:
            ops.cls_loss_flags(self.device)
        if self.graph_steps:
            ops.use_seed_offset(True)    # one dropout-seed regime for eager and replayed steps

    # -- helpers ------------------------------------------------------------------------------------
    def sync_replicas(self, src: int = 0):
        """Broadcast the parameter arena, the EMA shadow (where there is one) and every module buffer from rank `src` (no-op at
        world size 1)."""
        if self.world <= 1:
            return
        dist.broadcast(self.flat.arena, src=src)
        if self.ema is not None:
            dist.broadcast(self.ema.shadow, src=src)
        for b in self.model.buffers():
            dist.broadcast(b, src=src)
        Fn.bump_param_epoch()

    def replicas_in_sync(self) -> bool:
        """True iff every rank holds bit-identical parameters — and, with the weight EMA on, a bit-identical shadow (a cheap
        checksum all-gather; used by tests / on demand)."""
        if self.world <= 1:
            return True

        def checksum(a):
            return torch.stack((a.double().sum(), a.double().abs().sum(), (a.double() * torch.arange(1, a.numel() + 1, device=a.device,
                                                                                                      dtype=torch.float64) % 9973).sum()))
        chk = checksum(self.flat.arena)
        if self.ema is not None:
            chk = torch.cat((chk, checksum(self.ema.shadow)))
        allc = [torch.empty_like(chk) for _ in range(self.world)]
        dist.all_gather(allc, chk)
        return all(torch.equal(allc[0], c) for c in allc[1:])

    def _zero_grad(self):
        for p in self.flat.params:
            p.grad = None

    def _arm(self, last: str, kind: str):
        if self.overlap is not None and last == kind:
            self.overlap.arm(kind)

    def _reduce_and_pack(self, kind: str = "cls") -> List[int]:
        if self.overlap is not None:
            return self.overlap.finish()
        idx = self.flat.pack_grads()
        if self.world > 1:
            idx = self._agreed(kind, idx)
            self._all_reduce_runs(idx)
        return idx

    def _all_reduce_runs(self, idx: List[int]):
        """Sum the flat gradient buffer over the ranks, one collective per contiguous run of parameters (usually one).
        grad_bf16 (DL_GRAD_BF16=1, off by default: the reference's DDP reduces fp32 and bit-parity tests need it): the
        run is cast to bf16, reduced (half the bytes on the xGMI links: 28 MB instead of 56 MB) and cast back into the
        fp32 buffer the optimiser reads — fp32 master weights and moments are untouched; every rank applies the same
        rounded sum, so replicas stay bit-identical to each other."""
        for s, e, _ in self.flat.runs(idx, lambda i: 0):
            g = self.flat.grads[s:e]
            if self.grad_bf16:
                h = ops.cast(g, torch.bfloat16)
                dist.all_reduce(h, op=dist.ReduceOp.SUM)
                g.copy_(h)
            else:
                dist.all_reduce(g, op=dist.ReduceOp.SUM)

    def _agreed(self, kind: str, have: List[int]) -> List[int]:
        """The parameter set every rank reduces for a backward pass of `kind`: the union over ranks of the parameters that
        received a gradient, agreed on ONCE per kind (one small MAX all-reduce in the first pass of that kind — the only
        host synchronisation; later steps issue no extra collective).  A parameter of the set without a local gradient
        contributes zeros (what DDP's find_unused_parameters does for the reference, trainer.py:147); a gradient OUTSIDE
        the agreed set means the graph changed between steps and raises (ranks must not silently issue different
        collectives)."""
        n = len(self.flat.params)
        if self._agreed_sets is None:
            self._agreed_sets = {}
        cached = self._agreed_sets.get(kind)
        if cached is None:
            mask = torch.zeros(n, dtype=torch.int32)
            mask[have] = 1
            mask = mask.to(self.flat.grads.device)
            dist.all_reduce(mask, op=dist.ReduceOp.MAX)
            cached = self._agreed_sets[kind] = frozenset(mask.cpu().nonzero().flatten().tolist())
        extra = set(have) - cached
        if extra:
            raise RuntimeError("Trainer: %d parameters outside the set agreed for '%s' backward passes received a gradient "
                               "(first: index %d); the graph changed between steps" % (len(extra), kind, min(extra)))
        missing = sorted(cached - set(have))
        if missing:
            torch._foreach_zero_([self.flat.grad_views[i] for i in missing])
        return sorted(cached)

    def set_lrs(self, lr=None, ssl_lr=None, cm_lr=None):
        if lr is not None:
            self.opt.lr = lr
        if ssl_lr is not None and self.opt_ssl:
            self.opt_ssl.lr = ssl_lr
        if cm_lr is not None and self.opt_cm:
            self.opt_cm.lr = cm_lr

    def model_has_global_ntxent(self) -> bool:
        ssl = getattr(self.model, "ssl_model", None)
        return bool(ssl is not None and getattr(ssl, "global_batch", False) and getattr(ssl, "drug_ssl_type", "") == "simclr")

    GRAPH_AUTO_MAX_BATCH = 128

    def wants_graph(self, batch_size: int, compute_cm: bool) -> bool:
        """graph_steps as a per-step decision (True / False / "auto": see the class docstring)."""
        if self.graph_steps == "auto":
            return batch_size <= self.GRAPH_AUTO_MAX_BATCH or bool(compute_cm)
        return bool(self.graph_steps)

    def graphed_kind_ok(self, compute_ssl: bool, compute_cm: bool) -> bool:
        """Whether a step kind may replay a graph at this world size (bench.py reports `hip_graph` from it)."""
        coll_ok = self.world == 1 or (bool(self.graph_allreduce) and dist.get_backend() == "nccl")
        cm = getattr(self.model, "cm_model", None)
        return ((not compute_ssl) or coll_ok or not self.model_has_global_ntxent()) and \
            ((not compute_cm) or coll_ok or not (cm is not None and cm.global_batch))

    def protein_plan_of(self, meta, batch, must_pay: bool = True):
        """The ProteinCNN distinct-row spec (protein_plan.PlanSpec: residue counts + the rows the compact layout needs; no
        tables — those are built on the device) of a batch from the collate's `Prot_Len` records (residue counts after the
        reference's truncation, handler/dataset.py:36,139), or None (no records / switched off / nothing to save)."""
        if not meta or not getattr(self.model, "compact_cnn", False) or any("Prot_Len" not in m_ for m_ in meta):
            return None
        vp = batch[1]
        if not (torch.is_tensor(vp) and vp.dim() == 2 and vp.shape[0] == len(meta)):
            return None
        from .protein_plan import PlanSpec
        spec = PlanSpec([m_["Prot_Len"] for m_ in meta], int(vp.shape[1]))
        return spec if (spec.pays() or not must_pay) else None

    def hints_of(self, meta, batch, own_tables: bool = False, kind: str = "cls", caps=None):
        """BatchHints for model(..., hints=...): the drug-token block (padding_hints_of) and the ProteinCNN plan's device
        tables.  Eager steps share one table set per shape (refilled in place, stream-ordered); own_tables=True gives the
        caller its own (a captured graph keeps pointing at them).  caps = (drug-token block, table rows or None): capacities
        to use instead of the tightest ones for this batch (the steps around a graph capture run at the capture's sizes)."""
        from .protein_plan import BatchHints, PlanDev
        if caps is None:
            caps = self.fixed_caps
        plan = self.protein_plan_of(meta, batch, must_pay=caps is None)
        blk = self.padding_hints_of(meta, batch).get("drug_tokens", 0)
        rows = 0
        if caps is not None:
            blk, rows = caps[0], caps[1]
            if rows is None:
                plan = None
        pd = None
        if plan is not None:
            rows = rows or plan.rows()
            key = (rows, plan.B, plan.S)
            if own_tables:
                pd = PlanDev(plan, self.device, rows=rows)
            else:
                pd = self._plan_devs.pop(key, None)
                if pd is None:
                    while len(self._plan_devs) >= 4:
                        del self._plan_devs[next(iter(self._plan_devs))]
                    pd = PlanDev(plan, self.device, rows=rows)
                else:
                    pd.fill(plan)
                self._plan_devs[key] = pd           # most recently used last
        # side streams for the forward's independent branches on cls steps only (measured; BatchHints.__init__), and never
        # while gradient buckets are reduced from backward hooks (one stream for the collectives)
        return BatchHints(blk, pd,
                          branch_streams=(kind == "cls" and self.overlap is None),
                          raw_attention=False)       # (a training step never reads the PGCA raw-logit maps: reference trainer.py:179-231)

    # -- device-side padding guards (ops.guard_flags): polled without a host sync, checked with one on demand -------------
    def _poll_guard(self):
        """Raise if a guard tripped in an earlier step (reads the pinned copy the previous steps posted; never waits)."""
        if self._guard_pin is None:
            return
        ev = self._guard_event
        if ev is not None and ev.query():
            bits = int(self._guard_pin[0])
            cls_bits = int(self._cls_pin[0]) if self._cls_pin is not None else 0
            self._guard_event = None
            if bits or cls_bits:
                ops.guard_flags(self.device).zero_()
                if cls_bits:
                    ops.cls_loss_flags(self.device).zero_()
                raise RuntimeError(ops.guard_message(bits, cls_bits, " in an earlier step"))

    def _post_guard(self):
        if self._guard_pin is None or self._guard_event is not None:
            return                                        # one copy in flight at a time (the word is sticky)
        self._guard_pin.copy_(ops.guard_flags(self.device), non_blocking=True)
        if self._cls_pin is not None:
            self._cls_pin.copy_(ops.cls_loss_flags(self.device), non_blocking=True)
        self._guard_event = torch.cuda.Event()
        self._guard_event.record()

    def check_device_flags(self):
        """Synchronising check of the padding guards (end of an epoch, of an evaluation, of a benchmark)."""
        if torch.device(self.device).type == "cuda":
            # (the copy of the word that an earlier step posted for _poll_guard is older than what is read here: drop it, or a
            #  trip raised — and cleared — below would be raised a second time by the next step's poll)
            self._guard_event = None
            ops.check_guard_flags(self.device)

    @staticmethod
    def padding_hints_of(meta, batch) -> dict:
        """Host-side knowledge about the batch for the model (functional.padding_hints).  drug_tokens: a block size (multiple
        of 64, so that captured graphs are keyed by few values) that covers the token count of every molecule of the batch,
        from the collate's `Drug_Tokens` records; absent records or a block that saves nothing: no hint."""
        if not meta or any("Drug_Tokens" not in m_ for m_ in meta):
            return {}
        n_rows = int(batch[3].shape[1]) if torch.is_tensor(batch[3]) and batch[3].dim() == 3 else 0
        blk = (max(int(m_["Drug_Tokens"]) for m_ in meta) + 127) // 128 * 128      # 128 / 256 / 384: few graph keys
        return {"drug_tokens": blk} if 0 < blk <= n_rows - 128 else {}

    # -- the step ---------------------------------------------------------------------------------------
    def training_step(self, batch, meta=None, cur_epoch: int = 1, ssl_masks=None) -> Dict[str, float]:
        """batch = (feat_d, feat_p, labels, llm_d, llm_p) as the reference's collate yields them.
        cur_epoch is 1-based (trainer.py:180).  Returns the losses as detached DEVICE scalars ({'cls': ..., 'ssl': ..., 'cm': ...}): the
        step itself never synchronises with the host (reading a value does), so steps are enqueued back to back."""
        m = self.model
        if self._ema_swapped:
            raise RuntimeError("Trainer.training_step inside ema_weights(): the arena holds the averaged weights")
        self._poll_guard()
        w_host = None
        if self.cls_loss is not None:
            w_host = meta_weights(meta)          # (raises when only some entries carry a "Weight")
            if w_host is not None and w_host.numel() != int(batch[2].shape[0]):
                raise ValueError("Trainer.training_step: meta holds %d weights for a batch of %d" % (w_host.numel(), int(batch[2].shape[0])))
        if not m.training:
            m.train()                  # (walks every submodule: 0.7 ms per call)
        compute_ssl = self.use_ssl and (cur_epoch % self.ssl_epoch_step == 0)
        compute_cm = self.use_cm and (cur_epoch >= self.cm_init_epoch)
        eager_caps = None
        # steps with the CM head replay a graph too (round 3) except: in the epoch the head starts (the cm_weight
        # auto-scale below reads losses on the host), without id records, and in the global-batch form (object collectives)
        # Heads that see the GLOBAL batch issue collectives in their forward and backward (NT-Xent rows, CM token means and
        # id codes: tensor collectives only since round 4).  A step with them is captured only where captured collectives
        # are switched on (DL_GRAPH_ALLREDUCE) AND the backend is RCCL; on gloo (every two-rank test) it stays eager.
        coll_ok = self.world == 1 or (bool(self.graph_allreduce) and dist.get_backend() == "nccl")
        cm_ok = (not compute_cm) or (cur_epoch > self.cm_init_epoch and meta is not None and
                                     (coll_ok or not m.cm_model.global_batch))
        ssl_ok = (not compute_ssl) or coll_ok or not self.model_has_global_ntxent()
        if self.wants_graph(int(batch[2].shape[0]), compute_cm) and cm_ok and ssl_ok and not self.run_dead_backward and \
                (not compute_ssl or ssl_masks is None):
            kind = (("ssl" if compute_ssl else "") + ("cm" if compute_cm else "")) or "cls"
            byval = (float(m.cm_model.m_sch_loss_fn.margin), float(self.cm_weight)) if compute_cm else ()
            # (frozen BatchNorm is by-value knowledge of a capture too: such a graph has no statistics launches)
            base = (kind,) + (("frozen_bn",) if getattr(m, "bn_frozen", False) else ()) + GraphedStep.signature(batch) + byval
            if self.cls_loss is not None:            # (the loss's constants are by-value arguments of a capture; with / without weights: another body)
                base += (("cls_loss", dataclasses.astuple(self.cls_loss), w_host is not None),)
            # (must_pay=False for the LOOKUP: a batch whose compact layout would not pay on its own still fits — and replays —
            #  a graph that holds tables of its size; GraphedStep.run builds its spec the same way)
            spec_any = self.protein_plan_of(meta, batch, must_pay=False)
            blk = self.padding_hints_of(meta, batch).get("drug_tokens", 0)
            g = self._find_graph(base, blk, spec_any)
            if g is not None:
                return self._graphed_step(g, batch, meta, w_host)
            spec = spec_any if (spec_any is not None and spec_any.pays()) else None
            # No captured graph serves this batch.  Capacities of the next capture: size CLASSES (row_class: a geometric
            # ladder; drug-token blocks of 128), never below what an earlier batch of this shape asked for — so the captures
            # of a shape form a chain of growing capacities and batches of varying lengths converge on one or two graphs
            # (round 4 keyed graphs by the exact 2048-row bucket: ~10 keys at batch 256, capture / eviction thrash).
            # The eager warm-up steps of a capacity run at that capacity (same shapes as the capture).
            eager_caps = self._capture_caps(base, blk, spec)
            key = base + eager_caps
            if self._eager_seen.get(key, 0) >= self.graph_warmup:
                return self._graphed_step(self._capture(key, base, byval, batch, kind, meta, eager_caps), batch, meta, w_host)
            if len(self._eager_seen) > 256:            # bounded bookkeeping (signatures of shapes seen once and never again)
                self._eager_seen.clear()
            self._eager_seen[key] = self._eager_seen.get(key, 0) + 1
        kind_now = "cm" if compute_cm else "ssl" if compute_ssl else "cls"
        out, last = self._forward_backward(batch, compute_ssl, compute_cm, hints=self.hints_of(meta, batch, kind=kind_now, caps=eager_caps),
                                           weights=w_host, ssl_masks=ssl_masks, cm_labels={"meta": meta},
                                           cm_autoscale=cur_epoch == self.cm_init_epoch)
        self._finish_step(self._reduce_and_pack(last), compute_ssl, compute_cm, out)
        return out

    def _forward_backward(self, batch, compute_ssl: bool, compute_cm: bool, *, hints, weights, cm_labels: dict, ssl_masks=None,
                          cm_autoscale: bool = False):
        """The body of a step, eager or under capture (GraphedStep._body): forward, classification loss, SSL head, CM head and
        the backward passes; returns (losses, the backward the optimisers consume).  What the two callers do differently is
        an argument: the hints, the per-sample weights (host or device, or None), ssl_masks, how the CM head gets its labels
        (cm_labels: {"meta": ...} or {"labels": ...}) and cm_autoscale, the cm_init_epoch step that scales cm_weight from the two
        losses — eager only, it reads the host.  The backward of head X runs when X is the last head or run_dead_backward is
        set; a captured step never has run_dead_backward."""
        m = self.model
        feat_d, feat_p, labels, llm_d, llm_p = batch
        _, _, ssl_input, cm_input, score = m(feat_d, feat_p, llm_d, llm_p, hints=hints)
        self._zero_grad()
        if self.cls_loss is not None:
            _, cls_loss = classification_loss(score, labels, self.cls_loss, None if weights is None else weights.to(self.device))
        else:
            _, cls_loss = binary_cross_entropy(score, labels) if self.n_class == 1 else cross_entropy_logits(score, labels)
        last = "cm" if compute_cm else "ssl" if compute_ssl else "cls"     # the backward the optimisers consume
        if last == "cls" or self.run_dead_backward:
            self._arm(last, "cls")
            cls_loss.backward(retain_graph=compute_ssl or compute_cm)
        out = {"cls": cls_loss.detach()}
        if compute_ssl:
            self._zero_grad()
            kw = dict(ssl_input)
            if ssl_masks is not None:
                kw.update(mask=ssl_masks[0], replace=ssl_masks[1])
            with m._glue(), Fn.deferred_bn_ticks():     # bf16 compute dtype: the heads' torch layers run under bf16 autocast; the
                d = m.ssl_model(**kw)                   # BatchNorm step counters of the heads advance in one launch
            ssl_loss = (d["prot_ssl"] + d["drug_ssl"]) * 0.1
            if last == "ssl" or self.run_dead_backward:
                self._arm(last, "ssl")
                ssl_loss.backward(retain_graph=compute_cm)
            out["ssl"] = ssl_loss.detach()
        if compute_cm:
            self._zero_grad()
            with m._glue():
                cm_loss = m.cm_model(**cm_input, **cm_labels)
            if cm_autoscale:
                c, l = float(cm_loss.detach()), float(cls_loss.detach())
                if c > 0:
                    while c * self.cm_weight / 10 > l:
                        self.cm_weight /= 10
                    while c * self.cm_weight * 10 < l:
                        self.cm_weight *= 10
            cm_loss = cm_loss * self.cm_weight
            self._arm(last, "cm")
            cm_loss.backward()
            out["cm"] = cm_loss.detach()
        return out, last

    def _finish_step(self, idx: List[int], ssl: bool, cm: bool, out: dict):
        """The tail of a step, eager or replayed, from the reduced gradients of `idx` on: the guard's decision ("grad_norm" goes
        into `out`), the optimiser steps, the EMA update, the weight images' epoch and the padding guards' poll copy."""
        scale = 1.0 / self.world
        guard = self._decide_grad_guard(idx, out)
        self.opt.step(idx, scale, guard)
        if ssl:
            self.opt_ssl.step(idx, scale, guard)
        if cm:
            self.opt_cm.step(idx, scale, guard)
        if self.ema is not None:
            self.ema.update(guard)
        Fn.bump_param_epoch()
        self._post_guard()

    # -- gradient guard ---------------------------------------------------------------------------------------------------
    def _decide_grad_guard(self, idx: List[int], out: dict):
        """Guard on: the step's ONE decision, from the reduced gradient runs of `idx` (sum-of-squares passes + finalize, no host
        sync); returns the device tensor the optimiser kernels read and puts "grad_norm" into the step's result.  Guard off:
        None, and nothing is launched."""
        gg = self.grad_guard
        if gg is None:
            return None
        key = tuple(idx)                     # (the runs of a parameter set are computed once: ~250 parameters of Python per call)
        if self._guard_runs is None or self._guard_runs[0] != key:
            self._guard_runs = (key, [self.flat.grads[s:e] for s, e, _ in self.flat.runs(idx, lambda i: 0)])
        guard = gg.decide(self._guard_runs[1], pre_scale=1.0 / self.world)
        out["grad_norm"] = guard[1]          # a view: read it before the next step overwrites it
        return guard

    def grad_guard_stats(self) -> Dict[str, float]:
        """Host values of the guard: the last step's norm (of the averaged gradient) and clip coefficient, and the cumulative
        numbers of skipped and clipped steps.  Reading synchronises, like reading a loss."""
        if self.grad_guard is None:
            raise RuntimeError("Trainer.grad_guard_stats: the gradient guard is off (max_grad_norm / skip_nonfinite)")
        g = self.grad_guard.guard.tolist()
        c = self.grad_guard.counters.tolist()
        return {"norm": g[1], "coef": g[0], "skipped": int(c[0]), "clipped": int(c[1])}

    # -- parameter groups -------------------------------------------------------------------------------------------------
    def set_param_group(self, name: str, lr_scale: Optional[float] = None, weight_decay: Optional[float] = None):
        """New lr_scale and / or weight_decay for one group ("default" included), from the next step on: one row of the device
        table is rewritten (a small copy between steps).  ValueError for an unknown name or a negative / non-finite value;
        whether a group is frozen cannot change."""
        if self.param_groups is None:
            raise RuntimeError("Trainer.set_param_group: parameter groups are off (param_groups)")
        self.param_groups.set(name, lr_scale=lr_scale, weight_decay=weight_decay)

    def param_group_table(self) -> List[tuple]:
        """[(group name, parameter name, numel)] in parameter order."""
        if self.param_groups is None:
            raise RuntimeError("Trainer.param_group_table: parameter groups are off (param_groups)")
        return self.param_groups.table()

    # -- weight EMA -------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the parameter arena holds the averaged weights (the live bits wait in a spare buffer); on exit,
        exceptions included, the live bits are back.  The parameter epoch is bumped both ways, so predict, evaluate, screen,
        build_library, screen_library and hit_* work unchanged on the averaged weights: weight images are refreshed, codes
        and libraries built inside are stale outside (the existing parameter-epoch check), and a library built inside carries
        the fingerprint of the averaged weights.  Buffers — BatchNorm running statistics among them — are SHARED with the live
        model, not averaged (torch.optim.swa_utils.AveragedModel's default, use_buffers=False).  Entering twice raises, and
        so does training_step inside the context."""
        if self.ema is None:
            raise RuntimeError("Trainer.ema_weights: the weight EMA is off (ema_decay)")
        if self._ema_swapped:
            raise RuntimeError("Trainer.ema_weights: already inside ema_weights()")
        if self._ema_spare is None:
            self._ema_spare = torch.empty_like(self.flat.arena)
        with torch.no_grad():
            self._ema_spare.copy_(self.flat.arena)
            self.flat.arena.copy_(self.ema.shadow)
        self._ema_swapped = True
        Fn.bump_param_epoch()
        try:
            yield self
        finally:
            with torch.no_grad():
                self.flat.arena.copy_(self._ema_spare)
            self._ema_swapped = False
            Fn.bump_param_epoch()

    def adopt_ema(self):
        """Copy the averaged weights into the live arena for good (model.state_dict() then holds them: deployment) and bump
        the parameter epoch.  The optimisers' moments are left as they are."""
        if self.ema is None:
            raise RuntimeError("Trainer.adopt_ema: the weight EMA is off (ema_decay)")
        if self._ema_swapped:
            raise RuntimeError("Trainer.adopt_ema inside ema_weights(): the exit would put the live weights back")
        with torch.no_grad():
            self.flat.arena.copy_(self.ema.shadow)
        Fn.bump_param_epoch()

    # -- captured graphs: lookup by capacity, capture at size classes -------------------------------------------------------
    _INF = 1 << 60

    def _find_graph(self, base, blk: int, spec):
        """The tightest captured graph of this (kind, batch signature, by-value scalars) whose capacities hold the batch: a
        drug-token block >= the batch's (0 = every row computed: holds anything) and ProteinCNN tables with >= the rows the
        batch needs (no tables = every position computed: holds anything)."""
        best, best_cost = None, None
        for g in self._graphs.values():
            if g.base != base:
                continue
            if g.block != 0 and (blk == 0 or g.block < blk):
                continue
            if g.rows_cap is not None and (spec is None or spec.need > g.rows_cap):
                continue
            cost = (g.rows_cap if g.rows_cap is not None else self._INF, g.block or self._INF)
            if best is None or cost < best_cost:
                best, best_cost = g, cost
        return best

    def fixed_caps_for(self, batches) -> tuple:
        """Capacities that hold every (batch, meta) of `batches` (for `fixed_caps`)."""
        from .protein_plan import row_class
        blks = [self.padding_hints_of(mt, b).get("drug_tokens", 0) for b, mt in batches]
        specs = [self.protein_plan_of(mt, b) for b, mt in batches]
        rows = None if any(sp is None for sp in specs) else row_class(max(sp.need for sp in specs))
        return (0 if 0 in blks else max(blks), rows)

    def _capture_caps(self, base, blk: int, spec) -> tuple:
        from .protein_plan import row_class
        if self.fixed_caps is not None:
            return tuple(self.fixed_caps)
        rows = None if spec is None else row_class(spec.need)
        if spec is not None and not spec.pays(rows):
            rows = None
        # The chain of growing capacities per shape.  A batch WITHOUT a usable plan (no Prot_Len records, or a compact layout
        # that does not pay) is served by the full layout for that batch only: it must not erase what earlier batches asked for
        # (round 5 made rows=None sticky: one such batch and every later capture of the shape used ~3.5x the rows).
        old = self._graph_caps.get(base)
        keep_blk, keep_rows = blk, rows
        if old is not None:
            if blk != 0 and old[0] != 0:
                blk = keep_blk = max(blk, old[0])
            elif blk == 0:
                keep_blk = old[0]               # (0 = every drug row computed: this batch has no token records)
            if rows is not None and old[1] is not None:
                rows = keep_rows = max(rows, old[1])
            elif rows is None:
                keep_rows = old[1]
        if len(self._graph_caps) > 256:
            self._graph_caps.clear()
        self._graph_caps[base] = (keep_blk, keep_rows)
        return (blk, rows)

    def _capture(self, key, base, byval, batch, kind, meta, caps) -> "GraphedStep":
        if "cm" in kind:
            # margin / cm_weight are by-value arguments of a capture: EVERY graph with the CM head ("cm" and "sslcm"
            # kinds, any shape or hint) captured under other values will not be replayed again (the margin moves once
            # per epoch) — release their pools first
            for old in [k for k, v in self._graphs.items() if "cm" in v.kind and v.byval != byval]:
                del self._graphs[old]
        # Every GraphedStep owns a private pool with a whole step's activations (GBs at batch 64-128): keep at most
        # graph_cache_max of them, least recently replayed first out
        while len(self._graphs) >= self.graph_cache_max:
            del self._graphs[next(iter(self._graphs))]
        g = self._graphs[key] = GraphedStep(self, batch, kind, meta, caps)     # records only; the replay that follows is the step
        g.base, g.byval, g.key = base, byval, key
        self.graph_captures += 1
        return g

    def _graphed_step(self, g: "GraphedStep", batch, meta=None, weights=None) -> Dict[str, float]:
        self._graphs[g.key] = self._graphs.pop(g.key)                        # most recently used last
        out, idx = g.run(batch, meta, weights)
        if self.world > 1 and not g.reduced:
            idx = self._agreed(g.last, idx)
            self._all_reduce_runs(idx)
        if self.grad_guard is not None:
            out = dict(out)                  # (the graph's own result dict stays as captured)
        self._finish_step(idx, "ssl" in g.kind, "cm" in g.kind, out)
        self._replays_since_sync += 1
        if self.graph_sync_every and self._replays_since_sync >= self.graph_sync_every:
            torch.cuda.current_stream(self.device).synchronize()
            self._replays_since_sync = 0
        return out

    def static_batch(self, batch):
        """The captured graph's own input tensors for batches of this shape (or `batch` itself while no graph exists):
        a producer that fills them in place — and passes them back — saves the per-step input copy."""
        shape = GraphedStep.signature(batch)
        g = next((v for k, v in self._graphs.items() if k[1:1 + len(shape)] == shape), None)
        return batch if g is None else g.static

    def on_train_epoch_end(self, cur_epoch: int):
        compute_ssl = self.use_ssl and (cur_epoch % self.ssl_epoch_step == 0)
        compute_cm = self.use_cm and (cur_epoch >= self.cm_init_epoch)
        self.opt.lr = self.schd.step()
        if compute_ssl:
            self.opt_ssl.lr = self.schd_ssl.step()
        if compute_cm:
            self.opt_cm.lr = self.schd_cm.step()
            self.model.cm_model.step()
        self.check_device_flags()                      # (an epoch boundary: a host sync costs nothing here)

    # -- checkpoints (checkpoint.py: the file format and its checks) --------------------------------------------------------
    def _opt_schd(self):
        """[(name, optimiser, its scheduler)] of the optimisers that exist."""
        return [(n, o, s) for n, o, s in (("opt", self.opt, self.schd), ("opt_ssl", self.opt_ssl, self.schd_ssl),
                                          ("opt_cm", self.opt_cm, self.schd_cm)) if o is not None]

    def checkpoint_signature(self) -> dict:
        """What a checkpoint of this trainer is valid for (checkpoint.MUST_MATCH: a load is refused on a difference;
        checkpoint.WARN_ONLY: a load warns)."""
        names = {id(p): n for n, p in self.model.named_parameters()}
        return {
            "model": type(self.model).__name__,
            "params": [[names[id(p)], list(p.shape), off] for p, off in zip(self.flat.params, self.flat.offsets)],
            "compute_dtype": str(self.compute_dtype).split(".")[-1],
            "world": int(self.world),
            "optimisers": [n for n, _, _ in self._opt_schd()],
            "ema": {"on": self.ema is not None, "decay": None if self.ema is None else self.ema.decay,
                    "warmup": None if self.ema is None else self.ema.warmup},
            "guard": {"on": self.grad_guard is not None, "max_grad_norm": self.max_grad_norm, "skip_nonfinite": self.skip_nonfinite},
            "freeze_bn": self.freeze_bn,
            "cls_loss": None if self.cls_loss is None else dataclasses.asdict(self.cls_loss),
            "param_groups": None if self.param_groups is None else self.param_groups.assignment(),
            "graph_steps": self.graph_steps,
            "fixed_caps": None if self.fixed_caps is None else list(self.fixed_caps),
        }

    def _gather_host(self, t: torch.Tensor) -> List[torch.Tensor]:
        """A small CPU tensor of every rank, in rank order (a list of one at world size 1; a collective otherwise)."""
        if self.world <= 1:
            return [t]
        mine = t.to(self.device) if dist.get_backend() == "nccl" else t
        out = [torch.empty_like(mine) for _ in range(self.world)]
        dist.all_gather(out, mine)
        return [o.cpu() for o in out]

    def _rng_state(self) -> dict:
        """The random state a step consumes, per rank: the dropout site-seed generator, the device-resident seed offset (and
        whether it is in use), torch's CPU generator and torch's device generator (the MLM mask draw of the SSL heads)."""
        seed = ops.seed_state(torch.device(self.device))
        on_gpu = torch.device(self.device).type == "cuda"
        dev_state = torch.cuda.get_rng_state(self.device) if on_gpu else torch.zeros(0, dtype=torch.uint8)
        return {"seed_gen": self._gather_host(seed["generator"]),
                "seed_offset": [int(t) for t in self._gather_host(torch.tensor([seed["offset"]], dtype=torch.int64))],
                "seed_offset_on": seed["offset_on"],
                "cpu": self._gather_host(torch.get_rng_state()),
                "device": self._gather_host(dev_state)}

    def save_checkpoint(self, path, extra: Optional[dict] = None) -> None:
        """Write everything a later load_checkpoint needs to go on from here bit for bit, as one file (checkpoint.py: the
        layout; the file is also a weight file that load_reference_checkpoint accepts).  Call it between steps: it
        synchronises the device once and runs check_device_flags() first — the checkpoint of a step that tripped a guard is
        refused (RuntimeError, nothing written).  Saved: the model's state_dict (parameters, buffers, the lazily created
        SimSiam projectors once they exist); per optimiser both moments, the step counts and the lr; the schedulers;
        cm_weight and the cross-modality head's margin schedule; the EMA shadow and its update count; the guard counters;
        the parameter groups' current values; fixed_caps; the random state of every rank (_rng_state); `extra`, a dict of
        plain data (tensors, scalars, strings, lists, dicts) that load_checkpoint returns.  Not saved, because they are
        rebuilt: the gradient buffer, captured graphs and their bookkeeping, agreed gradient sets, weight images, workspaces.
        The write is atomic (an existing file survives a failed write).  At world > 1 EVERY rank calls this (the ranks' random
        states are gathered), rank 0 writes, and all ranks leave together once the file exists.
        A trainer that saved launches exactly what it launches otherwise: no hook, stream or flag is left behind."""
        if self._ema_swapped:
            raise RuntimeError("Trainer.save_checkpoint inside ema_weights(): the arena holds the averaged weights")
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize(self.device)
        self.check_device_flags()
        cm = getattr(self.model, "cm_model", None)
        state = {
            "optimisers": {n: o.state() for n, o, _ in self._opt_schd()},
            "schedulers": {n: s.state() for n, _, s in self._opt_schd()},
            "cm_weight": float(self.cm_weight),
            # (the margin schedule of the CM head is host state outside its state_dict: on_train_epoch_end steps it)
            "cm_margin": None if cm is None else {"step": int(cm.m_sch_loss_fn._step), "m_cur": float(cm.m_sch_loss_fn.m_cur)},
            "ema": None if self.ema is None else self.ema.state(),
            "grad_guard": None if self.grad_guard is None else self.grad_guard.state(),
            "param_groups": None if self.param_groups is None else self.param_groups.state(),
            "fixed_caps": None if self.fixed_caps is None else list(self.fixed_caps),
            "rng": self._rng_state(),
        }
        err = None
        if self.rank == 0:
            try:
                ckpt.write(ckpt.pack(self.model.state_dict(), state, self.checkpoint_signature(), extra), path)
            except BaseException as e:          # (the other ranks wait at the barrier below: reach it before raising)
                if self.world <= 1:
                    raise
                err = e
        if self.world > 1:
            dist.barrier()
            if err is not None:
                raise err

    def _check_checkpoint(self, blob: dict, path) -> List[str]:
        """Everything load_checkpoint checks before it writes; returns the warning lines.  RuntimeError names the difference."""
        notes = ckpt.validate(blob, self.checkpoint_signature(), "Trainer.load_checkpoint(%s)" % (path,))
        sd, own = blob["state_dict"], self.model.state_dict()
        lazy = lambda k: ".projector." in k             # noqa: E731  (the SimSiam projectors: in the file once they exist)
        for k, v in own.items():
            if k not in sd:
                if lazy(k):
                    continue
                raise RuntimeError("checkpoint: %s has no entry %r in its state_dict" % (path, k))
            check_tensor("state_dict[%r]" % k, sd[k], v.shape, v.dtype)
        unknown = [k for k in sd if k not in own and not lazy(k)]
        if unknown:
            raise RuntimeError("checkpoint: %s holds %d state_dict entries the model does not have (first: %s)" % (path, len(unknown), unknown[0]))
        if any(lazy(k) for k in sd) and not hasattr(self.model, "ssl_model"):
            raise RuntimeError("checkpoint: %s holds SimSiam projectors, the model has no SSL head" % (path,))
        st = blob["trainer"]
        n = self.flat.numel
        for name, o, _ in self._opt_schd():
            if name not in st.get("optimisers", {}) or name not in st.get("schedulers", {}):
                raise RuntimeError("checkpoint: %s has no state of %s" % (path, name))
            o.check_state(st["optimisers"][name], name)
            sc = st["schedulers"][name]
            if any(not isinstance(sc.get(k), t) for k, t in (("step_in_cycle", int), ("cycle", int), ("lr", float))):
                raise RuntimeError("checkpoint: the scheduler state of %s is incomplete" % name)
        if self.ema is not None:
            check_tensor("ema.shadow", (st.get("ema") or {}).get("shadow"), (n,), torch.float32)
            int(st["ema"]["updates"])
        if self.grad_guard is not None:
            check_tensor("grad_guard.counters", (st.get("grad_guard") or {}).get("counters"), (2,), torch.int64)
            check_tensor("grad_guard.guard", st["grad_guard"].get("guard"), (4,), torch.float32)
        if self.param_groups is not None:
            try:
                self.param_groups.check_state(st.get("param_groups") or {})
            except ValueError as e:
                raise RuntimeError("checkpoint: %s" % e) from e
        if getattr(self.model, "cm_model", None) is not None and not isinstance(st.get("cm_margin"), dict):
            raise RuntimeError("checkpoint: %s has no margin schedule for the cross-modality head" % (path,))
        float(st["cm_weight"])
        rng = st.get("rng") or {}
        for k in ("seed_gen", "cpu", "device", "seed_offset"):
            if not isinstance(rng.get(k), list) or len(rng[k]) != self.world:
                raise RuntimeError("checkpoint: %s holds no %s random state for each of the %d ranks" % (path, k, self.world))
        return notes

    def load_checkpoint(self, path) -> dict:
        """Take over the state a save_checkpoint wrote; returns the `extra` dict of the save ({} where none was given).
        EVERYTHING is checked first — the file reads (weights_only=True), its format is known, its signature fits this trainer
        (model class, parameter names / shapes / arena offsets, world size, which optimisers exist, EMA and guard on or off,
        the parameter-group assignment: RuntimeError naming the first difference), every tensor has its shape — and only then
        written: a refused file leaves every tensor and count of the trainer untouched.  A different graph_steps or fixed_caps
        (and compute dtype, EMA / guard / loss settings, freeze_bn) only warns: the state is the same either way, the trainer
        keeps its own.  Frozen parameters keep requires_grad=False and still take the file's values.
        After writing: the parameter epoch is bumped (weight images are refreshed; entity codes and libraries built before the
        load are refused by their epoch checks), every captured graph and the bookkeeping that keys graphs is dropped (they
        bake site seeds and capacities of another history; the next steps warm up and capture anew), the device-side
        parameter-group table is rewritten.  At world > 1 every rank loads the same file (each finds its own random state in
        it) and replicas_in_sync() is verified.
        PROCESS-GLOBAL: the dropout site-seed generator, the device seed offset (value and switch) and torch's CPU and
        device generators belong to the process, not to this trainer.  A load sets them for everything in the process."""
        if self._ema_swapped:
            raise RuntimeError("Trainer.load_checkpoint inside ema_weights(): the exit would overwrite the loaded weights")
        blob = ckpt.read(path)
        notes = self._check_checkpoint(blob, path)
        from .model.model_interface import load_reference_checkpoint
        on_gpu = torch.device(self.device).type == "cuda"
        if on_gpu:
            torch.cuda.synchronize(self.device)          # (graphs are released below: nothing of them may still run)
        st, sd = blob["trainer"], blob["state_dict"]
        ssl = getattr(self.model, "ssl_model", None)
        if ssl is not None and not any(".projector." in k for k in sd):
            ssl.net.projector = ssl.llm_net.projector = None       # (not created yet in the saved history: the first SSL forward draws them)
        with torch.no_grad():
            load_reference_checkpoint(self.model, {"state_dict": sd}, strict=True)    # (builds the projectors the file holds first)
            for name, o, s in self._opt_schd():
                o.load_state(st["optimisers"][name])
                s.load_state(st["schedulers"][name])
            self.cm_weight = float(st["cm_weight"])
            cm = getattr(self.model, "cm_model", None)
            if cm is not None:
                cm.m_sch_loss_fn._step, cm.m_sch_loss_fn.m_cur = int(st["cm_margin"]["step"]), float(st["cm_margin"]["m_cur"])
            if self.ema is not None:
                self.ema.load_state(st["ema"])
            if self.grad_guard is not None:
                self.grad_guard.load_state(st["grad_guard"])
            if self.param_groups is not None:
                self.param_groups.load_state(st["param_groups"])
        rng, r = st["rng"], self.rank
        # (a graph-replaying trainer needs the offset whatever the saving one did: one seed regime for its eager and replayed steps)
        ops.set_seed_state({"generator": rng["seed_gen"][r], "offset": rng["seed_offset"][r],
                            "offset_on": bool(rng["seed_offset_on"]) or bool(self.graph_steps)}, torch.device(self.device))
        torch.set_rng_state(rng["cpu"][r])
        if on_gpu and rng["device"][r].numel():
            torch.cuda.set_rng_state(rng["device"][r], self.device)
        Fn.bump_param_epoch()
        self._graphs.clear()
        self._eager_seen.clear()
        self._graph_caps.clear()
        self._agreed_sets.clear()
        if self.overlap is not None:
            self.overlap.expected.clear()
        self._guard_runs, self._guard_event, self._replays_since_sync = None, None, 0
        if self.world > 1 and not self.replicas_in_sync():
            raise RuntimeError("Trainer.load_checkpoint(%s): the replicas are not in sync after the load (did every rank read the same file?)" % (path,))
        for line in notes:
            warnings.warn("Trainer.load_checkpoint(%s): %s" % (path, line))
        return blob["extra"]

    # -- evaluation (trainer.py:256-292; torchmetrics replaced by sklearn on the gathered predictions) -----
    @torch.no_grad()
    def predict(self, batches):
        """Eval-mode forward over `batches` (any batch size: the reference validates / tests at batch 1, main.py:146-153;
        the per-sample results do not depend on the batch because BatchNorm uses its running statistics).  Returns this
        rank's (probabilities, labels, summed BCE, sample count)."""
        self.model.eval()
        preds, labs = [], []
        loss_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        for batch in batches:
            feat_d, feat_p, labels, llm_d, llm_p = batch
            _, _, _, _, score = self.model(feat_d, feat_p, llm_d, llm_p)
            n, loss = binary_cross_entropy(score, labels) if self.n_class == 1 else cross_entropy_logits(score, labels)
            preds.append(n.float().reshape(-1))
            labs.append(labels.float().reshape(-1))
            loss_sum += loss.double() * labels.numel()              # per-batch means -> a sum over samples
        p = torch.cat(preds) if preds else torch.zeros(0, device=self.device)
        y = torch.cat(labs) if labs else torch.zeros(0, device=self.device)
        self.check_device_flags()
        return p, y, loss_sum, p.numel()

    @torch.no_grad()
    def screen(self, protein_batches, drug_batches, pair_batch: int = 256) -> torch.Tensor:
        """Library screening: the (P, D) fp32 probabilities `predict` would give for every (protein, drug) pair, with the
        per-entity part of the forward paid once per protein and once per drug (druglamp_amd/screening.py).
        protein_batches yields (feat_p, llm_p), drug_batches yields (feat_d, llm_d) as the collate hands them over (llm_d is None
        for a model without an LLM branch; llm_p is always needed: the fill bit comes from it).  The protein codes stay
        resident; the drug batches are streamed — encode one, score it against every protein in chunks of pair_batch pairs, drop
        its code — so memory is bounded by one drug batch whatever the library size.  Inside a chunk the pairs are ordered
        drug-major: consecutive workgroups of the attention launch share a drug's K | V' in L2."""
        from .screening import ProteinCode
        if pair_batch < 1:
            raise ValueError("screen: pair_batch must be positive")
        self.model.eval()
        pcode = ProteinCode.cat([self.model.encode_proteins(feat_p, llm_p) for feat_p, llm_p in protein_batches])
        P = pcode.n
        cols = []
        for feat_d, llm_d in drug_batches:
            dcode = self.model.encode_drugs(feat_d, llm_d)
            Dn = dcode.n
            di = torch.arange(Dn).repeat_interleave(P)          # drug-major
            pi = torch.arange(P).repeat(Dn)
            scores = [self.model.score_codes(pcode, dcode, pi[s:s + pair_batch], di[s:s + pair_batch]) for s in range(0, Dn * P, pair_batch)]
            score = torch.cat(scores)
            prob = torch.sigmoid(score).squeeze(1) if self.n_class == 1 else torch.softmax(score, dim=1)[:, 1]
            cols.append(prob.view(Dn, P).t())
            del dcode
        out = torch.cat(cols, dim=1).contiguous() if cols else torch.zeros((P, 0), dtype=torch.float32, device=self.device)
        self.check_device_flags()
        return out

    @torch.no_grad()
    def build_library(self, drug_batches, hints=None):
        """A resident screening.DrugLibrary of every drug of `drug_batches` (yields (feat_d, llm_d) as `screen` takes them):
        encode_drugs per batch, every drug trimmed to its own keys whatever layout its batch was encoded in.  hints: None, one
        BatchHints for every batch, or a sequence with one entry (BatchHints or None) per batch."""
        from .screening import DrugLibrary
        self.model.eval()
        per_batch = hints is not None and not hasattr(hints, "drug_tokens")
        hs = iter(hints) if per_batch else None

        def codes():
            for feat_d, llm_d in drug_batches:
                yield self.model.encode_drugs(feat_d, llm_d, next(hs) if per_batch else hints)
        lib = DrugLibrary.from_codes(codes(), self.model)
        self.check_device_flags()
        return lib

    @torch.no_grad()
    def _check_shortlist(self, who, lib, M):
        """The checks of a shortlisted call: M in [1, min(D, 1024)] (ValueError), a library with latents and a model whose
        codes carry them (RuntimeError)."""
        from . import ops
        D, M = lib.n, int(M)
        if not 1 <= M <= D:
            raise ValueError("%s: shortlist %d not in [1, %d] (the library's size)" % (who, M, D))
        if M > ops.LATENT_TOPK_MAX:
            raise ValueError("%s: shortlist %d is above the kernel's limit of %d" % (who, M, ops.LATENT_TOPK_MAX))
        if not getattr(self.model, "has_latents", False):
            raise RuntimeError("%s: the model has no cross-modality latents (a shortlist needs a two_c2p model with an LLM branch, "
                               "DrugLAMP2C2P; this is %s)" % (who, type(self.model).__name__))
        if getattr(lib, "latent", None) is None:
            raise RuntimeError("%s: the library holds no latents (built from codes of another model kind, or saved before latents "
                               "existed); build it again with Trainer.build_library" % who)
        return M

    def _shortlist_of(self, pcode, lib, M):
        from . import ops
        if pcode.latent is None:
            raise RuntimeError("shortlist: the protein codes carry no latents")
        return ops.latent_topk(pcode.latent.to(lib.latent.dtype).contiguous(), lib.latent, M)

    @torch.no_grad()
    def shortlist(self, protein_batches, lib, M: int):
        """The prefilter of a two-stage screen: for every protein the M library drugs whose cross-modality latent is nearest
        (largest cosine: both latents are l2-normalised), by ops.latent_topk against the library's resident latents.  Returns
        (sims (P, M) fp32, indices (P, M) int64), similarity descending, ties by ascending index.  The protein batches are
        streamed as in screen_library; each batch's latents are cast to the library's dtype.  How much of the exhaustive
        top-k a given M keeps depends on the trained head: shortlist_recall measures it."""
        M = self._check_shortlist("shortlist", lib, M)
        self.model.eval()
        sims, idxs = [], []
        for feat_p, llm_p in protein_batches:
            s, i = self._shortlist_of(self.model.encode_proteins(feat_p, llm_p), lib, M)
            sims.append(s)
            idxs.append(i)
        self.check_device_flags()
        if not sims:
            return (torch.zeros((0, M), dtype=torch.float32, device=self.device), torch.zeros((0, M), dtype=torch.int64, device=self.device))
        return torch.cat(sims).contiguous(), torch.cat(idxs).contiguous()

    def _screen_shortlisted(self, protein_batches, lib, pair_batch, k, M):
        """screen_library(top_k=k, shortlist=M): per protein batch the M nearest drugs by latent, the pair stage on those
        Pn x M pairs alone (chunks of pair_batch pairs, drug-major inside a chunk), then the k most probable of the M."""
        vals, idxs = [], []
        for feat_p, llm_p in protein_batches:
            pcode = self.model.encode_proteins(feat_p, llm_p)
            Pn = pcode.n
            _, cand = self._shortlist_of(pcode, lib, M)                 # (Pn, M) int64 on the device
            di_all = cand.reshape(-1).cpu()                              # (score_library takes host indices: one sync per protein batch)
            pi_all = torch.arange(Pn).repeat_interleave(M)
            prob = torch.empty(Pn * M, dtype=torch.float32, device=cand.device)
            for s0 in range(0, Pn * M, pair_batch):
                di, pi = di_all[s0:s0 + pair_batch], pi_all[s0:s0 + pair_batch]
                order = torch.argsort(di * Pn + pi)                      # drug-major: pairs of one drug sit side by side
                score = self.model.score_library(pcode, lib, pi[order], di[order])
                pr = torch.sigmoid(score).squeeze(1) if self.n_class == 1 else torch.softmax(score, dim=1)[:, 1]
                prob[s0 + order.to(prob.device)] = pr
            best_v, sel = torch.topk(prob.view(Pn, M), k, dim=1)
            vals.append(best_v)
            idxs.append(torch.gather(cand, 1, sel))
            del pcode
        self.check_device_flags()
        if not vals:
            return (torch.zeros((0, k), dtype=torch.float32, device=self.device), torch.zeros((0, k), dtype=torch.int64, device=self.device))
        return torch.cat(vals).contiguous(), torch.cat(idxs).contiguous()

    @torch.no_grad()
    def shortlist_recall(self, protein_batches, lib, top_k: int, shortlist: int, pair_batch: int = 256):
        """How much of the exhaustive screen a shortlist keeps, on the given proteins: one exhaustive screen_library(top_k) and
        one with shortlist=shortlist; per protein the share of the exhaustive top_k drugs that the shortlisted result also
        holds.  Returns {"recall": their mean (float), "per_protein": (P,) fp32 tensor}.  The diagnostic to run on a sample
        of proteins before trusting an M: the recall of the latent prefilter depends on the trained cross-modality head.
        protein_batches is walked twice (a list, or anything that can be iterated again)."""
        _, full = self.screen_library(protein_batches, lib, pair_batch=pair_batch, top_k=top_k)
        _, short = self.screen_library(protein_batches, lib, pair_batch=pair_batch, top_k=top_k, shortlist=shortlist)
        if full.shape != short.shape:
            raise RuntimeError("shortlist_recall: protein_batches gave %d proteins on the first walk and %d on the second"
                               % (full.shape[0], short.shape[0]))
        per = (full.unsqueeze(2) == short.unsqueeze(1)).any(dim=2).float().mean(dim=1) if full.shape[0] else torch.zeros(0, device=self.device)
        return {"recall": float(per.mean()) if per.numel() else float("nan"), "per_protein": per}

    @torch.no_grad()
    def screen_library(self, protein_batches, lib, pair_batch: int = 256, top_k: Optional[int] = None, shortlist: Optional[int] = None):
        """`screen` against a resident drug library: the library stays where it is, the protein batches are streamed — encode
        one, score it against every drug in chunks of pair_batch pairs (drug-major, as in `screen`), drop its code.
        top_k=None: the (P, D) fp32 probabilities of `screen`.  top_k=k: (values (P, k), indices (P, k) int64), the k most
        probable drugs per protein in descending order, merged chunk by chunk with torch.topk on the device: memory is
        O(P k + pair_batch) whatever the library size.
        shortlist=M (with top_k=k <= M <= min(D, 1024); DrugLAMP2C2P and a library with latents): retrieve, then re-rank —
        each protein's M nearest drugs by cross-modality latent (ops.latent_topk, see `shortlist`), the pair stage on those
        P x M pairs only, the k most probable of them; same return type.  The cost no longer grows with D, the result is
        the exhaustive one only as far as the latent prefilter keeps the hits (shortlist_recall measures that)."""
        if pair_batch < 1:
            raise ValueError("screen_library: pair_batch must be positive")
        D = lib.n
        if top_k is not None and not 1 <= int(top_k) <= D:
            raise ValueError("screen_library: top_k %s not in [1, %d]" % (top_k, D))
        if shortlist is not None:
            if top_k is None:
                raise ValueError("screen_library: shortlist needs top_k (the dense (P, D) result has no shortlisted form)")
            if int(shortlist) < int(top_k):
                raise ValueError("screen_library: shortlist %d is smaller than top_k %d" % (int(shortlist), int(top_k)))
            M = self._check_shortlist("screen_library", lib, shortlist)
            self.model.eval()
            return self._screen_shortlisted(protein_batches, lib, pair_batch, int(top_k), M)
        self.model.eval()
        rows, vals, idxs = [], [], []
        for feat_p, llm_p in protein_batches:
            pcode = self.model.encode_proteins(feat_p, llm_p)
            Pn = pcode.n
            d_step = max(1, pair_batch // Pn)                  # whole drugs per chunk: a chunk is a (drugs, Pn) block
            best_v = best_i = None
            cols = []
            for d0 in range(0, D, d_step):
                d1 = min(D, d0 + d_step)
                di = torch.arange(d0, d1).repeat_interleave(Pn)     # drug-major
                pi = torch.arange(Pn).repeat(d1 - d0)
                score = self.model.score_library(pcode, lib, pi, di)
                prob = torch.sigmoid(score).squeeze(1) if self.n_class == 1 else torch.softmax(score, dim=1)[:, 1]
                prob = prob.view(d1 - d0, Pn).t()                   # (Pn, drugs d0 .. d1 - 1)
                if top_k is None:
                    cols.append(prob)
                    continue
                ids = torch.arange(d0, d1, device=prob.device).expand(Pn, -1)
                if best_v is not None:
                    prob, ids = torch.cat([best_v, prob], dim=1), torch.cat([best_i, ids], dim=1)
                best_v, sel = torch.topk(prob, min(int(top_k), prob.shape[1]), dim=1)
                best_i = torch.gather(ids, 1, sel)
            if top_k is None:
                rows.append(torch.cat(cols, dim=1))
            else:
                vals.append(best_v)
                idxs.append(best_i)
            del pcode
        self.check_device_flags()
        if top_k is None:
            return torch.cat(rows).contiguous() if rows else torch.zeros((0, D), dtype=torch.float32, device=self.device)
        if not vals:
            return (torch.zeros((0, int(top_k)), dtype=torch.float32, device=self.device),
                    torch.zeros((0, int(top_k)), dtype=torch.int64, device=self.device))
        return torch.cat(vals).contiguous(), torch.cat(idxs).contiguous()

    @torch.no_grad()
    def hit_maps(self, protein_batches, lib, indices, branch: str = "v", pair_batch: int = 64) -> torch.Tensor:
        """The PGCA attention maps of screening hits: for protein p and its j-th hit, drug indices[p, j] of the library (the
        (P, k) int64 indices of screen_library(top_k=k)), the softmax weights of `branch` that get_cross_attn_prob gives after an
        eval forward on that pair — which drug atoms / tokens each protein site attends to.  Returns (P, k, n_site, cols) fp32
        on the CPU, cols = the largest full key count among the hits (512 on the model's path).  The protein batches are
        streamed as in screen_library (the same ones, in the same order); the maps come straight from the cached codes
        (model.cross_attn_prob_library), pair_batch pairs at a time, each chunk copied to the host: device memory holds
        O(pair_batch) maps whatever P and k."""
        P, k, cols, outs = self._hit_stream("hit_maps", protein_batches, lib, indices, branch, pair_batch,
                                            lambda pcode, pi, di, cols: (self.model.cross_attn_prob_library(pcode, lib, pi, di, branch=branch, cols=cols),))
        if outs is None:
            return torch.zeros((0, k, 0, 0), dtype=torch.float32)
        return outs[0].view(P, k, outs[0].shape[1], cols)

    @torch.no_grad()
    def hit_profiles(self, protein_batches, lib, indices, branch: str = "v", pair_batch: int = 256) -> HitProfiles:
        """The hit profiles of screening hits: what hit_maps' maps reduce to, for every hit of a large screen (about 4 KB per
        hit where a map is 512 KB; no map is written anywhere).  For protein p and its j-th hit, drug indices[p, j]:
        key_mass[p, j, c] is the share of the protein's attention that drug key c receives (the map's mean over the sites;
        cols = the largest full key count among the hits, +0.0 behind a drug's own), site_peak[p, j, r] the largest probability
        in site r's row and site_key[p, j, r] the stored key of the drug that receives it.  Returns HitProfiles(key_mass
        (P, k, cols) fp32, site_peak (P, k, n_site) fp32, site_key (P, k, n_site) int32) on the CPU.  The protein batches are
        streamed and the arguments checked as in hit_maps; the profiles come from model.cross_attn_profile_library, pair_batch
        pairs per launch."""
        P, k, cols, outs = self._hit_stream("hit_profiles", protein_batches, lib, indices, branch, pair_batch,
                                            lambda pcode, pi, di, cols: self.model.cross_attn_profile_library(pcode, lib, pi, di, branch=branch, cols=cols))
        if outs is None:
            return HitProfiles(torch.zeros((0, k, 0), dtype=torch.float32), torch.zeros((0, k, 0), dtype=torch.float32),
                               torch.zeros((0, k, 0), dtype=torch.int32))
        return HitProfiles(*(o.view(P, k, o.shape[1]) for o in outs))

    def hit_attributions(self, protein_batches, lib, indices, pair_batch: int = 64) -> HitAttributions:
        """Gradient x code attributions of screening hits: what moves the score, where hit_profiles says where the attention
        looks.  For protein p and its j-th hit, drug indices[p, j]: logit[p, j] is the logit whose sigmoid screen_library
        reports; key_attr[branch][p, j, c] the share of it that gradient x code assigns to drug key c (one copy's value, in
        hit_profiles' key_mass columns: cols_b = the largest full key count among the hits in that branch, +0.0 behind a
        drug's own) and site_attr[branch][p, j, r] the share of protein site r.  The leaves are the cached codes at the pair
        stage, not the raw inputs; the values are signed.  Returns HitAttributions(logit (P, k) fp32, key_attr {branch:
        (P, k, cols_b)} fp32, site_attr {branch: (P, k, n_site)} fp32) on the CPU.  The protein batches are streamed and the
        arguments checked as in hit_profiles; every branch of a chunk of pair_batch pairs comes from ONE tail backward
        (model.attribute_library)."""
        names = sorted(lib.branches)

        def fetch(pcode, pi, di, cols):
            logit, per = self.model.attribute_library(pcode, lib, pi, di, cols=cols)
            return (logit,) + tuple(t for b in names for t in per[b])
        P, k, cols, outs = self._hit_stream("hit_attributions", protein_batches, lib, indices, names, pair_batch, fetch)
        if outs is None:
            z = lambda: {b: torch.zeros((0, k, 0), dtype=torch.float32) for b in names}
            return HitAttributions(torch.zeros((0, k), dtype=torch.float32), z(), z())
        shaped = [o.view(P, k, o.shape[1]) for o in outs[1:]]
        return HitAttributions(outs[0].view(P, k), {b: shaped[2 * i] for i, b in enumerate(names)},
                               {b: shaped[2 * i + 1] for i, b in enumerate(names)})

    def _hit_stream(self, who, protein_batches, lib, indices, branch, pair_batch, fetch):
        """What hit_maps, hit_profiles and hit_attributions share: the checks of their arguments, the streaming of the protein
        batches and the chunking of the hits.  fetch(pcode, pi, di, cols) gives a chunk's results as a tuple of device tensors
        whose first dimension is the pair; each is copied to the host behind the chunks before it.  branch: one branch (cols:
        an int), or a list of branches (cols: {branch: int}).  Returns (P, k, cols, the tuple of (P * k, ...) CPU tensors, or
        None where no protein came)."""
        if pair_batch < 1:
            raise ValueError("%s: pair_batch must be positive" % who)
        per_branch = not isinstance(branch, str)                # hit_attributions: every branch at once, cols = {branch: columns}
        for b in (branch if per_branch else (branch,)):
            if b not in lib.branches:
                raise ValueError("%s: unknown branch %r (the library has %s)" % (who, b, sorted(lib.branches)))
        idx = torch.as_tensor(indices, dtype=torch.int64).cpu()
        if idx.dim() != 2:
            raise ValueError("%s: indices must be (P, k), got %s" % (who, tuple(idx.shape),))
        P, k = idx.shape
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= lib.n):
            raise IndexError("%s: drug index out of range [0, %d)" % (who, lib.n))
        full = lambda b: int(lib.full_keys(b)[idx.reshape(-1)].max()) if idx.numel() else 0
        cols = {b: full(b) for b in branch} if per_branch else full(branch)
        self.model.eval()
        outs, p0 = None, 0
        for feat_p, llm_p in protein_batches:
            pcode = self.model.encode_proteins(feat_p, llm_p)
            Pn = pcode.n
            if p0 + Pn > P:
                raise ValueError("%s: indices has %d rows, the protein batches yield more proteins" % (who, P))
            pi = torch.arange(Pn).repeat_interleave(k)
            di = idx[p0:p0 + Pn].reshape(-1)
            for s in range(0, max(Pn * k, 1), pair_batch):          # (k == 0: one empty chunk gives the results' shapes)
                parts = fetch(pcode, pi[s:s + pair_batch], di[s:s + pair_batch], cols)
                if outs is None:
                    outs = tuple(torch.empty((P * k,) + tuple(t.shape[1:]), dtype=t.dtype) for t in parts)
                for o, t in zip(outs, parts):
                    o[p0 * k + s:p0 * k + s + t.shape[0]].copy_(t)
            p0 += Pn
            del pcode
        if p0 != P:
            raise ValueError("%s: indices has %d rows, the protein batches yielded %d proteins" % (who, P, p0))
        self.check_device_flags()
        return P, k, cols, outs

    def evaluate(self, batches) -> Dict[str, float]:
        """Metrics over the union of all ranks' samples (the reference's torchmetrics objects gather their states at
        epoch end, trainer.py:262-292; its logged loss is `sync_dist=True`): ranks may hold different numbers of samples."""
        p, y, loss_sum, n = self.predict(batches)
        p, y, loss_sum, n = gather_predictions(p, y, loss_sum, n, self.world)
        out = binary_metrics(p.cpu().numpy(), y.cpu().numpy())
        out["loss"] = float(loss_sum) / max(n, 1)
        return out

    def _epoch_losses(self, sums, steps) -> Dict[str, float]:
        return _epoch_loss_means(sums, steps, self.world, self.device)

    def fit(self, train_batches, val_batches, epochs: Optional[int] = None, on_epoch=None, checkpoint_dir=None,
            checkpoint_every: int = 1, resume: bool = False) -> Dict[str, object]:
        """The reference's run_experiment loop (trainer.py:131-135,150-163): one pass over `train_batches()` per epoch
        (a callable yielding (batch, meta) pairs), on_train_epoch_end, validation; the parameters with the best
        `val_ausum` (AUROC + AUPRC: ModelCheckpoint(monitor='val_ausum', mode='max')) are kept, training stops after
        patience = epochs / 4 epochs without improvement (EarlyStopping, min_delta 0), and the best parameters are
        reloaded before returning (trainer.py:134) — ready for evaluate(test_batches).
        With the weight EMA on, validation runs under ema_weights() (selection and early stopping judge the averaged weights),
        every history entry says so ("weights": "ema"), and the best snapshot holds the live arena, the shadow and the
        buffers: all three are reloaded.
        checkpoint_dir (None: nothing is written and the loop is exactly the one above): a directory, created if need be.
        After the validation and bookkeeping of every checkpoint_every-th epoch (and of the epoch early stopping ends on)
        `last.pt` is written there: a save_checkpoint whose `extra` carries the epoch number, `history`, the early-stopping
        count and the best snapshot (arena, buffers, shadow, epoch, ausum).  Whenever the best snapshot improves, `best.pt` is
        written: the parameters of that moment as a plain checkpoint (also a weight file for load_reference_checkpoint).
        resume=True with an existing `last.pt`: load it and go on with the next epoch, same patience arithmetic; the returned
        history is the whole run's.  Without a `last.pt` the run starts from scratch.  An eager run resumed this way leaves
        the bits of the uninterrupted run (INTEGRATION.md "Checkpoints and resuming")."""
        epochs = int(epochs or self.epochs)
        patience = max(int(epochs / 4), 1)
        best = {"ausum": -float("inf"), "epoch": 0, "arena": None, "buffers": None, "shadow": None}
        history, bad, first = [], 0, 1
        if checkpoint_dir is None and resume:
            raise ValueError("Trainer.fit(resume=True) needs a checkpoint_dir")
        if checkpoint_dir is not None:
            if int(checkpoint_every) < 1:
                raise ValueError("Trainer.fit: checkpoint_every must be a positive number of epochs")
            os.makedirs(checkpoint_dir, exist_ok=True)
            last_path, best_path = os.path.join(checkpoint_dir, "last.pt"), os.path.join(checkpoint_dir, "best.pt")
            if resume and os.path.exists(last_path):
                ex = self.load_checkpoint(last_path).get("fit")
                if ex is None:
                    raise RuntimeError("Trainer.fit(resume=True): %s was not written by fit" % last_path)
                history, bad, first = [dict(h) for h in ex["history"]], int(ex["bad"]), int(ex["epoch"]) + 1
                to_dev = lambda t: None if t is None else t.to(self.device)      # noqa: E731
                best = {"ausum": float(ex["best"]["ausum"]), "epoch": int(ex["best"]["epoch"]), "arena": to_dev(ex["best"]["arena"]),
                        "buffers": None if ex["best"]["buffers"] is None else [to_dev(b) for b in ex["best"]["buffers"]],
                        "shadow": to_dev(ex["best"]["shadow"])}
                if bad >= patience:                      # (the saved run had stopped early already)
                    first = epochs + 1
        for ep in range(first, epochs + 1):
            sums: Dict[str, torch.Tensor] = {}
            steps = 0
            guard_before = self.grad_guard.counters.clone() if self.grad_guard is not None else None
            for batch, meta in train_batches():
                out = self.training_step(batch, meta=meta, cur_epoch=ep)
                for k, v in out.items():                 # device-side running sums: no host synchronisation per step
                    if k == "grad_norm":
                        continue
                    sums[k] = sums[k] + v.detach().float() if k in sums else v.detach().float().clone()
                steps += 1
            self.on_train_epoch_end(ep)
            if self.ema is not None:
                with self.ema_weights():
                    val = self.evaluate(val_batches() if callable(val_batches) else val_batches)
                val["weights"] = "ema"
            else:
                val = self.evaluate(val_batches() if callable(val_batches) else val_batches)
            val.update(self._epoch_losses(sums, steps))
            if guard_before is not None:                 # (the epoch boundary has synchronised already: check_device_flags)
                skipped, clipped = (self.grad_guard.counters - guard_before).tolist()
                val.update(grad_skipped=int(skipped), grad_clipped=int(clipped))
            history.append(val)
            if on_epoch is not None:
                on_epoch(ep, val)
            score = val["ausum"]
            if score == score and score > best["ausum"]:
                best.update(ausum=score, epoch=ep, arena=self.flat.arena.clone(),
                            buffers=[b.detach().clone() for b in self.model.buffers()],
                            shadow=self.ema.shadow.clone() if self.ema is not None else None)
                bad = 0
                if checkpoint_dir is not None:
                    self.save_checkpoint(best_path, extra={"epoch": ep, "ausum": float(score)})
            else:
                bad += 1
            if checkpoint_dir is not None and (ep % int(checkpoint_every) == 0 or bad >= patience):
                self.save_checkpoint(last_path, extra={"fit": {"epoch": ep, "history": history, "bad": bad, "best": best}})
            if bad >= patience:
                break
        if best["arena"] is not None:                                    # reload the best checkpoint (trainer.py:134)
            with torch.no_grad():
                self.flat.arena.copy_(best["arena"])
                if best["shadow"] is not None:
                    self.ema.shadow.copy_(best["shadow"])
                for b, src in zip(self.model.buffers(), best["buffers"]):
                    b.copy_(src)
            Fn.bump_param_epoch()
        return {"best_epoch": best["epoch"], "best_val_ausum": best["ausum"], "epochs_run": len(history), "history": history}


def _epoch_loss_means(sums: Dict[str, torch.Tensor], steps: int, world: int, device) -> Dict[str, float]:
    """Epoch means of the step losses over steps AND ranks — what the reference logs with `on_epoch=True, sync_dist=True`
    (trainer.py:201,208,222,231): train_loss (cls), ssl_loss, cm_loss (weighted, as added to the total) and all_loss (their
    sum on the steps that had them).  One all-reduce of a 4-vector of sums + a step count per epoch."""
    keys = ("cls", "ssl", "cm")
    vec = torch.zeros(len(keys) + 1, dtype=torch.float64, device=device)
    for i, k in enumerate(keys):
        if k in sums:
            vec[i] = sums[k].double()
    vec[len(keys)] = float(steps)
    if world > 1:
        dist.all_reduce(vec, op=dist.ReduceOp.SUM)
    v = vec.tolist()
    n = max(v[len(keys)], 1.0)
    out = {"train_loss": v[0] / n, "ssl_loss": v[1] / n, "cm_loss": v[2] / n}
    out["all_loss"] = out["train_loss"] + out["ssl_loss"] + out["cm_loss"]
    return out


def gather_predictions(p: torch.Tensor, y: torch.Tensor, loss_sum: torch.Tensor, n: int, world: int):
    """All ranks' predictions / labels / loss sums, for shards of DIFFERENT sizes: counts are gathered first, every
    shard is padded to the largest and trimmed after the gather (equal-size all_gather would hang or mis-slice)."""
    if world <= 1:
        return p, y, loss_sum, n
    dev = p.device
    counts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([n], dtype=torch.int64, device=dev))
    counts = [int(c) for c in counts]
    m = max(max(counts), 1)
    buf = torch.zeros((2, m), dtype=torch.float32, device=dev)
    buf[0, :n], buf[1, :n] = p.float(), y.float()
    bufs = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(bufs, buf)
    ls = loss_sum.detach().double().reshape(1).clone()
    dist.all_reduce(ls, op=dist.ReduceOp.SUM)
    p = torch.cat([b[0, :c] for b, c in zip(bufs, counts)])
    y = torch.cat([b[1, :c] for b, c in zip(bufs, counts)])
    return p, y, ls[0], sum(counts)


def binary_metrics(p, y) -> Dict[str, float]:
    """AUROC / AUPRC (sklearn = torchmetrics' exact, threshold-free definitions), their sum (the reference's BinaryAUSum,
    trainer.py:17-37) and the thresholded metrics at 0.5 (trainer.py:109-119)."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    auroc = float(roc_auc_score(y, p)) if len(set(y.tolist())) > 1 else float("nan")
    auprc = float(average_precision_score(y, p)) if y.sum() > 0 else float("nan")
    yhat = (p >= 0.5).astype("float32")
    tp, tn = float(((yhat == 1) & (y == 1)).sum()), float(((yhat == 0) & (y == 0)).sum())
    fp, fn = float(((yhat == 1) & (y == 0)).sum()), float(((yhat == 0) & (y == 1)).sum())
    prec = tp / max(tp + fp, 1.0)
    rec = tp / max(tp + fn, 1.0)
    return {"auroc": auroc, "auprc": auprc, "ausum": auroc + auprc, "acc": (tp + tn) / max(len(y), 1), "sn": rec,
            "sp": tn / max(tn + fp, 1.0), "pr": prec, "f1": 2 * prec * rec / max(prec + rec, 1e-12)}
