"""The imbalance-aware classification loss of the classifier step: weighted / focal binary cross entropy on the classifier's
logits as one HIP kernel pair (csrc/cls_loss.hip, dl_cls_loss_fwd / dl_cls_loss_bwd).

For row i with z = score[i, 0] (one output) or score[i, 1] - score[i, 0] (two), y = labels[i] in [0, 1], w = weights[i] (1 without
weights), p = sigmoid(z):

    d = |y - p|,  m = d^gamma (gamma = 0: exactly 1),
    l = -w m [pos_weight y log p + neg_weight (1 - y) log(1 - p)],     loss = sum l / den,  den = N, or sum w with weights

  * ClsLoss(pos_weight=pw)            F.binary_cross_entropy_with_logits(pos_weight=pw)
  * ClsLoss.focal(alpha, gamma)       the reference's FocalLossV1(alpha, gamma, reduction='mean') (dead code there: SURVEY row 16)
  * ClsLoss() on two outputs          the cross entropy of the default step

The gradient is the full derivative (the focal factor is differentiated, as the reference's autograd does).  A non-finite
score, a label outside [0, 1] and a negative or non-finite weight poison their sample (loss NaN, that sample's gradient NaN)
without a device assert; the last two also raise FLAG_CLS_LABEL in the loss's device guard word (ops.cls_loss_flags), which
ops.check_guard_flags and the trainer's polling report.  Trainer(cls_loss=ClsLoss(...)) puts it into the step; per-sample
weights travel in meta as "Weight" (meta_weights)."""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import torch

from . import ops


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError("ClsLoss: %s must be a number (got %r)" % (name, v))
    return float(v)


@dataclasses.dataclass(frozen=True)
class ClsLoss:
    """What the classifier step minimises (immutable).  pos_weight / neg_weight: finite, >= 0, not both 0; gamma: 0 (no focal
    term) or in [1, 8].  Anything else raises ValueError."""
    pos_weight: float = 1.0
    neg_weight: float = 1.0
    gamma: float = 0.0

    def __post_init__(self):
        for name in ("pos_weight", "neg_weight", "gamma"):
            object.__setattr__(self, name, _number(name, getattr(self, name)))
        for name in ("pos_weight", "neg_weight"):
            v = getattr(self, name)
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError("ClsLoss: %s = %r must be finite and >= 0" % (name, v))
        if self.pos_weight == 0.0 and self.neg_weight == 0.0:
            raise ValueError("ClsLoss: pos_weight and neg_weight are both 0")
        if not (self.gamma == 0.0 or 1.0 <= self.gamma <= 8.0):
            raise ValueError("ClsLoss: gamma = %r must be 0 or in [1, 8]" % (self.gamma,))

    @classmethod
    def focal(cls, alpha: float = 0.25, gamma: float = 2.0) -> "ClsLoss":
        """The focal loss: pos_weight = alpha, neg_weight = 1 - alpha, alpha in [0, 1]."""
        a = _number("alpha", alpha)
        if not 0.0 <= a <= 1.0:
            raise ValueError("ClsLoss.focal: alpha = %r must lie in [0, 1]" % (alpha,))
        return cls(pos_weight=a, neg_weight=1.0 - a, gamma=gamma)


class ClsLossFn(torch.autograd.Function):
    """(loss, probs) = dl_cls_loss_fwd(score (N, 1 | 2) fp32 / bf16, labels fp32 (N,), weights fp32 (N,) | None); follows
    functional.CrossEntropyRowsFn.  probs = sigmoid(z) (fp32, not differentiable); the backward recomputes from z."""

    @staticmethod
    def forward(ctx, score, labels, weights, a_pos, a_neg, gamma):
        score = score if score.stride(-1) == 1 else score.contiguous()
        out2, probs = ops.cls_loss_fwd(score, labels, weights, a_pos, a_neg, gamma)
        ctx.save_for_backward(score, labels, out2) if weights is None else ctx.save_for_backward(score, labels, out2, weights)
        ctx.cfg = (a_pos, a_neg, gamma)
        ctx.mark_non_differentiable(probs)
        return out2[0], probs

    @staticmethod
    def backward(ctx, g, _gprobs):
        score, labels, out2, *w = ctx.saved_tensors
        a_pos, a_neg, gamma = ctx.cfg
        d = ops.cls_loss_bwd(score, labels, w[0] if w else None, a_pos, a_neg, gamma, out2, g.float().contiguous())
        return d, None, None, None, None, None


def classification_loss(score, labels, spec: ClsLoss, weights: Optional[torch.Tensor] = None):
    """(n, loss) as basic_model.binary_cross_entropy / cross_entropy_logits return them: n (N,) fp32 the probability of the
    positive class, loss a device scalar.  score (N, 1) or (N, 2) in the dtype the classifier produced (no fp32 copy), labels
    (N,) or (N, 1), weights (N,) or None."""
    if not isinstance(spec, ClsLoss):
        raise TypeError("classification_loss: spec must be a ClsLoss (got %r)" % (spec,))
    y = labels.reshape(-1).float().contiguous()
    w = None if weights is None else weights.reshape(-1).float().contiguous()
    loss, probs = ClsLossFn.apply(score, y, w, spec.pos_weight, spec.neg_weight, spec.gamma)
    return probs, loss


def meta_weights(meta) -> Optional[torch.Tensor]:
    """The per-sample weights of a step from its meta records: a (B,) fp32 host tensor when EVERY entry has a "Weight" key,
    None when none has (or there is no meta); only some: ValueError."""
    if not meta:
        return None
    have = sum(1 for m_ in meta if "Weight" in m_)
    if have == 0:
        return None
    if have != len(meta):
        raise ValueError("meta: %d of %d entries carry a 'Weight'; per-sample weights need all of them or none" % (have, len(meta)))
    return torch.tensor([float(m_["Weight"]) for m_ in meta], dtype=torch.float32)
