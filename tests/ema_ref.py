"""fp64 restatement of the weight EMA (csrc/optim.hip; contract in include/druglamp_hip.h; trainer.WeightEMA): the recurrence
e + w (p - e) with the weight the C ABI receives (w rounded to fp32), the weight schedule, the element-wise bound of the GPU
tests and an fp32 emulation of the kernel's arithmetic.  numpy / torch on the CPU.
"""
import numpy as np
import torch

WEIGHTS = [0.0, 1e-4, 1e-3, 0.1, 0.5, 0.9, 1.0]


def f32(w):
    """w rounded to fp32, as a Python float: what a c_float argument holds."""
    return float(np.float32(w))


def weight(decay, t, warmup=False):
    """The weight of the update that follows t earlier ones, as the kernel receives it: 1 - decay, or with warmup
    1 - min(decay, (1 + t) / (10 + t)), rounded to fp32."""
    d = min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)
    return f32(1.0 - d)


def _f64(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(np.float64)


def update(e, p, w):
    """One update in fp64: e + w (p - e), w rounded to fp32 first.  Non-finite operands propagate as the arithmetic says."""
    e, p = _f64(e), _f64(p)
    with np.errstate(invalid="ignore", over="ignore"):
        return e + f32(w) * (p - e)


def run(e0, params, decay, warmup=False):
    """The shadow after an update towards each of `params` in turn, from e0 (fp64)."""
    e = _f64(e0)
    for t, p in enumerate(params):
        e = update(e, p, weight(decay, t, warmup))
    return e


def bound(e, p):
    """The element-wise bound of ONE kernel update against `update`: 2^-22 max(|e|, |p|).  Derivation: the difference p - e is
    rounded once (relative 2^-24 of |p - e| <= 2 max), scaled by w <= 1: 2 * 2^-24 max; the fma rounds once, and its result
    lies between e and p for w in [0, 1]: 2^-24 max.  Together at most 3 * 2^-24 max < 2^-22 max."""
    return 2.0 ** -22 * np.maximum(np.abs(_f64(e)), np.abs(_f64(p)))


def kernel_f32(e, p, w, fma=True):
    """The kernel's arithmetic emulated in fp32 numpy: d = fl(p - e); fl(w d + e) in one rounding (fma: the exact product of
    two fp32 values in fp64, added and rounded to fp64 and then to fp32 — one double rounding away from a true fma) or two
    (fma=False); a zero difference keeps e."""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    w32 = np.float32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - e
        if fma:
            r = (np.float64(w32) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)
        else:
            r = (w32 * d).astype(np.float32) + e
    return np.where(d == 0, e, r)


def pairs(n, seed):
    """(ema, param) fp32 arrays of n elements: |ema| log-uniform in [1e-3, 10], param = ema +- a difference log-uniform in
    [1e-6, 10], random signs."""
    g = np.random.default_rng(seed)
    e = np.exp(g.uniform(np.log(1e-3), np.log(10.0), n)) * g.choice([-1.0, 1.0], n)
    d = np.exp(g.uniform(np.log(1e-6), np.log(10.0), n)) * g.choice([-1.0, 1.0], n)
    e32 = e.astype(np.float32)
    return e32, (e32.astype(np.float64) + d).astype(np.float32)
