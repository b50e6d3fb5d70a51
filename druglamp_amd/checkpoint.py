"""Trainer checkpoints: the file format and its checks (Trainer.save_checkpoint / load_checkpoint / fit(checkpoint_dir=...)).

Pure Python and torch: neither the library nor ops is imported here; what lives on the device is collected and written back
by the trainer.  A checkpoint is ONE torch.save of a dict of tensors (on the CPU), plain scalars, strings, lists and dicts,
so it reads back with torch.load(..., weights_only=True):

    "format"      1
    "state_dict"  model.state_dict() under the reference's key names: every parameter and buffer, the lazily created SimSiam
                  projectors once they exist — load_reference_checkpoint(model, path) accepts the file as it stands
    "trainer"     what a step reads or writes besides the model (optimiser moments and step counts, schedulers, EMA, guard
                  counters, parameter-group values, random state, ...): see Trainer.save_checkpoint
    "signature"   what the file is valid for: compared field by field before a load writes anything
    "extra"       the caller's plain data (fit keeps its epoch, history and best snapshot here)

write() is atomic: the bytes go to a temporary name in the target's directory and os.replace moves them onto the target, so a
writer that dies midway leaves an existing file as it was."""
from __future__ import annotations

import os
import tempfile
from typing import List, Optional, Tuple

import torch

FORMAT = 1
KEYS = ("format", "state_dict", "trainer", "signature", "extra")

# signature fields whose difference refuses a load, in the order they are compared; every other field only warns
MUST_MATCH = ("model", "params", "world", "optimisers", "ema.on", "guard.on", "param_groups")
WARN_ONLY = ("compute_dtype", "ema.decay", "ema.warmup", "guard.max_grad_norm", "guard.skip_nonfinite", "freeze_bn", "cls_loss",
             "graph_steps", "fixed_caps")


def _plain(x, where: str = "extra"):
    """x rebuilt from what weights_only=True reads back: tensors (detached, on the CPU), None, bool, int, float, str, and
    lists / dicts of those (tuples become lists; dict keys must be str or int).  Anything else is a TypeError that says where."""
    if torch.is_tensor(x):
        return x.detach().cpu()
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, (list, tuple)):
        return [_plain(v, "%s[%d]" % (where, i)) for i, v in enumerate(x)]
    if isinstance(x, dict):
        for k in x:
            if not isinstance(k, (str, int)) or isinstance(k, bool):
                raise TypeError("checkpoint: %s has the key %r; keys must be str or int" % (where, k))
        return {k: _plain(v, "%s[%r]" % (where, k)) for k, v in x.items()}
    raise TypeError("checkpoint: %s holds a %s; only tensors, plain scalars, strings, lists and dicts can be saved" % (where, type(x).__name__))


def pack(state_dict, trainer_state: dict, signature: dict, extra: Optional[dict] = None) -> dict:
    """The dict that write() saves."""
    if extra is not None and not isinstance(extra, dict):
        raise TypeError("checkpoint: extra must be a dict or None (got %s)" % type(extra).__name__)
    return {"format": FORMAT,
            "state_dict": {str(k): v.detach().cpu() for k, v in state_dict.items()},
            "trainer": _plain(trainer_state, "trainer"),
            "signature": _plain(signature, "signature"),
            "extra": _plain(extra if extra is not None else {}, "extra")}


def write(blob: dict, path) -> None:
    """torch.save(blob) to a temporary file beside `path`, then os.replace onto it.  On any failure the temporary file is
    removed and an existing `path` keeps its bytes."""
    path = os.fspath(path)
    folder = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=folder)
    try:
        with os.fdopen(fd, "wb") as f:
            torch.save(blob, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def read(path) -> dict:
    """The dict of a checkpoint file (weights_only=True, tensors on the CPU).  RuntimeError for a file that cannot be read (a
    truncated one, say), that is no checkpoint of this package, or whose "format" this loader does not know."""
    try:
        blob = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:
        raise RuntimeError("checkpoint: %s cannot be read (%s: %s)" % (path, type(e).__name__, str(e).splitlines()[0] if str(e) else "")) from e
    if not isinstance(blob, dict) or "format" not in blob:
        raise RuntimeError("checkpoint: %s is not a trainer checkpoint (no \"format\" entry)" % (path,))
    if blob["format"] != FORMAT:
        raise RuntimeError("checkpoint: %s has format %r; this loader knows format %d" % (path, blob["format"], FORMAT))
    missing = [k for k in KEYS if k not in blob]
    if missing:
        raise RuntimeError("checkpoint: %s lacks the entries %s" % (path, ", ".join(missing)))
    return blob


def _field(sig: dict, name: str):
    v = sig
    for part in name.split("."):
        v = v.get(part) if isinstance(v, dict) else None
    return v


def _first_list_difference(what: str, saved, now, item: str) -> str:
    for i, (a, b) in enumerate(zip(saved, now)):
        if a != b:
            return "%s: %s %d is %r in the file and %r here" % (what, item, i, a, b)
    return "%s: the file has %d %ss, the trainer %d" % (what, len(saved), item, len(now))


def _params_difference(saved, now) -> str:
    """The first differing parameter of two [[name, shape, arena offset], ...] lists, in words."""
    for i, (a, b) in enumerate(zip(saved, now)):
        if list(a) == list(b):
            continue
        if a[0] != b[0]:
            return "parameter %d is named %r in the file and %r here" % (i, a[0], b[0])
        if list(a[1]) != list(b[1]):
            return "parameter %r has shape %s in the file and %s here" % (a[0], tuple(a[1]), tuple(b[1]))
        return "parameter %r sits at arena offset %s in the file and %s here" % (a[0], a[2], b[2])
    return "the file has %d parameters, the trainer %d" % (len(saved), len(now))


def _norm(v):
    """Tuples and lists compare equal (a signature that went through a file holds lists)."""
    if isinstance(v, (list, tuple)):
        return [_norm(x) for x in v]
    if isinstance(v, dict):
        return {k: _norm(x) for k, x in v.items()}
    return v


def compare_signatures(saved: dict, now: dict) -> Tuple[Optional[str], List[str]]:
    """(the first difference among the MUST_MATCH fields in words, or None; one line per differing WARN_ONLY field)."""
    error = None
    for name in MUST_MATCH:
        a, b = _norm(_field(saved, name)), _norm(_field(now, name))
        if a == b:
            continue
        if name == "params" and isinstance(a, list) and isinstance(b, list):
            error = _params_difference(a, b)
        elif name == "param_groups" and isinstance(a, list) and isinstance(b, list):
            error = _first_list_difference("parameter-group assignment", a, b, "entry")
        elif name == "param_groups":
            error = "parameter groups are %s in the file and %s here" % ("off" if a is None else "on", "off" if b is None else "on")
        elif name == "model":
            error = "the file holds a %s, the trainer a %s" % (a, b)
        elif name == "world":
            error = "world size is %r in the file and %r here" % (a, b)
        elif name in ("ema.on", "guard.on"):
            what = "weight EMA" if name == "ema.on" else "gradient guard"
            error = "the %s is %s in the file and %s here" % (what, "on" if a else "off", "on" if b else "off")
        else:
            error = "%s is %r in the file and %r here" % (name, a, b)
        break
    notes = []
    for name in WARN_ONLY:
        a, b = _norm(_field(saved, name)), _norm(_field(now, name))
        if a != b:
            notes.append("%s is %r in the file and %r here" % (name, a, b))
    return error, notes


def validate(blob: dict, signature: dict, what: str = "checkpoint") -> List[str]:
    """RuntimeError naming the first difference when blob["signature"] does not fit `signature`; returns the warning lines."""
    error, notes = compare_signatures(blob["signature"], signature)
    if error is not None:
        raise RuntimeError("%s: the file does not fit this trainer: %s" % (what, error))
    return notes


def check_tensor(what: str, t, shape, dtype) -> None:
    """RuntimeError unless t is a tensor of this shape and dtype."""
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
        got = "%s %s" % (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__
        raise RuntimeError("checkpoint: %s is %s; expected %s %s" % (what, got, tuple(shape), dtype))
