"""Tensor-level wrappers over the C ABI (druglamp_amd/_lib.py) and the autograd Functions built on
them.  torch is used for device memory, streams and autograd plumbing only: every arithmetic op on
the hot path below is a libdruglamp_hip entry point.  There is no CPU path here — tensors must live
on a HIP device and the shared library must be present.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from typing import Optional

import torch

from . import _lib
from ._lib import (DL_BF16, DL_F32, AttnBwdArgs, AttnFwdArgs, AttnProbsArgs, GemmArgs, PgcaPairsArgs, PgcaPairsAttrArgs, PgcaPairsProbsArgs,
                   PgcaPairsProfileArgs, PgcaPairsRaggedArgs, PgcaPairsRaggedAttrArgs, PgcaPairsRaggedProbsArgs, PgcaPairsRaggedProfileArgs,
                   check)

_DT = {torch.float32: DL_F32, torch.bfloat16: DL_BF16}


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError("druglamp_amd: unsupported dtype %s (float32 / bfloat16 only)" % t.dtype)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """The current torch stream's hipStream_t.  torch.cuda.current_stream() builds a Stream object through three
    Python layers (9 us, ~260 times per step); the raw getter is the same handle in well under a microsecond."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("druglamp_amd: the HIP hot path needs device tensors (got a %s tensor); "
                               "there is no CPU fallback" % t.device)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


class _Workspace:
    """One growing scratch buffer per device; all launches that use it are stream-ordered."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes: int, device) -> torch.Tensor:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            # a captured launch must not point into the shared buffer: that buffer is REPLACED (and the old one freed) the
            # first time an eager call needs more room, and a later replay would write through the stale address.  Scratch
            # taken during capture comes from the graph's own pool and stays reserved for as long as the graph lives.
            return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        # one buffer per (device, stream): launches that share it are stream-ordered; branches of the forward that run on
        # side streams (DL_BRANCH_STREAMS) get their own
        key = (device.type, device.index, _stream() if device.type == "cuda" else 0)
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        return buf


_ws = _Workspace()
_ws2 = _Workspace()  # second buffer so that two scratch users can be live inside one op


# ------------------------------------------------------------------------------------------------
# raw ops
# ------------------------------------------------------------------------------------------------
# Sub-family tag of the dl_gemm launches issued inside a `with prof_tag(T):` block (dl_gemm_args.prof_tag; timing hooks
# only).  Weight-gradient products outside the ProteinCNN are tagged TAG_WGRAD whatever the block says.
_prof_tag = 0


class prof_tag:
    __slots__ = ("tag", "prev")

    def __init__(self, tag: int):
        self.tag = tag

    def __enter__(self):
        global _prof_tag
        self.prev = _prof_tag
        _prof_tag = self.tag
        return self

    def __exit__(self, *exc):
        global _prof_tag
        _prof_tag = self.prev
        return False


def _gemm_args(x: torch.Tensor, w: torch.Tensor, *, M: int, N: int, K: int, x_kslow=False, w_kslow=False,
               ldx: Optional[int] = None, ldw: Optional[int] = None, bias=None, residual=None, res_row_mod=0,
               res_before_dropout=False, act=0, pre_out=None, dact_pre=None, dropout_p=0.0, seed=0, out=None,
               out_dtype=None, accumulate=False, split_k=-1, x_colsum=None, algo=0):
    """The dl_gemm_args block of one product (and its output tensor)."""
    _need_gpu(x, w)
    out_dtype = out_dtype or x.dtype
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=x.device)
    a = GemmArgs()
    a.X, a.W, a.C = x.data_ptr(), w.data_ptr(), out.data_ptr()
    a.ldx = ldx if ldx is not None else (M if x_kslow else K)
    a.ldw = ldw if ldw is not None else (N if w_kslow else K)
    a.ldc = out.stride(0) if out.dim() == 2 else N
    a.x_kslow, a.w_kslow = int(x_kslow), int(w_kslow)
    a.M, a.N, a.K = M, N, K
    a.in_dtype, a.out_dtype = _dt(x), _dt(out)
    a.bias = _ptr(bias)
    a.residual = _ptr(residual)
    a.ldr = N if residual is None else residual.stride(-2)
    a.res_row_mod = res_row_mod
    a.res_before_dropout = int(res_before_dropout)
    a.act = act
    a.pre_out = _ptr(pre_out)
    a.ldp = N
    a.dact_pre = _ptr(dact_pre)
    a.lddp = N
    a.dropout_p = float(dropout_p)
    a.dropout_seed = int(seed)
    a.accumulate = int(accumulate)
    a.split_k = split_k
    a.x_colsum = _ptr(x_colsum)
    a.dropout_seed_offset = _seed_offset_ptr(x.device) if dropout_p > 0 else None
    a.algo = algo
    a.tile_tickets = _tickets_ptr(x.device)
    a.prof_tag = _lib.TAG_WGRAD if (x_kslow and w_kslow and _prof_tag != _lib.TAG_CONV) else _prof_tag
    return a, out


def gemm(x: torch.Tensor, w: torch.Tensor, **kw) -> torch.Tensor:
    """C[M,N] = epilogue(sum_k X[m,k] W[n,k]); see include/druglamp_hip.h (dl_gemm).  Keywords: _gemm_args."""
    a, out = _gemm_args(x, w, **kw)
    accumulate, x_colsum = kw.get("accumulate", False), kw.get("x_colsum")
    if (_wgroup is not None and a.x_kslow and a.w_kslow and a.split_k == 0 and not accumulate
            and (a.K <= group_wgrad_max_k or a.M * a.N < group_wgrad_small_mn)
            and x.dtype == torch.bfloat16 and out.dtype == torch.float32 and a.bias is None and a.residual is None and not a.act):
        _wgroup.append((a, out, x_colsum, x, w))         # leaves with the block's other weight gradients (flush_wgrads)
        return out
    _gemm_launch(a, out, x, accumulate, x_colsum)
    return out


def _gemm_launch(a, out, x, accumulate, x_colsum) -> None:
    L = _lib.lib()
    if accumulate and (_pending or _wgroup):
        flush_reductions()                  # an accumulating product must see every earlier (queued) write to its output
    nbytes = L.dl_gemm_workspace_bytes(C.byref(a))
    item = None
    if nbytes:
        if _pending is not None and not accumulate:
            # inside deferred_reductions(): the slabs get a buffer of their own (it has to outlive the batched launch) and
            # the reduction is queued instead of launched
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            item = _lib.ReduceItem()
            a.deferred = C.pointer(item)
        else:
            ws = _ws.get(nbytes, x.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    check(L.dl_gemm(C.byref(a), _stream()), "dl_gemm")
    if item is not None and item.kind != 0:
        _pending.append((item, ws, out, x_colsum))


# Grouped weight gradients (dl_gemm_group, round 3).  Inside deferred_reductions() — a block's backward — the weight-gradient
# products (bf16, both operands K-slow, f32 output, at most group_wgrad_max_k rows) are not launched one by one: they queue
# up and leave as ONE launch when the block ends (16 per launch), followed by the block's one batched reduction.  At 32-64
# pairs per GPU each of them alone is a few tiles over 8192-16384 rows behind a 16- to 32-way split; together they fill the
# chip with 1-4 slabs each.  The rule of deferred_reductions() covers it: nothing inside the block reads these outputs,
# and their operands (saved activations, fresh gradient tensors) are not written again before the block ends.
# Measured (bench.py, same box, off -> on): batch 32 4.71 -> 4.23 ms, 64 6.22 -> 5.75, 128 9.32 -> 8.77, 256 15.53 -> 15.0.
group_wgrad_max_k = int(os.environ.get("DL_GROUP_WGRAD_MAX_K", "65536"))         # 0 (and small_mn 0): off
group_wgrad_small_mn = int(os.environ.get("DL_GROUP_WGRAD_SMALL_MN", "655360"))  # products with fewer outputs are grouped at any K
group_wgrad_min_n = 2          # a single queued product takes its usual dl_gemm path
_wgroup = None


def flush_wgrads() -> None:
    if not _wgroup:
        return
    L = _lib.lib()
    todo = list(_wgroup)
    del _wgroup[:]
    for i in range(0, len(todo), _lib.GEMM_GROUP_MAX):
        part = todo[i:i + _lib.GEMM_GROUP_MAX]
        n = len(part)
        arr = (GemmArgs * n)(*[t[0] for t in part])
        splits = (C.c_int32 * n)()
        if n < group_wgrad_min_n or L.dl_gemm_group_plan(arr, n, splits) != 0:
            for a, out, x_colsum, x, _w in part:             # not a group the library takes: one by one, as before
                _gemm_launch(a, out, x, False, x_colsum)
            continue
        keep = []
        for k, (a, out, x_colsum, x, _w) in enumerate(part):
            nbytes = int(splits[k]) * a.M * (a.N + (1 if x_colsum is not None else 0)) * 4
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            item = _lib.ReduceItem()
            arr[k].workspace, arr[k].workspace_bytes = ws.data_ptr(), nbytes
            arr[k].deferred = C.pointer(item)
            keep.append((item, ws, out, x_colsum))
        check(L.dl_gemm_group(arr, n, _stream()), "dl_gemm_group")
        _pending.extend(keep)


def gemm_pair(xs, ws, **kw):
    """Two products of one shape / layout / epilogue — the two streams of a paired block — through dl_gemm_pair: ONE launch
    when both are on the 128-tile path without split-K, two otherwise; bit-identical to two gemm() calls.  xs, ws: the two
    operand pairs; every other keyword of gemm() is either one value for both or a 2-tuple / 2-list (one per problem)."""
    L = _lib.lib()
    per = [{k: (v[i] if isinstance(v, (tuple, list)) else v) for k, v in kw.items()} for i in range(2)]
    (a0, o0), (a1, o1) = _gemm_args(xs[0], ws[0], **per[0]), _gemm_args(xs[1], ws[1], **per[1])
    if L.dl_gemm_workspace_bytes(C.byref(a0)) or L.dl_gemm_workspace_bytes(C.byref(a1)):
        return gemm(xs[0], ws[0], **per[0]), gemm(xs[1], ws[1], **per[1])      # split-K shapes: the plain path (own workspaces)
    check(L.dl_gemm_pair(C.byref(a0), C.byref(a1), _stream()), "dl_gemm_pair")
    return o0, o1


# Deferred second-stage reductions (dl_reduce_item / dl_reduce_batch): inside `with deferred_reductions():` every split-K
# GEMM (and LayerNorm backward) only writes its partial results; the reductions leave together, DL_REDUCE_BATCH_MAX per
# launch, when the block ends.  NOTHING inside the block may read an output of those calls — the backward passes that use
# it only hand the gradients back to autograd.
_pending = None


@contextlib.contextmanager
def deferred_reductions():
    global _pending, _wgroup
    if _pending is not None:            # nested: the outermost block flushes
        yield
        return
    _pending = []
    _wgroup = [] if (group_wgrad_max_k > 0 or group_wgrad_small_mn > 0) else None
    try:
        yield
    finally:
        try:
            flush_reductions()
        finally:
            _pending = None
            _wgroup = None


def flush_reductions() -> None:
    """Launch what is queued (keeps the deferred mode, if any, active): the grouped weight gradients first — their slabs
    are part of the batched reduction."""
    flush_wgrads()
    if not _pending:
        return
    L = _lib.lib()
    todo = list(_pending)
    del _pending[:]
    for i in range(0, len(todo), _lib.REDUCE_BATCH_MAX):
        part = todo[i:i + _lib.REDUCE_BATCH_MAX]
        arr = (_lib.ReduceItem * len(part))(*[t[0] for t in part])
        check(L.dl_reduce_batch(arr, len(part), _stream()), "dl_reduce_batch")


# Dynamic tile hand-out of the persistent large-tile GEMM (dl_gemm_args.tile_tickets): on while gradient buckets are being
# all-reduced DURING backward (trainer.GradOverlap), when RCCL channel workgroups occupy some CUs for a while — a CU that
# starts late then simply takes fewer tiles.  Two int32 per device, zero between launches (the kernel restores them).
# ONE pair of words per device, not per stream: the last workgroup of a launch zeroes them for the next launch ON ITS
# STREAM, so they are valid only for ticketed launches that are ordered on one stream — two such launches running at once
# on different streams would draw from one counter and each would skip tiles.  The switch is process-global; the models
# therefore keep their forward on one stream while it is on (dynamic_tiles_enabled(): DrugLAMP._forward).
_tickets = {}
_tickets_on = False


def dynamic_tiles(on: bool) -> None:
    global _tickets_on
    _tickets_on = bool(on)


def dynamic_tiles_enabled() -> bool:
    """True while the large-tile GEMMs draw their tiles from the per-device ticket words (one stream only, see above)."""
    return _tickets_on


def reset_tickets() -> None:
    """Zero the ticket words (Trainer construction; after a failed launch they could hold a stale count and later
    ticketed GEMMs would skip tiles — ADVICE round 2)."""
    for t in _tickets.values():
        t.zero_()


def _tickets_ptr(device):
    if not _tickets_on:
        return None
    key = (device.type, device.index)
    t = _tickets.get(key)
    if t is None:
        t = _tickets[key] = torch.zeros(2, dtype=torch.int32, device=device)
    return t.data_ptr()


def colsum(x2d: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate=False) -> torch.Tensor:
    _need_gpu(x2d)
    L = _lib.lib()
    M, N = x2d.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x2d.device)
    ws = _ws2.get(L.dl_colsum_workspace_bytes(M, N), x2d.device)
    check(L.dl_colsum(x2d.data_ptr(), x2d.stride(0), M, N, _dt(x2d), out.data_ptr(), int(accumulate),
                      ws.data_ptr(), ws.numel(), _stream()), "dl_colsum")
    return out


def layernorm_fwd(x2d, gamma, beta, eps):
    _need_gpu(x2d, gamma, beta)
    L = _lib.lib()
    M, D = x2d.shape
    y = torch.empty_like(x2d)
    mean = torch.empty(M, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x2d.device)
    check(L.dl_layernorm_fwd(x2d.data_ptr(), x2d.stride(0), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                             y.stride(0), mean.data_ptr(), rstd.data_ptr(), M, D, float(eps), _dt(x2d), _stream()),
          "dl_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy2d, x2d, mean, rstd, gamma, dres=None, need_param_grads=True, out=None, dy_share=1):
    """dy_share > 1: dy2d has M / dy_share rows, each shared by dy_share consecutive rows of x2d."""
    L = _lib.lib()
    M, D = x2d.shape
    if dy2d.shape[0] * dy_share != M:
        raise ValueError("layernorm_bwd: dy has %d rows, x %d, dy_share %d" % (dy2d.shape[0], M, dy_share))
    dx = torch.empty_like(x2d) if out is None else out
    dgamma = dbeta = None
    if need_param_grads:
        gb = torch.empty((2, D), dtype=torch.float32, device=x2d.device)   # adjacent: one final-reduction launch
        dgamma, dbeta = gb[0], gb[1]
    nbytes = L.dl_layernorm_bwd_workspace_bytes(M, D)
    item = None
    if _pending is not None and need_param_grads:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x2d.device)     # the partials outlive this call (deferred_reductions)
        item = _lib.ReduceItem()
    else:
        ws = _ws.get(nbytes, x2d.device)
    check(L.dl_layernorm_bwd(dy2d.data_ptr(), dy2d.stride(0), int(dy_share), x2d.data_ptr(), x2d.stride(0), mean.data_ptr(),
                             rstd.data_ptr(), gamma.data_ptr(), _ptr(dres), 0 if dres is None else dres.stride(0),
                             dx.data_ptr(), dx.stride(0), _ptr(dgamma), _ptr(dbeta), 0, M, D, _dt(x2d),
                             ws.data_ptr(), ws.numel(), None if item is None else C.pointer(item), _stream()), "dl_layernorm_bwd")
    if item is not None and item.kind != 0:
        _pending.append((item, ws, gb, None))
    return dx, dgamma, dbeta


def cast(src: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    if src.dtype == dtype:
        return src
    _need_gpu(src)
    src = src.contiguous()
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    check(_lib.lib().dl_cast(src.data_ptr(), _dt(src), dst.data_ptr(), _DT[dtype], src.numel(), _stream()), "dl_cast")
    return dst


def attn_fwd(q, k, v, *, n_problems, n_heads, n_segments, partner_shift, Lq, Lk, head_dim, scale,
             q_strides, k_strides, v_strides, out, o_strides, o_ss, need_lse=True, raw_logits=None, algo=0, key_tail=None):
    """Strides are (problem, head, row) in elements.  Returns the LSE tensor (or None).
    key_tail = (rows, weight): the last `rows` keys each stand for `weight` identical keys (dl_attn_fwd_args.key_tail_rows);
    raw_logits of such a key then hold scale * q.k + log(weight), the logit the softmax uses (a softmax over a raw row gives
    the weights of the distinct keys; GuidedCrossAttentionFn asks for no raw logits with key_tail)."""
    _need_gpu(q, k, v, out)
    a = AttnFwdArgs()
    a.Q, a.K, a.V, a.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    lse = None
    if need_lse:
        lse = torch.empty((n_segments, n_problems, n_heads, Lq), dtype=torch.float32, device=q.device)
    a.LSE = _ptr(lse)
    a.raw_logits = _ptr(raw_logits)
    a.q_ps, a.q_hs, a.q_rs = q_strides
    a.k_ps, a.k_hs, a.k_rs = k_strides
    a.v_ps, a.v_hs, a.v_rs = v_strides
    a.o_ps, a.o_hs, a.o_rs = o_strides
    a.o_ss = o_ss
    a.n_problems, a.n_heads, a.n_segments, a.partner_shift = n_problems, n_heads, n_segments, partner_shift
    a.Lq, a.Lk, a.head_dim, a.dtype = Lq, Lk, head_dim, _dt(q)
    a.scale = float(scale)
    a.algo = algo
    if key_tail is not None:
        a.key_tail_rows, a.key_tail_weight = int(key_tail[0]), float(key_tail[1])
    check(_lib.lib().dl_attn_fwd(C.byref(a), _stream()), "dl_attn_fwd")
    return lse


_ATTN_BWD_ALGO = int(os.environ.get("DL_ATTN_BWD_ALGO", "0"))    # A/B switch: 2 = always the dQ + dK/dV kernel pair, 3 = one-pass wherever eligible


def attn_bwd(q, k, v, o, do, lse, *, n_problems, n_heads, n_segments, partner_shift, Lq, Lk, head_dim, scale,
             q_strides, k_strides, v_strides, o_strides, o_ss, do_strides, do_ss, dq, dq_strides, dk, dk_strides,
             dv, dv_strides, algo=0, key_tail=None):
    _need_gpu(q, k, v, o, do)
    a = AttnBwdArgs()
    delta = torch.empty_like(lse)
    a.Q, a.K, a.V, a.O, a.dO = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr()
    a.LSE, a.Delta = lse.data_ptr(), delta.data_ptr()
    a.dQ, a.dK, a.dV = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.q_ps, a.q_hs, a.q_rs = q_strides
    a.k_ps, a.k_hs, a.k_rs = k_strides
    a.v_ps, a.v_hs, a.v_rs = v_strides
    a.o_ps, a.o_hs, a.o_rs = o_strides
    a.o_ss = o_ss
    a.do_ps, a.do_hs, a.do_rs = do_strides
    a.do_ss = do_ss
    a.dq_ps, a.dq_hs, a.dq_rs = dq_strides
    a.dk_ps, a.dk_hs, a.dk_rs = dk_strides
    a.dv_ps, a.dv_hs, a.dv_rs = dv_strides
    a.n_problems, a.n_heads, a.n_segments, a.partner_shift = n_problems, n_heads, n_segments, partner_shift
    a.Lq, a.Lk, a.head_dim, a.dtype = Lq, Lk, head_dim, _dt(q)
    a.scale = float(scale)
    a.algo = algo if algo else _ATTN_BWD_ALGO
    if key_tail is not None:
        a.key_tail_rows, a.key_tail_weight = int(key_tail[0]), float(key_tail[1])
    check(_lib.lib().dl_attn_bwd(C.byref(a), _stream()), "dl_attn_bwd")


def attn_probs(q, k, *, n_problems, n_heads, n_segments, partner_shift, Lq, Lk, head_dim, scale, q_strides, k_strides,
               lse=None, head_mean=False, key_tail=None, expand_tail=False, out=None, out_ld=None):
    """The attention probability map softmax(scale q k^T) in fp32 (dl_attn_probs): Q / K addressed as in attn_fwd.
    Returns (S, P, Lq, cols) with head_mean, (S, P, H, Lq, cols) otherwise; cols = Lk, or with key_tail = (rows, weight) and
    expand_tail the full key count Lk - rows + rows * weight in functional.ExpandTailFn's order.  lse: the LSE of an attn_fwd
    call on the same q, k, scale and key_tail; None = computed here into a workspace.  out / out_ld (elements): write into
    this buffer with this row pitch instead (the same rows, out_ld apart; returns `out`)."""
    _need_gpu(q, k, lse, out)
    a = AttnProbsArgs()
    a.Q, a.K, a.LSE = q.data_ptr(), k.data_ptr(), _ptr(lse)
    a.q_ps, a.q_hs, a.q_rs = q_strides
    a.k_ps, a.k_hs, a.k_rs = k_strides
    a.n_problems, a.n_heads, a.n_segments, a.partner_shift = n_problems, n_heads, n_segments, partner_shift
    a.Lq, a.Lk, a.head_dim, a.dtype = Lq, Lk, head_dim, _dt(q)
    a.scale = float(scale)
    a.head_mean, a.expand_tail = int(bool(head_mean)), int(bool(expand_tail))
    cols = Lk
    if key_tail is not None:
        a.key_tail_rows, a.key_tail_weight = int(key_tail[0]), float(key_tail[1])
        if expand_tail:
            cols = Lk - int(key_tail[0]) + int(key_tail[0]) * int(key_tail[1])
    if lse is not None and (lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != n_segments * n_problems * n_heads * Lq):
        raise ValueError("attn_probs: lse must be a contiguous float32 tensor of (n_segments, n_problems, n_heads, Lq)")
    if out is None:
        shape = (n_segments, n_problems, Lq, cols) if head_mean else (n_segments, n_problems, n_heads, Lq, cols)
        out = torch.empty(shape, dtype=torch.float32, device=q.device)
        out_ld = cols
    else:
        rows = n_segments * n_problems * (1 if head_mean else n_heads) * Lq
        if out.dtype != torch.float32 or out_ld is None or not out.is_contiguous() or out.device != q.device:
            raise ValueError("attn_probs: out must be a contiguous float32 tensor on q's device and come with its row pitch out_ld")
        if out_ld < cols or out.numel() < (rows - 1) * int(out_ld) + cols:
            raise ValueError("attn_probs: out holds %d elements, %d rows of %d columns at pitch %d need %d"
                             % (out.numel(), rows, cols, out_ld, (rows - 1) * int(out_ld) + cols))
    a.out, a.out_ld = out.data_ptr(), int(out_ld)
    L = _lib.lib()
    if lse is None:
        ws = _ws.get(L.dl_attn_probs_workspace_bytes(C.byref(a)), q.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    check(L.dl_attn_probs(C.byref(a), _stream()), "dl_attn_probs")
    return out


def _check_pair_operands(who, q, store, store_name, store_dims, q_index, kv_index):
    """The operand checks of every pair-indexed launch: q, the [K | V'] store and the index vectors."""
    if (q.dim() != 3 or store.dim() != len(store_dims) + 1 or q.shape[2] != 128 or store.shape[-1] != 256 or q.stride(2) != 1
            or store.stride(-1) != 1):
        raise ValueError("%s: q must be (n_q, Lq, 128) and %s (%s, 256) with contiguous columns" % (who, store_name, ", ".join(store_dims)))
    if store.dtype != q.dtype:
        raise ValueError("%s: q is %s, %s is %s" % (who, q.dtype, store_name, store.dtype))
    for t in (q_index, kv_index):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != q_index.numel():
            raise ValueError("%s: q_index / kv_index must be contiguous int32 vectors of one length" % who)


def _fill_pair_head(a, q, store, q_index, kv_index, scale):
    """The fields that all eight pair-indexed argument blocks share (after _check_pair_operands)."""
    a.Q, a.K = q.data_ptr(), store.data_ptr()
    a.q_index, a.kv_index, a.flags = q_index.data_ptr(), kv_index.data_ptr(), guard_flags(q.device).data_ptr()
    a.q_es, a.q_rs = q.stride(0), q.stride(1)
    a.k_rs = store.stride(-2)
    a.n_pairs, (a.n_q, a.Lq, a.head_dim), a.dtype = q_index.numel(), q.shape, _dt(q)
    a.scale = float(scale)


def _check_cols(who, cols):
    cols = int(cols)
    if cols < 1:
        raise ValueError("%s: cols %d must be positive" % (who, cols))
    return cols


def _dense_keys(a, kv, key_tail, cols=0, expand=False):
    """The dense-key fields of an argument block: key_tail = (rows, weight), and from kv (n_kv, Lk, 256) the entity stride and
    counts.  Returns cols, by default the columns of a map: Lk, or under `expand` the full key count Lk - rows + rows * weight
    (0 where kv has no such shape: the operand checks that follow reject it)."""
    t, w = (int(key_tail[0]), float(key_tail[1])) if key_tail is not None else (0, 1.0)
    if key_tail is not None:
        a.key_tail_rows, a.key_tail_weight = t, w
    if kv.dim() == 3:
        a.k_es = kv.stride(0)
        a.n_kv, a.Lk = kv.shape[:2]
        if cols is None:
            cols = kv.shape[1] - t + t * int(w) if (expand and t) else kv.shape[1]
    return cols or 0


def _check_key_table(who, q, row0, n_keys, tail_weight, key_tail_rows=0):
    for t, dt, what in ((row0, torch.int64, "row0 int64"), (n_keys, torch.int32, "n_keys int32"), (tail_weight, torch.float32, "tail_weight float32")):
        if t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.numel() != row0.numel() or t.device != q.device:
            raise ValueError("%s: the key table is three contiguous vectors of one length on q's device "
                             "(row0 int64, n_keys int32, tail_weight float32); %s is %s %s" % (who, what, t.dtype, tuple(t.shape)))
    if int(key_tail_rows) < 0:
        raise ValueError("%s: key_tail_rows %d is negative" % (who, int(key_tail_rows)))


def _fill_key_table(a, rows, row0, n_keys, tail_weight, key_tail_rows):
    """The ragged-key fields of an argument block (after _check_key_table and _check_pair_operands)."""
    a.kv_row0, a.kv_keys, a.kv_tail_weight = row0.data_ptr(), n_keys.data_ptr(), tail_weight.data_ptr()
    a.kv_total_rows, a.n_kv = rows.shape[0], row0.numel()
    a.key_tail_rows = int(key_tail_rows)


def _rows_out_ok(out, specs, n_pairs, device):
    """out is one 2-D tensor per (dtype, width) of specs: (n_pairs, >= width) on device, contiguous columns, non-overlapping rows."""
    ok = isinstance(out, (tuple, list)) and len(out) == len(specs)
    for t, (dt, width) in zip(out if ok else (), specs):
        ok = ok and (t.dim() == 2 and t.dtype == dt and t.device == device and t.shape[0] == n_pairs and t.shape[1] >= width
                     and t.stride(1) == 1 and t.stride(0) >= width)
    return ok


def _pgca_pairs_common(who, a, q, store, store_name, store_dims, q_index, kv_index, scale, left, bias, out):
    """What pgca_pairs and pgca_pairs_ragged share: the checks of q, of the [K | V'] store (store_name and the names of its
    leading dimensions are what the messages call it), of the index vectors, left and bias; out, allocated or validated; the
    fields that PgcaPairsArgs and PgcaPairsRaggedArgs have in common, filled into `a`.  Returns out."""
    _check_pair_operands(who, q, store, store_name, store_dims, q_index, kv_index)
    n_pairs, (n_q, Lq, E) = q_index.numel(), q.shape
    left_cols = 0
    if left is not None:
        if left.dim() != 3 or left.shape[:2] != q.shape[:2] or left.dtype != q.dtype or left.stride(2) != 1:
            raise ValueError("%s: left must be (n_q, Lq, cols) of q's dtype with contiguous columns" % who)
        left_cols = left.shape[2]
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != E or not bias.is_contiguous()):
        raise ValueError("%s: bias must be a contiguous float32 vector of %d" % (who, E))
    cols = left_cols + E
    if out is None:
        out = torch.empty((n_pairs, Lq, cols), dtype=q.dtype, device=q.device)
    elif (out.dim() != 3 or out.dtype != q.dtype or out.device != q.device or out.shape[0] != n_pairs or out.shape[1] != Lq
          or out.shape[2] < cols or out.stride(2) != 1 or out.stride(1) < cols or (n_pairs > 1 and out.stride(0) < (Lq - 1) * out.stride(1) + cols)):
        raise ValueError("%s: out must be a %s tensor of (%d, %d, >= %d) on q's device with contiguous columns and "
                         "non-overlapping rows (got %s, strides %s)" % (who, q.dtype, n_pairs, Lq, cols, tuple(out.shape), out.stride()))
    _fill_pair_head(a, q, store, q_index, kv_index, scale)
    a.V, a.left, a.out, a.bias = store.data_ptr() + E * store.element_size(), _ptr(left), out.data_ptr(), _ptr(bias)
    a.v_rs = a.k_rs
    if left is not None:
        a.left_es, a.left_rs = left.stride(0), left.stride(1)
    a.out_ps, a.out_rs = out.stride(0), out.stride(1)
    a.left_cols, a.out_col0 = left_cols, left_cols
    return out


def pgca_pairs(q, kv, q_index, kv_index, *, scale, left=None, bias=None, key_tail=None, out=None):
    """The pair-indexed PGCA attention core over cached entity codes (dl_pgca_pairs_fwd).  q (n_q, Lq, 128): the projected
    queries per protein; kv (n_kv, Lk, 256) = [K | V']: the projected keys and the values behind the out-projection per drug
    (screening.DrugCode); q_index / kv_index (n_pairs,) int32 device tensors.  Pair n gets softmax(scale q[qi] k[ki]^T) v'[ki]
    (+ bias, fp32 (128,)) at columns left_cols.. of out[n], and left[qi] (n_q, Lq, left_cols) bit for bit in front of it.
    Entities may be views with any 16-byte-aligned entity and row strides (columns contiguous).  out (n_pairs, Lq, left_cols
    + 128) is allocated unless given; a caller's out may have wider rows.  key_tail = (rows, weight) as in attn_fwd.  A pair
    with an index out of range is skipped and sets FLAG_PAIR_INDEX in the device guard word (check_guard_flags)."""
    _need_gpu(q, kv, q_index, kv_index, left, bias, out)
    a = PgcaPairsArgs()
    _dense_keys(a, kv, key_tail)
    a.v_es = a.k_es
    out = _pgca_pairs_common("pgca_pairs", a, q, kv, "kv", ("n_kv", "Lk"), q_index, kv_index, scale, left, bias, out)
    check(_lib.lib().dl_pgca_pairs_fwd(C.byref(a), _stream()), "dl_pgca_pairs_fwd")
    return out


def pgca_pairs_ragged(q, rows, row0, n_keys, tail_weight, q_index, kv_index, *, scale, key_tail_rows, left=None, bias=None, out=None):
    """pgca_pairs over a packed per-drug row store (dl_pgca_pairs_ragged_fwd; screening.DrugLibrary).  q (n_q, Lq, 128) as in
    pgca_pairs; rows (R, 256) = [K | V'] of every drug back to back; drug d owns rows row0[d] .. row0[d] + n_keys[d] - 1, and
    each of its last key_tail_rows rows (launch-wide) stands for tail_weight[d] >= 1 identical keys.  row0 int64, n_keys int32,
    tail_weight float32: contiguous device vectors of one length (the number of drugs).  left / bias / out as in pgca_pairs.
    A pair with an index out of range sets FLAG_PAIR_INDEX, one whose drug's table entry does not describe rows inside
    `rows` sets FLAG_KEY_TABLE in the device guard word (check_guard_flags); either pair is skipped."""
    _need_gpu(q, rows, row0, n_keys, tail_weight, q_index, kv_index, left, bias, out)
    _check_key_table("pgca_pairs_ragged", q, row0, n_keys, tail_weight, key_tail_rows)
    a = PgcaPairsRaggedArgs()
    out = _pgca_pairs_common("pgca_pairs_ragged", a, q, rows, "rows", ("R",), q_index, kv_index, scale, left, bias, out)
    _fill_key_table(a, rows, row0, n_keys, tail_weight, key_tail_rows)
    check(_lib.lib().dl_pgca_pairs_ragged_fwd(C.byref(a), _stream()), "dl_pgca_pairs_ragged_fwd")
    return out


def _pgca_maps_common(who, a, q, store, store_name, store_dims, q_index, kv_index, scale, cols, expand_tail, out):
    """What pgca_pairs_probs and pgca_pairs_ragged_probs share: the checks of q, of the [K | V'] store and of the index vectors;
    out (n_pairs, Lq, cols) fp32, allocated or validated; the fields the two argument blocks have in common.  Returns out."""
    _check_pair_operands(who, q, store, store_name, store_dims, q_index, kv_index)
    cols = _check_cols(who, cols)
    n_pairs, Lq = q_index.numel(), q.shape[1]
    if out is None:
        out = torch.empty((n_pairs, Lq, cols), dtype=torch.float32, device=q.device)
    elif (out.dim() != 3 or out.dtype != torch.float32 or out.device != q.device or out.shape[0] != n_pairs or out.shape[1] != Lq
          or out.shape[2] < cols or out.stride(2) != 1 or out.stride(1) < cols or (n_pairs > 1 and out.stride(0) < (Lq - 1) * out.stride(1) + cols)):
        raise ValueError("%s: out must be a float32 tensor of (%d, %d, >= %d) on q's device with contiguous columns and "
                         "non-overlapping rows (got %s %s, strides %s)" % (who, n_pairs, Lq, cols, out.dtype, tuple(out.shape), out.stride()))
    _fill_pair_head(a, q, store, q_index, kv_index, scale)
    a.out, a.out_ps, a.out_rs = out.data_ptr(), out.stride(0), out.stride(1)
    a.out_cols, a.expand_tail = cols, int(bool(expand_tail))
    return out


def pgca_pairs_probs(q, kv, q_index, kv_index, *, scale, key_tail=None, expand_tail=False, cols=None, out=None):
    """The PGCA probability maps of (protein, drug) pairs over cached entity codes (dl_pgca_pairs_probs): pair n gets
    softmax(scale q[qi] k[ki]^T) as fp32, k = the first 128 columns of kv (n_kv, Lk, 256) = [K | V'] as pgca_pairs takes it (the
    values are not read).  key_tail = (rows, weight) as in attn_fwd: without expand_tail a row has Lk columns and a tail column
    carries the mass of the keys it stands for; with expand_tail it has the full key count Lk - rows + rows * weight in
    functional.ExpandTailFn's order (weight must be whole).  Returns (n_pairs, Lq, cols) float32; cols defaults to that column
    count, columns beyond it are +0.0.  out: write into this tensor instead (a caller's out may have wider rows).  A pair with
    an index out of range is skipped and sets FLAG_PAIR_INDEX in the device guard word (check_guard_flags)."""
    _need_gpu(q, kv, q_index, kv_index, out)
    a = PgcaPairsProbsArgs()
    cols = _dense_keys(a, kv, key_tail, cols, expand_tail)
    out = _pgca_maps_common("pgca_pairs_probs", a, q, kv, "kv", ("n_kv", "Lk"), q_index, kv_index, scale, cols, expand_tail, out)
    check(_lib.lib().dl_pgca_pairs_probs(C.byref(a), _stream()), "dl_pgca_pairs_probs")
    return out


def pgca_pairs_ragged_probs(q, rows, row0, n_keys, tail_weight, q_index, kv_index, *, scale, key_tail_rows, cols, expand_tail=False, out=None):
    """pgca_pairs_probs over a packed per-drug row store (dl_pgca_pairs_ragged_probs; screening.DrugLibrary): the key table is
    pgca_pairs_ragged's.  Drug d's map has n_keys[d] columns, or with expand_tail n_keys[d] - key_tail_rows + key_tail_rows *
    tail_weight[d]; every row is written over `cols` columns (+0.0 behind the drug's own).  Returns (n_pairs, Lq, cols) float32.
    A pair is skipped and flagged in the device guard word (check_guard_flags) when its index is out of range (FLAG_PAIR_INDEX),
    its drug's table entry does not describe rows inside `rows` (FLAG_KEY_TABLE), or its map has more than `cols` columns or
    expand_tail meets a weight that is not whole (FLAG_MAP_COLS)."""
    _need_gpu(q, rows, row0, n_keys, tail_weight, q_index, kv_index, out)
    _check_key_table("pgca_pairs_ragged_probs", q, row0, n_keys, tail_weight, key_tail_rows)
    a = PgcaPairsRaggedProbsArgs()
    out = _pgca_maps_common("pgca_pairs_ragged_probs", a, q, rows, "rows", ("R",), q_index, kv_index, scale, cols, expand_tail, out)
    _fill_key_table(a, rows, row0, n_keys, tail_weight, key_tail_rows)
    check(_lib.lib().dl_pgca_pairs_ragged_probs(C.byref(a), _stream()), "dl_pgca_pairs_ragged_probs")
    return out


def _pgca_profile_common(who, a, q, store, store_name, store_dims, q_index, kv_index, scale, cols, out):
    """What pgca_pairs_profile and pgca_pairs_ragged_profile share: the checks of q, of the [K | V'] store and of the index
    vectors; the outputs (key_mass (n_pairs, cols) fp32, site_peak (n_pairs, Lq) fp32, site_key (n_pairs, Lq) int32), allocated
    or validated; the fields the two argument blocks have in common.  Returns the three outputs."""
    _check_pair_operands(who, q, store, store_name, store_dims, q_index, kv_index)
    cols = _check_cols(who, cols)
    n_pairs, Lq = q_index.numel(), q.shape[1]
    if out is None:
        out = (torch.empty((n_pairs, cols), dtype=torch.float32, device=q.device),
               torch.empty((n_pairs, Lq), dtype=torch.float32, device=q.device),
               torch.empty((n_pairs, Lq), dtype=torch.int32, device=q.device))
    else:
        ok = _rows_out_ok(out, ((torch.float32, cols), (torch.float32, Lq), (torch.int32, Lq)), n_pairs, q.device)
        if not ok or out[1].stride(0) != out[2].stride(0):
            raise ValueError("%s: out must be (key_mass float32 (%d, >= %d), site_peak float32 (%d, >= %d), site_key int32 (%d, >= %d)) "
                             "on q's device with contiguous columns, non-overlapping rows and one row pitch for the two site "
                             "outputs" % (who, n_pairs, cols, n_pairs, Lq, n_pairs, Lq))
        out = tuple(out)
    mass, peak, skey = out
    _fill_pair_head(a, q, store, q_index, kv_index, scale)
    a.key_mass, a.site_peak, a.site_key = mass.data_ptr(), peak.data_ptr(), skey.data_ptr()
    a.mass_ps, a.site_ps = mass.stride(0), peak.stride(0)
    a.out_cols = cols
    return out


def pgca_pairs_profile(q, kv, q_index, kv_index, *, scale, key_tail=None, cols=None, out=None):
    """Hit profiles of (protein, drug) pairs over cached entity codes (dl_pgca_pairs_profile): the two reductions of the map P
    that pgca_pairs_probs(expand_tail=True) gives for pair n, from ONE launch that never writes the map.  Returns
    (key_mass (n_pairs, cols) fp32: the mean of P over the query rows, the share of the protein's attention each drug key
    receives, +0.0 behind the drug's full key count; site_peak (n_pairs, Lq) fp32: a row's largest probability; site_key
    (n_pairs, Lq) int32: the stored key that receives it — the smallest column attaining the maximum, so a tail key is named by
    its copy 0 and competes with ONE copy's probability).  q, kv, key_tail, cols as in pgca_pairs_probs (the weight must be
    whole; kv of at most 576 keys).  out: the three tensors to write into (rows may be wider; the two site outputs share one
    pitch).  A pair with an index out of range is skipped and sets FLAG_PAIR_INDEX in the device guard word."""
    _need_gpu(q, kv, q_index, kv_index, *(out if isinstance(out, (tuple, list)) else ()))
    a = PgcaPairsProfileArgs()
    cols = _dense_keys(a, kv, key_tail, cols, True)
    out = _pgca_profile_common("pgca_pairs_profile", a, q, kv, "kv", ("n_kv", "Lk"), q_index, kv_index, scale, cols, out)
    check(_lib.lib().dl_pgca_pairs_profile(C.byref(a), _stream()), "dl_pgca_pairs_profile")
    return out


def pgca_pairs_ragged_profile(q, rows, row0, n_keys, tail_weight, q_index, kv_index, *, scale, key_tail_rows, cols, out=None):
    """pgca_pairs_profile over a packed per-drug row store (dl_pgca_pairs_ragged_profile; screening.DrugLibrary): the key table
    is pgca_pairs_ragged's, the profile that of the drug's map over its full key set (n_keys[d] - key_tail_rows + key_tail_rows *
    tail_weight[d] columns of `cols`).  A pair is skipped — none of the three outputs is written for it — and flagged in the
    device guard word (check_guard_flags) when its index is out of range (FLAG_PAIR_INDEX), its drug's table entry does not
    describe rows inside `rows` (FLAG_KEY_TABLE), or its map has more than `cols` columns, its weight is not whole or it has
    more than 576 stored keys (FLAG_MAP_COLS)."""
    _need_gpu(q, rows, row0, n_keys, tail_weight, q_index, kv_index, *(out if isinstance(out, (tuple, list)) else ()))
    _check_key_table("pgca_pairs_ragged_profile", q, row0, n_keys, tail_weight, key_tail_rows)
    a = PgcaPairsRaggedProfileArgs()
    out = _pgca_profile_common("pgca_pairs_ragged_profile", a, q, rows, "rows", ("R",), q_index, kv_index, scale, cols, out)
    _fill_key_table(a, rows, row0, n_keys, tail_weight, key_tail_rows)
    check(_lib.lib().dl_pgca_pairs_ragged_profile(C.byref(a), _stream()), "dl_pgca_pairs_ragged_profile")
    return out


def _pgca_attr_common(who, a, q, store, store_name, store_dims, d_out, q_index, kv_index, scale, cols, sites, d_sites, out):
    """What pgca_pairs_attr and pgca_pairs_ragged_attr share: the checks of q, of the [K | V'] store, of the index vectors, of
    d_out and of sites / d_sites; the outputs (key_attr (n_pairs, cols) fp32, site_attr (n_pairs, Lq) fp32), allocated or
    validated; the fields the two argument blocks have in common.  Returns the two outputs."""
    _check_pair_operands(who, q, store, store_name, store_dims, q_index, kv_index)
    cols = _check_cols(who, cols)
    n_pairs, (Lq, E) = q_index.numel(), q.shape[1:]
    if d_out.dtype != q.dtype:
        raise ValueError("%s: q is %s, d_out is %s" % (who, q.dtype, d_out.dtype))
    if d_out.dim() != 3 or tuple(d_out.shape) != (n_pairs, Lq, E) or d_out.stride(2) != 1:
        raise ValueError("%s: d_out must be (%d, %d, %d) with contiguous columns (got %s, strides %s)"
                         % (who, n_pairs, Lq, E, tuple(d_out.shape), d_out.stride()))
    if (sites is None) != (d_sites is None):
        raise ValueError("%s: sites and d_sites are given both or neither" % who)
    if sites is not None:
        if sites.dim() != 3 or sites.shape[:2] != q.shape[:2] or sites.dtype != q.dtype or sites.stride(2) != 1:
            raise ValueError("%s: sites must be (n_q, Lq, cols) of q's dtype with contiguous columns" % who)
        if (d_sites.dim() != 3 or tuple(d_sites.shape) != (n_pairs, Lq, sites.shape[2]) or d_sites.dtype != q.dtype
                or d_sites.stride(2) != 1):
            raise ValueError("%s: d_sites must be (%d, %d, %d) of q's dtype with contiguous columns" % (who, n_pairs, Lq, sites.shape[2]))
    if out is None:
        out = (torch.empty((n_pairs, cols), dtype=torch.float32, device=q.device),
               torch.empty((n_pairs, Lq), dtype=torch.float32, device=q.device))
    else:
        if not _rows_out_ok(out, ((torch.float32, cols), (torch.float32, Lq)), n_pairs, q.device):
            raise ValueError("%s: out must be (key_attr float32 (%d, >= %d), site_attr float32 (%d, >= %d)) on q's device with "
                             "contiguous columns and non-overlapping rows" % (who, n_pairs, cols, n_pairs, Lq))
        out = tuple(out)
    kattr, sattr = out
    _fill_pair_head(a, q, store, q_index, kv_index, scale)
    a.dO, a.sites, a.d_sites = d_out.data_ptr(), _ptr(sites), _ptr(d_sites)
    a.key_attr, a.site_attr = kattr.data_ptr(), sattr.data_ptr()
    a.do_ps, a.do_rs = d_out.stride(0), d_out.stride(1)
    if sites is not None:
        a.left_es, a.left_rs = sites.stride(0), sites.stride(1)
        a.dl_ps, a.dl_rs = d_sites.stride(0), d_sites.stride(1)
        a.left_cols = sites.shape[2]
    a.mass_ps, a.site_ps = kattr.stride(0), sattr.stride(0)
    a.out_cols = cols
    return out


def pgca_pairs_attr(q, kv, d_out, q_index, kv_index, *, scale, key_tail=None, cols=None, sites=None, d_sites=None, out=None):
    """Hit attributions of (protein, drug) pairs over cached entity codes (dl_pgca_pairs_attr): gradient x code at the pair-stage
    interface, from ONE launch that forms no dQ, dK or dV'.  d_out (n_pairs, Lq, 128) is the gradient of a target w.r.t. the
    attention output of pair n (contiguous columns, any 16-byte-aligned row and pair strides: the right half of a concat's
    gradient is fine).  Returns (key_attr (n_pairs, cols) fp32: per drug key, (<dK_c, K_c> + <dV'_c, V'_c>) for ONE copy of the
    key, at the column of every copy as pgca_pairs_profile's key_mass lays them out, +0.0 behind the drug's full key count;
    site_attr (n_pairs, Lq) fp32: per protein site, <dq_r, q_r>, plus <d_sites_r, sites_r> when sites (n_q, Lq, c) and d_sites
    (n_pairs, Lq, c) are given — both or neither).  The leaves are the cached codes q, sites and [K | V'], not the raw inputs
    in front of the encoders; the values are signed.  q, kv, key_tail, cols and the flags as in pgca_pairs_profile; out: the two
    tensors to write into (rows may be wider)."""
    _need_gpu(q, kv, d_out, q_index, kv_index, sites, d_sites, *(out if isinstance(out, (tuple, list)) else ()))
    a = PgcaPairsAttrArgs()
    cols = _dense_keys(a, kv, key_tail, cols, True)
    out = _pgca_attr_common("pgca_pairs_attr", a, q, kv, "kv", ("n_kv", "Lk"), d_out, q_index, kv_index, scale, cols, sites, d_sites, out)
    check(_lib.lib().dl_pgca_pairs_attr(C.byref(a), _stream()), "dl_pgca_pairs_attr")
    return out


def pgca_pairs_ragged_attr(q, rows, row0, n_keys, tail_weight, d_out, q_index, kv_index, *, scale, key_tail_rows, cols, sites=None,
                           d_sites=None, out=None):
    """pgca_pairs_attr over a packed per-drug row store (dl_pgca_pairs_ragged_attr; screening.DrugLibrary): the key table is
    pgca_pairs_ragged's, the columns those of the drug's full key set (n_keys[d] - key_tail_rows + key_tail_rows *
    tail_weight[d] of `cols`).  Gradient x code at the pair-stage interface: the leaves are the cached codes, not the raw inputs.
    A pair is skipped — neither output is written for it — and flagged in the device guard word (check_guard_flags) under
    pgca_pairs_ragged_profile's conditions."""
    _need_gpu(q, rows, row0, n_keys, tail_weight, d_out, q_index, kv_index, sites, d_sites, *(out if isinstance(out, (tuple, list)) else ()))
    _check_key_table("pgca_pairs_ragged_attr", q, row0, n_keys, tail_weight, key_tail_rows)
    a = PgcaPairsRaggedAttrArgs()
    out = _pgca_attr_common("pgca_pairs_ragged_attr", a, q, rows, "rows", ("R",), d_out, q_index, kv_index, scale, cols, sites, d_sites, out)
    _fill_key_table(a, rows, row0, n_keys, tail_weight, key_tail_rows)
    check(_lib.lib().dl_pgca_pairs_ragged_attr(C.byref(a), _stream()), "dl_pgca_pairs_ragged_attr")
    return out


def dropout_apply(x2d: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    y = torch.empty_like(x2d)
    rows, D = x2d.shape
    check(_lib.lib().dl_dropout_apply(x2d.data_ptr(), y.data_ptr(), rows, D, x2d.stride(0), y.stride(0), float(p),
                                      int(seed), _seed_offset_ptr(x2d.device), _dt(x2d), _stream()), "dl_dropout_apply")
    return y


# ------------------------------------------------------------------------------------------------
# dropout seeds: one generator per process; each dropout site draws a fresh 63-bit seed per forward
# ------------------------------------------------------------------------------------------------
_seed_gen = torch.Generator(device="cpu")
_seed_gen.manual_seed(0x5EED)


def manual_seed(seed: int) -> None:
    _seed_gen.manual_seed(int(seed))


# Device-resident seed offset (one uint64 per device): every dropout site keys its mask by (site seed + offset), the
# kernels read the offset when they RUN.  Eager steps leave it at 0; a hipGraph-captured step (trainer.GraphedStep)
# bumps it with an in-graph add so that each replay of the frozen launch arguments still draws fresh masks.
_seed_offsets = {}
_seed_offset_on = False


def seed_offset_tensor(device) -> torch.Tensor:
    key = (device.type, device.index)
    t = _seed_offsets.get(key)
    if t is None:
        t = torch.zeros(1, dtype=torch.int64, device=device)
        _seed_offsets[key] = t
    return t


def use_seed_offset(on: bool) -> None:
    """Route dropout sites through the device-resident offset (needed while capturing / replaying a graphed step)."""
    global _seed_offset_on
    _seed_offset_on = bool(on)


def _seed_offset_ptr(device):
    return seed_offset_tensor(device).data_ptr() if _seed_offset_on else None


def next_seed() -> int:
    return int(torch.randint(0, 2 ** 62, (1,), generator=_seed_gen).item())


def seed_state(device) -> dict:
    """What the dropout sites of the next step depend on, for a checkpoint: the site-seed generator's state (a CPU byte
    tensor), the device-resident offset's value (reading it waits for the device) and whether the offset is in use."""
    return {"generator": _seed_gen.get_state().clone(), "offset": int(seed_offset_tensor(device).item()), "offset_on": bool(_seed_offset_on)}


def set_seed_state(state: dict, device) -> None:
    """Put a seed_state() back.  Generator, offset and the switch are process-global: every model of the process draws from
    them."""
    _seed_gen.set_state(state["generator"].to(torch.uint8).cpu())
    seed_offset_tensor(device).fill_(int(state["offset"]))
    use_seed_offset(bool(state["offset_on"]))


def rowmod_sum(x2d: torch.Tensor, L: int) -> torch.Tensor:
    M, D = x2d.shape
    out = torch.empty((L, D), dtype=torch.float32, device=x2d.device)
    check(_lib.lib().dl_rowmod_sum(x2d.data_ptr(), out.data_ptr(), M, D, L, 0, _dt(x2d), _stream()), "dl_rowmod_sum")
    return out


def add_rowmod_dropout(x2d: torch.Tensor, pe2d: Optional[torch.Tensor], p: float, seed: int) -> torch.Tensor:
    M, D = x2d.shape
    y = torch.empty_like(x2d)
    Lr = pe2d.shape[0] if pe2d is not None else 1
    check(_lib.lib().dl_add_rowmod_dropout(x2d.data_ptr(), _ptr(pe2d), y.data_ptr(), M, D, Lr, float(p), int(seed),
                                           _seed_offset_ptr(x2d.device) if p > 0 else None, _dt(x2d), _stream()),
          "dl_add_rowmod_dropout")
    return y


def token_gate_fwd(v: torch.Tensor, logits: torch.Tensor, H: int, add_residual: bool):
    B, L, D = v.shape
    out = torch.empty_like(v)
    gate = torch.empty((B, H, L), dtype=torch.float32, device=v.device)
    check(_lib.lib().dl_token_gate_fwd(v.data_ptr(), logits.data_ptr(), out.data_ptr(), gate.data_ptr(), B, L, D, H,
                                       int(add_residual), _dt(v), _stream()), "dl_token_gate_fwd")
    return out, gate


def token_gate_bwd(dout, v, gate, H: int, add_residual: bool):
    B, L, D = v.shape
    dv = torch.empty_like(v)
    dlogits = torch.empty((B, L, H), dtype=v.dtype, device=v.device)
    check(_lib.lib().dl_token_gate_bwd(dout.data_ptr(), v.data_ptr(), gate.data_ptr(), dv.data_ptr(),
                                       dlogits.data_ptr(), B, L, D, H, int(add_residual), _dt(v), _stream()),
          "dl_token_gate_bwd")
    return dv, dlogits


# ---- fused AdamW (csrc/optim.hip): the plain, the guarded and the grouped step are one kernel behind three entry points ----
def _adamw(who, param, grad, exp_avg, exp_avg_sq, *, lr, beta1, beta2, eps, weight_decay=0.0, step, grad_scale, lowp,
           guard=None, quad_group=None, group_tab=None):
    """Validate the tensors (TypeError / ValueError before the library is called, nothing launched), then call the entry point
    the optional operands select: dl_adamw_step_groups with a group table, dl_adamw_step_guarded with a guard alone,
    dl_adamw_step with neither."""
    n = param.numel()
    _need_gpu(param, grad, exp_avg, exp_avg_sq, lowp, guard, quad_group, group_tab)
    for name, t in (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("lowp", lowp),
                    ("guard", guard), ("quad_group", quad_group), ("group_tab", group_tab)):
        if t is None:
            continue
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (who, name))
        if t.device != param.device:
            raise ValueError("%s: %s is on %s, param on %s" % (who, name, t.device, param.device))
    for name, t in (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("guard", guard)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("%s: %s must be float32 (got %s)" % (who, name, t.dtype))
    for name, t in (("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("lowp", lowp)):
        if t is not None and t.numel() != n:
            raise ValueError("%s: %s has %d elements, param %d" % (who, name, t.numel(), n))
    if lowp is not None and lowp.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("%s: lowp must be float32 or bfloat16 (got %s)" % (who, lowp.dtype))
    if guard is not None and guard.numel() < 4:
        raise ValueError("%s: guard must hold 4 floats (got %d)" % (who, guard.numel()))
    lead = (param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n, float(lr), float(beta1), float(beta2),
            float(eps))
    tail = (int(step), float(grad_scale), _ptr(lowp), _DT[lowp.dtype] if lowp is not None else 0)
    if group_tab is not None:
        if quad_group.dtype != torch.uint8 or quad_group.numel() != (n + 3) // 4:
            raise ValueError("%s: quad_group must be a contiguous uint8 tensor of ceil(n / 4) = %d entries (got %s, %d)"
                             % (who, (n + 3) // 4, quad_group.dtype, quad_group.numel()))
        if group_tab.dtype != torch.float32 or group_tab.dim() != 2 or group_tab.shape[1] != 2:
            raise ValueError("%s: group_tab must be a contiguous float32 (n_groups, 2) tensor (got %s, %s)"
                             % (who, group_tab.dtype, tuple(group_tab.shape)))
        rc = _lib.lib().dl_adamw_step_groups(*lead, *tail, quad_group.data_ptr(), group_tab.data_ptr(), int(group_tab.shape[0]),
                                             _ptr(guard), _stream())
    elif guard is not None:
        rc = _lib.lib().dl_adamw_step_guarded(*lead, float(weight_decay), *tail, guard.data_ptr(), _stream())
    else:
        rc = _lib.lib().dl_adamw_step(*lead, float(weight_decay), *tail, _stream())
    check(rc, "dl_" + who)


def adamw_step(param, grad, exp_avg, exp_avg_sq, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, step,
               grad_scale=1.0, lowp=None):
    _adamw("adamw_step", param, grad, exp_avg, exp_avg_sq, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
           step=step, grad_scale=grad_scale, lowp=lowp)


# ---- gradient guard (csrc/grad_guard.hip): global-norm clipping and the non-finite step skip, decided on the device ----
def grad_sqnorm_workspace_bytes(n: int) -> int:
    """include/druglamp_hip.h: 8 * min(2048, ceil(n / 4096))."""
    return 8 * min(2048, (int(n) + 4095) // 4096)


def grad_sqnorm(g, acc, workspace, accumulate: bool = False):
    """acc[0] (+)= sum of squares of the fp32 run g, in fp64, fixed order (two calls agree bitwise)."""
    check(_lib.lib().dl_grad_sqnorm(g.data_ptr(), g.numel(), acc.data_ptr(), int(bool(accumulate)), workspace.data_ptr(),
                                    workspace.numel() * workspace.element_size(), _stream()), "dl_grad_sqnorm")


def grad_guard_finalize(acc, guard, counters, *, pre_scale: float = 1.0, max_norm: float = 0.0, skip_nonfinite: bool = False):
    """acc -> guard = {clip coefficient, norm, skip flag, 0}; counters = {skipped, clipped} are added to."""
    check(_lib.lib().dl_grad_guard_finalize(acc.data_ptr(), float(pre_scale), float(max_norm), int(bool(skip_nonfinite)),
                                            guard.data_ptr(), counters.data_ptr(), _stream()), "dl_grad_guard_finalize")


def adamw_step_guarded(param, grad, exp_avg, exp_avg_sq, guard, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, step,
                       grad_scale=1.0, lowp=None):
    """adamw_step with the gradient scaled by grad_scale * guard[0]; writes nothing when guard[2] != 0."""
    if guard is None:
        raise ValueError("adamw_step_guarded: guard is None")
    _adamw("adamw_step_guarded", param, grad, exp_avg, exp_avg_sq, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
           weight_decay=weight_decay, step=step, grad_scale=grad_scale, lowp=lowp, guard=guard)


def adamw_step_groups(param, grad, exp_avg, exp_avg_sq, quad_group, group_tab, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, step,
                      grad_scale=1.0, lowp=None, guard=None):
    """adamw_step (guard None) / adamw_step_guarded with a learning-rate scale and a weight decay per group (csrc/optim.hip):
    quad_group, uint8, one id per 16-byte chunk of param (ceil(n / 4) entries); group_tab, fp32 (n_groups, 2) rows
    {lr_scale, weight_decay}.  A maximal segment of equal id gets the bits of adamw_step[_guarded] on that segment alone with
    lr = float32(lr) * float32(lr_scale) and that decay; a chunk whose id has no row is not touched."""
    if quad_group is None or group_tab is None:
        raise ValueError("adamw_step_groups: quad_group and group_tab are required")
    _adamw("adamw_step_groups", param, grad, exp_avg, exp_avg_sq, lr=lr, beta1=beta1, beta2=beta2, eps=eps, step=step,
           grad_scale=grad_scale, lowp=lowp, guard=guard, quad_group=quad_group, group_tab=group_tab)


class GradGuard:
    """The device state of one trainer's gradient guard: the fp64 sum, the partials workspace (sized once for `numel`
    elements: it serves any run of at most that many), guard = {coefficient, norm, skip flag, 0} and the cumulative
    counters {skipped, clipped}.  max_norm <= 0: no clipping (the coefficient is exactly 1)."""

    def __init__(self, numel: int, device, max_norm: float = 0.0, skip_nonfinite: bool = False):
        self.max_norm, self.skip_nonfinite = float(max_norm), bool(skip_nonfinite)
        self.acc = torch.zeros(1, dtype=torch.float64, device=device)
        self.workspace = torch.empty(grad_sqnorm_workspace_bytes(numel) // 8, dtype=torch.float64, device=device)
        self.guard = torch.zeros(4, dtype=torch.float32, device=device)
        self.counters = torch.zeros(2, dtype=torch.int64, device=device)

    def decide(self, runs, pre_scale: float = 1.0):
        """One decision from the gradient runs (flat fp32 tensors, 16-byte aligned): a sum-of-squares pass per run, then
        the finalize launch.  No host synchronisation."""
        if not runs:
            self.acc.zero_()            # (no gradient at all: norm 0, nothing clipped, nothing skipped)
        for k, g in enumerate(runs):
            grad_sqnorm(g, self.acc, self.workspace, accumulate=k > 0)
        grad_guard_finalize(self.acc, self.guard, self.counters, pre_scale=pre_scale, max_norm=self.max_norm,
                            skip_nonfinite=self.skip_nonfinite)
        return self.guard

    def state(self) -> dict:
        """For a checkpoint: the cumulative counters {skipped, clipped} and the last decision (what grad_guard_stats reads);
        the sum and the workspace are rewritten by every decision."""
        return {"counters": self.counters.detach().cpu(), "guard": self.guard.detach().cpu()}

    def load_state(self, state: dict) -> None:
        self.counters.copy_(state["counters"])
        self.guard.copy_(state["guard"])


# ---- weight EMA (csrc/optim.hip): a shadow of the parameter arena moved towards the live parameters -----------------------
def ema_update(ema, param, weight: float, guard=None):
    """ema += weight * (param - ema) in place, fp32, lerp form (ema == param is a bitwise fixed point); param is not written.
    guard (ops.GradGuard.guard or None): nothing is written when guard[2] != 0.  Alignment, the weight's range [0, 1], empty
    and aliased operands are checked by the entry point (RuntimeError through `check`, nothing launched)."""
    _need_gpu(ema, param, guard)
    for name, t in (("ema", ema), ("param", param), ("guard", guard)):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise TypeError("ema_update: %s must be float32 (got %s)" % (name, t.dtype))
        if not t.is_contiguous():
            raise ValueError("ema_update: %s must be contiguous" % name)
        if t.device != ema.device:
            raise ValueError("ema_update: %s is on %s, ema on %s" % (name, t.device, ema.device))
    if ema.numel() != param.numel():
        raise ValueError("ema_update: ema has %d elements, param %d" % (ema.numel(), param.numel()))
    if guard is not None and guard.numel() < 4:
        raise ValueError("ema_update: guard must hold 4 floats (got %d)" % guard.numel())
    check(_lib.lib().dl_ema_update(ema.data_ptr(), param.data_ptr(), ema.numel(), float(weight), _ptr(guard), _stream()),
          "dl_ema_update")


def cos_rowloss_fwd(x, y):
    n, D = x.shape
    row = torch.empty(n, dtype=torch.float32, device=x.device)
    check(_lib.lib().dl_cos_rowloss_fwd(x.data_ptr(), y.data_ptr(), row.data_ptr(), None, n, D, _stream()),
          "dl_cos_rowloss_fwd")
    return row


def cos_rowloss_bwd(x, y, grad_scale: float):
    n, D = x.shape
    dx = torch.empty_like(x)
    check(_lib.lib().dl_cos_rowloss_bwd(x.data_ptr(), y.data_ptr(), float(grad_scale), dx.data_ptr(), n, D, _stream()),
          "dl_cos_rowloss_bwd")
    return dx


def ntxent_fwd(q, k, temperature: float):
    n, d = q.shape
    L = _lib.lib()
    loss = torch.empty(1, dtype=torch.float32, device=q.device)
    lse = torch.empty(2 * n, dtype=torch.float32, device=q.device)
    ws = _ws.get(L.dl_ntxent_workspace_bytes(n, d), q.device)
    check(L.dl_ntxent_fwd(q.data_ptr(), k.data_ptr(), n, d, float(temperature), loss.data_ptr(), lse.data_ptr(),
                          ws.data_ptr(), ws.numel(), _stream()), "dl_ntxent_fwd")
    return loss, lse


def ntxent_bwd(q, k, temperature: float, lse, grad_out: float):
    n, d = q.shape
    dq, dk = torch.empty_like(q), torch.empty_like(k)
    check(_lib.lib().dl_ntxent_bwd(q.data_ptr(), k.data_ptr(), n, d, float(temperature), lse.data_ptr(),
                                   float(grad_out), dq.data_ptr(), dk.data_ptr(), _stream()), "dl_ntxent_bwd")
    return dq, dk


def _ntx_args(aq, ak, bq, bk, off_a, off_b, n_global, temperature, lse_a=None, lse_b=None):
    _need_gpu(aq, ak, bq, bk)
    assert aq.dtype == ak.dtype == bq.dtype == bk.dtype and aq.dtype in (torch.float32, torch.bfloat16)
    assert aq.is_contiguous() and ak.is_contiguous() and bq.is_contiguous() and bk.is_contiguous()
    assert aq.shape == ak.shape and bq.shape == bk.shape and aq.shape[1] == bq.shape[1]
    a = _lib.NtxentArgs()
    a.a.q, a.a.k, a.a.n, a.a.gid_offset = aq.data_ptr(), ak.data_ptr(), aq.shape[0], int(off_a)
    a.b.q, a.b.k, a.b.n, a.b.gid_offset = bq.data_ptr(), bk.data_ptr(), bq.shape[0], int(off_b)
    a.a.lse = lse_a.data_ptr() if lse_a is not None else None
    a.b.lse = lse_b.data_ptr() if lse_b is not None else None
    a.n_global, a.d, a.dtype, a.temperature = int(n_global), aq.shape[1], _dt(aq), float(temperature)
    return a


def ntxent_fwd_ex(aq, ak, bq, bk, off_a: int, off_b: int, n_global: int, temperature: float):
    """Rows [aq; ak] scored against rows [bq; bk] (dl_ntxent_fwd_ex): returns (mean row loss (1,), row_lse (2 n_a,),
    row_loss (2 n_a,)), all fp32."""
    a = _ntx_args(aq, ak, bq, bk, off_a, off_b, n_global, temperature)
    n2 = 2 * aq.shape[0]
    loss = torch.empty(1, dtype=torch.float32, device=aq.device)
    lse = torch.empty(n2, dtype=torch.float32, device=aq.device)
    row_loss = torch.empty(n2, dtype=torch.float32, device=aq.device)
    check(_lib.lib().dl_ntxent_fwd_ex(a, lse.data_ptr(), row_loss.data_ptr(), loss.data_ptr(), _stream()), "dl_ntxent_fwd_ex")
    return loss, lse, row_loss


def ntxent_bwd_ex(aq, ak, bq, bk, off_a: int, off_b: int, n_global: int, temperature: float, lse_a, lse_b, grad_scale: float):
    """Gradient with respect to the rows [aq; ak] (dl_ntxent_bwd_ex), fp32."""
    a = _ntx_args(aq, ak, bq, bk, off_a, off_b, n_global, temperature, lse_a, lse_b)
    da_q = torch.empty(aq.shape, dtype=torch.float32, device=aq.device)
    da_k = torch.empty(ak.shape, dtype=torch.float32, device=aq.device)
    check(_lib.lib().dl_ntxent_bwd_ex(a, float(grad_scale), da_q.data_ptr(), da_k.data_ptr(), _stream()), "dl_ntxent_bwd_ex")
    return da_q, da_k


LATENT_DIM = 256          # row width of dl_latent_topk
LATENT_TOPK_MAX = 1024    # its largest M


def latent_topk(q, lib, M: int, slab: Optional[int] = None):
    """For every row of q (P, 256) the M rows of lib (D, 256) with the largest dot product (dl_latent_topk): (values (P, M)
    fp32, indices (P, M) int64), value descending, equal values by ascending index, NaN first as in torch.topk.  q and lib both
    fp32 or both bf16, contiguous; nothing is normalised.  slab (tests): library rows per workgroup pass, a multiple of 64 —
    the result does not depend on it.  Stream-ordered, no host synchronisation.  Bad arguments raise ValueError."""
    _need_gpu(q, lib)
    if q.dim() != 2 or lib.dim() != 2 or q.shape[1] != LATENT_DIM or lib.shape[1] != LATENT_DIM:
        raise ValueError("latent_topk: q and lib must be (rows, %d) (got %s and %s)" % (LATENT_DIM, tuple(q.shape), tuple(lib.shape)))
    if q.dtype != lib.dtype or q.dtype not in _DT:
        raise ValueError("latent_topk: q and lib must both be float32 or both bfloat16 (got %s and %s)" % (q.dtype, lib.dtype))
    if not (q.is_contiguous() and lib.is_contiguous()):
        raise ValueError("latent_topk: q and lib must be contiguous")
    P, D, M = q.shape[0], lib.shape[0], int(M)
    if P < 1 or not 1 <= M <= min(D, LATENT_TOPK_MAX) or D >= 1 << 31:
        raise ValueError("latent_topk: needs P >= 1, D < 2^31 and 1 <= M <= min(D, %d) (got P %d, D %d, M %d)" % (LATENT_TOPK_MAX, P, D, M))
    if slab is not None and (int(slab) < 64 or int(slab) % 64):
        raise ValueError("latent_topk: slab must be a positive multiple of 64 (got %s)" % (slab,))
    slab = 0 if slab is None else int(slab)          # 0: the host's choice
    L = _lib.lib()
    values = torch.empty((P, M), dtype=torch.float32, device=q.device)
    indices = torch.empty((P, M), dtype=torch.int32, device=q.device)
    ws = _ws.get(L.dl_latent_topk_workspace_bytes(P, D, M, slab), q.device)
    rc = L.dl_latent_topk(q.data_ptr(), lib.data_ptr(), P, D, M, _dt(q), slab, values.data_ptr(), indices.data_ptr(),
                          _stream(), ws.data_ptr(), ws.numel())
    if rc in (-1, -2, -3):            # DL_ERR_ARG / _SHAPE / _ALIGN: the caller's arguments
        raise ValueError("latent_topk: %s" % L.dl_last_error().decode())
    check(rc, "dl_latent_topk")
    return values, indices.to(torch.int64)


def triplet_sigcos_fwd(p_lats, d_lats, gt_i8, margin: float):
    n_p, dim = p_lats.shape
    n_d = d_lats.shape[0]
    L = _lib.lib()
    buf = torch.empty(L.dl_triplet_sigcos_buffer_floats(n_p, n_d), dtype=torch.float32, device=p_lats.device)
    loss = torch.empty(1, dtype=torch.float32, device=p_lats.device)
    ntri = torch.empty(1, dtype=torch.float32, device=p_lats.device)
    check(L.dl_triplet_sigcos_fwd(p_lats.data_ptr(), d_lats.data_ptr(), gt_i8.data_ptr(), n_p, n_d, dim, float(margin),
                                  buf.data_ptr(), loss.data_ptr(), ntri.data_ptr(), _stream()), "dl_triplet_sigcos_fwd")
    return loss, ntri, buf


def triplet_sigcos_bwd(p_lats, d_lats, gt_i8, margin: float, buf, ntri, grad_out: float):
    n_p, dim = p_lats.shape
    n_d = d_lats.shape[0]
    dp, dd = torch.empty_like(p_lats), torch.empty_like(d_lats)
    check(_lib.lib().dl_triplet_sigcos_bwd(p_lats.data_ptr(), d_lats.data_ptr(), gt_i8.data_ptr(), buf.data_ptr(), n_p,
                                           n_d, dim, float(margin), ntri.data_ptr(), float(grad_out), dp.data_ptr(),
                                           dd.data_ptr(), _stream()), "dl_triplet_sigcos_bwd")
    return dp, dd


def _bn_entry(name, rw, win, halo, valid):
    """(C function, its name, its row-rule arguments): rw (R,) fp32 row weights (< 0 halo, 0 context, m >= 1 multiplicity) go to
    dl_<name>_rw as `row_w`, exactly where dl_<name> takes the window rule `win, halo, valid`."""
    name, rows = (name + "_rw", (rw.data_ptr(),)) if rw is not None else (name, (win, halo, valid))
    return getattr(_lib.lib(), name), name, rows


def _bn_sums_ws(y2d):
    """(sums [2C] fp32, the workspace of the partial-sum kernels) for a column reduction over y2d."""
    R, Cc = y2d.shape
    sums = torch.empty(2 * Cc, dtype=torch.float32, device=y2d.device)
    return sums, _ws2.get(_lib.lib().dl_bn_workspace_bytes(R, Cc), y2d.device)


def bn_stats(y2d, win, halo, valid, rw=None):
    R, Cc = y2d.shape
    fn, name, rows = _bn_entry("dl_bn_stats", rw, win, halo, valid)
    sums, ws = _bn_sums_ws(y2d)
    check(fn(y2d.data_ptr(), R, Cc, *rows, _dt(y2d), sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), name)
    return sums


def bn_stats_finalize(y2d, win, halo, valid, n, eps, momentum=0.0, running_mean=None, running_var=None, rw=None):
    """bn_stats + bn_finalize in two launches instead of three (dl_bn_stats_finalize): (mean, biased var, rstd), bit-identical."""
    R, Cc = y2d.shape
    L = _lib.lib()
    out = torch.empty((3, Cc), dtype=torch.float32, device=y2d.device)
    ws = _ws2.get(L.dl_bn_workspace_bytes(R, Cc), y2d.device)
    check(L.dl_bn_stats_finalize(y2d.data_ptr(), R, Cc, win, halo, valid, _ptr(rw), _dt(y2d), int(n), float(eps), float(momentum), None,
                                 out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _ptr(running_mean), _ptr(running_var),
                                 ws.data_ptr(), ws.numel(), _stream()), "dl_bn_stats_finalize")
    return out[0], out[1], out[2]


def bn_finalize(sums, n, eps, momentum=0.0, running_mean=None, running_var=None):
    """(mean, biased var, rstd) from dl_bn_stats sums; updates the running statistics in place when given."""
    Cc = sums.numel() // 2
    out = torch.empty((3, Cc), dtype=torch.float32, device=sums.device)
    check(_lib.lib().dl_bn_finalize(sums.data_ptr(), int(n), float(eps), float(momentum), out[0].data_ptr(), out[1].data_ptr(),
                                    out[2].data_ptr(), _ptr(running_mean), _ptr(running_var), Cc, _stream()), "dl_bn_finalize")
    return out[0], out[1], out[2]


def bn_apply_fwd(y2d, mean, rstd, gamma, beta, win, halo, valid, rw=None):
    R, Cc = y2d.shape
    fn, name, rows = _bn_entry("dl_bn_apply_fwd", rw, win, halo, valid)
    z = torch.empty_like(y2d)
    check(fn(y2d.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), R, Cc, *rows, _dt(y2d),
             _stream()), name)
    return z


def bn_bwd_reduce(dz2d, y2d, mean, rstd, win, halo, valid, rw=None):
    R, Cc = y2d.shape
    fn, name, rows = _bn_entry("dl_bn_bwd_reduce", rw, win, halo, valid)
    sums, ws = _bn_sums_ws(y2d)
    check(fn(dz2d.data_ptr(), y2d.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, Cc, *rows, _dt(y2d), sums.data_ptr(), ws.data_ptr(),
             ws.numel(), _stream()), name)
    return sums


def bn_bwd_apply(dz2d, y2d, mean, rstd, gamma, sums, inv_n, relu_mask, win, halo, valid, rw=None):
    R, Cc = y2d.shape
    fn, name, rows = _bn_entry("dl_bn_bwd_apply", rw, win, halo, valid)
    dy = torch.empty_like(y2d)
    check(fn(dz2d.data_ptr(), y2d.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), sums.data_ptr(), float(inv_n),
             int(relu_mask), dy.data_ptr(), R, Cc, *rows, _dt(y2d), _stream()), name)
    return dy


def bn_apply_relu_fwd(y2d, mean, rstd, gamma, beta):
    """z = max(0, BN(y)) (dl_bn_apply_relu_fwd)."""
    R, Cc = y2d.shape
    z = torch.empty_like(y2d)
    check(_lib.lib().dl_bn_apply_relu_fwd(y2d.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                          R, Cc, _dt(y2d), _stream()), "dl_bn_apply_relu_fwd")
    return z


def bn_relu_bwd(dz2d, y2d, mean, rstd, gamma, beta, inv_n):
    """Backward of z = max(0, BN(y)): (dy, sums [2C] = (d beta | d gamma)) (dl_bn_relu_bwd)."""
    R, Cc = y2d.shape
    dy = torch.empty_like(y2d)
    sums, ws = _bn_sums_ws(y2d)
    check(_lib.lib().dl_bn_relu_bwd(dz2d.data_ptr(), y2d.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                    float(inv_n), dy.data_ptr(), sums.data_ptr(), R, Cc, _dt(y2d), ws.data_ptr(), ws.numel(), _stream()),
          "dl_bn_relu_bwd")
    return dy, sums


def bn_eval_bwd(dz, y, mean, rstd, gamma, beta=None, *, relu_in=False, relu_out=False, win=0, halo=0, valid=0, row_w=None,
                want_sums=True):
    """Backward of a BatchNorm on fixed statistics (eval mode) in one pass (dl_bn_eval_bwd): (dx, sums [2C] = (d beta | d gamma) or
    None).  relu_out: a ReLU behind the BatchNorm (needs beta); relu_in: y is the output of a ReLU in front of it; row_w < 0
    marks excluded rows and is otherwise not applied (a compact row's dz already is the sum over the rows it stands for)."""
    R, Cc = y.shape
    if relu_out and beta is None:
        raise ValueError("bn_eval_bwd: relu_out needs beta")
    dx = torch.empty_like(y)
    sums, ws = _bn_sums_ws(y) if want_sums else (None, None)
    check(_lib.lib().dl_bn_eval_bwd(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                    _ptr(beta) if relu_out else None, int(relu_in), int(relu_out), dx.data_ptr(), _ptr(sums), R, Cc, int(win),
                                    int(halo), int(valid), _ptr(row_w), _dt(y), _ptr(ws), ws.numel() if ws is not None else 0, _stream()),
          "dl_bn_eval_bwd")
    return dx, sums


def bn_tail_fix(dy2d, y2d, mean, rstd, gamma, sums, inv_n, w, win, lead):
    """In place: the tail rows of every `win`-row window take the mean terms of the BatchNorm backward w times (dl_bn_tail_fix)."""
    R, Cc = y2d.shape
    check(_lib.lib().dl_bn_tail_fix(dy2d.data_ptr(), y2d.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                    sums.data_ptr(), float(inv_n), int(w), R, Cc, int(win), int(lead), _dt(y2d), _stream()),
          "dl_bn_tail_fix")
    return dy2d


def ce_rows_fwd(logits2d, labels, C: int, ignore_index: int):
    """Cross entropy over the first C columns of logits2d (N, >= C) (dl_ce_rows_fwd): (out2 = [mean loss, counted rows], lse (N,))."""
    _need_gpu(logits2d, labels)
    N, ld = logits2d.shape[0], logits2d.stride(0)
    L = _lib.lib()
    lse = torch.empty(N, dtype=torch.float32, device=logits2d.device)
    out2 = torch.empty(2, dtype=torch.float32, device=logits2d.device)
    ws = _ws2.get(L.dl_ce_rows_workspace_bytes(N), logits2d.device)
    check(L.dl_ce_rows_fwd(logits2d.data_ptr(), ld, labels.data_ptr(), N, C, int(ignore_index), _dt(logits2d), lse.data_ptr(),
                           out2.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "dl_ce_rows_fwd")
    return out2, lse


def ce_rows_bwd(logits2d, labels, C: int, ignore_index: int, lse, out2, grad_out):
    """d(mean loss) / d logits, (N, width of logits2d): zeros in the columns >= C and in ignored rows (dl_ce_rows_bwd)."""
    N, Cp = logits2d.shape
    d = torch.empty((N, Cp), dtype=logits2d.dtype, device=logits2d.device)
    check(_lib.lib().dl_ce_rows_bwd(logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), N, C, int(ignore_index), _dt(logits2d),
                                    lse.data_ptr(), out2.data_ptr(), grad_out.data_ptr(), d.data_ptr(), Cp, Cp, _stream()), "dl_ce_rows_bwd")
    return d


def _cls_loss_operands(score2d, labels, weights, who):
    _need_gpu(score2d, labels, weights)
    if score2d.dim() != 2 or score2d.shape[1] not in (1, 2) or score2d.stride(1) != 1:
        raise ValueError("%s: score must be (N, 1) or (N, 2) with unit column stride (got %s, strides %s)"
                         % (who, tuple(score2d.shape), tuple(score2d.stride())))
    N = score2d.shape[0]
    for name, t in (("labels", labels), ("weights", weights)):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.shape != (N,) or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous float32 (%d,) tensor (got %s %s)" % (who, name, N, t.dtype, tuple(t.shape)))
    return N, score2d.stride(0) if N > 1 else max(score2d.stride(0), score2d.shape[1])


def cls_loss_fwd(score2d, labels, weights, a_pos: float, a_neg: float, gamma: float):
    """Weighted / focal BCE on the logits score2d (N, 1 | 2) (dl_cls_loss_fwd): (out2 = [loss, den], probs (N,) fp32 = sigmoid(z)).
    labels fp32 (N,), weights fp32 (N,) or None.  A non-finite score, a label outside [0, 1] and a negative or non-finite weight make the
    loss NaN; the last two also raise FLAG_CLS_LABEL in the loss's device guard word (cls_loss_flags; check_guard_flags reports it)."""
    N, ld = _cls_loss_operands(score2d, labels, weights, "cls_loss_fwd")
    L = _lib.lib()
    dev = score2d.device
    probs = torch.empty(N, dtype=torch.float32, device=dev)
    out2 = torch.empty(2, dtype=torch.float32, device=dev)
    nws = L.dl_cls_loss_workspace_bytes(N)
    ws = _ws2.get(nws, dev) if nws else None             # (the one-workgroup form takes none)
    check(L.dl_cls_loss_fwd(score2d.data_ptr(), ld, score2d.shape[1], _dt(score2d), labels.data_ptr(), _ptr(weights), N, float(a_pos),
                            float(a_neg), float(gamma), probs.data_ptr(), out2.data_ptr(), _ptr(ws), ws.numel() if ws is not None else 0,
                            FLAG_CLS_LABEL, cls_loss_flags(dev).data_ptr(), _stream()), "dl_cls_loss_fwd")
    return out2, probs


def cls_loss_bwd(score2d, labels, weights, a_pos: float, a_neg: float, gamma: float, out2, grad_out):
    """d loss / d score2d in score2d's dtype (dl_cls_loss_bwd); out2 from cls_loss_fwd, grad_out a device fp32 scalar."""
    N, ld = _cls_loss_operands(score2d, labels, weights, "cls_loss_bwd")
    d = torch.empty((N, score2d.shape[1]), dtype=score2d.dtype, device=score2d.device)
    check(_lib.lib().dl_cls_loss_bwd(score2d.data_ptr(), ld, score2d.shape[1], _dt(score2d), labels.data_ptr(), _ptr(weights), N,
                                     float(a_pos), float(a_neg), float(gamma), out2.data_ptr(), grad_out.data_ptr(), d.data_ptr(),
                                     score2d.shape[1], _stream()), "dl_cls_loss_bwd")
    return d


def gate_dpre(dl2d, w2, pre2d):
    """dpre = gelu'(pre) o (dl @ w2): dl (M, 8), w2 (8, d_diff), pre (M, d_diff), all in one compute dtype (dl_gate_dpre)."""
    _need_gpu(dl2d, w2, pre2d)
    M, H = dl2d.shape
    dd = pre2d.shape[1]
    out = torch.empty_like(pre2d)
    check(_lib.lib().dl_gate_dpre(dl2d.data_ptr(), w2.data_ptr(), pre2d.data_ptr(), out.data_ptr(), M, dd, H, _dt(pre2d), _stream()),
          "dl_gate_dpre")
    return out


def gelu_bwd(dy2d, pre2d):
    dx = torch.empty_like(dy2d)
    check(_lib.lib().dl_gelu_bwd(dy2d.data_ptr(), pre2d.data_ptr(), dx.data_ptr(), dy2d.numel(), _dt(dy2d), _stream()),
          "dl_gelu_bwd")
    return dx


def fill_pool(x: torch.Tensor, site_len: int, out_dtype: torch.dtype):
    """x (B, S, F) -> (fill (B, S) in x.dtype, pooled (B, S // site_len, ceil8(F + 1)) in out_dtype)."""
    _need_gpu(x)
    x = x.contiguous()
    B, S, F = x.shape
    Fp = (F + 1 + 7) // 8 * 8
    fill = torch.empty((B, S), dtype=x.dtype, device=x.device)
    pooled = torch.empty((B, S // site_len, Fp), dtype=out_dtype, device=x.device)
    check(_lib.lib().dl_fill_pool(x.data_ptr(), fill.data_ptr(), pooled.data_ptr(), B, S, F, site_len, _dt(x),
                                  _DT[out_dtype], _stream()), "dl_fill_pool")
    return fill, pooled


_weight_prep_launches = 0


def weight_prep_launches() -> int:
    """dl_weight_prep launches issued so far (GraphedStep checks that its capture recorded one)."""
    return _weight_prep_launches


def weight_prep(items_dev: torch.Tensor, block_map_dev: torch.Tensor, n_blocks: int, out_dtype: torch.dtype) -> None:
    """One launch over a device-side list of (fp32 master -> image) copies; see dl_weight_prep."""
    global _weight_prep_launches
    _need_gpu(items_dev, block_map_dev)
    _weight_prep_launches += 1
    check(_lib.lib().dl_weight_prep(items_dev.data_ptr(), block_map_dev.data_ptr(), int(n_blocks), _DT[out_dtype],
                                    _stream()), "dl_weight_prep")


def cnn_sitepool_fwd(z: torch.Tensor, L: int, halo: int, site_len: int) -> torch.Tensor:
    """z (B, L + 2*halo, C) channel-last -> pooled (B, L // site_len, C); see dl_cnn_sitepool_fwd."""
    _need_gpu(z)
    B, LP, C = z.shape
    out = torch.empty((B, L // site_len, C), dtype=z.dtype, device=z.device)
    check(_lib.lib().dl_cnn_sitepool_fwd(z.data_ptr(), out.data_ptr(), B, L, C, halo, site_len, _dt(z), _stream()),
          "dl_cnn_sitepool_fwd")
    return out


def cnn_sitepool_bwd(dpooled: torch.Tensor, L: int, halo: int, site_len: int) -> torch.Tensor:
    _need_gpu(dpooled)
    dpooled = dpooled.contiguous()
    B, _, C = dpooled.shape
    dz = torch.empty((B, L + 2 * halo, C), dtype=dpooled.dtype, device=dpooled.device)
    check(_lib.lib().dl_cnn_sitepool_bwd(dpooled.data_ptr(), dz.data_ptr(), B, L, C, halo, site_len, _dt(dpooled),
                                         _stream()), "dl_cnn_sitepool_bwd")
    return dz


def cnn_sitepool_rows_supported(L: int, site_len: int, C: int, dtype: torch.dtype) -> bool:
    """The shape rules of dl_cnn_sitepool_rows_fwd / _bwd (bf16; the forward's strip of site_len x 32 rows and the backward's
    image of one sample's pooled gradient must fit the 160 KB of LDS: 256 sites at 128 channels do, the 1024 sites of
    PROTEIN.SEQ_LEN 9216 do not — such shapes take the expansion + dense pooling kernels)."""
    if dtype != torch.bfloat16 or site_len <= 0 or L % site_len or C % 8 or site_len > C:
        return False
    n_site = L // site_len
    return n_site % 8 == 0 and site_len * C * 34 * 2 <= 160 * 1024 and (n_site + 2) * C * 2 + C * 16 + 16 * 1024 <= 160 * 1024


def cnn_sitepool_rows_fwd(z2d: torch.Tensor, row_of: torch.Tensor, B: int, L: int, site_len: int) -> torch.Tensor:
    """compact rows z2d (R, C) + position map -> pooled (B, L // site_len, C); see dl_cnn_sitepool_rows_fwd."""
    _need_gpu(z2d, row_of)
    z2d = z2d.contiguous()
    Cc = z2d.shape[1]
    out = torch.empty((B, L // site_len, Cc), dtype=z2d.dtype, device=z2d.device)
    check(_lib.lib().dl_cnn_sitepool_rows_fwd(z2d.data_ptr(), row_of.data_ptr(), out.data_ptr(), B, L, Cc, site_len, _dt(z2d), _stream()),
          "dl_cnn_sitepool_rows_fwd")
    return out


def cnn_sitepool_rows_bwd(dpooled: torch.Tensor, rep: torch.Tensor, row_of: torch.Tensor, L: int, site_len: int) -> torch.Tensor:
    _need_gpu(dpooled, rep, row_of)
    dpooled = dpooled.contiguous()
    B, _, Cc = dpooled.shape
    R = rep.shape[0]
    dz = torch.empty((R, Cc), dtype=dpooled.dtype, device=dpooled.device)
    check(_lib.lib().dl_cnn_sitepool_rows_bwd(dpooled.data_ptr(), rep.data_ptr(), row_of.data_ptr(), dz.data_ptr(), B, L, Cc, R, site_len,
                                              _dt(dpooled), _stream()), "dl_cnn_sitepool_rows_bwd")
    return dz


def embed_pad(ids: torch.Tensor, weight: torch.Tensor, fill: torch.Tensor, halo: int) -> torch.Tensor:
    """ids (B, L) int64, weight (V, D), fill (B, L) -> (B, L + 2*halo, D + 1); see dl_embed_pad."""
    _need_gpu(ids, weight, fill)
    B, L = ids.shape
    V, D = weight.shape
    ids = ids.contiguous()
    weight = torch.nn.functional.pad(weight, (0, 1)).contiguous()      # [V][D + 1]: 16-byte aligned table rows
    fill = fill.to(weight.dtype).contiguous()
    out = torch.empty((B, L + 2 * halo, D + 1), dtype=weight.dtype, device=weight.device)
    check(_lib.lib().dl_embed_pad(ids.data_ptr(), weight.data_ptr(), fill.data_ptr(), out.data_ptr(), B, L, V, D, halo,
                                  _dt(weight), _stream()), "dl_embed_pad")
    return out


# Device-side guard flags (dl_embed_rows / dl_rows_equal_check OR sticky bits into one int32 word per device): the compact
# padding forms are only valid for inputs with the padding structure of the reference's collate; Trainer polls the word.
_guard_flags = {}
FLAG_TEXT = {_lib.FLAG_PROT_PERIOD: "a protein's residue codes / fill bits are not tiled with the period its length gives "
                                    "(utils.py:392-412 repeat_integer_label_protein); disable with DL_CNN_COMPACT=0",
             _lib.FLAG_DRUG_TOKEN_PAD: "drug LLM token rows beyond the hinted block (meta 'Drug_Tokens') are not identical padding rows; "
                                       "disable with DL_PAD_COMPACT=0",
             _lib.FLAG_GCN_NODE_PAD: "drug graph nodes beyond the adjacency block are not identical virtual padding nodes "
                                     "(handler/dataset.py:216-221); disable with DL_GCN_COMPACT=0",
             _lib.FLAG_PLAN_ROWS: "the ProteinCNN row tables were built with fewer rows than the batch's residue counts need "
                                  "(dl_protein_plan_build capacity)",
             _lib.FLAG_PAIR_INDEX: "a (protein, drug) pair of a screening launch names an entity outside the cached codes; the pair "
                                   "was skipped (dl_pgca_pairs_fwd)",
             _lib.FLAG_KEY_TABLE: "a drug's entry of a library screening launch's key table does not describe rows inside the row store "
                                  "(negative first row, fewer keys than the tail, rows past the end, or a weight that is not a finite "
                                  "value >= 1); the pair was skipped (dl_pgca_pairs_ragged_fwd)",
             _lib.FLAG_MAP_COLS: "a drug's attention map of a pair-map launch does not fit the columns it was given, or its keys' "
                                 "multiplicity cannot be expanded (not a whole number <= 2^24); the pair was skipped (dl_pgca_pairs_probs)"}


def guard_flags(device) -> torch.Tensor:
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else (torch.cuda.current_device() if dev.type == "cuda" else 0))
    t = _guard_flags.get(key)
    if t is None:
        t = _guard_flags[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def guard_text(bits: int) -> str:
    return "; ".join(v for k, v in FLAG_TEXT.items() if bits & k) or "unknown flag bits %#x" % bits


# The classification loss's own word (dl_cls_loss_fwd ORs FLAG_CLS_LABEL into it): the word above is the padding guards', and a
# bad label is no padding fault.  One int32 per device, created by the first cls_loss_fwd on it: without the loss it does not
# exist and nothing reads it.  check_guard_flags and the trainer's polling report both words.
FLAG_CLS_LABEL = 1
CLS_FLAG_TEXT = {FLAG_CLS_LABEL: "FLAG_CLS_LABEL: a label of the classification loss is outside [0, 1] or not finite, or a sample weight "
                                 "(meta 'Weight') is negative or not finite; that sample's loss and gradient are NaN (dl_cls_loss_fwd)"}
_cls_flags = {}


def _dev_key(device):
    dev = torch.device(device)
    return dev, (dev.type, dev.index if dev.index is not None else (torch.cuda.current_device() if dev.type == "cuda" else 0))


def cls_loss_flags(device, create: bool = True) -> Optional[torch.Tensor]:
    """The classification loss's guard word of `device` (create=False: None while no cls_loss_fwd has run there)."""
    dev, key = _dev_key(device)
    t = _cls_flags.get(key)
    if t is None and create:
        t = _cls_flags[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def guard_message(bits: int, cls_bits: int = 0, when: str = "") -> str:
    """The error text of tripped guard words (when: e.g. " in an earlier step")."""
    parts = []
    if bits:
        parts.append("padding guard tripped%s — %s" % (when, guard_text(bits)))
    if cls_bits:
        parts.append("classification loss guard tripped%s — %s"
                     % (when, "; ".join(v for k, v in CLS_FLAG_TEXT.items() if cls_bits & k) or "unknown flag bits %#x" % cls_bits))
    return "druglamp_amd: " + "; ".join(parts)


def check_guard_flags(device) -> None:
    """Synchronising check of the device guard words: raises (and clears them) when a compact padding form ran on a batch
    that does not have the structure it assumes, or the classification loss met a bad label or sample weight."""
    t = guard_flags(device)
    bits = int(t.item())
    c = cls_loss_flags(device, create=False)
    cls_bits = int(c.item()) if c is not None else 0
    if bits or cls_bits:
        t.zero_()
        if c is not None:
            c.zero_()
        raise RuntimeError(guard_message(bits, cls_bits))


def embed_rows(ids: torch.Tensor, weight: torch.Tensor, fill: torch.Tensor, src: torch.Tensor, period: Optional[torch.Tensor]) -> torch.Tensor:
    """Compact ProteinCNN input (dl_embed_rows): ids (B, L) int64, weight (V, D), fill (B, L), src (R,) int32 flat indices or -1
    -> (R, D + 1).  period (B,) int32: also run the periodicity guard (sets the device guard word on a violation)."""
    _need_gpu(ids, weight, fill, src)
    B, L = ids.shape
    V, D = weight.shape
    ids = ids.contiguous()
    weight = torch.nn.functional.pad(weight, (0, 1)).contiguous()
    fill = fill.to(weight.dtype).contiguous()
    R = src.numel()
    out = torch.empty((R, D + 1), dtype=weight.dtype, device=weight.device)
    flags = guard_flags(weight.device) if period is not None else None
    check(_lib.lib().dl_embed_rows(ids.data_ptr(), weight.data_ptr(), fill.data_ptr(), src.data_ptr(), out.data_ptr(), R, V, D,
                                   _ptr(period), B, L, _ptr(flags), _dt(weight), _stream()), "dl_embed_rows")
    return out


def protein_plan_build(pd) -> None:
    """The ProteinCNN distinct-row tables of protein_plan.PlanDev `pd` from its residue counts `pd.len_dev`, on the device
    (dl_protein_plan_build, current stream); a capacity overflow sets the device guard word."""
    _need_gpu(pd.buf)
    check(_lib.lib().dl_protein_plan_build(pd.len_dev.data_ptr(), pd.B, pd.S, pd.rows, pd.src.data_ptr(), pd.w.data_ptr(),
                                           pd.rep.data_ptr(), pd.row_of.data_ptr(), pd.period.data_ptr(),
                                           guard_flags(pd.buf.device).data_ptr(), _stream()), "dl_protein_plan_build")


def rows_gather(src2d: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """out[i] = src2d[index[i]] (zeros where index[i] < 0); index int32 (dl_rows_gather)."""
    _need_gpu(src2d, index)
    src2d = src2d.contiguous()
    N, Cc = index.numel(), src2d.shape[1]
    out = torch.empty((N, Cc), dtype=src2d.dtype, device=src2d.device)
    check(_lib.lib().dl_rows_gather(src2d.data_ptr(), index.data_ptr(), out.data_ptr(), N, Cc * src2d.element_size(), _stream()),
          "dl_rows_gather")
    return out


def rows_sum_strided(x2d: torch.Tensor, rep: torch.Tensor) -> torch.Tensor:
    """out[r] = sum_{k < rep[r, 2]} x2d[rep[r, 0] + k * rep[r, 1]]; rep (R, 3) int32 (dl_rows_sum_strided)."""
    _need_gpu(x2d, rep)
    x2d = x2d.contiguous()
    R, Cc = rep.shape[0], x2d.shape[1]
    out = torch.empty((R, Cc), dtype=x2d.dtype, device=x2d.device)
    check(_lib.lib().dl_rows_sum_strided(x2d.data_ptr(), rep.data_ptr(), out.data_ptr(), R, Cc, _dt(x2d), _stream()),
          "dl_rows_sum_strided")
    return out


def rows_equal_check(x3d: torch.Tensor, row0: int, code: int) -> None:
    """Guard: rows row0.. of every sample of x3d (B, N, F) must equal row row0 of sample 0 (dl_rows_equal_check)."""
    _need_gpu(x3d)
    x3d = x3d.contiguous()
    B, N, F_ = x3d.shape
    check(_lib.lib().dl_rows_equal_check(x3d.data_ptr(), B, N, F_ * x3d.element_size(), int(row0), int(code),
                                         guard_flags(x3d.device).data_ptr(), _stream()), "dl_rows_equal_check")


def interleave_streams(x: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """x [S, ..., d] -> [..., S * d] (cat of the streams along the last dim); inverse: x [..., S * d] with S = 2 -> [2, ..., d]."""
    _need_gpu(x)
    x = x.contiguous()
    if not inverse:
        S, d = x.shape[0], x.shape[-1]
        R = x[0].numel() // d
        out = torch.empty(x.shape[1:-1] + (S * d,), dtype=x.dtype, device=x.device)
    else:
        S, d = 2, x.shape[-1] // 2
        R = x.numel() // (S * d)
        out = torch.empty((S,) + x.shape[:-1] + (d,), dtype=x.dtype, device=x.device)
    check(_lib.lib().dl_interleave_streams(x.data_ptr(), out.data_ptr(), R, d * x.element_size(), S, int(inverse), _stream()),
          "dl_interleave_streams")
    return out


def norm_adjacency(adj: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """(B, n, n) fp32 adjacency -> normalised, transposed adjacency in `dtype` (dl_norm_adjacency)."""
    _need_gpu(adj)
    adj = adj.contiguous()
    B, n, _ = adj.shape
    out = torch.empty((B, n, n), dtype=dtype, device=adj.device)
    check(_lib.lib().dl_norm_adjacency(adj.data_ptr(), out.data_ptr(), B, n, _DT[dtype], _stream()), "dl_norm_adjacency")
    return out


def graph_aggregate(ahat: torch.Tensor, feat: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """ahat (B, n, n), feat (B, N, C) -> (B, N, C): [A' @ feat[:, :n] ; feat[:, n:]] with A' = ahat or ahat^T (dl_graph_aggregate)."""
    _need_gpu(ahat, feat)
    ahat, feat = ahat.contiguous(), feat.contiguous()
    B, N, Cc = feat.shape
    out = torch.empty_like(feat)
    check(_lib.lib().dl_graph_aggregate(ahat.data_ptr(), feat.data_ptr(), out.data_ptr(), B, ahat.shape[-1], N, Cc, int(bool(transpose)),
                                        _dt(feat), _stream()), "dl_graph_aggregate")
    return out


def concat2(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """cat((a, b), -1) for two tensors with equal leading shape."""
    _need_gpu(a, b)
    a, b = a.contiguous(), b.contiguous()
    R = a.numel() // a.shape[-1]
    out = torch.empty(a.shape[:-1] + (a.shape[-1] + b.shape[-1],), dtype=a.dtype, device=a.device)
    check(_lib.lib().dl_concat2(a.data_ptr(), b.data_ptr(), out.data_ptr(), R, a.shape[-1] * a.element_size(),
                                b.shape[-1] * b.element_size(), 0, _stream()), "dl_concat2")
    return out


def split2(cat: torch.Tensor, wa: int):
    """inverse of concat2: (cat[..., :wa], cat[..., wa:]) as two contiguous tensors."""
    _need_gpu(cat)
    cat = cat.contiguous()
    wb = cat.shape[-1] - wa
    R = cat.numel() // cat.shape[-1]
    a = torch.empty(cat.shape[:-1] + (wa,), dtype=cat.dtype, device=cat.device)
    b = torch.empty(cat.shape[:-1] + (wb,), dtype=cat.dtype, device=cat.device)
    check(_lib.lib().dl_concat2(a.data_ptr(), b.data_ptr(), cat.data_ptr(), R, wa * cat.element_size(), wb * cat.element_size(),
                                1, _stream()), "dl_concat2")
    return a, b


def gather_pad(store: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, S: int, repeat: bool) -> torch.Tensor:
    """store (rows, F), offsets (B,) int64, lengths (B,) int32 -> (B, S, F); see dl_gather_pad."""
    _need_gpu(store, offsets, lengths)
    B, F = offsets.numel(), store.shape[1]
    out = torch.empty((B, S, F), dtype=store.dtype, device=store.device)
    check(_lib.lib().dl_gather_pad(store.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), out.data_ptr(), B, S, F,
                                   int(bool(repeat)), _dt(store), _stream()), "dl_gather_pad")
    return out
