"""fp64 reference of dl_gemm / dl_colsum (include/druglamp_hip.h), the dropout keep mask, and the magnitudes the rounding
bound of tests/test_gemm_paths_gpu.py multiplies.  Plain torch / numpy: runs on the CPU or on the device the operands live on.

The reference reads the kernel's own operands (bf16 / fp32 values are exact in fp64) straight from their storage, through the
same (layout, pitch) description the kernel gets, so overlapping rows (ldx < K) and pitch gaps are part of what is compared.
"""
import math

import numpy as np
import torch

F64 = torch.float64
SQRT1_2 = 0.70710678118654752440


# ---- operands ---------------------------------------------------------------------------------------------------------------
def operand(flat, rows, K, ld, kslow):
    """The logical [rows][K] operand in fp64.  flat: 1-D storage starting at the operand's base pointer.
    kslow == 0: element (r, k) at r * ld + k;  kslow == 1: element (r, k) at k * ld + r."""
    v = torch.as_strided(flat, (rows, K), (1, ld) if kslow else (ld, 1))
    return v.to(F64)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * SQRT1_2))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * SQRT1_2)) + x * torch.exp(-0.5 * x * x) * 0.39894228040143267794


# ---- dropout ------------------------------------------------------------------------------------------------------------------
def thr16(p):
    """round(p * 65536) as the fp32 host code forms it, limited to 16 bits."""
    t = np.float32(p) * np.float32(65536.0) + np.float32(0.5)
    return 0 if t <= 0 else (65535 if t >= 65535 else int(t))


def inv_keep(p):
    """1 / (1 - p) in fp32 (returned as a Python float holding the fp32 value)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _fmix32(h):
    h = h.copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def draws(seed, groups):
    """The 64-bit draw of every group index in `groups` (uint64 array): two murmur3 finalisers on 32-bit keys made of
    the low words' sum and the high words' xor (common.cuh, dl_splitmix)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = np.asarray(groups, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (g & np.uint64(0xFFFFFFFF)).astype(np.uint32) + np.uint32(seed & 0xFFFFFFFF)
        hi = (g >> np.uint64(32)).astype(np.uint32) ^ np.uint32(seed >> 32)
        a = _fmix32(x ^ hi)
        rot = (hi << np.uint32(13)) | (hi >> np.uint32(19))
        b = _fmix32((x + np.uint32(0x9E3779B9)) ^ rot ^ np.uint32(0x7F4A7C15))
    return (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)


def keep_mask(seed, seed_offset, M, N, p):
    """Boolean [M][N]: element (row, col) is kept iff the 16-bit field ((row * N + col) & 3) (lowest bits first) of the draw
    of group (row * N + col) >> 2, keyed by seed + seed_offset (mod 2^64), is >= thr16."""
    t = thr16(p)
    n = M * N
    bits = draws((int(seed) + int(seed_offset)) & 0xFFFFFFFFFFFFFFFF, np.arange((n + 3) // 4, dtype=np.uint64))
    sh = np.arange(4, dtype=np.uint64) * np.uint64(16)
    f = ((bits[:, None] >> sh[None, :]) & np.uint64(0xFFFF)).reshape(-1)[:n]
    return (f >= np.uint64(t)).reshape(M, N)


# ---- the product and its epilogue ---------------------------------------------------------------------------------------------
def reference(X, W, *, bias=None, act=0, dact_pre=None, residual=None, res_row_mod=0, res_before_dropout=False, keep=None,
              keep_scale=1.0, old_c=None, want_colsum=False):
    """X [M][K], W [N][K] fp64 (see `operand`).  Everything else is a logical fp64 tensor or None: bias [N], dact_pre [M][N],
    residual [M or res_row_mod][N], keep bool [M][N], old_c [M][N] (accumulate).
    Epilogue in the order of gemm_kernel's general path: bias, pre-activation copy, activation, x gelu'(dact_pre), residual
    before dropout, dropout, residual after dropout, + old C.  Returns a dict: acc, pre, C, S = sum_k |X||W|, and the
    magnitudes of the added terms."""
    M = X.shape[0]
    acc = X @ W.t()
    S = X.abs() @ W.abs().t()
    r = {"acc": acc, "S": S}
    pre = acc + bias[None, :] if bias is not None else acc
    r["pre"] = pre
    v = pre
    if act == 1:
        v = gelu(v)
    elif act == 2:
        v = torch.clamp_min(v, 0.0)
    r["act"] = v
    if dact_pre is not None:
        r["g"] = gelu_grad(dact_pre)
        v = v * r["g"]
    res = None
    if residual is not None:
        res = residual[torch.arange(M, device=X.device) % res_row_mod] if res_row_mod > 0 else residual
        r["res"] = res
        if res_before_dropout:
            v = v + res
    r["before_drop"] = v
    if keep is not None:
        v = torch.where(keep, v * keep_scale, torch.zeros_like(v))
    r["dropped"] = v
    if res is not None and not res_before_dropout:
        v = v + res
    r["before_acc"] = v
    if old_c is not None:
        v = v + old_c
    r["C"] = v
    if want_colsum:
        r["x_colsum"] = X.sum(dim=1)
        r["x_colsum_mag"] = X.abs().sum(dim=1)
    return r


def colsum(X, old=None):
    """dl_colsum: out[n] (+)= sum_m X[m][n]; returns (sum, sum of magnitudes)."""
    s = X.sum(dim=0)
    return (s + old if old is not None else s), X.abs().sum(dim=0) + (old.abs() if old is not None else 0.0)


# ---- host dispatch, mirrored (csrc/gemm.hip) ----------------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def es_of(bf16):
    return 2 if bf16 else 4


def plain(c):
    return not (c.bias or c.res or c.act or c.pre or c.dact or c.p > 0.0)


def pick_epi(c, split):
    epi = 1
    if (not split and c.N % 8 == 0 and not c.acc and c.rmod == 0 and not (c.res == "before")):
        drop = thr16(c.p) != 0 if c.p > 0 else False
        res = c.res is not None
        if not res and not c.act and not c.pre and not c.dact and not drop:
            epi = 0
        elif c.act == 1 and c.pre and not res and not c.dact:
            epi = 2
        elif res and not c.act and not c.pre and not c.dact:
            epi = 3
        elif c.dact and not res and not c.act and not c.pre and not c.bias:
            epi = 4
        elif c.act == 2 and not res and not c.pre and not c.dact and not drop:
            epi = 5
    return epi


def pick_tw(c):
    if c.xs and c.ws and c.split >= 0:
        tiles128 = _cdiv(c.M, 128) * _cdiv(c.N, 128)
        if tiles128 <= 4 and c.M >= 64 and c.N >= 64 and c.K % (128 // es_of(c.bf_in)) == 0:
            return 2
    return 4


def auto_split(M, N, K, bke, bt):
    tiles = _cdiv(M, bt) * _cdiv(N, bt)
    if tiles >= 192:
        return 1
    want = max(512 // tiles, 1)
    maxs = max(_cdiv(K, bke) // 4, 1)
    return max(min(want, maxs, 256), 1)


def trim_splits(K, step, sp):
    ksteps = _cdiv(K, step)
    sp = max(min(sp, ksteps), 1)
    per = _cdiv(ksteps, sp)
    return _cdiv(ksteps, per)


def big_tt_plan(c):
    """(slabs before trimming, tile rows) or (0, 0)."""
    if c.algo == 1 or not c.bf_in or not c.xs or not c.ws or c.split != 0:
        return 0, 0
    if not plain(c) or c.M % 8 or c.N % 8 or c.N < 192 or c.M < 96 or c.K < 4096:
        return 0, 0
    big = c.M > 128 and c.M * c.N >= 640 * 1024
    bm = 256 if big else 128
    if not big:
        work = float(c.M) * float(c.N) * float(c.K)
        if (work < 1.0e10) if c.M > 128 else (c.N < 640 or c.K < 262144):
            return 0, 0
    tiles = _cdiv(c.M, bm) * _cdiv(c.N, 256)
    if tiles > 256:
        return 0, 0
    sp = max(min(256 // tiles, _cdiv(c.K, 64) // 4), 1)
    return sp, bm


def resolve_split(c):
    sp, _ = big_tt_plan(c)
    if sp > 0:
        return trim_splits(c.K, 64, sp)
    bke = 128 // es_of(c.bf_in)
    if c.split > 0:
        return trim_splits(c.K, bke, c.split)
    if c.split < 0:
        return 1
    ok = plain(c) and not c.bf_out and c.N % 4 == 0
    return trim_splits(c.K, bke, auto_split(c.M, c.N, c.K, bke, 32 * pick_tw(c))) if ok else 1


def _large_common(c, sp):
    if c.algo == 1:
        return False
    if sp > 1 or not c.bf_in or not c.bf_out or c.xs or c.ws:
        return False
    return pick_epi(c, False) != 1 and c.K % 64 == 0


def big_eligible(c, sp):
    if not _large_common(c, sp) or c.N <= 128:
        return False
    return _cdiv(c.M, 256) * _cdiv(c.N, 256) >= 192


def lat_eligible(c, sp):
    if not _large_common(c, sp) or c.K < 512 or c.N < 128:
        return False
    return _cdiv(c.M, 128) * _cdiv(c.N, 128) <= 256


def workspace_bytes(c):
    sp = resolve_split(c)
    cs = sp * c.M * 4 if c.cs else 0
    if big_tt_plan(c)[0] > 0 or sp > 1 or c.cs:
        return sp * c.M * c.N * 4 + cs
    return 0


def select(c, pair=False):
    """The launch form dl_gemm picks for case c, as the short text the CASES tables use."""
    tn = lambda b: "bf16" if b else "f32"
    tt, bm = big_tt_plan(c)
    sp = resolve_split(c)
    slab = sp > 1 or tt > 0 or c.cs
    red = " reduce<%s>" % tn(c.bf_out) if slab else ""
    if tt > 0:
        return "tt2 bm%d sp%d%s%s" % (bm, sp, " cs" if c.cs else "", red)
    if big_eligible(c, sp):
        return "big256 epi%d" % pick_epi(c, False)
    if not pair and lat_eligible(c, sp):
        return "lat128 epi%d" % pick_epi(c, False)
    bke = 128 // es_of(c.bf_in)
    dma = c.K % bke == 0
    epi = pick_epi(c, slab)
    if slab:
        epi = 1
    elif not dma:
        epi = 0 if epi == 0 else 1
    tw = pick_tw(c) if slab else 4
    s = "k128 %s>%s X%dW%d %s epi%d" % (tn(c.bf_in), tn(c.bf_out and not slab), c.xs, c.ws, "dma" if dma else "reg", epi)
    if slab:
        s += " sp%d tw%d%s%s" % (sp, tw, " cs" if c.cs else "", red)
    return s


def group_plan(members):
    """members: (M, N, K) of bf16 weight-gradient products.  Returns (tile rows, [slabs per member])."""
    min_steps = min(_cdiv(K, 64) for _, _, K in members)
    all_mn = sum(M * N for M, N, _ in members)
    big_mn = sum(M * N for M, N, _ in members if M * N >= 640 * 1024)
    min_m = min(M for M, _, _ in members)
    bm = 256 if (2 * big_mn >= all_mn and min_m >= 256 and min_steps >= 256) else 128
    tiles = sum(_cdiv(M, bm) * _cdiv(N, 256) for M, N, _ in members)
    sp = max(min(256 // tiles, min_steps // 8), 1)
    return bm, [trim_splits(K, 64, sp) for _, _, K in members]


def colsum_plan(M, N):
    """(rows per workgroup, chunks) of dl_colsum."""
    colgroups = _cdiv(N, 256)
    chunks = _cdiv(1024, colgroups)
    rows = max(_cdiv(M, chunks), 32)
    rows = _cdiv(rows, 4) * 4
    return rows, _cdiv(M, rows)
