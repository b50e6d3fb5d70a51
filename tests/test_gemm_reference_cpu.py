"""The GEMM pin's CPU half: the fp64 reference of tests/gemm_ref.py against torch's own operators, the dropout mask's
properties, the data conditions the GPU cases rely on, and the Python mirror of the host dispatch against the CASES table of
tests/test_gemm_paths_gpu.py and against the library where it answers on the host.  No GPU; the two mirror-against-the-library
tests call host entry points of the built library (libdruglamp_hip.so) and fail without a build."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as R
from tests import test_gemm_paths_gpu as T

F64 = torch.float64
SINGLE = [c for c in T.CASES if c.kind == "gemm"]
ALL = [q for c in T.CASES for q in getattr(c, "members", [c])]


# ---- the reference against torch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xs,ws,ldx_extra,ldw_extra", [(0, 0, 0, 0), (0, 0, 8, 24), (0, 0, -20, 0), (0, 1, 0, 0), (0, 1, 8, 24), (0, 1, -20, 8),
                                                       (1, 1, 0, 0), (1, 1, 8, 24)])
def test_reference_matches_torch(xs, ws, ldx_extra, ldw_extra):
    """acc / pre / C against F.linear, F.gelu, F.relu and autograd's gelu' in fp64, for the three layouts, with pitch gaps and
    (K-contiguous X) overlapping rows."""
    g = torch.Generator().manual_seed(3 + 7 * xs + 11 * ws + ldx_extra)
    M, N, K = 24, 16, 40
    ldx = (M if xs else K) + ldx_extra
    ldw = (N if ws else K) + ldw_extra
    fx = torch.randn(T.storage_span(*((K, M) if xs else (M, K)), ldx) + 5, generator=g, dtype=F64)
    fw = torch.randn(T.storage_span(*((K, N) if ws else (N, K)), ldw) + 5, generator=g, dtype=F64)
    X, W = R.operand(fx, M, K, ldx, xs), R.operand(fw, N, K, ldw, ws)
    Xe = torch.stack([torch.stack([fx[(k * ldx + m) if xs else (m * ldx + k)] for k in range(K)]) for m in range(M)])
    We = torch.stack([torch.stack([fw[(k * ldw + n) if ws else (n * ldw + k)] for k in range(K)]) for n in range(N)])
    assert torch.equal(X, Xe) and torch.equal(W, We)
    bias = torch.randn(N, generator=g, dtype=F64)
    res = torch.randn(M, N, generator=g, dtype=F64)
    resmod = torch.randn(6, N, generator=g, dtype=F64)
    dact = torch.randn(M, N, generator=g, dtype=F64).requires_grad_()
    old = torch.randn(M, N, generator=g, dtype=F64)
    keep = torch.from_numpy(R.keep_mask(5, 0, M, N, 0.37))
    sc = R.inv_keep(0.37)
    gp, = torch.autograd.grad(F.gelu(dact).sum(), dact)
    lin = F.linear(Xe, We, bias)
    tol = 1e-12
    r = R.reference(X, W, bias=bias)
    assert (r["acc"] - F.linear(Xe, We)).abs().max() <= tol and (r["C"] - lin).abs().max() <= tol
    assert (r["S"] - F.linear(Xe.abs(), We.abs())).abs().max() <= tol
    r = R.reference(X, W, bias=bias, act=1, keep=keep, keep_scale=sc)
    assert (r["pre"] - lin).abs().max() <= tol and (r["C"] - F.gelu(lin) * keep * sc).abs().max() <= tol
    r = R.reference(X, W, bias=bias, act=2, residual=res)
    assert (r["C"] - (F.relu(lin) + res)).abs().max() <= tol
    r = R.reference(X, W, dact_pre=dact.detach(), keep=keep, keep_scale=sc)
    assert (r["C"] - F.linear(Xe, We) * gp * keep * sc).abs().max() <= tol
    r = R.reference(X, W, bias=bias, residual=res, keep=keep, keep_scale=sc)                       # EPI 3: residual AFTER dropout
    assert (r["C"] - (lin * keep * sc + res)).abs().max() <= tol
    r = R.reference(X, W, bias=bias, residual=resmod, res_row_mod=6, res_before_dropout=True, keep=keep, keep_scale=sc, old_c=old)
    assert (r["C"] - ((lin + resmod.repeat(4, 1)) * keep * sc + old)).abs().max() <= tol
    r = R.reference(X, W, want_colsum=True)
    assert (r["x_colsum"] - Xe.sum(1)).abs().max() <= tol
    o = torch.randn(K, generator=g, dtype=F64)
    s, mag = R.colsum(Xe, o)
    assert (s - (Xe.sum(0) + o)).abs().max() <= tol and (mag >= s.abs() - tol).all()
    assert (R.colsum(Xe)[0] - Xe.sum(0)).abs().max() <= tol


# ---- the dropout mask ---------------------------------------------------------------------------------------------------------
def test_fmix32_is_the_murmur3_finaliser():
    """Known values of the murmur3 32-bit finaliser (fmix32(0) = 0; fmix32 is a bijection: distinct inputs stay distinct)."""
    x = np.arange(1 << 16, dtype=np.uint32)
    y = R._fmix32(x)
    assert int(y[0]) == 0 and len(np.unique(y)) == len(x)

    def scalar(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    for v in (1, 2, 0xDEADBEEF, 0xFFFFFFFF, 12345):
        assert int(R._fmix32(np.array([v], dtype=np.uint32))[0]) == scalar(v)


def test_draw_against_plain_integer_arithmetic():
    def one(seed, idx):
        def f(h):
            h = ((h ^ (h >> 16)) * 0x85EBCA6B) & 0xFFFFFFFF
            h = ((h ^ (h >> 13)) * 0xC2B2AE35) & 0xFFFFFFFF
            return h ^ (h >> 16)
        x = ((idx & 0xFFFFFFFF) + (seed & 0xFFFFFFFF)) & 0xFFFFFFFF
        hi = ((idx >> 32) ^ (seed >> 32)) & 0xFFFFFFFF
        rot = ((hi << 13) | (hi >> 19)) & 0xFFFFFFFF
        return (f(x ^ hi) << 32) | f(((x + 0x9E3779B9) & 0xFFFFFFFF) ^ rot ^ 0x7F4A7C15)
    for seed in (0, 1, 0xFFFFFFFF, 0x123456789ABCDEF0, 2 ** 64 - 1):
        idx = [0, 1, 0xFFFFFFFF, 0x100000000, 0x7FFFFFFF12345678]
        got = R.draws(seed, np.array(idx, dtype=np.uint64))
        assert [int(v) for v in got] == [one(seed, i) for i in idx]


@pytest.mark.parametrize("p", [0.1, 0.37, 0.5])
def test_keep_mask_properties(p):
    M, N = 300, 136
    t = R.thr16(p)
    assert t == int(math.floor(p * 65536 + 0.5)) and (p not in (0.1, 0.37) or t % 16 != 0)
    a, b = R.keep_mask(77, 0, M, N, p), R.keep_mask(77, 0, M, N, p)
    assert a.shape == (M, N) and a.dtype == np.bool_ and np.array_equal(a, b)
    q = 1.0 - t / 65536.0
    assert abs(a.mean() - q) <= 6.0 * math.sqrt(q * (1 - q) / (M * N))
    c = R.keep_mask(78, 0, M, N, p)
    assert 0.2 * min(q, 1 - q) < (a != c).mean()                      # another seed: another mask
    assert np.array_equal(R.keep_mask(70, 7, M, N, p), a)              # seed + offset is a shifted seed
    assert np.array_equal(R.keep_mask(2 ** 64 - 1, 78, M, N, p), a)    # ... modulo 2^64
    # four consecutive columns share one draw, 16 bits each, lowest first
    bits = R.draws(77, np.arange(M * N // 4, dtype=np.uint64))
    for j in range(4):
        f = (bits >> np.uint64(16 * j)) & np.uint64(0xFFFF)
        assert np.array_equal(a.reshape(-1, 4)[:, j], f >= t)
    # the scale is 1 / (1 - p) in fp32
    assert R.inv_keep(p) == float(np.float32(1.0) / np.float32(1.0 - np.float32(p)))


def test_keep_mask_rows_follow_the_flat_index():
    """The group index is (row * N + col) >> 2 of the LOGICAL [M][N] output: a mask of more rows starts with the mask of fewer,
    and another N reshuffles it."""
    a = R.keep_mask(9, 0, 40, 24, 0.37)
    assert np.array_equal(R.keep_mask(9, 0, 64, 24, 0.37)[:40], a)
    assert np.array_equal(R.keep_mask(9, 0, 20, 48, 0.37).reshape(40, 24), a)


# ---- the table: forms, flags, conditions --------------------------------------------------------------------------------------
def test_case_names_are_unique_and_ordered_by_family():
    names = [c.name for c in T.CASES]
    assert len(set(names)) == len(names)
    fam = [c.form.split(" ")[0] for c in T.CASES]
    seen = []
    for f in fam:
        if not seen or seen[-1] != f:
            assert f not in seen, "family %s is not contiguous in the table" % f
            seen.append(f)
    assert seen == ["k128", "big256", "lat128", "tt2", "group", "pair"]


@pytest.mark.parametrize("c", SINGLE, ids=lambda c: c.name)
def test_case_selects_the_form_it_names(c):
    assert R.select(c) == c.form
    bke = 128 // R.es_of(c.bf_in)
    assert ("dma" in c.form) == (c.K % bke == 0) or c.form.split(" ")[0] != "k128"
    if c.form.startswith("big256") or c.form.startswith("lat128"):
        assert c.form.endswith("epi%d" % R.pick_epi(c, False))


def test_epilogue_flags_match_the_epi_each_case_claims():
    want = {0: lambda c: not (c.res or c.act or c.pre or c.dact or c.p),
            2: lambda c: c.act == 1 and c.pre and c.bias and not c.res and not c.dact,
            3: lambda c: c.res == "after" and not c.act and not c.pre and not c.dact and c.rmod == 0,
            4: lambda c: c.dact and not c.bias and not c.res and not c.act and not c.pre,
            5: lambda c: c.act == 2 and not c.res and not c.pre and not c.dact and not c.p}
    for c in SINGLE:
        if "sp" in c.form.split("epi")[-1] or c.form.startswith("tt2"):
            assert R.plain(c)
            continue
        epi = int(c.form.split("epi")[1][0])
        if epi != 1:
            assert want[epi](c) and c.N % 8 == 0 and not c.acc, c.name
        elif "dma" in c.form:
            assert c.N % 8 or c.acc or c.rmod or c.res == "before" or (c.act and (c.res or c.dact)), c.name
    # every dropout-capable specialised epilogue of the large-tile kernels runs with dropout
    for fam in ("big256", "lat128", "k128 bf16>bf16 X0W0 dma", "k128 f32>f32 X0W0 dma"):
        for e in (2, 3, 4):
            assert any(c.form.startswith(fam) and c.form.endswith("epi%d" % e) and c.p > 0 for c in SINGLE), (fam, e)
    assert all(R.thr16(c.p) % 256 != 0 for c in ALL if c.p > 0)


def test_coverage_of_the_dispatch_thresholds():
    f = {c.form for c in SINGLE}
    for epi in (0, 2, 3, 4, 5):
        assert {"big256 epi%d" % epi, "lat128 epi%d" % epi, "k128 bf16>bf16 X0W0 dma epi%d" % epi, "k128 f32>f32 X0W0 dma epi%d" % epi} <= f
    big = [c for c in SINGLE if c.form.startswith("big256")]
    assert min(R._cdiv(c.M, 256) * R._cdiv(c.N, 256) for c in big) == 192          # the threshold itself
    assert any(R._cdiv(c.M, 256) * R._cdiv(c.N, 256) > 256 for c in big)            # a second tile per workgroup
    assert any(R._cdiv(c.M, 128) * R._cdiv(c.N, 128) > 512 for c in SINGLE if c.form.startswith("k128"))
    assert any(c.form.startswith("lat128") and c.K == 512 for c in SINGLE)          # LAT_MIN_K itself
    assert {"tw2", "tw4"} <= {w for c in SINGLE for w in c.form.split(" ")}
    assert any(c.split > 0 and R.resolve_split(c) < c.split for c in SINGLE)        # trim_splits lowers the request
    assert any(c.form.startswith("tt2 bm256") and c.K % 64 for c in SINGLE) and any(c.form.startswith("tt2 bm128") for c in SINGLE)


def _args(c):
    from druglamp_amd import _lib
    a = _lib.GemmArgs()
    p16 = 1 << 20
    a.X = a.W = a.C = p16
    a.M, a.N, a.K, a.ldx, a.ldw, a.ldc = c.M, c.N, c.K, c.ldx, c.ldw, c.N + 8
    a.x_kslow, a.w_kslow = c.xs, c.ws
    a.in_dtype = _lib.DL_BF16 if c.bf_in else _lib.DL_F32
    a.out_dtype = _lib.DL_BF16 if c.bf_out else _lib.DL_F32
    a.bias = p16 if c.bias else None
    a.residual = p16 if c.res else None
    a.pre_out = p16 if c.pre else None
    a.dact_pre = p16 if c.dact else None
    a.act, a.dropout_p, a.accumulate, a.split_k, a.algo = c.act, c.p, int(c.acc), c.split, c.algo
    a.res_row_mod, a.res_before_dropout = c.rmod, int(c.res == "before")
    a.x_colsum = p16 if c.cs else None
    return a


def test_mirror_against_the_library_workspace_bytes():
    """dl_gemm_workspace_bytes gives the slab count of every slab path (resolve_split, auto_split, trim_splits, pick_tw through
    auto_split's tile size, big_tt_plan) and the x_colsum strip."""
    from druglamp_amd import _lib
    L = _lib.lib()
    for c in SINGLE:
        a = _args(c)
        assert L.dl_gemm_workspace_bytes(C.byref(a)) == R.workspace_bytes(c), c.name
    # and over a sweep around every threshold of the plans, case-independent
    for M, N, K, bf, cs in [(64, 64, 4096, 1, 0), (64, 64, 4032, 1, 1), (63, 64, 4096, 1, 0), (512, 512, 65536, 1, 0), (256, 512, 65536, 1, 0),
                            (1280, 512, 4096, 1, 1), (1280, 504, 4096, 1, 0), (128, 640, 262144, 1, 0), (128, 640, 262143, 1, 0), (96, 632, 262144, 1, 1),
                            (256, 256, 1024, 0, 0), (2048, 2048, 512, 1, 0), (136, 264, 1000, 1, 1), (136, 264, 96, 0, 0)]:
        c = T.G("sweep", "", M, N, K, bf_in=bool(bf), bf_out=False, xs=1, ws=1, split=0, cs=bool(cs))
        assert L.dl_gemm_workspace_bytes(C.byref(_args(c))) == R.workspace_bytes(c), (M, N, K, bf, cs)
        for sk in (1, 2, 5, 64):
            c = T.G("sweep", "", M, N, K, bf_in=bool(bf), bf_out=False, split=sk)
            assert L.dl_gemm_workspace_bytes(C.byref(_args(c))) == R.workspace_bytes(c), (M, N, K, bf, sk)


def test_mirror_against_the_library_group_plan():
    from druglamp_amd import _lib
    L = _lib.lib()
    groups = [c for c in T.CASES if c.kind == "group"]
    assert {c.form.split(" ")[1] for c in groups} == {"bm128", "bm256"}
    extra = [[(256, 1024, 8192), (1024, 256, 8192), (256, 256, 8192)], [(2048, 512, 65536), (512, 2048, 65536)], [(128, 128, 1024), (128, 128, 1000)]]
    for members in [[(q.M, q.N, q.K) for q in c.members] for c in groups] + extra:
        arr = (_lib.GemmArgs * len(members))(*[_args(T.G("g", "", M, N, K, xs=1, ws=1, split=0, bf_out=False)) for M, N, K in members])
        sp = (C.c_int32 * len(members))()
        assert L.dl_gemm_group_plan(arr, len(members), sp) == 0
        assert list(sp) == R.group_plan(members)[1], members
    for c in groups:
        bm, sp = R.group_plan([(q.M, q.N, q.K) for q in c.members])
        assert c.form == "group bm%d sp%s" % (bm, ",".join(str(s) for s in sp))
        assert any(q.cs for q in c.members) and any(q.K % 64 for q in c.members)
        if bm == 256:
            assert all(q.M >= 256 and q.K >= 16384 for q in c.members)
            assert 2 * sum(q.M * q.N for q in c.members if q.M * q.N >= 640 * 1024) >= sum(q.M * q.N for q in c.members)


def test_pairs_share_a_launch():
    for c in T.CASES:
        if c.kind == "pair":
            a, b = c.members
            assert "pair " + R.select(a, pair=True) == c.form and R.workspace_bytes(a) == 0
            assert not R.big_eligible(a, 1) and not R.lat_eligible(a, 1)
            assert a.seed != b.seed and (a.M, a.N, a.K, a.ldx, a.ldw) == (b.M, b.N, b.K, b.ldx, b.ldw)
            # dl_gemm_pair shares the launch only if every pointer of the second member is 16-byte aligned and the pitches are
            # equal, and otherwise runs two launches without saying so.  The pitches follow from (N, flags), equal above; the
            # pointers are allocation + these leads (the GPU case asserts the same on the real argument blocks).
            es_in, es_out, ldn = R.es_of(b.bf_in), R.es_of(b.bf_out), b.N + (8 if b.N % 4 == 0 else 5)
            leads = {"X": T.Buf.operand_lead(b.ldx) * es_in, "W": T.Buf.operand_lead(b.ldw) * es_in, "C": T.Buf.out_lead(2, ldn) * es_out}
            if b.bias:
                leads["bias"] = T.Buf.operand_lead(b.N) * 4
            if b.res:
                leads["residual"] = T.Buf.operand_lead(ldn) * es_in
            if b.dact:
                leads["dact_pre"] = T.Buf.operand_lead(ldn) * es_in
            if b.pre:
                leads["pre_out"] = T.Buf.out_lead(1, ldn) * es_in
            assert all(v % 16 == 0 for v in leads.values()), leads


@pytest.mark.parametrize("c", [q for q in ALL if not R.plain(q) or q.M * q.N * q.K <= 1 << 26], ids=lambda c: c.name)
def test_data_conditions(c):
    """|pre| <= 12 where the polynomial GELU is used, |dact_pre| <= 5.5 for gelu', no bound dominated by the polynomial's
    absolute term — on the very tensors the GPU case uses (same generator, same seed)."""
    form = c.form if c.form and c.form != "group" else R.select(c, pair=not c.form)
    d = T.gen(c)
    fx, fw = d["X"].reshape(-1), d["W"].reshape(-1)
    if d["X"].dim() == 2:           # place at the pitch, as the device buffers do (gaps are never read by the reference)
        fx = torch.zeros(T.storage_span(*d["X"].shape, c.ldx), dtype=d["X"].dtype)
        torch.as_strided(fx, tuple(d["X"].shape), (c.ldx, 1)).copy_(d["X"])
    if d["W"].dim() == 2:
        fw = torch.zeros(T.storage_span(*d["W"].shape, c.ldw), dtype=d["W"].dtype)
        torch.as_strided(fw, tuple(d["W"].shape), (c.ldw, 1)).copy_(d["W"])
    r, keep = T.reference(c, fx, fw, d, "cpu")
    T.conditions(c, r, form, keep, d)
    b = T.bounds(c, r, R.resolve_split(c), T.poly_form(c, form), keep)
    live = r["C"] != 0
    assert bool((b["C"][0][live] > 0).all()) and bool(torch.isfinite(b["C"][0]).all())
    assert float(r["S"].min()) > 0
