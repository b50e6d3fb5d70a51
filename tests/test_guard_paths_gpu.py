"""The device-side padding guards of csrc/compact.hip, launch form by launch form, against the host predicates of
tests/guard_ref.py: dl_rows_equal_check, the guard workgroups of dl_embed_rows, dl_protein_plan_build and its capacity flag.
Everything is boolean or bitwise: no tolerance anywhere.

Every launch gets a flag word of its own out of one int32 tensor, pre-set to a sentinel bit that must survive; the only bit a
launch may add is its `code`.  The launches of a test are enqueued back to back and read after ONE synchronisation.  Inputs
lie between junk (rows), out-of-range values (ids, periods, lengths: reading them would flag) or NaN (fill values); outputs
and tables in NaN / -7 filled buffers whose unaddressed elements must stay bitwise unchanged.

Every malformed input is malformed as data only (tests/guard_ref.py): no launch here can address memory outside its buffers.
"""
import itertools

import numpy as np
import pytest
import torch

from tests import elem_ref as er
from tests import guard_ref as G
from tests.test_norm_paths_gpu import BF, DEV, F32, Guarded, _lib

pytestmark = pytest.mark.gpu

SENT = 1 << 30
DT = {"bf16": BF, "f32": F32}


def flag_words(n):
    """n flag words in the middle of a tensor of sentinels: (the whole tensor, the words)."""
    t = torch.full((n + 128,), SENT, dtype=torch.int32, device=DEV)
    return t, t[64:64 + n]


def check_flags(whole, want, names):
    got = whole.cpu().numpy()
    assert (got[:64] == SENT).all() and (got[64 + len(want):] == SENT).all(), "a flag word outside the launches' words changed"
    got = got[64:64 + len(want)]
    bad = np.nonzero(got != np.asarray(want, dtype=np.int32))[0]
    assert bad.size == 0, "%d of %d launches raised the wrong flag, first %s: got %#x, want %#x" % (
        bad.size, len(want), names[bad[0]], got[bad[0]], want[bad[0]])


def banded(n, dt, fill):
    """(whole, view): n elements with 256 elements of `fill` in front and behind."""
    t = torch.full((n + 512,), fill, dtype=dt, device=DEV)
    return t, t[256:256 + n]


def bits32(t):
    return t.contiguous().view(torch.int32)


# ---- dl_rows_equal_check ---------------------------------------------------------------------------------------------------------
def run_rows(cases):
    """One launch per case.  Cases of one geometry share a device buffer: slot i holds case i's bytes, `base_off` bytes behind
    a 16-byte address, between junk bytes that differ from slot to slot."""
    L, ok, stream, _, _ = _lib()
    whole, flags = flag_words(len(cases))
    want, keep, k = [], [], 0
    for geo, grp in itertools.groupby(cases, key=lambda c: (c.B, c.N, c.row_bytes, c.row0, c.base_off)):
        grp = list(grp)
        B, N, rb, row0, off = geo
        nbytes = B * N * rb
        first = 16 + off
        slot = (first + nbytes + 16 + 15) // 16 * 16
        host = np.empty((len(grp), slot), np.uint8)
        junk = ((np.arange(len(grp))[:, None] * 37 + np.arange(slot - nbytes)[None, :] * 11 + 5) & 0xFF).astype(np.uint8)
        host[:, :first], host[:, first + nbytes:] = junk[:, :first], junk[:, first:]
        for i, c in enumerate(grp):
            host[i, first:first + nbytes] = G.rows_data(c)
        dev = torch.from_numpy(host).to(DEV)
        keep.append(dev)
        assert dev.data_ptr() % 16 == 0
        for i, c in enumerate(grp):
            code = 1 << (k % 29)
            ok(L.dl_rows_equal_check(dev.data_ptr() + i * slot + first, B, N, rb, row0, code, flags.data_ptr() + 4 * k, stream),
               "dl_rows_equal_check")
            want.append(SENT | (0 if G.rows_equal(host[i, first:first + nbytes], B, N, rb, row0) else code))
            k += 1
    torch.cuda.synchronize()
    check_flags(whole, want, [c.name for c in cases])
    return len(cases), sum(1 for w in want if w != SENT)


@pytest.mark.parametrize("geo", G.ROWS_SMALL, ids=["%s_rb%d_off%d_row0%d" % (g[0].replace(" ", "_"), g[1], g[2], g[3]) for g in G.ROWS_SMALL])
def test_rows_equal_every_word_of_a_small_input(geo):
    """B = 3, N = 6: the untouched input, then one bit flipped in the low and in the high half of EVERY 32-bit word — the
    words of rows >= row0 must raise `code`, the words of the free rows must not."""
    n, tripped = run_rows(G.rows_small_cases(*geo))
    form, rb, off, row0 = geo
    assert tripped == 2 * 3 * (6 - row0) * rb // 4
    print("%s: %d guard launches, %d tripped" % (form, n, tripped))


def test_rows_equal_at_the_product_widths():
    """784- and 1568-byte rows, N = 512, row0 = 128 / 384, B = 2 and B = 1: first and last chunk of the last row of the last
    sample, a low bit and +0.0 -> -0.0; NaNs with equal bits and an edit in a free row are quiet."""
    n, tripped = run_rows(G.rows_product_cases())
    assert tripped == 2 * 2 * 2 * 4
    print("rows_equal wide, product widths: %d guard launches, %d tripped" % (n, tripped))


def test_rows_equal_grid_stride():
    """Just above 4096 * 256 * 2 chunks (33.7 MB checked): the single deviation lies in the last chunk."""
    n, tripped = run_rows(G.rows_grid_cases())
    assert tripped == 2
    print("rows_equal grid-stride: %d guard launches, %d tripped" % (n, tripped))


def test_rows_equal_refusals():
    L, ok, stream, _, _ = _lib()
    whole, flags = flag_words(1)
    x = torch.zeros(4 * 6 * 32, dtype=torch.uint8, device=DEV)
    for what, args in (("row_bytes % 4 != 0", (x.data_ptr(), 4, 6, 30, 2, 2, flags.data_ptr())),
                       ("row0 == N", (x.data_ptr(), 4, 6, 32, 6, 2, flags.data_ptr())),
                       ("code == 0", (x.data_ptr(), 4, 6, 32, 2, 0, flags.data_ptr())),
                       ("null flags", (x.data_ptr(), 4, 6, 32, 2, 2, None)),
                       ("null x", (None, 4, 6, 32, 2, 2, flags.data_ptr())),
                       ("a base that is no 4-byte multiple", (x.data_ptr() + 2, 4, 6, 32, 2, 2, flags.data_ptr()))):
        with pytest.raises(RuntimeError, match="dl_rows_equal_check"):
            ok(L.dl_rows_equal_check(*args, stream), "dl_rows_equal_check (%s)" % what)
    ok(L.dl_rows_equal_check(x.data_ptr(), 4, 6, 32, 5, 2, flags.data_ptr(), stream), "dl_rows_equal_check")   # row0 = N - 1 runs
    torch.cuda.synchronize()
    check_flags(whole, [SENT], ["refusals"])


# ---- dl_embed_rows with period -----------------------------------------------------------------------------------------------------
def fill_tensor(fb, dt):
    """fp32 bit patterns (exact in bf16) -> values of dtype dt, bit for bit."""
    if dt == F32:
        return torch.from_numpy(fb.view(np.int32).copy()).view(F32)
    return torch.from_numpy((fb >> 16).astype(np.uint16).view(np.int16)).view(BF)


@pytest.mark.parametrize("dtn,Lp", G.PERIOD_SETS, ids=["%s_L%d" % s for s in G.PERIOD_SETS])
def test_embed_rows_period_guard(dtn, Lp):
    """V = 27, D = 127, four samples per launch: for every period of guard_ref.period_values and every edit position, one launch
    with the guard workgroups and one without.  The flag is the OR of `not period_ok` over the samples; `out` is bitwise the
    plain launch's, and nothing is written around it."""
    L, ok, stream, DTC, lib_mod = _lib()
    dt, V, D, B = DT[dtn], G.PERIOD_V, G.PERIOD_D, G.PERIOD_B
    cases = G.period_cases(dtn, Lp)
    n, C = len(cases), D + 1
    data = [G.period_batch(c) for c in cases]
    ids_h = np.stack([d[0] for d in data])
    fb_h = np.stack([d[1] for d in data])
    per_h = np.stack([d[2] for d in data])
    g = torch.Generator().manual_seed(Lp)
    src_h = torch.randperm(B * Lp, generator=g)[:136].to(torch.int32)
    src_h = torch.cat((src_h[:5], torch.tensor([-1, -1], dtype=torch.int32), src_h[5:], torch.tensor([-1, 0, B * Lp - 1], dtype=torch.int32)))
    R = src_h.numel()
    assert R * (C // 8) > 2048                                      # more than one gather workgroup in front of the guards
    weight = torch.randn(V, C, generator=g).to(dt)
    weight[:, D] = float("nan")                                    # (the padded column: never read into an output)

    def between(values, fill, dtype):
        t = torch.full((values.numel() + 128,), fill, dtype=dtype, device=DEV)
        v = t[64:64 + values.numel()].view(values.shape)
        v.copy_(values)
        return v

    ids = between(torch.from_numpy(ids_h), V + 1000, torch.int64)
    period = between(torch.from_numpy(per_h), -7, torch.int32)
    src = between(src_h, -7, torch.int32)
    fg = Guarded(n * B * Lp, dt)
    fill = fg.view((n, B, Lp))
    fill.copy_(fill_tensor(fb_h, dt))
    wg = Guarded(V * C, dt)
    w = wg.view((V, C))
    w.copy_(weight)
    whole, flags = flag_words(n)
    gap = 64
    outs = []
    for guarded in (True, False):
        og = Guarded(n * (R * C + gap), dt)
        ov = og.view((n, R * C), (R * C + gap, 1))
        before = og.bits()
        for i in range(n):
            ok(L.dl_embed_rows(ids[i].data_ptr(), w.data_ptr(), fill[i].data_ptr(), src.data_ptr(), ov[i].data_ptr(), R, V, D,
                               period[i].data_ptr() if guarded else None, B if guarded else 0, Lp if guarded else 0,
                               flags.data_ptr() + 4 * i if guarded else None, DTC[dt], stream), "dl_embed_rows")
        outs.append((og, ov, before))
    torch.cuda.synchronize()
    want = [SENT | (lib_mod.FLAG_PROT_PERIOD if G.period_flag(ids_h[i], fb_h[i], per_h[i], Lp) else 0) for i in range(n)]
    check_flags(whole, want, [c.name for c in cases])
    for og, ov, before in outs:
        og.untouched("embed_rows_period_%s_L%d" % (dtn, Lp), before)
    a, b = outs[0][1], outs[1][1]
    isz = torch.int16 if dt == BF else torch.int32
    assert torch.equal(a.contiguous().view(isz), b.contiguous().view(isz)), "the launch with guard workgroups wrote another `out`"
    for i in (0, n // 2, n - 1):                                    # ... and the plain launch is the gather it always was
        ref = er.embed_rows(ids[i], w, fill[i], src, D)
        assert torch.equal(b[i].view(R, C).contiguous().view(isz), ref.contiguous().view(isz)), cases[i].name
    # the inputs are what they were
    assert torch.equal(ids.cpu(), torch.from_numpy(ids_h)) and torch.equal(period.cpu(), torch.from_numpy(per_h))
    tripped = sum(1 for v in want if v != SENT)
    assert 0 < tripped < n
    print("embed_rows guard %s L = %d: %d guard launches (+ %d plain), %d tripped" % (dtn, Lp, n, n, tripped))


# ---- dl_protein_plan_build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.PLAN_CASES, ids=[c.name for c in G.PLAN_CASES])
def test_plan_build_tables_and_capacity(c):
    """Device tables against protein_plan.ProteinPlan entry by entry, with B > 256 (the per-workgroup prefix sum takes a second
    trip), at R = need (quiet), below it and far above it.

    A refused build (plan_build_kernel): every sample's workgroup decides for itself from its own prefix sum — `off + rows > R`
    returns before the first store, so a sample that fits is FULLY written (rows, row_of, period) and one that does not fit
    writes nothing; the padding workgroups see `off > R`, raise the flag and write nothing.  So with R < need the tables equal
    the host tables of the leading samples that fit and are untouched behind them."""
    from druglamp_amd.protein_plan import ProteinPlan
    L, ok, stream, _, lib_mod = _lib()
    S, lengths = c.S, G.plan_lengths(c)
    B = len(lengths)
    need, R, fit = G.plan_rows(c)
    len_t = torch.full((B + 128,), -7, dtype=torch.int32, device=DEV)
    len_t[64:64 + B] = torch.from_numpy(lengths).to(DEV)
    src_w, src = banded(R, torch.int32, -7)
    w_w, w = banded(R, F32, float("nan"))
    rep_w, rep = banded(3 * R, torch.int32, -7)
    map_w, row_of = banded(B * S, torch.int32, -7)
    per_w, period = banded(B, torch.int32, -7)
    whole, flags = flag_words(1)
    ok(L.dl_protein_plan_build(len_t[64:].data_ptr(), B, S, R, src.data_ptr(), w.data_ptr(), rep.data_ptr(), row_of.data_ptr(),
                               period.data_ptr(), flags.data_ptr(), stream), "dl_protein_plan_build")
    torch.cuda.synchronize()
    check_flags(whole, [SENT | (lib_mod.FLAG_PLAN_ROWS if need > R else 0)], [c.name])
    assert (need > R) == (fit < B) and fit >= 1
    host = ProteinPlan(lengths[:fit], S, bucket=1)
    n = host.rows                                                   # rows of the samples that fit
    # the expected buffers, bands included: host tables, then bucket padding (a complete build) or the fill (a refused one)
    nan_bits = int(bits32(torch.full((1,), float("nan"), dtype=F32))[0])
    e_src = np.full(R + 512, -7, np.int32)
    e_w = np.full(R + 512, nan_bits, np.int32)
    e_rep = np.full(3 * R + 512, -7, np.int32)
    e_map = np.full(B * S + 512, -7, np.int32)
    e_per = np.full(B + 512, -7, np.int32)
    e_src[256:256 + n] = host.src
    e_w[256:256 + n] = host.w.view(np.int32)
    e_rep[256:256 + 3 * n] = host.rep.reshape(-1)
    e_map[256:256 + fit * S] = host.row_of
    e_per[256:256 + fit] = host.period
    if fit == B:
        assert n == need
        e_src[256 + n:256 + R] = -1
        e_w[256 + n:256 + R] = np.array([-1.0], np.float32).view(np.int32)[0]
        e_rep[256 + 3 * n:256 + 3 * R] = np.tile(np.array([0, 1, 0], np.int32), R - n)
    for what, got, want in (("src", src_w, e_src), ("w", w_w, e_w), ("rep", rep_w, e_rep), ("row_of", map_w, e_map), ("period", per_w, e_per)):
        got = bits32(got).cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s: %s differs in %d entries, first at %d (band 256): got %d, want %d" % (
            c.name, what, bad.size, bad[0], got[bad[0]], want[bad[0]])
    assert torch.equal(len_t[64:64 + B].cpu(), torch.from_numpy(lengths))
    print("%s: 1 launch, B = %d, need = %d, R = %d, %d samples fit" % (c.name, B, need, R, fit))


def test_plan_build_refusals():
    L, ok, stream, _, _ = _lib()
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = t.data_ptr()
    for what, args in (("B == 0", (p, 0, 8, 16, p, p, p, p, p, p)), ("R == 0", (p, 1, 8, 0, p, p, p, p, p, p)),
                       ("null tables", (p, 1, 8, 16, None, p, p, p, p, p)), ("B >= 2^20", (p, 1 << 20, 8, 16, p, p, p, p, p, p))):
        with pytest.raises(RuntimeError, match="dl_protein_plan_build"):
            ok(L.dl_protein_plan_build(*args, stream), "dl_protein_plan_build (%s)" % what)
    torch.cuda.synchronize()
    assert not bool(t.any())
