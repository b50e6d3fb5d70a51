"""dl_pgca_pairs_probs / dl_pgca_pairs_ragged_probs (csrc/pgca_pairs_probs.hip) through ops.pgca_pairs_probs and
ops.pgca_pairs_ragged_probs, element-wise against the fp64 reference of tests/attn_ref.py: per drug, reference_fwd(...)["Pm"] on
the explicitly gathered queries and that drug's own rows, count and (key_tail_rows, w_d); expanded maps are Pm[..., lead:] / w
repeated, as _expected in tests/test_attention_probs_gpu.py.

Bound: that file's rounding model (u_f = 2^-24, MARGIN = 2, lam and mag_lse from attn_ref), no new tolerance:
    |got - ref| <= 2 ref ((hd + 2) u_f (lam_qk + mag_lse_q) + (Lk_full + 8) u_f) + 2^-120
and a row of an expanded or tail-less map sums to 1 within (Lk_full + 8) u_f plus the row's summed bounds.  Every case asserts
lam <= 96, the cap that file uses (at input scale 0.7 and the largest weight, 63, the fp64 reference alone gives lam < 10: checked
without a device through _setup(name, dt, expand, "cpu")).  The worst ratio is printed before it is asserted.

Buffers as in tests/test_pgca_ragged_gpu.py: Q and the row store are NaN outside the addressed elements (a never-referenced NaN
segment between two drugs and one behind the rows the call is told about), `out` is NaN with guard bands and a pitch above the
column count: every addressed element — the zero-fill columns included, exactly +0.0 — must be overwritten, every other element
must stay bitwise unchanged.  Every case runs twice; the two runs must agree bitwise.
"""
import collections
import functools
import math

import pytest
import torch

from tests.attn_ref import reference_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
U_F, MARGIN, LAM, FLOOR = 2.0 ** -24, 2.0, 96.0, 2.0 ** -120

E = 128
GAP = 16            # rows of a never-referenced NaN segment of the row store
G = 256             # guard band of NaN elements in front of and behind every buffer
Case = collections.namedtuple("Case", "name n_q drugs tail_rows pi di Lq cols pitch")
# (a) the six layouts of tests/test_pgca_ragged_gpu.py (a tail with no lead; at a tile's start; ending tile 0; w = 1 across
#     tiles 0 and 1; inside tile 1; the model's own), 14 permuted pairs.  Expanded they have 504, 512, 512, 65, 508, 512
#     columns: with cols = 520 every drug shows zero fill; the pitches are multiples of 4 (16-byte stores)
# (b) no tail: 1, 40 and 512 keys, a partial query block, an odd pitch (4-byte stores throughout)
# (c) many workgroups resident at once: a tile read before its DMA has landed would show here
_A_DRUGS = ((8, 63.0), (16, 63.0), (64, 57.0), (65, 1.0), (100, 52.0), (136, 48.0))
_A_PI = (2, 0, 1, 0, 2, 2, 1, 0, 1, 2, 0, 1, 2, 0)
_A_DI = (5, 0, 3, 5, 1, 4, 0, 2, 2, 3, 4, 5, 0, 1)
CASES = {
    ("a_six_layouts", False): Case("a_six_layouts", 3, _A_DRUGS, 8, _A_PI, _A_DI, 256, 136, 144),
    ("a_six_layouts", True): Case("a_six_layouts", 3, _A_DRUGS, 8, _A_PI, _A_DI, 256, 520, 528),
    ("b_no_tail", True): Case("b_no_tail", 2, ((1, 1.0), (40, 5.0), (512, 1.0)), 0, (1, 0, 1, 0, 1), (0, 1, 2, 2, 1), 40, 513, 515),
    ("c_many_pairs", True): Case("c_many_pairs", 2, ((24, 61.0), (72, 55.0)), 8, tuple(i % 2 for i in range(300)),
                                 tuple((i // 2) % 2 for i in range(300)), 64, 504, 508),
}
PARAMS = [("a_six_layouts", BF, False), ("a_six_layouts", BF, True), ("a_six_layouts", F32, False), ("a_six_layouts", F32, True),
          ("b_no_tail", BF, True), ("b_no_tail", F32, True), ("c_many_pairs", BF, True)]


def _nan_view(n_ent, L, cols, dt, fill, dev):
    """(n_ent, L, cols) view of a NaN buffer with guard bands and one NaN spare entity behind; entities get `fill`."""
    es = L * cols
    flat = torch.full(((n_ent + 1) * es + 2 * G,), float("nan"), device=dev, dtype=dt)
    v = torch.as_strided(flat, (n_ent, L, cols), (es, cols, 1), G)
    v.copy_(fill)
    return v


def _drug_map(Q, K, t, w, expand, scale):
    """fp64 map of every query entity of Q (n_q, Lq, E) over one drug's keys K (Lk, E), tail (t, w): (map, bound, Lk_full, lam)
    with the map in the layout the call writes (n_q, Lq, columns of this drug)."""
    n_q, Lq, _ = Q.shape
    Lk = K.shape[0]
    ref = reference_fwd(Q, K, K, n_problems=n_q, n_heads=1, n_segments=1, partner_shift=0, Lq=Lq, Lk=Lk, head_dim=E, scale=scale,
                        q_strides=(Lq * E, E, E), k_strides=(0, E, E), v_strides=(0, E, E), key_tail=(t, w) if t else None)
    pm, lam = ref["Pm"][0][:, 0], ref["lam"][0][:, 0]                                # (n_q, Lq, Lk)
    lead = Lk - t
    lk_full = int(math.ceil(lead + t * w)) if t else Lk
    rel = (E + 2) * U_F * (lam + ref["mag_lse"][0][:, 0].unsqueeze(-1)) + (lk_full + 8) * U_F
    if expand and t:
        copies = int(w)
        assert copies == w
        pm = torch.cat([pm[..., :lead], (pm[..., lead:] / w).repeat(1, 1, copies)], -1)      # column lead + i t + j <- tail key j
        rel = torch.cat([rel[..., :lead], rel[..., lead:].repeat(1, 1, copies)], -1)
    return pm, MARGIN * pm * rel + FLOOR, lk_full, float(lam.max())


def build(name, dt, expand, dev=DEV):
    """Inputs of a case and its fp64 reference (computed once per (protein, drug), shared by the tests that use the case, never
    modified).

    Row store: the drugs' segments back to back with a NaN segment of GAP rows in front of the middle drug and one behind the
    last; `rows` is the view of the rows the call is told about (kv_total_rows), the allocation goes on for that last NaN
    segment.  Table: the case's n_kv entries, then (for the guard test, whose calls are told about n_kv + 4 drugs) an entry that
    runs one row past the declared store, an entry of 4 keys, the last drug's rows with a weight that makes its map 8 columns
    wider, the second-to-last drug's rows with weight 2.5, and a spare entry of NaN weight that no call is told about."""
    c = CASES[(name, expand)]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    scale = E ** -0.5
    n_kv = len(c.drugs)
    q = _nan_view(c.n_q, c.Lq, E, dt, torch.randn(c.n_q, c.Lq, E, generator=g) * 0.7, dev)
    row0, r = [], 0
    for d, (Lk, _) in enumerate(c.drugs):
        if d == n_kv // 2:
            r += GAP
        row0.append(r)
        r += Lk
    R = r                                                                     # the rows the call is told about
    flat = torch.full(((R + GAP) * 2 * E + 2 * G,), float("nan"), device=dev, dtype=dt)
    store = torch.as_strided(flat, (R + GAP, 2 * E), (2 * E, 1), G)
    for (Lk, _), r0 in zip(c.drugs, row0):
        store[r0:r0 + Lk].copy_(torch.cat([torch.randn(Lk, E, generator=g) * 0.7, torch.randn(Lk, E, generator=g)], dim=1))
    (lk_a, w_a), (lk_b, _) = c.drugs[-1], c.drugs[-2]
    t_row0 = torch.tensor(row0 + [R - 8 + 1, row0[0], row0[-1], row0[-2], 0], dtype=torch.int64, device=dev)
    t_keys = torch.tensor([d[0] for d in c.drugs] + [8, 4, lk_a, lk_b, 8], dtype=torch.int32, device=dev)
    t_w = torch.tensor([d[1] for d in c.drugs] + [2.0, 2.0, w_a + 2.0, 2.5, float("nan")], dtype=torch.float32, device=dev)
    pi = torch.tensor(c.pi, dtype=torch.int32, device=dev)
    di = torch.tensor(c.di, dtype=torch.int32, device=dev)
    n = len(c.pi)
    assert set(c.di) == set(range(n_kv)), "every drug of the case is used"
    want = torch.zeros(n, c.Lq, c.cols, dtype=torch.float64, device=dev)
    bound = torch.zeros_like(want)
    ncols = torch.zeros(n, dtype=torch.int64, device=dev)
    full = torch.zeros(n, dtype=torch.int64, device=dev)
    lam = 0.0
    for d, (Lk, w) in enumerate(c.drugs):                                     # per drug: every protein against its own rows
        pm, bd, lk_full, lm = _drug_map(q.contiguous(), store[row0[d]:row0[d] + Lk, :E].contiguous(), c.tail_rows, w, expand, scale)
        sel = (di == d).nonzero().flatten()
        k = pm.shape[-1]
        assert k <= c.cols
        want[sel, :, :k], bound[sel, :, :k] = pm[pi[sel].long()], bd[pi[sel].long()]
        ncols[sel], full[sel] = k, lk_full
        lam = max(lam, lm)
    return dict(c=c, dt=dt, expand=expand, scale=scale, q=q, rows=store[:R], n_kv=n_kv, row0=t_row0, keys=t_keys, w=t_w, pi=pi, di=di,
                n=n, want=want, bound=bound, ncols=ncols, full=full, lam=lam)


@functools.lru_cache(maxsize=None)
def _setup(name, dt, expand, dev=DEV):
    """build(), computed once per case and shared by the tests of this file, which never modify it."""
    return build(name, dt, expand, dev)


def _out_store(n, Lq, cols, pitch):
    """A NaN fp32 `out` buffer with guard bands: (flat, view (n, Lq, cols) at the pitch, mask of the addressed elements)."""
    n_el = n * Lq * pitch
    flat = torch.full((n_el + 2 * G,), float("nan"), device=DEV, dtype=F32)
    mask = torch.zeros(n_el + 2 * G, dtype=torch.bool, device=DEV)
    shape, st = (n, Lq, cols), (Lq * pitch, pitch, 1)
    torch.as_strided(mask, shape, st, G).fill_(True)
    return flat, torch.as_strided(flat, shape, st, G), mask


def _bits(t):
    return t.view(torch.int32).clone()


def _run(s, di=None, n_kv=None):
    from druglamp_amd import ops
    c = s["c"]
    n_kv = s["n_kv"] if n_kv is None else n_kv
    flat, out, mask = _out_store(s["n"], c.Lq, c.cols, c.pitch)
    before = _bits(flat)
    got = ops.pgca_pairs_ragged_probs(s["q"], s["rows"], s["row0"][:n_kv], s["keys"][:n_kv], s["w"][:n_kv], s["pi"],
                                      s["di"] if di is None else di, scale=s["scale"], key_tail_rows=c.tail_rows, cols=c.cols,
                                      expand_tail=s["expand"], out=out)
    assert got is out
    torch.cuda.synchronize()
    return flat, out, mask, before


def _check(what, got, want, bound, ncols, full, sums, pairs=None):
    """Worst |err| / bound and worst row-sum deviation over `pairs` (all), printed before they are asserted; the zero-fill
    columns bitwise +0.0."""
    idx = torch.arange(got.shape[0], device=got.device) if pairs is None else pairs
    g, w, b = got[idx], want[idx], bound[idx]
    assert torch.isfinite(g).all(), "%s: addressed elements left unwritten or non-finite" % what
    fill = torch.arange(g.shape[-1], device=g.device).view(1, 1, -1) >= ncols[idx].view(-1, 1, 1)
    assert bool((_bits(g.contiguous())[fill.expand_as(g)] == 0).all()), "%s: a zero-fill column is not +0.0" % what
    gd = g.double()
    ratio = float(((gd - w).abs() / b)[~fill.expand_as(g)].max())
    print("%s: worst |err| / bound = %.4g" % (what, ratio))
    assert ratio <= 1.0, "%s: exceeds its rounding bound by x%.3g" % (what, ratio)
    if sums:                                            # an expanded or tail-less map: rows sum to 1
        dev = (gd.sum(-1) - 1.0).abs()
        lim = (full[idx].double().view(-1, 1) + 8) * U_F + b.sum(-1)
        rs = float((dev / lim).max())
        print("%s: worst |row sum - 1| / limit = %.4g" % (what, rs))
        assert rs <= 1.0, "%s: a row sums to 1 +- %.3g (allowed x%.3g)" % (what, float(dev.max()), rs)


def _name(s):
    return "pgca_pairs_ragged_probs %s %s %s" % (s["c"].name, "expanded" if s["expand"] else "distinct", str(s["dt"]).split(".")[1])


@pytest.mark.parametrize("name,dt,expand", PARAMS, ids=["%s-%s-%s" % (n, str(d).split(".")[1], "expanded" if e else "distinct") for n, d, e in PARAMS])
def test_ragged_maps_against_fp64(name, dt, expand):
    from druglamp_amd import ops
    s = _setup(name, dt, expand)
    c = s["c"]
    assert s["lam"] <= LAM, "%s: logits beyond the range the bound assumes" % name
    word = ops.guard_flags(DEV)
    word.zero_()
    flat, out, mask, before = _run(s)
    assert int(word.item()) == 0
    _check(_name(s), out, s["want"], s["bound"], s["ncols"], s["full"], sums=expand or not c.tail_rows)
    # nothing at or beyond column `cols` of a row, nothing outside the rows
    assert torch.equal(_bits(flat)[~mask], before[~mask]), "%s: a store outside the addressed elements" % name
    assert torch.equal(_bits(_run(s)[0]), _bits(flat)), "%s: two calls differ" % name
    if expand and name == "a_six_layouts":                                # the case does show zero fill on every drug
        assert s["ncols"].max() == 512 and sorted(set(s["ncols"].tolist())) == [65, 504, 508, 512] and c.cols == 520


def test_unfit_pairs_are_skipped_and_flagged():
    """On the allocation of case (a), expanded, told about 10 drugs: one pair names drug 10 (the NaN spare table entry, inside the
    allocation); one names drug 6, whose entry ends one row behind the declared store (the allocation goes on for a NaN
    segment); one names drug 7, whose entry has 4 keys < key_tail_rows; one names drug 8 — the model-layout drug's rows at
    weight 50: 528 columns > out_cols = 520; one names drug 9 — real rows at weight 2.5.  So even a missing guard reads inside
    real allocations.  The five pairs' rows stay bitwise unchanged, exactly the three flag bits are set and named, every other
    pair meets its bound."""
    from druglamp_amd import _lib, ops
    s = _setup("a_six_layouts", BF, True)
    c = s["c"]
    word = ops.guard_flags(DEV)
    word.zero_()
    bad = {4: 10, 7: 6, 11: 7, 12: 8, 10: 9}
    di = s["di"].clone()
    for n, d in bad.items():
        di[n] = d
    try:
        flat, out, mask, before = _run(s, di=di, n_kv=10)
        bits = int(word.item())
    finally:
        word.zero_()
    assert bits == _lib.FLAG_PAIR_INDEX | _lib.FLAG_KEY_TABLE | _lib.FLAG_MAP_COLS, bits
    text = ops.guard_text(bits)
    assert "dl_pgca_pairs_fwd" in text and "key table" in text and "does not fit" in text and text.count("skipped") == 3
    for n in bad:
        lo, hi = G + n * c.Lq * c.pitch, G + (n + 1) * c.Lq * c.pitch
        assert torch.equal(_bits(flat)[lo:hi], before[lo:hi]), "the skipped pair %d's rows were written" % n
    assert torch.equal(_bits(flat)[~mask], before[~mask])
    others = torch.tensor([i for i in range(s["n"]) if i not in bad], device=DEV)
    _check(_name(s) + " +guards", out, s["want"], s["bound"], s["ncols"], s["full"], sums=True, pairs=others)
    assert int(word.item()) == 0


@pytest.mark.parametrize("d,expand,flag", [(6, True, "FLAG_KEY_TABLE"), (7, True, "FLAG_KEY_TABLE"), (8, True, "FLAG_MAP_COLS"),
                                           (9, True, "FLAG_MAP_COLS"), (9, False, None)])
def test_each_unfit_entry_alone_sets_only_its_flag(d, expand, flag):
    """(The weight-2.5 entry is a valid drug where no copy is asked for: a tail column then carries the mass of 2.5 keys.)"""
    from druglamp_amd import _lib, ops
    s = _setup("a_six_layouts", BF, expand)
    word = ops.guard_flags(DEV)
    word.zero_()
    di = s["di"].clone()
    di[0] = d
    try:
        _, out, _, _ = _run(s, di=di, n_kv=10)
        bits = int(word.item())
    finally:
        word.zero_()
    assert bits == (getattr(_lib, flag) if flag else 0), (d, bits)
    assert bool(torch.isnan(out[0]).all()) == (flag is not None)


@pytest.mark.parametrize("expand", [True, False], ids=["expanded", "distinct"])
def test_dense_entry_point_against_fp64(expand):
    """(3, 72, 256) codes with key_tail = (8, 3.0): 64 + 24 = 88 columns expanded (cols = 92: zero fill), 72 distinct; Lq = 40 is
    a partial query block; a pitch of 100."""
    from druglamp_amd import ops
    g = torch.Generator().manual_seed(7203)
    n_q, n_kv, Lq, Lk, t, w = 2, 3, 40, 72, 8, 3.0
    cols, pitch = (92, 100) if expand else (72, 100)
    q = _nan_view(n_q, Lq, E, BF, torch.randn(n_q, Lq, E, generator=g) * 0.7, DEV)
    kv = _nan_view(n_kv, Lk, 2 * E, BF, torch.cat([torch.randn(n_kv, Lk, E, generator=g) * 0.7, torch.randn(n_kv, Lk, E, generator=g)], 2), DEV)
    pi = torch.tensor((0, 1, 1, 0, 1), dtype=torch.int32, device=DEV)
    di = torch.tensor((2, 0, 1, 1, 2), dtype=torch.int32, device=DEV)
    n = pi.numel()
    want = torch.zeros(n, Lq, cols, dtype=torch.float64, device=DEV)
    bound = torch.zeros_like(want)
    lam = 0.0
    for d in range(n_kv):
        pm, bd, lk_full, lm = _drug_map(q.contiguous(), kv[d, :, :E].contiguous(), t, w, expand, E ** -0.5)
        sel = (di == d).nonzero().flatten()
        want[sel, :, :pm.shape[-1]], bound[sel, :, :pm.shape[-1]] = pm[pi[sel].long()], bd[pi[sel].long()]
        lam = max(lam, lm)
    assert lam <= LAM
    ncols = torch.full((n,), 88 if expand else 72, dtype=torch.int64, device=DEV)
    full = torch.full((n,), 88, dtype=torch.int64, device=DEV)
    runs = []
    for _ in range(2):
        flat, out, mask = _out_store(n, Lq, cols, pitch)
        before = _bits(flat)
        got = ops.pgca_pairs_probs(q, kv, pi, di, scale=E ** -0.5, key_tail=(t, w), expand_tail=expand, cols=cols, out=out)
        torch.cuda.synchronize()
        assert got is out and torch.equal(_bits(flat)[~mask], before[~mask])
        runs.append(_bits(flat))
    assert torch.equal(runs[0], runs[1])
    _check("pgca_pairs_probs dense %s" % ("expanded" if expand else "distinct"), out, want, bound, ncols, full, sums=expand)
    # cols defaults to the map's own column count
    own = ops.pgca_pairs_probs(q, kv, pi, di, scale=E ** -0.5, key_tail=(t, w), expand_tail=expand)
    assert own.shape == (n, Lq, 88 if expand else 72) and own.dtype == F32
    assert torch.equal(_bits(own), _bits(out[:, :, :own.shape[2]].contiguous()))


@pytest.mark.parametrize("dt", [BF, F32], ids=["bfloat16", "float32"])
def test_dense_and_ragged_entry_points_agree_bitwise_on_a_uniform_store(dt):
    """Both entry points launch one kernel that differs only in where a workgroup finds its keys, so on a store whose drugs all
    have Lk = 72 keys the two must give the same bits: `kv` as (3, 72, 256) for the dense entry point, the same memory as
    (216, 256) with row0 = (0, 72, 144) for the ragged one.  Weight 1 and no tail rows: the dense tail bias is a host logf and
    the ragged one a device logf, and equality is only guaranteed where both are exactly 0 (tests/test_pgca_ragged_gpu.py)."""
    from druglamp_amd import ops
    g = torch.Generator().manual_seed(72)
    n_q, n_kv, Lq, Lk = 2, 3, 40, 72
    q = (torch.randn(n_q, Lq, E, generator=g) * 0.7).to(DEV, dt)
    kv = torch.cat([torch.randn(n_kv, Lk, E, generator=g) * 0.7, torch.randn(n_kv, Lk, E, generator=g)], dim=2).to(DEV, dt)
    pi = torch.tensor((0, 1, 1, 0, 1), dtype=torch.int32, device=DEV)
    di = torch.tensor((2, 0, 1, 1, 2), dtype=torch.int32, device=DEV)
    dense = ops.pgca_pairs_probs(q, kv, pi, di, scale=E ** -0.5, cols=80)
    row0 = torch.arange(n_kv, dtype=torch.int64, device=DEV) * Lk
    n_keys = torch.full((n_kv,), Lk, dtype=torch.int32, device=DEV)
    w = torch.ones(n_kv, dtype=torch.float32, device=DEV)
    ragged = ops.pgca_pairs_ragged_probs(q, kv.view(n_kv * Lk, 2 * E), row0, n_keys, w, pi, di, scale=E ** -0.5, key_tail_rows=0, cols=80)
    torch.cuda.synchronize()
    assert dense.shape == ragged.shape == (5, Lq, 80) and torch.isfinite(dense).all() and bool((dense[:, :, 72:] == 0).all())
    assert float((dense.double().sum(-1) - 1).abs().max()) <= 1e-5
    assert torch.equal(_bits(dense), _bits(ragged))


def test_host_tensors_a_small_out_and_a_wrong_table_are_rejected():
    from druglamp_amd import ops
    s = _setup("b_no_tail", BF, True)
    c, k = s["c"], s["n_kv"]
    q, rows, tab = s["q"], s["rows"], (s["row0"][:k], s["keys"][:k], s["w"][:k])
    kw = dict(scale=s["scale"], key_tail_rows=0, cols=c.cols)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_ragged_probs(q.cpu(), rows, *tab, s["pi"], s["di"], **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_ragged_probs(q, rows, tab[0].cpu(), tab[1], tab[2], s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="out must be"):                 # bf16 rows cannot take an fp32 map
        ops.pgca_pairs_ragged_probs(q, rows, *tab, s["pi"], s["di"], out=torch.empty(s["n"], c.Lq, c.cols, device=DEV, dtype=BF), **kw)
    with pytest.raises(ValueError, match="out must be"):                 # rows of 512 columns cannot take 513
        ops.pgca_pairs_ragged_probs(q, rows, *tab, s["pi"], s["di"], out=torch.empty(s["n"], c.Lq, 512, device=DEV), **kw)
    with pytest.raises(ValueError, match="key table"):                   # row0 must be int64
        ops.pgca_pairs_ragged_probs(q, rows, tab[0].int(), tab[1], tab[2], s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="key table"):                   # n_keys must be int32
        ops.pgca_pairs_ragged_probs(q, rows, tab[0], tab[1].long(), tab[2], s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="key table"):                   # tail_weight must be float32
        ops.pgca_pairs_ragged_probs(q, rows, tab[0], tab[1], tab[2].double(), s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="cols"):
        ops.pgca_pairs_ragged_probs(q, rows, *tab, s["pi"], s["di"], scale=s["scale"], key_tail_rows=0, cols=0)
    with pytest.raises(RuntimeError, match="does not fit"):              # the dense column count is checked on the host
        ops.pgca_pairs_probs(q, rows[:80].view(2, 40, 256), s["pi"][:2], s["pi"][:2], scale=s["scale"], cols=39)
