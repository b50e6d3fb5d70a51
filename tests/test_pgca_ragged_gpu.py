"""dl_pgca_pairs_ragged_fwd (csrc/pgca_pairs.hip, RaggedKeys) through ops.pgca_pairs_ragged, element-wise against the fp64 reference of
tests/attn_ref.py run per pair on the explicitly gathered Q[pi] and that drug's own rows, Lk_d and (key_tail_rows, w_d).

Bound: |O - ref| <= tau_O (mag_O + |bias|), the rounding model written out in tests/test_attention_paths_gpu.py and restated
in tests/test_pgca_pairs_gpu.py (same constants below): the kernel performs the arithmetic of pgca_pairs_kernel — only where a
workgroup finds its keys differs — so no new tolerance is invented.  The bound assumes logits lam <= 96; every case asserts it
(at input scale 0.7 and the largest weight, 63, the fp64 reference alone gives lam < 10: checked without a device through
_setup(name, dt, "cpu")).  The left copy is compared bitwise.

Every buffer is NaN outside the addressed elements: inputs (a stray read poisons the result), `out` (every addressed element
must be overwritten, every other element must stay bitwise unchanged), and the row store carries a never-referenced NaN
segment between two drugs and one behind the rows the call is told about.

DL_PGCA_BOUND_LOG=<file>: every check appends one JSON line (case, dtype, worst |err| / bound).
"""
import collections
import functools
import json
import os

import pytest
import torch

from tests.attn_ref import reference_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32

# ---- rounding model (tests/test_attention_paths_gpu.py, tests/test_pgca_pairs_gpu.py: same constants) -----------------------
U_B, U_F = 2.0 ** -8, 2.0 ** -24
LAM, HD, LEN, MARGIN = 96.0, 128, 2048, 2.0
E_S = (HD + 2) * U_F * LAM
E_LSE = E_S + (LEN + 4) * U_F
TAU_O = {BF: MARGIN * (2 * U_B + E_S + E_LSE + LEN * U_F), F32: MARGIN * (E_S + E_LSE + (LEN + 2) * U_F)}

E = 128
GAP = 16            # rows of a never-referenced NaN segment of the row store
G = 256             # guard band of NaN elements in front of and behind every buffer
Case = collections.namedtuple("Case", "name n_q drugs tail_rows pi di Lq left_cols pitch bias")
# (a) a tail with no lead; a tail that is a whole first tile's start; a tail that ends tile 0 exactly; a tail (w = 1) that
#     straddles tiles 0 and 1; a tail inside tile 1; the model's own layout.  14 pairs, permuted and repeated: neighbouring
#     workgroups differ in tile count (1, 1, 1, 2, 2, 3 tiles)
_A_DRUGS = ((8, 63.0), (16, 63.0), (64, 57.0), (65, 1.0), (100, 52.0), (136, 48.0))
_A_PI = (2, 0, 1, 0, 2, 2, 1, 0, 1, 2, 0, 1, 2, 0)
_A_DI = (5, 0, 3, 5, 1, 4, 0, 2, 2, 3, 4, 5, 0, 1)
CASES = {
    "a_six_layouts": Case("a_six_layouts", 3, _A_DRUGS, 8, _A_PI, _A_DI, 256, 128, 256, True),
    "b_no_tail": Case("b_no_tail", 2, ((1, 1.0), (40, 5.0), (512, 1.0)), 0, (1, 0, 1, 0, 1), (0, 1, 2, 2, 1), 40, 0, 136, False),
    "c_many_pairs": Case("c_many_pairs", 2, ((24, 61.0), (72, 55.0)), 8, tuple(i % 2 for i in range(300)),
                         tuple((i // 2) % 2 for i in range(300)), 64, 128, 256, False),
}
PARAMS = [("a_six_layouts", BF), ("a_six_layouts", F32), ("b_no_tail", BF), ("b_no_tail", F32), ("c_many_pairs", BF)]


def _nan_view(n_ent, L, cols, dt, fill, dev):
    """(n_ent, L, cols) view of a NaN buffer with guard bands and one NaN spare entity behind; entities get `fill`."""
    es = L * cols
    flat = torch.full(((n_ent + 1) * es + 2 * G,), float("nan"), device=dev, dtype=dt)
    v = torch.as_strided(flat, (n_ent, L, cols), (es, cols, 1), G)
    v.copy_(fill)
    return v


def build(name, dt, dev=DEV):
    """Inputs of a case and its fp64 reference (computed once, shared by the tests that use the case, never modified).

    Row store: the drugs' segments back to back with a NaN segment of GAP rows in front of the middle drug and one behind the
    last; `rows` is the view of the rows the call is told about (kv_total_rows), the allocation goes on for that last NaN
    segment.  Table: the case's n_kv entries, then (for the guard test) an entry that runs one row past the declared store,
    an entry of 4 keys, and a spare entry of NaN weight that no call is told about."""
    c = CASES[name]
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
    t_row0 = torch.tensor(row0 + [R - 8 + 1, row0[0], 0], dtype=torch.int64, device=dev)
    t_keys = torch.tensor([d[0] for d in c.drugs] + [8, 4, 8], dtype=torch.int32, device=dev)
    t_w = torch.tensor([d[1] for d in c.drugs] + [2.0, 2.0, float("nan")], dtype=torch.float32, device=dev)
    left = _nan_view(c.n_q, c.Lq, c.left_cols, dt, torch.randn(c.n_q, c.Lq, c.left_cols, generator=g), dev) if c.left_cols else None
    bias = (torch.randn(E, generator=g) * 0.5).to(dev) if c.bias else None
    pi = torch.tensor(c.pi, dtype=torch.int32, device=dev)
    di = torch.tensor(c.di, dtype=torch.int32, device=dev)
    n = len(c.pi)
    O = torch.zeros(n, c.Lq, E, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(O)
    lam = 0.0
    for d, (Lk, w) in enumerate(c.drugs):                                     # per drug: its pairs against its own rows
        sel = (di == d).nonzero().flatten()
        if not sel.numel():
            continue
        Qg = q[pi[sel].long()].contiguous()
        Kd, Vd = store[row0[d]:row0[d] + Lk, :E].contiguous(), store[row0[d]:row0[d] + Lk, E:].contiguous()
        ref = reference_fwd(Qg, Kd, Vd, n_problems=sel.numel(), n_heads=1, n_segments=1, partner_shift=0, Lq=c.Lq, Lk=Lk, head_dim=E,
                            scale=scale, q_strides=(c.Lq * E, E, E), k_strides=(0, E, E), v_strides=(0, E, E),
                            key_tail=(c.tail_rows, w) if c.tail_rows else None)
        O[sel], mag[sel] = ref["O"][0, :, 0], ref["mag_O"][0, :, 0]
        lam = max(lam, float(ref["lam"][0].max()))
    if bias is not None:
        O, mag = O + bias.double(), mag + bias.double().abs()
    assert set(c.di) == set(range(n_kv)), "every drug of the case is used"
    return dict(c=c, dt=dt, scale=scale, q=q, rows=store[:R], n_kv=n_kv, row0=t_row0, keys=t_keys, w=t_w, left=left, bias=bias,
                pi=pi, di=di, n=n, O=O, bound=TAU_O[dt] * mag + 1e-300, lam=lam)


@functools.lru_cache(maxsize=None)
def _setup(name, dt, dev=DEV):
    """build(), computed once per case and shared by the tests of this file, which never modify it."""
    return build(name, dt, dev)


def _out_store(s):
    """A NaN `out` buffer with guard bands: (flat, view (n, Lq, cols) at the case's pitch, mask of the addressed elements)."""
    c = s["c"]
    cols = c.left_cols + E
    n_el = s["n"] * c.Lq * c.pitch
    flat = torch.full((n_el + 2 * G,), float("nan"), device=DEV, dtype=s["dt"])
    mask = torch.zeros(n_el + 2 * G, dtype=torch.bool, device=DEV)
    shape, st = (s["n"], c.Lq, cols), (c.Lq * c.pitch, c.pitch, 1)
    torch.as_strided(mask, shape, st, G).fill_(True)
    return flat, torch.as_strided(flat, shape, st, G), mask


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32).clone()


def _run(s, di=None, n_kv=None):
    from druglamp_amd import ops
    c = s["c"]
    n_kv = s["n_kv"] if n_kv is None else n_kv
    flat, out, mask = _out_store(s)
    before = _bits(flat)
    got = ops.pgca_pairs_ragged(s["q"], s["rows"], s["row0"][:n_kv], s["keys"][:n_kv], s["w"][:n_kv], s["pi"], s["di"] if di is None else di,
                                scale=s["scale"], key_tail_rows=c.tail_rows, left=s["left"], bias=s["bias"], out=out)
    assert got is out
    torch.cuda.synchronize()
    return flat, out, mask, before


def _check(s, out, pairs=None, tag=""):
    """Worst |err| / bound over the attention columns of `pairs` (all), printed and logged before it is asserted; the left
    columns bitwise."""
    c = s["c"]
    idx = torch.arange(s["n"], device=DEV) if pairs is None else pairs
    got = out[idx][:, :, c.left_cols:].double()
    assert torch.isfinite(got).all(), "%s: non-finite addressed elements" % c.name
    ratio = float(((got - s["O"][idx]).abs() / s["bound"][idx]).max())
    print("pgca_pairs_ragged %s%s %s: worst |err| / bound = %.4f (lam %.2f)" % (c.name, tag, str(s["dt"]).split(".")[1], ratio, s["lam"]))
    path = os.environ.get("DL_PGCA_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": "ragged_" + c.name + tag, "dtype": str(s["dt"]).split(".")[1], "ratio": ratio}) + "\n")
    assert ratio <= 1.0, "%s: O exceeds its rounding bound by x%.3g" % (c.name, ratio)
    if c.left_cols:
        want = s["left"][s["pi"].long()[idx]]
        assert torch.equal(_bits(out[idx][:, :, :c.left_cols].contiguous()), _bits(want.contiguous())), "%s: left copy differs" % c.name


@pytest.mark.parametrize("name,dt", PARAMS, ids=["%s-%s" % (n, str(d).split(".")[1]) for n, d in PARAMS])
def test_pgca_pairs_ragged_against_fp64(name, dt):
    s = _setup(name, dt)
    assert s["lam"] <= LAM, "%s: logits beyond the range the bound assumes" % name
    flat, out, mask, before = _run(s)
    _check(s, out)
    # nothing outside the addressed columns of the addressed rows was written (case b: nothing beyond column 127 of a 136-pitch row)
    assert torch.equal(_bits(flat)[~mask], before[~mask]), "%s: a store outside the addressed elements" % name
    if name == "b_no_tail":
        assert torch.isnan(torch.as_strided(flat, (s["n"] * s["c"].Lq, 8), (136, 1), G + 128)).all()


def test_bad_index_and_bad_table_entries_are_skipped_and_flagged():
    """On the allocation of case (a), told about 8 drugs: one pair names drug 8 — the NaN spare table entry, inside the
    allocation; one names drug 6, whose entry ends one row behind the declared store (the allocation goes on for a NaN
    segment); one names drug 7, whose entry has 4 keys < key_tail_rows.  So even a missing guard reads inside real
    allocations.  The three pairs' rows stay bitwise unchanged, both flag bits are set and named, every other pair meets
    its bound."""
    from druglamp_amd import _lib, ops
    s = _setup("a_six_layouts", BF)
    c = s["c"]
    word = ops.guard_flags(DEV)
    word.zero_()
    bad = {4: 8, 7: 6, 11: 7}
    di = s["di"].clone()
    for n, d in bad.items():
        di[n] = d
    try:
        flat, out, mask, before = _run(s, di=di, n_kv=8)
        bits = int(word.item())
    finally:
        word.zero_()
    assert bits & _lib.FLAG_PAIR_INDEX and bits & _lib.FLAG_KEY_TABLE and bits == _lib.FLAG_PAIR_INDEX | _lib.FLAG_KEY_TABLE
    text = ops.guard_text(bits)
    assert "dl_pgca_pairs_fwd" in text and "key table" in text and text.count("skipped") == 2
    for n in bad:
        lo, hi = G + n * c.Lq * c.pitch, G + (n + 1) * c.Lq * c.pitch
        assert torch.equal(_bits(flat)[lo:hi], before[lo:hi]), "the skipped pair %d's rows were written" % n
    assert torch.equal(_bits(flat)[~mask], before[~mask])
    others = torch.tensor([i for i in range(s["n"]) if i not in bad], device=DEV)
    _check(s, out, pairs=others, tag="+guards")
    assert int(word.item()) == 0


def test_each_bad_table_entry_alone_sets_only_the_table_flag():
    from druglamp_amd import _lib, ops
    s = _setup("a_six_layouts", BF)
    word = ops.guard_flags(DEV)
    for d in (6, 7):
        word.zero_()
        di = s["di"].clone()
        di[0] = d
        try:
            _run(s, di=di, n_kv=8)
            bits = int(word.item())
        finally:
            word.zero_()
        assert bits == _lib.FLAG_KEY_TABLE, (d, bits)


def test_two_calls_are_bitwise_identical():
    s = _setup("a_six_layouts", BF)
    a, b = _run(s)[0], _run(s)[0]
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dt", [BF, F32], ids=["bfloat16", "float32"])
def test_dense_and_ragged_entry_points_agree_bitwise_on_a_uniform_store(dt):
    """dl_pgca_pairs_fwd and dl_pgca_pairs_ragged_fwd launch one kernel that differs only in where a workgroup finds its keys, so
    on a store whose drugs all have Lk = 72 keys (two key tiles, the second partial) the two must give the same bits: `kv` as
    (3, 72, 256) for the dense entry point, the same memory as (216, 256) with row0 = (0, 72, 144) for the ragged one.  Lq = 40
    is a partial query block in both dtypes.  Weight 1 and no tail rows: the dense tail bias is a host logf and the ragged one
    a device logf, and equality is only guaranteed where both are exactly 0."""
    from druglamp_amd import ops
    g = torch.Generator().manual_seed(72)
    n_q, n_kv, Lq, Lk = 2, 3, 40, 72
    q = (torch.randn(n_q, Lq, E, generator=g) * 0.7).to(DEV, dt)
    kv = torch.cat([torch.randn(n_kv, Lk, E, generator=g) * 0.7, torch.randn(n_kv, Lk, E, generator=g)], dim=2).to(DEV, dt)
    left = torch.randn(n_q, Lq, 128, generator=g).to(DEV, dt)
    bias = (torch.randn(E, generator=g) * 0.5).to(DEV)
    pi = torch.tensor((0, 1, 1, 0, 1), dtype=torch.int32, device=DEV)
    di = torch.tensor((2, 0, 1, 1, 2), dtype=torch.int32, device=DEV)
    dense = ops.pgca_pairs(q, kv, pi, di, scale=E ** -0.5, left=left, bias=bias)
    row0 = torch.arange(n_kv, dtype=torch.int64, device=DEV) * Lk
    n_keys = torch.full((n_kv,), Lk, dtype=torch.int32, device=DEV)
    w = torch.ones(n_kv, dtype=torch.float32, device=DEV)
    ragged = ops.pgca_pairs_ragged(q, kv.view(n_kv * Lk, 2 * E), row0, n_keys, w, pi, di, scale=E ** -0.5, key_tail_rows=0, left=left, bias=bias)
    torch.cuda.synchronize()
    assert dense.shape == ragged.shape == (5, Lq, 128 + E) and torch.isfinite(dense.float()).all()
    assert torch.equal(_bits(dense), _bits(ragged))


def test_host_tensors_a_small_out_and_a_wrong_table_are_rejected():
    from druglamp_amd import ops
    s = _setup("b_no_tail", BF)
    c, k = s["c"], s["n_kv"]
    q, rows, tab = s["q"], s["rows"], (s["row0"][:k], s["keys"][:k], s["w"][:k])
    kw = dict(scale=s["scale"], key_tail_rows=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_ragged(q.cpu(), rows, *tab, s["pi"], s["di"], **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_ragged(q, rows, tab[0].cpu(), tab[1], tab[2], s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="out must be"):
        ops.pgca_pairs_ragged(q, rows, *tab, s["pi"], s["di"], out=torch.empty(s["n"], c.Lq - 1, E, device=DEV, dtype=BF), **kw)
    with pytest.raises(ValueError, match="out must be"):                 # rows of 120 columns cannot take 128
        ops.pgca_pairs_ragged(q, rows, *tab, s["pi"], s["di"], out=torch.empty(s["n"], c.Lq, 120, device=DEV, dtype=BF), **kw)
    with pytest.raises(ValueError, match="key table"):                   # row0 must be int64
        ops.pgca_pairs_ragged(q, rows, tab[0].int(), tab[1], tab[2], s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="key table"):                   # n_keys must be int32
        ops.pgca_pairs_ragged(q, rows, tab[0], tab[1].long(), tab[2], s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="key table"):                   # tail_weight must be float32
        ops.pgca_pairs_ragged(q, rows, tab[0], tab[1], tab[2].double(), s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="key table"):                   # one length
        ops.pgca_pairs_ragged(q, rows, tab[0], tab[1][:k - 1], tab[2], s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="key_tail_rows"):
        ops.pgca_pairs_ragged(q, rows, *tab, s["pi"], s["di"], scale=s["scale"], key_tail_rows=-8)
