"""dl_pgca_pairs_profile / dl_pgca_pairs_ragged_profile (csrc/pgca_pairs_profile.hip) through ops.pgca_pairs_profile and
ops.pgca_pairs_ragged_profile, element-wise against the fp64 reference of tests/attn_ref.py reduced as tests/profile_ref.py defines
(bounds there: no new tolerance).  The inputs, the fp64 maps and their element bounds are the expanded cases of
tests/test_pgca_pairs_probs_gpu.py (_setup: computed once per case and shared with the map tests, never modified):
    a  six ragged layouts (a tail with no lead; at a tile's start; ending tile 0; w = 1 across two tiles; inside tile 1; the
       model's own), 3 proteins, 14 permuted pairs, Lq 256 (a workgroup's query block is 256 rows in bf16 and 128 in fp32: one
       block in bf16, two in fp32), cols 520: every drug shows zero fill
    b  no tail: 1, 40 and 512 keys, Lq 40 (a partial block, no multiple of 16: rows >= Lq must not enter the sums), cols 513
       at an odd pitch
    c  300 pairs over two drugs of 24 and 72 keys, Lq 64: many workgroups resident (a tile read before its DMA landed)
    d  (registered here) bf16 with Lq 300: two query blocks of which the second is partial, so the cross-block sum and the
       restart of the tile pipeline are exercised in bf16 as (a) exercises them in fp32; drugs of 40 and 136 keys, cols 520
Every case asserts lam <= 96 (the fp64 reference alone gives lam < 10: tests/test_pgca_pairs_profile_cpu.py), prints its worst
|err| / bound before asserting it, and runs twice; the two runs must agree bitwise.

Buffers: Q and the row store are NaN outside the addressed elements (a never-referenced NaN segment between two drugs and one
behind the declared rows: _setup); the three outputs are NaN with guard bands and pitches above their widths.  Every addressed
element — the zero fill of key_mass included, exactly +0.0 — must be overwritten, everything else must stay bitwise unchanged.
"""
import pytest
import torch

from tests.profile_ref import profile_ref, site_key_slack
from tests.test_pgca_pairs_probs_gpu import BF, CASES, DEV, F32, LAM, Case, E, G, _bits, _setup

pytestmark = pytest.mark.gpu
SITE_PAD = 5          # the site outputs' pitch is Lq + SITE_PAD (odd for every case)
# case (d) goes through the map tests' _setup like the others: it is added to that table (nothing there iterates over it)
CASES.setdefault(("d_two_blocks", True), Case("d_two_blocks", 2, ((40, 60.0), (136, 48.0)), 8, (1, 0, 0, 1, 0), (0, 1, 0, 1, 1), 300, 520, 524))
PARAMS = [("a_six_layouts", BF), ("a_six_layouts", F32), ("b_no_tail", BF), ("b_no_tail", F32), ("c_many_pairs", BF), ("d_two_blocks", BF)]


def _nan_rows(n, width, pitch):
    """A NaN fp32 buffer with guard bands: (flat, view (n, width) at the pitch, mask of the addressed elements)."""
    flat = torch.full((n * pitch + 2 * G,), float("nan"), device=DEV, dtype=F32)
    mask = torch.zeros(n * pitch + 2 * G, dtype=torch.bool, device=DEV)
    torch.as_strided(mask, (n, width), (pitch, 1), G).fill_(True)
    return flat, torch.as_strided(flat, (n, width), (pitch, 1), G), mask


def _run(s, di=None, n_kv=None):
    """One call on fresh NaN outputs: [(flat, view, mask, bits before)] for key_mass, site_peak, site_key (the int32 output lives
    in a NaN-patterned buffer too)."""
    from druglamp_amd import ops
    c = s["c"]
    n_kv = s["n_kv"] if n_kv is None else n_kv
    bufs = [_nan_rows(s["n"], c.cols, c.pitch), _nan_rows(s["n"], c.Lq, c.Lq + SITE_PAD), _nan_rows(s["n"], c.Lq, c.Lq + SITE_PAD)]
    before = [_bits(b[0]) for b in bufs]
    out = (bufs[0][1], bufs[1][1], bufs[2][1].view(torch.int32))
    got = ops.pgca_pairs_ragged_profile(s["q"], s["rows"], s["row0"][:n_kv], s["keys"][:n_kv], s["w"][:n_kv], s["pi"],
                                        s["di"] if di is None else di, scale=s["scale"], key_tail_rows=c.tail_rows, cols=c.cols, out=out)
    assert all(g is o for g, o in zip(got, out))
    torch.cuda.synchronize()
    return [(b[0], o, b[2], bf) for b, o, bf in zip(bufs, out, before)]


@pytest.fixture(scope="module")
def refs():
    """{(case, dtype): the reduced fp64 reference} — computed once, never modified."""
    cache = {}

    def get(name, dt):
        if (name, dt) not in cache:
            s = _setup(name, dt, True)
            cache[(name, dt)] = profile_ref(s["want"], s["bound"])
        return cache[(name, dt)]
    return get


def _check(what, s, ref, res, pairs=None):
    """Worst |err| / bound of the three outputs over `pairs` (all), printed before they are asserted."""
    km, km_b, peak, peak_b, _ = ref
    idx = torch.arange(s["n"], device=DEV) if pairs is None else pairs
    mass, pk, sk = (r[1][idx] for r in res)
    assert torch.isfinite(mass).all() and torch.isfinite(pk).all(), "%s: addressed elements left unwritten or non-finite" % what
    fill = torch.arange(mass.shape[-1], device=DEV).view(1, -1) >= s["ncols"][idx].view(-1, 1)
    assert bool((_bits(mass.contiguous())[fill] == 0).all()), "%s: a zero-fill column of key_mass is not +0.0" % what
    md = mass.double()
    r_mass = float(((md - km[idx]).abs() / km_b[idx])[~fill].max())
    r_sum = float(((md.sum(-1) - 1.0).abs() / km_b[idx].sum(-1)).max())
    r_peak = float(((pk.double() - peak[idx]).abs() / peak_b[idx]).max())
    slack, in_range = site_key_slack(s["want"][idx], s["bound"][idx], sk, s["keys"][s["di_used"][idx].long()].view(-1, 1))
    print("%s: worst |err| / bound: key_mass %.4g, its row sum %.4g, site_peak %.4g; least site_key slack %.4g"
          % (what, r_mass, r_sum, r_peak, float(slack.min())))
    assert r_mass <= 1.0, "%s: key_mass exceeds its rounding bound by x%.3g" % (what, r_mass)
    assert r_sum <= 1.0, "%s: key_mass sums to 1 outside the summed bounds (x%.3g)" % (what, r_sum)
    assert r_peak <= 1.0, "%s: site_peak exceeds its rounding bound by x%.3g" % (what, r_peak)
    assert bool(in_range.all()), "%s: a site_key outside the drug's stored keys" % what
    assert float(slack.min()) >= 0.0, "%s: a site_key whose reference probability is below the peak by more than the two bounds" % what


def _name(s):
    return "pgca_pairs_ragged_profile %s %s" % (s["c"].name, str(s["dt"]).split(".")[1])


def _with_di(s, di=None):
    return dict(s, di_used=s["di"] if di is None else di)


@pytest.mark.parametrize("name,dt", PARAMS, ids=["%s-%s" % (n, str(d).split(".")[1]) for n, d in PARAMS])
def test_ragged_profiles_against_fp64(name, dt, refs):
    from druglamp_amd import ops
    s = _with_di(_setup(name, dt, True))
    assert s["lam"] <= LAM, "%s: logits beyond the range the bound assumes" % name
    word = ops.guard_flags(DEV)
    word.zero_()
    res = _run(s)
    assert int(word.item()) == 0
    _check(_name(s), s, refs(name, dt), res)
    again = _run(s)
    for what, (flat, _, mask, before), (flat2, _, _, _) in zip(("key_mass", "site_peak", "site_key"), res, again):
        assert torch.equal(_bits(flat)[~mask], before[~mask]), "%s: a store to %s outside the addressed elements" % (name, what)
        assert bool((_bits(flat)[mask] != before[mask]).all()), "%s: an addressed element of %s was not written" % (name, what)
        assert torch.equal(_bits(flat2), _bits(flat)), "%s: two calls differ in %s" % (name, what)
    if name == "a_six_layouts":                                            # the case does show zero fill on every drug
        assert sorted(set(s["ncols"].tolist())) == [65, 504, 508, 512] and s["c"].cols == 520


@pytest.mark.parametrize("d,flag", [(10, "FLAG_PAIR_INDEX"), (6, "FLAG_KEY_TABLE"), (7, "FLAG_KEY_TABLE"), (8, "FLAG_MAP_COLS"),
                                    (9, "FLAG_MAP_COLS")])
def test_each_unfit_pair_is_skipped_alone_under_its_own_flag(d, flag, refs):
    """On the allocation of case (a), told about 10 drugs (_setup's table): pair 4 names drug 10 (out of range: the NaN spare
    entry, inside the allocation), drug 6 (its entry ends one row behind the declared store), drug 7 (4 keys < key_tail_rows),
    drug 8 (the model-layout drug's rows at weight 50: 528 columns > 520) or drug 9 (real rows at weight 2.5).  Only that flag is
    set, the pair's rows of all three outputs stay bitwise NaN, every other pair meets its bounds."""
    from druglamp_amd import _lib, ops
    s0 = _setup("a_six_layouts", BF, True)
    di = s0["di"].clone()
    di[4] = d
    s = _with_di(s0, di)
    word = ops.guard_flags(DEV)
    word.zero_()
    try:
        res = _run(s, di=di, n_kv=10)
        bits = int(word.item())
    finally:
        word.zero_()
    assert bits == getattr(_lib, flag), (d, bits)
    for (flat, view, mask, before), pitch in zip(res, (s["c"].pitch, s["c"].Lq + SITE_PAD, s["c"].Lq + SITE_PAD)):
        lo, hi = G + 4 * pitch, G + 5 * pitch
        assert torch.equal(_bits(flat)[lo:hi], before[lo:hi]), "the skipped pair's row was written"
        assert torch.equal(_bits(flat)[~mask], before[~mask])
    others = torch.tensor([i for i in range(s["n"]) if i != 4], device=DEV)
    _check(_name(s) + " + drug %d" % d, s, refs("a_six_layouts", BF), res, pairs=others)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bfloat16", "float32"])
def test_dense_and_ragged_entry_points_agree_bitwise_on_a_uniform_store(dt):
    """Both entry points launch one kernel that differs only in where a workgroup finds its keys (the tail bias is taken on the
    device for both): `kv` as (3, 72, 256) with key_tail (8, 3.0) for the dense entry point, the same memory as (216, 256) with
    row0 = (0, 72, 144) and weights 3.0 for the ragged one.  88 columns, cols = 92 by request / 88 by default."""
    from druglamp_amd import ops
    g = torch.Generator().manual_seed(72)
    n_q, n_kv, Lq, Lk, t, w = 2, 3, 40, 72, 8, 3.0
    q = (torch.randn(n_q, Lq, E, generator=g) * 0.7).to(DEV, dt)
    kv = torch.cat([torch.randn(n_kv, Lk, E, generator=g) * 0.7, torch.randn(n_kv, Lk, E, generator=g)], dim=2).to(DEV, dt)
    pi = torch.tensor((0, 1, 1, 0, 1), dtype=torch.int32, device=DEV)
    di = torch.tensor((2, 0, 1, 1, 2), dtype=torch.int32, device=DEV)
    dense = ops.pgca_pairs_profile(q, kv, pi, di, scale=E ** -0.5, key_tail=(t, w), cols=92)
    row0 = torch.arange(n_kv, dtype=torch.int64, device=DEV) * Lk
    n_keys = torch.full((n_kv,), Lk, dtype=torch.int32, device=DEV)
    tw = torch.full((n_kv,), w, dtype=torch.float32, device=DEV)
    ragged = ops.pgca_pairs_ragged_profile(q, kv.view(n_kv * Lk, 2 * E), row0, n_keys, tw, pi, di, scale=E ** -0.5, key_tail_rows=t, cols=92)
    torch.cuda.synchronize()
    for a, b, shape, dtype in zip(dense, ragged, ((5, 92), (5, Lq), (5, Lq)), (F32, F32, torch.int32)):
        assert a.shape == b.shape == shape and a.dtype == b.dtype == dtype
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    mass, peak, key = dense
    assert bool((mass[:, 88:] == 0).all()) and float((mass.double().sum(-1) - 1).abs().max()) <= 1e-5
    assert bool((mass[:, 64:72] == mass[:, 72:80]).all()) and bool((mass[:, 64:72] == mass[:, 80:88]).all())    # a tail key's copies
    assert int(key.min()) >= 0 and int(key.max()) < Lk and float(peak.min()) > 0 and float(peak.max()) <= 1
    own = ops.pgca_pairs_profile(q, kv, pi, di, scale=E ** -0.5, key_tail=(t, w))          # cols defaults to the map's own count
    assert own[0].shape == (5, 88) and torch.equal(own[0], mass[:, :88]) and torch.equal(own[1], peak) and torch.equal(own[2], key)


def test_host_tensors_small_outputs_and_a_wrong_table_are_rejected():
    from druglamp_amd import ops
    s = _setup("b_no_tail", BF, True)
    c, k, n = s["c"], s["n_kv"], s["n"]
    q, rows, tab = s["q"], s["rows"], (s["row0"][:k], s["keys"][:k], s["w"][:k])
    kw = dict(scale=s["scale"], key_tail_rows=0, cols=c.cols)

    def outs(mass=(n, c.cols), peak=(n, c.Lq), key=(n, c.Lq), mass_dt=F32, key_dt=torch.int32, dev=DEV):
        return (torch.empty(mass, device=dev, dtype=mass_dt), torch.empty(peak, device=dev), torch.empty(key, device=dev, dtype=key_dt))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_ragged_profile(q.cpu(), rows, *tab, s["pi"], s["di"], **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_ragged_profile(q, rows, tab[0].cpu(), tab[1], tab[2], s["pi"], s["di"], **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_ragged_profile(q, rows, *tab, s["pi"], s["di"], out=outs(dev="cpu"), **kw)
    for bad in (outs(mass=(n, 512)), outs(peak=(n, c.Lq - 1)), outs(key=(n, c.Lq + 8)), outs(mass_dt=BF), outs(key_dt=torch.int64),
                outs()[:2], outs(mass=(n - 1, c.cols))):                        # (key (n, Lq + 8): another pitch than site_peak's)
        with pytest.raises(ValueError, match="out must be"):
            ops.pgca_pairs_ragged_profile(q, rows, *tab, s["pi"], s["di"], out=bad, **kw)
    with pytest.raises(ValueError, match="key table"):                   # row0 must be int64
        ops.pgca_pairs_ragged_profile(q, rows, tab[0].int(), tab[1], tab[2], s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="key table"):                   # n_keys must be int32
        ops.pgca_pairs_ragged_profile(q, rows, tab[0], tab[1].long(), tab[2], s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="key table"):                   # tail_weight must be float32
        ops.pgca_pairs_ragged_profile(q, rows, tab[0], tab[1], tab[2].double(), s["pi"], s["di"], **kw)
    with pytest.raises(ValueError, match="cols"):
        ops.pgca_pairs_ragged_profile(q, rows, *tab, s["pi"], s["di"], scale=s["scale"], key_tail_rows=0, cols=0)
    with pytest.raises(RuntimeError, match="does not fit"):              # the dense column count is checked on the host
        ops.pgca_pairs_profile(q, rows[:80].view(2, 40, 256), s["pi"][:2], s["pi"][:2], scale=s["scale"], cols=39)
    with pytest.raises(RuntimeError, match="Lk 600"):                    # more stored keys than a profile launch serves
        ops.pgca_pairs_profile(q, torch.zeros(1, 600, 256, device=DEV, dtype=BF), s["pi"][:2] * 0, s["pi"][:2] * 0, scale=s["scale"])
