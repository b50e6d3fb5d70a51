"""dl_pgca_pairs_attr / dl_pgca_pairs_ragged_attr (csrc/pgca_pairs_attr.hip) through ops.pgca_pairs_attr and
ops.pgca_pairs_ragged_attr, element-wise against the fp64 closed form of tests/attr_ref.py (bounds derived there from the map's
element bound and fp32 dot / sum bounds: no new tolerance; tests/test_pgca_pairs_attr_cpu.py shows the closed form to be autograd's
gradient x value and the bound to have room and teeth).  The inputs are the expanded cases of tests/test_pgca_pairs_probs_gpu._setup
(imported, never modified) with case (d) of the profile test:
    a  six ragged layouts, Lq 256 (one query block in bf16, two in fp32), cols 520        bf16, fp32
    b  no tail: 1, 40 and 512 keys, Lq 40 (a partial block), cols 513 at an odd pitch     bf16, fp32
    c  300 pairs over two drugs: many workgroups resident                                 bf16
    d  Lq 300: two blocks of which the second is partial                                  bf16
d_out is 0.05 * randn from a fixed generator, the right half of a (n, Lq, 256) NaN-guarded buffer whose left half is d_sites;
one parametrisation runs without sites / d_sites (the left half then stays NaN: it must not be read).  Every case asserts
lam <= 96, prints its worst |err| / bound before asserting it and runs twice; the two runs must agree bitwise.  The outputs sit
in NaN buffers with guard bands and pitches above their widths: every addressed element — the zero fill of key_attr included,
exactly +0.0 — must be overwritten, everything else must stay bitwise unchanged."""
import functools

import pytest
import torch

from tests import attr_ref
from tests.test_pgca_pairs_probs_gpu import BF, DEV, F32, LAM, E, G, _bits, _nan_view, _setup
from tests.test_pgca_pairs_profile_gpu import SITE_PAD, _nan_rows          # (importing it registers case (d))

pytestmark = pytest.mark.gpu
PARAMS = [("a_six_layouts", BF, True), ("a_six_layouts", F32, True), ("b_no_tail", BF, True), ("b_no_tail", F32, True),
          ("c_many_pairs", BF, True), ("d_two_blocks", BF, True), ("a_six_layouts", BF, False)]
IDS = ["%s-%s-%s" % (n, str(d).split(".")[1], "sites" if w else "no_sites") for n, d, w in PARAMS]


@functools.lru_cache(maxsize=None)
def _extra(name, dt):
    """The gradients and the left half of a case: computed once, never modified."""
    s = _setup(name, dt, True)
    c = s["c"]
    g = torch.Generator().manual_seed(4242)
    grad = _nan_view(s["n"], c.Lq, 2 * E, dt, 0.05 * torch.randn(s["n"], c.Lq, 2 * E, generator=g), DEV)
    only_right = _nan_view(s["n"], c.Lq, 2 * E, dt, torch.full((s["n"], c.Lq, 2 * E), float("nan")), DEV)
    only_right[..., E:] = grad[..., E:]
    sites = _nan_view(c.n_q, c.Lq, E, dt, 0.7 * torch.randn(c.n_q, c.Lq, E, generator=g), DEV)
    return dict(d_out=grad[..., E:], d_sites=grad[..., :E], sites=sites, d_out_alone=only_right[..., E:])


@functools.lru_cache(maxsize=None)
def _ref(name, dt, with_sites):
    return attr_ref.case_reference(_setup(name, dt, True), _extra(name, dt), with_sites)


def _run(s, x, with_sites, di=None, n_kv=None):
    """One call on fresh NaN outputs: [(flat, view, mask, bits before)] for key_attr and site_attr."""
    from druglamp_amd import ops
    c = s["c"]
    n_kv = s["n_kv"] if n_kv is None else n_kv
    bufs = [_nan_rows(s["n"], c.cols, c.pitch), _nan_rows(s["n"], c.Lq, c.Lq + SITE_PAD)]
    before = [_bits(b[0]) for b in bufs]
    out = (bufs[0][1], bufs[1][1])
    kw = dict(sites=x["sites"], d_sites=x["d_sites"]) if with_sites else {}
    got = ops.pgca_pairs_ragged_attr(s["q"], s["rows"], s["row0"][:n_kv], s["keys"][:n_kv], s["w"][:n_kv],
                                     x["d_out"] if with_sites else x["d_out_alone"], s["pi"], s["di"] if di is None else di,
                                     scale=s["scale"], key_tail_rows=c.tail_rows, cols=c.cols, out=out, **kw)
    assert all(g is o for g, o in zip(got, out))
    torch.cuda.synchronize()
    return [(b[0], o, b[2], bf) for b, o, bf in zip(bufs, out, before)]


def _check(what, s, ref, res, pairs=None):
    """Worst |err| / bound of the two outputs over `pairs` (all), printed before they are asserted."""
    idx = torch.arange(s["n"], device=DEV) if pairs is None else pairs
    key, site = (r[1][idx] for r in res)
    assert torch.isfinite(key).all() and torch.isfinite(site).all(), "%s: addressed elements left unwritten or non-finite" % what
    fill = torch.arange(key.shape[-1], device=DEV).view(1, -1) >= s["ncols"][idx].view(-1, 1)
    assert bool((_bits(key.contiguous())[fill] == 0).all()), "%s: a zero-fill column of key_attr is not +0.0" % what
    r_key = float(((key.double() - ref["key"][idx]).abs() / ref["key_b"][idx])[~fill].max())
    r_site = float(((site.double() - ref["site"][idx]).abs() / ref["site_b"][idx]).max())
    print("%s: worst |err| / bound: key_attr %.4g, site_attr %.4g" % (what, r_key, r_site))
    assert r_key <= 1.0, "%s: key_attr exceeds its rounding bound by x%.3g" % (what, r_key)
    assert r_site <= 1.0, "%s: site_attr exceeds its rounding bound by x%.3g" % (what, r_site)


def _name(s, with_sites):
    return "pgca_pairs_ragged_attr %s %s%s" % (s["c"].name, str(s["dt"]).split(".")[1], "" if with_sites else " (no sites)")


@pytest.mark.parametrize("name,dt,with_sites", PARAMS, ids=IDS)
def test_ragged_attributions_against_fp64(name, dt, with_sites):
    from druglamp_amd import ops
    s, x = _setup(name, dt, True), _extra(name, dt)
    assert s["lam"] <= LAM, "%s: logits beyond the range the bound assumes" % name
    word = ops.guard_flags(DEV)
    word.zero_()
    res = _run(s, x, with_sites)
    assert int(word.item()) == 0
    _check(_name(s, with_sites), s, _ref(name, dt, with_sites), res)
    again = _run(s, x, with_sites)
    for what, (flat, _, mask, before), (flat2, _, _, _) in zip(("key_attr", "site_attr"), res, again):
        assert torch.equal(_bits(flat)[~mask], before[~mask]), "%s: a store to %s outside the addressed elements" % (name, what)
        assert bool((_bits(flat)[mask] != before[mask]).all()), "%s: an addressed element of %s was not written" % (name, what)
        assert torch.equal(_bits(flat2), _bits(flat)), "%s: two calls differ in %s" % (name, what)


@pytest.mark.parametrize("name,dt", [("a_six_layouts", BF), ("a_six_layouts", F32), ("d_two_blocks", BF)],
                         ids=["a-bfloat16", "a-float32", "d-bfloat16"])
def test_the_identity_against_the_forward_kernels_own_output(name, dt):
    """sum_col key_attr = sum_r site_attr (without the left half) + sum_r <dO_r, O_r>, O from ops.pgca_pairs_ragged (no bias),
    within the summed bounds of the two outputs; in bf16 plus the rounding of O: 2^-9 sum_r sum_i |dO_ri O_ri|."""
    from druglamp_amd import ops
    s, x = _setup(name, dt, True), _extra(name, dt)
    c, ref = s["c"], _ref(name, dt, False)
    k = s["n_kv"]
    key, site = (r[1] for r in _run(s, x, False))
    O = ops.pgca_pairs_ragged(s["q"], s["rows"], s["row0"][:k], s["keys"][:k], s["w"][:k], s["pi"], s["di"], scale=s["scale"],
                              key_tail_rows=c.tail_rows)
    torch.cuda.synchronize()
    prod = x["d_out_alone"].double() * O.double()
    lhs = key.double().sum(-1)
    rhs = site.double().sum(-1) + prod.sum((-1, -2))
    lim = ref["key_b"].sum(-1) + ref["site_b"].sum(-1) + (2.0 ** -9 * prod.abs().sum((-1, -2)) if dt == BF else 0.0)
    ratio = float(((lhs - rhs).abs() / lim).max())
    print("%s %s: identity, worst |lhs - rhs| / limit = %.4g" % (name, dt, ratio))
    assert ratio <= 1.0
    # and the reference's own two sides, for the record of what the kernel is compared with
    assert float(((ref["key"].sum(-1) - ref["core_sum"] - ref["d_sum"]).abs() / lim).max()) <= 1e-6


@pytest.mark.parametrize("d,flag", [(10, "FLAG_PAIR_INDEX"), (6, "FLAG_KEY_TABLE"), (7, "FLAG_KEY_TABLE"), (8, "FLAG_MAP_COLS"),
                                    (9, "FLAG_MAP_COLS")])
def test_each_unfit_pair_is_skipped_alone_under_its_own_flag(d, flag):
    """On the allocation of case (a), told about 10 drugs (_setup's table), pair 4 names an unfit drug (the profile test's five):
    only that flag is set, the pair's rows of both outputs stay bitwise NaN, every other pair meets its bounds."""
    from druglamp_amd import _lib, ops
    s, x = _setup("a_six_layouts", BF, True), _extra("a_six_layouts", BF)
    di = s["di"].clone()
    di[4] = d
    word = ops.guard_flags(DEV)
    word.zero_()
    try:
        res = _run(s, x, True, di=di, n_kv=10)
        bits = int(word.item())
    finally:
        word.zero_()
    assert bits == getattr(_lib, flag), (d, bits)
    for (flat, view, mask, before), pitch in zip(res, (s["c"].pitch, s["c"].Lq + SITE_PAD)):
        lo, hi = G + 4 * pitch, G + 5 * pitch
        assert torch.equal(_bits(flat)[lo:hi], before[lo:hi]), "the skipped pair's row was written"
        assert torch.equal(_bits(flat)[~mask], before[~mask])
    others = torch.tensor([i for i in range(s["n"]) if i != 4], device=DEV)
    _check(_name(s, True) + " + drug %d" % d, s, _ref("a_six_layouts", BF, True), res, pairs=others)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bfloat16", "float32"])
def test_dense_and_ragged_entry_points_agree_bitwise_on_a_uniform_store(dt):
    """`kv` as (3, 72, 256) with key_tail (8, 3.0) for the dense entry point, the same memory as (216, 256) with row0 = (0, 72,
    144) and weights 3.0 for the ragged one; 88 columns, cols = 92 by request / 88 by default."""
    from druglamp_amd import ops
    g = torch.Generator().manual_seed(72)
    n_q, n_kv, Lq, Lk, t, w = 2, 3, 40, 72, 8, 3.0
    q = (torch.randn(n_q, Lq, E, generator=g) * 0.7).to(DEV, dt)
    kv = torch.cat([torch.randn(n_kv, Lk, E, generator=g) * 0.7, torch.randn(n_kv, Lk, E, generator=g)], dim=2).to(DEV, dt)
    grad = (0.05 * torch.randn(5, Lq, 2 * E, generator=g)).to(DEV, dt)
    sites = (torch.randn(n_q, Lq, E, generator=g) * 0.7).to(DEV, dt)
    pi = torch.tensor((0, 1, 1, 0, 1), dtype=torch.int32, device=DEV)
    di = torch.tensor((2, 0, 1, 1, 2), dtype=torch.int32, device=DEV)
    kw = dict(scale=E ** -0.5, sites=sites, d_sites=grad[..., :E])
    dense = ops.pgca_pairs_attr(q, kv, grad[..., E:], pi, di, key_tail=(t, w), cols=92, **kw)
    row0 = torch.arange(n_kv, dtype=torch.int64, device=DEV) * Lk
    n_keys = torch.full((n_kv,), Lk, dtype=torch.int32, device=DEV)
    tw = torch.full((n_kv,), w, dtype=torch.float32, device=DEV)
    ragged = ops.pgca_pairs_ragged_attr(q, kv.view(n_kv * Lk, 2 * E), row0, n_keys, tw, grad[..., E:], pi, di, key_tail_rows=t, cols=92, **kw)
    torch.cuda.synchronize()
    for a, b, shape in zip(dense, ragged, ((5, 92), (5, Lq))):
        assert a.shape == b.shape == shape and a.dtype == b.dtype == F32
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    key, site = dense
    assert bool((_bits(key[:, 88:].contiguous()) == 0).all()) and float(key[:, :88].abs().max()) > 0 and bool(torch.isfinite(site).all())
    assert bool((key[:, 64:72] == key[:, 72:80]).all()) and bool((key[:, 64:72] == key[:, 80:88]).all())    # a tail key's copies
    own = ops.pgca_pairs_attr(q, kv, grad[..., E:], pi, di, key_tail=(t, w), **kw)     # cols defaults to the drug's own count
    assert own[0].shape == (5, 88) and torch.equal(own[0], key[:, :88]) and torch.equal(own[1], site)


def test_wrong_arguments_are_rejected():
    from druglamp_amd import ops
    s, x = _setup("b_no_tail", BF, True), _extra("b_no_tail", BF)
    c, k, n = s["c"], s["n_kv"], s["n"]
    q, rows, tab = s["q"], s["rows"], (s["row0"][:k], s["keys"][:k], s["w"][:k])
    kw = dict(scale=s["scale"], key_tail_rows=0, cols=c.cols)
    call = lambda d_out=x["d_out"], **extra: ops.pgca_pairs_ragged_attr(q, rows, *tab, d_out, s["pi"], s["di"], **dict(kw, **extra))
    with pytest.raises(ValueError, match="d_out is"):                    # d_out comes in the dtype of q
        call(x["d_out"].float())
    with pytest.raises(ValueError, match="d_out must be"):
        call(x["d_out"][:, :-1])
    with pytest.raises(ValueError, match="both or neither"):
        call(sites=x["sites"])
    with pytest.raises(ValueError, match="both or neither"):
        call(d_sites=x["d_sites"])
    with pytest.raises(ValueError, match="d_sites must be"):
        call(sites=x["sites"], d_sites=x["d_sites"][:-1])
    with pytest.raises(ValueError, match="cols"):
        call(cols=0)
    for bad in ((torch.empty(n, 512, device=DEV), torch.empty(n, c.Lq, device=DEV)), (torch.empty(n, c.cols, device=DEV), torch.empty(n, c.Lq - 1, device=DEV)),
                (torch.empty(n, c.cols, device=DEV, dtype=BF), torch.empty(n, c.Lq, device=DEV)), (torch.empty(n, c.cols, device=DEV),),
                (torch.empty(n - 1, c.cols, device=DEV), torch.empty(n, c.Lq, device=DEV))):
        with pytest.raises(ValueError, match="out must be"):
            call(out=bad)
    with pytest.raises(RuntimeError, match="does not fit"):              # the dense column count is checked on the host: cols too small
        ops.pgca_pairs_attr(q, rows[:80].view(2, 40, 256), x["d_out"][:2], s["pi"][:2], s["pi"][:2], scale=s["scale"], cols=39)
    with pytest.raises(RuntimeError, match="Lk 600"):
        ops.pgca_pairs_attr(q, torch.zeros(1, 600, 256, device=DEV, dtype=BF), x["d_out"][:2], s["pi"][:2] * 0, s["pi"][:2] * 0, scale=s["scale"])
