"""dl_pgca_pairs_attr / dl_pgca_pairs_ragged_attr without a device: export, ctypes signature and struct layout, the argument
validation that runs before any launch, the wrappers' and Trainer.hit_attributions' host-side refusals — and the reference the
GPU test goes against (tests/attr_ref.py):
    the closed form equals torch fp64 autograd gradient x value on the leaves q, sites, K, V' (tail keys physically expanded) to
    1e-12 relative, and the identity sum_col key_attr = sum_r sum_c w ds s + sum_r <dO_r, O_r> holds;
    the bound has ROOM: an fp32 emulation of the kernel's arithmetic (s and g in fp32 from the rounded inputs, fp32 sums in
    block order) stays inside it on every case of the GPU test;
    the bound has TEETH: (i) D dropped, (ii) D summed without the multiplicities, (iii) the tail bias left inside the factor s,
    (iv) rows r >= Lq of a partial block entering key_attr — each leaves it."""
import ctypes as C
import functools
import math
import os
import re

import pytest
import torch

from druglamp_amd import _lib
from tests import attr_ref

OK, ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3, -6
DENSE_PTRS = ("Q", "K", "dO", "sites", "d_sites", "key_attr", "site_attr", "q_index", "kv_index", "flags")
RAGGED_PTRS = ("Q", "K", "dO", "sites", "d_sites", "key_attr", "site_attr", "q_index", "kv_index", "kv_row0", "kv_keys",
               "kv_tail_weight", "flags")
OPTIONAL = ("sites", "d_sites", "flags")
BF, F32 = torch.bfloat16, torch.float32
GPU_PARAMS = [("a_six_layouts", BF), ("a_six_layouts", F32), ("b_no_tail", BF), ("b_no_tail", F32), ("c_many_pairs", BF), ("d_two_blocks", BF)]


def _entry(form):
    if form == "dense":
        return "dl_pgca_pairs_attr", _lib.PgcaPairsAttrArgs, DENSE_PTRS
    return "dl_pgca_pairs_ragged_attr", _lib.PgcaPairsRaggedAttrArgs, RAGGED_PTRS


def _args(form, buf, **kw):
    """A valid call description (bf16, 2 proteins x 3 drugs of 40 keys whose last 8 stand for 3 each, 4 pairs, Lq 16, 56 columns;
    key_attr rows of 64, site rows of 24; dO and d_sites the halves of a 256-wide gradient) pointing into `buf`."""
    _, cls, ptrs = _entry(form)
    p16 = (C.addressof(buf) + 15) // 16 * 16
    a = cls()
    for name in ptrs:
        setattr(a, name, p16)
    a.q_es, a.q_rs, a.k_rs, a.mass_ps, a.site_ps = 16 * 128, 128, 256, 64, 24
    a.do_ps, a.do_rs, a.dl_ps, a.dl_rs, a.left_es, a.left_rs = 16 * 256, 256, 16 * 256, 256, 16 * 128, 128
    a.n_pairs, a.n_q, a.n_kv, a.Lq, a.head_dim, a.dtype = 4, 2, 3, 16, 128, _lib.DL_BF16
    a.out_cols, a.left_cols, a.scale, a.key_tail_rows = 56, 128, 128 ** -0.5, 8
    if form == "dense":
        a.k_es, a.Lk, a.key_tail_weight = 40 * 256, 40, 3.0
    else:
        a.kv_total_rows = 120
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _caller(form):
    L = _lib.lib()
    fn = getattr(L, _entry(form)[0])
    buf = (C.c_char * 4096)()
    p16 = (C.addressof(buf) + 15) // 16 * 16
    return (lambda **kw: fn(C.byref(_args(form, buf, **kw)), None)), L.dl_last_error, p16


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_symbols_are_exported_with_their_signatures_and_field_order(form):
    L = _lib.lib()
    name, cls, ptrs = _entry(form)
    res, args = _lib.SIGNATURES[name]
    fn = getattr(L, name)
    assert fn.restype is res and list(fn.argtypes) == list(args) == [C.POINTER(cls), C.c_void_p]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "druglamp_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} %s_args;" % name, hdr).group(1)
    names = [re.findall(r"\w+", piece)[-1] for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    assert names == [f[0] for f in cls._fields_] and names[:len(ptrs)] == list(ptrs)
    # pointers first, then 8-byte strides, then 4-byte fields: dense 10 + 12 + 13, ragged 13 + 12 + 11; the struct ends on its
    # 8-byte alignment
    sizes = [C.sizeof(f[1]) for f in cls._fields_]
    assert sizes == sorted(sizes, reverse=True) and all(f[1] is C.c_void_p for f in cls._fields_[:len(ptrs)])
    assert sum(sizes) == ((10 + 12) * 8 + 13 * 4 if form == "dense" else (13 + 12) * 8 + 11 * 4)
    assert C.sizeof(cls) == (sum(sizes) + 7) // 8 * 8


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_null_argument_block_fails_with_a_message(form):
    L = _lib.lib()
    name = _entry(form)[0]
    assert getattr(L, name)(None, None) == ERR_ARG
    assert name.encode() in L.dl_last_error() and b"null argument block" in L.dl_last_error()


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_every_rejection_returns_its_code_and_names_the_field(form):
    rc, err, p16 = _caller(form)
    for name in _entry(form)[2]:
        if name not in OPTIONAL:
            assert rc(**{name: None}) == ERR_ARG and b"null pointer" in err() and name.encode() in err(), name
    assert rc(sites=None) == ERR_ARG and b"both or neither" in err()
    assert rc(d_sites=None) == ERR_ARG and b"both or neither" in err()
    assert rc(dtype=7) == ERR_ARG and b"dtype" in err()
    assert rc(head_dim=64) == ERR_UNSUPPORTED and b"head_dim" in err()
    assert rc(out_cols=0) == ERR_SHAPE and b"out_cols" in err()
    assert rc(mass_ps=48) == ERR_SHAPE and b"mass_ps" in err() and b"out_cols" in err()
    assert rc(site_ps=15) == ERR_SHAPE and b"site_ps" in err() and b"Lq" in err()
    assert rc(reserved=1) == ERR_ARG and b"reserved" in err()
    assert rc(k_rs=128) == ERR_SHAPE and b"k_rs" in err()                            # a [K | V'] row has 256 columns
    assert rc(left_cols=4) == ERR_SHAPE and b"left_cols" in err()                    # 4 bf16 = 8 bytes
    assert rc(left_cols=0) == ERR_SHAPE and b"left_cols" in err()
    for name in ("key_attr", "site_attr"):
        assert rc(**{name: p16 + 2}) == ERR_ALIGN and b"4-byte" in err() and name.encode() in err(), name
    for name in ("Q", "K", "dO", "sites", "d_sites"):
        assert rc(**{name: p16 + 8}) == ERR_ALIGN and b"16-byte" in err() and name.encode() in err(), name
    assert rc(q_index=p16 + 2) == ERR_ALIGN and b"q_index" in err()
    for name in ("q_es", "q_rs", "k_rs", "do_ps", "do_rs") + (("k_es",) if form == "dense" else ()):
        assert rc(**{name: 260}) == ERR_ALIGN and name.encode() in err(), name       # 260 bf16 = 520 bytes: no multiple of 16
        assert rc(**{name: -256}) == ERR_ALIGN and name.encode() in err(), name
    for name in ("left_es", "left_rs", "dl_ps", "dl_rs"):
        assert rc(**{name: 260}) == ERR_ALIGN and b"sites / d_sites" in err(), name
    assert rc(dtype=_lib.DL_F32, do_rs=130) == ERR_ALIGN and b"do_rs" in err()       # fp32: multiples of 4 elements
    assert rc(key_tail_rows=-1) == ERR_ARG and b"key_tail_rows" in err()
    assert rc(n_pairs=-1) == ERR_SHAPE and b"negative" in err()
    assert rc(Lq=0) == ERR_SHAPE and b"Lq" in err()
    assert rc(scale=0.0) == ERR_ARG and b"scale" in err()
    if form == "ragged":
        assert rc(kv_row0=p16 + 4) == ERR_ALIGN and b"kv_row0" in err()
        assert rc(kv_keys=p16 + 2) == ERR_ALIGN and b"kv_keys" in err()
        assert rc(kv_total_rows=-1) == ERR_SHAPE and b"kv_total_rows" in err()
        assert rc(key_tail_rows=577) == ERR_UNSUPPORTED and b"key_tail_rows" in err()
    else:
        assert rc(out_cols=55) == ERR_SHAPE and b"56 columns" in err() and b"out_cols" in err()
        assert rc(key_tail_weight=2.5) == ERR_ARG and b"whole key_tail_weight" in err()
        assert rc(key_tail_weight=0.5) == ERR_ARG and b"below 1" in err()
        assert rc(key_tail_rows=41) == ERR_ARG and b"key_tail_rows" in err()
        assert rc(Lk=0) == ERR_SHAPE and b"Lk" in err()
        assert rc(Lk=577, out_cols=1024, mass_ps=1024) == ERR_UNSUPPORTED and b"Lk 577" in err()


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_no_pairs_is_ok_without_a_launch(form):
    rc, _, _ = _caller(form)
    assert rc(n_pairs=0) == OK                                                       # (no device here: a launch would have failed)
    assert rc(n_pairs=0, **{name: None for name in _entry(form)[2]}) == OK


# ---- the reference ----------------------------------------------------------------------------------------------------------
def _small(seed, Lq, Lk, t, w, hd=8, left=6):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).double()
    return dict(q=r(Lq, hd), K=r(Lk, hd), V=r(Lk, hd), dO=0.05 * r(Lq, hd), t=t, w=w, scale=0.3, sites=r(Lq, left), dL=0.05 * r(Lq, left))


@pytest.mark.parametrize("Lq,Lk,t,w", [(5, 6, 2, 3.0), (7, 9, 0, 1.0), (4, 8, 8, 5.0), (3, 1, 0, 1.0), (6, 11, 4, 1.0)])
@pytest.mark.parametrize("with_sites", [True, False], ids=["sites", "no_sites"])
def test_closed_form_is_autograd_gradient_times_value_and_the_identity_holds(Lq, Lk, t, w, with_sites):
    x = _small(Lq * 100 + Lk, Lq, Lk, t, w)
    if not with_sites:
        x["sites"] = x["dL"] = None
    r = attr_ref.closed_form(**x)
    key, site, O = attr_ref.autograd_form(**x)
    for got, want in ((r["key"], key), (r["site"], site)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (got, want)
    # the identity: over the expanded columns a tail key counts w times; D[r] = <dO_r, O_r>
    cols = Lk - t + t * int(w) + 3
    full = attr_ref.expand(r["key"], t, w, cols)
    assert bool((full[cols - 3:] == 0).all()) and (t == 0 or w < 2 or torch.equal(full[Lk - t:Lk], full[Lk:Lk + t]))
    d = (x["dO"] * O).sum(-1)
    assert float((r["D"].squeeze(-1) - d).abs().max()) <= 1e-12 * float(d.abs().max())
    lhs, rhs = float(full.sum()), float(r["core"].sum() + d.sum())
    assert abs(lhs - rhs) <= 1e-12 * (float(full.abs().sum()) + float(d.abs().sum()))


# ---- room and teeth of the bound, on the GPU test's cases (built on the CPU) ----------------------------------------------------
LOG2E = 1.4426950408889634


def _emulate(q, K, V, dO, t, w, scale, qb, variant=None, pad=None, sites=None, dL=None):
    """The kernel's arithmetic in fp32 torch: s and g as fp32 products of the inputs as stored, the online quantities of sweep 1
    (maximum and sums with the tail bias), sweep 2 without it, fp32 sums in block order (a wave's 16 * QT rows, a wave's
    running column sum over the blocks, the eight waves in the kernel's fixed order).  variant: one of the wrong kernels of the
    module docstring; pad = (q rows, dO rows) that an unguarded partial block would bring in (variant iv)."""
    f = torch.float32
    Lq, Lk = q.shape[0], K.shape[0]
    qx, dx = q.to(f), dO.to(f)
    if variant == "iv":
        qx, dx = torch.cat([qx, pad[0].to(f)]), torch.cat([dx, pad[1].to(f)])
    sc, c = torch.tensor(scale, dtype=f), torch.tensor(scale * LOG2E, dtype=f)
    s = qx @ K.to(f).t()
    g = dx @ V.to(f).t()
    wk = attr_ref.key_weights(Lk, t, w).to(f)
    bias = torch.log(wk) / sc
    sb = s + bias
    m = sb.max(-1, keepdim=True).values
    e = torch.exp2(sb * c - m * c)
    l = e.sum(-1, keepdim=True)
    if variant == "ii":
        D = (torch.exp2(s * c - m * c) * g).sum(-1, keepdim=True) / l
    else:
        D = (e * g).sum(-1, keepdim=True) / l
    if variant == "i":
        D = torch.zeros_like(D)
    lse2 = (m * sc + torch.log(l)) * torch.tensor(LOG2E, dtype=f)
    p = torch.exp2(s * c - lse2)
    fac = (sb if variant == "iii" else s) * sc
    ds = p * (g - D)
    T = ds * fac
    site = (wk * T).sum(-1)[:Lq]
    if sites is not None:
        site = site + (sites.to(f) * dL.to(f)).sum(-1)
    T = T + p * g
    rows = T.shape[0]
    wr = qb // 8
    waves = [torch.zeros(Lk, dtype=f) for _ in range(8)]
    for b0 in range(0, rows, qb):
        for wv in range(8):
            chunk = T[b0 + wv * wr:min(b0 + (wv + 1) * wr, rows)]
            if chunk.shape[0]:
                waves[wv] = waves[wv] + chunk.sum(0)
    key = ((waves[0] + waves[1]) + (waves[2] + waves[3])) + ((waves[4] + waves[5]) + (waves[6] + waves[7]))
    return key.double(), site.double()


@functools.lru_cache(maxsize=None)
def _case(name, dt):
    import tests.test_pgca_pairs_profile_gpu                                          # registers case (d)
    from tests.test_pgca_pairs_probs_gpu import _setup
    s = _setup(name, dt, True, "cpu")
    g = torch.Generator().manual_seed(4242)
    c = s["c"]
    grad = (0.05 * torch.randn(s["n"], c.Lq, 256, generator=g)).to(dt)
    sites = (0.7 * torch.randn(c.n_q, c.Lq, 128, generator=g)).to(dt)
    return s, dict(d_out=grad[..., 128:], d_sites=grad[..., :128], sites=sites)


def _pairs(s, limit=6):
    """A few pairs of a case that between them name every drug."""
    seen, out = set(), []
    for i, d in enumerate(s["di"].tolist()):
        if d not in seen:
            seen.add(d)
            out.append(i)
    return out[:limit]


def _one(s, x, i, variant=None):
    c = s["c"]
    E = 128
    pi, di = int(s["pi"][i]), int(s["di"][i])
    Lk, w = c.drugs[di]
    r0 = int(s["row0"][di])
    rows = s["rows"][r0:r0 + Lk]
    ops_ = (s["q"][pi], rows[:, :E], rows[:, E:], x["d_out"][i], c.tail_rows, w, s["scale"])
    r = attr_ref.closed_form(*ops_, x["sites"][pi], x["d_sites"][i])
    kb, sb = attr_ref.bounds(r, s["bound"][i, :, :Lk], E)
    qb = 256 if s["dt"] == BF else 128
    pad = None
    if variant == "iv":                         # the rows an unguarded block would fetch: the next protein's, the next pair's
        n_pad = -c.Lq % qb
        reps = (n_pad + c.Lq - 1) // c.Lq
        pad = (s["q"][(pi + 1) % c.n_q].repeat(reps, 1)[:n_pad], x["d_out"][(i + 1) % s["n"]].repeat(reps, 1)[:n_pad])
    key, site = _emulate(*ops_, qb, variant, pad, x["sites"][pi], x["d_sites"][i])
    return float(((key - r["key"]).abs() / kb).max()), float(((site - r["site"]).abs() / sb).max())


@pytest.mark.parametrize("name,dt", GPU_PARAMS, ids=["%s-%s" % (n, str(d).split(".")[1]) for n, d in GPU_PARAMS])
def test_the_bound_has_room_for_fp32_arithmetic(name, dt):
    s, x = _case(name, dt)
    assert s["lam"] < 10.0 and math.isfinite(s["lam"])
    worst = [max(v) for v in zip(*(_one(s, x, i) for i in _pairs(s)))]
    print("%s %s: fp32 emulation, worst |err| / bound: key_attr %.4g, site_attr %.4g" % (name, dt, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


@pytest.mark.parametrize("variant,name", [("i", "a_six_layouts"), ("i", "b_no_tail"), ("ii", "a_six_layouts"), ("ii", "c_many_pairs"),
                                          ("iii", "a_six_layouts"), ("iii", "d_two_blocks"), ("iv", "b_no_tail"), ("iv", "c_many_pairs"),
                                          ("iv", "d_two_blocks")])
def test_the_bound_has_teeth(variant, name):
    """(ii) and (iii) differ from the kernel only on a drug with a tail of weight > 1, (iv) only where Lq is no multiple of the
    block: each is shown on cases that have them, and there on EVERY such pair looked at."""
    s, x = _case(name, BF)
    c = s["c"]
    for i in _pairs(s):
        Lk, w = c.drugs[int(s["di"][i])]
        if variant in ("ii", "iii") and not (c.tail_rows and w > 1):
            continue
        key_r, site_r = _one(s, x, i, variant)
        print("%s variant %s pair %d: |err| / bound: key_attr %.4g, site_attr %.4g" % (name, variant, i, key_r, site_r))
        assert key_r > 1.0, (variant, name, i, key_r)
        # (a drug that is all tail has one bias on every key: sum_c w ds = 0 takes it out of site_attr, not out of key_attr)
        if variant in ("i", "ii") or (variant == "iii" and Lk > c.tail_rows):
            assert site_r > 1.0, (variant, name, i, site_r)


# ---- host-side refusals -------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_host_tensors():
    from druglamp_amd import ops
    q = torch.zeros(2, 16, 128, dtype=BF)
    kv = torch.zeros(3, 40, 256, dtype=BF)
    d_out = torch.zeros(4, 16, 128, dtype=BF)
    pi = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_attr(q, kv, d_out, pi, pi, scale=0.1, key_tail=(8, 3.0))
    row0, n_keys, w = torch.arange(3) * 40, torch.full((3,), 40, dtype=torch.int32), torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_ragged_attr(q, kv.view(120, 256), row0, n_keys, w, d_out, pi, pi, scale=0.1, key_tail_rows=8, cols=64)


class _Lib:
    n, branches = 4, {"v": None, "x": None}

    def full_keys(self, branch):
        return torch.full((4,), 512, dtype=torch.int64)


def test_hit_attributions_refusals_that_fire_before_any_encode():
    from druglamp_amd.trainer import HitAttributions, Trainer
    tr = Trainer.__new__(Trainer)

    class _NoModel:
        def eval(self):
            return self

        def encode_proteins(self, *a):
            raise AssertionError("a refusal must come before any encode")
    tr.model = _NoModel()
    tr.check_device_flags = lambda: None
    idx = torch.tensor([[0, 1], [2, 3], [1, 0]])
    who = "hit_attributions"
    with pytest.raises(ValueError, match="%s: pair_batch must be positive" % who):
        tr.hit_attributions([], _Lib(), idx, pair_batch=0)
    with pytest.raises(ValueError, match=r"%s: indices must be \(P, k\), got \(6,\)" % who):
        tr.hit_attributions([], _Lib(), idx.reshape(-1))
    with pytest.raises(IndexError, match=r"%s: drug index out of range \[0, 4\)" % who):
        tr.hit_attributions([], _Lib(), idx + 2)
    with pytest.raises(ValueError, match="%s: indices has 3 rows, the protein batches yielded 0 proteins" % who):
        tr.hit_attributions([], _Lib(), idx)
    empty = tr.hit_attributions([], _Lib(), torch.zeros((0, 2), dtype=torch.int64))
    assert isinstance(empty, HitAttributions) and empty._fields == ("logit", "key_attr", "site_attr")
    assert empty.logit.shape == (0, 2) and sorted(empty.key_attr) == ["v", "x"] and empty.site_attr["x"].shape == (0, 2, 0)
