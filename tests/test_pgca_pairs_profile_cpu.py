"""dl_pgca_pairs_profile / dl_pgca_pairs_ragged_profile: export, ctypes signature, struct layout and the argument validation that
runs before any launch (status code + dl_last_error() naming the offending field), in the mould of
tests/test_pgca_pairs_probs_cpu.py; the wrappers' and Trainer.hit_profiles' host-side refusals; tests/profile_ref.py against a
direct fp64 softmax; the logit range of the GPU cases' fp64 reference.  None of this needs a device: the library loads without
one."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from druglamp_amd import _lib

OK, ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3, -6
DENSE_PTRS = ("Q", "K", "key_mass", "site_peak", "site_key", "q_index", "kv_index", "flags")
RAGGED_PTRS = ("Q", "K", "key_mass", "site_peak", "site_key", "q_index", "kv_index", "kv_row0", "kv_keys", "kv_tail_weight", "flags")


def _entry(form):
    if form == "dense":
        return "dl_pgca_pairs_profile", _lib.PgcaPairsProfileArgs, DENSE_PTRS
    return "dl_pgca_pairs_ragged_profile", _lib.PgcaPairsRaggedProfileArgs, RAGGED_PTRS


def _args(form, buf, **kw):
    """A valid call description (bf16, 2 proteins x 3 drugs of 40 keys whose last 8 stand for 3 each, 4 pairs, Lq 16, maps of 56
    columns; key_mass rows of 64, site rows of 24) pointing into `buf`."""
    _, cls, ptrs = _entry(form)
    p16 = (C.addressof(buf) + 15) // 16 * 16
    a = cls()
    for name in ptrs:
        setattr(a, name, p16)
    a.q_es, a.q_rs, a.k_rs, a.mass_ps, a.site_ps = 16 * 128, 128, 256, 64, 24
    a.n_pairs, a.n_q, a.n_kv, a.Lq, a.head_dim, a.dtype = 4, 2, 3, 16, 128, _lib.DL_BF16
    a.out_cols, a.scale, a.key_tail_rows = 56, 128 ** -0.5, 8
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
    # pointers first, then 8-byte strides, then 4-byte fields: dense 8 + 6 + 12, ragged 11 + 6 + 10 — no padding inside or behind
    sizes = [C.sizeof(f[1]) for f in cls._fields_]
    assert sizes == sorted(sizes, reverse=True) and all(f[1] is C.c_void_p for f in cls._fields_[:len(ptrs)])
    assert C.sizeof(cls) == sum(sizes) == ((8 + 6) * 8 + 12 * 4 if form == "dense" else (11 + 6) * 8 + 10 * 4)


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_null_argument_block_fails_with_a_message(form):
    L = _lib.lib()
    name = _entry(form)[0]
    assert getattr(L, name)(None, None) == ERR_ARG
    assert name.encode() in L.dl_last_error() and b"null argument block" in L.dl_last_error()


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_every_rejection_returns_its_code_and_names_the_field(form):
    rc, err, p16 = _caller(form)
    for name in _entry(form)[2][:-1]:
        assert rc(**{name: None}) == ERR_ARG and b"null pointer" in err() and name.encode() in err(), name
    assert rc(dtype=7) == ERR_ARG and b"dtype" in err()
    assert rc(head_dim=64) == ERR_UNSUPPORTED and b"head_dim" in err()
    assert rc(out_cols=0) == ERR_SHAPE and b"out_cols" in err()
    assert rc(out_cols=-8) == ERR_SHAPE and b"out_cols" in err()
    assert rc(mass_ps=48) == ERR_SHAPE and b"mass_ps" in err() and b"out_cols" in err()  # rows of 48 cannot take 56 columns
    assert rc(mass_ps=-64) == ERR_SHAPE and b"mass_ps" in err()
    assert rc(site_ps=15) == ERR_SHAPE and b"site_ps" in err() and b"Lq" in err()        # rows of 15 cannot take 16 sites
    assert rc(reserved=1) == ERR_ARG and b"reserved" in err()
    for name in ("key_mass", "site_peak", "site_key"):
        assert rc(**{name: p16 + 2}) == ERR_ALIGN and b"4-byte" in err() and name.encode() in err(), name
    for name in ("Q", "K"):
        assert rc(**{name: p16 + 8}) == ERR_ALIGN and b"16-byte" in err(), name
    assert rc(q_index=p16 + 2) == ERR_ALIGN and b"q_index" in err()
    for name in ("q_es", "q_rs", "k_rs") + (("k_es",) if form == "dense" else ()):
        assert rc(**{name: 260}) == ERR_ALIGN and name.encode() in err(), name       # 260 bf16 = 520 bytes: no multiple of 16
        assert rc(**{name: -256}) == ERR_ALIGN and name.encode() in err(), name
    assert rc(dtype=_lib.DL_F32, q_rs=130) == ERR_ALIGN and b"q_rs" in err()         # fp32: multiples of 4 elements
    assert rc(key_tail_rows=-1) == ERR_ARG and b"key_tail_rows" in err()
    assert rc(n_pairs=-1) == ERR_SHAPE and b"negative" in err()
    assert rc(n_kv=-2) == ERR_SHAPE and b"negative" in err()
    assert rc(Lq=0) == ERR_SHAPE and b"Lq" in err()
    assert rc(scale=0.0) == ERR_ARG and b"scale" in err()
    if form == "ragged":
        assert rc(kv_row0=p16 + 4) == ERR_ALIGN and b"kv_row0" in err()
        assert rc(kv_keys=p16 + 2) == ERR_ALIGN and b"kv_keys" in err()
        assert rc(kv_total_rows=-1) == ERR_SHAPE and b"kv_total_rows" in err()
        assert rc(key_tail_rows=577) == ERR_UNSUPPORTED and b"key_tail_rows" in err()
    else:
        # launch-wide quantities are known on the host: 32 + 8 * 3 = 56 columns; at most 576 stored keys
        assert rc(out_cols=55) == ERR_SHAPE and b"56 columns" in err() and b"out_cols" in err()
        assert rc(key_tail_weight=2.5) == ERR_ARG and b"whole key_tail_weight" in err()
        assert rc(key_tail_weight=2.0 ** 25, out_cols=2 ** 30, mass_ps=2 ** 30) == ERR_ARG and b"whole key_tail_weight" in err()
        assert rc(key_tail_weight=0.5) == ERR_ARG and b"below 1" in err()
        assert rc(key_tail_rows=41) == ERR_ARG and b"key_tail_rows" in err()
        assert rc(Lk=0) == ERR_SHAPE and b"Lk" in err()
        assert rc(Lk=577, out_cols=1024, mass_ps=1024) == ERR_UNSUPPORTED and b"Lk 577" in err()


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_no_pairs_is_ok_without_a_launch(form):
    rc, _, _ = _caller(form)
    assert rc(n_pairs=0) == OK                                                       # (no device here: a launch would have failed)
    assert rc(n_pairs=0, **{name: None for name in _entry(form)[2]}) == OK


def test_profile_ref_against_a_direct_softmax():
    """2 proteins x 5 rows over a drug of 6 keys whose last 2 stand for 3 each (10 columns: lead 4, copies at 4-5, 6-7, 8-9)."""
    from tests.profile_ref import FLOOR, U_F, profile_ref, site_key_slack
    g = torch.Generator().manual_seed(5)
    q, k = torch.randn(2, 5, 8, generator=g).double(), torch.randn(6, 8, generator=g).double()
    full = torch.cat([k[:4], k[4:], k[4:], k[4:]])                                    # the expanded key set, ExpandTailFn's order
    pm = torch.softmax(0.3 * q @ full.t(), -1)
    b = 1e-3 * pm
    km, km_b, peak, peak_b, arg = profile_ref(pm, b)
    assert torch.allclose(km, pm.mean(1), rtol=0, atol=1e-15) and float((km.sum(-1) - 1).abs().max()) <= 1e-14
    assert torch.equal(peak, pm.amax(-1)) and torch.equal(pm.gather(-1, arg.unsqueeze(-1)).squeeze(-1), peak)
    assert torch.allclose(km_b, b.mean(1) + (5 + 8) * U_F * km + FLOOR, rtol=1e-14, atol=0) and torch.equal(peak_b, b.amax(-1))
    assert bool((km[:, 4:6] == km[:, 6:8]).all()) and bool((km[:, 4:6] == km[:, 8:10]).all())
    stored = torch.where(arg >= 4, 4 + (arg - 4) % 2, arg).int()                      # the stored key of the first maximal column
    slack, ok = site_key_slack(pm, b, stored, 6)
    assert bool(ok.all()) and bool((slack >= 0).all())
    worst = pm.argmin(-1)                                                             # the least probable key cannot pass
    slack, _ = site_key_slack(pm, b, torch.where(worst >= 4, 4 + (worst - 4) % 2, worst).int(), 6)
    assert bool((slack < 0).all())
    _, ok = site_key_slack(pm, b, torch.full((2, 5), 6, dtype=torch.int32), 6)
    assert not bool(ok.any())


@pytest.mark.parametrize("name", ["a_six_layouts", "b_no_tail", "c_many_pairs", "d_two_blocks"])
def test_the_fp64_reference_of_the_gpu_cases_has_small_logits(name):
    """The bound's cap is lam <= 96; at input scale 0.7 the fp64 reference alone gives lam < 10 (built on the CPU)."""
    import tests.test_pgca_pairs_profile_gpu                                          # registers case (d)
    from tests.test_pgca_pairs_probs_gpu import _setup
    s = _setup(name, torch.float32, True, "cpu")
    assert s["lam"] < 10.0 and math.isfinite(s["lam"])


def test_wrappers_refuse_host_tensors_and_wrong_table_dtypes():
    from druglamp_amd import ops
    q = torch.zeros(2, 16, 128, dtype=torch.bfloat16)
    kv = torch.zeros(3, 40, 256, dtype=torch.bfloat16)
    pi = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_profile(q, kv, pi, pi, scale=0.1, key_tail=(8, 3.0))
    row0, n_keys, w = torch.arange(3) * 40, torch.full((3,), 40, dtype=torch.int32), torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_ragged_profile(q, kv.view(120, 256), row0, n_keys, w, pi, pi, scale=0.1, key_tail_rows=8, cols=64)
    for bad in ((row0.int(), n_keys, w), (row0, n_keys.long(), w), (row0, n_keys, w.double()), (row0, n_keys[:2], w)):
        with pytest.raises(ValueError, match="pgca_pairs_ragged_profile: the key table"):
            ops._check_key_table("pgca_pairs_ragged_profile", q, *bad)


class _Lib:
    """What Trainer.hit_profiles looks at before it encodes anything."""
    n, branches = 4, {"v": None}

    def full_keys(self, branch):
        return torch.full((4,), 512, dtype=torch.int64)


def test_hit_profiles_refusals_that_fire_before_any_encode():
    """The checks and texts are hit_maps' (one helper): a bad pair_batch, an unknown branch, indices that are not (P, k), a drug
    index out of range, and protein batches that yield fewer proteins than indices has rows (none at all: nothing is encoded)."""
    from druglamp_amd.trainer import HitProfiles, Trainer
    tr = Trainer.__new__(Trainer)                                                     # no model is touched by these paths

    class _NoModel:
        def eval(self):
            return self

        def encode_proteins(self, *a):
            raise AssertionError("a refusal must come before any encode")
    tr.model = _NoModel()
    tr.check_device_flags = lambda: None
    idx = torch.tensor([[0, 1], [2, 3], [1, 0]])
    for fn, who in ((tr.hit_profiles, "hit_profiles"), (tr.hit_maps, "hit_maps")):
        with pytest.raises(ValueError, match="%s: pair_batch must be positive" % who):
            fn([], _Lib(), idx, pair_batch=0)
        with pytest.raises(ValueError, match=r"%s: unknown branch 'x' \(the library has \['v'\]\)" % who):
            fn([], _Lib(), idx, branch="x")
        with pytest.raises(ValueError, match=r"%s: indices must be \(P, k\), got \(6,\)" % who):
            fn([], _Lib(), idx.reshape(-1))
        with pytest.raises(IndexError, match=r"%s: drug index out of range \[0, 4\)" % who):
            fn([], _Lib(), idx + 2)
        with pytest.raises(IndexError, match="%s: drug index out of range" % who):
            fn([], _Lib(), idx - 1)
        with pytest.raises(ValueError, match="%s: indices has 3 rows, the protein batches yielded 0 proteins" % who):
            fn([], _Lib(), idx)
    empty = tr.hit_profiles([], _Lib(), torch.zeros((0, 2), dtype=torch.int64))
    assert isinstance(empty, HitProfiles) and empty._fields == ("key_mass", "site_peak", "site_key")
    assert empty.key_mass.shape == (0, 2, 0) and empty.site_key.dtype == torch.int32
