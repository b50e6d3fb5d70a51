"""ops.latent_topk (dl_latent_topk, csrc/latent_topk.hip) against the fp64 reference of tests/latent_topk_ref.py.

Shapes: P in {1, 17, 65} (one row, a partial 16-row wave tile, more than one 64-row workgroup tile), D in {64, 65, 1000, 4099}
(one full 64-row library tile, one row more, a ragged tail, more than one slab under the host's own slab choice),
M in {1, 8, 100, min(D, 1024)}, both dtypes, and slab= values that force 16, 8 and 4 slabs at D = 1000.

Tolerance, derived: the operands are unit-norm rows, so sum |a_i b_i| <= 1 (Cauchy-Schwarz); bf16 products are exact in fp32, and
each of the 256 fp32 accumulation steps adds at most 2^-24 of a partial sum that is bounded by 1 in magnitude: the accumulated
error is at most 256 * 2^-24 = 1.53e-5.  tol = 2e-5, for both dtypes (the fp32 path is an exact-product fma chain)."""
import functools

import numpy as np
import pytest
import torch

from tests import latent_topk_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 2e-5
DTYPES = [torch.float32, torch.bfloat16]
PS, DS = (1, 17, 65), (64, 65, 1000, 4099)


def _ms(D):
    return sorted({m for m in (1, 8, 100, min(D, 1024)) if m <= D})


@functools.lru_cache(maxsize=None)
def _unit(dtype, D):
    """(q (65, 256), lib (D, 256)) on the device and their fp64 score matrix: computed once, shared, never written."""
    q, lib = R.unit_rows(65, 11, dtype), R.unit_rows(D, 12 + D, dtype)
    return q.to(DEV), lib.to(DEV), R.sims64(q, lib)


def _topk(q, lib, M, slab=None):
    from druglamp_amd import ops
    v, i = ops.latent_topk(q, lib, M, slab=slab)
    assert v.shape == i.shape == (q.shape[0], M) and v.dtype == torch.float32 and i.dtype == torch.int64 and v.is_cuda and i.is_cuda
    return v.cpu().numpy(), i.cpu().numpy()


def _check_rows(v, i, s64, what):
    """The per-row checks of a result (v, i) (P, M) against the fp64 scores s64 (P, D)."""
    P, D = s64.shape
    M = v.shape[1]
    assert i.min() >= 0 and i.max() < D, what
    srt = np.sort(i, axis=1)
    assert (np.diff(srt, axis=1) > 0).all(), "%s: an index twice in a row" % what
    at = np.take_along_axis(s64, i, axis=1)
    err = float(np.abs(v - at).max())
    assert err <= TOL, "%s: max |value - fp64 score of its index| = %.3g > %.3g" % (what, err, TOL)
    dv = np.diff(v.astype(np.float64), axis=1)
    assert (dv <= 0).all(), "%s: values increase somewhere" % what
    assert ((dv != 0) | (np.diff(i, axis=1) > 0)).all(), "%s: equal neighbours out of index order" % what
    if M < D:
        rest = s64.copy()
        np.put_along_axis(rest, i, -np.inf, axis=1)
        over = float((rest.max(axis=1) - v.min(axis=1)).max())
        assert over <= TOL, "%s: a left-out drug beats the weakest kept one by %.3g > %.3g" % (what, over, TOL)
    return err


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_top_m_against_fp64(dtype, D):
    q, lib, s64 = _unit(dtype, D)
    worst = 0.0
    for P in PS:
        for M in _ms(D):
            v, i = _topk(q[:P].contiguous(), lib, M)
            worst = max(worst, _check_rows(v, i, s64[:P], "P %d D %d M %d %s" % (P, D, M, dtype)))
    print("%s D %d: max |value - fp64| = %.3g (tolerance %.3g)" % (dtype, D, worst, TOL))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_forced_slabs_against_fp64_and_equal_to_each_other(dtype):
    q, lib, s64 = _unit(dtype, 1000)
    for M in (8, 100, 1000):
        base = _topk(q, lib, M)
        for slab in (64, 128, 320):                       # 16, 8 and 4 slabs: the merge kernel joins their lists
            v, i = _topk(q, lib, M, slab=slab)
            _check_rows(v, i, s64, "slab %d M %d %s" % (slab, M, dtype))
            assert np.array_equal(v.view(np.int32), base[0].view(np.int32)) and np.array_equal(i, base[1]), (slab, M)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_exact_scores_and_ties_equal_the_reference(dtype):
    """Small-integer operands: every dot product is exact in fp32, so values AND indices must be the reference's.  The second
    library has 37 distinct rows among 1000: about 27 exact ties per value, at and above every cut."""
    q = R.int_rows(17, 5, dtype)
    for lib, name in ((R.int_rows(1000, 6, dtype), "distinct rows"), (R.int_rows(1000, 7, dtype, distinct=37), "repeated rows")):
        s64 = R.sims64(q, lib)
        assert np.abs(s64).max() <= 1024 and (s64 == np.round(s64)).all()
        if name == "repeated rows":
            assert len(np.unique(s64[0])) <= 37
        qd, ld = q.to(DEV), lib.to(DEV)
        for M in (1, 8, 100, 1000):
            want_v, want_i = R.topm(s64, M)
            for slab in (None, 64, 320):
                v, i = _topk(qd, ld, M, slab=slab)
                assert np.array_equal(i, want_i), "%s M %d slab %s: indices differ from the reference" % (name, M, slab)
                assert np.array_equal(v.astype(np.float64), want_v), "%s M %d slab %s: values differ" % (name, M, slab)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_a_nan_library_row_is_first_in_every_row(dtype):
    q, lib = R.int_rows(17, 5, dtype), R.int_rows(1000, 6, dtype)
    lib[333, 100] = float("nan")
    s64 = R.sims64(q, lib)
    assert np.isnan(s64[:, 333]).all() and np.isnan(s64).sum() == 17
    for M, slab in ((1, None), (8, 64), (100, None), (100, 320), (1000, 128)):
        want_v, want_i = R.topm(s64, M)
        v, i = _topk(q.to(DEV), lib.to(DEV), M, slab=slab)
        assert (i[:, 0] == 333).all() and np.isnan(v[:, 0]).all(), (M, slab)
        assert np.array_equal(i, want_i) and np.array_equal(v[:, 1:].astype(np.float64), want_v[:, 1:]), (M, slab)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_repeatable_and_independent_of_the_tile_position(dtype):
    q, lib, _ = _unit(dtype, 1000)
    a, b = _topk(q, lib, 100), _topk(q, lib, 100)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
    # row p of the 65-row launch against that query alone: lane 0 of wave 0 of a workgroup of its own computes the same bits
    for p in (0, 15, 16, 33, 63, 64):
        v1, i1 = _topk(q[p:p + 1].contiguous(), lib, 100)
        assert np.array_equal(v1[0].view(np.int32), a[0][p].view(np.int32)) and np.array_equal(i1[0], a[1][p]), p
    # ... and the same pair scored in another library position and tile column: drug 700 moved to the front
    perm = torch.cat([torch.tensor([700]), torch.arange(700), torch.arange(701, 1000)]).to(DEV)
    v2, i2 = _topk(q, lib[perm].contiguous(), 1000)
    full_v, full_i = _topk(q, lib, 1000)
    at = lambda v, i, d: v[i == d].view(np.int32)                 # noqa: E731  (each drug is in every row's full list once)
    assert np.array_equal(at(v2, i2, 0), at(full_v, full_i, 700))


def test_bad_arguments_raise_value_error():
    from druglamp_amd import ops
    q, lib, _ = _unit(torch.float32, 64)
    for kw in (dict(M=0), dict(M=65), dict(M=8, slab=100), dict(M=8, slab=0)):
        with pytest.raises(ValueError):
            ops.latent_topk(q, lib, **kw)
    with pytest.raises(ValueError):
        ops.latent_topk(q, lib.bfloat16(), 8)
    with pytest.raises(ValueError):
        ops.latent_topk(q[:, :128], lib[:, :128], 8)
    with pytest.raises(ValueError):
        ops.latent_topk(q[:0], lib, 8)
    big = torch.zeros(1100, 256, device=DEV)
    with pytest.raises(ValueError):
        ops.latent_topk(q, big, 1025)


def test_launches_only_on_the_current_stream():
    """The stream contract, by the procedure of tests/test_stream_contract_gpu.py: the call is made on a side stream that is
    held back, behind copies that only then put the real inputs in place of a decoy; both launches (slabs and merge) must wait."""
    from druglamp_amd import ops
    from tests.test_stream_contract_gpu import _equal, run_procedure

    def make(g):
        unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 256, generator=g), dim=1).to(DEV)     # noqa: E731
        return {"q": unit(65), "lib": unit(1000)}
    seen = set()
    ref, got, d = run_procedure(make, lambda t: ops.latent_topk(t["q"], t["lib"], 100, slab=128), record=seen)
    assert "dl_latent_topk" in seen
    assert _equal(ref, got), "outputs differ when the call runs on a side stream held back by %.1f ms: a launch went elsewhere" % d
