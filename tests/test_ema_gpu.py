"""The weight-EMA kernel (csrc/optim.hip) through druglamp_amd.ops, against tests/ema_ref.py.

  * parity: every element within 2^-22 max(|e|, |p|) of the fp64 recurrence (derived in ema_ref.bound, checked on an fp32
    emulation in tests/test_ema_reference_cpu.py), param never written, at sizes that take every path of the launch shape:
    below one 16-byte chunk, a scalar tail of 1 / 3 elements, exactly one chunk, a ragged last workgroup, several workgroups.
    The grid is one chunk per thread (AdamW's), not capped: there is no second grid pass to cover;
  * the fixed point ema == param, bit for bit, zeros of either sign included;
  * the guard: nothing written on a skipped step, the same bits with a clear flag as without a guard;
  * NaN / +inf / -inf planted first, in the middle and last (in the scalar tail);
  * every rejected argument raises through ops.check and writes nothing."""
import numpy as np
import pytest
import torch

from tests import ema_ref as er

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [1, 3, 4, 5, 1003, 1028, (1 << 20) + 5]
SKIP = (0.0, float("nan"), 1.0, 0.0)
GO = (0.37, 2.5, 0.0, 0.0)


def _pair(n, seed=None):
    e, p = er.pairs(n, seed=n % 97 if seed is None else seed)
    return torch.from_numpy(e).to(DEV), torch.from_numpy(p).to(DEV), e, p


def _guard(values):
    return torch.tensor(values, dtype=torch.float32, device=DEV)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("w", er.WEIGHTS)
@pytest.mark.parametrize("n", SIZES)
def test_update_against_the_fp64_recurrence(n, w):
    from druglamp_amd import ops
    ema, param, e, p = _pair(n)
    ops.ema_update(ema, param, w)
    got = ema.cpu().numpy().astype(np.float64)
    ratio = float((np.abs(got - er.update(e, p, w)) / er.bound(e, p)).max())
    print("n", n, "w", w, "worst error / bound", ratio)
    assert ratio <= 1.0
    assert np.array_equal(param.cpu().numpy().view(np.int32), p.view(np.int32)), "param was written"
    if w == 0.0:
        assert np.array_equal(got, e.astype(np.float64))


@pytest.mark.parametrize("w", er.WEIGHTS)
@pytest.mark.parametrize("n", [5, 1003, (1 << 20) + 5])
def test_equal_operands_are_a_bitwise_fixed_point(n, w):
    from druglamp_amd import ops
    ema, _, _, _ = _pair(n)
    ema[0] = -0.0                                       # (-0, -0): the fma alone would give +0
    ema[n - 1] = -0.0                                   # in the scalar tail
    ema[n // 2] = 0.0
    ema[1] = 1e-42                                      # a subnormal
    param, keep = ema.clone(), ema.clone()
    ops.ema_update(ema, param, w)
    assert torch.equal(_bits(ema), _bits(keep)) and torch.equal(_bits(param), _bits(keep))
    assert int(_bits(ema)[0]) == -2 ** 31 and int(_bits(ema)[n - 1]) == -2 ** 31


@pytest.mark.parametrize("n", SIZES)
def test_a_set_skip_flag_writes_nothing_and_a_clear_one_changes_nothing(n):
    from druglamp_amd import ops
    for w in er.WEIGHTS:
        ema, param, _, _ = _pair(n)
        keep_e, keep_p = ema.clone(), param.clone()
        ops.ema_update(ema, param, w, _guard(SKIP))
        assert torch.equal(_bits(ema), _bits(keep_e)) and torch.equal(_bits(param), _bits(keep_p)), ("skipped step wrote", w)
        plain = keep_e.clone()
        ops.ema_update(plain, param, w)
        ops.ema_update(ema, param, w, _guard(GO))
        assert torch.equal(_bits(ema), _bits(plain)), ("guard with a clear flag differs from no guard", w)
        if w == 1.0:                                    # (a small weight times a small difference may round away at n = 1)
            assert not torch.equal(ema, keep_e), "the update with a clear flag did not run"


@pytest.mark.parametrize("w", er.WEIGHTS)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_parameters_pass_through_as_the_recurrence_says(bad, w):
    from druglamp_amd import ops
    n = 1003                                            # n % 4 == 3: the last element is in the scalar tail
    spots = [0, 501, n - 1]
    ema, param, e, p = _pair(n, seed=5)
    clean = ema.clone()
    ops.ema_update(clean, param, w)
    for s in spots:
        param[s] = bad
        p[s] = bad
    ops.ema_update(ema, param, w)
    want = er.update(e, p, w)
    got = ema.cpu().numpy()
    for s in spots:
        assert not np.isfinite(want[s])
        assert (np.isnan(got[s]) and np.isnan(want[s])) or got[s] == want[s], (s, got[s], want[s])
    if bad != bad or w == 0.0:
        assert all(np.isnan(got[s]) for s in spots)     # a NaN parameter; 0 * inf
    else:
        assert all(got[s] == bad for s in spots)
    others = torch.ones(n, dtype=torch.bool, device=DEV)
    others[spots] = False
    assert torch.equal(_bits(ema)[others], _bits(clean)[others]), "a neighbour of a planted element changed"
    assert bool(torch.isfinite(ema[others]).all())


def test_rejected_arguments_raise_through_check_and_write_nothing():
    from druglamp_amd import _lib, ops
    n = 64
    ema, param, _, _ = _pair(n)
    big_e, big_p = torch.zeros(n + 4, device=DEV), torch.ones(n + 4, device=DEV)
    gbuf = torch.tensor([0.0] + list(GO) + [0.0] * 3, dtype=torch.float32, device=DEV)
    keep = ema.clone()
    L = _lib.lib()
    cases = [
        ("null", lambda: ops.check(L.dl_ema_update(None, param.data_ptr(), n, 0.1, None, None), "dl_ema_update")),
        ("null", lambda: ops.check(L.dl_ema_update(ema.data_ptr(), None, n, 0.1, None, None), "dl_ema_update")),
        ("null|positive", lambda: ops.ema_update(ema[:0], param[:0].clone(), 0.1)),     # (an empty tensor: no data, no elements)
        ("positive", lambda: ops.check(L.dl_ema_update(ema.data_ptr(), param.data_ptr(), 0, 0.1, None, None), "dl_ema_update")),
        ("aligned", lambda: ops.ema_update(big_e[1:1 + n], param, 0.1)),
        ("aligned", lambda: ops.ema_update(ema, big_p[3:3 + n], 0.1)),
        ("aligned", lambda: ops.ema_update(ema, param, 0.1, gbuf[1:5])),
        ("weight", lambda: ops.ema_update(ema, param, -0.001)),
        ("weight", lambda: ops.ema_update(ema, param, 1.001)),
        ("weight", lambda: ops.ema_update(ema, param, float("nan"))),
        ("weight", lambda: ops.ema_update(ema, param, float("inf"))),
        ("same buffer", lambda: ops.ema_update(ema, ema, 0.1)),
    ]
    for word, call in cases:
        with pytest.raises(RuntimeError, match=word):
            call()
    with pytest.raises(TypeError):
        ops.ema_update(ema, param.double(), 0.1)
    with pytest.raises(TypeError):
        ops.ema_update(ema.bfloat16(), param.bfloat16(), 0.1)
    with pytest.raises(ValueError, match="contiguous"):
        ops.ema_update(big_e[::2][:n // 2], param[:n // 2], 0.1)
    with pytest.raises(ValueError, match="elements"):
        ops.ema_update(ema, big_p, 0.1)
    with pytest.raises(ValueError, match="4 floats"):
        ops.ema_update(ema, param, 0.1, gbuf[:2])
    torch.cuda.synchronize()
    assert torch.equal(_bits(ema), _bits(keep)) and float(big_e.abs().max()) == 0.0
    ops.ema_update(ema, param, 0.1, gbuf[4:8])          # (a 16-byte aligned slice is accepted: flag clear, the update runs)
    assert not torch.equal(ema, keep)
