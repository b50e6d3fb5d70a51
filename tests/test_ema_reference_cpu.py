"""The weight EMA without a GPU: the fp64 recurrence of tests/ema_ref.py pinned against torch.optim.swa_utils.AveragedModel,
the warmup schedule, the GPU tests' element-wise bound checked on an fp32 emulation of the kernel's arithmetic, and the host
logic of the entry point and of the Trainer's arguments (validation happens before any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ema_ref as er


def test_recurrence_equals_torch_averaged_model_over_five_updates():
    """AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d)) after one seeding update_parameters is the shadow cloned at
    construction; every later update is lerp(ema, param, 1 - d).  d = 0.875: 1 - d is exact in fp32, so the weight the C ABI
    would receive is torch's."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    d = 0.875
    torch.manual_seed(3)
    m = torch.nn.Linear(7, 5).double()
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(d))
    avg.update_parameters(m)                                    # the seeding update: a copy
    e0 = [p.detach().clone() for p in m.parameters()]
    snaps = []
    g = torch.Generator().manual_seed(4)
    for _ in range(5):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.1)
        avg.update_parameters(m)
        snaps.append([p.detach().clone() for p in m.parameters()])
    worst = 0.0
    for k, got in enumerate(avg.module.parameters()):
        want = er.run(e0[k], [s[k] for s in snaps], d)
        assert not np.array_equal(want, e0[k].numpy())
        worst = max(worst, float(np.abs(got.detach().numpy() - want).max()))
    print("recurrence against AveragedModel: max |difference|", worst)
    assert worst <= 1e-15


def test_warmup_schedule():
    assert er.weight(0.999, 0, warmup=True) == er.f32(1.0 - 0.1) and abs((1.0 - er.weight(0.999, 0, warmup=True)) - 0.1) < 1e-7
    assert er.weight(0.999, 0) == er.weight(0.999, 10 ** 6) == er.f32(1.0 - 0.999)
    # (1 + t) / (10 + t) >= d  <=>  t >= (10 d - 1) / (1 - d): 890 for d = 0.99 (891 / 900 = 0.99), 8990 for d = 0.999
    for d, cross in ((0.99, 890), (0.999, 8990), (0.5, 8)):
        before, at = er.weight(d, cross - 1, warmup=True), er.weight(d, cross, warmup=True)
        assert before == er.f32(1.0 - cross / (9.0 + cross)) and before > er.f32(1.0 - d), (d, cross)
        assert at == er.weight(d, cross + 1000, warmup=True) == er.f32(1.0 - d), (d, cross)
    ws = [er.weight(0.99, t, warmup=True) for t in range(900)]
    assert all(a >= b for a, b in zip(ws, ws[1:]))              # the weight only falls towards 1 - decay
    from druglamp_amd.trainer import WeightEMA

    class Flat:
        arena = torch.zeros(4)
    for warm in (False, True):
        ema = WeightEMA(Flat(), 0.99, warmup=warm)
        assert ema.updates == 0 and ema.shadow.data_ptr() != Flat.arena.data_ptr()
        assert [er.f32(ema.weight(t)) for t in (0, 5, 889, 890, 5000)] == [er.weight(0.99, t, warm) for t in (0, 5, 889, 890, 5000)]


@pytest.mark.parametrize("w", er.WEIGHTS)
def test_fp32_arithmetic_stays_within_the_gpu_tests_bound(w):
    e, p = er.pairs(1 << 20, seed=11)
    want = er.update(e, p, w)
    lim = er.bound(e, p)
    assert float(np.abs(e).min()) >= 0.99e-3 and float(np.abs(e).max()) <= 10.0 and float(np.abs(p.astype(np.float64) - e).min()) > 0
    for fma in (True, False):
        got = er.kernel_f32(e, p, w, fma=fma).astype(np.float64)
        ratio = float((np.abs(got - want) / lim).max())
        print("w", w, "fma" if fma else "mul+add", "worst error / bound", ratio)
        assert ratio <= 1.0
    same = er.kernel_f32(e, e, w)
    assert np.array_equal(same.view(np.int32), e.view(np.int32))          # the fixed point
    z = np.array([-0.0, 0.0], dtype=np.float32)
    assert np.array_equal(er.kernel_f32(z, z, w).view(np.int32), z.view(np.int32))


def test_reference_passes_nonfinite_values_through():
    e = np.array([1.0, 2.0, -3.0, float("inf")], dtype=np.float32)
    p = np.array([float("nan"), float("inf"), float("-inf"), float("inf")], dtype=np.float32)
    r = er.update(e, p, 0.1)
    assert np.isnan(r[0]) and r[1] == np.inf and r[2] == -np.inf and np.isnan(r[3])
    r0 = er.update(e, p, 0.0)
    assert np.isnan(r0).all()                                    # 0 * inf
    k = er.kernel_f32(e, p, 0.1)
    assert np.isnan(k[0]) and k[1] == np.inf and k[2] == -np.inf and np.isnan(k[3])


def test_entry_point_validates_its_arguments_before_any_launch():
    from druglamp_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    a = (C.addressof(buf) + 15) // 16 * 16
    b, g = a + 1024, a + 2048
    cases = [
        ("null", lambda: L.dl_ema_update(None, b, 16, 0.1, None, None)),
        ("null", lambda: L.dl_ema_update(a, None, 16, 0.1, None, None)),
        ("positive", lambda: L.dl_ema_update(a, b, 0, 0.1, None, None)),
        ("positive", lambda: L.dl_ema_update(a, b, -4, 0.1, None, None)),
        ("aligned", lambda: L.dl_ema_update(a + 4, b, 16, 0.1, None, None)),
        ("aligned", lambda: L.dl_ema_update(a, b + 8, 16, 0.1, None, None)),
        ("aligned", lambda: L.dl_ema_update(a, b, 16, 0.1, g + 4, None)),
        ("weight", lambda: L.dl_ema_update(a, b, 16, -1e-6, None, None)),
        ("weight", lambda: L.dl_ema_update(a, b, 16, 1.0 + 1e-6, None, None)),
        ("weight", lambda: L.dl_ema_update(a, b, 16, float("nan"), None, None)),
        ("weight", lambda: L.dl_ema_update(a, b, 16, float("inf"), None, g)),
        ("same buffer", lambda: L.dl_ema_update(a, a, 16, 0.1, None, None)),
    ]
    for word, call in cases:
        assert call() == -1, word
        err = L.dl_last_error()
        assert b"dl_ema_update" in err and word.encode() in err, (word, err)
    assert bytes(buf) == bytes(4096)


@pytest.mark.parametrize("bad", [1.0, 1.5, -0.1, float("nan"), float("inf"), "0.9", True])
def test_trainer_rejects_an_ema_decay_outside_zero_one(bad):
    from druglamp_amd.trainer import Trainer
    with pytest.raises(ValueError, match="ema_decay"):
        Trainer(None, None, ema_decay=bad)


def test_ops_wrapper_refuses_host_tensors_and_other_dtypes():
    from druglamp_amd import ops
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.ema_update(x, x.clone(), 0.1)
