"""The three ops.adamw_step* wrappers validate their tensors alike (ops._adamw, in front of csrc/optim.hip): a CPU tensor, a
float64 gradient, moments of another size and a non-contiguous parameter raise before the library is called, and param, grad,
exp_avg and exp_avg_sq keep their bits.  n = 8: two 16-byte chunks."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = 8
KW = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=3)


def _bits(t):
    return t.view(torch.int32)


def _forms():
    from druglamp_amd import ops
    guard = torch.tensor([0.5, 2.0, 0.0, 0.0], device=DEV)
    quads = torch.zeros((N + 3) // 4, dtype=torch.uint8, device=DEV)
    tab = torch.tensor([[1.0, 1e-2]], device=DEV)
    return [("adamw_step", lambda p, g, m, v: ops.adamw_step(p, g, m, v, **KW)),
            ("adamw_step_guarded", lambda p, g, m, v: ops.adamw_step_guarded(p, g, m, v, guard, **KW)),
            ("adamw_step_groups", lambda p, g, m, v: ops.adamw_step_groups(p, g, m, v, quads, tab, **KW)),
            ("adamw_step_groups+guard", lambda p, g, m, v: ops.adamw_step_groups(p, g, m, v, quads, tab, guard=guard, **KW))]


@pytest.mark.parametrize("form", range(4), ids=["plain", "guarded", "groups", "groups_guarded"])
def test_bad_tensors_raise_and_nothing_is_written(form):
    name, call = _forms()[form]
    gen = torch.Generator().manual_seed(8)
    wide = torch.randn(2 * N, generator=gen).to(DEV)            # the non-contiguous parameter is every other element of it
    t = [torch.randn(N, generator=gen).to(DEV) for _ in range(3)] + [torch.rand(N, generator=gen).to(DEV)]
    keep = [x.clone() for x in t] + [wide.clone()]
    p, g, m, v = t
    with pytest.raises(RuntimeError, match="device tensors"):
        call(p.cpu(), g, m, v)
    with pytest.raises(RuntimeError, match="device tensors"):
        call(p, g, m, v.cpu())
    with pytest.raises(TypeError, match="grad must be float32"):
        call(p, g.double(), m, v)
    with pytest.raises(ValueError, match="exp_avg has %d elements" % (N - 4)):
        call(p, g, m[:N - 4], v)
    with pytest.raises(ValueError, match="param must be contiguous"):
        call(wide[::2], g, m, v)
    torch.cuda.synchronize()
    for x, y in zip(keep, t + [wide]):
        assert torch.equal(_bits(x), _bits(y)), name
    call(p, g, m, v)                                             # the probe works: the same operands, valid, are stepped
    torch.cuda.synchronize()
    assert not torch.equal(_bits(keep[0]), _bits(p)) and torch.equal(_bits(keep[1]), _bits(g))
