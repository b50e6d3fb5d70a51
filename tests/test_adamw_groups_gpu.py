"""dl_adamw_step_groups (csrc/optim.hip) through druglamp_amd.ops: the bit contract of include/druglamp_hip.h.

For every maximal segment of equal group id the result is dl_adamw_step (guard null) / dl_adamw_step_guarded on that segment
alone with lr = float32(lr) * float32(lr_scale) and the group's weight decay, BIT FOR BIT, in param, exp_avg, exp_avg_sq and
the low-precision image — which ties the kernel to the fp64-bounded pin tests/test_elem_paths_gpu.py holds on dl_adamw_step;
no tolerance appears here.  Comparisons are on int32 / int16 views (pattern of tests/test_grad_guard_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import param_groups_ref as pr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KW = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=3)
NAMES = ("param", "grad", "exp_avg", "exp_avg_sq", "lowp")
# {lr_scale, weight_decay}: the issue's four groups and one no chunk belongs to
TAB = [(1.0, 1e-2), (0.1, 0.0), (0.0, 1e-2), (3.0, 0.5), (7.0, 0.25)]


def _operands(n, lowp, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(DEV)
    grad = (torch.randn(n, generator=g) * 3).to(DEV)
    m = (torch.randn(n, generator=g) * 0.1).to(DEV)
    v = (torch.rand(n, generator=g) * 0.01).to(DEV)
    lp = None if lowp is None else torch.full((n,), 5.0, dtype=lowp, device=DEV)
    return p, grad, m, v, lp


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b, what=""):
    for x, y, name in zip(a, b, NAMES):
        if x is not None:
            assert torch.equal(_bits(x), _bits(y)), (name, what)


def _tab(rows=TAB):
    return torch.tensor(rows, dtype=torch.float32, device=DEV)


def _quads(n):
    """Ids that alternate on consecutive chunks at the start (neighbouring lanes differ), segments of every group behind them, at
    n = 1028 a boundary at element 1024 (the workgroup boundary: 256 threads x 4 elements); at n = 1003 the last segment ends in
    the scalar tail (3 elements)."""
    nq = (n + 3) // 4
    q = ([c % 4 for c in range(24)] + [1] * 40 + [3] * 100 + [2] * 50 + [0] * (256 - 214) + [2] * 8)[:nq]
    assert len(q) == nq and (nq <= 256 or q[255] != q[256]) and set(q) == {0, 1, 2, 3}
    return q


def _per_segment(ops_fn, t, quads, rows, guard=None, gscale=1.0):
    """The expectation: one ungrouped call per maximal segment, on the operands' own slices."""
    n = t[0].numel()
    vals = pr.group_values(rows, KW["lr"])
    for s, e, k in pr.segments(quads, n):
        if k >= len(rows):
            continue
        kw = dict(KW, lr=vals[k][0], weight_decay=vals[k][1], grad_scale=gscale, lowp=None if t[4] is None else t[4][s:e])
        args = (t[0][s:e], t[1][s:e], t[2][s:e], t[3][s:e]) + (() if guard is None else (guard,))
        ops_fn(*args, **kw)


@pytest.mark.parametrize("lowp", [None, torch.float32, torch.bfloat16], ids=["nolowp", "lowp32", "lowp16"])
@pytest.mark.parametrize("n", [1, 4, 1003, 1028])
def test_a_single_group_is_adamw_step(n, lowp):
    from druglamp_amd import ops
    for wd, gscale in ((1e-2, 1.0), (0.0, 0.5), (0.3, 0.125)):
        a, b = _operands(n, lowp, seed=n), _operands(n, lowp, seed=n)
        ops.adamw_step(a[0], a[1], a[2], a[3], weight_decay=wd, grad_scale=gscale, lowp=a[4], **KW)
        q = torch.zeros((n + 3) // 4, dtype=torch.uint8, device=DEV)
        ops.adamw_step_groups(b[0], b[1], b[2], b[3], q, _tab([(1.0, wd)]), grad_scale=gscale, lowp=b[4], **KW)
        _same(a, b, (wd, gscale))
        assert not torch.equal(a[0], _operands(n, lowp, seed=n)[0])              # (the step did move the parameters)


@pytest.mark.parametrize("lowp", [None, torch.float32, torch.bfloat16], ids=["nolowp", "lowp32", "lowp16"])
@pytest.mark.parametrize("n", [1028, 1003])
def test_several_groups_equal_a_per_segment_adamw_step(n, lowp):
    from druglamp_amd import ops
    quads = _quads(n)
    a, b = _operands(n, lowp, seed=n + 1), _operands(n, lowp, seed=n + 1)
    _per_segment(ops.adamw_step, a, quads, TAB, gscale=0.5)
    ops.adamw_step_groups(b[0], b[1], b[2], b[3], torch.tensor(quads, dtype=torch.uint8, device=DEV), _tab(), grad_scale=0.5,
                          lowp=b[4], **KW)
    _same(a, b)
    start = _operands(n, lowp, seed=n + 1)
    assert bool((_bits(b[2]) != _bits(start[2])).float().mean() > 0.99)          # every group moved its elements (lr_scale 0: the moments)
    moved = (_bits(b[0]) != _bits(start[0])).cpu()
    ids = torch.tensor(quads).repeat_interleave(4)[:n]
    assert not bool(moved[ids == 2].any()) and bool(moved[ids != 2].float().mean() > 0.99)    # lr 0: p * 1 - 0 * (m / denom)
    # the fp64 restatement agrees within the fp32 arithmetic's few roundings (a sanity link; the bound on dl_adamw_step is
    # tests/test_elem_paths_gpu.py's, and the bits above carry it over)
    want, _, _ = pr.adamw_groups(start[0], start[1], start[2], start[3], quads, TAB, KW["lr"], KW["beta1"], KW["beta2"], KW["eps"],
                                 KW["step"], 0.5)
    assert float((b[0].cpu().double() - want).abs().max()) <= 1e-5


@pytest.mark.parametrize("lowp", [None, torch.bfloat16], ids=["nolowp", "lowp16"])
@pytest.mark.parametrize("n", [1028, 1003])
def test_with_a_guard_that_does_not_skip_it_is_a_per_segment_adamw_step_guarded(n, lowp):
    from druglamp_amd import ops
    quads = _quads(n)
    guard = torch.tensor([0.37, 123.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    a, b = _operands(n, lowp, seed=n + 2), _operands(n, lowp, seed=n + 2)
    _per_segment(ops.adamw_step_guarded, a, quads, TAB, guard=guard, gscale=0.5)
    ops.adamw_step_groups(b[0], b[1], b[2], b[3], torch.tensor(quads, dtype=torch.uint8, device=DEV), _tab(), grad_scale=0.5,
                          lowp=b[4], guard=guard, **KW)
    _same(a, b)
    c = _operands(n, lowp, seed=n + 2)                                            # ... and adamw_step at the effective scale
    _per_segment(ops.adamw_step, c, quads, TAB, gscale=float(np.float32(0.5) * np.float32(0.37)))
    _same(c, b)


@pytest.mark.parametrize("lowp", [None, torch.float32, torch.bfloat16], ids=["nolowp", "lowp32", "lowp16"])
def test_a_skipped_step_writes_nothing(lowp):
    from druglamp_amd import ops
    n = 1003
    guard = torch.tensor([0.0, float("nan"), 1.0, 0.0], dtype=torch.float32, device=DEV)
    b = _operands(n, lowp, seed=9)
    b[1].fill_(float("nan"))
    keep = [None if t is None else t.clone() for t in b]
    ops.adamw_step_groups(b[0], b[1], b[2], b[3], torch.tensor(_quads(n), dtype=torch.uint8, device=DEV), _tab(), grad_scale=0.5,
                          lowp=b[4], guard=guard, **KW)
    _same(keep, b, "skipped step wrote")


@pytest.mark.parametrize("n", [1028, 1003])
def test_chunks_with_an_id_beyond_the_table_keep_their_bits(n):
    from druglamp_amd import ops
    quads = _quads(n)
    rows = TAB[:3]                                       # ids 3 (a whole segment and alternating chunks) have no row now
    for c in (5, 200, (n + 3) // 4 - 1):                 # ... and so have 255 and 64 (the last one owns the scalar tail at n = 1003)
        quads[c] = 255 if c != 200 else 64
    a, b = _operands(n, torch.bfloat16, seed=n + 3), _operands(n, torch.bfloat16, seed=n + 3)
    start = _operands(n, torch.bfloat16, seed=n + 3)
    _per_segment(ops.adamw_step, a, quads, rows)
    ops.adamw_step_groups(b[0], b[1], b[2], b[3], torch.tensor(quads, dtype=torch.uint8, device=DEV), _tab(rows), lowp=b[4], **KW)
    _same(a, b)
    dead = torch.tensor([k >= 3 for k in quads], device=DEV).repeat_interleave(4)[:n]
    assert int(dead.sum()) > 400
    for x, y, name in zip(start, b, NAMES):
        assert torch.equal(_bits(x)[dead], _bits(y)[dead]), name
    assert bool((_bits(start[2])[~dead] != _bits(b[2])[~dead]).float().mean() > 0.99)


def test_two_launches_give_equal_bits():
    from druglamp_amd import ops
    n = 1003
    q = torch.tensor(_quads(n), dtype=torch.uint8, device=DEV)
    guard = torch.tensor([0.37, 1.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2):
        b = _operands(n, torch.bfloat16, seed=21)
        ops.adamw_step_groups(b[0], b[1], b[2], b[3], q, _tab(), grad_scale=0.5, lowp=b[4], guard=guard, **KW)
        outs.append(b)
    _same(outs[0], outs[1])


def test_argument_errors_are_reported_before_any_launch():
    from druglamp_amd import _lib, ops
    L = _lib.lib()
    n = 1003
    t = _operands(n, None, seed=1)
    keep = [x.clone() for x in t[:4]]
    q = torch.zeros((n + 3) // 4, dtype=torch.uint8, device=DEV)
    tab = _tab([(1.0, 1e-2)])
    guard = torch.zeros(8, dtype=torch.float32, device=DEV)
    good = dict(param=t[0].data_ptr(), grad=t[1].data_ptr(), m=t[2].data_ptr(), v=t[3].data_ptr(), n=n, step=3, quads=q.data_ptr(),
                tab=tab.data_ptr(), n_groups=1, guard=None)

    def call(**over):
        a = dict(good, **over)
        return L.dl_adamw_step_groups(a["param"], a["grad"], a["m"], a["v"], a["n"], 1e-3, 0.9, 0.999, 1e-8, a["step"], 1.0, None, 0,
                                      a["quads"], a["tab"], a["n_groups"], a["guard"], None)

    cases = [("param", None), ("grad", None), ("m", None), ("v", None), ("quads", None), ("tab", None), ("n", 0), ("n", -4),
             ("step", 0), ("n_groups", 0), ("n_groups", 65), ("n_groups", -1), ("guard", guard.data_ptr() + 4)]
    for key, val in cases:
        rc = call(**{key: val})
        msg = L.dl_last_error().decode()
        assert rc != 0 and "dl_adamw_step_groups" in msg, (key, val, rc, msg)
    torch.cuda.synchronize()
    for x, y in zip(keep, t[:4]):
        assert torch.equal(_bits(x), _bits(y))           # nothing was launched
    assert call() == 0 and call(n_groups=64, guard=guard.data_ptr() + 16) == 0       # (64 groups and an aligned guard are fine)
    # the wrapper's own checks
    with pytest.raises(ValueError, match="quad_group"):
        ops.adamw_step_groups(t[0], t[1], t[2], t[3], q[:-1], tab, **KW)
    with pytest.raises(ValueError, match="group_tab"):
        ops.adamw_step_groups(t[0], t[1], t[2], t[3], q, tab.double(), **KW)
    with pytest.raises(RuntimeError, match="n_groups"):
        ops.adamw_step_groups(t[0], t[1], t[2], t[3], q, torch.zeros(65, 2, device=DEV), **KW)
