"""The fp64 references of tests/loss_ref.py against the library formulations (the oracle's nt_xent, cos_rowloss and
triplet_sigcos, torch.nn.functional.cross_entropy) in fp64 on small shapes, values and autograd gradients to 1e-12
relative; the rank-split identity of the NT-Xent sides; chunked against unchunked evaluation; and the conditions
tests/test_loss_paths_gpu.py places on its references (weight of every streamed column, logit range, no ambiguous hinge)
for every case small enough for a CPU."""
import math

import pytest
import torch

from oracle import druglamp_oracle as O
from tests import loss_ref as R
from tests import test_loss_paths_gpu as G

F64 = torch.float64
TOL = 1e-12


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _qk(n, d, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g, dtype=F64) * scale, torch.randn(n, d, generator=g, dtype=F64) * scale


@pytest.mark.parametrize("n,d,T", [(1, 8, 0.5), (5, 16, 0.1), (33, 64, 0.1)])
def test_ntx_single_process_equals_the_oracle_value_and_gradient(n, d, T):
    q, k = _qk(n, d, n)
    qa, ka = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    ref = O.nt_xent(qa, ka, T)
    ref.backward()
    f = R.ntx_fwd(q, k, q, k, 0, 0, n, T)
    assert rel(f["row_loss"].mean(), ref.detach()) <= TOL
    assert bool(f["has_pos"].all())
    b = R.ntx_bwd(q, k, q, k, 0, 0, n, T, f["lse"], f["lse"], 1.0 / (2 * n))
    assert rel(b["dq"], qa.grad) <= TOL and rel(b["dk"], ka.grad) <= TOL
    assert bool((b["mag_dq"] >= b["dq"].abs() * (1 - 1e-12)).all()) and bool((b["mag_dk"] >= b["dk"].abs() * (1 - 1e-12)).all())


def test_ntx_three_way_rank_split_reproduces_the_single_process_loss_and_gradient():
    """Rows of rank r against all rows, then all rows against rank r's softmax rows (wmode 1 and 2): the rank means average
    to the full loss and query-side + summed key-side gradients are world x the full gradient; rows whose positive or own
    column the streamed side lacks take no such term."""
    n, d, world, T = 12, 16, 3, 0.1
    q, k = _qk(n, d, 5)
    qa, ka = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    ref = O.nt_xent(qa, ka, T)
    ref.backward()
    nl = n // world
    losses, dq, dk = [], torch.zeros_like(q), torch.zeros_like(k)
    for r in range(world):
        ql, kl = q[r * nl:(r + 1) * nl], k[r * nl:(r + 1) * nl]
        f = R.ntx_fwd(ql, kl, q, k, r * nl, 0, n, T)
        losses.append(float(f["row_loss"].mean()))
        b = R.ntx_bwd(ql, kl, q, k, r * nl, 0, n, T, f["lse"], None, 1.0 / (2 * nl))
        dq[r * nl:(r + 1) * nl] += b["dq"]
        dk[r * nl:(r + 1) * nl] += b["dk"]
        cb = R.ntx_bwd(q, k, ql, kl, 0, r * nl, n, T, None, f["lse"], 1.0 / (2 * nl))
        dq += cb["dq"]
        dk += cb["dk"]
        sw = R.ntx_fwd(q, k, ql, kl, 0, r * nl, n, T)                 # positives / own columns present for rank r's rows only
        want = torch.zeros(n, dtype=torch.bool)
        want[r * nl:(r + 1) * nl] = True
        assert torch.equal(sw["has_pos"], torch.cat((want, want)))
    assert rel(sum(losses) / world, ref.detach()) <= TOL
    assert rel(dq / world, qa.grad) <= TOL and rel(dk / world, ka.grad) <= TOL


def test_ntx_chunked_equals_unchunked_and_an_absent_positive_leaves_the_lse():
    n, d, T = 21, 16, 0.5
    q, k = _qk(40, d, 9)
    a = (q[7:7 + n], k[7:7 + n], q[3:33], k[3:33], 7, 3, 40, T)
    f1, f2 = R.ntx_fwd(*a, chunk=5), R.ntx_fwd(*a, chunk=1 << 20)
    for key in ("lse", "row_loss", "lam", "colw"):
        assert rel(f1[key], f2[key]) <= 1e-15, key
    la, lb = f1["lse"], R.ntx_fwd(a[2], a[3], a[0], a[1], 3, 7, 40, T)["lse"]
    for x, y in ((la, lb), (la, None), (None, lb)):
        b1, b2 = R.ntx_bwd(*a, x, y, 0.37, chunk=4), R.ntx_bwd(*a, x, y, 0.37, chunk=1 << 20)
        for key in ("dq", "dk", "mag_dq", "mag_dk", "lam"):
            assert rel(b1[key], b2[key]) <= 1e-15, key
    # a resident side whose positives lie outside the streamed side: row_loss is the bare log-sum-exp over all columns
    f = R.ntx_fwd(q[:4], k[:4], q[10:20], k[10:20], 0, 10, 40, T)
    assert not bool(f["has_pos"].any()) and torch.equal(f["row_loss"], f["lse"])
    A, B = torch.cat((q[:4], k[:4])), torch.cat((q[10:20], k[10:20]))
    assert rel(f["lse"], torch.logsumexp(A @ B.t() / T, 1)) <= TOL


def test_cos_rows_equal_the_oracle_and_take_the_piecewise_eps_semantics():
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(9, 20, generator=g, dtype=F64), torch.randn(9, 20, generator=g, dtype=F64)
    xa = x.clone().requires_grad_(True)
    rows = O.cos_rowloss(xa, y)
    wt = torch.linspace(-1, 2, 9, dtype=F64)
    (rows * wt).sum().backward()
    assert rel(R.cos_rows(x, y)["row_loss"], rows.detach()) <= TOL
    assert rel(R.cos_rows_bwd(x, y, 1.0)["dx"] * wt.unsqueeze(1), xa.grad) <= TOL
    assert rel(R.cos_rows_bwd(x, y, -0.3)["dx"], -0.3 * R.cos_rows_bwd(x, y, 1.0)["dx"]) <= TOL
    # clamped rows: x / eps, a constant divisor, so the second gradient term is zero
    x[0] = 0.0
    y[1] = 0.0
    x[2] = x[2] * (1e-20 / float(x[2].norm()))
    f, b = R.cos_rows(x, y), R.cos_rows_bwd(x, y, 1.0)
    assert float(f["row_loss"][0]) == 2.0 and float(f["row_loss"][1]) == 2.0
    assert rel(f["row_loss"][2], 2.0 - 2.0 * (x[2] * y[2]).sum() / (R.NORM_EPS * y[2].norm())) <= TOL
    assert rel(b["dx"][0], -2.0 * y[0] / (R.NORM_EPS * y[0].norm())) <= TOL
    assert rel(b["dx"][2], -2.0 * y[2] / (R.NORM_EPS * y[2].norm())) <= TOL and float(b["t2"][2].max()) == 0.0
    assert float(b["dx"][1].abs().max()) <= 1e-300 + float(2.0 * (x[1] * y[1]).sum().abs() * x[1].abs().max() / (x[1].norm() ** 3 * R.NORM_EPS))


@pytest.mark.parametrize("N,C,ld,Cp,ignore", [(1, 5, 5, 5, -100), (40, 27, 32, 32, 0), (33, 7, 9, 8, -100)])
def test_ce_rows_equal_torch_cross_entropy(N, C, ld, Cp, ignore):
    g = torch.Generator().manual_seed(N + C)
    x = torch.randn(N, ld, generator=g, dtype=F64) * 3
    y = torch.randint(0, C, (N,), generator=g)
    if ignore < 0 and N > 3:
        y[::3] = ignore
    xa = x.clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(xa[:, :C], y, ignore_index=ignore)
    (ref * 0.7).backward()
    f = R.ce_rows(x, y, C, ignore)
    assert rel(f["mean"], ref.detach()) <= TOL and f["count"] == int((y != ignore).sum())
    assert rel(f["lse"], torch.logsumexp(x[:, :C], 1)) <= TOL
    b = R.ce_rows_bwd(x, y, C, ignore, f["lse"], f["count"], 0.7, Cp)
    assert rel(b["dlogits"][:, :C], xa.grad[:, :C]) <= TOL
    assert float(b["dlogits"][:, C:].abs().max()) == 0.0 if Cp > C else True


def test_ce_rows_all_ignored_and_out_of_range_labels_give_nan():
    x = torch.randn(6, 8, dtype=F64)
    y = torch.zeros(6, dtype=torch.int64)
    f = R.ce_rows(x, y, 5, 0)
    assert math.isnan(f["mean"]) and f["count"] == 0
    assert float(R.ce_rows_bwd(x, y, 5, 0, f["lse"], 0, 1.0, 8)["dlogits"].abs().max()) == 0.0
    y = torch.tensor([1, 2, 5, 0, 3, 4])
    f = R.ce_rows(x, y, 5, 0)
    assert math.isnan(f["mean"]) and f["count"] == 5
    b = R.ce_rows_bwd(x, y, 5, 0, f["lse"], f["count"], 1.0, 8)
    assert float(b["dlogits"][2].abs().max()) == 0.0 and float(b["dlogits"][0].abs().max()) > 0.0
    y[2] = -3
    assert math.isnan(R.ce_rows(x, y, 5, 0)["mean"])


@pytest.mark.parametrize("n_p,n_d,dim,margin", [(1, 5, 4, 0.25), (6, 11, 16, 0.3), (4, 9, 70, 0.25)])
def test_triplet_equals_the_oracle_value_and_gradient(n_p, n_d, dim, margin):
    g = torch.Generator().manual_seed(n_p * n_d)
    p, d = torch.randn(n_p, dim, generator=g, dtype=F64), torch.randn(n_d, dim, generator=g, dtype=F64)
    u = torch.rand(n_p, n_d, generator=g)
    gt = torch.where(u < 0.3, -1, torch.where(u < 0.7, 0, 1)).to(torch.int8)
    gt[0][gt[0] == 1] = 0                            # anchor 0: negatives only (anchor as positive)
    if n_p > 3:
        gt[1][gt[1] == 0] = 1                        # no negatives
        gt[2] = -1                                   # all ignored
    pa, da = p.clone().requires_grad_(True), d.clone().requires_grad_(True)
    ref = O.triplet_sigcos(pa, da, gt.numpy(), margin)
    r = R.triplet(p, d, gt, margin)
    assert rel(r["loss"], ref.detach()) <= TOL
    assert r["hv"].numel() == r["n_tri"] and rel(r["hv"].clamp(min=0).sum(), r["hinge_sum"]) <= TOL
    if ref.requires_grad:
        ref.backward()
        assert rel(r["dp"], pa.grad) <= TOL and rel(r["dd"], da.grad) <= TOL
    assert bool((r["mag_dp"] >= r["dp"].abs() * (1 - 1e-12)).all()) and bool((r["mag_dd"] >= r["dd"].abs() * (1 - 1e-12)).all())


# ---- the conditions the GPU cases place on their references -------------------------------------------------------------------
CPU_NTX = [c for c in G.NTX_CASES if c.name not in G.NTX_BIG]


@pytest.mark.parametrize("c", CPU_NTX, ids=[c.name for c in CPU_NTX])
def test_ntx_case_conditions_hold(c):
    q, k = G.ntx_batch(c)
    refs = []
    for launch in c.launches:
        aq, ak, bq, bk = G.ntx_sides(q, k, launch)
        refs.append((launch, R.ntx_fwd(aq, ak, bq, bk, launch[0], launch[2], c.ng, c.T, chunk=8192)))
    G.ntx_conditions(c, refs)
    if c.kind == "equal":                            # identical rows: lse = s / T + log(#unmasked columns) exactly
        (a0, na, b0, nb, _), r = refs[0]
        s = float((q[0].double() ** 2).sum()) / c.T
        assert rel(r["lse"], torch.full_like(r["lse"], s + math.log(2 * nb - 1))) <= 1e-14
    if c.ng == 1:                                    # one pair: the only unmasked column is the positive, the loss is 0
        assert float(refs[0][1]["row_loss"].abs().max()) <= 1e-14 * float(refs[0][1]["lse"].abs().max())


def test_ntx_cases_name_every_instantiation_and_weight_loop():
    forms = {f for c in G.NTX_CASES for f in c.forms}
    for t in ("float", "bf16"):
        for d in (64, 128):
            for rt in ((1,) if t == "float" else (1, 2)):
                for w in ("fwd", "bwd"):
                    assert any(f.startswith("ntxent<%s,%d,%d,%s>" % (t, d, rt, w)) for f in forms), (t, d, rt, w)
    for c in G.NTX_CASES:                            # the form a case names is the one ntx_launch selects for its launches
        for a0, na, b0, nb, wm in c.launches:
            rt = 2 if (c.dt == G.BF and 2 * na >= 65536) else 1
            assert c.forms[0].startswith("ntxent<%s,%d,%d,fwd>" % ("bf16" if c.dt == G.BF else "float", c.d, rt)), c.name
            assert a0 + na <= c.ng and b0 + nb <= c.ng
    assert {w for c in G.NTX_CASES for l in c.launches for w in l[4]} == {0, 1, 2}


@pytest.mark.parametrize("c", G.TRI_CASES, ids=[c.name for c in G.TRI_CASES])
def test_triplet_case_conditions_hold(c):
    p, d, gt = G.tri_data(c)
    r = R.triplet(p, d, gt, c.margin)
    G.triplet_conditions(c, r)
    assert r["n_tri"] > 0 and (c.n_d <= 5 or bool((r["hv"] <= 0).any()))      # hinges on both sides of zero
    pos, neg = (gt == 1).sum(1), (gt == 0).sum(1)
    if c.n_d == 8192:
        assert pos.tolist() == [3, 0] and neg.tolist() == [8189, 8192]
    elif c.n_p == 3:
        assert int((pos[0] * neg[0])) > 256 and int(pos[1]) == 0 and int(neg[1]) > 0 and int(neg[2]) == 0
    else:
        assert int(pos[0]) == 0 and int(neg[0]) > 0
        if c.n_p >= 5:
            assert int(neg[1]) == 0 and int((gt[2] == -1).sum()) == c.n_d and bool(((pos > 0) & (neg > 0)).any())
