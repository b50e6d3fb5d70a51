"""The fp64 attention reference of tests/attn_ref.py against torch autograd of the plain softmax formula (CPU only): paired
segments with the model's shift and a general one, key multiplicities against explicitly expanded keys, strided gathers.
tests/test_attention_paths_gpu.py checks every kernel form against this reference."""
import math

import pytest
import torch

from tests.attn_ref import reference_bwd, reference_fwd


def _plain(Q, K, V, scale):
    """[P][H][L][hd] float64 leaves -> O, LSE, logits of softmax(scale Q K^T) V."""
    s = scale * (Q @ K.transpose(-1, -2))
    return torch.softmax(s, -1) @ V, torch.logsumexp(s, -1), s


def _close(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.allclose(a, b, rtol=1e-10, atol=1e-12), float((a - b).abs().max())


@pytest.mark.parametrize("P,shift", [(4, 2), (3, 1), (5, 3)])
def test_paired_reference_equals_autograd(P, shift):
    H, Lq, Lk, hd, scale = 2, 5, 7, 8, 0.4
    g = torch.Generator().manual_seed(P * 10 + shift)
    q, k, v = (torch.randn(P, H, L, hd, generator=g, dtype=torch.float64) for L in (Lq, Lk, Lk))
    do = torch.randn(2, P, H, Lq, hd, generator=g, dtype=torch.float64)
    cs = lambda L: (H * L * hd, L * hd, hd)                                       # noqa: E731  contiguous [P][H][L][hd]
    f = reference_fwd(q, k, v, n_problems=P, n_heads=H, n_segments=2, partner_shift=shift, Lq=Lq, Lk=Lk, head_dim=hd,
                      scale=scale, q_strides=cs(Lq), k_strides=cs(Lk), v_strides=cs(Lk))
    b = reference_bwd(f, do, do_strides=cs(Lq), do_ss=P * H * Lq * hd, scale=scale)
    Q, K, V = (t.clone().requires_grad_(True) for t in (q, k, v))
    partner = [(p + shift) % P for p in range(P)]
    o0, l0, s0 = _plain(Q, K, V, scale)
    o1, l1, _ = _plain(Q[partner], K, V, scale)
    ((o0 * do[0]).sum() + (o1 * do[1]).sum()).backward()
    _close(f["O"][0], o0.detach())
    _close(f["O"][1], o1.detach())
    _close(f["LSE"], torch.stack([l0, l1]).detach())
    _close(f["raw"], s0.detach())
    _close(b["dQ"], Q.grad)
    _close(b["dK"], K.grad)
    _close(b["dV"], V.grad)
    # the magnitudes bound the values they describe
    for name in ("O", "dQ", "dK", "dV"):
        val, mag = (f[name].abs(), f["mag_" + name]) if name == "O" else (b[name].abs(), b["mag_" + name])
        assert (val <= mag * (1 + 1e-12) + 1e-300).all(), name
    assert (f["raw"].abs() <= f["mag_raw"] * (1 + 1e-12)).all()


@pytest.mark.parametrize("lead,tail,w", [(5, 1, 3.0), (3, 4, 2.5), (0, 6, 7.0), (4, 2, 1.0)])
def test_key_multiplicities_equal_expanded_keys(lead, tail, w):
    P, H, Lq, hd, scale = 2, 2, 6, 8, 0.3
    g = torch.Generator().manual_seed(lead * 7 + tail)
    Lk = lead + tail
    q = torch.randn(P, H, Lq, hd, generator=g, dtype=torch.float64)
    k, v = (torch.randn(P, H, Lk, hd, generator=g, dtype=torch.float64) for _ in range(2))
    do = torch.randn(P, H, Lq, hd, generator=g, dtype=torch.float64)
    cs = lambda L: (H * L * hd, L * hd, hd)                                       # noqa: E731
    f = reference_fwd(q, k, v, n_problems=P, n_heads=H, n_segments=1, partner_shift=0, Lq=Lq, Lk=Lk, head_dim=hd,
                      scale=scale, q_strides=cs(Lq), k_strides=cs(Lk), v_strides=cs(Lk), key_tail=(tail, w))
    b = reference_bwd(f, do, do_strides=cs(Lq), do_ss=0, scale=scale)
    # the expanded key set: a non-integer weight w = n + frac is n copies of the key plus one whose weight is frac, i.e. a key
    # whose logit carries + log(frac) — the autograd side adds that log explicitly, the reference gets it from key_tail
    n = int(math.floor(w))
    frac = w - n
    reps = n + (1 if frac > 0 else 0)
    Q, K, V = (t.clone().requires_grad_(True) for t in (q, k, v))
    Ke = torch.cat([K[:, :, :lead]] + [K[:, :, lead:]] * reps, 2)
    Ve = torch.cat([V[:, :, :lead]] + [V[:, :, lead:]] * reps, 2)
    bias = torch.zeros(Ke.shape[2], dtype=torch.float64)
    if frac > 0:
        bias[lead + n * tail:] = math.log(frac)
    s = scale * (Q @ Ke.transpose(-1, -2)) + bias
    o = torch.softmax(s, -1) @ Ve
    (o * do).sum().backward()
    _close(f["O"][0], o.detach())
    _close(f["LSE"][0], torch.logsumexp(s, -1).detach())
    _close(b["dQ"], Q.grad)
    _close(b["dK"], K.grad)                            # autograd of the expanded keys sums over the copies of a tail key
    _close(b["dV"], V.grad)
    # raw logits of a tail key carry + log(w): softmax over a raw row gives the weights of the distinct keys
    _close(f["raw"][..., :lead], (scale * (q @ k.transpose(-1, -2)))[..., :lead])
    _close(f["raw"][..., lead:], (scale * (q @ k.transpose(-1, -2)))[..., lead:] + math.log(w))


def test_strided_gathers_equal_contiguous_operands():
    """Separate buffers with row pitches wider than H*hd, problem and head strides out of order, o / dO segments apart
    by a stride that is not d, and the fused [P][L][3d] layout: the same numbers as contiguous operands."""
    P, H, Lq, Lk, hd, scale, shift = 3, 2, 4, 5, 8, 0.5, 1
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(P, H, L, hd, generator=g, dtype=torch.float64) for L in (Lq, Lk, Lk))
    do = torch.randn(2, P, H, Lq, hd, generator=g, dtype=torch.float64)
    cs = lambda L: (H * L * hd, L * hd, hd)                                       # noqa: E731
    kw = dict(n_problems=P, n_heads=H, n_segments=2, partner_shift=shift, Lq=Lq, Lk=Lk, head_dim=hd, scale=scale)
    ref = reference_fwd(q, k, v, q_strides=cs(Lq), k_strides=cs(Lk), v_strides=cs(Lk), **kw)
    bref = reference_bwd(ref, do, do_strides=cs(Lq), do_ss=P * H * Lq * hd, scale=scale)
    # pitched rows: [P][L][pitch] with heads hd apart
    pitch = H * hd + 8
    qb = torch.full((P, Lq, pitch), float("nan"), dtype=torch.float64)
    qb[:, :, :H * hd] = q.permute(0, 2, 1, 3).reshape(P, Lq, H * hd)
    # head-major K: [H][P][Lk][hd + 8] (problem stride smaller than head stride)
    kb = torch.full((H, P, Lk, hd + 8), float("nan"), dtype=torch.float64)
    kb[..., :hd] = k.permute(1, 0, 2, 3)
    # fused [P][L][3d] for V (at column 2d), like the projection GEMM writes q, k, v
    L, d = max(Lq, Lk), H * hd
    vb = torch.full((P, L, 3 * d), float("nan"), dtype=torch.float64)
    vb[:, :Lk, 2 * d:] = v.permute(0, 2, 1, 3).reshape(P, Lk, d)
    got = reference_fwd(qb, kb, vb[..., 2 * d:], q_strides=(Lq * pitch, hd, pitch),
                        k_strides=((Lk * (hd + 8)), P * Lk * (hd + 8), hd + 8), v_strides=(L * 3 * d, hd, 3 * d), **kw)
    for name in ("O", "LSE", "raw", "mag_O", "mag_lse"):
        _close(got[name], ref[name])
    # dO with segments o_ss = d apart inside rows of 2d (the model's [attn | attn_p]) and a given O laid out the same way
    dob = torch.full((P, Lq, 2 * d + 8), float("nan"), dtype=torch.float64)
    ob = torch.full((P, Lq, 2 * d + 8), float("nan"), dtype=torch.float64)
    for s in range(2):
        dob[:, :, s * d:(s + 1) * d] = do[s].permute(0, 2, 1, 3).reshape(P, Lq, d)
        ob[:, :, s * d:(s + 1) * d] = ref["O"][s].permute(0, 2, 1, 3).reshape(P, Lq, d)
    st = (Lq * (2 * d + 8), hd, 2 * d + 8)
    bgot = reference_bwd(got, dob, do_strides=st, do_ss=d, scale=scale, o=ob, o_strides=st, o_ss=d)
    for name in ("dQ", "dK", "dV", "mag_dQ", "mag_dK", "mag_dV"):
        _close(bgot[name], bref[name])
