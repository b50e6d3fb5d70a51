"""GuidedCrossAttention(need_weights=True, need_raw=False): the stock MultiheadAttention contract — the softmax weights
averaged over the heads as the second output (guided_cross_attention_model.py:324-327) — written by dl_attn_probs from the
forward's projections and LSE, also over compact keys (key_tail), where the map is expanded to the full key count."""
import pytest
import torch

from tests.helpers import T, det_state_dict, load, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_TOL, BF16_TOL = 1e-4, 3e-2


def _module(H, dtype, sd=None):
    from druglamp_amd.model.PGCA import GuidedCrossAttention
    m = GuidedCrossAttention(embed_dim=128, num_heads=H)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    else:
        with torch.no_grad():                           # (the constructor zeroes the biases: give them values)
            m.in_proj_bias.copy_(T("pgca_w.in_b", (384,), 0.2))
            m.out_proj.bias.copy_(T("pgca_w.out_b", (128,), 0.2))
    m = m.to(DEV).eval()
    m.compute_dtype = dtype
    return m


def _weights_fp64(m, q, kv):
    """The head-averaged softmax weights (B, Lq, Lk) restated in fp64 torch from the module's parameters; q / kv seq-first."""
    E, H = m.embed_dim, m.num_heads
    hd = E // H
    w, b = m.in_proj_weight.detach().double(), m.in_proj_bias.detach().double()
    qp = q.detach().double().transpose(0, 1) @ w[:E].T + b[:E]                    # (B, Lq, E)
    kp = kv.detach().double().transpose(0, 1) @ w[E:2 * E].T + b[E:2 * E]         # (B, Lk, E)
    B, Lq, Lk = qp.shape[0], qp.shape[1], kp.shape[1]
    qh = qp.view(B, Lq, H, hd).transpose(1, 2)
    kh = kp.view(B, Lk, H, hd).transpose(1, 2)
    return torch.softmax(qh @ kh.transpose(-1, -2) * hd ** -0.5, -1).mean(1)


def test_one_head_weights_against_the_raw_logits_and_fp64_and_the_golden_backward():
    Lq, Lk, B = 48, 80, 3
    g = load("pgca_small")
    m = _module(1, torch.float32, det_state_dict(g))
    q = T("pgca_small.q", (Lq, B, 128)).to(DEV).requires_grad_(True)
    kv = T("pgca_small.kv", (Lk, B, 128)).to(DEV).requires_grad_(True)
    out, wts = m(q, kv, kv, need_weights=True, need_raw=False)
    assert tuple(wts.shape) == (B, Lq, Lk) and wts.dtype == torch.float32
    assert not wts.requires_grad and wts.grad_fn is None                          # detached
    out_r, raw = m(q, kv, kv, need_weights=True, need_raw=True)
    assert relerr(wts, torch.softmax(raw.double(), -1)[:, 0]) <= F32_TOL
    assert relerr(wts, _weights_fp64(m, q, kv)) <= F32_TOL
    assert relerr(wts.double().sum(-1), torch.ones(B, Lq, dtype=torch.float64)) <= 1e-5
    out_n, none = m(q, kv, kv, need_weights=False)
    assert none is None
    assert torch.equal(out, out_n) and torch.equal(out, out_r)
    assert relerr(out, g["out"]) <= F32_TOL
    (out * T("pgca_small.G", tuple(out.shape)).to(DEV)).sum().backward()
    assert relerr(q.grad, g["dq"]) <= F32_TOL * 3
    assert relerr(kv.grad, g["dkv"]) <= F32_TOL * 3


@pytest.mark.parametrize("dtype,tol", [(torch.float32, F32_TOL), (torch.bfloat16, BF16_TOL)])
def test_two_heads_are_averaged(dtype, tol):
    Lq, Lk, B = 70, 130, 3
    torch.manual_seed(5)
    m = _module(2, dtype)
    q = T("pgca_w2.q", (Lq, B, 128)).to(DEV)
    kv = T("pgca_w2.kv", (Lk, B, 128)).to(DEV)
    with torch.no_grad():
        out, wts = m(q, kv, kv, need_weights=True, need_raw=False)
        out_n, _ = m(q, kv, kv, need_weights=False)
    assert tuple(wts.shape) == (B, Lq, Lk) and wts.dtype == torch.float32
    assert torch.equal(out, out_n)
    assert relerr(wts, _weights_fp64(m, q, kv)) <= tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, F32_TOL), (torch.bfloat16, BF16_TOL)])
def test_compact_keys_give_the_map_of_the_full_key_set(dtype, tol):
    """40 distinct rows + 8 tail rows of weight 5 against the same module over the 80 rows they stand for (the 40 rows followed
    by functional.ExpandTailFn's expansion of the tail)."""
    from druglamp_amd import functional as Fn
    Lq, B, lead, tail, w = 48, 3, 40, 8, 5
    torch.manual_seed(6)
    m = _module(1, dtype, det_state_dict(load("pgca_small")))
    q = T("pgca_wt.q", (Lq, B, 128)).to(DEV)
    kc = T("pgca_wt.kv", (lead + tail, B, 128)).to(DEV)
    kfull = Fn.ExpandTailFn.apply(kc.transpose(0, 1).contiguous(), lead, w).transpose(0, 1)
    assert kfull.shape[0] == 80
    with torch.no_grad():
        out_c, w_c = m(q, kc, kc, need_weights=True, need_raw=False, key_tail=(tail, w))
        out_f, w_f = m(q, kfull, kfull, need_weights=True, need_raw=False)
        out_n, _ = m(q, kc, kc, need_weights=False, key_tail=(tail, w))
    assert tuple(w_c.shape) == (B, Lq, 80) and tuple(w_f.shape) == (B, Lq, 80)
    assert torch.equal(out_c, out_n)
    assert relerr(w_c, w_f) <= tol
    if dtype == torch.float32:
        assert relerr(w_c, _weights_fp64(m, q, kfull)) <= tol
    assert relerr(out_c, out_f) <= tol
    with pytest.raises(ValueError):
        m(q, kc, kc, need_weights=True, need_raw=True, key_tail=(tail, w))


def test_raw_and_probs_together_are_refused():
    from druglamp_amd import functional as Fn
    m = _module(1, torch.float32)
    q = torch.zeros(16, 1, 128, device=DEV)
    with pytest.raises(ValueError):
        Fn.GuidedCrossAttentionFn.apply(q, q, m.in_proj_weight, m.in_proj_bias, m.out_proj.weight, m.out_proj.bias, 1, True, None, True)
