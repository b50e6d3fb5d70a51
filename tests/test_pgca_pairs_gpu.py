"""dl_pgca_pairs_fwd (csrc/pgca_pairs.hip) through ops.pgca_pairs, element-wise against the fp64 reference of tests/attn_ref.py
run on the explicitly gathered Q[pi], K[di], V[di] (n_problems = n_pairs, one head).

Bound: |O - ref| <= tau_O (mag_O + |bias|).  tau_O is the rounding model written out in tests/test_attention_paths_gpu.py
(read it there; restated below with the same constants): the kernel performs the arithmetic of the streamed forward — bf16
products exact in fp32, fp32 accumulation, online maximum / sum, P rounded to bf16 in front of the PV product (bf16 only),
one rounding at the store — so no new tolerance is invented.  The bias is added in fp32 in front of that one store; its
rounding is relative to |O + bias| <= mag_O + |bias|.  The left copy is compared bitwise.

Every buffer is NaN outside the addressed elements: inputs (a stray read poisons the result), `out` (every addressed
element must be overwritten, every other element must stay bitwise unchanged), and each code buffer carries one
never-referenced NaN-filled entity behind the entities the call is told about.

DL_PGCA_BOUND_LOG=<file>: every check appends one JSON line (case, dtype, worst |err| / bound).
"""
import collections
import functools
import json
import os

import pytest
import torch

from tests.attn_ref import reference_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32

# ---- rounding model (tests/test_attention_paths_gpu.py, same constants) ----------------------------------------------------
U_B, U_F = 2.0 ** -8, 2.0 ** -24
LAM, HD, LEN, MARGIN = 96.0, 128, 2048, 2.0
E_S = (HD + 2) * U_F * LAM
E_LSE = E_S + (LEN + 4) * U_F
TAU_O = {BF: MARGIN * (2 * U_B + E_S + E_LSE + LEN * U_F), F32: MARGIN * (E_S + E_LSE + (LEN + 2) * U_F)}

E = 128
Case = collections.namedtuple("Case", "name n_q n_kv pi di Lq Lk tail left_cols pitch bias pad")
_A_PI, _A_DI = (2, 0, 1, 0, 2, 2, 1), (3, 3, 0, 2, 1, 3, 0)          # repeated and permuted indices
CASES = {
    "a_compact": Case("a_compact", 3, 4, _A_PI, _A_DI, 256, 136, (8, 47.0), 128, 256, False, 0),
    "b_full_keys": Case("b_full_keys", 3, 4, _A_PI, _A_DI, 256, 512, None, 128, 256, False, 0),
    "c_partial_tiles": Case("c_partial_tiles", 2, 2, (1, 0, 1), (0, 1, 1), 40, 40, None, 0, 136, False, 0),
    "d_tail_bias_padded": Case("d_tail_bias_padded", 2, 2, (1,), (0,), 72, 200, (8, 3.0), 128, 256, True, 3),
    "e_many_pairs": Case("e_many_pairs", 2, 2, tuple(i % 2 for i in range(300)), tuple((i // 2) % 2 for i in range(300)), 64, 64,
                         None, 128, 256, False, 0),
}
PARAMS = [("a_compact", BF), ("a_compact", F32), ("b_full_keys", BF), ("c_partial_tiles", BF), ("c_partial_tiles", F32),
          ("d_tail_bias_padded", BF), ("e_many_pairs", BF)]
G = 256             # guard band of NaN elements in front of and behind every buffer


def _nan_view(n_ent, L, cols, dt, pad_rows, fill):
    """(n_ent + 1, L, cols) view, entity stride (L + pad_rows) * cols, of a NaN buffer with guard bands; entities < n_ent get
    `fill` (n_ent, L, cols), the spare entity and the gaps stay NaN."""
    es = (L + pad_rows) * cols
    flat = torch.full(((n_ent + 1) * es + 2 * G,), float("nan"), device=DEV, dtype=dt)
    v = torch.as_strided(flat, (n_ent + 1, L, cols), (es, cols, 1), G)
    v[:n_ent].copy_(fill)
    return v


@functools.lru_cache(maxsize=None)
def _setup(name, dt):
    """Inputs of a case and its fp64 reference (computed once, shared by the tests that use the case, never modified)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    scale = E ** -0.5
    q = _nan_view(c.n_q, c.Lq, E, dt, c.pad, torch.randn(c.n_q, c.Lq, E, generator=g) * 0.7)
    kvf = torch.cat([torch.randn(c.n_kv, c.Lk, E, generator=g) * 0.7, torch.randn(c.n_kv, c.Lk, E, generator=g)], dim=2)
    kv = _nan_view(c.n_kv, c.Lk, 2 * E, dt, c.pad, kvf)
    left = _nan_view(c.n_q, c.Lq, c.left_cols, dt, c.pad, torch.randn(c.n_q, c.Lq, c.left_cols, generator=g)) if c.left_cols else None
    bias = (torch.randn(E, generator=g) * 0.5).to(DEV) if c.bias else None
    pi = torch.tensor(c.pi, dtype=torch.int32, device=DEV)
    di = torch.tensor(c.di, dtype=torch.int32, device=DEV)
    n = len(c.pi)
    Qg, Kg, Vg = q[pi.long()].contiguous(), kv[di.long(), :, :E].contiguous(), kv[di.long(), :, E:].contiguous()
    ref = reference_fwd(Qg, Kg, Vg, n_problems=n, n_heads=1, n_segments=1, partner_shift=0, Lq=c.Lq, Lk=c.Lk, head_dim=E,
                        scale=scale, q_strides=(c.Lq * E, E, E), k_strides=(c.Lk * E, E, E), v_strides=(c.Lk * E, E, E),
                        key_tail=c.tail)
    lam = float(ref["lam"][0].max())
    O, mag = ref["O"][0, :, 0], ref["mag_O"][0, :, 0]                    # (n, Lq, E)
    if bias is not None:
        O, mag = O + bias.double(), mag + bias.double().abs()
    return dict(c=c, dt=dt, scale=scale, q=q, kv=kv, left=left, bias=bias, pi=pi, di=di, n=n, O=O, bound=TAU_O[dt] * mag + 1e-300, lam=lam)


def _out_store(s):
    """A NaN `out` buffer with guard bands: (flat, view (n, Lq, cols) at the case's pitch, mask of the addressed elements)."""
    c = s["c"]
    cols = c.left_cols + E
    n_el = s["n"] * c.Lq * c.pitch
    flat = torch.full((n_el + 2 * G,), float("nan"), device=DEV, dtype=s["dt"])
    mask = torch.zeros(n_el + 2 * G, dtype=torch.bool, device=DEV)
    shape, st = (s["n"], c.Lq, cols), (c.Lq * c.pitch, c.pitch, 1)
    torch.as_strided(mask, shape, st, G).fill_(True)
    return flat, torch.as_strided(flat, shape, st, G), mask


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32).clone()


def _run(s, di=None):
    from druglamp_amd import ops
    c = s["c"]
    flat, out, mask = _out_store(s)
    before = _bits(flat)
    got = ops.pgca_pairs(s["q"][:c.n_q], s["kv"][:c.n_kv], s["pi"], s["di"] if di is None else di, scale=s["scale"],
                         left=None if s["left"] is None else s["left"][:c.n_q], bias=s["bias"], key_tail=c.tail, out=out)
    assert got is out
    torch.cuda.synchronize()
    return flat, out, mask, before


def _check(s, out, pairs=None, tag=""):
    """Worst |err| / bound over the attention columns of `pairs` (all), printed and logged before it is asserted; the left
    columns bitwise."""
    c = s["c"]
    idx = torch.arange(s["n"], device=DEV) if pairs is None else pairs
    got = out[idx][:, :, c.left_cols:].double()
    assert torch.isfinite(got).all(), "%s: non-finite addressed elements" % c.name
    ratio = float(((got - s["O"][idx]).abs() / s["bound"][idx]).max())
    print("pgca_pairs %s%s %s: worst |err| / bound = %.4f (lam %.2f)" % (c.name, tag, str(s["dt"]).split(".")[1], ratio, s["lam"]))
    path = os.environ.get("DL_PGCA_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": c.name + tag, "dtype": str(s["dt"]).split(".")[1], "ratio": ratio}) + "\n")
    assert ratio <= 1.0, "%s: O exceeds its rounding bound by x%.3g" % (c.name, ratio)
    if c.left_cols:
        want = s["left"][s["pi"].long()[idx]]
        assert torch.equal(_bits(out[idx][:, :, :c.left_cols].contiguous()), _bits(want.contiguous())), "%s: left copy differs" % c.name


@pytest.mark.parametrize("name,dt", PARAMS, ids=["%s-%s" % (n, str(d).split(".")[1]) for n, d in PARAMS])
def test_pgca_pairs_against_fp64(name, dt):
    s = _setup(name, dt)
    assert s["lam"] <= LAM, "%s: logits beyond the range the bound assumes" % name
    flat, out, mask, before = _run(s)
    _check(s, out)
    # nothing outside the addressed columns of the addressed rows was written (case c: nothing beyond column 127 of a 136-pitch row)
    assert torch.equal(_bits(flat)[~mask], before[~mask]), "%s: a store outside the addressed elements" % name
    if name == "c_partial_tiles":
        assert torch.isnan(torch.as_strided(flat, (s["n"] * s["c"].Lq, 8), (136, 1), G + 128)).all()


def test_out_of_range_pair_is_skipped_and_flagged():
    """On the allocation of case (a): one pair names drug n_kv exactly — the NaN spare entity, so even a missing guard reads
    inside the allocation.  Its rows stay bitwise unchanged, FLAG_PAIR_INDEX is set, every other pair meets its bound."""
    from druglamp_amd import _lib, ops
    s = _setup("a_compact", BF)
    c = s["c"]
    word = ops.guard_flags(DEV)
    word.zero_()
    bad = 4
    di = s["di"].clone()
    di[bad] = c.n_kv
    try:
        flat, out, mask, before = _run(s, di=di)
        bits = int(word.item())
    finally:
        word.zero_()
    assert bits & _lib.FLAG_PAIR_INDEX and "skipped" in ops.guard_text(bits)
    lo, hi = G + bad * c.Lq * c.pitch, G + (bad + 1) * c.Lq * c.pitch
    assert torch.equal(_bits(flat)[lo:hi], before[lo:hi]), "the skipped pair's rows were written"
    assert torch.equal(_bits(flat)[~mask], before[~mask])
    others = torch.tensor([i for i in range(s["n"]) if i != bad], device=DEV)
    _check(s, out, pairs=others, tag="+guard")
    assert int(word.item()) == 0


def test_two_calls_are_bitwise_identical():
    s = _setup("a_compact", BF)
    a, b = _run(s)[0], _run(s)[0]
    assert torch.equal(_bits(a), _bits(b))


def test_host_tensors_and_a_small_out_are_rejected():
    from druglamp_amd import ops
    s = _setup("c_partial_tiles", BF)
    c = s["c"]
    q, kv = s["q"][:c.n_q], s["kv"][:c.n_kv]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs(q.cpu(), kv, s["pi"], s["di"], scale=s["scale"])
    with pytest.raises(ValueError, match="out must be"):
        ops.pgca_pairs(q, kv, s["pi"], s["di"], scale=s["scale"], out=torch.empty(s["n"], c.Lq - 1, E, device=DEV, dtype=BF))
    with pytest.raises(ValueError, match="out must be"):                 # rows of 120 columns cannot take 128
        ops.pgca_pairs(q, kv, s["pi"], s["di"], scale=s["scale"], out=torch.empty(s["n"], c.Lq, 120, device=DEV, dtype=BF))
