"""The fp64 reference of tests/latent_topk_ref.py against torch.topk and on hand-made tie / NaN rows; the latent's way through
screening.DrugLibrary on CPU tensors (from_codes, append, nbytes, save, load: bit for bit; a latent-free library writes exactly
the keys it wrote before latents existed); and the compact-form token mean.  Nothing here needs a device."""
import numpy as np
import pytest
import torch

from druglamp_amd import screening
from druglamp_amd.screening import DrugBranch, DrugCode, DrugLibrary, ProteinCode
from tests import latent_topk_ref as R

BF, F32 = torch.bfloat16, torch.float32


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_reference_is_torch_topk_on_tie_free_scores(dtype):
    q, lib = R.unit_rows(9, 1, dtype), R.unit_rows(300, 2, dtype)
    s = R.sims64(q, lib)
    assert s.shape == (9, 300)
    assert all(len(np.unique(s[p])) == 300 for p in range(9)), "the draw has ties: torch.topk's order among them is not specified"
    for M in (1, 7, 300):
        v, i = R.topm(s, M)
        tv, ti = torch.topk(torch.from_numpy(s), M, dim=1)
        assert np.array_equal(i, ti.numpy()) and np.array_equal(v, tv.numpy())


def test_reference_orders_ties_by_index_and_puts_nan_first():
    nan = float("nan")
    s = np.array([[1.0, 3.0, 3.0, -2.0, 3.0, 0.0, -0.0, 1.0],
                  [nan, 5.0, nan, 5.0, np.inf, -np.inf, 0.0, 5.0]])
    v, i = R.topm(s, 8)
    assert i[0].tolist() == [1, 2, 4, 0, 7, 5, 6, 3]                  # 3 3 3 | 1 1 | 0 -0 (equal by value: index order) | -2
    assert i[1].tolist() == [0, 2, 4, 1, 3, 7, 6, 5]                  # NaN NaN | inf | 5 5 5 | 0 | -inf
    assert np.isnan(v[1, :2]).all() and v[1, 2] == np.inf and v[1, -1] == -np.inf
    v, i = R.topm(s, 2)                                               # at the cut the lower index wins
    assert i.tolist() == [[1, 2], [0, 2]]
    assert R.topm(s, 4)[1][0].tolist() == [1, 2, 4, 0]


def test_exact_integer_rows_have_exact_scores_and_ties():
    q, lib = R.int_rows(5, 3, BF), R.int_rows(200, 4, BF, distinct=7)
    s = R.sims64(q, lib)
    assert (s == np.round(s)).all() and np.abs(s).max() <= 1024
    assert torch.equal(lib[0], lib[7]) and not torch.equal(lib[0], lib[1])
    _, i = R.topm(s, 60)
    best = np.flatnonzero(s[0] == s[0].max())
    assert i[0][:len(best)].tolist() == best.tolist()                 # the ties of the best value, ascending


# ---- latents in codes and libraries -------------------------------------------------------------------------------------------
def _drug_code(n, seed, dt, latent=True, layout=(136, 8, 48)):
    g = torch.Generator().manual_seed(seed)
    kv = torch.randn(n, layout[0], 256, generator=g).to(dt)
    kv[:, 40:] = kv[:, -1:]                                            # a trailing run of equal rows, as a real drug has
    lat = torch.nn.functional.normalize(torch.randn(n, 256, generator=g), dim=1) if latent else None
    return DrugCode({"v": DrugBranch(kv, torch.randn(128, generator=g), layout)}, dt, 0, latent=lat)


def _tiny_model():
    torch.manual_seed(3)
    return torch.nn.Linear(4, 4)


def test_codes_carry_latents_and_cat_concatenates_them():
    a, b = _drug_code(2, 1, F32), _drug_code(3, 2, F32)
    cat = DrugCode.cat([a, b])
    assert cat.n == 5 and torch.equal(cat.latent, torch.cat([a.latent, b.latent]))
    assert DrugCode.cat([_drug_code(2, 1, F32, latent=False), _drug_code(3, 2, F32, latent=False)]).latent is None
    with pytest.raises(ValueError):
        DrugCode.cat([a, _drug_code(3, 2, F32, latent=False)])
    # positional meaning unchanged, latent keyword-only
    assert DrugCode(a.branches, F32, 0).latent is None and ProteinCode({}, F32, 0).latent is None
    with pytest.raises(TypeError):
        DrugCode(a.branches, F32, 0, a.latent)
    sites = torch.zeros(2, 4, 128)
    p = ProteinCode.cat([ProteinCode({"v": (sites, sites)}, F32, 0, latent=a.latent), ProteinCode({"v": (sites, sites)}, F32, 0, latent=a.latent)])
    assert p.n == 4 and torch.equal(p.latent, torch.cat([a.latent, a.latent]))


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
def test_library_carries_latents_bit_for_bit(dt, tmp_path):
    a, b, c = _drug_code(2, 1, dt), _drug_code(3, 2, dt), _drug_code(2, 3, dt)
    model = _tiny_model()
    lib = DrugLibrary.from_codes([a, b], model)
    want = torch.cat([a.latent, b.latent]).to(dt)                      # rounded once, at build
    assert lib.latent.dtype == dt and lib.latent.shape == (5, 256) and torch.equal(lib.latent, want)
    bare = DrugLibrary.from_codes([_drug_code(2, 1, dt, latent=False), _drug_code(3, 2, dt, latent=False)], model)
    assert bare.latent is None and lib.nbytes == bare.nbytes + 5 * 256 * want.element_size()
    lib.append(c)
    want = torch.cat([want, c.latent.to(dt)])
    assert lib.n == 7 and torch.equal(lib.latent, want)
    with pytest.raises(ValueError):
        lib.append(_drug_code(2, 3, dt, latent=False))
    with pytest.raises(ValueError):
        bare.append(c)
    with pytest.raises(ValueError):
        DrugLibrary.from_codes([a, _drug_code(3, 2, dt, latent=False)])
    path = tmp_path / "lib.pt"
    lib.save(path)
    back = DrugLibrary.load(path, model, "cpu")
    assert back.latent.dtype == dt and torch.equal(back.latent.view(torch.uint8), want.view(torch.uint8))
    assert torch.equal(back.branches["v"].rows, lib.branches["v"].rows) and back.nbytes == lib.nbytes
    assert set(torch.load(path, weights_only=True)) - {"latent"} == set(_blob_keys(bare, tmp_path))


def _blob_keys(lib, tmp_path):
    path = tmp_path / "bare.pt"
    lib.save(path)
    return list(torch.load(path, weights_only=True))


def test_a_latent_free_library_writes_exactly_the_keys_of_before(tmp_path):
    model = _tiny_model()
    bare = DrugLibrary.from_codes([_drug_code(2, 1, F32, latent=False)], model)
    keys = _blob_keys(bare, tmp_path)
    assert sorted(keys) == sorted(["format", "dtype", "fingerprint", "branches", "v.rows", "v.row0", "v.n_keys", "v.tail_weight", "v.bias"])
    back = DrugLibrary.load(tmp_path / "bare.pt", model, "cpu")
    assert back.latent is None and back.n == 2


# ---- the token mean of a compact form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead,w", [(128, 48), (64, 56), (8, 63)])
def test_compact_token_mean_is_the_mean_over_the_expanded_rows(lead, w):
    g = torch.Generator().manual_seed(lead)
    y = torch.randn(3, lead + 8, 128, generator=g)
    idx = torch.cat([torch.arange(lead), lead + torch.arange(8 * w) % 8])          # DrugBranch.full()'s order
    full = y.index_select(1, idx)
    assert full.shape[1] == lead + 8 * w == 512
    got = screening.token_mean(full, (y, w))
    assert got.dtype == torch.float32 and got.shape == (3, 128)
    assert float((got - full.mean(dim=1)).abs().max()) <= 1e-6
    assert float((got - full.double().mean(dim=1).float()).abs().max()) <= 1e-6
    assert torch.equal(screening.token_mean(full), full.float().mean(dim=1))
    assert screening.token_mean(full.bfloat16(), (y.bfloat16(), w)).dtype == torch.float32
