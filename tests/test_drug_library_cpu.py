"""screening.DrugLibrary on CPU tensors: the per-drug trimming rule, the packed layout, expand, save / load and the parameter
fingerprint.  Hand-built DrugCodes; nothing here needs a device (the library's layout logic is plain torch ops).

Layouts (Lk, 8, 47) and (Lk, 8, 55) stand for (Lk - 8) + 8 * 47 or 55 = 504 keys, the model's (136, 8, 48) and a 512-row code
for 512: what every drug must satisfy is  n_keys - 8 + 8 * tail_weight == the number of keys its code stood for, and that is
asserted with the number written out per case (512 wherever the code stood for 512 keys)."""
import functools

import pytest
import torch

from druglamp_amd.screening import DrugBranch, DrugCode, DrugLibrary

BF, F32 = torch.bfloat16, torch.float32
DTYPES = [BF, F32]
IDS = ["bf16", "fp32"]


def _rows(n, seed, dt):
    """n <= 512 pairwise distinct random rows of 256 (the first column is made strictly increasing)."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(n, 256, generator=g)
    r[:, 0] = torch.arange(n, dtype=torch.float32) - 256.0                # integers of at most 8 bits: exact in bf16, distinct
    return r.to(dt)


def _drug(Lk, real, seed, dt, pad_value=0.5):
    """(Lk, 256): `real` distinct rows, then copies of one padding row."""
    kv = torch.full((Lk, 256), pad_value).to(dt)
    kv[:, 0] = 1024.0                                                       # (differs from every real row's first column)
    kv[:real] = _rows(real, seed, dt)
    return kv


def _code(kvs, layout, dt, bias_seed=99):
    g = torch.Generator().manual_seed(bias_seed)
    bias = torch.randn(128, generator=g)
    return DrugCode({"v": DrugBranch(torch.stack(kvs), bias, layout)}, dt, 0)


@functools.lru_cache(maxsize=None)
def _cases(dt):
    """[(name, code, expected [(n_keys, tail_weight, keys stood for)] per drug)]"""
    out = []
    # 1. compact layout, real rows ending at 20 and 33
    out.append(("compact_136", _code([_drug(136, 20, 1, dt), _drug(136, 33, 2, dt)], (136, 8, 47), dt), [(32, 60, 504), (48, 58, 504)]))
    # 2. all 64 lead rows distinct: unchanged
    out.append(("compact_72_whole", _code([_drug(72, 64, 3, dt)], (72, 8, 55), dt), [(72, 55, 504)]))
    # 3. full 512-row code, no tail: trailing equal rows from row 41; and a drug with no two rows equal
    out.append(("full_512", _code([_drug(512, 41, 4, dt), _rows(512, 5, dt)], (512, 0, 1), dt), [(56, 58, 512), (512, 1, 512)]))
    # 4. the 8 tail rows are not all equal: kept whole with its own weight
    kv = _drug(136, 20, 6, dt)
    kv[130, 5] = 9.0
    out.append(("tail_not_equal", _code([kv], (136, 8, 48), dt), [(136, 48, 512)]))
    # 5. padding row with -0.0 that meets +0.0 in the in-block copies: equal by value, trimmed
    kv = _drug(136, 20, 7, dt, pad_value=-0.0)
    kv[20:128, 1:] = 0.0                                                    # the in-block copies carry +0.0
    assert torch.signbit(kv[135, 1]) and not torch.signbit(kv[50, 1])
    out.append(("signed_zero", _code([kv], (136, 8, 48), dt), [(32, 61, 512)]))
    # 6. a NaN padding row never compares equal: not trimmed (with and without a tail)
    kv = _drug(136, 20, 8, dt)
    kv[20:, 3] = float("nan")
    out.append(("nan_tail", _code([kv], (136, 8, 48), dt), [(136, 48, 512)]))
    kv = _drug(512, 41, 9, dt)
    kv[41:, 3] = float("nan")
    out.append(("nan_full", _code([kv], (512, 0, 1), dt), [(512, 1, 512)]))
    # the model's own layout, real rows ending on a multiple of 8 and one short of it
    out.append(("model_136", _code([_drug(136, 24, 10, dt), _drug(136, 23, 11, dt), _drug(136, 128, 12, dt)], (136, 8, 48), dt),
                [(32, 61, 512), (32, 61, 512), (136, 48, 512)]))
    return out


def _same_values(a, b):
    """Equal by value, NaN at the same places (-0.0 == +0.0: the rule is stated by value)."""
    a, b = a.double(), b.double()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_every_case_alone_trims_as_the_rule_says(dt):
    for name, code, want in _cases(dt):
        lib = DrugLibrary.from_codes([code])
        b = lib.branches["v"]
        assert lib.n == len(want) == code.n, name
        assert b.rows.dtype == dt and b.row0.dtype == torch.int64 and b.n_keys.dtype == torch.int32 and b.tail_weight.dtype == F32
        assert lib.keys("v").tolist() == [w[0] for w in want], name
        assert b.tail_weight.tolist() == [float(w[1]) for w in want], name
        full = code.branches["v"].full()
        for i, (nk, w, stood) in enumerate(want):
            assert nk - 8 + 8 * w == stood == full.kv.shape[1], (name, i)
            assert _same_values(lib.expand("v", i), full.kv[i]), (name, i)
        assert b.rows.shape == (sum(w[0] for w in want), 256), name
        assert b.row0.tolist() == [sum(w[0] for w in want[:i]) for i in range(len(want))], name
        assert torch.equal(b.bias, code.branches["v"].bias)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_mixed_layouts_pack_into_one_store_without_the_512_key_expansion(dt):
    cases = _cases(dt)
    codes = [c for _, c, _ in cases]
    want = [w for _, _, ws in cases for w in ws]
    lib = DrugLibrary.from_codes(codes)
    b = lib.branches["v"]
    assert lib.n == len(want) == 12
    assert lib.keys("v").tolist() == [w[0] for w in want]
    assert b.rows.shape[0] == int(lib.keys("v").sum()) == sum(w[0] for w in want) < lib.n * 504
    assert b.row0.tolist() == [sum(w[0] for w in want[:i]) for i in range(len(want))]
    assert lib.nbytes == sum(t.numel() * t.element_size() for t in (b.rows, b.row0, b.n_keys, b.tail_weight, b.bias))
    i = 0
    for _, code, ws in cases:
        full = code.branches["v"].full()
        for j in range(len(ws)):
            assert _same_values(lib.expand("v", i), full.kv[j]), i
            i += 1
    # append gives the library from_codes gives
    inc = DrugLibrary.from_codes(codes[:1])
    for c in codes[1:]:
        assert inc.append(c) is inc
    for f in ("rows", "row0", "n_keys", "tail_weight"):
        x, y = getattr(inc.branches["v"], f), getattr(b, f)
        assert x.dtype == y.dtype and _same_values(x, y), f
    # codes of another dtype, epoch or branch set are refused
    other = cases[0][1]
    with pytest.raises(ValueError):
        lib.append(DrugCode(other.branches, other.dtype, other.epoch + 1))
    with pytest.raises(ValueError):
        DrugLibrary.from_codes([other, DrugCode({"v": other.branches["v"], "x": other.branches["v"]}, other.dtype, other.epoch)])
    with pytest.raises(ValueError):
        DrugLibrary.from_codes([])


class _Standin(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.lin = torch.nn.Linear(4, 3)
        self.bn = torch.nn.BatchNorm1d(3)          # (a 0-dim integer buffer in the state_dict)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_save_then_load_is_bitwise_equal_and_checks_the_parameters(dt, tmp_path):
    model = _Standin()
    codes = [c for _, c, _ in _cases(dt)]
    with pytest.raises(RuntimeError, match="fingerprint"):
        DrugLibrary.from_codes(codes).save(tmp_path / "nofp.pt")
    lib = DrugLibrary.from_codes(codes, model)
    path = tmp_path / "lib.pt"
    lib.save(path)
    back = DrugLibrary.load(path, model, "cpu")
    assert back.dtype == dt and back.fingerprint == lib.fingerprint and back.n == lib.n and set(back.branches) == {"v"}
    from druglamp_amd.screening import param_epoch
    assert back.epoch == param_epoch()
    bits = torch.int16 if dt == BF else torch.int32
    a, b = lib.branches["v"], back.branches["v"]
    assert torch.equal(a.rows.view(bits), b.rows.view(bits))                 # bitwise: NaN and signed zeros included
    assert torch.equal(a.row0, b.row0) and torch.equal(a.n_keys, b.n_keys)
    assert torch.equal(a.tail_weight.view(torch.int32), b.tail_weight.view(torch.int32)) and torch.equal(a.bias, b.bias)
    assert b.row0.dtype == torch.int64 and b.n_keys.dtype == torch.int32 and b.tail_weight.dtype == F32
    # one changed parameter (by one ulp), or one changed buffer: the file is refused
    with torch.no_grad():
        w = model.lin.weight
        w[1, 2] = torch.nextafter(w[1, 2], torch.tensor(10.0))
    with pytest.raises(RuntimeError, match="other parameters"):
        DrugLibrary.load(path, model, "cpu")
    model2 = _Standin()
    assert DrugLibrary.load(path, model2, "cpu").n == lib.n
    model2.bn.num_batches_tracked += 1
    with pytest.raises(RuntimeError, match="other parameters"):
        DrugLibrary.load(path, model2, "cpu")
