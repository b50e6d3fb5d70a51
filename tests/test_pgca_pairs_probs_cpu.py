"""dl_pgca_pairs_probs / dl_pgca_pairs_ragged_probs: export, ctypes signature, struct layout and the argument validation that
runs before any launch (status code + dl_last_error() naming the offending field), in the mould of tests/test_pgca_ragged_cpu.py;
the wrappers' host-side refusals.  None of this needs a device: the library loads without one."""
import ctypes as C
import os
import re

import pytest
import torch

from druglamp_amd import _lib

OK, ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3, -6
DENSE_PTRS = ("Q", "K", "out", "q_index", "kv_index", "flags")
RAGGED_PTRS = ("Q", "K", "out", "q_index", "kv_index", "kv_row0", "kv_keys", "kv_tail_weight", "flags")
ENTRY = {"dense": ("dl_pgca_pairs_probs", _lib.PgcaPairsProbsArgs, DENSE_PTRS),
         "ragged": ("dl_pgca_pairs_ragged_probs", _lib.PgcaPairsRaggedProbsArgs, RAGGED_PTRS)}


def _args(form, buf, **kw):
    """A valid call description (bf16, 2 proteins x 3 drugs of 40 keys whose last 8 stand for 3 each, 4 pairs, Lq 16, expanded
    maps of 56 columns in rows of 64) pointing into `buf`."""
    _, cls, ptrs = ENTRY[form]
    p16 = (C.addressof(buf) + 15) // 16 * 16
    a = cls()
    for name in ptrs:
        setattr(a, name, p16)
    a.q_es, a.q_rs, a.k_rs, a.out_ps, a.out_rs = 16 * 128, 128, 256, 16 * 64, 64
    a.n_pairs, a.n_q, a.n_kv, a.Lq, a.head_dim, a.dtype = 4, 2, 3, 16, 128, _lib.DL_BF16
    a.out_cols, a.expand_tail, a.scale, a.key_tail_rows = 56, 1, 128 ** -0.5, 8
    if form == "dense":
        a.k_es, a.Lk, a.key_tail_weight = 40 * 256, 40, 3.0
    else:
        a.kv_total_rows = 120
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _caller(form):
    L = _lib.lib()
    fn = getattr(L, ENTRY[form][0])
    buf = (C.c_char * 4096)()
    p16 = (C.addressof(buf) + 15) // 16 * 16
    return (lambda **kw: fn(C.byref(_args(form, buf, **kw)), None)), L.dl_last_error, p16


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_symbols_are_exported_with_their_signatures_and_field_order(form):
    L = _lib.lib()
    name, cls, ptrs = ENTRY[form]
    res, args = _lib.SIGNATURES[name]
    fn = getattr(L, name)
    assert fn.restype is res and list(fn.argtypes) == list(args) == [C.POINTER(cls), C.c_void_p]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "druglamp_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} %s_args;" % name, hdr).group(1)
    names = [re.findall(r"\w+", piece)[-1] for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    assert names == [f[0] for f in cls._fields_] and names[:len(ptrs)] == list(ptrs)
    # dense: 6 pointers + 6 eight-byte strides + 12 four-byte fields; ragged: 9 + 6 + 10 — no padding inside
    assert C.sizeof(cls) == ((6 + 6) * 8 + 12 * 4 if form == "dense" else (9 + 6) * 8 + 10 * 4)
    assert _lib.FLAG_MAP_COLS == 64 and re.search(r"DL_FLAG_MAP_COLS\s*=\s*64\b", hdr)


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_null_argument_block_fails_with_a_message(form):
    L = _lib.lib()
    name = ENTRY[form][0]
    assert getattr(L, name)(None, None) == ERR_ARG
    assert name.encode() in L.dl_last_error() and b"null argument block" in L.dl_last_error()


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_every_rejection_returns_its_code_and_names_the_field(form):
    rc, err, p16 = _caller(form)
    for name in ENTRY[form][2][:-1]:
        assert rc(**{name: None}) == ERR_ARG and b"null pointer" in err() and name.encode() in err(), name
    assert rc(dtype=7) == ERR_ARG and b"dtype" in err()
    assert rc(head_dim=64) == ERR_UNSUPPORTED and b"head_dim" in err()
    assert rc(out_cols=0) == ERR_SHAPE and b"out_cols" in err()
    assert rc(out_cols=-8) == ERR_SHAPE and b"out_cols" in err()
    assert rc(out_rs=48) == ERR_SHAPE and b"out_rs" in err() and b"out_cols" in err()   # rows of 48 cannot take 56 columns
    assert rc(out_ps=-64) == ERR_SHAPE and b"out_ps" in err()
    assert rc(out=p16 + 2) == ERR_ALIGN and b"out not 4-byte" in err()
    assert rc(expand_tail=2) == ERR_ARG and b"expand_tail" in err()
    assert rc(expand_tail=-1) == ERR_ARG and b"expand_tail" in err()
    for name in ("Q", "K"):
        assert rc(**{name: p16 + 8}) == ERR_ALIGN and b"16-byte" in err(), name
    assert rc(q_index=p16 + 2) == ERR_ALIGN and b"q_index" in err()
    for name in ("q_es", "q_rs", "k_rs") + (("k_es",) if form == "dense" else ()):
        assert rc(**{name: 260}) == ERR_ALIGN and name.encode() in err(), name       # 260 bf16 = 520 bytes: no multiple of 16
        assert rc(**{name: -256}) == ERR_ALIGN and name.encode() in err(), name
    assert rc(dtype=_lib.DL_F32, q_rs=130) == ERR_ALIGN and b"q_rs" in err()         # fp32: multiples of 4 elements
    assert rc(key_tail_rows=-1) == ERR_ARG and b"key_tail_rows" in err()
    assert rc(n_pairs=-1) == ERR_SHAPE and b"negative" in err()
    assert rc(n_kv=-2) == ERR_SHAPE and b"negative" in err()
    assert rc(Lq=0) == ERR_SHAPE and b"Lq" in err()
    assert rc(scale=0.0) == ERR_ARG and b"scale" in err()
    assert rc(n_pairs=2 ** 31 - 1, Lq=129) == ERR_SHAPE and b"workgroups" in err()
    if form == "ragged":
        assert rc(kv_row0=p16 + 4) == ERR_ALIGN and b"kv_row0" in err()
        assert rc(kv_keys=p16 + 2) == ERR_ALIGN and b"kv_keys" in err()
        assert rc(kv_total_rows=-1) == ERR_SHAPE and b"kv_total_rows" in err()
    else:
        # the dense column count is known on the host: 32 + 8 * 3 = 56 expanded, 40 unexpanded
        assert rc(out_cols=55) == ERR_SHAPE and b"56 columns" in err() and b"out_cols" in err()
        assert rc(out_cols=39, expand_tail=0) == ERR_SHAPE and b"40 columns" in err()
        assert rc(key_tail_weight=2.5) == ERR_ARG and b"whole key_tail_weight" in err()
        assert rc(key_tail_weight=2.0 ** 25, out_cols=2 ** 30, out_rs=2 ** 30) == ERR_ARG and b"whole key_tail_weight" in err()
        assert rc(key_tail_weight=0.5) == ERR_ARG and b"below 1" in err()
        assert rc(key_tail_rows=41) == ERR_ARG and b"key_tail_rows" in err()
        assert rc(Lk=0) == ERR_SHAPE and b"Lk" in err()


@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_no_pairs_is_ok_without_a_launch(form):
    rc, _, _ = _caller(form)
    assert rc(n_pairs=0) == OK                                                       # (no device here: a launch would have failed)
    assert rc(n_pairs=0, **{name: None for name in ENTRY[form][2]}) == OK


def test_guard_text_names_the_new_flag():
    from druglamp_amd import ops
    text = ops.guard_text(_lib.FLAG_MAP_COLS)
    assert "does not fit" in text and "whole number" in text and "skipped" in text and "dl_pgca_pairs_probs" in text
    assert ops.guard_text(_lib.FLAG_KEY_TABLE | _lib.FLAG_PAIR_INDEX | _lib.FLAG_MAP_COLS).count("skipped") == 3


def test_wrappers_refuse_host_tensors_and_wrong_table_dtypes():
    """_need_gpu runs first, so without a device the table-dtype refusals are exercised through the helper the wrapper shares
    with pgca_pairs_ragged (tests/test_pgca_pairs_probs_gpu.py sends them through the wrapper itself)."""
    from druglamp_amd import ops
    q = torch.zeros(2, 16, 128, dtype=torch.bfloat16)
    kv = torch.zeros(3, 40, 256, dtype=torch.bfloat16)
    pi = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_probs(q, kv, pi, pi, scale=0.1, key_tail=(8, 3.0), expand_tail=True)
    row0, n_keys, w = torch.arange(3) * 40, torch.full((3,), 40, dtype=torch.int32), torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pgca_pairs_ragged_probs(q, kv.view(120, 256), row0, n_keys, w, pi, pi, scale=0.1, key_tail_rows=8, cols=64)
    for bad in ((row0.int(), n_keys, w), (row0, n_keys.long(), w), (row0, n_keys, w.double()), (row0, n_keys[:2], w)):
        with pytest.raises(ValueError, match="pgca_pairs_ragged_probs: the key table"):
            ops._check_key_table("pgca_pairs_ragged_probs", q, *bad)
    ops._check_key_table("pgca_pairs_ragged_probs", q, row0, n_keys, w)
