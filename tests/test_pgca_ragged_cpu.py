"""dl_pgca_pairs_ragged_fwd: export, ctypes signature, struct layout and the argument validation that runs before any launch
(status code + dl_last_error() naming the offending field), in the mould of tests/test_pgca_pairs_cpu.py.  None of this needs
a device: the library loads without one."""
import ctypes as C

from druglamp_amd import _lib

OK, ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3, -6
POINTERS = ("Q", "K", "V", "left", "out", "bias", "q_index", "kv_index", "kv_row0", "kv_keys", "kv_tail_weight", "flags")


def _args(buf, **kw):
    """A valid call description (bf16, 2 proteins x 3 drugs in a store of 120 rows, 4 pairs, Lq 16, 128 left columns) pointing
    into `buf`."""
    p16 = (C.addressof(buf) + 15) // 16 * 16
    a = _lib.PgcaPairsRaggedArgs()
    for name in POINTERS:
        setattr(a, name, p16)
    a.q_es, a.q_rs, a.k_rs, a.v_rs = 16 * 128, 128, 256, 256
    a.left_es, a.left_rs, a.out_ps, a.out_rs, a.kv_total_rows = 16 * 128, 128, 16 * 256, 256, 120
    a.n_pairs, a.n_q, a.n_kv, a.Lq, a.head_dim, a.dtype = 4, 2, 3, 16, 128, _lib.DL_BF16
    a.left_cols, a.out_col0, a.scale, a.key_tail_rows = 128, 128, 128 ** -0.5, 8
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbol_is_exported_with_its_signature_and_field_order():
    L = _lib.lib()
    assert "dl_pgca_pairs_ragged_fwd" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["dl_pgca_pairs_ragged_fwd"]
    fn = L.dl_pgca_pairs_ragged_fwd
    assert fn.restype is res and list(fn.argtypes) == list(args) == [C.POINTER(_lib.PgcaPairsRaggedArgs), C.c_void_p]
    assert [f[0] for f in _lib.PgcaPairsRaggedArgs._fields_] == list(POINTERS) + [
        "q_es", "q_rs", "k_rs", "v_rs", "left_es", "left_rs", "out_ps", "out_rs", "kv_total_rows",
        "n_pairs", "n_q", "n_kv", "Lq", "head_dim", "dtype", "left_cols", "out_col0", "scale", "key_tail_rows"]
    # 12 pointers + 9 eight-byte integers + 10 four-byte fields: the C struct's size with no padding inside
    assert C.sizeof(_lib.PgcaPairsRaggedArgs) == 12 * 8 + 9 * 8 + 10 * 4
    assert _lib.FLAG_KEY_TABLE == 32 and _lib.FLAG_PAIR_INDEX == 16
    # the header declares the struct with the same fields in the same order, and the flag's value
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "druglamp_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} dl_pgca_pairs_ragged_args;", hdr).group(1)
    names = [re.findall(r"\w+", piece)[-1] for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    assert names == [f[0] for f in _lib.PgcaPairsRaggedArgs._fields_]
    assert re.search(r"DL_FLAG_KEY_TABLE\s*=\s*32\b", hdr)


def test_null_argument_block_fails_with_a_message():
    L = _lib.lib()
    assert L.dl_pgca_pairs_ragged_fwd(None, None) == ERR_ARG
    assert b"dl_pgca_pairs_ragged_fwd" in L.dl_last_error() and b"null" in L.dl_last_error()


def test_every_rejection_returns_its_code_and_names_the_field():
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    p16 = (C.addressof(buf) + 15) // 16 * 16

    def rc(**kw):
        return L.dl_pgca_pairs_ragged_fwd(C.byref(_args(buf, **kw)), None)

    def err():
        return L.dl_last_error()

    for name in ("Q", "K", "V", "out", "q_index", "kv_index", "kv_row0", "kv_keys", "kv_tail_weight"):
        assert rc(**{name: None}) == ERR_ARG and b"null pointer" in err() and name.encode() in err(), name
    assert rc(dtype=7) == ERR_ARG and b"dtype" in err()
    assert rc(head_dim=64) == ERR_UNSUPPORTED and b"head_dim" in err()
    for name in ("Q", "K", "V", "left", "out", "bias"):
        assert rc(**{name: p16 + 8}) == ERR_ALIGN and b"16-byte" in err(), name
    assert rc(q_index=p16 + 2) == ERR_ALIGN and b"q_index" in err()
    assert rc(kv_row0=p16 + 4) == ERR_ALIGN and b"kv_row0" in err()
    assert rc(kv_keys=p16 + 2) == ERR_ALIGN and b"kv_keys" in err()
    assert rc(kv_tail_weight=p16 + 2) == ERR_ALIGN and b"kv_tail_weight" in err()
    for name in ("q_es", "q_rs", "k_rs", "v_rs", "left_es", "left_rs", "out_ps", "out_rs"):
        assert rc(**{name: 260}) == ERR_ALIGN and name.encode() in err(), name       # 260 bf16 = 520 bytes: no multiple of 16
        assert rc(**{name: -256}) == ERR_ALIGN and name.encode() in err(), name
    assert rc(dtype=_lib.DL_F32, q_rs=130) == ERR_ALIGN and b"q_rs" in err()         # fp32: multiples of 4 elements
    assert rc(left_cols=4, out_col0=128) == ERR_ALIGN and b"left_cols" in err()
    assert rc(out_col0=132) == ERR_ALIGN and b"out_col0" in err()
    assert rc(left_cols=128, out_col0=64) == ERR_ARG and b"overlaps" in err()
    assert rc(left=None) == ERR_ARG and b"left" in err()                             # left_cols > 0 without left
    assert rc(left_cols=0) == ERR_ARG and b"left" in err()                           # left without left_cols
    assert rc(out_rs=248) == ERR_SHAPE and b"out_rs" in err()                        # 128 + 128 columns do not fit
    assert rc(key_tail_rows=-1) == ERR_ARG and b"key_tail_rows" in err()
    assert rc(kv_total_rows=-1) == ERR_SHAPE and b"kv_total_rows" in err()
    assert rc(n_pairs=-1) == ERR_SHAPE and b"negative" in err()
    assert rc(n_q=-1) == ERR_SHAPE and b"negative" in err()
    assert rc(n_kv=-2) == ERR_SHAPE and b"negative" in err()
    assert rc(Lq=0) == ERR_SHAPE and b"Lq" in err()
    assert rc(scale=0.0) == ERR_ARG and b"scale" in err()
    # the workgroup count (n_pairs x ceil(Lq / 128) in bf16) must fit in int32
    assert rc(n_pairs=2 ** 31 - 1, Lq=129) == ERR_SHAPE and b"workgroups" in err()


def test_no_pairs_is_ok_without_a_launch():
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    assert L.dl_pgca_pairs_ragged_fwd(C.byref(_args(buf, n_pairs=0)), None) == OK
    # (no device here: a launch would have failed)
    assert L.dl_pgca_pairs_ragged_fwd(C.byref(_args(buf, n_pairs=0, Q=None, out=None, kv_row0=None)), None) == OK


def test_guard_text_names_the_new_flag():
    from druglamp_amd import ops
    text = ops.guard_text(_lib.FLAG_KEY_TABLE)
    assert "key table" in text and "skipped" in text and "dl_pgca_pairs_ragged_fwd" in text
    both = ops.guard_text(_lib.FLAG_KEY_TABLE | _lib.FLAG_PAIR_INDEX)
    assert "dl_pgca_pairs_fwd" in both and "dl_pgca_pairs_ragged_fwd" in both
