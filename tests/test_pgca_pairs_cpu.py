"""dl_pgca_pairs_fwd: export, ctypes signature, struct layout and the argument validation that runs before any launch (status
code + dl_last_error() naming the offending field).  None of this needs a device: the library loads without one."""
import ctypes as C

from druglamp_amd import _lib

OK, ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3, -6


def _args(buf, **kw):
    """A valid call description (bf16, 2 proteins x 3 drugs, 4 pairs, Lq 16, Lk 40, 128 left columns) pointing into `buf`."""
    p16 = (C.addressof(buf) + 15) // 16 * 16
    a = _lib.PgcaPairsArgs()
    a.Q = a.K = a.V = a.left = a.out = a.bias = a.q_index = a.kv_index = a.flags = p16
    a.q_es, a.q_rs, a.k_es, a.k_rs, a.v_es, a.v_rs = 16 * 128, 128, 40 * 256, 256, 40 * 256, 256
    a.left_es, a.left_rs, a.out_ps, a.out_rs = 16 * 128, 128, 16 * 256, 256
    a.n_pairs, a.n_q, a.n_kv, a.Lq, a.Lk, a.head_dim, a.dtype = 4, 2, 3, 16, 40, 128, _lib.DL_BF16
    a.left_cols, a.out_col0, a.scale = 128, 128, 128 ** -0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbol_is_exported_with_its_signature_and_field_order():
    L = _lib.lib()
    assert "dl_pgca_pairs_fwd" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["dl_pgca_pairs_fwd"]
    fn = L.dl_pgca_pairs_fwd
    assert fn.restype is res and list(fn.argtypes) == list(args) == [C.POINTER(_lib.PgcaPairsArgs), C.c_void_p]
    assert [f[0] for f in _lib.PgcaPairsArgs._fields_] == [
        "Q", "K", "V", "left", "out", "bias", "q_index", "kv_index", "flags",
        "q_es", "q_rs", "k_es", "k_rs", "v_es", "v_rs", "left_es", "left_rs", "out_ps", "out_rs",
        "n_pairs", "n_q", "n_kv", "Lq", "Lk", "head_dim", "dtype", "left_cols", "out_col0", "scale",
        "key_tail_rows", "key_tail_weight"]
    # 9 pointers + 10 strides + 12 four-byte fields: the C struct's size with no padding inside
    assert C.sizeof(_lib.PgcaPairsArgs) == 9 * 8 + 10 * 8 + 12 * 4
    assert _lib.FLAG_PAIR_INDEX == 16


def test_null_argument_block_fails_with_a_message():
    L = _lib.lib()
    assert L.dl_pgca_pairs_fwd(None, None) == ERR_ARG
    assert b"dl_pgca_pairs_fwd" in L.dl_last_error() and b"null" in L.dl_last_error()


def test_every_rejection_returns_its_code_and_names_the_field():
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    p16 = (C.addressof(buf) + 15) // 16 * 16

    def rc(**kw):
        return L.dl_pgca_pairs_fwd(C.byref(_args(buf, **kw)), None)

    def err():
        return L.dl_last_error()

    for name in ("Q", "K", "V", "out", "q_index", "kv_index"):
        assert rc(**{name: None}) == ERR_ARG and b"null pointer" in err(), name
    assert rc(dtype=7) == ERR_ARG and b"dtype" in err()
    assert rc(head_dim=64) == ERR_UNSUPPORTED and b"head_dim" in err()
    for name in ("Q", "K", "V", "left", "out", "bias"):
        assert rc(**{name: p16 + 8}) == ERR_ALIGN and b"16-byte" in err(), name
    assert rc(q_index=p16 + 2) == ERR_ALIGN and b"q_index" in err()
    for name in ("q_es", "q_rs", "k_es", "k_rs", "v_es", "v_rs", "left_es", "left_rs", "out_ps", "out_rs"):
        assert rc(**{name: 260}) == ERR_ALIGN and name.encode() in err(), name       # 260 bf16 = 520 bytes: no multiple of 16
    assert rc(dtype=_lib.DL_F32, q_rs=130) == ERR_ALIGN and b"q_rs" in err()         # fp32: multiples of 4 elements
    assert rc(left_cols=4, out_col0=128) == ERR_ALIGN and b"left_cols" in err()
    assert rc(out_col0=132) == ERR_ALIGN and b"out_col0" in err()
    assert rc(left_cols=128, out_col0=64) == ERR_ARG and b"overlaps" in err()
    assert rc(left=None) == ERR_ARG and b"left" in err()                             # left_cols > 0 without left
    assert rc(left_cols=0) == ERR_ARG and b"left" in err()                           # left without left_cols
    assert rc(out_rs=248) == ERR_SHAPE and b"out_rs" in err()                        # 128 + 128 columns do not fit
    assert rc(key_tail_rows=41, key_tail_weight=2.0) == ERR_ARG and b"key_tail_rows" in err()
    assert rc(key_tail_rows=8, key_tail_weight=0.5) == ERR_ARG and b"key_tail_weight" in err()
    assert rc(n_pairs=-1) == ERR_SHAPE and b"negative" in err()
    assert rc(n_q=-1) == ERR_SHAPE and b"negative" in err()
    assert rc(n_kv=-2) == ERR_SHAPE and b"negative" in err()
    assert rc(Lq=0) == ERR_SHAPE and b"Lq" in err()
    assert rc(scale=0.0) == ERR_ARG and b"scale" in err()


def test_no_pairs_is_ok_without_a_launch():
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    assert L.dl_pgca_pairs_fwd(C.byref(_args(buf, n_pairs=0)), None) == OK
    # (no device here: a launch would have failed)
    assert L.dl_pgca_pairs_fwd(C.byref(_args(buf, n_pairs=0, Q=None, out=None)), None) == OK
