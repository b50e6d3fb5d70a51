"""dl_attn_probs / dl_attn_probs_workspace_bytes: export, ctypes signatures and the argument validation that runs before any
launch (status code + dl_last_error()).  None of this needs a device: the library loads without one."""
import ctypes as C

from druglamp_amd import _lib

OK, ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -6


def _args(buf, **kw):
    """A valid call description (bf16, head_dim 64, 2 problems x 2 heads, Lq 16, Lk 40) pointing into `buf`."""
    p16 = (C.addressof(buf) + 15) // 16 * 16
    a = _lib.AttnProbsArgs()
    a.Q = a.K = a.LSE = a.out = p16
    a.n_problems, a.n_heads, a.n_segments, a.partner_shift = 2, 2, 1, 0
    a.Lq, a.Lk, a.head_dim, a.dtype = 16, 40, 64, _lib.DL_BF16
    a.q_ps, a.q_hs, a.q_rs = 16 * 128, 64, 128
    a.k_ps, a.k_hs, a.k_rs = 40 * 128, 64, 128
    a.scale, a.out_ld = 0.125, 40
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_are_exported_with_signatures():
    L = _lib.lib()
    for name in ("dl_attn_probs", "dl_attn_probs_workspace_bytes"):
        assert name in _lib.SIGNATURES
        fn = getattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert [f[0] for f in _lib.AttnProbsArgs._fields_][:5] == ["Q", "K", "LSE", "out", "out_ld"]
    assert [f[0] for f in _lib.AttnProbsArgs._fields_][-6:] == ["head_mean", "key_tail_rows", "key_tail_weight", "expand_tail",
                                                                "workspace", "workspace_bytes"]


def test_null_argument_block_fails_with_a_message():
    L = _lib.lib()
    assert L.dl_attn_probs(None, None) == ERR_ARG
    assert b"dl_attn_probs" in L.dl_last_error() and b"null" in L.dl_last_error()
    assert L.dl_attn_probs_workspace_bytes(None) == 0


def test_every_rejection_returns_its_code_before_any_launch():
    L = _lib.lib()
    buf = (C.c_char * 4096)()

    def rc(**kw):
        return L.dl_attn_probs(C.byref(_args(buf, **kw)), None)

    assert rc(head_dim=32) == ERR_UNSUPPORTED and b"head_dim" in L.dl_last_error()
    assert rc(n_segments=2, partner_shift=1, key_tail_rows=8, key_tail_weight=3.0) == ERR_UNSUPPORTED
    assert b"one segment only" in L.dl_last_error()
    assert rc(key_tail_rows=8, key_tail_weight=2.5, expand_tail=1, out_ld=4096) == ERR_ARG and b"whole" in L.dl_last_error()
    assert rc(out_ld=39) == ERR_SHAPE and b"out_ld" in L.dl_last_error()
    # expanded: 32 + 8 * 3 = 56 columns
    assert rc(key_tail_rows=8, key_tail_weight=3.0, expand_tail=1, out_ld=55) == ERR_SHAPE and b"56" in L.dl_last_error()
    need = 4 * 1 * 2 * 2 * 16
    assert rc(LSE=None, workspace=C.addressof(buf), workspace_bytes=need - 1) == ERR_WORKSPACE and b"workspace" in L.dl_last_error()
    assert rc(LSE=None, workspace=None, workspace_bytes=need) == ERR_WORKSPACE
    assert rc(key_tail_rows=41, key_tail_weight=2.0) == ERR_ARG and b"key_tail_rows" in L.dl_last_error()
    assert rc(key_tail_rows=8, key_tail_weight=0.5) == ERR_ARG
    assert rc(q_rs=3) == ERR_ALIGN
    assert rc(Q=(C.addressof(buf) + 15) // 16 * 16 + 2) == ERR_ALIGN
    assert rc(out=None) == ERR_ARG
    assert rc(dtype=7) == ERR_ARG
    assert rc(head_mean=2) == ERR_ARG


def test_workspace_bytes_is_four_bytes_per_statistic():
    L = _lib.lib()
    buf = (C.c_char * 64)()
    for S, P, H, Lq in ((1, 2, 2, 16), (2, 3, 4, 65), (1, 256, 1, 256), (2, 512, 4, 256)):
        a = _args(buf, n_segments=S, n_problems=P, n_heads=H, Lq=Lq)
        assert L.dl_attn_probs_workspace_bytes(C.byref(a)) == 4 * S * P * H * Lq
