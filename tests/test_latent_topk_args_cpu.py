"""dl_latent_topk: the argument validation that runs before any launch (status code + dl_last_error() naming the entry) and
dl_latent_topk_workspace_bytes against the candidate-buffer rule.  None of this needs a device: the library loads without one,
and every call below is rejected before its first launch (in the style of tests/test_bn_args_cpu.py)."""
import ctypes as C

import pytest

from druglamp_amd import _lib

ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_WORKSPACE = -1, -2, -3, -4
ENTRY = "dl_latent_topk"
PARAMS = "q lib P D M dtype slab values indices stream ws ws_bytes".split()
PTRS = ("q", "lib", "values", "indices", "ws")
_buf = (C.c_char * 4096)()
_p16 = (C.addressof(_buf) + 15) // 16 * 16


def call(**kw):
    """dl_latent_topk with a valid argument list (bf16, P 70, D 1000, M 100, distinct 16-byte aligned pointers, a workspace of
    exactly dl_latent_topk_workspace_bytes) changed by `kw`: (status, dl_last_error()).  Valid as it stands, it would launch:
    every test changes at least one argument into one that is rejected first."""
    L = _lib.lib()
    a = dict(P=70, D=1000, M=100, dtype=_lib.DL_BF16, slab=0, stream=None)
    a.update({p: _p16 + 64 * i for i, p in enumerate(PTRS)})
    a.update(kw)
    a.setdefault("ws_bytes", L.dl_latent_topk_workspace_bytes(a["P"], a["D"], a["M"], a["slab"]))
    rc = getattr(L, ENTRY)(*[a[p] for p in PARAMS])
    return rc, L.dl_last_error()


def rejected(code, **kw):
    rc, err = call(**kw)
    return rc == code and (ENTRY + ":").encode() in err


def test_the_entry_points_are_exported_with_their_signatures():
    L = _lib.lib()
    res, args = _lib.SIGNATURES[ENTRY]
    assert getattr(L, ENTRY).restype is res is _lib.c_i32 and len(args) == len(PARAMS)
    res, args = _lib.SIGNATURES["dl_latent_topk_workspace_bytes"]
    assert L.dl_latent_topk_workspace_bytes.restype is res is _lib.c_sz and len(args) == 4


def test_null_and_misaligned_pointers():
    for p in ("q", "lib", "values", "indices"):
        assert rejected(ERR_ARG, **{p: None}), p
    for p in ("q", "lib"):
        for off in (2, 4, 8):
            assert rejected(ERR_ALIGN, **{p: _p16 + 256 + off}), (p, off)
    for p in ("values", "indices"):
        assert rejected(ERR_ALIGN, **{p: _p16 + 256 + 2}), p


def test_shape_limits():
    assert rejected(ERR_ARG, M=0) and rejected(ERR_ARG, M=-1)
    assert rejected(ERR_ARG, M=1001)                               # M > D
    assert rejected(ERR_ARG, M=1025, D=5000)                       # M > 1024
    assert rejected(ERR_ARG, P=0) and rejected(ERR_ARG, P=-3)
    assert rejected(ERR_SHAPE, D=0) and rejected(ERR_SHAPE, D=1 << 31)
    rc, err = call(M=1025, D=5000)
    assert b"min(D, 1024)" in err
    # the largest library passes the shape checks and gets as far as the workspace check
    assert rejected(ERR_WORKSPACE, D=(1 << 31) - 1, ws_bytes=0)


def test_bad_dtype_and_slab():
    rc, err = call(dtype=7)
    assert rc == ERR_ARG and b"dl_latent_topk: bad dtype" in err
    for slab in (-64, 1, 63, 100):
        rc, err = call(slab=slab, ws_bytes=1 << 30)
        assert rc == ERR_ARG and b"dl_latent_topk: slab" in err, slab


def test_workspace_null_misaligned_or_one_byte_short():
    L = _lib.lib()
    for P, D, M, slab in ((70, 1000, 100, 0), (1, 64, 1, 0), (65, 1000, 1000, 64), (1024, 1 << 20, 1024, 0)):
        need = L.dl_latent_topk_workspace_bytes(P, D, M, slab)
        assert need > 0
        rc, err = call(P=P, D=D, M=M, slab=slab, ws_bytes=need - 1)
        assert rc == ERR_WORKSPACE and b"dl_latent_topk: workspace too small" in err, (P, D, M, slab, rc, err)
    assert rejected(ERR_WORKSPACE, ws=None)
    assert rejected(ERR_WORKSPACE, ws=_p16 + 1024 + 4)


def test_workspace_bytes_follow_the_candidate_buffers():
    """Per (64-row query tile, slab, row): CAP = pow2(2 M + 64) clamped to [128, 2048] keys of 8 bytes (room for the M kept, as
    many new ones and one tile of 64); 0 for arguments the entry rejects."""
    L = _lib.lib()
    for P in (1, 64, 65, 1000):
        for D, slab in ((64, 64), (1000, 64), (1000, 320), (4099, 1024), (1 << 20, 1 << 16)):
            for M in (1, 8, 64, 65, 100, 1000, 1024):
                if M > D:
                    assert L.dl_latent_topk_workspace_bytes(P, D, M, slab) == 0
                    continue
                cap = min(2048, max(128, 1 << (2 * M + 64 - 1).bit_length()))
                assert cap >= M + 64
                want = -(-P // 64) * -(-D // slab) * 64 * cap * 8
                assert L.dl_latent_topk_workspace_bytes(P, D, M, slab) == want, (P, D, M, slab)
    # the host's own slab: at least one slab, never more buffers than an explicit 64-row slab would take
    for P, D, M in ((1, 64, 1), (1024, 1 << 20, 1024), (17, 4099, 100)):
        own = L.dl_latent_topk_workspace_bytes(P, D, M, 0)
        assert 0 < own <= L.dl_latent_topk_workspace_bytes(P, D, M, 64)
    for bad in ((0, 100, 1, 0), (1, 0, 1, 0), (1, 100, 0, 0), (1, 100, 1, 63), (1, 1 << 31, 1, 0), (1, 5000, 1025, 0)):
        assert L.dl_latent_topk_workspace_bytes(*bad) == 0, bad
