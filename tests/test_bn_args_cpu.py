"""The dl_bn_* entry points: the argument validation that runs before any launch (status code + dl_last_error() naming the
entry), and dl_bn_workspace_bytes against the chunking rule of the partial-sum kernels.  None of this needs a device: the
library loads without one, and every call below is rejected before its first launch."""
import ctypes as C

import pytest

from druglamp_amd import _lib

OK, ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -4

# entry -> its parameters in C order.  Pointers: every name of PTRS; `ws` goes with `ws_bytes`.
ENTRIES = {
    "dl_bn_stats": "y R C win halo valid dtype sums ws ws_bytes stream",
    "dl_bn_stats_rw": "y R C row_w dtype sums ws ws_bytes stream",
    "dl_bn_bwd_reduce": "dz y mean rstd R C win halo valid dtype sums ws ws_bytes stream",
    "dl_bn_bwd_reduce_rw": "dz y mean rstd R C row_w dtype sums ws ws_bytes stream",
    "dl_bn_apply_fwd": "y z mean rstd gamma beta R C win halo valid dtype stream",
    "dl_bn_apply_fwd_rw": "y z mean rstd gamma beta R C row_w dtype stream",
    "dl_bn_bwd_apply": "dz y mean rstd gamma sums inv_n relu_mask dy R C win halo valid dtype stream",
    "dl_bn_bwd_apply_rw": "dz y mean rstd gamma sums inv_n relu_mask dy R C row_w dtype stream",
    "dl_bn_tail_fix": "dy y mean rstd gamma sums inv_n w R C twin lead dtype stream",
    "dl_bn_finalize": "sums n eps momentum mean var rstd rmean rvar C stream",
    "dl_bn_stats_finalize": "y R C win halo valid row_w dtype n eps momentum sums mean var rstd rmean rvar ws ws_bytes stream",
    "dl_bn_apply_relu_fwd": "y z mean rstd gamma beta R C dtype stream",
    "dl_bn_relu_bwd": "dz y mean rstd gamma beta inv_n dy sums R C dtype ws ws_bytes stream",
    "dl_bn_eval_bwd": "dz y mean rstd gamma beta relu_in relu_out dy sums R C win halo valid row_w dtype ws ws_bytes stream",
}
PTRS = ("y", "z", "dz", "dy", "mean", "var", "rstd", "gamma", "beta", "sums", "rmean", "rvar", "row_w", "ws")
# the pointers an entry may be given as NULL (dl_bn_eval_bwd: no sums wanted, no ReLU behind; the running statistics; plain rows)
OPTIONAL = {"dl_bn_stats_finalize": ("sums", "rmean", "rvar", "row_w"), "dl_bn_finalize": ("rmean", "rvar"),
            "dl_bn_eval_bwd": ("beta", "sums", "row_w")}
SCALARS = dict(R=72, C=64, win=36, halo=4, valid=27, dtype=_lib.DL_BF16, inv_n=1.0 / 72, relu_mask=0, relu_in=0, relu_out=0, w=5,
               twin=24, lead=16, n=72, eps=1e-5, momentum=0.1, stream=None)
WINDOWED = [e for e, p in ENTRIES.items() if " win " in p]
WORKSPACE = [e for e, p in ENTRIES.items() if " ws " in p]
APPLY = [e for e, p in ENTRIES.items() if "apply" in e or e == "dl_bn_relu_bwd"]     # one thread per 4 elements, 32-bit index
_buf = (C.c_char * 4096)()
_p16 = (C.addressof(_buf) + 15) // 16 * 16


def call(entry, **kw):
    """`entry` with a valid argument list (bf16 [72][64], distinct 16-byte aligned pointers, a workspace of exactly
    dl_bn_workspace_bytes) changed by `kw`: (status, dl_last_error())."""
    L = _lib.lib()
    a = dict(SCALARS)
    a.update({p: _p16 + 64 * i for i, p in enumerate(PTRS)})
    a.update(kw)
    a.setdefault("ws_bytes", L.dl_bn_workspace_bytes(a["R"], a["C"]) if a["R"] > 0 and a["C"] > 0 else 0)
    rc = getattr(L, entry)(*[a[p] for p in ENTRIES[entry].split()])
    return rc, L.dl_last_error()


def rejected(entry, code, **kw):
    rc, err = call(entry, **kw)
    return rc == code and (entry + ":").encode() in err


def test_the_fourteen_entry_points_are_exported_with_their_signatures():
    L = _lib.lib()
    assert len(ENTRIES) == 14
    for entry, params in ENTRIES.items():
        res, args = _lib.SIGNATURES[entry]
        assert getattr(L, entry).restype is res and len(args) == len(params.split()), entry


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_pointers_and_bad_columns(entry):
    params = ENTRIES[entry].split()
    for p in params:
        if p in PTRS and p != "ws" and p not in OPTIONAL.get(entry, ()):
            assert rejected(entry, ERR_ARG, **{p: None}), (entry, p)
    if entry == "dl_bn_finalize":
        assert rejected(entry, ERR_ARG, C=0) and rejected(entry, ERR_ARG, n=0)
        return
    assert rejected(entry, ERR_ARG, C=66), entry          # C % 4 != 0
    assert rejected(entry, ERR_ARG, C=0) and rejected(entry, ERR_ARG, R=0), entry


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e not in ("dl_bn_finalize", "dl_bn_tail_fix")])
def test_row_count_must_fit_31_bits(entry):
    rc, err = call(entry, R=1 << 31, C=4)
    assert rc == ERR_SHAPE and (entry + ":").encode() in err and b"fit" in err, (entry, rc, err)


@pytest.mark.parametrize("entry", APPLY)
def test_apply_passes_index_quads_with_32_bits(entry):
    rc, err = call(entry, R=1 << 30, C=16)                # R * C / 4 = 2^32
    assert rc == ERR_SHAPE and (entry + ":").encode() in err and b"R * C / 4 must fit 32 bits" in err, (entry, rc, err)


@pytest.mark.parametrize("entry", WORKSPACE)
def test_workspace_one_byte_too_small(entry):
    L = _lib.lib()
    for R, Cc in ((72, 64), (8300, 72), (591864, 128)):
        need = L.dl_bn_workspace_bytes(R, Cc)
        rc, err = call(entry, R=R, C=Cc, win=0, halo=0, valid=0, ws_bytes=need - 1)
        assert rc == ERR_WORKSPACE and (entry + ": workspace too small").encode() in err, (entry, R, Cc, rc, err)
    assert rejected(entry, ERR_WORKSPACE, ws=None), entry


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e.endswith("_rw")])
def test_rw_entries_need_row_weights(entry):
    rc, err = call(entry, row_w=None)
    assert rc == ERR_ARG and (entry + ":").encode() in err and b"null" in err, (entry, rc, err)


def test_eval_bwd_flags_and_aliasing():
    e = "dl_bn_eval_bwd"
    rc, err = call(e, relu_out=1, beta=None)
    assert rc == ERR_ARG and b"dl_bn_eval_bwd: relu_out needs beta" in err
    for other in ("dz", "y"):
        rc, err = call(e, dy=_p16 + 64 * PTRS.index(other))
        assert rc == ERR_ARG and b"dl_bn_eval_bwd: dy must not alias dz or y" in err, other


def test_tail_fix_window():
    e = "dl_bn_tail_fix"
    for kw in (dict(twin=0), dict(lead=24), dict(lead=-1), dict(twin=25), dict(w=0)):     # (twin 25: R % win != 0)
        assert rejected(e, ERR_ARG, **kw), kw


# ---- the two deliberate changes of the shared-argument-check refactor: before it only some entries checked these ----------
@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "dl_bn_finalize"])
def test_unknown_dtype_is_rejected_everywhere(entry):
    rc, err = call(entry, dtype=7)
    assert rc == ERR_ARG and (entry + ": bad dtype").encode() in err, (entry, rc, err)


@pytest.mark.parametrize("entry", WINDOWED)
def test_bad_window_is_rejected_everywhere(entry):
    for kw in (dict(win=-1), dict(halo=-1), dict(valid=-1), dict(win=30, halo=4, valid=27), dict(win=1 << 31, halo=0, valid=1)):
        rc, err = call(entry, **kw)
        assert rc == ERR_ARG and (entry + ": bad window").encode() in err, (entry, kw, rc, err)
    if entry in WORKSPACE:      # win == 0: no window, halo / valid are not looked at; the call gets as far as the workspace check
        assert rejected(entry, ERR_WORKSPACE, win=0, halo=3, valid=9, ws=None), entry


def test_workspace_bytes_cover_the_partials_of_every_chunk():
    """partial[chunks][2][C] floats, chunks = ceil(R / rows) with rows = ceil(R / ceil(1024 / ceil(C / 256))), at least 32,
    rounded up to a multiple of 4 (four waves walk a chunk's rows)."""
    L = _lib.lib()
    for R in (1, 31, 32, 33, 70, 8300, 32768, 32769, 163840, 591864):
        for Cc in (4, 64, 72, 128, 256, 512):
            colgroups = -(-Cc // 256)
            rows = max(32, -(-R // -(-1024 // colgroups)))
            rows = -(-rows // 4) * 4
            chunks = -(-R // rows)
            assert L.dl_bn_workspace_bytes(R, Cc) >= chunks * 2 * Cc * 4, (R, Cc)
