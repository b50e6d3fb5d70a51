"""Host statements of the three padding contracts that csrc/compact.hip guards on the device, and the case tables the GPU
tests run (tests/test_guard_paths_gpu.py).  numpy only; tests/test_guard_reference_cpu.py pins the predicates, shows that the
tables separate every mutant predicate below from the true one, and that the cases cover FORMS exactly.

  rows_equal    dl_rows_equal_check: x [B][N][row_bytes]; every row r >= row0 of every sample equals row row0 of SAMPLE 0 byte
                for byte (rows < row0 are free).  The drug LLM adaptor's token tail and MolecularGCN's virtual padding nodes.
  period_ok     the guard workgroups of dl_embed_rows, per sample, as the kernel's comment states it: sym(t) = (id, bit pattern
                of the fill value); P == 0 checks nothing; P < 0 or P > L is bad; otherwise sym(t) == sym(t + P) while
                t + P < E = (L // P) * P, and one constant symbol on [E, L).  Fill values are compared as BITS: -0.0 != +0.0,
                two NaNs with equal patterns are equal.
  row tables    dl_protein_plan_build: protein_plan.ProteinPlan(lengths, S, bucket=1) is the host statement already; here only
                the cases (lengths, capacity R) and what a refused build may touch.

Every malformed input is malformed as DATA only: ids stay inside the vocabulary, periods that are out of range are never used
as an offset by the kernel (it flags the sample before reading anything), capacities below the need make the build write
less, never elsewhere.
"""
import collections
import functools

import numpy as np

from druglamp_amd.protein_plan import PlanSpec

# launch form -> the condition that selects it (host dispatch of csrc/compact.hip)
FORMS = collections.OrderedDict([
    ("rows_equal wide", "dl_rows_equal_check, row_bytes % 16 == 0 and a 16-byte-aligned base: rows_equal_check_kernel<u32x4>"),
    ("rows_equal narrow by width", "dl_rows_equal_check, row_bytes % 16 != 0 (12, 300 = MolecularGCN's 75 fp32 features): <uint32_t>"),
    ("rows_equal narrow by alignment", "dl_rows_equal_check, row_bytes % 16 == 0 but the base 4 bytes behind a 16-byte address "
                                       "(a direct call only: torch allocations are aligned): <uint32_t>"),
    ("rows_equal grid-stride", "dl_rows_equal_check, more than 4096 * 256 * 2 chunks: ceil(chunks / 2048) workgroups (capped at "
                               "4096), every thread walks ci += gridDim * 256 eight times, chunk indices pass 2^21"),
    ("embed_rows guard bf16 L <= 256", "dl_embed_rows with period, bf16: B guard workgroups behind the gather workgroups; one trip of t += 256"),
    ("embed_rows guard bf16 L > 256", "the same, positions reached only in a later trip of t += 256"),
    ("embed_rows guard f32 L <= 256", "dl_embed_rows with period, fp32; one trip of t += 256"),
    ("embed_rows guard f32 L > 256", "the same, positions reached only in a later trip of t += 256"),
    ("plan_build B <= 256", "dl_protein_plan_build: the per-workgroup prefix sum `for (i = tid; i < upto; i += 256)` takes one trip"),
    ("plan_build B > 256", "the same loop takes a second trip for the samples (and the padding workgroups) behind sample 256"),
    ("plan_build pad stride", "R >= 64 * 4096: all 64 padding workgroups run and stride by nb * 256 rows several times"),
    ("plan_build capacity", "the padding workgroups' `off > R`: R == need is the last quiet capacity, R == need - 1 raises "
                            "DL_FLAG_PLAN_ROWS and the samples that do not fit write nothing"),
])


# ---- rows_equal ----------------------------------------------------------------------------------------------------------------
def rows_equal(x_bytes, B, N, row_bytes, row0):
    x = np.asarray(x_bytes, dtype=np.uint8).reshape(B, N, row_bytes)
    return bool((x[:, row0:] == x[0, row0]).all())


def _re_ignores_last_word(x, B, N, rb, row0):
    x = np.asarray(x, np.uint8).reshape(B, N, rb)
    return bool((x[:, row0:, :rb - 4] == x[0, row0, :rb - 4]).all())


def _re_ignores_last_sample(x, B, N, rb, row0):
    x = np.asarray(x, np.uint8).reshape(B, N, rb)
    return bool((x[:B - 1, row0:] == x[0, row0]).all())


def _re_ignores_sample0_tail(x, B, N, rb, row0):
    x = np.asarray(x, np.uint8).reshape(B, N, rb)
    return bool((x[1:, row0:] == x[0, row0]).all())


def _re_same_sample_reference(x, B, N, rb, row0):
    x = np.asarray(x, np.uint8).reshape(B, N, rb)
    return bool((x[:, row0:] == x[:, row0:row0 + 1]).all())


def _re_first_word_of_chunk_only(x, B, N, rb, row0):
    x = np.asarray(x, np.uint8).reshape(B, N, rb)
    keep = (np.arange(rb) % 16) < 4
    return bool((x[:, row0:, keep] == x[0, row0, keep]).all())


def _re_starts_one_row_late(x, B, N, rb, row0):
    x = np.asarray(x, np.uint8).reshape(B, N, rb)
    return bool((x[:, row0 + 1:] == x[0, row0]).all())


ROWS_MUTANTS = collections.OrderedDict([
    ("ignores the last 4-byte word of a row", _re_ignores_last_word),
    ("ignores the last sample", _re_ignores_last_sample),
    ("ignores sample 0's own tail rows", _re_ignores_sample0_tail),
    ("compares with row row0 of the same sample", _re_same_sample_reference),
    ("ignores words 1..3 of a 16-byte chunk", _re_first_word_of_chunk_only),
    ("starts at row0 + 1", _re_starts_one_row_late),
])

# base_off: bytes between a 16-byte address and the first byte; edits: ((byte index, xor mask), ...) applied to rows_base
RowsCase = collections.namedtuple("RowsCase", "name form B N row_bytes row0 base_off edits")
NAN_WORD = 0x7FC07FC0              # a quiet NaN as two bf16 values; as one fp32 value a NaN too


@functools.lru_cache(maxsize=4)
def rows_base(B, N, row_bytes, row0):
    """A well-formed input: free rows (< row0) arbitrary and all different, the tail rows one pattern — whose first and last
    word are +0.0 and whose second word is a NaN (equal NaN bits are equal rows)."""
    rs = np.random.RandomState(B * 1000003 + N * 1009 + row_bytes * 7 + row0)
    x = np.frombuffer(rs.bytes(B * N * row_bytes), dtype=np.uint8).reshape(B, N, row_bytes).copy()
    pat = rs.randint(1, 256, row_bytes).astype(np.uint8)
    w = pat.view(np.uint32)
    w[0] = w[-1] = 0
    if w.size > 2:
        w[1] = NAN_WORD
    x[:, row0:] = pat
    x.setflags(write=False)
    return x.reshape(-1)


def rows_data(c):
    x = rows_base(c.B, c.N, c.row_bytes, c.row0).copy()
    for i, m in c.edits:
        x[i] ^= m
    return x


def _flip(word, half):
    """(byte, mask) of one bit of 32-bit word `word`: bit (7 word + 3) % 16 of its low (half 0) or high (half 1) half-word."""
    bit = (7 * word + 3) % 16 + 16 * half
    return (4 * word + bit // 8, 1 << (bit % 8))


ROWS_SMALL = tuple((form, rb, off, row0) for (form, rb, off) in (("rows_equal wide", 32, 0), ("rows_equal narrow by width", 12, 0),
                                                               ("rows_equal narrow by width", 300, 0),
                                                               ("rows_equal narrow by alignment", 32, 4))
                   for row0 in (0, 2, 5))


def rows_small_cases(form, rb, off, row0, B=3, N=6):
    """The untouched input, then one case per 32-bit word and half-word of the WHOLE input with one bit flipped: the words of
    the checked region (rows >= row0) must trip, the words of the free rows must stay quiet."""
    tag = "rows_B%d_N%d_rb%d_row0%d_off%d" % (B, N, rb, row0, off)
    out = [RowsCase(tag + "_clean", form, B, N, rb, row0, off, ())]
    for word in range(B * N * rb // 4):
        for half in (0, 1):
            out.append(RowsCase("%s_w%d_h%d" % (tag, word, half), form, B, N, rb, row0, off, (_flip(word, half),)))
    return out


def rows_product_cases():
    """The product's widths (392 bf16 = 784 bytes, 1568 bytes), N = 512, the hinted blocks 128 and 384, B = 2 and B = 1: a
    deviation in the first and in the last chunk of the last row of the last sample, as a low bit and as +0.0 -> -0.0."""
    out = []
    for B in (2, 1):
        for rb in (784, 1568):
            for row0 in (128, 384):
                tag = "rows_B%d_N512_rb%d_row0%d" % (B, rb, row0)
                last = (B * 512 - 1) * rb
                out.append(RowsCase(tag + "_clean_with_equal_nans", "rows_equal wide", B, 512, rb, row0, 0, ()))
                for what, byte, mask in (("first_chunk_bit", last + 8, 1), ("first_chunk_negative_zero", last + 3, 0x80),
                                         ("last_chunk_bit", last + rb - 16, 4), ("last_chunk_negative_zero", last + rb - 1, 0x80),
                                         ("free_row", last - (512 - row0) * rb, 1)):
                    out.append(RowsCase("%s_%s" % (tag, what), "rows_equal wide", B, 512, rb, row0, 0, ((byte, mask),)))
    return out


GRID_B, GRID_N, GRID_RB, GRID_ROW0 = 56, 400, 1568, 16        # 56 * 384 * 98 = 2 107 392 chunks > 4096 * 256 * 2 (33.7 MB checked)


def rows_grid_cases():
    tag = "rows_grid_B%d_N%d_rb%d_row0%d" % (GRID_B, GRID_N, GRID_RB, GRID_ROW0)
    n = GRID_B * GRID_N * GRID_RB
    return [RowsCase(tag + "_clean", "rows_equal grid-stride", GRID_B, GRID_N, GRID_RB, GRID_ROW0, 0, ()),
            RowsCase(tag + "_last_chunk", "rows_equal grid-stride", GRID_B, GRID_N, GRID_RB, GRID_ROW0, 0, ((n - 1, 0x80),)),
            RowsCase(tag + "_last_chunk_first_word", "rows_equal grid-stride", GRID_B, GRID_N, GRID_RB, GRID_ROW0, 0, ((n - 16, 1),))]


def rows_cases(small=True, product=True, grid=True):
    out = []
    if small:
        for g in ROWS_SMALL:
            out += rows_small_cases(*g)
    if product:
        out += rows_product_cases()
    if grid:
        out += rows_grid_cases()
    return out


# ---- the protein period --------------------------------------------------------------------------------------------------------
def period_ok(ids, fill_bits, P, L):
    P, L = int(P), int(L)
    if P == 0:
        return True
    if P < 0 or P > L:
        return False
    ids, fb = np.asarray(ids).reshape(-1)[:L], np.asarray(fill_bits).reshape(-1)[:L]
    E = (L // P) * P
    ok = bool((ids[:E - P] == ids[P:E]).all() and (fb[:E - P] == fb[P:E]).all())
    return ok and bool((ids[E:] == ids[L - 1]).all() and (fb[E:] == fb[L - 1]).all())


def _period_loop(ids, fb, P, L, pair=lambda t, P, E: t + P < E, tail=True, fills=True, limit=None):
    """The kernel's loop, position by position, with the knobs the mutants turn."""
    P, L = int(P), int(L)
    if P == 0:
        return True
    if P < 0 or P > L:
        return False
    E = (L // P) * P
    for t in range(L if limit is None else min(L, limit)):
        if pair(t, P, E) and t + P < L and (ids[t] != ids[t + P] or (fills and fb[t] != fb[t + P])):
            return False
        if tail and t >= E and (ids[t] != ids[L - 1] or (fills and fb[t] != fb[L - 1])):
            return False
    return True


PERIOD_MUTANTS = collections.OrderedDict([
    ("t + P <= E", lambda i, f, P, L: _period_loop(i, f, P, L, pair=lambda t, P_, E: t + P_ <= E)),
    ("no [E, L) clause", lambda i, f, P, L: _period_loop(i, f, P, L, tail=False)),
    ("ignores fill bits", lambda i, f, P, L: _period_loop(i, f, P, L, fills=False)),
    ("ignores positions >= 256", lambda i, f, P, L: _period_loop(i, f, P, L, limit=256)),
])

PERIOD_V, PERIOD_D, PERIOD_B = 27, 127, 4
PERIOD_L = (40, 300, 700)
FILL_ZERO, FILL_ONE, FILL_NAN, FILL_SIGN = 0x00000000, 0x3F800000, 0x7FC00000, 0x80000000     # fp32 patterns, exact in bf16 too
# t: the edited position (None: the tiled sample as it is); kind: "id" | "fill" (0 <-> 1) | "sign" (+0.0 -> -0.0 and alike)
PeriodCase = collections.namedtuple("PeriodCase", "name form dt L P slot t kind")


def period_values(L):
    return (0, 1, 3, 13, L // 2, L // 2 + 1, L - 1, L, L + 1, -1)


def period_positions(L, P):
    P_ = P if 0 < P <= L else 13
    E = (L // P_) * P_
    return sorted(t for t in {0, P_ - 1, P_, E - P_ - 1, E - P_, E - 1, E, L - 2, L - 1, 255, 256, 511} if 0 <= t < L)


def tiled_sample(L, P, seed):
    """ids [L] int64 and fill bits [L] uint32 tiled with period P (13 where P makes no claim or is out of range); the tail
    [E, L) is one symbol (0, 1.0) that differs from every symbol of the period — NaN and +0.0 fills are among those."""
    P = P if 0 < P <= L else 13
    rs = np.random.RandomState(seed)
    E = (L // P) * P
    ids = np.zeros(L, np.int64)
    fb = np.full(L, FILL_ONE, np.uint32)
    ids[:E] = np.tile(rs.randint(1, PERIOD_V, P), L // P)
    fb[:E] = np.tile(np.array([FILL_ZERO, FILL_NAN, FILL_ZERO, FILL_ONE], np.uint32)[rs.randint(0, 4, P)], L // P)
    return ids, fb


def period_batch(c):
    """(ids [4][L], fill bits [4][L], period [4]) of one launch: three tiled samples and, in slot c.slot, the sample of the
    case.  A period that is out of range stands in its slot only; the other samples then use period 13."""
    valid = 0 <= c.P <= c.L
    ids = np.zeros((PERIOD_B, c.L), np.int64)
    fb = np.zeros((PERIOD_B, c.L), np.uint32)
    period = np.full(PERIOD_B, c.P if valid else 13, np.int32)
    for b in range(PERIOD_B):
        ids[b], fb[b] = tiled_sample(c.L, c.P, 31 * c.L + 7 * (c.P + 1) + b)
    period[c.slot] = c.P
    if c.t is not None:
        if c.kind == "id":
            ids[c.slot, c.t] = (ids[c.slot, c.t] + 1) % PERIOD_V
        else:
            fb[c.slot, c.t] ^= FILL_ONE if c.kind == "fill" else FILL_SIGN
    return ids, fb, period


def period_flag(ids, fb, period, L):
    return any(not period_ok(ids[b], fb[b], period[b], L) for b in range(len(period)))


def period_cases(dt, L):
    form = "embed_rows guard %s L %s 256" % (dt, "<=" if L <= 256 else ">")
    out, k = [], 0
    for P in period_values(L):
        out.append(PeriodCase("period_%s_L%d_P%d_tiled" % (dt, L, P), form, dt, L, P, k % PERIOD_B, None, None))
        k += 1
        for t in period_positions(L, P):
            for kind in ("id", "fill", "sign"):
                out.append(PeriodCase("period_%s_L%d_P%d_%s_t%d_slot%d" % (dt, L, P, kind, t, k % PERIOD_B), form, dt, L, P,
                                      k % PERIOD_B, t, kind))
                k += 1
    return out


PERIOD_SETS = tuple((dt, L) for dt in ("bf16", "f32") for L in PERIOD_L)


# ---- the row tables ----------------------------------------------------------------------------------------------------------------
PAD_ROWS = 64 * 4096 + 1000        # all 64 padding workgroups, several trips of their nb * 256 stride
# lengths: "all" = 1 .. S + 40, "seeded" = 700 seeded lengths + the boundary lengths of the existing test
# R: "need" | "need-1" | "sample300" (capacity ends inside sample 300) | "pad" (PAD_ROWS, above the need)
PlanCase = collections.namedtuple("PlanCase", "name forms S lengths R")
PLAN_CASES = [
    PlanCase("plan_S64_all_need", ("plan_build B <= 256", "plan_build capacity"), 64, "all", "need"),
    PlanCase("plan_S64_all_need-1", ("plan_build B <= 256", "plan_build capacity"), 64, "all", "need-1"),
    PlanCase("plan_S300_all_need", ("plan_build B > 256", "plan_build capacity"), 300, "all", "need"),
    PlanCase("plan_S300_all_need-1", ("plan_build B > 256", "plan_build capacity"), 300, "all", "need-1"),
    PlanCase("plan_S300_all_sample300", ("plan_build B > 256", "plan_build capacity"), 300, "all", "sample300"),
    PlanCase("plan_S300_all_pad", ("plan_build B > 256", "plan_build pad stride"), 300, "all", "pad"),
    PlanCase("plan_S2304_seeded_need", ("plan_build B > 256", "plan_build capacity"), 2304, "seeded", "need"),
    # (R >= 64 * 4096 here too: all 64 padding workgroups take the overflow exit and write nothing)
    PlanCase("plan_S2304_seeded_need-1", ("plan_build B > 256", "plan_build pad stride", "plan_build capacity"), 2304, "seeded", "need-1"),
]


def plan_lengths(c):
    S = c.S
    if c.lengths == "all":
        return np.arange(1, S + 41, dtype=np.int32)
    edge = [S // 2 - 2, S // 2 - 1, S // 2, S // 3 - 2, S // 3 - 1, S - 2, S - 1, S, S + 5]
    return np.concatenate([np.random.RandomState(S).randint(1, S + 30, 700), edge]).astype(np.int32)


def plan_rows(c):
    """(need, R, fit): rows the lengths need, the capacity the kernel is given, the number of leading samples that fit."""
    from druglamp_amd.protein_plan import sample_rows
    lengths = plan_lengths(c)
    rows = sample_rows(lengths, c.S)
    ends = np.cumsum(rows)
    need = int(ends[-1])
    assert need == PlanSpec(lengths, c.S).need
    R = {"need": need, "need-1": need - 1, "pad": PAD_ROWS}.get(c.R)
    if R is None:
        R = int(ends[299]) + 5
    return need, R, int((ends <= R).sum())


def plan_trips(c):
    need, R, _ = plan_rows(c)
    return need > R
