"""The host statements of the padding contracts (tests/guard_ref.py) on hand-written examples, the case tables of
tests/test_guard_paths_gpu.py against mutant predicates (a table that cannot tell a wrong guard from the right one pins
nothing), FORMS against the cases, and the flag constants against the C header.  No GPU."""
import os
import re

import numpy as np

from tests import guard_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- rows_equal ----------------------------------------------------------------------------------------------------------------
def _rows(B, N, words):
    """[B][N][words] uint32, every row = [7, 8, ...]."""
    return np.tile(np.arange(7, 7 + words, dtype=np.uint32), (B, N, 1))


def test_rows_equal_on_hand_written_examples():
    x = _rows(2, 4, 3)
    assert G.rows_equal(x.view(np.uint8), 2, 4, 12, 0)
    y = x.copy()
    y[0, 0, 0], y[1, 1, 2] = 99, 98                                 # rows < row0 are free, in either sample
    assert G.rows_equal(y.view(np.uint8), 2, 4, 12, 2) and not G.rows_equal(y.view(np.uint8), 2, 4, 12, 1)
    assert not G.rows_equal(y.view(np.uint8), 2, 4, 12, 0)
    for (b, r, w) in ((0, 2, 0), (0, 3, 2), (1, 2, 1), (1, 3, 2)):   # the reference row itself, sample 0's tail, sample 1's
        y = x.copy()
        y[b, r, w] ^= 1 << 31
        assert not G.rows_equal(y.view(np.uint8), 2, 4, 12, 2), (b, r, w)
        assert G.rows_equal(y.view(np.uint8), 2, 4, 12, 3) == (r < 3), (b, r, w)
    y = x.copy()
    y[1, 2:] += 1                                                  # sample 1's tail is constant — but not sample 0's row
    assert not G.rows_equal(y.view(np.uint8), 2, 4, 12, 2)
    f = np.zeros((1, 3, 2), np.float32)
    f[0, :, 1] = np.float32("nan")
    assert G.rows_equal(f.view(np.uint8), 1, 3, 8, 0)              # equal NaN patterns are equal rows
    f[0, 2, 0] = -0.0
    assert not G.rows_equal(f.view(np.uint8), 1, 3, 8, 0)          # -0.0 is not +0.0
    assert G.rows_equal(f.view(np.uint8), 1, 3, 8, 2)              # one row: nothing to compare (B = 1, row0 = N - 1)


# ---- period_ok -----------------------------------------------------------------------------------------------------------------
def _protein(L, S, seed=0):
    """ids [S], fill bits [S] as the collate tiles a protein of L residues: period L + 2, zeros and fill 1.0 behind E."""
    from druglamp_amd.data import repeat_integer_label
    ids = np.asarray(repeat_integer_label(np.random.RandomState(seed).randint(1, 26, L), S)).astype(np.int64)
    fb = np.zeros(S, np.uint32)
    fb[(S // (L + 2)) * (L + 2):] = G.FILL_ONE
    return ids, fb


def test_period_ok_on_the_examples_of_the_model_tests():
    S = 2304
    ids, fb = _protein(398, S)
    assert G.period_ok(ids, fb, 400, S)                            # a tiled protein (E = 2000, 304 tail positions)
    assert (ids[2000:] == 0).all() and ids[1] != 0
    bad = ids.copy()
    bad[700] = 25 if bad[700] != 25 else 24                        # one residue of a later period
    assert not G.period_ok(bad, fb, 400, S)
    assert not G.period_ok(ids, fb, 401, S) and not G.period_ok(ids, fb, 399, S)      # a wrong length record
    ids98, fb98 = _protein(98, S)
    assert G.period_ok(ids98, fb98, 100, S) and not G.period_ok(ids98, fb98, 101, S)
    f2 = fb98.copy()
    f2[S - 3] = G.FILL_ZERO                                        # a fill bit in the zero tail
    assert not G.period_ok(ids98, f2, 100, S)
    f2 = fb98.copy()
    f2[S - 1] = G.FILL_ZERO                                        # ... also when it is the position the kernel compares with
    assert not G.period_ok(ids98, f2, 100, S)
    assert G.period_ok(bad, f2, 0, S)                              # P > L is recorded as period 0: no claim, nothing checked
    assert not G.period_ok(ids, fb, S + 1, S) and not G.period_ok(ids, fb, -1, S)
    # fewer than two whole periods: nothing periodic to compare, only the tail clause; P == L: nothing at all
    assert G.period_ok(np.arange(10), np.zeros(10, np.uint32), 10, 10)
    assert G.period_ok(np.array([1, 2, 3, 4, 5, 6, 9, 9, 9, 9]), np.zeros(10, np.uint32), 6, 10)
    assert not G.period_ok(np.array([1, 2, 3, 4, 5, 6, 9, 9, 8, 9]), np.zeros(10, np.uint32), 6, 10)
    # the boundary t + P < E: position E - P is compared with nothing behind it
    assert G.period_ok(np.array([1, 2, 3, 1, 2, 3, 0, 0]), np.zeros(8, np.uint32), 3, 8)
    assert not G.period_ok(np.array([1, 2, 3, 1, 2, 4, 0, 0]), np.zeros(8, np.uint32), 3, 8)
    # fill values as bits
    z = np.zeros(6, np.uint32)
    n = np.full(6, G.FILL_NAN, np.uint32)
    assert G.period_ok(np.ones(6), n, 2, 6)
    n[3] ^= 1
    assert not G.period_ok(np.ones(6), n, 2, 6)
    z[4] = G.FILL_SIGN
    assert not G.period_ok(np.ones(6), z, 2, 6)
    for name, mutant in G.PERIOD_MUTANTS.items():                    # the mutants are the same predicate away from their knob
        assert mutant(ids98[:200], fb98[:200], 100, 200) and not mutant(bad[:200], fb[:200], 57, 200), name


# ---- the tables bite -----------------------------------------------------------------------------------------------------------
def test_rows_cases_separate_every_mutant():
    cases = G.rows_cases(grid=False)
    split = {name: [] for name in G.ROWS_MUTANTS}
    for c in cases:
        x = G.rows_data(c)
        want = G.rows_equal(x, c.B, c.N, c.row_bytes, c.row0)
        for name, mutant in G.ROWS_MUTANTS.items():
            if mutant(x, c.B, c.N, c.row_bytes, c.row0) != want:
                split[name].append(c.name)
    for name, hits in split.items():
        assert hits, "no rows_equal case separates the mutant that %s" % name
    # ... and in the wide form in particular (the u32x4 compare is where a component can go missing)
    wide = [n for n in split["ignores words 1..3 of a 16-byte chunk"] if "_rb32_" in n and "_off0" in n]
    assert len(wide) >= 3 * 2 * 3


def test_rows_small_cases_are_exhaustive():
    for (form, rb, off, row0) in G.ROWS_SMALL:
        cases = G.rows_small_cases(form, rb, off, row0)
        words = 3 * 6 * rb // 4
        assert len(cases) == 1 + 2 * words
        hit = set()
        for c in cases[1:]:
            (byte, mask), = c.edits
            assert mask in (1, 2, 4, 8, 16, 32, 64, 128)
            hit.add((byte // 4, (byte % 4) // 2))
            x = G.rows_data(c)
            row = (byte // rb) % 6
            assert G.rows_equal(x, 3, 6, rb, row0) == (row < row0), c.name
        assert hit == {(w, h) for w in range(words) for h in (0, 1)}
        assert G.rows_equal(G.rows_data(cases[0]), 3, 6, rb, row0)


def test_period_cases_separate_every_mutant():
    split = {name: [] for name in G.PERIOD_MUTANTS}
    slots_bad = set()
    for (dt, L) in G.PERIOD_SETS[:len(G.PERIOD_L)]:                 # (the dtype changes no predicate)
        for c in G.period_cases(dt, L):
            ids, fb, period = G.period_batch(c)
            want = [G.period_ok(ids[b], fb[b], period[b], L) for b in range(G.PERIOD_B)]
            assert all(want[b] for b in range(G.PERIOD_B) if b != c.slot), c.name
            if not want[c.slot]:
                slots_bad.add(c.slot)
            for name, mutant in G.PERIOD_MUTANTS.items():
                if mutant(ids[c.slot], fb[c.slot], period[c.slot], L) != want[c.slot]:
                    split[name].append(c.name)
    for name, hits in split.items():
        assert hits, "no period case separates the mutant with %s" % name
    assert slots_bad == set(range(G.PERIOD_B))
    c = [c for c in G.period_cases("f32", 700) if c.P == 3 and c.t == 511 and c.kind == "id"][0]
    ids, fb, period = G.period_batch(c)
    assert not G.period_ok(ids[c.slot], fb[c.slot], 3, 700) and G.PERIOD_MUTANTS["ignores positions >= 256"](ids[c.slot], fb[c.slot], 3, 700)


def test_period_positions_hold_the_boundaries():
    for L in G.PERIOD_L:
        assert G.period_values(L) == (0, 1, 3, 13, L // 2, L // 2 + 1, L - 1, L, L + 1, -1)
        for P in (1, 3, 13, L // 2, L // 2 + 1, L - 1, L):
            E = (L // P) * P
            ts = set(G.period_positions(L, P))
            want = {0, P - 1, P, E - P - 1, E - P, E - 1, E, L - 2, L - 1} | {t for t in (255, 256, 511)}
            assert ts == {t for t in want if 0 <= t < L}, (L, P)


# ---- FORMS -----------------------------------------------------------------------------------------------------------------------
def test_forms_are_covered_exactly_with_quiet_and_tripping_cases():
    quiet, trips = set(), set()
    for c in G.rows_cases():
        x = G.rows_data(c)
        (quiet if G.rows_equal(x, c.B, c.N, c.row_bytes, c.row0) else trips).add(c.form)
        # the dispatch condition the form's name states
        wide = c.row_bytes % 16 == 0 and c.base_off % 16 == 0
        chunks = c.B * (c.N - c.row0) * c.row_bytes // (16 if wide else 4)
        if c.form == "rows_equal grid-stride":
            assert wide and 4096 * 256 * 2 < chunks <= 4096 * 256 * 2 + 16384 and chunks * 16 < 35e6
        else:
            assert c.form == ("rows_equal wide" if wide else "rows_equal narrow by width" if c.row_bytes % 16 else
                              "rows_equal narrow by alignment")
            assert c.base_off in (0, 4)
    for (dt, L) in G.PERIOD_SETS:
        for c in G.period_cases(dt, L):
            assert c.form == "embed_rows guard %s L %s 256" % (dt, "<=" if L <= 256 else ">")
            ids, fb, period = G.period_batch(c)
            (trips if G.period_flag(ids, fb, period, L) else quiet).add(c.form)
    for c in G.PLAN_CASES:
        B = len(G.plan_lengths(c))
        need, R, fit = G.plan_rows(c)
        assert ("plan_build B > 256" in c.forms) == (B > 256) and ("plan_build B <= 256" in c.forms) == (B <= 256)
        assert ("plan_build pad stride" in c.forms) <= (R >= 64 * 4096)
        assert ("plan_build capacity" in c.forms) == (R in (need, need - 1) or fit < B)
        assert (fit == B) == (need <= R) and B < (1 << 20)
        for f in c.forms:
            (trips if G.plan_trips(c) else quiet).add(f)
    assert quiet == set(G.FORMS), quiet ^ set(G.FORMS)
    assert trips == set(G.FORMS), trips ^ set(G.FORMS)


def test_plan_cases_hold_every_mode_boundary():
    """All lengths 1 .. S + 40 in one batch: plain, merged-tail and three-segment samples and a period beyond the sequence."""
    from druglamp_amd.protein_plan import ProteinPlan, _segments
    for c in G.PLAN_CASES:
        lengths = G.plan_lengths(c)
        if c.lengths == "all":
            assert list(lengths) == list(range(1, c.S + 41))
        else:
            assert len(lengths) == 709 and {c.S // 2 - 2, c.S // 2 - 1, c.S - 2, c.S + 5} <= set(int(v) for v in lengths)
        kinds = {(None if s is None else len(s)) for s in (_segments(int(v) + 2, c.S) for v in lengths)}
        assert kinds == ({None} if c.S == 64 else {None, 2, 3}), (c.name, kinds)
    c = G.PLAN_CASES[4]
    need, R, fit = G.plan_rows(c)
    assert c.R == "sample300" and fit == 300 and need > R
    assert ProteinPlan(G.plan_lengths(G.PLAN_CASES[0]), 64, bucket=1).rows == G.plan_rows(G.PLAN_CASES[0])[0]


# ---- the flag constants ------------------------------------------------------------------------------------------------------------
def test_flag_bits_match_the_header_and_have_texts():
    from druglamp_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "druglamp_hip.h")) as f:
        hdr = f.read()
    for name, py, value in (("DL_FLAG_PROT_PERIOD", _lib.FLAG_PROT_PERIOD, 1), ("DL_FLAG_DRUG_TOKEN_PAD", _lib.FLAG_DRUG_TOKEN_PAD, 2),
                            ("DL_FLAG_GCN_NODE_PAD", _lib.FLAG_GCN_NODE_PAD, 4), ("DL_FLAG_PLAN_ROWS", _lib.FLAG_PLAN_ROWS, 8)):
        assert py == value and re.search(r"%s\s*=\s*%d\b" % (name, value), hdr), name
    bits = {int(m) for m in re.findall(r"DL_FLAG_[A-Z_]+\s*=\s*(\d+)", hdr)}
    assert bits == {1, 2, 4, 8, 16, 32, 64}
    assert set(ops.FLAG_TEXT) == bits and all(isinstance(v, str) and len(v) > 20 for v in ops.FLAG_TEXT.values())
    texts = [ops.guard_text(b) for b in sorted(bits)]
    assert len(set(texts)) == len(bits) and not any("unknown" in t for t in texts)
    assert ops.guard_text(1 | 4) == ops.FLAG_TEXT[1] + "; " + ops.FLAG_TEXT[4] and "unknown" in ops.guard_text(1 << 20)
