"""The entry points of the resident route (include/parsnp_mum.h: pm_store_*), call by call against the sequential restatement of
tests/storecalls.py, in the kernel emulation (tests/emu: one host thread plays every lane of the kernels of store_kernels.h).
tests/test_gpu_store_calls.py runs the same checks on the device.  The end-to-end tests (test_resident_route* in
test_emu_engine.py, test_gpu_parity.py, the fuzz runs) say that a run's bytes are the reference's; these say WHICH call is wrong
when they are not, and they go where the named sets do not: marks across 64-bit words and the 256-row walks of StoreMarkOrdered,
more than 64 genomes (lanes_for wraps), gaps of exactly 0 and exactly d, LCBs of length exactly c, the ratio test at equality,
reverse pairs in the chain.

Every case asserts its floors: the counts that say the path was really taken, from the fixed seeds of the generator."""
import contextlib
import functools
import os

import numpy as np
import pytest

import storecalls as sc
from parsnp_amd.binding import Lib

SETS = {
    "collinear6": dict(seed=11, n=6, length=20000, pairs=12),
    "collinear70": dict(seed=12, n=70, length=12000, pairs=7),
    "collinear131": dict(seed=13, n=131, length=8000, pairs=5),
    "rearranged8": dict(seed=14, n=8, length=20000, pairs=12, inversions=((7, 0.22, 0.55),), translocate=(5, 0.62, 0.68)),
    "inverted70": dict(seed=15, n=70, length=12000, pairs=7, inversions=((2, 0.30, 0.45), (66, 0.30, 0.45))),
}
# case -> (set, tunables of the session, floors).  The floors lie below what the generator gives in the emulation (in brackets).
CASES = {
    # the default flagged_div: the list is taken as it is (PM_OK); 398 rows cross a 256-row walk of StoreMarkOrdered
    "collinear6": ("collinear6", {}, dict(rows=257, flagged=20, tangled=12, trimmed=20, lone=4)),                # [398, 31, 24, 31, 7]
    "collinear6_atomic_marks": ("collinear6", {"atomic_marks": 1}, dict(rows=257, flagged=20, tangled=12, trimmed=20)),
    "collinear6_serial_tangle": ("collinear6", {"tangle_rounds": 0}, dict(rows=257, flagged=20, tangled=12, trimmed=20)),
    "collinear6_walks_reversed": ("collinear6", {}, dict(rows=257, flagged=20, tangled=12, trimmed=20)),
    "collinear70": ("collinear70", {}, dict(rows=200, flagged=12, tangled=8, trimmed=12)),                      # [252, 20, 14, 20]
    "collinear131": ("collinear131", {}, dict(rows=128, flagged=10, tangled=6, trimmed=10)),                    # [161, 15, 10, 15]
    "rearranged8": ("rearranged8", {"flagged_div": 1}, dict(rows=257, flagged=60, tangled=16, trimmed=20, reverse=5, verdicts=3, early=1, unordered=1, cross_right=1)),
    "inverted70": ("inverted70", {}, dict(rows=200, flagged=30, tangled=10, trimmed=12, reverse=5, verdicts=3, early=1)),
}
# (emulation only) the launch whose wavefronts run last to first in the case: neighbouring walks of StoreMarkOrdered share a word, and
# the one thread of the emulation meets a lost update there only when the LATER walk has written first
REVERSED = {"collinear6_walks_reversed": "store_mark_ordered"}
CHAIN_CASES = ["collinear6", "collinear70", "collinear131", "rearranged8", "inverted70"]
# (diag_diff, d) of the chain runs: 0.5 and 0.7 with d = 10 meet the planted (1, 2) and (3, 10) gaps with the ratio exactly at the bar
# (1 / 2, and 3 / 10 = 1 - float(0.7) in the reference's float / double mix) and the gap of 10 exactly at d
CHAIN_GRID = [(1.0, 2), (0.5, 10), (0.7, 10), (0.12, 300)]


@pytest.fixture(scope="module")
def lib(emu):
    return Lib(emu[0])


@functools.lru_cache(maxsize=None)
def sequences(name):
    return sc.make_set(**SETS[name])


def same_layout(got, want, what):
    for j, (a, b) in enumerate(zip(got, want)):
        if not np.array_equal(a, b):
            x = int(np.flatnonzero(a != b)[0])
            raise AssertionError("%s: layout of genome %d differs first at base %d (word %d, bit %d): engine %d, restatement %d; %d bases differ"
                                 % (what, j, x, x >> 6, x & 63, a[x], b[x], int((a != b).sum())))


def first_diff(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shapes %s and %s" % (got.shape, want.shape)
    x = np.argwhere(got != want)
    return None if not len(x) else "first at %s: engine %s, restatement %s (%d differ)" % (tuple(x[0]), got[tuple(x[0])], want[tuple(x[0])], len(x))


@contextlib.contextmanager
def wave_order(case):
    """the order of the wavefronts of the case's launches (tests/emu/engine_emu.cpp: PM_EMU_REVERSE_WAVES)"""
    if case in REVERSED:
        os.environ["PM_EMU_REVERSE_WAVES"] = REVERSED[case]
    try:
        yield
    finally:
        os.environ.pop("PM_EMU_REVERSE_WAVES", None)


class Outcome:
    """the calls of one session on one case, and what the restatement says to each"""


_outcomes = {}


def outcome(lib, case):
    """settle, info, rows, judge, fill and unmark in ONE session (run once per library and case, shared by the tests below)"""
    key = (lib.path, case)
    if key in _outcomes:
        return _outcomes[key]
    name, tune, floors = CASES[case]
    seqs = sequences(name)
    o = Outcome()
    o.floors = floors
    with wave_order(case), sc.Store(lib, seqs, tune=tune) as st:
        o.lon, o.flags, o.raw_start, o.strand, o.glen = st.lon, st.flags, st.raw_start, st.strand, st.glen
        o.rc, o.info = st.settle()
        assert o.rc == sc.PM_OK, "pm_store_settle declined the list (code %d)" % o.rc
        m = o.model = sc.Model(seqs, st.raw_start, st.strand, st.lon, st.flags).settle()
        o.layout = st.layout()
        o.info_again = st.info(0, st.A)
        o.trimmed_start, o.trimmed_strand = st.rows(None, 0, st.A, raw=False)
        o.acc = m.acc_rows()
        back = o.acc[::-1]
        o.listed = back, st.rows(back, 0, 0, raw=False), st.rows(back, 0, 0, raw=True)
        o.sorted, o.tie = m.sorted_rows()
        cur, prev = o.sorted[1:], o.sorted[:-1]
        at300 = [m.judge(a, b, 300) for a, b in zip(cur, prev)]
        o.G = max(mx for v, mn, mx in at300 if v == 0)      # the largest gap of the list that d = 300 takes
        o.judge = {}
        for d in (o.G, o.G - 1, 0, 300):
            o.judge[d] = st.judge(cur, prev, d), [m.judge(a, b, d) for a, b in zip(cur, prev)]
        lay = m.layout()
        o.fill = st.fill(prev, cur), [m.fill(b, a, lay) for a, b in zip(cur, prev)]
        o.unmarked = o.acc[::3]
        st.unmark(o.unmarked)
        o.layout_unmarked = st.layout()
    _outcomes[key] = o
    return o


# ------------------------------------------------------------------------------------------------------------------ settle
def check_settle(lib, case):
    """pm_store_settle: per row the accepted bit, the left trim, the length and the trimmed reference start; the state bits that
    follow from the flags; and the floors of the case"""
    o = outcome(lib, case)
    m, f = o.model, o.floors
    state = o.info["state_flags"] & 0xff
    assert np.array_equal(o.info["state_flags"] >> 8, o.flags), "pm_row_info does not carry the PM_ROW_* bits of the result"
    d = first_diff((state & sc.ST_ACCEPTED) != 0, m.accepted)
    assert d is None, "accepted rows: " + d
    d = first_diff(o.info["shift"], m.shift)
    assert d is None, "left trim (shift): " + d
    d = first_diff(o.info["len"], m.len)
    assert d is None, "length: " + d
    d = first_diff(o.info["start0"], o.raw_start[:, 0].astype(np.int64) + np.array(m.shift))
    assert d is None, "start0: " + d
    bad, outside, dirty = ((o.flags & b) != 0 for b in (sc.ROW_BAD, sc.ROW_OUTSIDE, sc.ROW_DIRTY))
    assert np.array_equal((state & sc.ST_BUILT) != 0, ~bad) and np.array_equal((state & sc.ST_OK) != 0, ~bad & ~outside)
    assert np.array_equal((state & sc.ST_FLAGGED) != 0, ~bad & dirty), "PM_ST_FLAGGED is PM_ROW_DIRTY of a constructed row"
    assert not ((state & sc.ST_TANGLED) != 0)[(state & sc.ST_FLAGGED) == 0].any(), "a tangled row that is not flagged"
    for field in o.info.dtype.names:
        assert np.array_equal(o.info[field], o.info_again[field]), "pm_store_info and pm_store_settle differ in " + field
    # floors
    flagged, tangled = (state & sc.ST_FLAGGED) != 0, (state & sc.ST_TANGLED) != 0
    trimmed = (o.info["shift"] != 0) | (o.info["len"] != o.lon)
    assert len(o.lon) >= f["rows"] and flagged.sum() >= f["flagged"] and tangled.sum() >= f["tangled"] and trimmed.sum() >= f["trimmed"], \
        (len(o.lon), int(flagged.sum()), int(tangled.sum()), int(trimmed.sum()))
    assert (flagged & ~tangled).sum() >= f.get("lone", 0), "flagged rows that meet no other flagged row"
    # trims whose marked run crosses a 64-base word of the layout: at the start of a row (img_run_up) in every case, at its end (img_run_down:
    # the row lies before an earlier one of the list, which takes an inversion) where the case says so
    assert m.crossings[0] >= 1 and m.crossings[1] >= f.get("cross_right", 0), m.crossings
    acc = np.array(m.accepted)
    assert (acc & (o.raw_start[:, 0] == 0)).any() and all((acc & (o.raw_start[:, j] + o.lon == o.glen[j])).any() for j in range(len(o.glen))), \
        "no MUM at the very start / the very end of a genome"
    ends = (o.raw_start[:, 0].astype(np.int64) + m.shift + m.len)[acc]
    starts = (o.raw_start[:, 0].astype(np.int64) + m.shift)[acc]
    assert all(((ends & 63) == x).any() or ((starts & 63) == x).any() for x in (63, 0, 1)), "no MUM end on both sides of a word boundary"
    assert ((o.flags & sc.ROW_REVERSE) != 0).sum() >= f.get("reverse", 0)
    assert (acc & ((o.flags & sc.ROW_EARLY) != 0)).sum() >= f.get("early", 0), "accepted rows with PM_ROW_EARLY"
    # the engine marks by atomics instead of StoreMarkOrdered's plain stores when a row that is accepted untrimmed starts before an earlier one ends
    unordered = ((o.flags & sc.ROW_EARLY) != 0) & ((o.flags & (sc.ROW_BAD | sc.ROW_OUTSIDE | sc.ROW_DIRTY)) == 0)
    assert unordered.sum() >= f.get("unordered", 0), "no row that takes the list off the ordered marking path"
    if case.startswith("collinear"):
        assert not unordered.any(), "the collinear list should be marked by StoreMarkOrdered"


def check_layout(lib, case):
    """pm_store_layout after pm_store_settle: the marks of the accepted rows and bit glen[j] of every genome, bit for bit"""
    o = outcome(lib, case)
    same_layout(o.layout, o.model.layout(), "after pm_store_settle")


def check_rows(lib, case):
    """pm_store_rows: raw as the search delivered them, trimmed = raw + shift in every genome, by range and by list"""
    o = outcome(lib, case)
    shift = np.array(o.model.shift, np.int64)[:, None]
    d = first_diff(o.trimmed_start, o.raw_start + shift)
    assert d is None, "trimmed rows by range: " + d
    assert np.array_equal(o.trimmed_strand, o.strand)
    rows, (ts, tf), (rs, rf) = o.listed
    d = first_diff(ts, (o.raw_start + shift)[rows])
    assert d is None, "trimmed rows by list: " + d
    d = first_diff(rs, o.raw_start[rows])
    assert d is None, "raw rows by list: " + d
    assert np.array_equal(tf, o.strand[rows]) and np.array_equal(rf, o.strand[rows])
    assert np.array_equal(o.strand[:, 0], np.ones(len(o.lon), np.uint8)), "the reference member is forward"
    assert np.array_equal((o.flags & sc.ROW_REVERSE) != 0, (o.strand == 0).any(axis=1)), "PM_ROW_REVERSE is a reverse member"


def check_judge(lib, case):
    """pm_store_judge on all consecutive accepted pairs in reference order, with d at the largest gap of the list that d = 300
    takes (a gap of exactly d), at that minus 1, at 0 and at 300: verdict, and min and max gap where there is one"""
    o = outcome(lib, case)
    f = o.floors
    assert not o.tie, "two accepted rows with one reference start: the generator is wrong for this purpose"
    for d, ((mn, mx, v), want) in o.judge.items():
        wv = np.array([w[0] for w in want])
        diff = first_diff(v, wv)
        assert diff is None, "verdicts at d = %d: %s" % (d, diff)
        fw = wv != 2
        diff = first_diff(mn[fw], [w[1] for w in want if w[0] != 2])
        assert diff is None, "min_gap at d = %d: %s" % (d, diff)
        diff = first_diff(mx[fw], [w[2] for w in want if w[0] != 2])
        assert diff is None, "max_gap at d = %d: %s" % (d, diff)
    at = {d: np.array([w[0] for w in o.judge[d][1]]) for d in o.judge}
    assert ((at[o.G] == 0) & (at[o.G - 1] == 1)).sum() >= 1, "no pair with a gap of exactly d"
    assert sum(1 for w in o.judge[300][1] if w[1] == 0) >= 3, "fewer than 3 gaps of exactly 0"
    assert (at[300] == 1).sum() >= 3, "fewer than 3 pairs further apart than d = 300"
    if "verdicts" in f:
        assert all((at[300] == k).sum() >= f["verdicts"] for k in (0, 1, 2)), [int((at[300] == k).sum()) for k in (0, 1, 2)]
    if len(o.glen) > 64:      # a verdict that a genome of the second 64-genome group decides alone
        m = o.model
        late = sum(1 for a, b, w in zip(o.sorted[1:], o.sorted, o.judge[300][1]) if w[0] == 1 and all(0 <= g <= 300 for g in m.gaps(a, b)[:64]))
        assert late >= 1, "no pair that only a genome past the first 64 closes"


def check_fill(lib, case):
    """pm_store_fill on the same pairs: add, and the rows of the fillers that are made (pm_store_fill_starts / _ends hold rows
    only for the pairs with add == 1, one after the other).

    add == 2 (the reference's bookkeeping would overrun, src/parsnp.cpp:2419-2433) cannot be reached with valid rows: FillBetween
    reports it when a genome whose scan does not run (chain end + 1 > genome length, i.e. the MUM ends at the genome's end)
    follows one whose scan did; but a MUM of the next LCB starts at or before genome length - its length in that genome, so
    next start - chain end <= 0 there, and the overlap test, which comes first, answers 0.  The restatement keeps the
    reference's bookkeeping all the same and the checks assert that neither side reports it."""
    o = outcome(lib, case)
    (add, fs, fe), want = o.fill
    wadd = np.array([w[0] for w in want])
    d = first_diff(add, wadd)
    assert d is None, "add: " + d
    made = [w for w in want if w[0] == 1]
    d = first_diff(fs, np.array([w[1] for w in made], np.int64).reshape(len(made), len(o.glen)))
    assert d is None, "filler starts: " + d
    d = first_diff(fe, np.array([w[2] for w in made], np.int64).reshape(len(made), len(o.glen)))
    assert d is None, "filler ends: " + d
    assert (wadd == 0).sum() >= 1 and (wadd == 1).sum() >= 1 and not (wadd == 2).any(), [int((wadd == k).sum()) for k in (0, 1, 2)]
    if len(o.glen) > 64:      # a pair that a genome of the second 64-genome group alone keeps from its filler
        m, lay = o.model, o.model.layout()
        late = sum(1 for a, b, w in zip(o.sorted[1:], o.sorted, want) if w[0] == 0 and m.fill(b, a, lay, range(64))[0] == 1)
        assert late >= 1, "no pair that only a genome past the first 64 decides"


def check_unmark(lib, case):
    """pm_store_unmark of every third accepted row: the layout against the restated marks without them"""
    o = outcome(lib, case)
    m = o.model
    marks = [x.copy() for x in m.marks]
    for c in o.unmarked:
        for j in range(m.n):
            marks[j][m.pos(c, j): m.pos(c, j) + m.len[c]] = False
    assert len(o.unmarked) >= 40
    same_layout(o.layout_unmarked, m.layout(marks), "after pm_store_unmark")


# ------------------------------------------------------------------------------------------------------------------ seeds
def check_settle_seeds(lib, case):
    """pm_store_settle_seeds in a second session: the rows of pm_store_settle, the regions of pm_store_seeds, every field of
    pm_region_info against determineRegion restated base by base, and pm_store_regions_equal on all neighbouring regions and on
    every region with itself against the equality of the restated request rows"""
    name, tune, _ = CASES[case]
    o = outcome(lib, case)
    m = o.model
    with wave_order(case), sc.Store(lib, sequences(name), tune=tune) as st:
        assert np.array_equal(st.raw_start, o.raw_start) and np.array_equal(st.flags, o.flags), "the anchor call is not repeatable"
        info, regs, ids = st.settle_seeds(0)
        for field in info.dtype.names:
            d = first_diff(info[field], o.info[field])
            assert d is None, "pm_store_settle_seeds and pm_store_settle differ in %s: %s" % (field, d)
        same_layout(st.layout(), m.layout(), "after pm_store_settle_seeds")
        seen = {}
        for q, fused in ((0, True), (0, False), (5, False), (-3, False)):      # (-3: every side of every anchor is kept)
            if not fused:
                regs, ids = st.seeds(o.acc, q)
            want = m.seeds(q)
            what = "pm_store_%s at q = %d" % ("settle_seeds" if fused else "seeds", q)
            assert len(regs) == len(want), "%s: %d regions, the restatement keeps %d" % (what, len(regs), len(want))
            for field in sc.REGION_INFO.names:
                d = first_diff(regs[field], [w[0][field] for w in want])
                assert d is None, "%s: %s of the regions: %s" % (what, field, d)
            assert len(set(ids.tolist())) == len(ids), what + ": region ids repeat"
            a = np.concatenate([ids[:-1], ids]).astype(np.int32)
            b = np.concatenate([ids[1:], ids]).astype(np.int32)
            rows = [w[1] for w in want]
            same = [rows[i] == rows[i + 1] for i in range(len(rows) - 1)] + [True] * len(rows)
            d = first_diff(st.regions_equal(a, b), np.array(same, np.uint8))
            assert d is None, what + ": pm_store_regions_equal: " + d
            seen[q] = want
        assert {w[0]["key"] & 1 for w in seen[0]} == {0, 1}, "no kept region on one of the sides at q = 0"
        assert len(seen[-3]) == 2 * len(o.acc) and 0 < len(seen[5]) < len(seen[0]) < len(seen[-3])
        assert any(w[0]["slength"] < w[0]["ref_len"] for w in seen[-3]), "no region whose shortest side is not the reference's"
        if m.n > 64:
            assert any(w[0]["slength"] < min(ln for _, ln in w[1][:64]) for w in seen[-3]), "no region whose shortest side lies past the first 64 genomes"


# ------------------------------------------------------------------------------------------------------------------ chain
def check_chain(lib, case):
    """pm_store_chain_begin / _end in fresh sessions: rows, heads, every counter of pm_chain_info and the layout afterwards, for
    diag_diff 1.0, 0.5, 0.7 and 0.12 and three values of c each -- 0, the restated length of the shortest non-last LCB (`<= c` at
    equality) and that of the median one (about half of the LCBs dissolve, again one of them at equality)"""
    name, tune, _ = CASES[case]
    o = outcome(lib, case)
    m = o.model
    seqs = sequences(name)
    dissolved = survived = fillers = ties = zeros = reverse_joins = 0
    for diag, d in CHAIN_GRID:
        heads = m.chain_pass(o.sorted, d, diag)[0]
        lens = m.lcb_lengths(o.sorted, heads)[:-1]
        assert len(lens) >= 4, "the first pass leaves too few LCBs at diag_diff %g, d %d" % (diag, d)
        reverse_joins += sum(1 for x in range(1, len(heads)) if not heads[x] and (m.flags[o.sorted[x]] | m.flags[o.sorted[x - 1]]) & sc.ROW_REVERSE)
        for c in (0, min(lens), sorted(lens)[len(lens) // 2]):
            what = "chain at diag_diff %g, d %d, c %d" % (diag, d, c)
            want, wrows, wheads, wlay, t = m.chain(d, diag, c)
            with sc.Store(lib, seqs, tune=tune) as st:
                assert np.array_equal(st.raw_start, o.raw_start) and np.array_equal(st.flags, o.flags), "the anchor call is not repeatable"
                rc, info = st.settle()
                assert rc == sc.PM_OK
                got, rows, gheads = st.chain(len(o.acc), d, diag, c)
                lay = st.layout()
            assert got["trouble"] == 0 and want["trouble"] == 0, "%s: trouble %d (restatement %d)" % (what, got["trouble"], want["trouble"])
            assert got == want, "%s: pm_chain_info %s, restatement %s" % (what, got, want)
            diff = first_diff(rows, wrows)
            assert diff is None, "%s: rows: %s" % (what, diff)
            diff = first_diff(gheads, wheads)
            assert diff is None, "%s: heads: %s" % (what, diff)
            same_layout(lay, wlay, what)
            if c:
                assert want["lcbs_dissolved"] >= 1, what + ": nothing dissolves at a c that equals an LCB's length"
            if want["lcbs_dissolved"]:
                dissolved += 1
                survived += want["n_lcbs"] >= 2
            fillers += want["n_fillers"]
            ties += t[0]
            zeros += t[1]
    assert dissolved >= 4 and survived >= 4 and fillers >= 4, (dissolved, survived, fillers)
    assert ties >= 4, "no pair joins with the ratio exactly at 1 - diag_diff"
    assert zeros >= 4, "no pair joins only because a smallest gap of 0 counts as 1"
    if "reverse" in CASES[case][2]:
        assert reverse_joins >= 4, "no pair with a reverse member joins a chain"


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", list(CASES))
def test_settle(lib, case):
    check_settle(lib, case)


@pytest.mark.parametrize("case", list(CASES))
def test_layout(lib, case):
    check_layout(lib, case)


@pytest.mark.parametrize("case", list(CASES))
def test_rows(lib, case):
    check_rows(lib, case)


@pytest.mark.parametrize("case", list(CASES))
def test_judge(lib, case):
    check_judge(lib, case)


@pytest.mark.parametrize("case", list(CASES))
def test_fill(lib, case):
    """add == 2 cannot be reached with valid rows (a chain end at a genome's end makes the overlap test, which comes first, answer 0:
    derived in check_fill's docstring), so the cases hold add == 0 and add == 1 only and assert that neither side reports 2"""
    check_fill(lib, case)


@pytest.mark.parametrize("case", list(CASES))
def test_unmark(lib, case):
    check_unmark(lib, case)


@pytest.mark.parametrize("case", list(CASES))
def test_settle_seeds(lib, case):
    check_settle_seeds(lib, case)


@pytest.mark.parametrize("case", CHAIN_CASES)
def test_chain(lib, case):
    check_chain(lib, case)
