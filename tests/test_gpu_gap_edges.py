"""The designed blocks of tests/gapedges.py on the device, one test per form and topic: every block in a call of its form's entry point
(pm_gap_align_batch for the narrow form, pm_gap_align_groups_wide / _tall / _long for the others), checked by test_gap_edges.run_call:
the reference's recorded rows, the exact decline predicate (cols = -1 exactly where gapedges.taken says so), a sentinel fill of
out_rows intact in every declined job's row area and behind the last row, and the statistics record as the exact numbers the
predicate gives.  The CPU side (the restatement, the generator's floors, the long form in the host emulation) is
tests/test_gap_edges.py; the narrow, the wide and the tall form, and the long blocks of 255 or more sequences, run only here."""
import ctypes as C
import re

import pytest

import gapedges
from parsnp_amd.paths import HIP_LIB
from test_gap_edges import block_call, run_call

pytestmark = pytest.mark.gpu
LDS_LIMIT = 160 * 1024 - 1024      # size_launch's rule (gap_plan.h): fixed + rows + trace-back <= 160 KB - 1 KB


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(HIP_LIB)
    assert hasattr(L, "pm_gap_align_groups_long") and hasattr(L, "pm_gap_align_groups_tall") and hasattr(L, "pm_gap_align_groups_wide")
    return L


def launches(err):
    """the `[gap batch]` launch lines of PARSNP_DEBUG_TIMERS -> [dict(form, jobs, n, cols, slots, rows, tb)]"""
    out = []
    for m in re.finditer(r"\[gap batch\] (?:(wide|tall|long) form: )?(\d+) jobs(?: in \d+ group\(s\))?, widest (\d+) sequences x (\d+) columns: (\d+) B of LDS per \w+"
                         r"(?: of 256 threads)? ?(?:\(rows in (the workspace|LDS), trace-back in (the workspace|LDS)\))?[^\n]*?(\d+) slots", err):
        out.append(dict(form=m.group(1) or "narrow", jobs=int(m.group(2)), n=int(m.group(3)), cols=int(m.group(4)), lds=int(m.group(5)),
                        rows=m.group(6), tb=m.group(7), slots=int(m.group(8))))
    return out


def test_narrow_pairs(lib):
    """every pair of 1, 2, 63, 64, 65, 95, 96 bases in every kind, and the alignments of exactly 64, 65, 96 and 97 columns (the 97s and
    the other pairs that outgrow 96 columns are the declines of this entry point)"""
    st, expect = run_call(lib, block_call("batch", "narrow_pairs"))
    assert expect["narrow"] >= 150 and expect["declined"] >= 3


def test_wide_pairs(lib):
    st, expect = run_call(lib, block_call("wide", "wide_pairs"))
    assert expect["wide"] == len(gapedges.cases("wide_pairs")) and expect["declined"] == 0


def test_long_pairs(lib):
    st, expect = run_call(lib, block_call("long", "long_pairs"))
    assert expect["long"] == len(gapedges.cases("long_pairs")) and expect["declined"] == 0


def test_counts_and_wildcards(lib):
    for entry, form in (("batch", "narrow"), ("wide", "wide"), ("long", "long")):
        st, expect = run_call(lib, block_call(entry, "counts_" + form))
        assert expect[form] == len(gapedges.cases("counts_" + form)) and expect["declined"] == 0


def test_distinct_and_ties(lib):
    for entry, form in (("batch", "narrow"), ("wide", "wide"), ("long", "long")):
        st, expect = run_call(lib, block_call(entry, "distinct_" + form))
        assert expect[form] == len(gapedges.cases("distinct_" + form)) and expect["declined"] == 0
    st, expect = run_call(lib, block_call("long", "long_many"))
    assert expect["long"] == 3


def test_tall(lib):
    """513, 576, 577, 2 047 and 2 048 sequences of 1..3 bases, 2 048 x 320 from two alleles, and 2 049 sequences declined"""
    call = block_call("tall", "tall")
    call = gapedges.Call("tall", call.jobs + [gapedges.Job(gapedges.too_tall(), 8, None, "2 049 sequences")], 0)
    st, expect = run_call(lib, call)
    assert expect["tall"] == len(gapedges.cases("tall")) and expect["declined"] == 1


@pytest.mark.parametrize("form", ["narrow", "wide", "tall", "long"])
def test_capacity_and_declines(lib, form):
    for call in gapedges.capacity_calls(form):
        st, expect = run_call(lib, call)
        assert expect[form] >= 3 and expect["declined"] >= 6


def test_second_wide_run(lib):
    """narrow strings whose alignment outgrows 96 columns: the narrow form declines them, and with max_cols above 96 the wide form
    runs them before the group is reported -- counted as wide jobs"""
    (call,) = gapedges.second_wide_run()
    st, expect = run_call(lib, call)
    assert expect["wide"] >= 4 and expect["narrow"] >= 1 and expect["declined"] >= 3


def test_slot_reuse(lib, monkeypatch, capfd):
    """more tiny jobs than the launch has slots, so that slots take a second job after a taken one, after a late decline (the columns
    are one short: the whole alignment was made) and after an early one (a 'U': nothing was)"""
    monkeypatch.setenv("PARSNP_DEBUG_TIMERS", "1")
    for form, count in (("narrow", 2304), ("wide", 640), ("long", 320)):
        capfd.readouterr()
        st, expect = run_call(lib, gapedges.slot_reuse(form, count))
        line = [x for x in launches(capfd.readouterr().err) if x["form"] == form]
        assert len(line) == 1, form
        device_jobs = count - count // 11      # (the 'U' jobs reach the device: the host declines for sizes only)
        assert line[0]["jobs"] == count and line[0]["jobs"] > line[0]["slots"] >= 64, (form, line)
        assert expect[form] + expect["declined"] == count and expect["declined"] == count // 11 + sum(i % 7 == 6 and i % 11 != 10 for i in range(count)), (form, device_jobs)


def _pick(topic, name, max_cols):
    k = [c.name for c in gapedges.cases(topic)].index(name)
    rows = gapedges.reference_rows(topic)[k]
    assert len(rows[0]) <= max_cols
    return gapedges.Job(gapedges.cases(topic)[k].block, max_cols, rows, name)


def test_wide_placements(lib, monkeypatch, capfd):
    """four launches of the wide form whose widest job puts the rows and the trace-back bytes in each combination of LDS and workspace,
    by size_launch's rule (gap_plan.h) (the fixed block is about 54 KB: n x cap bytes of rows beside it up to 159 KB, then (cap + 1)^2 trace-back
    bytes if they still fit); then the same blocks with PM_GAP_WIDE_PLACE = 1, 2, 3, which force the workspace: same rows"""
    monkeypatch.setenv("PARSNP_DEBUG_TIMERS", "1")
    pairs = [_pick("wide_pairs", "wide 97x127 copy", 200), _pick("wide_pairs", "wide 128x97 straddle0", 180), _pick("wide_pairs", "wide 97x97 unrelated", 199)]
    big = lambda cap: _pick("distinct_wide", "wide count 512", cap)      # noqa: E731
    cases = [("LDS", "LDS", pairs), ("LDS", "the workspace", pairs + [_pick("wide_pairs", "wide 320x320 unrelated", 640)]),
             ("the workspace", "LDS", pairs + [big(220)]), ("the workspace", "the workspace", pairs + [big(640)])]
    assert 2 * 200 + 201 * 201 + 60 * 1024 < LDS_LIMIT < 641 * 641 and 512 * 220 + 50 * 1024 > LDS_LIMIT > 60 * 1024 + 221 * 221
    for rows_in, tb_in, jobs in cases:
        capfd.readouterr()
        run_call(lib, gapedges.Call("wide", jobs, 0))
        line = [x for x in launches(capfd.readouterr().err) if x["form"] == "wide"]
        assert len(line) == 1 and (line[0]["rows"], line[0]["tb"]) == (rows_in, tb_in), (rows_in, tb_in, line)
        assert line[0]["n"] == max(len(j.block) for j in jobs) and line[0]["cols"] == max(j.max_cols for j in jobs)
    for place, want in ((1, ("LDS", "the workspace")), (2, ("the workspace", "LDS")), (3, ("the workspace", "the workspace"))):
        monkeypatch.setenv("PM_GAP_WIDE_PLACE", str(place))
        capfd.readouterr()
        run_call(lib, gapedges.Call("wide", cases[0][2], 0))
        line = [x for x in launches(capfd.readouterr().err) if x["form"] == "wide"]
        assert len(line) == 1 and (line[0]["rows"], line[0]["tb"]) == want, (place, line)
        run_call(lib, gapedges.Call("wide", cases[3][2], 0))
        capfd.readouterr()
    monkeypatch.delenv("PM_GAP_WIDE_PLACE")
