"""The host side of the device gap aligner that needs no device (parsnp_amd/csrc/engine/gap_plan.h: the table of the five forms,
plan_jobs, size_launch) as a stand-alone program under AddressSanitizer and UBSan (tests/emu/gap_plan_check.cpp, its own main):
which jobs a call takes, the form each goes to and the order of the launches against a restatement in a few lines, on batches made
of the edge values of every limit; the geometry of a launch against numbers worked out by hand, and at the points where the rows
or the trace-back bytes stop fitting the LDS.  A CPU program: no GPU, nothing loaded into python."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "emu", "gap_plan_check_asan")
NARROW, WIDE, TALL, LONG, LONG_TALL = range(5)
# per entry point: most sequences, most bases, narrow_only
RECTS = {"batch": (512, 96, 1), "wide": (512, 320, 0), "tall": (2048, 320, 0), "long": (512, 1024, 0), "long_tall": (2048, 1024, 0)}
CUS = 256


@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "emu", "gap_plan_check.cpp")
    deps = [src, os.path.join(ROOT, "parsnp_amd", "csrc", "engine", "gap_plan.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", src, "-o", BIN], check=True)
    return BIN


def run(checker, tmp_path, commands):
    """the program's answers to a list of commands (each a list of numbers behind its name)"""
    path = str(tmp_path / "commands.txt")
    with open(path, "w") as f:
        for c in commands:
            f.write(" ".join(str(x) for x in c) + "\n")
    p = subprocess.run([checker, path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = [json.loads(line) for line in p.stdout.splitlines()]
    assert len(out) == len(commands)
    return out


@pytest.fixture(scope="module")
def table(checker, tmp_path_factory):
    return run(checker, tmp_path_factory.mktemp("table"), [["table"]])[0]


# ---- routing and ordering

def edge_jobs():
    """(lengths, max_cols) of one job per pair of edge values, the widest string somewhere in the job, in a shuffled order; then a job
    with one empty string, one with max_cols = 0, and two small ones the last of which decides whether the row areas fit"""
    jobs = []
    k = 0
    for n in (1, 2, 512, 513, 2048, 2049):
        for w in (1, 96, 97, 320, 321, 1024, 1025):
            lens = [1 + (7 * i + k) % w for i in range(n)]
            lens[(5 * k) % n] = w
            jobs.append((lens, (1, 95, 96, 97, 640, 641, 2048, 3000)[k % 8]))
            k += 1
    order = sorted(range(len(jobs)), key=lambda i: (i * 29) % 43)
    jobs = [jobs[i] for i in order]
    jobs.insert(11, ([5, 0, 7], 16))
    jobs.insert(23, ([40, 41], 0))
    return jobs + [([3, 4], 8), ([90, 96, 3], 120)]


def form_of(n, w):
    return {(False, False, False): NARROW, (False, False, True): WIDE, (False, True, True): LONG, (True, False, False): TALL, (True, False, True): TALL,
            (True, True, True): LONG_TALL}[(n > 512, w > 320, w > 96)]


def restated(rect, jobs, row_off, out_bytes, group_end):
    """plan_jobs in a few lines -> (jobs [first_seq, n, max_cols, row_off] in launch order, which, first, nmax, cap)"""
    seqs, length, _ = rect
    taken, seq, g = [], 0, 0
    nmax, cap = 2, 1
    for j, ((lens, mc), ro) in enumerate(zip(jobs, row_off)):
        while g + 1 < len(group_end) and j >= group_end[g]:
            g += 1
        n = len(lens)
        if 2 <= n <= seqs and all(1 <= x <= length for x in lens) and mc >= 1 and ro + n * mc <= out_bytes:
            form = form_of(n, max(lens))
            taken.append((g, form, -max(lens), j, [seq, n, mc, ro]))
            if form == NARROW:
                nmax, cap = max(nmax, n), max(cap, min(mc, 96))
        seq += n
    taken.sort(key=lambda t: t[:3])      # (stable)
    first = [0] * (5 * len(group_end) + 1)
    for t in taken:
        first[5 * t[0] + t[1] + 1] += 1
    for i in range(1, len(first)):
        first[i] += first[i - 1]
    return [t[4] for t in taken], [t[3] for t in taken], first, nmax, cap, seq


@pytest.mark.parametrize("short_by", [0, 1])
def test_plans_equal_the_restatement(checker, tmp_path, short_by):
    """every rectangle x 1, 2 and 3 groups (one of them empty) on the edge batch; short_by = 1: the row area of the last job ends one
    byte behind out_bytes"""
    jobs = edge_jobs()
    row_off, at = [], 0
    for lens, mc in jobs:
        row_off.append(at)
        at += len(lens) * mc
    out_bytes = at - short_by
    nj = len(jobs)
    groupings = [[nj], [0, nj], [17, 17, nj]]
    text = []
    for (lens, mc), ro in zip(jobs, row_off):
        text += [len(lens), mc, ro] + lens
    cases = [(name, ge) for name in RECTS for ge in groupings]
    got = run(checker, tmp_path, [["plan", *RECTS[name], out_bytes, len(ge), *ge, nj] + text for name, ge in cases])
    seen = set()
    for (name, ge), g in zip(cases, got):
        want_jobs, which, first, nmax, cap, seq = restated(RECTS[name], jobs, row_off, out_bytes, ge)
        assert g["error"] is None
        assert g["which"] == which and g["jobs"] == want_jobs and g["first"] == first, (name, ge)
        assert (g["nmax"], g["cap"], g["seqs"]) == (nmax, cap, seq), (name, ge)
        assert g["cols"] == [-1] * nj
        assert (nj - 1 in which) == (short_by == 0), "the last job's rows fit exactly, or are one byte short"
        seen |= {form_of(j[1], max(jobs[w][0])) for j, w in zip(want_jobs, which)}
        if name == "long_tall" and len(ge) == 3:      # the floor under the restatement: every form in both full groups, the jobs at a limit in
            assert all(first[5 * grp + f + 1] > first[5 * grp + f] for grp in (0, 2) for f in range(5)) and first[5] == first[10]
            sizes = {(j[1], max(jobs[w][0])) for j, w in zip(want_jobs, which)}
            assert {(2, 1), (512, 96), (512, 97), (512, 320), (512, 321), (512, 1024), (513, 320), (2048, 320), (513, 321), (2048, 1024)} <= sizes
            assert not {s for s in sizes if s[0] in (1, 2049) or s[1] == 1025}
    assert seen == {NARROW, WIDE, TALL, LONG, LONG_TALL}


def test_refused_arguments(checker, tmp_path):
    one = [2, 8, 0, 3, 4]      # a job of two strings
    got = run(checker, tmp_path, [["plan", 512, 96, 1, 16, 0, 1] + one, ["plan", 512, 96, 1, 16, 1, 2, 1] + one, ["plan", 512, 96, 1, 16, 2, 1, 0, 2] + one + one,
                                  ["plan", 512, 96, 1, 16, 2, 2, 1, 1] + one, ["plan", 512, 96, 1, 16, 1, 0, 0], ["plan", 512, 96, 1, 16, 1, 1, 1] + one])
    assert [g["error"] for g in got] == ["bad job groups"] * 4 + [None, None]
    assert got[4]["jobs"] == [] and got[4]["first"] == [0] * 6
    assert got[5]["jobs"] == [[0, 2, 8, 0]] and got[5]["first"] == [0, 1, 1, 1, 1, 1]


# ---- geometry

def r16(b):
    return (b + 15) & ~15


def slot_bytes(n, cap, seq, rows, tb):
    """what a slot's workspace holds (carve() in gapalign_hip.hip), array by array"""
    arrays = [4 * (n * (n - 1) // 2 + 1), 2 * n * n, 2 * n * seq, n * seq, 4 * n, 8 * n] + [4 * n] * 4 + [8 * n] * 3 + [16 * n, 4 * n, 8 * n, 16 * n, 4 * n, 8 * n, 8 * n, 4 * n, 8 * n, 46656]
    return sum(r16(a) for a in arrays) + (r16(n * cap) if rows else 0) + (r16((cap + 1) ** 2) if tb else 0) + 256


def size(checker, tmp_path, form, n_jobs, place, given, cus=CUS):
    flat = [x for j in given for x in j]
    return run(checker, tmp_path, [["size", form, n_jobs, cus, place, len(given)] + flat])[0]


def test_the_table(table):
    rows = table["forms"]
    assert [r["name"] for r in rows] == ["", "wide", "tall", "long", "long-tall"]
    assert [(r["seqs"], r["seq"], r["cols"]) for r in rows] == [(512, 96, 96), (512, 320, 640), (2048, 320, 640), (512, 1024, 2048), (2048, 1024, 2048)]
    assert [r["threads"] for r in rows] == [64, 64, 64, 256, 256]
    assert [r["ws_cap"] for r in rows] == [0, 0, 8 << 30, 8 << 30, 8 << 30]
    assert [r["counter"] for r in rows] == [0, 1, 3, 4, 5] and table["wide_again"] == 2 and table["counters"] == 6
    assert all(r["fixed"] % 16 == 0 and r["fixed"] <= table["lds_limit"] for r in rows) and table["lds_limit"] == 160 * 1024 - 1024


def test_one_launch_per_form_by_hand(checker, tmp_path, table):
    """at 256 CUs.  The widest job is the maximum over the jobs given, the columns cut at the form's"""
    fixed = [r["fixed"] for r in table["forms"]]
    # narrow: 30 x 96 -> rows 2 880 B, trace-back 97^2 = 9 409 -> 9 424 B behind the fixed block; 160 KB / (that + 256) per CU
    g = size(checker, tmp_path, NARROW, 5000, 3, [(30, 200), (7, 50)])
    lds = fixed[NARROW] + 2880 + 9424
    assert g == dict(wn=30, wc=96, lds=lds, dyn=2880 + 9424, rows_ws=0, tb_ws=0, fits=1, per_cu=min(8, 163840 // (lds + 256)), slots=min(5000, CUS * min(8, 163840 // (lds + 256))),
                     stride=slot_bytes(30, 96, 96, False, False))
    assert fixed[NARROW] == 15040 and g["per_cu"] == 5 and g["slots"] == 1280 and g["stride"] == 63008
    # wide: 12 x 300 -> rows 3 600 B, trace-back 301^2 = 90 601 -> 90 608 B: both beside the 54 480 B of the fixed block, one per CU
    g = size(checker, tmp_path, WIDE, 90, 0, [(12, 300), (3, 280)])
    assert fixed[WIDE] == 54480
    assert g == dict(wn=12, wc=300, lds=54480 + 3600 + 90608, dyn=54480 + 3600 + 90608, rows_ws=0, tb_ws=0, fits=1, per_cu=1, slots=90, stride=slot_bytes(12, 300, 320, False, False))
    assert g["stride"] == 60528
    # tall: 600 x 640 -> neither fits: the fixed block alone, two per CU
    g = size(checker, tmp_path, TALL, 40, 0, [(600, 900)])
    assert g == dict(wn=600, wc=640, lds=fixed[TALL], dyn=fixed[TALL], rows_ws=1, tb_ws=1, fits=1, per_cu=2, slots=40, stride=slot_bytes(600, 640, 320, True, True))
    # long forms: a workgroup per CU, everything in the workspace, and the six sums of 2 048 columns behind it
    g = size(checker, tmp_path, LONG, 1000, 0, [(100, 1800), (500, 3000)])
    assert g == dict(wn=500, wc=2048, lds=fixed[LONG], dyn=fixed[LONG], rows_ws=1, tb_ws=1, fits=1, per_cu=1, slots=256, stride=slot_bytes(500, 2048, 1024, True, True) + 6 * 4 * 2048)
    g = size(checker, tmp_path, LONG_TALL, 3, 0, [(2048, 2048)])
    assert g == dict(wn=2048, wc=2048, lds=fixed[LONG_TALL], dyn=fixed[LONG_TALL], rows_ws=1, tb_ws=1, fits=1, per_cu=1, slots=3, stride=slot_bytes(2048, 2048, 1024, True, True) + 6 * 4 * 2048)
    assert 31e6 < g["stride"] < 32e6      # (the 31 MB of the source's comment)


def test_where_the_placement_flips(checker, tmp_path, table):
    fixed, limit = table["forms"][WIDE]["fixed"], table["lds_limit"]
    # the rows: 640 columns, as many sequences as just fit beside the fixed block, then one more
    wn = (limit - fixed) // 640
    a, b = size(checker, tmp_path, WIDE, 9, 0, [(wn, 640)]), size(checker, tmp_path, WIDE, 9, 0, [(wn + 1, 640)])
    assert fixed + wn * 640 <= limit < fixed + (wn + 1) * 640
    assert (a["rows_ws"], a["tb_ws"], a["lds"]) == (0, 1, fixed + wn * 640) and (b["rows_ws"], b["tb_ws"], b["lds"]) == (1, 1, fixed)
    assert a["stride"] == slot_bytes(wn, 640, 320, False, True) and b["stride"] == slot_bytes(wn + 1, 640, 320, True, True)
    # the trace-back bytes of two sequences: the widest that fits beside the fixed block and the rows, then a column more
    need = lambda wc: fixed + r16(2 * wc) + r16((wc + 1) ** 2)      # noqa: E731
    wc = max(c for c in range(1, 641) if need(c) <= limit)
    assert wc < 640
    a, b = size(checker, tmp_path, WIDE, 9, 0, [(2, wc)]), size(checker, tmp_path, WIDE, 9, 0, [(2, wc + 1)])
    assert (a["rows_ws"], a["tb_ws"], a["lds"]) == (0, 0, need(wc)) and (b["rows_ws"], b["tb_ws"], b["lds"]) == (0, 1, fixed + r16(2 * (wc + 1)))
    # the narrow form has nowhere else to put them: it is refused
    nfixed = table["forms"][NARROW]["fixed"]
    wn = (limit - nfixed - r16(97 * 97)) // 96
    assert size(checker, tmp_path, NARROW, 9, 0, [(wn, 96)])["fits"] == 1 and size(checker, tmp_path, NARROW, 9, 0, [(wn + 1, 96)])["fits"] == 0
    # PM_GAP_WIDE_PLACE on a launch where both fit
    for place, rows_ws, tb_ws in ((1, 0, 1), (2, 1, 0), (3, 1, 1)):
        g = size(checker, tmp_path, WIDE, 9, place, [(4, 100)])
        assert (g["rows_ws"], g["tb_ws"]) == (rows_ws, tb_ws)
        assert g["lds"] == fixed + (0 if rows_ws else 400) + (0 if tb_ws else r16(101 * 101)) and g["stride"] == slot_bytes(4, 100, 320, bool(rows_ws), bool(tb_ws))
        assert g["per_cu"] == min(8, 163840 // (g["lds"] + 256))
    # a tall launch of more jobs than 8 GB of workspace have slots for
    stride = slot_bytes(2048, 640, 320, True, True)
    g = size(checker, tmp_path, TALL, 1000, 0, [(2048, 640)])
    assert g["stride"] == stride and g["per_cu"] == 2 and g["slots"] == (8 << 30) // stride < 2 * CUS
    assert 20e6 < stride < 21e6      # (the 20 MB of the source's comment)
