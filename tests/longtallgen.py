"""Seeded inputs for the long-tall form of the gap aligner: gaps of 513 to 2 048 sequences with a string of 321 to 1 024 bases, what
an alignment of more than 511 query genomes run with a raised cluster distance d (up to 1 000) leaves between adjacent MUMs, and the
synthetic genome set whose windows make the whole pipeline meet them at d = 1000.  The reference's rows of the blocks are recorded
in tests/golden/muscle_long_tall_runs.json.xz, its whole run in tests/golden/long_tall_gap_runs.json.xz
(tests/golden/make_long_tall_gap_runs.py).  The family is small and cheap on purpose: a block of more than 50 sequences draws from
24 haplotypes unless its purpose is the number of DISTINCT strings."""
import collections
import os
import random

import gapgen
import widegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUSCLE_LONG_TALL_GOLDEN = os.path.join(ROOT, "tests", "golden", "muscle_long_tall_runs.json.xz")
LONG_TALL_RUNS_GOLDEN = os.path.join(ROOT, "tests", "golden", "long_tall_gap_runs.json.xz")
# the limits of the device's long-tall form as include/parsnp_mum.h documents them; the tests read them from pm_gap_limits_long_tall
# and check that they are these
LT_SEQS, LT_SEQ_LEN, LT_COLS = 2048, 1024, 2048
OLD_SEQS, OLD_SEQ_LEN = 512, 320      # beyond both at once: the long-tall form
CLUSTER_D = 1000
HAPLOTYPES = 24
SENTINEL = 0xEE

Case = collections.namedtuple("Case", "name block")


def _distinct_short(rng, count, lo, hi):
    """`count` distinct strings of lo .. hi bases, the first of lo and the second of hi bases"""
    seen, out = set(), []
    while len(out) < count:
        length = lo if not out else (hi if len(out) == 1 else rng.randint(max(lo, 5), hi))
        s = widegen._string(rng, length, "ACGT")
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def _haplotypes(rng, n, length, rate, jitter=0):
    """n strings drawn from HAPLOTYPES diverged copies of one string of `length` bases (the first HAPLOTYPES are the copies)"""
    base = widegen._string(rng, length, "ACGT")
    haps = [gapgen.mutate(rng, base, rate, "ACGT")[:LT_SEQ_LEN] for _ in range(HAPLOTYPES)]
    return [haps[i] if i < HAPLOTYPES else haps[rng.randrange(HAPLOTYPES)] for i in range(n)]


def long_tall_blocks():
    """the family, every block beyond 512 sequences AND 320 bases and inside 2 048 x 1 024:
      first         513 sequences: one string of 321 bases and 512 distinct strings of 1 to 40 bases -- the first job beyond both older
                    limits, about 512 cheap pairwise steps
      rounds 576 / 577 / 640   one string of 400 bases, the rest from 24 haplotypes of 5 to 40 bases: a boundary of the merge's rounds
                    of 64 sequences and of the 256-thread loops
      distinct 700  700 distinct strings of 330 to 360 bases, diverged copies at 0.1 (more than 512 distinct strings: the common-count
                    and distance tables beyond the long form's range)
      far corner    2 048 sequences: one string of 1 024 bases, the rest from 24 haplotypes of about 1 000 bases at divergence 0.05
      whole run     2 001 sequences of about 900 bases from 24 haplotypes at divergence 0.1: the shape longtall600x60k-like runs produce"""
    rng = random.Random(20261020)
    out = []
    first = [widegen._string(rng, OLD_SEQ_LEN + 1, "ACGT")] + _distinct_short(rng, 512, 1, 40)
    out.append(Case("first", first))
    for n in (576, 577, 640):
        haps = [widegen._string(rng, rng.randint(5, 40), "ACGT") for _ in range(HAPLOTYPES)]
        blk = [haps[i] if i < HAPLOTYPES else haps[rng.randrange(HAPLOTYPES)] for i in range(n - 1)]
        blk.insert(rng.randrange(n), widegen._string(rng, 400, "ACGT"))
        out.append(Case("rounds %d" % n, blk))
    base = widegen._string(rng, 345, "ACGT")
    seen, many = set(), []
    while len(many) < 700:
        s = gapgen.mutate(rng, base, 0.1, "ACGT")[:rng.randint(330, 360)]
        if len(s) >= 330 and s not in seen:
            seen.add(s)
            many.append(s)
    out.append(Case("distinct 700", many))
    far = _haplotypes(rng, LT_SEQS - 1, 1000, 0.05)
    far.insert(1000, widegen._string(rng, LT_SEQ_LEN, "ACGT")[:24] + gapgen.mutate(rng, far[0], 0.05, "ACGT").ljust(LT_SEQ_LEN, "A")[24:LT_SEQ_LEN])
    out.append(Case("far corner", far))
    out.append(Case("whole run", _haplotypes(rng, 2001, 900, 0.1)))
    return out


def reference_align(blks):
    """the reference's MuscleInterface on every block (oracle/_ref/muscle_ref), from its record"""
    return widegen.reference_align(blks, golden=MUSCLE_LONG_TALL_GOLDEN)


_rows = {}


def family():
    """-> (the cases, the reference's rows of each)"""
    if "rows" not in _rows:
        cs = long_tall_blocks()
        _rows["cases"], _rows["rows"] = cs, reference_align([c.block for c in cs])
    return _rows["cases"], _rows["rows"]


# ---- calls, the exact decline predicate and the check of a whole call

Job = collections.namedtuple("Job", "block max_cols rows why")      # rows: the reference's (None where it is not needed)


def capacity(block):
    """the writer's row capacity of a long gap: 1.75 x the longest string + 16, capped at the columns of the form"""
    m = max(len(s) for s in block)
    return min(LT_COLS, m + (3 * m) // 4 + 16)


def taken(block, max_cols, ref_cols, row_off, out_bytes):
    """(taken, reason) at pm_gap_align_groups_long_tall: the job is aligned if and only if 2 <= n <= 2 048, every length in 1 .. 1 024,
    row_off + n * max_cols <= out_bytes, upper case without 'U', and the reference's column count <= min(max_cols, 2 048) (progressive
    alignment never removes a column: no intermediate alignment is wider than the final one).  ref_cols: a callable, asked last."""
    n = len(block)
    if not 2 <= n <= LT_SEQS or max_cols < 1:
        return False, "n"
    if not all(1 <= len(s) <= LT_SEQ_LEN for s in block):
        return False, "len"
    if row_off + n * max_cols > out_bytes:
        return False, "out_bytes"
    if any(ch.islower() or ch == "U" for s in block for ch in s):
        return False, "alphabet"
    if ref_cols() > min(max_cols, LT_COLS):
        return False, "cols"
    return True, None


def decline_jobs():
    """the declines, on the cheap blocks: 2 049 sequences; a 1 025-base string among 600; max_cols one short of the reference's columns;
    max_cols exactly the reference's columns (taken); a 'U' as the last character; and a last job that out_bytes one byte short declines
    (and that is taken with out_bytes exact)"""
    cs, rows = family()
    first, first_rows = cs[0].block, rows[0]
    r576, r576_rows = cs[1].block, rows[1]
    c = len(first_rows[0])
    return [Job([first[1]] * (LT_SEQS + 1), 48, None, "2 049 sequences"),
            Job([r576[i % len(r576)] for i in range(599)] + ["A" * (LT_SEQ_LEN + 1)], 2 * LT_SEQ_LEN, None, "a 1 025-base string among 600"),
            Job(first, c - 1, first_rows, "max_cols one short"),
            Job(first, c, first_rows, "max_cols exact"),
            Job(first[:-1] + [first[-1][:-1] + "U"], c + 4, None, "U last"),
            Job(r576, len(r576_rows[0]) + 2, r576_rows, "last job")]


def form_of(block, cols):
    n, w = len(block), max(len(s) for s in block)
    if n > OLD_SEQS:
        return "long_tall" if w > OLD_SEQ_LEN else "tall"
    return "long" if w > OLD_SEQ_LEN else ("wide" if w > 96 or cols > 96 else "narrow")


def run_call(L, jobs, short_by=0, stats_type=None):
    """one call of pm_gap_align_groups_long_tall on the library L, checked in full as tests/test_gap_edges.run_call does: the
    reference's rows and column count for every job the predicate takes, cols = -1 for every other, the sentinel bytes intact in the
    row area of every declined job and behind the last area, the statistics as the predicate gives them -> (statistics, expected)"""
    import ctypes as C

    import numpy as np
    nseq = np.array([len(j.block) for j in jobs], np.int32)
    flat = [s.encode() for j in jobs for s in j.block]
    off = np.zeros(len(flat) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in flat])
    chars = np.frombuffer(b"".join(flat) or b"\0", np.uint8).copy()
    maxc = np.array([j.max_cols for j in jobs], np.int32)
    ro = np.zeros(len(jobs), np.int64)
    ro[1:] = np.cumsum(nseq[:-1].astype(np.int64) * maxc[:-1])
    total = int((nseq.astype(np.int64) * maxc).sum())
    out_bytes = total - short_by
    verdict = [taken(j.block, j.max_cols, (lambda j=j: len(j.rows[0])), int(r), out_bytes) for j, r in zip(jobs, ro)]
    out = np.full(total + 64, SENTINEL, np.uint8)
    cols = np.full(len(jobs), -7, np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    st = (stats_type or LongTallStats)()
    ge = np.array([len(jobs)], np.int64)
    L.pm_gap_last_error.restype = C.c_char_p
    L.pm_gap_align_groups_long_tall.restype = C.c_int
    rc = L.pm_gap_align_groups_long_tall(C.c_int(-1), C.c_int64(len(jobs)), p(nseq, C.c_int32), p(off, C.c_int64), p(chars, C.c_uint8), p(maxc, C.c_int32),
                                         p(ro, C.c_int64), p(out, C.c_uint8), C.c_int64(out_bytes), p(cols, C.c_int32), C.c_int(1), p(ge, C.c_int64), None, None, C.byref(st))
    assert rc == 0, L.pm_gap_last_error()
    expect = dict(narrow=0, wide=0, tall=0, long=0, long_tall=0, declined=0)
    for k, (j, (ok, why)) in enumerate(zip(jobs, verdict)):
        base, w, n = int(ro[k]), j.max_cols, len(j.block)
        area = out[base: base + n * w]
        if ok:
            want = j.rows
            assert cols[k] == len(want[0]), (k, j.why, int(cols[k]), len(want[0]))
            got = [area[i * w: i * w + len(want[0])].tobytes().decode() for i in range(n)]
            assert got == want, (k, j.why)
            expect[form_of(j.block, len(want[0]))] += 1
        else:
            assert cols[k] == -1, (k, j.why, why, int(cols[k]))
            assert (area == SENTINEL).all(), "the row area of declined job %d (%s: %s) was written" % (k, j.why, why)
            expect["declined"] += 1
    assert (out[total:] == SENTINEL).all(), "bytes behind the last row were written"
    assert (st.jobs_narrow, st.jobs_wide, st.jobs_tall, st.jobs_long, st.jobs_long_tall, st.declined) == \
        tuple(expect[k] for k in ("narrow", "wide", "tall", "long", "long_tall", "declined")), expect
    return st, expect


def _stats_type():
    import ctypes as C

    class LongTallStats(C.Structure):
        _fields_ = [("jobs_narrow", C.c_int64), ("jobs_wide", C.c_int64), ("jobs_tall", C.c_int64), ("jobs_long", C.c_int64), ("jobs_long_tall", C.c_int64),
                    ("declined", C.c_int64), ("ms_narrow", C.c_double), ("ms_wide", C.c_double), ("ms_tall", C.c_double), ("ms_long", C.c_double),
                    ("ms_long_tall", C.c_double)]
    return LongTallStats


LongTallStats = _stats_type()


def long_tall_run(core, name, tmp_path, env=None, threads=16, clusterd=CLUSTER_D, reference="record"):
    """the set `name` of parsnp_amd.synth through `core` with the cluster distance `clusterd`: checked against the reference binary's
    record (reference = "record") or not at all (reference = None) -> (the run's result, its PARSNP_TIMING record)"""
    import json

    import refruns
    from parsnp_amd import synth
    ref, gs = synth.make(name)
    rp, qs = synth.write_set(str(tmp_path / "in"), ref, gs)
    kw = dict(threads=threads, clusterd=clusterd)
    if reference == "record":
        want = refruns.recorded(LONG_TALL_RUNS_GOLDEN, refruns.case_key(widegen.run_core, rp, qs, kw), refruns.REFBIN,
                                lambda: widegen.run_core(refruns.REFBIN, rp, qs, str(tmp_path / "ref"), kw))
    timing = str(tmp_path / "timing.json")
    got = refruns.normal(widegen.run_core(core, rp, qs, str(tmp_path / "mine"), kw, env=dict(os.environ if env is None else env, PARSNP_TIMING=timing)))
    assert got[0] == 0, got
    if reference == "record":
        assert got == want, name
    return got, json.load(open(timing))
