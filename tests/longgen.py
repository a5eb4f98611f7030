"""Seeded inputs for the long form of the gap aligner: gap strings of 321 to 1 024 bases, what a cluster distance d above the
reference driver's default 300 (up to 1 000) leaves between adjacent MUMs, and the two synthetic genome sets whose windows of 330
to 900 bases make the whole pipeline meet them when it is run with d = 1000.  The reference's rows of the blocks are recorded in
tests/golden/muscle_long_runs.json.xz, its whole runs in tests/golden/long_gap_runs.json.xz (tests/golden/make_long_gap_runs.py)."""
import os
import random

import gapgen
import widegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUSCLE_LONG_GOLDEN = os.path.join(ROOT, "tests", "golden", "muscle_long_runs.json.xz")
LONG_RUNS_GOLDEN = os.path.join(ROOT, "tests", "golden", "long_gap_runs.json.xz")
# the limits of the device's long form as include/parsnp_mum.h documents them; the tests read them from pm_gap_limits_long and
# check that they are these
LONG_SEQS, LONG_SEQ_LEN, LONG_COLS = 512, 1024, 2048
CLUSTER_D = 1000      # the d= of the whole runs


def _family(rng, n, length, rate, alpha, mode, haplotypes=24):
    """the three models of widegen._family at any length: own copies, a few shared haplotypes, unrelated strings of nearly `length`"""
    base = widegen._string(rng, length, alpha)
    seqs = []
    for i in range(n):
        if mode == "copies":
            seqs.append(gapgen.mutate(rng, base, rate, alpha))
        elif mode == "haplotypes":
            seqs.append(gapgen.mutate(rng, base, rate, alpha) if i < haplotypes else seqs[rng.randrange(haplotypes)])
        else:
            seqs.append(widegen._string(rng, rng.randint(length - 24, length), alpha))
    seqs = [s[:LONG_SEQ_LEN] for s in seqs]
    if max(len(s) for s in seqs) <= widegen.WIDE_SEQ_LEN:      # every block of the family is a long one
        seqs[0] = (seqs[0] + widegen._string(rng, widegen.WIDE_SEQ_LEN + 1, alpha))[:widegen.WIDE_SEQ_LEN + 1]
    return seqs


def long_blocks():
    """the family: 2 to 512 sequences whose longest string has 321 to 1 024 bases, at divergence 0.02 to 0.6 over ACGT and ACGTN, as
    diverged copies, shared haplotypes and unrelated strings.  Block 0 is 2 x 321, block 1 has every string at 1 024 bases, one block
    has 512 sequences, one 200 of about 900 bases, and the 40 unrelated strings of about 1 024 bases align to more than 1 700
    columns.  All lie inside the long form's limits.  The blocks of more than 50 sequences draw from 24 haplotypes."""
    rng = random.Random(20261018)
    out = [[s.ljust(321, "A")[:321] for s in _family(rng, 2, 321, 0.3, "ACGT", "copies")],
           [s.ljust(LONG_SEQ_LEN, "A")[:LONG_SEQ_LEN] for s in _family(rng, 6, LONG_SEQ_LEN, 0.1, "ACGT", "copies")]]
    for n, length, rate, alpha, mode in [
            (2, 1024, 0.3, "ACGT", "copies"), (3, 700, 0.6, "ACGTN", "copies"), (5, 500, 0.3, "ACGTN", "copies"), (8, 1024, 0.6, "ACGT", "copies"),
            (12, 1000, 0.1, "ACGT", "copies"), (12, 900, 0.3, "ACGT", "copies"), (20, 700, 0.0, "ACGT", "unrelated"), (30, 400, 0.1, "ACGTN", "haplotypes"),
            (40, 1024, 0.0, "ACGT", "unrelated"), (50, 350, 0.02, "ACGT", "copies"), (50, 600, 0.25, "ACGT", "copies"),
            (100, 800, 0.1, "ACGTN", "haplotypes"), (200, 900, 0.1, "ACGT", "haplotypes"), (512, 400, 0.05, "ACGT", "haplotypes")]:
        out.append(_family(rng, n, length, rate, alpha, mode))
    return out


def reference_align(blks):
    """the reference's MuscleInterface on every block (oracle/_ref/muscle_ref), from its record"""
    return widegen.reference_align(blks, golden=MUSCLE_LONG_GOLDEN)


def long_run(core, name, tmp_path, env=None, threads=8, clusterd=CLUSTER_D, reference="record"):
    """the set `name` of parsnp_amd.synth through `core` with the cluster distance `clusterd`: checked against the reference binary's
    record (reference = "record") or not at all (reference = None) -> (the run's result, its PARSNP_TIMING record)"""
    import json
    import refruns
    from parsnp_amd import synth
    ref, gs = synth.make(name)
    rp, qs = synth.write_set(str(tmp_path / "in"), ref, gs)
    kw = dict(threads=threads, clusterd=clusterd)
    if reference == "record":
        want = refruns.recorded(LONG_RUNS_GOLDEN, refruns.case_key(widegen.run_core, rp, qs, kw), refruns.REFBIN,
                                lambda: widegen.run_core(refruns.REFBIN, rp, qs, str(tmp_path / "ref"), kw))
    timing = str(tmp_path / "timing.json")
    got = refruns.normal(widegen.run_core(core, rp, qs, str(tmp_path / "mine"), kw, env=dict(os.environ if env is None else env, PARSNP_TIMING=timing)))
    assert got[0] == 0, got
    if reference == "record":
        assert got == want, name
    return got, json.load(open(timing))
