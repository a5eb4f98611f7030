"""Seeded inputs for the tall form of the gap aligner: gaps of alignments with 513 to 2 048 genomes (one string per genome), and
the two synthetic genome sets that make the whole pipeline meet them.  The reference's rows of the blocks are recorded in
tests/golden/muscle_tall_runs.json.xz, its whole runs in tests/golden/tall_gap_runs.json.xz (tests/golden/make_tall_gap_runs.py)."""
import os
import random

import gapgen
import widegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUSCLE_TALL_GOLDEN = os.path.join(ROOT, "tests", "golden", "muscle_tall_runs.json.xz")
TALL_RUNS_GOLDEN = os.path.join(ROOT, "tests", "golden", "tall_gap_runs.json.xz")
# the limits of the device's tall form as include/parsnp_mum.h documents them; the GPU tests read them from pm_gap_limits_tall
# and check that they are these
TALL_SEQS, TALL_SEQ_LEN, TALL_COLS = 2048, 320, 640
TALL_SIZES = (513, 601, 1001, 2001, 2048)
OUTGROWS = 3      # the block of tall_blocks() whose strings have at most 96 bases and whose alignment has more than 96 columns


def _family(rng, n, length, rate, alpha, mode, haplotypes=24):
    """the three models of widegen._family at any length: own copies, a few shared haplotypes, unrelated strings"""
    base = widegen._string(rng, length, alpha)
    seqs = []
    for i in range(n):
        if mode == "copies":
            seqs.append(gapgen.mutate(rng, base, rate, alpha))
        elif mode == "haplotypes":
            seqs.append(gapgen.mutate(rng, base, rate, alpha) if i < haplotypes else seqs[rng.randrange(haplotypes)])
        else:
            seqs.append(widegen._string(rng, rng.randint(1, length), alpha))
    return [s[:TALL_SEQ_LEN] for s in seqs]


def tall_blocks():
    """the family: 513, 601, 1 001, 2 001 and 2 048 sequences; strings of 1 to 90 bases and a few of 97 to 320; diverged copies,
    shared haplotypes and unrelated strings over ACGT and ACGTN; one block whose alignment outgrows 96 columns from strings of at
    most 96 bases (index OUTGROWS) and one of 2 048 sequences of 320 bases each.  All lie inside the tall form's limits.  Two
    blocks have (nearly) as many distinct strings as sequences; the others repeat a few strings, as the genomes of a population do."""
    rng = random.Random(20261017)
    out = []
    for n, length, rate, alpha, mode in [
            (513, 30, 0.1, "ACGT", "haplotypes"), (513, 3, 0.3, "ACGTN", "copies"), (513, 97, 0.02, "ACGT", "haplotypes"),
            (601, 80, 0.05, "ACGT", "copies"), (601, 8, 0.3, "ACGTN", "copies"), (601, 12, 0.0, "ACGT", "unrelated"), (601, 300, 0.1, "ACGT", "haplotypes"),
            (1001, 40, 0.1, "ACGT", "haplotypes"), (1001, 150, 0.05, "ACGTN", "haplotypes"), (1001, 1, 0.3, "ACGT", "copies"),
            (2001, 30, 0.05, "ACGT", "haplotypes"), (2001, 60, 0.1, "ACGT", "copies"), (2001, 230, 0.1, "ACGT", "haplotypes"),
            (2048, 12, 0.3, "ACGTN", "haplotypes"), (2048, 90, 0.02, "ACGT", "haplotypes")]:
        out.append(_family(rng, n, length, rate, alpha, mode))
    out[OUTGROWS] = [s[:widegen.NARROW_COLS] for s in out[OUTGROWS]]
    out.append([s.ljust(TALL_SEQ_LEN, "A")[:TALL_SEQ_LEN] for s in _family(rng, TALL_SEQS, TALL_SEQ_LEN, 0.1, "ACGT", "haplotypes")])
    return out



def reference_align(blks):
    """the reference's MuscleInterface on every block (oracle/_ref/muscle_ref), from its record"""
    return widegen.reference_align(blks, golden=MUSCLE_TALL_GOLDEN)


def tall_run(core, name, tmp_path, env=None, threads=16):
    """the set `name` of parsnp_amd.synth through `core`, checked against the reference binary's record
    -> (the run's result, its PARSNP_TIMING record)"""
    import json
    import refruns
    from parsnp_amd import synth
    ref, gs = synth.make(name)
    rp, qs = synth.write_set(str(tmp_path / "in"), ref, gs)
    kw = dict(threads=threads)
    want = refruns.recorded(TALL_RUNS_GOLDEN, refruns.case_key(widegen.run_core, rp, qs, kw), refruns.REFBIN,
                            lambda: widegen.run_core(refruns.REFBIN, rp, qs, str(tmp_path / "ref"), kw))
    timing = str(tmp_path / "timing.json")
    got = refruns.normal(widegen.run_core(core, rp, qs, str(tmp_path / "mine"), kw, env=dict(os.environ if env is None else env, PARSNP_TIMING=timing)))
    assert got[0] == 0, got
    assert got == want, name
    return got, json.load(open(timing))
