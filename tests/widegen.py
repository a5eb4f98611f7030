"""Seeded inputs for the wide form of the gap aligner: gap strings of 97 to 320 bases, the gaps between adjacent MUMs that the
reference's default cluster distance d = 300 produces on real genomes (src/parsnp.cpp:2635-2693), and the synthetic genome set
with hypervariable windows that makes the whole pipeline meet them.  The reference's rows of the blocks are recorded in
tests/golden/muscle_wide_runs.json.xz, its whole runs in tests/golden/wide_gap_runs.json.xz (tests/golden/make_wide_gap_runs.py)."""
import hashlib
import os
import random
import subprocess

import gapgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUSCLE_WIDE_GOLDEN = os.path.join(ROOT, "tests", "golden", "muscle_wide_runs.json.xz")
WIDE_RUNS_GOLDEN = os.path.join(ROOT, "tests", "golden", "wide_gap_runs.json.xz")
# the limits of the device's wide form as include/parsnp_mum.h documents them; the GPU tests read them from pm_gap_limits(1, ...)
# and check that they are these
WIDE_SEQS, WIDE_SEQ_LEN, WIDE_COLS = 512, 320, 640
NARROW_COLS = 96


def _string(rng, length, alpha):
    return "".join(rng.choice(alpha) for _ in range(length))


def _family(rng, n, length, rate, alpha, mode):
    base = _string(rng, length, alpha)
    seqs = []
    for i in range(n):
        if mode == "copies":        # every sequence its own diverged copy
            seqs.append(gapgen.mutate(rng, base, rate, alpha))
        elif mode == "haplotypes":  # a few haplotypes shared by many genomes
            seqs.append(gapgen.mutate(rng, base, rate, alpha) if i < 4 else seqs[rng.randrange(4)])
        else:                       # unrelated strings
            seqs.append(_string(rng, rng.randint(NARROW_COLS + 1, length), alpha))
    seqs = [s[:WIDE_SEQ_LEN] for s in seqs]
    if max(len(s) for s in seqs) <= NARROW_COLS:      # every block of the family is a wide one
        seqs[0] = (seqs[0] + _string(rng, NARROW_COLS + 1, alpha))[:NARROW_COLS + 1]
    return seqs


def wide_blocks():
    """the family: 2 to 200 sequences of 97 to 320 bases at divergence 0.02 to 0.6 over ACGT and ACGTN, as diverged copies, shared
    haplotypes and unrelated strings; one block with as many sequences as the device takes, one with sequences of the longest
    length it takes, and one whose alignment is wider than 600 columns.  All lie inside the wide form's limits."""
    rng = random.Random(20261016)
    out = []
    for n, length, rate, alpha, mode in [
            (2, 97, 0.02, "ACGT", "copies"), (2, 320, 0.3, "ACGT", "copies"), (3, 150, 0.6, "ACGTN", "copies"), (4, 200, 0.1, "ACGT", "unrelated"),
            (5, 250, 0.3, "ACGTN", "copies"), (6, 120, 0.1, "ACGT", "haplotypes"), (8, 300, 0.02, "ACGT", "copies"), (8, 180, 0.6, "ACGT", "copies"),
            (12, 300, 0.1, "ACGT", "copies"), (12, 280, 0.3, "ACGTN", "haplotypes"), (12, 320, 0.1, "ACGT", "copies"), (20, 130, 0.3, "ACGT", "unrelated"),
            (20, 260, 0.6, "ACGT", "haplotypes"), (30, 99, 0.1, "ACGTN", "copies"), (50, 300, 0.3, "ACGT", "copies"), (50, 160, 0.02, "ACGT", "haplotypes"),
            (100, 220, 0.1, "ACGT", "haplotypes"), (200, 300, 0.1, "ACGT", "copies"), (200, 120, 0.3, "ACGTN", "copies"), (200, 300, 0.3, "ACGT", "haplotypes")]:
        out.append(_family(rng, n, length, rate, alpha, mode))
    out.append(_family(rng, WIDE_SEQS, 110, 0.05, "ACGT", "haplotypes"))      # the sequence limit (its rows do not fit the LDS)
    out.append([s.ljust(WIDE_SEQ_LEN, "A")[:WIDE_SEQ_LEN] for s in _family(rng, 6, WIDE_SEQ_LEN, 0.1, "ACGT", "copies")])      # every sequence at the length limit
    rng = random.Random(1040)
    out.append([_string(rng, rng.randint(300, 320), "ACGT") for _ in range(40)])      # unrelated long strings: 614 columns
    return out


def reference_align(blks, golden=MUSCLE_WIDE_GOLDEN):
    """the reference's MuscleInterface on every block (oracle/_ref/muscle_ref), from its record"""
    import refruns
    inp = "\n\n".join("\n".join(b) for b in blks) + "\n"

    def compute():
        out = subprocess.run([gapgen.MUSCLE_REF], input=inp.encode(), capture_output=True, check=True).stdout.decode()
        return [b.split("\n") for b in out.strip("\n").split("\n\n")]
    return refruns.recorded(golden, hashlib.sha256(inp.encode()).hexdigest(), gapgen.MUSCLE_REF, compute)


def run_core(core, rp, qs, out, kw, env=None):
    """one run of a parsnp_core binary with the driver's default settings (d = 300) -> (exit code, XMFA md5, log counters)"""
    import xmfa_util
    from parsnp_amd import driver
    rc, _ = driver.run_core(core, rp, qs, out, timeout=1500, env=env, **kw)
    x = os.path.join(out, "parsnpAligner.xmfa")
    lg = os.path.join(out, "parsnpAligner.log")
    return (rc, xmfa_util.md5(x) if os.path.exists(x) else None, xmfa_util.log_counters(lg) if os.path.exists(x) else open(lg).read())


def hyper_run(core, name, tmp_path, env=None, threads=8, reference="record"):
    """the set `name` of parsnp_amd.synth (hypervariable windows) through `core`: checked against the reference binary's record
    (reference = "record") or not at all (reference = None) -> (the run's result, its PARSNP_TIMING record, inputs)"""
    import json
    import refruns
    from parsnp_amd import synth
    ref, gs = synth.make(name)
    rp, qs = synth.write_set(str(tmp_path / "in"), ref, gs)
    kw = dict(threads=threads)
    if reference == "record":
        want = refruns.recorded(WIDE_RUNS_GOLDEN, refruns.case_key(run_core, rp, qs, kw), refruns.REFBIN,
                                lambda: run_core(refruns.REFBIN, rp, qs, str(tmp_path / "ref"), kw))
    timing = str(tmp_path / "timing.json")
    got = refruns.normal(run_core(core, rp, qs, str(tmp_path / "mine"), kw, env=dict(os.environ if env is None else env, PARSNP_TIMING=timing)))
    assert got[0] == 0, got
    if reference == "record":
        assert got == want, name
    return got, json.load(open(timing)), (rp, qs, kw)
