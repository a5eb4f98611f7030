"""Gaps of 97 to 320 bases between adjacent MUMs -- what the reference's default cluster distance d = 300 produces on real genomes --
on the CPU: the host restatement of the gap aligner (parsnp_amd/csrc/host/gapalign.cpp) against the reference's recorded rows on
the wide block family (tests/widegen.py), and the whole pipeline on a synthetic set with hypervariable windows against the reference
binary's recorded run.  The device's side is tests/test_gpu_wide_gaps.py."""
import widegen
from test_gapalign import aligner  # noqa: F401  (fixture: the host restatement)


def test_host_restatement_on_the_wide_family(aligner):  # noqa: F811
    """pins the oracle the GPU test compares against: identical rows on every block of the family, all of which the reference
    aligns itself (a block on which MUSCLE quits comes back as its input, which the check of equal row lengths would catch)"""
    family = widegen.wide_blocks()
    wants = widegen.reference_align(family)
    assert len(wants) == len(family) >= 20
    sizes = [len(b) for b in family]
    assert min(sizes) == 2 and 200 in sizes and widegen.WIDE_SEQS in sizes
    assert all(widegen.NARROW_COLS < max(len(s) for s in b) <= widegen.WIDE_SEQ_LEN for b in family)
    assert any(all(len(s) == widegen.WIDE_SEQ_LEN for s in b) for b in family)
    assert 600 < max(len(w[0]) for w in wants) <= widegen.WIDE_COLS
    for blk, want in zip(family, wants):
        assert len({len(r) for r in want}) == 1 and [r.replace("-", "") for r in want] == blk      # the reference aligned it
        assert len(want[0]) <= widegen.WIDE_COLS
        assert aligner(blk) == want, (len(blk), blk[0][:40])


def test_hypervariable_windows_whole_run(cpu_checkers, tmp_path):
    """10 genomes of 300 kb with 160 hypervariable windows through the CPU build of parsnp_core, default d = 300: the reference
    binary's XMFA bytes and log counters, and the set really has wide gaps -- counted by width in the PARSNP_TIMING record
    (on this build every gap is aligned on the host)"""
    got, t, _ = widegen.hyper_run(cpu_checkers, "hyper10x300k", tmp_path)
    assert t["gap_jobs_wide"] >= 50 and t["gap_longest"] >= 250, t
    assert t["gap_jobs"] >= t["gap_jobs_wide"] and t["gap_host"] == t["gap_jobs"] and t["gap_device_wide"] == 0 and t["gap_device_narrow"] == 0, t
    assert t["gap_host_s"] > 0


def test_windows_are_off_by_default():
    """the new argument of the population generator changes no existing set, and a set with windows keeps every copy of a
    window under 300 bases and within 12 % of the others"""
    from parsnp_amd import synth
    kw = dict(seed=9, n=60_000, n_genomes=4, div=0.02, indel_frac=0.05)
    assert synth.population(**kw) == synth.population(windows=None, **kw)
    ref, gs = synth.population(windows=dict(count=20), **kw)
    assert ref == synth.population(**kw)[0]
    assert all(abs(len(g) - len(ref)) < 20 * 15 + 0.02 * 0.05 * len(ref) for g in gs) and len(set(gs)) == 4
