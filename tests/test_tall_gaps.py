"""Gaps of alignments with more than 512 genomes on the CPU: the host restatement of the gap aligner
(parsnp_amd/csrc/host/gapalign.cpp) against the reference's recorded rows on the tall block family (tests/tallgen.py), and the whole
pipeline on a set of 640 genomes against the reference binary's recorded run.  These pin the oracle of the device's tall form
(tests/test_gpu_tall_gaps.py) and the path the writer takes where no device form is available."""
import hashlib

import tallgen
import widegen
from test_gapalign import aligner  # noqa: F401  (fixture: the host restatement)


def test_host_restatement_on_the_tall_family(aligner):  # noqa: F811
    """identical rows on every block of the family, all of which the reference aligns itself (a block on which MUSCLE quits comes
    back as its input, which the check of equal row lengths would catch)"""
    family = tallgen.tall_blocks()
    wants = tallgen.reference_align(family)
    assert len(wants) == len(family) >= 15
    assert {len(b) for b in family} == set(tallgen.TALL_SIZES)
    assert all(widegen.WIDE_SEQS < len(b) <= tallgen.TALL_SEQS and 1 <= min(len(s) for s in b) and max(len(s) for s in b) <= tallgen.TALL_SEQ_LEN for b in family)
    assert any(len(b) == tallgen.TALL_SEQS and all(len(s) == tallgen.TALL_SEQ_LEN for s in b) for b in family)
    assert sum(max(len(s) for s in b) > widegen.NARROW_COLS for b in family) >= 4
    assert sum(max(len(s) for s in b) <= 90 for b in family) >= 8
    assert any("N" in s for b in family for s in b)
    assert max(len(s) for s in family[tallgen.OUTGROWS]) <= widegen.NARROW_COLS < len(wants[tallgen.OUTGROWS][0])
    assert sum(len(set(b)) > 500 for b in family) >= 2
    for blk, want in zip(family, wants):
        assert len(want) == len(blk) and len({len(r) for r in want}) == 1 and [r.replace("-", "") for r in want] == blk      # the reference aligned it
        assert len(want[0]) <= tallgen.TALL_COLS
        assert aligner(blk) == want, (len(blk), blk[0][:40])


def test_six_hundred_and_forty_genomes_whole_run(cpu_checkers, tmp_path):
    """640 genomes of 100 kb with 12 windows of 24 haplotypes through the CPU build of parsnp_core, default settings, 16 threads: the
    reference binary's XMFA bytes and log counters; every gap has 641 sequences and (on this build) is aligned on the host"""
    got, t = tallgen.tall_run(cpu_checkers, "tall640x100k", tmp_path)
    assert t["gap_host"] == t["gap_jobs"] >= 300 and t["gap_jobs_wide"] >= 8, t
    assert t["gap_device_narrow"] == 0 and t["gap_device_wide"] == 0 and t.get("gap_device_tall", 0) == 0, t


def test_new_configs_changed_no_existing_set():
    from parsnp_amd import synth

    def md5(name):
        ref, gs = synth.make(name)
        return hashlib.md5(b"\n".join([ref] + list(gs))).hexdigest()
    assert md5("hyper10x300k") == HYPER10_MD5 and md5("pop6x200k") == POP6_MD5
    assert synth.CONFIGS["tall640x100k"][1]["n_genomes"] == 640 and synth.CONFIGS["tall2000x30k"][1]["n_genomes"] == 2000


# md5 of b"\n".join([ref] + genomes) of the two sets, from the commit before the tall configurations were added
HYPER10_MD5 = "49f3234f7a8a2de4fc51ecd689f5d283"
POP6_MD5 = "0494de74139a79f31fe53bb56ab13c09"
