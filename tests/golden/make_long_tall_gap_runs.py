"""Records the reference's side of tests/test_long_tall_gaps.py and tests/test_gpu_long_tall_gaps.py: libMUSCLE's rows of the long-tall
block family (tests/longtallgen.py) into tests/golden/muscle_long_tall_runs.json.xz and the reference binary's run at d = 1000 on the
set of 600 genomes with windows of 330 to 900 bases into tests/golden/long_tall_gap_runs.json.xz (both read through tests/refruns.py).  Needs
oracle/_ref/muscle_ref and oracle/_ref/parsnp_core_ref (`make -C oracle ref`) and a built tree; like make_wide_gap_runs.py it runs
the tests with PARSNP_REF_RECORD set, so every test stops once the reference's side of its case is recorded.  A block of the family
on which MUSCLE quits, one outside the long-tall limits, or one whose alignment is wider than 2 048 columns or than the writer's row
capacity stops the recording: change the family (drop the seed), not the test -- the tests' "no block of the family is declined"
rests on it.  libMUSCLE needs a few minutes for the family (the two blocks of about 2 000 sequences), the reference binary likewise.

  python tests/golden/make_long_tall_gap_runs.py"""
import json
import lzma
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TESTS = ["tests/test_long_tall_gaps.py::test_host_restatement_on_the_long_tall_family",
         "tests/test_long_tall_gaps.py::test_six_hundred_genomes_with_long_windows_whole_run"]
sys.path.insert(0, os.path.join(ROOT, "tests"))


def check_rows(runs):
    import longtallgen as g
    family = [c.block for c in g.long_tall_blocks()]
    for key, rows in runs.items():
        if len(rows) != len(family):
            sys.exit("the record holds %d blocks, the long-tall family %d" % (len(rows), len(family)))
        for blk, want in zip(family, rows):
            if len(want) != len(blk) or len({len(r) for r in want}) != 1 or [r.replace("-", "") for r in want] != blk:
                sys.exit("MUSCLE did not align a block of the long-tall family (%d sequences): drop its seed" % len(blk))
            if not (g.OLD_SEQS < len(blk) <= g.LT_SEQS and g.OLD_SEQ_LEN < max(len(s) for s in blk) <= g.LT_SEQ_LEN and min(len(s) for s in blk) >= 1):
                sys.exit("a block of the long-tall family (%d sequences) is not beyond both older limits and inside the new ones" % len(blk))
            if len(want[0]) > min(g.LT_COLS, g.capacity(blk)):
                sys.exit("a block of the long-tall family (%d sequences, %d columns) is wider than 2 048 columns or than its row capacity %d" % (len(blk), len(want[0]), g.capacity(blk)))


def check_runs(runs):
    for k, v in runs.items():
        if v[0] != 0:
            sys.exit("the reference binary did not finish case %s cleanly: %r" % (k, v[:2]))


def main():
    for b in ("muscle_ref", "parsnp_core_ref"):
        if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", b)):
            sys.exit("oracle/_ref/%s is not built (make -C oracle ref)" % b)
    with tempfile.TemporaryDirectory() as d:
        cmd = [sys.executable, "-m", "pytest", "-q", "-m", "", "-p", "no:cacheprovider"] + TESTS + sys.argv[1:]
        if subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PARSNP_REF_RECORD=d)).returncode != 0:
            sys.exit("a test failed while recording")
        for name, check in (("muscle_long_tall_runs.json.xz", check_rows), ("long_tall_gap_runs.json.xz", check_runs)):
            src = os.path.join(d, name)
            if not os.path.isdir(src):
                continue
            runs = {f[:-len(".json")]: json.load(open(os.path.join(src, f))) for f in sorted(os.listdir(src))}
            check(runs)
            golden = os.path.join(ROOT, "tests", "golden", name)
            with lzma.open(golden, "wt", preset=9 | lzma.PRESET_EXTREME) as f:
                f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(runs.items())) + "\n}\n")
            print("%d reference results -> %s (%d bytes)" % (len(runs), os.path.relpath(golden, ROOT), os.path.getsize(golden)))


if __name__ == "__main__":
    main()
