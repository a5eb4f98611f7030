"""Records the reference's side of tests/test_long_gaps.py and tests/test_gpu_long_gaps.py: libMUSCLE's rows of the long block
family (tests/longgen.py) into tests/golden/muscle_long_runs.json.xz and the reference binary's runs at d = 1000 on the two sets
with windows of 330 to 900 bases into tests/golden/long_gap_runs.json.xz (both read through tests/refruns.py).  Needs
oracle/_ref/muscle_ref and oracle/_ref/parsnp_core_ref (`make -C oracle ref`) and a built tree; like make_wide_gap_runs.py it runs
the tests with PARSNP_REF_RECORD set, so every test stops once the reference's side of its case is recorded.  A block of the family
on which MUSCLE quits, or one outside the long limits, stops the recording: change the family (drop the seed), not the test.
libMUSCLE needs about a minute for the family and the reference binary about two for the two sets.

  python tests/golden/make_long_gap_runs.py"""
import json
import lzma
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TESTS = ["tests/test_long_gaps.py::test_host_restatement_on_the_long_family", "tests/test_long_gaps.py::test_long_windows_whole_run_at_d_1000",
         "tests/test_gpu_long_gaps.py::test_two_hundred_genomes_with_long_windows"]
sys.path.insert(0, os.path.join(ROOT, "tests"))


def check_rows(runs):
    import longgen
    import widegen
    family = longgen.long_blocks()
    for key, rows in runs.items():
        if len(rows) != len(family):
            sys.exit("the record holds %d blocks, the long family %d" % (len(rows), len(family)))
        for blk, want in zip(family, rows):
            if len(want) != len(blk) or len({len(r) for r in want}) != 1 or [r.replace("-", "") for r in want] != blk:
                sys.exit("MUSCLE did not align a block of the long family (%d sequences): drop its seed" % len(blk))
            if not (2 <= len(blk) <= longgen.LONG_SEQS and widegen.WIDE_SEQ_LEN < max(len(s) for s in blk) <= longgen.LONG_SEQ_LEN and len(want[0]) <= longgen.LONG_COLS):
                sys.exit("a block of the long family (%d sequences, %d columns) lies outside the long limits" % (len(blk), len(want[0])))


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
        for name, check in (("muscle_long_runs.json.xz", check_rows), ("long_gap_runs.json.xz", check_runs)):
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
