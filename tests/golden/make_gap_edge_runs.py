"""Records the reference's side of tests/test_gap_edges.py and tests/test_gpu_gap_edges.py: libMUSCLE's rows of every designed block
of tests/gapedges.py, one record per topic, into tests/golden/muscle_edge_runs.json.xz (read through tests/refruns.py).  Needs
oracle/_ref/muscle_ref (`make -C oracle ref`) and a built tree; like make_long_gap_runs.py it runs the test with PARSNP_REF_RECORD
set, so every case of it stops once the reference's side of its topic is recorded.  A block on which MUSCLE quits stops the
recording: change the block, not the test.  libMUSCLE needs about a minute, most of it for the 2 048 x 320 block.

The record must stay no larger than the largest fixture beside it; it is a third of that with every kind at every length, so no
"unrelated" pair is dropped (gapedges.UNRELATED_MOST).

  python tests/golden/make_gap_edge_runs.py"""
import json
import lzma
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TESTS = ["tests/test_gap_edges.py::test_restatement_equals_the_record"]
NAME = "muscle_edge_runs.json.xz"
MOST_BYTES = 322341      # the largest fixture under tests/golden when this one was added
sys.path.insert(0, os.path.join(ROOT, "tests"))


def check_rows(runs):
    import hashlib
    import gapedges
    for topic in gapedges.TOPICS:
        blocks = [c.block for c in gapedges.cases(topic)]
        key = hashlib.sha256(("\n\n".join("\n".join(b) for b in blocks) + "\n").encode()).hexdigest()
        if key not in runs:
            sys.exit("no record of the topic %s" % topic)
        if len(runs[key]) != len(blocks):
            sys.exit("the record of %s holds %d blocks, the topic %d" % (topic, len(runs[key]), len(blocks)))
        for c, want in zip(gapedges.cases(topic), runs[key]):
            if len(want) != len(c.block) or len({len(r) for r in want}) != 1 or [r.replace("-", "") for r in want] != c.block:
                sys.exit("MUSCLE did not align the block %r: change it" % c.name)
    if len(runs) != len(gapedges.TOPICS):
        sys.exit("%d records for %d topics" % (len(runs), len(gapedges.TOPICS)))


def main():
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "muscle_ref")):
        sys.exit("oracle/_ref/muscle_ref is not built (make -C oracle ref)")
    with tempfile.TemporaryDirectory() as d:
        cmd = [sys.executable, "-m", "pytest", "-q", "-m", "", "-p", "no:cacheprovider"] + TESTS + sys.argv[1:]
        if subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PARSNP_REF_RECORD=d)).returncode != 0:
            sys.exit("a test failed while recording")
        src = os.path.join(d, NAME)
        runs = {f[:-len(".json")]: json.load(open(os.path.join(src, f))) for f in sorted(os.listdir(src))}
        check_rows(runs)
        golden = os.path.join(ROOT, "tests", "golden", NAME)
        with lzma.open(golden, "wt", preset=9 | lzma.PRESET_EXTREME) as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(runs.items())) + "\n}\n")
        size = os.path.getsize(golden)
        print("%d reference results -> %s (%d bytes)" % (len(runs), os.path.relpath(golden, ROOT), size))
        if size > MOST_BYTES:
            sys.exit("the record is larger than %d bytes: lower gapedges.UNRELATED_MOST to 513" % MOST_BYTES)


if __name__ == "__main__":
    main()
