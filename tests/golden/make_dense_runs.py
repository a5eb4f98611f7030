"""Records the reference binary's results for the tandem-array sets of tests/test_dense_repeats.py and
tests/test_gpu_dense_repeats.py into tests/golden/dense_runs.json.xz (read through tests/refruns.py).  Needs
oracle/_ref/parsnp_core_ref (`make -C oracle ref`) and a built tree; like make_reference_runs.py it runs the tests with
PARSNP_REF_RECORD set, so every test stops once the reference's side of its case is recorded.

  python tests/golden/make_dense_runs.py"""
import json
import lzma
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TESTS = ["tests/test_dense_repeats.py::test_whole_runs_small_budget", "tests/test_dense_repeats.py::test_whole_run_sharded_gloo",
         "tests/test_gpu_dense_repeats.py::test_whole_runs_small_budget_on_gpu", "tests/test_gpu_dense_repeats.py::test_shipped_binary_default_budget"]


def main():
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "parsnp_core_ref")):
        sys.exit("oracle/_ref/parsnp_core_ref is not built (make -C oracle ref)")
    with tempfile.TemporaryDirectory() as d:
        cmd = [sys.executable, "-m", "pytest", "-q", "-m", "", "-p", "no:cacheprovider"] + TESTS + sys.argv[1:]
        if subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PARSNP_REF_RECORD=d)).returncode != 0:
            sys.exit("a test failed while recording")
        name = "dense_runs.json.xz"
        src = os.path.join(d, name)
        runs = {f[:-len(".json")]: json.load(open(os.path.join(src, f))) for f in sorted(os.listdir(src))}
        for k, v in runs.items():
            if v[0] != 0:
                sys.exit("the reference binary did not finish case %s cleanly: %r" % (k, v[:2]))
        golden = os.path.join(ROOT, "tests", "golden", name)
        with lzma.open(golden, "wt", preset=9 | lzma.PRESET_EXTREME) as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(runs.items())) + "\n}\n")
        print("%d reference results -> %s" % (len(runs), os.path.relpath(golden, ROOT)))


if __name__ == "__main__":
    main()
