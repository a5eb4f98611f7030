"""Records the reference programs' results for the side-by-side tests into tests/golden/reference_runs.json.xz and
tests/golden/muscle_runs.json.xz (read by tests/refruns.py).  Needs oracle/_ref/parsnp_core_ref and muscle_ref (`make -C oracle
ref`) and a built tree.  Runs every test that asks tests/refruns.py for a result -- the GPU ones too: in this mode a test
stops once the reference's side of its case is recorded, before the product's side -- and writes what they recorded, one
case per line, xz-compressed.

  python tests/golden/make_reference_runs.py [more pytest arguments, e.g. -n 8]"""
import json
import lzma
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TESTS = ["tests/test_edge_vs_reference.py", "tests/test_fuzz_vs_reference.py", "tests/test_ingest_vs_reference.py",
         "tests/test_gpu_parity.py::test_parsnp_core_vs_reference_binary_fresh_input", "tests/test_gapalign.py::test_fresh_sets_against_reference",
         "tests/test_gpu_gapalign.py::test_fresh_sets_against_reference"]


def main():
    for prog in ("parsnp_core_ref", "muscle_ref"):
        if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", prog)):
            sys.exit("oracle/_ref/%s is not built (make -C oracle ref)" % prog)
    with tempfile.TemporaryDirectory() as d:
        cmd = [sys.executable, "-m", "pytest", "-q", "-m", "", "-p", "no:cacheprovider"] + TESTS + sys.argv[1:]
        if subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PARSNP_REF_RECORD=d)).returncode != 0:
            sys.exit("a test failed while recording")
        for name in sorted(os.listdir(d)):
            runs = {f[:-len(".json")]: json.load(open(os.path.join(d, name, f))) for f in sorted(os.listdir(os.path.join(d, name)))}
            golden = os.path.join(ROOT, "tests", "golden", name)
            with lzma.open(golden, "wt", preset=9 | lzma.PRESET_EXTREME) as f:
                f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(runs.items())) + "\n}\n")
            print("%d reference results -> %s" % (len(runs), os.path.relpath(golden, ROOT)))


if __name__ == "__main__":
    main()
