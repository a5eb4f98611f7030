"""Records tests/golden/unalign.json for the end-to-end tests of tests/test_unalign_runs.py and tests/test_gpu_unalign_runs.py: for every
set of test_unalign_runs.E2E_SETS, run with unaligned=1, what the REFERENCE binary (oracle/_ref/parsnp_core_ref, `make -C oracle
ref`) wrote -- the md5 and size of its parsnp.unalign and the md5 of its XMFA.  A set whose file holds fewer than 20 records is
refused: it would not show the writer.  Runs on the CPU.

  python tests/golden/make_golden_unalign.py"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import test_host_logic
    import test_unalign_runs as T
    import xmfa_util
    from parsnp_amd import driver
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "parsnp_core_ref")
    if not os.path.exists(ref_bin):
        sys.exit("%s is not built (make -C oracle ref)" % os.path.relpath(ref_bin, ROOT))
    out = {}
    for name in T.E2E_SETS:
        with tempfile.TemporaryDirectory() as d:
            rp, qs, kw = test_host_logic.harsh_inputs(name, d)
            o = os.path.join(d, "ref")
            rc, _ = driver.run_core(ref_bin, rp, qs, o, threads=4, unaligned=1, **kw)
            if rc != 0:
                sys.exit("%s: the reference ended with code %d" % (name, rc))
            u = os.path.join(o, "parsnp.unalign")
            records = open(u, "rb").read().count(b">")
            if records < 20:
                sys.exit("%s: %d records in parsnp.unalign: the set does not show the writer" % (name, records))
            out[name] = dict(unalign_md5=xmfa_util.md5(u), unalign_bytes=os.path.getsize(u), unalign_records=records,
                             xmfa_md5=xmfa_util.md5(os.path.join(o, "parsnpAligner.xmfa")))
            print("%s: %s" % (name, out[name]))
    path = os.path.join(ROOT, "tests", "golden", "unalign.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("-> %s (%d bytes)" % (os.path.relpath(path, ROOT), os.path.getsize(path)))


if __name__ == "__main__":
    main()
