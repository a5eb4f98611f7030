"""Records tests/golden/e2e_chain_bp.json for tests/test_chain_bp.py and tests/test_gpu_chain_bp.py: for every set of
test_chain_bp.E2E_SETS (a diagonal difference given in bases: diagdiff=25, and once literally 100bp) what the REFERENCE binary
(oracle/_ref/parsnp_core_ref, `make -C oracle ref`) wrote -- the md5 of its XMFA, its MUM / LCB signature, the counters of its log --
and, from the product's host-logic run (oracle/_ref/parsnp_core_oracle: the host code over the CPU provider of the ABI),
chain_passed: the MUMs that neither joined nor closed a chain in the first chaining pass.  A set with fewer than 10 of them is
refused: it would not show the mode.  Runs on the CPU.

  python tests/golden/make_chain_bp_golden.py"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import test_chain_bp as T
    import xmfa_util
    from parsnp_amd import driver
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "parsnp_core_ref")
    host_bin = os.path.join(ROOT, "oracle", "_ref", "parsnp_core_oracle")
    for b in (ref_bin, host_bin):
        if not os.path.exists(b):
            sys.exit("%s is not built (make -C oracle ref hosttest)" % os.path.relpath(b, ROOT))
    out = {}
    for name in sorted(T.E2E_SETS):
        with tempfile.TemporaryDirectory() as d:
            rp, qs, kw = T.e2e_inputs(name, d)
            rec = {"set": list(T.E2E_SETS[name][:2]), "ini": kw}
            for who, core in (("ref", ref_bin), ("host", host_bin)):
                o = os.path.join(d, who)
                timing = os.path.join(d, who + ".json")
                rc, _ = driver.run_core(core, rp, qs, o, timing=timing, threads=4, **kw)
                if rc != 0:
                    sys.exit("%s: %s ended with code %d" % (name, os.path.basename(core), rc))
                x, lg = os.path.join(o, "parsnpAligner.xmfa"), os.path.join(o, "parsnpAligner.log")
                got = dict(xmfa_md5=xmfa_util.md5(x), signature=xmfa_util.mum_lcb_signature(x), log=xmfa_util.log_counters(lg), log_lines=open(lg).read().splitlines())
                if who == "ref":
                    rec.update(got)
                else:
                    if got["xmfa_md5"] != rec["xmfa_md5"] or got["log"] != rec["log"]:
                        sys.exit("%s: the product's host logic and the reference differ" % name)
                    rec["chain_passed"] = driver.read_timing(timing)["chain_passed"]
            if rec["chain_passed"] < 10:
                sys.exit("%s: %d passed MUMs in the first chaining pass: the set does not show the mode" % (name, rec["chain_passed"]))
            print("%s: md5 %s, %d passed MUMs in the first pass, log %s" % (name, rec["xmfa_md5"], rec["chain_passed"], rec["log"]))
            out[name] = rec
    path = os.path.join(ROOT, "tests", "golden", "e2e_chain_bp.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("-> %s (%d bytes)" % (os.path.relpath(path, ROOT), os.path.getsize(path)))


if __name__ == "__main__":
    main()
