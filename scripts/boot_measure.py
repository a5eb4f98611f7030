"""Measurements of the bootstrap support (profiles/boot/README.md) on one MI355X.

  python scripts/boot_measure.py kernels OUT.json [SNPS.mfa]   B = 100 replicates over a designed collection of 2 048 rows x 23 704 core
                                                               SNP columns and, with a .snps.mfa file, over that collection (bact200:
                                                               201 rows): the phases boot_draw, boot_dist, boot_nj and boot_support of
                                                               pm_last_timing, 7 calls each after a warm-up (nothing is downloaded in
                                                               the timed calls); snp_dist of the same collection; and B calls of
                                                               pm_nj_tree on the same replicate matrices (the sum of their `nj` phases
                                                               and the wall time), whose records must be the batch's bit for bit
  python scripts/boot_measure.py product SET OUT.json [N]      parsnp_core on a synth set (bact200) with tree=1 and bootstrap=100 in
                                                               turn, N whole processes each (default 3); the labelled tree of the last
                                                               run is checked against tests/bootsupport.newick_of of its .snps.mfa
"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bootsupport                                      # noqa: E402
import njtree                                           # noqa: E402
from parsnp_amd import driver, synth                    # noqa: E402
from parsnp_amd.binding import Lib, Session             # noqa: E402
from parsnp_amd.paths import CORE_BIN                   # noqa: E402

REPS, SEED = 100, 1
# vector instructions of SnpDistBoot per (pair, word, replicate), read in the gfx950 ISA of its inner loop, and the issue rate
# scripts/valu_calib.hip measured (cycles per wave64 instruction and SIMD); 256 CUs x 4 SIMDs at 2.4 GHz
INSTR_PER_PAIR_WORD_REP, CYCLES_PER_INSTR, SIMDS, HZ = 22.6, 2.2, 1024, 2.4e9


def phases(s):
    return dict(s.last_timing())


def med(xs):
    return sorted(xs)[len(xs) // 2]


def kernels(out_path, mfa=None):
    lib = Lib()
    L = lib.L
    v = C.c_void_p
    sets = {"designed2048": bootsupport.snp_letters(2048, 23704, 1)}
    if mfa:
        lines = open(mfa, "rb").read().split(b"\n")
        letters = np.array([np.frombuffer(x, np.uint8) for x in lines[1:-1:2]], np.uint8)
        sets["file%d" % letters.shape[0]] = letters
    res = {}
    for name, letters in sets.items():
        n, nv = letters.shape
        with Session(lib, [b"ACGTTGCAAGGCTTAACCGGTACGATCGATTACGGCAT" * 4] * 2) as s:
            main_dist = s.core_snps([letters])[3]
            L.pm_snp_distances.argtypes = [v, v]
            L.pm_boot_distances.argtypes = [v, C.c_int32, C.c_uint64, v, C.c_int64, v, v]
            L.pm_nj_trees.argtypes = [v, C.c_int32, C.c_int32, v, v, v]
            t = dict(snp_dist=[], boot_draw=[], boot_dist=[], boot_nj=[], boot_support=[], boot_nj_wall=[])
            main = s.nj_tree()
            for rep in range(8):      # (the first is the warm-up: allocations, code objects)
                lib._check(L.pm_snp_distances(s.h, main_dist.ctypes.data_as(v)))
                a = phases(s)
                lib._check(L.pm_boot_distances(s.h, REPS, SEED, None, 0, None, None))
                b = phases(s)
                t0 = time.perf_counter()
                lib._check(L.pm_nj_trees(s.h, n, REPS, None, None, None))
                wall = (time.perf_counter() - t0) * 1e3
                c = phases(s)
                s._boot_trees = REPS
                sup = s.nj_support(n, main[0])
                d = phases(s)
                if rep:
                    t["snp_dist"].append(a["snp_dist"]); t["boot_draw"].append(b["boot_draw"]); t["boot_dist"].append(b["boot_dist"])      # noqa: E702
                    t["boot_nj"].append(c["boot_nj"]); t["boot_nj_wall"].append(wall); t["boot_support"].append(d["boot_support"])      # noqa: E702
            # the same replicate matrices, one pm_nj_tree call each (the parent commit's only way)
            s._boot_reps = REPS
            _, dist = s.boot_distances(REPS, SEED)
            joins, last = s.nj_trees()
            seq_ms, seq_wall = [], []
            for rep in range(4 if n > 1000 else 8):
                dev, t0 = 0.0, time.perf_counter()
                for k in range(REPS):
                    got = s.nj_tree(dist[k])
                    dev += phases(s)["nj"]
                    if not rep:
                        njtree.same_records((joins[k], last[k]), got)
                if rep:
                    seq_ms.append(dev); seq_wall.append((time.perf_counter() - t0) * 1e3)      # noqa: E702
            words = (nv + 63) // 64
            pair_words = n * (n + 1) / 2 * words
            bound_ms = pair_words * REPS * INSTR_PER_PAIR_WORD_REP / 64 * CYCLES_PER_INSTR / (SIMDS * HZ) * 1e3
            r = {k: sorted(x) for k, x in t.items()}
            r.update(n=n, core_snps=nv, reps=REPS, launches_per_batch=2 * (n - 3) + 2, support_min=int(sup.min()), support_max=int(sup.max()),
                     sequential_nj_ms=sorted(seq_ms), sequential_wall_ms=sorted(seq_wall),
                     nj_ratio=med(seq_ms) / med(t["boot_nj"]), nj_wall_ratio=med(seq_wall) / med(t["boot_nj_wall"]),
                     dist_over_reps_snp_dist=med(t["boot_dist"]) / (REPS * med(t["snp_dist"])), dist_issue_bound_ms=bound_ms,
                     dist_over_bound=med(t["boot_dist"]) / bound_ms)
            res[name] = r
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def product(name, out_path, reps=3):
    base = tempfile.mkdtemp(prefix="boot_measure_")
    ref, gs = synth.make(name)
    rp, qs = synth.write_set(os.path.join(base, "in"), ref, gs)
    res = dict(set=name, tree=[], boot=[])
    for rep in range(reps):
        for tag, kw in (("tree", dict(tree=1)), ("boot", dict(bootstrap=REPS))):
            out = os.path.join(base, "out_" + tag)
            t0 = time.perf_counter()
            rc, _ = driver.run_core(CORE_BIN, rp, qs, out, threads=16, timing=os.path.join(base, "t.json"), **kw)
            wall = time.perf_counter() - t0
            assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
            t = driver.read_timing(os.path.join(base, "t.json"))
            res[tag].append(dict({k: t[k] for k in t if k.startswith(("nj_", "boot_")) or k in ("total_s", "output_s", "snp_dist_ms")}, wall_s=wall))
    names, letters, _, _ = driver.read_snps(os.path.join(base, "out_boot"))
    assert driver.read_boot_tree(os.path.join(base, "out_boot")) == bootsupport.newick_of(names, letters, REPS, 1), "the labelled tree is not the restatement's"
    assert open(os.path.join(base, "out_boot", "parsnpAligner.snps.nwk"), "rb").read() == open(os.path.join(base, "out_tree", "parsnpAligner.snps.nwk"), "rb").read()
    res["mfa_file"] = os.path.join(base, "out_boot", "parsnpAligner.snps.mfa")
    res["leaves"], res["core_snps"] = len(names), int(letters.shape[1])
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if sys.argv[1] == "kernels":
        kernels(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        product(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3)
