"""Measurements of the neighbour-joining tree (profiles/nj/README.md) on one MI355X.

  python scripts/nj_measure.py tree OUT.json [DIST.tsv]    the `nj` time of pm_last_timing at the designed n = 2 048 (tests/njtree.balanced)
                                                           and, with a .snps.dist file, at that matrix (bact200: n = 201): 7 calls
                                                           each after a warm-up; the wall time of the call; and the plain OpenMP
                                                           host program of the same definition on 16 threads (scripts/nj_host.cpp,
                                                           compiled here without FMA), whose records must be the device's bit for bit
  python scripts/nj_measure.py product SET OUT.json [N]    parsnp_core on a synth set (bact200) with snps=1 and tree=1 in turn, N
                                                           whole processes each (default 3); the tree of the last run is checked
                                                           against tests/njtree.newick_of of its .snps.dist
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import njtree                                           # noqa: E402
from parsnp_amd import driver, synth                    # noqa: E402
from parsnp_amd.binding import Lib, Session             # noqa: E402
from parsnp_amd.paths import CORE_BIN                   # noqa: E402


def read_dist(path):
    lines = open(path).read().split("\n")[1:-1]
    return np.array([[int(x) for x in line.split("\t")[1:]] for line in lines], np.int32)


def tree(out_path, dist_path=None):
    lib = Lib()
    mats = {"balanced2048": njtree.balanced(11)[0]}
    if dist_path:
        mats["file%d" % len(read_dist(dist_path))] = read_dist(dist_path)
    v = C.c_void_p
    res = {}
    with tempfile.TemporaryDirectory() as td, Session(lib, [b"ACGTTGCAAGGCTTAACCGGTACGATCGATTACGGCAT" * 4] * 2) as s:
        so = os.path.join(td, "libnj_host.so")
        subprocess.run(["g++", "-O3", "-mavx2", "-fopenmp", "-shared", "-fPIC", os.path.join(ROOT, "scripts", "nj_host.cpp"), "-o", so], check=True)
        H = C.CDLL(so)
        H.nj_host.argtypes = [v, C.c_int, v, v, C.c_int]
        for name, d in mats.items():
            n = d.shape[0]
            dev_ms, wall_ms, host_ms = [], [], []
            for rep in range(8):      # (the first is the warm-up: allocations, code objects)
                t0 = time.perf_counter()
                got = s.nj_tree(d)
                wall = (time.perf_counter() - t0) * 1e3
                if rep:
                    wall_ms.append(wall)
                    dev_ms.append(dict(s.last_timing())["nj"])
            joins, last = np.zeros(max(n - 3, 1), njtree.JOIN), np.zeros(1, Session.NJ_LAST)
            for rep in range(4):
                t0 = time.perf_counter()
                H.nj_host(d.ctypes.data_as(v), n, joins.ctypes.data_as(v), last.ctypes.data_as(v), 16)
                if rep:
                    host_ms.append((time.perf_counter() - t0) * 1e3)
            njtree.same_records(got, (joins[:n - 3], last[0]))
            launches = 2 * (n - 3) + 2
            med = sorted(dev_ms)[len(dev_ms) // 2]
            res[name] = dict(n=n, launches=launches, nj_ms=sorted(dev_ms), nj_ms_median=med, us_per_launch=med * 1e3 / launches,
                             call_wall_ms=sorted(wall_ms), host16_ms=sorted(host_ms), host_over_device=sorted(host_ms)[1] / med)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def product(name, out_path, reps=3):
    base = tempfile.mkdtemp(prefix="nj_measure_")
    ref, gs = synth.make(name)
    rp, qs = synth.write_set(os.path.join(base, "in"), ref, gs)
    res = dict(set=name, snps=[], tree=[])
    for rep in range(reps):
        for tag, kw in (("snps", dict(snps=1)), ("tree", dict(tree=1))):
            out = os.path.join(base, "out_" + tag)
            t0 = time.perf_counter()
            rc, _ = driver.run_core(CORE_BIN, rp, qs, out, threads=16, timing=os.path.join(base, "t.json"), **kw)
            wall = time.perf_counter() - t0
            assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
            t = driver.read_timing(os.path.join(base, "t.json"))
            res[tag].append(dict({k: t[k] for k in t if k.startswith("nj_") or k in ("total_s", "output_s", "snp_dist_ms")}, wall_s=wall))
    names, _, _, dist = driver.read_snps(os.path.join(base, "out_tree"))
    assert driver.read_tree(os.path.join(base, "out_tree")) == njtree.newick_of(names, dist), "the tree is not the restatement's"
    res["dist_file"] = os.path.join(base, "out_tree", "parsnpAligner.snps.dist")
    res["leaves"] = len(names)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if sys.argv[1] == "tree":
        tree(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        product(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3)
