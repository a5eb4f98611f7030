"""Measurements of the SNP collection (profiles/snp/README.md) on one MI355X.

  python scripts/snp_measure.py matrix OUT.json            a designed 2 048 x 100 000 matrix, a quarter of its columns core SNPs
  python scripts/snp_measure.py product SET OUT.json [N]   parsnp_core on a synth set (bact200, tall2000x30k) with snps=0 and
                                                           snps=1 in turn, N whole processes each (default 3)
  python scripts/snp_measure.py check BASE                 the three files of BASE/out1 (the "base" of a product record) against
                                                           tests/snpcols.scan_xmfa of its XMFA

matrix: HIP-event time of classify, scan, pack (all adds) and dist (pm_last_timing), the bytes uploaded, and SnpDist against a plain
OpenMP loop over the same planes on 16 host threads (scripts/snp_dist_host.cpp, compiled here), each timed 5 times after a warm-up
call."""
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

from parsnp_amd import driver, synth                    # noqa: E402
from parsnp_amd.binding import Lib, Session             # noqa: E402
from parsnp_amd.paths import CORE_BIN                   # noqa: E402


def build_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "worktree"
    except OSError:
        return "worktree"


def designed(n=2048, cols=100_000, seed=1):
    """n x cols letters: a random base row, a quarter of the columns with a second letter in a random third of the rows, one column in
    twenty with a '-' somewhere"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    base = rng.integers(0, 4, cols)
    m = np.repeat(acgt[base][None, :], n, axis=0)
    snp = np.flatnonzero(rng.random(cols) < 0.25)
    for c in snp:
        rows = np.flatnonzero(rng.random(n) < 1 / 3)
        m[rows if len(rows) else [0], c] = acgt[(base[c] + 1 + int(rng.integers(0, 3))) % 4]
    other = np.flatnonzero(rng.random(cols) < 0.05)
    m[rng.integers(0, n, len(other)), other] = ord("-")
    return m


def matrix(out_path):
    lib = Lib()
    L = lib.L
    v = C.c_void_p
    L.pm_snp_begin.argtypes = [v, C.c_int32]
    L.pm_snp_add.argtypes = [v, C.c_int64, C.c_int64, v, v]
    L.pm_snp_columns.argtypes = [v, v, v]
    L.pm_snp_distances.argtypes = [v, v]
    m = designed()
    n, cols = m.shape
    chunk = 16384
    res = dict(build=build_hash(), rows=n, columns=cols, chunk_columns=chunk, runs=[])
    with Session(lib, [b"ACGTTGCAAGGCTTAACCGGTACGATCGATTACGGCAT" * 4] * 2) as s:
        for rep in range(6):      # (the first is the warm-up: allocations, code objects)
            phases = {}
            t0 = time.perf_counter()
            lib._check(L.pm_snp_begin(s.h, n))
            totals = np.zeros(4, np.int64)
            for c0 in range(0, cols, chunk):
                part = m[:, c0:c0 + chunk]
                lib._check(L.pm_snp_add(s.h, part.shape[1], part.strides[0], part.ctypes.data_as(v), totals.ctypes.data_as(v)))
                for name, ms in s.last_timing():
                    phases[name] = phases.get(name, 0.0) + ms
            t_add = time.perf_counter() - t0
            nv = int(totals[2])
            dist = np.zeros((n, n), np.int32)
            t0 = time.perf_counter()
            lib._check(L.pm_snp_distances(s.h, dist.ctypes.data_as(v)))
            t_dist = time.perf_counter() - t0
            for name, ms in s.last_timing():
                phases[name] = phases.get(name, 0.0) + ms
            if rep:
                res["runs"].append(dict(phases_ms=phases, adds_wall_s=t_add, dist_wall_s=t_dist))
        letters = np.zeros((n, nv), np.uint8)
        lib._check(L.pm_snp_columns(s.h, None, letters.ctypes.data_as(v)))
    res["counts"] = dict(zip(("columns", "core_invariant", "core_snps", "other"), (int(x) for x in totals)))
    res["h2d_bytes"] = n * cols
    # the same planes on the host, row-major
    code = (letters >> 1) & 3
    words = (nv + 63) // 64
    planes = []
    for bit in (0, 1):
        bits = np.zeros((n, words * 64), np.uint8)
        bits[:, :nv] = (code >> bit) & 1
        planes.append(np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view(np.uint64)))
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libsnp_dist_host.so")
        subprocess.run(["g++", "-O3", "-march=native", "-fopenmp", "-shared", "-fPIC", os.path.join(ROOT, "scripts", "snp_dist_host.cpp"), "-o", so], check=True)
        H = C.CDLL(so)
        H.snp_dist_host.argtypes = [v, v, C.c_int, C.c_long, v, C.c_int]
        host = np.zeros((n, n), np.int32)
        times = []
        for rep in range(6):
            t0 = time.perf_counter()
            H.snp_dist_host(planes[0].ctypes.data_as(v), planes[1].ctypes.data_as(v), n, words, host.ctypes.data_as(v), 16)
            times.append(time.perf_counter() - t0)
    assert np.array_equal(host, dist), "SnpDist and the host loop disagree"
    res["host_loop_16_threads_s"] = times[1:]
    dist_ms = sorted(r["phases_ms"]["snp_dist"] for r in res["runs"])
    pair_words = n * (n - 1) // 2 * words
    res["dist"] = dict(words=words, pair_words=pair_words, kernel_ms=dist_ms, host_over_kernel=sorted(times[1:])[2] / (dist_ms[2] / 1e3),
                       pair_words_per_s=pair_words / (dist_ms[2] / 1e3))
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("counts", "dist")}))


def inputs(name, base):
    ref, gs = synth.make(name)
    return synth.write_set(os.path.join(base, "in"), ref, gs)


def product(name, out_path, reps=3):
    base = tempfile.mkdtemp(prefix="snp_measure_")
    rp, qs = inputs(name, base)
    res = dict(build=build_hash(), set=name, snps0=[], snps1=[])
    md5 = set()
    import xmfa_util
    for rep in range(reps):
        for snps in (0, 1):
            out = os.path.join(base, "out%d" % snps)
            kw = dict(snps=1) if snps else {}
            t0 = time.perf_counter()
            rc, _ = driver.run_core(CORE_BIN, rp, qs, out, threads=16, timing=os.path.join(base, "t.json"), **kw)
            wall = time.perf_counter() - t0
            assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
            t = driver.read_timing(os.path.join(base, "t.json"))
            keep = {k: t[k] for k in t if k.startswith("snp_") or k in ("total_s", "output_s", "path_s", "genomes")}
            res["snps%d" % snps].append(dict(keep, wall_s=wall))
            md5.add(xmfa_util.md5(os.path.join(out, "parsnpAligner.xmfa")))
    assert len(md5) == 1, "the XMFA differs between runs"
    res["xmfa_md5"] = md5.pop()
    res["xmfa_bytes"] = os.path.getsize(os.path.join(base, "out1", "parsnpAligner.xmfa"))
    res["base"] = base
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def check(base):
    """the files of <base>/out1 against the scan of its XMFA (a one-off for the large sets: the scan is pure Python)"""
    import snpcols
    out = os.path.join(base, "out1")
    t0 = time.perf_counter()
    names, letters, rows, dist, counts = snpcols.scan_xmfa(os.path.join(out, "parsnpAligner.xmfa"))
    g = driver.read_snps(out)
    ok = g[0] == names and np.array_equal(g[1], letters) and g[2] == rows and np.array_equal(g[3], dist)
    print(json.dumps(dict(agree=bool(ok), counts=counts, scan_s=time.perf_counter() - t0)))
    assert ok


if __name__ == "__main__":
    if sys.argv[1] == "matrix":
        matrix(sys.argv[2])
    elif sys.argv[1] == "product":
        product(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3)
    else:
        check(sys.argv[2])
