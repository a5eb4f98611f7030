"""Measurements of the LCB extension (profiles/ext/README.md) on one MI355X.

  python scripts/ext_measure.py product SET OUT.json [N] [KEY=VALUE ...]
                                                           parsnp_core on a synth set (bact200) without the key and with lcbext=1 in turn, N
                                                           whole processes each (default 3): ext_ms and the counts of PARSNP_TIMING, total_s,
                                                           the wall clock; every other file of the two runs must have the same bytes;
                                                           OUT.json names the run's input and output directories.  KEY=VALUE: further
                                                           arguments of driver.ini_text for both runs (clusterd=60 ends an LCB at every gap
                                                           of more than 60 bases between MUMs: many LCBs with homologous flanks)
  python scripts/ext_measure.py kernels OUT.json [OUT_OF_PRODUCT.json]
                                                           the defaults over a designed set of 64 jobs of 2 048 rows with flanks of 256
                                                           bases and, with the record of a product run, over the jobs of that run's
                                                           XMFA: the phases ext_reach, ext_cut, ext_trace, ext_merge of pm_last_timing
                                                           (5 calls each after a warm-up), and scripts/ext_host.cpp with 16 threads on
                                                           the same flanks, whose reaches, columns, j_r and rows must be the device's
  python scripts/ext_measure.py counters                   two calls of either entry point over the designed set: the program of a counter
                                                           collection (rocprofv3 --pmc ... -- python scripts/ext_measure.py counters)
"""
import bisect
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import lcbext                                           # noqa: E402
from parsnp_amd import driver, synth                    # noqa: E402
from parsnp_amd.binding import Lib, Session             # noqa: E402
from parsnp_amd.paths import CORE_BIN                   # noqa: E402

THREADS = 16
HOST_BIN = os.path.join(ROOT, "parsnp_amd", "bin", "ext_host")
PHASES = ("ext_reach", "ext_cut", "ext_trace", "ext_merge")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_RUN = re.compile(b"[ACGT]*")


def med(xs):
    return sorted(xs)[len(xs) // 2]


def host_binary():
    src = os.path.join(ROOT, "scripts", "ext_host.cpp")
    if not os.path.exists(HOST_BIN) or os.path.getmtime(HOST_BIN) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(HOST_BIN), exist_ok=True)
        subprocess.run(["g++", "-O3", "-march=x86-64-v3", "-std=c++17", "-fopenmp", src, "-o", HOST_BIN], check=True)
    return HOST_BIN


def letters_of(genomes, rows):
    out = []
    for g, step, comp, n, first in rows:
        s = genomes[g][first:first + n] if step == 1 else genomes[g][first - n + 1:first + 1][::-1] if n else b""
        out.append(s.translate(_COMP) if comp else s)
    return out


def run_host(p, row_off, flanks):
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        f.write(struct.pack("<7i", *lcbext.key_of(p)))
        f.write(struct.pack("<q", len(row_off) - 1))
        f.write(np.ascontiguousarray(row_off, np.int64).tobytes())
        f.write(np.array([len(x) for x in flanks], np.int32).tobytes())
        f.write(b"".join(flanks))
    try:
        return [json.loads(subprocess.run([host_binary(), f.name, str(THREADS)], check=True, capture_output=True, text=True).stdout) for _ in range(3)]
    finally:
        os.unlink(f.name)


def fnv(blocks):
    """the position-weighted byte sum of scripts/ext_host.cpp over the rows of every kept job in order"""
    kept = [np.ascontiguousarray(b).ravel() for b in blocks if b is not None]
    if not kept:
        return "%016x" % 0
    a = np.concatenate(kept).astype(np.uint64)
    w = (np.arange(len(a), dtype=np.uint64) % np.uint64(65521)) + np.uint64(1)
    return "%016x" % int((a * w).sum(dtype=np.uint64))


def device(lib, genomes, p, row_off, rows, reps=6):
    t = {k: [] for k in PHASES}
    wall = dict(reach=[], align=[])
    rec = np.array([tuple(r) for r in rows], Session.EXT_ROW)
    with Session(lib, genomes) as s:
        for rep in range(reps):
            t0 = time.perf_counter()
            reach = s.ext_reach(row_off, rec, p)
            t1 = time.perf_counter()
            a = dict(s.last_timing())
            cols, used, blocks = s.ext_align(row_off, rec, reach, p)
            t2 = time.perf_counter()
            a.update(dict(s.last_timing()))
            if rep:      # (the first call loads the code objects)
                for k in PHASES:
                    t[k].append(a.get(k, 0.0))
                wall["reach"].append((t1 - t0) * 1e3); wall["align"].append((t2 - t1) * 1e3)      # noqa: E702
    r = {k: sorted(v) for k, v in t.items()}
    r.update(wall_ms={k: sorted(v) for k, v in wall.items()}, ext_ms=sum(med(t[k]) for k in PHASES), jobs=len(row_off) - 1, pairs=len(rows),
             sum_reach=int(reach.sum()), kept=int((cols > 0).sum()), wide=int((cols < 0).sum()), sum_cols=int(np.maximum(cols, 0).sum()), sum_used=int(used.sum()))
    return r, blocks


def designed(n_rows=2048, n_jobs=64, F=256):
    """jobs of n_rows rows whose flanks are 16 variants of the job's reference flank (identity about 97 %, some with an indel), laid
    down in 8 genomes"""
    rng = np.random.default_rng(1)
    pool = lcbext.Pool(8, seed=1)
    jobs = []
    for j in range(n_jobs):
        base = lcbext.rand_seq(rng, F)
        var = [base] + [lcbext.mutate(rng, base, subs=8, dels=[(40 + 9 * k, k % 4)] if k % 3 == 0 else (), inss=[(150, k % 5)] if k % 4 == 1 else ())[:F] for k in range(1, 16)]
        jobs.append([pool.row(var[r % 16 if r else 0], mode=r % 4) for r in range(n_rows)])
    return pool.genomes(), jobs


def read_fasta(path):
    return b"".join(l.strip() for l in open(path, "rb") if not l.startswith(b">")).upper()


def jobs_of_run(xmfa, indir, F):
    """the descriptors of every job of an XMFA of single-contig genomes (tests/lcbext.jobs_of, with interval lists instead of bit maps)"""
    head, lcbs = lcbext.read_xmfa(xmfa)
    names = [h.split(" ", 1)[1] for h in head if h.startswith("##SequenceFile ")]
    genomes = [read_fasta(os.path.join(indir, n)) for n in names]
    iv = [[] for _ in genomes]
    for recs in lcbs:
        for seq, lo, hi, _, _ in recs:
            if lo <= hi:
                iv[seq - 1].append((lo - 1, hi))
    starts, ends = [], []
    for g, v in enumerate(iv):
        v.sort()
        m = []
        for a, b in v:
            if m and a <= m[-1][1]:
                m[-1][1] = max(m[-1][1], b)
            else:
                m.append([a, b])
        starts.append([a for a, _ in m]); ends.append([b for _, b in m])      # noqa: E702
    jobs = []
    for recs in lcbs:
        for side in "LR":
            rows = []
            for seq, lo, hi, strand, _ in recs:
                g, glen = seq - 1, len(genomes[seq - 1])
                up = (side == "R") == (strand == "+")
                first, n = (hi if up else lo - 2), 0
                if 0 <= first < glen:
                    k = bisect.bisect_right(ends[g], first)      # the first covered stretch that ends after `first`
                    if not (k < len(starts[g]) and starts[g][k] <= first):
                        if up:
                            run = (starts[g][k] if k < len(starts[g]) else glen) - first
                            avail = min(F, (run + 1) // 2 if k < len(starts[g]) else run)
                            n = _RUN.match(genomes[g], first, first + avail).end() - first
                        else:
                            run = first + 1 - (ends[g][k - 1] if k else 0)
                            avail = min(F, run // 2 if k else run)
                            n = len(_RUN.match(genomes[g][first - avail + 1:first + 1][::-1]).group())
                rows.append((g, 1 if up else -1, int(strand == "-"), n, first if n else 0))
            jobs.append(rows)
    return genomes, jobs


def measure(lib, name, genomes, jobs, p):
    row_off = np.concatenate(([0], np.cumsum([len(j) for j in jobs]))).astype(np.int64)
    rows = [r for j in jobs for r in j]
    r, blocks = device(lib, genomes, p, row_off, rows)
    r["rows_hash"] = fnv(blocks)
    host = run_host(p, row_off, letters_of(genomes, rows))
    for h in host:
        same = ("jobs", "pairs", "sum_reach", "kept", "wide", "sum_cols", "sum_used", "rows_hash")
        assert all(h[k] == r[k] for k in same), ({k: h[k] for k in same}, {k: r[k] for k in same})
    hm = {k: med([h[k] for h in host]) for k in ("reach_ms", "align_ms")}
    r.update(host_runs=host, host_ms=hm, host_total_ms=sum(hm.values()), host_over_device=sum(hm.values()) / r["ext_ms"] if r["ext_ms"] else None)
    print(name, json.dumps({k: v for k, v in r.items() if k != "host_runs"}), flush=True)
    return r


def kernels(out_path, product_json=None):
    lib = Lib()
    p = lcbext.params()
    res = {}
    genomes, jobs = designed()
    res["designed2048"] = measure(lib, "designed2048", genomes, jobs, p)
    if product_json:
        rec = json.load(open(product_json))
        genomes, jobs = jobs_of_run(os.path.join(rec["outdir"], "parsnpAligner.xmfa"), rec["indir"], p["max_flank"])
        res["file%d" % len(genomes)] = measure(lib, "file%d" % len(genomes), genomes, jobs, p)
        t = rec["ext"][-1]
        r = res["file%d" % len(genomes)]
        assert (t["ext_jobs"], t["ext_kept"], t["ext_wide"], t["ext_bases"]) == (r["jobs"], r["kept"], r["wide"], r["sum_reach"] - 0), (t, r["jobs"], r["kept"], r["wide"], r["sum_reach"])
    json.dump(res, open(out_path, "w"), indent=1)


def product(name, out_path, reps=3, extra=None):
    base = tempfile.mkdtemp(prefix="ext_measure_")
    ref, gs = synth.make(name)
    rp, qs = synth.write_set(os.path.join(base, "in"), ref, gs)
    res = dict(set=name, extra=extra or {}, plain=[], ext=[])
    for rep in range(reps):
        for tag, kw in (("plain", dict(extra or {})), ("ext", dict(extra or {}, lcbext=1))):
            out = os.path.join(base, "out_" + tag)
            t0 = time.perf_counter()
            rc, _ = driver.run_core(CORE_BIN, rp, qs, out, threads=THREADS, timing=os.path.join(base, "t.json"), **kw)
            wall = time.perf_counter() - t0
            assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
            t = driver.read_timing(os.path.join(base, "t.json"))
            res[tag].append(dict({k: t[k] for k in t if k.startswith("ext_") or k in ("total_s", "output_s")}, wall_s=wall))
    o1, o2 = os.path.join(base, "out_plain"), os.path.join(base, "out_ext")
    for f in sorted(os.listdir(o1)):
        if f not in ("parsnp-aligner.err", "parsnp-aligner.out", "parsnpAligner.log", "parsnpAligner.ini"):
            assert open(os.path.join(o1, f), "rb").read() == open(os.path.join(o2, f), "rb").read(), f
    head, jobs = driver.read_extended(o2)
    res.update(outdir=o2, indir=os.path.join(base, "in"), rows=len(gs) + 1, kept_jobs=len(jobs), extended_bytes=os.path.getsize(os.path.join(o2, "parsnpAligner.xmfa.extended")),
               xmfa_bytes=os.path.getsize(os.path.join(o2, "parsnpAligner.xmfa")), genome_bases=len(ref))
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def counters():
    """two calls of either entry point over the designed set and nothing else: the program to run under a counter collection
    (rocprofv3 --pmc ... -- python scripts/ext_measure.py counters), a run of its own"""
    lib = Lib()
    genomes, jobs = designed()
    row_off = np.concatenate(([0], np.cumsum([len(j) for j in jobs]))).astype(np.int64)
    rec = np.array([tuple(r) for j in jobs for r in j], Session.EXT_ROW)
    with Session(lib, genomes) as s:
        for _ in range(2):
            reach = s.ext_reach(row_off, rec, lcbext.params())
            s.ext_align(row_off, rec, reach, lcbext.params())


if __name__ == "__main__":
    if sys.argv[1] == "counters":
        counters()
    elif sys.argv[1] == "kernels":
        kernels(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        product(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3, {a.split("=")[0]: int(a.split("=")[1]) for a in sys.argv[5:]})
