"""Measurements of the recombination scan (profiles/rec/README.md) on one MI355X.

  python scripts/rec_measure.py product SET OUT.json [N]   parsnp_core on a synth set (bact200) with snps=1 and recomb=1 in turn, N whole
                                                           processes each (default 3): rec_ms and the counts of PARSNP_TIMING; the
                                                           two files of the last run are checked against tests/recphi of its
                                                           .snps.mfa / .snps.tsv; OUT.json names the run's output directory
  python scripts/rec_measure.py kernels OUT.json [OUTDIR]  the defaults (K = 100, H = 10, P = 1000, seed 1) over a designed collection
                                                           of 2 048 rows x 100 000 core SNP columns in one LCB (1 999 windows) and,
                                                           with the output directory of a product run, over that run's collection:
                                                           the phases rec_sites, rec_incompat and rec_permute of pm_last_timing (5
                                                           calls each after a warm-up; rec_sites once per fresh collection), and
                                                           scripts/rec_host.cpp with 16 threads on the same letters, whose phi and
                                                           le must be the device's
"""
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import recphi                                           # noqa: E402
from parsnp_amd import driver, synth                    # noqa: E402
from parsnp_amd.binding import Lib, Session             # noqa: E402
from parsnp_amd.paths import CORE_BIN                   # noqa: E402

K, H, P, SEED, THREADS = 100, 10, 1000, 1, 16
HOST_BIN = os.path.join(ROOT, "parsnp_amd", "bin", "rec_host")
# 256 CUs x 4 SIMDs at 2.4 GHz; cycles per wave64 integer instruction and SIMD as scripts/valu_calib.hip measured
SIMDS, CUS, HZ, CYCLES_PER_INSTR = 1024, 256, 2.4e9, 2.2
# vector instructions of RecIncompat per (pair, row word), read in the gfx950 ISA of its inner loop (profiles/rec/README.md)
INSTR_PER_PAIR_WORD = 86
# LDS cycles of RecPermute per permutation of a window of k sites: per key of the rank loop one broadcast ds_read_b64 per slot of 64
# sites (1 lane group: 1 cycle each, the compare chain behind it is not LDS), per look-up of T two ds_read_u8 of the order and one of
# the matrix (scattered bytes: 64 lanes over 64 banks, up to 1 cycle per lane group of 16 -> 4 cycles an instruction)
LDS_CYCLES = lambda k, h: -(-k // 64) * k * 1 + sum(-(-(k - d) // 64) for d in range(1, h + 1)) * 3 * 4      # noqa: E731


def med(xs):
    return sorted(xs)[len(xs) // 2]


def host_binary():
    src = os.path.join(ROOT, "scripts", "rec_host.cpp")
    if not os.path.exists(HOST_BIN) or os.path.getmtime(HOST_BIN) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(HOST_BIN), exist_ok=True)
        subprocess.run(["g++", "-O3", "-march=x86-64-v3", "-std=c++17", "-fopenmp", src, "-o", HOST_BIN], check=True)
    return HOST_BIN


def run_host(letters, cluster):
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        f.write(struct.pack("<qq", *letters.shape))
        f.write(np.ascontiguousarray(letters).tobytes())
        f.write(np.ascontiguousarray(cluster, np.int32).tobytes())
    try:
        runs = [json.loads(subprocess.run([host_binary(), f.name, str(K), str(H), str(P), str(SEED), str(THREADS)], check=True, capture_output=True, text=True).stdout)
                for _ in range(3)]
    finally:
        os.unlink(f.name)
    return runs


def device(lib, letters, cluster, fresh=3):
    n, nv = letters.shape
    t = dict(rec_sites=[], rec_incompat=[], rec_permute=[])
    with Session(lib, [b"ACGTTGCAAGGCTTAACCGGTACGATCGATTACGGCAT" * 4] * 2) as s:
        s.core_snps([recphi.random_letters(8, 200, 1)])
        s.rec_sites()      # (the warm-up of the two kernels of rec_sites: code objects)
        for _ in range(fresh):
            assert s.core_snps([letters])[0]["core_snps"] == nv
            flags = s.rec_sites()
            t["rec_sites"].append(dict(s.last_timing()).get("rec_sites", 0.0))
        rows = [(int(c), i, i) for i, c in enumerate(cluster)]
        sites, off = [], [0]
        for a, b in recphi.lcb_runs(rows):
            inf = [c for c in range(a, b) if flags[c]]
            for st, k in recphi.windows_of(len(inf), K):
                sites += inf[st:st + k]
                off.append(len(sites))
        sites, off = np.array(sites, np.int64), np.array(off, np.int64)
        import ctypes as C
        v = C.c_void_p
        L = lib.L
        L.pm_rec_incompat.argtypes = [v, C.c_int64, v, C.c_int64, v, v]
        phi = le = None
        for rep in range(6):
            lib._check(L.pm_rec_incompat(s.h, len(sites), sites.ctypes.data_as(v), len(off) - 1, off.ctypes.data_as(v), None))      # (nothing is downloaded)
            a = dict(s.last_timing())
            t0 = time.perf_counter()
            phi, le = s.rec_test(off, H, P, SEED)
            wall = (time.perf_counter() - t0) * 1e3
            b = dict(s.last_timing())
            if rep:
                t["rec_incompat"].append(a.get("rec_incompat", 0.0)); t["rec_permute"].append(b.get("rec_permute", 0.0))      # noqa: E702
                t.setdefault("rec_test_wall", []).append(wall)
    ks = np.diff(off)
    pair_words = float((ks * (ks - 1) // 2).sum()) * ((n + 63) // 64)
    # (a wavefront computes the whole 8 x 8 tile on the diagonal and pads the last tile: the bound counts the pairs that are asked for)
    inc_bound = pair_words * INSTR_PER_PAIR_WORD / 64 * CYCLES_PER_INSTR / (SIMDS * HZ) * 1e3
    hs = np.minimum(H, ks - 1)
    lds_bound = sum((P + 1) * LDS_CYCLES(int(k), int(h)) for k, h in zip(ks, hs)) / (CUS * HZ) * 1e3
    r = {k: sorted(x) for k, x in t.items()}
    r.update(n=n, core_snps=nv, informative=int(flags.sum()), windows=len(ks), flagged=int(sum(recphi.flagged(int(x), P) for x in le)), sum_phi=int(phi.sum()), sum_le=int(le.sum()),
             incompat_issue_bound_ms=inc_bound, incompat_over_bound=med(t["rec_incompat"]) / inc_bound if inc_bound else None,
             permute_lds_bound_ms=lds_bound, permute_over_bound=med(t["rec_permute"]) / lds_bound if lds_bound else None,
             rec_ms=med(t["rec_sites"]) + med(t["rec_incompat"]) + med(t["rec_permute"]))
    return r, phi, le


def designed(n, v):
    """n x v random letters, every column a core SNP (rows 0 and 1 differ)"""
    rng = np.random.default_rng(1)
    code = rng.integers(0, 4, (n, v), dtype=np.uint8)
    code[1] = (code[0] + rng.integers(1, 4, v, dtype=np.uint8)) % 4
    return np.frombuffer(b"ACGT", np.uint8)[code]


def kernels(out_path, outdir=None):
    lib = Lib()
    sets = {"designed2048": (designed(2048, 100_000), np.ones(100_000, np.int32))}
    if outdir:
        _, letters, rows, _ = driver.read_snps(outdir)
        sets["file%d" % letters.shape[0]] = (letters, np.array([r[0] for r in rows], np.int32))
    res = {}
    for name, (letters, cluster) in sets.items():
        r, phi, le = device(lib, letters, cluster, 2 if letters.shape[0] > 1000 else 3)
        host = run_host(letters, cluster)
        for h in host:
            assert (h["windows"], h["informative"], h["sum_phi"], h["sum_le"], h["flagged"]) == (r["windows"], r["informative"], r["sum_phi"], r["sum_le"], r["flagged"]), (h, r)
        hm = {k: med([h[k] for h in host]) for k in ("sites_ms", "incompat_ms", "permute_ms")}
        r.update(host_runs=host, host_ms=hm, host_total_ms=sum(hm.values()), host_over_device=sum(hm.values()) / r["rec_ms"] if r["rec_ms"] else None)
        res[name] = r
        print(name, json.dumps({k: v for k, v in r.items() if k != "host_runs"}), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)


def product(name, out_path, reps=3):
    base = tempfile.mkdtemp(prefix="rec_measure_")
    ref, gs = synth.make(name)
    rp, qs = synth.write_set(os.path.join(base, "in"), ref, gs)
    res = dict(set=name, snps=[], rec=[])
    for rep in range(reps):
        for tag, kw in (("snps", dict(snps=1)), ("rec", dict(recomb=1))):
            out = os.path.join(base, "out_" + tag)
            t0 = time.perf_counter()
            rc, _ = driver.run_core(CORE_BIN, rp, qs, out, threads=THREADS, timing=os.path.join(base, "t.json"), **kw)
            wall = time.perf_counter() - t0
            assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
            t = driver.read_timing(os.path.join(base, "t.json"))
            res[tag].append(dict({k: t[k] for k in t if k.startswith("rec_") or k in ("total_s", "output_s", "snp_core", "snp_dist_ms")}, wall_s=wall))
    out = os.path.join(base, "out_rec")
    _, letters, rows, _ = driver.read_snps(out)
    t0 = time.perf_counter()
    recs, n_inf = recphi.scan(letters, rows)
    tsv, bed = recphi.files_text(recs)
    res["restatement_s"] = time.perf_counter() - t0
    assert open(os.path.join(out, "parsnpAligner.rec.tsv")).read() == tsv and open(os.path.join(out, "parsnpAligner.rec")).read() == bed, "the files are not the restatement's"
    for f in ("parsnpAligner.xmfa", "parsnpAligner.snps.mfa", "parsnpAligner.snps.tsv", "parsnpAligner.snps.dist"):
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(base, "out_snps", f), "rb").read(), f
    res.update(outdir=out, rows=int(letters.shape[0]), core_snps=int(letters.shape[1]), informative=n_inf, windows=len(recs), flagged=sum(r["flagged"] for r in recs),
               lcbs=len(recphi.lcb_runs(rows)))
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if sys.argv[1] == "kernels":
        kernels(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        product(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3)
