"""Cases and checks for the index build by buckets (parsnp_amd/csrc/engine/index_kernels.h), shared by tests/test_index_buckets.py
(kernel emulation) and tests/test_gpu_index_buckets.py (libparsnp_hip.so).  Every case is a reference and a few query genomes searched
whole (one region), with the tunes that make the piece under test run at a small size: `index_bucket_min` = 1 sends every table
through the bucket build (two buckets at least).  check() runs a case with `index_build` = 1 and = 0, both with `index_verify` = 1,
and compares the multi-MUMs of both with the restatement, the events of pm_find_events on the first query's forward strand (rep'
column included; the call builds the index anew, so a second strand would test the same table) of both with each other and with
the restatement, and reads the counts of pm_last_timing.

The seeds of the probe cases were chosen in the emulation with overflow_model(), a restatement in python of the hash and of the
fill's probe runs: which records reach their bucket's end, and whether one of the LAST bucket does (it then wraps to the region's
first slot in IndexOverflow's loop)."""
import os
import sys
import time

import numpy as np

import oracles
from parsnp_amd.binding import Session
from seqgen import mutate, random_seq

BUCKET_BITS = 10          # index_kernels.h: kBucketBits
BUCKET_FILTER_BITS = 14   # ... kBucketFilterBits
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- the rule and the hash, restated
def table_shape(nR, slot_factor=2, filter_factor=8):
    slots = 16
    while slots < slot_factor * nR:
        slots <<= 1
    fbits = 64
    while fbits < filter_factor * nR:
        fbits <<= 1
    ls, lf = slots.bit_length() - 1, fbits.bit_length() - 1
    sb = min(BUCKET_BITS, ls - 1)
    return slots, fbits, sb, lf - (ls - sb)


def qualifies(nR, bucket_min, slot_factor=2, filter_factor=8):
    slots, _, _, fb = table_shape(nR, slot_factor, filter_factor)
    return slots >= bucket_min and 5 <= fb <= BUCKET_FILTER_BITS


def _fmix32(h):
    h ^= h >> 16; h = h * 0x85EBCA6B & M32; h ^= h >> 13; h = h * 0xC2B2AE35 & M32; h ^= h >> 16
    return h


def hash_tag(t):
    lo, hi = t & M32, t >> 32
    a = _fmix32(lo ^ (hi * 0x9E3779B1 & M32))
    b = (_fmix32(a ^ lo ^ 0x68BC21EB) + hi) & M32
    return (b << 32) | a


def canonical_tags(ref, K):
    """canonical tag of every K-mer of an ACGT-only sequence (kernels.h: kmer_tag, rc_tag)"""
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    c = [code[x] for x in ref]
    out = []
    for p in range(len(c) - K + 1):
        f = r = 0
        for i in range(K):
            f |= c[p + i] << (2 * i)
            r |= (3 - c[p + K - 1 - i]) << (2 * i)
        out.append(min(f, r))
    return out


def overflow_model(ref, K, slot_factor=2):
    """-> (records that reach their bucket's end, those of them in the region's last bucket), filling in position order"""
    slots, _, sb, _ = table_shape(len(ref), slot_factor)
    table = {}
    total = last = 0
    over = set()
    for t in canonical_tags(ref, K):
        h = hash_tag(t) & M32 & (slots - 1)
        end = ((h >> sb) + 1) << sb
        while h < end and h in table and table[h] != t:
            h += 1
        if h < end and t not in over:
            table[h] = t
        else:
            over.add(t); total += 1; last += end == slots
    return total, last


# ---------------------------------------------------------------------------------------------- the cases
class Case:
    def __init__(self, name, ref, qs, minsize, tunes=None, overflow=False, bucketed=True, planted=None, min_mums=1):
        self.name, self.ref, self.qs, self.minsize = name, ref, qs, minsize
        self.tunes = dict(tunes or {})
        self.overflow = overflow          # the case is about the overflow list: the share of overflow records is not bounded
        self.bucketed = bucketed          # the one region qualifies
        self.planted = planted or []      # (position, occurrences of its K-mer in either orientation)
        self.min_mums = min_mums


def _queries(rng, ref, n=2):
    return [mutate(rng, ref, sub=0.02, indel=0.002) if g % 2 == 0 else oracles.revcomp(mutate(rng, ref, sub=0.02)) for g in range(n)]


def probe_small():
    """1 000 bases, slot_factor 1: 1 024 slots in two buckets at 96 % load -- probe runs across the bucket's end and the region's end"""
    rng = np.random.default_rng(4101)
    ref = random_seq(rng, 1000)
    return Case("probe_small", ref, _queries(rng, ref), 16, {"slot_factor": 1}, overflow=True)


def probe_default():
    rng = np.random.default_rng(4102)
    ref = random_seq(rng, 3000)
    return Case("probe_default", ref, _queries(rng, ref), 16, overflow=True)


def chains():
    rng = np.random.default_rng(4103)
    ref = bytearray(random_seq(rng, 20000))
    planted = []
    at = 300
    for copies in (2, 3, 64, 65, 200):
        mer = random_seq(rng, 16)
        rc = 3 if copies == 200 else 0
        for i in range(copies + rc):
            ref[at:at + 16] = oracles.revcomp(mer) if i >= copies else mer
            planted.append((at, copies + rc))
            at += 37 + int(rng.integers(0, 9))
    ref = bytes(ref)
    # the first query: for every planted position a base that differs from the one before it in the reference, then the 40 bases
    # from it -- a maximal match that STARTS at the planted position and is longer than its rep', so pm_find_events reports an event
    # with l = the position and rep' of the position in its last column
    q = b"".join(bytes([b"ACGT"[(b"ACGT".index(ref[pos - 1]) + 1) % 4]]) + ref[pos:pos + 40] for pos, _ in planted)
    return Case("chains", ref, [q] + _queries(rng, ref, 1), 16, planted=planted)


def all_n():
    return Case("all_n", b"N" * 20000, [b"N" * 300 + b"ACGTTGCA" * 40, b"ACGGT" * 100], 16, min_mums=0)


def homopolymer():
    return Case("homopolymer", b"A" * 20000, [b"A" * 500 + b"C" + b"A" * 200, b"T" * 700], 16, min_mums=0)


def tandem():
    rng = np.random.default_rng(4104)
    ref = random_seq(rng, 13000) + b"ACGGTCA" * 2000 + random_seq(rng, 13000)
    return Case("tandem", ref, _queries(rng, ref), 16)


def short_seeds(minsize):
    rng = np.random.default_rng(4105 + minsize)
    ref = random_seq(rng, 4000)
    return Case("short_%d" % minsize, ref, _queries(rng, ref), minsize)


def region_end():
    """one bucket plus one slot of positions: 1 025 bases at slot_factor 1 (2 048 slots); the last K - 1 positions start no K-mer"""
    rng = np.random.default_rng(4106)
    ref = random_seq(rng, 1025)
    return Case("region_end", ref, _queries(rng, ref), 16, {"slot_factor": 1})


def tiny_filter():
    """filter_factor 1 beside slot_factor 64: 64 buckets share 1 024 filter bits, 16 a bucket -- under one word, so not bucketed"""
    rng = np.random.default_rng(4107)
    ref = random_seq(rng, 1000)
    return Case("tiny_filter", ref, _queries(rng, ref), 16, {"filter_factor": 1, "slot_factor": 64}, bucketed=False)


def full_list():
    c = probe_small()
    c.name = "full_list"; c.tunes["index_overflow_cap"] = 1
    return c


def all_n_short():
    return Case("all_n_short", b"N" * 4000, [b"N" * 300 + b"ACGTTGCA" * 40, b"ACGGT" * 100], 16, min_mums=0)


def homopolymer_short():
    return Case("homopolymer_short", b"A" * 4000, [b"A" * 500 + b"C" + b"A" * 200, b"T" * 700], 16, min_mums=0)


def tandem_short():
    rng = np.random.default_rng(4108)
    ref = random_seq(rng, 2600) + b"ACGGTCA" * 400 + random_seq(rng, 2600)
    return Case("tandem_short", ref, _queries(rng, ref), 16)


CASES = {f.__name__: f for f in (probe_small, probe_default, chains, all_n, homopolymer, tandem, all_n_short, homopolymer_short, tandem_short, region_end, tiny_filter,
                                 full_list)}
for _m in (5, 11, 15):
    CASES["short_%d" % _m] = (lambda m: lambda: short_seeds(m))(_m)
DEGENERATE = ("all_n", "homopolymer", "tandem")


# ---------------------------------------------------------------------------------------------- running and checking
def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


def run_whole(lib, case, build):
    with Session(lib, [case.ref] + case.qs) as s:
        s.tune("index_build", build); s.tune("index_bucket_min", 1); s.tune("index_verify", 1)
        for k, v in case.tunes.items():
            s.tune(k, v)
        t0 = time.perf_counter()
        got = s.whole(case.minsize)
        return got, dict(s.last_timing()), time.perf_counter() - t0


def events(lib, case, build):
    tune = ["index_build=%d" % build, "index_bucket_min=1"] + ["%s=%d" % kv for kv in case.tunes.items()]
    old = os.environ.get("PARSNP_TUNE")
    os.environ["PARSNP_TUNE"] = ",".join(tune)
    try:
        out = []
        for strand in (0,):
            j, l, n, r = lib.find_events(case.ref, case.qs[0], case.minsize, strand)
            order = np.lexsort((n, j, l))
            out.append((l[order], j[order], n[order], r[order]))
        return out
    finally:
        if old is None:
            del os.environ["PARSNP_TUNE"]
        else:
            os.environ["PARSNP_TUNE"] = old


_WANT = {}      # the restatement's answers: once per case and process


def check(lib, O, case, more_tunes=None):
    """-> (timing of the bucket build, seconds of the two runs)"""
    case.tunes.update(more_tunes or {})
    K = min(max(case.minsize, 1), 16)
    if case.name not in _WANT:
        q = case.qs[0]
        j, l, n, r = oracles.restatement_events(O, case.ref, q, case.minsize)
        r = np.where(r >= K, r, 0)
        order = np.lexsort((n, j, l))
        _WANT[case.name] = (oracles.restatement_multi_mum(O, [case.ref] + case.qs, case.minsize, 1), (l[order], j[order], n[order], r[order]))
    want, want_ev = _WANT[case.name]
    got1, t1, s1 = run_whole(lib, case, 1)
    got0, t0, s0 = run_whole(lib, case, 0)
    assert same(want, got1) and same(want, got0) and len(want[0]) >= case.min_mums, case.name
    ev1, ev0 = events(lib, case, 1)[0], events(lib, case, 0)[0]
    for a, b, c in zip(want_ev, ev1, ev0):
        assert np.array_equal(a, b) and np.array_equal(a, c), case.name
    for pos, occ in case.planted:      # rep' at every planted position: an event starts there (the first query is built so) and carries it
        l, _, n, r = ev1
        at = l == pos
        assert occ > 1 and np.any(at) and np.all(r[at] >= K) and np.all(n[at] > r[at]), (case.name, pos, occ)
    assert t1["index_lost"] == 0 and t0["index_lost"] == 0, (case.name, t1, t0)
    assert t0["index_bucketed"] == 0 and t0["index_overflow"] == 0
    nR = len(case.ref); records = max(nR - K + 1, 0)
    tunes = {k: case.tunes[k] for k in ("slot_factor", "filter_factor") if k in case.tunes}
    assert qualifies(nR, 1, **tunes) == case.bucketed, case.name
    if "index_overflow_cap" in case.tunes:       # the list was full: built again by IndexInsert
        assert t1["index_bucketed"] == 0 and t1["index_overflow"] > case.tunes["index_overflow_cap"], (case.name, t1)
    elif not case.bucketed:
        assert t1["index_bucketed"] == 0 and t1["index_overflow"] == 0, (case.name, t1)
    else:
        assert t1["index_bucketed"] == nR, (case.name, t1)
        if case.overflow:
            assert t1["index_overflow"] > 0, (case.name, t1)
        else:
            assert t1["index_overflow"] <= records / 8, (case.name, t1, records)
    return t1, s1, s0


MIXED_MIN = 16384      # check_mixed: index_bucket_min


def mixed_runs(lib, O, T):
    """test_emu_engine.batch_case with 24 regions of 200 ... 20 200 bases (tables of 512 ... 65 536 slots, bucketed from 16 384 up), by
    both builds -> [(timing, seqs, starts, lens, mins, results)] of build 1 and build 0; batch_case compares with the restatement"""
    log = []

    class Spy(Session):
        def __init__(self, lib_, seqs, *a, **k):
            super().__init__(lib_, seqs, *a, **k)
            self.seqs_ = list(seqs)

        def multi_mum_batch(self, starts, lens, mins):
            self.tune("index_verify", 1)
            out = super().multi_mum_batch(starts, lens, mins)
            log.append((dict(self.last_timing()), self.seqs_, np.asarray(starts).copy(), np.asarray(lens).copy(), np.asarray(mins).copy(), out))
            return out

    keep = T.Session
    T.Session = Spy
    try:
        got = []
        for build in (1, 0):
            rng = np.random.default_rng(4110)
            n = T.batch_case(rng, lib, O, n_regions=24, glen=40000, nq=4, big_minsize=True, tune=("index_bucket_min", MIXED_MIN) if build else ("index_build", 0))
            assert n > 10
            got.append(n)
        assert got[0] == got[1]
    finally:
        T.Session = keep
    return log


def check_mixed(lib, O, T):
    (t1, _, _, lens1, _, _), (t0, _, _, _, _, _) = mixed_runs(lib, O, T)
    q = [qualifies(int(n), MIXED_MIN) for n in lens1[:, 0]]
    assert 0 < sum(q) < len(q)
    assert t1["index_bucketed"] == sum(int(n) for n, ok in zip(lens1[:, 0], q) if ok), t1
    assert t1["index_overflow"] <= t1["index_bucketed"] / 8 and t1["index_lost"] == 0
    assert t0["index_bucketed"] == 0 and t0["index_lost"] == 0


# ---------------------------------------------------------------------------------------------- the one-K-mer cases under a watchdog
# The case runs in a process of its own, first with index_build = 0 -- today's build, the parent's code for the case -- under
# PARENT_LIMIT_S, and the wall time of that process is the parent's time.  Then with index_build = 1 under a time limit of the
# parent's time + WATCHDOG_MARGIN_S: a fill that does not end, or one that pays per occurrence what today's build does not, is killed
# and fails the test.  The margin covers what varies between two processes that do the same: interpreter and library start (0.3 s
# here), the first load of a kernel, a host that other work loads -- 3 s is ten times the start-up and well under any of the limits.
PARENT_LIMIT_S = 120
WATCHDOG_MARGIN_S = 3.0


def watchdog(lib_path, name, more_tunes=None):
    """-> (wall seconds by IndexInsert, by buckets), or raises AssertionError naming what did not come back"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")]))
    tunes = ["%s=%d" % kv for kv in (more_tunes or {}).items()]
    wall = []
    for build, limit in ((0, PARENT_LIMIT_S), (1, None)):
        limit = limit if limit is not None else wall[0] + WATCHDOG_MARGIN_S
        t0 = time.perf_counter()
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "timed", name, lib_path, str(build)] + tunes, capture_output=True, text=True, env=env, timeout=limit)
        except subprocess.TimeoutExpired:
            raise AssertionError("%s with index_build = %d did not come back in %.1f s (today's build: %s s)" % (name, build, limit, wall[:1]))
        wall.append(time.perf_counter() - t0)
        assert p.returncode == 0 and "timed ok" in p.stdout, (name, build, p.returncode, p.stdout[-800:], p.stderr[-2000:])
    return wall[0], wall[1]


def write_cases(path, lib, O, T):
    """the cases as a text file for tests/emu/index_buckets_check.cpp: tunes, genomes, regions, the multi-MUMs the restatement gives and the
    counts the emulation reports -- every case of CASES (the 20 000-base one-K-mer cases with work_budget 2^14: under the sanitizers their
    quadratic walks at the default budget take minutes) and the mixed batch"""
    with open(path, "w") as f:
        def put(name, tunes, seqs, starts, lens, mins, results, t1):
            f.write("CASE %s %d %d %d %d %d\n" % (name, len(tunes), len(seqs), len(mins), int(t1["index_bucketed"]), int(t1["index_overflow"])))
            for kv in tunes.items():
                f.write("%s %d\n" % kv)
            for s in seqs:
                f.write(s.decode() + "\n")
            for r in range(len(mins)):
                k, lon, sp, fw = results[r][:4]
                f.write("%d %s %s %d\n" % (mins[r], " ".join(map(str, starts[r])), " ".join(map(str, lens[r])), len(k)))
                for c in range(len(k)):
                    f.write("%d %d %s %s\n" % (k[c], lon[c], " ".join(map(str, sp[c])), " ".join(map(str, fw[c]))))
        for name, make in CASES.items():
            case = make()
            if name in DEGENERATE:
                case.tunes["work_budget"] = 1 << 14
            want = oracles.restatement_multi_mum(O, [case.ref] + case.qs, case.minsize, 1)
            _, t1, _ = run_whole(lib, case, 1)
            seqs = [case.ref] + case.qs
            put(name, dict(case.tunes, index_bucket_min=1), seqs, [[0] * len(seqs)], [[len(s) for s in seqs]], [case.minsize], [want], t1)
        (t1, seqs, starts, lens, mins, results), _ = mixed_runs(lib, O, T)
        put("mixed", {"index_bucket_min": MIXED_MIN}, seqs, starts, lens, mins, results, t1)


def main(argv):
    """`python tests/indexgen.py timed CASE LIB BUILD [key=value ...]`: one search of one case by one build, for watchdog()"""
    from parsnp_amd.binding import Lib
    assert argv[1] == "timed"
    case = CASES[argv[2]]()
    case.tunes.update({kv.split("=")[0]: int(kv.split("=")[1]) for kv in argv[5:]})
    _, t, s = run_whole(Lib(argv[3]), case, int(argv[4]))
    assert t["index_lost"] == 0, t
    print("%s index_build %s: %.3f s, %d positions by buckets, %d overflow records\ntimed ok" % (argv[2], argv[4], s, t["index_bucketed"], t["index_overflow"]))


if __name__ == "__main__":
    main(sys.argv)
