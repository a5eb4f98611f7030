"""The LCB extension (pm_ext_reach, pm_ext_align; ext_kernels.h) against the numpy restatement of tests/lcbext.py, in the kernel
emulation; tests/test_gpu_lcb_extend.py runs the same checks on the device.  Line maxima, reaches, j_r and column counts are compared
as integers, the rows and .xmfa.extended as bytes.  No tolerances.

One case of the issue's list cannot occur under the definition: a row never inserts in slot A.  The path ends at the SMALLEST j that
holds the maximum of line A, and a left move into that cell would make H(A, j) = H(A, j - 1) - G < H(A, j - 1) (G >= 1), so the
cell would not hold the maximum.  check_paths asserts ins(A) == 0 for every row instead, and exercises slot 0, a middle slot and
slot A - 3."""
import functools
import os

import numpy as np
import pytest

import lcbext as X
from parsnp_amd.binding import Lib, PmError, Session


@pytest.fixture(scope="module")
def lib(emu):
    return Lib(emu[0])


def same_ints(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = tuple(int(x) for x in np.argwhere(got != want)[0])
        raise AssertionError("%s: entry %r is %d, restatement %d (%d differ)" % (what, at, got[at], want[at], int((got != want).sum())))


def run_jobs(s, genomes, jobs, p, best=False, **kw):
    """jobs: a list of lists of descriptors.  Runs both entry points and compares everything with the restatement; -> its results"""
    row_off = np.concatenate(([0], np.cumsum([len(j) for j in jobs]))).astype(np.int64)
    rows = [r for j in jobs for r in j]
    want = [X.job([X.read_row(genomes, r) for r in j], p) for j in jobs]
    got = s.ext_reach(row_off, rows, p, best=best)
    if best:
        got, table = got
        same_ints(table, np.concatenate([np.stack(w["best"]) for w in want]), "best")
    same_ints(got, [w["reach"] for w in want], "reach")
    cols, used, blocks = s.ext_align(row_off, rows, got, p, **kw)
    same_ints(cols, [w["cols"] for w in want], "cols")
    same_ints(used, [u for w in want for u in w["used"]], "used")
    for j, (w, blk) in enumerate(zip(want, blocks)):
        assert (blk is None) == (w["rows"] is None), j
        if blk is not None:
            for r, (x, y) in enumerate(zip(blk, w["rows"])):
                assert x.tobytes() == y, "job %d row %d: %r, restatement %r" % (j, r, x.tobytes(), y)
    return want


# ------------------------------------------------------------------------------------------------------- tables
TABLES = [(W, F, sc) for W in (1, 31, 32, 63) for F, sc in ((16, (1, 1, 1)), (512, (5, 4, 2)))] + [(32, 512, (1, 1, 1)), (63, 16, (5, 4, 2))]


@functools.lru_cache(maxsize=None)
def table_case(W, F, scores):
    rng = np.random.default_rng(1000 * W + F)
    p = X.params(band=W, max_flank=F, match=scores[0], mismatch=scores[1], gap=scores[2], ani=60, min_len=1)
    pool = X.Pool(3, seed=W + F)
    base = X.rand_seq(rng, F)
    var = X.mutate(rng, base, subs=F // 16)
    lens = sorted({n for n in (0, 1, 2, W, W + 1, F) if n <= F})
    jobs = [[pool.row(base[:la]), pool.row(var[:lb])] for la in lens for lb in lens if la != lb]
    for k in (W, W + 1):      # an indel of exactly W and of W + 1 bases, either way, near the start and past the middle
        for at in (3, F // 2 + 1):
            if at + k < F:
                gone = X.mutate(rng, base, dels=[(at, k)])
                more = X.mutate(rng, base, inss=[(at, k)])[:F]
                jobs += [[pool.row(base), pool.row(gone)], [pool.row(gone), pool.row(base)], [pool.row(base), pool.row(more)]]
    return p, pool.genomes(), jobs


def check_tables(lib, W, F, scores):
    p, genomes, jobs = table_case(W, F, scores)
    assert len(jobs) >= 12
    with Session(lib, genomes) as s:
        want = run_jobs(s, genomes, jobs, p, best=True)
    assert any(w["reach"] == 0 for w in want) and (F == 16 and W > 16 or any(w["reach"] > 0 for w in want))
    return want


@pytest.mark.parametrize("W,F,scores", TABLES)
def test_tables(lib, W, F, scores):
    check_tables(lib, W, F, scores)


# ------------------------------------------------------------------------------------------------------- rows
ROWS = (2, 3, 63, 64, 65, 2048)


@functools.lru_cache(maxsize=None)
def rows_case(n):
    """per failing index one job in which that row alone stops the others' reach; one job without such a row"""
    rng = np.random.default_rng(n)
    pool = X.Pool(4, seed=n)
    base = X.rand_seq(rng, 120)
    good = [base] + [X.mutate(rng, base, subs=k % 3) for k in range(1, 6)]
    bad = base[:40] + X.rand_seq(rng, 80)      # like the others for 40 bases
    jobs, fails = [], [i for i in (1, 63, 64, n - 1) if i < n]
    for f in sorted(set(fails)) + [None]:
        jobs.append([pool.row(bad if r == f else good[r % len(good) if r else 0], mode=r % 4) for r in range(n)])
    return pool.genomes(), jobs, len(set(fails))


def check_rows(lib, n):
    genomes, jobs, nf = rows_case(n)
    p = X.params(max_flank=128)
    with Session(lib, genomes) as s:
        want = run_jobs(s, genomes, jobs, p)
        reach = [w["reach"] for w in want]
        assert all(40 <= a < 60 for a in reach[:nf]) and reach[nf] == 120, reach
        # A = L - 1 against A = L: the same jobs with min_len one above and exactly at the first job's reach
        A = reach[0]
        over = run_jobs(s, genomes, jobs[:1], X.params(max_flank=128, min_len=A + 1))
        at = run_jobs(s, genomes, jobs[:1], X.params(max_flank=128, min_len=A))
        assert over[0]["reach"] == 0 and over[0]["cols"] == 0 and at[0]["reach"] == A


@pytest.mark.parametrize("n", ROWS)
def test_rows(lib, n):
    check_rows(lib, n)


# ------------------------------------------------------------------------------------------------------- batches
@functools.lru_cache(maxsize=None)
def batch_case(n_jobs):
    rng = np.random.default_rng(n_jobs)
    pool = X.Pool(5, seed=n_jobs)
    bases = [X.rand_seq(rng, 64) for _ in range(4)]
    jobs = []
    for j in range(n_jobs):
        base = bases[j % 4]
        n = (2, 3, 5, 9, 2, 4)[j % 6]
        la = (64, 30, 17, 64, 1, 45)[j % 6]
        rows = [pool.row(base[:la])]
        for r in range(1, n):
            kind = (j + r) % 5
            b = base[:(64, 50, 33, 64, 20)[kind]]
            if kind == 1:
                b = X.mutate(rng, b, dels=[(12, 3)])
            elif kind == 2:
                b = X.mutate(rng, b, inss=[(10, 2 + r % 3)])
            elif kind == 3 and j % 7 == 3:
                b = X.rand_seq(rng, 64)      # nothing in common: reach 0
            rows.append(pool.row(b))
        jobs.append(rows)
    return pool.genomes(), jobs


def check_batches(lib, n_jobs=257):
    """ext_batch 1, 3 and 7 (a job's pairs straddle launches; jobs have 2 ... 9 rows) give what the default gives"""
    genomes, jobs = batch_case(n_jobs)
    p = X.params(max_flank=64, band=20, ani=80)
    names = []
    for k in (0, 1, 3, 7) if n_jobs > 2 else (0, 1):
        with Session(lib, genomes) as s:
            s.tune("ext_batch", k)
            want = run_jobs(s, genomes, jobs, p)
            names += [x for x, _ in s.last_timing()]
            s.ext_reach([0, 2], jobs[0][:2], p)
            names += [x for x, _ in s.last_timing()]
    if n_jobs == 257:
        cols = [w["cols"] for w in want]
        assert any(a > 0 and b == 0 and c > 0 for a, b, c in zip(cols, cols[1:], cols[2:]))      # a reach-0 job between kept ones
    return names


@pytest.mark.parametrize("n_jobs", [1, 2, 257])
def test_batches(lib, n_jobs):
    check_batches(lib, n_jobs)


@pytest.mark.parametrize("launch", ["ext_reach", "ext_cut", "ext_trace", "ext_width", "ext_merge"])
def test_wavefronts_of_a_launch_do_not_depend_on_one_another(lib, launch, monkeypatch):
    monkeypatch.setenv("PM_EMU_REVERSE_WAVES", launch)
    check_batches(lib, 2)
    check_paths(lib)


# ------------------------------------------------------------------------------------------------------- paths and columns
@functools.lru_cache(maxsize=None)
def paths_case():
    rng = np.random.default_rng(77)
    pool = X.Pool(3, seed=77)
    base = X.rand_seq(rng, 60)
    jobs, p = [], X.params(max_flank=64, band=20, ani=70, min_len=20)
    def put(at, k):      # k equal letters that differ from both neighbours: the insertion cannot slide to another slot
        letter = [c for c in b"ACGT" if c not in (base[at - 1] if at else 0, base[at])][0]
        return (base[:at] + bytes([letter]) * k + base[at:])[:64]
    for at in (0, 25, 57):      # two rows insert different lengths in one slot: slot 0, a middle one, one near the end (not slot A: see above)
        jobs.append([pool.row(base), pool.row(put(at, 2)), pool.row(put(at, 5)), pool.row(base)])
    jobs.append([pool.row(base), pool.row(X.mutate(rng, base, dels=[(7, 3), (30, 1), (44, 6)])), pool.row(base[:50])])      # deletions only
    jobs.append([pool.row(base), pool.row(base.translate(bytes.maketrans(b"ACGT", b"CGTA"))), pool.row(base)])      # reach 0 between kept ones
    jobs.append([pool.row(base), pool.row(X.mutate(rng, base, inss=[(0, 3), (20, 1)], dels=[(40, 2)])[:64])])
    return p, pool.genomes(), jobs


@functools.lru_cache(maxsize=None)
def ties_case():
    """scores (1, 1, 1) over two letters: diagonal, up and left explain many cells at once"""
    pool = X.Pool(2, seed=3)
    p = X.params(max_flank=32, band=5, match=1, mismatch=1, gap=1, ani=50, min_len=1)
    words = [b"AAAAAAAAAAAAAAAA", b"AAAAAAAAAAAA", b"ACACACACACACACAC", b"CACACACACACACA", b"AACCAACCAACCAACCAACC", b"ACCAACCAACCAACCA", b"AAAACAAAACAAAA", b"AAACAAACAAACAAAAC"]
    jobs = [[pool.row(a), pool.row(b)] for a in words for b in words if a != b]
    jobs.append([pool.row(w) for w in words])
    return p, pool.genomes(), jobs


@functools.lru_cache(maxsize=None)
def wide_case():
    """F = 16: a job of C = 2 F columns and one of C = 2 F + 1, found by the restatement among seeded candidates"""
    p = X.params(max_flank=16, band=10, ani=50, min_len=1)
    found = {}
    for seed in range(400):
        rng = np.random.default_rng(seed)
        base = X.rand_seq(rng, 16)
        rows = [base]
        for r in range(4 + seed % 4):      # rows that each insert 2 ... 5 bases somewhere
            at, k = int(rng.integers(0, 13)), int(rng.integers(2, 6))
            rows.append(X.mutate(rng, base, inss=[(at, k)])[:16])
        C = X.job(rows, p)["width"]
        if C in (32, 33) and C not in found:
            found[C] = rows
        if len(found) == 2:
            break
    assert set(found) == {32, 33}
    pool = X.Pool(2, seed=9)
    return p, [[pool.row(r) for r in found[32]], [pool.row(r) for r in found[33]], [pool.row(r) for r in found[32][:3]]], pool


def check_paths(lib):
    p, genomes, jobs = paths_case()
    with Session(lib, genomes) as s:
        want = run_jobs(s, genomes, jobs, p)
    for j, slot in ((0, 0), (1, 25), (2, 57)):
        ins = want[j]["ins"]
        assert ins[1][slot] == 2 and ins[2][slot] == 5 and ins[3][slot] == 0 and want[j]["cols"] == want[j]["reach"] + 5, (j, ins)
    assert not want[3]["ins"][1].any() and want[3]["cols"] == want[3]["reach"] == 60 and b"-" in want[3]["rows"][1]
    assert want[4]["reach"] == 0 and want[5]["reach"] > 0
    assert all(i[-1] == 0 for w in want if w["ins"] for i in w["ins"])      # (no row inserts in slot A: see the module's docstring)
    p, genomes, jobs = ties_case()
    with Session(lib, genomes) as s:
        want = run_jobs(s, genomes, jobs, p, best=True)
    assert sum(w["cols"] > w["reach"] > 0 for w in want) > 5
    p, jobs, pool = wide_case()
    with Session(lib, pool.genomes()) as s:
        want = run_jobs(s, pool.genomes(), jobs, p)
        assert [w["cols"] for w in want][:2] == [32, -1] and want[2]["cols"] > 0
        run_jobs(s, pool.genomes(), jobs, p, max_cols=40, out_off=[1000, 0, 400])      # the caller's own pitch and places


def test_paths(lib):
    check_paths(lib)


# ------------------------------------------------------------------------------------------------------- orientation
def check_orientation(lib):
    """flanks that begin at position 0 and at the genome's last base, with either step and complement"""
    rng = np.random.default_rng(11)
    base = X.rand_seq(rng, 40)
    var = X.mutate(rng, base, subs=1, inss=[(20, 2)])
    comp = lambda t: t.translate(X._COMP)      # noqa: E731
    g0 = base + b"NN" + comp(var)[::-1]                  # base from position 0 upwards; var complemented, read down from the last base
    g1 = var[::-1] + b"N" + comp(base)                   # var read down to position 0; base complemented, up to the last base
    genomes = [g0, g1]
    n0, n1 = len(g0), len(g1)
    r_base = [(0, 1, 0, 40, 0), (1, 1, 1, 40, n1 - 40)]
    r_var = [(0, -1, 1, 42, n0 - 1), (1, -1, 0, 42, 41)]
    assert all(X.read_row(genomes, r) == base for r in r_base) and all(X.read_row(genomes, r) == var for r in r_var)
    jobs = [[r_base[0], r_var[0]], [r_base[1], r_var[1], r_base[0]], [r_var[1], r_base[1]], [r_var[0], r_var[1], r_base[0], r_base[1]]]
    with Session(lib, genomes) as s:
        want = run_jobs(s, genomes, jobs, X.params(max_flank=64, band=8, ani=80))
    assert all(w["reach"] >= 38 for w in want)


def test_orientation(lib):
    check_orientation(lib)


# ------------------------------------------------------------------------------------------------------- arguments
def check_arguments(lib):
    assert lib.ext_limits() == (X.MAX_ROWS, X.MAX_FLANK, X.MAX_BAND)
    g = [X.rand_seq(np.random.default_rng(1), 600)] * 2
    ok = [(0, 1, 0, 30, 5), (1, 1, 0, 30, 5)]
    with Session(lib, g) as s:
        assert s.ext_reach([0], [], None).shape == (0,) and not [k for k, _ in s.last_timing() if k.startswith("ext_")]      # no job: valid, nothing launched
        same_ints(s.ext_reach([0, 2], ok), [30], "a plain job")
        for key, vals in (("max_flank", (15, 513)), ("band", (0, 64)), ("match", (0, 16)), ("mismatch", (-1, 16)), ("gap", (0, 16)), ("ani", (49, 101)), ("min_len", (0, 257))):
            for v in vals:
                with pytest.raises(PmError, match=r"code -2"):
                    s.ext_reach([0, 2], ok, X.params(**{key: v}))
                with pytest.raises(PmError, match=r"code -2"):
                    s.ext_align([0, 2], ok, [30], X.params(**{key: v}))
        s.ext_reach([0, 2], ok, X.params(max_flank=512, band=63, match=15, mismatch=15, gap=15, ani=100, min_len=512))
        bad_rows = [(2, 1, 0, 30, 5), (-1, 1, 0, 30, 5), (1, 2, 0, 30, 5), (1, 0, 0, 30, 5), (1, 1, 0, -1, 5), (1, 1, 0, 30, 571), (1, 1, 0, 30, -1), (1, 1, 0, 30, 600),
                    (1, -1, 0, 30, 28), (1, -1, 0, 30, 600), (1, 1, 2, 30, 5)]
        for r in bad_rows:      # a descriptor that leaves its genome, names none, or has no step
            with pytest.raises(PmError, match=r"code -2"):
                s.ext_reach([0, 2], [ok[0], r])
            with pytest.raises(PmError, match=r"code -2"):
                s.ext_align([0, 2], [ok[0], r], [0])
        s.ext_reach([0, 2], [ok[0], (1, 1, 0, 30, 570)])
        s.ext_reach([0, 2], [ok[0], (1, -1, 1, 30, 29)])
        for off, rows in (([0, 1], ok[:1]), ([0, 2, 3], ok + ok[:1]), ([0, 2, 2], ok), ([1, 3], ok + ok), ([0, 3, 2], ok + ok)):      # n < 2, offsets that do not ascend from 0
            with pytest.raises(PmError, match=r"code -2"):
                s.ext_reach(off, rows)
        with pytest.raises(PmError, match=r"code -5"):      # len > max_flank
            s.ext_reach([0, 2], [ok[0], (1, 1, 0, 257, 5)])
        s.ext_reach([0, 2], [ok[0], (1, 1, 0, 256, 5)])
        with pytest.raises(PmError, match=r"code -5"):      # 2 049 rows
            s.ext_reach([0, 2049], [ok[0]] * 2049)
        for reach in ([31], [-1]):      # a reach outside the reference flank
            with pytest.raises(PmError, match=r"code -2"):
                s.ext_align([0, 2], ok, reach)
        with pytest.raises(PmError, match=r"code -2"):
            s.ext_align([0, 2], ok, [30], max_cols=511)
        # a caller's own reach: any line on which every row of the job has a cell (len + band), none beyond
        short = [ok[0], (1, 1, 0, 2, 5)]
        p5 = X.params(band=5)
        for reach in (8, 30):
            with pytest.raises(PmError, match=r"code -2"):
                s.ext_align([0, 2], short, [reach], p5)
        cols, used, blocks = s.ext_align([0, 2], short, [7], p5)
        flanks = [X.read_row(g, r) for r in short]
        paths = [X.path(X.table(flanks[0], b, p5), flanks[0], b, 7, p5) for b in flanks]
        assert list(used) == [pt[0] for pt in paths] == [7, 2] and [r.tobytes() for r in blocks[0]] == X.columns(paths, flanks, 7) and cols[0] == 7
        # every byte of a job's block that holds no letter is 0: past column C, and the rows of a dropped job
        mine = np.full(4 * 512, 255, np.uint8)
        cols, used, blocks = s.ext_align([0, 2, 4], ok + ok, [30, 0], out=mine)
        raw = mine.reshape(4, 512)
        assert list(cols) == [30, 0] and not raw[:2, 30:].any() and not raw[2:].any() and raw[:2, :30].all()
        cols, used, blocks = s.ext_align([0, 2], ok, [30])
        assert cols[0] == 30 and list(used) == [30, 30] and blocks[0][0].tobytes() == blocks[0][1].tobytes() == g[0][5:35]


def test_arguments(lib):
    check_arguments(lib)


# ---------------------------------------------------------------------------------------------------------------- end to end
TIMING_KEYS = {"ext_jobs", "ext_kept", "ext_wide", "ext_bases", "ext_ms"}
EXT_FILE = "parsnpAligner.xmfa.extended"
E2E = dict(extani=80, extmin=12)


@functools.lru_cache(maxsize=None)
def file_seqs():
    return X.file_design()


def file_inputs(base):
    from parsnp_amd import synth
    seqs = file_seqs()
    return synth.write_set(os.path.join(base, "in"), seqs[0], seqs[1:])


def run(core_bin, rpath, qs, base, tag, threads, **kw):
    from parsnp_amd import driver
    out = os.path.join(base, "out_" + tag)
    timing = os.path.join(base, "t_%s.json" % tag)
    rc, _ = driver.run_core(core_bin, rpath, qs, out, threads=threads, timing=timing, unaligned=1, **kw)
    assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
    return out, driver.read_timing(timing)


def genomes_of(out):
    """the genomes in the XMFA's order, as the run held them (single contigs: the FASTA's letters, upper case)"""
    head, _ = X.read_xmfa(os.path.join(out, "parsnpAligner.xmfa"))
    names = [h.split(" ", 1)[1] for h in head if h.startswith("##SequenceFile ")]
    return names


def check_extended_of(out, seqs_by_name, **kw):
    from parsnp_amd import driver
    p = X.params(**{{"extmax": "max_flank", "extband": "band", "extmatch": "match", "extmismatch": "mismatch", "extgap": "gap", "extani": "ani", "extmin": "min_len"}[k]: v
                    for k, v in kw.items()})
    genomes = [seqs_by_name[name] for name in genomes_of(out)]
    text, counts = X.extended_text(os.path.join(out, "parsnpAligner.xmfa"), genomes, p)
    got = open(os.path.join(out, EXT_FILE), "rb").read()
    assert got == text.encode(), "first difference at byte %d" % next((i for i, (x, y) in enumerate(zip(got, text.encode())) if x != y), min(len(got), len(text)))
    head, jobs = driver.read_extended(out)
    xhead, lcbs = X.read_xmfa(os.path.join(out, "parsnpAligner.xmfa"))
    assert head == xhead and len(jobs) == counts["ext_kept"]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    taken = [[] for _ in genomes]
    for recs in lcbs:
        for seq, lo, hi, _, _ in recs:
            taken[seq - 1].append((lo, hi))
    for cluster, side, recs in jobs:
        assert len({len(r[4]) for r in recs}) == 1 and len(recs) == len(genomes)
        for seq, lo, hi, strand, letters in recs:
            bases = letters.replace("-", "").encode()
            assert letters == letters.upper() and set(letters) <= set("ACGT-")
            if not bases:
                assert (lo, hi) == (0, 0)
                continue
            want = genomes[seq - 1][lo - 1:hi]
            assert bases == (want.translate(comp)[::-1] if strand == "-" else want), (cluster, side, seq)
            taken[seq - 1].append((lo, hi))
    for iv in taken:      # no two records of a genome overlap each other or the XMFA's records
        iv.sort()
        assert all(a[1] < b[0] for a, b in zip(iv, iv[1:]))
    return counts, jobs, lcbs


def check_e2e(core_bin, base, threads=4):
    import xmfa_util
    rpath, qs = file_inputs(base)
    seqs = file_seqs()
    by_name = {os.path.basename(p): s for p, s in zip([rpath] + list(qs), seqs)}
    (o1, t1), (o2, t2) = run(core_bin, rpath, qs, base, "plain", threads), run(core_bin, rpath, qs, base, "ext", threads, lcbext=1, **E2E)
    for f in sorted(os.listdir(o1)):
        if f not in ("parsnp-aligner.err", "parsnp-aligner.out", "parsnpAligner.log", "parsnpAligner.ini"):
            assert xmfa_util.md5(os.path.join(o1, f)) == xmfa_util.md5(os.path.join(o2, f)), f
    strip = lambda p: [l for l in open(p) if "elapsed time" not in l and "running time" not in l]      # noqa: E731
    assert strip(os.path.join(o1, "parsnpAligner.log")) == strip(os.path.join(o2, "parsnpAligner.log"))
    assert sorted(set(os.listdir(o2)) - set(os.listdir(o1))) == [EXT_FILE]
    assert set(t2) - set(t1) == TIMING_KEYS and set(t1) <= set(t2) and not [k for k in t1 if k.startswith("ext_")]
    counts, jobs, lcbs = check_extended_of(o2, by_name, **E2E)
    assert all(t2[k] == counts[k] for k in counts) and t2["ext_ms"] >= 0
    assert counts["ext_jobs"] == 2 * len(lcbs) and 0 < counts["ext_kept"] < counts["ext_jobs"]
    err = open(os.path.join(o2, "parsnp-aligner.err")).read()
    assert "LCB extension: %d jobs, %d kept, %d reference bases added" % (counts["ext_jobs"], counts["ext_kept"], counts["ext_bases"]) in err
    assert "LCB extension" not in open(os.path.join(o1, "parsnp-aligner.err")).read()
    # what the design is for: reverse rows, a side L that reaches position 1, a flank cut short by the N run, a halved run
    strands = {r[3] for _, _, recs in jobs for r in recs}
    assert strands == {"+", "-"}
    assert any(side == "L" and recs[0][1] == 1 for _, side, recs in jobs)
    assert any(side == "R" and recs[0][2] > 12100 and r[0] != 1 and r[2] == 12100 for _, side, recs in jobs for r in recs), "the N run ends one row's flank, not the job"
    ref_iv = sorted((lo, hi) for recs in lcbs for seq, lo, hi, _, _ in recs if seq == 1)
    gaps = [(a[1] + 1, b[0] - 1) for a, b in zip(ref_iv, ref_iv[1:]) if 0 < b[0] - a[1] - 1 < 512]
    assert gaps, ref_iv
    lo, hi = gaps[0]
    halves = sorted((r[1], r[2]) for _, _, recs in jobs for r in recs[:1] if lo <= r[1] and r[2] <= hi)
    assert len(halves) == 2 and halves[0] == (lo, lo + (hi - lo + 2) // 2 - 1) and halves[1][1] == hi, (gaps, halves)
    # other settings: the restatement's text again
    o3, _ = run(core_bin, rpath, qs, base, "narrow", threads, lcbext=1, extmax=64, extband=5, extani=75, extmin=1, extmatch=1, extmismatch=1, extgap=1)
    check_extended_of(o3, by_name, extmax=64, extband=5, extani=75, extmin=1, extmatch=1, extmismatch=1, extgap=1)
    return counts


def test_files(emu, tmp_path):
    check_e2e(emu[1], str(tmp_path))


def check_limits(core_bin, base):
    """2 049 sequences or a key outside its range: exit 5 before any sequence is read"""
    from parsnp_amd import driver
    qs = ["/nonexistent/g%d.fna" % i for i in range(2048)]
    cases = [("many", qs, {})] + [("%s%d" % (k, v), qs[:3], {k: v}) for k, vals in (("extmax", (15, 513)), ("extband", (0, 64)), ("extmatch", (0, 16)), ("extmismatch", (-1, 16)),
                                                                                  ("extgap", (0, 16)), ("extani", (49, 101)), ("extmin", (0, 257))) for v in vals]
    for tag, q, kw in cases:
        rc, _ = driver.run_core(core_bin, "/nonexistent/ref.fna", q, os.path.join(base, tag), lcbext=1, **kw)
        assert rc == 5 and "limit of the multi-MUM engine" in open(os.path.join(base, tag, "parsnp-aligner.err")).read(), tag
    rc, _ = driver.run_core(core_bin, "/nonexistent/ref.fna", qs[:3], os.path.join(base, "ok"), lcbext=1, extmax=512, extband=63, extmatch=15, extmismatch=15, extgap=15,
                            extani=100, extmin=512)
    assert rc == 1      # (within the limits: the run goes on and fails to read the sequences)
    rc, _ = driver.run_core(core_bin, "/nonexistent/ref.fna", qs, os.path.join(base, "off"))
    assert rc == 1      # (without the key 2 049 sequences are no limit of this feature)


def test_limits(emu, tmp_path):
    check_limits(emu[1], str(tmp_path))


def test_ini_text():
    from parsnp_amd import driver
    import test_snp_columns as S
    args = ("/x/ref.fna", ["/x/a.fna", "/x/b.fna"], "/x/out")
    assert driver.ini_text(*args, threads=3) == S.INI_TODAY
    assert driver.ini_text(*args, threads=3, lcbext=1) == S.INI_TODAY + "lcbext=1\n"
    assert driver.ini_text(*args, threads=3, recomb=1, lcbext=1, extmax=128, extband=9, extmatch=4, extmismatch=3, extgap=1, extani=90, extmin=7) == \
        S.INI_TODAY + "recomb=1\nlcbext=1\nextmax=128\nextband=9\nextmatch=4\nextmismatch=3\nextgap=1\nextani=90\nextmin=7\n"
