"""The recombination scan of the core SNP columns (pm_rec_sites, pm_rec_incompat, pm_rec_test; rec_kernels.h) against the numpy
restatement of tests/recphi.py, in the kernel emulation; tests/test_gpu_rec_phi.py runs the same checks on the device.  Flags,
scores, phi and le are compared as integers, the two files as bytes.  No tolerances.  Then the writer: with recomb=1 the files
.rec.tsv and .rec are the restatement's text for the .snps.mfa / .snps.tsv of the same run, and every other file has the bytes of a
run without the key."""
import functools
import os

import numpy as np
import pytest

import recphi as rp
import test_snp_columns as S
from bootsupport import chunks_of
from parsnp_amd.binding import Lib, PmError

ROWS = (2, 3, 4, 5, 63, 64, 65, 129)
COLS = (0, 1, 63, 64, 65, 129)
SHAPES = [(2, 65), (3, 129), (4, 64), (5, 63), (63, 1), (64, 129), (65, 65), (129, 64), (5, 0)]
assert {s[0] for s in SHAPES} == set(ROWS) and {s[1] for s in SHAPES} == set(COLS)
SEEDS = (1, 0xFEDCBA9876543210)


@pytest.fixture(scope="module")
def lib(emu):
    return Lib(emu[0])


@functools.lru_cache(maxsize=None)
def letters_of(n, v):
    return rp.random_letters(n, v, 1000 * n + v)


def collection(s, letters, chunks=None):
    got = s.core_snps(chunks if chunks is not None else chunks_of(letters))
    assert got[0]["core_snps"] == letters.shape[1] and np.array_equal(got[2], letters)


def same_ints(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = tuple(int(x) for x in np.argwhere(got != want)[0])
        raise AssertionError("%s: entry %r is %d, restatement %d (%d differ)" % (what, at, got[at], want[at], int((got != want).sum())))


def windows_over(v, sizes, rng):
    """windows of the given sizes over columns 0 ... v - 1, in any order, overlapping: (sites, win_off)"""
    sites = np.concatenate([rng.permutation(v)[:k] for k in sizes]).astype(np.int64)
    return sites, np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)


# ------------------------------------------------------------------------------------------------------- flags and scores
def check_sites(lib, n, v):
    """informative flags and the scores of all pairs (one window, two where V allows), at the row-word and plane-word edges"""
    letters = letters_of(n, v)
    with S.two_genomes(lib) as s:
        collection(s, letters)
        flags = s.rec_sites()
        same_ints(flags, rp.informative(letters), "informative flags")
        if n < 4:
            assert not flags.any()
        if v >= 2:
            rng = np.random.default_rng(v)
            sites, off = windows_over(v, [v, 2, min(v, 17)], rng)
            mats = s.rec_incompat(sites, off)
            for w, m in enumerate(mats):
                same_ints(m, rp.matrix(letters, sites[off[w]:off[w + 1]]), "scores of window %d" % w)
                assert np.array_equal(m, m.T) and not m.diagonal().any() and m.max(initial=0) <= 9
        return flags


@pytest.mark.parametrize("n,v", SHAPES)
def test_sites(lib, n, v):
    check_sites(lib, n, v)


@functools.lru_cache(maxsize=None)
def rows2048():
    letters = rp.random_letters(2048, 65, 2048)
    letters[:, 7] = ord("A")
    letters[2047, 7] = ord("C")            # a single row past 31 full row words: not informative
    letters[2046:, 9] = ord("G")
    letters[:2046, 9] = ord("T")           # two rows of one letter at the end: informative
    return letters, rp.informative(letters), rp.matrix(letters, np.arange(65))


def check_rows2048(lib):
    letters, flags, mat = rows2048()
    assert flags[7] == 0 and flags[9] == 1
    with S.two_genomes(lib) as s:
        collection(s, letters)
        same_ints(s.rec_sites(), flags, "informative flags")
        same_ints(s.rec_incompat(np.arange(65), [0, 65])[0], mat, "scores")


def test_rows2048(lib):
    check_rows2048(lib)


def check_adds(lib):
    """a collection built by several adds whose widths are no multiple of 64"""
    letters = letters_of(65, 129)
    chunks = [np.ascontiguousarray(letters[:, a:b]) for a, b in ((0, 7), (7, 70), (70, 71), (71, 129))]
    with S.two_genomes(lib) as s:
        collection(s, letters, chunks)
        same_ints(s.rec_sites(), rp.informative(letters), "informative flags")
        same_ints(s.rec_incompat(np.arange(129), [0, 129])[0], rp.matrix(letters, np.arange(129)), "scores")
        # a new collection forgets the transposed planes of the last one
        collection(s, letters_of(5, 63))
        same_ints(s.rec_sites(), rp.informative(letters_of(5, 63)), "flags of a new collection")


def test_adds(lib):
    check_adds(lib)


@functools.lru_cache(maxsize=None)
def pair_case():
    names, letters = rp.pair_design()
    mat = rp.matrix(letters, np.arange(len(names)))
    return names, letters, mat


def test_pair_design_reaches_its_classes():
    names, letters, mat = pair_case()
    at = {k: i for i, k in enumerate(names)}
    sc = lambda a, b: int(mat[at[a], at[b]])      # noqa: E731
    assert sc("two", "two_b") == 1                 # one cycle of four
    assert sc("two", "four") == 0 and sc("two", "three") == 0      # forests
    assert sc("four", "four_b") == 9               # the complete graph
    assert sc("four", "four_c") == 1               # one cycle of eight
    assert sc("two", "same") == 0                  # two components: E 2, V 4, C 2
    assert sc("three", "four_b") == 6 and sc("three", "three_b") == 4
    assert {len(set(letters[:, at[k]])) for k in names} == {2, 3, 4}
    assert set(int(x) for x in np.unique(mat)) >= {0, 1, 4, 6, 9}
    # every score the definition can give between two columns of 16 rows that this design's patterns make
    for a in names:
        for b in names:
            if a != b:
                x, y = letters[:, at[a]], letters[:, at[b]]
                e = len(set(zip(x, y)))
                assert sc(a, b) == rp.inc(x, y) and 0 <= sc(a, b) <= 9 and sc(a, b) <= e - 1


def check_pairs(lib):
    names, letters, mat = pair_case()
    with S.two_genomes(lib) as s:
        collection(s, letters)
        same_ints(s.rec_incompat(np.arange(len(names)), [0, len(names)])[0], mat, "pair design")
        rev = np.arange(len(names))[::-1].copy()
        same_ints(s.rec_incompat(rev, [0, len(names)])[0], mat[np.ix_(rev, rev)], "pair design, sites in reverse")
    for n, row in ((65, 64), (129, 128), (5, 4)):      # the only conflicting row is row 64 / row n - 1
        x, y = rp.conflict_in_one_row(n, row)
        assert rp.inc(x, y) == 1 and rp.inc(np.delete(x, row), np.delete(y, row)) == 0
        pair = np.stack([x, y], axis=1)
        with S.two_genomes(lib) as s:
            collection(s, pair)
            same_ints(s.rec_incompat([0, 1], [0, 2])[0], [[0, 1], [1, 0]], "conflict in row %d of %d" % (row, n))


def test_pairs(lib):
    check_pairs(lib)


# ------------------------------------------------------------------------------------------------------- the permutation test
K_SIZES = (2, 16, 17, 63, 64, 65, 255, 256)
PERMS = (1, 99, 100, 101, 1000)
PERMS_OF = {2: (1, 99), 16: (100,), 17: (101,), 63: (100,), 64: (99, 1000), 65: (101,), 255: (99,), 256: (100,)}      # (P <= 200 where k is 255 or 256)
assert set(PERMS_OF) == set(K_SIZES) and {p for v in PERMS_OF.values() for p in v} == set(PERMS)


@functools.lru_cache(maxsize=None)
def random_matrix(k, seed):
    rng = np.random.default_rng(seed)
    m = np.triu(rng.integers(0, 10, (k, k)) * (rng.random((k, k)) < 0.3), 1).astype(np.uint8)
    return m + m.T


def check_windows(lib, k):
    """one call per (H, P, seed): windows of size k beside one of 16 sites, the caller's matrices, win_id omitted and given"""
    perms_of = PERMS_OF[k]
    with S.two_genomes(lib) as s:
        for near in (1, 10, k - 1, k + 5):
            for perms in perms_of:
                seed = SEEDS[(near + perms) % 2]
                mats = [random_matrix(k, k), random_matrix(16, 16), random_matrix(k, k)]
                off = np.cumsum([0, k, 16, k])
                phi, le = s.rec_test(off, near, perms, seed, inc=mats)
                want = [rp.test_window(m, g, near, perms, seed) for g, m in enumerate(mats)]
                same_ints(phi, [w[0] for w in want], "phi, k %d H %d P %d" % (k, near, perms))
                same_ints(le, [w[1] for w in want], "le, k %d H %d P %d" % (k, near, perms))
                assert phi[0] == phi[2]      # (the same matrix under another g: the same phi, other permutations)
                ids = np.array([5, 0, 2 ** 40], np.int64)
                phi2, le2 = s.rec_test(off, near, perms, seed, inc=mats, win_id=ids)
                want = [rp.test_window(m, int(g), near, perms, seed) for g, m in zip(ids, mats)]
                same_ints(phi2, [w[0] for w in want], "phi with win_id")
                same_ints(le2, [w[1] for w in want], "le with win_id")


@pytest.mark.parametrize("k", K_SIZES)
def test_windows(lib, k):
    check_windows(lib, k)


def test_window_rules():
    assert rp.flagged(0, 100) and not rp.flagged(0, 99) and not rp.flagged(1, 100) and rp.flagged(9, 1000) and not rp.flagged(10, 1000)
    assert [rp.windows_of(m) for m in (15, 16, 99)] == [[], [(0, 16)], [(0, 99)]]
    assert rp.windows_of(100) == [(0, 100)] and rp.windows_of(150) == [(0, 100), (50, 100)] and rp.windows_of(151) == [(0, 100), (50, 100), (51, 100)]
    assert rp.windows_of(40, 16) == [(0, 16), (8, 16), (16, 16), (24, 16)] and rp.windows_of(33, 17) == [(0, 17), (8, 17), (16, 17)]


@functools.lru_cache(maxsize=None)
def batch_case():
    """7 windows that overlap, over the columns of one collection"""
    letters = letters_of(64, 129)
    rng = np.random.default_rng(7)
    sizes = [40, 16, 129, 2, 65, 17, 64]
    sites, off = windows_over(129, sizes, rng)
    mats = [rp.matrix(letters, sites[off[w]:off[w + 1]]) for w in range(7)]
    want = [rp.test_window(m, g, 10, 150, 1) for g, m in enumerate(mats)]
    return letters, sites, off, mats, want


def check_batches(lib):
    """rec_batch 1 and 3 with 7 windows give what the default gives: sites -> incompat -> test, the matrices from the device"""
    letters, sites, off, mats, want = batch_case()
    assert len(set(sites[off[0]:off[1]]) & set(sites[off[2]:off[3]])) > 0      # windows that overlap
    names = []
    for k in (0, 1, 3):
        with S.two_genomes(lib) as s:
            s.tune("rec_batch", k)
            collection(s, letters)
            got = s.rec_incompat(sites, off)
            names += [x for x, _ in s.last_timing()]      # (the phases of a call: the device's tests look at them)
            for w in range(7):
                same_ints(got[w], mats[w], "scores of window %d, batch %d" % (w, k))
            phi, le = s.rec_test(off, 10, 150, 1)
            same_ints(phi, [x[0] for x in want], "phi, batch %d" % k)
            same_ints(le, [x[1] for x in want], "le, batch %d" % k)
            names += [x for x, _ in s.last_timing()]
    return names


def test_batches(lib):
    check_batches(lib)


@pytest.mark.parametrize("launch", ["rec_transpose", "rec_incompat", "rec_permute"])
def test_wavefronts_of_a_launch_do_not_depend_on_one_another(lib, launch, monkeypatch):
    monkeypatch.setenv("PM_EMU_REVERSE_WAVES", launch)
    check_batches(lib)


# ------------------------------------------------------------------------------------------------------- designed outcomes
@functools.lru_cache(maxsize=None)
def designed():
    tree = rp.tree_letters(12, 40, 5)
    mosaic = rp.mosaic_letters(12, 20, 20, 3)
    out = {}
    for name, letters in (("tree", tree), ("mosaic", mosaic)):
        mat = rp.matrix(letters, np.arange(40))
        out[name] = (letters, mat, rp.test_window(mat, 0, 5, 1000, 1))
    return out


def test_designs():
    """the restatement's verdicts first: a design that flags nothing cannot pass silently"""
    d = designed()
    letters, mat, (phi, le) = d["tree"]
    assert rp.informative(letters).all() and not mat.any() and phi == 0 and le == 1000 and not rp.flagged(le, 1000)
    letters, mat, (phi, le) = d["mosaic"]
    assert rp.informative(letters).all() and not mat[:20, :20].any() and not mat[20:, 20:].any() and mat[:20, 20:].all()
    across = [(i, j) for i in range(20) for j in range(20, 40) if j - i <= 5]      # the pairs across the break point at identity order
    assert len(across) == 15 and phi == sum(int(mat[i, j]) for i, j in across) == 15
    assert le <= 2 and rp.flagged(le, 1000)


def check_designed(lib):
    for name, (letters, mat, (phi, le)) in designed().items():
        with S.two_genomes(lib) as s:
            collection(s, letters)
            assert s.rec_sites().all()
            same_ints(s.rec_incompat(np.arange(40), [0, 40])[0], mat, name)
            gphi, gle = s.rec_test([0, 40], 5, 1000, 1)
            assert (int(gphi[0]), int(gle[0])) == (phi, le), name
            assert rp.flagged(int(gle[0]), 1000) == (name == "mosaic")


def test_designed(lib):
    check_designed(lib)


# ------------------------------------------------------------------------------------------------------- arguments
def check_arguments(lib):
    assert lib.rec_limits() == (rp.MAX_ROWS, rp.MAX_SITES, rp.MAX_PERMS)
    letters = letters_of(5, 63)
    big = [np.zeros((257, 257), np.uint8)]
    with S.two_genomes(lib) as s:
        for call in (s.rec_sites, lambda: s.rec_incompat([0, 1], [0, 2]), lambda: s.rec_test([0, 2])):      # no collection, no matrices
            with pytest.raises(PmError, match=r"code -2"):
                call()
        collection(s, letters)
        with pytest.raises(PmError, match=r"code -2"):      # no matrices on the device yet
            s.rec_test([0, 2])
        assert s.rec_incompat([], [0]) == [] and s.rec_incompat([1, 2], [0]) == []      # no window: valid, nothing launched
        phi, le = s.rec_test([0])
        assert phi.shape == (0,) and le.shape == (0,) and not [k for k, _ in s.last_timing() if k.startswith("rec_")]
        for sites, off in (([0, 63], [0, 2]), ([-1, 3], [0, 2]), ([0, 1, 2], [0, 2, 1]), ([0, 1, 2], [0, 1, 3]), ([0, 1, 2], [0, 2, 2]), ([0, 1, 2], [0, 4]),
                           ([0, 1, 2], [-1, 2])):
            with pytest.raises(PmError, match=r"code -2"):
                s.rec_incompat(sites, off)
        with pytest.raises(PmError, match=r"code -5"):
            s.rec_incompat(np.arange(257) % 63, [0, 257])
        assert len(s.rec_incompat(np.arange(256) % 63, [0, 256])) == 1
        with pytest.raises(PmError, match=r"code -2"):      # other sizes than the matrices on the device
            s.rec_test([0, 255])
        s.rec_test([0, 256], perms=3)
        s.rec_test([7, 263], perms=3)      # (only the sizes count)
        mats = [random_matrix(16, 16)]
        for kw in (dict(near=0), dict(perms=0), dict(near=-3), dict(perms=-1)):
            with pytest.raises(PmError, match=r"code -2"):
                s.rec_test([0, 16], inc=mats, **kw)
        with pytest.raises(PmError, match=r"code -2"):
            s.rec_test([0, 1], inc=[np.zeros((1, 1), np.uint8)])
        with pytest.raises(PmError, match=r"code -5"):
            s.rec_test([0, 16], inc=mats, perms=rp.MAX_PERMS + 1)
        with pytest.raises(PmError, match=r"code -5"):
            s.rec_test([0, 257], inc=big)
        same_ints(s.rec_test([0, 16], inc=mats, perms=7)[0], [rp.test_window(mats[0], 0, 10, 7, 1)[0]], "after refused calls")


def test_arguments(lib):
    check_arguments(lib)


# ---------------------------------------------------------------------------------------------------------------- end to end
TIMING_KEYS = {"rec_sites", "rec_windows", "rec_flagged", "rec_ms"}
REC_FILES = ["parsnpAligner.rec", "parsnpAligner.rec.tsv"]
E2E = dict(recsites=40, recperms=300, recnear=5, recseed=3)


@functools.lru_cache(maxsize=None)
def planted_letters(n=12):
    """100 columns that fit one tree, 20 that fit a conflicting one (the planted segment), 100 of the first kind again"""
    a, b = rp.mosaic_letters(n, 100, 20, 11), rp.mosaic_letters(n, 100, 0, 12)
    return np.concatenate((a, b), axis=1)


def planted_inputs(base, n=12, spacing=250):
    """FASTA files of n sequences: a constant random backbone with column c of the letters matrix at base 200 + spacing * c"""
    from parsnp_amd import synth
    letters = planted_letters(12)[:n]
    rng = np.random.default_rng(99)
    back = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 400 + spacing * letters.shape[1])]
    seqs = []
    for i in range(n):
        g = back.copy()
        g[200 + spacing * np.arange(letters.shape[1])] = letters[i]
        seqs.append(g.tobytes())
    return synth.write_set(os.path.join(base, "in%d" % n), seqs[0], seqs[1:])


def run(core_bin, rpath, qs, base, tag, threads, env=None, **kw):
    from parsnp_amd import driver
    out = os.path.join(base, "out_" + tag)
    timing = os.path.join(base, "t_%s.json" % tag)
    rc, _ = driver.run_core(core_bin, rpath, qs, out, threads=threads, timing=timing, unaligned=1, env=env, **kw)
    assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
    return out, driver.read_timing(timing)


def check_rec_of(out, **kw):
    """the two files of a run are the restatement's text for that run's .snps.mfa and .snps.tsv"""
    from parsnp_amd import driver
    _, letters, rows, _ = driver.read_snps(out)
    recs, n_inf = rp.scan(letters, rows, perms=kw.get("recperms", 1000), seed=kw.get("recseed", 1), K=kw.get("recsites", 100), near=kw.get("recnear", 10))
    tsv, bed = rp.files_text(recs)
    assert open(os.path.join(out, REC_FILES[1]), "rb").read() == tsv.encode()
    assert open(os.path.join(out, REC_FILES[0]), "rb").read() == bed.encode()
    got_rows, got_bed = driver.read_rec(out)
    assert len(got_rows) == len(recs) and len(got_bed) == sum(r["flagged"] for r in recs)
    return recs, n_inf


def check_e2e(core_bin, base, threads=4):
    import xmfa_util
    rpath, qs = planted_inputs(base)
    (o1, t1), (o2, t2) = run(core_bin, rpath, qs, base, "snps", threads, snps=1), run(core_bin, rpath, qs, base, "rec", threads, recomb=1, **E2E)
    for f in ("parsnpAligner.xmfa", "parsnp.unalign") + S.FILES:
        assert xmfa_util.md5(os.path.join(o1, f)) == xmfa_util.md5(os.path.join(o2, f)), f
    strip = lambda p: [l for l in open(p) if "elapsed time" not in l and "running time" not in l]      # noqa: E731
    assert strip(os.path.join(o1, "parsnpAligner.log")) == strip(os.path.join(o2, "parsnpAligner.log"))
    assert sorted(set(os.listdir(o2)) - set(os.listdir(o1))) == REC_FILES
    assert set(t2) - set(t1) == TIMING_KEYS and set(t1) <= set(t2) and not [k for k in t1 if k.startswith("rec_")]
    recs, n_inf = check_rec_of(o2, **E2E)
    flags = [r["flagged"] for r in recs]
    assert any(flags) and not all(flags), flags      # (the restatement's verdicts: the planted segment is found, the rest is not)
    assert all(r["sites"] == 40 for r in recs) and len(recs) >= 8
    assert (t2["rec_sites"], t2["rec_windows"], t2["rec_flagged"]) == (n_inf, len(recs), sum(flags)) and t2["rec_ms"] >= 0
    err = open(os.path.join(o2, "parsnp-aligner.err")).read()
    assert "Recombination scan: %d windows of %d informative sites, %d flagged" % (len(recs), n_inf, sum(flags)) in err
    assert "Recombination" not in open(os.path.join(o1, "parsnp-aligner.err")).read()
    # a staging matrix of 7 columns (the collection is built by many adds): the same files; tree and bootstrap beside it: the same
    o3, _ = run(core_bin, rpath, qs, base, "stage7", threads, env=dict(os.environ, PARSNP_SNP_STAGE_COLUMNS="7"), recomb=1, **E2E)
    o4, _ = run(core_bin, rpath, qs, base, "boot", threads, recomb=1, bootstrap=3, **E2E)
    for f in REC_FILES + list(S.FILES):
        assert xmfa_util.md5(os.path.join(o2, f)) == xmfa_util.md5(os.path.join(o3, f)) == xmfa_util.md5(os.path.join(o4, f)), f
    return recs


def test_files(emu, tmp_path):
    check_e2e(emu[1], str(tmp_path))


def check_few_and_limits(core_bin, base, threads=4):
    """three sequences: the header alone and an empty .rec; 2 049 sequences or a key outside its range: exit 5 before any sequence is
    read"""
    from parsnp_amd import driver
    rpath, qs = planted_inputs(base, 3)
    out, t = run(core_bin, rpath, qs, base, "three", threads, recomb=1)
    assert open(os.path.join(out, REC_FILES[1])).read() == rp.HEADER and open(os.path.join(out, REC_FILES[0])).read() == ""
    assert check_rec_of(out) == ([], 0) and (t["rec_sites"], t["rec_windows"], t["rec_flagged"]) == (0, 0, 0)
    qs = ["/nonexistent/g%d.fna" % i for i in range(2048)]
    for tag, q, kw in (("many", qs, {}), ("sites", qs[:3], dict(recsites=300)), ("sites15", qs[:3], dict(recsites=15)), ("perms", qs[:3], dict(recperms=65537)),
                       ("perms0", qs[:3], dict(recperms=0)), ("near", qs[:3], dict(recnear=0))):
        rc, _ = driver.run_core(core_bin, "/nonexistent/ref.fna", q, os.path.join(base, tag), recomb=1, **kw)
        assert rc == 5 and "limit of the multi-MUM engine" in open(os.path.join(base, tag, "parsnp-aligner.err")).read(), tag
    rc, _ = driver.run_core(core_bin, "/nonexistent/ref.fna", qs[:3], os.path.join(base, "ok"), recomb=1, recsites=256, recperms=65536)
    assert rc == 1      # (within the limits: the run goes on and fails to read the sequences)


def test_few_and_limits(emu, tmp_path):
    check_few_and_limits(emu[1], str(tmp_path))


def test_ini_text():
    from parsnp_amd import driver
    args = ("/x/ref.fna", ["/x/a.fna", "/x/b.fna"], "/x/out")
    assert driver.ini_text(*args, threads=3) == S.INI_TODAY
    assert driver.ini_text(*args, threads=3, recomb=1) == S.INI_TODAY + "recomb=1\n"
    assert driver.ini_text(*args, threads=3, tree=1, recomb=1, recperms=99, recseed=7, recsites=64, recnear=3) == S.INI_TODAY + "tree=1\nrecomb=1\nrecperms=99\nrecseed=7\nrecsites=64\nrecnear=3\n"
