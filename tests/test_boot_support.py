"""Bootstrap support of the SNP tree (pm_boot_distances, pm_nj_trees, pm_nj_support; boot_kernels.h) against the numpy restatement
of tests/bootsupport.py, in the kernel emulation; tests/test_gpu_boot_support.py runs the same checks on the device.  Distances,
weights, join slots and supports are compared as integers, every double bit for bit (njtree.same_records).  No tolerances.
Then the writer: with bootstrap=B the file .snps.boot.nwk is the restatement's for the .snps.mfa and the names of the same run, and
every other file has the bytes of a tree=1 run."""
import functools
import os

import numpy as np
import pytest

import bootsupport as bs
import njtree as nt
import test_nj_tree as T
import test_snp_columns as S
from parsnp_amd.binding import Lib, PmError

ROWS = (2, 3, 5, 33, 64, 65)
COLS = (0, 1, 63, 64, 65, 129, 513)      # 513: past one slab of 8 words; 65: a last word with one bit
REPS = (1, 2, 5, 7)                      # 5 and 7 are no multiple of the replicate group of 4
SEEDS = (1, 0xFEDCBA9876543210)
# (n, V, reps): every n, every V and every reps occur; the large shapes once
SHAPES = [(2, 65, 2), (3, 0, 5), (5, 1, 1), (33, 63, 7), (64, 64, 5), (65, 129, 2), (5, 513, 7), (65, 513, 5), (33, 0, 1)]
assert {s[0] for s in SHAPES} == set(ROWS) and {s[1] for s in SHAPES} == set(COLS) and {s[2] for s in SHAPES} == set(REPS) and bs.GROUP == 4


@pytest.fixture(scope="module")
def lib(emu):
    return Lib(emu[0])


@functools.lru_cache(maxsize=None)
def letters_of(n, v):
    return bs.snp_letters(n, v, 1000 * n + v)


def collection(s, letters):
    got = s.core_snps(bs.chunks_of(letters))
    assert got[0]["core_snps"] == letters.shape[1] and np.array_equal(got[2], letters)
    return got[3]


def same_ints(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        at = tuple(int(x) for x in np.argwhere(got != want)[0])
        raise AssertionError("%s: entry %r is %d, restatement %d (%d differ)" % (what, at, got[at], want[at], int((got != want).sum())))


# ------------------------------------------------------------------------------------------------------- weights and distances
def check_generated(lib, n, v, reps):
    letters = letters_of(n, v)
    with S.two_genomes(lib) as s:
        collection(s, letters)
        for seed in SEEDS:
            w, d = s.boot_distances(reps, seed)
            exp_w = bs.weights(reps, seed, v)
            same_ints(w, exp_w, "weights")
            same_ints(d, bs.distances(letters, exp_w), "distances")
            assert all(np.array_equal(x, x.T) and not x.diagonal().any() for x in d)
            if v:
                assert int(w.astype(np.int64).sum(axis=1).max()) <= v      # (equal to V unless the cap cut a counter)


@pytest.mark.parametrize("n,v,reps", SHAPES)
def test_generated_weights(lib, n, v, reps):
    check_generated(lib, n, v, reps)


def check_caller_weights(lib, n, v, reps):
    letters = letters_of(n, v)
    with S.two_genomes(lib) as s:
        plain = collection(s, letters)
        for name, w in bs.caller_weights(reps, v).items():
            got_w, d = s.boot_distances(reps, 0, w)
            same_ints(got_w, w, name)
            same_ints(d, bs.distances(letters, w), name)
            if name == "ones":
                assert all(np.array_equal(x, plain) for x in d)      # pm_snp_distances
            if name == "zeros":
                assert not d.any()
        if v:
            wide = np.zeros((reps, v + 9), np.uint8)      # a view whose rows lie further apart than V: the pitch
            wide[:, :v] = np.random.default_rng(v).integers(0, 16, (reps, v))
            same_ints(s.boot_distances(reps, 0, wide[:, :v])[1], bs.distances(letters, wide[:, :v]), "pitch")
            bad = np.ones((reps, v), np.uint8)
            bad[reps - 1, v - 1] = 16
            with pytest.raises(PmError, match=r"code -2"):
                s.boot_distances(reps, 0, bad)
            same_ints(s.boot_distances(reps, 0, np.ones((reps, v), np.uint8))[1][0], plain, "after a refused call")


@pytest.mark.parametrize("n,v,reps", [x for x in SHAPES if x[1]])
def test_caller_weights(lib, n, v, reps):
    check_caller_weights(lib, n, v, reps)


def check_batches(lib):
    """boot_batch 1 and 3 give the bytes of the default, through all three calls"""
    letters, w, d, trees, main, sup = bs.chain_case("33x129")
    n = letters.shape[0]
    for k in (0, 1, 3):
        with S.two_genomes(lib) as s:
            s.tune("boot_batch", k)
            collection(s, letters)
            gw, gd = s.boot_distances(7, bs.CHAIN_SEED)
            same_ints(gw, w[:7], "weights, batch %d" % k)
            same_ints(gd, d[:7], "distances, batch %d" % k)
            joins, last = s.nj_trees()
            for b in range(7):
                nt.same_records((joins[b], last[b]), trees[b])
            same_ints(s.nj_support(n, main[0]), bs.support(n, main[0], [t[0] for t in trees[:7]]), "support, batch %d" % k)
            own = np.array([t[0] for t in trees[:7]])
            same_ints(s.nj_support(n, main[0], own), bs.support(n, main[0], [t[0] for t in trees[:7]]), "support of caller's records, batch %d" % k)


def test_batches(lib):
    check_batches(lib)


def check_arguments(lib):
    assert lib.boot_limits() == (bs.MAX_ROWS, bs.MAX_REPS, bs.MAX_WEIGHT)
    letters = letters_of(5, 65)
    with S.two_genomes(lib) as s:
        with pytest.raises(PmError, match=r"code -2"):      # no collection
            s.boot_distances(2, 1)
        collection(s, letters)
        with pytest.raises(PmError, match=r"code -2"):      # no replicate distances yet
            s.nj_trees(n=5, count=2)
        with pytest.raises(PmError, match=r"code -2"):
            s.boot_distances(0, 1)
        with pytest.raises(PmError, match=r"code -5"):
            s.boot_distances(bs.MAX_REPS + 1, 1)
        s.boot_distances(2, 1)
        with pytest.raises(PmError, match=r"code -2"):      # more trees than replicates, another n
            s.nj_trees(n=5, count=3)
        with pytest.raises(PmError, match=r"code -2"):
            s.nj_trees(n=6, count=2)
        main = nt.nj(nt.random_matrix(5, 1))[0]
        with pytest.raises(PmError, match=r"code -2"):      # no records on the device yet
            s.nj_support(5, main, count=2)
        s.nj_trees(n=5, count=2)
        assert s.nj_support(5, main, count=2).shape == (2,)
        with pytest.raises(PmError, match=r"code -2"):
            s.nj_support(5, main, count=3)
        with pytest.raises(PmError, match=r"code -5"):
            s.nj_trees(np.zeros((1, 2049, 2049), np.int32))
        bad = np.array([nt.random_matrix(5, 1), nt.random_matrix(5, 2)])
        bad[1, 1, 3] += 1
        with pytest.raises(PmError, match=r"code -2"):      # the second matrix is not symmetric
            s.nj_trees(bad)
        with pytest.raises(PmError, match=r"code -2"):
            s.nj_trees(np.zeros((1, 2, 2), np.int32))
        names = [k for k, _ in s.last_timing()]
    return names


def test_arguments(lib):
    check_arguments(lib)


@pytest.mark.parametrize("launch", ["boot_pack", "snp_dist_boot", "nj_init_b", "nj_rowmin_b", "nj_last_b", "boot_splits", "boot_match"])
def test_wavefronts_of_a_launch_do_not_depend_on_one_another(lib, launch, monkeypatch):
    monkeypatch.setenv("PM_EMU_REVERSE_WAVES", launch)
    check_generated(lib, 65, 129, 2)
    check_chain(lib, "33x129")


# ------------------------------------------------------------------------------------------------------------- batched trees
@functools.lru_cache(maxsize=None)
def tree_batches():
    """name -> int32 [count, n, n]"""
    c = T.cases()
    b = {}
    b["designs130"] = [c["min_at_%d_%d" % p][0] for p in nt.WHERE] + [c["two_minima_one_row_" + k][0] for k in nt.TIES_ROW] + \
                      [c["two_minima_rows_lanes"][0], c["two_minima_rows_waves"][0], c["duplicated_rows"][0]]
    b["designs300"] = [c["two_minima_rows_waves_far"][0], c["two_minima_rows_thread"][0]]
    for n in (3, 4, 5, 63, 64, 65, 129, 257):
        for count in (1, 2, 5):
            if count == 1 or n in (3, 4, 65, 257) or (count == 2 and n in (5, 64)) or (count == 5 and n in (63, 129)):
                b["random%d_x%d" % (n, count)] = [nt.random_matrix(n, 7000 + 10 * n + k) for k in range(count)]
    b["zero_caterpillar_random80"] = [nt.constant(80, 0), nt.caterpillar(80), nt.random_matrix(80, 80)]
    out = {k: np.array(v, np.int32) for k, v in b.items()}
    assert {v.shape[1] for v in out.values()} >= {3, 4, 5, 63, 64, 65, 80, 129, 130, 257, 300}
    return out


@functools.lru_cache(maxsize=None)
def tree_want(name):
    return [nt.nj(d) for d in tree_batches()[name]]


BATCH_NAMES = list(tree_batches())


def check_trees(lib, name):
    dist = tree_batches()[name]
    with S.two_genomes(lib) as s:
        joins, last = s.nj_trees(dist)
        assert joins.shape == (dist.shape[0], dist.shape[1] - 3) and last.shape == (dist.shape[0],)
        for b, exp in enumerate(tree_want(name)):
            nt.same_records((joins[b], last[b]), exp)
        if dist.shape[0] == 1:      # count == 1 equals pm_nj_tree
            one = s.nj_tree(dist[0])
            nt.same_records(one, tree_want(name)[0])
            assert joins[0].tobytes() == one[0].tobytes()


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_trees(lib, name):
    check_trees(lib, name)


@functools.lru_cache(maxsize=None)
def limit_batch():
    """balanced(11) and a copy whose leaves are renumbered (leaf k of the copy is leaf k ^ 1365 of the design)"""
    dist, design = T.limit_case()
    p = np.arange(dist.shape[0]) ^ 1365
    renum = {frozenset(int(p[x]) for x in s): v for s, v in design.items()}
    everything = frozenset(range(dist.shape[0]))
    renum = {(everything - s if 0 in s else s): v for s, v in renum.items()}
    return np.array([dist, dist[np.ix_(p, p)]], np.int32), (design, renum)


def check_limit(lib):
    dist, designs = limit_batch()
    assert dist.shape == (2, nt.MAX_ROWS, nt.MAX_ROWS) and not np.array_equal(dist[0], dist[1])
    with S.two_genomes(lib) as s:
        joins, last = s.nj_trees(dist)
        names = [k for k, _ in s.last_timing()]
    for b in range(2):
        nt.check_balanced(nt.MAX_ROWS, joins[b], last[b], designs[b])
    return names


def test_limit(lib):
    check_limit(lib)


# ------------------------------------------------------------------------------------------------- support on caller's records
SUPPORT_ROWS = (4, 5, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def support_case(n):
    dist = nt.random_matrix(n, 300 + n)
    main = nt.nj(dist)[0]
    root = bs.nested(n, *nt.nj(dist))
    return dict(main=main, same=bs.records(root), reverse=bs.records(root, True), renumbered=bs.renumbered(dist, 7),
                interchange=bs.records(bs.interchange(root)), caterpillar=bs.records(bs.caterpillar_tree(n)), balanced=bs.records(bs.balanced_tree(n)))


def check_support(lib, n):
    c = support_case(n)
    main = c["main"]
    ones = np.ones(n - 3, np.int32)
    with S.two_genomes(lib) as s:
        def sup(m, reps):
            got = s.nj_support(n, m, np.array(reps))
            same_ints(got, bs.support(n, m, reps), "support")
            return got
        assert np.array_equal(sup(main, [main]), ones)
        for k in ("same", "reverse", "renumbered"):      # the same topology, the records in another order
            assert np.array_equal(sup(main, [c[k]]), ones), k
        if n > 5:
            assert not np.array_equal(c["reverse"]["i"], main["i"]) or not np.array_equal(c["reverse"]["j"], main["j"])
        one = sup(main, [c["interchange"]])
        assert int((one == 0).sum()) == 1 and int(one.sum()) == n - 4      # one nearest-neighbour interchange: exactly one split is gone
        # a main tree whose FIRST node holds leaf 0 (its split is the complement), and every later one too: the caterpillar
        cat, bal = c["caterpillar"], c["balanced"]
        assert (cat["i"] == 0).all() and bs.splits(n, cat)[0] == frozenset(range(2, n))
        assert np.array_equal(sup(cat, [cat]), ones)
        mixed = sup(cat, [bal])
        assert n < 6 or 0 < int(mixed.sum()) < n - 3
        sup(bal, [cat])
        three = sup(main, [main, c["interchange"], bal])
        assert np.array_equal(three, sup(main, [main]) + sup(main, [c["interchange"]]) + sup(main, [bal]))
        if n == 65:      # a split with leaf 64 alone in the second word
            pair = bs.records(((63, 64), bs.balanced_tree(63)[0], (bs.balanced_tree(63)[1], bs.balanced_tree(63)[2])))
            assert frozenset([63, 64]) in bs.splits(n, pair)
            assert int(sup(pair, [pair, main]).min()) >= 1
        for field, t, value in (("j", 0, n), ("i", 0, -1), ("j", 0, int(main["i"][0])), ("i", n - 4, int(main["j"][0]))):      # j out of range, i negative, i == j, a retired slot
            bad = main.copy()
            bad[field][t] = value
            with pytest.raises(PmError, match=r"code -2"):
                s.nj_support(n, main, np.array([main, bad]))
            with pytest.raises(PmError, match=r"code -2"):
                s.nj_support(n, bad, np.array([main]))
        assert np.array_equal(sup(main, [main]), ones)      # (a refused call leaves the session usable)


@pytest.mark.parametrize("n", SUPPORT_ROWS)
def test_support(lib, n):
    check_support(lib, n)


@functools.lru_cache(maxsize=None)
def support_limit_case():
    """2 048 leaves: sets of 32 words, the hash table at its 4 096 entries"""
    n = bs.MAX_ROWS
    bal, cat = bs.balanced_tree(n), bs.caterpillar_tree(n)
    main = bs.records(bal)
    reps = [bs.records(bal, True), bs.records(bs.interchange(bal)), bs.records(cat)]
    return main, reps, bs.support(n, main, reps), bs.support(n, reps[2], [main] + reps)


def check_support_limit(lib):
    main, reps, want, want_cat = support_limit_case()
    # (the split the interchange drops is one the caterpillar holds; 18 splits are in all four trees)
    assert np.bincount(want).tolist() == [0, 0, 2027, 18] and np.bincount(want_cat).tolist() == [0, 2026, 0, 1, 18]
    with S.two_genomes(lib) as s:
        same_ints(s.nj_support(bs.MAX_ROWS, main, np.array(reps)), want, "support at 2 048 leaves")
        same_ints(s.nj_support(bs.MAX_ROWS, reps[2], np.array([main] + reps)), want_cat, "support of the caterpillar at 2 048 leaves")


def test_support_limit(lib):
    check_support_limit(lib)


# ------------------------------------------------------------------------------------------------------------- the whole chain
def check_chain(lib, name):
    letters, w, d, trees, main, sup = bs.chain_case(name)
    n = letters.shape[0]
    with S.two_genomes(lib) as s:
        collection(s, letters)
        gw, gd = s.boot_distances(bs.CHAIN_REPS, bs.CHAIN_SEED)
        same_ints(gw, w, "weights")
        same_ints(gd, d, "distances")
        joins, last = s.nj_trees()
        for b in range(bs.CHAIN_REPS):
            nt.same_records((joins[b], last[b]), trees[b])
        mj, ml = s.nj_tree()      # (over the unweighted distances core_snps computed)
        nt.same_records((mj, ml), main)
        same_ints(s.nj_support(n, mj), sup, "support")
        names = [k for k, _ in s.last_timing()]
    return names


@pytest.mark.parametrize("name", list(bs.CHAIN_DESIGNS))
def test_chain(lib, name):
    check_chain(lib, name)


def test_designs():
    """what the designs promise, asserted of the restatement"""
    for name, (lo, top) in (("33x129", (10, 7)), ("65x513", (7, 6))):
        letters, w, d, trees, main, sup = bs.chain_case(name)
        n, v, _ = bs.CHAIN_DESIGNS[name]
        # branches that are sometimes absent and branches that never are; no counter reaches the cap
        assert (int(sup.min()), int(sup.max())) == (lo, bs.CHAIN_REPS) and len(set(sup.tolist())) > 5
        assert int(bs.counts(bs.CHAIN_REPS, bs.CHAIN_SEED, v).max()) == top < bs.MAX_WEIGHT
        assert (w.astype(np.int64).sum(axis=1) == v).all()
    assert int(bs.mix(np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF      # splitmix64's first output for the state 0
    assert bs.draws(3, 9, 0).shape == (0,) and bs.weights(2, 1, 0).shape == (2, 0)
    assert (bs.draws(0, 1, 1) == 0).all() and bs.weights(1, 1, 1)[0, 0] == 1
    root = ((0, 1), (2, 3), 4)
    assert bs.splits(5, bs.records(root)) == [frozenset([2, 3, 4]), frozenset([2, 3])]
    assert bs.records(root, True)["i"].tolist() == [2, 0] and bs.interchange(root) == ((0, (2, 3)), 1, 4)
    names = ["a", "b", "c", "d"]
    dist = np.array([[0, 2, 4, 6], [2, 0, 4, 6], [4, 4, 0, 5], [6, 6, 5, 0]])
    assert bs.newick(names, *nt.nj(dist), [7]) == "((a:1,b:1)7:1.5,c:1.5,d:3.5);"


# ---------------------------------------------------------------------------------------------------------------- the writer
BOOT = "parsnpAligner.snps.boot.nwk"
TIMING_KEYS = {"boot_reps", "boot_ms"}
E2E_REPS = 20


def check_boot_of(out, reps, seed=1):
    from parsnp_amd import driver
    names, letters, _, _ = driver.read_snps(out)
    text = driver.read_boot_tree(out)
    assert text == bs.newick_of(names, letters, reps, seed)
    return names, text


def check_e2e(core_bin, base, threads=4):
    import xmfa_util
    rp, qs = S.e2e_inputs("pop6x200k", base)
    (o1, t1), (o2, t2), (o3, t3) = (T.run(core_bin, rp, qs, base, tag, threads, **kw) for tag, kw in
                                    (("tree", dict(tree=1)), ("boot", dict(bootstrap=E2E_REPS)), ("seed", dict(tree=1, bootstrap=E2E_REPS, bootseed=77))))
    for f in ("parsnpAligner.xmfa", "parsnp.unalign", T.NWK) + S.FILES:
        assert xmfa_util.md5(os.path.join(o1, f)) == xmfa_util.md5(os.path.join(o2, f)), f
    strip = lambda p: [l for l in open(p) if "elapsed time" not in l and "running time" not in l]      # noqa: E731
    assert strip(os.path.join(o1, "parsnpAligner.log")) == strip(os.path.join(o2, "parsnpAligner.log"))
    assert sorted(set(os.listdir(o2)) - set(os.listdir(o1))) == [BOOT] and not os.path.exists(os.path.join(o1, BOOT))
    assert set(t2) - set(t1) == TIMING_KEYS and set(t1) <= set(t2) and not [k for k in t1 if k.startswith("boot_")]
    names, text = check_boot_of(o2, E2E_REPS)
    n = len(names)
    assert n == len(qs) + 1 and t2["boot_reps"] == E2E_REPS and t2["boot_ms"] >= 0
    assert text.count(")") == n - 2 and "Bootstrap: %d replicates of %d leaves on the device" % (E2E_REPS, n) in open(os.path.join(o2, "parsnp-aligner.err")).read()
    assert "Bootstrap" not in open(os.path.join(o1, "parsnp-aligner.err")).read()
    import re
    labels = [int(x) for x in re.findall(r"\)(\d+):", text)]
    assert len(labels) == n - 3 and all(0 <= x <= E2E_REPS for x in labels)
    check_boot_of(o3, E2E_REPS, 77)
    assert re.sub(r"\)\d+:", "):", text) == T.check_tree_of(o2, n)[1]      # the tree=1 text with the labels taken out


def test_files(emu, tmp_path):
    check_e2e(emu[1], str(tmp_path))


def check_few_and_too_many(core_bin, base, threads=4):
    """two and three sequences: no label, no device call for the bootstrap; bootstrap=1025 and too many sequences: exit 5 before any
    sequence is read"""
    from parsnp_amd import driver
    rp, qs = S.e2e_inputs("pop6x200k", base)
    for k in (1, 2):
        out, t = T.run(core_bin, rp, qs[:k], base, "few%d" % k, threads, bootstrap=5)
        names, text = check_boot_of(out, 5)
        assert len(names) == k + 1 and text == driver.read_tree(out) and t["boot_reps"] == 0 and t["boot_ms"] == 0
    qs = ["/nonexistent/g%d.fna" % i for i in range(2048)]
    for tag, q, kw in (("many", qs, dict(bootstrap=3)), ("reps", qs[:3], dict(bootstrap=1025))):
        rc, _ = driver.run_core(core_bin, "/nonexistent/ref.fna", q, os.path.join(base, tag), **kw)
        assert rc == 5 and "limit of the multi-MUM engine" in open(os.path.join(base, tag, "parsnp-aligner.err")).read()
    rc, _ = driver.run_core(core_bin, "/nonexistent/ref.fna", qs[:3], os.path.join(base, "ok"), bootstrap=1024)
    assert rc == 1      # (within the limits: the run goes on and fails to read the sequences)


def test_few_and_too_many(emu, tmp_path):
    check_few_and_too_many(emu[1], str(tmp_path))


def test_ini_text():
    from parsnp_amd import driver
    args = ("/x/ref.fna", ["/x/a.fna", "/x/b.fna"], "/x/out")
    assert driver.ini_text(*args, threads=3) == S.INI_TODAY
    assert driver.ini_text(*args, threads=3, bootstrap=100) == S.INI_TODAY + "bootstrap=100\n"
    assert driver.ini_text(*args, threads=3, tree=1, bootstrap=5, bootseed=9) == S.INI_TODAY + "tree=1\nbootstrap=5\nbootseed=9\n"
