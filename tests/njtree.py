"""The neighbour-joining tree of INTEGRATION.md 1b restated in numpy, and the designs of the test matrices (test_nj_tree.py,
test_gpu_nj_tree.py).

Everything is IEEE double arithmetic, every operation rounded once in the order written: numpy evaluates one elementwise operation
per call and never fuses two.  Each join works on the ACTIVE SUBMATRIX; `np.argmin` over its row-major upper triangle is the tie
rule (the first of the smallest values: the smallest i, then the smallest j; -0 and +0 compare equal)."""
import re

import numpy as np

JOIN = np.dtype([("i", np.int32), ("j", np.int32), ("dij", np.float64), ("ri", np.float64), ("rj", np.float64)])
LAST = np.dtype([("a", np.int32), ("b", np.int32), ("c", np.int32), ("dab", np.float64), ("dac", np.float64), ("dbc", np.float64)])
MAX_ROWS = 2048


def nj(dist):
    """dist: int [n, n], symmetric, zero diagonal, no negative entry, n >= 3 -> (joins [n - 3] of JOIN, last of LAST)"""
    dist = np.asarray(dist)
    n = dist.shape[0]
    assert n >= 3 and dist.shape == (n, n) and np.array_equal(dist, dist.T) and not dist.diagonal().any() and dist.min() >= 0
    D = dist.astype(np.float64)
    R = dist.astype(np.int64).sum(axis=1).astype(np.float64)      # below 2^42: exact
    act = np.arange(n)
    joins = np.zeros(n - 3, JOIN)
    for t in range(n - 3):
        r = n - t
        assert len(act) == r
        sub, ra = D[np.ix_(act, act)], R[act]
        q = ((np.float64(r - 2) * sub) - ra[:, None]) - ra[None, :]      # in the upper triangle the row is the lower slot
        iu = np.triu_indices(r, 1)                                      # row-major
        k = int(np.argmin(q[iu]))
        i, j = int(act[iu[0][k]]), int(act[iu[1][k]])
        dij, ri, rj = D[i, j], R[i], R[j]
        joins[t] = (i, j, dij, ri, rj)
        oth = act[(act != i) & (act != j)]
        dik, djk = D[i, oth].copy(), D[j, oth].copy()
        du = ((dik + djk) - dij) * 0.5
        R[oth] = ((R[oth] - dik) - djk) + du
        D[i, oth] = du
        D[oth, i] = du
        R[i] = ((ri + rj) - np.float64(r) * dij) * 0.5
        act = act[act != j]
    a, b, c = (int(x) for x in act)
    last = np.zeros(1, LAST)[0]
    last["a"], last["b"], last["c"], last["dab"], last["dac"], last["dbc"] = a, b, c, D[a, b], D[a, c], D[b, c]
    return joins, last


def lengths(n, joins, last):
    """-> (li [n - 3], lj [n - 3], (la, lb, lc)), float64"""
    r = n - np.arange(n - 3, dtype=np.float64)
    li = 0.5 * joins["dij"] + (joins["ri"] - joins["rj"]) / (2.0 * (r - 2.0))
    lj = joins["dij"] - li
    dab, dac, dbc = np.float64(last["dab"]), np.float64(last["dac"]), np.float64(last["dbc"])
    return li, lj, (((dab + dac) - dbc) * 0.5, ((dab + dbc) - dac) * 0.5, ((dac + dbc) - dab) * 0.5)


def fmt(v):
    return "0" if v == 0 else "%.10g" % float(v)


def quote(name):
    return name if re.fullmatch(r"[A-Za-z0-9_.-]+", name) else "'" + name.replace("'", "''") + "'"


def newick(names, joins, last):
    n = len(names)
    li, lj, (la, lb, lc) = lengths(n, joins, last)
    slot = [quote(x) for x in names]
    for t in range(n - 3):
        i, j = int(joins["i"][t]), int(joins["j"][t])
        slot[i] = "(%s:%s,%s:%s)" % (slot[i], fmt(li[t]), slot[j], fmt(lj[t]))
        slot[j] = None
    return "(%s:%s,%s:%s,%s:%s);" % (slot[int(last["a"])], fmt(la), slot[int(last["b"])], fmt(lb), slot[int(last["c"])], fmt(lc))


def newick_of(names, dist):
    """the whole file (without its newline) from names and distances, n >= 2"""
    dist = np.asarray(dist)
    if len(names) == 2:
        h = fmt(0.5 * np.float64(dist[0, 1]))
        return "(%s:%s,%s:%s);" % (quote(names[0]), h, quote(names[1]), h)
    return newick(names, *nj(dist))


def same_records(got, want):
    """joins and slots as integers, every double bit for bit; got: the binding's arrays (its last record has a padding field)"""
    gj, gl = got
    wj, wl = want
    assert len(gj) == len(wj)
    for f in ("i", "j"):
        if not np.array_equal(gj[f], wj[f]):
            t = int(np.argmax(gj[f] != wj[f]))
            raise AssertionError("join %d is (%d, %d), restatement (%d, %d)" % (t, gj["i"][t], gj["j"][t], wj["i"][t], wj["j"][t]))
    for f in ("dij", "ri", "rj"):
        a, b = np.ascontiguousarray(gj[f]).view(np.int64), np.ascontiguousarray(wj[f]).view(np.int64)
        if not np.array_equal(a, b):
            t = int(np.argmax(a != b))
            raise AssertionError("%s of join %d is %r, restatement %r" % (f, t, float(gj[f][t]), float(wj[f][t])))
    assert [int(gl[f]) for f in "abc"] == [int(wl[f]) for f in "abc"]
    for f in ("dab", "dac", "dbc"):
        assert np.float64(gl[f]).view(np.int64) == np.float64(wl[f]).view(np.int64), (f, float(gl[f]), float(wl[f]))


def splits(n, joins, last, li, lj, l3):
    """{leaf set of the side without leaf 0 (a frozenset): branch length} of the unrooted tree: 2 n - 3 edges"""
    held = [frozenset([k]) for k in range(n)]
    everything = frozenset(range(n))
    out = {}

    def edge(s, length):
        s = everything - s if 0 in s else s
        assert s not in out
        out[s] = float(length)
    for t in range(n - 3):
        i, j = int(joins["i"][t]), int(joins["j"][t])
        edge(held[i], li[t]); edge(held[j], lj[t])      # noqa: E702
        held[i] = held[i] | held[j]
        held[j] = None
    for s, length in zip("abc", l3):
        edge(held[int(last[s])], length)
    return out


# ------------------------------------------------------------------------------------------------------------------ designs
def random_matrix(n, seed):
    """seeded random integers below 1 000, symmetrised, zero diagonal"""
    a = np.triu(np.random.default_rng(seed).integers(0, 1000, (n, n)), 1)
    return (a + a.T).astype(np.int32)


def constant(n, c, ones=()):
    d = np.full((n, n), c, np.int32)
    np.fill_diagonal(d, 0)
    for a, b in ones:
        d[a, b] = d[b, a] = 1
    return d


WHERE_N, WHERE_C = 130, 100
WHERE = [(0, 1), (62, 63), (63, 64), (64, 65), (127, 128), (0, WHERE_N - 1), (WHERE_N - 2, WHERE_N - 1)]
# two equal minima: ((a, b), (c, d)) with d = 1 for both, the first one the pair the definition joins.  In different rows: rows that are
# different lanes of one wavefront of NjJoin, rows of different wavefronts, rows of one thread (t and t + 256); in one row: columns in
# different lanes of one pass of NjRowMin, in one lane of different passes, and a later pass that holds the smaller lane
TIES_ROWS = {"lanes": (130, (3, 100), (5, 70)), "waves": (130, (10, 120), (70, 100)), "waves_far": (300, (63, 299), (64, 65)),
             "thread": (300, (5, 270), (261, 280))}
TIES_ROW = {"lanes": (130, (2, 40), (2, 50)), "passes": (130, (2, 30), (2, 94)), "later_lane": (130, (2, 45), (2, 100)), "edge": (130, (63, 64), (63, 129))}


def duplicated_rows(n, seed, pairs=((3, 70), (64, 65), (0, 129))):
    """a random matrix in which b is a copy of a (distance 0 between them) for every (a, b)"""
    d = random_matrix(n, seed)
    for a, b in pairs:
        d[b, :] = d[a, :]; d[:, b] = d[:, a]      # noqa: E702
        d[a, b] = d[b, a] = 0
        d[b, b] = 0
    assert np.array_equal(d, d.T) and not d.diagonal().any()
    return d


def caterpillar(n=80, seed=7):
    """a caterpillar-shaped metric that is NOT additive: leaf k hangs at spine node k, the spine's edges grow towards the far end (the
    cherry at the near end is joined first and the new node is joined again and again), and odd noise on every distance makes every
    one of those joins halve an odd numerator: one more fractional bit per join, more than 52 in a row"""
    rng = np.random.default_rng(seed)
    pend = rng.integers(1, 20, n)
    spine = np.concatenate([[0], np.cumsum(20 + 40 * np.arange(n - 1))])
    d = np.abs(spine[:, None] - spine[None, :]) + pend[:, None] + pend[None, :]
    noise = np.triu(rng.integers(0, 2, (n, n)) * 2 + 1, 1)
    d = d + noise + noise.T
    np.fill_diagonal(d, 0)
    return d.astype(np.int32)


def rounds(dist, joins):
    """whether the definition's doubles round somewhere on this matrix: the updates of D along the given joins once more in exact
    rational arithmetic; True when a distance of the last three slots differs from what nj() computed in doubles"""
    from fractions import Fraction
    n = dist.shape[0]
    D = [[Fraction(int(x)) for x in row] for row in dist]
    act = list(range(n))
    for t in range(n - 3):
        i, j = int(joins["i"][t]), int(joins["j"][t])
        for k in act:
            if k != i and k != j:
                D[i][k] = D[k][i] = (D[i][k] + D[j][k] - D[i][j]) / 2
        act.remove(j)
    last = nj(dist)[1]
    a, b, c = act
    return [D[a][b], D[a][c], D[b][c]] != [Fraction(float(last[f])) for f in ("dab", "dac", "dbc")]


def longest_chain(joins):
    """the longest run of successive joins in which the node made by the join before is joined again"""
    best = run = 0
    for t in range(1, len(joins)):
        run = run + 1 if joins["i"][t - 1] in (joins["i"][t], joins["j"][t]) else 0
        best = max(best, run)
    return best


def balanced(levels, seed=11):
    """an additive metric of a balanced binary tree with 2^levels leaves and integer edge lengths (1 .. 9) -> (dist int32, {split:
    length} of the unrooted tree as `splits` gives it).  Node v of level l (the root is level 0) spans the leaves v * 2^(levels - l) ..."""
    n = 1 << levels
    rng = np.random.default_rng(seed)
    edge = [None] + [rng.integers(1, 10, 1 << lv) for lv in range(1, levels + 1)]      # edge[l][v]: from node v of level l to its parent
    depth = np.zeros((levels + 1, n), np.int64)                                       # depth[l][leaf]: root to the leaf's ancestor of level l
    leaf = np.arange(n)
    for lv in range(1, levels + 1):
        depth[lv] = depth[lv - 1] + edge[lv][leaf >> (levels - lv)]
    x = leaf[:, None] ^ leaf[None, :]
    lca = np.full((n, n), levels, np.int64)      # level of the lowest common ancestor: levels - bit length of a xor b
    for b in range(levels):
        lca[x >= (1 << b)] = levels - 1 - b
    h = depth[levels]
    dist = h[:, None] + h[None, :] - 2 * depth[lca, leaf[:, None]]
    np.fill_diagonal(dist, 0)
    want = {}
    for lv in range(2, levels + 1):
        for v in range(1 << lv):
            w = 1 << (levels - lv)
            s = frozenset(range(v * w, (v + 1) * w))
            want[s] = float(edge[lv][v])
    want[frozenset(range(n // 2, n))] = float(edge[1][0] + edge[1][1])      # the root's two edges are one edge of the unrooted tree
    for s in [s for s in want if 0 in s]:
        want[frozenset(range(n)) - s] = want.pop(s)
    assert len(want) == 2 * n - 3
    return dist.astype(np.int32), want


def check_balanced(n, joins, last, want):
    li, lj, l3 = lengths(n, joins, last)
    got = splits(n, joins, last, li, lj, l3)
    assert got.keys() == want.keys(), "the splits differ from the design's"
    bad = [s for s in got if got[s] != want[s]]
    assert not bad, "%d branch lengths differ from the design's, e.g. %r against %r" % (len(bad), got[bad[0]], want[bad[0]])
