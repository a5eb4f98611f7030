"""The recombination scan of the core SNP columns restated in numpy, and the designs of tests/test_rec_phi.py and
tests/test_gpu_rec_phi.py.  Pure Python and numpy, written from the definition:

informative flags are letter counts per column; windows are lists of positions in an LCB's site list; `inc` of two columns builds
the bipartite graph of their letters (an edge per pair of letters that share a row) and counts its edges, vertices and connected
components with a union-find; a permutation is a stable argsort of uint64 keys; T sums the matrix over the pairs of positions at
most h apart; the two files are formatted line by line."""
import functools

import numpy as np

from bootsupport import mix

MAX_ROWS, MAX_SITES, MAX_PERMS = 2048, 256, 65536
_MASK = (1 << 64) - 1
_ACGT = np.frombuffer(b"ACGT", np.uint8)
HEADER = "cluster\tfirst_column\tlast_column\tfirst_ref\tlast_ref\tsites\tphi\tle\tperms\tp\n"


def informative(letters):
    """uint8 [V]: 1 where at least two letters occur in at least two rows each"""
    n, v = letters.shape
    many = sum(((letters == c).sum(axis=0) >= 2).astype(np.int64) for c in _ACGT) if v else np.zeros(0, np.int64)
    return (many >= 2).astype(np.uint8).reshape(v)


def window_starts(m, K=100):
    """the starts of the windows over a site list of length m"""
    if m < 16:
        return []
    if m < K:
        return [0]
    step = K // 2
    starts = list(range(0, m - K + 1, step))
    if starts[-1] + K != m:
        starts.append(m - K)
    return starts


def windows_of(m, K=100):
    """[(start, length)]"""
    return [(s, min(K, m)) for s in window_starts(m, K)]


def inc(x, y):
    """the score of two columns (uint8 [n] of A C G T each) by the graph definition"""
    edges = sorted(set(zip((int(a) for a in x), (int(b) + 256 for b in y))))
    verts = sorted(set(v for e in edges for v in e))
    parent = {v: v for v in verts}

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    for a, b in edges:
        parent[find(a)] = find(b)
    comps = len(set(find(v) for v in verts))
    return len(edges) - len(verts) + comps


@functools.lru_cache(maxsize=None)
def mask_score(mask):
    """the score of an edge mask (bit 4 a + b: letter a at x and letter b at y share a row), by the same graph definition"""
    pairs = [(a, b) for a in range(4) for b in range(4) if mask >> (4 * a + b) & 1]
    return inc(np.array([a for a, _ in pairs], np.uint8), np.array([b for _, b in pairs], np.uint8))


def masks(letters, sites):
    """int64 [k, k]: the edge masks of all pairs of a window's sites (one-hot products; counts up to 2 048 are exact in float32)"""
    hot = [(letters[:, np.asarray(sites, np.int64)] == c).astype(np.float32) for c in _ACGT]
    out = np.zeros((len(sites), len(sites)), np.int64)
    for a in range(4):
        for b in range(4):
            out |= ((hot[a].T @ hot[b]) > 0).astype(np.int64) << (4 * a + b)
    return out


def matrix(letters, sites):
    """uint8 [k, k] of a window's sites (indices into the columns of `letters`); the diagonal is 0"""
    m = masks(letters, sites)
    out = np.zeros(m.shape, np.uint8)
    for value in np.unique(m):
        out[m == value] = mask_score(int(value))
    np.fill_diagonal(out, 0)
    return out


def stat(mat, order, near):
    k = len(order)
    h = min(near, k - 1)
    m = mat[np.ix_(order, order)].astype(np.int64)
    return int(sum(np.trace(m, offset=d) for d in range(1, h + 1)))


def orders(g, k, perms, seed):
    """int64 [perms, k]: the permuted orders of window number g"""
    with np.errstate(over="ignore"):
        wkey = mix(np.array([(seed + g) & _MASK], np.uint64))[0]
        pkey = mix(wkey + np.arange(perms, dtype=np.uint64))
        keys = mix(pkey[:, None] + np.arange(k, dtype=np.uint64)[None, :])
    return np.argsort(keys, axis=1, kind="stable")


def test_window(mat, g, near, perms, seed):
    """-> (phi, le)"""
    k = mat.shape[0]
    h = min(near, k - 1)
    phi = stat(mat, np.arange(k), near)
    o = orders(g, k, perms, seed)
    m = mat.astype(np.int64)
    t = np.zeros(perms, np.int64)
    for d in range(1, h + 1):
        t += m[o[:, :-d], o[:, d:]].sum(axis=1)
    return phi, int((t <= phi).sum())


test_window.__test__ = False


def flagged(le, perms):
    return 100 * (le + 1) < perms + 1


def lcb_runs(rows):
    """[(first row, one past the last)] of every run of rows of one cluster: the LCBs as printed"""
    out, a = [], 0
    for i in range(1, len(rows) + 1):
        if i == len(rows) or rows[i][0] != rows[a][0]:
            out.append((a, i))
            a = i
    return out if rows else []


def scan(letters, rows, perms=1000, seed=1, K=100, near=10):
    """letters uint8 [n, V] and rows [(cluster, column, ref_pos)] of the .snps files -> the window records, in order g"""
    n, v = letters.shape
    info = informative(letters) if n >= 4 else np.zeros(v, np.uint8)
    recs = []
    for a, b in lcb_runs(rows):
        sites = [c for c in range(a, b) if info[c]]
        for s, k in windows_of(len(sites), K):
            win = sites[s:s + k]
            phi, le = test_window(matrix(letters, win), len(recs), near, perms, seed)
            ref = [rows[c][2] for c in win]
            recs.append(dict(cluster=rows[win[0]][0], first_column=rows[win[0]][1], last_column=rows[win[-1]][1], first_ref=min(ref), last_ref=max(ref),
                             sites=k, phi=phi, le=le, perms=perms, flagged=flagged(le, perms), g=len(recs)))
    return recs, int(info.sum())


def files_text(recs):
    """-> (the text of .rec.tsv, the text of .rec)"""
    tsv = HEADER
    for r in recs:
        p = (r["le"] + 1) / (r["perms"] + 1)
        tsv += "%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\n" % (r["cluster"], r["first_column"], r["last_column"], r["first_ref"], r["last_ref"], r["sites"], r["phi"],
                                                                 r["le"], r["perms"], p)
    bed = ""
    for r in sorted((r for r in recs if r["flagged"]), key=lambda r: (r["first_ref"], r["g"])):
        bed += "1\t%d\t%d\tREC\t%.3f\t+\n" % (r["first_ref"], r["last_ref"] + 1, (r["le"] + 1) / (r["perms"] + 1))
    return tsv, bed


# ------------------------------------------------------------------------------------------------------------------- designs
def random_letters(n, v, seed):
    """n x v letters, every column a core SNP (rows 0 and 1 differ)"""
    rng = np.random.default_rng(seed)
    code = rng.integers(0, 4, (n, v))
    if n >= 2 and v:
        code[1] = (code[0] + rng.integers(1, 4, v)) % 4
    return _ACGT[code].astype(np.uint8)


def tree_letters(n, v, seed, lo=2, hi=None):
    """columns that all fit ONE tree (a caterpillar over the rows in order): column c gives the rows before a cut one letter and
    the rest another; cuts between lo >= 2 and hi <= n - 2, so every column is informative for n >= 4"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, v), np.uint8)
    hi = n - 2 if hi is None else hi
    for c in range(v):
        cut = int(rng.integers(lo, hi + 1))
        a, b = rng.choice(4, 2, replace=False)
        out[:cut, c], out[cut:, c] = _ACGT[a], _ACGT[b]
    return out


def mosaic_letters(n=12, first=20, second=20, seed=3):
    """the first columns fit the caterpillar over the rows in order (splits {0, 1}, {0, 1, 2} or {0 ... 3} against the rest), the
    others the caterpillar over the even rows, then the odd ones (splits {0, 2, 4}, ... {0, 2 ... 10} against the rest).  A split of
    either kind meets the other kind's in row 0, holds a row the other lacks (row 1; row 4) and leaves the last row out with it: all
    four pairs of letters occur, so every pair of columns across the break point scores 1 and every pair on one side 0."""
    assert n >= 12
    a = tree_letters(n, first, seed, 2, 4)
    perm = np.concatenate((np.arange(0, n, 2), np.arange(1, n, 2)))
    b = np.zeros((n, second), np.uint8)
    b[perm] = tree_letters(n, second, seed + 1, 3, 6)
    return np.concatenate((a, b), axis=1)


@functools.lru_cache(maxsize=None)
def pair_design():
    """16 rows, and columns whose pairs reach every class of 4 x 4 edge mask the test names: 2, 3, 4 letters on either side, forests,
    one cycle, the complete graph, two components.  Every column over 16 rows from a small alphabet of patterns."""
    r = np.arange(16)
    pats = {
        "two": r // 8,                      # 2 letters, 8 rows each
        "two_b": r % 2,                     # 2 letters, interleaved: with `two` a 4-cycle
        "three": np.minimum(r // 4, 2),     # 3 letters
        "four": r // 4,                     # 4 letters: nested in `two` (forest)
        "four_b": r % 4,                    # with `four` the complete 4 x 4 graph (score 9)
        "four_c": (r // 4 + (r % 4 == 3)) % 4,      # with `four` one cycle of length 8
        "same": r // 8 * 3,                 # `two` with other letters: two components, score 0
        "three_b": (r % 4 == 0) + 2 * (r % 4 == 1),
        "single": (r == 15) * 1,            # differs in the last row only
        "single0": (r == 0) * 2,
    }
    names = list(pats)
    letters = np.array([_ACGT[pats[k]] for k in names], np.uint8).T.copy()
    return names, letters


def conflict_in_one_row(n, row):
    """two columns over n rows that conflict (score 1) only because of `row`: without it three of the four letter pairs occur"""
    x = np.zeros(n, np.int64)
    y = np.zeros(n, np.int64)
    x[1], y[1] = 1, 0
    x[0], y[0] = 0, 1
    x[row], y[row] = 1, 1
    x[2:row] = 0
    rest = [i for i in range(2, n) if i != row]
    for i in rest:
        x[i], y[i] = 0, 0
    return _ACGT[x].astype(np.uint8), _ACGT[y].astype(np.uint8)


def snps_rows(v, lcbs=1):
    """rows of a .snps.tsv for v columns spread over `lcbs` clusters: (cluster, column, ref_pos)"""
    per = -(-v // lcbs) if v else 1
    return [(1 + c // per, 3 * (c % per), 1000 * (c // per) + 7 * (c % per) + 5) for c in range(v)]
