"""Bootstrap support of the SNP tree restated in numpy, and the designs of tests/test_boot_support.py and
tests/test_gpu_boot_support.py.  Pure Python and numpy.

`mix` works on uint64 arrays (arithmetic modulo 2^64), the weights are `np.bincount` of the draws capped at 15, a replicate's
distances are the weighted Hamming distances of the letter rows, its tree is `njtree.nj` of them, and a split is a frozenset of
leaves (the side without leaf 0).  support[t] counts the replicate trees that hold the split of join t of the main tree."""
import functools

import numpy as np

import njtree as nt

MAX_ROWS, MAX_REPS, MAX_WEIGHT = 2048, 1024, 15
GROUP = 4                       # replicates a wavefront of SnpDistBoot serves (boot_kernels.h: kBootGroup)
_MASK = (1 << 64) - 1
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def mix(z):
    z = np.asarray(z, np.uint64).copy()
    with np.errstate(over="ignore"):
        z += np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draws(b, seed, v):
    """the V columns replicate b picks, in draw order"""
    key = int(mix(np.array([(seed + b) & _MASK], np.uint64))[0])
    with np.errstate(over="ignore"):
        m = mix(np.uint64(key) + np.arange(v, dtype=np.uint64))
    return (((m >> np.uint64(32)) * np.uint64(v)) >> np.uint64(32)).astype(np.int64)


def counts(reps, seed, v):
    """uncapped: how often replicate b drew column v, int64 [reps, V]"""
    return np.array([np.bincount(draws(b, seed, v), minlength=v) for b in range(reps)], np.int64).reshape(reps, v)


def weights(reps, seed, v):
    return np.minimum(MAX_WEIGHT, counts(reps, seed, v)).astype(np.uint8)


def distances(letters, w):
    """letters uint8 [n, V] of A C G T, w [reps, V] -> int32 [reps, n, n]: the sum of w over the columns in which two rows differ
    (the weighted one-hot product in float64 is exact: sums below 2^53)"""
    n, v = letters.shape
    w = np.asarray(w, np.float64)
    w = w.reshape(w.shape[0] if w.ndim == 2 else 1, v)
    hot = [(letters == c).astype(np.float64) for c in _ACGT]
    out = np.zeros((w.shape[0], n, n), np.int32)
    for b in range(w.shape[0]):
        same = sum((h * w[b]) @ h.T for h in hot) if v else np.zeros((n, n))
        out[b] = np.rint(w[b].sum() - same).astype(np.int32)
    return out


def splits(n, joins):
    """the split of every join, in join order"""
    held = [frozenset([k]) for k in range(n)]
    everything = frozenset(range(n))
    out = []
    for t in range(n - 3):
        i, j = int(joins["i"][t]), int(joins["j"][t])
        held[i] = held[i] | held[j]
        held[j] = None
        out.append(everything - held[i] if 0 in held[i] else held[i])
    assert len(set(out)) == len(out)
    return out


def support(n, main_joins, rep_joins):
    sets = [set(splits(n, j)) for j in rep_joins]
    return np.array([sum(s in x for x in sets) for s in splits(n, main_joins)], np.int32).reshape(max(n - 3, 0))


def newick(names, joins, last, sup):
    """njtree.newick with the support of join t behind its node"""
    n = len(names)
    li, lj, (la, lb, lc) = nt.lengths(n, joins, last)
    slot = [nt.quote(x) for x in names]
    for t in range(n - 3):
        i, j = int(joins["i"][t]), int(joins["j"][t])
        slot[i] = "(%s:%s,%s:%s)%d" % (slot[i], nt.fmt(li[t]), slot[j], nt.fmt(lj[t]), int(sup[t]))
        slot[j] = None
    return "(%s:%s,%s:%s,%s:%s);" % (slot[int(last["a"])], nt.fmt(la), slot[int(last["b"])], nt.fmt(lb), slot[int(last["c"])], nt.fmt(lc))


def chain(letters, reps, seed):
    """the whole of 1c for a letter matrix -> (weights, dist [reps, n, n], [(joins, last)] per replicate, (joins, last) of the main
    tree, support)"""
    n, v = letters.shape
    w = weights(reps, seed, v)
    d = distances(letters, w)
    trees = [nt.nj(d[b]) for b in range(reps)]
    main = nt.nj(distances(letters, np.ones((1, v)))[0])
    return w, d, trees, main, support(n, main[0], [t[0] for t in trees])


def newick_of(names, letters, reps, seed):
    """the text of .snps.boot.nwk (without its newline) for the names and letters of a run"""
    n, v = letters.shape
    d = distances(letters, np.ones((1, v)))[0]
    if n <= 3:
        return nt.newick_of(names, d)
    _, _, _, main, sup = chain(letters, reps, seed)
    return newick(names, main[0], main[1], sup)


# ------------------------------------------------------------------------------------------------------------------ designs
def snp_letters(n, v, seed):
    """n x v letters in which every column is a core SNP: rows 0 and 1 differ everywhere"""
    rng = np.random.default_rng(seed)
    code = rng.integers(0, 4, (n, v))
    code[1] = (code[0] + rng.integers(1, 4, v)) % 4
    return _ACGT[code].astype(np.uint8)


def invariant_chunk(n, w=40):
    return np.full((n, w), ord("A"), np.uint8)


def chunks_of(letters):
    """what to hand to core_snps for a collection of exactly these core SNP columns (V = 0: a chunk without a core SNP)"""
    return [letters] if letters.shape[1] else [invariant_chunk(letters.shape[0])]


def mutated_rows(n, v, seed, per_row=0.06):
    """a letter matrix whose rows are mutated from one another: row k copies an earlier row and changes a share of the columns, and
    column c is changed in row 1 + c % (n - 1) at the least, so every column is a core SNP.  Clades with many columns behind them
    and clades with a few."""
    rng = np.random.default_rng(seed)
    code = np.zeros((n, v), np.int64)
    code[0] = rng.integers(0, 4, v)
    for k in range(1, n):
        code[k] = code[rng.integers(max(0, k - 3), k)]
        hit = rng.random(v) < per_row * rng.random()
        hit[np.arange(v) % (n - 1) == k - 1] = True
        code[k, hit] = (code[k, hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    letters = _ACGT[code].astype(np.uint8)
    assert (letters != letters[0]).any(axis=0).all()
    return letters


CHAIN_REPS, CHAIN_SEED = 40, 12345
CHAIN_DESIGNS = {"33x129": (33, 129, 5), "65x513": (65, 513, 6)}


@functools.lru_cache(maxsize=None)
def chain_case(name):
    n, v, seed = CHAIN_DESIGNS[name]
    letters = mutated_rows(n, v, seed)
    return (letters,) + chain(letters, CHAIN_REPS, CHAIN_SEED)


def caller_weights(reps, v):
    """name -> uint8 [reps, V]"""
    out = {"zeros": np.zeros((reps, v), np.uint8), "ones": np.ones((reps, v), np.uint8), "fifteens": np.full((reps, v), 15, np.uint8)}
    for p in (1, 2, 4, 8):
        out["plane%d" % p] = np.full((reps, v), p, np.uint8)
    for rank in sorted({0, 63, 64, v - 1}):
        if 0 <= rank < v:
            w = np.zeros((reps, v), np.uint8)
            w[:, rank] = 15
            out["one_at_%d" % rank] = w
    return out


# trees as nested tuples: a leaf is an int, an inner node a pair, the root a triple
def nested(n, joins, last):
    slot = list(range(n))
    for t in range(n - 3):
        i, j = int(joins["i"][t]), int(joins["j"][t])
        slot[i] = (slot[i], slot[j])
        slot[j] = None
    return tuple(slot[int(last[f])] for f in "abc")


def records(root, reverse=False):
    """join records (doubles zero) of a nested tree: every inner node below the root in a post-order (reverse: the children and the
    root's subtrees in the opposite order), a subtree living in the slot of its smallest leaf"""
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * MAX_ROWS))      # (a caterpillar is as deep as it has leaves)
    out = []

    def walk(node):
        if isinstance(node, int):
            return node
        kids = [walk(k) for k in (node[::-1] if reverse else node)]
        out.append((min(kids), max(kids)))
        return min(kids)
    for sub in (root[::-1] if reverse else root):
        walk(sub)
    rec = np.zeros(len(out), nt.JOIN)
    rec["i"], rec["j"] = [a for a, _ in out], [b for _, b in out]
    return rec


def interchange(root):
    """one nearest-neighbour interchange at the root's first inner subtree: ((A, B), c, d) -> ((A, c), B, d)"""
    subs = list(root)
    k = next(x for x in range(3) if not isinstance(subs[x], int))
    o = (k + 1) % 3
    (a, b), c = subs[k], subs[o]
    subs[k], subs[o] = (a, c), b
    return tuple(subs)


def caterpillar_tree(n):
    node = (0, 1)
    for k in range(2, n - 2):
        node = (node, k)
    return (node, n - 2, n - 1)


def balanced_tree(n):
    def build(lo, hi):
        return lo if hi - lo == 1 else (build(lo, (lo + hi) // 2), build((lo + hi) // 2, hi))
    a, b = n // 3, 2 * n // 3
    return (build(0, max(a, 1)), build(max(a, 1), max(b, 2)), build(max(b, 2), n))


def renumbered(dist, seed):
    """the records of nj over the matrix with its leaves renumbered, told in the ORIGINAL numbers: the same tree unless a tie fell
    differently, its nodes in the slots of their smallest leaves"""
    n = dist.shape[0]
    p = np.random.default_rng(seed).permutation(n)
    joins, _ = nt.nj(dist[np.ix_(p, p)])
    cur = [int(x) for x in p]
    rec = np.zeros(n - 3, nt.JOIN)
    for t in range(n - 3):
        i, j = int(joins["i"][t]), int(joins["j"][t])
        a, b = cur[i], cur[j]
        rec[t]["i"], rec[t]["j"] = min(a, b), max(a, b)
        cur[i] = min(a, b)
    return rec
