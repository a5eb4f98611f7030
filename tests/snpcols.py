"""Core SNP columns and SNP distances: the definitions restated in numpy, a scan of an XMFA by them, and the designed column
matrices of tests/test_snp_columns.py and tests/test_gpu_snp_columns.py.  Pure Python and numpy; of the product it reads only
output files.

Judged case-insensitively, a column is a CORE SNP when every row holds one of A C G T and at least two different letters occur,
CORE INVARIANT when every row holds the same one of the four, OTHER when some row holds anything else.  The SNP matrix is the core
SNP columns in input order, upper case; dist[i][j] is the number of core SNP columns in which rows i and j differ.  In an XMFA the
reference position of a column is the `a` of `> 1:a-b` of its LCB plus the characters other than '-' of the reference row to its
left."""
import re

import numpy as np

INV, SNP, OTHER = 0, 1, 2
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def upper(m):
    m = np.asarray(m, np.uint8)
    return np.where((m >= 97) & (m <= 122), m - 32, m).astype(np.uint8)


def classes(m):
    """class of every column of an (n, w) uint8 matrix"""
    u = upper(m)
    if u.shape[1] == 0:
        return np.zeros(0, np.int64)
    core = np.isin(u, _ACGT).all(axis=0)
    varies = (u != u[0]).any(axis=0)
    return np.where(~core, OTHER, np.where(varies, SNP, INV))


def distances(letters):
    """Hamming distances of the rows of an (n, V) matrix of A C G T: V minus the one-hot dot product"""
    n, v = letters.shape
    hot = np.concatenate([(letters == c) for c in _ACGT], axis=1).astype(np.float32)      # n x 4V; a sum of at most V < 2^24 ones is exact
    return (v - np.rint(hot @ hot.T)).astype(np.int32)


def expected(chunks):
    """(counts, col, letters, dist) of the concatenation of the chunks, by the definitions"""
    n = chunks[0].shape[0]
    m = np.concatenate([np.asarray(c) for c in chunks], axis=1) if chunks else np.zeros((n, 0), np.uint8)
    cl = classes(m)
    col = np.flatnonzero(cl == SNP).astype(np.int64)
    letters = np.ascontiguousarray(upper(m)[:, col])
    counts = dict(columns=int(m.shape[1]), core_invariant=int((cl == INV).sum()), core_snps=int(len(col)), other=int((cl == OTHER).sum()))
    return counts, col, letters, distances(letters)


# ---------------------------------------------------------------------------------------------------------------- an XMFA
def scan_xmfa(path):
    """-> (names, letters [n, V] uint8, rows [(cluster, column, ref_pos)], dist [n, n] int32, counts) of the XMFA as it stands"""
    import xmfa_util
    head, recs = xmfa_util.records(path)
    names = [h[len("##SequenceFile "):] for h in head if h.startswith("##SequenceFile ")]
    n = len(names)
    parts, rows = [], []
    counts = dict(columns=0, core_invariant=0, core_snps=0, other=0)
    block = []
    for hdr, seq in recs:
        if hdr != "=":
            block.append((hdr, seq))
            continue
        if not block:
            continue
        m = np.zeros((n, len(block[0][1])), np.uint8)
        seen = set()
        ref_a = cluster = None
        for h, s in block:
            g = re.match(r"> (\d+):(\d+)-(\d+) ([+-]) cluster(\d+)", h)
            k = int(g.group(1)) - 1
            assert k not in seen and len(s) == m.shape[1], h
            seen.add(k)
            m[k] = np.frombuffer(s.encode(), np.uint8)
            if k == 0:
                ref_a, cluster = int(g.group(2)), int(g.group(5))
        assert len(seen) == n, "an LCB without a record of every sequence"
        cl = classes(m)
        counts["columns"] += m.shape[1]
        counts["core_invariant"] += int((cl == INV).sum()); counts["core_snps"] += int((cl == SNP).sum()); counts["other"] += int((cl == OTHER).sum())
        at = np.flatnonzero(cl == SNP)
        left = np.concatenate([[0], np.cumsum(m[0] != ord("-"))])      # left[c]: characters other than '-' of the reference row before column c
        parts.append(upper(m)[:, at])
        rows += [(cluster, int(c), int(ref_a + left[c])) for c in at]
        block = []
    letters = np.ascontiguousarray(np.concatenate(parts, axis=1)) if parts else np.zeros((n, 0), np.uint8)
    return names, letters, rows, distances(letters), counts


# ---------------------------------------------------------------------------------------------------------------- designed matrices
KINDS = ("inv", "inv_case", "snp_row0", "snp_last", "snp_row63", "snp_row64", "snp4", "snp_rand", "other_dash", "other_n", "other_u", "other_0")
KIND_CLASS = dict(inv=INV, inv_case=INV, snp_row0=SNP, snp_last=SNP, snp_row63=SNP, snp_row64=SNP, snp4=SNP, snp_rand=SNP, other_dash=OTHER, other_n=OTHER,
                  other_u=OTHER, other_0=OTHER)


def column(kind, n, rng):
    """one column of n rows of the kind; its class is KIND_CLASS[kind]"""
    a, b = rng.choice(4, 2, replace=False)
    col = np.full(n, _ACGT[a], np.uint8)
    if kind == "inv_case":                       # lower against upper case of one letter
        col[rng.random(n) < 0.5] += 32
        col[0], col[-1] = _ACGT[a], _ACGT[a] + 32
    elif kind == "snp_row0":
        col[0] = _ACGT[b]
    elif kind == "snp_last":
        col[-1] = _ACGT[b]
    elif kind in ("snp_row63", "snp_row64"):     # (the last row where the matrix has no such row)
        col[min(int(kind[7:]), n - 1)] = _ACGT[b]
    elif kind == "snp4":                         # all four letters (two where there are fewer than four rows)
        col[:] = _ACGT[rng.integers(0, 4, n)]
        if n >= 4:
            col[rng.choice(n, 4, replace=False)] = _ACGT
        else:
            col[rng.choice(n, 2, replace=False)] = _ACGT[[a, b]]
        col[rng.random(n) < 0.3] += 32
    elif kind == "snp_rand":
        col[:] = _ACGT[[a, b]][rng.integers(0, 2, n)]
        col[rng.choice(n, 2, replace=False)] = _ACGT[[a, b]]
    elif kind == "other_dash":                   # a '-' in one row beside two letters
        col[0] = _ACGT[b]
        col[1 + int(rng.integers(0, n - 1))] = ord("-")
    elif kind == "other_n":                      # an N as the only deviation
        col[int(rng.integers(0, n))] = ord("N") if rng.random() < 0.5 else ord("n")
    elif kind == "other_u":
        col[int(rng.integers(0, n))] = ord("U")
    elif kind == "other_0":
        col[int(rng.integers(0, n))] = 0
    else:
        assert kind == "inv"
    return col


def matrix(kinds, n, rng):
    m = np.stack([column(k, n, rng) for k in kinds], axis=1) if len(kinds) else np.zeros((n, 0), np.uint8)
    return m, np.array([KIND_CLASS[k] for k in kinds], np.int64)


def mixed(w, n, rng, snps=None):
    """w kinds; snps: exactly that many core SNP columns, at random places"""
    if snps is None:
        return [KINDS[i] for i in rng.integers(0, len(KINDS), w)]
    snp_kinds = [k for k in KINDS if KIND_CLASS[k] == SNP]
    rest = [k for k in KINDS if KIND_CLASS[k] != SNP]
    kinds = [rest[i] for i in rng.integers(0, len(rest), w)]
    for c in rng.choice(w, snps, replace=False):
        kinds[c] = snp_kinds[int(rng.integers(0, len(snp_kinds)))]
    return kinds


def placed(m, pitch_extra, rng):
    """the matrix as a view that starts at an address that is no multiple of 4, its rows pitch_extra bytes further apart than wide,
    '-' between them (a read past a row's end turns columns into `other`)"""
    n, w = m.shape
    pitch = w + pitch_extra
    buf = np.full(n * pitch + 16, ord("-"), np.uint8)
    off = 1 + (-(buf.ctypes.data + 1) % 4 == 0)      # 1, or 2 where buf + 1 is a multiple of 4
    view = buf[off: off + n * pitch].reshape(n, pitch)[:, :w]
    view[:] = m
    assert w == 0 or view.ctypes.data % 4 != 0
    return view


class Case:
    def __init__(self, name, chunks, designed):
        self.name, self.chunks, self.designed = name, chunks, designed      # designed: class of every column, by construction
        self.n = chunks[0].shape[0]


ADD_WIDTHS = (1, 63, 64, 65, 130, 0, 7)
ADD_SNPS = (1, 62, 1, 1, 100, 0, 3)      # core SNPs before each add: 0, 1, 63, 64, 65, 165, 165


def matrix_cases(seed=1):
    """name -> Case.  Rows at the lane and tile edges; widths and pitches of one add; core SNP counts at the word edges; single columns
    of every kind; several adds that share a plane word in every way; distances of identical and opposite rows"""
    rng = np.random.default_rng(seed)
    cases = {}

    def add(name, mats, extra=0):
        chunks = [placed(m, extra, rng) for m, _ in mats]
        cases[name] = Case(name, chunks, np.concatenate([d for _, d in mats]) if mats else np.zeros(0, np.int64))

    for n in (2, 3, 63, 64, 65, 129):
        add("rows%d" % n, [matrix(list(KINDS) + mixed(150, n, rng), n, rng)])
    # the row limit: a few hundred core SNPs, so that every tile of the pair grid (the last, partial word included) computes
    add("rows2048", [matrix(mixed(400, 2048, rng, snps=300), 2048, rng)])
    for w in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
        for extra in (0, 7):
            add("width%d_pitch%d" % (w, w + extra), [matrix(mixed(w, 5, rng), 5, rng)], extra)
    for k in (0, 1, 63, 64, 65):
        add("snps%d" % k, [matrix(mixed(130, 5, rng, snps=k), 5, rng)])
    add("snps0_all_other", [matrix([k for k in KINDS if KIND_CLASS[k] == OTHER] * 20, 5, rng)])
    add("snps0_all_invariant", [matrix(["inv", "inv_case"] * 40, 5, rng)])
    add("snps_all", [matrix(mixed(130, 5, rng, snps=130), 5, rng)])
    add("snps_last_only", [matrix(["inv"] * 99 + ["snp_rand"], 5, rng)])
    add("snps128", [matrix(mixed(300, 7, rng, snps=128), 7, rng)])      # V a multiple of 64, and one more: the mask of the last word
    add("snps129", [matrix(mixed(300, 7, rng, snps=129), 7, rng)])
    add("snps513", [matrix(mixed(700, 33, rng, snps=513), 33, rng)])    # nine plane words: a second slab of SnpDist's words, one word in it
    for kind in KINDS:
        add("single_" + kind, [matrix([kind], 66, rng)])
    add("adds", [matrix(mixed(w, 9, rng, snps=k), 9, rng) for w, k in zip(ADD_WIDTHS, ADD_SNPS)], 3)
    # rows 0 and 1 identical, rows 2 and 3 different in every core SNP column
    m, d = matrix(mixed(200, 6, rng, snps=70), 6, rng)
    m[1] = m[0]
    comp = {65: 67, 67: 65, 71: 84, 84: 71}
    at = np.flatnonzero(classes(m) == SNP)
    m[3, at] = [comp[int(x)] for x in upper(m[2:3, at])[0]]
    cases["pairs"] = Case("pairs", [placed(m, 0, rng)], classes(m))
    return cases
