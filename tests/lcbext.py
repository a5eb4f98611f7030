"""A numpy restatement of the LCB extension: the pair table line by line (the left moves of a line as a prefix
maximum -- the device walks anti-diagonals), the cut, the paths, the columns, the jobs from an XMFA plus the genomes, and the text of
.xmfa.extended.  `table_slow` states the table cell by cell, as 1e writes it; `table` is checked against it.  Everything is integers
and bytes.  Then seeded designs for the tests."""
import functools
import re

import numpy as np

MAX_ROWS, MAX_FLANK, MAX_BAND = 2048, 512, 63
DEFAULTS = dict(match=5, mismatch=4, gap=2, band=50, ani=95, min_len=10, max_flank=256)
UNDEF = int(np.iinfo(np.int32).min)
_NEG = -10 ** 9
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
ACGT = frozenset(b"ACGTacgt")


def params(**kw):
    return dict(DEFAULTS, **kw)


def key_of(p):
    return tuple(p[k] for k in ("match", "mismatch", "gap", "band", "ani", "min_len", "max_flank"))


def _sub(x, y, p):
    return p["match"] if x == y and x in b"ACGT" else -p["mismatch"]


# ------------------------------------------------------------------------------------------------------- the pair table
def table_slow(a, b, p):
    """H as a dict over the cells that exist, literally as 1e defines it"""
    W, G = p["band"], p["gap"]
    H = {}
    for i in range(len(a) + 1):
        for j in range(len(b) + 1):
            if abs(i - j) > W:
                continue
            if i == 0 and j == 0:
                H[0, 0] = 0
                continue
            c = []
            if (i - 1, j - 1) in H:
                c.append(H[i - 1, j - 1] + _sub(a[i - 1], b[j - 1], p))
            if (i - 1, j) in H:
                c.append(H[i - 1, j] - G)
            if (i, j - 1) in H:
                c.append(H[i, j - 1] - G)
            H[i, j] = max(c)
    return H


def table(a, b, p):
    """H as int64 [La + 1, Lb + 1], _NEG-ish where the cell does not exist; use exists()"""
    a, b = a.upper(), b.upper()
    W, G, M, X = p["band"], p["gap"], p["match"], p["mismatch"]
    La, Lb = len(a), len(b)
    H = np.full((La + 1, Lb + 1), _NEG, np.int64)
    bb = np.frombuffer(b, np.uint8)
    ok = np.isin(bb, np.frombuffer(b"ACGT", np.uint8))
    for i in range(La + 1):
        lo, hi = max(0, i - W), min(Lb, i + W)
        if lo > hi:
            break
        j = np.arange(lo, hi + 1)
        T = np.full(len(j), _NEG, np.int64)
        if i == 0:
            T[0] = 0
        else:
            up = H[i - 1, lo:hi + 1] - G
            d0 = max(lo, 1)
            sub = np.where((bb[d0 - 1:hi] == a[i - 1]) & ok[d0 - 1:hi], M, -X)
            diag = np.full(len(j), _NEG, np.int64)
            diag[d0 - lo:] = H[i - 1, d0 - 1:hi] + sub
            T = np.maximum(up, diag)
        H[i, lo:hi + 1] = np.maximum.accumulate(T + G * j) - G * j
    return H


def exists(H, p):
    i, j = np.indices(H.shape)
    return np.abs(i - j) <= p["band"]


def best_of(H, p, width=None):
    """best(i) for i = 0 ... La, UNDEF where no cell of the line exists; padded with UNDEF to `width` entries"""
    ex = exists(H, p)
    out = np.full(max(width or 0, H.shape[0]), UNDEF, np.int64)
    for i in range(H.shape[0]):
        if ex[i].any():
            out[i] = H[i][ex[i]].max()
    return out


def passes(i, best, p):
    return best != UNDEF and 100 * int(best) >= i * (p["ani"] * p["match"] - (100 - p["ani"]) * p["mismatch"])


def cut(bests, La, p):
    """the reach of a job from the best() of its rows (row 0: i M)"""
    A = 0
    for i in range(1, La + 1):
        if all(passes(i, b[i], p) for b in bests):
            A = i
    return A if A >= p["min_len"] else 0


def path(H, a, b, A, p):
    """(j_r, ins [A + 1], has [A]) of the path that ends on line A"""
    a, b = a.upper(), b.upper()
    W, G = p["band"], p["gap"]
    line = [(j, int(H[A, j])) for j in range(H.shape[1]) if abs(A - j) <= W]
    top = max(v for _, v in line)
    jr = min(j for j, v in line if v == top)
    ins, has = np.zeros(A + 1, np.int64), np.zeros(A, np.int64)
    i, j = A, jr
    while (i, j) != (0, 0):
        h = int(H[i, j])
        if i > 0 and j > 0 and h == int(H[i - 1, j - 1]) + _sub(a[i - 1], b[j - 1], p):
            i, j = i - 1, j - 1
            has[i] = 1
        elif i > 0 and abs(i - 1 - j) <= W and h == int(H[i - 1, j]) - G:
            i -= 1
        else:
            assert j > 0 and abs(i - (j - 1)) <= W and h == int(H[i, j - 1]) - G
            j -= 1
            ins[i] += 1
    return jr, ins, has


def columns(paths, flanks, A):
    """the rows of a job as bytes of one length C, in the flank's own order"""
    w = np.max([ins for _, ins, _ in paths], axis=0)
    rows = []
    for (jr, ins, has), b in zip(paths, flanks):
        b, out, at = b.upper(), bytearray(), 0
        for k in range(A + 1):
            out += b[at:at + ins[k]] + b"-" * int(w[k] - ins[k])
            at += int(ins[k])
            if k < A:
                out += b[at:at + 1] if has[k] else b"-"
                at += int(has[k])
        assert at == jr
        rows.append(bytes(out))
    assert len({len(r) for r in rows}) == 1 and len(rows[0]) == A + int(w.sum())
    return rows


@functools.lru_cache(maxsize=None)
def _pair(a, b, pk):
    p = dict(zip(("match", "mismatch", "gap", "band", "ani", "min_len", "max_flank"), pk))
    H = table(a, b, p)
    return H, best_of(H, p, p["max_flank"] + 1)


def job(flanks, p):
    """a job from its rows' flanks (bytes, the reference's first) -> dict(reach, cols, used, rows, best): cols 0 with reach 0, -1 when
    too wide (rows None in both cases)"""
    pk = key_of(p)
    a = flanks[0]
    pairs = [_pair(a, b, pk) for b in flanks]
    bests = [bst for _, bst in pairs]
    A = cut(bests, len(a), p)
    out = dict(reach=A, cols=0, width=0, used=[0] * len(flanks), rows=None, best=bests, ins=None)
    if A:
        paths = [path(H, a, b, A, p) for (H, _), b in zip(pairs, flanks)]
        out["used"] = [jr for jr, _, _ in paths]
        C = A + int(np.max([ins for _, ins, _ in paths], axis=0).sum())
        out["width"], out["ins"] = C, [ins for _, ins, _ in paths]
        out["cols"] = -1 if C > 2 * p["max_flank"] else C
        if out["cols"] > 0:
            out["rows"] = columns(paths, flanks, A)
    return out


# ------------------------------------------------------------------------------------------------------- jobs from an XMFA
def read_xmfa(path):
    """(header lines, [[(seq, lo, hi, strand, cluster) per record] per LCB])"""
    head, lcbs, cur = [], [], []
    for line in open(path):
        line = line.rstrip("\n")
        if line.startswith("#"):
            head.append(line)
        elif line.startswith(">"):
            m = re.match(r"> (\d+):(\d+)-(\d+) ([+-]) cluster(\d+) ", line)
            cur.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4), int(m.group(5))))
        elif line == "=":
            lcbs.append(cur)
            cur = []
    return head, lcbs


def covered_of(lcbs, genomes):
    cov = [np.zeros(len(g), bool) for g in genomes]
    for recs in lcbs:
        for seq, lo, hi, _, _ in recs:
            cov[seq - 1][max(lo - 1, 0):max(hi, 0)] = True
    return cov


def flank_of(genome, cov, lo, hi, strand, side, F):
    """(first, step, complement, letters): the flank of a record on a side, read away from the LCB as the XMFA prints the row"""
    up = (side == "R") == (strand == "+")
    first, step = (hi, 1) if up else (lo - 2, -1)
    comp = int(strand == "-")
    n = 0
    if 0 <= first < len(genome) and not cov[first]:
        q = first
        while 0 <= q < len(genome) and not cov[q]:
            q += step
        run = abs(q - first)
        touches = 0 <= q < len(genome)
        avail = run if not touches else (run + 1) // 2 if step == 1 else run // 2
        while n < min(avail, F) and genome[first + n * step] in ACGT:
            n += 1
    letters = bytes(genome[first + k * step] for k in range(n)).upper()
    return first, step, comp, letters.translate(_COMP) if comp else letters


def jobs_of(lcbs, genomes, p):
    """[(cluster, side, [record], [(first, step, complement, letters)])] in the file's order, L before R"""
    cov = covered_of(lcbs, genomes)
    out = []
    for recs in lcbs:
        for side in "LR":
            out.append((recs[0][4], side, recs, [flank_of(genomes[s - 1], cov[s - 1], lo, hi, st, side, p["max_flank"]) for s, lo, hi, st, _ in recs]))
    return out


def extended_text(xmfa_path, genomes, p):
    """-> (the text of .xmfa.extended, counts): genomes as the run held them (bytes, contigs joined as the run joins them)"""
    head, lcbs = read_xmfa(xmfa_path)
    text = "".join(h + "\n" for h in head)
    counts = dict(ext_jobs=0, ext_kept=0, ext_wide=0, ext_bases=0)
    for cluster, side, recs, flanks in jobs_of(lcbs, genomes, p):
        counts["ext_jobs"] += 1
        res = job([f[3] for f in flanks], p)
        if res["cols"] < 0:
            counts["ext_wide"] += 1
        if res["cols"] <= 0:
            continue
        counts["ext_kept"] += 1
        counts["ext_bases"] += res["reach"]
        for (seq, _, _, strand, _), (first, step, _, _), used, row in zip(recs, flanks, res["used"], res["rows"]):
            ends = sorted((first, first + (used - 1) * step))
            lo, hi = (ends[0] + 1, ends[1] + 1) if used else (0, 0)
            row = row[::-1] if side == "L" else row
            text += "> %d:%d-%d %s cluster%d %s\n" % (seq, lo, hi, strand, cluster, side)
            text += "".join(row[k:k + 80].decode() + "\n" for k in range(0, len(row), 80))
        text += "=\n"
    return text, counts


# ------------------------------------------------------------------------------------------------------- designs
def rand_seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def mutate(rng, s, subs=0, dels=(), inss=()):
    """s with `subs` substitutions at random places, deletions (at, len) and insertions (at, len), places in s's coordinates"""
    s = bytearray(s)
    for at in rng.choice(len(s), subs, replace=False) if subs else []:
        s[at] = b"ACGT"[(b"ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4]
    edits = sorted([(at, -n) for at, n in dels] + [(at, n) for at, n in inss], reverse=True)
    for at, n in edits:
        if n < 0:
            del s[at:at - n]
        else:
            s[at:at] = rand_seq(rng, n)
    return bytes(s)


class Pool:
    """genomes made of the designs' strings, and the descriptors that read them back: every string is laid down forward, reversed,
    complemented or both, so that step and complement are exercised; strings are spread over `n_genomes` genomes"""

    def __init__(self, n_genomes=3, seed=1):
        self.rng = np.random.default_rng(seed)
        self.parts = [[b"ACGTTGCA"] for _ in range(n_genomes)]
        self.at = [8] * n_genomes
        self.memo = {}
        self.count = 0

    def row(self, s, mode=None):
        """the descriptor (genome, step, complement, len, first) of string s"""
        mode = self.count % 4 if mode is None else mode
        self.count += 1
        if (s, mode) not in self.memo:
            g = self.count % len(self.parts)
            rev, comp = mode & 1, mode >> 1
            t = s.translate(_COMP) if comp else s
            t = t[::-1] if rev else t
            first = self.at[g] + (len(s) - 1 if rev else 0)
            self.parts[g] += [t, b"N"]
            self.at[g] += len(s) + 1
            self.memo[s, mode] = (g, -1 if rev else 1, comp, len(s), first if s else 0)
        return self.memo[s, mode]

    def genomes(self):
        return [b"".join(p) for p in self.parts]


def read_row(genomes, row):
    g, step, comp, n, first = row
    s = bytes(genomes[g][first + k * step] for k in range(n))
    return s.translate(_COMP) if comp else s


def noisy(rng, s, a, b, every=8):
    """s with one substitution in every `every` bases of [a, b), at a place of the genome's own: no long exact match survives there,
    the identity stays near 1 - 1 / every"""
    s = bytearray(s)
    for k in range(a, b, every):
        at = k + int(rng.integers(0, every))
        if at < b:
            s[at] = b"ACGT"[(b"ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(s)


def file_design(seed=4, n=6, size=24000):
    """a small single-contig set whose LCBs break where the test wants them: sparse substitutions everywhere; a head of 200 noisy
    bases (the first LCB's left flank runs to position 0); 400 noisy bases at 6000 (two LCBs closer than 2 F: the halving); 1000
    noisy bases at 12000 with an N run inside the flank of genome 2; an inversion of [16000, 19000) in genome 3 (reverse rows)"""
    rng = np.random.default_rng(seed)
    ref = rand_seq(rng, size)
    out = [ref]
    for g in range(1, n):
        s = bytearray(ref)
        for at in rng.choice(size, size // 150, replace=False):
            s[at] = b"ACGT"[(b"ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4]
        s = bytes(s)
        for a, b in ((0, 200), (6000, 6400), (12000, 13000)):
            s = noisy(rng, s, a, b)
        if g == 2:
            s = s[:12100] + b"N" * 12 + s[12112:]
        if g == 3:
            s = s[:16000] + s[16000:19000].translate(_COMP)[::-1] + s[19000:]
        out.append(s)
    return out
