"""Call-level checks of the resident route (include/parsnp_mum.h: pm_store_*): a ctypes driver over a `binding.Lib`, a sequential
restatement of every call, and a seeded generator of small sets that take the paths where the kernels can go wrong.

Plain Python and numpy, no engine code.  The restatement reads only what the host could know -- the sequences, the raw rows the
anchor call left in the store, their lengths and the PM_ROW_* bits -- and works on one bool array per genome (the reference's
mumlayout), base by base, the way src/parsnp.cpp does: setMums1's second half (:1781-1841) with Aligner::trim (:1399-1477),
determineRegion (:1199-1290) with setInitialClusters' test (:2150-2172), the pairwise test of setFinalClusters (:2596-2700),
filterRandomClustersSimple1 (:433-497) and setInterClusterRegions (:2389-2460)."""
import ctypes as C

import numpy as np

from parsnp_amd.binding import Session

PM_OK, PM_EAGAIN = 0, -6
ROW_BAD, ROW_OUTSIDE, ROW_REVERSE, ROW_DIRTY, ROW_EARLY = 1, 2, 4, 8, 16
ST_BUILT, ST_OK, ST_FLAGGED, ST_TANGLED, ST_ACCEPTED = 1, 2, 4, 8, 16
MINSIZE = 16      # minimum MUM length of the anchor call (no chance match of that length in sets of this size)

ROW_INFO = np.dtype([("start0", "<i4"), ("len", "<i4"), ("shift", "<i4"), ("state_flags", "<u4")])
REGION_INFO = np.dtype([("key", "<i8"), ("ref_start", "<i8"), ("ref_len", "<i8"), ("slength", "<i4"), ("parent", "<i4")])
CHAIN_FIELDS = ("n_in", "lcbs_first", "lcbs_dissolved", "mums_dissolved", "n_mums", "n_lcbs", "n_fillers", "trouble")


# ---------------------------------------------------------------------------------------------------------------- driver
def declare(L):
    """argument and result types of the entry points the driver calls"""
    v, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    P = C.POINTER
    sig = {
        "pm_session_rows": (C.c_int, [v, C.c_int]),
        "pm_session_tune": (C.c_int, [v, C.c_char_p, i64]),
        "pm_result_table_id": (i64, [v]),
        "pm_result_store_base": (i64, [v]),
        "pm_result_lon": (P(i32), [v]),
        "pm_result_flags": (P(C.c_uint32), [v]),
        "pm_result_total": (i64, [v]),
        "pm_store_settle": (C.c_int, [v, i64, v]),
        "pm_store_settle_seeds": (C.c_int, [v, i64, i32, v, P(i64)]),
        "pm_store_seeds": (C.c_int, [v, i64, v, i64, i32, P(i64)]),
        "pm_store_new_regions": (v, [v]),
        "pm_store_new_region_ids": (P(i32), [v]),
        "pm_store_regions_equal": (C.c_int, [v, v, v, i64, v]),
        "pm_store_info": (C.c_int, [v, i64, i64, v]),
        "pm_store_rows": (C.c_int, [v, v, i64, i64, C.c_int, v, v]),
        "pm_store_layout_words": (i64, [v, v]),
        "pm_store_layout": (C.c_int, [v, v, i64]),
        "pm_store_judge": (C.c_int, [v, v, v, i64, i32, v, v, v]),
        "pm_store_unmark": (C.c_int, [v, v, i64]),
        "pm_store_fill": (C.c_int, [v, v, v, i64, v]),
        "pm_store_fill_starts": (P(i64), [v]),
        "pm_store_fill_ends": (P(i64), [v]),
        "pm_store_chain_begin": (C.c_int, [v, i64, i32, C.c_float, i64]),
        "pm_store_chain_end": (C.c_int, [v, v, P(P(i32)), P(P(C.c_uint8))]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _i32(x):
    return np.ascontiguousarray(x, np.int32)


class Store:
    """One session in resident mode after its anchor call: the candidate list of ONE whole-genome region is the anchor table
    (rows [0, A) of the MUM store).  The pm_result stays alive until close(), as resident.cpp keeps it in kept_results_."""

    def __init__(self, lib, seqs, tune=None, minsize=MINSIZE):
        self.lib, self.L = lib, lib.L
        declare(self.L)
        self.sess = Session(lib, seqs)
        self.h = self.sess.h
        self.n = len(seqs)
        self.glen = np.array([len(s) for s in seqs], np.int64)
        self.res = C.c_void_p()
        try:
            knobs = {"dirty_min": 8}      # a small list becomes the anchor table
            knobs.update(tune or {})
            for k, val in knobs.items():
                self.check(self.L.pm_session_tune(self.h, k.encode(), val))
            self.check(self.L.pm_session_rows(self.h, 2))
            starts = np.zeros(self.n, np.int64)
            lens = self.glen.copy()
            mins = np.array([minsize], np.int32)
            p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
            self.check(self.L.pm_multi_mum_batch(self.h, 1, p(starts, C.c_int64), p(lens, C.c_int64), p(mins, C.c_int32), C.byref(self.res)))
            self.table = self.L.pm_result_table_id(self.res)
            assert self.table != 0 and self.L.pm_result_store_base(self.res) == 0, "the anchor call left no anchor table in the store"
            self.A = A = int(self.L.pm_result_total(self.res))
            self.lon = np.ctypeslib.as_array(self.L.pm_result_lon(self.res), (A,)).copy()
            self.flags = np.ctypeslib.as_array(self.L.pm_result_flags(self.res), (A,)).copy()
            self.raw_start, self.strand = self.rows(None, 0, A, raw=True)
        except BaseException:
            self.close()
            raise

    def check(self, rc):
        self.lib._check(rc)

    def close(self):
        if self.res:
            self.L.pm_result_free(self.res)
            self.res = C.c_void_p()
        self.sess.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def settle(self):
        """-> (return code, pm_row_info per row of the table)"""
        info = np.zeros(self.A, ROW_INFO)
        rc = self.L.pm_store_settle(self.h, self.table, _ptr(info))
        if rc != PM_EAGAIN:
            self.check(rc)
        return rc, info

    def _regions(self, n):
        regs = np.zeros(n, REGION_INFO)
        if n:
            C.memmove(_ptr(regs), self.L.pm_store_new_regions(self.h), n * REGION_INFO.itemsize)
        ids = np.ctypeslib.as_array(self.L.pm_store_new_region_ids(self.h), (n,)).copy() if n else np.zeros(0, np.int32)
        return regs, ids

    def settle_seeds(self, q):
        info = np.zeros(self.A, ROW_INFO)
        nreg = C.c_int64()
        self.check(self.L.pm_store_settle_seeds(self.h, self.table, q, _ptr(info), C.byref(nreg)))
        return (info,) + self._regions(nreg.value)

    def seeds(self, anchors, q):
        anchors = _i32(anchors)
        nreg = C.c_int64()
        self.check(self.L.pm_store_seeds(self.h, self.table, _ptr(anchors), len(anchors), q, C.byref(nreg)))
        return self._regions(nreg.value)

    def regions_equal(self, a, b):
        a, b = _i32(a), _i32(b)
        same = np.full(len(a), 7, np.uint8)
        self.check(self.L.pm_store_regions_equal(self.h, _ptr(a), _ptr(b), len(a), _ptr(same)))
        return same

    def info(self, first, count):
        info = np.zeros(count, ROW_INFO)
        self.check(self.L.pm_store_info(self.h, first, count, _ptr(info)))
        return info

    def rows(self, rows, first, n, raw):
        """-> (start[n, genomes], strand[n, genomes]); rows None: store rows [first, first + n)"""
        if rows is not None:
            rows = _i32(rows)
            n = len(rows)
        start = np.zeros((n, self.n), np.int32)
        strand = np.zeros((n, self.n), np.uint8)
        self.check(self.L.pm_store_rows(self.h, _ptr(rows) if rows is not None else None, first, n, 1 if raw else 0, _ptr(start), _ptr(strand)))
        return start, strand

    def layout(self):
        """-> one bool array of glen[j] + 1 entries per genome (the last one the sentinel)"""
        off = np.zeros(self.n + 1, np.int64)
        words = int(self.L.pm_store_layout_words(self.h, _ptr(off)))
        img = np.zeros(words, np.uint64)
        self.check(self.L.pm_store_layout(self.h, _ptr(img), words))
        out = []
        for j in range(self.n):
            bits = np.unpackbits(img[off[j]:off[j + 1]].view(np.uint8), bitorder="little")
            assert not bits[self.glen[j] + 1:].any(), "marks past the sentinel of genome %d" % j
            out.append(bits[:self.glen[j] + 1].astype(bool))
        return out

    def judge(self, cur, back, d):
        cur, back = _i32(cur), _i32(back)
        m = len(cur)
        mn, mx, v = np.zeros(m, np.int32), np.zeros(m, np.int32), np.full(m, 9, np.uint8)
        self.check(self.L.pm_store_judge(self.h, _ptr(cur), _ptr(back), m, d, _ptr(mn), _ptr(mx), _ptr(v)))
        return mn, mx, v

    def unmark(self, rows):
        rows = _i32(rows)
        self.check(self.L.pm_store_unmark(self.h, _ptr(rows), len(rows)))

    def fill(self, last_of, first_of_next):
        """-> (add per pair, starts[m, genomes], ends[m, genomes] of the m pairs with add == 1, one after the other)"""
        a, b = _i32(last_of), _i32(first_of_next)
        add = np.full(len(a), 9, np.uint8)
        self.check(self.L.pm_store_fill(self.h, _ptr(a), _ptr(b), len(a), _ptr(add)))
        m = int((add == 1).sum())
        if not m:
            return add, np.zeros((0, self.n), np.int64), np.zeros((0, self.n), np.int64)
        fs = np.ctypeslib.as_array(self.L.pm_store_fill_starts(self.h), (m * self.n,)).copy().reshape(m, self.n)
        fe = np.ctypeslib.as_array(self.L.pm_store_fill_ends(self.h), (m * self.n,)).copy().reshape(m, self.n)
        return add, fs, fe

    def chain(self, n_expected, d, diag_diff, c):
        """pm_store_chain_begin + _end -> (pm_chain_info as a dict, rows, heads)"""
        self.check(self.L.pm_store_chain_begin(self.h, n_expected, d, C.c_float(diag_diff), c))
        info = np.zeros(8, np.int64)
        rows, heads = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint8)()
        self.check(self.L.pm_store_chain_end(self.h, _ptr(info), C.byref(rows), C.byref(heads)))
        out = dict(zip(CHAIN_FIELDS, (int(x) for x in info)))
        m = out["n_mums"]
        return out, np.ctypeslib.as_array(rows, (m,)).copy() if m else np.zeros(0, np.int32), np.ctypeslib.as_array(heads, (m,)).copy() if m else np.zeros(0, np.uint8)


# ---------------------------------------------------------------------------------------------------------------- restatement
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s):
    return s.translate(_COMP)[::-1]


class Model:
    """The store as the reference would hold it: the rows in list order, what setMums1 made of each, and the layout."""

    def __init__(self, seqs, raw_start, strand, lon, flags):
        self.seqs = seqs
        self.n = len(seqs)
        self.glen = [len(s) for s in seqs]
        self.start = np.asarray(raw_start, np.int64)
        self.strand = np.asarray(strand)
        self.lon = [int(x) for x in lon]
        self.flags = [int(x) for x in flags]
        self.A = len(self.lon)
        self.marks = [np.zeros(g + 1, bool) for g in self.glen]      # (the entry at glen stays unset here: layout() adds the sentinel)
        self.accepted = [False] * self.A
        self.shift = [0] * self.A
        self.len = list(self.lon)
        self.crossings = [0, 0]      # trims at the start / at the end of a row whose marked run crosses a 64-base word of the genome's layout

    # ------------------------------------------------------------------ settle
    def settle(self):
        return self.settle_rows(range(self.A))

    def settle_rows(self, rows):
        """setMums1's second half for the listed rows, in that order, against the marks as they are"""
        n = self.n
        for c in rows:
            f, ln, sh = self.flags[c], self.lon[c], 0
            if (f & (ROW_BAD | ROW_OUTSIDE)) or ln < 5:
                continue
            st = [int(x) for x in self.start[c]]
            for j in range(n):      # Aligner::trim: the marked run at the start moves the start in EVERY genome, the one at the end follows
                m, s = self.marks[j], st[j] + sh
                lft = 0
                while lft < ln and m[s + lft]:
                    lft += 1
                rgt = 0
                while rgt < ln - lft and m[s + ln - 1 - rgt]:
                    rgt += 1
                self.crossings[0] += lft > 0 and (s >> 6) != ((s + lft - 1) >> 6)
                self.crossings[1] += rgt > 0 and ((s + ln - 1) >> 6) != ((s + ln - rgt) >> 6)
                sh += lft
                ln -= lft + rgt
            self.shift[c], self.len[c] = sh, ln
            if ln < 2 or n <= 1 or not self.strand[c, 0]:
                continue
            ref = self.seqs[0][st[0] + sh: st[0] + sh + ln]
            if any(not self.strand[c, j] and revcomp(self.seqs[j][st[j] + sh: st[j] + sh + ln]) != ref for j in range(n)):
                continue
            self.accepted[c] = True
            for j in range(n):
                self.marks[j][st[j] + sh: st[j] + sh + ln] = True
        return self

    def acc_rows(self):
        return [c for c in range(self.A) if self.accepted[c]]

    def pos(self, c, j):
        """start of row c in genome j with the trim applied"""
        return int(self.start[c, j]) + self.shift[c]

    def layout(self, marks=None):
        out = []
        for m in (marks or self.marks):
            m = m.copy()
            m[-1] = True
            out.append(m)
        return out

    # ------------------------------------------------------------------ seeds
    def region_side(self, c, side, j):
        """determineRegion for one genome: (start, end) of the request; its length is end - start (TRegion, LCR.cpp:29)"""
        m, s = self.marks[j], self.pos(c, j)
        if side == 0:
            cur = s
            while True:
                cur -= 1
                if cur < 0:
                    cur = 0
                    break
                if m[cur]:
                    break
            return cur + 1, s - 1
        end = s + self.len[c]
        cur = end
        while True:
            cur += 1
            if cur >= self.glen[j] or m[cur]:
                break
        return end + 1, cur - 1

    def seeds(self, q):
        """-> list of (pm_region_info fields as a dict, rows [(start, length)] per genome), in push order"""
        out = []
        for i, c in enumerate(self.acc_rows()):
            for side in (0, 1):
                rows = []
                for j in range(self.n):
                    a, b = self.region_side(c, side, j)
                    rows.append((a, b - a))
                sl = min(ln for _, ln in rows)
                if sl > q:
                    out.append((dict(key=2 * i + side, ref_start=rows[0][0], ref_len=rows[0][1], slength=sl, parent=c), rows))
        return out

    # ------------------------------------------------------------------ judge
    def gaps(self, a, b):
        """per genome: start of row a minus the end of row b"""
        return [self.pos(a, j) - (self.pos(b, j) + self.len[b]) for j in range(self.n)]

    def judge(self, a, b, d):
        """-> (verdict, min gap, max gap); a reverse pair has no gaps to report"""
        if (self.flags[a] | self.flags[b]) & ROW_REVERSE:
            return 2, None, None
        g = self.gaps(a, b)
        return (1 if any(x < 0 or x > d for x in g) else 0), min(g), max(g)

    # ------------------------------------------------------------------ fill
    def fill(self, ct, nx, lay, genomes=None):
        """setInterClusterRegions for the pair (last MUM ct of an LCB, first MUM nx of the next) on the layout `lay` (with its
        sentinels) -> (add, starts, ends); genomes: as if the set held only these (which genome decides a pair?)"""
        genomes = range(self.n) if genomes is None else genomes
        start, end, flag = [], [], False
        for j in genomes:
            e = self.pos(ct, j) + self.len[ct]
            if self.pos(nx, j) - e <= 0:
                return 0, None, None
            stop = self.glen[j]
            start.append(e)
            for m in range(e + 1, stop + 1):      # (`flag` keeps its value where this loop has nothing to run over, :2419-2433)
                flag = bool(lay[j][m])
                if flag:
                    end.append(m - 1)
                    break
            if not flag:
                end.append(stop - 1)
        if len(end) != len(genomes):
            return 2, None, None
        end = [x + 1 for x in end]      # (the closing TMum has length 1)
        if any(b - a < 5 for a, b in zip(start, end)):
            return 0, None, None
        return 1, start, end

    # ------------------------------------------------------------------ chain
    def chain_verdict(self, a, b, d, diag_diff):
        """the test of setFinalClusters of MUM a against the open chain's last MUM b -> (joins, the ratio is exactly at the bar, it
        joins only because a smallest gap of 0 counts as 1)"""
        f32 = np.float32
        max_gap, min_gap = f32(0), f32(d + 10)
        if not ((self.flags[a] | self.flags[b]) & ROW_REVERSE):
            g = self.gaps(a, b)
            if any(x < 0 or x > d for x in g):
                return False, False, False
            for x in g:
                if f32(x) > max_gap:
                    max_gap = f32(x)
                if f32(x) < min_gap:
                    min_gap = f32(x)
        else:
            for k in range(self.n):      # :2604-2642, genome by genome
                ns, bs = self.pos(a, k), self.pos(b, k)
                fgap = ns - (bs + self.len[b])       # nt->start - cluster.end
                rgap = bs - (ns + self.len[a])       # cluster.mums.back().start - nt->end
                fw = bool(self.strand[a, k])
                if fw and f32(fgap) > max_gap:
                    max_gap = f32(fgap)
                elif not fw and f32(rgap) > max_gap:
                    max_gap = f32(fgap)      # (:2610 assigns the forward gap)
                if fw and f32(fgap) < min_gap:
                    min_gap = f32(fgap)
                elif not fw and f32(rgap) < min_gap:
                    min_gap = f32(rgap)
                if bool(self.strand[b, k]) != fw:
                    return False, False, False
                if fw and fgap < 0:
                    return False, False, False
                if not fw and fgap >= 0:
                    return False, False, False
                if fw and fgap > d:
                    return False, False, False
                if not fw and rgap > d:
                    return False, False, False
        zero = bool(min_gap == 0)
        if min_gap == 0:
            min_gap = f32(1)
        if max_gap == 0:
            max_gap = f32(1)
        ratio = np.float64(min_gap / max_gap)      # a float division, compared as a double (:2693)
        bar = 1.0 - np.float64(f32(diag_diff))
        return bool(ratio >= bar), bool(ratio == bar), zero and bool(ratio >= bar) and bar > 0

    def chain_pass(self, rows, d, diag_diff):
        """-> (head flag per MUM of the sorted list, [pairs that join with the ratio exactly at the bar, pairs that join only because
        a smallest gap of 0 counts as 1])"""
        heads, edge = [1], [0, 0]
        for x in range(1, len(rows)):
            joins, tie, zero = self.chain_verdict(rows[x], rows[x - 1], d, diag_diff)
            heads.append(0 if joins else 1)
            edge[0] += tie
            edge[1] += zero
        return heads, edge

    def lcb_lengths(self, rows, heads):
        out = []
        for x, c in enumerate(rows):
            if heads[x]:
                out.append(0)
            out[-1] += self.len[c]
        return out

    def sorted_rows(self):
        rows = sorted(self.acc_rows(), key=lambda c: self.pos(c, 0))
        tie = any(self.pos(a, 0) == self.pos(b, 0) for a, b in zip(rows, rows[1:]))
        return rows, tie

    def chain(self, d, diag_diff, c):
        """phases C-D -> (pm_chain_info as a dict, rows, heads, layout afterwards, the edge counts of chain_pass over both passes)"""
        rows, tie = self.sorted_rows()
        heads, edge = self.chain_pass(rows, d, diag_diff)
        lens = self.lcb_lengths(rows, heads)
        info = dict(n_in=len(rows), lcbs_first=len(lens), lcbs_dissolved=0, mums_dissolved=0, trouble=1 if tie else 0)
        marks = [m.copy() for m in self.marks]
        keep, lcb = [], -1
        for x, r in enumerate(rows):
            lcb += heads[x]
            if lcb != len(lens) - 1 and lens[lcb] <= c:      # (the last LCB is never examined, :447)
                info["mums_dissolved"] += 1
                info["lcbs_dissolved"] += heads[x]
                for j in range(self.n):
                    marks[j][self.pos(r, j): self.pos(r, j) + self.len[r]] = False
            else:
                keep.append(r)
        heads2, edge2 = self.chain_pass(keep, d, diag_diff)
        lay = self.layout(marks)
        fillers = 0
        for x in range(1, len(keep)):
            if heads2[x]:
                add = self.fill(keep[x - 1], keep[x], lay)[0]
                fillers += add == 1
                if add == 2:
                    info["trouble"] |= 2
        info.update(n_mums=len(keep), n_lcbs=sum(heads2), n_fillers=fillers)
        return info, keep, heads2, lay, [a + b for a, b in zip(edge, edge2)]


# ---------------------------------------------------------------------------------------------------------------- generator
def _repeat_units():
    """one unit of 2 to 4 bases (as codes 0..3 = ACGT) per class of primitive units under rotation and reverse complement: tandem
    arrays of two different classes share no match of MUM length on either strand, so every repeat of a set has a locus of its own"""
    seen, out = set(), []
    for u in (2, 3, 4):
        for x in range(4 ** u):
            s = tuple((x >> (2 * i)) & 3 for i in range(u))
            if any(u % p == 0 and s == s[:p] * (u // p) for p in range(1, u)):
                continue
            rc = tuple(3 - b for b in reversed(s))
            key = min(t[i:] + t[:i] for t in (s, rc) for i in range(u))
            if key not in seen:
                seen.add(key)
                out.append(s)
    return out


def make_set(seed, n, length, pairs, inversions=(), translocate=None):
    """n sequences of about `length` bases (sequence 0 = the reference) whose anchor list takes the paths of the resident route:

    * unique sequence interleaved with `pairs` pairs of short tandem repeats 20 to 30 bases apart whose copy number differs from
      the reference's by at most 2 in every genome: the MUMs on both sides of a repeat overlap where a genome has fewer copies
      (flagged rows, trims, gaps of exactly 0), and the MUM between the two repeats of a pair overlaps both (tangled rows); every
      other pair is followed by a repeat that stands alone (a flagged row that meets no other flagged row), with a unit of 2 or
      3 bases and one copy less or none: gaps of 0 and 2 or 3 bases, which join a chain only because the ratio test counts a
      smallest gap of 0 as 1.  Every repeat has a
      unit of its own (_repeat_units);
    * a substitution shared by all query genomes at reference position 64 k - 1, 64 k or 64 k + 1 for every k: MUM ends on both
      sides of a word boundary of the reference's layout; single substitutions at a rate of 1 / (120 (n - 1)) per genome and base;
    * planted sites -- a run of r substituted bases in all query genomes and an insertion of i bases behind it (i < 0: the last -i
      bases of the run deleted) in ONE of them, so that the two MUMs around it lie r bases apart in every genome but one and
      r + i there: (r, r + i) = (3, 10), (1, 2), (6, 14), (6, 4) -- the ratio test of the chaining at 0.3 and 0.5 exactly, gaps
      that take a filler (at least 5 bases in every genome) and gaps that one genome alone keeps from it.  That genome is the
      last one at every other site (past a 64-genome group where there are that many);
    * three insertions of 320 bases in the last genome: pairs of MUMs further apart than the reference's default d = 300;
    * the first and last 48 bases are the same in all genomes: MUMs that start at 0 and end at the genome's end;
    * inversions: (genome, from, to) as fractions of its length, reverse-complemented in place (PM_ROW_REVERSE rows); the
      insertion of a site goes to the LAST inverted genome at every other site;
    * translocate: (genome, from, to): that piece moves to the very start of the genome -- its first MUM in list order lies
      before everything earlier in that genome (PM_ROW_EARLY without PM_ROW_DIRTY: marks by atomics)."""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", np.uint8)
    ref = rng.integers(0, 4, length).astype(np.int8)
    prot = np.zeros(length, bool)
    prot[:48] = True
    prot[-48:] = True
    repeats = []      # (position, unit length, copies, stands alone)
    units = _repeat_units()
    units = [units[i] for i in rng.permutation(len(units))]
    assert 3 * pairs <= len(units)
    span = (length - 400) // pairs
    for p in range(pairs):
        at = 150 + p * span + int(rng.integers(0, span // 4))
        first = at
        for r in range(2 if p % 2 else 3):      # (every other pair is followed by a repeat that stands alone, 150 bases on)
            if r == 2:
                prot[first - 8: at] = True
                at += 150
                first = at
            unit = np.array(units.pop(next(i for i in range(len(units) - 1, -1, -1) if r < 2 or len(units[i]) <= 3)), np.int8)
            u = len(unit)
            copies = int(rng.integers(6, 10))
            ref[at: at + u * copies] = np.tile(unit, copies)
            repeats.append((at, u, copies, r == 2))
            at += u * copies + int(rng.integers(20, 31))
        prot[first - 8: at] = True
    sites = []        # (position, run, insertion length)
    shapes = [(3, 7), (1, 1), (6, 8), (6, -2)]
    ks = [k for k in range(2, length // 64 - 1) if not prot[64 * k + 8: 64 * k + 60].any()]
    for i, k in enumerate(ks[::max(1, len(ks) // 18)][:18]):
        at = 64 * k + 24 + int(rng.integers(0, 12))
        sites.append((at,) + shapes[i % 4])
        prot[at - 10: at + 16] = True
    longs = []        # positions of an insertion of 320 bases in the last genome: a gap above the reference's default d of 300
    for frac in (0.12, 0.52, 0.9):
        k = next(k for k in range(int(frac * length) // 64, length // 64 - 1) if not prot[64 * k + 8: 64 * k + 60].any())
        longs.append(64 * k + 32)
        prot[64 * k + 22: 64 * k + 42] = True
    shared = {}       # reference position -> base of every query genome
    for k in range(1, length // 64):
        at = 64 * k + (k % 3) - 1
        if not prot[at - 2: at + 3].any():
            shared[at] = (int(ref[at]) + 1 + int(rng.integers(0, 3))) % 4
    for at, run, _ in sites:
        for x in range(at, at + run):
            shared[x] = (int(ref[x]) + 1 + int(rng.integers(0, 3))) % 4
    last_inv = inversions[-1][0] if inversions else None
    seqs = [bases[ref].tobytes()]
    for g in range(1, n):
        a = ref.copy()
        for at, b in shared.items():
            a[at] = b
        hit = np.flatnonzero((rng.random(length) < 1.0 / (120 * (n - 1))) & ~prot)
        a[hit] = (a[hit] + rng.integers(1, 4, len(hit))) % 4
        edits = []    # (position, bases deleted, bases inserted)
        for at, u, copies, lone in repeats:
            delta = int(rng.integers(-1, 1)) if lone else int(rng.integers(-2, 3))
            if delta < 0:
                edits.append((at, -delta * u, a[:0]))
            elif delta > 0:
                edits.append((at, 0, np.tile(a[at: at + u], delta)))
        for i, (at, run, ins) in enumerate(sites):
            where = (last_inv if last_inv is not None else n - 1) if (i // 4 + i) % 2 == 0 else 1 + (i * 7) % (n - 1)
            if where == g:
                edits.append((at + run, 0, rng.integers(0, 4, ins).astype(np.int8)) if ins > 0 else (at + run + ins, -ins, a[:0]))
        if g == n - 1:
            edits += [(at, 0, rng.integers(0, 4, 320).astype(np.int8)) for at in longs]
        for at, cut, ins in sorted(edits, key=lambda e: -e[0]):
            a = np.concatenate([a[:at], ins, a[at + cut:]])
        s = bases[a].tobytes()
        for who, lo, hi in inversions:
            if who == g:
                lo, hi = int(lo * len(s)), int(hi * len(s))
                s = s[:lo] + revcomp(s[lo:hi]) + s[hi:]
        if translocate and translocate[0] == g:
            lo, hi = int(translocate[1] * len(s)), int(translocate[2] * len(s))
            s = s[lo:hi] + s[:lo] + s[hi:]
        seqs.append(s)
    return seqs
