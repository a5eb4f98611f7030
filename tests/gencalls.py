"""Call-level checks of the resident route's RECURSION (include/parsnp_mum.h: pm_store_search / _search_beside, pm_store_validate,
pm_store_order_check): a ctypes driver on top of storecalls.Store, the sequential restatement of the reference's work list on top
of storecalls.Model, a Python restatement of the generation former of Aligner::resident_extend (csrc/host/resident.cpp), and the
cases.  Plain Python and numpy, no engine code.

The restatement (GenModel) is the reference's doWork (src/parsnp.cpp:173-317) base by base: the candidates of a region are
oracles.restatement_multi_mum on the region's piece of every genome, mapped to whole-genome coordinates the way the TMum constructor
does (a reverse member is flipped against the WHOLE genome, TMum.cpp:33-35); they are settled with the loop of Model.settle against
the marks as they are (setMums1's second half); determineRegion on both sides of every new MUM gives the children, kept when longer
than q in every genome, in push order (:215-254); the list is sorted by reference start and a region equal to its neighbour erased
(:291-306).  do_work() is that list from the first pushed seed to the end.

What the generation scheme adds -- which clusters of a call run, which wait, where a cluster stops -- is checked as PROPERTIES
against a base-exact restatement of "two clusters meet" (cluster_relations: extents always; what the clusters' candidates touch only
in the calls that took the exact cluster test, which is all the header promises), because the engine defers by 64-base words and may
wait a generation longer than needed; everything a call DID is then compared exactly: the model is advanced by the regions the
engine reports as processed (advance_cluster: the rule of ClusterValidate) and every row, child and layout bit must agree.  At
the end, where the engine reports no trouble, the whole run must equal do_work(): the reference's order could not be seen.

Floors (every case, from do_work() and the model-only generation run, never from the engine): generations, regions with and
without candidates, accepted MUMs with a trim, kept children, children refused with slength == q exactly; on the rearranged sets
clusters that wait for one they meet in a genome but not on the reference, and reverse-strand candidates with a member outside their
region.  The restatement shows NO DROPPED DUPLICATE child (a child equal to a region still waiting in its cluster) on any set:
determineRegion begins a left neighbour on the base after a marked one and a right neighbour TWO bases after the MUM's last one,
on a base whose predecessor is unmarked; marks only grow and an accepted MUM keeps two bases or more, so two regions of different
MUMs cannot begin on one reference base unless one of them is stale, and then they differ in their end.
There is no floor for it; CASES records the count (0) and test_floors asserts that it stays 0.
On every case the model-only generation run gives do_work()'s accepted rows and layout, so every case must finish with trouble == 0
and an order check of 0.  On the two *_order cases it does NOT give do_work()'s rejected rows: there the order check has something to
decide (noted candidates whose marks differ between the orders) and must still answer 0; the restatement finds no set of this
family on which an ACCEPTED row differs, i.e. none on which the check must answer non-zero.
Every generation is also run as ONE cluster (`coarse`): the engine takes such lists, and the end state must be do_work()'s.

A tie run in which two regions have candidates would end a case as "route left" (the reference's unstable sort decides there); no
case holds one (RouteLeft is never raised, Reference.open_ties is 0, both asserted)."""
import copy
import ctypes as C
import functools
import math

import numpy as np

import oracles
import storecalls as sc
import test_store_calls as T
from storecalls import PM_OK, ROW_BAD, ROW_OUTSIDE, ROW_REVERSE, ST_ACCEPTED, ST_BUILT, ST_OK, ROW_INFO

PM_EINVAL = -2
K_PIECES = 8                     # store_kernels.h: kPieces
TR_PARTIAL, TR_REVERSE, TR_LIMIT, TR_DEFERRED = 1, 2, 4, 8      # the trouble bits of pm_store_validate
ROW_MASK = ROW_BAD | ROW_OUTSIDE | ROW_REVERSE      # (PM_ROW_DIRTY / _EARLY belong to the anchor call's overlap test; the recursion reads neither)
BESIDE = C.CFUNCTYPE(None, C.c_void_p)


def region_minsize(slength):
    """minimum MUM length of a recursion search, from the region's shortest side (the caller's choice: any rule does, this one falls
    with the region so that a child finds what its parent could not)"""
    return max(5, int(1.5 * math.log2(max(slength, 2))))


# ---------------------------------------------------------------------------------------------------------------- driver
def declare(L):
    sc.declare(L)
    v, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    P = C.POINTER
    sig = {
        "pm_store_search": (C.c_int, [v, v, v, i64, P(i64), v]),
        "pm_store_search_beside": (C.c_int, [v, v, v, i64, P(i64), v, BESIDE, v]),
        "pm_store_validate": (C.c_int, [v, v, v, v, i64, v, i64, i32, P(u32), P(i64), i64, i64, v, i64, P(i32), i32, v]),
        "pm_store_order_check": (C.c_int, [v, P(u32)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Answer:
    """what one pm_store_validate call returned"""


class GenStore(sc.Store):
    """storecalls.Store with the recursion's calls.  rows_total: the rows the MUM store holds (the anchor table + every search)."""

    def __init__(self, lib, seqs, tune=None, minsize=sc.MINSIZE):
        super().__init__(lib, seqs, tune=tune, minsize=minsize)
        declare(self.L)
        self.rows_total = self.A

    def search(self, ids, mins, beside=False):
        """-> (return code, first_row, offsets[n + 1], calls of the callback or None)"""
        ids, mins = sc._i32(ids), sc._i32(mins)
        n = len(ids)
        first, off = C.c_int64(-1), np.full(n + 1, -1, np.int64)
        calls = []
        if beside:
            cb = BESIDE(lambda ctx: calls.append(1))
            rc = self.L.pm_store_search_beside(self.h, _ptr(ids), _ptr(mins), n, C.byref(first), _ptr(off), cb, None)
        else:
            rc = self.L.pm_store_search(self.h, _ptr(ids), _ptr(mins), n, C.byref(first), _ptr(off))
        if rc == PM_OK:
            self.rows_total += int(off[n])
        return rc, first.value, off, (len(calls) if beside else None)

    def validate(self, regions, row0, cnt, cluster_first, q, generation, stage_first=0, with_done=True, info_range=None):
        """info_range None: the range the product asks for -- from the first to the last candidate of the list"""
        regions, cnt = sc._i32(regions), sc._i32(cnt)
        row0, first = np.ascontiguousarray(row0, np.int64), np.ascontiguousarray(cluster_first, np.int64)
        ncl = len(first) - 1
        if info_range is None:
            have = cnt > 0
            info_range = (int(row0[have].min()), int((row0[have] + cnt[have]).max())) if have.any() else (0, 0)
        lo, hi = info_range
        a = Answer()
        a.info_first, a.info = lo, np.zeros(max(hi - lo, 0), ROW_INFO)
        trouble, nkids, ran = C.c_uint32(0x55), C.c_int64(-1), C.c_int32(-1)
        a.done = np.full(ncl, -7, np.int32) if with_done else None
        a.rc = self.L.pm_store_validate(self.h, _ptr(regions), _ptr(row0), _ptr(cnt), len(regions), _ptr(first), ncl, q, C.byref(trouble), C.byref(nkids),
                                        lo, hi - lo, _ptr(a.info) if hi > lo else None, stage_first, C.byref(ran), generation, _ptr(a.done) if with_done else None)
        a.trouble, a.second_ran = trouble.value, ran.value
        if a.rc == PM_OK:
            a.kids, a.kid_ids = self._regions(nkids.value)
        return a

    def order_check(self):
        t = C.c_uint32(0x55)
        self.check(self.L.pm_store_order_check(self.h, C.byref(t)))
        return t.value

    def timing(self):
        return dict(self.sess.last_timing())


# ---------------------------------------------------------------------------------------------------------------- restatement
class Region:
    """a TRegion: rows = ((start, length) per genome), length = end - start (LCR.cpp:29)"""
    __slots__ = ("rows", "ref_start", "ref_len", "slength", "parent", "eid", "row0", "cnt")

    def __init__(self, rows, parent):
        self.rows = tuple((int(a), int(ln)) for a, ln in rows)
        self.ref_start, self.ref_len = self.rows[0]
        self.slength = min(ln for _, ln in self.rows)
        self.parent = parent
        self.eid = self.row0 = self.cnt = None      # the engine's id; where its candidates lie in the store (None: not searched yet)

    def twin(self):
        return Region(self.rows, self.parent)


class Stats:
    def __init__(self):
        self.with_cands = self.without = self.trimmed = self.kept = self.at_q = self.dups = self.reverse_outside = self.accepted = self.long_outside = 0

    def __repr__(self):
        return repr(self.__dict__)


class GenModel(sc.Model):
    """storecalls.Model whose store grows: every search appends its candidates as rows, as pm_store_search does"""
    MEMO = {}      # memo key (one per set) -> {(region rows, minsize): candidates}: the model runs of one set share their searches

    def __init__(self, seqs, raw_start, strand, lon, flags, memo_key):
        super().__init__(seqs, raw_start, strand, lon, flags)
        self.strand = np.asarray(strand, np.uint8)
        self.memo = GenModel.MEMO.setdefault(memo_key, {})
        self.stats = Stats()
        self.processed = []

    def fork(self):
        m = copy.copy(self)
        m.marks = [x.copy() for x in self.marks]
        for name in ("lon", "flags", "accepted", "shift", "len", "crossings", "processed"):
            setattr(m, name, list(getattr(self, name)))
        m.stats = Stats()
        return m

    def search(self, rows, minsize):
        """the candidates of one region -> (lon[c], raw start[c, genomes], strand[c, genomes], PM_ROW_* bits[c]) in candidate order"""
        key = (rows, minsize)
        if key not in self.memo:
            sub = [self.seqs[j][a: a + ln] for j, (a, ln) in enumerate(rows)]
            k, lon, sp, fw = oracles.restatement_multi_mum(oracles.load_restatement(), sub, minsize, 1)
            c, n = len(k), self.n
            lon = lon.astype(np.int64)
            start, strand, flags = np.zeros((c, n), np.int64), np.ones((c, n), np.uint8), np.zeros(c, np.uint32)
            start[:, 0] = rows[0][0] + k
            flags[k >= rows[0][1]] |= ROW_BAD
            for j in range(1, n):
                at, f = rows[j][0] + sp[:, j - 1], fw[:, j - 1] != 0
                start[:, j] = np.where(f, at, self.glen[j] - (at + lon))      # (TMum.cpp:33-35: against the whole genome)
                strand[:, j] = f
                flags[(sp[:, j - 1] < 0) | (sp[:, j - 1] >= rows[j][1])] |= ROW_BAD
                flags[~f] |= ROW_REVERSE
            outside = ((start < 0) | (start + lon[:, None] > np.array(self.glen)[None, :])).any(axis=1) if c else np.zeros(0, bool)
            flags[outside] |= ROW_OUTSIDE
            self.memo[key] = (lon, start, strand, flags)
        return self.memo[key]

    def append(self, found):
        """-> (first row, count) of the candidates in the model's store"""
        lon, start, strand, flags = found
        row0, c = self.A, len(lon)
        if c:
            self.start = np.vstack([self.start, start])
            self.strand = np.vstack([self.strand, strand])
            self.lon += [int(x) for x in lon]
            self.len += [int(x) for x in lon]
            self.flags += [int(x) for x in flags]
            self.accepted += [False] * c
            self.shift += [0] * c
            self.A += c
        return row0, c

    def search_region(self, reg):
        if reg.row0 is None:
            reg.row0, reg.cnt = self.append(self.search(reg.rows, region_minsize(reg.slength)))

    def reverse_outside(self, reg, c):
        """a reverse-strand member of candidate c outside its region (the test of ClusterValidate: one base of margin)"""
        if (self.flags[c] & (ROW_BAD | ROW_OUTSIDE)) or not (self.flags[c] & ROW_REVERSE):
            return False
        return any(not self.strand[c, j] and (self.start[c, j] < rs - 1 or self.start[c, j] + self.lon[c] > rs + rl + 1) for j, (rs, rl) in enumerate(reg.rows))

    def validate_region(self, reg, q):
        """setMums1's second half on the region's candidates against the current marks, then determineRegion on both sides of every
        new MUM -> the kept children in push order (left then right, candidate by candidate)"""
        rows = range(reg.row0, reg.row0 + reg.cnt)
        self.settle_rows(rows)
        s = self.stats
        s.with_cands += reg.cnt > 0
        s.without += reg.cnt == 0
        kept = []
        for c in rows:
            s.reverse_outside += self.reverse_outside(reg, c)
            s.long_outside += self.lon[c] > 64 and self.reverse_outside(reg, c)      # (the engine notes 64 bases of marks per member: longer ones end the route, trouble bit 2)
            if not self.accepted[c]:
                continue
            s.accepted += 1
            s.trimmed += self.shift[c] > 0 or self.len[c] < self.lon[c]
            for side in (0, 1):
                rr = [self.region_side(c, side, j) for j in range(self.n)]
                child = Region([(a, b - a) for a, b in rr], c)
                if child.slength > q:
                    kept.append(child)
                else:
                    s.at_q += child.slength == q
        s.kept += len(kept)
        self.processed.append(reg)
        return kept

    def do_work(self, seeds, q):
        """the reference's work list (:173-317) -> the number of tie runs in which two regions have candidates (its unstable sort
        would decide there: the cases must not hold one)"""
        work = [r.twin() for r in seeds]
        open_ties = 0
        while work:
            reg = work.pop(0)
            self.search_region(reg)
            work += self.validate_region(reg, q)
            work.sort(key=lambda r: r.ref_start)
            i = 0
            while i < len(work) - 1:
                if work[i].rows == work[i + 1].rows:
                    del work[i]
                    self.stats.dups += 1
                else:
                    i += 1
            i = 0
            while i < len(work):
                e = i + 1
                while e < len(work) and work[e].ref_start == work[i].ref_start:
                    e += 1
                if e - i > 1:
                    open_ties += sum(1 for r in work[i:e] if len(self.search(r.rows, region_minsize(r.slength))[0]) > 0) > 1
                i = e
        return open_ties

    def by_region(self, raw=False):
        """{region rows: [(accepted, shift, len) per candidate]} of the processed regions; shift and len of a row that is NOT accepted are
        left out (None): such a row leaves nothing in the run's output, what its trim found depends on the marks at the moment it was
        looked at, and the engine's own order check compares them for accepted rows only (verdict_differs); raw: all of it"""
        out = {}
        for r in self.processed:
            assert r.rows not in out, "a region was processed twice"
            out[r.rows] = [(self.accepted[c], self.shift[c], self.len[c]) if raw or self.accepted[c] else (False, None, None) for c in range(r.row0, r.row0 + r.cnt)]
        return out


def advance_cluster(m, regs, q):
    """one wavefront of ClusterValidate on the model: the regions of a cluster in list order until a kept, non-duplicate child of a
    processed region sorts before (or ties with) the next one -> (regions processed, children listed)"""
    pending, kids = -1, []
    for x, r in enumerate(regs):
        if pending >= 0 and pending <= r.ref_start:
            return x, kids
        for k in m.validate_region(r, q):
            if any(k.rows == y.rows for y in regs[x + 1:]):      # equal to a region still waiting in its cluster: dropped (:294-306)
                m.stats.dups += 1
                continue
            kids.append((x, k))
            pending = k.ref_start if pending < 0 else min(pending, k.ref_start)
    return len(regs), kids


# ---------------------------------------------------------------------------------------------------------------- clusters that meet
def _clip(a, b, nbits):
    return max(a, 0), min(b, nbits)


def cluster_pieces(m, now, first, cl):
    """what cluster cl touches, per genome: (extents, readers, markers) as lists of [a, b) -- the union of its regions with two bases
    of margin (the hull above K_PIECES regions), the reverse members outside their region and every member of every candidate with
    one base of margin"""
    regs = now[first[cl]: first[cl + 1]]
    ext, rd, mk = [], [], []
    for j in range(m.n):
        nbits = m.glen[j] + 1
        if len(regs) > K_PIECES:
            e = [_clip(min(r.rows[j][0] for r in regs), max(r.rows[j][0] + r.rows[j][1] for r in regs) + 2, nbits)]
        else:
            e = [_clip(r.rows[j][0], r.rows[j][0] + r.rows[j][1] + 2, nbits) for r in regs]
        ext.append([(a, b) for a, b in e if a < b])
        rj, mj = [], []
        for r in regs:
            rs, rl = r.rows[j]
            for c in range(r.row0, r.row0 + r.cnt):
                if m.flags[c] & (ROW_BAD | ROW_OUTSIDE):
                    continue
                a, b = int(m.start[c, j]), int(m.start[c, j]) + m.lon[c]
                mj.append(_clip(a - 1, b + 1, nbits))
                if (m.flags[c] & ROW_REVERSE) and not m.strand[c, j] and (a < rs - 1 or b > rs + rl + 1):
                    rj.append(_clip(a - 1, b + 1, nbits))
        rd.append(rj)
        mk.append(mj)
    return ext, rd, mk


def cluster_relations(m, now, first, c0=0, candidates=True):
    """-> (must[cl], pieces, clusters that wait for their margins alone) for the clusters [c0, ...) of a call that run side by side:
    must -- the cluster meets an EARLIER one base-exactly in some genome (extents with their two bases of margin under each other, or
    a reader of one under a marker of the other with their one base of margin): it has to wait.  candidates = False: extents only --
    what the engine promises for a call that passes its collinear test (ClustersDisjoint looks at extents; a reader beside a marker is
    then left to pm_store_order_check)"""
    ncl = len(first) - 1
    P = {cl: cluster_pieces(m, now, first, cl) for cl in range(c0, ncl)}
    must, close = {cl: False for cl in P}, {cl: False for cl in P}      # close: the cluster waits for a reader and a marker ONE base apart
    for j in range(m.n):
        active = []
        for a, b, cl in sorted((a, b, cl) for cl in P for a, b in P[cl][0][j]):
            active = [(e, c) for e, c in active if e > a]
            for _, c in active:
                if c != cl:
                    must[max(c, cl)] = True
            active.append((b, cl))
        readers = [(a, b, cl) for cl in P for a, b in P[cl][1][j]]
        if readers and candidates:
            markers = [(a, b, cl) for cl in P for a, b in P[cl][2][j]]
            for a, b, cl in readers:
                for c, d, other in markers:
                    if other != cl and a < d and c < b:
                        if min(b, d) - max(a, c) == 1:      # the two members lie ONE base apart: only both margins together see it
                            close[max(cl, other)] = True
                        else:
                            must[max(cl, other)] = True
    margin = sum(1 for cl in P if close[cl] and not must[cl])      # ... and for nothing else
    for cl in P:
        must[cl] = must[cl] or close[cl]
    return must, P, margin


def shares_a_word(P, cl, n):
    """does the cluster share a 64-base word of some genome with another cluster's extents or candidates (the engine may let it wait)?"""
    def words(c, j):
        return {w for k in range(3) for a, b in P[c][k][j] for w in range(a >> 6, ((b - 1) >> 6) + 1)}
    for j in range(n):
        mine = words(cl, j)
        if mine and any(mine & words(c, j) for c in P if c != cl):
            return True
    return False


# ---------------------------------------------------------------------------------------------------------------- generation former
class RouteLeft(Exception):
    pass


def sort_unique(gen, out, equal):
    """sorted by reference start; a region equal to one with its reference start dropped -> the tie runs (first, count, lost a duplicate)"""
    ties, run0, lost = [], len(out), False

    def close():
        if len(out) - run0 > 1:
            ties.append((run0, len(out) - run0, lost))
    for r in sorted(gen, key=lambda r: r.ref_start):
        if len(out) > run0 and out[run0].ref_start != r.ref_start:
            close()
            run0, lost = len(out), False
        if any(o.ref_len == r.ref_len and o.slength == r.slength and equal(o, r) for o in out[run0:]):
            lost = True
            continue
        out.append(r)
    close()
    return ties


def settle_ties(now, ties):
    for t0, count, lost in ties:
        have = [y for y in range(t0, t0 + count) if now[y].cnt > 0]
        if len(have) > 1 or (have and lost):
            raise RouteLeft("two different regions with candidates share a reference start")
        if have and have[0] != t0 + count - 1:
            now[have[0]], now[t0 + count - 1] = now[t0 + count - 1], now[have[0]]


def clusters(now, base, first, coarse):
    """maximal runs that overlap or touch on the reference; coarse: ONE cluster, the serial extreme"""
    reach = -1
    for i in range(base, len(now)):
        if i == base or (now[i].ref_start > reach + 1 and not coarse):
            first.append(i)
        reach = max(reach, now[i].ref_start + now[i].ref_len)
    first.append(len(now))


def run_generations(side, seeds, q, two_stage=False, coarse=False, stop_after=None):
    """Aligner::resident_extend around the calls (csrc/host/resident.cpp): `side` makes them (EngineSide: the engine, checked
    against the model; ModelSide: the model alone).  -> the generations run; stop_after: leave after that many calls"""
    gen, gi, calls = list(seeds), 0, 0
    while gen:
        now, first, stage_first, rest = [], [], 0, None
        if gi == 0:
            side.search(gen)
            now, first, gen = [gen[0]], [0], gen[1:]
            if two_stage and gen:
                rest = list(gen)
                settle_ties(now, sort_unique(gen, now, side.equal))
                clusters(now, 1, first, coarse)
                stage_first, gen = 1, []
            else:
                first.append(1)
        else:
            ties = sort_unique(gen, now, side.equal)
            side.search(now)
            settle_ties(now, ties)
            clusters(now, 0, first, coarse)
            gen = []
        done, kids, second_ran, trouble = side.validate(now, first, q, gi, stage_first)
        calls += 1
        if trouble or (stop_after is not None and calls >= stop_after):
            return gi
        if stage_first > 0 and not second_ran:
            first, done, gen, stage_first = [0, 1], done[:1], rest, 0
        for cl in range(len(first) - 1):
            gen += now[first[cl] + done[cl]: first[cl + 1]]
        assert done[0] >= 1, "a generation processed nothing"
        gen += kids
        gi += 2 if stage_first > 0 else 1
    return gi


def in_reference_order(m, now, first, c0=0):
    """ClustersDisjoint: every cluster of the stage starts after its predecessor ends, with a base between, in every genome"""
    for cl in range(c0 + 1, len(first) - 1):
        for j in range(1, m.n):
            hi = max(r.rows[j][0] + r.rows[j][1] for r in now[first[cl - 1]: first[cl]])
            lo = min(r.rows[j][0] for r in now[first[cl]: first[cl + 1]])
            if lo <= hi + 1:
                return False
    return True


class ModelSide:
    """the generation scheme on the model alone, as the header promises it: while every call holds its clusters in reference order in
    every genome they all run; from the first call that does not, a cluster waits exactly when it meets an earlier one base-exactly
    (extents, readers under markers).  reverse: the clusters of a stage are processed last to first -- what the emulation does with
    the wavefronts of cluster_validate reversed, and one of the orders a device may take"""

    def __init__(self, m, reverse=False):
        self.m, self.met, self.by_margin, self.calls, self.reverse, self.exact = m, 0, 0, [], reverse, False

    def equal(self, a, b):
        return a.rows == b.rows

    def search(self, regs):
        for r in regs:
            self.m.search_region(r)

    def validate(self, now, first, q, gi, stage_first):
        ncl = len(first) - 1
        done, kids = [0] * ncl, {}
        if not self.exact and not in_reference_order(self.m, now, first, 0):
            self.exact = True
        for c0, c1 in ((0, stage_first), (stage_first, ncl)) if stage_first else ((0, ncl),):
            if c0 and kids:
                break
            must, _, margin = cluster_relations(self.m, now, first[: c1 + 1], c0) if self.exact and c1 - c0 > 1 else ({cl: False for cl in range(c0, c1)}, None, 0)
            self.met += sum(must.values())
            self.by_margin += margin
            for cl in (range(c1 - 1, c0 - 1, -1) if self.reverse else range(c0, c1)):
                if not must[cl]:
                    done[cl], k = advance_cluster(self.m, now[first[cl]: first[cl + 1]], q)
                    kids[cl] = [x[1] for x in k]
        ran2 = 1 if stage_first and (done[stage_first:] != [0] * (ncl - stage_first) or not kids.get(0)) else 0
        self.calls.append((gi, list(done)))
        return done, [k for cl in sorted(kids) for k in kids[cl]], ran2, 0


def anchor_model(seqs, minsize, memo_key):
    """the anchor table from the restatement alone (the whole genomes as one region), settled"""
    probe = GenModel(seqs, np.zeros((0, len(seqs)), np.int64), np.zeros((0, len(seqs)), np.uint8), [], [], memo_key)
    whole = tuple((0, len(s)) for s in seqs)
    lon, start, strand, flags = probe.search(whole, minsize)
    return GenModel(seqs, start, strand, lon, flags, memo_key).settle()


def seed_regions(m, q):
    return [Region(rows, d["parent"]) for d, rows in m.seeds(q)]



# ---------------------------------------------------------------------------------------------------------------- the engine's side
def _words(xs):
    return " ".join(str(int(x)) if not isinstance(x, str) else x for x in xs) or "-"


def _same(got, want, what):
    d = T.first_diff(got, want)
    assert d is None, "%s: %s" % (what, d)


class EngineSide:
    """the calls on the engine, every one compared with the model, which is advanced by exactly the regions the engine reports as
    processed, cluster by cluster and in list order"""

    def __init__(self, st, m, collinear):
        self.st, self.m, self.collinear = st, m, collinear
        self.trace = []           # per validate call, what must not change from run to run: done[], info[], the listed children, the layout
        self.calls = []           # per validate call: its lists and what came back
        self.searches = 0
        self.script = []          # the calls as text, with what the restatement says to them (write_cases)
        self.seen_ids = set()
        self.loose_rows = set()   # rejected rows of readers decided beside a marker: their trim is not compared
        self.null_done_at = self.null_expect = None      # the call that passes done == NULL, and the done[] an earlier run saw there

    def equal(self, a, b):
        same = bool(self.st.regions_equal([a.eid], [b.eid])[0])
        assert same == (a.rows == b.rows), "pm_store_regions_equal(%d, %d) = %d; the restated rows are %s" % (a.eid, b.eid, same, "equal" if a.rows == b.rows else "different")
        return same

    def search(self, regs):
        st, m = self.st, self.m
        want = [r for r in regs if r.row0 is None]
        if not want:
            return
        mins = [region_minsize(r.slength) for r in want]
        before = st.rows_total
        rc, first, off, calls = st.search([r.eid for r in want], mins, beside=self.searches % 2 == 1)      # (every other search through _beside)
        self.searches += 1
        st.check(rc)
        self.script.append("SEARCH %d %d %s %s %d %s" % (len(want), self.searches % 2 == 0, _words(r.eid for r in want), _words(mins), first, _words(off)))
        assert first == before == m.A, "first_row %d; the store held %d rows (the restatement's %d)" % (first, before, m.A)
        assert calls in (None, 1), "pm_store_search_beside called back %s times" % calls
        self.compare_search(want, mins, first, off)

    def compare_search(self, want, mins, first, off):
        """store rows [first + off[i], first + off[i + 1]) against Model.search of region i; the model's store takes them too"""
        st, m = self.st, self.m
        total = int(off[len(want)])
        assert off[0] == 0 and (np.diff(off) >= 0).all(), off
        if total:
            start, strand = st.rows(None, first, total, raw=True)
            info = st.info(first, total)
        for i, r in enumerate(want):
            found = m.search(r.rows, mins[i])
            lon, ws, wf, wflags = found
            a, b = int(off[i]), int(off[i + 1])
            what = "pm_store_search of region %d+%d (minimum length %d)" % (r.ref_start, r.ref_len, mins[i])
            assert b - a == len(lon), "%s: %d candidates, the restatement finds %d" % (what, b - a, len(lon))
            if b > a:
                _same(start[a:b], ws, what + ": raw starts")
                _same(strand[a:b], wf, what + ": strands")
                _same(info["len"][a:b], lon, what + ": lengths")
                _same((info["state_flags"][a:b] >> 8) & ROW_MASK, wflags, what + ": PM_ROW_* bits")
                _same(info["start0"][a:b], ws[:, 0], what + ": start0")
                assert not (info["state_flags"][a:b] & 0xff).any() and not info["shift"][a:b].any(), what + ": a fresh row with a state or a shift"
            r.row0, r.cnt = m.append(found)
            assert r.row0 == first + a

    def validate(self, now, first, q, gi, stage_first):
        st, m = self.st, self.m
        ncl = len(first) - 1
        call = len(self.calls)
        with_done = self.null_done_at != call
        what = "pm_store_validate, call %d (generation %d, %d regions in %d clusters)" % (call, gi, len(now), ncl)
        ans = st.validate([r.eid for r in now], [r.row0 for r in now], [r.cnt for r in now], first, q, gi, stage_first, with_done=with_done)
        st.check(ans.rc)
        timing = st.timing()
        exact = timing.get("exact_cluster_tests", 0) > 0      # the call asked which clusters meet: only then do their CANDIDATES count
        assert not (ans.trouble & TR_LIMIT), what + ": trouble bit 2 on a list of this size"
        if self.collinear and with_done:
            assert ans.trouble == 0, "%s: trouble %d on a collinear set" % (what, ans.trouble)
        if with_done:
            assert not (ans.trouble & (TR_PARTIAL | TR_DEFERRED)), what + ": trouble bits 0 / 3 although done[] was given"
        done = [int(x) for x in ans.done] if with_done else list(self.null_expect)
        assert ans.second_ran in (0, 1) and (stage_first or ans.second_ran == 0), ans.second_ran
        assert done[0] >= 1, what + ": nothing processed"
        stages = [(0, stage_first), (stage_first, ncl)] if stage_first else [(0, ncl)]
        if stage_first and not ans.second_ran:
            stages = stages[:1]
            assert not any(done[stage_first:]), what + ": the second stage did not run and done[] is not 0 there"
        expect, met, waiting, ran = [], 0, 0, [False] * len(now)
        for c0, c1 in stages:
            must, P, _ = cluster_relations(m, now, first[: c1 + 1], c0, exact) if c1 - c0 > 1 else ({c0: False}, None, 0)
            met += sum(must.values())
            for cl in range(c0, c1):
                size = first[cl + 1] - first[cl]
                assert 0 <= done[cl] <= size, (what, cl, done[cl], size)
                if done[cl] == 0:
                    assert cl > c0, what + ": the first cluster of a stage waits"
                    waiting += 1
                    assert shares_a_word(P, cl, m.n), "%s: cluster %d waits and shares no 64-base word with another cluster's extents or candidates" % (what, cl)
                    continue
                assert not must[cl], "%s: cluster %d meets an earlier cluster in some genome and was processed beside it (done %d)" % (what, cl, done[cl])
                d, kids = advance_cluster(m, now[first[cl]: first[cl + 1]], q)
                assert d == done[cl], "%s: done[%d] = %d; the rule of ClusterValidate stops after %d of %d" % (what, cl, done[cl], d, size)
                expect += [(first[cl] + x, k) for x, k in kids]
                for x in range(first[cl], first[cl] + d):
                    ran[x] = True
        # the rows: those of processed regions as the model decided them, the others untouched
        lo, info = ans.info_first, ans.info
        rows_said = []
        for x, r in enumerate(now):
            for c in range(r.row0, r.row0 + r.cnt):
                g, f = info[c - lo], m.flags[c]
                got = (int(g["state_flags"]) & 0xff, int(g["shift"]), int(g["len"]), int(g["start0"]))
                if ran[x]:
                    state = (0 if f & ROW_BAD else ST_BUILT) | (0 if f & (ROW_BAD | ROW_OUTSIDE) else ST_OK) | (ST_ACCEPTED if m.accepted[c] else 0)
                    want = (state, m.shift[c], m.len[c], int(m.start[c, 0]) + m.shift[c])
                else:
                    want = (0, 0, m.lon[c], int(m.start[c, 0]))
                rows_said.append("%d %d %d %d %d" % ((c,) + want))
                if ran[x] and not m.accepted[c] and not got[0] & ST_ACCEPTED and m.reverse_outside(r, c):
                    # a rejected row with a reverse member outside its region: in a call that passed the collinear test what its trim found
                    # depends on how far the cluster beside it had come, and nothing of it reaches the output (by_region).  Not compared
                    # there, and in no call part of what must repeat from run to run (trace)
                    self.loose_rows.add(c)
                    if not exact:
                        got, want = got[:1], want[:1]
                assert got == want, "%s: row %d of region %d+%d (%s): (state, shift, len, start0) = %s, restatement %s" % (
                    what, c, r.ref_start, r.ref_len, "processed" if ran[x] else "waiting", got, want)
                assert (int(g["state_flags"]) >> 8) & ROW_MASK == f & ROW_MASK
        if len(info):
            again = st.info(lo, len(info))
            assert again.tobytes() == info.tobytes(), what + ": pm_store_info differs from the info[] of the call"
        layout = st.layout()
        T.same_layout(layout, m.layout(), what)
        # the children, through the listed order
        kids, ids = ans.kids, [int(x) for x in ans.kid_ids]
        assert len(kids) == len(expect), "%s: %d children listed, the restatement keeps %d" % (what, len(kids), len(expect))
        assert (np.diff(kids["key"]) > 0).all(), what + ": the children's keys do not rise"
        _same(kids["key"] >> 24, [x for x, _ in expect], what + ": list position of the children's parents")
        for field in ("ref_start", "ref_len", "slength", "parent"):
            _same(kids[field], [getattr(k, field) for _, k in expect], what + ": " + field + " of the children")
        assert len(set(ids)) == len(ids) and not (set(ids) & self.seen_ids), what + ": region ids repeat"
        self.seen_ids |= set(ids)
        for (_, k), eid in zip(expect, ids):
            k.eid = eid
        if ids:      # every genome's extent of a child: each child against itself and against the next one, as the seed-region test does
            rows = [k.rows for _, k in expect]
            same = st.regions_equal(ids + ids[:-1], ids + ids[1:])
            _same(same, [1] * len(ids) + [int(a == b) for a, b in zip(rows, rows[1:])], what + ": pm_store_regions_equal on the children")
        if with_done:
            self.script.append("VALIDATE %d %d %d %d %s %s %s %s %d %d %s %d %s %d %s" % (
                len(now), ncl, gi, stage_first, _words(r.eid for r in now), _words(r.row0 for r in now), _words(r.cnt for r in now), _words(first), ans.trouble, ans.second_ran,
                _words(done), len(expect), _words("%d %d %d %d" % (k.ref_start, k.ref_len, k.slength, k.parent) for _, k in expect), len(rows_said), _words(rows_said)))
        steady = info.copy()
        for field in ("shift", "len", "start0"):      # (rows of earlier calls lie in the window too)
            steady[field][[c - lo for c in self.loose_rows if lo <= c < lo + len(info)]] = 0
        self.trace.append((tuple(done), steady.tobytes(), kids.tobytes(), tuple(x.tobytes() for x in layout)))
        self.calls.append(dict(gi=gi, regions=len(now), first=list(first), stage_first=stage_first, done=done, trouble=ans.trouble, second_ran=ans.second_ran, met=met,
                               deferred=waiting, partial=sum(1 for cl, d in enumerate(done) if 0 < d < first[cl + 1] - first[cl]),
                               largest=max(first[cl + 1] - first[cl] for cl in range(ncl)), kids=len(kids), timing=timing, exact=exact))
        return done, [k for _, k in expect], ans.second_ran, ans.trouble


# ---------------------------------------------------------------------------------------------------------------- cases
# case -> (set of test_store_calls.SETS, minimum MUM length of the anchor call, q, what the restatement gives).  Both numbers were picked
# from the restatement's output alone (anchor_model + do_work + the model-only generation run) on a grid of 30 .. 120 x 3 .. 10: an
# anchor length at which every floor holds, no tie run is open, the model-only generation run equals do_work() and no reverse candidate
# with a member outside is longer than 64 bases (80 on the collinear sets, 70, 66 and 60 on the rearranged ones); q = 3 keeps the most
# regions.  In brackets what they give: [generations, regions with candidates, regions without, accepted MUMs
# with a trim, kept children, refused at slength == q, dropped duplicates, clusters that wait for an earlier one, reverse candidates
# with a member outside].  An anchor call at 80 finds a dozen anchors; everything shorter stays between them for the recursion.
# (At an anchor length of 70 the model-only run of collinear6 and of inverted70 DIFFERS from do_work(): a reverse member outside its
# region reads where a cluster beside it marks, in a call that passes the engine's collinear test, which looks at extents only.  The
# header leaves that to pm_store_order_check; the claim "a reader under a marker waits" is asserted here for the calls of these cases,
# where it holds, and is not the engine's promise for every list.)
CASES = {
    "collinear6": ("collinear6", 80, 3, [4, 117, 20, 20, 114, 13, 0, 0, 1]),
    "collinear70": ("collinear70", 80, 3, [4, 80, 15, 15, 82, 8, 0, 0, 1]),
    "collinear131": ("collinear131", 80, 3, [4, 54, 14, 11, 60, 9, 0, 0, 2]),
    "rearranged8": ("rearranged8", 70, 3, [11, 90, 20, 11, 81, 10, 0, 22, 6]),
    # the same set with 19 bases behind the end of its inverted genome: a reverse member is flipped against the WHOLE genome, so every
    # member outside its region lands 19 bases further on -- one of them then lies exactly ONE base from a candidate of another cluster
    # of its call, which meets it in no other way: only ReaderMark's and MarkerLook's margins together make that cluster wait (MARGIN_FLOOR;
    # the offset was searched with the restatement alone, 0 .. 63 bases at anchor lengths 60 and 70)
    "rearranged8_margin": ("rearranged8_margin", 60, 3, [6, 136, 41, 5, 38, 6, 0, 19, 8]),
    # (no reverse candidate with a member outside may be longer than 64 bases -- the engine notes 64 bases of marks per member and ends the route
    # beyond, trouble bit 2 -- which bounds the anchor call's minimum length on this set)
    "inverted70": ("inverted70", 66, 3, [11, 78, 19, 5, 77, 5, 0, 14, 4]),
    # the order SHOWS in the restatement: a rejected candidate with a reverse member outside its region is trimmed differently in list order
    # and in generation order (ORDER_ROWS), in calls that pass the collinear test -- a reader beside a marker, which the engine leaves to
    # pm_store_order_check.  The accepted rows agree in both orders of the clusters (the restatement finds no set of this family on which
    # they do not: such a candidate fails its sequence check whatever it reads), so the check has to answer 0 and the run equal do_work()
    "collinear6_order": ("collinear6", 70, 3, [4, 121, 20, 14, 112, 13, 0, 0, 3]),
    "inverted70_order": ("inverted70", 70, 3, [4, 83, 16, 7, 81, 4, 0, 0, 6]),
}
ORDER_ROWS = {"collinear6_order": 1, "inverted70_order": 1}      # regions with a row whose (shift, len) differ between the two orders
FLOORS = dict(generations=3, with_cands=10, without=1, trimmed=5, kept=3, at_q=1)
REARRANGED_FLOORS = dict(met=1, reverse_outside=1)

TAILS = {"rearranged8_margin": ("rearranged8", 7, (b"ACGTTGCA" * 3)[:19])}      # set -> (set of test_store_calls.SETS, genome, bases appended to it)
MARGIN_FLOOR = {"rearranged8_margin": 1}      # clusters of a call that wait ONLY because a reader and a marker of two clusters lie one base apart


@functools.lru_cache(maxsize=None)
def sequences(name):
    if name in TAILS:
        base, who, tail = TAILS[name]
        seqs = list(sequences(base))
        seqs[who] += tail
        return seqs
    return sc.make_set(**T.SETS[name])


class Reference:
    """what the restatement alone says about a case"""


@functools.lru_cache(maxsize=None)
def reference(case, rotate=0):
    """do_work() and the model-only generation run of a case, from the restatement's own anchor table; rotate: the seed list starts
    with its rotate-th entry (the first pushed seed is processed before anything is sorted)"""
    name, ams, q, _ = CASES[case]
    base = anchor_model(sequences(name), ams, (name, ams))
    seeds = seed_regions(base, q)
    seeds = seeds[rotate:] + seeds[:rotate]
    r = Reference()
    r.base, r.seeds = base, seeds
    r.work = base.fork()
    r.open_ties = r.work.do_work(seeds, q)
    r.gen = base.fork()
    r.side = ModelSide(r.gen)
    r.generations = run_generations(r.side, [s.twin() for s in seeds], q)
    r.order_free = r.work.by_region() == r.gen.by_region() and all(np.array_equal(a, b) for a, b in zip(r.work.marks, r.gen.marks))
    r.order_rows = 0
    if case in ORDER_ROWS:      # ... and with the clusters of every call last to first
        back = base.fork()
        run_generations(ModelSide(back, reverse=True), [s.twin() for s in seeds], q)
        assert back.by_region() == r.work.by_region(), "the accepted rows depend on the order of the clusters"
        want = r.work.by_region(raw=True)
        r.order_rows = max(sum(1 for k, v in want.items() if x.by_region(raw=True).get(k) != v) for x in (r.gen, back))
    s = r.work.stats
    r.numbers = [r.generations, s.with_cands, s.without, s.trimmed, s.kept, s.at_q, s.dups + r.gen.stats.dups, r.side.met, s.reverse_outside]
    return r


class Run:
    """one session on a case"""


def run_case(lib, case, two_stage=False, coarse=False, tune=None, rotate=0, null_done_at=None, null_expect=None, stop_after=None, then=None):
    """the anchor call, pm_store_settle_seeds and the generations of one session -> Run; then(st, side, run): more calls on the open session"""
    name, ams, q, _ = CASES[case]
    seqs = sequences(name)
    ref = reference(case, rotate)
    r = Run()
    knobs = {"dirty_min": 1}      # (an anchor call at this minimum length leaves a handful of rows: they become the anchor table all the same)
    knobs.update(dict(tune) if tune else {})
    with GenStore(lib, seqs, tune=knobs, minsize=ams) as st:
        base = ref.base
        assert st.A == base.A, "the anchor call found %d candidates, the restatement %d" % (st.A, base.A)
        _same(st.raw_start, base.start[:st.A], "the anchor call's raw starts")
        _same(st.lon, base.lon[:st.A], "the anchor call's lengths")
        _same(st.flags & ROW_MASK, np.array(base.flags[:st.A]) & ROW_MASK, "the anchor call's PM_ROW_* bits")
        m = GenModel(seqs, st.raw_start, st.strand, st.lon, st.flags, (name, ams)).settle()
        info, regs, ids = st.settle_seeds(q)
        _same((info["state_flags"] & ST_ACCEPTED) != 0, m.accepted, "accepted anchors")
        seeds = seed_regions(m, q)
        assert len(regs) == len(seeds) and len(set(ids.tolist())) == len(ids)
        for field in ("ref_start", "ref_len", "slength", "parent"):
            _same(regs[field], [getattr(s, field) for s in seeds], field + " of the seed regions")
        for s, eid in zip(seeds, ids):
            s.eid = int(eid)
        seeds = seeds[rotate:] + seeds[:rotate]
        side = EngineSide(st, m, case.startswith("collinear"))
        side.seen_ids = set(int(x) for x in ids)
        side.null_done_at, side.null_expect = null_done_at, null_expect
        r.left = None
        try:
            r.generations = run_generations(side, seeds, q, two_stage=two_stage, coarse=coarse, stop_after=stop_after)
        except RouteLeft as e:
            r.left = str(e)
        r.side, r.model, r.calls, r.trace = side, m, side.calls, side.trace
        r.trouble = side.calls[-1]["trouble"] if side.calls else 0
        r.finished = r.left is None and stop_after is None and r.trouble == 0
        r.order = st.order_check() if r.finished else None
        r.layout = st.layout()
        if r.finished:
            lay = m.layout()
            r.script = ["CASE %s %d %d %d %d %s" % (case, len(seqs), ams, q, len(knobs), _words("%s %d" % kv for kv in knobs.items()))] + [s.decode() for s in seqs] + \
                       ["SEEDS %d" % len(regs)] + side.script + ["END %d %s" % (r.order, _words("%d %d" % (int(x.sum()), int(np.flatnonzero(x).sum())) for x in lay))]
        if then:
            then(st, side, r)
    return r


def same_end_state(run, ref, what):
    """every row's (accepted, shift, len), the layout and the set of processed regions against do_work()"""
    got, want = run.model.by_region(), ref.work.by_region()
    assert set(got) == set(want), "%s: %d regions processed that the work list never holds, %d of the work list's missing" % (what, len(set(got) - set(want)), len(set(want) - set(got)))
    for rows, verdicts in want.items():
        assert got[rows] == verdicts, "%s: region %d+%d: (accepted, shift, len) per candidate %s, the work list gives %s" % (what, rows[0][0], rows[0][1], got[rows], verdicts)
    T.same_layout(run.layout, ref.work.layout(), what + ": the layout at the end")


def write_cases(path, runs):
    """the calls of finished runs as a text file for tests/emu/gen_calls_check.cpp: per case the sequences, every pm_store_search and
    pm_store_validate list as the former made it; from the restatement the children in listed order, (state, shift, len, start0) of
    every row of the listed regions and the layout's marks per genome at the end; from this run of the engine, checked above against
    the restatement's properties, the offsets, done[], trouble and second_stage_ran"""
    with open(path, "w") as f:
        for r in runs:
            f.write("\n".join(r.script) + "\n")
