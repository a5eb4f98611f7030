"""The candidate side of a search call (include/parsnp_mum.h: pm_multi_mum_batch), from the sorted events to the rows a caller receives
-- Master.EP, the candidate listing, the fold over the genomes, the compaction into (sp, fwd) or MUM rows, the overlap flags of a long
one-region list and the grouped downloads: a ctypes driver over a `binding.Lib`, a sequential restatement, and a seeded generator of the
smallest sets that put something on each lane, group, block and round edge of those kernels.

Plain Python and numpy, no engine code.  The restatement takes the (k, lon, sp, fwd) of `oracles.restatement_multi_mum` per region,
the request rows and the genome lengths and derives what the second half of setMums1 derives per candidate (src/parsnp.cpp:1717-1781,
the TMum constructor src/TMum.cpp:25-60) and what the sequential walk of the anchor validation (host/aligner.cpp: validate_parallel)
finds: a running maximum end and a running minimum start per genome, kept as Python integers."""
import ctypes as C

import numpy as np

import oracles
import storecalls as S
from parsnp_amd.binding import Session

ROW_BAD, ROW_OUTSIDE, ROW_REVERSE, ROW_DIRTY, ROW_EARLY = S.ROW_BAD, S.ROW_OUTSIDE, S.ROW_REVERSE, S.ROW_DIRTY, S.ROW_EARLY
DIRTY_BLOCK = 256      # rows per wavefront of the overlap test (kernels.h: kDirtyBlock; test_generator_matches_the_source)
MARK_ROUND = 8         # rows in flight in one round of DirtyMark
PREFIX_ROUND = 16      # blocks in flight in one round of DirtyPrefix
LANES = 64
COPY_PIECE = 65536     # bytes of one download that one workgroup of the grouped copy takes


# ---------------------------------------------------------------------------------------------------------------- driver
def _declare(L):
    S.declare(L)
    P = C.POINTER
    L.pm_result_start.restype, L.pm_result_start.argtypes = P(C.c_int32), [C.c_void_p]
    L.pm_result_strand.restype, L.pm_result_strand.argtypes = P(C.c_uint8), [C.c_void_p]
    L.pm_result_dirty_known.restype, L.pm_result_dirty_known.argtypes = C.c_int, [C.c_void_p]


class Call:
    """what one pm_multi_mum_batch gave: per region the offsets, per candidate k / lon and either (sp, fwd) or the MUM row"""
    pass


class RowSession:
    """binding.Session plus what it lacks: pm_session_rows and the accessors of MUM-row mode.  mode 0: (sp, fwd); 1: rows to the host;
    2: resident (the rows of an anchor call stay in the store and come back through pm_store_rows(raw = 1), as storecalls.Store reads them)"""

    def __init__(self, lib, seqs, mode, tune=None):
        self.lib, self.L = lib, lib.L
        _declare(self.L)
        self.sess = Session(lib, seqs)
        self.h, self.n, self.mode = self.sess.h, len(seqs), mode
        self.kept = []
        try:
            for k, v in (tune or {}).items():
                lib._check(self.L.pm_session_tune(self.h, k.encode(), v))
            lib._check(self.L.pm_session_rows(self.h, mode))
        except BaseException:
            self.close()
            raise

    def close(self):
        for r in self.kept:
            self.L.pm_result_free(r)
        self.kept = []
        self.sess.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def call(self, starts, lens, minsize):
        L, n = self.L, self.n
        starts, lens = np.ascontiguousarray(starts, np.int64), np.ascontiguousarray(lens, np.int64)
        minsize = np.ascontiguousarray(minsize, np.int32)
        nreg = starts.shape[0]
        assert starts.shape == (nreg, n) == lens.shape and minsize.shape == (nreg,)
        res = C.c_void_p()
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
        self.lib._check(L.pm_multi_mum_batch(self.h, nreg, p(starts, C.c_int64), p(lens, C.c_int64), p(minsize, C.c_int32), C.byref(res)))
        self.kept.append(res)
        o = Call()
        o.timing = dict(self.sess.last_timing())
        o.total = t = int(L.pm_result_total(res))
        o.off = np.ctypeslib.as_array(L.pm_result_offsets(res), (nreg + 1,)).copy()
        take = lambda ptr, shape, dt: (np.ctypeslib.as_array(ptr, (int(np.prod(shape)),)).copy().reshape(shape) if t else np.zeros(shape, dt))   # noqa: E731
        o.k = take(L.pm_result_k(res), (t,), np.int32)
        o.lon = take(L.pm_result_lon(res), (t,), np.int32)
        o.dirty_known = int(L.pm_result_dirty_known(res))
        o.table_id = int(L.pm_result_table_id(res))
        o.store_base = int(L.pm_result_store_base(res))
        if self.mode == 0:
            o.sp = take(L.pm_result_sp(res), (t, n - 1), np.int32)
            o.fwd = take(L.pm_result_fwd(res), (t, n - 1), np.uint8)
            return o
        assert not L.pm_result_sp(res) and not L.pm_result_fwd(res), "sp / fwd of a result in MUM-row mode are not NULL"
        o.flags = take(L.pm_result_flags(res), (t,), np.uint32)
        if t and not L.pm_result_start(res):
            assert self.mode == 2 and o.table_id != 0 and o.store_base == 0 and not L.pm_result_strand(res), "no rows in a result that left no table"
            o.start, o.strand = np.zeros((t, n), np.int32), np.zeros((t, n), np.uint8)
            self.lib._check(L.pm_store_rows(self.h, None, 0, t, 1, S._ptr(o.start), S._ptr(o.strand)))
        else:
            o.start = take(L.pm_result_start(res), (t, n), np.int32)
            o.strand = take(L.pm_result_strand(res), (t, n), np.uint8)
        return o


# ---------------------------------------------------------------------------------------------------------------- restatement
_lib = None


def checker():
    global _lib
    if _lib is None:
        _lib = oracles.load_restatement()
    return _lib


def region_mums(seqs, starts, lens, minsize, want_master=False):
    """oracles.restatement_multi_mum on the substrings of one request row (a region without reference bases has no candidate)"""
    if lens[0] == 0:
        z = (np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros((0, len(seqs) - 1), np.int64), np.zeros((0, len(seqs) - 1), np.uint8))
        return z + ((np.zeros(0, np.int32), np.zeros(0, np.int32)) if want_master else ())
    sub = [seqs[j][int(starts[j]): int(starts[j]) + int(lens[j])] for j in range(len(seqs))]
    return oracles.restatement_multi_mum(checker(), sub, int(minsize), want_master=want_master)


def listed_candidates(master_ep, minsize):
    """the positions the extraction loop looks at BEFORE the fold's UP < EP test (parsnp.cpp:1657-1663): Master.EP rises, and reaches
    minsize bases or more"""
    prev, out = 0, []
    for k, e in enumerate(int(x) for x in master_ep):
        if e > prev and e - k >= minsize:
            out.append(k)
        prev = e
    return out


def rows_of(mums, wstart, wlen, glen):
    """(k, lon, sp, fwd) of one region -> (start[c][j], strand[c][j], flags[c]) as the TMum constructor derives them; Python integers"""
    k, lon, sp, fwd = mums
    n = len(glen)
    start, strand, flags = [], [], []
    for c in range(len(k)):
        ln, st, sd, f = int(lon[c]), [], [], 0
        for j in range(n):
            q = int(k[c]) if j == 0 else int(sp[c][j - 1])
            fw = 1 if j == 0 else int(fwd[c][j - 1])
            if q + 1 > int(wlen[j]):      # DSP[j] - r1.start[j] > length[j] (:1723), DSP one-based
                f |= ROW_BAD
            at = q + int(wstart[j])
            s = at if fw else int(glen[j]) - (at + ln)      # TMum.cpp:33-35: flipped against the whole genome
            if not fw:
                f |= ROW_REVERSE
            if s + ln > int(glen[j]) or s < 0:              # TMum.cpp:47-56
                f |= ROW_OUTSIDE
            st.append(s)
            sd.append(fw)
        start.append(st)
        strand.append(sd)
        flags.append(f)
    return start, strand, flags


class Walk:
    """the sequential walk of the cheap overlap test: per genome a running maximum end from -1 and a running minimum start from
    +infinity; a row that marks nothing (BAD, OUTSIDE, shorter than `shortest`) takes no part.  Besides the bits it records which
    genomes decide each row and where an equality decides, for the floors"""

    def __init__(self, start, lon, flags, shortest=5):
        n = len(start[0]) if start else 0
        inf = float("inf")
        maxend, minstart = [-1] * n, [inf] * n
        self.bits, self.early_in, self.dirty_in = [], [], []
        self.eq = dict(a_eq_maxend=[], a_eq_maxend_m1=[], b_eq_minstart=[], b_eq_minstart_p1=[])      # rows, with the genome
        for c in range(len(start)):
            ln, ein, din = int(lon[c]), [], []
            if not (flags[c] & (ROW_BAD | ROW_OUTSIDE)) and ln >= shortest:
                for j in range(n):
                    a = int(start[c][j])
                    b = a + ln
                    early = not (a >= maxend[j])
                    dirty = early and not (b <= minstart[j])
                    if a == maxend[j]:
                        self.eq["a_eq_maxend"].append((c, j))
                    if a == maxend[j] - 1 and dirty:
                        self.eq["a_eq_maxend_m1"].append((c, j))
                    if early and b == minstart[j]:
                        self.eq["b_eq_minstart"].append((c, j))
                    if early and b == minstart[j] + 1:
                        self.eq["b_eq_minstart_p1"].append((c, j))
                    if early:
                        ein.append(j)
                    if dirty:
                        din.append(j)
                    if b > maxend[j]:
                        maxend[j] = b
                    if a < minstart[j]:
                        minstart[j] = a
            self.bits.append((ROW_EARLY if ein else 0) | (ROW_DIRTY if din else 0))
            self.early_in.append(ein)
            self.dirty_in.append(din)


class Expect:
    """what the reference's code gives for one call: per region the candidates, and in row mode rows and flags"""

    def __init__(self, seqs, starts, lens, minsize, dirty_min, rows=True):
        n, glen = len(seqs), [len(s) for s in seqs]
        self.off, self.k, self.lon, self.sp, self.fwd = [0], [], [], [], []
        self.start, self.strand, self.flags = [], [], []
        for r in range(len(starts)):
            m = region_mums(seqs, starts[r], lens[r], minsize[r])
            self.k += [int(x) for x in m[0]]
            self.lon += [int(x) for x in m[1]]
            self.sp += [[int(x) for x in row] for row in m[2]]
            self.fwd += [[int(x) for x in row] for row in m[3]]
            st, sd, fl = rows_of(m, starts[r], lens[r], glen)
            self.start += st
            self.strand += sd
            self.flags += fl
            self.off.append(len(self.k))
        self.total = len(self.k)
        self.walk = None
        self.long_list = rows and len(starts) == 1 and self.total >= dirty_min
        if self.long_list:
            self.walk = Walk(self.start, self.lon, self.flags)
            self.flags = [f | b for f, b in zip(self.flags, self.walk.bits)]


def compare(what, got, want, mode):
    """-> None, or the first difference as (what, row, genome, want, got)"""
    if list(got.off) != want.off:
        return (what, "offsets", None, want.off, list(got.off))
    for c in range(want.total):
        if (int(got.k[c]), int(got.lon[c])) != (want.k[c], want.lon[c]):
            return (what, c, None, (want.k[c], want.lon[c]), (int(got.k[c]), int(got.lon[c])))
        if mode == 0:
            for g in range(len(want.sp[c])):
                if (int(got.sp[c][g]), int(got.fwd[c][g])) != (want.sp[c][g], want.fwd[c][g]):
                    return (what, c, g + 1, (want.sp[c][g], want.fwd[c][g]), (int(got.sp[c][g]), int(got.fwd[c][g])))
            continue
        for j in range(len(want.start[c])):
            if (int(got.start[c][j]), int(got.strand[c][j])) != (want.start[c][j], want.strand[c][j]):
                return (what, c, j, (want.start[c][j], want.strand[c][j]), (int(got.start[c][j]), int(got.strand[c][j])))
        if int(got.flags[c]) != want.flags[c]:
            j = (want.walk.early_in[c] + want.walk.dirty_in[c] + [None])[0] if want.walk else None
            return (what, c, j, "flags %d" % want.flags[c], "flags %d" % int(got.flags[c]))
    if mode:
        if got.dirty_known != int(want.long_list) or (got.table_id != 0) != want.long_list:
            return (what, "dirty_known / table", None, int(want.long_list), (got.dirty_known, got.table_id))
    return None


# ---------------------------------------------------------------------------------------------------------------- generator
_BASES = np.frombuffer(b"ACGT", np.uint8)
_cache = {}


def _other(rng, b):
    return (int(b) + 1 + int(rng.integers(0, 3))) % 4


def _text(a):
    return _BASES[np.asarray(a, np.int8)].tobytes()


def _rc(a):
    return (3 - np.asarray(a, np.int8))[::-1]


def whole(seqs):
    glen = np.array([[len(s) for s in seqs]], np.int64)
    return np.zeros_like(glen), glen


# ------------------------------------------------------------------------------------------------ 4. overlap flags of a long list
def flag_set(seed, n, rows, spacing, minsize, deletions=(), move=None, insertions=()):
    """n sequences whose anchor list has exactly `rows` rows, in list order: every query differs from the reference at the last base
    of every stretch of `spacing` bases (all at the same places), so that row i is reference [spacing i, spacing i + spacing - 1)
    in every genome; the last stretch runs to the end.

    deletions: (genome, b) -- the substitution between stretch b - 1 and b is left out, the two reference bases there are made equal
    (with different neighbours) and genome g loses the second: row b - 1 ends behind the first of the two in every genome, row b
    begins ON it in genome g (a == maxend - 1: early and dirty) and right behind it everywhere else (a == maxend: not early).
    insertions: (genome, b) -- the substitution between stretch b - 1 and b is left out and genome g holds one base more there: row b
    begins exactly where row b - 1 ends in every other genome (a == maxend) and is early in none.
    move: (genome, first, overlap) -- the stretches from `first` on move to the very start of genome g: every row of them starts
    before the end of the rows listed before it (early); the first of them ends exactly where row 0 begins when it is the only one
    (b == minstart: not dirty); overlap: the reference's last base is made equal to its first and the genome holds it once, so that
    row ends ON row 0's first base (b == minstart + 1: dirty).

    Chance matches of minsize bases (hundreds in 57 kb at minsize 12) would put rows anywhere and make every later row early and
    dirty, so the reference is repaired until the restatement lists the designed rows and no other: a base inside every row too
    many or too few is drawn again."""
    rng = np.random.default_rng(seed)
    length = rows * spacing
    ref = rng.integers(0, 4, length).astype(np.int8)
    off = rng.integers(1, 4, length).astype(np.int8)      # what a query adds to the reference's base where it differs
    cuts = {b: g for g, b in deletions}
    joins = {b: g for g, b in insertions}
    assert not set(cuts) & set(joins)
    fixed = np.zeros(length, bool)
    fixed[[0, length - 1, length - 2]] = True
    for b in cuts:
        fixed[spacing * b - 2: spacing * b + 2] = True
    designed = set()
    for i in range(rows):
        designed.add((spacing * i, spacing if i == rows - 1 or i + 1 in cuts or i + 1 in joins else spacing - 1))

    def constrain():
        for b in cuts:
            p = spacing * b - 1
            ref[p + 1] = ref[p]
            for x in (p - 1, p + 2):
                if ref[x] == ref[p]:
                    ref[x] = (ref[p] + 1) % 4
        if move and move[2]:
            ref[length - 1] = ref[0]
            if ref[length - 2] == ref[length - 1]:
                ref[length - 2] = (ref[length - 1] + 1) % 4

    def derive():
        seqs = [_text(ref)]
        for g in range(1, n):
            a = ref.copy()
            for i in range(1, rows):
                if i not in cuts and i not in joins:
                    a[spacing * i - 1] = (a[spacing * i - 1] + off[spacing * i - 1]) % 4
            if move and move[0] == g:
                assert g not in cuts.values() and g not in joins.values(), "a genome is moved or changes its length, not both"
                lo = spacing * move[1]
                a = np.concatenate([a[lo: length - (1 if move[2] else 0)], a[:lo]])
            for b, gg in sorted(list(cuts.items()) + list(joins.items()), reverse=True):
                if gg == g and b in cuts:
                    a = np.delete(a, spacing * b)
                elif gg == g:      # a base that is neither of its neighbours: neither row grows by it
                    a = np.insert(a, spacing * b, next(x for x in range(4) if x not in (a[spacing * b - 1], a[spacing * b])))
            seqs.append(_text(a))
        return seqs

    for _ in range(60):
        constrain()
        seqs = derive()
        m = region_mums(seqs, [0] * n, [len(s) for s in seqs], minsize)
        got = list(zip((int(x) for x in m[0]), (int(x) for x in m[1])))
        wrong = designed.symmetric_difference(got) | {got[c] for c in range(len(got)) if not m[3][c].all()}      # (an equal reach on the reverse strand wins the tie)
        if not wrong and len(got) == len(designed):
            return seqs
        for k, lon in sorted(wrong):
            free = [x for x in range(k, min(k + lon, length)) if not fixed[x]]
            x = free[int(rng.integers(0, len(free)))]
            ref[x] = _other(rng, ref[x])
    raise AssertionError("the designed rows could not be reached")


# name -> (seed, genomes, rows, spacing, minsize, deletions, move, insertions): the rows are asserted from the restatement (test_floors)
FLAG_CASES = {
    # list lengths around dirty_min (the three relations are three tunes of the test), a pair inside a block and at rows 7 / 8
    "short40": (11, 5, 40, 20, 16, ((2, 8), (4, 30)), (1, 39, False), ((3, 20),)),
    # rows per block: the last block full, one row over, a last round of DirtyMark with clamped reads (260), two blocks and one over;
    # the deleted base at rows 7 / 8 and at the last two rows of block 0, or across its end (255 / 256)
    "rows255": (12, 4, 255, 20, 16, ((2, 8), (3, 253)), (1, 254, True), ((3, 100), (2, 248))),
    "rows256": (13, 4, 256, 20, 16, ((2, 8), (3, 254)), (1, 255, False), ((3, 100), (2, 250))),
    "rows257": (14, 4, 257, 20, 16, ((2, 8), (3, 256)), (1, 250, True), ((3, 100), (2, 248))),
    "rows260": (15, 4, 260, 20, 16, ((2, 8), (3, 256)), (1, 257, False), ((3, 100), (2, 255))),
    "rows512": (16, 4, 512, 20, 16, ((2, 256), (3, 510)), (1, 511, False), ((3, 100), (2, 505))),
    "rows513": (17, 4, 513, 20, 16, ((2, 256), (3, 511)), (1, 512, True), ((3, 100), (2, 500))),
    # DirtyPrefix's rounds of 16 blocks: 16 blocks, and a 17th of one row that row 0 (block 0, sixteen blocks before it) decides
    "rows4096": (18, 4, 4096, 14, 12, ((2, 8), (3, 4094), (2, 2304)), (1, 4095, False), ((3, 100), (2, 4000))),
    "rows4097": (19, 4, 4097, 14, 12, ((2, 8), (3, 2048)), (1, 4096, True), ((3, 100), (2, 4090))),
    # the deciding genome in column 1, 63 and 64 (the last of 65) -- strand bytes of 257 x 65 (no multiple of 4), starts of 300 x 65 x 4
    # (more than one piece of a grouped download); row 270 is early in genome 2 alone and dirty in genome 64 alone
    "g65_257": (20, 65, 257, 20, 16, ((1, 8), (63, 100), (64, 253)), (2, 256, False), ((1, 50), (64, 60))),
    "g65_300": (21, 65, 300, 20, 16, ((1, 8), (63, 100), (64, 200), (64, 270)), (2, 270, False), ((1, 50), (64, 60))),
    # ... and in column 1, 63, 64, 65 and 129 of 130: row 280 is early in genome 2 (group 0) and dirty in genome 70 (group 1)
    "g130_300": (22, 130, 300, 20, 16, ((1, 8), (63, 100), (64, 150), (65, 200), (129, 250), (70, 280), (128, 290)), (2, 280, False), ((1, 50), (64, 60), (129, 70))),
}


def flag_case(name):
    if ("flag", name) not in _cache:
        seed, n, rows, spacing, minsize, dels, move, ins = FLAG_CASES[name]
        _cache["flag", name] = (flag_set(seed, n, rows, spacing, minsize, dels, move, ins), minsize)
    return _cache["flag", name]


def flag_floors(name, want):
    """what the case is for, from the restatement's rows alone -> dict of counts (asserted in test_floors)"""
    n = FLAG_CASES[name][1]
    w = want.walk
    bits = w.bits
    both = [c for c, b in enumerate(bits) if b == ROW_EARLY | ROW_DIRTY]
    group = lambda js: {j // LANES for j in js}   # noqa: E731
    out = dict(rows=want.total, early_only=sum(1 for b in bits if b == ROW_EARLY), early_dirty=len(both))
    out["clean_beside"] = sum(1 for c, b in enumerate(bits) if b == 0 and ((c > 0 and bits[c - 1]) or (c + 1 < len(bits) and bits[c + 1])))
    for k, v in w.eq.items():
        out[k] = len(v)
    out["a_eq_maxend_clean"] = len({c for c, j in w.eq["a_eq_maxend"] if not bits[c]})      # (rows that begin ON an earlier row's end and are early nowhere)
    out["deciding_columns"] = sorted({j for c in both for j in w.dirty_in[c]})
    out["past_first_group_only"] = sum(1 for c in range(len(bits)) if bits[c] and min(w.early_in[c]) >= LANES)
    out["early_here_dirty_there"] = sum(1 for c in both if group(set(w.early_in[c]) - set(w.dirty_in[c])) - group(w.dirty_in[c]))
    out["pair_at_round_end"] = sum(1 for c, j in w.eq["a_eq_maxend_m1"] if (c - 1) % MARK_ROUND == MARK_ROUND - 1)
    out["pair_across_blocks"] = sum(1 for c, j in w.eq["a_eq_maxend_m1"] if c % DIRTY_BLOCK == 0)
    out["pair_inside_block"] = sum(1 for c, j in w.eq["a_eq_maxend_m1"] if c % DIRTY_BLOCK)
    out["decided_blocks_away"] = max([c // DIRTY_BLOCK for c, j in w.eq["b_eq_minstart"] + w.eq["b_eq_minstart_p1"]] + [0])      # (row 0, block 0, holds the minimum start)
    tail = want.total % MARK_ROUND
    out["last_round_rows"] = tail      # (0: the last round is a full one)
    out["flagged_in_last_round"] = sum(1 for c in range(want.total - (tail or MARK_ROUND), want.total) if bits[c])
    out["strand_bytes"] = want.total * n
    out["start_bytes"] = 4 * want.total * n
    return out


def short_rows_set(seed):
    """three short sequences at minsize 4 whose list holds rows of 4 and of 5 bases among longer ones: a reference of 90 bases,
    queries with a substitution every 5 to 12 bases and the last third of one query moved to its start"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, 90).astype(np.int8)
    seqs = [_text(ref)]
    for g in (1, 2):
        a = ref.copy()
        x = int(rng.integers(3, 9))
        while x < 88:
            a[x] = _other(rng, a[x])
            x += int(rng.integers(5, 13))
        if g == 2:
            a = np.concatenate([a[60:], a[:60]])
        seqs.append(_text(a))
    return seqs, 4


SHORT_ROWS_SEED = 0      # the first seed at which every floor of short_rows_floors() is reached (find_short_rows_seed)


def short_rows_floors(want):
    """-> (rows of 4 bases, rows of 5 bases, rows of 5 bases or more whose bits would change if the rows of 4 bases took part in the walk,
    rows whose bits would change if the rows of 5 bases did not)"""
    base = [f & ~(ROW_EARLY | ROW_DIRTY) for f in want.flags]
    four, six = Walk(want.start, want.lon, base, 4).bits, Walk(want.start, want.lon, base, 6).bits
    five = want.walk.bits
    return (sum(1 for x in want.lon if x == 4), sum(1 for x in want.lon if x == 5),
            sum(1 for c in range(want.total) if want.lon[c] >= 5 and four[c] != five[c]), sum(1 for c in range(want.total) if six[c] != five[c]))


def find_short_rows_seed(limit=20000):
    for seed in range(limit):
        seqs, ms = short_rows_set(seed)
        st, ln = whole(seqs)
        want = Expect(seqs, st, ln, [ms], 2)
        if want.long_list and all(x >= 1 for x in short_rows_floors(want)) and not any(f & (ROW_BAD | ROW_OUTSIDE) for f in want.flags):
            return seed
    return None


# ------------------------------------------------------------------------------------------------ 1. genome-group edges of the fold
FOLD_QUERIES = (1, 63, 64, 65, 127, 128, 129, 193)
FOLD_MINSIZE = 12
_SITE = 40      # bases of a designed site: the candidate at its first base, a substitution of every query at base 38


def fold_sites(nq):
    """the designed sites of a set of nq queries (query index 0 .. nq - 1 = genome 1 .. nq): (kind, short, duals, up) --
    short: (query, a) that query differs at base a of the site (the shortest reach); duals: (query, f, r) -- that query holds the
    reverse complement of the site's first r bases as well (reach k + r on the reverse strand) and differs at base f (None: not before
    base 38); up: the query whose event starts ON the site's first base, inside a 20-base repeat of the reference"""
    last = nq - 1
    sites = []
    for p in (0, 62, 63, 64, 65, 127, 128, last):
        if p < nq and not any(s[1] and s[1][0] == p and s[0] == "short" for s in sites):
            duals = [(j, None, 20) for j in sorted({last, p - 1}) if j >= 0 and j != p]      # behind the short one: clipped; before it: forward
            sites.append(("short", (p, 13), duals, None))
    for t in (63, 64):
        if t < nq:
            sites.append(("tie", None, [(t, 18, 18)], None))
    if nq > 10:
        sites.append(("clip", (3, 13), [(10, None, 16)], None))      # the earlier genome in the same 64-group
    if nq > 70:
        sites.append(("clip", (10, 13), [(70, None, 16)], None))     # ... and in the group before
    for u in sorted({64, last}):
        if 0 < u < nq:
            sites.append(("up", (0, 14), [], u))
    return sites


def fold_set(nq):
    """a reference of about 600 bases (no multiple of 4) and nq queries that are copies of it with the substitutions and reverse
    copies of fold_sites(nq)"""
    if ("fold", nq) in _cache:
        return _cache["fold", nq]
    rng = np.random.default_rng(5000 + nq)
    sites = fold_sites(nq)
    nup = sum(1 for s in sites if s[0] == "up")
    length = max(21 + _SITE * len(sites) + 30 * nup + 14, 601)      # (the sets with few sites end in a stretch that every query copies)
    length += 1 if length % 4 == 0 else 0
    ref = rng.integers(0, 4, length).astype(np.int8)
    zone = 21 + _SITE * len(sites)
    ups = 0
    for s, (kind, short, duals, up) in enumerate(sites):
        k = 21 + _SITE * s
        if kind == "up":      # the site's first 20 bases a second time behind the sites, with other neighbours on both sides
            z = zone + 30 * ups + 5
            ups += 1
            ref[z: z + 20] = ref[k: k + 20]
            for x, y in ((z - 1, k - 1), (z + 20, k + 20)):
                if ref[x] == ref[y]:
                    ref[x] = (ref[y] + 1) % 4
    body = [ref.copy() for _ in range(nq)]
    tails = [[] for _ in range(nq)]
    for s, (kind, short, duals, up) in enumerate(sites):
        k = 21 + _SITE * s
        for g in range(nq):
            body[g][k + 38] = (ref[k + 38] + 1 + (g + s) % 3) % 4
            if kind != "up" or g == up:
                body[g][k - 1] = (ref[k - 1] + 1 + (g + s) % 3) % 4
        if short:
            body[short[0]][k + short[1]] = (ref[k + short[1]] + 2) % 4
        for j, f, r in duals:
            if f is not None:
                body[j][k + f] = (ref[k + f] + 2) % 4
            piece = np.concatenate([[(ref[k - 1] + 2) % 4], ref[k: k + r], [(ref[k + r] + 2) % 4]]).astype(np.int8)
            tails[j].append(_rc(piece))
    seqs = [_text(ref)] + [_text(np.concatenate([body[g]] + tails[g])) for g in range(nq)]
    _cache["fold", nq] = seqs
    return seqs


def per_genome_reach(seqs, minsize):
    """per query genome the propagated (EP, UP) of both strands at every reference position (oracles.restatement_find_um)"""
    key = ("reach", id(seqs), minsize)
    if key not in _cache:
        out = []
        for q in seqs[1:]:
            uf, ef, _ = oracles.restatement_find_um(checker(), seqs[0], q, minsize, propagate=True)
            ur, er, _ = oracles.restatement_find_um(checker(), seqs[0], oracles.revcomp(q), minsize, propagate=True)
            out.append((ef, er, uf, ur))
        _cache[key] = (seqs, out)
    return _cache[key][1]


def fold_floors(seqs, minsize):
    """by the per-genome reaches at the accepted and the listed candidates: which query alone has the shortest reach, ties of the two
    strands (lane 63 / lane 0 of a group), choices that an earlier genome's reach clips to reverse (same group / the group before), and
    candidates that only UP >= EP rejects, with the query that holds the largest UP"""
    nq = len(seqs) - 1
    reach = per_genome_reach(seqs, minsize)
    m = region_mums(seqs, [0] * len(seqs), [len(s) for s in seqs], minsize, want_master=True)
    accepted, (mu, me) = {int(x) for x in m[0]}, m[4:6]
    listed = listed_candidates(me, minsize)
    out = dict(listed=len(listed), accepted=len(accepted), shortest=set(), ties=set(), clipped_same=0, clipped_before=0, up_alone=set())
    for k in listed:
        tops = [max(int(r[0][k]), int(r[1][k])) for r in reach]
        low = min(tops)
        if k in accepted and tops.count(low) == 1:
            out["shortest"].add(tops.index(low))
        before = len(seqs[0])
        for g, r in enumerate(reach):
            ef, er = int(r[0][k]), int(r[1][k])
            if k in accepted and ef == er and er - k >= minsize and before > er:
                out["ties"].add(g)
            if k in accepted and ef > er and before <= er and er - k >= minsize:
                who = next(x for x in range(g) if tops[x] == before)
                out["clipped_same" if who // LANES == g // LANES else "clipped_before"] += 1
            before = min(before, tops[g])
        if k not in accepted:      # listed: Master.EP rises and is long enough; so UP >= EP alone rejects it
            assert int(mu[k]) >= int(me[k])
            ups = [int(r[2][k]) if int(r[0][k]) > int(r[1][k]) else int(r[3][k]) for r in reach]
            big = [g for g in range(nq) if ups[g] >= int(me[k])]
            if len(big) == 1:
                out["up_alone"].add(big[0])
    return out


def count_set(subs):
    """one query that differs from a reference of 40 (subs + 1) bases at `subs` places: subs + 1 candidates before the fold"""
    rng = np.random.default_rng(7000 + subs)
    ref = rng.integers(0, 4, 40 * (subs + 1) + 1).astype(np.int8)
    q = ref.copy()
    for i in range(1, subs + 1):
        q[40 * i - 1] = (q[40 * i - 1] + 1) % 4
    return [_text(ref), _text(q)]


# ------------------------------------------------------------------------------------------------ 2. chunk edges of Master.EP
CHUNK = 256
CHUNK_MINSIZE = 12
CHUNK_STARTS = ((255, 511), (256, 512), (257,))      # event starts of one set (a substitution of the queries one base before)
CHUNK_TAILS = (0, 1, 3)


def chunk_set(starts, tail, late):
    """a reference of 3 x 256 + tail bases and four or five queries: queries 0, 2 and 3 differ from it one base before each of `starts`
    (and every 64 bases besides); query 1 differs at base 100 alone -- no event of its starts in the middle chunk or the last; late:
    a fifth query whose first 300 bases are unrelated -- no event before the second chunk, its carry-in there is 0"""
    key = ("chunk", starts, tail, late)
    if key in _cache:
        return _cache[key]
    length = 3 * CHUNK + tail
    for attempt in range(100):      # (the first seed without a chance event of minsize bases in the queries that are to have none)
        rng = np.random.default_rng(8000 + 10 * starts[0] + tail + (100 if late else 0) + 1000 * attempt)
        ref = rng.integers(0, 4, length).astype(np.int8)
        qs = []
        for g in range(5 if late else 4):
            a = ref.copy()
            if g == 1:
                a[100] = (a[100] + 1) % 4
            elif g == 4:
                a[:300] = rng.integers(0, 4, 300)
                a[299] = (ref[299] + 1) % 4
            else:
                for x in [s - 1 for s in starts] + [30, 94, 158, 222, 330, 394, 458, 586, 650, 714]:
                    a[x] = (ref[x] + 1 + g % 3) % 4
            qs.append(_text(a))
        seqs = [_text(ref)] + qs
        ev = events_of(seqs, CHUNK_MINSIZE)
        if sorted(ev[1]) == [0, 101] and (not late or min(ev[4]) >= 300):
            break
    else:
        raise AssertionError("no seed for the chunk set")
    _cache[key] = seqs
    return _cache[key]


def events_of(seqs, minsize):
    """per query genome: the reference starts of the restatement's events of both strands"""
    out = []
    for q in seqs[1:]:
        l1 = oracles.restatement_events(checker(), seqs[0], q, minsize)[1]
        l2 = oracles.restatement_events(checker(), seqs[0], oracles.revcomp(q), minsize)[1]
        out.append([int(x) for x in l1] + [int(x) for x in l2])
    return out


STAGE_MINSIZE = 6
STAGE_CAP = 2048      # kernels.h: kEpCap (test_generator_matches_the_source)


def staging_set():
    """70 queries over a reference of 768 bases at minsize 6: the first 64 (one group of MasterEP's staging) differ from it about
    every seventh base inside the middle chunk, each at places of its own -- more than 2 048 events of that chunk in the group; the
    last 6 differ every 40 bases"""
    if "staging" in _cache:
        return _cache["staging"]
    rng = np.random.default_rng(8800)
    ref = rng.integers(0, 4, 3 * CHUNK).astype(np.int8)
    qs = []
    for g in range(70):
        a = ref.copy()
        if g < 64:
            x = CHUNK - 7 + int(rng.integers(0, 3))
            while x < 2 * CHUNK + 7:
                a[x] = _other(rng, a[x])
                x += 7
            for x in (40, 120, 200, 560, 640, 720):
                a[x] = _other(rng, a[x])
        else:
            for x in range(20 + g, 3 * CHUNK, 40):
                a[x] = _other(rng, a[x])
        qs.append(_text(a))
    _cache["staging"] = [_text(ref)] + qs
    return _cache["staging"]


# ------------------------------------------------------------------------------------------------ 3. candidate listing in batches
BATCH_MINSIZE = 12


def batch_set():
    """-> (seqs, starts[7][4], lens[7][4], minsize[7]): a reference of 520 bases and three queries -- 20 and 7 unrelated bases before a
    copy, and the reverse complement of a copy between 11 and 5 unrelated bases -- that differ from it at base 324; seven regions as
    windows of the four (none starts at 0; the third query's lie on its reverse strand): reference bases [10, 73), [100, 165), [200, 240),
    an empty one, [300, 360), [400, 440) against unrelated windows of the queries, and [450, 500)"""
    if "batch" in _cache:
        return _cache["batch"]
    rng = np.random.default_rng(9100)
    ref = rng.integers(0, 4, 520).astype(np.int8)
    copy = ref.copy()
    copy[324] = (copy[324] + 1) % 4
    junk = lambda m: rng.integers(0, 4, m).astype(np.int8)   # noqa: E731
    seqs = [_text(ref), _text(np.concatenate([junk(20), copy])), _text(np.concatenate([junk(7), copy])), _text(np.concatenate([junk(11), _rc(copy), junk(5)]))]
    starts, lens = [], []
    for a, ln, shift in ((10, 63, 0), (100, 65, 0), (200, 40, 0), (250, 0, 0), (300, 60, 0), (400, 40, -150), (450, 50, 0)):
        b = a + shift      # (the region without a candidate: the queries' windows lie 150 bases away from the reference's)
        starts.append([a, 20 + b, 7 + b, 11 + 520 - b - ln])
        lens.append([ln] * 4)
    _cache["batch"] = (seqs, np.array(starts, np.int64), np.array(lens, np.int64), np.full(7, BATCH_MINSIZE, np.int32))
    return _cache["batch"]


def batch_floors(want, lens):
    """-> (flat position mod 64 of every candidate -- the regions' reference windows one behind the other, engine_core.h: posbase --,
    regions with candidates, a candidate at l = 0 behind a region whose last candidate ends at its last base, reverse members)"""
    base = np.concatenate([[0], np.cumsum(lens[:, 0])])
    flat, follows = set(), 0
    for r in range(len(lens)):
        for c in range(want.off[r], want.off[r + 1]):
            flat.add(int(base[r] + want.k[c]) % LANES)
            if want.k[c] == 0 and r > 0 and want.off[r] > want.off[r - 1] and want.k[want.off[r] - 1] + want.lon[want.off[r] - 1] == lens[r - 1, 0]:
                follows += 1
    with_c = [want.off[r + 1] > want.off[r] for r in range(len(lens))]
    return flat, with_c, follows, sum(1 for f in want.flags if f & ROW_REVERSE)


# ------------------------------------------------------------------------------------------------ 5. capacities carried over
CAP_MINSIZE = (20, 20, 12)      # the three anchor calls of one session


def capacity_set():
    """four sequences: 30 stretches of 40 bases and 420 of 14, the queries differing from the reference at every stretch's last base --
    at minsize 20 the list holds the long stretches only, at 12 fifteen times as many"""
    if "cap" in _cache:
        return _cache["cap"]
    rng = np.random.default_rng(9300)
    length = 30 * 40 + 420 * 14
    ref = rng.integers(0, 4, length).astype(np.int8)
    marks = [40 * i - 1 for i in range(1, 31)] + [1200 + 14 * i - 1 for i in range(1, 420)]
    seqs = [_text(ref)]
    for g in range(3):
        a = ref.copy()
        for x in marks:
            a[x] = (a[x] + 1 + g) % 4
        seqs.append(_text(a))
    _cache["cap"] = seqs
    return seqs


# ------------------------------------------------------------------------------------------------ the sanitized program's case file
def write_case(f, name, seqs, mode, tune, calls):
    """calls: (starts, lens, minsize, Expect, tail) -- tail: -1 no statement, 0 no tail repeated, 1 at least one"""
    n = len(seqs)
    f.write("CASE %s %d %d %d %s\n" % (name, n, mode, len(tune), " ".join("%s %d" % kv for kv in tune.items())))
    for s in seqs:
        f.write(s.decode() + "\n")
    for starts, lens, minsize, want, tail in calls:
        nreg = len(starts)
        nums = [nreg] + [int(x) for x in np.asarray(starts).ravel()] + [int(x) for x in np.asarray(lens).ravel()] + [int(x) for x in minsize]
        nums += [tail, want.total] + want.off + want.k + want.lon
        if mode == 0:
            nums += [x for row in want.sp for x in row] + [x for row in want.fwd for x in row]
        else:
            nums += [x for row in want.start for x in row] + [x for row in want.strand for x in row] + want.flags + [int(want.long_list)]
        f.write("CALL " + " ".join(str(x) for x in nums) + "\n")
    f.write("END\n")
