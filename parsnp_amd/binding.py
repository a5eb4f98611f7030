"""ctypes binding of the C ABI in include/parsnp_mum.h.

`load(path=None)` opens parsnp_amd/lib/libparsnp_hip.so (the product) by default and raises if it is missing: there is
no CPU fallback on the product side.  Tests pass an explicit path to open their CPU checkers through the same
binding."""
import ctypes as C
import os

import numpy as np

from .paths import HIP_LIB


class PmError(RuntimeError):
    pass


class Lib:
    def __init__(self, path=None):
        path = path or HIP_LIB
        if not os.path.exists(path):
            raise PmError("engine library %s not built (python -c 'import __graft_entry__ as g; g.build()')" % path)
        self.path = path
        L = self.L = C.CDLL(path)
        L.pm_last_error.restype = C.c_char_p
        L.pm_provider.restype = C.c_char_p
        L.pm_session_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]
        L.pm_session_destroy.argtypes = [C.c_void_p]
        L.pm_multi_mum_batch.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_void_p)]
        for name, t in (("pm_result_regions", C.c_int64), ("pm_result_total", C.c_int64), ("pm_result_offsets", C.POINTER(C.c_int64)),
                        ("pm_result_k", C.POINTER(C.c_int32)), ("pm_result_lon", C.POINTER(C.c_int32)),
                        ("pm_result_sp", C.POINTER(C.c_int32)), ("pm_result_fwd", C.POINTER(C.c_uint8))):
            getattr(L, name).restype = t
            getattr(L, name).argtypes = [C.c_void_p]
        L.pm_result_free.argtypes = [C.c_void_p]
        L.pm_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.POINTER(C.c_float)]

    @property
    def provider(self):
        return self.L.pm_provider().decode()

    def gap_limits(self, wide=True):
        """(sequences, bases of a sequence, columns of an alignment) the device gap aligner takes: pm_gap_limits -- wide: those of
        pm_gap_align_groups_wide, else those of pm_gap_align_batch / pm_gap_align_groups"""
        if not hasattr(self.L, "pm_gap_limits"):
            raise PmError("this provider of the ABI has no pm_gap_limits")
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self.L.pm_gap_limits(C.c_int(1 if wide else 0), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def gap_limits_long(self):
        """(sequences, bases of a sequence, columns of an alignment) of the device gap aligner's long form: pm_gap_limits_long, the
        limits of pm_gap_align_groups_long (gaps of a cluster distance d of up to 1 000)"""
        return self._gap_limits_of("pm_gap_limits_long")

    def gap_limits_tall(self):
        """(sequences, bases of a sequence, columns of an alignment) of the device gap aligner's tall form: pm_gap_limits_tall, the
        limits of pm_gap_align_groups_tall (gaps of alignments with more than 512 genomes)"""
        return self._gap_limits_of("pm_gap_limits_tall")

    def gap_limits_long_tall(self):
        """(sequences, bases of a sequence, columns of an alignment) of the device gap aligner's long-tall form: pm_gap_limits_long_tall,
        the limits of pm_gap_align_groups_long_tall (more than 512 genomes and a cluster distance d of up to 1 000 at once)"""
        return self._gap_limits_of("pm_gap_limits_long_tall")

    def group_limits(self, wide=True):
        """(distinct pieces of a region, events of one (piece, strand), query genomes of a batch) of the kernels that find the events of
        small regions once per distinct piece: pm_group_limits -- wide: the wide form's, else the first form's"""
        if not hasattr(self.L, "pm_group_limits"):
            raise PmError("this provider of the ABI has no pm_group_limits")
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self.L.pm_group_limits(C.c_int(1 if wide else 0), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def snp_limits(self):
        """rows a SNP collection takes (Session.core_snps): pm_snp_limits"""
        if not hasattr(self.L, "pm_snp_limits"):
            raise PmError("this provider of the ABI has no pm_snp_limits")
        a = C.c_int()
        self._check(self.L.pm_snp_limits(C.byref(a)))
        return a.value

    def nj_limits(self):
        """rows a neighbour-joining tree takes (Session.nj_tree): pm_nj_limits"""
        if not hasattr(self.L, "pm_nj_limits"):
            raise PmError("this provider of the ABI has no pm_nj_limits")
        a = C.c_int()
        self._check(self.L.pm_nj_limits(C.byref(a)))
        return a.value

    def boot_limits(self):
        """(rows, replicates of a call, largest column weight) of the bootstrap (Session.boot_distances, nj_trees, nj_support):
        pm_boot_limits"""
        return self._gap_limits_of("pm_boot_limits")

    def rec_limits(self):
        """(rows, sites of a window, permutations of a call) of the recombination scan (Session.rec_sites, rec_incompat, rec_test):
        pm_rec_limits"""
        return self._gap_limits_of("pm_rec_limits")

    def ext_limits(self):
        """(rows of a job, longest flank, widest band) of the LCB extension (Session.ext_reach, ext_align): pm_ext_limits"""
        return self._gap_limits_of("pm_ext_limits")

    def _gap_limits_of(self, name):
        if not hasattr(self.L, name):
            raise PmError("this provider of the ABI has no %s" % name)
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(getattr(self.L, name)(C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def _check(self, rc):
        if rc != 0:
            raise PmError("%s (code %d)" % (self.L.pm_last_error().decode(), rc))

    def rccl_unique_id(self) -> bytes:
        ident = (C.c_uint8 * 128)()
        self._check(self.L.pm_rccl_unique_id(ident))
        return bytes(ident)

    def find_events(self, ref: bytes, query: bytes, min_len: int, strand: int = 0):
        cap = len(query) + 16
        j = np.zeros(cap, np.int64); l = np.zeros(cap, np.int64); ln = np.zeros(cap, np.int32); rp = np.zeros(cap, np.int32)
        cnt = C.c_int64()
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        self._check(self.L.pm_find_events(ref, C.c_int64(len(ref)), query, C.c_int64(len(query)), C.c_int32(min_len), C.c_int(strand),
                                          C.c_int64(cap), C.byref(cnt), p(j, C.c_int64), p(l, C.c_int64), p(ln, C.c_int32), p(rp, C.c_int32)))
        c = cnt.value
        return j[:c].copy(), l[:c].copy(), ln[:c].copy(), rp[:c].copy()


class Session:
    """genomes resident on the device; genome 0 is the reference"""

    def __init__(self, lib: Lib, seqs, device=-1, rccl=None):
        """rccl = (rank, world, id bytes): a sharded session whose exchanges run over the engine's own RCCL communicator
        (pm_session_create_rccl); `Lib.rccl_unique_id()` makes the id on rank 0"""
        self.lib = lib
        self.n = len(seqs)
        self._seqs = [bytes(s) for s in seqs]
        arr = (C.c_char_p * self.n)(*self._seqs)
        lens = (C.c_int64 * self.n)(*[len(s) for s in self._seqs])
        h = C.c_void_p()
        if rccl is not None:
            rank, world, ident = rccl
            lib.L.pm_session_create_rccl.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64),
                                                     C.c_int, C.c_int, C.POINTER(C.c_uint8)]
            lib._check(lib.L.pm_session_create_rccl(C.byref(h), device, self.n, arr, lens, rank, world, (C.c_uint8 * 128).from_buffer_copy(ident)))
        else:
            lib._check(lib.L.pm_session_create(C.byref(h), device, self.n, arr, lens))
        self.h = h

    def close(self):
        if self.h:
            self.lib.L.pm_session_destroy(self.h)
            self.h = None

    def tune(self, key: str, value: int):
        """pm_session_tune: "work_budget", "dirty_min", "group_small", "group_wide", ... (include/parsnp_mum.h)"""
        self.lib.L.pm_session_tune.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        self.lib._check(self.lib.L.pm_session_tune(self.h, key.encode(), value))

    def chain_passed(self):
        """pm_store_chain_passed: MUMs in no LCB after the first and the second chaining pass of the last pm_store_chain_end (a
        diagonal difference in bases: pm_store_chain_begin with diag_diff > 1)"""
        if not hasattr(self.lib.L, "pm_store_chain_passed"):
            raise PmError("this provider of the ABI has no pm_store_chain_passed")
        a, b = C.c_int64(), C.c_int64()
        self.lib.L.pm_store_chain_passed.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self.lib._check(self.lib.L.pm_store_chain_passed(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def unaligned_runs(self):
        """pm_store_unalign_count + pm_store_unalign_runs: what parsnp.unalign lists, from the layout on the device -> (runs, all_runs,
        kept_runs): runs[j] = (start, end, ordinal) of the kept runs of genome j (int32 arrays; end inclusive; ordinal among all runs
        of the genome, the one-base runs included), all_runs[j] / kept_runs[j] the counts (int64)"""
        L = self.lib.L
        if not hasattr(L, "pm_store_unalign_count"):
            raise PmError("this provider of the ABI has no pm_store_unalign_count")
        v = C.c_void_p
        L.pm_store_unalign_count.argtypes = [v, v, v]
        L.pm_store_unalign_runs.argtypes = [v, v, v, v, C.c_int64]
        ptr = lambda a: a.ctypes.data_as(v)      # noqa: E731
        all_runs, kept = np.zeros(self.n, np.int64), np.zeros(self.n, np.int64)
        self.lib._check(L.pm_store_unalign_count(self.h, ptr(all_runs), ptr(kept)))
        total = int(kept.sum())
        start, end, ordinal = (np.zeros(total, np.int32) for _ in range(3))
        self.lib._check(L.pm_store_unalign_runs(self.h, ptr(start), ptr(end), ptr(ordinal), total))
        at = np.concatenate([[0], np.cumsum(kept)])
        return [(start[at[j]:at[j + 1]], end[at[j]:at[j + 1]], ordinal[at[j]:at[j + 1]]) for j in range(self.n)], all_runs, kept

    def core_snps(self, chunks, n_rows=None):
        """pm_snp_begin, a pm_snp_add per chunk, pm_snp_columns, pm_snp_distances -> (counts, col, letters, dist).  chunks: uint8
        arrays of shape (n_rows, w), ASCII; a view whose rows lie further apart than w bytes (a slice of a wider array) is handed
        over as it lies, with its row stride as the pitch.  counts: dict of columns, core_invariant, core_snps, other; col: int64
        [V], the index of every core SNP column among all columns; letters: uint8 [n_rows, V], upper case; dist: int32 [n_rows, n_rows]"""
        L = self.lib.L
        if not hasattr(L, "pm_snp_begin"):
            raise PmError("this provider of the ABI has no pm_snp_begin")
        v = C.c_void_p
        L.pm_snp_begin.argtypes = [v, C.c_int32]
        L.pm_snp_add.argtypes = [v, C.c_int64, C.c_int64, v, v]
        L.pm_snp_columns.argtypes = [v, v, v]
        L.pm_snp_distances.argtypes = [v, v]
        n = int(chunks[0].shape[0]) if n_rows is None else int(n_rows)
        self.lib._check(L.pm_snp_begin(self.h, n))
        totals = np.zeros(4, np.int64)
        for ch in chunks:
            assert ch.dtype == np.uint8 and ch.ndim == 2 and ch.shape[0] == n
            w = int(ch.shape[1])
            if w and not (ch.strides[1] == 1 and ch.strides[0] >= w):
                ch = np.ascontiguousarray(ch)
            pitch = int(ch.strides[0]) if w else 0
            self.lib._check(L.pm_snp_add(self.h, w, pitch, ch.ctypes.data_as(v) if w else None, totals.ctypes.data_as(v)))
        nv = int(totals[2])
        col, letters, dist = np.zeros(nv, np.int64), np.zeros((n, nv), np.uint8), np.zeros((n, n), np.int32)
        self.lib._check(L.pm_snp_columns(self.h, col.ctypes.data_as(v), letters.ctypes.data_as(v)))
        self.lib._check(L.pm_snp_distances(self.h, dist.ctypes.data_as(v)))
        self._snp_rows, self._snp_core = n, nv
        return dict(zip(("columns", "core_invariant", "core_snps", "other"), (int(x) for x in totals))), col, letters, dist

    NJ_JOIN = np.dtype([("i", np.int32), ("j", np.int32), ("dij", np.float64), ("ri", np.float64), ("rj", np.float64)])
    NJ_LAST = np.dtype([("a", np.int32), ("b", np.int32), ("c", np.int32), ("pad", np.int32), ("dab", np.float64), ("dac", np.float64), ("dbc", np.float64)])

    def nj_tree(self, dist=None, n=None):
        """pm_nj_tree -> (joins, last): the neighbour-joining tree over dist, int32 [n, n], or with dist=None over
        the distances of the last core_snps of this session (still on the device; n: its rows).  joins: a record array of n - 3
        entries with the fields i, j (int32) and dij, ri, rj (float64); last: one record with a, b, c, dab, dac, dbc."""
        L = self.lib.L
        if not hasattr(L, "pm_nj_tree"):
            raise PmError("this provider of the ABI has no pm_nj_tree")
        v = C.c_void_p
        L.pm_nj_tree.argtypes = [v, C.c_int32, v, v, v]
        if dist is not None:
            dist = np.ascontiguousarray(dist, np.int32)
            assert dist.ndim == 2 and dist.shape[0] == dist.shape[1]
            n = int(dist.shape[0])
        elif n is None:
            n = int(getattr(self, "_snp_rows", 3))
        joins, last = np.zeros(max(n - 3, 0), self.NJ_JOIN), np.zeros(1, self.NJ_LAST)
        self.lib._check(L.pm_nj_tree(self.h, n, dist.ctypes.data_as(v) if dist is not None else None, joins.ctypes.data_as(v), last.ctypes.data_as(v)))
        return joins, last[0]

    def boot_distances(self, reps, seed=1, weights=None):
        """pm_boot_distances -> (weights, dist): the weighted SNP distances of `reps` bootstrap replicates over the
        core SNP columns of the last core_snps of this session.  weights=None: the columns are drawn from `seed`; otherwise uint8
        [reps, V], every value at most 15 (a view with a larger row stride is handed over as it lies).  weights: uint8 [reps, V] as
        used; dist: int32 [reps, n, n].  The distances stay on the device for nj_trees()."""
        L = self.lib.L
        if not hasattr(L, "pm_boot_distances"):
            raise PmError("this provider of the ABI has no pm_boot_distances")
        v = C.c_void_p
        L.pm_boot_distances.argtypes = [v, C.c_int32, C.c_uint64, v, C.c_int64, v, v]
        n, nv = int(getattr(self, "_snp_rows", 0)), int(getattr(self, "_snp_core", 0))
        given, pitch = None, 0
        if weights is not None:
            weights = np.asarray(weights)
            assert weights.dtype == np.uint8 and weights.shape == (reps, nv)
            if nv and not (weights.strides[1] == 1 and weights.strides[0] >= nv):
                weights = np.ascontiguousarray(weights)
            given, pitch = weights.ctypes.data_as(v), int(weights.strides[0]) if nv else 0
        wout, dist = np.zeros((max(reps, 0), nv), np.uint8), np.zeros((max(reps, 0), n, n), np.int32)
        self.lib._check(L.pm_boot_distances(self.h, reps, seed & (2 ** 64 - 1), given, pitch, wout.ctypes.data_as(v), dist.ctypes.data_as(v)))
        self._boot_reps = reps
        return wout, dist

    def nj_trees(self, dist=None, n=None, count=None):
        """pm_nj_trees -> (joins, last): `count` neighbour-joining trees of one n, each the tree of nj_tree() bit for bit, joined in
        lock step.  dist: int32 [count, n, n], or None for the replicate distances of the last boot_distances (n: its rows, count:
        its replicates).  joins: record array [count, n - 3]; last: record array [count].  The records stay on the device for
        nj_support()."""
        L = self.lib.L
        if not hasattr(L, "pm_nj_trees"):
            raise PmError("this provider of the ABI has no pm_nj_trees")
        v = C.c_void_p
        L.pm_nj_trees.argtypes = [v, C.c_int32, C.c_int32, v, v, v]
        if dist is not None:
            dist = np.ascontiguousarray(dist, np.int32)
            assert dist.ndim == 3 and dist.shape[1] == dist.shape[2]
            count, n = int(dist.shape[0]), int(dist.shape[1])
        else:
            n = int(getattr(self, "_snp_rows", 3)) if n is None else n
            count = int(getattr(self, "_boot_reps", 1)) if count is None else count
        joins, last = np.zeros((max(count, 0), max(n - 3, 0)), self.NJ_JOIN), np.zeros(max(count, 0), self.NJ_LAST)
        self.lib._check(L.pm_nj_trees(self.h, n, count, dist.ctypes.data_as(v) if dist is not None else None, joins.ctypes.data_as(v), last.ctypes.data_as(v)))
        self._boot_trees = count
        return joins, last

    def nj_support(self, n, main_joins, rep_joins=None, count=None):
        """pm_nj_support -> support, int32 [n - 3]: in how many of `count` trees the split of every join of main_joins occurs, as a set
        of leaves.  rep_joins: record array [count, n - 3], or None for the records of the last nj_trees() on the device."""
        L = self.lib.L
        if not hasattr(L, "pm_nj_support"):
            raise PmError("this provider of the ABI has no pm_nj_support")
        v = C.c_void_p
        L.pm_nj_support.argtypes = [v, C.c_int32, v, C.c_int32, v, v]
        main_joins = np.ascontiguousarray(main_joins, self.NJ_JOIN)
        assert main_joins.shape == (max(n - 3, 0),)
        if rep_joins is not None:
            rep_joins = np.ascontiguousarray(rep_joins, self.NJ_JOIN)
            assert rep_joins.ndim == 2 and rep_joins.shape[1] == max(n - 3, 0)
            count = int(rep_joins.shape[0])
        elif count is None:
            count = int(getattr(self, "_boot_trees", 1))
        support = np.zeros(max(n - 3, 0), np.int32)
        self.lib._check(L.pm_nj_support(self.h, n, main_joins.ctypes.data_as(v), count, rep_joins.ctypes.data_as(v) if rep_joins is not None else None,
                                        support.ctypes.data_as(v)))
        return support

    def _rec_fn(self, name, argtypes):
        L = self.lib.L
        if not hasattr(L, name):
            raise PmError("this provider of the ABI has no %s" % name)
        fn = getattr(L, name)
        fn.argtypes = argtypes
        return fn

    def rec_sites(self):
        """pm_rec_sites -> uint8 [V]: 1 where a core SNP column of the last core_snps of this session is informative (INTEGRATION.md
        1d).  The transposed planes stay on the device for rec_incompat()."""
        v = C.c_void_p
        fn = self._rec_fn("pm_rec_sites", [v, v, v])
        flags, count = np.zeros(int(getattr(self, "_snp_core", 0)), np.uint8), C.c_int64(-1)
        self.lib._check(fn(self.h, flags.ctypes.data_as(v), C.byref(count)))
        assert count.value == int(flags.sum())
        return flags

    @staticmethod
    def _rec_offsets(win_off):
        win_off = np.ascontiguousarray(win_off, np.int64)
        assert win_off.ndim == 1 and len(win_off) >= 1
        return win_off, len(win_off) - 1

    def rec_incompat(self, sites, win_off):
        """pm_rec_incompat -> list of uint8 [k, k]: the pair scores of every window sites[win_off[w]:win_off[w + 1]] (indices into
        the core SNP columns).  The matrices stay on the device for rec_test()."""
        v = C.c_void_p
        fn = self._rec_fn("pm_rec_incompat", [v, C.c_int64, v, C.c_int64, v, v])
        sites = np.ascontiguousarray(sites, np.int64)
        win_off, nw = self._rec_offsets(win_off)
        k = np.diff(win_off)
        ok = nw > 0 and bool((k >= 0).all()) and bool((k <= 4096).all())
        out = np.zeros(int((k * k).sum()) if ok else 0, np.uint8)
        self.lib._check(fn(self.h, len(sites), sites.ctypes.data_as(v), nw, win_off.ctypes.data_as(v), out.ctypes.data_as(v)))
        at = np.concatenate(([0], np.cumsum(k * k))) if ok else [0]
        return [out[at[w]:at[w + 1]].reshape(int(k[w]), int(k[w])) for w in range(nw)]

    def rec_test(self, win_off, near=10, perms=1000, seed=1, inc=None, win_id=None):
        """pm_rec_test -> (phi, le), int32 [windows] each: the statistic at identity order and the number of the `perms`
        permutations that do not exceed it.  inc: a list of uint8 [k, k] (or their packed bytes), None: the matrices of the last
        rec_incompat() on the device.  win_id: the windows' numbers g (int64), None: 0, 1, ..."""
        v = C.c_void_p
        fn = self._rec_fn("pm_rec_test", [v, C.c_int64, v, v, C.c_int32, C.c_int32, C.c_uint64, v, v, v])
        win_off, nw = self._rec_offsets(win_off)
        if inc is not None:
            if isinstance(inc, (list, tuple)):
                inc = np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(m, np.uint8).ravel() for m in inc])
            inc = np.ascontiguousarray(inc, np.uint8)
        if win_id is not None:
            win_id = np.ascontiguousarray(win_id, np.int64)
            assert win_id.shape == (nw,)
        phi, le = np.zeros(nw, np.int32), np.zeros(nw, np.int32)
        self.lib._check(fn(self.h, nw, win_off.ctypes.data_as(v), inc.ctypes.data_as(v) if inc is not None else None, near, perms, seed & (2 ** 64 - 1),
                           win_id.ctypes.data_as(v) if win_id is not None else None, phi.ctypes.data_as(v), le.ctypes.data_as(v)))
        return phi, le

    EXT_ROW = np.dtype([("genome", np.int32), ("step", np.int32), ("complement", np.int32), ("len", np.int32), ("first", np.int64)])
    EXT_DEFAULTS = dict(match=5, mismatch=4, gap=2, band=50, ani=95, min_len=10, max_flank=256)

    @classmethod
    def _ext_args(cls, params, row_off, rows):
        p = dict(cls.EXT_DEFAULTS, **(params or {}))
        prm = np.array([p[k] for k in ("match", "mismatch", "gap", "band", "ani", "min_len", "max_flank")], np.int32)
        row_off = np.ascontiguousarray(row_off, np.int64)
        assert row_off.ndim == 1 and len(row_off) >= 1
        if not (isinstance(rows, np.ndarray) and rows.dtype == cls.EXT_ROW):
            rows = np.array([tuple(r) for r in rows], cls.EXT_ROW)      # (genome, step, complement, len, first) per row
        rows = np.ascontiguousarray(rows)
        assert len(rows) >= row_off[-1]
        return p, prm, row_off, rows, len(row_off) - 1

    def ext_reach(self, row_off, rows, params=None, best=False):
        """pm_ext_reach -> reach, int32 [jobs]: the rows of job j are rows[row_off[j]:row_off[j + 1]], tuples
        (genome, step, complement, len, first) or a record array of EXT_ROW, the first of a job its reference row.  params: a dict
        over EXT_DEFAULTS.  best=True: -> (reach, best), best int32 [rows, max_flank + 1] with INT32_MIN where undefined."""
        v = C.c_void_p
        fn = self._rec_fn("pm_ext_reach", [v, v, C.c_int64, v, v, v, v])
        p, prm, row_off, rows, nj = self._ext_args(params, row_off, rows)
        reach = np.zeros(nj, np.int32)
        table = np.zeros((len(rows), max(int(p["max_flank"]), 0) + 1), np.int32) if best else None
        self.lib._check(fn(self.h, prm.ctypes.data_as(v), nj, row_off.ctypes.data_as(v), rows.ctypes.data_as(v), reach.ctypes.data_as(v),
                           table.ctypes.data_as(v) if best else None))
        return (reach, table) if best else reach

    def ext_align(self, row_off, rows, reach, params=None, max_cols=None, out_off=None, out=None):
        """pm_ext_align -> (cols, used, blocks): cols int32 [jobs] (0: reach 0, -1: too wide), used int32 [rows] (j_r), blocks a list
        per job of uint8 [rows of the job, cols] (None where cols <= 0), the letters in the flank's own order.  max_cols: the pitch
        of a row (default 2 max_flank); out_off: the byte offsets of the jobs' blocks (default: one after the other); out: the caller's
        own uint8 buffer for the blocks (it must hold them all; the blocks returned are views of it)."""
        v = C.c_void_p
        fn = self._rec_fn("pm_ext_align", [v, v, C.c_int64, v, v, v, C.c_int64, v, v, v, v])
        p, prm, row_off, rows, nj = self._ext_args(params, row_off, rows)
        reach = np.ascontiguousarray(reach, np.int32)
        assert reach.shape == (nj,)
        pitch = 2 * int(p["max_flank"]) if max_cols is None else int(max_cols)
        out_off = np.ascontiguousarray(row_off[:-1] * pitch if out_off is None else out_off, np.int64)
        assert out_off.shape == (nj,)
        n = np.diff(row_off)
        size = int((out_off + n * pitch).max()) if nj and pitch > 0 and bool((n >= 0).all()) and bool((out_off >= 0).all()) else 0
        if out is None:
            out = np.zeros(size, np.uint8)
        assert out.dtype == np.uint8 and out.ndim == 1 and out.flags.c_contiguous and len(out) >= size
        cols, used = np.zeros(nj, np.int32), np.zeros(len(rows), np.int32)
        self.lib._check(fn(self.h, prm.ctypes.data_as(v), nj, row_off.ctypes.data_as(v), rows.ctypes.data_as(v), reach.ctypes.data_as(v), pitch,
                           out_off.ctypes.data_as(v), out.ctypes.data_as(v), cols.ctypes.data_as(v), used.ctypes.data_as(v)))
        blocks = [out[out_off[j]:out_off[j] + n[j] * pitch].reshape(int(n[j]), pitch)[:, :cols[j]] if cols[j] > 0 else None for j in range(nj)]
        return cols, used, blocks

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def multi_mum_batch(self, starts, lens, minsize):
        """starts, lens: [n_regions, n_genomes]; minsize: [n_regions] -> list of (k, lon, sp[c, n-1], fwd[c, n-1]) per region"""
        starts = np.ascontiguousarray(starts, np.int64); lens = np.ascontiguousarray(lens, np.int64)
        minsize = np.ascontiguousarray(minsize, np.int32)
        nreg = starts.shape[0]
        assert starts.shape == (nreg, self.n) == lens.shape and minsize.shape == (nreg,)
        res = C.c_void_p()
        L = self.lib.L
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        self.lib._check(L.pm_multi_mum_batch(self.h, nreg, p(starts, C.c_int64), p(lens, C.c_int64), p(minsize, C.c_int32), C.byref(res)))
        try:
            total = L.pm_result_total(res); q = self.n - 1
            off = np.ctypeslib.as_array(L.pm_result_offsets(res), (nreg + 1,)).copy()
            if total:
                k = np.ctypeslib.as_array(L.pm_result_k(res), (total,)).copy()
                lon = np.ctypeslib.as_array(L.pm_result_lon(res), (total,)).copy()
                sp = np.ctypeslib.as_array(L.pm_result_sp(res), (total * q,)).astype(np.int64).reshape(total, q)
                fw = np.ctypeslib.as_array(L.pm_result_fwd(res), (total * q,)).copy().reshape(total, q)
            else:
                k = np.zeros(0, np.int32); lon = np.zeros(0, np.int32); sp = np.zeros((0, q), np.int64); fw = np.zeros((0, q), np.uint8)
        finally:
            L.pm_result_free(res)
        return [(k[off[r]:off[r + 1]].astype(np.int64), lon[off[r]:off[r + 1]], sp[off[r]:off[r + 1]], fw[off[r]:off[r + 1]]) for r in range(nreg)]

    def whole(self, minsize):
        """the anchor call: one region = every genome in full"""
        lens = np.array([[len(s) for s in self._seqs]], np.int64)
        return self.multi_mum_batch(np.zeros_like(lens), lens, [minsize])[0]

    def mumi_coverage(self):
        """calcmumi: reference positions covered by pairwise MUMs >= 15, per query genome (whole genomes)"""
        lens = (C.c_int64 * self.n)(*[len(s) for s in self._seqs])
        starts = (C.c_int64 * self.n)(*([0] * self.n))
        cov = (C.c_int64 * max(1, self.n - 1))()
        self.lib.L.pm_mumi_coverage.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self.lib._check(self.lib.L.pm_mumi_coverage(self.h, starts, lens, cov))
        return [int(cov[i]) for i in range(self.n - 1)]

    def last_timing(self):
        cnt = C.c_int(64); names = (C.c_char_p * 64)(); ms = (C.c_float * 64)()
        self.lib.L.pm_last_timing(self.h, C.byref(cnt), names, ms)
        return [(names[i].decode(), float(ms[i])) for i in range(cnt.value)]
