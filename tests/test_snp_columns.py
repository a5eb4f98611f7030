"""Core SNP columns and SNP distances (pm_snp_*; SnpClassify, SnpRank, SnpPack and SnpDist of snp_kernels.h) against the numpy
restatement of tests/snpcols.py, in the kernel emulation (one host thread plays every lane); tests/test_gpu_snp_columns.py runs the
same checks on the device.  Then the writer: with snps=1 the three files beside the XMFA equal what snpcols.scan_xmfa derives from
the XMFA of the same run, and the XMFA is the one of snps=0."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import snpcols as sn
from parsnp_amd.binding import Lib, PmError, Session

PM_EINVAL, PM_ELIMIT = -2, -5


@functools.lru_cache(maxsize=None)
def cases():
    return sn.matrix_cases(1)


@functools.lru_cache(maxsize=None)
def want(name):
    """the restatement's answer for a case: computed once, shared by the emulation's and the device's tests, never changed"""
    return sn.expected(cases()[name].chunks)


CASE_NAMES = list(cases())


@pytest.fixture(scope="module")
def lib(emu):
    return Lib(emu[0])


def two_genomes(lib):
    return Session(lib, [b"ACGTTGCAAGGCTTAACCGGTACGATCGATTACGGCAT" * 4] * 2)


def compare(got, exp, what=""):
    counts, col, letters, dist = got
    e_counts, e_col, e_letters, e_dist = exp
    assert counts == e_counts, (what, counts, e_counts)
    assert sum(counts[k] for k in ("core_invariant", "core_snps", "other")) == counts["columns"]
    assert col.dtype == np.int64 and np.array_equal(col, e_col), what
    assert letters.shape == e_letters.shape
    if not np.array_equal(letters, e_letters):
        r, v = np.argwhere(letters != e_letters)[0]
        raise AssertionError("%s: letter of row %d, core SNP %d is %r, restatement %r (%d differ)" % (what, r, v, chr(letters[r, v]), chr(e_letters[r, v]), int((letters != e_letters).sum())))
    assert dist.dtype == np.int32 and dist.shape == e_dist.shape
    if not np.array_equal(dist, e_dist):
        i, j = np.argwhere(dist != e_dist)[0]
        raise AssertionError("%s: dist[%d][%d] is %d, restatement %d (%d differ)" % (what, i, j, dist[i, j], e_dist[i, j], int((dist != e_dist).sum())))
    assert np.array_equal(dist, dist.T) and not dist.diagonal().any()


def check_case(lib, name):
    case = cases()[name]
    exp = want(name)
    assert np.array_equal(sn.classes(np.concatenate(case.chunks, axis=1)), case.designed), "the restatement disagrees with the design of " + name
    with two_genomes(lib) as s:
        compare(s.core_snps(case.chunks), exp, name)
        if name == "adds":
            # one add of the concatenation gives the same; and a collection begun after another starts from zero
            whole = [np.ascontiguousarray(np.concatenate(case.chunks, axis=1))]
            compare(s.core_snps(whole), exp, "adds as one add")
            assert [int((sn.classes(c) == sn.SNP).sum()) for c in case.chunks] == list(sn.ADD_SNPS) and [c.shape[1] for c in case.chunks] == list(sn.ADD_WIDTHS)
            assert list(np.cumsum((0,) + sn.ADD_SNPS)[:-1]) == [0, 1, 63, 64, 65, 165, 165]      # the core SNPs before every add
            compare(s.core_snps(case.chunks[:1]), sn.expected(case.chunks[:1]), "a new collection")
        if name == "pairs":
            v = exp[0]["core_snps"]
            assert v > 64 and exp[3][0, 1] == 0 and exp[3][2, 3] == v


@pytest.mark.parametrize("name", CASE_NAMES)
def test_matrix(lib, name):
    check_case(lib, name)


def test_designs_reach_their_edges():
    c = cases()
    assert {c[k].n for k in c} >= {2, 3, 63, 64, 65, 129, 2048}
    assert [want("snps%d" % k)[0]["core_snps"] for k in (0, 1, 63, 64, 65, 128, 129)] == [0, 1, 63, 64, 65, 128, 129]
    assert want("snps_all")[0]["core_snps"] == 130 and list(want("snps_last_only")[1]) == [99]
    assert want("snps0_all_other")[0]["other"] == want("snps0_all_other")[0]["columns"] > 0
    assert want("snps0_all_invariant")[0]["core_invariant"] == want("snps0_all_invariant")[0]["columns"] > 0
    assert want("rows2048")[0]["core_snps"] == 300
    for kind in sn.KINDS:
        cl = sn.KIND_CLASS[kind]
        assert [want("single_" + kind)[0][k] for k in ("core_invariant", "core_snps", "other")] == [int(cl == x) for x in (sn.INV, sn.SNP, sn.OTHER)], kind


def check_arguments(lib):
    L = lib.L
    v = C.c_void_p
    assert lib.snp_limits() == 2048
    buf = np.full((2, 8), ord("A"), np.uint8)
    p = buf.ctypes.data_as(v)
    with two_genomes(lib) as s:
        L.pm_snp_begin.argtypes = [v, C.c_int32]
        L.pm_snp_add.argtypes = [v, C.c_int64, C.c_int64, v, v]
        L.pm_snp_columns.argtypes = [v, v, v]
        L.pm_snp_distances.argtypes = [v, v]
        dist = np.full((2, 2), 7, np.int32)
        # before a collection is started
        assert L.pm_snp_add(s.h, 8, 8, p, None) == PM_EINVAL
        assert L.pm_snp_columns(s.h, None, None) == PM_EINVAL
        assert L.pm_snp_distances(s.h, dist.ctypes.data_as(v)) == PM_EINVAL
        assert L.pm_snp_begin(s.h, 1) == PM_EINVAL
        assert L.pm_snp_begin(s.h, 2049) == PM_ELIMIT
        assert L.pm_snp_add(s.h, 8, 8, p, None) == PM_EINVAL      # (a refused begin starts nothing)
        assert L.pm_snp_begin(s.h, 2) == 0
        assert L.pm_snp_add(s.h, 8, 7, p, None) == PM_EINVAL
        assert L.pm_snp_add(s.h, -1, 8, p, None) == PM_EINVAL
        assert L.pm_snp_add(s.h, 8, 8, None, None) == PM_EINVAL
        assert L.pm_snp_add(s.h, 0, 0, None, None) == 0
        assert L.pm_snp_add(s.h, 8, 8, p, None) == 0               # totals may be NULL
        assert L.pm_snp_add(s.h, (1 << 31) - 8, 1 << 31, p, None) == PM_ELIMIT      # 2^31 columns in all
        # no core SNP: the columns call writes nothing, the distances are zeros
        col, letters = np.full(4, 7, np.int64), np.full(4, 7, np.uint8)
        assert L.pm_snp_columns(s.h, col.ctypes.data_as(v), letters.ctypes.data_as(v)) == 0
        assert (col == 7).all() and (letters == 7).all()
        assert L.pm_snp_distances(s.h, dist.ctypes.data_as(v)) == 0 and not dist.any()
        with pytest.raises(PmError):
            s.core_snps([np.zeros((1, 3), np.uint8)])


def test_arguments(lib):
    check_arguments(lib)


@pytest.mark.parametrize("launch", ["snp_pack", "snp_dist"])
def test_wavefronts_of_a_launch_do_not_depend_on_one_another(lib, launch, monkeypatch):
    """the launch's wavefronts last to first: the first plane word of an add, which holds bits of the add before it, is where an
    ordering would show"""
    monkeypatch.setenv("PM_EMU_REVERSE_WAVES", launch)
    check_case(lib, "adds")
    check_case(lib, "rows129")


# ---------------------------------------------------------------------------------------------------------------- end to end
# cut-down sets of parsnp_amd.synth: a collinear population; one with inverted segments (reverse-strand rows); hypervariable windows
# (aligned gaps); multi-contig FASTA with N runs, IUPAC codes and lower case
E2E_SETS = {
    "pop6x200k": dict(n=60_000),
    "popinv12x400k": dict(n=120_000, n_genomes=6, inv_every=3, inv_len=20_000),
    "hyper10x300k": dict(n=80_000, n_genomes=6, windows=dict(count=40)),
    "messy": dict(n=60_000),
}
# the streaming writer; every LCB as strings (the slow way); the LCBs in three groups; a staging matrix of 7 columns (test hook: the
# gaps of one LCB go to the engine in many adds, a wider block makes the matrix grow), streamed and as strings
E2E_VARIANTS = {"fast": {}, "plain": {"PARSNP_PLAIN_OUTPUT": "1"}, "groups3": {"PARSNP_GAP_GROUPS": "3"},
                "stage7": {"PARSNP_SNP_STAGE_COLUMNS": "7"}, "stage7_plain": {"PARSNP_SNP_STAGE_COLUMNS": "7", "PARSNP_PLAIN_OUTPUT": "1"},
                "mix2": {"PARSNP_OUTPUT_MIX": "2"}}      # (every second LCB takes the string route late, as an overlap-trimmed one does)
TIMING_KEYS = {"snp_columns", "snp_core", "snp_other", "snp_h2d_bytes", "snp_scan_ms", "snp_dist_ms"}
FILES = ("parsnpAligner.snps.mfa", "parsnpAligner.snps.tsv", "parsnpAligner.snps.dist")


def e2e_inputs(name, base):
    from parsnp_amd import synth
    if name == "messy":
        return synth.messy_set(os.path.join(base, "in"), **E2E_SETS[name])
    r, gs = synth.make(name, **E2E_SETS[name])
    return synth.write_set(os.path.join(base, "in"), r, gs)


def check_e2e(core_bin, name, variant, base, threads=4):
    """snps=1: the three files are what scan_xmfa derives from the XMFA of the same run, exactly; XMFA, log and parsnp.unalign are
    those of the same run with snps=0, which leaves no new file and no new key in its timing record"""
    import xmfa_util
    from parsnp_amd import driver
    rp, qs = e2e_inputs(name, base)
    env = dict(os.environ, **E2E_VARIANTS[variant])
    got = {}
    for snps in (0, 1):
        out = os.path.join(base, "out%d" % snps)
        kw = dict(snps=1) if snps else {}
        rc, _ = driver.run_core(core_bin, rp, qs, out, env=env, threads=threads, timing=os.path.join(base, "t%d.json" % snps), unaligned=1, **kw)
        assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
        got[snps] = driver.read_timing(os.path.join(base, "t%d.json" % snps))
    out0, out1 = os.path.join(base, "out0"), os.path.join(base, "out1")
    for f in ("parsnpAligner.xmfa", "parsnp.unalign"):
        assert xmfa_util.md5(os.path.join(out0, f)) == xmfa_util.md5(os.path.join(out1, f)), f
    strip = lambda p: [l for l in open(p) if "elapsed time" not in l and "running time" not in l]      # noqa: E731
    assert strip(os.path.join(out0, "parsnpAligner.log")) == strip(os.path.join(out1, "parsnpAligner.log"))
    assert not [f for f in FILES if os.path.exists(os.path.join(out0, f))]
    assert sorted(set(os.listdir(out1)) - set(os.listdir(out0))) == sorted(FILES)
    assert set(got[1]) - set(got[0]) == TIMING_KEYS and set(got[0]) <= set(got[1])

    names, letters, rows, dist, counts = sn.scan_xmfa(os.path.join(out1, "parsnpAligner.xmfa"))
    g_names, g_letters, g_rows, g_dist = driver.read_snps(out1)
    assert g_names == names and len(names) == len(qs) + 1
    assert counts["core_snps"] > 100 and counts["other"] > 0, counts      # (the set must have something to find)
    assert g_letters.shape == letters.shape and np.array_equal(g_letters, letters)
    assert g_rows == rows
    assert np.array_equal(g_dist, dist)
    t = got[1]
    assert (t["snp_columns"], t["snp_core"], t["snp_other"]) == (counts["columns"], counts["core_snps"], counts["other"])
    assert counts["core_invariant"] + counts["core_snps"] + counts["other"] == counts["columns"]
    assert 0 < t["snp_h2d_bytes"] < len(names) * counts["columns"]      # (the MUM columns are not uploaded)
    err = open(os.path.join(out1, "parsnp-aligner.err")).read()
    assert "SNP columns: %d columns, %d core invariant, %d core SNPs, %d other" % (counts["columns"], counts["core_invariant"], counts["core_snps"], counts["other"]) in err
    return counts


@pytest.mark.parametrize("variant", list(E2E_VARIANTS))
@pytest.mark.parametrize("name", list(E2E_SETS))
def test_files(emu, tmp_path, name, variant):
    check_e2e(emu[1], name, variant, str(tmp_path))


INI_TODAY = """;Parsnp configuration File
;
[Reference]
file=/x/ref.fna
reverse=0
[Query]
file1=/x/a.fna
reverse1=0
file2=/x/b.fna
reverse2=0
[MUM]
anchors=1.1*(Log(S))
anchorfile=
anchorsonly=0
calcmumi=0
mums=1.1*(Log(S))
mumfile=
filter=1
factor=2.0
extendmums=0
[LCB]
recombfilter=0
cores=3
diagdiff=0.12
doalign=2
c=21
d=300
q=30
p=15000000
icr=0
unaligned=0
[Output]
outdir=/x/out
prefix=parsnp
showbps=1
"""


def test_ini_text():
    from parsnp_amd import driver
    args = ("/x/ref.fna", ["/x/a.fna", "/x/b.fna"], "/x/out")
    assert driver.ini_text(*args, threads=3) == INI_TODAY
    assert driver.ini_text(*args, threads=3, snps=1) == INI_TODAY + "snps=1\n"


def test_too_many_sequences(emu, tmp_path):
    """snps=1 and more than 2 048 sequences: the engine-limit message and exit 5 before any work (no sequence is read: the files
    need not exist); without snps the same ini gets as far as the missing files (exit 1)"""
    from parsnp_amd import driver
    qs = ["/nonexistent/g%d.fna" % i for i in range(2048)]
    rc, _ = driver.run_core(emu[1], "/nonexistent/ref.fna", qs, str(tmp_path / "a"), snps=1)
    assert rc == 5 and "limit of the multi-MUM engine" in open(str(tmp_path / "a" / "parsnp-aligner.err")).read()
    rc, _ = driver.run_core(emu[1], "/nonexistent/ref.fna", qs[:-1], str(tmp_path / "b"), snps=1)
    assert rc == 1
