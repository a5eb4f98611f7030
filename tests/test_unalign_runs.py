"""pm_store_unalign_count / pm_store_unalign_runs (the runs parsnp.unalign lists, counted and listed by the engine from the layout it
holds) against the restatement of tests/unalignruns.py, in the kernel emulation (one host thread plays every lane of UnalignCount
and UnalignWrite); tests/test_gpu_unalign_runs.py runs the same checks on the device.

The store calls are driven to a settled layout by the ctypes driver of tests/storecalls.py, the image is fetched with
pm_store_layout, and counts, starts, ends and ordinals are compared with the runs of that image element for element; the image
must be the same afterwards, and a second pair of calls must give the same answer.  Every case asserts its floors: that the runs
the generator aims at -- on both sides of a word of the image and of the 64 words of a wavefront -- are in the layout."""
import functools

import numpy as np
import pytest

import storecalls as sc
import unalignruns as ur
from parsnp_amd.binding import Lib

# case -> (set, unmark every accepted row first, floors)
WORDS = {"len%d_%s" % (ln, w) for ln in (1, 2, 3) for w in ("ends_word", "starts_word")} | {"len2_across_words", "len3_across_words"}
CASES = {
    "edges": ("edges", False, WORDS | {"starts_at_0", "ends_at_last_base", "whole_words_64", "whole_words_128", "len63", "len65", "ends_block", "starts_block",
                                      "starts_block_plus_1", "across_blocks", "spans_a_block"}),
    "last_has_more": ("last_has_more", False, WORDS | {"whole_words_64", "len63", "len65"}),
    "last_has_none": ("last_has_none", False, WORDS | {"no_unmarked_base"}),
    "tiny": ("tiny", False, {"starts_at_0", "ends_at_last_base"}),
    "k4": ("k4", False, {"ends_at_last_base", "across_blocks", "len63", "len65"}),
    "edges_unmarked": ("edges", True, {"no_marked_base", "spans_a_block", "starts_at_0", "ends_at_last_base"}),
}


@pytest.fixture(scope="module")
def lib(emu):
    return Lib(emu[0])


@functools.lru_cache(maxsize=None)
def sequences(name):
    return ur.SETS[name]()


def settled(lib, case):
    name, unmark, _ = CASES[case]
    st = sc.Store(lib, sequences(name), tune={"dirty_min": 1, "flagged_div": 1})
    try:
        rc, info = st.settle()
        assert rc == sc.PM_OK
        acc = np.flatnonzero(info["state_flags"] & sc.ST_ACCEPTED)
        assert len(acc) >= 2, "the set left no MUMs"
        if unmark:
            st.unmark(acc)
    except BaseException:
        st.close()
        raise
    return st


def check_runs(lib, case):
    with settled(lib, case) as st:
        before = st.layout()
        missing = CASES[case][2] - ur.floors(before)
        assert not missing, "the layout of %s lacks %s" % (case, sorted(missing))
        runs, all_runs, kept = st.sess.unaligned_runs()
        again = st.sess.unaligned_runs()
        after = st.layout()
        names = [n for n, _ in st.sess.last_timing()]
    for j, m in enumerate(before):
        start, end, ordinal, total = ur.runs_of(m)
        assert (int(all_runs[j]), int(kept[j])) == (total, len(start)), "genome %d: runs and kept runs %d, %d; restatement %d, %d" % (j, all_runs[j], kept[j], total, len(start))
        for what, got, want in (("start", runs[j][0], start), ("end", runs[j][1], end), ("ordinal", runs[j][2], ordinal)):
            assert got.dtype == np.int32
            if not np.array_equal(got, want):
                x = int(np.flatnonzero(got != want)[0])
                raise AssertionError("genome %d: %s of kept run %d is %d, restatement %d (%d of %d differ)" % (j, what, x, got[x], want[x], int((got != want).sum()), len(want)))
        assert np.array_equal(m, after[j]), "the calls changed the layout of genome %d" % j
        assert all(np.array_equal(a, b) for a, b in zip(runs[j], again[0][j]))
    assert np.array_equal(all_runs, again[1]) and np.array_equal(kept, again[2])
    assert "unalign_write" in names or lib.provider == "emu"      # (the emulation's backend keeps no phase times)


@pytest.mark.parametrize("case", list(CASES))
def test_runs(lib, case):
    check_runs(lib, case)


def check_wrong_size(lib):
    """the write call takes exactly the sum of the kept counts: anything else is refused and writes nothing past its arrays"""
    import ctypes as C
    from parsnp_amd.binding import PmError
    with settled(lib, "tiny") as st:
        _, _, kept = st.sess.unaligned_runs()
        n = int(kept.sum()) - 1
        guard = 12345
        arrays = [np.full(n + 4, guard, np.int32) for _ in range(3)]
        with pytest.raises(PmError):
            lib._check(lib.L.pm_store_unalign_runs(st.h, *(a.ctypes.data_as(C.c_void_p) for a in arrays), C.c_int64(n)))
        assert all((a[n:] == guard).all() for a in arrays)


def test_wrong_size_is_refused(lib):
    check_wrong_size(lib)


def test_before_settle_is_refused(lib):
    """valid where pm_store_layout is: not before the anchor list is settled"""
    from parsnp_amd.binding import PmError
    st = sc.Store(lib, sequences("tiny"), tune={"dirty_min": 1})
    with st:
        with pytest.raises(PmError):
            st.sess.unaligned_runs()


@pytest.mark.parametrize("name", list(ur.SETS))
def test_closed_form_of_the_records(name):
    """the file as {(r, k): r < runs[k], r <= runs[n - 1], kept} in the order of (r, k) is the file of the reference's loop -- on layouts
    made from the sets' own blocks and fillers, and with the sentinel of every genome cleared (a run that ends AT the sentinel)"""
    seqs = sequences(name)
    rng = np.random.default_rng(1)
    names = [b"g%d.fna" % k for k in range(len(seqs))]
    for variant in range(3):
        layout = []
        for s in seqs:
            m = np.ones(len(s) + 1, bool)
            for _ in range(40):
                a = int(rng.integers(0, len(s) + 1))
                m[a: a + int(rng.choice([1, 1, 2, 3, 64, 65]))] = False
            m[-1] = variant != 2
            layout.append(m)
        if variant == 1:
            layout[-1][:] = True
        assert ur.records_closed(layout, names, seqs) == ur.records(layout, names, seqs)


# ---------------------------------------------------------------------------------------------------------------- end to end
# set -> flagged_div of the resident run (1 lets a rearranged anchor list onto the route).  Collinear, rearranged, draft contigs
# joined by N padding, multi-contig / IUPAC / lower-case FASTA
E2E_SETS = {"pop6x200k": 8, "rearr6x300k": 1, "draft8x300k": 8, "messy": 8}


def golden():
    import json
    import os
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unalign.json")))


def check_e2e(core_hooks, name, route, base, threads=4):
    """parsnp.unalign of the writer (runs from the engine's two calls on the resident route, from the word-wise scan of the host's
    bitmaps on the host route; records formatted in parallel) is byte for byte the file of the old bit-by-bit walk (test hook
    PARSNP_UNALIGN_WALK) and the reference binary's (tests/golden/unalign.json); on the resident route the engine sends the host less
    than the layout image in the WHOLE process (the walk's run, which fetches the image, sends more)"""
    import os
    import test_host_logic
    import xmfa_util
    from parsnp_amd import driver
    want = golden()[name]
    rp, qs, kw = test_host_logic.harsh_inputs(name, base)
    env = dict(os.environ, PARSNP_PARALLEL_MIN="8", PARSNP_FREE_MIN="2", PM_DIRTY_MIN="8", PM_FLAGGED_DIV=str(E2E_SETS[name]))
    if route == "host":
        env["PARSNP_NO_RESIDENT"] = "1"
    got = {}
    for who in ("runs", "walk"):
        out = os.path.join(base, who)
        e = dict(env, PARSNP_RESIDENT_LOG=os.path.join(base, who + ".log"))
        if who == "walk":
            e["PARSNP_UNALIGN_WALK"] = "1"
        rc, _ = driver.run_core(core_hooks, rp, qs, out, env=e, threads=threads, timing=os.path.join(base, who + ".json"), unaligned=1, **kw)
        assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
        assert ("resident=1" in open(e["PARSNP_RESIDENT_LOG"]).read()) == (route == "resident")
        assert xmfa_util.md5(os.path.join(out, "parsnpAligner.xmfa")) == want["xmfa_md5"]
        got[who] = (open(os.path.join(out, "parsnp.unalign"), "rb").read(), driver.read_timing(os.path.join(base, who + ".json")))
    assert got["runs"][0] == got["walk"][0], "the writer and the bit-by-bit walk differ"
    import hashlib
    assert len(got["runs"][0]) == want["unalign_bytes"] and hashlib.md5(got["runs"][0]).hexdigest() == want["unalign_md5"]
    t, tw = got["runs"][1], got["walk"][1]
    assert t["unalign_runs"] >= t["unalign_kept"] >= want["unalign_records"] > 0 and t["unalign_s"] > 0
    if route == "resident":
        # pm_session_traffic is a running count: what the writer downloads is its difference over the writer (unalign_d2h_bytes).  The
        # whole process downloads more than a layout image on sets this small whatever the writer does -- the MUM rows of the XMFA
        # writer alone are 4 to 6 images here -- so the whole-process count is compared between the two runs instead
        assert t["resident"] == 1 and 0 < t["unalign_d2h_bytes"] < t["layout_bytes"], (t["unalign_d2h_bytes"], t["layout_bytes"])
        assert t["unalign_d2h_bytes"] <= 12 * t["unalign_kept"] + 16 * t["genomes"] + 16
        # (the walk's run fetches the image and lists no runs; the rest of the two processes downloads the same, up to a search that had to repeat a part)
        assert tw["session_d2h_bytes"] - t["session_d2h_bytes"] >= (tw["layout_bytes"] - t["unalign_d2h_bytes"]) // 2, (t["session_d2h_bytes"], tw["session_d2h_bytes"])
    else:
        assert t["resident"] == 0 and t["unalign_d2h_bytes"] == 0


@pytest.mark.parametrize("route", ["resident", "host"])
@pytest.mark.parametrize("name", list(E2E_SETS))
def test_parsnp_unalign(emu, tmp_path, name, route):
    check_e2e(emu[1], name, route, str(tmp_path))


def check_twice(core_lib, base, env):
    """step, write, step, write in one process with unaligned=1: the same XMFA and the same parsnp.unalign both times -- the writer
    leaves nothing behind that the next step reads"""
    import os
    import subprocess
    import sys
    import test_host_logic
    from parsnp_amd import driver
    want = golden()["pop6x200k"]
    rp, qs, kw = test_host_logic.harsh_inputs("pop6x200k", base)
    out = os.path.join(base, "out")
    os.makedirs(out)
    ini = os.path.join(out, "parsnpAligner.ini")
    open(ini, "w").write(driver.ini_text(rp, qs, out, unaligned=1, threads=2))
    code = (
        "import sys, hashlib, os; sys.path.insert(0, %r)\n"
        "from parsnp_amd.core_api import CoreRun\n"
        "r = CoreRun(%r, lib_path=%r)\n"
        "for k in range(2):\n"
        "    s = r.step(); assert s['resident'] == 1, s\n"
        "    assert r.write() == 0\n"
        "    print(hashlib.md5(open(os.path.join(%r, 'parsnpAligner.xmfa'), 'rb').read()).hexdigest(), hashlib.md5(open(os.path.join(%r, 'parsnp.unalign'), 'rb').read()).hexdigest())\n"
        % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), ini, core_lib, out, out))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), cwd=out)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()[-2:]
    assert lines == ["%s %s" % (want["xmfa_md5"], want["unalign_md5"])] * 2, lines


def test_unaligned_twice_in_one_process(emu, tmp_path):
    import os
    check_twice(os.path.join(os.path.dirname(emu[0]), "libparsnp_core_emu.so"), str(tmp_path), dict(PARSNP_PARALLEL_MIN="8", PARSNP_FREE_MIN="2", PM_DIRTY_MIN="8"))
