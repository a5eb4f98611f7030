"""The index build by buckets on the device: the cases of tests/indexgen.py through libparsnp_hip.so -- the runs over neighbouring
lanes, the compare-and-swap in LDS, the overflow list and IndexOverflow's loop, none of which the emulation executes the way a
wavefront does.  The one-K-mer cases come first, each build in a process of its own under a watchdog sized from today's build: a kernel that
does not come back fails that test, and every other test of the file with it, before anything else is launched."""
import os
import subprocess
import sys

import pytest

import indexgen as G
import oracles
import test_emu_engine as T
from conftest import ROOT
from parsnp_amd import synth
from parsnp_amd.binding import Lib, Session
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def guard(cpu_checkers):
    """the one-K-mer cases at the default work budget, each under G.watchdog (today's build first, in a process of its own; the bucket
    build within that time + G.WATCHDOG_MARGIN_S) -> {case: None or what went wrong}; after the first that fails nothing more is launched"""
    out = {}
    for name in G.DEGENERATE + tuple(n + "_short" for n in G.DEGENERATE):
        if any(out.values()):
            out[name] = "not run: an earlier case failed"
            continue
        try:
            w0, w1 = G.watchdog(HIP_LIB, name)
            print("%s: %.2f s by IndexInsert, %.2f s by buckets" % (name, w0, w1))
            out[name] = None
        except AssertionError as e:
            out[name] = str(e)
    return out


@pytest.fixture(scope="module")
def libs(guard, cpu_checkers):
    bad = {k: v for k, v in guard.items() if v}
    assert not bad, "a one-K-mer case failed under its watchdog (test_one_kmer_for_nearly_everything): nothing else is launched\n%s" % bad
    H = Lib(HIP_LIB)
    assert H.provider == "hip"
    return H, oracles.load_restatement()


@pytest.mark.parametrize("name", G.DEGENERATE + tuple(n + "_short" for n in G.DEGENERATE))
def test_one_kmer_for_nearly_everything(guard, libs, name):
    assert guard[name] is None, guard[name]
    G.check(libs[0], libs[1], G.CASES[name]())


@pytest.mark.parametrize("name", [n for n in G.CASES if n not in G.DEGENERATE and not n.endswith("_short")])
def test_case(libs, name):
    G.check(libs[0], libs[1], G.CASES[name]())


def test_mixed_batch(libs):
    G.check_mixed(libs[0], libs[1], T)


def test_overflow_counts_match_the_model(libs):
    for c, sf in ((G.probe_small(), 1), (G.probe_default(), 2)):
        t = G.run_whole(libs[0], c, 1)[1]
        assert t["index_overflow"] == G.overflow_model(c.ref, 16, slot_factor=sf)[0]


def test_at_size(libs):
    """a 200 kb population, the table in 512 buckets (index_bucket_min lowered: the default admits tables of 2^24 slots and more): thousands
    of candidates, the same by both builds"""
    ref, gs = synth.make("pop6x200k")
    got = []
    for build in (1, 0):
        with Session(libs[0], [ref] + gs) as s:
            s.tune("index_build", build); s.tune("index_bucket_min", 1 << 16); s.tune("index_verify", 1)
            got.append(s.whole(19))
            t = dict(s.last_timing())
        assert t["index_lost"] == 0 and t["index_bucketed"] == (len(ref) if build else 0), t
        assert t["index_overflow"] <= len(ref) / 8
    assert len(got[0][0]) > 1000 and T.same(got[0], got[1])
