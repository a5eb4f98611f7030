"""The host side of the recombination scan that needs no device (parsnp_amd/csrc/host/recomb.cpp: the windows over the LCBs' site
lists, the text of .rec.tsv and .rec) as a stand-alone program under AddressSanitizer and UBSan (tests/emu/rec_host_check.cpp, its
own main) against the numpy restatement of tests/recphi.py.  A CPU program: no GPU, nothing loaded into python."""
import os
import subprocess

import numpy as np
import pytest

import recphi as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "emu", "rec_host_check_asan")
HOST = os.path.join(ROOT, "parsnp_amd", "csrc", "host")


@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "emu", "rec_host_check.cpp")
    deps = [src, os.path.join(HOST, "recomb.cpp"), os.path.join(HOST, "aligner.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-w",
                        "-I" + HOST, src, "-o", BIN], check=True)
    return BIN


def case(lcb_sites, K, perms, seed):
    """LCBs with the given numbers of informative sites, uninformative columns strewn between them; the second LCB's reference
    positions descend (a reverse-strand LCB), two LCBs share a first reference position"""
    rng = np.random.default_rng(seed)
    rows, inf = [], []
    for b, m in enumerate(lcb_sites):
        flags = [1] * m + [0] * int(rng.integers(0, 9))
        rng.shuffle(flags)
        base = 5000 * (b // 2)      # (LCBs 2 j and 2 j + 1 overlap on the reference: ties of first_ref in .rec)
        refs = base + np.cumsum(rng.integers(1, 9, len(flags)))
        if b == 1:
            refs = refs[::-1]
        for c, (fl, r) in enumerate(zip(flags, refs)):
            rows.append((b + 1, 3 * c + b, int(r)))
            inf.append(int(fl))
    return rows, inf, K, perms


CASES = {
    "edges100": ([15, 16, 99, 100, 101, 149, 150, 151, 0, 250], 100, 1000),
    "k16": ([16, 17, 31, 32, 33, 40, 1], 16, 99),
    "k17": ([33, 34, 35, 17, 16], 17, 100),
    "k256": ([255, 256, 257, 600], 256, 65536),
    "none": ([3, 15, 0], 100, 1000),
    "empty": ([], 100, 1000),
}


def want(rows, inf, K, perms):
    sites, off, recs = [], [0], []
    for a, b in rp.lcb_runs(rows):
        lst = [c for c in range(a, b) if inf[c]]
        for s, k in rp.windows_of(len(lst), K):
            win = lst[s:s + k]
            sites += win
            off.append(len(sites))
            g = len(recs)
            ref = [rows[c][2] for c in win]
            le = (7 * g) % 11 % (perms + 1)
            recs.append(dict(cluster=rows[win[0]][0], first_column=rows[win[0]][1], last_column=rows[win[-1]][1], first_ref=min(ref), last_ref=max(ref), sites=k,
                             phi=3 * g + 1, le=le, perms=perms, flagged=rp.flagged(le, perms), g=g))
    tsv, bed = rp.files_text(recs)
    text = "sites" + "".join(" %d" % s for s in sites) + "\noffsets" + "".join(" %d" % o for o in off) + "\n"
    return text + tsv + "----\n" + bed + "----\n%d\n" % sum(r["flagged"] for r in recs), recs


@pytest.mark.parametrize("name", list(CASES))
def test_windows_and_text(checker, tmp_path, name):
    lcbs, K, perms = CASES[name]
    rows, inf, K, perms = case(lcbs, K, perms, len(name))
    path = str(tmp_path / "in.txt")
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (len(rows), K, perms))
        for (cl, col, ref), fl in zip(rows, inf):
            f.write("%d %d %d %d\n" % (cl, col, ref, fl))
    p = subprocess.run([checker, path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    text, recs = want(rows, inf, K, perms)
    assert p.stdout == text
    if name == "edges100":
        assert [r["sites"] for r in recs].count(99) == 1 and len(recs) == 0 + 1 + 1 + 1 + 2 + 2 + 2 + 3 + 0 + 4 and any(r["flagged"] for r in recs)
        flagged = [r for r in recs if r["flagged"]]
        assert any(r["first_ref"] > r2["first_ref"] and r["g"] < r2["g"] for r in flagged for r2 in flagged)      # (.rec is not in order g)
    if name in ("none", "empty"):
        assert recs == [] and p.stdout.endswith(rp.HEADER + "----\n----\n0\n")
