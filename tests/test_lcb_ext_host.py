"""The host side of the LCB extension that needs no device (parsnp_amd/csrc/host/extend.cpp: the covered stretches from the records'
intervals, the halving of a run between two records, the stop at a letter that is none of ACGT, the descriptors, the records' text)
as a stand-alone program under AddressSanitizer and UBSan (tests/emu/ext_host_check.cpp, its own main) against the numpy restatement
of tests/lcbext.py.  A CPU program: no GPU, nothing loaded into python."""
import os
import subprocess

import numpy as np
import pytest

import lcbext as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "emu", "ext_host_check_asan")
HOST = os.path.join(ROOT, "parsnp_amd", "csrc", "host")


@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "emu", "ext_host_check.cpp")
    deps = [src, os.path.join(HOST, "extend.cpp"), os.path.join(HOST, "aligner.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-w",
                        "-I" + HOST, "-I" + os.path.join(ROOT, "include"), src, "-o", BIN], check=True)
    return BIN


def design(seed, F):
    """three genomes of 700 bases and LCBs whose gaps are 0, 1, 2, odd, even, shorter and longer than 2 F; N runs and lower-case
    letters inside gaps; a reverse row; an LCB that ends at the genome's last base and one that starts at its first"""
    rng = np.random.default_rng(seed)
    genomes = [bytearray(X.rand_seq(rng, 700)) for _ in range(3)]
    genomes[1][130:134] = b"NNNN"
    genomes[2][395:396] = b"N"
    genomes[0][120:140] = bytes(genomes[0][120:140]).lower()
    lcbs = [
        [(1, 11, 100, "+", 1), (2, 1, 95, "+", 1), (3, 20, 110, "+", 1)],            # genome 2: the record begins at base 1
        [(1, 161, 200, "+", 2), (2, 150, 190, "+", 2), (3, 111, 150, "-", 2)],       # 60 / 54 apart (even runs); genome 3 touches LCB 1, reverse
        [(1, 202, 300, "+", 3), (2, 192, 290, "+", 3), (3, 152, 250, "+", 3)],       # one base apart everywhere
        [(1, 304, 350, "+", 4), (2, 290, 340, "+", 4), (3, 251, 300, "-", 4)],       # three apart; overlapping by a base; touching
        [(1, 351 + 2 * F + 5, 690, "+", 5), (2, 400, 700, "+", 5), (3, 420, 650, "+", 5)],      # a run longer than 2 F; to the last base; N in the run
    ]
    return [bytes(g) for g in genomes], lcbs


def expected(genomes, lcbs, F, printable):
    head = "#FormatVersion Mauve\n#SequenceCount %d\n" % len(genomes)
    for i in range(len(genomes)):
        head += "##SequenceIndex %d\n##SequenceFile g%d.fna\n##SequenceHeader >h%d\n##SequenceLength %dbp\n" % (i + 1, i + 1, i + 1, len(genomes[i]) - i)
    text = head + "#IntervalCount %d\n" % printable
    for g, c in enumerate(X.covered_of(lcbs, genomes)):
        edges = np.flatnonzero(np.diff(np.concatenate(([0], c.astype(np.int8), [0]))))
        text += "covered %d" % (g + 1) + "".join(" %d-%d" % (a, b) for a, b in zip(edges[::2], edges[1::2])) + "\n"
    flanks_all = []
    for cluster, side, recs, flanks in X.jobs_of(lcbs, genomes, X.params(max_flank=F)):
        flanks_all.append(flanks)
        text += "job %d %s" % (cluster, side)
        for (seq, _, _, _, _), (first, step, comp, letters) in zip(recs, flanks):
            text += " (%d %d %d %d %d)" % (seq - 1, step, comp, len(letters), first if letters else 0)
        text += "\n"
        for r, ((seq, _, _, strand, _), (first, step, _, letters)) in enumerate(zip(recs, flanks)):
            used = min(len(letters), 3 + 5 * r)
            ends = sorted((first, first + (used - 1) * step))
            row = "".join("ACGT"[(k + r) % 4] for k in range(163))
            row = row[::-1] if side == "L" else row
            text += "> %d:%d-%d %s cluster%d %s\n" % ((seq,) + ((ends[0] + 1, ends[1] + 1) if used else (0, 0)) + (strand, cluster, side))
            text += "".join(row[k:k + 80] + "\n" for k in range(0, 163, 80))
        text += "=\n"
    return text, flanks_all


@pytest.mark.parametrize("F", [16, 64, 512])
def test_flanks_and_text(checker, tmp_path, F):
    genomes, lcbs = design(F, F)
    path = str(tmp_path / "in.txt")
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (len(genomes), F, len(lcbs) + 2))
        for i, g in enumerate(genomes):
            f.write("g%d.fna >h%d %d %s\n" % (i + 1, i + 1, len(g) - i, g.decode()))
        f.write("%d\n" % len(lcbs))
        for recs in lcbs:
            f.write("%d %d\n" % (recs[0][4], len(recs)))
            for seq, lo, hi, strand, _ in recs:
                f.write("%d %d %d %d\n" % (seq, lo, hi, strand == "+"))
    p = subprocess.run([checker, path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    text, flanks = expected(genomes, lcbs, F, len(lcbs) + 2)
    assert p.stdout == text
    lens = {(z, s, r): len(fl[3]) for (z, s), rows in zip(((z, s) for z in range(len(lcbs)) for s in "LR"), flanks) for r, fl in enumerate(rows)}
    # the design's points, in the restatement's own numbers: halves of even and odd runs, flanks of 0 and 1 bases, the N stops, the genome's ends
    assert lens[0, "R", 0] == min(F, 30) and lens[1, "L", 0] == min(F, 30)            # 60 between LCB 1 and 2 on genome 1: 30 + 30
    assert lens[0, "R", 1] == min(F, 27) and lens[1, "L", 1] == min(F, 15)            # 54 on genome 2: 27 + 27, the upper half cut by the N run at 131 ... 134
    assert lens[0, "L", 1] == 0 and lens[0, "L", 0] == min(F, 10)                      # a record at base 1; ten bases to the genome's start, all of them
    assert lens[1, "R", 0] == 1 and lens[2, "L", 0] == 0                              # one base apart: the low side takes it
    assert lens[2, "R", 0] == 2 and lens[3, "L", 0] == 1                              # three apart: 2 + 1
    assert lens[1, "R", 2] == 0 and lens[1, "L", 2] == 1 and lens[2, "L", 2] == 0     # genome 3, reverse row: its side R touches LCB 1, its side L reads upwards and takes the one base
    assert lens[4, "R", 1] == 0 and lens[4, "R", 0] == min(F, 10)                     # to the last base; ten bases to the genome's end
    assert lens[4, "L", 2] == 419 - 396 if F > 23 else lens[4, "L", 2] == F            # the N at 396 (1-based) ends the flank read downwards from 419
    # a run of 2 F + 5 bases: the low side's half, capped at F; at F = 512 the next record would begin past the genome (lo > hi covers nothing) and the run reaches the end
    assert lens[3, "R", 0] == (min(F, (2 * F + 5 + 1) // 2) if F < 512 else 350)
