"""The host side of parsnp.unalign (parsnp_amd/csrc/host/unalign.cpp: the word-wise scan of a layout bitmap, the records from the runs,
formatted in chunks on several threads) as a stand-alone program under AddressSanitizer and UBSan (tests/emu/unalign_check.cpp, its
own main), on layouts over the sets of tests/unalignruns.py: the counts and the bytes of the file against the restatement's loop.
The layouts are the sets' own (every block marked), the same with marks and holes scattered over them, with the sentinel cleared
(a run that ends AT the last bit of the bitmap), all marked and none marked.  A CPU program: no GPU, nothing loaded into python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import unalignruns as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "emu", "unalign_check_asan")


@pytest.fixture(scope="module")
def checker():
    host = os.path.join(ROOT, "parsnp_amd", "csrc", "host")
    src = [os.path.join(ROOT, "tests", "emu", "unalign_check.cpp"), os.path.join(host, "unalign.cpp")]
    deps = src + [os.path.join(host, "aligner.h"), os.path.join(ROOT, "include", "parsnp_mum.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-w"] + src + ["-o", BIN], check=True)
    return BIN


def layouts(seqs, seed):
    """name -> one bool array of len + 1 per genome"""
    rng = np.random.default_rng(seed)
    out = {}
    for variant in ("scattered", "no_sentinel", "last_all_marked", "all_marked", "none_marked", "last_one_base"):
        lay = []
        for s in seqs:
            m = np.ones(len(s) + 1, bool)
            if variant == "none_marked":
                m[:] = False
            elif variant != "all_marked":
                for _ in range(60):
                    a = int(rng.integers(0, len(s) + 1))
                    a -= a % 64 if rng.random() < 0.5 else 0      # (half of the holes start a word)
                    m[max(0, a - int(rng.integers(0, 3))): a + int(rng.choice([1, 1, 2, 3, 63, 64, 65, 128, 200]))] = False
            m[-1] = variant != "no_sentinel" and variant != "none_marked"
            lay.append(m)
        if variant == "last_all_marked":
            lay[-1][:] = True
        if variant == "last_one_base":      # the last genome's only run has one base: it costs the round and ends the file after the next
            lay[-1][:] = True
            lay[-1][len(lay[-1]) // 2] = False
        out[variant] = lay
    return out


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("name", list(ur.SETS))
def test_scan_and_records_under_sanitizers(checker, tmp_path, name, threads):
    seqs = ur.SETS[name]()
    names = [b"genome%d.fna" % k for k in range(len(seqs))]
    for variant, lay in layouts(seqs, 9).items():
        src, dst = str(tmp_path / (variant + ".in")), str(tmp_path / (variant + ".out"))
        with open(src, "wb") as f:
            f.write(struct.pack("<q", len(seqs)))
            for nm, s, m in zip(names, seqs, lay):
                words = np.packbits(np.concatenate([m, np.zeros(-len(m) % 64, bool)]), bitorder="little").view(np.uint64)
                f.write(struct.pack("<q", len(nm)) + nm + struct.pack("<q", len(s)) + s + struct.pack("<q", len(m)) + words.tobytes())
        p = subprocess.run([checker, src, dst, str(threads)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", OMP_NUM_THREADS=str(threads)))
        assert p.returncode == 0, "%s %s: %s" % (name, variant, p.stderr[-3000:])
        counts = [tuple(int(x) for x in ln.split()) for ln in p.stdout.split("\n") if ln]
        want = [ur.runs_of(m) for m in lay]
        assert counts == [(w[3], len(w[0])) for w in want], (name, variant)
        assert open(dst, "rb").read() == ur.records(lay, names, seqs), "%s %s: the records differ from the loop's" % (name, variant)
