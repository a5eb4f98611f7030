"""The caller's side of the drop-in boundary: write the .ini exactly as the reference's Python driver does and run a
parsnp_core binary on it.

ini text = the reference's template.ini with the placeholder substitutions of `parsnp` write_inifile_1/2
(parsnp:1047-1067, :1097-1133) and the driver's argparse defaults (parsnp:416-469, :554-558)."""
import os
import random
import subprocess

DEFAULTS = dict(anchors="1.1*(Log(S))", mums="1.1*(Log(S))", extend=0, recombfilt=0, threads=1, diagdiff=0.12, aligner=2,
                mincluster=21, clusterd=300, partpos=15000000, unaligned=0, calcmumi=0)

_TEMPLATE = """;Parsnp configuration File
;
[Reference]
file={ref}
reverse=0
[Query]
{files}[MUM]
anchors={anchors}
anchorfile=
anchorsonly=0
calcmumi={calcmumi}
mums={mums}
mumfile=
filter=1
factor=2.0
extendmums={extend}
[LCB]
recombfilter={recombfilt}
cores={threads}
diagdiff={diagdiff}
doalign={aligner}
c={mincluster}
d={clusterd}
q=30
p={partpos}
icr=0
unaligned={unaligned}
[Output]
outdir={outdir}
prefix=parsnp
showbps=1
"""


def driver_order(paths):
    """query order of the reference driver: sorted(), then random.Random(42).shuffle (parsnp:29, :1509-1510)."""
    out = sorted(paths)
    random.Random(42).shuffle(out)
    return out


def ini_text(ref, queries, outdir, snps=None, tree=None, bootstrap=None, bootseed=None, recomb=None, recperms=None, recseed=None, recsites=None, recnear=None,
             lcbext=None, extmax=None, extband=None, extmatch=None, extmismatch=None, extgap=None, extani=None, extmin=None, **kw):
    """snps=1: `snps=1` under [Output] (core SNP columns and SNP distances beside the XMFA: read_snps; the reference ignores the
    key).  tree=1: `tree=1` there (it implies snps=1: the neighbour-joining tree of the SNP distances, read_tree).  bootstrap=B:
    `bootstrap=B` there (it implies tree=1: the tree once more with the support of B bootstrap replicates on its branches,
    read_boot_tree); bootseed=S: the seed of the replicates (default 1).  recomb=1: `recomb=1` there (it implies snps=1: the
    recombination scan of the core SNP columns, read_rec), with recperms=P permutations (default 1000), recseed=S (1), recsites=K
    sites a window (100) and recnear=H (10).  lcbext=1: `lcbext=1` there (every printed LCB grows into its flanks: read_extended), with
    extmax=F the longest flank (default 256), extband=W the band's half-width (50), extmatch, extmismatch, extgap the scores (5, 4,
    2), extani the per cent a row must keep (95) and extmin the shortest kept extension (10).  Without the arguments the text is the reference driver's, byte for byte."""
    p = dict(DEFAULTS, **kw)
    files = "".join("file%d=%s\nreverse%d=0\n" % (i, q, i) for i, q in enumerate(queries, 1))
    text = _TEMPLATE.format(ref=ref, files=files, outdir=outdir, **p)
    if snps is not None:
        text += "snps=%d\n" % int(snps)
    if tree is not None:
        text += "tree=%d\n" % int(tree)
    if bootstrap is not None:
        text += "bootstrap=%d\n" % int(bootstrap)
    if bootseed is not None:
        text += "bootseed=%d\n" % int(bootseed)
    for key, value in (("recomb", recomb), ("recperms", recperms), ("recseed", recseed), ("recsites", recsites), ("recnear", recnear), ("lcbext", lcbext),
                       ("extmax", extmax), ("extband", extband), ("extmatch", extmatch), ("extmismatch", extmismatch), ("extgap", extgap), ("extani", extani),
                       ("extmin", extmin)):
        if value is not None:
            text += "%s=%d\n" % (key, int(value))
    return text


def run_core(core_bin, ref, queries, outdir, timing=None, env=None, timeout=None, **kw):
    """-> (returncode, ini path).  stdout/stderr go to <outdir>/parsnp-aligner.{out,err} like the driver's log dir."""
    os.makedirs(outdir, exist_ok=True)
    ini = os.path.join(outdir, "parsnpAligner.ini")
    with open(ini, "w") as f:
        f.write(ini_text(ref, queries, outdir, **kw))
    e = dict(os.environ if env is None else env)
    if timing:
        e["PARSNP_TIMING"] = timing
    with open(os.path.join(outdir, "parsnp-aligner.out"), "w") as so, open(os.path.join(outdir, "parsnp-aligner.err"), "w") as se:
        rc = subprocess.run([core_bin, ini], stdout=so, stderr=se, cwd=outdir, env=e, timeout=timeout).returncode
    return rc, ini


def read_timing(path):
    """the PARSNP_TIMING record a run_core(..., timing=path) left: one JSON object with the wall-clock split, the counters of the
    search and, for the gaps between adjacent MUMs that the writer aligned, gap_jobs, gap_jobs_wide (a string of more than 96
    bases), gap_longest, gap_device_narrow / gap_device_wide / gap_device_tall (aligned by the device's narrow, wide and tall
    form -- the last takes the gaps of alignments with more than 512 genomes --, with gap_device_*_ms of kernel time), gap_host and gap_host_s (aligned by the host restatement);
    gap_jobs_long (a string of more than 320 bases: a cluster distance above the default) and gap_device_long / gap_device_long_ms (the device's long form);
    gap_device_long_tall / gap_device_long_tall_ms (its long-tall form: more than 512 genomes and a string of more than 320 bases at once)"""
    import json
    with open(path) as f:
        return json.load(f)


def read_snps(outdir, stem="parsnpAligner"):
    """the three files a run with snps=1 leaves beside the XMFA -> (names, letters, rows, dist): the sequence names in header order,
    letters uint8 [n, V] (the rows' letters in the core SNP columns, upper case), rows = [(cluster, column, ref_pos)] per core SNP
    column, dist int32 [n, n] (the number of core SNP columns in which two sequences differ)"""
    import numpy as np
    base = os.path.join(outdir, stem)
    lines = open(base + ".snps.mfa", "rb").read().split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    names = [x[1:].decode() for x in lines[0:-1:2]]
    assert all(x[:1] == b">" for x in lines[0:-1:2])
    letters = np.array([np.frombuffer(x, np.uint8) for x in lines[1:-1:2]], np.uint8).reshape(len(names), -1)
    tsv = open(base + ".snps.tsv").read().split("\n")
    assert tsv[0] == "cluster\tcolumn\tref_pos" and tsv[-1] == ""
    rows = [tuple(int(x) for x in line.split("\t")) for line in tsv[1:-1]]
    dl = open(base + ".snps.dist").read().split("\n")
    assert dl[-1] == "" and dl[0].split("\t") == [""] + names and [x.split("\t")[0] for x in dl[1:-1]] == names
    dist = np.array([[int(x) for x in line.split("\t")[1:]] for line in dl[1:-1]], np.int32).reshape(len(names), len(names))
    return names, letters, rows, dist


def read_tree(outdir, stem="parsnpAligner"):
    """the Newick string a run with tree=1 leaves beside the SNP files (one line: the file without its newline)"""
    text = open(os.path.join(outdir, stem + ".snps.nwk")).read()
    assert text.endswith(";\n") and text.count("\n") == 1
    return text[:-1]


def read_boot_tree(outdir, stem="parsnpAligner"):
    """the Newick string a run with bootstrap=B leaves beside the tree: the text of read_tree with the number of replicate trees that
    hold a branch behind the closing bracket of its node (one line: the file without its newline)"""
    text = open(os.path.join(outdir, stem + ".snps.boot.nwk")).read()
    assert text.endswith(";\n") and text.count("\n") == 1
    return text[:-1]


def read_rec(outdir, stem="parsnpAligner"):
    """the two files a run with recomb=1 leaves beside the SNP files -> (rows, bed): rows = a dict per window of .rec.tsv in order g
    (cluster, first_column, last_column, first_ref, last_ref, sites, phi, le, perms as int, p as printed), bed = the lines of .rec
    (the upstream driver's parsnp.rec: a record per flagged window) without their newlines"""
    lines = open(os.path.join(outdir, stem + ".rec.tsv")).read().split("\n")
    head = lines[0].split("\t")
    assert head == ["cluster", "first_column", "last_column", "first_ref", "last_ref", "sites", "phi", "le", "perms", "p"] and lines[-1] == ""
    rows = []
    for line in lines[1:-1]:
        f = line.split("\t")
        rows.append(dict(zip(head, [int(x) for x in f[:-1]] + [f[-1]])))
    bed = open(os.path.join(outdir, stem + ".rec")).read().split("\n")
    assert bed[-1] == ""
    return rows, bed[:-1]


def read_extended(outdir, stem="parsnpAligner"):
    """the file a run with lcbext=1 leaves beside the XMFA -> (header lines, [(cluster, side, [(seq, lo, hi, strand, letters)])]): a
    job per kept extension in the file's order, side "L" or "R", a record per row with its 1-based inclusive interval (0, 0 for a row
    that contributes no base)"""
    import re
    head, jobs, recs = [], [], []
    for line in open(os.path.join(outdir, stem + ".xmfa.extended")).read().split("\n")[:-1]:
        if line.startswith("#"):
            head.append(line)
        elif line.startswith(">"):
            m = re.fullmatch(r"> (\d+):(\d+)-(\d+) ([+-]) cluster(\d+) ([LR])", line)
            recs.append([int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4), ""])
            key = (int(m.group(5)), m.group(6))
        elif line == "=":
            jobs.append((key[0], key[1], [tuple(r) for r in recs]))
            recs = []
        else:
            recs[-1][4] += line
    assert not recs
    return head, jobs
