"""The unaligned runs of a layout (parsnp.unalign: include/parsnp_mum.h, pm_store_unalign_count / pm_store_unalign_runs) restated in
plain Python, and a seeded generator of small sets whose layouts put runs where the kernels of store_kernels.h ("the unaligned
runs") and the host's word-wise scan can go wrong.

Restatement.  `runs_of` reads one genome of a layout as tests/storecalls.py's Store.layout() returns it (pm_store_layout: one bool
per base and the sentinel) and lists every maximal stretch of unmarked entries; `records` is the loop of
Aligner::setUnalignableRegions (src/parsnp.cpp:2310-2381) written out: round after round, every genome walks its layout from
where it stopped, marks what it found, and the loop ends after the first round in which the LAST genome finds nothing.

Generator.  A set is a list of shared blocks (every genome holds every block, in the same order: the MUMs of the anchor call)
with private filler between them (the runs).  `from_runs` turns a list of (start, length) of the runs wanted in ONE genome into
block and filler lengths; the other genomes repeat it with a longer or shorter first filler, which moves every later run by
that many bases, so what ends at bit 63 of a word (or at base 4 095 of a genome: the last bit of a wavefront's 64 words) in
one genome starts a word (a block) in the next."""
import numpy as np

WORD, BLOCK = 64, 64 * 64      # bits of an image word; of the 64 words one wavefront takes


# ---------------------------------------------------------------------------------------------------------------- restatement
def runs_of(lay):
    """lay: bool per bit of one genome, sentinel included -> (start, end inclusive, ordinal) of the kept runs (int arrays) and the
    number of all runs"""
    z = np.concatenate([[False], ~np.asarray(lay, bool), [False]])
    edge = np.flatnonzero(z[1:] != z[:-1])
    start, end = edge[0::2], edge[1::2] - 1
    keep = end > start
    return start[keep].astype(np.int64), end[keep].astype(np.int64), np.flatnonzero(keep).astype(np.int64), len(start)


def records(layout, names, seqs):
    """the bytes of parsnp.unalign by the reference's loop, bit by bit, marking as it goes (layout: list of bool arrays; copied)"""
    lay = [np.array(m, bool) for m in layout]
    n = len(lay)
    lastpos = [0] * n
    out = []
    stop = False
    while not stop:
        for k in range(n):
            bm, size = lay[k], len(lay[k])
            startpos = endpos = -1
            m = lastpos[k]
            while m < size and bm[m]:
                m += 1
            if m < size:
                startpos = m
                while m < size and not bm[m]:
                    m += 1
                endpos = m - 1
                bm[startpos:m] = True
                if m < size:
                    lastpos[k] = endpos + 1
            if startpos != endpos:
                out.append(record(k, startpos, endpos, names[k], seqs[k]))
            elif startpos == -1 and k == n - 1:
                stop = True
    return b"".join(out)


def record(k, startpos, endpos, name, seq):
    """one record: end - start bases (the run's last base is dropped), 80 columns, a trailing single character not printed"""
    rec = [b">%d:%d-%d + %s\n" % (k + 1, startpos, endpos, name)]
    avail = min(endpos - startpos, max(0, len(seq) - startpos))
    pos = 0
    while pos + 80 < avail:
        rec.append(seq[startpos + pos: startpos + pos + 80] + b"\n")
        pos += 80
    if pos + 1 < avail:
        rec.append(seq[startpos + pos: startpos + avail] + b"\n")
    if avail == 0:
        rec.append(b"-\n")
    rec.append(b"=\n")
    return b"".join(rec)


def records_closed(layout, names, seqs):
    """the same bytes from the runs: {(r, k): r < runs[k], r <= runs[n - 1], run r of genome k is kept} in the order of (r, k)"""
    per = [runs_of(m) for m in layout]
    last = per[-1][3]
    recs = sorted((int(o), k, int(s), int(e)) for k, (st, en, od, _) in enumerate(per) for s, e, o in zip(st, en, od) if o <= last)
    return b"".join(record(k, s, e, names[k], seqs[k]) for _, k, s, e in recs)


# ---------------------------------------------------------------------------------------------------------------- generator
def from_runs(runs, tail):
    """runs: (start, length) of the runs of one genome, in order and at least 20 bases apart; tail: bases after the last run (0: the
    genome ends with it) -> (block lengths, filler lengths: one more than blocks)"""
    blocks, fillers, at = [], [], 0
    for s, ln in runs:
        if s == 0:
            fillers.append(ln)
        else:
            if not fillers:
                fillers.append(0)
            assert s - at >= 20, (s, at)
            blocks.append(s - at)
            fillers.append(ln)
        at = s + ln
    if tail:
        blocks.append(tail)
        fillers.append(0)
    assert len(fillers) == len(blocks) + 1
    return blocks, fillers


def build(seed, blocks, fillers):
    """blocks: lengths of the shared blocks; fillers[g]: lengths of genome g's private stretches around them -> list of sequences.
    The base next to a block differs from what follows (precedes) the block in a genome without filler there, and between the
    first two genomes that have filler: no block grows into its neighbourhood in every genome at once."""
    rng = np.random.default_rng(seed)
    B = [rng.integers(0, 4, ln).astype(np.int8) for ln in blocks]
    n, m = len(fillers), len(blocks)
    parts = [[None] * (m + 1) for _ in range(n)]
    for s in range(m + 1):
        before = int(B[s - 1][-1]) if s > 0 else -1      # what a genome without filler here has before block s / after block s - 1
        after = int(B[s][0]) if s < m else -1
        seen = 0
        for g in range(n):
            f = fillers[g][s]
            x = rng.integers(0, 4, f).astype(np.int8)
            if f:
                free = [b for b in range(4) if b != before and b != after]
                x[0] = free[seen % len(free)]
                x[-1] = free[seen % len(free)]
                seen += 1
            parts[g][s] = x
    bases = np.frombuffer(b"ACGT", np.uint8)
    seqs = []
    for g in range(n):
        a = [parts[g][0]]
        for s in range(m):
            a += [B[s], parts[g][s + 1]]
        seqs.append(bases[np.concatenate(a)].tobytes())
    return seqs


def shifted(fillers, by):
    out = list(fillers)
    out[0] += by
    assert out[0] >= 0
    return out


# the runs of the design genome of "edges" (21 kb): around the word boundaries 128, 256, ..., whole words, the block boundaries
# 4 096, 8 192, 12 288 and -- by one run of 8 100 bases -- 16 384 and 20 480 with the whole block between them
EDGE_RUNS = [(0, 5),
             (127, 1), (256, 1),                                    # one base: the last bit of a word, the first
             (382, 2), (511, 2), (640, 2),                          # two: ends a word, across, starts one
             (765, 3), (894, 3), (1023, 3), (1152, 3),              # three: ends a word, 2 + 1, 1 + 2, starts one
             (1280, 64), (1409, 63), (1535, 65), (1664, 128),       # a whole word; all but its first bit; a word and the bit before; two words
             (1900, 63), (2048, 65),
             (4094, 2), (8192, 3), (12287, 2),                      # ends at base 4 095; starts a block; across a block boundary
             (12400, 8100),                                         # base 12 400 to 20 499: more than the whole block 16 384 .. 20 479
             (20600, 7)]                                            # the genome's last bases (the sentinel follows)


def edges(seed=3):
    """five genomes of about 20.6 kb: the design genome, the same moved by +1, +2 and -1 bases, and a last genome with FEWER runs (every
    other filler empty) whose last run has one base"""
    blocks, f0 = from_runs(EDGE_RUNS, 0)
    last = [f if i % 2 else 0 for i, f in enumerate(f0)]
    last[-1] = 1
    return build(seed, blocks, [f0, shifted(f0, 1), shifted(f0, 2), shifted(f0, -1), last])


def last_has_more(seed=4):
    """the last genome has MORE runs than the others (their fillers past the eighth are empty): the rounds go on without them"""
    blocks, f0 = from_runs(EDGE_RUNS[:16], 40)
    few = [f if i < 8 else 0 for i, f in enumerate(f0)]
    return build(seed, blocks, [few, shifted(few, 1), shifted(few, 63), f0])


def last_has_none(seed=5):
    """the last genome is blocks only -- no unmarked base, no run: the file holds the first run of every other genome and ends"""
    blocks, f0 = from_runs(EDGE_RUNS[:16], 40)
    return build(seed, blocks, [f0, shifted(f0, 2), shifted(f0, 64), [0] * len(f0)])


def tiny(seed=6):
    """two blocks of 20 bases: genomes of 51 bits (less than a word), 64 bits (exactly one), 65 and 130"""
    return build(seed, [20, 20], [[3, 4, 3], [10, 13, 0], [0, 1, 23], [44, 2, 43]])


def k4(seed=7):
    """ten blocks: genomes of 4 096 bits (one wavefront's words exactly, sentinel in the last bit), 4 097 (a second block of one bit: the
    sentinel), 4 098 with a run in the two last bases (across the block boundary) and 4 032 (63 words)"""
    blocks = [300] * 10
    def fill(total, lastf):
        f = [7, 64, 1, 130, 2, 63, 65, 3, 0, 40, lastf]
        f[3] += total - 3000 - sum(f)
        return f
    return build(seed, blocks, [fill(4095, 0), fill(4096, 1), fill(4097, 2), fill(4031, 5)])


SETS = {"edges": edges, "last_has_more": last_has_more, "last_has_none": last_has_none, "tiny": tiny, "k4": k4}


def floors(layout):
    """what the layouts of a set hold, for the floors of the tests: run lengths by where they lie"""
    got = set()
    for m in layout:
        z = np.concatenate([[False], ~np.asarray(m, bool), [False]])
        edge = np.flatnonzero(z[1:] != z[:-1])
        for s, e in zip(edge[0::2], edge[1::2] - 1):
            ln = int(e - s + 1)
            if ln <= 3:
                if e % WORD == WORD - 1:
                    got.add("len%d_ends_word" % ln)
                if s % WORD == 0:
                    got.add("len%d_starts_word" % ln)
                if s // WORD != e // WORD:
                    got.add("len%d_across_words" % ln)
            if s == 0:
                got.add("starts_at_0")
            if e == len(m) - 2:
                got.add("ends_at_last_base")
            if s % WORD == 0 and ln in (64, 128):
                got.add("whole_words_%d" % ln)
            if ln in (63, 65):
                got.add("len%d" % ln)
            for b in range(BLOCK, len(m) + BLOCK, BLOCK):
                if e == b - 1:
                    got.add("ends_block")
                if s == b:
                    got.add("starts_block")
                if s == b + 1:
                    got.add("starts_block_plus_1")
                if s < b <= e:
                    got.add("across_blocks")
                if s <= b and e >= b + BLOCK - 1:
                    got.add("spans_a_block")
        if not (~np.asarray(m, bool)).any():
            got.add("no_unmarked_base")
        if not np.asarray(m, bool)[:-1].any():
            got.add("no_marked_base")
    return got
