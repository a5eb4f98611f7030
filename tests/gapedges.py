"""Designed inputs for the four forms of the device gap aligner (parsnp_amd/csrc/engine/gapalign_hip.hip): blocks built to put a DP
stripe boundary, a hand-over ring wrap, a ballot word, an 8-bit counter wrap or a capacity limit exactly on the edge, where the
seeded families (gapgen, widegen, tallgen, longgen) reach such a place by luck or not at all.  Deterministic; the reference's rows
of every block are recorded in tests/golden/muscle_edge_runs.json.xz (tests/golden/make_gap_edge_runs.py).

Which string is which profile.  A two-sequence block has one distance d(0, 1), so both row minima of the guide tree are d and both
nearest-neighbour entries point at the other sequence.  wave_argmin keeps the lower index on equal values, so lmin = 0 and rmin =
nearest[0] = 1; the one internal node gets left = 0, right = 1, and the progressive step aligns left as profile A (a lane per row,
`la` = len(block[0])) against right as profile B (`lb` = len(block[1]) columns).  tests/test_gap_edges.py checks this once on the
reference's record and on the host restatement: two alignments of AACAAA and CCACAC score alike, and in either order of the two the
string at index 0 gets the leading gap ("narrow order ab" / "ba"); and the straddle floors find the deletion runs at the rows of
sequence 0 they were placed at.

CONSTANTS is what the generator assumes of the kernel; test_generator_matches_the_kernel reads the same numbers out of the source."""
import collections
import os
import random

import gapgen
import widegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUSCLE_EDGE_GOLDEN = os.path.join(ROOT, "tests", "golden", "muscle_edge_runs.json.xz")

CONSTANTS = dict(kMaxCols=96, kWideSeq=320, kWideCols=640, kMaxSeqs=512, kTallSeqs=2048, kLongSeqs=512, kLongSeq=1024, kLongCols=2048,
                 kLongChunk=64, kLongLag=2, kLongRing=256, kLongThreads=256)
# per form: (sequences, bases of a string, columns of an alignment)
LIMITS = {"narrow": (512, 96, 96), "wide": (512, 320, 640), "tall": (2048, 320, 640), "long": (512, 1024, 2048)}
# per entry point: the forms it has, most sequences, most bases
ENTRIES = {"batch": (("narrow",), 512, 96), "wide": (("narrow", "wide"), 512, 320), "tall": (("narrow", "wide", "tall"), 2048, 320),
           "long": (("narrow", "wide", "long"), 512, 1024)}
WILD = "MRWSYKVHDBXN"

LONG_LA = (1, 2, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 320, 321, 322, 512, 513, 1023, 1024)      # against lb in LONG_LA_LB
LONG_LA_LB = (321, 386)
LONG_LB = (1, 2, 64, 65, 66, 129, 130, 255, 256, 257, 258, 322, 1023, 1024)                                  # against la in LONG_LB_LA
LONG_LB_LA = (321, 385)
LONG_CORNERS = ((1024, 1024), (1023, 1024), (1024, 1), (1, 1024))
WIDE_LENGTHS = (97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320)       # each against 97 and against 320, both ways round
NARROW_LENGTHS = (1, 2, 63, 64, 65, 95, 96)                                       # all pairs
STRADDLE_ROWS = (54, 246, 310)       # a 20-base run of sequence 0 from each of these rows (0-based): across rows 64, 256 and 320
STRADDLE_COL = 246                   # ... and one of sequence 1 from this column: across the ring's column 256
RUN = 20
FIRSTS_130 = (0, 63, 64, 65, 127, 128, 129)
FIRSTS_257 = FIRSTS_130 + (255, 256)
COUNTS = (2, 3, 63, 64, 65, 128, 129, 255, 256, 257, 512)
TALL_COUNTS = (513, 576, 577, 2047, 2048)
UNRELATED_MOST = 1024                # the longest string of an "unrelated" pair (the record stays far below the size of its neighbours with all of them)

Case = collections.namedtuple("Case", "name block")


def _s(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _fit(rng, s, n):
    return (s + _s(rng, max(0, n - len(s))))[:n]


def form_of(block):
    """the form a job of this block runs in at the entry point that takes it (align_groups: by sequences, then by its longest string)"""
    w = max(len(s) for s in block)
    return "tall" if len(block) > 512 else ("long" if w > 320 else ("wide" if w > 96 else "narrow"))


def pair_kinds(rng, la, lb):
    """the kinds of one (la, lb): copy, unrelated, the two repeats, the straddles -> [(kind, [sequence 0, sequence 1])]"""
    out = []
    base = _s(rng, max(la, lb))
    out.append(("copy", [_fit(rng, gapgen.mutate(rng, base, 0.1), la), _fit(rng, gapgen.mutate(rng, base, 0.1), lb)]))
    if max(la, lb) <= UNRELATED_MOST:
        out.append(("unrelated", [_s(rng, la), _s(rng, lb)]))
    n = max(la, lb)
    out.append(("repeatA", ["A" * la, "A" * lb]))
    out.append(("repeatAC", [("AC" * n)[:la], ("CA" * n)[:lb]]))
    # straddle: a copy in which sequence 0 has RUN bases of its own from each row of STRADDLE_ROWS that fits -- sequence 1 lacks them,
    # so the alignment deletes them: the D state carried from the last lane of a stripe to the first of the next (outD / inD)
    at = [r for r in STRADDLE_ROWS if r + RUN + 10 <= la]
    if at and la - RUN * len(at) >= 40:
        common = _s(rng, la - RUN * len(at))
        s0, used = "", 0
        for r in at:
            take = r - len(s0)
            s0 += common[used:used + take] + _s(rng, RUN, "T" if common[used + take - 1] != "T" else "G")
            used += take
        s0 += common[used:]
        assert len(s0) == la
        out.append(("straddle0", [s0, _fit(rng, common, lb)]))
    # ... and the same in sequence 1 across column 256: the I state of a lane while the ring index j & 255 wraps
    if lb >= STRADDLE_COL + RUN + 10 and la >= 40:
        common = _s(rng, lb - RUN)
        s1 = common[:STRADDLE_COL] + _s(rng, RUN, "T" if common[STRADDLE_COL - 1] != "T" else "G") + common[STRADDLE_COL:]
        assert len(s1) == lb
        out.append(("straddle1", [_fit(rng, common, la), s1]))
    return out


def long_pair_lengths():
    return ([(la, lb) for la in LONG_LA for lb in LONG_LA_LB] + [(la, lb) for la in LONG_LB_LA for lb in LONG_LB] + list(LONG_CORNERS))


def wide_pair_lengths():
    out = []
    for x in WIDE_LENGTHS:
        for y in (97, 320):
            for p in ((x, y), (y, x)):
                if p not in out:
                    out.append(p)
    return out


def _pairs(seed, lengths, tag):
    rng = random.Random(seed)
    return [Case("%s %dx%d %s" % (tag, la, lb, kind), blk) for la, lb in lengths for kind, blk in pair_kinds(rng, la, lb)]


def long_pairs():
    return _pairs(20261101, long_pair_lengths(), "long")


def wide_pairs():
    """... and "A" * x against "C" * y, which align end to end with one shared column (x + y - 1 columns): one path length in every
    64-column bracket from 65..128 to 577..640, so that the right-to-left re-spelling runs 2, 3, .. 10 chunks"""
    out = _pairs(20261102, wide_pair_lengths(), "wide")
    for k in range(2, 11):
        t = 64 * k - 9
        x = max(97, t + 1 - 320)
        out.append(Case("wide chunks %d" % k, ["A" * x, "C" * (t + 1 - x)]))
    return out


def narrow_pairs():
    """... and "A" * x against "C" * y around 64, 65, 96 and 97 columns (the two-columns-per-lane re-spelling, c2 = lane + 64; 97 columns
    is the decline)"""
    out = _pairs(20261103, [(la, lb) for la in NARROW_LENGTHS for lb in NARROW_LENGTHS], "narrow")
    for t in (64, 65, 96, 97):
        for x in ((t + 1) // 2, (t + 1) // 2 + 1, (t + 1) - 1 if t < 97 else 96):
            out.append(Case("narrow columns %d/%d" % (t, x), ["A" * x, "C" * (t + 1 - x)]))
    # two alignments of these strings score alike, and the tie goes by which string is profile A: the module's docstring
    out += [Case("narrow order ab", ["AACAAA", "CCACAC"]), Case("narrow order ba", ["CCACAC", "AACAAA"])]
    return out


def _pad(rng, s, form):
    """s, made a string of the form: a long block needs a string above 320 bases, a wide one above 96 (the tail starts with a 'C' and
    has no run of A's, so it adds nothing to the 6-mers of a homopolymer in s)"""
    need = {"narrow": 0, "wide": 97, "long": 321}[form]
    return s if len(s) >= need else s + "C" + _s(rng, need + 8 - len(s), "CGT")


def counts_and_wildcards(form):
    """6-mer multiplicities at the 8-bit wrap, strings shorter than a 6-mer, N in every 6-mer, and the wildcard alphabet"""
    rng = random.Random(20261104 + len(form))
    out = []
    short = ["ACGTA", "ACGTAC", "ACGTACG"]
    if form != "narrow":      # (260 A's do not fit the narrow form)
        runs = ["A" * 260, "A" * 261, "A" * 262]
        if form == "long":
            runs = [r + "C" + _s(rng, 70, "CGT") for r in runs]
        out.append(Case("%s counts 255 256 257" % form, runs))
        out.append(Case("%s counts beside short strings" % form, runs + short))
        # ... and the wrap deciding the guide tree: P and Q share a run of 261 (262) A's, whose 6-mer counts 256 -> 0 (257 -> 1), so
        # by the reference's counts P is nearest to R, which shares P's tail -- with counts that did not wrap it would be nearest to Q
        tail = 70 if form == "long" else 58
        for run in (261, 262):
            t1, t2 = _s(rng, tail, "CGT"), _s(rng, tail, "CGT")
            out.append(Case("%s wrap decides the tree %d" % (form, run), [_s(rng, 50, "CGT") + t1[:50] + _s(rng, 20, "CGT"), "A" * run + t1, "A" * run + t2]))
    out.append(Case("%s short strings" % form, [_pad(rng, "ACGTTGCAAC" * 3, form)] + short + ["ACG", "A"]))
    out.append(Case("%s N in every 6-mer" % form, [_pad(rng, "ACGTN" * 12, form), "ACGTN" * 10 + "AC", "CGTNA" * 9, "ACGTACGTAC"]))
    length = {"narrow": 60, "wide": 200, "long": 340}[form]
    base = _s(rng, length, "ACGT" * 3 + WILD)
    blk = [gapgen.mutate(rng, base, 0.1, "ACGT" * 3 + WILD)[:LIMITS[form][1]] for _ in range(5)]
    blk[0] = _fit(rng, blk[0], length)
    blk[1] = blk[1] + WILD      # every wildcard at least once
    out.append(Case("%s wildcards" % form, [s[:LIMITS[form][1]] for s in blk]))
    out.append(Case("%s X and N" % form, [_pad(rng, "ACXGTXXACGNNXACGT" * 3, form), "ACGGTAXACGTXACGT" * 3, "XXXXXXXX", "ACGTXN"]))
    return out


def _with_firsts(rng, n, firsts, distinct):
    """n strings whose first occurrences sit at `firsts`; everything else repeats an earlier one"""
    out, k = [], 0
    for i in range(n):
        if i in firsts:
            out.append(distinct[k])
            k += 1
        else:
            out.append(out[rng.randrange(len(out))] if i != 1 else out[0])
    return out


def distinct_and_ties(form):
    """the ordered lists across ballot words, u = 1, exact ties in every UPGMA step, zero distances across lanes and rounds, and the
    sequence counts at the strides of the loops.  The big blocks keep one string of the form's length (at index 0) and short ones
    beside it: the cost of a block is its n - 1 pairwise steps."""
    rng = random.Random(20261105 + len(form))
    lead = {"narrow": 12, "wide": 110, "long": 330}[form]
    out = []

    def strings(k):      # k distinct strings: the form's lead first, short ones behind it
        got = [_s(rng, lead)]
        while len(got) < k:
            s = _s(rng, rng.randint(4, 12))
            if s not in got:
                got.append(s)
        return got
    for n, firsts in ((130, FIRSTS_130), (257, FIRSTS_257)):
        out.append(Case("%s firsts %d" % (form, n), _with_firsts(rng, n, firsts, strings(len(firsts)))))
    s, t = strings(2)
    out.append(Case("%s all identical" % form, [s] * 5))
    out.append(Case("%s s t s t" % form, [s, t] * 4))
    blk = strings(128)
    blk = blk[:70] + [blk[5]] + blk[70:]          # (5, 70) are the same string
    blk = blk[:129] + [blk[64]]                    # ... and (64, 129)
    assert len(blk) == 130 and blk[70] == blk[5] and blk[129] == blk[64] and len(set(blk)) == 128
    out.append(Case("%s zero pairs 5-70 64-129" % form, blk))
    for n in COUNTS:
        hap = strings(6)
        out.append(Case("%s count %d" % (form, n), [hap[0]] + [hap[rng.randrange(1, 6)] if i >= 6 else hap[i % 6] for i in range(1, n)]))
    return out


def long_many():
    """one string of 321..400 bases and the rest 1..12 bases at 255, 256 and 257 sequences: the strides of the 256-thread loops and
    of the partner-per-wavefront loop (b += 4); the short strings are all distinct, so u = n"""
    rng = random.Random(20261106)
    out = []
    for n in (255, 256, 257):
        seen, blk = set(), [_s(rng, rng.randint(321, 400))]
        while len(blk) < n:
            s = _s(rng, rng.randint(1, 12))
            if s not in seen or len(s) < 4:
                seen.add(s)
                blk.append(s)
        out.append(Case("long many %d" % n, blk))
    return out


def tall_blocks():
    rng = random.Random(20261107)
    out = [Case("tall %d" % n, [_s(rng, rng.randint(1, 3)) for _ in range(n)]) for n in TALL_COUNTS]
    out.append(Case("tall 513 wider", [_s(rng, rng.randint(1, 8)) for _ in range(513)]))
    a = _s(rng, 320)
    b = a[:100] + _s(rng, 3) + a[103:200] + a[215:] + _s(rng, 15)
    assert len(a) == len(b) == 320
    out.append(Case("tall 2048x320 two alleles", [a if rng.random() < 0.5 else b for _ in range(2048)]))
    return out


def too_tall():
    """2 049 sequences: outside every form (no reference rows are needed to say so)"""
    return ["ACG"[:1 + i % 3] for i in range(2049)]


TOPICS = collections.OrderedDict([
    ("narrow_pairs", narrow_pairs), ("wide_pairs", wide_pairs), ("long_pairs", long_pairs),
    ("counts_narrow", lambda: counts_and_wildcards("narrow")), ("counts_wide", lambda: counts_and_wildcards("wide")), ("counts_long", lambda: counts_and_wildcards("long")),
    ("distinct_narrow", lambda: distinct_and_ties("narrow")), ("distinct_wide", lambda: distinct_and_ties("wide")), ("distinct_long", lambda: distinct_and_ties("long")),
    ("long_many", long_many), ("tall", tall_blocks),
    ("slots_narrow", lambda: slot_blocks("narrow")), ("slots_wide", lambda: slot_blocks("wide")), ("slots_long", lambda: slot_blocks("long"))])
_cases = {}


def cases(topic):
    if topic not in _cases:
        _cases[topic] = TOPICS[topic]()
    return _cases[topic]


_rows = {}


def reference_rows(topic):
    """the reference's rows of every block of cases(topic) (oracle/_ref/muscle_ref, from its record)"""
    if topic not in _rows:
        _rows[topic] = widegen.reference_align([c.block for c in cases(topic)], golden=MUSCLE_EDGE_GOLDEN)
    return _rows[topic]


# ---- the exact decline predicate

def taken(entry, block, max_cols, ref_cols, row_off, out_bytes, launch_cap=None):
    """(taken, reason): the job is aligned (cols >= 1) if and only if all of: 2 <= n <= the entry point's sequences; every length in
    1 .. min(the entry point's bases, the launch's cap); upper case without 'U'; the reference's column count <= min(max_cols, the
    columns of the form the job ends in); row_off + n * max_cols <= out_bytes.  Progressive alignment never removes a column, so no
    intermediate alignment is wider than the final one.  The form a job ends in: the long form for a string above 320 bases, the
    tall form above 512 sequences; else the wide form (a narrow job that outgrows 96 columns runs again in it), except at
    pm_gap_align_batch, which has the narrow form alone.  ref_cols: a callable, asked only where the other conditions hold.
    reason: None, or the first of "n", "len", "out_bytes", "alphabet", "cols" that declines it."""
    forms, seqs, bases = ENTRIES[entry]
    n = len(block)
    if not 2 <= n <= seqs or max_cols < 1:
        return False, "n"
    most = bases if launch_cap is None else min(bases, launch_cap)
    if not all(1 <= len(s) <= most for s in block):
        return False, "len"
    if row_off + n * max_cols > out_bytes:
        return False, "out_bytes"
    if any(ch.islower() or ch == "U" for s in block for ch in s):
        return False, "alphabet"
    form = form_of(block)
    columns = 96 if entry == "batch" else (LIMITS[form][2] if form in ("long", "tall") else 640)
    if (ref_cols() if callable(ref_cols) else ref_cols) > min(max_cols, columns):
        return False, "cols"
    return True, None


Job = collections.namedtuple("Job", "block max_cols rows why")      # rows: the reference's (None where it was not asked); why: what the case is for
Call = collections.namedtuple("Call", "entry jobs short_by")         # short_by: out_bytes is this much less than the sum of n * max_cols


def _by_name(topic, name):
    k = [c.name for c in cases(topic)].index(name)
    return cases(topic)[k].block, reference_rows(topic)[k]


def capacity_calls(form):
    """per form one or two calls of its entry point (narrow: pm_gap_align_batch) that hold, beside a wider job that makes the launch's
    cap larger: max_cols equal to the reference's column count and one less; a string longer than the job's own max_cols but not
    than the launch's cap; a lower-case letter and a 'U' as the last character of the last sequence; one sequence, no sequence more
    than the limit, a string one base above the limit; and out_bytes exact (first call) and one byte short (second call)"""
    entry = "batch" if form == "narrow" else form
    pairs = {"narrow": ("narrow_pairs", "narrow 63x65 copy", "narrow 96x95 repeatA"), "wide": ("wide_pairs", "wide 97x127 copy", "wide 320x320 copy"),
             "long": ("long_pairs", "long 2x321 copy", "long 512x386 copy"), "tall": ("tall", "tall 513", "tall 513 wider")}[form]
    blk, rows = _by_name(pairs[0], pairs[1])
    big, big_rows = _by_name(pairs[0], pairs[2])
    c = len(rows[0])
    seqs, bases, columns = LIMITS[form]
    assert len(big_rows[0]) > c
    jobs = [Job(big, len(big_rows[0]) + 3, big_rows, "the wider job"), Job(blk, c, rows, "max_cols exact"), Job(blk, c - 1, rows, "max_cols one short")]
    jobs.append(Job(blk, max(len(s) for s in blk) - 1, rows, "a string longer than its own max_cols"))
    lower = blk[:-1] + [blk[-1][:-1] + blk[-1][-1].lower()]
    jobs += [Job(lower, c + 4, None, "lower case last"), Job(blk[:-1] + [blk[-1][:-1] + "U"], c + 4, None, "U last"),
             Job(blk[:1], c + 4, None, "one sequence"), Job(blk, c + 4, rows, "plain")]
    if form in ("narrow", "wide", "long"):
        jobs.append(Job([blk[0], "A" * (ENTRIES[entry][2] + 1)], 2 * ENTRIES[entry][2] + 8, None, "a string above the limit"))
        jobs.append(Job(["ACGT"] * (ENTRIES[entry][1] + 1), 8, None, "a sequence too many"))
    else:
        jobs.append(Job(too_tall(), 8, None, "a sequence too many"))
    jobs.append(Job(blk, c, rows, "last job"))
    return [Call(entry, jobs, 0), Call(entry, jobs, 1)]


def second_wide_run():
    """narrow strings whose alignment has more than 96 columns, given to pm_gap_align_groups_wide: with max_cols above 96 the narrow
    form declines them and the wide form runs them (`again` in align_groups); with max_cols = 96 they stay declined"""
    names = ["narrow columns 97/49", "narrow columns 97/50", "narrow columns 97/96"]
    jobs = []
    for nm in names:
        blk, rows = _by_name("narrow_pairs", nm)
        jobs += [Job(blk, len(rows[0]), rows, "second run, exact"), Job(blk, 96, rows, "no second run"), Job(blk, 200, rows, "second run")]
    blk, rows = _by_name("narrow_pairs", "narrow 96x96 unrelated")
    jobs += [Job(blk, 192, rows, "96x96 unrelated"), Job(blk, len(rows[0]) - 1, rows, "96x96 unrelated one short")]
    blk, rows = _by_name("narrow_pairs", "narrow 63x65 copy")
    jobs.append(Job(blk, 130, rows, "stays narrow"))
    return [Call("wide", jobs, 0)]


def slot_blocks(form):
    """16 tiny blocks of the form: 2 x 1..6 bases, 2 x 97, 2 x 321"""
    rng = random.Random(20261108 + len(form))
    length = {"narrow": None, "wide": 97, "long": 321}[form]
    out = []
    for k in range(16):
        base = _s(rng, length or rng.randint(1, 6))
        out.append(Case("%s slot %d" % (form, k), [base, _fit(rng, gapgen.mutate(rng, base, 0.1), length or rng.randint(1, 6))]))
    return out


def slot_reuse(form, count):
    """`count` tiny jobs of the form, cycling through slot_blocks(form); every seventh is a late decline (max_cols one short of the
    reference's columns), every eleventh an early one (a 'U')"""
    blocks, rows = [c.block for c in cases("slots_" + form)], reference_rows("slots_" + form)
    jobs = []
    for i in range(count):
        blk, want = blocks[i % 16], rows[i % 16]
        if i % 11 == 10:
            jobs.append(Job([blk[0], blk[1][:-1] + "U"], len(want[0]) + 2, None, "early decline"))
        elif i % 7 == 6:
            jobs.append(Job(blk, len(want[0]) - 1, want, "late decline"))
        else:
            jobs.append(Job(blk, len(want[0]) + (i % 3), want, "taken"))
    return Call("batch" if form == "narrow" else form, jobs, 0)


def lay_out(call):
    """-> (row_off per job, out_bytes, per job (taken, reason)) of a Call, rows laid one job after the other"""
    off, row_off = 0, []
    for j in call.jobs:
        row_off.append(off)
        off += len(j.block) * j.max_cols
    out_bytes = off - call.short_by
    caps = {}
    for j in call.jobs:      # the launch's cap: the widest max_cols among the jobs that share the job's form (as extent() of gap_plan.h sizes it)
        f = form_of(j.block)
        caps[f] = max(caps.get(f, 1), min(j.max_cols, LIMITS[f][2]))
    verdict = []
    for j, ro in zip(call.jobs, row_off):
        verdict.append(taken(call.entry, j.block, j.max_cols, (lambda j=j: len(j.rows[0])), ro, out_bytes,
                             launch_cap=None if form_of(j.block) == "narrow" else caps[form_of(j.block)]))
    return row_off, out_bytes, verdict
