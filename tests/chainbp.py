"""Phases C-D for a diagonal difference given in bases (pm_store_chain_begin with diag_diff > 1): a seeded generator of small MUM
lists with designed gaps, and a sequential restatement of the walk of setFinalClusters (src/parsnp.cpp:2563-2719) in that mode --
a MUM whose largest and smallest gap differ by diag_diff or more is neither joined nor does it close the chain (:2684-2692): it
is PASSED, and the next MUM is judged against the chain's last joined MUM.

    B(1) = 0;  v(x) = judge(x, B(x));  B(x + 1) = x where v(x) is JOIN or CLOSE, B(x) where it is PASS

Plain Python and numpy over tests/storecalls.py (its ctypes driver, its Model of the store as the reference would hold it, its
fill test); no engine code.

A list is written as blocks and sites.  A block is unique sequence shared by all genomes: one MUM.  A site lies between two
blocks: a run of r bases that every query genome has substituted (so the MUMs end exactly at it), and per genome an indel behind
the run -- delta > 0 bases inserted, delta < 0 the last bases of the run deleted -- so that the gap between the two MUMs is r in
every genome but r + delta there."""
import numpy as np

import storecalls as sc

JOIN, CLOSE, PASS = 0, 1, 2
WINDOW_BIT = 8
BLOCK = 20      # bases of a block unless said otherwise (the anchor call's minimum MUM length is 16)


# ---------------------------------------------------------------------------------------------------------------- restatement
def judge(m, a, b, d, diag):
    """Aligner::judge_pair (the test of :2596-2700) of store row a against the chain's last MUM b, on the Model's rows"""
    f32 = np.float32
    max_gap, min_gap = f32(0), f32(d + 10)
    for k in range(m.n):
        ns, bs = m.pos(a, k), m.pos(b, k)
        fgap = ns - (bs + m.len[b])
        rgap = bs - (ns + m.len[a])
        fw = bool(m.strand[a, k])
        if fw and f32(fgap) > max_gap:
            max_gap = f32(fgap)
        elif not fw and f32(rgap) > max_gap:
            max_gap = f32(fgap)      # (:2610 assigns the forward gap)
        if fw and f32(fgap) < min_gap:
            min_gap = f32(fgap)
        elif not fw and f32(rgap) < min_gap:
            min_gap = f32(rgap)
        if bool(m.strand[b, k]) != fw:
            return CLOSE
        if (fgap < 0 or fgap > d) if fw else (fgap >= 0 or rgap > d):
            return CLOSE
    if min_gap == 0:
        min_gap = f32(1)
    if max_gap == 0:
        max_gap = f32(1)
    if f32(diag) > 1.0:
        return JOIN if f32(max_gap - min_gap) < f32(diag) else PASS
    return JOIN if np.float64(min_gap / max_gap) >= 1.0 - np.float64(f32(diag)) else CLOSE


def walk(m, rows, d, diag, first=0, back=None):
    """the recurrence from list position `first` on, whose MUM is judged against `back` (None: it opens the list's first chain)
    -> (verdict per MUM, position of the MUM each one was judged against)"""
    v, backs = [], []
    for x in range(first, len(rows)):
        if back is None:
            v.append(CLOSE), backs.append(x)
        else:
            v.append(judge(m, rows[x], rows[back], d, diag)), backs.append(back)
        if v[-1] != PASS:
            back = x
    return v, backs


def windows(v, backs):
    """the runs of passed MUMs -> [(first passed position, passed MUMs, verdict of the MUM that ends the run or None at the list's end)]"""
    out, x = [], 0
    while x < len(v):
        if v[x] != PASS:
            x += 1
            continue
        z = x
        while z < len(v) and v[z] == PASS:
            z += 1
        out.append((x, z - x, v[z] if z < len(v) else None))
        x = z + 1      # (the MUM that ends a run was judged against the run's back: it is no start)
    return out


class Want:
    """what the restatement says to one chain call"""


def chain(m, d, diag, c, cap=4096):
    """phases C-D with a diagonal difference in bases -> Want: pm_chain_info as a dict, rows, the byte per MUM, the counts of
    passed MUMs, the layout afterwards; trouble bit 3 when a run of passed MUMs is longer than cap (nothing has changed then)"""
    w = Want()
    rows, tie = m.sorted_rows()
    v1, b1 = walk(m, rows, d, diag)
    w.v1, w.b1, w.rows1, w.win1 = v1, b1, rows, windows(v1, b1)
    lens = []
    for x, r in enumerate(rows):
        if v1[x] == CLOSE:
            lens.append(0)
        if v1[x] != PASS:
            lens[-1] += m.len[r]
    info = dict(n_in=len(rows), lcbs_first=len(lens), lcbs_dissolved=0, mums_dissolved=0, trouble=1 if tie else 0)
    over = any(p > cap for _, p, _ in w.win1)
    marks = [x.copy() for x in m.marks]
    keep, lcb = [], -1
    for x, r in enumerate(rows):
        lcb += v1[x] == CLOSE
        if v1[x] != PASS and lcb != len(lens) - 1 and lens[lcb] <= c:      # (the last LCB is never examined, :447)
            info["mums_dissolved"] += 1
            info["lcbs_dissolved"] += v1[x] == CLOSE
            for j in range(m.n):
                marks[j][m.pos(r, j): m.pos(r, j) + m.len[r]] = False
        else:
            keep.append(r)
    v2, b2 = walk(m, keep, d, diag)
    w.v2, w.b2, w.win2 = v2, b2, windows(v2, b2)
    over = over or any(p > cap for _, p, _ in w.win2)
    lay = m.layout(marks)
    fillers = w.fillers_over_passed = 0
    for x in range(1, len(keep)):
        if v2[x] == CLOSE:
            add = m.fill(keep[b2[x]], keep[x], lay)[0]
            fillers += add == 1
            w.fillers_over_passed += add == 1 and b2[x] != x - 1
            if add == 2:
                info["trouble"] |= 2
    info.update(n_mums=len(keep), n_lcbs=sum(1 for x in v2 if x == CLOSE), n_fillers=fillers)
    if over:
        info["trouble"] |= WINDOW_BIT
    w.info, w.rows, w.heads = info, keep, [2 if x == PASS else x for x in v2]
    w.passed = (sum(1 for x in v1 if x == PASS), sum(1 for x in v2 if x == PASS))
    w.layout = m.layout() if over else lay
    return w


# ---------------------------------------------------------------------------------------------------------------- generator
def M(length=BLOCK):
    return ("m", length)


def S(r=1, **delta):
    """a site: S(3, g1=25) -- a run of 3 substituted bases and 25 bases inserted behind it in genome 1"""
    return ("s", r, {int(k[1:]): v for k, v in delta.items()})


def SWAP(g):
    """in genome g the last two blocks change places (the sites stay where they are): the later one lies before the earlier one's end there"""
    return ("swap", g)


def INV(g, on):
    """genome g is reverse-complemented from the next block (on) up to the last one (off)"""
    return ("inv", g, on)


def plain(k, length=BLOCK):
    """k blocks one base apart, with a site in front"""
    return [x for _ in range(k) for x in (S(), M(length))]


def build(seed, n, items):
    """-> n sequences (sequence 0 = the reference)"""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", np.uint8)
    assert items[0][0] == "m" and items[-1][0] == "m"
    block = {i: rng.integers(0, 4, it[1]).astype(np.int8) for i, it in enumerate(items) if it[0] == "m"}
    pieces = [[] for _ in range(n)]          # per genome: arrays of codes 0..3
    blocks = [[] for _ in range(n)]          # per genome: the piece index of every block so far
    inv = {}                                 # genome -> [first piece, one past the last piece]
    for i, it in enumerate(items):
        if it[0] == "m":
            for g in range(n):
                blocks[g].append(len(pieces[g]))
                pieces[g].append(block[i])
        elif it[0] == "s":
            _, r, delta = it
            assert all(g < n for g in delta)
            before = block[max(k for k in block if k < i)]
            after = block[min(k for k in block if k > i)]
            run = rng.integers(0, 4, r).astype(np.int8)
            sub = ((run + rng.integers(1, 4, r)) % 4).astype(np.int8)
            for g in range(n):
                a = run if g == 0 else sub
                dl = delta.get(g, 0)
                if dl < 0:
                    assert -dl <= r
                    a = a[:r + dl]
                elif dl > 0:
                    ins = rng.integers(0, 4, dl).astype(np.int8)
                    if r == 0:      # (with no run the insertion alone ends the MUMs on both sides)
                        ins[0] = next(b for b in range(4) if b != after[0] and (dl > 1 or b != before[-1]))
                        ins[-1] = next(b for b in range(4) if b != before[-1] and (dl > 1 or b != after[0]))
                    a = np.concatenate([a, ins])
                pieces[g].append(a)
        elif it[0] == "swap":
            g = it[1]
            a, b = blocks[g][-2], blocks[g][-1]
            pieces[g][a], pieces[g][b] = pieces[g][b], pieces[g][a]
        elif it[2]:
            inv[it[1]] = [len(pieces[it[1]]), None]
        else:
            inv[it[1]][1] = len(pieces[it[1]])
    seqs = []
    for g in range(n):
        if g in inv:
            lo, hi = inv[g]
            mid = np.concatenate(pieces[g][lo:hi])
            pieces[g][lo:hi] = [(3 - mid)[::-1]]
        seqs.append(bases[np.concatenate(pieces[g])].tobytes())
    return seqs


def window(p, end, D, g=1, big=0):
    """a run of p passed MUMs: D + 3 bases inserted in genome g, p blocks, then the block that ends the run -- "join": the same
    bases deleted again (the diagonal is restored), "close": a run of `big` bases, more than d, in front of it"""
    out = [S(3, **{"g%d" % g: D + 3}), M()] + plain(p - 1)
    out += [S(D + 4, **{"g%d" % g: -(D + 3)}), M()] if end == "join" else [S(big), M()]
    return out


# ---------------------------------------------------------------------------------------------------------------- the designed lists
def _bar(D):
    """largest gap less smallest gap of D - 1 (joins), D and D + 1 (passed; the bases are deleted again behind one block), then the
    gaps (0, D), which join only because a smallest gap of 0 counts as 1, and (0, D + 1), which do not"""
    out = [M()] + plain(2) + [S(3, g1=D - 1), M()] + plain(1)
    for k in (D, D + 1):
        out += [S(3, g1=k), M(), S(k + 1, g1=-k), M()] + plain(1)
    out += [S(0, g2=D), M()] + plain(1) + [S(0, g2=D + 1), M(), S(D + 2, g2=-(D + 1)), M()] + plain(2)
    return out


def _inside(D):
    """a run that begins with D + 3 bases inserted in genome 1; inside it genome 2 gains D + 3 bases and loses them again two blocks
    later -- walked from there, that block joins; in truth it is passed, as genome 1 is still off the diagonal"""
    k = D + 3
    return ([M()] + plain(2) + [S(3, g1=k), M()] + plain(1) + [S(3, g2=k), M()] + plain(1) + [S(k + 1, g2=-k), M()] + plain(1)
            + [S(k + 1, g1=-k), M()] + plain(2))


def _reverse(D):
    k = D + 3
    return ([M()] + plain(2) + [S(), INV(3, True), M()] + plain(1) + [S(3, g1=k), M()] + plain(1) + [S(k + 1, g1=-k), M()] + plain(1)
            + [INV(3, False)] + plain(2))


def _second_pass(D):
    """B (30 bases), H (17), P: in genome 2 H lies before B, so H closes B's chain (it begins before B ends there) and is an LCB of
    17 bases; P is passed against H (genome 2: B lies in between) and so are the blocks behind it until the gap exceeds d = 100;
    with H dissolved, P joins B.  Further on two MUMs that stay passed, and a last LCB of one block, which is never examined"""
    return ([M()] + plain(1) + [S(), M(30), S(), M(17), SWAP(2)] + plain(7) + window(2, "join", D) + plain(2) + [S(101), M()])


def _second_pass_run(D):
    """5 blocks passed against A; H, reverse in genome 3, closes A's chain and is an LCB of its own that c = 25 dissolves; the 4
    blocks behind it form an LCB (the first closes H's); with H gone they are passed against A as well: a run of 9 in the
    second pass, of 5 in the first.  Then the diagonal is restored"""
    k = D + 3
    return ([M()] + plain(4) + [S(3, g1=k), M()] + plain(4) + [S(), INV(3, True), M(), INV(3, False)] + plain(4)
            + [S(k + 1, g1=-k), M()] + plain(2) + [S(301), M()] + plain(1))


BIG = 2000      # a cluster distance d that a run of 65 passed blocks stays below
CASES = {
    # name: (genomes, list, d, diag_diff in bases, c, tunables, the runs of passed MUMs of the first pass: (MUMs, what ends them))
    "bar2": (3, _bar(2), 300, 2, 0, {}, [(1, JOIN), (1, JOIN), (1, JOIN)]),
    "bar25": (4, _bar(25), 300, 25, 0, {}, [(1, JOIN), (1, JOIN), (1, JOIN)]),
    "no_pass": (3, [M()] + plain(2) + [S(3, g1=24), M(), S(0, g2=25), M(), S(30, g1=-24), M(), S(301), M()] + plain(2), 300, 25, 0, {}, []),
    "pass_at_1": (3, [M(), S(3, g1=28), M(), S(29, g1=-28), M()] + plain(6), 300, 25, 0, {}, [(1, JOIN)]),
    "pass_last": (3, [M()] + plain(7) + [S(3, g1=28), M()], 300, 25, 0, {}, [(1, None)]),
    "pass_after_head": (3, [M()] + plain(2) + [S(301), M(), S(3, g1=28), M(), S(29, g1=-28), M()] + plain(2), 300, 25, 0, {}, [(1, JOIN)]),
    "pass_before_close": (3, [M()] + plain(3) + window(1, "close", 25, big=301) + plain(3), 300, 25, 0, {}, [(1, CLOSE)]),
    "runs123_join": (5, [M()] + plain(2) + window(1, "join", 25) + plain(2) + window(2, "join", 25, g=4) + plain(2) + window(3, "join", 25, g=2) + plain(2),
                     300, 25, 0, {}, [(1, JOIN), (2, JOIN), (3, JOIN)]),
    "runs123_close": (5, [M()] + plain(2) + window(1, "close", 25, big=301) + plain(2) + window(2, "close", 25, g=4, big=301) + plain(2)
                      + window(3, "close", 25, g=2, big=301) + plain(2), 300, 25, 0, {}, [(1, CLOSE), (2, CLOSE), (3, CLOSE)]),
    "runs123_131": (131, [M()] + plain(2) + window(1, "join", 25, g=130) + plain(2) + window(2, "close", 25, g=70, big=301) + plain(2)
                    + window(3, "join", 25, g=64) + plain(2), 300, 25, 0, {}, [(1, JOIN), (2, CLOSE), (3, JOIN)]),
    "meet_after_join": (4, [M()] + plain(2) + window(2, "join", 25) + window(2, "join", 25, g=2) + plain(2), 300, 25, 0, {}, [(2, JOIN), (2, JOIN)]),
    "meet_after_close": (4, [M()] + plain(2) + window(2, "close", 25, big=301) + window(1, "join", 25, g=2) + plain(2), 300, 25, 0, {}, [(2, CLOSE), (1, JOIN)]),
    "start_inside": (4, _inside(25), 300, 25, 0, {}, [(6, JOIN)]),
    "reverse": (4, _reverse(25), 300, 25, 0, {"flagged_div": 1}, None),
    "second_pass": (4, _second_pass(25), 100, 25, 20, {"flagged_div": 1}, None),
    "filler": (4, [M()] + plain(3) + [S(6, g1=28), M(), S(301), M()] + plain(2), 300, 25, 0, {}, [(1, CLOSE)]),
    "cap_8": (3, [M()] + plain(2) + [S(301), M()] + plain(1) + window(8, "join", 25) + plain(2), 300, 25, 70, {"chain_window": 8}, [(8, JOIN)]),
    "cap_9": (3, [M()] + plain(2) + [S(301), M()] + plain(1) + window(9, "join", 25) + plain(2), 300, 25, 70, {"chain_window": 8}, [(9, JOIN)]),
    "second_pass_cap_8": (4, _second_pass_run(25), 300, 25, 25, {"chain_window": 8, "flagged_div": 1}, None),
    "second_pass_cap_9": (4, _second_pass_run(25), 300, 25, 25, {"chain_window": 9, "flagged_div": 1}, None),
    "tie": (3, [M()] + plain(3) + window(1, "join", 25) + plain(3), 300, 25, 0, {"chain_tie": 1}, [(1, JOIN)]),
}
for _p in (63, 64, 65):
    CASES["run%d_join" % _p] = (3, [M()] + plain(1) + window(_p, "join", 25) + plain(1), BIG, 25, 0, {}, [(_p, JOIN)])
    CASES["run%d_close" % _p] = (3, [M()] + plain(1) + window(_p, "close", 25, big=BIG + 1) + plain(1), BIG, 25, 0, {}, [(_p, CLOSE)])
SMALLEST = "pass_at_1"


def first_diff(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shapes %s and %s" % (got.shape, want.shape)
    x = np.flatnonzero(got != want)
    return None if not len(x) else "first at %d: engine %s, restatement %s (%d differ)" % (x[0], got[x[0]], want[x[0]], len(x))


def same_layout(got, want, what):
    for j, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "%s: layout of genome %d differs first at base %d" % (what, j, int(np.flatnonzero(a != b)[0]))


def check_case(lib, name, seed=7):
    """one chain call on the list of the case: the row list, the byte per MUM, pm_chain_info, pm_store_chain_passed and the layout
    afterwards against the restatement; then the floors that say the list took the path it was designed for"""
    n, items, d, D, c, tune, runs = CASES[name]
    seqs = build(seed, n, items)
    cap = tune.get("chain_window", 4096)
    with sc.Store(lib, seqs, tune=tune) as st:
        rc, _ = st.settle()
        assert rc == sc.PM_OK, "pm_store_settle declined the list (code %d)" % rc
        m = sc.Model(seqs, st.raw_start, st.strand, st.lon, st.flags).settle()
        assert len(m.acc_rows()) == sum(1 for it in items if it[0] == "m"), "%s: %d MUMs from %d blocks" % (name, len(m.acc_rows()), sum(1 for it in items if it[0] == "m"))
        before = st.layout()
        same_layout(before, m.layout(), name + " (settled)")
        w = chain(m, d, float(D), c, cap)
        got, rows, heads = st.chain(len(m.acc_rows()), d, float(D), c)
        passed = st.sess.chain_passed()
        after = st.layout()
    if "chain_tie" in tune:
        assert got["trouble"] & 1, "%s: trouble %d" % (name, got["trouble"])
        same_layout(after, before, name)
        return w
    assert got["trouble"] == w.info["trouble"], "%s: trouble %d, restatement %d" % (name, got["trouble"], w.info["trouble"])
    same_layout(after, w.layout, name)
    if w.info["trouble"] & WINDOW_BIT:
        same_layout(after, before, name)      # (nothing on the device has changed)
        assert runs is None or [(p, e) for _, p, e in w.win1] == runs, "%s: the restatement's runs of passed MUMs are %s" % (name, w.win1)
        return w
    assert got == w.info, "%s: pm_chain_info %s, restatement %s" % (name, got, w.info)
    diff = first_diff(rows, w.rows)
    assert diff is None, "%s: rows: %s" % (name, diff)
    diff = first_diff(heads, w.heads)
    assert diff is None, "%s: heads: %s" % (name, diff)
    assert passed == w.passed, "%s: pm_store_chain_passed %s, restatement %s" % (name, passed, w.passed)
    assert runs is None or [(p, e) for _, p, e in w.win1] == runs, "%s: the restatement's runs of passed MUMs are %s" % (name, w.win1)
    w.model = m
    return w


if __name__ == "__main__":      # `python tests/chainbp.py first LIB`: the smallest list, in a process of its own
    import sys

    from parsnp_amd.binding import Lib
    assert sys.argv[1] == "first"
    check_case(Lib(sys.argv[2]), SMALLEST)
    print("first ok")
