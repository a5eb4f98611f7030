// pair_words_check.cpp -- the bit-plane machinery of the small-region event search, checked on the host against the product's own
// header with no engine around it (tests only; built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_small_pairs.py --
// every helper guards a shift by 64 in its own way, and UBSan's shift checks are the point):
//   1. W64 and W128 against unsigned __int128: ones(n), shr(k), low, run_at(s), clear_below(k) at every n, k and s of their domains
//      (W64: what pair_diagonals asks of it with sides of at most 64 bases -- n <= 64, k <= 63; W128: n, k <= 128), on random
//      words, all ones, and runs that cross bit 63 / 64 or end on bit 127;
//   2. planes64 against the bytes at every p & 31, over sequences packed by the product's PackStrand in the layout of
//      Engine::load_genomes (2 guard blocks before, 2 behind every strand, 8 behind the last) in an allocation of exactly that size:
//      windows that end on the last base of the last strand read the last blocks the engine owns;
//   3. pair_diagonals<W64> and <W128> against a naive enumeration of the maximal runs of every diagonal: every (nR, m) of the
//      length list, every L of the suite's list, on random two-letter strings (many runs), on strings with N, and on pairs with a
//      stretch planted in a corner;
//   4. the (first, step) split for shares of 1, 2, 4, .. 64 lanes: the union is exactly the whole, no event comes twice.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <tuple>
#include <vector>
#include "../../parsnp_amd/csrc/engine/kernels.h"
using namespace pm;
typedef unsigned __int128 u128;

static std::mt19937_64 rng(20240607);
static int fail(const char* what, long a = 0, long b = 0, long c = 0) { printf("pair_words_check: %s (%ld, %ld, %ld)\n", what, a, b, c); return 1; }

static u128 u_ones(int n) { return n >= 128 ? ~(u128)0 : (((u128)1 << n) - 1); }
static u128 u_shr(u128 v, int k) { return k >= 128 ? 0 : v >> k; }
static int u_low(u128 v) { for (int i = 0; i < 128; i++) if ((v >> i) & 1) return i; return 128; }
static int u_run(u128 v, int s, int bits) { int n = 0; while (s + n < bits && ((v >> (s + n)) & 1)) n++; return n; }
static u128 of(const W128& w) { return ((u128)w.hi << 64) | w.lo; }
static W128 to128(u128 v) { W128 w; w.lo = (uint64_t)v; w.hi = (uint64_t)(v >> 64); return w; }

static int check_words() {
    std::vector<u128> words;
    words.push_back(~(u128)0); words.push_back(0); words.push_back((u128)1 << 127); words.push_back((u128)1 << 64); words.push_back((u128)1 << 63);
    for (int a = 0; a < 128; a += 7) for (int n : {1, 2, 63, 64, 65, 127}) if (a + n <= 128) words.push_back(u_ones(n) << a);      // runs: across 63 / 64, ending on 127
    for (int n = 1; n <= 128; n++) words.push_back(u_ones(n) << (128 - n));
    for (int i = 0; i < 300; i++) { u128 v = ((u128)rng() << 64) | rng(); if (i % 3 == 0) v |= ((u128)rng() << 64) | rng(); if (i % 3 == 1) v |= u_ones(40) << (rng() % 89); words.push_back(v); }
    for (int n = 0; n <= 128; n++) if (of(W128::ones(n)) != u_ones(n)) return fail("W128::ones", n);
    for (int n = 0; n <= 64; n++) if (W64::ones(n).v != (uint64_t)u_ones(n)) return fail("W64::ones", n);
    for (size_t i = 0; i < words.size(); i++) {
        const u128 v = words[i]; const W128 w = to128(v);
        W64 h; h.v = (uint64_t)v; const u128 hv = (uint64_t)v;
        if (w.any() != (v != 0) || h.any() != (hv != 0)) return fail("any", (long)i);
        if (v != 0 && w.low() != u_low(v)) return fail("W128::low", (long)i);
        if (hv != 0 && h.low() != u_low(hv)) return fail("W64::low", (long)i);
        if (of(~w) != ~v || (~h).v != ~(uint64_t)v) return fail("operator~", (long)i);
        for (int k = 0; k <= 128; k++) {
            if (of(w.shr(k)) != u_shr(v, k)) return fail("W128::shr", (long)i, k);
            if (of(w.clear_below(k)) != (v & ~u_ones(k))) return fail("W128::clear_below", (long)i, k);
            if (k < 128 && w.run_at(k) != u_run(v, k, 128)) return fail("W128::run_at", (long)i, k, w.run_at(k));
        }
        for (int k = 0; k <= 64; k++) {
            if (k < 64 && h.shr(k).v != (uint64_t)(hv >> k)) return fail("W64::shr", (long)i, k);
            if (h.clear_below(k).v != (uint64_t)(hv & ~u_ones(k))) return fail("W64::clear_below", (long)i, k);
            if (k < 64 && h.run_at(k) != u_run(hv, k, 64)) return fail("W64::run_at", (long)i, k, h.run_at(k));
        }
        const W128 o = to128(words[(i * 7 + 3) % words.size()]);
        if (of(w ^ o) != (v ^ of(o)) || of(w | o) != (v | of(o)) || of(w & o) != (v & of(o))) return fail("W128 ^ | &", (long)i);
    }
    return 0;
}

// the genomes as the engine keeps them: Engine::load_genomes' layout, PackStrand's blocks
struct Store {
    std::vector<std::string> seqs; std::vector<int64_t> goff, glen; std::unique_ptr<SeqBlock[]> blk; int64_t words = 0; Packed P;
    explicit Store(const std::vector<std::string>& s) : seqs(s) {
        words = 2;
        for (const std::string& x : seqs) { glen.push_back((int64_t)x.size()); for (int st = 0; st < 2; st++) { goff.push_back(words * 32); words += ((int64_t)x.size() + 31) / 32 + 2; } }
        words += 8;
        blk.reset(new SeqBlock[(size_t)words]);      // exactly what the engine allocates: a read past it is AddressSanitizer's
        memset(blk.get(), 0, (size_t)words * sizeof(SeqBlock));
        for (size_t g = 0; g < seqs.size(); g++)
            for (int st = 0; st < 2; st++) {
                PackStrand ps{(const uint8_t*)seqs[g].data(), glen[g], st, blk.get(), goff[2 * g + st] / 32};
                for (int64_t t = 0; t < (glen[g] + 31) / 32; t++) ps(t);
            }
        P = Packed{blk.get(), goff.data(), glen.data()};
    }
    // base x of strand st of genome g as the engine defines it: 0..3, 4 = N, -1 = outside (guards: A without N)
    int base(size_t g, int st, int64_t x) const {
        if (x < 0 || x >= glen[g]) return -1;
        const char c = st ? seqs[g][(size_t)(glen[g] - 1 - x)] : seqs[g][(size_t)x];
        const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
        return code == 4 ? 4 : st ? 3 - code : code;
    }
};

static std::string random_string(size_t n, const char* alphabet) { std::string s(n, 'A'); const size_t k = strlen(alphabet); for (char& c : s) c = alphabet[rng() % k]; return s; }

static int check_planes() {
    long windows = 0;
    for (int len : {1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 200, 257}) {
        Store S({random_string(70, "ACGT"), random_string((size_t)len, "ACGTN"), random_string((size_t)len, "ACGTTGCAN")});
        const size_t g = 2;      // the last genome: its reverse strand is the last the engine stores
        for (int st = 0; st < 2; st++)
            for (int64_t x = 0; x < len; x++) {      // every window that begins inside the strand: every p & 31, every distance from its end
                uint64_t b0, b1, nm; planes64(S.P.blk, S.goff[2 * g + st] + x, &b0, &b1, &nm);
                for (int t = 0; t < 64; t++) {
                    const int c = S.base(g, st, x + t);
                    const int w0 = c < 0 || c == 4 ? 0 : c & 1, w1 = c < 0 || c == 4 ? 0 : c >> 1, wn = c == 4;
                    if ((int)((b0 >> t) & 1) != w0 || (int)((b1 >> t) & 1) != w1 || (int)((nm >> t) & 1) != wn) return fail("planes64", len, (long)x, t);
                }
                for (int pl = 0; pl < 3; pl++) {      // the two words of a W128 are the windows at p and p + 64
                    const W128 w = W128::load(S.P.blk, S.goff[2 * g + st] + x, pl);
                    uint64_t a[3], c[3]; planes64(S.P.blk, S.goff[2 * g + st] + x, a, a + 1, a + 2); planes64(S.P.blk, S.goff[2 * g + st] + x + 64, c, c + 1, c + 2);
                    if (w.lo != a[pl] || w.hi != c[pl] || W64::load(S.P.blk, S.goff[2 * g + st] + x, pl).v != a[pl]) return fail("W128::load", len, (long)x, pl);
                }
                windows++;
            }
    }
    printf("planes64: %ld windows\n", windows);
    return 0;
}

typedef std::tuple<int, int, int> Ev;      // (l0, j0, len)
// every maximal run of equal symbols (N equals N and nothing else) of at least L on every diagonal, from the bytes
static std::vector<Ev> naive(const std::string& r, const std::string& q, int L) {
    std::vector<Ev> out;
    const int nR = (int)r.size(), m = (int)q.size();
    auto code = [](char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' ? c : 'N'; };
    for (int d = -(m - 1); d <= nR - 1; d++) {
        int l = d > 0 ? d : 0, j = l - d, run = 0;
        for (;; l++, j++) {
            const bool in = l < nR && j < m, eq = in && code(r[(size_t)l]) == code(q[(size_t)j]);
            if (eq) { run++; continue; }
            if (run >= L) out.emplace_back(l - run, j - run, run);
            run = 0;
            if (!in) break;
        }
    }
    std::sort(out.begin(), out.end());
    return out;
}

template <class W>
static std::vector<Ev> scan(const Store& S, int64_t rpos, int64_t qpos, int nR, int m, int L, int first = 0, int step = 1) {
    std::vector<Ev> out;
    pair_diagonals<W>(S.P, rpos, qpos, nR, m, L, [&](int32_t l0, int32_t j0, int32_t len) { out.emplace_back(l0, j0, len); }, first, step);
    return out;
}

static const int kLengths[] = {1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128};
static const int kL[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128};

static int check_one(const std::string& r, const std::string& q, int L, int off_r, int off_q, long* events) {
    // the pair as windows inside longer genomes, so that both sides begin at any p & 31 and are followed by other bases (the
    // validity masks of pair_diagonals, not the guards, end the sides); the query also as the LAST strand: genome 2 holds its
    // reverse complement at its very end
    const int nR = (int)r.size(), m = (int)q.size();
    std::string rc(q.rbegin(), q.rend());
    for (char& c : rc) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    Store S({random_string((size_t)off_r, "ACGT") + r + random_string(5, "ACGT"), random_string((size_t)off_q, "ACGT") + q + random_string(3, "ACGT"), rc + random_string((size_t)off_q, "ACGT")});
    const int64_t rpos = S.goff[0] + off_r;
    const int64_t qpos[2] = {S.goff[2] + off_q, S.goff[5] + (S.glen[2] - 0 - m)};      // (the reverse base glen - qs - m at qs = 0)
    const std::vector<Ev> want = naive(r, q, L);
    for (int where = 0; where < 2; where++) {
        std::vector<Ev> wide = scan<W128>(S, rpos, qpos[where], nR, m, L);
        const size_t n = wide.size();
        std::sort(wide.begin(), wide.end());
        if (std::adjacent_find(wide.begin(), wide.end()) != wide.end()) return fail("pair_diagonals<W128>: an event twice", nR, m, L);
        if (wide != want) return fail("pair_diagonals<W128> differs from the naive enumeration", nR, m, L);
        if (nR <= 64 && m <= 64) {
            std::vector<Ev> narrow = scan<W64>(S, rpos, qpos[where], nR, m, L);
            std::sort(narrow.begin(), narrow.end());
            if (narrow != want) return fail("pair_diagonals<W64> differs from the naive enumeration", nR, m, L);
        }
        for (int share = 1; share <= 64; share *= 2) {      // the lanes of one (piece, strand) task split its diagonals
            std::vector<Ev> all;
            for (int sub = 0; sub < share; sub++) {
                const std::vector<Ev> part = nR <= 64 && m <= 64 ? scan<W64>(S, rpos, qpos[where], nR, m, L, sub, share) : scan<W128>(S, rpos, qpos[where], nR, m, L, sub, share);
                all.insert(all.end(), part.begin(), part.end());
            }
            if (all.size() != n) return fail("the (first, step) split loses or repeats events", nR, m, share);
            std::sort(all.begin(), all.end());
            if (all != want) return fail("the (first, step) split differs from the whole", nR, m, share);
        }
        *events += (long)n;
    }
    return 0;
}

static int check_diagonals() {
    long events = 0, pairs = 0; int turn = 0;
    for (int nR : kLengths) for (int m : kLengths) {
        const int shorter = nR < m ? nR : m;
        for (int L : kL) {
            if (L > shorter) continue;
            turn++;
            // random two-letter strings: many runs on every diagonal
            if (check_one(random_string((size_t)nR, "AC"), random_string((size_t)m, "AC"), L, turn % 32, (turn * 5 + 1) % 32, &events)) return 1;
            // N on both sides (N equals N only)
            if (turn % 3 == 0 && check_one(random_string((size_t)nR, "ACNN"), random_string((size_t)m, "CANN"), L, (turn * 7) % 32, (turn * 3) % 32, &events)) return 1;
            // a stretch of exactly L bases in each corner of two unrelated strings, and the whole shorter side
            std::string r = random_string((size_t)nR, "ACGT"), q = random_string((size_t)m, "ACGT");
            switch (turn % 5) {
                case 0: q.replace(0, (size_t)L, r, 0, (size_t)L); break;
                case 1: q.replace((size_t)(m - L), (size_t)L, r, 0, (size_t)L); break;                       // the outermost diagonal d = -(m - L)
                case 2: q.replace(0, (size_t)L, r, (size_t)(nR - L), (size_t)L); break;                      // ... and d = nR - L
                case 3: q.replace((size_t)(m - L), (size_t)L, r, (size_t)(nR - L), (size_t)L); break;
                default: q.replace(0, (size_t)shorter, r, 0, (size_t)shorter); break;
            }
            if (check_one(r, q, L, (turn * 11 + 31) % 32, (turn * 13 + 31) % 32, &events)) return 1;
            pairs += 2;
        }
    }
    // homopolymers: one run per diagonal, each as long as the diagonal (len 128 on the main one)
    if (check_one(std::string(128, 'A'), std::string(128, 'A'), 1, 31, 1, &events) || check_one(std::string(128, 'A'), std::string(127, 'A') + "C", 127, 0, 31, &events) ||
        check_one(std::string(64, 'A'), std::string(64, 'A'), 64, 5, 9, &events) || check_one(std::string(128, 'N'), std::string(128, 'N'), 128, 7, 3, &events)) return 1;
    printf("pair_diagonals: %ld pairs, %ld events\n", pairs, events);
    return events > 100000 ? 0 : fail("too few events: the strings stopped producing runs", events);
}

int main() {
    if (check_words() || check_planes() || check_diagonals()) return 1;
    printf("pair_words_check ok\n");
    return 0;
}
