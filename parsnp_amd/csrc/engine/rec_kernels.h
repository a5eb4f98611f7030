// rec_kernels.h -- recombination scan of the core SNP columns: the pairwise homoplasy index of windows of informative sites and its
// permutation test (pm_rec_sites, pm_rec_incompat, pm_rec_test of include/parsnp_mum.h; the definition is INTEGRATION.md §1d).
// All of it is integer work over the collection's bit planes (snp_kernels.h).
//
//   tp            the planes the other way round: per core SNP column a bit set over the ROWS, [column][plane][RB] 64-bit words,
//                 RB = ceil(n / 64); bits of rows >= n are zero (so the rows with letter code 0 are ~lo & ~hi & the valid-row word)
//   flag          per column 1 where it is informative (at least two letters occur in at least two rows each)
//   inc           per window of k sites a k x k byte matrix of pair scores 0 ... 9, the windows packed one after the other
//   phi, le       per window the statistic at identity order and the number of permutations that do not exceed it
//
// RecTranspose (a wavefront per plane word and block of 64 rows) -> RecInform (a lane per column); RecIncompat (a wavefront per window
// and tile of 8 x 8 site pairs, a pair per lane); RecPermute (a wavefront per window and chunk of kRecChunk permutations, the
// window's matrix in LDS; a permutation at a time, the lanes over its sites).  The bodies are written once for the device and the
// emulation (store_kernels.h, "lanes"); every loop has a constant trip count or one that is uniform over the wavefront, no lane
// polls memory, no wavefront waits for another, and wave_sync and the LDS traffic stand where all 64 lanes arrive.
#pragma once
#include "boot_kernels.h"

namespace pm {

constexpr int kRecMaxSites = 256;        // sites of a window
constexpr int kRecMaxPerms = 65536;
constexpr int kRecTile = 8;              // RecIncompat: a wavefront takes kRecTile x kRecTile pairs of sites
constexpr int kRecSlab = 8;              // ... and stages kRecSlab row words of its 2 x kRecTile sites at a time
constexpr int kRecChunk = 64;            // RecPermute: permutations a wavefront works off

// the valid-row word of row block b: ones for the rows b * 64 ... that exist
PM_HD uint64_t rec_valid_word(int32_t nrows, int32_t b) {
    const int32_t left = nrows - b * 64;
    return left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1;
}

// ---------------------------------------------------------------------------------------------------------------- transposed planes
// One wavefront per (plane word w, block of 64 rows rb): lane t loads the word of row 64 rb + t in both planes (zero past the last
// row); the ballot of bit c over the lanes is the row word of column 64 w + c, which lane c keeps and stores.
struct RecTranspose {
    const uint64_t* lo; const uint64_t* hi; int32_t nrows; int64_t V; int32_t RB; uint64_t* tp;      // tp[(col * 2 + plane) * RB + rb]
    PM_HD void wave(int64_t item) const {
        const int64_t w = item / RB; const int32_t rb = (int32_t)(item % RB);
        uint64_t l[kLaneSlots], h[kLaneSlots], ol[kLaneSlots], oh[kLaneSlots];
        lanes_for(0, 64, [&](int t) {
            const int64_t r = (int64_t)rb * 64 + t;
            l[lane_slot(t)] = r < nrows ? lo[w * nrows + r] : 0ull;
            h[lane_slot(t)] = r < nrows ? hi[w * nrows + r] : 0ull;
            ol[lane_slot(t)] = 0; oh[lane_slot(t)] = 0;
        });
#pragma unroll 8
        for (int c = 0; c < 64; c++) {
            const uint64_t bl = wave_ballot_of([&](int t) { return ((l[lane_slot(t)] >> c) & 1) != 0; });
            const uint64_t bh = wave_ballot_of([&](int t) { return ((h[lane_slot(t)] >> c) & 1) != 0; });
            lanes_for(0, 64, [&](int t) { if (t == c) { ol[lane_slot(t)] = bl; oh[lane_slot(t)] = bh; } });
        }
        lanes_for(0, 64, [&](int t) {
            const int64_t col = w * 64 + t;
            if (col < V) { tp[(col * 2 + 0) * RB + rb] = ol[lane_slot(t)]; tp[(col * 2 + 1) * RB + rb] = oh[lane_slot(t)]; }
        });
    }
};
// one lane per column: the rows of each letter by population counts; informative when two letters have two rows or more
struct RecInform {
    const uint64_t* tp; int32_t nrows; int32_t RB; uint8_t* flag;
    PM_HD void operator()(int64_t col) const {
        const uint64_t* L = tp + (col * 2 + 0) * RB;
        const uint64_t* H = tp + (col * 2 + 1) * RB;
        int32_t c1 = 0, c2 = 0, c3 = 0;
        for (int32_t b = 0; b < RB; b++) {
            const uint64_t l = L[b], h = H[b];
            c1 += __builtin_popcountll(l & ~h); c2 += __builtin_popcountll(~l & h); c3 += __builtin_popcountll(l & h);
        }
        const int32_t c0 = nrows - c1 - c2 - c3;
        flag[col] = (uint8_t)(((c0 >= 2) + (c1 >= 2) + (c2 >= 2) + (c3 >= 2)) >= 2);
    }
};

// ---------------------------------------------------------------------------------------------------------------- pair scores
// inc of a 4 x 4 edge mask, bit a * 4 + b: letter a at x and letter b at y share a row.  E edges, Vx non-empty rows, Vy non-empty
// columns, C connected components: the rows' column sets are closed under "shares a column" (three sweeps over the six pairs of rows
// reach every path of four rows), after which the rows of one component hold the same set and those of different ones disjoint
// sets; a component is counted at its first row.  Every non-empty column belongs to a row, so the rows' components are all.
PM_HD int32_t rec_score(uint32_t mask) {
    uint32_t r[4];
#pragma unroll
    for (int a = 0; a < 4; a++) r[a] = (mask >> (4 * a)) & 15u;
    const int32_t E = __builtin_popcount(mask);
    const int32_t Vx = (r[0] != 0) + (r[1] != 0) + (r[2] != 0) + (r[3] != 0);
    const int32_t Vy = __builtin_popcount(r[0] | r[1] | r[2] | r[3]);
#pragma unroll
    for (int sweep = 0; sweep < 3; sweep++)
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = a + 1; b < 4; b++) {
                const uint32_t u = (r[a] & r[b]) ? (r[a] | r[b]) : 0u;
                r[a] |= u; r[b] |= u;
            }
    int32_t C = 0;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        bool first = r[a] != 0;
#pragma unroll
        for (int b = 0; b < a; b++) first = first && (r[a] & r[b]) == 0;
        C += first;
    }
    return E - Vx - Vy + C;
}
// One wavefront per (window of the batch, tile of kRecTile x kRecTile pairs of its sites); lane (a, b) owns the pair of sites
// x = 8 ti + a and y = 8 tj + b.  The row words of the 2 x 8 sites go through LDS in slabs of kRecSlab words per plane (a site's
// line is padded by one word: the eight a's and the eight b's of a wavefront read different banks, equal addresses broadcast), so
// the LDS a window needs does not grow with the rows.  Per row word: the four letter sets of either site, then 16 ANDs, each folded
// into a 32-bit accumulator by one three-way OR.  Only tiles with tj >= ti compute; both halves are written, the diagonal as 0.
struct RecIncompat {
    const uint64_t* tp; int32_t nrows; int32_t RB;
    const int64_t* sites; const int64_t* win_off; const int64_t* mat_off;      // of the batch's windows: win_off[w] ... win_off[w + 1] into sites
    int32_t tiles;                                                             // tiles per side of the largest window of the batch
    uint8_t* inc;                                                              // window w: inc + mat_off[w], k x k
    PM_HD void wave(int64_t item) const {
        const int64_t tt = (int64_t)tiles * tiles;
        const int64_t w = item / tt; const int32_t tile = (int32_t)(item % tt);
        const int32_t ti = tile / tiles, tj = tile % tiles;
        const int64_t s0 = win_off[w];
        const int32_t k = (int32_t)(win_off[w + 1] - s0);
        if (tj < ti || tj * kRecTile >= k) return;      // (uniform)
        constexpr int kLine = 2 * kRecSlab + 1;
        PM_WAVE_SHARED uint64_t sh[2][kRecTile][kLine];
        uint32_t acc[kLaneSlots][16];
        lanes_for(0, 64, [&](int t) {
#pragma unroll
            for (int e = 0; e < 16; e++) acc[lane_slot(t)][e] = 0;
        });
        constexpr int kPer = 2 * kRecTile * 2 * kRecSlab / 64;      // slab entries per lane
        for (int32_t b0 = 0; b0 < RB; b0 += kRecSlab) {
            uint64_t got[kLaneSlots][kPer];
            lanes_for(0, 64, [&](int t) {
#pragma unroll
                for (int q = 0; q < kPer; q++) {
                    const int e = q * 64 + t;
                    const int wd = e % kRecSlab, plane = e / kRecSlab % 2, site = e / (2 * kRecSlab) % kRecTile, side = e / (2 * kRecSlab * kRecTile);
                    const int32_t pos = (side ? tj : ti) * kRecTile + site;
                    uint64_t v = 0;
                    if (pos < k && b0 + wd < RB) v = tp[(sites[s0 + pos] * 2 + plane) * RB + b0 + wd];
                    got[lane_slot(t)][q] = v;
                }
            });
            lanes_for(0, 64, [&](int t) {
#pragma unroll
                for (int q = 0; q < kPer; q++) {
                    const int e = q * 64 + t;
                    const int wd = e % kRecSlab, plane = e / kRecSlab % 2, site = e / (2 * kRecSlab) % kRecTile, side = e / (2 * kRecSlab * kRecTile);
                    sh[side][site][plane * kRecSlab + wd] = got[lane_slot(t)][q];
                }
            });
            wave_sync();
            lanes_for(0, 64, [&](int t) {
                const int a = t >> 3, b = t & 7;
                // (two row words at a time: unrolled over the slab the letter sets of all eight took 182 registers, two wavefronts a SIMD)
#pragma unroll 2
                for (int wd = 0; wd < kRecSlab; wd++) {
                    const uint64_t valid = rec_valid_word(nrows, b0 + wd);      // (zero past the last row word: the staged words are zero there too)
                    const uint64_t xl = sh[0][a][wd], xh = sh[0][a][kRecSlab + wd], yl = sh[1][b][wd], yh = sh[1][b][kRecSlab + wd];
                    const uint64_t X[4] = {~xl & ~xh & valid, xl & ~xh, ~xl & xh, xl & xh};
                    const uint64_t Y[4] = {~yl & ~yh & valid, yl & ~yh, ~yl & yh, yl & yh};
#pragma unroll
                    for (int p = 0; p < 4; p++)
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const uint64_t m = X[p] & Y[q];
                            acc[lane_slot(t)][p * 4 + q] |= (uint32_t)m | (uint32_t)(m >> 32);
                        }
                }
            });
            wave_sync();
        }
        uint8_t* out = inc + mat_off[w];
        lanes_for(0, 64, [&](int t) {
            const int32_t x = ti * kRecTile + (t >> 3), y = tj * kRecTile + (t & 7);
            if (x > y || y >= k) return;
            uint32_t mask = 0;
#pragma unroll
            for (int e = 0; e < 16; e++) mask |= acc[lane_slot(t)][e] ? 1u << e : 0u;
            const uint8_t s = x == y ? (uint8_t)0 : (uint8_t)rec_score(mask);
            out[(int64_t)x * k + y] = s; out[(int64_t)y * k + x] = s;
        });
    }
};

// ---------------------------------------------------------------------------------------------------------------- permutation test
// One wavefront per (window of the batch, chunk of kRecChunk permutations).  The window's matrix lies in LDS (KM x KM bytes at the
// most: KM = 128 or 256, chosen by the batch's largest window).  A permutation at a time: lane t makes the keys of its sites t,
// t + 64, ... (KM / 64 of them, kept in registers) and notes them in LDS; the rank of a site is the number of keys below its own,
// counted against every key in turn -- ONE broadcast read of a key serves all the lane's sites, a compare and an add with carry
// each.  `mix` is a bijection of the 64-bit words (an add, two multiplications by odd numbers, three xor-shifts), so the keys
// mix(pkey + i) of one permutation are pairwise different: the order by (key, index) of 1d is the order by key, and the ranks are a
// permutation of 0 ... k - 1.  order[rank] = site; T: the lanes over the positions i, a loop over the distances d = 1 ... h (uniform;
// a position past k - d adds nothing), two byte reads a look-up; one reduction.  Every wavefront computes phi for itself (k h
// look-ups); the first chunk's notes it.  le is one add per wavefront on a counter the call has cleared; the adds commute.
// (The first form -- a loop over the keys per site, with the index compare of the tie rule -- took 9.85 ms where this one takes
// less on the windows of `bact200`: profiles/rec.)
template <int KM> struct RecPermute {
    const uint8_t* inc; const int64_t* win_off; const int64_t* mat_off;      // of the batch's windows
    const int64_t* win_id; int64_t g0;                                         // the window's number g: win_id[w], or g0 + w
    int32_t near, perms, chunks; uint64_t seed;
    int32_t* phi; uint32_t* le;
    static constexpr int kSlots = KM / 64;
    PM_HD uint32_t stat(const uint8_t* mat, const uint8_t* order, int32_t k, int32_t h) const {
        uint32_t sum = 0;
        lanes_for(0, k, [&](int i) {
            const uint8_t* row = mat + (int32_t)order[i] * k;
            for (int32_t d = 1; d <= h; d++) sum += i + d < k ? row[order[i + d]] : 0u;
        });
        return (uint32_t)wave_sum_u64(sum);
    }
    PM_HD void wave(int64_t item) const {
        const int64_t w = item / chunks; const int32_t chunk = (int32_t)(item % chunks);
        const int32_t k = (int32_t)(win_off[w + 1] - win_off[w]);
        const int32_t h = near < k - 1 ? near : k - 1;
        PM_WAVE_SHARED uint8_t mat[KM * KM];
        PM_WAVE_SHARED uint64_t skey[KM];
        PM_WAVE_SHARED uint8_t order[KM];
        const uint8_t* src = inc + mat_off[w];
        lanes_for(0, k * k, [&](int e) { mat[e] = src[e]; });
        lanes_for(0, k, [&](int i) { order[i] = (uint8_t)i; });
        wave_sync();
        const uint32_t phi0 = stat(mat, order, k, h);
        if (chunk == 0 && wave_leader()) phi[w] = (int32_t)phi0;
        const uint64_t wkey = boot_mix(seed + (uint64_t)(win_id ? win_id[w] : g0 + w));
        const int32_t p1 = (chunk + 1) * kRecChunk < perms ? (chunk + 1) * kRecChunk : perms;
        uint32_t count = 0;
        for (int32_t p = chunk * kRecChunk; p < p1; p++) {
            const uint64_t pkey = boot_mix(wkey + (uint64_t)p);
            wave_sync();      // (the last permutation's keys and order have been read)
            lanes_for(0, k, [&](int i) { skey[i] = boot_mix(pkey + (uint64_t)i); });
            wave_sync();
            lanes_for(0, 64, [&](int t) {
                uint64_t mine[kSlots]; uint32_t rank[kSlots];
#pragma unroll
                for (int q = 0; q < kSlots; q++) { mine[q] = boot_mix(pkey + (uint64_t)(q * 64 + t)); rank[q] = 0; }
#pragma unroll 4
                for (int32_t j = 0; j < k; j++) {
                    const uint64_t kj = skey[j];
#pragma unroll
                    for (int q = 0; q < kSlots; q++) rank[q] += kj < mine[q] ? 1u : 0u;
                }
#pragma unroll
                for (int q = 0; q < kSlots; q++) if (q * 64 + t < k) order[rank[q]] = (uint8_t)(q * 64 + t);
            });
            wave_sync();
            count += stat(mat, order, k, h) <= phi0 ? 1u : 0u;
        }
        if (wave_leader() && count) count_add32(le + w, count);
    }
};

}  // namespace pm
