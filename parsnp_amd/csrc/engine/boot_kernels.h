// boot_kernels.h -- Felsenstein's bootstrap of the SNP tree (pm_boot_distances, pm_nj_trees, pm_nj_support of include/parsnp_mum.h;
// the definition is INTEGRATION.md §1c).  A replicate resamples the V core SNP columns with replacement; on the device it is the
// collection's bit planes (snp_kernels.h) under an integer weight per column, capped at 15: four WEIGHT PLANES of 64-bit words.
//
//   cnt           per replicate of a batch and column the number of draws that picked it (uint32; atomic adds, which commute: the
//                 same bytes in every run)
//   w8, planes    the capped weights as bytes [replicate][V] and as planes [replicate][4][words]; bits past V are zero
//   dist          int32 [replicate][n][n], kept for pm_nj_trees
//   D, R, ...     the state of nj_kernels.h once per tree of a batch; joins [tree][n - 3], last [tree], kept for pm_nj_support
//   sets, keys    per tree its n - 3 splits: ceil(n / 64) words each (the side without leaf 0) and a 64-bit key, the sum of a
//                 constant per leaf
//
// BootDraw (a lane per draw) -> BootPack (a wavefront per replicate and plane word) -> SnpDistBoot (a wavefront per 32 x 32 tile of
// row pairs and group of kBootGroup replicates); NjInitB / NjRowMinB (a wavefront per (tree, slot)), NjJoinB (a workgroup of 256
// threads per tree) and NjLastB (a wavefront per tree) run the bodies of nj_kernels.h on the trees of a batch in lock step: the
// same 2 (n - 3) + 2 launches, whatever the number of trees; BootSplits and BootMatch (a wavefront per tree) count the support.
// The bodies are written once for the device and the emulation (store_kernels.h, "lanes"); every loop has a constant trip count
// or one that is uniform over the wavefront's active lanes, no lane polls memory, no kernel waits for another workgroup, and the
// barriers and the LDS traffic stand where all lanes arrive.
#pragma once
#include "nj_kernels.h"

namespace pm {

constexpr int kBootMaxReps = 1024;
constexpr int kBootMaxWeight = 15, kBootPlanes = 4;
constexpr int kBootGroup = 4;            // replicates a wavefront of SnpDistBoot serves with one difference word
constexpr int kBootTable = 4096;         // entries of BootMatch's hash table: a power of two >= 2 (kNjMaxRows - 3)

// splitmix64's output function: the draws of §1c (arithmetic modulo 2^64)
PM_HD uint64_t boot_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
PM_HD uint64_t boot_leaf_key(int32_t leaf) { return boot_mix(0xB0075EEDull + (uint64_t)leaf); }      // any constants do: a key picks candidates, the words decide

// *p += v on a counter in memory (commutative: the order of the adds does not show), the plain update in the emulation
PM_HD void count_add32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
// compare-and-swap on an LDS word (returns what was there)
PM_HD int32_t lds_cas32(int32_t* p, int32_t expect, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const int32_t o = *p; if (o == expect) *p = v; return o;
#endif
}
// whether any ACTIVE lane holds `x`: the condition of a loop that the active lanes of a wavefront leave together
PM_HD bool wave_any(bool x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(x) != 0;
#else
    return x;
#endif
}

// ---------------------------------------------------------------------------------------------------------------- weights
// one lane per (replicate of the batch, draw)
struct BootDraw {
    uint64_t seed; int64_t b0; int64_t V; uint32_t* cnt;      // cnt[bl * V + v]; b0: the batch's first replicate
    PM_HD void operator()(int64_t x) const {
        const int64_t bl = x / V, t = x % V;
        const uint64_t key = boot_mix(seed + (uint64_t)(b0 + bl));
        const uint64_t c = ((boot_mix(key + (uint64_t)t) >> 32) * (uint64_t)V) >> 32;      // < V
        count_add32(cnt + bl * V + (int64_t)c, 1u);
    }
};
// one wavefront per (replicate of the batch, plane word), one lane per column: the weight is the capped counter (noted as a byte
// for the caller) or the caller's byte; a ballot per plane is the complete word, as in SnpPack
struct BootPack {
    const uint32_t* cnt; const uint8_t* given; int64_t V; int64_t words; uint8_t* w8; uint64_t* planes;      // planes[(bl * 4 + p) * words + word]
    PM_HD void wave(int64_t w) const {
        const int64_t bl = w / words, word = w % words;
        uint32_t c[kLaneSlots];
        lanes_for(0, 64, [&](int t) {
            const int64_t v = word * 64 + t;
            uint32_t x = 0;
            if (v < V) {
                if (given) x = given[bl * V + v];
                else { x = cnt[bl * V + v]; x = x > (uint32_t)kBootMaxWeight ? (uint32_t)kBootMaxWeight : x; w8[bl * V + v] = (uint8_t)x; }
            }
            c[lane_slot(t)] = x;
        });
#pragma unroll
        for (int p = 0; p < kBootPlanes; p++) {
            const uint64_t m = wave_ballot_of([&](int t) { return ((c[lane_slot(t)] >> p) & 1u) != 0; });
            if (wave_leader()) planes[(bl * kBootPlanes + p) * words + word] = m;
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------- distances
// dist_b[i][j] = sum over the planes p of popcount(diff & plane_p of b) << p, diff = (lo_i ^ lo_j) | (hi_i ^ hi_j).  The tile, the
// staging through LDS and the 4 x 4 pairs of a lane are SnpDist's; the difference word of a pair and word is formed once and serves
// the kBootGroup replicates of the wavefront's group.  A weight word is the same for the whole wavefront (its address depends on
// the workgroup and the loop counters only): scalar loads into scalar registers.  Replicates past the batch's last in the last
// group read the last one's planes and write nothing.  No mask of the last word: the weight planes are zero past V.
struct SnpDistBoot {
    const uint64_t* lo; const uint64_t* hi; int32_t nrows; int64_t words; int32_t tiles;
    const uint64_t* planes; int32_t reps; int32_t* dist;      // of the batch: planes[(b * 4 + p) * words + w], dist[(b * n + i) * n + j]
    PM_HD void wave(int64_t w) const {
        const int64_t tt = (int64_t)tiles * tiles;
        const int32_t grp = (int32_t)(w / tt), tile = (int32_t)(w % tt);
        const int32_t ti = tile / tiles, tj = tile % tiles;
        if (tj < ti) return;
        const int32_t base[2] = {ti * kSnpTile, tj * kSnpTile};
        const uint64_t* wp[kBootGroup];
#pragma unroll
        for (int k = 0; k < kBootGroup; k++) { const int32_t b = grp * kBootGroup + k; wp[k] = planes + (int64_t)(b < reps ? b : reps - 1) * kBootPlanes * words; }
        PM_WAVE_SHARED uint64_t sh[2][2][kSnpSlab][kSnpTile];
        uint32_t acc[kLaneSlots][kBootGroup][16];
        lanes_for(0, 64, [&](int t) {
#pragma unroll
            for (int k = 0; k < kBootGroup; k++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[lane_slot(t)][k][e] = 0;
        });
        constexpr int kPer = 2 * 2 * kSnpSlab * kSnpTile / 64;
        uint64_t got[kLaneSlots][kPer];
        for (int64_t s0 = 0; s0 < words; s0 += kSnpSlab) {
            lanes_for(0, 64, [&](int t) {
#pragma unroll
                for (int k = 0; k < kPer; k++) {
                    const int e = k * 64 + t;
                    const int row = e % kSnpTile, wd = e / kSnpTile % kSnpSlab, plane = e / (kSnpTile * kSnpSlab) % 2, side = e / (kSnpTile * kSnpSlab * 2);
                    const int64_t r = base[side] + row, gw = s0 + wd;
                    uint64_t v = 0;
                    if (r < nrows && gw < words) v = (plane ? hi : lo)[gw * nrows + r];
                    got[lane_slot(t)][k] = v;
                }
            });
            lanes_for(0, 64, [&](int t) {
#pragma unroll
                for (int k = 0; k < kPer; k++) (&sh[0][0][0][0])[k * 64 + t] = got[lane_slot(t)][k];
            });
            wave_sync();
            lanes_for(0, 64, [&](int t) {
                const int a = (t >> 3) * 4, b = (t & 7) * 4;
                // (not unrolled: the 32 weight words of ONE plane word fill the scalar registers; unrolled over the slab they and the
                // 64 accumulators spilled)
#pragma unroll 1
                for (int wd = 0; wd < kSnpSlab; wd++) {
                    const int64_t gw = s0 + wd < words ? s0 + wd : words - 1;      // (past the last word the staged words are zero)
                    uint64_t al[4], ah[4], bl[4], bh[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) { al[k] = sh[0][0][wd][a + k]; ah[k] = sh[0][1][wd][a + k]; bl[k] = sh[1][0][wd][b + k]; bh[k] = sh[1][1][wd][b + k]; }
                    uint64_t wt[kBootGroup][kBootPlanes];
#pragma unroll
                    for (int k = 0; k < kBootGroup; k++)
#pragma unroll
                        for (int p = 0; p < kBootPlanes; p++) wt[k][p] = wp[k][p * words + gw];
#pragma unroll
                    for (int x = 0; x < 4; x++)
#pragma unroll
                        for (int y = 0; y < 4; y++) {
                            const uint64_t diff = (al[x] ^ bl[y]) | (ah[x] ^ bh[y]);
#pragma unroll
                            for (int k = 0; k < kBootGroup; k++) {
                                uint32_t s = acc[lane_slot(t)][k][x * 4 + y];
#pragma unroll
                                for (int p = 0; p < kBootPlanes; p++) s += (uint32_t)__builtin_popcountll(diff & wt[k][p]) << p;
                                acc[lane_slot(t)][k][x * 4 + y] = s;
                            }
                        }
                }
            });
            wave_sync();
        }
        lanes_for(0, 64, [&](int t) {
            const int a = (t >> 3) * 4, b = (t & 7) * 4;
#pragma unroll
            for (int k = 0; k < kBootGroup; k++) {
                const int32_t rep = grp * kBootGroup + k;
                if (rep >= reps) continue;
                int32_t* out = dist + (int64_t)rep * nrows * nrows;
#pragma unroll
                for (int x = 0; x < 4; x++)
#pragma unroll
                    for (int y = 0; y < 4; y++) {
                        const int64_t i = base[0] + a + x, j = base[1] + b + y;
                        if (i < nrows && j < nrows) {
                            const int32_t d = (int32_t)acc[lane_slot(t)][k][x * 4 + y];
                            out[i * nrows + j] = d; out[j * nrows + i] = d;
                        }
                    }
            }
        });
    }
};

// ---------------------------------------------------------------------------------------------------------------- trees of a batch
// The trees of a batch have one n and make their joins in lock step, so they share the launches of one tree.  Each functor hands
// its work item to the body of nj_kernels.h over the state of ITS tree: the arithmetic and the tie rule are those bodies', bit for
// bit.  NjJoinB is launched with 256 items per tree: on the device they are the 256 threads of the tree's workgroup, in the
// emulation the first call of every 256 plays the group (NjJoin returns at once for the others).
struct NjInitB {
    const int32_t* dist; int32_t n; double* D; double* R; uint8_t* active;
    PM_HD void wave(int64_t w) const {
        const int64_t b = w / n, nn = (int64_t)n * n;
        NjInit{dist + b * nn, n, D + b * nn, R + b * n, active + b * n}.wave(w % n);
    }
};
struct NjRowMinB {
    const double* D; const double* R; const uint8_t* active; int32_t n; int32_t r; double* row_q; int32_t* row_j;
    PM_HD void wave(int64_t w) const {
        const int64_t b = w / n;
        NjRowMin{D + b * n * n, R + b * n, active + b * n, n, r, row_q + b * n, row_j + b * n}.wave(w % n);
    }
};
struct NjJoinB {
    double* D; double* R; uint8_t* active; int32_t n; int32_t r; const double* row_q; const int32_t* row_j; NjJoinRec* rec; int32_t t;      // rec[b * (n - 3) + t]
    PM_HD void operator()(int64_t tid) const {
        const int64_t b = tid / kNjGroup;
        NjJoin{D + b * n * n, R + b * n, active + b * n, n, r, row_q + b * n, row_j + b * n, rec + b * (n - 3) + t}(tid % kNjGroup);
    }
};
struct NjLastB {
    const double* D; const uint8_t* active; int32_t n; NjLastRec* rec;
    PM_HD void wave(int64_t b) const { NjLast{D + b * n * n, active + b * n, n, rec + b}.wave(0); }
};

// ---------------------------------------------------------------------------------------------------------------- splits, support
// One wavefront per tree: the leaf set of the node of every join, lanes over its W = ceil(n / 64) words.  tab[slot] says what the
// slot holds (-1: its own leaf, else the join whose node it is) and kraw[slot] the key of that leaf set, both in LDS.  A split is
// stored as the side WITHOUT leaf 0.  Leaf 0 begins in slot 0 and slot 0 never retires (a join retires j > i), so the node of a
// join holds leaf 0 exactly when i == 0: its set is stored complemented, and read back complemented when slot 0 is joined again.
// A lane reads only words it wrote itself (word w of an earlier join).  Slots out of range (records that are not a tree's) are
// brought into range: nothing is indexed by what a record says without that.
struct BootSplits {
    const NjJoinRec* joins; int32_t n; int32_t W; uint64_t* sets; uint64_t* keys;      // tree b: joins + b (n - 3), sets + b (n - 3) W, keys + b (n - 3)
    PM_HD void wave(int64_t b) const {
        const int64_t m = n - 3;
        const NjJoinRec* J = joins + b * m;
        uint64_t* S = sets + b * m * W;
        uint64_t* K = keys + b * m;
        PM_WAVE_SHARED int32_t tab[kNjMaxRows];
        PM_WAVE_SHARED uint64_t kraw[kNjMaxRows];
        uint64_t total = 0;
        lanes_for(0, n, [&](int k) { tab[k] = -1; const uint64_t c = boot_leaf_key(k); kraw[k] = c; total += c; });
        total = wave_sum_u64(total);
        wave_sync();
        const uint64_t last_mask = (n & 63) ? ((1ull << (n & 63)) - 1) : ~0ull;
        for (int64_t t = 0; t < m; t++) {
            int32_t i = J[t].i, j = J[t].j;
            i = i < 0 ? 0 : i >= n ? n - 1 : i; j = j < 0 ? 0 : j >= n ? n - 1 : j;
            const int32_t ui = tab[i], uj = tab[j];
            lanes_for(0, W, [&](int w) {
                const uint64_t full = w == W - 1 ? last_mask : ~0ull;
                uint64_t a = ui < 0 ? ((i >> 6) == w ? 1ull << (i & 63) : 0ull) : S[(int64_t)ui * W + w];
                if (ui >= 0 && i == 0) a = ~a & full;
                uint64_t c = uj < 0 ? ((j >> 6) == w ? 1ull << (j & 63) : 0ull) : S[(int64_t)uj * W + w];
                if (uj >= 0 && j == 0) c = ~c & full;
                const uint64_t u = a | c;
                S[t * W + w] = (i == 0 || j == 0) ? ~u & full : u;
            });
            wave_sync();      // (every lane has read tab[i] and tab[j])
            if (wave_leader()) {
                const uint64_t k = kraw[i] + kraw[j];
                kraw[i] = k; tab[i] = (int32_t)t;
                K[t] = (i == 0 || j == 0) ? total - k : k;
            }
            wave_sync();
        }
    }
};
// One wavefront per replicate tree.  The keys of the main tree's n - 3 splits go into a hash table in LDS (open addressing, at most
// half full, so every walk ends at an empty entry); every split of the replicate walks from its key's entry, compares the WORDS
// where the keys agree, and adds one to the support of the main split it equals.  The splits of a tree are pairwise different:
// a replicate adds at most one to a main split.  The adds commute.
struct BootMatch {
    const uint64_t* msets; const uint64_t* mkeys; const uint64_t* rsets; const uint64_t* rkeys; int32_t n; int32_t W; uint32_t* support;
    PM_HD void wave(int64_t b) const {
        const int32_t m = n - 3;
        int32_t size = 64;
        while (size < 2 * m && size < kBootTable) size <<= 1;      // (uniform; 2 m <= kBootTable)
        const uint32_t mask = (uint32_t)size - 1;
        PM_WAVE_SHARED int32_t tidx[kBootTable];
        PM_WAVE_SHARED uint64_t tkey[kBootTable];
        lanes_for(0, size, [&](int h) { tidx[h] = -1; });
        wave_sync();
        lanes_for(0, m, [&](int t) {
            const uint64_t key = mkeys[t];
            uint32_t h = (uint32_t)(key >> 17) & mask;
            bool live = true;
            while (wave_any(live)) {
                if (live) {
                    if (lds_cas32(&tidx[h], -1, t) == -1) { tkey[h] = key; live = false; }
                    else h = (h + 1) & mask;
                }
            }
        });
        wave_sync();
        lanes_for(0, m, [&](int t) {
            const uint64_t key = rkeys[b * m + t];
            const uint64_t* mine = rsets + (b * m + t) * W;
            uint32_t h = (uint32_t)(key >> 17) & mask;
            bool live = true;
            while (wave_any(live)) {
                if (live) {
                    const int32_t at = tidx[h];
                    if (at < 0) live = false;
                    else {
                        if (tkey[h] == key) {
                            bool same = true;
                            for (int32_t w = 0; w < W; w++) same &= msets[(int64_t)at * W + w] == mine[w];
                            if (same) { count_add32(support + at, 1u); live = false; }
                        }
                        h = (h + 1) & mask;
                    }
                }
            }
        });
    }
};

}  // namespace pm
