// snp_kernels.h -- core-genome SNP columns and pairwise SNP distances (pm_snp_* of include/parsnp_mum.h).
//
// The caller hands over alignment columns in chunks of n rows (ASCII, any case).  A column is a CORE SNP when every row holds one
// of A C G T and at least two different letters occur, CORE INVARIANT when every row holds the same one of the four, and OTHER
// when some row holds anything else.  The collection keeps, on the device:
//
//   counts        core invariant, core SNP, other (uint64 each); one atomic add per wavefront and class
//   col           the index of core SNP v among all columns added (int64), in the order added
//   planes        the rows' letters in the core SNP columns, two bits per letter ((byte >> 1) & 3: A 0, C 1, T 2, G 3 -- a core column
//                 holds nothing else) in two bit planes lo / hi of 64-bit words, WORD-MAJOR: word w of row r at plane[w * n + r].
//                 Appending columns appends words (no row is ever moved), the rows of a word lie side by side for the loads of
//                 SnpDist, and the bits of the last word past V are zero.
//
// SnpClassify (a lane per column) -> exclusive scan of its flags -> SnpRank (a lane per column: col[]) -> SnpPack (a wavefront per
// plane word) per add; SnpDist (a wavefront per 32 x 32 tile of row pairs) once.  The bodies are written once for the device and the
// emulation (store_kernels.h, "lanes"); every loop has a constant trip count or one that is uniform over the wavefront, no lane
// polls memory, and wave_sync and the LDS traffic stand where all 64 lanes arrive.
#pragma once
#include "store_kernels.h"

namespace pm {

constexpr int kSnpMaxRows = 2048;      // the gap aligner's sequence limit (2 000 genomes and the reference); dist stays at 16 MB

// the 64-bit word whose bit t is f(t), f evaluated by lane t; on the host one thread plays every lane
template <class F> PM_HD uint64_t wave_ballot_of(F f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__ballot(f((int)__lane_id()));
#else
    uint64_t m = 0;
    for (int t = 0; t < 64; t++) if (f(t)) m |= 1ull << t;
    return m;
#endif
}
// counter += the number of ACTIVE lanes with `want`: one atomic per wavefront (wave_reserve01 without the slots)
PM_HD void wave_count01(uint64_t* counter, bool want) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long mask = __ballot(want);
    if (mask == 0) return;
    if ((int)__lane_id() == __ffsll((long long)mask) - 1) atomicAdd((unsigned long long*)counter, (unsigned long long)__popcll(mask));
#else
    *counter += want ? 1 : 0;
#endif
}
// a value every lane keeps for itself across several lanes_for bodies: a register on the device, a slot per lane on the host
#if defined(__HIP_DEVICE_COMPILE__)
constexpr int kLaneSlots = 1;
__device__ inline int lane_slot(int) { return 0; }
#else
constexpr int kLaneSlots = 64;
inline int lane_slot(int t) { return t; }
#endif

// what a byte is: A 1, C 2, G 4, T 8 (either case), anything else 16
PM_HD uint32_t snp_letter_set(uint8_t b) {
    const uint8_t u = b & 0xdf;
    return u == 'A' ? 1u : u == 'C' ? 2u : u == 'G' ? 4u : u == 'T' ? 8u : 16u;
}
PM_HD uint32_t snp_code(uint8_t b) { return (b >> 1) & 3u; }      // of A C G T in either case: 0 1 3 2
PM_HD uint8_t snp_letter(uint32_t code) { return (uint8_t)("ACTG"[code & 3]); }

// one lane per column of the chunk: neighbouring lanes read neighbouring bytes of one row
struct SnpClassify {
    const uint8_t* chars; int64_t pitch; int64_t ncols; int32_t nrows;
    int64_t* flag;          // [ncols + 1]: 1 where the column is a core SNP; the last entry 0 (the scan's total lands there)
    uint64_t* counts;       // core invariant, core SNP, other
    PM_HD void operator()(int64_t c) const {
        uint32_t seen = 0;
        for (int32_t r = 0; r < nrows; r++) seen |= snp_letter_set(chars[(int64_t)r * pitch + c]);
        const bool other = (seen & 16u) != 0, snp = !other && (seen & (seen - 1)) != 0;
        flag[c] = snp ? 1 : 0;
        if (c == ncols - 1) flag[ncols] = 0;
        wave_count01(counts + 0, !other && !snp);
        wave_count01(counts + 1, snp);
        wave_count01(counts + 2, other);
    }
};
// one lane per column: a core SNP column notes its index among all columns at its rank (rank within the chunk + V so far)
struct SnpRank {
    const int64_t* flag; const int64_t* rank; int64_t v0; int64_t col0; int64_t* col;
    PM_HD void operator()(int64_t c) const {
        if (flag[c]) col[v0 + rank[c]] = col0 + c;
    }
};
// one wavefront per plane word (64 consecutive ranks), one lane per column.  For each row the lanes fetch that row's byte of their
// columns; a ballot per plane is the complete word of that row, which the leader stores.  Only the first word of an add can hold
// bits of the add before it (v0 is no multiple of 64): wavefront 0 alone owns it and ORs into it with a plain load and store.
struct SnpPack {
    const uint8_t* chars; int64_t pitch; int32_t nrows;
    const int64_t* col; int64_t col0;      // col[v] - col0: the column of rank v in this chunk
    int64_t v0, v1;                        // ranks [v0, v1) are this add's
    uint64_t* lo; uint64_t* hi;
    PM_HD void wave(int64_t w) const {
        const int64_t word = v0 / 64 + w;
        const bool shared = w == 0 && (v0 & 63) != 0;
        int64_t mine[kLaneSlots];      // the lane's column in the chunk, -1: none
        lanes_for(0, 64, [&](int t) { const int64_t v = word * 64 + t; mine[lane_slot(t)] = v >= v0 && v < v1 ? col[v] - col0 : -1; });
        for (int32_t r = 0; r < nrows; r++) {
            const uint8_t* row = chars + (int64_t)r * pitch;
            uint64_t code[kLaneSlots];
            lanes_for(0, 64, [&](int t) { const int64_t c = mine[lane_slot(t)]; code[lane_slot(t)] = c >= 0 ? 4u | snp_code(row[c]) : 0u; });
            uint64_t l = wave_ballot_of([&](int t) { return (code[lane_slot(t)] & 1) != 0; });
            uint64_t h = wave_ballot_of([&](int t) { return (code[lane_slot(t)] & 2) != 0; });
            if (wave_leader()) {
                const int64_t at = word * (int64_t)nrows + r;
                if (shared) { l |= lo[at]; h |= hi[at]; }
                lo[at] = l; hi[at] = h;
            }
        }
    }
};
// dist[i][j] = popcount over the words of (lo_i ^ lo_j) | (hi_i ^ hi_j).  A wavefront takes a tile of 32 x 32 row pairs and stages
// the words of its two row groups through LDS in slabs of kSnpSlab words, [side][plane][word][row]: lane (a, b) of the 8 x 8 lanes
// owns the 4 x 4 pairs of rows 4a.. and 4b.., so its four rows of one word are 32 consecutive bytes (two 16-byte LDS reads, the
// eight a's or b's of a wavefront on different banks, equal addresses broadcast) and every word read from memory serves 32 pairs.
// Integer VALU work: two XORs, an OR and a population count per pair and word; 16 accumulators of 32 bits per lane (V < 2^31).
// Only tiles with tj >= ti compute; both halves are written.
constexpr int kSnpTile = 32, kSnpSlab = 8;
struct SnpDist {
    const uint64_t* lo; const uint64_t* hi; int32_t nrows; int64_t words; uint64_t last_mask; int32_t tiles; int32_t* dist;
    PM_HD void wave(int64_t w) const {
        const int32_t ti = (int32_t)(w / tiles), tj = (int32_t)(w % tiles);
        if (tj < ti) return;
        const int32_t base[2] = {ti * kSnpTile, tj * kSnpTile};
        PM_WAVE_SHARED uint64_t sh[2][2][kSnpSlab][kSnpTile];
        uint32_t acc[kLaneSlots][16];
        lanes_for(0, 64, [&](int t) {
#pragma unroll
            for (int k = 0; k < 16; k++) acc[lane_slot(t)][k] = 0;
        });
        constexpr int kPer = 2 * 2 * kSnpSlab * kSnpTile / 64;      // slab entries per lane: all its loads leave before the first LDS store waits for one
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
                for (int k = 0; k < kPer; k++) {      // (the mask of the last word here: nothing above needs a loaded value)
                    const int e = k * 64 + t;
                    const bool last = s0 + e / kSnpTile % kSnpSlab == words - 1;
                    (&sh[0][0][0][0])[e] = last ? got[lane_slot(t)][k] & last_mask : got[lane_slot(t)][k];
                }
            });
            wave_sync();
            lanes_for(0, 64, [&](int t) {
                const int a = (t >> 3) * 4, b = (t & 7) * 4;
#pragma unroll
                for (int wd = 0; wd < kSnpSlab; wd++) {
                    uint64_t al[4], ah[4], bl[4], bh[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) { al[k] = sh[0][0][wd][a + k]; ah[k] = sh[0][1][wd][a + k]; bl[k] = sh[1][0][wd][b + k]; bh[k] = sh[1][1][wd][b + k]; }
#pragma unroll
                    for (int x = 0; x < 4; x++)
#pragma unroll
                        for (int y = 0; y < 4; y++) acc[lane_slot(t)][x * 4 + y] += (uint32_t)__builtin_popcountll((al[x] ^ bl[y]) | (ah[x] ^ bh[y]));
                }
            });
            wave_sync();
        }
        lanes_for(0, 64, [&](int t) {
            const int a = (t >> 3) * 4, b = (t & 7) * 4;
#pragma unroll
            for (int x = 0; x < 4; x++)
#pragma unroll
                for (int y = 0; y < 4; y++) {
                    const int64_t i = base[0] + a + x, j = base[1] + b + y;
                    if (i < nrows && j < nrows) {
                        const int32_t d = (int32_t)acc[lane_slot(t)][x * 4 + y];
                        dist[i * nrows + j] = d; dist[j * nrows + i] = d;
                    }
                }
        });
    }
};

}  // namespace pm
