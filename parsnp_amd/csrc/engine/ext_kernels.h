// ext_kernels.h -- extension of the LCB ends into their flanks: a banded dynamic programme per (job, row) against the reference's
// flank, a cut common to the rows of a job, the paths and their star merge into columns (pm_ext_reach, pm_ext_align of
// include/parsnp_mum.h; the definition is INTEGRATION.md §1e).  All of it is integer work; the letters come from the session's
// resident genomes through descriptors.
//
//   row           {genome, step, complement, len, first}: letter q of the row is base first + q step of the genome's forward strand,
//                 complemented where `complement` is set; a base that is none of ACGT has code 4, matches nothing and prints N
//   pair          a (job, row); pair p is row p of the call's row list, its job row_job[p], the job's reference row rows[row_off[job]]
//   bits          per pair 9 words: bit i set where the row passes at line i (1 ... La)
//   pk            per pair and slot k = 0 ... A one 16-bit word: ins_r(k) << 1 | (the row holds a base under reference base k)
//   cs            per job and slot k the column at which the slot begins
//
// ExtReach (a wavefront per pair, scores only) -> ExtCut (a wavefront per job) ; ExtTrace (a wavefront per pair: the table once more
// up to line A, two bits a cell in LDS, the path walked back by the first lane) -> ExtWidth (a wavefront per job: slot widths and
// their prefix sum) -> ExtMerge (a wavefront per pair: the row's letters).
//
// The table is walked by ANTI-DIAGONALS.  With d = j - i + W (0 ... 2 W, at most 127 values) and s = i + j, the cells of one
// anti-diagonal s have d of one parity, (s + W) & 1, so at most 64 of them exist: one per lane.  Lane t keeps the cells d = 2 t and
// d = 2 t + 1 in two registers ("two a lane").  A cell's diagonal predecessor is the lane's own register of the same parity (two
// steps old), its other two predecessors are one step old: the lane's other register and that of ONE neighbouring lane -- a single
// cross-lane move per step and no scan inside a line.  (A line at a time would need the prefix maximum of T(d) + G d over the band,
// seven cross-lane steps for two cells a lane, on 512 lines; the anti-diagonals need La + Lb <= 1 024 steps of one move each.)
// A line's maximum gathers over the 2 W + 1 steps that touch it, by an LDS max per live cell; within a step the live cells lie on
// different lines.  The bodies are written once for the device and the emulation (store_kernels.h, "lanes"): every loop has a trip
// count that is uniform over the wavefront, the cross-lane moves and wave_sync stand where all 64 lanes arrive, no wavefront waits
// for another and none writes where another reads.
#pragma once
#include "rec_kernels.h"

namespace pm {

constexpr int kExtMaxRows = 2048;        // rows of a job
constexpr int kExtMaxFlank = 512;
constexpr int kExtMaxBand = 63;
constexpr int kExtBitWords = kExtMaxFlank / 64 + 1;      // pass bits of lines 0 ... 512
PM_HD constexpr int ext_mv_pitch(int flank) { return flank / 16 + 1; }      // 32-bit words of two-bit moves per band position (lines 0 ... flank)
constexpr int32_t kExtNeg = -(1 << 28);                  // a cell that does not exist

struct ExtRow { int32_t genome, step, complement, len; int64_t first; };      // pm_ext_row
struct ExtParams { int32_t match, mismatch, gap, band, ani, min_len, max_flank; };      // pm_ext_params

PM_HD void lds_max32(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
// the value lane t + 1 (t - 1) keeps in v, `edge` in the last (first) lane; every lane of the wavefront arrives
PM_HD int32_t lane_next_i32(const int32_t* v, int t, int32_t edge) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int32_t y = __shfl_down(v[0], 1, 64);
    return t == 63 ? edge : y;
#else
    return t == 63 ? edge : v[t + 1];
#endif
}
PM_HD int32_t lane_prev_i32(const int32_t* v, int t, int32_t edge) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int32_t y = __shfl_up(v[0], 1, 64);
    return t == 0 ? edge : y;
#else
    return t == 0 ? edge : v[t - 1];
#endif
}

// letter q of a row as a code: 0 ... 3 = ACGT, 4 = anything else
PM_HD uint8_t ext_code(const Packed& P, const ExtRow& r, int32_t q) {
    const int64_t p = P.goff[2 * (int64_t)r.genome] + r.first + (int64_t)q * r.step;
    const SeqBlock& blk = P.blk[p >> 5];
    const int k = (int)(p & 31);
    if ((blk.nm >> k) & 1u) return 4;
    const uint32_t c = (uint32_t)(blk.b2 >> (2 * k)) & 3u;
    return (uint8_t)(r.complement ? 3u - c : c);
}
PM_HD uint8_t ext_letter(uint8_t code) { return code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : code == 3 ? 'T' : 'N'; }
// the rows' letters as codes into LDS
PM_HD void ext_stage(const Packed& P, const ExtRow& r, uint8_t* dst) {
    lanes_for(0, r.len, [&](int q) { dst[q] = ext_code(P, r, q); });
}

// The table of a pair, lines 0 ... Lmax (Lmax <= La), by anti-diagonals.  best[i]: the line's maximum (the caller has set best[0] = 0
// and the others to INT32_MIN).  kTrace: mv gets the two-bit move of every cell (1 diagonal, 2 up, 3 left; the caller has cleared
// it), last[d] the cell of line Lmax at band position d (the caller has set it to kExtNeg).
template <bool kTrace> PM_HD void ext_walk(const uint8_t* a, const uint8_t* b, int32_t Lmax, int32_t Lb, const ExtParams& prm, int32_t* best, uint32_t* mv,
                                           int32_t mv_pitch, int32_t* last) {
    const int32_t W = prm.band, M = prm.match, X = prm.mismatch, G = prm.gap;
    int32_t E[kLaneSlots], O[kLaneSlots];      // the cells d = 2 t and d = 2 t + 1 of the lane, each as of its last step
    lanes_for(0, 64, [&](int t) {
        E[lane_slot(t)] = 2 * t == W ? 0 : kExtNeg;      // (cell (0, 0) lies at d = W)
        O[lane_slot(t)] = 2 * t + 1 == W ? 0 : kExtNeg;
    });
    const int32_t jmax = Lb < Lmax + W ? Lb : Lmax + W;
    for (int32_t s = 1; s <= Lmax + jmax; s++) {
        const int par = (s + W) & 1;
        lanes_for(0, 64, [&](int t) {
            const int q = lane_slot(t);
            const int32_t d = 2 * t + par, i2 = s - d + W, j2 = s + d - W;
            const int32_t i = i2 >> 1, j = j2 >> 1;
            const bool live = d <= 2 * W && i2 >= 0 && j2 >= 0 && i <= Lmax && j <= Lb;
            const int32_t own = par ? O[q] : E[q];
            const int32_t up = par ? lane_next_i32(E, t, kExtNeg) : O[q];
            const int32_t left = par ? E[q] : lane_prev_i32(O, t, kExtNeg);
            int32_t h = kExtNeg;
            if (live) {
                int32_t sub = -X;
                if (i > 0 && j > 0) { const uint8_t ca = a[i - 1]; if (ca == b[j - 1] && ca < 4) sub = M; }
                const int32_t dv = own + sub, uv = up - G, lv = left - G;
                h = dv > uv ? dv : uv;
                h = h > lv ? h : lv;
                lds_max32(best + i, h);
                if (kTrace) {
                    const uint32_t move = h == dv ? 1u : h == uv ? 2u : 3u;      // (a predecessor that does not exist is far below h)
                    mv[d * mv_pitch + (i >> 4)] |= move << (2 * (i & 15));      // (the lane's own words)
                    if (i == Lmax) last[d] = h;
                }
            }
            if (par) O[q] = h; else E[q] = h;
        });
    }
}

// row r passes at line i
PM_HD bool ext_passes(const ExtParams& prm, int32_t i, int32_t best) {
    return best != INT32_MIN && 100 * best >= i * (prm.ani * prm.match - (100 - prm.ani) * prm.mismatch);
}

// ---------------------------------------------------------------------------------------------------------------- reach
struct ExtReach {
    Packed P; const ExtRow* rows; const int32_t* row_job; const int64_t* row_off; ExtParams prm; int64_t p0;
    uint64_t* bits;          // [pair][kExtBitWords]
    int32_t* best_out;       // [pair - p0][max_flank + 1] or nullptr
    PM_HD void wave(int64_t item) const {
        const int64_t p = p0 + item;
        const ExtRow ra = rows[row_off[row_job[p]]], rb = rows[p];
        PM_WAVE_SHARED uint8_t a[kExtMaxFlank], b[kExtMaxFlank];
        PM_WAVE_SHARED int32_t best[kExtMaxFlank + 1];
        ext_stage(P, ra, a); ext_stage(P, rb, b);
        lanes_for(0, kExtMaxFlank + 1, [&](int i) { best[i] = i ? INT32_MIN : 0; });
        wave_sync();
        ext_walk<false>(a, b, ra.len, rb.len, prm, best, nullptr, 0, nullptr);
        wave_sync();
        for (int32_t w = 0; w < kExtBitWords; w++) {
            const uint64_t m = wave_ballot_of([&](int t) { const int32_t i = 64 * w + t; return i >= 1 && i <= ra.len && ext_passes(prm, i, best[i]); });
            if (wave_leader()) bits[p * kExtBitWords + w] = m;
        }
        if (best_out) lanes_for(0, prm.max_flank + 1, [&](int i) { best_out[item * (prm.max_flank + 1) + i] = i <= ra.len ? best[i] : INT32_MIN; });
    }
};
// One wavefront per job: the lanes AND the bits of the job's rows, the highest common bit is the reach (0 below min_len).
struct ExtCut {
    const int64_t* row_off; ExtParams prm; const uint64_t* bits; int32_t* reach;
    PM_HD void wave(int64_t job) const {
        const int64_t r0 = row_off[job], r1 = row_off[job + 1];
        int32_t A = 0;
        for (int32_t w = 0; w < kExtBitWords; w++) {
            uint64_t miss = 0;
            lanes_for(0, (int)(r1 - r0), [&](int r) { miss |= ~bits[(r0 + r) * kExtBitWords + w]; });
            const uint64_t all = ~wave_or_u64(miss);
            if (all) A = 64 * w + 63 - __builtin_clzll(all);
        }
        if (wave_leader()) reach[job] = A >= prm.min_len ? A : 0;
    }
};

// ---------------------------------------------------------------------------------------------------------------- paths
// KF: the longest flank the instance takes (256 or 512).  The moves are what fills the LDS: 128 band positions x (KF / 16 + 1) words,
// 8.5 KB at 256 and 16.5 KB at 512, and with them the wavefronts a CU holds.  (The first form had the 512 size alone: 21.5 KB a
// wavefront, two wavefronts a SIMD, 17.2 ms on the designed set of profiles/ext where this one takes 10.1 at the default max_flank of 256.)
template <int KF> struct ExtTrace {
    Packed P; const ExtRow* rows; const int32_t* row_job; const int64_t* row_off; ExtParams prm; int64_t p0;
    const int32_t* reach;
    uint16_t* pk;            // [pair - p0][max_flank + 1]
    int32_t* used;           // [pair]
    PM_HD void wave(int64_t item) const {
        const int64_t p = p0 + item;
        const int32_t job = row_job[p], A = reach[job];
        if (A == 0) { if (wave_leader()) used[p] = 0; return; }      // (uniform)
        const ExtRow ra = rows[row_off[job]], rb = rows[p];
        constexpr int kPitch = ext_mv_pitch(KF);
        PM_WAVE_SHARED uint8_t a[KF], b[KF];
        PM_WAVE_SHARED int32_t best[KF + 1];
        PM_WAVE_SHARED uint32_t mv[2 * (kExtMaxBand + 1) * kPitch];
        PM_WAVE_SHARED int32_t last[2 * (kExtMaxBand + 1)];
        PM_WAVE_SHARED uint16_t slot[KF + 1];
        ext_stage(P, ra, a); ext_stage(P, rb, b);
        lanes_for(0, KF + 1, [&](int i) { best[i] = i ? INT32_MIN : 0; slot[i] = 0; });
        lanes_for(0, 2 * (kExtMaxBand + 1) * kPitch, [&](int e) { mv[e] = 0; });
        lanes_for(0, 2 * (kExtMaxBand + 1), [&](int d) { last[d] = kExtNeg; });
        wave_sync();
        ext_walk<true>(a, b, A, rb.len, prm, best, mv, kPitch, last);
        wave_sync();
        // j_r: the smallest j, that is the smallest d, whose cell of line A holds the line's maximum
        const int32_t top = best[A];
        const uint64_t m0 = wave_ballot_of([&](int t) { return last[t] == top; });
        const uint64_t m1 = wave_ballot_of([&](int t) { return last[64 + t] == top; });
        int32_t d = m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1 | (1ull << 63));
        int32_t i = A, j = A + d - prm.band;
        if (wave_leader()) {
            used[p] = j;
            // (every move takes a base of a or of b: at most A + j_r of them.  The host refuses a reach whose line has no cell in some
            // row; the bound and the band test keep the walk inside mv whatever the words hold)
            for (int32_t left = A + j; left > 0 && (i > 0 || j > 0) && d >= 0 && d <= 2 * prm.band; left--) {
                const uint32_t move = (mv[d * kPitch + (i >> 4)] >> (2 * (i & 15))) & 3u;
                if (move == 1u) { i--; j--; slot[i] |= 1; }
                else if (move == 2u) { i--; d++; }
                else if (move == 3u) { j--; d--; slot[i] += 2; }
                else break;
            }
        }
        wave_sync();
        uint16_t* out = pk + (p - p0) * (prm.max_flank + 1);
        lanes_for(0, A + 1, [&](int k) { out[k] = slot[k]; });
    }
};

// ---------------------------------------------------------------------------------------------------------------- columns
// One wavefront per job of the batch: the lanes take the slots, a loop over the rows gives the slot's width; the first lane sums.
struct ExtWidth {
    const int64_t* row_off; ExtParams prm; int64_t j0, p0;
    const int32_t* reach; const uint16_t* pk;
    int32_t* cs;             // [job - j0][max_flank + 2]: the column at which slot k begins, k = 0 ... A, then C
    int32_t* cols;           // [job]
    PM_HD void wave(int64_t item) const {
        const int64_t job = j0 + item;
        const int32_t A = reach[job];
        if (A == 0) { if (wave_leader()) cols[job] = 0; return; }      // (uniform)
        const int64_t r0 = row_off[job] - p0, r1 = row_off[job + 1] - p0;
        const int32_t pitch = prm.max_flank + 1;
        PM_WAVE_SHARED int32_t w[kExtMaxFlank + 2];
        lanes_for(0, A + 1, [&](int k) {
            int32_t m = 0;
            for (int64_t r = r0; r < r1; r++) { const int32_t v = pk[r * pitch + k] >> 1; m = v > m ? v : m; }
            w[k] = m;
        });
        wave_sync();
        if (wave_leader()) {
            int32_t at = 0;
            for (int32_t k = 0; k <= A; k++) { const int32_t wk = w[k]; w[k] = at; at += wk + (k < A ? 1 : 0); }
            w[A + 1] = at;
            cols[job] = at > 2 * prm.max_flank ? -1 : at;
        }
        wave_sync();
        int32_t* out = cs + item * (prm.max_flank + 2);
        lanes_for(0, A + 2, [&](int k) { out[k] = w[k]; });
    }
};
// One wavefront per pair of the batch: the first lane sums the bases the row has spent before every slot, then the lanes take the
// slots and write the slot's columns and the reference base's column of the row.
struct ExtMerge {
    Packed P; const ExtRow* rows; const int32_t* row_job; ExtParams prm; int64_t j0, p0;
    const int32_t* reach; const int32_t* cols; const uint16_t* pk; const int32_t* cs;
    int64_t pitch;           // bytes of a row of out
    uint8_t* out;            // [pair - p0][pitch]
    PM_HD void wave(int64_t item) const {
        const int64_t p = p0 + item;
        const int32_t job = row_job[p], A = reach[job], C = cols[job];
        if (C <= 0) return;      // (uniform)
        const ExtRow rb = rows[p];
        const uint16_t* mine = pk + item * (prm.max_flank + 1);
        const int32_t* start = cs + (job - j0) * (prm.max_flank + 2);
        PM_WAVE_SHARED int32_t spent[kExtMaxFlank + 1];
        lanes_for(0, A + 1, [&](int k) { spent[k] = (mine[k] >> 1) + (mine[k] & 1); });
        wave_sync();
        if (wave_leader()) {
            int32_t at = 0;
            for (int32_t k = 0; k <= A; k++) { const int32_t v = spent[k]; spent[k] = at; at += v; }
        }
        wave_sync();
        uint8_t* dst = out + item * pitch;
        lanes_for(0, A + 1, [&](int k) {
            const int32_t ins = mine[k] >> 1, c0 = start[k], wk = start[k + 1] - c0 - (k < A ? 1 : 0);
            for (int32_t q = 0; q < wk; q++) dst[c0 + q] = q < ins ? ext_letter(ext_code(P, rb, spent[k] + q)) : (uint8_t)'-';
            if (k < A) dst[c0 + wk] = (mine[k] & 1) ? ext_letter(ext_code(P, rb, spent[k] + ins)) : (uint8_t)'-';
        });
    }
};

}  // namespace pm
