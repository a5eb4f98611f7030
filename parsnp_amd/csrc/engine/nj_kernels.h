// nj_kernels.h -- neighbour joining over an n x n integer distance matrix (pm_nj_tree of include/parsnp_mum.h; the definition is
// INTEGRATION.md §1b).  The tree keeps, on the device:
//
//   D             n x n doubles, full and symmetric: the distances between the slots (a join writes row i AND column i, so that every
//                 read is a read along a row)
//   R             n doubles: the row sums over the active slots (the integer sums at the start, the closed form after a join)
//   active        n bytes: 1 while the slot holds a node
//   rowmin        per slot i its smallest Q(i, j) over the active j > i and that j (-1: none)
//   joins, last   the records the host turns into branch lengths and Newick (pm_nj_join, pm_nj_last)
//
// NjInit (a wavefront per row) once; then per join NjRowMin (a wavefront per slot) and NjJoin (ONE workgroup of 256 threads: the
// arg-min over rowmin, the record, and after a workgroup barrier the update of row / column i and of R); NjLast (one wavefront) writes
// the record of the last three slots.  The number of joins is known, so all launches of a tree are queued without a host wait.
// The bodies are written once for the device and the emulation (store_kernels.h, "lanes"); every loop has a constant trip count or
// one that is uniform over the wavefront, no lane polls memory, no kernel waits for another workgroup, and the barriers and the
// LDS traffic stand where all lanes arrive.
//
// ARITHMETIC.  Every result is bit-exact by definition: IEEE doubles, each operation rounded once, in the order written, never fused.
// Neither this header's device translation unit nor the emulation is built with -ffp-contract=off, so the few operations go through
// nj_mul / nj_add / nj_sub:
//   device   plain `a * b`, `a + b`, `a - b` in bodies that stand under `#pragma clang fp contract(off)`: the pragma takes the
//            `contract` flag off exactly these operations, the backend fuses a multiply and an add only when BOTH carry the flag,
//            and the flag stays with the operation through inlining.  NOT __dmul_rn / __dadd_rn / __dsub_rn: this toolchain's
//            header defines them as the plain operators (their correctly rounded library forms only under a macro that HIP does
//            not set), compiled under the translation unit's own mode (-ffp-contract=fast), so the pragma of a caller does not
//            reach them -- with them the gfx950 ISA of NjRowMin and NjJoin held one v_fma_f64 each.  With the operators under the
//            pragma NjRowMin, NjJoin and NjLast hold none (read once in the ISA).
//   host     the result passes through an empty asm statement that takes and returns it in a register: the compiler has to
//            materialise the rounded product (sum) there and cannot see through it, whatever -ffp-contract or -mfma say.
#pragma once
#include "snp_kernels.h"

namespace pm {

constexpr int kNjMaxRows = 2048;      // kSnpMaxRows: D stays at 32 MB
constexpr int kNjGroup = 256;         // the threads of NjJoin's one workgroup

struct NjJoinRec { int32_t i, j; double dij, ri, rj; };
struct NjLastRec { int32_t a, b, c; double dab, dac, dbc; };

#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline double nj_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ inline double nj_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ inline double nj_sub(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
#else
inline double nj_opaque(double v) {
#if defined(__x86_64__)
    asm volatile("" : "+x"(v));
#else
    asm volatile("" : "+m"(v));
#endif
    return v;
}
inline double nj_mul(double a, double b) { return nj_opaque(a * b); }
inline double nj_add(double a, double b) { return nj_opaque(a + b); }
inline double nj_sub(double a, double b) { return nj_opaque(a - b); }
#endif

// (q, i, j) before (q2, i2, j2): the smaller Q, then the smaller i, then the smaller j; values that compare equal tie (-0 and +0 too)
PM_HD bool nj_before(double q, int32_t i, int32_t j, double q2, int32_t i2, int32_t j2) {
    return (q < q2) | ((q == q2) & ((i < i2) | ((i == i2) & (j < j2))));
}
// the (double, int, int) arg-min over the wavefront under nj_before, beside wave_min_i32: a shuffle butterfly on the device (the
// compare is a total order on distinct (i, j), so every order of the exchanges ends with the same triple in every lane), the
// identity on the host, where the one thread has kept the best of all lanes
#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline void wave_argmin_f64(double& q, int32_t& i, int32_t& j) {
    for (int d = 32; d >= 1; d >>= 1) {
        const double q2 = __shfl_xor(q, d, 64);
        const int32_t i2 = __shfl_xor(i, d, 64), j2 = __shfl_xor(j, d, 64);
        if (nj_before(q2, i2, j2, q, i, j)) { q = q2; i = i2; j = j2; }
    }
}
__device__ inline int nj_thread() { return (int)threadIdx.x; }
__device__ inline void group_sync() { __syncthreads(); }
#define PM_GROUP_SHARED __shared__
// lanes_for for a body that only loads and selects, four passes at a time: f(index, valid) is called for EVERY lane in every
// pass, with an index that is in bounds also where the lane has no element (valid == false: index n - 1), so the body has no branch
// and the loads of four passes leave together instead of each pass waiting out a memory latency.  Uniform trip count.
template <class F> __device__ inline void lanes_for4(int from, int n, F f) {
    for (int base = from & ~63; base < n; base += 256) {
#pragma unroll
        for (int u = 0; u < 4; u++) { const int j = base + 64 * u + (int)__lane_id(); const bool valid = (j >= from) & (j < n); f(valid ? j : n - 1, valid); }
    }
}
// the workgroup's walk in two steps: `load` (branch-free: index in bounds, valid says whether the thread has an element) of four
// passes first, into registers, then `use` of the four -- no store of a pass stands between the loads of the next
template <class T, class L, class U> __device__ inline void group_for4(int n, L load, U use) {
    for (int base = 0; base < n; base += 4 * kNjGroup) {
        T got[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int k = base + kNjGroup * u + (int)threadIdx.x; const bool valid = k < n; got[u] = load(valid ? k : n - 1, valid); }
#pragma unroll
        for (int u = 0; u < 4; u++) { const int k = base + kNjGroup * u + (int)threadIdx.x; if (k < n) use(k, got[u]); }
    }
}
#else
inline void wave_argmin_f64(double&, int32_t&, int32_t&) {}
inline int nj_thread() { return 0; }
inline void group_sync() {}
#define PM_GROUP_SHARED
template <class F> inline void lanes_for4(int from, int n, F f) { for (int j = from; j < n; j++) f(j, true); }
template <class T, class L, class U> inline void group_for4(int n, L load, U use) { for (int k = 0; k < n; k++) { const T got = load(k, true); use(k, got); } }
#endif
constexpr double kNjNone = __builtin_huge_val();      // +infinity: no pair yet
constexpr int32_t kNjNoSlot = 0x7fffffff;

// one wavefront per row: D from the integers, the row sum in 64-bit integers, the flag
struct NjInit {
    const int32_t* dist; int32_t n; double* D; double* R; uint8_t* active;
    PM_HD void wave(int64_t i) const {
        const int32_t* src = dist + i * n;
        double* dst = D + i * n;
        uint64_t sum = 0;
        lanes_for(0, n, [&](int j) { const int32_t v = src[j]; dst[j] = (double)v; sum += (uint64_t)(int64_t)v; });
        sum = wave_sum_u64(sum);
        if (wave_leader()) { R[i] = (double)(int64_t)sum; active[i] = 1; }
    }
};

// one wavefront per slot i: the smallest Q(i, j) over the active j > i.  An inactive row returns before it reads anything else; the
// lanes read D[i][.], R[.] and the flags side by side.
struct NjRowMin {
    const double* D; const double* R; const uint8_t* active; int32_t n; int32_t r;      // r: the active slots of this join
    double* row_q; int32_t* row_j;
    PM_HD void wave(int64_t w) const {
        const int32_t i = (int32_t)w;
        if (!active[i]) return;
        const double* row = D + (int64_t)i * n;
        const double ri = R[i], r2 = (double)(r - 2);
        double q = kNjNone; int32_t bi = i, bj = kNjNoSlot;
        // (loads and selects only, lanes_for4: with the flag tested first and a pass at a time a launch took 12 us at 2 048 slots, two
        // memory latencies a pass)
        lanes_for4(i + 1, n, [&](int j, bool valid) {
            const bool on = valid & (active[j] != 0);
            const double v = nj_sub(nj_sub(nj_mul(r2, row[j]), ri), R[j]);
            const bool take = on & nj_before(v, i, j, q, bi, bj);
            q = take ? v : q; bj = take ? j : bj;
        });
        wave_argmin_f64(q, bi, bj);
        if (wave_leader()) { row_q[i] = q; row_j[i] = bj == kNjNoSlot ? -1 : bj; }
    }
};

// ONE workgroup of 256 threads, launched as 256 items of the thread-per-item launch: on the device the 256 calls are the threads of
// one workgroup, which meet at the barriers; in the emulation call 0 plays every thread and the others return.
// (1) every thread takes the rows t, t + 256, ... and keeps the best (Q, i, j); a butterfly per wavefront, the four results through
//     LDS, and every thread folds the four: (i, j) is uniform over the workgroup without a broadcast.
// (2) every thread reads dij, ri, rj; thread 0 writes the record.  BARRIER: nothing below may overwrite what (1) and (2) read.
// (3) the threads take the k: du, R[k], D[i][k] and D[k][i].  Thread 0 writes R[i] and retires slot j.
struct NjJoin {
    double* D; double* R; uint8_t* active; int32_t n; int32_t r;
    const double* row_q; const int32_t* row_j; NjJoinRec* rec;
    PM_HD void operator()(int64_t tid) const {
#if !defined(__HIP_DEVICE_COMPILE__)
        if (tid != 0) return;
#endif
        (void)tid;
        PM_GROUP_SHARED double sh_q[kNjGroup / 64];
        PM_GROUP_SHARED int32_t sh_i[kNjGroup / 64], sh_j[kNjGroup / 64];
        double q = kNjNone; int32_t bi = kNjNoSlot, bj = kNjNoSlot;
        struct Row { double q; int32_t j; bool on; };
        group_for4<Row>(n,      // (a retired row's rowmin is stale, its flag says so)
            [&](int a, bool valid) { return Row{row_q[a], row_j[a], (bool)(valid & (active[a] != 0))}; },
            [&](int a, const Row& w) {
                const bool take = w.on & (w.j >= 0) & nj_before(w.q, a, w.j, q, bi, bj);
                q = take ? w.q : q; bi = take ? a : bi; bj = take ? w.j : bj;
            });
        wave_argmin_f64(q, bi, bj);
#if defined(__HIP_DEVICE_COMPILE__)
        const int wv = nj_thread() >> 6;
        if ((nj_thread() & 63) == 0) { sh_q[wv] = q; sh_i[wv] = bi; sh_j[wv] = bj; }
        group_sync();
#pragma unroll
        for (int k = 0; k < kNjGroup / 64; k++)
            if (nj_before(sh_q[k], sh_i[k], sh_j[k], q, bi, bj)) { q = sh_q[k]; bi = sh_i[k]; bj = sh_j[k]; }
#else
        (void)sh_q; (void)sh_i; (void)sh_j;
#endif
        if (bj == kNjNoSlot) return;       // (uniform; r >= 4 active slots: a pair exists, so this never leaves -- no index is formed from "none")
        const int32_t i = bi, j = bj;
        const double dij = D[(int64_t)i * n + j], ri = R[i], rj = R[j];
        if (nj_thread() == 0) *rec = NjJoinRec{i, j, dij, ri, rj};
        group_sync();
        double* row_i = D + (int64_t)i * n;
        const double* row_jj = D + (int64_t)j * n;
        struct Col { double dik, djk, rk; bool on; };
        group_for4<Col>(n,
            [&](int k, bool valid) { return Col{row_i[k], row_jj[k], R[k], (bool)(valid & (k != i) & (k != j) & (active[k] != 0))}; },
            [&](int k, const Col& c) {
                if (!c.on) return;
                const double du = nj_mul(nj_sub(nj_add(c.dik, c.djk), dij), 0.5);
                R[k] = nj_add(nj_sub(nj_sub(c.rk, c.dik), c.djk), du);
                row_i[k] = du;
                D[(int64_t)k * n + i] = du;
            });
        if (nj_thread() == 0) {
            R[i] = nj_mul(nj_sub(nj_add(ri, rj), nj_mul((double)r, dij)), 0.5);
            active[j] = 0;
        }
    }
};

// one wavefront: the three slots still active, in ascending order, from ballots over the flags (uniform: every lane walks the same
// bits), and their three distances
struct NjLast {
    const double* D; const uint8_t* active; int32_t n; NjLastRec* rec;
    PM_HD void wave(int64_t) const {
        int32_t slot[3] = {0, 0, 0};
        int found = 0;
        for (int32_t base = 0; base < n; base += 64) {
            uint64_t m = wave_ballot_of([&](int t) { return base + t < n && active[base + t] != 0; });
            while (m && found < 3) { slot[found++] = base + ctz64(m); m &= m - 1; }
        }
        if (wave_leader() && found == 3) {
            const int64_t a = slot[0], b = slot[1], c = slot[2];
            *rec = NjLastRec{slot[0], slot[1], slot[2], D[a * n + b], D[a * n + c], D[b * n + c]};
        }
    }
};

}  // namespace pm
