// nj_host.cpp -- the plain host program scripts/nj_measure.py compares the device's neighbour joining with (not part of the product):
// the definition of INTEGRATION.md 1b, a row's smallest Q by one thread, OpenMP over the rows; the arg-min over the rows and the
// record by one thread; the update of row / column i over the k in parallel.  Built without FMA (no -march=native): the doubles
// must round as the definition says.
#include <cstddef>
#include <cstdint>
#include <vector>

struct Join { int32_t i, j; double dij, ri, rj; };
struct Last { int32_t a, b, c; double dab, dac, dbc; };

extern "C" void nj_host(const int32_t* dist, int n, Join* joins, Last* last, int threads) {
    const long N = n;
    std::vector<double> D((size_t)(N * N)), R((size_t)N), rq((size_t)N);
    std::vector<int32_t> rj((size_t)N);
    std::vector<uint8_t> act((size_t)N, 1);
#pragma omp parallel for schedule(static) num_threads(threads)
    for (long i = 0; i < N; i++) {
        int64_t sum = 0;
        for (long j = 0; j < N; j++) { D[i * N + j] = (double)dist[i * N + j]; sum += dist[i * N + j]; }
        R[i] = (double)sum;
    }
    for (int t = 0; t + 3 < n; t++) {
        const int r = n - t;
        const double r2 = (double)(r - 2);
#pragma omp parallel for schedule(dynamic, 16) num_threads(threads)
        for (long i = 0; i < N; i++) {
            if (!act[i]) continue;
            double best = __builtin_huge_val(); int32_t bj = -1;
            const double* row = &D[i * N];
            const double ri = R[i];
            for (long j = i + 1; j < N; j++) {
                if (!act[j]) continue;
                const double q = r2 * row[j] - ri - R[j];
                if (q < best) { best = q; bj = (int32_t)j; }
            }
            rq[i] = best; rj[i] = bj;
        }
        int32_t bi = -1, bj = -1; double best = __builtin_huge_val();
        for (long i = 0; i < N; i++) if (act[i] && rj[i] >= 0 && rq[i] < best) { best = rq[i]; bi = (int32_t)i; bj = rj[i]; }
        const long i = bi, j = bj;
        const double dij = D[i * N + j], ri = R[i], rjv = R[j];
        joins[t] = Join{bi, bj, dij, ri, rjv};
#pragma omp parallel for schedule(static) num_threads(threads)
        for (long k = 0; k < N; k++) {
            if (k == i || k == j || !act[k]) continue;
            const double dik = D[i * N + k], djk = D[j * N + k];
            const double du = ((dik + djk) - dij) * 0.5;
            R[k] = ((R[k] - dik) - djk) + du;
            D[i * N + k] = du; D[k * N + i] = du;
        }
        R[i] = ((ri + rjv) - (double)r * dij) * 0.5;
        act[j] = 0;
    }
    int32_t s[3]; int f = 0;
    for (long k = 0; k < N && f < 3; k++) if (act[k]) s[f++] = (int32_t)k;
    *last = Last{s[0], s[1], s[2], D[(long)s[0] * N + s[1]], D[(long)s[0] * N + s[2]], D[(long)s[1] * N + s[2]]};
}
