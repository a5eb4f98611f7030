// snp_dist_host.cpp -- the plain host loop scripts/snp_measure.py compares SnpDist with (not part of the product): the same two bit
// planes, row-major here (words of one row side by side), every pair i < j by one thread, OpenMP over i.
#include <cstdint>

extern "C" void snp_dist_host(const uint64_t* lo, const uint64_t* hi, int n, long words, int32_t* dist, int threads) {
#pragma omp parallel for schedule(dynamic, 4) num_threads(threads)
    for (int i = 0; i < n; i++) {
        dist[(long)i * n + i] = 0;
        for (int j = i + 1; j < n; j++) {
            const uint64_t *li = lo + (long)i * words, *hi_i = hi + (long)i * words, *lj = lo + (long)j * words, *hj = hi + (long)j * words;
            long d = 0;
            for (long w = 0; w < words; w++) d += __builtin_popcountll((li[w] ^ lj[w]) | (hi_i[w] ^ hj[w]));
            dist[(long)i * n + j] = dist[(long)j * n + i] = (int32_t)d;
        }
    }
}
