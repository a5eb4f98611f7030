// rec_host.cpp -- the recombination scan of INTEGRATION.md 1d as a host program with OpenMP threads, written for the comparison of
// DESIGN.md §8 (scripts/rec_measure.py builds and runs it; not part of the product).  The same definition as rec_kernels.h: bit sets
// over the rows per column and letter, the 4 x 4 edge mask of a pair by AND-and-test over the row words, the score from the mask, the
// permuted orders by sorting (key, index) pairs, T by look-ups in the window's matrix.  The windows are spread over the threads.
//
//   rec_host IN.bin K H P SEED THREADS
//   IN.bin: int64 n, int64 V, uint8 letters[n][V] (A C G T), int32 cluster[V]
//   prints one JSON line: windows, informative, flagged, the sums of phi and le, a hash of (phi, le) in order g, and the
//   wall-clock milliseconds of the three steps
#include <omp.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

static uint64_t mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static int score(uint32_t mask) {
    uint32_t r[4];
    for (int a = 0; a < 4; a++) r[a] = (mask >> (4 * a)) & 15u;
    const int E = __builtin_popcount(mask), Vx = (r[0] != 0) + (r[1] != 0) + (r[2] != 0) + (r[3] != 0), Vy = __builtin_popcount(r[0] | r[1] | r[2] | r[3]);
    for (int sweep = 0; sweep < 3; sweep++)
        for (int a = 0; a < 4; a++)
            for (int b = a + 1; b < 4; b++)
                if (r[a] & r[b]) r[a] = r[b] = r[a] | r[b];
    int C = 0;
    for (int a = 0; a < 4; a++) {
        bool first = r[a] != 0;
        for (int b = 0; b < a; b++) first = first && !(r[a] & r[b]);
        C += first;
    }
    return E - Vx - Vy + C;
}
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: rec_host IN.bin K H P SEED THREADS\n"); return 2; }
    const size_t K = (size_t)atol(argv[2]);
    const int H = atoi(argv[3]), P = atoi(argv[4]);
    const uint64_t seed = strtoull(argv[5], nullptr, 10);
    omp_set_num_threads(atoi(argv[6]));
    FILE* f = fopen(argv[1], "rb");
    int64_t n = 0, V = 0;
    if (!f || fread(&n, 8, 1, f) != 1 || fread(&V, 8, 1, f) != 1) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    std::vector<uint8_t> letters((size_t)(n * V));
    std::vector<int32_t> cluster((size_t)V);
    if (fread(letters.data(), 1, letters.size(), f) != letters.size() || fread(cluster.data(), 4, (size_t)V, f) != (size_t)V) { fprintf(stderr, "short file\n"); return 1; }
    fclose(f);

    const double t0 = now_ms();
    const size_t RB = (size_t)(n + 63) / 64;
    std::vector<uint64_t> sets((size_t)V * 4 * RB, 0);      // [column][letter code][row word]
    std::vector<uint8_t> informative((size_t)V, 0);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < V; c++) {
        uint64_t* S = sets.data() + (size_t)c * 4 * RB;
        int cnt[4] = {0, 0, 0, 0};
        for (int64_t r = 0; r < n; r++) {
            const int code = (letters[(size_t)(r * V + c)] >> 1) & 3;
            S[(size_t)code * RB + (size_t)(r >> 6)] |= 1ull << (r & 63);
            cnt[code]++;
        }
        informative[(size_t)c] = (uint8_t)(((cnt[0] >= 2) + (cnt[1] >= 2) + (cnt[2] >= 2) + (cnt[3] >= 2)) >= 2);
    }
    std::vector<int64_t> sites, win_off(1, 0), list;
    long n_inf = 0;
    for (int64_t a = 0; a < V;) {
        int64_t b = a;
        while (b < V && cluster[(size_t)b] == cluster[(size_t)a]) b++;
        list.clear();
        for (int64_t c = a; c < b; c++) if (informative[(size_t)c]) list.push_back(c);
        n_inf += (long)list.size();
        const size_t m = list.size(), k = std::min(K, m);
        std::vector<size_t> starts;
        if (m >= 16 && m < K) starts.push_back(0);
        else if (m >= K) {
            for (size_t s = 0; s + K <= m; s += K / 2) starts.push_back(s);
            if (starts.back() + K != m) starts.push_back(m - K);
        }
        for (size_t s : starts) {
            for (size_t i = s; i < s + k; i++) sites.push_back(list[i]);
            win_off.push_back((int64_t)sites.size());
        }
        a = b;
    }
    const size_t nw = win_off.size() - 1;
    const double t1 = now_ms();

    std::vector<std::vector<uint8_t>> mats(nw);
#pragma omp parallel for schedule(dynamic, 1)
    for (size_t w = 0; w < nw; w++) {
        const size_t k = (size_t)(win_off[w + 1] - win_off[w]);
        const int64_t* st = sites.data() + win_off[w];
        std::vector<uint8_t>& M = mats[w];
        M.assign(k * k, 0);
        for (size_t x = 0; x < k; x++)
            for (size_t y = x + 1; y < k; y++) {
                const uint64_t* X = sets.data() + (size_t)st[x] * 4 * RB;
                const uint64_t* Y = sets.data() + (size_t)st[y] * 4 * RB;
                uint32_t mask = 0;
                for (int a = 0; a < 4; a++)
                    for (int b = 0; b < 4; b++) {
                        uint64_t any = 0;
                        for (size_t i = 0; i < RB; i++) any |= X[(size_t)a * RB + i] & Y[(size_t)b * RB + i];
                        if (any) mask |= 1u << (a * 4 + b);
                    }
                M[x * k + y] = M[y * k + x] = (uint8_t)score(mask);
            }
    }
    const double t2 = now_ms();

    std::vector<int32_t> phi(nw), le(nw);
#pragma omp parallel
    {
        std::vector<std::pair<uint64_t, int32_t>> keys;
        std::vector<int32_t> order;
#pragma omp for schedule(dynamic, 1)
        for (size_t w = 0; w < nw; w++) {
            const int32_t k = (int32_t)(win_off[w + 1] - win_off[w]);
            const int32_t h = std::min(H, k - 1);
            const uint8_t* M = mats[w].data();
            auto stat = [&](const int32_t* o) {
                int32_t t = 0;
                for (int32_t i = 0; i < k; i++) {
                    const uint8_t* row = M + (size_t)o[i] * (size_t)k;
                    for (int32_t j = i + 1; j <= i + h && j < k; j++) t += row[o[j]];
                }
                return t;
            };
            order.resize((size_t)k); keys.resize((size_t)k);
            for (int32_t i = 0; i < k; i++) order[(size_t)i] = i;
            const int32_t phi0 = stat(order.data());
            const uint64_t wkey = mix(seed + (uint64_t)w);
            int32_t count = 0;
            for (int32_t p = 0; p < P; p++) {
                const uint64_t pkey = mix(wkey + (uint64_t)p);
                for (int32_t i = 0; i < k; i++) keys[(size_t)i] = std::make_pair(mix(pkey + (uint64_t)i), i);
                std::sort(keys.begin(), keys.end());
                for (int32_t i = 0; i < k; i++) order[(size_t)i] = keys[(size_t)i].second;
                count += stat(order.data()) <= phi0;
            }
            phi[w] = phi0; le[w] = count;
        }
    }
    const double t3 = now_ms();
    long long sum_phi = 0, sum_le = 0, flagged = 0;
    uint64_t hash = 0;
    for (size_t w = 0; w < nw; w++) {
        sum_phi += phi[w]; sum_le += le[w]; flagged += 100LL * (le[w] + 1) < (long long)P + 1;
        hash = mix(hash ^ (((uint64_t)(uint32_t)phi[w] << 32) | (uint32_t)le[w]));
    }
    printf("{\"windows\": %zu, \"informative\": %ld, \"flagged\": %lld, \"sum_phi\": %lld, \"sum_le\": %lld, \"hash\": \"%016llx\", "
           "\"sites_ms\": %.3f, \"incompat_ms\": %.3f, \"permute_ms\": %.3f, \"threads\": %d}\n",
           nw, n_inf, flagged, sum_phi, sum_le, (unsigned long long)hash, t1 - t0, t2 - t1, t3 - t2, atoi(argv[6]));
    return 0;
}
