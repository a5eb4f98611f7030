// ext_host.cpp -- the LCB extension of INTEGRATION.md 1e as a host program with OpenMP threads: what the device path (ext_kernels.h) is
// measured against by scripts/ext_measure.py.  The same definition, a line of the band at a time: the left moves of a line are a running
// maximum, the moves are kept as bytes for the walk back.
//
//   ext_host JOBS.bin THREADS      JOBS.bin: int32 match, mismatch, gap, band, ani, min_len, max_flank; int64 n_jobs; int64
//                                  row_off[n_jobs + 1]; int32 len[rows]; the rows' letters one after the other
//   prints one JSON line: reach_ms, align_ms, and the sums the device's results must equal: reach, kept, wide, cols, used, and an
//   position-weighted byte sum (mod 2^64) over the rows of every kept job in order
#include <omp.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

struct Prm { int32_t match, mismatch, gap, band, ani, min_len, max_flank; };
static const int NEG = -(1 << 28);

// the table of a pair up to line Lmax; best[i] per line (INT_MIN: no cell); mv (or null): 1 diagonal, 2 up, 3 left per cell (i, d)
static void table(const Prm& p, const uint8_t* a, int Lmax, const uint8_t* b, int Lb, int* best, uint8_t* mv, int* last) {
    const int W = p.band, D = 2 * W + 1;
    std::vector<int> prev(D + 2, NEG), cur(D + 2, NEG);      // index d + 1, guards at both ends
    for (int i = 0; i <= Lmax; i++) {
        best[i] = INT_MIN;
        std::fill(cur.begin(), cur.end(), NEG);
        for (int d = 0; d < D; d++) {
            const int j = i + d - W;
            if (j < 0 || j > Lb) continue;
            int h, m = 0;
            if (i == 0 && j == 0) h = 0;
            else {
                const int dv = (i > 0 && j > 0 ? prev[d + 1] : NEG) + (i > 0 && j > 0 && a[i - 1] == b[j - 1] ? p.match : -p.mismatch);
                const int uv = (i > 0 ? prev[d + 2] : NEG) - p.gap, lv = cur[d] - p.gap;
                h = std::max(dv, std::max(uv, lv));
                m = h == dv ? 1 : h == uv ? 2 : 3;
            }
            cur[d + 1] = h;
            if (h > best[i]) best[i] = h;
            if (mv) mv[(size_t)i * D + d] = (uint8_t)m;
        }
        if (last && i == Lmax) for (int d = 0; d < D; d++) last[d] = cur[d + 1];
        prev.swap(cur);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    Prm p; int64_t nj = 0;
    if (!f || fread(&p, sizeof p, 1, f) != 1 || fread(&nj, 8, 1, f) != 1) return 1;
    std::vector<int64_t> off((size_t)nj + 1);
    if (fread(off.data(), 8, off.size(), f) != off.size()) return 1;
    const size_t np = (size_t)off.back();
    std::vector<int32_t> len(np);
    if (fread(len.data(), 4, np, f) != np) return 1;
    std::vector<size_t> at(np + 1, 0);
    for (size_t r = 0; r < np; r++) at[r + 1] = at[r] + (size_t)len[r];
    std::vector<uint8_t> text(at.back() + 1);
    if (at.back() && fread(text.data(), 1, at.back(), f) != at.back()) return 1;
    fclose(f);
    omp_set_num_threads(atoi(argv[2]));
    const int F = p.max_flank, D = 2 * p.band + 1, need = p.ani * p.match - (100 - p.ani) * p.mismatch;
    std::vector<int32_t> reach((size_t)nj, 0), cols((size_t)nj, 0), used(np, 0);
    std::vector<std::string> rows((size_t)nj);

    const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel
    {
        std::vector<int> best((size_t)F + 1);
        std::vector<uint8_t> pass((size_t)F + 1);
#pragma omp for schedule(dynamic, 1)
        for (int64_t j = 0; j < nj; j++) {
            const size_t r0 = (size_t)off[(size_t)j], r1 = (size_t)off[(size_t)j + 1];
            const int La = len[r0];
            std::fill(pass.begin(), pass.end(), 1);
            for (size_t r = r0; r < r1; r++) {
                table(p, &text[at[r0]], La, &text[at[r]], len[r], best.data(), nullptr, nullptr);
                for (int i = 1; i <= La; i++) if (best[(size_t)i] == INT_MIN || 100 * best[(size_t)i] < i * need) pass[(size_t)i] = 0;
            }
            int A = 0;
            for (int i = 1; i <= La; i++) if (pass[(size_t)i]) A = i;
            reach[(size_t)j] = A >= p.min_len ? A : 0;
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
#pragma omp parallel
    {
        std::vector<int> best((size_t)F + 1), last((size_t)D);
        std::vector<uint8_t> mv((size_t)(F + 1) * (size_t)D);
#pragma omp for schedule(dynamic, 1)
        for (int64_t j = 0; j < nj; j++) {
            const int A = reach[(size_t)j];
            if (!A) continue;
            const size_t r0 = (size_t)off[(size_t)j], r1 = (size_t)off[(size_t)j + 1], n = r1 - r0;
            std::vector<uint16_t> ins(n * (size_t)(A + 1), 0);
            std::vector<uint8_t> has(n * (size_t)A, 0);
            for (size_t r = r0; r < r1; r++) {
                table(p, &text[at[r0]], A, &text[at[r]], len[r], best.data(), mv.data(), last.data());
                int d = 0;
                while (last[(size_t)d] != best[(size_t)A]) d++;
                int i = A, jj = A + d - p.band;
                used[r] = jj;
                while (i > 0 || jj > 0) {
                    const int m = mv[(size_t)i * D + (size_t)d];
                    if (m == 1) { i--; jj--; has[(r - r0) * (size_t)A + (size_t)i] = 1; }
                    else if (m == 2) { i--; d++; }
                    else { jj--; d--; ins[(r - r0) * (size_t)(A + 1) + (size_t)i]++; }
                }
            }
            std::vector<int> w((size_t)A + 1, 0);
            int C = A;
            for (int k = 0; k <= A; k++) { for (size_t r = 0; r < n; r++) w[(size_t)k] = std::max<int>(w[(size_t)k], ins[r * (size_t)(A + 1) + (size_t)k]); C += w[(size_t)k]; }
            if (C > 2 * F) { cols[(size_t)j] = -1; continue; }
            cols[(size_t)j] = C;
            std::string& out = rows[(size_t)j];
            out.reserve(n * (size_t)C);
            for (size_t r = 0; r < n; r++) {
                const uint8_t* b = &text[at[r0 + r]];
                int q = 0;
                for (int k = 0; k <= A; k++) {
                    const int m = ins[r * (size_t)(A + 1) + (size_t)k];
                    for (int x = 0; x < w[(size_t)k]; x++) out += x < m ? (char)b[q + x] : '-';
                    q += m;
                    if (k < A) { if (has[r * (size_t)A + (size_t)k]) out += (char)b[q++]; else out += '-'; }
                }
            }
        }
    }
    const auto t2 = std::chrono::steady_clock::now();
    long long sr = 0, sc = 0, su = 0, kept = 0, wide = 0;
    uint64_t h = 0, idx = 0;
    for (int64_t j = 0; j < nj; j++) {
        sr += reach[(size_t)j]; kept += cols[(size_t)j] > 0; wide += cols[(size_t)j] < 0; sc += std::max(cols[(size_t)j], 0);
        for (unsigned char c : rows[(size_t)j]) h += (uint64_t)c * (idx++ % 65521 + 1);
    }
    for (size_t r = 0; r < np; r++) su += used[r];
    printf("{\"jobs\": %lld, \"pairs\": %zu, \"reach_ms\": %.3f, \"align_ms\": %.3f, \"sum_reach\": %lld, \"kept\": %lld, \"wide\": %lld, \"sum_cols\": %lld, \"sum_used\": %lld, \"rows_hash\": \"%016llx\"}\n",
           (long long)nj, np, std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count(), sr, kept, wide, sc, su,
           (unsigned long long)h);
    return 0;
}
