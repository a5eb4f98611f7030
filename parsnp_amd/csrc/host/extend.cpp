// extend.cpp -- [Output] lcbext=1: every printed LCB grows into the unaligned bases beside it.  The host knows the
// interval of every record of the XMFA; from them it derives the covered stretches of every genome, the two jobs of every LCB (side
// L, side R) and a descriptor per row -- where the row's flank begins in its genome, which way it is read, whether it is
// complemented, how long it is.  The engine aligns every row's flank against the reference's and cuts the job where all rows still
// pass (pm_ext_reach), then walks the paths back and merges them into columns (pm_ext_align): only descriptors go up, only reaches
// and rows come back.  The host formats the records and writes <stem>.xmfa.extended: the XMFA's header lines, then for every kept job
// a record per row (`> i:lo-hi s clusterC L|R`) and `=`.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "aligner.h"
#include "engine_step.h"

// Weak, like the pm_rec_* calls: a provider of the ABI without them still links; lcbext=1 then ends the run.
extern "C" int pm_ext_limits(int* max_rows, int* max_flank, int* max_band) __attribute__((weak));
extern "C" int pm_ext_reach(pm_session* s, const pm_ext_params* params, int64_t n_jobs, const int64_t* row_off, const pm_ext_row* rows, int32_t* reach, int32_t* best)
    __attribute__((weak));
extern "C" int pm_ext_align(pm_session* s, const pm_ext_params* params, int64_t n_jobs, const int64_t* row_off, const pm_ext_row* rows, const int32_t* reach,
                            int64_t max_cols, const int64_t* out_off, uint8_t* out_rows, int32_t* cols, int32_t* used) __attribute__((weak));

namespace parsnp {
ExtCounts ext_counts;

void ext_limits(int* rows, int* flank, int* band) {
    *rows = 2048; *flank = 512; *band = 63;
    if (pm_ext_limits) (void)pm_ext_limits(rows, flank, band);
}

// the header lines of the XMFA (output.cpp writes its own with it)
std::string ext_header_text(const std::vector<Genome>& genomes, int printable) {
    std::string t = "#FormatVersion Mauve\n#SequenceCount " + std::to_string(genomes.size()) + "\n";
    for (size_t i = 0; i < genomes.size(); i++) {
        t += "##SequenceIndex " + std::to_string(i + 1) + "\n##SequenceFile " + genomes[i].fname + "\n##SequenceHeader " + genomes[i].header + "\n";
        t += "##SequenceLength " + std::to_string(genomes[i].size_nopad) + "bp\n";
    }
    return t + "#IntervalCount " + std::to_string(printable) + "\n";
}

// per genome the covered stretches [a, b), 0-based, ascending and merged
ExtCovered ext_covered(const std::vector<std::vector<ExtRecord>>& lcbs, const std::vector<int64_t>& lens) {
    ExtCovered cov(lens.size());
    for (const auto& recs : lcbs)
        for (const ExtRecord& r : recs) {
            const size_t g = (size_t)r.seq - 1;
            const int64_t a = std::max<int64_t>(r.lo - 1, 0), b = std::min<int64_t>(std::max<int64_t>(r.hi, 0), lens[g]);
            if (a < b) cov[g].emplace_back(a, b);
        }
    for (auto& v : cov) {
        std::sort(v.begin(), v.end());
        size_t k = 0;
        for (size_t i = 0; i < v.size(); i++) {
            if (k && v[i].first <= v[k - 1].second) v[k - 1].second = std::max(v[k - 1].second, v[i].second);
            else v[k++] = v[i];
        }
        v.resize(k);
    }
    return cov;
}

// The flank of a record on a side: read away from the LCB in the orientation in which the XMFA prints the row.  The uncovered run it
// enters is halved where its other end touches a record too (the low side takes the odd base); the flank ends before the first
// letter that is none of ACGT and at F.
pm_ext_row ext_flank(const std::string& seq, const std::vector<std::pair<int64_t, int64_t>>& cov, const ExtRecord& r, char side, int F) {
    const bool up = (side == 'R') == r.fwd;
    const int64_t glen = (int64_t)seq.size();
    pm_ext_row row;
    row.genome = r.seq - 1; row.step = up ? 1 : -1; row.complement = r.fwd ? 0 : 1; row.len = 0; row.first = up ? r.hi : r.lo - 2;
    if (row.first < 0 || row.first >= glen) { row.first = 0; return row; }
    // the first covered stretch that ends after `first`
    auto it = std::upper_bound(cov.begin(), cov.end(), row.first, [](int64_t p, const std::pair<int64_t, int64_t>& s) { return p < s.second; });
    if (it != cov.end() && it->first <= row.first) { row.first = 0; return row; }      // (covered)
    const int64_t run_hi = it != cov.end() ? it->first : glen, run_lo = it != cov.begin() ? (it - 1)->second : 0;
    int64_t avail;
    if (up) { const int64_t run = run_hi - row.first; avail = it != cov.end() ? (run + 1) / 2 : run; }
    else { const int64_t run = row.first + 1 - run_lo; avail = it != cov.begin() ? run / 2 : run; }
    avail = std::min<int64_t>(avail, F);
    int32_t n = 0;
    while (n < avail) {
        const char c = seq[(size_t)(row.first + (int64_t)n * row.step)];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'a' && c != 'c' && c != 'g' && c != 't') break;
        n++;
    }
    row.len = n;
    if (!n) row.first = 0;
    return row;
}

// the records of a kept job: rows of `cols` letters at `pitch`, in the flank's own order (side L prints them reversed)
std::string ext_job_text(const std::vector<ExtRecord>& recs, const pm_ext_row* rows, const int32_t* used, const uint8_t* letters, int64_t pitch, int32_t cols, char side) {
    std::string t;
    char buf[160];
    for (size_t r = 0; r < recs.size(); r++) {
        long long lo = 0, hi = 0;
        if (used[r] > 0) {
            const long long a = (long long)rows[r].first, b = a + (long long)(used[r] - 1) * rows[r].step;
            lo = std::min(a, b) + 1; hi = std::max(a, b) + 1;
        }
        const int w = snprintf(buf, sizeof buf, "> %d:%lld-%lld %c cluster%d %c\n", recs[r].seq, lo, hi, recs[r].fwd ? '+' : '-', recs[r].cluster, side);
        t.append(buf, (size_t)w);
        const uint8_t* src = letters + (int64_t)r * pitch;
        for (int32_t k = 0; k < cols; k += 80) {
            const int32_t n = std::min(80, cols - k);
            for (int32_t q = 0; q < n; q++) t += (char)(side == 'L' ? src[cols - 1 - (k + q)] : src[k + q]);
            t += '\n';
        }
    }
    return t + "=\n";
}

void write_extended(pm_session* session, const std::vector<Genome>& genomes, int printable, const std::vector<std::vector<ExtRecord>>& lcbs, const ExtSettings& st,
                    const std::string& dir, const std::string& stem, int threads) {
    if (!pm_ext_reach || !pm_ext_align || !session) {
        std::cerr << "parsnp_core: this provider of the engine's ABI cannot extend the LCBs (lcbext=1)" << std::endl;
        exit(1);
    }
    double ms = 0;
    auto step = [&](int rc, const char* what) {
        engine_check(rc, std::string("cannot extend the LCBs (") + what + ")");
        ms += phase_ms(session, "ext_", true);
    };
    std::vector<int64_t> lens;
    for (const Genome& g : genomes) lens.push_back((int64_t)g.seq.size());
    const ExtCovered cov = ext_covered(lcbs, lens);
    const pm_ext_params prm{st.match, st.mismatch, st.gap, st.band, st.ani, st.min_len, st.max_flank};
    const int64_t pitch = 2 * (int64_t)st.max_flank;
    std::ofstream out((dir + stem + ".xmfa.extended").c_str(), std::ios::binary);
    out << ext_header_text(genomes, printable);
    ExtCounts cnt;
    cnt.on = true;
    const size_t nl = lcbs.size();
    constexpr size_t kChunkPairs = (size_t)1 << 18;      // rows of one round trip: their letters come back at 2 F bytes a row
    for (size_t z0 = 0; z0 < nl; ) {
        size_t z1 = z0, pairs = 0;
        while (z1 < nl && (z1 == z0 || pairs + 2 * lcbs[z1].size() <= kChunkPairs)) pairs += 2 * lcbs[z1++].size();
        const size_t nj = 2 * (z1 - z0);
        std::vector<int64_t> row_off(nj + 1, 0), out_off(nj);
        for (size_t j = 0; j < nj; j++) { row_off[j + 1] = row_off[j] + (int64_t)lcbs[z0 + j / 2].size(); out_off[j] = row_off[j] * pitch; }
        std::vector<pm_ext_row> rows(pairs);
#pragma omp parallel for schedule(dynamic, 16) num_threads(threads)
        for (long j = 0; j < (long)nj; j++) {
            const std::vector<ExtRecord>& recs = lcbs[z0 + (size_t)j / 2];
            for (size_t r = 0; r < recs.size(); r++)
                rows[(size_t)row_off[(size_t)j] + r] = ext_flank(genomes[(size_t)recs[r].seq - 1].seq, cov[(size_t)recs[r].seq - 1], recs[r], j % 2 ? 'R' : 'L', st.max_flank);
        }
        std::vector<int32_t> reach(nj), cols(nj), used(pairs);
        std::vector<uint8_t> letters(pairs * (size_t)pitch);
        step(pm_ext_reach(session, &prm, (int64_t)nj, row_off.data(), rows.data(), reach.data(), nullptr), "reach");
        step(pm_ext_align(session, &prm, (int64_t)nj, row_off.data(), rows.data(), reach.data(), pitch, out_off.data(), letters.data(), cols.data(), used.data()), "columns");
        std::vector<std::string> text(nj);
#pragma omp parallel for schedule(dynamic, 16) num_threads(threads)
        for (long j = 0; j < (long)nj; j++)
            if (cols[(size_t)j] > 0)
                text[(size_t)j] = ext_job_text(lcbs[z0 + (size_t)j / 2], rows.data() + row_off[(size_t)j], used.data() + row_off[(size_t)j], letters.data() + out_off[(size_t)j],
                                               pitch, cols[(size_t)j], j % 2 ? 'R' : 'L');
        for (size_t j = 0; j < nj; j++) {
            cnt.jobs++;
            if (cols[j] < 0) cnt.wide++;
            if (cols[j] > 0) { cnt.kept++; cnt.bases += reach[j]; out << text[j]; }
        }
        z0 = z1;
    }
    cnt.ms = ms;
    ext_counts = cnt;
    std::cerr << "LCB extension: " << cnt.jobs << " jobs, " << cnt.kept << " kept, " << cnt.bases << " reference bases added" << std::endl;
}

}  // namespace parsnp
