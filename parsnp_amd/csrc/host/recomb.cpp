// recomb.cpp -- [Output] recomb=1: the recombination scan of the core SNP columns.  The engine holds the letters of
// the columns (the collection of snps.cpp); the host holds their cluster, column within the LCB and reference position.  The engine
// says which columns are informative (pm_rec_sites); the host lists the informative sites of every LCB as printed and cuts the lists
// into windows; the engine scores the pairs of every window (pm_rec_incompat) and tests every window against its permutations
// (pm_rec_test); nothing but phi and le of every window comes back.  Two files with the XMFA's stem:
//   <stem>.rec.tsv   a line per window: cluster, first and last column within the LCB, smallest and largest reference position,
//                    sites, phi, le, perms, p = (le + 1) / (perms + 1)
//   <stem>.rec       the upstream driver's BED record of every window with 100 (le + 1) < perms + 1, by first reference position
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "aligner.h"
#include "engine_step.h"

// Weak, like the pm_nj_* calls: a provider of the ABI without them still links; recomb=1 then ends the run.
extern "C" int pm_rec_limits(int* max_rows, int* max_window_sites, int* max_perms) __attribute__((weak));
extern "C" int pm_rec_sites(pm_session* s, uint8_t* informative, int64_t* n_informative) __attribute__((weak));
extern "C" int pm_rec_incompat(pm_session* s, int64_t n_sites, const int64_t* sites, int64_t n_windows, const int64_t* win_off, uint8_t* inc_out) __attribute__((weak));
extern "C" int pm_rec_test(pm_session* s, int64_t n_windows, const int64_t* win_off, const uint8_t* inc, int32_t near, int32_t perms, uint64_t seed,
                           const int64_t* win_id, int32_t* phi, int32_t* le) __attribute__((weak));

namespace parsnp {
RecCounts rec_counts;

void rec_limits(int* rows, int* sites, int* perms) {
    *rows = 2048; *sites = 256; *perms = 65536;
    if (pm_rec_limits) (void)pm_rec_limits(rows, sites, perms);
}

// the starts of the windows over a site list of length m: none below kRecMinSites, one below K, else steps of K / 2 and a last one
// that ends at m
std::vector<size_t> rec_window_starts(size_t m, size_t K) {
    std::vector<size_t> starts;
    if (m < kRecMinSites) return starts;
    if (m < K) { starts.push_back(0); return starts; }
    const size_t step = K / 2;
    for (size_t s = 0; s + K <= m; s += step) starts.push_back(s);
    if (starts.back() + K != m) starts.push_back(m - K);
    return starts;
}

std::vector<RecWindow> rec_windows(const std::vector<RecColumn>& cols, const uint8_t* informative, size_t K, std::vector<int64_t>* sites, std::vector<int64_t>* win_off) {
    std::vector<RecWindow> out;
    sites->clear(); win_off->assign(1, 0);
    std::vector<int64_t> list;
    for (size_t a = 0; a < cols.size(); ) {
        size_t b = a;
        while (b < cols.size() && cols[b].cluster == cols[a].cluster) b++;      // an LCB as printed: a run of columns of one cluster
        list.clear();
        for (size_t c = a; c < b; c++) if (informative[c]) list.push_back((int64_t)c);
        const size_t k = std::min(K, list.size());
        for (size_t s : rec_window_starts(list.size(), K)) {
            RecWindow w;
            w.cluster = cols[(size_t)list[s]].cluster; w.first_column = cols[(size_t)list[s]].column; w.last_column = cols[(size_t)list[s + k - 1]].column;
            w.first_ref = w.last_ref = cols[(size_t)list[s]].ref_pos; w.sites = (int32_t)k;
            for (size_t i = s; i < s + k; i++) {
                const int64_t r = cols[(size_t)list[i]].ref_pos;
                w.first_ref = std::min(w.first_ref, r); w.last_ref = std::max(w.last_ref, r);
                sites->push_back(list[i]);
            }
            win_off->push_back((int64_t)sites->size());
            out.push_back(w);
        }
        a = b;
    }
    return out;
}

bool rec_flagged(int32_t le, int32_t perms) { return 100 * ((int64_t)le + 1) < (int64_t)perms + 1; }

std::string rec_tsv_text(const std::vector<RecWindow>& win, const int32_t* phi, const int32_t* le, int32_t perms) {
    std::string text = "cluster\tfirst_column\tlast_column\tfirst_ref\tlast_ref\tsites\tphi\tle\tperms\tp\n";
    char buf[256];
    for (size_t g = 0; g < win.size(); g++) {
        const RecWindow& w = win[g];
        const double p = (double)(le[g] + 1) / (double)(perms + 1);
        snprintf(buf, sizeof buf, "%d\t%lld\t%lld\t%lld\t%lld\t%d\t%d\t%d\t%d\t%.6f\n", w.cluster, (long long)w.first_column, (long long)w.last_column,
                 (long long)w.first_ref, (long long)w.last_ref, w.sites, phi[g], le[g], perms, p);
        text += buf;
    }
    return text;
}

std::string rec_bed_text(const std::vector<RecWindow>& win, const int32_t* le, int32_t perms, long* flagged) {
    std::vector<size_t> hit;
    for (size_t g = 0; g < win.size(); g++) if (rec_flagged(le[g], perms)) hit.push_back(g);
    std::stable_sort(hit.begin(), hit.end(), [&](size_t a, size_t b) { return win[a].first_ref < win[b].first_ref; });      // (then g: stable)
    std::string text;
    char buf[128];
    for (size_t g : hit) {
        snprintf(buf, sizeof buf, "1\t%lld\t%lld\tREC\t%.3f\t+\n", (long long)win[g].first_ref, (long long)win[g].last_ref + 1, (double)(le[g] + 1) / (double)(perms + 1));
        text += buf;
    }
    if (flagged) *flagged = (long)hit.size();
    return text;
}

void write_recomb(pm_session* session, const std::vector<RecColumn>& cols, const RecParams& prm, const std::string& dir, const std::string& stem) {
    if (!pm_rec_sites || !pm_rec_incompat || !pm_rec_test) {
        std::cerr << "parsnp_core: this provider of the engine's ABI cannot scan for recombination (recomb=1)" << std::endl;
        exit(1);
    }
    double ms = 0;
    auto step = [&](int rc, const char* what) {
        engine_check(rc, std::string("cannot scan for recombination (") + what + ")");
        ms += phase_ms(session, "rec_", true);
    };
    std::vector<uint8_t> informative(cols.size());
    int64_t n_inf = 0;
    step(pm_rec_sites(session, informative.data(), &n_inf), "sites");
    std::vector<int64_t> sites, win_off;
    const std::vector<RecWindow> win = rec_windows(cols, informative.data(), (size_t)prm.sites, &sites, &win_off);
    std::vector<int32_t> phi(win.size()), le(win.size());
    if (!win.empty()) {
        step(pm_rec_incompat(session, (int64_t)sites.size(), sites.data(), (int64_t)win.size(), win_off.data(), nullptr), "scores");
        step(pm_rec_test(session, (int64_t)win.size(), win_off.data(), nullptr, prm.near, prm.perms, prm.seed, nullptr, phi.data(), le.data()), "permutations");
    }
    long flagged = 0;
    const std::string bed = rec_bed_text(win, le.data(), prm.perms, &flagged);
    {
        std::ofstream out((dir + stem + ".rec.tsv").c_str(), std::ios::binary);
        out << rec_tsv_text(win, phi.data(), le.data(), prm.perms);
    }
    {
        std::ofstream out((dir + stem + ".rec").c_str(), std::ios::binary);
        out << bed;
    }
    rec_counts.on = true; rec_counts.sites = (long)n_inf; rec_counts.windows = (long)win.size(); rec_counts.flagged = flagged; rec_counts.ms = ms;
    std::cerr << "Recombination scan: " << win.size() << " windows of " << n_inf << " informative sites, " << flagged << " flagged" << std::endl;
}

}  // namespace parsnp
