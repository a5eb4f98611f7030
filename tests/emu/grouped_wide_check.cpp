// grouped_wide_check.cpp -- TEST INFRASTRUCTURE ONLY: GroupedPairEventsWide (store_kernels.h) in the kernel emulation as a program of
// its own, so that it can be compiled with -fsanitize=address,undefined and run as a plain process (never loaded into python, never
// run on a device).  It builds the piece batches of tests/groupedwide.py in small -- 200 query genomes of 4 kb that carry exactly 33
// and exactly 128 distinct pieces in each of 16 windows of 64-128 bases (version v: one private substitution at position v / 3 of
// every window), every fifth genome with a third of it inverted, and 1 100 genomes with 5 pieces (the wide form alone) -- and runs each
// through pm_multi_mum_batch with group_wide = 1, by default (the wide form is off), with group_wide = 0 and with group_small = 0, under both orders of the wide launch's
// wavefronts: the same multi-MUMs every time, and the counts of pm_last_timing say which form took the regions.
#include <cstdio>
#include <random>
#include "engine_emu.cpp"

static std::string revcomp(const std::string& s) {
    std::string o(s.rbegin(), s.rend());
    for (char& c : o) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return o;
}
struct Got { std::vector<int64_t> off; std::vector<int32_t> k, lon, sp; std::vector<uint8_t> fwd; float wide = 0, back = 0, grouped = 0; };
static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static Got run(const std::vector<std::string>& seqs, int64_t nreg, const std::vector<int64_t>& starts, const std::vector<int64_t>& lens, const std::vector<int32_t>& mins,
               const char* key, int64_t value) {
    std::vector<const uint8_t*> p; std::vector<int64_t> l;
    for (const auto& s : seqs) { p.push_back((const uint8_t*)s.data()); l.push_back((int64_t)s.size()); }
    pm_session* s = nullptr;
    Got g;
    if (pm_session_create(&s, -1, (int)seqs.size(), p.data(), l.data()) != PM_OK) { CHECK(!"session"); return g; }
    if (key) CHECK(pm_session_tune(s, key, value) == PM_OK);
    pm_result* res = nullptr;
    if (pm_multi_mum_batch(s, nreg, starts.data(), lens.data(), mins.data(), &res) != PM_OK) { CHECK(!"batch"); pm_session_destroy(s); return g; }
    const int64_t total = pm_result_total(res), q = (int64_t)seqs.size() - 1;
    g.off.assign(pm_result_offsets(res), pm_result_offsets(res) + nreg + 1);
    if (total) {
        g.k.assign(pm_result_k(res), pm_result_k(res) + total); g.lon.assign(pm_result_lon(res), pm_result_lon(res) + total);
        g.sp.assign(pm_result_sp(res), pm_result_sp(res) + total * q); g.fwd.assign(pm_result_fwd(res), pm_result_fwd(res) + total * q);
    }
    pm_result_free(res);
    int cnt = 64; const char* names[64]; float ms[64];
    CHECK(pm_last_timing(s, &cnt, names, ms) == PM_OK);
    for (int i = 0; i < cnt; i++) {
        if (!strcmp(names[i], "n_grouped_wide")) g.wide = ms[i];
        if (!strcmp(names[i], "n_handed_back")) g.back = ms[i];
        if (!strcmp(names[i], "n_grouped")) g.grouped = ms[i];
    }
    pm_session_destroy(s);
    return g;
}
static bool same(const Got& a, const Got& b) { return a.off == b.off && a.k == b.k && a.lon == b.lon && a.sp == b.sp && a.fwd == b.fwd; }

static void batch(uint64_t seed, int nq, int npieces, bool expect_wide) {
    std::mt19937_64 rng(seed);
    const int glen = 4000, nreg = 16, a = glen / 4, b = a + glen / 3;
    std::string ref(glen, 'A');
    for (char& c : ref) c = "ACGT"[rng() % 4];
    std::vector<std::pair<int, int>> wins;
    while ((int)wins.size() < nreg) {
        const int ln = 64 + (int)(rng() % 65), st = 8 + (int)(rng() % (glen - 16 - ln));
        bool ok = !(st <= a && a < st + ln) && !(st <= b && b < st + ln);
        for (auto& w : wins) if (st < w.first + w.second + 2 && w.first < st + ln + 2) ok = false;
        if (ok) wins.push_back({st, ln});
    }
    std::vector<std::string> versions;
    for (int v = 0; v < npieces; v++) {
        std::string s = ref;
        for (auto& w : wins) { char& c = s[w.first + v / 3]; const char* all = "ACGT"; c = all[(strchr(all, c) - all + 1 + v % 3) % 4]; }
        versions.push_back(s);
    }
    std::vector<int> inv_v, fwd_v;
    for (int v = 0; v < npieces; v++) (v % 5 == 4 ? inv_v : fwd_v).push_back(v);
    std::vector<std::string> seqs{ref}; std::vector<char> inverted{0};
    size_t ni = 0, nf = 0;
    for (int g = 0; g < nq; g++) {
        const bool inv = g % 5 == 4 && !inv_v.empty();
        std::string q = inv ? versions[inv_v[ni++ % inv_v.size()]] : versions[fwd_v[nf++ % fwd_v.size()]];
        if (inv) q = q.substr(0, a) + revcomp(q.substr(a, b - a)) + q.substr(b);
        seqs.push_back(q); inverted.push_back(inv);
    }
    const int ngen = nq + 1;
    std::vector<int64_t> starts((size_t)nreg * ngen), lens((size_t)nreg * ngen); std::vector<int32_t> mins(nreg);
    for (int r = 0; r < nreg; r++) {
        for (int g = 0; g < ngen; g++) {
            const bool inside = inverted[g] && a <= wins[r].first && wins[r].first + wins[r].second <= b;
            starts[(size_t)r * ngen + g] = inside ? a + b - wins[r].first - wins[r].second : wins[r].first;
            lens[(size_t)r * ngen + g] = wins[r].second;
        }
        mins[r] = 8 + (int)(rng() % 5);
    }
    unsetenv("PM_EMU_REVERSE_WAVES");
    const Got plain = run(seqs, nreg, starts, lens, mins, "group_small", 0);
    const Got first = run(seqs, nreg, starts, lens, mins, "group_wide", 0);
    const Got dflt = run(seqs, nreg, starts, lens, mins, nullptr, 0);
    const Got wide = run(seqs, nreg, starts, lens, mins, "group_wide", 1);
    setenv("PM_EMU_REVERSE_WAVES", "grouped_pair_events_wide", 1);
    const Got rev = run(seqs, nreg, starts, lens, mins, "group_wide", 1);
    unsetenv("PM_EMU_REVERSE_WAVES");
    CHECK(!plain.k.empty());
    CHECK(same(plain, first)); CHECK(same(plain, wide)); CHECK(same(plain, rev));
    CHECK(plain.grouped == 0 && first.wide == 0 && first.back == -1);
    CHECK(same(plain, dflt) && dflt.wide == 0 && dflt.back == -1 && dflt.grouped == first.grouped);
    CHECK((wide.wide > 0) == expect_wide && wide.back == 0 && rev.wide == wide.wide && rev.grouped == wide.grouped);
    printf("nq %d pieces %d: %zu multi-MUMs, %.0f grouped events, %.0f of them by the wide form\n", nq, npieces, plain.k.size(), wide.grouped, wide.wide);
}

int main() {
    batch(33, 200, 33, true);
    batch(128, 200, 128, true);
    batch(32, 200, 32, false);
    batch(1100, 1100, 5, true);
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("grouped_wide_check ok\n");
    return 0;
}
