// index_buckets_check.cpp -- TEST INFRASTRUCTURE ONLY: the index build by buckets (index_kernels.h) in the kernel emulation as a program
// of its own, so that it can be compiled with -fsanitize=address,undefined and run as a plain process (never loaded into python, never
// run on a device).  argv[1]: the case file that tests/indexgen.py write_cases() wrote -- every case of indexgen.CASES at its full
// length and the mixed batch of 24 regions (some bucketed, some not: the host's layout of both kinds of slice, the first-bucket table
// with its ties), each with its tunes, its genomes, its regions, the multi-MUMs of the restatement and the counts the emulation
// reported to python.  Every case runs with index_build = 1 and = 0 under index_verify: the restatement's multi-MUMs both times,
// index_lost = 0, and by buckets the same index_bucketed and index_overflow.
#include <cstdio>
#include <fstream>
#include "engine_emu.cpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (case %s)\n", __LINE__, #c, g_case.c_str()); fails++; } } while (0)
static std::string g_case;
struct Got { std::vector<int64_t> off; std::vector<int32_t> k, lon, sp; std::vector<uint8_t> fwd; float bucketed = -1, overflow = -1, lost = -1; bool ok = false; };
struct Tune { std::string key; int64_t value; };

static Got run(const std::vector<std::string>& seqs, int64_t nreg, const std::vector<int64_t>& starts, const std::vector<int64_t>& lens, const std::vector<int32_t>& mins,
               int build, const std::vector<Tune>& tunes) {
    std::vector<const uint8_t*> p; std::vector<int64_t> l;
    for (const auto& s : seqs) { p.push_back((const uint8_t*)s.data()); l.push_back((int64_t)s.size()); }
    pm_session* s = nullptr;
    Got g;
    if (pm_session_create(&s, -1, (int)seqs.size(), p.data(), l.data()) != PM_OK) { CHECK(!"session"); return g; }
    for (const Tune& t : tunes) CHECK(pm_session_tune(s, t.key.c_str(), t.value) == PM_OK);
    CHECK(pm_session_tune(s, "index_build", build) == PM_OK && pm_session_tune(s, "index_verify", 1) == PM_OK);
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
        if (!strcmp(names[i], "index_bucketed")) g.bucketed = ms[i];
        if (!strcmp(names[i], "index_overflow")) g.overflow = ms[i];
        if (!strcmp(names[i], "index_lost")) g.lost = ms[i];
    }
    pm_session_destroy(s);
    g.ok = true;
    return g;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: index_buckets_check CASES (tests/indexgen.py write_cases)\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string word;
    int ncases = 0;
    while (in >> word) {
        if (word != "CASE") { printf("bad case file at '%s'\n", word.c_str()); return 2; }
        int ntunes, ngen; int64_t nreg, bucketed, overflow;
        in >> g_case >> ntunes >> ngen >> nreg >> bucketed >> overflow;
        std::vector<Tune> tunes((size_t)ntunes);
        for (Tune& t : tunes) in >> t.key >> t.value;
        std::vector<std::string> seqs((size_t)ngen);
        for (auto& s : seqs) in >> s;
        const int nq = ngen - 1;
        std::vector<int64_t> starts((size_t)(nreg * ngen)), lens((size_t)(nreg * ngen)), off{0}; std::vector<int32_t> mins((size_t)nreg), k, lon, sp; std::vector<uint8_t> fwd;
        for (int64_t r = 0; r < nreg; r++) {
            int64_t count;
            in >> mins[(size_t)r];
            for (int g = 0; g < ngen; g++) in >> starts[(size_t)(r * ngen + g)];
            for (int g = 0; g < ngen; g++) in >> lens[(size_t)(r * ngen + g)];
            in >> count;
            for (int64_t c = 0; c < count; c++) {
                int64_t v;
                in >> v; k.push_back((int32_t)v);
                in >> v; lon.push_back((int32_t)v);
                for (int g = 0; g < nq; g++) { in >> v; sp.push_back((int32_t)v); }
                for (int g = 0; g < nq; g++) { in >> v; fwd.push_back((uint8_t)v); }
            }
            off.push_back(off.back() + count);
        }
        if (!in) { printf("case file ends inside case %s\n", g_case.c_str()); return 2; }
        for (int build : {1, 0}) {
            const Got g = run(seqs, nreg, starts, lens, mins, build, tunes);
            CHECK(g.ok && g.off == off && g.k == k && g.lon == lon && g.sp == sp && g.fwd == fwd);
            CHECK(g.lost == 0);
            if (build) CHECK(g.bucketed == (float)bucketed && g.overflow == (float)overflow);
            else CHECK(g.bucketed == 0 && g.overflow == 0);
        }
        printf("%s: %lld regions, %zu multi-MUMs, %lld positions by buckets, %lld overflow records\n", g_case.c_str(), (long long)nreg, k.size(), (long long)bucketed, (long long)overflow);
        ncases++;
    }
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("index_buckets_check ok: %d cases\n", ncases);
    return 0;
}
