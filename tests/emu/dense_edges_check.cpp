// dense_edges_check.cpp -- TEST INFRASTRUCTURE ONLY: the suffix-array path of the event search (dense_kernels.h, dense_build) in the kernel
// emulation as a program of its own, so that it can be compiled with -fsanitize=address,undefined and run as a plain process (never loaded
// into python, never run on a device).  argv[1]: the case file that tests/densegen.py write_cases() wrote --
//   PAIR name L strand count / reference / query / count lines "l j len rep'": one call of pm_find_events, the restatement's events of that
//        strand sorted by (l, j, len, rep'), rep' zeroed below K;
//   BATCH name ngen nreg / the genomes / per region "L starts.. lens.. count" and count lines "k len sp.. fwd..": one call of
//        pm_multi_mum_batch with group_small = 1 and one with 0, the restatement's multi-MUMs of every region.
// Every session takes the path: PARSNP_TUNE=dense_all=1 is set here (pm_find_events opens its session itself).  What the sanitizers are
// for: sym_at and the LCE reads past a piece or a strand, shifts, and any index that leaves a buffer.  A read ONE element past lcp[] or a
// rank array stays inside the buffer's slack (Engine::ensure allocates n + n / 4 + 16 elements) and is not seen here: that is what
// test_smaller_call_after_a_larger is designed for.
#include <cstdio>
#include <fstream>
#include <tuple>
#include "engine_emu.cpp"

static int fails = 0;
static std::string g_case;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (case %s)\n", __LINE__, #c, g_case.c_str()); fails++; } } while (0)
typedef std::tuple<int64_t, int64_t, int64_t, int64_t> Event;

static void run_pair(const std::string& ref, const std::string& q, int L, int strand, const std::vector<Event>& want) {
    const int64_t cap = (int64_t)q.size() + 16;
    std::vector<int64_t> j((size_t)cap), l((size_t)cap); std::vector<int32_t> n((size_t)cap), r((size_t)cap);
    int64_t count = -1;
    if (pm_find_events((const uint8_t*)ref.data(), (int64_t)ref.size(), (const uint8_t*)q.data(), (int64_t)q.size(), L, strand, cap, &count,
                       j.data(), l.data(), n.data(), r.data()) != PM_OK) { CHECK(!"pm_find_events"); return; }
    CHECK(count >= 0 && count <= cap);
    std::vector<Event> got;
    for (int64_t i = 0; i < count && i < cap; i++) got.push_back(Event(l[(size_t)i], j[(size_t)i], n[(size_t)i], r[(size_t)i]));
    std::sort(got.begin(), got.end());
    CHECK(got == want);
}

struct Got { std::vector<int64_t> off; std::vector<int32_t> k, lon, sp; std::vector<uint8_t> fwd; float regions = -1; bool ok = false; };

static Got run_batch(const std::vector<std::string>& seqs, int64_t nreg, const std::vector<int64_t>& starts, const std::vector<int64_t>& lens, const std::vector<int32_t>& mins, int group) {
    std::vector<const uint8_t*> p; std::vector<int64_t> l;
    for (const auto& s : seqs) { p.push_back((const uint8_t*)s.data()); l.push_back((int64_t)s.size()); }
    pm_session* s = nullptr;
    Got g;
    if (pm_session_create(&s, -1, (int)seqs.size(), p.data(), l.data()) != PM_OK) { CHECK(!"session"); return g; }
    CHECK(pm_session_tune(s, "dense_all", 1) == PM_OK && pm_session_tune(s, "group_small", group) == PM_OK);
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
    for (int i = 0; i < cnt; i++) if (!strcmp(names[i], "dense_regions")) g.regions = ms[i];
    pm_session_destroy(s);
    g.ok = true;
    return g;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: dense_edges_check CASES (tests/densegen.py write_cases)\n"); return 2; }
    setenv("PARSNP_TUNE", "dense_all=1", 1);
    std::ifstream in(argv[1]);
    std::string word;
    int npairs = 0, nbatches = 0; int64_t nevents = 0, nmums = 0;
    while (in >> word) {
        if (word == "PAIR") {
            int L, strand; int64_t count;
            std::string ref, q;
            in >> g_case >> L >> strand >> count >> ref >> q;
            std::vector<Event> want((size_t)count);
            for (Event& e : want) in >> std::get<0>(e) >> std::get<1>(e) >> std::get<2>(e) >> std::get<3>(e);
            if (!in) { printf("case file ends inside case %s\n", g_case.c_str()); return 2; }
            run_pair(ref, q, L, strand, want);
            npairs++; nevents += count;
        } else if (word == "BATCH") {
            int ngen; int64_t nreg;
            in >> g_case >> ngen >> nreg;
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
            for (int group : {1, 0}) {
                const Got g = run_batch(seqs, nreg, starts, lens, mins, group);
                CHECK(g.ok && g.off == off && g.k == k && g.lon == lon && g.sp == sp && g.fwd == fwd);
                CHECK(g.regions == (float)nreg);
            }
            nbatches++; nmums += (int64_t)k.size();
        } else { printf("bad case file at '%s'\n", word.c_str()); return 2; }
    }
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("%lld events, %lld multi-MUMs\n", (long long)nevents, (long long)nmums);
    printf("dense_edges_check ok: %d pairs, %d batches\n", npairs, nbatches);
    return 0;
}
