// cand_rows_check.cpp -- TEST INFRASTRUCTURE ONLY: the candidate side of pm_multi_mum_batch (Master.EP, the candidate listing, the fold, the
// compaction into (sp, fwd) or MUM rows, the overlap flags of a long one-region list) in the kernel emulation as a program of its own,
// so that it can be compiled with -fsanitize=address,undefined and run as a plain process (never loaded into python, never run on a
// device).  argv[1]: the case file that tests/candrows.py write_case() wrote -- per case the sequences, the row mode and the tunes, then
// every call with its request rows and what the sequential restatement expects of it: offsets, k, lon and either (sp, fwd) or the MUM
// rows with their PM_ROW_* bits, whether the list is a long one (dirty_known, an anchor table), and what is known of "tail_repeats".
#include <cstdio>
#include <fstream>
#include "engine_emu.cpp"

static int fails = 0;
static std::string g_case;
static int g_call = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (case %s, call %d)\n", __LINE__, #c, g_case.c_str(), g_call); fails++; } } while (0)

template <class T> static std::vector<T> take(std::ifstream& in, int64_t n) {
    std::vector<T> v((size_t)n);
    for (auto& x : v) { int64_t y; in >> y; x = (T)y; }
    return v;
}
template <class T, class U> static bool same(const T* got, const std::vector<U>& want) {
    if (!got) return want.empty();
    for (size_t i = 0; i < want.size(); i++) if ((int64_t)got[i] != (int64_t)want[i]) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: cand_rows_check CASES (tests/candrows.py write_case)\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string word;
    int ncases = 0, ngen = 0, mode = 0;
    int64_t ncalls = 0, nrows = 0;
    pm_session* s = nullptr;
    std::vector<pm_result*> kept;
    while (in >> word) {
        if (word == "CASE") {
            int64_t ntunes;
            in >> g_case >> ngen >> mode >> ntunes;
            g_call = 0;
            std::vector<std::pair<std::string, int64_t>> tunes((size_t)ntunes);
            for (auto& t : tunes) in >> t.first >> t.second;
            std::vector<std::string> seqs((size_t)ngen);
            for (auto& x : seqs) in >> x;
            if (!in) { printf("bad case file in the head of case %s\n", g_case.c_str()); return 2; }
            std::vector<const uint8_t*> p; std::vector<int64_t> l;
            for (const auto& x : seqs) { p.push_back((const uint8_t*)x.data()); l.push_back((int64_t)x.size()); }
            if (pm_session_create(&s, -1, ngen, p.data(), l.data()) != PM_OK) { printf("no session for case %s\n", g_case.c_str()); return 1; }
            for (const auto& t : tunes) CHECK(pm_session_tune(s, t.first.c_str(), t.second) == PM_OK);
            CHECK(pm_session_rows(s, mode) == PM_OK);
        } else if (word == "CALL") {
            int64_t nreg, tail, total, long_list = 0;
            in >> nreg;
            const std::vector<int64_t> starts = take<int64_t>(in, nreg * ngen), lens = take<int64_t>(in, nreg * ngen);
            const std::vector<int32_t> minsize = take<int32_t>(in, nreg);
            in >> tail >> total;
            const std::vector<int64_t> off = take<int64_t>(in, nreg + 1), k = take<int64_t>(in, total), lon = take<int64_t>(in, total);
            const int64_t nq = ngen - 1;
            std::vector<int64_t> a, b, flags;
            if (mode == 0) { a = take<int64_t>(in, total * nq); b = take<int64_t>(in, total * nq); }
            else { a = take<int64_t>(in, total * ngen); b = take<int64_t>(in, total * ngen); flags = take<int64_t>(in, total); in >> long_list; }
            if (!in) { printf("case file ends inside case %s\n", g_case.c_str()); return 2; }
            pm_result* r = nullptr;
            if (pm_multi_mum_batch(s, nreg, starts.data(), lens.data(), minsize.data(), &r) != PM_OK) { printf("call %d of case %s failed: %s\n", g_call, g_case.c_str(), pm_last_error()); return 1; }
            kept.push_back(r);
            int count = 64; const char* names[64]; float ms[64];
            CHECK(pm_last_timing(s, &count, names, ms) == PM_OK);
            float repeats = 0;
            for (int i = 0; i < count; i++) if (!strcmp(names[i], "tail_repeats")) repeats = ms[i];
            CHECK(tail < 0 || (tail == 0 ? repeats == 0 : repeats >= 1));
            CHECK(pm_result_regions(r) == nreg && pm_result_total(r) == total);
            if (pm_result_total(r) == total) {
                CHECK(same(pm_result_offsets(r), off) && same(pm_result_k(r), k) && same(pm_result_lon(r), lon));
                if (mode == 0) CHECK(same(pm_result_sp(r), a) && same(pm_result_fwd(r), b));
                else {
                    CHECK(!pm_result_sp(r) && !pm_result_fwd(r));
                    CHECK(same(pm_result_flags(r), flags));
                    CHECK(pm_result_dirty_known(r) == (int)long_list && (pm_result_table_id(r) != 0) == (long_list != 0));
                    if (total && !pm_result_start(r)) {
                        CHECK(mode == 2 && long_list && pm_result_store_base(r) == 0 && !pm_result_strand(r));
                        std::vector<int32_t> st((size_t)(total * ngen)); std::vector<uint8_t> sd((size_t)(total * ngen));
                        CHECK(pm_store_rows(s, nullptr, 0, total, 1, st.data(), sd.data()) == PM_OK);
                        CHECK(same(st.data(), a) && same(sd.data(), b));
                    } else CHECK(same(pm_result_start(r), a) && same(pm_result_strand(r), b));
                }
            }
            ncalls++; nrows += total;
            g_call++;
        } else if (word == "END") {
            for (pm_result* r : kept) pm_result_free(r);
            kept.clear();
            pm_session_destroy(s); s = nullptr;
            ncases++;
        } else { printf("bad case file at '%s'\n", word.c_str()); return 2; }
    }
    if (s) { printf("case file ends without END\n"); return 2; }
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("cand_rows_check ok: %d cases, %lld calls, %lld rows\n", ncases, (long long)ncalls, (long long)nrows);
    return 0;
}
