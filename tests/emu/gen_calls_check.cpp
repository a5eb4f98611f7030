// gen_calls_check.cpp -- TEST INFRASTRUCTURE ONLY: the generation calls of the resident route's recursion (pm_store_search /
// _search_beside, pm_store_validate, pm_store_order_check) in the kernel emulation as a program of its own, so that it can be compiled
// with -fsanitize=address,undefined and run as a plain process (never loaded into python, never run on a device).  argv[1]: the
// case file that tests/gencalls.py write_cases() wrote -- per case the sequences, the anchor call's minimum length, q and the tunes,
// then every search and validation list as the generation former made it.  From the sequential restatement: the children in listed
// order (ref_start, ref_len, slength, parent), (state, shift, len, start0) of every row of the listed regions -- processed or still
// waiting -- and the layout's marks per genome at the end (how many, and the sum of their positions).  From the emulation's own run in
// python, where tests/gencalls.py had checked them against the restatement's properties (they are the engine's answers, not the
// restatement's): first_row and the offsets, trouble, second_stage_ran, done[] and the order check's word.
#include <cstdio>
#include <fstream>
#include "engine_emu.cpp"

static int fails = 0;
static std::string g_case;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (case %s, call %d)\n", __LINE__, #c, g_case.c_str(), g_call); fails++; } } while (0)
static int g_call = 0;
static int g_beside = 0;

template <class T> static std::vector<T> take(std::ifstream& in, int64_t n) {
    std::vector<T> v((size_t)n);
    if (n == 0) { std::string dash; in >> dash; return v; }      // (an empty list is written as "-")
    for (auto& x : v) { int64_t y; in >> y; x = (T)y; }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: gen_calls_check CASES (tests/gencalls.py write_cases)\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string word;
    int ncases = 0;
    pm_session* s = nullptr;
    pm_result* anchors = nullptr;
    int ngen = 0;
    int64_t rows_total = 0, searches = 0, validations = 0, q_case = 0;
    while (in >> word) {
        if (word == "CASE") {
            int64_t ams, q, ntunes;
            in >> g_case >> ngen >> ams >> q >> ntunes;
            g_call = 0;
            std::vector<std::pair<std::string, int64_t>> tunes((size_t)ntunes);
            for (auto& t : tunes) in >> t.first >> t.second;
            std::vector<std::string> seqs((size_t)ngen);
            for (auto& x : seqs) in >> x;
            int64_t nseeds = -1;
            in >> word >> nseeds;
            if (!in || word != "SEEDS") { printf("bad case file in the head of case %s\n", g_case.c_str()); return 2; }
            std::vector<const uint8_t*> p; std::vector<int64_t> l, zero((size_t)ngen, 0);
            for (const auto& x : seqs) { p.push_back((const uint8_t*)x.data()); l.push_back((int64_t)x.size()); }
            if (pm_session_create(&s, -1, ngen, p.data(), l.data()) != PM_OK) { printf("no session for case %s\n", g_case.c_str()); return 1; }
            for (const auto& t : tunes) CHECK(pm_session_tune(s, t.first.c_str(), t.second) == PM_OK);
            CHECK(pm_session_rows(s, 2) == PM_OK);
            const int32_t minsize = (int32_t)ams;
            if (pm_multi_mum_batch(s, 1, zero.data(), l.data(), &minsize, &anchors) != PM_OK) { printf("the anchor call of case %s failed\n", g_case.c_str()); return 1; }
            rows_total = pm_result_total(anchors);
            std::vector<pm_row_info> info((size_t)rows_total);
            int64_t nreg = -1;
            CHECK(pm_result_table_id(anchors) != 0 && pm_store_settle_seeds(s, pm_result_table_id(anchors), (int32_t)q, info.data(), &nreg) == PM_OK);
            CHECK(nreg == nseeds);
            q_case = q;
        } else if (word == "SEARCH") {
            int64_t n, beside, first_want;
            in >> n >> beside;
            const std::vector<int32_t> ids = take<int32_t>(in, n), mins = take<int32_t>(in, n);
            in >> first_want;
            const std::vector<int64_t> off_want = take<int64_t>(in, n + 1);
            std::vector<int64_t> off((size_t)n + 1, -1);
            int64_t first = -1;
            g_beside = 0;
            if (beside) CHECK(pm_store_search_beside(s, ids.data(), mins.data(), n, &first, off.data(), [](void*) { g_beside++; }, nullptr) == PM_OK && g_beside == 1);
            else CHECK(pm_store_search(s, ids.data(), mins.data(), n, &first, off.data()) == PM_OK);
            CHECK(first == first_want && first == rows_total && off == off_want);
            rows_total += off[(size_t)n];
            searches++;
        } else if (word == "VALIDATE") {
            int64_t nreg, ncl, gi, stage_first, trouble_want, ran_want, nkids_want, nrows;
            in >> nreg >> ncl >> gi >> stage_first;
            const std::vector<int32_t> ids = take<int32_t>(in, nreg);
            const std::vector<int64_t> row0 = take<int64_t>(in, nreg);
            const std::vector<int32_t> cnt = take<int32_t>(in, nreg);
            const std::vector<int64_t> first = take<int64_t>(in, ncl + 1);
            in >> trouble_want >> ran_want;
            const std::vector<int32_t> done_want = take<int32_t>(in, ncl);
            in >> nkids_want;
            const std::vector<int64_t> kids_want = take<int64_t>(in, 4 * nkids_want);
            in >> nrows;
            const std::vector<int64_t> rows_want = take<int64_t>(in, 5 * nrows);
            if (!in) { printf("case file ends inside case %s\n", g_case.c_str()); return 2; }
            int64_t lo = INT64_MAX, hi = -1;
            for (int64_t i = 0; i < nreg; i++) if (cnt[(size_t)i] > 0) { lo = std::min(lo, row0[(size_t)i]); hi = std::max(hi, row0[(size_t)i] + cnt[(size_t)i]); }
            std::vector<pm_row_info> info(hi > lo ? (size_t)(hi - lo) : 0);
            std::vector<int32_t> done((size_t)ncl, -7);
            uint32_t trouble = 0x55; int64_t nkids = -1; int32_t ran = -1;
            CHECK(pm_store_validate(s, ids.data(), row0.data(), cnt.data(), nreg, first.data(), ncl, (int32_t)q_case, &trouble, &nkids, hi > lo ? lo : 0, hi > lo ? hi - lo : 0,
                                    hi > lo ? info.data() : nullptr, stage_first, &ran, (int32_t)gi, done.data()) == PM_OK);
            CHECK((int64_t)trouble == trouble_want && ran == ran_want && done == done_want && nkids == nkids_want);
            const pm_region_info* kids = pm_store_new_regions(s);
            for (int64_t i = 0; i < nkids && i < nkids_want; i++) {
                const int64_t* w = kids_want.data() + 4 * i;
                CHECK(kids[i].ref_start == w[0] && kids[i].ref_len == w[1] && kids[i].slength == w[2] && kids[i].parent == w[3]);
                CHECK(i == 0 || kids[i].key > kids[i - 1].key);
            }
            for (int64_t i = 0; i < nrows; i++) {
                const int64_t* w = rows_want.data() + 5 * i;
                if (w[0] < lo || w[0] >= hi) { CHECK(!"a listed row outside the info range"); continue; }
                const pm_row_info& g = info[(size_t)(w[0] - lo)];
                CHECK((int64_t)(g.state_flags & 0xffu) == w[1] && g.shift == w[2] && g.len == w[3] && g.start0 == w[4]);
            }
            if (!info.empty()) {
                std::vector<pm_row_info> again(info.size());
                CHECK(pm_store_info(s, lo, hi - lo, again.data()) == PM_OK && !memcmp(again.data(), info.data(), sizeof(pm_row_info) * info.size()));
            }
            validations++;
            g_call++;
        } else if (word == "END") {
            int64_t order_want;
            in >> order_want;
            const std::vector<int64_t> marks_want = take<int64_t>(in, 2 * (int64_t)ngen);
            uint32_t order = 0x55;
            CHECK(pm_store_order_check(s, &order) == PM_OK && (int64_t)order == order_want);
            std::vector<int64_t> off((size_t)ngen + 1);
            const int64_t words = pm_store_layout_words(s, off.data());
            std::vector<uint64_t> img((size_t)words);
            CHECK(pm_store_layout(s, img.data(), words) == PM_OK);
            for (int j = 0; j < ngen; j++) {
                int64_t count = 0, sum = 0;
                for (int64_t w = off[(size_t)j]; w < off[(size_t)j + 1]; w++)
                    for (int b = 0; b < 64; b++) if (img[(size_t)w] >> b & 1) { count++; sum += (w - off[(size_t)j]) * 64 + b; }
                CHECK(count == marks_want[2 * (size_t)j] && sum == marks_want[2 * (size_t)j + 1]);
            }
            pm_result_free(anchors); anchors = nullptr;
            pm_session_destroy(s); s = nullptr;
            printf("%s: %d generations replayed\n", g_case.c_str(), g_call);
            ncases++;
        } else { printf("bad case file at '%s'\n", word.c_str()); return 2; }
        if (!in) { printf("case file ends inside case %s\n", g_case.c_str()); return 2; }
    }
    if (s) { printf("case file ends without END\n"); return 2; }
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("gen_calls_check ok: %d cases, %lld searches, %lld validations\n", ncases, (long long)searches, (long long)validations);
    return 0;
}
