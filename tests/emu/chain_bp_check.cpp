// chain_bp_check.cpp -- TEST INFRASTRUCTURE ONLY: phases C-D for a diagonal difference given in bases (pm_store_chain_begin with
// diag_diff > 1; store_kernels.h: ChainWindow, ChainSelect, ChainWindowFill) in the kernel emulation as a program of its own, so
// that it can be compiled with -fsanitize=address,undefined and run as a plain process (never loaded into python, never run on a
// device).  It builds lists in the manner of tests/chainbp.py -- blocks of 20 unique bases one substituted base apart in 3 genomes;
// 28 bases inserted in genome 1 in front of a run of p blocks, which are passed, and then either deleted again (the block behind
// joins) or a run of d + 1 substituted bases (it closes) -- for p = 1, 2, 3, 63, 64, 65, and p = 8 and 9 under "chain_window" = 8,
// and checks the byte per MUM, the counters, pm_store_chain_passed and, where the cap is met, that the layout has not changed.
#include <cstdio>
#include <random>
#include "engine_emu.cpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static std::string bases(std::mt19937_64& rng, int n) { std::string s((size_t)n, 'A'); for (char& c : s) c = "ACGT"[rng() % 4]; return s; }
static std::string other(std::mt19937_64& rng, const std::string& s) {
    std::string o = s;
    for (char& c : o) { const char* all = "ACGT"; c = all[(strchr(all, c) - all + 1 + rng() % 3) % 4]; }
    return o;
}

// lead blocks, the run of p passed blocks, the block that ends it, two more
static void list(uint64_t seed, int p, bool join, int d, int64_t window, bool expect_trouble) {
    std::mt19937_64 rng(seed);
    const int D = 25, lead = 5, n = 3;
    std::vector<std::string> g((size_t)n);
    auto block = [&] { const std::string b = bases(rng, 20); for (auto& s : g) s += b; };
    auto site = [&](int r, int ins, int del) {      // a run of r bases substituted in the query genomes; genome 1 gains ins bases behind it or loses its last del
        const std::string a = bases(rng, r), b = other(rng, a);
        g[0] += a; g[1] += b.substr(0, (size_t)(r - del)) + bases(rng, ins); g[2] += b;
    };
    block();
    for (int i = 1; i < lead; i++) { site(1, 0, 0); block(); }
    site(3, D + 3, 0); block();
    for (int i = 1; i < p; i++) { site(1, 0, 0); block(); }
    if (join) site(D + 4, 0, D + 3); else site(d + 1, 0, 0);
    block();
    for (int i = 0; i < 2; i++) { site(1, 0, 0); block(); }
    const int64_t nm = lead + p + 3;

    std::vector<const uint8_t*> ptr; std::vector<int64_t> len;
    for (const auto& s : g) { ptr.push_back((const uint8_t*)s.data()); len.push_back((int64_t)s.size()); }
    pm_session* s = nullptr;
    if (pm_session_create(&s, -1, n, ptr.data(), len.data()) != PM_OK) { CHECK(!"session"); return; }
    CHECK(pm_session_tune(s, "dirty_min", 8) == PM_OK && pm_session_tune(s, "chain_window", window) == PM_OK && pm_session_rows(s, 2) == PM_OK);
    std::vector<int64_t> starts((size_t)n, 0); const int32_t minsize = 16;
    pm_result* res = nullptr;
    if (pm_multi_mum_batch(s, 1, starts.data(), len.data(), &minsize, &res) != PM_OK) { CHECK(!"anchor call"); pm_session_destroy(s); return; }
    const int64_t table = pm_result_table_id(res), A = pm_result_total(res);
    CHECK(table != 0 && A == nm);
    std::vector<pm_row_info> info((size_t)A);
    CHECK(pm_store_settle(s, table, info.data()) == PM_OK);
    std::vector<int64_t> off((size_t)n + 1);
    const int64_t words = pm_store_layout_words(s, off.data());
    std::vector<uint64_t> before((size_t)words), after((size_t)words);
    CHECK(pm_store_layout(s, before.data(), words) == PM_OK);
    pm_chain_info ci; const int32_t* rows = nullptr; const uint8_t* heads = nullptr;
    // c = 110 where the cap is met: the LCB of the lead blocks (100 bases) would be dissolved where the run closes a chain
    CHECK(pm_store_chain_begin(s, nm, d, (float)D, expect_trouble ? 110 : 0) == PM_OK);
    if (pm_store_chain_end(s, &ci, &rows, &heads) != PM_OK) { CHECK(!"chain call"); pm_result_free(res); pm_session_destroy(s); return; }
    int64_t p1 = -1, p2 = -1;
    CHECK(pm_store_chain_passed(s, &p1, &p2) == PM_OK);
    CHECK(pm_store_layout(s, after.data(), words) == PM_OK);
    if (expect_trouble) {
        CHECK(ci.trouble == 8 && before == after);
    } else {
        CHECK(ci.trouble == 0 && ci.n_in == nm && ci.n_mums == nm && p1 == p && p2 == p);
        CHECK(ci.lcbs_first == (join ? 1 : 2) && ci.mums_dissolved == 0 && ci.n_lcbs == (join ? 1 : 2) && before == after);
        for (int64_t x = 0; x < ci.n_mums; x++) {
            const int want = x == 0 ? 1 : (x >= lead && x < lead + p) ? 2 : (!join && x == lead + p) ? 1 : 0;
            if (heads[x] != want) { printf("p %d: byte %d at %ld, not %d\n", p, heads[x], (long)x, want); fails++; break; }
        }
    }
    printf("run of %d ended by a %s, cap %ld: trouble %lu, %ld MUMs, %ld / %ld passed\n", p, join ? "join" : "close", (long)window, (unsigned long)ci.trouble, (long)ci.n_mums, (long)p1, (long)p2);
    pm_result_free(res);
    pm_session_destroy(s);
}

int main() {
    for (int p : {1, 2, 3, 63, 64, 65}) { list(100 + p, p, true, 2000, 4096, false); list(200 + p, p, false, 2000, 4096, false); }
    list(308, 8, true, 300, 8, false);
    list(309, 9, true, 300, 8, true);
    list(408, 8, false, 300, 8, false);
    list(409, 9, false, 300, 8, true);
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("chain_bp_check ok\n");
    return 0;
}
