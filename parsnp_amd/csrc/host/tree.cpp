// tree.cpp -- [Output] tree=1: the neighbour-joining tree of the SNP distances, <stem>.snps.nwk beside the three SNP files.
//
// The engine joins (pm_nj_tree: include/parsnp_mum.h) over the distance matrix the session computed a moment ago, which is still on
// the device; what comes back are the n - 3 join records (i, j, D[i][j], R[i], R[j] before the update) and the record of the last
// three slots.  The host derives the branch lengths from them -- the device never divides -- and writes one line of Newick, by the
// definition of INTEGRATION.md 1b:
//   a join of r active slots   Li = 0.5 * dij + (ri - rj) / (2 * (r - 2)),  Lj = dij - Li
//   the last three             La = ((dab + dac) - dbc) * 0.5,  Lb = ((dab + dbc) - dac) * 0.5,  Lc = ((dac + dbc) - dab) * 0.5
// Every operation is an IEEE double operation rounded once, in the order written.  The host writer is compiled for plain x86-64
// with AVX2 and WITHOUT FMA (no -mfma, no -march=native: csrc/Makefile), so the compiler has no fused instruction to contract these
// into; each result additionally passes through `once`, an empty asm statement the optimiser cannot see through.
// Lengths are not clamped (a negative one is printed as it is); the unit is core SNP columns.
//
// [Output] bootstrap=B: after the main tree the engine draws B replicates of the core SNP columns, computes their
// weighted distances (pm_boot_distances), joins the B replicate trees in lock step (pm_nj_trees) and counts, for every join of the
// main tree, the replicate trees that hold its split (pm_nj_support).  Nothing but the n - 3 counts comes back.  <stem>.snps.boot.nwk
// is the same Newick text with the count of join t behind the closing bracket of its node; <stem>.snps.nwk keeps its bytes.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "aligner.h"
#include "engine_step.h"

// Weak, like the pm_snp_* calls: a provider of the ABI without them still links; tree=1 then ends the run.
extern "C" int pm_nj_limits(int* max_rows) __attribute__((weak));
extern "C" int pm_nj_tree(pm_session* s, int32_t n, const int32_t* dist, pm_nj_join* joins, pm_nj_last* last) __attribute__((weak));
extern "C" int pm_boot_limits(int* max_rows, int* max_reps, int* max_weight) __attribute__((weak));
extern "C" int pm_boot_distances(pm_session* s, int32_t reps, uint64_t seed, const uint8_t* weights, int64_t pitch, uint8_t* weights_out, int32_t* dist_out) __attribute__((weak));
extern "C" int pm_nj_trees(pm_session* s, int32_t n, int32_t count, const int32_t* dist, pm_nj_join* joins, pm_nj_last* last) __attribute__((weak));
extern "C" int pm_nj_support(pm_session* s, int32_t n, const pm_nj_join* main_joins, int32_t count, const pm_nj_join* rep_joins, int32_t* support) __attribute__((weak));

namespace parsnp {
TreeCounts tree_counts;

namespace {
inline double once(double v) {
#if defined(__x86_64__)
    asm volatile("" : "+x"(v));
#else
    asm volatile("" : "+m"(v));
#endif
    return v;
}
// %.10g; a value equal to zero (either sign) is `0`
void put_length(std::string& out, double v) {
    if (v == 0) { out += '0'; return; }
    char buf[48];
    snprintf(buf, sizeof buf, "%.10g", v);
    out += buf;
}
// bare when it matches [A-Za-z0-9_.-]+, in single quotes with a quote inside doubled otherwise
std::string newick_name(const std::string& name) {
    bool bare = !name.empty();
    for (const char c : name)
        if (!((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_' || c == '.' || c == '-')) bare = false;
    if (bare) return name;
    std::string q = "'";
    for (const char c : name) { q += c; if (c == '\'') q += '\''; }
    return q + "'";
}
}  // namespace

int tree_max_rows() {
    int rows = 2048;
    if (pm_nj_limits) (void)pm_nj_limits(&rows);
    return rows;
}

int boot_max_reps() {
    int reps = 1024;
    if (pm_boot_limits) (void)pm_boot_limits(nullptr, &reps, nullptr);
    return reps;
}

// Every slot holds the text of its subtree; a join replaces slot i's by the new node's.  No recursion: a caterpillar of 2 046 joins
// is 2 046 passes of this loop.
std::string nj_newick(const std::vector<std::string>& names, const pm_nj_join* joins, const pm_nj_last& last, const int32_t* support) {
    const size_t n = names.size();
    std::vector<std::string> slot(n);
    for (size_t i = 0; i < n; i++) slot[i] = newick_name(names[i]);
    for (size_t t = 0; t + 3 < n; t++) {
        const pm_nj_join& J = joins[t];
        const double r = (double)(n - t);
        const double half = once(0.5 * J.dij), diff = once(J.ri - J.rj), den = 2.0 * (r - 2.0);      // (den: a small integer, exact)
        const double li = once(half + once(diff / den)), lj = once(J.dij - li);
        std::string node = "(";
        node += slot[(size_t)J.i]; node += ':'; put_length(node, li); node += ',';
        node += slot[(size_t)J.j]; node += ':'; put_length(node, lj); node += ')';
        if (support) node += std::to_string(support[t]);
        slot[(size_t)J.i].swap(node);
        std::string().swap(slot[(size_t)J.j]);
    }
    const double la = once(once(once(last.dab + last.dac) - last.dbc) * 0.5);
    const double lb = once(once(once(last.dab + last.dbc) - last.dac) * 0.5);
    const double lc = once(once(once(last.dac + last.dbc) - last.dab) * 0.5);
    std::string out = "(";
    out += slot[(size_t)last.a]; out += ':'; put_length(out, la); out += ',';
    out += slot[(size_t)last.b]; out += ':'; put_length(out, lb); out += ',';
    out += slot[(size_t)last.c]; out += ':'; put_length(out, lc); out += ");";
    return out;
}

void write_tree(pm_session* session, const std::vector<std::string>& names, const int32_t* dist, const std::string& dir, const std::string& stem,
                int bootstrap, uint64_t bootseed) {
    const size_t n = names.size();
    std::string text, boot_text;
    long boot_reps = 0;
    double boot_ms = 0;
    long joins_made = 0;
    double ms = 0;
    if (n == 2) {      // no device call: the one distance, halved
        const double h = once(0.5 * (double)dist[1]);
        text = "(" + newick_name(names[0]) + ":";
        put_length(text, h);
        text += "," + newick_name(names[1]) + ":";
        put_length(text, h);
        text += ");";
    } else {
        if (!pm_nj_tree) {
            std::cerr << "parsnp_core: this provider of the engine's ABI cannot build a tree (tree=1)" << std::endl;
            exit(1);
        }
        std::vector<pm_nj_join> joins(n - 3 ? n - 3 : 1);
        pm_nj_last last;
        memset(&last, 0, sizeof last);
        engine_check(pm_nj_tree(session, (int32_t)n, nullptr, joins.data(), &last), "cannot build the neighbour-joining tree");
        ms = phase_ms(session, "nj", false);
        joins_made = (long)n - 3;
        text = nj_newick(names, joins.data(), last);
        if (bootstrap > 0 && n > 3) {      // (three leaves have no internal branch: no label, no call)
            if (!pm_boot_distances || !pm_nj_trees || !pm_nj_support) {
                std::cerr << "parsnp_core: this provider of the engine's ABI cannot bootstrap a tree (bootstrap=" << bootstrap << ")" << std::endl;
                exit(1);
            }
            std::vector<int32_t> support(n - 3);
            auto step = [&](int rc, const char* what) {
                engine_check(rc, std::string("cannot bootstrap the tree (") + what + ")");
                boot_ms += phase_ms(session, "boot_", true);
            };
            step(pm_boot_distances(session, bootstrap, bootseed, nullptr, 0, nullptr, nullptr), "distances");
            step(pm_nj_trees(session, (int32_t)n, bootstrap, nullptr, nullptr, nullptr), "trees");
            step(pm_nj_support(session, (int32_t)n, joins.data(), bootstrap, nullptr, support.data()), "support");
            boot_reps = bootstrap;
            boot_text = nj_newick(names, joins.data(), last, support.data());
        }
    }
    text += '\n';
    std::ofstream out((dir + stem + ".snps.nwk").c_str(), std::ios::binary);
    out << text;
    tree_counts.on = true; tree_counts.nj_ms = ms; tree_counts.joins = joins_made;
    std::cerr << "Neighbour-joining tree: " << n << " leaves, " << joins_made << " joins on the device" << std::endl;
    if (bootstrap > 0) {
        std::ofstream bout((dir + stem + ".snps.boot.nwk").c_str(), std::ios::binary);
        bout << (boot_reps ? boot_text + '\n' : text);
        tree_counts.boot_on = true; tree_counts.boot_reps = boot_reps; tree_counts.boot_ms = boot_ms;
        if (boot_reps) std::cerr << "Bootstrap: " << boot_reps << " replicates of " << n << " leaves on the device" << std::endl;
    }
}

}  // namespace parsnp
