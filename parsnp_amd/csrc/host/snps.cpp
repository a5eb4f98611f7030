// snps.cpp -- [Output] snps=1: the core SNP columns of the XMFA being written and the pairwise SNP distances of its sequences.
//
// A multi-MUM is an exact match in every genome, so only the columns between the MUMs can vary.  The writer (output.cpp) hands
// those over block by block, in the order of the file; they lie side by side in a staging matrix of n rows that goes to the engine
// (pm_snp_add: include/parsnp_mum.h) whenever it is full -- kStageBytes of it at the most, whatever the size of the XMFA.  Every block
// leaves an entry (first column handed over, cluster, first column within the LCB, width) and its columns' reference positions;
// after the last add the indices of the core SNP columns, the rows' letters in them and the distances come back, and the
// indices are mapped through the entries.  Three files with the XMFA's stem:
//   <stem>.snps.mfa    per sequence ">name", its letters in the core SNP columns on one line
//   <stem>.snps.tsv    cluster, column within the LCB (0-based), reference position (as in the `> 1:a-b` header: a + the characters
//                      other than '-' of the reference row to the left of the column)
//   <stem>.snps.dist   the names, then per sequence its name and its row of distances, tab-separated
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "aligner.h"
#include "engine_step.h"
#include "hooks.h"

// Weak: a provider of the ABI without them (the CPU checker of the test builds) still links; snps=1 then ends the run.
extern "C" int pm_snp_limits(int* max_rows) __attribute__((weak));
extern "C" int pm_snp_begin(pm_session* s, int32_t n_rows) __attribute__((weak));
extern "C" int pm_snp_add(pm_session* s, int64_t n_cols, int64_t pitch, const uint8_t* chars, pm_snp_counts* totals) __attribute__((weak));
extern "C" int pm_snp_columns(pm_session* s, int64_t* col, uint8_t* letters) __attribute__((weak));
extern "C" int pm_snp_distances(pm_session* s, int32_t* dist) __attribute__((weak));

namespace parsnp {
SnpCounts snp_counts;

namespace {
constexpr size_t kStageBytes = (size_t)32 << 20;      // the staging matrix: 16 K columns of 2 000 rows
}  // namespace

int snp_max_rows() {
    int rows = 2048;
    if (pm_snp_limits) (void)pm_snp_limits(&rows);
    return rows;
}

SnpCollector::SnpCollector(pm_session* session, size_t n_rows, int threads) : session_(session), n_(n_rows), threads_(threads) {
    if (!pm_snp_begin || !pm_snp_add || !pm_snp_columns || !pm_snp_distances) {
        std::cerr << "parsnp_core: this provider of the engine's ABI cannot collect SNP columns (snps=1)" << std::endl;
        exit(1);
    }
    engine_check(pm_snp_begin(session_, (int32_t)n_rows), "cannot start the SNP collection");
    pitch_ = std::min<size_t>(std::max<size_t>(kStageBytes / n_, 1024), (size_t)1 << 20);
    if (const char* v = test_hook("PARSNP_SNP_STAGE_COLUMNS")) pitch_ = (size_t)std::max(1L, atol(v));      // test hook: a staging matrix of a few columns
    stage_.resize(n_ * pitch_);
}

uint8_t* SnpCollector::reserve(size_t width) {
    if (used_ + width > pitch_) flush();
    if (width > pitch_) { pitch_ = width; stage_.resize(n_ * pitch_); }      // (wider than the matrix: only after a flush, when it is empty)
    return stage_.data() + used_;
}

long SnpCollector::commit(int cluster, long c0, size_t width, const int64_t* ref_pos, int64_t ref_base) {
    entries_.push_back(Entry{total_, (int32_t)cluster, (int32_t)width, (int64_t)c0});
    long ref_chars = 0;
    const uint8_t* r0 = stage_.data() + used_;
    for (size_t c = 0; c < width; c++) {
        ref_pos_.push_back(ref_pos ? ref_pos[c] : ref_base + ref_chars);
        ref_chars += r0[c] != '-';
    }
    used_ += width; total_ += (int64_t)width;
    return ref_chars;
}

long SnpCollector::add_block(int cluster, long c0, size_t width, const std::function<void(size_t, uint8_t*)>& row, const int64_t* ref_pos, int64_t ref_base) {
    if (!width) return 0;
    uint8_t* at = reserve(width);
    const long nr = (long)n_;
#pragma omp parallel for schedule(static) num_threads(threads_) if (n_ * width >= 65536)
    for (long i = 0; i < nr; i++) row((size_t)i, at + (size_t)i * pitch_);
    return commit(cluster, c0, width, ref_pos, ref_base);
}

void SnpCollector::flush() {
    if (!used_) return;
    uint64_t h0 = 0, h1 = 0;
    (void)pm_session_traffic(session_, &h0, nullptr);
    engine_check(pm_snp_add(session_, (int64_t)used_, (int64_t)pitch_, stage_.data(), &counts_), "cannot classify the columns");
    (void)pm_session_traffic(session_, &h1, nullptr);
    h2d_bytes_ += (double)(h1 - h0);
    scan_ms_ += phase_ms(session_, "snp_", true);
    used_ = 0;
}

SnpCollector::Result SnpCollector::finish(const std::vector<Genome>& genomes, const std::string& dir, const std::string& stem, bool want_columns) {
    flush();
    const size_t v = (size_t)counts_.core_snps;
    std::vector<int64_t> col(v);
    std::vector<uint8_t> letters(n_ * v);
    Result res;
    std::vector<int32_t>& dist = res.dist;
    dist.resize(n_ * n_);
    for (size_t i = 0; i < n_; i++) res.names.push_back(genomes[i].fname);
    engine_check(pm_snp_columns(session_, col.data(), letters.data()), "cannot fetch the SNP columns");
    engine_check(pm_snp_distances(session_, dist.data()), "cannot compute the SNP distances");
    const double dist_ms = v ? phase_ms(session_, "snp_dist", false) : 0;
    {
        std::ofstream mfa((dir + stem + ".snps.mfa").c_str(), std::ios::binary);
        for (size_t i = 0; i < n_; i++) {
            mfa << '>' << genomes[i].fname << '\n';
            mfa.write((const char*)letters.data() + i * v, (std::streamsize)v);
            mfa << '\n';
        }
    }
    {
        std::ofstream tsv((dir + stem + ".snps.tsv").c_str(), std::ios::binary);
        tsv << "cluster\tcolumn\tref_pos\n";
        if (want_columns) res.columns.reserve(v);
        size_t e = 0;      // (col ascends: the entries are walked once)
        for (size_t k = 0; k < v; k++) {
            while (e + 1 < entries_.size() && entries_[e + 1].first <= col[k]) e++;
            const Entry& en = entries_[e];
            tsv << en.cluster << '\t' << en.c0 + (col[k] - en.first) << '\t' << ref_pos_[(size_t)col[k]] << '\n';
            if (want_columns) res.columns.push_back(RecColumn{en.cluster, en.c0 + (col[k] - en.first), ref_pos_[(size_t)col[k]]});
        }
    }
    {
        std::ofstream out((dir + stem + ".snps.dist").c_str(), std::ios::binary);
        std::string line;
        for (size_t i = 0; i < n_; i++) { line += '\t'; line += genomes[i].fname; }
        line += '\n';
        out << line;
        for (size_t i = 0; i < n_; i++) {
            line = genomes[i].fname;
            for (size_t j = 0; j < n_; j++) { line += '\t'; line += std::to_string(dist[i * n_ + j]); }
            line += '\n';
            out << line;
        }
    }
    snp_counts.on = true;
    snp_counts.columns = (long)counts_.columns + invariant_; snp_counts.invariant = (long)counts_.core_invariant + invariant_;
    snp_counts.core = (long)counts_.core_snps; snp_counts.other = (long)counts_.other;
    snp_counts.h2d_bytes = h2d_bytes_; snp_counts.scan_ms = scan_ms_; snp_counts.dist_ms = dist_ms;
    return res;
}

void SnpCollector::report() const {
    std::cerr << "SNP columns: " << snp_counts.columns << " columns, " << snp_counts.invariant << " core invariant, " << snp_counts.core << " core SNPs, "
              << snp_counts.other << " other" << std::endl;
}

}  // namespace parsnp
