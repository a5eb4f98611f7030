// unalign.cpp -- parsnp.unalign without the Aligner: the word-wise scan of one genome's layout bitmap for its runs of unmarked bits,
// and the records of the file from the runs of all genomes (write_unaligned, output.cpp, puts the two together).  Nothing here
// touches the engine or the rest of the host code: the suite's stand-alone checker links this file alone, under sanitizers.
#include <algorithm>
#include <ostream>
#include <string>

#include "aligner.h"

namespace parsnp {

UnalignCounts unalign_counts;

int64_t scan_unaligned_words(const uint64_t* w, int64_t nbits, std::vector<int32_t>* start, std::vector<int32_t>* end, std::vector<int32_t>* ordinal) {
    const int64_t nw = (nbits + 63) / 64;
    // unmarked valid bits of word i
    auto zword = [&](int64_t i) -> uint64_t { const int64_t left = nbits - i * 64; return ~w[i] & (left >= 64 ? ~0ull : ((1ull << left) - 1)); };
    int64_t runs = 0;
    uint64_t below = 0, z = nw ? zword(0) : 0;
    for (int64_t i = 0; i < nw; i++) {
        const uint64_t above = i + 1 < nw ? zword(i + 1) : 0;
        // a run starts at a bit whose lower neighbour is marked and ends at one whose upper neighbour is; both at once: a one-base run
        const uint64_t st = z & ~((z << 1) | (below >> 63)), en = z & ~((z >> 1) | (above << 63));
        for (uint64_t m = st & ~en; m; m &= m - 1) {
            const int bit = __builtin_ctzll(m);
            start->push_back((int32_t)(i * 64 + bit));
            ordinal->push_back((int32_t)(runs + __builtin_popcountll(st & ((1ull << bit) - 1))));
        }
        for (uint64_t m = en & ~st; m; m &= m - 1) end->push_back((int32_t)(i * 64 + __builtin_ctzll(m)));      // (kept ends pair with kept starts by rank)
        runs += __builtin_popcountll(st);
        below = z; z = above;
    }
    return runs;
}

void append_unaligned_record(std::string& rec, size_t k, long startpos, long endpos, const Genome& gn) {
    using namespace std;
    rec += ">" + to_string(k + 1) + ":" + to_string(startpos) + "-" + to_string(endpos) + " + " + gn.fname + "\n";
    const string& g = gn.seq;
    const size_t len = (size_t)(endpos - startpos);
    const size_t from = (size_t)startpos;
    const size_t avail = from <= g.size() ? min(len, g.size() - from) : 0;
    size_t pos = 0;
    while (pos + 80 < avail) { rec.append(g, from + pos, 80); rec.push_back('\n'); pos += 80; }
    if (pos + 1 < avail) { rec.append(g, from + pos, avail - pos); rec.push_back('\n'); }
    if (avail == 0) rec += "-\n";
    rec += "=\n";
}

void write_unaligned_records(const UnalignRuns& R, const std::vector<Genome>& genomes, int threads, std::ostream& out) {
    using namespace std;
    const size_t n = genomes.size();
    if (n == 0) return;
    const int64_t rounds = R.all[n - 1] + 1;      // rounds 0 .. runs[n - 1]
    // the records in the order of (round, genome): counted per round, then placed genome after genome (a genome's ordinals rise)
    vector<int64_t> at((size_t)rounds + 1, 0);
    for (size_t k = 0; k < n; k++)
        for (int64_t i = R.first[k]; i < R.first[k + 1] && R.ordinal[(size_t)i] < rounds; i++) at[(size_t)R.ordinal[(size_t)i] + 1]++;
    for (int64_t r = 0; r < rounds; r++) at[(size_t)r + 1] += at[(size_t)r];
    const size_t total = (size_t)at[(size_t)rounds];
    vector<int64_t> run(total); vector<int32_t> genome(total);
    for (size_t k = 0; k < n; k++)
        for (int64_t i = R.first[k]; i < R.first[k + 1] && R.ordinal[(size_t)i] < rounds; i++) {
            const size_t slot = (size_t)at[(size_t)R.ordinal[(size_t)i]]++;
            run[slot] = i; genome[slot] = (int32_t)k;
        }
    // formatted in chunks of the list, a few chunks per thread at a time, written in order
    const size_t kChunk = 1024;
    const size_t chunks = (total + kChunk - 1) / kChunk;
    if (threads < 1) threads = 1;
    const size_t wave = (size_t)threads * 4;
    vector<string> text(min(wave, max<size_t>(chunks, 1)));
    for (size_t c0 = 0; c0 < chunks; c0 += wave) {
        const long m = (long)min(wave, chunks - c0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
        for (long c = 0; c < m; c++) {
            string& rec = text[(size_t)c];
            rec.clear();
            const size_t a = (c0 + (size_t)c) * kChunk, b = min(total, a + kChunk);
            for (size_t x = a; x < b; x++) append_unaligned_record(rec, (size_t)genome[x], (long)R.start[(size_t)run[x]], (long)R.end[(size_t)run[x]], genomes[(size_t)genome[x]]);
        }
        for (long c = 0; c < m; c++) out.write(text[(size_t)c].data(), (streamsize)text[(size_t)c].size());
    }
}

}  // namespace parsnp
