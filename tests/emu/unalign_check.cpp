// tests/emu/unalign_check.cpp -- TEST INFRASTRUCTURE ONLY.
// The host side of parsnp.unalign on its own: parsnp_amd/csrc/host/unalign.cpp (the word-wise scan of a layout bitmap and the
// formatter of the records) behind a main() that reads layouts from a file, so that tests/test_unalign_host.py can run the two under
// AddressSanitizer and UBSan on the generator's sets and compare the file with the restatement's.
//
//   unalign_check <in> <out> <threads>
//   <in>:  int64 n, then per genome: int64 name bytes, name, int64 sequence bytes, sequence, int64 nbits, (nbits + 63) / 64 words
//          (exactly that many: a read past the last word of a bitmap is a finding)
//   <out>: the records; stdout: per genome "all kept"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>

#include "../../parsnp_amd/csrc/host/aligner.h"

using namespace parsnp;

static int64_t rd64(FILE* f) { int64_t v = 0; if (fread(&v, 8, 1, f) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static std::string rdstr(FILE* f) { std::string s((size_t)rd64(f), '\0'); if (!s.empty() && fread(&s[0], 1, s.size(), f) != s.size()) { fprintf(stderr, "short input\n"); exit(2); } return s; }

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: unalign_check <in> <out> <threads>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const size_t n = (size_t)rd64(f);
    std::vector<Genome> genomes(n);
    UnalignRuns R;
    R.all.assign(n, 0); R.kept.assign(n, 0); R.first.assign(n + 1, 0);
    for (size_t k = 0; k < n; k++) {
        genomes[k].fname = rdstr(f);
        genomes[k].seq = rdstr(f);
        const int64_t nbits = rd64(f);
        const size_t nw = (size_t)((nbits + 63) / 64);
        std::unique_ptr<uint64_t[]> w(new uint64_t[nw ? nw : 1]);      // (its own block of exactly nw words: the sanitizer sees a word too many)
        if (nw && fread(w.get(), 8, nw, f) != nw) { fprintf(stderr, "short input\n"); return 2; }
        R.all[k] = scan_unaligned_words(w.get(), nbits, &R.start, &R.end, &R.ordinal);
        if (R.start.size() != R.end.size() || R.start.size() != R.ordinal.size()) { fprintf(stderr, "genome %zu: kept starts and kept ends do not pair\n", k); return 1; }
        R.first[k + 1] = (int64_t)R.start.size();
        R.kept[k] = R.first[k + 1] - R.first[k];
        printf("%lld %lld\n", (long long)R.all[k], (long long)R.kept[k]);
    }
    fclose(f);
    std::ofstream out(argv[2], std::ios::binary);
    write_unaligned_records(R, genomes, atoi(argv[3]), out);
    out.close();
    return out ? 0 : 1;
}
