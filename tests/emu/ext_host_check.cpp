// ext_host_check.cpp -- the host side of the LCB extension that needs no device (csrc/host/extend.cpp: the covered stretches from the
// records' intervals, the flank of every row with its halving and its stop at a letter that is none of ACGT, the descriptors, the text
// of a job's records, the header lines) as a program of its own, built under AddressSanitizer + UBSan by tests/test_lcb_ext_host.py.
// Never loaded into Python.
//
//   ext_host_check IN.txt      IN.txt: "n F printable", then n lines "fname header size_nopad sequence", then "L" and per LCB a line
//                              "cluster rows" followed by `rows` lines "seq lo hi fwd"
//   prints the header lines, the covered stretches, then per job its descriptors and the record text for used[r] = min(len, 3 + 5 r)
//   and letters that spell the row number
#include "../../parsnp_amd/csrc/host/extend.cpp"

// what extend.cpp's device path refers to: this program never takes it
extern "C" const char* pm_last_error(void) { return ""; }
extern "C" int pm_last_timing(const pm_session*, int* count, const char**, float*) { *count = 0; return 0; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    int n = 0, F = 0, printable = 0;
    if (!f || fscanf(f, "%d %d %d", &n, &F, &printable) != 3) return 1;
    std::vector<parsnp::Genome> genomes((size_t)n);
    std::vector<int64_t> lens;
    std::vector<char> buf(1 << 20);
    for (int g = 0; g < n; g++) {
        char name[256], header[256];
        if (fscanf(f, "%255s %255s %d %1048575s", name, header, &genomes[(size_t)g].size_nopad, buf.data()) != 4) return 1;
        genomes[(size_t)g].fname = name; genomes[(size_t)g].header = header; genomes[(size_t)g].seq = buf.data();
        if (genomes[(size_t)g].seq == ".") genomes[(size_t)g].seq.clear();
        lens.push_back((int64_t)genomes[(size_t)g].seq.size());
    }
    int L = 0;
    if (fscanf(f, "%d", &L) != 1) return 1;
    std::vector<std::vector<parsnp::ExtRecord>> lcbs((size_t)L);
    for (int z = 0; z < L; z++) {
        int cluster = 0, rows = 0;
        if (fscanf(f, "%d %d", &cluster, &rows) != 2) return 1;
        for (int r = 0; r < rows; r++) {
            int seq = 0, fwd = 0; long long lo = 0, hi = 0;
            if (fscanf(f, "%d %lld %lld %d", &seq, &lo, &hi, &fwd) != 4) return 1;
            lcbs[(size_t)z].push_back(parsnp::ExtRecord{seq, lo, hi, fwd != 0, cluster});
        }
    }
    fclose(f);
    printf("%s", parsnp::ext_header_text(genomes, printable).c_str());
    const parsnp::ExtCovered cov = parsnp::ext_covered(lcbs, lens);
    for (size_t g = 0; g < cov.size(); g++) {
        printf("covered %zu", g + 1);
        for (const auto& s : cov[g]) printf(" %lld-%lld", (long long)s.first, (long long)s.second);
        printf("\n");
    }
    for (size_t z = 0; z < lcbs.size(); z++)
        for (char side : {'L', 'R'}) {
            std::vector<pm_ext_row> rows;
            std::vector<int32_t> used;
            for (const parsnp::ExtRecord& r : lcbs[z]) rows.push_back(parsnp::ext_flank(genomes[(size_t)r.seq - 1].seq, cov[(size_t)r.seq - 1], r, side, F));
            printf("job %d %c", lcbs[z][0].cluster, side);
            for (const pm_ext_row& r : rows) printf(" (%d %d %d %d %lld)", r.genome, r.step, r.complement, r.len, (long long)r.first);
            printf("\n");
            const int32_t cols = 163;
            const int64_t pitch = 2 * (int64_t)F > cols ? 2 * (int64_t)F : cols;
            std::vector<uint8_t> letters(rows.size() * (size_t)pitch, '-');
            for (size_t r = 0; r < rows.size(); r++) {
                used.push_back(std::min<int32_t>(rows[r].len, 3 + 5 * (int32_t)r));
                for (int32_t k = 0; k < cols; k++) letters[r * (size_t)pitch + (size_t)k] = (uint8_t)"ACGT"[(k + (int32_t)r) % 4];
            }
            printf("%s", parsnp::ext_job_text(lcbs[z], rows.data(), used.data(), letters.data(), pitch, cols, side).c_str());
        }
    return 0;
}
