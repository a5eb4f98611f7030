// rec_host_check.cpp -- the host side of the recombination scan that needs no device (csrc/host/recomb.cpp: the windows over the
// LCBs' site lists, the text of the two files) as a program of its own, built under AddressSanitizer + UBSan by
// tests/test_rec_host.py.  Never loaded into Python.
//
//   rec_host_check IN.txt      IN.txt: "V K perms", then V lines "cluster column ref_pos informative"
//   prints the sites and window offsets, then .rec.tsv and .rec for phi[g] = 3 g + 1 and le[g] = 7 g mod 11 mod (perms + 1)
#include "../../parsnp_amd/csrc/host/recomb.cpp"

// what recomb.cpp's device path refers to: this program never takes it
extern "C" const char* pm_last_error(void) { return ""; }
extern "C" int pm_last_timing(const pm_session*, int* count, const char**, float*) { *count = 0; return 0; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    long V = 0, K = 0, perms = 0;
    if (!f || fscanf(f, "%ld %ld %ld", &V, &K, &perms) != 3) return 1;
    std::vector<parsnp::RecColumn> cols((size_t)V);
    std::vector<uint8_t> informative((size_t)V);
    for (long c = 0; c < V; c++) {
        int cluster = 0, inf = 0; long long column = 0, ref = 0;
        if (fscanf(f, "%d %lld %lld %d", &cluster, &column, &ref, &inf) != 4) return 1;
        cols[(size_t)c] = parsnp::RecColumn{cluster, column, ref};
        informative[(size_t)c] = (uint8_t)inf;
    }
    fclose(f);
    std::vector<int64_t> sites, win_off;
    const std::vector<parsnp::RecWindow> win = parsnp::rec_windows(cols, informative.data(), (size_t)K, &sites, &win_off);
    printf("sites");
    for (int64_t s : sites) printf(" %lld", (long long)s);
    printf("\noffsets");
    for (int64_t o : win_off) printf(" %lld", (long long)o);
    printf("\n");
    std::vector<int32_t> phi(win.size()), le(win.size());
    for (size_t g = 0; g < win.size(); g++) { phi[g] = (int32_t)(3 * g + 1); le[g] = (int32_t)((7 * g) % 11 % (size_t)(perms + 1)); }
    long flagged = -1;
    const std::string bed = parsnp::rec_bed_text(win, le.data(), (int32_t)perms, &flagged);
    printf("%s----\n%s----\n%ld\n", parsnp::rec_tsv_text(win, phi.data(), le.data(), (int32_t)perms).c_str(), bed.c_str(), flagged);
    return 0;
}
