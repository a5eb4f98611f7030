// tests/emu/gap_plan_check.cpp -- TEST INFRASTRUCTURE ONLY.
// The host side of the device gap aligner that needs no device (parsnp_amd/csrc/engine/gap_plan.h: the form table, plan_jobs,
// size_launch) behind a main(), so that tests/test_gap_plan.py can compare plans and geometries with its restatement -- the
// program built with AddressSanitizer and UBSan.  Lengths are all a plan needs: the bases are one buffer of 'A'.
//
//   gap_plan_check <in>      one JSON object per command of <in> on stdout
//   table
//   plan   <max_seqs> <max_seq_len> <narrow_only> <out_bytes> <n_groups> <group_end ...> <n_jobs>, then per job:
//          <n> <max_cols> <row_off> <n lengths>
//   size   <form> <n_jobs> <cu_count> <place> <n_given>, then per given job: <n> <max_cols>     (extent, then size_launch)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "../../parsnp_amd/csrc/engine/gap_plan.h"

static long long rd(FILE* f) { long long v = 0; if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: gap_plan_check <in>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        const std::string c = cmd;
        if (c == "table") {
            printf("{\"forms\": [");
            for (int k = 0; k < kForms; k++) {
                const FormRow& r = kFormTable[k];
                printf("%s{\"name\": \"%s\", \"seqs\": %d, \"seq\": %d, \"cols\": %d, \"threads\": %d, \"fixed\": %zu, \"ws_cap\": %zu, \"counter\": %d}", k ? ", " : "", r.name, r.seqs, r.seq, r.cols,
                       r.threads, r.fixed, r.ws_cap, r.counter);
            }
            printf("], \"counters\": %d, \"wide_again\": %d, \"lds_limit\": %zu, \"long_acc\": %zu}\n", kCounters, kWideAgain, kLdsLimit, kLongAccBytes);
        } else if (c == "plan") {
            Rect rect{(int)rd(f), (int)rd(f), rd(f) != 0};
            const int64_t out_bytes = rd(f);
            const int n_groups = (int)rd(f);
            std::vector<int64_t> group_end((size_t)n_groups);
            for (auto& g : group_end) g = rd(f);
            const int64_t nj = rd(f);
            std::vector<int32_t> n_seqs, max_cols, cols((size_t)nj, -7);
            std::vector<int64_t> row_off, seq_off(1, 0);
            for (int64_t j = 0; j < nj; j++) {
                n_seqs.push_back((int32_t)rd(f)); max_cols.push_back((int32_t)rd(f)); row_off.push_back(rd(f));
                for (int i = 0; i < n_seqs.back(); i++) seq_off.push_back(seq_off.back() + rd(f));
            }
            // exactly as many bytes as the offsets name: a read of a base, or past the last offset, is a finding
            std::unique_ptr<uint8_t[]> chars(new uint8_t[(size_t)seq_off.back() + 1]), out(new uint8_t[1]);
            const Plan p = plan_jobs(rect, nj, n_seqs.data(), seq_off.data(), chars.get(), max_cols.data(), row_off.data(), out.get(), out_bytes, cols.data(), n_groups, group_end.data());
            if (p.error) { printf("{\"error\": \"%s\"}\n", p.error); continue; }
            printf("{\"error\": null, \"nmax\": %d, \"cap\": %d, \"seqs\": %lld, \"jobs\": [", p.nmax, p.cap, (long long)p.seqs);
            for (size_t i = 0; i < p.jobs.size(); i++) printf("%s[%lld, %d, %d, %lld]", i ? ", " : "", (long long)p.jobs[i].first_seq, p.jobs[i].n, p.jobs[i].max_cols, (long long)p.jobs[i].row_off);
            printf("], \"which\": [");
            for (size_t i = 0; i < p.which.size(); i++) printf("%s%lld", i ? ", " : "", (long long)p.which[i]);
            printf("], \"first\": [");
            for (size_t i = 0; i < p.first.size(); i++) printf("%s%zu", i ? ", " : "", p.first[i]);
            printf("], \"cols\": [");
            for (size_t i = 0; i < cols.size(); i++) printf("%s%d", i ? ", " : "", cols[i]);
            printf("]}\n");
        } else if (c == "size") {
            const Form form = (Form)rd(f);
            const size_t n_jobs = (size_t)rd(f);
            const int cu = (int)rd(f), place = (int)rd(f);
            std::vector<Job> given((size_t)rd(f));
            for (Job& j : given) { j = Job{0, (int32_t)rd(f), 0, 0}; j.max_cols = (int32_t)rd(f); }
            int wn, wc;
            extent(form, given.data(), given.size(), &wn, &wc);
            const Geometry g = size_launch(form, wn, wc, n_jobs, cu, place);
            printf("{\"wn\": %d, \"wc\": %d, \"lds\": %zu, \"dyn\": %zu, \"rows_ws\": %d, \"tb_ws\": %d, \"fits\": %d, \"per_cu\": %d, \"slots\": %lld, \"stride\": %zu}\n", g.wn, g.wc, g.lds, g.dyn,
                   (int)g.rows_ws, (int)g.tb_ws, (int)g.fits, g.per_cu, (long long)g.slots, g.stride);
        } else { fprintf(stderr, "unknown command %s\n", cmd); return 2; }
    }
    fclose(f);
    return 0;
}
