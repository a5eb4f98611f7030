// gap_plan.h -- the host side of the device gap aligner that needs no device: the table of its five forms, the routing of a job
// to a form, the plan of one call (which jobs the device takes, in which order) and the geometry of one launch.  Plain C++17
// without a HIP include: gapalign_hip.hip includes it, tests/emu/gap_plan_check.cpp runs it on the CPU.
// Everything lies in an unnamed namespace: the file is part of the one translation unit that includes it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define GAP_PLAN_HD __host__ __device__
#else
#define GAP_PLAN_HD
#endif

namespace {

constexpr int kMaxSeqs = 512;      // sequences per alignment on the device: narrow and wide form
constexpr int kTallSeqs = 2048;    // ... and in the tall form (columns and bases: those of the wide form)
constexpr size_t kTallWorkspace = (size_t)8 << 30;      // bytes of slot workspace a tall launch may ask for (a slot of 2 048 sequences needs 20 MB)
constexpr int kMaxCols = 96;       // narrow form: bases of a sequence and columns of any intermediate alignment (LDS per wavefront ~25 KB: 6 alignments in flight per CU)
constexpr int kWideSeq = 320;      // wide form: bases of a sequence (every gap the default d = 300 of the reference's driver can produce) ...
constexpr int kWideCols = 640;     // ... and columns of any intermediate alignment (300-base strings align to about 1.65 times their length)
constexpr int kLongSeqs = 512, kLongSeq = 1024, kLongCols = 2048;      // the long form: one alignment = one workgroup ...
constexpr int kLongThreads = 256;                                      // ... of four wavefronts
constexpr size_t kLongWorkspace = (size_t)8 << 30;      // bytes of slot workspace a long launch may ask for (a slot of 512 x 2 048 needs 8 MB)
constexpr size_t kLongAccBytes = (size_t)6 * 4 * kLongCols;      // the six sums of a profile column, behind a long slot's trace-back bytes
constexpr int kLongTallSeqs = 2048;      // the long-tall form: the long form's bases and columns for as many sequences as the tall form
constexpr int kTable = 46656;      // 6^6 (fastdistnuc.cpp:82)
constexpr size_t kLdsLimit = 160 * 1024 - 1024;      // LDS a workgroup may ask for

struct Job { int64_t first_seq; int32_t n; int32_t max_cols; int64_t row_off; };

// ---- the forms.  A group's jobs lie form after form in the sorted job list, and every launch of a group has a queue counter of its
// own: one per form, and one for the second wide run of what the narrow form declined (kWideAgain)
enum Form { kNarrow, kWide, kTall, kLong, kLongTall, kForms };
constexpr int kCounters = 6, kWideAgain = 2;
struct FormRow {
    const char* name;       // as the `[gap batch]` line prints it
    int seqs, seq, cols;    // the limits: sequences of a job, bases of a sequence, columns of an alignment
    int threads;            // of a workgroup: one wavefront, or the long forms' four
    size_t fixed;           // bytes of the form's fixed block in LDS: sizeof of its Shared struct, device code -- gapalign_hip.hip asserts the number
    size_t ws_cap;          // bytes of slot workspace a launch may ask for (0: as many slots as the LDS allows)
    int counter;            // index of the queue counter among a group's kCounters
};
constexpr FormRow kFormTable[kForms] = {
    {"", kMaxSeqs, kMaxCols, kMaxCols, 64, 15040, 0, 0},
    {"wide", kMaxSeqs, kWideSeq, kWideCols, 64, 54480, 0, 1},
    {"tall", kTallSeqs, kWideSeq, kWideCols, 64, 72912, kTallWorkspace, 3},
    {"long", kLongSeqs, kLongSeq, kLongCols, kLongThreads, 146496, kLongWorkspace, 4},
    {"long-tall", kLongTallSeqs, kLongSeq, kLongCols, kLongThreads, 156736, kLongWorkspace, 5},
};

// n sequences, the widest of w bases: the smallest form that holds the job -- whichever entry point the job came through
constexpr Form route(int n, int w) { return n > kMaxSeqs ? (w > kWideSeq ? kLongTall : kTall) : (w > kWideSeq ? kLong : (w > kMaxCols ? kWide : kNarrow)); }

// What an entry point accepts: jobs of up to max_seqs sequences of up to max_seq_len bases -- the limits of the largest form it
// has.  narrow_only: pm_gap_align_batch / pm_gap_align_groups, the narrow form alone with the launch they have always had: slots
// sized by the jobs of the whole call, no second wide run of what the narrow form declined, one wait per group.
struct Rect { int max_seqs, max_seq_len; bool narrow_only; };
constexpr Rect rect_of(Form f) { return Rect{kFormTable[f].seqs, kFormTable[f].seq, f == kNarrow}; }

// ---- the plan of one call: the jobs the device takes, per group the narrow ones, then the wide, the tall, the long, the long-tall
// ones, each widest first (the cost of one alignment grows with the square of its width)
struct Plan {
    const char* error = nullptr;      // an argument the call refuses (then nothing else is filled in)
    std::vector<Job> jobs;            // in launch order
    std::vector<int64_t> which;       // jobs[i] is job which[i] of the call
    std::vector<size_t> first;        // form f of group g = jobs [first[kForms g + f], first[kForms g + f + 1])
    int nmax = 2, cap = 1;            // of the narrow form: the widest job of the call
    int64_t seqs = 0;                 // sequences of the call, declined jobs included
};
// (sets cols[j] = -1 for every job: a job that is not in the plan stays with the caller's host path)
inline Plan plan_jobs(const Rect& rect, int64_t n_jobs, const int32_t* n_seqs, const int64_t* seq_off, const uint8_t* chars, const int32_t* max_cols,
                      const int64_t* row_off, const uint8_t* out_rows, int64_t out_bytes, int32_t* cols, int n_groups, const int64_t* group_end) {
    Plan p;
    if (n_jobs < 0 || (n_jobs > 0 && (!n_seqs || !seq_off || !chars || !max_cols || !row_off || !out_rows || !cols))) { p.error = "bad argument"; return p; }
    if (n_groups < 1 || !group_end || group_end[n_groups - 1] != n_jobs) { p.error = "bad job groups"; return p; }
    for (int g = 0; g < n_groups; g++) if (group_end[g] < (g ? group_end[g - 1] : 0)) { p.error = "bad job groups"; return p; }
    std::vector<int> group_of, form_of, widest;
    int grp = 0;
    for (int64_t j = 0; j < n_jobs; j++) {
        while (grp + 1 < n_groups && j >= group_end[grp]) grp++;
        cols[j] = -1;
        const int n = n_seqs[j];
        int w = 0; bool ok = n >= 2 && n <= rect.max_seqs && max_cols[j] >= 1;
        for (int i = 0; i < n && ok; i++) { const int64_t L = seq_off[p.seqs + i + 1] - seq_off[p.seqs + i]; if (L <= 0 || L > rect.max_seq_len) ok = false; else w = std::max<int>(w, (int)L); }
        if (ok && row_off[j] + (int64_t)n * max_cols[j] > out_bytes) ok = false;
        if (ok) {
            const Form form = route(n, w);
            p.jobs.push_back(Job{p.seqs, n, max_cols[j], row_off[j]}); p.which.push_back(j); group_of.push_back(grp); form_of.push_back(form); widest.push_back(w);
            if (form == kNarrow) { p.nmax = std::max(p.nmax, n); p.cap = std::max(p.cap, std::min<int>(max_cols[j], kMaxCols)); }
        }
        p.seqs += n;
    }
    p.first.assign((size_t)n_groups * kForms + 1, 0);
    std::vector<size_t> order(p.jobs.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        if (group_of[a] != group_of[b]) return group_of[a] < group_of[b];
        if (form_of[a] != form_of[b]) return form_of[a] < form_of[b];
        return widest[a] > widest[b];
    });
    std::vector<Job> j2; std::vector<int64_t> w2;
    for (size_t i : order) { j2.push_back(p.jobs[i]); w2.push_back(p.which[i]); p.first[(size_t)group_of[i] * kForms + (size_t)form_of[i] + 1]++; }
    for (size_t k = 0; k < (size_t)n_groups * kForms; k++) p.first[k + 1] += p.first[k];
    p.jobs.swap(j2); p.which.swap(w2);
    return p;
}

// ---- a slot's workspace
// the trace-back bytes of one pairwise DP of up to cap x cap columns (nw_small)
GAP_PLAN_HD inline size_t tb_bytes(int cap) { return ((size_t)cap + 1) * ((size_t)cap + 1); }
// what carve() hands out.  seq: the form's limit on the bases of a sequence; rows / tb: the alignment rows and the trace-back bytes
// are in the workspace
inline size_t slot_bytes(int nmax, int cap, int seq, bool rows, bool tb) {
    const size_t n = (size_t)nmax;
    auto r = [](size_t b) { return (b + 15) & ~(size_t)15; };
    return r(4 * (n * (n - 1) / 2 + 1)) + r(2 * n * n) + r(2 * n * (size_t)seq) + r(n * (size_t)seq) + r(4 * n) + r(8 * n) + 4 * r(4 * n) + 3 * r(8 * n) + r(16 * n) +
           r(4 * n) + r(8 * n) + r(16 * n) + r(4 * n) + 2 * r(8 * n) + r(4 * n) + r(8 * n) + r(kTable) + (rows ? r(n * (size_t)cap) : 0) +
           (tb ? r(tb_bytes(cap)) : 0) + 256;
}

// ---- the geometry of one launch, from the jobs it is given.  Where things live:
//   narrow      the fixed block is static LDS, the rows (n x cap bytes) and the trace-back bytes (tb_bytes) dynamic LDS behind it; a
//               launch whose rows do not fit is refused (fits = false).  Sized once per call: wn x wc is the widest narrow job of
//               the CALL (Plan::nmax, cap), n_jobs the narrow jobs of its largest group (narrow_only: all jobs of the call)
//   wide, tall  the fixed block is dynamic LDS; the rows in LDS when they fit beside it, and the trace-back bytes too when both
//               fit; what does not fit lies in the slot's workspace, which one wavefront re-reads out of L2.  No job is declined
//               for its size in LDS.  place (PM_GAP_WIDE_PLACE, measurements): 1 the trace-back bytes, 2 the rows, 3 both in the
//               workspace whatever fits.  The tall form's rows never fit, and its slots are bounded by the workspace they need
//   long forms  a workgroup of four wavefronts per slot, one per CU (the fixed block takes most of the LDS); rows, trace-back bytes
//               and profile sums in the slot's workspace, which also bounds the slots (a slot of 2 048 x 2 048 needs 31 MB)
struct Geometry {
    int wn, wc;               // the widest job: sequences, columns (at most the form's)
    size_t lds, dyn;          // LDS of a workgroup, and the part of it that the launch asks for (narrow: all but the fixed block)
    bool rows_ws, tb_ws;      // the rows / the trace-back bytes are in the slot's workspace
    bool fits;
    int per_cu;
    int64_t slots;
    size_t stride;            // bytes of a slot's workspace
};
// the widest of a launch's jobs
inline void extent(Form form, const Job* jobs, size_t n_jobs, int* wn, int* wc) {
    *wn = 2; *wc = 1;
    for (size_t i = 0; i < n_jobs; i++) { *wn = std::max(*wn, jobs[i].n); *wc = std::max(*wc, std::min<int>(jobs[i].max_cols, kFormTable[form].cols)); }
}
inline Geometry size_launch(Form form, int wn, int wc, size_t n_jobs, int cu_count, int place) {
    const FormRow& row = kFormTable[form];
    auto r16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const bool is_long = row.threads > 64;
    const size_t fixed = r16(row.fixed), rows_b = r16((size_t)wn * (size_t)wc), tb_b = r16(tb_bytes(wc));
    Geometry g{};
    g.wn = wn; g.wc = wc; g.fits = true;
    if (is_long) g.rows_ws = g.tb_ws = true;
    else if (form == kNarrow) g.fits = fixed + rows_b + tb_b <= kLdsLimit;
    else {
        g.rows_ws = (place & 2) != 0; g.tb_ws = (place & 1) != 0;
        if (!g.rows_ws && fixed + rows_b > kLdsLimit) g.rows_ws = true;
        if (!g.tb_ws && fixed + (g.rows_ws ? 0 : rows_b) + tb_b > kLdsLimit) g.tb_ws = true;
    }
    g.lds = fixed + (g.rows_ws ? 0 : rows_b) + (g.tb_ws ? 0 : tb_b);
    g.dyn = form == kNarrow ? g.lds - fixed : g.lds;
    g.per_cu = is_long ? 1 : (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / (g.lds + 256)));
    g.stride = slot_bytes(wn, wc, row.seq, g.rows_ws, g.tb_ws) + (is_long ? kLongAccBytes : 0);
    g.slots = std::min<int64_t>((int64_t)n_jobs, (int64_t)cu_count * g.per_cu);
    if (row.ws_cap) g.slots = std::min<int64_t>(g.slots, std::max<int64_t>(1, (int64_t)(row.ws_cap / g.stride)));
    return g;
}

}  // namespace
