// output.cpp -- parsnpAligner.xmfa + parsnpAligner.log, the output contract of the reference's
// Aligner::writeOutput (src/parsnp.cpp:505-1191).  MUM columns are lower case, inter-MUM gap columns upper case.
// Gaps in which every genome has >= 1 base and some genome has >= 2 go to libMUSCLE in the reference
// (:790-865, src/MuscleInterface.cpp:37-78); here they go to the device gap aligner (include/parsnp_mum.h: strings of up to 320
// bases in alignments of up to 2 048 sequences, of up to 1 024 bases -- a cluster distance d of up to 1 000 -- in alignments of
// up to 512) and, beyond its limits, to gapalign.cpp, the restatement of that aligner.  Should it ever decline an input, the gap is
// emitted left-justified and '-'-padded and the log carries a note.  write_output(), at the end, lists the stages: XmfaWriter's members.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <fstream>
#include <future>
#include <iomanip>
#include <iostream>
#include <sys/mman.h>
#include <unistd.h>

#include "aligner.h"
#include "hooks.h"
#include "gapalign.h"

// The device gap aligner with all its forms behind one entry point (include/parsnp_mum.h).  Weak: a provider of the ABI without it
// (the CPU providers of the test builds) still links, and the writer then uses pm_gap_align_groups with its narrow limits.  An
// engine library with some of the forms but not all of them is not provided for: libparsnp_hip.so and parsnp_core are built
// from one tree.
extern "C" int pm_gap_align_groups_long_tall(int device, int64_t n_jobs, const int32_t* n_seqs, const int64_t* seq_off, const uint8_t* chars,
                                             const int32_t* max_cols, const int64_t* row_off, uint8_t* out_rows, int64_t out_bytes, int32_t* cols,
                                             int n_groups, const int64_t* group_end, void (*done)(void* ctx, int group), void* ctx, pm_gap_long_tall_stats* stats) __attribute__((weak));
extern "C" int pm_gap_limits_long_tall(int* max_seqs, int* max_seq_len, int* max_cols) __attribute__((weak));

namespace parsnp {
GapCounts gap_counts;

namespace {
std::string upper(std::string s) { std::transform(s.begin(), s.end(), s.begin(), ::toupper); return s; }
std::string sub(const std::string& g, long pos, long len) {   // std::string::substr semantics incl. size_t wrap of len
    if (pos < 0 || (size_t)pos > g.size()) { std::cerr << "parsnp_core: substr out of range" << std::endl; exit(1); }
    return g.substr((size_t)pos, (size_t)len);
}
double clock_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// A base as the records print it: upper case in a gap column, lower case in a MUM column, and the complement of either for a row
// on the reverse strand (= upper / lower of reverse_complement(), ingest.cpp / parsnp.cpp:1294-1393: anything but a c g t u gives n,
// and the characters reversec drops, parsnp.cpp:1369-1380, give 0)
const struct CaseTable { char up[256], low[256], rc_up[256], rc_low[256]; CaseTable() {
    for (int c = 0; c < 256; c++) {
        up[c] = (char)toupper(c); low[c] = (char)tolower(c);
        switch (toupper(c)) {
            case 'A': rc_up[c] = 'T'; break; case 'C': rc_up[c] = 'G'; break; case 'G': rc_up[c] = 'C'; break;
            case 'T': rc_up[c] = 'A'; break; case 'U': rc_up[c] = 'T'; break;
            case '\r': case '\n': case '\t': case ' ': case '>': case '.': rc_up[c] = 0; break;
            default: rc_up[c] = 'N'; break;
        }
        rc_low[c] = (char)tolower((unsigned char)rc_up[c]);
    }
} } kCase;

// ---- the rules that more than one stage applies
// reference: MUSCLE(maxiters=1) over the n gap strings (:848-861); a single genome is never aligned (:809-826)
bool gap_is_aligned(long longest, long shortest, size_t n) { return longest > 1 && shortest > 0 && n > 1; }
// columns of an LCB's rows: its MUMs and, between MUM t and MUM t+1, gap_width(t)
template <class Width> long long lcb_columns(const Aligner& a, const Lcb& ct, Width gap_width) {
    long long cols = 0;
    for (size_t t = 0; t < ct.mums.size(); t++) {
        cols += a.pool[(size_t)ct.mums[t]].length;
        if (t + 1 < ct.mums.size()) cols += gap_width(t);
    }
    return cols;
}
// the a-b of `> i:a-b` for row i of a printed LCB (ct: after the overlap trim); a reverse row runs from its last MUM to its first (:980-1049)
struct Interval { long lo, hi; bool fwd; };
Interval printed_interval(const Aligner& a, const Lcb& ct, size_t i) {
    const Mum& first = a.pool[(size_t)ct.mums.front()];
    if (first.fwd[i]) return Interval{(long)ct.start[i] + 1, (long)ct.end[i], true};
    return Interval{(long)a.pool[(size_t)ct.mums.back()].start[i] + 1, first.end(i), false};
}

// ---- the string route.  Rows of one LCB: MUMs interleaved with the gaps between consecutive MUMs (:663-916): gap_between() per gap,
// gap_align() by the caller for those the reference would hand to MUSCLE (the others are padded on the fly), build_rows() concatenates.
// It reproduces the reference's substr clamping and wrap, which the integer route (XmfaWriter::gap_length) only flags.
struct Gap {
    std::vector<std::string> seq;       // per genome
    std::vector<std::string> aligned;   // filled when `align`
    unsigned max_len = 0;
    bool align = false, failed = false;
};

// the gap between MUM t and MUM t+1 of an LCB (gp is reused by the caller: no allocation in the common one-column case)
void gap_between(const Aligner& a, const Lcb& ct, size_t t, Gap* gp) {
    const size_t n = a.n;
    const Mum& first = a.pool[(size_t)ct.mums[0]];
    const Mum& m = a.pool[(size_t)ct.mums[t]];
    const Mum& nx = a.pool[(size_t)ct.mums[t + 1]];
    gp->seq.resize(n);
    unsigned max_len = 0, min_len = 1000000;
    for (size_t i = 0; i < n; i++) {
        const std::string& g = a.genomes[i].seq;
        if (!first.fwd[i]) {
            if (m.start[i] - nx.end(i) >= 1) gp->seq[i] = upper(reverse_complement(sub(g, nx.end(i), m.start[i] - nx.end(i))));
            else gp->seq[i].clear();
        } else {
            gp->seq[i] = upper(sub(g, m.end(i), nx.start[i] - m.end(i)));
        }
        if (gp->seq[i].size() > max_len) max_len = (unsigned)gp->seq[i].size();
        if (gp->seq[i].size() < min_len) min_len = (unsigned)gp->seq[i].size();
    }
    gp->max_len = max_len;
    gp->align = gap_is_aligned((long)max_len, (long)min_len, n);
    gp->failed = false;
}

void build_rows(const Aligner& a, const Lcb& ct, const std::vector<std::pair<size_t, Gap>>& aligned, std::vector<std::string>* rows, bool* gap_note) {
    const size_t n = a.n;
    rows->assign(n, "");
    {   // final row length, roughly: reference span plus a little for gap columns (avoids repeated regrowth)
        const long span = ct.end[0] - ct.start[0];
        const size_t guess = span > 0 ? (size_t)span + (size_t)span / 16 + 64 : 64;
        for (size_t i = 0; i < n; i++) (*rows)[i].reserve(guess);
    }
    const Mum& first = a.pool[(size_t)ct.mums[0]];
    // a MUM's text, lower case, the reverse complement for a reverse member (= lower(reverse_complement(sub(...))), written
    // straight into the row: 14 million of these per run at 200 x 5 Mb)
    auto append_mum = [&](std::string& dst, const Mum& m, size_t i) {
        const std::string& g = a.genomes[i].seq;
        const long pos = m.start[i];
        if (pos < 0 || (size_t)pos > g.size()) { std::cerr << "parsnp_core: substr out of range" << std::endl; exit(1); }
        const size_t len = std::min<size_t>((size_t)m.length, g.size() - (size_t)pos);     // substr clamps
        const size_t at = dst.size();
        if (first.fwd[i]) {
            dst.resize(at + len);
            const char* src = g.data() + pos; char* out = &dst[at];
            for (size_t x = 0; x < len; x++) out[x] = kCase.low[(unsigned char)src[x]];
        } else {
            dst.reserve(at + len);
            const char* src = g.data() + pos;
            for (size_t x = len; x-- > 0;) { const char c = kCase.rc_low[(unsigned char)src[x]]; if (c) dst.push_back(c); }
        }
    };
    Gap gp;
    size_t next_aligned = 0;
    for (size_t t = 0; t < ct.mums.size(); t++) {
        const Mum& m = a.pool[(size_t)ct.mums[t]];
        for (size_t i = 0; i < n; i++) append_mum((*rows)[i], m, i);
        if (t + 1 == ct.mums.size()) break;
        if (next_aligned < aligned.size() && aligned[next_aligned].first == t) {
            const Gap& ag = aligned[next_aligned++].second;
            if (!ag.failed) { for (size_t i = 0; i < n; i++) (*rows)[i] += ag.aligned[i]; continue; }
            *gap_note = true;
        }
        gap_between(a, ct, t, &gp);
        if (gp.max_len > 0)
            for (size_t i = 0; i < n; i++) (*rows)[i] += gp.seq[i] + std::string(gp.max_len - gp.seq[i].size(), '-');
    }
}

// ---- the file.  Its blocks are reserved while the gaps are being aligned, and the records are later stored through a shared
// mapping: positioned writes to ONE file queue up behind its inode lock whatever the number of threads (2 GB/s here), page faults
// on a mapping do not.  A file system that cannot reserve (or PARSNP_OUTPUT_PWRITE=1, test hook: no reserve() at all) gets the
// positioned writes.
struct FileSink {
    std::string path;
    int fd = -1;
    bool dbg = false, decided = false;
    long long reserved = 0, map_len = 0;
    std::future<bool> reserve_done;
    char* map = nullptr;
    [[noreturn]] void fail() const { std::cerr << "parsnp_core: cannot write " << path << std::endl; exit(1); }
    void open(const std::string& p, bool debug) { path = p; dbg = debug; fd = ::open(path.c_str(), O_RDWR); if (fd < 0) fail(); }
    void reserve(long long est) {      // an async task: the caller goes on
        reserved = est;
        reserve_done = std::async(std::launch::async, [fd = fd, est, dbg = dbg] {
            const double t0 = clock_s();
            const bool ok = fallocate(fd, 0, 0, (off_t)est) == 0;
            if (dbg) fprintf(stderr, "[output] reserve %lld MB: %s, %.4f s\n", est >> 20, ok ? "ok" : "not supported", clock_s() - t0);
            return ok;
        });
    }
    // bytes [0, upto) can be stored.  The first call decides how; later the mapping grows if a group needs more than was reserved
    // (only when gaps were aligned wider than the estimate allows for: host-aligned ones)
    void ensure(long long upto) {
        if (!decided) {
            decided = true;
            if (reserve_done.valid() && reserve_done.get()) {
                map_len = std::max(reserved, upto);
                if (map_len > reserved && fallocate(fd, 0, (off_t)reserved, (off_t)(map_len - reserved)) != 0) fail();
                if (map_len > 0) {
                    void* m = mmap(nullptr, (size_t)map_len, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
                    if (m != MAP_FAILED) map = (char*)m;
                }
            }
            if (dbg) fprintf(stderr, "[output] records through %s\n", map ? "a shared mapping" : "positioned writes");
        }
        if (map && upto > map_len) {
            const long long grown = upto + (upto - map_len);
            if (fallocate(fd, 0, (off_t)map_len, (off_t)(grown - map_len)) != 0) fail();
            void* m = mremap(map, (size_t)map_len, (size_t)grown, MREMAP_MAYMOVE);
            if (m == MAP_FAILED) fail();
            map = (char*)m; map_len = grown;
        }
    }
    bool store(long long off, const char* p, size_t len) const {      // any thread; false: the write failed
        if (map) { memcpy(map + off, p, len); return true; }
        for (size_t done = 0; done < len;) {
            const ssize_t k = pwrite(fd, p + done, len - done, (off_t)(off + (long long)done));
            if (k <= 0) return false;
            done += (size_t)k;
        }
        return true;
    }
    void close(long long final_size) {
        const bool bad = map && munmap(map, (size_t)map_len) != 0;
        if (ftruncate(fd, (off_t)final_size) != 0 || ::close(fd) != 0 || bad) { std::cerr << "parsnp_core: error writing " << path << std::endl; exit(1); }
    }
};

// a thread's buffer of stage_write: filled with wrapped text, stored whenever it is nearly full
struct RowStream {
    static constexpr size_t kBuf = (size_t)1 << 18, kPiece = 4096;
    const FileSink& sink;
    std::vector<char> buf;
    size_t w = 0; long long off = 0; int col = 0; long long produced = 0;
    int bad = 0;      // 1: a write failed, 2: a record is not of the size its place was worked out from
    explicit RowStream(const FileSink& s) : sink(s), buf(kBuf + 2 * kPiece) {}
    void flush() {
        if (!sink.store(off, buf.data(), w)) bad = 1;
        off += (long long)w; w = 0;
    }
    void text(const char* src, size_t len) {      // as it is, outside the rows (a header line)
        if (w + len >= kBuf) flush();
        memcpy(&buf[w], src, len); w += len;
    }
    void push(char c) { buf[w++] = c; }
    // `len` sequence characters src[0..len) through `table`, forwards or backwards, with a line end before every 81st
    void put(const char* src, size_t len, const char* table, bool backwards) {
        produced += (long long)len;
        size_t x = 0;
        while (x < len) {
            if (w >= kBuf) flush();
            size_t piece = std::min(len - x, kPiece);
            while (piece) {
                if (col == 80) { buf[w++] = '\n'; col = 0; }
                const size_t k = std::min(piece, (size_t)(80 - col));
                char* dst = &buf[w];      // (locals: a store through dst may be any member's, as far as the compiler knows)
                const char* s = backwards ? src + (len - 1 - x) : src + x;
                bool dropped = false;
                if (!table) memcpy(dst, s, k);
                else if (!backwards) for (size_t y = 0; y < k; y++) dst[y] = table[(unsigned char)s[y]];
                else for (size_t y = 0; y < k; y++) { const char c = table[(unsigned char)*(s - y)]; dst[y] = c; dropped |= !c; }
                if (dropped) bad = 2;
                w += k; x += k; col += (int)k; piece -= k;
            }
        }
    }
    void fill(char c, size_t len) {
        produced += (long long)len;
        while (len) {
            if (w >= kBuf) flush();
            if (col == 80) { buf[w++] = '\n'; col = 0; }
            const size_t k = std::min(std::min(len, (size_t)(80 - col)), kPiece);
            memset(&buf[w], c, k); w += k; col += (int)k; len -= k;
        }
    }
};

// ---- the record of one write_output call.  Every printable LCB is laid out first (which gaps are aligned, how many columns each
// contributes), the aligned gaps of ALL LCBs go to the device in one batch, and then every record is generated straight into its place
// in the file: with the column counts known, the size of every record -- and so the file offset of every row -- is known before a
// single base is formatted, and the threads stream the rows (MUM text from the genomes, gap rows from the aligner's output) through
// small buffers.  Nothing of the 1 GB text (200 x 5 Mb) is held in memory.  An LCB the stream cannot print as it stands -- one that
// overlaps the previous printed LCB on the reference (the trim of :928-952 works on the finished rows), or whose coordinates would make
// std::string::substr clamp or wrap -- is built as strings, the way the reference does it ("slow" below); so is everything with
// recombfilter (blocks/b<k>/seq.fna wants the records twice) or PARSNP_PLAIN_OUTPUT=1 (test hook: both ways give the same file).
struct XmfaWriter {
    struct Plan {
        bool regular = false;              // the stream can print it (unless it turns out to need the overlap trim)
        std::vector<int32_t> gmax;         // per gap: longest gap string
        std::vector<int32_t> gjob;         // per gap: index into `jobs` when the gap is aligned, else -1
        std::vector<int32_t> gcols;        // per gap: columns in the rows
        long cols = 0;                     // row length
    };
    struct Job { size_t z, t; unsigned max_len; long dev = -1; int grp = 0; Gap host; bool on_host = false, failed = false; };
    struct Group { size_t z0 = 0, z1 = 0, y0 = 0, y1 = 0; };      // its LCBs [z0, z1) and its device jobs [y0, y1)
    struct Batch { std::vector<int32_t> nseq, maxcols, cols; std::vector<int64_t> seqoff, rowoff; std::vector<uint8_t> chars, out; std::vector<long> job; };
    struct SlowSnp { long cols = 0; std::vector<int32_t> col; std::vector<int64_t> ref_left; std::vector<uint8_t> m; };      // m: n x col.size(), row-major
    static constexpr unsigned kNarrowCols = 96;      // a gap with a longer string counts as wide (GapCounts::jobs_wide)
    static constexpr unsigned kWideLen = 320;        // ... and one with a string longer than this as long (GapCounts::jobs_long)

    Aligner& a;
    const Params& prm;
    const size_t n;
    const long nl;
    const int threads;
    const bool dbg;
    const std::string stem, dir;
    const bool all_slow, all_forms;              // every LCB as strings; the provider has the device aligner with all its forms
    int dev_seqs = 512, dev_len = (int)kNarrowCols, dev_cols = (int)kNarrowCols, printable = 0;
    std::ofstream log;
    double tl = 0;
    std::vector<Plan> plan;
    std::vector<Job> jobs;
    long nj = 0, declined = 0;
    size_t ngroups = 1;
    std::vector<Group> batch;
    Batch B;
    std::vector<double> jt;                      // host seconds per job
    bool device_gaps_failed = false;
    std::vector<std::vector<std::string>> rows;  // per LCB.  Slow ones: the rows, until their text is made
    std::vector<std::string> text, heads;        // slow ones: the whole record text; all: the headers
    std::vector<std::vector<uint32_t>> head_end;
    std::vector<long long> bytes, where;         // a record's size and its place in the file
    std::vector<char> printed, slow, notes;
    std::vector<Lcb> trimmed;
    std::vector<SlowSnp> snp_slow;
    int prev_end = 0;                            // (stage_in_order) reference end of the last printed LCB
    FileSink file;
    long long text_at = 0, at = 0;               // where the records start, and those of the next group
    std::unique_ptr<SnpCollector> snp;
    // the device call (last: what its thread refers to is still there when the future goes away)
    std::vector<std::promise<int>> batch_done;
    std::vector<std::future<int>> batch_ready;
    size_t reported = 0;                         // groups whose promise is kept (the side thread's)
    pm_gap_long_tall_stats device_stats{0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0};
    std::future<void> device_side;

    static bool plain_output() { static const bool v = test_hook("PARSNP_PLAIN_OUTPUT") != nullptr; return v; }
    XmfaWriter(Aligner& al, const std::string& stem_)
        : a(al), prm(al.prm), n(al.n), nl((long)al.lcbs.size()), threads(al.prm.cores > 0 ? al.prm.cores : 1), dbg(getenv("PARSNP_DEBUG_TIMERS") != nullptr),
          stem(stem_), dir(al.prm.outdir + "/"), all_slow(plain_output() || al.prm.recomb_filter),
          all_forms(pm_gap_align_groups_long_tall != nullptr && pm_gap_limits_long_tall != nullptr),
          plan((size_t)nl), rows((size_t)nl), text((size_t)nl), heads((size_t)nl), head_end((size_t)nl), bytes((size_t)nl, 0), where((size_t)nl, 0),
          printed((size_t)nl, 0), slow((size_t)nl, 0), notes((size_t)nl, 0), trimmed((size_t)nl) {
        if (all_forms) pm_gap_limits_long_tall(&dev_seqs, &dev_len, &dev_cols);
    }

    void lap(const char* what) { if (dbg) { double t = clock_s(); fprintf(stderr, "[output] %-14s %.4f s\n", what, t - tl); tl = t; } }
    bool printable_lcb(const Lcb& ct) const { return ct.type == 1 && !ct.mums.empty() && prm.do_align != 0; }
    static long long wrapped(long long s) { return s + (s == 0 ? 1 : (s + 79) / 80); }     // s columns + their line ends

    // the directory, the log (written last), the XMFA's header lines
    void open_files() {
        using namespace std;
        if (!ofstream((dir + "parsnpAligner.log").c_str()).good() && system(("mkdir " + prm.outdir).c_str())) {
            cerr << "ParSNP:: error creating output directory, exiting.." << endl;
            exit(1);
        }
        if (prm.recomb_filter) { int rc = system(("mkdir " + dir + "blocks/").c_str()); (void)rc; }
        ofstream xmfa((dir + stem + ".xmfa").c_str());
        log.open((dir + stem + ".log").c_str());
        { ofstream allmums("allmums.out"); }   // the reference leaves an empty file in the cwd (:600-601)
        for (const Lcb& c : a.lcbs) if (c.type == 1) printable++;
        xmfa << ext_header_text(a.genomes, printable);
        xmfa.flush();
        text_at = at = (long long)xmfa.tellp();
        tl = clock_s();
    }

    // ---- layout of every LCB, from integers: the length of genome i's gap string between two MUMs (*clean = false: the string
    // route's substr would clamp, wrap or refuse here)
    long gap_length(const Mum& first, const Mum& m, const Mum& nx, size_t i, bool* clean) const {
        const long gs = (long)a.genomes[i].seq.size();
        if (!first.fwd[i]) {
            const long pos = nx.end(i), len = m.start[i] - nx.end(i);
            if (pos < 0 || pos > gs) { *clean = false; return 0; }
            if (len < 1) return 0;
            if (pos + len > gs) *clean = false;
            return len;
        }
        const long pos = m.end(i), len = nx.start[i] - m.end(i);
        if (pos < 0 || pos > gs || len < 0 || pos + len > gs) { *clean = false; return 0; }
        return len;
    }
    void plan_lcbs() {
#pragma omp parallel for schedule(dynamic, 4) num_threads(threads)
        for (long z = 0; z < nl; z++) {
            const Lcb& ct = a.lcbs[(size_t)z];
            if (!printable_lcb(ct)) continue;
            Plan& pl = plan[(size_t)z];
            const size_t T = ct.mums.size();
            pl.gmax.assign(T - 1, 0); pl.gjob.assign(T - 1, -1); pl.gcols.assign(T - 1, 0);
            const Mum& first = a.pool[(size_t)ct.mums[0]];
            bool clean = true;
            for (size_t t = 0; t < T; t++) {
                const Mum& m = a.pool[(size_t)ct.mums[t]];
                for (size_t i = 0; i < n; i++) {
                    const long pos = m.start[i];
                    if (pos < 0 || m.length < 0 || pos + m.length > (long)a.genomes[i].seq.size()) clean = false;
                }
                if (t + 1 == T) break;
                const Mum& nx = a.pool[(size_t)ct.mums[t + 1]];
                long mx = 0, mn = 1000000;
                for (size_t i = 0; i < n; i++) { const long l = gap_length(first, m, nx, i, &clean); mx = std::max(mx, l); mn = std::min(mn, l); }
                pl.gmax[t] = (int32_t)mx;
                if (gap_is_aligned(mx, mn, n)) pl.gjob[t] = 0;      // (numbered by list_jobs)
            }
            pl.regular = clean;
            slow[(size_t)z] = all_slow || !clean;
        }
    }
    // ---- the gaps that are aligned
    void list_jobs() {
        for (long z = 0; z < nl; z++) {
            Plan& pl = plan[(size_t)z];
            if (!pl.regular) continue;                               // (an irregular LCB aligns its own gaps: slow_rows)
            for (size_t t = 0; t < pl.gjob.size(); t++)
                if (pl.gjob[t] == 0) { Job j; j.z = (size_t)z; j.t = t; j.max_len = (unsigned)pl.gmax[t]; jobs.push_back(std::move(j)); }
                else pl.gjob[t] = -1;
        }
        // longest first: the cost of one alignment grows with the square of the gap length, and a long one started last
        // would leave every other thread idle
        std::stable_sort(jobs.begin(), jobs.end(), [](const Job& x, const Job& y) { return x.max_len > y.max_len; });
        nj = (long)jobs.size();
        jt.assign((size_t)nj, 0.0);
        for (long x = 0; x < nj; x++) plan[jobs[(size_t)x].z].gjob[jobs[(size_t)x].t] = (int32_t)x;
        gap_counts.jobs = nj;
        for (const Job& j : jobs) { gap_counts.jobs_wide += j.max_len > kNarrowCols; gap_counts.jobs_long += j.max_len > kWideLen; gap_counts.longest = std::max<long>(gap_counts.longest, (long)j.max_len); }
    }
    // The LCBs are cut into a few groups of consecutive LCBs with about the same alignment work, one device batch each:
    // the file offsets of a group's records only depend on the groups before it, so its records are written while the
    // device aligns the gaps of the next group.  PARSNP_GAP_GROUPS (test hook) sets the number.
    void cut_groups() {
        static const long want_groups = test_hook("PARSNP_GAP_GROUPS") ? atol(test_hook("PARSNP_GAP_GROUPS")) : 0;
        ngroups = (size_t)std::max<long>(1, std::min<long>(16, want_groups > 0 ? want_groups : (nj >= 6000 && !all_slow ? 3 : 1)));
        batch.assign(ngroups, Group());
        std::vector<double> work((size_t)nl + 1, 0.0);            // alignment work before LCB z (a gap costs about its width squared)
        for (const Job& j : jobs) work[j.z + 1] += (double)(j.max_len + 4) * (j.max_len + 4);
        for (long z = 0; z < nl; z++) work[(size_t)z + 1] += work[(size_t)z] + 1e-9;
        size_t z = 0;
        for (size_t g = 0; g < ngroups; g++) {
            batch[g].z0 = z;
            const double upto = work[(size_t)nl] * (double)(g + 1) / (double)ngroups;
            while (z < (size_t)nl && (g + 1 == ngroups || work[z + 1] <= upto)) z++;
            batch[g].z1 = z;
        }
        batch[ngroups - 1].z1 = (size_t)nl;
        for (Job& j : jobs) for (size_t g = 0; g < ngroups; g++) if (j.z >= batch[g].z0 && j.z < batch[g].z1) j.grp = (int)g;
    }
    // the gap string of genome i between MUM t and t+1 of a regular LCB (upper case; reverse complement on a reverse LCB row)
    size_t gap_text(const Lcb& ct, size_t t, size_t i, char* dst) const {
        const Mum& first = a.pool[(size_t)ct.mums[0]];
        const Mum& m = a.pool[(size_t)ct.mums[t]];
        const Mum& nx = a.pool[(size_t)ct.mums[t + 1]];
        const char* g = a.genomes[i].seq.data();
        if (first.fwd[i]) {
            const long pos = m.end(i), len = nx.start[i] - pos;
            for (long x = 0; x < len; x++) dst[x] = kCase.up[(unsigned char)g[pos + x]];
            return (size_t)len;
        }
        const long pos = nx.end(i), len = m.start[i] - pos;
        size_t w = 0;
        for (long x = len; x-- > 0;) { const char c = kCase.rc_up[(unsigned char)g[pos + x]]; if (c) dst[w++] = c; }
        return w;
    }
    // The gaps go to the device in ONE batch (pm_gap_align_groups_long_tall: include/parsnp_mum.h); the few the device does not take
    // -- outside its limits (pm_gap_limits_long_tall: 2 048 sequences of 1 024 bases, 2 048 columns: every gap of a d up to 1 000),
    // or declined -- are aligned here by the host threads, the widest ones while the device works on the rest.  The library
    // gives every job the smallest of its forms that holds it, so a run makes this one call whatever its gaps are.
    // PARSNP_HOST_GAPS=1: everything on the host (measurement / tests).
    void pack_device_batch() {
        static const bool host_gaps = test_hook("PARSNP_HOST_GAPS") != nullptr;
        if (host_gaps || n > (size_t)dev_seqs) return;
        int64_t out_bytes = 0;
        for (size_t g = 0; g < ngroups; g++) {               // group after group; the sorted order carries over: every group is longest first
            batch[g].y0 = B.job.size();
            for (long x = 0; x < nj; x++) {
                Job& j = jobs[(size_t)x];
                if (j.grp != (int)g || j.max_len > (unsigned)dev_len) continue;
                j.dev = (long)B.job.size(); B.job.push_back(x);
                // row capacity: half as much again as the longest string and a little (a job that needs more is declined and goes
                // to the host); three quarters for the long ones, whose alignments reach 1.65 times their strings
                const int32_t cap = (int32_t)std::min<unsigned>((unsigned)dev_cols, j.max_len > kNarrowCols ? j.max_len + (3 * j.max_len) / 4 + 16 : j.max_len + j.max_len / 2 + 16);
                B.nseq.push_back((int32_t)n); B.maxcols.push_back(cap); B.rowoff.push_back(out_bytes);
                out_bytes += (int64_t)n * cap;
            }
            batch[g].y1 = B.job.size();
        }
        int short_rows = 0;
        const long nd = (long)B.job.size();
        // the strings, job after job: lengths first (one offset per sequence), then the text by all threads
        B.seqoff.assign((size_t)nd * n + 1, 0);
#pragma omp parallel for schedule(dynamic, 64) num_threads(threads)
        for (long y = 0; y < nd; y++) {
            const Job& j = jobs[(size_t)B.job[(size_t)y]];
            const Lcb& ct = a.lcbs[j.z];
            const Mum& first = a.pool[(size_t)ct.mums[0]];
            const Mum& m = a.pool[(size_t)ct.mums[j.t]];
            const Mum& nx = a.pool[(size_t)ct.mums[j.t + 1]];
            bool clean = true;
            for (size_t i = 0; i < n; i++) B.seqoff[(size_t)y * n + i + 1] = gap_length(first, m, nx, i, &clean);
        }
        for (size_t k = 1; k < B.seqoff.size(); k++) B.seqoff[k] += B.seqoff[k - 1];
        B.chars.resize((size_t)B.seqoff.back() + 1);
#pragma omp parallel for schedule(dynamic, 64) num_threads(threads) reduction(| : short_rows)
        for (long y = 0; y < nd; y++) {
            const Job& j = jobs[(size_t)B.job[(size_t)y]];
            for (size_t i = 0; i < n; i++) {
                const size_t at = (size_t)B.seqoff[(size_t)y * n + i], want = (size_t)(B.seqoff[(size_t)y * n + i + 1] - B.seqoff[(size_t)y * n + i]);
                if (gap_text(a.lcbs[j.z], j.t, i, (char*)B.chars.data() + at) != want) short_rows = 1;
            }
        }
        B.out.resize((size_t)out_bytes); B.cols.assign((size_t)nd, -1);
        if (short_rows) { std::cerr << "parsnp_core: a genome holds a character its reverse complement drops" << std::endl; exit(1); }
    }
    // The file's blocks are reserved while the gaps are being aligned: an estimate of its size, aligned gaps at their row capacity
    void reserve_file() {
        file.open(dir + stem + ".xmfa", dbg);
        static const bool force_pwrite = test_hook("PARSNP_OUTPUT_PWRITE") != nullptr;
        if (force_pwrite || all_slow) return;
        long long est = text_at;
        for (long z = 0; z < nl; z++) {
            const Plan& pl = plan[(size_t)z];
            if (!pl.regular) continue;
            const long long cols = lcb_columns(a, a.lcbs[(size_t)z], [&](size_t t) {
                return pl.gjob[t] >= 0 && jobs[(size_t)pl.gjob[t]].dev >= 0 ? B.maxcols[(size_t)jobs[(size_t)pl.gjob[t]].dev] : pl.gmax[t]; });
            est += (long long)n * (cols + cols / 80 + 2 + 64) + 2;
        }
        if (test_hook("PARSNP_RESERVE_TINY")) est = text_at + 4096;      // test hook: the mapping has to grow with every group
        file.reserve(est);
    }
    // one side thread makes the ONE device call; the library reports every group as its rows arrive (pm_gap_align_groups),
    // and the main thread takes them in that order (take_group)
    void start_device_call() {
        batch_done = std::vector<std::promise<int>>(ngroups);
        for (auto& pr : batch_done) batch_ready.push_back(pr.get_future());
        device_side = std::async(std::launch::async, [this] {
            int rc = PM_OK;
            if (!B.job.empty()) {
                std::vector<int64_t> group_end(ngroups);
                for (size_t g = 0; g < ngroups; g++) group_end[g] = (int64_t)batch[g].y1;
                const double t0 = clock_s();
                auto report = [](void* ctx, int) { XmfaWriter* w = (XmfaWriter*)ctx; w->batch_done[w->reported++].set_value(PM_OK); };
                if (all_forms)
                    rc = pm_gap_align_groups_long_tall(-1, (int64_t)B.job.size(), B.nseq.data(), B.seqoff.data(), B.chars.data(), B.maxcols.data(), B.rowoff.data(),
                                                       B.out.data(), (int64_t)B.out.size(), B.cols.data(), (int)ngroups, group_end.data(), report, this, &device_stats);
                else
                    rc = pm_gap_align_groups(-1, (int64_t)B.job.size(), B.nseq.data(), B.seqoff.data(), B.chars.data(), B.maxcols.data(), B.rowoff.data(),
                                             B.out.data(), (int64_t)B.out.size(), B.cols.data(), (int)ngroups, group_end.data(), report, this);
                if (dbg) fprintf(stderr, "[output] gaps: device   %.4f s (%zu gaps in %zu groups)\n", clock_s() - t0, B.job.size(), ngroups);
            }
            while (reported < ngroups) batch_done[reported++].set_value(rc);      // (no device jobs, or a failure: the rest hears of it)
        });
    }
    void host_align(const std::vector<long>& which) {
        const long nw = (long)which.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
        for (long y = 0; y < nw; y++) {
            const long x = which[(size_t)y];
            Job& j = jobs[(size_t)x];
            const double t0 = clock_s();
            gap_between(a, a.lcbs[j.z], j.t, &j.host);
            j.on_host = true;
            j.failed = !gap_align(j.host.seq, &j.host.aligned);
            if (!j.failed)                       // (rows of one alignment have one length; anything else is not printable here)
                for (const std::string& r : j.host.aligned) if (r.size() != j.host.aligned[0].size()) { std::cerr << "parsnp_core: ragged gap alignment" << std::endl; exit(1); }
            jt[(size_t)x] = clock_s() - t0;
        }
    }
    void host_align_rest() {      // the jobs that did not go into the batch, while the device works
        std::vector<long> rest;
        for (long x = 0; x < nj; x++) if (jobs[(size_t)x].dev < 0) rest.push_back(x);
        host_align(rest);
    }
    // snps=1 (snps.cpp): the columns between the MUMs go to the collector group after group, once the group is written.  A slow LCB
    // keeps, from its finished rows (after the overlap trim), the columns that are not the same one of a c g t in every row.
    void start_snp_collection() {
        snp_counts = SnpCounts();
        if (prm.snps) snp.reset(new SnpCollector(a.session(), n, threads));
        snp_slow.resize(snp ? (size_t)nl : 0);
    }

    // ---- group after group: wait for its alignments, lay it out, write it
    void take_group(size_t g) {
        const Group& G = batch[g];
        if (batch_ready[g].get() != PM_OK) {
            // the alignment itself is complete by now; a device that cannot take the gaps (out of memory for the workspace, a
            // part that refuses the LDS request, a stream error) only costs time: every job of the group counts as declined
            // and goes through the host aligner, which produces the same rows
            if (!device_gaps_failed) std::cerr << "parsnp_core: gap alignment on the device failed (" << pm_gap_last_error() << "): aligning the gaps on the host" << std::endl;
            device_gaps_failed = true;
            for (size_t y = G.y0; y < G.y1; y++) B.cols[y] = -1;
        }
        std::vector<long> rest;
        for (size_t y = G.y0; y < G.y1; y++) if (B.cols[y] < 0) rest.push_back(B.job[y]);
        declined += (long)rest.size();
        host_align(rest);
    }
    // row i of an aligned gap: pointer + length (nullptr: the alignment failed, the gap is padded instead)
    const char* aligned_row(const Job& j, size_t i, size_t* len) const {
        if (j.on_host) { if (j.failed) return nullptr; *len = j.host.aligned[i].size(); return j.host.aligned[i].data(); }
        const size_t y = (size_t)j.dev;
        *len = (size_t)B.cols[y];
        return (const char*)B.out.data() + B.rowoff[y] + (int64_t)i * B.maxcols[y];
    }
    void stage_columns(const Group& G) {
#pragma omp parallel for schedule(dynamic, 4) num_threads(threads)
        for (long z = (long)G.z0; z < (long)G.z1; z++) {
            Plan& pl = plan[(size_t)z];
            if (!pl.regular) continue;
            for (size_t t = 0; t < pl.gjob.size(); t++) {
                pl.gcols[t] = pl.gmax[t];
                if (pl.gjob[t] < 0) continue;
                size_t len = 0;
                if (aligned_row(jobs[(size_t)pl.gjob[t]], 0, &len)) pl.gcols[t] = (int32_t)len; else notes[(size_t)z] = 1;
            }
            pl.cols = (long)lcb_columns(a, a.lcbs[(size_t)z], [&](size_t t) { return pl.gcols[t]; });
        }
    }
    // the slow way for one LCB: its rows as strings (build_rows), from the same gap alignments
    void slow_rows(size_t z) {
        const Lcb& ct = a.lcbs[z];
        const Plan& pl = plan[z];
        std::vector<std::pair<size_t, Gap>> aligned;
        if (!pl.regular) {                                   // its gaps were not in the batch
            Gap gp;
            for (size_t t = 0; t + 1 < ct.mums.size(); t++) { gap_between(a, ct, t, &gp); if (gp.align) aligned.emplace_back(t, gp); }
            const double t0 = clock_s();
            for (auto& tg : aligned) tg.second.failed = !gap_align(tg.second.seq, &tg.second.aligned);
            long wide_here = 0, long_here = 0, longest_here = 0;
            for (auto& tg : aligned) { wide_here += tg.second.max_len > kNarrowCols; long_here += tg.second.max_len > kWideLen; longest_here = std::max<long>(longest_here, (long)tg.second.max_len); }
            const double spent = clock_s() - t0;
#pragma omp critical(parsnp_gap_counts)
            { gap_counts.jobs += (long)aligned.size(); gap_counts.host += (long)aligned.size(); gap_counts.jobs_wide += wide_here; gap_counts.jobs_long += long_here;
              gap_counts.longest = std::max(gap_counts.longest, longest_here); gap_counts.host_s += spent; }
        } else {
            for (size_t t = 0; t < pl.gjob.size(); t++) {
                if (pl.gjob[t] < 0) continue;
                const Job& j = jobs[(size_t)pl.gjob[t]];
                aligned.emplace_back(t, Gap());
                Gap& gp = aligned.back().second;
                gap_between(a, ct, t, &gp);
                gp.aligned.resize(n);
                for (size_t i = 0; i < n; i++) { size_t len = 0; const char* r = aligned_row(j, i, &len); if (!r) { gp.failed = true; break; } gp.aligned[i].assign(r, len); }
            }
        }
        bool note = false;
        build_rows(a, ct, aligned, &rows[z], &note);
        if (note) notes[z] = 1;
    }
    void stage_slow_rows(const Group& G) {
        std::vector<long> which;
        for (long z = (long)G.z0; z < (long)G.z1; z++) if (slow[(size_t)z]) which.push_back(z);
        const long nw = (long)which.size();
#pragma omp parallel for schedule(dynamic) num_threads(threads)
        for (long y = 0; y < nw; y++) slow_rows((size_t)which[(size_t)y]);
    }
    // In LCB order: the overlap trim against the previous printed LCB (it shortens rows and shifts the starts).
    void stage_in_order(const Group& G) {
        using namespace std;
        for (size_t z = G.z0; z < G.z1; z++) {
            const Lcb& c0 = a.lcbs[z];
            if (!printable_lcb(c0)) continue;
            const int lcb_start = (int)c0.start[0] + 1, lcb_end = (int)c0.end[0];
            if (!slow[z]) {
                if (!(plan[z].cols > (long)(prm.c * 1))) continue;
                static const long mix = test_hook("PARSNP_OUTPUT_MIX") ? atol(test_hook("PARSNP_OUTPUT_MIX")) : 0;   // test hook: every mix-th LCB takes the late string route
                if (std::max(0, prev_end - lcb_start) == 0 && !(mix > 0 && z % (size_t)mix == 0)) { prev_end = lcb_end; trimmed[z] = c0; printed[z] = 1; continue; }
                slow_rows(z); slow[z] = 1;                       // it has to be trimmed: as strings
            }
            Lcb ct = c0;
            vector<string>& row = rows[z];
            if (!(row[0].size() > (size_t)(prm.c * 1))) continue;
            // trim the overlap with the previous printed LCB on the reference (:928-952, quirks kept: the column scan
            // never advances, and the start shift counts the non-gap columns of the whole reference row -- for genomes
            // after the first through the already shortened row 0, whose buffer still holds the old tail)
            int overlap = std::max(0, prev_end - lcb_start);
            if (overlap > 0) {
                if (row[0].empty() || row[0][0] == '-') { cerr << "parsnp_core: overlap trim would not terminate in the reference" << endl; exit(1); }
                const int cols = overlap;
                const string orig0 = row[0];
                const size_t newsize = orig0.size() > (size_t)cols ? orig0.size() - (size_t)cols : 0;
                auto stale0 = [&](size_t pos) -> char {   // row 0 as the reference sees it after its erase(0, cols)
                    if (pos < newsize) return orig0[pos + (size_t)cols];
                    if (pos == newsize) return '\0';
                    return pos < orig0.size() ? orig0[pos] : '\0';
                };
                for (size_t i = 0; i < n; i++) {
                    int count = 0;
                    for (size_t pos = 0; pos < row[i].size(); pos++) {
                        char ch = i == 0 ? (pos < orig0.size() ? orig0[pos] : '\0') : stale0(pos);
                        if (ch != '-') count++;
                    }
                    ct.start[i] += count;
                    row[i].erase(0, (size_t)cols);
                }
            }
            prev_end = lcb_end;
            if (!(row[0].size() > (size_t)(prm.c * 1))) continue;
            trimmed[z] = ct; printed[z] = 1;
        }
    }
    // headers of LCB z, one per genome, each ending in '\n' (:980-1049)
    void headers(size_t z, std::string* out, std::vector<uint32_t>* ends) const {
        const Lcb& ct = trimmed[z];
        const Mum& first = a.pool[(size_t)ct.mums.front()];
        out->clear(); ends->clear();
        char b[160];
        for (size_t i = 0; i < n; i++) {
            // contig label and offset: last pos2hdr entry at or before the LCB start (:994-1037)
            // (the reference scans the map in key order; the entry it ends on is the last key <= start)
            const std::string* hdr = nullptr;
            int seqstart = 0;
            {
                const auto& p2h = a.genomes[i].pos2hdr;
                auto it = p2h.upper_bound((int)ct.start[i]);
                if (it != p2h.begin()) { --it; hdr = &it->second; seqstart = it->first; }
            }
            static const std::string s1 = "s1";
            int offset = 0;
            if (!hdr || *hdr == "") { hdr = &s1; offset = -1; }
            else if (*hdr != "s1") offset = -1;
            const Interval iv = printed_interval(a, ct, i);
            int w = snprintf(b, sizeof b, "> %zu:%ld-%ld %c cluster%d ", i + 1, iv.lo, iv.hi, iv.fwd ? '+' : '-', (int)z + 1);
            out->append(b, (size_t)w);
            out->append(*hdr);
            w = snprintf(b, sizeof b, ":p%ld\n", (long)(ct.start[i] - seqstart) + 1 + (iv.fwd ? 0 : first.length) + offset);
            out->append(b, (size_t)w);
            ends->push_back((uint32_t)out->size());
        }
    }
    // a slow LCB's record text from its finished rows; with recombfilter also blocks/b<z+1>/seq.fna: the same records, without the terminator
    void slow_text(size_t z) {
        using namespace std;
        const vector<string>& row = rows[z];
        string& out = text[z];
        size_t total = 4 + heads[z].size();
        for (size_t i = 0; i < n; i++) total += row[i].size() + row[i].size() / 80 + 2;
        out.reserve(total);
        for (size_t i = 0; i < n; i++) {
            const string& s = row[i];
            out.append(heads[z], i ? head_end[z][i - 1] : 0, head_end[z][i] - (i ? head_end[z][i - 1] : 0));
            size_t k = 0;
            const size_t width = 80;
            for (; k + width < s.size(); k += width) { out.append(s, k, width); out += '\n'; }
            out.append(s, k, string::npos); out += '\n';
        }
        if (prm.recomb_filter) {
            string bdir = dir + "blocks/b" + std::to_string((int)z + 1);
            int rc = system(("mkdir -p " + bdir).c_str()); (void)rc;
            ofstream block((bdir + "/seq.fna").c_str());
            block.write(out.data(), (std::streamsize)out.size());
        }
        out += "=\n";
    }
    // ... and what the SNP collector gets of it
    void slow_snp_columns(size_t z) {
        const std::vector<std::string>& row = rows[z];
        SlowSnp& sv = snp_slow[z];
        sv.cols = (long)row[0].size();
        auto at = [&](size_t i, size_t c) -> char { return c < row[i].size() ? row[i][c] : '-'; };
        int64_t left = 0;
        for (size_t c = 0; c < row[0].size(); c++) {
            const char c0 = row[0][c];
            bool mum = c0 == 'a' || c0 == 'c' || c0 == 'g' || c0 == 't';
            for (size_t i = 1; i < n && mum; i++) mum = at(i, c) == c0;
            if (!mum) { sv.col.push_back((int32_t)c); sv.ref_left.push_back(left); }
            left += c0 != '-';
        }
        const size_t k = sv.col.size();
        sv.m.resize(n * k);
        for (size_t i = 0; i < n; i++) for (size_t x = 0; x < k; x++) sv.m[i * k + x] = (uint8_t)at(i, (size_t)sv.col[x]);
    }
    // All threads: headers and sizes of the records of every printed LCB, hence their places in the file.
    void stage_sizes(const Group& G) {
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
        for (long zz = (long)G.z0; zz < (long)G.z1; zz++) {
            const size_t z = (size_t)zz;
            if (!printed[z]) continue;
            headers(z, &heads[z], &head_end[z]);
            if (!slow[z]) { bytes[z] = (long long)heads[z].size() + (long long)n * wrapped(plan[z].cols) + 2; continue; }
            slow_text(z);
            bytes[z] = (long long)text[z].size();
            if (snp) slow_snp_columns(z);
            std::vector<std::string>().swap(rows[z]);
        }
    }
    // All threads: the records, wrapped at 80 columns, stored where they belong (1 GB at 200 x 5 Mb).
    void stage_write(const Group& G) {
        for (size_t z = G.z0; z < G.z1; z++) { where[z] = at; at += bytes[z]; }
        file.ensure(at);
        // work items: a slow LCB's text, or a run of rows of a streamed LCB (about 1 MB of file each; the rows of one LCB
        // have one size, so every row's place follows from its number)
        struct Item { size_t z; size_t i0, i1; };
        std::vector<Item> items;
        for (size_t z = G.z0; z < G.z1; z++) {
            if (!printed[z]) continue;
            if (slow[z]) { items.push_back(Item{z, 0, 0}); continue; }
            const long long rowb = wrapped(plan[z].cols) + 48;
            const size_t per = (size_t)std::max<long long>(1, ((long long)1 << 20) / rowb);
            for (size_t i0 = 0; i0 < n; i0 += per) items.push_back(Item{z, i0, std::min(n, i0 + per)});
        }
        const long ni = (long)items.size();
        int bad = 0;
#pragma omp parallel num_threads(threads) reduction(| : bad)
        {
            RowStream rs(file);
            std::vector<char> gbuf;
#pragma omp for schedule(dynamic, 1)
            for (long it = 0; it < ni; it++) {
                const Item& item = items[(size_t)it];
                const size_t z = item.z;
                if (slow[z]) { if (!file.store(where[z], text[z].data(), text[z].size())) rs.bad = 1; continue; }
                const Lcb& ct = a.lcbs[z];
                const Plan& pl = plan[z];
                const Mum& first = a.pool[(size_t)ct.mums[0]];
                const long long rowb = wrapped(pl.cols);
                const size_t T = ct.mums.size();
                rs.w = 0; rs.col = 0;
                rs.off = where[z] + (long long)(item.i0 ? head_end[z][item.i0 - 1] : 0) + (long long)item.i0 * rowb;
                for (size_t i = item.i0; i < item.i1; i++) {
                    const uint32_t h0 = i ? head_end[z][i - 1] : 0, h1 = head_end[z][i];
                    rs.text(heads[z].data() + h0, h1 - h0);
                    rs.col = 0; rs.produced = 0;
                    const char* g = a.genomes[i].seq.data();
                    const bool fw = first.fwd[i] != 0;
                    for (size_t t = 0; t < T; t++) {
                        const Mum& m = a.pool[(size_t)ct.mums[t]];
                        // a MUM's text, lower case, the reverse complement for a reverse member
                        rs.put(g + m.start[i], (size_t)m.length, fw ? kCase.low : kCase.rc_low, !fw);
                        if (t + 1 == T) break;
                        const long gc = pl.gcols[t];
                        size_t len = 0;
                        const char* r = pl.gjob[t] >= 0 ? aligned_row(jobs[(size_t)pl.gjob[t]], i, &len) : nullptr;
                        if (r) { rs.put(r, len, nullptr, false); continue; }
                        if (gc == 0) continue;
                        if (gbuf.size() < (size_t)gc + 8) gbuf.resize((size_t)gc + 8);
                        len = gap_text(ct, t, i, gbuf.data());          // left-justified, '-' padded
                        rs.put(gbuf.data(), len, nullptr, false);
                        rs.fill('-', (size_t)gc - len);
                    }
                    rs.push('\n');
                    if (rs.produced != pl.cols) rs.bad = 2;                     // (a dropped character: cannot happen with ingest()'s alphabet)
                }
                if (item.i1 == n) { rs.push('='); rs.push('\n'); }
                rs.flush();
                const long long end = where[z] + (long long)head_end[z][item.i1 - 1] + (long long)item.i1 * rowb + (item.i1 == n ? 2 : 0);
                if (rs.off != end) rs.bad = 2;
            }
            bad |= rs.bad;
        }
        if (bad) { std::cerr << "parsnp_core: error writing " << file.path << (bad == 2 ? " (record sizes)" : "") << std::endl; exit(1); }
    }
    void slow_snps(size_t z, int64_t ref_a) {
        SlowSnp& sv = snp_slow[z];
        const size_t k = sv.col.size();
        std::vector<int64_t> ref_pos;
        snp->add_invariant(sv.cols - (long)k);
        for (size_t p = 0; p < k;) {      // runs of consecutive columns, 4 096 at the most
            size_t q = p + 1;
            while (q < k && q - p < 4096 && sv.col[q] == sv.col[q - 1] + 1) q++;
            ref_pos.clear();
            for (size_t x = p; x < q; x++) ref_pos.push_back(ref_a + sv.ref_left[x]);
            snp->add_block((int)z + 1, sv.col[p], q - p, [&](size_t i, uint8_t* dst) { memcpy(dst, sv.m.data() + i * k + p, q - p); }, ref_pos.data(), 0);
            p = q;
        }
        SlowSnp().m.swap(sv.m);
    }
    void stage_snps(const Group& G) {
        if (!snp) return;
        for (size_t z = G.z0; z < G.z1; z++) {
            if (!printed[z]) continue;
            const int64_t ref_a = printed_interval(a, trimmed[z], 0).lo;
            if (slow[z]) { slow_snps(z, ref_a); continue; }
            // the gaps of a streamed LCB: listed, then filled by all threads (a thread takes rows, every block of them), as many
            // blocks at a time as the staging matrix holds, then committed in order (the reference positions run from left to right)
            const Lcb& c0 = a.lcbs[z];
            const Plan& pl = plan[z];
            struct Blk { size_t t; long col, gc; const Job* j; size_t at; };
            std::vector<Blk> blks;
            long col = 0;
            for (size_t t = 0; t < c0.mums.size(); t++) {
                const long len = a.pool[(size_t)c0.mums[t]].length;
                snp->add_invariant(len); col += len;
                if (t + 1 == c0.mums.size()) break;
                const long gc = pl.gcols[t];
                if (gc == 0) continue;
                const Job* j = pl.gjob[t] >= 0 ? &jobs[(size_t)pl.gjob[t]] : nullptr;
                size_t len0 = 0;
                if (j && !aligned_row(*j, 0, &len0)) j = nullptr;      // (the alignment failed: padded, as it was written)
                blks.push_back(Blk{t, col, gc, j, 0});
                col += gc;
            }
            int64_t ref_left = 0; long last_col = 0;      // characters other than '-' of the reference row left of last_col
            for (size_t b0 = 0; b0 < blks.size();) {
                size_t b1 = b0, need = 0;
                while (b1 < blks.size() && (b1 == b0 || need + (size_t)blks[b1].gc <= snp->pitch())) { blks[b1].at = need; need += (size_t)blks[b1].gc; b1++; }
                uint8_t* base = snp->reserve(need);
                const size_t pitch = snp->pitch();
#pragma omp parallel for schedule(static) num_threads(threads)
                for (long i = 0; i < (long)n; i++)
                    for (size_t b = b0; b < b1; b++) {
                        const Blk& k = blks[b];
                        uint8_t* dst = base + (size_t)i * pitch + k.at;
                        size_t w = 0;
                        if (k.j) { const char* r = aligned_row(*k.j, (size_t)i, &w); memcpy(dst, r, w); }
                        else w = gap_text(c0, k.t, (size_t)i, (char*)dst);
                        memset(dst + w, '-', (size_t)k.gc - w);
                    }
                for (size_t b = b0; b < b1; b++) {
                    const Blk& k = blks[b];
                    ref_left += k.col - last_col;      // (the MUM columns in between hold no '-')
                    ref_left += snp->commit((int)z + 1, k.col, (size_t)k.gc, nullptr, ref_a + ref_left);
                    last_col = k.col + k.gc;
                }
                b0 = b1;
            }
        }
    }

    // ---- after the last group
    void close_file() {
        device_side.get();
        file.close(at);
    }
    void gap_summary(bool* gap_note) {
        for (char c : notes) if (c) *gap_note = true;
        const size_t on_device = B.job.size();
        double sum = 0, mx = 0; long arg = 0, on_host = 0;
        for (long x = 0; x < nj; x++) { sum += jt[(size_t)x]; on_host += jobs[(size_t)x].on_host; if (jt[(size_t)x] > mx) { mx = jt[(size_t)x]; arg = x; } }
        gap_counts.host += on_host; gap_counts.host_s += sum;
        if (device_gaps_failed) device_stats = pm_gap_long_tall_stats{0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0};
        else if (!all_forms) device_stats.jobs_narrow = (int64_t)on_device - declined;      // (a provider with the narrow form alone reports nothing)
        gap_counts.device_narrow = (long)device_stats.jobs_narrow; gap_counts.device_wide = (long)device_stats.jobs_wide;
        gap_counts.device_narrow_ms = device_stats.ms_narrow; gap_counts.device_wide_ms = device_stats.ms_wide;
        gap_counts.device_tall = (long)device_stats.jobs_tall; gap_counts.device_tall_ms = device_stats.ms_tall;
        gap_counts.device_long = (long)device_stats.jobs_long; gap_counts.device_long_ms = device_stats.ms_long;
        gap_counts.device_long_tall = (long)device_stats.jobs_long_tall; gap_counts.device_long_tall_ms = device_stats.ms_long_tall;
        if (!dbg) return;
        if (nj)
            fprintf(stderr, "[output] %ld gap alignments: %zu on the device (%lld narrow form in %.1f ms, %lld wide form in %.1f ms, %lld tall form in %.1f ms, %lld long form in %.1f ms, %lld long-tall form in %.1f ms, %ld declined), %.3f s of host work, longest %.3f s (gap of %u columns)\n",
                    nj, on_device, (long long)device_stats.jobs_narrow, device_stats.ms_narrow, (long long)device_stats.jobs_wide, device_stats.ms_wide, (long long)device_stats.jobs_tall, device_stats.ms_tall, (long long)device_stats.jobs_long, device_stats.ms_long, (long long)device_stats.jobs_long_tall, device_stats.ms_long_tall, declined, sum, mx, jobs[(size_t)arg].max_len);
        long ns = 0, np = 0, nt = 0;
        for (size_t z = 0; z < (size_t)nl; z++) { np += printed[z]; ns += printed[z] && slow[z]; nt += printed[z] && trimmed[z].start != a.lcbs[z].start; }
        fprintf(stderr, "[output] %ld LCBs printed: %ld streamed, %ld as strings (%ld trimmed against their predecessor); %lld MB in %zu group(s)\n", np, np - ns, ns, nt, at >> 20, ngroups);
    }
    // the steps that read what the XMFA's records left on the device or in `trimmed`: SNP files, then the tree of their distances (the
    // last engine call before it is the collector's pm_snp_distances), then the scan of their columns, then the extension
    void steps_after_xmfa() {
        tree_counts = TreeCounts();
        rec_counts = RecCounts();
        if (snp) {
            const SnpCollector::Result r = snp->finish(a.genomes, dir, stem, prm.recomb);
            if (prm.tree) write_tree(a.session(), r.names, r.dist.data(), dir, stem, prm.bootstrap, prm.bootseed);
            if (prm.recomb) write_recomb(a.session(), r.columns, RecParams{prm.recperms, prm.recseed, prm.recsites, prm.recnear}, dir, stem);
            snp->report();
            lap("snp columns");
        }
        ext_counts = ExtCounts();
        if (prm.lcbext) {      // the intervals of the records as their header lines print them: extend.cpp grows the LCBs from them
            std::vector<std::vector<ExtRecord>> ext_lcbs;
            for (size_t z = 0; z < (size_t)nl; z++) {
                if (!printed[z]) continue;
                std::vector<ExtRecord> recs;
                for (size_t i = 0; i < n; i++) { const Interval iv = printed_interval(a, trimmed[z], i); recs.push_back(ExtRecord{(int32_t)i + 1, iv.lo, iv.hi, iv.fwd, (int32_t)z + 1}); }
                ext_lcbs.push_back(std::move(recs));
            }
            const ExtSettings ext_st{prm.extmax, prm.extband, prm.extmatch, prm.extmismatch, prm.extgap, prm.extani, prm.extmin};
            write_extended(a.session(), a.genomes, printable, ext_lcbs, ext_st, dir, stem, threads);
            lap("lcb extension");
        }
    }
};

// ---- log (:1082-1190); stream flags are sticky exactly as in the reference
void write_log(std::ostream& log, const Aligner& a, const Params& prm, bool gap_note) {
    using namespace std;
    const size_t n = a.n;
    log << "Number of sequences analyzed:" << setiosflags(ios::fixed) << setprecision(1) << setw(10) << n << endl << endl;
    for (size_t i = 0; i < n; i++) {
        log << "Sequence " << i + 1 << " : " << a.genomes[i].path << endl;
        log << a.genomes[i].fname << endl;
        log << "Length:" << setw(10) << a.genomes[i].size_nopad << " bps" << endl;
        log << " GC:" << setw(10) << setiosflags(ios::fixed) << setprecision(1) << a.genomes[i].gc << endl;
        log << " AT:" << setw(10) << setiosflags(ios::fixed) << setprecision(1) << a.genomes[i].at << endl;
    }
    log << setw(2) << setiosflags(ios::left) << "d value:   " << setw(2) << prm.d << endl;
    log << setw(2) << "q value:   " << setw(2) << prm.q << endl << endl;
    log << setw(2) << "Mum anchor size:   " << setw(2) << a.l << endl;
    log << setw(2) << "Number of MUM anchors found:   " << setw(2) << a.m0 << endl;
    const long total = (long)a.mums.size() + a.filtered;
    log << setw(2) << "Number of MUMs found:   " << setw(2) << (total >= a.m0 ? total - a.m0 : 0) << endl;
    log << setw(2) << "Total MUMs found((Anchors+MUMs)-filtered):   " << setw(2) << a.mums.size() << endl << endl;
    log << setw(2) << "Random MUM length:   " << setw(2) << a.random << endl;
    log << setw(2) << "Minimum Cluster length:   " << setw(2) << prm.c << endl;
    log << setw(2) << "Number of MUMs filtered:   " << setw(2) << a.filtered << endl;
    log << setw(2) << "Number of Clusters filtered:   " << setw(2) << a.filtered_lcbs << endl << endl;
    long ccount = 0;
    for (const Lcb& c : a.lcbs) if (c.type && !c.mums.empty()) ccount++;
    log << setw(2) << "Number of clusters created:   " << setw(2) << ccount << endl;
    if (a.lcbs.empty()) log << setw(2) << "Number of clusters created:   " << setw(2) << "NONE" << endl;
    if (ccount == 0) { cerr << "parsnp_core: no clusters (the reference divides by zero here)" << endl; exit(1); }
    log << setw(2) << "Average number of MUMs per cluster:   " << setw(2) << a.mums.size() / (size_t)ccount << endl;
    vector<long> coverage(n, 0);
    long avg = 0, totcoverage = 0, totsize = 0;
    for (size_t i = 0; i < n; i++) {
        for (const Lcb& c : a.lcbs) {
            if (!c.type || c.mums.empty()) continue;
            const Mum& f = a.pool[(size_t)c.mums.front()];
            const Mum& bk = a.pool[(size_t)c.mums.back()];
            long span = f.fwd[i] ? labs((bk.start[i] + bk.length) - f.start[i]) : labs((f.start[i] + f.length) - bk.start[i]);
            coverage[i] += span;
            if (i == 0) avg += span;
        }
    }
    log << setw(2) << "Average cluster length:   " << avg / ccount << " bps" << endl;
    float percent;
    for (size_t i = 0; i < n; i++) {
        percent = (float)coverage[i] / ((float)a.genomes[i].gc + (float)a.genomes[i].at);
        log << setw(2) << "Cluster coverage in sequence " << i + 1 << ":   " << setiosflags(ios::fixed) << setprecision(1)
            << 100.00 * percent << "%" << endl;
        totcoverage += coverage[i];
        totsize += a.genomes[i].size_nopad;
    }
    percent = (float)totcoverage / (float)totsize;
    log << setw(2) << "Total coverage among all sequences:   " << setiosflags(ios::fixed) << setprecision(1) << 100.00 * percent
        << "%" << endl << endl;
    log << setw(2) << " MUM anchor search elapsed time:   " << a.anchor_time << "s " << endl;
    log << setw(2) << " MUM coarsening elapsed time:   " << a.coarsen_time << "s " << endl;
    if (prm.random) log << setw(2) << " MUM filtering elapsed time:   " << a.random_time << "s " << endl;
    log << setw(2) << " MUM clustering elapsed time:   " << a.clusters_time << "s " << endl;
    log << setw(2) << " Inter-clustering elapsed time:   " << a.iclusters_time << "s " << endl;
    log << setw(2) << " Total running time:   "
        << a.anchor_time + a.coarsen_time + a.random_time + a.clusters_time + a.iclusters_time << "s " << endl;
    if (gap_note)
        log << "NOTE: multi-column inter-MUM gaps were emitted unaligned ('-' padded); MUM and LCB coordinates are unaffected." << endl;
}
}  // namespace

void write_output(Aligner& a, const std::string& stem, bool* gap_note) {
    a.require_lists("write_output");      // (CoreRun::write: materialize() writes them)
    gap_counts = GapCounts();
    if (a.prm.do_align) std::cerr << "Writing output files & aligning LCBs..." << std::endl;
    XmfaWriter w(a, stem);
    w.open_files();
    w.plan_lcbs();
    w.list_jobs();
    w.cut_groups();
    w.pack_device_batch();
    w.lap("gap strings");
    w.reserve_file();
    w.start_device_call();
    w.host_align_rest();
    w.lap("wide gaps: host");
    w.start_snp_collection();
    for (size_t g = 0; g < w.ngroups; g++) {
        const XmfaWriter::Group& G = w.batch[g];
        w.take_group(g);
        w.stage_columns(G);
        w.stage_slow_rows(G);
        w.stage_in_order(G);
        w.stage_sizes(G);
        w.stage_write(G);
        w.stage_snps(G);
        if (w.dbg) { char what[48]; snprintf(what, sizeof what, "group %zu written", g + 1); w.lap(what); }
    }
    w.close_file();      // (first the side thread's end: nothing it refers to goes away before)
    w.gap_summary(gap_note);
    w.lap("xmfa records");
    w.steps_after_xmfa();
    write_log(w.log, a, a.prm, *gap_note);
    w.log.close();
}

// parsnp.unalign (Aligner::setUnalignableRegions, src/parsnp.cpp:2310-2381): round-robin over the genomes, each round
// emitting the next run of bases no MUM covers.  Quirks kept: the record holds end-start bases (the last base of the run is
// dropped), runs of one base are skipped, a trailing single character of the 80-column wrap is not printed, and the
// coordinates are 0-based positions of the padded in-memory genome.
//
// The reference walks the layout bit by bit, marking every run it has printed so that the next round finds the next one.  Here
// the work is split: THE RUNS (Aligner::unaligned_runs: per genome every maximal stretch of unmarked bits, the kept ones -- at
// least 2 bases -- with their index among all runs of the genome) and THE RECORDS.  Round r of the reference's loop emits run r
// of every genome that has one and keeps it (a one-base run costs its genome the round), and the loop ends after the first
// round in which the LAST genome has no run left, so the file is
//     { (r, k) : r < runs[k], r <= runs[n - 1], run r of genome k is kept }   in the order of (r, k).
// (the scan of a bitmap's words and the records: unalign.cpp)
#if defined(PARSNP_TEST_HOOKS)
namespace {
// the reference's walk, bit by bit and marking as it goes: the checker of the writer above (test hook PARSNP_UNALIGN_WALK)
void walk_unaligned(Aligner& a) {
    using namespace std;
    a.attach_layout_image();
    a.wait_layout();
    const size_t n = a.n;
    ofstream out((a.prm.outdir + "/parsnp.unalign").c_str());
    vector<long> lastpos(n, 0);
    vector<char> exhausted(n, 0);   // no unmarked base left at or after lastpos: the reference rescans to the same answer
    string rec;
    bool stop = false;
    while (!stop) {
        for (size_t k = 0; k < n; k++) {
            Bitmap& bm = a.layout[k];
            const long size = (long)bm.bits();
            long startpos = -1, endpos = -1;
            if (!exhausted[k]) {
                long m = lastpos[k];
                while (m < size && bm.get(m)) m++;
                if (m >= size) exhausted[k] = 1;
                else {
                    startpos = m;
                    while (m < size && !bm.get(m)) m++;
                    endpos = m - 1;
                    bm.set_range(startpos, m);
                    if (m < size) lastpos[k] = endpos + 1;
                }
            }
            if (startpos != endpos) {
                rec.clear();
                append_unaligned_record(rec, k, startpos, endpos, a.genomes[k]);
                out.write(rec.data(), (streamsize)rec.size());
            } else if (startpos == -1 && k == n - 1) {
                stop = true;
            }
        }
    }
    out.close();
}
}  // namespace
#endif

void write_unaligned(Aligner& a) {
    a.require_lists("write_unaligned");
    using namespace std;
    const auto t0 = chrono::steady_clock::now();
    unalign_counts = UnalignCounts();
#if defined(PARSNP_TEST_HOOKS)
    if (test_hook("PARSNP_UNALIGN_WALK")) { walk_unaligned(a); unalign_counts.s = chrono::duration<double>(chrono::steady_clock::now() - t0).count(); return; }
#endif
    UnalignRuns runs;
    a.unaligned_runs(&runs);
    ofstream out((a.prm.outdir + "/parsnp.unalign").c_str());
    write_unaligned_records(runs, a.genomes, a.prm.cores > 0 ? a.prm.cores : 1, out);
    out.close();
    for (size_t k = 0; k < a.n; k++) { unalign_counts.runs += (long)runs.all[k]; unalign_counts.kept += (long)runs.kept[k]; }
    unalign_counts.device_ms = runs.device_ms; unalign_counts.d2h_bytes = runs.d2h_bytes;
    unalign_counts.s = chrono::duration<double>(chrono::steady_clock::now() - t0).count();
}

}  // namespace parsnp
