// aligner.h -- host side of the parsnp_core replacement: everything of the reference's Aligner that sits
// AROUND the csgmum calls (the csgmum work itself runs on the GPU behind include/parsnp_mum.h).
//
// Reference map (all src/parsnp.cpp unless noted):
//   Genome / ingest()          main() FASTA loop                      :2913-3160
//   Bitmap                     mumlayout (vector<vector<bool>>)       :3181-3186
//   Mum                        TMum                                   src/TMum.cpp:8-162
//   Region                     TRegion                                src/LCR.cpp:12-58
//   Lcb                        Cluster                                src/LCB.cpp:8-57
//   Aligner::find_anchors      setInitialClusters()                   :2121-2174
//   Aligner::validate          setMums1, second half                  :1713-1841
//   Aligner::trim              trim                                   :1399-1477
//   Aligner::neighbour_region  determineRegion                        :1199-1290
//   Aligner::extend            doWork                                 :173-317
//   Aligner::filter_mums       filterRandom1                          :327-425
//   Aligner::chain             setFinalClusters()                     :2563-2719
//   Aligner::filter_lcbs       filterRandomClustersSimple1            :433-497
//   Aligner::fill_between      setInterClusterRegions                 :2389-2460
//   write_output               writeOutput                            :505-1191
#pragma once
#include <ctime>
#include <cstdint>
#include <algorithm>
#include <functional>
#include <future>
#include <iosfwd>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/parsnp_mum.h"

namespace parsnp {

// CPU seconds of the whole process since the previous call (PARSNP_DEBUG_TIMERS laps: wall time beside the work of all threads)
inline double cpu_lap_s() {
    static double last = 0;
    timespec ts;
    clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &ts);
    const double t = (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec, d = t - last;
    last = t;
    return d;
}


struct Params {
    int c = 0, d = 0, q = 0, p = 0, do_align = 0, cores = 2, random = 0;
    bool unaligned = false, recomb_filter = false, anchors_only = false, calc_mumi = false, extend_mums = false;
    bool snps = false;      // [Output] snps: core SNP columns and SNP distances beside the XMFA (snps.cpp); the reference ignores the key
    int bootstrap = 0;      // [Output] bootstrap=B: B bootstrap replicates label the tree's branches with their support (tree.cpp); implies tree
    uint64_t bootseed = 1;  // [Output] bootseed: the seed of the replicates' draws
    bool recomb = false;    // [Output] recomb: the recombination scan of the core SNP columns beside them (recomb.cpp); implies snps
    int recperms = 1000, recsites = 100, recnear = 10;      // [Output] recperms, recsites, recnear: permutations, sites of a window, H
    uint64_t recseed = 1;   // [Output] recseed: the seed of the permutations
    bool lcbext = false;    // [Output] lcbext: every printed LCB grows into its flanks, written to <stem>.xmfa.extended (extend.cpp)
    int extmax = 256, extband = 50, extmatch = 5, extmismatch = 4, extgap = 2, extani = 95, extmin = 10;      // [Output] ext*: longest flank, band, scores, per cent, shortest kept
    bool tree = false;      // [Output] tree: the neighbour-joining tree of the SNP distances beside them (tree.cpp); implies snps
    float diag_diff = 1.0f, factor = 0.0f;
    std::string anchors, mums, anchorfile, mumfile, prefix, outdir;
};

struct Genome {
    std::string path, fname, header;   // files / fasta / headers of the reference's Aligner
    std::string seq;                   // 'A','C','G','T','N' only; query contigs joined by d+10 'N'
    int size_nopad = 0;                // genome_sizes: length without the contig padding
    float gc = 0, at = 0;              // gcCount / atCount
    std::map<int, std::string> pos2hdr;
};
// returns false when the file cannot be opened; *console receives what the reference prints to stdout for this file
bool ingest(const std::string& path, bool is_ref, bool reverse, int d, Genome* out, std::string* console);

// The runs of bases no MUM covers (parsnp.unalign): per genome the maximal stretches of unmarked bits of its layout, sentinel bit
// included.  Kept are the runs of at least 2 bases, genome after genome in position order (genome k: [first[k], first[k + 1]));
// the ordinal of a run counts ALL runs of its genome before it, the one-base runs included.
struct UnalignRuns {
    std::vector<int64_t> all, kept, first;
    std::vector<int32_t> start, end, ordinal;      // end inclusive
    double device_ms = 0, d2h_bytes = 0;           // kernel time of the engine's two calls and what they sent to the host (resident route)
};

// n+1 bits per genome, bit [n] is the sentinel (parsnp.cpp:3184-3185)
class Bitmap {
public:
    void init(size_t nbits_with_sentinel);
    void init_zero_lazy(size_t nbits) {   // scratch: no sentinel; storage (and its mapped pages) is kept when the size repeats
        const size_t words = (nbits + 63) / 64 + 1;
        nbits_ = nbits;
        if (words_ == words) std::fill(w_, w_ + words_, 0); else fresh(words);
    }
    void release() { fresh(0); nbits_ = 0; }
    // a bitmap whose words live elsewhere (the layout image the engine delivers, pm_layout_image): not cleared, not owned
    void attach(uint64_t* words, size_t nwords, size_t nbits_with_sentinel) {
        decltype(own_)().swap(own_);
        w_ = words; words_ = nwords; nbits_ = nbits_with_sentinel;
        logging_ = false; log_.clear();
    }
    bool attached() const { return w_ && own_.empty(); }
    uint64_t bits64(long a, long len) const {      // marks of [a, a + len), len <= 64: bit t = base a + t (outside the bitmap: unmarked)
        uint64_t m = 0;
        for (long t = a < 0 ? -a : 0; t < len; ) {
            const long p = a + t;
            if (p >= (long)nbits_) break;
            const int lo = (int)(p & 63);
            const long span = std::min<long>(64 - lo, len - t);
            m |= ((__atomic_load_n(&w_[(size_t)p >> 6], __ATOMIC_RELAXED) >> lo) & (span == 64 ? ~0ull : ((1ull << span) - 1))) << t;      // (other threads may be marking: set_range_atomic)
            t += span;
        }
        return m;
    }
    size_t count_set() const { size_t c = 0; for (size_t i = 0; i < words_; i++) c += (size_t)__builtin_popcountll(w_[i]); return c; }
    Bitmap() = default;
    Bitmap(Bitmap&& o) noexcept { *this = std::move(o); }
    Bitmap& operator=(Bitmap&& o) noexcept {
        own_ = std::move(o.own_); w_ = o.w_; words_ = o.words_; nbits_ = o.nbits_; logging_ = o.logging_; log_ = std::move(o.log_);
        o.w_ = nullptr; o.words_ = 0; o.nbits_ = 0;
        return *this;
    }
    Bitmap(const Bitmap&) = delete;
    Bitmap& operator=(const Bitmap&) = delete;
    bool test_and_set(long a, long b) {    // [a,b) := 1; was any of it marked?  (scratch use: no undo log)
        if (a < 0) a = 0;
        if (b > (long)nbits_) b = (long)nbits_;
        bool hit = false;
        while (a < b) {
            const size_t wi = (size_t)a >> 6;
            const int lo = (int)(a & 63);
            const long span = std::min<long>(64 - lo, b - a);
            const uint64_t mask = (span == 64 ? ~0ull : ((1ull << span) - 1)) << lo;
            hit |= (w_[wi] & mask) != 0;
            w_[wi] |= mask;
            a += span;
        }
        return hit;
    }
    bool get(long i) const { return (w_[(size_t)i >> 6] >> (i & 63)) & 1; }
    void prefetch(long i) const { if (i >= 0 && (size_t)i < nbits_) __builtin_prefetch(&w_[(size_t)i >> 6], 1, 1); }
    void prefetch_read(long i) const { if (i >= 0 && (size_t)i < nbits_) __builtin_prefetch(&w_[(size_t)i >> 6], 0, 1); }
    void set_range(long a, long b) {    // [a,b) := 1
        if (a >= 0 && b <= (long)nbits_ && a < b && ((size_t)a >> 6) == ((size_t)(b - 1) >> 6)) {   // inside one word: the common case
            const size_t wi = (size_t)a >> 6;
            const long span = b - a;
            store(wi, w_[wi] | ((span == 64 ? ~0ull : ((1ull << span) - 1)) << (a & 63)));
        } else set_range_slow(a, b);
    }
    void set_range_slow(long a, long b);
    // [a,b) := 1 for a range known to lie inside the bitmap, no undo log active (the bulk marking of validate_parallel)
    void set_range_inside(long a, long b) {
        uint64_t* w = w_;
        const size_t wa = (size_t)a >> 6, wb = (size_t)(b - 1) >> 6;
        const uint64_t first = ~0ull << (a & 63), last = ~0ull >> (63 - ((b - 1) & 63));
        if (wa == wb) { w[wa] |= first & last; return; }
        w[wa] |= first;
        for (size_t i = wa + 1; i < wb; i++) w[i] = ~0ull;
        w[wb] |= last;
    }
    void set_range_atomic(long a, long b);   // [a,b) := 1 with atomic word updates: threads marking neighbouring ranges may share a word
    void clear_range_atomic(long a, long b); // [a,b) := 0, likewise (no undo log)
    void clear_range(long a, long b);   // [a,b) := 0
    long next_set(long from) const;     // smallest i >= from with bit set; the sentinel guarantees one for from <= n
    long prev_set(long from) const;     // largest i <= from with bit set, or -1
    size_t bits() const { return nbits_; }
    const uint64_t* words() const { return w_; }      // (bits() + 63) / 64 of them hold the bits; the word-wise scan of parsnp.unalign reads them
    // undo log support (speculative replay): words changed since begin_log() are restored by rollback()
    void begin_log() { logging_ = true; log_.clear(); }
    bool logging() const { return logging_; }
    bool any_set(long a, long b) const {   // any marked base in [a,b)?  (touches only the words of the range)
        if (a < 0) a = 0;
        if (b > (long)nbits_) b = (long)nbits_;
        if (a >= b) return false;
        size_t wa = (size_t)a >> 6, wb = (size_t)(b - 1) >> 6;
        uint64_t first = ~0ull << (a & 63), last = ((b & 63) == 0) ? ~0ull : ((1ull << (b & 63)) - 1);
        if (wa == wb) return (w_[wa] & first & last) != 0;
        if (w_[wa] & first) return true;
        for (size_t w = wa + 1; w < wb; w++) if (w_[w]) return true;
        return (w_[wb] & last) != 0;
    }
    void rollback();
    void end_log() { logging_ = false; log_.clear(); }
private:
    // zero-on-demand storage: calloc hands out fresh zero pages for a block this size and resize() does not write to
    // them, so a new bitmap costs nothing until its words are touched (125 MB of bitmaps per run at 200 x 5 Mb)
    template <class T> struct ZeroAlloc {
        typedef T value_type;
        ZeroAlloc() = default;
        template <class U> ZeroAlloc(const ZeroAlloc<U>&) {}
        T* allocate(size_t k) { void* p = calloc(k ? k : 1, sizeof(T)); if (!p) throw std::bad_alloc(); return (T*)p; }
        void deallocate(T* p, size_t) { free(p); }
        template <class U, class... A> void construct(U*, A&&...) {}      // storage is zero already
        template <class U> bool operator==(const ZeroAlloc<U>&) const { return true; }
        template <class U> bool operator!=(const ZeroAlloc<U>&) const { return false; }
    };
    std::vector<uint64_t, ZeroAlloc<uint64_t>> own_;
    uint64_t* w_ = nullptr;       // own_.data(), or the attached words
    size_t words_ = 0;
    void fresh(size_t words) { decltype(own_)().swap(own_); own_.resize(words); w_ = words ? own_.data() : nullptr; words_ = words; }
    size_t nbits_ = 0;
    bool logging_ = false;
    std::vector<std::pair<size_t, uint64_t>> log_;
    inline void store(size_t wi, uint64_t v) { if (logging_ && w_[wi] != v) log_.emplace_back(wi, w_[wi]); w_[wi] = v; }
};

// bump allocator with stable addresses and rewind (per-genome coordinate rows of MUMs and regions live here: at 200
// genomes the reference's three std::vector per object dominate its run time)
template <class T>
class Arena {
public:
    T* alloc(size_t n) {
        if (blocks_.empty() || off_ + n > cap_[cur_]) {
            size_t next = blocks_.empty() ? 0 : cur_ + 1;
            if (next == blocks_.size()) {
                size_t c = std::max(n, kBlock);
                blocks_.emplace_back(new T[c]);
                cap_.push_back(c);
            } else if (cap_[next] < n) {
                blocks_[next].reset(new T[n]); cap_[next] = n;
            }
            cur_ = next; off_ = 0;
        }
        T* p = blocks_[cur_].get() + off_;
        off_ += n;
        return p;
    }
    struct Mark { size_t cur, off; bool empty; };
    Mark mark() const { return Mark{cur_, off_, blocks_.empty()}; }
    void rewind(const Mark& m) { if (m.empty) { cur_ = 0; off_ = 0; } else { cur_ = m.cur; off_ = m.off; } }
    void reset() { cur_ = 0; off_ = 0; }      // start over, keeping the blocks (and their mapped pages)
private:
    static constexpr size_t kBlock = 1 << 20;
    std::vector<std::unique_ptr<T[]>> blocks_;
    std::vector<size_t> cap_;
    size_t cur_ = 0, off_ = 0;
};

// rows of n entries in Aligner's arenas.  TMum keeps start, end and a strand flag per genome as vector<long>/<bool>
// (TMum.h); end == start + length in every genome at all times (constructor TMum.cpp:25-60, trimleft/trimright
// :104-148 move start or end together with length), so only start is stored, as int32 (a genome longer than 2^31 - 1
// is refused at construction): 5 bytes per genome and MUM instead of 20 -- the host phases that walk 60 000 anchors x
// 200 genomes are bound by the bytes of these rows, not by arithmetic.
struct Mum {
    long id = 0;
    long length = 0;
    long slength = 0;
    int32_t* start = nullptr;
    uint8_t* fwd = nullptr;
    bool dirty = false;      // (anchor validation) overlapped an earlier candidate and went through the ordered pass
    bool touched = false;    // ... and was trimmed there
    int32_t row = -1;        // (resident route) its row in the engine's MUM store
    long end(size_t j) const { return (long)start[j] + length; }
};

struct Region {          // rows of n entries in Aligner's arenas; immutable once built
    long* start = nullptr;
    long* end = nullptr;
    long* length = nullptr;
    long slength = 0, llength = 0;
    bool same_as(const Region& o, size_t n) const;   // TRegion operator== (LCR.cpp:48-58)
};

struct Lcb {
    int type = 1;
    std::vector<int> mums;         // indices into Aligner::pool
    std::vector<long> start, end;
    long length = 0;
};

// raw candidate list of one finder request (one reference chunk of one region)
// (a view into the engine's result, which stays alive as long as a cache entry refers to it: nothing is copied)
struct Raw {
    const int32_t* k = nullptr; const int32_t* lon = nullptr;
    const int32_t* sp = nullptr;
    const uint8_t* fwd = nullptr;
    // MUM-row mode of the engine (pm_session_rows): rows of n entries per candidate built on the device, and their flags
    int32_t* start = nullptr; uint8_t* strand = nullptr; const uint32_t* flags = nullptr;
    bool dirty_known = false;
    size_t row0 = 0;             // this list's first candidate in the result
    size_t count = 0;
    std::shared_ptr<pm_result> owner;
};

struct Stats {   // wall-clock split reported next to the reference's own phase timers
    double anchor_s = 0, extend_s = 0, filter_s = 0, lcb_s = 0, finder_s = 0;
    double t_pack = 0;      // request rows -> the flat arrays of the C ABI
    double alg_bytes = 0;   // sum over the regions sent to the engine of (m/4 + 16 m + 16 n) per query genome
    double alg_bytes_query = 0;    // ... of which the query pieces (m/2): the one coalesced stream that reaches the fabric
    double alg_bytes_kernel = 0;   // the same sum of what THIS engine's event search must move: (m + n)/2 + 64 B per sampled K-mer (run_batch)
    double grouped_wide = 0, wide_regions = 0, handed_back = 0;   // pm_last_timing's counts of the wide grouped form, summed over the step's calls: its events, the regions it took, the small regions it handed back
    long finder_calls = 0, finder_regions = 0, regions_processed = 0, cache_hits = 0, cache_misses = 0, spec_rounds = 0;
    // device-side phase times (HIP events, pm_last_timing): summed over every engine call of the step, and of the
    // anchor call alone (the one launch that sees whole genomes)
    std::vector<std::pair<std::string, double>> engine_ms, anchor_ms;
    long generations = 0, generation_regions = 0, generation_handover = -1;   // parallel generations, regions in them, generation at which the in-order replay took over (-1: never)
    long generation_restarts = 0;   // generation-parallel extension abandoned after its second generation (see extend_generations)
    long regions_deferred = 0;      // (resident route) regions a generation left on the work list: their cluster met an earlier one in some genome, or a child sorted first
    long tie_runs = 0, tie_runs_open = 0;   // (resident route) runs of different regions with one reference start; ... of which more than one region had candidates (the route is left)
    long resident = 0;              // 1: phases A-D ran on the resident route (resident.cpp: rows, layout and regions stayed on the device)
    long chain_passed = -1;         // MUMs that neither joined nor closed a chain in the first chaining pass (diag_diff in bases); -1: no pass has run
    long device_chain = 0;          // 1: phases C-D (sort, chaining, LCB filter, fillers) came from the device in one call (pm_store_chain_*)
    long resident_retry = 0;        // 1: the resident route was left (the reference's processing order would have shown) and the step ran again on the host route
    long tie_fallbacks = 0, literal_iterations = 0, parallel_candidates = 0, parallel_dirty = 0, parallel_tangled = 0;   // work-list ties between different regions (extend_pass)
    double t_validate = 0, t_neighbour = 0, t_key = 0, t_sweep = 0, t_replay = 0, t_sort = 0, t_unpack = 0;   // host split
};

// The arenas of a run.  A caller that runs the path repeatedly (CoreRun::step) keeps one of these across runs: giving
// hundreds of MB back to the OS and faulting them in again costs more than the reset.
struct AlignerMemory {
    Arena<long> rows, cache_rows, req_rows;
    Arena<int32_t> irows;                    // MUM start rows
    Arena<uint8_t> brows;                    // MUM strand rows
    std::vector<Bitmap> layout;              // the run's mumlayout: storage kept mapped across runs, cleared per run
    bool layout_clean = false;               // `layout` holds the sentinels and nothing else: the run that used it never wrote to it (the resident route)
    std::vector<Bitmap> scratch;             // validate_parallel's scratch bitmaps (each stripe thread clears and fills its own)
    std::vector<int64_t> batch_starts, batch_lens;   // run_batch's flat request arrays
    std::vector<pm_row_info> anchor_info_store;      // resident route: the block the anchors' per-row scalars arrive in, kept between runs (1.3 MB: not zero-filled per step)
    std::vector<Mum> pool_store, candidates;         // storage of Aligner::pool / validate_parallel's candidate records between runs
    // resident route: the per-MUM and per-region vectors of a run (Aligner::mums, Resident::start0 ... below), a few MB that a step
    // fills from empty.  Their storage is lent to the run and comes back cleared with ~Aligner: freed and allocated again, blocks of
    // this size are mapped afresh and faulted in page by page in every step
    struct ResidentStore {
        std::vector<int> mums;
        std::vector<int32_t> start0, of_row, len_of_row, gen_id;
        std::vector<int64_t> found_key;
        std::vector<pm_region_info> gen_info;
        std::vector<pm_row_info> info;                // resident_extend: the scalars of the recursion's candidates, by store row (never zero-filled: a generation reads what its own call wrote)
    } resident_store;
    std::vector<int> minlen_flat[2]; std::string minlen_expr[2];   // Aligner::min_length for lengths below 2^16, by expression (mums, anchors)
    // extend_generations: a candidate with a reverse-strand member outside its region, with the marks it saw in every genome's
    // interval and what was decided (engine/store_kernels.h: ForeignRead / ForeignBound)
    struct ForeignCase {
        std::vector<int32_t> start; std::vector<uint8_t> fwd; std::vector<uint64_t> mask;
        long length, key; int uid; size_t own_before; const long* rstart; const long* rend;
        bool accepted; long acc_start0, acc_length;
    };
    struct PerThread { Arena<long> rows; Arena<int32_t> irows; Arena<uint8_t> brows; std::vector<long> scratch; std::vector<ForeignCase> foreign; };
    std::vector<std::unique_ptr<PerThread>> per_thread;   // rows written by the threads of the generation-parallel replay
    void reset() { rows.reset(); cache_rows.reset(); req_rows.reset(); irows.reset(); brows.reset(); for (auto& t : per_thread) { t->rows.reset(); t->irows.reset(); t->brows.reset(); } }
};

class Aligner {
    std::unique_ptr<AlignerMemory> own_memory_;   // when the caller did not lend one (declared first: `layout` refers into it)
    AlignerMemory* memory_;
public:
    Aligner(std::vector<Genome>& genomes, const Params& prm, pm_session* session, AlignerMemory* memory = nullptr);
    ~Aligner();
    size_t n;
    Params prm;
    std::vector<Genome>& genomes;
    std::vector<Bitmap>& layout;  // mumlayout; lives in the run's AlignerMemory
    std::vector<Mum> pool;        // every MUM ever accepted; `mums` and Lcb::mums index into it
    std::vector<int> mums;        // this->mums of the reference, in its order
    std::vector<Lcb> lcbs;        // this->clusters
    std::vector<Region> regions;  // this->regions (work list of extend())
    float l = 0;                  // anchor min length ("Mum anchor size")
    long m0 = 0, filtered = 0, filtered_lcbs = 0;
    bool unique_order = false;   // chain(): the MUM list had no two MUMs with the same reference start (one sorted order)
    int random = 0;
    float anchor_time = 0, coarsen_time = 0, random_time = 0, clusters_time = 0, iclusters_time = 0;
    Stats stats;
    bool sharded_ = false;       // (set by the owner) a rank of a sharded run: every rank makes the same engine calls in the same order, no helper thread
    // The resident route (resident.cpp): MUM rows, layout and regions stay on the device; the host keeps the list logic.
    bool resident_allowed_ = true;                       // (set by the owner) false: the run that repeats a step the route was left in
    bool announce_ = true;      // find_anchors prints its two progress lines (false: the step is being run again on the host route, they are out already)
    bool resident_active() const { return res_.active; }
    bool resident_failed() const { return res_.failed; }
    const std::string& resident_why() const { return res_.why; }
    bool resident_chain();                               // phases C-D from the device (resident.cpp); false: the caller runs them
    void materialize();                                  // rows of the LCBs' MUMs for the writer; no-op on the host route
    pm_session* session() const { return session_; }      // (the writer's SNP collection runs on it)
    void unaligned_runs(UnalignRuns* out);               // the runs parsnp.unalign lists: from the device's layout on the resident route, from `layout` otherwise
    void attach_layout_image();                          // resident route: the device's layout fetched into `layout` (the bit-by-bit checker of parsnp.unalign, a test hook)
    // After resident_chain() returned true `mums` and `lcbs` are NOT written yet: the device's answer is kept (Resident::chain_*)
    // and the step report reads its counts from summary().  final_mums() / final_lcbs() write the lists on first use; whoever
    // reads `mums` / `lcbs` of a finished run goes through them (or calls require_lists() where it takes the members directly).
    struct Summary { long mums = 0, lcbs = 0, core_bp = 0; };
    Summary summary() const;
    const std::vector<int>& final_mums() { build_lists(); return mums; }
    const std::vector<Lcb>& final_lcbs() { build_lists(); return lcbs; }
    void require_lists(const char* who) const;           // fatal when the lists of a resident chain have not been written
    long key0(int idx) const { return res_.active ? (long)res_.start0[(size_t)idx] : (long)pool[(size_t)idx].start[0]; }      // reference start of a MUM

    bool find_anchors();       // returns m0 != 0
    bool extend();             // returns !mums.empty()
    void filter_mums(int rvalue);
    void chain();
    void filter_lcbs();
    void fill_between();
    void complete_lcbs();      // the LCBs' start / end rows in every genome (host route; chain() leaves the reference column)

    Region neighbour_region(const Mum& m, bool left);
    void neighbour_into(const Mum& m, bool left, Region* out) const;   // rows of *out already allocated
    bool neighbour_if_longer(const Mum& m, bool left, long q, Region* out, long* short_j, long* short_len, long* short_stop) const;
    Region new_region();

    void wait_layout();           // the layout bitmaps are set up in the background (constructor); the first reader awaits them
    enum : uint8_t { kJoin = 0, kClose = 1, kPass = 2 };
    uint8_t judge_pair(const Mum& nt, const Mum& back) const;     // chain()'s test of a MUM against the open chain's last MUM

private:
    struct Resident {
        bool active = false, failed = false, materialized = false;
        std::string why;
        int64_t table = 0;
        std::vector<int32_t> start0;                                           // reference start of pool[i]
        std::vector<int64_t> found_key;                                        // pool[i] of the recursion: where its REGION stands in the reference's processing order (reference start, generation; -1: the first pushed seed)
        std::vector<pm_region_info> gen_info; std::vector<int32_t> gen_id;     // the seed regions, in push order
        std::vector<int32_t> fallback_start; std::vector<uint8_t> fallback_strand;   // rows fetched for the host route
        std::vector<uint64_t> image;                                           // the layout, fetched for the checker of parsnp.unalign (attach_layout_image)
        std::vector<pm_row_info> anchor_info; size_t anchor_rows = 0; const int32_t* anchor_lon = nullptr; long anchor_slength = 0; size_t anchor_accepted = 0;   // what resident_records() writes the anchors' MUM records from
        bool records_done = true;
        std::vector<int32_t> of_row, len_of_row;      // store row -> index of its MUM record in the pool (-1: none), and its length
        bool chain_queued = false;                                             // pm_store_chain_begin is in flight (resident_chain() collects it)
        // the chain's answer, kept until someone asks for the lists (rows / heads: the engine's block, valid until the session's
        // next pm_store_chain_begin -- a later step, on a later Aligner)
        bool lists_pending = false;
        pm_chain_info chain_info{}; const int32_t* chain_rows = nullptr; const uint8_t* chain_heads = nullptr;
        Summary chain_summary;
        std::string chain_why;                                                 // why phases C-D fell back to the host's list logic
    } res_;
    bool resident_try_ = false;           // run_batch: ask for resident mode (the anchor call of the route)
    bool layout_written_ = false;         // this run wrote to `layout`
    bool resident_anchors(const Region& whole, std::vector<int>* found);
    bool resident_extend();
    void resident_chain_begin(size_t expect);
    void resident_records();
    void build_lists();                   // mums / lcbs from the kept answer of the chain (no-op when they are written)
    void resident_verdicts();
    uint8_t resident_judge_rows(int cur, int back);
    void resident_fill_between();
    std::vector<std::future<void>> layout_ready_;
    // set by validate_parallel for the list it accepted into an EMPTY layout (the anchor call): in every genome the accepted
    // MUMs lie in list order, one after the other without overlap -- then the marked base next to a MUM is its list
    // neighbour's, and find_anchors() derives the seed regions from the rows instead of walking bitmaps
    bool anchors_ordered_ = false;
    std::vector<int> judged_pred_;            // chain(): predecessor against which a MUM was last judged, and the verdict
    std::vector<uint8_t> judged_verdict_;
    pm_session* session_;
    long next_id_ = 1;
    Arena<long>& rows_;      // region coordinate rows
    Arena<int32_t>& irows_;  // MUM start rows
    Arena<uint8_t>& brows_;  // MUM strand rows
    // --- finder plumbing -------------------------------------------------------------------------------------
    // one engine request = one reference chunk of one region; rows of n entries (the region's own rows when the
    // region is a single unclamped chunk, else rows in req_rows_)
    struct Request {
        const long* start; const long* len; int32_t minsize; long ref_ini; uint64_t hash; bool plain = false;   // plain: the rows are the region's own (one unclamped chunk)
    };
    void chunk_requests(const Region& r, int minsize, std::vector<Request>* out);   // the p-chunk loop, :1519-1547
    void run_batch(const std::vector<Request>& reqs, std::vector<Raw>* out, bool rows = false);   // rows: every request is its region (plain)
    void unpack_result(pm_result* res, size_t nregions, bool rows, std::vector<Raw>* out);
    int rows_mode_ = -1; bool rows_supported_ = true;     // pm_session_rows: 0 (sp, fwd), 1 MUM rows, 2 resident; -1: as an earlier run of the session left it
    bool timing_first_call_ = false;
    void collect_engine_timing();
    std::vector<std::shared_ptr<pm_result>> kept_results_;   // results whose row blocks hold the rows of accepted MUMs
    // cache of raw results keyed by request coordinates (results are a pure function of them); entries own a copy of
    // the coordinates and are compared in full on a hash hit
    struct CacheEntry { const long* start; const long* len; int32_t minsize; bool pending; Raw raw; };
    std::unordered_multimap<uint64_t, CacheEntry> cache_;
    Arena<long>& cache_rows_;
    Arena<long>& req_rows_;
    CacheEntry* cache_find(const Request& q);
    CacheEntry* cache_put(const Request& q, bool pending);
    std::unordered_map<long, int> minlen_memo_[2];
    std::vector<long> gsize_;
    // --- setMums1 ---------------------------------------------------------------------------------------------
    int min_length(bool anchors, long slength);
    // finder for one region + validate(); `speculative`: a missing cache entry is recorded in `wanted_` and the
    // region is treated as yielding nothing instead of calling the GPU.
    void region_mums(const Region& r, bool anchors, std::vector<int>* accepted, bool speculative);
    void validate(const Region& r, const Request& q, const Raw& raw, std::vector<int>* accepted);
    void validate_parallel(const Region& r, const Request& q, const Raw& raw, std::vector<int>* accepted, int threads);
    bool candidate_rows(const Region& r, const Request& q, const Raw& raw, size_t c, Mum& m, bool* ok, bool* any_reverse) const;
    bool settle(Mum& m, bool touches, bool any_reverse) const;
    bool reverse_members_spell(const Mum& m) const;      // the sequence check of settle() alone (:1791-1825)
    void trim(Mum& m) const;
    bool extend_pass(bool speculative, bool sorted_start = false);
    bool extend_generations();
    bool disjoint_clusters(const std::vector<Region>& w, std::vector<size_t>* first) const;
    void prefetch(const std::vector<Region>& gen);
    void speculate(std::vector<Region> gen);
    std::function<void(std::vector<Region>*)> remaining_;
    bool speculation_ = true;
    int sweeps_ = 0;
    long misses_since_sweep_ = 0;
    std::vector<Request> wanted_;
    std::vector<CacheEntry*> wanted_entries_;
};

// What the last write_output did with the gaps between adjacent MUMs that the reference hands to MUSCLE (PARSNP_TIMING: gap_*)
struct GapCounts {
    long jobs = 0;                 // gaps aligned
    long jobs_wide = 0;            // ... of them with a string of more than 96 bases, wherever they were aligned
    long jobs_long = 0;            // ... of them with a string of more than 320 bases (what a cluster distance above 300 brings)
    long longest = 0;              // bases of the longest gap string
    long device_narrow = 0, device_wide = 0;      // aligned by the device's narrow / wide form
    long device_tall = 0;          // ... and by its tall form (alignments of more than 512 genomes)
    long device_long = 0;          // ... and by its long form (a string of more than 320 bases)
    long device_long_tall = 0;     // ... and by its long-tall form (both: more than 512 genomes and a string of more than 320 bases)
    long host = 0;                 // aligned by the host restatement (gapalign.cpp)
    double host_s = 0;             // ... in this many seconds, summed over the threads
    double device_narrow_ms = 0, device_wide_ms = 0, device_tall_ms = 0, device_long_ms = 0, device_long_tall_ms = 0;      // kernel time of each form
};
extern GapCounts gap_counts;
// XMFA + log (writeOutput).  gap_note: set when the gap aligner (gapalign.h) declined an inter-MUM gap and it was written '-'-padded.
void write_output(Aligner& a, const std::string& stem, bool* gap_note);
// parsnp.unalign (setUnalignableRegions): the runs (Aligner::unaligned_runs), then the records; the layout is read, not written.
void write_unaligned(Aligner& a);
// the records of parsnp.unalign from the runs, in the reference's round-robin order, formatted on `threads` threads
void write_unaligned_records(const UnalignRuns& runs, const std::vector<Genome>& genomes, int threads, std::ostream& out);
// one record: header line, end - start bases in lines of 80, "=" (the quirks: write_unaligned)
void append_unaligned_record(std::string& rec, size_t k, long startpos, long endpos, const Genome& gn);
// the runs of unmarked bits in [0, nbits) of one genome's bitmap words, word by word: appends start / end / ordinal of the kept ones
// (at least 2 bases), returns the number of all runs
int64_t scan_unaligned_words(const uint64_t* w, int64_t nbits, std::vector<int32_t>* start, std::vector<int32_t>* end, std::vector<int32_t>* ordinal);
// what the last write_unaligned did (PARSNP_TIMING: unalign_*)
struct UnalignCounts { double s = 0; long runs = 0, kept = 0; double device_ms = 0, d2h_bytes = 0; };
extern UnalignCounts unalign_counts;

// Core SNP columns and SNP distances of the XMFA being written ([Output] snps=1; snps.cpp).  The writer hands over, LCB by LCB in
// print order, the columns that are not MUM columns as blocks of n rows; MUM columns are core invariant by construction and are
// only counted.  The blocks lie side by side in a staging matrix that goes to the engine (pm_snp_add) whenever it is full; after
// the last one the core SNP columns and the distances come back and are mapped to (cluster, column, reference position).
struct SnpCounts { bool on = false; long columns = 0, invariant = 0, core = 0, other = 0; double h2d_bytes = 0, scan_ms = 0, dist_ms = 0; };
extern SnpCounts snp_counts;      // what the last write_output collected (PARSNP_TIMING: snp_*, with snps=1 only)
int snp_max_rows();               // sequences a run with snps=1 may have
struct RecColumn { int32_t cluster; int64_t column, ref_pos; };      // a core SNP column as <stem>.snps.tsv prints it
class SnpCollector {
public:
    SnpCollector(pm_session* session, size_t n_rows, int threads);
    void add_invariant(long cols) { invariant_ += cols; }
    // `width` columns of the LCB printed as cluster<cluster>, the first one its column c0.  row(i, dst) writes the width characters of
    // row i (any thread).  ref_pos: the reference position of every column, or null: ref_base + the characters other than '-' of row
    // 0 to the left, inside the block.  Returns the characters other than '-' of row 0 in the block.
    long add_block(int cluster, long c0, size_t width, const std::function<void(size_t, uint8_t*)>& row, const int64_t* ref_pos, int64_t ref_base);
    // the same in steps, for many blocks at once: room for `width` columns side by side (row i at the returned pointer + i * pitch();
    // what was staged before goes to the engine first when they do not fit), which the caller fills, then a commit per block, in order
    size_t pitch() const { return pitch_; }
    uint8_t* reserve(size_t width);
    long commit(int cluster, long c0, size_t width, const int64_t* ref_pos, int64_t ref_base);
    // the three files beside the XMFA and snp_counts.  Handed back is what the steps after it need (the columns and the distances are
    // still on the device, too): the names, the n x n distances and, when asked for, every core SNP column as the .snps.tsv prints it
    struct Result { std::vector<std::string> names; std::vector<int32_t> dist; std::vector<RecColumn> columns; };
    Result finish(const std::vector<Genome>& genomes, const std::string& dir, const std::string& stem, bool want_columns);
    void report() const;      // the console line, from snp_counts (the writer prints it after those steps' lines, as ever)

private:
    struct Entry { int64_t first; int32_t cluster; int32_t width; int64_t c0; };      // columns [first, first + width) of all columns handed over
    void flush();
    pm_session* session_; size_t n_; int threads_;
    std::vector<uint8_t> stage_; size_t pitch_ = 0, used_ = 0;
    std::vector<Entry> entries_; std::vector<int64_t> ref_pos_;
    int64_t total_ = 0; long invariant_ = 0;
    pm_snp_counts counts_{0, 0, 0, 0};
    double scan_ms_ = 0, h2d_bytes_ = 0;
};

// The neighbour-joining tree of the SNP distances ([Output] tree=1; tree.cpp): the engine joins (pm_nj_tree over the
// distances the session has just computed), the host turns the join records into branch lengths and one line of Newick.
struct TreeCounts { bool on = false; double nj_ms = 0; long joins = 0; bool boot_on = false; long boot_reps = 0; double boot_ms = 0; };
extern TreeCounts tree_counts;      // what the last write_output built (PARSNP_TIMING: nj_*, with tree=1 only)
int tree_max_rows();                // sequences a run with tree=1 may have
int boot_max_reps();                // replicates a run with bootstrap=B may ask for
// the Newick line (without the newline) of n >= 3 names from the engine's records
// (support: null, or a label per join)
std::string nj_newick(const std::vector<std::string>& names, const pm_nj_join* joins, const pm_nj_last& last, const int32_t* support = nullptr);
// <stem>.snps.nwk; dist: the n x n distances on the host (read for n == 2 only: the engine is not called then)
// bootstrap > 0: then <stem>.snps.boot.nwk, the same text with the support of join t behind its node
void write_tree(pm_session* session, const std::vector<std::string>& names, const int32_t* dist, const std::string& dir, const std::string& stem,
                int bootstrap = 0, uint64_t bootseed = 1);

// The recombination scan of the core SNP columns ([Output] recomb=1; recomb.cpp): the engine flags the informative
// columns, scores the pairs of sites of every window and tests every window against its permutations (pm_rec_*); the host cuts the
// LCBs' site lists into windows and writes <stem>.rec.tsv and <stem>.rec.
struct RecParams { int perms = 1000; uint64_t seed = 1; int sites = 100; int near = 10; };
struct RecCounts { bool on = false; long sites = 0, windows = 0, flagged = 0; double ms = 0; };
extern RecCounts rec_counts;        // what the last write_output scanned (PARSNP_TIMING: rec_*, with recomb=1 only)
constexpr size_t kRecMinSites = 16; // an LCB with fewer informative sites has no window
struct RecWindow { int32_t cluster; int64_t first_column, last_column, first_ref, last_ref; int32_t sites; };
void rec_limits(int* rows, int* sites, int* perms);      // sequences, recsites and recperms a run with recomb=1 may have
std::vector<size_t> rec_window_starts(size_t m, size_t K);
// the windows in order g over the informative columns of every LCB; sites / win_off: what pm_rec_incompat takes
std::vector<RecWindow> rec_windows(const std::vector<RecColumn>& cols, const uint8_t* informative, size_t K, std::vector<int64_t>* sites, std::vector<int64_t>* win_off);
bool rec_flagged(int32_t le, int32_t perms);
std::string rec_tsv_text(const std::vector<RecWindow>& win, const int32_t* phi, const int32_t* le, int32_t perms);
std::string rec_bed_text(const std::vector<RecWindow>& win, const int32_t* le, int32_t perms, long* flagged);
void write_recomb(pm_session* session, const std::vector<RecColumn>& cols, const RecParams& prm, const std::string& dir, const std::string& stem);

// The extension of the LCB ends into their flanks ([Output] lcbext=1; extend.cpp): the host derives the covered
// stretches of every genome from the records' intervals, the two jobs of every printed LCB and a descriptor per row; the engine
// aligns, cuts and merges (pm_ext_*); the host formats the records and writes <stem>.xmfa.extended.
struct ExtSettings { int max_flank = 256, band = 50, match = 5, mismatch = 4, gap = 2, ani = 95, min_len = 10; };
struct ExtCounts { bool on = false; long jobs = 0, kept = 0, wide = 0, bases = 0; double ms = 0; };
extern ExtCounts ext_counts;        // what the last write_output extended (PARSNP_TIMING: ext_*, with lcbext=1 only)
struct ExtRecord { int32_t seq; int64_t lo, hi; bool fwd; int32_t cluster; };      // a record as its header line prints it: `> seq:lo-hi +|- cluster<cluster>`
typedef std::vector<std::vector<std::pair<int64_t, int64_t>>> ExtCovered;        // per genome the covered stretches [a, b), 0-based, ascending, merged
void ext_limits(int* rows, int* flank, int* band);      // sequences, extmax and extband a run with lcbext=1 may have
std::string ext_header_text(const std::vector<Genome>& genomes, int printable);
ExtCovered ext_covered(const std::vector<std::vector<ExtRecord>>& lcbs, const std::vector<int64_t>& lens);
pm_ext_row ext_flank(const std::string& seq, const std::vector<std::pair<int64_t, int64_t>>& cov, const ExtRecord& r, char side, int F);
std::string ext_job_text(const std::vector<ExtRecord>& recs, const pm_ext_row* rows, const int32_t* used, const uint8_t* letters, int64_t pitch, int32_t cols, char side);
void write_extended(pm_session* session, const std::vector<Genome>& genomes, int printable, const std::vector<std::vector<ExtRecord>>& lcbs, const ExtSettings& st,
                    const std::string& dir, const std::string& stem, int threads);

std::string reverse_complement(const std::string& s);   // Aligner::reversec, :1294-1393

}  // namespace parsnp
