// engine_core.h -- orchestration of one pm_multi_mum_batch call, templated on the execution backend.
// HipBackend (engine_hip.hip) = the product: HIP kernels on gfx950, one stream, HIP-event timing.
// tests/emu/ instantiates it with a sequential host backend to check the logic without a GPU (tests only).
//
// A search (run -> run_once) is a call record (SearchCall, on run_once's stack: what more than one stage reads, and every host
// landing target of the call's asynchronous downloads) handed through named stages, each a private member function:
//   plan_call -> upload_and_clear -> build_index -> count_units -> search_events { event_pass } -> order_events
//   -> mumi_tail | master_ep -> candidate_tail { tail_attempt { exchange_states, compact_sp | compact_rows } }
// A stage returns kNext, kRepeat (inside the two loops: a capacity was too small) or the value the call ends with.  run() repeats
// the whole call for the index rebuild and the suffix-array path.  The words of the counter block are named once (kCtr*), the
// store's four counters move together (store_mark / store_rewind / store_reset).
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "kernels.h"
#include "store_kernels.h"
#include "dense_kernels.h"
#include "index_kernels.h"
#include "snp_kernels.h"
#include "nj_kernels.h"
#include "boot_kernels.h"
#include "rec_kernels.h"
#include "ext_kernels.h"

namespace pm {

// Host buffers the results are downloaded into (ordinary memory).  They are recycled: a result gives its
// blocks back when it is freed, the next batch of the same shape takes them, so the steady state allocates nothing and
// touches no fresh pages.  Shared by the session and every result it handed out (a result may outlive the session).
struct HostPool {
    void* (*alloc_fn)(size_t) = nullptr;
    void (*free_fn)(void*) = nullptr;
    struct Block { void* p = nullptr; size_t cap = 0; };
    std::vector<Block> idle;
    std::mutex mu;      // results are freed by whichever thread holds them while another thread's call takes blocks
    Block take(size_t n) {
        std::lock_guard<std::mutex> lk(mu);
        size_t best = idle.size();
        for (size_t i = 0; i < idle.size(); i++)
            if (idle[i].cap >= n && (best == idle.size() || idle[i].cap < idle[best].cap)) best = i;
        if (best != idle.size() && idle[best].cap <= 2 * n + (1u << 20)) { Block b = idle[best]; idle.erase(idle.begin() + (long)best); return b; }
        Block b; b.cap = n + n / 8 + 256; b.p = alloc_fn(b.cap);
        if (!b.p) throw std::bad_alloc();
        return b;
    }
    void give(Block b) { std::lock_guard<std::mutex> lk(mu); if (b.p) idle.push_back(b); }
    ~HostPool() { for (auto& b : idle) free_fn(b.p); }
};

struct ClearJob { void* p; size_t bytes; int value; };      // backend clear_many: several clears in one launch
struct BatchResult {
    int64_t nregions = 0, total = 0;
    int nq = 0;
    std::vector<int64_t> off;
    HostPool::Block kb, lonb, spb, fwdb;     // int32 k[total], int32 lon[total], int32 sp[total*nq], uint8 fwd[total*nq]
    // a session in MUM-row mode (pm_session_rows) fills these instead of sp / fwd:
    HostPool::Block startb, strandb, flagsb; // int32 start[total*(nq+1)], uint8 strand[total*(nq+1)], uint32 flags[total]
    bool rows = false, dirty_known = false;  // dirty_known: the kRowDirty bits were computed (one-region batch with a long list)
    int64_t table_id = 0;                    // != 0: the rows of this result stay on the device as the session's anchor table = rows [0, A) of the MUM store
    int64_t store_base = -1;                 // resident mode: the result's rows are rows [store_base, store_base + total) of the session's MUM store (no start / strand blocks)
    std::shared_ptr<HostPool> pool;
    int32_t* start() const { return (int32_t*)startb.p; }
    uint8_t* strand() const { return (uint8_t*)strandb.p; }
    const uint32_t* flags() const { return (const uint32_t*)flagsb.p; }
    const int32_t* k() const { return (const int32_t*)kb.p; }
    const int32_t* lon() const { return (const int32_t*)lonb.p; }
    const int32_t* sp() const { return (const int32_t*)spb.p; }
    const uint8_t* fwd() const { return (const uint8_t*)fwdb.p; }
    void release() {
        if (pool) { pool->give(kb); pool->give(lonb); pool->give(spb); pool->give(fwdb); pool->give(startb); pool->give(strandb); pool->give(flagsb); }
        kb = lonb = spb = fwdb = startb = strandb = flagsb = HostPool::Block();
    }
    BatchResult() = default;
    BatchResult(const BatchResult&) = delete;
    BatchResult& operator=(const BatchResult&) = delete;
    ~BatchResult() { release(); }
};

struct PhaseTime { const char* name; float ms; };

// Sharded run: the query genomes are split into contiguous blocks, one per rank/GPU; every rank holds the
// reference.  The two exchange steps of a batch go through these callbacks (host buffers; the embedding process
// implements them with torch.distributed -- RCCL on GPUs, gloo in tests).  Return 0 on success.
struct Collectives {
    int rank = 0, world = 1;
    int (*allreduce_min_i32)(void* ctx, int32_t* buf, int64_t count) = nullptr;
    int (*allgather)(void* ctx, const void* send, int64_t send_bytes, void* recv) = nullptr;   // recv: world * send_bytes
    void* ctx = nullptr;
    // device collectives (pm_session_create_rccl): the backend owns an RCCL communicator and the exchanges run on device
    // buffers on the engine's stream; the callbacks above are not used then
    bool device = false;
};

inline int bits_for(uint64_t v) { int b = 1; while (b < 64 && (v >> b)) b++; return b; }

template <class B>
class Engine {
public:
    explicit Engine(B& backend) : be(backend), pool(std::make_shared<HostPool>()) { pool->alloc_fn = &B::host_alloc; pool->free_fn = &B::host_free; }
    std::shared_ptr<HostPool> pool;
    ~Engine() { release(); }

    std::string error;
    std::vector<PhaseTime> timing;
    int64_t last_events = 0, last_candidates = 0, last_rest = 0, last_positions = 0, last_accepted = 0;
    double last_alg[3] = {0, 0, 0};      // last search of store regions: SURVEY 8d bytes, this engine's bytes, query-stream bytes (AlgBytes)
    uint64_t alg_raw[3] = {0, 0, 0};
    uint64_t alg_sets[8 * kAlgSets] = {};

    int ngen = 0;
    bool want_rows = false;           // pm_session_rows: results as MUM rows (start, strand, flags) instead of (sp, fwd)
    std::vector<int64_t> glen_h;
    Collectives coll;                 // world == 1: not sharded
    int g_first = 1, g_last = 1;      // query genomes [g_first, g_last) are resident on this GPU
    void set_shard(const Collectives& c) { coll = c; }
    // contiguous split of the n-1 query genomes over the ranks
    static void shard_range(int n, int rank, int world, int* first, int* last) {
        int q = n - 1;
        *first = 1 + (int)((int64_t)q * rank / world);
        *last = 1 + (int)((int64_t)q * (rank + 1) / world);
    }

    // ---- genomes -> packed strands in device memory
    int load_genomes(int n, const uint8_t* const* seqs, const int64_t* lens) {
        const bool dbg = getenv("PARSNP_DEBUG_TIMERS") != nullptr;
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        double tl = now();
        auto lap = [&](const char* what) { if (dbg) { be.sync(); const double t = now(); fprintf(stderr, "[upload] %-14s %.4f s\n", what, t - tl); tl = t; } };
        ngen = n;
        glen_h.assign(lens, lens + n);
        shard_range(n, coll.rank, coll.world, &g_first, &g_last);
        // every rank of a sharded run keeps ALL genomes resident (one byte per base and strand: 57 000 5-Mb genomes fit one GPU):
        // the SEARCH is what is sharded -- a rank streams the query genomes of its block only (CountUnits, SmallPairEvents,
        // MasterEP) -- while the resident route's validation checks reverse-strand members of any genome against the sequence
        auto resident = [&](int) { return true; };
        std::vector<int64_t> goff(2 * (size_t)n);
        int64_t words = 2;                       // leading guard (64 bases)
        int64_t maxlen = 0;
        for (int g = 0; g < n; g++) {
            if (!resident(g)) { goff[2 * (size_t)g] = goff[2 * (size_t)g + 1] = 64; continue; }   // never read
            maxlen = std::max(maxlen, lens[g]);
            for (int s = 0; s < 2; s++) {
                goff[2 * (size_t)g + s] = words * 32;
                words += (lens[g] + 31) / 32 + 2;   // + trailing guard
            }
        }
        words += 8;                              // SmallPairEvents reads a 128-base window + 2 blocks from any position of the last strand
        blk = (SeqBlock*)be.alloc((size_t)words * sizeof(SeqBlock));
        d_goff = (int64_t*)be.alloc(sizeof(int64_t) * 2 * (size_t)n);
        d_glen = (int64_t*)be.alloc(sizeof(int64_t) * (size_t)n);
        if (!blk || !d_goff || !d_glen) { error = "device allocation failed (genomes)"; return -3; }
        lap("allocate");
        be.memset(blk, 0, (size_t)words * sizeof(SeqBlock));
        be.h2d(d_goff, goff.data(), sizeof(int64_t) * goff.size());
        be.h2d(d_glen, lens, sizeof(int64_t) * (size_t)n);
        // ASCII genomes -> packed strands: a few host threads copy the genomes into page-locked staging slots, each slot's
        // DMA and its two PackStrand launches run on the slot's own stream while the next genome is being staged
        // (the genomes arrive in ordinary memory, from which a direct copy is staged by the runtime at ~6 GB/s)
        std::vector<char> res((size_t)n, 0);
        for (int g = 0; g < n; g++) res[(size_t)g] = resident(g) && lens[g] > 0;
        lap("clear + tables");
        if (!be.stage_genomes(n, seqs, lens, res, goff, blk, maxlen)) { error = "genome upload failed: " + be.error(); return -3; }
        lap("stage + pack");
        P = Packed{blk, d_goff, d_glen};
        return 0;
    }

    // ---- one batch of regions (include/parsnp_mum.h: pm_multi_mum_batch)
    // Host round trips of one call: the event counters (+ error word), the candidate count, the accepted count and the
    // result download.  Everything else the device needs from the host (region table, prefix arrays, request rows) is
    // assembled in ONE page-locked block and sent by asynchronous copies on the engine's stream.
    std::vector<int64_t> mumi_covered;   // result of run(..., mumi = true): per query genome
    // A batch whose repeat structure exhausts the per-thread work budget (a tandem repeat of period > 1 with thousands of
    // copies inside ONE region: every copy's K-mer chain is walked by every sample that hits it) is run again.  The walk that
    // ran out flagged its region (dense[]); in the second run the flagged regions take the suffix-array path
    // (dense_kernels.h: rep' and the queued samples' events, at a cost independent of the copy number), every other region
    // walks as before.  In a sharded run the verdict is common to all ranks (it travels with the first exchange), so every
    // rank repeats the batch together, each with its own flags (the suffix array gives what a walk gives wherever one ends).
    // A walk that runs out in the second run still fails the call (PM_ELIMIT); it cannot: the flagged regions do not walk.
    // Requests whose rows are regions of the session's region store (resident route): the host holds their reference columns only.
    struct GapBatch {
        const int64_t* ref_start = nullptr; const int64_t* ref_len = nullptr;   // [nreg]: the reference column of every region (sizes the index)
        const int32_t* store_ids = nullptr;                                      // [nreg]: the regions
    };
    int run(int64_t nreg, const int64_t* starts, const int64_t* lens, const int32_t* minsize, BatchResult* out, bool want_events = false,
            bool mumi = false, const GapBatch* gb = nullptr) {
        budget_exceeded = false;
        dense_mode = false; dense_h.clear(); last_dense_regions = 0; last_dense_overrun_ms = -1;      // (nothing of the path outlives a call)
        const int64_t ordinal = call_ordinal;
        if (dense_all && nreg > 0) { dense_h.assign((size_t)nreg, 1); dense_mode = true; }
        const auto t0 = std::chrono::steady_clock::now();
        index_rebuild = false;
        auto once = [&] {
            int rc = run_once(nreg, starts, lens, minsize, out, want_events, mumi, gb);
            if (rc == kIndexRebuild) {      // the overflow list of the bucket build was full: the same call, every region built by IndexInsert
                (void)be.collect();
                call_ordinal = ordinal;
                index_rebuild = true;
                rc = run_once(nreg, starts, lens, minsize, out, want_events, mumi, gb);
            }
            return rc;
        };
        int rc = once();
        if (rc == -5 && budget_exceeded && !dense_mode) {
            budget_retries++;
            last_dense_overrun_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            // the flags of the pass that ran out: one download of nreg bytes, on this path only
            dense_h.resize((size_t)nreg);
            be.d2h(dense_h.data(), d_dense.p, (size_t)nreg);
            (void)be.collect();          // (that pass's phases are not the second run's)
            call_ordinal = ordinal;      // (the same call of the step: the same capacities)
            dense_mode = true; budget_exceeded = false;
            rc = once();
        }
        dense_mode = false; index_rebuild = false;
        return rc;
    }
    bool dense_all = false;             // pm_session_tune "dense_all": every region of every batch takes the suffix-array path (tests)
    int64_t last_dense_regions = 0;     // regions of the last call that took the suffix-array path
    float last_dense_overrun_ms = -1;   // ... and the time of the pass that ran out of budget before it (-1: none)
    int dense_rounds = 0;               // prefix-doubling rounds of the last suffix-array build
    int64_t anchor_table_id = 0, anchor_table_rows = 0;      // the anchor table: rows of the last long one-region call in row mode = rows [0, A) of the MUM store
    bool budget_exceeded = false;
    long budget_retries = 0;
    static constexpr int kIndexRebuild = -99;      // run_once: the bucket build's overflow list was full (never leaves run())
    bool index_rebuild = false;                    // this run of the batch builds every region with IndexInsert
    int64_t index_overflow_seen = 0;               // ... after a bucket build that left this many overflow records

    // The counter block of a search (d_counter): kSlices event counters one 64-byte line apart, then these words.  It is cleared and
    // read back as a whole (round trip 1).
    static constexpr size_t kCtrBase = (size_t)kSlices * kSliceStride;
    static constexpr size_t kCtrErr = kCtrBase;             // the error word of the batch (kErr*)
    static constexpr size_t kCtrGrouped = kCtrBase + 2;     // the block counter of the grouped events
    static constexpr size_t kCtrWide = kCtrBase + 3;        // the wide form's kCtrWideWords counts: events, regions handed back, regions taken
    static constexpr size_t kCtrWideWords = 3;
    static constexpr size_t kCtrOverflow = kCtrBase + 6;    // overflow records of the index's bucket build
    static constexpr size_t kCtrLost = kCtrBase + 7;        // IndexVerify's count
    static constexpr size_t kCtrWords = kCtrBase + 8;       // the block's size
    static_assert(kCtrErr < kCtrGrouped && kCtrGrouped < kCtrWide && kCtrWide + kCtrWideWords <= kCtrOverflow && kCtrOverflow < kCtrLost && kCtrLost < kCtrWords,
                  "the words of the counter block are distinct and inside it");

private:
    // what call number `i` of the last step needed (i = 0: the anchor call; then the searches of store regions in their order): the
    // capacities call i of this step launches over instead of waiting for its counts
    struct CallHint { int64_t units = 0, ncand = 0, nok = 0; };
    // the four counters of the MUM store and the region store that a search may move, as one thing: store_mark() before the tail
    // of a call writes rows, store_rewind() when that tail is repeated, store_reset() when an anchor call begins a new store
    struct StoreCounts { int64_t ms_count, rg_count, layout_rows, rg_pkey_init; };
    StoreCounts store_mark() const { return StoreCounts{ms_count, rg_count, layout_rows, rg_pkey_init}; }
    void store_rewind(const StoreCounts& m) { ms_count = m.ms_count; rg_count = m.rg_count; layout_rows = m.layout_rows; rg_pkey_init = m.rg_pkey_init; }
    void store_reset() { store_rewind(StoreCounts{0, 0, -1, 0}); }      // (a new region store: none of its regions has been processed)

    // One search call (run_once): what more than one of its stages reads.  It lives on run_once's stack for the whole call, and EVERY
    // host landing target of an asynchronous download of the call is a member of it (the last group; alg_sets is the engine's own):
    // however a stage returns between a d2h_async and the wait that fills its target, the target outlives that wait.
    struct SearchCall {
        // the arguments
        const int64_t nreg; const int64_t* const starts; const int64_t* const lens; const int32_t* const minsize; BatchResult* const out;
        const bool want_events, mumi; const GapBatch* const gb;
        bool from_store = false;      // the rows are regions of the region store: the host never sees them
        // geometry (plan_call; nwv and d_err: upload_and_clear)
        int nq = 0, no_small = 0, lbits = 0;
        size_t nrow = 0, regz = 0, bytes_R = 0, bytes_pre = 0;
        int64_t npairs = 0, npos = 0, tsize = 0, fwords = 0, tsize_clear = 0, fwords_clear = 0, nbk = 0, npos_bucketed = 0, nchunks = 0, centries = 0, nwv = 0;
        // the page-locked parameter block  [ RegionInfo x nreg | posbase | cbase | starts rows | lens rows ], the first bucket of every region
        RegionInfo* R = nullptr; int64_t *posbase = nullptr, *cbase = nullptr, *stage = nullptr;
        std::vector<int64_t> bbase;
        uint32_t* d_err = nullptr;        // the error word of the counter block
        // index: regions flagged for the suffix-array path, capacity of the bucket build's overflow list, its counts were read
        int64_t nflag = 0; uint64_t ovf_cap = 0; bool index_counts_read = false;
        // event search: the hints of this call of the step, capacities and live counts
        CallHint none; CallHint* hint = nullptr;
        int64_t nunits = 0; bool units_known = false;
        size_t ev_guess = 0, slice_cap = 0, queue_cap = 0, grp_cap = 0;
        uint64_t nev = 0, nrest = 0, ngrp = 0, worst_slice = 0;
        uint32_t errbits = 0, sticky = 0;
        bool first_form = false, wide_form = false, grouping = false, by_buckets = false, coarse_by_buckets = false, sharded = false;
        uint64_t *skey = nullptr, *sval = nullptr;      // the events in order
        // candidate tail: where the device keeps the candidate count; the call looks like an anchor call
        const int64_t* ncand_p = nullptr; bool anchor_guess = false;
        // ... and its current attempt: counts waited for (exact) or capacities, where the device keeps the accepted count
        bool exact = false, anchor_call = false;
        int64_t ncand_i = 0, nok = 0; uint64_t ncand = 0; size_t nokz = 0; const int64_t* nok_p = nullptr;
        // landing targets of asynchronous downloads
        std::vector<uint64_t> counts, qcounts; int64_t nunits_live = 0;      // search_events: round trip 1
        int32_t verdict = 0;                                                  // master_ep: read with the candidate count
        std::vector<int32_t> reg_h; int64_t counts_h[2] = {0, 0};             // candidate_tail: round trip 4
    };
    // what a stage returns: a value <= 0 ends the call with it (0: done, nothing more to do; < 0: an error code), else
    static constexpr int kNext = 1, kRepeat = 2;      // go on with the next stage; the stage's loop goes round again

    // The stages, in order: plan_call (host only), upload_and_clear, build_index, count_units (waits for the unit count unless a hint
    // stands in), search_events (round trip 1, once per pass), order_events, then mumi_tail (waits, ends the call) or master_ep and
    // candidate_tail (round trips 2-4; with fast_tail the last one only).
    int run_once(int64_t nreg, const int64_t* starts, const int64_t* lens, const int32_t* minsize, BatchResult* out, bool want_events,
                 bool mumi, const GapBatch* gb = nullptr) {
        SearchCall c{nreg, starts, lens, minsize, out, want_events, mumi, gb};
        int rc = plan_call(c);
        if (rc != kNext) return rc;
        upload_and_clear(c);
        if ((rc = build_index(c)) != kNext) return rc;
        if ((rc = count_units(c)) != kNext) return rc;
        if ((rc = search_events(c)) != kNext) return rc;
        order_events(c);
        if (mumi) return mumi_tail(c);
        if ((rc = master_ep(c)) != kNext) return rc;
        return candidate_tail(c);
    }

    int plan_call(SearchCall& c) {
        const int64_t nreg = c.nreg; const int64_t* const starts = c.starts; const int64_t* const lens = c.lens; const int32_t* const minsize = c.minsize;
        BatchResult* const out = c.out; const GapBatch* const gb = c.gb;
        timing.clear();
        const int nq = c.nq = ngen - 1;
        out->nregions = nreg; out->nq = nq; out->total = 0;
        out->off.assign((size_t)nreg + 1, 0);
        out->release();
        out->pool = pool;
        if (nreg == 0) return 0;
        if (nq < 1) { error = "need at least one query genome"; return -2; }
        const int no_small = c.no_small = c.mumi ? 1 : 0;

        // -- host: the page-locked parameter block  [ RegionInfo x nreg | posbase | cbase | starts rows | lens rows ]
        // (regions of the region store: the rows part holds their ids only)
        const size_t nrow = c.nrow = (size_t)nreg * (size_t)ngen;
        const size_t regz = c.regz = (size_t)nreg;
        const size_t bytes_R = c.bytes_R = sizeof(RegionInfo) * regz, bytes_pre = c.bytes_pre = 8 * (regz + 1);
        const bool from_store = c.from_store = gb && gb->store_ids;
        if (gb && !from_store) { error = "bad region list"; return -2; }
        const size_t nrow_staged = gb ? 0 : nrow;
        uint8_t* block = (uint8_t*)be.staging(bytes_R + 2 * bytes_pre + 16 * nrow_staged + (gb ? 4 * regz : 0) + 64);
        if (!block) { error = "cannot allocate the request staging block"; return -3; }
        RegionInfo* R = c.R = (RegionInfo*)block;
        int64_t* posbase = c.posbase = (int64_t*)(block + bytes_R);
        int64_t* cbase = c.cbase = posbase + regz + 1;
        int64_t* stage = c.stage = cbase + regz + 1;
        std::vector<size_t> guess_r(regz, 0);
        std::vector<int64_t> units_r(regz, 0);
        if (from_store) {
            for (int64_t r = 0; r < nreg; r++) {
                if (gb->store_ids[r] < 0 || gb->store_ids[r] >= rg_count) { error = "region outside the region store"; return -2; }
                if (gb->ref_start[r] < 0 || gb->ref_len[r] < 0 || gb->ref_start[r] + gb->ref_len[r] > glen_h[0]) { error = "region outside its genome"; return -2; }
                if (gb->ref_len[r] >= (1ll << 31)) { error = "region longer than 2^31"; return -5; }
            }
            memcpy(stage, gb->store_ids, sizeof(int32_t) * regz);
        } else {
            // the request rows (2 x 8 bytes per region and genome: 26 MB for a recursion batch of 8 000 regions x 201) are
            // checked and copied by a few threads; the same pass counts the SeedExtend work units of every region (what
            // CountUnits computes on the device) so that the grid size needs no read-back
            const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(8, nreg / 512));
            std::vector<int> bad((size_t)nt, 0);
            auto part = [&](int t) {
                const int64_t r0 = nreg * t / nt, r1 = nreg * (t + 1) / nt;
                for (int64_t r = r0; r < r1; r++) {
                    const int64_t* st = starts + r * ngen; const int64_t* ln = lens + r * ngen;
                    const int minlen = minsize[r] < 1 ? 1 : minsize[r];
                    const int div = std::max(8, minlen);
                    const int K = minlen < kMaxK ? minlen : kMaxK, stride = minlen - K + 1;
                    const int64_t nR = ln[0];
                    size_t gs = 0;
                    int64_t units = 0;
                    int b = 0;
                    for (int g = 0; g < ngen; g++) {
                        if (st[g] < 0 || ln[g] < 0 || st[g] + ln[g] > glen_h[(size_t)g]) b |= 1;
                        if (ln[g] >= (1ll << 31)) b |= 2;
                        if (!g) continue;
                        gs += (size_t)(2 * ln[g] / div);
                        int64_t ns = (ln[g] >= K && nR >= K && g >= g_first && g < g_last) ? (ln[g] - K) / stride + 1 : 0;
                        if (small_pair(nR, ln[g]) && !no_small) ns = 0;
                        units += (ns + kUnitSamples - 1) / kUnitSamples;
                    }
                    guess_r[(size_t)r] = gs; units_r[(size_t)r] = units;
                    bad[(size_t)t] |= b;
                    memcpy(stage + r * ngen, st, sizeof(int64_t) * (size_t)ngen);
                    memcpy(stage + nrow + r * ngen, ln, sizeof(int64_t) * (size_t)ngen);
                }
            };
            if (nt == 1) part(0);
            else {
                std::vector<std::thread> th;
                for (int t = 1; t < nt; t++) th.emplace_back(part, t);
                part(0);
                for (auto& x : th) x.join();
            }
            int b = 0;
            for (int x : bad) b |= x;
            if (b & 1) { error = "region outside its genome"; return -2; }
            if (b & 2) { error = "region longer than 2^31"; return -5; }
        }
        int64_t &npos = c.npos, &tsize = c.tsize, &fwords = c.fwords, &nunits = c.nunits;      // (all 0)
        int64_t tsize_b = 0, fwords_b = 0, &nbk = c.nbk, &npos_bucketed = c.npos_bucketed;     // of the regions built by buckets: slots, filter words, buckets, positions
        std::vector<int64_t>& bbase = c.bbase;                                                 // first bucket of every region
        bbase.assign(regz + 1, 0);
        const bool by_index_buckets = index_build && !index_rebuild;
        int32_t max_nr = 1;
        size_t& ev_guess = c.ev_guess = 1 << 16;     // first-call event buffer: a match of length >= minsize every max(8,minsize) bases is generous
        cbase[0] = 0;
        for (int64_t r = 0; r < nreg; r++) {
            RegionInfo& ri = R[(size_t)r];
            ri.ref_pos = gb ? gb->ref_start[r] : starts[r * ngen];
            ri.nR = (int32_t)(gb ? gb->ref_len[r] : lens[r * ngen]);
            ri.minsize = minsize[r];
            ri.minlen = minsize[r] < 1 ? 1 : minsize[r];
            ri.K = ri.minlen < kMaxK ? ri.minlen : kMaxK;
            ri.stride = ri.minlen - ri.K + 1;
            int64_t slots = 16;
            while (slots < slot_factor * (int64_t)ri.nR) slots <<= 1;   // load factor <= 1 / slot_factor (x2: the next power of two)
            ri.tmask = (uint32_t)(slots - 1);
            int64_t fbits = 64;
            while (fbits < filter_factor * (int64_t)ri.nR) fbits <<= 1;
            ri.fmask = (uint32_t)(fbits - 1);
            // built by buckets (index_kernels.h): a table of index_bucket_min slots or more, in buckets of at most kBucketSlots slots
            // (two buckets at least), if a bucket's piece of the filter is a 32-bit word or more and fits the wavefront's LDS
            const int ls = bits_for((uint64_t)slots) - 1, lf = bits_for((uint64_t)fbits) - 1;
            const int sb = std::min(kBucketBits, ls - 1), fb = lf - (ls - sb);
            const bool bucketed = by_index_buckets && slots >= index_bucket_min && fb >= 5 && fb <= kBucketFilterBits;
            ri.pad_ = bucketed ? (uint32_t)sb | ((uint32_t)fb << 8) | kBucketed : (uint32_t)ls | ((uint32_t)std::min(lf, 29) << 8);
            bbase[(size_t)r] = nbk;
            if (bucketed) { nbk += slots >> sb; npos_bucketed += ri.nR; }
            // the slices of the bucketed regions lie behind the others': the build writes them whole, only the others are cleared
            ri.tbase = bucketed ? -1 - tsize_b : tsize; (bucketed ? tsize_b : tsize) += slots;
            ri.fbase = bucketed ? -1 - fwords_b : fwords; (bucketed ? fwords_b : fwords) += fbits / 32;
            ri.posbase = npos; posbase[(size_t)r] = npos; npos += ri.nR;
            cbase[(size_t)r + 1] = cbase[(size_t)r] + (((int64_t)ri.nR + kChunkPos - 1) >> kCoarseShift) + 1;
            max_nr = std::max(max_nr, ri.nR);
            ev_guess += guess_r[(size_t)r];
            nunits += units_r[(size_t)r];
        }
        posbase[regz] = npos;
        bbase[regz] = nbk;
        const int64_t tsize_clear = c.tsize_clear = tsize, fwords_clear = c.fwords_clear = fwords;
        for (int64_t r = 0; r < nreg; r++) {
            RegionInfo& ri = R[(size_t)r];
            if (ri.tbase < 0) { ri.tbase = tsize_clear + (-1 - ri.tbase); ri.fbase = fwords_clear + (-1 - ri.fbase); }
        }
        tsize += tsize_b; fwords += fwords_b;
        reset_call_counts();      // (last_events and last_rest stand until the event search of this call has counted)
        last_index_bucketed = npos_bucketed; last_index_overflow = index_rebuild ? index_overflow_seen : 0;
        last_positions = npos;
        const int64_t npairs = c.npairs = nreg * nq;
        c.nchunks = cbase[regz] - nreg;                  // 256-position chunks of the batch
        const int64_t centries = c.centries = cbase[regz] * nq;
        const int lbits = c.lbits = bits_for((uint64_t)max_nr);
        if (bits_for((uint64_t)npairs) + lbits + 1 > 64) { error = "batch too large for 64-bit event keys"; return -5; }
        if (npairs >= (1ll << 31) || nreg >= (1ll << 31)) { error = "too many regions in one batch"; return -5; }
        if (nunits >= (1ll << 31)) { error = "too many work units in one batch"; return -5; }
        if (centries >= (1ll << 31)) { error = "coarse event index too large"; return -5; }
        return kNext;
    }

    void upload_and_clear(SearchCall& c) {
        const int64_t nreg = c.nreg, npos = c.npos, tsize = c.tsize, fwords = c.fwords, tsize_clear = c.tsize_clear, fwords_clear = c.fwords_clear, npairs = c.npairs, centries = c.centries;
        const int nq = c.nq;
        const size_t nrow = c.nrow, regz = c.regz, bytes_R = c.bytes_R, bytes_pre = c.bytes_pre;
        const GapBatch* const gb = c.gb; const bool from_store = c.from_store;
        RegionInfo* const R = c.R; int64_t* const posbase = c.posbase; int64_t* const cbase = c.cbase; int64_t* const stage = c.stage;
        be.mark("setup");
        ensure(d_R, regz);
        ensure(d_starts, nrow); ensure(d_lens, nrow);
        ensure(d_posbase, regz + 1); ensure(d_cbase, regz + 1);
        be.h2d_staged(d_R.p, R, bytes_R);
        be.h2d_staged(d_posbase.p, posbase, bytes_pre);
        be.h2d_staged(d_cbase.p, cbase, bytes_pre);
        if (!gb) {
            be.h2d_staged(d_starts.p, stage, sizeof(int64_t) * nrow);
            be.h2d_staged(d_lens.p, stage + nrow, sizeof(int64_t) * nrow);
        } else if (from_store) {
            ensure(d_list, regz);
            be.h2d_staged(d_list.p, stage, sizeof(int32_t) * regz);
            be.launch("gather_regions", (int64_t)nrow, GatherRegions{d_list.p, ngen, d_rg_start.p, d_rg_len.p, d_starts.p, d_lens.p});
        }
        // event counters: kSlices counters one 64-byte line apart, then the error word of the batch (read back together)
        ensure(d_counter, kCtrWords);
        uint32_t* d_err = c.d_err = (uint32_t*)(d_counter.p + kCtrErr);

        // -- reference index + repeat lengths
        ensure(d_slots, (size_t)tsize); ensure(d_filter, (size_t)fwords);
        ensure(d_next, (size_t)std::max<int64_t>(npos, 1)); ensure(d_rep, (size_t)std::max<int64_t>(npos, 1));
        ensure(d_epm, (size_t)std::max<int64_t>(npos, 1) + 1);     // + the verdict word of a sharded run
        // everything the call clears before it starts, in one launch: presence filter, slots (0xff = empty), event counters + error
        // word, the repeated-K-mer bits, the coarse index, the closing words of the two prefix scans, the byte counters
        const int64_t nwv = c.nwv = (npos + 63) / 64;
        ensure(d_repeated, (size_t)(npos / 32 + 2));       // (SeedExtend reads the word after a position's own)
        ensure(d_ucount, (size_t)npairs + 1); ensure(d_uoff, (size_t)npairs + 1);
        ensure(d_coarse, (size_t)std::max<int64_t>(centries, 1));
        // (a call whose events go through the buckets writes every entry of the coarse index -- CoarseFromBuckets, zeros for the pairs
        // without a bucketed event -- so the 16 MB of an anchor call are not cleared first; order_events clears them if no event came)
        c.coarse_by_buckets = bucket_sort && (int64_t)c.nq * c.nchunks < ((int64_t)1 << 31);
        ensure(d_wmask, (size_t)nwv + 1); ensure(d_wcount, (size_t)nwv + 1); ensure(d_woff, (size_t)nwv + 1);
        if (from_store) ensure(d_alg, 8 * (size_t)kAlgSets);
        ensure(d_dense, regz);
        {
            // (the regions' dense flags as well -- but in the suffix-array run, which sets them from the host below)
            const ClearJob jobs[] = {
                {d_filter.p, sizeof(uint32_t) * (size_t)fwords_clear, 0}, {d_slots.p, sizeof(uint64_t) * (size_t)tsize_clear, 0xff}, {d_counter.p, 8 * kCtrWords, 0},
                {d_repeated.p, 4 * (size_t)(npos / 32 + 2), 0}, {c.coarse_by_buckets ? nullptr : d_coarse.p, c.coarse_by_buckets ? 0 : 4 * (size_t)std::max<int64_t>(centries, 1), 0},
                {d_ucount.p + npairs, 8, 0}, {d_wcount.p + nwv, 8, 0}, {from_store ? d_alg.p : nullptr, from_store ? (size_t)64 * kAlgSets : 0, 0},
                {dense_mode ? nullptr : d_dense.p, dense_mode ? 0 : regz, 0}};
            be.clear_many(jobs, (int)(sizeof jobs / sizeof jobs[0]));
        }
        int64_t& nflag = c.nflag;      // the suffix-array run: regions flagged (by the pass that ran out of budget, or all: dense_all)
        if (dense_mode) {
            for (int64_t r = 0; r < nreg; r++) nflag += dense_h[(size_t)r] ? 1 : 0;
            be.h2d(d_dense.p, dense_h.data(), regz);
            last_dense_regions = nflag;
        }
        // rows the device derived itself (gaps of the anchor table, rows of the region store) were never seen by the host: the
        // same checks the explicit rows get above, raised through the batch's error word
        if (gb) be.launch("check_rows", (int64_t)nrow, CheckRows{d_R.p, d_starts.p, d_lens.p, ngen, d_glen, d_err});
        if (from_store) {      // the algorithmic bytes of a search whose rows the host never saw (read back with the event counters)
            be.launch_wave("alg_bytes", (nreg * nq + kAlgPairs - 1) / kAlgPairs, AlgBytes{d_R.p, d_lens.p, ngen, nreg * nq, d_alg.p});
        }
    }

    int build_index(SearchCall& c) {
        const int64_t nreg = c.nreg, npos = c.npos, nbk = c.nbk, npos_bucketed = c.npos_bucketed, nflag = c.nflag;
        const size_t regz = c.regz;
        const RegionInfo* const R = c.R; const std::vector<int64_t>& bbase = c.bbase; uint32_t* const d_err = c.d_err;
        be.mark("index");
        const uint64_t ovf_cap = c.ovf_cap = nbk > 0 ? (uint64_t)(index_overflow_cap > 0 ? index_overflow_cap : npos_bucketed / 32 + 1024) : 0;
        if (nbk > 0) {
            // the bucketed regions (index_kernels.h): keys, sorted by bucket, a wavefront per bucket, then the overflow records
            const int pbits = bits_for((uint64_t)npos), bbits = bits_for((uint64_t)nbk);
            if (pbits + bbits > 64) { error = "batch too large for 64-bit index keys"; return -5; }
            ensure(d_bkbase, regz + 1); ensure(d_ikey, (size_t)npos); ensure(d_ikey2, (size_t)npos); ensure(d_bkbegin, (size_t)nbk + 1); ensure(d_ovf, (size_t)ovf_cap);
            be.h2d(d_bkbase.p, bbase.data(), 8 * (regz + 1));
            be.launch("index_keys", npos, IndexKeys{P, d_R.p, nreg, d_posbase.p, d_bkbase.p, pbits, d_ikey.p, d_next.p, d_rep.p});
            if (!sort_keys_on(be, d_ikey.p, d_ikey2.p, (size_t)npos, pbits, pbits + bbits, 0)) {
                // a backend without sort_keys (the emulation): the keys as the values of a pair sort by their bucket number
                ensure(d_ikey3, (size_t)npos); ensure(d_ikey4, (size_t)npos);
                be.launch("index_key_buckets", npos, IndexKeyBuckets{d_ikey.p, pbits, d_ikey3.p});
                be.sort_pairs(d_ikey3.p, d_ikey4.p, d_ikey.p, d_ikey2.p, (size_t)npos, bbits);
            }
            be.launch("index_bucket_bounds", nbk + 1, IndexBucketBounds{d_ikey2.p, npos, pbits, d_bkbegin.p});
            be.launch_wave("index_bucket_fill", nbk, IndexBucketFill{P, d_R.p, nreg, d_bkbase.p, d_ikey2.p, d_bkbegin.p, pbits, d_slots.p, d_filter.p, d_next.p, d_rep.p,
                                                                     d_counter.p + kCtrOverflow, d_ovf.p, ovf_cap});
            be.launch("index_overflow", (int64_t)ovf_cap, IndexOverflow{P, d_R.p, nreg, d_posbase.p, d_counter.p + kCtrOverflow, d_ovf.p, ovf_cap, d_slots.p, d_next.p, d_rep.p});
        }
        if (npos_bucketed < npos) be.launch("index_insert", npos, IndexInsert{P, d_R.p, nreg, d_posbase.p, d_slots.p, d_next.p, d_filter.p, d_rep.p});
        if (index_verify) be.launch("index_verify", npos, IndexVerify{P, d_R.p, nreg, d_posbase.p, d_slots.p, d_filter.p, d_next.p, d_counter.p + kCtrLost});
        be.mark("repeat");
        ensure(d_run, (size_t)std::max<int64_t>(npos, 1));
        be.launch("run_length", npos, RunLength{P, d_R.p, nreg, d_posbase.p, d_run.p});
        be.launch("repeat_length", npos, RepeatLength{P, d_R.p, nreg, d_posbase.p, d_slots.p, d_filter.p, d_next.p, d_run.p, d_rep.p, d_repeated.p, d_err, work_budget, d_dense.p});
        if (nflag > 0) {
            be.mark("dense_sa");
            if (int rc = dense_build(R, nreg, nflag)) return rc;
        }
        return kNext;
    }

    int count_units(SearchCall& c) {
        const int64_t nreg = c.nreg, npairs = c.npairs; const int no_small = c.no_small; const GapBatch* const gb = c.gb;
        int64_t& nunits = c.nunits; size_t& ev_guess = c.ev_guess; bool& units_known = c.units_known;
        // -- work units (pairs that fit 128 bases on both sides go to SmallPairEvents instead)
        be.mark("units");
        be.launch("count_units", npairs, CountUnits{d_R.p, d_lens.p, ngen, d_ucount.p, g_first, g_last, no_small});
        be.exclusive_scan(d_ucount.p, d_uoff.p, (size_t)npairs + 1);
        // the host never saw the rows of a store search: the unit count is the device's.  The call used to wait for it (8 bytes); now it
        // launches over a CAPACITY from the last call of the shape, the kernels read the live count, and the count comes back with the
        // event counters (a capacity that was too small repeats the event search, like a full event buffer)
        // (which call of the step this is: the anchor call is number 0, the searches of store regions follow it -- a step that repeats
        // makes the same calls in the same order, and the capacities of a call come from the same call of the step before)
        if (!gb && nreg == 1) call_ordinal = 0; else if (gb) call_ordinal++;
        const size_t ord = gb || nreg == 1 ? (size_t)call_ordinal : (size_t)-1;      // (-1: a batch of the host route -- it waits for its counts)
        if (ord != (size_t)-1 && call_hints.size() <= ord) call_hints.resize(ord + 1);
        CallHint& hint = *(c.hint = ord != (size_t)-1 ? &call_hints[ord] : &c.none);
        if (hint_shrink > 1) {      // (tests) capacities carried over from the last step, made too small: the repeat paths run
            if (hint.units > 0) hint.units = std::max<int64_t>(1, hint.units / hint_shrink);
            if (hint.ncand > 0) hint.ncand = std::max<int64_t>(1, hint.ncand / hint_shrink);
        }
        units_known = !gb;
        if (gb && !(fast_tail && hint.units > 0)) {
            be.d2h(&nunits, d_uoff.p + npairs, 8);
            units_known = true;
        } else if (gb) nunits = hint.units + hint.units / 8 + 64;
        if (nunits >= (1ll << 31)) { error = "too many work units in one batch"; return -5; }
        if (gb) ev_guess += (size_t)nunits * 16;
        return kNext;
    }

    // One pass of the event search over the capacities in the record, up to its wait (round trip 1).  kRepeat: a capacity was too
    // small (the unit count's, an event slice's, a queue's, the grouped events') and has been raised; the pass runs again.
    int event_pass(SearchCall& c, bool again) {
        const int64_t nreg = c.nreg, npairs = c.npairs, nbk = c.nbk, nflag = c.nflag; const int lbits = c.lbits, no_small = c.no_small;
        const bool from_store = c.from_store, first_form = c.first_form, wide_form = c.wide_form, grouping = c.grouping;
        uint32_t* const d_err = c.d_err; const uint64_t ovf_cap = c.ovf_cap;
        int64_t &nunits = c.nunits, &nunits_live = c.nunits_live; bool& units_known = c.units_known;
        size_t &slice_cap = c.slice_cap, &queue_cap = c.queue_cap, &grp_cap = c.grp_cap;
        std::vector<uint64_t> &counts = c.counts, &qcounts = c.qcounts;
        uint64_t &nev = c.nev, &nrest = c.nrest, &ngrp = c.ngrp; uint32_t& errbits = c.errbits; bool& index_counts_read = c.index_counts_read;
        ensure(d_units, (size_t)std::max<int64_t>(nunits, 1));
        be.launch("fill_units", nunits, FillUnits{P, d_starts.p, d_lens.p, ngen, d_uoff.p, d_ucount.p, npairs, d_units.p});
        ensure(d_evkey, slice_cap * kSlices); ensure(d_evval, slice_cap * kSlices); ensure(d_rest, queue_cap * kSlices);
        if (again) be.memset(d_counter.p, 0, 8 * kCtrWords);      // event counters, error word, grouped events
        if (grouping) {
            ensure(d_evkey3, grp_cap + ev_cap_hint); ensure(d_evval3, grp_cap + ev_cap_hint);
            ensure(d_state, grp_cap + ev_cap_hint); ensure(d_emax, grp_cap + ev_cap_hint);
            be.mark("grouped_events");
            if (first_form)
                be.launch_wave("grouped_pair_events", xcd_grid(nreg),
                               GroupedPairEvents{P, d_R.p, d_starts.p, d_lens.p, ngen, d_rep.p, d_evkey3.p, d_evval3.p, d_counter.p + kCtrGrouped, (uint64_t)grp_cap, lbits,
                                                 d_glo.p, g_first, g_last, d_gflag.p, d_state.p, d_emax.p, d_epm.p, (int64_t)nreg});
            if (wide_form)
                be.launch_wave("grouped_pair_events_wide", xcd_grid(nreg),
                               GroupedPairEventsWide{P, d_R.p, d_starts.p, d_lens.p, ngen, d_rep.p, d_evkey3.p, d_evval3.p, d_counter.p + kCtrGrouped, (uint64_t)grp_cap, lbits,
                                                     d_glo.p, g_first, g_last, d_gflag.p, d_state.p, d_emax.p, d_epm.p, (int64_t)nreg, first_form ? 1 : 0, d_counter.p + kCtrWide});
        }
        be.memset(d_qcount.p, 0, 8 * (size_t)kSlices * kSliceStride);
        be.mark("seed_extend");
        be.launch("seed_extend", nunits * 64,
                  SeedExtend{P, d_R.p, d_units.p, d_slots.p, d_filter.p, d_next.p, d_rep.p, d_repeated.p,
                             d_evkey.p, d_evval.p, d_counter.p, (uint64_t)slice_cap, lbits, d_err, work_budget, d_rest.p, d_qcount.p, (uint64_t)queue_cap, d_uoff.p + npairs});
        if (nunits > 0)      // one lane per queued sample; lanes past a sub-queue's count leave at once (the counts stay on the device)
            be.launch("seed_rest", (int64_t)(queue_cap * kSlices),
                      SeedRest{P, d_R.p, d_units.p, d_rest.p, d_qcount.p, (uint64_t)queue_cap, d_slots.p, d_filter.p, d_next.p, d_rep.p,
                               d_evkey.p, d_evval.p, d_counter.p, (uint64_t)slice_cap, lbits, d_err, work_budget, d_dense.p});
        if (nunits > 0 && nflag > 0) {      // the probe items of the flagged regions
            be.mark("dense_search");
            be.launch("seed_dense", (int64_t)(queue_cap * kSlices),
                      SeedDense{P, d_R.p, d_units.p, d_rest.p, d_qcount.p, (uint64_t)queue_cap, d_dfi.p, d_dstart.p, d_dval2.p, d_rep.p,
                                d_evkey.p, d_evval.p, d_counter.p, (uint64_t)slice_cap, lbits});
            be.mark("seed_extend");
        }
        if (!no_small)
            be.launch("small_pair_events", npairs * 2,
                      SmallPairEvents{P, d_R.p, d_starts.p, d_lens.p, ngen, d_rep.p, d_evkey.p, d_evval.p, d_counter.p, (uint64_t)slice_cap, lbits, g_first, g_last, grouping ? d_gflag.p : nullptr});
        be.mark("sort");
        be.launch_wave("slice_offsets", 1, SliceOffsets{d_counter.p, d_sliceoff.p});
        group_downloads();      // (the read-backs of this wait: one launch)
        be.d2h_async(qcounts.data(), d_qcount.p, 8 * qcounts.size());
        if (from_store) be.d2h_async(alg_sets, d_alg.p, sizeof alg_sets);
        if (!units_known) be.d2h_async(&nunits_live, d_uoff.p + npairs, 8);
        run_beside();      // (the caller's host work that needs nothing of this call: the device is busy with the event search)
        be.d2h(counts.data(), d_counter.p, 8 * counts.size());            // round trip 1: event counts + error word (+ the queues' lengths, + the unit count)
        if (!index_counts_read) {      // (the first pass of this loop: a repeat clears the counters)
            index_counts_read = true;
            if (nbk > 0) last_index_overflow = (int64_t)counts[kCtrOverflow];
            if (index_verify) last_index_lost = (int64_t)counts[kCtrLost];
            if (nbk > 0 && counts[kCtrOverflow] > ovf_cap) { index_overflow_seen = (int64_t)counts[kCtrOverflow]; return kIndexRebuild; }
        }
        if (!units_known) {
            units_known = true;
            if (nunits_live >= (1ll << 31)) { error = "too many work units in one batch"; return -5; }
            if (nunits_live > nunits) {      // more units than the capacity: the event search again, over all of them
                nunits = nunits_live;
                queue_cap = std::max<size_t>(queue_cap, (size_t)nunits * kUnitSamples / 16 / kSlices + 64);
                tail_repeats++;
                return kRepeat;
            }
        }
        uint64_t worst = 0, qworst = 0;
        nev = 0; nrest = 0;
        for (int sl = 0; sl < kSlices; sl++) {
            const uint64_t n = counts[(size_t)sl * kSliceStride]; nev += n; worst = std::max(worst, n);
            const uint64_t q = qcounts[(size_t)sl * kSliceStride]; nrest += q; qworst = std::max(qworst, q);
        }
        errbits = (uint32_t)counts[kCtrErr];
        ngrp = grouping ? counts[kCtrGrouped] : 0;
        c.worst_slice = worst;      // events of the fullest sub-buffer
        if (worst <= slice_cap && qworst <= queue_cap && ngrp <= grp_cap) return kNext;
        if (ngrp > grp_cap) grp_cap = (size_t)(ngrp + ngrp / 8 + 64);
        if (worst > slice_cap) slice_cap = (size_t)(worst + worst / 8 + 64);
        if (qworst > queue_cap) queue_cap = (size_t)(qworst + qworst / 8 + 64);
        c.sticky |= errbits & (kErrWork | kErrRows);      // (RepeatLength's and CheckRows' verdicts: the word is cleared with the counters)
        return kRepeat;
    }

    int search_events(SearchCall& c) {
        const int64_t nreg = c.nreg, npairs = c.npairs, nunits = c.nunits; const int nq = c.nq, no_small = c.no_small;
        // -- events: kSlices append buffers (retry with larger ones on overflow), gathered, then sorted by (pair, l, strand)
        ensure(d_sliceoff, (size_t)kSlices + 1);
        c.slice_cap = (std::min<size_t>(std::max<size_t>(ev_cap_hint, c.ev_guess), (size_t)1 << 31) + kSlices - 1) / kSlices + 64;
        c.counts.assign(kCtrWords, 0);
        // samples that SeedExtend hands to SeedRest: kSlices sub-queues sized from what earlier calls needed (first guess: one
        // sample in sixteen), repeated with the exact size if one overflows (the counters keep counting past the capacity)
        ensure(d_qcount, (size_t)kSlices * kSliceStride);
        c.queue_cap = std::max<size_t>(std::max<size_t>(rest_cap_hint[nreg == 1], (size_t)nunits * kUnitSamples / 16 / kSlices), 64) + 64;      // (anchor-shaped and recursion-shaped calls alternate)
        c.qcounts.assign((size_t)kSlices * kSliceStride, 0);
        // the small regions of a recursion batch: their events once per distinct piece, straight into the head of the final array
        // (the first form up to kGrpGenomes query genomes; the wide form after it over the regions it left, or alone up to kWideGenomes)
        const bool small_groups = group_small && !no_small && !c.want_events && nreg >= 2;
        const bool first_form = c.first_form = small_groups && nq <= kGrpGenomes;
        const bool wide_form = c.wide_form = small_groups && group_wide && nq <= kWideGenomes;
        const bool grouping = c.grouping = first_form || wide_form;
        c.grp_cap = grouping ? std::max<size_t>(grp_cap_hint, (size_t)npairs * 3) + 64 : 0;
        if (grouping) { ensure(d_gflag, (size_t)nreg); ensure(d_glo, (size_t)npairs); }
        c.nunits_live = nunits;
        int rc;
        for (bool again = false; (rc = event_pass(c, again)) == kRepeat; again = true) {}
        if (rc != kNext) return rc;

        const GapBatch* const gb = c.gb; const bool from_store = c.from_store; CallHint& hint = *c.hint;
        const std::vector<uint64_t>& counts = c.counts;
        const uint64_t nev = c.nev, nrest = c.nrest, ngrp = c.ngrp; const size_t queue_cap = c.queue_cap; const int64_t nunits_live = c.nunits_live;
        uint32_t& errbits = c.errbits;
        errbits |= c.sticky;
        if (from_store) {
            alg_raw[0] = alg_raw[1] = alg_raw[2] = 0;
            for (int x = 0; x < kAlgSets; x++) for (int k = 0; k < 3; k++) alg_raw[k] += alg_sets[8 * x + k];
        }
        if (from_store) { last_alg[0] = (double)alg_raw[0] / 4.0; last_alg[1] = (double)alg_raw[1] / 2.0; last_alg[2] = (double)alg_raw[2] / 2.0; }
        if (errbits & kErrRows) { error = "region outside its genome"; return -2; }
        rest_cap_hint[nreg == 1] = queue_cap - 64;      // (the margin is added again by the next call: storing it with the margin let the queues grow by 64 items a call, and every ~20 steps the 100 MB block was reallocated -- an 8-16 ms step)
        if (gb) hint.units = std::max<int64_t>(nunits_live, 1);
        last_rest = (int64_t)nrest;
        ev_cap_hint = (size_t)(nev + nev / 4);
        if (grouping) grp_cap_hint = (size_t)(ngrp + ngrp / 4);
        last_events = (int64_t)(nev + ngrp);
        last_grouped = (int64_t)ngrp;
        last_grouped_wide = wide_form ? (int64_t)counts[kCtrWide] : 0;
        last_handed_back = wide_form ? (int64_t)counts[kCtrWide + 1] : -1;      // (-1: nobody counted them -- the wide form did not run)
        last_wide_regions = wide_form ? (int64_t)counts[kCtrWide + 2] : 0;
        // a rank of a sharded run that ran out of budget must not leave the others waiting in the collectives: the
        // verdict travels with the first exchange (below) and every rank returns the error together
        const bool sharded = c.sharded = coll.world > 1 || coll.device;      // (a one-rank RCCL session still runs the exchanges: that is how a 1-GPU box tests them)
        if ((errbits & kErrWork) && !sharded) { budget_exceeded = true; error = "per-thread work budget exceeded (degenerate repeat structure in a region)"; return -5; }
        return kNext;
    }

    void order_events(SearchCall& c) {
        const int64_t nreg = c.nreg, npairs = c.npairs, npos = c.npos, nchunks = c.nchunks, centries = c.centries; const int nq = c.nq, lbits = c.lbits;
        const uint64_t ngrp = c.ngrp, worst_slice = c.worst_slice; const size_t slice_cap = c.slice_cap; const bool grouping = c.grouping;
        uint64_t& nev = c.nev;
        ensure(d_evkey2, std::max<size_t>(nev, 1)); ensure(d_evval2, std::max<size_t>(nev, 1));
        // the final array: [ grouped events, contiguous and ordered per pair | the other events, sorted by (pair, l, strand) ]
        ensure_keep(d_evkey3, std::max<size_t>(ngrp + nev, 1), (size_t)ngrp); ensure_keep(d_evval3, std::max<size_t>(ngrp + nev, 1), (size_t)ngrp);
        const int keybits = bits_for((uint64_t)npairs) + lbits + 1;
        uint64_t *skey = c.skey = d_evkey3.p, *sval = c.sval = d_evval3.p;
        // the events in order: by buckets (pair, 256-position block) whose scanned counts are the readers' coarse table as well, or
        // (tune bucket_sort = 0: rounds 1-5) gathered, radix-sorted, and the table from a pass over the sorted keys
        const int64_t nbuckets = (int64_t)nq * nchunks;
        const bool by_buckets = c.by_buckets = bucket_sort && nev > 0 && nbuckets < ((int64_t)1 << 31);
        if (c.coarse_by_buckets && !by_buckets) be.memset(d_coarse.p, 0, 4 * (size_t)std::max<int64_t>(centries, 1));      // (no bucketed event: nobody else writes the table's zeros)
        ensure(d_lo, (size_t)npairs + 1);
        if (by_buckets) {
            ensure(d_bcount, (size_t)nbuckets + 2); ensure(d_bbegin, (size_t)nbuckets + 2); ensure(d_pbase, (size_t)npairs);
            int shift = 6;
            while (((uint64_t)1 << shift) < worst_slice) shift++;      // (the fullest slice's count: known since the wait above)
            // the counts one element up behind a 0: their scan is 0, begin[0 .. nbuckets] -- EventPlace's cursors from the second
            // element on, and begin[] from the first once the events are placed (kernels.h)
            be.memset(d_bcount.p, 0, 8 * ((size_t)nbuckets + 2));
            be.launch("pair_bucket_base", npairs, PairBucketBase{nq, d_cbase.p, d_pbase.p});
            be.launch("event_bucket_count", (int64_t)kSlices << shift, EventBucketCount{d_evkey.p, d_counter.p, (uint64_t)slice_cap, shift, lbits, d_pbase.p, d_bcount.p + 1});
            be.exclusive_scan(d_bcount.p, d_bbegin.p, (size_t)nbuckets + 2);
            be.launch("event_place", (int64_t)kSlices << shift,
                      EventPlace{d_evkey.p, d_evval.p, d_counter.p, (uint64_t)slice_cap, shift, lbits, d_pbase.p, d_bbegin.p + 1, d_evkey3.p + ngrp, d_evval3.p + ngrp});
            be.launch("event_order", nbuckets, EventOrder{d_bbegin.p, nbuckets, d_evkey3.p + ngrp, d_evval3.p + ngrp});
        } else if (nev > 0) {
            be.launch("compact_events", (int64_t)nev, CompactEvents{d_evkey.p, d_evval.p, d_sliceoff.p, (uint64_t)slice_cap, d_evkey2.p, d_evval2.p});
            be.sort_pairs(d_evkey2.p, d_evkey3.p + ngrp, d_evval2.p, d_evval3.p + ngrp, (size_t)nev, keybits);
        }
        be.mark("scan");
        const int64_t nev_sorted = (int64_t)nev;
        nev += ngrp;
        if (by_buckets) be.launch_wave("coarse_from_buckets", coarse_tiles(centries / nq, nq), CoarseFromBuckets{d_bbegin.p, d_cbase.p, nreg, nq, (int64_t)ngrp, d_coarse.p, d_lo.p, npairs, nev_sorted, centries / nq});
        else be.launch("pair_bounds", npairs, PairBounds{skey, (int64_t)nev, lbits, npairs, d_lo.p, (int64_t)ngrp});
        if (grouping) be.launch("grouped_bounds", npairs, GroupedBounds{d_gflag.p, d_glo.p, nq, d_lo.p});
        // (the grouped events came with their states: the scan runs over the sorted part, its event numbers relative to it)
        ensure_keep(d_state, std::max<size_t>(nev, 1), (size_t)ngrp); ensure_keep(d_emax, std::max<size_t>(nev, 1), (size_t)ngrp);
        const int64_t nsorted = (int64_t)(nev - ngrp);
        if (nsorted > 0) {
            const int64_t nwaves = (nsorted + kWaveEvents - 1) / kWaveEvents;
            ensure(d_wsummary, (size_t)nwaves); ensure(d_wcarry, (size_t)nwaves);
            const WaveScanCore core{skey + ngrp, sval + ngrp, nsorted, lbits, d_R.p, nq, d_rep.p};
            be.launch_wave("wave_summary", nwaves, WaveSummary{core, d_wsummary.p});
            be.launch_wave("summary_carry", (nwaves + kCarryTiles - 1) / kCarryTiles, SummaryCarry{core, d_wsummary.p, nwaves, d_lo.p, (int64_t)ngrp, d_wcarry.p});
            be.launch_wave("wave_scan", nwaves, WaveScan{core, d_wcarry.p, d_state.p + ngrp, d_emax.p + ngrp});
        }

        if (c.want_events) {   // parity hook (pm_find_events): sorted events + rep'
            ev_key_h.resize((size_t)nev); ev_val_h.resize((size_t)nev); rep_h.resize((size_t)npos);
            if (nev) { be.d2h(ev_key_h.data(), skey, 8 * (size_t)nev); be.d2h(ev_val_h.data(), sval, 8 * (size_t)nev); }
            if (npos) be.d2h(rep_h.data(), d_rep.p, 4 * (size_t)npos);
            ev_lbits = lbits;
        }
    }

    // the widest genome block of a sharded run (one genome at least): what every rank's block is padded to in an exchange
    int widest_block() const {
        int widest = 0;
        for (int r = 0; r < coll.world; r++) { int a, b; shard_range(ngen, r, coll.world, &a, &b); widest = std::max(widest, b - a); }
        return std::max(widest, 1);
    }

    int mumi_tail(SearchCall& c) {
        const int64_t npairs = c.npairs; const int lbits = c.lbits; const bool sharded = c.sharded;
        uint64_t* const skey = c.skey; uint64_t* const sval = c.sval; uint32_t& errbits = c.errbits;
        be.mark("mumi_coverage");
        ensure(d_cov, (size_t)npairs);
        be.launch("mumi_coverage", npairs, MumiCoverage{d_R.p, skey, sval, d_lo.p, d_state.p, d_rep.p, lbits, ngen, d_cov.p});
        mumi_covered.resize((size_t)npairs);
        be.d2h(mumi_covered.data(), d_cov.p, 8 * (size_t)npairs);
        if (sharded) {   // every rank computed its own genome block: gather the blocks (+ the ranks' error words)
            const size_t per = (size_t)widest_block() + 1;
            std::vector<int64_t> send(per, 0), recv(per * (size_t)coll.world);
            for (int g = g_first; g < g_last; g++) send[(size_t)(g - g_first)] = mumi_covered[(size_t)(g - 1)];
            send[per - 1] = errbits;
            if (allgather_host(send.data(), (int64_t)(8 * send.size()), recv.data())) { error = "all-gather of MUMi coverage failed"; return -4; }
            for (int r = 0; r < coll.world; r++) {
                int a, b; shard_range(ngen, r, coll.world, &a, &b);
                for (int g = a; g < b; g++) mumi_covered[(size_t)(g - 1)] = recv[(size_t)r * per + (size_t)(g - a)];
                errbits |= (uint32_t)recv[(size_t)r * per + per - 1];
            }
            if (errbits & kErrWork) { budget_exceeded = true; error = "per-thread work budget exceeded on some rank (degenerate repeat structure in a region)"; return -5; }
        }
        be.mark(nullptr);
        collect_timing();
        return 0;
    }

    int master_ep(SearchCall& c) {
        const int64_t nreg = c.nreg, npos = c.npos, nchunks = c.nchunks, nwv = c.nwv; const int nq = c.nq, lbits = c.lbits;
        const uint64_t nev = c.nev, ngrp = c.ngrp; const uint32_t errbits = c.errbits; const bool by_buckets = c.by_buckets, grouping = c.grouping, sharded = c.sharded;
        uint64_t* const skey = c.skey; int32_t& verdict = c.verdict;
        // -- Master.EP, candidates
        be.mark("master_ep");
        // (by buckets: the table came with the order -- but for the grouped regions' pairs, whose events never were in a bucket)
        if (!by_buckets) be.launch("coarse_fill", (int64_t)nev, CoarseFill{skey, (int64_t)nev, lbits, d_lo.p, d_R.p, d_cbase.p, nq, d_coarse.p});
        else if (ngrp > 0) be.launch("coarse_fill", (int64_t)ngrp, CoarseFill{skey, (int64_t)ngrp, lbits, d_lo.p, d_R.p, d_cbase.p, nq, d_coarse.p});
        if (master_seg) be.launch_wave("master_ep_seg", xcd_grid(nchunks), MasterEPSeg{d_R.p, nreg, ngen, skey, d_lo.p, d_emax.p, lbits, d_epm.p, d_cbase.p, d_coarse.p, g_first, g_last, grouping ? d_gflag.p : nullptr, nchunks});
        else be.launch_wave("master_ep", xcd_grid(nchunks), MasterEP{d_R.p, nreg, ngen, skey, d_lo.p, d_emax.p, lbits, d_epm.p, d_cbase.p, d_coarse.p, g_first, g_last, grouping ? d_gflag.p : nullptr, nchunks});
        if (sharded && coll.device) {   // exchange 1 on the device: RCCL all-reduce(min) of Master.EP in place, + the error verdict word
            be.mark("exchange_ep");
            be.fill32(d_epm.p + npos, (errbits & kErrWork) ? -1 : 0);
            if (be.allreduce_min_i32_dev(d_epm.p, npos + 1)) { error = "RCCL all-reduce of Master.EP failed: " + be.error(); return -4; }
            be.d2h_async(&verdict, d_epm.p + npos, 4);       // read with the candidate count below
        } else if (sharded) {   // exchange 1: Master.EP = min over the ranks' genome blocks; the last word carries the error verdict
            be.mark("exchange_ep");
            std::vector<int32_t> h((size_t)npos + 1);
            if (npos) be.d2h(h.data(), d_epm.p, 4 * (size_t)npos);
            h[(size_t)npos] = (errbits & kErrWork) ? -1 : 0;
            if (coll.allreduce_min_i32(coll.ctx, h.data(), npos + 1)) { error = "all-reduce of Master.EP failed"; return -4; }
            verdict = h[(size_t)npos];
            if (verdict >= 0 && npos) be.h2d(d_epm.p, h.data(), 4 * (size_t)npos);
        }
        be.mark("candidates");
        be.launch_wave("cand_mark", nwv, CandMark{d_R.p, nreg, d_posbase.p, npos, d_epm.p, d_wmask.p, d_wcount.p});
        be.exclusive_scan(d_wcount.p, d_woff.p, (size_t)nwv + 1);
        c.ncand_p = d_woff.p + nwv;      // the candidate count, where the device keeps it
        return kNext;
    }

    int candidate_tail(SearchCall& c) {
        const int64_t nreg = c.nreg; const GapBatch* const gb = c.gb; const bool from_store = c.from_store, sharded = c.sharded; const CallHint& hint = *c.hint;
        // The rest of the call -- candidates listed, folded over the genomes, the accepted ones compacted into rows, the overlap flags
        // of a long list -- used to wait twice for the device, for the candidate count and for the accepted count, because the
        // launches and buffers were sized with them.  A call whose rows stay on the device (the resident route's anchor call and its
        // store searches) no longer does: launches and buffers take CAPACITIES from what the last call of the same shape needed,
        // every kernel reads the live count from device memory, and both counts come back with the results, in the call's one last
        // wait.  A capacity that turns out too small (or an anchor list that turns out short) repeats the tail the exact way.
        const bool anchor_guess = c.anchor_guess = nreg == 1 && !gb && hint.nok >= dirty_min;
        const bool may_skip_waits = !sharded && want_rows && resident && hint.ncand > 0 && (from_store || anchor_guess) && fast_tail;
        int rc;
        for (int attempt = may_skip_waits ? 0 : 1; (rc = tail_attempt(c, attempt > 0)) == kRepeat; attempt++) {}
        if (rc != kNext) return rc;
        collect_timing();
        return 0;
    }

    // exchange 2 of a sharded run: the candidates' states in every genome, each rank's block from the rank that searched it (d_at).
    // -> 0, or an error code
    int exchange_states(SearchCall& c) {
        const int nq = c.nq, lbits = c.lbits; const uint64_t ncand = c.ncand; const uint64_t* const scand = d_cand.p;
        uint64_t* const skey = c.skey; uint64_t* const sval = c.sval;
        ensure(d_at, (size_t)ncand * (size_t)nq);
        be.launch("state_at_candidate", (int64_t)ncand * nq, StateAtCandidate{d_R.p, scand, ngen, skey, sval, d_lo.p, d_state.p, d_rep.p, lbits, d_at.p, d_cbase.p, d_coarse.p});
        be.mark("exchange_states");
        const size_t nqz = (size_t)nq, cz = (size_t)ncand;
        const int widest = widest_block();
        const size_t blk = cz * (size_t)widest;
        if (coll.device) {      // pack this rank's columns, RCCL all-gather on the engine's stream, spread the blocks: nothing leaves the device
            ensure(d_xsend, blk); ensure(d_xrecv, blk * (size_t)coll.world);
            be.launch("pack_states", (int64_t)blk, PackStates{d_at.p, nq, g_first - 1, g_last - g_first, widest, d_xsend.p});
            if (be.allgather_dev(d_xsend.p, (int64_t)(sizeof(GenomeAtK) * blk), d_xrecv.p)) { error = "RCCL all-gather of candidate states failed: " + be.error(); return -4; }
            be.launch("unpack_states", (int64_t)(cz * nqz), UnpackStates{d_xrecv.p, nq, coll.world, widest, (int64_t)ncand, d_at.p});
        } else {
            std::vector<GenomeAtK> all(cz * nqz);
            be.d2h(all.data(), d_at.p, sizeof(GenomeAtK) * all.size());
            std::vector<GenomeAtK> send(blk), recv(blk * (size_t)coll.world);
            const size_t mine = (size_t)(g_last - g_first);
            for (size_t k = 0; k < cz; k++)
                for (size_t x = 0; x < mine; x++) send[k * (size_t)widest + x] = all[k * nqz + (size_t)(g_first - 1) + x];
            if (coll.allgather(coll.ctx, send.data(), (int64_t)(sizeof(GenomeAtK) * send.size()), recv.data())) { error = "all-gather of candidate states failed"; return -4; }
            for (int r = 0; r < coll.world; r++) {
                int a, b; shard_range(ngen, r, coll.world, &a, &b);
                const GenomeAtK* src = recv.data() + (size_t)r * send.size();
                for (size_t k = 0; k < cz; k++)
                    for (int x = 0; x < b - a; x++) all[k * nqz + (size_t)(a - 1 + x)] = src[k * (size_t)widest + (size_t)x];
            }
            be.h2d(d_at.p, all.data(), sizeof(GenomeAtK) * all.size());
        }
        be.mark("fold");
        return 0;
    }

    // One attempt at the tail.  exact: it waits for the candidate count and the accepted count (round trips 2 and 3); else it runs over
    // capacities from the hint and returns kRepeat if one of them was too small, or the list is not the long list it was taken for.
    int tail_attempt(SearchCall& c, const bool exact) {
        const int64_t nreg = c.nreg, nwv = c.nwv; const int nq = c.nq, lbits = c.lbits; const GapBatch* const gb = c.gb; BatchResult* const out = c.out;
        const bool from_store = c.from_store, sharded = c.sharded; CallHint& hint = *c.hint;
        uint64_t* const skey = c.skey; uint64_t* const sval = c.sval; const int64_t* const ncand_p = c.ncand_p;
        const int32_t& verdict = c.verdict;      // (a reference: the device exchange's verdict lands with the wait for the candidate count)
        int64_t &ncand_i = c.ncand_i, &nok = c.nok; int64_t (&counts_h)[2] = c.counts_h; std::vector<int32_t>& reg_h = c.reg_h;
        c.exact = exact;
        ncand_i = 0;
        if (exact) be.d2h(&ncand_i, ncand_p, 8);                                   // round trip 2: candidate count
        if (verdict < 0) { budget_exceeded = true; error = "per-thread work budget exceeded on some rank (degenerate repeat structure in a region)"; return -5; }
        if (exact) {
            last_candidates = ncand_i;
            if (ncand_i == 0) { hint.ncand = 1; hint.nok = 0; if (resident && from_store) out->store_base = ms_count; be.mark(nullptr); collect_timing(); return 0; }
        }
        // capacity of the candidate list: the count itself when it is known
        const uint64_t ncand = c.ncand = exact ? (uint64_t)ncand_i : (uint64_t)(hint.ncand + hint.ncand / 8 + 256);
        ensure(d_cand, (size_t)ncand);
        be.launch("cand_write", nwv * 64, CandWrite{d_R.p, nreg, d_posbase.p, d_wmask.p, d_woff.p, d_cand.p, ncand});
        const uint64_t* scand = d_cand.p;        // in (region, k) order by construction

        // -- per-candidate genome fold
        be.mark("fold");
        ensure(d_ok, (size_t)ncand); ensure(d_ok_k, (size_t)ncand); ensure(d_ok_lon, (size_t)ncand);
        ensure(d_osp, (size_t)ncand * (size_t)nq); ensure(d_ofwd, (size_t)ncand * (size_t)nq);
        const GenomeAtK* at = nullptr;
        if (sharded) {   // exchange 2: every rank contributes the (EP,UP,SP) columns of its genome block
            if (int rc = exchange_states(c)) return rc;
            at = d_at.p;
        }
        be.launch_wave("fold_candidates", xcd_grid((int64_t)ncand),
                       FoldCandidates{d_R.p, scand, ngen, at, skey, sval, d_lo.p, d_state.p, d_rep.p, lbits, d_cbase.p, d_coarse.p,
                                      d_ok_k.p, d_ok_lon.p, d_osp.p, d_ofwd.p, d_ok.p, (int64_t)ncand, ncand_p});

        // -- accepted candidates, compacted on the device and downloaded straight into the result's blocks
        be.mark("compact");
        ensure(d_okcnt, (size_t)ncand + 1); ensure(d_okpos, (size_t)ncand + 1);
        be.launch("ok_count", (int64_t)ncand + 1, OkCount{d_ok.p, ncand_p, d_okcnt.p, (int64_t)ncand});
        be.exclusive_scan(d_okcnt.p, d_okpos.p, (size_t)ncand + 1);
        const int64_t* nok_p = c.nok_p = d_okpos.p + ncand;      // the accepted count, where the device keeps it
        nok = 0;
        if (exact) be.d2h(&nok, nok_p, 8);                                    // round trip 3: accepted count
        // capacity of the accepted rows: the count itself when it is known, else every candidate could be accepted
        const size_t nokz = c.nokz = exact ? (size_t)nok : (size_t)ncand;
        ensure(d_creg, std::max<size_t>(nokz, 1)); ensure(d_ck, std::max<size_t>(nokz, 1)); ensure(d_clon, std::max<size_t>(nokz, 1));
        reg_h.assign(nokz, 0);
        out->release();
        out->kb = pool->take(4 * nokz); out->lonb = pool->take(4 * nokz);
        out->rows = want_rows; out->dirty_known = false; out->table_id = 0; out->store_base = -1;
        const StoreCounts before = store_mark();
        c.anchor_call = false;
        if (!want_rows) compact_sp(c); else compact_rows(c);
        be.d2h_async(reg_h.data(), d_creg.p, 4 * nokz);
        be.d2h_async(out->kb.p, d_ck.p, 4 * nokz);
        counts_h[0] = ncand_i; counts_h[1] = nok;
        if (!exact) { be.d2h_async(&counts_h[0], ncand_p, 8); be.d2h_async(&counts_h[1], nok_p, 8); }
        flush_downloads();
        be.mark(nullptr);
        be.sync();                                                         // round trip 4: the results (and, where the call did not wait for them, the two counts)
        const bool anchor_call = c.anchor_call;
        if (!exact) {
            ncand_i = counts_h[0]; nok = counts_h[1];
            const bool fits = (uint64_t)ncand_i <= ncand && anchor_call == (nreg == 1 && !gb && nok >= dirty_min);
            if (!fits) {      // the capacity was too small, or the list is not the long list it was taken for: again, with the counts
                store_rewind(before);
                tail_repeats++;
                be.mark("candidates");
                return kRepeat;
            }
            last_candidates = ncand_i;
            if (out->store_base >= 0) ms_count = out->store_base + nok;
        }
        hint.ncand = std::max<int64_t>(ncand_i, 1); hint.nok = nok;
        last_accepted = nok;
        if (anchor_call) { anchor_table_rows = nok; anchor_table_id = out->table_id; }
        for (int64_t w = 0; w < nok; w++) out->off[(size_t)reg_h[(size_t)w] + 1]++;
        for (int64_t r = 0; r < nreg; r++) out->off[(size_t)r + 1] += out->off[(size_t)r];
        out->total = out->off[(size_t)nreg];
        if (out->table_id && out->store_base == 0) anchor_flags_h.assign(out->flags(), out->flags() + nok);      // (settle() lists the flagged rows from it)
        return kNext;
    }

    // the accepted candidates as (sp, fwd) rows, and their downloads
    void compact_sp(SearchCall& c) {
        const int nq = c.nq; const uint64_t ncand = c.ncand; const size_t nokz = c.nokz, nqz2 = (size_t)nq; BatchResult* const out = c.out;
        const uint64_t* const scand = d_cand.p; const int64_t* const ncand_p = c.ncand_p;
        ensure(d_csp, std::max<size_t>(nokz * nqz2, 1)); ensure(d_cfwd, std::max<size_t>(nokz * nqz2, 1));
        be.launch("compact_sp", (int64_t)ncand * nq,
                  CompactSp{scand, d_ok.p, d_okpos.p, nq, d_ok_k.p, d_ok_lon.p, d_osp.p, d_ofwd.p, d_creg.p, d_ck.p, d_clon.p, d_csp.p, d_cfwd.p, ncand_p});
        be.mark("download");
        group_downloads();
        out->spb = pool->take(4 * nokz * nqz2); out->fwdb = pool->take(nokz * nqz2);
        be.d2h_async(out->spb.p, d_csp.p, 4 * nokz * nqz2);
        be.d2h_async(out->fwdb.p, d_cfwd.p, nokz * nqz2);
        be.d2h_async(out->lonb.p, d_clon.p, 4 * nokz);
    }

    // the accepted candidates as MUM rows (start, strand, flags), into the MUM store where they stay on the device; their downloads
    void compact_rows(SearchCall& c) {
        const int64_t nreg = c.nreg; const GapBatch* const gb = c.gb; const bool from_store = c.from_store, exact = c.exact, anchor_guess = c.anchor_guess;
        const int64_t nok = c.nok; const uint64_t ncand = c.ncand; const size_t nokz = c.nokz, ngz = (size_t)ngen; BatchResult* const out = c.out;
        const uint64_t* const scand = d_cand.p; const int64_t* const ncand_p = c.ncand_p; const int64_t* const nok_p = c.nok_p;
        bool& anchor_call = c.anchor_call;
        // Resident mode (pm_session_rows(s, 2)): the rows of the anchor call, and of every search of regions of the region store,
        // stay on the device as rows of the MUM store -- the host receives the per-row scalars only (flags, k, length).  The
        // anchor call's rows are the session's anchor table (= rows [0, A) of the store) in either mode.  The compaction
        // writes such rows straight into the store (a copy of the 60 MB anchor table is half a millisecond).
        anchor_call = nreg == 1 && !gb && (exact ? nok >= dirty_min : anchor_guess);
        const bool keep_rows = resident && (anchor_call || from_store);
        const bool to_store = anchor_call || keep_rows;
        int32_t* p_start; uint8_t* p_strand; int32_t* p_lon; uint32_t* p_flags;
        if (to_store) {
            if (anchor_call) store_reset();
            const size_t base = (size_t)ms_count, upto = base + nokz;
            ensure_keep(d_anchor_start, std::max<size_t>(upto * ngz, 1), base * ngz); ensure_keep(d_ms_strand, std::max<size_t>(upto * ngz, 1), base * ngz);
            ensure_keep(d_anchor_lon, std::max<size_t>(upto, 1), base); ensure_keep(d_anchor_flags, std::max<size_t>(upto, 1), base);
            ensure_keep(d_ms_shift, std::max<size_t>(upto, 1), base); ensure_keep(d_ms_len, std::max<size_t>(upto, 1), base); ensure_keep(d_ms_state, std::max<size_t>(upto, 1), base);
            p_start = d_anchor_start.p + base * ngz; p_strand = d_ms_strand.p + base * ngz; p_lon = d_anchor_lon.p + base; p_flags = d_anchor_flags.p + base;
            out->store_base = (int64_t)base;
            ms_count = (int64_t)upto;      // (capacity: set to base + the accepted count once that is known)
        } else {
            ensure(d_csp, std::max<size_t>(nokz * ngz, 1)); ensure(d_cfwd, std::max<size_t>(nokz * ngz, 1)); ensure(d_cflags, std::max<size_t>(nokz, 1));
            p_start = d_csp.p; p_strand = d_cfwd.p; p_lon = d_clon.p; p_flags = d_cflags.p;
        }
        const bool long_list = nreg == 1 && (exact ? nok >= dirty_min : anchor_guess);
        if (long_list) ensure(d_dirty, nokz);
        {      // the flags of the rows (OR-ed into), the cheap overlap test's marks, shift and state of the new store rows: one launch
            const ClearJob jobs[] = {{p_flags, 4 * nokz, 0}, {long_list ? d_dirty.p : nullptr, long_list ? 4 * nokz : 0, 0},
                                     {to_store ? d_ms_shift.p + (ms_count - (int64_t)nokz) : nullptr, to_store ? 4 * nokz : 0, 0},
                                     {to_store ? d_ms_state.p + (ms_count - (int64_t)nokz) : nullptr, to_store ? nokz : 0, 0}};
            be.clear_many(jobs, 4);
        }
        be.launch("compact_candidates", (int64_t)ncand * ngen,
                  CompactCandidates{scand, d_ok.p, d_okpos.p, ngen, d_ok_k.p, d_ok_lon.p, d_osp.p, d_ofwd.p, d_starts.p, d_lens.p, d_glen,
                                    d_creg.p, d_ck.p, p_lon, p_start, p_strand, p_flags, ncand_p});
        if (long_list) {     // a long list of one region (the anchor call): the cheap overlap test on the device
            const int64_t nblocks = ((int64_t)nokz + kDirtyBlock - 1) / kDirtyBlock, groups = (ngen + 63) / 64;
            ensure(d_bmax, (size_t)nblocks * ngz); ensure(d_bmin, (size_t)nblocks * ngz);
            be.launch_wave("dirty_extent", nblocks * groups, DirtyExtent{p_start, p_lon, p_flags, nok_p, ngen, d_bmax.p, d_bmin.p});
            be.launch_wave("dirty_prefix", groups, DirtyPrefix{nblocks, ngen, d_bmax.p, d_bmin.p});
            be.launch_wave("dirty_mark", nblocks * groups, DirtyMark{p_start, p_lon, nok_p, ngen, d_bmax.p, d_bmin.p, p_flags, d_dirty.p});
            be.launch("dirty_merge", (int64_t)nokz, DirtyMerge{d_dirty.p, p_flags, nok_p});
            out->dirty_known = true;
        }
        if (to_store) {
            be.d2d(d_ms_len.p + (ms_count - (int64_t)nokz), p_lon, 4 * nokz);
            if (anchor_call) out->table_id = ++table_counter;
        }
        be.mark("download");
        group_downloads();      // (flags, lengths, regions, k and the two counts: one launch instead of seven copies)
        out->flagsb = pool->take(4 * nokz);
        be.d2h_async(out->flagsb.p, p_flags, 4 * nokz);
        if (!keep_rows) {
            out->startb = pool->take(4 * nokz * ngz); out->strandb = pool->take(nokz * ngz);
            be.d2h_async(out->startb.p, p_start, 4 * nokz * ngz);
            be.d2h_async(out->strandb.p, p_strand, nokz * ngz);
        }
        be.d2h_async(out->lonb.p, p_lon, 4 * nokz);
    }

public:

    // =====================================================================================================================
    // The resident route (store_kernels.h; include/parsnp_mum.h: pm_store_*): what the reference does with the candidate lists
    // AFTER csgmum produced them, on rows that never leave the device.  Every method is one call of the C ABI.
    // =====================================================================================================================
    bool resident = false;            // pm_session_rows(s, 2)
    int64_t ms_count = 0;             // rows of the MUM store: [0, anchor_table_rows) = the anchor table, then every search of store regions
    int64_t rg_count = 0;             // regions of the region store
    std::vector<RegInfo> rg_info_h;   // host mirror of what the device said about each region (by region id)
    std::vector<uint32_t> anchor_flags_h;
    static constexpr int kAgain = -6; // PM_EAGAIN: the resident route does not apply; the caller takes the host route

    // "nothing of the last call": the counts of a search that travel with pm_last_timing (a search sets last_events and last_rest itself)
    void reset_call_counts() {
        last_positions = last_candidates = last_accepted = last_grouped = last_grouped_wide = last_wide_regions = 0; last_handed_back = -1;
        last_index_bucketed = last_index_overflow = 0; last_index_lost = -1; last_alg[0] = last_alg[1] = last_alg[2] = 0;
    }
    void begin_store_call() { timing.clear(); last_events = last_rest = 0; reset_call_counts(); }
    Store store_view() { return Store{d_anchor_start.p, d_ms_strand.p, d_anchor_lon.p, d_anchor_flags.p, d_ms_shift.p, d_ms_len.p, d_ms_state.p, ngen}; }
    // coherent: the reader must see marks made while its kernel runs (a wavefront that validates candidates in order)
    Layout layout_view(uint64_t* image, bool coherent = true) { return Layout{image, d_lay_off.p, d_lay_bits.p, coherent ? 1 : 0}; }
    // geometry of the layout image: genome j has glen[j] + 1 bits (the last one the sentinel, src/parsnp.cpp:3184-3185)
    size_t layout_geometry() {
        const size_t ngz = (size_t)ngen;
        if (lay_words == 0) {
            std::vector<int64_t> off(ngz + 1, 0), bits(ngz);
            for (size_t j = 0; j < ngz; j++) { bits[j] = glen_h[j] + 1; off[j + 1] = off[j] + (bits[j] + 63) / 64 + 1; }
            ensure(d_lay_off, ngz + 1); ensure(d_lay_bits, ngz);
            be.h2d(d_lay_off.p, off.data(), 8 * (ngz + 1)); be.h2d(d_lay_bits.p, bits.data(), 8 * ngz);
            lay_words = (size_t)off[ngz];
            lay_off_h = off;
        }
        return lay_words;
    }
    int need_resident(int64_t table_id) {
        if (!resident) { error = "the session is not in resident mode"; return -2; }
        if (table_id == 0 || table_id != anchor_table_id) { error = "the anchor table of this request is no longer resident"; return -2; }
        return 0;
    }
    // Second half of setMums1 (src/parsnp.cpp:1713-1841) for the resident anchor list, into an EMPTY layout: rows that overlap
    // nothing earlier are settled at once and marked; the flagged ones against those marks -- all at once where they meet no
    // other flagged row, in list order where they do.  out[c] for every row of the table.
    int store_settle(int64_t table_id, RowInfo* out) {
        if (int rc = settle_launch(table_id)) return rc;
        return store_info(0, anchor_table_rows, out);
    }
    // the launches of store_settle (nothing is waited for)
    int settle_launch(int64_t table_id) {
        if (int rc = need_resident(table_id)) return rc;
        begin_store_call();
        const int64_t rows = anchor_table_rows;
        // (the clears are queued first: the device wipes 2 x 126 MB while the host looks through the list's flags)
        const size_t words = layout_geometry();
        ensure(d_image, words);
        be.mark("settle");
        ensure(d_foreign_count, 2);
        be.memset(d_foreign_count.p, 0, 16);      // (candidates noted for store_order_check: none yet)
        ms_key_rows = 0; foreign_seen = 0;
        be.memset(d_image.p, 0, 8 * words);
        ensure(d_recwords, words);
        be.memset(d_recwords.p, 0, words);      // (where the recursion marks: ClusterValidate, for the order check)
        const Store S = store_view();
        const Layout L = layout_view(d_image.p);
        be.launch_wave("settle_clean", rows, SettleClean{S, P});
        std::vector<int32_t> fl;
        for (int64_t c = 0; c < rows; c++) { const uint32_t f = anchor_flags_h[(size_t)c]; if (!(f & (kRowBad | kRowOutside)) && (f & kRowDirty)) fl.push_back((int32_t)c); }
        // The cheap running-extent test flags every row of an inverted or moved block, whether it overlaps anything or not: a
        // population with a few inversions has a third of its rows flagged and a handful tangled, a set with 10 % of every one of its
        // 500 genomes rearranged has all of them flagged and thousands tangled.  The flagged rows that meet no other flagged row cost a
        // wavefront each, side by side; the TANGLED ones are settled in list order where they meet one another -- in rounds, every
        // row as soon as the tangled rows before it that share a 64-base word with it are done (TangleOwner / TangleSettle), and what
        // kTangleRounds rounds leave by one wavefront.  With more than one row in flagged_div flagged the tangled rows are counted
        // first (one 8-byte read-back) and the list is declined above tangled_max of them (PM_EAGAIN: the host route's exact overlap
        // test and threads).  flagged_div = 1: never declined (tests).
        const bool many_flagged = flagged_div > 1 && fl.size() * (size_t)flagged_div > (size_t)rows;
        // do the rows that can be accepted untrimmed lie in list order in every genome (none starts before the end of an earlier
        // row: the engine's kRowEarly bit)?  Then their marks need no atomics (StoreMarkOrdered)
        bool ordered = true;
        for (int64_t c = 0; c < rows && ordered; c++) { const uint32_t f = anchor_flags_h[(size_t)c]; ordered = !((f & kRowEarly) && !(f & (kRowBad | kRowOutside | kRowDirty))); }
        if (ordered && !force_atomic_marks) be.launch_wave("store_mark_ordered", ((rows + kMarkRows - 1) / kMarkRows) * ((ngen + 63) / 64), StoreMarkOrdered{S, L, rows});
        else be.launch("store_mark", rows * ngen, StoreMark{S, L, 0, (uint8_t)(kStAccepted | kStFlagged), kStAccepted});
        be.launch("layout_sentinel", (int64_t)ngen, LayoutSentinel{d_lay_off.p, d_lay_bits.p, d_image.p});
        if (!fl.empty()) {
            const uint64_t* before_once = d_once.p; const uint64_t* before_twice = d_twice.p;
            ensure(d_once, words); ensure(d_twice, words); ensure(d_list, fl.size());
            if (d_once.p != before_once || d_twice.p != before_twice) { be.memset(d_once.p, 0, 8 * words); be.memset(d_twice.p, 0, 8 * words); }      // (kept all zero between calls: CollideClear)
            be.h2d(d_list.p, fl.data(), 4 * fl.size());
            be.launch("collide_mark", (int64_t)fl.size() * ngen, CollideMark{S, d_list.p, layout_view(d_once.p), d_twice.p});
            be.launch_wave("collide_test", (int64_t)fl.size(), CollideTest{S, d_list.p, layout_view(d_twice.p, false)});
            be.launch("collide_clear", (int64_t)fl.size() * ngen, CollideClear{S, d_list.p, layout_view(d_once.p), d_twice.p});
            ensure(d_t_rem, 2); ensure(d_t_done, fl.size());
            {
                const ClearJob jobs[] = {{d_t_rem.p, 16, 0}, {d_t_done.p, fl.size(), 0}};
                be.clear_many(jobs, 2);
            }
            be.launch("count_tangled", (int64_t)fl.size(), CountTangled{S, d_list.p, d_t_rem.p});
            if (many_flagged) {
                uint64_t tangled = 0;
                be.d2h(&tangled, d_t_rem.p, 8);
                if ((int64_t)tangled > tangled_max) {
                    be.mark(nullptr);
                    collect_timing_more();
                    error = "too many rows of the list overlap one another (rearranged genomes): the host route decides";
                    return kAgain;
                }
            }
            be.launch_wave("settle_flagged", (int64_t)fl.size(), SettleFlagged{S, layout_view(d_image.p, false), P, d_list.p});
            {
                const int32_t* before = d_owner.p;
                ensure(d_owner, words);
                if (d_owner.p != before) be.memset(d_owner.p, 0, 4 * words);      // (kept all zero between calls)
            }
            // as many rounds as the last step of the session needed, + 1 (a round that settles nothing costs three launches of 4 us;
            // what the rounds leave is the serial wavefront's either way): every round notes how many rows it left
            int rounds = tangle_rounds ? kTangleRounds : 0;
            if (rounds && tangle_ran > 0) {
                int last = 0;
                for (int r = 1; r < tangle_ran; r++) if (tangle_left[r] < tangle_left[r - 1]) last = r;
                rounds = std::min(kTangleRounds, last + 2);
            }
            ensure(d_t_left, kTangleRounds);
            for (int round = 0; round < rounds; round++) {
                be.launch_wave("tangle_owner", (int64_t)fl.size(), TangleOwner{S, d_list.p, d_lay_off.p, d_lay_bits.p, d_owner.p, d_t_done.p, d_t_rem.p});
                be.launch_wave("tangle_settle", (int64_t)fl.size(), TangleSettle{S, layout_view(d_image.p, false), P, d_list.p, d_owner.p, d_t_done.p, d_t_rem.p});
                be.launch_wave("tangle_clear", (int64_t)fl.size(), TangleClear{S, d_list.p, d_lay_off.p, d_lay_bits.p, d_owner.p, d_t_done.p, d_t_rem.p, d_t_left.p + round});
            }
            tangle_ran = 0;
            if (rounds) { be.d2h_async(tangle_left, d_t_left.p, 8 * (size_t)rounds); tangle_ran = rounds; }      // (lands with the call's results)
            be.launch_wave("settle_tangled", 1, SettleTangled{S, L, P, d_list.p, (int64_t)fl.size(), d_t_done.p, d_t_rem.p});
        }
        layout_rows = rows;
        return 0;
    }
    // store_settle and store_seeds in one call, without the round trip between them: the accepted anchors are listed on the device,
    // the kept regions are placed in the reference's push order (SeedCount / SeedPlace), and the per-row scalars of the table travel
    // with the regions' summaries.  infos / ids: as store_seeds leaves them.
    int store_settle_seeds(int64_t table_id, int32_t q, RowInfo* out, std::vector<RegInfo>* infos, std::vector<int32_t>* ids) {
        infos->clear(); ids->clear();
        if (int rc = settle_launch(table_id)) return rc;
        const int64_t rows = anchor_table_rows;
        rg_count = 0;
        if (rows == 0) return 0;
        const Store S = store_view();
        ensure(d_rowinfo, (size_t)rows);
        be.launch("store_info", rows, StoreInfoOut{S, 0, d_rowinfo.p});
        be.mark("seeds");
        ensure(d_ch_flag, (size_t)rows + 1); ensure(d_ch_pos, (size_t)rows + 1); ensure(d_list, (size_t)rows);
        ensure(d_sd_cnt, (size_t)rows + 1); ensure(d_sd_off, (size_t)rows + 1); ensure(d_sd_keep, (size_t)rows);
        be.launch("chain_flag", rows + 1, ChainFlag{S, rows, d_ch_flag.p});
        be.exclusive_scan(d_ch_flag.p, d_ch_pos.p, (size_t)rows + 1);
        be.launch("anchor_list", rows, AnchorList{S, d_ch_pos.p, d_list.p});
        const int64_t* nacc = d_ch_pos.p + rows;
        const Layout L = layout_view(d_image.p, false);
        be.memset(d_sd_cnt.p + rows, 0, 8);
        be.launch_wave("seed_count", xcd_grid(rows), SeedCount{S, L, P, d_list.p, nacc, q, d_sd_cnt.p, d_sd_keep.p, rows});
        be.exclusive_scan(d_sd_cnt.p, d_sd_off.p, (size_t)rows + 1);
        size_t cap = std::max<size_t>(rg_cap_hint, (size_t)rows / 4 + 1024);
        std::vector<RegInfo> raw;
        for (bool again = false;; again = true) {
            ensure(d_rg_start, cap * (size_t)ngen); ensure(d_rg_len, cap * (size_t)ngen); ensure(d_rg_info, cap);
            be.launch_wave("seed_place", xcd_grid(rows), SeedPlace{S, L, P, d_list.p, nacc, d_sd_off.p, d_sd_keep.p, d_rg_start.p, d_rg_len.p, d_rg_info.p, (uint64_t)cap, rows});
            be.mark(nullptr);
            // the summaries travel with the count: as many as the last run had (a run with more fetches the rest)
            const size_t guess = std::min(cap, rg_cap_hint / (size_t)hint_shrink);
            raw.resize(guess);
            group_downloads();
            if (guess) be.d2h_async(raw.data(), d_rg_info.p, sizeof(RegInfo) * guess);
            if (!again) be.d2h_async(out, d_rowinfo.p, sizeof(RowInfo) * (size_t)rows);
            int64_t got = 0;
            be.d2h(&got, d_sd_off.p + rows, 8);
            if ((size_t)got <= cap) {
                rg_count = got;
                raw.resize((size_t)got);
                if ((size_t)got > guess) be.d2h(raw.data() + guess, d_rg_info.p + guess, sizeof(RegInfo) * ((size_t)got - guess));
                break;
            }
            cap = (size_t)got + (size_t)got / 8 + 64;
            be.mark("seeds");
        }
        rg_cap_hint = (size_t)rg_count + (size_t)rg_count / 4;
        if (rg_info_h.size() < (size_t)rg_count) rg_info_h.resize((size_t)rg_count);
        bool sorted = true;
        for (int64_t i = 0; i < rg_count; i++) { rg_info_h[(size_t)i] = raw[(size_t)i]; if (i && raw[(size_t)i - 1].key >= raw[(size_t)i].key) sorted = false; }
        if (!sorted) { error = "seed regions out of order"; return -4; }
        infos->swap(raw);
        ids->resize((size_t)rg_count);
        for (int64_t i = 0; i < rg_count; i++) (*ids)[(size_t)i] = (int32_t)i;
        collect_timing_more();
        return 0;
    }
    // per-row scalars of store rows [first, first + count)
    int store_info(int64_t first, int64_t count, RowInfo* out) {
        if (!resident || first < 0 || count < 0 || first + count > ms_count) { error = "rows outside the MUM store"; return -2; }
        if (count == 0) return 0;
        ensure(d_rowinfo, (size_t)count);
        be.launch("store_info", count, StoreInfoOut{store_view(), first, d_rowinfo.p});
        be.mark(nullptr);
        be.d2h(out, d_rowinfo.p, sizeof(RowInfo) * (size_t)count);
        collect_timing_more();
        return 0;
    }
    // the regions the device appended since `first`, as the host wants them: sorted by key, dropped ones left out
    void take_regions(int64_t first, int64_t upto, std::vector<RegInfo>* infos, std::vector<int32_t>* ids) {
        const size_t m = (size_t)(upto - first);
        std::vector<RegInfo> raw(m);
        if (m) be.d2h(raw.data(), d_rg_info.p + first, sizeof(RegInfo) * m);
        if (rg_info_h.size() < (size_t)upto) rg_info_h.resize((size_t)upto);
        std::vector<int32_t> order;
        for (size_t i = 0; i < m; i++) { rg_info_h[(size_t)first + i] = raw[i]; if (raw[i].key >= 0) order.push_back((int32_t)i); }
        std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return raw[(size_t)x].key < raw[(size_t)y].key; });
        infos->clear(); ids->clear();
        for (int32_t i : order) { infos->push_back(raw[(size_t)i]); ids->push_back((int32_t)(first + i)); }
    }
    // setInitialClusters' seed regions (src/parsnp.cpp:2150-2172): both neighbour regions of every accepted anchor (acc: their rows,
    // in list order) by walks over the image, kept when longer than q in every genome; in the reference's push order
    int store_seeds(int64_t table_id, const int32_t* acc, int64_t nacc, int32_t q, std::vector<RegInfo>* infos, std::vector<int32_t>* ids) {
        if (int rc = need_resident(table_id)) return rc;
        if (layout_rows < 0) { error = "the anchor list has not been settled"; return -2; }
        for (int64_t i = 0; i < nacc; i++) if (acc[i] < 0 || acc[i] >= anchor_table_rows) { error = "anchor outside the table"; return -2; }
        rg_count = 0;
        infos->clear(); ids->clear();
        begin_store_call();
        if (nacc == 0) return 0;
        ensure(d_list, (size_t)nacc); ensure(d_rg_count, 2);
        be.h2d(d_list.p, acc, 4 * (size_t)nacc);
        be.mark("seeds");
        size_t cap = std::max<size_t>(rg_cap_hint, (size_t)nacc / 4 + 1024);
        for (;;) {
            ensure(d_rg_start, cap * (size_t)ngen); ensure(d_rg_len, cap * (size_t)ngen); ensure(d_rg_info, cap);
            be.memset(d_rg_count.p, 0, 16);
            be.launch_wave("seed_walk", xcd_grid(nacc), SeedWalk{store_view(), layout_view(d_image.p, false), P, d_list.p, q, d_rg_start.p, d_rg_len.p, d_rg_info.p, d_rg_count.p, (uint64_t)cap, (int64_t)nacc});
            uint64_t got = 0;
            be.d2h(&got, d_rg_count.p, 8);
            if (got <= cap) { rg_count = (int64_t)got; break; }
            cap = (size_t)got + (size_t)got / 8 + 64;
        }
        rg_cap_hint = (size_t)rg_count + (size_t)rg_count / 4;
        be.mark(nullptr);
        take_regions(0, rg_count, infos, ids);
        collect_timing_more();
        return 0;
    }
    // are regions a[i] and b[i] the same in every genome (TRegion operator==)?
    int store_regions_equal(const int32_t* a, const int32_t* b, int64_t n, uint8_t* same) {
        if (!resident) { error = "the session is not in resident mode"; return -2; }
        for (int64_t i = 0; i < n; i++) if (a[i] < 0 || a[i] >= rg_count || b[i] < 0 || b[i] >= rg_count) { error = "region outside the region store"; return -2; }
        if (n == 0) return 0;
        ensure(d_list, (size_t)n); ensure(d_list2, (size_t)n); ensure(d_small8, (size_t)n);
        be.h2d(d_list.p, a, 4 * (size_t)n); be.h2d(d_list2.p, b, 4 * (size_t)n);
        be.launch_wave("regions_equal", n, RegionsEqual{d_list.p, d_list2.p, ngen, d_rg_start.p, d_rg_len.p, d_small8.p});
        be.d2h(same, d_small8.p, (size_t)n);
        return 0;
    }
    // the multi-MUM search of regions of the store (pm_multi_mum_batch on their rows); the candidates become rows
    // [*first_row + off[i], *first_row + off[i + 1]) of the MUM store
    // beside / beside_ctx: host work of the caller that does not depend on the search (pm_store_search_beside).  It runs once, on
    // the calling thread, when the event search has been queued and before the call first waits for the device -- or, where the
    // call returns without getting there, on the way out.  It must not call the engine.
    void (*beside_fn)(void*) = nullptr; void* beside_ctx = nullptr;
    void run_beside() { if (beside_fn) { void (*f)(void*) = beside_fn; beside_fn = nullptr; f(beside_ctx); } }
    int store_search(const int32_t* ids, const int32_t* minsize, int64_t n, int64_t* first_row, int64_t* off, void (*beside)(void*) = nullptr, void* ctx = nullptr) {
        beside_fn = beside; beside_ctx = ctx;
        struct Always { Engine* e; ~Always() { e->run_beside(); } } on_every_way_out{this};
        if (!resident) { error = "the session is not in resident mode"; return -2; }
        std::vector<int64_t> rs((size_t)n), rl((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            if (ids[i] < 0 || ids[i] >= rg_count) { error = "region outside the region store"; return -2; }
            rs[(size_t)i] = rg_info_h[(size_t)ids[i]].ref_start; rl[(size_t)i] = rg_info_h[(size_t)ids[i]].ref_len;
        }
        *first_row = ms_count;
        off[0] = 0;
        if (n == 0) return 0;
        GapBatch gb;
        gb.store_ids = ids; gb.ref_start = rs.data(); gb.ref_len = rl.data();
        BatchResult br;
        const bool keep = want_rows;
        want_rows = true;
        const int rc = run(n, nullptr, nullptr, minsize, &br, false, false, &gb);
        want_rows = keep;
        if (rc) return rc;
        *first_row = br.store_base >= 0 ? br.store_base : ms_count;
        for (int64_t i = 0; i <= n; i++) off[i] = br.off[(size_t)i];
        return 0;
    }
    // One generation of the recursion (doWork, src/parsnp.cpp:173-317) over clusters of waiting regions that the caller found
    // pairwise disjoint in every genome: candidates settled against the image and marked, children appended to the region store.
    int store_validate(const int32_t* regions, const int64_t* row0, const int32_t* cnt, int64_t nreg, const int64_t* cluster_first, int64_t ncl, int32_t q,
                       uint32_t* trouble, std::vector<RegInfo>* kids, std::vector<int32_t>* kid_ids, int64_t info_first = 0, int64_t info_count = 0, RowInfo* info = nullptr,
                       int64_t stage_first = 0, int32_t* second_stage_ran = nullptr, int32_t generation_no = 1, int32_t* done = nullptr) {
        // stage_first > 0: clusters [0, stage_first) are a generation of their own (the first pushed seed, which the reference
        // processes before anything is sorted); the rest -- the generation the caller formed on the assumption that the first leaves
        // no child region -- runs behind it in the same call if that held, and is left untouched if not (*second_stage_ran = 0)
        // done[cluster]: how many regions of the cluster were processed -- all of them, or fewer: none where the cluster meets an
        // earlier one in some genome (it waits for that one and for everything it leads to), the first few where a child sorts
        // before the next waiting region.  done == nullptr: a caller that cannot keep regions waiting; either case is trouble then
        // (bits 3 / 0) and the run must be discarded
        if (!resident || layout_rows < 0) { error = "the anchor list has not been settled"; return -2; }
        kids->clear(); kid_ids->clear(); *trouble = 0;
        if (nreg == 0 || ncl == 0) return 0;
        int64_t total = 0;
        for (int64_t x = 0; x < nreg; x++) {
            if (regions[x] < 0 || regions[x] >= rg_count || row0[x] < 0 || cnt[x] < 0 || row0[x] + cnt[x] > ms_count) { error = "bad generation list"; return -2; }
            total += cnt[x];
        }
        if (cluster_first[0] != 0 || cluster_first[ncl] != nreg) { error = "bad cluster list"; return -2; }
        if (stage_first < 0 || stage_first >= ncl) { error = "bad stage boundary"; return -2; }
        begin_store_call();
        const size_t cap = (size_t)rg_count + 2 * (size_t)total + 16;       // (every accepted candidate has two neighbour regions)
        ensure_keep(d_rg_start, cap * (size_t)ngen, (size_t)rg_count * (size_t)ngen); ensure_keep(d_rg_len, cap * (size_t)ngen, (size_t)rg_count * (size_t)ngen);
        ensure_keep(d_rg_info, cap, (size_t)rg_count);
        const size_t bytes = 4 * (size_t)nreg + 8 * (size_t)nreg + 4 * (size_t)nreg + 8 * ((size_t)ncl + 1) + 64;
        uint8_t* block = (uint8_t*)be.staging(bytes);
        if (!block) { error = "cannot allocate the request staging block"; return -3; }
        int64_t* s_row0 = (int64_t*)block; int64_t* s_first = s_row0 + nreg; int32_t* s_reg = (int32_t*)(s_first + ncl + 1); int32_t* s_cnt = s_reg + nreg;
        memcpy(s_row0, row0, 8 * (size_t)nreg); memcpy(s_first, cluster_first, 8 * ((size_t)ncl + 1)); memcpy(s_reg, regions, 4 * (size_t)nreg); memcpy(s_cnt, cnt, 4 * (size_t)nreg);
        ensure(d_v_row0, (size_t)nreg); ensure(d_v_first, (size_t)ncl + 1); ensure(d_list, (size_t)nreg); ensure(d_list2, (size_t)nreg); ensure(d_rg_count, 4);
        ensure(d_v_done, (size_t)ncl); ensure(d_v_defer, (size_t)ncl); ensure(d_v_involved, (size_t)ncl);
        be.h2d_staged(d_v_row0.p, s_row0, 8 * (size_t)nreg); be.h2d_staged(d_v_first.p, s_first, 8 * ((size_t)ncl + 1));
        be.h2d_staged(d_list.p, s_reg, 4 * (size_t)nreg); be.h2d_staged(d_list2.p, s_cnt, 4 * (size_t)nreg);
        // candidates with a member outside their region are noted for store_order_check (store_kernels.h: ForeignRead); the counter is
        // zeroed by settle_launch, once per anchor list
        foreign_cap = std::min<size_t>((size_t)1 << 16, ((size_t)32 << 20) / (8 * (size_t)ngen));
        ensure(d_foreign, foreign_cap); ensure(d_foreign_masks, foreign_cap * (size_t)ngen); ensure(d_foreign_count, 2);
        ensure_keep(d_ms_key, (size_t)ms_count, (size_t)ms_key_rows); ms_key_rows = ms_count;
        // what every region was processed with (0: it waits), and the accepted members outside their region of this call (OutsideWriteCheck)
        if (rg_pkey_init > rg_count) rg_pkey_init = 0;
        ensure_keep(d_rg_pkey, cap, (size_t)rg_pkey_init);
        if (rg_pkey_init < rg_count) { be.memset(d_rg_pkey.p + rg_pkey_init, 0, 8 * (size_t)(rg_count - rg_pkey_init)); rg_pkey_init = rg_count; }
        constexpr size_t kOutwCap = 4096; constexpr int64_t kOutwWaves = 256;
        ensure(d_outw, kOutwCap); ensure(d_outw_count, 2);
        const int64_t na = stage_first > 0 ? stage_first : ncl;
        uint64_t head[4] = {(uint64_t)rg_count, 0, 0, 0};       // [0] the region counter, [1] the trouble word, [2] the gate of the second stage, [3] collinear test failed
        if (info_count > 0) {      // the scalars of the candidates just decided come back with the same round trip
            if (info_first < 0 || info_first + info_count > ms_count) { error = "rows outside the MUM store"; return -2; }
            ensure(d_rowinfo, (size_t)info_count);
        }
        std::vector<int32_t> done_h((size_t)ncl, 0);
        // the launches of the call and its one wait.  exact = false: the clusters are expected in reference order in every genome
        // (ClustersDisjoint looks; if not, nothing runs).  exact = true: which clusters meet an earlier one is worked out first
        // (ClusterExtents ... ClusterDefer, for the stage that runs clusters side by side) and those wait
        auto generation = [&](bool exact) {
            be.h2d(d_rg_count.p, head, 32);
            be.memset(d_v_done.p, 0, 4 * (size_t)ncl);
            be.memset(d_outw_count.p, 0, 16);
            const uint8_t* defer = nullptr;
            if (exact) {
                be.memset(d_v_defer.p, 0, (size_t)ncl);
                const int64_t c0 = stage_first > 0 ? na : 0, cn = ncl - c0;      // (the first stage of a two-stage call is one cluster)
                if (cn >= 2) {
                    const size_t words = layout_geometry();
                    const uint64_t* b1 = d_once.p; const uint64_t* b2 = d_twice.p; const int32_t* b3 = d_owner.p;
                    ensure(d_once, words); ensure(d_twice, words); ensure(d_owner, words);
                    if (d_once.p != b1 || d_twice.p != b2) { be.memset(d_once.p, 0, 8 * words); be.memset(d_twice.p, 0, 8 * words); }      // (kept all zero between calls)
                    if (d_owner.p != b3) be.memset(d_owner.p, 0, 4 * words);
                    be.launch_wave("cluster_extents", cn, ClusterExtents{ngen, d_rg_start.p, d_rg_len.p, d_list.p, d_v_first.p, layout_view(d_once.p), d_twice.p, d_owner.p, c0, 1});
                    be.launch_wave("cluster_involved", cn, ClusterInvolved{ngen, d_rg_start.p, d_rg_len.p, d_list.p, d_v_first.p, layout_view(d_twice.p, false), d_owner.p, d_v_involved.p, c0});
                    be.launch_wave("cluster_defer", cn, ClusterDefer{ngen, d_rg_start.p, d_rg_len.p, d_list.p, d_v_first.p, d_lay_off.p, d_lay_bits.p, d_owner.p, d_v_involved.p, d_v_defer.p, c0});
                    be.launch_wave("cluster_extents", cn, ClusterExtents{ngen, d_rg_start.p, d_rg_len.p, d_list.p, d_v_first.p, layout_view(d_once.p), d_twice.p, d_owner.p, c0, 0});
                    // ... and where a candidate's member outside its region reads beside a cluster that may mark there (the same scratch arrays,
                    // wiped in between; `twice` lends its memory to the second owner array)
                    int32_t* owner2 = (int32_t*)d_twice.p;
                    be.launch_wave("reader_mark", cn, ReaderMark{store_view(), d_v_row0.p, d_list2.p, ngen, d_rg_start.p, d_rg_len.p, d_list.p, d_v_first.p, layout_view(d_once.p), d_owner.p, owner2, c0, 1});
                    be.launch_wave("marker_look", cn, MarkerLook{store_view(), d_v_row0.p, d_list2.p, ngen, d_v_first.p, layout_view(d_once.p, false), d_owner.p, owner2, d_v_defer.p, c0});
                    be.launch_wave("reader_look", cn, ReaderLook{store_view(), d_v_row0.p, d_list2.p, ngen, d_rg_start.p, d_rg_len.p, d_list.p, d_v_first.p, d_lay_off.p, d_lay_bits.p, owner2, d_v_defer.p, c0});
                    be.launch_wave("reader_mark", cn, ReaderMark{store_view(), d_v_row0.p, d_list2.p, ngen, d_rg_start.p, d_rg_len.p, d_list.p, d_v_first.p, layout_view(d_once.p), d_owner.p, owner2, c0, 0});
                }
                defer = d_v_defer.p;
                exact_cluster_tests++;
            } else be.launch_wave("clusters_disjoint", ncl - 1, ClustersDisjoint{ngen, d_rg_start.p, d_rg_len.p, d_list.p, d_v_first.p, d_rg_count.p + 3, stage_first, force_unsure ? 1 : 0});
            // a stage of the call: `count` clusters from cluster `first` on, behind `gate` (nullptr: none), as generation `gen`
            auto validate = [&](int64_t count, int64_t first, const uint64_t* gate, int32_t gen) {
                be.launch_wave("cluster_validate", xcd_grid(count),
                               ClusterValidate{store_view(), layout_view(d_image.p), P, d_rg_start.p, d_rg_len.p, d_rg_info.p, d_rg_count.p, (uint64_t)cap,
                                               d_list.p, d_v_row0.p, d_list2.p, d_v_first.p, q, (uint32_t*)(d_rg_count.p + 1), count, first, gate, d_rg_count.p + 3,
                                               d_foreign.p, d_foreign_count.p, (uint64_t)foreign_cap, d_foreign_masks.p, d_ms_key.p, gen, d_recwords.p, defer, d_v_done.p,
                                               d_rg_pkey.p, d_outw.p, d_outw_count.p, (uint64_t)kOutwCap});
            };
            validate(na, 0, nullptr, generation_no);
            if (stage_first > 0) {
                be.launch("stage_gate", 1, StageGate{d_rg_count.p, (uint64_t)rg_count, force_gate ? 1 : 0});
                validate(ncl - na, na, d_rg_count.p + 2, generation_no + 1);
            }
            be.launch_wave("outside_write_check", kOutwWaves,
                           OutsideWriteCheck{store_view(), d_rg_start.p, d_rg_len.p, d_rg_info.p, d_rg_pkey.p, d_rg_count.p, (uint64_t)cap, d_list.p, d_outw.p, d_outw_count.p, (uint64_t)kOutwCap,
                                             d_ms_key.p, anchor_table_rows, (uint32_t*)(d_rg_count.p + 1), kOutwWaves});
            if (info_count > 0) be.launch("store_info", info_count, StoreInfoOut{store_view(), info_first, d_rowinfo.p});
            be.mark(nullptr);
            group_downloads();
            if (info_count > 0) be.d2h_async(info, d_rowinfo.p, sizeof(RowInfo) * (size_t)info_count);
            be.d2h_async(&foreign_seen, d_foreign_count.p, 8);
            be.d2h_async(&outside_writes_call, d_outw_count.p, 8);
            be.d2h_async(done_h.data(), d_v_done.p, 4 * (size_t)ncl);
            be.d2h(head, d_rg_count.p, 32);
        };
        be.mark("validate");
        // a session whose genomes have once held the clusters in another order (an inversion) asks the exact question at once:
        // the collinear test would fail again, at the price of a round trip
        generation(clusters_out_of_order);
        if (head[3] != 0 && !clusters_out_of_order) {
            // some genome does not hold the clusters in reference order: nothing has been validated (ClusterValidate saw the word)
            clusters_out_of_order = true;
            head[0] = (uint64_t)rg_count; head[1] = head[2] = head[3] = 0;
            be.mark("validate");
            generation(true);
        }
        *trouble = (uint32_t)head[1];
        outside_writes += (int64_t)outside_writes_call;
        const bool ran2 = stage_first > 0 && head[2] == 0;
        if (second_stage_ran) *second_stage_ran = ran2 ? 1 : 0;
        for (int64_t cl = 0; cl < ncl; cl++) {
            if (stage_first > 0 && cl >= na && !ran2) { done_h[(size_t)cl] = 0; continue; }
            const int64_t size = cluster_first[cl + 1] - cluster_first[cl];
            if (done_h[(size_t)cl] < size) {
                deferred_regions += size - done_h[(size_t)cl];
                if (!done && !*trouble) *trouble |= done_h[(size_t)cl] == 0 ? 8u : 1u;
            }
        }
        if (done) memcpy(done, done_h.data(), 4 * (size_t)ncl);
        if (head[0] > cap) { error = "region store overflow"; return -4; }
        const int64_t before = rg_count;
        rg_count = (int64_t)head[0];
        take_regions(before, rg_count, kids, kid_ids);
        collect_timing_more();
        return 0;
    }
    // chain()'s test of MUM cur[i] against the open chain's last MUM back[i] (setFinalClusters :2596-2700): verdict 0 = every
    // genome's gap inside [0, d] (min_gap / max_gap for the caller's ratio test), 1 = the chain closes, 2 = a reverse member: from the rows
    int store_judge(const int32_t* cur, const int32_t* back, int64_t n, int32_t d, int32_t* min_gap, int32_t* max_gap, uint8_t* verdict) {
        if (!resident) { error = "the session is not in resident mode"; return -2; }
        for (int64_t i = 0; i < n; i++) if (cur[i] < 0 || cur[i] >= ms_count || back[i] < 0 || back[i] >= ms_count) { error = "rows outside the MUM store"; return -2; }
        if (n == 0) return 0;
        begin_store_call();
        ensure(d_list, (size_t)n); ensure(d_list2, (size_t)n); ensure(d_j_min, (size_t)n); ensure(d_j_max, (size_t)n); ensure(d_small8, (size_t)n);
        int32_t* block = (int32_t*)be.staging(8 * (size_t)n);
        if (!block) { error = "cannot allocate the request staging block"; return -3; }
        memcpy(block, cur, 4 * (size_t)n); memcpy(block + n, back, 4 * (size_t)n);
        be.h2d_staged(d_list.p, block, 4 * (size_t)n); be.h2d_staged(d_list2.p, block + n, 4 * (size_t)n);
        be.mark("judge");
        be.launch_wave("judge_pairs", n, JudgePairs{store_view(), d_list.p, d_list2.p, d, d_j_min.p, d_j_max.p, d_small8.p});
        be.mark(nullptr);
        be.d2h_async(min_gap, d_j_min.p, 4 * (size_t)n); be.d2h_async(max_gap, d_j_max.p, 4 * (size_t)n);
        be.d2h(verdict, d_small8.p, (size_t)n);
        collect_timing_more();
        return 0;
    }
    // the listed MUMs leave the layout (filterRandom1 :415-418, filterRandomClustersSimple1 :460-466)
    int store_unmark(const int32_t* rows, int64_t n) {
        if (!resident || layout_rows < 0) { error = "the anchor list has not been settled"; return -2; }
        for (int64_t i = 0; i < n; i++) if (rows[i] < 0 || rows[i] >= ms_count) { error = "rows outside the MUM store"; return -2; }
        if (n == 0) return 0;
        ensure(d_list, (size_t)n);
        be.h2d(d_list.p, rows, 4 * (size_t)n);
        be.launch("store_unmark", n * ngen, StoreUnmark{store_view(), layout_view(d_image.p), d_list.p});
        return 0;
    }
    // setInterClusterRegions (:2389-2460) for consecutive LCBs given by (last MUM of one, first MUM of the next); rows of the
    // fillers that are made, [n_made][ngen] each, in pair order
    int store_fill(const int32_t* last_of, const int32_t* first_of_next, int64_t n, uint8_t* add, std::vector<int64_t>* starts, std::vector<int64_t>* ends) {
        if (!resident || layout_rows < 0) { error = "the anchor list has not been settled"; return -2; }
        for (int64_t i = 0; i < n; i++) if (last_of[i] < 0 || last_of[i] >= ms_count || first_of_next[i] < 0 || first_of_next[i] >= ms_count) { error = "rows outside the MUM store"; return -2; }
        starts->clear(); ends->clear();
        if (n == 0) return 0;
        begin_store_call();
        const size_t ngz = (size_t)ngen;
        ensure(d_list, (size_t)n); ensure(d_list2, (size_t)n); ensure(d_small8, (size_t)n); ensure(d_f_start, (size_t)n * ngz); ensure(d_f_end, (size_t)n * ngz);
        be.h2d(d_list.p, last_of, 4 * (size_t)n); be.h2d(d_list2.p, first_of_next, 4 * (size_t)n);
        be.mark("fill");
        be.launch_wave("fill_between", n, FillBetween{store_view(), layout_view(d_image.p, false), P, d_list.p, d_list2.p, d_small8.p, d_f_start.p, d_f_end.p});
        be.mark(nullptr);
        be.d2h(add, d_small8.p, (size_t)n);
        std::vector<int32_t> which;
        for (int64_t i = 0; i < n; i++) if (add[i] == 1) which.push_back((int32_t)i);
        if (!which.empty()) {      // the rows of the fillers, packed on the device: one copy
            const size_t m = which.size();
            ensure(d_list, m); ensure(d_f_pack, 2 * m * ngz);
            be.h2d(d_list.p, which.data(), 4 * m);
            be.launch("fill_gather", (int64_t)m * ngen, FillGather{d_list.p, ngen, d_f_start.p, d_f_end.p, d_f_pack.p});
            std::vector<int64_t> pack(2 * m * ngz);
            be.d2h(pack.data(), d_f_pack.p, 8 * pack.size());
            starts->resize(m * ngz); ends->resize(m * ngz);
            for (size_t k = 0; k < m; k++) {
                memcpy(starts->data() + k * ngz, pack.data() + (2 * k) * ngz, 8 * ngz);
                memcpy(ends->data() + k * ngz, pack.data() + (2 * k + 1) * ngz, 8 * ngz);
            }
        }
        collect_timing_more();
        return 0;
    }
    // Phases C-D where their list logic is order-free (store_kernels.h, "phases C-D on the store"): the accepted rows sorted by
    // reference start, chained, the short LCBs dissolved, chained again, the fillers counted -- one queue of launches, no round
    // trip.  Two halves: begin() queues the work and the copies, end() waits for them; the caller may work in between.
    // expect: the number of accepted rows (the caller's MUM list).
    struct ChainInfo { int64_t n_in, lcbs_first, lcbs_dissolved, mums_dissolved, n_mums, n_lcbs, n_fillers; uint64_t trouble; };
    // After the last generation: every candidate that read marks outside its region, decided again the way the reference's order
    // had them (store_kernels.h: ForeignRead and what follows it).  *trouble != 0: the order would show.  store_chain_begin runs
    // the same check first (bit kChainOrder of pm_chain_info.trouble); store_order_check is for a caller that does not queue phases C-D.
    void order_check_launch(uint32_t* word, uint32_t bit) {
        const int64_t cnt = (int64_t)std::min<uint64_t>(foreign_seen, (uint64_t)foreign_cap);
        const int64_t rows = ms_count - layout_rows;
        if (cnt <= 0 || rows <= 0) return;      // (nothing was noted)
        ensure(d_hits, kHitCap); ensure(d_hit_count, 2); ensure(d_hit_owned, kHitCap * (size_t)ngen); ensure(d_hit_present, kHitCap * (size_t)ngen);
        be.memset(d_hit_count.p, 0, 16);
        const Store S = store_view();
        const Layout L = layout_view(d_image.p, false);
        be.launch_wave("foreign_bound", cnt, ForeignBound{S, L, P, d_rg_start.p, d_rg_len.p, d_foreign.p, cnt, d_foreign_masks.p, d_recwords.p, d_hits.p, d_hit_count.p, (uint64_t)kHitCap,
                                                         d_hit_owned.p, d_hit_present.p, word, bit});
        const int64_t chunks = (rows + kScanRows - 1) / kScanRows, waves = 8192;
        be.launch_wave("foreign_scan", waves, ForeignScan{S, d_rg_start.p, d_rg_len.p, d_ms_key.p, d_foreign.p, d_hits.p, d_hit_count.p, (uint64_t)kHitCap, d_hit_owned.p, d_hit_present.p,
                                                         layout_rows, ms_count, chunks, waves});
        be.launch_wave("foreign_decide_hits", (int64_t)kHitCap, ForeignDecideHits{S, L, P, d_rg_start.p, d_rg_len.p, d_foreign.p, d_foreign_masks.p, d_hits.p, d_hit_count.p, (uint64_t)kHitCap,
                                                                                 d_hit_owned.p, d_hit_present.p, word, bit});
        if (order_debug) {      // (pm_session_tune "order_debug": waits for the queue and says what the check had to do)
            uint64_t nh = 0;
            be.d2h(&nh, d_hit_count.p, 8);
            fprintf(stderr, "[order check] %ld noted candidates, %ld left to the scan (launched for %ld), %ld recursion rows\n", (long)cnt, (long)nh, (long)kHitCap, (long)rows);
        }
    }
    int store_order_check(uint32_t* trouble) {
        if (!resident || layout_rows < 0) { error = "the anchor list has not been settled"; return -2; }
        *trouble = 0;
        begin_store_call();
        ensure(d_rg_count, 4);
        be.mark("validate");
        be.memset(d_rg_count.p + 1, 0, 8);
        order_check_launch((uint32_t*)(d_rg_count.p + 1), 1u);
        be.mark(nullptr);
        uint64_t word = 0;
        be.d2h(&word, d_rg_count.p + 1, 8);
        *trouble = (uint32_t)word;
        collect_timing_more();
        return 0;
    }
    int store_chain_begin(int64_t expect, int32_t d, float diag_diff, int64_t c) {
        if (!resident || layout_rows < 0) { error = "the anchor list has not been settled"; return -2; }
        if (expect <= 0 || expect > ms_count) { error = "bad MUM count"; return -2; }
        if (chain_event) { be.event_wait(chain_event); be.event_release(chain_event); chain_event = nullptr; }
        begin_store_call();
        const size_t rows = (size_t)ms_count, cap = (size_t)expect;
        ensure(d_ch_flag, rows + 1); ensure(d_ch_pos, rows + 1);
        ensure(d_ch_key, cap); ensure(d_ch_val, cap); ensure(d_ch_skey, cap); ensure(d_ch_srow, cap); ensure(d_ch_key2, cap); ensure(d_ch_row2, cap);
        ensure(d_ch_verdict, cap); ensure(d_ch_head, cap + 1); ensure(d_ch_hpos, cap + 1); ensure(d_ch_survive, cap + 1); ensure(d_ch_spos, cap + 1);
        ensure(d_ch_lcblen, cap); ensure(d_ch_hdr, kChWords); ensure(d_ch_outrow, cap); ensure(d_ch_outhead, cap);
        const size_t host_bytes = 8 * (size_t)kChWords + 4 * cap + cap;
        if (host_bytes > chain_host_cap) {
            if (chain_host) be.pinned_free(chain_host);
            chain_host_cap = 0;
            chain_host = (uint8_t*)be.pinned_alloc(host_bytes + host_bytes / 4 + 64);
            if (!chain_host) { error = "cannot allocate the chain result block"; return -3; }
            chain_host_cap = host_bytes + host_bytes / 4 + 64;
        }
        chain_cap = (int64_t)cap;
        const Store S = store_view();
        be.mark("chain");
        {
            const ClearJob jobs[] = {{d_ch_hdr.p, 8 * (size_t)kChWords, 0}, {d_ch_lcblen.p, 8 * cap, 0}};
            be.clear_many(jobs, 2);
        }
        order_check_launch((uint32_t*)(d_ch_hdr.p + kChTrouble), (uint32_t)kChainOrder);      // (before anything leaves the layout)
        be.launch("chain_flag", (int64_t)rows + 1, ChainFlag{S, (int64_t)rows, d_ch_flag.p});
        be.exclusive_scan(d_ch_flag.p, d_ch_pos.p, rows + 1);
        be.launch("chain_keys", (int64_t)rows, ChainKeys{S, d_ch_pos.p, d_ch_key.p, d_ch_val.p, (int64_t)cap});
        be.sort_pairs(d_ch_key.p, d_ch_skey.p, d_ch_val.p, d_ch_srow.p, cap, bits_for((uint64_t)glen_h[0]));
        const int64_t* n1 = d_ch_pos.p + rows;
        int64_t* hdr = d_ch_hdr.p;
        uint64_t* trouble = (uint64_t*)(hdr + kChTrouble);
        // diag_diff in bases: a MUM may be passed, so the verdicts against the list predecessor are followed by the windows (store_kernels.h,
        // "phases C-D on the store"), and a dissolved MUM leaves the layout only when the windows of BOTH passes had nothing to report
        const bool bp = diag_diff > 1.0f;
        int64_t* back = nullptr;
        if (bp) {
            ensure(d_ch_back, cap); ensure(d_ch_wflag, cap + 1); ensure(d_ch_wpos, cap + 1); ensure(d_ch_wend, cap); ensure(d_ch_wverdict, cap);
            ensure(d_ch_wlist, (size_t)kChainStarts); ensure(d_ch_wkeep, (size_t)kChainStarts);
            back = d_ch_back.p;
        }
        const int64_t nstarts = std::min<int64_t>((int64_t)cap, kChainStarts);
        auto windows = [&](const uint64_t* row, const int64_t* n) {
            be.launch("chain_starts", (int64_t)cap + 1, ChainHeads{d_ch_verdict.p, n, d_ch_wflag.p, kChPass});
            be.exclusive_scan(d_ch_wflag.p, d_ch_wpos.p, cap + 1);
            be.launch_wave("chain_window", (int64_t)cap, ChainWindow{S, row, n, d, diag_diff, d_ch_verdict.p, chain_window, d_ch_wpos.p, d_ch_wlist.p, d_ch_wend.p, d_ch_wverdict.p});
            be.launch("chain_select", 1, ChainSelect{n, d_ch_wpos.p, d_ch_wlist.p, d_ch_wend.p, d_ch_wkeep.p, trouble});
            be.launch_wave("chain_window_fill", nstarts, ChainWindowFill{n, d_ch_wpos.p, d_ch_wlist.p, d_ch_wend.p, d_ch_wverdict.p, d_ch_wkeep.p, trouble, d_ch_verdict.p, back});
        };
        // first pass: verdicts, chains, their lengths, the dissolved ones out of the layout and out of the list
        be.launch_wave("chain_judge", (int64_t)cap, ChainJudge{S, d_ch_skey.p, d_ch_srow.p, n1, d, diag_diff, d_ch_verdict.p, trouble, force_chain_tie ? 1 : 0, back});
        be.launch("chain_judge_reverse", (int64_t)cap, ChainJudgeReverse{S, d_ch_srow.p, n1, d, diag_diff, d_ch_verdict.p});
        if (bp) windows(d_ch_srow.p, n1);
        be.launch("chain_heads", (int64_t)cap + 1, ChainHeads{d_ch_verdict.p, n1, d_ch_head.p, kChClose});
        be.exclusive_scan(d_ch_head.p, d_ch_hpos.p, cap + 1);
        be.launch("chain_lcb_sum", (int64_t)cap, ChainLcbSum{S, d_ch_srow.p, n1, d_ch_hpos.p, d_ch_verdict.p, d_ch_lcblen.p, hdr});
        be.launch("chain_dissolve", (int64_t)cap + 1, ChainDissolve{n1, d_ch_hpos.p, d_ch_head.p, d_ch_verdict.p, d_ch_lcblen.p, c, d_ch_survive.p, hdr});
        if (!bp) be.launch_wave("chain_unmark", (int64_t)cap, ChainUnmark{S, layout_view(d_image.p), d_ch_srow.p, n1, d_ch_survive.p, nullptr});
        be.exclusive_scan(d_ch_survive.p, d_ch_spos.p, cap + 1);
        be.launch("chain_compact", (int64_t)cap, ChainCompact{n1, d_ch_survive.p, d_ch_spos.p, d_ch_skey.p, d_ch_srow.p, d_ch_key2.p, d_ch_row2.p, hdr});
        // second pass (the reference chains again after dissolving, :3261-3268), then the fillers between the final LCBs
        const int64_t* n2 = hdr + kChN2;
        be.launch_wave("chain_judge", (int64_t)cap, ChainJudge{S, d_ch_key2.p, d_ch_row2.p, n2, d, diag_diff, d_ch_verdict.p, trouble, 0, back});
        be.launch("chain_judge_reverse", (int64_t)cap, ChainJudgeReverse{S, d_ch_row2.p, n2, d, diag_diff, d_ch_verdict.p});
        if (bp) {
            windows(d_ch_row2.p, n2);
            be.launch_wave("chain_unmark", (int64_t)cap, ChainUnmark{S, layout_view(d_image.p), d_ch_srow.p, n1, d_ch_survive.p, trouble});
        }
        be.launch("chain_heads", (int64_t)cap + 1, ChainHeads{d_ch_verdict.p, n2, d_ch_head.p, kChClose});
        be.exclusive_scan(d_ch_head.p, d_ch_hpos.p, cap + 1);
        if (cap > 1) be.launch_wave("chain_fill", (int64_t)cap - 1, ChainFill{S, layout_view(d_image.p, false), P, d_ch_row2.p, n2, d_ch_head.p, back, hdr});
        be.launch("chain_out", (int64_t)cap, ChainOut{d_ch_row2.p, n2, d_ch_head.p, d_ch_hpos.p, d_ch_verdict.p, d_ch_outrow.p, d_ch_outhead.p, hdr});
        be.mark(nullptr);
        be.d2h_async_pinned(chain_host, hdr, 8 * (size_t)kChWords);
        be.d2h_async_pinned(chain_host + 8 * (size_t)kChWords, d_ch_outrow.p, 4 * cap);
        be.d2h_async_pinned(chain_host + 8 * (size_t)kChWords + 4 * cap, d_ch_outhead.p, cap);
        chain_event = be.event_record();
        chain_pending = true;
        return 0;
    }
    int store_chain_end(ChainInfo* info, const int32_t** rows, const uint8_t** heads) {
        if (!chain_pending) { error = "no chain call in flight"; return -2; }
        chain_pending = false;
        if (chain_event) { be.event_wait(chain_event); be.event_release(chain_event); chain_event = nullptr; }
        else be.sync();
        const int64_t* h = (const int64_t*)chain_host;
        *info = ChainInfo{h[kChN1], h[kChLcb1], h[kChLcbDissolved], h[kChMumDissolved], h[kChN2], h[kChLcb2], h[kChFill], (uint64_t)h[kChTrouble]};
        *rows = (const int32_t*)(chain_host + 8 * (size_t)kChWords);
        *heads = chain_host + 8 * (size_t)kChWords + 4 * (size_t)chain_cap;
        collect_timing_more();
        chain_passed[0] = h[kChPass1]; chain_passed[1] = h[kChPass2];
        if (info->n_in != chain_cap) { error = "the MUM list of the caller and the accepted rows of the store differ"; return -2; }
        return 0;
    }
    // rows of the store for the host (the XMFA writer after phase D; a caller that falls back to the host route): start per genome
    // with the trim applied (raw: as the search delivered them) + strand byte.  rows == nullptr: rows [first, first + n)
    int store_rows(const int32_t* rows, int64_t first, int64_t n, bool raw, int32_t* out_start, uint8_t* out_strand) {
        if (!resident) { error = "the session is not in resident mode"; return -2; }
        if (n == 0) return 0;
        const size_t ngz = (size_t)ngen;
        if (!rows) {
            if (first < 0 || first + n > ms_count) { error = "rows outside the MUM store"; return -2; }
            if (raw) {      // contiguous and untouched: straight copies
                be.d2h_async(out_start, d_anchor_start.p + (size_t)first * ngz, 4 * (size_t)n * ngz);
                be.d2h(out_strand, d_ms_strand.p + (size_t)first * ngz, (size_t)n * ngz);
                return 0;
            }
        } else for (int64_t i = 0; i < n; i++) if (rows[i] < 0 || rows[i] >= ms_count) { error = "rows outside the MUM store"; return -2; }
        // in pieces: the gathered copy of a 60 000-row list is 60 MB of device memory otherwise
        const int64_t piece = std::max<int64_t>(1, (int64_t)((32u << 20) / (5 * ngz)));
        ensure(d_list, (size_t)std::min(n, piece)); ensure(d_o_start, (size_t)std::min(n, piece) * ngz); ensure(d_o_strand, (size_t)std::min(n, piece) * ngz);
        std::vector<int32_t> seq;
        for (int64_t at = 0; at < n; at += piece) {
            const int64_t m = std::min(piece, n - at);
            const int32_t* src = rows ? rows + at : nullptr;
            if (!src) { seq.resize((size_t)m); for (int64_t i = 0; i < m; i++) seq[(size_t)i] = (int32_t)(first + at + i); src = seq.data(); }
            be.h2d(d_list.p, src, 4 * (size_t)m);
            be.launch("store_rows", m * ngen, StoreRowsOut{store_view(), d_list.p, d_o_start.p, d_o_strand.p, raw ? 1 : 0});
            be.d2h_async(out_start + (size_t)at * ngz, d_o_start.p, 4 * (size_t)m * ngz);
            be.d2h(out_strand + (size_t)at * ngz, d_o_strand.p, (size_t)m * ngz);
        }
        return 0;
    }
    // the layout as the host keeps it (write_unaligned reads it): one block, words of genome j at off[j]
    int store_layout(uint64_t* out, int64_t words) {
        if (!resident || layout_rows < 0) { error = "the anchor list has not been settled"; return -2; }
        if ((size_t)words != layout_geometry()) { error = "layout size does not match"; return -2; }
        be.d2h(out, d_image.p, 8 * (size_t)words);
        return 0;
    }
    std::vector<int64_t> lay_off_h;
    // The unaligned runs of the layout (store_kernels.h, "the unaligned runs"): what parsnp.unalign lists, without the image
    // leaving the device.  Both calls read the image and change nothing in it.
    // the count pass and its scans, queued: per block the runs, kept starts and kept ends before it; per genome the totals
    int64_t unalign_launch() {
        const size_t ngz = (size_t)ngen;
        layout_geometry();
        if (un_blk_h.size() != ngz + 1) {
            un_blk_h.assign(ngz + 1, 0);
            for (size_t j = 0; j < ngz; j++) un_blk_h[j + 1] = un_blk_h[j] + ((glen_h[j] + 1 + 63) / 64 + kUnalignWords - 1) / kUnalignWords;
            ensure(d_un_blk, ngz + 1);
            be.h2d(d_un_blk.p, un_blk_h.data(), 8 * (ngz + 1));
        }
        const int64_t nblocks = un_blk_h[ngz];
        ensure(d_un_cnt, 3 * ((size_t)nblocks + 1)); ensure(d_un_scan, 3 * ((size_t)nblocks + 1)); ensure(d_un_tot, 2 * ngz);
        const size_t row = (size_t)nblocks + 1;
        be.launch_wave("unalign_count", nblocks, UnalignCount{unalign_geom(), nblocks, d_un_cnt.p, d_un_cnt.p + row, d_un_cnt.p + 2 * row});
        for (size_t k = 0; k < 3; k++) be.exclusive_scan(d_un_cnt.p + k * row, d_un_scan.p + k * row, row);
        be.launch("unalign_totals", (int64_t)ngen, UnalignTotals{d_un_blk.p, d_un_scan.p, d_un_scan.p + row, d_un_tot.p});
        return nblocks;
    }
    UnalignGeom unalign_geom() {
        int32_t steps = 0;
        while (((int64_t)1 << steps) < ngen) steps++;
        return UnalignGeom{d_image.p, d_lay_off.p, d_lay_bits.p, d_un_blk.p, ngen, steps};
    }
    // per genome: the number of all runs and of the kept ones (the call's one wait)
    int store_unalign_count(int64_t* all_runs, int64_t* kept_runs) {
        if (!resident || layout_rows < 0) { error = "the anchor list has not been settled"; return -2; }
        begin_store_call();
        be.mark("unalign_count");
        unalign_launch();
        be.mark(nullptr);
        std::vector<int64_t> tot(2 * (size_t)ngen);
        be.d2h(tot.data(), d_un_tot.p, 8 * tot.size());
        for (size_t j = 0; j < (size_t)ngen; j++) { all_runs[j] = tot[2 * j]; kept_runs[j] = tot[2 * j + 1]; }
        collect_timing_more();
        return 0;
    }
    // start, end (inclusive) and ordinal of every kept run, genome after genome, in position order: n = the sum of the kept counts.
    // The counts are taken again (the image may have changed since the count call: the sum is checked after the one wait, and a
    // rank past n is never written)
    int store_unalign_write(int32_t* start, int32_t* end, int32_t* ordinal, int64_t n) {
        if (!resident || layout_rows < 0) { error = "the anchor list has not been settled"; return -2; }
        begin_store_call();
        be.mark("unalign_write");
        const int64_t nblocks = unalign_launch();
        const size_t row = (size_t)nblocks + 1, nz = (size_t)n;
        ensure(d_un_out, 3 * std::max<size_t>(nz, 1));
        be.launch_wave("unalign_write", nblocks, UnalignWrite{unalign_geom(), nblocks, d_un_scan.p, d_un_scan.p + row, d_un_scan.p + 2 * row, d_un_out.p, d_un_out.p + nz, d_un_out.p + 2 * nz, n});
        be.mark(nullptr);
        int64_t total[2] = {0, 0};      // kept starts, kept ends
        be.d2h_async(&total[0], d_un_scan.p + row + nblocks, 8);
        be.d2h_async(&total[1], d_un_scan.p + 2 * row + nblocks, 8);
        if (n) { be.d2h_async(start, d_un_out.p, 4 * nz); be.d2h_async(end, d_un_out.p + nz, 4 * nz); be.d2h_async(ordinal, d_un_out.p + 2 * nz, 4 * nz); }
        be.sync();
        collect_timing_more();
        if (total[0] != n || total[1] != n) { error = "the number of kept runs does not match the layout"; return -2; }
        return 0;
    }
    std::vector<int64_t> un_blk_h;

    // Core SNP columns and SNP distances (snp_kernels.h).  A collection is independent of the session's genomes: n rows, columns
    // added chunk by chunk.  Every add waits once, for its counts: the planes grow by the chunk's core SNPs, not by its columns.
    int snp_begin(int32_t n_rows) {
        if (n_rows < 2) { error = "a SNP collection needs at least 2 rows"; return -2; }
        if (n_rows > kSnpMaxRows) { error = "a SNP collection takes at most " + std::to_string(kSnpMaxRows) + " rows"; return -5; }
        snp_rows = n_rows; snp_cols = 0; snp_v = 0; snp_up_bytes = 0; snp_dist_ready = false; boot_dist_ready = false; rec_forget();
        ensure(d_snp_counts, 4);
        ClearJob job{d_snp_counts.p, 4 * sizeof(uint64_t), 0};
        be.clear_many(&job, 1);
        return 0;
    }
    int snp_add(int64_t n_cols, int64_t pitch, const uint8_t* chars, int64_t* totals) {
        if (snp_rows < 2) { error = "no SNP collection has been started"; return -2; }
        if (snp_cols + n_cols >= ((int64_t)1 << 31)) { error = "a SNP collection takes fewer than 2^31 columns"; return -5; }
        timing.clear();
        snp_dist_ready = false; boot_dist_ready = false; rec_forget();
        const size_t n = (size_t)snp_rows, nc = (size_t)n_cols;
        uint64_t counts[4] = {0, 0, 0, 0};
        if (n_cols) {
            // the chunk, its rows packed side by side (pitch n_cols on the device), through the page-locked staging block
            uint8_t* stage = (uint8_t*)be.staging(n * nc);
            if (!stage) throw DeviceOutOfMemory{n * nc};
            for (size_t r = 0; r < n; r++) memcpy(stage + r * nc, chars + r * (size_t)pitch, nc);
            ensure(d_snp_chunk, n * nc); ensure(d_snp_flag, nc + 1); ensure(d_snp_rank, nc + 1);
            be.h2d_staged(d_snp_chunk.p, stage, n * nc);
            snp_up_bytes += n * nc;
            be.mark("snp_classify");
            be.launch("snp_classify", n_cols, SnpClassify{d_snp_chunk.p, n_cols, n_cols, snp_rows, d_snp_flag.p, d_snp_counts.p});
            be.mark("snp_scan");
            be.exclusive_scan(d_snp_flag.p, d_snp_rank.p, nc + 1);
            be.mark(nullptr);
        }
        be.d2h(counts, d_snp_counts.p, sizeof counts);
        const int64_t v1 = (int64_t)counts[1];
        if (v1 > snp_v) {
            const size_t w0 = (size_t)((snp_v + 63) / 64), w1 = (size_t)((v1 + 63) / 64);
            ensure_keep(d_snp_col, (size_t)v1, (size_t)snp_v);
            ensure_keep(d_snp_lo, w1 * n, w0 * n); ensure_keep(d_snp_hi, w1 * n, w0 * n);
            be.mark("snp_pack");
            be.launch("snp_rank", n_cols, SnpRank{d_snp_flag.p, d_snp_rank.p, snp_v, snp_cols, d_snp_col.p});
            be.launch_wave("snp_pack", (int64_t)w1 - snp_v / 64, SnpPack{d_snp_chunk.p, n_cols, snp_rows, d_snp_col.p, snp_cols, snp_v, v1, d_snp_lo.p, d_snp_hi.p});
            be.mark(nullptr);
            be.sync();      // (the staging block and the chunk are free for the next add)
            snp_v = v1;
        }
        snp_cols += n_cols;
        collect_timing_more();
        if (totals) { totals[0] = snp_cols; totals[1] = (int64_t)counts[0]; totals[2] = (int64_t)counts[1]; totals[3] = (int64_t)counts[2]; }
        return 0;
    }
    int64_t snp_core() const { return snp_v; }
    // col[v]: the index of core SNP v among all columns added; letters: n_rows x V, row-major, upper case (either may be null)
    int snp_columns(int64_t* col, uint8_t* letters) {
        if (snp_rows < 2) { error = "no SNP collection has been started"; return -2; }
        if (!snp_v) return 0;
        const size_t n = (size_t)snp_rows, v = (size_t)snp_v, words = (v + 63) / 64;
        if (col) be.d2h_async(col, d_snp_col.p, 8 * v);
        std::vector<uint64_t> lo, hi;
        if (letters) {
            lo.resize(words * n); hi.resize(words * n);
            be.d2h_async(lo.data(), d_snp_lo.p, 8 * words * n); be.d2h_async(hi.data(), d_snp_hi.p, 8 * words * n);
        }
        be.sync();
        if (letters)
            for (size_t r = 0; r < n; r++)
                for (size_t w = 0; w < words; w++) {
                    const uint64_t l = lo[w * n + r], h = hi[w * n + r];
                    const size_t upto = std::min<size_t>(64, v - w * 64);
                    for (size_t t = 0; t < upto; t++) letters[r * v + w * 64 + t] = snp_letter((uint32_t)(((l >> t) & 1) | (((h >> t) & 1) << 1)));
                }
        return 0;
    }
    // dist: n_rows x n_rows, row-major
    int snp_distances(int32_t* dist) {
        if (snp_rows < 2) { error = "no SNP collection has been started"; return -2; }
        const size_t n = (size_t)snp_rows;
        if (!snp_v) { memset(dist, 0, 4 * n * n); snp_dist_ready = true; return 0; }
        timing.clear();
        ensure(d_snp_dist, n * n);
        snp_dist_ready = true;
        const int32_t tiles = (snp_rows + kSnpTile - 1) / kSnpTile;
        const int64_t words = (snp_v + 63) / 64;
        const uint64_t last_mask = (snp_v & 63) ? ((1ull << (snp_v & 63)) - 1) : ~0ull;
        be.mark("snp_dist");
        be.launch_wave("snp_dist", (int64_t)tiles * tiles, SnpDist{d_snp_lo.p, d_snp_hi.p, snp_rows, words, last_mask, tiles, d_snp_dist.p});
        be.mark(nullptr);
        be.d2h(dist, d_snp_dist.p, 4 * n * n);
        collect_timing_more();
        return 0;
    }
    int32_t snp_rows = 0; int64_t snp_cols = 0, snp_v = 0; uint64_t snp_up_bytes = 0;
    bool snp_dist_ready = false;      // the collection's distances have been computed (nj_tree may take them from the device)

    // Neighbour joining (nj_kernels.h) over a caller's matrix or over the distances of the session's SNP collection,
    // which are still on the device.  The number of joins is known: all 2 (n - 3) + 2 launches are queued without a wait, and the
    // records come back in one download.  joins: n - 3 records (may be null for n == 3), last: one.
    int nj_tree(int32_t n, const int32_t* dist, NjJoinRec* joins, NjLastRec* last) {
        if (n < 3) { error = "a neighbour-joining tree needs at least 3 rows"; return -2; }
        if (n > kNjMaxRows) { error = "a neighbour-joining tree takes at most " + std::to_string(kNjMaxRows) + " rows"; return -5; }
        const size_t N = (size_t)n;
        if (!dist) {
            if (!snp_dist_ready || snp_rows != n) { error = "no SNP distances of " + std::to_string(n) + " rows have been computed in this session"; return -2; }
        } else {
            for (size_t i = 0; i < N; i++) {
                if (dist[i * N + i] != 0) { error = "the distance matrix has a non-zero diagonal"; return -2; }
                for (size_t j = i + 1; j < N; j++) {
                    if (dist[i * N + j] < 0) { error = "the distance matrix has a negative entry"; return -2; }
                    if (dist[i * N + j] != dist[j * N + i]) { error = "the distance matrix is not symmetric"; return -2; }
                }
            }
        }
        timing.clear();
        ensure(d_nj_D, N * N); ensure(d_nj_R, N); ensure(d_nj_active, N); ensure(d_nj_q, N); ensure(d_nj_j, N);
        ensure(d_nj_joins, N); ensure(d_nj_last, 1);
        const int32_t* src;
        if (dist) {
            ensure(d_nj_dist, N * N);
            be.h2d(d_nj_dist.p, dist, 4 * N * N);
            src = d_nj_dist.p;
        } else {
            if (!snp_v) {      // no core SNP: the distances call wrote zeros to the caller and launched nothing
                ensure(d_snp_dist, N * N);
                ClearJob job{d_snp_dist.p, 4 * N * N, 0};
                be.clear_many(&job, 1);
            }
            src = d_snp_dist.p;
        }
        be.mark("nj");
        be.launch_wave("nj_init", n, NjInit{src, n, d_nj_D.p, d_nj_R.p, d_nj_active.p});
        for (int32_t t = 0; t + 3 < n; t++) {
            const int32_t r = n - t;
            be.launch_wave("nj_rowmin", n, NjRowMin{d_nj_D.p, d_nj_R.p, d_nj_active.p, n, r, d_nj_q.p, d_nj_j.p});
            be.launch("nj_join", kNjGroup, NjJoin{d_nj_D.p, d_nj_R.p, d_nj_active.p, n, r, d_nj_q.p, d_nj_j.p, d_nj_joins.p + t});
        }
        be.launch_wave("nj_last", 1, NjLast{d_nj_D.p, d_nj_active.p, n, d_nj_last.p});
        be.mark(nullptr);
        if (n > 3 && joins) be.d2h_async(joins, d_nj_joins.p, (N - 3) * sizeof(NjJoinRec));
        be.d2h_async(last, d_nj_last.p, sizeof(NjLastRec));
        be.sync();
        collect_timing_more();
        return 0;
    }

    // Bootstrap support of the SNP tree (boot_kernels.h).  Replicates are worked off in batches: the draw counters
    // of a batch stay within kBootCounterBytes and the D matrices of a batch of trees within kBootTreeBytes ("boot_batch" forces the
    // size; no result depends on it).  The replicate distances and the join records of all replicates stay on the device for the
    // next call.  Nothing here touches the state of snp_distances / nj_tree.
    static constexpr size_t kBootCounterBytes = (size_t)256 << 20, kBootTreeBytes = (size_t)1 << 30;
    int64_t boot_batch = 0;      // pm_session_tune "boot_batch": replicates (trees) per batch, 0: the largest that fits
    int boot_distances(int32_t reps, uint64_t seed, const uint8_t* weights, int64_t pitch, uint8_t* weights_out, int32_t* dist_out) {
        if (snp_rows < 2) { error = "no SNP collection has been started"; return -2; }
        if (reps < 1) { error = "a bootstrap needs at least 1 replicate"; return -2; }
        if (reps > kBootMaxReps) { error = "a bootstrap takes at most " + std::to_string(kBootMaxReps) + " replicates"; return -5; }
        const size_t n = (size_t)snp_rows, v = (size_t)snp_v, nrep = (size_t)reps;
        if (weights) {
            if (pitch < snp_v) { error = "the pitch of the weights is smaller than the number of core SNP columns"; return -2; }
            for (size_t b = 0; b < nrep; b++)
                for (size_t c = 0; c < v; c++)
                    if (weights[b * (size_t)pitch + c] > kBootMaxWeight) { error = "a column weight above " + std::to_string(kBootMaxWeight); return -2; }
        }
        if (v * sizeof(uint32_t) > kBootCounterBytes) { error = "the draw counters of one replicate do not fit"; return -5; }
        timing.clear();
        boot_dist_ready = false;
        ensure(d_boot_dist, nrep * n * n);
        if (!v) {      // no column, no draw: every distance is 0
            ClearJob job{d_boot_dist.p, 4 * nrep * n * n, 0};
            be.clear_many(&job, 1);
            if (dist_out) memset(dist_out, 0, 4 * nrep * n * n);
            be.sync();
            boot_dist_ready = true; boot_reps = reps;
            return 0;
        }
        const size_t batch = std::min(nrep, boot_batch ? (size_t)boot_batch : kBootCounterBytes / (v * sizeof(uint32_t)));
        const size_t words = (v + 63) / 64;
        const int32_t tiles = (snp_rows + kSnpTile - 1) / kSnpTile;
        ensure(d_boot_planes, batch * kBootPlanes * words); ensure(d_boot_w8, batch * v);
        if (!weights) ensure(d_boot_cnt, batch * v);
        std::vector<uint8_t> packed;
        for (size_t b0 = 0; b0 < nrep; b0 += batch) {
            const size_t nb = std::min(batch, nrep - b0);
            be.mark("boot_draw");
            if (weights) {
                packed.resize(nb * v);
                for (size_t b = 0; b < nb; b++) memcpy(packed.data() + b * v, weights + (b0 + b) * (size_t)pitch, v);
                be.h2d(d_boot_w8.p, packed.data(), nb * v);
            } else {
                ClearJob job{d_boot_cnt.p, nb * v * sizeof(uint32_t), 0};
                be.clear_many(&job, 1);
                be.launch("boot_draw", (int64_t)(nb * v), BootDraw{seed, (int64_t)b0, snp_v, d_boot_cnt.p});
            }
            be.launch_wave("boot_pack", (int64_t)(nb * words), BootPack{d_boot_cnt.p, weights ? d_boot_w8.p : nullptr, snp_v, (int64_t)words, d_boot_w8.p, d_boot_planes.p});
            be.mark("boot_dist");
            const int64_t groups = ((int64_t)nb + kBootGroup - 1) / kBootGroup;
            be.launch_wave("snp_dist_boot", (int64_t)tiles * tiles * groups,
                           SnpDistBoot{d_snp_lo.p, d_snp_hi.p, snp_rows, (int64_t)words, tiles, d_boot_planes.p, (int32_t)nb, d_boot_dist.p + b0 * n * n});
            be.mark(nullptr);
            if (weights_out && !weights) be.d2h_async(weights_out + b0 * v, d_boot_w8.p, nb * v);      // (queued in front of the next batch's launches)
        }
        if (weights && weights_out) for (size_t b = 0; b < nrep; b++) memcpy(weights_out + b * v, weights + b * (size_t)pitch, v);
        if (dist_out) be.d2h_async(dist_out, d_boot_dist.p, 4 * nrep * n * n);
        be.sync();
        collect_timing_more();
        boot_dist_ready = true; boot_reps = reps;
        return 0;
    }
    int32_t boot_reps = 0; bool boot_dist_ready = false;      // replicate distances of boot_reps x snp_rows x snp_rows are on the device
    int32_t boot_trees = 0, boot_trees_n = 0;                 // join records of boot_trees trees of boot_trees_n leaves are on the device

    static const char* nj_matrix_fault(const int32_t* dist, size_t N) {
        for (size_t i = 0; i < N; i++) {
            if (dist[i * N + i] != 0) return "the distance matrix has a non-zero diagonal";
            for (size_t j = i + 1; j < N; j++) {
                if (dist[i * N + j] < 0) return "the distance matrix has a negative entry";
                if (dist[i * N + j] != dist[j * N + i]) return "the distance matrix is not symmetric";
            }
        }
        return nullptr;
    }
    // count trees of one n, the trees of a batch in lock step: 2 (n - 3) + 2 launches a batch, no wait before the download
    int nj_trees(int32_t n, int32_t count, const int32_t* dist, NjJoinRec* joins, NjLastRec* last) {
        if (n < 3) { error = "a neighbour-joining tree needs at least 3 rows"; return -2; }
        if (n > kNjMaxRows) { error = "a neighbour-joining tree takes at most " + std::to_string(kNjMaxRows) + " rows"; return -5; }
        if (count < 1) { error = "at least 1 tree"; return -2; }
        if (count > kBootMaxReps) { error = "at most " + std::to_string(kBootMaxReps) + " trees a call"; return -5; }
        const size_t N = (size_t)n, cnt = (size_t)count, M = N - 3;
        if (!dist) {
            if (!boot_dist_ready || snp_rows != n || count > boot_reps) { error = "no distances of " + std::to_string(count) + " replicates of " + std::to_string(n) + " rows have been computed in this session"; return -2; }
        } else {
            for (size_t b = 0; b < cnt; b++)
                if (const char* fault = nj_matrix_fault(dist + b * N * N, N)) { error = fault; return -2; }
        }
        if (N * N * sizeof(double) > kBootTreeBytes) { error = "the matrix of one tree does not fit"; return -5; }
        timing.clear();
        boot_trees = 0;
        const size_t batch = std::min(cnt, boot_batch ? (size_t)boot_batch : kBootTreeBytes / (N * N * sizeof(double)));
        ensure(d_bt_D, batch * N * N); ensure(d_bt_R, batch * N); ensure(d_bt_active, batch * N); ensure(d_bt_q, batch * N); ensure(d_bt_j, batch * N);
        ensure(d_bt_joins, cnt * M + 1); ensure(d_bt_last, cnt);
        if (dist) ensure(d_bt_dist, batch * N * N);
        for (size_t b0 = 0; b0 < cnt; b0 += batch) {
            const size_t nb = std::min(batch, cnt - b0);
            const int32_t* src = d_boot_dist.p + b0 * N * N;
            if (dist) { be.h2d(d_bt_dist.p, dist + b0 * N * N, 4 * nb * N * N); src = d_bt_dist.p; }
            be.mark("boot_nj");
            be.launch_wave("nj_init_b", (int64_t)(nb * N), NjInitB{src, n, d_bt_D.p, d_bt_R.p, d_bt_active.p});
            for (int32_t t = 0; t + 3 < n; t++) {
                const int32_t r = n - t;
                be.launch_wave("nj_rowmin_b", (int64_t)(nb * N), NjRowMinB{d_bt_D.p, d_bt_R.p, d_bt_active.p, n, r, d_bt_q.p, d_bt_j.p});
                be.launch("nj_join_b", (int64_t)nb * kNjGroup, NjJoinB{d_bt_D.p, d_bt_R.p, d_bt_active.p, n, r, d_bt_q.p, d_bt_j.p, d_bt_joins.p + b0 * M, t});
            }
            be.launch_wave("nj_last_b", (int64_t)nb, NjLastB{d_bt_D.p, d_bt_active.p, n, d_bt_last.p + b0});
            be.mark(nullptr);
        }
        if (M && joins) be.d2h_async(joins, d_bt_joins.p, cnt * M * sizeof(NjJoinRec));
        if (last) be.d2h_async(last, d_bt_last.p, cnt * sizeof(NjLastRec));
        be.sync();
        collect_timing_more();
        boot_trees = count; boot_trees_n = n;
        return 0;
    }
    // a caller's n - 3 records: 0 <= i < j < n, both slots still active
    static bool nj_records_valid(const NjJoinRec* J, size_t N, std::vector<uint8_t>& active) {
        active.assign(N, 1);
        for (size_t t = 0; t + 3 < N; t++) {
            const int32_t i = J[t].i, j = J[t].j;
            if (i < 0 || j <= i || (size_t)j >= N || !active[(size_t)i] || !active[(size_t)j]) return false;
            active[(size_t)j] = 0;
        }
        return true;
    }
    // support[t]: in how many of the count trees the split of join t of the main tree occurs (as a set of leaves)
    int nj_support(int32_t n, const NjJoinRec* main_joins, int32_t count, const NjJoinRec* rep_joins, int32_t* support) {
        if (n < 3) { error = "a neighbour-joining tree needs at least 3 rows"; return -2; }
        if (n > kNjMaxRows) { error = "a neighbour-joining tree takes at most " + std::to_string(kNjMaxRows) + " rows"; return -5; }
        if (count < 1) { error = "at least 1 tree"; return -2; }
        if (count > kBootMaxReps) { error = "at most " + std::to_string(kBootMaxReps) + " trees a call"; return -5; }
        if (n == 3) return 0;      // no internal branch
        const size_t N = (size_t)n, cnt = (size_t)count, M = N - 3, W = (N + 63) / 64;
        std::vector<uint8_t> scratch;
        if (!nj_records_valid(main_joins, N, scratch)) { error = "a join record of the main tree is not a join of two active slots"; return -2; }
        if (rep_joins) {
            for (size_t b = 0; b < cnt; b++)
                if (!nj_records_valid(rep_joins + b * M, N, scratch)) { error = "a join record of tree " + std::to_string(b) + " is not a join of two active slots"; return -2; }
        } else if (boot_trees_n != n || count > boot_trees) { error = "no records of " + std::to_string(count) + " trees of " + std::to_string(n) + " leaves are on the device"; return -2; }
        timing.clear();
        const size_t batch = std::min(cnt, boot_batch ? (size_t)boot_batch : std::max<size_t>(1, kBootTreeBytes / (N * N * sizeof(double))));
        ensure(d_bs_mj, M); ensure(d_bs_msets, M * W); ensure(d_bs_mkeys, M); ensure(d_bs_support, M);
        ensure(d_bs_rsets, batch * M * W); ensure(d_bs_rkeys, batch * M);
        if (rep_joins) ensure(d_bs_rj, batch * M);
        be.h2d(d_bs_mj.p, main_joins, M * sizeof(NjJoinRec));
        be.mark("boot_support");
        ClearJob job{d_bs_support.p, M * sizeof(uint32_t), 0};
        be.clear_many(&job, 1);
        be.launch_wave("boot_splits", 1, BootSplits{d_bs_mj.p, n, (int32_t)W, d_bs_msets.p, d_bs_mkeys.p});
        be.mark(nullptr);
        for (size_t b0 = 0; b0 < cnt; b0 += batch) {
            const size_t nb = std::min(batch, cnt - b0);
            const NjJoinRec* src = d_bt_joins.p + b0 * M;
            if (rep_joins) { be.h2d(d_bs_rj.p, rep_joins + b0 * M, nb * M * sizeof(NjJoinRec)); src = d_bs_rj.p; }
            be.mark("boot_support");
            be.launch_wave("boot_splits", (int64_t)nb, BootSplits{src, n, (int32_t)W, d_bs_rsets.p, d_bs_rkeys.p});
            be.launch_wave("boot_match", (int64_t)nb, BootMatch{d_bs_msets.p, d_bs_mkeys.p, d_bs_rsets.p, d_bs_rkeys.p, n, (int32_t)W, d_bs_support.p});
            be.mark(nullptr);
        }
        be.d2h(support, d_bs_support.p, M * sizeof(int32_t));
        collect_timing_more();
        return 0;
    }

    // Recombination scan of the SNP collection (rec_kernels.h).  The transposed planes are made once per collection
    // (any add forgets them) and stay on the device; so do the matrices of the last rec_incompat for rec_test.  Windows are worked off
    // in batches: a launch takes at most kRecLaunchItems wavefronts, an upload of caller's matrices at most kRecUploadBytes
    // ("rec_batch" forces the windows of a batch; no result depends on it: a window's keys come from its number g, not its place).
    static constexpr size_t kRecMatrixBytes = (size_t)1 << 30, kRecUploadBytes = (size_t)256 << 20;
    static constexpr int64_t kRecLaunchItems = (int64_t)1 << 30;
    int64_t rec_batch = 0;      // pm_session_tune "rec_batch": windows per batch, 0: the largest that fits
    bool rec_tp_ready = false, rec_inc_ready = false;      // the transposed planes / the matrices of rec_sizes are on the device
    std::vector<int32_t> rec_sizes;                         // the sites of every window of those matrices
    void rec_forget() { rec_tp_ready = false; rec_inc_ready = false; }
    int32_t rec_row_blocks() const { return (snp_rows + 63) / 64; }
    // queues RecTranspose and RecInform unless the planes of this collection are there already (phase rec_sites)
    void rec_queue_sites() {
        if (rec_tp_ready || !snp_v) return;
        const int32_t RB = rec_row_blocks();
        const int64_t words = (snp_v + 63) / 64;
        ensure(d_rec_tp, (size_t)snp_v * 2 * (size_t)RB); ensure(d_rec_flag, (size_t)snp_v);
        be.mark("rec_sites");
        be.launch_wave("rec_transpose", words * RB, RecTranspose{d_snp_lo.p, d_snp_hi.p, snp_rows, snp_v, RB, d_rec_tp.p});
        be.launch("rec_inform", snp_v, RecInform{d_rec_tp.p, snp_rows, RB, d_rec_flag.p});
        be.mark(nullptr);
        rec_tp_ready = true;
    }
    int rec_sites(uint8_t* informative, int64_t* n_informative) {
        if (snp_rows < 2) { error = "no SNP collection has been started"; return -2; }
        timing.clear();
        int64_t count = 0;
        if (snp_v) {
            rec_queue_sites();
            std::vector<uint8_t> own;
            uint8_t* f = informative;
            if (!f) { own.resize((size_t)snp_v); f = own.data(); }
            be.d2h(f, d_rec_flag.p, (size_t)snp_v);
            for (int64_t c = 0; c < snp_v; c++) count += f[c];
        }
        collect_timing_more();
        if (n_informative) *n_informative = count;
        return 0;
    }
    // the windows of a call: -2 / -5 with `error` set, or 0 with the sizes
    int rec_windows_of(int64_t n_windows, const int64_t* win_off, int64_t n_sites, std::vector<int32_t>* sizes) {
        if (n_windows < 0 || (n_windows && !win_off)) { error = "bad window list"; return -2; }
        sizes->assign((size_t)n_windows, 0);
        if (n_windows && (win_off[0] < 0 || (n_sites >= 0 && win_off[n_windows] > n_sites))) { error = "the windows lie outside the site list"; return -2; }
        for (int64_t w = 0; w < n_windows; w++)
            if (win_off[w + 1] - win_off[w] < 2) { error = "window " + std::to_string(w) + " has fewer than 2 sites (win_off must ascend)"; return -2; }
        for (int64_t w = 0; w < n_windows; w++) {
            if (win_off[w + 1] - win_off[w] > kRecMaxSites) { error = "a window takes at most " + std::to_string(kRecMaxSites) + " sites"; return -5; }
            (*sizes)[(size_t)w] = (int32_t)(win_off[w + 1] - win_off[w]);
        }
        return 0;
    }
    static std::vector<int64_t> rec_matrix_offsets(const std::vector<int32_t>& sizes) {
        std::vector<int64_t> off(sizes.size() + 1, 0);
        for (size_t w = 0; w < sizes.size(); w++) off[w + 1] = off[w] + (int64_t)sizes[w] * sizes[w];
        return off;
    }
    int rec_incompat(int64_t n_sites, const int64_t* sites, int64_t n_windows, const int64_t* win_off, uint8_t* inc_out) {
        if (snp_rows < 2) { error = "no SNP collection has been started"; return -2; }
        if (n_sites < 0 || (n_sites && !sites)) { error = "bad site list"; return -2; }
        for (int64_t i = 0; i < n_sites; i++) if (sites[i] < 0 || sites[i] >= snp_v) { error = "site " + std::to_string(i) + " is no core SNP column of the collection"; return -2; }
        std::vector<int32_t> sizes;
        if (const int rc = rec_windows_of(n_windows, win_off, n_sites, &sizes)) return rc;
        const std::vector<int64_t> moff = rec_matrix_offsets(sizes);
        if ((size_t)moff.back() > kRecMatrixBytes) { error = "the matrices of the windows of one call do not fit"; return -5; }
        timing.clear();
        rec_inc_ready = false;
        const size_t nw = (size_t)n_windows, total = (size_t)moff.back();
        if (nw) {
            ensure(d_rec_sites, (size_t)n_sites); ensure(d_rec_woff, nw + 1); ensure(d_rec_moff, nw + 1); ensure(d_rec_inc, total);
            be.h2d(d_rec_sites.p, sites, 8 * (size_t)n_sites);
            be.h2d(d_rec_woff.p, win_off, 8 * (nw + 1));
            be.h2d(d_rec_moff.p, moff.data(), 8 * (nw + 1));
            rec_queue_sites();
            const size_t full = (size_t)((kRecMaxSites / kRecTile) * (kRecMaxSites / kRecTile));
            const size_t batch = std::min(nw, rec_batch ? (size_t)rec_batch : (size_t)kRecLaunchItems / full);
            be.mark("rec_incompat");
            for (size_t b0 = 0; b0 < nw; b0 += batch) {
                const size_t nb = std::min(batch, nw - b0);
                int32_t kmax = 0;
                for (size_t w = b0; w < b0 + nb; w++) kmax = std::max(kmax, sizes[w]);
                const int32_t tiles = (kmax + kRecTile - 1) / kRecTile;
                be.launch_wave("rec_incompat", (int64_t)nb * tiles * tiles,
                               RecIncompat{d_rec_tp.p, snp_rows, rec_row_blocks(), d_rec_sites.p, d_rec_woff.p + b0, d_rec_moff.p + b0, tiles, d_rec_inc.p});
            }
            be.mark(nullptr);
            if (inc_out) be.d2h_async(inc_out, d_rec_inc.p, total);
            be.sync();
            collect_timing_more();
        }
        rec_sizes.swap(sizes); rec_inc_ready = true;
        return 0;
    }
    int rec_test(int64_t n_windows, const int64_t* win_off, const uint8_t* inc, int32_t near, int32_t perms, uint64_t seed, const int64_t* win_id,
                 int32_t* phi, int32_t* le) {
        if (near < 1) { error = "near must be at least 1"; return -2; }
        if (perms < 1) { error = "a permutation test needs at least 1 permutation"; return -2; }
        std::vector<int32_t> sizes;
        if (const int rc = rec_windows_of(n_windows, win_off, -1, &sizes)) return rc;
        if (perms > kRecMaxPerms) { error = "a permutation test takes at most " + std::to_string(kRecMaxPerms) + " permutations"; return -5; }
        if (!inc && (!rec_inc_ready || sizes != rec_sizes)) { error = "no matrices of these windows are on the device"; return -2; }
        if (n_windows && (!phi || !le)) { error = "bad argument"; return -2; }
        const std::vector<int64_t> moff = rec_matrix_offsets(sizes);
        if ((size_t)moff.back() > kRecMatrixBytes) { error = "the matrices of the windows of one call do not fit"; return -5; }
        timing.clear();
        const size_t nw = (size_t)n_windows, total = (size_t)moff.back();
        if (!nw) return 0;
        std::vector<int64_t> woff(nw + 1, 0);
        for (size_t w = 0; w < nw; w++) woff[w + 1] = woff[w] + sizes[w];
        ensure(d_rec_woff, nw + 1); ensure(d_rec_moff, nw + 1); ensure(d_rec_phi, nw); ensure(d_rec_le, nw);
        if (inc) { rec_inc_ready = false; ensure(d_rec_inc, total); }
        be.h2d(d_rec_woff.p, woff.data(), 8 * (nw + 1));
        be.h2d(d_rec_moff.p, moff.data(), 8 * (nw + 1));
        if (win_id) { ensure(d_rec_wid, nw); be.h2d(d_rec_wid.p, win_id, 8 * nw); }
        ClearJob job{d_rec_le.p, nw * sizeof(uint32_t), 0};
        be.clear_many(&job, 1);
        const int32_t chunks = (perms + kRecChunk - 1) / kRecChunk;
        size_t batch = std::min(nw, rec_batch ? (size_t)rec_batch : (size_t)(kRecLaunchItems / chunks));
        for (size_t b0 = 0; b0 < nw; ) {
            size_t nb = std::min(batch, nw - b0);
            if (inc && !rec_batch)      // (a caller's matrices go up batch by batch)
                while (nb > 1 && (size_t)(moff[b0 + nb] - moff[b0]) > kRecUploadBytes) nb--;
            if (inc) be.h2d(d_rec_inc.p + moff[b0], inc + moff[b0], (size_t)(moff[b0 + nb] - moff[b0]));
            int32_t kmax = 0;
            for (size_t w = b0; w < b0 + nb; w++) kmax = std::max(kmax, sizes[w]);
            const int64_t* wid = win_id ? d_rec_wid.p + b0 : nullptr;
            be.mark("rec_permute");
            if (kmax <= 128)
                be.launch_wave("rec_permute", (int64_t)nb * chunks, RecPermute<128>{d_rec_inc.p, d_rec_woff.p + b0, d_rec_moff.p + b0, wid, (int64_t)b0, near, perms, chunks, seed, d_rec_phi.p + b0, d_rec_le.p + b0});
            else
                be.launch_wave("rec_permute", (int64_t)nb * chunks, RecPermute<256>{d_rec_inc.p, d_rec_woff.p + b0, d_rec_moff.p + b0, wid, (int64_t)b0, near, perms, chunks, seed, d_rec_phi.p + b0, d_rec_le.p + b0});
            be.mark(nullptr);
            b0 += nb;
        }
        be.d2h_async(phi, d_rec_phi.p, 4 * nw); be.d2h_async(le, d_rec_le.p, 4 * nw);
        be.sync();
        collect_timing_more();
        if (inc) { rec_sizes.swap(sizes); rec_inc_ready = true; }
        return 0;
    }

    // Extension of the LCB ends into their flanks (ext_kernels.h).  A pair is a (job, row): pair p is row p of the
    // call's list.  The reach goes pair by pair in launches of at most `ext_batch` pairs (a job's pairs may straddle launches: the cut
    // runs after the last); the alignment goes in batches of whole jobs of about as many pairs, whose paths and column starts stay in
    // a workspace of the batch's size.  Only descriptors go up; reaches, `best` (for the tests), `used` and the rows come back.
    static constexpr int64_t kExtBatchPairs = 1 << 16;
    int64_t ext_batch = 0;      // pm_session_tune "ext_batch": pairs per launch, 0: kExtBatchPairs
    // the jobs of a call: -2 / -5 with `error` set, or 0 with the job of every pair
    int ext_check(const ExtParams& prm, int64_t n_jobs, const int64_t* row_off, const ExtRow* rows, std::vector<int32_t>* row_job) {
        if (prm.max_flank < 16 || prm.max_flank > kExtMaxFlank || prm.band < 1 || prm.band > kExtMaxBand || prm.match < 1 || prm.match > 15 || prm.mismatch < 0 ||
            prm.mismatch > 15 || prm.gap < 1 || prm.gap > 15 || prm.ani < 50 || prm.ani > 100 || prm.min_len < 1 || prm.min_len > prm.max_flank) {
            error = "extension parameters out of range (16 <= max_flank <= 512, 1 <= band <= 63, 1 <= match <= 15, 0 <= mismatch <= 15, 1 <= gap <= 15, "
                    "50 <= ani <= 100, 1 <= min_len <= max_flank)";
            return -2;
        }
        if (n_jobs < 0 || !row_off || (n_jobs && !rows) || row_off[0] != 0) { error = "bad job list"; return -2; }
        for (int64_t j = 0; j < n_jobs; j++)
            if (row_off[j + 1] - row_off[j] < 2) { error = "job " + std::to_string(j) + " has fewer than 2 rows (row_off must ascend)"; return -2; }
        if (n_jobs >= ((int64_t)1 << 31) || row_off[n_jobs] >= ((int64_t)1 << 31)) { error = "too many jobs or rows in one call"; return -5; }
        for (int64_t j = 0; j < n_jobs; j++)
            if (row_off[j + 1] - row_off[j] > kExtMaxRows) { error = "a job takes at most " + std::to_string(kExtMaxRows) + " rows"; return -5; }
        row_job->assign((size_t)row_off[n_jobs], 0);
        for (int64_t j = 0; j < n_jobs; j++)
            for (int64_t p = row_off[j]; p < row_off[j + 1]; p++) {
                const ExtRow& r = rows[p];
                (*row_job)[(size_t)p] = (int32_t)j;
                if (r.genome < 0 || r.genome >= ngen || (r.step != 1 && r.step != -1) || r.len < 0 || (r.complement != 0 && r.complement != 1)) { error = "row " + std::to_string(p) + ": bad descriptor"; return -2; }
                if (r.len > prm.max_flank) { error = "row " + std::to_string(p) + " is longer than max_flank"; return -5; }
                const int64_t end = r.first + (int64_t)(r.len - 1) * r.step;
                if (r.len && (r.first < 0 || r.first >= glen_h[(size_t)r.genome] || end < 0 || end >= glen_h[(size_t)r.genome])) { error = "row " + std::to_string(p) + " leaves its genome"; return -2; }
            }
        return 0;
    }
    void ext_upload(int64_t n_jobs, const int64_t* row_off, const ExtRow* rows, const std::vector<int32_t>& row_job) {
        const size_t np = row_job.size();
        ensure(d_ext_rows, np); ensure(d_ext_job, np); ensure(d_ext_off, (size_t)n_jobs + 1);
        be.h2d(d_ext_rows.p, rows, sizeof(ExtRow) * np);
        be.h2d(d_ext_job.p, row_job.data(), 4 * np);
        be.h2d(d_ext_off.p, row_off, 8 * ((size_t)n_jobs + 1));
    }
    int ext_reach(const ExtParams& prm, int64_t n_jobs, const int64_t* row_off, const ExtRow* rows, int32_t* reach, int32_t* best) {
        std::vector<int32_t> row_job;
        if (const int rc = ext_check(prm, n_jobs, row_off, rows, &row_job)) return rc;
        if (n_jobs && !reach) { error = "bad argument"; return -2; }
        timing.clear();
        if (!n_jobs) return 0;
        const int64_t np = (int64_t)row_job.size(), pitch = prm.max_flank + 1;
        const int64_t batch = ext_batch ? ext_batch : kExtBatchPairs;
        ext_upload(n_jobs, row_off, rows, row_job);
        ensure(d_ext_bits, (size_t)np * kExtBitWords); ensure(d_ext_reach, (size_t)n_jobs);
        if (best) ensure(d_ext_best, (size_t)std::min(batch, np) * (size_t)pitch);
        for (int64_t p0 = 0; p0 < np; p0 += batch) {
            const int64_t nb = std::min(batch, np - p0);
            be.mark("ext_reach");
            be.launch_wave("ext_reach", nb, ExtReach{P, d_ext_rows.p, d_ext_job.p, d_ext_off.p, prm, p0, d_ext_bits.p, best ? d_ext_best.p : nullptr});
            be.mark(nullptr);
            if (best) be.d2h(best + p0 * pitch, d_ext_best.p, 4 * (size_t)(nb * pitch));
        }
        be.mark("ext_cut");
        be.launch_wave("ext_cut", n_jobs, ExtCut{d_ext_off.p, prm, d_ext_bits.p, d_ext_reach.p});
        be.mark(nullptr);
        be.d2h_async(reach, d_ext_reach.p, 4 * (size_t)n_jobs);
        be.sync();
        collect_timing_more();
        return 0;
    }
    int ext_align(const ExtParams& prm, int64_t n_jobs, const int64_t* row_off, const ExtRow* rows, const int32_t* reach, int64_t max_cols, const int64_t* out_off,
                  uint8_t* out_rows, int32_t* cols, int32_t* used) {
        std::vector<int32_t> row_job;
        if (const int rc = ext_check(prm, n_jobs, row_off, rows, &row_job)) return rc;
        if (n_jobs && (!reach || !out_off || !out_rows || !cols || !used)) { error = "bad argument"; return -2; }
        if (max_cols < 2 * (int64_t)prm.max_flank) { error = "max_cols must be at least 2 max_flank"; return -2; }
        for (int64_t j = 0; j < n_jobs; j++) {
            if (reach[j] < 0 || reach[j] > rows[row_off[j]].len) { error = "job " + std::to_string(j) + ": the reach lies outside the reference flank"; return -2; }
            for (int64_t p = row_off[j]; p < row_off[j + 1]; p++)      // (line A of a row's table has a cell only up to len + band)
                if (reach[j] > rows[p].len + prm.band) { error = "job " + std::to_string(j) + ": line " + std::to_string(reach[j]) + " of row " + std::to_string(p) + " has no cell"; return -2; }
            if (out_off[j] < 0) { error = "bad output offset"; return -2; }
        }
        timing.clear();
        if (!n_jobs) return 0;
        const int64_t np = (int64_t)row_job.size();
        const int64_t batch = ext_batch ? ext_batch : kExtBatchPairs;
        ext_upload(n_jobs, row_off, rows, row_job);
        ensure(d_ext_reach, (size_t)n_jobs); ensure(d_ext_cols, (size_t)n_jobs); ensure(d_ext_used, (size_t)np);
        be.h2d(d_ext_reach.p, reach, 4 * (size_t)n_jobs);
        std::vector<uint8_t> stage;
        for (int64_t j0 = 0; j0 < n_jobs; ) {      // whole jobs, about `batch` pairs
            int64_t j1 = j0 + 1;
            while (j1 < n_jobs && row_off[j1 + 1] - row_off[j0] <= batch) j1++;
            const int64_t p0 = row_off[j0], nb = row_off[j1] - p0, nj = j1 - j0;
            ensure(d_ext_pk, (size_t)nb * (size_t)(prm.max_flank + 1)); ensure(d_ext_cs, (size_t)nj * (size_t)(prm.max_flank + 2)); ensure(d_ext_out, (size_t)(nb * max_cols));
            be.memset(d_ext_out.p, 0, (size_t)(nb * max_cols));      // (what no kernel writes -- past column C, the rows of a dropped job -- reaches the caller as zeros)
            be.mark("ext_trace");
            if (prm.max_flank <= 256)
                be.launch_wave("ext_trace", nb, ExtTrace<256>{P, d_ext_rows.p, d_ext_job.p, d_ext_off.p, prm, p0, d_ext_reach.p, d_ext_pk.p, d_ext_used.p});
            else
                be.launch_wave("ext_trace", nb, ExtTrace<512>{P, d_ext_rows.p, d_ext_job.p, d_ext_off.p, prm, p0, d_ext_reach.p, d_ext_pk.p, d_ext_used.p});
            be.mark(nullptr);
            be.mark("ext_merge");
            be.launch_wave("ext_width", nj, ExtWidth{d_ext_off.p, prm, j0, p0, d_ext_reach.p, d_ext_pk.p, d_ext_cs.p, d_ext_cols.p});
            be.launch_wave("ext_merge", nb, ExtMerge{P, d_ext_rows.p, d_ext_job.p, prm, j0, p0, d_ext_reach.p, d_ext_cols.p, d_ext_pk.p, d_ext_cs.p, max_cols, d_ext_out.p});
            be.mark(nullptr);
            bool natural = true;      // the caller's rows lie as the batch's do: one copy
            for (int64_t j = j0; j < j1; j++) natural = natural && out_off[j] - out_off[j0] == (row_off[j] - p0) * max_cols;
            if (natural) be.d2h(out_rows + out_off[j0], d_ext_out.p, (size_t)(nb * max_cols));
            else {
                stage.resize((size_t)(nb * max_cols));
                be.d2h(stage.data(), d_ext_out.p, stage.size());
                for (int64_t j = j0; j < j1; j++) memcpy(out_rows + out_off[j], stage.data() + (row_off[j] - p0) * max_cols, (size_t)((row_off[j + 1] - row_off[j]) * max_cols));
            }
            j0 = j1;
        }
        be.d2h_async(cols, d_ext_cols.p, 4 * (size_t)n_jobs); be.d2h_async(used, d_ext_used.p, 4 * (size_t)np);
        be.sync();
        collect_timing_more();
        return 0;
    }

    // The suffix array of the flagged regions of a batch (dense_kernels.h) and their rep' (after RepeatLength, which skipped them).
    // One segmented prefix-doubling sort over all of them; every round waits for its count of distinct ranks (8 bytes) -- a round
    // trip per round, on this path only.
    int dense_build(const RegionInfo* R, int64_t nreg, int64_t nflag) {
        std::vector<int32_t> fi_h((size_t)nreg, -1), list_h;
        std::vector<int64_t> start_h(1, 0);
        for (int64_t r = 0; r < nreg; r++)
            if (dense_h[(size_t)r]) { fi_h[(size_t)r] = (int32_t)list_h.size(); list_h.push_back((int32_t)r); start_h.push_back(start_h.back() + R[r].nR); }
        const int64_t n = start_h.back();
        ensure(d_dfi, (size_t)nreg); ensure(d_dlist, (size_t)nflag); ensure(d_dstart, (size_t)nflag + 1);
        be.h2d(d_dfi.p, fi_h.data(), 4 * (size_t)nreg);
        be.h2d(d_dlist.p, list_h.data(), 4 * (size_t)nflag);
        be.h2d(d_dstart.p, start_h.data(), 8 * ((size_t)nflag + 1));
        ensure(d_dval2, (size_t)std::max<int64_t>(n, 1));
        dense_rounds = 0;
        if (n == 0) return 0;
        if (n >= (1ll << 31) || (uint64_t)nflag * 5 >= ((uint64_t)1 << 32)) { error = "suffix-array batch too large"; return -5; }
        ensure(d_dkey, (size_t)n); ensure(d_dval, (size_t)n); ensure(d_dkey2, (size_t)n);
        ensure(d_dhead, (size_t)n + 1); ensure(d_dfirst, (size_t)n + 1); ensure(d_dlcp, (size_t)n);
        DenseLevels L{};
        ensure(d_drank[0], (size_t)n);
        be.launch("dense_rank0", n, DenseRank0{P, d_R.p, d_dlist.p, d_dstart.p, nflag, d_drank[0].p});
        L.lv[0] = d_drank[0].p;
        int64_t groups = 0;
        int k = 0;
        for (; k + 1 < kDenseMaxLevels; k++) {
            // (ranks of round 0 are < 5 nflag, of later rounds < n: the sort looks at the bits they can have)
            const uint64_t top_rank = k == 0 ? (uint64_t)nflag * 5 : (uint64_t)n;
            be.launch("dense_keys", n, DenseKeys{d_dstart.p, nflag, d_drank[k].p, (int64_t)1 << k, d_dkey.p, d_dval.p});
            be.sort_pairs(d_dkey.p, d_dkey2.p, d_dval.p, d_dval2.p, (size_t)n, 32 + bits_for(top_rank));
            be.launch("dense_heads", n + 1, DenseHeads{d_dkey2.p, n, d_dhead.p});
            be.exclusive_scan(d_dhead.p, d_dfirst.p, (size_t)n + 1);
            ensure(d_drank[k + 1], (size_t)n);
            be.launch("dense_rerank", n, DenseRerank{d_dval2.p, d_dhead.p, d_dfirst.p, d_drank[k + 1].p});
            L.lv[k + 1] = d_drank[k + 1].p;
            be.d2h(&groups, d_dfirst.p + n, 8);
            if (groups == n) break;
        }
        if (groups != n) { error = "suffix-array sort did not converge"; return -5; }
        dense_rounds = k + 1;
        L.top = k;      // round k + 1 ranks every suffix apart: the lifting starts below it
        be.launch("dense_lcp", n, DenseLcp{L, d_dval2.p, d_dstart.p, nflag, d_dlcp.p});
        be.launch("dense_rep", n, DenseRep{d_R.p, d_dlist.p, d_dval2.p, d_dstart.p, nflag, d_dlcp.p, d_rep.p});
        return 0;
    }
    bool dense_mode = false;            // this run of the batch takes the suffix-array path for the regions flagged in dense_h
    std::vector<uint8_t> dense_h;
    void collect_timing_more() { for (const PhaseTime& t : be.collect()) timing.push_back(t); }

    // small host-side all-gather (calcmumi's per-genome results): through device staging when the collectives are RCCL
    int allgather_host(const void* send, int64_t bytes, void* recv) {
        if (!coll.device) return coll.allgather(coll.ctx, send, bytes, recv);
        ensure(d_hsend, (size_t)bytes); ensure(d_hrecv, (size_t)bytes * (size_t)coll.world);
        be.h2d(d_hsend.p, send, (size_t)bytes);
        if (be.allgather_dev(d_hsend.p, bytes, d_hrecv.p)) return 1;
        be.d2h(recv, d_hrecv.p, (size_t)bytes * (size_t)coll.world);
        return 0;
    }

    // parity hook output (valid after run(..., want_events = true))
    std::vector<uint64_t> ev_key_h, ev_val_h;
    std::vector<int32_t> rep_h;
    int ev_lbits = 0;
    // tunables of a session (pm_session_tune): per-thread work budget of the index walks (a region whose walks exceed it takes the
    // suffix-array path); shortest one-region candidate list
    // that gets the device overlap test and stays resident as the anchor table (the host's threshold for its long-list routes)
    int64_t work_budget = 1 << 22;
    int64_t dirty_min = 4096;
    int64_t flagged_div = 8;      // store_settle: above one flagged row in flagged_div the tangled rows are counted before the list is taken (1: never declined)
    int64_t tangled_max = 1 << 17;   // ... and the list declined (PM_EAGAIN) with more tangled rows than this
    bool fast_tail = true;        // a call whose rows stay on the device does not wait for its candidate and accepted counts (run_once); false: it does (tests, before/after measurements)
    int64_t tail_repeats = 0;     // tails repeated the exact way (a capacity too small, an anchor list that turned out short)
    bool tangle_rounds = true;    // tangled rows settled in rounds (TangleOwner / TangleSettle) before the one wavefront that takes what is left; false: that wavefront takes them all (tests)
    bool group_small = true;      // the events of a recursion batch's small regions once per distinct piece (GroupedPairEvents)
    bool group_wide = false;      // ... and the small regions that form leaves (more pieces, more events, more genomes) by its wide form (GroupedPairEventsWide); off unless asked for: measured slower than pair by pair on every workload of DESIGN.md 8
    int64_t last_grouped = 0;
    int64_t last_grouped_wide = 0, last_handed_back = -1, last_wide_regions = 0;      // of last_grouped, the wide form's events; small regions neither form took (-1: not counted); regions the wide form took
    bool force_atomic_marks = false;      // (tests) store_settle marks with atomic ORs although the list is in order
    int filter_factor = 8;                // presence-filter bits per reference position, before rounding up to a power of two
    int slot_factor = 2;                  // index slots per reference position, before rounding up to a power of two (a measurement switch)
    bool bucket_sort = true;              // the events put in order by (pair, 256-position block) buckets (EventBucketCount ... CoarseFromBuckets); false: gathered and radix-sorted
    bool index_build = true;              // the index of a region with index_bucket_min slots or more built by buckets in LDS (index_kernels.h); false: IndexInsert for every region
    int64_t index_bucket_min = 1 << 24;   // ... slots of the smallest table built that way: the one shape it was measured faster at (a 5 Mb reference); a smaller table pays ~8 launches where IndexInsert's atomic rate is no problem
    bool index_verify = false;            // (tests) IndexVerify after the build: pm_last_timing "index_lost"
    int64_t index_overflow_cap = 0;       // (tests) capacity of the bucket build's overflow list (0: a 32nd of the bucketed positions + 1024)
    int64_t last_index_bucketed = 0, last_index_overflow = 0, last_index_lost = -1;      // positions built by buckets, their overflow records, IndexVerify's violations (-1: not run)
    bool master_seg = true;               // Master.EP from the genomes' segments (MasterEPSeg); false: every lane against every staged event (MasterEP)
    bool force_gate = false;              // (tests) the second stage of a two-stage store_validate never runs
    int64_t chain_window = 4096;          // passed MUMs in a row that a window of store_chain_begin walks (diag_diff in bases); more: kChainWindow, the caller's list logic
    int64_t chain_passed[2] = {-1, -1};   // MUMs in no LCB after the first / the second chaining pass of the last store_chain_end (-1: none yet)
    bool force_chain_tie = false;         // (tests) store_chain_begin reports two MUMs with one reference start
    bool force_unsure = false;            // (tests) store_validate's collinear test of the clusters reports failure: the exact test decides
    bool order_debug = false;             // the order check prints its counts (noted candidates, candidates left to the scan) to stderr
    int64_t outside_writes = 0;           // accepted reverse-strand members outside their region that OutsideWriteCheck looked at
    int64_t exact_cluster_tests = 0;      // generations validated with the exact test of their clusters (ClusterExtents ... ClusterDefer)
    int64_t deferred_regions = 0;         // regions a validation call left on the caller's work list (their cluster met an earlier one, or a child sorted first)
    bool clusters_out_of_order = false;   // a generation of this session failed the collinear test of its clusters: the exact test is asked at once from then on
    int64_t hint_shrink = 1;              // (tests) divides the capacities a call takes from the same call of the last step (CallHint, the seed regions' summaries)
    bool phase_timing = true;             // HIP events around the phases of a call (pm_last_timing); off: the marks cost nothing
    bool tune(const std::string& key, int64_t value) {
        if (key == "flagged_div" && value >= 1) { flagged_div = value; return true; }
        if (key == "tangled_max" && value >= 0) { tangled_max = value; return true; }
        if (key == "tangle_rounds") { tangle_rounds = value != 0; return true; }
        if (key == "fast_tail") { fast_tail = value != 0; return true; }
        if (key == "atomic_marks") { force_atomic_marks = value != 0; return true; }
        if (key == "master_seg") { master_seg = value != 0; return true; }
        if (key == "bucket_sort") { bucket_sort = value != 0; return true; }
        if (key == "index_build") { index_build = value != 0; return true; }
        if (key == "index_bucket_min" && value >= 1) { index_bucket_min = value; return true; }
        if (key == "index_verify") { index_verify = value != 0; return true; }
        if (key == "index_overflow_cap" && value >= 0) { index_overflow_cap = value; return true; }
        if (key == "filter_factor") { filter_factor = value < 1 ? 1 : (int)value; return true; }
        if (key == "slot_factor") { slot_factor = value < 1 ? 1 : (int)value; return true; }
        if (key == "stage_gate") { force_gate = value != 0; return true; }
        if (key == "chain_window" && value >= 1 && value <= kChainWindowMax) { chain_window = value; return true; }
        if (key == "chain_tie") { force_chain_tie = value != 0; return true; }
        if (key == "cluster_unsure") { force_unsure = value != 0; return true; }
        if (key == "order_debug") { order_debug = value != 0; return true; }
        if (key == "timing") { phase_timing = value != 0; be.timing_on = phase_timing; return true; }
        if (key == "group_small") { group_small = value != 0; return true; }
        if (key == "group_wide") { group_wide = value != 0; return true; }
        if (key == "work_budget" && value > 0) { work_budget = value; return true; }
        if (key == "dense_all") { dense_all = value != 0; return true; }
        if (key == "dirty_min" && value >= 0) { dirty_min = value; return true; }
        if (key == "hint_shrink" && value >= 1) { hint_shrink = value; return true; }
        if (key == "copy_kernel") { return tune_copy_kernel(be, value != 0, 0); }
        if (key == "boot_batch" && value >= 0) { boot_batch = value; return true; }
        if (key == "rec_batch" && value >= 0) { rec_batch = value; return true; }
        if (key == "ext_batch" && value >= 0) { ext_batch = value; return true; }
        return false;
    }

    void release() {
        if (chain_event) { be.event_wait(chain_event); be.event_release(chain_event); chain_event = nullptr; }
        for (BufBase* b : all_bufs) { if (b->raw) be.free(b->raw); b->raw = nullptr; b->cap = 0; }
        if (chain_host) be.pinned_free(chain_host);
        chain_host = nullptr; chain_host_cap = 0; chain_pending = false;
        if (blk) be.free(blk);
        if (d_goff) be.free(d_goff);
        if (d_glen) be.free(d_glen);
        blk = nullptr; d_goff = nullptr; d_glen = nullptr;
    }

    // device allocation failure inside run(): mapped to PM_ENOMEM at the C ABI (abi_glue.h), never abort()
    struct DeviceOutOfMemory { size_t bytes; };

private:
    B& be;
    // every device buffer of the engine registers itself here, so release() cannot miss one
    struct BufBase { void* raw = nullptr; size_t cap = 0; };
    std::vector<BufBase*> all_bufs;
    template <class T> struct Buf : BufBase {
        T* p = nullptr;
    };
    template <class T> void ensure(Buf<T>& b, size_t n) {
        if (n <= b.cap && b.p) return;
        if (std::find(all_bufs.begin(), all_bufs.end(), (BufBase*)&b) == all_bufs.end()) all_bufs.push_back(&b);
        if (b.raw) be.free(b.raw);
        b.raw = nullptr; b.p = nullptr; b.cap = 0;
        const size_t want = n + n / 4 + 16;
        b.raw = be.alloc(want * sizeof(T));
        if (!b.raw) throw DeviceOutOfMemory{want * sizeof(T)};
        b.p = (T*)b.raw; b.cap = want;
    }
    // the same, keeping the first `keep` elements (the stores grow while the run appends to them)
    template <class T> void ensure_keep(Buf<T>& b, size_t n, size_t keep) {
        if (n <= b.cap && b.p) return;
        if (std::find(all_bufs.begin(), all_bufs.end(), (BufBase*)&b) == all_bufs.end()) all_bufs.push_back(&b);
        const size_t want = n + n / 2 + 16;
        void* raw = be.alloc(want * sizeof(T));
        if (!raw) throw DeviceOutOfMemory{want * sizeof(T)};
        if (b.p && keep) { be.d2d(raw, b.p, keep * sizeof(T)); be.sync(); }
        if (b.raw) be.free(b.raw);
        b.raw = raw; b.p = (T*)raw; b.cap = want;
    }
    void collect_timing() { timing = be.collect(); }
    // Downloads in one launch (HipBackend::d2h_group): the downloads queued from here to the call's next wait may leave together;
    // flush_downloads() makes them leave now (where a phase of the call ends before the wait).  A backend without the grouping
    // (the emulation: a download is a memcpy) copies one by one.
    template <class T> static auto group_on(T& b, int) -> decltype(b.d2h_group(), void()) { b.d2h_group(); }
    template <class T> static void group_on(T&, long) {}
    template <class T> static auto flush_on(T& b, int) -> decltype(b.d2h_flush(), void()) { b.d2h_flush(); }
    template <class T> static void flush_on(T&, long) {}
    template <class T> static auto tune_copy_kernel(T& b, bool on, int) -> decltype(b.group_copies = on, true) { b.group_copies = on; return true; }
    template <class T> static bool tune_copy_kernel(T&, bool, long) { return true; }
    // keys ordered by the bits [lo, hi) (stable), where the backend has the operation (HipBackend::sort_keys: rocprim::radix_sort_keys)
    template <class T> static auto sort_keys_on(T& b, uint64_t* ki, uint64_t* ko, size_t n, int lo, int hi, int) -> decltype(b.sort_keys(ki, ko, n, lo, hi), true) { b.sort_keys(ki, ko, n, lo, hi); return true; }
    template <class T> static bool sort_keys_on(T&, uint64_t*, uint64_t*, size_t, int, int, long) { return false; }
    void group_downloads() { group_on(be, 0); }
    void flush_downloads() { flush_on(be, 0); }

    SeqBlock* blk = nullptr; int64_t* d_goff = nullptr; int64_t* d_glen = nullptr;
    Packed P{};
    size_t ev_cap_hint = 0, rest_cap_hint[2] = {0, 0}, grp_cap_hint = 0;
    std::vector<CallHint> call_hints;      // by call number of the step
    int64_t call_ordinal = 0;      // candidates / accepted rows of the last call of a shape ([1]: one region = an anchor call): capacities of the next one's tail
    Buf<uint8_t> d_gflag; Buf<int64_t> d_glo;
    Buf<int64_t> d_bkbase, d_bkbegin, d_ovf; Buf<uint64_t> d_ikey, d_ikey2, d_ikey3, d_ikey4;      // the bucket build of the index: first bucket per region, first record per bucket, overflow list, keys
    Buf<RegionInfo> d_R; Buf<int64_t> d_starts, d_lens, d_posbase;
    Buf<uint64_t> d_slots; Buf<uint32_t> d_filter, d_repeated; Buf<int32_t> d_next, d_rep, d_run, d_epm;
    Buf<int64_t> d_ucount, d_uoff; Buf<UnitRec> d_units;
    Buf<uint64_t> d_counter, d_evkey, d_evval, d_evkey2, d_evval2, d_evkey3, d_evval3; Buf<int64_t> d_sliceoff;
    Buf<int64_t> d_lo, d_cov; Buf<EventAtK> d_state; Buf<PairState> d_wsummary, d_wcarry; Buf<int32_t> d_emax;
    Buf<uint64_t> d_cand; Buf<GenomeAtK> d_at; Buf<uint8_t> d_ok; Buf<int32_t> d_ok_k, d_ok_lon, d_osp; Buf<uint8_t> d_ofwd;
    Buf<uint64_t> d_wmask; Buf<int64_t> d_wcount, d_woff;
    Buf<int64_t> d_bcount, d_bbegin, d_pbase;      // the event buckets: counts (behind a 0), where each begins (EventPlace's cursors), every pair's first
    Buf<int64_t> d_okcnt, d_okpos, d_cbase; Buf<int32_t> d_coarse; Buf<int32_t> d_creg, d_ck, d_clon, d_csp; Buf<uint8_t> d_cfwd;
    Buf<uint32_t> d_cflags, d_dirty; Buf<int32_t> d_bmax, d_bmin;
    Buf<GenomeAtK> d_xsend, d_xrecv; Buf<uint8_t> d_hsend, d_hrecv;
    Buf<RestItem> d_rest; Buf<uint64_t> d_qcount;
    // the suffix-array path (dense_kernels.h): flags per region, flagged index per region, the flagged regions and their dense
    // bases, sort keys / values (d_dval2: the suffix array), heads and ranks of a round, every round's ranks, LCP of SA neighbours
    Buf<uint8_t> d_dense; Buf<int32_t> d_dfi, d_dlist, d_dlcp; Buf<int64_t> d_dstart, d_dhead, d_dfirst;
    Buf<uint64_t> d_dkey, d_dkey2, d_dval, d_dval2; Buf<uint32_t> d_drank[kDenseMaxLevels];
    Buf<int32_t> d_anchor_start, d_anchor_lon; Buf<uint32_t> d_anchor_flags;      // the MUM store's rows as the searches delivered them
    int64_t table_counter = 0;
    Buf<uint64_t> d_image;
    Buf<int64_t> d_un_blk, d_un_cnt, d_un_scan, d_un_tot; Buf<int32_t> d_un_out;      // the unaligned runs: block geometry, counts per block, their scans, totals per genome, the runs
    Buf<double> d_nj_D, d_nj_R, d_nj_q; Buf<uint8_t> d_nj_active; Buf<int32_t> d_nj_j, d_nj_dist; Buf<NjJoinRec> d_nj_joins; Buf<NjLastRec> d_nj_last;      // a neighbour-joining tree (nj_kernels.h)
    // the bootstrap (boot_kernels.h): draw counters, weights as bytes and planes, replicate distances; the trees of a batch; splits and support
    Buf<uint32_t> d_boot_cnt, d_bs_support; Buf<uint8_t> d_boot_w8, d_bt_active; Buf<uint64_t> d_boot_planes, d_bs_msets, d_bs_mkeys, d_bs_rsets, d_bs_rkeys;
    Buf<int32_t> d_boot_dist, d_bt_dist, d_bt_j; Buf<double> d_bt_D, d_bt_R, d_bt_q; Buf<NjJoinRec> d_bt_joins, d_bs_mj, d_bs_rj; Buf<NjLastRec> d_bt_last;
    // the recombination scan (rec_kernels.h): transposed planes, informative flags; sites, window and matrix offsets, window numbers; matrices, phi, le
    Buf<uint64_t> d_rec_tp; Buf<uint8_t> d_rec_flag, d_rec_inc; Buf<int64_t> d_rec_sites, d_rec_woff, d_rec_moff, d_rec_wid; Buf<int32_t> d_rec_phi; Buf<uint32_t> d_rec_le;
    // the LCB extension (ext_kernels.h): descriptors, the job of every pair, row offsets; pass bits, reaches, line maxima; paths, column starts, widths, j_r, rows
    Buf<ExtRow> d_ext_rows; Buf<int32_t> d_ext_job, d_ext_reach, d_ext_best, d_ext_cs, d_ext_cols, d_ext_used; Buf<int64_t> d_ext_off; Buf<uint64_t> d_ext_bits; Buf<uint16_t> d_ext_pk; Buf<uint8_t> d_ext_out;
    Buf<uint64_t> d_snp_counts, d_snp_lo, d_snp_hi; Buf<uint8_t> d_snp_chunk; Buf<int64_t> d_snp_flag, d_snp_rank, d_snp_col; Buf<int32_t> d_snp_dist;      // the SNP collection (snp_kernels.h)
    Buf<uint8_t> d_ms_strand, d_ms_state, d_small8, d_o_strand; Buf<int32_t> d_ms_shift, d_ms_len, d_list, d_list2, d_j_min, d_j_max, d_o_start;
    Buf<int64_t> d_rg_start, d_rg_len, d_lay_off, d_lay_bits, d_v_row0, d_v_first, d_f_start, d_f_end, d_f_pack; Buf<RegInfo> d_rg_info; Buf<uint64_t> d_rg_count, d_once, d_twice;
    Buf<RowInfo> d_rowinfo; Buf<uint64_t> d_alg;
    Buf<int64_t> d_sd_cnt, d_sd_off; Buf<uint8_t> d_sd_keep;      // store_settle_seeds
    Buf<uint64_t> d_t_rem; Buf<uint8_t> d_t_done;      // settle_launch: tangled rows left, settled flags per flagged row
    Buf<int32_t> d_v_done, d_owner; Buf<uint8_t> d_v_defer, d_v_involved;      // store_validate: regions processed per cluster; the exact test of the clusters
    Buf<uint64_t> d_t_left; uint64_t tangle_left[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int tangle_ran = 0;      // settle_launch: what each round of the tangled rows left, last step
    Buf<int64_t> d_rg_pkey; Buf<OutsideWrite> d_outw; Buf<uint64_t> d_outw_count; int64_t rg_pkey_init = 0; uint64_t outside_writes_call = 0;      // store_validate: OutsideWriteCheck
    Buf<ForeignRead> d_foreign; Buf<uint64_t> d_foreign_count, d_foreign_masks; Buf<int64_t> d_ms_key;       // store_validate / store_order_check: candidates with a member outside their region
    size_t foreign_cap = 0; int64_t ms_key_rows = 0; uint64_t foreign_seen = 0;      // foreign_seen: the device's counter as of the last validation call
    static constexpr size_t kHitCap = 256;      // noted candidates that the bounds of ForeignBound do not decide
    Buf<uint64_t> d_hit_count, d_hit_owned, d_hit_present; Buf<int32_t> d_hits; Buf<uint8_t> d_recwords;      // d_recwords: one byte per image word, set where the recursion has marked
    // store_chain_begin / _end
    Buf<int64_t> d_ch_flag, d_ch_pos, d_ch_head, d_ch_hpos, d_ch_survive, d_ch_spos, d_ch_hdr;
    Buf<uint64_t> d_ch_key, d_ch_val, d_ch_skey, d_ch_srow, d_ch_key2, d_ch_row2, d_ch_lcblen;
    Buf<uint8_t> d_ch_verdict, d_ch_outhead; Buf<int32_t> d_ch_outrow;
    Buf<int64_t> d_ch_back, d_ch_wflag, d_ch_wpos, d_ch_wlist, d_ch_wend; Buf<uint8_t> d_ch_wverdict, d_ch_wkeep;      // diag_diff in bases: the windows
    uint8_t* chain_host = nullptr; size_t chain_host_cap = 0; void* chain_event = nullptr; bool chain_pending = false; int64_t chain_cap = 0;
    size_t lay_words = 0, rg_cap_hint = 0;
    int64_t layout_rows = -1;       // >= 0: the image holds the layout of the current anchor table (store_settle ran)
};

}  // namespace pm
