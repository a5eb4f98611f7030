/* include/parsnp_mum.h -- C ABI of the MI355X multi-MUM engine (libparsnp_hip.so).
 *
 * This is the drop-in boundary for the one hot path of marbl/parsnp that this project replaces: the
 * csgmum calls made by Aligner::setMums1.  The reference has no FFI for it (csgmum is #included C,
 * src/parsnp.cpp:73-78); the entry points below are what a binding for that path would bind, one per
 * reference call site.  Plain pointers and sizes only; every function returns 0 on success or a negative
 * PM_E* code (no exceptions cross the boundary).  pm_last_error() gives a message for the calling thread.
 *
 * Sequences are ASCII over {A,C,G,T,N}, exactly the strings parsnp_core holds after ingest
 * (src/parsnp.cpp:2999-3141): any other byte is treated as N.  'N' matches 'N' (src/csgmum/csg.c:13-25).
 * Coordinates are 0-based; all arithmetic is integer (int32 reference positions, int64 query positions).
 */
#ifndef PARSNP_MUM_H
#define PARSNP_MUM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_OK 0
#define PM_ENODEV (-1)   /* no usable gfx950 device / HIP runtime error at start-up */
#define PM_EINVAL (-2)   /* bad argument */
#define PM_ENOMEM (-3)   /* host or device allocation failed */
#define PM_EHIP (-4)     /* a HIP call or kernel failed */
#define PM_ELIMIT (-5)   /* a hard size limit of the engine was exceeded: a region of 2^31 bases or more, a batch too large for
                            64-bit event keys or 2^31 work units (repeat structure is no such limit: see "work_budget") */
#define PM_EAGAIN (-6)   /* the resident route (pm_store_*) does not apply to this input: the caller takes the host route */

typedef struct pm_session pm_session; /* genomes resident in HBM (2-bit + N-mask, both strands) */
typedef struct pm_result pm_result;   /* output of one batch call, owned by the library until pm_result_free */

const char* pm_last_error(void);
/* "hip" for libparsnp_hip.so. (The test-only CPU provider under oracle/ answers "oracle".) */
const char* pm_provider(void);

/* Optional: start the HIP runtime of this process (device discovery, context, code objects -- ~0.15 s when nothing else has
 * touched the GPU yet).  Thread-safe; meant to be called from a side thread while the caller is still reading its input,
 * as parsnp_core does during FASTA ingest.  device < 0: PARSNP_DEVICE or the current device. */
int pm_warmup(int device);

/* Upload the n genomes once (genome 0 = reference).  Replaces the per-call substr()+reversec()+strcpy of
 * src/parsnp.cpp:1540-1561: regions are addressed by (start,len) into these resident copies.
 * device < 0 selects the current HIP device. */
int pm_session_create(pm_session** out, int device, int n_genomes, const uint8_t* const* seqs, const int64_t* lens);
/* Sharded run over the GPUs of one node: rank r of `world` SEARCHES a contiguous block of the query genomes
 * (block r of world equal blocks of genomes 1..n-1, in ini order) against the reference; every rank keeps all genomes
 * resident (one byte per base and strand -- memory is not what a 288 GB GPU runs out of -- so that the validation of the
 * resident route can check any member of a MUM against its sequence).  Every rank makes the same sequence of calls with the
 * same arguments and receives the same results.  Per batch the engine exchanges
 *   (1) Master.EP, reduced with min over the ranks           (allreduce_min, one int32 per reference position), and
 *   (2) the per-genome (EP,UP,SP) columns at the candidates  (allgather of equal-size blocks),
 * through the two callbacks (host buffers; 0 = success), which the embedding process implements with
 * torch.distributed -- RCCL over xGMI on the GPUs, gloo in the CPU tests.  The strand/UP fold then runs over all
 * genomes in ini order on every rank, so results are bit-identical to the unsharded run. */
typedef int (*pm_allreduce_min_i32_fn)(void* ctx, int32_t* buf, int64_t count);
typedef int (*pm_allgather_fn)(void* ctx, const void* send, int64_t send_bytes, void* recv /* world * send_bytes */);
int pm_session_create_sharded(pm_session** out, int device, int n_genomes, const uint8_t* const* seqs, const int64_t* lens,
                              int rank, int world, pm_allreduce_min_i32_fn allreduce_min, pm_allgather_fn allgather, void* ctx);
/* The same sharded run with the two exchanges ON THE DEVICE: the library owns an RCCL communicator (one rank per process
 * and GPU, xGMI inside a node) and runs all-reduce(min) on Master.EP in place and the all-gather of the candidate columns
 * on its own stream, between its kernels -- no host staging, no callback.  Rank 0 obtains an id with pm_rccl_unique_id
 * and hands its 128 bytes to the other ranks by whatever channel launched them (a file, MPI, torch.distributed's store);
 * every rank then calls pm_session_create_rccl with its rank.  RCCL is loaded on demand from PARSNP_RCCL_LIB or
 * /opt/rocm/lib/librccl.so.1; a one-rank communicator (world = 1) is legal and runs the same exchange code. */
#define PM_RCCL_ID_BYTES 128
int pm_rccl_unique_id(uint8_t* id /* PM_RCCL_ID_BYTES */);
int pm_session_create_rccl(pm_session** out, int device, int n_genomes, const uint8_t* const* seqs, const int64_t* lens,
                           int rank, int world, const uint8_t* id /* PM_RCCL_ID_BYTES */);
/* number of ranks of the session's RCCL communicator as RCCL reports it (ncclCommCount); 0 for a session without one */
int pm_session_rccl_ranks(const pm_session* s);
void pm_session_destroy(pm_session* s);
int pm_session_genomes(const pm_session* s);

/* Multi-MUM candidates for a batch of regions.  For region r (r = 0..n_regions-1) and genome g:
 *   starts[r*n_genomes+g], lens[r*n_genomes+g] : the substring of genome g   (TRegion start/length, src/LCR.cpp:12-37;
 *                                                 the reference chunk of src/parsnp.cpp:1519-1547 when g == 0)
 *   minsize[r]                                 : minimum MUM length          (src/parsnp.cpp:1502-1514)
 * Per region this is the whole of src/parsnp.cpp:1563-1695:
 *   new_CSG/build_CSG/find_leaves (csg.c:105-575)  -> device index of the reference substring
 *   Find_UM x 2 per query (mum.c:177-250)          -> R-unique maximal matches, both strands
 *   Intersect_UM x 2 (mum.c:125-175)               -> forward carry + fold into Master
 *   Merge_Master (mum.c:92-123)                    -> strand choice in ini order, ties to reverse
 *   extraction loop (parsnp.cpp:1633-1695)         -> candidates (k, LON, per-genome SP and strand)
 * The candidate list is bit-identical to the reference's list_mums for the same region. */
int pm_multi_mum_batch(pm_session* s, int64_t n_regions, const int64_t* starts, const int64_t* lens,
                       const int32_t* minsize, pm_result** out);

/* Result accessors.  Candidates of region r are c in [off[r], off[r+1]).  For candidate c:
 *   k[c]   reference offset inside the region (Mum.DSP[0]-1-ini_region, parsnp.cpp:1671)
 *   lon[c] length (Mum.LON, :1687)
 *   sp[c*(n_genomes-1)+g-1]  start inside genome g's substring, on the chosen strand's string (SPF[g-1].MSP[k], :1681; region lengths are < 2^31, so int32)
 *   fwd[c*(n_genomes-1)+g-1] 1 = forward, 0 = reverse complement (SPF[g-1].forward[k], :1678)            */
int64_t pm_result_regions(const pm_result* r);
int64_t pm_result_total(const pm_result* r);
const int64_t* pm_result_offsets(const pm_result* r);
const int32_t* pm_result_k(const pm_result* r);
const int32_t* pm_result_lon(const pm_result* r);
const int32_t* pm_result_sp(const pm_result* r);
const uint8_t* pm_result_fwd(const pm_result* r);
void pm_result_free(pm_result* r);

/* MUM-row mode.  After pm_session_rows(s, 1) the results of pm_multi_mum_batch carry, instead of sp / fwd (those accessors
 * then return NULL), what the second half of setMums1 derives from them per candidate (src/parsnp.cpp:1717-1780 and the
 * TMum constructor src/TMum.cpp:25-60), built on the device; n = n_genomes, genome 0 = the reference:
 *   start[c*n+j]   start of the MUM in genome j on the genome's forward coordinates: window start + sp for a forward
 *                  member, genome length - (window start + sp + lon) for a reverse one (flipped against the WHOLE genome)
 *   strand[c*n+j]  1 forward, 0 reverse (genome 0: always 1)
 *   flags[c]       PM_ROW_BAD      a start position outside its window: the reference skips the candidate (:1723)
 *                  PM_ROW_OUTSIDE  start < 0 or start + lon > genome length in some genome (`notgood`)
 *                  PM_ROW_REVERSE  some member is on the reverse strand
 *                  PM_ROW_DIRTY    (only when pm_result_dirty_known) overlaps an earlier candidate of the list in some
 *                                  genome by the running-extent test of the anchor validation; computed for one-region
 *                                  batches with at least "dirty_min" (4096) accepted candidates
 *                  PM_ROW_EARLY    (with PM_ROW_DIRTY's condition) starts, in some genome, before the end of an earlier
 *                                  candidate of the list: candidates WITHOUT it lie in list order in every genome
 * The window of genome j is the starts/lens row the caller passed, so the rows equal the reference's only for requests
 * whose rows ARE the region (one unclamped reference chunk); a caller with clamped or chunked rows keeps to sp / fwd.
 * The blocks are writable: the caller may trim the rows in place (Aligner::trim) and keep them as its MUM table. */
#define PM_ROW_BAD 1u
#define PM_ROW_OUTSIDE 2u
#define PM_ROW_REVERSE 4u
#define PM_ROW_DIRTY 8u
#define PM_ROW_EARLY 16u
int pm_session_rows(pm_session* s, int enable);
int32_t* pm_result_start(pm_result* r);
uint8_t* pm_result_strand(pm_result* r);
const uint32_t* pm_result_flags(const pm_result* r);
int pm_result_dirty_known(const pm_result* r);

/* The rows of a long ONE-region result in row mode (the anchor call: at least "dirty_min" candidates) stay on the device as the
 * session's ANCHOR TABLE; pm_result_table_id() names it (0: this result left no table).  The resident route below works on it. */
int64_t pm_result_table_id(const pm_result* r);
/* Tunables of a session (tests lower the thresholds of the long-list routes so that small inputs take them):
 *   "work_budget"  per-thread step budget of the index walks (default 2^22): the threshold at which a region switches to the
 *                  suffix-array path.  A batch in which a walk exhausts it is run again, and the regions whose walks ran out
 *                  (tandem repeats of period > 1 with thousands of copies) get rep' and their events from a suffix array of the
 *                  region instead (cost independent of the copy number); every other region walks as before.  Not an error
 *   "dense_all"    != 0: every region of every batch takes the suffix-array path from the start (tests compare it with the walks;
 *                  default 0; the same result)
 *   "dirty_min"    shortest one-region candidate list that gets the overlap / order flags and stays on the device as the
 *                  anchor table (default 4096)
 *   "flagged_div"  pm_store_settle takes an anchor table of which at most one row in flagged_div is flagged (overlaps an earlier
 *                  one by the cheap running-extent test: default 8) as it is; above that it counts the TANGLED rows first (flagged rows
 *                  that overlap one another: settled in list order where they meet, in rounds) and answers PM_EAGAIN with more than
 *                  "tangled_max" of them (default 131072).  1: never PM_EAGAIN (tests)
 *   "tangle_rounds" 0: the tangled rows are settled by ONE wavefront in list order instead of in rounds (default 1; the same result)
 *   "fast_tail"    0: a search whose rows stay on the device waits for its unit, candidate and accepted counts before it sizes the
 *                  launches that need them, as every other search does (default 1: capacities from the last call of the shape, the
 *                  kernels read the live counts, the counts come back with the results; the same result)
 *   "hint_shrink"  N > 1: the capacities a "fast_tail" call takes from the same call of the last step (units, candidates, the seed
 *                  regions' summaries) are divided by N (tests: the capacities are too small, the call repeats the part that
 *                  needed them -- "tail_repeats" of pm_last_timing counts it -- and the result is the same; default 1)
 *   "copy_kernel"  0: every download a call queues in front of a wait is a copy command of its own (rounds 1-6), instead of all of
 *                  them leaving in one kernel launch that stores into page-locked host memory (default 1; the same bytes arrive)
 *   "atomic_marks" != 0: pm_store_settle marks the layout with atomic ORs even where the list's order allows plain stores (tests)
 *   "group_small"  0: the events of a recursion batch's small regions are found pair by pair and sorted with the others, instead of
 *                  once per distinct query piece (default 1; both give the same events, tests compare the two)
 *   "group_wide"   != 0: the small regions that form does not take -- more than 32 distinct pieces, more than 8 events of one (piece,
 *                  strand), a batch of more than 1 024 query genomes -- are taken by its wide form up to the limits of
 *                  pm_group_limits(1), instead of pair by pair (default 0: as measured the wide form costs more than it saves,
 *                  DESIGN.md 8; never on while "group_small" is 0; the same events either way, tests compare the two)
 *   "slot_factor"  index slots per reference position before rounding up to a power of two (default 2: load <= 1/2; 1 = rounds 1-5,
 *                  load <= 2/3 -- the wavefronts of IndexInsert and of the probes run as long as their longest probe sequence);
 *   "filter_factor" presence-filter bits per reference position before rounding up (default 8; 4 ... 32 measured: flat)
 *   "bucket_sort"  0: the events of a search are gathered and radix-sorted by (pair, l, strand) and the readers' table of events per
 *                  256-position block comes from a pass over the sorted keys (rounds 1-5), instead of a counting sort by (pair, block)
 *                  buckets whose scanned counts ARE that table (default 1; the same events in the same order up to equal keys)
 *   "master_seg"   0: Master.EP by the round-4 kernel (every lane tests every staged event: MasterEP) instead of from the genomes'
 *                  segments (MasterEPSeg; default 1; the same values, tests compare the two)
 *   "stage_gate"   != 0: the second stage of a two-stage pm_store_validate is never run (tests: the caller forms it again)
 *   "cluster_unsure" != 0: pm_store_validate's collinear test of the clusters reports failure although they are in order (tests:
 *                  the exact test -- extents ORed into a scratch image -- must find them disjoint and the same bytes result)
 *   "order_debug"  != 0: the order check (pm_store_order_check / pm_store_chain_begin) waits for its kernels and prints to stderr
 *                  how many candidates it had noted and how many its bounds left to the scan
 *   "chain_window" 1 .. 65 536 (4 096): the passed MUMs in a row that pm_store_chain_begin follows with diag_diff > 1; a longer
 *                  run is reported in bit 3 of pm_chain_info.trouble (tests set it low)
 *   "chain_tie"    != 0: pm_store_chain_begin reports two MUMs with one reference start although there is none (tests: the
 *                  caller's own list logic must give the same bytes)
 *   "timing"       0: no HIP events around the phases of a call (pm_last_timing then reports counts only)
 *   "index_build"  0: the reference index of every region is built by IndexInsert (compare-and-swap in global memory) as before; default 1: a
 *                  region with "index_bucket_min" slots or more is built by buckets in LDS (index_kernels.h: keys sorted by bucket, a
 *                  wavefront per bucket, the table and the filter written once); the same multi-MUMs either way, tests compare the two
 *   "index_bucket_min" slots of the smallest table that "index_build" = 1 builds by buckets (default 2^24: a region of more than 4 194 304
 *                  bases at the default "slot_factor", the shape the build was measured at; tests and measurements lower it); a smaller region, or one whose filter piece per bucket would be under 32 bits
 *                  or over 16 384, is built by IndexInsert in the same launch as before
 *   "index_verify" != 0: after the index build a kernel looks every reference position up again (its K-mer's slot found, the
 *                  position on that slot's chain, the filter word passing, next = -1 outside chains) and pm_last_timing reports the
 *                  violations as "index_lost" (tests; default 0)
 *   "index_overflow_cap" capacity of the bucket build's overflow list in records (0, the default: a 32nd of the bucketed
 *                  positions + 1 024); a list that is full makes the call build every region with IndexInsert (tests set it to 1)
 * PM_EINVAL for an unknown key or a value out of range.
 * PARSNP_TUNE="key=value,key=value" in the environment applies these to every session from its start, the sessions that
 * pm_find_events opens for itself included; an unknown key or a refused value fails the session's creation with PM_EINVAL. */
int pm_session_tune(pm_session* s, const char* key, int64_t value);

/* ---------------------------------------------------------------------------------------------------------------------------
 * The RESIDENT route.  What Aligner does with a candidate list after csgmum produced it -- validation and trimming (second half
 * of setMums1, src/parsnp.cpp:1713-1841; Aligner::trim :1399-1477), the neighbour regions (determineRegion :1199-1290), the
 * generations of the work list (doWork :173-317), the pairwise test of the LCB chaining (setFinalClusters :2596-2700) and the
 * inter-LCB fillers (setInterClusterRegions :2389-2460) -- on rows that never leave the device.  One entry point per reference
 * function; the order-dependent list logic (work-list order, ties, the chain walk) stays with the caller, which receives a few
 * bytes per MUM instead of its rows.
 *
 * pm_session_rows(s, 2) switches the session to resident mode: the rows of a long one-region result (the anchor call: the
 * condition of the anchor table, above) stay on the device as rows [0, A) of the session's MUM STORE -- pm_result_start /
 * _strand of such a result are NULL, pm_result_store_base() is 0 -- and every pm_store_search appends its candidates.  A store
 * row has, besides the row the search delivered (never rewritten), `shift` (bases trimmed on the left: TMum::trimleft moves the
 * start in EVERY genome), `len` (current length) and a state.  The layout (mumlayout, :3181-3186) is an image in device memory.
 * The REGION STORE holds the request rows of seed and child regions.  A later anchor call of the session starts all three over.
 * Every function returns PM_OK, PM_EAGAIN (the caller falls back to the host route: pm_store_rows(raw) gives it the rows it
 * did not receive) or an error; a session is single-threaded. */
#define PM_ST_BUILT 1u      /* the reference constructs a TMum for the candidate (no PM_ROW_BAD) */
#define PM_ST_OK 2u         /* inside every genome (no PM_ROW_OUTSIDE) */
#define PM_ST_FLAGGED 4u    /* (anchor list) overlapped an earlier row: settled against the marks of the others */
#define PM_ST_TANGLED 8u    /* ... and another flagged row: settled in list order */
#define PM_ST_ACCEPTED 16u  /* a MUM of the run: marked in the layout */
typedef struct { int32_t start0, len, shift; uint32_t state_flags; } pm_row_info;   /* start on the reference (trim applied), length, left trim, state | PM_ROW_* << 8 */
typedef struct { int64_t key, ref_start, ref_len; int32_t slength, parent; } pm_region_info;   /* push order, reference column, shortest length, store row of the MUM it lies next to */
int64_t pm_result_store_base(const pm_result* r);      /* first store row of a result whose rows stayed resident, else -1 */
/* setMums1, second half, for the anchor table `table_id` into an EMPTY layout (:1781-1841): rows that overlap nothing earlier
 * are settled and marked at once; the flagged ones (PM_ROW_DIRTY) are trimmed against those marks (Aligner::trim) -- side by
 * side where they meet no other flagged row, in list order where they do (rounds: a tangled row is settled once the tangled
 * rows before it that share a 64-base word with it are).  rows[c] for every row of the table.  PM_EAGAIN only above
 * "tangled_max" tangled rows (the exact overlap test and the threads of the host route decide); rearranged sets are taken. */
int pm_store_settle(pm_session* s, int64_t table_id, pm_row_info* rows);
int pm_store_info(pm_session* s, int64_t first, int64_t count, pm_row_info* out);
/* setInitialClusters' seed regions (:2150-2172): determineRegion on both sides of every accepted anchor (anchors[]: their store
 * rows in list order), kept when longer than q in every genome.  The kept regions are regions [0, *n_regions) of the region
 * store; pm_store_new_regions / _ids list them in the reference's push order. */
int pm_store_seeds(pm_session* s, int64_t table_id, const int32_t* anchors, int64_t n_anchors, int32_t q, int64_t* n_regions);
/* pm_store_settle and pm_store_seeds in one call, without the round trip between them: the accepted anchors are listed on the
 * device and the kept regions arrive in the reference's push order (pm_store_new_regions / _ids).  PM_EAGAIN as pm_store_settle. */
int pm_store_settle_seeds(pm_session* s, int64_t table_id, int32_t q, pm_row_info* rows, int64_t* n_regions);
const pm_region_info* pm_store_new_regions(const pm_session* s);   /* of the last pm_store_seeds / pm_store_validate, valid until the next */
const int32_t* pm_store_new_region_ids(const pm_session* s);
int pm_store_regions_equal(pm_session* s, const int32_t* a, const int32_t* b, int64_t n, uint8_t* same);   /* TRegion operator== (LCR.cpp:48-58) */
/* pm_multi_mum_batch on the rows of the listed regions; the candidates of region i become store rows
 * [*first_row + offsets[i], *first_row + offsets[i + 1]) (offsets[n + 1]). */
int pm_store_search(pm_session* s, const int32_t* regions, const int32_t* minsize, int64_t n, int64_t* first_row, int64_t* offsets);
/* The same with host work of the caller's that does not depend on the search: beside(ctx) is called exactly once, on the calling
 * thread -- when the event search is queued and before the call first waits for the device, or on the way out of a call that never
 * gets there (no region, an error).  It must not call the engine. */
int pm_store_search_beside(pm_session* s, const int32_t* regions, const int32_t* minsize, int64_t n, int64_t* first_row, int64_t* offsets,
                           void (*beside)(void*), void* ctx);
/* One generation of doWork (:173-317).  The caller lists the waiting regions in the reference's order (reference start), with the
 * store rows of their candidates, cut into clusters (cluster c = regions [cluster_first[c], cluster_first[c + 1])) that it has
 * formed on the reference (maximal runs that overlap or touch there); the clusters are validated side by side, each in order: candidates settled against
 * the layout and marked (setMums1 second half), the neighbour regions of every new MUM longer than q appended to the region
 * store (:215-254; pm_store_new_regions lists them parent by parent, in push order; one equal to a region still waiting in its
 * cluster is dropped as the work list would, :294-306).  The caller clusters on the reference only; what the other genomes do
 * to the clusters is the call's business, and its answer is done[c] (n_clusters values): how many regions of cluster c were
 * processed.  All of them where the cluster meets no EARLIER cluster in any genome (clusters in reference order follow each
 * other with a base between in every genome -- or, where a genome holds them in another order, their extents are tested
 * exactly, and so is what their CANDIDATES touch: a member outside its region reads where another cluster may mark); NONE where it does: the reference (doWork pops the smallest reference start, and children lie inside their parents)
 * finishes the earlier cluster and everything it leads to first, so the cluster must wait -- the caller keeps its regions on
 * the work list for the next generation, where the question is put again; the FIRST FEW where a child of a processed region
 * sorts before (or ties with) the next waiting region of the cluster: the rest waits as well, the next generation sorts it
 * with the children (:291-292).  Every call processes at least the first region of its first cluster.  done == NULL: a caller
 * that cannot keep regions waiting -- either case is then reported as trouble (bits 3 / 0) instead.
 * *trouble != 0: the reference's order would show and the caller must discard the run and take the host route -- bit 1 (2): a
 * reverse-strand member outside its region (TMum.cpp:33-35 flips it against the whole genome) was accepted where a region on the
 * wrong side of the order covers its marks (one walked out or processed by a MUM the reference takes LATER, or one that still
 * waits and sorts EARLIER; an accepted member whose marks fall on ground no such region covers is harmless and stays); bit 2 (4): a
 * region with 2^22 candidates or more, or more candidates with a member outside their region (or one longer than 64 bases) than
 * the engine notes for pm_store_order_check; bits 0 (1) and 3 (8): only with done == NULL, see above.
 * info_count > 0: the per-row scalars (pm_store_info) of store rows [info_first, info_first + info_count) -- the candidates
 * just decided -- come back with the same round trip.
 * stage_first > 0: TWO generations in one call.  Clusters [0, stage_first) are validated first (the first pushed seed, which the
 * reference processes before its work list is ever sorted, :194-195 before :291-292); clusters [stage_first, n_clusters) -- the
 * generation the caller formed on the assumption that the first stage pushes no child region -- are validated behind them if
 * that held (*second_stage_ran = 1) and are left untouched if not (0: the caller forms the generation again, with the children;
 * their done[] is 0).
 * generation: the number of the (first) generation of the call, 0 = the first pushed seed alone; with the regions' reference
 * starts it orders the regions as the reference's work list does (pm_store_order_check). */
int pm_store_validate(pm_session* s, const int32_t* regions, const int64_t* row_first, const int32_t* row_count, int64_t n_regions,
                      const int64_t* cluster_first, int64_t n_clusters, int32_t q, uint32_t* trouble, int64_t* n_children,
                      int64_t info_first, int64_t info_count, pm_row_info* info, int64_t stage_first, int32_t* second_stage_ran, int32_t generation, int32_t* done);
/* After the LAST generation.  A candidate with a reverse-strand member outside its region reads layout marks in another
 * cluster's territory, and what is marked there when the reference looks depends on its order (doWork :173-317: the first pushed
 * seed, then always the waiting region with the smallest reference start).  pm_store_validate notes every such candidate with
 * the marks it saw; this call decides each of them again with the marks the reference's order had in place -- the anchors' and
 * those of the recursion's MUMs whose region comes earlier in that order -- and reports *trouble != 0 when a verdict, a shift or
 * a length differs from what the generations stored: the caller must discard the run and take the host route.
 * pm_store_chain_begin runs the same check ahead of phases C-D (bit 2 of pm_chain_info.trouble): a caller that queues them
 * does not call this. */
int pm_store_order_check(pm_session* s, uint32_t* trouble);
/* The test of setFinalClusters (:2596-2700) of MUM cur[i] against the open chain's last MUM back[i]: verdict[i] = 0 every
 * genome's gap lies in [0, d] (min_gap / max_gap: what the ratio test :2693 reads), 1 the chain closes, 2 a reverse-strand
 * member (the strand rules of :2604-2625 depend on the genome order): the caller judges the pair from its rows. */
int pm_store_judge(pm_session* s, const int32_t* cur, const int32_t* back, int64_t n, int32_t d, int32_t* min_gap, int32_t* max_gap, uint8_t* verdict);
int pm_store_unmark(pm_session* s, const int32_t* rows, int64_t n);      /* the MUMs leave the layout (:415-418, :460-466) */
/* setInterClusterRegions (:2389-2460) for consecutive LCBs (last MUM of one, first MUM of the next): add[i] = 1 a filler is made
 * -- its rows, [n_genomes] each, follow one another in pm_store_fill_starts / _ends --, 0 none, 2 the reference's bookkeeping
 * would overrun (:2419-2433). */
int pm_store_fill(pm_session* s, const int32_t* last_of, const int32_t* first_of_next, int64_t n, uint8_t* add);
const int64_t* pm_store_fill_starts(const pm_session* s);
const int64_t* pm_store_fill_ends(const pm_session* s);
/* Phases C-D in one queue of launches, for a run whose list logic is order-free -- all reference starts of the accepted MUMs
 * differ, no MUM short enough for filterRandom1 (:338-425): the sort by reference start (:338, :2571), the chain walk of
 * setFinalClusters (:2563-2719; the pairwise test of pm_store_judge, pairs with reverse-strand members included, with the test
 * of :2684-2700 applied on the device in the reference's float / double mix), the dissolving of LCBs no longer than c by
 * filterRandomClustersSimple1 (:433-497; the last LCB is never examined, :447; their MUMs leave the layout), the second
 * chaining pass (:3261-3268) and the fillers of setInterClusterRegions (:2389-2460; counted: a filler is never printed, it
 * shifts the numbers of the LCBs behind it).  diag_diff <= 1 is a ratio (a MUM joins the open chain or closes it, :2693);
 * diag_diff > 1 is a difference in bases (:2684-2692): a MUM whose gaps differ by that much or more is PASSED -- neither joined
 * nor closing; the next MUM is judged against the chain's last joined MUM -- stays in the list in no LCB, and is judged again
 * in the second pass.  _begin queues the work and returns; _end waits for it: n_mums store rows in reference order (rows), a
 * byte per MUM (heads: 0 a member of the LCB open at it, 1 it begins an LCB, 2 it is in no LCB; 2 only with diag_diff > 1) --
 * both valid until the session's next chain call -- and the counters of the log.  trouble != 0: bit 0 two MUMs share a
 * reference start (the reference's unstable sort decides: nothing on the device has changed, the caller runs pm_store_judge /
 * _unmark / _fill with its own list logic); bit 1 the reference's filler bookkeeping would overrun (:2419-2433, pm_store_fill's
 * add = 2); bit 2 the order check (pm_store_order_check) failed: nothing has changed, the caller discards the run and takes
 * the host route; bit 3 (diag_diff > 1) more passed MUMs in a row than "chain_window" (pm_session_tune), or more than 65 536
 * places where a run of them may begin: nothing has changed, the caller runs its own list logic as for bit 0.
 * n_expected: the number of accepted store rows (the caller's MUM list); a mismatch is an error.
 * pm_store_chain_passed: the number of MUMs in no LCB after the first and after the second chaining pass of the last
 * pm_store_chain_end (PM_EINVAL before the first one). */
typedef struct { int64_t n_in, lcbs_first, lcbs_dissolved, mums_dissolved, n_mums, n_lcbs, n_fillers; uint64_t trouble; } pm_chain_info;
int pm_store_chain_begin(pm_session* s, int64_t n_expected, int32_t d, float diag_diff, int64_t c);
int pm_store_chain_end(pm_session* s, pm_chain_info* info, const int32_t** rows, const uint8_t** heads);
int pm_store_chain_passed(const pm_session* s, int64_t* first_pass, int64_t* second_pass);
/* Rows for the host (the XMFA writer after the LCBs are final; a caller falling back to the host route): start[i * n_genomes + j]
 * with the trim applied (raw != 0: as the search delivered it), strand byte.  rows == NULL: store rows [first, first + n). */
int pm_store_rows(pm_session* s, const int32_t* rows, int64_t first, int64_t n, int raw, int32_t* start, uint8_t* strand);
/* the layout image: genome j = words [word_off[j], word_off[j + 1]) (word_off[n_genomes + 1] filled in), n_j + 1 bits, returns the
 * number of words; pm_store_layout copies it out */
int64_t pm_store_layout_words(pm_session* s, int64_t* word_off);
int pm_store_layout(pm_session* s, uint64_t* out, int64_t words);
/* The unaligned runs of the layout, for parsnp.unalign (Aligner::setUnalignableRegions, src/parsnp.cpp:2310-2381), without the
 * image leaving the device.  A run of genome j is a maximal stretch of unmarked bits in [0, n_j + 1) of its slice of the image;
 * it is kept when it has at least 2 bases; its ordinal is its index among ALL runs of its genome, the one-base runs included.
 * pm_store_unalign_count: per genome the number of all runs and of the kept ones (one wait).  pm_store_unalign_runs: start,
 * end (inclusive) and ordinal of every kept run, genome after genome and in position order inside a genome, into arrays of n =
 * the sum of kept_runs entries each (a different n is an error: the layout has changed since the count).  Valid where
 * pm_store_layout is, sharded sessions included; both read the image and change nothing.  Phases `unalign_count` and
 * `unalign_write` in pm_last_timing. */
int pm_store_unalign_count(pm_session* s, int64_t* all_runs, int64_t* kept_runs);
int pm_store_unalign_runs(pm_session* s, int32_t* start, int32_t* end, int32_t* ordinal, int64_t n);
/* Core-genome SNP columns and pairwise SNP distances of alignment columns the caller hands over in chunks of n_rows rows.  Judged
 * case-insensitively, a column is a CORE SNP when every row holds one of A C G T and at least two different letters occur, CORE
 * INVARIANT when every row holds the same one of the four, and OTHER when some row holds anything else ('-', 'N', ...).  n_rows is
 * independent of the session's genomes.  A collection is started with its row count (an earlier one is forgotten); an add takes
 * row i of its chunk at chars + i * pitch (ASCII, any case), numbers the columns across adds in the order added, and reports the
 * running counts (totals may be NULL; n_cols == 0 is a valid add); the columns call gives col[v], the index of core SNP v among all
 * columns added, and letters, n_rows x core_snps, row-major, upper case (either may be NULL; nothing is written for no core SNP);
 * the distances call gives dist, n_rows x n_rows, row-major: the number of core SNP columns in which two rows differ.
 * PM_EINVAL: n_rows < 2, pitch < n_cols, n_cols < 0, chars NULL with n_cols > 0, any call before a collection was started.
 * PM_ELIMIT: more rows than the limits call reports (2 048; it needs no device), or 2^31 or more columns in all.  Phases
 * `snp_classify`, `snp_scan`, `snp_pack` and `snp_dist` in pm_last_timing. */
typedef struct pm_snp_counts { int64_t columns, core_invariant, core_snps, other; } pm_snp_counts;
int pm_snp_limits(int* max_rows);
int pm_snp_begin(pm_session* s, int32_t n_rows);
int pm_snp_add(pm_session* s, int64_t n_cols, int64_t pitch, const uint8_t* chars, pm_snp_counts* totals);
int pm_snp_columns(pm_session* s, int64_t* col, uint8_t* letters);
int pm_snp_distances(pm_session* s, int32_t* dist);
/* Neighbour-joining tree over an n x n matrix of distances (3 <= n <= the limits call's 2 048, which needs no device): the caller's
 * `dist` (row-major, symmetric, zero diagonal, no negative entry: checked on the host before the upload), or with dist == NULL the
 * distances of the session's SNP collection, which must have been computed (pm_snp_distances) and have n rows; they are still on the
 * device.  The tree is DEFINED in INTEGRATION.md 1b: IEEE double arithmetic, every operation rounded once in the order written, ties
 * to the smallest (i, j).  joins: the n - 3 join records in order (slot i keeps the new node, slot j retires; dij, ri, rj are D[i][j],
 * R[i], R[j] before the update; may be NULL for n == 3), last: the three slots left, ascending, and their distances.  Branch lengths
 * and Newick are the caller's (host/tree.cpp): the device never divides.  All launches of a tree are queued without a host wait.
 * PM_EINVAL: n < 3, a matrix that is not symmetric / has a non-zero diagonal / a negative entry, dist NULL without computed SNP
 * distances or with another n.  PM_ELIMIT: n > 2 048.  Phase `nj` in pm_last_timing. */
typedef struct pm_nj_join { int32_t i, j; double dij, ri, rj; } pm_nj_join;
typedef struct pm_nj_last { int32_t a, b, c; double dab, dac, dbc; } pm_nj_last;
int pm_nj_limits(int* max_rows);
int pm_nj_tree(pm_session* s, int32_t n, const int32_t* dist, pm_nj_join* joins, pm_nj_last* last);
/* Bootstrap support of the neighbour-joining tree of the session's SNP collection (DEFINED in INTEGRATION.md 1c; exact, like 1a and
 * 1b).  The limits call reports the rows (2 048), the replicates of a call (1 024) and the largest column weight (15); it needs no
 * device.
 * pm_boot_distances: `reps` weighted distance matrices over the collection's core SNP columns (its own distances need not have been
 * computed).  weights == NULL: replicate b draws V columns with replacement from `seed` (the draws of 1c) and a column's weight is
 * the number of draws that picked it, capped at 15.  Otherwise weights is uint8 [reps][V] with row pitch `pitch`.  weights_out
 * (uint8 [reps][V], packed) and dist_out (int32 [reps][n][n]) may be NULL; the distances stay on the device for pm_nj_trees.
 * PM_EINVAL: no collection started, reps < 1, pitch < V, a weight above 15 (checked on the host before the upload).  PM_ELIMIT:
 * reps > 1 024, or the draw counters of ONE replicate do not fit the batch's budget.  Phases `boot_draw` and `boot_dist`.
 * pm_nj_trees: `count` trees of one n (3 <= n <= 2 048), each the tree of pm_nj_tree bit for bit, the trees of a batch joined in lock
 * step: 2 (n - 3) + 2 launches a batch and no host wait.  dist: the caller's int32 [count][n][n], every matrix checked like
 * pm_nj_tree's; NULL: the first `count` replicate distances on the device.  joins is [count][n - 3] and last is [count]; either may be
 * NULL; the records stay on the device for pm_nj_support.  PM_EINVAL: n < 3, count < 1, a bad matrix, dist NULL without replicate
 * distances of n rows and at least count replicates.  PM_ELIMIT: n > 2 048, count > 1 024.  Phase `boot_nj`.
 * pm_nj_support: support[t] (int32 [n - 3]) = the number of the `count` trees one of whose n - 3 splits equals, as a set of leaves,
 * the split of join t of main_joins (the node of a join holds the leaves of both slots joined; its split is that set, or the
 * complement when leaf 0 is in it).  rep_joins: the caller's [count][n - 3] records, or NULL for the device's (the last
 * pm_nj_trees of this n with at least count trees).  n == 3: nothing to count, nothing is written.  PM_EINVAL: n < 3, count < 1, a
 * caller's record that does not have 0 <= i < j < n with both slots still active, rep_joins NULL without such records on the
 * device.  PM_ELIMIT: n > 2 048, count > 1 024.  Phase `boot_support`.
 * Replicates are worked off in batches (a batch's draw counters within 256 MiB, its trees' matrices within 1 GiB);
 * pm_session_tune(s, "boot_batch", k) forces k a batch (0: the default); no result depends on k. */
int pm_boot_limits(int* max_rows, int* max_reps, int* max_weight);
int pm_boot_distances(pm_session* s, int32_t reps, uint64_t seed, const uint8_t* weights, int64_t pitch, uint8_t* weights_out, int32_t* dist_out);
int pm_nj_trees(pm_session* s, int32_t n, int32_t count, const int32_t* dist, pm_nj_join* joins, pm_nj_last* last);
int pm_nj_support(pm_session* s, int32_t n, const pm_nj_join* main_joins, int32_t count, const pm_nj_join* rep_joins, int32_t* support);
/* Recombination scan of the session's SNP collection (DEFINED in INTEGRATION.md 1d; all integers, exact): the pairwise homoplasy
 * index of windows of sites and its permutation test.  The limits call reports the rows (2 048), the sites of a window (256) and the
 * permutations of a call (65 536); it needs no device.
 * pm_rec_sites: informative[v] (uint8 [V], may be NULL) = 1 where core SNP column v has at least two letters that each occur in at
 * least two rows; n_informative: their number.  The collection's distances need not have been computed.  The planes transposed
 * for this (per column a bit set over the rows) stay on the device until the collection changes.  Phase `rec_sites`.
 * pm_rec_incompat: for every window w (sites[win_off[w]] ... sites[win_off[w + 1] - 1], indices into the V core SNP columns in any
 * order, informative or not) the k x k byte matrix of the pair scores `inc` of 1d, the diagonal 0.  inc_out: the matrices packed one
 * after the other (sum of k^2 bytes), may be NULL; they stay on the device for pm_rec_test.  Phase `rec_incompat`.
 * pm_rec_test: phi[w] = T(identity) and le[w] = the number of the `perms` permutations with T <= phi, for windows of the sizes
 * win_off gives.  inc: the caller's packed matrices, or NULL for those of the last pm_rec_incompat (the sizes must be its).
 * win_id[w]: the window's number g (its keys come from seed + g), NULL: 0, 1, ...  Phase `rec_permute`.
 * PM_EINVAL: no collection started (sites, incompat), a site outside 0 ... V - 1, a win_off that does not ascend or leaves the site
 * list, a window of fewer than 2 sites, near < 1, perms < 1, inc NULL without matrices of these sizes on the device.  PM_ELIMIT: a
 * window of more than 256 sites, perms > 65 536, more than 1 GiB of matrices in one call.  n_windows == 0 is valid and launches
 * nothing.  Windows are worked off in batches; pm_session_tune(s, "rec_batch", k) forces k a batch (0: the default); no result
 * depends on k.  Everything of one call is queued without a wait in between. */
int pm_rec_limits(int* max_rows, int* max_window_sites, int* max_perms);
int pm_rec_sites(pm_session* s, uint8_t* informative, int64_t* n_informative);
int pm_rec_incompat(pm_session* s, int64_t n_sites, const int64_t* sites, int64_t n_windows, const int64_t* win_off, uint8_t* inc_out);
int pm_rec_test(pm_session* s, int64_t n_windows, const int64_t* win_off, const uint8_t* inc, int32_t near, int32_t perms, uint64_t seed,
                const int64_t* win_id, int32_t* phi, int32_t* le);
/* Extension of LCB ends into their flanks (DEFINED in INTEGRATION.md 1e; all integers, exact): a banded alignment of every row's
 * flank against the reference's, a cut common to the rows of a job, the paths and their star merge into columns.  The limits call
 * reports the rows of a job (2 048), the longest flank (512) and the widest band (63); it needs no device.
 * A row is a descriptor into the session's resident genomes: letter q (0 <= q < len) is base first + q step (0-based) of the forward
 * strand of `genome`, complemented where `complement` is 1.  A row may name any genome, any number of times.  The rows of job j are
 * rows[row_off[j]] ... rows[row_off[j + 1] - 1] (row_off[0] = 0), the first of them the reference row.  A base that is none of ACGT
 * matches nothing and prints as N.
 * pm_ext_reach: reach[j] = the job's reach A of 1e (0: dropped).  best: NULL, or for every row (max_flank + 1) int32, best_r(i) for
 * i = 0 ... La and INT32_MIN where it is undefined or i > La (the reference row is aligned with itself like any other).  Phases
 * `ext_reach`, `ext_cut`.
 * pm_ext_align: for the reaches given (those of pm_ext_reach, or any 0 <= reach[j] <= La at which every row of the job has a cell:
 * reach[j] <= len + band for each of its rows; another is PM_EINVAL): used[p] = j_r of every row (0 in a job
 * of reach 0), cols[j] = the job's columns C, 0 for reach 0, -1 where C > 2 max_flank (no letters are written then).  Every byte of
 * the n_j x max_cols block of a job that holds no letter is written as 0.  The row r of job j
 * is written to out_rows + out_off[j] + r max_cols, C letters of ACGTN- in the flank's own order (the column next to the LCB first;
 * a caller that prints a left flank reverses it).  max_cols >= 2 max_flank.  Phases `ext_trace`, `ext_merge`.
 * PM_EINVAL: a parameter outside its range (16 <= max_flank <= 512, 1 <= band <= 63, 1 <= match <= 15, 0 <= mismatch <= 15,
 * 1 <= gap <= 15, 50 <= ani <= 100, 1 <= min_len <= max_flank), a job of fewer than 2 rows, a row_off that does not ascend from 0,
 * a step other than +1 / -1, a len < 0, a descriptor that leaves its genome, a reach outside 0 ... La, max_cols too small.
 * PM_ELIMIT: a len > max_flank, a job of more than 2 048 rows, 2^31 rows or jobs in a call.  n_jobs == 0 is valid and launches nothing.  The
 * pairs are worked off in batches; pm_session_tune(s, "ext_batch", k) forces k pairs a launch (0: the default); no result depends
 * on k. */
typedef struct pm_ext_params { int32_t match, mismatch, gap, band, ani, min_len, max_flank; } pm_ext_params;
typedef struct pm_ext_row { int32_t genome, step, complement, len; int64_t first; } pm_ext_row;
int pm_ext_limits(int* max_rows, int* max_flank, int* max_band);
int pm_ext_reach(pm_session* s, const pm_ext_params* params, int64_t n_jobs, const int64_t* row_off, const pm_ext_row* rows, int32_t* reach, int32_t* best);
int pm_ext_align(pm_session* s, const pm_ext_params* params, int64_t n_jobs, const int64_t* row_off, const pm_ext_row* rows, const int32_t* reach,
                 int64_t max_cols, const int64_t* out_off, uint8_t* out_rows, int32_t* cols, int32_t* used);
/* bytes this session has moved over the host link so far (every copy the engine issued, both directions) */
int pm_session_traffic(const pm_session* s, uint64_t* h2d_bytes, uint64_t* d2h_bytes);

/* calcmumi mode (Aligner::setMumi, src/parsnp.cpp:1869-2115): every query genome ALONE against the reference chunk
 * starts[0],lens[0] (query g: starts[g],lens[g]).  covered[g-1] = number of reference positions covered by the
 * pairwise MUMs of length >= 15 of query g, i.e. total_M_LON of :2064-2069 before the length-ratio and clamp rules
 * (:2074-2077), which stay with the caller together with the "%d:%f" distance (:2080).
 * Replaces, per query: Find_UM x2, Intersect_UM x2, Merge_Master and the coverage loop (:2015-2063). */
int pm_mumi_coverage(pm_session* s, const int64_t* starts, const int64_t* lens, int64_t* covered);

/* Single-strand entry point mirroring Find_UM (src/csgmum/mum.c:177-250) for parity tests: the event stream of one
 * query strand against ref -- every maximal exact match (j, l, len) of length >= min_len whose reference side is unique
 * in ref -- in increasing l.  strand 0: the query as given, 1: its reverse complement (Aligner::reversec).
 * rep[i] is the uniqueness point pos_label - l of mum.c:219-224 (longest repeated prefix of ref[l..)) where it is
 * >= min(min_len,16) and 0 below that (values that small cannot change any MUM).
 * At most cap events are written; *count receives the total. */
int pm_find_events(const uint8_t* ref, int64_t n, const uint8_t* query, int64_t m, int32_t min_len, int strand,
                   int64_t cap, int64_t* count, int64_t* ev_j, int64_t* ev_l, int32_t* ev_len, int32_t* ev_rep);

/* Inter-MUM gap alignment for a whole batch of gaps on the device.  Replaces MuscleInterface::CallMuscleFast
 * (src/MuscleInterface.cpp:37-78; call site src/parsnp.cpp:854-855): libMUSCLE 3.7 with SEQTYPE_DNA, one iteration,
 * ClustalW weights, over the n_seqs[j] gap strings of gap j -- the rows it returns are byte-identical to MUSCLE's.
 *   seq_off[0 .. total_seqs]   offsets into chars of all sequences of all jobs, job after job (ASCII, upper case)
 *   max_cols[j], row_off[j]    row capacity of job j and where its rows go: sequence i of job j is written to
 *                              out_rows[row_off[j] + i*max_cols[j] ..], cols[j] columns of it
 *   cols[j] = -1               the device declined the job (more than 512 sequences, an intermediate alignment wider than
 *                              96 columns or than max_cols[j], an empty sequence, a lower-case letter or a 'U' -- its rows
 *                              are kept as one code byte per column, which round-trips upper-case DNA without 'U' -- or a
 *                              case in which MUSCLE itself quits): the caller aligns it on the host
 * device < 0: PARSNP_DEVICE or the current device.  Returns PM_OK or a PM_E* code (pm_gap_last_error()). */
int pm_gap_align_batch(int device, int64_t n_jobs, const int32_t* n_seqs, const int64_t* seq_off, const uint8_t* chars,
                       const int32_t* max_cols, const int64_t* row_off, uint8_t* out_rows, int64_t out_bytes, int32_t* cols);
/* The same batch in n_groups groups of consecutive jobs (group g = jobs [group_end[g-1], group_end[g]), group_end[n_groups-1]
 * = n_jobs): everything is uploaded once, the groups are aligned one after the other, and as soon as the rows and column
 * counts of group g are in the caller's arrays `done(ctx, g)` is called from the calling thread -- the caller may use them
 * while the later groups are still being aligned (the XMFA writer lays out and writes the records of the LCBs whose gaps
 * are done).  On an error return the groups after the last one reported have not been reported.  done may be NULL.
 * The rows of a group come back as the row areas of its aligned jobs, neighbouring areas in one copy (a group without a
 * declined job, laid out job after job as the batch form lays them out, is ONE copy).  Only those areas are written: the
 * row area of a declined job (cols[j] = -1) and everything outside the row areas keep the caller's bytes; inside the area
 * of an aligned job the bytes behind column cols[j] of a row are unspecified.
 * pm_gap_last_error(): the message of the last failed call of this process, from any thread. */
int pm_gap_align_groups(int device, int64_t n_jobs, const int32_t* n_seqs, const int64_t* seq_off, const uint8_t* chars,
                        const int32_t* max_cols, const int64_t* row_off, uint8_t* out_rows, int64_t out_bytes, int32_t* cols,
                        int n_groups, const int64_t* group_end, void (*done)(void* ctx, int group), void* ctx);
const char* pm_gap_last_error(void);
/* The same call with the device's wide form beside the narrow one.  pm_gap_align_batch and pm_gap_align_groups keep the narrow
 * limits above exactly (512 sequences, 96 bases, 96 columns); this entry point takes every job within pm_gap_limits(1, ...):
 * up to 512 sequences of up to 320 bases each whose intermediate alignments stay within 640 columns -- every gap that the
 * reference driver's default --max-cluster-d 300 can produce.  A job whose sequences all have at most 96 bases runs in the narrow
 * form (same kernel, same LDS, same workgroups per CU as in the two calls above); when the narrow form declines it and
 * max_cols[j] > 96, it runs again in the wide form before its group is reported.  A job with a longer sequence runs in the wide
 * form; per group the narrow jobs are launched first, then the wide ones, each longest first.
 *   cols[j] = -1   only: fewer than 2 or more than 512 sequences, a sequence that is empty or longer than 320 bases, an
 *                  intermediate alignment wider than 640 columns or than max_cols[j], a lower-case letter or a 'U', or a case in
 *                  which MUSCLE itself quits.  No job is declined for the LDS it would need: rows and trace-back bytes that do not
 *                  fit lie in the device workspace.
 * stats (may be NULL): what the call did. */
typedef struct pm_gap_stats {
    int64_t jobs_narrow, jobs_wide;   /* jobs aligned by each form (a job run again in the wide form counts as wide) */
    int64_t declined;                 /* jobs answered with cols = -1 */
    double ms_narrow, ms_wide;        /* kernel time of each form, summed over the launches (HIP events) */
} pm_gap_stats;
int pm_gap_align_groups_wide(int device, int64_t n_jobs, const int32_t* n_seqs, const int64_t* seq_off, const uint8_t* chars,
                             const int32_t* max_cols, const int64_t* row_off, uint8_t* out_rows, int64_t out_bytes, int32_t* cols,
                             int n_groups, const int64_t* group_end, void (*done)(void* ctx, int group), void* ctx, pm_gap_stats* stats);
/* The device gap aligner's limits: wide = 0 those of pm_gap_align_batch / pm_gap_align_groups, wide != 0 those of
 * pm_gap_align_groups_wide.  max_seqs: sequences of a job; max_seq_len: bases of a sequence; max_cols: columns of an
 * alignment.  Any pointer may be NULL.  Needs no device. */
int pm_gap_limits(int wide, int* max_seqs, int* max_seq_len, int* max_cols);
/* The same call with the device's tall form beside the other two: gaps of alignments with more than 512 genomes.  The three entry
 * points above keep their limits exactly; this one takes every job within pm_gap_limits_tall: up to 2 048 sequences (2 000 genomes
 * and the reference in one alignment) of up to 320 bases each whose intermediate alignments stay within 640 columns.  A job of at
 * most 512 sequences runs exactly as in pm_gap_align_groups_wide (narrow or wide form, the second run included); a job of 513 to
 * 2 048 sequences runs in the tall form -- the wide form's kernel with per-sequence arrays of 2 048 entries, its rows in the device
 * workspace when they do not fit the LDS; per group the tall jobs are launched after the wide ones, longest first, on as many
 * slots as 8 GiB of workspace allow (a slot of 2 048 sequences needs 20 MB).
 *   cols[j] = -1   only: fewer than 2 or more than 2 048 sequences, a sequence that is empty or longer than 320 bases, an
 *                  intermediate alignment wider than 640 columns or than max_cols[j], a lower-case letter or a 'U', or a case in
 *                  which MUSCLE itself quits.
 * stats (may be NULL): what the call did; a record of its own, pm_gap_stats keeps its size. */
typedef struct pm_gap_tall_stats {
    int64_t jobs_narrow, jobs_wide, jobs_tall;   /* jobs aligned by each form */
    int64_t declined;                            /* jobs answered with cols = -1 */
    double ms_narrow, ms_wide, ms_tall;          /* kernel time of each form, summed over the launches (HIP events) */
} pm_gap_tall_stats;
int pm_gap_align_groups_tall(int device, int64_t n_jobs, const int32_t* n_seqs, const int64_t* seq_off, const uint8_t* chars,
                             const int32_t* max_cols, const int64_t* row_off, uint8_t* out_rows, int64_t out_bytes, int32_t* cols,
                             int n_groups, const int64_t* group_end, void (*done)(void* ctx, int group), void* ctx, pm_gap_tall_stats* stats);
/* The limits of pm_gap_align_groups_tall (2 048 sequences, 320 bases, 640 columns).  Any pointer may be NULL.  Needs no device. */
int pm_gap_limits_tall(int* max_seqs, int* max_seq_len, int* max_cols);
/* The same call with the device's long form beside the narrow and the wide one: gaps of up to 1 024 bases, what a cluster
 * distance of up to 1 000 (the reference driver's -C/--max-cluster-d, the ini's d=) produces.  The four entry points above keep
 * their limits exactly; this one takes every job within pm_gap_limits_long: up to 512 sequences of up to 1 024 bases each whose
 * intermediate alignments stay within 2 048 columns.  A job with no sequence longer than 320 bases runs exactly as in
 * pm_gap_align_groups_wide (narrow or wide form, the second run included); a job with a longer sequence runs in the long form --
 * one workgroup of four wavefronts per alignment, four 64-row stripes of the pairwise DP in flight at once, its rows and
 * trace-back bytes in the device workspace; per group the long jobs are launched after the wide ones, longest first, with a
 * queue of their own, on one slot per compute unit (as far as 8 GiB of workspace allow: a slot of 512 x 2 048 needs 8 MB).
 * More than 512 sequences COMBINED with a sequence of more than 320 bases is outside this entry point and the one above
 * (pm_gap_align_groups_tall takes more sequences, this entry point longer ones, neither both): pm_gap_align_groups_long_tall below
 * takes such a job.
 *   cols[j] = -1   only: fewer than 2 or more than 512 sequences, a sequence that is empty or longer than 1 024 bases, an
 *                  intermediate alignment wider than 2 048 columns or than max_cols[j], a lower-case letter or a 'U', or a case
 *                  in which MUSCLE itself quits.  No job is declined for the LDS it would need.
 * stats (may be NULL): what the call did; a record of its own, the older ones keep their size. */
typedef struct pm_gap_long_stats {
    int64_t jobs_narrow, jobs_wide, jobs_long;   /* jobs aligned by each form */
    int64_t declined;                            /* jobs answered with cols = -1 */
    double ms_narrow, ms_wide, ms_long;          /* kernel time of each form, summed over the launches (HIP events) */
} pm_gap_long_stats;
int pm_gap_align_groups_long(int device, int64_t n_jobs, const int32_t* n_seqs, const int64_t* seq_off, const uint8_t* chars,
                             const int32_t* max_cols, const int64_t* row_off, uint8_t* out_rows, int64_t out_bytes, int32_t* cols,
                             int n_groups, const int64_t* group_end, void (*done)(void* ctx, int group), void* ctx, pm_gap_long_stats* stats);
/* The limits of pm_gap_align_groups_long (512 sequences, 1 024 bases, 2 048 columns).  Any pointer may be NULL.  Needs no device. */
int pm_gap_limits_long(int* max_seqs, int* max_seq_len, int* max_cols);
/* The same call with the device's long-tall form beside the other four: the whole rectangle of 2 048 sequences x 1 024 bases,
 * what an alignment of more than 511 query genomes run with a raised cluster distance produces.  The five entry points above keep
 * their limits exactly; this one takes every job within pm_gap_limits_long_tall: up to 2 048 sequences of up to 1 024 bases each
 * whose intermediate alignments stay within 2 048 columns.  A job of at most 512 sequences runs exactly as in
 * pm_gap_align_groups_long (narrow, wide or long form, the second run included); a job of 513 to 2 048 sequences with no sequence
 * longer than 320 bases runs in the tall form exactly as in pm_gap_align_groups_tall; a job of 513 to 2 048 sequences with a
 * longer sequence runs in the long-tall form -- the long form's kernel with its per-sequence arrays four times as long and the
 * per-node weight totals in the device workspace; per group the long-tall jobs are launched after the long ones, longest first,
 * with a queue of their own, on one slot per compute unit (as far as 8 GiB of workspace allow: a slot of 2 048 x 2 048 needs 31 MB).
 *   cols[j] = -1   only: fewer than 2 or more than 2 048 sequences, a sequence that is empty or longer than 1 024 bases, an
 *                  intermediate alignment wider than 2 048 columns or than max_cols[j], a lower-case letter or a 'U', or a case
 *                  in which MUSCLE itself quits.  No job is declined for the LDS it would need.
 * stats (may be NULL): what the call did; a record of its own, the older ones keep their size. */
typedef struct pm_gap_long_tall_stats {
    int64_t jobs_narrow, jobs_wide, jobs_tall, jobs_long, jobs_long_tall;   /* jobs aligned by each form */
    int64_t declined;                                                       /* jobs answered with cols = -1 */
    double ms_narrow, ms_wide, ms_tall, ms_long, ms_long_tall;              /* kernel time of each form, summed over the launches (HIP events) */
} pm_gap_long_tall_stats;
int pm_gap_align_groups_long_tall(int device, int64_t n_jobs, const int32_t* n_seqs, const int64_t* seq_off, const uint8_t* chars,
                                  const int32_t* max_cols, const int64_t* row_off, uint8_t* out_rows, int64_t out_bytes, int32_t* cols,
                                  int n_groups, const int64_t* group_end, void (*done)(void* ctx, int group), void* ctx, pm_gap_long_tall_stats* stats);
/* The limits of pm_gap_align_groups_long_tall (2 048 sequences, 1 024 bases, 2 048 columns).  Any pointer may be NULL.  Needs no device. */
int pm_gap_limits_long_tall(int* max_seqs, int* max_seq_len, int* max_cols);

/* Device-side timing of the last pm_multi_mum_batch on this session (HIP events on the engine's stream):
 * names[i] / ms[i] for i < *count (count in: capacity, out: filled).  Used by bench.py's roofline line.
 * A call that took the suffix-array path (see "work_budget") also reports the counts "dense_regions" (regions on the path) and
 * "dense_rounds" (prefix-doubling rounds of its sort), the phases "dense_sa" (suffix array + rep') and "dense_search" (its
 * events), and "dense_overrun" (wall ms of the pass that ran out of budget before it; not with "dense_all").  Other calls
 * report none of these keys.
 * Counts of the index build (see "index_build"): "index_bucketed" -- reference positions of the regions whose index was built by
 * buckets in LDS (0 after a full overflow list sent the call back to IndexInsert); "index_overflow" -- records of them whose probe
 * run reached their bucket's end and went through the overflow list; "index_lost" -- only with "index_verify": its violations. */
int pm_last_timing(const pm_session* s, int* count, const char** names, float* ms);

/* The limits of the kernels that find the events of a recursion batch's small regions (every side at most 128 bases) once per
 * distinct query piece: distinct pieces of a region, events of one (piece, strand), query genomes of the batch.  wide = 0: the
 * first form (32, 8, 1 024); wide != 0: the wide form (128, 32, 2 047), which takes what the first leaves when "group_wide" is set.  A
 * region beyond both is searched pair by pair; pm_last_timing counts them ("n_handed_back"; "n_grouped_wide": the events the wide
 * form wrote).  Any pointer may be NULL. */
int pm_group_limits(int wide, int* max_pieces, int* max_events, int* max_genomes);

#ifdef __cplusplus
}
#endif
#endif
