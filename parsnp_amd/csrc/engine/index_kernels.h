// parsnp_amd/csrc/engine/index_kernels.h -- the reference index of large regions, built by buckets in LDS.
//
// IndexInsert (kernels.h) inserts every reference position with a compare-and-swap in global memory: two memory-side atomics and a
// random read per position into a table that was cleared just before, and RepeatLength then reads a random slot per position only
// to learn that its K-mer occurs once.  A region whose slot table has at least `index_bucket_min` slots is built here instead:
//   IndexKeys          one 64-bit key per reference position: (global bucket of its K-mer's home slot, flat position); a position
//                      that starts no K-mer, or lies in a region that is not bucketed, gets the bucket number past the last one;
//                      next[] and rep[] (the slot handed to RepeatLength) of the bucketed regions are set to -1 here
//   sort_keys          by the bucket bits only (stable: the positions of a bucket stay ascending)
//   IndexBucketBounds  first record of every bucket, a search per bucket
//   IndexBucketFill    one wavefront per bucket: the bucket's 2^sb slots and its piece of the presence filter are built in LDS and
//                      written out once, empty slots included (the slice needs no clear); next[] and rep[] only for chain members
//   IndexOverflow      the records whose probe run reached the bucket's end, by IndexInsert's global loop from their home slot
// The slot index, the table's meaning (linear probing over the region's slice, entries never removed) and the readers are
// unchanged.  WHICH occurrence of a repeated K-mer is the head of its chain, and the order of the chain, differ from IndexInsert's:
// they already differ from run to run there (the order in which the threads' atomics arrive), and no reader depends on them.
#pragma once
#include "kernels.h"

namespace pm {

constexpr int kBucketBits = 10;                      // slots of a bucket at most: 8 KB of LDS
constexpr int kBucketSlots = 1 << kBucketBits;
constexpr int kBucketFilterBits = 14;                // filter bits of a bucket at most: 2 KB of LDS (10 KB a wavefront: 16 wavefronts a CU)
constexpr int kBucketFilterWords = 1 << (kBucketFilterBits - 5);

// tid = flat reference position over the batch.  bbase[r]: first global bucket of region r (bbase[nregions]: number of buckets)
struct IndexKeys {
    Packed P; const RegionInfo* R; int64_t nregions; const int64_t* posbase; const int64_t* bbase; int pbits;
    uint64_t* key; int32_t* next; int32_t* home;
    PM_HD void operator()(int64_t tid) const {
        const int64_t r = upper_slot(posbase, nregions, tid);
        const RegionInfo& ri = R[r];
        uint64_t b = (uint64_t)bbase[nregions];
        if (ri.pad_ & kBucketed) {
            const int32_t l = (int32_t)(tid - ri.posbase);
            next[tid] = -1; home[tid] = -1;
            if (l + ri.K <= ri.nR) {
                const uint64_t hv = hash_tag(canonical_tag(kmer_tag(P, P.goff[0] + ri.ref_pos + l, ri.K), ri.K));
                b = (uint64_t)bbase[r] + (((uint32_t)hv & ri.tmask) >> region_sb(ri));
            }
        }
        key[tid] = (b << pbits) | (uint64_t)tid;
    }
};
// tid = key: its bucket number alone (for a backend that sorts pairs only: engine_core.h)
struct IndexKeyBuckets {
    const uint64_t* key; int pbits; uint64_t* bucket;
    PM_HD void operator()(int64_t tid) const { bucket[tid] = key[tid] >> pbits; }
};
// tid = global bucket, 0 .. number of buckets (the last entry: the end of the records)
struct IndexBucketBounds {
    const uint64_t* key; int64_t n; int pbits; int64_t* begin;
    PM_HD void operator()(int64_t b) const {
        const uint64_t want = (uint64_t)b << pbits;
        int64_t a = 0, z = n;
        while (a < z) { const int64_t mid = (a + z) >> 1; if (key[mid] < want) a = mid + 1; else z = mid; }
        begin[b] = a;
    }
};

// one occurrence into a slot sequence in GLOBAL memory, from slot h of the region's slice: IndexInsert's loop, with next[] and
// home[] written for the members of chains only (the head that was alone until now becomes one)
PM_HD void index_insert_global(const Packed& P, const RegionInfo& ri, uint64_t* slots, int32_t* next, int32_t* home, int32_t l, uint64_t tag, uint64_t fp, uint32_t h) {
    const int64_t base = P.goff[0] + ri.ref_pos;
    for (;;) {
        uint64_t* slot = &slots[ri.tbase + h];
        uint64_t seen = *slot;
        if (seen == kEmpty) {
            seen = atomic_cas64(slot, kEmpty, fp | (uint64_t)l);
            if (seen == kEmpty) return;
        }
        if ((seen & 0xffffffff00000000ull) == fp && canonical_tag(kmer_tag(P, base + slot_head(seen), ri.K), ri.K) == tag) {
            for (;;) {
                next[ri.posbase + l] = slot_head(seen);
                const uint64_t prev = atomic_cas64(slot, seen, fp | kMulti | (uint64_t)l);
                if (prev == seen) {
                    home[ri.posbase + l] = (int32_t)h;
                    if (!(seen & kMulti)) home[ri.posbase + slot_head(seen)] = (int32_t)h;
                    return;
                }
                seen = prev;
            }
        }
        h = (h + 1) & ri.tmask;
    }
}

// wave(w) = global bucket w.  Records of the bucket 64 at a time; a lane takes one.  Neighbouring lanes that carry the same K-mer
// (a run of N, a homopolymer: the records of a bucket are in position order) form a run that its first lane inserts as a whole --
// the run is linked in registers and costs one LDS update, as in EventBucketCount -- so a K-mer with millions of occurrences is
// 1/64 of its occurrences in LDS updates, not 64 retries a round.  The probe run does not wrap inside the bucket: a record that
// reaches the bucket's end without a match or a free slot goes to the overflow list (so do all records of its K-mer, before and
// after it: the slots it passed stay full).  Every loop is bounded by a wave-uniform count; no lane waits for memory to change.
struct IndexBucketFill {
    Packed P; const RegionInfo* R; int64_t nregions; const int64_t* bbase; const uint64_t* key; const int64_t* begin; int pbits;
    uint64_t* slots; uint32_t* filter; int32_t* next; int32_t* home;
    uint64_t* ovf_count; int64_t* ovf; uint64_t ovf_cap;      // overflow list: flat positions (the count keeps counting past the capacity)
    PM_HD void wave(int64_t w) const {
        const int64_t r = upper_slot(bbase, nregions, w);
        const RegionInfo& ri = R[r];
        const uint32_t sb = region_sb(ri), fb = region_fb(ri);
        const int32_t nslots = 1 << sb, nfw = 1 << (fb - 5);
        const uint32_t bk = (uint32_t)(w - bbase[r]);               // the bucket inside the region
        const int64_t base = P.goff[0] + ri.ref_pos;
        const int64_t a = begin[w], e = begin[w + 1];
        const uint64_t pmask = (1ull << pbits) - 1;
        uint64_t* out = slots + ri.tbase + ((int64_t)bk << sb);
        uint32_t* fout = filter + ri.fbase + ((int64_t)bk << (fb - 5));
#if defined(__HIP_DEVICE_COMPILE__)
        __shared__ uint64_t s_tab[kBucketSlots];
        __shared__ uint32_t s_fil[kBucketFilterWords];
        const int lane = (int)__lane_id();
        for (int32_t i = lane; i < nslots; i += 64) s_tab[i] = kEmpty;
        for (int32_t i = lane; i < nfw; i += 64) s_fil[i] = 0;
        __syncthreads();
        for (int64_t i0 = a; i0 < e; i0 += 64) {
            const bool act = i0 + lane < e;
            int32_t l = 0; uint64_t tag = ~0ull, fp = 0; int32_t hl = 0;
            if (act) {
                l = (int32_t)((int64_t)(key[i0 + lane] & pmask) - ri.posbase);
                tag = canonical_tag(kmer_tag(P, base + l, ri.K), ri.K);
                const uint64_t hv = hash_tag(tag);
                fp = hv & 0xffffffff00000000ull;
                const uint32_t h = (uint32_t)hv & ri.tmask;
                hl = (int32_t)(h & (uint32_t)(nslots - 1));
                const uint32_t bit = filter_bit(ri, hv, h) & ((1u << fb) - 1u);
                atomicOr(&s_fil[bit >> 5], filter_mask(hv, bit));
            }
            // runs of one K-mer over neighbouring lanes (a tag is 48 bits: ~0 is none)
            const uint64_t ptag = ((uint64_t)(uint32_t)__shfl_up((int)(tag >> 32), 1, 64) << 32) | (uint32_t)__shfl_up((int)(uint32_t)tag, 1, 64);
            const int32_t pl = __shfl_up(l, 1, 64);
            const bool head = act && (lane == 0 || ptag != tag);
            const unsigned long long heads = __ballot(head), acts = __ballot(act);
            const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
            const int upto = above ? __ffsll((long long)above) - 1 : __popcll(acts);      // (for a head: one past its run's last lane)
            const int32_t l_last = __shfl(l, head ? upto - 1 : lane, 64);
            const bool run_many = head && upto - lane > 1;
            // the heads probe: look, then claim an empty slot or push onto the chain of their K-mer; a lost compare-and-swap means
            // that another lane of this round won that slot, which happens at most 63 times in a round
            bool pending = head;
            int32_t at = -1, below = -1;      // where the run went (-1: overflow); the head it was pushed onto (-1: none)
            for (int32_t it = 0; it < nslots + 64; it++) {
                if (!__any(pending)) break;
                if (!pending) continue;
                if (hl >= nslots) { pending = false; continue; }      // the bucket's end: overflow
                uint64_t seen = s_tab[hl];
                if (seen == kEmpty) {
                    const uint64_t mine = fp | (run_many ? kMulti : 0) | (uint64_t)(uint32_t)l_last;
                    seen = (uint64_t)atomicCAS((unsigned long long*)&s_tab[hl], (unsigned long long)kEmpty, (unsigned long long)mine);
                    if (seen == kEmpty) { at = hl; pending = false; continue; }
                }
                if ((seen & 0xffffffff00000000ull) == fp && canonical_tag(kmer_tag(P, base + slot_head(seen), ri.K), ri.K) == tag) {
                    const uint64_t mine = fp | kMulti | (uint64_t)(uint32_t)l_last;
                    const uint64_t prev = (uint64_t)atomicCAS((unsigned long long*)&s_tab[hl], (unsigned long long)seen, (unsigned long long)mine);
                    if (prev == seen) {
                        at = hl; below = slot_head(seen); pending = false;
                        if (!(seen & kMulti)) home[ri.posbase + below] = (int32_t)(((uint32_t)bk << sb) + (uint32_t)hl);      // the head that was alone
                    }
                    continue;      // (lost: the same slot again, it holds this K-mer)
                }
                hl++;
            }
            // every record learns from its run's head where the run went
            const unsigned long long upto_me = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
            const int mine_head = upto_me ? 63 - __clzll((long long)upto_me) : 0;
            const int32_t r_at = __shfl(at, mine_head, 64), r_below = __shfl(below, mine_head, 64);
            const int r_upto = __shfl(upto, mine_head, 64);
            if (act) {
                if (r_at < 0) {
                    const uint64_t o = atomic_add64(ovf_count, 1);      // (not returning per position: per overflowing record)
                    if (o < ovf_cap) ovf[o] = ri.posbase + l;
                } else if (r_below >= 0 || r_upto - mine_head > 1) {    // a chain of two or more
                    next[ri.posbase + l] = lane == mine_head ? r_below : pl;
                    home[ri.posbase + l] = (int32_t)(((uint32_t)bk << sb) + (uint32_t)r_at);
                }
            }
        }
        __syncthreads();
        for (int32_t i = lane; i < nslots; i += 64) out[i] = s_tab[i];
        for (int32_t i = lane; i < nfw; i += 64) fout[i] = s_fil[i];
#else
        uint64_t s_tab[kBucketSlots]; uint32_t s_fil[kBucketFilterWords];
        for (int32_t i = 0; i < nslots; i++) s_tab[i] = kEmpty;
        for (int32_t i = 0; i < nfw; i++) s_fil[i] = 0;
        for (int64_t i = a; i < e; i++) {
            const int32_t l = (int32_t)((int64_t)(key[i] & pmask) - ri.posbase);
            const uint64_t tag = canonical_tag(kmer_tag(P, base + l, ri.K), ri.K);
            const uint64_t hv = hash_tag(tag);
            const uint64_t fp = hv & 0xffffffff00000000ull;
            const uint32_t h = (uint32_t)hv & ri.tmask;
            const uint32_t bit = filter_bit(ri, hv, h) & ((1u << fb) - 1u);
            s_fil[bit >> 5] |= filter_mask(hv, bit);
            int32_t hl = (int32_t)(h & (uint32_t)(nslots - 1));
            for (;; hl++) {
                if (hl >= nslots) {
                    const uint64_t o = atomic_add64(ovf_count, 1);
                    if (o < ovf_cap) ovf[o] = ri.posbase + l;
                    break;
                }
                const uint64_t seen = s_tab[hl];
                if (seen == kEmpty) { s_tab[hl] = fp | (uint64_t)(uint32_t)l; break; }
                if ((seen & 0xffffffff00000000ull) == fp && canonical_tag(kmer_tag(P, base + slot_head(seen), ri.K), ri.K) == tag) {
                    const int32_t slot = (int32_t)(((uint32_t)bk << sb) + (uint32_t)hl);
                    s_tab[hl] = fp | kMulti | (uint64_t)(uint32_t)l;
                    next[ri.posbase + l] = slot_head(seen); home[ri.posbase + l] = slot;
                    if (!(seen & kMulti)) home[ri.posbase + slot_head(seen)] = slot;
                    break;
                }
            }
        }
        for (int32_t i = 0; i < nslots; i++) out[i] = s_tab[i];
        for (int32_t i = 0; i < nfw; i++) fout[i] = s_fil[i];
#endif
    }
};
// tid = entry of the overflow list (launched over its capacity; the count stays on the device)
struct IndexOverflow {
    Packed P; const RegionInfo* R; int64_t nregions; const int64_t* posbase; const uint64_t* ovf_count; const int64_t* ovf; uint64_t ovf_cap;
    uint64_t* slots; int32_t* next; int32_t* home;
    PM_HD void operator()(int64_t tid) const {
        const uint64_t n = *ovf_count;
        if ((uint64_t)tid >= n || n > ovf_cap) return;      // (a full list: the call builds these regions again with IndexInsert)
        const int64_t pos = ovf[tid];
        const RegionInfo& ri = R[upper_slot(posbase, nregions, pos)];
        const int32_t l = (int32_t)(pos - ri.posbase);
        const uint64_t tag = canonical_tag(kmer_tag(P, P.goff[0] + ri.ref_pos + l, ri.K), ri.K);
        const uint64_t hv = hash_tag(tag);
        index_insert_global(P, ri, slots, next, home, l, tag, hv & 0xffffffff00000000ull, (uint32_t)hv & ri.tmask);
    }
};

// (tests: tune index_verify) tid = flat reference position, after the build: the K-mer that starts there must be found by
// index_lookup in a slot whose chain holds the position, its filter word must pass, and a position in no chain has next = -1
struct IndexVerify {
    Packed P; const RegionInfo* R; int64_t nregions; const int64_t* posbase; const uint64_t* slots; const uint32_t* filter; const int32_t* next; uint64_t* lost;
    PM_HD void operator()(int64_t tid) const {
        const RegionInfo& ri = R[upper_slot(posbase, nregions, tid)];
        const int32_t l = (int32_t)(tid - ri.posbase);
        bool bad = false;
        if (l + ri.K > ri.nR) bad = next[tid] != -1;
        else {
            const uint64_t tag = canonical_tag(kmer_tag(P, P.goff[0] + ri.ref_pos + l, ri.K), ri.K);
            const uint64_t hv = hash_tag(tag);
            const uint32_t bit = filter_bit(ri, hv, (uint32_t)hv & ri.tmask);
            const uint32_t fm = filter_mask(hv, bit);
            const uint64_t slot = index_lookup(P, ri, slots, filter, tag);
            if ((filter[ri.fbase + (bit >> 5)] & fm) != fm || slot == kEmpty) bad = true;
            else if (!(slot & kMulti)) bad = slot_head(slot) != l || next[tid] != -1;
            else {
                int32_t o = slot_head(slot);
                for (int32_t steps = 0; o >= 0 && o != l && steps < ri.nR; steps++) o = next[ri.posbase + o];
                bad = o != l;
            }
        }
        if (bad) atomic_add64(lost, 1);
    }
};

}  // namespace pm
