// dense_kernels.h -- the suffix-array path of the event search, for the regions whose K-mer chain walks ran out of budget.
//
// A tandem repeat of period > 1 with thousands of copies puts thousands of positions on one K-mer chain: RepeatLength
// compares each of them with every other entry, SeedRest walks the whole chain for every sample that hits it -- a cost that
// grows with the square of the copy number.  A region whose walks exhaust the per-thread work budget is flagged (dense[])
// and the batch is run again; in that run the flagged regions get rep' and their queued samples' events from a suffix
// array instead, whose cost does not depend on the copy number (the restatement of oracle/mum_oracle.c on the device):
//   - DenseRank0 .. DenseRerank: one segmented prefix-doubling sort over the flat positions of ALL flagged regions of the
//     batch (initial rank = (flagged region, symbol)), every round's rank array kept;
//   - DenseLcp / DenseRep: LCP of SA neighbours by binary lifting over the kept rounds, rep' = max over both neighbours;
//   - SeedDense: every queued sample of a flagged region (SeedRest's probe items) binary-searches the query suffixes of its
//     owner windows in the region's SA segment.
// "Dense index" = position in the concatenation of the flagged regions: region fi (the fi-th flagged one) holds dense indices
// [dstart[fi], dstart[fi+1]).  Symbols: A=0 C=1 G=2 T=3 (the 2-bit plane) and N=4 (the mask plane); N equals N (csg.c:13-25).
#pragma once
#include "kernels.h"

namespace pm {

constexpr int kDenseMaxLevels = 33;      // rank arrays of prefix lengths 1, 2, 4, ... 2^32 (regions are shorter than 2^31)

PM_HD int sym_at(const SeqBlock* blk, int64_t p) {
    const SeqBlock b = blk[p >> 5];
    const int s = (int)(p & 31);
    return ((b.nm >> s) & 1u) ? 4 : (int)((b.b2 >> (2 * s)) & 3u);
}

// tid = dense index: rank of the one-symbol prefix, made distinct between the flagged regions
struct DenseRank0 {
    Packed P; const RegionInfo* R; const int32_t* dlist; const int64_t* dstart; int64_t nflag; uint32_t* rank;
    PM_HD void operator()(int64_t tid) const {
        const int64_t fi = upper_slot(dstart, nflag, tid);
        const RegionInfo& ri = R[dlist[fi]];
        rank[tid] = (uint32_t)(fi * 5 + sym_at(P.blk, P.goff[0] + ri.ref_pos + (tid - dstart[fi])));
    }
};
// tid = dense index: the sort key of one doubling round, (rank of the first h symbols, rank of the next h + 1 -- 0 where the
// suffix ends before: it sorts before every suffix that goes on)
struct DenseKeys {
    const int64_t* dstart; int64_t nflag; const uint32_t* rank; int64_t h; uint64_t* key; uint64_t* val;
    PM_HD void operator()(int64_t tid) const {
        const int64_t fi = upper_slot(dstart, nflag, tid);
        const uint32_t second = tid + h < dstart[fi + 1] ? rank[tid + h] + 1u : 0u;
        key[tid] = ((uint64_t)rank[tid] << 32) | second;
        val[tid] = (uint64_t)tid;
    }
};
// tid = sorted position t (n + 1 threads): 1 where a new key begins
struct DenseHeads {
    const uint64_t* key; int64_t n; int64_t* head;
    PM_HD void operator()(int64_t t) const { head[t] = t < n && (t == 0 || key[t] != key[t - 1]) ? 1 : 0; }
};
// tid = sorted position t: the dense rank of its key = (keys that begin at or before t) - 1, back to the suffix's own index
struct DenseRerank {
    const uint64_t* val; const int64_t* head; const int64_t* first; uint32_t* rank;
    PM_HD void operator()(int64_t t) const { rank[val[t]] = (uint32_t)(first[t] + head[t] - 1); }
};
// longest common prefix of the suffixes at dense indices a, b of one flagged region (end = its dense end): binary lifting over
// the kept rounds -- equal ranks of round k mean equal prefixes of 2^k symbols, both inside the region
struct DenseLevels { const uint32_t* lv[kDenseMaxLevels]; int top; };      // top: highest round whose ranks may still tie
PM_HD int32_t dense_lcp(const DenseLevels& L, int64_t a, int64_t b, int64_t end) {
    int32_t n = 0;
    for (int k = L.top; k >= 0; k--)
        if (a < end && b < end && L.lv[k][a] == L.lv[k][b]) { a += (int64_t)1 << k; b += (int64_t)1 << k; n += (int32_t)1 << k; }
    return n;
}
// tid = SA position t: LCP with the suffix before it in the same region's segment (0 at the segment's first)
struct DenseLcp {
    DenseLevels L; const uint64_t* sa; const int64_t* dstart; int64_t nflag; int32_t* lcp;
    PM_HD void operator()(int64_t t) const {
        const int64_t fi = upper_slot(dstart, nflag, t);
        lcp[t] = t > dstart[fi] ? dense_lcp(L, (int64_t)sa[t], (int64_t)sa[t - 1], dstart[fi + 1]) : 0;
    }
};
// tid = SA position t: rep'[l] = the longer LCP with the two SA neighbours, 0 below K (what RepeatLength stores)
struct DenseRep {
    const RegionInfo* R; const int32_t* dlist; const uint64_t* sa; const int64_t* dstart; int64_t nflag; const int32_t* lcp; int32_t* rep;
    PM_HD void operator()(int64_t t) const {
        const int64_t fi = upper_slot(dstart, nflag, t);
        const RegionInfo& ri = R[dlist[fi]];
        int32_t v = lcp[t];
        if (t + 1 < dstart[fi + 1] && lcp[t + 1] > v) v = lcp[t + 1];
        rep[ri.posbase + ((int64_t)sa[t] - dstart[fi])] = v >= ri.K ? v : 0;
    }
};

// tid = queued sample (SeedRest's queue): a probe item (l < 0) of a flagged region.  Instead of walking the chain of its K-mer,
// the sample finds every event whose left end lies in its owner window -- forward strand j0 in (j - stride, j], mirrored piece
// jr0 in (jr - stride, jr] with jr = m - K - j (the left < stride rule of SeedRest's forward_seed / reverse_seed) -- from the
// longest match of each of those query suffixes in the region: (l0, ms) is an event iff ms >= minlen, ms > rep'[l0] (unique in
// R) and the match is left-maximal.  minlen = K + stride - 1: such a match contains the sample's K-mer, so the owner windows of
// the queued samples hold every event the walks would have found, and no other sample emits one of them.
struct SeedDense {
    Packed P; const RegionInfo* R; const UnitRec* units; const RestItem* queue; const uint64_t* queue_count; uint64_t queue_cap;
    const int32_t* dfi; const int64_t* dstart; const uint64_t* sa; const int32_t* rep;
    uint64_t* ev_key; uint64_t* ev_val; uint64_t* ev_counters; uint64_t slice_cap; int lbits;
    // (l0, ms) of the longest match of the query suffix at global qpos (qlen bases) in SA segment [s0, s1) of a region at rpos
    PM_HD int32_t longest(int64_t qpos, int32_t qlen, int64_t rpos, int32_t nR, int64_t s0, int64_t s1, int32_t* l_out) const {
        int64_t lo = s0 - 1, hi = s1;      // suffix(lo) < query <= suffix(hi); lo, hi outside the segment: no suffix
        int32_t llo = 0, lhi = 0;          // the query's LCP with suffix(lo), suffix(hi)
        while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            const int32_t l = (int32_t)((int64_t)sa[mid] - s0);
            const int32_t rlen = nR - l;
            const int32_t c0 = llo < lhi ? llo : lhi;      // what both bounds share with the query, suffix(mid) shares too
            const int32_t most = qlen < rlen ? qlen : rlen;
            const int32_t c = c0 + lce_fwd64(P, qpos + c0, rpos + l + c0, most - c0);
            bool below;      // query < suffix(mid)
            if (c == qlen) below = true;
            else if (c == rlen) below = false;
            else below = sym_at(P.blk, qpos + c) < sym_at(P.blk, rpos + l + c);
            if (below) { hi = mid; lhi = c; } else { lo = mid; llo = c; }
        }
        if (lo >= s0 && (hi >= s1 || llo >= lhi)) { *l_out = (int32_t)((int64_t)sa[lo] - s0); return llo; }
        if (hi < s1) { *l_out = (int32_t)((int64_t)sa[hi] - s0); return lhi; }
        *l_out = -1; return 0;
    }
    PM_HD void operator()(int64_t tid) const {
        const uint64_t sub = (uint64_t)tid / queue_cap, idx = (uint64_t)tid % queue_cap;
        const uint64_t have = queue_count[sub * kSliceStride];
        if (idx >= (have < queue_cap ? have : queue_cap)) return;
        const RestItem it = queue[tid];
        if (it.l >= 0) return;                               // reverse seeds confirmed by SeedExtend: SeedRest
        const UnitRec rec = units[it.unit];
        const int32_t fi = dfi[rec.region];
        if (fi < 0) return;                                  // not a flagged region: SeedRest walks
        const RegionInfo& ri = R[rec.region];
        const int64_t s0 = dstart[fi], s1 = dstart[fi + 1];
        const int64_t m = rec.m;
        const int64_t rbase = P.goff[0] + ri.ref_pos;
        const int32_t K = ri.K, stride = ri.stride;
        const uint64_t slice = (uint64_t)((tid >> 8) & (kSlices - 1));      // one sub-buffer per workgroup, as SeedRest
        uint64_t* ev_count = ev_counters + slice * kSliceStride;
        const int64_t j = (int64_t)it.sample * stride;
        for (int strand = 0; strand < 2; strand++) {
            const int64_t top = strand ? m - K - j : j;      // the sample's K-mer on this strand
            const int64_t qb = strand ? rec.qbase_r : rec.qbase;
            for (int64_t j0 = top; j0 > top - stride && j0 >= 0; j0--) {
                if (m - j0 < ri.minlen) continue;
                int32_t l0;
                const int32_t ms = longest(qb + j0, (int32_t)(m - j0), rbase, ri.nR, s0, s1, &l0);
                if (l0 < 0 || ms < ri.minlen || ms <= rep[ri.posbase + l0]) continue;
                if (j0 > 0 && l0 > 0 && sym_at(P.blk, qb + j0 - 1) == sym_at(P.blk, rbase + l0 - 1)) continue;      // not left-maximal
                const uint64_t ek = ((((uint64_t)rec.pair << lbits) | (uint64_t)l0) << 1) | (uint64_t)strand;
                const uint64_t at = atomic_add64(ev_count, 1);
                if (at < slice_cap) { ev_key[slice * slice_cap + at] = ek; ev_val[slice * slice_cap + at] = ((uint64_t)j0 << 32) | (uint32_t)ms; }
            }
        }
    }
};

}  // namespace pm
