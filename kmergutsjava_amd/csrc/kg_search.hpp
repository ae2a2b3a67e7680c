// kg_search.hpp -- device side of kg_proteins_search / kg_proteins_search_device (include/kmerguts_hip.h states the rule): the
// queries' 8-mers joined with the database's, the shared-k-mer count per (query, target), the best few targets per query, and
// the order of a query's aligned candidates.  Integers only.
//
// The front half is the cluster call's (kg_derive.hpp): every valid window becomes key = v * 2^b + p, the radix sort orders the
// keys, derive_collapse_kernel leaves the distinct (k-mer, protein) pairs pk[P].  Targets have the smaller indices, so within a
// k-mer's run of pairs the targets come first and the queries behind them.  Behind it:
//
//   1. search_kmer_heads_kernel     per pair: the k-mer run head flag; a prefix sum and cluster_link_starts_kernel give the runs
//   2. search_run_weights_kernel    per run: the split nd(v) by a binary search for n_db inside the run, nq = the rest, and
//                                   w(v) = nd * nq in 64 bits where 1 <= nd <= max_db_per_kmer and nq >= 1, else 0.  The 64-bit sum
//                                   of the weights is kept by one integer atomic per wave (the stored weights are saturated at
//                                   2^32 - 1, so prefix_sum's total, though exact, is not theirs: the limit check uses this sum)
//   3. search_run_compact_kernel    the runs of weight >= 1 compacted by a prefix sum of their flags: every listed run has
//                                   weight >= 1, so wx, the prefix sum of the listed weights, is strictly increasing and a tile
//                                   of kSearchTile items touches at most kSearchTile runs
//   4. search_join_kernel           item j of the join_pairs items: run r with wx[r] <= j < wx[r + 1], t = j - wx[r],
//                                   pair (t / nd, t % nd) -> key = q * 2^bits(n_db) + d
//   5. the radix sort, derive_key_heads_kernel, a prefix sum and cluster_link_starts_kernel: runs of equal keys = distinct (q, d),
//      run length = s(q, d)
//   6. search_cand_flags_kernel / search_cand_emit_kernel
//                                   s >= min_shared, compacted in (q, d) order; the largest s of the call; the second sort's keys
//                                   q * 2^sb + (smax - s) with the record index as the value
//   7. the radix sort again (stable: ties of s stay in ascending d), search_query_heads_kernel, a prefix sum and
//      cluster_link_starts_kernel: the rank within the query = the index minus the query's run start
//      search_top_flags_kernel / search_top_emit_kernel: ranks below max_cand, compacted: (query, target) pairs and s
//   8. align_run (kg_host_align.hpp), unchanged
//   9. search_order_kernel          one wave per query, one lane per candidate: the ratio test, the rank under the output order
//                                   by a shuffle sweep over the wave, the 40-byte record at hit_start[q] + rank
//
// What bounds a lane's work: steps 1, 3, 6 and 7 are one item per lane; step 2 is one binary search inside a run (log2 of its
// length); step 4 is kSearchTile / kSearchThreads items per lane, two per binary search over at most kSearchTile LDS words; step 9
// is a sweep over the query's candidates, at most 64.  No run is walked by one lane and no loop's length depends on another lane.
// The join tile: the workgroup's first and last run are found by one binary search each over wx (every lane computes the same
// two, so nothing is handed from lane 0 to the rest and no loop stands round lane-0 work), the runs' wx, start and nd go to LDS, and
// each lane places two consecutive items per step so that the keys leave as 16 bytes a lane, 1 KiB a wave: full lines.
#pragma once

#include "kg_device.hpp"
#include "kg_cluster.hpp"
#include "kg_align.hpp"

namespace kg {

constexpr int kSearchThreads = 256;
constexpr int kSearchTile = 2048;                   // consecutive join items of one workgroup
constexpr int kSearchMaxCand = 64;                  // one lane per candidate of a query
constexpr uint32_t kSearchSat = 0xFFFFFFFFu;        // a weight of 2^32 or more, as stored
// the counter words of a call
enum : int { kSearchJoinPairs = 0, kSearchJoined = 1, kSearchMasked = 2, kSearchSmax = 3, kSearchHits = 4, kSearchBelow = 5,
             kSearchSkipped = 6, kSearchQueriesHit = 7, kSearchWords = 8 };

__device__ __forceinline__ unsigned long long search_wave_sum(unsigned long long v)
{
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// rank_of[p] = p: the derive emit kernel ranks proteins; here the index is the rank
__global__ __launch_bounds__(256) void search_init_kernel(uint32_t n, uint32_t *__restrict__ rank_of)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rank_of[i] = i;
}

// pair j = (k-mer, protein) in sorted order: kh[j] = 1 where its k-mer differs from the pair before
__global__ __launch_bounds__(256) void search_kmer_heads_kernel(const uint64_t *__restrict__ pk, uint64_t n, uint32_t b, uint32_t *__restrict__ kh)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    kh[j] = (j == 0 || (pk[j - 1] >> b) != (pk[j] >> b)) ? 1u : 0u;
}

// k-mer run r = pairs [kstart[r], kstart[r + 1]): nd[r] = its targets, w[r] = its weight (saturated), wf[r] = weight >= 1;
// words: the 64-bit sum of the weights, the joined and the masked k-mers (one atomic per wave each)
__global__ __launch_bounds__(256) void search_run_weights_kernel(const uint64_t *__restrict__ pk, const uint32_t *__restrict__ kstart,
                                                                 uint64_t n_runs, uint32_t b, uint32_t n_db, uint32_t max_db,
                                                                 uint32_t *__restrict__ nd_out, uint32_t *__restrict__ w,
                                                                 uint32_t *__restrict__ wf, unsigned long long *__restrict__ words)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long weight = 0;
    bool masked = false;
    if (r < n_runs) {
        const uint32_t lo = kstart[r], hi = kstart[r + 1];
        const uint64_t mask = (1ull << b) - 1;
        uint32_t a = lo, z = hi;                        // the first pair of the run whose protein is a query
        while (a < z) {
            const uint32_t mid = a + (z - a) / 2;
            if ((uint32_t)(pk[mid] & mask) < n_db) a = mid + 1; else z = mid;
        }
        const uint32_t nd = a - lo, nq = hi - a;
        masked = nd > max_db;
        if (nd >= 1 && !masked && nq >= 1) weight = (unsigned long long)nd * nq;
        nd_out[r] = nd;
        w[r] = weight > kSearchSat ? kSearchSat : (uint32_t)weight;
        wf[r] = weight ? 1u : 0u;
    }
    const unsigned long long joined = __ballot(weight != 0), mk = __ballot(masked);
    const unsigned long long sum = search_wave_sum(weight);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (sum) atomicAdd(&words[kSearchJoinPairs], sum);
        if (joined) atomicAdd(&words[kSearchJoined], (unsigned long long)__popcll(joined));
        if (mk) atomicAdd(&words[kSearchMasked], (unsigned long long)__popcll(mk));
    }
}

// the runs with wf[r] to their places wpos[r] (the exclusive scan of wf): first pair, targets, weight
__global__ __launch_bounds__(256) void search_run_compact_kernel(const uint32_t *__restrict__ kstart, const uint32_t *__restrict__ nd,
                                                                 const uint32_t *__restrict__ w, const uint32_t *__restrict__ wf,
                                                                 const uint32_t *__restrict__ wpos, uint64_t n_runs, uint64_t n_listed,
                                                                 uint32_t *__restrict__ cstart, uint32_t *__restrict__ cnd,
                                                                 uint32_t *__restrict__ cw)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs || !wf[r]) return;
    const uint32_t o = wpos[r];
    if (o >= n_listed) return;
    cstart[o] = kstart[r];
    cnd[o] = nd[r];
    cw[o] = w[r];
}

// the largest r in [0, n) with wx[r] <= j (wx[0] = 0)
__device__ __forceinline__ uint32_t search_run_of(const uint32_t *wx, uint32_t n, uint32_t j)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (wx[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// Workgroup g places items [g * kSearchTile, (g + 1) * kSearchTile) of the n_items join items.  wx[n_runs + 1]: the exclusive
// scan of the listed runs' weights (all >= 1), wx[n_runs] = n_items; cstart / cnd: a run's first pair in pk and its targets.
// keys[j] = q << db | d, vals[j] = 0.
__global__ __launch_bounds__(kSearchThreads) void search_join_kernel(const uint64_t *__restrict__ pk, const uint32_t *__restrict__ wx,
                                                                     const uint32_t *__restrict__ cstart, const uint32_t *__restrict__ cnd,
                                                                     uint32_t n_runs, uint32_t n_items, uint32_t b, uint32_t n_db,
                                                                     uint32_t db, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    __shared__ uint32_t s_wx[kSearchTile], s_start[kSearchTile], s_nd[kSearchTile];
    const uint32_t j0 = blockIdx.x * (uint32_t)kSearchTile;
    if (j0 >= n_items) return;
    const uint32_t j1 = n_items - j0 > (uint32_t)kSearchTile ? j0 + kSearchTile : n_items;
    // the same two searches in every lane: the tile's first and last run
    const uint32_t r0 = search_run_of(wx, n_runs, j0), r1 = search_run_of(wx, n_runs, j1 - 1);
    uint32_t nr = r1 - r0 + 1;
    nr = nr > (uint32_t)kSearchTile ? (uint32_t)kSearchTile : nr;      // (weights >= 1: it never is more)
    for (uint32_t k = threadIdx.x; k < nr; k += kSearchThreads) {
        s_wx[k] = wx[r0 + k];
        s_start[k] = cstart[r0 + k];
        s_nd[k] = cnd[r0 + k];
    }
    __syncthreads();
    const uint64_t mask = (1ull << b) - 1;
    for (uint32_t base = j0 + 2 * threadIdx.x; base < j1; base += 2 * kSearchThreads) {
        uint32_t k = search_run_of(s_wx, nr, base);
        uint64_t key[2] = {0, 0};
        const int cnt = j1 - base >= 2 ? 2 : 1;
        for (int i = 0; i < cnt; i++) {
            const uint32_t j = base + i;
            if (i && k + 1 < nr && s_wx[k + 1] <= j) k++;   // (the next item is in this run or in the next: weights >= 1)
            const uint32_t t = j - s_wx[k], nd = s_nd[k], start = s_start[k];
            const uint32_t qi = t / nd, di = t - qi * nd;
            const uint32_t d = (uint32_t)(pk[start + di] & mask), q = (uint32_t)(pk[start + nd + qi] & mask) - n_db;
            key[i] = ((uint64_t)q << db) | d;
        }
        if (cnt == 2) {
            *reinterpret_cast<ulonglong2 *>(keys + base) = make_ulonglong2(key[0], key[1]);     // (base is even: 16-byte aligned)
            *reinterpret_cast<uint2 *>(vals + base) = make_uint2(0u, 0u);
        } else {
            keys[base] = key[0];
            vals[base] = 0;
        }
    }
}

// distinct (q, d) r with s = lstart[r + 1] - lstart[r]: cf[r] = s >= min_shared; words[kSearchSmax] = the largest such s
__global__ __launch_bounds__(256) void search_cand_flags_kernel(const uint32_t *__restrict__ lstart, uint64_t n_runs, uint32_t min_shared,
                                                                uint32_t *__restrict__ cf, unsigned long long *__restrict__ words)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s = 0;
    if (r < n_runs) {
        s = lstart[r + 1] - lstart[r];
        s = s >= min_shared ? s : 0u;
        cf[r] = s ? 1u : 0u;
    }
    uint32_t big = s;
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)big, d);
        big = o > big ? o : big;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && big) atomicMax(&words[kSearchSmax], (unsigned long long)big);
}

// candidate cx[r] of every flagged (q, d): ckey = its join key, cs = s, and the second sort's pair: key q << sb | (smax - s), the
// candidate's index as the value
__global__ __launch_bounds__(256) void search_cand_emit_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ lstart,
                                                               const uint32_t *__restrict__ cf, const uint32_t *__restrict__ cx,
                                                               uint64_t n_runs, uint64_t n_cand, uint32_t db, uint32_t sb, uint32_t smax,
                                                               uint64_t *__restrict__ ckey, uint32_t *__restrict__ cs,
                                                               uint64_t *__restrict__ skey, uint32_t *__restrict__ sval)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs || !cf[r]) return;
    const uint32_t o = cx[r];
    if (o >= n_cand) return;
    const uint32_t first = lstart[r], s = lstart[r + 1] - first;
    const uint64_t key = keys[first];
    ckey[o] = key;
    cs[o] = s;
    skey[o] = ((key >> db) << sb) | (uint64_t)(smax - (s < smax ? s : smax));
    sval[o] = o;
}

// sorted candidate i: qh[i] = 1 where its query differs from the candidate before
__global__ __launch_bounds__(256) void search_query_heads_kernel(const uint64_t *__restrict__ skey, uint64_t n, uint32_t sb, uint32_t *__restrict__ qh)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    qh[i] = (i == 0 || (skey[i - 1] >> sb) != (skey[i] >> sb)) ? 1u : 0u;
}

// tf[i] = 1 where sorted candidate i stands below max_cand in its query's run (qx: the exclusive scan of qh, qstart: the runs' starts)
__global__ __launch_bounds__(256) void search_top_flags_kernel(const uint32_t *__restrict__ qh, const uint32_t *__restrict__ qx,
                                                               const uint32_t *__restrict__ qstart, uint64_t n, uint32_t max_cand,
                                                               uint32_t *__restrict__ tf)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    tf[i] = (uint32_t)i - qstart[qx[i] + qh[i] - 1u] < max_cand ? 1u : 0u;
}

// kept candidate tx[i]: pairs = (n_db + q, d), the batch indices align_run takes; shared = s
__global__ __launch_bounds__(256) void search_top_emit_kernel(const uint32_t *__restrict__ sval, const uint64_t *__restrict__ ckey,
                                                              const uint32_t *__restrict__ cs, const uint32_t *__restrict__ tf,
                                                              const uint32_t *__restrict__ tx, uint64_t n, uint64_t n_kept, uint32_t db,
                                                              uint32_t n_db, int32_t *__restrict__ pairs, int32_t *__restrict__ shared)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !tf[i]) return;
    const uint32_t o = tx[i];
    if (o >= n_kept) return;
    const uint32_t c = sval[i];
    const uint64_t key = ckey[c];
    pairs[2 * (size_t)o] = (int32_t)(n_db + (uint32_t)(key >> db));
    pairs[2 * (size_t)o + 1] = (int32_t)(uint32_t)(key & ((1ull << db) - 1));
    shared[o] = (int32_t)cs[c];
}

// One wave per query q, one lane per candidate: candidates [hit_start[q], hit_start[q + 1]) of pairs / aln / shared, at most
// kSearchMaxCand.  The lane's rank is the number of the query's candidates that precede its own under (not-skipped first, larger
// score, larger s, smaller target): a shuffle sweep over the wave, no LDS and no atomic.  out: five int2 per record.
__global__ __launch_bounds__(256) void search_order_kernel(const int32_t *__restrict__ pairs, const AlignRec *__restrict__ aln,
                                                           const int32_t *__restrict__ shared, const int64_t *__restrict__ hit_start,
                                                           uint32_t n_q, int64_t min_ratio_pct, int ref_member, int2 *__restrict__ out,
                                                           unsigned long long *__restrict__ words)
{
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (256 / kWave) + (threadIdx.x >> 6)));
    if (q >= n_q) return;                               // (the whole wave)
    const int64_t first = hit_start[q];
    int c = __builtin_amdgcn_readfirstlane((int)(hit_start[q + 1] - first));
    c = c > kSearchMaxCand ? kSearchMaxCand : c;
    if (c <= 0) return;
    const bool have = lane < c;
    AlignRec a = {0, 0, 0, -1, -1, 0};
    int s = 0, d = 0;
    if (have) {
        a = aln[first + lane];
        s = shared[first + lane];
        d = pairs[2 * (size_t)(first + lane) + 1];
    }
    const bool skip = have && a.status != 0;
    const uint32_t hi = ((skip ? 1u : 0u) << 31) | (0x7FFFFFFFu - (uint32_t)(skip || a.score < 0 ? 0 : a.score));
    const unsigned long long lo = ((unsigned long long)(0xFFFFFFFFu - (uint32_t)s) << 32) | (unsigned long long)(uint32_t)d;
    int rank = 0;
    for (int k = 0; k < c; k++) {
        const uint32_t oh = (uint32_t)__shfl((int)hi, k);
        const unsigned long long ol = __shfl(lo, k);
        rank += (oh < hi || (oh == hi && ol < lo)) ? 1 : 0;
    }
    int status = 2;
    if (!skip) {
        const int64_t ref = ref_member ? (int64_t)a.self_a : (int64_t)(a.self_a > a.self_b ? a.self_a : a.self_b);
        status = (a.score >= 1 && 100 * (int64_t)a.score >= min_ratio_pct * ref) ? 0 : 1;
    }
    if (have && rank < c) {
        int2 *o = out + (size_t)(first + rank) * 5;
        o[0] = make_int2((int)q, d);
        o[1] = make_int2(s, a.score);
        o[2] = make_int2(a.self_a, a.self_b);
        o[3] = make_int2(a.end_a, a.end_b);
        o[4] = make_int2(status, rank);
    }
    const unsigned long long mh = __ballot(have && status == 0), mb = __ballot(have && status == 1), ms = __ballot(have && status == 2);
    const unsigned long long mq = __ballot(have && rank == 0 && status == 0);
    if (lane == 0) {
        if (mh) atomicAdd(&words[kSearchHits], (unsigned long long)__popcll(mh));
        if (mb) atomicAdd(&words[kSearchBelow], (unsigned long long)__popcll(mb));
        if (ms) atomicAdd(&words[kSearchSkipped], (unsigned long long)__popcll(ms));
        if (mq) atomicAdd(&words[kSearchQueriesHit], 1ull);
    }
}

}  // namespace kg
