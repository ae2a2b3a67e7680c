// kg_searchdb.hpp -- device side of kg_searchdb_* (include/kmerguts_hip.h states the rule): a search against a resident index of
// the targets.  The index holds what the one-batch search's front half leaves of the targets alone: the distinct (k-mer, target)
// pairs dpk[P] = v << bits(n_db) | d in sorted order with dpv beside them, the k-mer run starts dstart[K + 1] and the K distinct
// k-mers dk[K], ascending.  A call runs the same front half over its queries alone (qpk = v << bits(n_q) | q, qpv, the k-mer runs
// qstart) and then:
//
//   2r. searchdb_probe_kernel       per query k-mer run: a lower-bound search for its k-mer in dk.  Found at i: nd = the length of
//                                   database run i, nq = the query run's length, w = nd * nq in 64 bits where nd <= max_db_per_kmer,
//                                   else 0; the database run's first pair beside it.  The 64-bit sum of the weights, the found and
//                                   the joined k-mers are one integer atomic per wave each, as search_run_weights_kernel keeps them
//   3r. searchdb_run_compact_kernel search_run_compact_kernel with the two first pairs of a run, the targets' and the queries'
//   4r. searchdb_join_kernel / searchdb_join_diag_kernel
//                                   search_join_kernel / search_join_diag_kernel, item for item and key for key: the target of item
//                                   (t / nd, t % nd) is read from dpk / dpv, the query from qpk / qpv
//       searchdb_masked_kernel      the database runs longer than max_db_per_kmer (kmers_masked: whether or not a query has them)
//       searchdb_kmers_kernel       build and open: dk[r] = the k-mer of database run r
//
// The query k-mers with a target are in ascending order what the one-batch call's joined runs are, so wx, the items and the keys
// are the one-batch call's and everything behind the join runs on its kernels unchanged.
//
// What bounds a lane's work: the probe is one search per lane whose trip count, ceil(log2 K), depends on K alone, the same in
// every lane; consecutive lanes hold ascending k-mers, so the upper levels of a wave's searches read the same words.  The compact,
// masked and k-mer kernels are one item per lane.  The join kernels are the one-batch join's tile: kSearchTile / kSearchThreads
// items per lane, two per binary search over at most kSearchTile LDS words.  No lane walks a run.
// LDS of the join tile: wx and the two first pairs of a run, 3 * kSearchTile words = 24 576 B, the one-batch join's; a run's
// targets stay in device memory as in search_join_diag_kernel.
#pragma once

#include "kg_search.hpp"
#include "kg_ungapped.hpp"

namespace kg {

// the counter words of a probe (a block of its own, beside the search's)
enum : int { kSearchDbFound = 0, kSearchDbMasked = 1, kSearchDbWords = 2 };

// dk[r] = the k-mer of run r = pairs [dstart[r], dstart[r + 1])
__global__ __launch_bounds__(256) void searchdb_kmers_kernel(const uint64_t *__restrict__ dpk, const uint32_t *__restrict__ dstart, uint64_t n_runs,
                                                             uint32_t b, uint64_t *__restrict__ dk)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_runs) dk[r] = dpk[dstart[r]] >> b;
}

// words[kSearchDbMasked] += the runs of more than max_db pairs (one atomic per wave)
__global__ __launch_bounds__(256) void searchdb_masked_kernel(const uint32_t *__restrict__ dstart, uint64_t n_runs, uint32_t max_db,
                                                              unsigned long long *__restrict__ words)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool masked = r < n_runs && dstart[r + 1] - dstart[r] > max_db;
    const unsigned long long mk = __ballot(masked);
    if ((threadIdx.x & (kWave - 1)) == 0 && mk) atomicAdd(&words[kSearchDbMasked], (unsigned long long)__popcll(mk));
}

// the first i in [0, n] with dk[i] >= v (n: none).  The trip count depends on n alone.
__device__ __forceinline__ uint32_t searchdb_lower_bound(const uint64_t *__restrict__ dk, uint32_t n, uint64_t v)
{
    if (n == 0) return 0;
    uint32_t base = 0, len = n;
    while (len > 1) {
        const uint32_t half = len / 2;
        base += dk[base + half - 1] < v ? half : 0u;    // (base + half - 1 < base + len <= n)
        len -= half;
    }
    return base + (dk[base] < v ? 1u : 0u);
}

// query k-mer run r = pairs [qstart[r], qstart[r + 1]) of qpk: rd[r] = the first pair of the database run of the same k-mer,
// nd[r] = its length (0: no such run), w[r] = the weight (saturated), wf[r] = weight >= 1; words: the 64-bit sum of the weights
// and the joined k-mers (the search's words), dwords: the found k-mers
__global__ __launch_bounds__(256) void searchdb_probe_kernel(const uint64_t *__restrict__ qpk, const uint32_t *__restrict__ qstart,
                                                             uint64_t n_runs, uint32_t qb, const uint64_t *__restrict__ dk,
                                                             const uint32_t *__restrict__ dstart, uint32_t n_dk, uint32_t max_db,
                                                             uint32_t *__restrict__ rd, uint32_t *__restrict__ nd_out,
                                                             uint32_t *__restrict__ w, uint32_t *__restrict__ wf,
                                                             unsigned long long *__restrict__ words, unsigned long long *__restrict__ dwords)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long weight = 0;
    bool found = false;
    if (r < n_runs) {
        const uint32_t lo = qstart[r], nq = qstart[r + 1] - lo;
        const uint64_t v = qpk[lo] >> qb;
        const uint32_t i = searchdb_lower_bound(dk, n_dk, v);
        uint32_t first = 0, nd = 0;
        if (i < n_dk && dk[i] == v) {
            found = true;
            first = dstart[i];
            nd = dstart[i + 1] - first;
        }
        if (nd >= 1 && nd <= max_db && nq >= 1) weight = (unsigned long long)nd * nq;
        rd[r] = first;
        nd_out[r] = nd;
        w[r] = weight > kSearchSat ? kSearchSat : (uint32_t)weight;
        wf[r] = weight ? 1u : 0u;
    }
    const unsigned long long joined = __ballot(weight != 0), fd = __ballot(found);
    const unsigned long long sum = search_wave_sum(weight);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (sum) atomicAdd(&words[kSearchJoinPairs], sum);
        if (joined) atomicAdd(&words[kSearchJoined], (unsigned long long)__popcll(joined));
        if (fd) atomicAdd(&dwords[kSearchDbFound], (unsigned long long)__popcll(fd));
    }
}

// the runs with wf[r] to their places wpos[r] (the exclusive scan of wf): first target pair, first query pair, targets, weight
__global__ __launch_bounds__(256) void searchdb_run_compact_kernel(const uint32_t *__restrict__ rd, const uint32_t *__restrict__ qstart,
                                                                   const uint32_t *__restrict__ nd, const uint32_t *__restrict__ w,
                                                                   const uint32_t *__restrict__ wf, const uint32_t *__restrict__ wpos,
                                                                   uint64_t n_runs, uint64_t n_listed, uint32_t *__restrict__ cdstart,
                                                                   uint32_t *__restrict__ cqstart, uint32_t *__restrict__ cnd,
                                                                   uint32_t *__restrict__ cw)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs || !wf[r]) return;
    const uint32_t o = wpos[r];
    if (o >= n_listed) return;
    cdstart[o] = rd[r];
    cqstart[o] = qstart[r];
    cnd[o] = nd[r];
    cw[o] = w[r];
}

// search_join_kernel with two sources: listed run k has its targets at dpk[cdstart[k] ..) and its queries at qpk[cqstart[k] ..).
// keys[j] = q << db | d, vals[j] = 0.
__global__ __launch_bounds__(kSearchThreads) void searchdb_join_kernel(const uint64_t *__restrict__ dpk, const uint64_t *__restrict__ qpk,
                                                                       const uint32_t *__restrict__ wx, const uint32_t *__restrict__ cdstart,
                                                                       const uint32_t *__restrict__ cqstart, const uint32_t *__restrict__ cnd,
                                                                       uint32_t n_runs, uint32_t n_items, uint32_t db, uint32_t qb,
                                                                       uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    __shared__ uint32_t s_wx[kSearchTile], s_dstart[kSearchTile], s_qstart[kSearchTile];
    const uint32_t j0 = blockIdx.x * (uint32_t)kSearchTile;
    if (j0 >= n_items) return;
    const uint32_t j1 = n_items - j0 > (uint32_t)kSearchTile ? j0 + kSearchTile : n_items;
    // the same two searches in every lane: the tile's first and last run
    const uint32_t r0 = search_run_of(wx, n_runs, j0), r1 = search_run_of(wx, n_runs, j1 - 1);
    uint32_t nr = r1 - r0 + 1;
    nr = nr > (uint32_t)kSearchTile ? (uint32_t)kSearchTile : nr;      // (weights >= 1: it never is more)
    for (uint32_t k = threadIdx.x; k < nr; k += kSearchThreads) {
        s_wx[k] = wx[r0 + k];
        s_dstart[k] = cdstart[r0 + k];
        s_qstart[k] = cqstart[r0 + k];
    }
    __syncthreads();
    const uint64_t dmask = (1ull << db) - 1, qmask = (1ull << qb) - 1;
    for (uint32_t base = j0 + 2 * threadIdx.x; base < j1; base += 2 * kSearchThreads) {
        uint32_t k = search_run_of(s_wx, nr, base);
        uint64_t key[2] = {0, 0};
        const int cnt = j1 - base >= 2 ? 2 : 1;
        for (int i = 0; i < cnt; i++) {
            const uint32_t j = base + i;
            if (i && k + 1 < nr && s_wx[k + 1] <= j) k++;   // (the next item is in this run or in the next: weights >= 1)
            const uint32_t t = j - s_wx[k], nd = cnd[r0 + k];
            const uint32_t qi = t / nd, di = t - qi * nd;
            const uint32_t d = (uint32_t)(dpk[s_dstart[k] + di] & dmask), q = (uint32_t)(qpk[s_qstart[k] + qi] & qmask);
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

// search_join_diag_kernel with two sources: keys[j] = (q << db | d) << gb | (g + bias), vals[j] = 0.  off: the offsets of the
// targets and, behind them, of the call's queries (query q is protein n_db + q).
__global__ __launch_bounds__(kSearchThreads) void searchdb_join_diag_kernel(const uint64_t *__restrict__ dpk, const uint32_t *__restrict__ dpv,
                                                                            const uint64_t *__restrict__ qpk, const uint32_t *__restrict__ qpv,
                                                                            const int64_t *__restrict__ off, const uint32_t *__restrict__ wx,
                                                                            const uint32_t *__restrict__ cdstart,
                                                                            const uint32_t *__restrict__ cqstart, const uint32_t *__restrict__ cnd,
                                                                            uint32_t n_runs, uint32_t n_items, uint32_t n_db, uint32_t db,
                                                                            uint32_t qb, uint32_t gb, int32_t bias,
                                                                            uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    __shared__ uint32_t s_wx[kSearchTile], s_dstart[kSearchTile], s_qstart[kSearchTile];
    const uint32_t j0 = blockIdx.x * (uint32_t)kSearchTile;
    if (j0 >= n_items) return;
    const uint32_t j1 = n_items - j0 > (uint32_t)kSearchTile ? j0 + kSearchTile : n_items;
    const uint32_t r0 = search_run_of(wx, n_runs, j0), r1 = search_run_of(wx, n_runs, j1 - 1);
    uint32_t nr = r1 - r0 + 1;
    nr = nr > (uint32_t)kSearchTile ? (uint32_t)kSearchTile : nr;
    for (uint32_t k = threadIdx.x; k < nr; k += kSearchThreads) {
        s_wx[k] = wx[r0 + k];
        s_dstart[k] = cdstart[r0 + k];
        s_qstart[k] = cqstart[r0 + k];
    }
    __syncthreads();
    const uint64_t dmask = (1ull << db) - 1, qmask = (1ull << qb) - 1;
    for (uint32_t base = j0 + 2 * threadIdx.x; base < j1; base += 2 * kSearchThreads) {
        uint32_t k = search_run_of(s_wx, nr, base);
        uint64_t key[2] = {0, 0};
        const int cnt = j1 - base >= 2 ? 2 : 1;
        for (int i = 0; i < cnt; i++) {
            const uint32_t j = base + i;
            if (i && k + 1 < nr && s_wx[k + 1] <= j) k++;
            const uint32_t t = j - s_wx[k], nd = cnd[r0 + k];
            const uint32_t qi = t / nd, di = t - qi * nd;
            const uint32_t at_d = s_dstart[k] + di, at_q = s_qstart[k] + qi;
            const uint32_t pd = (uint32_t)(dpk[at_d] & dmask), q = (uint32_t)(qpk[at_q] & qmask), pq = n_db + q;
            const int32_t len_d = (int32_t)(off[pd + 1] - off[pd]), len_q = (int32_t)(off[pq + 1] - off[pq]);
            const int32_t g = (len_q - (int32_t)qpv[at_q]) - (len_d - (int32_t)dpv[at_d]);
            key[i] = (((((uint64_t)q) << db) | pd) << gb) | (uint64_t)(uint32_t)(g + bias);
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

}  // namespace kg
