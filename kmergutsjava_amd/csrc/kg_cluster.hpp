// kg_cluster.hpp -- device side of kg_proteins_cluster / kg_proteins_cluster_device (include/kmerguts_hip.h): proteins ->
// families by shared 8-mers (the rule is stated in the header, next to the entry points).  Integers only.
//
// The front half is the derive call's (kg_derive.hpp): derive_windows_kernel encodes and emits every valid window as
//     key = v * 2^b + p          (b = ceil(log2 n_prot) <= 29, v < 20^8 < 2^35; rank_of is the identity here)
// the radix sort of kg_build.hpp orders the keys and derive_collapse_kernel leaves the distinct (k-mer, protein) pairs.  Behind it:
//
//   1. cluster_pair_kernel      per pair: the k-mer run head flag, and d_p += 1 (one integer atomic per pair)
//   2. cluster_centre_kernel    per k-mer run: the maximum of (len_p << 32 | ~p) = the longest member, on a tie the smallest index
//   3. cluster_link_flags_kernel / cluster_link_emit_kernel
//                               every pair whose protein is not its run's centre -> one key (m << 32 | c), compacted by a prefix sum
//   4. the radix sort again, derive_key_heads_kernel and a prefix sum: runs of equal keys = distinct links, run length = s(m, c)
//   5. cluster_link_starts_kernel, cluster_edge_kernel
//                               per distinct link: the two tests; an edge keeps its key, and best / shared of the member is an
//                               atomicMax of (s << 32 | ~c)
//   6. cluster_hook_kernel / cluster_jump_kernel, once per round while the device flag says something changed:
//                               hook the larger root under the smaller (atomicMin on the larger root's parent), then
//                               parent[i] = parent[parent[i]].  parent[i] <= i always holds, so a tree's root is its smallest
//                               member and the fixed point does not depend on scheduling.
//   7. cluster_compress_kernel  root[i] = the end of i's parent chain, size[root] += 1
//      cluster_root_flags_kernel + prefix sum: the roots numbered in ascending order
//      cluster_emit_kernel      the 16-byte records and the family counts
//
// A run is never given to one lane: step 2 takes 16 consecutive pairs per lane and meets at run borders through plain stores (a
// run wholly inside the lane's pairs) or atomicMax (a run that crosses a border), steps 3 and 5 are one item per lane, and the
// run length of step 5 is a difference of two run starts.  The only loops whose length the data decide are the parent walks of
// steps 6 and 7: a walk is as long as the node's depth in its tree, and every round's jump halves the depths.
#pragma once

#include "kg_device.hpp"
#include "kg_derive.hpp"

namespace kg {

constexpr uint64_t kClusterNoEdge = ~0ull;          // a distinct link that failed a test
// the counter words of a call
enum : int { kClusterEdges = 0, kClusterMulti = 1, kClusterLargest = 2, kClusterChanged = 3, kClusterWords = 4 };

// rank_of[p] = p (the derive emit kernel ranks proteins; here the index is the rank), parent[p] = p, and the per-protein words cleared
__global__ __launch_bounds__(256) void cluster_init_kernel(uint32_t n, uint32_t *__restrict__ rank_of, uint32_t *__restrict__ parent,
                                                           uint32_t *__restrict__ d_cnt, uint32_t *__restrict__ size,
                                                           unsigned long long *__restrict__ best)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rank_of[i] = i;
    parent[i] = i;
    d_cnt[i] = 0;
    size[i] = 0;
    best[i] = 0;
}

// pair j = (k-mer, protein) in sorted order: kh[j] = 1 where its k-mer differs from the pair before; d_cnt[p] += 1
__global__ __launch_bounds__(256) void cluster_pair_kernel(const uint64_t *__restrict__ pk, uint64_t n, uint32_t b, uint32_t n_prot,
                                                           uint32_t *__restrict__ kh, uint32_t *__restrict__ d_cnt)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t k = pk[j];
    kh[j] = (j == 0 || (pk[j - 1] >> b) != (k >> b)) ? 1u : 0u;
    const uint32_t p = (uint32_t)(k & ((1ull << b) - 1));
    if (p < n_prot) atomicAdd(&d_cnt[p], 1u);
}

__device__ __forceinline__ unsigned long long cluster_rank(const uint64_t *__restrict__ pk, uint64_t j, uint32_t b, uint32_t n_prot,
                                                          const int64_t *__restrict__ off)
{
    uint32_t p = (uint32_t)(pk[j] & ((1ull << b) - 1));
    p = p < n_prot ? p : n_prot - 1;
    return ((unsigned long long)(uint32_t)(off[p + 1] - off[p]) << 32) | (unsigned long long)(0xFFFFFFFFu - p);
}

// kbest[k-mer run] = max over its pairs of (len_p << 32 | ~p) (kbest zeroed beforehand; len_p >= 9); kx = the exclusive scan of
// kh.  Thread t takes pairs [16 t, 16 t + 16).
__global__ __launch_bounds__(256) void cluster_centre_kernel(const uint64_t *__restrict__ pk, uint64_t n, uint32_t b, uint32_t n_prot,
                                                             const int64_t *__restrict__ off, const uint32_t *__restrict__ kh,
                                                             const uint32_t *__restrict__ kx, unsigned long long *__restrict__ kbest)
{
    const uint64_t base = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kDeriveChunk;
    if (base >= n) return;
    const uint64_t end = base + kDeriveChunk < n ? base + kDeriveChunk : n;
    bool head = kh[base] != 0;
    uint32_t r = kx[base] + (head ? 1u : 0u) - 1u;
    unsigned long long m = cluster_rank(pk, base, b, n_prot, off);
    for (uint64_t j = base + 1; j < end; j++) {
        const unsigned long long v = cluster_rank(pk, j, b, n_prot, off);
        if (kh[j]) {
            if (head) kbest[r] = m; else atomicMax(&kbest[r], m);
            head = true; r++; m = v;
        } else {
            m = v > m ? v : m;
        }
    }
    if (head && (end == n || kh[end])) kbest[r] = m;
    else atomicMax(&kbest[r], m);
}

// lf[j] = 1 where pair j's protein is not the centre of its k-mer run: the pair gives a link
__global__ __launch_bounds__(256) void cluster_link_flags_kernel(const uint64_t *__restrict__ pk, uint64_t n, uint32_t b,
                                                                 const uint32_t *__restrict__ kh, const uint32_t *__restrict__ kx,
                                                                 const unsigned long long *__restrict__ kbest, uint32_t *__restrict__ lf)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t p = (uint32_t)(pk[j] & ((1ull << b) - 1));
    const uint32_t c = 0xFFFFFFFFu - (uint32_t)kbest[kx[j] + kh[j] - 1u];
    lf[j] = p != c ? 1u : 0u;
}

// keys[lx[j]] = m << 32 | c for every pair with lf[j] (lx = the exclusive scan of lf)
__global__ __launch_bounds__(256) void cluster_link_emit_kernel(const uint64_t *__restrict__ pk, uint64_t n, uint32_t b,
                                                                const uint32_t *__restrict__ kh, const uint32_t *__restrict__ kx,
                                                                const unsigned long long *__restrict__ kbest, const uint32_t *__restrict__ lf,
                                                                const uint32_t *__restrict__ lx, uint64_t n_links, uint64_t *__restrict__ keys,
                                                                uint32_t *__restrict__ vals)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !lf[j]) return;
    const uint32_t o = lx[j];
    if (o >= n_links) return;
    const uint32_t p = (uint32_t)(pk[j] & ((1ull << b) - 1));
    const uint32_t c = 0xFFFFFFFFu - (uint32_t)kbest[kx[j] + kh[j] - 1u];
    keys[o] = ((uint64_t)p << 32) | c;
    vals[o] = 0;
}

// lstart[run] = the first item of every run of equal link keys, lstart[*n_runs] = n (lh = the heads, lr = their exclusive scan)
__global__ __launch_bounds__(256) void cluster_link_starts_kernel(const uint32_t *__restrict__ lh, const uint32_t *__restrict__ lr, uint64_t n,
                                                                  const uint64_t *__restrict__ n_runs, uint32_t *__restrict__ lstart)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) lstart[*n_runs] = (uint32_t)n;
    if (j >= n) return;
    if (lh[j]) lstart[lr[j]] = (uint32_t)j;
}

// Distinct link r = (m, c) with s = its run length.  An edge iff s >= min_shared and 100 s >= min_cover_pct d_m (int64):
// edge[r] = its key, else kClusterNoEdge; best[m] = max of (s << 32 | ~c) over m's edges; words[kClusterEdges] counts them (one
// atomic per wave).
__global__ __launch_bounds__(256) void cluster_edge_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ lstart, uint64_t n_runs,
                                                           uint32_t n_prot, const uint32_t *__restrict__ d_cnt, int64_t min_shared,
                                                           int64_t min_cover_pct, uint64_t *__restrict__ edge,
                                                           unsigned long long *__restrict__ best, unsigned long long *__restrict__ words)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool pass = false;
    if (r < n_runs) {
        const uint32_t first = lstart[r];
        const uint64_t key = keys[first];
        const int64_t s = (int64_t)(lstart[r + 1] - first);
        const uint32_t m = (uint32_t)(key >> 32), c = (uint32_t)key;
        if (m < n_prot && c < n_prot) {
            pass = s >= min_shared && 100 * s >= min_cover_pct * (int64_t)d_cnt[m];
            if (pass) atomicMax(&best[m], ((unsigned long long)s << 32) | (unsigned long long)(0xFFFFFFFFu - c));
        }
        edge[r] = pass ? key : kClusterNoEdge;
    }
    const unsigned long long mask = __ballot(pass);
    if ((threadIdx.x & (kWave - 1)) == 0 && mask) atomicAdd(&words[kClusterEdges], (unsigned long long)__popcll(mask));
}

// the end of x's parent chain (parent[i] <= i: the walk descends and ends at a node that is its own parent)
__device__ __forceinline__ uint32_t cluster_find(const uint32_t *parent, uint32_t x)
{
    for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
    return x;
}

// per edge: the roots of its two ends; where they differ the larger root goes under the smaller and the flag is raised.  A
// root that another lane hooks first keeps the smaller parent (atomicMin): the edge is then looked at again next round.
__global__ __launch_bounds__(256) void cluster_hook_kernel(const uint64_t *__restrict__ edge, uint64_t n_runs, uint32_t *parent,
                                                           unsigned long long *__restrict__ words)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    const uint64_t e = edge[r];
    if (e == kClusterNoEdge) return;
    const uint32_t ru = cluster_find(parent, (uint32_t)(e >> 32)), rv = cluster_find(parent, (uint32_t)e);
    if (ru == rv) return;
    atomicMin(&parent[ru > rv ? ru : rv], ru > rv ? rv : ru);
    words[kClusterChanged] = 1;
}

// pointer jumping: parent[i] = parent[parent[i]]; the flag is raised where that changed something
__global__ __launch_bounds__(256) void cluster_jump_kernel(uint32_t n, uint32_t *parent, unsigned long long *__restrict__ words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = parent[i], g = parent[p];
    if (g != p) {
        parent[i] = g;
        words[kClusterChanged] = 1;
    }
}

// the full compress behind the last round: root[i], size[root[i]] += 1, flag[i] = 1 for a root
__global__ __launch_bounds__(256) void cluster_compress_kernel(uint32_t n, const uint32_t *__restrict__ parent, uint32_t *__restrict__ root,
                                                               uint32_t *__restrict__ size, uint32_t *__restrict__ flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = cluster_find(parent, i);
    root[i] = r;
    flag[i] = r == i ? 1u : 0u;
    atomicAdd(&size[r], 1u);
}

// out[i] = { family = the number of its root (fx = the exclusive scan of the root flags), root, best, shared }; the roots count
// the families of two or more members (one atomic per wave) and find the largest
__global__ __launch_bounds__(256) void cluster_emit_kernel(uint32_t n, const uint32_t *__restrict__ root, const uint32_t *__restrict__ fx,
                                                           const uint32_t *__restrict__ size, const unsigned long long *__restrict__ best,
                                                           int4 *__restrict__ out, unsigned long long *__restrict__ words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t sz = 0;                                    // a root's family size, 0 for every other lane
    if (i < n) {
        const uint32_t r = root[i];
        const unsigned long long bv = best[i];
        out[i] = make_int4((int)fx[r], (int)r, bv ? (int)(0xFFFFFFFFu - (uint32_t)bv) : -1, (int)(bv >> 32));
        if (r == i) sz = size[i];
    }
    const unsigned long long mask = __ballot(sz >= 2);
    uint32_t big = sz;
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)big, d);
        big = o > big ? o : big;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (mask) atomicAdd(&words[kClusterMulti], (unsigned long long)__popcll(mask));
        if (big) atomicMax(&words[kClusterLargest], (unsigned long long)big);
    }
}

}  // namespace kg
