// kg_regions.hpp -- device side of kg_result_regions / kg_regions_calls (include/kmerguts_hip.h): the CALL records of a DNA scan
// -> function regions in contig coordinates (the rule is stated in the header, next to the entry points).
//
//   1. region_keys_kernel      one lane per CALL: container -> (sequence, strand, frame), x0 / x1, validation (error words by
//                              atomicMin, firing only on bad input); key = x0, value = the CALL's index.
//   2. the stable LSD radix sort of kg_build.hpp by x0; region_group_keys_kernel then keys the items, in that order, by
//      (sequence * 2 + strand) : (fI ^ 2^31), and a second stable sort makes every group one run ordered by (x0, index).
//   3. region_gather_kernel    the CALLs' fields in group order (so that everything below streams) and the group-head flags;
//                              their prefix sum numbers the groups.
//   4. one inclusive prefix maximum over (group << 32) | x1 -- the group number ascends, so the plain maximum is the segmented
//      one: region_tile_max_kernel, the build's build_tile_scan_kernel over the tile maxima, and region_heads_kernel, which
//      applies it: a CALL opens a region iff it is a group head or x0 - (maximum in front of it) - 1 > merge_gap.
//   5. prefix sum of the region heads = region numbers; region_walk_kernel: each region head's lane walks its own run in group
//      order (weighted must be summed in that order), loading kRegionWalk items ahead, and writes the region's record and its
//      two sort keys.  Only a region's own length is serial.
//   6. two stable sorts of the region numbers, by (right, strand, fI) and then by (sequence, left), give the output order;
//      region_emit_kernel copies the records into it and counts the kept and the multi-frame ones (one atomic per wave),
//      region_seq_start_kernel finds every contig's first region by a binary search over the sorted keys.
//
// The only returning atomics are atomicMin on the error words, and they run only for bad input.
#pragma once

#include "kg_build.hpp"
#include "kg_device.hpp"

namespace kg {

constexpr int kRegionWalk = 16;         // items a region walk loads ahead
constexpr unsigned long long kRegionNoErr = 0x7F7F7F7F7F7F7F7Full;   // the error words' "none" (a byte memset)

// error words: the first CALL (index in calls[]) [0] whose container is 6 * n_seqs or more, [1] whose container is below its
// predecessor's, [2] with a negative count, [3] outside its contig; [4] the smallest first_call of a region whose score or
// CALL count is 2^31 or more
enum { kRegionErrContainer = 0, kRegionErrOrder = 1, kRegionErrCount = 2, kRegionErrRange = 3, kRegionErrLimit = 4, kRegionErrWords = 5 };
// counter words: [0] kept regions, [1] regions with more than one frame bit
enum { kRegionCntKept = 0, kRegionCntMulti = 1 };

struct RegionSpan {
    uint32_t seq, strand, frame;        // clamped: seq < n_seqs
    uint32_t x0, x1;                    // clamped: x0 <= x1 < max(L, 1)
    int64_t L;
    bool ok;                            // the record as given lies inside its contig
};

// rule 1.  A bad record is clamped, so that nothing derived from it leaves its arrays (the call fails with KG_ERR_ARG anyway).
__device__ inline RegionSpan region_span(const kg_call &c, const int64_t *__restrict__ offsets, uint64_t n_seqs)
{
    RegionSpan r;
    const uint64_t n_cont = 6 * n_seqs;
    const uint64_t cont = c.container < n_cont ? c.container : n_cont - 1;
    r.seq = (uint32_t)(cont / 6);
    const uint32_t k = (uint32_t)(cont % 6);
    r.strand = k >= 3 ? 1u : 0u;
    r.frame = k % 3;
    r.L = offsets[r.seq + 1] - offsets[r.seq];
    const int64_t x0 = (int64_t)r.frame + 3 * (int64_t)c.start, x1 = (int64_t)r.frame + 3 * (int64_t)c.end + 2;
    r.ok = x0 >= 0 && x0 <= x1 && x1 <= r.L - 1;
    const int64_t top = r.L > 0 ? r.L - 1 : 0;
    const int64_t a = x0 < 0 ? 0 : (x0 > top ? top : x0);
    const int64_t b = x1 < a ? a : (x1 > top ? top : x1);
    r.x0 = (uint32_t)a;
    r.x1 = (uint32_t)b;
    return r;
}

__global__ __launch_bounds__(256) void region_keys_kernel(const kg_call *__restrict__ calls, uint64_t n,
                                                          const int64_t *__restrict__ offsets, uint64_t n_seqs,
                                                          uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                          unsigned long long *err)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const kg_call c = calls[i];
    if ((uint64_t)c.container >= 6 * n_seqs) atomicMin(&err[kRegionErrContainer], (unsigned long long)i);
    if (i > 0 && calls[i - 1].container > c.container) atomicMin(&err[kRegionErrOrder], (unsigned long long)i);
    if (c.count < 0) atomicMin(&err[kRegionErrCount], (unsigned long long)i);
    const RegionSpan r = region_span(c, offsets, n_seqs);
    if (!r.ok) atomicMin(&err[kRegionErrRange], (unsigned long long)i);
    keys[i] = r.x0;
    vals[i] = (uint32_t)i;
}

// the items in x0 order -> their group keys, in that order
__global__ __launch_bounds__(256) void region_group_keys_kernel(const kg_call *__restrict__ calls, uint64_t n, uint64_t n_seqs,
                                                                const uint32_t *__restrict__ vals, uint64_t *__restrict__ keys)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t v = vals[j];
    const uint64_t i = v < n ? v : n - 1;
    const uint64_t n_cont = 6 * n_seqs;
    const uint64_t cont = calls[i].container < n_cont ? calls[i].container : n_cont - 1;
    const uint64_t hi = (cont / 6) * 2 + (cont % 6 >= 3 ? 1 : 0);
    keys[j] = (hi << 32) | (uint64_t)((uint32_t)calls[i].fI ^ 0x80000000u);
}

// group order: the fields the later kernels stream over, and the group heads
__global__ __launch_bounds__(256) void region_gather_kernel(const kg_call *__restrict__ calls, uint64_t n,
                                                            const int64_t *__restrict__ offsets, uint64_t n_seqs,
                                                            const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                            uint32_t *__restrict__ sx0, uint32_t *__restrict__ sx1,
                                                            int32_t *__restrict__ scount, float *__restrict__ sweight,
                                                            uint8_t *__restrict__ sframe, uint32_t *__restrict__ ghead)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t v = vals[j];
    const kg_call c = calls[v < n ? v : n - 1];
    const RegionSpan r = region_span(c, offsets, n_seqs);
    sx0[j] = r.x0;
    sx1[j] = r.x1;
    scount[j] = c.count < 0 ? 0 : c.count;
    sweight[j] = c.weightedHits;
    sframe[j] = (uint8_t)r.frame;
    ghead[j] = (j == 0 || keys[j - 1] != keys[j]) ? 1u : 0u;
}

// (group << 32) | x1 as a signed value whose order is the unsigned one; INT64_MIN, the scans' identity, is group 0 / x1 0
__device__ inline int64_t region_value(uint32_t group, uint32_t x1)
{
    return (int64_t)((((uint64_t)group << 32) | x1) ^ 0x8000000000000000ull);
}

// tile_max[tile] = max over the tile's items of region_value(group, x1); group = (heads in front) + (own head) - 1
__global__ __launch_bounds__(kBuildThreads) void region_tile_max_kernel(const uint32_t *__restrict__ ghead,
                                                                        const uint32_t *__restrict__ gexcl,
                                                                        const uint32_t *__restrict__ sx1, uint64_t n,
                                                                        int64_t *__restrict__ tile_max)
{
    __shared__ int64_t wmax[kBuildThreads / kWave];
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile;
    int64_t m = INT64_MIN;
    for (int k = 0; k < kBuildItems; k++) {
        const uint64_t i = base + (uint64_t)k * kBuildThreads + threadIdx.x;
        if (i >= n) break;
        const int64_t a = region_value(gexcl[i] + ghead[i] - 1, sx1[i]);
        m = a > m ? a : m;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t y = __shfl_down(m, off);
        m = y > m ? y : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBuildThreads / kWave; w++) m = wmax[w] > m ? wmax[w] : m;
        tile_max[blockIdx.x] = m;
    }
}

// Thread t of a tile takes items [tile * 4096 + t * 16, + 16), as build_place_kernel does: `run` = the maximum over everything
// in front of the item.  rhead[i] = the item opens a region; rmax[i] = the largest x1 of its group up to and including it.
__global__ __launch_bounds__(kBuildThreads) void region_heads_kernel(const uint32_t *__restrict__ ghead,
                                                                     const uint32_t *__restrict__ gexcl,
                                                                     const uint32_t *__restrict__ sx0,
                                                                     const uint32_t *__restrict__ sx1, uint64_t n,
                                                                     const int64_t *__restrict__ tile_pre, int64_t merge_gap,
                                                                     uint32_t *__restrict__ rhead, uint32_t *__restrict__ rmax)
{
    __shared__ int64_t wmax[kBuildThreads / kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile + (uint64_t)threadIdx.x * kBuildItems;
    int64_t a[kBuildItems];
    uint32_t head[kBuildItems], x0[kBuildItems];
    int64_t m = INT64_MIN;
#pragma unroll
    for (int k = 0; k < kBuildItems; k++) {
        const uint64_t i = base + k;
        a[k] = INT64_MIN;
        head[k] = 0;
        x0[k] = 0;
        if (i < n) {
            head[k] = ghead[i];
            x0[k] = sx0[i];
            a[k] = region_value(gexcl[i] + head[k] - 1, sx1[i]);
        }
        m = a[k] > m ? a[k] : m;
    }
    int64_t incl = m;
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t y = __shfl_up(incl, off);
        if (lane >= off) incl = y > incl ? y : incl;
    }
    int64_t run = __shfl_up(incl, 1);
    if (lane == 0) run = INT64_MIN;
    if (lane == 63) wmax[wave] = incl;
    __syncthreads();
    const int64_t tp = tile_pre[blockIdx.x];
    run = tp > run ? tp : run;
    for (int w = 0; w < wave; w++) run = wmax[w] > run ? wmax[w] : run;
#pragma unroll
    for (int k = 0; k < kBuildItems; k++) {
        const uint64_t i = base + k;
        if (i >= n) break;
        // not a group head: the item in front is of the same group, so `run` carries this group's number and its largest x1
        const int64_t R = (int64_t)(uint32_t)(uint64_t)run;
        rhead[i] = (head[k] || (int64_t)x0[k] - R - 1 > merge_gap) ? 1u : 0u;
        run = a[k] > run ? a[k] : run;
        rmax[i] = (uint32_t)(uint64_t)run;
    }
}

struct RegionKeys {
    uint64_t *k1;                       // (right << 33) | (strand << 32) | (fI ^ 2^31)
    uint64_t *k2;                       // (seq << left_bits) | left
    uint32_t *val;                      // the region's number in group order
};

// One lane per region head: walks its run in group order and writes the region's record (rule 4) and sort keys.
__global__ __launch_bounds__(256) void region_walk_kernel(const uint32_t *__restrict__ rhead, const uint32_t *__restrict__ rexcl,
                                                          const uint32_t *__restrict__ rmax, const uint32_t *__restrict__ sx0,
                                                          const int32_t *__restrict__ scount, const float *__restrict__ sweight,
                                                          const uint8_t *__restrict__ sframe, const uint64_t *__restrict__ gkeys,
                                                          const uint32_t *__restrict__ vals, uint64_t n,
                                                          const int64_t *__restrict__ offsets, int32_t min_score, int32_t min_len,
                                                          uint32_t left_bits, kg_region *__restrict__ out, RegionKeys rk,
                                                          unsigned long long *err)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !rhead[j]) return;
    int64_t score = 0;
    float w = 0.0f;
    uint64_t cnt = 0, last = j;
    uint32_t frames = 0;
    int32_t best_count = -1, best_frame = 0;
    bool more = true;
    for (uint64_t b = j; more && b < n; b += kRegionWalk) {
        uint32_t hh[kRegionWalk];
        int32_t cc[kRegionWalk];
        float ww[kRegionWalk];
        uint8_t ff[kRegionWalk];
#pragma unroll
        for (int u = 0; u < kRegionWalk; u++) {
            const uint64_t q = b + u;
            const bool in = q < n;
            hh[u] = in ? rhead[q] : 1u;
            cc[u] = in ? scount[q] : 0;
            ww[u] = in ? sweight[q] : 0.0f;
            ff[u] = in ? sframe[q] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < kRegionWalk; u++) {
            if (!more) continue;
            if (hh[u] && b + u != j) {  // the next region's head (or the end of the list)
                more = false;
                continue;
            }
            score += cc[u];
            w = __fadd_rn(w, ww[u]);
            frames |= 1u << ff[u];
            if (cc[u] > best_count) { best_count = cc[u]; best_frame = ff[u]; }
            cnt++;
            last = b + u;
        }
    }
    const uint64_t key = gkeys[j];
    const uint32_t hi = (uint32_t)(key >> 32), seq = hi >> 1, strand = hi & 1u;
    const uint32_t fix = (uint32_t)key;
    const int64_t L = offsets[seq + 1] - offsets[seq];
    const uint32_t xa = sx0[j], R = rmax[last];
    // x0 <= R < max(L, 1) after the clamp, so neither difference is negative for L >= 1
    const uint32_t left = strand ? (uint32_t)(L > 0 ? L - 1 - R : 0) : xa;
    const uint32_t right = strand ? (uint32_t)(L > 0 ? L - 1 - xa : 0) : R;
    const uint32_t first = vals[j];
    if (score >= (1ll << 31) || cnt >= (1ull << 31)) atomicMin(&err[kRegionErrLimit], (unsigned long long)first);
    kg_region r;
    r.seq = (int32_t)seq;
    r.strand = (int32_t)strand;
    r.left = (int32_t)left;
    r.right = (int32_t)right;
    r.fI = (int32_t)(fix ^ 0x80000000u);
    r.score = (int32_t)score;
    r.weighted = w;
    r.n_calls = (int32_t)cnt;
    r.frames = frames;
    r.best_frame = best_frame;
    r.first_call = first;
    r.kept = (score >= (int64_t)min_score && (int64_t)right - (int64_t)left + 1 >= (int64_t)min_len) ? 1 : 0;
    const uint32_t ri = rexcl[j];
    out[ri] = r;
    rk.k1[ri] = ((uint64_t)right << 33) | ((uint64_t)strand << 32) | fix;
    rk.k2[ri] = ((uint64_t)seq << left_bits) | left;
    rk.val[ri] = ri;
}

// the second sort's keys, in the order the first sort left the regions in
__global__ __launch_bounds__(256) void region_rekey_kernel(const uint64_t *__restrict__ k2, const uint32_t *__restrict__ vals,
                                                           uint64_t n, uint64_t *__restrict__ keys)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t v = vals[k];
    keys[k] = k2[v < n ? v : n - 1];
}

// output order; cnt[kRegionCnt*] by one atomic per wave
__global__ __launch_bounds__(256) void region_emit_kernel(const kg_region *__restrict__ in, const uint32_t *__restrict__ vals,
                                                          uint64_t n, kg_region *__restrict__ out, unsigned long long *cnt)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t kept = 0, multi = 0;
    if (k < n) {
        const uint32_t v = vals[k];
        const kg_region r = in[v < n ? v : n - 1];
        out[k] = r;
        kept = r.kept ? 1u : 0u;
        multi = (r.frames & (r.frames - 1)) ? 1u : 0u;
    }
    const uint32_t nk = (uint32_t)__popcll(__ballot(kept)), nm = (uint32_t)__popcll(__ballot(multi));
    if ((threadIdx.x & 63) == 0) {
        if (nk) atomicAdd(&cnt[kRegionCntKept], (unsigned long long)nk);
        if (nm) atomicAdd(&cnt[kRegionCntMulti], (unsigned long long)nm);
    }
}

// seq_start[s] = the first region (output order) of a contig >= s, for s in [0, n_seqs]: a binary search over the sorted keys
__global__ __launch_bounds__(256) void region_seq_start_kernel(const uint64_t *__restrict__ keys, uint64_t n_regions,
                                                               uint32_t left_bits, uint64_t n_seqs, int64_t *__restrict__ seq_start)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_seqs) return;
    uint64_t lo = 0, hi = n_regions;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((keys[mid] >> left_bits) < s) lo = mid + 1;
        else hi = mid;
    }
    seq_start[s] = (int64_t)lo;
}

}  // namespace kg
