// kg_merge.hpp -- device side of kg_table_merge_signatures / kg_table_merge_signatures_device (include/kmerguts_hip.h states
// the rule): the records of a resident table united with a list of new signatures, one record per k-mer, in k-mer order.
//
//   1. merge_extract_kernel   one pass over the resident records in tiles of kBuildTile: every record of B (0 <= kmer < 20^8)
//                             becomes the pair (kmer << 1 | 0, slot), compacted in slot order -- ballot ranks inside the wave,
//                             the 64 (step, wave) counts of the tile scanned in LDS, ONE global atomic per tile for the tile's
//                             place in the list; the same pass counts the records the lookup can never find (base_ignored)
//   2. merge_new_keys_kernel  (kmer << 1 | 1, input index) for the new signatures, with the range checks of the k-mer and of
//                             the two map indices by atomicMin, as build_keys_kernel does
//   3. SortPairs::sort        the build's LSD radix sort over the |B| + n pairs, 36 key bits (35 of the k-mer, 1 of the source)
//   4. merge_resolve_kernel   one pair per lane, looking at its two neighbours only: equal keys are a k-mer twice in one
//                             source (atomicMin per source); a base pair followed by the new pair of the same k-mer is a
//                             conflict, wherever a wave or tile border falls; the survivor flag follows the policy
//   5. prefix_sum of the flags, then merge_emit_kernel: 24 bytes gathered from the table by slot or from the input by index
//      (the maps applied) to the record's rank
// No lane is given a k-mer, a run or a slot range: the extract lanes take kBuildItems fixed records, every other lane one pair.
// The 24 record bytes move as three 8-byte words and are never read as anything but integers.
#pragma once

#include "kg_build.hpp"

namespace kg {

constexpr uint32_t kMergeKeyBits = 36;                  // (20^8 - 1) << 1 | 1 < 2^36
// d_cnt words of one merge call
enum : int { kMrgBadKmer = 0, kMrgBadFn = 1, kMrgBadOtu = 2, kMrgDupNew = 3, kMrgDupBase = 4 /* ~0: none */,
             kMrgCursor = 5 /* |B| */, kMrgIgnored = 6, kMrgOverflow = 7 /* more records of B than the table counted when opened */,
             kMrgConflicts = 8, kMrgSame = 9, kMrgAdded = 10, kMrgWords = 12, kMrgErrWords = 5 };

// Item k of thread t of a tile is record tile * 4096 + k * 256 + t, so that a wave reads 64 consecutive records per step.  The
// pairs of a tile go to keys / vals[at + base ..) in record order: (step, wave, lane).
__global__ __launch_bounds__(kBuildThreads) void merge_extract_kernel(const uint8_t *__restrict__ entries, uint64_t records, uint64_t at,
                                                                      uint64_t cap, uint64_t *__restrict__ keys,
                                                                      uint32_t *__restrict__ vals, unsigned long long *cnt)
{
    constexpr int kWaves = kBuildThreads / kWave;
    __shared__ uint32_t pre[kBuildItems * kWaves];
    __shared__ unsigned long long tile_base;
    __shared__ uint32_t tile_total;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t first = (uint64_t)blockIdx.x * kBuildTile + threadIdx.x;
    int64_t kmer[kBuildItems];
    uint32_t ignored = 0;
#pragma unroll
    for (int k = 0; k < kBuildItems; k++) {
        const uint64_t j = first + (uint64_t)k * kBuildThreads;
        kmer[k] = j < records ? build_load_kmer(entries, j) : (int64_t)kEmptyKey;
        ignored += kmer[k] < 0 || kmer[k] == KG_MAX_ENCODED;
        const uint64_t in = __ballot(kmer[k] >= 0 && kmer[k] < KG_MAX_ENCODED);
        if (lane == 0) pre[k * kWaves + wave] = (uint32_t)__popcll(in);
    }
    __syncthreads();
    if (wave == 0) {                                    // exclusive scan of the 64 counts, then the tile's place in the list
        const uint32_t x = pre[lane];
        uint32_t incl = x;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(incl, off);
            if (lane >= off) incl += y;
        }
        pre[lane] = incl - x;
        if (lane == 63) {
            tile_total = incl;
            tile_base = incl ? atomicAdd(cnt + kMrgCursor, (unsigned long long)incl) : 0ull;
        }
    }
    for (int off = 32; off > 0; off >>= 1) ignored += __shfl_down(ignored, off);
    if (lane == 0 && ignored) atomicAdd(cnt + kMrgIgnored, (unsigned long long)ignored);
    __syncthreads();
    const uint64_t base = tile_base;
    if (base + tile_total > cap) {                      // never with a table that is unchanged since it was opened
        if (threadIdx.x == 0) cnt[kMrgOverflow] = 1;
        return;
    }
    const uint64_t lt = (1ull << lane) - 1;
#pragma unroll
    for (int k = 0; k < kBuildItems; k++) {
        const bool mine = kmer[k] >= 0 && kmer[k] < KG_MAX_ENCODED;
        const uint64_t in = __ballot(mine);
        if (mine) {
            const uint64_t o = at + base + pre[k * kWaves + wave] + (uint32_t)__popcll(in & lt);
            keys[o] = (uint64_t)kmer[k] << 1;
            vals[o] = (uint32_t)(first + (uint64_t)k * kBuildThreads);
        }
    }
}

// keys[i] = kmer << 1 | 1, vals[i] = i; cnt[kMrgBadKmer / BadFn / BadOtu] = the smallest input index whose k-mer lies outside
// [0, 20^8) / whose function_index lies outside [0, n_fn) with a function map / the same for otu_index (each stays ~0 when none)
__global__ __launch_bounds__(kBuildThreads) void merge_new_keys_kernel(const uint8_t *__restrict__ sigs, uint64_t n, int has_fn,
                                                                       uint64_t n_fn, int has_otu, uint64_t n_otu,
                                                                       uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                                       unsigned long long *cnt)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad_kmer = ~0ull, bad_fn = ~0ull, bad_otu = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t kmer = build_load_kmer(sigs, i);
        const uint2 b = *reinterpret_cast<const uint2 *>(sigs + i * 24 + 8);        // otu_index, avg_from_end
        const uint2 c = *reinterpret_cast<const uint2 *>(sigs + i * 24 + 16);       // function_index, the weight's bits
        uint64_t key = 1;
        if (kmer < 0 || kmer >= KG_MAX_ENCODED) {
            if (bad_kmer == ~0ull) bad_kmer = i;
        } else {
            key = (uint64_t)kmer << 1 | 1;
        }
        if (has_fn && (uint64_t)(int64_t)(int32_t)c.x >= n_fn && bad_fn == ~0ull) bad_fn = i;     // (a negative index wraps above n_fn)
        if (has_otu && (uint64_t)(int64_t)(int32_t)b.x >= n_otu && bad_otu == ~0ull) bad_otu = i;
        keys[i] = key;
        vals[i] = (uint32_t)i;
    }
    if (bad_kmer != ~0ull) atomicMin(cnt + kMrgBadKmer, bad_kmer);
    if (bad_fn != ~0ull) atomicMin(cnt + kMrgBadFn, bad_fn);
    if (bad_otu != ~0ull) atomicMin(cnt + kMrgBadOtu, bad_otu);
}

__device__ __forceinline__ uint32_t merge_load_word(const uint8_t *rec, uint64_t i, uint32_t byte)
{
    return *reinterpret_cast<const uint32_t *>(rec + i * 24 + byte);
}

// One sorted pair per lane.  flag[i] = 1 iff the pair's record is in U.  A pair equal to its predecessor is a k-mer twice in
// one source.  Base pair i and new pair i + 1 of one k-mer are a conflict, counted (and its two functions compared, the new one
// through the map) by the base lane; a new pair without the base pair in front of it is an addition.
__global__ __launch_bounds__(kBuildThreads) void merge_resolve_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                                      uint64_t n_pairs, int policy, const uint8_t *__restrict__ entries,
                                                                      uint64_t records, const uint8_t *__restrict__ sigs, uint64_t n,
                                                                      const int32_t *__restrict__ fn_map, uint64_t n_fn,
                                                                      uint32_t *__restrict__ flag, unsigned long long *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBuildThreads + threadIdx.x;
    const bool valid = i < n_pairs;
    bool conflict = false, same = false, added = false;
    if (valid) {
        const uint64_t key = keys[i];
        const uint64_t before = i > 0 ? keys[i - 1] : ~0ull, behind = i + 1 < n_pairs ? keys[i + 1] : ~0ull;
        const bool is_new = key & 1;
        if (before == key) atomicMin(cnt + (is_new ? kMrgDupNew : kMrgDupBase), (unsigned long long)(key >> 1));
        bool keep;
        if (is_new) {
            const bool met = before == (key ^ 1);
            added = !met;
            keep = !met || policy == KG_MERGE_REPLACE;
        } else {
            conflict = behind == (key | 1);
            keep = !conflict || policy == KG_MERGE_KEEP;
            if (conflict) {
                const uint64_t slot = vals[i], from = vals[i + 1];
                if (slot < records && from < n) {
                    const uint32_t f_base = merge_load_word(entries, slot, 16);
                    uint32_t f_new = merge_load_word(sigs, from, 16);
                    if (fn_map) f_new = (uint64_t)(int64_t)(int32_t)f_new < n_fn ? (uint32_t)fn_map[f_new] : ~f_base;
                    same = f_base == f_new;
                }
                if (policy == KG_MERGE_DROP) keep = same;
            }
        }
        flag[i] = keep;
    }
    const uint64_t b_conflict = __ballot(conflict), b_same = __ballot(same), b_added = __ballot(added);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (b_conflict) atomicAdd(cnt + kMrgConflicts, (unsigned long long)__popcll(b_conflict));
        if (b_same) atomicAdd(cnt + kMrgSame, (unsigned long long)__popcll(b_same));
        if (b_added) atomicAdd(cnt + kMrgAdded, (unsigned long long)__popcll(b_added));
    }
}

// One sorted pair per lane: a flagged pair's 24 bytes go to out[rank[i]], from the table by slot or from the input by index
// with the maps applied to the two index fields.
__global__ __launch_bounds__(kBuildThreads) void merge_emit_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                                   const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank,
                                                                   uint64_t n_pairs, const uint8_t *__restrict__ entries, uint64_t records,
                                                                   const uint8_t *__restrict__ sigs, uint64_t n,
                                                                   const int32_t *__restrict__ fn_map, uint64_t n_fn,
                                                                   const int32_t *__restrict__ otu_map, uint64_t n_otu,
                                                                   uint8_t *__restrict__ out, uint64_t n_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBuildThreads + threadIdx.x;
    if (i >= n_pairs || !flag[i]) return;
    const bool is_new = keys[i] & 1;
    const uint64_t from = vals[i], to = rank[i];
    if (from >= (is_new ? n : records) || to >= n_out) return;          // (never: the indices are the call's own)
    const uint2 *src = reinterpret_cast<const uint2 *>((is_new ? sigs : entries) + from * 24);
    const uint2 r0 = src[0];
    uint2 r1 = src[1], r2 = src[2];
    if (is_new) {
        if (otu_map && (uint64_t)(int64_t)(int32_t)r1.x < n_otu) r1.x = (uint32_t)otu_map[r1.x];
        if (fn_map && (uint64_t)(int64_t)(int32_t)r2.x < n_fn) r2.x = (uint32_t)fn_map[r2.x];
    }
    uint2 *dst = reinterpret_cast<uint2 *>(out + to * 24);
    dst[0] = r0; dst[1] = r1; dst[2] = r2;
}

}  // namespace kg
