// kg_build.hpp -- device side of kg_table_build / kg_table_build_device (include/kmerguts_hip.h): a signature list -> the
// records of kmer.table.mem_map, placed the way the reference's lookup finds them (KGJ:944-1034: from the home slot
// kmer % numSigs forward over occupied slots, no wrap-around).
//
// Placement (synth.build_table restates it in torch): sort the signatures by (home, kmer); pos_0 = home_0 and
// pos_i = max(home_i, pos_{i-1} + 1); a signature with pos_i >= numSigs is dropped; every other slot holds the empty record.
//
//   1. build_keys_kernel     c_i = home_i * Q + q_i (q_i = kmer_i / numSigs < Q): one integer with the order of (home, kmer),
//                            below 20^8 + numSigs; the key range is checked in the same pass
//   2. LSD radix sort of (c, input index), stable, <= 8 bits a pass:
//        build_hist_kernel     per-tile digit counts (LDS), digit-major: hist[d * n_tiles + tile]
//        prefix_sum            exclusive scan of hist = where every (digit, tile) starts
//        build_scatter_kernel  each wave takes 1024 consecutive items of its tile, ranks them stably among equal digits
//                              with ballots, and writes them behind the items of earlier waves / tiles
//   3. pos_i - i = max(home_i - i, pos_{i-1} - (i-1)): pos is i plus an inclusive prefix max of home_i - i, done as
//      reduce-then-scan over tiles (build_tile_max_kernel, build_tile_scan_kernel, then build_place_kernel applies it);
//      the tile pass also flags equal neighbours in c (a duplicated k-mer)
//   4. build_fill_kernel writes the empty pattern with 16-byte stores, build_place_kernel the placed records at pos_i
//      (payload gathered by input index); pos is strictly increasing, so the placed records are a prefix of the sorted list.
#pragma once

#include "kg_device.hpp"

namespace kg {

constexpr int kBuildThreads = 256;
constexpr int kBuildItems = 16;                                   // per thread
constexpr int kBuildTile = kBuildThreads * kBuildItems;           // 4096 items per workgroup
constexpr uint32_t kBuildWaveItems = kWave * kBuildItems;         // 1024 consecutive items per wave in the scatter pass
constexpr uint64_t kEmptyKey = (uint64_t)KG_MAX_ENCODED + 1;      // synth.EMPTY_KEY (KGJ:1000: any key > 20^8 is empty)

// floor(v / d) and v % d for any v < 2^63 with magic = floor(2^64 / d) (~0 for d = 1): q_est is q or q - 1, as in split_value.
__device__ __forceinline__ uint64_t build_divmod(uint64_t v, uint64_t d, uint64_t magic, uint64_t *r_out)
{
    uint64_t q = __umul64hi(v, magic);
    uint64_t r = v - q * d;
    if (r >= d) { r -= d; q += 1; }
    *r_out = r;
    return q;
}

__device__ __forceinline__ int64_t build_load_kmer(const uint8_t *sigs, uint64_t i)
{
    const uint2 a = *reinterpret_cast<const uint2 *>(sigs + i * 24);
    return (int64_t)(((uint64_t)a.y << 32) | a.x);
}

// keys[i] = home * Q + q, vals[i] = i; *bad = the smallest index whose k-mer lies outside [0, 20^8) (stays ~0 when none)
__global__ __launch_bounds__(kBuildThreads) void build_keys_kernel(const uint8_t *__restrict__ sigs, uint64_t n, uint64_t num_sigs,
                                                                   uint64_t magic, uint64_t Q, uint64_t *__restrict__ keys,
                                                                   uint32_t *__restrict__ vals, unsigned long long *bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long first_bad = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t kmer = build_load_kmer(sigs, i);
        uint64_t c = 0;
        if (kmer < 0 || kmer >= KG_MAX_ENCODED) {
            if (first_bad == ~0ull) first_bad = i;
        } else {
            uint64_t home;
            const uint64_t q = build_divmod((uint64_t)kmer, num_sigs, magic, &home);
            c = home * Q + q;
        }
        keys[i] = c;
        vals[i] = (uint32_t)i;
    }
    if (first_bad != ~0ull) atomicMin(bad, first_bad);
}

// hist[d * n_tiles + tile] = items of the tile whose digit (key >> shift) & (radix - 1) is d
__global__ __launch_bounds__(kBuildThreads) void build_hist_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint32_t shift,
                                                                   uint32_t radix, uint32_t n_tiles, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile;
    const uint64_t mask = radix - 1;
#pragma unroll 4
    for (int k = 0; k < kBuildItems; k++) {
        const uint64_t i = base + (uint64_t)k * kBuildThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & mask], 1u);
    }
    __syncthreads();
    if (threadIdx.x < radix) hist[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// offs = exclusive scan of hist.  Wave w of a tile owns items [tile * 4096 + w * 1024, + 1024), in 16 steps of 64: lane l
// holds item step * 64 + l.  The wave's digit counts put its items behind those of waves 0..w-1 of the tile; within a step
// the lanes with the same digit (found with one ballot per digit bit) take consecutive places in lane order.
__global__ __launch_bounds__(kBuildThreads) void build_scatter_kernel(const uint64_t *__restrict__ kin, const uint32_t *__restrict__ vin,
                                                                      uint64_t n, uint32_t shift, uint32_t bits, uint32_t n_tiles,
                                                                      const uint32_t *__restrict__ offs, uint64_t *__restrict__ kout,
                                                                      uint32_t *__restrict__ vout)
{
    constexpr int kWaves = kBuildThreads / kWave;
    __shared__ uint32_t cnt[kWaves][256];
    __shared__ uint32_t at[kWaves][256];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t radix = 1u << bits, mask = radix - 1;
    for (uint32_t j = threadIdx.x; j < kWaves * 256; j += kBuildThreads) (&cnt[0][0])[j] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile + (uint64_t)wave * kBuildWaveItems + lane;
    uint64_t k[kBuildItems];
    uint32_t v[kBuildItems];
#pragma unroll
    for (int s = 0; s < kBuildItems; s++) {
        const uint64_t i = base + (uint64_t)s * kWave;
        k[s] = i < n ? kin[i] : 0;
        v[s] = i < n ? vin[i] : 0;
        if (i < n) atomicAdd(&cnt[wave][(uint32_t)(k[s] >> shift) & mask], 1u);
    }
    __syncthreads();
    if (threadIdx.x < radix) {
        uint32_t run = offs[(uint64_t)threadIdx.x * n_tiles + blockIdx.x];
        for (int w = 0; w < kWaves; w++) {
            at[w][threadIdx.x] = run;
            run += cnt[w][threadIdx.x];
        }
    }
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1;
#pragma unroll
    for (int s = 0; s < kBuildItems; s++) {
        const uint64_t i = base + (uint64_t)s * kWave;
        const bool valid = i < n;
        const uint32_t d = (uint32_t)(k[s] >> shift) & mask;
        uint64_t peers = __ballot(valid);
        for (uint32_t b = 0; b < bits; b++) {
            const uint64_t set = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? set : ~set;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lt);
        uint32_t o = 0;
        if (valid) o = at[wave][d] + rank;
        wave_sync();                                    // every lane has read its base before the first lane of a group moves it
        if (valid && o < n) {                            // (o < n holds whenever the counts agree with the histogram pass)
            kout[o] = k[s];
            vout[o] = v[s];
            if (rank == 0) at[wave][d] += (uint32_t)__popcll(peers);
        }
        wave_sync();
    }
}

// tile_max[tile] = max over the tile's items of home_i - i; *dup = the smallest k-mer that occurs twice (stays ~0 when none)
__global__ __launch_bounds__(kBuildThreads) void build_tile_max_kernel(const uint64_t *__restrict__ c, uint64_t n, uint64_t Q,
                                                                       uint64_t magic_q, uint64_t num_sigs, int64_t *__restrict__ tile_max,
                                                                       unsigned long long *dup)
{
    __shared__ int64_t wmax[kBuildThreads / kWave];
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile;
    int64_t m = INT64_MIN;
    unsigned long long d = ~0ull;
    for (int k = 0; k < kBuildItems; k++) {
        const uint64_t i = base + (uint64_t)k * kBuildThreads + threadIdx.x;
        if (i >= n) break;
        const uint64_t ci = c[i];
        uint64_t q;
        const uint64_t home = build_divmod(ci, Q, magic_q, &q);
        const int64_t a = (int64_t)home - (int64_t)i;
        m = a > m ? a : m;
        if (i > 0 && c[i - 1] == ci) {
            const unsigned long long kmer = q * num_sigs + home;
            d = kmer < d ? kmer : d;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t y = __shfl_down(m, off);
        m = y > m ? y : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x / kWave] = m;
    if (d != ~0ull) atomicMin(dup, d);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBuildThreads / kWave; w++) m = wmax[w] > m ? wmax[w] : m;
        tile_max[blockIdx.x] = m;
    }
}

// one workgroup: tile_pre[t] = max(tile_max[0 .. t)) (INT64_MIN for t = 0)
__global__ __launch_bounds__(kBuildThreads) void build_tile_scan_kernel(const int64_t *__restrict__ tile_max, uint32_t n_tiles,
                                                                        int64_t *__restrict__ tile_pre)
{
    __shared__ int64_t carry;
    __shared__ int64_t wsum[kBuildThreads / kWave];
    if (threadIdx.x == 0) carry = INT64_MIN;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t b = 0; b < n_tiles; b += kBuildThreads) {
        const uint32_t i = b + threadIdx.x;
        const int64_t x = i < n_tiles ? tile_max[i] : INT64_MIN;
        int64_t incl = x;
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t y = __shfl_up(incl, off);
            if (lane >= off) incl = y > incl ? y : incl;
        }
        int64_t excl = __shfl_up(incl, 1);
        if (lane == 0) excl = INT64_MIN;
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int64_t pre = carry, all = carry;
        for (int w = 0; w < kBuildThreads / kWave; w++) {
            const int64_t s = wsum[w];
            if (w < wave) pre = s > pre ? s : pre;
            all = s > all ? s : all;
        }
        if (i < n_tiles) tile_pre[i] = excl > pre ? excl : pre;
        __syncthreads();
        if (threadIdx.x == 0) carry = all;
        __syncthreads();
    }
}

// the empty pattern over n_chunks 16-byte chunks: two records are three chunks {key lo, key hi, 0, 0} {0, 0, key lo, key hi} {0 x 4}
__global__ __launch_bounds__(kBuildThreads) void build_fill_kernel(uint4 *__restrict__ dst, uint64_t n_chunks)
{
    const uint32_t lo = (uint32_t)kEmptyKey, hi = (uint32_t)(kEmptyKey >> 32);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_chunks; j += stride) {
        const uint32_t r = (uint32_t)(j % 3);
        dst[j] = r == 0 ? make_uint4(lo, hi, 0, 0) : r == 1 ? make_uint4(0, 0, lo, hi) : make_uint4(0, 0, 0, 0);
    }
}

// Thread t of a tile takes items [tile * 4096 + t * 16, + 16): pos_i = i + max(tile_pre, the maxima of the threads in front,
// home_j - j for the thread's items j <= i).  Records with pos_i < num_sigs are copied to entries[pos_i]; *placed counts them.
__global__ __launch_bounds__(kBuildThreads) void build_place_kernel(const uint64_t *__restrict__ c, const uint32_t *__restrict__ idx,
                                                                    uint64_t n, uint64_t Q, uint64_t magic_q,
                                                                    const int64_t *__restrict__ tile_pre, const uint8_t *__restrict__ sigs,
                                                                    uint64_t num_sigs, uint8_t *__restrict__ entries,
                                                                    unsigned long long *placed)
{
    __shared__ int64_t wmax[kBuildThreads / kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile + (uint64_t)threadIdx.x * kBuildItems;
    int64_t a[kBuildItems];
    int64_t m = INT64_MIN;
#pragma unroll
    for (int k = 0; k < kBuildItems; k++) {
        const uint64_t i = base + k;
        a[k] = INT64_MIN;
        if (i < n) {
            uint64_t q;
            const uint64_t home = build_divmod(c[i], Q, magic_q, &q);
            a[k] = (int64_t)home - (int64_t)i;
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
    unsigned long long cnt = 0;
#pragma unroll
    for (int k = 0; k < kBuildItems; k++) {
        const uint64_t i = base + k;
        if (i >= n) break;
        run = a[k] > run ? a[k] : run;
        const int64_t pos = run + (int64_t)i;            // >= home_i >= 0
        const uint64_t from = idx[i];
        if (pos < (int64_t)num_sigs && from < n) {
            const uint2 *src = reinterpret_cast<const uint2 *>(sigs + from * 24);
            uint2 *dst = reinterpret_cast<uint2 *>(entries + (uint64_t)pos * 24);
            const uint2 r0 = src[0], r1 = src[1], r2 = src[2];
            dst[0] = r0; dst[1] = r1; dst[2] = r2;
            cnt++;
        }
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if (lane == 0 && cnt) atomicAdd(placed, cnt);
}

}  // namespace kg
