// kg_seed.hpp -- device side of kg_proteins_search_seeded (include/kmerguts_hip.h states the rule): the window kernel that turns
// residues into seed ids under a reduced alphabet and up to four spaced shapes.  It stands where derive_windows_kernel stands in
// the exact search; the sort, the collapse and everything behind them (kg_derive.hpp, kg_search.hpp) read "seed id" for "k-mer".
//
// One wave per block of 64 window positions of one protein, grid-stride over the blocks (the block list is build_blocks_kernel's,
// counted for len - span_min positions).  The wave loads the block's min(64 + span_max - 1, len - 64 j) characters, two byte
// loads per lane and never one behind the protein's end, and leaves their class codes in its LDS row: cls[code] for a residue,
// 0xFF for anything else and for the places behind the end.  A shape is then w byte reads per lane at lane + j over the set
// bits j of its mask: the mask is a kernel argument, so the walk over its bits is scalar and the same for every lane.
//   EMIT = false: *count += the valid (window, shape) pairs: a ballot per shape, one LDS atomic per wave, one global per workgroup
//   EMIT = true : keys[o] = id << b | rank_of[p], vals[o] = len_p - i; one cursor atomic per wave and block for all its shapes
// The emission order does not matter: the sort follows.
#pragma once

#include "kg_device.hpp"

namespace kg {

constexpr int kSeedMaxShapes = 4;
constexpr int kSeedMaxSpan = 32;
constexpr int kSeedRow = 128;                       // class codes of a block: 64 + 31 are read, two stores of 64 are made

struct SeedSpec {                                   // a checked kg_seed_params, by value in the kernel arguments
    uint32_t n_shapes, alphabet, span_max, pad;
    uint32_t shape[kSeedMaxShapes];
    uint32_t cls4[5];                               // cls[c] = byte c & 3 of cls4[c >> 2]
    uint32_t pad2;
    uint64_t per_shape;                             // alphabet^weight: the id of (shape k, value) is k * per_shape + value
};

// the lane's window under one shape (`mask` is wave-uniform: the walk over its bits is scalar): whether every care position holds
// a residue, and the base-A value over the care positions, lowest position first
__device__ __forceinline__ bool seed_valid(const uint8_t *row, int lane, uint32_t mask)
{
    uint32_t any = 0;
    for (uint32_t m = mask; m; m &= m - 1) any |= row[lane + __builtin_ctz(m)];
    return (any & 0x80u) == 0u;
}

__device__ __forceinline__ uint64_t seed_value(const uint8_t *row, int lane, uint32_t mask, uint32_t alphabet)
{
    uint64_t v = 0;
    for (uint32_t m = mask; m; m &= m - 1) v = v * alphabet + row[lane + __builtin_ctz(m)];
    return v;
}

template <bool EMIT>
__global__ __launch_bounds__(kWave * kWavesPerWG) void seed_windows_kernel(const uint8_t *__restrict__ seq, const BlockDesc *__restrict__ blocks,
                                                                           uint32_t n_blocks, SeedSpec sd, unsigned long long *__restrict__ count,
                                                                           const uint32_t *__restrict__ rank_of, uint32_t b,
                                                                           uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                                           unsigned long long *cursor, uint64_t cap)
{
    __shared__ uint8_t table[256];
    __shared__ __attribute__((aligned(16))) uint8_t rows[kWavesPerWG][kSeedRow];
    __shared__ unsigned long long wg_count;
    for (uint32_t ch = threadIdx.x; ch < 256; ch += kWave * kWavesPerWG) {      // (the launch has kWave * kWavesPerWG threads: one step)
        uint32_t c = 0xFFu;
#pragma unroll
        for (uint32_t i = 0; i < 20; i++)
            if ("ACDEFGHIKLMNPQRSTVWY"[i] == (char)ch) c = (sd.cls4[i >> 2] >> (8u * (i & 3u))) & 255u;
        table[ch] = (uint8_t)c;
    }
    if (!EMIT && threadIdx.x == 0) wg_count = 0;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    uint8_t *row = rows[wave];
    const uint64_t lt = (1ull << lane) - 1;
    unsigned long long counted = 0;
    for (uint32_t it = blockIdx.x * kWavesPerWG + wave; it < n_blocks; it += gridDim.x * kWavesPerWG) {
        const BlockDesc bd = blocks[it];
        const uint32_t w0 = bd.j * kAaWinPerBlock;
        const uint32_t nload = min((uint32_t)kAaWinPerBlock + sd.span_max - 1u, bd.len - w0);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint32_t q = (uint32_t)lane + 64u * k;
            const uint32_t ch = q < nload ? seq[bd.soff + w0 + q] : 0u;
            row[q] = q < nload ? table[ch & 255u] : (uint8_t)0xFFu;
        }
        wave_sync();
        const uint32_t i = w0 + (uint32_t)lane;
        // pass 1: which (window, shape) pairs are valid -- bit k of okbits, and their number in the wave
        uint32_t okbits = 0, n_ok = 0;
#pragma unroll 1
        for (uint32_t k = 0; k < sd.n_shapes; k++) {
            const uint32_t mask = sd.shape[k];
            const uint32_t span = 32u - (uint32_t)__builtin_clz(mask);
            const bool ok = seed_valid(row, lane, mask) && (uint64_t)i + span < (uint64_t)bd.len;
            okbits |= (ok ? 1u : 0u) << k;
            n_ok += (uint32_t)__popcll(__ballot(ok));
        }
        if (!EMIT) {
            counted += n_ok;
        } else {
            // pass 2: one cursor step for the wave's seeds of all shapes, then the values shape by shape
            unsigned long long base = 0;
            if (lane == 0 && n_ok) base = atomicAdd(cursor, (unsigned long long)n_ok);
            base = __shfl(base, 0);
            const uint64_t r = rank_of[bd.seq];
#pragma unroll 1
            for (uint32_t k = 0; k < sd.n_shapes; k++) {
                const bool ok = (okbits >> k) & 1u;
                const uint64_t m = __ballot(ok);
                const uint64_t o = base + (uint64_t)__popcll(m & lt);
                const uint64_t v = seed_value(row, lane, sd.shape[k], sd.alphabet);
                if (ok && o < cap) {
                    keys[o] = (((uint64_t)k * sd.per_shape + v) << b) | r;
                    vals[o] = bd.len - i;
                }
                base += (uint64_t)__popcll(m);
            }
        }
        wave_sync();                                    // the wave's row is rewritten by its next block
    }
    if (!EMIT) {
        if (lane == 0 && counted) atomicAdd(&wg_count, counted);
        __syncthreads();
        if (threadIdx.x == 0 && wg_count) atomicAdd(count, wg_count);
    }
}

}  // namespace kg
