// kg_mask.hpp -- device side of kg_proteins_mask and of the soft masking in kg_proteins_search_masked / kg_proteins_cluster_masked
// (include/kmerguts_hip.h states the rule): low-complexity segments of proteins by SEG's trigger window and extension.
//
// Four passes over the block list of build_blocks_kernel, counted for the len - W + 1 window positions of every protein:
//   mask_windows_kernel  one wave per block of 64 window positions, grid-stride.  The wave loads the block's min(64 + W - 1,
//                        len - 64 j) characters, two byte loads per lane and never one behind the protein's end, and leaves their
//                        letters 0..20 in its LDS row.  A lane counts the letters of its window in three registers of seven
//                        8-bit fields, adds n * Lg(n) of the 21 fields from the LDS table and has D.  Two ballots per block,
//                        `low` and `ext`, leave as 64-bit words.  A position without a window has neither bit.
//   mask_runs_kernel     one lane per protein over its words: the ext runs that hold a low bit, filled upwards with a carry from
//                        word to word and then downwards with a carry back.  The words that come out are the masking windows.
//   mask_residues_kernel one wave per block: residue r is masked iff a masking window lies in r - W + 1 .. r.  The last block of a
//                        protein takes the W - 1 residues behind its last window too.  One flag byte per residue, and per block
//                        the number of segment starts, which a prefix sum turns into the index of the block's first segment.
//   mask_segments_kernel one wave per block: a start writes (protein, start) of its segment and an end writes (end, 0).  Segment
//                        k's end is the k-th end in (protein, residue) order, so an end needs only the starts in front of it.
// mask_apply_kernel writes the seeding copy: a masked byte with 0x20 set (a letter in lowercase), any other byte as it is.
// Nothing depends on the grid: a block's words, flags and counts have one writer each.
#pragma once

#include "kg_device.hpp"

namespace kg {

constexpr int kMaskMaxWindow = 32;
constexpr int kMaskRow = 128;                       // letters of a block: 64 + 31 are read, two stores of 64 are made
constexpr int kMaskLetters = 21;                    // toAminoAcidOff's 0..19 and 20 for every other byte
enum : int { kMaskWindows = 0, kMaskLow = 1, kMaskExt = 2, kMaskMasking = 3, kMaskResidues = 4, kMaskProteins = 5, kMaskWords = 6 };

struct MaskSpec {                                   // a checked kg_mask_params, by value in the kernel arguments
    uint32_t window, low_max, ext_max, full;        // D <= low_max: low; D <= ext_max: ext; full = W * Lg(W)
    uint16_t nlg[kMaskMaxWindow + 1];               // n * Lg(n), nlg[0] = 0
    uint16_t pad;
};

struct MaskSeg { int32_t protein, start, end, reserved; };
static_assert(sizeof(MaskSeg) == sizeof(kg_mask_segment), "record layouts of include/kmerguts_hip.h");

__global__ __launch_bounds__(kWave * kWavesPerWG) void mask_windows_kernel(const uint8_t *__restrict__ seq, const BlockDesc *__restrict__ blocks,
                                                                           uint32_t n_blocks, MaskSpec ms, uint64_t *__restrict__ low_words,
                                                                           uint64_t *__restrict__ ext_words)
{
    __shared__ uint32_t nlg[kMaskMaxWindow + 1];
    __shared__ __attribute__((aligned(16))) uint8_t rows[kWavesPerWG][kMaskRow];
    if (threadIdx.x <= kMaskMaxWindow) nlg[threadIdx.x] = ms.nlg[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    uint8_t *row = rows[wave];
    for (uint32_t it = blockIdx.x * kWavesPerWG + wave; it < n_blocks; it += gridDim.x * kWavesPerWG) {
        const BlockDesc bd = blocks[it];
        const uint32_t w0 = bd.j * kAaWinPerBlock;
        const uint32_t nload = min((uint32_t)kAaWinPerBlock + ms.window - 1u, bd.len - w0);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint32_t q = (uint32_t)lane + 64u * k;
            const uint32_t ch = q < nload ? seq[bd.soff + w0 + q] : 0u;
            row[q] = (uint8_t)aa_code_of_rt((char)ch);
        }
        wave_sync();
        // the lane's window: the counts of letters 7 g .. 7 g + 6 are the bytes of c[g]
        uint64_t c0 = 0, c1 = 0, c2 = 0;
#pragma unroll 1
        for (uint32_t k = 0; k < ms.window; k++) {
            const uint32_t a = row[lane + k], g = a / 7u;
            const uint64_t one = 1ull << (8u * (a - 7u * g));
            c0 += g == 0u ? one : 0ull;
            c1 += g == 1u ? one : 0ull;
            c2 += g == 2u ? one : 0ull;
        }
        uint32_t sum = 0;
#pragma unroll
        for (int f = 0; f < 7; f++)
            sum += nlg[(c0 >> (8 * f)) & 255u] + nlg[(c1 >> (8 * f)) & 255u] + nlg[(c2 >> (8 * f)) & 255u];
        const uint32_t D = ms.full - sum;
        const bool exists = (uint64_t)w0 + (uint32_t)lane + ms.window <= (uint64_t)bd.len;
        const uint64_t low = __ballot(exists && D <= ms.low_max), ext = __ballot(exists && D <= ms.ext_max);
        if (lane == 0) {
            low_words[it] = low;
            ext_words[it] = ext;
        }
        wave_sync();                                    // the wave's row is rewritten by its next block
    }
}

// the bits of p that a run of p bits joins to a bit of g, upwards (towards bit 63) and downwards; g is within p
__device__ __forceinline__ uint64_t mask_fill_up(uint64_t g, uint64_t p)
{
    g |= p & (g << 1);  p &= p << 1;
    g |= p & (g << 2);  p &= p << 2;
    g |= p & (g << 4);  p &= p << 4;
    g |= p & (g << 8);  p &= p << 8;
    g |= p & (g << 16); p &= p << 16;
    g |= p & (g << 32);
    return g;
}

__device__ __forceinline__ uint64_t mask_fill_down(uint64_t g, uint64_t p)
{
    g |= p & (g >> 1);  p &= p >> 1;
    g |= p & (g >> 2);  p &= p >> 2;
    g |= p & (g >> 4);  p &= p >> 4;
    g |= p & (g >> 8);  p &= p >> 8;
    g |= p & (g >> 16); p &= p >> 16;
    g |= p & (g >> 32);
    return g;
}

// ibase[p] .. ibase[p + 1]: the words of protein p.  windows[p]: its window positions (for the statistics)
__global__ void mask_runs_kernel(const uint32_t *__restrict__ ibase, const int64_t *__restrict__ off, uint32_t n_prot, uint32_t window,
                                 const uint64_t *__restrict__ low_words, const uint64_t *__restrict__ ext_words, uint64_t *__restrict__ mask_words,
                                 unsigned long long *__restrict__ counts)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_prot) return;
    const uint32_t a = ibase[p], b = ibase[p + 1];
    const int64_t len = off[p + 1] - off[p];
    unsigned long long n_low = 0, n_ext = 0, n_mask = 0;
    uint64_t carry = 0;
    for (uint32_t k = a; k < b; k++) {
        const uint64_t e = ext_words[k], l = low_words[k] & e;
        const uint64_t up = mask_fill_up(l | (carry & e), e);
        mask_words[k] = up;
        carry = up >> 63;
        n_low += (unsigned long long)__popcll(l);
        n_ext += (unsigned long long)__popcll(e);
    }
    carry = 0;
    for (uint32_t k = b; k > a; k--) {
        const uint64_t e = ext_words[k - 1];
        const uint64_t dn = mask_fill_down(mask_words[k - 1] | ((carry << 63) & e), e);
        mask_words[k - 1] = dn;
        carry = dn & 1ull;
        n_mask += (unsigned long long)__popcll(dn);
    }
    if (len >= (int64_t)window) atomicAdd(counts + kMaskWindows, (unsigned long long)(len - window + 1));
    if (n_low) atomicAdd(counts + kMaskLow, n_low);
    if (n_ext) atomicAdd(counts + kMaskExt, n_ext);
    if (n_mask) atomicAdd(counts + kMaskMasking, n_mask);
}

// whether residue r of a protein with nwin >= 1 window positions is masked; words: the protein's masking words
__device__ __forceinline__ bool mask_residue(const uint64_t *__restrict__ words, uint32_t r, uint32_t window, uint32_t nwin)
{
    const uint32_t lo = r + 1u >= window ? r + 1u - window : 0u, hi = min(r, nwin - 1u);
    if (hi < lo) return false;
    const uint32_t wa = lo >> 6, wb = hi >> 6;
    const uint64_t upto = ~0ull >> (63u - (hi & 63u));                  // bits 0 .. hi & 63
    if (wa == wb) return ((words[wa] & upto) >> (lo & 63u)) != 0ull;
    return (words[wa] >> (lo & 63u)) != 0ull || (words[wb] & upto) != 0ull;
}

// The residues of a block: w0 .. w0 + 63, and in a protein's last block on to its end (at most W - 1 more: two steps of 64).
// SEGMENTS = false: flags[soff + r], blk_starts[it] = the segment starts among them, counts[kMaskResidues]
// SEGMENTS = true : segs[blk_base[it] + the starts in front of r in the block] from the flags
template <bool SEGMENTS>
__global__ __launch_bounds__(kWave * kWavesPerWG) void mask_residues_kernel(const BlockDesc *__restrict__ blocks, uint32_t n_blocks, uint32_t window,
                                                                            const uint64_t *__restrict__ mask_words, uint8_t *__restrict__ flags,
                                                                            uint32_t *__restrict__ blk_starts, const uint32_t *__restrict__ blk_base,
                                                                            MaskSeg *__restrict__ segs, uint64_t n_segs,
                                                                            unsigned long long *__restrict__ counts)
{
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const uint64_t le = ~0ull >> (63 - lane);                           // lanes 0 .. lane
    unsigned long long masked_total = 0;
    for (uint32_t it = blockIdx.x * kWavesPerWG + wave; it < n_blocks; it += gridDim.x * kWavesPerWG) {
        const BlockDesc bd = blocks[it];
        const uint32_t w0 = bd.j * kAaWinPerBlock, nwin = bd.len - window + 1u;
        const uint32_t r_end = bd.j + 1u == bd.nk ? bd.len : w0 + (uint32_t)kAaWinPerBlock;
        const uint64_t *words = mask_words + bd.ibase;
        uint32_t starts_before = 0;
#pragma unroll 1
        for (uint32_t step = 0; step < 2u; step++) {
            const uint32_t r = w0 + 64u * step + (uint32_t)lane;
            const bool in = r < r_end;
            bool m, before, after;
            if (!SEGMENTS) {
                m = in && mask_residue(words, r, window, nwin);
                before = in && r > 0u && mask_residue(words, r - 1u, window, nwin);
                after = false;
                if (in) flags[bd.soff + r] = m ? 1 : 0;
                masked_total += (unsigned long long)__popcll(__ballot(m));
            } else {
                m = in && flags[bd.soff + r] != 0;
                before = in && r > 0u && flags[bd.soff + r - 1u] != 0;
                after = in && r + 1u < bd.len && flags[bd.soff + r + 1u] != 0;
            }
            const uint64_t starts = __ballot(m && !before);
            if (SEGMENTS) {
                const uint64_t k = (uint64_t)blk_base[it] + starts_before + (uint64_t)__popcll(starts & le) - 1u;   // m: a start at or in front of r
                if (m && !before && k < n_segs) *(int2 *)&segs[k].protein = make_int2((int)bd.seq, (int)r);
                if (m && !after && k < n_segs) *(int2 *)&segs[k].end = make_int2((int)r, 0);
            }
            starts_before += (uint32_t)__popcll(starts);
        }
        if (!SEGMENTS && lane == 0) blk_starts[it] = starts_before;
    }
    if (!SEGMENTS && lane == 0 && masked_total) atomicAdd(counts + kMaskResidues, masked_total);
}

// seg_start[p] = the segments in front of protein p (blk_base of its first block; *total behind the last block), p <= n_prot;
// counts[kMaskProteins] += the proteins with a segment
__global__ void mask_starts_kernel(const uint32_t *__restrict__ ibase, uint32_t n_prot, uint32_t n_blocks, const uint32_t *__restrict__ blk_base,
                                   const uint64_t *__restrict__ total, int64_t *__restrict__ seg_start, unsigned long long *__restrict__ counts)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    int64_t s = 0, e = 0;
    if (p <= n_prot) {
        const uint32_t a = ibase[p];
        s = e = a < n_blocks ? (int64_t)blk_base[a] : (int64_t)*total;
        seg_start[p] = s;
    }
    if (p < n_prot) {
        const uint32_t b = ibase[p + 1];
        e = b < n_blocks ? (int64_t)blk_base[b] : (int64_t)*total;
    }
    const uint64_t any = __ballot(e > s);
    if ((threadIdx.x & (kWave - 1)) == 0 && any) atomicAdd(counts + kMaskProteins, (unsigned long long)__popcll(any));
}

// dst[k] = seq[k] with 0x20 set where flags[k] is set and lo <= k < hi, else seq[k]; k < n
__global__ void mask_apply_kernel(const uint8_t *__restrict__ seq, const uint8_t *__restrict__ flags, uint64_t n, uint64_t lo, uint64_t hi,
                                  uint8_t *__restrict__ dst)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t ch = seq[k];
        dst[k] = k >= lo && k < hi && flags[k] ? (uint8_t)(ch | 0x20u) : ch;
    }
}

}  // namespace kg
