// kg_coding.hpp -- device side of kg_orfset_coding / kg_coding_counts_orfs / kg_coding_score_orfs (include/kmerguts_hip.h): the
// in-frame hexamer (dicodon) log-odds score of every ORF record (the rule is stated in the header, next to the entry points).
//
// Everything is integer: counts are 64-bit atomic adds, scores are sums of int32 table entries, so no order can matter.
//
//   1. coding_background_kernel  one streaming pass over the batch's bytes.  A lane owns kCodingBgPerLane consecutive hexamer
//                                starts (two 8-byte reads), a workgroup step kCodingBgTile of them; the grid is capped and strides.
//                                Contig borders come from the offsets: a lane looks up "the smallest offset above x" once and
//                                again only when a start passes it.  Forward hexamers go into a 4096-bin LDS histogram, flushed
//                                once per workgroup with 64-bit global atomics.  coding_fold_kernel then adds the other strand:
//                                B[h] = F[h] + F[rc(h)].
//   2. coding_lens_kernel        one lane per record: validation (error words by atomicMin, firing only on bad input; a bad record
//                                gets no pair and is never used as an index), the pairs max(n_res - 1, 0), the training records.
//      prefix_sum of the pairs.
//   3. coding_count_kernel       one lane per pair: the record by binary search in the prefix, the six bases by one 8-byte read
//                                of the contig (backwards and complemented on '-'), the training records' pairs into an LDS
//                                histogram as in 1.
//   4. coding_score_kernel       one lane per pair again, T[4096] in LDS: a wave's lanes hold consecutive pairs, so their records
//                                are sorted; a segmented wave sum and one 64-bit atomic add per wave and record segment.
//   5. coding_decide_kernel      one lane per record: rule 7.
// No lane walks a record's pairs: a 10^4-codon ORF is 10^4 lanes like any others.  A histogram add whose active lanes all hold
// one bin (a homopolymer) is one add of the lane count by one lane, so that case does not serialise on the bin.
#pragma once

#include "kg_device.hpp"
#include "kg_orfs.hpp"

namespace kg {

constexpr int kCodingBins = 4096;
constexpr int kCodingThreads = 256;
constexpr int kCodingBgPerLane = 8;                                 // hexamer starts of one lane of the background pass
constexpr int kCodingBgTile = kCodingThreads * kCodingBgPerLane;    // ... and of one workgroup step
constexpr uint32_t kCodingMaxGrid = 2048;                           // workgroups of the striding kernels
// error words: the first record [0] with a bad seq, [1] strand, [2] left / right outside the contig, [3] more codons than its extent
enum { kCodingErrSeq = 0, kCodingErrStrand = 1, kCodingErrRange = 2, kCodingErrLen = 3, kCodingErrWords = 4 };
// counter words: training records, non-coding records, then the pair total (the prefix sum's)
enum { kCodingCntTrain = 0, kCodingCntNoncoding = 1, kCodingCntPairs = 2, kCodingCntWords = 3 };
constexpr unsigned long long kCodingNoErr = 0x7F7F7F7F7F7F7F7Full;

// the index of the reverse complement: every 2-bit digit complemented, their order reversed
__host__ __device__ constexpr uint32_t coding_rc(uint32_t h)
{
    const uint32_t x = h ^ 0xFFFu;
    return ((x & 0x3u) << 10) | ((x & 0xCu) << 6) | ((x & 0x30u) << 2) | ((x >> 2) & 0x30u) | ((x >> 6) & 0xCu) | ((x >> 10) & 0x3u);
}

// One histogram add per lane that is `on`, from wave-uniform control flow.  When every active lane holds the same bin, one lane
// adds their number.
__device__ __forceinline__ void coding_hist_add(uint32_t *hist, bool on, uint32_t h)
{
    const uint64_t act = __ballot(on);
    if (act == 0) return;
    const int first = (int)__builtin_ctzll(act);
    const uint32_t h0 = (uint32_t)__shfl((int)h, first);
    if (__ballot(on && h == h0) == act) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[h0], (uint32_t)__builtin_popcountll(act));
    } else if (on) {
        atomicAdd(&hist[h], 1u);
    }
}

__device__ __forceinline__ void coding_hist_clear(uint32_t *hist)
{
    for (int b = threadIdx.x; b < kCodingBins; b += kCodingThreads) hist[b] = 0;
    __syncthreads();
}

__device__ __forceinline__ void coding_hist_flush(const uint32_t *hist, unsigned long long *out)
{
    __syncthreads();
    for (int b = threadIdx.x; b < kCodingBins; b += kCodingThreads)
        if (const uint32_t c = hist[b]) atomicAdd(&out[b], (unsigned long long)c);
}

// the smallest offsets[j] > x with j >= 1 -- the end of the contig that holds byte x -- or 0 when no contig holds it
__device__ inline int64_t coding_contig_end(const int64_t *__restrict__ offsets, uint64_t n_seqs, int64_t x)
{
    uint64_t lo = 0, hi = n_seqs + 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (offsets[mid] > x) hi = mid; else lo = mid + 1;
    }
    return (lo == 0 || lo == n_seqs + 1) ? 0 : offsets[lo];
}

// F[4096] += the forward hexamers of the batch.  n_tiles = ceil(total / kCodingBgTile).  A workgroup counts at most
// ceil(n_tiles / grid) * kCodingBgTile hexamers in 32 bits: the host keeps that below 2^32.
__global__ __launch_bounds__(kCodingThreads) void coding_background_kernel(const uint8_t *__restrict__ seq, uint64_t total,
                                                                           const int64_t *__restrict__ offsets, uint64_t n_seqs,
                                                                           uint64_t n_tiles, unsigned long long *F)
{
    __shared__ uint32_t hist[kCodingBins];
    coding_hist_clear(hist);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t a = tile * kCodingBgTile + (uint64_t)threadIdx.x * kCodingBgPerLane;
        const uint64_t w0 = orf_load8(seq, total, a), w1 = orf_load8(seq, total, a + 8);
        int64_t end = a < total ? coding_contig_end(offsets, n_seqs, (int64_t)a) : 0;
        uint32_t h = 0;
        int last_bad = -1;                              // the last base of code 4 among bases 0 .. j
#pragma unroll
        for (int j = 0; j < kCodingBgPerLane + 5; j++) {
            const uint32_t c = dna_code((uint32_t)((j < 8 ? w0 >> (8 * j) : w1 >> (8 * (j - 8))) & 0xFFu));
            h = ((h << 2) | (c & 3u)) & 0xFFFu;
            if (c > 3) last_bad = j;
            if (j >= 5) {
                const int k = j - 5;                    // the hexamer that starts at a + k and ends at base j
                const int64_t x = (int64_t)a + k;
                if (x >= end && (uint64_t)x < total && k > 0) end = coding_contig_end(offsets, n_seqs, x);
                coding_hist_add(hist, x + 6 <= end && last_bad < k, h);
            }
        }
    }
    coding_hist_flush(hist, F);
}

__global__ __launch_bounds__(kCodingThreads) void coding_fold_kernel(const unsigned long long *__restrict__ F, int64_t *__restrict__ B)
{
    const uint32_t h = blockIdx.x * kCodingThreads + threadIdx.x;
    if (h < (uint32_t)kCodingBins) B[h] = (int64_t)(F[h] + F[coding_rc(h)]);
}

__device__ __forceinline__ bool coding_is_training(const kg_orf &o)
{
    return o.kept != 0 && (o.flags & (KG_ORF_FREE | KG_ORF_INTERRUPTED)) == 0;
}

__global__ __launch_bounds__(256) void coding_lens_kernel(const kg_orf *__restrict__ orfs, uint64_t n, const int64_t *__restrict__ offsets,
                                                          uint64_t n_seqs, uint32_t *__restrict__ lens, unsigned long long *err,
                                                          unsigned long long *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const kg_orf o = orfs[i];
    uint32_t len = 0;
    if (o.seq < 0 || (uint64_t)o.seq >= n_seqs) {
        atomicMin(&err[kCodingErrSeq], (unsigned long long)i);
    } else if (o.strand != 0 && o.strand != 1) {
        atomicMin(&err[kCodingErrStrand], (unsigned long long)i);
    } else {
        const int64_t L = offsets[o.seq + 1] - offsets[o.seq];
        if (o.left < 0 || o.left > o.right || (int64_t)o.right >= L) {
            atomicMin(&err[kCodingErrRange], (unsigned long long)i);
        } else if (3 * (int64_t)o.n_res > (int64_t)o.right - o.left + 1) {
            atomicMin(&err[kCodingErrLen], (unsigned long long)i);
        } else {
            len = o.n_res > 1 ? (uint32_t)o.n_res - 1u : 0u;
            if (coding_is_training(o)) atomicAdd(&cnt[kCodingCntTrain], 1ull);
        }
    }
    lens[i] = len;
}

// Pair p of the list: its record (n > 0; the last i with excl[i] <= p) and its hexamer.  -> the pair exists; *known: none of its
// six bases has code 4.  Only a record that passed coding_lens_kernel owns pairs, so its fields are safe indices.
__device__ inline bool coding_pair(uint64_t p, const kg_orf *__restrict__ orfs, uint64_t n, const uint32_t *__restrict__ excl,
                                   const uint8_t *__restrict__ seq, uint64_t total, const int64_t *__restrict__ offsets, uint32_t *rec,
                                   kg_orf *o, uint32_t *h, bool *known)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)excl[mid] > p) hi = mid; else lo = mid + 1;
    }
    const uint64_t i = lo - 1;
    *rec = (uint32_t)i;
    *o = orfs[i];
    const uint64_t k = p - excl[i];
    if (o->n_res < 2 || k >= (uint64_t)(o->n_res - 1)) return false;
    const int64_t off = offsets[o->seq];
    // '+': strand bases 0 .. 5 of the pair are bytes a .. a + 5; '-': they are the complements of bytes a + 5 .. a
    const uint64_t a = (uint64_t)(o->strand == 0 ? off + o->left + 3 * (int64_t)k : off + o->right - 3 * (int64_t)k - 5);
    const uint64_t w = orf_load8(seq, total, a);
    uint32_t x = 0;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const uint32_t c = dna_code((uint32_t)(w >> (8 * j)) & 0xFFu);
        ok = ok && c < 4;
        x |= (c & 3u) << (2 * (5 - j));         // byte j as digit j, the first most significant
    }
    *h = o->strand == 0 ? x : coding_rc(x);
    *known = ok;
    return true;
}

// C[4096] += the pairs of the training records.  *d_pairs: the pair total; 2^32 or more is the host's KG_ERR_LIMIT, nothing is read.
__global__ __launch_bounds__(kCodingThreads) void coding_count_kernel(const kg_orf *__restrict__ orfs, uint64_t n,
                                                                      const uint32_t *__restrict__ excl, const uint64_t *__restrict__ d_pairs,
                                                                      const uint8_t *__restrict__ seq, uint64_t total,
                                                                      const int64_t *__restrict__ offsets, unsigned long long *C)
{
    __shared__ uint32_t hist[kCodingBins];
    const uint64_t P = *d_pairs;
    if (P >= (1ull << 32) || n == 0) return;
    coding_hist_clear(hist);
    for (uint64_t base = (uint64_t)blockIdx.x * kCodingThreads; base < P; base += (uint64_t)gridDim.x * kCodingThreads) {
        const uint64_t p = base + threadIdx.x;
        bool on = false;
        uint32_t h = 0;
        if (p < P) {
            uint32_t rec;
            kg_orf o;
            bool known;
            if (coding_pair(p, orfs, n, excl, seq, total, offsets, &rec, &o, &h, &known)) on = known && coding_is_training(o);
        }
        coding_hist_add(hist, on, h);
    }
    coding_hist_flush(hist, C);
}

// S[rec] += T[h] over the pairs of every record.
__global__ __launch_bounds__(kCodingThreads) void coding_score_kernel(const kg_orf *__restrict__ orfs, uint64_t n,
                                                                      const uint32_t *__restrict__ excl, const uint64_t *__restrict__ d_pairs,
                                                                      const uint8_t *__restrict__ seq, uint64_t total,
                                                                      const int64_t *__restrict__ offsets, const int32_t *__restrict__ T,
                                                                      int64_t *S)
{
    __shared__ int32_t tab[kCodingBins];
    const uint64_t P = *d_pairs;
    if (P >= (1ull << 32) || n == 0) return;
    for (int b = threadIdx.x; b < kCodingBins; b += kCodingThreads) tab[b] = T[b];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kCodingThreads; base < P; base += (uint64_t)gridDim.x * kCodingThreads) {
        const uint64_t p = base + threadIdx.x;
        uint32_t rec = 0xFFFFFFFFu;                     // no pair: behind every record
        long long v = 0;                                // 64 bits: a caller's table is any int32[4096]
        if (p < P) {
            uint32_t r, h;
            kg_orf o;
            bool known;
            if (coding_pair(p, orfs, n, excl, seq, total, offsets, &r, &o, &h, &known)) {
                rec = r;
                v = known ? (long long)tab[h] : 0;
            }
        }
        // the wave's records are sorted: an inclusive sum inside every run of equal records
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long y = __shfl_up(v, d);
            const uint32_t ry = (uint32_t)__shfl_up((int)rec, d);
            if (lane >= d && ry == rec) v += y;
        }
        const uint32_t next = (uint32_t)__shfl_down((int)rec, 1);
        if (rec != 0xFFFFFFFFu && (lane == 63 || next != rec))
            atomicAdd((unsigned long long *)&S[rec], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void coding_decide_kernel(kg_orf *__restrict__ out, uint64_t n, const int64_t *__restrict__ S,
                                                            int32_t min_coding, unsigned long long *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t flags = out[i].flags;
    if ((flags & KG_ORF_FREE) != 0 && out[i].kept != 0 && S[i] < (int64_t)min_coding) {
        out[i].kept = 0;
        out[i].flags = flags | KG_ORF_NONCODING;
        atomicAdd(&cnt[kCodingCntNoncoding], 1ull);
    }
}

}  // namespace kg
