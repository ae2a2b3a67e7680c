// kg_compose.hpp -- device side of kg_contigs_compose (include/kmerguts_hip.h): the tetranucleotide composition of every contig,
// the label rows of the training contigs, and every contig's score under every model (the rule is stated in the header, next
// to the entry point).
//
// Everything is integer: counts are 32-bit atomic adds into a contig's row (a contig has fewer than 2^30 windows), label rows
// are 64-bit atomic adds, scores are 64-bit sums of products, so no order can matter.
//
//   1. comp_count_kernel   one streaming pass over the batch's bytes, shaped like coding_background_kernel.  A lane owns
//                          kCompPerLane consecutive tetramer starts (two 8-byte reads), a workgroup step kCompTile of them; a
//                          workgroup owns a run of consecutive steps.  The 256-bin LDS histogram holds the contig the step's
//                          first byte lies in and is flushed to that contig's row F_s when a step begins in another contig: a
//                          4 Mbp contig is flushed once per workgroup.  A window of a further contig inside the step goes
//                          straight to its own row with one global atomic add -- such a contig begins inside the step, so it
//                          adds fewer than kCompTile of them, and 70 000 contigs of 10 bp stream like one long contig.
//      comp_fold_kernel    one workgroup step per contig, in place: N_s[t] = F_s[t] + F_s[rc(t)], windows_s = the row's sum.
//   2. comp_train_kernel   the rows of equal label summed: the host groups the contigs by row (and all of them once more for
//                          the background) and cuts every group into pieces of kCompTrainChunk contigs; a workgroup sums a
//                          piece in registers, lane t the bin t, and adds it with one 64-bit atomic per bin and piece.
//   3. comp_score_kernel   integer N x W^T.  A wave holds one contig's row (four bins a lane); W goes through LDS in tiles of
//                          kCompScoreTile models, so M is bounded by no LDS size; a wave sum per (contig, model) in 64 bits; the
//                          first two rows of rule 7 are kept on the way and the class record is written at the end (rule 8).
// No lane walks a contig.  A histogram add whose active lanes all hold one bin (a homopolymer) is one add of the lane count by
// one lane (coding_hist_add).
#pragma once

#include "kg_device.hpp"
#include "kg_orfs.hpp"
#include "kg_coding.hpp"

namespace kg {

constexpr int kCompBins = 256;
constexpr int kCompThreads = 256;                                   // = kCompBins: lane t of a workgroup owns bin t of a row
constexpr int kCompPerLane = 8;                                     // tetramer starts of one lane of the count pass
constexpr int kCompTile = kCompThreads * kCompPerLane;              // ... and of one workgroup step
constexpr uint32_t kCompMaxGrid = 2048;                             // workgroups of the count pass and the striding kernels
constexpr int kCompTrainChunk = 64;                                 // contigs of one piece of the train pass
constexpr int kCompScoreTile = 16;                                  // models of one LDS tile of W (16 KiB)
constexpr int kCompScoreSeqs = kCompThreads / 64;                   // contigs of one workgroup step of the score pass: one a wave
// counter words: decided contigs, decided unlabelled contigs, conflicts, all windows
enum { kCompCntDecided = 0, kCompCntUnlabelled = 1, kCompCntConflicts = 2, kCompCntWindows = 3, kCompCntWords = 4 };

struct CompWork { uint32_t row, first, count, pad; };               // a piece of the train pass: order[first .. first + count) into row
struct CompDecide { int32_t min_len, min_margin; };

// the index of the reverse complement: every 2-bit digit complemented, their order reversed
__host__ __device__ constexpr uint32_t comp_rc(uint32_t t)
{
    const uint32_t x = t ^ 0xFFu;
    return ((x & 0x3u) << 6) | ((x & 0xCu) << 2) | ((x >> 2) & 0xCu) | ((x >> 6) & 0x3u);
}

// the contig that holds byte x -- offsets[j] <= x < offsets[j + 1] -- or -1 when none does
__device__ inline int64_t comp_contig_of(const int64_t *__restrict__ offsets, uint64_t n_seqs, int64_t x)
{
    uint64_t lo = 0, hi = n_seqs + 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (offsets[mid] > x) hi = mid; else lo = mid + 1;
    }
    return (lo == 0 || lo == n_seqs + 1) ? -1 : (int64_t)lo - 1;
}

// the histogram into row `cur` (none when cur < 0), and cleared
__device__ __forceinline__ void comp_hist_flush(uint32_t *hist, uint32_t *__restrict__ F, int64_t cur)
{
    __syncthreads();
    const uint32_t c = hist[threadIdx.x];
    if (c != 0 && cur >= 0) atomicAdd(&F[(uint64_t)cur * kCompBins + threadIdx.x], c);
    hist[threadIdx.x] = 0;
    __syncthreads();
}

// F[n_seqs][256] += the forward tetramers of every contig.  n_tiles = ceil(total / kCompTile); workgroup b owns the steps
// b * tiles_per_wg .. and counts at most tiles_per_wg * kCompTile windows in 32 bits (total < 2^40: below 2^30).
__global__ __launch_bounds__(kCompThreads) void comp_count_kernel(const uint8_t *__restrict__ seq, uint64_t total,
                                                                  const int64_t *__restrict__ offsets, uint64_t n_seqs, uint64_t n_tiles,
                                                                  uint64_t tiles_per_wg, uint32_t *__restrict__ F)
{
    __shared__ uint32_t hist[kCompBins];
    hist[threadIdx.x] = 0;
    __syncthreads();
    int64_t cur = -1;                                   // the contig the histogram holds
    const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_wg, t1 = t0 + tiles_per_wg < n_tiles ? t0 + tiles_per_wg : n_tiles;
    for (uint64_t tile = t0; tile < t1; tile++) {
        const uint64_t x0 = tile * kCompTile;
        const int64_t first = comp_contig_of(offsets, n_seqs, (int64_t)x0);     // (the same in every lane)
        if (first != cur) {
            comp_hist_flush(hist, F, cur);
            cur = first;
        }
        const uint64_t a = x0 + (uint64_t)threadIdx.x * kCompPerLane;
        const uint64_t w0 = orf_load8(seq, total, a), w1 = orf_load8(seq, total, a + 8);
        int64_t si = a < total ? comp_contig_of(offsets, n_seqs, (int64_t)a) : -1;
        int64_t end = si >= 0 ? offsets[si + 1] : 0;
        uint32_t t = 0;
        int last_bad = -1;                              // the last base of code 4 among bases 0 .. j
#pragma unroll
        for (int j = 0; j < kCompPerLane + 3; j++) {
            const uint32_t c = dna_code((uint32_t)((j < 8 ? w0 >> (8 * j) : w1 >> (8 * (j - 8))) & 0xFFu));
            t = ((t << 2) | (c & 3u)) & 0xFFu;
            if (c > 3) last_bad = j;
            if (j >= 3) {
                const int k = j - 3;                    // the tetramer that starts at a + k and ends at base j
                const int64_t x = (int64_t)a + k;
                if (k > 0 && x >= end && (uint64_t)x < total) {
                    si = comp_contig_of(offsets, n_seqs, x);
                    end = si >= 0 ? offsets[si + 1] : 0;
                }
                const bool ok = x + 4 <= end && last_bad < k;       // (end > 0 only with si >= 0)
                coding_hist_add(hist, ok && si == cur, t);
                if (ok && si != cur) atomicAdd(&F[(uint64_t)si * kCompBins + t], 1u);
            }
        }
    }
    comp_hist_flush(hist, F, cur);
}

// In place: N_s[t] = F_s[t] + F_s[rc(t)]; windows[s] = the sum of N_s; cnt[kCompCntWindows] += it.
__global__ __launch_bounds__(kCompThreads) void comp_fold_kernel(uint32_t *__restrict__ F, uint64_t n_seqs, int64_t *__restrict__ windows,
                                                                 unsigned long long *cnt)
{
    __shared__ long long part[kCompThreads / 64];
    const uint32_t t = threadIdx.x;
    for (uint64_t s = blockIdx.x; s < n_seqs; s += gridDim.x) {
        uint32_t *row = F + s * kCompBins;
        const uint32_t v = row[t] + row[comp_rc(t)];
        __syncthreads();                                // every read of the row, and of part[], before a write
        row[t] = v;
        long long x = (long long)v;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
        if ((t & 63) == 0) part[t >> 6] = x;
        __syncthreads();
        if (t == 0) {
            long long sum = 0;
            for (int w = 0; w < kCompThreads / 64; w++) sum += part[w];
            windows[s] = sum;
            if (sum) atomicAdd(&cnt[kCompCntWindows], (unsigned long long)sum);
        }
    }
}

// C[row][t] += N[order[i]][t] over the contigs of every piece.
__global__ __launch_bounds__(kCompThreads) void comp_train_kernel(const uint32_t *__restrict__ N, const uint32_t *__restrict__ order,
                                                                  const CompWork *__restrict__ work, uint64_t n_work,
                                                                  unsigned long long *C)
{
    for (uint64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        const CompWork k = work[w];
        unsigned long long acc = 0;
#pragma unroll 4
        for (uint32_t i = 0; i < k.count; i++) acc += N[(uint64_t)order[k.first + i] * kCompBins + threadIdx.x];
        if (acc) atomicAdd(&C[(uint64_t)k.row * kCompBins + threadIdx.x], acc);
    }
}

// S[s][m] = sum_t N[s][t] * W[m][t] for m = 0 .. M (W has M + 1 rows, the background last), rules 7 and 8 into cls[s].
// S: the matrix [n_seqs][M + 1], or null when it is not kept.
__global__ __launch_bounds__(kCompThreads) void comp_score_kernel(const uint32_t *__restrict__ N, const int64_t *__restrict__ windows,
                                                                  const int64_t *__restrict__ offsets, const int32_t *__restrict__ labels,
                                                                  uint64_t n_seqs, const int32_t *__restrict__ W,
                                                                  const int32_t *__restrict__ model_labels, uint32_t M, CompDecide prm,
                                                                  kg_comp_class *__restrict__ cls, int64_t *__restrict__ S,
                                                                  unsigned long long *cnt)
{
    __shared__ __attribute__((aligned(16))) int32_t tile[kCompScoreTile * kCompBins];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kCompScoreSeqs; base < n_seqs; base += (uint64_t)gridDim.x * kCompScoreSeqs) {
        const uint64_t s = base + wave;
        const bool have = s < n_seqs;
        uint4 n = make_uint4(0, 0, 0, 0);
        if (have) n = reinterpret_cast<const uint4 *>(N + s * kCompBins)[lane];
        long long best_v = 0, second_v = 0;
        uint32_t best_m = 0xFFFFFFFFu, second_m = 0xFFFFFFFFu;             // none yet
        for (uint32_t m0 = 0; m0 <= M; m0 += kCompScoreTile) {
            const uint32_t nm = M + 1 - m0 < (uint32_t)kCompScoreTile ? M + 1 - m0 : (uint32_t)kCompScoreTile;
            __syncthreads();                            // the reads of the tile before
            for (uint32_t i = threadIdx.x; i < nm * (kCompBins / 4); i += kCompThreads)
                reinterpret_cast<int4 *>(tile)[i] = reinterpret_cast<const int4 *>(W + (uint64_t)m0 * kCompBins)[i];
            __syncthreads();
            if (have) {
                for (uint32_t j = 0; j < nm; j++) {
                    const int4 w = reinterpret_cast<const int4 *>(tile)[j * (kCompBins / 4) + lane];
                    long long v = (long long)n.x * w.x + (long long)n.y * w.y + (long long)n.z * w.z + (long long)n.w * w.w;
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
                    const uint32_t m = m0 + j;
                    // rule 7 with m ascending: only a larger score moves an earlier row down
                    if (best_m == 0xFFFFFFFFu || v > best_v) {
                        second_v = best_v; second_m = best_m;
                        best_v = v; best_m = m;
                    } else if (second_m == 0xFFFFFFFFu || v > second_v) {
                        second_v = v; second_m = m;
                    }
                    if (S && lane == 0) S[s * ((uint64_t)M + 1) + m] = v;
                }
            }
        }
        if (have && lane == 0) {
            kg_comp_class c;
            c.label = labels[s];
            c.windows = windows[s];
            c.score_best = best_v;
            if (M == 0) {                               // only the background
                c.best = c.second = -1;
                c.score_second = best_v;
                c.decided = 0;
            } else {
                c.best = best_m < M ? model_labels[best_m] : -1;
                c.second = second_m < M ? model_labels[second_m] : -1;
                c.score_second = second_v;
                c.decided = (offsets[s + 1] - offsets[s] >= (int64_t)prm.min_len && best_m < M &&
                             best_v - second_v >= (long long)prm.min_margin) ? 1 : 0;
            }
            cls[s] = c;
            if (c.decided) {
                atomicAdd(&cnt[kCompCntDecided], 1ull);
                if (c.label < 0) atomicAdd(&cnt[kCompCntUnlabelled], 1ull);
                else if (c.best != c.label) atomicAdd(&cnt[kCompCntConflicts], 1ull);
            }
        }
    }
}

}  // namespace kg
