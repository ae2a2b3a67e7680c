// kg_align.hpp -- device side of kg_proteins_align and of the alignment step of kg_proteins_cluster_aligned
// (include/kmerguts_hip.h states the rule): local alignment scores with affine gaps, no traceback.  Integers only.
//
//   1. align_pairs_kernel<kLong>  one wave per pair, pairs handed out through a counter in descending order of their cells (the
//                                 host orders them), so that one long pair starts first and does not end the launch alone
//   2. align_cut_kernel           per link that passed the 8-mer tests: the ratio test, the 32-byte edge record, kClusterNoEdge
//                                 over a cut link, best / shared of the member over the kept ones, the counts
//
// The wave.  Rows are a's residues, columns b's.  Lane l owns row i0 + l of a 64-row stripe and at step t stands in column
// j = t - l: the wave walks an anti-diagonal, and what lane l needs from row i - 1 at column j is what lane l - 1 made one step
// earlier.  H-left and E stay in the lane's registers; H-up and F-up come from lane l - 1 by one DPP move each (wave_shr:1,
// no LDS), and H-diagonal is the H-up of the step before.  b's residues are read once per stripe, 64 at a time (lane l
// loads column t0 + 1 + l: one ahead), handed to lane 0 one per step by a v_readlane and passed down the lanes by a third DPP move.  The
// stripe's last row, (H, F) per column, is written by lane 63 and read by the next stripe 64 columns at a time, ahead of
// the writes: in LDS for b of at most kAlignLdsCols residues (kLong = false), else in a slab of device memory of the
// workgroup's own (kLong = true).  No barrier and no atomic in the loop.
// The substitution score is one byte read from a 21 x 32 LDS table at (row of a_i) + code of b_j: the row base is fixed per
// stripe, and the read of step t + 1 is issued in step t (the residue is known one step ahead), so its latency is off
// the recurrence's chain.
// A cell outside the matrix (j < 0: the lane has not started; j >= m or i >= n: it is done) has its H forced to 0: with
// H = 0 there, E and F of the cells behind it are exactly the boundary's, and such a cell never is the maximum.
// Each lane keeps the first maximum of its row (strictly greater: the smallest j), merges it per stripe into the lane's
// running one (strictly greater: the smallest i among the lane's rows), and the wave reduces with the total order
// (score, then -i, then -j): the result depends on nothing else.
#pragma once

#include "kg_device.hpp"
#include "kg_cluster.hpp"

namespace kg {

constexpr int kAlignLdsCols = 1024;                 // b up to this length keeps the stripe carry in LDS (8 bytes a column)
constexpr int kAlignRowStride = 32;                 // bytes per row of the LDS score table
constexpr int kAlignNeg = -(1 << 30);               // -infinity: no recurrence step goes below it (gap costs are capped at 2^29 each)
constexpr int kAlignGapCap = 1 << 29;               // a gap that costs this much never pays: every H is below 2^28
constexpr uint32_t kAlignMaxLen = 1u << 24;         // len_p below this: 16 * 2^24 < 2^31

// the built-in scores: BLOSUM62 in code order (ACDEFGHIKLMNPQRSTVWY, then "everything else" = -1)
__constant__ int8_t kBlosum62[21 * 21] = {
     4,  0, -2, -1, -2,  0, -2, -1, -1, -1, -1, -2, -1, -1, -1,  1,  0,  0, -3, -2, -1,   // A
     0,  9, -3, -4, -2, -3, -3, -1, -3, -1, -1, -3, -3, -3, -3, -1, -1, -1, -2, -2, -1,   // C
    -2, -3,  6,  2, -3, -1, -1, -3, -1, -4, -3,  1, -1,  0, -2,  0, -1, -3, -4, -3, -1,   // D
    -1, -4,  2,  5, -3, -2,  0, -3,  1, -3, -2,  0, -1,  2,  0,  0, -1, -2, -3, -2, -1,   // E
    -2, -2, -3, -3,  6, -3, -1,  0, -3,  0,  0, -3, -4, -3, -3, -2, -2, -1,  1,  3, -1,   // F
     0, -3, -1, -2, -3,  6, -2, -4, -2, -4, -3,  0, -2, -2, -2,  0, -2, -3, -2, -3, -1,   // G
    -2, -3, -1,  0, -1, -2,  8, -3, -1, -3, -2,  1, -2,  0,  0, -1, -2, -3, -2,  2, -1,   // H
    -1, -1, -3, -3,  0, -4, -3,  4, -3,  2,  1, -3, -3, -3, -3, -2, -1,  3, -3, -1, -1,   // I
    -1, -3, -1,  1, -3, -2, -1, -3,  5, -2, -1,  0, -1,  1,  2,  0, -1, -2, -3, -2, -1,   // K
    -1, -1, -4, -3,  0, -4, -3,  2, -2,  4,  2, -3, -3, -2, -2, -2, -1,  1, -2, -1, -1,   // L
    -1, -1, -3, -2,  0, -3, -2,  1, -1,  2,  5, -2, -2,  0, -1, -1, -1,  1, -1, -1, -1,   // M
    -2, -3,  1,  0, -3,  0,  1, -3,  0, -3, -2,  6, -2,  0,  0,  1,  0, -3, -4, -2, -1,   // N
    -1, -3, -1, -1, -4, -2, -2, -3, -1, -3, -2, -2,  7, -1, -2, -1, -1, -2, -4, -3, -1,   // P
    -1, -3,  0,  2, -3, -2,  0, -3,  1, -2,  0,  0, -1,  5,  1,  0, -1, -2, -2, -1, -1,   // Q
    -1, -3, -2,  0, -3, -2,  0, -3,  2, -2, -1,  0, -2,  1,  5, -1, -1, -3, -3, -2, -1,   // R
     1, -1,  0,  0, -2,  0, -1, -2,  0, -2, -1,  1, -1,  0, -1,  4,  1, -2, -3, -2, -1,   // S
     0, -1, -1, -1, -2, -2, -2, -1, -1, -1, -1,  0, -1, -1, -1,  1,  5,  0, -2, -2, -1,   // T
     0, -1, -3, -2, -1, -3, -3,  3, -2,  1,  1, -3, -2, -2, -3, -2,  0,  4, -3, -1, -1,   // V
    -3, -2, -4, -3,  1, -2, -2, -3, -3, -2, -1, -4, -4, -2, -3, -3, -2, -3, 11,  2, -1,   // W
    -2, -2, -3, -2,  3, -3,  2, -1, -2, -1, -1, -2, -3, -1, -2, -2, -2, -1,  2,  7, -1,   // Y
    -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,   // everything else
};

struct AlignRec { int score, self_a, self_b, end_a, end_b, status; };   // kg_alignment

// lane l <- lane l - 1 of the wave (DPP wave_shr:1); lane 0 keeps `first`
__device__ __forceinline__ int align_from_prev_lane(int first, int v)
{
    return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xF, 0xF, false);
}

__device__ __forceinline__ int align_wave_sum(int v)
{
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// self(p): the diagonal scores of p's residues with code < 20, summed by the wave
__device__ __forceinline__ int align_self(const uint8_t *__restrict__ seq, int64_t at, int len, const int8_t *table, int lane)
{
    int sum = 0;
    for (int i = lane; i < len; i += kWave) {
        const int c = (int)aa_code_of_rt((char)seq[at + i]);
        sum += c < 20 ? (int)table[c * kAlignRowStride + c] : 0;
    }
    return align_wave_sum(sum);
}

// the next pair's place in the order: lane 0 asks the counter, every lane gets the answer
__device__ __forceinline__ uint32_t align_next_pair(unsigned int *counter, int lane)
{
    uint32_t k = 0;
    if (lane == 0) k = atomicAdd(counter, 1u);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
}

// One workgroup = one wave.  order[k] = the k-th pair to hand out; *counter hands them out; slab: kLong only, the carry of
// workgroup w is slab[w * slab_cols ..).  pairs / out: pair p = (pairs[2p], pairs[2p + 1]) -> out[p].
template <bool kLong>
__global__ __launch_bounds__(kWave) void align_pairs_kernel(const uint8_t *__restrict__ seq, const int64_t *__restrict__ off,
                                                            const int32_t *__restrict__ pairs, const uint32_t *__restrict__ order,
                                                            uint32_t n_order, unsigned int *__restrict__ counter,
                                                            const int8_t *__restrict__ matrix, int gap_open, int gap_extend,
                                                            int64_t max_cells, int2 *__restrict__ slab, uint64_t slab_cols,
                                                            AlignRec *__restrict__ out)
{
    __shared__ int8_t table[21 * kAlignRowStride];
    __shared__ int2 lds_carry[kLong ? 1 : kAlignLdsCols];
    const int lane = (int)threadIdx.x;
    for (int k = lane; k < 21 * 21; k += kWave) table[(k / 21) * kAlignRowStride + k % 21] = matrix ? matrix[k] : kBlosum62[k];
    __syncthreads();
    int2 *const carry_g = kLong ? slab + (uint64_t)blockIdx.x * slab_cols : nullptr;

    // One exit and one latch: the loop's only branches on the way round are wave-uniform, so that the wave stays whole for the
    // hand-out (a `continue` behind a lane-0 store gave lanes 1 .. 63 a back edge of their own, on which they read their
    // own k = 0 for ever).
    for (uint32_t k = align_next_pair(counter, lane); k < n_order; k = align_next_pair(counter, lane)) {
        const uint32_t p = order[k];
        const int32_t pa = pairs[2 * (size_t)p], pb = pairs[2 * (size_t)p + 1];
        const int64_t at_a = off[pa], at_b = off[pb];
        const int n = (int)(off[pa + 1] - at_a), m = (int)(off[pb + 1] - at_b);
        const int self_a = align_self(seq, at_a, n, table, lane), self_b = align_self(seq, at_b, m, table, lane);
        // not aligned: more cells than the cap (or, never sent here by the host, a b too long for this instantiation's carry)
        const bool skip = (int64_t)n * m > max_cells || (!kLong && m > kAlignLdsCols);
        int run_h = 0, run_i = -1, run_j = -1;          // the lane's best over its rows
        const int steps = m + kWave - 1;                // lane 63 reaches column m - 1 at step m + 62
        for (int i0 = 0; i0 < n && m > 0 && !skip; i0 += kWave) {
            const int i = i0 + lane;
            const bool row = i < n, first = i0 == 0, last = i0 + kWave >= n;
            const int row_base = (row ? (int)aa_code_of_rt((char)seq[at_a + i]) : 20) * kAlignRowStride;
            int h_left = 0, e = kAlignNeg;              // this row, the column before
            int h_cur = 0, f_cur = kAlignNeg;           // what this lane made in the step before (lane l + 1 reads it)
            int h_diag = 0;                             // the H-up of the step before
            int best_h = 0, best_j = -1;
            // the residue code of this step's column and its score against this row: lane 0 starts in column 0
            int res = lane == 0 ? (int)aa_code_of_rt((char)seq[at_b]) : 20;
            int s_next = (int)table[row_base + res];
            for (int t0 = 0; t0 < steps; t0 += kWave) {
                // the chunk: the carry of columns t0 + l, and b's residues ONE column ahead (lane 0 takes the next step's)
                const int col = t0 + lane;
                const int chunk_res = col + 1 < m ? (int)aa_code_of_rt((char)seq[at_b + col + 1]) : 20;
                int chunk_h = 0, chunk_f = kAlignNeg;
                if (!first && col < m) {
                    const int2 c = kLong ? carry_g[col] : lds_carry[col];
                    chunk_h = c.x; chunk_f = c.y;
                }
                const int kmax = steps - t0 < kWave ? steps - t0 : kWave;
                for (int q = 0; q < kmax; q++) {
                    const int j = t0 + q - lane;
                    const int s_now = s_next;
                    const int res_next = align_from_prev_lane(__builtin_amdgcn_readlane(chunk_res, q), res);
                    s_next = (int)table[row_base + res_next];           // (issued a step early: off the recurrence's chain)
                    // row i - 1, column j: from lane l - 1, lane 0 from the carry
                    const int h_up = align_from_prev_lane(__builtin_amdgcn_readlane(chunk_h, q), h_cur);
                    const int f_up = align_from_prev_lane(__builtin_amdgcn_readlane(chunk_f, q), f_cur);
                    e = max(e, h_left - gap_open) - gap_extend;
                    const int f = max(f_up, h_up - gap_open) - gap_extend;
                    int h = max(max(0, h_diag + s_now), max(e, f));
                    const bool inside = row && (unsigned)j < (unsigned)m;
                    h = inside ? h : 0;
                    if (h > best_h) { best_h = h; best_j = j; }
                    if (!last && lane == kWave - 1 && inside) {
                        if (kLong) carry_g[j] = make_int2(h, f); else lds_carry[j] = make_int2(h, f);
                    }
                    h_diag = h_up;
                    h_left = h; h_cur = h; f_cur = f;
                    res = res_next;
                }
            }
            if (row && best_h > run_h) { run_h = best_h; run_i = i; run_j = best_j; }
        }
        // the total order: score, then the smallest i, then the smallest j
        int top = run_h;
        for (int d = kWave / 2; d > 0; d >>= 1) top = max(top, __shfl_xor(top, d));
        unsigned long long key = run_h == top && top > 0 ? ((unsigned long long)(uint32_t)run_i << 32) | (uint32_t)run_j : ~0ull;
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const unsigned long long o = __shfl_xor(key, d);
            key = o < key ? o : key;
        }
        const bool have = top > 0 && !skip;
        const AlignRec rec{skip ? -1 : have ? top : 0, self_a, self_b, have ? (int)(key >> 32) : -1, have ? (int)(uint32_t)key : -1, skip ? 1 : 0};
        if (lane == 0) out[p] = rec;
        __builtin_amdgcn_wave_barrier();                // the lanes meet again here, in front of the hand-out
    }
}

// Passing link k = (member, centre) with its alignment aln[k], its shared count and its place ridx[k] among the distinct links.
// kept iff skipped, or score >= 1 and 100 score >= min_ratio_pct ref (int64); a cut link's edge becomes kClusterNoEdge; best[m] =
// max of (s << 32 | ~c) over the kept; words[kClusterEdges] counts the kept, tally[0 / 1] the cut and the skipped.
__global__ __launch_bounds__(256) void align_cut_kernel(const int32_t *__restrict__ pairs, const AlignRec *__restrict__ aln,
                                                        const int32_t *__restrict__ shared, const uint32_t *__restrict__ ridx, uint64_t n,
                                                        int64_t min_ratio_pct, int ref_member, uint64_t *__restrict__ edge,
                                                        unsigned long long *__restrict__ best, unsigned long long *__restrict__ words,
                                                        unsigned long long *__restrict__ tally, int4 *__restrict__ rec)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false, cut = false, skipped = false;
    if (k < n) {
        const AlignRec a = aln[k];
        const int m = pairs[2 * k], c = pairs[2 * k + 1], s = shared[k];
        const int ref = ref_member ? a.self_a : max(a.self_a, a.self_b);
        skipped = a.status != 0;
        keep = skipped || (a.score >= 1 && 100ll * a.score >= min_ratio_pct * (int64_t)ref);
        cut = !keep;
        if (keep) atomicMax(&best[m], ((unsigned long long)(uint32_t)s << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)c));
        else edge[ridx[k]] = kClusterNoEdge;
        rec[2 * k] = make_int4(m, c, s, a.score);
        rec[2 * k + 1] = make_int4(ref, a.end_a, a.end_b, skipped ? 2 : cut ? 1 : 0);
    }
    const unsigned long long mk = __ballot(keep), mc = __ballot(cut), ms = __ballot(skipped);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (mk) atomicAdd(&words[kClusterEdges], (unsigned long long)__popcll(mk));
        if (mc) atomicAdd(&tally[0], (unsigned long long)__popcll(mc));
        if (ms) atomicAdd(&tally[1], (unsigned long long)__popcll(ms));
    }
}

}  // namespace kg
