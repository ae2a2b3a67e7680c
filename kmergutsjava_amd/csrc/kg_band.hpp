// kg_band.hpp -- device side of kg_proteins_align_banded and of the alignment step of kg_proteins_search_banded
// (include/kmerguts_hip.h states the rule): kg_align.hpp's local alignment over the cells of a band around one diagonal per pair.
// Integers only.
//
//   align_band_kernel   one wave per pair, pairs handed out through a counter in descending order of their band cells (the host
//                       orders them), exactly as align_pairs_kernel hands its pairs out
//
// The rule.  Cell (i, j) of pair (a, b) with diagonal g and half-width W is in the band iff |(i - j) - g| <= W.  A cell outside
// the band has H = 0, as a cell outside the matrix has; E, F, the maximum and its tie rule are kg_align.hpp's.
// The wave is align_pairs_kernel's with its column range moved.  Lane l owns row i0 + l of a 64-row stripe.  The stripe's window
// is the columns c_lo = max(0, i0 - g - W) .. c_hi = min(m - 1, (the stripe's last row) - g + W): every in-band cell of its rows
// lies in it.  At step t lane l stands in column j = c_lo + t - l, so a stripe takes c_hi - c_lo + 64 <= 2 W + 127 steps whatever m
// is.  H-up, F-up and b's residue come down the lanes by DPP; the score byte is read from the LDS table one step early.  Only the
// stripes that hold a row with an in-band column are walked: rows max(0, g - W) .. min(n - 1, m - 1 + g + W).
// The carry.  Lane 63 stores (H, F) of its in-band cells at slot j - c_lo of the LDS carry: at most 2 W + 64 slots, so no pair
// needs the device-memory carry of align_pairs_kernel<true>.  The next stripe reads column j at slot j - (the window start of the
// stripe before), and only where row i0 - 1 has written: its in-band columns p_lo .. p_hi.  Every other column of that row is
// outside the band and reads as (0, kAlignNeg) -- never what an earlier stripe or an earlier pair of the workgroup left in LDS.
// The next window starts at or right of this one, so a slot is overwritten only after its column has been read (the reads of a
// 64-column chunk stand in front of the chunk's steps, in program order of the one wave).
// The diagonal of lane 0's first cell, H[i0 - 1][c_lo - 1], is the one value of row i0 - 1 left of the window that can be in the
// band (it is when the window is not clipped at column 0): it is read from the carry in front of the stripe.  For every other
// lane the cell up and left of its first column is outside the band: 0.
#pragma once

#include "kg_align.hpp"

namespace kg {

constexpr int kBandMax = 256;                           // KG_BAND_MAX: the largest half-width W
constexpr int kBandCarryCols = 2 * kBandMax + kWave;    // columns of one stripe's window at most: the carry's slots
constexpr int kBandDiagCap = 1 << 25;                   // |g| above this misses every matrix (n, m < 2^24): clamped, so that g +- W fits
static_assert(kBandCarryCols <= kAlignLdsCols, "the band's carry is no larger than align_pairs_kernel<false>'s");

// the cells that count against max_cells: min(n m, min(n, m) (2 W + 1))
__host__ __device__ constexpr int64_t band_cells(int64_t n, int64_t m, int64_t band)
{
    const int64_t full = n * m, strip = (n < m ? n : m) * (2 * band + 1);
    return full < strip ? full : strip;
}

// One workgroup = one wave.  order[k] = the k-th pair to hand out; *counter hands them out.  pair p = (pairs[2p], pairs[2p + 1])
// with diagonal diags[p] -> out[p].  band = W in 0 .. kBandMax.
__global__ __launch_bounds__(kWave) void align_band_kernel(const uint8_t *__restrict__ seq, const int64_t *__restrict__ off,
                                                           const int32_t *__restrict__ pairs, const int32_t *__restrict__ diags,
                                                           const uint32_t *__restrict__ order, uint32_t n_order,
                                                           unsigned int *__restrict__ counter, const int8_t *__restrict__ matrix,
                                                           int gap_open, int gap_extend, int64_t max_cells, int band,
                                                           AlignRec *__restrict__ out)
{
    __shared__ int8_t table[21 * kAlignRowStride];
    __shared__ int2 lds_carry[kBandCarryCols];
    const int lane = (int)threadIdx.x;
    for (int k = lane; k < 21 * 21; k += kWave) table[(k / 21) * kAlignRowStride + k % 21] = matrix ? matrix[k] : kBlosum62[k];
    __syncthreads();

    // One exit and one latch, only wave-uniform branches on the way round: see align_pairs_kernel.
    for (uint32_t k = align_next_pair(counter, lane); k < n_order; k = align_next_pair(counter, lane)) {
        const uint32_t p = order[k];
        const int32_t pa = pairs[2 * (size_t)p], pb = pairs[2 * (size_t)p + 1];
        const int64_t at_a = off[pa], at_b = off[pb];
        const int n = (int)(off[pa + 1] - at_a), m = (int)(off[pb + 1] - at_b);
        const int g = __builtin_amdgcn_readfirstlane(min(max(diags[p], -kBandDiagCap), kBandDiagCap));
        const int self_a = align_self(seq, at_a, n, table, lane), self_b = align_self(seq, at_b, m, table, lane);
        const bool skip = band_cells(n, m, band) > max_cells;
        int run_h = 0, run_i = -1, run_j = -1;          // the lane's best over its rows
        const int r_lo = max(0, g - band), r_hi = min(n - 1, m - 1 + g + band);     // the rows that have an in-band column (m > 0)
        const int i_start = r_lo & ~(kWave - 1);
        for (int i0 = i_start; i0 <= r_hi && r_lo <= r_hi && m > 0 && !skip; i0 += kWave) {
            const int i = i0 + lane;
            const int c_lo = max(0, i0 - g - band), c_hi = min(m - 1, min(i0 + kWave - 1, n - 1) - g + band);       // the window
            const int steps = c_hi - c_lo + kWave;      // lane 63 reaches column c_hi at step c_hi - c_lo + 63
            const bool carried = i0 > i_start, last = i0 + kWave > r_hi;
            // what the stripe before left: row i0 - 1's in-band columns, at slots counted from that stripe's window start
            const int p_lo = max(0, i0 - 1 - g - band), p_hi = min(m - 1, i0 - 1 - g + band);
            const int c_lo_prev = max(0, i0 - kWave - g - band);
            // this row's in-band columns
            const int lo = max(0, i - g - band), hi = min(m - 1, i - g + band);
            const bool row = i < n && hi >= lo;
            const unsigned width = row ? (unsigned)(hi - lo) : 0u;
            const int row_base = (i < n ? (int)aa_code_of_rt((char)seq[at_a + i]) : 20) * kAlignRowStride;
            int h_left = 0, e = kAlignNeg;              // this row, the column before
            int h_cur = 0, f_cur = kAlignNeg;           // what this lane made in the step before (lane l + 1 reads it)
            int h_diag = 0;                             // the H-up of the step before
            if (carried && c_lo - 1 >= p_lo && c_lo - 1 <= p_hi) {                 // (wave-uniform: one address, lane 0 keeps it)
                const int up_left = lds_carry[c_lo - 1 - c_lo_prev].x;
                h_diag = lane == 0 ? up_left : 0;
            }
            int best_h = 0, best_j = -1;
            int res = lane == 0 && c_lo < m ? (int)aa_code_of_rt((char)seq[at_b + c_lo]) : 20;
            int s_next = (int)table[row_base + res];
            for (int t0 = 0; t0 < steps; t0 += kWave) {
                // the chunk: the carry of columns c_lo + t0 + l, and b's residues ONE column ahead (lane 0 takes the next step's)
                const int col = c_lo + t0 + lane;
                const int chunk_res = col + 1 < m ? (int)aa_code_of_rt((char)seq[at_b + col + 1]) : 20;
                int chunk_h = 0, chunk_f = kAlignNeg;
                if (carried && col >= p_lo && col <= p_hi) {
                    const int2 c = lds_carry[col - c_lo_prev];
                    chunk_h = c.x; chunk_f = c.y;
                }
                const int kmax = steps - t0 < kWave ? steps - t0 : kWave;
                for (int q = 0; q < kmax; q++) {
                    const int j = c_lo + t0 + q - lane;
                    const int s_now = s_next;
                    const int res_next = align_from_prev_lane(__builtin_amdgcn_readlane(chunk_res, q), res);
                    s_next = (int)table[row_base + res_next];           // (issued a step early: off the recurrence's chain)
                    // row i - 1, column j: from lane l - 1, lane 0 from the carry
                    const int h_up = align_from_prev_lane(__builtin_amdgcn_readlane(chunk_h, q), h_cur);
                    const int f_up = align_from_prev_lane(__builtin_amdgcn_readlane(chunk_f, q), f_cur);
                    e = max(e, h_left - gap_open) - gap_extend;
                    const int f = max(f_up, h_up - gap_open) - gap_extend;
                    int h = max(max(0, h_diag + s_now), max(e, f));
                    const bool inside = row && (unsigned)(j - lo) <= width;        // in the matrix and in the band
                    h = inside ? h : 0;
                    if (h > best_h) { best_h = h; best_j = j; }
                    if (!last && lane == kWave - 1 && inside) lds_carry[t0 + q - (kWave - 1)] = make_int2(h, f);     // slot j - c_lo
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

}  // namespace kg
