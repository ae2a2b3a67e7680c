// kg_trace.hpp -- device side of kg_proteins_align_paths and kg_proteins_search_paths (include/kmerguts_hip.h states the rule):
// the second half of the local alignment.  For a pair whose end cell the alignment pass (kg_align.hpp) has found, the recurrence
// runs again over the prefix box that ends in that cell, keeps four direction bits per cell in device memory, and the same wave
// walks back from the end cell and writes one 32-byte path record.  Integers only.
//
//   trace_pairs_kernel<kLong>     one wave per pair, pairs handed out through a counter in descending order of their box cells
//                                 (the host orders them), exactly as align_pairs_kernel hands its pairs out
//   trace_columns_kernel<kLong>   the same pass with the walk's columns recorded: two bits a column into the job's staging words,
//                                 and the record's op count (kg_ops.hpp turns the staged columns into ops)
//
//   trace_band_kernel<kLong>, trace_band_columns_kernel<kLong>   the two under a band (kg_band.hpp): the cells of the box outside
//                                 the band of the job's diagonal have H = 0
//
// All are instantiations of trace_pairs_body; the recording is compiled out of trace_pairs_kernel, the band out of both.
// Forward.  The wave is kg_align.hpp's: lane l owns row i0 + l of a 64-row stripe and stands in column j = t - l at step t, H-up,
// F-up and the residue come down the lanes by DPP, the stripe's last row is carried in LDS (kLong = false: box columns up to
// kAlignLdsCols) or in a slab of device memory (kLong = true).  Each cell adds four bits: the source of H (0 none: H = 0,
// 1 diagonal, 2 E, 3 F, in that order of preference), "E opened here" (E[i][j] = H[i][j-1] - open - ext, preferred to an extension)
// and "F opened here".  A lane packs kTraceCellsPerWord consecutive steps into one dword and stores it at
// [stripe][t / 8][lane]: every store instruction of the wave writes one contiguous 256-byte line.  The last partial word of a
// stripe is flushed behind the loop, so every word of the pair's stripes is written before the walk reads it: nothing depends
// on what the slab held before, and a workgroup's next pair reuses the slab without clearing.
// Walk.  Wave-uniform: every lane keeps the same (row, column, state).  Within a stripe every move lowers t = j + lane by 1 or
// 2, so the word blocks are consumed in descending order: one coalesced load (each lane loads the word it wrote itself) serves
// at least four moves, and the block below is loaded together with the current one.  The current row's word comes by
// v_readlane, a_i's code the same way from the lanes' row codes, b's codes 64 columns at a time.  Going up from lane 0 enters
// lane 63 of the stripe above.  The loop is bounded by (end_a + 1) + (end_b + 1) moves; a walk that does not end within them, a gap that reaches a cell
// with H = 0 or the boundary, a box whose end cell does not reproduce the score, and a pair that does not fit the workgroup's
// slab set a bit of the launches' error word (the host turns it into KG_ERR_DEVICE), never a spin and never a store outside the slab.
// Columns (kCols).  Column c of the walk (c = 0 is the alignment's last column) is two bits, 0 '=', 1 'X', 2 (a_i, -), 3 (-, b_j),
// at bits 2 * (c % 16) of staging word c / 16.  Lane (c / 16) % 64 gathers that word in a vector register, so the walk's scalar
// state grows by the column count alone, and the wave stores 64 words (1024 columns) with one coalesced instruction; the words
// of the last, partial block follow behind the loop.  A walk has at most end_a + end_b + 1 columns and the job's staging region
// has ceil of that over 16 words (the host lays the regions out in hand-out order): a column past it is a walk error, not a store.
// The op count is the number of kind changes, '=' and 'X' being one kind unless eqx is set; it is kept as the walk's other
// counts are and is 0 for a record without a path.
#pragma once

#include <type_traits>

#include "kg_align.hpp"

namespace kg {

constexpr int kTraceCellBits = 4;                       // source of H (2 bits), E opened here, F opened here
constexpr int kTraceCellsPerWord = 8;                   // steps a lane packs into one dword
constexpr unsigned kTraceErrScore = 1u;                 // error bits: the box's end cell does not reproduce the score
constexpr unsigned kTraceErrWalk = 2u;                  //       the walk left the rule (bound, gap into H = 0, boundary)
constexpr unsigned kTraceErrSlab = 4u;                  //       a traced pair does not fit the workgroup's slab

// One pair to hand out: the proteins, what the alignment pass found (score 0: no path is asked for) and the record's place
struct TraceJob { int a, b, score, end_a, end_b, slot; };
struct TraceBandJob { int a, b, score, end_a, end_b, slot, diag, band; };      // the same under a band: diagonal g and half-width W
// kg_ops.hpp / trace_columns_kernel: where record `slot`'s staging words begin, and its end cell (in record order)
struct OpsRec { uint64_t stage_at; int end_a, end_b; };
// what the recording needs beyond the plain pass, behind one pointer: trace_pairs_kernel<true> leaves two scalar registers free,
// so the kernel reads these where it uses them (at a block's store and at a record's end), not at its entry.
// Record `slot`'s staging words are stage[recs[slot].stage_at ..), its op count -> n_ops[slot]; eqx: '=' and 'X' are two kinds.
struct TraceOpsArgs { const OpsRec *recs; uint32_t *stage; uint32_t *n_ops; int eqx; };
constexpr int kTraceColsPerWord = 16;                   // columns of the walk in one staging word
__host__ __device__ constexpr uint64_t trace_stage_words(uint64_t na, uint64_t mb)      // of a traced box: na + mb - 1 columns at most
{
    return (na + mb - 1 + kTraceColsPerWord - 1) / kTraceColsPerWord;
}
constexpr int kTraceWords = 3;                          // the launches' words: the two hand-out counters, then the error bits
struct TracePath { int start_a, start_b, identical, positive, gap_opens, gap_cols_a, gap_cols_b, status; };   // kg_alignment_path

// direction words of one stripe of a box with mb columns: one per lane and eight steps, mb + 63 steps
__host__ __device__ constexpr uint64_t trace_stripe_words(uint64_t mb)
{
    return (mb + kWave - 1 + kTraceCellsPerWord - 1) / kTraceCellsPerWord * kWave;
}

// One workgroup = one wave.  jobs[k]: the k-th pair to hand out, record -> out[jobs[k].slot]; words: kTraceWords words, this
// instantiation's counter first or second.  dirs: workgroup w's direction words are dirs[w * dir_words ..); carry (kLong only):
// its stripe carry is carry[w * carry_cols ..).
// oa (kCols only): where the columns and the op counts go.
// kBand (kg_band.hpp's rule): a job carries its diagonal g and W, and a cell of the box with |(i - j) - g| > W has H = 0 as a cell
// outside the box has.  Nothing else differs.  The pass has no scalar register to spare (trace_pairs_kernel<true>), so what it
// keeps of the two values is lane-dependent and lives in vector registers: lane - g - W and lane - g + W.
template <bool kLong, bool kCols, bool kBand = false>
__device__ __forceinline__ void trace_pairs_body(const uint8_t *__restrict__ seq, const int64_t *__restrict__ off,
                                                 const std::conditional_t<kBand, TraceBandJob, TraceJob> *__restrict__ jobs, uint32_t n_jobs,
                                                 unsigned int *__restrict__ words,
                                                 const int8_t *__restrict__ matrix, int gap_open, int gap_extend, int64_t max_trace_cells,
                                                 uint32_t *__restrict__ dirs, uint64_t dir_words, int2 *__restrict__ carry, uint64_t carry_cols,
                                                 TracePath *__restrict__ out, const TraceOpsArgs *oa)
{
    __shared__ int8_t table[21 * kAlignRowStride];
    __shared__ int2 lds_carry[kLong ? 1 : kAlignLdsCols];
    const int lane = (int)threadIdx.x;
    for (int k = lane; k < 21 * 21; k += kWave) table[(k / 21) * kAlignRowStride + k % 21] = matrix ? matrix[k] : kBlosum62[k];
    __syncthreads();
    uint32_t *const my_dirs = dirs + (uint64_t)blockIdx.x * dir_words;
    int2 *const carry_g = kLong ? carry + (uint64_t)blockIdx.x * carry_cols : nullptr;
    unsigned int *const counter = words + (kLong ? 1 : 0);

    // One exit and one latch, only wave-uniform branches on the way round: see align_pairs_kernel.
    for (uint32_t k = align_next_pair(counter, lane); k < n_jobs; k = align_next_pair(counter, lane)) {
        const auto job = jobs[k];
        [[maybe_unused]] int band_first = 0, band_last = 0;    // kBand: lane - g - W and lane - g + W (|g| > 2^25 misses every box: clamped)
        if constexpr (kBand) {
            band_first = lane - min(max(job.diag, -(1 << 25)), 1 << 25) - job.band;
            band_last = band_first + 2 * job.band;
        }
        const int64_t at_a = off[job.a], at_b = off[job.b];
        const int n = (int)(off[job.a + 1] - at_a), m = (int)(off[job.b + 1] - at_b);
        const int score = __builtin_amdgcn_readfirstlane(job.score);
        const int na = __builtin_amdgcn_readfirstlane(job.end_a) + 1, mb = __builtin_amdgcn_readfirstlane(job.end_b) + 1;   // the box
        const bool want = score > 0 && na >= 1 && mb >= 1 && na <= n && mb <= m;
        const bool over = want && (int64_t)na * mb > max_trace_cells;
        const int steps = mb + kWave - 1;               // lane 63 reaches column mb - 1 at step mb + 62
        const uint32_t stripe_words = (uint32_t)trace_stripe_words((uint64_t)(mb > 0 ? mb : 0));      // (mb < 2^24: below 2^28)
        bool go = want && !over;
        unsigned bad = 0;
        if (go && ((uint64_t)((na + kWave - 1) / kWave) * stripe_words > dir_words || (kLong ? (uint64_t)mb > carry_cols : mb > kAlignLdsCols))) {
            bad = kTraceErrSlab;
            go = false;
        }

        // ---- forward: the recurrence over the box, four bits a cell ----
        int end_h = 0;
        for (int i0 = 0; i0 < na && go; i0 += kWave) {
            const int i = i0 + lane;
            const bool row = i < na, first = i0 == 0, last = i0 + kWave >= na;
            const int row_base = (row ? (int)aa_code_of_rt((char)seq[at_a + i]) : 20) * kAlignRowStride;
            uint32_t *const dst = my_dirs + (uint64_t)(i0 / kWave) * stripe_words + lane;
            [[maybe_unused]] int band_lo = 0;           // kBand: the row's in-band columns of the box are band_lo .. band_lo + band_width
            [[maybe_unused]] unsigned band_width = 0;
            if constexpr (kBand) {
                const int hi = min(mb - 1, i0 + band_last);
                band_lo = max(0, i0 + band_first);
                band_width = hi >= band_lo ? (unsigned)(hi - band_lo) : 0u;
                if (hi < band_lo) band_lo = kAlignNeg;  // no in-band column: j - band_lo is above every width
            }
            int h_left = 0, e = kAlignNeg;
            int h_cur = 0, f_cur = kAlignNeg;
            int h_diag = 0;
            uint32_t word = 0;
            int res = lane == 0 ? (int)aa_code_of_rt((char)seq[at_b]) : 20;
            int s_next = (int)table[row_base + res];
            for (int t0 = 0; t0 < steps; t0 += kWave) {
                const int col = t0 + lane;
                const int chunk_res = col + 1 < mb ? (int)aa_code_of_rt((char)seq[at_b + col + 1]) : 20;
                int chunk_h = 0, chunk_f = kAlignNeg;
                if (!first && col < mb) {
                    const int2 c = kLong ? carry_g[col] : lds_carry[col];
                    chunk_h = c.x; chunk_f = c.y;
                }
                const int kmax = steps - t0 < kWave ? steps - t0 : kWave;
                for (int q = 0; q < kmax; q++) {
                    const int j = t0 + q - lane;
                    const int s_now = s_next;
                    const int res_next = align_from_prev_lane(__builtin_amdgcn_readlane(chunk_res, q), res);
                    s_next = (int)table[row_base + res_next];
                    const int h_up = align_from_prev_lane(__builtin_amdgcn_readlane(chunk_h, q), h_cur);
                    const int f_up = align_from_prev_lane(__builtin_amdgcn_readlane(chunk_f, q), f_cur);
                    const int e_from_h = h_left - gap_open, f_from_h = h_up - gap_open;
                    const uint32_t e_open = e_from_h >= e ? 4u : 0u, f_open = f_from_h >= f_up ? 8u : 0u;      // a tie opens
                    e = max(e, e_from_h) - gap_extend;
                    const int f = max(f_up, f_from_h) - gap_extend;
                    const int d = h_diag + s_now;
                    int h = max(max(0, d), max(e, f));
                    // in_box: a cell of the box.  Lane 63 carries every one of them, so that the next stripe reads no column that this
                    // stripe has not written; under a band the ones outside it carry H = 0 and the F the recurrence gives them.
                    const bool in_box = row && (unsigned)j < (unsigned)mb;
                    bool inside = in_box;
                    if constexpr (kBand) inside = row && (unsigned)(j - band_lo) <= band_width;
                    h = inside ? h : 0;
                    const uint32_t src = h == 0 ? 0u : h == d ? 1u : h == e ? 2u : 3u;                          // diagonal, then E, then F
                    word |= (src | e_open | f_open) << (kTraceCellBits * (q & (kTraceCellsPerWord - 1)));
                    if ((q & (kTraceCellsPerWord - 1)) == kTraceCellsPerWord - 1) {                               // (t0 is a multiple of 8)
                        dst[(size_t)((t0 + q) / kTraceCellsPerWord) * kWave] = word;
                        word = 0;
                    }
                    if (inside && i == na - 1 && j == mb - 1) end_h = h;
                    if (!last && lane == kWave - 1 && in_box) {
                        if (kLong) carry_g[j] = make_int2(h, f); else lds_carry[j] = make_int2(h, f);
                    }
                    h_diag = h_up;
                    h_left = h; h_cur = h; f_cur = f;
                    res = res_next;
                }
            }
            if (steps % kTraceCellsPerWord) dst[(size_t)(steps / kTraceCellsPerWord) * kWave] = word;           // the last partial word
        }

        // ---- the walk: from the end cell in state H, every lane with the same (row, column, state) ----
        // The counts are kept by the lane of the current row (in vector registers: the walk's scalar state stays small) and
        // summed at the end.  The start is where the walk stopped: the cell itself behind a diagonal step to the boundary,
        // one down the diagonal when the step reached a cell with H = 0.
        int identical = 0, positive = 0, gap_opens = 0, gap_cols_a = 0, gap_cols_b = 0;
        [[maybe_unused]] int n_op = 0, n_op_eqx = 0;     // kind changes with '=' and 'X' as one kind, and apart
        int gi = na - 1, j = mb - 1;
        bool at_zero = false;
        if (go) {
            if (__builtin_amdgcn_readlane(end_h, (na - 1) & (kWave - 1)) != score) bad |= kTraceErrScore;
            int state = 0;                              // 0 H, 1 E, 2 F
            int kind = 3;                               // the column emitted last: 0 a residue pair (kCols: 4 when not identical), 1 (-, b_j), 2 (a_i, -), 3 none yet
            int ld_s = -1, ld_tb = -1, ld_bc = -1;      // what the lanes hold: stripe, word block, chunk of b
            uint32_t w = 0, w_below = 0;                // the lane's word of block ld_tb, and of the block below it
            int a_codes = 20, b_codes = 20;
            bool done = bad != 0;
            // At most (end_a + 1) + (end_b + 1) moves: every emitted column is one and lowers the row, the column or both.  An
            // iteration that emits nothing changes the state from H to E or F, and the next one emits: the loop cannot spin.
            int moves = na + mb;
            // The recording's state beside the walk's is two vector registers: the staging word the lane gathers and the second
            // count.  The column's number is the moves made; the kind before is `kind`, which here tells a residue pair that is
            // not identical (4) from one that is (0); the staging region's offset is read again at each of the rare stores.
            [[maybe_unused]] uint32_t cw = 0;
            // one emitted column (kCols), in front of its moves--: count a kind change, gather the two bits, store a full block.
            // code: the staged two bits; next: what `kind` becomes
            auto record = [&](int code, int next, int mine) {
                if constexpr (kCols) {
                    n_op += mine & (int)((next & 3) != (kind & 3));
                    n_op_eqx += mine & (int)(next != kind);
                    const int c = na + mb - moves;      // (a box has na + mb - 1 columns at most: the last move never emits)
                    if (moves >= 2) {
                        cw |= lane == ((c / kTraceColsPerWord) & (kWave - 1)) ? (uint32_t)code << (2 * (c & (kTraceColsPerWord - 1))) : 0u;
                        if ((c & (kTraceColsPerWord * kWave - 1)) == kTraceColsPerWord * kWave - 1) {
                            oa->stage[oa->recs[job.slot].stage_at + (size_t)(c / (kTraceColsPerWord * kWave)) * kWave + lane] = cw;
                            cw = 0;
                        }
                    } else {
                        bad |= kTraceErrWalk;
                    }
                }
            };
            for (; moves > 0 && !done;) {
                const int s = gi / kWave, r = gi & (kWave - 1), t = j + r, tb = t / kTraceCellsPerWord;
                const uint32_t *const src_w = my_dirs + (uint64_t)s * stripe_words + lane;
                if (s != ld_s) {
                    const int i = s * kWave + lane;
                    a_codes = i < na ? (int)aa_code_of_rt((char)seq[at_a + i]) : 20;
                }
                if (s == ld_s && tb == ld_tb - 1) {
                    w = w_below;
                    if (tb > 0) w_below = src_w[(size_t)(tb - 1) * kWave];
                } else if (s != ld_s || tb != ld_tb) {
                    w = src_w[(size_t)tb * kWave];
                    if (tb > 0) w_below = src_w[(size_t)(tb - 1) * kWave];
                }
                ld_s = s; ld_tb = tb;
                if (j / kWave != ld_bc) {
                    ld_bc = j / kWave;
                    const int col = ld_bc * kWave + lane;
                    b_codes = col < mb ? (int)aa_code_of_rt((char)seq[at_b + col]) : 20;
                }
                const uint32_t bits = ((uint32_t)__builtin_amdgcn_readlane((int)w, r) >> (kTraceCellBits * (t & (kTraceCellsPerWord - 1)))) & 15u;
                const int mine = lane == r;
                if (state == 0) {
                    const uint32_t src = bits & 3u;
                    if (src == 0) {                     // H = 0: the path began in the cell before, which a diagonal step left
                        if ((kind & 3) != 0) bad |= kTraceErrWalk;
                        at_zero = true;
                        done = true;
                    } else if (src == 1) {
                        const int ca = __builtin_amdgcn_readlane(a_codes, r), cb = __builtin_amdgcn_readlane(b_codes, j & (kWave - 1));
                        identical += mine & (int)(ca == cb && ca < 20);
                        positive += mine & (int)(table[ca * kAlignRowStride + cb] > 0);
                        const int same = (int)(ca == cb && ca < 20);
                        record(1 - same, 4 - 4 * same, mine);
                        kind = kCols ? 4 - 4 * same : 0;
                        moves--;
                        if (gi == 0 || j == 0) done = true;
                        else { gi--; j--; }
                    } else {
                        state = (int)src - 1;
                    }
                } else if (state == 1) {
                    gap_cols_a += mine;
                    gap_opens += mine & (int)(kind != 1);
                    record(3, 1, mine);
                    kind = 1;
                    moves--;
                    if (bits & 4u) state = 0;
                    if (j == 0) { bad |= kTraceErrWalk; done = true; }
                    else j--;
                } else {
                    gap_cols_b += mine;
                    gap_opens += mine & (int)(kind != 2);
                    record(2, 2, mine);
                    kind = 2;
                    moves--;
                    if (bits & 8u) state = 0;
                    if (gi == 0) { bad |= kTraceErrWalk; done = true; }
                    else gi--;
                }
            }
            if (!done) bad |= kTraceErrWalk;
            identical = align_wave_sum(identical); positive = align_wave_sum(positive); gap_opens = align_wave_sum(gap_opens);
            gap_cols_a = align_wave_sum(gap_cols_a); gap_cols_b = align_wave_sum(gap_cols_b);
            if constexpr (kCols) {
                n_op = align_wave_sum(oa->eqx ? n_op_eqx : n_op);
                // the last block's words: word sw of the record holds columns 16 sw .., and exists while 16 sw < n_cols < na + mb
                const int n_cols = na + mb - moves;
                const int sw = n_cols / (kTraceColsPerWord * kWave) * kWave + lane;
                if (sw * kTraceColsPerWord < n_cols && moves >= 1) oa->stage[oa->recs[job.slot].stage_at + sw] = cw;
            }
        }
        const int start_a = gi + (at_zero ? 1 : 0), start_b = j + (at_zero ? 1 : 0);
        const bool traced = go && bad == 0;
        const TracePath rec{traced ? start_a : -1, traced ? start_b : -1, traced ? identical : 0, traced ? positive : 0,
                            traced ? gap_opens : 0, traced ? gap_cols_a : 0, traced ? gap_cols_b : 0, !want ? 1 : over ? 2 : traced ? 0 : 1};
        if (lane == 0) {
            out[job.slot] = rec;
            if constexpr (kCols) oa->n_ops[job.slot] = traced ? (uint32_t)n_op : 0u;
            if (bad) atomicOr(words + kTraceWords - 1, bad);
        }
        __builtin_amdgcn_wave_barrier();                // the lanes meet again here, in front of the hand-out
    }
}

template <bool kLong>
__global__ __launch_bounds__(kWave) void trace_pairs_kernel(const uint8_t *__restrict__ seq, const int64_t *__restrict__ off,
                                                            const TraceJob *__restrict__ jobs, uint32_t n_jobs,
                                                            unsigned int *__restrict__ words, const int8_t *__restrict__ matrix,
                                                            int gap_open, int gap_extend, int64_t max_trace_cells,
                                                            uint32_t *__restrict__ dirs, uint64_t dir_words, int2 *__restrict__ carry,
                                                            uint64_t carry_cols, TracePath *__restrict__ out)
{
    trace_pairs_body<kLong, false>(seq, off, jobs, n_jobs, words, matrix, gap_open, gap_extend, max_trace_cells, dirs, dir_words, carry,
                                   carry_cols, out, nullptr);
}

template <bool kLong>
__global__ __launch_bounds__(kWave) void trace_columns_kernel(const uint8_t *__restrict__ seq, const int64_t *__restrict__ off,
                                                              const TraceJob *__restrict__ jobs, uint32_t n_jobs,
                                                              unsigned int *__restrict__ words, const int8_t *__restrict__ matrix,
                                                              int gap_open, int gap_extend, int64_t max_trace_cells,
                                                              uint32_t *__restrict__ dirs, uint64_t dir_words, int2 *__restrict__ carry,
                                                              uint64_t carry_cols, TracePath *__restrict__ out, const TraceOpsArgs *oa)
{
    trace_pairs_body<kLong, true>(seq, off, jobs, n_jobs, words, matrix, gap_open, gap_extend, max_trace_cells, dirs, dir_words, carry,
                                  carry_cols, out, oa);
}

// the same two passes under a band: kg_proteins_align_banded and kg_proteins_search_banded
template <bool kLong>
__global__ __launch_bounds__(kWave) void trace_band_kernel(const uint8_t *__restrict__ seq, const int64_t *__restrict__ off,
                                                           const TraceBandJob *__restrict__ jobs, uint32_t n_jobs,
                                                           unsigned int *__restrict__ words, const int8_t *__restrict__ matrix,
                                                           int gap_open, int gap_extend, int64_t max_trace_cells,
                                                           uint32_t *__restrict__ dirs, uint64_t dir_words, int2 *__restrict__ carry,
                                                           uint64_t carry_cols, TracePath *__restrict__ out)
{
    trace_pairs_body<kLong, false, true>(seq, off, jobs, n_jobs, words, matrix, gap_open, gap_extend, max_trace_cells, dirs, dir_words, carry,
                                         carry_cols, out, nullptr);
}

template <bool kLong>
__global__ __launch_bounds__(kWave) void trace_band_columns_kernel(const uint8_t *__restrict__ seq, const int64_t *__restrict__ off,
                                                                   const TraceBandJob *__restrict__ jobs, uint32_t n_jobs,
                                                                   unsigned int *__restrict__ words, const int8_t *__restrict__ matrix,
                                                                   int gap_open, int gap_extend, int64_t max_trace_cells,
                                                                   uint32_t *__restrict__ dirs, uint64_t dir_words, int2 *__restrict__ carry,
                                                                   uint64_t carry_cols, TracePath *__restrict__ out, const TraceOpsArgs *oa)
{
    trace_pairs_body<kLong, true, true>(seq, off, jobs, n_jobs, words, matrix, gap_open, gap_extend, max_trace_cells, dirs, dir_words, carry,
                                        carry_cols, out, oa);
}

}  // namespace kg
