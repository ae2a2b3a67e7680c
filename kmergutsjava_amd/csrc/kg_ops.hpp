// kg_ops.hpp -- the alignments themselves: the columns trace_columns_kernel (kg_trace.hpp) staged, run-length encoded into ops
// (include/kmerguts_hip.h states the rule: one uint32_t an op, len << 4 | code, BAM's codes, in alignment order).  Integers only.
//
//   ops_starts_kernel   the 32-bit prefix sum of the records' op counts and its exact total -> op_start[0..n], int64
//   ops_fill_kernel     one wave per record: the record's columns in alignment order, 64 at a time, -> its ops
//
// Fill.  A traced record has columns = (end_a - start_a + 1) + gap_cols_a columns (the header's formula); alignment column p is
// walk column columns - 1 - p, two bits of the record's staging words.  Lane l reads column p0 + l and maps its kind for the
// mode; a lane whose kind differs from the lane below (lane 0: from the chunk before, the first column: from nothing) is a run
// start, and the wave ballots the starts.  The lane at run start number s >= 1 of the record writes run s - 1, which ended
// there: its kind is the lane below's, its length the distance to the start before, which is the highest start below the lane in
// this ballot or the one carried from an earlier chunk.  The last run is closed behind the loop.  Every store is bounded by
// op_start[r + 1], and a record whose runs are not n_ops[r], or whose columns do not fit its staging words, sets kTraceErrOps:
// never a store or a load out of range.
#pragma once

#include "kg_trace.hpp"

namespace kg {

constexpr unsigned kTraceErrOps = 8u;                   // error bit: a record's runs and its counted ops differ
constexpr int kOpsThreads = 256;                        // ops_fill_kernel: four records a workgroup
constexpr int kOpM = 0, kOpI = 1, kOpD = 2, kOpEq = 7, kOpX = 8;        // BAM's codes

__global__ __launch_bounds__(256) void ops_starts_kernel(const uint32_t *__restrict__ x, uint64_t n, const uint64_t *__restrict__ total,
                                                         int64_t *__restrict__ op_start)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * 256)
        op_start[i] = i < n ? (int64_t)x[i] : (int64_t)*total;
}

// the op code of a staged column kind (0 '=', 1 'X', 2 (a_i, -), 3 (-, b_j))
__device__ __forceinline__ int ops_code_of(int kind, int eqx)
{
    return kind == 2 ? kOpI : kind == 3 ? kOpD : !eqx ? kOpM : kind == 0 ? kOpEq : kOpX;
}

__global__ __launch_bounds__(kOpsThreads) void ops_fill_kernel(const TracePath *__restrict__ paths, const OpsRec *__restrict__ recs,
                                                               const uint32_t *__restrict__ stage, const uint32_t *__restrict__ n_ops,
                                                               const int64_t *__restrict__ op_start, uint64_t n, int eqx,
                                                               uint32_t *__restrict__ ops, unsigned int *__restrict__ err)
{
    const int lane = (int)threadIdx.x & (kWave - 1);
    const uint64_t waves = (uint64_t)gridDim.x * (kOpsThreads / kWave);
    for (uint64_t r = (uint64_t)blockIdx.x * (kOpsThreads / kWave) + threadIdx.x / kWave; r < n; r += waves) {
        const TracePath path = paths[r];
        const OpsRec rec = recs[r];
        const uint32_t want = n_ops[r];
        const int64_t base = op_start[r], limit = op_start[r + 1];
        const int64_t room = (int64_t)rec.end_a + rec.end_b + 1;                  // columns the staging words hold at most
        int64_t columns = path.status == 0 ? (int64_t)(rec.end_a - path.start_a + 1) + path.gap_cols_a : 0;
        const bool bad = path.status == 0 && (columns < 1 || columns > room);
        if (bad) columns = 0;
        const uint32_t *const st = stage + rec.stage_at;
        int64_t count = 0;                              // run starts so far
        int carry_start = 0, carry_code = -1;           // the open run: where it began and its op code (-1: no column yet)
        for (int p0 = 0; p0 < (int)columns; p0 += kWave) {
            const int p = p0 + lane;
            const bool valid = p < (int)columns;
            int code = -2;
            if (valid) {
                const int c = (int)columns - 1 - p;
                code = ops_code_of((int)(st[c / kTraceColsPerWord] >> (2 * (c & (kTraceColsPerWord - 1))) & 3u), eqx);
            }
            int below = __shfl_up(code, 1);
            if (lane == 0) below = carry_code;
            const bool start = valid && code != below;
            const uint64_t mask = __ballot(start);
            const uint64_t lower = mask & ((1ull << lane) - 1);
            const int64_t s = count + __popcll(lower);  // this start's number in the record
            if (start && s >= 1) {
                const int before = lower ? p0 + 63 - __clzll((long long)lower) : carry_start;
                const int64_t at = base + s - 1;
                if (at < limit) ops[at] = (uint32_t)(p - before) << 4 | (uint32_t)below;
            }
            count += __popcll(mask);
            if (mask) carry_start = p0 + 63 - __clzll((long long)mask);
            const int last = (int)columns - 1 - p0 < kWave - 1 ? (int)columns - 1 - p0 : kWave - 1;
            carry_code = __shfl(code, last);
        }
        if (lane == 0) {
            if (count >= 1 && base + count - 1 < limit) ops[base + count - 1] = (uint32_t)((int)columns - carry_start) << 4 | (uint32_t)carry_code;
            if (bad || count != (int64_t)want || base + count != limit) atomicOr(err, kTraceErrOps);
        }
    }
}

}  // namespace kg
