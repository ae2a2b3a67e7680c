// kg_assign.hpp -- device side of kg_result_assign / kg_assign_calls (include/kmerguts_hip.h): the CALL records of an -a scan
// -> one kg_assignment per protein (the rule is stated in the header, next to the entry points).
//
//   1. assign_short_kernel     one lane per protein.  A protein with at most kAssignShort CALLs is grouped by that lane: for
//                              each CALL whose fI has not occurred before in the protein, one in-order pass over the rest sums
//                              S_f and W_f (W_f strictly in emission order).  Longer proteins are only flagged (flag, length).
//   2. prefix sums of the flags and lengths (the table build's prefix_sum) number the long proteins and place their CALLs;
//      assign_long_scatter_kernel lists them, deterministically (no atomics).
//   3. assign_long_keys_kernel one wave per long protein: key = (rank << 32) | (fI ^ 2^31), value = the CALL's index.
//   4. the stable LSD radix sort of kg_build.hpp: one protein's CALLs of one function become one run, in emission order.
//   5. assign_long_runs_kernel one lane per run head walks its run in order (S_f in int64, W_f by float adds in emission order),
//                              loading kAssignWalk items ahead, so that only a run's own length is serial.
//   6. assign_long_reduce_kernel one wave per long protein: top two of its runs by (S desc, W desc, f asc), T and the number
//                              of runs, merged across the wave with shuffles.
//
// A protein with 2 * 10^4 CALLs of distinct functions costs 2 * 10^4 sorted items and 2 * 10^4 one-item runs; a protein whose
// CALLs all name one function costs one run walked by one lane.  The only atomics are atomicMin on the error words, and they
// run only for bad input.
#pragma once

#include "kg_device.hpp"

namespace kg {

constexpr uint32_t kAssignShort = 16;   // CALLs a single lane groups on its own (quadratic in at most this many)
constexpr int kAssignWalk = 16;         // items a run walk loads ahead
constexpr unsigned long long kAssignNoErr = 0x7F7F7F7F7F7F7F7Full;   // the error words' "none" (a byte memset)

// error words: [0] first protein whose call_start decreases, [1] first protein with a negative count, [2] first protein whose
// S_best or T (or CALL count) is 2^31 or more
enum { kAssignErrOrder = 0, kAssignErrCount = 1, kAssignErrLimit = 2 };

struct AssignCand {
    int64_t s;
    float w;
    int32_t f;
};

__device__ inline AssignCand assign_none() { return AssignCand{INT64_MIN, 0.0f, -1}; }

// the ranking of the rule: larger S, then larger W, then smaller f
__device__ inline bool assign_better(const AssignCand &a, const AssignCand &b)
{
    return a.s > b.s || (a.s == b.s && (a.w > b.w || (a.w == b.w && a.f < b.f)));
}

__device__ inline void assign_push(AssignCand &best, AssignCand &second, const AssignCand &c)
{
    if (assign_better(c, best)) { second = best; best = c; }
    else if (assign_better(c, second)) second = c;
}

__device__ inline void assign_span(const int64_t *__restrict__ cs, uint64_t p, uint64_t n_calls, uint64_t *lo, uint64_t *hi,
                                   unsigned long long *err)
{
    const int64_t a = cs[p], b = cs[p + 1];
    if (b < a) atomicMin(&err[kAssignErrOrder], (unsigned long long)p);
    // clamped, so that a bad call_start never reads outside calls[] (the call fails with KG_ERR_ARG anyway)
    const uint64_t l = a < 0 ? 0 : ((uint64_t)a > n_calls ? n_calls : (uint64_t)a);
    const uint64_t h = b < (int64_t)l ? l : ((uint64_t)b > n_calls ? n_calls : (uint64_t)b);
    *lo = l;
    *hi = h;
}

__device__ inline int32_t assign_otu(const kg_otu *__restrict__ otu, uint64_t p)
{
    if (!otu) return -1;
    return otu[p].n > 0 ? otu[p].oI[0] : -1;
}

__device__ inline void assign_write(kg_assignment *__restrict__ out, uint64_t p, uint64_t n, int32_t nf, const AssignCand &best,
                                    const AssignCand &second, int64_t total, int32_t otu, int32_t min_score, int32_t min_share,
                                    unsigned long long *err)
{
    if (total >= (1ll << 31) || best.s >= (1ll << 31) || n >= (1ull << 31)) atomicMin(&err[kAssignErrLimit], (unsigned long long)p);
    kg_assignment a;
    const bool any = n > 0;
    a.fI = any ? best.f : -1;
    a.score = any ? (int32_t)best.s : 0;
    a.total = (int32_t)total;
    a.weighted = any ? best.w : 0.0f;
    a.assigned = (any && best.s >= (int64_t)min_score && 100 * best.s >= (int64_t)min_share * total) ? 1 : 0;
    a.n_calls = (int32_t)n;
    a.n_functions = nf;
    a.second_fi = nf > 1 ? second.f : -1;
    a.second_score = nf > 1 ? (int32_t)second.s : 0;
    a.otu = otu;
    out[p] = a;
}

__global__ __launch_bounds__(256) void assign_short_kernel(const kg_call *__restrict__ calls, uint64_t n_calls,
                                                           const int64_t *__restrict__ cs, uint64_t n_prot,
                                                           const kg_otu *__restrict__ otu, int32_t min_score, int32_t min_share,
                                                           kg_assignment *__restrict__ out, uint32_t *__restrict__ long_flag,
                                                           uint32_t *__restrict__ long_len, unsigned long long *err)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_prot) return;
    uint64_t lo, hi;
    assign_span(cs, p, n_calls, &lo, &hi, err);
    const uint64_t n = hi - lo;
    const bool is_long = n > kAssignShort;
    long_flag[p] = is_long ? 1u : 0u;
    long_len[p] = is_long ? (uint32_t)n : 0u;
    if (is_long) return;
    AssignCand best = assign_none(), second = assign_none();
    int64_t total = 0;
    int32_t nf = 0;
    for (uint64_t i = lo; i < hi; i++) {
        const int32_t f = calls[i].fI;
        const int32_t c = calls[i].count;
        if (c < 0) atomicMin(&err[kAssignErrCount], (unsigned long long)p);
        total += c;
        bool seen = false;
        for (uint64_t j = lo; j < i; j++) seen |= calls[j].fI == f;
        if (seen) continue;
        nf++;
        AssignCand cand{0, 0.0f, f};
        for (uint64_t j = i; j < hi; j++)
            if (calls[j].fI == f) {
                cand.s += calls[j].count;
                cand.w = __fadd_rn(cand.w, calls[j].weightedHits);
            }
        assign_push(best, second, cand);
    }
    assign_write(out, p, n, nf, best, second, total, assign_otu(otu, p), min_score, min_share, err);
}

// long protein r (rank = exclusive prefix sum of the flags) -> its index and the first sorted item of its CALLs
__global__ __launch_bounds__(256) void assign_long_scatter_kernel(const uint32_t *__restrict__ long_flag,
                                                                  const uint32_t *__restrict__ rank, const uint32_t *__restrict__ base,
                                                                  uint64_t n_prot, uint32_t *__restrict__ long_ids,
                                                                  uint32_t *__restrict__ long_base)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_prot || !long_flag[p]) return;
    long_ids[rank[p]] = (uint32_t)p;
    long_base[rank[p]] = base[p];
}

__global__ __launch_bounds__(256) void assign_long_keys_kernel(const kg_call *__restrict__ calls, uint64_t n_calls,
                                                               const int64_t *__restrict__ cs, const uint32_t *__restrict__ long_ids,
                                                               const uint32_t *__restrict__ long_base, uint32_t n_long,
                                                               uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                               unsigned long long *err)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / kWave);
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave; r < n_long; r += waves) {
        const uint64_t p = long_ids[r];
        uint64_t lo, hi;
        assign_span(cs, p, n_calls, &lo, &hi, err);
        const uint64_t base = long_base[r];
        for (uint64_t k = lane; k < hi - lo; k += kWave) {
            const uint64_t i = lo + k;
            if (calls[i].count < 0) atomicMin(&err[kAssignErrCount], (unsigned long long)p);
            keys[base + k] = (r << 32) | (uint64_t)((uint32_t)calls[i].fI ^ 0x80000000u);
            vals[base + k] = (uint32_t)i;
        }
    }
}

// run heads of the sorted (protein, fI) keys: S_f and W_f of the run, summed in the run's (= emission) order.  Other items get
// run_s = INT64_MIN.
__global__ __launch_bounds__(256) void assign_long_runs_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                               uint64_t n, const kg_call *__restrict__ calls,
                                                               int64_t *__restrict__ run_s, float *__restrict__ run_w)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    if (i > 0 && keys[i - 1] == key) {
        run_s[i] = INT64_MIN;
        return;
    }
    int64_t s = 0;
    float w = 0.0f;
    for (uint64_t j = i; j < n; j += kAssignWalk) {
        uint64_t kk[kAssignWalk];
        uint32_t vv[kAssignWalk];
#pragma unroll
        for (int u = 0; u < kAssignWalk; u++) {
            const uint64_t q = j + u;
            kk[u] = q < n ? keys[q] : ~0ull;
            vv[u] = q < n ? vals[q] : 0u;
        }
        int32_t cc[kAssignWalk];
        float ww[kAssignWalk];
#pragma unroll
        for (int u = 0; u < kAssignWalk; u++) {
            cc[u] = kk[u] == key ? calls[vv[u]].count : 0;
            ww[u] = kk[u] == key ? calls[vv[u]].weightedHits : 0.0f;
        }
        bool more = true;
#pragma unroll
        for (int u = 0; u < kAssignWalk; u++) {
            if (kk[u] == key) {             // sorted: once the key changes it never comes back
                s += cc[u];
                w = __fadd_rn(w, ww[u]);
            } else {
                more = false;
            }
        }
        if (!more) break;
    }
    run_s[i] = s;
    run_w[i] = w;
}

__device__ inline AssignCand assign_shfl(const AssignCand &c, int m)
{
    AssignCand o;
    o.s = __shfl_xor(c.s, m);
    o.w = __shfl_xor(c.w, m);
    o.f = __shfl_xor(c.f, m);
    return o;
}

__global__ __launch_bounds__(256) void assign_long_reduce_kernel(const uint64_t *__restrict__ keys, const int64_t *__restrict__ run_s,
                                                                 const float *__restrict__ run_w, const kg_call *__restrict__ calls,
                                                                 uint64_t n_calls, const int64_t *__restrict__ cs,
                                                                 const kg_otu *__restrict__ otu, const uint32_t *__restrict__ long_ids,
                                                                 const uint32_t *__restrict__ long_base, uint32_t n_long,
                                                                 int32_t min_score, int32_t min_share, kg_assignment *__restrict__ out,
                                                                 unsigned long long *err)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / kWave);
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave; r < n_long; r += waves) {
        const uint64_t p = long_ids[r];
        uint64_t lo, hi;
        assign_span(cs, p, n_calls, &lo, &hi, err);
        const uint64_t base = long_base[r], n = hi - lo;
        AssignCand best = assign_none(), second = assign_none();
        int64_t total = 0;
        int32_t nf = 0;
        for (uint64_t k = lane; k < n; k += kWave) {
            const int64_t s = run_s[base + k];
            if (s == INT64_MIN) continue;
            nf++;
            total += s;
            assign_push(best, second, AssignCand{s, run_w[base + k], (int32_t)((uint32_t)keys[base + k] ^ 0x80000000u)});
        }
        for (int m = kWave / 2; m >= 1; m >>= 1) {
            total += __shfl_xor(total, m);
            nf += __shfl_xor(nf, m);
            const AssignCand ob = assign_shfl(best, m), os = assign_shfl(second, m);
            // top two of {best, second, ob, os}, where best >= second and ob >= os
            if (assign_better(ob, best)) {
                second = assign_better(best, os) ? best : os;
                best = ob;
            } else if (assign_better(ob, second)) {
                second = ob;
            }
        }
        if (lane == 0) assign_write(out, p, n, nf, best, second, total, assign_otu(otu, p), min_score, min_share, err);
    }
}

}  // namespace kg
