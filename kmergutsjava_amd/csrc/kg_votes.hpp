// kg_votes.hpp -- device side of kg_result_otu_votes / kg_otu_votes_hits (include/kmerguts_hip.h): the hit, event and CALL records
// of a scan -> every (sequence, OTU) vote tally, one class record per sequence, the bins of the batch (the rule is stated in the
// header, next to the entry points).
//
//   1. vote_calls_check_kernel one lane per CALL: it lies in its container's slice, starts ascend strictly (error words only).
//      vote_mark_kernel        one lane per hit: the workgroup's 256 records come through LDS in 8-byte pieces, so the 24-byte
//                              records are read coalesced; a binary search over the container's CALL slice finds c_k; the lane
//                              writes its vote flag and k.  Per wave: one atomicAdd (accepted hits), one atomicMax (largest
//                              voting oI, which sizes the sort key).
//   2. prefix sum of the flags; vote_compact_kernel writes key = (seq << oi_bits) | oI, value = k for every vote.
//   3. the stable LSD radix sort of kg_build.hpp over bits_for(n_seqs) + oi_bits key bits.
//   4. vote_heads_kernel: run heads and CALL changes (k is non-decreasing inside a run: hit order is CALL order within a
//      sequence and the sort is stable); two prefix sums number the runs and count the changes in front of every vote;
//      vote_runs_kernel notes both at every head, vote_pairs_kernel takes votes and n_calls as differences of neighbouring
//      heads.  Nothing walks a run.
//   5. a second stable sort of the run numbers by (seq << v_bits) | (max_votes - votes): rule 3's order, oI ascending kept on
//      ties; vote_emit_kernel copies the pairs into it.  region_seq_start_kernel (kg_regions.hpp) finds vote_start over the
//      sorted keys, and a sequence's vote total as a slice of the first sort's keys.
//   6. vote_class_kernel       one lane per sequence: the class record, the assigned flag, the statistics (one atomicAdd per
//                              wave and counter).
//   7. the assigned sequences compacted to (key = oI, value = seq) and sorted; run heads number the bins;
//      vote_bin_sum_kernel adds every sequence into its bin (int64 atomicAdd: one per wave where the wave lies in one bin, else
//      one per lane); two more stable sorts (votes, then length, both descending) order the bins.
//
// Integers only; the atomics are adds and maxima of integers, so no result depends on the order they arrive in.  The returning
// atomics are atomicMin on the error words, and they run only for bad input.
#pragma once

#include "kg_build.hpp"
#include "kg_device.hpp"
#include "kg_regions.hpp"

namespace kg {

constexpr unsigned long long kVoteNoErr = 0x7F7F7F7F7F7F7F7Full;     // the error words' "none" (a byte memset)
constexpr int kVoteThreads = 256;

// error words: the first hit [0] outside its container's slice, [1] below its predecessor's from0InProt; the first CALL [2]
// outside its container's slice, [3] whose start does not exceed its predecessor's; [4] the first voting hit with oI < 0;
// [5] the first sequence whose votes or CALLs number 2^31 or more
enum { kVoteErrHitSlice = 0, kVoteErrHitOrder = 1, kVoteErrCallSlice = 2, kVoteErrCallOrder = 3, kVoteErrOtu = 4, kVoteErrTotal = 5,
       kVoteErrWords = 6 };
// counter words
enum { kVoteCntAccepted = 0, kVoteCntMaxOtu = 1, kVoteCntMaxVotes = 2, kVoteCntWithVotes = 3, kVoteCntAssigned = 4,
       kVoteCntAssignedLen = 5, kVoteCntWords = 6 };

__device__ inline uint32_t vote_wave_max(uint32_t x)
{
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t y = __shfl_down(x, off);
        x = y > x ? y : x;
    }
    return x;                           // lane 0 holds the maximum
}

__device__ inline uint64_t vote_wave_sum(uint64_t x)
{
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
    return x;                           // lane 0 holds the sum
}

__global__ __launch_bounds__(kVoteThreads) void vote_calls_check_kernel(const kg_call *__restrict__ calls, uint64_t n_calls,
                                                                        const int64_t *__restrict__ ccs, uint64_t n_cont,
                                                                        unsigned long long *err)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_calls) return;
    const kg_call c = calls[i];
    const uint64_t cont = c.container < n_cont ? c.container : n_cont - 1;
    const int64_t lo = ccs[cont], hi = ccs[cont + 1];
    if (c.container >= n_cont || (int64_t)i < lo || (int64_t)i >= hi) atomicMin(&err[kVoteErrCallSlice], (unsigned long long)i);
    else if ((int64_t)i > lo && calls[i - 1].start >= c.start) atomicMin(&err[kVoteErrCallOrder], (unsigned long long)i);
}

// rule 1.  flag[i] = hit i votes, cidx[i] = the CALL it votes in (index in calls[]).
__global__ __launch_bounds__(kVoteThreads) void vote_mark_kernel(const kg_hit *__restrict__ hits, const uint8_t *__restrict__ ev,
                                                                 uint64_t n, const int64_t *__restrict__ chs,
                                                                 const kg_call *__restrict__ calls, uint64_t n_calls,
                                                                 const int64_t *__restrict__ ccs, uint64_t n_cont,
                                                                 uint32_t *__restrict__ flag, uint32_t *__restrict__ cidx,
                                                                 unsigned long long *err, unsigned long long *cnt)
{
    static_assert(sizeof(kg_hit) == 24, "three 8-byte pieces per record");
    __shared__ uint2 sh[kVoteThreads * 3];
    const uint64_t base = (uint64_t)blockIdx.x * kVoteThreads;
    const uint32_t here = (uint32_t)(n - base < (uint64_t)kVoteThreads ? n - base : (uint64_t)kVoteThreads);
    const uint2 *src = (const uint2 *)(hits + base);
    for (uint32_t q = threadIdx.x; q < here * 3; q += kVoteThreads) sh[q] = src[q];
    __syncthreads();
    const uint32_t t = threadIdx.x;
    const uint64_t i = base + t;
    const bool in = t < here;
    uint32_t vote = 0, acc = 0, k_out = 0, oi = 0;
    if (in) {
        const uint2 a = sh[3 * t], b = sh[3 * t + 1], c2 = sh[3 * t + 2];
        const uint32_t container = a.x;
        const int32_t pos = (int32_t)a.y, h_oi = (int32_t)b.x, h_fi = (int32_t)c2.x;
        const uint64_t cont = container < n_cont ? container : n_cont - 1;
        const int64_t hlo = chs[cont], hhi = chs[cont + 1];
        if (container >= n_cont || (int64_t)i < hlo || (int64_t)i >= hhi) {
            atomicMin(&err[kVoteErrHitSlice], (unsigned long long)i);
        } else if ((int64_t)i > hlo) {
            const int32_t prev = t > 0 ? (int32_t)sh[3 * t - 3].y : hits[i - 1].from0InProt;
            if (prev > pos) atomicMin(&err[kVoteErrHitOrder], (unsigned long long)i);
        }
        acc = (ev[i] & KG_EV_ACCEPTED) ? 1u : 0u;
        int64_t lo = ccs[cont], hi = ccs[cont + 1];
        lo = lo < 0 ? 0 : (lo > (int64_t)n_calls ? (int64_t)n_calls : lo);
        hi = hi < lo ? lo : (hi > (int64_t)n_calls ? (int64_t)n_calls : hi);
        int64_t x = lo, y = hi;             // the first CALL of the slice whose start is beyond the hit
        while (x < y) {
            const int64_t mid = x + (y - x) / 2;
            if (calls[mid].start <= pos) x = mid + 1;
            else y = mid;
        }
        if (acc && x > lo) {
            const kg_call c = calls[x - 1];
            if (c.fI == h_fi && (int64_t)pos + (KG_K - 1) <= (int64_t)c.end) {
                vote = 1;
                k_out = (uint32_t)(x - 1);
                if (h_oi < 0) atomicMin(&err[kVoteErrOtu], (unsigned long long)i);
                else oi = (uint32_t)h_oi;
            }
        }
        flag[i] = vote;
        cidx[i] = k_out;
    }
    const uint32_t n_acc = (uint32_t)__popcll(__ballot(acc));
    const uint32_t top = vote_wave_max(oi);
    if ((threadIdx.x & 63) == 0) {
        if (n_acc) atomicAdd(&cnt[kVoteCntAccepted], (unsigned long long)n_acc);
        if (top) atomicMax(&cnt[kVoteCntMaxOtu], (unsigned long long)top);
    }
}

// the votes, in hit order: key = (seq << oi_bits) | oI, value = the CALL's index
__global__ __launch_bounds__(kVoteThreads) void vote_compact_kernel(const kg_hit *__restrict__ hits, const uint32_t *__restrict__ flag,
                                                                    const uint32_t *__restrict__ excl,
                                                                    const uint32_t *__restrict__ cidx, uint64_t n, uint64_t n_cont,
                                                                    uint32_t per, uint32_t oi_bits, uint64_t n_votes,
                                                                    uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint32_t at = excl[i];
    if (at >= n_votes) return;
    const uint64_t cont = hits[i].container < n_cont ? hits[i].container : n_cont - 1;
    const int32_t oi = hits[i].oI;
    const uint64_t low = oi < 0 ? 0u : ((uint64_t)(uint32_t)oi & ((1ull << oi_bits) - 1));
    keys[at] = ((cont / per) << oi_bits) | low;
    vals[at] = cidx[i];
}

// sorted pairs: head[j] = a new key; chg[j] (when given) = a new key or a new value
__global__ __launch_bounds__(kVoteThreads) void vote_heads_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                                  uint64_t n, uint32_t *__restrict__ head, uint32_t *__restrict__ chg)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const bool h = j == 0 || keys[j - 1] != keys[j];
    head[j] = h ? 1u : 0u;
    if (chg) chg[j] = (h || vals[j - 1] != vals[j]) ? 1u : 0u;
}

// run r begins at vote run_start[r] with run_cc[r] CALL changes in front of it; entry n_runs closes the last run
__global__ __launch_bounds__(kVoteThreads) void vote_runs_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ hexcl,
                                                                 const uint32_t *__restrict__ cexcl, uint64_t n, uint64_t n_runs,
                                                                 const uint64_t *__restrict__ total_chg,
                                                                 uint32_t *__restrict__ run_start, uint32_t *__restrict__ run_cc)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (j == 0) {
        run_start[n_runs] = (uint32_t)n;
        run_cc[n_runs] = (uint32_t)*total_chg;
    }
    if (!head[j]) return;
    const uint32_t r = hexcl[j];
    if (r >= n_runs) return;
    run_start[r] = (uint32_t)j;
    run_cc[r] = cexcl[j];
}

// rule 2: one lane per run
__global__ __launch_bounds__(kVoteThreads) void vote_pairs_kernel(const uint32_t *__restrict__ run_start, const uint32_t *__restrict__ run_cc,
                                                                  const uint64_t *__restrict__ keys, uint64_t n_votes, uint64_t n_runs,
                                                                  uint32_t oi_bits, kg_otu_vote *__restrict__ out, unsigned long long *cnt)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t votes = 0;
    if (r < n_runs) {
        const uint32_t a = run_start[r];
        const uint64_t key = keys[a < n_votes ? a : n_votes - 1];
        votes = run_start[r + 1] - a;
        kg_otu_vote v;
        v.seq = (int32_t)(key >> oi_bits);
        v.oI = (int32_t)(key & ((1ull << oi_bits) - 1));
        v.votes = (int32_t)votes;
        v.n_calls = (int32_t)(run_cc[r + 1] - run_cc[r]);
        out[r] = v;
    }
    const uint32_t top = vote_wave_max(votes);
    if ((threadIdx.x & 63) == 0 && top) atomicMax(&cnt[kVoteCntMaxVotes], (unsigned long long)top);
}

// rule 3's sort key, the runs being in (seq, oI) order
__global__ __launch_bounds__(kVoteThreads) void vote_order_keys_kernel(const kg_otu_vote *__restrict__ pairs, uint64_t n_runs,
                                                                       uint32_t max_votes, uint32_t v_bits,
                                                                       uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    const uint32_t votes = (uint32_t)pairs[r].votes;
    keys[r] = ((uint64_t)(uint32_t)pairs[r].seq << v_bits) | (uint64_t)(max_votes - (votes < max_votes ? votes : max_votes));
    vals[r] = (uint32_t)r;
}

__global__ __launch_bounds__(kVoteThreads) void vote_emit_kernel(const kg_otu_vote *__restrict__ in, const uint32_t *__restrict__ vals,
                                                                 uint64_t n, kg_otu_vote *__restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t v = vals[k];
    out[k] = in[v < n ? v : n - 1];
}

// rule 4: one lane per sequence.  tally_start: the sequence's slice of the votes in the first sort's order.
__global__ __launch_bounds__(kVoteThreads) void vote_class_kernel(const kg_otu_vote *__restrict__ pairs, const int64_t *__restrict__ vote_start,
                                                                  const int64_t *__restrict__ tally_start, const int64_t *__restrict__ ccs,
                                                                  const int64_t *__restrict__ offsets, uint64_t n_seqs, uint32_t per,
                                                                  kg_vote_params prm, kg_otu_class *__restrict__ out,
                                                                  uint32_t *__restrict__ aflag, unsigned long long *err,
                                                                  unsigned long long *cnt)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t with = 0, assigned = 0;
    uint64_t len = 0;
    if (s < n_seqs) {
        const int64_t a = vote_start[s], b = vote_start[s + 1];
        const int64_t total = tally_start[s + 1] - tally_start[s];
        const int64_t tc = ccs[(s + 1) * per] - ccs[s * per];
        if (total >= (1ll << 31) || tc >= (1ll << 31)) atomicMin(&err[kVoteErrTotal], (unsigned long long)s);
        kg_otu_class c;
        c.otu = -1; c.assigned = 0; c.votes = 0; c.total = (int32_t)total; c.n_calls = 0; c.total_calls = (int32_t)tc;
        c.n_otus = (int32_t)(b - a); c.second_otu = -1; c.second_votes = 0; c.reserved = 0;
        if (b > a) {
            const kg_otu_vote best = pairs[a];
            c.otu = best.oI;
            c.votes = best.votes;
            c.n_calls = best.n_calls;
            if (b - a > 1) {
                const kg_otu_vote second = pairs[a + 1];
                c.second_otu = second.oI;
                c.second_votes = second.votes;
            }
            with = 1;
            assigned = (best.votes >= prm.min_votes && best.n_calls >= prm.min_calls &&
                        100ll * (int64_t)best.votes >= (int64_t)prm.min_share_pct * total) ? 1u : 0u;
            c.assigned = (int32_t)assigned;
        }
        out[s] = c;
        aflag[s] = assigned;
        if (assigned) len = (uint64_t)(offsets[s + 1] - offsets[s]);
    }
    const uint32_t nw = (uint32_t)__popcll(__ballot(with)), na = (uint32_t)__popcll(__ballot(assigned));
    const uint64_t sum = vote_wave_sum(len);
    if ((threadIdx.x & 63) == 0) {
        if (nw) atomicAdd(&cnt[kVoteCntWithVotes], (unsigned long long)nw);
        if (na) atomicAdd(&cnt[kVoteCntAssigned], (unsigned long long)na);
        if (sum) atomicAdd(&cnt[kVoteCntAssignedLen], (unsigned long long)sum);
    }
}

// the assigned sequences, in sequence order: key = their OTU, value = the sequence
__global__ __launch_bounds__(kVoteThreads) void vote_bin_keys_kernel(const kg_otu_class *__restrict__ cls, const uint32_t *__restrict__ aflag,
                                                                     const uint32_t *__restrict__ aexcl, uint64_t n_seqs, uint64_t n_assigned,
                                                                     uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seqs || !aflag[s]) return;
    const uint32_t at = aexcl[s];
    if (at >= n_assigned) return;
    keys[at] = (uint64_t)(uint32_t)cls[s].otu;
    vals[at] = (uint32_t)s;
}

// rule 5's sums: acc[4 * bin + {0, 1, 2, 3}] += 1, length, votes, n_calls; bin_oi[bin] by the bin's head
__global__ __launch_bounds__(kVoteThreads) void vote_bin_sum_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                                    const uint32_t *__restrict__ head, const uint32_t *__restrict__ bexcl,
                                                                    uint64_t n, uint64_t n_bins, const kg_otu_class *__restrict__ cls,
                                                                    const int64_t *__restrict__ offsets, uint64_t n_seqs,
                                                                    int32_t *__restrict__ bin_oi, unsigned long long *acc)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t wave_first = j - (threadIdx.x & 63);
    if (wave_first >= n) return;            // (the whole wave)
    const bool in = j < n;
    uint64_t bin = 0, one = 0, len = 0, votes = 0, calls = 0;
    if (in) {
        bin = (uint64_t)bexcl[j] + head[j] - 1;
        bin = bin < n_bins ? bin : n_bins - 1;
        const uint64_t s = vals[j] < n_seqs ? vals[j] : n_seqs - 1;
        one = 1;
        len = (uint64_t)(offsets[s + 1] - offsets[s]);
        votes = (uint64_t)cls[s].votes;
        calls = (uint64_t)cls[s].n_calls;
        if (head[j]) bin_oi[bin] = (int32_t)(uint32_t)keys[j];
    }
    const uint64_t first_bin = __shfl(bin, 0);      // lane 0 is inside the list
    if (!in) bin = first_bin;
    if (__all(bin == first_bin)) {
        one = vote_wave_sum(one); len = vote_wave_sum(len); votes = vote_wave_sum(votes); calls = vote_wave_sum(calls);
        if ((threadIdx.x & 63) != 0) return;
    } else if (!in) {
        return;
    }
    atomicAdd(&acc[4 * bin + 0], (unsigned long long)one);
    atomicAdd(&acc[4 * bin + 1], (unsigned long long)len);
    atomicAdd(&acc[4 * bin + 2], (unsigned long long)votes);
    atomicAdd(&acc[4 * bin + 3], (unsigned long long)calls);
}

// the bins in oI order, and the first of their two sort keys: votes descending
__global__ __launch_bounds__(kVoteThreads) void vote_bin_records_kernel(const unsigned long long *__restrict__ acc,
                                                                        const int32_t *__restrict__ bin_oi, uint64_t n_bins,
                                                                        uint64_t votes_top, kg_otu_bin *__restrict__ out,
                                                                        uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bins) return;
    kg_otu_bin r;
    r.oI = bin_oi[b];
    r.n_seqs = (int32_t)acc[4 * b + 0];
    r.length = (int64_t)acc[4 * b + 1];
    r.votes = (int64_t)acc[4 * b + 2];
    r.n_calls = (int64_t)acc[4 * b + 3];
    out[b] = r;
    const uint64_t v = (uint64_t)r.votes;
    keys[b] = votes_top - (v < votes_top ? v : votes_top);
    vals[b] = (uint32_t)b;
}

// the second key, in the order the first sort left the bins in: length descending
__global__ __launch_bounds__(kVoteThreads) void vote_bin_rekey_kernel(const kg_otu_bin *__restrict__ bins, const uint32_t *__restrict__ vals,
                                                                      uint64_t n_bins, uint64_t length_top, uint64_t *__restrict__ keys)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_bins) return;
    const uint32_t v = vals[k];
    const uint64_t len = (uint64_t)bins[v < n_bins ? v : n_bins - 1].length;
    keys[k] = length_top - (len < length_top ? len : length_top);
}

__global__ __launch_bounds__(kVoteThreads) void vote_bin_emit_kernel(const kg_otu_bin *__restrict__ in, const uint32_t *__restrict__ vals,
                                                                     uint64_t n, kg_otu_bin *__restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t v = vals[k];
    out[k] = in[v < n ? v : n - 1];
}

}  // namespace kg
