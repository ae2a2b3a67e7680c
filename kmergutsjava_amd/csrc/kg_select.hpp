// kg_select.hpp -- device side of kg_regionset_select / kg_orfset_select / kg_select_intervals (include/kmerguts_hip.h): the
// non-overlapping selection among the candidates of a region set, an ORF set or a caller's list (the rule is stated in the
// header, next to the entry points).
//
//   1. select_keys_kernel      one lane per candidate: validation (one error word by atomicMin, firing only on bad input);
//                              key = (seq << left_bits) | left, value = the candidate's index.  The stable LSD radix sort of
//                              kg_build.hpp gives (seq, left, index) order; a region set is in that order by its own rule 5 and
//                              is not sorted.  select_flags_kernel marks the eligible candidates in that order, their prefix
//                              sum numbers them, select_compact_kernel writes their fields side by side.
//   2. select_count_kernel     the later candidates that overlap candidate m are the contiguous run with the same seq and
//                              left_j <= right_m: its end by binary search over the sorted keys, never a walk.  It also adds
//                              the run lengths up in 64 bits (one atomic per wave): the total P, which the host reads (the one
//                              wait before the rounds).  The prefix sum of the run lengths is pair_start[]; it adds in 32 bits
//                              and is right whenever P < 2^32, so it is used only behind the check of P.
//   3. select_expand_kernel    divided by output position: a lane owns kSelectPairsPerLane consecutive pair slots, finds the
//                              owner of each by binary search in pair_start (the neighbour first), tests rule 2 and writes the
//                              edge (strong, weak) by rule 3, or a dead marker.  No lane's trip count depends on a candidate's
//                              degree.
//   4. rounds                  select_edge_kernel: one lane per pair slot (a dead slot returns at once); select_node_kernel: one
//                              lane per candidate.  See the comment in front of them for why a stale read cannot change a
//                              decision.
//   5. select_by_kernel        atomicMin(by[weak], index of strong) over the live edges selected -> overlapped;
//      select_emit_kernel      the records back in the set's index order, and the counters (one atomic per wave).
//
// Atomics, none of which uses its return value: atomicMin on the error word (bad input only) and on by[] (one per edge from a
// selected to an overlapped candidate), and one atomicAdd per wave on the counters of select_count_kernel (pairs),
// select_expand_kernel (conflicts), select_node_kernel (still undecided) and select_emit_kernel (selected, overlapped).
#pragma once

#include "kg_device.hpp"

namespace kg {

constexpr int kSelectPairsPerLane = 8;  // pair slots a lane of select_expand_kernel owns
constexpr uint32_t kSelectDead = 0xFFFFFFFFu;     // pairs[p].x of a pair that does not conflict
// per eligible candidate
enum : uint32_t { kSelUndecided = 0, kSelSelected = 1, kSelOverlapped = 2 };
// the call's 64-bit words: the error word (the first bad candidate, kNoErr = none), then the counters
enum { kSelectErr = 0, kSelectEligible = 1, kSelectPairs = 2, kSelectConflicts = 3, kSelectSelected = 4, kSelectOverlapped = 5,
       kSelectUndecided = 6 /* [+ k]: still undecided after round k of a batch of rounds */, kSelectRoundsPerRead = 4,
       kSelectScanTotal = kSelectUndecided + kSelectRoundsPerRead /* the 32-bit prefix sum's total: not read */,
       kSelectWords = kSelectScanTotal + 1 };

struct SelectCand { int32_t seq, left, right, score, eligible; };

__device__ inline SelectCand select_cand(const kg_interval &c) { return {c.seq, c.left, c.right, c.score, c.eligible}; }
__device__ inline SelectCand select_cand(const kg_region &r) { return {r.seq, r.left, r.right, r.score, r.kept}; }
__device__ inline SelectCand select_cand(const kg_orf &o) { return {o.seq, o.left, o.right, o.score, o.kept}; }

__device__ inline bool select_bad(const SelectCand &c, uint64_t n_seqs)
{
    return c.seq < 0 || (uint64_t)c.seq >= n_seqs || c.left < 0 || c.right < c.left;
}

// A bad candidate's fields are clamped before they go into a key (the call fails with KG_ERR_ARG anyway); no field of any
// candidate is ever an index.
template <typename T>
__global__ __launch_bounds__(256) void select_keys_kernel(const T *__restrict__ in, uint64_t n, uint64_t n_seqs, uint32_t left_bits,
                                                          uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                          unsigned long long *err)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SelectCand c = select_cand(in[i]);
    const bool bad = select_bad(c, n_seqs);
    if (bad) atomicMin(&err[kSelectErr], (unsigned long long)i);
    const uint64_t mask = (1ull << left_bits) - 1;
    const uint64_t seq = bad ? 0 : (uint64_t)c.seq;
    const uint64_t left = bad ? 0 : ((uint64_t)c.left < mask ? (uint64_t)c.left : mask);
    keys[i] = (seq << left_bits) | left;
    vals[i] = (uint32_t)i;
}

// (seq, left) order: flag[j] = the candidate there takes part
template <typename T>
__global__ __launch_bounds__(256) void select_flags_kernel(const T *__restrict__ in, uint64_t n, uint64_t n_seqs,
                                                           const uint32_t *__restrict__ vals, uint32_t *__restrict__ flag)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t v = vals[j];
    const SelectCand c = select_cand(in[v < n ? v : n - 1]);
    flag[j] = (c.eligible != 0 && !select_bad(c, n_seqs)) ? 1u : 0u;
}

// the eligible candidates side by side, numbered m = pos[j] in (seq, left, index) order
struct SelectCols {
    uint64_t *key;                      // (seq << left_bits) | left
    int32_t *right, *score;
    uint32_t *orig;                     // index in the set
};

template <typename T>
__global__ __launch_bounds__(256) void select_compact_kernel(const T *__restrict__ in, uint64_t n, const uint64_t *__restrict__ keys,
                                                             const uint32_t *__restrict__ vals, const uint32_t *__restrict__ flag,
                                                             const uint32_t *__restrict__ pos, SelectCols c)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !flag[j]) return;
    const uint32_t v = vals[j], m = pos[j];
    const SelectCand a = select_cand(in[v < n ? v : n - 1]);
    c.key[m] = keys[j];
    c.right[m] = a.right;
    c.score[m] = a.score;
    c.orig[m] = v;
}

// count[m] = the candidates behind m that overlap it (rule 1): those up to the last key <= (seq_m, right_m), found by binary
// search.  right_m may be beyond every left: it is held to the key's left field.  count[m] = 0 for m in [E, n).
// words[kSelectPairs] += the counts, in 64 bits, by one atomic per wave.
__global__ __launch_bounds__(256) void select_count_kernel(const uint64_t *__restrict__ key, const int32_t *__restrict__ right,
                                                           const uint64_t *__restrict__ n_eligible, uint64_t n, uint32_t left_bits,
                                                           uint32_t *__restrict__ count, unsigned long long *words)
{
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t E = *n_eligible;
    unsigned long long mine = 0;
    if (m < E) {
        const uint64_t mask = (1ull << left_bits) - 1;
        const uint64_t r = (uint64_t)right[m];
        const uint64_t bound = (key[m] & ~mask) | (r < mask ? r : mask);
        uint64_t lo = m + 1, hi = E;    // the first j > m with key[j] > bound
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (key[mid] <= bound) lo = mid + 1;
            else hi = mid;
        }
        mine = lo - m - 1;
    }
    if (m < n) count[m] = (uint32_t)mine;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&words[kSelectPairs], mine);
}

// the last m in [0, E) with pair_start[m] <= p (p < P): the candidate that owns pair slot p.  Candidates without pairs share
// their successor's start and are never the last.
__device__ inline uint64_t select_owner(const uint32_t *__restrict__ pair_start, uint64_t E, uint64_t p)
{
    uint64_t lo = 0, hi = E;            // pair_start[lo] <= p < pair_start[hi] (pair_start[E] = P)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (pair_start[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// rule 3: a is stronger than b
__device__ inline bool select_stronger(int32_t score_a, int64_t len_a, uint32_t orig_a, int32_t score_b, int64_t len_b, uint32_t orig_b)
{
    if (score_a != score_b) return score_a > score_b;
    if (len_a != len_b) return len_a > len_b;
    return orig_a < orig_b;
}

// A lane owns pair slots [kSelectPairsPerLane * q, + kSelectPairsPerLane).  Slot p of owner m is the pair (m, m + 1 + p -
// pair_start[m]).  pairs[p] = (strong, weak) in the eligible numbering when the two conflict, else (kSelectDead, 0).
__global__ __launch_bounds__(256) void select_expand_kernel(SelectCols c, const uint32_t *__restrict__ pair_start, uint64_t E, uint64_t P,
                                                            uint32_t left_bits, int64_t max_overlap, int64_t max_pct,
                                                            uint2 *__restrict__ pairs, unsigned long long *words)
{
    const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kSelectPairsPerLane;
    const uint64_t mask = (1ull << left_bits) - 1;
    uint32_t live = 0;
    if (first < P) {
        uint64_t m = select_owner(pair_start, E, first);
        uint64_t begin = pair_start[m], end = m + 1 < E ? pair_start[m + 1] : P;
        int64_t left_m = (int64_t)(c.key[m] & mask), right_m = c.right[m];
        int32_t score_m = c.score[m];
        uint32_t orig_m = c.orig[m];
        for (int k = 0; k < kSelectPairsPerLane && first + k < P; k++) {
            const uint64_t p = first + k;
            if (p >= end) {
                // the neighbour first (a candidate with one pair), else a new search: candidates without pairs cost nothing
                bool next = false;
                if (m + 1 < E) {
                    const uint64_t b1 = pair_start[m + 1], e1 = m + 2 < E ? pair_start[m + 2] : P;
                    next = b1 <= p && p < e1;
                }
                m = next ? m + 1 : select_owner(pair_start, E, p);
                begin = pair_start[m];
                end = m + 1 < E ? pair_start[m + 1] : P;
                left_m = (int64_t)(c.key[m] & mask);
                right_m = c.right[m];
                score_m = c.score[m];
                orig_m = c.orig[m];
            }
            uint64_t j = m + 1 + (p - begin);
            if (j >= E) j = E - 1;      // (cannot happen: the run of m ends inside the list)
            const int64_t left_j = (int64_t)(c.key[j] & mask), right_j = c.right[j];
            const int32_t score_j = c.score[j];
            const uint32_t orig_j = c.orig[j];
            // left_m <= left_j, and left_j <= right_m by the run: ov > 0
            const int64_t ov = (right_m < right_j ? right_m : right_j) - left_j + 1;
            const int64_t len_m = right_m - left_m + 1, len_j = right_j - left_j + 1;
            const int64_t shorter = len_m < len_j ? len_m : len_j;
            uint2 e = make_uint2(kSelectDead, 0u);
            if (ov > max_overlap || 100 * ov > max_pct * shorter) {
                const bool m_wins = select_stronger(score_m, len_m, orig_m, score_j, len_j, orig_j);
                e = m_wins ? make_uint2((uint32_t)m, (uint32_t)j) : make_uint2((uint32_t)j, (uint32_t)m);
                live++;
            }
            pairs[p] = e;
        }
    }
    for (int off = 32; off > 0; off >>= 1) live += __shfl_down(live, off);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(&words[kSelectConflicts], (unsigned long long)live);
}

// ---- the rounds ----
// state[m] is undecided, selected or overlapped; selected and overlapped are final.  Round r:
//   edge kernel, per live edge (s, w):  state[s] selected -> state[w] = overlapped (a plain store: every writer stores the same
//                                       value); both ends undecided -> blocked[w] = r (likewise).
//   node kernel, per candidate m:       undecided and blocked[m] != r -> selected.
// Invariant: a candidate is marked selected only when every stronger candidate it conflicts with is overlapped, and overlapped
// only when a stronger one it conflicts with is selected -- which is the definition of the greedy fixed point (rule 4), taken
// in strength order, and that fixed point is unique.  The edge kernel's lanes read state[] while other lanes of the same launch
// store overlapped into it, so a lane may see an end as undecided that another lane has just marked overlapped.  Whichever value
// it sees, the invariant holds: seeing the strong end s still undecided only sets blocked[w], which keeps w undecided for one
// more round; seeing it overlapped leaves w alone, which is right because s is out for good; and seeing the weak end w already
// overlapped writes nothing.  No read can make a lane store selected or overlapped where the fixed point says otherwise, so a
// stale read delays a decision by a round and never changes it: the result does not depend on timing, launch geometry or how
// many rounds the host runs per read (rule 7).  Kernel boundaries order the rounds: what the node kernel of round r stores is
// visible to the edge kernel of round r + 1.
// Progress: the strongest undecided candidate has no undecided stronger neighbour, so nothing blocks it: it is decided in this
// round (selected) or the next edge kernel (overlapped).  The number of rounds is the longest chain of decisions that wait for
// each other, at most the number of candidates.  Rounds after the last decision change nothing.
__global__ __launch_bounds__(256) void select_edge_kernel(const uint2 *__restrict__ pairs, uint64_t P, uint32_t *state, uint32_t *blocked,
                                                          uint32_t round)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const uint2 e = pairs[p];
    if (e.x == kSelectDead) return;
    const uint32_t ss = state[e.x];
    if (ss == kSelSelected) state[e.y] = kSelOverlapped;
    else if (ss == kSelUndecided && state[e.y] == kSelUndecided) blocked[e.y] = round;
}

// undecided[0] += the candidates still undecided after this round: one non-returning atomic per wave
__global__ __launch_bounds__(256) void select_node_kernel(uint32_t *state, const uint32_t *__restrict__ blocked, uint64_t E, uint32_t round,
                                                          unsigned long long *undecided)
{
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool still = false;
    if (m < E && state[m] == kSelUndecided) {
        if (blocked[m] != round) state[m] = kSelSelected;
        else still = true;
    }
    const uint32_t n_still = (uint32_t)__popcll(__ballot(still));
    if ((threadIdx.x & 63) == 0 && n_still) atomicAdd(undecided, (unsigned long long)n_still);
}

// by[w] = the smallest set index among the selected candidates w lost to (by[] starts as 0xFFFFFFFF = -1)
__global__ __launch_bounds__(256) void select_by_kernel(const uint2 *__restrict__ pairs, uint64_t P, const uint32_t *__restrict__ state,
                                                        const uint32_t *__restrict__ orig, uint32_t *by)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const uint2 e = pairs[p];
    if (e.x == kSelectDead) return;
    if (state[e.x] == kSelSelected && state[e.y] == kSelOverlapped) atomicMin(&by[e.y], orig[e.x]);
}

// the records in the set's index order; words[kSelectSelected / kSelectOverlapped] by one atomic per wave
__global__ __launch_bounds__(256) void select_emit_kernel(const uint32_t *__restrict__ vals, const uint32_t *__restrict__ flag,
                                                          const uint32_t *__restrict__ pos, uint64_t n, const uint32_t *__restrict__ state,
                                                          const uint32_t *__restrict__ by, kg_selection *__restrict__ out,
                                                          unsigned long long *words)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool sel = false, ovl = false;
    if (j < n) {
        const uint32_t v = vals[j];
        kg_selection r;
        r.state = KG_SEL_NOT_ELIGIBLE;
        r.by = -1;
        if (flag[j]) {
            const uint32_t m = pos[j], st = state[m];
            sel = st == kSelSelected;
            ovl = st == kSelOverlapped;
            r.state = ovl ? KG_SEL_OVERLAPPED : KG_SEL_SELECTED;
            if (ovl) r.by = (int32_t)by[m];
        }
        out[v < n ? v : n - 1] = r;
    }
    const uint32_t ns = (uint32_t)__popcll(__ballot(sel)), no = (uint32_t)__popcll(__ballot(ovl));
    if ((threadIdx.x & 63) == 0) {
        if (ns) atomicAdd(&words[kSelectSelected], (unsigned long long)ns);
        if (no) atomicAdd(&words[kSelectOverlapped], (unsigned long long)no);
    }
}

}  // namespace kg
