// kg_ungapped.hpp -- device side of kg_proteins_search_filtered / _device (include/kmerguts_hip.h states the rule): every shared
// seed carries its diagonal through the join, each candidate's best seed diagonal is chosen, the whole diagonal is scored without
// gaps, and the per-query cut is made by that score.  Integers only.
//
// The front half is the search call's (kg_search.hpp, steps 1 to 3): the window pairs pk / pv, the k-mer runs, their weights and
// the listed runs.  pv[j] = len_p - i of the first window of pair j's seed in its protein, which the plain search overwrites and
// this stage keeps.  Behind it:
//
//   4u. search_join_diag_kernel     search_join_kernel's tile and hand-out, with key = (q << db | d) << gb | (g + bias):
//                                   g = (len_q - pv_q) - (len_d - pv_d), the lengths from the device offsets, bias = the longest
//                                   target - 1, gb = bits(longest query + longest target)
//   5u. the radix sort over all qb + db + gb bits: the diagonals stand in order inside every (q, d) run.  Heads at two levels
//       (search_query_heads_kernel on key >> gb, derive_key_heads_kernel on the key), a prefix sum and
//       cluster_link_starts_kernel each: the (q, d) runs (length s) and the (q, d, g) runs (length m(g))
//       ungapped_best_kernel        per (q, d, g) run one atomicMax of m << 32 | ~(g + bias) on its (q, d) run's word: the largest
//                                   m, on a tie the smallest g, whatever the order of the lanes
//   6u. search_cand_flags_kernel as it is, then ungapped_cand_kernel: the candidates compacted in (q, d) order with s, g* and m(g*)
//       search_ungapped_kernel      one wave per candidate: u, the best run of the diagonal's cells
//       ungapped_keep_kernel / ungapped_emit_kernel
//                                   u >= min_ungapped, compacted; the second sort's key q << (ub + sb) | (umax - u) << sb | (smax - s)
//   7u. the radix sort, search_query_heads_kernel, search_top_flags_kernel and search_top_emit_kernel as they are;
//       ungapped_top_emit_kernel carries (u, g*, m) beside s
//   9u. behind search_order_kernel: ungapped_place_kernel gives every ordered record the 16 bytes of its candidate
//
// What bounds a lane's work: every kernel but two is one item per lane.  search_join_diag_kernel is the join's tile;
// search_ungapped_kernel walks one diagonal with the whole wave, 64 cells a step, so its trips are the diagonal's length / 64 and
// the same in every lane; ungapped_place_kernel looks through its query's kept candidates, at most kSearchMaxCand.  No lane walks
// a run of the join.
//
// The diagonal walk.  With P_j the sum of the cells 0 .. j and E_j = P_j - cell_j the sum in front of cell j, the best non-empty
// run ending at j is P_j - min_{k <= j} E_k, and u = max(0, max_j of that).  Per step the wave makes P by a prefix sum over its
// lanes and the running minimum of E by a prefix minimum (shuffles), and two values go on to the next step: P of the last lane
// and the minimum so far.  A lane behind the diagonal's end holds a cell of 0: its P is the last cell's and its term is a run that
// ends there, or 0.  |cell| <= 16 and fewer than 2^24 cells: |P| < 2^28 (kAlignMaxLen bounds the alignment's sums the same way).
// No LDS but the score table, which the workgroup fills once; the statistics are one atomic per wave and word, behind the loops.
#pragma once

#include "kg_search.hpp"

namespace kg {

constexpr int kUngappedThreads = 256;
// the counter words of the stage (a block of its own, behind the search's)
enum : int { kUngappedCells = 0, kUngappedUmax = 1, kUngappedWords = 2 };

struct UngappedRec { int32_t ungapped, diagonal, on_diagonal, reserved; };      // kg_search_ungapped

// search_join_kernel with the diagonal in the key's low gb bits: keys[j] = (q << db | d) << gb | (g + bias), vals[j] = 0.
// pv: beside pk; off: the batch's offsets (protein p has off[p + 1] - off[p] residues).
__global__ __launch_bounds__(kSearchThreads) void search_join_diag_kernel(const uint64_t *__restrict__ pk, const uint32_t *__restrict__ pv,
                                                                          const int64_t *__restrict__ off, const uint32_t *__restrict__ wx,
                                                                          const uint32_t *__restrict__ cstart, const uint32_t *__restrict__ cnd,
                                                                          uint32_t n_runs, uint32_t n_items, uint32_t b, uint32_t n_db,
                                                                          uint32_t db, uint32_t gb, int32_t bias,
                                                                          uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    __shared__ uint32_t s_wx[kSearchTile], s_start[kSearchTile];       // (a run's targets stay in device memory: 16 KiB, eight waves)
    const uint32_t j0 = blockIdx.x * (uint32_t)kSearchTile;
    if (j0 >= n_items) return;
    const uint32_t j1 = n_items - j0 > (uint32_t)kSearchTile ? j0 + kSearchTile : n_items;
    const uint32_t r0 = search_run_of(wx, n_runs, j0), r1 = search_run_of(wx, n_runs, j1 - 1);
    uint32_t nr = r1 - r0 + 1;
    nr = nr > (uint32_t)kSearchTile ? (uint32_t)kSearchTile : nr;
    for (uint32_t k = threadIdx.x; k < nr; k += kSearchThreads) {
        s_wx[k] = wx[r0 + k];
        s_start[k] = cstart[r0 + k];
    }
    __syncthreads();
    const uint64_t mask = (1ull << b) - 1;
    for (uint32_t base = j0 + 2 * threadIdx.x; base < j1; base += 2 * kSearchThreads) {
        uint32_t k = search_run_of(s_wx, nr, base);
        uint64_t key[2] = {0, 0};
        const int cnt = j1 - base >= 2 ? 2 : 1;
        for (int i = 0; i < cnt; i++) {
            const uint32_t j = base + i;
            if (i && k + 1 < nr && s_wx[k + 1] <= j) k++;
            const uint32_t t = j - s_wx[k], nd = cnd[r0 + k], start = s_start[k];
            const uint32_t qi = t / nd, di = t - qi * nd;
            const uint32_t pd = (uint32_t)(pk[start + di] & mask), pq = (uint32_t)(pk[start + nd + qi] & mask);
            const int32_t len_d = (int32_t)(off[pd + 1] - off[pd]), len_q = (int32_t)(off[pq + 1] - off[pq]);
            const int32_t g = (len_q - (int32_t)pv[start + nd + qi]) - (len_d - (int32_t)pv[start + di]);
            key[i] = (((((uint64_t)(pq - n_db)) << db) | pd) << gb) | (uint64_t)(uint32_t)(g + bias);
        }
        if (cnt == 2) {
            *reinterpret_cast<ulonglong2 *>(keys + base) = make_ulonglong2(key[0], key[1]);     // (base is even: 16-byte aligned)
            *reinterpret_cast<uint2 *>(vals + base) = make_uint2(0u, 0u);
        } else {
            keys[base] = key[0];
            vals[base] = 0;
        }
    }
}

// (q, d, g) run r = items [gstart[r], gstart[r + 1]) of the sorted join, inside the (q, d) run lx[first] + lh[first] - 1 (lh: the
// heads of key >> gb, lx: their exclusive scan): best[that run] = max of m << 32 | ~(g + bias) (best zeroed beforehand)
__global__ __launch_bounds__(256) void ungapped_best_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ gstart,
                                                            uint64_t n_gruns, const uint32_t *__restrict__ lh, const uint32_t *__restrict__ lx,
                                                            uint32_t gb, unsigned long long *__restrict__ best)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_gruns) return;
    const uint32_t first = gstart[r], m = gstart[r + 1] - first;
    const uint32_t gbias = (uint32_t)(keys[first] & ((1ull << gb) - 1));
    atomicMax(&best[lx[first] + lh[first] - 1u], ((unsigned long long)m << 32) | (unsigned long long)(0xFFFFFFFFu - gbias));
}

// candidate cx[r] of every flagged (q, d) run r: ckey = q << db | d, cs = s, cdiag = (g* + bias, m(g*))
__global__ __launch_bounds__(256) void ungapped_cand_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ lstart,
                                                            const uint32_t *__restrict__ cf, const uint32_t *__restrict__ cx,
                                                            const unsigned long long *__restrict__ best, uint64_t n_runs, uint64_t n_cand,
                                                            uint32_t gb, uint64_t *__restrict__ ckey, uint32_t *__restrict__ cs,
                                                            uint2 *__restrict__ cdiag)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs || !cf[r]) return;
    const uint32_t o = cx[r];
    if (o >= n_cand) return;
    const uint32_t first = lstart[r];
    const unsigned long long w = best[r];
    ckey[o] = keys[first] >> gb;
    cs[o] = lstart[r + 1] - first;
    cdiag[o] = make_uint2(0xFFFFFFFFu - (uint32_t)w, (uint32_t)(w >> 32));
}

__device__ __forceinline__ int ungapped_wave_max(int v)
{
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const int o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// One wave per candidate, 64 candidates per wave and trip: lane k of the wave reads candidate 64 * chunk + k and keeps its u, the
// wave scores the 64 diagonals one after the other, and the 64 results leave in one store.  The chunks are handed out grid-stride.
// ckey = q << db | d, cdiag.x = g* + bias; u_out[c] = u.  words: the cells scored and the largest u, one atomic each per wave.
__global__ __launch_bounds__(kUngappedThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void search_ungapped_kernel(const uint8_t *__restrict__ seq, const int64_t *__restrict__ off,
                                                                           const uint64_t *__restrict__ ckey, const uint2 *__restrict__ cdiag,
                                                                           uint32_t n_cand, uint32_t n_db, uint32_t db, int32_t bias,
                                                                           const int8_t *__restrict__ matrix, int32_t *__restrict__ u_out,
                                                                           unsigned long long *__restrict__ words)
{
    __shared__ int8_t table[21 * kAlignRowStride];
    for (int k = (int)threadIdx.x; k < 21 * 21; k += kUngappedThreads)
        table[(k / 21) * kAlignRowStride + k % 21] = matrix ? matrix[k] : kBlosum62[k];
    __syncthreads();
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const uint32_t waves = gridDim.x * (uint32_t)(kUngappedThreads / kWave);
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kUngappedThreads / kWave) + (threadIdx.x >> 6)));
    const uint32_t n_chunks = (n_cand + kWave - 1) / kWave;
    unsigned long long cells = 0;                       // (wave-uniform)
    int umax = 0;
    for (uint32_t chunk = wave0; chunk < n_chunks; chunk += waves) {
        const uint32_t c = chunk * kWave + (uint32_t)lane;
        const int cnt = (int)(n_cand - chunk * kWave < (uint32_t)kWave ? n_cand - chunk * kWave : (uint32_t)kWave);
        uint64_t my_key = 0;
        int my_g = 0, my_u = 0;
        if (c < n_cand) {
            my_key = ckey[c];
            my_g = (int)cdiag[c].x - bias;
        }
        for (int k = 0; k < cnt; k++) {
            const unsigned long long key = __shfl((unsigned long long)my_key, k);
            const int g = __builtin_amdgcn_readfirstlane(__shfl(my_g, k));
            const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key >> db));
            const uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key & ((1ull << db) - 1)));
            const int64_t at_q = off[n_db + q], at_d = off[d];
            const int len_q = (int)(off[n_db + q + 1] - at_q), len_d = (int)(off[d + 1] - at_d);
            const int a0 = g > 0 ? g : 0, a1 = len_q < len_d + g ? len_q : len_d + g;
            const int n = a1 > a0 ? a1 - a0 : 0;        // the cells (a, a - g), a0 <= a < a1
            int carry_p = 0, carry_min = 0, best = 0;
            for (int t0 = 0; t0 < n; t0 += kWave) {
                const int a = a0 + t0 + lane;
                int cell = 0;
                if (t0 + lane < n) {
                    const int ca = (int)aa_code_of_rt((char)seq[at_q + a]), cb = (int)aa_code_of_rt((char)seq[at_d + (a - g)]);
                    cell = (int)table[ca * kAlignRowStride + cb];
                }
                int p = cell;                           // the inclusive prefix sum over the lanes
                for (int s = 1; s < kWave; s <<= 1) {
                    const int o = __shfl_up(p, s);
                    p += lane >= s ? o : 0;
                }
                p += carry_p;
                int e = p - cell;                       // the inclusive prefix minimum of the sums in front of each cell
                for (int s = 1; s < kWave; s <<= 1) {
                    const int o = __shfl_up(e, s);
                    e = lane >= s && o < e ? o : e;
                }
                e = carry_min < e ? carry_min : e;
                best = p - e > best ? p - e : best;
                carry_p = __shfl(p, kWave - 1);
                carry_min = __shfl(e, kWave - 1);
            }
            const int u = ungapped_wave_max(best);
            my_u = lane == k ? u : my_u;
            umax = u > umax ? u : umax;
            cells += (unsigned long long)n;
        }
        if (c < n_cand) u_out[c] = my_u;
    }
    if (lane == 0) {
        if (cells) atomicAdd(&words[kUngappedCells], cells);
        if (umax) atomicMax(&words[kUngappedUmax], (unsigned long long)umax);
    }
}

// kf[c] = u[c] >= min_ungapped
__global__ __launch_bounds__(256) void ungapped_keep_kernel(const int32_t *__restrict__ u, uint64_t n, int32_t min_ungapped, uint32_t *__restrict__ kf)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    kf[c] = u[c] >= min_ungapped ? 1u : 0u;
}

// kept candidate kx[c] (still in (q, d) order): its join key, s and 16-byte record, and the second sort's pair: key
// q << (ub + sb) | (umax - u) << sb | (smax - s), the kept candidate's index as the value
__global__ __launch_bounds__(256) void ungapped_emit_kernel(const uint64_t *__restrict__ ckey, const uint32_t *__restrict__ cs,
                                                            const uint2 *__restrict__ cdiag, const int32_t *__restrict__ u,
                                                            const uint32_t *__restrict__ kf, const uint32_t *__restrict__ kx, uint64_t n,
                                                            uint64_t n_kept, uint32_t db, uint32_t sb, uint32_t ub, uint32_t smax,
                                                            uint32_t umax, int32_t bias, uint64_t *__restrict__ kkey, uint32_t *__restrict__ ks,
                                                            UngappedRec *__restrict__ krec, uint64_t *__restrict__ skey, uint32_t *__restrict__ sval)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n || !kf[c]) return;
    const uint32_t o = kx[c];
    if (o >= n_kept) return;
    const uint64_t key = ckey[c];
    const uint32_t s = cs[c], uu = (uint32_t)u[c];
    const uint2 dg = cdiag[c];
    kkey[o] = key;
    ks[o] = s;
    krec[o] = UngappedRec{(int32_t)uu, (int32_t)dg.x - bias, (int32_t)dg.y, 0};
    skey[o] = ((((key >> db) << ub) | (uint64_t)(umax - (uu < umax ? uu : umax))) << sb) | (uint64_t)(smax - (s < smax ? s : smax));
    sval[o] = o;
}

// search_top_emit_kernel's companion: the 16-byte record of kept candidate tx[i]
__global__ __launch_bounds__(256) void ungapped_top_emit_kernel(const uint32_t *__restrict__ sval, const UngappedRec *__restrict__ krec,
                                                                const uint32_t *__restrict__ tf, const uint32_t *__restrict__ tx, uint64_t n,
                                                                uint64_t n_kept, UngappedRec *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !tf[i]) return;
    const uint32_t o = tx[i];
    if (o >= n_kept) return;
    out[o] = krec[sval[i]];
}

// ordered record i = (query, target, ...): out[i] = the record of the query's kept candidate with that target, which stands in
// [hit_start[q], hit_start[q + 1]) of pairs / rec (at most kSearchMaxCand of them, every target once)
__global__ __launch_bounds__(256) void ungapped_place_kernel(const int2 *__restrict__ hits, const int64_t *__restrict__ hit_start,
                                                             const int32_t *__restrict__ pairs, const UngappedRec *__restrict__ rec,
                                                             uint64_t n, uint32_t n_q, UngappedRec *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int2 qd = hits[i * 5];
    int64_t at = -1;
    if ((uint32_t)qd.x < n_q) {
        const int64_t first = hit_start[qd.x];
        int64_t c = hit_start[qd.x + 1] - first;
        c = c > kSearchMaxCand ? kSearchMaxCand : c;
        for (int64_t k = 0; k < c; k++)
            if (first + k < (int64_t)n && pairs[2 * (size_t)(first + k) + 1] == qd.y) at = first + k;
    }
    int4 r = make_int4(0, 0, 0, 0);
    if (at >= 0) r = reinterpret_cast<const int4 *>(rec)[at];
    reinterpret_cast<int4 *>(out)[i] = r;
}

}  // namespace kg
