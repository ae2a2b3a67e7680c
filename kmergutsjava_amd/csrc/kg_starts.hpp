// kg_starts.hpp -- device side of kg_orfset_starts / kg_starts_orfs (include/kmerguts_hip.h): the start codon of every movable
// ORF record, chosen by a trained start-site score (the rule is stated in the header, next to the entry points).
//
// Everything is integer: counts are 64-bit atomic adds, scores are int64 sums, the choice is an atomic maximum and an atomic
// minimum, so no order can matter.
//
//   1. starts_lens_kernel     one lane per record: the validation of coding_lens_kernel, the limit of rule 3 (a region set or the
//                             caller's list), the largest k a candidate may have, the codons n_res of the movable records.
//      prefix_sum of the codons: codon p of the list is codon k of one record.
//   2. starts_pairs_kernel    one lane per codon, T[4096] in LDS, a workgroup per kStartChunk codons: the sum of the chunk's pair
//                             values (int64) and the number of its candidates.  starts_top_kernel scans both over the chunks.
//   3. starts_cands_kernel    one lane per codon again: a workgroup scan in 64 bits behind the chunk's carry gives E[p], the sum of
//                             every pair value in front of codon p, and the candidate's place in the list -- the list is in (record,
//                             k) order.  Suf(k) = E[the record's last codon] - E[p]: a difference of two list-wide sums, so no
//                             segmented scan is needed and a record may span any number of chunks.  A candidate is (record, k, E,
//                             the 20 window codes and the type in one 64-bit word).
//      starts_window_kernel   one lane per candidate: the window codes (no lane without a window to read), and the cand counts of
//                             rule 6 in an 84-bin LDS histogram flushed once per workgroup.
//   4. per round              starts_count_kernel: one lane per candidate, the chosen counts into the same histogram;
//                             (host: counts down, weights up);
//                             starts_choose_kernel<false>: the score, a segmented wave maximum, one 64-bit atomicMax per wave and
//                             record; starts_choose_kernel<true>: the smallest k among the candidates that equal the maximum, the
//                             same way.
//   5. starts_chosen_kernel   one lane per candidate: Suf and the type of every record's chosen k > 0;
//      starts_apply_kernel    one lane per record: rule 9.  The proteins are then written by orf_residues_kernel from the new records,
//      and orf_keep_repaired_kernel puts the given bytes back where a record is a repaired one: it does not read in one frame.
// No lane walks a record: a 10^4-codon ORF is 10^4 lanes like any others, and its 10^4 candidates are 10^4 lanes of the rounds.
// A histogram add whose active lanes all hold one bin is one add of the lane count by one lane (coding_hist_add).
#pragma once

#include "kg_coding.hpp"

namespace kg {

constexpr int kStartThreads = 256;
constexpr int kStartSteps = 4;                                      // codons of one lane of the two codon passes
constexpr int kStartChunk = kStartThreads * kStartSteps;            // ... and of one workgroup
constexpr int kStartWin = 20;                                       // upstream positions of rule 4
constexpr int kStartBins = 4 * kStartWin + 4;                       // pos[20][4], then type[4]
constexpr uint32_t kStartMaxGrid = 2048;                            // workgroups of the striding candidate kernels
// error words: kCodingErr* of the record, then [4] the first record whose region does not fit it (rule 3)
enum { kStartErrLimit = kCodingErrWords, kStartErrWords = kCodingErrWords + 1 };
// counter words
enum { kStartCntMovable = 0, kStartCntTrain = 1, kStartCntCodons = 2, kStartCntCands = 3, kStartCntMoved = 4, kStartCntResidues = 5,
       kStartCntWords = 6 };
constexpr uint32_t kStartNone = 0xFFFFFFFFu;
constexpr uint8_t kStartMovable = 1, kStartTraining = 2;            // kind[i]

// where the limits of rule 3 come from: a region set (record i < n_regions belongs to region i), a list (-1: none), or neither
struct StartLimits {
    const kg_region *regions;
    uint64_t n_regions;
    const int32_t *limits;
};

__device__ __forceinline__ bool starts_movable(const kg_orf &o)
{
    return o.kept != 0 && o.start_codon != 0 && (o.flags & (KG_ORF_INTERRUPTED | KG_ORF_NONCODING)) == 0 && o.n_res >= 1;
}

// n = 3 or 6 bytes at p, all of them inside the batch, as a little-endian word
__device__ __forceinline__ uint64_t starts_bytes(const uint8_t *__restrict__ p, int n)
{
    uint16_t lo;
    __builtin_memcpy(&lo, p, 2);
    uint64_t w = (uint64_t)lo | ((uint64_t)p[2] << 16);
    if (n == 6) {
        uint16_t hi;
        __builtin_memcpy(&hi, p + 4, 2);
        w |= ((uint64_t)p[3] << 24) | ((uint64_t)hi << 32);
    }
    return w;
}

__global__ __launch_bounds__(256) void starts_lens_kernel(const kg_orf *__restrict__ orfs, uint64_t n, const int64_t *__restrict__ offsets,
                                                          uint64_t n_seqs, StartLimits lim, int32_t min_res, uint32_t *__restrict__ lens,
                                                          int32_t *__restrict__ kcap, uint8_t *__restrict__ kind, unsigned long long *err,
                                                          unsigned long long *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const kg_orf o = orfs[i];
    uint32_t len = 0;
    int32_t cap = 0;
    uint8_t what = 0;
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
            int64_t K = (int64_t)o.n_res - min_res;
            bool ok = true;
            if (lim.limits) {
                const int32_t l = lim.limits[i];
                if (l >= 0) K = l;
            } else if (i < lim.n_regions) {
                // the region's fields are compared and subtracted, never used as an index
                const kg_region r = lim.regions[i];
                const int64_t d = o.strand == 0 ? (int64_t)r.left - o.left : (int64_t)o.right - r.right;    // xa - xs
                if (r.seq != o.seq || r.strand != o.strand || d < -2) {      // ceil(d / 3) < 0
                    atomicMin(&err[kStartErrLimit], (unsigned long long)i);
                    ok = false;
                } else {
                    K = (d + 2) / 3;
                }
            }
            if (ok && starts_movable(o)) {
                len = (uint32_t)o.n_res;
                cap = (int32_t)(K < 0 ? 0 : K > (int64_t)o.n_res - 1 ? (int64_t)o.n_res - 1 : K);
                what = kStartMovable;
                atomicAdd(&cnt[kStartCntMovable], 1ull);
                if ((o.flags & (KG_ORF_FREE | KG_ORF_PARTIAL5)) == 0) {
                    what |= kStartTraining;
                    atomicAdd(&cnt[kStartCntTrain], 1ull);
                }
            }
        }
    }
    lens[i] = len;
    kcap[i] = cap;
    kind[i] = what;
}

// what the two codon passes read
struct StartBatch {
    const kg_orf *orfs;
    uint64_t n;
    const uint32_t *excl;               // the exclusive prefix of the movable records' codons
    const int32_t *kcap;
    const uint8_t *seq;
    const int64_t *offsets;
    uint32_t start_codons;
};

// Codon p of the list (p below the codon total, n > 0): its record (the last i with excl[i] <= p) and k, the value of pair k
// (0 for the last codon and for a pair with an unknown base), the codon's type and whether it is a candidate.  Only a record
// that passed starts_lens_kernel owns codons, so its fields are safe indices.
struct StartCodon {
    uint32_t rec;
    int32_t k;
    kg_orf o;
    long long v;
    uint32_t type;
    bool cand;
};

__device__ inline StartCodon starts_codon(const StartBatch &b, uint64_t p, const int32_t *tab)
{
    uint64_t lo = 0, hi = b.n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)b.excl[mid] > p) hi = mid; else lo = mid + 1;
    }
    StartCodon c;
    c.rec = (uint32_t)(lo - 1);
    c.o = b.orfs[c.rec];
    c.k = (int32_t)(p - b.excl[c.rec]);
    const int64_t off = b.offsets[c.o.seq];
    // The pair's six bases lie inside the record's extent (3 * n_res <= right - left + 1); the last codon has no pair and only
    // its own three are read.  '+': strand base j is byte a + j; '-': it is the complement of byte a - j.
    const int nb = c.k < c.o.n_res - 1 ? 6 : 3;
    const int64_t a = c.o.strand == 0 ? off + c.o.left + 3 * (int64_t)c.k : off + c.o.right - 3 * (int64_t)c.k;
    uint64_t w = starts_bytes(b.seq + (c.o.strand == 0 ? a : a - (nb - 1)), nb);
    if (c.o.strand != 0) w = __builtin_bswap64(w) >> (nb == 6 ? 16 : 40);
    uint32_t h = 0, code[3];
    bool known = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        uint32_t x = dna_code((uint32_t)(w >> (8 * j)) & 0xFFu);
        if (c.o.strand != 0 && x < 4) x = 3 - x;
        known = known && x < 4;
        h |= (x & 3u) << (2 * (5 - j));
        if (j < 3) code[j] = x;
    }
    c.v = (nb == 6 && known) ? (long long)tab[h] : 0;     // (without a pair, bases 3 .. 5 read as A: h stays an index)
    c.type = (code[1] == 3 && code[2] == 2) ? (code[0] == 0 ? 1u : code[0] == 2 ? 2u : code[0] == 3 ? 3u : 0u) : 0u;
    const bool start = c.type != 0 && ((b.start_codons >> (c.type - 1)) & 1u) != 0;
    c.cand = c.k == 0 || (start && c.k <= b.kcap[c.rec]);
    return c;
}

__device__ __forceinline__ void starts_load_table(int32_t *tab, const int32_t *__restrict__ T)
{
    for (int h = threadIdx.x; h < kCodingBins; h += kStartThreads) tab[h] = T[h];
    __syncthreads();
}

// partial_v[chunk] = the sum of the chunk's pair values, partial_c[chunk] = the number of its candidates.  P: the codon total.
__global__ __launch_bounds__(kStartThreads) void starts_pairs_kernel(StartBatch b, uint64_t P, const int32_t *__restrict__ T,
                                                                     unsigned long long *__restrict__ partial_v,
                                                                     unsigned long long *__restrict__ partial_c)
{
    __shared__ int32_t tab[kCodingBins];
    __shared__ unsigned long long wv[kStartThreads / 64], wc[kStartThreads / 64];
    starts_load_table(tab, T);
    unsigned long long v = 0, c = 0;
#pragma unroll 1
    for (int s = 0; s < kStartSteps; s++) {
        const uint64_t p = (uint64_t)blockIdx.x * kStartChunk + (uint64_t)s * kStartThreads + threadIdx.x;
        if (p < P) {
            const StartCodon x = starts_codon(b, p, tab);
            v += (unsigned long long)x.v;
            c += x.cand ? 1u : 0u;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        v += __shfl_xor(v, d);
        c += __shfl_xor(c, d);
    }
    if ((threadIdx.x & 63) == 0) { wv[threadIdx.x >> 6] = v; wc[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial_v[blockIdx.x] = wv[0] + wv[1] + wv[2] + wv[3];
        partial_c[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
    }
}

// the inclusive sum of the wave's lanes below and at `lane`
__device__ __forceinline__ unsigned long long starts_wave_scan(unsigned long long v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long y = __shfl_up(v, d);
        if (lane >= d) v += y;
    }
    return v;
}

// The exclusive sums of two values over the workgroup's lanes, from wave-uniform control flow; *tv, *tc: the workgroup's totals.
// (Signed values are added as unsigned ones: the sums are the same bits.)
__device__ inline void starts_block_scan(unsigned long long *wv, unsigned long long *wc, unsigned long long &v, unsigned long long &c,
                                         unsigned long long *tv, unsigned long long *tc)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long iv = starts_wave_scan(v, lane), ic = starts_wave_scan(c, lane);
    __syncthreads();                                    // (the words of the step before have been read)
    if (lane == 63) { wv[wave] = iv; wc[wave] = ic; }
    __syncthreads();
    unsigned long long bv = 0, bc = 0, sv = 0, sc = 0;
#pragma unroll
    for (int w = 0; w < kStartThreads / 64; w++) {
        if (w < wave) { bv += wv[w]; bc += wc[w]; }
        sv += wv[w]; sc += wc[w];
    }
    v = bv + iv - v;
    c = bc + ic - c;
    *tv = sv;
    *tc = sc;
}

// partial_v, partial_c -> their exclusive sums in place; the candidate total -> *cands
__global__ __launch_bounds__(kStartThreads) void starts_top_kernel(unsigned long long *partial_v, unsigned long long *partial_c,
                                                                   uint32_t n_chunks, unsigned long long *cands)
{
    __shared__ unsigned long long wv[kStartThreads / 64], wc[kStartThreads / 64];
    unsigned long long cv = 0, cc = 0;
    for (uint32_t base = 0; base < n_chunks; base += kStartThreads) {
        const uint32_t q = base + threadIdx.x;
        unsigned long long v = q < n_chunks ? partial_v[q] : 0, c = q < n_chunks ? partial_c[q] : 0, tv, tc;
        starts_block_scan(wv, wc, v, c, &tv, &tc);
        if (q < n_chunks) { partial_v[q] = cv + v; partial_c[q] = cc + c; }
        cv += tv;
        cc += tc;
    }
    if (threadIdx.x == 0) *cands = cc;
}

// the 84-bin histogram of rule 6, counted like the 4096 bins of the coding section
__device__ __forceinline__ void starts_hist_window(uint32_t *hist, bool on, uint64_t win)
{
    if (__ballot(on) == 0) return;
#pragma unroll
    for (int i = 0; i < kStartWin; i++) {
        const uint32_t x = (uint32_t)(win >> (3 * i)) & 7u;
        coding_hist_add(hist, on && x < 4, 4u * i + x);
    }
    const uint32_t type = (uint32_t)(win >> 60) & 3u;
    coding_hist_add(hist, on && type != 0, 4u * kStartWin + type);
}

__device__ __forceinline__ void starts_hist_flush(const uint32_t *hist, unsigned long long *out)
{
    __syncthreads();
    for (int b = threadIdx.x; b < kStartBins; b += kStartThreads)
        if (const uint32_t c = hist[b]) atomicAdd(&out[b], (unsigned long long)c);
}

// the candidate list
struct StartCands {
    uint32_t *rec;
    int32_t *k;
    uint64_t *win;                      // code i of the window in bits 3i .. 3i + 2, the type in bits 60 and 61
    int64_t *E;                         // the pair values in front of the candidate's codon
};

// the 20 window codes of codon k of record o (rule 4)
__device__ inline uint64_t starts_window(const StartBatch &b, const kg_orf &o, int32_t k)
{
    const int64_t off = b.offsets[o.seq], L = b.offsets[o.seq + 1] - off;
    const int64_t xs = o.strand == 0 ? (int64_t)o.left : L - 1 - o.right;
    const int64_t s0 = xs + 3 * (int64_t)k - kStartWin;             // the window's first strand position
    // '+': window position i is byte a + i; '-': it is the complement of byte a - i.  A position outside the contig reads the
    // contig's nearest byte instead and gets code 4: no branch, and no byte outside the contig is touched.
    const int64_t a = o.strand == 0 ? off + s0 : off + L - 1 - s0, step = o.strand == 0 ? 1 : -1;
    uint64_t win = 0;
#pragma unroll
    for (int i = 0; i < kStartWin; i++) {
        const int64_t s = s0 + i;                       // (s < L always: the window lies in front of a codon of the contig)
        const bool inside = s >= 0;
        uint32_t x = dna_code(b.seq[inside ? a + step * i : (o.strand == 0 ? off : off + L - 1)]);
        if (o.strand != 0 && x < 4) x = 3 - x;
        win |= (uint64_t)(inside ? x : 4u) << (3 * i);
    }
    return win;
}

// The candidate list in (record, k) order -- rec, k, E, and the type in win -- and E_end[i] = the pair values in front of the
// last codon of movable record i.
__global__ __launch_bounds__(kStartThreads) void starts_cands_kernel(StartBatch b, uint64_t P, const int32_t *__restrict__ T,
                                                                     const unsigned long long *__restrict__ partial_v,
                                                                     const unsigned long long *__restrict__ partial_c, uint64_t n_cands,
                                                                     StartCands out, int64_t *__restrict__ E_end)
{
    __shared__ int32_t tab[kCodingBins];
    __shared__ unsigned long long wv[kStartThreads / 64], wc[kStartThreads / 64];
    starts_load_table(tab, T);
    unsigned long long cv = partial_v[blockIdx.x], cc = partial_c[blockIdx.x];
#pragma unroll 1
    for (int s = 0; s < kStartSteps; s++) {
        const uint64_t p = (uint64_t)blockIdx.x * kStartChunk + (uint64_t)s * kStartThreads + threadIdx.x;
        StartCodon x;
        x.cand = false;
        x.v = 0;
        if (p < P) x = starts_codon(b, p, tab);
        unsigned long long v = (unsigned long long)x.v, c = x.cand ? 1u : 0u, tv, tc;
        starts_block_scan(wv, wc, v, c, &tv, &tc);
        const int64_t E = (int64_t)(cv + v);
        const uint64_t at = cc + c;
        if (p < P) {
            if (x.k == x.o.n_res - 1) E_end[x.rec] = E;
            if (x.cand && at < n_cands) {               // (at < n_cands always: the list was sized by these very flags)
                out.rec[at] = x.rec;
                out.k[at] = x.k;
                out.win[at] = (uint64_t)x.type << 60;
                out.E[at] = E;
            }
        }
        cv += tv;
        cc += tc;
    }
}

// One lane per candidate: the window codes into win, and cand_counts[84] += the windows and types of the training records'
// candidates.  Every lane has a window to read.
__global__ __launch_bounds__(kStartThreads) void starts_window_kernel(StartBatch b, StartCands cands, uint64_t n_cands,
                                                                      const uint8_t *__restrict__ kind, unsigned long long *cand_counts)
{
    __shared__ uint32_t hist[kStartBins];
    if (threadIdx.x < kStartBins) hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * kStartThreads; base < n_cands; base += (uint64_t)gridDim.x * kStartThreads) {
        const uint64_t q = base + threadIdx.x;
        bool train = false;
        uint64_t win = 0;
        if (q < n_cands) {
            const uint32_t rec = cands.rec[q];
            win = cands.win[q] | starts_window(b, b.orfs[rec], cands.k[q]);
            cands.win[q] = win;
            train = (kind[rec] & kStartTraining) != 0;
        }
        starts_hist_window(hist, train, win);
    }
    starts_hist_flush(hist, cand_counts);
}

// chosen_counts[84] += the window and type of every training record's chosen candidate
__global__ __launch_bounds__(kStartThreads) void starts_count_kernel(StartCands cands, uint64_t n_cands, const uint8_t *__restrict__ kind,
                                                                     const uint32_t *__restrict__ cur, unsigned long long *chosen_counts)
{
    __shared__ uint32_t hist[kStartBins];
    if (threadIdx.x < kStartBins) hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * kStartThreads; base < n_cands; base += (uint64_t)gridDim.x * kStartThreads) {
        const uint64_t q = base + threadIdx.x;
        bool on = false;
        uint64_t win = 0;
        if (q < n_cands) {
            const uint32_t rec = cands.rec[q];
            on = (kind[rec] & kStartTraining) != 0 && cur[rec] == (uint32_t)cands.k[q];
            win = cands.win[q];
        }
        starts_hist_window(hist, on, win);
    }
    starts_hist_flush(hist, chosen_counts);
}

// rule 5 as an unsigned key whose order is the score's
__device__ __forceinline__ unsigned long long starts_key(const int32_t *W, uint64_t win, long long suf)
{
    long long s = suf;
#pragma unroll
    for (int i = 0; i < kStartWin; i++) {
        const uint32_t x = (uint32_t)(win >> (3 * i)) & 7u;
        if (x < 4) s += W[4 * i + x];
    }
    s += W[4 * kStartWin + ((uint32_t)(win >> 60) & 3u)];
    return (unsigned long long)s ^ 0x8000000000000000ull;
}

// best[rec] = the largest key among the record's candidates (best[] zeroed); kPick: next[rec] = the smallest k among those whose
// key is best[rec] (next[] filled with kStartNone).  The list is sorted by record, so a wave holds runs of equal records: a
// segmented wave maximum (minimum) and one atomic per wave and run.
template <bool kPick>
__global__ __launch_bounds__(kStartThreads) void starts_choose_kernel(StartCands cands, uint64_t n_cands, const int64_t *__restrict__ E_end,
                                                                      const int32_t *__restrict__ weights, unsigned long long *best,
                                                                      uint32_t *next)
{
    __shared__ int32_t W[kStartBins];
    if (threadIdx.x < kStartBins) W[threadIdx.x] = weights[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kStartThreads; base < n_cands; base += (uint64_t)gridDim.x * kStartThreads) {
        const uint64_t q = base + threadIdx.x;
        uint32_t rec = kStartNone;
        unsigned long long key = 0;
        uint32_t k = kStartNone;
        if (q < n_cands) {
            rec = cands.rec[q];
            key = starts_key(W, cands.win[q], (long long)(E_end[rec] - cands.E[q]));
            if (kPick && key == best[rec]) k = (uint32_t)cands.k[q];
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ry = (uint32_t)__shfl_up((int)rec, d);
            if (kPick) {
                const uint32_t y = (uint32_t)__shfl_up((int)k, d);
                if (lane >= d && ry == rec && y < k) k = y;
            } else {
                const unsigned long long y = __shfl_up(key, d);
                if (lane >= d && ry == rec && y > key) key = y;
            }
        }
        const uint32_t after = (uint32_t)__shfl_down((int)rec, 1);
        if (rec != kStartNone && (lane == 63 || after != rec)) {
            if (kPick) {
                if (k != kStartNone) atomicMin(&next[rec], k);
            } else {
                atomicMax(&best[rec], key);
            }
        }
    }
}

// suf[rec], type[rec] of every record whose chosen k is above 0: one candidate, so one writer, per record
__global__ __launch_bounds__(kStartThreads) void starts_chosen_kernel(StartCands cands, uint64_t n_cands, const uint32_t *__restrict__ cur,
                                                                      const int64_t *__restrict__ E_end, int64_t *__restrict__ suf,
                                                                      uint32_t *__restrict__ type)
{
    for (uint64_t q = (uint64_t)blockIdx.x * kStartThreads + threadIdx.x; q < n_cands; q += (uint64_t)gridDim.x * kStartThreads) {
        const uint32_t rec = cands.rec[q];
        const int32_t k = cands.k[q];
        if (k > 0 && cur[rec] == (uint32_t)k) {
            suf[rec] = E_end[rec] - cands.E[q];
            type[rec] = (uint32_t)(cands.win[q] >> 60) & 3u;
        }
    }
}

// Rule 9.  cur == null: nothing was chosen (an untrained call), every shift is 0.  out_S: the set's coding scores (a copy of the
// given set's), or null.  new_lens[i]: the bytes of record i behind the new prot_start (null for a caller's list).
__global__ __launch_bounds__(256) void starts_apply_kernel(const kg_orf *__restrict__ in, uint64_t n, const uint8_t *__restrict__ kind,
                                                           const uint32_t *__restrict__ cur, const int64_t *__restrict__ suf,
                                                           const uint32_t *__restrict__ type, const int64_t *__restrict__ prot_start,
                                                           kg_orf *__restrict__ out, int32_t *__restrict__ shifts, int64_t *out_S,
                                                           uint32_t *new_lens, unsigned long long *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    kg_orf o = in[i];
    const uint32_t k = (cur && (kind[i] & kStartMovable) != 0) ? cur[i] : 0u;
    if (k > 0) {
        if (o.strand == 0) o.left += 3 * (int32_t)k; else o.right -= 3 * (int32_t)k;
        o.n_res -= (int32_t)k;
        o.start_codon = (int32_t)type[i];
        o.flags |= KG_ORF_START_MOVED;
        if (out_S) out_S[i] = suf[i];
        atomicAdd(&cnt[kStartCntMoved], 1ull);
    }
    out[i] = o;
    shifts[i] = (int32_t)k;
    if (new_lens) {
        const uint32_t len = (uint32_t)(prot_start[i + 1] - prot_start[i]);
        new_lens[i] = len - (k < len ? k : len);
    }
}

}  // namespace kg
