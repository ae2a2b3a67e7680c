// kg_derive.hpp -- device side of kg_signatures_derive / kg_signatures_derive_device (include/kmerguts_hip.h): annotated
// proteins -> the signature k-mers of a KmerGuts table (the semantics are stated in the header, next to the entry points).
//
// Proteins are ranked by (fn, otu, p) first (a radix sort of (fn + 1, otu) keys carrying p, stable), so that one 64-bit key
//     key = (v - range_lo) * 2^b + rank(p)          (b = ceil(log2 n_prot) <= 29, v < 20^8 < 2^35)
// sorts a window into (k-mer, function, OTU, protein) order.  Every later step is run-length arithmetic on the sorted keys.
//
//   1. derive_windows_kernel<false>  histogram of the valid windows' k-mers over a k-mer range (the host cuts the k-mer
//                                    space into passes of at most max_windows_per_pass windows with it, refining a bin
//                                    that is too full)
//   2. derive_windows_kernel<true>   per pass: encode (encode_block<true>, the scan's own -a encode) and emit (key, len_p - i)
//                                    for the windows in the pass's range, compacted with one ballot and one atomic per wave
//   3. the LSD radix sort of kg_build.hpp (build_hist_kernel / prefix_sum / build_scatter_kernel)
//   4. derive_collapse_kernel        equal keys (one protein's repeats of a k-mer) -> one pair keeping the largest len_p - i
//                                    = len_p - i_p(v); the emission order does not matter
//   5. derive_run_flags_kernel       run heads of the pairs at three levels: k-mer, (k-mer, fn), (k-mer, fn, otu); prefix
//                                    sums number the runs; derive_run_starts_kernel writes each run's first pair
//   6. derive_run_sums_kernel        sum of len_p - i_p(v) per (k-mer, fn) run
//      derive_fn_best_kernel         per (k-mer, fn >= 0) run: atomicMax of (c_f, -run) on its k-mer: f* with its smallest f
//      derive_otu_best_kernel        per OTU run inside the f* run: atomicMax of (count, -otu): the mode with its smallest OTU
//   7. derive_select_kernel          per k-mer: the signature test; a prefix sum places the signatures in k-mer order
//
// Runs are never given to one thread or one workgroup: the segmented steps (4, 6) take 16 consecutive items per thread and
// meet at run boundaries through plain stores (a run wholly inside the thread's items) or atomics (a run that crosses one),
// so a k-mer in 10^6 proteins costs what its items cost.
#pragma once

#include "kg_device.hpp"
#include "kg_build.hpp"

namespace kg {

constexpr int kDeriveThreads = kWave * kWavesPerWG;
constexpr uint32_t kDeriveBins = 4096;              // histogram bins per k-mer range
constexpr int kDeriveChunk = 16;                    // consecutive items per thread in the segmented steps

// rank keys: (fn + 1) * 2^31 + otu (otu counts only where fn >= 0), carrying the protein index
__global__ __launch_bounds__(256) void derive_rank_keys_kernel(const int32_t *__restrict__ fn, const int32_t *__restrict__ otu,
                                                               uint64_t n, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t f = fn[i];
    keys[i] = ((uint64_t)((uint32_t)f + 1u) << 31) | (uint64_t)(f >= 0 ? (uint32_t)otu[i] : 0u);
    vals[i] = (uint32_t)i;
}

// sorted order j -> rank_of[p_j] = j, fn_r[j] = fn[p_j], otu_r[j] = otu[p_j] (0 for an unannotated protein)
__global__ __launch_bounds__(256) void derive_rank_scatter_kernel(const uint32_t *__restrict__ order, const int32_t *__restrict__ fn,
                                                                  const int32_t *__restrict__ otu, uint64_t n, uint32_t *__restrict__ rank_of,
                                                                  int32_t *__restrict__ fn_r, int32_t *__restrict__ otu_r)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t p = order[j];
    if (p >= n) return;
    rank_of[p] = (uint32_t)j;
    fn_r[j] = fn[p];
    otu_r[j] = fn[p] >= 0 ? otu[p] : 0;
}

// One wave per window block (64 windows of one protein), grid-stride over the blocks.  Window i of protein p is valid as in
// an -a scan (row_halves<true>: i < len - 8, no code >= 20).  Of the valid windows with lo <= v < hi:
//   EMIT = false: bins[(v - lo) >> shift] += 1 (LDS, then one global atomic per non-empty bin and workgroup)
//   EMIT = true : keys[o] = (v - lo) << b | rank_of[p], vals[o] = len_p - i at o = *cursor++ (o < cap always holds when the
//                 histogram was right; checked anyway)
template <bool EMIT>
__global__ __launch_bounds__(kDeriveThreads) void derive_windows_kernel(const uint8_t *__restrict__ seq, const BlockDesc *__restrict__ blocks,
                                                                        uint32_t n_blocks, uint64_t lo, uint64_t hi, uint32_t shift,
                                                                        unsigned long long *__restrict__ bins, const uint32_t *__restrict__ rank_of,
                                                                        uint32_t b, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                                        unsigned long long *cursor, uint64_t cap)
{
    __shared__ EncTablesAa enc_tables;
    __shared__ WaveLdsAa lds[kWavesPerWG];
    __shared__ uint32_t h[EMIT ? 1 : kDeriveBins];
    encode_init<true>(enc_tables, threadIdx.x, blockDim.x);
    if (!EMIT)
        for (uint32_t k = threadIdx.x; k < kDeriveBins; k += blockDim.x) h[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    WaveLdsAa &l = lds[wave];
    const uint64_t lt = (1ull << lane) - 1;
    for (uint32_t it = blockIdx.x * kWavesPerWG + wave; it < n_blocks; it += gridDim.x * kWavesPerWG) {
        const BlockDesc bd = blocks[it];
        encode_block<true>(l, enc_tables, seq, bd, lane);
        uint32_t hh, ll;
        const bool valid = row_halves<true>(l, 0, lane, bd, &hh, &ll);
        const uint64_t v = (uint64_t)hh * 160000ull + ll;
        const bool in = valid && v >= lo && v < hi;
        if (!EMIT) {
            if (in) atomicAdd(&h[(uint32_t)((v - lo) >> shift)], 1u);
        } else {
            const uint64_t m = __ballot(in);
            unsigned long long base = 0;
            if (lane == 0 && m) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
            base = __shfl(base, 0);
            const uint64_t o = base + (uint64_t)__popcll(m & lt);
            if (in && o < cap) {
                const uint32_t i = bd.j * kAaWinPerBlock + (uint32_t)lane;
                keys[o] = ((v - lo) << b) | rank_of[bd.seq];
                vals[o] = bd.len - i;
            }
        }
        wave_sync();                                    // the wave's LDS is rewritten by its next block
    }
    if (!EMIT) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < kDeriveBins; k += blockDim.x)
            if (h[k]) atomicAdd(&bins[k], (unsigned long long)h[k]);
    }
}

// flags[j] = 1 where key j starts a run of equal keys
__global__ __launch_bounds__(256) void derive_key_heads_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint32_t *__restrict__ flags)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    flags[j] = (j == 0 || keys[j] != keys[j - 1]) ? 1u : 0u;
}

// Pair p = the p-th run of equal keys (pidx = exclusive scan of the heads): pk[p] = its key, pv[p] = the largest val of the run
// (pv zeroed beforehand; vals are >= 9).  Thread t takes items [16 t, 16 t + 16).
__global__ __launch_bounds__(256) void derive_collapse_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t n,
                                                              const uint32_t *__restrict__ pidx, uint64_t *__restrict__ pk, uint32_t *__restrict__ pv)
{
    const uint64_t base = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kDeriveChunk;
    if (base >= n) return;
    const uint64_t end = base + kDeriveChunk < n ? base + kDeriveChunk : n;
    uint64_t ck = keys[base];
    bool head = base == 0 || keys[base - 1] != ck;
    uint32_t m = vals[base];
    uint32_t p = pidx[base] + (head ? 1u : 0u) - 1u;
    if (head) pk[p] = ck;
    for (uint64_t j = base + 1; j < end; j++) {
        const uint64_t k = keys[j];
        const uint32_t v = vals[j];
        if (k != ck) {
            if (head) pv[p] = m; else atomicMax(&pv[p], m);
            ck = k; head = true; m = v; p++;
            pk[p] = k;
        } else {
            m = v > m ? v : m;
        }
    }
    if (head && (end == n || keys[end] != ck)) pv[p] = m;
    else atomicMax(&pv[p], m);
}

struct DeriveRun {      // the three run levels of pair j
    bool kh, fh, oh;
    int32_t f, o;
};

__device__ __forceinline__ DeriveRun derive_heads(const uint64_t *__restrict__ pk, uint64_t j, uint32_t b, const int32_t *__restrict__ fn_r,
                                                  const int32_t *__restrict__ otu_r)
{
    const uint64_t rmask = (1ull << b) - 1;
    const uint64_t k = pk[j];
    DeriveRun r;
    r.f = fn_r[k & rmask];
    r.o = otu_r[k & rmask];
    if (j == 0) { r.kh = r.fh = r.oh = true; return r; }
    const uint64_t q = pk[j - 1];
    r.kh = (k >> b) != (q >> b);
    r.fh = r.kh || fn_r[q & rmask] != r.f;
    r.oh = r.fh || otu_r[q & rmask] != r.o;
    return r;
}

__global__ __launch_bounds__(256) void derive_run_flags_kernel(const uint64_t *__restrict__ pk, uint64_t n, uint32_t b,
                                                               const int32_t *__restrict__ fn_r, const int32_t *__restrict__ otu_r,
                                                               uint32_t *__restrict__ kh, uint32_t *__restrict__ fh, uint32_t *__restrict__ oh)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const DeriveRun r = derive_heads(pk, j, b, fn_r, otu_r);
    kh[j] = r.kh; fh[j] = r.fh; oh[j] = r.oh;
}

// kx / fx / ox = exclusive scans of the heads; *_total = their totals (device).  Writes the first pair of every run (and the
// end sentinel behind the last run of each level), the k-mer run of every fn run, the fn run of every OTU run and the values.
__global__ __launch_bounds__(256) void derive_run_starts_kernel(const uint64_t *__restrict__ pk, uint64_t n, uint32_t b,
                                                                const int32_t *__restrict__ fn_r, const int32_t *__restrict__ otu_r,
                                                                const uint32_t *__restrict__ kx, const uint32_t *__restrict__ fx,
                                                                const uint32_t *__restrict__ ox, const uint64_t *__restrict__ k_total,
                                                                const uint64_t *__restrict__ f_total, const uint64_t *__restrict__ o_total,
                                                                uint32_t *__restrict__ kstart, uint32_t *__restrict__ fstart,
                                                                uint32_t *__restrict__ f_kmer, int32_t *__restrict__ f_fn,
                                                                uint32_t *__restrict__ ostart, uint32_t *__restrict__ o_frun,
                                                                int32_t *__restrict__ o_otu)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) {
        kstart[*k_total] = (uint32_t)n;
        fstart[*f_total] = (uint32_t)n;
        ostart[*o_total] = (uint32_t)n;
    }
    if (j >= n) return;
    const DeriveRun r = derive_heads(pk, j, b, fn_r, otu_r);
    if (r.kh) kstart[kx[j]] = (uint32_t)j;
    if (r.fh) {
        const uint32_t fi = fx[j];
        fstart[fi] = (uint32_t)j;
        f_kmer[fi] = kx[j] + (r.kh ? 1u : 0u) - 1u;
        f_fn[fi] = r.f;
    }
    if (r.oh) {
        const uint32_t oi = ox[j];
        ostart[oi] = (uint32_t)j;
        o_frun[oi] = fx[j] + (r.fh ? 1u : 0u) - 1u;
        o_otu[oi] = r.o;
    }
}

// fsum[fn run] = sum of pv over its pairs (fsum zeroed beforehand); 16 consecutive pairs per thread
__global__ __launch_bounds__(256) void derive_run_sums_kernel(const uint32_t *__restrict__ pv, uint64_t n, const uint32_t *__restrict__ fh,
                                                              const uint32_t *__restrict__ fx, unsigned long long *__restrict__ fsum)
{
    const uint64_t base = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kDeriveChunk;
    if (base >= n) return;
    const uint64_t end = base + kDeriveChunk < n ? base + kDeriveChunk : n;
    bool head = fh[base] != 0;
    uint32_t r = fx[base] + (head ? 1u : 0u) - 1u;
    unsigned long long s = pv[base];
    for (uint64_t j = base + 1; j < end; j++) {
        if (fh[j]) {
            if (head) fsum[r] = s; else atomicAdd(&fsum[r], s);
            head = true; r++; s = 0;
        }
        s += pv[j];
    }
    if (head && (end == n || fh[end])) fsum[r] = s;
    else atomicAdd(&fsum[r], s);
}

// kbest[k] = max over the fn runs of k-mer k with fn >= 0 of (c_f << 32 | ~run): the largest c_f, on a tie the first run = the
// smallest f (runs are in fn order).  0 = no annotated protein.
__global__ __launch_bounds__(256) void derive_fn_best_kernel(const uint32_t *__restrict__ fstart, const uint32_t *__restrict__ f_kmer,
                                                             const int32_t *__restrict__ f_fn, uint64_t n_f, unsigned long long *__restrict__ kbest)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_f || f_fn[i] < 0) return;
    const unsigned long long c = fstart[i + 1] - fstart[i];
    atomicMax(&kbest[f_kmer[i]], (c << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i));
}

// kotu[k] = max over the OTU runs inside k's f* run of (count << 32 | ~otu): the most frequent OTU, on a tie the smallest
__global__ __launch_bounds__(256) void derive_otu_best_kernel(const uint32_t *__restrict__ ostart, const uint32_t *__restrict__ o_frun,
                                                              const int32_t *__restrict__ o_otu, uint64_t n_o, const uint32_t *__restrict__ f_kmer,
                                                              const unsigned long long *__restrict__ kbest, unsigned long long *__restrict__ kotu)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_o) return;
    const uint32_t fi = o_frun[i];
    const uint32_t k = f_kmer[fi];
    const unsigned long long kb = kbest[k];
    if (kb == 0 || 0xFFFFFFFFu - (uint32_t)kb != fi) return;
    const unsigned long long c = ostart[i + 1] - ostart[i];
    atomicMax(&kotu[k], (c << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)o_otu[i]));
}

// Per k-mer k: n_v = its pairs, c = c_f*.  A signature iff f* exists, n_v >= min_proteins and 100 c >= purity_pct n_v.
//   EMIT = false: flags[k] = 1 for a signature;  EMIT = true: out[sidx[k]] = its record
template <bool EMIT>
__global__ __launch_bounds__(256) void derive_select_kernel(uint64_t n_k, const uint32_t *__restrict__ kstart,
                                                            const unsigned long long *__restrict__ kbest, const unsigned long long *__restrict__ kotu,
                                                            const unsigned long long *__restrict__ fsum, const int32_t *__restrict__ f_fn,
                                                            const uint64_t *__restrict__ pk, uint32_t b, uint64_t lo, int64_t min_proteins,
                                                            int64_t purity_pct, uint32_t *__restrict__ flags, const uint32_t *__restrict__ sidx,
                                                            uint8_t *__restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_k) return;
    const uint32_t first = kstart[k];
    const int64_t n = (int64_t)(kstart[k + 1] - first);
    const unsigned long long kb = kbest[k];
    const int64_t c = (int64_t)(kb >> 32);
    const bool sig = kb != 0 && n >= min_proteins && 100 * c >= purity_pct * n;
    if (!EMIT) {
        flags[k] = sig ? 1u : 0u;
        return;
    }
    if (!sig) return;
    const uint32_t fi = 0xFFFFFFFFu - (uint32_t)kb;
    const int64_t kmer = (int64_t)(lo + (pk[first] >> b));
    const int32_t otu = (int32_t)(0xFFFFFFFFu - (uint32_t)kotu[k]);
    const int32_t avg = (int32_t)(fsum[fi] / (unsigned long long)c);
    const float wt = __fdiv_rn((float)c, (float)n);
    uint2 *dst = reinterpret_cast<uint2 *>(out + (uint64_t)sidx[k] * 24);
    dst[0] = make_uint2((uint32_t)kmer, (uint32_t)((uint64_t)kmer >> 32));
    dst[1] = make_uint2((uint32_t)otu, (uint32_t)avg);
    dst[2] = make_uint2((uint32_t)f_fn[fi], __float_as_uint(wt));
}

}  // namespace kg
