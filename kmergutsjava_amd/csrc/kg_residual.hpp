// kg_residual.hpp -- device side of kg_contigs_search_residual / kg_result_search_residual (include/kmerguts_hip.h states the
// rule): the stop-to-stop fragments that a list of signature CALLs has not explained are compacted into an ORF set of their own,
// searched as kg_contigs_search_translated searches all of them, and the two kinds of CALL are merged by container.  The
// fragments are the records of orf_free_kernel (kg_orfs.hpp), the hit records those of the search and the homology CALLs those
// of evidence_flag_kernel / evidence_emit_kernel (kg_evidence.hpp), all launched as they are; what is new lies around them:
//
//   1. residual_keys_kernel     per fragment F: key[F] = (c(F) << 32) | (b(F) + n_res - 1), its container and last codon, and
//                               first[F] = b(F); explain[F] = 0.  The fragments are sorted by (c, b) and disjoint within a
//                               container, so key[] ascends strictly: what the CALLs search in.
//   2. residual_mark_kernel     one lane per signature CALL s: validation (error words by atomicMin, firing only on bad input; a
//                               bad record marks nothing), a binary search for the first fragment with key >= (s.container,
//                               s.start), then a walk forward while the fragment lies in the container and first <= s.end, adding
//                               s.count to explain[F] with one 64-bit integer atomic each.  The walk is one or two fragments in
//                               practice and as long as the CALL spans fragments.
//   3. residual_choose_kernel   per fragment: flag[F] = explain[F] < explain_min (searched), len[F] = flag ? n_res : 0.  Two shared
//                               prefix sums (kg_device.hpp) follow: over flag for the query index and their number, over len for
//                               the new prot_start and the searched residues.  The fragments' residues are below 2^32
//                               (kg_orfs_free refuses more), so the 32-bit prefix is exact and the 64-bit total is the shared
//                               sum's own.
//   4. residual_layout_kernel   per searched fragment: its record to out[q], new_start[q], searched[q] = F; one more lane writes
//                               new_start[n_q].
//   5. residual_copy_kernel     the residues, divided by destination position: a lane owns kResidualChunk = 16 consecutive
//                               destination bytes, finds their fragment by binary search in new_start and writes them with one
//                               16-byte store (the destination block is aligned and a chunk starts at a multiple of 16).  A chunk
//                               inside one fragment -- three of four at 70 residues a fragment -- reads its source as four or
//                               five aligned dwords around an arbitrary source offset and shifts; a chunk across fragment
//                               borders reads byte by byte and changes fragment as orf_residues_kernel does.  Consecutive lanes
//                               read and write consecutive bytes; no lane walks more than its 16 bytes.
//   6. residual_keep_kernel     per homology CALL: keep[j] = count >= min_db_count; the shared prefix sum gives the kept ones'
//                               ranks and their number.
//   7. residual_merge_kernel    one lane per CALL of either list.  Both lists ascend by container, so a signature CALL i of
//                               container c lies behind the kept homology CALLs of containers below c (a binary search in the
//                               homology list), and kept homology CALL j behind the signature CALLs of containers up to its own:
//                               every merged CALL, kind, source and hit has one writer.
//
// Order cannot matter: explain[] is a sum of integers, and every other word has one writer.  No LDS.
#pragma once

#include "kg_device.hpp"
#include "kg_orfs.hpp"
#include "kg_regions.hpp"

namespace kg {

constexpr int kResidualChunk = 16;      // destination bytes of one lane of residual_copy_kernel
// error words: the first signature CALL (index in the list) [0] whose container is below its predecessor's, [1] whose container
// is 6 * n_seqs or more, [2] with a negative count, [3] with start > end, [4] outside its contig
enum { kResidualErrOrder = 0, kResidualErrContainer = 1, kResidualErrCount = 2, kResidualErrEnds = 3, kResidualErrRange = 4, kResidualErrWords = 5 };
// the words behind them: the searched fragments, their residues, the kept homology CALLs
enum { kResidualQueries = 5, kResidualResidues = 6, kResidualKept = 7, kResidualWords = 8 };

// off[n_seqs + 1] the contigs' offsets; n_seqs >= 1 whenever n >= 1
__global__ __launch_bounds__(256) void residual_keys_kernel(const kg_orf *__restrict__ frags, uint64_t n, const int64_t *__restrict__ off,
                                                            uint32_t n_seqs, uint64_t *__restrict__ key, int32_t *__restrict__ first,
                                                            unsigned long long *__restrict__ explain)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const kg_orf f = frags[i];
    const uint32_t s = min((uint32_t)f.seq, n_seqs - 1);
    const int64_t len = off[s + 1] - off[s];
    const int64_t x = f.strand ? len - 1 - f.right : f.left;     // the fragment's first nucleotide on its own strand
    const int32_t b = (int32_t)((x - f.frame) / 3);
    const uint32_t c = 6u * (uint32_t)f.seq + 3u * (uint32_t)f.strand + (uint32_t)f.frame;
    key[i] = ((uint64_t)c << 32) | (uint32_t)(b + f.n_res - 1);
    first[i] = b;
    explain[i] = 0;
}

__global__ __launch_bounds__(256) void residual_mark_kernel(const kg_call *__restrict__ calls, uint64_t n, const int64_t *__restrict__ off,
                                                            uint64_t n_seqs, const uint64_t *__restrict__ key,
                                                            const int32_t *__restrict__ first, uint64_t n_frags,
                                                            unsigned long long *__restrict__ explain, unsigned long long *err)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const kg_call c = calls[i];
    bool ok = true;
    if (i > 0 && calls[i - 1].container > c.container) atomicMin(&err[kResidualErrOrder], (unsigned long long)i);
    if ((uint64_t)c.container >= 6 * n_seqs) { atomicMin(&err[kResidualErrContainer], (unsigned long long)i); ok = false; }
    if (c.count < 0) { atomicMin(&err[kResidualErrCount], (unsigned long long)i); ok = false; }
    if (c.start > c.end) {
        atomicMin(&err[kResidualErrEnds], (unsigned long long)i);
        ok = false;
    } else if (!region_span(c, off, n_seqs).ok) {        // (the span's own indices are clamped)
        atomicMin(&err[kResidualErrRange], (unsigned long long)i);
        ok = false;
    }
    if (!ok) return;
    const uint64_t want = ((uint64_t)c.container << 32) | (uint32_t)c.start;
    uint64_t lo = 0, hi = n_frags;       // key[k] < want for k < lo, key[k] >= want for k >= hi
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (key[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    for (uint64_t k = lo; k < n_frags && (uint32_t)(key[k] >> 32) == c.container && first[k] <= c.end; k++)
        atomicAdd(&explain[k], (unsigned long long)c.count);
}

__global__ __launch_bounds__(256) void residual_choose_kernel(const unsigned long long *__restrict__ explain, const kg_orf *__restrict__ frags,
                                                              uint64_t n, int64_t explain_min, uint32_t *__restrict__ flag,
                                                              uint32_t *__restrict__ len)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool searched = (int64_t)explain[i] < explain_min;
    flag[i] = searched ? 1u : 0u;
    len[i] = searched ? (uint32_t)frags[i].n_res : 0u;
}

// totals[0] = n_q, totals[1] = the searched residues (the two prefix sums' totals); out[max(n_q, 1)], new_start[n_q + 1], searched[max(n_q, 1)]
__global__ __launch_bounds__(256) void residual_layout_kernel(const kg_orf *__restrict__ frags, const uint32_t *__restrict__ flag,
                                                              const uint32_t *__restrict__ qidx, const uint32_t *__restrict__ excl,
                                                              const uint64_t *__restrict__ totals, uint64_t n, kg_orf *__restrict__ out,
                                                              int64_t *__restrict__ new_start, int64_t *__restrict__ searched)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const uint64_t n_q = totals[0];
    if (i == n) { new_start[n_q] = (int64_t)totals[1]; return; }
    if (!flag[i]) return;
    const uint64_t q = qidx[i];
    if (q >= n_q) return;                // (cannot happen: the sum's total counts every flag)
    out[q] = frags[i];
    new_start[q] = (int64_t)excl[i];
    searched[q] = (int64_t)i;
}

// the aligned dword at q, which holds at least one byte of src[0 .. total): whole where it lies inside, else its bytes inside
__device__ inline uint32_t residual_dword(const uint8_t *__restrict__ src, uint64_t total, const uint8_t *q)
{
    const uint8_t *end = src + total;
    if (q >= src && q + 4 <= end) return *reinterpret_cast<const uint32_t *>(q);
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (q + b >= src && q + b < end) w |= (uint32_t)q[b] << (8 * b);
    return w;
}

// src[src_total]: all fragments' residues behind old_start; dst[total]: the searched ones' behind new_start[n_q + 1] (n_q >= 1,
// total >= 1); searched[q] < n_frags.  dst is 16-byte aligned.
__global__ __launch_bounds__(256) void residual_copy_kernel(const uint8_t *__restrict__ src, uint64_t src_total,
                                                            const int64_t *__restrict__ old_start, uint64_t n_frags,
                                                            const int64_t *__restrict__ searched, const int64_t *__restrict__ new_start,
                                                            uint64_t n_q, uint64_t total, uint8_t *__restrict__ dst)
{
    const uint64_t at = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kResidualChunk;
    if (at >= total) return;
    uint64_t q = orf_owner(new_start, n_q, (int64_t)at);
    int64_t begin = new_start[q], end = new_start[q + 1];
    int64_t from = old_start[min((uint64_t)searched[q], n_frags - 1)];     // the source of destination byte p is from + (p - begin)
    uint32_t w[4] = {0, 0, 0, 0};
    int k = 0;
    if ((int64_t)at + kResidualChunk <= end && (uint64_t)(from + ((int64_t)at - begin)) + kResidualChunk <= src_total) {
        const uint8_t *p = src + from + ((int64_t)at - begin);
        const uint8_t *p4 = (const uint8_t *)((uintptr_t)p & ~(uintptr_t)3);
        const uint32_t sh = (uint32_t)(p - p4) * 8;
        uint32_t d[5];
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = residual_dword(src, src_total, p4 + 4 * j);
        d[4] = sh ? residual_dword(src, src_total, p4 + 16) : 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) w[j] = sh ? (d[j] >> sh) | (d[j + 1] << (32 - sh)) : d[j];
        k = kResidualChunk;
    } else {
        for (; k < kResidualChunk && at + k < total; k++) {
            const int64_t pos = (int64_t)(at + k);
            if (pos >= end) {
                // the neighbour first (short fragments), else a new search: nothing is empty here, min_res >= 1
                q = (q + 2 <= n_q && new_start[q + 1] <= pos && pos < new_start[q + 2]) ? q + 1 : orf_owner(new_start, n_q, pos);
                begin = new_start[q];
                end = new_start[q + 1];
                from = old_start[min((uint64_t)searched[q], n_frags - 1)];
            }
            const uint64_t a = (uint64_t)(from + (pos - begin));
            const uint32_t ch = a < src_total ? src[a] : 0u;
            w[k >> 2] |= ch << (8 * (k & 3));
        }
    }
    if (k == kResidualChunk) {
        *reinterpret_cast<uint4 *>(dst + at) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int b = 0; b < k; b++) dst[at + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
}

__global__ __launch_bounds__(256) void residual_keep_kernel(const kg_call *__restrict__ db_calls, uint64_t n, int32_t min_db_count,
                                                            uint32_t *__restrict__ keep)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) keep[j] = db_calls[j].count >= min_db_count ? 1u : 0u;
}

// calls[k].container of a sorted list: the first k in [0, n) with container >= c (upper = false) or > c (upper = true), else n
__device__ inline uint64_t residual_bound(const kg_call *__restrict__ calls, uint64_t n, uint32_t c, bool upper)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const uint32_t m = calls[mid].container;
        if (upper ? m <= c : m < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// sig[n_sig] and db[n_db] ascend by container; keep / kpos[n_db]: residual_keep_kernel's flags and their exclusive sum, *n_kept its
// total; db_hit[n_db]: the hit record of every homology CALL.  out / kind / source / hit: n_sig + *n_kept records.
__global__ __launch_bounds__(256) void residual_merge_kernel(const kg_call *__restrict__ sig, uint64_t n_sig, const kg_call *__restrict__ db,
                                                             uint64_t n_db, const uint32_t *__restrict__ keep,
                                                             const uint32_t *__restrict__ kpos, const uint64_t *__restrict__ n_kept,
                                                             const int64_t *__restrict__ db_hit, kg_call *__restrict__ out,
                                                             uint8_t *__restrict__ kind, int64_t *__restrict__ source,
                                                             int64_t *__restrict__ hit)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sig + n_db) return;
    const uint64_t total = n_sig + *n_kept;
    if (i < n_sig) {
        const kg_call c = sig[i];
        const uint64_t below = residual_bound(db, n_db, c.container, false);      // homology CALLs of containers below c
        const uint64_t k = i + (below < n_db ? (uint64_t)kpos[below] : *n_kept);
        if (k >= total) return;
        out[k] = c;
        kind[k] = 0;
        source[k] = (int64_t)i;
        hit[k] = -1;
    } else {
        const uint64_t j = i - n_sig;
        if (!keep[j]) return;
        const kg_call c = db[j];
        const uint64_t k = (uint64_t)kpos[j] + residual_bound(sig, n_sig, c.container, true);
        if (k >= total) return;
        out[k] = c;
        kind[k] = 1;
        source[k] = (int64_t)j;
        hit[k] = db_hit[j];
    }
}

}  // namespace kg
