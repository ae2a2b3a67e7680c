// kg_evidence.hpp -- device side of kg_contigs_search_translated (include/kmerguts_hip.h states the rule): the hit records of a
// translated search made into the CALL records the region, ORF, repair and selection stages read.  The fragments are the records
// of orf_free_kernel (kg_orfs.hpp) and the hit records and paths those of the search against the resident index
// (kg_searchdb.hpp, kg_trace.hpp), both launched as they are; what is new is the stage between the two record kinds:
//
//   1. evidence_flag_kernel   per hit record r: keep[r] = 1 iff the record is a hit, of rank below max_hits, with a traced path.
//                             The first test that fails names the drop (status, then rank, then untraced); the three drop counts
//                             are one ballot each and one integer atomic per wave and count
//   2. prefix_sum             the shared exclusive sum (kg_device.hpp) over keep: the place of every kept record, and their number
//   3. evidence_emit_kernel   per kept record: its fragment's record gives the container and b, the fragment's first codon in its
//                             frame; CALL pos[r] = (container, b + start_a, b + end_query, score, fI, (float) score) and
//                             call_hit[pos[r]] = r
//
// What bounds a lane's work: one record per lane in both kernels, no loop.  The flag kernel reads 12 of a record's 72 bytes (hit
// and path), the emit kernel a kept record's hit, path and fragment record once; consecutive lanes read consecutive hit and path
// records, and consecutive kept records of one query the same fragment record.  Order cannot matter: the counts are integer sums
// and every CALL has one writer.  A record's fragment, contig and target are clamped before they are used as indices.
// No LDS.
#pragma once

#include "kg_device.hpp"

namespace kg {

// the counter words of the stage: the three drop counts, then the prefix sum's total (the CALLs)
enum : int { kEvidenceDropStatus = 0, kEvidenceDropRank = 1, kEvidenceDropUntraced = 2, kEvidenceCalls = 3, kEvidenceWords = 4 };

__global__ __launch_bounds__(256) void evidence_flag_kernel(const kg_search_hit *__restrict__ hits, const kg_alignment_path *__restrict__ paths,
                                                            uint64_t n, int32_t max_hits, uint32_t *__restrict__ keep,
                                                            unsigned long long *__restrict__ words)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = r < n;
    int32_t status = 0, rank = 0, traced = 0;
    if (in) {
        status = hits[r].status;
        rank = hits[r].rank;
        traced = paths[r].status;
    }
    const bool by_status = in && status != 0;
    const bool by_rank = in && !by_status && rank >= max_hits;
    const bool by_trace = in && !by_status && !by_rank && traced != 0;
    if (in) keep[r] = by_status || by_rank || by_trace ? 0u : 1u;
    const unsigned long long ms = __ballot(by_status), mr = __ballot(by_rank), mt = __ballot(by_trace);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (ms) atomicAdd(&words[kEvidenceDropStatus], (unsigned long long)__popcll(ms));
        if (mr) atomicAdd(&words[kEvidenceDropRank], (unsigned long long)__popcll(mr));
        if (mt) atomicAdd(&words[kEvidenceDropUntraced], (unsigned long long)__popcll(mt));
    }
}

// frags[n_frags] (n_frags >= 1 whenever n >= 1), off[n_seqs + 1] the contigs' offsets, fn[n_db] or null
__global__ __launch_bounds__(256) void evidence_emit_kernel(const kg_search_hit *__restrict__ hits, const kg_alignment_path *__restrict__ paths,
                                                            uint64_t n, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos,
                                                            const kg_orf *__restrict__ frags, uint32_t n_frags, const int64_t *__restrict__ off,
                                                            uint32_t n_seqs, const int32_t *__restrict__ fn, uint32_t n_db,
                                                            kg_call *__restrict__ calls, int64_t *__restrict__ call_hit)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n || !keep[r]) return;
    const kg_search_hit h = hits[r];
    const kg_orf f = frags[min((uint32_t)h.query, n_frags - 1)];
    const uint32_t s = min((uint32_t)f.seq, n_seqs - 1);
    const int64_t len = off[s + 1] - off[s];
    const int64_t x = f.strand ? len - 1 - f.right : f.left;     // the fragment's first nucleotide on its own strand
    const int32_t b = (int32_t)((x - f.frame) / 3);
    kg_call c;
    c.container = 6u * (uint32_t)f.seq + 3u * (uint32_t)f.strand + (uint32_t)f.frame;
    c.start = b + paths[r].start_a;
    c.end = b + h.end_query;
    c.count = h.score;
    c.fI = fn ? fn[min((uint32_t)h.target, n_db - 1)] : h.target;
    c.weightedHits = (float)h.score;
    const uint32_t k = pos[r];
    calls[k] = c;
    call_hit[k] = (int64_t)r;
}

}  // namespace kg
