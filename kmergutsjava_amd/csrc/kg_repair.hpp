// kg_repair.hpp -- device side of kg_regionset_repair / kg_result_repair (include/kmerguts_hip.h): the frames of a multi-frame
// region joined into one protein (the rule is stated in the header, next to the entry points).
//
// No lane's work grows with a region's CALL count, a protein's length or the distance to a stop: a lane owns one CALL, one
// segment, one region (a chain of at most max_junctions + 1 parts, a constant) or kOrfResPerLane residues, and every search for
// a stop or a start is orf_find_up / orf_find_down of kg_orfs.hpp: a walk inside one tile plus one scanned key.
//
//   1. the CALLs in the region stage's group order, by that stage's own kernels and two sorts (region_keys_kernel,
//      region_group_keys_kernel, region_gather_kernel); repair_inverse_kernel turns the permutation round.
//   2. region i begins at the group-order position of its first_call: repair_owner_kernel marks the heads (one lane per region),
//      their prefix sum numbers the runs, repair_runs_kernel notes where each begins and whose it is.  repair_calls_kernel, one
//      lane per CALL, checks that the CALL lies in the region of its run; repair_sums_kernel, one lane per region, that the run
//      has the region's n_calls and score (a difference of two prefix values).  A foreign CALL list fails here, before anything
//      is used as an index.
//   3. the CALLs of the candidates with count >= min_count are compacted (prefix sum of the keep flags); a segment head is a
//      compacted CALL whose left neighbour has another region or frame; the heads' prefix sum numbers the segments.  C_k is one
//      atomicMax per CALL on the segment's word -- an integer maximum, so order cannot matter.
//   4. repair_junction_kernel  one lane per segment: J_k between it and the next one, two bounded finds.
//      repair_parts_kernel     one lane per segment: its part's first codon and length, the ends of the chain for the first and
//                              the last one, and the part's first stop.
//      repair_record_kernel    one lane per region: the at most max_junctions + 1 parts added up, the record, the lengths.
//   5. prefix sums of the lengths and of the junction counts; repair_junction_records_kernel, one lane per segment;
//      repair_residues_kernel, divided by output position as orf_residues_kernel is: a lane finds its ORF by binary search, and
//      in a repaired one its part among the ORF's at most eight junction records.  Every other protein is copied.
#pragma once

#include "kg_orfs.hpp"
#include "kg_regions.hpp"

namespace kg {

constexpr uint32_t kRepairNone = 0xFFFFFFFFu;
constexpr int kRepairMaxJunctions = 8;
// error words behind the region stage's: the first region with a bad seq, strand or first_call; the first CALL (index in
// calls[]) that lies in no region of its group; the first region whose run differs from its n_calls or score
enum { kRepairErrRegion = kRegionErrWords, kRepairErrCall = kRegionErrWords + 1, kRepairErrSums = kRegionErrWords + 2,
       kRepairErrWords = kRegionErrWords + 3 };
// counter words
enum { kRepairCntCandidates = 0, kRepairCntRepaired = 1, kRepairCntFailed = 2, kRepairCntSingle = 3, kRepairCntSkipped = 4,
       kRepairCntResidues = 5, kRepairCntWasComplete = 6, kRepairCntNewInterrupted = 7, kRepairCntPartial5Up = 8,
       kRepairCntPartial5Down = 9, kRepairCntWords = 10 };
// bits of a segment's meta word: the start class of the chain's first codon (1 ATG, 2 GTG, 4 TTG), no stop in front of it,
// a stop behind the last part
constexpr uint32_t kRepairMetaPartial5 = 8u, kRepairMetaHasStop = 16u;

// what the chain kernels keep per segment (arrays of one entry per compacted CALL: there are no more segments than those)
struct RepairSegments {
    uint32_t *reg;                      // the region (= ORF) of the segment
    uint32_t *frame;
    uint32_t *A, *C;                    // x0 of its first CALL, the largest x1 among its CALLs
    int32_t *J;                         // junction to the next segment, -1: failed
    int32_t *first_codon, *len;         // of its part; len 0: the chain has failed
    int32_t *stop;                      // the part's first stop as an index into the part, -1: none
    int32_t *end_codon;                 // last segment: the extent's last codon
    uint32_t *meta;
    int32_t *res;                       // protein index of the part's first residue
};

// frame f of a strand of contig s as orf_find_up / orf_find_down walk it, with the searches in codons j of the frame
struct RepairFrame {
    OrfSegment sg;
    int strand;
    int32_t n;
};

__device__ inline RepairFrame repair_frame(const uint8_t *__restrict__ seq, const OrfGeometry &geo, const int64_t *__restrict__ keys,
                                           int32_t s, int strand, int32_t f)
{
    const int64_t off = geo.offsets[s], L = geo.offsets[s + 1] - off;
    RepairFrame F;
    F.strand = strand;
    F.n = L >= f ? (int32_t)((L - f) / 3) : 0;
    const uint32_t g = strand ? (L >= f ? (uint32_t)((L - f) % 3) : 0u) : (uint32_t)f;
    const uint64_t tb = (uint64_t)geo.tile_base[s], nt = (uint64_t)geo.tile_base[s + 1] - tb;
    F.sg.bytes = seq + off + g;
    F.sg.keys = keys;
    F.sg.n_tiles = geo.n_tiles;
    F.sg.seg = 3 * (uint64_t)s + g;
    F.sg.mseg = 3 * geo.n_seqs - 1 - F.sg.seg;
    F.sg.gt0 = 3 * tb + (uint64_t)g * nt;
    F.sg.n = F.n;
    return F;
}

// the smallest stop > j, else n
__device__ inline int32_t repair_stop_after(const RepairFrame &F, int32_t j)
{
    if (!F.strand) {
        const int32_t x = orf_find_up(F.sg, kOrfFStop, kOrfUpFStop, j + 1, F.n - 1);
        return x < 0 ? F.n : x;
    }
    const int32_t me = orf_find_down(F.sg, kOrfRStop, kOrfDownRStop, 0, F.n - 1 - j - 1);
    return me < 0 ? F.n : F.n - 1 - me;
}

// the largest stop < j, else -1
__device__ inline int32_t repair_stop_before(const RepairFrame &F, int32_t j)
{
    if (!F.strand) return orf_find_down(F.sg, kOrfFStop, kOrfDownFStop, 0, j - 1);
    const int32_t mu = orf_find_up(F.sg, kOrfRStop, kOrfUpRStop, F.n - 1 - j + 1, F.n - 1);
    return mu < 0 ? -1 : F.n - 1 - mu;
}

// the smallest stop in [ja, jb], else -1
__device__ inline int32_t repair_first_stop(const RepairFrame &F, int32_t ja, int32_t jb)
{
    if (ja > jb) return -1;
    if (!F.strand) return orf_find_up(F.sg, kOrfFStop, kOrfUpFStop, ja, jb);
    const int32_t mi = orf_find_down(F.sg, kOrfRStop, kOrfDownRStop, F.n - 1 - jb, F.n - 1 - ja);
    return mi < 0 ? -1 : F.n - 1 - mi;
}

// the smallest start of the mask in [ja, jb], else -1; *bcls its start bits
__device__ inline int32_t repair_first_start(const RepairFrame &F, int32_t ja, int32_t jb, uint32_t start_codons, uint32_t *bcls)
{
    *bcls = 0;
    if (ja > jb) return -1;
    const int shift = F.strand ? 5 : 1;
    const uint32_t want = (start_codons & 7u) << shift;
    if (!want) return -1;
    const int32_t m = F.strand ? orf_find_down(F.sg, want, kOrfDownRStart, F.n - 1 - jb, F.n - 1 - ja)
                               : orf_find_up(F.sg, want, kOrfUpFStart, ja, jb);
    if (m < 0) return -1;
    *bcls = (kOrfTables.cls[orf_codon_index(F.sg, m)] & want) >> shift;
    return F.strand ? F.n - 1 - m : m;
}

__device__ inline bool repair_region_ok(const kg_region &r, uint64_t n_seqs, uint64_t n_calls)
{
    return r.seq >= 0 && (uint64_t)r.seq < n_seqs && (r.strand == 0 || r.strand == 1) && (uint64_t)r.first_call < n_calls;
}

__device__ inline bool repair_candidate(const kg_region &r) { return r.kept != 0 && (r.frames & (r.frames - 1)) != 0; }

// pos[perm[j]] = j: where a CALL of calls[] stands in group order
__global__ __launch_bounds__(256) void repair_inverse_kernel(const uint32_t *__restrict__ perm, uint64_t n, uint32_t *__restrict__ pos)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t v = perm[j];
    if (v < n) pos[v] = (uint32_t)j;
}

// One lane per region: head[p] = 1 and owner[p] = the smallest region that begins at group-order position p (owner: 0xFF bytes).
__global__ __launch_bounds__(256) void repair_owner_kernel(const kg_region *__restrict__ regions, uint64_t nr, uint64_t n,
                                                           uint64_t n_seqs, const uint32_t *__restrict__ pos,
                                                           uint32_t *__restrict__ head, uint32_t *owner, unsigned long long *err)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nr) return;
    const kg_region r = regions[i];
    if (!repair_region_ok(r, n_seqs, n)) {
        atomicMin(&err[kRepairErrRegion], (unsigned long long)i);
        return;
    }
    const uint32_t p = pos[r.first_call];
    if (p >= n) return;
    head[p] = 1u;
    atomicMin(&owner[p], (uint32_t)i);
}

// One lane per CALL in group order: run k begins at run_start[k] and is region run_region[k]'s; run_start[runs] = n.
__global__ __launch_bounds__(256) void repair_runs_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ hexcl,
                                                          const uint32_t *__restrict__ owner, uint64_t n,
                                                          uint32_t *__restrict__ run_start, uint32_t *__restrict__ run_region)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (head[j]) {
        run_start[hexcl[j]] = (uint32_t)j;
        run_region[hexcl[j]] = owner[j];
    }
    if (j == n - 1) run_start[hexcl[j] + head[j]] = (uint32_t)n;
}

// One lane per CALL in group order: it must lie in the region of its run.  keep[j] = it takes part in a chain; creg[j] = its region.
__global__ __launch_bounds__(256) void repair_calls_kernel(const kg_region *__restrict__ regions, uint64_t nr,
                                                           const int64_t *__restrict__ offsets, const uint64_t *__restrict__ gkeys,
                                                           const uint32_t *__restrict__ perm, const uint32_t *__restrict__ sx0,
                                                           const uint32_t *__restrict__ sx1, const int32_t *__restrict__ scount,
                                                           const uint32_t *__restrict__ head, const uint32_t *__restrict__ hexcl,
                                                           const uint32_t *__restrict__ run_region, uint64_t n, int32_t min_count,
                                                           uint32_t *__restrict__ keep, uint32_t *__restrict__ creg,
                                                           unsigned long long *err)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    keep[j] = 0;
    creg[j] = 0;
    const uint32_t runs = hexcl[j] + head[j];
    bool ok = runs > 0;
    uint32_t i = 0;
    if (ok) {
        i = run_region[runs - 1];
        ok = i < nr;
    }
    bool cand = false;
    if (ok) {
        const kg_region r = regions[i];       // repair_owner_kernel has checked seq and strand of every owner
        const uint64_t key = gkeys[j];
        const int64_t L = offsets[r.seq + 1] - offsets[r.seq];
        const int64_t xa = r.strand ? L - 1 - r.right : r.left, xb = r.strand ? L - 1 - r.left : r.right;
        ok = (uint32_t)(key >> 32) == (uint32_t)r.seq * 2u + (uint32_t)r.strand && (uint32_t)key == ((uint32_t)r.fI ^ 0x80000000u) &&
             (int64_t)sx0[j] >= xa && (int64_t)sx1[j] <= xb;
        cand = repair_candidate(r);
    }
    if (!ok) {
        atomicMin(&err[kRepairErrCall], (unsigned long long)perm[j]);
        return;
    }
    creg[j] = i;
    keep[j] = (cand && scount[j] >= min_count) ? 1u : 0u;
}

// One lane per region: its run has n_calls CALLs whose counts add up to score (both as differences of prefix values, mod 2^32).
__global__ __launch_bounds__(256) void repair_sums_kernel(const kg_region *__restrict__ regions, uint64_t nr, uint64_t n, uint64_t n_seqs,
                                                          const uint32_t *__restrict__ pos, const uint32_t *__restrict__ owner,
                                                          const uint32_t *__restrict__ hexcl, const uint32_t *__restrict__ run_start,
                                                          const uint32_t *__restrict__ cexcl, const uint64_t *__restrict__ ctotal,
                                                          unsigned long long *err)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nr) return;
    const kg_region r = regions[i];
    if (!repair_region_ok(r, n_seqs, n)) return;        // reported by repair_owner_kernel
    const uint32_t p = pos[r.first_call];
    bool ok = p < n && owner[p] == (uint32_t)i;
    if (ok) {
        const uint32_t k = hexcl[p], s0 = run_start[k], s1 = run_start[k + 1];
        const uint32_t sum = (s1 < n ? cexcl[s1] : (uint32_t)*ctotal) - cexcl[s0];
        ok = s1 - s0 == (uint32_t)r.n_calls && sum == (uint32_t)r.score;
    }
    if (!ok) atomicMin(&err[kRepairErrSums], (unsigned long long)i);
}

// the kept CALLs side by side, in group order
__global__ __launch_bounds__(256) void repair_compact_kernel(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ kexcl,
                                                             const uint32_t *__restrict__ creg, const uint32_t *__restrict__ sx0,
                                                             const uint32_t *__restrict__ sx1, const uint8_t *__restrict__ sframe,
                                                             uint64_t n, uint32_t *__restrict__ ireg, uint32_t *__restrict__ ix0,
                                                             uint32_t *__restrict__ ix1, uint32_t *__restrict__ iframe)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !keep[j]) return;
    const uint32_t c = kexcl[j];
    ireg[c] = creg[j];
    ix0[c] = sx0[j];
    ix1[c] = sx1[j];
    iframe[c] = sframe[j];
}

__global__ __launch_bounds__(256) void repair_seg_heads_kernel(const uint32_t *__restrict__ ireg, const uint32_t *__restrict__ iframe,
                                                               uint64_t nk, uint32_t *__restrict__ shead)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nk) return;
    shead[c] = (c == 0 || ireg[c - 1] != ireg[c] || iframe[c - 1] != iframe[c]) ? 1u : 0u;
}

// One lane per kept CALL: its segment's frame, A and C, and the first and last segment of its region (0xFF bytes: none).
__global__ __launch_bounds__(256) void repair_segments_kernel(const uint32_t *__restrict__ ireg, const uint32_t *__restrict__ ix0,
                                                              const uint32_t *__restrict__ ix1, const uint32_t *__restrict__ iframe,
                                                              const uint32_t *__restrict__ shead, const uint32_t *__restrict__ sexcl,
                                                              uint64_t nk, RepairSegments S, uint32_t *__restrict__ reg_first,
                                                              uint32_t *__restrict__ reg_last)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nk) return;
    const uint32_t sg = sexcl[c] + shead[c] - 1, i = ireg[c];
    if (shead[c]) {
        S.reg[sg] = i;
        S.frame[sg] = iframe[c];
        S.A[sg] = ix0[c];
    }
    if (c == 0 || ireg[c - 1] != i) reg_first[i] = sg;
    if (c + 1 == nk || ireg[c + 1] != i) reg_last[i] = sg;
    atomicMax(&S.C[sg], ix1[c]);
}

// One lane per segment: rule 3 for the junction behind it.
__global__ __launch_bounds__(256) void repair_junction_kernel(const kg_region *__restrict__ regions, const uint8_t *__restrict__ seq,
                                                              OrfGeometry geo, const int64_t *__restrict__ keys,
                                                              const uint64_t *__restrict__ n_segments, RepairSegments S,
                                                              const uint32_t *__restrict__ reg_first, const uint32_t *__restrict__ reg_last,
                                                              uint32_t max_junctions)
{
    const uint64_t sg = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sg >= *n_segments) return;
    const uint32_t i = S.reg[sg], first = reg_first[i], last = reg_last[i];
    if (sg >= last || last - first > max_junctions) return;
    const kg_region r = regions[i];
    const int32_t p = (int32_t)S.frame[sg], q = (int32_t)S.frame[sg + 1];
    const int64_t C = S.C[sg], A = S.A[sg + 1];
    const RepairFrame P = repair_frame(seq, geo, keys, r.seq, r.strand, p), Q = repair_frame(seq, geo, keys, r.seq, r.strand, q);
    const int32_t lp = (int32_t)((C - 2 - p) / 3), tp = repair_stop_after(P, lp);
    const int32_t gq = (int32_t)((A - q) / 3), sq = repair_stop_before(Q, gq);
    const int64_t hi = (int64_t)p + 3 * (int64_t)tp, lo = (int64_t)q + 3 * ((int64_t)sq + 1), mid = (C + 1 + A) / 2;
    S.J[sg] = lo > hi ? -1 : (int32_t)(mid < lo ? lo : mid > hi ? hi : mid);
}

// One lane per segment: rules 4 and 5 for its part.
__global__ __launch_bounds__(256) void repair_parts_kernel(const kg_region *__restrict__ regions, const uint8_t *__restrict__ seq,
                                                           OrfGeometry geo, const int64_t *__restrict__ keys,
                                                           const uint64_t *__restrict__ n_segments, RepairSegments S,
                                                           const uint32_t *__restrict__ reg_first, const uint32_t *__restrict__ reg_last,
                                                           uint32_t max_junctions, uint32_t start_codons)
{
    const uint64_t sg = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sg >= *n_segments) return;
    const uint32_t i = S.reg[sg], first = reg_first[i], last = reg_last[i];
    if (last == first || last - first > max_junctions) return;
    const kg_region r = regions[i];
    const int32_t f = (int32_t)S.frame[sg];
    const bool is_first = sg == first, is_last = sg == last;
    const int32_t jprev = is_first ? 0 : S.J[sg - 1], jnext = is_last ? 0 : S.J[sg];
    S.len[sg] = 0;
    if ((!is_first && jprev < 0) || (!is_last && jnext < 0) || (!is_first && !is_last && jprev >= jnext)) return;
    const RepairFrame F = repair_frame(seq, geo, keys, r.seq, r.strand, f);
    int32_t jf, je, end_codon = 0;
    uint32_t meta = 0;
    if (is_first) {
        const int32_t j0 = ((int32_t)S.A[sg] - f) / 3, u = repair_stop_before(F, j0);
        const int32_t sb = repair_first_start(F, u + 1, j0, start_codons, &meta);
        jf = sb < 0 ? u + 1 : sb;
        if (u < 0) meta |= kRepairMetaPartial5;
    } else {
        jf = (jprev - f + 2) / 3;           // ceil: jprev - f >= -2
    }
    if (is_last) {
        const int32_t jl = ((int32_t)S.C[sg] - 2 - f) / 3, e = repair_stop_after(F, jl);
        je = e < F.n ? e : F.n;
        end_codon = e < F.n ? e : F.n - 1;
        if (e < F.n) meta |= kRepairMetaHasStop;
    } else {
        je = jnext < f ? -1 : (jnext - f) / 3;
    }
    if (je - jf <= 0) return;
    const int32_t st = repair_first_stop(F, jf, je - 1);
    S.first_codon[sg] = jf;
    S.stop[sg] = st < 0 ? -1 : st - jf;
    S.end_codon[sg] = end_codon;
    S.meta[sg] = meta;
    S.len[sg] = je - jf;
}

// One lane per region: rule 6.  out[] holds the given records; lens[] the given lengths; jcount[] zeros.
__global__ __launch_bounds__(256) void repair_record_kernel(const kg_region *__restrict__ regions, uint64_t nr,
                                                            const int64_t *__restrict__ offsets, RepairSegments S,
                                                            const uint32_t *__restrict__ reg_first, const uint32_t *__restrict__ reg_last,
                                                            uint32_t max_junctions, kg_orf *__restrict__ out,
                                                            uint32_t *__restrict__ lens, uint32_t *__restrict__ jcount,
                                                            unsigned long long *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t state = 0;                 // 1 repaired, 2 failed, 3 single, 4 skipped
    uint32_t residues = 0, was_complete = 0, new_interrupted = 0, p5_up = 0, p5_down = 0;
    if (i < nr) {
        const kg_region r = regions[i];
        // (a candidate has CALLs in the list, so repair_owner_kernel has checked its seq and strand)
        if (repair_candidate(r)) {
            const uint32_t first = reg_first[i], last = reg_last[i];
            if (first == kRepairNone || last == first) {
                state = 3;
            } else if (last - first > max_junctions) {
                state = 4;
            } else {
                int32_t total = 0, inner = -1;
                state = 1;
                for (uint32_t sg = first; sg <= last; sg++) {          // at most max_junctions + 1 parts
                    const int32_t len = S.len[sg];
                    if (len <= 0) { state = 2; break; }
                    S.res[sg] = total;
                    if (inner < 0 && S.stop[sg] >= 0) inner = total + S.stop[sg];
                    total += len;
                }
                if (state == 1) {
                    const kg_orf old = out[i];
                    const int64_t L = offsets[r.seq + 1] - offsets[r.seq];
                    const uint32_t m1 = S.meta[first], mm = S.meta[last];
                    const int64_t xs = (int64_t)S.frame[first] + 3 * (int64_t)S.first_codon[first];
                    const int64_t xe = (int64_t)S.frame[last] + 3 * (int64_t)S.end_codon[last] + 2;
                    kg_orf o = old;
                    o.seq = r.seq;
                    o.strand = r.strand;
                    o.frame = (int32_t)S.frame[first];
                    o.left = (int32_t)(r.strand ? L - 1 - xe : xs);
                    o.right = (int32_t)(r.strand ? L - 1 - xs : xe);
                    o.n_res = total;
                    o.start_codon = m1 & 1u ? 1 : m1 & 2u ? 2 : m1 & 4u ? 3 : 0;
                    o.first_inner = inner;
                    o.flags = (mm & kRepairMetaHasStop ? KG_ORF_HAS_STOP : 0u) | (m1 & kRepairMetaPartial5 ? KG_ORF_PARTIAL5 : 0u) |
                              KG_ORF_INTERRUPTED | KG_ORF_MULTI_FRAME | KG_ORF_REPAIRED;
                    o.fI = r.fI;
                    o.score = r.score;
                    o.kept = r.kept;
                    out[i] = o;
                    lens[i] = (uint32_t)total;
                    jcount[i] = last - first;
                    residues = (uint32_t)total;
                    was_complete = (old.flags & KG_ORF_HAS_STOP) && old.start_codon != 0 && !(old.flags & KG_ORF_INTERRUPTED) ? 1u : 0u;
                    new_interrupted = old.flags & KG_ORF_INTERRUPTED ? 0u : 1u;
                    p5_up = (o.flags & KG_ORF_PARTIAL5) && !(old.flags & KG_ORF_PARTIAL5) ? 1u : 0u;
                    p5_down = !(o.flags & KG_ORF_PARTIAL5) && (old.flags & KG_ORF_PARTIAL5) ? 1u : 0u;
                }
            }
        }
    }
    const uint32_t flags[9] = {state != 0, state == 1, state == 2, state == 3, state == 4, was_complete, new_interrupted, p5_up, p5_down};
    const int words[9] = {kRepairCntCandidates, kRepairCntRepaired, kRepairCntFailed, kRepairCntSingle, kRepairCntSkipped,
                          kRepairCntWasComplete, kRepairCntNewInterrupted, kRepairCntPartial5Up, kRepairCntPartial5Down};
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const uint32_t c = (uint32_t)__popcll(__ballot(flags[k]));
        if (c && (threadIdx.x & 63) == 0) atomicAdd(&cnt[words[k]], (unsigned long long)c);
    }
    for (int off = 32; off > 0; off >>= 1) residues += __shfl_down(residues, off);
    if (residues && (threadIdx.x & 63) == 0) atomicAdd(&cnt[kRepairCntResidues], (unsigned long long)residues);
}

// One lane per segment: rule 7 for the junction behind it, at its final index.
__global__ __launch_bounds__(256) void repair_junction_records_kernel(const kg_orf *__restrict__ out, const int64_t *__restrict__ offsets,
                                                                      const uint64_t *__restrict__ n_segments, RepairSegments S,
                                                                      const uint32_t *__restrict__ reg_first,
                                                                      const uint32_t *__restrict__ reg_last,
                                                                      const int64_t *__restrict__ junction_start,
                                                                      kg_junction *__restrict__ junctions)
{
    const uint64_t sg = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sg >= *n_segments) return;
    const uint32_t i = S.reg[sg], first = reg_first[i], last = reg_last[i];
    // (not by KG_ORF_REPAIRED: a given record may carry the flag of an earlier call, and this call has left it alone)
    if (sg >= last || junction_start[i + 1] == junction_start[i]) return;
    const kg_orf o = out[i];
    const int64_t L = offsets[o.seq + 1] - offsets[o.seq], J = S.J[sg];
    kg_junction j;
    j.orf = (int32_t)i;
    j.pos = (int32_t)(o.strand ? L - 1 - J : J);
    j.from_frame = (int32_t)S.frame[sg];
    j.to_frame = (int32_t)S.frame[sg + 1];
    j.res = S.res[sg + 1];
    j.gap = (int32_t)((int64_t)S.A[sg + 1] - (int64_t)S.C[sg] - 1);
    junctions[junction_start[i] + (sg - first)] = j;
}

// A lane owns residues [kOrfResPerLane * q, + kOrfResPerLane) of the new proteins.  The residue of an ORF repaired in this call
// (it has junctions: a chain that holds has at least one) is translated from its part's frame; every other one is the given
// set's byte, also where the given record carries KG_ORF_REPAIRED from an earlier call.
__global__ __launch_bounds__(256) void repair_residues_kernel(const kg_orf *__restrict__ orfs, uint64_t n,
                                                              const int64_t *__restrict__ prot_start, uint64_t total,
                                                              const int64_t *__restrict__ old_start, const uint8_t *__restrict__ old_res,
                                                              const int64_t *__restrict__ junction_start,
                                                              const kg_junction *__restrict__ junctions,
                                                              const uint8_t *__restrict__ seq, const int64_t *__restrict__ offsets,
                                                              uint8_t *__restrict__ res)
{
    const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kOrfResPerLane;
    if (first >= total) return;
    uint64_t i = orf_owner(prot_start, n, (int64_t)first);
    int64_t begin = prot_start[i], end = prot_start[i + 1];
    kg_orf o = orfs[i];
    uint64_t word = 0;
    int k = 0;
    for (; k < kOrfResPerLane && first + k < total; k++) {
        const int64_t pos = (int64_t)(first + k);
        if (pos >= end) {
            i = (i + 2 <= n && prot_start[i + 1] <= pos && pos < prot_start[i + 2]) ? i + 1 : orf_owner(prot_start, n, pos);
            begin = prot_start[i];
            end = prot_start[i + 1];
            o = orfs[i];
        }
        const int64_t q = pos - begin;                                  // residue of ORF i
        const int64_t js = junction_start[i], je = junction_start[i + 1];
        uint32_t ch;
        if (je == js) {                                                 // not repaired in this call, whatever its flags say
            ch = old_res[old_start[i] + q];
        } else {
            const int64_t off = offsets[o.seq], L = offsets[o.seq + 1] - off;
            int64_t part = 0;
            for (int64_t t = js; t < je && t < js + kRepairMaxJunctions; t++) part += junctions[t].res <= q ? 1 : 0;
            int64_t x;                                                  // the codon's first strand position
            if (part == 0) {
                x = (o.strand ? L - 1 - o.right : o.left) + 3 * q;
            } else {
                const kg_junction jr = junctions[js + part - 1];
                const int64_t J = o.strand ? L - 1 - jr.pos : jr.pos;
                x = jr.to_frame + 3 * ((J - jr.to_frame + 2) / 3 + q - jr.res);
            }
            uint32_t c0, c1, c2;
            if (!o.strand) {
                const uint8_t *p = seq + off + x;
                c0 = dna_code(p[0]); c1 = dna_code(p[1]); c2 = dna_code(p[2]);
            } else {
                const uint8_t *p = seq + off + (L - 1 - x);
                c0 = dna_code(p[0]); c1 = dna_code(p[-1]); c2 = dna_code(p[-2]);
                c0 = c0 < 4 ? 3 - c0 : 4; c1 = c1 < 4 ? 3 - c1 : 4; c2 = c2 < 4 ? 3 - c2 : 4;
            }
            ch = (uint8_t)kOrfTables.letter[c0 * 25 + c1 * 5 + c2];
            if (q == 0 && o.start_codon != 0) ch = 'M';
        }
        word |= (uint64_t)ch << (8 * k);
    }
    if (k == kOrfResPerLane) {
        *reinterpret_cast<uint64_t *>(res + first) = word;
    } else {
        for (int b = 0; b < k; b++) res[first + b] = (uint8_t)(word >> (8 * b));
    }
}

}  // namespace kg
