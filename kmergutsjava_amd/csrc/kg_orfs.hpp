// kg_orfs.hpp -- device side of kg_regionset_orfs / kg_orfs_regions (include/kmerguts_hip.h): function regions -> the open
// reading frame around each and its translated protein (the rule is stated in the header, next to the entry points).
//
// Everything works on the forward bytes.  Codon m of forward phase g of a contig is the bytes g+3m .. g+3m+2, 0 <= m < n_g.
// Frame f of '+' is phase f with j = m; frame f of '-' is phase g = (L - f) mod 3 read backwards, j = n_g - 1 - m (n_g = n_f),
// and its codon is a stop when the forward bytes read TTA / CTA / TCA, a start when they read CAT / CAC / CAA.  So "the largest
// stop below j0" on '-' is "the smallest reverse stop above m0", and one tiling of the forward codons serves both strands.
//
//   1. orf_summary_kernel     one wave per tile row = kOrfTile codons of each of the three phases of a contig (3 * kOrfTile
//                             bytes and two more, each read from HBM once -- a lane's three aligned dwords overlap its neighbours',
//                             which the caches serve): per phase the last and first forward stop, the first
//                             forward start, the first and last reverse stop and the last reverse start of the tile, found
//                             with ballots, as six keys (segment : position).
//   2. six prefix maxima across the tiles, reduce-then-scan without any cross-workgroup wait: orf_tile_max_kernel, the build's
//      build_tile_scan_kernel over the scan tiles' maxima, orf_scan_apply_kernel.  The segment (contig * 3 + phase) is packed
//      into the high bits, so the plain maximum is the segmented one; the three "first" arrays are stored mirrored (index,
//      segment and position), which turns their suffix minimum into the same prefix maximum.
//   3. orf_region_kernel      one lane per region: validation (error words by atomicMin, firing only on bad input; a bad region
//                             is not used as an index), then u, e, b, i* -- each a walk inside ONE tile (at most kOrfTile
//                             codons) plus one read of a scanned array -- the record and the protein's length.
//   4. prefix_sum of the lengths -> prot_start (orf_prot_start_kernel); orf_residues_kernel, divided by output position: a lane
//      owns kOrfResPerLane consecutive residues and finds its ORF by binary search in prot_start.
//
// kg_orfs_free / kg_orfset_add_free (evidence-free candidates, the rule is in the header too) use 1, 2 and 4 as they are and put
//   3'. orf_free_kernel<false / true>  in the place of 3: one wave per tile row again.  A candidate is owned by its closing stop
//                             (the run that reaches the contig's end: by lane 0 of the container's last tile in codon order), so
//                             a lane owns at most two stops of each of the six containers.  u comes from the tile's ballots or one
//                             scanned key; only a run of min_res codons or more then looks for its start, one walk inside one
//                             tile plus one scanned key.  The first pass counts per (container, tile) in output order -- on '-'
//                             the tiles mirrored -- prefix_sum turns the counts into first indices, and the second pass writes
//                             every record at its final index with in-tile ranks from ballots: no sort, no wait between
//                             workgroups, and one non-returning add per wave and counter.
#pragma once

#include "kg_build.hpp"
#include "kg_device.hpp"

namespace kg {

constexpr int kOrfTile = 128;           // codons of one phase per tile (two per lane of the summary wave)
constexpr int kOrfResPerLane = 8;
constexpr int kOrfPlanes = 6;
// the scanned arrays; the kOrfUp* ones are stored mirrored
enum { kOrfDownFStop = 0, kOrfDownRStop = 1, kOrfDownRStart = 2, kOrfUpFStop = 3, kOrfUpFStart = 4, kOrfUpRStop = 5 };
// error words: the first region [0] with a bad seq, [1] strand, [2] best_frame, [3] left / right outside the contig,
// [4] without a whole codon of its frame inside it
enum { kOrfErrSeq = 0, kOrfErrStrand = 1, kOrfErrFrame = 2, kOrfErrRange = 3, kOrfErrAnchor = 4, kOrfErrWords = 5 };
// counter words
enum { kOrfCntComplete = 0, kOrfCntInterrupted = 1, kOrfCntPartial5 = 2, kOrfCntWords = 3 };
// the words of orf_free_kernel's host: the candidates, two counters, then the residue total
enum { kOrfFreeCount = 0, kOrfFreeComplete = 1, kOrfFreePartial5 = 2, kOrfFreeResidues = 3, kOrfFreeWords = 4 };

// codon classes, by b0 * 25 + b1 * 5 + b2 (dna_code values): bit 0 forward stop, bits 1-3 forward start (ATG, GTG, TTG),
// bit 4 reverse stop, bits 5-7 reverse start (of ATG, GTG, TTG)
constexpr uint32_t kOrfFStop = 1u, kOrfRStop = 0x10u;
struct OrfTables {
    uint8_t cls[128];
    char letter[128];                   // the residue of the forward codon; 'X' with an unknown base
};
constexpr uint32_t orf_class_of(uint32_t a, uint32_t b, uint32_t c)
{
    if (a > 3 || b > 3 || c > 3) return 0;
    uint32_t r = 0;
    if (a == 3 && ((b == 0 && (c == 0 || c == 2)) || (b == 2 && c == 0))) r |= kOrfFStop;           // TAA TAG TGA
    if (b == 3 && c == 2) r |= a == 0 ? 2u : a == 2 ? 4u : a == 3 ? 8u : 0u;                         // ATG GTG TTG
    return r;
}
constexpr OrfTables orf_tables()
{
    OrfTables t{};
    for (uint32_t i = 0; i < 128; i++) {
        const uint32_t a = i / 25, b = (i / 5) % 5, c = i % 5;
        t.cls[i] = 0;
        t.letter[i] = 'X';
        if (i >= 125 || a > 3 || b > 3 || c > 3) continue;
        const uint32_t fw = orf_class_of(a, b, c), rv = orf_class_of(3 - c, 3 - b, 3 - a);
        t.cls[i] = (uint8_t)(fw | (rv << 4));
        t.letter[i] = kGeneticCode[a * 16 + b * 4 + c];
    }
    return t;
}
__constant__ OrfTables kOrfTables = orf_tables();

// (segment, position) of the "last" arrays: larger = later; 0 in the low 31 bits = none.  Signed so that build_tile_scan_kernel
// (identity INT64_MIN = segment 0, none) applies.  The key is full but does not overflow: segment < 3 * n_seqs < 3 * 2^31 < 2^33
// (check_region_offsets), so segment << 31 < 2^64; position + 1 <= 2^31 / 3.
__device__ inline int64_t orf_key(uint64_t seg, uint32_t low31)
{
    return (int64_t)(((seg << 31) | low31) ^ 0x8000000000000000ull);
}
__device__ inline uint64_t orf_key_seg(int64_t k) { return ((uint64_t)k ^ 0x8000000000000000ull) >> 31; }
__device__ inline uint32_t orf_key_low(int64_t k) { return (uint32_t)((uint64_t)k & 0x7FFFFFFFu); }

struct OrfGeometry {
    const int64_t *offsets;             // n_seqs + 1
    const int64_t *tile_base;           // n_seqs + 1: tile rows in front of a contig
    uint64_t n_seqs;
    uint64_t n_tiles;                   // 3 * tile_base[n_seqs]: the items of one scanned array
};

// bytes a .. a + 7 of seq[0 .. total) as a little-endian word, 0 where there is none; whole aligned dwords where they lie inside
__device__ inline uint64_t orf_load8(const uint8_t *__restrict__ seq, uint64_t total, uint64_t a)
{
    const uint8_t *p = seq + a, *end = seq + total;
    const uint8_t *p4 = (const uint8_t *)((uintptr_t)p & ~(uintptr_t)3);
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint8_t *q = p4 + 4 * k;
        if (q >= seq && q + 4 <= end) {
            w[k] = *reinterpret_cast<const uint32_t *>(q);
        } else {
            w[k] = 0;
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (q + b >= seq && q + b < end) w[k] |= (uint32_t)q[b] << (8 * b);
        }
    }
    const uint32_t sh = (uint32_t)(p - p4) * 8;
    const uint64_t lo = ((uint64_t)w[1] << 32) | w[0];
    return sh ? (lo >> sh) | ((uint64_t)w[2] << (64 - sh)) : lo;
}

// first / last set position among codons 2 * lane + k, from the two ballots; -1 = none
__device__ inline int orf_first2(uint64_t b0, uint64_t b1)
{
    const int x0 = b0 ? 2 * (int)__builtin_ctzll(b0) : 1 << 20, x1 = b1 ? 2 * (int)__builtin_ctzll(b1) + 1 : 1 << 20;
    const int x = x0 < x1 ? x0 : x1;
    return x == 1 << 20 ? -1 : x;
}
__device__ inline int orf_last2(uint64_t b0, uint64_t b1)
{
    const int x0 = b0 ? 2 * (63 - (int)__builtin_clzll(b0)) : -1, x1 = b1 ? 2 * (63 - (int)__builtin_clzll(b1)) + 1 : -1;
    return x0 > x1 ? x0 : x1;
}

// the tile row a wave works on: tile t of the nt of contig s
struct OrfRow {
    uint64_t s, tb, nt, t;
    int64_t off, L;
};

__device__ inline OrfRow orf_row_of(const OrfGeometry &geo, uint64_t row)
{
    // the contig of the row: the last s with tile_base[s] <= row
    uint64_t lo = 0, hi = geo.n_seqs;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)geo.tile_base[mid] <= row) lo = mid;
        else hi = mid;
    }
    OrfRow r;
    r.s = lo;
    r.off = geo.offsets[lo];
    r.L = geo.offsets[lo + 1] - r.off;
    r.tb = (uint64_t)geo.tile_base[lo];
    r.nt = (uint64_t)geo.tile_base[lo + 1] - r.tb;
    r.t = row - r.tb;
    return r;
}

// the dna_code values of the eight bytes that hold the lane's two codons (2 * lane, 2 * lane + 1 of the tile) of every phase;
// 4 behind the contig's end
__device__ inline void orf_row_codes(const uint8_t *__restrict__ seq, uint64_t total, const OrfRow &r, int lane, uint32_t (&code)[8])
{
    const uint64_t m0 = r.t * kOrfTile + 2 * (uint64_t)lane;                   // the lane's first codon of every phase
    const uint64_t at = 3 * m0;                                                // its first byte in the contig
    uint64_t w = 0;
    if ((int64_t)at < r.L) w = orf_load8(seq, total, (uint64_t)r.off + at);
#pragma unroll
    for (int k = 0; k < 8; k++) code[k] = ((int64_t)(at + k) < r.L) ? dna_code((uint32_t)(w >> (8 * k)) & 255u) : 4u;
}

// One wave per tile row.  keys: kOrfPlanes arrays of geo.n_tiles items.
__global__ __launch_bounds__(256) void orf_summary_kernel(const uint8_t *__restrict__ seq, uint64_t total, OrfGeometry geo,
                                                          uint64_t n_rows, uint32_t start_codons, int64_t *__restrict__ keys)
{
    const int lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const OrfRow rw = orf_row_of(geo, row);
    const uint64_t s = rw.s, tb = rw.tb, nt = rw.nt, t = rw.t;
    uint32_t code[8];
    orf_row_codes(seq, total, rw, lane, code);
    const uint32_t fstart = (start_codons & 7u) << 1, rstart = (start_codons & 7u) << 5;
#pragma unroll
    for (int g = 0; g < 3; g++) {
        uint32_t c[2];
#pragma unroll
        for (int k = 0; k < 2; k++) c[k] = kOrfTables.cls[code[g + 3 * k] * 25 + code[g + 3 * k + 1] * 5 + code[g + 3 * k + 2]];
        const uint64_t fs0 = __ballot(c[0] & kOrfFStop), fs1 = __ballot(c[1] & kOrfFStop);
        const uint64_t fa0 = __ballot(c[0] & fstart), fa1 = __ballot(c[1] & fstart);
        const uint64_t rs0 = __ballot(c[0] & kOrfRStop), rs1 = __ballot(c[1] & kOrfRStop);
        const uint64_t ra0 = __ballot(c[0] & rstart), ra1 = __ballot(c[1] & rstart);
        if (lane != 0) continue;
        const uint64_t seg = 3 * s + g, gt = 3 * tb + (uint64_t)g * nt + t;
        const uint64_t mseg = 3 * geo.n_seqs - 1 - seg, mgt = geo.n_tiles - 1 - gt;
        const uint32_t base = (uint32_t)(t * kOrfTile);
        const int down[3] = {orf_last2(fs0, fs1), orf_last2(rs0, rs1), orf_last2(ra0, ra1)};
        const int up[3] = {orf_first2(fs0, fs1), orf_first2(fa0, fa1), orf_first2(rs0, rs1)};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            keys[(uint64_t)a * geo.n_tiles + gt] = orf_key(seg, down[a] < 0 ? 0u : base + (uint32_t)down[a] + 1u);
            keys[(uint64_t)(3 + a) * geo.n_tiles + mgt] = orf_key(mseg, up[a] < 0 ? 0u : 0x7FFFFFFFu - (base + (uint32_t)up[a]));
        }
    }
}

// grid (scan tiles, planes): tile_max[plane * gridDim.x + tile] = the maximum of the scan tile's keys
__global__ __launch_bounds__(kBuildThreads) void orf_tile_max_kernel(const int64_t *__restrict__ keys, uint64_t n,
                                                                     int64_t *__restrict__ tile_max)
{
    __shared__ int64_t wmax[kBuildThreads / kWave];
    const int64_t *k = keys + (uint64_t)blockIdx.y * n;
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile;
    int64_t m = INT64_MIN;
    for (int q = 0; q < kBuildItems; q++) {
        const uint64_t i = base + (uint64_t)q * kBuildThreads + threadIdx.x;
        if (i >= n) break;
        m = k[i] > m ? k[i] : m;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t y = __shfl_down(m, off);
        m = y > m ? y : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBuildThreads / kWave; w++) m = wmax[w] > m ? wmax[w] : m;
        tile_max[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
    }
}

// grid (scan tiles, planes): the keys become their inclusive prefix maximum, in place.  Thread t of a scan tile takes items
// [tile * 4096 + t * 16, + 16), as region_heads_kernel does.
__global__ __launch_bounds__(kBuildThreads) void orf_scan_apply_kernel(int64_t *__restrict__ keys, uint64_t n,
                                                                       const int64_t *__restrict__ tile_pre)
{
    __shared__ int64_t wmax[kBuildThreads / kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t *k = keys + (uint64_t)blockIdx.y * n;
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile + (uint64_t)threadIdx.x * kBuildItems;
    int64_t a[kBuildItems];
    int64_t m = INT64_MIN;
#pragma unroll
    for (int q = 0; q < kBuildItems; q++) {
        a[q] = base + q < n ? k[base + q] : INT64_MIN;
        m = a[q] > m ? a[q] : m;
    }
    int64_t incl = m;
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t y = __shfl_up(incl, off);
        if (lane >= off) incl = y > incl ? y : incl;
    }
    int64_t run = __shfl_up(incl, 1);
    if (lane == 0) run = INT64_MIN;
    if (lane == 63) wmax[wave] = incl;
    __syncthreads();
    const int64_t tp = tile_pre[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x];
    run = tp > run ? tp : run;
    for (int w = 0; w < wave; w++) run = wmax[w] > run ? wmax[w] : run;
#pragma unroll
    for (int q = 0; q < kBuildItems; q++) {
        if (base + q >= n) break;
        run = a[q] > run ? a[q] : run;
        k[base + q] = run;
    }
}

// one (contig, phase) as the region kernel walks it
struct OrfSegment {
    const uint8_t *bytes;               // the contig's first byte of the phase: codon m is bytes[3m .. 3m + 2]
    const int64_t *keys;                // the scanned arrays
    uint64_t n_tiles, seg, mseg, gt0;   // gt0: the segment's first tile
    int32_t n;                          // codons
};

__device__ inline uint32_t orf_codon_index(const OrfSegment &sg, int32_t m)
{
    const uint8_t *p = sg.bytes + 3 * (int64_t)m;
    return dna_code(p[0]) * 25 + dna_code(p[1]) * 5 + dna_code(p[2]);
}

// the smallest m in [lo, hi] whose class has a bit of `want`, else -1: the rest of lo's tile, then one scanned "first" key
__device__ inline int32_t orf_find_up(const OrfSegment &sg, uint32_t want, int plane, int32_t lo, int32_t hi)
{
    if (lo > hi) return -1;
    const int32_t tl = lo / kOrfTile, tile_end = (tl + 1) * kOrfTile - 1, end = hi < tile_end ? hi : tile_end;
    for (int32_t m = lo; m <= end; m++)
        if (kOrfTables.cls[orf_codon_index(sg, m)] & want) return m;
    if (end == hi) return -1;
    const uint64_t gt = sg.gt0 + (uint64_t)tl + 1;
    if (gt >= sg.n_tiles) return -1;
    const int64_t k = sg.keys[(uint64_t)plane * sg.n_tiles + (sg.n_tiles - 1 - gt)];
    if (orf_key_seg(k) != sg.mseg || orf_key_low(k) == 0) return -1;
    const int32_t pos = (int32_t)(0x7FFFFFFFu - orf_key_low(k));
    return pos <= hi ? pos : -1;
}

// the largest m in [lo, hi] whose class has a bit of `want`, else -1: the front of hi's tile, then one scanned "last" key
__device__ inline int32_t orf_find_down(const OrfSegment &sg, uint32_t want, int plane, int32_t lo, int32_t hi)
{
    if (lo > hi) return -1;
    const int32_t th = hi / kOrfTile, tile_begin = th * kOrfTile, begin = lo > tile_begin ? lo : tile_begin;
    for (int32_t m = hi; m >= begin; m--)
        if (kOrfTables.cls[orf_codon_index(sg, m)] & want) return m;
    if (begin == lo || th == 0) return -1;
    const int64_t k = sg.keys[(uint64_t)plane * sg.n_tiles + sg.gt0 + (uint64_t)th - 1];
    if (orf_key_seg(k) != sg.seg || orf_key_low(k) == 0) return -1;
    const int32_t pos = (int32_t)orf_key_low(k) - 1;
    return pos >= lo ? pos : -1;
}

// One lane per region: rules 1-4.  lens[i] = the bytes the protein takes behind prot_start.
__global__ __launch_bounds__(256) void orf_region_kernel(const kg_region *__restrict__ regions, uint64_t n,
                                                         const uint8_t *__restrict__ seq, OrfGeometry geo,
                                                         const int64_t *__restrict__ keys, uint32_t start_codons, int only_kept,
                                                         kg_orf *__restrict__ out, uint32_t *__restrict__ lens,
                                                         unsigned long long *err, unsigned long long *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t complete = 0, interrupted = 0, partial5 = 0;
    if (i < n) {
        const kg_region r = regions[i];
        kg_orf o = {};
        o.first_inner = -1;
        bool ok = true;
        if (r.seq < 0 || (uint64_t)r.seq >= geo.n_seqs) { atomicMin(&err[kOrfErrSeq], (unsigned long long)i); ok = false; }
        if (r.strand != 0 && r.strand != 1) { atomicMin(&err[kOrfErrStrand], (unsigned long long)i); ok = false; }
        if (r.best_frame < 0 || r.best_frame > 2) { atomicMin(&err[kOrfErrFrame], (unsigned long long)i); ok = false; }
        int64_t L = 0, off = 0;
        if (ok) {
            off = geo.offsets[r.seq];
            L = geo.offsets[r.seq + 1] - off;
            if (r.left < 0 || r.left > r.right || (int64_t)r.right >= L) { atomicMin(&err[kOrfErrRange], (unsigned long long)i); ok = false; }
        }
        int32_t f = 0, nf = 0, j0 = 0, j1 = 0;
        if (ok) {
            f = r.best_frame;
            nf = L >= f ? (int32_t)((L - f) / 3) : 0;
            const int64_t xa = r.strand ? L - 1 - r.right : r.left, xb = r.strand ? L - 1 - r.left : r.right;
            const int64_t d = xa - f, v = xb - 2 - f;
            j0 = d <= 0 ? 0 : (int32_t)((d + 2) / 3);
            j1 = v < 0 ? -1 : (int32_t)(v / 3);
            if (j0 > j1 || j1 >= nf) { atomicMin(&err[kOrfErrAnchor], (unsigned long long)i); ok = false; }
        }
        if (ok) {
            const uint32_t g = r.strand ? (uint32_t)((L - f) % 3) : (uint32_t)f;
            const uint64_t tb = (uint64_t)geo.tile_base[r.seq], nt = (uint64_t)geo.tile_base[r.seq + 1] - tb;
            OrfSegment sg;
            sg.bytes = seq + off + g;
            sg.keys = keys;
            sg.n_tiles = geo.n_tiles;
            sg.seg = 3 * (uint64_t)r.seq + g;
            sg.mseg = 3 * geo.n_seqs - 1 - sg.seg;
            sg.gt0 = 3 * tb + (uint64_t)g * nt;
            sg.n = nf;
            const uint32_t fstart = (start_codons & 7u) << 1, rstart = (start_codons & 7u) << 5;
            int32_t u, e, b, istar;     // in j
            uint32_t bcls;
            if (!r.strand) {
                u = orf_find_down(sg, kOrfFStop, kOrfDownFStop, 0, j0 - 1);
                const int32_t x = orf_find_up(sg, kOrfFStop, kOrfUpFStop, j1 + 1, nf - 1);
                e = x < 0 ? nf : x;
                const int32_t sb = orf_find_up(sg, fstart, kOrfUpFStart, u + 1, j0);
                b = sb < 0 ? u + 1 : sb;
                bcls = sb < 0 ? 0u : (kOrfTables.cls[orf_codon_index(sg, sb)] & fstart) >> 1;
                istar = orf_find_up(sg, kOrfFStop, kOrfUpFStop, j0, j1);
            } else {
                const int32_t m0 = nf - 1 - j0, m1 = nf - 1 - j1;
                const int32_t mu = orf_find_up(sg, kOrfRStop, kOrfUpRStop, m0 + 1, nf - 1);
                u = mu < 0 ? -1 : nf - 1 - mu;
                const int32_t me = orf_find_down(sg, kOrfRStop, kOrfDownRStop, 0, m1 - 1);
                e = me < 0 ? nf : nf - 1 - me;
                const int32_t mb = orf_find_down(sg, rstart, kOrfDownRStart, m0, mu < 0 ? nf - 1 : mu - 1);
                b = mb < 0 ? u + 1 : nf - 1 - mb;
                bcls = mb < 0 ? 0u : (kOrfTables.cls[orf_codon_index(sg, mb)] & rstart) >> 5;
                const int32_t mi = orf_find_down(sg, kOrfRStop, kOrfDownRStop, m1, m0);
                istar = mi < 0 ? -1 : nf - 1 - mi;
            }
            const int32_t last = e < nf ? e : nf - 1;
            const int64_t xs = (int64_t)f + 3 * (int64_t)b, xe = (int64_t)f + 3 * (int64_t)last + 2;
            o.seq = r.seq;
            o.strand = r.strand;
            o.frame = f;
            o.left = (int32_t)(r.strand ? L - 1 - xe : xs);
            o.right = (int32_t)(r.strand ? L - 1 - xs : xe);
            o.n_res = (e < nf ? e : nf) - b;
            o.start_codon = bcls & 1u ? 1 : bcls & 2u ? 2 : bcls & 4u ? 3 : 0;
            o.first_inner = istar >= 0 ? istar - b : -1;
            o.flags = (e < nf ? KG_ORF_HAS_STOP : 0u) | (u < 0 ? KG_ORF_PARTIAL5 : 0u) | (istar >= 0 ? KG_ORF_INTERRUPTED : 0u) |
                      ((r.frames & (r.frames - 1)) ? KG_ORF_MULTI_FRAME : 0u);
            o.fI = r.fI;
            o.score = r.score;
            o.kept = r.kept;
            interrupted = istar >= 0 ? 1u : 0u;
            partial5 = u < 0 ? 1u : 0u;
            complete = (e < nf && o.start_codon != 0 && istar < 0) ? 1u : 0u;
        }
        out[i] = o;
        lens[i] = (only_kept && !o.kept) ? 0u : (uint32_t)o.n_res;
    }
    const uint32_t nc = (uint32_t)__popcll(__ballot(complete)), ni = (uint32_t)__popcll(__ballot(interrupted)),
                   np = (uint32_t)__popcll(__ballot(partial5));
    if ((threadIdx.x & 63) == 0) {
        if (nc) atomicAdd(&cnt[kOrfCntComplete], (unsigned long long)nc);
        if (ni) atomicAdd(&cnt[kOrfCntInterrupted], (unsigned long long)ni);
        if (np) atomicAdd(&cnt[kOrfCntPartial5], (unsigned long long)np);
    }
}

// Rules 2 and 3 of the free candidates for the run between two neighbouring stops of one container, in forward codons m of
// its phase.  '+': mu < me, mu = -1 without a stop in front, me = n for the run that reaches the contig's end.  '-': mu > me,
// mu = n and me = -1 in the same places.  -> whether the run gives a candidate; *mb its first codon, *bcls that codon's start bits.
__device__ inline bool orf_free_run(const OrfSegment &sg, int strand, int32_t me, int32_t mu, int32_t min_res, uint32_t start_codons,
                                    int32_t *mb, uint32_t *bcls)
{
    if ((strand ? mu - me : me - mu) - 1 < min_res) return false;             // the cheap necessary test: most stops end here
    const int shift = strand ? 5 : 1;
    const uint32_t want = (start_codons & 7u) << shift;
    int32_t x = -1;
    if (want) x = strand ? orf_find_down(sg, want, kOrfDownRStart, me + 1, mu - 1) : orf_find_up(sg, want, kOrfUpFStart, mu + 1, me - 1);
    const bool first = strand ? mu == sg.n : mu == -1;                        // u == -1
    if (x < 0 && want && !first) return false;
    *bcls = x < 0 ? 0u : (kOrfTables.cls[orf_codon_index(sg, x)] & want) >> shift;
    *mb = x >= 0 ? x : strand ? mu - 1 : mu + 1;
    return (strand ? *mb - me : me - *mb) >= min_res;
}

// rule 4 of the free candidates
__device__ inline kg_orf orf_free_record(int32_t seq, int strand, int32_t f, int64_t L, int32_t n, int32_t me, int32_t mu, int32_t mb,
                                         uint32_t bcls)
{
    const int32_t e = strand ? n - 1 - me : me, b = strand ? n - 1 - mb : mb;   // in j: e == n for the run that reaches the end
    const bool first = strand ? mu == n : mu == -1;
    const int32_t last = e < n ? e : n - 1;
    const int64_t xs = (int64_t)f + 3 * (int64_t)b, xe = (int64_t)f + 3 * (int64_t)last + 2;
    kg_orf o = {};
    o.seq = seq;
    o.strand = strand;
    o.frame = f;
    o.left = (int32_t)(strand ? L - 1 - xe : xs);
    o.right = (int32_t)(strand ? L - 1 - xs : xe);
    o.n_res = (e < n ? e : n) - b;
    o.start_codon = bcls & 1u ? 1 : bcls & 2u ? 2 : bcls & 4u ? 3 : 0;
    o.first_inner = -1;
    o.flags = KG_ORF_FREE | (e < n ? KG_ORF_HAS_STOP : 0u) | (first ? KG_ORF_PARTIAL5 : 0u);
    o.fI = -1;
    o.score = 0;
    o.kept = 1;
    return o;
}

// One wave per tile row, as orf_summary_kernel; keys: the scanned arrays.  slots: 6 * n_rows words, one per (container, tile) in
// output order: contig, strand, frame, and the tiles in the strand's codon order.  kEmit = false writes every slot's candidates
// there; kEmit = true reads the slot's first index from it and writes out[] and lens[] (= n_res) and adds to cnt[kOrfFree*].
template <bool kEmit>
__global__ __launch_bounds__(256) void orf_free_kernel(const uint8_t *__restrict__ seq, uint64_t total, OrfGeometry geo, uint64_t n_rows,
                                                       const int64_t *__restrict__ keys, int32_t min_res, uint32_t start_codons,
                                                       uint32_t *__restrict__ slots, kg_orf *__restrict__ out,
                                                       uint32_t *__restrict__ lens, unsigned long long *cnt)
{
    const int lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const OrfRow rw = orf_row_of(geo, row);
    uint32_t code[8];
    orf_row_codes(seq, total, rw, lane, code);
    const uint64_t below = (1ull << lane) - 1, above = lane == 63 ? 0ull : ~0ull << (lane + 1), self = 1ull << lane;
    const int32_t base = (int32_t)(rw.t * kOrfTile);
    uint32_t complete = 0, partial5 = 0;
#pragma unroll
    for (int g = 0; g < 3; g++) {
        uint32_t c[2];
#pragma unroll
        for (int k = 0; k < 2; k++) c[k] = kOrfTables.cls[code[g + 3 * k] * 25 + code[g + 3 * k + 1] * 5 + code[g + 3 * k + 2]];
        const uint64_t fs0 = __ballot(c[0] & kOrfFStop), fs1 = __ballot(c[1] & kOrfFStop);
        const uint64_t rs0 = __ballot(c[0] & kOrfRStop), rs1 = __ballot(c[1] & kOrfRStop);
        OrfSegment sg;
        sg.bytes = seq + rw.off + g;
        sg.keys = keys;
        sg.n_tiles = geo.n_tiles;
        sg.seg = 3 * rw.s + g;
        sg.mseg = 3 * geo.n_seqs - 1 - sg.seg;
        sg.gt0 = 3 * rw.tb + (uint64_t)g * rw.nt;
        sg.n = rw.L >= g ? (int32_t)((rw.L - g) / 3) : 0;
        const int32_t n = sg.n;
        const uint64_t gt = sg.gt0 + rw.t;
        for (int strand = 0; strand < 2; strand++) {
            const uint64_t s0 = strand ? rs0 : fs0, s1 = strand ? rs1 : fs1;
            // the neighbouring stop outside the tile: '+' the last one below it (-1: none), '-' the first one above it (n: none)
            int32_t outer = strand ? n : -1;
            if (!strand && rw.t > 0) {
                const int64_t k = keys[(uint64_t)kOrfDownFStop * geo.n_tiles + gt - 1];
                if (orf_key_seg(k) == sg.seg && orf_key_low(k) != 0) outer = (int32_t)orf_key_low(k) - 1;
            } else if (strand && rw.t + 1 < rw.nt) {
                const int64_t k = keys[(uint64_t)kOrfUpRStop * geo.n_tiles + (geo.n_tiles - 1 - (gt + 1))];
                if (orf_key_seg(k) == sg.mseg && orf_key_low(k) != 0) outer = (int32_t)(0x7FFFFFFFu - orf_key_low(k));
            }
            // [0], [1]: the lane's two codons as closing stops; [2]: lane 0 of the owning tile for the run that reaches the end
            bool has[3] = {false, false, false};
            int32_t me[3], mu[3], mb[3] = {0, 0, 0};
            uint32_t bc[3] = {0, 0, 0};
#pragma unroll
            for (int k = 0; k < 2; k++) {
                me[k] = base + 2 * lane + k;
                const int x = strand ? orf_first2(s0 & above, s1 & (k ? above : above | self))
                                     : orf_last2(s0 & (k ? below | self : below), s1 & below);
                mu[k] = x < 0 ? outer : base + x;
                if (c[k] & (strand ? kOrfRStop : kOrfFStop)) has[k] = orf_free_run(sg, strand, me[k], mu[k], min_res, start_codons, &mb[k], &bc[k]);
            }
            {
                me[2] = strand ? -1 : n;
                const int x = strand ? orf_first2(s0, s1) : orf_last2(s0, s1);
                mu[2] = x < 0 ? outer : base + x;
                const bool owner = strand ? rw.t == 0 : rw.t + 1 == rw.nt;
                if (owner && lane == 0 && n > 0) has[2] = orf_free_run(sg, strand, me[2], mu[2], min_res, start_codons, &mb[2], &bc[2]);
            }
            const uint64_t b0 = __ballot(has[0]), b1 = __ballot(has[1]), b2 = __ballot(has[2]);
            const int32_t f = strand ? (int32_t)((rw.L - g) % 3) : g;
            const uint64_t slot = 6 * rw.tb + (uint64_t)(3 * strand + f) * rw.nt + (strand ? rw.nt - 1 - rw.t : rw.t);
            if (!kEmit) {
                if (lane == 0) slots[slot] = (uint32_t)(__popcll(b0) + __popcll(b1) + __popcll(b2));
                continue;
            }
            // the ranks inside the slot, in the strand's codon order; the run that reaches the end comes last
            const uint64_t before = strand ? above : below;
            const uint32_t first = slots[slot], r = (uint32_t)(__popcll(b0 & before) + __popcll(b1 & before));
            const uint32_t rank[3] = {r + (strand && has[1] ? 1u : 0u), r + (!strand && has[0] ? 1u : 0u),
                                      (uint32_t)(__popcll(b0) + __popcll(b1))};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (!has[k]) continue;
                const kg_orf o = orf_free_record((int32_t)rw.s, strand, f, rw.L, n, me[k], mu[k], mb[k], bc[k]);
                out[first + rank[k]] = o;
                lens[first + rank[k]] = (uint32_t)o.n_res;
                complete += (o.flags & KG_ORF_HAS_STOP) && o.start_codon != 0 ? 1u : 0u;
                partial5 += o.flags & KG_ORF_PARTIAL5 ? 1u : 0u;
            }
        }
    }
    if (kEmit) {
        for (int off = 32; off > 0; off >>= 1) {
            complete += __shfl_down(complete, off);
            partial5 += __shfl_down(partial5, off);
        }
        if (lane == 0) {
            if (complete) atomicAdd(&cnt[kOrfFreeComplete], (unsigned long long)complete);
            if (partial5) atomicAdd(&cnt[kOrfFreePartial5], (unsigned long long)partial5);
        }
    }
}

// lens[i] = the bytes ORF i takes behind prot_start (kg_orfset_add_free: the given set's lengths, zeros of only_kept included)
__global__ __launch_bounds__(256) void orf_lens_kernel(const int64_t *__restrict__ prot_start, uint64_t n, uint32_t *__restrict__ lens)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lens[i] = (uint32_t)(prot_start[i + 1] - prot_start[i]);
}

// prot_start[i] = excl[i] for i < n, prot_start[n] = *total
__global__ __launch_bounds__(256) void orf_prot_start_kernel(const uint32_t *__restrict__ excl, const uint64_t *__restrict__ total,
                                                             uint64_t n, int64_t *__restrict__ prot_start)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    prot_start[i] = i < n ? (int64_t)excl[i] : (int64_t)*total;
}

// the last ORF i in [0, n) with prot_start[i] <= pos (pos < prot_start[n]): the one that holds residue pos
__device__ inline uint64_t orf_owner(const int64_t *__restrict__ prot_start, uint64_t n, int64_t pos)
{
    uint64_t lo = 0, hi = n;            // prot_start[lo] <= pos < prot_start[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (prot_start[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A lane owns residues [kOrfResPerLane * q, + kOrfResPerLane) of the concatenated proteins (rule 5).
__global__ __launch_bounds__(256) void orf_residues_kernel(const kg_orf *__restrict__ orfs, uint64_t n,
                                                           const int64_t *__restrict__ prot_start, uint64_t total,
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
            // the neighbour first (one-codon ORFs), else a new search: empty ORFs in between cost nothing
            i = (i + 2 <= n && prot_start[i + 1] <= pos && pos < prot_start[i + 2]) ? i + 1 : orf_owner(prot_start, n, pos);
            begin = prot_start[i];
            end = prot_start[i + 1];
            o = orfs[i];
        }
        const int64_t q = pos - begin;                                  // residue of ORF i
        const int64_t off = offsets[o.seq];
        uint32_t c0, c1, c2;
        if (!o.strand) {
            const uint8_t *p = seq + off + o.left + 3 * q;
            c0 = dna_code(p[0]); c1 = dna_code(p[1]); c2 = dna_code(p[2]);
        } else {
            const uint8_t *p = seq + off + o.right - 3 * q;
            c0 = dna_code(p[0]); c1 = dna_code(p[-1]); c2 = dna_code(p[-2]);
            c0 = c0 < 4 ? 3 - c0 : 4; c1 = c1 < 4 ? 3 - c1 : 4; c2 = c2 < 4 ? 3 - c2 : 4;
        }
        uint32_t ch = (uint8_t)kOrfTables.letter[c0 * 25 + c1 * 5 + c2];
        if (q == 0 && o.start_codon != 0) ch = 'M';
        word |= (uint64_t)ch << (8 * k);
    }
    if (k == kOrfResPerLane) {
        *reinterpret_cast<uint64_t *>(res + first) = word;
    } else {
        for (int b = 0; b < k; b++) res[first + b] = (uint8_t)(word >> (8 * b));
    }
}

// A repaired record (kg_repair.hpp) does not read in one frame, so orf_residues_kernel cannot rebuild its protein from the record.
// A stage that makes a set from a given one never changes such a record (it is KG_ORF_INTERRUPTED: not movable), so record i keeps
// its index and its length, and its protein is the given set's bytes.  A lane owns residues [kOrfResPerLane * q, + kOrfResPerLane)
// of the new proteins, as there, and writes those of repaired records only.
__global__ __launch_bounds__(256) void orf_keep_repaired_kernel(const kg_orf *__restrict__ orfs, uint64_t n,
                                                                const int64_t *__restrict__ prot_start, uint64_t total,
                                                                const int64_t *__restrict__ old_start, const uint8_t *__restrict__ old_res,
                                                                uint8_t *__restrict__ res)
{
    const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kOrfResPerLane;
    if (first >= total) return;
    uint64_t i = orf_owner(prot_start, n, (int64_t)first);
    int64_t begin = prot_start[i], end = prot_start[i + 1];
    bool repaired = (orfs[i].flags & KG_ORF_REPAIRED) != 0;
    for (int k = 0; k < kOrfResPerLane && first + k < total; k++) {
        const int64_t pos = (int64_t)(first + k);
        if (pos >= end) {
            i = (i + 2 <= n && prot_start[i + 1] <= pos && pos < prot_start[i + 2]) ? i + 1 : orf_owner(prot_start, n, pos);
            begin = prot_start[i];
            end = prot_start[i + 1];
            repaired = (orfs[i].flags & KG_ORF_REPAIRED) != 0;
        }
        if (repaired) res[pos] = old_res[old_start[i] + (pos - begin)];
    }
}

}  // namespace kg
