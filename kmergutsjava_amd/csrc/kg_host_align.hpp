// kg_host_align.hpp -- kg_proteins_align / kg_proteins_align_device: local alignment scores of protein pairs, and align_run, the
// step kg_proteins_cluster_aligned puts between its edge test and its component rounds (kernels: kg_align.hpp).  With a BandAsk
// align_run is the alignment step of kg_proteins_align_banded and kg_proteins_search_banded (kernel: kg_band.hpp).
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_derive.hpp (its offsets checks and its sequence
// staging) and in front of kg_host_cluster.hpp and kg_host_search.hpp, which call align_run.
#pragma once

static_assert(sizeof(kg_alignment) == 24 && sizeof(kg::AlignRec) == 24 && sizeof(kg_family_edge) == 32 && sizeof(kg_align_params) == 40 &&
              sizeof(kg_align_stats) == 40, "record layouts of include/kmerguts_hip.h");

// kg_proteins_align_ops: op_start[n + 1] (int64), then the ops, in one block of the set's context
struct kg_opset : SetBase {
    uint8_t *d_block = nullptr;
    int64_t n = 0, count = 0;           // records, ops
    float ms_ops = 0;
    const int64_t *starts() const { return (const int64_t *)d_block; }
    const uint32_t *ops() const { return (const uint32_t *)(d_block + ((size_t)n + 1) * 8); }
};

namespace {

constexpr uint32_t kAlignGrid = 256 * 18;               // workgroups of one wave: what 256 CUs hold at 9 KB of LDS each
constexpr uint32_t kAlignLongGrid = 1024;               // ... of the long-centre launch at most, and its slabs' bytes in all
constexpr uint64_t kAlignSlabBytes = 256ull << 20;

// the parameter checks both entry points share: the message names the first bad one
int align_check_params(const kg_align_params *p)
{
    if (p->min_ratio_pct < 0 || p->min_ratio_pct > 100) return fail(KG_ERR_ARG, "min_ratio_pct must be in 0..100");
    if (p->ref != KG_ALIGN_REF_LONGER && p->ref != KG_ALIGN_REF_MEMBER)
        return fail(KG_ERR_ARG, "ref must be KG_ALIGN_REF_LONGER or KG_ALIGN_REF_MEMBER");
    if (p->gap_open < 0) return fail(KG_ERR_ARG, "gap_open must be >= 0");
    if (p->gap_extend < 1) return fail(KG_ERR_ARG, "gap_extend must be >= 1");
    if (p->max_cells < 1) return fail(KG_ERR_ARG, "max_cells must be >= 1");
    if (p->reserved != 0) return fail(KG_ERR_ARG, "kg_align_params.reserved must be 0");
    if (p->matrix)
        for (int r = 0; r < 21; r++)
            for (int c = 0; c < 21; c++) {
                const int v = p->matrix[r * 21 + c];
                if (v < -16 || v > 16)
                    return fail(KG_ERR_ARG, "matrix entry (" + kmer_text(r) + ", " + kmer_text(c) + ") is outside -16..16");
                if (v != p->matrix[c * 21 + r])
                    return fail(KG_ERR_ARG, "matrix is not symmetric at (" + kmer_text(r) + ", " + kmer_text(c) + ")");
            }
    return KG_OK;
}

struct AlignTotals { int64_t cells = 0, skipped = 0, band_cells = 0; };

// kg_proteins_align_banded / kg_proteins_search_banded: one diagonal per pair (host) and the half-width W
struct BandAsk { const int32_t *diag; int band; };

static_assert(KG_BAND_MAX == kg::kBandMax && sizeof(kg_band_params) == 16 && sizeof(kg_band_stats) == 24, "the band of include/kmerguts_hip.h");

int band_check_params(const kg_band_params *b)
{
    if (!b) return fail(KG_ERR_ARG, "null kg_band_params");
    if (b->band < 0 || b->band > KG_BAND_MAX) return fail(KG_ERR_ARG, "band must be in [0, 256]");
    if (b->reserved[0] != 0 || b->reserved[1] != 0 || b->reserved[2] != 0) return fail(KG_ERR_ARG, "kg_band_params.reserved must be 0");
    return KG_OK;
}

// Pairs (a, b) of the proteins at d_seq / d_off (offsets: the same on the host) -> one AlignRec per pair in the call's scratch,
// in pair order; *d_pairs_out: the uploaded pairs.  The pairs are handed out in descending order of their cells; a pair whose b
// is longer than kAlignLdsCols goes to the launch that carries its stripes' last rows in device memory.
// band: align_band_kernel in their place, one launch (its carry always fits LDS), the order and the cap by the band cells;
// tot->cells stays the n * m of the aligned pairs and tot->band_cells is their band cells.
int align_run(kg_table *t, Scratch &sc, const kg_align_params *prm, const uint8_t *d_seq, const int64_t *d_off, const int64_t *offsets,
              const int32_t *h_pairs, uint64_t n_pairs, const int32_t **d_pairs_out, kg::AlignRec **d_out, AlignTotals *tot,
              const BandAsk *band = nullptr)
{
    hipStream_t s = t->stream;
    int rc;
    std::vector<uint32_t> order[2];                     // [1]: the long centres
    std::vector<uint64_t> cells(n_pairs);
    uint64_t slab_cols = 0;
    for (uint64_t k = 0; k < n_pairs; k++) {
        const int64_t n = offsets[h_pairs[2 * k] + 1] - offsets[h_pairs[2 * k]], m = offsets[h_pairs[2 * k + 1] + 1] - offsets[h_pairs[2 * k + 1]];
        const int64_t counted = band ? kg::band_cells(n, m, band->band) : n * m;       // (n, m < 2^24: no overflow)
        const bool skip = counted > prm->max_cells;
        cells[k] = skip ? 0 : (uint64_t)counted;
        if (skip) tot->skipped++; else { tot->cells += n * m; tot->band_cells += counted; }
        const bool lng = !skip && m > kg::kAlignLdsCols;
        const bool slab = lng && !band;                 // (the band's carry always fits LDS)
        if (slab) slab_cols = std::max<uint64_t>(slab_cols, ((uint64_t)m + 63) / 64 * 64);
        order[slab].push_back((uint32_t)k);
    }
    for (auto &o : order) std::stable_sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { return cells[x] > cells[y]; });
    const uint64_t n_short = order[0].size(), n_long = order[1].size();
    order[0].insert(order[0].end(), order[1].begin(), order[1].end());

    int32_t *d_pairs = nullptr;
    uint32_t *d_order = nullptr;
    unsigned int *d_counter = nullptr;
    int8_t *d_matrix = nullptr;
    int2 *d_slab = nullptr;
    int32_t *d_diag = nullptr;
    uint32_t long_grid = 0;
    if ((rc = sc.get(&d_pairs, std::max<uint64_t>(2 * n_pairs, 2))) || (rc = sc.get(&d_order, std::max<uint64_t>(n_pairs, 1))) ||
        (rc = sc.get(&d_counter, 2)) || (rc = sc.get(d_out, std::max<uint64_t>(n_pairs, 1))))
        return rc;
    if (prm->matrix && (rc = sc.get(&d_matrix, 21 * 21))) return rc;
    if (band && (rc = sc.get(&d_diag, std::max<uint64_t>(n_pairs, 1)))) return rc;
    if (n_long) {
        long_grid = (uint32_t)std::min<uint64_t>({n_long, (uint64_t)kAlignLongGrid, std::max<uint64_t>(1, kAlignSlabBytes / (slab_cols * 8))});
        if ((rc = sc.get(&d_slab, (size_t)long_grid * slab_cols))) return rc;
    }
    *d_pairs_out = d_pairs;
    HIP_TRY(hipMemsetAsync(d_counter, 0, 8, s));
    if (n_pairs) {
        HIP_TRY(hipMemcpyAsync(d_pairs, h_pairs, n_pairs * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_order, order[0].data(), n_pairs * 4, hipMemcpyHostToDevice, s));
        if (band) HIP_TRY(hipMemcpyAsync(d_diag, band->diag, n_pairs * 4, hipMemcpyHostToDevice, s));
    }
    if (d_matrix) HIP_TRY(hipMemcpyAsync(d_matrix, prm->matrix, 21 * 21, hipMemcpyHostToDevice, s));
    const int open = std::min(prm->gap_open, kg::kAlignGapCap), ext = std::min(prm->gap_extend, kg::kAlignGapCap);
    if (band && n_short)
        hipLaunchKernelGGL(kg::align_band_kernel, dim3((uint32_t)std::min<uint64_t>(n_short, kAlignGrid)), dim3(kg::kWave), 0, s, d_seq, d_off,
                           d_pairs, d_diag, d_order, (uint32_t)n_short, d_counter, d_matrix, open, ext, (int64_t)prm->max_cells, band->band,
                           *d_out);
    if (!band && n_short)
        hipLaunchKernelGGL(kg::align_pairs_kernel<false>, dim3((uint32_t)std::min<uint64_t>(n_short, kAlignGrid)), dim3(kg::kWave), 0, s, d_seq,
                           d_off, d_pairs, d_order, (uint32_t)n_short, d_counter, d_matrix, open, ext, (int64_t)prm->max_cells, nullptr,
                           (uint64_t)0, *d_out);
    if (n_long)
        hipLaunchKernelGGL(kg::align_pairs_kernel<true>, dim3(long_grid), dim3(kg::kWave), 0, s, d_seq, d_off, d_pairs, d_order + n_short,
                           (uint32_t)n_long, d_counter + 1, d_matrix, open, ext, (int64_t)prm->max_cells, d_slab, slab_cols, *d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));                   // (the host vectors above are the copies' sources)
    return KG_OK;
}

// kg_proteins_align_paths: the paths asked for beside the records (kg_host_trace.hpp runs the pass behind align_run)
// kg_proteins_align_ops: the ops as well, in `set` (ops_mode: KG_TRACE_OPS or KG_TRACE_OPS_EQX; 0: none)
struct AlignPathsAsk { int64_t max_trace_cells; kg_alignment_path *paths; int ops_mode = 0; kg_opset *set = nullptr; };
int align_ops_empty(kg_table *t, kg_opset *set);
int align_paths_behind(kg_table *t, Scratch &sc, const kg_align_params *prm, const uint8_t *d_seq, const int64_t *d_off, const int32_t *pairs,
                       int64_t n_pairs, const kg_alignment *aln, const AlignPathsAsk *ask, const BandAsk *band);

int align_impl(kg_table *t, const kg_align_params *prm, const uint8_t *h_seq, const uint8_t *d_seq_in, const int64_t *offsets, int64_t n_prot,
               const int32_t *pairs, int64_t n_pairs, kg_alignment *out, const AlignPathsAsk *ask, const BandAsk *band)
{
    if (n_pairs == 0) return ask && ask->set ? align_ops_empty(t, ask->set) : KG_OK;
    hipStream_t s = t->stream;
    Scratch sc(t);
    int rc;
    const uint8_t *d_seq = nullptr;
    if ((rc = stage_sequence(t, sc, h_seq, d_seq_in, (uint64_t)offsets[n_prot], &d_seq))) return rc;
    int64_t *d_off = nullptr;
    if ((rc = sc.get(&d_off, (size_t)n_prot + 1))) return rc;
    HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)n_prot + 1) * 8, hipMemcpyHostToDevice, s));
    const int32_t *d_pairs = nullptr;
    kg::AlignRec *d_out = nullptr;
    AlignTotals tot;
    if ((rc = align_run(t, sc, prm, d_seq, d_off, offsets, pairs, (uint64_t)n_pairs, &d_pairs, &d_out, &tot, band))) return rc;
    HIP_TRY(hipMemcpy(out, d_out, (size_t)n_pairs * sizeof(kg_alignment), hipMemcpyDeviceToHost));
    return ask ? align_paths_behind(t, sc, prm, d_seq, d_off, pairs, n_pairs, out, ask, band) : KG_OK;
}

int align_entry(int device, const kg_align_params *prm, const uint8_t *h_seq, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                const int32_t *pairs, int64_t n_pairs, kg_alignment *out, const AlignPathsAsk *ask_in = nullptr, kg_opset **ops_out = nullptr,
                const BandAsk *band = nullptr)
{
    if (!prm) return fail(KG_ERR_ARG, "null kg_align_params");
    int rc;
    if ((rc = align_check_params(prm))) return rc;
    if (n_prot < 0) return fail(KG_ERR_ARG, "n_prot < 0");
    if (n_prot >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more proteins in one call");
    if (n_pairs < 0) return fail(KG_ERR_ARG, "n_pairs < 0");
    if (n_pairs >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more pairs in one call");
    if ((rc = check_protein_offsets(offsets, n_prot, (int64_t)kg::kAlignMaxLen, "2^24"))) return rc;
    if (n_pairs && (!pairs || !out)) return fail(KG_ERR_ARG, "null argument");
    if (ask_in && ask_in->max_trace_cells < 1) return fail(KG_ERR_ARG, "max_trace_cells must be >= 1");
    if (ask_in && n_pairs && !ask_in->paths) return fail(KG_ERR_ARG, "null paths");
    if (band && n_pairs && !band->diag) return fail(KG_ERR_ARG, "null diagonals");
    for (int64_t k = 0; k < 2 * n_pairs; k++)
        if (pairs[k] < 0 || pairs[k] >= n_prot)
            return fail(KG_ERR_ARG, "pair " + kmer_text(k / 2) + ": protein index " + kmer_text(pairs[k]) + " is outside [0, n_prot)");
    const uint64_t seq_bytes = n_prot ? (uint64_t)offsets[n_prot] : 0;
    if (seq_bytes && n_pairs && !h_seq && !d_seq) return fail(KG_ERR_ARG, "null sequence");
    CallScope cs(device);
    if (cs.rc) return cs.rc;
    std::unique_ptr<kg_opset> set;                      // kg_proteins_align_ops only: the set keeps the context and its block
    AlignPathsAsk with_set;
    const AlignPathsAsk *ask = ask_in;
    if (ops_out) {
        if ((rc = make_set(cs, set))) return rc;
        with_set = *ask_in;
        with_set.set = set.get();
        ask = &with_set;
    }
    rc = d_seq && hipDeviceSynchronize() != hipSuccess ? fail(KG_ERR_DEVICE, "hipDeviceSynchronize failed") : KG_OK;
    if (!rc) rc = align_impl(cs.t, prm, h_seq, d_seq, offsets, n_prot, pairs, n_pairs, out, ask, band);
    if (!rc && ops_out) return hand_out(cs, set, ops_out);      // (the scratch, back in the cache, goes to the driver there)
    cs.t->cache.release_all();                          // scratch goes back to the driver
    return rc;
}

}  // namespace

extern "C" {

int kg_proteins_align(int device, const kg_align_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot, const int32_t *pairs,
                      int64_t n_pairs, kg_alignment *out)
{
    return align_entry(device, p, seq, nullptr, offsets, n_prot, pairs, n_pairs, out);
}

int kg_proteins_align_device(int device, const kg_align_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                             const int32_t *pairs, int64_t n_pairs, kg_alignment *out)
{
    return align_entry(device, p, nullptr, d_seq, offsets, n_prot, pairs, n_pairs, out);
}

}  // extern "C"
