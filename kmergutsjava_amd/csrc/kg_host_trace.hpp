// kg_host_trace.hpp -- the traceback pass behind align_run (kernels: kg_trace.hpp, kg_ops.hpp): trace_run, which
// kg_proteins_align_paths and kg_proteins_search_paths call with the end cells the alignment pass found, the ops behind it when a
// call asks for them (KG_TRACE_OPS, KG_TRACE_OPS_EQX), and the kg_proteins_align_paths / kg_proteins_align_ops entry points.
// Part of kmerguts_hip.hip's translation unit, behind kg_host_align.hpp.
#pragma once

static_assert(sizeof(kg_alignment_path) == 32 && sizeof(kg::TracePath) == 32 && sizeof(kg::TraceJob) == 24 && sizeof(kg_trace_stats) == 32 &&
                  sizeof(kg::OpsRec) == 16,
              "record layouts of include/kmerguts_hip.h");
static_assert(KG_OP_M == kg::kOpM && KG_OP_I == kg::kOpI && KG_OP_D == kg::kOpD && KG_OP_EQ == kg::kOpEq && KG_OP_X == kg::kOpX, "op codes");

namespace {

constexpr uint32_t kTraceGrid = 256 * 18;               // workgroups of one wave, as kAlignGrid: the LDS is align_pairs_kernel's
constexpr uint32_t kTraceLongGrid = 1024;               // ... of the large-box launch at most
constexpr uint64_t kTraceShortSlabBytes = 512ull << 10; // a box whose direction words fit this goes to the wide launch
constexpr uint64_t kTraceSlabBytes = 2048ull << 20;     // direction words and carries of one launch in all (the launches share them)

struct TraceTotals { int64_t traced = 0, untraced = 0, cells = 0; float ms = 0; };

// The ops a call asks for beside the paths.  mode: KG_TRACE_OPS or KG_TRACE_OPS_EQX.  -> d_block: op_start[n_pairs + 1] (int64), then
// `count` ops, a block of the call's scratch that the caller keeps (SetBase::keep) or detaches; ms: the prefix sum and the fill.
struct OpsAsk { int mode; uint8_t *d_block = nullptr; int64_t count = 0; float ms = 0; };

// the staging words of one call at most, in bytes: kTraceSlabBytes, or what the test hook KG_TEST_OPS_STAGE_BYTES lowers it to
uint64_t ops_stage_limit()
{
    const uint32_t hook = test_hook("KG_TEST_OPS_STAGE_BYTES");
    return hook ? (uint64_t)hook : kTraceSlabBytes;
}

// what the alignment pass found for a pair, and whether the pair asks for a path
struct TraceEnd { int score, end_a, end_b; bool want; };

// Pairs (a, b) with their ends -> one TracePath per pair in the call's scratch, in pair order.  A pair is traced iff it asks,
// its score is >= 1 and its box has at most max_trace_cells cells.  The pairs are handed out in descending order of their box
// cells; a box whose columns do not fit the LDS carry or whose direction words exceed kTraceShortSlabBytes goes to the second
// launch, whose few workgroups own large slabs, so that one large pair does not narrow the launch of the small ones.
// ops: the walk records its columns into staging words (trace_columns_kernel in trace_pairs_kernel's place), the op counts are
// summed in pair order and ops_fill_kernel writes the ops; tot->ms then covers that work as well.
// band: the same boxes, launches and slabs with the cells outside the band of pair k's diagonal forced to H = 0
// (trace_band_kernel, trace_band_columns_kernel).
int trace_run(kg_table *t, Scratch &sc, const kg_align_params *prm, const uint8_t *d_seq, const int64_t *d_off, const int32_t *h_pairs,
              const std::vector<TraceEnd> &ends, uint64_t n_pairs, int64_t max_trace_cells, kg::TracePath **d_out, TraceTotals *tot,
              OpsAsk *ops = nullptr, const BandAsk *band = nullptr)
{
    hipStream_t s = t->stream;
    int rc;
    Events<4> ev;
    if ((rc = ev.create())) return rc;
    std::vector<uint32_t> order[2];                     // [1]: the large boxes
    std::vector<uint64_t> cells(n_pairs);
    std::vector<kg::OpsRec> recs(ops ? n_pairs : 0);
    uint64_t words[2] = {0, 0}, carry_cols = 0;         // per workgroup: direction words of each launch, carry columns of the second
    for (uint64_t k = 0; k < n_pairs; k++) {
        const TraceEnd &e = ends[k];
        const bool want = e.want && e.score > 0 && e.end_a >= 0 && e.end_b >= 0;
        const uint64_t na = want ? (uint64_t)e.end_a + 1 : 0, mb = want ? (uint64_t)e.end_b + 1 : 0;
        const bool over = want && na * mb > (uint64_t)max_trace_cells;      // (na, mb < 2^24: no overflow)
        const bool go = want && !over;
        cells[k] = go ? na * mb : 0;
        if (go) { tot->traced++; tot->cells += (int64_t)(na * mb); }
        if (over) tot->untraced++;
        const uint64_t w = go ? (na + kg::kWave - 1) / kg::kWave * kg::trace_stripe_words(mb) : 0;
        const bool lng = go && (mb > (uint64_t)kg::kAlignLdsCols || w * 4 > kTraceShortSlabBytes);
        if (ops) recs[k] = kg::OpsRec{go ? kg::trace_stage_words(na, mb) : 0, e.end_a, e.end_b};      // (the words: the offset below)
        words[lng] = std::max(words[lng], w);
        if (lng) carry_cols = std::max(carry_cols, (mb + 63) / 64 * 64);
        order[lng].push_back((uint32_t)k);
    }
    for (auto &o : order) std::stable_sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { return cells[x] > cells[y]; });
    const uint64_t n_short = order[0].size(), n_long = order[1].size();
    std::vector<kg::TraceJob> jobs;
    jobs.reserve(n_pairs);
    for (auto &o : order)
        for (uint32_t k : o) jobs.push_back(kg::TraceJob{h_pairs[2 * (size_t)k], h_pairs[2 * (size_t)k + 1], ends[k].want ? ends[k].score : 0,
                                                         ends[k].end_a, ends[k].end_b, (int)k});
    uint64_t stage_words = 0;                           // the staging regions, laid out in hand-out order
    if (ops) {
        for (const kg::TraceJob &j : jobs) {
            const uint64_t w = recs[(size_t)j.slot].stage_at;
            recs[(size_t)j.slot].stage_at = stage_words;
            stage_words += w;
        }
        if (stage_words * 4 > ops_stage_limit())
            return fail(KG_ERR_LIMIT, "the alignments' columns need " + kmer_text((int64_t)(stage_words * 4)) +
                                          " bytes of staging, over the " + kmer_text((int64_t)ops_stage_limit()) + " one call holds");
    }
    const uint32_t short_grid =
        (uint32_t)std::min<uint64_t>({n_short, (uint64_t)kTraceGrid, std::max<uint64_t>(1, kTraceSlabBytes / std::max<uint64_t>(words[0] * 4, 1))});
    const uint32_t long_grid = (uint32_t)std::min<uint64_t>(
        {n_long, (uint64_t)kTraceLongGrid, std::max<uint64_t>(1, kTraceSlabBytes / std::max<uint64_t>(words[1] * 4 + carry_cols * 8, 1))});

    kg::TraceJob *d_jobs = nullptr;
    uint32_t *d_dirs = nullptr;
    unsigned int *d_words = nullptr;                    // the two hand-out counters and the error bits
    int8_t *d_matrix = nullptr;
    int2 *d_carry = nullptr;
    kg::TraceBandJob *d_bjobs = nullptr;                // under a band the jobs carry their diagonal and W
    std::vector<kg::TraceBandJob> bjobs;
    if (band) {
        bjobs.reserve(n_pairs);
        for (const kg::TraceJob &j : jobs)
            bjobs.push_back(kg::TraceBandJob{j.a, j.b, j.score, j.end_a, j.end_b, j.slot, band->diag[j.slot], band->band});
        if ((rc = sc.get(&d_bjobs, std::max<uint64_t>(n_pairs, 1)))) return rc;
    }
    if ((rc = sc.get(&d_jobs, std::max<uint64_t>(n_pairs, 1))) || (rc = sc.get(&d_words, kg::kTraceWords + 1)) ||
        (rc = sc.get(d_out, std::max<uint64_t>(n_pairs, 1))) ||
        (rc = sc.get(&d_dirs, std::max<uint64_t>({(uint64_t)short_grid * words[0], (uint64_t)long_grid * words[1], 1}))))
        return rc;
    if (prm->matrix && (rc = sc.get(&d_matrix, 21 * 21))) return rc;
    if (n_long && (rc = sc.get(&d_carry, (size_t)long_grid * carry_cols))) return rc;
    kg::OpsRec *d_recs = nullptr;
    uint32_t *d_stage = nullptr, *d_nops = nullptr, *d_opx = nullptr;
    uint64_t *d_partial = nullptr, *d_total = nullptr;
    kg::TraceOpsArgs *d_oa = nullptr;
    if (ops && ((rc = sc.get(&d_oa, 1)) || (rc = sc.get(&d_recs, std::max<uint64_t>(n_pairs, 1))) || (rc = sc.get(&d_stage, std::max<uint64_t>(stage_words, 1))) ||
                (rc = sc.get(&d_nops, std::max<uint64_t>(n_pairs, 1))) || (rc = sc.get(&d_opx, std::max<uint64_t>(n_pairs, 1))) ||
                (rc = sc.get(&d_partial, n_pairs / kg::kScanChunk + 3)) || (rc = sc.get(&d_total, 1))))
        return rc;
    const int eqx = ops && ops->mode == KG_TRACE_OPS_EQX;
    HIP_TRY(hipEventRecord(ev[0], s));
    const kg::TraceOpsArgs oa{d_recs, d_stage, d_nops, eqx};
    if (ops) HIP_TRY(hipMemcpyAsync(d_oa, &oa, sizeof oa, hipMemcpyHostToDevice, s));
    if (ops && n_pairs) HIP_TRY(hipMemcpyAsync(d_recs, recs.data(), n_pairs * sizeof(kg::OpsRec), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_words, 0, (kg::kTraceWords + 1) * 4, s));
    if (n_pairs) HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), n_pairs * sizeof(kg::TraceJob), hipMemcpyHostToDevice, s));
    if (d_matrix) HIP_TRY(hipMemcpyAsync(d_matrix, prm->matrix, 21 * 21, hipMemcpyHostToDevice, s));
    if (band && n_pairs) HIP_TRY(hipMemcpyAsync(d_bjobs, bjobs.data(), n_pairs * sizeof(kg::TraceBandJob), hipMemcpyHostToDevice, s));
    const int open = std::min(prm->gap_open, kg::kAlignGapCap), ext = std::min(prm->gap_extend, kg::kAlignGapCap);
    // (one stream: the second launch starts behind the first, so the two share the direction words)
    if (band) {
        if (ops && n_short)
            hipLaunchKernelGGL(kg::trace_band_columns_kernel<false>, dim3(short_grid), dim3(kg::kWave), 0, s, d_seq, d_off, d_bjobs,
                               (uint32_t)n_short, d_words, d_matrix, open, ext, max_trace_cells, d_dirs, words[0], nullptr, (uint64_t)0, *d_out,
                               d_oa);
        if (ops && n_long)
            hipLaunchKernelGGL(kg::trace_band_columns_kernel<true>, dim3(long_grid), dim3(kg::kWave), 0, s, d_seq, d_off, d_bjobs + n_short,
                               (uint32_t)n_long, d_words, d_matrix, open, ext, max_trace_cells, d_dirs, words[1], d_carry, carry_cols, *d_out,
                               d_oa);
        if (!ops && n_short)
            hipLaunchKernelGGL(kg::trace_band_kernel<false>, dim3(short_grid), dim3(kg::kWave), 0, s, d_seq, d_off, d_bjobs, (uint32_t)n_short,
                               d_words, d_matrix, open, ext, max_trace_cells, d_dirs, words[0], nullptr, (uint64_t)0, *d_out);
        if (!ops && n_long)
            hipLaunchKernelGGL(kg::trace_band_kernel<true>, dim3(long_grid), dim3(kg::kWave), 0, s, d_seq, d_off, d_bjobs + n_short,
                               (uint32_t)n_long, d_words, d_matrix, open, ext, max_trace_cells, d_dirs, words[1], d_carry, carry_cols, *d_out);
    } else if (ops) {
        if (n_short)
            hipLaunchKernelGGL(kg::trace_columns_kernel<false>, dim3(short_grid), dim3(kg::kWave), 0, s, d_seq, d_off, d_jobs, (uint32_t)n_short,
                               d_words, d_matrix, open, ext, max_trace_cells, d_dirs, words[0], nullptr, (uint64_t)0, *d_out, d_oa);
        if (n_long)
            hipLaunchKernelGGL(kg::trace_columns_kernel<true>, dim3(long_grid), dim3(kg::kWave), 0, s, d_seq, d_off, d_jobs + n_short,
                               (uint32_t)n_long, d_words, d_matrix, open, ext, max_trace_cells, d_dirs, words[1], d_carry, carry_cols, *d_out,
                               d_oa);
    } else if (n_short)
        hipLaunchKernelGGL(kg::trace_pairs_kernel<false>, dim3(short_grid), dim3(kg::kWave), 0, s, d_seq, d_off, d_jobs, (uint32_t)n_short,
                           d_words, d_matrix, open, ext, max_trace_cells, d_dirs, words[0], nullptr, (uint64_t)0, *d_out);
    if (!band && !ops && n_long)
        hipLaunchKernelGGL(kg::trace_pairs_kernel<true>, dim3(long_grid), dim3(kg::kWave), 0, s, d_seq, d_off, d_jobs + n_short,
                           (uint32_t)n_long, d_words, d_matrix, open, ext, max_trace_cells, d_dirs, words[1], d_carry, carry_cols, *d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], s));
    unsigned int h_err = 0;
    HIP_TRY(hipMemcpyAsync(&h_err, d_words + kg::kTraceWords - 1, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                   // (the host vectors above are the copies' sources)
    if (h_err & kg::kTraceErrScore) return fail(KG_ERR_DEVICE, "internal: a prefix box does not reproduce its pair's score");
    if (h_err & kg::kTraceErrWalk) return fail(KG_ERR_DEVICE, "internal: a traceback walk left the rule or did not end");
    if (h_err & kg::kTraceErrSlab) return fail(KG_ERR_DEVICE, "internal: a traced pair does not fit its workgroup's slab");
    tot->ms = ev.ms(0, 1);
    if (!ops) return KG_OK;

    // ---- the ops: the counts summed in pair order, the block of the exact size, the fill ----
    uint64_t total = 0;
    HIP_TRY(hipEventRecord(ev[2], s));
    if ((rc = prefix_sum(t, d_nops, n_pairs, d_opx, d_partial, d_total))) return rc;
    HIP_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (total >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more ops in one call");      // (d_opx is exact below that)
    const size_t start_bytes = ((size_t)n_pairs + 1) * 8;
    if ((rc = sc.get(&ops->d_block, start_bytes + std::max<uint64_t>(total, 1) * 4))) return rc;
    int64_t *const d_start = (int64_t *)ops->d_block;
    hipLaunchKernelGGL(kg::ops_starts_kernel, dim3(std::min<uint32_t>(grid_of(n_pairs + 1), 4096u)), dim3(256), 0, s, d_opx, n_pairs, d_total,
                       d_start);
    if (n_pairs)
        hipLaunchKernelGGL(kg::ops_fill_kernel, dim3(std::min<uint32_t>(grid_of(n_pairs, kg::kOpsThreads / kg::kWave), 256u * 8)),
                           dim3(kg::kOpsThreads), 0, s, *d_out, d_recs, d_stage, d_nops, d_start, n_pairs, eqx,
                           (uint32_t *)(ops->d_block + start_bytes), d_words + kg::kTraceWords - 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[3], s));
    HIP_TRY(hipMemcpyAsync(&h_err, d_words + kg::kTraceWords - 1, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h_err & kg::kTraceErrOps) return fail(KG_ERR_DEVICE, "internal: a record's ops and its counted kind changes differ");
    ops->count = (int64_t)total;
    ops->ms = ev.ms(2, 3);
    tot->ms = ev.ms(0, 3);
    return KG_OK;
}

// what kg_proteins_align_paths does behind align_run: every aligned pair asks for a path
int align_paths_behind(kg_table *t, Scratch &sc, const kg_align_params *prm, const uint8_t *d_seq, const int64_t *d_off, const int32_t *pairs,
                       int64_t n_pairs, const kg_alignment *aln, const AlignPathsAsk *ask, const BandAsk *band)
{
    std::vector<TraceEnd> ends((size_t)n_pairs);
    for (int64_t k = 0; k < n_pairs; k++) ends[(size_t)k] = TraceEnd{aln[k].score, aln[k].end_a, aln[k].end_b, aln[k].status == 0};
    kg::TracePath *d_paths = nullptr;
    TraceTotals tot;
    OpsAsk ops{ask->ops_mode};
    if (int rc = trace_run(t, sc, prm, d_seq, d_off, pairs, ends, (uint64_t)n_pairs, ask->max_trace_cells, &d_paths, &tot,
                           ask->set ? &ops : nullptr, band))
        return rc;
    HIP_TRY(hipMemcpy(ask->paths, d_paths, (size_t)n_pairs * sizeof(kg_alignment_path), hipMemcpyDeviceToHost));
    if (kg_opset *set = ask->set) {
        set->d_block = set->keep(sc, ops.d_block);      // the set's block leaves the scratch: everything else goes back to the cache
        set->n = n_pairs;
        set->count = ops.count;
        set->ms_ops = ops.ms;
    }
    return KG_OK;
}

// no pairs: op_start[0] = 0 and no ops
int align_ops_empty(kg_table *t, kg_opset *set)
{
    Scratch sc(t);
    uint8_t *p = nullptr;
    if (int rc = sc.get(&p, 16)) return rc;
    HIP_TRY(hipMemsetAsync(p, 0, 16, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    set->d_block = set->keep(sc, p);
    return KG_OK;
}

// the getters' shared checks: starts [first, first + count] and ops [first, first + count) of a block made with ops
int ops_starts_copy(const void *s, int device, const int64_t *src, int64_t n, int64_t first, int64_t count, int64_t *dst, const char *what)
{
    if (s && (first < 0 || count < 0 || first + count > n)) return fail(KG_ERR_ARG, std::string(what) + ": range outside the set");
    return copy_records(s, device, src, 1, n + 1, first, count + 1, dst, what);
}

int align_ops_entry(int device, const kg_align_params *p, const uint8_t *h_seq, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                    const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, int ops_mode, kg_alignment *out, kg_alignment_path *paths,
                    kg_opset **ops)
{
    if (!ops) return fail(KG_ERR_ARG, "null argument");
    *ops = nullptr;
    if (ops_mode != KG_TRACE_OPS && ops_mode != KG_TRACE_OPS_EQX) return fail(KG_ERR_ARG, "ops_mode must be KG_TRACE_OPS or KG_TRACE_OPS_EQX");
    const AlignPathsAsk ask{max_trace_cells, paths, ops_mode};
    return align_entry(device, p, h_seq, d_seq, offsets, n_prot, pairs, n_pairs, out, &ask, ops);
}

// kg_proteins_align_banded: the records alone, with paths, or with paths and ops
int align_banded_entry(int device, const kg_align_params *p, const uint8_t *h_seq, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                       const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, int ops_mode, kg_alignment *out, kg_alignment_path *paths,
                       kg_opset **ops, const kg_band_params *band, const int32_t *diagonals)
{
    if (ops) *ops = nullptr;
    if (int rc = band_check_params(band)) return rc;
    if (ops && !paths && n_pairs) return fail(KG_ERR_ARG, "ops without paths");
    if (!ops && ops_mode != 0) return fail(KG_ERR_ARG, "ops_mode must be 0 without ops");
    const BandAsk b{diagonals, band->band};
    if (ops) {
        if (ops_mode != KG_TRACE_OPS && ops_mode != KG_TRACE_OPS_EQX) return fail(KG_ERR_ARG, "ops_mode must be KG_TRACE_OPS or KG_TRACE_OPS_EQX");
        const AlignPathsAsk ask{max_trace_cells, paths, ops_mode};
        return align_entry(device, p, h_seq, d_seq, offsets, n_prot, pairs, n_pairs, out, &ask, ops, &b);
    }
    const AlignPathsAsk ask{max_trace_cells, paths};
    return align_entry(device, p, h_seq, d_seq, offsets, n_prot, pairs, n_pairs, out, paths ? &ask : nullptr, nullptr, &b);
}

}  // namespace

extern "C" {

int kg_proteins_align_banded(int device, const kg_align_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                             const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, int ops_mode, kg_alignment *out,
                             kg_alignment_path *paths, kg_opset **ops, const kg_band_params *band, const int32_t *diagonals)
{
    return align_banded_entry(device, p, seq, nullptr, offsets, n_prot, pairs, n_pairs, max_trace_cells, ops_mode, out, paths, ops, band, diagonals);
}

int kg_proteins_align_banded_device(int device, const kg_align_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                                    const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, int ops_mode, kg_alignment *out,
                                    kg_alignment_path *paths, kg_opset **ops, const kg_band_params *band, const int32_t *diagonals)
{
    return align_banded_entry(device, p, nullptr, d_seq, offsets, n_prot, pairs, n_pairs, max_trace_cells, ops_mode, out, paths, ops, band,
                              diagonals);
}

int kg_proteins_align_paths(int device, const kg_align_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                            const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, kg_alignment *out, kg_alignment_path *paths)
{
    const AlignPathsAsk ask{max_trace_cells, paths};
    return align_entry(device, p, seq, nullptr, offsets, n_prot, pairs, n_pairs, out, &ask);
}

int kg_proteins_align_paths_device(int device, const kg_align_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                                   const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, kg_alignment *out,
                                   kg_alignment_path *paths)
{
    const AlignPathsAsk ask{max_trace_cells, paths};
    return align_entry(device, p, nullptr, d_seq, offsets, n_prot, pairs, n_pairs, out, &ask);
}

int kg_proteins_align_ops(int device, const kg_align_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                          const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, int ops_mode, kg_alignment *out,
                          kg_alignment_path *paths, kg_opset **ops)
{
    return align_ops_entry(device, p, seq, nullptr, offsets, n_prot, pairs, n_pairs, max_trace_cells, ops_mode, out, paths, ops);
}

int kg_proteins_align_ops_device(int device, const kg_align_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                                 const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, int ops_mode, kg_alignment *out,
                                 kg_alignment_path *paths, kg_opset **ops)
{
    return align_ops_entry(device, p, nullptr, d_seq, offsets, n_prot, pairs, n_pairs, max_trace_cells, ops_mode, out, paths, ops);
}

int64_t kg_opset_ops_count(const kg_opset *s) { return s ? s->count : 0; }

int kg_opset_op_starts_copy(const kg_opset *s, int64_t first, int64_t count, int64_t *dst)
{
    return ops_starts_copy(s, device_of(s), s ? s->starts() : nullptr, s ? s->n : 0, first, count, dst, "kg_opset_op_starts_copy");
}

int kg_opset_ops_copy(const kg_opset *s, int64_t first_op, int64_t count, uint32_t *dst)
{
    return copy_records(s, device_of(s), s ? s->ops() : nullptr, 1, s ? s->count : 0, first_op, count, dst, "kg_opset_ops_copy");
}

int kg_opset_ms_ops(const kg_opset *s, float *out)
{
    if (!s || !out) return fail(KG_ERR_ARG, "null argument");
    *out = s->ms_ops;
    return KG_OK;
}

void kg_opset_free(kg_opset *s) { delete s; }

}  // extern "C"
