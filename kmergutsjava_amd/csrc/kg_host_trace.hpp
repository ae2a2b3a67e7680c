// kg_host_trace.hpp -- the traceback pass behind align_run (kernel: kg_trace.hpp): trace_run, which kg_proteins_align_paths and
// kg_proteins_search_paths call with the end cells the alignment pass found, and the two kg_proteins_align_paths entry points.
// Part of kmerguts_hip.hip's translation unit, behind kg_host_align.hpp.
#pragma once

static_assert(sizeof(kg_alignment_path) == 32 && sizeof(kg::TracePath) == 32 && sizeof(kg::TraceJob) == 24 && sizeof(kg_trace_stats) == 32,
              "record layouts of include/kmerguts_hip.h");

namespace {

constexpr uint32_t kTraceGrid = 256 * 18;               // workgroups of one wave, as kAlignGrid: the LDS is align_pairs_kernel's
constexpr uint32_t kTraceLongGrid = 1024;               // ... of the large-box launch at most
constexpr uint64_t kTraceShortSlabBytes = 512ull << 10; // a box whose direction words fit this goes to the wide launch
constexpr uint64_t kTraceSlabBytes = 2048ull << 20;     // direction words and carries of one launch in all (the launches share them)

struct TraceTotals { int64_t traced = 0, untraced = 0, cells = 0; float ms = 0; };

// what the alignment pass found for a pair, and whether the pair asks for a path
struct TraceEnd { int score, end_a, end_b; bool want; };

// Pairs (a, b) with their ends -> one TracePath per pair in the call's scratch, in pair order.  A pair is traced iff it asks,
// its score is >= 1 and its box has at most max_trace_cells cells.  The pairs are handed out in descending order of their box
// cells; a box whose columns do not fit the LDS carry or whose direction words exceed kTraceShortSlabBytes goes to the second
// launch, whose few workgroups own large slabs, so that one large pair does not narrow the launch of the small ones.
int trace_run(kg_table *t, Scratch &sc, const kg_align_params *prm, const uint8_t *d_seq, const int64_t *d_off, const int32_t *h_pairs,
              const std::vector<TraceEnd> &ends, uint64_t n_pairs, int64_t max_trace_cells, kg::TracePath **d_out, TraceTotals *tot)
{
    hipStream_t s = t->stream;
    int rc;
    Events<2> ev;
    if ((rc = ev.create())) return rc;
    std::vector<uint32_t> order[2];                     // [1]: the large boxes
    std::vector<uint64_t> cells(n_pairs);
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
    const uint32_t short_grid =
        (uint32_t)std::min<uint64_t>({n_short, (uint64_t)kTraceGrid, std::max<uint64_t>(1, kTraceSlabBytes / std::max<uint64_t>(words[0] * 4, 1))});
    const uint32_t long_grid = (uint32_t)std::min<uint64_t>(
        {n_long, (uint64_t)kTraceLongGrid, std::max<uint64_t>(1, kTraceSlabBytes / std::max<uint64_t>(words[1] * 4 + carry_cols * 8, 1))});

    kg::TraceJob *d_jobs = nullptr;
    uint32_t *d_dirs = nullptr;
    unsigned int *d_words = nullptr;                    // the two hand-out counters and the error bits
    int8_t *d_matrix = nullptr;
    int2 *d_carry = nullptr;
    if ((rc = sc.get(&d_jobs, std::max<uint64_t>(n_pairs, 1))) || (rc = sc.get(&d_words, kg::kTraceWords + 1)) ||
        (rc = sc.get(d_out, std::max<uint64_t>(n_pairs, 1))) ||
        (rc = sc.get(&d_dirs, std::max<uint64_t>({(uint64_t)short_grid * words[0], (uint64_t)long_grid * words[1], 1}))))
        return rc;
    if (prm->matrix && (rc = sc.get(&d_matrix, 21 * 21))) return rc;
    if (n_long && (rc = sc.get(&d_carry, (size_t)long_grid * carry_cols))) return rc;
    HIP_TRY(hipEventRecord(ev[0], s));
    HIP_TRY(hipMemsetAsync(d_words, 0, (kg::kTraceWords + 1) * 4, s));
    if (n_pairs) HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), n_pairs * sizeof(kg::TraceJob), hipMemcpyHostToDevice, s));
    if (d_matrix) HIP_TRY(hipMemcpyAsync(d_matrix, prm->matrix, 21 * 21, hipMemcpyHostToDevice, s));
    const int open = std::min(prm->gap_open, kg::kAlignGapCap), ext = std::min(prm->gap_extend, kg::kAlignGapCap);
    // (one stream: the second launch starts behind the first, so the two share the direction words)
    if (n_short)
        hipLaunchKernelGGL(kg::trace_pairs_kernel<false>, dim3(short_grid), dim3(kg::kWave), 0, s, d_seq, d_off, d_jobs, (uint32_t)n_short,
                           d_words, d_matrix, open, ext, max_trace_cells, d_dirs, words[0], nullptr, (uint64_t)0, *d_out);
    if (n_long)
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
    return KG_OK;
}

// what kg_proteins_align_paths does behind align_run: every aligned pair asks for a path
int align_paths_behind(kg_table *t, Scratch &sc, const kg_align_params *prm, const uint8_t *d_seq, const int64_t *d_off, const int32_t *pairs,
                       int64_t n_pairs, const kg_alignment *aln, const AlignPathsAsk *ask)
{
    std::vector<TraceEnd> ends((size_t)n_pairs);
    for (int64_t k = 0; k < n_pairs; k++) ends[(size_t)k] = TraceEnd{aln[k].score, aln[k].end_a, aln[k].end_b, aln[k].status == 0};
    kg::TracePath *d_paths = nullptr;
    TraceTotals tot;
    if (int rc = trace_run(t, sc, prm, d_seq, d_off, pairs, ends, (uint64_t)n_pairs, ask->max_trace_cells, &d_paths, &tot)) return rc;
    HIP_TRY(hipMemcpy(ask->paths, d_paths, (size_t)n_pairs * sizeof(kg_alignment_path), hipMemcpyDeviceToHost));
    return KG_OK;
}

}  // namespace

extern "C" {

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

}  // extern "C"
