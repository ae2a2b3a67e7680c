// kg_host_residual.hpp -- kg_contigs_search_residual / kg_result_search_residual: the fragments a list of signature CALLs does not
// explain searched against a resident protein database, and the two kinds of CALL merged (kernels: kg_residual.hpp).  A driver
// like kg_contigs_search_translated (kg_host_evidence.hpp), with two stages of its own around that call's three: kg_orfs_free
// gives the fragments; residual_choose marks, chooses and compacts the searched ones into a second ORF set in the fragments'
// context; searchdb_search_entry takes that set's residues where they lie (it is not entered when there are none);
// evidence_calls flags, sums and emits over these hit records; residual_merge cuts by min_db_count and merges.
// Nothing new is kept in the index handle: every block of the new stages comes out of the fragments' context.
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_evidence.hpp.
#pragma once

static_assert(sizeof(kg_residual_params) == 16 && sizeof(kg_residual_stats) == 80 && offsetof(kg_residual_params, min_db_count) == 8 &&
              offsetof(kg_residual_stats, ms_explain) == 64, "record layouts of include/kmerguts_hip.h");
static_assert(kg::kResidualWords <= kPinStageWords, "stage words must fit their pinned words");

namespace {

int check_residual_params(const kg_residual_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_residual_params");
    if (p->explain_min < 1) return fail(KG_ERR_ARG, "explain_min must be >= 1");
    if (p->min_db_count < 0) return fail(KG_ERR_ARG, "min_db_count must be >= 0");
    if (p->reserved != 0) return fail(KG_ERR_ARG, "kg_residual_params.reserved must be 0");
    return KG_OK;
}

// a block of the evidence goes back to its context's cache (only while the context's stream is idle)
template <typename T>
void evidence_drop(kg_evidence *e, T *&p)
{
    if (!p) return;
    e->blocks.erase(std::find(e->blocks.begin(), e->blocks.end(), (void *)p));
    dfree(e->tab, p);
    p = nullptr;
}

// The signature list of a call: sig[n] in host memory (on_device = 0: copied into a block of the evidence) or in device memory.
struct ResidualCalls { const kg_call *sig; int on_device; uint64_t n; };

// Mark, choose and compact, in the fragments' context t (held by the caller): fills e->searched, d_searched, d_explain and the
// counts and two times of e->rst; *d_sig: the signature CALLs on the device.  offsets: the contigs', host, checked.  room: the
// residues the handle's query room takes.
int residual_choose(kg_table *t, kg_evidence *e, const ResidualCalls &in, const int64_t *offsets, uint64_t n_seqs,
                    const kg_residual_params *rp, int64_t room, const kg_call **d_sig)
{
    Scratch sc(t);
    hipStream_t s = t->stream;
    const kg_orfset *frags = e->frags;
    const uint64_t n = (uint64_t)frags->count, n1 = std::max<uint64_t>(n, 1);
    int rc;
    Events<3> ev;
    if ((rc = ev.create())) return rc;
    unsigned long long *words = nullptr, *explain = nullptr;
    int64_t *d_off = nullptr;
    uint64_t *key = nullptr, *partial = nullptr;
    int32_t *first = nullptr;
    uint32_t *flag = nullptr, *len = nullptr, *qidx = nullptr, *excl = nullptr;
    if ((rc = sc.get(&words, kg::kResidualWords)) || (rc = sc.get(&d_off, n_seqs + 1)) || (rc = sc.get(&key, n1)) || (rc = sc.get(&first, n1)) ||
        (rc = sc.get(&explain, n1)) || (rc = sc.get(&flag, n1)) || (rc = sc.get(&len, n1)) || (rc = sc.get(&qidx, n1)) ||
        (rc = sc.get(&excl, n1)) || (rc = sc.get(&partial, n / kg::kScanChunk + 2)))
        return rc;
    *d_sig = in.sig;
    if (in.on_device) {
        if (in.n) HIP_TRY(hipDeviceSynchronize());          // the list is complete, whichever stream wrote it
    } else {
        kg_call *copy = nullptr;
        if ((rc = sc.get(&copy, std::max<uint64_t>(in.n, 1)))) return rc;
        if (in.n) HIP_TRY(hipMemcpyAsync(copy, in.sig, in.n * sizeof(kg_call), hipMemcpyHostToDevice, s));
        *d_sig = e->d_sig = e->keep(sc, copy);
    }
    HIP_TRY(hipMemsetAsync(words, 0x7F, kg::kResidualErrWords * 8, s));
    HIP_TRY(hipMemsetAsync(words + kg::kResidualErrWords, 0, (kg::kResidualWords - kg::kResidualErrWords) * 8, s));
    HIP_TRY(hipMemcpyAsync(d_off, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(ev[0], s));
    if (n) hipLaunchKernelGGL(kg::residual_keys_kernel, dim3(grid_of(n)), dim3(256), 0, s, frags->d_orfs, n, d_off, (uint32_t)n_seqs, key, first, explain);
    if (in.n)
        hipLaunchKernelGGL(kg::residual_mark_kernel, dim3(grid_of(in.n)), dim3(256), 0, s, *d_sig, in.n, d_off, n_seqs, key, first, n, explain, words);
    if (n) {
        hipLaunchKernelGGL(kg::residual_choose_kernel, dim3(grid_of(n)), dim3(256), 0, s, explain, frags->d_orfs, n, rp->explain_min, flag, len);
        HIP_TRY(hipGetLastError());
        // the fragments' residues are below 2^32 (kg_orfs_free), so the second sum's 32-bit prefix is exact
        if ((rc = prefix_sum(t, flag, n, qidx, partial, (uint64_t *)(words + kg::kResidualQueries))) ||
            (rc = prefix_sum(t, len, n, excl, partial, (uint64_t *)(words + kg::kResidualResidues))))
            return rc;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], s));
    // the one wait of the stage: the list's errors, the queries and their residues
    if ((rc = read_error_words(t, words, kg::kResidualWords, kPinStage,          // (in the order they are reported)
                               {{kg::kResidualErrOrder, KG_ERR_ARG, "CALL ", ": container below its predecessor's (calls[] must be in container order)"},
                                {kg::kResidualErrContainer, KG_ERR_ARG, "CALL ", ": container >= 6 * n_seqs"},
                                {kg::kResidualErrCount, KG_ERR_ARG, "CALL ", ": negative count"},
                                {kg::kResidualErrEnds, KG_ERR_ARG, "CALL ", ": start > end"},
                                {kg::kResidualErrRange, KG_ERR_ARG, "CALL ", ": outside its contig (0 <= x0 <= x1 <= L - 1 does not hold)"}})))
        return rc;
    const uint64_t n_q = t->h_pin[kPinStage + kg::kResidualQueries], n_res = t->h_pin[kPinStage + kg::kResidualResidues];
    if (n_q > n || n_res > (uint64_t)frags->residues) return fail(KG_ERR_DEVICE, "internal: more searched fragments or residues than there are");
    if ((int64_t)n_res > room)
        return fail(KG_ERR_LIMIT, kmer_text((int64_t)n_res) + " residues of queries do not fit the room of " + kmer_text(room) +
                                      " residues; kg_searchdb_reserve regrows it");
    kg_orf *out = nullptr;
    int64_t *new_start = nullptr, *searched = nullptr;
    uint8_t *res = nullptr;
    if ((rc = sc.get(&out, std::max<uint64_t>(n_q, 1))) || (rc = sc.get(&new_start, n_q + 1)) || (rc = sc.get(&searched, std::max<uint64_t>(n_q, 1))) ||
        (rc = sc.get(&res, std::max<uint64_t>(n_res, 1))))
        return rc;
    std::unique_ptr<kg_orfset> set(new (std::nothrow) kg_orfset());
    if (!set) return fail(KG_ERR_NOMEM, "out of host memory");
    hipLaunchKernelGGL(kg::residual_layout_kernel, dim3(grid_of(n + 1)), dim3(256), 0, s, frags->d_orfs, flag, qidx, excl,
                       (const uint64_t *)(words + kg::kResidualQueries), n, out, new_start, searched);
    if (n_res)
        hipLaunchKernelGGL(kg::residual_copy_kernel, dim3(grid_of((n_res + kg::kResidualChunk - 1) / kg::kResidualChunk)), dim3(256), 0, s,
                           frags->d_res, (uint64_t)frags->residues, frags->d_prot_start, n, searched, new_start, n_q, n_res, res);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[2], s));
    HIP_TRY(hipStreamSynchronize(s));
    set->tab = t;                       // (not owned: the fragments' set closes the context)
    keep_orfs(set.get(), sc, out, new_start, res, n_q, n_res, n_seqs);
    set->l_max = frags->l_max;
    set->st.orfs = (int64_t)n_q;
    set->st.residues = (int64_t)n_res;
    e->searched = set.release();
    e->d_searched = e->keep(sc, searched);
    e->d_explain = (int64_t *)e->keep(sc, explain);
    kg_residual_stats &st = e->rst;
    st.sig_calls = (int64_t)in.n;
    st.searched = (int64_t)n_q;
    st.searched_residues = (int64_t)n_res;
    st.explained = (int64_t)(n - n_q);
    st.explained_residues = frags->residues - (int64_t)n_res;
    st.ms_explain = ev.ms(0, 1);
    st.ms_compact = ev.ms(1, 2);
    return KG_OK;
}

// The hit set of zero queries, as a search would shape it, without a search: its blocks come out of the context t
int residual_no_hits(kg_table *t, const kg_searchdb *db, int trace, const kg_mask_params *query_mask, const kg_ungapped_params *ung,
                     const kg_band_params *band, kg_hitset **out)
{
    std::unique_ptr<kg_hitset> set(new (std::nothrow) kg_hitset());
    if (!set) return fail(KG_ERR_NOMEM, "out of host memory");
    set->device = t->device;
    int rc;
    if ((rc = dalloc_detached(t, &set->d_block.p, 8 + sizeof(kg_search_hit))) || (rc = dalloc_detached(t, &set->d_paths.p, sizeof(kg_alignment_path))))
        return rc;
    HIP_TRY(hipMemsetAsync(set->d_block.p, 0, 8, t->stream));       // hit_start = {0}
    set->has_paths = true;
    if (trace & (KG_TRACE_OPS | KG_TRACE_OPS_EQX)) {
        if ((rc = dalloc_detached(t, &set->d_ops.p, 8 + 4))) return rc;
        HIP_TRY(hipMemsetAsync(set->d_ops.p, 0, 8, t->stream));     // op_start = {0}
        set->has_ops = true;
    }
    if (db->has_mask || query_mask) {
        if (db->has_mask) set->mst = db->mst;
        set->mst.ms_mask = 0;
        set->has_mask = true;
    }
    if (ung) {
        if ((rc = dalloc_detached(t, &set->d_ung.p, sizeof(kg_search_ungapped)))) return rc;
        set->has_ung = true;
    }
    if (band) {
        set->bst.band = band->band;
        set->has_band = true;
    }
    set->st.targets = db->n_db;
    set->has_db = true;
    HIP_TRY(hipStreamSynchronize(t->stream));
    *out = set.release();
    return KG_OK;
}

// The min_db_count cut and the merge, in the fragments' context t (held by the caller, idle): e->d_calls / d_call_hit, the
// homology CALLs of evidence_calls, give way to the merged arrays.
int residual_merge(kg_table *t, kg_evidence *e, const kg_call *d_sig, uint64_t n_sig, const kg_residual_params *rp)
{
    Scratch sc(t);
    hipStream_t s = t->stream;
    const uint64_t n_db = (uint64_t)e->n_calls, n_all = n_sig + n_db;
    int rc;
    if (n_all >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more CALL records in one call");
    Events<2> ev;
    if ((rc = ev.create())) return rc;
    uint64_t *words = nullptr, *partial = nullptr;
    uint32_t *keep = nullptr, *kpos = nullptr;
    kg_call *out = nullptr;
    uint8_t *kind = nullptr;
    int64_t *source = nullptr, *hit = nullptr;
    const uint64_t n1 = std::max<uint64_t>(n_all, 1);
    if ((rc = sc.get(&words, 1)) || (rc = sc.get(&keep, std::max<uint64_t>(n_db, 1))) || (rc = sc.get(&kpos, std::max<uint64_t>(n_db, 1))) ||
        (rc = sc.get(&partial, n_db / kg::kScanChunk + 2)) || (rc = sc.get(&out, n1)) || (rc = sc.get(&kind, n1)) || (rc = sc.get(&source, n1)) ||
        (rc = sc.get(&hit, n1)))
        return rc;
    HIP_TRY(hipMemsetAsync(words, 0, 8, s));
    HIP_TRY(hipEventRecord(ev[0], s));
    if (n_db) {
        hipLaunchKernelGGL(kg::residual_keep_kernel, dim3(grid_of(n_db)), dim3(256), 0, s, e->d_calls, n_db, rp->min_db_count, keep);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, keep, n_db, kpos, partial, words))) return rc;
    }
    if (n_all) {
        hipLaunchKernelGGL(kg::residual_merge_kernel, dim3(grid_of(n_all)), dim3(256), 0, s, d_sig, n_sig, e->d_calls, n_db, keep, kpos, words,
                           e->d_call_hit, out, kind, source, hit);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[1], s));
    if ((rc = read_error_words(t, words, 1, kPinStage, {}))) return rc;
    const uint64_t n_kept = t->h_pin[kPinStage];
    if (n_kept > n_db) return fail(KG_ERR_DEVICE, "internal: more kept homology CALLs than there are");
    evidence_drop(e, e->d_calls);
    evidence_drop(e, e->d_call_hit);
    evidence_drop(e, e->d_sig);
    e->d_calls = e->keep(sc, out);
    e->d_call_hit = e->keep(sc, hit);
    e->d_call_kind = e->keep(sc, kind);
    e->d_call_source = e->keep(sc, source);
    e->n_calls = (int64_t)(n_sig + n_kept);
    kg_residual_stats &st = e->rst;
    st.db_calls = (int64_t)n_db;
    st.dropped_min_count = (int64_t)(n_db - n_kept);
    st.merged = e->n_calls;
    st.ms_merge = ev.ms(0, 1);
    st.ms_total = e->st.ms_total + st.ms_explain + st.ms_compact + st.ms_merge;
    return KG_OK;
}

int residual_entry(kg_searchdb *db, const kg_search_params *p, const kg_align_params *align, const kg_translate_params *tp, const uint8_t *seq,
                   int seq_on_device, const int64_t *offsets, int64_t n_seqs, int64_t max_windows, int64_t max_pairs, int trace,
                   int64_t max_trace_cells, const kg_mask_params *query_mask, const kg_ungapped_params *ungapped, const kg_band_params *band,
                   const int32_t *target_fn, const kg_call *sig, int calls_on_device, int64_t n_sig, const kg_residual_params *rp, kg_evidence **out)
{
    if ((trace & 3) == 0) trace |= KG_TRACE_HITS;       // a CALL needs the path's start
    MaskPlan qplan;
    int rc = searchdb_check_ask(db, p, align, max_windows, max_pairs, SearchPathsAsk{trace, max_trace_cells}, query_mask, ungapped, band, &qplan);
    if (rc || (rc = check_translate_params(tp)) || (rc = check_residual_params(rp))) return rc;
    if (!target_fn) return fail(KG_ERR_ARG, "null target_fn: the two kinds of CALL need one function index space");
    for (int64_t d = 0; d < db->n_db; d++)
        if (target_fn[d] < 0) return fail(KG_ERR_ARG, "target_fn[" + kmer_text(d) + "] < 0");
    if (n_seqs >= (1ll << 32) / 6) return fail(KG_ERR_LIMIT, "so many contigs that a container index 6 * seq + 5 reaches 2^32");
    if (n_sig < 0) return fail(KG_ERR_ARG, "n_calls < 0");
    if ((uint64_t)n_sig >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more CALL records in one call");
    if (n_sig && !sig) return fail(KG_ERR_ARG, "null CALL records");
    if (n_sig && n_seqs == 0) return fail(KG_ERR_ARG, "CALL 0: container >= 6 * n_seqs");
    EvidenceGuard g;
    // ---- the fragments: every stop-to-stop run of the six frames, in a context of their own ----
    kg_orfset *frags = nullptr;
    const kg_free_params fp = {tp->min_res, 0, 0};
    if ((rc = kg_orfs_free(db->t->device, &fp, seq, seq_on_device, offsets, n_seqs, &frags))) return rc;
    g.e = new (std::nothrow) kg_evidence();
    if (!g.e) { kg_orfset_free(frags); return fail(KG_ERR_NOMEM, "out of host memory"); }
    kg_evidence *e = g.e;
    e->frags = frags;
    e->tab = frags->tab;
    e->residual = true;
    // ---- explained or searched: the searched fragments become an ORF set of their own ----
    const kg_call *d_sig = nullptr;
    {
        CallScope cs(frags->tab, "a call is in flight on the fragments' context");
        if (cs.rc) return cs.rc;
        if ((rc = residual_choose(cs.t, e, ResidualCalls{sig, calls_on_device, (uint64_t)n_sig}, offsets, (uint64_t)n_seqs, rp, db->room, &d_sig)))
            return rc;
        cs.t->cache.release_free();
    }
    // ---- the search: the searched fragments' residues go into the handle's room device to device ----
    const int64_t n_q = e->searched->count;
    if (n_q) {
        std::vector<int64_t> h_start((size_t)n_q + 1, 0);
        HIP_TRY(hipMemcpy(h_start.data(), e->searched->d_prot_start, ((size_t)n_q + 1) * 8, hipMemcpyDeviceToHost));
        if ((rc = searchdb_search_entry(db, p, align, nullptr, e->searched->d_res, h_start.data(), n_q, max_windows, max_pairs, trace, max_trace_cells,
                                        query_mask, ungapped, band, &e->hits)))
            return rc;
    } else {
        CallScope held(db->t, kSearchDbBusy);            // nothing is launched on the handle, but a call in flight on it is still an error
        if (held.rc) return held.rc;
    }
    // ---- the homology CALLs, the cut and the merge ----
    {
        CallScope cs(frags->tab, "a call is in flight on the fragments' context");
        if (cs.rc) return cs.rc;
        if (!n_q && (rc = residual_no_hits(cs.t, db, trace, query_mask, ungapped, band, &e->hits))) return rc;
        if ((rc = evidence_calls(cs.t, e, tp, offsets, (uint64_t)n_seqs, target_fn, (uint64_t)db->n_db, e->searched)) ||
            (rc = residual_merge(cs.t, e, d_sig, (uint64_t)n_sig, rp)))
            return rc;
        cs.t->cache.release_free();
    }
    if (getenv("KG_DEBUG"))
        fprintf(stderr, "[kg] kg_contigs_search_residual: fragments=%lld sig_calls=%lld explained=%lld searched=%lld searched_residues=%lld records=%lld "
                        "db_calls=%lld merged=%lld explain_ms=%.3f compact_ms=%.3f search_ms=%.3f merge_ms=%.3f\n",
                (long long)e->st.fragments, (long long)e->rst.sig_calls, (long long)e->rst.explained, (long long)e->rst.searched,
                (long long)e->rst.searched_residues, (long long)e->st.records, (long long)e->rst.db_calls, (long long)e->rst.merged,
                e->rst.ms_explain, e->rst.ms_compact, e->st.ms_search, e->rst.ms_merge);
    *out = g.release();
    return KG_OK;
}

const kg_evidence *residual_of(const kg_evidence *e, const char *what)
{
    if (!e) { fail(KG_ERR_ARG, "null argument"); return nullptr; }
    if (!e->residual) { fail(KG_ERR_ARG, std::string(what) + ": the evidence was made without signature CALLs"); return nullptr; }
    return e;
}

}  // namespace

extern "C" {

int kg_contigs_search_residual(kg_searchdb *db, const kg_search_params *p, const kg_align_params *align, const kg_translate_params *tp,
                               const uint8_t *seq, int seq_on_device, const int64_t *offsets, int64_t n_seqs, int64_t max_windows,
                               int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *query_mask,
                               const kg_ungapped_params *ungapped, const kg_band_params *band, const int32_t *target_fn, const kg_call *sig_calls,
                               int calls_on_device, int64_t n_sig_calls, const kg_residual_params *rp, kg_evidence **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    return residual_entry(db, p, align, tp, seq, seq_on_device, offsets, n_seqs, max_windows, max_pairs, trace, max_trace_cells, query_mask, ungapped,
                          band, target_fn, sig_calls, calls_on_device, n_sig_calls, rp, out);
}

int kg_result_search_residual(kg_result *r, kg_searchdb *db, const kg_search_params *p, const kg_align_params *align, const kg_translate_params *tp,
                              const uint8_t *seq, int seq_on_device, const int64_t *offsets, int64_t n_seqs, int64_t max_windows,
                              int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *query_mask,
                              const kg_ungapped_params *ungapped, const kg_band_params *band, const int32_t *target_fn,
                              const kg_residual_params *rp, kg_evidence **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!r) return fail(KG_ERR_ARG, "null kg_result");
    if (!db) return fail(KG_ERR_ARG, "null kg_searchdb");
    if (!r->d_ccs) return fail(KG_ERR_ARG, "a KG_F_SKIP_AGGREGATE result has no CALL records to explain fragments with");
    if (r->per != 6) return fail(KG_ERR_ARG, "a protein (-a) result: fragments need a DNA scan, six containers per sequence");
    if (r->tab->device != db->t->device) return fail(KG_ERR_ARG, "the result lies on another device than the kg_searchdb");
    if (r->st.n_seqs != n_seqs) return fail(KG_ERR_ARG, "n_seqs is not the result's number of sequences");
    CallScope held(r->tab, "a kg_scan* is in flight on this result's kg_table");
    if (held.rc) return held.rc;
    return residual_entry(db, p, align, tp, seq, seq_on_device, offsets, n_seqs, max_windows, max_pairs, trace, max_trace_cells, query_mask, ungapped,
                          band, target_fn, r->d_calls, 1, r->st.n_calls, rp, out);
}

const kg_orfset *kg_residual_searched_fragments(const kg_evidence *e)
{
    const kg_evidence *re = residual_of(e, "kg_residual_searched_fragments");
    return re ? re->searched : nullptr;
}

int kg_residual_searched_copy(const kg_evidence *e, int64_t first, int64_t count, int64_t *dst)
{
    if (!residual_of(e, "kg_residual_searched_copy")) return KG_ERR_ARG;
    return copy_records(e, device_of(e), e->d_searched, 1, e->searched->count, first, count, dst, "kg_residual_searched_copy");
}

int kg_residual_explain_copy(const kg_evidence *e, int64_t first, int64_t count, int64_t *dst)
{
    if (!residual_of(e, "kg_residual_explain_copy")) return KG_ERR_ARG;
    return copy_records(e, device_of(e), e->d_explain, 1, e->frags->count, first, count, dst, "kg_residual_explain_copy");
}

int kg_residual_call_kinds_copy(const kg_evidence *e, int64_t first, int64_t count, uint8_t *dst)
{
    if (!residual_of(e, "kg_residual_call_kinds_copy")) return KG_ERR_ARG;
    return copy_records(e, device_of(e), e->d_call_kind, 1, e->n_calls, first, count, dst, "kg_residual_call_kinds_copy");
}

int kg_residual_call_sources_copy(const kg_evidence *e, int64_t first, int64_t count, int64_t *dst)
{
    if (!residual_of(e, "kg_residual_call_sources_copy")) return KG_ERR_ARG;
    return copy_records(e, device_of(e), e->d_call_source, 1, e->n_calls, first, count, dst, "kg_residual_call_sources_copy");
}

int kg_residual_stats_of(const kg_evidence *e, kg_residual_stats *out)
{
    if (!residual_of(e, "kg_residual_stats_of")) return KG_ERR_ARG;
    return copy_stats(e, &e->rst, out);
}

}  // extern "C"
