// kg_host_evidence.hpp -- kg_contigs_search_translated: the stop-to-stop fragments of a batch of contigs searched against a
// resident protein database, and the hits made into CALL records (kernels: kg_evidence.hpp).  The call is a driver over two
// calls that exist and one stage that is new: kg_orfs_free with start_codons = 0 (kg_host_orfs.hpp) gives the fragments as an ORF
// set in a context of its own; searchdb_search_entry (kg_host_searchdb.hpp) takes that set's residues where they lie on the
// device, with prot_start brought to the host for its offsets; evidence_calls flags, sums and emits over the hit records.
// The kg_evidence a call hands out owns the ORF set and the hit set and lends them; its own two arrays, the CALLs and call_hit,
// are blocks of the ORF set's context, so they are given back before that set is freed.  kg_contigs_search_residual
// (kg_host_residual.hpp) hands out the same kg_evidence with a second ORF set, the searched fragments, between the two.
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_searchdb.hpp and kg_host_orfs.hpp.
#pragma once

struct kg_evidence : SetBase {
    kg_orfset *frags = nullptr;         // owned: the fragments, an ordinary ORF set (its context is `tab`)
    kg_hitset *hits = nullptr;          // owned: the hit records, an ordinary hit set
    kg_call *d_calls = nullptr;         // n_calls records (a block of one record when there are none)
    int64_t *d_call_hit = nullptr;      // n_calls
    int64_t n_calls = 0;
    kg_translate_stats st = {};
    // kg_contigs_search_residual (kg_host_residual.hpp): the hits are those of `searched`, the CALLs the merged list
    bool residual = false;
    kg_orfset *searched = nullptr;      // owned: the fragments that were searched, an ORF set in the fragments' context
    int64_t *d_searched = nullptr;      // searched->count: every query's index among the fragments
    int64_t *d_explain = nullptr;       // frags->count
    uint8_t *d_call_kind = nullptr;     // n_calls
    int64_t *d_call_source = nullptr;   // n_calls
    kg_call *d_sig = nullptr;           // the call's own device copy of a host list of signature CALLs, until the merge
    kg_residual_stats rst = {};
};

static_assert(sizeof(kg_translate_params) == 16 && sizeof(kg_translate_stats) == 72, "record layouts of include/kmerguts_hip.h");
static_assert(kg::kEvidenceWords <= kPinStageWords, "stage words must fit their pinned words");

namespace {

// the evidence's own blocks first (into the context's cache), then the two sets; the ORF set closes the context
void evidence_delete(kg_evidence *e)
{
    if (!e) return;
    kg_orfset *frags = e->frags, *searched = e->searched;
    kg_hitset *hits = e->hits;
    delete e;
    kg_hitset_free(hits);
    kg_orfset_free(searched);
    kg_orfset_free(frags);
}

// a failed call gives up what it has made and keeps its error text
struct EvidenceGuard {
    kg_evidence *e = nullptr;
    ~EvidenceGuard()
    {
        if (!e) return;
        std::string keep = g_err;
        evidence_delete(e);
        g_err = keep;
    }
    kg_evidence *release() { kg_evidence *out = e; e = nullptr; return out; }
};

int check_translate_params(const kg_translate_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_translate_params");
    if (p->min_res < 1) return fail(KG_ERR_ARG, "min_res must be >= 1");
    if (p->max_hits < 1 || p->max_hits > kg::kSearchMaxCand) return fail(KG_ERR_ARG, "max_hits must be in 1..64");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(KG_ERR_ARG, "kg_translate_params.reserved must be 0");
    return KG_OK;
}

// The CALLs of e->hits over e->frags, in the ORF set's context t (held by the caller): flag, the shared prefix sum, emit.
// offsets: the contigs', host, checked; target_fn: host int32[n_db] or null, checked.  queries: the ORF set whose proteins were
// searched, e->frags or a subset of it in the same context (kg_host_residual.hpp); the statistics count e->frags either way.
int evidence_calls(kg_table *t, kg_evidence *e, const kg_translate_params *prm, const int64_t *offsets, uint64_t n_seqs,
                   const int32_t *target_fn, uint64_t n_db, const kg_orfset *queries)
{
    Scratch sc(t);
    hipStream_t s = t->stream;
    const kg_hitset *hs = e->hits;
    const uint64_t n = (uint64_t)hs->count, n_frags = (uint64_t)queries->count;
    int rc;
    if (n >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more hit records in one call");
    if (n && (!hs->has_paths || n_frags == 0 || n_seqs == 0 || n_db == 0))
        return fail(KG_ERR_DEVICE, "internal: hit records without paths, fragments, contigs or targets");
    unsigned long long *words = nullptr;
    uint32_t *keep = nullptr, *pos = nullptr;
    uint64_t *partial = nullptr;
    int64_t *d_off = nullptr;
    int32_t *d_fn = nullptr;
    if ((rc = sc.get(&words, kg::kEvidenceWords)) || (rc = sc.get(&keep, std::max<uint64_t>(n, 1))) || (rc = sc.get(&pos, std::max<uint64_t>(n, 1))) ||
        (rc = sc.get(&partial, n / kg::kScanChunk + 2)) || (rc = sc.get(&d_off, n_seqs + 1)))
        return rc;
    if (target_fn && n_db && (rc = sc.get(&d_fn, n_db))) return rc;
    HIP_TRY(hipMemsetAsync(words, 0, kg::kEvidenceWords * 8, s));
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_off, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, s));
        if (d_fn) HIP_TRY(hipMemcpyAsync(d_fn, target_fn, n_db * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipEventRecord(t->ev[kEvStageBegin], s));
    const kg_search_hit *d_hits = hs->hits();
    const kg_alignment_path *d_paths = (const kg_alignment_path *)hs->d_paths.p;
    if (n) {
        hipLaunchKernelGGL(kg::evidence_flag_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_hits, d_paths, n, prm->max_hits, keep, words);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, keep, n, pos, partial, (uint64_t *)(words + kg::kEvidenceCalls)))) return rc;
    }
    // the one wait of the stage: how many CALLs there are, and the drop counts with them
    if ((rc = read_error_words(t, words, kg::kEvidenceWords, kPinStage, {}))) return rc;
    const uint64_t *h = t->h_pin + kPinStage;
    const uint64_t n_calls = h[kg::kEvidenceCalls];
    if (n_calls > n || n_calls + h[kg::kEvidenceDropStatus] + h[kg::kEvidenceDropRank] + h[kg::kEvidenceDropUntraced] != n)
        return fail(KG_ERR_DEVICE, "internal: the CALLs and the dropped records do not add up to the hit records");
    kg_call *d_calls = nullptr;
    int64_t *d_call_hit = nullptr;
    if ((rc = sc.get(&d_calls, std::max<uint64_t>(n_calls, 1))) || (rc = sc.get(&d_call_hit, std::max<uint64_t>(n_calls, 1)))) return rc;
    if (n_calls) {
        hipLaunchKernelGGL(kg::evidence_emit_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_hits, d_paths, n, keep, pos, queries->d_orfs,
                           (uint32_t)n_frags, d_off, (uint32_t)n_seqs, d_fn, (uint32_t)n_db, d_calls, d_call_hit);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(t->ev[kEvStageEnd], s));
    HIP_TRY(hipStreamSynchronize(s));
    kg_translate_stats &st = e->st;
    st.fragments = e->frags->count;
    st.fragment_residues = e->frags->residues;
    st.records = (int64_t)n;
    st.calls = (int64_t)n_calls;
    st.dropped_status = (int64_t)h[kg::kEvidenceDropStatus];
    st.dropped_rank = (int64_t)h[kg::kEvidenceDropRank];
    st.dropped_untraced = (int64_t)h[kg::kEvidenceDropUntraced];
    HIP_TRY(hipEventElapsedTime(&st.ms_calls, t->ev[kEvStageBegin], t->ev[kEvStageEnd]));
    st.ms_fragments = e->frags->st.ms;
    st.ms_search = hs->st.ms_total + hs->tst.ms_trace;
    st.ms_total = st.ms_fragments + st.ms_search + st.ms_calls;
    e->d_calls = e->keep(sc, d_calls);
    e->d_call_hit = e->keep(sc, d_call_hit);
    e->n_calls = (int64_t)n_calls;
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_contigs_search_translated(kg_searchdb *db, const kg_search_params *p, const kg_align_params *align, const kg_translate_params *tp,
                                 const uint8_t *seq, int seq_on_device, const int64_t *offsets, int64_t n_seqs, int64_t max_windows,
                                 int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *query_mask,
                                 const kg_ungapped_params *ungapped, const kg_band_params *band, const int32_t *target_fn, kg_evidence **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if ((trace & 3) == 0) trace |= KG_TRACE_HITS;       // a CALL needs the path's start
    MaskPlan qplan;
    int rc = searchdb_check_ask(db, p, align, max_windows, max_pairs, SearchPathsAsk{trace, max_trace_cells}, query_mask, ungapped, band, &qplan);
    if (rc || (rc = check_translate_params(tp))) return rc;
    if (target_fn)
        for (int64_t d = 0; d < db->n_db; d++)
            if (target_fn[d] < 0) return fail(KG_ERR_ARG, "target_fn[" + kmer_text(d) + "] < 0");
    if (n_seqs >= (1ll << 32) / 6) return fail(KG_ERR_LIMIT, "so many contigs that a container index 6 * seq + 5 reaches 2^32");
    EvidenceGuard g;
    // ---- the fragments: every stop-to-stop run of the six frames, in a context of their own ----
    kg_orfset *frags = nullptr;
    const kg_free_params fp = {tp->min_res, 0, 0};
    if ((rc = kg_orfs_free(db->t->device, &fp, seq, seq_on_device, offsets, n_seqs, &frags))) return rc;
    g.e = new (std::nothrow) kg_evidence();
    if (!g.e) { kg_orfset_free(frags); return fail(KG_ERR_NOMEM, "out of host memory"); }
    g.e->frags = frags;
    g.e->tab = frags->tab;
    const int64_t n_frags = frags->count;
    std::vector<int64_t> h_start((size_t)n_frags + 1, 0);
    HIP_TRY(hipMemcpy(h_start.data(), frags->d_prot_start, ((size_t)n_frags + 1) * 8, hipMemcpyDeviceToHost));
    // ---- the search: the fragments' residues go into the handle's room device to device ----
    if ((rc = searchdb_search_entry(db, p, align, nullptr, frags->d_res, h_start.data(), n_frags, max_windows, max_pairs, trace, max_trace_cells,
                                    query_mask, ungapped, band, &g.e->hits)))
        return rc;
    // ---- the CALLs ----
    {
        CallScope cs(frags->tab, "a call is in flight on the fragments' context");
        if (cs.rc) return cs.rc;
        if ((rc = evidence_calls(cs.t, g.e, tp, offsets, (uint64_t)n_seqs, target_fn, (uint64_t)db->n_db, frags))) return rc;
        cs.t->cache.release_free();                     // the stage's scratch goes back to the driver, the two arrays stay
    }
    if (getenv("KG_DEBUG"))
        fprintf(stderr, "[kg] kg_contigs_search_translated: fragments=%lld residues=%lld records=%lld calls=%lld fragments_ms=%.3f search_ms=%.3f calls_ms=%.3f\n",
                (long long)g.e->st.fragments, (long long)g.e->st.fragment_residues, (long long)g.e->st.records, (long long)g.e->st.calls,
                g.e->st.ms_fragments, g.e->st.ms_search, g.e->st.ms_calls);
    *out = g.release();
    return KG_OK;
}

const kg_orfset *kg_evidence_fragments(const kg_evidence *e) { return e ? e->frags : nullptr; }

const kg_hitset *kg_evidence_hits(const kg_evidence *e) { return e ? e->hits : nullptr; }

int64_t kg_evidence_calls_count(const kg_evidence *e) { return e ? e->n_calls : 0; }

const kg_call *kg_evidence_calls_device(const kg_evidence *e) { return e ? e->d_calls : nullptr; }

int kg_evidence_calls_copy(const kg_evidence *e, int64_t first, int64_t count, kg_call *dst)
{
    return copy_records(e, device_of(e), e ? e->d_calls : nullptr, 1, e ? e->n_calls : 0, first, count, dst, "kg_evidence_calls_copy");
}

int kg_evidence_call_hits_copy(const kg_evidence *e, int64_t first, int64_t count, int64_t *dst)
{
    return copy_records(e, device_of(e), e ? e->d_call_hit : nullptr, 1, e ? e->n_calls : 0, first, count, dst, "kg_evidence_call_hits_copy");
}

int kg_evidence_stats(const kg_evidence *e, kg_translate_stats *out) { return copy_stats(e, e ? &e->st : nullptr, out); }

void kg_evidence_free(kg_evidence *e) { evidence_delete(e); }

}  // extern "C"
