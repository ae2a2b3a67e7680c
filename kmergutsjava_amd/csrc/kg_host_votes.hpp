// kg_host_votes.hpp -- kg_result_otu_votes / kg_otu_votes_hits: the hit, event and CALL records of a scan -> every OTU vote per
// sequence, one class record per sequence, the bins of the batch (kernels: kg_votes.hpp).
// Part of kmerguts_hip.hip's translation unit: one of the batch stages, included behind the kernel headers, kg_host.hpp and the
// hosts of the table, the result and the scan.
#pragma once

struct kg_voteset : SetBase {
    kg_otu_vote *d_votes = nullptr;     // count records, rule 3's order
    int64_t *d_seq_start = nullptr;     // n_seqs + 1
    kg_otu_class *d_classes = nullptr;  // n_seqs
    kg_otu_bin *d_bins = nullptr;       // n_bins, rule 5's order
    int64_t count = 0, n_seqs = 0, n_bins = 0;
    kg_vote_stats st = {};
};

namespace {

// the stage area of kg_table::h_pin: the error and counter words, then up to three totals
static_assert(kg::kVoteErrWords + kg::kVoteCntWords + 3 <= kPinStageWords, "stage words must fit their pinned words");
static_assert(kNoErr == kg::kVoteNoErr, "the stages' kernels share the error words' \"none\"");

int check_vote_params(const kg_vote_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_vote_params");
    if (p->min_votes < 0) return fail(KG_ERR_ARG, "min_votes must be >= 0");
    if (p->min_share_pct < 0 || p->min_share_pct > 100) return fail(KG_ERR_ARG, "min_share_pct must be in 0 .. 100");
    if (p->min_calls < 0) return fail(KG_ERR_ARG, "min_calls must be >= 0");
    if (p->reserved != 0) return fail(KG_ERR_ARG, "kg_vote_params.reserved must be 0");
    return KG_OK;
}

// the host checks of offsets[n_seqs + 1]
int check_vote_offsets(const int64_t *offsets, int64_t n_seqs)
{
    if (n_seqs < 0) return fail(KG_ERR_ARG, "n_seqs < 0");
    if (!offsets) return fail(KG_ERR_ARG, "null offsets");
    if (n_seqs >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more sequences in one call");
    for (int64_t k = 0; k < n_seqs; k++)
        if (offsets[k + 1] < offsets[k]) return fail(KG_ERR_ARG, "sequence " + kmer_text(k) + ": offsets decrease (offsets[s+1] < offsets[s])");
    return KG_OK;
}

// a caller-held start array: begins at 0 and never decreases
int check_vote_starts(const int64_t *start, int64_t n_cont, const char *name)
{
    if (start[0] != 0) return fail(KG_ERR_ARG, std::string(name) + "[0] must be 0");
    for (int64_t c = 0; c < n_cont; c++)
        if (start[c + 1] < start[c]) return fail(KG_ERR_ARG, "container " + kmer_text(c) + ": " + name + " decreases");
    return KG_OK;
}

// d_words + word .. (+ count) -> h_pin[kPinStage ..], waited for
int vote_read_back(kg_table *t, const unsigned long long *d_words, int word, int count)
{
    HIP_TRY(hipMemcpyAsync(t->h_pin + kPinStage, d_words + word, (size_t)count * 8, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return KG_OK;
}

// The device arrays are complete on t->stream; offsets: host, checked.  Fills set (its arrays come out of the cache with the
// call's scratch and are kept only on success).
int votes_impl(kg_table *t, const kg_vote_params *prm, const kg_hit *d_hits, const uint8_t *d_ev, uint64_t n, const int64_t *d_chs,
               const kg_call *d_calls, uint64_t n_calls, const int64_t *d_ccs, uint64_t n_seqs, uint32_t per, const int64_t *offsets,
               kg_voteset *set)
{
    Scratch sc(t);
    hipStream_t s = t->stream;
    int rc;
    const uint64_t n_cont = n_seqs * per;
    const uint64_t length_top = n_seqs ? (uint64_t)(offsets[n_seqs] - offsets[0]) : 0;
    int64_t *d_off = nullptr, *d_start = nullptr, *d_tally = nullptr;
    kg_otu_vote *d_votes = nullptr;
    kg_otu_class *d_cls = nullptr;
    kg_otu_bin *d_bins = nullptr;
    unsigned long long *words = nullptr;    // the error words, the counter words, then the totals of the prefix sums
    enum { kSumVotes = 0, kSumRuns = 1, kSumChanges = 2, kSumAssigned = 3, kSumBins = 4, kSumCount = 5 };
    constexpr int kWordsCnt = kg::kVoteErrWords, kWordsTot = kWordsCnt + kg::kVoteCntWords;
    if ((rc = sc.get(&d_off, n_seqs + 1)) || (rc = sc.get(&d_start, n_seqs + 1)) || (rc = sc.get(&d_tally, n_seqs + 1)) ||
        (rc = sc.get(&d_cls, std::max<uint64_t>(n_seqs, 1))) || (rc = sc.get(&words, kWordsTot + kSumCount)))
        return rc;
    unsigned long long *err = words, *cnt = words + kWordsCnt;
    uint64_t *totals = (uint64_t *)(words + kWordsTot);
    HIP_TRY(hipMemcpyAsync(d_off, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(err, 0x7F, kg::kVoteErrWords * 8, s));
    HIP_TRY(hipMemsetAsync(cnt, 0, (kg::kVoteCntWords + kSumCount) * 8, s));
    HIP_TRY(hipEventRecord(t->ev[kEvStageBegin], s));
    const uint64_t *h = t->h_pin + kPinStage;
    uint64_t n_votes = 0, n_runs = 0, n_assigned = 0, n_bins = 0;
    uint32_t oi_bits = 0, v_bits = 0;
    const uint64_t *tally_keys = nullptr, *order_keys = nullptr;
    uint64_t *partial = nullptr;
    if ((rc = sc.get(&partial, std::max(n, n_seqs) / kg::kScanChunk + 2))) return rc;
    if (n_calls > 0) {
        hipLaunchKernelGGL(kg::vote_calls_check_kernel, dim3(grid_of(n_calls)), dim3(kg::kVoteThreads), 0, s, d_calls, n_calls, d_ccs,
                           n_cont, err);
        HIP_TRY(hipGetLastError());
    }
    SortPairs tally;                    // (the first sort's keys live until the class kernel has run)
    if (n > 0) {
        uint32_t *flag = nullptr, *excl = nullptr, *cidx = nullptr;
        if ((rc = sc.get(&flag, n)) || (rc = sc.get(&excl, n)) || (rc = sc.get(&cidx, n))) return rc;
        hipLaunchKernelGGL(kg::vote_mark_kernel, dim3(grid_of(n)), dim3(kg::kVoteThreads), 0, s, d_hits, d_ev, n, d_chs, d_calls, n_calls,
                           d_ccs, n_cont, flag, cidx, err, cnt);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, flag, n, excl, partial, totals + kSumVotes))) return rc;
        if ((rc = vote_read_back(t, words, kWordsCnt, kg::kVoteCntWords + 1))) return rc;
        n_votes = h[kg::kVoteCntWords + kSumVotes];
        oi_bits = bit_width(h[kg::kVoteCntMaxOtu]);
        if (n_votes > 0) {
            if ((rc = tally.alloc(sc, n_votes))) return rc;
            hipLaunchKernelGGL(kg::vote_compact_kernel, dim3(grid_of(n)), dim3(kg::kVoteThreads), 0, s, d_hits, flag, excl, cidx, n, n_cont,
                               per, oi_bits, n_votes, tally.keys(), tally.vals());
            HIP_TRY(hipGetLastError());
            if ((rc = tally.sort(t, sc, n_votes, bits_for(n_seqs) + oi_bits))) return rc;
            tally_keys = tally.keys();
            // the hits' three arrays are free: the votes' run heads and CALL changes take them (n_votes <= n)
            uint32_t *head = flag, *chg = cidx, *hexcl = excl, *cexcl = nullptr;
            if ((rc = sc.get(&cexcl, n_votes))) return rc;
            hipLaunchKernelGGL(kg::vote_heads_kernel, dim3(grid_of(n_votes)), dim3(kg::kVoteThreads), 0, s, tally.keys(), tally.vals(),
                               n_votes, head, chg);
            HIP_TRY(hipGetLastError());
            if ((rc = prefix_sum(t, head, n_votes, hexcl, partial, totals + kSumRuns))) return rc;
            if ((rc = prefix_sum(t, chg, n_votes, cexcl, partial, totals + kSumChanges))) return rc;
            if ((rc = vote_read_back(t, words, kWordsTot + kSumRuns, 1))) return rc;
            n_runs = h[0];
            uint32_t *run_start = nullptr, *run_cc = nullptr;
            kg_otu_vote *unsorted = nullptr;
            SortPairs order;
            if ((rc = sc.get(&run_start, n_runs + 1)) || (rc = sc.get(&run_cc, n_runs + 1)) || (rc = sc.get(&unsorted, n_runs)) ||
                (rc = sc.get(&d_votes, n_runs)) || (rc = order.alloc(sc, n_runs)))
                return rc;
            hipLaunchKernelGGL(kg::vote_runs_kernel, dim3(grid_of(n_votes)), dim3(kg::kVoteThreads), 0, s, head, hexcl, cexcl, n_votes,
                               n_runs, totals + kSumChanges, run_start, run_cc);
            hipLaunchKernelGGL(kg::vote_pairs_kernel, dim3(grid_of(n_runs)), dim3(kg::kVoteThreads), 0, s, run_start, run_cc, tally.keys(),
                               n_votes, n_runs, oi_bits, unsorted, cnt);
            HIP_TRY(hipGetLastError());
            if ((rc = vote_read_back(t, words, kWordsCnt + kg::kVoteCntMaxVotes, 1))) return rc;
            const uint32_t max_votes = (uint32_t)h[0];
            v_bits = bit_width(max_votes);
            hipLaunchKernelGGL(kg::vote_order_keys_kernel, dim3(grid_of(n_runs)), dim3(kg::kVoteThreads), 0, s, unsorted, n_runs, max_votes,
                               v_bits, order.keys(), order.vals());
            HIP_TRY(hipGetLastError());
            if ((rc = order.sort(t, sc, n_runs, bits_for(n_seqs) + v_bits))) return rc;
            order_keys = order.keys();
            hipLaunchKernelGGL(kg::vote_emit_kernel, dim3(grid_of(n_runs)), dim3(kg::kVoteThreads), 0, s, unsorted, order.vals(), n_runs,
                               d_votes);
            HIP_TRY(hipGetLastError());
        }
    }
    if (!d_votes && (rc = sc.get(&d_votes, 1))) return rc;
    // vote_start and the vote totals: every sequence's slice of the two sorted key arrays
    hipLaunchKernelGGL(kg::region_seq_start_kernel, dim3(grid_of(n_seqs + 1)), dim3(256), 0, s, order_keys, n_runs, v_bits, n_seqs, d_start);
    hipLaunchKernelGGL(kg::region_seq_start_kernel, dim3(grid_of(n_seqs + 1)), dim3(256), 0, s, tally_keys, n_votes, oi_bits, n_seqs, d_tally);
    HIP_TRY(hipGetLastError());
    if (n_seqs > 0) {
        uint32_t *aflag = nullptr, *aexcl = nullptr;
        if ((rc = sc.get(&aflag, n_seqs)) || (rc = sc.get(&aexcl, n_seqs))) return rc;
        hipLaunchKernelGGL(kg::vote_class_kernel, dim3(grid_of(n_seqs)), dim3(kg::kVoteThreads), 0, s, d_votes, d_start, d_tally, d_ccs, d_off,
                           n_seqs, per, *prm, d_cls, aflag, err, cnt);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, aflag, n_seqs, aexcl, partial, totals + kSumAssigned))) return rc;
        if ((rc = vote_read_back(t, words, kWordsTot + kSumAssigned, 1))) return rc;
        n_assigned = h[0];
        if (n_assigned > 0) {
            SortPairs byotu;
            uint32_t *head = nullptr, *bexcl = nullptr;
            if ((rc = byotu.alloc(sc, n_assigned)) || (rc = sc.get(&head, n_assigned)) || (rc = sc.get(&bexcl, n_assigned))) return rc;
            hipLaunchKernelGGL(kg::vote_bin_keys_kernel, dim3(grid_of(n_seqs)), dim3(kg::kVoteThreads), 0, s, d_cls, aflag, aexcl, n_seqs,
                               n_assigned, byotu.keys(), byotu.vals());
            HIP_TRY(hipGetLastError());
            if ((rc = byotu.sort(t, sc, n_assigned, oi_bits))) return rc;
            hipLaunchKernelGGL(kg::vote_heads_kernel, dim3(grid_of(n_assigned)), dim3(kg::kVoteThreads), 0, s, byotu.keys(), byotu.vals(),
                               n_assigned, head, (uint32_t *)nullptr);
            HIP_TRY(hipGetLastError());
            if ((rc = prefix_sum(t, head, n_assigned, bexcl, partial, totals + kSumBins))) return rc;
            if ((rc = vote_read_back(t, words, kWordsTot + kSumBins, 1))) return rc;
            n_bins = h[0];
            unsigned long long *acc = nullptr;
            int32_t *bin_oi = nullptr;
            kg_otu_bin *unsorted = nullptr;
            SortPairs byvotes;
            if ((rc = sc.get(&acc, 4 * n_bins)) || (rc = sc.get(&bin_oi, n_bins)) || (rc = sc.get(&unsorted, n_bins)) ||
                (rc = sc.get(&d_bins, n_bins)) || (rc = byvotes.alloc(sc, n_bins)))
                return rc;
            HIP_TRY(hipMemsetAsync(acc, 0, 4 * n_bins * 8, s));
            hipLaunchKernelGGL(kg::vote_bin_sum_kernel, dim3(grid_of(n_assigned)), dim3(kg::kVoteThreads), 0, s, byotu.keys(), byotu.vals(),
                               head, bexcl, n_assigned, n_bins, d_cls, d_off, n_seqs, bin_oi, acc);
            hipLaunchKernelGGL(kg::vote_bin_records_kernel, dim3(grid_of(n_bins)), dim3(kg::kVoteThreads), 0, s, acc, bin_oi, n_bins, n_votes,
                               unsorted, byvotes.keys(), byvotes.vals());
            HIP_TRY(hipGetLastError());
            if ((rc = byvotes.sort(t, sc, n_bins, bit_width(n_votes)))) return rc;
            SortPairs bylen = byvotes.next();
            if (!bylen.k[0] && (rc = sc.get(&bylen.k[0], n_bins))) return rc;
            hipLaunchKernelGGL(kg::vote_bin_rekey_kernel, dim3(grid_of(n_bins)), dim3(kg::kVoteThreads), 0, s, unsorted, bylen.vals(), n_bins,
                               length_top, bylen.keys());
            HIP_TRY(hipGetLastError());
            if ((rc = bylen.sort(t, sc, n_bins, bit_width(length_top)))) return rc;
            hipLaunchKernelGGL(kg::vote_bin_emit_kernel, dim3(grid_of(n_bins)), dim3(kg::kVoteThreads), 0, s, unsorted, bylen.vals(), n_bins,
                               d_bins);
            HIP_TRY(hipGetLastError());
        }
    }
    if (!d_bins && (rc = sc.get(&d_bins, 1))) return rc;
    HIP_TRY(hipEventRecord(t->ev[kEvStageEnd], s));
    if ((rc = read_error_words(t, words, kWordsTot, kPinStage,                      // (in the order they are reported)
                               {{kg::kVoteErrHitSlice, KG_ERR_ARG, "hit ", ": its container field is not the container whose slice of hits[] it lies in"},
                                {kg::kVoteErrHitOrder, KG_ERR_ARG, "hit ", ": from0InProt below its predecessor's (hits[] must be in (container, from0InProt) order)"},
                                {kg::kVoteErrCallSlice, KG_ERR_ARG, "CALL ", ": its container field is not the container whose slice of calls[] it lies in"},
                                {kg::kVoteErrCallOrder, KG_ERR_ARG, "CALL ", ": start does not exceed its predecessor's (the CALL starts of a container must ascend strictly)"},
                                {kg::kVoteErrOtu, KG_ERR_ARG, "hit ", ": a voting hit with oI < 0"},
                                {kg::kVoteErrTotal, KG_ERR_LIMIT, "sequence ", ": 2^31 or more votes or CALLs"}})))
        return rc;
    set->st.hits = (int64_t)n;
    set->st.accepted = (int64_t)h[kWordsCnt + kg::kVoteCntAccepted];
    set->st.votes = (int64_t)n_votes;
    set->st.pairs = (int64_t)n_runs;
    set->st.seqs_with_votes = (int64_t)h[kWordsCnt + kg::kVoteCntWithVotes];
    set->st.assigned = (int64_t)h[kWordsCnt + kg::kVoteCntAssigned];
    set->st.bins = (int64_t)n_bins;
    set->st.assigned_length = (int64_t)h[kWordsCnt + kg::kVoteCntAssignedLen];
    set->st.total_length = (int64_t)length_top;
    HIP_TRY(hipEventElapsedTime(&set->st.ms, t->ev[kEvStageBegin], t->ev[kEvStageEnd]));
    // the four arrays of the set leave the scratch: everything else goes back to the cache
    set->d_votes = set->keep(sc, d_votes);
    set->d_seq_start = set->keep(sc, d_start);
    set->d_classes = set->keep(sc, d_cls);
    set->d_bins = set->keep(sc, d_bins);
    set->count = (int64_t)n_runs;
    set->n_seqs = (int64_t)n_seqs;
    set->n_bins = (int64_t)n_bins;
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_result_otu_votes(kg_result *r, const kg_vote_params *p, const int64_t *offsets, kg_voteset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!r) return fail(KG_ERR_ARG, "null kg_result");
    int rc = check_vote_params(p);
    if (rc) return rc;
    if (!r->d_ccs) return fail(KG_ERR_ARG, "a KG_F_SKIP_AGGREGATE result has no CALL records and no events to vote by");
    if ((rc = check_vote_offsets(offsets, r->st.n_seqs))) return rc;
    if ((uint64_t)r->st.n_hits >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more hit records in one call");
    if ((uint64_t)r->st.n_calls >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more CALL records in one call");
    if (r->st.n_hits > 0 && !r->d_ev) return fail(KG_ERR_ARG, "the result has no hit events");
    CallScope cs(r->tab, "a kg_scan* is in flight on this result's kg_table");
    if (cs.rc) return cs.rc;
    std::unique_ptr<kg_voteset> set;
    if ((rc = make_set(cs, set))) return rc;
    if ((rc = votes_impl(cs.t, p, r->d_hits, r->d_ev, (uint64_t)r->st.n_hits, r->d_chs, r->d_calls, (uint64_t)r->st.n_calls, r->d_ccs,
                         (uint64_t)r->st.n_seqs, r->per, offsets, set.get())))
        return rc;
    return hand_out(cs, set, out);
}

int kg_otu_votes_hits(int device, const kg_vote_params *p, const kg_hit *hits, const int64_t *container_hit_start,
                      const uint8_t *hit_events, const kg_call *calls, const int64_t *container_call_start, int64_t n_seqs,
                      int32_t per, const int64_t *offsets, kg_voteset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = check_vote_params(p);
    if (rc) return rc;
    if (per != 1 && per != 6) return fail(KG_ERR_ARG, "per must be 6 (DNA) or 1 (-a): " + kmer_text(per));
    if ((rc = check_vote_offsets(offsets, n_seqs))) return rc;
    if (!container_hit_start || !container_call_start) return fail(KG_ERR_ARG, "null container start array");
    const int64_t n_cont = n_seqs * per;
    if ((rc = check_vote_starts(container_hit_start, n_cont, "container_hit_start")) ||
        (rc = check_vote_starts(container_call_start, n_cont, "container_call_start")))
        return rc;
    const int64_t n = container_hit_start[n_cont], n_calls = container_call_start[n_cont];
    if ((uint64_t)n >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more hit records in one call");
    if ((uint64_t)n_calls >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more CALL records in one call");
    if (n && (!hits || !hit_events)) return fail(KG_ERR_ARG, "null hit records or hit events");
    if (n_calls && !calls) return fail(KG_ERR_ARG, "null CALL records");
    CallScope cs(device);               // the call's context: closed on every failure below, kept by the set on success
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    std::unique_ptr<kg_voteset> set;
    if ((rc = make_set(cs, set))) return rc;
    {
        Scratch sc(t);
        kg_hit *d_hits = nullptr;
        uint8_t *d_ev = nullptr;
        kg_call *d_calls = nullptr;
        int64_t *d_chs = nullptr, *d_ccs = nullptr;
        if ((rc = sc.get(&d_hits, n ? (size_t)n : 1)) || (rc = sc.get(&d_ev, n ? (size_t)n : 1)) ||
            (rc = sc.get(&d_calls, n_calls ? (size_t)n_calls : 1)) || (rc = sc.get(&d_chs, (size_t)n_cont + 1)) ||
            (rc = sc.get(&d_ccs, (size_t)n_cont + 1)))
            return rc;
        if (n) {
            HIP_TRY(hipMemcpyAsync(d_hits, hits, (size_t)n * sizeof(kg_hit), hipMemcpyHostToDevice, t->stream));
            HIP_TRY(hipMemcpyAsync(d_ev, hit_events, (size_t)n, hipMemcpyHostToDevice, t->stream));
        }
        if (n_calls) HIP_TRY(hipMemcpyAsync(d_calls, calls, (size_t)n_calls * sizeof(kg_call), hipMemcpyHostToDevice, t->stream));
        HIP_TRY(hipMemcpyAsync(d_chs, container_hit_start, ((size_t)n_cont + 1) * 8, hipMemcpyHostToDevice, t->stream));
        HIP_TRY(hipMemcpyAsync(d_ccs, container_call_start, ((size_t)n_cont + 1) * 8, hipMemcpyHostToDevice, t->stream));
        if ((rc = votes_impl(t, p, d_hits, d_ev, (uint64_t)n, d_chs, d_calls, (uint64_t)n_calls, d_ccs, (uint64_t)n_seqs, (uint32_t)per,
                             offsets, set.get())))
            return rc;
    }
    return hand_out(cs, set, out);
}

int64_t kg_voteset_count(const kg_voteset *s) { return s ? s->count : 0; }

int64_t kg_voteset_bins(const kg_voteset *s) { return s ? s->n_bins : 0; }

int kg_voteset_copy_votes(const kg_voteset *s, int64_t first, int64_t count, kg_otu_vote *dst)
{
    return copy_records(s, device_of(s), s ? s->d_votes : nullptr, 1, s ? s->count : 0, first, count, dst, "kg_voteset_copy_votes");
}

int kg_voteset_copy_classes(const kg_voteset *s, int64_t first, int64_t count, kg_otu_class *dst)
{
    return copy_records(s, device_of(s), s ? s->d_classes : nullptr, 1, s ? s->n_seqs : 0, first, count, dst, "kg_voteset_copy_classes");
}

int kg_voteset_copy_bins(const kg_voteset *s, int64_t first, int64_t count, kg_otu_bin *dst)
{
    return copy_records(s, device_of(s), s ? s->d_bins : nullptr, 1, s ? s->n_bins : 0, first, count, dst, "kg_voteset_copy_bins");
}

int kg_voteset_seq_start(const kg_voteset *s, int64_t *dst)
{
    return copy_starts(s, device_of(s), s ? s->d_seq_start : nullptr, s ? s->n_seqs : 0, dst);
}

int kg_voteset_stats(const kg_voteset *s, kg_vote_stats *out) { return copy_stats(s, s ? &s->st : nullptr, out); }

void kg_voteset_free(kg_voteset *s) { delete s; }

}  // extern "C"
