// kg_host_starts.hpp -- kg_orfset_starts / kg_starts_orfs / kg_start_weights_from: the start codon of every movable ORF record,
// chosen by a trained start-site score (kernels: kg_starts.hpp).
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_coding.hpp (it reads and makes kg_orfset, and uses
// that stage's Lg and checks).
#pragma once

static_assert(kg::kStartErrWords + kg::kStartCntWords <= kPinStageWords, "stage words must fit their pinned words");
static_assert(sizeof(kg_start_params) == 24 && sizeof(kg_start_model) == 8 * 2 * kg::kStartBins &&
              sizeof(kg_start_weights) == 4 * kg::kStartBins && sizeof(kg_start_stats) == 48,
              "record layouts of include/kmerguts_hip.h");

namespace {

int check_start_params(const kg_start_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_start_params");
    if (p->min_res < 1) return fail(KG_ERR_ARG, "min_res must be >= 1");
    if (p->start_codons < 0 || p->start_codons > 7) return fail(KG_ERR_ARG, "start_codons must be a mask of 1 (ATG), 2 (GTG), 4 (TTG)");
    if (p->rounds < 1 || p->rounds > 16) return fail(KG_ERR_ARG, "rounds must be between 1 and 16");
    if (p->reserved != 0) return fail(KG_ERR_ARG, "kg_start_params.reserved must be 0");
    if (p->min_train_starts < 0) return fail(KG_ERR_ARG, "min_train_starts must be >= 0");
    return KG_OK;
}

// rule 7 for one row of `width` bins: w[c] from chosen[c] and cand[c], c in [first, width)
int start_weight_row(const int64_t *chosen, const int64_t *cand, int first, int width, const std::string &name, int32_t *w)
{
    uint64_t sum[2] = {0, 0};
    for (int which = 0; which < 2; which++) {
        const int64_t *c = which ? cand : chosen;
        for (int b = first; b < width; b++) {
            if (c[b] < 0) return fail(KG_ERR_ARG, std::string(which ? "candidate" : "chosen") + " count of " + name + " is negative");
            sum[which] += (uint64_t)c[b];
            if (sum[which] >= (1ull << 62))
                return fail(KG_ERR_ARG, std::string(which ? "candidate" : "chosen") + " counts of " + name + " sum to 2^62 or more");
        }
    }
    const int32_t lg_s = coding_lg(sum[0] + (uint64_t)(width - first)), lg_c = coding_lg(sum[1] + (uint64_t)(width - first));
    for (int b = first; b < width; b++) w[b] = coding_lg((uint64_t)chosen[b] + 1) - lg_s - coding_lg((uint64_t)cand[b] + 1) + lg_c;
    return KG_OK;
}

int start_weights_of(const kg_start_model *m, kg_start_weights *w)
{
    int rc;
    for (int i = 0; i < kg::kStartWin; i++)
        if ((rc = start_weight_row(m->chosen[i], m->cand[i], 0, 4, "position " + kmer_text(i), w->pos[i]))) return rc;
    w->type[0] = 0;
    return start_weight_row(m->type_chosen, m->type_cand, 1, 4, "the types", w->type);
}

// The passes of one call over d_orfs[n] (device records complete on t->stream), d_seq (the batch's bytes on the device, null
// when there are none) and offsets (host, checked): begin() -- the records, with a wait --, list() -- the candidates, with a
// wait --, choose() -- the rounds, each with a wait when the call trains --, then apply().
struct StartsWork {
    kg_table *t;
    // host memory that copies on the stream read or write (in front of the scratch, whose destructor waits for that stream)
    std::vector<kg_start_weights> round_weights;
    uint64_t h_counts[2 * kg::kStartBins] = {};
    Scratch sc;
    kg::StartBatch b = {};
    const uint8_t *kind_c = nullptr;
    int64_t *d_off = nullptr;
    unsigned long long *words = nullptr, *err = nullptr, *cnt = nullptr, *counts = nullptr, *partial_v = nullptr, *partial_c = nullptr,
                       *best = nullptr;
    uint32_t *lens = nullptr, *excl = nullptr, *cur = nullptr, *next = nullptr, *type = nullptr;
    int32_t *kcap = nullptr, *d_T = nullptr, *d_W = nullptr;
    uint8_t *kind = nullptr;
    uint64_t *partial = nullptr;
    int64_t *E_end = nullptr, *suf = nullptr;
    kg::StartCands cands = {};
    uint64_t n = 0, P = 0, NC = 0;
    uint32_t n_chunks = 0, cand_grid = 1;
    bool chosen = false;                // choose() has run: cur[] holds every movable record's k
    kg_start_model model = {};
    kg_start_stats st = {};

    explicit StartsWork(kg_table *tt) : t(tt), sc(tt) {}

    int begin(const kg_start_params *p, const kg_orf *orfs, uint64_t n_orfs, const kg::StartLimits &lim, const uint8_t *seq,
              const int64_t *offsets, uint64_t n_seqs)
    {
        n = n_orfs;
        hipStream_t s = t->stream;
        int rc;
        const uint64_t n1 = std::max<uint64_t>(n, 1);
        if ((rc = sc.get(&d_off, n_seqs + 1)) || (rc = sc.get(&words, 16)) || (rc = sc.get(&lens, n1)) || (rc = sc.get(&excl, n1)) ||
            (rc = sc.get(&kcap, n1)) || (rc = sc.get(&kind, n1)) || (rc = sc.get(&partial, n / kg::kScanChunk + 2)))
            return rc;
        err = words;
        cnt = words + kg::kStartErrWords;
        b = kg::StartBatch{orfs, n, excl, kcap, seq, d_off, (uint32_t)p->start_codons};
        kind_c = kind;
        HIP_TRY(hipMemcpyAsync(d_off, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(err, 0x7F, kg::kStartErrWords * 8, s));
        HIP_TRY(hipMemsetAsync(cnt, 0, kg::kStartCntWords * 8, s));
        if (n > 0) {
            hipLaunchKernelGGL(kg::starts_lens_kernel, dim3(grid_of(n)), dim3(256), 0, s, orfs, n, d_off, n_seqs, lim, p->min_res, lens, kcap,
                               kind, err, cnt);
            HIP_TRY(hipGetLastError());
            if ((rc = prefix_sum(t, lens, n, excl, partial, (uint64_t *)(cnt + kg::kStartCntCodons)))) return rc;
        }
        if ((rc = check())) return rc;
        P = counter(kg::kStartCntCodons);
        if (P >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more codons in one call");
        st.movable = (int64_t)counter(kg::kStartCntMovable);
        st.training_records = (int64_t)counter(kg::kStartCntTrain);
        n_chunks = (uint32_t)((P + kg::kStartChunk - 1) / kg::kStartChunk);
        return KG_OK;
    }
    // the candidate list and the cand counts of rule 6; T: host memory that lives until the stream has been waited for
    int list(const int32_t *T)
    {
        hipStream_t s = t->stream;
        int rc;
        const uint64_t n1 = std::max<uint64_t>(n, 1), c1 = std::max<uint32_t>(n_chunks, 1);
        if ((rc = sc.get(&d_T, kg::kCodingBins)) || (rc = sc.get(&d_W, kg::kStartBins)) || (rc = sc.get(&counts, 2 * kg::kStartBins)) ||
            (rc = sc.get(&partial_v, c1)) || (rc = sc.get(&partial_c, c1)) || (rc = sc.get(&E_end, n1)) || (rc = sc.get(&best, n1)) ||
            (rc = sc.get(&cur, n1)) || (rc = sc.get(&next, n1)) || (rc = sc.get(&suf, n1)) || (rc = sc.get(&type, n1)))
            return rc;
        HIP_TRY(hipMemcpyAsync(d_T, T, kg::kCodingBins * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(counts, 0, 2 * kg::kStartBins * 8, s));
        if (n_chunks > 0) {
            hipLaunchKernelGGL(kg::starts_pairs_kernel, dim3(n_chunks), dim3(kg::kStartThreads), 0, s, b, P, d_T, partial_v, partial_c);
            hipLaunchKernelGGL(kg::starts_top_kernel, dim3(1), dim3(kg::kStartThreads), 0, s, partial_v, partial_c, n_chunks,
                               cnt + kg::kStartCntCands);
            HIP_TRY(hipGetLastError());
        }
        // the wait that sizes the list
        if ((rc = check())) return rc;
        NC = counter(kg::kStartCntCands);
        st.candidates = (int64_t)NC;
        const uint64_t nc1 = std::max<uint64_t>(NC, 1);
        if ((rc = sc.get(&cands.rec, nc1)) || (rc = sc.get(&cands.k, nc1)) || (rc = sc.get(&cands.win, nc1)) || (rc = sc.get(&cands.E, nc1)))
            return rc;
        cand_grid = (uint32_t)std::min<uint64_t>(kg::kStartMaxGrid, std::max<uint64_t>(1, (NC + kg::kStartThreads - 1) / kg::kStartThreads));
        if (n_chunks > 0) {
            hipLaunchKernelGGL(kg::starts_cands_kernel, dim3(n_chunks), dim3(kg::kStartThreads), 0, s, b, P, d_T, partial_v, partial_c, NC,
                               cands, E_end);
            hipLaunchKernelGGL(kg::starts_window_kernel, dim3(cand_grid), dim3(kg::kStartThreads), 0, s, b, cands, NC, kind_c,
                               counts + kg::kStartBins);
            HIP_TRY(hipGetLastError());
        }
        return KG_OK;
    }
    // rule 8: the rounds, or one pass with the caller's weights
    int choose(const kg_start_params *p, const kg_start_weights *caller)
    {
        hipStream_t s = t->stream;
        const int R = caller ? 1 : p->rounds;
        round_weights.resize((size_t)R);
        int rc;
        if (n > 0) HIP_TRY(hipMemsetAsync(cur, 0, n * 4, s));
        for (int r = 0; r < R; r++) {
            if (caller) {
                round_weights[r] = *caller;
            } else {
                HIP_TRY(hipMemsetAsync(counts, 0, kg::kStartBins * 8, s));
                if (NC > 0) {
                    hipLaunchKernelGGL(kg::starts_count_kernel, dim3(cand_grid), dim3(kg::kStartThreads), 0, s, cands, NC, kind_c, cur, counts);
                    HIP_TRY(hipGetLastError());
                }
                // the round's wait: the counts come down, the weights are made on the host and go up
                HIP_TRY(hipMemcpyAsync(h_counts, counts, sizeof h_counts, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                for (int i = 0; i < kg::kStartWin; i++)
                    for (int c = 0; c < 4; c++) {
                        model.chosen[i][c] = (int64_t)h_counts[4 * i + c];
                        model.cand[i][c] = (int64_t)h_counts[kg::kStartBins + 4 * i + c];
                    }
                for (int c = 0; c < 4; c++) {
                    model.type_chosen[c] = (int64_t)h_counts[4 * kg::kStartWin + c];
                    model.type_cand[c] = (int64_t)h_counts[kg::kStartBins + 4 * kg::kStartWin + c];
                }
                if ((rc = start_weights_of(&model, &round_weights[r]))) return rc;
            }
            HIP_TRY(hipMemcpyAsync(d_W, &round_weights[r], sizeof(kg_start_weights), hipMemcpyHostToDevice, s));
            if (n > 0) {
                HIP_TRY(hipMemsetAsync(best, 0, n * 8, s));
                HIP_TRY(hipMemsetAsync(next, 0xFF, n * 4, s));
            }
            if (NC > 0) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(kg::starts_choose_kernel<false>), dim3(cand_grid), dim3(kg::kStartThreads), 0, s, cands, NC,
                                   E_end, d_W, best, next);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(kg::starts_choose_kernel<true>), dim3(cand_grid), dim3(kg::kStartThreads), 0, s, cands, NC,
                                   E_end, d_W, best, next);
                HIP_TRY(hipGetLastError());
            }
            std::swap(cur, next);
        }
        if (NC > 0) {
            hipLaunchKernelGGL(kg::starts_chosen_kernel, dim3(cand_grid), dim3(kg::kStartThreads), 0, s, cands, NC, cur, E_end, suf, type);
            HIP_TRY(hipGetLastError());
        }
        st.rounds_run = R;
        chosen = true;
        return KG_OK;
    }
    // rule 9 into out[n] and shifts[n] (device); prot_start, S and new_lens as starts_apply_kernel takes them
    int apply(const int64_t *prot_start, kg_orf *out, int32_t *shifts, int64_t *S, uint32_t *new_lens)
    {
        if (n == 0) return KG_OK;
        hipLaunchKernelGGL(kg::starts_apply_kernel, dim3(grid_of(n)), dim3(256), 0, t->stream, b.orfs, n, kind_c,
                           chosen ? (const uint32_t *)cur : (const uint32_t *)nullptr, suf, type, prot_start, out, shifts, S, new_lens, cnt);
        HIP_TRY(hipGetLastError());
        return KG_OK;
    }
    int check()
    {
        static const char *const what[kg::kStartErrWords] = {
            ": seq outside [0, n_seqs)", ": strand is neither 0 nor 1", ": outside its contig (0 <= left <= right <= L - 1 does not hold)",
            ": 3 * n_res exceeds right - left + 1", ": its region has another seq or strand, or begins in front of the record's start"};
        return read_record_errors(t, words, kg::kStartErrWords + kg::kStartCntWords, kg::kStartErrWords, what);
    }
    uint64_t counter(int k) const { return t->h_pin[kPinStage + kg::kStartErrWords + k]; }
    // behind begin(): trained 0 / 1 / 2 of the statistics, and when it is not 0 list() and choose(); ev[1], ev[2]: the list has
    // ended, the choices begin
    int list_and_choose(const kg_start_params *p, const int32_t *T, const kg_start_weights *caller, const Events<4> &ev)
    {
        int rc;
        st.trained = caller ? 2 : st.training_records >= p->min_train_starts ? 1 : 0;
        if (st.trained && (rc = list(T))) return rc;
        HIP_TRY(hipEventRecord(ev[1], t->stream));
        HIP_TRY(hipEventRecord(ev[2], t->stream));
        return st.trained ? choose(p, caller) : KG_OK;
    }
    // behind the call's last wait: what moved, and the times between ev[0], ev[1] and ev[2], ev[3]
    void finish(const Events<4> &ev)
    {
        st.moved = (int64_t)counter(kg::kStartCntMoved);
        st.ms_count = ev.ms(0, 1);
        st.ms_choose = ev.ms(2, 3);
    }
};

constexpr const char *kNoShifts = "the set has no shifts (it is not from kg_orfset_starts)";

}  // namespace

extern "C" {

int kg_start_weights_from(const kg_start_model *model, kg_start_weights *weights)
{
    if (!model || !weights) return fail(KG_ERR_ARG, "null argument");
    return start_weights_of(model, weights);
}

int kg_orfset_starts(kg_orfset *os, const kg_start_params *p, const int32_t *table, const kg_start_weights *weights,
                     const kg_regionset *rs, const uint8_t *seq, int seq_on_device, const int64_t *offsets, int64_t n_seqs,
                     kg_orfset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!os) return fail(KG_ERR_ARG, "null kg_orfset");
    int rc = check_start_params(p);
    if (rc) return rc;
    if (!table) return fail(KG_ERR_ARG, "null coding table");
    uint64_t total = 0;
    if ((rc = check_orf_batch(seq, offsets, n_seqs, &total, "ORF set's", os->n_seqs))) return rc;
    if (rs && rs->n_seqs != n_seqs) return fail(KG_ERR_ARG, "n_seqs is not the region set's");
    if (rs && rs->count > os->count) return fail(KG_ERR_ARG, "the ORF set is shorter than the region set");
    if (total >= (1ull << 40)) return fail(KG_ERR_LIMIT, "2^40 or more bytes in one call");
    if (os->count >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more records in one call");
    Events<4> ev;                       // the candidate list begins, ends; the choices begin, end
    CallScope cs(os->tab, "a kg_scan* is in flight on this ORF set's kg_table");
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    hipStream_t s = t->stream;
    std::unique_ptr<kg_orfset> set;
    if ((rc = make_set(cs, set))) return rc;
    set->start_model.reset(new (std::nothrow) kg_start_model());
    if (!set->start_model) return fail(KG_ERR_NOMEM, "out of host memory");
    if ((rc = inherit(set.get(), os))) return rc;
    if ((rc = ev.create())) return rc;
    StartsWork w(t);
    const uint8_t *d_seq = nullptr;
    if ((rc = batch_on_device(t, w.sc, seq, seq_on_device, total, &d_seq))) return rc;
    const uint64_t n = (uint64_t)os->count, n1 = std::max<uint64_t>(n, 1);
    kg_orf *d_out = nullptr;
    int64_t *d_start = nullptr, *d_S = nullptr;
    int32_t *d_shift = nullptr;
    uint32_t *new_lens = nullptr, *new_excl = nullptr;
    if ((rc = w.sc.get(&d_out, n1)) || (rc = w.sc.get(&d_start, n + 1)) || (rc = w.sc.get(&d_shift, n1)) ||
        (os->d_coding && (rc = w.sc.get(&d_S, n1))) || (rc = w.sc.get(&new_lens, n1)) || (rc = w.sc.get(&new_excl, n1)))
        return rc;
    HIP_TRY(hipEventRecord(ev[0], s));
    const kg::StartLimits lim = {rs ? rs->d_regions : nullptr, rs ? (uint64_t)rs->count : 0, nullptr};
    if ((rc = w.begin(p, os->d_orfs, n, lim, d_seq, offsets, (uint64_t)n_seqs))) return rc;
    if ((rc = w.list_and_choose(p, table, weights, ev))) return rc;
    if (d_S && n > 0) HIP_TRY(hipMemcpyAsync(d_S, os->d_coding, n * 8, hipMemcpyDeviceToDevice, s));
    if ((rc = w.apply(os->d_prot_start, d_out, d_shift, d_S, new_lens))) return rc;
    // No 2^32-residue limit here: starts_apply_kernel writes new_lens[i] = len - min(k, len), so no record grows, and every chunk's
    // sum and the total are at most the given set's, which passed that limit when the set was made.
    if ((rc = layout_proteins(t, new_lens, n, new_excl, w.partial, (uint64_t *)(w.cnt + kg::kStartCntResidues), d_start))) return rc;
    // the wait for the residue total
    if ((rc = w.check())) return rc;
    const uint64_t n_res = w.counter(kg::kStartCntResidues);
    uint8_t *d_res = nullptr;
    // rule 9's "old protein from residue k on, residue 0 = 'M'" is the translation of the new record: rule 5 of the ORF section
    // ... but for a repaired record, whose protein is not its extent read through: it has not moved, and keeps the given bytes
    if ((rc = translate_orfs(t, w.sc, d_out, n, d_start, n_res, d_seq, w.d_off, &d_res)) ||
        (rc = keep_repaired(t, d_out, n, d_start, n_res, os, d_res)))
        return rc;
    HIP_TRY(hipEventRecord(ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    w.finish(ev);
    keep_orfs(set.get(), w.sc, d_out, d_start, d_res, n, n_res, (uint64_t)n_seqs);
    set->d_coding = set->keep(w.sc, d_S);
    set->d_shift = set->keep(w.sc, d_shift);
    set->st.residues = (int64_t)n_res;
    *set->start_model = w.model;
    set->start_st = w.st;
    return hand_out(cs, set, out);
}

int kg_orfset_start_shifts(const kg_orfset *s, int64_t first, int64_t count, int32_t *dst)
{
    if (int rc = need_of_set(s, count <= 0 || dst, s && s->d_shift, "kg_orfset_start_shifts", kNoShifts)) return rc;
    return copy_records(s, device_of(s), s->d_shift, 1, s->count, first, count, dst, "kg_orfset_start_shifts");
}

int kg_orfset_start_stats(const kg_orfset *s, kg_start_stats *out)
{
    if (int rc = need_of_set(s, out, s && s->d_shift, "kg_orfset_start_stats", kNoShifts)) return rc;
    *out = s->start_st;
    return KG_OK;
}

int kg_orfset_start_model(const kg_orfset *s, kg_start_model *out)
{
    if (int rc = need_of_set(s, out, s && s->d_shift && s->start_model, "kg_orfset_start_model", kNoShifts)) return rc;
    *out = *s->start_model;
    return KG_OK;
}

int kg_starts_orfs(int device, const kg_start_params *p, const int32_t *table, const kg_start_weights *weights, const kg_orf *orfs,
                   int64_t n, const int32_t *limits, const uint8_t *seq, const int64_t *offsets, int64_t n_seqs, kg_orf *out,
                   int32_t *shifts, kg_start_model *model, kg_start_stats *stats)
{
    int rc = check_start_params(p);
    if (rc) return rc;
    if (!table) return fail(KG_ERR_ARG, "null coding table");
    if (n > 0 && (!out || !shifts)) return fail(KG_ERR_ARG, "null argument");
    uint64_t total = 0;
    int64_t l_max = 0;
    if ((rc = check_coding_lists(orfs, n, seq, offsets, n_seqs, &total, &l_max))) return rc;
    Events<4> ev;
    CallScope cs(device);               // the call's context: closed when the call returns
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    hipStream_t s = t->stream;
    if ((rc = ev.create())) return rc;
    StartsWork w(t);
    kg_orf *d_orfs = nullptr, *d_out = nullptr;
    uint8_t *d_seq = nullptr;
    int32_t *d_lim = nullptr, *d_shift = nullptr;
    const uint64_t n1 = n ? (uint64_t)n : 1;
    if ((rc = coding_upload(t, w.sc, orfs, (uint64_t)n, seq, total, &d_orfs, &d_seq))) return rc;
    if ((rc = w.sc.get(&d_out, n1)) || (rc = w.sc.get(&d_shift, n1)) || (limits && (rc = w.sc.get(&d_lim, n1)))) return rc;
    if (limits && n) HIP_TRY(hipMemcpyAsync(d_lim, limits, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(ev[0], s));
    const kg::StartLimits lim = {nullptr, 0, d_lim};
    if ((rc = w.begin(p, d_orfs, (uint64_t)n, lim, d_seq, offsets, (uint64_t)n_seqs))) return rc;
    if ((rc = w.list_and_choose(p, table, weights, ev))) return rc;
    if ((rc = w.apply(nullptr, d_out, d_shift, nullptr, nullptr))) return rc;
    HIP_TRY(hipEventRecord(ev[3], s));
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(kg_orf), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(shifts, d_shift, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    }
    if ((rc = w.check())) return rc;
    w.finish(ev);
    if (model) *model = w.model;
    if (stats) *stats = w.st;
    return KG_OK;
}

}  // extern "C"
