// kg_host_compose.hpp -- kg_contigs_compose: the tetranucleotide counts of every contig, the label rows of the training
// contigs, every contig's score under every model and its bin (kernels: kg_compose.hpp).
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_coding.hpp (it uses its Lg) and kg_host_votes.hpp.
#pragma once

struct kg_compset : SetBase {
    kg_comp_class *d_classes = nullptr; // n_seqs
    uint32_t *d_counts = nullptr;       // N: n_seqs * 256
    int64_t *d_scores = nullptr;        // S: n_seqs * (n_models + 1), only when kept
    int64_t n_seqs = 0;
    std::vector<int32_t> row_labels;    // the label rows the call made, ascending ...
    std::vector<int64_t> row_counts;    // ... 256 counts each
    int64_t background[kg::kCompBins] = {};
    std::vector<int32_t> model_labels;  // the models the scores are under, in their order
    kg_comp_stats st = {};
};

static_assert(sizeof(kg_comp_params) == 24 && sizeof(kg_comp_class) == 40 && sizeof(kg_comp_stats) == 72, "record layouts of include/kmerguts_hip.h");

namespace {

static_assert(kg::kCompCntWords <= kPinStageWords, "stage words must fit their pinned words");
constexpr int64_t kCompMaxRows = 1ll << 20;

int check_comp_params(const kg_comp_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_comp_params");
    if (p->min_len < 0) return fail(KG_ERR_ARG, "min_len must be >= 0");
    if (p->min_margin < 0) return fail(KG_ERR_ARG, "min_margin must be >= 0");
    if (p->min_train < 0) return fail(KG_ERR_ARG, "min_train must be >= 0");
    if (p->reserved != 0) return fail(KG_ERR_ARG, "kg_comp_params.reserved must be 0");
    return KG_OK;
}

// rule 4's conditions on a caller's model
int check_comp_model(const int32_t *labels, const int64_t *counts, int64_t n_models)
{
    if (n_models < 0) return fail(KG_ERR_ARG, "n_models < 0");
    if (!counts) {
        if (labels || n_models) return fail(KG_ERR_ARG, "model_labels without model_counts (both are given or both are NULL)");
        return KG_OK;
    }
    if (n_models > kCompMaxRows) return fail(KG_ERR_LIMIT, "more than 2^20 model rows");
    if (n_models && !labels) return fail(KG_ERR_ARG, "model_counts without model_labels (both are given or both are NULL)");
    for (int64_t m = 0; m <= n_models; m++) {
        const std::string name = m < n_models ? "model row " + kmer_text(m) : std::string("the model's background row");
        if (m < n_models && labels[m] < 0) return fail(KG_ERR_ARG, name + ": label below 0");
        if (m > 0 && m < n_models && labels[m] <= labels[m - 1]) return fail(KG_ERR_ARG, name + ": labels must ascend strictly");
        uint64_t sum = 0;
        for (int t = 0; t < kg::kCompBins; t++) {
            const int64_t c = counts[m * kg::kCompBins + t];
            if (c < 0) return fail(KG_ERR_ARG, name + ": count " + kmer_text(t) + " is negative");
            sum += (uint64_t)c;
            if (sum >= (1ull << 62)) return fail(KG_ERR_ARG, name + ": counts sum to 2^62 or more");
        }
    }
    return KG_OK;
}

// rule 5: one row of counts -> one row of W
void comp_weights_of(const int64_t *c, int32_t *w)
{
    uint64_t sum = 0;
    for (int t = 0; t < kg::kCompBins; t++) sum += (uint64_t)c[t];
    const int32_t lg_s = coding_lg(sum + kg::kCompBins);
    for (int t = 0; t < kg::kCompBins; t++) w[t] = coding_lg((uint64_t)c[t] + 1) - lg_s;
}

}  // namespace

extern "C" {

int kg_contigs_compose(int device, const kg_comp_params *p, const uint8_t *seq, int seq_on_device, const int64_t *offsets,
                       int64_t n_seqs, const int32_t *labels, const int32_t *model_labels, const int64_t *model_counts,
                       int64_t n_models, kg_compset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = check_comp_params(p);
    if (rc) return rc;
    uint64_t total = 0;
    if ((rc = check_orf_batch(seq, offsets, n_seqs, &total))) return rc;
    if (total >= (1ull << 40)) return fail(KG_ERR_LIMIT, "2^40 or more bytes in one call");
    const uint64_t n = (uint64_t)n_seqs;
    int64_t n_labelled = 0;
    for (uint64_t k = 0; k < n; k++) {
        if (offsets[k + 1] - offsets[k] >= (1ll << 30)) return fail(KG_ERR_LIMIT, "contig " + kmer_text((int64_t)k) + ": 2^30 or more nucleotides");
        if (labels && labels[k] < -1) return fail(KG_ERR_ARG, "contig " + kmer_text((int64_t)k) + ": label " + kmer_text(labels[k]) + " is below -1");
        if (labels && labels[k] >= 0) n_labelled++;
    }
    if ((rc = check_comp_model(model_labels, model_counts, n_models))) return rc;
    const bool own_model = model_counts != nullptr;
    // Host memory the stream copies from or into: declared in front of the scratch, whose destructor waits for the stream.
    std::vector<int32_t> rows;          // the distinct labels >= 0, ascending
    std::vector<uint32_t> order;        // the contigs grouped by row, then all of them for the background
    std::vector<kg::CompWork> work;
    std::vector<int64_t> counts;        // (R + 1) * 256: the label rows, then G
    std::vector<int32_t> W;
    std::vector<int32_t> mlab;
    if (!own_model) {
        if (labels) {
            for (uint64_t k = 0; k < n; k++) if (labels[k] >= 0) rows.push_back(labels[k]);
            std::sort(rows.begin(), rows.end());
            rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        }
        if ((int64_t)rows.size() > kCompMaxRows) return fail(KG_ERR_LIMIT, "more than 2^20 label rows");
        // the dense numbering: a counting sort of the labelled contigs by row
        const size_t R = rows.size();
        std::vector<uint32_t> start(R + 2, 0);
        std::vector<uint32_t> row_of(n_labelled ? n : 0);
        for (uint64_t k = 0; n_labelled && k < n; k++) {
            if (labels[k] < 0) continue;
            row_of[k] = (uint32_t)(std::lower_bound(rows.begin(), rows.end(), labels[k]) - rows.begin());
            start[row_of[k] + 1]++;
        }
        for (size_t r = 0; r < R; r++) start[r + 1] += start[r];
        start[R + 1] = start[R] + (uint32_t)n;
        order.resize((size_t)n_labelled + n);
        {
            std::vector<uint32_t> at(start.begin(), start.begin() + R);
            for (uint64_t k = 0; n_labelled && k < n; k++) if (labels[k] >= 0) order[at[row_of[k]]++] = (uint32_t)k;
            for (uint64_t k = 0; k < n; k++) order[(size_t)n_labelled + k] = (uint32_t)k;
        }
        for (size_t r = 0; r <= R; r++)
            for (uint32_t a = start[r]; a < start[r + 1]; a += kg::kCompTrainChunk)
                work.push_back({(uint32_t)r, a, std::min<uint32_t>(kg::kCompTrainChunk, start[r + 1] - a), 0u});
        counts.assign((R + 1) * kg::kCompBins, 0);
    }
    Events<4> ev;                       // the counting passes begin, end; the scores begin, end
    CallScope cs(device);               // the call's context: closed on every failure below, kept by the set on success
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    hipStream_t s = t->stream;
    std::unique_ptr<kg_compset> set;
    if ((rc = make_set(cs, set))) return rc;
    if ((rc = ev.create())) return rc;
    {
        Scratch sc(t);
        const uint8_t *d_seq = nullptr;
        if ((rc = batch_on_device(t, sc, seq, seq_on_device, total, &d_seq))) return rc;
        int64_t *d_off = nullptr, *d_win = nullptr, *d_S = nullptr;
        int32_t *d_lab = nullptr, *d_W = nullptr, *d_mlab = nullptr;
        uint32_t *d_N = nullptr;
        kg_comp_class *d_cls = nullptr;
        unsigned long long *cnt = nullptr;
        if ((rc = sc.get(&d_off, n + 1)) || (rc = sc.get(&d_lab, std::max<uint64_t>(n, 1))) || (rc = sc.get(&d_win, std::max<uint64_t>(n, 1))) ||
            (rc = sc.get(&d_N, std::max<uint64_t>(n, 1) * kg::kCompBins)) || (rc = sc.get(&d_cls, std::max<uint64_t>(n, 1))) ||
            (rc = sc.get(&cnt, kg::kCompCntWords)))
            return rc;
        HIP_TRY(hipMemcpyAsync(d_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s));
        if (n && labels) HIP_TRY(hipMemcpyAsync(d_lab, labels, n * 4, hipMemcpyHostToDevice, s));
        else HIP_TRY(hipMemsetAsync(d_lab, 0xFF, std::max<uint64_t>(n, 1) * 4, s));        // (all -1)
        HIP_TRY(hipMemsetAsync(d_N, 0, std::max<uint64_t>(n, 1) * kg::kCompBins * 4, s));
        HIP_TRY(hipMemsetAsync(cnt, 0, kg::kCompCntWords * 8, s));
        HIP_TRY(hipEventRecord(ev[0], s));
        const uint64_t n_tiles = (total + kg::kCompTile - 1) / kg::kCompTile;
        if (n_tiles > 0 && n > 0) {
            const uint64_t per_wg = (n_tiles + kg::kCompMaxGrid - 1) / kg::kCompMaxGrid;
            hipLaunchKernelGGL(kg::comp_count_kernel, dim3((uint32_t)((n_tiles + per_wg - 1) / per_wg)), dim3(kg::kCompThreads), 0, s, d_seq,
                               total, d_off, n, n_tiles, per_wg, d_N);
        }
        if (n > 0)
            hipLaunchKernelGGL(kg::comp_fold_kernel, dim3((uint32_t)std::min<uint64_t>(n, kg::kCompMaxGrid * 16)), dim3(kg::kCompThreads), 0, s,
                               d_N, n, d_win, cnt);
        HIP_TRY(hipGetLastError());
        int64_t M = n_models;
        if (!own_model) {
            // the wait in the middle: the rows come down, W is made on the host and goes up
            const size_t R = rows.size();
            if (!work.empty()) {
                uint32_t *d_order = nullptr;
                kg::CompWork *d_work = nullptr;
                unsigned long long *d_C = nullptr;
                if ((rc = sc.get(&d_order, order.size())) || (rc = sc.get(&d_work, work.size())) || (rc = sc.get(&d_C, counts.size()))) return rc;
                HIP_TRY(hipMemcpyAsync(d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, s));
                HIP_TRY(hipMemcpyAsync(d_work, work.data(), work.size() * sizeof(kg::CompWork), hipMemcpyHostToDevice, s));
                HIP_TRY(hipMemsetAsync(d_C, 0, counts.size() * 8, s));
                hipLaunchKernelGGL(kg::comp_train_kernel, dim3((uint32_t)std::min<uint64_t>(work.size(), kg::kCompMaxGrid * 16)),
                                   dim3(kg::kCompThreads), 0, s, d_N, d_order, d_work, (uint64_t)work.size(), d_C);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(counts.data(), d_C, counts.size() * 8, hipMemcpyDeviceToHost, s));
            }
            HIP_TRY(hipEventRecord(ev[1], s));
            HIP_TRY(hipStreamSynchronize(s));
            for (size_t r = 0; r <= R; r++) {
                const int64_t *c = counts.data() + r * kg::kCompBins;
                int64_t sum = 0;
                for (int b = 0; b < kg::kCompBins; b++) sum += c[b];
                if (r < R && sum < p->min_train) continue;
                W.resize(W.size() + kg::kCompBins);
                comp_weights_of(c, W.data() + W.size() - kg::kCompBins);
                if (r < R) mlab.push_back(rows[r]);
            }
            M = (int64_t)mlab.size();
        } else {
            HIP_TRY(hipEventRecord(ev[1], s));
            W.resize((size_t)(M + 1) * kg::kCompBins);
            for (int64_t m = 0; m <= M; m++) comp_weights_of(model_counts + m * kg::kCompBins, W.data() + m * kg::kCompBins);
            mlab.assign(model_labels, model_labels + M);
        }
        const bool keep = p->keep_scores != 0;
        if (keep && (unsigned __int128)n * (uint64_t)(M + 1) * 8 >= ((unsigned __int128)1 << 40))
            return fail(KG_ERR_LIMIT, "a score matrix of 2^40 bytes or more");
        if ((rc = sc.get(&d_W, W.size())) || (rc = sc.get(&d_mlab, std::max<size_t>(mlab.size(), 1)))) return rc;
        if (keep && (rc = sc.get(&d_S, std::max<uint64_t>(n * (uint64_t)(M + 1), 1)))) return rc;
        HIP_TRY(hipMemcpyAsync(d_W, W.data(), W.size() * 4, hipMemcpyHostToDevice, s));
        if (M) HIP_TRY(hipMemcpyAsync(d_mlab, mlab.data(), mlab.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(ev[2], s));
        if (n > 0) {
            const kg::CompDecide dec = {p->min_len, p->min_margin};
            const uint64_t steps = (n + kg::kCompScoreSeqs - 1) / kg::kCompScoreSeqs;
            hipLaunchKernelGGL(kg::comp_score_kernel, dim3((uint32_t)std::min<uint64_t>(steps, kg::kCompMaxGrid * 4)), dim3(kg::kCompThreads), 0,
                               s, d_N, d_win, d_off, d_lab, n, d_W, d_mlab, (uint32_t)M, dec, d_cls, d_S, cnt);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(ev[3], s));
        if ((rc = read_error_words(t, cnt, kg::kCompCntWords, kPinStage, {}))) return rc;
        const uint64_t *h = t->h_pin + kPinStage;
        kg_comp_stats &st = set->st;
        st.seqs = n_seqs;
        st.labelled = n_labelled;
        st.label_rows = (int64_t)rows.size();
        st.models = M;
        st.windows = (int64_t)h[kg::kCompCntWindows];
        st.decided = (int64_t)h[kg::kCompCntDecided];
        st.decided_unlabelled = (int64_t)h[kg::kCompCntUnlabelled];
        st.conflicts = (int64_t)h[kg::kCompCntConflicts];
        st.ms_count = ev.ms(0, 1);
        st.ms_score = ev.ms(2, 3);
        // the set's arrays leave the scratch: everything else goes back to the cache
        set->d_classes = set->keep(sc, d_cls);
        set->d_counts = set->keep(sc, d_N);
        set->d_scores = set->keep(sc, d_S);
    }
    set->n_seqs = n_seqs;
    set->row_labels = std::move(rows);
    if (!own_model) {
        std::copy(counts.end() - kg::kCompBins, counts.end(), set->background);
        counts.resize(counts.size() - kg::kCompBins);
        set->row_counts = std::move(counts);
    }
    set->model_labels = std::move(mlab);
    return hand_out(cs, set, out);
}

int64_t kg_compset_rows(const kg_compset *s) { return s ? (int64_t)s->row_labels.size() : 0; }

int64_t kg_compset_models(const kg_compset *s) { return s ? (int64_t)s->model_labels.size() : 0; }

int kg_compset_copy_classes(const kg_compset *s, int64_t first, int64_t count, kg_comp_class *dst)
{
    return copy_records(s, device_of(s), s ? s->d_classes : nullptr, 1, s ? s->n_seqs : 0, first, count, dst, "kg_compset_copy_classes");
}

int kg_compset_copy_counts(const kg_compset *s, int64_t first, int64_t count, int32_t *dst)
{
    return copy_records(s, device_of(s), s ? (const int32_t *)s->d_counts : nullptr, kg::kCompBins, s ? s->n_seqs : 0, first, count, dst, "kg_compset_copy_counts");
}

int kg_compset_copy_rows(const kg_compset *s, int64_t first, int64_t count, int32_t *labels_dst, int64_t *counts_dst)
{
    if (!s) return fail(KG_ERR_ARG, "null argument");
    const int64_t have = (int64_t)s->row_labels.size();
    if (first < 0 || count < 0 || first + count > have) return fail(KG_ERR_ARG, "kg_compset_copy_rows: range outside the set");
    if (count == 0) return KG_OK;
    HIP_TRY(hipSetDevice(s->tab->device));
    if (labels_dst) HIP_TRY(hipMemcpy(labels_dst, s->row_labels.data() + first, (size_t)count * 4, hipMemcpyDefault));
    if (counts_dst)
        HIP_TRY(hipMemcpy(counts_dst, s->row_counts.data() + (size_t)first * kg::kCompBins, (size_t)count * kg::kCompBins * 8, hipMemcpyDefault));
    return KG_OK;
}

int kg_compset_background(const kg_compset *s, int64_t *dst)
{
    if (!s || !dst) return fail(KG_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(s->tab->device));
    HIP_TRY(hipMemcpy(dst, s->background, sizeof s->background, hipMemcpyDefault));
    return KG_OK;
}

int kg_compset_model_labels(const kg_compset *s, int64_t first, int64_t count, int32_t *dst)
{
    return copy_records(s, device_of(s), s ? s->model_labels.data() : nullptr, 1, s ? (int64_t)s->model_labels.size() : 0, first, count, dst,
                        "kg_compset_model_labels");
}

int kg_compset_copy_scores(const kg_compset *s, int64_t first, int64_t count, int64_t *dst)
{
    if (s && !s->d_scores) return fail(KG_ERR_ARG, "kg_compset_copy_scores: the call did not keep the score matrix (keep_scores was 0)");
    return copy_records(s, device_of(s), s ? s->d_scores : nullptr, s ? s->model_labels.size() + 1 : 0, s ? s->n_seqs : 0, first, count, dst,
                        "kg_compset_copy_scores");
}

int kg_compset_stats(const kg_compset *s, kg_comp_stats *out) { return copy_stats(s, s ? &s->st : nullptr, out); }

void kg_compset_free(kg_compset *s) { delete s; }

}  // extern "C"
