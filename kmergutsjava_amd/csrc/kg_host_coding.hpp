// kg_host_coding.hpp -- kg_orfset_coding / kg_coding_counts_orfs / kg_coding_score_orfs / kg_coding_table: the in-frame hexamer
// log-odds score of every ORF record, and the free ORFs it drops (kernels: kg_coding.hpp).
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_orfs.hpp (it reads and makes kg_orfset).
#pragma once

static_assert(kg::kCodingErrWords + kg::kCodingCntWords <= kPinStageWords, "stage words must fit their pinned words");
static_assert(sizeof(kg_coding_params) == 16 && sizeof(kg_coding_model) == 2 * 8 * kg::kCodingBins && sizeof(kg_coding_stats) == 56,
              "record layouts of include/kmerguts_hip.h");
static_assert(kg::kCodingNoErr == kNoErr, "the stages' kernels share the error words' \"none\"");

namespace {

int check_coding_params(const kg_coding_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_coding_params");
    if (p->reserved != 0) return fail(KG_ERR_ARG, "kg_coding_params.reserved must be 0");
    if (p->min_train_pairs < 0) return fail(KG_ERR_ARG, "min_train_pairs must be >= 0");
    return KG_OK;
}

// Lg of rule 5, for 1 <= x < 2^63: 256 * floor(log2 x) and eight more bits by repeated squaring
int32_t coding_lg(uint64_t x)
{
    const uint32_t n = 63u - (uint32_t)__builtin_clzll(x);
    unsigned __int128 y = x << (63u - n);               // 2^63 <= y < 2^64
    uint32_t f = 0;
    for (int k = 0; k < 8; k++) {
        y = (y * y) >> 63;
        if (y >> 64) { y >>= 1; f = 2 * f + 1; } else f = 2 * f;
    }
    return (int32_t)(256u * n + f);
}

// rule 5: the counts -> T[4096]
int coding_table_of(const kg_coding_model *m, int32_t *T)
{
    uint64_t sum[2] = {0, 0};
    for (int which = 0; which < 2; which++) {
        const int64_t *c = which ? m->background : m->coding;
        for (int h = 0; h < kg::kCodingBins; h++) {
            if (c[h] < 0) return fail(KG_ERR_ARG, std::string(which ? "background" : "coding") + " count " + kmer_text(h) + " is negative");
            sum[which] += (uint64_t)c[h];
            if (sum[which] >= (1ull << 62)) return fail(KG_ERR_ARG, std::string(which ? "background" : "coding") + " counts sum to 2^62 or more");
        }
    }
    const int32_t lg_sc = coding_lg(sum[0] + kg::kCodingBins), lg_sb = coding_lg(sum[1] + kg::kCodingBins);
    for (int h = 0; h < kg::kCodingBins; h++)
        T[h] = coding_lg((uint64_t)m->coding[h] + 1) - lg_sc - coding_lg((uint64_t)m->background[h] + 1) + lg_sb;
    return KG_OK;
}

// The passes of one call over d_orfs[n] (device records complete on t->stream), d_seq (the batch's bytes on the device, null
// when there are none) and offsets (host, checked).  begin(), then count() and / or score(), each followed by check() -- the
// wait that reads the error and counter words -- before anything of theirs is used on the host.
struct CodingWork {
    kg_table *t;
    Scratch sc;
    const kg_orf *d_orfs = nullptr;
    uint64_t n = 0, n_seqs = 0, total = 0;
    const uint8_t *d_seq = nullptr;
    int64_t *d_off = nullptr;
    unsigned long long *words = nullptr, *err = nullptr, *cnt = nullptr;
    uint32_t *lens = nullptr, *excl = nullptr;
    uint64_t *partial = nullptr, *d_pairs = nullptr;
    uint32_t pair_grid = 1;

    explicit CodingWork(kg_table *tt) : t(tt), sc(tt) {}

    int begin(const kg_orf *orfs, uint64_t n_orfs, const uint8_t *seq, const int64_t *offsets, uint64_t ns, uint64_t bytes, int64_t l_max)
    {
        d_orfs = orfs; n = n_orfs; d_seq = seq; n_seqs = ns; total = bytes;
        hipStream_t s = t->stream;
        int rc;
        if ((rc = sc.get(&d_off, n_seqs + 1)) || (rc = sc.get(&words, 16)) || (rc = sc.get(&lens, std::max<uint64_t>(n, 1))) ||
            (rc = sc.get(&excl, std::max<uint64_t>(n, 1))) || (rc = sc.get(&partial, n / kg::kScanChunk + 2)))
            return rc;
        err = words;
        cnt = words + kg::kCodingErrWords;
        d_pairs = (uint64_t *)(cnt + kg::kCodingCntPairs);
        HIP_TRY(hipMemcpyAsync(d_off, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(err, 0x7F, kg::kCodingErrWords * 8, s));
        HIP_TRY(hipMemsetAsync(cnt, 0, kg::kCodingCntWords * 8, s));
        if (n > 0) {
            hipLaunchKernelGGL(kg::coding_lens_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_orfs, n, d_off, n_seqs, lens, err, cnt);
            HIP_TRY(hipGetLastError());
            if ((rc = prefix_sum(t, lens, n, excl, partial, d_pairs))) return rc;
        }
        // a record has fewer than l_max / 3 pairs: enough workgroups for one lane per pair, up to the cap they stride with
        const uint64_t most = n * (uint64_t)std::max<int64_t>(l_max / 3, 1);
        pair_grid = (uint32_t)std::min<uint64_t>(kg::kCodingMaxGrid, std::max<uint64_t>(1, (most + kg::kCodingThreads - 1) / kg::kCodingThreads));
        return KG_OK;
    }
    // rules 3 and 4 into *m (host memory that lives until check() has returned)
    int count(kg_coding_model *m)
    {
        hipStream_t s = t->stream;
        unsigned long long *F = nullptr, *C = nullptr;
        int64_t *B = nullptr;
        int rc;
        if ((rc = sc.get(&F, kg::kCodingBins)) || (rc = sc.get(&C, kg::kCodingBins)) || (rc = sc.get(&B, kg::kCodingBins))) return rc;
        HIP_TRY(hipMemsetAsync(F, 0, kg::kCodingBins * 8, s));
        HIP_TRY(hipMemsetAsync(C, 0, kg::kCodingBins * 8, s));
        const uint64_t n_tiles = (total + kg::kCodingBgTile - 1) / kg::kCodingBgTile;
        if (n_tiles > 0)
            hipLaunchKernelGGL(kg::coding_background_kernel, dim3((uint32_t)std::min<uint64_t>(n_tiles, kg::kCodingMaxGrid)),
                               dim3(kg::kCodingThreads), 0, s, d_seq, total, d_off, n_seqs, n_tiles, F);
        hipLaunchKernelGGL(kg::coding_fold_kernel, dim3(kg::kCodingBins / kg::kCodingThreads), dim3(kg::kCodingThreads), 0, s, F, B);
        if (n > 0)
            hipLaunchKernelGGL(kg::coding_count_kernel, dim3(pair_grid), dim3(kg::kCodingThreads), 0, s, d_orfs, n, excl, d_pairs, d_seq,
                               total, d_off, C);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(m->coding, C, kg::kCodingBins * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(m->background, B, kg::kCodingBins * 8, hipMemcpyDeviceToHost, s));
        return KG_OK;
    }
    // rule 6 with T (host memory that lives until the stream has been waited for) into d_S[n]
    int score(const int32_t *T, int64_t *d_S)
    {
        hipStream_t s = t->stream;
        int32_t *d_T = nullptr;
        int rc;
        if ((rc = sc.get(&d_T, kg::kCodingBins))) return rc;
        HIP_TRY(hipMemcpyAsync(d_T, T, kg::kCodingBins * 4, hipMemcpyHostToDevice, s));
        if (n > 0) {
            HIP_TRY(hipMemsetAsync(d_S, 0, n * 8, s));
            hipLaunchKernelGGL(kg::coding_score_kernel, dim3(pair_grid), dim3(kg::kCodingThreads), 0, s, d_orfs, n, excl, d_pairs, d_seq,
                               total, d_off, d_T, d_S);
            HIP_TRY(hipGetLastError());
        }
        return KG_OK;
    }
    int check()
    {
        static const char *const what[kg::kCodingErrWords] = {
            ": seq outside [0, n_seqs)", ": strand is neither 0 nor 1", ": outside its contig (0 <= left <= right <= L - 1 does not hold)",
            ": 3 * n_res exceeds right - left + 1"};
        int rc;
        if ((rc = read_record_errors(t, words, kg::kCodingErrWords + kg::kCodingCntWords, kg::kCodingErrWords, what))) return rc;
        if (counter(kg::kCodingCntPairs) >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more codon pairs in one call");
        return KG_OK;
    }
    uint64_t counter(int k) const { return t->h_pin[kPinStage + kg::kCodingErrWords + k]; }
};

constexpr const char *kNoScores = "the set has no scores (it is not from kg_orfset_coding)";

int64_t coding_sum(const int64_t *c)
{
    int64_t s = 0;
    for (int h = 0; h < kg::kCodingBins; h++) s += c[h];
    return s;
}

// the checks the two caller-held entry points share; *total = the batch's bytes, *l_max = the longest contig
int check_coding_lists(const kg_orf *orfs, int64_t n, const uint8_t *seq, const int64_t *offsets, int64_t n_seqs, uint64_t *total,
                       int64_t *l_max)
{
    if (n < 0) return fail(KG_ERR_ARG, "n < 0");
    if (n >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more records in one call");
    if (n && !orfs) return fail(KG_ERR_ARG, "null ORF records");
    int rc = check_orf_batch(seq, offsets, n_seqs, total);
    if (rc) return rc;
    if (*total >= (1ull << 40)) return fail(KG_ERR_LIMIT, "2^40 or more bytes in one call");
    return check_region_offsets(offsets, n_seqs, l_max);
}

// the caller's records and bytes into the call's scratch
int coding_upload(kg_table *t, Scratch &sc, const kg_orf *orfs, uint64_t n, const uint8_t *seq, uint64_t total, kg_orf **d_orfs, uint8_t **d_seq)
{
    int rc;
    if ((rc = sc.get(d_orfs, n ? n : 1)) || (rc = sc.get(d_seq, total ? total : 1))) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(*d_orfs, orfs, n * sizeof(kg_orf), hipMemcpyHostToDevice, t->stream));
    if (total && (rc = upload_batch(t, seq, total, *d_seq))) return rc;
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_coding_table(const kg_coding_model *model, int32_t *table)
{
    if (!model || !table) return fail(KG_ERR_ARG, "null argument");
    return coding_table_of(model, table);
}

int kg_orfset_coding(kg_orfset *os, const kg_coding_params *p, const int32_t *table, const uint8_t *seq, int seq_on_device,
                     const int64_t *offsets, int64_t n_seqs, kg_orfset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!os) return fail(KG_ERR_ARG, "null kg_orfset");
    int rc = check_coding_params(p);
    if (rc) return rc;
    uint64_t total = 0;
    if ((rc = check_orf_batch(seq, offsets, n_seqs, &total, "ORF set's", os->n_seqs))) return rc;
    if (total >= (1ull << 40)) return fail(KG_ERR_LIMIT, "2^40 or more bytes in one call");
    if (os->count >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more records in one call");
    std::vector<int32_t> own_table;     // (in front of the scratch, whose destructor waits for the stream that copies it)
    Events<4> ev;                       // the counting passes begin, end; the scores begin, end
    CallScope cs(os->tab, "a kg_scan* is in flight on this ORF set's kg_table");
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    hipStream_t s = t->stream;
    std::unique_ptr<kg_orfset> set;
    if ((rc = make_set(cs, set)) || (rc = inherit(set.get(), os))) return rc;
    set->coding_model.reset(new (std::nothrow) kg_coding_model());
    if (!set->coding_model) return fail(KG_ERR_NOMEM, "out of host memory");
    if ((rc = ev.create())) return rc;
    CodingWork w(t);
    const uint8_t *d_seq = nullptr;
    if ((rc = batch_on_device(t, w.sc, seq, seq_on_device, total, &d_seq))) return rc;
    const uint64_t n = (uint64_t)os->count, n_res = (uint64_t)os->residues;
    kg_orf *d_out = nullptr;
    int64_t *d_start = nullptr, *d_S = nullptr;
    uint8_t *d_res = nullptr;
    if ((rc = w.sc.get(&d_out, std::max<uint64_t>(n, 1))) || (rc = w.sc.get(&d_start, n + 1)) ||
        (rc = w.sc.get(&d_res, std::max<uint64_t>(n_res, 1))) || (rc = w.sc.get(&d_S, std::max<uint64_t>(n, 1))))
        return rc;
    HIP_TRY(hipEventRecord(ev[0], s));
    if ((rc = w.begin(os->d_orfs, n, d_seq, offsets, (uint64_t)n_seqs, total, os->l_max))) return rc;
    kg_coding_stats st = {};
    st.scored = (int64_t)n;
    st.trained = 2;
    if (!table) {
        // the wait in the middle: the counts come down, T is made on the host and goes up
        if ((rc = w.count(set->coding_model.get()))) return rc;
        HIP_TRY(hipEventRecord(ev[1], s));
        if ((rc = w.check())) return rc;
        st.training_pairs = coding_sum(set->coding_model->coding);
        st.background = coding_sum(set->coding_model->background);
        st.trained = st.training_pairs >= p->min_train_pairs ? 1 : 0;
        if (st.trained) {
            own_table.resize(kg::kCodingBins);
            if ((rc = coding_table_of(set->coding_model.get(), own_table.data()))) return rc;
            table = own_table.data();
        }
    } else {
        HIP_TRY(hipEventRecord(ev[1], s));
    }
    HIP_TRY(hipEventRecord(ev[2], s));
    if (n > 0) {
        if (!st.trained) HIP_TRY(hipMemsetAsync(d_S, 0, n * 8, s));     // (all scores are 0)
        HIP_TRY(hipMemcpyAsync(d_out, os->d_orfs, n * sizeof(kg_orf), hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(d_start, os->d_prot_start, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
    if (n_res > 0) HIP_TRY(hipMemcpyAsync(d_res, os->d_res, n_res, hipMemcpyDeviceToDevice, s));
    if (st.trained) {
        if ((rc = w.score(table, d_S))) return rc;
        if (n > 0) {
            hipLaunchKernelGGL(kg::coding_decide_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_out, n, d_S, p->min_coding, w.cnt);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(ev[3], s));
    if ((rc = w.check())) return rc;
    st.training_records = (int64_t)w.counter(kg::kCodingCntTrain);
    st.noncoding = (int64_t)w.counter(kg::kCodingCntNoncoding);
    st.ms_count = ev.ms(0, 1);
    st.ms_score = ev.ms(2, 3);
    keep_orfs(set.get(), w.sc, d_out, d_start, d_res, n, n_res, (uint64_t)n_seqs);
    set->d_coding = set->keep(w.sc, d_S);
    set->coding_st = st;
    return hand_out(cs, set, out);
}

int kg_orfset_coding_scores(const kg_orfset *s, int64_t first, int64_t count, int64_t *dst)
{
    if (int rc = need_of_set(s, count <= 0 || dst, s && s->d_coding, "kg_orfset_coding_scores", kNoScores)) return rc;
    return copy_records(s, device_of(s), s->d_coding, 1, s->count, first, count, dst, "kg_orfset_coding_scores");
}

int kg_orfset_coding_stats(const kg_orfset *s, kg_coding_stats *out)
{
    if (int rc = need_of_set(s, out, s && s->d_coding, "kg_orfset_coding_stats", kNoScores)) return rc;
    *out = s->coding_st;
    return KG_OK;
}

int kg_orfset_coding_model(const kg_orfset *s, kg_coding_model *out)
{
    if (int rc = need_of_set(s, out, s && s->d_coding && s->coding_model, "kg_orfset_coding_model", kNoScores)) return rc;
    *out = *s->coding_model;
    return KG_OK;
}

int kg_coding_counts_orfs(int device, const kg_orf *orfs, int64_t n, const uint8_t *seq, const int64_t *offsets, int64_t n_seqs,
                          kg_coding_model *out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    uint64_t total = 0;
    int64_t l_max = 0;
    int rc = check_coding_lists(orfs, n, seq, offsets, n_seqs, &total, &l_max);
    if (rc) return rc;
    // (in front of the scratch, whose destructor waits for the stream that copies into it)
    std::unique_ptr<kg_coding_model> m(new (std::nothrow) kg_coding_model());
    if (!m) return fail(KG_ERR_NOMEM, "out of host memory");
    CallScope cs(device);               // the call's context: closed when the call returns
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    CodingWork w(t);
    kg_orf *d_orfs = nullptr;
    uint8_t *d_seq = nullptr;
    if ((rc = coding_upload(t, w.sc, orfs, (uint64_t)n, seq, total, &d_orfs, &d_seq))) return rc;
    if ((rc = w.begin(d_orfs, (uint64_t)n, d_seq, offsets, (uint64_t)n_seqs, total, l_max))) return rc;
    if ((rc = w.count(m.get())) || (rc = w.check())) return rc;
    *out = *m;
    return KG_OK;
}

int kg_coding_score_orfs(int device, const int32_t *table, const kg_orf *orfs, int64_t n, const uint8_t *seq, const int64_t *offsets,
                         int64_t n_seqs, int64_t *scores)
{
    if (!table || (n > 0 && !scores)) return fail(KG_ERR_ARG, "null argument");
    uint64_t total = 0;
    int64_t l_max = 0;
    int rc = check_coding_lists(orfs, n, seq, offsets, n_seqs, &total, &l_max);
    if (rc) return rc;
    CallScope cs(device);               // the call's context: closed when the call returns
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    CodingWork w(t);
    kg_orf *d_orfs = nullptr;
    uint8_t *d_seq = nullptr;
    int64_t *d_S = nullptr;
    if ((rc = coding_upload(t, w.sc, orfs, (uint64_t)n, seq, total, &d_orfs, &d_seq))) return rc;
    if ((rc = w.sc.get(&d_S, n ? (size_t)n : 1))) return rc;
    if ((rc = w.begin(d_orfs, (uint64_t)n, d_seq, offsets, (uint64_t)n_seqs, total, l_max))) return rc;
    if ((rc = w.score(table, d_S)) || (rc = w.check())) return rc;
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(scores, d_S, (size_t)n * 8, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
    }
    return KG_OK;
}

}  // extern "C"
