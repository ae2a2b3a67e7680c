// kg_host_select.hpp -- kg_regionset_select / kg_orfset_select / kg_select_intervals: the non-overlapping selection among
// regions, ORFs or a caller's intervals (kernels: kg_select.hpp).
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_regions.hpp and kg_host_orfs.hpp (it reads
// kg_regionset and kg_orfset).
#pragma once

struct kg_selectset : SetBase {
    kg_selection *d_sel = nullptr;      // count records, index-aligned with the candidates
    int64_t count = 0;
    kg_select_stats st = {};
};

static_assert(kg::kSelectWords <= kPinStageWords, "stage words must fit their pinned words");
static_assert(sizeof(kg_selection) == 8 && sizeof(kg_interval) == 20, "record layouts of include/kmerguts_hip.h");

namespace {

int check_select_params(const kg_select_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_select_params");
    if (p->max_overlap < 0) return fail(KG_ERR_ARG, "max_overlap must be >= 0");
    if (p->max_overlap_pct < 0 || p->max_overlap_pct > 100) return fail(KG_ERR_ARG, "max_overlap_pct must be 0..100");
    if (p->reserved != 0) return fail(KG_ERR_ARG, "kg_select_params.reserved must be 0");
    return KG_OK;
}

// d_in[n]: device records complete on t->stream (kg_region, kg_orf or kg_interval); sorted: they are in (seq, left) order
// already.  left_bits: every valid left is below 2^left_bits.  Fills set (its array comes out of the cache with the call's
// scratch and is kept only on success).
template <typename T>
int select_impl(kg_table *t, const kg_select_params *prm, const T *d_in, uint64_t n, uint64_t n_seqs, uint32_t left_bits, bool sorted,
                kg_selectset *set)
{
    Scratch sc(t);
    hipStream_t s = t->stream;
    int rc;
    unsigned long long *words = nullptr;
    kg_selection *d_out = nullptr;
    if ((rc = sc.get(&words, 16)) || (rc = sc.get(&d_out, std::max<uint64_t>(n, 1)))) return rc;
    HIP_TRY(hipMemsetAsync(words, 0x7F, 8, s));
    HIP_TRY(hipMemsetAsync(words + 1, 0, (kg::kSelectWords - 1) * 8, s));
    HIP_TRY(hipEventRecord(t->ev[kEvStageBegin], s));
    const uint64_t *h = t->h_pin + kPinStage;
    uint64_t E = 0, P = 0;
    uint32_t rounds = 0;
    if (n > 0) {
        SortPairs ord;
        uint32_t *flag = nullptr, *pos = nullptr, *count = nullptr, *pair_start = nullptr;
        uint64_t *partial = nullptr;
        kg::SelectCols c = {};
        if ((rc = ord.alloc(sc, n))) return rc;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(kg::select_keys_kernel<T>), dim3(grid_of(n)), dim3(256), 0, s, d_in, n, n_seqs, left_bits,
                           ord.keys(), ord.vals(), words);
        HIP_TRY(hipGetLastError());
        if (!sorted && (rc = ord.sort(t, sc, n, left_bits + bits_for(n_seqs)))) return rc;
        if ((rc = sc.get(&flag, n)) || (rc = sc.get(&pos, n)) || (rc = sc.get(&count, n)) || (rc = sc.get(&pair_start, n)) ||
            (rc = sc.get(&partial, n / kg::kScanChunk + 2)) || (rc = sc.get(&c.key, n)) || (rc = sc.get(&c.right, n)) ||
            (rc = sc.get(&c.score, n)) || (rc = sc.get(&c.orig, n)))
            return rc;
        uint64_t *d_E = (uint64_t *)(words + kg::kSelectEligible);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(kg::select_flags_kernel<T>), dim3(grid_of(n)), dim3(256), 0, s, d_in, n, n_seqs, ord.vals(), flag);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, flag, n, pos, partial, d_E))) return rc;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(kg::select_compact_kernel<T>), dim3(grid_of(n)), dim3(256), 0, s, d_in, n, ord.keys(), ord.vals(),
                           flag, pos, c);
        hipLaunchKernelGGL(kg::select_count_kernel, dim3(grid_of(n)), dim3(256), 0, s, c.key, c.right, d_E, n, left_bits, count, words);
        HIP_TRY(hipGetLastError());
        // (the scan's total is exact and equals P, the count kernel's own 64-bit sum, which the limit check reads; pair_start is
        // the prefix modulo 2^32 and is used only when P < 2^31, where it is exact)
        if ((rc = prefix_sum(t, count, n, pair_start, partial, (uint64_t *)(words + kg::kSelectScanTotal)))) return rc;
        // the one wait before the rounds: the error word, the eligible candidates and the overlapping pairs
        if ((rc = read_error_words(t, words, kg::kSelectWords, kPinStage,
                                   {{kg::kSelectErr, KG_ERR_ARG, "candidate ", ": seq outside [0, n_seqs), left < 0 or right < left"}})))
            return rc;
        E = h[kg::kSelectEligible];
        P = h[kg::kSelectPairs];
        if (P >= (1ull << 31)) return fail(KG_ERR_LIMIT, "2^31 or more overlapping pairs of candidates in one call");
        uint2 *pairs = nullptr;
        uint32_t *state = nullptr, *blocked = nullptr, *by = nullptr;
        if ((rc = sc.get(&pairs, std::max<uint64_t>(P, 1))) || (rc = sc.get(&state, std::max<uint64_t>(E, 1))) ||
            (rc = sc.get(&blocked, std::max<uint64_t>(E, 1))) || (rc = sc.get(&by, std::max<uint64_t>(E, 1))))
            return rc;
        if (E > 0) {
            HIP_TRY(hipMemsetAsync(state, 0, E * 4, s));
            HIP_TRY(hipMemsetAsync(blocked, 0, E * 4, s));
            HIP_TRY(hipMemsetAsync(by, 0xFF, E * 4, s));
        }
        if (P > 0) {
            const uint64_t lanes = (P + kg::kSelectPairsPerLane - 1) / kg::kSelectPairsPerLane;
            hipLaunchKernelGGL(kg::select_expand_kernel, dim3(grid_of(lanes)), dim3(256), 0, s, c, pair_start, E, P, left_bits,
                               (int64_t)prm->max_overlap, (int64_t)prm->max_overlap_pct, pairs, words);
            HIP_TRY(hipGetLastError());
        }
        // kSelectRoundsPerRead rounds per read of the undecided counts; the rounds behind the last decision change nothing
        unsigned long long *und = words + kg::kSelectUndecided;
        for (bool done = E == 0; !done;) {
            HIP_TRY(hipMemsetAsync(und, 0, kg::kSelectRoundsPerRead * 8, s));
            for (int k = 0; k < kg::kSelectRoundsPerRead; k++) {
                const uint32_t r = rounds + 1 + (uint32_t)k;
                if (P > 0) hipLaunchKernelGGL(kg::select_edge_kernel, dim3(grid_of(P)), dim3(256), 0, s, pairs, P, state, blocked, r);
                hipLaunchKernelGGL(kg::select_node_kernel, dim3(grid_of(E)), dim3(256), 0, s, state, blocked, E, r, und + k);
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(t->h_pin + kPinStage + kg::kSelectUndecided, und, kg::kSelectRoundsPerRead * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            int k = 0;
            while (k < kg::kSelectRoundsPerRead && h[kg::kSelectUndecided + k] != 0) k++;
            done = k < kg::kSelectRoundsPerRead;
            rounds += done ? (uint32_t)k + 1 : (uint32_t)kg::kSelectRoundsPerRead;
        }
        if (P > 0) hipLaunchKernelGGL(kg::select_by_kernel, dim3(grid_of(P)), dim3(256), 0, s, pairs, P, state, c.orig, by);
        hipLaunchKernelGGL(kg::select_emit_kernel, dim3(grid_of(n)), dim3(256), 0, s, ord.vals(), flag, pos, n, state, by, d_out, words);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(t->ev[kEvStageEnd], s));
    HIP_TRY(hipMemcpyAsync(t->h_pin + kPinStage, words, kg::kSelectWords * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    set->st.candidates = (int64_t)n;
    set->st.eligible = (int64_t)E;
    set->st.selected = (int64_t)h[kg::kSelectSelected];
    set->st.overlapped = (int64_t)h[kg::kSelectOverlapped];
    set->st.pairs = (int64_t)P;
    set->st.conflicts = (int64_t)h[kg::kSelectConflicts];
    set->st.rounds = (int32_t)rounds;
    HIP_TRY(hipEventElapsedTime(&set->st.ms, t->ev[kEvStageBegin], t->ev[kEvStageEnd]));
    set->d_sel = set->keep(sc, d_out);  // the set's array leaves the scratch: everything else goes back to the cache
    set->count = (int64_t)n;
    return KG_OK;
}

// the two calls on a set of the library's: the set's context is borrowed, its records stay where they are
template <typename T>
int select_of_set(kg_table *tab, const kg_select_params *p, const T *d_in, int64_t count, int64_t n_seqs, uint32_t left_bits, bool sorted,
                  const char *busy_text, kg_selectset **out)
{
    int rc = check_select_params(p);
    if (rc) return rc;
    if (count >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more candidates in one call");
    CallScope cs(tab, busy_text);
    if (cs.rc) return cs.rc;
    std::unique_ptr<kg_selectset> set;
    if ((rc = make_set(cs, set))) return rc;
    if ((rc = select_impl(cs.t, p, d_in, (uint64_t)count, (uint64_t)n_seqs, left_bits, sorted, set.get()))) return rc;
    return hand_out(cs, set, out);
}

}  // namespace

extern "C" {

int kg_regionset_select(kg_regionset *rs, const kg_select_params *p, kg_selectset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!rs) return fail(KG_ERR_ARG, "null kg_regionset");
    // a region set is in (seq, left) order by rule 5 of the regions: no sort, and the key only has to hold any left (a contig
    // has fewer than 2^31 nucleotides, check_region_offsets)
    return select_of_set(rs->tab, p, rs->d_regions, rs->count, rs->n_seqs, 31, true, "a kg_scan* is in flight on this region set's kg_table",
                         out);
}

int kg_orfset_select(kg_orfset *os, const kg_select_params *p, kg_selectset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!os) return fail(KG_ERR_ARG, "null kg_orfset");
    // the sort key's width from the longest contig, as the regions' sorts take theirs
    const uint32_t left_bits = std::max(1u, bits_for((uint64_t)std::max<int64_t>(os->l_max, 1)));
    return select_of_set(os->tab, p, os->d_orfs, os->count, os->n_seqs, left_bits, false, "a kg_scan* is in flight on this ORF set's kg_table",
                         out);
}

int kg_select_intervals(int device, const kg_select_params *p, const kg_interval *iv, int64_t n, int64_t n_seqs, kg_selectset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = check_select_params(p);
    if (rc) return rc;
    if (n < 0) return fail(KG_ERR_ARG, "n < 0");
    if (n_seqs < 0) return fail(KG_ERR_ARG, "n_seqs < 0");
    if (n >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more candidates in one call");
    if (n_seqs >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more contigs in one call");
    if (n && !iv) return fail(KG_ERR_ARG, "null interval records");
    int32_t left_max = 0;               // the sort key's width (the kernels validate)
    for (int64_t i = 0; i < n; i++) left_max = std::max(left_max, iv[i].left);
    CallScope cs(device);               // the call's context: closed on every failure below, kept by the set on success
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    std::unique_ptr<kg_selectset> set;
    if ((rc = make_set(cs, set))) return rc;
    {
        Scratch sc(t);
        kg_interval *d_iv = nullptr;
        if ((rc = sc.get(&d_iv, n ? (size_t)n : 1))) return rc;
        if (n) HIP_TRY(hipMemcpyAsync(d_iv, iv, (size_t)n * sizeof(kg_interval), hipMemcpyHostToDevice, t->stream));
        if ((rc = select_impl(t, p, d_iv, (uint64_t)n, (uint64_t)n_seqs, std::max(1u, bit_width((uint64_t)left_max)), false, set.get())))
            return rc;
    }
    return hand_out(cs, set, out);
}

int64_t kg_selectset_count(const kg_selectset *s) { return s ? s->count : 0; }

const kg_selection *kg_selectset_device(const kg_selectset *s) { return s ? s->d_sel : nullptr; }

int kg_selectset_copy(const kg_selectset *s, int64_t first, int64_t count, kg_selection *dst)
{
    return copy_records(s, device_of(s), s ? s->d_sel : nullptr, 1, s ? s->count : 0, first, count, dst, "kg_selectset_copy");
}

int kg_selectset_stats(const kg_selectset *s, kg_select_stats *out) { return copy_stats(s, s ? &s->st : nullptr, out); }

void kg_selectset_free(kg_selectset *s) { delete s; }

}  // extern "C"
