// kg_host_regions.hpp -- kg_result_regions / kg_regions_calls: the CALL records of a DNA scan -> function regions on the contigs
// (kernels: kg_regions.hpp).
// Part of kmerguts_hip.hip's translation unit: one of the batch stages, included behind the kernel headers, kg_host.hpp and the
// hosts of the table, the result and the scan.
#pragma once

struct kg_regionset : SetBase {
    kg_region *d_regions = nullptr;     // count records, output order
    int64_t *d_seq_start = nullptr;     // n_seqs + 1
    int64_t count = 0, n_seqs = 0;
    kg_region_stats st = {};
};

static_assert(kg::kRegionErrWords + 2 <= kPinStageWords, "stage words must fit their pinned words");

namespace {

int check_region_params(const kg_region_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_region_params");
    if (p->merge_gap < 0) return fail(KG_ERR_ARG, "merge_gap must be >= 0");
    if (p->min_score < 0) return fail(KG_ERR_ARG, "min_score must be >= 0");
    if (p->min_len < 0) return fail(KG_ERR_ARG, "min_len must be >= 0");
    return KG_OK;
}

// the host checks of offsets[n_seqs + 1]; *l_max = the longest contig
int check_region_offsets(const int64_t *offsets, int64_t n_seqs, int64_t *l_max)
{
    if (n_seqs < 0) return fail(KG_ERR_ARG, "n_seqs < 0");
    if (!offsets) return fail(KG_ERR_ARG, "null offsets");
    if (n_seqs >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more contigs in one call");
    *l_max = 0;
    for (int64_t k = 0; k < n_seqs; k++) {
        const int64_t L = offsets[k + 1] - offsets[k];
        if (L < 0) return fail(KG_ERR_ARG, "contig " + kmer_text(k) + ": offsets decrease (offsets[s+1] < offsets[s])");
        if (L >= (1ll << 31)) return fail(KG_ERR_LIMIT, "contig " + kmer_text(k) + ": 2^31 or more nucleotides");
        *l_max = std::max(*l_max, L);
    }
    return KG_OK;
}

// d_calls[n_calls]: device array complete on t->stream; offsets: host, checked.  Fills set (its arrays come out of the cache
// with the call's scratch and are kept only on success).
int regions_impl(kg_table *t, const kg_region_params *prm, const kg_call *d_calls, uint64_t n, const int64_t *offsets,
                 uint64_t n_seqs, int64_t l_max, kg_regionset *set)
{
    Scratch sc(t);
    hipStream_t s = t->stream;
    int rc;
    int64_t *d_off = nullptr, *d_start = nullptr;
    unsigned long long *words = nullptr;           // [0 .. kRegionErrWords): error words, then 2 counters, then 2 totals
    if ((rc = sc.get(&d_off, n_seqs + 1)) || (rc = sc.get(&d_start, n_seqs + 1)) || (rc = sc.get(&words, 16))) return rc;
    unsigned long long *err = words, *cnt = words + kg::kRegionErrWords;
    uint64_t *totals = (uint64_t *)(words + kg::kRegionErrWords + 2);
    HIP_TRY(hipMemcpyAsync(d_off, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(err, 0x7F, kg::kRegionErrWords * 8, s));
    HIP_TRY(hipMemsetAsync(cnt, 0, 4 * 8, s));
    HIP_TRY(hipEventRecord(t->ev[kEvStageBegin], s));
    uint64_t *h = t->h_pin + kPinStage;
    uint64_t n_groups = 0, n_regions = 0;
    kg_region *d_out = nullptr;
    const uint32_t left_bits = bits_for((uint64_t)std::max<int64_t>(l_max, 1));
    const uint64_t *region_keys = nullptr;         // the regions' final sort keys
    if (n > 0) {
        uint64_t *partial = nullptr;
        SortPairs byx0;
        if ((rc = byx0.alloc(sc, n))) return rc;
        hipLaunchKernelGGL(kg::region_keys_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_calls, n, d_off, n_seqs, byx0.keys(), byx0.vals(), err);
        HIP_TRY(hipGetLastError());
        if ((rc = byx0.sort(t, sc, n, left_bits))) return rc;
        // second sort: the group keys, in x0 order, into the buffer the first sort left free (or a new one)
        SortPairs grp = byx0.next();
        if (!grp.k[0] && (rc = sc.get(&grp.k[0], n))) return rc;
        hipLaunchKernelGGL(kg::region_group_keys_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_calls, n, n_seqs, grp.vals(), grp.keys());
        HIP_TRY(hipGetLastError());
        if ((rc = grp.sort(t, sc, n, 32 + bits_for(2 * n_seqs)))) return rc;
        const uint64_t *gkeys = grp.keys();
        const uint32_t *perm = grp.vals();
        uint32_t *sx0 = nullptr, *sx1 = nullptr, *ghead = nullptr, *gexcl = nullptr, *rhead = nullptr, *rexcl = nullptr, *rmax = nullptr;
        int32_t *scount = nullptr;
        float *sweight = nullptr;
        uint8_t *sframe = nullptr;
        int64_t *tile_max = nullptr, *tile_pre = nullptr;
        const uint32_t n_tiles = (uint32_t)((n + kg::kBuildTile - 1) / kg::kBuildTile);
        if ((rc = sc.get(&sx0, n)) || (rc = sc.get(&sx1, n)) || (rc = sc.get(&scount, n)) || (rc = sc.get(&sweight, n)) ||
            (rc = sc.get(&sframe, n)) || (rc = sc.get(&ghead, n)) || (rc = sc.get(&gexcl, n)) || (rc = sc.get(&rhead, n)) ||
            (rc = sc.get(&rexcl, n)) || (rc = sc.get(&rmax, n)) || (rc = sc.get(&tile_max, n_tiles)) ||
            (rc = sc.get(&tile_pre, n_tiles)) || (rc = sc.get(&partial, n / kg::kScanChunk + 2)))
            return rc;
        hipLaunchKernelGGL(kg::region_gather_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_calls, n, d_off, n_seqs, gkeys, perm, sx0, sx1,
                           scount, sweight, sframe, ghead);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, ghead, n, gexcl, partial, totals))) return rc;
        hipLaunchKernelGGL(kg::region_tile_max_kernel, dim3(n_tiles), dim3(kg::kBuildThreads), 0, s, ghead, gexcl, sx1, n, tile_max);
        hipLaunchKernelGGL(kg::build_tile_scan_kernel, dim3(1), dim3(kg::kBuildThreads), 0, s, tile_max, n_tiles, tile_pre);
        hipLaunchKernelGGL(kg::region_heads_kernel, dim3(n_tiles), dim3(kg::kBuildThreads), 0, s, ghead, gexcl, sx0, sx1, n, tile_pre,
                           (int64_t)prm->merge_gap, rhead, rmax);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, rhead, n, rexcl, partial, totals + 1))) return rc;
        HIP_TRY(hipMemcpyAsync(h, totals, 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        n_groups = h[0];
        n_regions = h[1];
        kg_region *unsorted = nullptr;
        uint64_t *k2 = nullptr;
        SortPairs byleft;
        if ((rc = sc.get(&d_out, n_regions)) || (rc = sc.get(&unsorted, n_regions)) || (rc = sc.get(&byleft.k[0], n_regions)) ||
            (rc = sc.get(&k2, n_regions)) || (rc = sc.get(&byleft.v[0], n_regions)))
            return rc;
        hipLaunchKernelGGL(kg::region_walk_kernel, dim3(grid_of(n)), dim3(256), 0, s, rhead, rexcl, rmax, sx0, scount, sweight, sframe,
                           gkeys, perm, n, d_off, prm->min_score, prm->min_len, left_bits, unsorted,
                           kg::RegionKeys{byleft.keys(), k2, byleft.vals()}, err);
        HIP_TRY(hipGetLastError());
        if ((rc = byleft.sort(t, sc, n_regions, 33 + left_bits))) return rc;
        SortPairs fin = byleft.next();
        if (!fin.k[0] && (rc = sc.get(&fin.k[0], n_regions))) return rc;
        hipLaunchKernelGGL(kg::region_rekey_kernel, dim3(grid_of(n_regions)), dim3(256), 0, s, k2, fin.vals(), n_regions, fin.keys());
        HIP_TRY(hipGetLastError());
        if ((rc = fin.sort(t, sc, n_regions, left_bits + bits_for(n_seqs)))) return rc;
        region_keys = fin.keys();
        hipLaunchKernelGGL(kg::region_emit_kernel, dim3(grid_of(n_regions)), dim3(256), 0, s, unsorted, fin.vals(), n_regions, d_out, cnt);
        HIP_TRY(hipGetLastError());
    } else if ((rc = sc.get(&d_out, 1))) {
        return rc;
    }
    hipLaunchKernelGGL(kg::region_seq_start_kernel, dim3(grid_of(n_seqs + 1)), dim3(256), 0, s, region_keys, n_regions, left_bits, n_seqs,
                       d_start);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t->ev[kEvStageEnd], s));
    if ((rc = read_error_words(t, words, kg::kRegionErrWords + 2, kPinStage,       // (in the order they are reported)
                               {{kg::kRegionErrContainer, KG_ERR_ARG, "CALL ", ": container >= 6 * n_seqs"},
                                {kg::kRegionErrOrder, KG_ERR_ARG, "CALL ", ": container below its predecessor's (calls[] must be in container order)"},
                                {kg::kRegionErrCount, KG_ERR_ARG, "CALL ", ": negative count"},
                                {kg::kRegionErrRange, KG_ERR_ARG, "CALL ", ": outside its contig (0 <= x0 <= x1 <= L - 1 does not hold)"},
                                {kg::kRegionErrLimit, KG_ERR_LIMIT, "the region of CALL ", " (its first_call): score or CALL count is 2^31 or more"}})))
        return rc;
    set->st.calls = (int64_t)n;
    set->st.groups = (int64_t)n_groups;
    set->st.regions = (int64_t)n_regions;
    set->st.kept = (int64_t)h[kg::kRegionErrWords + kg::kRegionCntKept];
    set->st.multi_frame = (int64_t)h[kg::kRegionErrWords + kg::kRegionCntMulti];
    HIP_TRY(hipEventElapsedTime(&set->st.ms, t->ev[kEvStageBegin], t->ev[kEvStageEnd]));
    // the two arrays of the set leave the scratch: everything else goes back to the cache
    set->d_regions = set->keep(sc, d_out);
    set->d_seq_start = set->keep(sc, d_start);
    set->count = (int64_t)n_regions;
    set->n_seqs = (int64_t)n_seqs;
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_result_regions(kg_result *r, const kg_region_params *p, const int64_t *offsets, kg_regionset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!r) return fail(KG_ERR_ARG, "null kg_result");
    int rc = check_region_params(p);
    if (rc) return rc;
    if (!r->d_ccs) return fail(KG_ERR_ARG, "a KG_F_SKIP_AGGREGATE result has no CALL records to merge");
    if (r->per != 6) return fail(KG_ERR_ARG, "a protein (-a) result: regions need a DNA scan, six containers per sequence");
    int64_t l_max = 0;
    if ((rc = check_region_offsets(offsets, r->st.n_seqs, &l_max))) return rc;
    if ((uint64_t)r->st.n_calls >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more CALL records in one call");
    CallScope cs(r->tab, "a kg_scan* is in flight on this result's kg_table");
    if (cs.rc) return cs.rc;
    std::unique_ptr<kg_regionset> set;
    if ((rc = make_set(cs, set))) return rc;
    if ((rc = regions_impl(cs.t, p, r->d_calls, (uint64_t)r->st.n_calls, offsets, (uint64_t)r->st.n_seqs, l_max, set.get()))) return rc;
    return hand_out(cs, set, out);
}

int kg_regions_calls(int device, const kg_region_params *p, const kg_call *calls, int64_t n_calls, const int64_t *offsets,
                     int64_t n_seqs, kg_regionset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = check_region_params(p);
    if (rc) return rc;
    if (n_calls < 0) return fail(KG_ERR_ARG, "n_calls < 0");
    if ((uint64_t)n_calls >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more CALL records in one call");
    if (n_calls && !calls) return fail(KG_ERR_ARG, "null CALL records");
    int64_t l_max = 0;
    if ((rc = check_region_offsets(offsets, n_seqs, &l_max))) return rc;
    if (n_calls && n_seqs == 0) return fail(KG_ERR_ARG, "CALL 0: container >= 6 * n_seqs");
    CallScope cs(device);               // the call's context: closed on every failure below, kept by the set on success
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    std::unique_ptr<kg_regionset> set;
    if ((rc = make_set(cs, set))) return rc;
    {
        Scratch sc(t);
        kg_call *d_calls = nullptr;
        if ((rc = sc.get(&d_calls, n_calls ? (size_t)n_calls : 1))) return rc;
        if (n_calls) HIP_TRY(hipMemcpyAsync(d_calls, calls, (size_t)n_calls * sizeof(kg_call), hipMemcpyHostToDevice, t->stream));
        if ((rc = regions_impl(t, p, d_calls, (uint64_t)n_calls, offsets, (uint64_t)n_seqs, l_max, set.get()))) return rc;
    }
    return hand_out(cs, set, out);
}

int64_t kg_regionset_count(const kg_regionset *s) { return s ? s->count : 0; }

const kg_region *kg_regionset_device(const kg_regionset *s) { return s ? s->d_regions : nullptr; }

int kg_regionset_copy(const kg_regionset *s, int64_t first, int64_t count, kg_region *dst)
{
    return copy_records(s, device_of(s), s ? s->d_regions : nullptr, 1, s ? s->count : 0, first, count, dst, "kg_regionset_copy");
}

int kg_regionset_seq_start(const kg_regionset *s, int64_t *dst)
{
    return copy_starts(s, device_of(s), s ? s->d_seq_start : nullptr, s ? s->n_seqs : 0, dst);
}

int kg_regionset_stats(const kg_regionset *s, kg_region_stats *out) { return copy_stats(s, s ? &s->st : nullptr, out); }

void kg_regionset_free(kg_regionset *s) { delete s; }

}  // extern "C"
