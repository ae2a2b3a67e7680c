// kg_host_repair.hpp -- kg_regionset_repair / kg_result_repair: the frames of every multi-frame region joined into one protein,
// and the junction list (kernels: kg_repair.hpp).
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_regions.hpp and kg_host_orfs.hpp (it reads both sets).
#pragma once

namespace {

// device words of a call: the error words, the counters, the two totals the second wait reads, then the totals of the first wait
enum : int { kRepairWResidues = kg::kRepairErrWords + kg::kRepairCntWords, kRepairWJunctions, kRepairWKept, kRepairWSegments, kRepairWCountSum,
             kRepairWRuns, kRepairWords };
static_assert(kg::kRepairErrWords + 1 <= kPinStageWords && kg::kRepairCntWords + 2 <= kPinStageWords,
              "stage words must fit their pinned words");

constexpr const char *kNotRepaired = "the set is not from kg_regionset_repair";

int check_repair_params(const kg_repair_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_repair_params");
    if (p->start_codons < 0 || p->start_codons > 7) return fail(KG_ERR_ARG, "start_codons must be a mask of 1 (ATG), 2 (GTG), 4 (TTG)");
    if (p->min_count < 0) return fail(KG_ERR_ARG, "min_count must be >= 0");
    if (p->max_junctions < 1 || p->max_junctions > kg::kRepairMaxJunctions) return fail(KG_ERR_ARG, "max_junctions must be between 1 and 8");
    if (p->reserved != 0) return fail(KG_ERR_ARG, "kg_repair_params.reserved must be 0");
    return KG_OK;
}

// rs, os: the region set and its index-aligned ORF set; d_calls[n]: device array complete on t->stream; d_seq, offsets as
// orfs_impl has them.  Fills set (its arrays come out of the cache with the call's scratch and are kept only on success).
int repair_impl(kg_table *t, const kg_repair_params *prm, const kg_regionset *rs, const kg_orfset *os, const kg_call *d_calls, uint64_t n,
                const uint8_t *d_seq, const int64_t *offsets, uint64_t n_seqs, kg_orfset *set)
{
    OrfPlanes pl;
    Scratch sc(t);
    hipStream_t s = t->stream;
    int rc;
    if ((rc = pl.plan(offsets, n_seqs))) return rc;
    const uint64_t nr = (uint64_t)rs->count, nr1 = std::max<uint64_t>(nr, 1), n1 = std::max<uint64_t>(n, 1);
    const kg_region *regions = rs->d_regions;
    unsigned long long *words = nullptr;
    kg_orf *d_out = nullptr;
    int64_t *d_start = nullptr, *d_jstart = nullptr;
    uint32_t *lens = nullptr, *excl = nullptr, *jcount = nullptr, *jexcl = nullptr, *reg_first = nullptr, *reg_last = nullptr;
    uint32_t *pos = nullptr, *head = nullptr, *hexcl = nullptr, *owner = nullptr, *run_start = nullptr, *run_region = nullptr;
    uint32_t *keep = nullptr, *kexcl = nullptr, *creg = nullptr, *cexcl = nullptr;
    uint64_t *partial = nullptr;
    if ((rc = pl.alloc_geometry(sc)) || (rc = sc.get(&words, (size_t)kRepairWords)) || (rc = pl.alloc_keys(sc)) || (rc = sc.get(&d_out, nr1)) ||
        (rc = sc.get(&d_start, nr + 1)) || (rc = sc.get(&d_jstart, nr + 1)) || (rc = sc.get(&lens, nr1)) || (rc = sc.get(&excl, nr1)) ||
        (rc = sc.get(&jcount, nr1)) || (rc = sc.get(&jexcl, nr1)) || (rc = sc.get(&reg_first, nr1)) || (rc = sc.get(&reg_last, nr1)) ||
        (rc = sc.get(&pos, n1)) || (rc = sc.get(&head, n1)) || (rc = sc.get(&hexcl, n1)) || (rc = sc.get(&owner, n1)) ||
        (rc = sc.get(&run_start, n + 1)) || (rc = sc.get(&run_region, n1)) || (rc = sc.get(&keep, n1)) || (rc = sc.get(&kexcl, n1)) ||
        (rc = sc.get(&creg, n1)) || (rc = sc.get(&cexcl, n1)) || (rc = sc.get(&partial, std::max(n, nr) / kg::kScanChunk + 2)))
        return rc;
    unsigned long long *err = words, *cnt = words + kg::kRepairErrWords;
    if ((rc = pl.upload(s, offsets))) return rc;
    HIP_TRY(hipMemsetAsync(err, 0x7F, kg::kRepairErrWords * 8, s));
    HIP_TRY(hipMemsetAsync(cnt, 0, (kRepairWords - kg::kRepairErrWords) * 8, s));
    HIP_TRY(hipEventRecord(t->ev[kEvStageBegin], s));
    const kg::OrfGeometry geo = pl.geometry();
    const uint32_t sc_mask = (uint32_t)prm->start_codons, max_j = (uint32_t)prm->max_junctions;
    if ((rc = pl.launch(s, d_seq, sc_mask))) return rc;
    // the new set starts as the given one: records, lengths (the zeros of only_kept too), no junction
    HIP_TRY(hipMemsetAsync(jcount, 0, nr1 * 4, s));
    HIP_TRY(hipMemsetAsync(reg_first, 0xFF, nr1 * 4, s));
    HIP_TRY(hipMemsetAsync(reg_last, 0xFF, nr1 * 4, s));
    HIP_TRY(hipMemsetAsync(head, 0, n1 * 4, s));
    HIP_TRY(hipMemsetAsync(owner, 0xFF, n1 * 4, s));
    if (nr > 0) {
        HIP_TRY(hipMemcpyAsync(d_out, os->d_orfs, nr * sizeof(kg_orf), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(kg::orf_lens_kernel, dim3(grid_of(nr)), dim3(256), 0, s, os->d_prot_start, nr, lens);
        HIP_TRY(hipGetLastError());
    }
    const uint64_t *gkeys = nullptr;
    const uint32_t *perm = nullptr;
    uint32_t *sx0 = nullptr, *sx1 = nullptr;
    uint8_t *sframe = nullptr;
    if (n > 0) {
        // the region stage's group order, by its own kernels: by x0, then by (sequence, strand, fI)
        SortPairs byx0;
        if ((rc = byx0.alloc(sc, n))) return rc;
        hipLaunchKernelGGL(kg::region_keys_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_calls, n, pl.d_off, n_seqs, byx0.keys(), byx0.vals(), err);
        HIP_TRY(hipGetLastError());
        if ((rc = byx0.sort(t, sc, n, bits_for((uint64_t)std::max<int64_t>(pl.l_max, 1))))) return rc;
        SortPairs grp = byx0.next();
        if (!grp.k[0] && (rc = sc.get(&grp.k[0], n))) return rc;
        hipLaunchKernelGGL(kg::region_group_keys_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_calls, n, n_seqs, grp.vals(), grp.keys());
        HIP_TRY(hipGetLastError());
        if ((rc = grp.sort(t, sc, n, 32 + bits_for(2 * n_seqs)))) return rc;
        gkeys = grp.keys();
        perm = grp.vals();
        int32_t *scount = nullptr;
        float *sweight = nullptr;
        uint32_t *ghead = nullptr;
        if ((rc = sc.get(&sx0, n)) || (rc = sc.get(&sx1, n)) || (rc = sc.get(&scount, n)) || (rc = sc.get(&sweight, n)) ||
            (rc = sc.get(&sframe, n)) || (rc = sc.get(&ghead, n)))
            return rc;
        hipLaunchKernelGGL(kg::region_gather_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_calls, n, pl.d_off, n_seqs, gkeys, perm, sx0, sx1,
                           scount, sweight, sframe, ghead);
        hipLaunchKernelGGL(kg::repair_inverse_kernel, dim3(grid_of(n)), dim3(256), 0, s, perm, n, pos);
        HIP_TRY(hipGetLastError());
        if (nr > 0) {
            hipLaunchKernelGGL(kg::repair_owner_kernel, dim3(grid_of(nr)), dim3(256), 0, s, regions, nr, n, n_seqs, pos, head, owner, err);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = prefix_sum(t, head, n, hexcl, partial, (uint64_t *)(words + kRepairWRuns)))) return rc;
        hipLaunchKernelGGL(kg::repair_runs_kernel, dim3(grid_of(n)), dim3(256), 0, s, head, hexcl, owner, n, run_start, run_region);
        hipLaunchKernelGGL(kg::repair_calls_kernel, dim3(grid_of(n)), dim3(256), 0, s, regions, nr, pl.d_off, gkeys, perm, sx0, sx1, scount, head,
                           hexcl, run_region, n, prm->min_count, keep, creg, err);
        HIP_TRY(hipGetLastError());
        // (region_gather_kernel has clamped the counts at 0).  The counts may add up to 2^32 or more, inside one chunk too, and no
        // limit is needed: repair_sums_kernel compares differences of cexcl, and of the total's low word, modulo 2^32 with the
        // low word of the region's score.  prefix_sum's d_out is the exact prefix modulo 2^32 whatever the total, and so is the
        // low word of its total: the check is the one exact 64-bit prefixes would give once reduced, and no chunk's sum can make a
        // foreign list pass it or a true one fail.
        if ((rc = prefix_sum(t, (const uint32_t *)scount, n, cexcl, partial, (uint64_t *)(words + kRepairWCountSum)))) return rc;
        if (nr > 0) {
            hipLaunchKernelGGL(kg::repair_sums_kernel, dim3(grid_of(nr)), dim3(256), 0, s, regions, nr, n, n_seqs, pos, owner, hexcl, run_start,
                               cexcl, (const uint64_t *)(words + kRepairWCountSum), err);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = prefix_sum(t, keep, n, kexcl, partial, (uint64_t *)(words + kRepairWKept)))) return rc;
    } else if (nr > 0) {
        // regions without a CALL list: every first_call lies outside it
        hipLaunchKernelGGL(kg::repair_owner_kernel, dim3(grid_of(nr)), dim3(256), 0, s, regions, nr, n, n_seqs, pos, head, owner, err);
        HIP_TRY(hipGetLastError());
    }
    // the first wait: the CALL list is the set's, and how many CALLs take part in a chain
    uint64_t *h = t->h_pin + kPinStage;
    HIP_TRY(hipMemcpyAsync(h + kg::kRepairErrWords, words + kRepairWKept, 8, hipMemcpyDeviceToHost, s));
    if ((rc = read_error_words(t, words, kg::kRepairErrWords, kPinStage,                 // (in the order they are reported)
                               {{kg::kRegionErrContainer, KG_ERR_ARG, "CALL ", ": container >= 6 * n_seqs"},
                                {kg::kRegionErrOrder, KG_ERR_ARG, "CALL ", ": container below its predecessor's (calls[] must be in container order)"},
                                {kg::kRegionErrCount, KG_ERR_ARG, "CALL ", ": negative count"},
                                {kg::kRegionErrRange, KG_ERR_ARG, "CALL ", ": outside its contig (0 <= x0 <= x1 <= L - 1 does not hold)"},
                                {kg::kRepairErrRegion, KG_ERR_ARG, "region ", ": seq, strand or first_call is not of this batch and CALL list"},
                                {kg::kRepairErrCall, KG_ERR_ARG, "CALL ", ": lies in no region of its group (the CALL list is not the region set's)"},
                                {kg::kRepairErrSums, KG_ERR_ARG, "region ",
                                 ": the CALLs inside it do not add up to its n_calls and score (the CALL list is not the region set's)"}})))
        return rc;
    const uint64_t nk = h[kg::kRepairErrWords];
    kg::RepairSegments S = {};
    if (nk > 0) {
        uint32_t *ireg = nullptr, *ix0 = nullptr, *ix1 = nullptr, *iframe = nullptr, *shead = nullptr, *sexcl = nullptr;
        if ((rc = sc.get(&ireg, nk)) || (rc = sc.get(&ix0, nk)) || (rc = sc.get(&ix1, nk)) || (rc = sc.get(&iframe, nk)) ||
            (rc = sc.get(&shead, nk)) || (rc = sc.get(&sexcl, nk)) || (rc = sc.get(&S.reg, nk)) || (rc = sc.get(&S.frame, nk)) ||
            (rc = sc.get(&S.A, nk)) || (rc = sc.get(&S.C, nk)) || (rc = sc.get(&S.J, nk)) || (rc = sc.get(&S.first_codon, nk)) ||
            (rc = sc.get(&S.len, nk)) || (rc = sc.get(&S.stop, nk)) || (rc = sc.get(&S.end_codon, nk)) || (rc = sc.get(&S.meta, nk)) ||
            (rc = sc.get(&S.res, nk)))
            return rc;
        HIP_TRY(hipMemsetAsync(S.C, 0, nk * 4, s));
        HIP_TRY(hipMemsetAsync(S.len, 0, nk * 4, s));
        hipLaunchKernelGGL(kg::repair_compact_kernel, dim3(grid_of(n)), dim3(256), 0, s, keep, kexcl, creg, sx0, sx1, sframe, n, ireg, ix0, ix1, iframe);
        hipLaunchKernelGGL(kg::repair_seg_heads_kernel, dim3(grid_of(nk)), dim3(256), 0, s, ireg, iframe, nk, shead);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, shead, nk, sexcl, partial, (uint64_t *)(words + kRepairWSegments)))) return rc;
        const uint64_t *d_ns = (const uint64_t *)(words + kRepairWSegments);
        hipLaunchKernelGGL(kg::repair_segments_kernel, dim3(grid_of(nk)), dim3(256), 0, s, ireg, ix0, ix1, iframe, shead, sexcl, nk, S, reg_first, reg_last);
        hipLaunchKernelGGL(kg::repair_junction_kernel, dim3(grid_of(nk)), dim3(256), 0, s, regions, d_seq, geo, pl.keys, d_ns, S, reg_first, reg_last, max_j);
        hipLaunchKernelGGL(kg::repair_parts_kernel, dim3(grid_of(nk)), dim3(256), 0, s, regions, d_seq, geo, pl.keys, d_ns, S, reg_first, reg_last, max_j,
                           sc_mask);
        HIP_TRY(hipGetLastError());
    }
    if (nr > 0) {
        hipLaunchKernelGGL(kg::repair_record_kernel, dim3(grid_of(nr)), dim3(256), 0, s, regions, nr, pl.d_off, S, reg_first, reg_last, max_j, d_out, lens,
                           jcount, cnt);
        HIP_TRY(hipGetLastError());
    }
    // where every protein and every record's junctions begin
    if ((rc = layout_proteins(t, lens, nr, excl, partial, (uint64_t *)(words + kRepairWResidues), d_start)) ||
        (rc = layout_proteins(t, jcount, nr, jexcl, partial, (uint64_t *)(words + kRepairWJunctions), d_jstart)))
        return rc;
    // the second wait: the residue and junction totals and the counters
    if ((rc = read_error_words(t, cnt, kg::kRepairCntWords + 2, kPinStage, {}))) return rc;
    const uint64_t n_res = h[kg::kRepairCntWords], n_junc = h[kg::kRepairCntWords + 1];
    if (n_res >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more residues in one call");
    uint8_t *d_res = nullptr;
    kg_junction *d_junc = nullptr;
    if ((rc = sc.get(&d_res, std::max<uint64_t>(n_res, 1))) || (rc = sc.get(&d_junc, std::max<uint64_t>(n_junc, 1)))) return rc;
    if (n_junc > 0) {
        hipLaunchKernelGGL(kg::repair_junction_records_kernel, dim3(grid_of(nk)), dim3(256), 0, s, d_out, pl.d_off,
                           (const uint64_t *)(words + kRepairWSegments), S, reg_first, reg_last, d_jstart, d_junc);
        HIP_TRY(hipGetLastError());
    }
    if (n_res > 0) {
        hipLaunchKernelGGL(kg::repair_residues_kernel, dim3(grid_of((n_res + kg::kOrfResPerLane - 1) / kg::kOrfResPerLane)), dim3(256), 0, s, d_out, nr,
                           d_start, n_res, os->d_prot_start, os->d_res, d_jstart, d_junc, d_seq, pl.d_off, d_res);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(t->ev[kEvStageEnd], s));
    HIP_TRY(hipStreamSynchronize(s));
    set->st = os->st;
    set->st.residues = (int64_t)n_res;
    set->st.complete -= (int64_t)h[kg::kRepairCntWasComplete];
    set->st.interrupted += (int64_t)h[kg::kRepairCntNewInterrupted];
    set->st.partial5 += (int64_t)h[kg::kRepairCntPartial5Up] - (int64_t)h[kg::kRepairCntPartial5Down];
    kg_repair_stats &st = set->repair_st;
    st.candidates = (int64_t)h[kg::kRepairCntCandidates];
    st.repaired = (int64_t)h[kg::kRepairCntRepaired];
    st.failed = (int64_t)h[kg::kRepairCntFailed];
    st.single = (int64_t)h[kg::kRepairCntSingle];
    st.skipped = (int64_t)h[kg::kRepairCntSkipped];
    st.junctions = (int64_t)n_junc;
    st.residues = (int64_t)h[kg::kRepairCntResidues];
    HIP_TRY(hipEventElapsedTime(&st.ms, t->ev[kEvStageBegin], t->ev[kEvStageEnd]));
    keep_orfs(set, sc, d_out, d_start, d_res, nr, n_res, n_seqs);
    set->d_junctions = set->keep(sc, d_junc);
    set->d_junction_start = set->keep(sc, d_jstart);
    set->junctions = (int64_t)n_junc;
    set->repaired = true;
    set->l_max = std::max(os->l_max, pl.l_max);
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_regionset_repair(kg_regionset *rs, kg_orfset *os, const kg_call *calls, int calls_on_device, int64_t n_calls,
                        const kg_repair_params *p, const uint8_t *seq, int seq_on_device, const int64_t *offsets, int64_t n_seqs,
                        kg_orfset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!rs) return fail(KG_ERR_ARG, "null kg_regionset");
    if (!os) return fail(KG_ERR_ARG, "null kg_orfset");
    int rc = check_repair_params(p);
    if (rc) return rc;
    if (n_calls < 0) return fail(KG_ERR_ARG, "n_calls < 0");
    if ((uint64_t)n_calls >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more CALL records in one call");
    if (n_calls && !calls) return fail(KG_ERR_ARG, "null CALL records");
    uint64_t total = 0;
    if ((rc = check_orf_batch(seq, offsets, n_seqs, &total, "region set's", rs->n_seqs))) return rc;
    if (n_calls && n_seqs == 0) return fail(KG_ERR_ARG, "CALL 0: container >= 6 * n_seqs");
    if (os->tab != rs->tab) return fail(KG_ERR_ARG, "the ORF set was not made from this region set (another context)");
    if (os->count != rs->count || os->n_seqs != rs->n_seqs)
        return fail(KG_ERR_ARG, "the ORF set is not index-aligned with the region set (repair runs before kg_orfset_add_free)");
    if (rs->count >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more regions in one call");
    CallScope cs(rs->tab, "a kg_scan* is in flight on this region set's kg_table");
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    std::unique_ptr<kg_orfset> set;
    if ((rc = make_set(cs, set))) return rc;
    Scratch sc(t);
    const uint8_t *d_seq = nullptr;
    if ((rc = batch_on_device(t, sc, seq, seq_on_device, total, &d_seq))) return rc;
    const kg_call *d_calls = calls;
    if (!calls_on_device) {
        kg_call *up = nullptr;
        if ((rc = sc.get(&up, n_calls ? (size_t)n_calls : 1))) return rc;
        if (n_calls) HIP_TRY(hipMemcpyAsync(up, calls, (size_t)n_calls * sizeof(kg_call), hipMemcpyHostToDevice, t->stream));
        d_calls = up;
    } else {
        HIP_TRY(hipDeviceSynchronize());            // the CALLs may have been produced on another stream
    }
    if ((rc = repair_impl(t, p, rs, os, d_calls, (uint64_t)n_calls, d_seq, offsets, (uint64_t)n_seqs, set.get()))) return rc;
    return hand_out(cs, set, out);
}

int kg_result_repair(kg_result *r, kg_regionset *rs, kg_orfset *os, const kg_repair_params *p, const uint8_t *seq, int seq_on_device,
                     const int64_t *offsets, int64_t n_seqs, kg_orfset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!r) return fail(KG_ERR_ARG, "null kg_result");
    if (!rs) return fail(KG_ERR_ARG, "null kg_regionset");
    if (!r->d_ccs) return fail(KG_ERR_ARG, "a KG_F_SKIP_AGGREGATE result has no CALL records");
    if (r->per != 6) return fail(KG_ERR_ARG, "a protein (-a) result: regions need a DNA scan, six containers per sequence");
    if (r->tab != rs->tab) return fail(KG_ERR_ARG, "the region set was not made from this result");
    return kg_regionset_repair(rs, os, r->d_calls, 1, r->st.n_calls, p, seq, seq_on_device, offsets, n_seqs, out);
}

int64_t kg_orfset_junctions_count(const kg_orfset *s) { return s ? s->junctions : 0; }

int kg_orfset_junctions_copy(const kg_orfset *s, int64_t first, int64_t count, kg_junction *dst)
{
    if (int rc = need_of_set(s, count <= 0 || dst, s && s->repaired, "kg_orfset_junctions_copy", kNotRepaired)) return rc;
    return copy_records(s, device_of(s), s->d_junctions, 1, s->junctions, first, count, dst, "kg_orfset_junctions_copy", "the list");
}

int kg_orfset_junctions_start(const kg_orfset *s, int64_t *dst)
{
    if (int rc = need_of_set(s, dst, s && s->repaired, "kg_orfset_junctions_start", kNotRepaired)) return rc;
    return copy_starts(s, device_of(s), s->d_junction_start, s->count, dst);
}

int kg_orfset_junctions_stats(const kg_orfset *s, kg_repair_stats *out)
{
    if (int rc = need_of_set(s, out, s && s->repaired, "kg_orfset_junctions_stats", kNotRepaired)) return rc;
    *out = s->repair_st;
    return KG_OK;
}

}  // extern "C"
