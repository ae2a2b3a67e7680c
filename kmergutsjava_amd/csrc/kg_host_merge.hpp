// kg_host_merge.hpp -- kg_table_merge_signatures / kg_table_merge_signatures_device: a resident table united with new
// signatures -> a signature set in k-mer order (kernels: kg_merge.hpp).
// Part of kmerguts_hip.hip's translation unit: one of the batch stages, included behind the kernel headers, kg_host.hpp and the
// hosts of the table, the result and the scan; behind kg_host_derive.hpp, whose kg_sigset it fills.
#pragma once

namespace {

// Everything between the argument checks and the set.  Scratch comes from the base table's block cache (KG_TEST_FAIL_ALLOC
// applies) and is back in it when this returns; the set's array leaves the cache for good.
int merge_impl(kg_table *t, int policy, const uint8_t *h_sigs, const uint8_t *d_sigs, uint64_t n, const int32_t *fn_map, uint64_t n_fn,
               const int32_t *otu_map, uint64_t n_otu, kg_sigset *set)
{
    const uint64_t records = t->limit, cap = std::min(t->occupied, records);
    Scratch sc(t);
    int rc;
    if (h_sigs && n) {
        uint8_t *d = nullptr;
        if ((rc = sc.get(&d, n * 24))) return rc;
        if ((rc = upload_pinned(t, h_sigs, n * 24, d))) return rc;
        d_sigs = d;
    }
    int32_t *d_fn = nullptr, *d_otu = nullptr;
    if (fn_map) {
        if ((rc = sc.get(&d_fn, std::max<uint64_t>(n_fn, 1)))) return rc;
        if (n_fn) HIP_TRY(hipMemcpyAsync(d_fn, fn_map, n_fn * 4, hipMemcpyHostToDevice, t->stream));
    }
    if (otu_map) {
        if ((rc = sc.get(&d_otu, std::max<uint64_t>(n_otu, 1)))) return rc;
        if (n_otu) HIP_TRY(hipMemcpyAsync(d_otu, otu_map, n_otu * 4, hipMemcpyHostToDevice, t->stream));
    }
    Events<4> ev;
    if ((rc = ev.create())) return rc;
    unsigned long long *d_cnt = nullptr;
    if ((rc = sc.get(&d_cnt, kg::kMrgWords))) return rc;
    HIP_TRY(hipMemsetAsync(d_cnt, 0xFF, kg::kMrgErrWords * 8, t->stream));
    HIP_TRY(hipMemsetAsync(d_cnt + kg::kMrgErrWords, 0, (kg::kMrgWords - kg::kMrgErrWords) * 8, t->stream));
    HIP_TRY(hipEventRecord(ev[0], t->stream));
    // the pairs: the new ones at [0, n), the base's behind them
    SortPairs sp;
    if (cap + n) {
        if ((rc = sp.alloc(sc, cap + n))) return rc;
    }
    if (n) {
        const uint64_t want = (n + kg::kBuildThreads - 1) / kg::kBuildThreads;
        hipLaunchKernelGGL(kg::merge_new_keys_kernel, dim3((uint32_t)std::min<uint64_t>(want, 256ull * 32)), dim3(kg::kBuildThreads), 0,
                           t->stream, d_sigs, n, d_fn != nullptr, n_fn, d_otu != nullptr, n_otu, sp.keys(), sp.vals(), d_cnt);
        HIP_TRY(hipGetLastError());
    }
    if (records && cap) {
        hipLaunchKernelGGL(kg::merge_extract_kernel, dim3((uint32_t)((records + kg::kBuildTile - 1) / kg::kBuildTile)),
                           dim3(kg::kBuildThreads), 0, t->stream, t->d_entries, records, n, cap, sp.keys(), sp.vals(), d_cnt);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[1], t->stream));
    unsigned long long cnt[kg::kMrgWords];
    HIP_TRY(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    if (cnt[kg::kMrgOverflow])
        return fail(KG_ERR_DEVICE, "kg_table_merge_signatures: the table holds more records than when it was opened (internal error)");
    const uint64_t n_base = cnt[kg::kMrgCursor], n_pairs = n_base + n;
    if (n_pairs >= (1ull << 32))
        return fail(KG_ERR_LIMIT, "kg_table_merge_signatures: 2^32 or more signatures (the table's and the new ones) in one call");
    if (const unsigned long long bad = cnt[kg::kMrgBadKmer]; bad != ~0ull) {
        int64_t kmer = 0;
        if (h_sigs) memcpy(&kmer, h_sigs + bad * 24, 8);
        else HIP_TRY(hipMemcpy(&kmer, d_sigs + bad * 24, 8, hipMemcpyDeviceToHost));
        return fail(KG_ERR_ARG, "signature " + kmer_text((int64_t)bad) + ": k-mer " + kmer_text(kmer) +
                                    " is outside [0, 20^8) (the smallest such input index)");
    }
    for (int which = 0; which < 2; which++) {
        const unsigned long long bad = cnt[which ? kg::kMrgBadOtu : kg::kMrgBadFn];
        if (bad == ~0ull) continue;
        int32_t v = 0;
        const size_t at = bad * 24 + (which ? 8 : 16);
        if (h_sigs) memcpy(&v, h_sigs + at, 4);
        else HIP_TRY(hipMemcpy(&v, d_sigs + at, 4, hipMemcpyDeviceToHost));
        return fail(KG_ERR_ARG, "signature " + kmer_text((int64_t)bad) + (which ? ": otu_index " : ": function_index ") + kmer_text(v) +
                                    " is outside [0, " + kmer_text((int64_t)(which ? n_otu : n_fn)) + ") of the " +
                                    (which ? "OTU" : "function") + " map (the smallest such input index)");
    }
    if ((rc = sp.sort(t, sc, n_pairs, kg::kMergeKeyBits))) return rc;
    HIP_TRY(hipEventRecord(ev[2], t->stream));
    // the flags and the ranks lie in the sort's free side when a sort ran
    uint32_t *flag = sp.v[sp.cur ^ 1], *rank = (uint32_t *)sp.k[sp.cur ^ 1];
    uint64_t *partial = nullptr;
    const uint64_t nb = std::max<uint64_t>(1, (n_pairs + kg::kScanChunk - 1) / kg::kScanChunk);
    if (n_pairs && !flag && ((rc = sc.get(&flag, n_pairs)) || (rc = sc.get(&rank, n_pairs)))) return rc;
    if ((rc = sc.get(&partial, nb + 2))) return rc;
    uint64_t n_out = 0;
    if (n_pairs) {
        hipLaunchKernelGGL(kg::merge_resolve_kernel, dim3(grid_of(n_pairs, kg::kBuildThreads)), dim3(kg::kBuildThreads), 0, t->stream,
                           sp.keys(), sp.vals(), n_pairs, policy, t->d_entries, records, d_sigs, n, d_fn, n_fn, flag, d_cnt);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, flag, n_pairs, rank, partial, partial + nb + 1))) return rc;
        HIP_TRY(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipMemcpyAsync(&n_out, partial + nb + 1, 8, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        if (cnt[kg::kMrgDupNew] != ~0ull)
            return fail(KG_ERR_ARG, "duplicate k-mer " + kmer_text((int64_t)cnt[kg::kMrgDupNew]) +
                                        " among the new signatures (the smallest k-mer that occurs more than once)");
        if (cnt[kg::kMrgDupBase] != ~0ull)
            return fail(KG_ERR_ARG, "duplicate k-mer " + kmer_text((int64_t)cnt[kg::kMrgDupBase]) +
                                        " in the table (the smallest k-mer that occurs more than once)");
        if (n_out) {
            if ((rc = dalloc_detached(t, &set->d_sigs, n_out * 24))) return rc;
            hipLaunchKernelGGL(kg::merge_emit_kernel, dim3(grid_of(n_pairs, kg::kBuildThreads)), dim3(kg::kBuildThreads), 0, t->stream,
                               sp.keys(), sp.vals(), flag, rank, n_pairs, t->d_entries, records, d_sigs, n, d_fn, n_fn, d_otu, n_otu,
                               set->d_sigs, n_out);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(ev[3], t->stream));
    HIP_TRY(hipEventSynchronize(ev[3]));
    kg_merge_stats &st = set->mst;
    st.base = (int64_t)n_base;
    st.base_ignored = (int64_t)cnt[kg::kMrgIgnored];
    st.added_in = (int64_t)n;
    st.added = (int64_t)cnt[kg::kMrgAdded];
    st.conflicts = (int64_t)cnt[kg::kMrgConflicts];
    st.conflicts_same_function = (int64_t)cnt[kg::kMrgSame];
    st.replaced = policy == KG_MERGE_REPLACE ? st.conflicts : 0;
    st.dropped = policy == KG_MERGE_DROP ? st.conflicts - st.conflicts_same_function : 0;
    st.merged = (int64_t)n_out;
    st.ms_extract = ev.ms(0, 1);
    st.ms_sort = ev.ms(1, 2);
    st.ms_resolve = ev.ms(2, 3);
    st.ms_total = ev.ms(0, 3);
    set->count = (int64_t)n_out;
    set->st.signatures = (int64_t)n_out;
    set->merged = true;
    return KG_OK;
}

int merge_entry(kg_table *base, const kg_merge_params *p, const uint8_t *h_sigs, const uint8_t *d_sigs, int64_t n, const int32_t *fn_map,
                int64_t n_fn, const int32_t *otu_map, int64_t n_otu, kg_sigset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!base) return fail(KG_ERR_ARG, "null table");
    if (!p) return fail(KG_ERR_ARG, "null kg_merge_params");
    if (p->on_conflict < KG_MERGE_KEEP || p->on_conflict > KG_MERGE_DROP)
        return fail(KG_ERR_ARG, "on_conflict must be KG_MERGE_KEEP, KG_MERGE_REPLACE or KG_MERGE_DROP");
    if (p->reserved != 0) return fail(KG_ERR_ARG, "kg_merge_params.reserved must be 0");
    if (n < 0) return fail(KG_ERR_ARG, "n < 0");
    if (n > 0 && !h_sigs && !d_sigs) return fail(KG_ERR_ARG, "null signature array");
    if ((fn_map && n_fn < 0) || (otu_map && n_otu < 0)) return fail(KG_ERR_ARG, "a map with a negative length");
    if (d_sigs && ((uintptr_t)d_sigs & 7))
        return fail(KG_ERR_ARG, "kg_table_merge_signatures_device: the signatures must be 8-byte aligned");
    CallScope cs(base, "a kg_scan* is in flight on this kg_table");
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    if (t->limit >= (1ull << 32)) return fail(KG_ERR_LIMIT, "kg_table_merge_signatures: a table of 2^32 or more records");
    if ((uint64_t)n >= (1ull << 32))
        return fail(KG_ERR_LIMIT, "kg_table_merge_signatures: 2^32 or more signatures (the table's and the new ones) in one call");
    std::unique_ptr<kg_sigset, void (*)(kg_sigset *)> set(new (std::nothrow) kg_sigset(), kg_sigset_free);
    if (!set) return fail(KG_ERR_NOMEM, "out of host memory");
    set->device = t->device;
    // a device input may still be written by another (blocking or non-blocking) stream
    int rc = d_sigs && hipDeviceSynchronize() != hipSuccess ? fail(KG_ERR_DEVICE, "hipDeviceSynchronize failed") : KG_OK;
    if (!rc) rc = merge_impl(t, p->on_conflict, h_sigs, d_sigs, (uint64_t)n, fn_map, (uint64_t)n_fn, otu_map, (uint64_t)n_otu, set.get());
    t->cache.release_free();                            // the merge's scratch goes back to the driver, not to the table's cache
    if (rc) { const std::string keep = g_err; set.reset(); g_err = keep; return rc; }
    if (getenv("KG_DEBUG")) {
        const kg_merge_stats &st = set->mst;
        fprintf(stderr, "[kg] kg_table_merge_signatures: base=%lld ignored=%lld new=%lld added=%lld conflicts=%lld same=%lld merged=%lld "
                        "extract_ms=%.3f sort_ms=%.3f resolve_ms=%.3f total_ms=%.3f\n",
                (long long)st.base, (long long)st.base_ignored, (long long)st.added_in, (long long)st.added, (long long)st.conflicts,
                (long long)st.conflicts_same_function, (long long)st.merged, st.ms_extract, st.ms_sort, st.ms_resolve, st.ms_total);
    }
    *out = set.release();
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_table_merge_signatures(kg_table *base, const kg_merge_params *p, const kg_signature *sigs, int64_t n, const int32_t *fn_map,
                              int64_t n_fn, const int32_t *otu_map, int64_t n_otu, kg_sigset **out)
{
    return merge_entry(base, p, (const uint8_t *)sigs, nullptr, n, fn_map, n_fn, otu_map, n_otu, out);
}

int kg_table_merge_signatures_device(kg_table *base, const kg_merge_params *p, const kg_signature *d_sigs, int64_t n, const int32_t *fn_map,
                                     int64_t n_fn, const int32_t *otu_map, int64_t n_otu, kg_sigset **out)
{
    return merge_entry(base, p, nullptr, (const uint8_t *)d_sigs, n, fn_map, n_fn, otu_map, n_otu, out);
}

int kg_sigset_merge_stats(const kg_sigset *s, kg_merge_stats *out)
{
    if (!s || !out) return fail(KG_ERR_ARG, "null argument");
    if (!s->merged) return fail(KG_ERR_ARG, "kg_sigset_merge_stats: the set was derived, not merged");
    *out = s->mst;
    return KG_OK;
}

}  // extern "C"
