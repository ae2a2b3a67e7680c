// kg_host_assign.hpp -- kg_result_assign / kg_assign_calls: the CALL records of an -a scan -> one kg_assignment per protein
// (kernels: kg_assign.hpp).
// Part of kmerguts_hip.hip's translation unit: one of the batch stages, included behind the kernel headers, kg_host.hpp and the
// hosts of the table, the result and the scan.
#pragma once

namespace {

int check_assign_params(const kg_assign_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_assign_params");
    if (p->min_score < 0) return fail(KG_ERR_ARG, "min_score must be >= 0");
    if (p->min_share_pct < 0 || p->min_share_pct > 100) return fail(KG_ERR_ARG, "min_share_pct must be in 0..100");
    return KG_OK;
}

// d_calls[n_calls], d_cs[n_prot + 1], d_otu[n_prot] (or null): device arrays complete on t->stream.  Writes dst (host or device).
int assign_impl(kg_table *t, const kg_assign_params *prm, const kg_call *d_calls, uint64_t n_calls, const int64_t *d_cs,
                uint64_t n_prot, const kg_otu *d_otu, kg_assignment *dst, float *ms)
{
    if (ms) *ms = 0;
    if (n_prot == 0) return KG_OK;
    hipPointerAttribute_t attr;
    const bool dev_dst = hipPointerGetAttributes(&attr, dst) == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == t->device;
    (void)hipGetLastError();
    Scratch sc(t);
    int rc;
    kg_assignment *d_out = dev_dst ? dst : nullptr;
    uint32_t *flag = nullptr, *len = nullptr, *rank = nullptr, *base = nullptr;
    uint64_t *partial = nullptr, *totals = nullptr;
    unsigned long long *err = nullptr;
    const uint64_t nb = n_prot / kg::kScanChunk + 2;
    if ((!dev_dst && (rc = sc.get(&d_out, n_prot))) || (rc = sc.get(&flag, n_prot)) || (rc = sc.get(&len, n_prot)) ||
        (rc = sc.get(&rank, n_prot)) || (rc = sc.get(&base, n_prot)) || (rc = sc.get(&partial, nb)) || (rc = sc.get(&totals, 4)) ||
        (rc = sc.get(&err, 4)))
        return rc;
    hipStream_t s = t->stream;
    HIP_TRY(hipMemsetAsync(err, 0x7F, 4 * 8, s));
    HIP_TRY(hipEventRecord(t->ev[kEvStageBegin], s));
    hipLaunchKernelGGL(kg::assign_short_kernel, dim3(grid_of(n_prot)), dim3(256), 0, s, d_calls, n_calls, d_cs, n_prot, d_otu,
                       prm->min_score, prm->min_share_pct, d_out, flag, len, err);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, flag, n_prot, rank, partial, totals))) return rc;
    if ((rc = prefix_sum(t, len, n_prot, base, partial, totals + 1))) return rc;
    HIP_TRY(hipMemcpyAsync(t->h_pin + kPinAssign, totals, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t n_long = t->h_pin[kPinAssign], n_items = t->h_pin[kPinAssign + 1];
    if (n_long > 0) {
        uint32_t *ids = nullptr, *lbase = nullptr;
        SortPairs sp;
        int64_t *run_s = nullptr;
        float *run_w = nullptr;
        if ((rc = sc.get(&ids, n_long)) || (rc = sc.get(&lbase, n_long)) || (rc = sp.alloc(sc, n_items)) ||
            (rc = sc.get(&run_s, n_items)) || (rc = sc.get(&run_w, n_items)))
            return rc;
        hipLaunchKernelGGL(kg::assign_long_scatter_kernel, dim3(grid_of(n_prot)), dim3(256), 0, s, flag, rank, base, n_prot, ids, lbase);
        const uint32_t wgrid = (uint32_t)std::min<uint64_t>((n_long + 3) / 4, 256ull * 64);
        hipLaunchKernelGGL(kg::assign_long_keys_kernel, dim3(wgrid), dim3(256), 0, s, d_calls, n_calls, d_cs, ids, lbase,
                           (uint32_t)n_long, sp.keys(), sp.vals(), err);
        HIP_TRY(hipGetLastError());
        if ((rc = sp.sort(t, sc, n_items, 32 + bits_for(n_long)))) return rc;        // (a long protein has more than kAssignShort items)
        hipLaunchKernelGGL(kg::assign_long_runs_kernel, dim3(grid_of(n_items)), dim3(256), 0, s, sp.keys(), sp.vals(), n_items, d_calls,
                           run_s, run_w);
        hipLaunchKernelGGL(kg::assign_long_reduce_kernel, dim3(wgrid), dim3(256), 0, s, sp.keys(), run_s, run_w, d_calls, n_calls,
                           d_cs, d_otu, ids, lbase, (uint32_t)n_long, prm->min_score, prm->min_share_pct, d_out, err);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(t->ev[kEvStageEnd], s));
    if ((rc = read_error_words(t, err, 3, kPinAssign + 2,         // (in the order they are reported)
                               {{kg::kAssignErrOrder, KG_ERR_ARG, "protein ", ": call_start decreases (call_start[p+1] < call_start[p])"},
                                {kg::kAssignErrCount, KG_ERR_ARG, "protein ", ": a CALL has a negative count"},
                                {kg::kAssignErrLimit, KG_ERR_LIMIT, "protein ", ": S_best or T is 2^31 or more"}})))
        return rc;
    if (ms) HIP_TRY(hipEventElapsedTime(ms, t->ev[kEvStageBegin], t->ev[kEvStageEnd]));
    if (!dev_dst) HIP_TRY(hipMemcpy(dst, d_out, n_prot * sizeof(kg_assignment), hipMemcpyDefault));
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_result_assign(kg_result *r, const kg_assign_params *p, kg_assignment *dst, float *ms)
{
    if (ms) *ms = 0;
    if (!r) return fail(KG_ERR_ARG, "null kg_result");
    int rc = check_assign_params(p);
    if (rc) return rc;
    if (!r->d_ccs || !r->d_otu) return fail(KG_ERR_ARG, "a KG_F_SKIP_AGGREGATE result has no CALL records to assign from");
    if (r->per != 1 || r->st.n_containers != r->st.n_seqs)
        return fail(KG_ERR_ARG, "a DNA result: assignment needs an -a (protein) scan, one container per sequence");
    if (r->st.n_seqs > 0 && !dst) return fail(KG_ERR_ARG, "null destination");
    CallScope cs(r->tab, "a kg_scan* is in flight on this result's kg_table");
    if (cs.rc) return cs.rc;
    return assign_impl(cs.t, p, r->d_calls, (uint64_t)r->st.n_calls, r->d_ccs, (uint64_t)r->st.n_seqs, r->d_otu, dst, ms);
}

int kg_assign_calls(int device, const kg_assign_params *p, const kg_call *calls, const int64_t *call_start, int64_t n_prot,
                    const kg_otu *otu, kg_assignment *dst)
{
    int rc = check_assign_params(p);
    if (rc) return rc;
    if (n_prot < 0 || !call_start) return fail(KG_ERR_ARG, "null call_start or n_prot < 0");
    if (n_prot >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more proteins in one call");
    if (n_prot > 0 && !dst) return fail(KG_ERR_ARG, "null destination");
    if (call_start[0] < 0) return fail(KG_ERR_ARG, "protein 0: call_start[0] < 0");
    const uint64_t n_calls = call_start[n_prot] > 0 ? (uint64_t)call_start[n_prot] : 0;
    if (n_calls >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more CALL records in one call");
    if (n_calls && !calls) return fail(KG_ERR_ARG, "null CALL records");
    if (n_prot == 0) return KG_OK;
    CallScope cs(device);               // the call's context: closed when the call returns, after its scratch is back
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    Scratch sc(t);
    kg_call *d_calls = nullptr;
    int64_t *d_cs = nullptr;
    kg_otu *d_otu = nullptr;
    if ((rc = sc.get(&d_calls, n_calls ? n_calls : 1)) || (rc = sc.get(&d_cs, (size_t)n_prot + 1)) ||
        (otu && (rc = sc.get(&d_otu, (size_t)n_prot))))
        return rc;
    if (n_calls) HIP_TRY(hipMemcpyAsync(d_calls, calls, n_calls * sizeof(kg_call), hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(d_cs, call_start, ((size_t)n_prot + 1) * 8, hipMemcpyHostToDevice, t->stream));
    if (otu) HIP_TRY(hipMemcpyAsync(d_otu, otu, (size_t)n_prot * sizeof(kg_otu), hipMemcpyHostToDevice, t->stream));
    return assign_impl(t, p, d_calls, n_calls, d_cs, (uint64_t)n_prot, d_otu, dst, nullptr);
}

}  // extern "C"
