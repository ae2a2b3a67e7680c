// kg_host_result.hpp -- what a caller does with a kg_result: kg_result_free, the lazy pinned host views behind the kg_result_*
// accessors, kg_result_copy_hits, kg_result_progress, the device pointers, and kg_restore_hits_device (kernel: kg_device.hpp,
// restore_hits_kernel).
// Part of kmerguts_hip.hip's translation unit: behind kg_host_table.hpp.
#pragma once

namespace {

template <typename T>
const T *host_view(kg_result *r, void *&slot, const T *d, size_t n)
{
    if (slot) return (const T *)slot;
    if (!d && n) { g_err = "record kind not computed (KG_F_SKIP_AGGREGATE?)"; return nullptr; }
    if (hipSetDevice(r->tab->device) != hipSuccess) { g_err = "hipSetDevice failed"; return nullptr; }
    void *h = nullptr;
    if (r->tab->pins.get(&h, n ? n * sizeof(T) : 64) != hipSuccess) { g_err = "pinned host allocation failed"; return nullptr; }
    if (n && hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) {
        r->tab->pins.put(h);
        g_err = "device to host copy failed";
        return nullptr;
    }
    slot = h;
    return (const T *)h;
}

}  // namespace

extern "C" {

void kg_result_free(kg_result *r)
{
    if (!r) return;
    kg_table *t = r->tab;
    if (t) {
        // a result is only handed out after its scan has synchronised the stream
        dfree(t, r->d_hits); dfree(t, r->d_chs); dfree(t, r->d_calls); dfree(t, r->d_ccs); dfree(t, r->d_otu);
        dfree(t, r->d_ev); dfree(t, r->d_tail_ev); dfree(t, r->d_hit_slots);
    }
    for (void *h : {r->h_hits, r->h_chs, r->h_ccs, r->h_calls, r->h_otu, r->h_ev, r->h_tail_ev, r->h_hit_slots})
        if (h) { if (t) t->pins.put(h); else (void)hipHostFree(h); }
    if (t && r->own_tab) kg_table_close(t);
    delete r;
}

int kg_result_stats(const kg_result *r, kg_stats *out)
{
    if (!r || !out) return fail(KG_ERR_ARG, "null argument");
    *out = r->st;
    return KG_OK;
}

const kg_hit *kg_result_hits(kg_result *r)
{
    return r ? host_view(r, r->h_hits, r->d_hits, (size_t)r->st.n_hits) : nullptr;
}
const int64_t *kg_result_container_hit_start(kg_result *r)
{
    return r ? host_view(r, r->h_chs, r->d_chs, (size_t)r->st.n_containers + 1) : nullptr;
}
const kg_call *kg_result_calls(kg_result *r)
{
    return r ? host_view(r, r->h_calls, r->d_calls, (size_t)r->st.n_calls) : nullptr;
}
const int64_t *kg_result_container_call_start(kg_result *r)
{
    if (!r) return nullptr;
    if (!r->d_ccs) { g_err = "calls not computed (KG_F_SKIP_AGGREGATE)"; return nullptr; }
    return host_view(r, r->h_ccs, r->d_ccs, (size_t)r->st.n_containers + 1);
}
const kg_otu *kg_result_otu(kg_result *r)
{
    if (!r) return nullptr;
    if (!r->d_otu) { g_err = "OTU votes not computed (KG_F_SKIP_AGGREGATE)"; return nullptr; }
    return host_view(r, r->h_otu, r->d_otu, (size_t)r->st.n_seqs);
}
const uint8_t *kg_result_hit_events(kg_result *r)
{
    if (!r) return nullptr;
    if (!r->d_ev) { g_err = "events not computed (KG_F_SKIP_AGGREGATE)"; return nullptr; }
    return host_view(r, r->h_ev, r->d_ev, (size_t)r->st.n_hits);
}
const uint8_t *kg_result_container_tail_events(kg_result *r)
{
    if (!r) return nullptr;
    if (!r->d_tail_ev) { g_err = "events not computed (KG_F_SKIP_AGGREGATE)"; return nullptr; }
    return host_view(r, r->h_tail_ev, r->d_tail_ev, (size_t)r->st.n_containers);
}
const uint32_t *kg_result_hit_slots(kg_result *r)
{
    if (!r || !r->has_progress) { g_err = "hit slots are recorded by KG_F_PROGRESS scans only"; return nullptr; }
    return host_view<uint32_t>(r, r->h_hit_slots, r->d_hit_slots, (size_t)r->st.n_hits);
}

int kg_result_progress(const kg_result *r, kg_progress *out)
{
    if (!r || !out) return fail(KG_ERR_ARG, "null argument");
    if (!r->has_progress) return fail(KG_ERR_ARG, "not a KG_F_PROGRESS scan");
    *out = r->progress;
    return KG_OK;
}

int kg_result_copy_hits(kg_result *r, int64_t first, int64_t count, kg_hit *dst)
{
    if (!r || first < 0 || count < 0 || first + count > r->st.n_hits) return fail(KG_ERR_ARG, "hit range out of bounds");
    if (count == 0) return KG_OK;
    if (!dst) return fail(KG_ERR_ARG, "null destination");
    HIP_TRY(hipSetDevice(r->tab->device));
    // pageable destinations go through the table's two cached pinned blocks, 64 MiB at a time: the device-to-host copy
    // of piece k+1 runs while piece k is moved into the caller's memory
    hipPointerAttribute_t attr;
    const bool pinned_dst = hipPointerGetAttributes(&attr, dst) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    if (pinned_dst) {
        HIP_TRY(hipMemcpy(dst, r->d_hits + first, (size_t)count * sizeof(kg_hit), hipMemcpyDeviceToHost));
        return KG_OK;
    }
    const size_t piece = (64u << 20) / sizeof(kg_hit);
    void *stage[2] = {nullptr, nullptr};
    for (auto &st : stage)
        if (r->tab->pins.get(&st, piece * sizeof(kg_hit)) != hipSuccess) {
            if (stage[0]) r->tab->pins.put(stage[0]);
            return fail(KG_ERR_NOMEM, "pinned staging allocation failed");
        }
    hipStream_t s = r->tab->stream;
    hipEvent_t done[2] = {r->tab->ev[kEvSpare], r->tab->ev[kEvBegin]};      // idle outside a scan
    int rc = KG_OK;
    int64_t sent = 0, got = 0;
    int which = 0;
    auto issue = [&](int w) {
        const int64_t n = std::min<int64_t>((int64_t)piece, count - sent);
        hipError_t e = hipMemcpyAsync(stage[w], r->d_hits + first + sent, (size_t)n * sizeof(kg_hit), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventRecord(done[w], s);
        if (e != hipSuccess) rc = fail(KG_ERR_DEVICE, std::string("device to host copy failed: ") + hipGetErrorString(e));
        sent += n;
    };
    issue(0);
    while (rc == KG_OK && got < count) {
        if (sent < count) issue(which ^ 1);
        if (rc != KG_OK) break;
        if (hipEventSynchronize(done[which]) != hipSuccess) { rc = fail(KG_ERR_DEVICE, "device to host copy failed"); break; }
        const int64_t n = std::min<int64_t>((int64_t)piece, count - got);
        memcpy(dst + got, stage[which], (size_t)n * sizeof(kg_hit));
        got += n;
        which ^= 1;
    }
    (void)hipStreamSynchronize(s);
    r->tab->pins.put(stage[0]); r->tab->pins.put(stage[1]);
    return rc;
}

int kg_restore_hits_device(int device, const kg_hit *d_src, int64_t n_hits, const int64_t *d_seq_first, int64_t n_seqs,
                           const int64_t *d_dst_first, const int32_t *d_container_shift, kg_hit *d_dst, void *stream)
{
    if (n_hits < 0 || n_seqs < 0) return fail(KG_ERR_ARG, "negative count");
    if (n_hits == 0) return KG_OK;
    if (!d_src || !d_seq_first || !d_dst_first || !d_container_shift || !d_dst || n_seqs == 0) return fail(KG_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(device));
    const uint32_t grid = (uint32_t)std::min<int64_t>((n_hits + 1023) / 1024, 256 * 16);
    hipLaunchKernelGGL(kg::restore_hits_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_src, (uint64_t)n_hits, d_seq_first,
                       (uint64_t)n_seqs, d_dst_first, d_container_shift, d_dst);
    HIP_TRY(hipGetLastError());
    return KG_OK;
}

const void *kg_result_device_hits(const kg_result *r) { return r ? r->d_hits : nullptr; }
const void *kg_result_device_calls(const kg_result *r) { return r ? r->d_calls : nullptr; }
const void *kg_result_device_otu(const kg_result *r) { return r ? r->d_otu : nullptr; }
const void *kg_result_device_container_hit_start(const kg_result *r) { return r ? r->d_chs : nullptr; }
const void *kg_result_device_container_call_start(const kg_result *r) { return r ? r->d_ccs : nullptr; }

}  // extern "C"
