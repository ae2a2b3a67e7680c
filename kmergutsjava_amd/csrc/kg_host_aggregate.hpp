// kg_host_aggregate.hpp -- hit records -> CALL records, OTU votes and events: aggregate_stage (the last stage of a scan), and the
// calls that aggregate records the caller brings, kg_aggregate_hits and kg_process_set_of_hits (kernels: kg_aggregate.hpp).
// Part of kmerguts_hip.hip's translation unit: behind kg_host_plan.hpp (AggPlan), in front of kg_host_scan.hpp.
#pragma once

namespace {

// gatherHits / processSetOfHits / the OTU buffer (KGJ:385-524) over res->d_hits + res->d_chs: fills the CALL, OTU and event
// arrays of res.  d_partial: prefix-sum scratch for n_cont items, d_totals: the counter words (kTotCalls: the CALL total).
// otu_init (device, one record
// per sequence, or null): the oICounts buffers the sequences start with (kg_aggregate_hits; the scan starts them empty).
// Everything is enqueued on t->stream and nothing is waited for: calls[] is allocated for the most CALLs n_hits records can
// make (n_hits / minHits), so the host does not need the CALL total before the records are compacted; the total arrives in
// t->h_pin[kPinCalls] once the caller has synchronised the stream.  ag: the knobs, read by the caller (plan_aggregate).
int aggregate_stage(kg_table *t, const kg_params *p, kg_result *res, Scratch &sc, int64_t n_seqs, uint64_t n_cont, uint64_t n_hits,
                    uint32_t PER, uint64_t *d_partial, uint64_t *d_totals, const kg_otu *d_otu_init, bool allow_pieces, const AggPlan &ag)
{
    int rc;
    kg::AggParams ap;
    ap.min_hits = p->min_hits; ap.min_weighted_hits = p->min_weighted_hits;
    ap.max_gap = p->max_gap; ap.order_constraint = p->order_constraint ? 1 : 0;
    uint32_t *d_ccnt = nullptr, *d_coff = nullptr, *d_first = nullptr;
    kg_call *d_staged = nullptr;
    uint8_t *d_vote = nullptr;
    if ((rc = dalloc(t, (void **)&res->d_ev, n_hits))) return rc;
    if ((rc = dalloc(t, (void **)&res->d_tail_ev, n_cont))) return rc;
    uint8_t *d_acc = res->d_ev;
    if ((rc = sc.get(&d_ccnt, n_cont))) return rc;
    if ((rc = sc.get(&d_first, n_cont))) return rc;
    if ((rc = sc.get(&d_coff, n_cont))) return rc;
    if ((rc = sc.get(&d_vote, n_hits))) return rc;
    // a hit votes for at most one CALL and a CALL needs >= minHits voters: the CALLs of a unit (a container, or a piece of a
    // long one) that starts at record b and ends before record e fit in [b / minHits, e / minHits) of the staging array
    if ((rc = sc.get(&d_staged, (size_t)(n_hits / (uint64_t)p->min_hits + 1)))) return rc;
    if ((rc = dalloc(t, (void **)&res->d_ccs, (n_cont + 1) * 8))) return rc;
    if ((rc = dalloc(t, (void **)&res->d_otu, (size_t)(n_seqs ? n_seqs : 1) * sizeof(kg_otu)))) return rc;
    // Long containers in pieces that start behind a gap > maxGap (kg_aggregate.hpp): exact when no -O (with it the gap
    // is measured from the last ACCEPTED record) and position + maxGap cannot wrap (the caller vouches for positions
    // < 2^30).
    const bool pieces = allow_pieces && !p->order_constraint && p->max_gap >= 0 && p->max_gap < (1 << 30) && n_cont &&
                        n_hits > (2ull << ag.pshift) && ag.pieces_on;
    const uint32_t n_pblocks = pieces ? (uint32_t)((n_hits + (1ull << ag.pshift) - 1) >> ag.pshift) : 0u;
    uint32_t *d_pstart = nullptr, *d_pcnt = nullptr;
    uint8_t *d_before = nullptr, *d_ppair = nullptr;
    t->h_pin[kPinCalls] = 0;
    t->h_pin[kPinPieces] = 0;
    if (pieces) {
        if ((rc = sc.get(&d_pstart, (size_t)n_pblocks + 1))) return rc;
        if ((rc = sc.get(&d_pcnt, (size_t)n_pblocks + 1))) return rc;
        if ((rc = sc.get(&d_before, ((size_t)n_pblocks + 4) & ~(size_t)3))) return rc;
        if ((rc = sc.get(&d_ppair, ((size_t)n_pblocks + 4) & ~(size_t)3))) return rc;
    }
    // clears: the containers' CALL totals (units add to them), the pieces' counts and hand-over bytes
    if ((rc = clear_words(t->stream, [](uint64_t most) { return (uint32_t)std::min<uint64_t>(1024, most / 1024 + 1); },
                          {{d_ccnt, n_cont}, {d_pcnt, pieces ? (uint64_t)n_pblocks + 1 : 0}, {d_before, pieces ? ((uint64_t)n_pblocks + 4) / 4 : 0}})))
        return rc;
    if (pieces)
        hipLaunchKernelGGL(kg::piece_starts_kernel, dim3((n_pblocks + 3) / 4), dim3(256), 0, t->stream, res->d_hits, res->d_chs,
                           (uint32_t)n_hits, ag.pshift, ap.max_gap, d_pstart, d_ppair, n_pblocks, ag.agg_pairs);
    // one wave per unit: the containers' first pieces (several consecutive containers per wave when there are millions of
    // them: short reads), then one per block of hits[] that a later piece may start in
    const uint32_t cpw = (uint32_t)std::min<uint64_t>(16, std::max<uint64_t>(1, n_cont / (1u << 17)));
    const uint32_t n_cwaves = (uint32_t)((n_cont + cpw - 1) / cpw);
    if (n_cont) {
        // what the kernel reads only where a unit ends: a block in device memory.  Its arrays come out of the table's block
        // cache, so in a run of like scans they do not change and nothing is sent.
        const kg::CallsCold cold = {d_staged, res->d_tail_ev, d_ccnt, d_first, d_pcnt, d_before, d_ppair};
        if (!t->d_calls_cold || memcmp(&cold, &t->h_calls_cold, sizeof cold)) {
            if (!t->d_calls_cold) HIP_TRY(hipMalloc((void **)&t->d_calls_cold, sizeof cold));
            t->h_calls_cold = cold;
            HIP_TRY(hipMemcpyAsync(t->d_calls_cold, &t->h_calls_cold, sizeof cold, hipMemcpyHostToDevice, t->stream));
        }
        hipLaunchKernelGGL(kg::calls_wave_kernel, dim3((n_cwaves + n_pblocks + 3) / 4), dim3(256), 0, t->stream, res->d_hits, res->d_chs,
                           (uint32_t)n_cont, ap, d_acc, d_vote, cpw, n_cwaves, d_pstart, ag.pshift, n_pblocks, t->d_calls_cold);
        if (pieces)
            hipLaunchKernelGGL(kg::merge_before_kernel, dim3((n_pblocks + 255) / 256), dim3(256), 0, t->stream, d_pstart, d_ppair, d_before,
                               n_pblocks, res->d_ev, (unsigned long long *)(d_totals + kTotPieces));
        HIP_TRY(hipGetLastError());
    }
    if ((rc = prefix_sum(t, d_ccnt, n_cont, d_coff, d_partial, d_totals + kTotCalls))) return rc;
    if (n_cont) HIP_TRY(hipMemcpyAsync(t->h_pin + kPinCalls, d_totals + kTotCalls, 8, hipMemcpyDeviceToHost, t->stream));
    if (pieces) HIP_TRY(hipMemcpyAsync(t->h_pin + kPinPieces, d_totals + kTotPieces, 8, hipMemcpyDeviceToHost, t->stream));
    if (n_seqs) {
        // the voters of all CALLs as one dense list of otuIndex values in record order, then the replay per sequence
        const uint32_t n_vchunks = (uint32_t)((n_hits + 63) / 64);
        uint32_t *d_vcnt = nullptr, *d_voff = nullptr;
        int32_t *d_vlist = nullptr;
        uint64_t *d_vpartial = nullptr;
        if ((rc = sc.get(&d_vcnt, (size_t)n_vchunks + 1))) return rc;
        if ((rc = sc.get(&d_voff, (size_t)n_vchunks + 1))) return rc;
        if ((rc = sc.get(&d_vlist, (size_t)n_hits + 1))) return rc;
        if ((rc = sc.get(&d_vpartial, (size_t)((n_vchunks + 1) / kg::kScanChunk + 2)))) return rc;
        if (n_hits) {
            const uint32_t vgrid = (uint32_t)((n_hits + 255) / 256);
            // (n_vchunks + 1 items: the kernel zeroes the entry behind the last chunk; its prefix is the total, read for
            //  "behind the last record")
            hipLaunchKernelGGL(kg::voter_count_kernel, dim3(vgrid), dim3(256), 0, t->stream, d_vote, (uint32_t)n_hits, d_vcnt);
            if ((rc = prefix_sum(t, d_vcnt, (uint64_t)n_vchunks + 1, d_voff, d_vpartial, d_totals + kTotVoters))) return rc;
            hipLaunchKernelGGL(kg::voter_scatter_kernel, dim3(vgrid), dim3(256), 0, t->stream, res->d_hits, d_vote, (uint32_t)n_hits, d_voff,
                               d_vlist);
        } else {
            HIP_TRY(hipMemsetAsync(d_voff, 0, 4, t->stream));
        }
        const uint32_t spw = (uint32_t)std::min<uint64_t>(16, std::max<uint64_t>(1, (uint64_t)n_seqs / (1u << 17)));
        hipLaunchKernelGGL(kg::otu_wave_kernel, dim3((uint32_t)((((uint64_t)n_seqs + spw - 1) / spw + 3) / 4)), dim3(256), 0, t->stream,
                           d_vlist, d_voff, d_vote, res->d_chs, (uint32_t)n_hits, (uint32_t)n_seqs, PER, res->d_otu, spw, d_otu_init);
    }
    hipLaunchKernelGGL(kg::call_starts_kernel, dim3((uint32_t)((n_cont + 1 + 255) / 256)), dim3(256), 0, t->stream, d_coff,
                       n_cont, d_totals + kTotCalls, res->d_ccs);
    if ((rc = dalloc(t, (void **)&res->d_calls, (size_t)(n_hits / (uint64_t)p->min_hits + 1) * sizeof(kg_call)))) return rc;
    if (n_cont) {
        if (n_cont < (1u << 17))
            hipLaunchKernelGGL((kg::compact_calls_kernel<64>), dim3((uint32_t)((n_cont * 64 + 255) / 256)), dim3(256), 0, t->stream,
                               d_staged, res->d_chs, d_first, d_coff, (uint32_t)n_cont, (uint32_t)p->min_hits, res->d_calls,
                               d_pstart, d_pcnt, ag.pshift);
        else
            hipLaunchKernelGGL((kg::compact_calls_kernel<1>), dim3((uint32_t)((n_cont + 255) / 256)), dim3(256), 0, t->stream,
                               d_staged, res->d_chs, d_first, d_coff, (uint32_t)n_cont, (uint32_t)p->min_hits, res->d_calls,
                               d_pstart, d_pcnt, ag.pshift);
    }
    HIP_TRY(hipGetLastError());
    return KG_OK;
}

// kg_aggregate_hits on its context t: the caller's records into r, the aggregation, r's statistics
int aggregate_records(kg_table *t, const kg_params *p, const kg_hit *hits, const int64_t *container_hit_start, int64_t n_seqs,
                      const kg_otu *otu_init, kg_result *r)
{
    const uint64_t n_cont = (uint64_t)n_seqs * r->per, n_hits = (uint64_t)container_hit_start[n_cont];
    Scratch sc(t);
    int rc;
    uint64_t *d_partial = nullptr, *d_totals = nullptr;
    kg_otu *d_init = nullptr;
    if ((rc = dalloc(t, (void **)&r->d_hits, (n_hits ? n_hits : 1) * sizeof(kg_hit)))) return rc;
    if ((rc = dalloc(t, (void **)&r->d_chs, (n_cont + 1) * 8))) return rc;
    if ((rc = sc.get(&d_partial, (size_t)(n_cont / kg::kScanChunk + 2)))) return rc;
    if ((rc = sc.get(&d_totals, 8))) return rc;
    if (otu_init && n_seqs && (rc = sc.get(&d_init, (size_t)n_seqs))) return rc;
    HIP_TRY(hipMemsetAsync(d_totals, 0, 64, t->stream));
    if (n_hits) HIP_TRY(hipMemcpyAsync(r->d_hits, hits, n_hits * sizeof(kg_hit), hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(r->d_chs, container_hit_start, (n_cont + 1) * 8, hipMemcpyHostToDevice, t->stream));
    if (d_init) HIP_TRY(hipMemcpyAsync(d_init, otu_init, (size_t)n_seqs * sizeof(kg_otu), hipMemcpyHostToDevice, t->stream));
    // (caller-supplied records: positions are whatever the caller says, so long containers stay in one piece)
    if ((rc = aggregate_stage(t, p, r, sc, n_seqs, n_cont, n_hits, r->per, d_partial, d_totals, d_init, false, plan_aggregate()))) return rc;
    HIP_TRY(hipStreamSynchronize(t->stream));
    r->st.n_seqs = n_seqs; r->st.n_containers = (int64_t)n_cont; r->st.n_hits = (int64_t)n_hits;
    r->st.n_calls = (int64_t)t->h_pin[kPinCalls];
    r->st.windows_valid = -1; r->st.slots_inspected = -1;
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_aggregate_hits(int device, const kg_params *p, const kg_hit *hits, const int64_t *container_hit_start, int64_t n_seqs,
                      const kg_otu *otu_init, kg_result **out)
{
    if (!p || !container_hit_start || !out || n_seqs < 0) return fail(KG_ERR_ARG, "null or negative argument");
    if (n_seqs > 0x7FFFFFF0ll / 6) return fail(KG_ERR_LIMIT, "too many sequences in one batch");
    if (p->min_hits < 2)
        return fail(KG_ERR_UNSUPPORTED, "minHits < 2: the reference throws in processSetOfHits (KGJ:442); refusing");
    const uint32_t PER = p->aa ? 1u : 6u;
    const uint64_t n_cont = (uint64_t)n_seqs * PER;
    if (container_hit_start[0] != 0) return fail(KG_ERR_ARG, "container_hit_start[0] must be 0");
    for (uint64_t c = 0; c < n_cont; c++)
        if (container_hit_start[c + 1] < container_hit_start[c]) return fail(KG_ERR_ARG, "container_hit_start must be non-decreasing");
    const uint64_t n_hits = (uint64_t)container_hit_start[n_cont];
    if (n_hits && !hits) return fail(KG_ERR_ARG, "null hit records");
    if (n_hits > 0xFFFFFF00ull) return fail(KG_ERR_LIMIT, "more than 2^32-256 hit records");
    CallScope cs(device, /* hook = */ false);          // (this call has never armed KG_TEST_FAIL_ALLOC)
    if (cs.rc) return cs.rc;
    kg_result *r = new (std::nothrow) kg_result();
    if (!r) return fail(KG_ERR_NOMEM, "out of host memory");
    r->tab = cs.t; r->per = PER;
    if (const int rc = aggregate_records(cs.t, p, hits, container_hit_start, n_seqs, otu_init, r)) return fail_and_free(r, rc);
    r->own_tab = true;                  // the result keeps the context
    cs.disown();
    *out = r;
    return KG_OK;
}

int kg_process_set_of_hits(int device, const kg_params *p, const kg_hit *hits, int32_t n_hits, int32_t current_fi, kg_otu *otu,
                           kg_call *call, int32_t *called, int32_t *new_current_fi, int32_t *keeps_last_two)
{
    if (!p || !hits || !otu || !call || !called || !new_current_fi || !keeps_last_two) return fail(KG_ERR_ARG, "null argument");
    if (n_hits < 2)
        return fail(KG_ERR_UNSUPPORTED, "processSetOfHits on fewer than two hits: the reference throws (hits.get(numHits-2), KGJ:442); refusing");
    if (otu->n < 0 || otu->n > KG_OI_BUFSZ) return fail(KG_ERR_ARG, "oICounts holds more than OI_BUFSZ entries");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(KG_ERR_DEVICE, "no HIP device: libkmerguts_hip needs an MI355X (gfx950) GPU; there is no CPU path");
    if (device < 0 || device >= ndev) return fail(KG_ERR_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    kg_hit *d_hits = nullptr;
    uint8_t *d_small = nullptr;                        // kg_otu | kg_call | int32 x 4
    const size_t small = sizeof(kg_otu) + sizeof(kg_call) + 16;
    HIP_TRY(hipMalloc((void **)&d_hits, (size_t)n_hits * sizeof(kg_hit)));
    hipError_t e = hipMalloc((void **)&d_small, small);
    if (e == hipSuccess) e = hipMemcpy(d_hits, hits, (size_t)n_hits * sizeof(kg_hit), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_small, 0, small);
    if (e == hipSuccess) e = hipMemcpy(d_small, otu, sizeof(kg_otu), hipMemcpyHostToDevice);
    uint8_t h_small[sizeof(kg_otu) + sizeof(kg_call) + 16];
    if (e == hipSuccess) {
        kg::AggParams ap;
        ap.min_hits = p->min_hits; ap.min_weighted_hits = p->min_weighted_hits;
        ap.max_gap = p->max_gap; ap.order_constraint = p->order_constraint ? 1 : 0;
        hipLaunchKernelGGL(kg::process_set_single_kernel, dim3(1), dim3(64), 0, nullptr, d_hits, n_hits, current_fi, ap,
                           (kg_otu *)d_small, (kg_call *)(d_small + sizeof(kg_otu)), (int32_t *)(d_small + sizeof(kg_otu) + sizeof(kg_call)));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(h_small, d_small, small, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d_hits);
    if (d_small) (void)hipFree(d_small);
    if (e != hipSuccess) return fail(KG_ERR_DEVICE, std::string("processSetOfHits on the device failed: ") + hipGetErrorString(e));
    memcpy(otu, h_small, sizeof(kg_otu));
    memcpy(call, h_small + sizeof(kg_otu), sizeof(kg_call));
    int32_t o3[4];
    memcpy(o3, h_small + sizeof(kg_otu) + sizeof(kg_call), 16);
    *called = o3[0]; *new_current_fi = o3[1]; *keeps_last_two = o3[2];
    return KG_OK;
}

}  // extern "C"
