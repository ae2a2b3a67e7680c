// kg_host_scan.hpp -- kg_scan / kg_scan_device: the stages that enqueue what kg_host_plan.hpp planned.  scan_entry -> scan_impl: the
// buffers both strategies use, scan_partitioned (chunk_passes and chunk_order per chunk) or scan_direct, the KG_F_PROGRESS
// helpers, then aggregate_stage (kg_host_aggregate.hpp) and the timings (kernels: kg_device.hpp, kg_partition.hpp, kg_order.hpp).
// Part of kmerguts_hip.hip's translation unit: behind kg_host_plan.hpp and kg_host_aggregate.hpp.
#pragma once

namespace {

// What every stage of one kg_scan* call works on.
struct ScanCtx {
    kg_table *t;
    kg_result *res;
    Scratch &sc;
    const BatchPlan &b;
    const uint8_t *d_seq, *h_seq;       // h_seq != null: d_seq is an empty device buffer; the characters are still to upload
    const int64_t *offsets;
    int64_t n_seqs;
    bool progress, counters;            // KG_F_PROGRESS; the walks are noted by the counting kernels (KG_F_COUNTERS or progress)
    bool seq_uploaded;
    uint64_t n_hits = 0;
    // device, shared by the strategies
    int64_t *d_off = nullptr;
    uint32_t *d_ibase = nullptr;
    kg::BlockDesc *d_blocks = nullptr;
    uint32_t *d_counts = nullptr, *d_offs = nullptr, *d_bsb = nullptr;      // direct: hits per row, their prefix, one staging base per (block, row group)
    uint64_t *d_partial = nullptr, *d_totals = nullptr;                     // prefix-sum scratch; the kTot* words
    kg::Progress *d_prog = nullptr;
};

// The characters [a, b) of the batch, where the caller's copy is still on the host.
int upload_seq(const ScanCtx &cx, int64_t a, int64_t b)
{
    if (cx.h_seq && b > a)
        HIP_TRY(hipMemcpyAsync(const_cast<uint8_t *>(cx.d_seq) + a, cx.h_seq + a, (size_t)(b - a), hipMemcpyHostToDevice, cx.t->stream));
    return KG_OK;
}

// Device blocks that are sized per attempt.  release(): straight back to the cache, for a resized attempt to reuse -- only
// while all streams are idle.  However else the owner's scope is left (an error return in the middle of an attempt included),
// the blocks go back with the rest of the scratch once the streams are idle (Scratch's destructor runs later).
template <int N>
struct BlockGuard {
    Scratch &sc;
    void **slot[N];
    void release() { for (void **q : slot) { dfree(sc.t, *q); *q = nullptr; } }
    ~BlockGuard() { for (void **q : slot) if (*q) { sc.adopt(*q); *q = nullptr; } }
};

// ... and the result's hit records of an attempt that is thrown away (all streams idle)
void drop_hits(kg_table *t, kg_result *res)
{
    dfree(t, res->d_hits); dfree(t, res->d_hit_slots);
    res->d_hits = nullptr; res->d_hit_slots = nullptr;
}

// The counters the host decides on, to their pinned words (a hipMemcpyAsync to pageable memory blocks the host per copy; to
// pinned memory it does not: one host round trip for all of them).  d_pc / d_ovfc: null for the direct strategy.
int send_counters(kg_table *t, const uint64_t *d_pc, const uint32_t *d_ovfc, const uint64_t *d_totals, hipStream_t s)
{
    if (d_pc) {
        HIP_TRY(hipMemcpyAsync(t->h_pin + kPinPc, d_pc, kPcWords * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(t->h_pin + kPinOvf, d_ovfc, kOvfWords * kMaxChunks * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipMemcpyAsync(t->h_pin + kPinTotals, d_totals, kTotSent * 8, hipMemcpyDeviceToHost, s));
    return KG_OK;
}

// The finished scan's totals (in their pinned words) into the stats, and the staging ratio's high-water mark into the table.
void note_totals(ScanCtx &cx, uint64_t n_hits, bool counted)
{
    kg_table *t = cx.t;
    kg_stats &st = cx.res->st;
    const uint64_t *h_tot = t->h_pin + kPinTotals;
    st.windows_valid = counted ? (int64_t)h_tot[kTotValid] : -1;
    st.slots_inspected = counted ? (int64_t)h_tot[kTotSlots] : -1;
    st.lookup_ran_off = h_tot[kTotRanOff] ? 1 : 0;
    if (cx.b.windows) {
        double ratio = (double)n_hits / (double)cx.b.windows * 1.1 + 1e-3;
        if (ratio > t->stage_ratio) t->stage_ratio = ratio > 1.0 ? 1.0 : ratio;
    }
    cx.n_hits = n_hits;
    st.n_hits = (int64_t)n_hits;
}

// KG_F_PROGRESS: the walks' summary (kg_device.hpp, Progress).  lo[f] = the smallest slot of tenth >= f, found with the
// reference's own double arithmetic (KGJ:1018) around ceil(f * numSigs / 10) - 1
int progress_begin(ScanCtx &cx)
{
    kg_table *t = cx.t;
    int rc;
    if (t->limit > 0xFFFFFFFFull) return fail(KG_ERR_UNSUPPORTED, "KG_F_PROGRESS: table streams of 2^32 records or more");
    if ((rc = cx.sc.get(&cx.d_prog, 1))) return rc;
    kg::Progress h;
    for (auto &x : h.first) x = ~0ull;
    h.last_plus1 = 0; h.first_beyond = ~0ull; h.walk_ran_off = 0;
    for (auto &x : h.found_upto) x = 0;
    h.kmers_found = 0;
    for (auto &x : h.miss_max1) x = 0;
    const double n = (double)t->num_sigs;
    auto tenth = [&](uint64_t s) { return (int)(10.0 * ((double)(s + 1) / n)); };
    for (int f = 0; f <= 10; f++) {
        const unsigned __int128 num = (unsigned __int128)(uint64_t)t->num_sigs * (unsigned)f;
        uint64_t s = (uint64_t)((num + 9) / 10);
        s = s > 3 ? s - 3 : 0;
        while (tenth(s) < f) s++;
        h.lo[f] = s;
    }
    HIP_TRY(hipMemcpyAsync(cx.d_prog, &h, sizeof h, hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));                             // (h is a stack object)
    return KG_OK;
}

// ... behind the scan: index_walks = the byte home index pass noted the certain misses' walks (all chunks are behind us:
// stream2 and stream3 were joined)
int progress_finish(ScanCtx &cx, bool index_walks)
{
    kg_table *t = cx.t;
    int rc;
    if (index_walks)
        hipLaunchKernelGGL(kg::progress_finish_kernel, dim3(1), dim3(256), 0, t->stream, cx.d_prog, t->d_tags, t->limit);
    // kmersFound / found-so-far: the distinct slots of the hit records (a bitmap over the stream's slots)
    uint32_t *d_bitmap = nullptr;
    const uint64_t n_words = (t->limit + 31) / 32 + 1;
    if ((rc = cx.sc.get(&d_bitmap, (size_t)n_words))) return rc;
    HIP_TRY(hipMemsetAsync(d_bitmap, 0, n_words * 4, t->stream));
    if (cx.n_hits)
        hipLaunchKernelGGL(kg::mark_found_kernel, dim3((uint32_t)std::min<uint64_t>(2048, (cx.n_hits + 255) / 256)), dim3(256), 0, t->stream,
                           cx.res->d_hit_slots, cx.n_hits, d_bitmap);
    hipLaunchKernelGGL(kg::count_found_kernel, dim3((uint32_t)std::min<uint64_t>(2048, (n_words + 255) / 256)), dim3(256), 0, t->stream,
                       d_bitmap, n_words, cx.d_prog);
    return KG_OK;
}

// ... and once the stream is idle: the summary into the result
int progress_fetch(ScanCtx &cx)
{
    kg::Progress h;
    HIP_TRY(hipMemcpy(&h, cx.d_prog, sizeof h, hipMemcpyDeviceToHost));
    kg_progress &g = cx.res->progress;
    for (int f = 0; f <= 10; f++) g.first_visited[f] = h.first[f] == ~0ull ? -1 : (int64_t)h.first[f];
    g.last_visited = (int64_t)h.last_plus1 - 1;
    g.first_beyond = h.first_beyond == ~0ull ? -1 : (int64_t)h.first_beyond;
    g.walk_ran_off = h.walk_ran_off ? 1 : 0;
    g.stream_slots = (int64_t)cx.t->limit;
    for (int f = 0; f <= 10; f++) g.found_upto[f] = g.first_visited[f] < 0 ? 0 : (int64_t)h.found_upto[f];
    g.kmers_found = (int64_t)h.kmers_found;
    cx.res->has_progress = true;
    return KG_OK;
}

// Device blocks of the partitioned pipeline: every array holds n_chunks slices (ChunkView).
struct PartBuffers {
    uint64_t *d_ent = nullptr, *d_ovf_ent = nullptr;
    uint32_t *d_fill = nullptr, *d_ovf_bucket = nullptr, *d_next = nullptr;
    uint32_t *d_ovfc = nullptr;          // kOvfWords per chunk (kOvf*)
    uint32_t *d_lowc = nullptr;          // block numbers set aside by the scatter pass
    kg::RowGeo *d_geo = nullptr;         // per row: container and position of its first window (kg_order.hpp)
    uint64_t *d_pc = nullptr;            // the kPc* words
    uint32_t *d_ghist = nullptr, *d_gbase = nullptr, *d_gcur1 = nullptr, *d_gcur2 = nullptr, *d_gtile = nullptr;
    // the lists, sized per attempt (BlockGuard): capacities per chunk
    uint64_t ucap = 0, ccap = 0;
    size_t cused_stride = 0, candused_stride = 0;
    kg_hit *d_ulist = nullptr, *d_sortA = nullptr, *d_sortB = nullptr;
    uint32_t *d_cused = nullptr, *d_candused = nullptr;
    kg::CandRec *d_cand = nullptr;
};

// Chunk c's slices of them.
struct ChunkView {
    uint32_t c, lo, nb;                  // blocks [lo, lo + nb)
    uint64_t *ent, *ovf_ent;
    uint32_t *fill, *next, *ovfc, *ovf_bucket;
    kg_hit *ulist, *sortA, *sortB;
    uint32_t *cused, *candused;
    kg::CandRec *cand;
    unsigned long long *ucur, *ccur;
    uint64_t *base, *ctot;
    uint32_t *ghist, *gbase, *gcur1, *gcur2, *gtile;
};

ChunkView chunk_view(const PartPlan &pl, const PartBuffers &pb, uint32_t c)
{
    ChunkView v;
    v.c = c; v.lo = (uint32_t)pl.clo[c]; v.nb = (uint32_t)(pl.clo[c + 1] - pl.clo[c]);
    v.ent = pb.d_ent + (uint64_t)c * pl.n_regions * pl.cap;
    v.fill = pb.d_fill + (uint64_t)c * pl.n_regions;
    v.next = pb.d_next + (size_t)c * pl.next_stride;
    v.ovfc = pb.d_ovfc + kOvfWords * c; v.ovf_bucket = pb.d_ovf_bucket + (size_t)c * pl.ovf_cap;
    v.ovf_ent = pb.d_ovf_ent + (size_t)c * pl.ovf_cap * kg::kGroup;
    v.ulist = pb.d_ulist + (uint64_t)c * pb.ucap;
    v.cused = pb.d_cused + c * pb.cused_stride; v.candused = pb.d_candused + c * pb.candused_stride;
    v.cand = pb.d_cand + (uint64_t)c * pb.ccap;
    v.ucur = (unsigned long long *)(pb.d_pc + kPcUcur + c); v.ccur = (unsigned long long *)(pb.d_pc + kPcCcur + c);
    v.base = pb.d_pc + kPcBase + c; v.ctot = pb.d_pc + kPcCtot + c;
    v.ghist = pb.d_ghist + (size_t)c * pl.groups_stride; v.gbase = pb.d_gbase + (size_t)c * (pl.groups_stride + 1);
    v.gcur1 = pb.d_gcur1 + (size_t)c * (kg::kHDigits + 1); v.gcur2 = pb.d_gcur2 + (size_t)c * pl.groups_stride;
    v.gtile = pb.d_gtile + (size_t)c * (kg::kHDigits + 1);
    v.sortA = pb.d_sortA + (uint64_t)c * pb.ucap; v.sortB = pb.d_sortB + (uint64_t)c * pb.ucap;
    return v;
}

// The scatter kernel's instantiation: 0 plain, 1 the record stream ends before numSigs (only then can a home slot lie beyond
// it), 2 the same with KG_F_PROGRESS (the slots beyond the stream are noted).
int scatter_variant_of(const ScanCtx &cx)
{
    return cx.t->limit >= (uint64_t)cx.t->num_sigs ? 0 : cx.d_prog ? 2 : 1;
}
template <typename F>
void scatter_variant(int variant, F &&f)
{
    if (variant == 0) f(std::false_type{}, std::false_type{});
    else if (variant == 1) f(std::true_type{}, std::false_type{});
    else f(std::true_type{}, std::true_type{});
}

// The chunks' cold-path parameter blocks of the scatter pass (kg::ScatterCold), in front of the first scatter pass on its
// stream.  The blocks they point to come out of the table's block cache, so in a run of like scans they do not change and
// nothing is sent.
int upload_scatter_cold(const ScanCtx &cx, const PartPlan &pl, const PartBuffers &pb)
{
    kg_table *t = cx.t;
    kg::ScatterCold h[kMaxChunks] = {};
    for (uint32_t c = 0; c < pl.n_chunks; c++) {
        uint32_t *ovfc = pb.d_ovfc + kOvfWords * c;
        h[c].ovf_cursor = ovfc; h[c].ovf_bucket = pb.d_ovf_bucket + (size_t)c * pl.ovf_cap;
        h[c].ovf_ent = pb.d_ovf_ent + (size_t)c * pl.ovf_cap * kg::kGroup;
        h[c].lowc_cursor = ovfc + kOvfLowc; h[c].lowc_blocks = pb.d_lowc + pl.clo[c];
        h[c].ctr = (unsigned long long *)(cx.d_totals + kTotValid); h[c].prog = cx.d_prog;
        h[c].ovf_cap = pl.ovf_cap;
    }
    if (!t->d_cold) HIP_TRY(hipMalloc((void **)&t->d_cold, sizeof h));
    else if (!memcmp(h, t->h_cold, sizeof h)) return KG_OK;
    memcpy(t->h_cold, h, sizeof h);
    HIP_TRY(hipMemcpyAsync(t->d_cold, t->h_cold, sizeof h, hipMemcpyHostToDevice, t->stream));
    return KG_OK;
}

// One chunk through scatter (stream) -> low-complexity blocks, tag or index pass (stream2) -> verify, overflow (stream3).
template <bool AA>
int chunk_passes(const ScanCtx &cx, const PartPlan &pl, const PartBuffers &pb, const ChunkView &v)
{
    kg_table *t = cx.t;
    kg::Progress *d_prog = cx.d_prog;
    unsigned long long *d_ctr = (unsigned long long *)(cx.d_totals + kTotValid);
    const hipStream_t s2 = t->stream2, s3 = t->stream3;
    uint32_t *lowc_cursor = v.ovfc + kOvfLowc, *lowc = pb.d_lowc + v.lo;
    const uint32_t limit32 = (uint32_t)std::min<uint64_t>(t->limit, 0xFFFFFFFFull);         // slots are < num_sigs < 2^31
    scatter_variant(scatter_variant_of(cx), [&](auto is_short, auto prog) {
        constexpr bool SHORT = decltype(is_short)::value, PROG = decltype(prog)::value;
        hipLaunchKernelGGL((kg::part_scatter_kernel<AA, SHORT, PROG>), dim3(pl.n_wg), dim3(kg::kWave * kg::kScatterWaves), pl.scatter_lds,
                           t->stream, cx.d_seq, cx.d_blocks, v.lo, v.nb, limit32, (uint32_t)t->num_sigs, t->m35, pl.shift, pl.buckets, pl.cap,
                           v.ent, v.fill, t->d_cold + v.c, pl.scatter_prio, pl.flush_list);
    });
    HIP_TRY(hipEventRecord(t->pev[kPevChunk + 2 * v.c], t->stream));
    HIP_TRY(hipStreamWaitEvent(s2, t->pev[kPevChunk + 2 * v.c], 0));
    // the low-complexity blocks the scatter pass set aside (usually none: every workgroup reads the count and
    // leaves).  In front of the chunk's tag pass, not behind its scatter pass, and in one-wave workgroups whose
    // 4.9 KB of LDS fit beside a resident scatter workgroup (153 KB of a CU's 160): with four-wave workgroups
    // (15.8 KB) the kernel -- and the tag pass behind it -- waited for the NEXT chunk's scatter pass to leave
    // the CUs (profiles/r02_pipeline.md).
    hipLaunchKernelGGL((kg::lowc_blocks_kernel<AA>), dim3(pl.lowc_grid), dim3(64 * kg::kLowcWaves), 0, s2, cx.d_seq, cx.d_blocks, lowc_cursor, lowc,
                       t->limit, (uint32_t)t->num_sigs, t->m35, pl.shift, pl.n_wg, pl.cap, v.ent, v.fill, v.ovfc, pl.ovf_cap,
                       v.ovf_bucket, v.ovf_ent, d_ctr, d_prog);
    if (pl.use_bidx) {
        // regions per hand-out by their expected fill (an iteration covers 256 * N / R entry slots of each); the
        // kernel for tables whose classes are their quotients has no q % 19
        const uint32_t tail_start = (uint32_t)std::min<uint64_t>(t->tail_start, 0xFFFFFFFFull);
        dispatch<int, 1, 2, 4>((int)pl.index_r, [&](auto r) {
            dispatch<bool, true, false>(t->bidx_exact, [&](auto exact) {
                dispatch<bool, true, false>(pl.prog_index, [&](auto prog) {
                    constexpr int R = decltype(r)::value;
                    constexpr bool EXACT = decltype(exact)::value, PROG = decltype(prog)::value;
                    hipLaunchKernelGGL((kg::bucket_index_kernel<kg::kIndexN, R, EXACT, PROG>), dim3(pl.index_grid), dim3(256), 0, s2,
                                       t->d_bidx, tail_start, v.ent, v.fill, pl.n_wg, pl.cap, pl.buckets, pl.shift, pl.probe_grab, v.next,
                                       v.cand, v.candused, v.ccur, pb.ccap, d_ctr, pl.index_prio, PROG ? d_prog : (kg::Progress *)nullptr);
                });
            });
        });
    } else {
        dispatch<bool, true, false>(pl.part_counters, [&](auto counters) {
            constexpr bool COUNTERS = decltype(counters)::value;
            hipLaunchKernelGGL((kg::bucket_tag_kernel<COUNTERS>), dim3(pl.probe_grid), dim3(256), 0, s2, t->d_tags, t->limit,
                               (uint64_t)t->num_sigs, v.ent, v.fill, pl.n_wg, pl.cap, pl.buckets, pl.shift, pl.probe_grab, v.next, v.cand,
                               v.candused, v.ccur, pb.ccap, d_ctr, COUNTERS ? d_prog : (kg::Progress *)nullptr);
        });
    }
    HIP_TRY(hipEventRecord(t->pev[kPevChunk + 2 * v.c + 1], s2));
    HIP_TRY(hipStreamWaitEvent(s3, t->pev[kPevChunk + 2 * v.c + 1], 0));
    // the walks: counted (0: no, 1: yes), or summarised for KG_F_PROGRESS without counting (2)
    dispatch<int, 1, 2, 0>(pl.part_counters ? 1 : pl.prog_index ? 2 : 0, [&](auto walks) {
        constexpr bool COUNTERS = decltype(walks)::value == 1, PROG = decltype(walks)::value == 2;
        hipLaunchKernelGGL((kg::verify_kernel<AA, COUNTERS, PROG>), dim3(pl.verify_grid), dim3(256), 0, s3, t->d_entries, t->d_tags, t->limit,
                           (uint64_t)t->num_sigs, t->magic, v.cand, v.candused, v.ccur, pb.ccap, v.ulist, v.cused, v.ucur, pb.ucap, d_ctr,
                           d_prog, pl.verify_prio);
        hipLaunchKernelGGL((kg::overflow_probe_kernel<AA, COUNTERS, PROG>), dim3(pl.ovf_grid), dim3(256), 0, s3, t->d_entries, t->d_tags,
                           t->limit, (uint64_t)t->num_sigs, t->magic, v.ovf_bucket, v.ovf_ent, v.ovfc, pl.ovf_cap, pl.shift, v.ulist,
                           v.cused, v.ucur, pb.ucap, d_ctr, d_prog);
    });
    HIP_TRY(hipEventRecord(t->pev[kPevVerified + v.c], s3));
    HIP_TRY(hipGetLastError());
    return KG_OK;
}

// One chunk's ordered placement (kg_order.hpp) behind its verify pass, on the scatter stream or an ordering stream: group histogram -> group starts -> two partition
// passes by key range -> ranking inside each group of rows.  hits_cap: records res->d_hits has room for.
template <bool AA>
int chunk_order(const ScanCtx &cx, const PartPlan &pl, const PartBuffers &pb, const ChunkView &v, uint64_t hits_cap)
{
    constexpr uint32_t PER = AA ? 1 : 6;
    kg_table *t = cx.t;
    kg_result *res = cx.res;
    const uint32_t c = v.c, gshift = pl.gshift;
    const bool last = c + 1 == pl.n_chunks;
    hipStream_t s = t->stream;           // (behind every scatter pass as it is)
    if (pl.n_os) {
        s = t->ostream[c % pl.n_os];
        HIP_TRY(hipStreamWaitEvent(s, t->ev[kEvScattered], 0));          // behind the last scatter pass
    }
    HIP_TRY(hipStreamWaitEvent(s, t->pev[kPevVerified + c], 0));
    const uint64_t row_lo = (uint64_t)v.lo * PER, row_hi = row_lo + (uint64_t)v.nb * PER;
    const uint32_t g0 = (uint32_t)(row_lo >> gshift);
    const uint32_t n_groups = v.nb ? (uint32_t)(((row_hi - 1) >> gshift) - g0 + 1) : 1u;
    hipLaunchKernelGGL(kg::hit_hist_kernel, dim3(pl.order_grid), dim3(kg::kHThreads), (size_t)n_groups * 4, s, v.ulist, v.cused, v.ucur, pb.ucap,
                       g0, 6u + gshift, n_groups, v.ghist);
    hipLaunchKernelGGL(kg::group_scan_kernel, dim3(1), dim3(kg::kGsThreads), 0, s, v.ghist, n_groups, v.gbase, v.gcur1, v.gcur2, v.ctot, v.gtile);
    if (pl.n_os && c) HIP_TRY(hipStreamWaitEvent(s, t->pev[kPevBase + c - 1], 0));      // base of chunk c = base + total of c - 1
    hipLaunchKernelGGL(kg::chunk_base_kernel, dim3(1), dim3(1), 0, s, v.ctot, v.base, last ? cx.d_totals : (uint64_t *)nullptr);
    if (pl.n_os) HIP_TRY(hipEventRecord(t->pev[kPevBase + c], s));
    if (pl.early_totals && last) {
        // Everything the host wants to know about this attempt is final here -- the list cursors (the last verify
        // pass is behind us on this stream), the overflow counters, the exact hit total (chunk_base_kernel just
        // above): it is sent now, and the host reads it, makes the aggregation's allocations and enqueues its
        // kernels while the last chunk's partition passes and placement still run (the round trip was ~70 us
        // of every scan, behind the ordering).
        int rc;
        if ((rc = send_counters(t, pb.d_pc, pb.d_ovfc, cx.d_totals, s))) return rc;
        HIP_TRY(hipEventRecord(t->pev[kPevTotals], s));
    }
    hipLaunchKernelGGL((kg::hit_partition_kernel<true>), dim3(pl.order_grid), dim3(kg::kHThreads), 0, s, v.ulist, v.cused, v.ucur, pb.ucap,
                       v.gbase, n_groups, g0, 6u + gshift, v.gcur1, v.sortA, pb.ucap, v.gtile);
    hipLaunchKernelGGL((kg::hit_partition_kernel<false>), dim3(pl.order_grid), dim3(kg::kHThreads), 0, s, v.sortA, v.cused, v.ucur, pb.ucap,
                       v.gbase, n_groups, g0, 6u + gshift, v.gcur2, v.sortB, pb.ucap, v.gtile);
    hipLaunchKernelGGL((kg::group_place_kernel<AA>), dim3(std::min(n_groups, 256u * 8u)), dim3(kg::kHThreads),
                       kg::group_place_lds(gshift, pl.place_staged), s,
                       v.sortB, v.gbase, n_groups, g0, gshift, (uint32_t)row_lo, (uint32_t)row_hi, pb.d_geo, (uint64_t)cx.b.n_rows,
                       pl.place_staged ? 1u : 0u, v.base, res->d_hits, hits_cap, cx.d_offs, res->d_hit_slots);
    HIP_TRY(hipGetLastError());
    return KG_OK;
}

// The blocks of the partitioned pipeline that do not depend on the attempt, and the dynamic LDS its kernels may ask for.
template <bool AA>
int part_allocate(ScanCtx &cx, const PartPlan &pl, PartBuffers &pb)
{
    kg_table *t = cx.t;
    Scratch &sc = cx.sc;
    const uint32_t n_chunks = pl.n_chunks, groups_stride = pl.groups_stride;
    int rc;
    if ((rc = sc.get(&pb.d_ent, (size_t)(pl.n_regions * pl.cap * n_chunks)))) return rc;
    if ((rc = sc.get(&pb.d_fill, (size_t)pl.n_regions * n_chunks))) return rc;
    if ((rc = sc.get(&pb.d_ovf_ent, (size_t)pl.ovf_cap * kg::kGroup * n_chunks))) return rc;
    if ((rc = sc.get(&pb.d_ovf_bucket, (size_t)pl.ovf_cap * n_chunks))) return rc;
    if ((rc = sc.get(&pb.d_next, pl.next_stride * n_chunks))) return rc;
    if ((rc = sc.get(&pb.d_ovfc, kOvfWords * kMaxChunks))) return rc;
    if ((rc = sc.get(&pb.d_lowc, (size_t)cx.b.nblocks + 1))) return rc;
    if ((rc = sc.get(&pb.d_geo, (size_t)cx.b.n_rows))) return rc;
    if ((rc = sc.get(&pb.d_ghist, (size_t)groups_stride * n_chunks))) return rc;
    if ((rc = sc.get(&pb.d_gbase, (size_t)(groups_stride + 1) * n_chunks))) return rc;
    if ((rc = sc.get(&pb.d_gcur1, (size_t)(kg::kHDigits + 1) * n_chunks))) return rc;
    if ((rc = sc.get(&pb.d_gcur2, (size_t)groups_stride * n_chunks))) return rc;
    if ((rc = sc.get(&pb.d_gtile, (size_t)(kg::kHDigits + 1) * n_chunks))) return rc;
    if (kg::group_place_lds(pl.gshift, pl.gshift == 10) > t->place_lds[AA ? 1 : 0]) {
        const size_t want_lds = kg::group_place_lds(pl.gshift, pl.gshift == 10);
        HIP_TRY(hipFuncSetAttribute((const void *)kg::group_place_kernel<AA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want_lds));
        t->place_lds[AA ? 1 : 0] = want_lds;
    }
    if (groups_stride * 4u > t->hist_lds) {
        HIP_TRY(hipFuncSetAttribute((const void *)kg::hit_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(groups_stride * 4u)));
        t->hist_lds = groups_stride * 4u;
    }
    if ((rc = sc.get(&pb.d_pc, kPcWords))) return rc;
    const int sv = scatter_variant_of(cx);
    if (t->scatter_lds[AA ? 1 : 0][sv] < pl.scatter_lds) {     // once per table (and geometry): the call costs tens of microseconds
        hipError_t e = hipSuccess;
        scatter_variant(sv, [&](auto is_short, auto prog) {
            e = hipFuncSetAttribute((const void *)kg::part_scatter_kernel<AA, decltype(is_short)::value, decltype(prog)::value>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.scatter_lds);
        });
        HIP_TRY(e);
        t->scatter_lds[AA ? 1 : 0][sv] = pl.scatter_lds;
    }
    return KG_OK;
}

// The partitioned strategy.  done = true: the hit records are placed (res->d_hits, cx.n_hits).  done = false with KG_OK: the
// batch is too skewed for the provisioned lists (st.fallback says how) and goes to the direct strategy.
template <bool AA>
int scan_partitioned(ScanCtx &cx, const PartPlan &pl, bool &done)
{
    constexpr uint32_t PER = AA ? 1 : 6;
    kg_table *t = cx.t;
    kg_result *res = cx.res;
    kg_stats &st = res->st;
    const uint32_t n_chunks = pl.n_chunks;
    const uint64_t nblocks = cx.b.nblocks;
    int rc;
    PartBuffers pb;
    if ((rc = part_allocate<AA>(cx, pl, pb))) return rc;
    BlockGuard<6> lists{cx.sc, {(void **)&pb.d_ulist, (void **)&pb.d_cused, (void **)&pb.d_cand, (void **)&pb.d_candused,
                                (void **)&pb.d_sortA, (void **)&pb.d_sortB}};
    pb.ucap = pl.ucap; pb.ccap = pl.ccap;
    HIP_TRY(hipEventRecord(t->ev[kEvScanBegin], t->stream));
    for (int attempt = 0; attempt < 3; attempt++) {
        const uint64_t ucap = pb.ucap, ccap = pb.ccap;
        const uint64_t hits_cap = ucap * n_chunks;
        pb.cused_stride = (size_t)(ucap / kg::kUChunk + 1); pb.candused_stride = (size_t)(ccap / kg::kUChunk + 1);
        if ((rc = dalloc(t, (void **)&res->d_hits, hits_cap * sizeof(kg_hit)))) return rc;
        if (cx.progress && (rc = dalloc(t, (void **)&res->d_hit_slots, hits_cap * 4))) return rc;
        if ((rc = dalloc(t, (void **)&pb.d_ulist, ucap * n_chunks * sizeof(kg_hit)))) return rc;
        if ((rc = dalloc(t, (void **)&pb.d_cused, pb.cused_stride * n_chunks * 4))) return rc;
        if ((rc = dalloc(t, (void **)&pb.d_cand, ccap * n_chunks * sizeof(kg::CandRec)))) return rc;
        if ((rc = dalloc(t, (void **)&pb.d_candused, pb.candused_stride * n_chunks * 4))) return rc;
        if ((rc = dalloc(t, (void **)&pb.d_sortA, ucap * n_chunks * sizeof(kg_hit)))) return rc;
        if ((rc = dalloc(t, (void **)&pb.d_sortB, ucap * n_chunks * sizeof(kg_hit)))) return rc;
        // one launch for all clears (d_totals: totals, counters and flags of a re-run start over); the grid follows the LARGEST list
        // (the kernel strides)
        if ((rc = clear_words(t->stream, [](uint64_t most) { return (uint32_t)std::min<uint64_t>(4096, (most / 4 + 255) / 256 + 1); },
                              {{pb.d_cused, (uint64_t)pb.cused_stride * n_chunks},
                               {pb.d_candused, (uint64_t)pb.candused_stride * n_chunks},
                               {pb.d_pc, kPcWords * 2},
                               {cx.d_totals, kTotWords * 2},
                               {pb.d_ovfc, kOvfWords * kMaxChunks},
                               {pb.d_next, (uint64_t)pl.next_stride * n_chunks},
                               {pb.d_ghist, (uint64_t)pl.groups_stride * n_chunks}})))
            return rc;
        if ((rc = upload_scatter_cold(cx, pl, pb))) return rc;
        HIP_TRY(hipEventRecord(t->pev[kPevFork], t->stream));               // fork: stream2 starts behind the clears
        HIP_TRY(hipStreamWaitEvent(t->stream2, t->pev[kPevFork], 0));
        HIP_TRY(hipStreamWaitEvent(t->stream3, t->pev[kPevFork], 0));
        // the rows' geometry records (kg_order.hpp): they depend on the batch only, and the verify stream has nothing to do
        // until the first chunk is scattered and probed
        hipLaunchKernelGGL((kg::row_geo_kernel<AA>), dim3((uint32_t)((nblocks * PER + 255) / 256)), dim3(256), 0, t->stream3, cx.d_blocks,
                           (uint32_t)nblocks, pb.d_geo);
        for (uint32_t c = 0; c < n_chunks; c++) {
            // (the upload of chunk c+1 runs while chunk c is scanned)
            if (!cx.seq_uploaded && (rc = upload_seq(cx, cx.offsets[pl.cseq[c]], cx.offsets[pl.cseq[c + 1]]))) return rc;
            if ((rc = chunk_passes<AA>(cx, pl, pb, chunk_view(pl, pb, c)))) return rc;
        }
        HIP_TRY(hipEventRecord(t->ev[kEvScattered], t->stream));   // all chunks scattered
        cx.seq_uploaded = true;
        // Ordered placement (kg_order.hpp), chunk by chunk, behind the LAST scatter pass and beside the tag passes that are
        // still running: its partition workgroups hold 51 KB of LDS and eight wave slots each, and started beside a scatter
        // pass (105 KB and 16 wave slots of every CU) the two starve each other -- chunk 0's two partition passes took
        // 2.2 + 4.3 ms instead of 0.15 + 0.55 and the scatter pass beside them 7.8 ms instead of 2 (profiles/r03_ordering.md).
        // Beside a tag pass the ordering kernels crawl (a partition pass 1.7-3.9 ms instead of 0.13: every memory access
        // queues behind the tag pass's line gathers) while the tag pass hardly notices them.  KG_ORDER_STREAMS=n (1..4; not
        // the default) gives the chunks' orderings n streams of their own, of the LOWEST priority because that gives them
        // hardware queues of their own (a fourth stream of normal priority shares a queue with the third): the orderings
        // of chunks 0-2 then all crawl beside the last tag passes, single scans 20.1-20.25 ms against 20.4, but twenty
        // scans back to back (bench.py) 21.45 against 21.23 ms per step (profiles/r03_experiments.md).
        for (uint32_t k = 0; k < pl.n_os; k++)
            if (!t->ostream[k]) {
                int pr_least = 0, pr_greatest = 0;
                HIP_TRY(hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
                HIP_TRY(hipStreamCreateWithPriority(&t->ostream[k], hipStreamNonBlocking, pr_least));
            }
        for (uint32_t c = 0; c < n_chunks; c++)
            if ((rc = chunk_order<AA>(cx, pl, pb, chunk_view(pl, pb, c), hits_cap))) return rc;

        for (uint32_t k = 0; k < pl.n_os; k++) {
            HIP_TRY(hipEventRecord(t->pev[kPevOrdered + k], t->ostream[k]));
            HIP_TRY(hipStreamWaitEvent(t->stream, t->pev[kPevOrdered + k], 0));
        }
        HIP_TRY(hipEventRecord(t->pev[kPevJoin2], t->stream2));              // join
        HIP_TRY(hipStreamWaitEvent(t->stream, t->pev[kPevJoin2], 0));
        HIP_TRY(hipEventRecord(t->pev[kPevJoin3], t->stream3));
        HIP_TRY(hipStreamWaitEvent(t->stream, t->pev[kPevJoin3], 0));
        HIP_TRY(hipEventRecord(t->ev[kEvJoined], t->stream));
        st.scan_launches++;
        HIP_TRY(hipEventRecord(t->ev[kEvScanEnd], t->stream));                 // end of the scan stage (of this attempt)
        if (pl.early_totals) {
            HIP_TRY(hipEventSynchronize(t->pev[kPevTotals]));                 // (the ordering of the last chunk may still be running)
        } else {
            if ((rc = send_counters(t, pb.d_pc, pb.d_ovfc, cx.d_totals, t->stream))) return rc;
            HIP_TRY(hipStreamSynchronize(t->stream));
        }
        const uint64_t *h_pc = t->h_pin + kPinPc;
        const uint32_t *h_ovf = reinterpret_cast<const uint32_t *>(t->h_pin + kPinOvf);
        uint64_t need_u = 0, need_c = 0;
        uint32_t max_ovf = 0, guard = 0;
        for (uint32_t c = 0; c < n_chunks; c++) {
            need_u = std::max(need_u, h_pc[kPcUcur + c]); need_c = std::max(need_c, h_pc[kPcCcur + c]);
            max_ovf = std::max(max_ovf, h_ovf[kOvfWords * c + kOvfGroups]);
            guard |= h_ovf[kOvfWords * c + kOvfGuard];
        }
        const uint64_t n_hits = h_pc[kPcBase + n_chunks];
        if (pl.debug)
            fprintf(stderr, "[kg] partition attempt %d: %u chunks (largest %llu of %llu blocks), overflow groups <= %u (cap %u), hit list <= %llu "
                            "(cap %llu), candidates <= %llu (cap %llu), regions/chunk %llu x %u entries, %u buckets, shift %u, %u scatter "
                            "workgroups, hits %llu, %s\n",
                    attempt, n_chunks, (unsigned long long)pl.max_chunk, (unsigned long long)nblocks, max_ovf, pl.ovf_cap,
                    (unsigned long long)need_u, (unsigned long long)ucap, (unsigned long long)need_c, (unsigned long long)ccap,
                    (unsigned long long)pl.n_regions, pl.cap, pl.buckets, pl.shift, pl.n_wg, (unsigned long long)n_hits, pl.use_bidx ? "byte home index" : "tags");
        const bool redo = guard || max_ovf > pl.ovf_cap || need_u > ucap || need_c > ccap;
        if (redo && pl.early_totals) HIP_TRY(hipStreamSynchronize(t->stream));   // the attempt is thrown away: its last kernels first
        if (guard || max_ovf > pl.ovf_cap) {
            // the scatter pass's spin guard fired (2), or more overflow than provisioned (1): direct path
            st.fallback = guard ? 2 : 1;
            lists.release();
            drop_hits(t, res);
            return KG_OK;
        }
        if (!redo) {
            note_totals(cx, n_hits, pl.part_counters);
            st.partitioned = 1;
            st.part_chunks = (int32_t)n_chunks; st.part_buckets = (int32_t)pl.buckets; st.part_shift = (int32_t)pl.shift;
            st.part_levels = pl.use_bidx ? 4 : 1;
            done = true;
            return KG_OK;
        }
        // a list was too small: now the exact need is known (masks are cleared and everything is redone; all streams are
        // idle, and the ordering buffers are sized by ucap as well)
        lists.release();
        drop_hits(t, res);
        if (attempt == 2) break;
        // which wave fills which reservation chunk differs from run to run: one partly used chunk per wave on top
        if (need_c > ccap) { pb.ccap = (need_c + pl.list_slack + kg::kUChunk - 1) / kg::kUChunk * kg::kUChunk; pb.ucap = std::max(ucap, pb.ccap); }   // hits <= candidates
        else pb.ucap = (need_u + pl.list_slack + kg::kUChunk - 1) / kg::kUChunk * kg::kUChunk;
    }
    return fail(KG_ERR_DEVICE, "hit list overflow after resize (internal error)");
}

// The direct strategy: encode + probe + staged compaction, then ordered placement; re-run once if the staging area was too small.
template <bool AA>
int scan_direct(ScanCtx &cx, const DirectPlan &pl)
{
    kg_table *t = cx.t;
    kg_result *res = cx.res;
    kg_stats &st = res->st;
    const uint64_t nblocks = cx.b.nblocks, n_rows = cx.b.n_rows;
    int rc;
    st.scan_launches = 0;
    // (the whole batch, when the partitioned strategy did not run or fell back before uploading everything)
    if (!cx.seq_uploaded) { if ((rc = upload_seq(cx, cx.offsets[0], cx.offsets[cx.n_seqs]))) return rc; cx.seq_uploaded = true; }
    uint64_t stage_cap = pl.stage_cap;
    kg_hit *d_stage = nullptr;
    uint32_t *d_stage_slot = nullptr;                                        // KG_F_PROGRESS: the found slots, parallel to d_stage
    BlockGuard<2> stage{cx.sc, {(void **)&d_stage, (void **)&d_stage_slot}};
    unsigned long long *d_cursor = (unsigned long long *)(cx.d_totals + kTotCursor);
    unsigned long long *d_ctr = (unsigned long long *)(cx.d_totals + kTotValid);
    for (int attempt = 0;; attempt++) {
        if ((rc = dalloc(t, (void **)&d_stage, stage_cap * sizeof(kg_hit)))) return rc;
        if (cx.progress && (rc = dalloc(t, (void **)&d_stage_slot, stage_cap * 4))) return rc;
        HIP_TRY(hipMemsetAsync(cx.d_totals, 0, kTotWords * 8, t->stream));
        HIP_TRY(hipEventRecord(t->ev[kEvScanBegin], t->stream));
        if (nblocks) {
            const uint64_t wgs = (nblocks + kg::kWavesPerWG - 1) / kg::kWavesPerWG;
            const uint32_t grid = (uint32_t)(wgs < pl.scan_grid ? wgs : pl.scan_grid);      // persistent waves stride over the blocks
            dispatch<bool, true, false>(cx.counters, [&](auto counters) {
                dispatch<int, 1, 2, 3, 6>((int)pl.rpg, [&](auto rpg) {
                    constexpr bool COUNTERS = decltype(counters)::value;
                    constexpr int RPG = AA ? 1 : decltype(rpg)::value;           // (a protein block has one row)
                    hipLaunchKernelGGL((kg::scan_kernel<AA, COUNTERS, RPG>), dim3(grid), dim3(kg::kWave * kg::kWavesPerWG), 0, t->stream,
                                       t->d_entries, t->d_tags, t->limit, (uint64_t)t->num_sigs, t->magic, t->m35, cx.d_seq, cx.d_blocks,
                                       (uint32_t)nblocks, cx.d_counts, cx.d_bsb, d_stage, d_cursor, stage_cap, pl.stage_chunk, d_ctr, cx.d_prog,
                                       d_stage_slot, pl.d_hbits, t->tail_start);
                });
            });
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(t->ev[kEvScanEnd], t->stream));
        st.scan_launches++;
        if ((rc = prefix_sum(t, cx.d_counts, n_rows, cx.d_offs, cx.d_partial, cx.d_totals + kTotHits))) return rc;
        if ((rc = send_counters(t, nullptr, nullptr, cx.d_totals, t->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(t->stream));
        const uint64_t need = t->h_pin[kPinTotals + kTotCursor];
        if (need <= stage_cap) break;
        // staging overflow: now the exact need is known
        stage.release();
        if (attempt == 1) return fail(KG_ERR_DEVICE, "staging overflow after resize (internal error)");
        stage_cap = need;
    }
    const uint64_t n_hits = n_rows ? t->h_pin[kPinTotals + kTotHits] : 0;
    note_totals(cx, n_hits, cx.counters);

    // ---- ordered placement ----
    if ((rc = dalloc(t, (void **)&res->d_hits, n_hits * sizeof(kg_hit)))) return rc;
    if (cx.progress && (rc = dalloc(t, (void **)&res->d_hit_slots, (n_hits ? n_hits : 1) * 4))) return rc;
    if (nblocks) {
        const uint32_t grid = (uint32_t)((nblocks + kg::kWavesPerWG - 1) / kg::kWavesPerWG);
        hipLaunchKernelGGL((kg::place_kernel<AA>), dim3(grid), dim3(kg::kWave * kg::kWavesPerWG), 0, t->stream, cx.d_blocks,
                           (uint32_t)nblocks, cx.d_counts, cx.d_offs, cx.d_bsb, pl.rpg, d_stage, res->d_hits, d_stage_slot, res->d_hit_slots);
    }
    return KG_OK;
}

// One batch: plan, the shared buffers, one of the two strategies, then container starts, aggregation and the timings.
template <bool AA>
int scan_impl(kg_table *t, const kg_params *p, const uint8_t *d_seq, const uint8_t *h_seq /* host copy still to upload, or null */,
              const int64_t *offsets, int64_t n_seqs, kg_result *res)
{
    constexpr uint32_t PER = AA ? 1 : 6;
    const bool progress = (p->flags & KG_F_PROGRESS) != 0;
    const bool counters_req = (p->flags & KG_F_COUNTERS) != 0;
    const bool aggregate = !(p->flags & KG_F_SKIP_AGGREGATE);
    kg_stats &st = res->st;
    res->per = PER;
    int rc;

    BatchPlan b;
    if ((rc = plan_batch<AA>(offsets, n_seqs, b))) return rc;
    const uint64_t nblocks = b.nblocks, n_rows = b.n_rows, n_cont = b.n_cont;
    st.n_seqs = n_seqs; st.n_containers = (int64_t)n_cont; st.n_blocks = (int64_t)nblocks;
    st.residues = (int64_t)b.residues; st.windows = (int64_t)b.windows;
    st.table_bytes = t->num_sigs * (int64_t)KG_TABLE_ENTRY_SIZE;

    // ---- the buffers both strategies use, the offsets, the window blocks ----
    Scratch sc(t);
    // the walks are noted by the counting kernels -- except on the partitioned path's byte home index (PartPlan::prog_index)
    ScanCtx cx{t, res, sc, b, d_seq, h_seq, offsets, n_seqs, progress, counters_req || progress, h_seq == nullptr};
    if ((rc = sc.get(&cx.d_off, (size_t)n_seqs + 1))) return rc;
    if ((rc = sc.get(&cx.d_ibase, (size_t)n_seqs + 1))) return rc;
    HIP_TRY(hipMemcpyAsync(cx.d_off, offsets, ((size_t)n_seqs + 1) * 8, hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(cx.d_ibase, b.ibase.data(), ((size_t)n_seqs + 1) * 4, hipMemcpyHostToDevice, t->stream));
    if ((rc = sc.get(&cx.d_blocks, nblocks))) return rc;
    if ((rc = sc.get(&cx.d_counts, n_rows))) return rc;
    if ((rc = sc.get(&cx.d_offs, n_rows))) return rc;
    if ((rc = sc.get(&cx.d_bsb, nblocks * 6))) return rc;      // one staging base per (block, row group)
    if ((rc = sc.get(&cx.d_partial, (size_t)(std::max(n_rows, n_cont) / kg::kScanChunk + 2)))) return rc;
    if ((rc = sc.get(&cx.d_totals, kTotWords))) return rc;
    HIP_TRY(hipMemsetAsync(cx.d_totals, 0, kTotWords * 8, t->stream));
    if ((rc = dalloc(t, (void **)&res->d_chs, (n_cont + 1) * 8))) return rc;
    if (progress && (rc = progress_begin(cx))) return rc;
    HIP_TRY(hipEventRecord(t->ev[kEvBegin], t->stream));
    if (nblocks) {
        hipLaunchKernelGGL(kg::build_blocks_kernel, dim3((uint32_t)((nblocks + 255) / 256)), dim3(256), 0, t->stream,
                           cx.d_off, cx.d_ibase, (uint32_t)n_seqs, (uint32_t)nblocks, cx.d_blocks);
        HIP_TRY(hipGetLastError());
    }

    // ---- strategy: partitioned probing where it applies and pays, else (or when the batch turns out too skewed) direct ----
    st.scan_launches = 0;
    PartPlan part;
    if ((rc = plan_partition<AA>(t, b, progress, counters_req, part))) return rc;
    bool part_done = false;
    if (part.applicable && (rc = scan_partitioned<AA>(cx, part, part_done))) return rc;
    if (!part_done && (rc = scan_direct<AA>(cx, plan_direct<AA>(t, b, cx.counters)))) return rc;

    if (progress && (rc = progress_finish(cx, part_done && part.prog_index))) return rc;
    hipLaunchKernelGGL((kg::container_starts_kernel<AA>), dim3((uint32_t)((n_cont + 1 + 255) / 256)), dim3(256), 0, t->stream,
                       cx.d_ibase, (uint32_t)n_seqs, cx.d_offs, n_rows, cx.d_totals, res->d_chs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t->ev[kEvOrderEnd], t->stream));

    // ---- aggregation: CALL records and OTU votes ----
    if (aggregate && (rc = aggregate_stage(t, p, res, sc, n_seqs, n_cont, cx.n_hits, PER, cx.d_partial, cx.d_totals, nullptr, b.longest < (1ll << 30),
                                         plan_aggregate())))
        return rc;
    HIP_TRY(hipEventRecord(t->ev[kEvAggEnd], t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    st.n_calls = aggregate ? (int64_t)t->h_pin[kPinCalls] : 0;
    if (progress && (rc = progress_fetch(cx))) return rc;
    st.agg_pieces = aggregate ? (int32_t)std::min<uint64_t>(t->h_pin[kPinPieces], 0x7FFFFFFF) : 0;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, t->ev[kEvScanBegin], t->ev[kEvScanEnd])); st.ms_scan = ms;
    HIP_TRY(hipEventElapsedTime(&ms, t->ev[kEvScanEnd], t->ev[kEvOrderEnd])); st.ms_order = ms;
    HIP_TRY(hipEventElapsedTime(&ms, t->ev[kEvOrderEnd], t->ev[kEvAggEnd])); st.ms_aggregate = ms;
    HIP_TRY(hipEventElapsedTime(&ms, t->ev[kEvBegin], t->ev[kEvAggEnd])); st.ms_total = ms;
    if (st.partitioned) {
        // the passes of different chunks overlap: "scatter" = until the last chunk is scattered, "tail" = what is left
        // of the tag / verify passes after that; ms_part_tag is kept for layout compatibility
        HIP_TRY(hipEventElapsedTime(&ms, t->ev[kEvScanBegin], t->ev[kEvScattered])); st.ms_part_scatter = ms;
        st.ms_part_tag = 0;
        HIP_TRY(hipEventElapsedTime(&ms, t->ev[kEvScattered], t->ev[kEvJoined])); st.ms_part_verify = ms;
    }
    return KG_OK;
}

int scan_entry(kg_table *t, const kg_params *p, const uint8_t *seq, bool on_device, const int64_t *offsets, int64_t n_seqs,
               kg_result **out)
{
    if (!t || !p || !offsets || !out || n_seqs < 0) return fail(KG_ERR_ARG, "null or negative argument");
    if (n_seqs > 0x7FFFFFF0ll / 6) return fail(KG_ERR_LIMIT, "too many sequences in one batch");
    if (p->min_hits < 2)
        return fail(KG_ERR_UNSUPPORTED, "minHits < 2: the reference throws in processSetOfHits (KGJ:442); refusing");
    // One scan at a time per table: the streams, events, pinned counter words and the block cache's "freed when the
    // stream is idle" rule are per table.  A second thread is turned away instead of corrupting them.
    CallScope cs(t, "another kg_scan* is in flight on this kg_table (one scan at a time per table; open a second table "
                    "object for concurrent scans)");
    if (cs.rc) return cs.rc;
    int64_t total = offsets[n_seqs] - offsets[0];
    if (total < 0) return fail(KG_ERR_ARG, "offsets must be non-decreasing");
    if (!seq && total > 0) return fail(KG_ERR_ARG, "null sequence buffer");
    kg_result *r = new (std::nothrow) kg_result();
    if (!r) return fail(KG_ERR_NOMEM, "out of host memory");
    r->tab = t;
    uint8_t *d_seq = nullptr;
    int rc = KG_OK;
    if (!on_device) {
        size_t end = (size_t)offsets[n_seqs];
        rc = dalloc(t, (void **)&d_seq, end + 16);       // filled by scan_impl (upload overlapped with the scan where possible)
    }
    if (rc == KG_OK) {
        const uint8_t *s = on_device ? seq : d_seq;
        const uint8_t *h = on_device ? nullptr : seq;
        rc = p->aa ? scan_impl<true>(t, p, s, h, offsets, n_seqs, r) : scan_impl<false>(t, p, s, h, offsets, n_seqs, r);
    }
    (void)hipStreamSynchronize(t->stream);
    if (d_seq) dfree(t, d_seq);
    if (rc != KG_OK) return fail_and_free(r, rc);
    *out = r;
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_scan(kg_table *t, const kg_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_seqs, kg_result **out)
{
    return scan_entry(t, p, seq, false, offsets, n_seqs, out);
}

int kg_scan_device(kg_table *t, const kg_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_seqs,
                   kg_result **out)
{
    return scan_entry(t, p, d_seq, true, offsets, n_seqs, out);
}

}  // extern "C"
