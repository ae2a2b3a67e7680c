// kg_host_cluster.hpp -- kg_proteins_cluster / kg_proteins_cluster_device: proteins -> families by shared 8-mers (kernels:
// kg_cluster.hpp; the window encode, the sort and the collapse are the derive call's, kg_derive.hpp).
// kg_proteins_cluster_aligned / _device: the same with the alignment step of kg_host_align.hpp between the edge test and the rounds.
// kg_proteins_cluster_masked / _device: either of them with the window kernels reading the seeding copy of kg_host_mask.hpp.
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_derive.hpp (its front half is that file's: the block
// counts, the staging, the histogram, the one-pass cap and the window-pairs pass) and kg_host_align.hpp.
#pragma once

struct kg_familyset {
    int device = 0;
    Detached d_fam;                     // count * 16 bytes
    int64_t count = 0;
    kg_cluster_stats st = {};
    // a set made with alignment: one record per link that passed the 8-mer tests
    bool aligned = false;
    Detached d_edges;                   // n_edges * 32 bytes
    int64_t n_edges = 0;
    kg_align_stats ast = {};
    bool has_mask = false;              // kg_proteins_cluster_masked only: the statistics of the mask behind the seeding copy
    kg_mask_stats mst = {};
};

static_assert(sizeof(kg_family) == 16 && sizeof(kg_cluster_params) == 12, "record layouts of include/kmerguts_hip.h");

namespace {

// al: null for kg_proteins_cluster; else the links that pass the 8-mer tests are aligned and the cut ones lose their edge.
// mask: null for no masking; else the window kernels read the seeding copy of kg_host_mask.hpp, the alignment the original
int cluster_impl(kg_table *t, const kg_cluster_params *prm, const kg_align_params *al, const uint8_t *h_seq, const uint8_t *d_seq_in,
                 const int64_t *offsets, int64_t n_prot, int64_t max_windows, kg_familyset *set, const MaskPlan *mask = nullptr)
{
    set->aligned = al != nullptr;
    kg_cluster_stats &st = set->st;
    std::vector<uint32_t> ibase;
    uint64_t nblocks = 0, windows = 0;
    int rc;
    if ((rc = derive_block_bases(offsets, n_prot, ibase, &nblocks, &windows))) return rc;
    st.proteins = n_prot;
    const uint32_t b = bits_for((uint64_t)n_prot), np = (uint32_t)n_prot;
    hipStream_t s = t->stream;

    Scratch sc(t);
    Events<10> ev;
    if ((rc = ev.create())) return rc;
    const uint8_t *d_seq = nullptr;
    if ((rc = stage_sequence(t, sc, h_seq, d_seq_in, n_prot ? (uint64_t)offsets[n_prot] : 0, &d_seq))) return rc;
    HIP_TRY(hipEventRecord(ev[0], s));
    unsigned long long *words = nullptr;
    uint64_t *d_tot = nullptr;
    if ((rc = sc.get(&words, kg::kClusterWords)) || (rc = sc.get(&d_tot, 4))) return rc;
    HIP_TRY(hipMemsetAsync(words, 0, kg::kClusterWords * 8, s));
    // ---- the result array: the set's from here on (detached: a set that is freed after a failure frees it, the cache does not) ----
    if ((rc = dalloc_detached(t, &set->d_fam.p, std::max<uint64_t>((uint64_t)n_prot * 16, 16)))) return rc;
    if (n_prot == 0) {
        HIP_TRY(hipEventRecord(ev[5], s));
        HIP_TRY(hipStreamSynchronize(s));
        st.ms_total = ev.ms(0, 5);
        set->has_mask = mask != nullptr;
        return KG_OK;
    }

    const uint8_t *d_seed = d_seq;
    if (mask) {
        if ((rc = mask_seeding_copy(t, sc, *mask, d_seq, offsets, 0, n_prot, (uint64_t)offsets[n_prot], &d_seed, &set->mst))) return rc;
        set->has_mask = true;
    }

    // ---- per-protein arrays, the window blocks ----
    Deriver dv{t, sc, d_seed};
    dv.ev[0] = ev[6]; dv.ev[1] = ev[7];
    int64_t *d_off = nullptr;
    uint32_t *rank_of = nullptr, *parent = nullptr, *d_cnt = nullptr, *size = nullptr, *root = nullptr, *rflag = nullptr,
             *fx = nullptr;
    unsigned long long *best = nullptr;
    uint64_t *fpartial = nullptr;
    if ((rc = sc.get(&dv.d_bins, kg::kDeriveBins)) || (rc = dv.window_blocks(offsets, ibase, n_prot, nblocks, &d_off)) ||
        (rc = sc.get(&rank_of, (size_t)n_prot)) || (rc = sc.get(&parent, (size_t)n_prot)) || (rc = sc.get(&d_cnt, (size_t)n_prot)) ||
        (rc = sc.get(&size, (size_t)n_prot)) || (rc = sc.get(&root, (size_t)n_prot)) || (rc = sc.get(&rflag, (size_t)n_prot)) ||
        (rc = sc.get(&fx, (size_t)n_prot)) || (rc = sc.get(&best, (size_t)n_prot)) ||
        (rc = sc.get(&fpartial, (size_t)n_prot / kg::kScanChunk + 3)))
        return rc;
    hipLaunchKernelGGL(kg::cluster_init_kernel, dim3(grid_of(n_prot)), dim3(256), 0, s, np, rank_of, parent, d_cnt, size, best);
    HIP_TRY(hipGetLastError());

    // ---- the valid windows, and whether they fit: one pass ----
    const uint64_t space = (uint64_t)KG_MAX_ENCODED;
    std::vector<unsigned long long> bins;
    if ((rc = dv.histogram(0, space, Deriver::shift_for(space), bins))) return rc;
    uint64_t n = 0;
    for (auto c : bins) n += c;
    st.valid_windows = (int64_t)n;
    if ((rc = windows_fit_one_pass(n, max_windows))) return rc;

    uint64_t P = 0, K = 0, NL = 0, ND = 0;
    uint64_t *edge = nullptr;
    const uint32_t *lstart_all = nullptr;
    HIP_TRY(hipEventRecord(ev[1], s));
    HIP_TRY(hipEventRecord(ev[2], s));
    HIP_TRY(hipEventRecord(ev[3], s));
    if (n > 0) {
        // ---- encode and emit (key = v << b | p), sort, collapse to the distinct pairs: the derive call's kernels ----
        WindowPairs w;
        unsigned long long *d_cur = nullptr;
        if ((rc = sc.get(&d_cur, 1)) || (rc = dv.window_pairs(sc, n, 0, space, nullptr, rank_of, b, d_cur, d_tot + 0, ev[1], ev[2], ev[3], &w)))
            return rc;
        P = w.P;
        uint64_t *const pk = w.pk, *const partial = w.partial;
        // ---- d_p, the k-mer runs and their centres (flags / pidx / partial are reused: P <= n) ----
        uint32_t *kh = w.flags, *kx = w.pidx, *lf = w.pv, *lx = nullptr;
        unsigned long long *kbest = nullptr;
        if ((rc = sc.get(&lx, P))) return rc;
        hipLaunchKernelGGL(kg::cluster_pair_kernel, dim3(grid_of(P)), dim3(256), 0, s, pk, P, b, np, kh, d_cnt);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, kh, P, kx, partial, d_tot + 1))) return rc;
        HIP_TRY(hipMemcpyAsync(&K, d_tot + 1, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if ((rc = sc.get(&kbest, K))) return rc;
        HIP_TRY(hipMemsetAsync(kbest, 0, K * 8, s));
        hipLaunchKernelGGL(kg::cluster_centre_kernel, dim3(grid_of((P + kg::kDeriveChunk - 1) / kg::kDeriveChunk)), dim3(256), 0, s, pk, P, b, np,
                           d_off, kh, kx, kbest);
        // ---- the links: every pair beside its run's centre (the collapse's values are not needed any more: lf reuses pv) ----
        hipLaunchKernelGGL(kg::cluster_link_flags_kernel, dim3(grid_of(P)), dim3(256), 0, s, pk, P, b, kh, kx, kbest, lf);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, lf, P, lx, partial, d_tot + 2))) return rc;
        HIP_TRY(hipMemcpyAsync(&NL, d_tot + 2, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (NL > 0) {
            // the window sort's buffers are free: the link keys go there (NL <= P <= n)
            SortPairs lk;
            lk.k[0] = w.sp.keys(); lk.v[0] = w.sp.vals();
            hipLaunchKernelGGL(kg::cluster_link_emit_kernel, dim3(grid_of(P)), dim3(256), 0, s, pk, P, b, kh, kx, kbest, lf, lx, NL, lk.keys(),
                               lk.vals());
            HIP_TRY(hipGetLastError());
            if ((rc = lk.sort(t, sc, NL, 32 + b))) return rc;
            // runs of equal keys = distinct links (kh / kx are free from here on: NL <= P)
            uint32_t *lh = kh, *lr = kx, *lstart = nullptr;
            hipLaunchKernelGGL(kg::derive_key_heads_kernel, dim3(grid_of(NL)), dim3(256), 0, s, lk.keys(), NL, lh);
            HIP_TRY(hipGetLastError());
            if ((rc = prefix_sum(t, lh, NL, lr, partial, d_tot + 3))) return rc;
            HIP_TRY(hipMemcpyAsync(&ND, d_tot + 3, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if ((rc = sc.get(&lstart, ND + 1)) || (rc = sc.get(&edge, ND))) return rc;
            lstart_all = lstart;
            hipLaunchKernelGGL(kg::cluster_link_starts_kernel, dim3(grid_of(NL)), dim3(256), 0, s, lh, lr, NL, d_tot + 3, lstart);
            hipLaunchKernelGGL(kg::cluster_edge_kernel, dim3(grid_of(ND)), dim3(256), 0, s, lk.keys(), lstart, ND, np, d_cnt,
                               (int64_t)prm->min_shared, (int64_t)prm->min_cover_pct, edge, best, words);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(ev[4], s));

    // ---- the alignment step: the passing links compacted (ascending (m, c): the links' order), aligned, cut; best made again ----
    unsigned long long *tally = nullptr;
    AlignTotals atot;
    uint64_t NP = 0;
    if (al && ND > 0) {
        std::vector<uint64_t> h_edge(ND);
        std::vector<uint32_t> h_lstart(ND + 1);
        HIP_TRY(hipMemcpyAsync(h_edge.data(), edge, ND * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h_lstart.data(), lstart_all, (ND + 1) * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<int32_t> h_pairs, h_shared;
        std::vector<uint32_t> h_ridx;
        for (uint64_t r = 0; r < ND; r++) {
            if (h_edge[r] == kg::kClusterNoEdge) continue;
            h_pairs.push_back((int32_t)(h_edge[r] >> 32));
            h_pairs.push_back((int32_t)(uint32_t)h_edge[r]);
            h_shared.push_back((int32_t)(h_lstart[r + 1] - h_lstart[r]));
            h_ridx.push_back((uint32_t)r);
        }
        NP = h_ridx.size();
        if (NP > 0) {
            const int32_t *d_pairs = nullptr;
            kg::AlignRec *d_aln = nullptr;
            int32_t *d_shared = nullptr;
            uint32_t *d_ridx = nullptr;
            if ((rc = align_run(t, sc, al, d_seq, d_off, offsets, h_pairs.data(), NP, &d_pairs, &d_aln, &atot))) return rc;
            if ((rc = sc.get(&d_shared, NP)) || (rc = sc.get(&d_ridx, NP)) || (rc = sc.get(&tally, 2)) ||
                (rc = dalloc_detached(t, &set->d_edges.p, NP * sizeof(kg_family_edge))))
                return rc;
            HIP_TRY(hipMemcpyAsync(d_shared, h_shared.data(), NP * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_ridx, h_ridx.data(), NP * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemsetAsync(best, 0, (size_t)n_prot * 8, s));
            HIP_TRY(hipMemsetAsync(words + kg::kClusterEdges, 0, 8, s));
            HIP_TRY(hipMemsetAsync(tally, 0, 16, s));
            hipLaunchKernelGGL(kg::align_cut_kernel, dim3(grid_of(NP)), dim3(256), 0, s, d_pairs, d_aln, d_shared, d_ridx, NP,
                               (int64_t)al->min_ratio_pct, (int)(al->ref == KG_ALIGN_REF_MEMBER), edge, best, words, tally,
                               (int4 *)set->d_edges.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s));           // (the host vectors above are the copies' sources)
        }
    }
    if (al) HIP_TRY(hipEventRecord(ev[8], s));

    // ---- connected components: hook and jump while the flag says something changed ----
    uint32_t rounds = 0;
    for (bool changed = ND > 0; changed;) {
        if (rounds > np) return fail(KG_ERR_DEVICE, "internal: the component rounds did not settle");
        HIP_TRY(hipMemsetAsync(words + kg::kClusterChanged, 0, 8, s));
        hipLaunchKernelGGL(kg::cluster_hook_kernel, dim3(grid_of(ND)), dim3(256), 0, s, edge, ND, parent, words);
        hipLaunchKernelGGL(kg::cluster_jump_kernel, dim3(grid_of(n_prot)), dim3(256), 0, s, np, parent, words);
        HIP_TRY(hipGetLastError());
        unsigned long long flag = 0;
        HIP_TRY(hipMemcpyAsync(&flag, words + kg::kClusterChanged, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        changed = flag != 0;
        rounds++;
    }
    hipLaunchKernelGGL(kg::cluster_compress_kernel, dim3(grid_of(n_prot)), dim3(256), 0, s, np, parent, root, size, rflag);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, rflag, (uint64_t)n_prot, fx, fpartial, d_tot + 0))) return rc;
    hipLaunchKernelGGL(kg::cluster_emit_kernel, dim3(grid_of(n_prot)), dim3(256), 0, s, np, root, fx, size, best, (int4 *)set->d_fam.p, words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[5], s));
    unsigned long long hw[kg::kClusterWords] = {}, ht[2] = {};
    uint64_t families = 0;
    HIP_TRY(hipMemcpyAsync(hw, words, sizeof hw, hipMemcpyDeviceToHost, s));
    if (tally) HIP_TRY(hipMemcpyAsync(ht, tally, sizeof ht, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&families, d_tot, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.pairs = (int64_t)P;
    st.kmers = (int64_t)K;
    st.links = (int64_t)ND;
    st.edges = (int64_t)hw[kg::kClusterEdges];
    st.families = (int64_t)families;
    st.families_multi = (int64_t)hw[kg::kClusterMulti];
    st.largest = (int64_t)hw[kg::kClusterLargest];
    st.rounds = (int32_t)rounds;
    st.ms_encode = dv.ms_hist + ev.ms(1, 2);
    st.ms_sort = ev.ms(2, 3);
    st.ms_link = ev.ms(3, 4);
    st.ms_components = ev.ms(al ? 8 : 4, 5);
    st.ms_total = ev.ms(0, 5);
    if (al) {
        if ((int64_t)ht[1] != atot.skipped) return fail(KG_ERR_DEVICE, "internal: the device and the host skipped different pairs");
        set->ast.aligned = (int64_t)NP - atot.skipped;
        set->ast.cut = (int64_t)ht[0];
        set->ast.skipped = atot.skipped;
        set->ast.cells = atot.cells;
        set->ast.ms_align = ev.ms(4, 8);
        set->n_edges = (int64_t)NP;
    }
    set->count = n_prot;
    return KG_OK;
}

int cluster_entry(int device, const kg_cluster_params *prm, const kg_align_params *al, const uint8_t *h_seq, const uint8_t *d_seq,
                  const int64_t *offsets, int64_t n_prot, int64_t max_windows, kg_familyset **out,
                  std::optional<const kg_mask_params *> mask = std::nullopt)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!prm) return fail(KG_ERR_ARG, "null kg_cluster_params");
    if (prm->min_shared < 1) return fail(KG_ERR_ARG, "min_shared must be >= 1");
    if (prm->min_cover_pct < 0 || prm->min_cover_pct > 100) return fail(KG_ERR_ARG, "min_cover_pct must be in 0..100");
    if (prm->reserved != 0) return fail(KG_ERR_ARG, "kg_cluster_params.reserved must be 0");
    if (al) if (int rc = align_check_params(al)) return rc;
    MaskPlan mplan;
    if (mask) if (int rc = mask_plan(*mask, &mplan)) return rc;
    if (max_windows < 0) return fail(KG_ERR_ARG, "max_windows must be >= 0");
    if (n_prot < 0) return fail(KG_ERR_ARG, "n_prot < 0");
    if (n_prot >= (1ll << 29)) return fail(KG_ERR_LIMIT, "2^29 or more proteins in one call");
    if (int rc = al ? check_protein_offsets(offsets, n_prot, (int64_t)kg::kAlignMaxLen, "2^24")      // (aligned: the smaller limit)
                    : check_protein_offsets(offsets, n_prot, 1ll << 31, "2^31"))
        return rc;
    const uint64_t seq_bytes = n_prot ? (uint64_t)offsets[n_prot] : 0;
    if (seq_bytes && !h_seq && !d_seq) return fail(KG_ERR_ARG, "null sequence");
    CallScope cs(device);               // the call's context: closed when the call returns, the set keeps only its records
    if (cs.rc) return cs.rc;
    kg_familyset *set = new (std::nothrow) kg_familyset();
    if (!set) return fail(KG_ERR_NOMEM, "out of host memory");
    set->device = device;
    int rc = d_seq && hipDeviceSynchronize() != hipSuccess ? fail(KG_ERR_DEVICE, "hipDeviceSynchronize failed") : KG_OK;
    if (!rc) rc = cluster_impl(cs.t, prm, al, h_seq, d_seq, offsets, n_prot, max_windows, set, mask ? &mplan : nullptr);
    cs.t->cache.release_all();                          // scratch goes back to the driver
    if (rc) { std::string keep = g_err; kg_familyset_free(set); g_err = keep; return rc; }
    if (getenv("KG_DEBUG"))
        fprintf(stderr, "[kg] kg_proteins_cluster: proteins=%lld valid=%lld pairs=%lld kmers=%lld links=%lld edges=%lld families=%lld multi=%lld largest=%lld rounds=%d encode_ms=%.3f sort_ms=%.3f link_ms=%.3f components_ms=%.3f total_ms=%.3f\n",
                (long long)set->st.proteins, (long long)set->st.valid_windows, (long long)set->st.pairs, (long long)set->st.kmers,
                (long long)set->st.links, (long long)set->st.edges, (long long)set->st.families, (long long)set->st.families_multi,
                (long long)set->st.largest, set->st.rounds, set->st.ms_encode, set->st.ms_sort, set->st.ms_link, set->st.ms_components,
                set->st.ms_total);
    *out = set;
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_proteins_cluster(int device, const kg_cluster_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                        int64_t max_windows, kg_familyset **out)
{
    return cluster_entry(device, p, nullptr, seq, nullptr, offsets, n_prot, max_windows, out);
}

int kg_proteins_cluster_device(int device, const kg_cluster_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                               int64_t max_windows, kg_familyset **out)
{
    return cluster_entry(device, p, nullptr, nullptr, d_seq, offsets, n_prot, max_windows, out);
}

int kg_proteins_cluster_aligned(int device, const kg_cluster_params *p, const kg_align_params *align, const uint8_t *seq,
                                const int64_t *offsets, int64_t n_prot, int64_t max_windows, kg_familyset **out)
{
    return cluster_entry(device, p, align, seq, nullptr, offsets, n_prot, max_windows, out);
}

int kg_proteins_cluster_aligned_device(int device, const kg_cluster_params *p, const kg_align_params *align, const uint8_t *d_seq,
                                       const int64_t *offsets, int64_t n_prot, int64_t max_windows, kg_familyset **out)
{
    return cluster_entry(device, p, align, nullptr, d_seq, offsets, n_prot, max_windows, out);
}

int kg_proteins_cluster_masked(int device, const kg_cluster_params *p, const kg_align_params *align, const uint8_t *seq,
                               const int64_t *offsets, int64_t n_prot, int64_t max_windows, const kg_mask_params *mask, kg_familyset **out)
{
    return cluster_entry(device, p, align, seq, nullptr, offsets, n_prot, max_windows, out, mask);
}

int kg_proteins_cluster_masked_device(int device, const kg_cluster_params *p, const kg_align_params *align, const uint8_t *d_seq,
                                      const int64_t *offsets, int64_t n_prot, int64_t max_windows, const kg_mask_params *mask,
                                      kg_familyset **out)
{
    return cluster_entry(device, p, align, nullptr, d_seq, offsets, n_prot, max_windows, out, mask);
}

int kg_familyset_mask_stats(const kg_familyset *s, kg_mask_stats *out)
{
    if (s && !s->has_mask) return fail(KG_ERR_ARG, "kg_familyset_mask_stats: the set was made without a mask");
    return copy_stats(s, s ? &s->mst : nullptr, out);
}

int64_t kg_familyset_count(const kg_familyset *s) { return s ? s->count : 0; }

int64_t kg_familyset_edges_count(const kg_familyset *s) { return s ? s->n_edges : 0; }

int kg_familyset_edges_copy(const kg_familyset *s, int64_t first, int64_t count, kg_family_edge *dst)
{
    return copy_records(s, s ? s->device : 0, s ? (const kg_family_edge *)s->d_edges.p : nullptr, 1, s ? s->n_edges : 0, first, count, dst,
                        "kg_familyset_edges_copy");
}

int kg_familyset_align_stats(const kg_familyset *s, kg_align_stats *out)
{
    if (s && !s->aligned) return fail(KG_ERR_ARG, "kg_familyset_align_stats: the set was made without alignment");
    return copy_stats(s, s ? &s->ast : nullptr, out);
}

int kg_familyset_copy(const kg_familyset *s, int64_t first, int64_t count, kg_family *dst)
{
    return copy_records(s, s ? s->device : 0, s ? (const kg_family *)s->d_fam.p : nullptr, 1, s ? s->count : 0, first, count, dst, "kg_familyset_copy");
}

int kg_familyset_stats(const kg_familyset *s, kg_cluster_stats *out) { return copy_stats(s, s ? &s->st : nullptr, out); }

void kg_familyset_free(kg_familyset *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;                           // (its blocks with it)
}

}  // extern "C"
