// kg_host_derive.hpp -- kg_signatures_derive / kg_signatures_derive_device: annotated proteins -> a signature set (kernels:
// kg_derive.hpp).  It also holds what the protein hosts behind it share (kg_host_align.hpp, kg_host_cluster.hpp, kg_host_search.hpp):
// the offsets checks, the sequence staging, the cap of a pass, and Deriver with the window blocks, the histogram and the
// window-pairs pass (windows -> sorted keys -> distinct (k-mer, protein) pairs), which the derive call runs once per k-mer range
// and the cluster and search calls once.
// Part of kmerguts_hip.hip's translation unit: one of the batch stages, included behind the kernel headers, kg_host.hpp and the
// hosts of the table, the result and the scan.
#pragma once

struct kg_sigset {
    int device = 0;
    uint8_t *d_sigs = nullptr;          // count * 24 bytes (hipMalloc, owned)
    int64_t count = 0;
    kg_derive_stats st = {};
    bool merged = false;                // made by kg_table_merge_signatures* (kg_host_merge.hpp): mst is valid, st holds only `signatures`
    kg_merge_stats mst = {};
};

static_assert(sizeof(kg_signature) == 24, "record layouts of include/kmerguts_hip.h");

namespace {

constexpr uint64_t kDeriveBytesPerWindow = 160;                       // device bytes one valid window of a pass needs, at most
constexpr uint64_t kDerivePassMax = (1ull << 32) - (1ull << 22);      // the 32-bit scans and indices of one pass

// The offsets checks of a protein batch, the first offender first: offsets[0] < 0, then per protein a decrease (KG_ERR_ARG) or
// max_len or more characters (KG_ERR_LIMIT; max_text says max_len: "2^24" where the proteins are aligned, else "2^31").
int check_protein_offsets(const int64_t *offsets, int64_t n_prot, int64_t max_len, const char *max_text)
{
    if (!offsets) return fail(KG_ERR_ARG, "null offsets");
    if (offsets[0] < 0) return fail(KG_ERR_ARG, "offsets[0] < 0");
    for (int64_t k = 0; k < n_prot; k++) {
        const int64_t L = offsets[k + 1] - offsets[k];
        if (L < 0) return fail(KG_ERR_ARG, "protein " + kmer_text(k) + ": offsets decrease (offsets[p+1] < offsets[p])");
        if (L >= max_len) return fail(KG_ERR_LIMIT, "protein " + kmer_text(k) + ": " + max_text + " or more characters");
    }
    return KG_OK;
}

// the sequence on the device: a host sequence goes to the scratch through pinned pieces, a device sequence is used where it lies
int stage_sequence(kg_table *t, Scratch &sc, const uint8_t *h_seq, const uint8_t *d_seq_in, uint64_t seq_bytes, const uint8_t **d_seq)
{
    *d_seq = d_seq_in;
    if (!h_seq || !seq_bytes) return KG_OK;
    uint8_t *d = nullptr;
    int rc;
    if ((rc = sc.get(&d, seq_bytes)) || (rc = upload_pinned(t, h_seq, seq_bytes, d))) return rc;
    *d_seq = d;
    return KG_OK;
}

// How many items a call holds at once: the caller's max_* figure or, where that is 0, what 0.8 of the free device memory holds at
// bytes_per_item each (2^20 at least); neither goes over `ceiling`, the 32-bit scans and indices.  how: the words a message says
// it with, max_words (" (max_windows)", " (max_pairs)") or the other.
struct Cap { uint64_t items; const char *how; };

int size_cap(int64_t max_items, const char *max_words, uint64_t bytes_per_item, uint64_t ceiling, Cap *out)
{
    uint64_t cap = (uint64_t)max_items;
    if (cap == 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        cap = std::max<uint64_t>(1u << 20, (uint64_t)(free_b * 0.8) / bytes_per_item);
    }
    *out = Cap{std::min(cap, ceiling), max_items ? max_words : " (sized from free device memory)"};
    return KG_OK;
}

// the cluster and search calls run one pass: n valid windows fit it, or the call ends here
int windows_fit_one_pass(uint64_t n, int64_t max_windows)
{
    Cap cap;
    if (int rc = size_cap(max_windows, " (max_windows)", kDeriveBytesPerWindow, kDerivePassMax, &cap)) return rc;
    if (n > cap.items)
        return fail(KG_ERR_LIMIT, kmer_text((int64_t)n) + " valid windows do not fit the one pass of this call, which holds " +
                                      kmer_text((int64_t)cap.items) + cap.how);
    return KG_OK;
}

// Workgroups of a window kernel (derive_windows_kernel, seed_windows_kernel): one wave per block of 64 windows, 16 workgroups per
// CU at most, one at least.  The count launches (histogram, seed_count) run only where n_blocks is not 0, so the "one at least"
// changes nothing for them: they and the emit launch have the same grid.
uint32_t emit_grid(uint32_t n_blocks)
{
    return std::max(std::min<uint32_t>((n_blocks + kg::kWavesPerWG - 1) / kg::kWavesPerWG, 256u * 16), 1u);
}

struct DeriveRange { uint64_t lo, hi, count; };

// What the window-pairs pass gives: pair j < P has key pk[j] = v << b | rank (ascending) and pv[j], the largest value of its windows.
// sp holds the n sorted windows; flags / pidx (n words each) and partial (the chunk sums of a prefix sum over n items) have done
// their work and are the caller's to use again for anything of at most n items.
struct WindowPairs {
    uint64_t n = 0, P = 0;
    uint64_t *pk = nullptr;
    uint32_t *pv = nullptr;
    SortPairs sp;
    uint32_t *flags = nullptr, *pidx = nullptr;
    uint64_t *partial = nullptr;
};

struct Deriver {
    kg_table *t;                        // the call's context: stream, block cache, KG_TEST_FAIL_ALLOC
    Scratch &sc;
    const uint8_t *d_seq;
    kg::BlockDesc *d_blocks = nullptr;
    uint32_t n_blocks = 0;
    unsigned long long *d_bins = nullptr;
    uint64_t cap = 0;
    std::vector<DeriveRange> elems;     // k-mer ranges in order, each within the cap
    hipEvent_t ev[2] = {nullptr, nullptr};
    float ms_hist = 0;

    // counts of the valid windows with k-mers in [lo, hi), in bins of 2^shift k-mers
    int histogram(uint64_t lo, uint64_t hi, uint32_t shift, std::vector<unsigned long long> &out)
    {
        HIP_TRY(hipMemsetAsync(d_bins, 0, kg::kDeriveBins * 8, t->stream));
        HIP_TRY(hipEventRecord(ev[0], t->stream));
        if (n_blocks) {
            hipLaunchKernelGGL(kg::derive_windows_kernel<false>, dim3(emit_grid(n_blocks)), dim3(kg::kDeriveThreads), 0, t->stream, d_seq,
                               d_blocks, n_blocks, lo, hi, shift, d_bins, nullptr, 0u, nullptr, nullptr, nullptr, (uint64_t)0);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(ev[1], t->stream));
        out.assign(kg::kDeriveBins, 0);
        HIP_TRY(hipMemcpyAsync(out.data(), d_bins, kg::kDeriveBins * 8, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        ms_hist += ms;
        return KG_OK;
    }

    static uint32_t shift_for(uint64_t width)
    {
        uint32_t s = 0;
        while (((width - 1) >> s) >= kg::kDeriveBins) s++;
        return s;
    }

    // the range [lo, hi) holds `count` windows: keep it, or cut it finer until every piece fits the cap
    int split(uint64_t lo, uint64_t hi, uint64_t count)
    {
        if (count <= cap) { elems.push_back({lo, hi, count}); return KG_OK; }
        if (hi - lo == 1)
            return fail(KG_ERR_LIMIT, "k-mer " + kmer_text((int64_t)lo) + " alone occurs in " + kmer_text((int64_t)count) +
                                          " valid windows, more than max_windows_per_pass = " + kmer_text((int64_t)cap));
        const uint32_t shift = shift_for(hi - lo);
        std::vector<unsigned long long> bins;
        int rc = histogram(lo, hi, shift, bins);
        if (rc) return rc;
        for (uint64_t i = 0; i < kg::kDeriveBins; i++) {
            const uint64_t a = lo + (i << shift);
            if (a >= hi) break;
            if (bins[i] && (rc = split(a, std::min<uint64_t>(hi, a + (1ull << shift)), bins[i]))) return rc;
        }
        return KG_OK;
    }

    // The per-protein arrays of n_prot >= 1 proteins in the call's scratch: the offsets (*d_off_out) and the block bases (ibase, of
    // derive_block_bases or seed_block_bases) uploaded, and from them the list of the nblocks window blocks (d_blocks, n_blocks).
    int window_blocks(const int64_t *offsets, const std::vector<uint32_t> &ibase, int64_t n_prot, uint64_t nblocks, int64_t **d_off_out)
    {
        int rc;
        int64_t *d_off = nullptr;
        uint32_t *d_ibase = nullptr;
        if ((rc = sc.get(&d_off, (size_t)n_prot + 1)) || (rc = sc.get(&d_ibase, (size_t)n_prot + 1))) return rc;
        if (nblocks && (rc = sc.get(&d_blocks, nblocks))) return rc;
        n_blocks = (uint32_t)nblocks;
        HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)n_prot + 1) * 8, hipMemcpyHostToDevice, t->stream));
        HIP_TRY(hipMemcpyAsync(d_ibase, ibase.data(), ((size_t)n_prot + 1) * 4, hipMemcpyHostToDevice, t->stream));
        if (nblocks) {
            hipLaunchKernelGGL(kg::build_blocks_kernel, dim3(grid_of(nblocks)), dim3(256), 0, t->stream, d_off, d_ibase, (uint32_t)n_prot,
                               (uint32_t)nblocks, d_blocks);
            HIP_TRY(hipGetLastError());
        }
        *d_off_out = d_off;
        return KG_OK;
    }

    // The window-pairs pass: the n >= 1 valid windows with k-mers in [lo, hi) (seed: with seed ids in [0, hi) of that spec, by
    // seed_windows_kernel; lo = 0) are emitted as key = v << b | rank_of[p], sorted, and collapsed into the distinct pairs.  n is
    // what the count pass (the histogram, seed_count) gave for the same range: the emit pass must write as many.  Allocates from
    // `from` (the derive call: the scratch of the pass); d_cur, d_total: one device word each, the emit cursor and where P is
    // summed.  Records e_emit in front of the emit launch, e_sort behind it and e_sorted behind the sort.  One host
    // synchronisation, between the prefix sum and the collapse, where P is read.
    int window_pairs(Scratch &from, uint64_t n, uint64_t lo, uint64_t hi, const kg::SeedSpec *seed, const uint32_t *rank_of, uint32_t b,
                     unsigned long long *d_cur, uint64_t *d_total, hipEvent_t e_emit, hipEvent_t e_sort, hipEvent_t e_sorted, WindowPairs *out)
    {
        hipStream_t s = t->stream;
        WindowPairs &w = *out;
        int rc;
        w.n = n;
        if ((rc = w.sp.alloc(from, n))) return rc;
        HIP_TRY(hipMemsetAsync(d_cur, 0, 8, s));
        HIP_TRY(hipEventRecord(e_emit, s));
        if (seed)
            hipLaunchKernelGGL(kg::seed_windows_kernel<true>, dim3(emit_grid(n_blocks)), dim3(kg::kDeriveThreads), 0, s, d_seq, d_blocks,
                               n_blocks, *seed, nullptr, rank_of, b, w.sp.keys(), w.sp.vals(), d_cur, n);
        else
            hipLaunchKernelGGL(kg::derive_windows_kernel<true>, dim3(emit_grid(n_blocks)), dim3(kg::kDeriveThreads), 0, s, d_seq, d_blocks,
                               n_blocks, lo, hi, 0u, nullptr, rank_of, b, w.sp.keys(), w.sp.vals(), d_cur, n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(e_sort, s));
        if ((rc = w.sp.sort(t, from, n, bit_width(hi - lo - 1) + b))) return rc;
        HIP_TRY(hipEventRecord(e_sorted, s));
        // collapse equal keys into (k-mer, protein) pairs.  (No kernel here or in a caller touches element n of flags / pidx.)
        if ((rc = from.get(&w.flags, n)) || (rc = from.get(&w.pidx, n)) || (rc = from.get(&w.partial, n / kg::kScanChunk + 3))) return rc;
        hipLaunchKernelGGL(kg::derive_key_heads_kernel, dim3(grid_of(n)), dim3(256), 0, s, w.sp.keys(), n, w.flags);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, w.flags, n, w.pidx, w.partial, d_total))) return rc;
        unsigned long long host_cur = 0;
        HIP_TRY(hipMemcpyAsync(&host_cur, d_cur, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&w.P, d_total, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (host_cur != n) return fail(KG_ERR_DEVICE, "internal: the emit pass wrote a different number of windows than the count pass counted");
        if ((rc = from.get(&w.pk, w.P)) || (rc = from.get(&w.pv, w.P))) return rc;
        HIP_TRY(hipMemsetAsync(w.pv, 0, w.P * 4, s));
        hipLaunchKernelGGL(kg::derive_collapse_kernel, dim3(grid_of((n + kg::kDeriveChunk - 1) / kg::kDeriveChunk)), dim3(256), 0, s,
                           w.sp.keys(), w.sp.vals(), n, w.pidx, w.pk, w.pv);
        HIP_TRY(hipGetLastError());
        return KG_OK;
    }
};

// host: block counts (kg_scan's -a trip counts, KGJ:912).  ibase[p] = the first window block of 64 windows of protein p,
// ibase[n_prot] = *nblocks; *windows = sum of max(len_p - 8, 0).  Shared with the cluster and search hosts.
int derive_block_bases(const int64_t *offsets, int64_t n_prot, std::vector<uint32_t> &ibase, uint64_t *nblocks_out, uint64_t *windows_out)
{
    ibase.assign((size_t)n_prot + 1, 0);
    uint64_t nblocks = 0, windows = 0;
    for (int64_t k = 0; k < n_prot; k++) {
        const int64_t L = offsets[k + 1] - offsets[k];
        ibase[(size_t)k] = (uint32_t)nblocks;
        const uint64_t nwin = L >= 9 ? (uint64_t)L - 8 : 0;
        windows += nwin;
        nblocks += (nwin + kg::kAaWinPerBlock - 1) / kg::kAaWinPerBlock;
        if (nblocks > 0x7FFFFFFFull) return fail(KG_ERR_LIMIT, "2^31 or more window blocks of 64 windows in one call");
    }
    ibase[(size_t)n_prot] = (uint32_t)nblocks;
    *nblocks_out = nblocks;
    *windows_out = windows;
    return KG_OK;
}

int derive_impl(kg_table *t, const kg_derive_params *prm, const uint8_t *h_seq, const uint8_t *d_seq_in, const int64_t *offsets,
                int64_t n_prot, const int32_t *fn, const int32_t *otu, kg_sigset *set)
{
    kg_derive_stats &st = set->st;
    std::vector<uint32_t> ibase;
    uint64_t nblocks = 0, windows = 0;
    if (int brc = derive_block_bases(offsets, n_prot, ibase, &nblocks, &windows)) return brc;
    st.proteins = n_prot;
    st.windows = (int64_t)windows;
    const uint32_t b = bits_for((uint64_t)n_prot);

    Scratch sc(t);
    int rc;
    Events<8> ev;
    if ((rc = ev.create())) return rc;

    const uint8_t *d_seq = nullptr;
    if ((rc = stage_sequence(t, sc, h_seq, d_seq_in, n_prot ? (uint64_t)offsets[n_prot] : 0, &d_seq))) return rc;
    HIP_TRY(hipEventRecord(ev[0], t->stream));

    Deriver dv{t, sc, d_seq};
    dv.ev[0] = ev[6]; dv.ev[1] = ev[7];
    if ((rc = sc.get(&dv.d_bins, kg::kDeriveBins))) return rc;
    int32_t *d_fn = nullptr, *d_otu = nullptr, *fn_r = nullptr, *otu_r = nullptr;
    uint32_t *rank_of = nullptr;
    if (n_prot) {
        int64_t *d_off = nullptr;
        if ((rc = sc.get(&d_fn, (size_t)n_prot)) || (rc = sc.get(&d_otu, (size_t)n_prot)) || (rc = sc.get(&fn_r, (size_t)n_prot)) ||
            (rc = sc.get(&otu_r, (size_t)n_prot)) || (rc = sc.get(&rank_of, (size_t)n_prot)))
            return rc;
        HIP_TRY(hipMemcpyAsync(d_fn, fn, (size_t)n_prot * 4, hipMemcpyHostToDevice, t->stream));
        HIP_TRY(hipMemcpyAsync(d_otu, otu, (size_t)n_prot * 4, hipMemcpyHostToDevice, t->stream));
        if ((rc = dv.window_blocks(offsets, ibase, n_prot, nblocks, &d_off))) return rc;
        // ---- rank the proteins by (fn, otu, p): a stable sort of (fn + 1, otu) keys carrying p ----
        HIP_TRY(hipEventRecord(ev[1], t->stream));
        SortPairs sp;
        if ((rc = sp.alloc(sc, (uint64_t)n_prot))) return rc;
        hipLaunchKernelGGL(kg::derive_rank_keys_kernel, dim3(grid_of(n_prot)), dim3(256), 0, t->stream, d_fn, d_otu, (uint64_t)n_prot,
                           sp.keys(), sp.vals());
        HIP_TRY(hipGetLastError());
        int32_t fmax = -1, omax = 0;
        for (int64_t k = 0; k < n_prot; k++) {
            fmax = std::max(fmax, fn[k]);
            if (fn[k] >= 0) omax = std::max(omax, otu[k]);
        }
        const uint64_t kmax = ((uint64_t)((uint32_t)fmax + 1u) << 31) | (uint64_t)(uint32_t)omax;
        if ((rc = sp.sort(t, sc, (uint64_t)n_prot, bit_width(kmax)))) return rc;
        hipLaunchKernelGGL(kg::derive_rank_scatter_kernel, dim3(grid_of(n_prot)), dim3(256), 0, t->stream, sp.vals(), d_fn, d_otu,
                           (uint64_t)n_prot, rank_of, fn_r, otu_r);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[2], t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        st.ms_sort += ev.ms(1, 2);
    }

    // ---- the pass plan: a histogram of the valid windows over the whole k-mer space, bins cut finer where needed ----
    Cap cap;
    if ((rc = size_cap(prm->max_windows_per_pass, "", kDeriveBytesPerWindow, kDerivePassMax, &cap))) return rc;
    dv.cap = cap.items;
    std::vector<unsigned long long> bins;
    const uint64_t space = (uint64_t)KG_MAX_ENCODED;
    const uint32_t shift0 = Deriver::shift_for(space);
    if ((rc = dv.histogram(0, space, shift0, bins))) return rc;
    uint64_t valid = 0;
    for (auto c : bins) valid += c;
    st.valid_windows = (int64_t)valid;
    for (uint64_t i = 0; i < kg::kDeriveBins; i++) {
        const uint64_t a = i << shift0;
        if (a >= space) break;
        if (bins[i] && (rc = dv.split(a, std::min<uint64_t>(space, a + (1ull << shift0)), bins[i]))) return rc;
    }
    std::vector<DeriveRange> passes;
    for (const auto &e : dv.elems) {
        if (!passes.empty() && passes.back().count + e.count <= dv.cap) {
            passes.back().hi = e.hi;
            passes.back().count += e.count;
        } else {
            passes.push_back(e);
        }
    }
    st.passes = (int32_t)passes.size();

    // ---- one pass per k-mer range ----
    std::vector<std::pair<uint8_t *, uint64_t>> outs;       // each pass's signatures (sc blocks), in k-mer order
    unsigned long long *d_cur = nullptr;
    uint64_t *d_tot = nullptr;
    if ((rc = sc.get(&d_cur, 2)) || (rc = sc.get(&d_tot, 8))) return rc;
    uint64_t total_sigs = 0;
    for (const DeriveRange &ps : passes) {
        const uint64_t n = ps.count;
        Scratch pass(t);                                    // this pass's scratch, back in the cache at its end
        WindowPairs w;
        if ((rc = dv.window_pairs(pass, n, ps.lo, ps.hi, nullptr, rank_of, b, d_cur, d_tot + 0, ev[1], ev[2], ev[3], &w))) return rc;
        const uint64_t P = w.P;
        uint64_t *const pk = w.pk, *const partial = w.partial;
        uint32_t *const pv = w.pv;
        // run heads and numbers at the three levels (flags / pidx / partial are reused: P <= n)
        uint32_t *kh = w.flags, *fh = nullptr, *oh = nullptr, *kx = w.pidx, *fx = nullptr, *ox = nullptr;
        if ((rc = pass.get(&fh, P)) || (rc = pass.get(&oh, P)) || (rc = pass.get(&fx, P)) || (rc = pass.get(&ox, P))) return rc;
        hipLaunchKernelGGL(kg::derive_run_flags_kernel, dim3(grid_of(P)), dim3(256), 0, t->stream, pk, P, b, fn_r, otu_r, kh, fh, oh);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, kh, P, kx, partial, d_tot + 1)) || (rc = prefix_sum(t, fh, P, fx, partial, d_tot + 2)) ||
            (rc = prefix_sum(t, oh, P, ox, partial, d_tot + 3)))
            return rc;
        uint64_t tot[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(tot, d_tot + 1, 24, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        const uint64_t K = tot[0], F = tot[1], O = tot[2];
        uint32_t *kstart = nullptr, *fstart = nullptr, *f_kmer = nullptr, *ostart = nullptr, *o_frun = nullptr;
        int32_t *f_fn = nullptr, *o_otu = nullptr;
        unsigned long long *fsum = nullptr, *kbest = nullptr, *kotu = nullptr;
        if ((rc = pass.get(&kstart, K + 1)) || (rc = pass.get(&fstart, F + 1)) || (rc = pass.get(&f_kmer, F)) ||
            (rc = pass.get(&f_fn, F)) || (rc = pass.get(&ostart, O + 1)) || (rc = pass.get(&o_frun, O)) || (rc = pass.get(&o_otu, O)) ||
            (rc = pass.get(&fsum, F)) || (rc = pass.get(&kbest, K)) || (rc = pass.get(&kotu, K)))
            return rc;
        hipLaunchKernelGGL(kg::derive_run_starts_kernel, dim3(grid_of(P)), dim3(256), 0, t->stream, pk, P, b, fn_r, otu_r, kx, fx, ox,
                           d_tot + 1, d_tot + 2, d_tot + 3, kstart, fstart, f_kmer, f_fn, ostart, o_frun, o_otu);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(fsum, 0, F * 8, t->stream));
        HIP_TRY(hipMemsetAsync(kbest, 0, K * 8, t->stream));
        HIP_TRY(hipMemsetAsync(kotu, 0, K * 8, t->stream));
        hipLaunchKernelGGL(kg::derive_run_sums_kernel, dim3(grid_of((P + kg::kDeriveChunk - 1) / kg::kDeriveChunk)), dim3(256), 0, t->stream,
                           pv, P, fh, fx, fsum);
        hipLaunchKernelGGL(kg::derive_fn_best_kernel, dim3(grid_of(F)), dim3(256), 0, t->stream, fstart, f_kmer, f_fn, F, kbest);
        hipLaunchKernelGGL(kg::derive_otu_best_kernel, dim3(grid_of(O)), dim3(256), 0, t->stream, ostart, o_frun, o_otu, O, f_kmer, kbest, kotu);
        HIP_TRY(hipGetLastError());
        // the signatures of the pass, in k-mer order (kflags / kidx reuse fh / fx: K <= P)
        uint32_t *kflags = fh, *kidx = fx;
        hipLaunchKernelGGL(kg::derive_select_kernel<false>, dim3(grid_of(K)), dim3(256), 0, t->stream, K, kstart, kbest, kotu, fsum, f_fn,
                           pk, b, ps.lo, (int64_t)prm->min_proteins, (int64_t)prm->purity_pct, kflags, nullptr, nullptr);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, kflags, K, kidx, partial, d_tot + 4))) return rc;
        uint64_t S = 0;
        HIP_TRY(hipMemcpyAsync(&S, d_tot + 4, 8, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        if (S) {
            uint8_t *o = nullptr;
            if ((rc = sc.get(&o, S * 24))) return rc;
            hipLaunchKernelGGL(kg::derive_select_kernel<true>, dim3(grid_of(K)), dim3(256), 0, t->stream, K, kstart, kbest, kotu, fsum, f_fn,
                               pk, b, ps.lo, (int64_t)prm->min_proteins, (int64_t)prm->purity_pct, nullptr, kidx, o);
            HIP_TRY(hipGetLastError());
            outs.emplace_back(o, S);
        }
        HIP_TRY(hipEventRecord(ev[4], t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        st.ms_encode += ev.ms(1, 2);
        st.ms_sort += ev.ms(2, 3);
        st.ms_reduce += ev.ms(3, 4);
        st.pairs += (int64_t)P;
        st.kmers += (int64_t)K;
        total_sigs += S;
    }
    if (total_sigs >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more signatures");
    // ---- the set: the passes' signatures back to back ----
    if ((rc = dalloc_detached(t, &set->d_sigs, std::max<uint64_t>(total_sigs * 24, 24)))) return rc;
    uint64_t at = 0;
    for (auto &o : outs) {
        HIP_TRY(hipMemcpyAsync(set->d_sigs + at * 24, o.first, o.second * 24, hipMemcpyDeviceToDevice, t->stream));
        at += o.second;
    }
    HIP_TRY(hipEventRecord(ev[5], t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    st.ms_encode += dv.ms_hist;
    st.ms_total = ev.ms(0, 5);
    st.signatures = (int64_t)total_sigs;
    set->count = (int64_t)total_sigs;
    return KG_OK;
}

int derive_entry(int device, const kg_derive_params *prm, const uint8_t *h_seq, const uint8_t *d_seq, const int64_t *offsets,
                 int64_t n_prot, const int32_t *fn, const int32_t *otu, kg_sigset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!prm) return fail(KG_ERR_ARG, "null kg_derive_params");
    if (prm->min_proteins < 1) return fail(KG_ERR_ARG, "min_proteins must be >= 1");
    if (prm->purity_pct < 1 || prm->purity_pct > 100) return fail(KG_ERR_ARG, "purity_pct must be in 1..100");
    if (prm->max_windows_per_pass < 0) return fail(KG_ERR_ARG, "max_windows_per_pass must be >= 0");
    if (n_prot < 0) return fail(KG_ERR_ARG, "n_prot < 0");
    if (n_prot >= (1ll << 29)) return fail(KG_ERR_LIMIT, "2^29 or more proteins in one call");
    if (!offsets) return fail(KG_ERR_ARG, "null offsets");
    if (n_prot > 0 && (!fn || !otu)) return fail(KG_ERR_ARG, "null fn / otu array");
    if (offsets[0] < 0) return fail(KG_ERR_ARG, "offsets[0] < 0");
    // (not check_protein_offsets: the null fn / otu check stands in front of the offsets, and the first offending protein is reported
    // whether its offsets or its annotation are wrong, so the four checks share the loop)
    for (int64_t k = 0; k < n_prot; k++) {
        const int64_t L = offsets[k + 1] - offsets[k];
        if (L < 0) return fail(KG_ERR_ARG, "protein " + kmer_text(k) + ": offsets decrease (offsets[p+1] < offsets[p])");
        if (L >= (1ll << 31)) return fail(KG_ERR_LIMIT, "protein " + kmer_text(k) + ": 2^31 or more characters");
        if (fn[k] < -1) return fail(KG_ERR_ARG, "protein " + kmer_text(k) + ": fn = " + kmer_text(fn[k]) + " < -1");
        if (fn[k] >= 0 && otu[k] < 0) return fail(KG_ERR_ARG, "protein " + kmer_text(k) + ": otu = " + kmer_text(otu[k]) + " < 0 on an annotated protein");
    }
    const uint64_t seq_bytes = n_prot ? (uint64_t)offsets[n_prot] : 0;
    if (seq_bytes && !h_seq && !d_seq) return fail(KG_ERR_ARG, "null sequence");
    CallScope cs(device);               // the call's context: closed when the call returns, the set keeps only its signatures
    if (cs.rc) return cs.rc;
    kg_sigset *set = new (std::nothrow) kg_sigset();
    if (!set) return fail(KG_ERR_NOMEM, "out of host memory");
    set->device = device;
    int rc = d_seq && hipDeviceSynchronize() != hipSuccess ? fail(KG_ERR_DEVICE, "hipDeviceSynchronize failed") : KG_OK;
    if (!rc) rc = derive_impl(cs.t, prm, h_seq, d_seq, offsets, n_prot, fn, otu, set);
    cs.t->cache.release_all();                          // scratch goes back to the driver
    if (rc) { kg_sigset_free(set); return rc; }
    if (getenv("KG_DEBUG"))
        fprintf(stderr, "[kg] kg_signatures_derive: proteins=%lld valid=%lld pairs=%lld kmers=%lld sigs=%lld passes=%d encode_ms=%.3f sort_ms=%.3f reduce_ms=%.3f total_ms=%.3f\n",
                (long long)set->st.proteins, (long long)set->st.valid_windows, (long long)set->st.pairs, (long long)set->st.kmers,
                (long long)set->st.signatures, set->st.passes, set->st.ms_encode, set->st.ms_sort, set->st.ms_reduce, set->st.ms_total);
    *out = set;
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_signatures_derive(int device, const kg_derive_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                         const int32_t *fn, const int32_t *otu, kg_sigset **out)
{
    return derive_entry(device, p, seq, nullptr, offsets, n_prot, fn, otu, out);
}

int kg_signatures_derive_device(int device, const kg_derive_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                                const int32_t *fn, const int32_t *otu, kg_sigset **out)
{
    return derive_entry(device, p, nullptr, d_seq, offsets, n_prot, fn, otu, out);
}

int64_t kg_sigset_count(const kg_sigset *s) { return s ? s->count : 0; }

const kg_signature *kg_sigset_device(const kg_sigset *s) { return s ? (const kg_signature *)s->d_sigs : nullptr; }

int kg_sigset_copy(const kg_sigset *s, int64_t first, int64_t count, kg_signature *dst)
{
    return copy_records(s, s ? s->device : 0, s ? (const kg_signature *)s->d_sigs : nullptr, 1, s ? s->count : 0, first, count, dst, "kg_sigset_copy");
}

int kg_sigset_stats(const kg_sigset *s, kg_derive_stats *out) { return copy_stats(s, s ? &s->st : nullptr, out); }

void kg_sigset_free(kg_sigset *s)
{
    if (!s) return;
    if (s->d_sigs) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->d_sigs);
    }
    delete s;
}

}  // extern "C"
