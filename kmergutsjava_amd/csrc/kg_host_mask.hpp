// kg_host_mask.hpp -- kg_proteins_mask / kg_proteins_mask_device: proteins -> their low-complexity segments (kernels: kg_mask.hpp),
// and what the search and cluster hosts need of it: mask_plan (a checked kg_mask_params), mask_run (flags, segments and
// statistics of a range of proteins) and mask_seeding_copy (the sequence with the masked residues turned into non-residues, which
// the window-pairs pass of kg_host_derive.hpp reads in the original's place).
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_derive.hpp and in front of kg_host_cluster.hpp and
// kg_host_search.hpp.
#pragma once

struct kg_maskset {
    int device = 0;
    Detached d_flags;                   // one byte per residue, residue 0 = offsets[0]
    Detached d_block;                   // seg_start[n_prot + 1] (int64), then count * 16 bytes
    int64_t count = 0, n_prot = 0, residues = 0;
    kg_mask_stats st = {};
    const int64_t *starts() const { return (const int64_t *)d_block.p; }
    const kg_mask_segment *segs() const { return (const kg_mask_segment *)(d_block.p + ((size_t)n_prot + 1) * 8); }
};

static_assert(sizeof(kg_mask_params) == 16 && sizeof(kg_mask_segment) == 16 && sizeof(kg_mask_stats) == 80, "record layouts of include/kmerguts_hip.h");

namespace {

int32_t coding_lg(uint64_t x);          // kg_host_coding.hpp: the header's Lg

struct MaskPlan { kg::MaskSpec spec; kg_mask_params prm; };

// the first offender of a kg_mask_params, in the header's order, or the plan
int mask_plan(const kg_mask_params *mp, MaskPlan *out)
{
    if (!mp) return fail(KG_ERR_ARG, "null kg_mask_params");
    if (mp->window < 4 || mp->window > kg::kMaskMaxWindow) return fail(KG_ERR_ARG, "window must be in 4..32");
    if (mp->trigger < 0) return fail(KG_ERR_ARG, "trigger must be >= 0");
    if (mp->extend < mp->trigger) return fail(KG_ERR_ARG, "extend must be >= trigger");
    const int32_t lgw = coding_lg((uint64_t)mp->window);
    if (mp->extend >= lgw) return fail(KG_ERR_ARG, "extend must be below Lg(window) = " + kmer_text(lgw));
    if (mp->reserved != 0) return fail(KG_ERR_ARG, "kg_mask_params.reserved must be 0");
    MaskPlan pl = {};
    pl.prm = *mp;
    pl.spec.window = (uint32_t)mp->window;
    pl.spec.low_max = (uint32_t)(mp->window * mp->trigger);
    pl.spec.ext_max = (uint32_t)(mp->window * mp->extend);
    pl.spec.full = (uint32_t)(mp->window * lgw);
    for (int n = 1; n <= kg::kMaskMaxWindow; n++) pl.spec.nlg[n] = (uint16_t)(n * coding_lg((uint64_t)n));
    *out = pl;
    return KG_OK;
}

// blocks of 64 over the max(len_p - W + 1, 0) window positions of protein p
int mask_block_bases(const int64_t *offsets, int64_t n_prot, uint32_t window, std::vector<uint32_t> &ibase, uint64_t *nblocks_out)
{
    ibase.assign((size_t)n_prot + 1, 0);
    uint64_t nblocks = 0;
    for (int64_t k = 0; k < n_prot; k++) {
        const int64_t L = offsets[k + 1] - offsets[k];
        ibase[(size_t)k] = (uint32_t)nblocks;
        const uint64_t nwin = L >= (int64_t)window ? (uint64_t)L - window + 1 : 0;
        nblocks += (nwin + kg::kAaWinPerBlock - 1) / kg::kAaWinPerBlock;
        if (nblocks > 0x7FFFFFFFull) return fail(KG_ERR_LIMIT, "2^31 or more window blocks of 64 windows in one call");
    }
    ibase[(size_t)n_prot] = (uint32_t)nblocks;
    *nblocks_out = nblocks;
    return KG_OK;
}

// What mask_run gives, in the caller's scratch: flags[k] for every byte k of the sequence below offsets[n_prot] (0 outside the
// proteins), seg_start[n_prot + 1], the n_seg segments (protein counted from the first protein of the range; null without
// want_segments or without a segment) and the statistics, ms_mask included.
struct MaskOut {
    uint8_t *flags = nullptr;
    int64_t *seg_start = nullptr;
    kg::MaskSeg *segs = nullptr;
    uint64_t n_seg = 0;
    kg_mask_stats st = {};
};

// The mask of the n_prot >= 0 proteins at offsets[0 .. n_prot] (host; a range of a batch's offsets) of the device sequence d_seq.
// flags is given by the caller: flags_bytes >= offsets[n_prot] bytes, zeroed here.  Three host synchronisations.
int mask_run(kg_table *t, Scratch &sc, const MaskPlan &pl, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot, uint8_t *flags,
             uint64_t flags_bytes, bool want_segments, MaskOut *out)
{
    hipStream_t s = t->stream;
    const uint32_t W = pl.spec.window;
    int rc;
    Events<2> ev;
    if ((rc = ev.create())) return rc;
    out->flags = flags;
    kg_mask_stats &st = out->st;
    st.proteins = n_prot;
    st.residues = n_prot ? offsets[n_prot] - offsets[0] : 0;
    HIP_TRY(hipEventRecord(ev[0], s));
    if (flags_bytes) HIP_TRY(hipMemsetAsync(flags, 0, flags_bytes, s));
    if ((rc = sc.get(&out->seg_start, (size_t)n_prot + 1))) return rc;
    HIP_TRY(hipMemsetAsync(out->seg_start, 0, ((size_t)n_prot + 1) * 8, s));
    std::vector<uint32_t> ibase;
    uint64_t nblocks = 0;
    if ((rc = mask_block_bases(offsets, n_prot, W, ibase, &nblocks))) return rc;
    if (nblocks) {
        const uint32_t nb = (uint32_t)nblocks, np = (uint32_t)n_prot;
        int64_t *d_off = nullptr;
        uint32_t *d_ibase = nullptr, *blk_starts = nullptr, *blk_base = nullptr;
        kg::BlockDesc *d_blocks = nullptr;
        uint64_t *low = nullptr, *ext = nullptr, *mw = nullptr, *partial = nullptr, *d_total = nullptr;
        unsigned long long *counts = nullptr;
        if ((rc = sc.get(&d_off, (size_t)n_prot + 1)) || (rc = sc.get(&d_ibase, (size_t)n_prot + 1)) || (rc = sc.get(&d_blocks, nblocks)) ||
            (rc = sc.get(&low, nblocks)) || (rc = sc.get(&ext, nblocks)) || (rc = sc.get(&mw, nblocks)) || (rc = sc.get(&blk_starts, nblocks)) ||
            (rc = sc.get(&blk_base, nblocks)) || (rc = sc.get(&partial, nblocks / kg::kScanChunk + 3)) || (rc = sc.get(&d_total, 1)) ||
            (rc = sc.get(&counts, kg::kMaskWords)))
            return rc;
        HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)n_prot + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_ibase, ibase.data(), ((size_t)n_prot + 1) * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(counts, 0, kg::kMaskWords * 8, s));
        hipLaunchKernelGGL(kg::build_blocks_kernel, dim3(grid_of(nblocks)), dim3(256), 0, s, d_off, d_ibase, np, nb, d_blocks);
        hipLaunchKernelGGL(kg::mask_windows_kernel, dim3(emit_grid(nb)), dim3(kg::kDeriveThreads), 0, s, d_seq, d_blocks, nb, pl.spec, low, ext);
        hipLaunchKernelGGL(kg::mask_runs_kernel, dim3(grid_of(np)), dim3(256), 0, s, d_ibase, d_off, np, W, low, ext, mw, counts);
        hipLaunchKernelGGL(kg::mask_residues_kernel<false>, dim3(emit_grid(nb)), dim3(kg::kDeriveThreads), 0, s, d_blocks, nb, W, mw, flags,
                           blk_starts, nullptr, nullptr, (uint64_t)0, counts);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, blk_starts, nblocks, blk_base, partial, d_total))) return rc;
        hipLaunchKernelGGL(kg::mask_starts_kernel, dim3(grid_of((uint64_t)n_prot + 1)), dim3(256), 0, s, d_ibase, np, nb, blk_base, d_total,
                           out->seg_start, counts);
        HIP_TRY(hipGetLastError());
        unsigned long long hc[kg::kMaskWords] = {};
        HIP_TRY(hipMemcpyAsync(hc, counts, sizeof hc, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&out->n_seg, d_total, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (out->n_seg >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more masked segments in one call");
        if (want_segments && out->n_seg) {
            if ((rc = sc.get(&out->segs, out->n_seg))) return rc;
            hipLaunchKernelGGL(kg::mask_residues_kernel<true>, dim3(emit_grid(nb)), dim3(kg::kDeriveThreads), 0, s, d_blocks, nb, W, mw, flags,
                               nullptr, blk_base, out->segs, out->n_seg, nullptr);
            HIP_TRY(hipGetLastError());
        }
        st.windows = (int64_t)hc[kg::kMaskWindows];
        st.low_windows = (int64_t)hc[kg::kMaskLow];
        st.ext_windows = (int64_t)hc[kg::kMaskExt];
        st.masking_windows = (int64_t)hc[kg::kMaskMasking];
        st.masked_residues = (int64_t)hc[kg::kMaskResidues];
        st.proteins_masked = (int64_t)hc[kg::kMaskProteins];
        st.segments = (int64_t)out->n_seg;
    }
    HIP_TRY(hipEventRecord(ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    st.ms_mask = ev.ms(0, 1);
    return KG_OK;
}

// The sequence the window-pairs pass reads under a mask: a copy of d_seq[0 .. seq_bytes) in the call's scratch in which the masked
// residues of proteins [p0, p1) of the batch have 0x20 set.  st: the mask's statistics, ms_mask with the copy's time.
int mask_seeding_copy(kg_table *t, Scratch &sc, const MaskPlan &pl, const uint8_t *d_seq, const int64_t *offsets, int64_t p0, int64_t p1,
                      uint64_t seq_bytes, const uint8_t **d_out, kg_mask_stats *st)
{
    *d_out = d_seq;
    if (!seq_bytes) { *st = {}; st->proteins = p1 - p0; return KG_OK; }
    int rc;
    uint8_t *flags = nullptr, *copy = nullptr;
    Events<2> ev;
    MaskOut mo;
    if ((rc = ev.create()) || (rc = sc.get(&flags, seq_bytes)) || (rc = sc.get(&copy, seq_bytes)) ||
        (rc = mask_run(t, sc, pl, d_seq, offsets + p0, p1 - p0, flags, seq_bytes, false, &mo)))
        return rc;
    HIP_TRY(hipEventRecord(ev[0], t->stream));
    hipLaunchKernelGGL(kg::mask_apply_kernel, dim3(std::min<uint32_t>(grid_of(seq_bytes), 256u * 32)), dim3(256), 0, t->stream, d_seq, flags,
                       seq_bytes, (uint64_t)offsets[p0], (uint64_t)offsets[p1], copy);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    *st = mo.st;
    st->ms_mask += ev.ms(0, 1);
    *d_out = copy;
    return KG_OK;
}

int mask_impl(kg_table *t, const MaskPlan &pl, const uint8_t *h_seq, const uint8_t *d_seq_in, const int64_t *offsets, int64_t n_prot,
              kg_maskset *set)
{
    Scratch sc(t);
    int rc;
    const uint64_t seq_bytes = n_prot ? (uint64_t)offsets[n_prot] : 0, first = n_prot ? (uint64_t)offsets[0] : 0;
    const uint8_t *d_seq = nullptr;
    uint8_t *flags = nullptr;
    if ((rc = stage_sequence(t, sc, h_seq, d_seq_in, seq_bytes, &d_seq)) || (rc = sc.get(&flags, std::max<uint64_t>(seq_bytes, 1)))) return rc;
    MaskOut mo;
    if ((rc = mask_run(t, sc, pl, d_seq, offsets, n_prot, flags, seq_bytes, true, &mo))) return rc;
    set->n_prot = n_prot;
    set->residues = (int64_t)(seq_bytes - first);
    set->count = (int64_t)mo.n_seg;
    set->st = mo.st;
    const size_t start_bytes = ((size_t)n_prot + 1) * 8;
    if ((rc = dalloc_detached(t, &set->d_flags.p, std::max<uint64_t>(seq_bytes - first, 1))) ||
        (rc = dalloc_detached(t, &set->d_block.p, start_bytes + std::max<uint64_t>(mo.n_seg, 1) * sizeof(kg_mask_segment))))
        return rc;
    if (seq_bytes > first) HIP_TRY(hipMemcpyAsync(set->d_flags.p, flags + first, seq_bytes - first, hipMemcpyDeviceToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(set->d_block.p, mo.seg_start, start_bytes, hipMemcpyDeviceToDevice, t->stream));
    if (mo.n_seg)
        HIP_TRY(hipMemcpyAsync(set->d_block.p + start_bytes, mo.segs, mo.n_seg * sizeof(kg_mask_segment), hipMemcpyDeviceToDevice, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return KG_OK;
}

int mask_entry(int device, const kg_mask_params *prm, const uint8_t *h_seq, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
               kg_maskset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    MaskPlan pl;
    if (int rc = mask_plan(prm, &pl)) return rc;
    if (n_prot < 0) return fail(KG_ERR_ARG, "n_prot < 0");
    if (n_prot >= (1ll << 29)) return fail(KG_ERR_LIMIT, "2^29 or more proteins in one call");
    if (int rc = check_protein_offsets(offsets, n_prot, (int64_t)kg::kAlignMaxLen, "2^24")) return rc;
    const uint64_t seq_bytes = n_prot ? (uint64_t)offsets[n_prot] : 0;
    if (seq_bytes && !h_seq && !d_seq) return fail(KG_ERR_ARG, "null sequence");
    CallScope cs(device);               // the call's context: closed when the call returns, the set keeps only its records
    if (cs.rc) return cs.rc;
    kg_maskset *set = new (std::nothrow) kg_maskset();
    if (!set) return fail(KG_ERR_NOMEM, "out of host memory");
    set->device = device;
    int rc = d_seq && hipDeviceSynchronize() != hipSuccess ? fail(KG_ERR_DEVICE, "hipDeviceSynchronize failed") : KG_OK;
    if (!rc) rc = mask_impl(cs.t, pl, h_seq, d_seq, offsets, n_prot, set);
    cs.t->cache.release_all();                          // scratch goes back to the driver
    if (rc) { std::string keep = g_err; kg_maskset_free(set); g_err = keep; return rc; }
    if (getenv("KG_DEBUG"))
        fprintf(stderr, "[kg] kg_proteins_mask: proteins=%lld residues=%lld windows=%lld low=%lld ext=%lld masking=%lld segments=%lld masked=%lld proteins_masked=%lld mask_ms=%.3f\n",
                (long long)set->st.proteins, (long long)set->st.residues, (long long)set->st.windows, (long long)set->st.low_windows,
                (long long)set->st.ext_windows, (long long)set->st.masking_windows, (long long)set->st.segments,
                (long long)set->st.masked_residues, (long long)set->st.proteins_masked, set->st.ms_mask);
    *out = set;
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_proteins_mask(int device, const kg_mask_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot, kg_maskset **out)
{
    return mask_entry(device, p, seq, nullptr, offsets, n_prot, out);
}

int kg_proteins_mask_device(int device, const kg_mask_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot, kg_maskset **out)
{
    return mask_entry(device, p, nullptr, d_seq, offsets, n_prot, out);
}

int64_t kg_maskset_count(const kg_maskset *s) { return s ? s->count : 0; }

int kg_maskset_copy(const kg_maskset *s, int64_t first, int64_t count, kg_mask_segment *dst)
{
    return copy_records(s, s ? s->device : 0, s ? s->segs() : nullptr, 1, s ? s->count : 0, first, count, dst, "kg_maskset_copy");
}

int kg_maskset_starts_copy(const kg_maskset *s, int64_t *dst)
{
    return copy_starts(s, s ? s->device : 0, s ? s->starts() : nullptr, s ? s->n_prot : 0, dst);
}

int kg_maskset_flags_copy(const kg_maskset *s, int64_t first, int64_t count, uint8_t *dst)
{
    return copy_records(s, s ? s->device : 0, s ? (const uint8_t *)s->d_flags.p : nullptr, 1, s ? s->residues : 0, first, count, dst,
                        "kg_maskset_flags_copy");
}

int kg_maskset_stats(const kg_maskset *s, kg_mask_stats *out) { return copy_stats(s, s ? &s->st : nullptr, out); }

void kg_maskset_free(kg_maskset *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;                           // (its blocks with it)
}

}  // extern "C"
