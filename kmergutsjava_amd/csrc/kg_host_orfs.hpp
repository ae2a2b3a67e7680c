// kg_host_orfs.hpp -- kg_regionset_orfs / kg_orfs_regions: function regions -> open reading frames and their proteins;
// kg_orfs_free / kg_orfset_add_free: the evidence-free open reading frames of the six frames (kernels: kg_orfs.hpp).
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_regions.hpp (it reads kg_regionset).  The stages that
// make a kg_orfset follow it (kg_host_repair.hpp, kg_host_coding.hpp, kg_host_starts.hpp) and share its helpers: the batch's
// checks and bytes, the protein layout, the translation, what a new set keeps and inherits, and the getters' guard.
#pragma once

struct kg_orfset : SetBase {
    kg_orf *d_orfs = nullptr;           // count records, index-aligned with the regions
    int64_t *d_prot_start = nullptr;    // count + 1
    uint8_t *d_res = nullptr;           // residues bytes
    int64_t count = 0, residues = 0;
    int64_t n_seqs = 0, l_max = 0;      // the batch's contigs and the longest of them (kg_orfset_select)
    kg_orf_stats st = {};
    // kg_orfset_coding (kg_host_coding.hpp): the score of every record, what the call counted and its statistics
    int64_t *d_coding = nullptr;        // count, null for a set that has no scores
    std::unique_ptr<kg_coding_model> coding_model;
    kg_coding_stats coding_st = {};
    // kg_orfset_starts (kg_host_starts.hpp): the shift of every record in codons, the last round's counts and the statistics
    int32_t *d_shift = nullptr;         // count, null for a set that is not from kg_orfset_starts
    std::unique_ptr<kg_start_model> start_model;
    kg_start_stats start_st = {};
    // kg_regionset_repair (kg_host_repair.hpp): the junction list, junction_start[count + 1] and the statistics
    kg_junction *d_junctions = nullptr; // junctions records, null for a set that is not from kg_regionset_repair
    int64_t *d_junction_start = nullptr;
    int64_t junctions = 0;
    bool repaired = false;
    kg_repair_stats repair_st = {};
};

static_assert(kg::kOrfErrWords + kg::kOrfCntWords + 1 <= kPinStageWords && kg::kOrfFreeWords <= kPinStageWords,
              "stage words must fit their pinned words");

namespace {

int check_orf_params(const kg_orf_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_orf_params");
    if (p->start_codons < 0 || p->start_codons > 7) return fail(KG_ERR_ARG, "start_codons must be a mask of 1 (ATG), 2 (GTG), 4 (TTG)");
    if (p->only_kept < 0 || p->only_kept > 1) return fail(KG_ERR_ARG, "only_kept must be 0 or 1");
    return KG_OK;
}

int check_free_params(const kg_free_params *p)
{
    if (!p) return fail(KG_ERR_ARG, "null kg_free_params");
    if (p->min_res < 1) return fail(KG_ERR_ARG, "min_res must be >= 1");
    if (p->start_codons < 0 || p->start_codons > 7) return fail(KG_ERR_ARG, "start_codons must be a mask of 1 (ATG), 2 (GTG), 4 (TTG)");
    if (p->reserved != 0) return fail(KG_ERR_ARG, "kg_free_params.reserved must be 0");
    return KG_OK;
}

// The tile rows of a batch and the six scanned arrays over them (kg_orfs.hpp, steps 1 and 2): what the region kernel and the
// free enumerator both walk.  Declare it in front of the call's scratch, whose destructor waits for the stream that copies
// tile_base.
struct OrfPlanes {
    // the tile rows in front of every contig: a row is kOrfTile codons of each of its three phases
    std::vector<int64_t> tile_base;
    uint64_t n_seqs = 0, n_rows = 0, n_tiles = 0, total = 0;
    uint32_t n_scan = 0;
    int64_t l_max = 0;
    int64_t *d_off = nullptr, *d_tb = nullptr, *keys = nullptr, *tile_max = nullptr, *tile_pre = nullptr;

    int plan(const int64_t *offsets, uint64_t n)
    {
        n_seqs = n;
        tile_base.assign(n_seqs + 1, 0);
        for (uint64_t k = 0; k < n_seqs; k++) {
            tile_base[k + 1] = tile_base[k] + ((offsets[k + 1] - offsets[k]) / 3 + kg::kOrfTile - 1) / kg::kOrfTile;
            l_max = std::max(l_max, offsets[k + 1] - offsets[k]);
        }
        n_rows = (uint64_t)tile_base[n_seqs];
        n_tiles = 3 * n_rows;
        total = n_seqs ? (uint64_t)offsets[n_seqs] : 0;
        if (n_rows >= (1ull << 31)) return fail(KG_ERR_LIMIT, "2^31 or more tile rows in one call");
        n_scan = (uint32_t)((n_tiles + kg::kBuildTile - 1) / kg::kBuildTile);
        return KG_OK;
    }
    int alloc_geometry(Scratch &sc)
    {
        int rc;
        if ((rc = sc.get(&d_off, n_seqs + 1)) || (rc = sc.get(&d_tb, n_seqs + 1))) return rc;
        return KG_OK;
    }
    int alloc_keys(Scratch &sc)
    {
        int rc;
        if ((rc = sc.get(&keys, std::max<uint64_t>(kg::kOrfPlanes * n_tiles, 1))) ||
            (rc = sc.get(&tile_max, std::max<uint64_t>((uint64_t)kg::kOrfPlanes * n_scan, 1))) ||
            (rc = sc.get(&tile_pre, std::max<uint64_t>((uint64_t)kg::kOrfPlanes * n_scan, 1))))
            return rc;
        return KG_OK;
    }
    int upload(hipStream_t s, const int64_t *offsets)
    {
        HIP_TRY(hipMemcpyAsync(d_off, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_tb, tile_base.data(), (n_seqs + 1) * 8, hipMemcpyHostToDevice, s));
        return KG_OK;
    }
    kg::OrfGeometry geometry() const { return kg::OrfGeometry{d_off, d_tb, n_seqs, n_tiles}; }
    // the summaries and their six prefix maxima
    int launch(hipStream_t s, const uint8_t *d_seq, uint32_t sc_mask)
    {
        if (n_rows == 0) return KG_OK;
        hipLaunchKernelGGL(kg::orf_summary_kernel, dim3((uint32_t)((n_rows + 3) / 4)), dim3(256), 0, s, d_seq, total, geometry(), n_rows, sc_mask, keys);
        hipLaunchKernelGGL(kg::orf_tile_max_kernel, dim3(n_scan, kg::kOrfPlanes), dim3(kg::kBuildThreads), 0, s, keys, n_tiles, tile_max);
        for (int a = 0; a < kg::kOrfPlanes; a++)
            hipLaunchKernelGGL(kg::build_tile_scan_kernel, dim3(1), dim3(kg::kBuildThreads), 0, s, tile_max + (uint64_t)a * n_scan, n_scan,
                               tile_pre + (uint64_t)a * n_scan);
        hipLaunchKernelGGL(kg::orf_scan_apply_kernel, dim3(n_scan, kg::kOrfPlanes), dim3(kg::kBuildThreads), 0, s, keys, n_tiles, tile_pre);
        HIP_TRY(hipGetLastError());
        return KG_OK;
    }
};

// the batch's bytes from (possibly pageable) host memory: large ones through pinned pieces on several threads, as a table's
// signatures go up (complete on return); small ones as one copy on the call's stream
int upload_batch(kg_table *t, const uint8_t *src, uint64_t bytes, uint8_t *d_dst)
{
    if (bytes >= (64ull << 20)) return upload_pinned(t, src, (size_t)bytes, d_dst);
    HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, t->stream));
    return KG_OK;
}

// the host checks the entry points share; *total = the batch's bytes.  whose ("region set's", "ORF set's"): the call works on a
// set of parent_n_seqs contigs, and the batch must be that set's
int check_orf_batch(const uint8_t *seq, const int64_t *offsets, int64_t n_seqs, uint64_t *total, const char *whose = nullptr,
                    int64_t parent_n_seqs = 0)
{
    int64_t l_max = 0;
    int rc = check_region_offsets(offsets, n_seqs, &l_max);
    if (rc) return rc;
    if (n_seqs && offsets[0] < 0) return fail(KG_ERR_ARG, "offsets[0] < 0");
    *total = n_seqs ? (uint64_t)offsets[n_seqs] : 0;
    if (*total && !seq) return fail(KG_ERR_ARG, "null sequence bytes");
    if (whose && n_seqs != parent_n_seqs) return fail(KG_ERR_ARG, std::string("n_seqs is not the ") + whose);
    return KG_OK;
}

// the batch's bytes where the kernels read them: the caller's device memory, or a copy in the call's scratch
int batch_on_device(kg_table *t, Scratch &sc, const uint8_t *seq, int seq_on_device, uint64_t total, const uint8_t **d_seq)
{
    *d_seq = seq;
    if (seq_on_device) {
        HIP_TRY(hipDeviceSynchronize());            // the bytes may have been produced on another stream
        return KG_OK;
    }
    uint8_t *up = nullptr;
    int rc = sc.get(&up, total ? total : 1);
    if (rc) return rc;
    if (total && (rc = upload_batch(t, seq, total, up))) return rc;
    *d_seq = up;
    return KG_OK;
}

// lens[n] -> d_start[n + 1], where every protein begins, and their total -> *d_total (excl[n], partial: the prefix sum's)
int layout_proteins(kg_table *t, const uint32_t *lens, uint64_t n, uint32_t *excl, uint64_t *partial, uint64_t *d_total, int64_t *d_start)
{
    int rc;
    if (n > 0 && (rc = prefix_sum(t, lens, n, excl, partial, d_total))) return rc;
    hipLaunchKernelGGL(kg::orf_prot_start_kernel, dim3(grid_of(n + 1)), dim3(256), 0, t->stream, excl, d_total, n, d_start);
    HIP_TRY(hipGetLastError());
    return KG_OK;
}

// the n_res residues of d_orfs[n], laid out by d_start, translated into *d_res (of the scratch; one byte when there are none)
int translate_orfs(kg_table *t, Scratch &sc, const kg_orf *d_orfs, uint64_t n, const int64_t *d_start, uint64_t n_res, const uint8_t *d_seq,
                   const int64_t *d_off, uint8_t **d_res)
{
    int rc;
    if ((rc = sc.get(d_res, std::max<uint64_t>(n_res, 1)))) return rc;
    if (n_res > 0) {
        hipLaunchKernelGGL(kg::orf_residues_kernel, dim3(grid_of((n_res + kg::kOrfResPerLane - 1) / kg::kOrfResPerLane)), dim3(256), 0,
                           t->stream, d_orfs, n, d_start, n_res, d_seq, d_off, *d_res);
        HIP_TRY(hipGetLastError());
    }
    return KG_OK;
}

// ... and over them the given set's bytes where a record is a repaired one (kg_repair.hpp: it does not read in one frame).  The
// given set's record i is d_orfs[i] and has kept its length; records behind the given set's are never repaired ones.
int keep_repaired(kg_table *t, const kg_orf *d_orfs, uint64_t n, const int64_t *d_start, uint64_t n_res, const kg_orfset *given, uint8_t *d_res)
{
    if (n_res == 0 || !given || given->count == 0) return KG_OK;
    hipLaunchKernelGGL(kg::orf_keep_repaired_kernel, dim3(grid_of((n_res + kg::kOrfResPerLane - 1) / kg::kOrfResPerLane)), dim3(256), 0,
                       t->stream, d_orfs, n, d_start, n_res, given->d_prot_start, given->d_res, d_res);
    HIP_TRY(hipGetLastError());
    return KG_OK;
}

// the three arrays of every ORF set leave the call's scratch, as a stage's own do beside them: the rest goes back to the cache
void keep_orfs(kg_orfset *set, Scratch &sc, kg_orf *d_orfs, int64_t *d_start, uint8_t *d_res, uint64_t n, uint64_t n_res, uint64_t n_seqs)
{
    set->d_orfs = set->keep(sc, d_orfs);
    set->d_prot_start = set->keep(sc, d_start);
    set->d_res = set->keep(sc, d_res);
    set->count = (int64_t)n;
    set->residues = (int64_t)n_res;
    set->n_seqs = (int64_t)n_seqs;
}

// what a stage that rewrites the records of `os` hands on: the longest contig, the ORF and coding statistics, the coding model
int inherit(kg_orfset *set, const kg_orfset *os)
{
    set->l_max = os->l_max;
    set->st = os->st;
    set->coding_st = os->coding_st;
    if (os->coding_model) {
        set->coding_model.reset(new (std::nothrow) kg_coding_model(*os->coding_model));
        if (!set->coding_model) return fail(KG_ERR_NOMEM, "out of host memory");
    }
    return KG_OK;
}

// The checks of a getter of something only some ORF sets have: the arguments (args: the others are there), then `has`, or
// "<name>: <why not>"
int need_of_set(const kg_orfset *s, bool args, bool has, const char *name, const char *why_not)
{
    if (!s || !args) return fail(KG_ERR_ARG, "null argument");
    if (!has) return fail(KG_ERR_ARG, std::string(name) + ": " + why_not);
    return KG_OK;
}

// d_regions[n]: device array complete on t->stream; d_seq: the batch's bytes on the device (null when there are none);
// offsets: host, checked.  Fills set (its arrays come out of the cache with the call's scratch and are kept only on success).
int orfs_impl(kg_table *t, const kg_orf_params *prm, const kg_region *d_regions, uint64_t n, const uint8_t *d_seq,
              const int64_t *offsets, uint64_t n_seqs, kg_orfset *set)
{
    OrfPlanes pl;
    Scratch sc(t);
    hipStream_t s = t->stream;
    int rc;
    if ((rc = pl.plan(offsets, n_seqs))) return rc;
    set->l_max = std::max(set->l_max, pl.l_max);
    const uint64_t n_tiles = pl.n_tiles;
    int64_t *d_start = nullptr;
    unsigned long long *words = nullptr;           // error words, counter words, then the residue total
    kg_orf *d_out = nullptr;
    uint32_t *lens = nullptr, *excl = nullptr;
    uint64_t *partial = nullptr;
    if ((rc = pl.alloc_geometry(sc)) || (rc = sc.get(&words, 16)) || (rc = pl.alloc_keys(sc)) ||
        (rc = sc.get(&d_out, std::max<uint64_t>(n, 1))) || (rc = sc.get(&d_start, n + 1)) || (rc = sc.get(&lens, std::max<uint64_t>(n, 1))) ||
        (rc = sc.get(&excl, std::max<uint64_t>(n, 1))) || (rc = sc.get(&partial, n / kg::kScanChunk + 2)))
        return rc;
    unsigned long long *err = words, *cnt = words + kg::kOrfErrWords;
    uint64_t *d_total = (uint64_t *)(words + kg::kOrfErrWords + kg::kOrfCntWords);
    if ((rc = pl.upload(s, offsets))) return rc;
    HIP_TRY(hipMemsetAsync(err, 0x7F, kg::kOrfErrWords * 8, s));
    HIP_TRY(hipMemsetAsync(cnt, 0, (kg::kOrfCntWords + 1) * 8, s));
    HIP_TRY(hipEventRecord(t->ev[kEvStageBegin], s));
    const kg::OrfGeometry geo = pl.geometry();
    const int64_t *keys = pl.keys, *d_off = pl.d_off;
    const uint32_t sc_mask = (uint32_t)prm->start_codons;
    if ((rc = pl.launch(s, d_seq, sc_mask))) return rc;
    if (n > 0) {
        hipLaunchKernelGGL(kg::orf_region_kernel, dim3(grid_of(n)), dim3(256), 0, s, d_regions, n, d_seq, geo, keys, sc_mask,
                           (int)prm->only_kept, d_out, lens, err, cnt);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = layout_proteins(t, lens, n, excl, partial, d_total, d_start))) return rc;
    // the one wait of the call: the residue total (and, with it, the error and counter words)
    constexpr int kWords = kg::kOrfErrWords + kg::kOrfCntWords + 1;
    if ((rc = read_error_words(t, words, kWords, kPinStage,                          // (in the order they are reported)
                               {{kg::kOrfErrSeq, KG_ERR_ARG, "region ", ": seq outside [0, n_seqs)"},
                                {kg::kOrfErrStrand, KG_ERR_ARG, "region ", ": strand is neither 0 nor 1"},
                                {kg::kOrfErrFrame, KG_ERR_ARG, "region ", ": best_frame outside 0..2"},
                                {kg::kOrfErrRange, KG_ERR_ARG, "region ", ": outside its contig (0 <= left <= right <= L - 1 does not hold)"},
                                {kg::kOrfErrAnchor, KG_ERR_ARG, "region ", ": holds no whole codon of its best_frame"}})))
        return rc;
    const uint64_t *h = t->h_pin + kPinStage;
    const uint64_t n_res = h[kg::kOrfErrWords + kg::kOrfCntWords];
    if (n_res >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more residues in one call");
    uint8_t *d_res = nullptr;
    if ((rc = translate_orfs(t, sc, d_out, n, d_start, n_res, d_seq, d_off, &d_res))) return rc;
    HIP_TRY(hipEventRecord(t->ev[kEvStageEnd], s));
    HIP_TRY(hipStreamSynchronize(s));
    set->st.orfs = (int64_t)n;
    set->st.complete = (int64_t)h[kg::kOrfErrWords + kg::kOrfCntComplete];
    set->st.interrupted = (int64_t)h[kg::kOrfErrWords + kg::kOrfCntInterrupted];
    set->st.partial5 = (int64_t)h[kg::kOrfErrWords + kg::kOrfCntPartial5];
    set->st.residues = (int64_t)n_res;
    set->st.tiles = (int64_t)n_tiles;
    HIP_TRY(hipEventElapsedTime(&set->st.ms, t->ev[kEvStageBegin], t->ev[kEvStageEnd]));
    keep_orfs(set, sc, d_out, d_start, d_res, n, n_res, n_seqs);
    return KG_OK;
}

// The free candidates of the batch behind the records of `parent` (null: alone).  d_seq, offsets and set as orfs_impl has them.
int free_impl(kg_table *t, const kg_free_params *prm, const kg_orfset *parent, const uint8_t *d_seq, const int64_t *offsets,
              uint64_t n_seqs, kg_orfset *set)
{
    OrfPlanes pl;
    Scratch sc(t);
    hipStream_t s = t->stream;
    int rc;
    if ((rc = pl.plan(offsets, n_seqs))) return rc;
    set->l_max = std::max(parent ? parent->l_max : 0, pl.l_max);
    const uint64_t n0 = parent ? (uint64_t)parent->count : 0, n_slots = 6 * pl.n_rows;
    unsigned long long *words = nullptr;           // kg::kOrfFree*
    uint32_t *slots = nullptr, *slot_first = nullptr;
    uint64_t *slot_partial = nullptr;
    if ((rc = pl.alloc_geometry(sc)) || (rc = sc.get(&words, 16)) || (rc = pl.alloc_keys(sc)) ||
        (rc = sc.get(&slots, std::max<uint64_t>(n_slots, 1))) || (rc = sc.get(&slot_first, std::max<uint64_t>(n_slots, 1))) ||
        (rc = sc.get(&slot_partial, n_slots / kg::kScanChunk + 2)))
        return rc;
    if ((rc = pl.upload(s, offsets))) return rc;
    HIP_TRY(hipMemsetAsync(words, 0, kg::kOrfFreeWords * 8, s));
    HIP_TRY(hipEventRecord(t->ev[kEvStageBegin], s));
    const kg::OrfGeometry geo = pl.geometry();
    const uint32_t sc_mask = (uint32_t)prm->start_codons, row_grid = (uint32_t)((pl.n_rows + 3) / 4);
    if ((rc = pl.launch(s, d_seq, sc_mask))) return rc;
    if (pl.n_rows > 0) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(kg::orf_free_kernel<false>), dim3(row_grid), dim3(256), 0, s, d_seq, pl.total, geo, pl.n_rows, pl.keys,
                           prm->min_res, sc_mask, slots, (kg_orf *)nullptr, (uint32_t *)nullptr, (unsigned long long *)nullptr);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, slots, n_slots, slot_first, slot_partial, (uint64_t *)(words + kg::kOrfFreeCount)))) return rc;
    }
    // the first wait: how many candidates there are
    if ((rc = read_error_words(t, words, kg::kOrfFreeWords, kPinStage, {}))) return rc;
    const uint64_t *h = t->h_pin + kPinStage;
    const uint64_t n_free = h[kg::kOrfFreeCount], n = n0 + n_free;
    if (n >= (1ull << 31)) return fail(KG_ERR_LIMIT, "2^31 or more candidates in one call");
    kg_orf *d_out = nullptr;
    int64_t *d_start = nullptr;
    uint32_t *lens = nullptr, *excl = nullptr;
    uint64_t *partial = nullptr;
    if ((rc = sc.get(&d_out, std::max<uint64_t>(n, 1))) || (rc = sc.get(&d_start, n + 1)) || (rc = sc.get(&lens, std::max<uint64_t>(n, 1))) ||
        (rc = sc.get(&excl, std::max<uint64_t>(n, 1))) || (rc = sc.get(&partial, n / kg::kScanChunk + 2)))
        return rc;
    uint64_t *d_total = (uint64_t *)(words + kg::kOrfFreeResidues);
    if (n0 > 0) {
        HIP_TRY(hipMemcpyAsync(d_out, parent->d_orfs, n0 * sizeof(kg_orf), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(kg::orf_lens_kernel, dim3(grid_of(n0)), dim3(256), 0, s, parent->d_prot_start, n0, lens);
    }
    if (n_free > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(kg::orf_free_kernel<true>), dim3(row_grid), dim3(256), 0, s, d_seq, pl.total, geo, pl.n_rows, pl.keys,
                           prm->min_res, sc_mask, slot_first, d_out + n0, lens + n0, words);
    HIP_TRY(hipGetLastError());
    if ((rc = layout_proteins(t, lens, n, excl, partial, d_total, d_start))) return rc;
    // the second wait: the residue total and the counters
    if ((rc = read_error_words(t, words, kg::kOrfFreeWords, kPinStage, {}))) return rc;
    const uint64_t n_res = h[kg::kOrfFreeResidues];
    if (n_res >= (1ull << 32)) return fail(KG_ERR_LIMIT, "2^32 or more residues in one call");
    uint8_t *d_res = nullptr;
    if ((rc = translate_orfs(t, sc, d_out, n, d_start, n_res, d_seq, pl.d_off, &d_res)) ||
        (rc = keep_repaired(t, d_out, n, d_start, n_res, parent, d_res)))
        return rc;
    HIP_TRY(hipEventRecord(t->ev[kEvStageEnd], s));
    HIP_TRY(hipStreamSynchronize(s));
    if (parent) set->st = parent->st;
    set->st.orfs = (int64_t)n;
    set->st.complete += (int64_t)h[kg::kOrfFreeComplete];
    set->st.partial5 += (int64_t)h[kg::kOrfFreePartial5];
    set->st.residues = (int64_t)n_res;
    set->st.tiles = (int64_t)pl.n_tiles;
    HIP_TRY(hipEventElapsedTime(&set->st.ms, t->ev[kEvStageBegin], t->ev[kEvStageEnd]));
    keep_orfs(set, sc, d_out, d_start, d_res, n, n_res, n_seqs);
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_regionset_orfs(kg_regionset *rs, const kg_orf_params *p, const uint8_t *seq, int seq_on_device, const int64_t *offsets,
                      int64_t n_seqs, kg_orfset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!rs) return fail(KG_ERR_ARG, "null kg_regionset");
    int rc = check_orf_params(p);
    if (rc) return rc;
    uint64_t total = 0;
    if ((rc = check_orf_batch(seq, offsets, n_seqs, &total, "region set's", rs->n_seqs))) return rc;
    if (rs->count >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more regions in one call");
    CallScope cs(rs->tab, "a kg_scan* is in flight on this region set's kg_table");
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    std::unique_ptr<kg_orfset> set;
    if ((rc = make_set(cs, set))) return rc;
    Scratch sc(t);
    const uint8_t *d_seq = nullptr;
    if ((rc = batch_on_device(t, sc, seq, seq_on_device, total, &d_seq))) return rc;
    if ((rc = orfs_impl(t, p, rs->d_regions, (uint64_t)rs->count, d_seq, offsets, (uint64_t)n_seqs, set.get()))) return rc;
    return hand_out(cs, set, out);
}

int kg_orfs_regions(int device, const kg_orf_params *p, const kg_region *regions, int64_t n_regions, const uint8_t *seq,
                    const int64_t *offsets, int64_t n_seqs, kg_orfset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = check_orf_params(p);
    if (rc) return rc;
    if (n_regions < 0) return fail(KG_ERR_ARG, "n_regions < 0");
    if (n_regions >= (1ll << 31)) return fail(KG_ERR_LIMIT, "2^31 or more regions in one call");
    if (n_regions && !regions) return fail(KG_ERR_ARG, "null region records");
    uint64_t total = 0;
    if ((rc = check_orf_batch(seq, offsets, n_seqs, &total))) return rc;
    if (n_regions && n_seqs == 0) return fail(KG_ERR_ARG, "region 0: seq outside [0, n_seqs)");
    CallScope cs(device);               // the call's context: closed on every failure below, kept by the set on success
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    std::unique_ptr<kg_orfset> set;
    if ((rc = make_set(cs, set))) return rc;
    {
        Scratch sc(t);
        kg_region *d_regions = nullptr;
        uint8_t *d_seq = nullptr;
        if ((rc = sc.get(&d_regions, n_regions ? (size_t)n_regions : 1)) || (rc = sc.get(&d_seq, total ? total : 1))) return rc;
        if (n_regions) HIP_TRY(hipMemcpyAsync(d_regions, regions, (size_t)n_regions * sizeof(kg_region), hipMemcpyHostToDevice, t->stream));
        if (total && (rc = upload_batch(t, seq, total, d_seq))) return rc;
        if ((rc = orfs_impl(t, p, d_regions, (uint64_t)n_regions, d_seq, offsets, (uint64_t)n_seqs, set.get()))) return rc;
    }
    return hand_out(cs, set, out);
}

int kg_orfs_free(int device, const kg_free_params *p, const uint8_t *seq, int seq_on_device, const int64_t *offsets, int64_t n_seqs,
                 kg_orfset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = check_free_params(p);
    if (rc) return rc;
    uint64_t total = 0;
    if ((rc = check_orf_batch(seq, offsets, n_seqs, &total))) return rc;
    CallScope cs(device);               // the call's context: closed on every failure below, kept by the set on success
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    std::unique_ptr<kg_orfset> set;
    if ((rc = make_set(cs, set))) return rc;
    {
        Scratch sc(t);
        const uint8_t *d_seq = nullptr;
        if ((rc = batch_on_device(t, sc, seq, seq_on_device, total, &d_seq))) return rc;
        if ((rc = free_impl(t, p, nullptr, d_seq, offsets, (uint64_t)n_seqs, set.get()))) return rc;
    }
    return hand_out(cs, set, out);
}

int kg_orfset_add_free(kg_orfset *os, const kg_free_params *p, const uint8_t *seq, int seq_on_device, const int64_t *offsets,
                       int64_t n_seqs, kg_orfset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!os) return fail(KG_ERR_ARG, "null kg_orfset");
    int rc = check_free_params(p);
    if (rc) return rc;
    uint64_t total = 0;
    if ((rc = check_orf_batch(seq, offsets, n_seqs, &total, "ORF set's", os->n_seqs))) return rc;
    CallScope cs(os->tab, "a kg_scan* is in flight on this ORF set's kg_table");
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    std::unique_ptr<kg_orfset> set;
    if ((rc = make_set(cs, set))) return rc;
    Scratch sc(t);
    const uint8_t *d_seq = nullptr;
    if ((rc = batch_on_device(t, sc, seq, seq_on_device, total, &d_seq))) return rc;
    if ((rc = free_impl(t, p, os, d_seq, offsets, (uint64_t)n_seqs, set.get()))) return rc;
    return hand_out(cs, set, out);
}

int64_t kg_orfset_count(const kg_orfset *s) { return s ? s->count : 0; }

const kg_orf *kg_orfset_device(const kg_orfset *s) { return s ? s->d_orfs : nullptr; }

int kg_orfset_copy(const kg_orfset *s, int64_t first, int64_t count, kg_orf *dst)
{
    return copy_records(s, device_of(s), s ? s->d_orfs : nullptr, 1, s ? s->count : 0, first, count, dst, "kg_orfset_copy");
}

int kg_orfset_prot_start(const kg_orfset *s, int64_t *dst)
{
    return copy_starts(s, device_of(s), s ? s->d_prot_start : nullptr, s ? s->count : 0, dst);
}

int kg_orfset_residues(const kg_orfset *s, int64_t first, int64_t count, uint8_t *dst)
{
    return copy_records(s, device_of(s), s ? s->d_res : nullptr, 1, s ? s->residues : 0, first, count, dst, "kg_orfset_residues", "the proteins");
}

int kg_orfset_stats(const kg_orfset *s, kg_orf_stats *out) { return copy_stats(s, s ? &s->st : nullptr, out); }

void kg_orfset_free(kg_orfset *s) { delete s; }

}  // extern "C"
