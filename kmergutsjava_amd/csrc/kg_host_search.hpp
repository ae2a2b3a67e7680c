// kg_host_search.hpp -- kg_proteins_search / kg_proteins_search_device: queries against a database of proteins by shared 8-mers,
// the best candidates aligned (kernels: kg_search.hpp; the window encode, the sort and the collapse are the derive call's,
// kg_derive.hpp; the alignment is align_run of kg_host_align.hpp, unchanged), and kg_proteins_search_paths, which traces the
// ordered records behind it (trace_run of kg_host_trace.hpp).  kg_proteins_search_seeded is the same call with the window kernel
// of kg_seed.hpp in the derive kernel's place: seed ids of a reduced alphabet and spaced shapes where the exact call has 8-mers.
// kg_proteins_search_masked is either call with the window kernels reading the seeding copy of kg_host_mask.hpp (the masked
// residues of one or both sides turned into non-residues); the alignment and the trace read the original.
// kg_proteins_search_filtered is any of them with the ungapped stage of kg_ungapped.hpp between the join and the alignment.
// kg_proteins_search_banded is that call with every candidate aligned, and traced, in a band around its g* (kg_band.hpp).
// search_impl is a driver over three stages: search_pairs (the front half the cluster call has too, by the functions of
// kg_host_derive.hpp: staging, block counts, count pass, one-pass cap, window-pairs pass), search_candidates (search_runs, the
// join and the per-query cut) or, chosen by the call, search_candidates_ungapped (search_runs, the join with the diagonals, the
// best diagonal, the ungapped scores, the cut by them) and search_finish (the result block, the alignment, the order, the
// statistics, the ungapped records' places, the paths).
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_derive.hpp, kg_host_align.hpp, kg_host_trace.hpp and
// kg_host_cluster.hpp (cluster_link_starts_kernel is launched here as well).
#pragma once

struct kg_hitset {
    int device = 0;
    Detached d_block;                   // hit_start[n_q + 1] (int64), then count * 40 bytes
    int64_t count = 0, n_q = 0;
    kg_search_stats st = {};
    Detached d_paths;                   // kg_proteins_search_paths only: one kg_alignment_path per hit record
    bool has_paths = false;
    kg_trace_stats tst = {};
    Detached d_ops;                     // KG_TRACE_OPS / KG_TRACE_OPS_EQX only: op_start[count + 1] (int64), then the ops
    int64_t ops_count = 0;
    bool has_ops = false;
    float ms_ops = 0;
    bool has_mask = false;              // kg_proteins_search_masked only: the statistics of the mask behind the seeding copy
    kg_mask_stats mst = {};
    Detached d_ung;                     // kg_proteins_search_filtered only: one kg_search_ungapped per hit record
    bool has_ung = false;
    kg_ungapped_stats ust = {};
    bool has_band = false;              // kg_proteins_search_banded only: the band's counts over the aligned pairs
    kg_band_stats bst = {};
    bool has_db = false;                // kg_searchdb_search only: the probe's counts and times
    kg_search_db_stats dbst = {};
    const int64_t *op_starts() const { return (const int64_t *)d_ops.p; }
    const uint32_t *ops() const { return (const uint32_t *)(d_ops.p + ((size_t)count + 1) * 8); }
    const int64_t *starts() const { return (const int64_t *)d_block.p; }
    const kg_search_hit *hits() const { return (const kg_search_hit *)(d_block.p + ((size_t)n_q + 1) * 8); }
};

static_assert(sizeof(kg_search_hit) == 40 && sizeof(kg_search_params) == 16 && sizeof(kg_search_stats) == 136 && sizeof(kg_seed_params) == 48,
              "record layouts of include/kmerguts_hip.h");
static_assert(sizeof(kg_ungapped_params) == 16 && sizeof(kg_search_ungapped) == 16 && sizeof(kg::UngappedRec) == 16 && sizeof(kg_ungapped_stats) == 40,
              "record layouts of include/kmerguts_hip.h");

namespace {

constexpr uint64_t kSearchBytesPerPair = 112;                         // device bytes one join pair needs, at most
constexpr uint64_t kSearchPairsMax = (1ull << 32) - (1ull << 22);     // the 32-bit scans and indices of the join
// The ungapped stage, per join pair at most: the sort's two sides 24, the heads of both levels and their scans 16, the starts of
// both levels 8, the best words 8; per candidate (at most one per pair) key, s, diagonal, u, flag and scan 32; per kept candidate
// key, s, record 28, the second sort's two sides 24, heads, scans and top flags 16; per aligned candidate pairs, s and record 28.
// 184, and the histograms and chunk sums of the sorts and scans on top.
constexpr uint64_t kUngappedBytesPerPair = 200;

// kg_proteins_search_paths: which records are traced (trace & 3), whether their ops are written (KG_TRACE_OPS, KG_TRACE_OPS_EQX), and
// the cap of a box.  trace = 0: no paths are asked for
struct SearchPathsAsk { int trace = 0; int64_t max_trace_cells = 0; };

// kg_proteins_search_seeded: a checked kg_seed_params.  space = n_shapes * alphabet^weight <= 2^35
struct SeedPlan { kg::SeedSpec spec; uint32_t span_min; uint64_t space; };

// the first offender of a kg_seed_params, in the header's order, or the plan
int seed_plan(const kg_seed_params *sp, SeedPlan *out)
{
    if (!sp) return fail(KG_ERR_ARG, "null kg_seed_params");
    if (sp->n_shapes < 1 || sp->n_shapes > kg::kSeedMaxShapes) return fail(KG_ERR_ARG, "n_shapes must be in 1..4");
    if (sp->alphabet_size < 2 || sp->alphabet_size > 20) return fail(KG_ERR_ARG, "alphabet_size must be in 2..20");
    uint32_t used = 0;
    for (int c = 0; c < 20; c++) {
        if (sp->cls[c] >= sp->alphabet_size)
            return fail(KG_ERR_ARG, "cls[" + kmer_text(c) + "] must be below alphabet_size: " + kmer_text(sp->cls[c]) + " is not below " +
                                        kmer_text(sp->alphabet_size));
        used |= 1u << sp->cls[c];
    }
    for (int a = 0; a < sp->alphabet_size; a++)
        if (!(used >> a & 1u)) return fail(KG_ERR_ARG, "class " + kmer_text(a) + " is used by no residue: every class below alphabet_size must be");
    for (int k = 0; k < sp->n_shapes; k++)
        if (!(sp->shape[k] & 1u)) return fail(KG_ERR_ARG, "shape[" + kmer_text(k) + "] must have bit 0 set");
    const int w = __builtin_popcount(sp->shape[0]);
    for (int k = 1; k < sp->n_shapes; k++)
        if (__builtin_popcount(sp->shape[k]) != w)
            return fail(KG_ERR_ARG, "shapes must have equal weights: shape[" + kmer_text(k) + "] has " +
                                        kmer_text(__builtin_popcount(sp->shape[k])) + " care positions, shape[0] has " + kmer_text(w));
    for (int k = sp->n_shapes; k < kg::kSeedMaxShapes; k++)
        if (sp->shape[k] != 0) return fail(KG_ERR_ARG, "shape[" + kmer_text(k) + "] must be 0: n_shapes is " + kmer_text(sp->n_shapes));
    if (sp->reserved != 0) return fail(KG_ERR_ARG, "kg_seed_params.reserved must be 0");
    uint64_t per = 1;
    for (int k = 0; k < w && per <= (1ull << 35); k++) per *= (uint64_t)sp->alphabet_size;
    if (per > (1ull << 35) || per * (uint64_t)sp->n_shapes > (1ull << 35))
        return fail(KG_ERR_ARG, "seed space over 2^35: n_shapes * alphabet_size^weight = " + kmer_text(sp->n_shapes) + " * " +
                                    kmer_text(sp->alphabet_size) + "^" + kmer_text(w));
    SeedPlan pl = {};
    pl.spec.n_shapes = (uint32_t)sp->n_shapes;
    pl.spec.alphabet = (uint32_t)sp->alphabet_size;
    pl.span_min = kg::kSeedMaxSpan;
    for (int k = 0; k < sp->n_shapes; k++) {
        const uint32_t span = 32u - (uint32_t)__builtin_clz(sp->shape[k]);
        pl.spec.shape[k] = sp->shape[k];
        pl.spec.span_max = std::max(pl.spec.span_max, span);
        pl.span_min = std::min(pl.span_min, span);
    }
    for (int c = 0; c < 20; c++) pl.spec.cls4[c >> 2] |= (uint32_t)sp->cls[c] << (8 * (c & 3));
    pl.spec.per_shape = per;
    pl.space = per * (uint64_t)sp->n_shapes;
    *out = pl;
    return KG_OK;
}

// derive_block_bases for a seed set: blocks of 64 over the max(len_p - span_min, 0) window positions of protein p
int seed_block_bases(const int64_t *offsets, int64_t n_prot, uint32_t span_min, std::vector<uint32_t> &ibase, uint64_t *nblocks_out)
{
    ibase.assign((size_t)n_prot + 1, 0);
    uint64_t nblocks = 0;
    for (int64_t k = 0; k < n_prot; k++) {
        const int64_t L = offsets[k + 1] - offsets[k];
        ibase[(size_t)k] = (uint32_t)nblocks;
        const uint64_t nwin = L > (int64_t)span_min ? (uint64_t)L - span_min : 0;
        nblocks += (nwin + kg::kAaWinPerBlock - 1) / kg::kAaWinPerBlock;
        if (nblocks > 0x7FFFFFFFull) return fail(KG_ERR_LIMIT, "2^31 or more window blocks of 64 windows in one call");
    }
    ibase[(size_t)n_prot] = (uint32_t)nblocks;
    *nblocks_out = nblocks;
    return KG_OK;
}

// the valid (window, shape) pairs of the batch: the count pass.  Its time goes where the histogram's goes (dv.ms_hist).
int seed_count(Deriver &dv, const SeedPlan *seed, unsigned long long *d_count, uint64_t *n_out)
{
    hipStream_t s = dv.t->stream;
    HIP_TRY(hipMemsetAsync(d_count, 0, 8, s));
    HIP_TRY(hipEventRecord(dv.ev[0], s));
    if (dv.n_blocks) {
        hipLaunchKernelGGL(kg::seed_windows_kernel<false>, dim3(emit_grid(dv.n_blocks)), dim3(kg::kDeriveThreads), 0, s, dv.d_seq, dv.d_blocks,
                           dv.n_blocks, seed->spec, d_count, nullptr, 0u, nullptr, nullptr, nullptr, (uint64_t)0);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(dv.ev[1], s));
    unsigned long long n = 0;
    HIP_TRY(hipMemcpyAsync(&n, d_count, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, dv.ev[0], dv.ev[1]));
    dv.ms_hist += ms;
    *n_out = n;
    return KG_OK;
}

// The ordered records -> one path record each, same index, in a block of the set's own.  KG_TRACE_HITS traces the records with
// status hit, KG_TRACE_ALL every aligned record with score >= 1; a is the query, b the target.
int search_paths_behind(kg_table *t, Scratch &sc, const kg_align_params *al, const uint8_t *d_seq, const int64_t *d_off, int64_t n_db,
                        const kg_search_hit *d_hits, uint64_t NK, const SearchPathsAsk &ask, kg_hitset *set, const kg_band_params *band)
{
    int rc;
    if ((rc = dalloc_detached(t, &set->d_paths.p, std::max<uint64_t>(NK, 1) * sizeof(kg_alignment_path)))) return rc;
    TraceTotals tot;
    const int which = ask.trace & 3;
    OpsAsk ops{ask.trace & (KG_TRACE_OPS | KG_TRACE_OPS_EQX)};
    if (NK == 0 && ops.mode) {                          // no records: op_start[0] = 0 and no ops
        if ((rc = sc.get(&ops.d_block, 16))) return rc;
        HIP_TRY(hipMemset(ops.d_block, 0, 16));
    }
    if (NK > 0) {
        std::vector<kg_search_hit> hits(NK);
        HIP_TRY(hipMemcpy(hits.data(), d_hits, NK * sizeof(kg_search_hit), hipMemcpyDeviceToHost));
        std::vector<int32_t> pairs(2 * NK);
        std::vector<TraceEnd> ends(NK);
        for (uint64_t k = 0; k < NK; k++) {
            const kg_search_hit &h = hits[k];
            pairs[2 * k] = (int32_t)(n_db + h.query);
            pairs[2 * k + 1] = h.target;
            ends[k] = TraceEnd{h.score, h.end_query, h.end_target, which == KG_TRACE_ALL ? h.status != 2 && h.score >= 1 : h.status == 0};
        }
        kg::TracePath *d_paths = nullptr;
        std::vector<int32_t> diag;                      // under a band: g* of every ordered record, from its ungapped record
        if (band) {
            std::vector<kg_search_ungapped> ung(NK);
            HIP_TRY(hipMemcpy(ung.data(), set->d_ung.p, NK * sizeof(kg_search_ungapped), hipMemcpyDeviceToHost));
            diag.resize(NK);
            for (uint64_t k = 0; k < NK; k++) diag[k] = ung[k].diagonal;
        }
        const BandAsk b{diag.data(), band ? band->band : 0};
        if ((rc = trace_run(t, sc, al, d_seq, d_off, pairs.data(), ends, NK, ask.max_trace_cells, &d_paths, &tot, ops.mode ? &ops : nullptr,
                            band ? &b : nullptr)))
            return rc;
        HIP_TRY(hipMemcpy(set->d_paths.p, d_paths, NK * sizeof(kg_alignment_path), hipMemcpyDeviceToDevice));
    }
    set->tst.traced = tot.traced;
    set->tst.untraced = tot.untraced;
    set->tst.cells = tot.cells;
    set->tst.ms_trace = tot.ms;
    set->has_paths = true;
    if (ops.mode) {                                     // the ops block leaves the cache for good, as the path block has
        sc.release(ops.d_block);
        t->cache.detach(ops.d_block);
        set->d_ops.p = ops.d_block;
        set->ops_count = ops.count;
        set->ms_ops = ops.ms;
        set->has_ops = true;
    }
    return KG_OK;
}

// kg_searchdb_search (kg_host_searchdb.hpp): what a call against a resident index reads of the index.  The targets' pairs, runs
// and k-mers are the index's and only the queries' are the call's (SearchPairs::w); d_off holds the targets' offsets and behind
// them the call's queries'.
struct SearchDbSide {
    const uint64_t *pk, *dk;            // the (k-mer, target) pairs v << bits(n_db) | d, and the K distinct k-mers
    const uint32_t *pv, *kstart;        // beside pk; the k-mer run starts, K + 1
    uint64_t P, K, masked;              // masked: the runs longer than the call's max_db_per_kmer
    int64_t longest;                    // the longest target
    unsigned long long *dwords;         // kSearchDbWords counters, zeroed
    hipEvent_t ev_probe[2];             // round the probe
    uint64_t q_kmers = 0, found = 0;    // what the probe gives back: the queries' k-mers, and those the targets have
};

// a checked call.  seed: null for the exact 8-mers; ask.trace = 0: no paths; mask: null for no masking, else `sides` says whose
// residues the seeding copy masks (KG_MASK_QUERIES | KG_MASK_TARGETS)
struct SearchArgs {
    const kg_search_params *prm;
    const kg_align_params *al;
    const uint8_t *h_seq, *d_seq;
    const int64_t *offsets;
    int64_t n_prot, n_db, max_windows, max_pairs;
    SearchPathsAsk ask;
    const SeedPlan *seed;
    const MaskPlan *mask;
    int sides;
    const kg_ungapped_params *ung = nullptr;    // kg_proteins_search_filtered: the ungapped stage in search_candidates' place
    const kg_band_params *band = nullptr;       // kg_proteins_search_banded: the alignment and the trace in a band around g*
    SearchDbSide *res = nullptr;        // kg_searchdb_search: the targets' side of the join is a resident index
};

// what search_impl sets up for its stages: they allocate from sc, enqueue on t->stream and record the timing events ev[1 .. 5]
// (ev[6], ev[7]: the count pass)
struct SearchCall {
    const SearchArgs &a;
    kg_table *t;
    Scratch &sc;
    const Events<8> &ev;
    const uint8_t *d_seq = nullptr;
    const uint8_t *d_seed = nullptr;            // what the window kernels read: d_seq, or under a mask its seeding copy
    unsigned long long *words = nullptr;        // kSearchWords counters, zeroed
    uint64_t *d_tot = nullptr;                  // the totals of the eight prefix sums
};

// search_pairs gives: the n valid windows (seeded: valid (window, shape) pairs) and, where n > 0, their distinct pairs w.P, w.pk,
// w.pv with the arrays of the pass that are free again; the offsets on the device (null: no proteins); the time of the count pass
struct SearchPairs {
    uint64_t n = 0;
    WindowPairs w;
    int64_t *d_off = nullptr;
    float ms_count = 0;
};

// Stage 1: per-protein arrays and window blocks, the count pass, whether the windows fit, the window-pairs pass
int search_pairs(SearchCall &c, SearchPairs *out)
{
    const SearchArgs &a = c.a;
    if (a.n_prot == 0) return KG_OK;
    hipStream_t s = c.t->stream;
    int rc;
    std::vector<uint32_t> ibase;
    uint64_t nblocks = 0, windows = 0;
    if ((rc = a.seed ? seed_block_bases(a.offsets, a.n_prot, a.seed->span_min, ibase, &nblocks)
                     : derive_block_bases(a.offsets, a.n_prot, ibase, &nblocks, &windows)))
        return rc;
    Deriver dv{c.t, c.sc, c.d_seed};
    dv.ev[0] = c.ev[6]; dv.ev[1] = c.ev[7];
    uint32_t *rank_of = nullptr;
    if ((rc = c.sc.get(&dv.d_bins, kg::kDeriveBins)) || (rc = dv.window_blocks(a.offsets, ibase, a.n_prot, nblocks, &out->d_off)) ||
        (rc = c.sc.get(&rank_of, (size_t)a.n_prot)))
        return rc;
    hipLaunchKernelGGL(kg::search_init_kernel, dim3(grid_of(a.n_prot)), dim3(256), 0, s, (uint32_t)a.n_prot, rank_of);
    HIP_TRY(hipGetLastError());

    // ---- the valid windows, and whether they fit: one pass ----
    const uint64_t space = a.seed ? a.seed->space : (uint64_t)KG_MAX_ENCODED;
    if (a.seed) {
        if ((rc = seed_count(dv, a.seed, dv.d_bins, &out->n))) return rc;
    } else {
        std::vector<unsigned long long> bins;
        if ((rc = dv.histogram(0, space, Deriver::shift_for(space), bins))) return rc;
        for (auto cnt : bins) out->n += cnt;
    }
    out->ms_count = dv.ms_hist;
    if ((rc = windows_fit_one_pass(out->n, a.max_windows))) return rc;
    for (int k = 1; k <= 4; k++) HIP_TRY(hipEventRecord(c.ev[k], s));
    if (out->n == 0) return KG_OK;

    // ---- encode and emit (key = v << b | p), sort, collapse to the distinct pairs: the derive call's pass ----
    unsigned long long *d_cur = nullptr;
    if ((rc = c.sc.get(&d_cur, 1))) return rc;
    return dv.window_pairs(c.sc, out->n, 0, space, a.seed ? &a.seed->spec : nullptr, rank_of, bits_for((uint64_t)a.n_prot), d_cur, c.d_tot + 0,
                           c.ev[1], c.ev[2], c.ev[3], &out->w);
}

// search_candidates gives: the NK kept candidates, d_kept_pairs[2 NK] = (n_db + q, d) in query order and d_shared[NK] = s(q, d),
// and the counts of the statistics.  A call that ends early (no windows, no join pair, no candidate) leaves what it did not reach at 0.
struct SearchCands {
    uint64_t K = 0, joined = 0, masked = 0, J = 0, NC = 0, NK = 0;
    int32_t *d_kept_pairs = nullptr, *d_shared = nullptr;
    // search_candidates_ungapped only: d_ung[NK] beside d_shared, the candidates that passed min_ungapped, the cells and the time
    kg::UngappedRec *d_ung = nullptr;
    uint64_t NU = 0, ucells = 0;
    float ms_ungapped = 0;
};

// what search_runs gives the join: the R listed runs (first pair, targets) and wx[R + 1], the exclusive scan of their weights with
// wx[R] = J, and the chunk sums of a prefix sum over J items
struct SearchRuns {
    uint64_t R = 0, J = 0;
    uint32_t *cstart = nullptr, *cnd = nullptr, *wx = nullptr;
    uint64_t *jpartial = nullptr;
    uint32_t *cqstart = nullptr;        // against a resident index: cstart is a run's first target pair, this its first query pair
};

// kg_host_searchdb.hpp: search_runs and the two join launches against a resident index
int searchdb_runs(SearchCall &c, const SearchPairs &in, bool keep_pv, uint64_t bytes_per_pair, SearchCands *out, SearchRuns *runs);
void searchdb_join(SearchCall &c, const SearchPairs &in, const SearchRuns &runs, const struct UngappedWidths *uw, uint64_t *keys, uint32_t *vals);

// Stage 2, its front: the k-mer runs and their weights, whether the join fits (at bytes_per_pair a pair), the listed runs.  J = 0:
// nothing to join.  keep_pv: the run flags get words of their own and in.w.pv stays what the window-pairs pass left.
int search_runs(SearchCall &c, const SearchPairs &in, bool keep_pv, uint64_t bytes_per_pair, SearchCands *out, SearchRuns *runs)
{
    const SearchArgs &a = c.a;
    if (a.res) return searchdb_runs(c, in, keep_pv, bytes_per_pair, out, runs);
    kg_table *t = c.t;
    Scratch &sc = c.sc;
    hipStream_t s = t->stream;
    unsigned long long *words = c.words;
    uint64_t *d_tot = c.d_tot;
    const uint32_t b = bits_for((uint64_t)a.n_prot), ndb = (uint32_t)a.n_db;
    const uint64_t P = in.w.P;
    uint64_t *const pk = in.w.pk, *const partial = in.w.partial;
    uint64_t K = 0, R = 0;
    int rc;

    // ---- the k-mer runs, their split at n_db and their weights (flags / pidx / partial are reused: K <= P <= n) ----
    uint32_t *kh = in.w.flags, *kx = in.w.pidx, *kstart = nullptr, *nd = nullptr, *w = nullptr, *wf = in.w.pv, *wpos = nullptr;
    hipLaunchKernelGGL(kg::search_kmer_heads_kernel, dim3(grid_of(P)), dim3(256), 0, s, pk, P, b, kh);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, kh, P, kx, partial, d_tot + 1))) return rc;
    HIP_TRY(hipMemcpyAsync(&K, d_tot + 1, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->K = K;
    if ((rc = sc.get(&kstart, K + 1)) || (rc = sc.get(&nd, K)) || (rc = sc.get(&w, K)) || (rc = sc.get(&wpos, K))) return rc;
    if (keep_pv && (rc = sc.get(&wf, K))) return rc;
    hipLaunchKernelGGL(kg::cluster_link_starts_kernel, dim3(grid_of(P)), dim3(256), 0, s, kh, kx, P, d_tot + 1, kstart);
    hipLaunchKernelGGL(kg::search_run_weights_kernel, dim3(grid_of(K)), dim3(256), 0, s, pk, kstart, K, b, ndb, (uint32_t)a.prm->max_db_per_kmer,
                       nd, w, wf, words);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, wf, K, wpos, partial, d_tot + 2))) return rc;
    unsigned long long hw[3] = {};
    HIP_TRY(hipMemcpyAsync(hw, words, sizeof hw, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&R, d_tot + 2, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t J = out->J = hw[kg::kSearchJoinPairs];
    out->joined = hw[kg::kSearchJoined];
    out->masked = hw[kg::kSearchMasked];
    if (R != hw[kg::kSearchJoined]) return fail(KG_ERR_DEVICE, "internal: the listed runs and the joined k-mers differ");

    // ---- whether the join fits: J is the 64-bit sum, exact whatever the stored weights saturate to ----
    Cap cap;
    if ((rc = size_cap(a.max_pairs, " (max_pairs)", bytes_per_pair, kSearchPairsMax, &cap))) return rc;
    if (J > cap.items)
        return fail(KG_ERR_LIMIT, kmer_text((int64_t)J) + " join pairs do not fit this call, which holds " + kmer_text((int64_t)cap.items) +
                                      cap.how + "; a smaller max_db_per_kmer masks more of the frequent k-mers");
    if (J == 0) return KG_OK;

    // ---- the runs of weight >= 1, the prefix sum of their weights (J < 2^32: no stored weight is saturated) ----
    uint32_t *cstart = nullptr, *cnd = nullptr, *cw = nullptr, *wx = nullptr;
    uint64_t *jpartial = nullptr;
    if ((rc = sc.get(&cstart, R)) || (rc = sc.get(&cnd, R)) || (rc = sc.get(&cw, R + 1)) || (rc = sc.get(&wx, R + 1)) ||
        (rc = sc.get(&jpartial, J / kg::kScanChunk + 3)))
        return rc;
    HIP_TRY(hipMemsetAsync(cw + R, 0, 4, s));
    hipLaunchKernelGGL(kg::search_run_compact_kernel, dim3(grid_of(K)), dim3(256), 0, s, kstart, nd, w, wf, wpos, K, R, cstart, cnd, cw);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, cw, R + 1, wx, partial, d_tot + 3))) return rc;
    *runs = SearchRuns{R, J, cstart, cnd, wx, jpartial};
    return KG_OK;
}

// Stage 2: search_runs, the join and its sort, the (q, d) runs, the candidates, the cut per query
int search_candidates(SearchCall &c, const SearchPairs &in, SearchCands *out)
{
    if (in.n == 0) return KG_OK;
    const SearchArgs &a = c.a;
    kg_table *t = c.t;
    Scratch &sc = c.sc;
    hipStream_t s = t->stream;
    unsigned long long *words = c.words;
    uint64_t *d_tot = c.d_tot;
    const uint32_t b = bits_for((uint64_t)a.n_prot), db = bits_for((uint64_t)a.n_db), ndb = (uint32_t)a.n_db, qb = bits_for((uint64_t)(a.n_prot - a.n_db));
    uint64_t *const pk = in.w.pk;
    uint64_t ND = 0;
    int rc;
    SearchRuns runs;
    if ((rc = search_runs(c, in, false, kSearchBytesPerPair, out, &runs))) return rc;
    const uint64_t R = runs.R, J = runs.J;
    if (J == 0) return KG_OK;
    uint32_t *const cstart = runs.cstart, *const cnd = runs.cnd, *const wx = runs.wx;
    uint64_t *const jpartial = runs.jpartial;
    // ---- the join: one key per (query, target) of every listed run ----
    SortPairs jp;
    if ((rc = jp.alloc(sc, J))) return rc;
    if (a.res)
        searchdb_join(c, in, runs, nullptr, jp.keys(), jp.vals());
    else
        hipLaunchKernelGGL(kg::search_join_kernel, dim3(grid_of(J, kg::kSearchTile)), dim3(kg::kSearchThreads), 0, s, pk, wx, cstart, cnd, (uint32_t)R,
                           (uint32_t)J, b, ndb, db, jp.keys(), jp.vals());
    HIP_TRY(hipGetLastError());
    uint64_t wtot = 0;
    HIP_TRY(hipMemcpyAsync(&wtot, d_tot + 3, 8, hipMemcpyDeviceToHost, s));
    if ((rc = jp.sort(t, sc, J, qb + db))) return rc;
    // ---- runs of equal keys = distinct (q, d), run length = s(q, d) ----
    uint32_t *lh = nullptr, *lr = nullptr, *lstart = nullptr;
    if ((rc = sc.get(&lh, J)) || (rc = sc.get(&lr, J))) return rc;
    hipLaunchKernelGGL(kg::derive_key_heads_kernel, dim3(grid_of(J)), dim3(256), 0, s, jp.keys(), J, lh);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, lh, J, lr, jpartial, d_tot + 4))) return rc;
    HIP_TRY(hipMemcpyAsync(&ND, d_tot + 4, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (wtot != J) return fail(KG_ERR_DEVICE, "internal: the prefix sum of the weights and their 64-bit sum differ");
    if ((rc = sc.get(&lstart, ND + 1))) return rc;
    uint32_t *cf = lh, *cx = lr;                        // (the heads and their scan are free behind the starts: ND <= J)
    hipLaunchKernelGGL(kg::cluster_link_starts_kernel, dim3(grid_of(J)), dim3(256), 0, s, lh, lr, J, d_tot + 4, lstart);
    hipLaunchKernelGGL(kg::search_cand_flags_kernel, dim3(grid_of(ND)), dim3(256), 0, s, lstart, ND, (uint32_t)a.prm->min_shared, cf, words);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, cf, ND, cx, jpartial, d_tot + 5))) return rc;
    unsigned long long smax = 0;
    uint64_t NC = 0;
    HIP_TRY(hipMemcpyAsync(&NC, d_tot + 5, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&smax, words + kg::kSearchSmax, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->NC = NC;
    if (NC == 0) return KG_OK;

    // ---- the candidates in (q, d) order, then stably by (q, descending s): ties stay in ascending d ----
    const uint32_t sb = bit_width(smax);
    uint64_t *ckey = nullptr;
    uint32_t *cs = nullptr, *qh = nullptr, *qx = nullptr, *qstart = nullptr, *tf = nullptr, *tx = nullptr;
    SortPairs cp;
    if ((rc = sc.get(&ckey, NC)) || (rc = sc.get(&cs, NC)) || (rc = cp.alloc(sc, NC)) || (rc = sc.get(&qh, NC)) || (rc = sc.get(&qx, NC)) ||
        (rc = sc.get(&tf, NC)) || (rc = sc.get(&tx, NC)))
        return rc;
    hipLaunchKernelGGL(kg::search_cand_emit_kernel, dim3(grid_of(ND)), dim3(256), 0, s, jp.keys(), lstart, cf, cx, ND, NC, db, sb, (uint32_t)smax,
                       ckey, cs, cp.keys(), cp.vals());
    HIP_TRY(hipGetLastError());
    if ((rc = cp.sort(t, sc, NC, qb + sb))) return rc;
    hipLaunchKernelGGL(kg::search_query_heads_kernel, dim3(grid_of(NC)), dim3(256), 0, s, cp.keys(), NC, sb, qh);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, qh, NC, qx, jpartial, d_tot + 6))) return rc;
    uint64_t NQ = 0, NK = 0;
    HIP_TRY(hipMemcpyAsync(&NQ, d_tot + 6, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = sc.get(&qstart, NQ + 1))) return rc;
    hipLaunchKernelGGL(kg::cluster_link_starts_kernel, dim3(grid_of(NC)), dim3(256), 0, s, qh, qx, NC, d_tot + 6, qstart);
    hipLaunchKernelGGL(kg::search_top_flags_kernel, dim3(grid_of(NC)), dim3(256), 0, s, qh, qx, qstart, NC, (uint32_t)a.prm->max_cand, tf);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, tf, NC, tx, jpartial, d_tot + 7))) return rc;
    HIP_TRY(hipMemcpyAsync(&NK, d_tot + 7, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->NK = NK;
    if ((rc = sc.get(&out->d_kept_pairs, 2 * NK)) || (rc = sc.get(&out->d_shared, NK))) return rc;
    hipLaunchKernelGGL(kg::search_top_emit_kernel, dim3(grid_of(NC)), dim3(256), 0, s, cp.vals(), ckey, cs, tf, tx, NC, NK, db, ndb,
                       out->d_kept_pairs, out->d_shared);
    HIP_TRY(hipGetLastError());
    return KG_OK;
}

// the widths of the ungapped stage's join key (q << db | d) << gb | (g + bias): bias = the longest target - 1, gb = the bits of
// the longest query + the longest target, which is above every g + bias
struct UngappedWidths { uint32_t qb, db, gb; int32_t bias; };

int ungapped_widths(const SearchArgs &a, UngappedWidths *out)
{
    int64_t lq = 0, ld = a.res ? a.res->longest : 0;
    for (int64_t p = a.res ? a.n_db : 0; p < a.n_prot; p++) {
        int64_t &longest = p < a.n_db ? ld : lq;
        longest = std::max(longest, a.offsets[p + 1] - a.offsets[p]);
    }
    const UngappedWidths w{bits_for((uint64_t)(a.n_prot - a.n_db)), bits_for((uint64_t)a.n_db), bits_for((uint64_t)(lq + ld)),
                           (int32_t)std::max<int64_t>(ld - 1, 0)};
    if (w.qb + w.db + w.gb > 64)
        return fail(KG_ERR_LIMIT, "the join key of the ungapped stage does not fit 64 bits: " + kmer_text(w.qb) + " bits of the queries, " +
                                      kmer_text(w.db) + " of the targets and " + kmer_text(w.gb) +
                                      " of the diagonals (the longest query plus the longest target)");
    *out = w;
    return KG_OK;
}

// Stage 2 of kg_proteins_search_filtered: search_runs with pv kept, the join with the diagonals, its sort, the (q, d) and
// (q, d, g) runs, the best diagonal of every candidate, the ungapped scores, the cut by min_ungapped and the cut per query by
// (u, s, d).  Gives what search_candidates gives, and d_ung beside d_shared.
int search_candidates_ungapped(SearchCall &c, const SearchPairs &in, SearchCands *out)
{
    if (in.n == 0) return KG_OK;
    const SearchArgs &a = c.a;
    kg_table *t = c.t;
    Scratch &sc = c.sc;
    hipStream_t s = t->stream;
    unsigned long long *words = c.words;
    uint64_t *d_tot = c.d_tot;
    const uint32_t b = bits_for((uint64_t)a.n_prot), ndb = (uint32_t)a.n_db;
    int rc;
    UngappedWidths uw;
    if ((rc = ungapped_widths(a, &uw))) return rc;
    const uint32_t qb = uw.qb, db = uw.db, gb = uw.gb;
    SearchRuns runs;
    if ((rc = search_runs(c, in, true, kUngappedBytesPerPair, out, &runs))) return rc;
    const uint64_t R = runs.R, J = runs.J;
    if (J == 0) return KG_OK;
    uint64_t *const jpartial = runs.jpartial;
    Events<2> uev;
    uint64_t *d_tot2 = nullptr;                         // the totals of this stage's own prefix sums
    unsigned long long *uwords = nullptr;
    if ((rc = uev.create()) || (rc = sc.get(&d_tot2, 4)) || (rc = sc.get(&uwords, kg::kUngappedWords))) return rc;
    HIP_TRY(hipMemsetAsync(uwords, 0, kg::kUngappedWords * 8, s));

    // ---- the join with the diagonals, sorted: inside a (q, d) run the diagonals ascend ----
    SortPairs jp;
    if ((rc = jp.alloc(sc, J))) return rc;
    if (a.res)
        searchdb_join(c, in, runs, &uw, jp.keys(), jp.vals());
    else
        hipLaunchKernelGGL(kg::search_join_diag_kernel, dim3(grid_of(J, kg::kSearchTile)), dim3(kg::kSearchThreads), 0, s, in.w.pk, in.w.pv, in.d_off,
                           runs.wx, runs.cstart, runs.cnd, (uint32_t)R, (uint32_t)J, b, ndb, db, gb, uw.bias, jp.keys(), jp.vals());
    HIP_TRY(hipGetLastError());
    uint64_t wtot = 0, ND = 0, NG = 0;
    HIP_TRY(hipMemcpyAsync(&wtot, d_tot + 3, 8, hipMemcpyDeviceToHost, s));
    if ((rc = jp.sort(t, sc, J, qb + db + gb))) return rc;
    // ---- the (q, d) runs (length s) and inside them the (q, d, g) runs (length m) ----
    uint32_t *lh = nullptr, *lr = nullptr, *gh = nullptr, *gr = nullptr, *lstart = nullptr, *gstart = nullptr;
    if ((rc = sc.get(&lh, J)) || (rc = sc.get(&lr, J)) || (rc = sc.get(&gh, J)) || (rc = sc.get(&gr, J))) return rc;
    hipLaunchKernelGGL(kg::search_query_heads_kernel, dim3(grid_of(J)), dim3(256), 0, s, jp.keys(), J, gb, lh);
    hipLaunchKernelGGL(kg::derive_key_heads_kernel, dim3(grid_of(J)), dim3(256), 0, s, jp.keys(), J, gh);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, lh, J, lr, jpartial, d_tot + 4)) || (rc = prefix_sum(t, gh, J, gr, jpartial, d_tot2 + 0))) return rc;
    HIP_TRY(hipMemcpyAsync(&ND, d_tot + 4, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&NG, d_tot2 + 0, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (wtot != J) return fail(KG_ERR_DEVICE, "internal: the prefix sum of the weights and their 64-bit sum differ");
    unsigned long long *best = nullptr;
    uint32_t *cf = nullptr, *cx = nullptr;
    if ((rc = sc.get(&lstart, ND + 1)) || (rc = sc.get(&gstart, NG + 1)) || (rc = sc.get(&best, ND)) || (rc = sc.get(&cf, ND)) ||
        (rc = sc.get(&cx, ND)))
        return rc;
    HIP_TRY(hipMemsetAsync(best, 0, ND * 8, s));
    hipLaunchKernelGGL(kg::cluster_link_starts_kernel, dim3(grid_of(J)), dim3(256), 0, s, lh, lr, J, d_tot + 4, lstart);
    hipLaunchKernelGGL(kg::cluster_link_starts_kernel, dim3(grid_of(J)), dim3(256), 0, s, gh, gr, J, d_tot2 + 0, gstart);
    hipLaunchKernelGGL(kg::ungapped_best_kernel, dim3(grid_of(NG)), dim3(256), 0, s, jp.keys(), gstart, NG, lh, lr, gb, best);
    hipLaunchKernelGGL(kg::search_cand_flags_kernel, dim3(grid_of(ND)), dim3(256), 0, s, lstart, ND, (uint32_t)a.prm->min_shared, cf, words);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, cf, ND, cx, jpartial, d_tot + 5))) return rc;
    unsigned long long smax = 0;
    uint64_t NC = 0;
    HIP_TRY(hipMemcpyAsync(&NC, d_tot + 5, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&smax, words + kg::kSearchSmax, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->NC = NC;
    if (NC == 0) return KG_OK;

    // ---- the candidates in (q, d) order with s, g* and m(g*); their ungapped scores ----
    uint64_t *ckey = nullptr;
    uint32_t *cs = nullptr, *kf = nullptr, *kx = nullptr;
    uint2 *cdiag = nullptr;
    int32_t *cu = nullptr;
    int8_t *d_matrix = nullptr;
    if ((rc = sc.get(&ckey, NC)) || (rc = sc.get(&cs, NC)) || (rc = sc.get(&cdiag, NC)) || (rc = sc.get(&cu, NC)) || (rc = sc.get(&kf, NC)) ||
        (rc = sc.get(&kx, NC)))
        return rc;
    if (a.al->matrix) {
        if ((rc = sc.get(&d_matrix, 21 * 21))) return rc;
        HIP_TRY(hipMemcpyAsync(d_matrix, a.al->matrix, 21 * 21, hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(kg::ungapped_cand_kernel, dim3(grid_of(ND)), dim3(256), 0, s, jp.keys(), lstart, cf, cx, best, ND, NC, gb, ckey, cs, cdiag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(uev[0], s));
    {
        // one wave per 64 candidates and trip; 8 workgroups of 4 waves per CU at most
        const uint32_t chunks = (uint32_t)((NC + kg::kWave - 1) / kg::kWave);
        const uint32_t grid = std::max(std::min<uint32_t>((chunks + 3) / 4, 256u * 8), 1u);
        hipLaunchKernelGGL(kg::search_ungapped_kernel, dim3(grid), dim3(kg::kUngappedThreads), 0, s, c.d_seq, in.d_off, ckey, cdiag, (uint32_t)NC,
                           ndb, db, uw.bias, d_matrix, cu, uwords);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(uev[1], s));
    hipLaunchKernelGGL(kg::ungapped_keep_kernel, dim3(grid_of(NC)), dim3(256), 0, s, cu, NC, (int32_t)a.ung->min_ungapped, kf);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, kf, NC, kx, jpartial, d_tot2 + 1))) return rc;
    unsigned long long huw[kg::kUngappedWords] = {};
    uint64_t NU = 0;
    HIP_TRY(hipMemcpyAsync(&NU, d_tot2 + 1, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(huw, uwords, sizeof huw, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->NU = NU;
    out->ucells = huw[kg::kUngappedCells];
    out->ms_ungapped = uev.ms(0, 1);
    if (NU == 0) return KG_OK;

    // ---- the kept candidates, still in (q, d) order, then stably by (q, descending u, descending s): ties stay in ascending d ----
    const uint64_t umax = huw[kg::kUngappedUmax];
    const uint32_t sb = bit_width(smax), ub = bit_width(umax);
    if (qb + ub + sb > 64)
        return fail(KG_ERR_LIMIT, "the cut key of the ungapped stage does not fit 64 bits: " + kmer_text(qb) + " bits of the queries, " +
                                      kmer_text(ub) + " of the ungapped scores and " + kmer_text(sb) + " of the shared counts");
    uint64_t *kkey = nullptr;
    uint32_t *ks = nullptr, *qh = nullptr, *qx = nullptr, *qstart = nullptr, *tf = nullptr, *tx = nullptr;
    kg::UngappedRec *krec = nullptr;
    SortPairs cp;
    if ((rc = sc.get(&kkey, NU)) || (rc = sc.get(&ks, NU)) || (rc = sc.get(&krec, NU)) || (rc = cp.alloc(sc, NU)) || (rc = sc.get(&qh, NU)) ||
        (rc = sc.get(&qx, NU)) || (rc = sc.get(&tf, NU)) || (rc = sc.get(&tx, NU)))
        return rc;
    hipLaunchKernelGGL(kg::ungapped_emit_kernel, dim3(grid_of(NC)), dim3(256), 0, s, ckey, cs, cdiag, cu, kf, kx, NC, NU, db, sb, ub, (uint32_t)smax,
                       (uint32_t)umax, uw.bias, kkey, ks, krec, cp.keys(), cp.vals());
    HIP_TRY(hipGetLastError());
    if ((rc = cp.sort(t, sc, NU, qb + ub + sb))) return rc;
    hipLaunchKernelGGL(kg::search_query_heads_kernel, dim3(grid_of(NU)), dim3(256), 0, s, cp.keys(), NU, ub + sb, qh);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, qh, NU, qx, jpartial, d_tot + 6))) return rc;
    uint64_t NQ = 0, NK = 0;
    HIP_TRY(hipMemcpyAsync(&NQ, d_tot + 6, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = sc.get(&qstart, NQ + 1))) return rc;
    hipLaunchKernelGGL(kg::cluster_link_starts_kernel, dim3(grid_of(NU)), dim3(256), 0, s, qh, qx, NU, d_tot + 6, qstart);
    hipLaunchKernelGGL(kg::search_top_flags_kernel, dim3(grid_of(NU)), dim3(256), 0, s, qh, qx, qstart, NU, (uint32_t)a.prm->max_cand, tf);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, tf, NU, tx, jpartial, d_tot + 7))) return rc;
    HIP_TRY(hipMemcpyAsync(&NK, d_tot + 7, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->NK = NK;
    if ((rc = sc.get(&out->d_kept_pairs, 2 * NK)) || (rc = sc.get(&out->d_shared, NK)) || (rc = sc.get(&out->d_ung, NK))) return rc;
    hipLaunchKernelGGL(kg::search_top_emit_kernel, dim3(grid_of(NU)), dim3(256), 0, s, cp.vals(), kkey, ks, tf, tx, NU, NK, db, ndb,
                       out->d_kept_pairs, out->d_shared);
    hipLaunchKernelGGL(kg::ungapped_top_emit_kernel, dim3(grid_of(NU)), dim3(256), 0, s, cp.vals(), krec, tf, tx, NU, NK, out->d_ung);
    HIP_TRY(hipGetLastError());
    return KG_OK;
}

// Stage 3: the result block with hit_start, the kept candidates aligned and ordered, the cross-checks, the statistics, and the
// paths where the call asks for them.  The set owns its blocks from their allocation on: a set freed after a failure frees them.
int search_finish(SearchCall &c, const SearchPairs &pairs, const SearchCands &cd, kg_hitset *set)
{
    const SearchArgs &a = c.a;
    kg_table *t = c.t;
    hipStream_t s = t->stream;
    const int64_t n_db = a.n_db, n_q = a.n_prot - a.n_db;
    const uint64_t NK = cd.NK;
    int rc;
    set->n_q = n_q;
    const size_t start_bytes = ((size_t)n_q + 1) * 8;
    if ((rc = dalloc_detached(t, &set->d_block.p, start_bytes + std::max<uint64_t>(NK, 1) * sizeof(kg_search_hit)))) return rc;
    uint8_t *const block = set->d_block.p;
    std::vector<int64_t> h_start((size_t)n_q + 1, 0);
    std::vector<int32_t> h_pairs(2 * NK);
    AlignTotals atot;
    if (NK > 0) {
        HIP_TRY(hipMemcpyAsync(h_pairs.data(), cd.d_kept_pairs, NK * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint64_t k = 0; k < NK; k++) {
            const int64_t q = (int64_t)h_pairs[2 * k] - n_db;
            if (q < 0 || q >= n_q || h_pairs[2 * k + 1] < 0 || h_pairs[2 * k + 1] >= n_db)
                return fail(KG_ERR_DEVICE, "internal: a candidate outside the batch");
            h_start[(size_t)q + 1]++;
        }
        for (int64_t q = 0; q < n_q; q++) {
            if (h_start[(size_t)q + 1] > a.prm->max_cand) return fail(KG_ERR_DEVICE, "internal: more than max_cand candidates of one query");
            h_start[(size_t)q + 1] += h_start[(size_t)q];
        }
    }
    HIP_TRY(hipMemcpyAsync(block, h_start.data(), start_bytes, hipMemcpyHostToDevice, s));
    if (NK > 0) {
        const int32_t *d_pairs = nullptr;
        kg::AlignRec *d_aln = nullptr;
        std::vector<int32_t> diag;                      // under a band: g* of every kept candidate, in the kept order
        if (a.band) {
            std::vector<kg::UngappedRec> ung(NK);
            HIP_TRY(hipMemcpyAsync(ung.data(), cd.d_ung, NK * sizeof(kg::UngappedRec), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            diag.resize(NK);
            for (uint64_t k = 0; k < NK; k++) diag[k] = ung[k].diagonal;
        }
        const BandAsk b{diag.data(), a.band ? a.band->band : 0};
        if ((rc = align_run(t, c.sc, a.al, c.d_seq, pairs.d_off, a.offsets, h_pairs.data(), NK, &d_pairs, &d_aln, &atot, a.band ? &b : nullptr)))
            return rc;
        hipLaunchKernelGGL(kg::search_order_kernel, dim3(grid_of((uint64_t)n_q, 256 / kg::kWave)), dim3(256), 0, s, d_pairs, d_aln, cd.d_shared,
                           (const int64_t *)block, (uint32_t)n_q, (int64_t)a.al->min_ratio_pct, (int)(a.al->ref == KG_ALIGN_REF_MEMBER),
                           (int2 *)(block + start_bytes), c.words);
        HIP_TRY(hipGetLastError());
    }
    if (a.ung) {                                        // the 16-byte records to the places the order gave their candidates
        if ((rc = dalloc_detached(t, &set->d_ung.p, std::max<uint64_t>(NK, 1) * sizeof(kg_search_ungapped)))) return rc;
        if (NK > 0) {
            hipLaunchKernelGGL(kg::ungapped_place_kernel, dim3(grid_of(NK)), dim3(256), 0, s, (const int2 *)(block + start_bytes),
                               (const int64_t *)block, cd.d_kept_pairs, cd.d_ung, NK, (uint32_t)n_q, (kg::UngappedRec *)set->d_ung.p);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(c.ev[5], s));
    unsigned long long hw[kg::kSearchWords] = {};
    HIP_TRY(hipMemcpyAsync(hw, c.words, sizeof hw, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((int64_t)hw[kg::kSearchSkipped] != atot.skipped) return fail(KG_ERR_DEVICE, "internal: the device and the host skipped different pairs");
    if (hw[kg::kSearchHits] + hw[kg::kSearchBelow] + hw[kg::kSearchSkipped] != NK)
        return fail(KG_ERR_DEVICE, "internal: the ordered records and the kept candidates differ");
    kg_search_stats &st = set->st;
    st.targets = n_db;
    st.queries = n_q;
    st.valid_windows = (int64_t)pairs.n;
    st.pairs = (int64_t)pairs.w.P;
    st.kmers = (int64_t)cd.K;
    st.kmers_joined = (int64_t)cd.joined;
    st.kmers_masked = (int64_t)cd.masked;
    st.join_pairs = (int64_t)cd.J;
    st.candidates = (int64_t)cd.NC;
    st.aligned = (int64_t)NK - atot.skipped;
    st.hits = (int64_t)hw[kg::kSearchHits];
    st.skipped = atot.skipped;
    st.queries_hit = (int64_t)hw[kg::kSearchQueriesHit];
    st.cells = atot.cells;
    st.ms_encode = pairs.ms_count + c.ev.ms(1, 2);
    st.ms_sort = c.ev.ms(2, 3);
    st.ms_join = c.ev.ms(3, 4);
    st.ms_align = c.ev.ms(4, 5);
    st.ms_total = c.ev.ms(0, 5);
    if (a.ung) {
        st.ms_join = std::max(st.ms_join - cd.ms_ungapped, 0.0f);
        set->ust.scored = (int64_t)cd.NC;
        set->ust.dropped = (int64_t)(cd.NC - cd.NU);
        set->ust.cut = (int64_t)(cd.NU - NK);
        set->ust.cells = (int64_t)cd.ucells;
        set->ust.ms_ungapped = cd.ms_ungapped;
        set->has_ung = true;
    }
    if (a.band) {
        set->bst.band_cells = atot.band_cells;
        set->bst.full_cells = atot.cells;
        set->bst.band = a.band->band;
        set->has_band = true;
    }
    set->count = (int64_t)NK;
    return a.ask.trace ? search_paths_behind(t, c.sc, a.al, c.d_seq, pairs.d_off, n_db, set->hits(), NK, a.ask, set, a.band) : KG_OK;
}

int search_impl(kg_table *t, const SearchArgs &a, kg_hitset *set)
{
    hipStream_t s = t->stream;
    Scratch sc(t);
    Events<8> ev;
    int rc;
    if ((rc = ev.create())) return rc;
    SearchCall c{a, t, sc, ev};
    if ((rc = stage_sequence(t, sc, a.h_seq, a.d_seq, a.n_prot ? (uint64_t)a.offsets[a.n_prot] : 0, &c.d_seq))) return rc;
    HIP_TRY(hipEventRecord(ev[0], s));
    if ((rc = sc.get(&c.words, kg::kSearchWords)) || (rc = sc.get(&c.d_tot, 8))) return rc;
    HIP_TRY(hipMemsetAsync(c.words, 0, kg::kSearchWords * 8, s));
    c.d_seed = c.d_seq;
    if (a.mask) {                               // the masked side's proteins: the targets [0, n_db), the queries [n_db, n_prot), or all
        const int64_t p0 = a.sides & KG_MASK_TARGETS ? 0 : a.n_db, p1 = a.sides & KG_MASK_QUERIES ? a.n_prot : a.n_db;
        if ((rc = mask_seeding_copy(t, sc, *a.mask, c.d_seq, a.offsets, p0, p1, a.n_prot ? (uint64_t)a.offsets[a.n_prot] : 0, &c.d_seed,
                                    &set->mst)))
            return rc;
        set->has_mask = true;
    }
    // the times of a call that ends early: every stage it did not reach is empty (a stage that is reached records its events again)
    for (int k = 1; k <= 4; k++) HIP_TRY(hipEventRecord(ev[k], s));
    SearchPairs pairs;
    SearchCands cands;
    UngappedWidths fits;                        // (a call whose diagonals do not fit its join key ends before the window pass)
    if (a.ung && (rc = ungapped_widths(a, &fits))) return rc;
    if ((rc = search_pairs(c, &pairs)) || (rc = a.ung ? search_candidates_ungapped(c, pairs, &cands) : search_candidates(c, pairs, &cands)))
        return rc;
    if (pairs.n > 0) HIP_TRY(hipEventRecord(ev[4], s));
    return search_finish(c, pairs, cands, set);
}

// seeds: no value for the exact call; of a seeded call the caller's pointer, checked here
int search_entry(int device, const kg_search_params *prm, const kg_align_params *al, const uint8_t *h_seq, const uint8_t *d_seq,
                 const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows, int64_t max_pairs, kg_hitset **out,
                 SearchPathsAsk ask = {}, std::optional<const kg_seed_params *> seeds = std::nullopt,
                 std::optional<const kg_mask_params *> mask = std::nullopt, int sides = 0,
                 std::optional<const kg_ungapped_params *> ung = std::nullopt, std::optional<const kg_band_params *> band = std::nullopt)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!prm) return fail(KG_ERR_ARG, "null kg_search_params");
    if (prm->min_shared < 1) return fail(KG_ERR_ARG, "min_shared must be >= 1");
    if (prm->max_cand < 1 || prm->max_cand > kg::kSearchMaxCand) return fail(KG_ERR_ARG, "max_cand must be in 1..64");
    if (prm->max_db_per_kmer < 1) return fail(KG_ERR_ARG, "max_db_per_kmer must be >= 1");
    if (prm->reserved != 0) return fail(KG_ERR_ARG, "kg_search_params.reserved must be 0");
    SeedPlan plan;
    if (seeds)
        if (int rc = seed_plan(*seeds, &plan)) return rc;
    MaskPlan mplan;
    if (mask) {
        if (int rc = mask_plan(*mask, &mplan)) return rc;
        if (sides < 1 || sides > (KG_MASK_QUERIES | KG_MASK_TARGETS)) return fail(KG_ERR_ARG, "sides must be KG_MASK_QUERIES, KG_MASK_TARGETS or both");
    }
    if (ung) {
        if (!*ung) return fail(KG_ERR_ARG, "null kg_ungapped_params");
        if ((*ung)->min_ungapped < 0) return fail(KG_ERR_ARG, "min_ungapped must be >= 0");
        if ((*ung)->reserved[0] != 0 || (*ung)->reserved[1] != 0 || (*ung)->reserved[2] != 0)
            return fail(KG_ERR_ARG, "kg_ungapped_params.reserved must be 0");
    }
    if (band)
        if (int rc = band_check_params(*band)) return rc;
    if (!al) return fail(KG_ERR_ARG, "null kg_align_params");
    if (int rc = align_check_params(al)) return rc;
    if (max_windows < 0) return fail(KG_ERR_ARG, "max_windows must be >= 0");
    if (max_pairs < 0) return fail(KG_ERR_ARG, "max_pairs must be >= 0");
    if (ask.trace && (ask.trace & 3) != KG_TRACE_HITS && (ask.trace & 3) != KG_TRACE_ALL)
        return fail(KG_ERR_ARG, "trace must be KG_TRACE_HITS or KG_TRACE_ALL");
    if (ask.trace && ((ask.trace & ~15) || (ask.trace & (KG_TRACE_OPS | KG_TRACE_OPS_EQX)) == (KG_TRACE_OPS | KG_TRACE_OPS_EQX)))
        return fail(KG_ERR_ARG, "trace takes at most one of KG_TRACE_OPS and KG_TRACE_OPS_EQX beside its mode, and no bit above 15");
    if (ask.trace && ask.max_trace_cells < 1) return fail(KG_ERR_ARG, "max_trace_cells must be >= 1");
    if (n_prot < 0) return fail(KG_ERR_ARG, "n_prot < 0");
    if (n_prot >= (1ll << 29)) return fail(KG_ERR_LIMIT, "2^29 or more proteins in one call");
    if (n_db < 0 || n_db > n_prot) return fail(KG_ERR_ARG, "n_db must be in 0..n_prot");
    if (int rc = check_protein_offsets(offsets, n_prot, (int64_t)kg::kAlignMaxLen, "2^24")) return rc;
    const uint64_t seq_bytes = n_prot ? (uint64_t)offsets[n_prot] : 0;
    if (seq_bytes && !h_seq && !d_seq) return fail(KG_ERR_ARG, "null sequence");
    CallScope cs(device);               // the call's context: closed when the call returns, the set keeps only its records
    if (cs.rc) return cs.rc;
    kg_hitset *set = new (std::nothrow) kg_hitset();
    if (!set) return fail(KG_ERR_NOMEM, "out of host memory");
    set->device = device;
    const SearchArgs args{prm, al, h_seq, d_seq, offsets, n_prot, n_db, max_windows, max_pairs, ask, seeds ? &plan : nullptr, mask ? &mplan : nullptr, sides,
                          ung ? *ung : nullptr, band ? *band : nullptr};
    int rc = d_seq && hipDeviceSynchronize() != hipSuccess ? fail(KG_ERR_DEVICE, "hipDeviceSynchronize failed") : KG_OK;
    if (!rc) rc = search_impl(cs.t, args, set);
    cs.t->cache.release_all();                          // scratch goes back to the driver
    if (rc) { std::string keep = g_err; kg_hitset_free(set); g_err = keep; return rc; }
    if (getenv("KG_DEBUG"))
        fprintf(stderr, "[kg] kg_proteins_search: targets=%lld queries=%lld valid=%lld pairs=%lld kmers=%lld joined=%lld masked=%lld join_pairs=%lld candidates=%lld aligned=%lld hits=%lld skipped=%lld queries_hit=%lld encode_ms=%.3f sort_ms=%.3f join_ms=%.3f align_ms=%.3f total_ms=%.3f\n",
                (long long)set->st.targets, (long long)set->st.queries, (long long)set->st.valid_windows, (long long)set->st.pairs,
                (long long)set->st.kmers, (long long)set->st.kmers_joined, (long long)set->st.kmers_masked, (long long)set->st.join_pairs,
                (long long)set->st.candidates, (long long)set->st.aligned, (long long)set->st.hits, (long long)set->st.skipped,
                (long long)set->st.queries_hit, set->st.ms_encode, set->st.ms_sort, set->st.ms_join, set->st.ms_align, set->st.ms_total);
    *out = set;
    return KG_OK;
}

// kg_proteins_search_paths must be given a mode: its trace = 0 is refused as trace = 3, neither mode, is, with the same words
SearchPathsAsk paths_ask(int trace, int64_t max_trace_cells) { return {trace ? trace : KG_TRACE_HITS | KG_TRACE_ALL, max_trace_cells}; }

}  // namespace

extern "C" {

int kg_proteins_search(int device, const kg_search_params *p, const kg_align_params *align, const uint8_t *seq, const int64_t *offsets,
                       int64_t n_prot, int64_t n_db, int64_t max_windows, int64_t max_pairs, kg_hitset **out)
{
    return search_entry(device, p, align, seq, nullptr, offsets, n_prot, n_db, max_windows, max_pairs, out);
}

int kg_proteins_search_device(int device, const kg_search_params *p, const kg_align_params *align, const uint8_t *d_seq,
                              const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows, int64_t max_pairs,
                              kg_hitset **out)
{
    return search_entry(device, p, align, nullptr, d_seq, offsets, n_prot, n_db, max_windows, max_pairs, out);
}

int kg_proteins_search_paths(int device, const kg_search_params *p, const kg_align_params *align, const uint8_t *seq, const int64_t *offsets,
                             int64_t n_prot, int64_t n_db, int64_t max_windows, int64_t max_pairs, int trace, int64_t max_trace_cells,
                             kg_hitset **out)
{
    return search_entry(device, p, align, seq, nullptr, offsets, n_prot, n_db, max_windows, max_pairs, out, paths_ask(trace, max_trace_cells));
}

int kg_proteins_search_paths_device(int device, const kg_search_params *p, const kg_align_params *align, const uint8_t *d_seq,
                                    const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows, int64_t max_pairs, int trace,
                                    int64_t max_trace_cells, kg_hitset **out)
{
    return search_entry(device, p, align, nullptr, d_seq, offsets, n_prot, n_db, max_windows, max_pairs, out, paths_ask(trace, max_trace_cells));
}

int kg_seed_params_builtin(int which, kg_seed_params *out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    if (which != KG_SEEDS_EXACT && which != KG_SEEDS_REDUCED) return fail(KG_ERR_ARG, "which must be KG_SEEDS_EXACT or KG_SEEDS_REDUCED");
    kg_seed_params p = {};
    if (which == KG_SEEDS_EXACT) {
        p.n_shapes = 1;
        p.alphabet_size = 20;
        for (int c = 0; c < 20; c++) p.cls[c] = (uint8_t)c;
        p.shape[0] = 0xFFu;
    } else {
        // reduced11: AST, C, DEKNQR, F, G, H, ILV, M, P, W, Y over the code order ACDEFGHIKLMNPQRSTVWY
        static const uint8_t cls[20] = {0, 1, 2, 2, 3, 4, 5, 6, 2, 6, 7, 2, 8, 2, 2, 0, 0, 6, 9, 10};
        p.n_shapes = 2;
        p.alphabet_size = 11;
        memcpy(p.cls, cls, 20);
        p.shape[0] = 0xD6Fu;            // 111101101011, position 0 leftmost = bit 0
        p.shape[1] = 0x659Bu;           // 110110011010011
    }
    *out = p;
    return KG_OK;
}

int kg_proteins_search_seeded(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                              const uint8_t *seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                              int64_t max_pairs, int trace, int64_t max_trace_cells, kg_hitset **out)
{
    return search_entry(device, p, align, seq, nullptr, offsets, n_prot, n_db, max_windows, max_pairs, out, {trace, max_trace_cells}, seeds);
}

int kg_proteins_search_seeded_device(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                                     const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                                     int64_t max_pairs, int trace, int64_t max_trace_cells, kg_hitset **out)
{
    return search_entry(device, p, align, nullptr, d_seq, offsets, n_prot, n_db, max_windows, max_pairs, out, {trace, max_trace_cells}, seeds);
}

// (seeds = NULL: the exact 8-mers, as kg_proteins_search_paths with trace = 0 allowed)
int kg_proteins_search_masked(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                              const uint8_t *seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                              int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides, kg_hitset **out)
{
    return search_entry(device, p, align, seq, nullptr, offsets, n_prot, n_db, max_windows, max_pairs, out, {trace, max_trace_cells},
                        seeds ? std::optional<const kg_seed_params *>(seeds) : std::nullopt, mask, sides);
}

int kg_proteins_search_masked_device(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                                     const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                                     int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                                     kg_hitset **out)
{
    return search_entry(device, p, align, nullptr, d_seq, offsets, n_prot, n_db, max_windows, max_pairs, out, {trace, max_trace_cells},
                        seeds ? std::optional<const kg_seed_params *>(seeds) : std::nullopt, mask, sides);
}

// (seeds = NULL: the exact 8-mers; mask = NULL: no mask, and sides is not read)
int kg_proteins_search_filtered(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                                const uint8_t *seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                                int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                                const kg_ungapped_params *ungapped, kg_hitset **out)
{
    return search_entry(device, p, align, seq, nullptr, offsets, n_prot, n_db, max_windows, max_pairs, out, {trace, max_trace_cells},
                        seeds ? std::optional<const kg_seed_params *>(seeds) : std::nullopt,
                        mask ? std::optional<const kg_mask_params *>(mask) : std::nullopt, sides, ungapped);
}

int kg_proteins_search_filtered_device(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                                       const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                                       int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                                       const kg_ungapped_params *ungapped, kg_hitset **out)
{
    return search_entry(device, p, align, nullptr, d_seq, offsets, n_prot, n_db, max_windows, max_pairs, out, {trace, max_trace_cells},
                        seeds ? std::optional<const kg_seed_params *>(seeds) : std::nullopt,
                        mask ? std::optional<const kg_mask_params *>(mask) : std::nullopt, sides, ungapped);
}

int kg_proteins_search_banded(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                              const uint8_t *seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                              int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                              const kg_ungapped_params *ungapped, const kg_band_params *band, kg_hitset **out)
{
    return search_entry(device, p, align, seq, nullptr, offsets, n_prot, n_db, max_windows, max_pairs, out, {trace, max_trace_cells},
                        seeds ? std::optional<const kg_seed_params *>(seeds) : std::nullopt,
                        mask ? std::optional<const kg_mask_params *>(mask) : std::nullopt, sides, ungapped, band);
}

int kg_proteins_search_banded_device(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                                     const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                                     int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                                     const kg_ungapped_params *ungapped, const kg_band_params *band, kg_hitset **out)
{
    return search_entry(device, p, align, nullptr, d_seq, offsets, n_prot, n_db, max_windows, max_pairs, out, {trace, max_trace_cells},
                        seeds ? std::optional<const kg_seed_params *>(seeds) : std::nullopt,
                        mask ? std::optional<const kg_mask_params *>(mask) : std::nullopt, sides, ungapped, band);
}

int kg_hitset_band_stats(const kg_hitset *s, kg_band_stats *out)
{
    if (s && !s->has_band) return fail(KG_ERR_ARG, "kg_hitset_band_stats: the set was made without a band");
    return copy_stats(s, s ? &s->bst : nullptr, out);
}

int kg_hitset_ungapped_copy(const kg_hitset *s, int64_t first, int64_t count, kg_search_ungapped *dst)
{
    if (s && !s->has_ung) return fail(KG_ERR_ARG, "kg_hitset_ungapped_copy: the set was made without the ungapped stage");
    return copy_records(s, s ? s->device : 0, s ? (const kg_search_ungapped *)s->d_ung.p : nullptr, 1, s ? s->count : 0, first, count, dst,
                        "kg_hitset_ungapped_copy");
}

int kg_hitset_ungapped_stats(const kg_hitset *s, kg_ungapped_stats *out)
{
    if (s && !s->has_ung) return fail(KG_ERR_ARG, "kg_hitset_ungapped_stats: the set was made without the ungapped stage");
    return copy_stats(s, s ? &s->ust : nullptr, out);
}

int kg_hitset_mask_stats(const kg_hitset *s, kg_mask_stats *out)
{
    if (s && !s->has_mask) return fail(KG_ERR_ARG, "kg_hitset_mask_stats: the set was made without a mask");
    return copy_stats(s, s ? &s->mst : nullptr, out);
}

int64_t kg_hitset_count(const kg_hitset *s) { return s ? s->count : 0; }

int kg_hitset_paths_copy(const kg_hitset *s, int64_t first, int64_t count, kg_alignment_path *dst)
{
    if (s && !s->has_paths) return fail(KG_ERR_ARG, "kg_hitset_paths_copy: the set was made without paths");
    return copy_records(s, s ? s->device : 0, s ? (const kg_alignment_path *)s->d_paths.p : nullptr, 1, s ? s->count : 0, first, count, dst, "kg_hitset_paths_copy");
}

int kg_hitset_trace_stats(const kg_hitset *s, kg_trace_stats *out)
{
    if (s && !s->has_paths) return fail(KG_ERR_ARG, "kg_hitset_trace_stats: the set was made without paths");
    return copy_stats(s, s ? &s->tst : nullptr, out);
}

int64_t kg_hitset_ops_count(const kg_hitset *s) { return s ? s->ops_count : 0; }

int kg_hitset_op_starts_copy(const kg_hitset *s, int64_t first, int64_t count, int64_t *dst)
{
    if (s && !s->has_ops) return fail(KG_ERR_ARG, "kg_hitset_op_starts_copy: the set was made without ops");
    return ops_starts_copy(s, s ? s->device : 0, s ? s->op_starts() : nullptr, s ? s->count : 0, first, count, dst, "kg_hitset_op_starts_copy");
}

int kg_hitset_ops_copy(const kg_hitset *s, int64_t first_op, int64_t count, uint32_t *dst)
{
    if (s && !s->has_ops) return fail(KG_ERR_ARG, "kg_hitset_ops_copy: the set was made without ops");
    return copy_records(s, s ? s->device : 0, s ? s->ops() : nullptr, 1, s ? s->ops_count : 0, first_op, count, dst, "kg_hitset_ops_copy");
}

int kg_hitset_ms_ops(const kg_hitset *s, float *out)
{
    if (!s || !out) return fail(KG_ERR_ARG, "null argument");
    if (!s->has_ops) return fail(KG_ERR_ARG, "kg_hitset_ms_ops: the set was made without ops");
    *out = s->ms_ops;
    return KG_OK;
}

int kg_hitset_copy(const kg_hitset *s, int64_t first, int64_t count, kg_search_hit *dst)
{
    return copy_records(s, s ? s->device : 0, s ? s->hits() : nullptr, 1, s ? s->count : 0, first, count, dst, "kg_hitset_copy");
}

int kg_hitset_starts_copy(const kg_hitset *s, int64_t *dst)
{
    return copy_starts(s, s ? s->device : 0, s ? s->starts() : nullptr, s ? s->n_q : 0, dst);
}

int kg_hitset_stats(const kg_hitset *s, kg_search_stats *out) { return copy_stats(s, s ? &s->st : nullptr, out); }

void kg_hitset_free(kg_hitset *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;                           // (its blocks with it)
}

}  // extern "C"
