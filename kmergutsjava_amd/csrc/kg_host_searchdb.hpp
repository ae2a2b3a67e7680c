// kg_host_searchdb.hpp -- kg_searchdb_*: a resident index of a protein database and the search against it (kernels:
// kg_searchdb.hpp; the file form: kg_searchdb_file.hpp).  The build is search_pairs of kg_host_search.hpp over the targets alone
// with what it leaves copied into the handle; a search is search_pairs over the queries alone, then search_candidates /
// search_candidates_ungapped and search_finish as they are, with searchdb_runs in search_runs' place (the probe where that has
// the split of a run at n_db) and searchdb_join launching the two-source join kernels.
// Sequence addressing: one device allocation holds the targets' residues with room for a query batch behind them, and one the
// offsets of the targets with the call's queries' behind them, so align_run, the trace and the ungapped scorer address both
// proteins of a pair through one base pointer and one offsets array, unchanged.
// The handle owns a context as kg_table is one; its blocks stay live in the context's cache, so the live bytes of the cache
// between calls are the handle's.
// Part of kmerguts_hip.hip's translation unit: a batch stage behind kg_host_search.hpp.
#pragma once

#include "kg_searchdb_file.hpp"

struct kg_searchdb {
    kg_table *t = nullptr;              // the handle's context (owned)
    int64_t n_db = 0, residues = 0, room = 0, longest = 0;
    int64_t off_room = 0;               // queries whose offsets fit behind the targets'
    uint64_t P = 0, K = 0, valid = 0;
    uint8_t *d_seq = nullptr;           // residues + room bytes
    int64_t *d_off = nullptr;           // n_db + 1 + off_room
    uint64_t *pk = nullptr, *dk = nullptr;
    uint32_t *pv = nullptr, *kstart = nullptr;
    std::vector<int64_t> h_off;         // the targets' offsets from 0; a search appends its queries' for the time of the call
    bool has_seeds = false, has_mask = false;
    kg_seed_params seeds = {};
    kg_mask_params maskp = {};
    SeedPlan plan = {};
    MaskPlan mplan = {};
    kg_mask_stats mst = {};
    std::vector<uint8_t> names;
    float ms_upload = 0, ms_encode = 0, ms_sort = 0, ms_index = 0, ms_total = 0;
    bool masked_known = false;          // the runs longer than masked_for: counted once per value of max_db_per_kmer
    uint32_t masked_for = 0;
    uint64_t masked = 0;
};

static_assert(sizeof(kg_searchdb_desc) == 240 && sizeof(kg_search_db_stats) == 24, "record layouts of include/kmerguts_hip.h");
static_assert(kgfile::kHeaderBytes == KG_SEARCHDB_HEADER_BYTES && kgfile::kVersion == KG_SEARCHDB_VERSION &&
              kgfile::kAtSeeds + sizeof(kg_seed_params) == kgfile::kAtMask && kgfile::kAtMask + sizeof(kg_mask_params) == kgfile::kAtMaskStats &&
              kgfile::kAtMaskStats + sizeof(kg_mask_stats) == kgfile::kAtSections && kgfile::kAtSections + 24 * kgfile::kSections == kgfile::kAtChecksum,
              "the file layout of include/kmerguts_hip.h");

namespace {

constexpr const char *kSearchDbBusy = "another call is in flight on this kg_searchdb";
constexpr int64_t kSearchDbOffRoom = 1024;

// search_runs against a resident index: the queries' k-mer runs, the probe, whether the join fits, the listed runs
int searchdb_runs(SearchCall &c, const SearchPairs &in, bool keep_pv, uint64_t bytes_per_pair, SearchCands *out, SearchRuns *runs)
{
    const SearchArgs &a = c.a;
    SearchDbSide &res = *a.res;
    kg_table *t = c.t;
    Scratch &sc = c.sc;
    hipStream_t s = t->stream;
    uint64_t *d_tot = c.d_tot;
    const uint32_t qb = bits_for((uint64_t)(a.n_prot - a.n_db));
    const uint64_t P = in.w.P;                          // the queries' pairs
    out->masked = res.masked;
    out->K = res.K;
    if (P == 0) return KG_OK;                           // queries without a window: nothing to join
    uint64_t *const pk = in.w.pk, *const partial = in.w.partial;
    uint64_t K = 0, R = 0;
    int rc;

    // ---- the queries' k-mer runs and the probe (flags / pidx / partial are reused: K <= P <= n) ----
    uint32_t *kh = in.w.flags, *kx = in.w.pidx, *qstart = nullptr, *rd = nullptr, *nd = nullptr, *w = nullptr, *wf = in.w.pv, *wpos = nullptr;
    hipLaunchKernelGGL(kg::search_kmer_heads_kernel, dim3(grid_of(P)), dim3(256), 0, s, pk, P, qb, kh);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, kh, P, kx, partial, d_tot + 1))) return rc;
    HIP_TRY(hipMemcpyAsync(&K, d_tot + 1, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = sc.get(&qstart, K + 1)) || (rc = sc.get(&rd, K)) || (rc = sc.get(&nd, K)) || (rc = sc.get(&w, K)) || (rc = sc.get(&wpos, K))) return rc;
    if (keep_pv && (rc = sc.get(&wf, K))) return rc;
    hipLaunchKernelGGL(kg::cluster_link_starts_kernel, dim3(grid_of(P)), dim3(256), 0, s, kh, kx, P, d_tot + 1, qstart);
    HIP_TRY(hipEventRecord(res.ev_probe[0], s));
    hipLaunchKernelGGL(kg::searchdb_probe_kernel, dim3(grid_of(K)), dim3(256), 0, s, pk, qstart, K, qb, res.dk, res.kstart, (uint32_t)res.K,
                       (uint32_t)a.prm->max_db_per_kmer, rd, nd, w, wf, c.words, res.dwords);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(res.ev_probe[1], s));
    if ((rc = prefix_sum(t, wf, K, wpos, partial, d_tot + 2))) return rc;
    unsigned long long hw[3] = {}, found = 0;
    HIP_TRY(hipMemcpyAsync(hw, c.words, sizeof hw, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&found, res.dwords + kg::kSearchDbFound, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&R, d_tot + 2, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t J = out->J = hw[kg::kSearchJoinPairs];
    out->joined = hw[kg::kSearchJoined];
    res.q_kmers = K;
    res.found = found;
    if (found > K) return fail(KG_ERR_DEVICE, "internal: the probe found more k-mers than the queries have");
    out->K = res.K + K - found;
    if (R != hw[kg::kSearchJoined]) return fail(KG_ERR_DEVICE, "internal: the listed runs and the joined k-mers differ");

    // ---- whether the join fits: J is the 64-bit sum, exact whatever the stored weights saturate to ----
    Cap cap;
    if ((rc = size_cap(a.max_pairs, " (max_pairs)", bytes_per_pair, kSearchPairsMax, &cap))) return rc;
    if (J > cap.items)
        return fail(KG_ERR_LIMIT, kmer_text((int64_t)J) + " join pairs do not fit this call, which holds " + kmer_text((int64_t)cap.items) +
                                      cap.how + "; a smaller max_db_per_kmer masks more of the frequent k-mers");
    if (J == 0) return KG_OK;

    // ---- the runs of weight >= 1, the prefix sum of their weights (J < 2^32: no stored weight is saturated) ----
    uint32_t *cdstart = nullptr, *cqstart = nullptr, *cnd = nullptr, *cw = nullptr, *wx = nullptr;
    uint64_t *jpartial = nullptr;
    if ((rc = sc.get(&cdstart, R)) || (rc = sc.get(&cqstart, R)) || (rc = sc.get(&cnd, R)) || (rc = sc.get(&cw, R + 1)) ||
        (rc = sc.get(&wx, R + 1)) || (rc = sc.get(&jpartial, J / kg::kScanChunk + 3)))
        return rc;
    HIP_TRY(hipMemsetAsync(cw + R, 0, 4, s));
    hipLaunchKernelGGL(kg::searchdb_run_compact_kernel, dim3(grid_of(K)), dim3(256), 0, s, rd, qstart, nd, w, wf, wpos, K, R, cdstart, cqstart,
                       cnd, cw);
    HIP_TRY(hipGetLastError());
    if ((rc = prefix_sum(t, cw, R + 1, wx, partial, d_tot + 3))) return rc;
    *runs = SearchRuns{R, J, cdstart, cnd, wx, jpartial, cqstart};
    return KG_OK;
}

// the join against a resident index (uw: the widths of the ungapped stage's key, or null for the plain join).  The caller
// looks at hipGetLastError behind it, as behind the one-batch launch.
void searchdb_join(SearchCall &c, const SearchPairs &in, const SearchRuns &runs, const UngappedWidths *uw, uint64_t *keys, uint32_t *vals)
{
    const SearchArgs &a = c.a;
    const SearchDbSide &res = *a.res;
    const uint32_t db = bits_for((uint64_t)a.n_db), qb = bits_for((uint64_t)(a.n_prot - a.n_db));
    const dim3 grid(grid_of(runs.J, kg::kSearchTile)), block(kg::kSearchThreads);
    if (uw)
        hipLaunchKernelGGL(kg::searchdb_join_diag_kernel, grid, block, 0, c.t->stream, res.pk, res.pv, in.w.pk, in.w.pv, in.d_off, runs.wx,
                           runs.cstart, runs.cqstart, runs.cnd, (uint32_t)runs.R, (uint32_t)runs.J, (uint32_t)a.n_db, db, qb, uw->gb, uw->bias,
                           keys, vals);
    else
        hipLaunchKernelGGL(kg::searchdb_join_kernel, grid, block, 0, c.t->stream, res.pk, in.w.pk, runs.wx, runs.cstart, runs.cqstart, runs.cnd,
                           (uint32_t)runs.R, (uint32_t)runs.J, db, qb, keys, vals);
}

// a block of the handle: live in the context's cache for the handle's lifetime, never 0 bytes
template <typename T>
int searchdb_block(kg_table *t, T **p, uint64_t count)
{
    return dalloc(t, (void **)p, std::max<uint64_t>(count, 1) * sizeof(T));
}

// the handle's sequence and offsets blocks for n_db targets of `residues` residues: room behind both
int searchdb_rooms(kg_searchdb *db, int64_t query_room)
{
    int rc;
    db->room = query_room ? query_room : KG_SEARCHDB_DEFAULT_ROOM;
    db->off_room = kSearchDbOffRoom;
    if ((rc = searchdb_block(db->t, &db->d_seq, (uint64_t)(db->residues + db->room))) ||
        (rc = searchdb_block(db->t, &db->d_off, (uint64_t)(db->n_db + 1 + db->off_room))))
        return rc;
    HIP_TRY(hipMemcpyAsync(db->d_off, db->h_off.data(), ((size_t)db->n_db + 1) * 8, hipMemcpyHostToDevice, db->t->stream));
    return KG_OK;
}

// dk from pk and kstart; the longest target.  The stream is idle when it returns.
int searchdb_finish(kg_searchdb *db)
{
    kg_table *t = db->t;
    int rc;
    if ((rc = searchdb_block(t, &db->dk, db->K))) return rc;
    if (db->K) {
        hipLaunchKernelGGL(kg::searchdb_kmers_kernel, dim3(grid_of(db->K)), dim3(256), 0, t->stream, db->pk, db->kstart, db->K,
                           bits_for((uint64_t)db->n_db), db->dk);
        HIP_TRY(hipGetLastError());
    }
    db->longest = 0;
    for (int64_t p = 0; p < db->n_db; p++) db->longest = std::max(db->longest, db->h_off[(size_t)p + 1] - db->h_off[(size_t)p]);
    HIP_TRY(hipStreamSynchronize(t->stream));
    return KG_OK;
}

int searchdb_build_impl(kg_searchdb *db, const uint8_t *h_seq, const uint8_t *d_seq_in, const int64_t *offsets, int64_t max_windows,
                        int64_t query_room)
{
    kg_table *t = db->t;
    hipStream_t s = t->stream;
    const int64_t n_db = db->n_db;
    int rc;
    Events<8> ev;
    Events<3> bev;
    if ((rc = ev.create()) || (rc = bev.create())) return rc;
    HIP_TRY(hipEventRecord(bev[0], s));
    if ((rc = searchdb_rooms(db, query_room))) return rc;
    if (db->residues) {
        if (h_seq) {
            if ((rc = upload_pinned(t, h_seq + offsets[0], (size_t)db->residues, db->d_seq))) return rc;
        } else {
            HIP_TRY(hipMemcpyAsync(db->d_seq, d_seq_in + offsets[0], (size_t)db->residues, hipMemcpyDeviceToDevice, s));
        }
    }
    HIP_TRY(hipEventRecord(bev[1], s));
    HIP_TRY(hipEventRecord(ev[0], s));
    {
        Scratch sc(t);
        const kg_search_params none = {};
        const SearchArgs a{&none, nullptr, nullptr, nullptr, db->h_off.data(), n_db, n_db, max_windows, 0, {}, db->has_seeds ? &db->plan : nullptr,
                           nullptr, 0};
        SearchCall c{a, t, sc, ev};
        c.d_seq = c.d_seed = db->d_seq;
        if ((rc = sc.get(&c.d_tot, 8))) return rc;
        if (db->has_mask && (rc = mask_seeding_copy(t, sc, db->mplan, db->d_seq, db->h_off.data(), 0, n_db, (uint64_t)db->residues, &c.d_seed, &db->mst)))
            return rc;
        for (int k = 1; k <= 4; k++) HIP_TRY(hipEventRecord(ev[k], s));
        SearchPairs pairs;
        if ((rc = search_pairs(c, &pairs))) return rc;
        db->valid = pairs.n;
        db->P = pairs.w.P;
        // ---- the k-mer runs of the targets' pairs, and the pairs, their values and the run starts into the handle ----
        const uint32_t b = bits_for((uint64_t)n_db);
        if (db->P) {
            hipLaunchKernelGGL(kg::search_kmer_heads_kernel, dim3(grid_of(db->P)), dim3(256), 0, s, pairs.w.pk, db->P, b, pairs.w.flags);
            HIP_TRY(hipGetLastError());
            if ((rc = prefix_sum(t, pairs.w.flags, db->P, pairs.w.pidx, pairs.w.partial, c.d_tot + 1))) return rc;
            HIP_TRY(hipMemcpyAsync(&db->K, c.d_tot + 1, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        if ((rc = searchdb_block(t, &db->pk, db->P)) || (rc = searchdb_block(t, &db->pv, db->P)) || (rc = searchdb_block(t, &db->kstart, db->K + 1)))
            return rc;
        if (db->P) {
            hipLaunchKernelGGL(kg::cluster_link_starts_kernel, dim3(grid_of(db->P)), dim3(256), 0, s, pairs.w.flags, pairs.w.pidx, db->P,
                               c.d_tot + 1, db->kstart);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(db->pk, pairs.w.pk, db->P * 8, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(db->pv, pairs.w.pv, db->P * 4, hipMemcpyDeviceToDevice, s));
        } else {
            HIP_TRY(hipMemsetAsync(db->kstart, 0, 4, s));
        }
        if ((rc = searchdb_finish(db))) return rc;
        HIP_TRY(hipEventRecord(bev[2], s));
        HIP_TRY(hipStreamSynchronize(s));
        db->ms_upload = bev.ms(0, 1);
        db->ms_encode = pairs.ms_count + ev.ms(1, 2);
        db->ms_sort = ev.ms(2, 3);
        db->ms_total = bev.ms(0, 2);
        db->ms_index = std::max(db->ms_total - db->ms_upload - db->ms_encode - db->ms_sort - db->mst.ms_mask, 0.0f);
    }                                                   // (the scratch is back in the cache: the caller gives it to the driver)
    return KG_OK;
}

// the checks of a build's arguments and what the handle keeps of them on the host
int searchdb_new(const int64_t *offsets, int64_t n_db, const kg_seed_params *seeds, const kg_mask_params *mask, const void *names,
                 int64_t names_bytes, int64_t query_room, std::unique_ptr<kg_searchdb> &db)
{
    db.reset(new (std::nothrow) kg_searchdb());
    if (!db) return fail(KG_ERR_NOMEM, "out of host memory");
    if (seeds) {
        if (int rc = seed_plan(seeds, &db->plan)) return rc;
        db->has_seeds = true;
        db->seeds = *seeds;
    }
    if (mask) {
        if (int rc = mask_plan(mask, &db->mplan)) return rc;
        db->has_mask = true;
        db->maskp = *mask;
    }
    if (names_bytes < 0) return fail(KG_ERR_ARG, "names_bytes must be >= 0");
    if (names_bytes > 0 && !names) return fail(KG_ERR_ARG, "null names");
    if (query_room < 0) return fail(KG_ERR_ARG, "query_room must be >= 0");
    if (n_db < 0) return fail(KG_ERR_ARG, "n_db < 0");
    if (n_db >= (1ll << 29)) return fail(KG_ERR_LIMIT, "2^29 or more proteins in one call");
    if (int rc = check_protein_offsets(offsets, n_db, (int64_t)kg::kAlignMaxLen, "2^24")) return rc;
    db->n_db = n_db;
    db->residues = offsets[n_db] - offsets[0];
    db->h_off.resize((size_t)n_db + 1);
    for (int64_t p = 0; p <= n_db; p++) db->h_off[(size_t)p] = offsets[p] - offsets[0];
    db->names.assign((const uint8_t *)names, (const uint8_t *)names + names_bytes);
    return KG_OK;
}

int searchdb_build_entry(int device, const uint8_t *h_seq, const uint8_t *d_seq, const int64_t *offsets, int64_t n_db,
                         const kg_seed_params *seeds, const kg_mask_params *mask, const void *names, int64_t names_bytes,
                         int64_t max_windows, int64_t query_room, kg_searchdb **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    std::unique_ptr<kg_searchdb> db;
    if (int rc = searchdb_new(offsets, n_db, seeds, mask, names, names_bytes, query_room, db)) return rc;
    if (max_windows < 0) return fail(KG_ERR_ARG, "max_windows must be >= 0");
    if (db->residues && !h_seq && !d_seq) return fail(KG_ERR_ARG, "null sequence");
    CallScope cs(device);               // the handle's context: the handle takes it over when the build has succeeded
    if (cs.rc) return cs.rc;
    db->t = cs.t;
    int rc = d_seq && hipDeviceSynchronize() != hipSuccess ? fail(KG_ERR_DEVICE, "hipDeviceSynchronize failed") : KG_OK;
    if (!rc) rc = searchdb_build_impl(db.get(), h_seq, d_seq, offsets, max_windows, query_room);
    if (rc) return rc;                  // (the context goes, and every block with it)
    cs.t->cache.release_free();         // the scratch goes back to the driver
    cs.disown();
    if (getenv("KG_DEBUG"))
        fprintf(stderr, "[kg] kg_searchdb_build: targets=%lld residues=%lld valid=%lld pairs=%lld kmers=%lld upload_ms=%.3f encode_ms=%.3f sort_ms=%.3f index_ms=%.3f total_ms=%.3f\n",
                (long long)db->n_db, (long long)db->residues, (long long)db->valid, (long long)db->P, (long long)db->K, db->ms_upload,
                db->ms_encode, db->ms_sort, db->ms_index, db->ms_total);
    *out = db.release();
    return KG_OK;
}

// the whole file into memory (KG_ERR_IO)
int searchdb_read_file(const char *path, std::vector<uint8_t> &buf)
{
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(KG_ERR_IO, std::string("cannot open ") + path + ": " + strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); return fail(KG_ERR_IO, std::string(path) + " is not a regular file"); }
    buf.resize((size_t)st.st_size);
    size_t at = 0;
    while (at < buf.size()) {
        const ssize_t got = read(fd, buf.data() + at, std::min<size_t>(buf.size() - at, 1u << 30));
        if (got < 0 && errno == EINTR) continue;
        if (got <= 0) { close(fd); return fail(KG_ERR_IO, std::string("reading ") + path + " failed" + (got < 0 ? std::string(": ") + strerror(errno) : std::string(": the file ended early"))); }
        at += (size_t)got;
    }
    close(fd);
    return KG_OK;
}

// the sections of a checked file image onto the device
int searchdb_open_impl(kg_searchdb *db, const uint8_t *file, const kgfile::Layout &l, int64_t query_room)
{
    kg_table *t = db->t;
    int rc;
    if ((rc = searchdb_rooms(db, query_room)) || (rc = searchdb_block(t, &db->pk, db->P)) || (rc = searchdb_block(t, &db->pv, db->P)) ||
        (rc = searchdb_block(t, &db->kstart, db->K + 1)))
        return rc;
    if (db->residues && (rc = upload_pinned(t, file + l.at[kgfile::kSecResidues], (size_t)db->residues, db->d_seq))) return rc;
    if (db->P && ((rc = upload_pinned(t, file + l.at[kgfile::kSecPairs], (size_t)db->P * 8, (uint8_t *)db->pk)) ||
                  (rc = upload_pinned(t, file + l.at[kgfile::kSecValues], (size_t)db->P * 4, (uint8_t *)db->pv))))
        return rc;
    if ((rc = upload_pinned(t, file + l.at[kgfile::kSecStarts], ((size_t)db->K + 1) * 4, (uint8_t *)db->kstart))) return rc;
    return searchdb_finish(db);
}

// what a search brings beside the handle, checked
struct SearchDbAsk {
    const kg_search_params *prm;
    const kg_align_params *al;
    const uint8_t *h_seq, *d_seq;
    const int64_t *offsets;
    int64_t n_q, max_windows, max_pairs;
    SearchPathsAsk ask;
    const MaskPlan *qmask;
    const kg_ungapped_params *ung;
    const kg_band_params *band;
};

int searchdb_search_impl(kg_searchdb *db, const SearchDbAsk &q, kg_hitset *set)
{
    kg_table *t = db->t;
    hipStream_t s = t->stream;
    const int64_t n_db = db->n_db, n_q = q.n_q, R = db->residues;
    const int64_t Rq = n_q ? q.offsets[n_q] - q.offsets[0] : 0;
    int rc;
    // ---- the queries behind the targets: offsets on the host and on the device, residues on the device ----
    Scratch sc(t);
    // more queries than the offsets' room: the call works on a larger copy of the offsets, which becomes the handle's only when
    // the call has succeeded (a failed call leaves the handle's blocks as they were)
    int64_t *d_off = db->d_off, *grown = nullptr;
    const int64_t want = std::max(n_q, 2 * db->off_room);
    if (n_q > db->off_room) {
        if ((rc = sc.get(&grown, (size_t)(n_db + 1 + want)))) return rc;
        HIP_TRY(hipMemcpy(grown, db->d_off, ((size_t)n_db + 1) * 8, hipMemcpyDeviceToDevice));
        d_off = grown;
    }
    struct Shrink {                     // the handle's host offsets are the targets' again when the call ends
        kg_searchdb *db;
        ~Shrink() { db->h_off.resize((size_t)db->n_db + 1); }
    } shrink{db};
    db->h_off.resize((size_t)(n_db + 1 + n_q));
    std::vector<int64_t> q_off((size_t)n_q + 1, 0);     // the queries' offsets from 0: what their own window pass reads
    for (int64_t k = 1; k <= n_q; k++) {
        q_off[(size_t)k] = q.offsets[k] - q.offsets[0];
        db->h_off[(size_t)(n_db + k)] = R + q_off[(size_t)k];
    }
    Events<8> ev;
    Events<4> dev;
    if ((rc = ev.create()) || (rc = dev.create())) return rc;
    HIP_TRY(hipEventRecord(dev[0], s));
    if (n_q) HIP_TRY(hipMemcpyAsync(d_off + n_db + 1, db->h_off.data() + n_db + 1, (size_t)n_q * 8, hipMemcpyHostToDevice, s));
    if (Rq) {
        if (q.h_seq) {
            if ((rc = upload_pinned(t, q.h_seq + q.offsets[0], (size_t)Rq, db->d_seq + R))) return rc;
        } else {
            HIP_TRY(hipMemcpyAsync(db->d_seq + R, q.d_seq + q.offsets[0], (size_t)Rq, hipMemcpyDeviceToDevice, s));
        }
    }
    HIP_TRY(hipEventRecord(dev[1], s));
    HIP_TRY(hipEventRecord(ev[0], s));

    SearchDbSide res = {};
    res.pk = db->pk; res.dk = db->dk; res.pv = db->pv; res.kstart = db->kstart;
    res.P = db->P; res.K = db->K; res.longest = db->longest;
    res.ev_probe[0] = dev[2]; res.ev_probe[1] = dev[3];
    unsigned long long *words = nullptr;
    uint64_t *d_tot = nullptr;
    if ((rc = sc.get(&words, kg::kSearchWords)) || (rc = sc.get(&d_tot, 8)) || (rc = sc.get(&res.dwords, kg::kSearchDbWords))) return rc;
    HIP_TRY(hipMemsetAsync(words, 0, kg::kSearchWords * 8, s));
    HIP_TRY(hipMemsetAsync(res.dwords, 0, kg::kSearchDbWords * 8, s));
    HIP_TRY(hipEventRecord(dev[2], s));
    HIP_TRY(hipEventRecord(dev[3], s));
    // the targets' runs longer than max_db_per_kmer: counted once per value
    const uint32_t max_db = (uint32_t)q.prm->max_db_per_kmer;
    if (!db->masked_known || db->masked_for != max_db) {
        unsigned long long m = 0;
        if (db->K) {
            hipLaunchKernelGGL(kg::searchdb_masked_kernel, dim3(grid_of(db->K)), dim3(256), 0, s, db->kstart, db->K, max_db, res.dwords);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&m, res.dwords + kg::kSearchDbMasked, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        db->masked = m;
        db->masked_for = max_db;
        db->masked_known = true;
    }
    res.masked = db->masked;

    const SeedPlan *seed = db->has_seeds ? &db->plan : nullptr;
    const SearchArgs a{q.prm, q.al, nullptr, nullptr, db->h_off.data(), n_db + n_q, n_db, q.max_windows, q.max_pairs, q.ask, seed, nullptr, 0,
                       q.ung, q.band, &res};
    SearchCall c{a, t, sc, ev};
    c.d_seq = db->d_seq;
    c.words = words;
    c.d_tot = d_tot;
    UngappedWidths fits;                        // (a call whose diagonals do not fit its join key ends before the window pass)
    if (a.ung && (rc = ungapped_widths(a, &fits))) return rc;

    // ---- the queries' front half: the one-batch call's, over the queries alone ----
    const SearchArgs aq{q.prm, q.al, nullptr, nullptr, q_off.data(), n_q, 0, q.max_windows, q.max_pairs, {}, seed, nullptr, 0};
    SearchCall cq{aq, t, sc, ev};
    cq.d_seq = cq.d_seed = db->d_seq + R;
    cq.words = words;
    cq.d_tot = d_tot;
    kg_mask_stats qmst = {};
    if (q.qmask && (rc = mask_seeding_copy(t, sc, *q.qmask, cq.d_seq, q_off.data(), 0, n_q, (uint64_t)Rq, &cq.d_seed, &qmst))) return rc;
    if (db->has_mask || q.qmask) {
        const kg_mask_stats &d = db->mst;
        kg_mask_stats &m = set->mst;
        if (db->has_mask) m = d;
        if (q.qmask) {
            m.proteins += qmst.proteins; m.residues += qmst.residues; m.windows += qmst.windows; m.low_windows += qmst.low_windows;
            m.ext_windows += qmst.ext_windows; m.masking_windows += qmst.masking_windows; m.segments += qmst.segments;
            m.masked_residues += qmst.masked_residues; m.proteins_masked += qmst.proteins_masked;
        }
        m.ms_mask = qmst.ms_mask;
        set->has_mask = true;
    }
    for (int k = 1; k <= 4; k++) HIP_TRY(hipEventRecord(ev[k], s));
    SearchPairs qp;
    if ((rc = search_pairs(cq, &qp))) return rc;

    // ---- the join against the handle's pairs, and everything behind it as the one-batch call has it ----
    SearchPairs pairs;
    pairs.n = qp.n + db->valid;
    pairs.w = qp.w;
    pairs.d_off = d_off;
    pairs.ms_count = qp.ms_count;
    SearchCands cands;
    if ((rc = a.ung ? search_candidates_ungapped(c, pairs, &cands) : search_candidates(c, pairs, &cands))) return rc;
    if (pairs.n > 0) HIP_TRY(hipEventRecord(ev[4], s));
    pairs.w.P += db->P;
    if ((rc = search_finish(c, pairs, cands, set))) return rc;
    set->dbst.query_kmers = (int64_t)res.q_kmers;
    set->dbst.found = (int64_t)res.found;
    set->dbst.ms_probe = dev.ms(2, 3);
    set->dbst.ms_upload = dev.ms(0, 1);
    set->has_db = true;
    if (grown) {
        HIP_TRY(hipStreamSynchronize(s));               // the old block goes back to the cache: only while the stream is idle
        sc.release(grown);
        dfree(t, db->d_off);
        db->d_off = grown;
        db->off_room = want;
    }
    return KG_OK;
}

// the checks of what a search is asked beside its queries, in the order their words are reported (qplan: the queries' mask plan,
// filled when query_mask is given)
int searchdb_check_ask(const kg_searchdb *db, const kg_search_params *prm, const kg_align_params *al, int64_t max_windows, int64_t max_pairs,
                       const SearchPathsAsk &ask, const kg_mask_params *query_mask, const kg_ungapped_params *ung, const kg_band_params *band,
                       MaskPlan *qplan)
{
    if (!db) return fail(KG_ERR_ARG, "null kg_searchdb");
    if (!prm) return fail(KG_ERR_ARG, "null kg_search_params");
    if (prm->min_shared < 1) return fail(KG_ERR_ARG, "min_shared must be >= 1");
    if (prm->max_cand < 1 || prm->max_cand > kg::kSearchMaxCand) return fail(KG_ERR_ARG, "max_cand must be in 1..64");
    if (prm->max_db_per_kmer < 1) return fail(KG_ERR_ARG, "max_db_per_kmer must be >= 1");
    if (prm->reserved != 0) return fail(KG_ERR_ARG, "kg_search_params.reserved must be 0");
    if (query_mask)
        if (int rc = mask_plan(query_mask, qplan)) return rc;
    if (band && !ung) return fail(KG_ERR_ARG, "null kg_ungapped_params");
    if (ung) {
        if (ung->min_ungapped < 0) return fail(KG_ERR_ARG, "min_ungapped must be >= 0");
        if (ung->reserved[0] != 0 || ung->reserved[1] != 0 || ung->reserved[2] != 0) return fail(KG_ERR_ARG, "kg_ungapped_params.reserved must be 0");
    }
    if (band)
        if (int rc = band_check_params(band)) return rc;
    if (!al) return fail(KG_ERR_ARG, "null kg_align_params");
    if (int rc = align_check_params(al)) return rc;
    if (max_windows < 0) return fail(KG_ERR_ARG, "max_windows must be >= 0");
    if (max_pairs < 0) return fail(KG_ERR_ARG, "max_pairs must be >= 0");
    if (ask.trace && (ask.trace & 3) != KG_TRACE_HITS && (ask.trace & 3) != KG_TRACE_ALL)
        return fail(KG_ERR_ARG, "trace must be KG_TRACE_HITS or KG_TRACE_ALL");
    if (ask.trace && ((ask.trace & ~15) || (ask.trace & (KG_TRACE_OPS | KG_TRACE_OPS_EQX)) == (KG_TRACE_OPS | KG_TRACE_OPS_EQX)))
        return fail(KG_ERR_ARG, "trace takes at most one of KG_TRACE_OPS and KG_TRACE_OPS_EQX beside its mode, and no bit above 15");
    if (ask.trace && ask.max_trace_cells < 1) return fail(KG_ERR_ARG, "max_trace_cells must be >= 1");
    return KG_OK;
}

int searchdb_search_entry(kg_searchdb *db, const kg_search_params *prm, const kg_align_params *al, const uint8_t *h_seq, const uint8_t *d_seq,
                          const int64_t *offsets, int64_t n_q, int64_t max_windows, int64_t max_pairs, int trace, int64_t max_trace_cells,
                          const kg_mask_params *query_mask, const kg_ungapped_params *ung, const kg_band_params *band, kg_hitset **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    const SearchPathsAsk ask{trace, max_trace_cells};
    MaskPlan qplan;
    if (int rc = searchdb_check_ask(db, prm, al, max_windows, max_pairs, ask, query_mask, ung, band, &qplan)) return rc;
    if (n_q < 0) return fail(KG_ERR_ARG, "n_q < 0");
    if (db->n_db + n_q >= (1ll << 29)) return fail(KG_ERR_LIMIT, "2^29 or more proteins in one call");
    if (int rc = check_protein_offsets(offsets, n_q, (int64_t)kg::kAlignMaxLen, "2^24")) return rc;
    const int64_t Rq = n_q ? offsets[n_q] - offsets[0] : 0;
    if (Rq && !h_seq && !d_seq) return fail(KG_ERR_ARG, "null sequence");
    CallScope cs(db->t, kSearchDbBusy);
    if (cs.rc) return cs.rc;
    // test hook: a second call on the handle while this one holds it, whose answer (KG_ERR_BUSY) is this call's
    if (test_hook("KG_TEST_SEARCHDB_REENTER")) return kg_searchdb_reserve(db, db->room);
    if (Rq > db->room)
        return fail(KG_ERR_LIMIT, kmer_text(Rq) + " residues of queries do not fit the room of " + kmer_text(db->room) +
                                      " residues; kg_searchdb_reserve regrows it");
    kg_hitset *set = new (std::nothrow) kg_hitset();
    if (!set) return fail(KG_ERR_NOMEM, "out of host memory");
    set->device = db->t->device;
    int rc = d_seq && hipDeviceSynchronize() != hipSuccess ? fail(KG_ERR_DEVICE, "hipDeviceSynchronize failed") : KG_OK;
    if (!rc) rc = searchdb_search_impl(db, SearchDbAsk{prm, al, h_seq, d_seq, offsets, n_q, max_windows, max_pairs, ask, query_mask ? &qplan : nullptr, ung, band}, set);
    cs.t->cache.release_free();                         // the scratch goes back to the driver, the handle's blocks stay
    if (rc) { std::string keep = g_err; kg_hitset_free(set); g_err = keep; return rc; }
    *out = set;
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_searchdb_build(int device, const uint8_t *seq, const int64_t *offsets, int64_t n_db, const kg_seed_params *seeds,
                      const kg_mask_params *mask, const void *names, int64_t names_bytes, int64_t max_windows, int64_t query_room,
                      kg_searchdb **out)
{
    return searchdb_build_entry(device, seq, nullptr, offsets, n_db, seeds, mask, names, names_bytes, max_windows, query_room, out);
}

int kg_searchdb_build_device(int device, const uint8_t *d_seq, const int64_t *offsets, int64_t n_db, const kg_seed_params *seeds,
                             const kg_mask_params *mask, const void *names, int64_t names_bytes, int64_t max_windows, int64_t query_room,
                             kg_searchdb **out)
{
    return searchdb_build_entry(device, nullptr, d_seq, offsets, n_db, seeds, mask, names, names_bytes, max_windows, query_room, out);
}

int kg_searchdb_open(int device, const char *path, int64_t query_room, kg_searchdb **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!path) return fail(KG_ERR_ARG, "null argument");
    if (query_room < 0) return fail(KG_ERR_ARG, "query_room must be >= 0");
    std::vector<uint8_t> buf;
    if (int rc = searchdb_read_file(path, buf)) return rc;
    kgfile::Layout l;
    const bool verify = test_hook("KG_SEARCHDB_NO_VERIFY") == 0;
    const std::string wrong = kgfile::searchdb_file_check(buf.data(), buf.size(), verify, &l);
    if (!wrong.empty()) return fail(KG_ERR_FORMAT, wrong);
    const uint8_t *file = buf.data();
    kg_seed_params seeds;
    kg_mask_params mask;
    memcpy(&seeds, file + kgfile::kAtSeeds, sizeof seeds);
    memcpy(&mask, file + kgfile::kAtMask, sizeof mask);
    std::vector<int64_t> offsets((size_t)l.n_db + 1);
    memcpy(offsets.data(), file + l.at[kgfile::kSecOffsets], offsets.size() * 8);
    std::unique_ptr<kg_searchdb> db;
    if (searchdb_new(offsets.data(), l.n_db, l.has_seeds ? &seeds : nullptr, l.has_mask ? &mask : nullptr, file + l.at[kgfile::kSecNames],
                     l.names_bytes, query_room, db))
        return fail(KG_ERR_FORMAT, "the header's parameters: " + g_err);
    if (l.has_mask) {
        memcpy(&db->mst, file + kgfile::kAtMaskStats, sizeof db->mst);
        db->mst.ms_mask = 0;
    }
    db->P = (uint64_t)l.pairs;
    db->K = (uint64_t)l.kmers;
    db->valid = (uint64_t)l.windows;
    CallScope cs(device);               // the handle's context: the handle takes it over when the upload has succeeded
    if (cs.rc) return cs.rc;
    db->t = cs.t;
    if (int rc = searchdb_open_impl(db.get(), file, l, query_room)) return rc;
    cs.t->cache.release_free();
    cs.disown();
    *out = db.release();
    return KG_OK;
}

int kg_searchdb_save(kg_searchdb *db, const char *path)
{
    if (!db || !path) return fail(KG_ERR_ARG, "null argument");
    CallScope cs(db->t, kSearchDbBusy);
    if (cs.rc) return cs.rc;
    kgfile::Layout l;
    l.n_db = db->n_db; l.residues = db->residues; l.pairs = (int64_t)db->P; l.kmers = (int64_t)db->K; l.windows = (int64_t)db->valid;
    l.names_bytes = (int64_t)db->names.size();
    kgfile::lay_out(l);
    // written under a temporary name next to the target and renamed at the end: a failed save leaves no file under `path`
    std::string tmp = std::string(path) + ".tmpXXXXXX";
    const int fd = mkstemp(&tmp[0]);
    if (fd < 0) return fail(KG_ERR_IO, std::string("cannot create a file next to ") + path + ": " + strerror(errno));
    const mode_t um = umask(0);
    umask(um);
    (void)fchmod(fd, 0666 & ~um);
    std::string why;
    bool ok = true;
    std::vector<uint8_t> buf;
    const void *src[kgfile::kSections] = {db->h_off.data(), db->d_seq, db->pk, db->pv, db->kstart, db->names.data()};
    // one section at a time through host memory: its checksum, its bytes and the zeros up to the next multiple of 64
    for (int k = 0; ok && k < kgfile::kSections; k++) {
        const uint64_t padded = (k + 1 < kgfile::kSections ? l.at[k + 1] : l.file_bytes) - l.at[k];
        buf.assign((size_t)padded, 0);
        if (l.bytes[k]) {
            const bool host = k == kgfile::kSecOffsets || k == kgfile::kSecNames;
            if (host) memcpy(buf.data(), src[k], (size_t)l.bytes[k]);
            else if (hipMemcpy(buf.data(), src[k], (size_t)l.bytes[k], hipMemcpyDeviceToHost) != hipSuccess) { ok = false; why = "device-to-host copy failed"; break; }
        }
        l.sum[k] = kgfile::checksum(buf.data(), l.bytes[k]);
        if (lseek(fd, (off_t)l.at[k], SEEK_SET) < 0 || !write_all(fd, nullptr, buf.data(), buf.size())) { ok = false; why = strerror(errno); }
    }
    uint8_t hdr[kgfile::kHeaderBytes] = {};
    memcpy(hdr, kgfile::kMagic, 8);
    kgfile::wr32(hdr + kgfile::kAtVersion, kgfile::kVersion);
    kgfile::wr32(hdr + kgfile::kAtHeaderBytes, (uint32_t)kgfile::kHeaderBytes);
    kgfile::wr64(hdr + kgfile::kAtTargets, (uint64_t)l.n_db);
    kgfile::wr64(hdr + kgfile::kAtResidues, (uint64_t)l.residues);
    kgfile::wr64(hdr + kgfile::kAtPairs, (uint64_t)l.pairs);
    kgfile::wr64(hdr + kgfile::kAtKmers, (uint64_t)l.kmers);
    kgfile::wr64(hdr + kgfile::kAtWindows, (uint64_t)l.windows);
    kgfile::wr64(hdr + kgfile::kAtNamesBytes, (uint64_t)l.names_bytes);
    kgfile::wr32(hdr + kgfile::kAtHasSeeds, db->has_seeds ? 1u : 0u);
    kgfile::wr32(hdr + kgfile::kAtHasMask, db->has_mask ? 1u : 0u);
    if (db->has_seeds) memcpy(hdr + kgfile::kAtSeeds, &db->seeds, sizeof db->seeds);
    if (db->has_mask) {
        kg_mask_stats m = db->mst;
        m.ms_mask = 0;
        m.reserved = 0;
        memcpy(hdr + kgfile::kAtMask, &db->maskp, sizeof db->maskp);
        memcpy(hdr + kgfile::kAtMaskStats, &m, sizeof m);
    }
    for (int k = 0; k < kgfile::kSections; k++) {
        uint8_t *e = hdr + kgfile::kAtSections + 24 * k;
        kgfile::wr64(e, l.at[k]);
        kgfile::wr64(e + 8, l.bytes[k]);
        kgfile::wr64(e + 16, l.sum[k]);
    }
    kgfile::wr64(hdr + kgfile::kAtChecksum, kgfile::checksum(hdr, kgfile::kChecked));
    if (ok && (lseek(fd, 0, SEEK_SET) < 0 || !write_all(fd, nullptr, hdr, sizeof hdr))) { ok = false; why = strerror(errno); }
    if (close(fd) != 0 && ok) { ok = false; why = strerror(errno); }
    if (ok && rename(tmp.c_str(), path) != 0) { ok = false; why = std::string("rename: ") + strerror(errno); }
    if (!ok) {
        (void)unlink(tmp.c_str());
        return fail(KG_ERR_IO, std::string("writing ") + path + " failed" + (why.empty() ? std::string() : ": " + why));
    }
    return KG_OK;
}

int kg_searchdb_info(const kg_searchdb *db, kg_searchdb_desc *out)
{
    if (!db || !out) return fail(KG_ERR_ARG, "null argument");
    kg_searchdb_desc i = {};
    i.targets = db->n_db;
    i.residues = db->residues;
    i.pairs = (int64_t)db->P;
    i.kmers = (int64_t)db->K;
    i.valid_windows = (int64_t)db->valid;
    i.names_bytes = (int64_t)db->names.size();
    i.query_room = db->room;
    i.device_bytes = (int64_t)db->t->cache.live_bytes();
    i.has_seeds = db->has_seeds;
    i.has_mask = db->has_mask;
    i.seeds = db->seeds;
    i.mask = db->maskp;
    i.mask_stats = db->mst;
    i.ms_upload = db->ms_upload;
    i.ms_encode = db->ms_encode;
    i.ms_sort = db->ms_sort;
    i.ms_index = db->ms_index;
    i.ms_total = db->ms_total;
    *out = i;
    return KG_OK;
}

int kg_searchdb_names_copy(const kg_searchdb *db, void *dst)
{
    if (!db || (!dst && !db->names.empty())) return fail(KG_ERR_ARG, "null argument");
    if (!db->names.empty()) memcpy(dst, db->names.data(), db->names.size());
    return KG_OK;
}

int64_t kg_searchdb_live_device_bytes(kg_searchdb *db) { return db ? (int64_t)db->t->cache.live_bytes() : 0; }

int kg_searchdb_reserve(kg_searchdb *db, int64_t query_room)
{
    if (!db) return fail(KG_ERR_ARG, "null kg_searchdb");
    if (query_room < 0) return fail(KG_ERR_ARG, "query_room must be >= 0");
    CallScope cs(db->t, kSearchDbBusy);
    if (cs.rc) return cs.rc;
    if (query_room <= db->room) return KG_OK;           // (the room never shrinks)
    uint8_t *grown = nullptr;
    if (int rc = searchdb_block(db->t, &grown, (uint64_t)(db->residues + query_room))) return rc;
    if (db->residues) HIP_TRY(hipMemcpy(grown, db->d_seq, (size_t)db->residues, hipMemcpyDeviceToDevice));
    dfree(db->t, db->d_seq);
    db->d_seq = grown;
    db->room = query_room;
    db->t->cache.release_free();
    return KG_OK;
}

void kg_searchdb_free(kg_searchdb *db)
{
    if (!db) return;
    kg_table_close(db->t);              // (its cache frees every block of the handle)
    delete db;
}

int kg_searchdb_search(kg_searchdb *db, const kg_search_params *p, const kg_align_params *align, const uint8_t *seq, const int64_t *offsets,
                       int64_t n_q, int64_t max_windows, int64_t max_pairs, int trace, int64_t max_trace_cells,
                       const kg_mask_params *query_mask, const kg_ungapped_params *ungapped, const kg_band_params *band, kg_hitset **out)
{
    return searchdb_search_entry(db, p, align, seq, nullptr, offsets, n_q, max_windows, max_pairs, trace, max_trace_cells, query_mask, ungapped,
                                 band, out);
}

int kg_searchdb_search_device(kg_searchdb *db, const kg_search_params *p, const kg_align_params *align, const uint8_t *d_seq,
                              const int64_t *offsets, int64_t n_q, int64_t max_windows, int64_t max_pairs, int trace, int64_t max_trace_cells,
                              const kg_mask_params *query_mask, const kg_ungapped_params *ungapped, const kg_band_params *band,
                              kg_hitset **out)
{
    return searchdb_search_entry(db, p, align, nullptr, d_seq, offsets, n_q, max_windows, max_pairs, trace, max_trace_cells, query_mask, ungapped,
                                 band, out);
}

int kg_hitset_db_stats(const kg_hitset *s, kg_search_db_stats *out)
{
    if (s && !s->has_db) return fail(KG_ERR_ARG, "kg_hitset_db_stats: the set was made without a kg_searchdb");
    return copy_stats(s, s ? &s->dbst : nullptr, out);
}

}  // extern "C"
