// kg_host_table.hpp -- a table's whole life: kg_table_open / kg_table_from_memory / kg_table_from_device (the records onto the
// device, then table_finish: tags, byte home index, bit digest, streams and events), kg_table_info, kg_table_save and
// kg_table_close; table_new, the table-less context CallScope makes for the calls that have no table; and the library's
// kg_last_error / kg_version (kernels: kg_device.hpp, build_tags_kernel / build_bidx_kernel / build_hbits_kernel).
// Part of kmerguts_hip.hip's translation unit: the first host file behind kg_host.hpp.
#pragma once

namespace {

int table_finish(kg_table *t)
{
    // tag array + occupancy count: one streaming pass over the records
    HIP_TRY(hipSetDevice(t->device));
    // the records may have been produced on another stream (kg_table_from_device): the library's
    // stream is non-blocking, so wait for everything the device has been given so far
    HIP_TRY(hipDeviceSynchronize());
    unsigned __int128 one = 1;
    if (t->num_sigs == 1) t->magic = ~0ull;
    else t->magic = (uint64_t)((one << 64) / (unsigned __int128)(uint64_t)t->num_sigs);
    t->m35 = (t->num_sigs >= 64 && t->num_sigs < (1ll << 31)) ? (uint32_t)((1ull << 35) / (uint64_t)t->num_sigs) : 0u;
    uint64_t n_tags = t->limit + kg::kTagPad;
    HIP_TRY(hipMalloc((void **)&t->d_tags, n_tags));
    unsigned long long *d_occ = nullptr;
    HIP_TRY(hipMalloc((void **)&d_occ, 16));
    HIP_TRY(hipMemsetAsync(d_occ, 0, 16, t->stream));
    uint64_t want = (n_tags + 255) / 256;
    uint32_t grid = (uint32_t)(want < 256ull * 16 ? (want ? want : 1) : 256ull * 16);
    hipLaunchKernelGGL(kg::build_tags_kernel, dim3(grid), dim3(256), 0, t->stream, t->d_entries, t->limit, n_tags,
                       (uint64_t)t->num_sigs, t->magic, t->d_tags, d_occ);
    HIP_TRY(hipGetLastError());
    // the byte home index: what the tag pass probes instead of the tags, for every table the scatter pass applies to
    // (KG_BIDX=0 switches it off per scan, not here: a table outlives the environment it was opened in)
    t->bidx_exact = (uint64_t)KG_MAX_ENCODED / (uint64_t)t->num_sigs + 1 <= kg::kBidxClasses;
    if (t->m35 != 0 && t->limit > 0) {
        const uint64_t n_bidx = t->limit + kg::kTagPad;
        HIP_TRY(hipMalloc((void **)&t->d_bidx, n_bidx));
        const uint64_t wantb = (n_bidx + 255) / 256;
        hipLaunchKernelGGL(kg::build_bidx_kernel, dim3((uint32_t)std::min<uint64_t>(wantb, 256ull * 32)), dim3(256), 0, t->stream,
                           t->d_entries, t->d_tags, t->limit, n_bidx, (uint64_t)t->num_sigs, t->magic, t->d_bidx);
        HIP_TRY(hipGetLastError());
        // ... and, for tables whose bits stay in an XCD's L2 or close to it, its one-bit-per-slot digest: the direct kernel asks it
        // first (scan_kernel).  2^26 slots = 8 MB of bits: the gather rate there is still twice that of a tag array eight times
        // the size (profiles/r01_gather_ceiling_small_tables.jsonl).
        if (n_bidx <= kHbitsMaxSlots) {
            const uint64_t n_words = (n_bidx + 31) / 32;
            HIP_TRY(hipMalloc((void **)&t->d_hbits, n_words * 4));
            hipLaunchKernelGGL(kg::build_hbits_kernel, dim3((uint32_t)std::min<uint64_t>((n_words + 255) / 256, 256ull * 32)), dim3(256), 0, t->stream,
                               t->d_bidx, n_bidx, t->d_hbits, n_words);
            HIP_TRY(hipGetLastError());
        }
    }
    unsigned long long occ[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(occ, d_occ, 16, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    HIP_TRY(hipFree(d_occ));
    t->occupied = occ[0];
    t->tail_start = occ[1];
    for (auto &e : t->pev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&t->stream2, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&t->stream3, hipStreamNonBlocking));
    return KG_OK;
}

int table_new(int device, kg_table **out)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(KG_ERR_DEVICE, "no HIP device: libkmerguts_hip needs an MI355X (gfx950) GPU; there is no CPU path");
    if (device < 0 || device >= ndev) return fail(KG_ERR_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    kg_table *t = new (std::nothrow) kg_table();
    if (!t) return fail(KG_ERR_NOMEM, "out of host memory");
    t->device = device;
    hipError_t e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc((void **)&t->h_pin, kPinWords * 8);
    for (auto &ev : t->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);               // (a table-less context of kg_aggregate_hits uses them too)
    if (e != hipSuccess) { kg_table_close(t); return fail(KG_ERR_DEVICE, std::string("hipStreamCreate / hipEventCreate: ") + hipGetErrorString(e)); }
    *out = t;
    return KG_OK;
}

int64_t rd_i64le(const uint8_t *b)
{
    uint64_t v = 0;
    for (int i = 7; i >= 0; i--) v = (v << 8) | b[i];
    return (int64_t)v;
}

int parse_header(const uint8_t *hdr, kg_table *t)
{
    // readKmerTableHeader, KGJ:933-935
    t->num_sigs = rd_i64le(hdr);
    t->entry_size = rd_i64le(hdr + 8);
    t->version = rd_i64le(hdr + 16);      // never checked by the reference (KGJ:97 VERSION unused)
    if (t->num_sigs <= 0) return fail(KG_ERR_FORMAT, "kmer table header: numSigs <= 0");
    if (t->entry_size != KG_TABLE_ENTRY_SIZE)
        return fail(KG_ERR_FORMAT, "kmer table header: entrySize != 24 (the reference reads 24-byte records, KGJ:995-999)");
    return KG_OK;
}

// kg_table_save: all of p[n] into the file, plain or gzip
bool write_all(int fd, gzFile g, const uint8_t *p, size_t n)
{
    while (n) {
        const size_t piece = std::min<size_t>(n, 1u << 30);
        long got;
        if (g) got = gzwrite(g, p, (unsigned)piece);
        else got = (long)write(fd, p, piece);
        if (got <= 0) {
            if (!g && got < 0 && errno == EINTR) continue;
            return false;
        }
        p += got;
        n -= (size_t)got;
    }
    return true;
}

}  // namespace

extern "C" {

const char *kg_last_error(void) { return g_err.c_str(); }
const char *kg_version(void) { return "libkmerguts_hip 0.1.0 gfx950"; }

int kg_table_from_memory(const void *image, size_t nbytes, int device, kg_table **out)
{
    if (!image || !out) return fail(KG_ERR_ARG, "null argument");
    if (nbytes < 24) return fail(KG_ERR_FORMAT, "kmer table image shorter than its 24-byte header");
    kg_table *t = nullptr;
    int rc = table_new(device, &t);
    if (rc) return rc;
    rc = parse_header((const uint8_t *)image, t);
    if (rc) { kg_table_close(t); return rc; }
    t->limit = (nbytes - 24) / KG_TABLE_ENTRY_SIZE;       // a trailing partial record is an EOF for the reference
    size_t bytes = (size_t)t->limit * KG_TABLE_ENTRY_SIZE;
    t->own_entries = true;
    hipError_t e = hipMalloc((void **)&t->d_entries, bytes ? bytes : 256);
    if (e != hipSuccess) { kg_table_close(t); return fail(KG_ERR_NOMEM, std::string("hipMalloc(table): ") + hipGetErrorString(e)); }
    if (bytes) {
        e = hipMemcpy(t->d_entries, (const uint8_t *)image + 24, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { kg_table_close(t); return fail(KG_ERR_DEVICE, std::string("hipMemcpy(table): ") + hipGetErrorString(e)); }
    }
    rc = table_finish(t);
    if (rc) { kg_table_close(t); return rc; }
    *out = t;
    return KG_OK;
}

// gzip members are inflated by one zlib stream (a gzip stream has no block index: it cannot be cut for several
// threads); what can overlap does: the inflate of piece k+1 with the upload of piece k, and no host copy of the
// table is ever held (the reference's GZIPInputStream is a stream too, KGJ:749-753, 927-929).
static int open_gz(const char *path, int device, kg_table **out)
{
    gzFile g = gzopen(path, "rb");
    if (!g) return fail(KG_ERR_IO, std::string("cannot open ") + path + ": " + strerror(errno));
    gzbuffer(g, 1u << 20);
    uint8_t hdr[24];
    if (gzread(g, hdr, 24) != 24) { gzclose(g); return fail(KG_ERR_FORMAT, "kmer table file shorter than its 24-byte header"); }
    kg_table *t = nullptr;
    int rc = table_new(device, &t);
    if (rc) { gzclose(g); return rc; }
    rc = parse_header(hdr, t);
    if (rc) { gzclose(g); kg_table_close(t); return rc; }
    // the header says how many records to expect; a stream that holds more keeps being read by the reference, so the
    // device buffer grows when it has to
    size_t cap = (size_t)t->num_sigs * KG_TABLE_ENTRY_SIZE;
    if (cap < 256) cap = 256;
    t->own_entries = true;
    hipError_t e = hipMalloc((void **)&t->d_entries, cap);
    if (e != hipSuccess) { gzclose(g); kg_table_close(t); return fail(KG_ERR_NOMEM, std::string("hipMalloc(table): ") + hipGetErrorString(e)); }
    const size_t CH = 64u << 20;
    uint8_t *pin[2] = {nullptr, nullptr};
    hipEvent_t done[2];
    bool ok = hipHostMalloc((void **)&pin[0], CH) == hipSuccess && hipHostMalloc((void **)&pin[1], CH) == hipSuccess &&
              hipEventCreate(&done[0]) == hipSuccess && hipEventCreate(&done[1]) == hipSuccess;
    size_t at = 0;
    int which = 0;
    bool used[2] = {false, false};
    std::string why;
    while (ok) {
        if (used[which]) ok = hipEventSynchronize(done[which]) == hipSuccess;
        if (!ok) break;
        size_t n = 0;
        while (n < CH) {                                   // gzread takes an unsigned int
            const int got = gzread(g, pin[which] + n, (unsigned)std::min<size_t>(CH - n, 1u << 30));
            if (got < 0) { int en = 0; why = gzerror(g, &en); ok = false; break; }
            if (got == 0) break;
            n += (size_t)got;
        }
        if (!ok || n == 0) break;
        if (at + n > cap) {
            size_t ncap = std::max(at + n, cap + cap / 2);
            uint8_t *bigger = nullptr;
            ok = hipStreamSynchronize(t->stream) == hipSuccess && hipMalloc((void **)&bigger, ncap) == hipSuccess &&
                 hipMemcpy(bigger, t->d_entries, at, hipMemcpyDeviceToDevice) == hipSuccess;
            if (!ok) { if (bigger) (void)hipFree(bigger); why = "out of device memory for a table longer than its header says"; break; }
            (void)hipFree(t->d_entries);
            t->d_entries = bigger; cap = ncap;
        }
        ok = hipMemcpyAsync(t->d_entries + at, pin[which], n, hipMemcpyHostToDevice, t->stream) == hipSuccess &&
             hipEventRecord(done[which], t->stream) == hipSuccess;
        used[which] = true;
        at += n;
        which ^= 1;
    }
    if (ok) ok = hipStreamSynchronize(t->stream) == hipSuccess;
    gzclose(g);
    if (pin[0]) (void)hipHostFree(pin[0]);
    if (pin[1]) (void)hipHostFree(pin[1]);
    (void)hipEventDestroy(done[0]);
    (void)hipEventDestroy(done[1]);
    if (!ok) { kg_table_close(t); return fail(KG_ERR_IO, "inflating/uploading the kmer table failed" + (why.empty() ? std::string() : ": " + why)); }
    t->limit = at / KG_TABLE_ENTRY_SIZE;                  // a trailing partial record is an EOF for the reference
    rc = table_finish(t);
    if (rc) { kg_table_close(t); return rc; }
    *out = t;
    return KG_OK;
}

int kg_table_open(const char *path, int device, kg_table **out)
{
    if (!path || !out) return fail(KG_ERR_ARG, "null argument");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(KG_ERR_IO, std::string("cannot open ") + path + ": " + strerror(errno));
    uint8_t hdr[24];
    const size_t got_hdr = fread(hdr, 1, 24, f);
    if (got_hdr >= 2 && hdr[0] == 0x1f && hdr[1] == 0x8b) {          // gzip magic: kmer.table.mem_map.gz
        fclose(f);
        return open_gz(path, device, out);
    }
    if (got_hdr != 24) { fclose(f); return fail(KG_ERR_FORMAT, "kmer table file shorter than its 24-byte header"); }
    if (fseeko(f, 0, SEEK_END) != 0) { fclose(f); return fail(KG_ERR_IO, "fseek failed"); }
    off_t fsz = ftello(f);
    fclose(f);
    kg_table *t = nullptr;
    int rc = table_new(device, &t);
    if (rc) return rc;
    rc = parse_header(hdr, t);
    if (rc) { kg_table_close(t); return rc; }
    t->limit = (uint64_t)(fsz - 24) / KG_TABLE_ENTRY_SIZE;
    size_t bytes = (size_t)t->limit * KG_TABLE_ENTRY_SIZE;
    t->own_entries = true;
    hipError_t e = hipMalloc((void **)&t->d_entries, bytes ? bytes : 256);
    if (e != hipSuccess) { kg_table_close(t); return fail(KG_ERR_NOMEM, std::string("hipMalloc(table): ") + hipGetErrorString(e)); }
    // Several reader threads pread() disjoint 32 MiB pieces of the file into their own pinned buffers (two each) and
    // hand them to the copy engine: one thread's read() runs at the page cache's single-core memcpy rate (~5 GB/s),
    // a 33.6 GB table should load at what the PCIe link takes.
    const int fd = open(path, O_RDONLY);
    if (fd < 0) { kg_table_close(t); return fail(KG_ERR_IO, std::string("cannot open ") + path + ": " + strerror(errno)); }
    const size_t CH = 32u << 20;
    const size_t n_pieces = (bytes + CH - 1) / CH;
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t n_thr = std::max<size_t>(1, std::min<size_t>({(size_t)8, (size_t)(hw ? hw : 4), n_pieces}));
    std::atomic<size_t> next{0};
    std::atomic<bool> ok{true};
    std::mutex err_mu;
    std::string why;
    auto worker = [&]() {
        if (hipSetDevice(device) != hipSuccess) { ok = false; return; }
        hipStream_t s = nullptr;
        uint8_t *pin[2] = {nullptr, nullptr};
        hipEvent_t done[2] = {nullptr, nullptr};
        bool good = hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess &&
                    hipHostMalloc((void **)&pin[0], CH) == hipSuccess && hipHostMalloc((void **)&pin[1], CH) == hipSuccess &&
                    hipEventCreate(&done[0]) == hipSuccess && hipEventCreate(&done[1]) == hipSuccess;
        bool used[2] = {false, false};
        int which = 0;
        while (good && ok.load()) {
            const size_t k = next.fetch_add(1);
            if (k >= n_pieces) break;
            const size_t at = k * CH, n = std::min(CH, bytes - at);
            if (used[which]) good = hipEventSynchronize(done[which]) == hipSuccess;
            size_t got = 0;
            while (good && got < n) {
                const ssize_t r = pread(fd, pin[which] + got, n - got, (off_t)(24 + at + got));
                if (r <= 0) { std::lock_guard<std::mutex> lk(err_mu); why = "short read on kmer table file"; good = false; break; }
                got += (size_t)r;
            }
            if (!good) break;
            good = hipMemcpyAsync(t->d_entries + at, pin[which], n, hipMemcpyHostToDevice, s) == hipSuccess &&
                   hipEventRecord(done[which], s) == hipSuccess;
            used[which] = true;
            which ^= 1;
        }
        if (s) (void)hipStreamSynchronize(s);
        if (!good) ok = false;
        for (int i = 0; i < 2; i++) { if (pin[i]) (void)hipHostFree(pin[i]); if (done[i]) (void)hipEventDestroy(done[i]); }
        if (s) (void)hipStreamDestroy(s);
    };
    {
        std::vector<std::thread> pool;
        for (size_t i = 1; i < n_thr; i++) pool.emplace_back(worker);
        worker();
        for (auto &th : pool) th.join();
    }
    close(fd);
    if (!ok.load()) { kg_table_close(t); return fail(KG_ERR_IO, "reading/uploading the kmer table failed" + (why.empty() ? std::string() : ": " + why)); }
    rc = table_finish(t);
    if (rc) { kg_table_close(t); return rc; }
    *out = t;
    return KG_OK;
}

int kg_table_from_device(const void *d_entries, int64_t num_sigs, int device, kg_table **out)
{
    if (!d_entries || !out) return fail(KG_ERR_ARG, "null argument");
    if (num_sigs <= 0) return fail(KG_ERR_ARG, "num_sigs <= 0");
    kg_table *t = nullptr;
    int rc = table_new(device, &t);
    if (rc) return rc;
    t->num_sigs = num_sigs;
    t->entry_size = KG_TABLE_ENTRY_SIZE;
    t->version = 1;
    t->limit = (uint64_t)num_sigs;
    t->own_entries = false;
    t->d_entries = (uint8_t *)d_entries;
    rc = table_finish(t);
    if (rc) { kg_table_close(t); return rc; }
    *out = t;
    return KG_OK;
}

int kg_table_info(const kg_table *t, int64_t *num_sigs, int64_t *entry_size, int64_t *version, int64_t *occupied)
{
    if (!t) return fail(KG_ERR_ARG, "null table");
    if (num_sigs) *num_sigs = t->num_sigs;
    if (entry_size) *entry_size = t->entry_size;
    if (version) *version = t->version;
    if (occupied) *occupied = (int64_t)t->occupied;
    return KG_OK;
}

void kg_table_close(kg_table *t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    if (t->own_entries && t->d_entries) (void)hipFree(t->d_entries);
    if (t->d_tags) (void)hipFree(t->d_tags);
    if (t->d_bidx) (void)hipFree(t->d_bidx);
    if (t->d_hbits) (void)hipFree(t->d_hbits);
    if (t->d_cold) (void)hipFree(t->d_cold);
    if (t->d_calls_cold) (void)hipFree(t->d_calls_cold);
    t->cache.release_all();
    t->pins.release_all();
    if (t->h_pin) (void)hipHostFree(t->h_pin);
    for (auto &e : t->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : t->pev)
        if (e) (void)hipEventDestroy(e);
    if (t->stream2) { (void)hipStreamSynchronize(t->stream2); (void)hipStreamDestroy(t->stream2); }
    if (t->stream3) { (void)hipStreamSynchronize(t->stream3); (void)hipStreamDestroy(t->stream3); }
    for (auto &os : t->ostream) if (os) { (void)hipStreamSynchronize(os); (void)hipStreamDestroy(os); }
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
}

int64_t kg_table_live_device_bytes(kg_table *t)
{
    return t ? (int64_t)t->cache.live_bytes() : 0;
}

// ---- a resident table -> kmer.table.mem_map[.gz] ----
const void *kg_table_device_entries(const kg_table *t) { return t ? t->d_entries : nullptr; }
int64_t kg_table_records(const kg_table *t) { return t ? (int64_t)t->limit : 0; }

int kg_table_save(kg_table *t, const char *path)
{
    if (!t || !path) return fail(KG_ERR_ARG, "null argument");
    CallScope cs(t, "a kg_scan* is in flight on this kg_table");
    if (cs.rc) return cs.rc;
    const size_t plen = strlen(path);
    const bool gz = plen >= 3 && strcmp(path + plen - 3, ".gz") == 0;
    // written under a temporary name next to the target and renamed at the end: a failed save leaves no file under `path`
    std::string tmp = std::string(path) + ".tmpXXXXXX";
    const int fd = mkstemp(&tmp[0]);
    if (fd < 0) return fail(KG_ERR_IO, std::string("cannot create a file next to ") + path + ": " + strerror(errno));
    const mode_t um = umask(0);
    umask(um);
    (void)fchmod(fd, 0666 & ~um);
    gzFile g = nullptr;
    bool ok = true;
    std::string why;
    if (gz) {
        g = gzdopen(fd, "wb1");
        if (!g) { ok = false; why = "gzdopen failed"; }
    }
    uint8_t hdr[24];
    const int64_t h3[3] = {t->num_sigs, t->entry_size, t->version};
    for (int f = 0; f < 3; f++)
        for (int b = 0; b < 8; b++) hdr[f * 8 + b] = (uint8_t)((uint64_t)h3[f] >> (8 * b));
    if (ok && !write_all(fd, g, hdr, 24)) { ok = false; why = strerror(errno); }
    // the records come down through two of the table's pinned blocks: piece k + 1 is copied while piece k is written
    const size_t bytes = (size_t)t->limit * KG_TABLE_ENTRY_SIZE, CH = 32u << 20;
    const size_t n_pieces = (bytes + CH - 1) / CH;
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    if (ok && n_pieces) {
        ok = t->pins.get(&pin[0], CH) == hipSuccess && t->pins.get(&pin[1], CH) == hipSuccess &&
             hipEventCreateWithFlags(&done[0], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&done[1], hipEventDisableTiming) == hipSuccess;
        if (!ok) why = "pinned staging allocation failed";
    }
    auto issue = [&](size_t k) {
        const size_t at = k * CH, n = std::min(CH, bytes - at);
        return hipMemcpyAsync(pin[k & 1], t->d_entries + at, n, hipMemcpyDeviceToHost, t->stream) == hipSuccess &&
               hipEventRecord(done[k & 1], t->stream) == hipSuccess;
    };
    if (ok && n_pieces && !issue(0)) { ok = false; why = "device-to-host copy failed"; }
    for (size_t k = 0; ok && k < n_pieces; k++) {
        if (k + 1 < n_pieces && !issue(k + 1)) { ok = false; why = "device-to-host copy failed"; break; }
        if (hipEventSynchronize(done[k & 1]) != hipSuccess) { ok = false; why = "device-to-host copy failed"; break; }
        if (!write_all(fd, g, (const uint8_t *)pin[k & 1], std::min(CH, bytes - k * CH))) { ok = false; why = strerror(errno); }
    }
    (void)hipStreamSynchronize(t->stream);
    for (int i = 0; i < 2; i++) {
        if (pin[i]) t->pins.put(pin[i]);
        if (done[i]) (void)hipEventDestroy(done[i]);
    }
    if (g) {
        if (gzclose(g) != Z_OK && ok) { ok = false; why = "gzip stream could not be completed"; }
    } else if (close(fd) != 0 && ok) {
        ok = false;
        why = strerror(errno);
    }
    if (ok && rename(tmp.c_str(), path) != 0) { ok = false; why = std::string("rename: ") + strerror(errno); }
    if (!ok) {
        (void)unlink(tmp.c_str());
        return fail(KG_ERR_IO, std::string("writing ") + path + " failed" + (why.empty() ? std::string() : ": " + why));
    }
    return KG_OK;
}

}  // extern "C"
