// kg_host.hpp -- what the host side of every stage needs: the error text, the device and pinned block caches, kg_table and
// kg_result with the names of their numbered slots, the environment readers, the per-call scope and scratch, the base of the
// result sets and their getters, and the helpers the stages share (prefix sum, one launch for several clears, radix sort of
// pairs, pinned upload).
// Part of kmerguts_hip.hip's translation unit: the first host file, behind the kernel headers; the hosts of the table, the
// result, the scan and the batch stages (kg_host_*.hpp) follow it.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(KG_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

// Device-memory cache of one table object.  Every scan ends with a stream synchronisation, and
// blocks are handed back only when the stream is idle, so a freed block can be reused by the next
// request without any ordering concern.  Keeps the working set of repeated scans resident in HBM
// (no hipMalloc/hipFree in the steady state).
struct DevCache {
    std::mutex mu;
    std::multimap<size_t, void *> free_;
    std::unordered_map<void *, size_t> live;

    static size_t round_up(size_t b)
    {
        if (b < 256) return 256;
        size_t g = b >= (8u << 20) ? (2u << 20) : 256;       // 2 MiB granules for large blocks
        return (b + g - 1) / g * g;
    }
    hipError_t get(void **p, size_t bytes)
    {
        bytes = round_up(bytes);
        std::lock_guard<std::mutex> lk(mu);
        auto it = free_.lower_bound(bytes);
        if (it != free_.end() && it->first <= bytes + bytes / 2 + (1u << 20)) {
            *p = it->second;
            live[*p] = it->first;
            free_.erase(it);
            return hipSuccess;
        }
        hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) {
            // give cached blocks back to the driver and retry once
            for (auto &kv : free_) (void)hipFree(kv.second);
            free_.clear();
            e = hipMalloc(p, bytes);
            if (e != hipSuccess) return e;
        }
        live[*p] = bytes;
        return hipSuccess;
    }
    void put(void *p)
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it == live.end()) return;
        free_.emplace(it->second, p);
        live.erase(it);
    }
    // hand a live block over to its user for good (kg_table_build: the table's records, freed with hipFree by kg_table_close)
    void detach(void *p)
    {
        std::lock_guard<std::mutex> lk(mu);
        live.erase(p);
    }
    size_t live_bytes()
    {
        std::lock_guard<std::mutex> lk(mu);
        size_t n = 0;
        for (auto &kv : live) n += kv.second;
        return n;
    }
    void release_all()
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &kv : free_) (void)hipFree(kv.second);
        for (auto &kv : live) (void)hipFree(kv.first);
        free_.clear();
        live.clear();
    }
    // the cached blocks back to the driver, the live ones kept (kg_regions_calls: the set keeps its context, not the scratch)
    void release_free()
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &kv : free_) (void)hipFree(kv.second);
        free_.clear();
    }
};

// Pinned host blocks for the result views.  hipHostMalloc / hipHostFree cost ~0.1-0.2 ms for a small block (more than
// a small scan) and ~0.5 s for the 880 MB of hit records of a 1 Gbp batch (page pinning: the copy itself takes 20 ms at
// PCIe rate), so blocks are kept for the next result: up to kKeepTotal bytes, largest dropped first.
struct PinCache {
    std::mutex mu;
    std::multimap<size_t, void *> free_;
    std::unordered_map<void *, size_t> live;
    size_t kept = 0;
    static constexpr size_t kKeepTotal = 6ull << 30;

    hipError_t get(void **p, size_t bytes)
    {
        bytes = bytes < 4096 ? 4096 : (bytes + 4095) / 4096 * 4096;
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = free_.lower_bound(bytes);
            if (it != free_.end() && it->first <= 2 * bytes + (1u << 16)) {
                *p = it->second;
                live[*p] = it->first;
                kept -= it->first;
                free_.erase(it);
                return hipSuccess;
            }
        }
        hipError_t e = hipHostMalloc(p, bytes);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lk(mu);
        live[*p] = bytes;
        return hipSuccess;
    }
    void put(void *p)
    {
        std::vector<void *> drop;
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = live.find(p);
            if (it == live.end()) return;
            const size_t bytes = it->second;
            live.erase(it);
            free_.emplace(bytes, p);
            kept += bytes;
            while (kept > kKeepTotal && !free_.empty()) {          // largest first
                auto big = std::prev(free_.end());
                kept -= big->first;
                drop.push_back(big->second);
                free_.erase(big);
            }
        }
        for (void *d : drop) (void)hipHostFree(d);
    }
    void release_all()
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &kv : free_) (void)hipHostFree(kv.second);
        for (auto &kv : live) (void)hipHostFree(kv.first);
        free_.clear();
        live.clear();
        kept = 0;
    }
};

}  // namespace

constexpr uint64_t kHbitsMaxSlots = 1ull << 26;     // tables up to this many slots get the bit-per-slot digest (8 MB of bits)

// ---- names for the numbered slots a scan uses: events, pinned words, device counter words ----
constexpr uint32_t kMaxChunks = 8;          // chunks of a partitioned scan (KG_PART_CHUNKS)
constexpr uint32_t kMaxOrderStreams = 4;    // KG_ORDER_STREAMS
// kg_table::pev, the edges between the streams of a partitioned scan
enum : int {
    kPevChunk = 0,                      // [+ 2c] chunk c scattered, [+ 2c + 1] chunk c tag-probed
    kPevFork = 16,                      // the attempt's clears are enqueued: stream2 and stream3 start behind them
    kPevJoin2 = 17, kPevJoin3 = 18,     // everything of the attempt on stream2 / stream3
    kPevTotals = 19,                    // the early totals are in their pinned words
    kPevVerified = 20,                  // [+ c] chunk c verified
    kPevBase = 32,                      // [+ c] ordering streams: chunk c's total is known (the base of chunk c + 1 follows)
    kPevOrdered = 40,                   // [+ k] everything of the attempt on ordering stream k
    kPevCount = 48
};
static_assert(kPevChunk + 2 * kMaxChunks <= kPevFork && kPevVerified + kMaxChunks <= kPevBase && kPevBase + kMaxChunks <= kPevOrdered &&
              kPevOrdered + kMaxOrderStreams <= kPevCount, "event slots overlap");
// kg_table::ev, the timing events of a scan (outside a scan they are free to any call that holds the table)
enum : int { kEvBegin = 0, kEvScanBegin = 1, kEvScanEnd = 2, kEvOrderEnd = 3, kEvAggEnd = 4, kEvScattered = 5 /* all chunks */, kEvSpare = 6,
             kEvJoined = 7 /* stream2 and stream3 joined */, kEvCount = 8, kEvStageBegin = kEvBegin, kEvStageEnd = kEvScanBegin };
// d_totals, the counter words of a scan
enum : int { kTotHits = 0, kTotCursor = 1 /* staging records asked for */, kTotValid = 2, kTotSlots = 3 /* windows / slots counted */,
             kTotCalls = 4, kTotRanOff = 5 /* a lookup ran off the stream (sticky) */, kTotPieces = 6, kTotVoters = 7, kTotWords = 8,
             kTotSent = 6 /* the first words: what the host reads back per attempt */ };
// d_pc, the per-chunk words of a partitioned scan; [kPcBase + n_chunks] = all hits
enum : int { kPcUcur = 0 /* [+ c] hit-list cursors */, kPcCcur = 8 /* candidate cursors */, kPcBase = 16 /* first hit record */,
             kPcCtot = 32 /* hit totals */, kPcWords = 48 };
static_assert(kPcUcur + kMaxChunks <= kPcCcur && kPcCcur + kMaxChunks <= kPcBase && kPcBase + kMaxChunks + 1 <= kPcCtot &&
              kPcCtot + kMaxChunks <= kPcWords, "per-chunk words overlap");
// d_ovfc, 32-bit words per chunk
enum : int { kOvfGroups = 0 /* overflow groups */, kOvfLowc = 1 /* low-complexity blocks set aside */, kOvfGuard = 2 /* spin guard fired */,
             kOvfWords = 8 };
// kg_table::h_pin, pinned host words for the few counters a call reads back (a hipMemcpyAsync to pageable memory blocks the
// host per copy; to pinned memory it does not)
enum : int { kPinPc = 0 /* d_pc */, kPinOvf = 48 /* d_ovfc */, kPinTotals = 80 /* d_totals[0 .. kTotSent) */, kPinCalls = 88 /* CALL total */,
             kPinPieces = 89, kPinWords = 96,
             // the stage area lies over the scan's totals: any call that holds the table and runs no scan may use it.  A stage
             // static_asserts the words it needs against kPinStageWords, beside its own word enums.
             kPinStage = 80, kPinStageWords = kPinWords - kPinStage,
             kPinAssign = 90 /* inside the stage area: long proteins, their CALLs, then the error words */ };
static_assert(kPinPc + kPcWords <= kPinOvf && kOvfWords * kMaxChunks * 4 <= (kPinTotals - kPinOvf) * 8 && kPinTotals + kTotSent <= kPinCalls,
              "counters must fit their pinned words");
static_assert(kPinAssign >= kPinStage && kPinAssign + 2 + 3 <= kPinWords, "stage words must fit their pinned words");

struct kg_table {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;      // partitioned scan: tag pass of chunk c while chunk c+1 is scattered (stream)
    hipStream_t stream3 = nullptr;      // ... and while chunk c-1 is verified and placed
    hipStream_t ostream[kMaxOrderStreams] = {};   // ordering streams (KG_ORDER_STREAMS), lowest priority: queues of their own
    hipEvent_t pev[kPevCount] = {};     // kPev*
    bool own_entries = false;
    uint8_t *d_entries = nullptr;
    uint8_t *d_tags = nullptr;
    uint8_t *d_bidx = nullptr;          // byte home index (kg_device.hpp, build_bidx_kernel): 1 byte per slot, limit + 64 bytes
    bool bidx_exact = false;            // every quotient < 19: its classes are quotients
    uint32_t *d_hbits = nullptr;        // one bit per slot: the byte above is not 0 (tables of at most kHbitsMaxSlots slots: the direct kernel's prefilter)
    uint64_t tail_start = 0;            // first slot of the occupied run that ends at the end of the record stream
    int64_t num_sigs = 0, entry_size = 0, version = 0;
    uint64_t limit = 0;          // complete 24-byte records present
    uint64_t magic = 0;          // floor(2^64 / num_sigs)
    uint32_t m35 = 0;            // floor(2^35 / num_sigs) when 64 <= num_sigs < 2^31 (kg::split_fast), else 0
    uint64_t occupied = 0;
    double stage_ratio = 1.0 / 16;   // staging records per window, grown to the high-water mark
    size_t scatter_lds[2][3] = {};   // dynamic LDS the scatter kernel (DNA / protein; plain / short stream / + progress) has been allowed so far
    kg::ScatterCold *d_cold = nullptr;          // the scatter pass's cold-path parameter blocks, one per chunk (kg_partition.hpp) ...
    kg::ScatterCold h_cold[kMaxChunks] = {};    // ... and what they hold: uploaded again only when a scan's blocks differ
    kg::CallsCold *d_calls_cold = nullptr;      // the same for the CALL pass (kg_aggregate.hpp)
    kg::CallsCold h_calls_cold = {};
    size_t hist_lds = 48 * 1024;     // ... and the hit histogram kernel (kg_order.hpp)
    size_t place_lds[2] = {48 * 1024, 48 * 1024};   // ... and group_place_kernel<DNA / AA>
    hipEvent_t ev[kEvCount] = {};       // kEv*
    uint64_t *h_pin = nullptr;          // kPin*
    std::atomic<int> busy{0};    // a kg_scan* is in flight on this table (its streams, events and pinned words are per table)
    uint32_t fail_alloc_at = 0, alloc_count = 0;   // test hook KG_TEST_FAIL_ALLOC (include/kmerguts_hip.h)
    DevCache cache;
    PinCache pins;
};

struct kg_result {
    kg_table *tab = nullptr;
    bool own_tab = false;        // kg_aggregate_hits: the result owns a table-less context (stream + block caches)
    kg_stats st = {};
    uint32_t per = 6;
    // device
    kg_hit *d_hits = nullptr;
    int64_t *d_chs = nullptr;
    kg_call *d_calls = nullptr;
    int64_t *d_ccs = nullptr;
    kg_otu *d_otu = nullptr;
    uint8_t *d_ev = nullptr, *d_tail_ev = nullptr;   // KG_EV_* per hit / per container
    uint32_t *d_hit_slots = nullptr;                 // KG_F_PROGRESS: the slot every hit was found at
    bool has_progress = false;
    kg_progress progress = {};
    // host copies (lazy), in pinned memory so the copy runs at PCIe rate
    void *h_hits = nullptr, *h_chs = nullptr, *h_ccs = nullptr, *h_calls = nullptr, *h_otu = nullptr, *h_ev = nullptr,
         *h_tail_ev = nullptr, *h_hit_slots = nullptr;
};

namespace {

uint32_t env_u32(const char *name, uint32_t dflt)
{
    const char *v = getenv(name);
    if (!v || !*v) return dflt;
    char *end = nullptr;
    long x = strtol(v, &end, 10);
    return (end != v && x >= 0) ? (uint32_t)x : dflt;
}

constexpr uint32_t kMaxGrid = 256u * 32u;      // the most workgroups a geometry knob asks for (the defaults: 256 .. 2048)

// A geometry knob (tuning aid): env_u32 held to [lo, hi], the range its kernels run with, and rounded up to a multiple of
// `mult` (ticketed grids: one hand-out counter per eight workgroups).  0, a value below lo or one beyond 2^32 become a
// legal geometry instead of an empty launch, a division by zero or a wrapped shift.
uint32_t env_knob(const char *name, uint32_t dflt, uint32_t lo, uint32_t hi, uint32_t mult = 1)
{
    uint32_t x = dflt;
    if (const char *v = getenv(name); v && *v) {
        char *end = nullptr;
        const long long y = strtoll(v, &end, 10);
        if (end != v && y >= 0) x = y > (long long)hi ? hi : (uint32_t)y;
    }
    x = std::min(hi, std::max(lo, x));
    return (x + mult - 1) / mult * mult;
}

// The two test hooks (KG_TEST_TINY_LISTS, KG_TEST_FAIL_ALLOC; include/kmerguts_hip.h) are read only when the process opted in
// with KG_ENABLE_TEST_HOOKS=1 -- looked at ONCE, at the first scan: a stray KG_TEST_* variable in a server's environment
// does nothing.
uint32_t test_hook(const char *name)
{
    static const bool enabled = env_u32("KG_ENABLE_TEST_HOOKS", 0u) != 0;
    return enabled ? env_u32(name, 0u) : 0u;
}

int dalloc(kg_table *t, void **p, size_t bytes)
{
    if (t->fail_alloc_at && ++t->alloc_count == t->fail_alloc_at)
        return fail(KG_ERR_NOMEM, "device allocation failed: KG_TEST_FAIL_ALLOC test hook");
    hipError_t e = t->cache.get(p, bytes);
    if (e != hipSuccess) return fail(KG_ERR_NOMEM, std::string("device allocation failed: ") + hipGetErrorString(e));
    return KG_OK;
}

// Only call while the table's stream is idle (see DevCache).
void dfree(kg_table *t, void *p)
{
    if (p) t->cache.put(p);
}

// a block that leaves the cache for good: its user frees it with hipFree (a built table's records, a signature set)
int dalloc_detached(kg_table *t, uint8_t **p, size_t bytes)
{
    const int rc = dalloc(t, (void **)p, bytes);
    if (rc == KG_OK) t->cache.detach(*p);
    return rc;
}

// The owner of one such block (null: none): kg_hitset and kg_familyset hold theirs in it, so a set that is deleted, after a failed
// call as well, frees what it has.  The sets' *_free functions select the device first.
struct Detached {
    uint8_t *p = nullptr;
    Detached() = default;
    Detached(const Detached &) = delete;
    Detached &operator=(const Detached &) = delete;
    ~Detached() { if (p) (void)hipFree(p); }
};

int table_new(int device, kg_table **out);       // kg_host_table.hpp, beside kg_table_close

// One C ABI call at work on a table, constructed after the argument checks; `rc` says whether the call may go on.  Either it
// borrows an open table (takes the busy flag, or reports KG_ERR_BUSY with the caller's words) or it owns a fresh table-less
// context (table_new: a stream, the block caches, the pinned words).  Both reset the allocation count and arm the
// KG_TEST_FAIL_ALLOC hook.  Exit: the hook is disarmed; a borrowed table is no longer busy; an owned context is closed unless
// disown() passed it on.  Declare the call's Scratch after this object: the blocks are then back in the cache first.
struct CallScope {
    kg_table *t = nullptr;              // null: nothing to give back (busy, table_new failed, or disowned)
    const bool owned;
    int rc;
    CallScope(kg_table *tab, const char *busy_text) : owned(false), rc(tab->busy.exchange(1) != 0 ? fail(KG_ERR_BUSY, busy_text) : KG_OK)
    {
        if (rc == KG_OK) { t = tab; rc = arm(true); }
    }
    explicit CallScope(int device, bool hook = true) : owned(true), rc(table_new(device, &t))
    {
        if (rc == KG_OK) arm(hook);
    }
    ~CallScope()
    {
        if (!t) return;
        t->fail_alloc_at = 0;
        if (owned) kg_table_close(t);                       // (synchronises; leaves the thread's error text alone)
        else t->busy.store(0);
    }
    int arm(bool hook)
    {
        t->fail_alloc_at = hook ? test_hook("KG_TEST_FAIL_ALLOC") : 0u;
        t->alloc_count = 0;
        if (!owned) HIP_TRY(hipSetDevice(t->device));       // (table_new has set the device of an owned context)
        return KG_OK;
    }
    // the context goes to what the call hands out (a table, kg_result::own_tab, SetBase::own_tab)
    kg_table *disown() { kg_table *out = t; t = nullptr; out->fail_alloc_at = 0; return out; }
};

// exclusive prefix sum of d_in[n] -> d_out[n], total -> d_total (device uint64).  The total is exact for any input: the chunk
// sums and their sum are 64 bits.  d_out is the prefix modulo 2^32, so it is exact if and only if the total is below 2^32: a
// caller whose items are not flags reads the total, and refuses the call at 2^32, before it uses d_out as a layout.
int prefix_sum(kg_table *t, const uint32_t *d_in, uint64_t n, uint32_t *d_out, uint64_t *d_partial, uint64_t *d_total,
               hipStream_t stream = nullptr)
{
    if (!stream) stream = t->stream;
    uint32_t nb = (uint32_t)((n + kg::kScanChunk - 1) / kg::kScanChunk);
    if (nb == 0) nb = 1;
    hipLaunchKernelGGL(kg::scan_partials_kernel, dim3(nb), dim3(kg::kScanThreads), 0, stream, d_in, n, d_partial);
    hipLaunchKernelGGL(kg::scan_top_kernel, dim3(1), dim3(kg::kScanThreads), 0, stream, d_partial, nb, d_total);
    hipLaunchKernelGGL(kg::scan_final_kernel, dim3(nb), dim3(kg::kScanThreads), 0, stream, d_in, n, d_partial, d_out);
    HIP_TRY(hipGetLastError());
    return KG_OK;
}

// Several arrays of 32-bit words zeroed by one launch (kg_device.hpp, clear_many_kernel: eight slots).  Entries of no words are
// left out, and nothing is launched when none is left.  grid(most): the workgroups for `most` words, the largest entry.
struct ClearItem { void *p; uint64_t words; };

template <typename G>
int clear_words(hipStream_t stream, G grid, std::initializer_list<ClearItem> items)
{
    kg::ClearList cl = {};              // (unused slots: null, no words)
    uint64_t most = 0;
    for (const ClearItem &it : items) {
        if (!it.words) continue;
        if (cl.n == (int)std::size(cl.p)) return fail(KG_ERR_DEVICE, "more than eight arrays in one clear (internal error)");
        cl.p[cl.n] = (uint32_t *)it.p; cl.words[cl.n++] = it.words;
        most = std::max(most, it.words);
    }
    if (cl.n) hipLaunchKernelGGL(kg::clear_many_kernel, dim3(grid(most)), dim3(256), 0, stream, cl);
    return KG_OK;
}

struct Scratch {
    kg_table *t;
    std::vector<void *> ptrs;
    explicit Scratch(kg_table *tt) : t(tt) {}
    ~Scratch()
    {
        (void)hipStreamSynchronize(t->stream);      // blocks go back to the cache only when both streams are idle
        if (t->stream2) (void)hipStreamSynchronize(t->stream2);
        if (t->stream3) (void)hipStreamSynchronize(t->stream3);
        for (auto &os : t->ostream) if (os) (void)hipStreamSynchronize(os);
        for (void *p : ptrs) dfree(t, p);
    }
    void adopt(void *p) { ptrs.push_back(p); }
    void release(void *p) { ptrs.erase(std::find(ptrs.begin(), ptrs.end(), p)); }      // p outlives the scratch: its user frees it
    template <typename T> int get(T **p, size_t count)
    {
        void *v = nullptr;
        int rc = dalloc(t, &v, count * sizeof(T));
        if (rc) return rc;
        ptrs.push_back(v);
        *p = (T *)v;
        return KG_OK;
    }
};

// What the result sets that live in a context share (kg_regionset, kg_orfset, kg_selectset, kg_voteset, kg_compset): the
// context, whether the set owns it, and the device blocks the set took out of its cache.  A set keeps typed d_* members
// for reading; only this list frees.  Delete a set only while its context's stream is idle (see DevCache).
struct SetBase {
    kg_table *tab = nullptr;            // the context whose block cache the arrays came from
    bool own_tab = false;               // the set owns a table-less context (hand_out)
    std::vector<void *> blocks;
    SetBase() = default;
    SetBase(const SetBase &) = delete;
    SetBase &operator=(const SetBase &) = delete;
    ~SetBase()
    {
        if (!tab) return;
        (void)hipSetDevice(tab->device);
        for (void *p : blocks) dfree(tab, p);
        if (own_tab) kg_table_close(tab);
    }
    // p leaves the call's scratch and is the set's from here on (null: nothing to keep)
    template <typename T> T *keep(Scratch &sc, T *p)
    {
        if (p) { blocks.push_back(p); sc.release(p); }
        return p;
    }
};

// The set a call will hand out, in the call's context.  Declare it behind the CallScope and in front of the call's Scratch: on a
// failure the blocks are back in the cache first, the set goes next and the context last.
template <typename S>
int make_set(const CallScope &cs, std::unique_ptr<S> &set)
{
    set.reset(new (std::nothrow) S());
    if (!set) return fail(KG_ERR_NOMEM, "out of host memory");
    set->tab = cs.t;
    return KG_OK;
}

// The call succeeded: the caller gets the set.  An owned context goes with it; the scratch, back in the cache by now, goes to
// the driver and the set's blocks stay.
template <typename S>
int hand_out(CallScope &cs, std::unique_ptr<S> &set, S **out)
{
    if (cs.owned) {
        cs.t->cache.release_free();
        set->own_tab = true;
        cs.disown();
    }
    *out = set.release();
    return KG_OK;
}

// the device a getter of such a set selects (a null set: the getter fails before it is used)
int device_of(const SetBase *s) { return s ? s->tab->device : 0; }

// The range getter of every set: records [first, first + count) of the `have` present, `per` elements of T each, from src
// (device or host memory) to dst (host or device memory).  s: the set, looked at only for null; what: the getter's name.
template <typename T>
int copy_records(const void *s, int device, const T *src, size_t per, int64_t have, int64_t first, int64_t count, T *dst, const char *what,
                 const char *of = "the set")
{
    if (!s || (count > 0 && !dst)) return fail(KG_ERR_ARG, "null argument");
    if (first < 0 || count < 0 || first + count > have) return fail(KG_ERR_ARG, std::string(what) + ": range outside " + of);
    if (count == 0) return KG_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(dst, src + (size_t)first * per, (size_t)count * per * sizeof(T), hipMemcpyDefault));
    return KG_OK;
}

// The getter of a start array: all n + 1 entries
int copy_starts(const void *s, int device, const int64_t *src, int64_t n, int64_t *dst)
{
    if (!s || !dst) return fail(KG_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(dst, src, ((size_t)n + 1) * 8, hipMemcpyDefault));
    return KG_OK;
}

// The getter of a set's statistics
template <typename St>
int copy_stats(const void *s, const St *st, St *out)
{
    if (!s || !out) return fail(KG_ERR_ARG, "null argument");
    *out = *st;
    return KG_OK;
}

uint32_t grid_of(uint64_t n, uint32_t threads = 256)
{
    return (uint32_t)std::max<uint64_t>(1, (n + threads - 1) / threads);
}

uint64_t magic_of(uint64_t d)
{
    return d == 1 ? ~0ull : (uint64_t)(((unsigned __int128)1 << 64) / d);
}

std::string kmer_text(int64_t v)
{
    char b[32];
    snprintf(b, sizeof b, "%lld", (long long)v);
    return b;
}

// a failed call that has a result to give up: kg_result_free must not cost the caller the error text
int fail_and_free(kg_result *r, int rc) { std::string keep = g_err; kg_result_free(r); g_err = keep; return rc; }

// bits needed to write v: 0 for 0, 64 from 2^63 on
uint32_t bit_width(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

// bits needed to write every value below n
uint32_t bits_for(uint64_t n) { return n > 1 ? bit_width(n - 1) : 0; }

// N timing events of one call, created by the call and destroyed with it
template <int N>
struct Events {
    hipEvent_t e[N] = {};
    ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    int create() { for (auto &x : e) HIP_TRY(hipEventCreate(&x)); return KG_OK; }
    hipEvent_t operator[](int i) const { return e[i]; }
    float ms(int i, int j) const { float m = 0; (void)hipEventElapsedTime(&m, e[i], e[j]); return m; }
};

// One error word of a stage's kernels (filled with 0x7F bytes = kNoErr, lowered to the first offending index) and what it says.
struct ErrWord { int word, code; const char *prefix, *suffix; };
constexpr uint64_t kNoErr = 0x7F7F7F7F7F7F7F7Full;
static_assert(kNoErr == kg::kAssignNoErr && kNoErr == kg::kRegionNoErr, "the stages' kernels share the error words' \"none\"");

// d_words[n_words] -> t->h_pin + pin (pinned: read only after the synchronisation), then the first word of `table` that holds an error
int read_error_words(kg_table *t, const void *d_words, size_t n_words, int pin, std::initializer_list<ErrWord> table)
{
    HIP_TRY(hipMemcpyAsync(t->h_pin + pin, d_words, n_words * 8, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    for (const ErrWord &w : table)
        if (const uint64_t at = t->h_pin[pin + w.word]; at != kNoErr) return fail(w.code, w.prefix + kmer_text((int64_t)at) + w.suffix);
    return KG_OK;
}

// The same for a stage whose first n_err words each hold the first record with their error (what[k]: the text of word k):
// d_words[n_words] -> the stage's pinned words, then "record N" + what[k] for the first record with any error
int read_record_errors(kg_table *t, const void *d_words, size_t n_words, int n_err, const char *const *what)
{
    int rc;
    if ((rc = read_error_words(t, d_words, n_words, kPinStage, {}))) return rc;
    const uint64_t *h = t->h_pin + kPinStage;
    const int first = (int)(std::min_element(h, h + n_err) - h);
    if (h[first] != kNoErr) return fail(KG_ERR_ARG, "record " + kmer_text((int64_t)h[first]) + what[first]);
    return KG_OK;
}

// Host bytes -> d_dst through pinned pieces: several threads copy disjoint 32 MiB pieces of the caller's (possibly pageable)
// buffer into two pinned buffers each and hand them to the copy engine, as kg_table_open does.
int upload_pinned(kg_table *t, const uint8_t *src, size_t bytes, uint8_t *d_dst)
{
    const size_t CH = 32u << 20;
    const size_t n_pieces = (bytes + CH - 1) / CH;
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t n_thr = std::max<size_t>(1, std::min<size_t>({(size_t)8, (size_t)(hw ? hw : 4), n_pieces}));
    std::atomic<size_t> next{0};
    std::atomic<bool> ok{true};
    auto worker = [&]() {
        if (hipSetDevice(t->device) != hipSuccess) { ok = false; return; }
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
            if (!good) break;
            memcpy(pin[which], src + at, n);
            good = hipMemcpyAsync(d_dst + at, pin[which], n, hipMemcpyHostToDevice, s) == hipSuccess &&
                   hipEventRecord(done[which], s) == hipSuccess;
            used[which] = true;
            which ^= 1;
        }
        if (s && hipStreamSynchronize(s) != hipSuccess) good = false;
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
    return ok.load() ? KG_OK : fail(KG_ERR_DEVICE, "uploading to the device failed (pinned staging or host-to-device copy)");
}

// (key, value) pairs and their stable sort.  Side `cur` of the two buffer pairs holds the pairs; the other side is allocated by
// the first sort that has something to do, and is free again after it.
struct SortPairs {
    uint64_t *k[2] = {nullptr, nullptr};
    uint32_t *v[2] = {nullptr, nullptr};
    int cur = 0;
    int alloc(Scratch &sc, uint64_t n) { int rc = sc.get(&k[0], n); return rc ? rc : sc.get(&v[0], n); }
    uint64_t *keys() const { return k[cur]; }
    uint32_t *vals() const { return v[cur]; }
    // the pairs of a following sort: these values in their order, keys still to be written into the free side (null: no sort ran)
    SortPairs next() const { SortPairs s; s.k[0] = k[cur ^ 1]; s.v[0] = v[cur]; return s; }
    int sort(kg_table *t, Scratch &sc, uint64_t n, uint32_t key_bits);
};

// LSD radix sort (kg_build.hpp: build_hist_kernel / prefix_sum / build_scatter_kernel, <= 8 bits a pass) of n pairs by their low
// key_bits key bits; n <= 1 and key_bits == 0 need none.
int SortPairs::sort(kg_table *t, Scratch &sc, uint64_t n, uint32_t key_bits)
{
    if (n <= 1 || key_bits == 0) return KG_OK;
    const uint32_t n_tiles = (uint32_t)((n + kg::kBuildTile - 1) / kg::kBuildTile);
    const uint32_t passes = (key_bits + 7) / 8, bits = passes ? (key_bits + passes - 1) / passes : 1, radix = 1u << bits;
    const uint64_t n_hist = (uint64_t)radix * n_tiles;
    const uint64_t nb = (n_hist + kg::kScanChunk - 1) / kg::kScanChunk;
    uint32_t *hist = nullptr, *offs = nullptr;
    uint64_t *partial = nullptr;
    int rc;
    if ((rc = sc.get(&k[cur ^ 1], n)) || (rc = sc.get(&v[cur ^ 1], n)) || (rc = sc.get(&hist, n_hist)) ||
        (rc = sc.get(&offs, n_hist)) || (rc = sc.get(&partial, nb + 2)))
        return rc;
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t shift = p * bits;
        hipLaunchKernelGGL(kg::build_hist_kernel, dim3(n_tiles), dim3(kg::kBuildThreads), 0, t->stream, k[cur], n, shift, radix,
                           n_tiles, hist);
        HIP_TRY(hipGetLastError());
        if ((rc = prefix_sum(t, hist, n_hist, offs, partial, partial + nb + 1))) return rc;
        hipLaunchKernelGGL(kg::build_scatter_kernel, dim3(n_tiles), dim3(kg::kBuildThreads), 0, t->stream, k[cur], v[cur], n,
                           shift, bits, n_tiles, offs, k[cur ^ 1], v[cur ^ 1]);
        HIP_TRY(hipGetLastError());
        cur ^= 1;
    }
    return KG_OK;
}

}  // namespace
