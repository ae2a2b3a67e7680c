// kg_host_plan.hpp -- the plans of a kg_scan* call: the window blocks of the batch (plan_batch), the geometry of the partitioned
// and of the direct strategy (plan_partition, plan_direct) and the aggregation's knobs (plan_aggregate).  Arithmetic on the
// table, the batch and the environment, nothing else: nothing here launches a kernel or allocates on the device, and every
// environment read of a scan or an aggregation is here (once per call, at call time).
// Part of kmerguts_hip.hip's translation unit: behind kg_host_result.hpp, in front of the stages that enqueue what it planned
// (kg_host_aggregate.hpp, kg_host_scan.hpp).
#pragma once

namespace {

// ---- kg_scan*: plan (host arithmetic and every environment read); the stages that enqueue follow in kg_host_scan.hpp ----

// Run-time value -> template argument: calls f(std::integral_constant<T, V>) for the V among the listed values that equals
// x, the last one listed when none does.
template <typename T, T V, T... Vs, typename F>
void dispatch(T x, F &&f)
{
    if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<T, V>{});
    else if (x == V) f(std::integral_constant<T, V>{});
    else dispatch<T, Vs...>(x, f);
}

// Window blocks per sequence (KGJ:912 trip counts) and what follows from them.
struct BatchPlan {
    std::vector<uint32_t> ibase;                    // first block of sequence k; [n_seqs] = nblocks
    uint64_t nblocks = 0, windows = 0, residues = 0;
    uint64_t n_rows = 0, n_cont = 0;                // nblocks x PER window rows, n_seqs x PER containers
    int64_t longest = 0;                            // (record positions are below the length of their sequence)
};

template <bool AA>
int plan_batch(const int64_t *offsets, int64_t n_seqs, BatchPlan &b)
{
    constexpr uint32_t PER = AA ? 1 : 6;
    b.ibase.resize((size_t)n_seqs + 1);
    for (int64_t k = 0; k < n_seqs; k++) {
        int64_t L = offsets[k + 1] - offsets[k];
        if (L < 0) return fail(KG_ERR_ARG, "offsets must be non-decreasing");
        b.longest = std::max(b.longest, L);
        if (L > 0xFFFFFFF0ll) return fail(KG_ERR_LIMIT, "a single sequence longer than 2^32-16 characters");
        b.ibase[(size_t)k] = (uint32_t)b.nblocks;
        uint64_t nb;
        if (AA) {
            uint64_t nwin = L >= 9 ? (uint64_t)L - 8 : 0;       // i < len - 8
            b.windows += nwin;
            b.residues += (uint64_t)L;
            nb = (nwin + kg::kAaWinPerBlock - 1) / kg::kAaWinPerBlock;
        } else {
            uint64_t npos = L >= 24 ? (uint64_t)L - 23 : 0;     // forward positions that start a 24-base window
            b.windows += 2 * npos;
            for (int f = 0; f < 3; f++)
                if (L - f >= 3) b.residues += 2 * (uint64_t)((L - f) / 3);
            nb = (npos + kg::kDnaPosPerBlock - 1) / kg::kDnaPosPerBlock;
        }
        b.nblocks += nb;
        if (b.nblocks > 0x7FFFFFFFull / PER) return fail(KG_ERR_LIMIT, "batch too large: more than 2^31-1 window rows; split the batch");
    }
    b.ibase[(size_t)n_seqs] = (uint32_t)b.nblocks;
    if (b.windows > 0xFFFFFF00ull) return fail(KG_ERR_LIMIT, "batch too large: more than 2^32-256 windows; split the batch");
    b.n_rows = b.nblocks * PER;
    b.n_cont = (uint64_t)n_seqs * PER;
    return KG_OK;
}

// Buckets of 2^shift slots that cover a record stream of `limit` slots.
uint64_t bucket_count(uint64_t limit, uint32_t shift) { return (limit + (1ull << shift) - 1) >> shift; }

// Geometry of the partitioned strategy (queries bucketed by slot range first; kg_partition.hpp) for one batch: arithmetic on
// the table, the batch and the environment, nothing else.
struct PartPlan {
    bool applicable = false;            // false: the batch takes the direct strategy (nothing below shift / buckets is set)
    uint32_t shift = 0, buckets = 0;    // bucket = 2^shift slots (= bytes of tags)
    uint32_t n_chunks = 0;
    std::vector<uint64_t> clo;          // chunk c = blocks [clo[c], clo[c+1])
    std::vector<int64_t> cseq;          //         = sequences [cseq[c], cseq[c+1])
    uint64_t max_chunk = 0;             // blocks of the largest chunk
    uint32_t n_wg = 0, cap = 0;         // scatter workgroups; entries per region (bucket x workgroup)
    uint64_t n_regions = 0;             // per chunk
    uint32_t ovf_cap = 0;               // overflow list of one chunk (groups)
    uint32_t gshift = 10, groups_stride = 0;        // ordered placement: groups of 2^gshift rows, groups provisioned per chunk
    size_t next_stride = 0;             // tag pass: hand-out counters per chunk
    size_t scatter_lds = 0;
    bool use_bidx = false, part_counters = false, prog_index = false;
    uint32_t probe_grid = 0, index_grid = 0, verify_grid = 0, lowc_grid = 0, ovf_grid = 0, order_grid = 0;
    uint32_t scatter_prio = 0, index_prio = 0, verify_prio = 0, index_r = 1, probe_grab = 0;
    uint32_t flush_list = 0;            // scatter pass: completed groups a wave flushes per pass
    uint64_t list_slack = 0, ucap = 0, ccap = 0;    // hit / candidate list capacities per chunk the first attempt starts with
    uint32_t n_os = 0;                  // ordering streams (KG_ORDER_STREAMS)
    bool early_totals = false, place_staged = false, debug = false;
};

template <bool AA>
int plan_partition(const kg_table *t, const BatchPlan &b, bool progress, bool counters_req, PartPlan &pl)
{
    constexpr uint32_t PER = AA ? 1 : 6;
    const uint64_t nblocks = b.nblocks;
    // bucket = 2^shift slots (= bytes of tags); at most kMaxBuckets buckets; quotient must fit 32 - shift bits
    uint32_t shift = env_knob("KG_PART_SHIFT", 21u, 4u, 31u);
    const uint64_t qmax = (uint64_t)KG_MAX_ENCODED / (uint64_t)t->num_sigs + 1;
    while (shift > 4 && qmax >= (1ull << (32 - shift))) shift--;     // small tables: large quotients, small buckets
    while (bucket_count(t->limit, shift) > (uint64_t)kg::kMaxBuckets) shift++;
    // the scatter workgroup keeps a 128-byte buffer per bucket in LDS: at most 160 KiB with its encode scratch
    while (kg::scatter_lds_bytes<AA>((uint32_t)bucket_count(t->limit, shift)) > 160u * 1024) shift++;
    // the scatter pass splits k-mers with kg::split_fast: 64 <= numSigs < 2^31
    // (and the tag / verify passes keep slots in 32 bits: a table FILE may be longer than numSigs, KGJ:964-999)
    const bool fits = shift < 32 && qmax < (1ull << (32 - shift)) && nblocks <= (1ull << 23) && t->m35 != 0 &&
                      t->limit < (1ull << 32) - 64;
    // Measured against the 33.6 GB table (profiles/r01_partition_path.md), whole scan incl. ordering, direct vs
    // partitioned: 1 Gbp 35.0 / 21.4 ms, 600 Mbp 21.8 / 13.6, 400 Mbp 14.6 / 9.4, 200 Mbp 7.0 / 5.4, 100 Mbp 3.6 / 3.4 (one chunk).
    // Small inputs and L2/MALL-sized tables stay on the direct kernel.
    // KG_PARTITION: 0 direct, 1 partitioned whenever possible, 2 (default) auto.
    const uint32_t mode = env_u32("KG_PARTITION", 2u);
    const bool worth = t->limit >= (64ull << 20) && b.windows >= (1ull << 27);
    if (!(fits && nblocks > 0 && (mode == 1 || (mode == 2 && worth)))) return KG_OK;
    pl.shift = shift;
    pl.buckets = (uint32_t)bucket_count(t->limit, shift);

    constexpr uint32_t WIN = AA ? 64u : 384u;                                    // windows per block
    // The batch is cut into chunks of whole sequences.  Chunk c goes through scatter (stream), tag pass (stream2),
    // then verification and ordered placement (stream3) while the chunks behind it are scattered and probed: the scatter pass is LDS/issue-
    // bound with one 16-wave workgroup per CU, the tag pass is L2-bound with few registers and no LDS, verification
    // and placement wait on random HBM lines, so they share the CUs.  A chunk's hits are a contiguous range of
    // hits[] (whole sequences), chained by a device-side running total.
    uint32_t want = env_u32("KG_PART_CHUNKS", 4u);
    if (want < 1) want = 1;
    if (want > kMaxChunks) want = kMaxChunks;
    // How many: a pass has costs that do not shrink with the chunk, so small batches take few.  Measured with the wave
    // priorities in place (r04 c59; ms per scan in 1 / 2 / 3 / 4 chunks): 100 Mbp 2.50 / 2.46 / 2.72 / -, 125 Mbp 2.94 / 2.87 /
    // 3.17 / -, 250 Mbp 5.15 / 4.83 / 5.17 / -, 500 Mbp - / - / 8.63 / 9.0, 1 Gbp - / - / 16.0 / 15.1 (five: 15.45):
    // round(sqrt(blocks / 325 000)) but at least two, one below 450 000 blocks (~85 Mbp).  KG_PART_MIN_CHUNK_BLOCKS (tests) replaces the
    // rule by "as many as KG_PART_CHUNKS allows with at least that many blocks each".
    if (getenv("KG_PART_MIN_CHUNK_BLOCKS")) {
        const uint64_t min_chunk = std::max(1u, env_u32("KG_PART_MIN_CHUNK_BLOCKS", 600000u));
        while (want > 1 && nblocks / want < min_chunk) want--;
    } else {
        const uint32_t by_size = nblocks < 450000 ? 1u : std::max(2u, (uint32_t)std::lround(std::sqrt((double)nblocks / 325000.0)));
        want = std::min(want, std::max(1u, by_size));
    }
    pl.clo.push_back(0); pl.cseq.push_back(0);
    // KG_PART_TAPER="30,30,25,15": chunk sizes in percent instead of equal chunks (tuning aid)
    std::vector<double> cum;
    if (const char *tp = getenv("KG_PART_TAPER")) {
        double acc = 0;
        for (const char *q = tp; *q;) {
            char *endp = nullptr;
            const double v = strtod(q, &endp);
            if (endp == q) break;
            acc += v; cum.push_back(acc);
            q = *endp == ',' ? endp + 1 : endp;
        }
        if (cum.size() >= 2 && cum.size() <= kMaxChunks && acc > 0) { for (auto &x : cum) x /= acc; want = (uint32_t)cum.size(); }
        else cum.clear();
    }
    for (uint32_t c = 1; c < want; c++) {
        const uint64_t target = cum.empty() ? nblocks * c / want : (uint64_t)((double)nblocks * cum[c - 1]);
        const auto it = std::lower_bound(b.ibase.begin(), b.ibase.end(), (uint32_t)target);        // a sequence start
        const uint64_t cut = *it;
        if (cut > pl.clo.back() && cut < nblocks) { pl.clo.push_back(cut); pl.cseq.push_back((int64_t)(it - b.ibase.begin())); }
    }
    pl.clo.push_back(nblocks); pl.cseq.push_back((int64_t)b.ibase.size() - 1);
    pl.n_chunks = (uint32_t)pl.clo.size() - 1;
    for (uint32_t c = 0; c < pl.n_chunks; c++) pl.max_chunk = std::max(pl.max_chunk, pl.clo[c + 1] - pl.clo[c]);
    const uint64_t max_chunk = pl.max_chunk;
    const uint64_t chunk_blocks = (max_chunk + kg::kScatterWaves - 1) / kg::kScatterWaves * kg::kScatterWaves;
    const double max_frac = (double)max_chunk / (double)nblocks;
    uint32_t n_wg = env_knob("KG_PART_WGS", 256u, 1u, kMaxGrid);
    if ((uint64_t)n_wg * kg::kScatterWaves > chunk_blocks) n_wg = (uint32_t)((chunk_blocks + kg::kScatterWaves - 1) / kg::kScatterWaves);
    const uint64_t blocks_per_wg = ((chunk_blocks + (uint64_t)n_wg * kg::kScatterWaves - 1) / ((uint64_t)n_wg * kg::kScatterWaves)) * kg::kScatterWaves;
    // region capacity: the mean if every window were valid and hashed uniformly, plus 6 sigma, in 16-entry groups
    const double mean = (double)blocks_per_wg * WIN / (double)pl.buckets * (env_u32("KG_PART_SLACK", 100u) / 100.0);
    const uint64_t cap64 = ((uint64_t)(mean + 6.0 * std::sqrt(mean) + 32.0) + 15) / 16 * 16;
    // the scatter pass's address arithmetic is in 24-bit multiplies (region number x capacity): geometries beyond that
    // (one bucket and millions of blocks per scatter workgroup; not reachable with the default knobs) take the direct path
    if (cap64 >= (1ull << 24) || (uint64_t)pl.buckets * n_wg >= (1ull << 24)) return KG_OK;
    pl.n_wg = n_wg;
    pl.cap = (uint32_t)cap64;
    pl.n_regions = (uint64_t)pl.buckets * n_wg;
    // overflow list of one chunk (groups): an eighth of the regions' capacity (low-complexity sequence: 3 % of the
    // bases in homopolymer runs overflow ~5 % of the entries; beyond the list the scan falls back to direct probing)
    pl.ovf_cap = env_u32("KG_PART_OVF_GROUPS", (uint32_t)std::min<uint64_t>(1u << 23, std::max<uint64_t>(65536, pl.n_regions * pl.cap / 16 / 8)));
    // ordered placement (kg_order.hpp): groups of 2^gshift rows, at most kMaxGroups per chunk (8192 while 4096-row groups allow it)
    while (pl.gshift < 12 && ((max_chunk * PER) >> pl.gshift) + 2 > 8192) pl.gshift++;
    pl.groups_stride = (uint32_t)(((max_chunk * PER) >> pl.gshift) + 2);      // a chunk's rows start anywhere inside a group
    if (pl.groups_stride > kg::kMaxGroups) return fail(KG_ERR_LIMIT, "a chunk of the batch holds more than 2^26 window rows");
    pl.next_stride = std::max<size_t>((size_t)pl.buckets + 8, 256);   // tag pass: one hand-out counter per XCD group, 128 B apart
    // the tag pass on the byte home index instead of the tags (bucket_index_kernel) unless the scan counts the slots it
    // inspects (the walk the index avoids) or KG_BIDX=0.  KG_F_PROGRESS alone runs the index pass's PROG variant (it
    // summarises the certain misses' walks) and the verify / overflow passes' PROG variants (they note theirs), nothing counted.
    pl.use_bidx = t->d_bidx != nullptr && !counters_req && env_u32("KG_BIDX", 1u) != 0;
    pl.part_counters = (counters_req || progress) && !pl.use_bidx;
    pl.prog_index = progress && pl.use_bidx;
    pl.scatter_lds = kg::scatter_lds_bytes<AA>(pl.buckets);
    // the scatter pass's flush list: what a wave's encode scratch holds, at most an entry per lane; KG_SCATTER_FLUSH_LIST (tests)
    // lowers it, so that a round's completed groups go in several passes
    pl.flush_list = env_knob("KG_SCATTER_FLUSH_LIST", kg::scatter_flush_list_max<AA>(), 1u, kg::scatter_flush_list_max<AA>());
    // Tag workgroups per CU.  How many of them run beside a scatter workgroup of the next chunk is decided by the SIMDs'
    // VGPRs (kg_partition.hpp, "Register budgets": two per CU since round 3, one before), the rest wait for the scatter
    // workgroup to leave; the hand-out is by ticket, so the count only decides how fast freed registers are taken up.
    // Round 2 (one tag wave per SIMD beside the scatter pass): 4 per CU 20.4 ms, 8 per CU 20.8 (profiles/r02_pipeline.md);
    // round 3 (two): 4 per CU 19.78 ms, 8 per CU 19.56, bench.py 20.5 -> 20.25 ms per step (profiles/r03_experiments.md).
    pl.probe_grid = env_knob("KG_PROBE_GRID", 256u * 8u, 8u, kMaxGrid, 8u);
    // the byte-index pass: four workgroups per CU -- at 32 VGPRs they are the four waves per SIMD that fit beside a scatter
    // workgroup (4 x 96 + 4 x 32 = 512); with eight queued the stage is 0.4 ms slower (16.37 against 15.93 ms, r04 c04)
    pl.index_grid = env_knob("KG_INDEX_GRID", 256u * 4u, 8u, kMaxGrid, 8u);
    // wave priorities (s_setprio) of the passes that share the CUs: kg_device.hpp, set_wave_prio
    pl.scatter_prio = std::min(3u, env_u32("KG_SCATTER_PRIO", 1u));
    pl.index_prio = std::min(3u, env_u32("KG_INDEX_PRIO", 2u));
    pl.verify_prio = std::min(3u, env_u32("KG_VERIFY_PRIO", pl.n_chunks == 1 ? 2u : 0u));
    // ... and the regions the byte-index pass takes per hand-out: regions expected to hold fewer than ~640 / ~320 entries
    // (about 0.7 of the mean the capacity was computed from is valid DNA) are handed out two / four at a time
    // (bucket_index_kernel)
    uint32_t index_r = env_u32("KG_INDEX_R", 0u);
    if (index_r == 0) index_r = mean * 0.7 >= 640.0 ? 1u : mean * 0.7 >= 320.0 ? 2u : 4u;
    if (index_r != 1 && index_r != 2) index_r = 4;
    while (index_r > 1 && (n_wg % index_r != 0 || kg::kIndexN % index_r != 0)) index_r /= 2;
    pl.index_r = index_r;
    // verify workgroups: two per CU.  With eight (until round 3) the pass alone is 15 % faster, but its workgroups take all the
    // registers an ending tag pass frees, and the next tag pass -- the critical chain -- starts behind them: stage 18.3 ->
    // 18.15 ms, 125 Mbp shard 3.18 -> 3.10 (profiles/r03_experiments.md)
    pl.verify_grid = env_knob("KG_VERIFY_GRID", 256u * 2u, 1u, kMaxGrid);
    // The two kernels that usually find nothing to do (no low-complexity block set aside, no overflow group) sit on the
    // stage's critical chain -- in front of every tag pass and behind every verify pass -- and beside the other passes a
    // grid of 2048 / 1024 workgroups takes 0.1 / 0.35 ms just to be scheduled and leave (profiles/r03_kernel_stats.csv);
    // one workgroup per CU leaves in microseconds and is still the whole chip when there is work.
    pl.lowc_grid = env_knob("KG_LOWC_GRID", 256u, 1u, kMaxGrid);
    pl.ovf_grid = env_knob("KG_OVF_GRID", 256u, 1u, kMaxGrid);
    // per-chunk lists: hits (unordered) and candidates = fingerprint matches (hits + ~0.4 % of the probes) + the
    // ~2 % of the probes whose first tag window decides nothing
    pl.list_slack = (uint64_t)(std::max(std::max(pl.probe_grid, pl.index_grid), pl.verify_grid) + 64) * 4 * kg::kUChunk + 4096;
    pl.ucap = ((uint64_t)((double)b.windows * t->stage_ratio * max_frac) + pl.list_slack + kg::kUChunk - 1) / kg::kUChunk * kg::kUChunk;
    pl.ccap = ((uint64_t)((double)b.windows * (t->stage_ratio * 1.25 + 0.03) * max_frac) + pl.list_slack + kg::kUChunk - 1) /
              kg::kUChunk * kg::kUChunk;
    if (test_hook("KG_TEST_TINY_LISTS")) pl.ucap = pl.ccap = kg::kUChunk;      // tests: force the resize-and-rerun path
    const uint32_t grab_unit = 256u * (uint32_t)std::max(kg::kProbeN, kg::kIndexN);      // (powers of two: the larger is a multiple of the other)
    pl.probe_grab = env_knob("KG_PROBE_GRAB", pl.cap, grab_unit, 1u << 24, grab_unit);
    // Ordering streams and early totals: scan_partitioned, in front of the chunks' orderings
    pl.n_os = pl.n_chunks < 2 ? 0u : std::min(env_u32("KG_ORDER_STREAMS", 0u), kMaxOrderStreams);
    pl.early_totals = pl.n_os == 0 && env_u32("KG_EARLY_TOTALS", 1u) != 0;     // (every chunk's ordering on one stream, in order: behind every verify pass)
    pl.order_grid = env_knob("KG_ORDER_GRID", 256u * 3u, 1u, kMaxGrid);
    pl.place_staged = pl.gshift == 10 && env_u32("KG_PLACE_STAGED", 1u) != 0;
    pl.debug = getenv("KG_DEBUG") != nullptr;
    pl.applicable = true;
    return KG_OK;
}

// Geometry of the direct strategy (every probe a random 128-byte line from HBM unless the tag array is L2-sized).
struct DirectPlan {
    uint32_t scan_grid, stage_chunk;
    const uint32_t *d_hbits;            // the table's bit-per-slot digest, or null
    uint32_t rpg;                       // rows probed together per lane
    uint64_t stage_cap;                 // staging records the first attempt starts with
};

template <bool AA>
DirectPlan plan_direct(const kg_table *t, const BatchPlan &b, bool counters)
{
    DirectPlan pl;
    // persistent grid: enough workgroups to fill 256 CUs, few enough that per-wave staging chunks stay small
    pl.scan_grid = env_knob("KG_SCAN_GRID", 256u * 8u, 1u, kMaxGrid);
    pl.stage_chunk = env_knob("KG_STAGE_CHUNK", 256u, 1u, 1u << 12);
    // the table's bit-per-slot digest as the direct kernel's first question (tables of <= kHbitsMaxSlots slots; not for scans
    // that count the slots they inspect): config 5's scan 2.28 -> 1.80 ms (r04 c34)
    // KG_DIRECT_FILTER: 0 never, 1 (default) when the tags no longer fit an XCD's 4 MB L2 (below that the bit is one more
    // dependent load in front of an L2 hit), 2 whenever the table has the digest (tests)
    const uint32_t filter_mode = env_u32("KG_DIRECT_FILTER", 1u);
    pl.d_hbits = (counters || filter_mode == 0 || (filter_mode == 1 && t->limit <= (4ull << 20))) ? nullptr : t->d_hbits;
    // rows probed together per lane: three; six behind the digest, where two probes out of three end at the bit (1.80 -> 1.75 ms)
    pl.rpg = AA ? 1u : env_u32("KG_SCAN_RPG", pl.d_hbits ? 6u : 3u);
    if (pl.rpg != 1 && pl.rpg != 2 && pl.rpg != 3 && pl.rpg != 6) pl.rpg = 3;
    pl.stage_cap = (uint64_t)((double)b.windows * t->stage_ratio) + 4096 + (uint64_t)pl.scan_grid * kg::kWavesPerWG * pl.stage_chunk;
    if (pl.stage_cap > 0xFFFFFF00ull) pl.stage_cap = 0xFFFFFF00ull;
    if (test_hook("KG_TEST_TINY_LISTS")) pl.stage_cap = 256;                    // tests: force the resize-and-rerun path
    return pl;
}

// The aggregation's knobs (kg_host_aggregate.hpp, aggregate_stage).
struct AggPlan {
    uint32_t pshift;                    // log2 of the records per block of the pieces (at most one piece start per block)
    bool pieces_on;
    uint32_t agg_pairs;
};

AggPlan plan_aggregate()
{
    AggPlan pl;
    // KG_AGG_BLOCK_SHIFT: log2 of the records per block of the pieces (at most one piece start per block; tests lower it)
    pl.pshift = std::min(20u, std::max(6u, env_u32("KG_AGG_BLOCK_SHIFT", 9u)));
    pl.pieces_on = env_u32("KG_AGG_PIECES", 1u) != 0;
    pl.agg_pairs = env_u32("KG_AGG_PAIRS", 1u);
    return pl;
}

}  // namespace
