// kg_host_build.hpp -- kg_table_build / kg_table_build_device: a signature list -> a resident table (kernels: kg_build.hpp).
// Part of kmerguts_hip.hip's translation unit: one of the batch stages, included behind the kernel headers, kg_host.hpp and the
// hosts of the table, the result and the scan.
#pragma once

namespace {

// Everything up to table_finish.  Scratch comes from the table's block cache (dalloc: KG_TEST_FAIL_ALLOC applies) and is
// back in it when this returns; the records are taken out of the cache and owned by the table.
int build_records(kg_table *t, const uint8_t *h_sigs, const uint8_t *d_sigs, uint64_t n, uint64_t *n_placed, float ms[4])
{
    const uint64_t S = (uint64_t)t->num_sigs;
    Scratch sc(t);
    int rc;
    if ((rc = dalloc_detached(t, &t->d_entries, (S * 24 + 15) / 16 * 16))) return rc;
    t->own_entries = true;
    if (h_sigs && n) {
        uint8_t *d = nullptr;
        if ((rc = sc.get(&d, n * 24))) return rc;
        if ((rc = upload_pinned(t, h_sigs, n * 24, d))) return rc;
        d_sigs = d;
    }
    Events<5> ev;
    if ((rc = ev.create())) return rc;
    // (home, kmer) order == (home, q) order; c = home * Q + q < 20^8 + S
    const uint64_t Q = (uint64_t)(KG_MAX_ENCODED - 1) / S + 1, magic = magic_of(S), magic_q = magic_of(Q);
    const uint64_t c_max = (uint64_t)((unsigned __int128)S * Q - 1);
    const uint32_t key_bits = std::max(1u, bit_width(c_max));
    const uint32_t n_tiles = (uint32_t)((n + kg::kBuildTile - 1) / kg::kBuildTile);
    unsigned long long *d_cnt = nullptr;                // [0] first bad index, [1] smallest duplicate, [2] placed
    if ((rc = sc.get(&d_cnt, 4))) return rc;
    HIP_TRY(hipMemsetAsync(d_cnt, 0xFF, 16, t->stream));
    HIP_TRY(hipMemsetAsync(d_cnt + 2, 0, 8, t->stream));
    HIP_TRY(hipEventRecord(ev[0], t->stream));
    SortPairs sp;
    if (n) {
        if ((rc = sp.alloc(sc, n))) return rc;
        const uint64_t want = (n + kg::kBuildThreads - 1) / kg::kBuildThreads;
        hipLaunchKernelGGL(kg::build_keys_kernel, dim3((uint32_t)std::min<uint64_t>(want, 256ull * 32)), dim3(kg::kBuildThreads), 0,
                           t->stream, d_sigs, n, S, magic, Q, sp.keys(), sp.vals(), d_cnt);
        HIP_TRY(hipGetLastError());
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, d_cnt, 8, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        if (bad != ~0ull) {
            int64_t kmer = 0;
            if (h_sigs) memcpy(&kmer, h_sigs + bad * 24, 8);
            else HIP_TRY(hipMemcpy(&kmer, d_sigs + bad * 24, 8, hipMemcpyDeviceToHost));
            return fail(KG_ERR_ARG, "signature " + kmer_text((int64_t)bad) + ": k-mer " + kmer_text(kmer) +
                                        " is outside [0, 20^8) (the smallest such input index)");
        }
        if ((rc = sp.sort(t, sc, n, key_bits))) return rc;
    }
    HIP_TRY(hipEventRecord(ev[1], t->stream));
    int64_t *tile_max = nullptr, *tile_pre = nullptr;
    if (n) {
        if ((rc = sc.get(&tile_max, n_tiles)) || (rc = sc.get(&tile_pre, n_tiles))) return rc;
        hipLaunchKernelGGL(kg::build_tile_max_kernel, dim3(n_tiles), dim3(kg::kBuildThreads), 0, t->stream, sp.keys(), n, Q, magic_q, S,
                           tile_max, d_cnt + 1);
        hipLaunchKernelGGL(kg::build_tile_scan_kernel, dim3(1), dim3(kg::kBuildThreads), 0, t->stream, tile_max, n_tiles, tile_pre);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[2], t->stream));
    const uint64_t n_chunks = (S * 24 + 15) / 16;
    hipLaunchKernelGGL(kg::build_fill_kernel, dim3((uint32_t)std::min<uint64_t>((n_chunks + 255) / 256, 256ull * 64)),
                       dim3(kg::kBuildThreads), 0, t->stream, (uint4 *)t->d_entries, n_chunks);
    HIP_TRY(hipGetLastError());
    if (n) {
        hipLaunchKernelGGL(kg::build_place_kernel, dim3(n_tiles), dim3(kg::kBuildThreads), 0, t->stream, sp.keys(), sp.vals(), n, Q,
                           magic_q, tile_pre, d_sigs, S, t->d_entries, d_cnt + 2);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[3], t->stream));
    unsigned long long cnt[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, d_cnt, 24, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    if (cnt[1] != ~0ull)
        return fail(KG_ERR_ARG, "duplicate k-mer " + kmer_text((int64_t)cnt[1]) + " (the smallest k-mer that occurs more than once)");
    for (int i = 0; i < 3; i++) HIP_TRY(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    *n_placed = cnt[2];
    return KG_OK;
}

int build_entry(const uint8_t *h_sigs, const uint8_t *d_sigs, int64_t n, int64_t num_sigs, int device, int64_t *n_placed, kg_table **out)
{
    if (!out) return fail(KG_ERR_ARG, "null argument");
    *out = nullptr;
    if (n < 0) return fail(KG_ERR_ARG, "n < 0");
    if (num_sigs <= 0) return fail(KG_ERR_ARG, "num_sigs <= 0");
    if ((uint64_t)n >= (1ull << 32)) return fail(KG_ERR_LIMIT, "kg_table_build: 2^32 or more signatures in one call");
    if (n > 0 && !h_sigs && !d_sigs) return fail(KG_ERR_ARG, "null signature array");
    if (d_sigs && ((uintptr_t)d_sigs & 7)) return fail(KG_ERR_ARG, "kg_table_build_device: the signatures must be 8-byte aligned");
    if ((uint64_t)num_sigs > (~0ull >> 1) / 24) return fail(KG_ERR_LIMIT, "num_sigs too large");
    CallScope cs(device);               // the table-to-be: closed again on every failure below
    if (cs.rc) return cs.rc;
    kg_table *t = cs.t;
    t->num_sigs = num_sigs;
    t->entry_size = KG_TABLE_ENTRY_SIZE;
    t->version = 1;
    t->limit = (uint64_t)num_sigs;
    // a device input may still be written by another (blocking or non-blocking) stream
    if (d_sigs && hipDeviceSynchronize() != hipSuccess) return fail(KG_ERR_DEVICE, "hipDeviceSynchronize failed");
    uint64_t placed = 0;
    float ms[5] = {0, 0, 0, 0, 0};
    int rc = build_records(t, h_sigs, d_sigs, (uint64_t)n, &placed, ms);
    t->cache.release_all();                             // the build's scratch goes back to the driver, not to the table
    if (rc) return rc;
    Events<2> fin;                                      // (only created under KG_DEBUG)
    const bool timed = getenv("KG_DEBUG") && fin.create() == KG_OK && hipEventRecord(fin[0], t->stream) == hipSuccess;
    rc = table_finish(t);
    if (timed && rc == KG_OK && hipEventRecord(fin[1], t->stream) == hipSuccess && hipEventSynchronize(fin[1]) == hipSuccess)
        ms[3] = fin.ms(0, 1);
    if (rc) return rc;
    if (getenv("KG_DEBUG"))
        fprintf(stderr, "[kg] kg_table_build: n=%lld num_sigs=%lld placed=%llu sort_ms=%.3f place_ms=%.3f fill_scatter_ms=%.3f finish_ms=%.3f\n",
                (long long)n, (long long)num_sigs, (unsigned long long)placed, ms[0], ms[1], ms[2], ms[3]);
    if (n_placed) *n_placed = (int64_t)placed;
    *out = cs.disown();
    return KG_OK;
}

}  // namespace

extern "C" {

int kg_table_build(const kg_signature *sigs, int64_t n, int64_t num_sigs, int device, int64_t *n_placed, kg_table **out)
{
    return build_entry((const uint8_t *)sigs, nullptr, n, num_sigs, device, n_placed, out);
}

int kg_table_build_device(const kg_signature *d_sigs, int64_t n, int64_t num_sigs, int device, int64_t *n_placed, kg_table **out)
{
    return build_entry(nullptr, (const uint8_t *)d_sigs, n, num_sigs, device, n_placed, out);
}

}  // extern "C"
