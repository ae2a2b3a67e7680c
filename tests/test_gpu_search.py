"""kg_proteins_search on the GPU against tests/search_model.py: records, starts and counts byte for byte.  The border cases are
derived from the constants of kg_search.hpp; cluster_model.token_batch gives proteins whose k-mer sets, and with them the order of
the k-mer runs, are chosen one by one."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import align_model as A
import cluster_model as M
import search_model as S
from kmergutsjava_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TEXT = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_search.hpp")).read()
TILE = int(re.search(r"constexpr int kSearchTile = (\d+);", _TEXT).group(1))
THREADS = int(re.search(r"constexpr int kSearchThreads = (\d+);", _TEXT).group(1))
MAX_CAND = int(re.search(r"constexpr int kSearchMaxCand = (\d+);", _TEXT).group(1))
NO_ALIGN = dict(max_cells=1)            # every pair skipped: the order is (s, target) and the model aligns nothing


def _search(seq, off, n_db, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.search_proteins(seq, off, n_db, **kw)


def _model(seq, off, n_db, **kw):
    kw = dict(kw)
    kw.update(kw.pop("align", None) or {})
    for k in ("max_windows", "max_pairs"):
        kw.pop(k, None)
    return S.search_model(seq, off, n_db, **kw)


def _same(seq, off, n_db, **kw):
    hits, start, st = _search(seq, off, n_db, **kw)
    want, wstart, wst = _model(seq, off, n_db, **kw)
    assert {k: st[k] for k in S.STAT_KEYS} == wst
    assert start.tobytes() == wstart.tobytes() and hits.tobytes() == want.tobytes()
    return hits, start, st


def test_the_constants():
    assert (TILE, MAX_CAND) == (N.SEARCH_TILE, N.SEARCH_MAX_CAND) and TILE % (2 * THREADS) == 0


# ---- the join at its borders ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_t", [1, 2, 63, 64, 65, 257])
def test_one_kmer_in_many_targets_and_queries(n_t):
    """One k-mer shared by n_t targets and 1, 63, 64, 65 queries; the mask at the target count, one below and one above."""
    for n_q in (1, 63, 64, 65):
        seq, off = M.token_batch([[5]] * (n_t + n_q))
        for mask in (n_t - 1, n_t, n_t + 1):
            if mask < 1:
                continue
            hits, start, st = _same(seq, off, n_t, min_shared=1, max_db_per_kmer=mask)
            assert st["join_pairs"] == (n_t * n_q if mask >= n_t else 0) and st["kmers_masked"] == (mask < n_t)
            assert len(hits) == (min(n_t, 8) * n_q if mask >= n_t else 0)


def _factor(n: int):
    nd = max(d for d in range(1, 257) if n % d == 0)
    return nd, n // nd


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_join_pairs_of_a_tile_and_one_more_or_less(extra):
    nd, nq = _factor(TILE + extra)
    seq, off = M.token_batch([[7]] * (nd + nq))
    hits, start, st = _same(seq, off, nd, min_shared=1, max_cand=2)
    assert st["join_pairs"] == TILE + extra and len(hits) == nq * min(nd, 2)


def test_one_run_over_three_tiles():
    """3 items, then one k-mer of 100 targets and ceil(2 tiles / 100) + 1 queries, then 1 item."""
    nq = 2 * TILE // 100 + 2
    members = [[2, 1] if d == 0 else [2] for d in range(100)] + [[2, 1] if q < 3 else [2] for q in range(nq)]
    members[99] = [2, 3]
    members[100 + nq - 1] = [2, 3]
    seq, off = M.token_batch(members)
    hits, start, st = _same(seq, off, 100, min_shared=1, max_cand=3)
    assert st["join_pairs"] == 3 + 100 * nq + 1 > 2 * TILE + 3 and st["kmers_joined"] == 3
    assert [tuple(r) for r in hits[["target", "shared"]][:3].tolist()] == [(0, 2), (1, 1), (2, 1)]


def _border_batch(n_zero: int = 300):
    """8 targets and 8 queries.  Runs in k-mer order: n_zero of weight 0 (target-only, query-only and masked in turn), a tile of
    weight-1 runs with n_zero weight-0 runs in its middle, n_zero weight-0 runs on the tile border, 100 weight-1 runs, n_zero
    weight-0 runs.  The masked k-mers are in targets 0, 1, 2 and a query: max_db_per_kmer = 2 masks them."""
    members = [[] for _ in range(16)]
    v = 0

    def zero(count):
        nonlocal v
        for k in range(count):
            if k % 3 == 0:
                members[v % 8].append(v)
            elif k % 3 == 1:
                members[8 + v % 8].append(v)
            else:
                for p in (0, 1, 2, 8 + v % 8):
                    members[p].append(v)
            v += 1

    def one(count):
        nonlocal v
        for _ in range(count):
            members[v % 8].append(v)
            members[8 + (v // 8) % 8].append(v)
            v += 1

    zero(n_zero); one(TILE // 2); zero(n_zero); one(TILE - TILE // 2); zero(n_zero); one(100); zero(n_zero)
    return M.token_batch(members)


def test_weight_zero_runs_on_both_sides_of_a_tile_border():
    seq, off = _border_batch()
    hits, start, st = _same(seq, off, 8, min_shared=1, max_cand=8, max_db_per_kmer=2, align=NO_ALIGN)
    assert st["join_pairs"] == TILE + 100 == st["kmers_joined"] and st["kmers_masked"] == 4 * 100 and st["skipped"] == len(hits) == 64
    # without the mask the same k-mers are joined: 3 items each
    hits, start, st = _same(seq, off, 8, min_shared=1, max_cand=8, max_db_per_kmer=3, align=NO_ALIGN)
    assert st["join_pairs"] == TILE + 100 + 3 * 400 and st["kmers_masked"] == 0


# ---- the cut at max_cand ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_c", [7, 8, 9, 1000])
def test_candidates_around_max_cand_with_ties_across_the_cut(n_c):
    """n_c targets share the same two k-mers with the query; the last shares a third: it is first, the smaller targets follow."""
    members = [[1, 2] for _ in range(n_c)] + [[1, 2, 3]]
    members[n_c - 1] = [1, 2, 3]
    seq, off = M.token_batch(members)
    hits, start, st = _same(seq, off, n_c, max_db_per_kmer=1000)
    assert st["candidates"] == n_c and len(hits) == min(n_c, 8)
    assert sorted(hits["target"].tolist()) == sorted([n_c - 1] + list(range(min(n_c, 8) - 1)))
    assert hits["target"][0] == n_c - 1 and hits["shared"][0] == 3


def test_max_cand_of_1_and_of_64_and_queries_at_the_wave_width():
    """Queries with exactly 63, 64 and 65 candidates: every lane of the order's wave, and the cut at 64."""
    counts = (MAX_CAND - 1, MAX_CAND, MAX_CAND + 1)
    members = [[] for _ in range(MAX_CAND + 1)]
    for k, c in enumerate(counts):
        for d in range(c):
            members[d] += [10 * k + 1, 10 * k + 2]
    for d in range(0, MAX_CAND + 1, 3):                  # every third target shares one more with each query
        members[d] += [100, 101, 102]
    members += [[10 * k + 1, 10 * k + 2, 100 + k] for k in range(3)]
    seq, off = M.token_batch(members)
    hits, start, st = _same(seq, off, MAX_CAND + 1, max_cand=MAX_CAND)
    assert np.diff(start).tolist() == [MAX_CAND - 1, MAX_CAND, MAX_CAND] and st["candidates"] == sum(counts)
    hits, start, st = _same(seq, off, MAX_CAND + 1, max_cand=1)
    assert np.diff(start).tolist() == [1, 1, 1] and hits["target"].tolist() == [0, 0, 0] and hits["shared"].tolist() == [3, 3, 3]
    _same(seq, off, MAX_CAND + 1, max_cand=MAX_CAND, align=NO_ALIGN)


# ---- thresholds, skips, ties ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_shared", [1, 2, 3])
def test_the_shared_count_at_min_shared(min_shared):
    own = [1, 2, 3, 4, 5, 6]
    seq, off = M.token_batch([own[:min_shared - 1] + [11], own[:min_shared] + [12], own[:min_shared + 1] + [13], own])
    hits, _, st = _same(seq, off, 3, min_shared=min_shared, align=dict(min_ratio_pct=0))
    assert hits["target"].tolist() == [2, 1] and st["candidates"] == 2


def test_the_ratio_test_at_its_bound():
    mat = np.full((21, 21), -3, dtype=np.int64)
    np.fill_diagonal(mat, 2)
    a, b = b"ACDEFGHIKL" + b"MMMMMMMMMM", b"ACDEFGHIKL" + b"WWWWWWWWWW"
    seq, off = S.batch([b, b + b"W" * 20, a])
    for pct, ref, want in ((50, "longer", [N.SEARCH_HIT, N.SEARCH_BELOW]), (51, "longer", [N.SEARCH_BELOW] * 2),
                           (50, "member", [N.SEARCH_HIT] * 2), (51, "member", [N.SEARCH_BELOW] * 2)):
        hits, _, _ = _same(seq, off, 2, align=dict(matrix=mat, gap_open=5, gap_extend=2, min_ratio_pct=pct, ref=ref))
        assert hits["score"].tolist() == [20, 20] and hits["target"].tolist() == [0, 1] and hits["status"].tolist() == want


def test_skipped_pairs_and_order_ties():
    rng = np.random.default_rng(31)
    p = M.random_protein(rng, 30)
    long_t = p + M.random_protein(rng, 40)
    part = p[:20] + M.random_protein(rng, 10)
    seq, off = S.batch([long_t, part, p, part, p, p, M.random_protein(rng, 30)])
    hits, start, st = _same(seq, off, 5, align=dict(max_cells=1000, min_ratio_pct=0))
    assert hits["target"][:5].tolist() == [2, 4, 1, 3, 0] and hits["status"][:5].tolist() == [0, 0, 0, 0, N.SEARCH_SKIPPED]
    assert np.diff(start).tolist() == [5, 0]
    hits, _, st = _same(seq, off, 5, align=dict(max_cells=100))
    assert st["skipped"] == 5 == len(hits) and st["queries_hit"] == 0 and hits["target"].tolist() == [0, 2, 4, 1, 3]


def test_queries_without_windows_and_empty_sides():
    rng = np.random.default_rng(32)
    p = M.random_protein(rng, 40)
    prots = [p, b"", b"ACDEFGHI", p[:8] + b"X" * 5, p, b"", b"XXXXXXXXXXXX", p[5:30]]
    seq, off = S.batch(prots)
    for n_db in (0, 1, 4, len(prots)):
        hits, start, st = _same(seq, off, n_db)
        assert len(start) == len(prots) - n_db + 1
    hits, start, st = _same(b"", np.zeros(1, dtype=np.int64), 0)
    assert len(hits) == 0 and start.tolist() == [0] and st["queries"] == 0
    _same(*S.batch([b"", b"ACD"]), 1)                    # proteins, and not one window


# ---- independence of the batch ------------------------------------------------------------------------------------------------

def test_a_querys_records_do_not_depend_on_the_other_queries():
    rng = np.random.default_rng(33)
    fam = [M.random_protein(rng, 80) for _ in range(6)]
    db = [A.mutate(rng, f, 0.08) for f in fam for _ in range(3)] + [M.random_protein(rng, 60) for _ in range(10)]
    q = A.mutate(rng, fam[2], 0.05)
    others = [M.random_protein(rng, 30) for _ in range(500)] + [A.mutate(rng, f, 0.1) for f in fam]
    alone, _, _ = _same(*S.batch(db + [q]), len(db), min_shared=1)
    assert len(alone) >= 3 and alone["status"][0] == N.SEARCH_HIT
    for at in (0, len(others), 250):
        qs = others[:at] + [q] + others[at:]
        hits, start, _ = _search(*S.batch(db + qs), len(db), min_shared=1)
        mine = hits[start[at]:start[at + 1]].copy()
        assert (mine["query"] == at).all()
        mine["query"] = 0
        assert mine.tobytes() == alone.tobytes()


def _relatives(rng, n_fam: int = 5):
    fam = [M.random_protein(rng, int(rng.integers(30, 90))) for _ in range(n_fam)]
    prots = [A.mutate(rng, fam[int(rng.integers(0, n_fam))], float(rng.choice([0.0, 0.05, 0.12, 0.25])))[int(rng.integers(0, 5)):]
             for _ in range(24)]
    prots += [M.random_protein(rng, int(rng.integers(0, 40))) for _ in range(6)] + [b"ACDEFGHIKX" * 3, b""]
    return [prots[i] for i in rng.permutation(len(prots))]


@pytest.mark.parametrize("seed", range(24))
def test_random_batches_with_planted_relatives(seed):
    rng = np.random.default_rng(100 + seed)
    prots = _relatives(rng)
    n_db = int(rng.integers(0, len(prots) + 1)) if seed % 6 else len(prots) // 2
    kw = dict(min_shared=int(rng.integers(1, 4)), max_cand=int(rng.choice([1, 2, 3, 8, 64])), max_db_per_kmer=int(rng.choice([1, 2, 4, 256])),
              align=dict(min_ratio_pct=int(rng.choice([0, 30, 50, 100])), ref=str(rng.choice(["longer", "member"])),
                         max_cells=int(rng.choice([2000, 1 << 26]))))
    _same(*S.batch(prots), n_db, **kw)


def test_the_same_call_twice_and_the_database_reversed():
    rng = np.random.default_rng(34)
    prots = _relatives(rng, 3)
    n_db = 20
    seq, off = S.batch(prots)
    first = _same(seq, off, n_db, max_cand=3)
    again = _search(seq, off, n_db, max_cand=3)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    # reversed: target d becomes n_db - 1 - d.  Only ties may change what is kept (equal s at the cut) and the order (equal
    # score and s); a query with no more candidates than max_cand keeps its set
    rseq, roff = S.batch(prots[:n_db][::-1] + prots[n_db:])
    rev = _same(rseq, roff, n_db, max_cand=3)
    s_of, _ = S.shared_numpy(seq, off, n_db)
    for q in range(len(prots) - n_db):
        if sum(1 for (qq, d), s in s_of.items() if qq == q and s >= 2) <= 3:
            a = first[0][first[1][q]:first[1][q + 1]]
            b = rev[0][rev[1][q]:rev[1][q + 1]]
            assert sorted(zip(a["target"].tolist(), a["shared"].tolist(), a["score"].tolist(), a["status"].tolist())) == \
                sorted(zip((n_db - 1 - b["target"]).tolist(), b["shared"].tolist(), b["score"].tolist(), b["status"].tolist()))


# ---- errors, limits, allocations, the device entry point ----------------------------------------------------------------------

def _raw(seq, off, n_db, prm=(2, 8, 256, 0), al=(50, 0, 11, 1, 1 << 26, None, 0), max_windows=0, max_pairs=0, null=()):
    lib = N.load()
    h = C.c_void_p()
    arr = np.frombuffer(bytes(seq), dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    p, a = N.KgSearchParams(*prm), N.KgAlignParams(*al)
    rc = lib.kg_proteins_search(0, None if "params" in null else C.byref(p), None if "align" in null else C.byref(a),
                                None if "seq" in null or not arr.size else arr.ctypes.data, None if "offsets" in null else off.ctypes.data,
                                len(off) - 1, n_db, max_windows, max_pairs, None if "out" in null else C.byref(h))
    msg = lib.kg_last_error().decode()
    if h.value:
        lib.kg_hitset_free(h)
    return rc, msg


def test_every_error_with_its_first_words():
    seq, off = S.batch([b"ACDEFGHIKLMN", b"ACDEFGHIKLMN"])
    dec = np.array([0, 12, 5], dtype=np.int64)
    cases = [
        (dict(null=("out",)), N.KG_ERR_ARG, "null argument"),
        (dict(null=("params",)), N.KG_ERR_ARG, "null kg_search_params"),
        (dict(prm=(0, 8, 256, 0)), N.KG_ERR_ARG, "min_shared must be >= 1"),
        (dict(prm=(2, 0, 256, 0)), N.KG_ERR_ARG, "max_cand must be in 1..64"),
        (dict(prm=(2, 65, 256, 0)), N.KG_ERR_ARG, "max_cand must be in 1..64"),
        (dict(prm=(2, 8, 0, 0)), N.KG_ERR_ARG, "max_db_per_kmer must be >= 1"),
        (dict(prm=(2, 8, 256, 1)), N.KG_ERR_ARG, "kg_search_params.reserved must be 0"),
        (dict(null=("align",)), N.KG_ERR_ARG, "null kg_align_params"),
        (dict(al=(101, 0, 11, 1, 1 << 26, None, 0)), N.KG_ERR_ARG, "min_ratio_pct must be in 0..100"),
        (dict(al=(50, 2, 11, 1, 1 << 26, None, 0)), N.KG_ERR_ARG, "ref must be"),
        (dict(al=(50, 0, 11, 0, 1 << 26, None, 0)), N.KG_ERR_ARG, "gap_extend must be >= 1"),
        (dict(al=(50, 0, 11, 1, 0, None, 0)), N.KG_ERR_ARG, "max_cells must be >= 1"),
        (dict(max_windows=-1), N.KG_ERR_ARG, "max_windows must be >= 0"),
        (dict(max_pairs=-1), N.KG_ERR_ARG, "max_pairs must be >= 0"),
        (dict(n_db=-1), N.KG_ERR_ARG, "n_db must be in 0..n_prot"),
        (dict(n_db=3), N.KG_ERR_ARG, "n_db must be in 0..n_prot"),
        (dict(null=("offsets",)), N.KG_ERR_ARG, "null offsets"),
        (dict(off=dec), N.KG_ERR_ARG, "protein 1: offsets decrease"),
        (dict(off=np.array([0, 1 << 24, (1 << 24) + 3], dtype=np.int64), null=("seq",)), N.KG_ERR_LIMIT, "protein 0: 2^24 or more characters"),
        (dict(null=("seq",)), N.KG_ERR_ARG, "null sequence"),
    ]
    for kw, code, words in cases:
        kw = dict(kw)
        rc, msg = _raw(seq, kw.pop("off", off), kw.pop("n_db", 1), **kw)
        assert rc == code and msg.startswith(words), (kw, rc, msg)
    lib = N.load()
    assert lib.kg_hitset_count(None) == 0 and lib.kg_hitset_copy(None, 0, 0, None) == N.KG_ERR_ARG
    assert lib.kg_hitset_starts_copy(None, None) == N.KG_ERR_ARG and lib.kg_hitset_stats(None, None) == N.KG_ERR_ARG
    lib.kg_hitset_free(None)


def test_max_pairs_and_max_windows_one_below_and_at_the_need():
    rng = np.random.default_rng(35)
    seq, off = S.batch(_relatives(rng))
    want, wstart, wst = _model(seq, off, 16)
    assert wst["join_pairs"] > 10
    hits, start, st = _search(seq, off, 16, max_pairs=wst["join_pairs"], max_windows=wst["valid_windows"])
    assert hits.tobytes() == want.tobytes()
    with pytest.raises(N.KmerGutsNativeError) as ei:
        _search(seq, off, 16, max_pairs=wst["join_pairs"] - 1)
    assert ei.value.code == N.KG_ERR_LIMIT and str(ei.value).find("%d join pairs do not fit this call, which holds %d (max_pairs)" % (
        wst["join_pairs"], wst["join_pairs"] - 1)) >= 0 and "max_db_per_kmer" in str(ei.value)
    with pytest.raises(N.KmerGutsNativeError) as ei:
        _search(seq, off, 16, max_windows=wst["valid_windows"] - 1)
    assert ei.value.code == N.KG_ERR_LIMIT and "%d valid windows do not fit" % wst["valid_windows"] in str(ei.value)


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    import torch
    from kmergutsjava_amd import hotpath, synth
    seq, off = S.batch(_relatives(np.random.default_rng(36)))
    want, wstart, _ = _model(seq, off, 16)
    assert len(want) > 4
    rec = synth.high_density_config(4, 100, 4001, 500, dna=False)[2]
    with hotpath.SignatureTable.from_bytes(synth.table_image(rec), 0) as tab:
        assert _search(seq, off, 16)[0].tobytes() == want.tobytes()
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        failed = 0
        for n in range(1, 600):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got = _search(seq, off, 16)
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
                assert tab.live_device_bytes() == live0
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= 60 and got[0].tobytes() == want.tobytes() and got[1].tobytes() == wstart.tobytes()
        assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0


def test_the_device_sequence_entry_point():
    import torch
    seq, off = S.batch(_relatives(np.random.default_rng(37)))
    want = _same(seq, off, 12)
    dev = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    got = _search(None, off, 12, device_ptr=dev.data_ptr())
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert {k: got[2][k] for k in S.STAT_KEYS} == {k: want[2][k] for k in S.STAT_KEYS}


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def test_end_to_end_with_transfer_and_truth(tmp_path):
    """The golden E. coli proteome as the database, 200 of its proteins with a substitution at every 12th residue as the queries,
    synthetic annotations (a function per sequence: the file holds some sequences under several ids, and the first of them is
    the rank-0 target); the --transfer file goes into make_signatures -A."""
    import zlib
    from kmergutsjava_amd.make_signatures import _read, parse_fasta
    faa = os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz")
    ids, seqs = parse_fasta(_read(faa), faa)
    pick = [k for k in range(0, len(ids), len(ids) // 200) if len(seqs[k]) >= 60][:200]
    alpha = A.ALPHA

    def sub(p):
        return bytes(alpha[(alpha.index(ch) + 3) % 20] if i % 12 == 6 and ch in alpha else ch for i, ch in enumerate(p))

    (tmp_path / "q.faa").write_bytes(b"".join(b">m_%s\n%s\n" % (ids[k], sub(seqs[k])) for k in pick))
    (tmp_path / "ann.tsv").write_bytes(b"".join(b"%s\tfunction %d\n" % (pid, zlib.crc32(seqs[k]) % 300) for k, pid in enumerate(ids)))
    (tmp_path / "truth.tsv").write_bytes(b"".join(b"m_%s\tfunction %d\n" % (ids[k], zlib.crc32(seqs[k]) % 300) for k in pick))
    out, tr = tmp_path / "hits.tsv", tmp_path / "transfer.tsv"
    r = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.search_proteins", "-d", faa, "-q", str(tmp_path / "q.faa"), "-o", str(out),
                        "-A", str(tmp_path / "ann.tsv"), "--transfer", str(tr), "--truth", str(tmp_path / "truth.tsv")],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = r.stderr.strip().splitlines()[-1]
    m = re.search(r"Queries: (\d+), targets: (\d+), .*queries hit: (\d+), transferred: (\d+), .*labelled: (\d+), agree: (\d+), disagree: (\d+), missed: (\d+)", line)
    assert m, line
    n_q, n_t, q_hit, moved, labelled, agree, disagree, missed = map(int, m.groups())
    assert (n_q, n_t, labelled) == (len(pick), len(ids), len(pick)) and moved == q_hit and agree + disagree + missed == labelled
    assert agree >= 0.9 * len(pick)                      # eleven residues between substitutions: 8-mers survive, 11 in 12 identical
    rows = [x.split(b"\t") for x in out.read_bytes().splitlines()]
    assert len(rows) == q_hit and all(len(x) == 11 and x[1] == b"0" and x[9] == b"hit" for x in rows)
    seq_of = dict(zip(ids, seqs))
    assert sum(seq_of[x[0][2:]] == seq_of[x[2]] for x in rows) >= 0.9 * len(pick)
    sig = tmp_path / "sigs.txt"
    r = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.make_signatures", "-p", str(tmp_path / "q.faa"), "-A", str(tr), "-o", str(sig)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
