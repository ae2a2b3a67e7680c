"""kg_searchdb on the GPU: a search against a resident index gives, byte for byte, what the one-batch call gives on "the targets,
then these queries" with the same options: records, hit_start, the count fields of the statistics and, where asked for, paths,
ops, ungapped records and band statistics.  The small cases are also compared with search_model.  The border cases are derived
from the constants of kg_search.hpp (the join tile is the one-batch join's; the probe has no stride of its own: its search is
over the whole k-mer array); cluster_model.token_batch gives proteins whose k-mer sets are chosen one by one."""
import gzip
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import cluster_model as M
import mask_model as MK
import search_model as S
import searchdb_model as DM
from kmergutsjava_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TEXT = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_search.hpp")).read()
TILE = int(re.search(r"constexpr int kSearchTile = (\d+);", _TEXT).group(1))
NO_ALIGN = dict(max_cells=1)            # every pair skipped: the order is (s, target) and the model aligns nothing
MASK = dict(window=12, trigger=563, extend=640)


def _db(seq, off, n_db, **kw):
    from kmergutsjava_amd import hotpath
    off = np.asarray(off, dtype=np.int64)
    return hotpath.SearchDb.build(seq, off[:n_db + 1], **kw)


def _counts(st: dict) -> dict:
    """The statistics without the times and the probe's own block, nested blocks included."""
    return {k: (_counts(v) if isinstance(v, dict) else v) for k, v in st.items() if not k.startswith("ms_") and k != "db"}


def _stats(got):
    return next(x for x in got if isinstance(x, dict))


def _equal(one, got):
    assert len(one) == len(got)
    for a, b in zip(one, got):
        if isinstance(a, dict):
            assert _counts(a) == _counts(b)
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _split(mask):
    """mask= of the one-batch call -> (the build's mask, the search's mask)."""
    if mask is None:
        return None, None
    m = {k: v for k, v in mask.items() if k != "sides"}
    sides = mask.get("sides", "both")
    return (m if sides in ("both", "targets") else None), (m if sides in ("both", "queries") else None)


def _same(seq, off, n_db, db=None, model=False, **kw):
    """The resident call against the one-batch call on the same batch (and, with model, against search_model); -> the resident
    call's result.  db: a handle to search (else one is built for the call); seeds and mask are split between build and search."""
    from kmergutsjava_amd import hotpath
    off = np.asarray(off, dtype=np.int64)
    one = hotpath.search_proteins(seq, off, n_db, **kw)
    skw = dict(kw)
    seeds, mask = skw.pop("seeds", None), skw.pop("mask", None)
    tmask, qmask = _split(mask)
    own = db is None
    if own:
        db = _db(seq, off, n_db, seeds=seeds, mask=tmask)
    try:
        got = db.search(seq, off[n_db:], mask=qmask, **skw)
    finally:
        if own:
            db.close()
    _equal(one, got)
    if model:
        d = _stats(got)
        mkw = dict(kw)
        mkw.update(mkw.pop("align", None) or {})
        want, wstart, wst = S.search_model(seq, off, n_db, **mkw)
        assert got[0].tobytes() == want.tobytes() and got[1].tobytes() == wstart.tobytes()
        assert {k: d[k] for k in S.STAT_KEYS} == wst
    return got


# ---- the probe at its borders -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k_db", [0, 1, 2, 63, 64, 65, 255, 256, 257])
def test_query_kmers_below_at_between_and_above_the_database_s(k_db):
    """The targets hold the k-mers 2, 4 .. 2 k_db; the queries one k-mer each: below the first, the first, between two, the
    last, above the last, and, all in one query, each of them."""
    t_members = [[2 * (i + 1) for i in range(k_db) if i % 3 == d] for d in range(3)]
    probes = [1, 2, 3, 2 * k_db, 2 * k_db + 1]
    q_members = [[v] for v in probes] + [sorted(set(probes))]
    seq, off = M.token_batch(t_members + q_members)
    got = _same(seq, off, 3, model=True, min_shared=1, align=NO_ALIGN)
    st = _stats(got)
    present = {v for v in probes if v % 2 == 0 and 2 <= v <= 2 * k_db}
    assert st["db"]["query_kmers"] == len(set(probes)) and st["db"]["found"] == len(present) == st["kmers_joined"]
    assert st["kmers"] == k_db + len(set(probes)) - len(present)
    assert np.diff(got[1]).tolist() == [int(v in present) for v in probes] + [len({(v // 2 - 1) % 3 for v in present})]


def test_all_query_kmers_absent_all_present_and_empty_sides():
    rng = np.random.default_rng(32)
    evens, odds = [2 * i for i in range(1, 400)], [2 * i + 1 for i in range(1, 400)]
    t = [evens[d::4] for d in range(4)]
    seq, off = M.token_batch(t + [odds[q::3] for q in range(3)])
    st = _stats(_same(seq, off, 4, model=True, min_shared=1))
    assert st["db"]["found"] == 0 == st["join_pairs"] and st["db"]["query_kmers"] == len(odds)
    seq, off = M.token_batch(t + [evens[q::3] for q in range(3)])
    st = _stats(_same(seq, off, 4, model=True, min_shared=1, align=NO_ALIGN))
    assert st["db"]["found"] == len(evens) == st["db"]["query_kmers"] == st["kmers"] == st["kmers_joined"]
    # queries without a window among queries with one; no queries; no targets; targets without a window
    p = M.random_protein(rng, 40)
    seq, off = S.batch([p, M.random_protein(rng, 30), b"", b"ACDEFGH", p, b"X" * 20, p[5:]])
    got = _same(seq, off, 2, model=True)
    assert np.diff(got[1]).tolist() == [0, 0, 1, 0, 1]
    _same(seq, off, 7, model=True)
    _same(seq, off, 0, model=True)
    seq, off = S.batch([b"", b"ACDEFGHI", p, p])
    st = _stats(_same(seq, off, 2, model=True))
    assert st["kmers"] == st["db"]["query_kmers"] == 32 and st["db"]["found"] == 0


# ---- the join at its borders, through the two-source kernels ----------------------------------------------------------------------------

@pytest.mark.parametrize("n_t", [1, 2, 63, 64, 65, 257])
def test_one_kmer_in_many_targets_and_queries(n_t):
    """One k-mer shared by n_t targets and 1, 63, 64, 65 queries; the mask at the target count, one below and one above; a second
    k-mer that only targets have, n_t of them, is masked with it and counted though no query has it."""
    for n_q in (1, 63, 64, 65):
        seq, off = M.token_batch([[5, 9]] * n_t + [[5]] * n_q)
        with _db(seq, off, n_t) as db:
            for mask in (n_t - 1, n_t, n_t + 1):
                if mask < 1:
                    continue
                got = _same(seq, off, n_t, db=db, model=n_q == 1, min_shared=1, max_db_per_kmer=mask)
                st = _stats(got)
                assert st["join_pairs"] == (n_t * n_q if mask >= n_t else 0) and st["kmers_masked"] == 2 * (mask < n_t)
                assert len(got[0]) == (min(n_t, 8) * n_q if mask >= n_t else 0)


def _factor(n: int):
    nd = max(d for d in range(1, 257) if n % d == 0)
    return nd, n // nd


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_join_pairs_of_a_tile_and_one_more_or_less(extra):
    nd, nq = _factor(TILE + extra)
    seq, off = M.token_batch([[7]] * (nd + nq))
    for ungapped in (None, True):
        got = _same(seq, off, nd, min_shared=1, max_cand=2, ungapped=ungapped)
        assert _stats(got)["join_pairs"] == TILE + extra and len(got[0]) == nq * min(nd, 2)


def test_one_run_over_three_tiles():
    nq = 2 * TILE // 100 + 2
    members = [[2, 1] if d == 0 else [2] for d in range(100)] + [[2, 1] if q < 3 else [2] for q in range(nq)]
    members[99] = [2, 3]
    members[100 + nq - 1] = [2, 3]
    seq, off = M.token_batch(members)
    for ungapped in (None, True):
        got = _same(seq, off, 100, min_shared=1, max_cand=3, ungapped=ungapped)
        st = _stats(got)
        assert st["join_pairs"] == 3 + 100 * nq + 1 > 2 * TILE + 3 and st["kmers_joined"] == 3


def _border_batch(n_zero: int = 300):
    """test_gpu_search's: 8 targets and 8 queries, weight-0 runs (target-only, query-only and masked in turn) in front, inside a
    tile, on the tile border and behind the last item."""
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
    with _db(seq, off, 8) as db:
        got = _same(seq, off, 8, db=db, model=True, min_shared=1, max_cand=8, max_db_per_kmer=2, align=NO_ALIGN)
        st = _stats(got)
        assert st["join_pairs"] == TILE + 100 == st["kmers_joined"] and st["kmers_masked"] == 4 * 100 and len(got[0]) == 64
        st = _stats(_same(seq, off, 8, db=db, min_shared=1, max_cand=8, max_db_per_kmer=3, align=NO_ALIGN))
        assert st["join_pairs"] == TILE + 100 + 3 * 400 and st["kmers_masked"] == 0
        _same(seq, off, 8, db=db, min_shared=1, max_cand=8, max_db_per_kmer=2, ungapped=True)


def test_max_pairs_and_max_windows_at_the_need_and_one_below():
    from kmergutsjava_amd import hotpath
    seq, off = M.token_batch([[1, 2, 3]] * 5 + [[1, 2], [3], [4]])
    off = np.asarray(off, dtype=np.int64)
    with _db(seq, off, 5) as db:
        got = _same(seq, off, 5, db=db, min_shared=1, max_pairs=15)
        assert _stats(got)["join_pairs"] == 15
        _equal(got, db.search(seq, off[5:], min_shared=1, max_pairs=15, max_windows=4))
        with pytest.raises(N.KmerGutsNativeError) as e:
            db.search(seq, off[5:], min_shared=1, max_pairs=14)
        with pytest.raises(N.KmerGutsNativeError) as e1:
            hotpath.search_proteins(seq, off, 5, min_shared=1, max_pairs=14)
        assert e.value.code == N.KG_ERR_LIMIT == e1.value.code and str(e.value) == str(e1.value)
        assert "15 join pairs do not fit this call, which holds 14 (max_pairs)" in str(e.value)
        # the windows of a resident call are the queries' alone: 4
        with pytest.raises(N.KmerGutsNativeError) as e:
            db.search(seq, off[5:], min_shared=1, max_windows=3)
        assert e.value.code == N.KG_ERR_LIMIT
        assert "4 valid windows do not fit the one pass of this call, which holds 3 (max_windows)" in str(e.value)
        _same(seq, off, 5, db=db, min_shared=1)                 # the handle answers after the refusals
    with pytest.raises(N.KmerGutsNativeError) as e:
        hotpath.SearchDb.build(seq, off[:6], max_windows=14)
    assert e.value.code == N.KG_ERR_LIMIT and "15 valid windows do not fit the one pass of this call, which holds 14 (max_windows)" in str(e.value)


# ---- every option once, and the full stack ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    prots, n_db = MK.planted_search(seed=41, n_targets=40, n_related=20, length=150)
    seq, off = S.batch(prots)
    return seq, np.asarray(off, dtype=np.int64), n_db


@pytest.mark.parametrize("kw", [
    dict(),
    dict(seeds="reduced"),
    dict(mask=dict(MASK, sides="targets")), dict(mask=dict(MASK, sides="queries")), dict(mask=dict(MASK, sides="both")),
    dict(ungapped=True), dict(ungapped={"min_score": 40}),
    dict(ungapped=True, band=0), dict(ungapped=True, band=8), dict(ungapped=True, band=256),
    dict(paths="hits", ops="m"), dict(paths="all", ops="eqx"), dict(paths="all"),
    dict(seeds="reduced", mask=dict(MASK, sides="both"), ungapped={"min_score": 40}, band=8, paths="all", ops="eqx"),
], ids=lambda kw: "+".join("%s=%s" % (k, v.get("sides", v.get("min_score", "")) if isinstance(v, dict) else v) for k, v in kw.items()) or "plain")
def test_every_option_on_a_planted_batch(planted, kw):
    seq, off, n_db = planted
    got = _same(seq, off, n_db, **kw)
    assert len(got[0]) > 0 and _stats(got)["hits"] >= 10


# ---- independence --------------------------------------------------------------------------------------------------------------------

def test_a_query_alone_first_last_among_others_and_the_batch_in_pieces(planted):
    seq, off, n_db = planted
    rng = np.random.default_rng(5)
    prots = [bytes(seq[off[k]:off[k + 1]]) for k in range(len(off) - 1)]
    targets, queries = prots[:n_db], prots[n_db:]
    others = [MK.mutate(rng, targets[int(rng.integers(0, n_db))], 0.2) for _ in range(500)]
    tseq, toff = S.batch(targets)
    kw = dict(ungapped=True, band=16, paths="all", ops="m")
    with _db(tseq, toff, n_db) as db, _db(tseq, toff, n_db) as db2:          # two handles alive at once
        def run(qs, handle=db):
            qseq, qoff = S.batch(qs)
            return handle.search(qseq, qoff, **kw)

        q = queries[3]
        alone = run([q])
        assert len(alone[0]) > 0
        for qs, at in (([q] + others, 0), (others + [q], 500), (others[:250] + [q] + others[250:], 250)):
            got = run(qs)
            lo, hi = int(got[1][at]), int(got[1][at + 1])
            rec = got[0][lo:hi].copy()
            assert (rec["query"] == at).all()
            rec["query"] = 0
            assert rec.tobytes() == alone[0].tobytes() and got[2][lo:hi].tobytes() == alone[2].tobytes()
            assert got[-1][lo:hi].tobytes() == alone[-1].tobytes()                   # the ungapped records
            ops_lo, ops_hi = int(got[4][lo]), int(got[4][hi])
            assert got[5][ops_lo:ops_hi].tobytes() == alone[5].tobytes()
        # the same queries in one call and in three, on either handle; and the same call twice
        whole = run(queries)
        _equal(whole, run(queries))
        cuts = [0, 7, 8, len(queries)]
        parts = [run(queries[a:b], handle=db2) for a, b in zip(cuts, cuts[1:])]
        recs = []
        for (a, _), part in zip(zip(cuts, cuts[1:]), parts):
            r = part[0].copy()
            r["query"] += a
            recs.append(r)
        assert np.concatenate(recs).tobytes() == whole[0].tobytes()
        assert np.concatenate([part[2] for part in parts]).tobytes() == whole[2].tobytes()
        assert np.concatenate([part[5] for part in parts]).tobytes() == whole[5].tobytes()
        assert sum(_stats(part)["hits"] for part in parts) == _stats(whole)["hits"]


# ---- persistence ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeds,mask", [(None, None), ("reduced", MASK)], ids=["exact", "reduced+mask"])
def test_build_save_open_search_and_the_file_s_bytes(planted, tmp_path, seeds, mask):
    from kmergutsjava_amd import hotpath, seeds as SDS
    seq, off, n_db = planted
    names = b"\n".join(b"t%d" % k for k in range(n_db))
    path, again = str(tmp_path / "db.kgsdb"), str(tmp_path / "again.kgsdb")
    kw = dict(ungapped=True, band=8, paths="all", ops="m", mask=mask)
    with hotpath.SearchDb.build(seq, off[:n_db + 1], seeds=seeds, mask=mask, names=names) as db:
        built = db.search(seq, off[n_db:], **kw)
        info = db.info()
        db.save(path)
    data = open(path, "rb").read()
    seed = None
    if seeds is not None:
        cls, _, masks = SDS.resolve(seeds)[:3]
        seed = (list(cls), list(masks))
    assert data == DM.write(bytes(seq), off[:n_db + 1], seed=seed, mask=mask, names=names)
    with hotpath.SearchDb.open(path) as db:
        assert db.names() == names
        opened = db.info()
        for k in ("targets", "residues", "pairs", "kmers", "valid_windows", "names_bytes", "seeds", "mask", "query_room"):
            assert opened[k] == info[k], k
        assert opened["mask_stats"] is None or _counts(opened["mask_stats"]) == _counts(info["mask_stats"])
        _equal(built, db.search(seq, off[n_db:], **kw))
        db.save(again)
    assert open(again, "rb").read() == data


def test_small_files_against_the_model(tmp_path):
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(77)
    path = str(tmp_path / "db.kgsdb")
    for prots in ([], [b""], [b"ACDEFGHIK"], MK.low_complexity_batch(rng, 30), [M.random_protein(rng, 200)] * 3):
        seq, off = S.batch(prots) if prots else (b"", np.zeros(1, dtype=np.int64))
        for mask in (None, MASK):
            with hotpath.SearchDb.build(seq, off, mask=mask, names=b"n") as db:
                db.save(path)
            assert open(path, "rb").read() == DM.write(bytes(seq), off, mask=mask, names=b"n")


# ---- hygiene -------------------------------------------------------------------------------------------------------------------------

def test_every_allocation_failed_in_turn(planted, tmp_path, monkeypatch):
    import torch
    from kmergutsjava_amd import hotpath
    seq, off, n_db = planted
    path = str(tmp_path / "db.kgsdb")
    kw = dict(ungapped=True, band=8, paths="hits", ops="m", mask=MASK)

    def fail_in_turn(call, after_failure, at_least):
        failed = 0
        for n in range(1, 900):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got = call()
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                after_failure(n)
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= at_least
        return got

    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]

    def nothing_live(n):
        assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n

    db = fail_in_turn(lambda: hotpath.SearchDb.build(seq, off[:n_db + 1], mask=MASK), nothing_live, 20)
    with db:
        want = db.search(seq, off[n_db:], **kw)
        db.save(path)
        live0, free1 = db.live_device_bytes(), torch.cuda.mem_get_info()[0]
        assert live0 == db.info()["device_bytes"] > 0

        def handle_as_it_was(n):
            assert db.live_device_bytes() == live0 and torch.cuda.mem_get_info()[0] == free1

        got = fail_in_turn(lambda: db.search(seq, off[n_db:], **kw), handle_as_it_was, 80)
        _equal(want, got)
        handle_as_it_was(0)
        _equal(want, db.search(seq, off[n_db:], **kw))
    assert torch.cuda.mem_get_info()[0] == free0
    db = fail_in_turn(lambda: hotpath.SearchDb.open(path), nothing_live, 6)
    with db:
        _equal(want, db.search(seq, off[n_db:], **kw))
    assert torch.cuda.mem_get_info()[0] == free0


def test_a_batch_over_the_room_and_reserve(planted):
    from kmergutsjava_amd import hotpath
    seq, off, n_db = planted
    need = int(off[-1] - off[n_db])
    with hotpath.SearchDb.build(seq, off[:n_db + 1], query_room=need - 1) as db:
        assert db.info()["query_room"] == need - 1
        with pytest.raises(N.KmerGutsNativeError) as e:
            db.search(seq, off[n_db:])
        assert e.value.code == N.KG_ERR_LIMIT
        assert "%d residues of queries do not fit the room of %d residues" % (need, need - 1) in str(e.value)
        live = db.live_device_bytes()
        db.reserve(need)
        assert db.info()["query_room"] == need and db.live_device_bytes() >= live
        _equal(hotpath.search_proteins(seq, off, n_db), db.search(seq, off[n_db:]))
        db.reserve(10)                                          # never shrinks
        assert db.info()["query_room"] == need


def test_a_second_call_on_a_held_handle_is_busy_and_a_closed_handle_is_refused(planted, monkeypatch):
    """KG_ERR_BUSY without a race: under KG_TEST_SEARCHDB_REENTER a search that holds the handle calls kg_searchdb_reserve on it
    and returns that call's answer.  A second thread meeting a call in flight cannot be arranged without a sleep at these sizes."""
    from kmergutsjava_amd import hotpath
    seq, off, n_db = planted
    with hotpath.SearchDb.build(seq, off[:n_db + 1]) as db:
        want = db.search(seq, off[n_db:])
        live = db.live_device_bytes()
        monkeypatch.setenv("KG_TEST_SEARCHDB_REENTER", "1")
        with pytest.raises(N.KmerGutsNativeError) as e:
            db.search(seq, off[n_db:])
        monkeypatch.delenv("KG_TEST_SEARCHDB_REENTER")
        assert e.value.code == N.KG_ERR_BUSY and "another call is in flight on this kg_searchdb" in str(e.value)
        assert db.live_device_bytes() == live
        out = []
        th = threading.Thread(target=lambda: out.append(db.search(seq, off[n_db:])))       # the flag is free again, from any thread
        th.start()
        th.join()
        _equal(want, out[0])
    with pytest.raises(ValueError):
        db.search(seq, off[n_db:])


def test_more_queries_than_the_offsets_room_and_reserve_with_allocations_failing(planted, monkeypatch):
    """1500 queries are more than the 1024 whose offsets fit behind the targets': the larger block becomes the handle's only when
    the call succeeds, so after every failed call the live bytes are what they were.  The same for kg_searchdb_reserve."""
    import torch
    from kmergutsjava_amd import hotpath
    seq, off, n_db = planted
    rng = np.random.default_rng(8)
    prots = [bytes(seq[off[k]:off[k + 1]]) for k in range(len(off) - 1)]
    queries = [MK.mutate(rng, prots[int(rng.integers(0, n_db))], 0.1)[:60] for _ in range(1500)]
    bseq, boff = S.batch(prots[:n_db] + queries)
    boff = np.asarray(boff, dtype=np.int64)
    one = hotpath.search_proteins(bseq, boff, n_db)
    with hotpath.SearchDb.build(seq, off[:n_db + 1], query_room=60 * 1500) as db:
        torch.cuda.synchronize()
        live, free = db.live_device_bytes(), torch.cuda.mem_get_info()[0]
        failed = 0
        for n in range(1, 900):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got = db.search(bseq, boff[n_db:])
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert db.live_device_bytes() == live and torch.cuda.mem_get_info()[0] == free, n
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= 30
        _equal(one, got)
        grown = db.live_device_bytes()
        assert grown > live                                     # the offsets' room has grown, once
        _equal(one, db.search(bseq, boff[n_db:]))
        assert db.live_device_bytes() == grown
        # reserve: its one allocation failed, then not
        monkeypatch.setenv("KG_TEST_FAIL_ALLOC", "1")
        with pytest.raises(N.KmerGutsNativeError) as e:
            db.reserve(1 << 22)
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert e.value.code == N.KG_ERR_NOMEM and db.live_device_bytes() == grown and db.info()["query_room"] == 60 * 1500
        db.reserve(1 << 22)
        assert db.info()["query_room"] == 1 << 22 and db.live_device_bytes() > grown
        _equal(one, db.search(bseq, boff[n_db:]))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def test_make_search_db_and_search_proteins_db_on_the_golden_proteome_in_three_batches(tmp_path):
    """make_search_db on the golden proteome file, then search_proteins --db as a subprocess: 192 of its proteins with a
    substitution at every 12th residue, in three batches, with the ungapped stage, a band of 32, paths, CIGARs, alignments and
    the transfer file.  The bytes are those of the -d run on the same FASTA files."""
    from kmergutsjava_amd import search_proteins as SP
    from kmergutsjava_amd.make_signatures import parse_fasta
    golden = os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz")
    ids, prots = parse_fasta(gzip.decompress(open(golden, "rb").read()))
    prots = [bytes(p) for p in prots]
    pick = [k for k in range(0, len(ids), len(ids) // 400) if 60 <= len(prots[k]) <= 400][:192]
    assert len(pick) == 192
    alpha = b"ACDEFGHIKLMNPQRSTVWY"
    queries = []
    for k in pick:
        p = bytearray(prots[k])
        for i in range(0, len(p), 12):
            p[i] = alpha[(alpha.find(bytes([p[i]])) + 7) % 20]
        queries.append(bytes(p))
    qfa, ann, db = tmp_path / "q.faa", tmp_path / "ann.tsv", tmp_path / "golden.kgsdb"
    qfa.write_bytes(b"".join(b">q%d\n%s\n" % (k, q) for k, q in enumerate(queries)))
    ann.write_bytes(b"".join(b"%s\tfunction %d\n" % (i, k % 97) for k, i in enumerate(ids) if k % 5))
    batch = sum(len(q) for q in queries) // 3 + 200
    assert len(SP.batch_cuts([len(q) for q in queries], batch)) == 4
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(module, *args):
        done = subprocess.run([sys.executable, "-m", "kmergutsjava_amd." + module] + [str(a) for a in args], env=env, cwd=str(tmp_path),
                              capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        return done.stderr

    made = run("make_search_db", "-d", golden, "-o", db, "-A", ann)
    assert "Targets: %d, residues: " % len(ids) in made
    options = ["--ungapped", "--band", "32", "--paths", "--cigar"]
    files = {}
    for tag, where in (("d", ["-d", golden, "-A", ann]), ("db", ["--db", db, "--batch-residues", batch])):
        names = {k: tmp_path / ("%s.%s" % (tag, k)) for k in ("o", "transfer", "alignments")}
        line = run("search_proteins", *where, "-q", qfa, "-o", names["o"], "--transfer", names["transfer"], "--alignments", names["alignments"],
                   *options)
        files[tag] = (tuple(names[k].read_bytes() for k in ("o", "transfer", "alignments")), line)
        assert ("db: index (%d targets)" % len(ids) in line) == (tag == "db")
    assert files["db"][0] == files["d"][0] and all(len(x) > 1000 for x in files["d"][0])
    assert files["d"][0][0].count(b"\n") >= 180
