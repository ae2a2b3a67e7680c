"""kg_proteins_cluster_aligned on the device against tests/align_model.py's cluster_aligned_model: the family records, the edge
records and the counts, byte for byte (include/kmerguts_hip.h states the rule)."""
import ctypes as C

import numpy as np
import pytest

import align_model as A
import cluster_model as M
from kmergutsjava_amd import _native as N

pytestmark = pytest.mark.gpu
ALIGN_COUNTS = ("aligned", "cut", "skipped", "cells")


def _cluster(seq, off, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.cluster_proteins(seq, off, **kw)


def _same(prots, min_shared=5, min_cover_pct=20, **align):
    seq, off = M.pack(prots) if isinstance(prots, list) else prots
    got, st = _cluster(seq, off, min_shared=min_shared, min_cover_pct=min_cover_pct, align=align)
    want, counts, edges, ast = A.cluster_aligned_model(seq, off, min_shared, min_cover_pct, **align)
    assert {k: st[k] for k in M.COUNTS} == counts
    assert {k: st["align"][k] for k in ALIGN_COUNTS} == ast
    assert st["edge_records"].tobytes() == edges.tobytes()
    assert got.tobytes() == want.tobytes()
    return got, st


def test_the_domain_chain():
    prots = A.domain_chain(np.random.default_rng(5))
    seq, off = M.pack(prots)
    own = [A.self_score(p) for p in prots]
    for m in (1, 2):                                            # the three numbers of each member, on the CPU
        score = A.sw_numpy(prots[m], prots[0])[0]
        assert 100 * score < 45 * own[0] and 100 * score > 80 * own[m] and A.links(seq, off)[0][(m, 0)] >= 5
    plain, st = _cluster(seq, off)
    assert st["families"] == 1 and st["largest"] == 3 and plain["best"].tolist() == [-1, 0, 0]
    got, st = _same(prots)
    assert st["families"] == 3 and st["edges"] == 0 and st["links"] == 2 and st["align"]["cut"] == 2
    assert got["best"].tolist() == [-1, -1, -1] and got["shared"].tolist() == [0, 0, 0]
    assert st["edge_records"]["status"].tolist() == [N.EDGE_CUT] * 2
    got, st = _same(prots, ref="member")
    assert st["families"] == 1 and st["align"]["cut"] == 0 and got.tobytes() == plain.tobytes()
    got, st = _same(prots, min_ratio_pct=0)                     # any positive score keeps the edge
    assert st["families"] == 1


def test_six_mutated_copies_stay_one_family():
    rng = np.random.default_rng(6)
    base = M.random_protein(rng, 250)
    prots = [base] + [A.mutate(rng, base, 0.06) for _ in range(5)] + [M.random_protein(rng, 250)]
    got, st = _same(prots)
    assert st["families"] == 2 and st["largest"] == 6 and st["align"]["cut"] == 0 and st["align"]["aligned"] >= 5
    assert M.partition(got) == {frozenset(range(6)), frozenset([6])}


def test_best_is_made_after_the_cut():
    prots = A.two_centres(np.random.default_rng(7))
    seq, off = M.pack(prots)
    plain, _ = _cluster(seq, off)
    assert plain["best"][2] == 0 and M.partition(plain) == {frozenset([0, 1, 2])}
    got, st = _same(prots)
    e = st["edge_records"]
    assert e["member"].tolist() == [2, 2] and e["centre"].tolist() == [0, 1] and e["status"].tolist() == [N.EDGE_CUT, N.EDGE_KEPT]
    assert e["shared"][0] > e["shared"][1] and got["best"][2] == 1 and got["shared"][2] == e["shared"][1]
    assert M.partition(got) == {frozenset([0]), frozenset([1, 2])}


def test_a_skipped_edge_is_kept():
    prots = A.domain_chain(np.random.default_rng(5))
    got, st = _same(prots, max_cells=120 * 270 - 1)
    assert st["edge_records"]["status"].tolist() == [N.EDGE_SKIPPED] * 2 and st["edge_records"]["score"].tolist() == [-1, -1]
    assert st["families"] == 1 and st["edges"] == 2 and st["align"] | dict(ms_align=0) == dict(aligned=0, cut=0, skipped=2, cells=0, ms_align=0)
    assert got["best"].tolist() == [-1, 0, 0]
    got, st = _same(prots, max_cells=120 * 270)
    assert st["families"] == 3


def test_a_path_with_every_second_edge_cut():
    prots, order = A.alternating_path(np.random.default_rng(8), 200)
    got, st = _same(prots)
    assert st["links"] == 199 and st["align"]["aligned"] == 199 and st["align"]["cut"] == 99 and st["edges"] == 100
    assert st["families"] == 100 and st["largest"] == 2
    where = np.argsort(order)                                   # the protein of path position i: i and i + 1 share segment i + 1
    assert M.partition(got) == {frozenset([int(where[i]), int(where[i + 1])]) for i in range(0, 199, 2)}
    plain, pst = _cluster(*M.pack(prots))
    assert pst["families"] == 1


@pytest.mark.parametrize("seed", range(24))
def test_random_batches(seed):
    rng = np.random.default_rng(100 + seed)
    prots = M.random_batch(rng)
    kw = [dict(), dict(ref="member"), dict(min_ratio_pct=70), dict(gap_open=5, gap_extend=2, min_ratio_pct=30)][seed % 4]
    _same(prots, [5, 2, 1][seed % 3], [20, 0][seed % 2], **kw)


def _raw_cluster(seq, off, align):
    lib = N.load()
    p = N.KgClusterParams(5, 20, 0)
    h = C.c_void_p()
    buf = np.frombuffer(seq, dtype=np.uint8)
    N.check(lib.kg_proteins_cluster_aligned(0, C.byref(p), C.byref(align) if align is not None else None, buf.ctypes.data, off.ctypes.data,
                                            len(off) - 1, 0, C.byref(h)))
    return lib, h


def test_a_null_align_is_the_plain_call_and_the_getters_check_their_ranges():
    prots = M.random_batch(np.random.default_rng(9), n_fam=10)
    seq, off = M.pack(prots)
    want, wst = _cluster(seq, off)
    lib, h = _raw_cluster(seq, off, None)
    try:
        got = np.zeros(len(prots), dtype=N.FAMILY_DTYPE)
        N.check(lib.kg_familyset_copy(h, 0, len(prots), got.ctypes.data))
        assert got.tobytes() == want.tobytes() and lib.kg_familyset_edges_count(h) == 0
        st = N.KgClusterStats()
        N.check(lib.kg_familyset_stats(h, C.byref(st)))
        assert {k: st.as_dict()[k] for k in M.COUNTS} == {k: wst[k] for k in M.COUNTS}
        ast = N.KgAlignStats()
        assert lib.kg_familyset_align_stats(h, C.byref(ast)) == N.KG_ERR_ARG
        assert lib.kg_last_error().decode().startswith("kg_familyset_align_stats: the set was made without alignment")
        assert lib.kg_familyset_edges_copy(h, 0, 0, None) == 0 and lib.kg_familyset_edges_copy(h, 0, 1, got.ctypes.data) == N.KG_ERR_ARG
    finally:
        lib.kg_familyset_free(h)
    lib, h = _raw_cluster(seq, off, N.KgAlignParams(50, 0, 11, 1, 1 << 26, None, 0))
    try:
        _, _, edges, _ = A.cluster_aligned_model(seq, off)
        n = int(lib.kg_familyset_edges_count(h))
        assert n == len(edges) >= 4
        part = np.zeros(2, dtype=N.FAMILY_EDGE_DTYPE)
        N.check(lib.kg_familyset_edges_copy(h, n - 2, 2, part.ctypes.data))
        assert part.tobytes() == edges[n - 2:].tobytes()
        N.check(lib.kg_familyset_edges_copy(h, 1, 2, part.ctypes.data))
        assert part.tobytes() == edges[1:3].tobytes()
        for first, count in ((n - 1, 2), (-1, 1), (0, n + 1), (n + 1, 0)):
            assert lib.kg_familyset_edges_copy(h, first, count, part.ctypes.data) == N.KG_ERR_ARG
            assert lib.kg_last_error().decode().startswith("kg_familyset_edges_copy: range outside the set")
        assert lib.kg_familyset_edges_copy(h, n, 0, None) == 0
        assert lib.kg_familyset_align_stats(None, C.byref(N.KgAlignStats())) == N.KG_ERR_ARG
    finally:
        lib.kg_familyset_free(h)
    bad = N.KgAlignParams(50, 0, 11, 0, 1 << 26, None, 0)
    with pytest.raises(N.KmerGutsNativeError) as ei:
        _raw_cluster(seq, off, bad)
    assert ei.value.code == N.KG_ERR_ARG and "gap_extend must be >= 1" in str(ei.value)
    # zero proteins, and proteins without a link
    got, st = _cluster(b"", np.zeros(1, dtype=np.int64), align={})
    assert len(got) == 0 and len(st["edge_records"]) == 0 and st["align"]["aligned"] == 0
    _same([M.random_protein(np.random.default_rng(k), 30) for k in range(5)])


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    import torch
    from kmergutsjava_amd import hotpath, synth
    seq, off = M.pack(M.random_batch(np.random.default_rng(16), n_fam=30))
    want, _, edges, _ = A.cluster_aligned_model(seq, off)
    rec = synth.high_density_config(4, 100, 4001, 500, dna=False)[2]
    with hotpath.SignatureTable.from_bytes(synth.table_image(rec), 0) as tab:
        assert _cluster(seq, off, align={})[0].tobytes() == want.tobytes()
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        failed = 0
        for n in range(1, 400):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got, st = _cluster(seq, off, align={})
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
                assert tab.live_device_bytes() == live0
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= 28 and got.tobytes() == want.tobytes() and st["edge_records"].tobytes() == edges.tobytes()
        assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0


def test_end_to_end_with_align_and_edges(tmp_path):
    """tests/test_gpu_cluster.py's end to end run with --align --edges: the three planted families are still found."""
    import test_gpu_cluster as T
    from kmergutsjava_amd import call_regions as CR, cluster_proteins as CP, synth
    rng = np.random.default_rng(17)
    genes = [M.random_protein(rng, 300) for _ in range(3)]
    contigs = [T._planted(rng, genes, k) for k in range(2)]
    d = tmp_path / "d"
    synth.write_data_dir(str(d), synth.table_image(synth.high_density_config(4, 100, 4001, 500, dna=True)[2]), 1000)
    (tmp_path / "two.fna").write_bytes(b"".join(b">genome%d\n%s\n" % (k, contigs[k][0]) for k in range(2)))
    faa, fam, ann, edges = tmp_path / "two.faa", tmp_path / "families.tsv", tmp_path / "ann.tsv", tmp_path / "edges.tsv"
    assert CR.main(["-D", str(d), "-q", str(tmp_path / "two.fna"), "-o", str(tmp_path / "two.tsv"), "--faa", str(faa), "--free-orfs"]) == 0
    assert CP.main(["-p", str(faa), "-o", str(fam), "-A", str(ann), "--align", "--edges", str(edges)]) == 0
    ids = [[b"genome%d_%d_%d_%s" % (k, left + 1, right + 1, b"-" if strand else b"+") for left, right, strand in contigs[k][1]] for k in range(2)]
    rows = [r.split(b"\t") for r in fam.read_bytes().splitlines()]
    assert all(len(r) == 8 for r in rows)
    families = {}
    for r in rows:
        families.setdefault(r[1], set()).add(r[0])
    mine = {name: who for name, who in families.items() if who & set(ids[0] + ids[1])}
    assert sorted(map(sorted, mine.values())) == sorted(sorted([ids[0][g], ids[1][g]]) for g in range(3))
    erows = [r.split(b"\t") for r in edges.read_bytes().splitlines()]
    assert erows and all(len(r) == 9 and r[8] in (b"kept", b"cut", b"skipped") for r in erows)
    names = set(r[0] for r in rows)
    for r in erows:
        assert int(r[2]) >= 5 and int(r[4]) > 0 and (r[8] != b"kept" or 100 * int(r[3]) >= 50 * int(r[4]))
        if r[8] == b"kept":
            assert r[0] in names and r[1] in names
    # the planted pairs: a substitution at every 12th residue, so the score is most of the self-score
    planted = [r for r in erows if r[0] in set(ids[0] + ids[1]) and r[1] in set(ids[0] + ids[1])]
    assert len(planted) == 3 and all(r[8] == b"kept" and int(r[5]) > 80 for r in planted)
