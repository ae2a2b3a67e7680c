"""kg_proteins_search_masked and kg_proteins_cluster_masked on the GPU against tests/mask_model.py: the seeding pass reads the
soft-masked copy, everything behind it the original.  Records, starts and counts byte for byte; the three front ends end to end."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_model as A
import cluster_model as CM
import mask_model as MM
import search_model as S
import seed_model as SD
from kmergutsjava_amd import _native as N

pytestmark = pytest.mark.gpu

HC = MM.ALPHA * 8


def _search(seq, off, n_db, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.search_proteins(seq, off, n_db, **kw)


def _same(got, want):
    hits, start, st = got[0], got[1], got[-1] if isinstance(got[-1], dict) else got[3]
    assert {k: st[k] for k in S.STAT_KEYS} == want[2]
    assert start.tobytes() == want[1].tobytes() and hits.tobytes() == want[0].tobytes()
    assert {k: st["mask"][k] for k in MM.COUNTS} == want[3]


@functools.lru_cache(maxsize=None)
def _planted():
    """The planted example and its models, computed once: (seq, off, n_db, {seeds: masked model})."""
    prots, n_db = MM.planted_search()
    seq, off = S.batch(prots)
    return seq, off, n_db, {None: MM.masked_search_model(seq, off, n_db), "reduced": MM.masked_search_model(seq, off, n_db, seed=SD.REDUCED)}


# ---- the test that shows the feature ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeds", [None, "reduced"])
def test_the_planted_insert_seeds_every_pair_unmasked_and_only_the_relatives_masked(seeds):
    """24 targets of 150 residues with the insert QE * 8 + Q * 10, 12 queries that are 5 %-mutated copies of targets 0..11 and 12
    unrelated queries with the same insert.  On the model: unmasked all 576 pairs are candidates; masked the unrelated queries
    have no record and the 12 related ones exactly their own target.  The device equals the model, and the related queries'
    rank-0 records have the scores of the unmasked call."""
    seq, off, n_db, models = _planted()
    shared = S.shared_numpy if seeds is None else SD.shared_numpy(SD.REDUCED)
    assert sum(1 for s in shared(seq, off, n_db)[0].values() if s >= S.MIN_SHARED) == 576
    want = models[seeds]
    assert want[2]["candidates"] == 12 and len(want[0]) == 12 and list(np.diff(want[1])) == [1] * 12 + [0] * 12
    assert [(h["query"], h["target"], h["rank"], h["status"]) for h in want[0]] == [(q, q, 0, N.SEARCH_HIT) for q in range(12)]
    assert want[3]["proteins_masked"] == 48 and want[3]["masked_residues"] >= 48 * 20
    plain = _search(seq, off, n_db, seeds=seeds)
    assert plain[2]["candidates"] == 576 and len(plain[0]) == 192 and int(plain[1][-1] - plain[1][12]) == 96
    got = _search(seq, off, n_db, seeds=seeds, mask=True)
    _same(got, want)
    assert [int(plain[0][plain[1][q]]["score"]) for q in range(12)] == [int(got[0][got[1][q]]["score"]) for q in range(12)]
    assert [int(plain[0][plain[1][q]]["target"]) for q in range(12)] == list(range(12))
    assert got[2]["mask"]["ms_mask"] > 0 and "mask" not in plain[2]


def test_without_a_low_window_the_masked_call_is_the_unmasked_call():
    rng = np.random.default_rng(71)
    fam = [HC[k:k + 90] for k in (0, 3, 7, 11)]
    prots = [A.mutate(rng, fam[k % 4], 0.04)[: 60 + 5 * k] for k in range(10)] + [HC[5:70], b"", HC[:9]]
    seq, off = S.batch(prots)
    assert MM.mask_numpy(seq, off)[3]["low_windows"] == 0
    for kw in ({}, dict(seeds="reduced")):
        plain, got = _search(seq, off, 6, **kw), _search(seq, off, 6, mask=True, **kw)
        assert len(plain[0]) > 0 and got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
        assert {k: got[2][k] for k in S.STAT_KEYS} == {k: plain[2][k] for k in S.STAT_KEYS}
        assert got[2]["mask"]["masked_residues"] == 0 and got[2]["mask"]["segments"] == 0 and got[2]["mask"]["proteins"] == len(prots)


def test_sides_mask_only_that_side():
    """The insert on the targets only: masking the targets takes their insert windows away, masking the queries changes nothing
    but the statistics of the mask."""
    rng = np.random.default_rng(72)
    bodies = [MM.random_protein(rng, 120) for _ in range(8)]
    targets = [MM.with_insert(rng, b) for b in bodies]
    queries = [MM.mutate(rng, b, 0.05) for b in bodies[:5]] + [MM.random_protein(rng, 100)]
    seq, off = S.batch(targets + queries)
    n_db = len(targets)
    seen = {}
    for sides in ("targets", "queries", "both"):
        want = MM.masked_search_model(seq, off, n_db, sides=sides)
        got = _search(seq, off, n_db, mask=dict(sides=sides))
        _same(got, want)
        seen[sides] = got[2]
    plain = _search(seq, off, n_db)[2]
    assert seen["queries"]["valid_windows"] == plain["valid_windows"] > seen["targets"]["valid_windows"] == seen["both"]["valid_windows"]
    assert seen["targets"]["mask"]["proteins"] == n_db and seen["queries"]["mask"]["proteins"] == len(queries)
    assert seen["targets"]["mask"]["proteins_masked"] == n_db and seen["queries"]["mask"]["masked_residues"] == 0


def test_paths_and_ops_behind_a_masked_search_are_the_unmasked_call_s():
    seq, off, n_db, models = _planted()
    plain = _search(seq, off, n_db, paths="hits", ops="eqx")
    got = _search(seq, off, n_db, paths="hits", ops="eqx", mask=True)
    assert got[0].tobytes() == models[None][0].tobytes() and len(got[0]) == 12
    at = {(int(h["query"]), int(h["target"])): k for k, h in enumerate(plain[0])}
    for k, h in enumerate(got[0]):
        j = at[(int(h["query"]), int(h["target"]))]
        assert got[2][k].tobytes() == plain[2][j].tobytes() and got[2][k]["status"] == N.PATH_TRACED
        assert got[5][got[4][k]:got[4][k + 1]].tobytes() == plain[5][plain[4][j]:plain[4][j + 1]].tobytes()
        assert int(h["score"]) == int(plain[0][j]["score"])
    assert got[3]["traced"] == 12 and got[3]["mask"]["segments"] >= 48


def test_the_device_sequence_zero_proteins_and_the_argument_errors():
    import torch
    from kmergutsjava_amd import hotpath
    seq, off, n_db, models = _planted()
    dev = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    _same(_search(None, off, n_db, device_ptr=dev.data_ptr(), mask=True), models[None])
    assert dev.cpu().numpy().tobytes() == seq                           # the caller's sequence is not written
    got = _search(b"", np.zeros(1, dtype=np.int64), 0, mask=True)
    assert len(got[0]) == 0 and got[2]["mask"]["proteins"] == 0
    for bad, word in ((dict(window=3), "window"), (dict(trigger=700), "extend"), (dict(extend=917), "Lg(window)")):
        with pytest.raises(N.KmerGutsNativeError) as ei:
            _search(seq, off, n_db, mask=bad)
        assert ei.value.code == N.KG_ERR_ARG and word in str(ei.value)
    lib = N.load()
    arr = np.frombuffer(seq, dtype=np.uint8)
    p, ap, mp, h = N.KgSearchParams(2, 8, 256, 0), hotpath._align_params()[0], N.KgMaskParams(12, 563, 640, 0), C.c_void_p()
    for sides in (0, 4):
        rc = lib.kg_proteins_search_masked(0, C.byref(p), None, C.byref(ap), arr.ctypes.data, off.ctypes.data, len(off) - 1, n_db, 0, 0, 0, 0,
                                           C.byref(mp), sides, C.byref(h))
        assert rc == N.KG_ERR_ARG and b"sides" in lib.kg_last_error() and not h.value
    assert lib.kg_proteins_search_masked(0, C.byref(p), None, C.byref(ap), arr.ctypes.data, off.ctypes.data, len(off) - 1, n_db, 0, 0, 0, 0,
                                         None, 3, C.byref(h)) == N.KG_ERR_ARG
    st = N.KgMaskStats()
    assert lib.kg_proteins_search(0, C.byref(p), C.byref(ap), arr.ctypes.data, off.ctypes.data, len(off) - 1, n_db, 0, 0, C.byref(h)) == N.KG_OK
    try:
        assert lib.kg_hitset_mask_stats(h, C.byref(st)) == N.KG_ERR_ARG and b"without a mask" in lib.kg_last_error()
    finally:
        lib.kg_hitset_free(h)


# ---- families -----------------------------------------------------------------------------------------------------------------

def _two_families(rng):
    """Two families of three 6 %-mutated copies each, every protein with the same 60-residue Q/E linker in it: the linker's
    8-mers are a third of a protein's, more than min_cover asks."""
    linker = bytes(rng.choice(np.frombuffer(b"QE", dtype=np.uint8), 60))
    a, b = MM.random_protein(rng, 110), MM.random_protein(rng, 110)
    return [MM.with_insert(rng, MM.mutate(rng, body, 0.06), linker) for body in (a, b, a, b, a, b)] + [MM.random_protein(rng, 80)]


def test_a_shared_linker_joins_two_families_unmasked_and_not_masked():
    from kmergutsjava_amd import hotpath
    prots = _two_families(np.random.default_rng(73))
    seq, off = S.batch(prots)
    plain_model = CM.cluster_numpy(seq, off)
    rec_model, counts, mcounts = MM.masked_cluster_model(seq, off)
    assert CM.partition(plain_model[0]) == {frozenset(range(6)), frozenset([6])}
    assert CM.partition(rec_model) == {frozenset([0, 2, 4]), frozenset([1, 3, 5]), frozenset([6])}
    rec, st = hotpath.cluster_proteins(seq, off)
    assert rec.tobytes() == plain_model[0].tobytes() and "mask" not in st
    rec, st = hotpath.cluster_proteins(seq, off, mask=True)
    assert rec.tobytes() == rec_model.tobytes() and {k: st[k] for k in CM.COUNTS} == counts
    assert {k: st["mask"][k] for k in MM.COUNTS} == mcounts and mcounts["proteins_masked"] == 6
    # the alignment step reads the proteins as they are: the scores of the links both calls have are the same
    # (min_ratio 20: the 6 %-mutated members with the linker at another place score 45 to 60 % of the longer self-score)
    rec_a, st_a = hotpath.cluster_proteins(seq, off, mask=dict(window=12), align=dict(min_ratio_pct=20))
    plain_a = hotpath.cluster_proteins(seq, off, align=dict(min_ratio_pct=20))[1]["edge_records"]
    score = {(int(e["member"]), int(e["centre"])): (int(e["score"]), int(e["ref"])) for e in plain_a}
    assert len(st_a["edge_records"]) > 0 and CM.partition(rec_a) == CM.partition(rec_model)
    both = [e for e in st_a["edge_records"] if (int(e["member"]), int(e["centre"])) in score]       # (the linker's 8-mers move some centres)
    assert len(both) > 0
    for e in both:
        assert score[(int(e["member"]), int(e["centre"]))] == (int(e["score"]), int(e["ref"]))
    lib, stm = N.load(), N.KgMaskStats()
    h = C.c_void_p()
    arr = np.frombuffer(seq, dtype=np.uint8)
    assert lib.kg_proteins_cluster(0, C.byref(N.KgClusterParams(5, 20, 0)), arr.ctypes.data, off.ctypes.data, len(off) - 1, 0, C.byref(h)) == N.KG_OK
    try:
        assert lib.kg_familyset_mask_stats(h, C.byref(stm)) == N.KG_ERR_ARG
    finally:
        lib.kg_familyset_free(h)
    assert hotpath.cluster_proteins(b"", np.zeros(1, dtype=np.int64), mask=True)[1]["mask"]["proteins"] == 0


# ---- the front ends -------------------------------------------------------------------------------------------------------------

def _fasta(ids, prots) -> bytes:
    return b"".join(b">" + i + b"\n" + p + b"\n" for i, p in zip(ids, prots))


def test_the_three_command_lines_end_to_end(tmp_path, capsys):
    from kmergutsjava_amd import cluster_proteins as CP
    from kmergutsjava_amd import mask_proteins as MP
    from kmergutsjava_amd import search_proteins as SP
    rng = np.random.default_rng(74)
    prots = _two_families(rng)
    ids = [b"p%d" % k for k in range(len(prots))]
    src = tmp_path / "all.faa"
    src.write_bytes(_fasta(ids, prots))
    seq, off = S.batch(prots)
    flags, segs, _, counts = MM.mask_numpy(seq, off)
    # mask_proteins
    out, tsv = tmp_path / "masked.faa", tmp_path / "segments.tsv"
    assert MP.main(["-p", str(src), "-o", str(out), "--segments", str(tsv)]) == 0
    assert out.read_bytes() == MP.format_fasta(ids, prots, flags, off) and tsv.read_bytes() == MP.format_segments(ids, segs)
    err = capsys.readouterr().err
    assert err.startswith("Proteins: 7, residues: %d, masked: %d (" % (counts["residues"], counts["masked_residues"]))
    assert ", segments: %d, proteins touched: 6, ms: " % counts["segments"] in err
    assert MP.main(["-p", str(src), "-o", str(out), "--x", "--window", "10", "--trigger", "500", "--extend", "600"]) == 0
    assert out.read_bytes() == MP.format_fasta(ids, prots, MM.mask_numpy(seq, off, 10, 500, 600)[0], off, x=True)
    capsys.readouterr()
    # cluster_proteins --mask
    fam, fam_m = tmp_path / "fam.tsv", tmp_path / "fam_masked.tsv"
    assert CP.main(["-p", str(src), "-o", str(fam)]) == 0
    plain_err = capsys.readouterr().err
    assert CP.main(["-p", str(src), "-o", str(fam_m), "--mask"]) == 0
    err = capsys.readouterr().err
    assert ", mask: 12/563/640, masked residues: %d" % counts["masked_residues"] in err and ", mask:" not in plain_err
    assert fam.read_bytes() == CP.format_families(ids, CM.cluster_numpy(seq, off)[0])
    assert fam_m.read_bytes() == CP.format_families(ids, MM.masked_cluster_model(seq, off)[0]) != fam.read_bytes()
    # search_proteins --mask: the first four proteins are the database, the rest the queries
    db, qs = tmp_path / "db.faa", tmp_path / "q.faa"
    db.write_bytes(_fasta(ids[:4], prots[:4]))
    qs.write_bytes(_fasta(ids[4:], prots[4:]))
    hits, hits_m = tmp_path / "hits.tsv", tmp_path / "hits_masked.tsv"
    assert SP.main(["-d", str(db), "-q", str(qs), "-o", str(hits), "--all"]) == 0
    plain_err = capsys.readouterr().err
    assert SP.main(["-d", str(db), "-q", str(qs), "-o", str(hits_m), "--all", "--mask", "queries", "--mask-extend", "650"]) == 0
    err = capsys.readouterr().err
    want = MM.masked_search_model(seq, off, 4, extend=650, sides="queries")
    assert ", mask: 12/563/650 queries, masked residues: %d" % want[3]["masked_residues"] in err and ", mask:" not in plain_err
    assert hits_m.read_bytes() == SP.format_hits(ids[4:], ids[:4], want[0], want[1], write_all=True)
    assert hits.read_bytes() == SP.format_hits(ids[4:], ids[:4], *S.search_model(seq, off, 4)[:2], write_all=True) != hits_m.read_bytes()
