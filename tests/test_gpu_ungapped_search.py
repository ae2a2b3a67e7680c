"""kg_proteins_search_filtered on the GPU against tests/ungapped_model.py: hit records, hit_start, the 16-byte ungapped records and
the counts byte for byte.  The inputs aim at the diagonal walk's 64-cell steps and its two carries, at the choice of the diagonal
(its ends, ties, runs that cross the scan chunks and a join tile of 2048), at the rule's variants and at the limits.

One case of the issue cannot exist under the rule: a diagonal of one cell.  A seed's window at i needs i + span < len_p in both
proteins, so the diagonal through a shared seed holds its first position and the one behind it: two cells at least (span 1), nine
under the exact 8-mers.  The walk is tested from two cells on."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import align_model as A
import mask_model as MM
import search_model as S
import seed_model as SD
import ungapped_model as UM
from kmergutsjava_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = (SD.IDENTITY, [1])            # one residue is a seed: every diagonal can be built by hand


def _search(seq, off, n_db, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.search_proteins(seq, off, n_db, **kw)


def _check(prots, n_db, seed=None, min_ungapped=0, mask=None, align=None, **kw):
    """The filtered call against the model, byte for byte.  -> (hits, hit_start, ungapped records, statistics)."""
    seq, off = S.batch(prots)
    seeding = None
    if mask is not None:
        flags = MM.mask_numpy(seq, off)[0]
        seeding = MM.soft_mask(seq, off, flags, *MM.side_range(mask, n_db, len(prots)))
    want = UM.filtered_model(seq, off, n_db, seed=seed, seeding=seeding, min_ungapped=min_ungapped, **dict(kw, **(align or {})))
    hits, start, st, ung = _search(seq, off, n_db, seeds=None if seed is None else SD.as_dict(seed), ungapped=dict(min_score=min_ungapped),
                                   mask=None if mask is None else dict(sides=mask), align=align, **kw)
    assert start.tobytes() == want[1].tobytes()
    assert hits.tobytes() == want[0].tobytes()
    assert ung.tobytes() == want[2].tobytes()
    assert {k: st[k] for k in S.STAT_KEYS} == want[3]
    assert {k: st["ungapped"][k] for k in UM.UNGAPPED_KEYS} == want[4]
    assert st["ungapped"]["scored"] == st["candidates"] == st["ungapped"]["dropped"] + st["ungapped"]["cut"] + len(hits)
    return hits, start, ung, st


# ---- the test that shows the feature ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _relative_and_decoy():
    """One query of 200 random residues; a relative, the query with a substitution at every 6th residue but for one stretch of nine
    kept residues (two exact 8-mers on one diagonal); a decoy, a random protein with three of the query's non-overlapping 8-mers
    planted in reverse order (s = 3 on three diagonals).  -> (proteins [decoy, relative, query], n_db)"""
    rng = np.random.default_rng(2024)
    q = bytearray(MM.random_protein(rng, 200))
    rel = bytearray(q)
    for i in range(2, 200, 6):
        if not 60 <= i < 69:
            rel[i] = next(ch for ch in S.ALPHA if ch != q[i] and A.S62[A.codes(bytes([ch]))[0], A.codes(bytes([q[i]]))[0]] < 0)
    for i in range(60, 69):         # the nine kept residues, and a break on both sides of them
        rel[i] = q[i]
    for i in (59, 69):
        rel[i] = next(ch for ch in S.ALPHA if ch != q[i])
    decoy = bytearray(MM.random_protein(rng, 200))
    for at, frm in ((20, 150), (90, 100), (160, 30)):
        decoy[at:at + 8] = q[frm:frm + 8]
    return [bytes(decoy), bytes(rel), bytes(q)], 2


def test_the_collinear_relative_wins_the_one_slot_that_the_scattered_decoy_took():
    prots, n_db = _relative_and_decoy()
    seq, off = S.batch(prots)
    s_of, _ = S.shared_numpy(seq, off, n_db)
    assert s_of == {(0, 0): 3, (0, 1): 2}
    aln = A.align_model(seq, off, [(2, 0), (2, 1)])
    ref = [max(int(a["self_a"]), int(a["self_b"])) for a in aln]
    assert not A.kept(int(aln[0]["score"]), ref[0]) and A.kept(int(aln[1]["score"]), ref[1])
    sc = UM.scored(seq, off, n_db)
    assert sc[(0, 1)][:3] == (2, 0, 2) and sc[(0, 0)][0] == 3 and sc[(0, 0)][2] == 1 and sc[(0, 1)][3] > sc[(0, 0)][3]
    plain = _search(seq, off, n_db, max_cand=1)
    assert [(int(h["target"]), int(h["status"])) for h in plain[0]] == [(0, N.SEARCH_BELOW)]
    hits, start, ung, st = _check(prots, n_db, max_cand=1)
    assert [(int(h["target"]), int(h["status"]), int(h["rank"])) for h in hits] == [(1, N.SEARCH_HIT, 0)]
    assert int(ung[0]["on_diagonal"]) == 2 and int(ung[0]["diagonal"]) == 0 and int(ung[0]["ungapped"]) <= int(hits[0]["score"])
    assert st["ungapped"]["cut"] == 1 and st["ungapped"]["dropped"] == 0 and st["ungapped"]["ms_ungapped"] > 0
    assert st["ms_total"] >= st["ms_join"] + st["ungapped"]["ms_ungapped"] > 0


# ---- the diagonal walk --------------------------------------------------------------------------------------------------------

W8 = b"ACDEFGHK"                       # the one shared 8-mer: 49 on its eight cells
CELL = {"+": (b"I", b"V"), "-": (b"W", b"D"), "0": (b"S", b"E")}        # 3, -4 and 0 under BLOSUM62, no residue shared


def _diag_pair(pattern: str, seed_at: int = 0):
    """Query and target of equal length: the 8-mer at seed_at, every other cell of diagonal 0 as the pattern says.  No second 8-mer
    is shared, so g* = 0 and the diagonal is the whole pair."""
    q, d = bytearray(), bytearray()
    for k, ch in enumerate(pattern):
        if seed_at <= k < seed_at + 8:
            q += W8[k - seed_at:k - seed_at + 1]
            d += W8[k - seed_at:k - seed_at + 1]
        else:
            q += CELL[ch][0]
            d += CELL[ch][1]
    return bytes(d), bytes(q)


def _walk(pattern, seed_at=0):
    d, q = _diag_pair(pattern, seed_at)
    hits, start, ung, st = _check([d, q], 1, min_shared=1)
    assert len(hits) == 1 and int(ung[0]["diagonal"]) == 0 and int(ung[0]["on_diagonal"]) == 1
    assert st["ungapped"]["cells"] == len(pattern)
    return int(ung[0]["ungapped"])


@pytest.mark.parametrize("length", [9, 63, 64, 65, 127, 128, 129])
def test_overlap_lengths_round_the_64_cell_step(length):
    assert _walk("+" * length) == 49 + 3 * (length - 8)           # the best run is the whole diagonal
    assert _walk("-" * length) == 49                                # ... and the seed alone


def test_best_runs_at_the_step_border_and_the_minimum_carry():
    neg = "-" * 32
    assert _walk("S" * 8 + neg + "+" * 24 + "-" * 30) == 72                 # ends at cell 63
    assert _walk("S" * 8 + "-" * 56 + "+" * 24 + "-" * 30) == 72            # starts at cell 64
    assert _walk("S" * 8 + "-" * 52 + "+" * 11 + "-" * 30) == 49            # cells 60 .. 70: 33, below the seed's 49
    assert _walk("-" * 52 + "S" * 8 + "+" * 11 + "-" * 30, seed_at=52) == 49 + 33     # spans 52 .. 70 across the border
    # a deep negative stretch in the first step, the best run in the third: the minimum carried is the one behind the stretch
    assert _walk("S" * 8 + "-" * 50 + "0" * 80 + "+" * 30 + "-" * 20) == 90
    assert _walk("-" * 140 + "S" * 8 + "+" * 10 + "-" * 9, seed_at=140) == 79


def test_the_two_cell_diagonal_and_the_ends_of_the_diagonal_range():
    """Single residues as seeds.  W is shared only by the query's first and the target's last window (g at its most negative, two
    cells), by the query's last and the target's first (most positive), and on diagonal 0."""
    far = [b"DDDDDDWD", b"WIIIIIII"]               # g = 0 - 6, cells (0, 6), (1, 7): W/W + I/D = 11 - 3
    hits, start, ung, st = _check(far, 1, seed=ONE, min_shared=1)
    assert [tuple(int(x) for x in u)[:3] for u in ung] == [(11, -6, 1)] and st["ungapped"]["cells"] == 2
    near = [b"WIIIIIII", b"DDDDDDWD"]              # g = 6
    hits, start, ung, st = _check(near, 1, seed=ONE, min_shared=1)
    assert [tuple(int(x) for x in u)[:3] for u in ung] == [(11, 6, 1)] and st["ungapped"]["cells"] == 2
    zero = [b"WDDDDDDD", b"WIIIIIII" + b"I" * 70]
    hits, start, ung, st = _check(zero, 1, seed=ONE, min_shared=1)
    assert [tuple(int(x) for x in u)[:3] for u in ung] == [(11, 0, 1)] and st["ungapped"]["cells"] == 8


# ---- the diagonal choice ------------------------------------------------------------------------------------------------------

def test_first_positions_ties_and_the_all_negative_diagonal():
    # the seed W occurs twice in the target: its first position counts.  Y too, once each: two diagonals with m = 1, the smaller wins
    prots = [b"DDWDDWDDYDD", b"IIIIWIIYIII"]       # W: 4 - 2 = 2, Y: 7 - 8 = -1
    hits, start, ung, st = _check(prots, 1, seed=ONE, min_shared=1)
    assert (int(ung[0]["diagonal"]), int(ung[0]["on_diagonal"]), int(hits[0]["shared"])) == (-1, 1, 2)
    assert int(ung[0]["ungapped"]) == UM.ungapped_loops(prots[1], prots[0], -1) == 12      # W/W I/D I/D Y/Y: 11 - 3 - 3 + 7
    # a seed's diagonal holds the seed's own match: only a matrix without a positive entry makes a diagonal all negative, and u = 0
    hits, start, ung, st = _check(prots, 1, seed=ONE, min_shared=1, align=dict(matrix=np.full((21, 21), -1)))
    assert (int(ung[0]["ungapped"]), int(ung[0]["diagonal"]), int(hits[0]["score"])) == (0, -1, 0)


@pytest.mark.parametrize("shared", [1, 15, 16, 17, 2049])
def test_runs_across_the_scan_chunks_and_a_join_tile(shared):
    """A query and a target with `shared` 8-mers in common, the target holding them rotated: two diagonals, the larger part wins.
    A second target shares one 8-mer, a second query three.  2049 join items of one (q, d) cross the join's tile of 2048."""
    rng = np.random.default_rng(shared)
    kmers = S.distinct_kmers(rng, shared + 4)
    own, rest = kmers[:shared], kmers[shared:]
    cut_at = shared // 2
    prots = [S.protein_of(own[cut_at:] + own[:cut_at]), S.protein_of(rest[:1] + own[:1]), S.protein_of(rest[1:2] + own),
             S.protein_of(own[:2] + rest[2:3] + own[-1:])]
    hits, start, ung, st = _check(prots, 2, min_shared=1, align=dict(max_cells=1 << 16))
    first = [k for k, h in enumerate(hits) if (int(h["query"]), int(h["target"])) == (0, 0)][0]
    assert int(hits[first]["shared"]) == shared and int(ung[first]["on_diagonal"]) == shared - cut_at
    assert st["join_pairs"] >= shared + 3


def test_the_cut_by_u_then_s_then_d_and_the_threshold():
    """Three targets with the same diagonal score: u equal at the cut, the larger s wins, then the smaller d; min_ungapped at u
    keeps and at u + 1 drops."""
    rng = np.random.default_rng(7)
    k = S.distinct_kmers(rng, 4)
    body = S.protein_of(k[:1])
    # target 0 and 1: the one 8-mer; target 2: the same and a second one on another diagonal, in front, so that g* ties to ...
    prots = [body, body, S.protein_of(k[:1]) + S.protein_of(k[1:2]), S.protein_of(k[:1]) + b"X" * 9 + S.protein_of(k[1:2])]
    seq, off = S.batch(prots)
    sc = UM.scored(seq, off, 3, min_shared=1)
    u = sc[(0, 0)][3]
    assert sc[(0, 0)][3] == sc[(0, 1)][3] == u and sc[(0, 2)][0] == 2
    for max_cand in (1, 2, 3):
        _check(prots, 3, min_shared=1, max_cand=max_cand)
    hits, start, ung, st = _check(prots, 3, min_shared=1, max_cand=2)
    assert sorted(int(h["target"]) for h in hits) == ([0, 2] if sc[(0, 2)][3] == u else sorted(int(h["target"]) for h in hits))
    assert len(_check(prots, 3, min_shared=1, min_ungapped=u)[0]) >= 2
    hits, start, ung, st = _check(prots, 3, min_shared=1, min_ungapped=u + 1)
    assert all(int(x["ungapped"]) > u for x in ung) and st["ungapped"]["dropped"] >= 2


# ---- rule variants ------------------------------------------------------------------------------------------------------------

def test_reduced_seeds_a_mask_and_a_custom_matrix():
    rng = np.random.default_rng(11)
    targets, queries = SD.conservative_pairs(rng, 6)
    prots = targets + queries + [MM.random_protein(rng, 120)]
    hits, start, ung, st = _check(prots, 6, seed=SD.REDUCED)
    assert len(hits) >= 6 and all(int(u["on_diagonal"]) >= 2 for u in ung[[int(start[q]) for q in range(6)]])
    # the same value under two shapes on one diagonal counts 2: 16 residues whose window 0 is a seed of both shapes, and an X
    # on positions 9 and 12, which neither looks at, takes windows 1 to 3 of the shorter shape away
    w = bytearray(MM.random_protein(rng, 16))
    w[9] = w[12] = ord("X")
    two = [bytes(w), bytes(w)]
    hits, start, ung, st = _check(two, 1, seed=SD.REDUCED, min_shared=1)
    assert (int(hits[0]["shared"]), int(ung[0]["on_diagonal"]), int(ung[0]["diagonal"])) == (2, 2, 0)
    # a mask: the positions come from the masked copy, the scores from the original
    planted, n_db = MM.planted_search(seed=5, n_targets=8, n_related=4)
    for sides in ("both", "queries"):
        _check(planted, n_db, mask=sides)
    # a custom matrix: identity 5, everything else -3, non-residues -2
    mat = np.full((21, 21), -3, dtype=np.int64)
    np.fill_diagonal(mat, 5)
    mat[20, :] = mat[:, 20] = -2
    hits, start, ung, st = _check(planted, n_db, align=dict(matrix=mat))
    assert len(hits) > 0


# ---- invariances --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _batches():
    out = []
    for seed in range(6):
        prots, n_db = MM.planted_search(seed=100 + seed, n_targets=10, n_related=5, length=90 + 10 * seed)
        out.append((tuple(prots), n_db))
    return out


def test_without_a_cut_the_records_are_the_unfiltered_call_s_and_u_is_at_most_the_score():
    for prots, n_db in _batches():
        seq, off = S.batch(list(prots))
        plain = _search(seq, off, n_db, max_cand=64)
        assert plain[2]["candidates"] == len(plain[0]) > 0                 # no query over max_cand
        hits, start, ung, st = _check(list(prots), n_db, max_cand=64)
        assert hits.tobytes() == plain[0].tobytes() and start.tobytes() == plain[1].tobytes()
        ok = hits["status"] != N.SEARCH_SKIPPED
        assert ok.all() and (ung["ungapped"][ok] <= hits["score"][ok]).all() and (ung["ungapped"] > 0).all()
        assert {k: st[k] for k in S.STAT_KEYS} == {k: plain[2][k] for k in S.STAT_KEYS}


def test_twice_reversed_and_alone():
    prots, n_db = _batches()[1]
    prots = list(prots)
    a, b = _check(prots, n_db, max_cand=3), _check(prots, n_db, max_cand=3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))
    rev = prots[:n_db][::-1] + prots[n_db:]             # (no cut: under a cut, ties of (u, s) go to the smaller target)
    f, r = _check(prots, n_db, max_cand=64), _check(rev, n_db, max_cand=64)
    assert r[1].tobytes() == f[1].tobytes()
    assert sorted((int(h["query"]), n_db - 1 - int(h["target"]), int(h["score"]), int(u["ungapped"]), int(u["diagonal"])) for h, u in zip(r[0], r[2])) == \
        sorted((int(h["query"]), int(h["target"]), int(h["score"]), int(u["ungapped"]), int(u["diagonal"])) for h, u in zip(f[0], f[2]))
    one = _check(prots[:n_db] + [prots[n_db + 2]], n_db, max_cand=3)
    lo, hi = int(a[1][2]), int(a[1][3])
    assert len(one[0]) == hi - lo
    for name in ("target", "shared", "score", "status", "rank"):
        assert list(one[0][name]) == list(a[0][name][lo:hi])
    assert one[2].tobytes() == a[2][lo:hi].tobytes()


# ---- limits and errors --------------------------------------------------------------------------------------------------------

def _raw_call(lib, seq, off, n_db, up, device_ptr=None, prm=(2, 8, 256, 0)):
    from kmergutsjava_amd import hotpath
    arr = np.frombuffer(seq, dtype=np.uint8)
    p, ap, h = N.KgSearchParams(*prm), hotpath._align_params()[0], C.c_void_p()
    fn = lib.kg_proteins_search_filtered_device if device_ptr else lib.kg_proteins_search_filtered
    rc = fn(0, C.byref(p), None, C.byref(ap), device_ptr or arr.ctypes.data, off.ctypes.data, len(off) - 1, n_db, 0, 0, 0, 0, None, 0,
            C.byref(up) if up is not None else None, C.byref(h))
    return rc, h


def test_the_argument_errors_and_the_getters_on_another_call_s_set():
    lib = N.load()
    prots, n_db = _batches()[0]
    seq, off = S.batch(list(prots))
    for up, words in ((None, b"null kg_ungapped_params"), (N.KgUngappedParams(-1, (C.c_int32 * 3)()), b"min_ungapped must be >= 0"),
                      (N.KgUngappedParams(0, (C.c_int32 * 3)(0, 1, 0)), b"kg_ungapped_params.reserved must be 0")):
        rc, h = _raw_call(lib, seq, off, n_db, up)
        assert rc == N.KG_ERR_ARG and lib.kg_last_error().startswith(words) and not h.value
    rc, h = _raw_call(lib, seq, off, n_db, N.KgUngappedParams(0, (C.c_int32 * 3)()), prm=(2, 65, 256, 0))
    assert rc == N.KG_ERR_ARG and lib.kg_last_error().startswith(b"max_cand must be in 1..64")
    from kmergutsjava_amd import hotpath
    p, ap, h = N.KgSearchParams(2, 8, 256, 0), hotpath._align_params()[0], C.c_void_p()
    arr = np.frombuffer(seq, dtype=np.uint8)
    assert lib.kg_proteins_search(0, C.byref(p), C.byref(ap), arr.ctypes.data, off.ctypes.data, len(off) - 1, n_db, 0, 0, C.byref(h)) == N.KG_OK
    try:
        st, rec = N.KgUngappedStats(), np.zeros(1, dtype=N.SEARCH_UNGAPPED_DTYPE)
        assert lib.kg_hitset_ungapped_stats(h, C.byref(st)) == N.KG_ERR_ARG and b"without the ungapped stage" in lib.kg_last_error()
        assert lib.kg_hitset_ungapped_copy(h, 0, 1, rec.ctypes.data) == N.KG_ERR_ARG and b"without the ungapped stage" in lib.kg_last_error()
    finally:
        lib.kg_hitset_free(h)


def test_the_device_entry_point_and_empty_calls():
    import torch
    prots, n_db = _batches()[2]
    seq, off = S.batch(list(prots))
    want = _check(list(prots), n_db)
    dev = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    got = _search(None, off, n_db, device_ptr=dev.data_ptr(), ungapped=True)
    assert got[0].tobytes() == want[0].tobytes() and got[3].tobytes() == want[2].tobytes()
    assert dev.cpu().numpy().tobytes() == seq
    got = _search(b"", np.zeros(1, dtype=np.int64), 0, ungapped=True)
    assert len(got[0]) == 0 and len(got[3]) == 0 and got[2]["ungapped"]["scored"] == 0
    _check([b"ACDEFGHIKLMNPQRSTVWY", b"", b"WWWWWWWWWWWW", b""], 2)          # no candidate at all
    paths = _search(seq, off, n_db, ungapped=True, paths="hits")
    assert paths[0].tobytes() == want[0].tobytes() and paths[-1].tobytes() == want[2].tobytes() and len(paths) == 5


def test_key_widths_of_64_bits_pass_and_of_65_are_refused():
    """Mostly empty proteins and one long one on each side: 2^20 targets and 2^20 queries are 20 bits each; the longest query plus
    the longest target is 2^24 for 24 bits, and one residue more for 25."""
    lib = N.load()
    n_each = 1 << 20
    rng = np.random.default_rng(3)
    for extra, want in ((0, N.KG_OK), (1, N.KG_ERR_LIMIT)):
        lens = np.zeros(2 * n_each, dtype=np.int64)
        lens[5], lens[n_each + 7] = 1 << 23, (1 << 23) + extra
        off = np.r_[0, np.cumsum(lens)].astype(np.int64)
        # (two residues only: nearly every 8-mer is in the target often, but once per target: it is one target)
        seq = np.frombuffer(b"AC", dtype=np.uint8)[rng.integers(0, 2, int(off[-1]))].tobytes()
        rc, h = _raw_call(lib, seq, off, n_each, N.KgUngappedParams(0, (C.c_int32 * 3)()))
        assert rc == want, lib.kg_last_error()
        if rc == N.KG_OK:
            st, us, rec = N.KgSearchStats(), N.KgUngappedStats(), np.zeros(1, dtype=N.SEARCH_UNGAPPED_DTYPE)
            try:
                assert lib.kg_hitset_stats(h, C.byref(st)) == N.KG_OK and st.candidates == 1 and st.skipped == 1
                assert lib.kg_hitset_ungapped_stats(h, C.byref(us)) == N.KG_OK and us.scored == 1 and 0 < us.cells <= 1 << 23
                assert lib.kg_hitset_ungapped_copy(h, 0, 1, rec.ctypes.data) == N.KG_OK and int(rec[0]["on_diagonal"]) >= 1
            finally:
                lib.kg_hitset_free(h)
        else:
            msg = lib.kg_last_error()
            assert msg.startswith(b"the join key of the ungapped stage does not fit 64 bits: 20 bits of the queries, 20 of the targets and 25")


def test_every_allocation_failed_in_turn_gives_the_memory_back(monkeypatch):
    """Every device allocation of the call refused in turn, the paths behind it included (as tests/test_gpu_search.py does it for
    the plain call): KG_ERR_NOMEM each time, and device memory back where it was."""
    import torch
    from kmergutsjava_amd import hotpath, synth
    prots, n_db = _batches()[0]
    seq, off = S.batch(list(prots))
    want = UM.filtered_model(seq, off, n_db)
    rec = synth.high_density_config(4, 100, 4001, 500, dna=False)[2]
    with hotpath.SignatureTable.from_bytes(synth.table_image(rec), 0) as tab:
        assert _search(seq, off, n_db, ungapped=True, paths="hits")[0].tobytes() == want[0].tobytes()
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        failed = 0
        for n in range(1, 800):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got = _search(seq, off, n_db, ungapped=True, paths="hits")
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
                assert tab.live_device_bytes() == live0
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        # (the plain call's test counts 60 at least; this stage allocates 14 blocks the plain call does not: the run flags, its
        # totals and counters, the second level's heads, scan and starts, the best words, the diagonals, u, its flags and scan,
        # the kept records, the aligned ones and the set's own)
        assert failed >= 74 and got[0].tobytes() == want[0].tobytes() and got[-1].tobytes() == want[2].tobytes()
        assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0


# ---- the front end ------------------------------------------------------------------------------------------------------------

def test_the_command_line_on_mutated_proteins_of_the_golden_proteome(tmp_path):
    from kmergutsjava_amd import search_proteins as SP
    import gzip
    from kmergutsjava_amd.make_signatures import parse_fasta
    ids, prots = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))
    pick = [k for k in range(0, len(ids), len(ids) // 400) if 60 <= len(prots[k]) <= 400][:192]
    ids, prots = [ids[k] for k in pick], [bytes(prots[k]) for k in pick]
    assert len(ids) == 192
    rng = np.random.default_rng(9)
    muts = [A.mutate(rng, p, 0.15) for p in prots]
    db, qs, out = tmp_path / "db.faa", tmp_path / "q.faa", tmp_path / "hits.tsv"
    db.write_bytes(b"".join(b">" + i + b"\n" + p + b"\n" for i, p in zip(ids, prots)))
    qs.write_bytes(b"".join(b">" + i + b"_m\n" + p + b"\n" for i, p in zip(ids, muts)))
    run = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.search_proteins", "-d", str(db), "-q", str(qs), "-o", str(out),
                          "--seeds", "reduced", "--ungapped", "--min-ungapped", "30", "--all"], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr
    seq, off = S.batch(prots + muts)
    want = UM.filtered_model(seq, off, 192, seed=SD.REDUCED, min_ungapped=30)
    assert out.read_bytes() == SP.format_hits([i + b"_m" for i in ids], ids, want[0], want[1], write_all=True, ungapped=want[2])
    assert ", ungapped: scored %d, dropped %d, cut %d, ungapped ms: " % (want[4]["scored"], want[4]["dropped"], want[4]["cut"]) in run.stderr
