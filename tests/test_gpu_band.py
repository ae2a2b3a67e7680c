"""kg_proteins_align_banded and kg_proteins_search_banded on the GPU against tests/band_model.py: the records, the paths, the ops
and the counts byte for byte.  The inputs aim at align_band_kernel's moved window (its clips at both ends of b, a start at a
stripe border, bands that miss the matrix), at the carry between stripes (gaps at the band's edge, across rows 63 / 64, what an
earlier stripe or pair left in LDS), at the tie rule under a band, at the cap by band cells and at the band's two ends: a
covering band is kg_proteins_align_ops byte for byte, and W = 0 is the ungapped score."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import align_model as A
import band_model as B
import search_model as S
import seed_model as SD
import ungapped_model as UM
from kmergutsjava_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN_GRID = 256 * 18               # kAlignGrid of kg_host_align.hpp: the workgroups of one launch


def _align(seq, off, pairs, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.align_proteins(seq, off, pairs, **kw)


def _search(seq, off, n_db, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.search_proteins(seq, off, n_db, **kw)


def _check(prots, pairs, diags, W, mode="m", matrix=None, max_cells=N.ALIGN_DEFAULT_MAX_CELLS, traced=True, **kw):
    """The banded call against the model, byte for byte: records, and with `traced` paths and ops.  -> the records (and paths,
    op_start, ops)."""
    seq, off = S.batch(prots)
    Sx = A.S62 if matrix is None else np.asarray(matrix, dtype=np.int64)
    want = B.align_model(seq, off, pairs, diags, W, Sx, max_cells=max_cells, **kw)
    if not traced:
        got = _align(seq, off, pairs, band=W, diagonals=diags, matrix=matrix, max_cells=max_cells, **kw)
        assert got.tobytes() == want.tobytes()
        return got
    got = _align(seq, off, pairs, band=W, diagonals=diags, matrix=matrix, max_cells=max_cells, paths=True, ops=mode, **kw)
    assert got[0].tobytes() == want.tobytes()
    pth, starts, ops = B.ops_model(seq, off, pairs, diags, W, want, mode, Sx, **kw)
    assert got[1].tobytes() == pth.tobytes()
    assert got[2].tobytes() == starts.tobytes() and got[3].tobytes() == ops.tobytes()
    return got


# ---- the feature itself ---------------------------------------------------------------------------------------------------------

def test_the_band_keeps_the_alignment_on_its_diagonal_where_the_full_matrix_joins_across_a_long_gap():
    a, b, x_score, joined = B.feature_case()
    seq, off = S.batch([a, b])
    full = _align(seq, off, [(0, 1)])
    assert int(full[0]["score"]) == joined and int(full[0]["end_a"]) >= 60          # the end lies in Y
    rec, pth, starts, ops = _check([a, b], [(0, 1)], [0], 8, mode="eqx")
    assert (int(rec[0]["score"]), int(rec[0]["end_a"]), int(rec[0]["end_b"])) == (x_score, 59, 59)
    assert int(pth[0]["gap_opens"]) == 0 and [int(x) for x in ops] == [60 << 4 | N.OP_EQ]


# ---- rows, widths, windows ------------------------------------------------------------------------------------------------------

ROWS, COLS = (1, 63, 64, 65, 128, 129), (1, 64, 200)


@functools.lru_cache(maxsize=None)
def _grid_proteins():
    """One base protein; a's are its mutated prefixes, b's windows of it: related everywhere, so that the best alignment is long
    and crosses the stripes."""
    rng = np.random.default_rng(64)
    base = A.M.random_protein(rng, 420)
    a_of = {n: A.mutate(rng, base[100:100 + n], 0.1) for n in ROWS}
    b_of = {m: base[100:100 + m] for m in COLS}
    return a_of, b_of


GRID_WIDTHS = [0, 1, 31, 32, 33, 63, 64, 256]


def _grid_case(W):
    """-> (prots, pairs, diags) of test_rows_widths_and_windows at half-width W."""
    a_of, b_of = _grid_proteins()
    prots, pairs, diags = [], [], []
    for k, (n, m) in enumerate((n, m) for n in ROWS for m in COLS):
        # the diagonal of the planted relation is 0.  In turn: on it; beside it; the window clipped at column 0 only (the band's
        # left edge left of the matrix); clipped at column m - 1; beginning exactly at the stripe border row 64; missing the matrix
        # below the last row and right of the last column, and just touching its two corners
        choice = [0, 3, W + 2, -(m - 1) + 1, 64 + W, n + W, -(m + W), n - 1 + W, -(m - 1 + W)]
        for g in (choice[k % len(choice)], choice[(k + 4) % len(choice)], choice[(k + 5 + k // 9) % len(choice)]):
            prots += [a_of[n], b_of[m]]
            pairs.append((len(prots) - 2, len(prots) - 1))
            diags.append(g)
    return prots, pairs, diags


@pytest.mark.parametrize("W", GRID_WIDTHS)
def test_rows_widths_and_windows(W):
    prots, pairs, diags = _grid_case(W)
    rec = _check(prots, pairs, diags, W)[0]
    for (pa, pb), g, r in zip(pairs, diags, rec):
        n, m = len(prots[pa]), len(prots[pb])
        if g - W > n - 1 or g + W < -(m - 1):           # the band misses the matrix
            assert (int(r["score"]), int(r["end_a"]), int(r["end_b"])) == (0, -1, -1)
        if g == 0 and min(n, m) >= 63:                  # the planted relation lies on diagonal 0
            assert int(r["score"]) > 60


def test_any_int32_is_a_diagonal():
    a_of, b_of = _grid_proteins()
    prots = [a_of[129], b_of[200]]
    rec = _check(prots, [(0, 1)] * 4, [2 ** 31 - 1, -2 ** 31, 1 << 25, -(1 << 25)], 256)[0]
    assert list(rec["score"]) == [0] * 4


# ---- gaps at the band's edge ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lp", [30, 61])
@pytest.mark.parametrize("mirror", [False, True])
def test_a_gap_of_six_needs_a_band_of_six(lp, mirror):
    """lp = 61: the insert lies across rows (mirror: columns) 63 / 64."""
    a, b, joined, half = B.insert_case(6, lp, mirror)
    wide = _check([a, b], [(0, 1)], [0], 6)
    assert int(wide[0][0]["score"]) == joined and int(wide[1][0]["gap_opens"]) == 1
    assert int(wide[1][0]["gap_cols_a" if mirror else "gap_cols_b"]) == 6
    narrow = _check([a, b], [(0, 1)], [0], 5)
    assert int(narrow[0][0]["score"]) == half and int(narrow[1][0]["gap_opens"]) == 0


# ---- ties -------------------------------------------------------------------------------------------------------------------------

def test_ties_inside_the_band_and_a_tie_outside_it_that_must_not_win():
    """a's filler is G and b's is D or P: no two different residues used here score above 0.  Y / Y and P / P both score 7."""
    for (a, b, g, W), want in B.tie_cases():
        got = _check([a, b], [(0, 1)], [g], W)
        assert (int(got[0][0]["score"]), int(got[0][0]["end_a"]), int(got[0][0]["end_b"])) == want, (a, b, g, W)


# ---- what an earlier stripe or pair left in LDS ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _stale_batch():
    """kAlignGrid + 400 pairs of a few kinds: long identical pairs (high H and F in every carry slot) that are handed out first,
    and behind them two-stripe pairs whose windows lie left, right and in the middle of those."""
    rng = np.random.default_rng(5)
    long_p = A.M.random_protein(rng, 330)
    base = A.M.random_protein(rng, 200)
    prots = [long_p, long_p, base[:150], A.mutate(rng, base[40:190], 0.1), base[:70], A.mutate(rng, base[:70], 0.2),
             A.mutate(rng, base[20:110], 0.1), base[:100]]
    kinds = [((2, 3), 40), ((2, 3), 37), ((4, 5), 0), ((4, 5), -6), ((7, 6), 20), ((7, 6), 26), ((6, 7), -20), ((5, 4), 3), ((3, 2), -40),
             ((4, 7), 0)]
    pairs, diags = [(0, 1)] * ALIGN_GRID, [0] * ALIGN_GRID
    for k in range(400):
        pairs.append(kinds[k % len(kinds)][0])
        diags.append(kinds[k % len(kinds)][1])
    return prots, pairs, diags


@pytest.mark.parametrize("W", [16, 0, 256])
def test_a_workgroup_s_second_pair_reads_nothing_of_its_first(W):
    prots, pairs, diags = _stale_batch()
    first = _check(prots, pairs, diags, W, traced=False)
    again = _check(prots, pairs, diags, W, traced=False)
    assert first.tobytes() == again.tobytes()
    back = _check(prots, pairs[::-1], diags[::-1], W, traced=False)
    assert back.tobytes() == first[::-1].tobytes()
    shifted = [g + 5 for g in diags]
    _check(prots, pairs, shifted, W, traced=False)
    _check(prots, pairs[-400:], diags[-400:], W)        # the short pairs, traced


# ---- the cap ------------------------------------------------------------------------------------------------------------------------

def test_the_cap_counts_band_cells():
    rng = np.random.default_rng(8)
    p = A.M.random_protein(rng, 300)
    q = A.mutate(rng, p, 0.1)
    seq, off = S.batch([p, q])
    assert int(_align(seq, off, [(0, 1)], max_cells=10000)[0]["status"]) == N.ALIGN_SKIPPED
    got = _check([p, q], [(0, 1)], [0], 8, max_cells=10000)
    assert int(got[0][0]["status"]) == N.ALIGN_ALIGNED and int(got[0][0]["score"]) > 0
    cells = B.band_cells(300, 300, 8)
    assert cells == 300 * 17
    assert int(_check([p, q], [(0, 1)], [0], 8, max_cells=cells)[0][0]["status"]) == N.ALIGN_ALIGNED
    skipped = _check([p, q], [(0, 1)], [0], 8, max_cells=cells - 1)
    assert (int(skipped[0][0]["status"]), int(skipped[0][0]["score"]), int(skipped[1][0]["status"])) == (N.ALIGN_SKIPPED, -1, N.PATH_NONE)
    short = A.M.random_protein(rng, 5)                  # n m below the strip: the full matrix counts
    assert B.band_cells(5, 300, 256) == 1500
    assert int(_check([short, p], [(0, 1)], [0], 256, max_cells=1500)[0][0]["status"]) == N.ALIGN_ALIGNED
    assert int(_check([short, p], [(0, 1)], [0], 256, max_cells=1499)[0][0]["status"]) == N.ALIGN_SKIPPED


# ---- the band's two ends ------------------------------------------------------------------------------------------------------------

def test_a_covering_band_is_the_full_alignment_byte_for_byte():
    rng = np.random.default_rng(21)
    prots, pairs, diags = [], [], []
    for k in range(200):
        n, m = int(rng.integers(1, 150)), int(rng.integers(1, 150))
        a = A.M.random_protein(rng, n)
        prots += [a, A.mutate(rng, (a + A.M.random_protein(rng, m))[int(rng.integers(0, 10)):][:m], 0.2)]
        pairs.append((2 * k, 2 * k + 1))
        diags.append(int(rng.integers(-40, 40)))
    W = max(B.covering(len(prots[a]), len(prots[b]), g) for (a, b), g in zip(pairs, diags))
    assert W <= B.BAND_MAX
    seq, off = S.batch(prots)
    for mode in ("m", "eqx"):
        full = _align(seq, off, pairs, paths=True, ops=mode)
        band = _align(seq, off, pairs, paths=True, ops=mode, band=W, diagonals=diags)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(full, band))
    assert (full[0]["score"] > 0).sum() > 150


def test_all_256_byte_values_and_a_custom_matrix():
    rng = np.random.default_rng(13)
    mat = np.full((21, 21), -3, dtype=np.int64)
    np.fill_diagonal(mat, 5)
    mat[20, :] = mat[:, 20] = -2
    mat[20, 20] = 1
    every = bytes(range(256))
    prots = [every, every[::-1], bytes(rng.permutation(256).astype(np.uint8)), every[3:] + every[:3]]
    pairs = [(0, 1), (0, 2), (0, 3), (3, 0), (2, 2)]
    _check(prots, pairs, [0, 10, 3, -3, 0], 12, matrix=mat, mode="eqx")
    _check(prots, pairs, [0, 10, 3, -3, 0], 12)


# ---- the search ---------------------------------------------------------------------------------------------------------------------

def _check_search(prots, n_db, W, seed=None, min_ungapped=0, paths=None, mode=None, **kw):
    seq, off = S.batch(prots)
    want = B.search_model(seq, off, n_db, W, seed=seed, min_ungapped=min_ungapped, **kw)
    got = _search(seq, off, n_db, seeds=None if seed is None else SD.as_dict(seed), ungapped=dict(min_score=min_ungapped), band=W,
                  paths=paths, ops=mode, **kw)
    hits, start, ung, st = got[0], got[1], got[-1], got[3] if paths else got[2]
    assert start.tobytes() == want[1].tobytes() and hits.tobytes() == want[0].tobytes() and ung.tobytes() == want[2].tobytes()
    assert {k: st[k] for k in S.STAT_KEYS} == want[3]
    assert {k: st["ungapped"][k] for k in UM.UNGAPPED_KEYS} == want[4]
    assert st["band"] == want[5] and st["band"]["full_cells"] == st["cells"]
    if paths:
        pth, starts, ops = B.search_ops_model(seq, off, n_db, W, want[0], want[2], mode or "m", paths)
        assert got[2].tobytes() == pth.tobytes()
        if mode:
            assert got[4].tobytes() == starts.tobytes() and got[5].tobytes() == ops.tobytes()
    return hits, start, ung, st


@pytest.mark.parametrize("batch", range(24))
def test_search_batches_with_indels(batch):
    prots, n_db = B.indel_search(300 + batch, length=90 + 5 * (batch % 7))
    W = (0, 1, 4, 8, 16, 32, 64, 256)[batch % 8]
    seed = SD.REDUCED if batch % 3 == 1 else None
    paths, mode = ((None, None), ("hits", None), ("all", "m"), ("hits", "eqx"))[batch % 4]
    hits, start, ung, st = _check_search(prots, n_db, W, seed=seed, paths=paths, mode=mode, max_cand=3 if batch % 5 == 0 else 8)
    seq, off = S.batch(prots)
    full = _search(seq, off, n_db, seeds=None if seed is None else SD.as_dict(seed), ungapped=True, max_cand=3 if batch % 5 == 0 else 8)
    assert len(hits) == len(full[0]) > 0
    by_pair = {(int(h["query"]), int(h["target"])): int(h["score"]) for h in full[0]}
    for h, u in zip(hits, ung):
        assert int(u["ungapped"]) <= int(h["score"]) <= by_pair[(int(h["query"]), int(h["target"]))]
    if W == 0:
        assert list(hits["score"]) == list(ung["ungapped"])


def test_search_with_a_mask():
    import mask_model as MM
    prots, n_db = MM.planted_search(seed=5, n_targets=8, n_related=4)
    seq, off = S.batch(prots)
    flags = MM.mask_numpy(seq, off)[0]
    seeding = MM.soft_mask(seq, off, flags, *MM.side_range("both", n_db, len(prots)))
    want = B.search_model(seq, off, n_db, 8, seeding=seeding)
    got = _search(seq, off, n_db, ungapped=True, band=8, mask=dict(sides="both"))
    assert got[0].tobytes() == want[0].tobytes() and got[-1].tobytes() == want[2].tobytes() and got[2]["band"] == want[5]


# ---- errors and failures ------------------------------------------------------------------------------------------------------------

def _raw_align(lib, seq, off, pairs, diags, bp, paths=True, ops=True, ops_mode=N.OPS_MODES["m"], device_ptr=None):
    from kmergutsjava_amd import hotpath
    arr = np.frombuffer(seq, dtype=np.uint8)
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    dg = np.ascontiguousarray(np.asarray(diags, dtype=np.int32)) if diags is not None else None
    out, pth = np.zeros(len(pr), dtype=N.ALIGNMENT_DTYPE), np.zeros(len(pr), dtype=N.ALIGN_PATH_DTYPE)
    ap, h = hotpath._align_params()[0], C.c_void_p()
    fn = lib.kg_proteins_align_banded_device if device_ptr else lib.kg_proteins_align_banded
    rc = fn(0, C.byref(ap), device_ptr or arr.ctypes.data, off.ctypes.data, len(off) - 1, pr.ctypes.data, len(pr), 1 << 24, ops_mode,
            out.ctypes.data, pth.ctypes.data if paths else None, C.byref(h) if ops else None, C.byref(bp) if bp is not None else None,
            dg.ctypes.data if dg is not None else None)
    return rc, h, out, pth


def _band(W, reserved=(0, 0, 0)):
    return N.KgBandParams(W, (C.c_int32 * 3)(*reserved))


def test_the_argument_errors_and_the_getter_on_another_call_s_set():
    lib = N.load()
    prots, n_db = B.indel_search(300)
    seq, off = S.batch(prots)
    cases = [(dict(bp=None), b"null kg_band_params"), (dict(bp=_band(-1)), b"band must be in [0, 256]"),
             (dict(bp=_band(257)), b"band must be in [0, 256]"), (dict(bp=_band(8, (0, 0, 1))), b"kg_band_params.reserved must be 0"),
             (dict(bp=_band(8), paths=False), b"ops without paths"), (dict(bp=_band(8), ops=False), b"ops_mode must be 0 without ops"),
             (dict(bp=_band(8), ops_mode=3), b"ops_mode must be KG_TRACE_OPS or KG_TRACE_OPS_EQX"),
             (dict(bp=_band(8), diags=None), b"null diagonals")]
    for kw, words in cases:
        kw = dict(dict(diags=[0]), **kw)
        rc, h, _, _ = _raw_align(lib, seq, off, [(n_db, 0)], **kw)
        assert rc == N.KG_ERR_ARG and lib.kg_last_error().startswith(words), (words, lib.kg_last_error())
        assert not h.value
    from kmergutsjava_amd import hotpath
    p, ap = N.KgSearchParams(2, 8, 256, 0), hotpath._align_params()[0]
    arr = np.frombuffer(seq, dtype=np.uint8)
    up = N.KgUngappedParams(0, (C.c_int32 * 3)())
    for bp, words in ((None, b"null kg_band_params"), (_band(300), b"band must be in [0, 256]"),
                      (_band(1, (1, 0, 0)), b"kg_band_params.reserved must be 0")):
        h = C.c_void_p()
        rc = lib.kg_proteins_search_banded(0, C.byref(p), None, C.byref(ap), arr.ctypes.data, off.ctypes.data, len(off) - 1, n_db, 0, 0, 0, 0,
                                           None, 0, C.byref(up), C.byref(bp) if bp is not None else None, C.byref(h))
        assert rc == N.KG_ERR_ARG and lib.kg_last_error().startswith(words) and not h.value
    h = C.c_void_p()
    rc = lib.kg_proteins_search_banded(0, C.byref(p), None, C.byref(ap), arr.ctypes.data, off.ctypes.data, len(off) - 1, n_db, 0, 0, 0, 0, None, 0,
                                       None, C.byref(_band(8)), C.byref(h))
    assert rc == N.KG_ERR_ARG and lib.kg_last_error().startswith(b"null kg_ungapped_params")
    with pytest.raises(ValueError):
        _search(seq, off, n_db, band=8)
    h = C.c_void_p()
    assert lib.kg_proteins_search_filtered(0, C.byref(p), None, C.byref(ap), arr.ctypes.data, off.ctypes.data, len(off) - 1, n_db, 0, 0, 0, 0, None,
                                           0, C.byref(up), C.byref(h)) == N.KG_OK
    try:
        st = N.KgBandStats()
        assert lib.kg_hitset_band_stats(h, C.byref(st)) == N.KG_ERR_ARG and b"without a band" in lib.kg_last_error()
    finally:
        lib.kg_hitset_free(h)


def test_the_device_entry_points_scores_only_and_empty_calls():
    import torch
    lib = N.load()
    prots, n_db = B.indel_search(301)
    seq, off = S.batch(prots)
    pairs = [(n_db + q, q) for q in range(5)]
    diags = [0, 2, -3, 1, 0]
    want = _check(prots, pairs, diags, 16, mode="eqx")
    dev = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    got = _align(None, off, pairs, band=16, diagonals=diags, paths=True, ops="eqx", device_ptr=dev.data_ptr())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(want, got))
    only = _align(None, off, pairs, band=16, diagonals=diags, device_ptr=dev.data_ptr())
    assert only.tobytes() == want[0].tobytes()
    both = _align(seq, off, pairs, band=16, diagonals=diags, paths=True)
    assert both[0].tobytes() == want[0].tobytes() and both[1].tobytes() == want[1].tobytes()
    wanted = _check_search(prots, n_db, 16, paths="hits", mode="m")
    sgot = _search(None, off, n_db, ungapped=True, band=16, paths="hits", ops="m", device_ptr=dev.data_ptr())
    assert sgot[0].tobytes() == wanted[0].tobytes() and sgot[-1].tobytes() == wanted[2].tobytes()
    assert dev.cpu().numpy().tobytes() == seq
    none = _align(seq, off, np.zeros((0, 2), dtype=np.int32), band=4, diagonals=[], paths=True, ops="m")
    assert len(none[0]) == 0 and list(none[2]) == [0] and len(none[3]) == 0
    empty = _search(b"", np.zeros(1, dtype=np.int64), 0, ungapped=True, band=4)
    assert len(empty[0]) == 0 and empty[2]["band"] == dict(band_cells=0, full_cells=0, band=4)
    rc, h, out, _ = _raw_align(lib, seq, off, pairs, diags, _band(16), paths=False, ops=False, ops_mode=0)
    assert rc == N.KG_OK and out.tobytes() == want[0].tobytes()


def test_every_allocation_failed_in_turn_gives_the_memory_back(monkeypatch):
    import torch
    from kmergutsjava_amd import hotpath, synth
    prots, n_db = B.indel_search(302)
    seq, off = S.batch(prots)
    pairs = [(n_db + q, q) for q in range(5)]
    diags = [0] * 5
    rec = synth.high_density_config(4, 100, 4001, 500, dna=False)[2]
    with hotpath.SignatureTable.from_bytes(synth.table_image(rec), 0) as tab:
        calls = (lambda: _align(seq, off, pairs, band=8, diagonals=diags, paths=True, ops="m"),
                 lambda: _search(seq, off, n_db, ungapped=True, band=8, paths="hits", ops="m"))
        for call, at_least in zip(calls, (10, 80)):
            want = call()
            torch.cuda.synchronize()
            free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
            failed = 0
            for n in range(1, 900):
                monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
                try:
                    got = call()
                    break
                except N.KmerGutsNativeError as e:
                    assert e.code == N.KG_ERR_NOMEM, e
                    failed += 1
                    assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
                    assert tab.live_device_bytes() == live0
            monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
            assert failed >= at_least and all(x.tobytes() == y.tobytes() for x, y in zip(want, got) if isinstance(x, np.ndarray))
            assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0


# ---- the front end ------------------------------------------------------------------------------------------------------------------

def test_the_command_line_on_mutated_proteins_of_the_golden_proteome_with_an_indel_each(tmp_path):
    from kmergutsjava_amd import search_proteins as SP
    import gzip
    from kmergutsjava_amd.make_signatures import parse_fasta
    ids, prots = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))
    pick = [k for k in range(0, len(ids), len(ids) // 400) if 60 <= len(prots[k]) <= 400][:192]
    ids, prots = [ids[k] for k in pick], [bytes(prots[k]) for k in pick]
    assert len(ids) == 192
    rng = np.random.default_rng(9)
    muts = []
    for p in prots:
        m = A.mutate(rng, p, 0.1)
        at, k = int(rng.integers(20, len(m) - 20)), int(rng.integers(1, 11))
        muts.append(m[:at] + (A.M.random_protein(rng, k) if rng.random() < 0.5 else b"") + m[at + (k if len(muts) % 2 else 0):])
    db, qs, out = tmp_path / "db.faa", tmp_path / "q.faa", tmp_path / "hits.tsv"
    db.write_bytes(b"".join(b">" + i + b"\n" + p + b"\n" for i, p in zip(ids, prots)))
    qs.write_bytes(b"".join(b">" + i + b"_m\n" + p + b"\n" for i, p in zip(ids, muts)))
    run = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.search_proteins", "-d", str(db), "-q", str(qs), "-o", str(out),
                          "--seeds", "reduced", "--ungapped", "--band", "32", "--paths", "--cigar"], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr
    seq, off = S.batch(prots + muts)
    want = B.search_model(seq, off, 192, 32, seed=SD.REDUCED)
    pth, starts, ops = B.search_ops_model(seq, off, 192, 32, want[0], want[2], "m", "hits")
    assert out.read_bytes() == SP.format_hits([i + b"_m" for i in ids], ids, want[0], want[1], paths=pth, qlens=[len(x) for x in muts],
                                              dlens=[len(x) for x in prots], cigars=(starts, ops), ungapped=want[2])
    assert ", band: 32, band cells: %d of %d" % (want[5]["band_cells"], want[5]["full_cells"]) in run.stderr
    assert (want[0]["status"] == N.SEARCH_HIT).sum() >= 150
