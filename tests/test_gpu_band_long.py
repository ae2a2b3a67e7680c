"""kg_proteins_align_banded and kg_proteins_search_banded on proteins of more than a thousand residues (the cases of
tests/band_long_cases.py; tests/test_band_long_host.py shows on the CPU that each reaches the path it names): align_band_kernel
with windows right of its carry and after many window moves, trace_band_kernel<true> and trace_band_columns_kernel<true> by
their two launch rules and with a slab used twice, a pair over the default cell cap, and the banded search on diagonals of more
than 1024 cells.  Everything is compared with tests/band_model.py byte for byte through test_gpu_band's _check and _check_search,
except the pair over the cap, whose answer follows from how it is made."""
import numpy as np
import pytest

import align_model as A
import band_long_cases as L
import band_model as B
import search_model as S
import seed_model as SD
import trace_model as T
import ungapped_model as UM
from kmergutsjava_amd import _native as N
from test_gpu_band import _align, _check, _check_search

pytestmark = pytest.mark.gpu


def _both_modes(case, **kw):
    """The case against the model with ops in both modes, its paths without ops (trace_band_kernel in the columns kernel's
    place) and its records alone.  -> (records, paths)"""
    got = _check(case.prots, case.pairs, case.diags, case.W, mode="m", **kw)
    eqx = _check(case.prots, case.pairs, case.diags, case.W, mode="eqx", **kw)
    assert got[0].tobytes() == eqx[0].tobytes() and got[1].tobytes() == eqx[1].tobytes()
    seq, off = S.batch(case.prots)
    plain = _align(seq, off, case.pairs, band=case.W, diagonals=case.diags, paths=True, **kw)
    assert plain[0].tobytes() == got[0].tobytes() and plain[1].tobytes() == got[1].tobytes()
    only = _align(seq, off, case.pairs, band=case.W, diagonals=case.diags, **kw)
    assert only.tobytes() == got[0].tobytes()
    return got[0], got[1]


def _launches(rec, pth):
    """trace_run's launch of every traced record, by the restated rule."""
    return [L.trace_launch(int(r["end_a"]) + 1, int(r["end_b"]) + 1) if int(p["status"]) == N.PATH_TRACED else "untraced" for r, p in zip(rec, pth)]


# ---- A: windows right of the carry ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", L.A_WIDTHS)
def test_a_window_far_right_of_the_carry(W):
    case = L.case_a(W)
    rec, pth = _both_modes(case)
    assert _launches(rec[:1], pth[:1]) == ["columns"] and int(rec[0]["end_b"]) >= L.LDS_COLS and int(rec[0]["end_a"]) >= 2 * L.WAVE
    assert (int(rec[3]["score"]), int(rec[3]["end_a"]), int(rec[3]["end_b"])) == (int(rec[0]["score"]), int(rec[0]["end_b"]), int(rec[0]["end_a"]))
    assert int(pth[3]["start_a"]) == int(pth[0]["start_b"]) >= L.LDS_COLS
    if W == 16:                                         # once through the device-pointer entry
        import torch
        seq, off = S.batch(case.prots)
        dev = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        want = _align(seq, off, case.pairs, band=W, diagonals=case.diags, paths=True, ops="eqx")       # (checked above)
        got = _align(None, off, case.pairs, band=W, diagonals=case.diags, paths=True, ops="eqx", device_ptr=dev.data_ptr())
        assert want[0].tobytes() == rec.tobytes() and want[1].tobytes() == pth.tobytes() and len(want[3]) > 0
        assert all(x.tobytes() == y.tobytes() for x, y in zip(want, got))
        assert dev.cpu().numpy().tobytes() == seq


# ---- B: box columns at the LDS border -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", L.B_COLS)
def test_b_box_columns_at_the_lds_border(m):
    rec, pth = _both_modes(L.case_b(m))
    assert (rec["end_b"] == m - 1).all() and rec["end_a"].tolist() == [n - 1 for n in L.B_ROWS] and (pth["status"] == N.PATH_TRACED).all()
    assert _launches(rec, pth) == ["columns" if m > L.LDS_COLS else None] * len(L.B_ROWS)
    assert pth["identical"][0] == 1 and (pth["identical"][1:] >= 30).all()


# ---- C: a long diagonal, many window moves --------------------------------------------------------------------------------------

@pytest.mark.parametrize("lp", L.C_LENGTHS)
@pytest.mark.parametrize("mirror", [False, True])
def test_c_a_gap_of_six_behind_a_long_diagonal(lp, mirror):
    a, b, joined, half = L.case_c_insert(lp, mirror)
    rec, pth = _both_modes(L.Case([a, b], [(0, 1)], [0], 6, ""))
    assert int(rec[0]["score"]) == joined and int(pth[0]["gap_opens"]) == 1
    assert int(pth[0]["gap_cols_a" if mirror else "gap_cols_b"]) == 6 and (int(pth[0]["start_a"]), int(pth[0]["start_b"])) == (0, 0)
    narrow, npth = _both_modes(L.Case([a, b], [(0, 1)], [0], 5, ""))
    assert int(narrow[0]["score"]) == half == 11 * lp and int(npth[0]["gap_opens"]) == 0
    assert _launches(rec, pth) == _launches(narrow, npth) == ["columns" if lp > L.LDS_COLS else None]


@pytest.mark.parametrize("W", L.C_INDEL_WIDTHS)
def test_c_a_path_with_several_gaps_across_the_lds_columns(W):
    rec, pth = _both_modes(L.case_c_indels(W))
    assert _launches(rec, pth) == ["columns"] and int(pth[0]["start_b"]) < L.CARRY_COLS and int(pth[0]["gap_opens"]) >= 5


# ---- D: the second launch by the size of the direction words --------------------------------------------------------------------

def test_d_the_slab_rule_below_the_lds_columns():
    case = L.case_d()
    rec, pth = _both_modes(case)
    lo, hi = L.d_rows()
    assert rec["end_a"].tolist() == [lo - 1, hi - 1] and rec["end_b"].tolist() == [L.D_COLS - 1] * 2
    assert _launches(rec, pth) == [None, "slab"]
    for k in range(2):                                  # each alone: the call's slab is then the pair's own
        one = L.Case(case.prots, case.pairs[k:k + 1], case.diags[k:k + 1], case.W, "")
        assert _check(one.prots, one.pairs, one.diags, one.W, mode="eqx")[1].tobytes() == pth[k:k + 1].tobytes()


# ---- E: a long launch that uses its slabs twice ---------------------------------------------------------------------------------

def test_e_a_workgroup_s_second_long_box_reads_nothing_of_its_first():
    case = L.case_e()
    seq, off = S.batch(case.prots)
    first = _check(case.prots, case.pairs, case.diags, case.W, mode="m")
    assert _launches(first[0], first[1]).count("columns") == L.E_LONG > L.LONG_GRID
    again = _align(seq, off, case.pairs, band=case.W, diagonals=case.diags, paths=True, ops="m")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
    plain = _align(seq, off, case.pairs, band=case.W, diagonals=case.diags, paths=True)
    assert plain[0].tobytes() == first[0].tobytes() and plain[1].tobytes() == first[1].tobytes()
    back = _check(case.prots, case.pairs[::-1], case.diags[::-1], case.W, mode="eqx")
    assert back[0].tobytes() == first[0][::-1].tobytes() and back[1].tobytes() == first[1][::-1].tobytes()
    shifted = L.case_e(5)
    moved = _check(shifted.prots, shifted.pairs, shifted.diags, shifted.W, mode="eqx")
    assert _launches(moved[0], moved[1]).count("columns") == L.E_LONG


# ---- F: a pair over the default cell cap ----------------------------------------------------------------------------------------

def test_f_a_pair_the_full_call_skips_is_aligned_and_traced_under_the_band():
    """p against itself: the one best local alignment is the whole diagonal (tests/test_band_long_host.py).  The traced variant
    runs at n = 8193, a box of 67 million cells in one wave."""
    n, p = L.F_N, L.f_protein()
    seq, off = S.batch([p])
    own = A.self_score(p)
    full = _align(seq, off, [(0, 0)])
    assert (int(full[0]["status"]), int(full[0]["score"])) == (N.ALIGN_SKIPPED, -1)
    for W in L.F_WIDTHS:
        assert B.band_cells(n, n, W) == n * (2 * W + 1) <= L.MAX_CELLS < n * n
        rec = _align(seq, off, [(0, 0)], band=W, diagonals=[0])
        assert tuple(int(x) for x in rec[0]) == (own, own, own, n - 1, n - 1, N.ALIGN_ALIGNED)
        over = _align(seq, off, [(0, 0)], band=W, diagonals=[0], paths=True, ops="eqx")        # the default max_trace_cells
        assert over[0].tobytes() == rec.tobytes() and tuple(int(x) for x in over[1][0]) == T.NO_PATH + (N.PATH_UNTRACED,)
        assert over[2].tolist() == [0, 0] and len(over[3]) == 0
        for mode, code in (("eqx", N.OP_EQ), ("m", N.OP_M)):
            got = _align(seq, off, [(0, 0)], band=W, diagonals=[0], paths=True, ops=mode, max_trace_cells=n * n)
            assert got[0].tobytes() == rec.tobytes() and tuple(int(x) for x in got[1][0]) == (0, 0, n, n, 0, 0, 0, N.PATH_TRACED)
            assert got[2].tolist() == [0, 1] and got[3].tolist() == [n << 4 | code]
        plain = _align(seq, off, [(0, 0)], band=W, diagonals=[0], paths=True, max_trace_cells=n * n)
        assert plain[0].tobytes() == rec.tobytes() and plain[1].tobytes() == got[1].tobytes()
        assert tuple(int(x) for x in _align(seq, off, [(0, 0)], band=W, diagonals=[0], paths=True, max_trace_cells=n * n - 1)[1][0]) == \
            T.NO_PATH + (N.PATH_UNTRACED,)


# ---- G: the search --------------------------------------------------------------------------------------------------------------

G_CALLS = [(W, seed, "hits", mode) for W in L.G_WIDTHS for seed in ("exact", "reduced") for mode in ("m", "eqx")] + [(64, "exact", "all", "m")]


@pytest.mark.parametrize("W,seed,paths,mode", G_CALLS)
def test_g_the_search_on_diagonals_of_more_than_1024_cells(W, seed, paths, mode):
    prots, n_db = L.case_g()
    hits, start, ung, st = _check_search(prots, n_db, W, seed=SD.REDUCED if seed == "reduced" else None, paths=paths, mode=mode)
    for q in range(2):
        h, u = hits[start[q]], ung[start[q]]
        assert (int(h["query"]), int(h["target"]), int(h["rank"]), int(h["status"])) == (q, q, 0, N.SEARCH_HIT)
        assert UM.cells_of(len(prots[n_db + q]), len(prots[q]), int(u["diagonal"])) > L.LDS_COLS
        assert L.trace_launch(int(h["end_query"]) + 1, int(h["end_target"]) + 1) == "columns"
    assert st["traced"] >= 3 and st["untraced"] == 0
