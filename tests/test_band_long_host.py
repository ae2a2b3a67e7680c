"""The inputs of tests/test_gpu_band_long.py on the CPU (tests/band_long_cases.py): the borders they are built around, read from
the headers, with the lines of trace_run and align_band_kernel that the cases restate; each case reaches the path it names, by
those restated rules; the model's two forms on the long shapes; the arithmetic of the pair over the default cap; and two
deliberately wrong models (a stripe carry addressed by absolute column, in the alignment pass and in the traced box), which the
long cases tell from the right one and the inputs of tests/test_gpu_band.py cannot."""
import numpy as np
import pytest

import align_model as A
import band_long_cases as L
import band_model as B
import search_model as S
import seed_model as SD
import test_gpu_band as SHORT
import trace_model as T
import ungapped_model as UM
from kmergutsjava_amd import _native as N


def _pair(case, k):
    (pa, pb), g = case.pairs[k], case.diags[k]
    return case.prots[pa], case.prots[pb], g


# ---- the constants and the restated lines ---------------------------------------------------------------------------------------

def test_the_constants_and_the_lines_the_cases_restate():
    assert (L.WAVE, L.WORD) == (64, 8) and L.LDS_COLS == N.ALIGN_LDS_COLS and L.BAND_MAX == N.BAND_MAX == B.BAND_MAX
    assert L.CARRY_COLS == 2 * L.BAND_MAX + L.WAVE < L.LDS_COLS and L.SHORT_SLAB < L.SLAB and 1 <= L.LONG_GRID <= L.GRID
    host, band, trace = L._text("kg_host_trace.hpp"), L._text("kg_band.hpp"), L._text("kg_trace.hpp")
    assert "const uint64_t w = go ? (na + kg::kWave - 1) / kg::kWave * kg::trace_stripe_words(mb) : 0;" in host
    assert "const bool lng = go && (mb > (uint64_t)kg::kAlignLdsCols || w * 4 > kTraceShortSlabBytes);" in host
    assert "if (lng) carry_cols = std::max(carry_cols, (mb + 63) / 64 * 64);" in host
    assert "{n_long, (uint64_t)kTraceLongGrid, std::max<uint64_t>(1, kTraceSlabBytes / std::max<uint64_t>(words[1] * 4 + carry_cols * 8, 1))}" in host
    assert "kg::trace_band_columns_kernel<true>, dim3(long_grid)" in host and "kg::trace_band_kernel<true>, dim3(long_grid)" in host
    assert "return (mb + kWave - 1 + kTraceCellsPerWord - 1) / kTraceCellsPerWord * kWave;" in trace
    assert "const int r_lo = max(0, g - band), r_hi = min(n - 1, m - 1 + g + band);" in band and "const int i_start = r_lo & ~(kWave - 1);" in band
    assert "const int c_lo = max(0, i0 - g - band), c_hi = min(m - 1, min(i0 + kWave - 1, n - 1) - g + band);" in band
    assert "const int c_lo_prev = max(0, i0 - kWave - g - band);" in band and "lds_carry[col - c_lo_prev]" in band
    assert "__shared__ int2 lds_carry[kBandCarryCols];" in band and "__shared__ int2 lds_carry[kLong ? 1 : kAlignLdsCols];" in trace
    # the stripe windows by hand: three stripes of case A at W = 16
    assert [tuple(s) for s in L.band_stripes(130, 1300, -1150, 16)] == [(0, 1134, 1229, None), (64, 1198, 1293, 1134), (128, 1262, 1295, 1198)]
    assert L.band_stripes(130, 1300, 200, 16) == [] and L.band_stripes(5, 0, 0, 4) == []
    assert L.trace_stripe_words(1000) == 8512 and L.trace_launch(960, 1000) is None and L.trace_launch(961, 1000) == "slab"
    assert L.trace_launch(1, L.LDS_COLS) is None and L.trace_launch(1, L.LDS_COLS + 1) == "columns"


# ---- each case reaches what it names --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", L.A_WIDTHS)
def test_case_a_lies_right_of_the_carry_and_is_traced_by_the_second_launch(W):
    case = L.case_a(W)
    a, b = case.prots
    assert (len(a), len(b)) == (130, 1300)
    for k in range(3):
        g = case.diags[k]
        stripes = L.band_stripes(len(a), len(b), g, W)
        assert len(stripes) == 3 and all(s.c_lo > L.CARRY_COLS for s in stripes)
        assert L.carried_right_of_the_carry(len(a), len(b), g, W) == 2
        end = L.model(a, b, g, W)[0]
        if W > 0 or k == 0:                             # (the planted relation is in the band)
            assert end[0] > 500 and end[1] >= 2 * L.WAVE and end[2] >= L.LDS_COLS, end
            assert L.trace_launch(end[1] + 1, end[2] + 1) == "columns"
    stripes = L.band_stripes(len(b), len(a), case.diags[3], W)
    assert stripes[0].i0 == (1088 if W < 63 else (1150 - W) & ~63) and stripes[0].c_lo == 0 and stripes[-1].c_hi == len(a) - 1
    end = L.model(b, a, case.diags[3], W)[0]
    assert end == (L.model(a, b, case.diags[0], W)[0][0], 1279, 129) and L.trace_launch(end[1] + 1, end[2] + 1) is None


@pytest.mark.parametrize("m", L.B_COLS)
def test_case_b_ends_in_the_last_column(m):
    case = L.case_b(m)
    for k, n in enumerate(L.B_ROWS):
        a, b, g = _pair(case, k)
        end, rec, _ = L.model(a, b, g, case.W)
        assert (len(a), len(b)) == (n, m) and end[1:] == (n - 1, m - 1) and rec[2] >= min(n, 30)
        assert L.trace_launch(n, m) == ("columns" if m > L.LDS_COLS else None)
    assert L.B_COLS[:3] == (L.LDS_COLS - 1, L.LDS_COLS, L.LDS_COLS + 1)


@pytest.mark.parametrize("lp", L.C_LENGTHS)
@pytest.mark.parametrize("mirror", [False, True])
def test_case_c_moves_the_window_past_the_carry_and_the_lds_columns(lp, mirror):
    a, b, joined, half = L.case_c_insert(lp, mirror)
    for W, want in ((6, joined), (5, half)):
        stripes = L.band_stripes(len(a), len(b), 0, W)
        assert len(stripes) == (len(a) + 63) // 64 >= 11 and L.carried_right_of_the_carry(len(a), len(b), 0, W) >= 1
        end, rec, cols = L.model(a, b, 0, W)
        assert end[0] == want == {(700, 6): 7731, (700, 5): 7700, (1100, 6): 12131, (1100, 5): 12100}[(lp, W)]
        assert rec[4] == (1 if W == 6 else 0) and rec[5] + rec[6] == (6 if W == 6 else 0)
        if W == 6:                                      # the gap lies past the carry's size (lp = 700) and the LDS columns (lp = 1100)
            at = cols[::-1].index("E" if mirror else "F")
            assert at == lp > (L.CARRY_COLS if lp == 700 else L.LDS_COLS)
        assert L.trace_launch(end[1] + 1, end[2] + 1) == ("columns" if lp == 1100 else None)


@pytest.mark.parametrize("W", L.C_INDEL_WIDTHS)
def test_case_c_s_realistic_path_crosses_the_lds_columns_with_gaps(W):
    case = L.case_c_indels(W)
    a, b, g = _pair(case, 0)
    end, rec, cols = L.model(a, b, g, W)
    assert len(a) == 1100 and rec[1] < L.CARRY_COLS and end[2] >= L.LDS_COLS and L.trace_launch(end[1] + 1, end[2] + 1) == "columns"
    assert rec[4] >= 5 and rec[5] > 0 and rec[6] > 0
    assert L.carried_right_of_the_carry(len(a), len(b), g, W) >= 5


def test_case_d_falls_on_both_sides_of_the_slab_border():
    case = L.case_d()
    lo, hi = L.d_rows()
    words = L.trace_stripe_words(L.D_COLS) * 4
    assert hi == lo + L.WAVE and lo // L.WAVE * words <= L.SHORT_SLAB < hi // L.WAVE * words and (lo, hi) == (960, 1024)
    for k, n in enumerate((lo, hi)):
        a, b, g = _pair(case, k)
        end = L.model(a, b, g, case.W)[0]
        assert (len(a), len(b)) == (n, L.D_COLS) and end[1:] == (n - 1, L.D_COLS - 1) and L.D_COLS <= L.LDS_COLS
        assert L.trace_launch(end[1] + 1, end[2] + 1) == (None if n == lo else "slab")


@pytest.mark.parametrize("shift", [0, 5])
def test_case_e_has_more_long_boxes_than_workgroups(shift):
    case = L.case_e(shift)
    n_long, long_grid = L.trace_long_grid(L.boxes_of(case))
    assert n_long == L.E_LONG > long_grid == L.LONG_GRID
    assert len(case.pairs) == L.E_LONG + L.E_SHORT and len({(p, g) for p, g in zip(case.pairs, case.diags) if p == (0, 1)}) == 3
    assert case.pairs[0] != (0, 1) != case.pairs[-1]


@pytest.mark.parametrize("W", L.G_WIDTHS)
@pytest.mark.parametrize("seed", [None, SD.REDUCED], ids=["exact", "reduced"])
def test_case_g_s_long_queries_hit_their_targets_on_long_diagonals(W, seed):
    prots, n_db = L.case_g()
    assert [len(p) for p in prots[:2]] == [1100, 1300] and n_db == 6 and len(prots) == 10
    seq, off = S.batch(prots)
    hits, start, ung = B.search_model(seq, off, n_db, W, seed=seed)[:3]
    for q in range(2):
        h, u = hits[start[q]], ung[start[q]]
        assert (int(h["query"]), int(h["target"]), int(h["rank"]), int(h["status"])) == (q, q, 0, N.SEARCH_HIT)
        assert UM.cells_of(len(prots[n_db + q]), len(prots[q]), int(u["diagonal"])) > L.LDS_COLS
        assert int(u["ungapped"]) < int(h["score"])                                 # the indels cost the diagonal something
        assert L.trace_launch(int(h["end_query"]) + 1, int(h["end_target"]) + 1) == "columns"
        assert L.carried_right_of_the_carry(len(prots[n_db + q]), len(prots[q]), int(u["diagonal"]), W) >= 5
    # the short relatives: indels of up to 10 residues, so a band of 8 may keep one of them below the ratio
    assert len(hits) - start[2] == 2 and (hits["status"][start[2]:] == N.SEARCH_HIT).sum() >= (2 if W == 64 else 1)


# ---- the model's forms on the long shapes -------------------------------------------------------------------------------------

def test_loops_numpy_and_rows_agree_on_the_long_shapes():
    case = L.case_a(16)
    for k in range(4):
        a, b, g = _pair(case, k)
        end, rec, cols = L.model(a, b, g, 16)
        assert B.band_loops(a, b, g, 16) == B.band_numpy(a, b, g, 16) == end
        assert L.rows_result(a, b, g, 16) == (end, (rec, cols))
    case = L.case_b(L.LDS_COLS + 1)
    a, b, g = _pair(case, 3)
    assert len(a) == 129 and B.band_loops(a, b, g, case.W) == B.band_numpy(a, b, g, case.W) == L.model(a, b, g, case.W)[0]
    # the row-wise form, the walk over its direction bits included, on gaps of both kinds
    for case in (L.case_c_indels(32), L.case_d()):
        for k in range(len(case.pairs)):
            a, b, g = _pair(case, k)
            end, rec, cols = L.model(a, b, g, case.W)
            assert L.rows_result(a, b, g, case.W) == (end, (rec, cols))
    rng = np.random.default_rng(7)
    for _ in range(40):
        a = A.M.random_protein(rng, int(rng.integers(1, 150)))
        b = B.with_indels(rng, A.mutate(rng, a, 0.2), every=20, longest=4) if rng.random() < 0.8 else A.M.random_protein(rng, 90)
        g, W = int(rng.integers(-6, 7)), int(rng.integers(0, 12))
        end, rec, cols = B.band_trace(a, b, g, W)
        assert L.rows_result(a, b, g, W) == (end, (rec, cols) if rec is not None else None)


# ---- the pair over the default cap --------------------------------------------------------------------------------------------

def test_case_f_s_arithmetic():
    n = L.F_N
    assert (n - 1) ** 2 == L.MAX_CELLS == 1 << 26 < n * n and L.MAX_TRACE_CELLS == 1 << 24 == 4096 ** 2 < n * n
    for W in L.F_WIDTHS:
        assert B.band_cells(n, n, W) == n * (2 * W + 1) <= L.MAX_CELLS
    assert L.trace_launch(n, n) == "columns" == L.trace_launch(4096, 4096)
    assert L.carried_right_of_the_carry(n, n, 0, 32) >= 100
    # the full diagonal is the one best alignment of a protein with itself: every diagonal entry of BLOSUM62 is positive, and no
    # entry off the diagonal is above either diagonal entry of its row and its column
    S62 = A.S62[:20, :20]
    diag = np.diag(S62)
    assert diag.min() >= 4 and (S62 <= np.minimum(diag[:, None], diag[None, :])).all()
    p = L.f_protein(2000)
    assert set(p) <= set(A.ALPHA)
    for W in L.F_WIDTHS:
        assert B.band_numpy(p, p, 0, W) == (A.self_score(p), 1999, 1999)
    end, rec, cols = B.band_trace(p[:300], p[:300], 0, 32)
    assert rec == (0, 0, 300, 300, 0, 0, 0) and cols == "M" * 300


# ---- what an absolutely addressed carry would lose ----------------------------------------------------------------------------

def test_the_long_cases_see_a_carry_addressed_by_absolute_column():
    """(i) the alignment pass with kBandCarryCols slots, (ii) the traced box with kAlignLdsCols slots."""
    long_pairs = [(L.case_a(W).prots[0], L.case_a(W).prots[1], L.A_DIAG, W) for W in L.A_WIDTHS]
    long_pairs += [L.case_c_insert(lp, mirror)[:2] + (0, 6) for lp in L.C_LENGTHS for mirror in (False, True)]
    long_pairs += [_pair(L.case_c_indels(32), 0) + (32,)]
    for a, b, g, W in long_pairs:
        right = L.rows_result(a, b, g, W)
        assert right[1] not in (None, "score")
        assert L.rows_result(a, b, g, W, lost_align=L.CARRY_COLS)[0] != right[0], (len(a), len(b), g, W)
        if max(len(a), len(b)) > L.LDS_COLS:
            assert L.rows_result(a, b, g, W, lost_trace=L.LDS_COLS) != right, (len(a), len(b), g, W)
    case = L.case_b(L.LDS_COLS + 2)
    for k in (2, 3):                                    # 65 and 129 rows: the path steps over rows 63 / 64 and 127 / 128 behind column LDS_COLS
        a, b, g = _pair(case, k)
        assert L.rows_result(a, b, g, case.W, lost_trace=L.LDS_COLS) != L.rows_result(a, b, g, case.W)
    case = L.case_d()                                   # (the slab rule's boxes: long in rows and in the carry, not in columns)
    for k in range(2):
        a, b, g = _pair(case, k)
        assert L.rows_result(a, b, g, case.W, lost_align=L.CARRY_COLS)[0] != L.rows_result(a, b, g, case.W)[0]


def test_the_short_inputs_cannot_see_it():
    seen = set()
    for W in SHORT.GRID_WIDTHS:
        prots, pairs, diags = SHORT._grid_case(W)
        seen |= {(prots[pa], prots[pb], g, W) for (pa, pb), g in zip(pairs, diags)}
    prots, pairs, diags = SHORT._stale_batch()
    seen |= {(prots[pa], prots[pb], g + s, W) for (pa, pb), g in set(zip(pairs, diags)) for W in (16, 0, 256) for s in (0, 5)}
    assert len(seen) > 400 and max(len(b) for _, b, _, _ in seen) < L.CARRY_COLS
    for a, b, g, W in sorted(seen):
        right = L.rows_result(a, b, g, W)
        assert L.rows_result(a, b, g, W, lost_align=L.CARRY_COLS, lost_trace=L.LDS_COLS) == right
    go, ge = B._caps(11, 1)
    for a, b, g, W in sorted(seen)[1::40]:              # ... and the row-wise form is the model's on them
        H, E, F = B.tables_numpy(T._codes(a), T._codes(b), g, W, A.S62, go, ge)
        Hr, Er, Fr, _ = L.tables_rows(T._codes(a), T._codes(b), g, W, A.S62, go, ge)
        assert (H == Hr).all() and (E[1:, 1:] == Er[1:, 1:]).all() and (F[1:, 1:] == Fr[1:, 1:]).all()
