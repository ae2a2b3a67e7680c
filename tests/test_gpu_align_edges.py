"""kg_proteins_align and the alignment step of kg_proteins_cluster_aligned on their internal borders (kg_align.hpp,
kg_host_align.hpp): a workgroup's second pair in both launches, b of 1023, 1024 and 1025 residues between the LDS carry and the
slab, the slab's stride under the cap on its bytes, ties of the best cell, every byte value and score tables at +-16, the
device entry point, and align_cut_kernel's counts at wave and workgroup sizes with its three statuses mixed.

The inputs and, where there is one, their answers by construction come from tests/align_edge_cases.py;
tests/test_align_edges_host.py checks the model against those answers and the shapes against the headers' constants on the CPU.
Here every device result must equal align_model.align_model / cluster_aligned_model (the numpy form) byte for byte: integers
only, no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import align_edge_cases as E  # noqa: E402
import cluster_model as M  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
ALIGN_COUNTS = ("aligned", "cut", "skipped", "cells")


def _align(prots, pairs, device=False, **kw):
    from kmergutsjava_amd import hotpath
    seq, off = M.pack(prots)
    if not device:
        return hotpath.align_proteins(seq, off, pairs, **kw)
    d = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    return hotpath.align_proteins(None, off, pairs, device_ptr=d.data_ptr(), **kw)


def _equal(got, want, what=""):
    bad = np.flatnonzero(got != want)
    assert got.tobytes() == want.tobytes(), (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _same(prots, pairs, want=None, device=False, what="", **kw):
    """The device's records == the model's (want: the model's, where the caller has them).  -> the records"""
    if want is None:
        want = E.model(prots, pairs, **kw)
    got = _align(prots, pairs, device=device, **kw)
    _equal(got, want, what)
    return got


def _triple(rec):
    return int(rec["score"]), int(rec["end_a"]), int(rec["end_b"])


# ---- A. a workgroup's second pair -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def short_call():
    prots, pairs, max_cells = E.second_pair_short()
    return prots, pairs, max_cells, E.model(prots, pairs, max_cells=max_cells)


@pytest.fixture(scope="module")
def long_call():
    prots, pairs = E.second_pair_long()
    return prots, pairs, E.model(prots, pairs)


def test_a_second_pair_in_the_short_launch(short_call):
    """Gap 1, the short launch: kAlignGrid + 400 pairs for kAlignGrid workgroups, so the hand-out loop goes round: lds_carry
    holds the pair before's last row, run_* its best cell, and the wave meets at wave_barrier in front of the counter.  The
    pairs handed out last are the skipped ones (their self-scores must still be right), pairs of one or two residues, and
    pairs of 65 x 63 that read the carry.  Twice, and with the list reversed (the stable order of equal cells changes)."""
    prots, pairs, max_cells, want = short_call
    assert len(pairs) > E.GRID
    got = _same(prots, pairs, want, max_cells=max_cells)
    skipped = got["status"] == N.ALIGN_SKIPPED
    assert 150 < skipped.sum() < 250 and (got["self_a"][skipped] > 400).all() and (got["self_b"][skipped] > 400).all()
    _same(prots, pairs, want, max_cells=max_cells, what="again")
    _same(prots, pairs[::-1], want[::-1], max_cells=max_cells, what="reversed")


def test_a_second_pair_in_the_long_launch(long_call):
    """Gap 1, the long launch: kAlignLongGrid + 76 long pairs, the first kAlignLongGrid of the order all of 129 rows, so the
    pairs of 65 rows behind them go to a workgroup whose slab holds the row 127 of a pair before, under b of another length.
    300 short pairs lie in between in the caller's list: both launches in one call, the long one's order at d_order + n_short
    and its counter the second one.  Twice, and with the list reversed."""
    prots, pairs, want = long_call
    h = E.hand_out(prots, pairs)
    assert len(h["long"]) > h["long_grid"] == E.LONG_GRID and len(h["short"]) == E.LONG_SHORT_PAIRS
    _same(prots, pairs, want)
    _same(prots, pairs, want, what="again")
    _same(prots, pairs[::-1], want[::-1], what="reversed")
    _same(prots, pairs[h["long"]], want[h["long"]], what="the long pairs alone, in hand-out order")


# ---- B. the LDS / slab border -------------------------------------------------------------------------------------------------

def test_b_of_1023_1024_and_1025_residues():
    """Gap 2 (and 6): b on both sides of kAlignLdsCols against a of 1, 64, 65, 129, 193 rows with a 12-row gap, each ending
    in b's last column.  All 15 in one call (both launches), each alone, and through kg_proteins_align_device."""
    prots, pairs, answer = E.border_pairs()
    want = E.model(prots, pairs)
    got = _same(prots, pairs, want)
    for k, ans in enumerate(answer):
        if ans is not None:
            assert _triple(got[k]) == ans, pairs[k]
        _same(prots, [pairs[k]], want[k:k + 1], what="pair %d alone" % k)
    _same(prots, pairs, want, device=True, what="device bytes")
    _same(prots, [(b, a) for a, b in pairs], what="b as the rows")             # 1023 .. 1025 rows: 16 and 17 stripes


@pytest.mark.parametrize("row,m", E.LAST_COLUMN)
def test_the_best_cell_in_the_last_column(row, m):
    """Gap 2: j = m - 1 for m = kAlignLdsCols (the last LDS carry column) and m = kAlignLdsCols + 1 (the slab's)."""
    a, b, want = E.last_column_case(row, m)
    got = _same([a, b], [(0, 1)])
    assert _triple(got[0]) == want
    _same([a, b], [(0, 1)], device=True)


def test_gaps_in_and_over_the_last_lds_column():
    """Gap 2: a vertical gap across the stripe border in column 1023 and in column 1024 (its F goes through the carry of
    exactly that column), and a horizontal gap over columns 1018 .. 1029."""
    cases = [E.vertical_gap_case(col) for col in E.GAP_COLUMNS] + [E.horizontal_gap_case()]
    prots = [p for a, b, _ in cases for p in (a, b)]
    got = _same(prots, [(0, 1), (2, 3), (4, 5)])
    assert [_triple(r) for r in got] == [want for _, _, want in cases]
    _same(prots, [(0, 1), (2, 3), (4, 5)], device=True)


# ---- C. the slab-bytes cap and the stride -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cap_call():
    prots, pairs = E.slab_cap_case()
    return prots, pairs, E.model(prots, pairs)


def test_the_slab_stride_under_the_bytes_cap(cap_call):
    """Gap 3: one b of 40000 residues makes slab_cols 40000 and the long launch kAlignSlabBytes / (8 * 40000) = 838
    workgroups for 901 pairs, each carrying at slab + blockIdx.x * slab_cols; 900 of the pairs have two or three stripes."""
    prots, pairs, want = cap_call
    h = E.hand_out(prots, pairs)
    assert h["long_grid"] == 838 < len(h["long"]) == 901 and h["slab_cols"] == 40000
    _same(prots, pairs, want)
    _same(prots, pairs[::-1], want[::-1], what="reversed")
    assert (want["score"] > 0).all() and len(set(want.tolist())) == 17


# ---- D. ties --------------------------------------------------------------------------------------------------------------------

def test_ties_of_the_best_cell():
    """Gap 4: cells of equal score in one lane's two stripes, in a later stripe's smaller lane, on a stripe border, in the
    first and last rows; in one row in one and in two chunks of columns; three and four cells.  The answer is the smallest
    row, then the smallest column, in the short instantiation (b of 90) and in the long one (b of 1025)."""
    cases = E.tie_cases()
    prots = [p for _, a, b, _ in cases for p in (a, b)]
    pairs = [(2 * k, 2 * k + 1) for k in range(len(cases))]
    got = _same(prots, pairs)
    for k, (name, _, _, want) in enumerate(cases):
        assert _triple(got[k]) == want, name
    _same(prots, [(b, a) for a, b in pairs], what="the columns as rows")


# ---- E. bytes and tables ----------------------------------------------------------------------------------------------------------

def test_every_byte_value():
    """Gap 5 (and 6): all 256 byte values through aa_code_of_rt, in both places and through both entry points."""
    prots, pairs = E.byte_proteins()
    got = _same(prots, pairs)
    assert got["self_a"][:6].tolist() == [116] * 6 and _triple(got[0]) == (111, ord("Y"), ord("Y"))
    _same(prots, pairs, device=True)


@pytest.mark.parametrize("name", list(E.tables()))
def test_score_tables_at_their_bounds(name):
    """Gap 5 (and 6): entries of 16 and -16, a positive "everything else" row, free gap opens."""
    prots, pairs = E.byte_proteins()
    mat, go, ge = E.tables()[name]
    got = _same(prots, pairs, matrix=mat, gap_open=go, gap_extend=ge)
    if name != "random, everything else positive":
        assert _triple(got[0]) == (4096, 255, 255) and got["self_a"][0] == 320
    _same(prots, pairs, device=True, matrix=mat, gap_open=go, gap_extend=ge)
    rel, rel_pairs, _ = E.border_pairs()
    _same(rel, rel_pairs[2::5], matrix=mat, gap_open=go, gap_extend=ge)        # 65 rows against 1023, 1024, 1025 columns


# ---- F. the cut kernel --------------------------------------------------------------------------------------------------------------

def _cluster_same(prots, min_shared=5, min_cover_pct=20, device=False, **align):
    """Families, edge records, counts and align counts == cluster_aligned_model's.  -> (records, statistics)"""
    from kmergutsjava_amd import hotpath
    seq, off = M.pack(prots)
    want, counts, edges, ast = E.cluster_model(prots, min_shared, min_cover_pct, **align)
    if device:
        d = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
        got, st = hotpath.cluster_proteins(None, off, min_shared=min_shared, min_cover_pct=min_cover_pct, align=align, device_ptr=d.data_ptr())
    else:
        got, st = hotpath.cluster_proteins(seq, off, min_shared=min_shared, min_cover_pct=min_cover_pct, align=align)
    assert {k: st[k] for k in M.COUNTS} == counts, align
    assert {k: st["align"][k] for k in ALIGN_COUNTS} == ast, align
    _equal(st["edge_records"], edges, align)
    _equal(got, want, align)
    return got, st


@pytest.mark.parametrize("L", E.CUT_L)
def test_the_cut_at_wave_and_workgroup_sizes(L):
    """Gap 7: exactly L links for align_cut_kernel, L around the 64 lanes of a ballot and the 256 of a workgroup (a partial
    last wave included), kept, cut and skipped links mixed without a period: words[kClusterEdges], both tallies, ridx, the
    edge records and best after the cut, under both ref modes and min_ratio_pct 0, 50 and 100."""
    prots, kinds = E.cut_links(L)
    for ref in ("longer", "member"):
        for pct in (0, 50, 100):
            got, st = _cluster_same(prots, ref=ref, min_ratio_pct=pct, max_cells=E.CUT_MAX_CELLS)
            assert st["links"] == L == len(st["edge_records"])
            if pct == 50:
                assert st["edge_records"]["status"].tolist() == [E.CUT_STATUS[ref][k] for k in kinds]
    _cluster_same(prots, device=True, max_cells=E.CUT_MAX_CELLS)


def test_the_ratio_test_at_exact_equality():
    """Gap 7: 100 * score == min_ratio_pct * ref is kept and one per cent more is cut, with ref the centre's self-score
    (ref = longer) and the member's (ref = member); a score of 0 is cut at min_ratio_pct = 0."""
    for name, (prots, ref, numbers) in E.half_cases().items():
        r = numbers[1] if ref == "member" else max(numbers[1:])
        for pct, status in ((50, N.EDGE_KEPT), (51, N.EDGE_CUT)):
            got, st = _cluster_same(prots, ref=ref, min_ratio_pct=pct, matrix=E.HALF_MATRIX, **E.HALF_GAPS)
            assert st["edge_records"].tolist() == [(0, 1, 13, 40, r, 19, 19, status)], (name, pct)
            assert st["families"] == 1 + (status == N.EDGE_CUT) and st["align"]["cut"] == (status == N.EDGE_CUT)
    prots = E.half_cases()["member"][0]
    for pct, status in ((40, N.EDGE_KEPT), (41, N.EDGE_CUT)):
        got, st = _cluster_same(prots, min_ratio_pct=pct, matrix=E.HALF_MATRIX, **E.HALF_GAPS)
        assert st["edge_records"]["status"].tolist() == [status] and st["edge_records"]["ref"].tolist() == [100]
    for pct in (0, 50):
        got, st = _cluster_same(E.identical_pair(), min_ratio_pct=pct, matrix=E.MINUS_ONE)
        assert st["edge_records"].tolist() == [(1, 0, 32, 0, -40, -1, -1, N.EDGE_CUT)] and st["families"] == 2 and st["edges"] == 0
    got, st = _cluster_same(E.identical_pair(), min_ratio_pct=100)
    assert st["edge_records"]["status"].tolist() == [N.EDGE_KEPT] and st["families"] == 1


@pytest.mark.parametrize("member_first", [True, False])
def test_best_after_the_cut_between_two_equal_centres(member_first):
    """Gap 7: the centre with the most shared 8-mers is cut and two kept centres share equally many: best is the smaller."""
    prots, m, centres = E.best_after_cut_case(member_first)
    got, st = _cluster_same(prots, **E.BEST_PARAMS)
    assert st["edge_records"]["status"].tolist() == [N.EDGE_KEPT, N.EDGE_CUT, N.EDGE_KEPT]
    assert got["best"][m] == centres[0] and got["shared"][m] == 18 and st["edges"] == 2
