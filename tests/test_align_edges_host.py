"""The inputs of tests/test_gpu_align_edges.py on the CPU: the constants tests/align_edge_cases.py is built around, parsed from
kg_align.hpp and kg_host_align.hpp; the hand-out order and the grids each call gives, by the restated arithmetic of align_run;
and tests/align_model.py against the answers the cases know by construction."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import align_edge_cases as E  # noqa: E402
import align_model as A  # noqa: E402
import cluster_model as M  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import align_scores as AS  # noqa: E402

ROOT = os.path.dirname(HERE)


def _s(x: str, y: str) -> int:
    return int(A.S62[AS.ALPHA.index(x.encode()), AS.ALPHA.index(y.encode())])


def _triple(rec):
    return int(rec["score"]), int(rec["end_a"]), int(rec["end_b"])


# ---- the constants ------------------------------------------------------------------------------------------------------------

def test_the_constants_the_edge_cases_are_built_around():
    csrc = os.path.join(ROOT, "kmergutsjava_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("kg_device.hpp", "kg_align.hpp", "kg_host_align.hpp", "kg_host_cluster.hpp")}

    def const(name, var):
        return int(re.search(r"constexpr int %s = (\d+);" % var, text[name]).group(1))

    assert const("kg_align.hpp", "kAlignLdsCols") == E.LDS_COLS == N.ALIGN_LDS_COLS == 1024
    assert const("kg_device.hpp", "kWave") == E.WAVE == 64
    a, b = re.search(r"constexpr uint32_t kAlignGrid = (\d+) \* (\d+);", text["kg_host_align.hpp"]).groups()
    assert int(a) * int(b) == E.GRID == 256 * 18
    assert int(re.search(r"constexpr uint32_t kAlignLongGrid = (\d+);", text["kg_host_align.hpp"]).group(1)) == E.LONG_GRID == 1024
    a, b = re.search(r"constexpr uint64_t kAlignSlabBytes = (\d+)ull << (\d+);", text["kg_host_align.hpp"]).groups()
    assert int(a) << int(b) == E.SLAB_BYTES == 256 * 1024 * 1024
    # the arithmetic E.hand_out restates: the two grids, the slab's columns, the stride, one wave per workgroup
    host = text["kg_host_align.hpp"]
    assert "dim3((uint32_t)std::min<uint64_t>(n_short, kAlignGrid)), dim3(kg::kWave)" in host
    assert "std::min<uint64_t>({n_long, (uint64_t)kAlignLongGrid, std::max<uint64_t>(1, kAlignSlabBytes / (slab_cols * 8))})" in host
    assert "slab_cols = std::max<uint64_t>(slab_cols, ((uint64_t)m + 63) / 64 * 64)" in host
    assert "const bool lng = !skip && m > kg::kAlignLdsCols;" in host and "return cells[x] > cells[y]" in host and "std::stable_sort" in host
    assert "dim3(long_grid), dim3(kg::kWave)" in host and "d_order + n_short" in host and "d_counter + 1" in host
    assert "slab + (uint64_t)blockIdx.x * slab_cols" in text["kg_align.hpp"]
    assert "__launch_bounds__(%d) void align_cut_kernel" % E.CUT_THREADS in text["kg_align.hpp"]
    assert "kg::align_cut_kernel, dim3(grid_of(NP)), dim3(%d)" % E.CUT_THREADS in text["kg_host_cluster.hpp"]
    # what the cases derive from them
    assert E.SHORT_PAIRS == E.GRID + 400 and E.LONG_PAIRS == E.LONG_GRID + 76 and sum(E.LONG_COUNT.values()) == E.LONG_PAIRS
    assert E.BORDER_M == (E.LDS_COLS - 1, E.LDS_COLS, E.LDS_COLS + 1) and E.GAP_COLUMNS == (E.LDS_COLS - 1, E.LDS_COLS)
    assert {m for _, m in E.LAST_COLUMN} == {E.LDS_COLS, E.LDS_COLS + 1} and {r for r, _ in E.LAST_COLUMN} == {E.WAVE - 1, E.WAVE, 2 * E.WAVE + 1}
    assert set(E.CUT_L) == {1, E.WAVE - 1, E.WAVE, E.WAVE + 1, E.CUT_THREADS - 1, E.CUT_THREADS, E.CUT_THREADS + 1, 2 * E.CUT_THREADS + 1}


# ---- A. a workgroup's second pair ---------------------------------------------------------------------------------------------

def test_the_short_call_has_more_pairs_than_workgroups():
    prots, pairs, max_cells = E.second_pair_short()
    assert len(prots) == 20 and {len(p) for p in prots} == set(E.SHORT_LENGTHS)
    assert {tuple(p) for p in pairs.tolist()} == {(i, 10 + j) for i in range(10) for j in range(10)}
    h = E.hand_out(prots, pairs, max_cells)
    n_short = len(h["short"])
    assert n_short == len(pairs) == E.SHORT_PAIRS > E.GRID == h["short_grid"] and len(h["long"]) == 0
    assert n_short - h["short_grid"] == 400                     # by pigeonhole, this many pairs are some workgroup's second or later
    # the skipped pairs are handed out last, all of them behind the first GRID pairs, and leave room for second pairs that align
    assert 150 < h["skipped"] < 250
    order = h["short"]
    cells = np.where(h["n"] * h["m"] > max_cells, 0, h["n"] * h["m"])[order]
    assert (cells[:-1] >= cells[1:]).all() and (cells[-h["skipped"]:] == 0).all() and cells[-h["skipped"] - 1] == 1
    assert (h["n"][order[:100]] > E.WAVE).all() and (h["n"][order[-h["skipped"]:]] > E.WAVE).all()     # two stripes at both ends
    later = order[E.GRID:len(order) - h["skipped"]]             # aligned, and some workgroup's second pair or later
    assert ((h["n"][later] == E.WAVE + 1) & (h["m"][later] == E.WAVE - 1)).sum() > 100 and (h["n"][later] <= 2).sum() > 10
    want = E.model(prots, pairs, max_cells=max_cells)
    skipped = want["status"] == N.ALIGN_SKIPPED
    assert skipped.sum() == h["skipped"] and (want["score"][skipped] == -1).all()
    assert (want["self_a"] == [A.self_score(prots[a]) for a in pairs[:, 0]]).all() and (want["self_a"][skipped] > 400).all()
    rel = (pairs[:, 0] < 5) & (pairs[:, 1] < 15) & ~skipped & (h["n"] >= 63) & (h["m"] >= 63)
    assert rel.sum() > 300 and want["score"][rel].min() > 150 > want["score"][(pairs[:, 0] >= 5) & ~skipped].max()


def test_the_long_call_hands_pairs_of_65_rows_to_slabs_that_held_129():
    prots, pairs = E.second_pair_long()
    assert [len(p) for p in prots[20:24]] == list(E.LONG_A) and [len(p) for p in prots[24:]] == list(E.LONG_B)
    h = E.hand_out(prots, pairs)
    order = h["long"]
    assert len(order) == E.LONG_PAIRS and h["long_grid"] == E.LONG_GRID and len(h["short"]) == E.LONG_SHORT_PAIRS and h["skipped"] == 0
    assert h["slab_cols"] == 1152 and h["slab_cols"] * 8 * E.LONG_GRID < E.SLAB_BYTES         # the cap does not bind here
    rows, cols = h["n"][order], h["m"][order]
    assert (rows[:E.LONG_GRID] == 129).all()                    # every workgroup's first pair has three stripes ...
    later = rows[E.LONG_GRID:].tolist()                         # ... and the 68 pairs of 65 rows come behind them all
    assert sorted(later[:72]) == [64] * 4 + [65] * 68 and later[72:] == [1] * 4
    assert set(cols[E.LONG_GRID:][rows[E.LONG_GRID:] == 65].tolist()) == set(E.LONG_B) == set(cols[:E.LONG_GRID].tolist())
    # both launches in one call, the two kinds of pair mixed in the caller's list
    is_long = np.zeros(len(pairs), dtype=bool)
    is_long[order] = True
    assert 200 < np.count_nonzero(is_long[1:] != is_long[:-1])
    want = E.model(prots, pairs)
    long_129 = want[order[:E.LONG_GRID]]
    assert (want["status"] == 0).all() and long_129["score"].min() > 150          # relatives: the carries hold real scores
    assert long_129["end_b"].min() >= 1000 and (long_129["end_a"] >= 2 * E.WAVE - 8).all()      # ... up to the third stripe


# ---- B. the LDS / slab border ---------------------------------------------------------------------------------------------------

def test_the_border_pairs_end_in_the_last_column():
    prots, pairs, answer = E.border_pairs()
    assert len(pairs) == 15 and sorted({len(prots[b]) for _, b in pairs}) == [1023, 1024, 1025]
    assert [len(prots[a]) for a, _ in pairs] == list(E.BORDER_N) * 3
    want = E.model(prots, pairs)
    for k, ans in enumerate(answer):
        if ans is not None:
            assert _triple(want[k]) == ans, (k, pairs[k])
        else:                                                   # one residue: its best match in b, the first of them
            row = A.S62[A.codes(prots[pairs[k][0]])[0]][A.codes(prots[pairs[k][1]])]
            assert _triple(want[k]) == (int(row.max()), 0, int(np.argmax(row)))
    assert (want["end_b"][[4, 9, 14]] == [1022, 1023, 1024]).all() and (want["end_a"][[3, 8, 13]] == 128).all()


@pytest.mark.parametrize("row,m", E.LAST_COLUMN)
def test_six_w_in_the_last_column(row, m):
    a, b, want = E.last_column_case(row, m)
    assert E.sw_cached(a, b) == want == (66, row, m - 1)


def test_gaps_at_the_last_lds_column():
    for col in E.GAP_COLUMNS:
        a, b, want = E.vertical_gap_case(col)
        assert len(b) == col + 141 > E.LDS_COLS and E.sw_cached(a, b) == want
    a, b, want = E.horizontal_gap_case()
    assert E.sw_cached(a, b) == want and want[2] == 1149


# ---- C. the slab-bytes cap ------------------------------------------------------------------------------------------------------

def test_the_cap_on_the_slabs_bytes_binds():
    prots, pairs = E.slab_cap_case()
    h = E.hand_out(prots, pairs)
    assert h["slab_cols"] == E.CAP_COLS == 40000 and h["slab_cols"] % E.WAVE == 0
    assert h["long_grid"] == E.SLAB_BYTES // (8 * E.CAP_COLS) == 838 < E.LONG_GRID
    assert len(h["long"]) == E.CAP_LONG_PAIRS + 1 == 901 > h["long_grid"] and len(h["short"]) == 0
    assert h["long_grid"] * h["slab_cols"] * 8 <= E.SLAB_BYTES < (h["long_grid"] + 1) * h["slab_cols"] * 8
    assert {(int(n), int(m)) for n, m in zip(h["n"], h["m"])} == {(1, 40000)} | {(n, m) for n in (65, 129) for m in (1025, 1100)}
    assert len({tuple(p) for p in pairs.tolist()}) == 17 and h["n"][h["long"][-1]] == 1        # 16 alignments and the one long one
    assert int((h["n"] * h["m"]).sum()) < 100_000_000


# ---- D. ties ----------------------------------------------------------------------------------------------------------------------

def test_the_planted_letters():
    assert _s("P", "P") == _s("Y", "Y") == 7 and _s("P", "Y") == -3
    for x in (E.FILL_A + E.FILL_B).decode():
        assert _s("P", x) < 0 and _s("Y", x) < 0
    for x in E.FILL_A.decode():
        for y in E.FILL_B.decode():
            assert _s(x, y) < 0


def test_ties_give_the_smallest_row_then_the_smallest_column():
    cases = E.tie_cases()
    assert len(cases) == 20 + 15 + 2 * 6 and len({name for name, _, _, _ in cases}) == len(cases)
    for name, a, b, want in cases:
        assert len(a) == E.TIE_N and len(b) in (E.TIE_M, E.LDS_COLS + 1) and want[0] == 7
        assert E.sw_cached(a, b) == want, name
        if len(b) == E.TIE_M:
            assert A.sw_loops(a, b) == want, name
    grid = {name: want for name, _, _, want in cases}
    for i1, i2 in E.TIE_ROWS:
        for j1, j2 in E.TIE_COLS:
            assert grid["rows %d %d cols %d %d of 90" % (i1, i2, j1, j2)] == (7, i1, j1) and i1 < i2


# ---- E. bytes and tables ----------------------------------------------------------------------------------------------------------

def test_only_the_twenty_upper_case_letters_have_a_code():
    every = bytes(range(256))
    c = A.codes(every)
    assert sorted(np.flatnonzero(c < 20).tolist()) == sorted(AS.ALPHA) and (c[[0, ord("a"), ord("*"), ord("X"), 128, 255]] == 20).all()
    prots, pairs = E.byte_proteins()
    assert prots[0] == every and prots[1] == every[::-1] and len(pairs) == 9
    want = E.model(prots, pairs)
    assert want["self_a"][:6].tolist() == [116] * 6 and want["self_b"][0] == 116
    # ascending against itself: the 25 bytes A .. Y with B, J, O, U and X at -1 each
    assert _triple(want[0]) == (116 - 5, ord("Y"), ord("Y")) and _triple(want[4]) == (111, 255 - ord("A"), 255 - ord("A"))
    assert want["score"][1] == want["score"][3] == 11              # against the reverse: one W on one W at the best


def test_the_tables_at_their_bounds():
    prots, pairs = E.byte_proteins()
    t = E.tables()
    assert len(t) == 4
    for name, (mat, go, ge) in t.items():
        assert mat.shape == (21, 21) and (mat == mat.T).all() and mat.min() >= -16 and mat.max() <= 16, name
    flat, rand = t["16 everywhere"][0], t["random, everything else positive"][0]
    assert (rand[20] > 0).all() and rand.min() == -16 and rand.max() == 16
    want = E.model(prots, pairs, flat)
    assert _triple(want[0]) == (4096, 255, 255) and want["self_a"][0] == 320 and _triple(want[1]) == (4096, 255, 255)
    assert _triple(want[2]) == (16 * 256, 255, 255) and _triple(want[8]) == (16 * 300, 299, 299)
    for name in ("16 and -16", "16 and -16, gaps 0 and 1"):
        mat, go, ge = t[name]
        want = E.model(prots, pairs, mat, go, ge)
        assert _triple(want[0]) == (4096, 255, 255) and want["self_a"][0] == 320 and _triple(want[8]) == (4800, 299, 299)
    # with free gap opens the reverse pair chains matches that a gap of 12 keeps apart
    a = E.model(prots, pairs, *t["16 and -16"])
    b = E.model(prots, pairs, *t["16 and -16, gaps 0 and 1"])
    assert (b["score"] >= a["score"]).all() and (b["score"] > a["score"]).any()


# ---- F. the cut kernel --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", E.CUT_L)
def test_the_cut_generator(L):
    prots, kinds = E.cut_links(L)
    assert len(kinds) == L and len(prots) == L + min(L, 8)
    for ref in ("longer", "member"):
        rec, counts, edges, st = E.cluster_model(prots, ref=ref, max_cells=E.CUT_MAX_CELLS)
        assert counts["links"] == L == len(edges) and len(set(edges["member"].tolist())) == L
        assert edges["status"].tolist() == [E.CUT_STATUS[ref][k] for k in kinds], ref
        assert counts["edges"] == L - st["cut"] and st["aligned"] + st["skipped"] == L
    rec, counts, edges, st = E.cluster_model(prots, max_cells=E.CUT_MAX_CELLS)
    status = edges["status"]
    if L >= 63:
        assert min((status == v).sum() for v in (N.EDGE_KEPT, N.EDGE_CUT, N.EDGE_SKIPPED)) >= L // 5
    if L > 2 * E.WAVE:
        # no period of 64: the ballots of consecutive waves count different numbers of every status
        assert (status[:-E.WAVE] != status[E.WAVE:]).sum() > L // 4
        for v in (N.EDGE_KEPT, N.EDGE_CUT, N.EDGE_SKIPPED):
            per_wave = [(status[w:w + E.WAVE] == v).sum() for w in range(0, L - E.WAVE + 1, E.WAVE)]
            assert len(set(per_wave)) > 1
    # any positive score is kept at 0; at 100 under ref = member, a member that is a piece of its centre scores exactly its own
    _, counts, edges, st = E.cluster_model(prots, min_ratio_pct=0, max_cells=E.CUT_MAX_CELLS)
    assert st["cut"] == 0 and counts["edges"] == L
    _, counts, edges, st = E.cluster_model(prots, min_ratio_pct=100, ref="member", max_cells=E.CUT_MAX_CELLS)
    assert edges["status"].tolist() == [E.CUT_STATUS["member"][k] for k in kinds]
    piece = np.array([k in ("kept", "member") for k in kinds])
    assert (edges["score"][piece] == edges["ref"][piece]).all()
    _, counts, edges, st = E.cluster_model(prots, min_ratio_pct=100, max_cells=E.CUT_MAX_CELLS)
    assert st["cut"] == st["aligned"]


def test_exactly_half_of_the_reference():
    for name, (prots, ref, numbers) in E.half_cases().items():
        got = E.model(prots, [(0, 1)], E.HALF_MATRIX, **E.HALF_GAPS)[0]
        assert (int(got["score"]), int(got["self_a"]), int(got["self_b"])) == numbers, name
        assert len(prots[0]) < len(prots[1])
        r = numbers[1] if ref == "member" else max(numbers[1:])
        assert 100 * numbers[0] == 50 * r and A.kept(numbers[0], r, 50) and not A.kept(numbers[0], r, 51)
        for pct, status in ((50, N.EDGE_KEPT), (51, N.EDGE_CUT)):
            _, counts, edges, st = E.cluster_model(prots, ref=ref, min_ratio_pct=pct, matrix=E.HALF_MATRIX, **E.HALF_GAPS)
            assert edges.tolist() == [(0, 1, 13, 40, r, 19, 19, status)] and counts["families"] == 1 + (status == N.EDGE_CUT)
    # the member case under ref = longer: the bound is at 40, where 100 * 40 == 40 * 100
    prots = E.half_cases()["member"][0]
    for pct, status in ((40, N.EDGE_KEPT), (41, N.EDGE_CUT), (50, N.EDGE_CUT)):
        assert E.cluster_model(prots, min_ratio_pct=pct, matrix=E.HALF_MATRIX, **E.HALF_GAPS)[2]["status"].tolist() == [status]


def test_a_score_of_zero_is_cut_at_any_percentage():
    prots = E.identical_pair()
    for pct in (0, 50):
        rec, counts, edges, st = E.cluster_model(prots, min_ratio_pct=pct, matrix=E.MINUS_ONE)
        assert edges.tolist() == [(1, 0, 32, 0, -40, -1, -1, N.EDGE_CUT)] and counts["families"] == 2 and st["cut"] == 1
    assert E.cluster_model(prots, min_ratio_pct=100)[2]["status"].tolist() == [N.EDGE_KEPT]       # BLOSUM62: score == ref


@pytest.mark.parametrize("member_first", [True, False])
def test_best_is_the_smaller_of_two_equal_kept_centres(member_first):
    prots, m, centres = E.best_after_cut_case(member_first)
    rec, counts, edges, st = E.cluster_model(prots, min_cover_pct=E.BEST_PARAMS["min_cover_pct"], min_ratio_pct=E.BEST_PARAMS["min_ratio_pct"])
    assert edges["member"].tolist() == [m] * 3 and edges["centre"].tolist() == centres
    assert edges["shared"].tolist() == [18, 33, 18] and edges["status"].tolist() == [N.EDGE_KEPT, N.EDGE_CUT, N.EDGE_KEPT]
    assert rec["best"][m] == centres[0] and rec["shared"][m] == 18 and counts["edges"] == 2
    assert M.partition(rec) == {frozenset([m, centres[0], centres[2]]), frozenset([centres[1]])}
    plain, _ = M.cluster_numpy(*M.pack(prots), 5, E.BEST_PARAMS["min_cover_pct"])
    assert plain["best"][m] == centres[1] and plain["shared"][m] == 33         # without the cut, best is the cut centre
