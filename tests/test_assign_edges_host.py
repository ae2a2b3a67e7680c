"""The inputs of tests/test_gpu_assign_edges.py on the CPU: both forms of tests/assign_model.py against each other and against
the answers of tests/assign_edge_cases.py, byte for byte; the constants and the grid expression the cases are built around; and
the conditions on the inputs themselves (the lane of every planted rank, the key widths, what the scan behind (j) emits)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import assign_edge_cases as E  # noqa: E402
import assign_model as A  # noqa: E402
import signature_model as M  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402


def _both(case, what=""):
    """assign == brute_force == the case's answer.  -> the answer"""
    calls, cs, otu, (ms, share), answer = case
    assert answer.dtype == N.ASSIGNMENT_DTYPE and len(answer) == len(cs) - 1, what
    assert A.assign(calls, cs, otu, ms, share).tobytes() == answer.tobytes(), what
    assert A.brute_force(calls, cs, otu, ms, share).tobytes() == answer.tobytes(), what
    return answer


def test_the_constants_the_edge_cases_are_built_around():
    assert (E.SHORT, E.WALK, E.WAVE, E.SCAN, E.TILE) == (16, 16, 64, 2048, 4096)
    # min((n_long + 3) / 4, 256 * 64) workgroups of four waves: a change to the expression fails the import of the cases
    assert E.GRID == 256 * 64 and E.WAVES_PER_WG == 4
    assert "dim3(wgrid), dim3(256)" in E.HOST_TEXT and E.HOST_TEXT.count("dim3(wgrid)") == 2 and E.WAVES_PER_WG * E.WAVE == 256
    assert "const bool is_long = n > kAssignShort;" in E.ASSIGN_TEXT
    assert "sp.sort(t, sc, n_items, 32 + bits_for(n_long))" in E.HOST_TEXT
    assert np.float32(E.BIG) + np.float32(1) == np.float32(E.BIG) and np.float32(E.BIG) + np.float32(2) > np.float32(E.BIG)


# ---- a ----------------------------------------------------------------------------------------------------------------------------

def test_split_lists_on_both_paths():
    lists, _ = E.split_lists()
    lens = [len(x) for x in lists]
    assert len(lists) == 200 and min(lens) == 1 and max(lens) == E.SHORT and {1, 15, 16} <= set(lens)
    case, source = E.split_case()
    calls, cs, otu, params, answer = case
    _both(case)
    n = np.diff(cs)
    for k in (0, 57, 199):                                      # the variants of one list: itself, then behind and in front per total
        mine = np.flatnonzero(source == k)
        totals = [t for t in E.SPLIT_TOTALS if t > lens[k]]
        assert n[mine].tolist() == [lens[k]] + [t for t in totals for _ in (0, 1)]
        for p in mine[1:]:
            body = calls[cs[p]:cs[p + 1]]
            pad = body[body["count"] == 0]
            assert len(pad) == n[p] - lens[k] and (pad["fI"] == lists[k]["fI"][0]).all()
            assert not np.signbit(pad["weightedHits"]).any() and (pad["weightedHits"] == 0).all()
    assert ((n <= E.SHORT).sum(), (n > E.SHORT).sum()) == (200 + 2 * sum(x < 16 for x in lens), 8 * 200)
    fields = [f for f in N.ASSIGNMENT_DTYPE.names if f != "n_calls"]
    assert (answer[fields] == answer[np.searchsorted(source, source)][fields]).all() and (answer["n_calls"] == n).all()


# ---- b ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", E.GRID_MODES)
def test_rank_grid(mode):
    case = E.grid_case(mode)
    calls, cs, _, _, answer = case
    _both(case)
    plan = E.grid_plan(mode)
    assert len(plan) == len(answer) == (2 if mode == 4 else 90 + 30)
    for p, (g, i, j) in enumerate(plan):
        c = calls[cs[p]:cs[p + 1]]
        assert len(c) == g["n"] and (len(c) > E.SHORT) == (g is E.GRID_LONG)
        f = np.sort(c["fI"])                                    # int32: the signed order, which is the key's (fI ^ 2^31, unsigned)
        assert (np.diff(f.astype(np.int64)) > 0).all() and {E.I32_MIN, -1, 0, E.I32_MAX} <= set(f.tolist())
        assert (np.argsort(c["fI"].astype(np.uint32) ^ np.uint32(2 ** 31), kind="stable") == np.argsort(c["fI"], kind="stable")).all()
        assert (c["fI"] != f).any()                             # emitted in another order than the sorted one
        rank_of = {int(v): k for k, v in enumerate(f)}
        planted = {rank_of[int(x["fI"])]: (int(x["count"]), float(x["weightedHits"])) for x in c if x["count"] > 1}
        if mode == 1:
            assert planted == {i: (3, 1.0), j: (2, 1.0)} and rank_of[int(answer[p]["fI"])] == i
        elif mode == 2:
            assert planted == {i: (2, 2.0), j: (2, 1.5)} and rank_of[int(answer[p]["fI"])] == i
        elif mode == 3:
            assert planted == {i: (2, 1.0), j: (2, 1.0)} and rank_of[int(answer[p]["fI"])] == min(i, j)
        elif mode == 4:
            assert planted == {} and rank_of[int(answer[p]["fI"])] == 0 and rank_of[int(answer[p]["second_fi"])] == 1
        else:
            assert planted == {i: (2, 1.0), j: (2, 1.0), g["above"]: (3, 1.0)} and rank_of[int(answer[p]["second_fi"])] == min(i, j)
    if mode != 4:
        # run k of a long protein is item base + k, read by lane k % 64 in round k / 64: the pairs the wave merge must get right
        lanes = {(i % E.WAVE, i // E.WAVE, j % E.WAVE, j // E.WAVE) for g, i, j in plan if g is E.GRID_LONG}
        assert {(0, 0, 0, 1), (0, 1, 0, 0), (0, 0, 0, 2), (63, 1, 63, 0), (1, 2, 1, 0)} <= lanes       # one lane, different rounds
        assert {(0, 0, 63, 0), (63, 0, 0, 0), (0, 0, 63, 1), (63, 1, 0, 2)} <= lanes                    # lanes 0 and 63
        assert {(31, 0, 32, 0), (32, 0, 31, 0), (0, 0, 1, 0), (1, 0, 0, 0)} <= lanes                    # neighbours across a butterfly step
        assert any(j < i for g, i, j in plan if g is E.GRID_LONG) and any(i < j for g, i, j in plan)    # the runner-up in front of the best


# ---- c ----------------------------------------------------------------------------------------------------------------------------

def _run_items(calls, cs, p):
    """Where the run of RUN_F stands among protein p's sorted items: (first item, length, items of the protein)"""
    f = np.sort(calls["fI"][cs[p]:cs[p + 1]], kind="stable")
    at = np.flatnonzero(f == E.RUN_F)
    assert (np.diff(at) == 1).all()
    return int(at[0]), len(at), len(f)


def test_walk_weights():
    for L in E.WALK_L:
        w, total = E.walk_weights(L, "big first")
        assert w[0] == E.BIG and w[1:] == [1.0] * (L - 1) and total == np.float32(2 ** 24)
        w, total = E.walk_weights(L, "big last")
        assert w[-1] == E.BIG and w[:-1] == [1.0] * (L - 1)
        assert float(total) == 2 ** 24 + L - 1 + {0: 0, 2: 0, 1: -1, 3: 1}[(L - 1) % 4]           # an odd L - 1: the tie goes to the even mantissa
    assert sorted(E.behind(L) for L in E.WALK_L)[0] == 1 and max(E.behind(L) for L in E.WALK_L) == E.WALK - 1


def test_walk_inner_runs():
    case = E.walk_inner_case()
    calls, cs, _, _, answer = case
    _both(case)
    assert len(answer) == 2 * 2 * len(E.WALK_L) and (np.diff(cs) > E.SHORT).all()
    assert (answer["fI"] == E.RUN_F).all() and sorted(set(answer["score"].tolist())) == sorted(E.WALK_L)
    k = len(E.WALK_L)
    for q, L in enumerate(E.WALK_L):
        for order in (0, 1):
            p = order * k + q                                   # contiguous
            c = calls[cs[p]:cs[p + 1]]
            assert (c["fI"][:L] == E.RUN_F).all() and len(c) == L + (17 if L <= 16 else 0)
            p = 2 * k + order * k + q                           # on the even positions
            c = calls[cs[p]:cs[p + 1]]
            assert (c["fI"][0:2 * L:2] == E.RUN_F).all() and (c["fI"][1:2 * L - 1:2] != E.RUN_F).all() and (c["fI"] == E.RUN_F).sum() == L
            assert len(set(c["fI"][1:2 * L - 1:2].tolist())) == L - 1 and _run_items(calls, cs, p)[0] > 0
    assert answer["weighted"][:k].tolist() == [2.0 ** 24] * k and answer["weighted"][2 * k:3 * k].tolist() == [2.0 ** 24] * k


@pytest.mark.parametrize("arrangement", ["last", "behind"])
def test_walk_runs_at_the_end_of_the_sorted_array(arrangement):
    seen = set()
    for L in E.WALK_L:
        for order in E.WALK_ORDERS:
            case = E.walk_end_case(L, order, arrangement)
            calls, cs, _, _, answer = case
            _both(case, (L, order))
            long = np.flatnonzero(np.diff(cs) > E.SHORT)
            assert long.tolist() == [1, 3] and len(answer) == 6
            first, length, n = _run_items(calls, cs, 3)
            assert length == L == answer[3]["score"] and first > 0
            assert n - (first + L) == (0 if arrangement == "last" else E.behind(L))
            seen.add(n - (first + L))
    assert seen == {0} if arrangement == "last" else {1, E.WALK - 1} <= seen and max(seen) < E.WALK


def test_walk_neighbours():
    for lengths in E.NEIGHBOURS + (sum(E.NEIGHBOURS, ()),):
        case = E.neighbours_case(lengths)
        calls, cs, _, _, answer = case
        _both(case, lengths)
        assert (calls["fI"] == 7).all() and answer["score"][::2].tolist() == list(lengths) and (answer["n_functions"][::2] == 1).all()
        assert (answer["n_calls"][1::2] == 0).all() and answer["weighted"][::2].tolist() == [float(n) for n in lengths]


# ---- d ----------------------------------------------------------------------------------------------------------------------------

def test_sort_tiles():
    case = E.tiles_case()
    calls, cs, _, _, answer = case
    _both(case)
    n = 2 * E.TILE + 1000
    assert cs.tolist() == [0, n] and np.flatnonzero(calls["fI"] == 3).tolist() == [0, 4095, 4096, 8191, 8192, n - 1]
    assert calls["weightedHits"][0] == E.BIG and (calls["weightedHits"][1:] == 1).all() and (calls["count"] == 1).all()
    assert (calls["fI"] < 3).sum() > E.TILE - 100 and (calls["fI"] > 3).sum() > E.TILE and len(set(calls["fI"].tolist())) == n - 5
    assert answer[0].tolist() == (3, 0, 6, n, 2.0 ** 24, n, n - 5, -4000, 1, -1)


# ---- e ----------------------------------------------------------------------------------------------------------------------------

def test_key_widths_passes_and_the_grid():
    assert E.KEY_WIDTH_N_LONG == (1, 2, 3, 256, 257, 65536, 65537)
    assert {n: (E.key_bits(n), E.passes(n)) for n in E.KEY_WIDTH_N_LONG} == E.KEY_WIDTHS
    assert [E.KEY_WIDTHS[n] for n in E.KEY_WIDTH_N_LONG] == [(32, 4), (33, 5), (34, 5), (40, 5), (41, 6), (48, 6), (49, 7)]
    assert {E.passes(n) % 2 for n in E.KEY_WIDTH_N_LONG} == {0, 1}                          # the result in either buffer
    assert 65537 > 4 * 16384 and 65537 > E.WAVES_PER_WG * E.GRID >= 65536                   # only the last takes a second trip
    assert (65537 + 3) // 4 > E.GRID >= (65536 + 3) // 4


@pytest.mark.parametrize("n_long", E.KEY_WIDTH_N_LONG)
def test_key_width_inputs(n_long):
    case = E.key_width_case(n_long)
    calls, cs, otu, _, answer = case
    _both(case)
    n = np.diff(cs)
    long = np.flatnonzero(n > E.SHORT)
    assert len(long) == n_long and (n[long] == 17).all() and (n[n <= E.SHORT] <= 3).all()
    assert (np.diff(np.concatenate([[-1], long])) - 1 == np.arange(n_long) % 5).all()       # r % 5 others in front of long protein r
    assert n_long < 5 or (long != np.arange(n_long)).any()
    assert len(calls) == cs[-1] and (n_long < 65537 or 1_100_000 < len(calls) < 1_400_000)
    for r in sorted({0, min(1, n_long - 1), n_long - 1, n_long // 2}):
        p = long[r]
        assert calls[cs[p]:cs[p + 1]][["fI", "count", "weightedHits"]].tolist() == E.long17_rows(r)
        assert answer[p].tolist() == (r % 7, 1, 18, 34, 2.0 ** 24, 17, 2, 7 + r % 3, 16, p % 11 if p % 3 else -1)
    assert (otu["n"] == np.arange(len(n)) % 3).all()


# ---- f ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", E.CHUNK_VARIANTS)
def test_prefix_sum_chunk_inputs(variant):
    case = E.chunk_case(variant)
    calls, cs, _, _, answer = case
    _both(case)
    long = np.flatnonzero(np.diff(cs) > E.SHORT).tolist()
    if variant == "borders":
        assert len(answer) == 3 * 2048 + 3 and long == [0, 2047, 2048, 2049, 4095, 4096, 3 * 2048 + 2]
        assert set(np.diff(cs).tolist()) == {0, 1, 2, 3, 17}
    elif variant == "all long":
        assert len(answer) == 2049 and long == list(range(2049))
    else:
        assert len(answer) == 1 and long == [0]


# ---- g ----------------------------------------------------------------------------------------------------------------------------

def test_limit_cases():
    for share, assigned in ((100, [1, 0, 1, 0]), (50, [1, 1, 1, 1])):
        case = E.below_limit_case(share)
        calls, cs, _, _, answer = case
        _both(case, share)
        assert E.totals(calls, cs) == [2 ** 31 - 1] * 4 and (np.diff(cs) > E.SHORT).tolist() == [False, False, True, True]
        assert answer["total"].tolist() == [2 ** 31 - 1] * 4 and answer["score"].tolist() == [2 ** 31 - 1, 2 ** 30] * 2
        assert answer["assigned"].tolist() == assigned
    names = []
    for name, calls, cs, at in E.limit_error_cases():
        names.append(name)
        t, n = E.totals(calls, cs), np.diff(cs)
        bad = [p for p in range(len(t)) if t[p] >= 2 ** 31]
        assert bad[0] == at and all(t[p] == 2 ** 31 and calls["count"][cs[p]:cs[p + 1]].max() == 2 ** 30 for p in bad), name
        assert (calls["count"] >= 0).all()
        if " at " in name:
            assert bad == [3, 5] and (n[3] > E.SHORT) == name.startswith("long") and (n[5] > E.SHORT) != (n[3] > E.SHORT)
        else:
            assert len(bad) == 1 and (n[at] > E.SHORT) == (name == "long")
    assert names == ["short", "long", "long at 3, short at 5", "short at 3, long at 5"]


# ---- h ----------------------------------------------------------------------------------------------------------------------------

def test_threshold_cases():
    seen = []
    for name, case, ok in E.threshold_cases():
        calls, cs, _, params, answer = case
        _both(case, name)
        assert (np.diff(cs) > E.SHORT).tolist() == [False, True] and answer["assigned"].tolist() == [ok, ok], name
        assert answer[["fI", "score", "total", "weighted"]][0] == answer[["fI", "score", "total", "weighted"]][1]
        seen.append((int(answer["score"][0]), int(answer["total"][0]), params, ok))
    assert seen == [(1, 2, (0, 50), 1), (1, 2, (0, 51), 0), (33, 100, (0, 34), 0), (34, 100, (0, 34), 1), (7, 7, (7, 50), 1),
                    (7, 7, (8, 50), 0), (0, 0, (0, 50), 1), (0, 0, (1, 50), 0)]
    assert case[4]["fI"].tolist() == [4, 4] and case[4]["n_functions"].tolist() == [3, 20]


# ---- i ----------------------------------------------------------------------------------------------------------------------------

def test_shifted_cases():
    for name, case in E.shifted_cases():
        calls, cs, otu, (ms, share), answer = case
        _both(case, name)
        assert cs[0] == 5 and (calls["count"][:5] < 0).sum() == 1 and (calls["count"][5:] >= 0).all()
        assert A.assign(calls[5:], cs - 5, otu, ms, share).tobytes() == answer.tobytes(), name
        assert (np.diff(cs) > E.SHORT).any() and (np.diff(cs) <= E.SHORT).any()


# ---- j ----------------------------------------------------------------------------------------------------------------------------

def scan_table_image(train):
    """The table of the family set, as tests/test_gpu_assign.py's _table builds it (the image alone)"""
    import torch
    from kmergutsjava_amd import synth
    from kmergutsjava_amd.make_table import default_num_sigs
    sigs = M.derive(*train, 2, 80)
    rec, _ = synth.build_table(torch.from_numpy(sigs["kmer"].copy()),
                               tuple(torch.from_numpy(sigs[k].copy()) for k in ("otuIndex", "avgFromEnd", "functionIndex", "functionWt")),
                               default_num_sigs(len(sigs)))
    return synth.table_image(rec)


def check_scan_records(ora, chimeras, order_constraint):
    """The condition on the input: what the oracle emits for the two chimeras.  -> their CALL counts"""
    cs = ora["container_call_start"]
    cyc, two = (ora["calls"][cs[p]:cs[p + 1]] for p in chimeras)
    assert cs[chimeras[0] + 2] == cs[chimeras[0] + 1]           # the empty protein between them
    assert len(set(two["fI"].tolist())) == 2
    if order_constraint:
        assert len(cyc) > E.SHORT and len(two) > E.SHORT
    else:
        assert len(cyc) > E.WAVE and len(set(cyc["fI"].tolist())) > E.SHORT and len(two) > E.WAVE
    return len(cyc), len(two)


@pytest.mark.parametrize("oc", [False, True])
def test_scan_inputs_reach_the_long_path(oracle, oc):
    train, (qseq, qoff), chimeras = E.scan_inputs()
    assert len(qoff) == len(train[1]) + 3 and qoff[chimeras[0] + 1] - qoff[chimeras[0]] == E.SEGMENTS * E.SEGMENT == 9000
    ora = oracle.run(scan_table_image(train), np.frombuffer(qseq, dtype=np.uint8), qoff, aa=True, lookup_mode=1, order_constraint=oc)
    check_scan_records(ora, chimeras, oc)
    want = A.assign(ora["calls"], ora["container_call_start"], ora["otu"])
    assert want.tobytes() == A.brute_force(ora["calls"], ora["container_call_start"], ora["otu"]).tobytes()
    assert want["n_functions"][chimeras[1]] == 2 and want["n_calls"][chimeras[0] + 1] == 0
