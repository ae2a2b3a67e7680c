"""Frameshift repair on the GPU at the edges of tests/repair_edge_cases.py: chains of 8 and 9 parts at the junction bound (and one
part more, and chains that fail on the last trips of the part loop), residue lanes that hold the end of a nine-part protein,
zero-length proteins and the start of a copied one, every end search of a chain over one tile row and more on contigs of every
length mod 3 between fillers, and a second call on a set that already holds repaired records.  Everything is compared byte for
byte with tests/repair_model.py as tests/test_gpu_repair.py does it, and field by field with the answers the cases state by
construction, so that a failure names the case; tests/test_repair_edges_host.py shows that the cases are what they say."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import orfs_model as O  # noqa: E402
import regions_model as R  # noqa: E402
import repair_cases as RC  # noqa: E402
import repair_edge_cases as E  # noqa: E402
import repair_model as M  # noqa: E402
from kmergutsjava_amd import _native as N  # noqa: E402
from test_gpu_repair import NAMES, _batch, _check  # noqa: E402

pytestmark = pytest.mark.gpu
TAIL_STRAND = [(t, s) for t in E.TAILS for s in (0, 1)]
IDS = ["tail%d%s" % (len(t), "-" if s else "+") for t, s in TAIL_STRAND]


@pytest.mark.parametrize("tail,strand", TAIL_STRAND, ids=IDS)
def test_chains_at_the_junction_bound(tail, strand):
    """8 and 9 parts with max_junctions = 8, 10 parts and 9 with max_junctions = 7 skipped, an empty ninth and eighth part and
    J_7 >= J_8: each alone, then all in one batch between the hand-made chains of tests/repair_cases.py."""
    cases = E.chain_cases(tail, strand)
    for k, c in enumerate(cases):
        want, _ = _check(*RC.lay(c["text"], strand, c["calls"]), start_codons=1, device_inputs=bool(k & 1), **c["params"])
        assert want[5]["candidates"] == 1 and want[5][c["state"]] == 1, (c["name"], want[5])
        if c["state"] == "repaired":
            E.assert_answers(c, want[0][0], want[3])
            assert want[5]["junctions"] == len(c["calls"]) - 1
    items, states = E.interleaved(cases, strand)
    want, _ = _check(*_batch(items), start_codons=1, max_junctions=E.MAX_J, device_inputs=bool(strand))
    E.assert_states(states, want[0], want[4], "interleaved")
    for at, (text, _, calls) in enumerate(items):
        c = next((c for c in cases if c["text"] == text and c["calls"] == list(calls)), None)
        if c is not None and c["state"] == "repaired":
            E.assert_answers(c, want[0][at], want[3][want[4][at]:want[4][at + 1]])
    assert (np.diff(want[4]) == E.MAX_J).sum() == 2


@pytest.mark.parametrize("only_kept", [True, False])
def test_lanes_across_orf_borders(only_kept):
    """The nine-part protein begins at every position of a residue lane; behind it stand two regions that are not kept and a
    single-frame one, whose protein is copied."""
    for p in range(E.LANE):
        items, at, chain = E.lane_batch(p)
        want, (regs, _, _, _) = _check(*_batch(items), min_score=E.LANE_MIN_SCORE, only_kept=only_kept, start_codons=1, max_junctions=E.MAX_J,
                                       device_inputs=bool(p & 1))
        assert want[5]["repaired"] == p + 1 and want[5]["junctions"] == p + E.MAX_J and want[5]["single"] == want[5]["skipped"] == 0, (p, want[5])
        assert regs["kept"].tolist() == [1] * (p + 1) + [0, 0, 1] and want[1][at] % E.LANE == p
        E.assert_answers(chain, want[0][at], want[3][want[4][at]:want[4][at + 1]])
        lens = np.diff(want[1])
        assert (lens[at + 1:at + 3] == 0).all() == only_kept and lens[at + 3] > 0 and not want[0]["flags"][at + 3] & M.REPAIRED, p


@pytest.mark.parametrize("tail,strand", TAIL_STRAND, ids=IDS)
def test_far_ends(tail, strand):
    """The start, the stop in front of it, the first inner stop of parts 1 and 2 and the end, each 0 or 1, T - 1, T, T + 1 and
    2 T + 1 codons from where its search begins, and not there at all: one contig each in one batch, every one between two fillers
    of three tile rows.  The chains without a start once more with start_codons = 0."""
    cases = E.far_cases(tail, strand)
    for sc, sel in ((1, cases), (0, [c for c in cases if c["name"].startswith("nostart")])):
        want, _ = _check(*_batch(E.far_batch(sel, strand)), start_codons=sc, device_inputs=bool(sc))
        E.assert_states(["repaired"] * len(sel), want[0], want[4], "far ends")
        for k, c in enumerate(sel):
            E.assert_answers(c, want[0][k], want[3][want[4][k]:want[4][k + 1]])


def _second_call(case, through_starts):
    """kg_regions_calls, kg_regionset_orfs, kg_regionset_repair with the defaults, (kg_orfset_starts, untrained,) and
    kg_regionset_repair with the case's parameters on the set that came out -> (the first call's set, the second call's)"""
    from kmergutsjava_amd import hotpath
    lib = N.load()
    calls, seq, off = _batch(case["items"])
    sb = np.ascontiguousarray(seq, dtype=np.uint8)
    n_seqs = len(off) - 1
    batch = (sb.ctypes.data, 0, off.ctypes.data, n_seqs)
    kw = dict(min_count=0, max_junctions=4)
    kw.update(case["params"])
    table = np.zeros(N.CODING_BINS, dtype=np.int32)
    rh, oh, h1, hs, h2 = (C.c_void_p() for _ in range(5))

    def take(h):
        o, ps, res, _ = hotpath._take_orfset(h, False, free=False)
        return (o, ps, res) + hotpath._junctions(h)

    N.check(lib.kg_regions_calls(0, C.byref(N.KgRegionParams(600, 0, 0)), calls.ctypes.data, calls.size, off.ctypes.data, n_seqs, C.byref(rh)))
    try:
        N.check(lib.kg_regionset_orfs(rh, C.byref(N.KgOrfParams(1, 1, 0)), *batch, C.byref(oh)))
        N.check(lib.kg_regionset_repair(rh, oh, calls.ctypes.data, 0, calls.size, C.byref(N.KgRepairParams(1, 0, 4, 0)), *batch, C.byref(h1)))
        first = take(h1)
        given = h1
        if through_starts:
            N.check(lib.kg_orfset_starts(h1, C.byref(N.KgStartParams(30, 1, 2, 0, 1 << 62)), table.ctypes.data, None, rh, *batch, C.byref(hs)))
            given = hs
            moved = hotpath._take_orfset(hs, False, free=False)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(moved[:3], first[:3])), case["name"]
        N.check(lib.kg_regionset_repair(rh, given, calls.ctypes.data, 0, calls.size,
                                        C.byref(N.KgRepairParams(1, kw["min_count"], kw["max_junctions"], 0)), *batch, C.byref(h2)))
        return (calls, seq, off), first, take(h2)
    finally:
        for h in (h2, hs, h1, oh):
            if h:
                lib.kg_orfset_free(h)
        lib.kg_regionset_free(rh)


def _second_pass_holds(case, through_starts):
    (calls, seq, off), first, second = _second_call(case, through_starts)
    regs, _ = R.regions(calls, off)
    o, ps, res = O.orfs(regs, seq, off, start_codons=1)
    w1 = M.repair(regs, o, ps, res, calls, seq, off, start_codons=1)
    w2 = M.repair(regs, w1[0], w1[1], w1[2], calls, seq, off, start_codons=1, **case["params"])
    for got, want, call in ((first, w1, "first"), (second, w2, "second")):
        for name, g, w in zip(NAMES, got[:5], want[:5]):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (case["name"], call, name, g, w)
        assert {k: got[5][k] for k in M.STAT_KEYS} == want[5], (case["name"], call, got[5], want[5])
    assert w1[5]["repaired"] == len(case["states"]) and [w2[5][s] for s in ("repaired", "skipped", "single")] == \
        [case["states"].count(s) for s in ("repaired", "skipped", "single")], (case["name"], w2[5])
    # what the second call leaves alone keeps its record and protein, flag and all, and has no junction in the new list
    assert second[0].tobytes() == first[0].tobytes() and second[2].tobytes() == first[2].tobytes() and (second[0]["flags"] & M.REPAIRED).all()
    assert np.diff(second[4]).tolist() == [n if s == "repaired" else 0 for n, s in zip(np.diff(first[4]).tolist(), case["states"])], case["name"]


@pytest.mark.parametrize("through_starts", [False, True], ids=["repaired-set", "starts-of-it"])
def test_a_second_call_keeps_what_it_does_not_repair(through_starts):
    """A region repaired by the first call and skipped or single in the second keeps its record and its protein byte for byte, and
    the junction list is the second call's alone: alone, in front of and behind a region that is repaired again, on the set of
    the first call and on the one kg_orfset_starts makes from it.  When the sets are freed no device memory stays in use."""
    import torch
    cases = E.second_pass_cases()
    _second_call(cases[0], through_starts)          # once first: what the runtime sets up on first use is not counted
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for case in cases:
        _second_pass_holds(case, through_starts)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0, "the freed sets left device memory in use"


def test_the_later_stages_keep_a_repaired_protein():
    """kg_orfset_add_free and kg_orfset_starts write the proteins of the set they make from its records, which a repaired record's
    protein cannot be read from: three repaired regions (two, three and nine parts, both strands) keep record and protein through
    both, in front of the free candidates, whose bytes are the free model's."""
    import free_orfs_model as F
    from kmergutsjava_amd import hotpath
    lib = N.load()
    by_name = {c["name"]: c for c in RC.cases()}
    chain = E.chain_cases(b"G", 1)[1]
    items = [(by_name["three"]["text"], 0, by_name["three"]["calls"]), (by_name["deletion"]["text"], 1, by_name["deletion"]["calls"]),
             (chain["text"], chain["strand"], chain["calls"])]
    calls, seq, off = _batch(items)
    sb = np.ascontiguousarray(seq, dtype=np.uint8)
    batch = (sb.ctypes.data, 0, off.ctypes.data, len(off) - 1)
    regs, _ = R.regions(calls, off)
    want = M.repair(regs, *O.orfs(regs, seq, off, start_codons=1), calls, seq, off, start_codons=1, max_junctions=E.MAX_J)
    assert want[5]["repaired"] == 3 and np.diff(want[4]).tolist() == [2, 1, E.MAX_J]
    full = F.concat(want[:3], F.free_orfs(seq, off, 10, 1))
    assert len(full[0]) > 3
    table = np.zeros(N.CODING_BINS, dtype=np.int32)
    rh, oh, h1, hf, hs = (C.c_void_p() for _ in range(5))
    N.check(lib.kg_regions_calls(0, C.byref(N.KgRegionParams(600, 0, 0)), calls.ctypes.data, calls.size, off.ctypes.data, len(off) - 1, C.byref(rh)))
    try:
        N.check(lib.kg_regionset_orfs(rh, C.byref(N.KgOrfParams(1, 1, 0)), *batch, C.byref(oh)))
        N.check(lib.kg_regionset_repair(rh, oh, calls.ctypes.data, 0, calls.size, C.byref(N.KgRepairParams(1, 0, E.MAX_J, 0)), *batch, C.byref(h1)))
        N.check(lib.kg_orfset_add_free(h1, C.byref(N.KgFreeParams(10, 1, 0)), *batch, C.byref(hf)))
        N.check(lib.kg_orfset_starts(hf, C.byref(N.KgStartParams(30, 1, 2, 0, 1 << 62)), table.ctypes.data, None, rh, *batch, C.byref(hs)))
        for h, stage, model in ((h1, "repair", want[:3]), (hf, "add_free", full), (hs, "starts", full)):
            got = hotpath._take_orfset(h, False, free=False)
            for name, g, w in zip(NAMES, got[:3], model):
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (stage, name, g, w)
    finally:
        for h in (hs, hf, h1, oh):
            if h:
                lib.kg_orfset_free(h)
        lib.kg_regionset_free(rh)
