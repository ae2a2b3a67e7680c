"""kg_proteins_cluster on its internal borders (kg_cluster.hpp, kg_host_cluster.hpp): k-mer runs against the 16 pairs of a lane
and the 4096 of a workgroup, link runs against the prefix sum's 2048-item chunk, the key widths of both sorts, the 64-window
blocks, component shapes that make many lanes hook the same roots or form deep chains, and the ranges of kg_familyset_copy.

The inputs and their answers come from tests/cluster_edge_cases.py, where the answers are worked out without the model's code
(closed forms, a token-level restatement in plain loops, a sequential union-find); tests/test_cluster_host.py checks the model
against them on the CPU.  Here every input goes through both entry points, host bytes and device bytes, and the records and
counts must equal the model's and the independent answer, byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cluster_edge_cases as E  # noqa: E402
import cluster_model as M  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(batch, answer=None, ms=1, pct=0, what=""):
    """Both entry points against cluster_numpy and, where the case has one, against its own answer.  -> (records, statistics)"""
    from kmergutsjava_amd import hotpath
    seq, off = batch
    want, counts = M.cluster_numpy(seq, off, ms, pct)
    got, st = hotpath.cluster_proteins(seq, off, min_shared=ms, min_cover_pct=pct)
    assert {k: st[k] for k in M.COUNTS} == counts, what
    assert got.tobytes() == want.tobytes(), what
    d = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    dev, dst = hotpath.cluster_proteins(None, off, min_shared=ms, min_cover_pct=pct, device_ptr=d.data_ptr() if d.numel() else 0)
    assert {k: dst[k] for k in M.COUNTS} == counts, what
    assert dev.tobytes() == want.tobytes(), what
    if answer is not None:
        assert got.tobytes() == answer[0].tobytes() and counts == answer[1], what
    return got, st


# ---- a. k-mer runs against lane and workgroup borders -------------------------------------------------------------------------

@pytest.mark.parametrize("lead,run", E.LANE_GRID)
def test_kmer_runs_at_lane_and_workgroup_borders(lead, run):
    """`lead` pairs of a smaller k-mer, the run under test, and 0 or 1 pair behind it (the run ends at end == n, or with a run
    behind it); the one longest member at the first pair, the last, and the pairs next to a lane border (E.lane_places), and all
    lengths equal.  Every other member of a run has best = its centre and shared = 1."""
    for name, batch, answer in E.lane_cases(lead, run):
        got, st = _check(batch, answer, what=name)
        assert st["links"] == st["edges"] == st["pairs"] - st["kmers"]


@pytest.mark.parametrize("name,lead,sizes", E.SHORT_RUNS, ids=[c[0] for c in E.SHORT_RUNS])
def test_many_short_kmer_runs(name, lead, sizes):
    got, st = _check(*E.short_runs_case(lead, sizes))
    assert st["kmers"] == len(sizes) + (lead > 0)


# ---- b. link runs against the scan chunk --------------------------------------------------------------------------------------

@pytest.mark.parametrize("lead_links", E.LINK_LEAD)
@pytest.mark.parametrize("s", E.LINK_S)
def test_link_runs_at_the_scan_chunk(s, lead_links):
    """Member m's run of s equal link keys starts at item lead_links of the sorted links: s(m, c) is lstart[r + 1] - lstart[r]
    across the 2048-item chunks of the prefix sum.  At the large s, both tests at their bounds."""
    got, st = _check(*E.link_case(s, lead_links))
    assert got[lead_links].tolist()[2:] == (lead_links + 1, s) and st["links"] == lead_links + 1
    if s >= 2047:
        for name, (ms, pct), batch, answer, edge in E.link_threshold_cases(s, lead_links):
            got, st = _check(batch, answer, ms, pct, what=name)
            assert got[lead_links].tolist()[2:] == ((lead_links + 1, s) if edge else (-1, 0)), name


@pytest.mark.parametrize("s,third,m_first", E.THREE_CENTRES)
def test_one_member_between_three_centres(s, third, m_first):
    """Equal s to two centres: the smaller index; a larger s to the highest-indexed centre: that one."""
    got, st = _check(*E.three_centres_case(s, third, m_first))
    m, cs = (0, (1, 2, 3)) if m_first else (3, (0, 1, 2))
    assert got[m].tolist()[2:] == ((cs[2], third) if third > s else (cs[0], s))


# ---- c. key widths ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", E.KEY_WIDTH_N)
def test_key_width_edges(n):
    """n_prot where ceil(log2 n_prot) changes: 35 + b window key bits with k-mers 0 and 20^8 - 1, 32 + b link key bits with the
    top bit of m and of c set."""
    members, pad = E.key_width_case(n)
    got, st = _check(M.token_batch(members, pad), E.token_answer(members, pad))
    assert st["families"] == 1 and st["largest"] == n


# ---- d. window blocks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("length", E.BLOCK_LENGTHS)
def test_protein_lengths_at_block_edges(length):
    prots = E.block_edge_batch(length)
    got, st = _check(M.pack(prots), None, 5, 20)
    E.check_block_edge_records(length, got, st)
    _check(M.pack(prots), None, 1, 0)


# ---- e. component shapes ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shapes():
    return E.component_shapes()


@pytest.mark.parametrize("shape", E.COMPONENT_SHAPES)
def test_component_shapes(shapes, shape):
    """root is the smallest member of the component whatever the order in which the lanes hooked: against the sequential
    union-find, twice.  rounds is printed; its only bound is the host's own guard."""
    n, edges = shapes[shape]
    batch = M.graph_batch(n, edges)
    got, st = _check(batch)
    E.check_component_records(n, edges, got, st)
    again, st2 = _check(batch)
    assert again.tobytes() == got.tobytes()
    print("%s: n = %d, edges = %d, rounds = %d and %d" % (shape, n, len(edges), st["rounds"], st2["rounds"]))
    assert 1 <= st["rounds"] <= n and 1 <= st2["rounds"] <= n


# ---- f. kg_familyset_copy ranges ----------------------------------------------------------------------------------------------

def test_familyset_copy_ranges():
    seq, off = M.pack(M.random_batch(np.random.default_rng(21), n_fam=300))
    want = M.cluster_numpy(seq, off)[0]
    lib, h = N.load(), C.c_void_p()
    arr = np.frombuffer(seq, dtype=np.uint8)
    assert lib.kg_proteins_cluster(0, C.byref(N.KgClusterParams(5, 20, 0)), arr.ctypes.data, off.ctypes.data, off.size - 1, 0, C.byref(h)) == N.KG_OK
    try:
        count = int(lib.kg_familyset_count(h))
        assert count == len(want) and 800 <= count <= 1500
        full = np.zeros(count, dtype=N.FAMILY_DTYPE)
        assert lib.kg_familyset_copy(h, 0, count, full.ctypes.data) == N.KG_OK and full.tobytes() == want.tobytes()
        guard = np.zeros(1, dtype=N.FAMILY_DTYPE)
        guard[0] = (-7, -7, -7, -7)
        for first, cnt in ((0, 0), (count, 0), (count // 3, count // 2), (count - 1, 1), (0, 1), (1, count - 1)):
            dst = np.repeat(guard, cnt + 2)                     # a record before and one behind must stay as they are
            assert lib.kg_familyset_copy(h, first, cnt, dst[1:].ctypes.data) == N.KG_OK, (first, cnt)
            assert dst[1:1 + cnt].tobytes() == full[first:first + cnt].tobytes(), (first, cnt)
            assert dst[0] == guard[0] and dst[-1] == guard[0]
        assert lib.kg_familyset_copy(h, 0, 0, None) == N.KG_OK and lib.kg_familyset_copy(h, count, 0, None) == N.KG_OK
        dst = np.repeat(guard, count + 2)
        for first, cnt in ((-1, 1), (-1, 0), (0, -1), (count, 1), (1, count), (0, count + 1), (count + 1, 0)):
            assert lib.kg_familyset_copy(h, first, cnt, dst.ctypes.data) == N.KG_ERR_ARG, (first, cnt)
            assert lib.kg_last_error() == b"kg_familyset_copy: range outside the set"
        assert lib.kg_familyset_copy(h, 0, 1, None) == N.KG_ERR_ARG and lib.kg_last_error() == b"null argument"
        assert lib.kg_familyset_copy(None, 0, 0, dst.ctypes.data) == N.KG_ERR_ARG and lib.kg_last_error() == b"null argument"
        assert (dst == guard[0]).all()                          # no failed call wrote anything
        again = np.zeros(count, dtype=N.FAMILY_DTYPE)
        assert lib.kg_familyset_copy(h, 0, count, again.ctypes.data) == N.KG_OK and again.tobytes() == want.tobytes()
    finally:
        lib.kg_familyset_free(h)
