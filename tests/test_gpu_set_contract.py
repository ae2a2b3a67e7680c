"""What the seven result sets of the C ABI promise alike (kg_sigset, kg_familyset, kg_regionset, kg_orfset, kg_selectset,
kg_voteset, kg_compset), each built at the smallest shape that still yields a non-empty set: every range getter refuses a
bad range and a null set with its own words, copies nothing for count = 0, and a whole copy is two half copies; the start
arrays come whole; the statistics getter refuses null; free takes null; a set that owns its context gives all device memory
back, and a set on a borrowed table holds blocks of the table's cache only until it is freed.

The error texts are written out here as include/kmerguts_hip.h's callers have always seen them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compose_cases as CC  # noqa: E402
import otu_votes_cases as VC  # noqa: E402
import repair_cases as RC  # noqa: E402
import select_model as S  # noqa: E402
import signature_model as M  # noqa: E402
import test_orfs_host as HO  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

NULL_ARG = "null argument"
KINDS = ["sigset", "familyset", "regionset", "orfset", "selectset", "voteset", "compset"]
OWNS_CONTEXT = {"regionset", "orfset", "selectset", "voteset", "compset"}


class Getter:
    """One range getter: fn(handle, first, count, dst) over `have` records of `size` bytes; text: what a bad range says."""

    def __init__(self, h, fn, name, have, size, of="the set", null_dst_is_an_error=True):
        self.h, self.fn, self.name, self.have, self.size = h, fn, name, int(have), int(size)
        self.text = "%s: range outside %s" % (name, of)
        self.null_dst_is_an_error = null_dst_is_an_error


class Built:
    """The sets of one case.  getters: every range getter, on the set that has its array; starts: (handle, fn, n, total) of the
    whole-array getters; stats: (fn, handle, struct); refused: (call, text) of the getters that first ask whether the set has
    the array; frees: (fn, handle) in the order the sets must go."""

    def __init__(self):
        self.getters, self.starts, self.stats, self.refused, self.frees = [], [], None, [], []

    def free(self):
        for fn, h in self.frees:
            fn(h)
        self.frees = []


def _err():
    return N.load().kg_last_error().decode()


def _ptr(a):
    return a.ctypes.data if a.size else None


def _proteins():
    """four short proteins, one family and one function: (bytes, offsets, fn, otu)"""
    rng = np.random.default_rng(11)
    one = np.frombuffer(M.ALPHA, dtype=np.uint8)[rng.integers(0, 20, size=30)]
    seq = np.ascontiguousarray(np.tile(one, 4))
    return seq, np.arange(5, dtype=np.int64) * 30, np.full(4, 3, dtype=np.int32), np.full(4, 1, dtype=np.int32)


def _two_repair_contigs():
    """repair_cases' deletion chain on two contigs: (CALLs in container order, bytes, offsets)"""
    case = RC.cases()[0]
    calls, contig, _ = RC.lay(case["text"], 0, case["calls"])
    second = calls.copy()
    second["container"] += 6
    return np.concatenate([calls, second]), np.concatenate([contig, contig]), np.array([0, RC.L, 2 * RC.L], dtype=np.int64)


def _build_sigset(lib, b):
    seq, off, fn, otu = _proteins()
    h = C.c_void_p()
    N.check(lib.kg_signatures_derive(0, C.byref(N.KgDeriveParams(2, 80, 0)), _ptr(seq), off.ctypes.data, 4, _ptr(fn), _ptr(otu), C.byref(h)))
    b.frees.append((lib.kg_sigset_free, h))
    b.getters.append(Getter(h, lib.kg_sigset_copy, "kg_sigset_copy", lib.kg_sigset_count(h), 24))
    b.stats = (lib.kg_sigset_stats, h, N.KgDeriveStats)


def _build_familyset(lib, b):
    seq, off, _, _ = _proteins()
    h = C.c_void_p()
    N.check(lib.kg_proteins_cluster(0, C.byref(N.KgClusterParams(5, 20, 0)), _ptr(seq), off.ctypes.data, 4, 0, C.byref(h)))
    b.frees.append((lib.kg_familyset_free, h))
    b.getters.append(Getter(h, lib.kg_familyset_copy, "kg_familyset_copy", lib.kg_familyset_count(h), 16))
    b.stats = (lib.kg_familyset_stats, h, N.KgClusterStats)


def _regions_of(lib, calls, off):
    h = C.c_void_p()
    N.check(lib.kg_regions_calls(0, C.byref(N.KgRegionParams(600, 0, 0)), _ptr(calls), calls.size, off.ctypes.data, off.size - 1, C.byref(h)))
    return h


def _build_regionset(lib, b):
    calls, _, off = _two_repair_contigs()
    h = _regions_of(lib, calls, off)
    b.frees.append((lib.kg_regionset_free, h))
    n = lib.kg_regionset_count(h)
    b.getters.append(Getter(h, lib.kg_regionset_copy, "kg_regionset_copy", n, N.REGION_DTYPE.itemsize))
    b.starts.append((h, lib.kg_regionset_seq_start, 2, n))
    b.stats = (lib.kg_regionset_stats, h, N.KgRegionStats)


def _build_orfset(lib, b):
    # the free ORFs of two contigs, then their scores and their starts: three sets in the first one's context
    rng = np.random.default_rng(5)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=700)].copy()
    off = np.array([0, 320, 700], dtype=np.int64)
    free, scored, moved = C.c_void_p(), C.c_void_p(), C.c_void_p()
    N.check(lib.kg_orfs_free(0, C.byref(N.KgFreeParams(10, 7, 0)), _ptr(seq), 0, off.ctypes.data, 2, C.byref(free)))
    b.frees.append((lib.kg_orfset_free, free))
    N.check(lib.kg_orfset_coding(free, C.byref(N.KgCodingParams(0, 0, 0)), None, _ptr(seq), 0, off.ctypes.data, 2, C.byref(scored)))
    b.frees.insert(0, (lib.kg_orfset_free, scored))
    table = np.zeros(N.CODING_BINS, dtype=np.int32)
    N.check(lib.kg_orfset_starts(scored, C.byref(N.KgStartParams(10, 7, 1, 0, 0)), table.ctypes.data, None, None, _ptr(seq), 0, off.ctypes.data,
                                 2, C.byref(moved)))
    b.frees.insert(0, (lib.kg_orfset_free, moved))
    st = N.KgOrfStats()
    N.check(lib.kg_orfset_stats(free, C.byref(st)))
    n = lib.kg_orfset_count(free)
    b.getters.append(Getter(free, lib.kg_orfset_copy, "kg_orfset_copy", n, N.ORF_DTYPE.itemsize))
    b.getters.append(Getter(free, lib.kg_orfset_residues, "kg_orfset_residues", st.residues, 1, "the proteins"))
    b.getters.append(Getter(scored, lib.kg_orfset_coding_scores, "kg_orfset_coding_scores", n, 8))
    b.getters.append(Getter(moved, lib.kg_orfset_start_shifts, "kg_orfset_start_shifts", n, 4))
    b.starts.append((free, lib.kg_orfset_prot_start, n, st.residues))
    b.stats = (lib.kg_orfset_stats, free, N.KgOrfStats)
    # ... and a repaired set with its junction list, in a region set's context
    calls, contigs, roff = _two_repair_contigs()
    rh, oh, fixed = _regions_of(lib, calls, roff), C.c_void_p(), C.c_void_p()
    b.frees.append((lib.kg_regionset_free, rh))
    N.check(lib.kg_regionset_orfs(rh, C.byref(N.KgOrfParams(1, 0, 0)), _ptr(contigs), 0, roff.ctypes.data, 2, C.byref(oh)))
    b.frees.insert(0, (lib.kg_orfset_free, oh))
    N.check(lib.kg_regionset_repair(rh, oh, _ptr(calls), 0, calls.size, C.byref(N.KgRepairParams(1, 0, 4, 0)), _ptr(contigs), 0, roff.ctypes.data, 2,
                                    C.byref(fixed)))
    b.frees.insert(0, (lib.kg_orfset_free, fixed))
    nj = lib.kg_orfset_junctions_count(fixed)
    b.getters.append(Getter(fixed, lib.kg_orfset_junctions_copy, "kg_orfset_junctions_copy", nj, N.JUNCTION_DTYPE.itemsize, "the list"))
    b.starts.append((fixed, lib.kg_orfset_junctions_start, lib.kg_orfset_count(fixed), nj))
    # the arrays a set may lack are asked for first: a bad range on a set without them says so, not "range outside"
    buf = np.zeros(8, dtype=np.int64)
    b.refused = [(lambda: lib.kg_orfset_coding_scores(free, -1, 1, buf.ctypes.data),
                  "kg_orfset_coding_scores: the set has no scores (it is not from kg_orfset_coding)"),
                 (lambda: lib.kg_orfset_start_shifts(scored, -1, 1, buf.ctypes.data),
                  "kg_orfset_start_shifts: the set has no shifts (it is not from kg_orfset_starts)"),
                 (lambda: lib.kg_orfset_junctions_copy(moved, -1, 1, buf.ctypes.data),
                  "kg_orfset_junctions_copy: the set is not from kg_regionset_repair"),
                 (lambda: lib.kg_orfset_junctions_start(oh, buf.ctypes.data),
                  "kg_orfset_junctions_start: the set is not from kg_regionset_repair")]


def _build_selectset(lib, b):
    iv = S.intervals([(0, 100, 400, 7), (0, 300, 600, 9), (1, 0, 50, 3), (1, 40, 90, 3)])
    h = C.c_void_p()
    N.check(lib.kg_select_intervals(0, C.byref(N.KgSelectParams(60, 50, 0)), _ptr(iv), iv.size, 2, C.byref(h)))
    b.frees.append((lib.kg_selectset_free, h))
    b.getters.append(Getter(h, lib.kg_selectset_copy, "kg_selectset_copy", lib.kg_selectset_count(h), N.SELECTION_DTYPE.itemsize))
    b.stats = (lib.kg_selectset_stats, h, N.KgSelectStats)


def _build_voteset(lib, b):
    hits, chs, ev, calls, ccs, n_seqs, per, off = VC.Lists(2, 6).call(0, 5, 3, 1).call(2, 9, 2, 4).call(7, 5, 2, 2).build()
    h = C.c_void_p()
    N.check(lib.kg_otu_votes_hits(0, C.byref(N.KgVoteParams(1, 50, 1, 0)), _ptr(hits), chs.ctypes.data, _ptr(ev), _ptr(calls), ccs.ctypes.data,
                                  n_seqs, per, off.ctypes.data, C.byref(h)))
    b.frees.append((lib.kg_voteset_free, h))
    n = lib.kg_voteset_count(h)
    b.getters.append(Getter(h, lib.kg_voteset_copy_votes, "kg_voteset_copy_votes", n, N.VOTE_DTYPE.itemsize))
    b.getters.append(Getter(h, lib.kg_voteset_copy_classes, "kg_voteset_copy_classes", n_seqs, N.OTU_CLASS_DTYPE.itemsize))
    b.getters.append(Getter(h, lib.kg_voteset_copy_bins, "kg_voteset_copy_bins", lib.kg_voteset_bins(h), N.OTU_BIN_DTYPE.itemsize))
    b.starts.append((h, lib.kg_voteset_seq_start, n_seqs, n))
    b.stats = (lib.kg_voteset_stats, h, N.KgVoteStats)


def _build_compset(lib, b):
    seq, off, _ = CC.batch(np.random.default_rng(3), [2000, 2100, 1900])
    labels = np.array([0, 1, -1], dtype=np.int32)
    h, plain = C.c_void_p(), C.c_void_p()
    for keep, out in ((1, h), (0, plain)):
        N.check(lib.kg_contigs_compose(0, C.byref(N.KgCompParams(0, 0, 0, keep, 0)), _ptr(seq), 0, off.ctypes.data, 3, labels.ctypes.data, None, None, 0,
                                       C.byref(out)))
        b.frees.append((lib.kg_compset_free, out))
    models = lib.kg_compset_models(h)
    b.getters.append(Getter(h, lib.kg_compset_copy_classes, "kg_compset_copy_classes", 3, N.COMP_CLASS_DTYPE.itemsize))
    b.getters.append(Getter(h, lib.kg_compset_copy_counts, "kg_compset_copy_counts", 3, 4 * N.COMP_BINS))
    b.getters.append(Getter(h, lib.kg_compset_model_labels, "kg_compset_model_labels", models, 4))
    b.getters.append(Getter(h, lib.kg_compset_copy_scores, "kg_compset_copy_scores", 3, 8 * (models + 1)))
    # (the label rows: two destinations, either may be null; here the labels alone)
    b.getters.append(Getter(h, lambda s, first, count, dst: lib.kg_compset_copy_rows(s, first, count, dst, None), "kg_compset_copy_rows",
                            lib.kg_compset_rows(h), 4, null_dst_is_an_error=False))
    b.stats = (lib.kg_compset_stats, h, N.KgCompStats)
    buf = np.zeros(64, dtype=np.int64)
    b.refused = [(lambda: lib.kg_compset_copy_scores(plain, -1, 1, buf.ctypes.data),
                  "kg_compset_copy_scores: the call did not keep the score matrix (keep_scores was 0)")]


def _build(kind):
    b = Built()
    try:
        globals()["_build_" + kind](N.load(), b)
    except BaseException:
        b.free()
        raise
    return b


def _check(b):
    for g in b.getters:
        assert g.have > 0, g.name
        whole = np.zeros(g.have * g.size, dtype=np.uint8)
        assert g.fn(g.h, 0, g.have, whole.ctypes.data) == N.KG_OK, _err()
        for first, count in ((-1, 1), (0, g.have + 1), (g.have, 1), (1, g.have), (0, -1)):
            assert g.fn(g.h, first, count, whole.ctypes.data) == N.KG_ERR_ARG and _err() == g.text, (g.name, first, count)
        assert g.fn(None, 0, 0, whole.ctypes.data) == N.KG_ERR_ARG and _err() == NULL_ARG, g.name
        if g.null_dst_is_an_error:
            assert g.fn(g.h, 0, 1, None) == N.KG_ERR_ARG and _err() == NULL_ARG, g.name
        for first in (0, g.have):
            assert g.fn(g.h, first, 0, None) == N.KG_OK, g.name
        # two halves
        cut = (g.have + 1) // 2
        halves = np.full(g.have * g.size, 0xA5, dtype=np.uint8)
        assert g.fn(g.h, 0, cut, halves.ctypes.data) == N.KG_OK, _err()
        assert g.fn(g.h, cut, g.have - cut, halves.ctypes.data + cut * g.size if g.have > cut else None) == N.KG_OK, _err()
        assert halves.tobytes() == whole.tobytes(), g.name
    for h, fn, n, total in b.starts:
        start = np.full(n + 1, -1, dtype=np.int64)
        assert fn(h, start.ctypes.data) == N.KG_OK, _err()
        assert start[0] == 0 and start[-1] == total and (np.diff(start) >= 0).all()
        assert fn(None, start.ctypes.data) == N.KG_ERR_ARG and _err() == NULL_ARG
        assert fn(h, None) == N.KG_ERR_ARG and _err() == NULL_ARG
    for call, text in b.refused:
        assert call() == N.KG_ERR_ARG and _err() == text
    fn, h, struct = b.stats
    st = struct()
    assert fn(h, C.byref(st)) == N.KG_OK, _err()
    assert fn(h, None) == N.KG_ERR_ARG and _err() == NULL_ARG
    assert fn(None, C.byref(st)) == N.KG_ERR_ARG and _err() == NULL_ARG
    for free, _ in b.frees:
        free(None)


@pytest.mark.parametrize("kind", KINDS)
def test_the_getters_of_a_set_keep_the_contract(kind):
    _build(kind).free()                 # once first: what the runtime sets up on first use is not counted
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    b = _build(kind)
    try:
        _check(b)
    finally:
        b.free()
    if kind in OWNS_CONTEXT:
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "the freed set left device memory in use"


_WORK = {}


@pytest.fixture(scope="module")
def scanned():
    """a table, a DNA scan of planted genes on it and the batch's offsets"""
    from kmergutsjava_amd import hotpath
    if not _WORK:
        _WORK["w"] = HO.planted_orf_contigs()
    img, dna, off, _ = _WORK["w"]
    sb = np.frombuffer(dna, dtype=np.uint8)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(sb, off, hotpath.Params()) as r:
        yield tab, r, sb, np.ascontiguousarray(off, dtype=np.int64)


@pytest.mark.parametrize("kind", ["regionset", "orfset", "selectset", "voteset"])
def test_a_set_on_a_borrowed_table_holds_its_blocks_until_it_is_freed(scanned, kind):
    tab, r, sb, off = scanned
    lib, rh, h = N.load(), C.c_void_p(), C.c_void_p()
    n_seqs = off.size - 1
    live0 = tab.live_device_bytes()
    if kind == "voteset":
        N.check(lib.kg_result_otu_votes(r._h, C.byref(N.KgVoteParams(1, 50, 1, 0)), off.ctypes.data, C.byref(h)))
        count, free = lib.kg_voteset_count(h), lib.kg_voteset_free
    else:
        N.check(lib.kg_result_regions(r._h, C.byref(N.KgRegionParams(600, 0, 0)), off.ctypes.data, C.byref(rh)))
        count, free = lib.kg_regionset_count(rh), lib.kg_regionset_free
    live_first = tab.live_device_bytes()
    try:
        assert count > 0 and live_first > live0
        if kind == "orfset":
            N.check(lib.kg_regionset_orfs(rh, C.byref(N.KgOrfParams(7, 0, 0)), sb.ctypes.data, 0, off.ctypes.data, n_seqs, C.byref(h)))
            count, free = lib.kg_orfset_count(h), lib.kg_orfset_free
        elif kind == "selectset":
            N.check(lib.kg_regionset_select(rh, C.byref(N.KgSelectParams(60, 50, 0)), C.byref(h)))
            count, free = lib.kg_selectset_count(h), lib.kg_selectset_free
        if kind in ("orfset", "selectset"):
            try:
                assert count > 0 and tab.live_device_bytes() > live_first
            finally:
                free(h)
                h = C.c_void_p()
            assert tab.live_device_bytes() == live_first
    finally:
        if rh:
            lib.kg_regionset_free(rh)
        if h:
            free(h)
    assert tab.live_device_bytes() == live0
