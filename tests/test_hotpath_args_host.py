"""The argument checks of kmergutsjava_amd.hotpath that run before the library is used: every malformed argument a public
function names raises ValueError with its text.  No library and no GPU take part: _native.load is replaced by an object that
raises when anything of it is touched, and the methods of ScanResult / SignatureTable run on stubs that hold a handle only."""
import ctypes as C

import numpy as np
import pytest

from kmergutsjava_amd import _native as N
from kmergutsjava_amd import hotpath as H


class _LibraryUsed(Exception):
    pass


class _NoLibrary:
    def __getattr__(self, name):
        raise _LibraryUsed(name)


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    monkeypatch.setattr(N, "load", lambda: _NoLibrary())


class _Result(H.ScanResult):
    def __init__(self, n_seqs=2, handle=1):
        self._h = C.c_void_p(handle)
        self.stats = {"n_seqs": n_seqs}

    def close(self):
        pass


class _Table(H.SignatureTable):
    def __init__(self, handle=1):
        self._h = C.c_void_p(handle)
        self.device = 0

    def close(self):
        pass


class _Tensor:
    """What build / merge_signatures look at of a CUDA tensor."""
    is_cuda = True

    class device:
        index = 0

    def __init__(self, nbytes, contiguous=True):
        self.nbytes, self.contiguous = nbytes, contiguous

    def is_contiguous(self):
        return self.contiguous

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1

    def data_ptr(self):
        return 256


SEQ = b"ACGTACGT"
OFF = [0, 4, 8]
TWO_D = [[0, 4, 8]]
A = "offsets must be int64[n_seqs + 1]"
P = "offsets must be int64[n_prot + 1]"
GIVEN = "offsets must be the int64[n_seqs + 1] the scan was given"
SHORT = "sequence buffer shorter than offsets[-1]"
TABLE = "a coding score table is int32[%d]" % N.CODING_BINS
WEIGHTS = "start weights are a pair (pos int32[%d][4], type int32[4])" % N.START_WINDOW
T = np.zeros(N.CODING_BINS, np.int32)
NO_ORFS = np.zeros(0, N.ORF_DTYPE)
NO_CALLS = np.zeros(0, N.CALL_DTYPE)
NO_HITS = np.zeros(0, N.HIT_DTYPE)
W = (np.zeros((N.START_WINDOW, 4), np.int32), np.zeros(4, np.int32))


def _votes(offsets=OFF, chs=None, ccs=None, ev=None):
    z = np.zeros(13, np.int64)
    return H.otu_votes(NO_HITS, z if chs is None else chs, np.zeros(0, np.uint8) if ev is None else ev, NO_CALLS,
                       z if ccs is None else ccs, 2, 6, offsets)


CASES = [
    # ---- offsets of the wrong rank or length ----
    ("scan rank", lambda: _Table().scan(SEQ, TWO_D), A),
    ("scan empty", lambda: _Table().scan(SEQ, []), A),
    ("derive rank", lambda: H.derive_signatures(SEQ, TWO_D, [0], [0]), P),
    ("derive empty", lambda: H.derive_signatures(SEQ, [], [], []), P),
    ("align rank", lambda: H.align_proteins(SEQ, TWO_D, []), P),
    ("align empty", lambda: H.align_proteins(SEQ, [], []), P),
    ("cluster rank", lambda: H.cluster_proteins(SEQ, TWO_D), P),
    ("search rank", lambda: H.search_proteins(SEQ, TWO_D, 1), P),
    ("region_calls rank", lambda: H.region_calls(NO_CALLS, TWO_D), A),
    ("region_calls empty", lambda: H.region_calls(NO_CALLS, []), A),
    ("otu_votes length", lambda: _votes(offsets=[0, 8]), A),
    ("otu_votes rank", lambda: _votes(offsets=TWO_D), A),
    ("compose rank", lambda: H.compose_contigs(SEQ, TWO_D), A),
    ("repair_orfs rank", lambda: H.repair_orfs(NO_CALLS, SEQ, TWO_D), A),
    ("repair_orfs empty", lambda: H.repair_orfs(NO_CALLS, SEQ, []), A),
    ("choose_starts rank", lambda: H.choose_starts(T, NO_ORFS, SEQ, TWO_D), A),
    ("start_counts rank", lambda: H.start_counts(T, NO_ORFS, SEQ, TWO_D), A),
    ("coding_counts rank", lambda: H.coding_counts(NO_ORFS, SEQ, TWO_D), A),
    ("coding_scores rank", lambda: H.coding_scores(T, NO_ORFS, SEQ, TWO_D), A),
    ("free_orfs rank", lambda: H.free_orfs(SEQ, TWO_D), A),
    ("free_orfs empty", lambda: H.free_orfs(SEQ, []), A),
    ("orf_regions rank", lambda: H.orf_regions(np.zeros(0, N.REGION_DTYPE), SEQ, TWO_D), A),
    ("regions length", lambda: _Result(2).regions([0, 8]), GIVEN),
    ("regions rank", lambda: _Result(2).regions(TWO_D), GIVEN),
    ("result otu_votes length", lambda: _Result(2).otu_votes([0, 8]), GIVEN),
    ("orfs length", lambda: _Result(2).orfs(SEQ, [0, 8]), GIVEN),
    ("orfs rank", lambda: _Result(2).orfs(SEQ, TWO_D), GIVEN),
    ("select length", lambda: _Result(2).select([0, 4, 8, 8]), GIVEN),
    ("select rank", lambda: _Result(2).select(TWO_D, SEQ, orfs=True), GIVEN),
    # ---- a short sequence buffer ----
    ("scan short", lambda: _Table().scan(SEQ[:7], OFF), SHORT),
    ("derive short", lambda: H.derive_signatures(SEQ[:7], OFF, [0, 0], [0, 0]), SHORT),
    ("align short", lambda: H.align_proteins(SEQ[:7], OFF, [[0, 1]]), SHORT),
    ("cluster short", lambda: H.cluster_proteins(SEQ[:7], OFF), SHORT),
    ("cluster aligned short", lambda: H.cluster_proteins(np.frombuffer(SEQ[:7], np.uint8), OFF, align={}), SHORT),
    ("search short", lambda: H.search_proteins(SEQ[:7], OFF, 1), SHORT),
    ("compose short", lambda: H.compose_contigs(SEQ[:7], OFF), SHORT),
    ("repair_orfs short", lambda: H.repair_orfs(NO_CALLS, SEQ[:7], OFF), SHORT),
    ("choose_starts short", lambda: H.choose_starts(T, NO_ORFS, SEQ[:7], OFF), SHORT),
    ("coding_counts short", lambda: H.coding_counts(NO_ORFS, SEQ[:7], OFF), SHORT),
    ("coding_scores short", lambda: H.coding_scores(T, NO_ORFS, SEQ[:7], OFF), SHORT),
    ("free_orfs short", lambda: H.free_orfs(SEQ[:7], OFF), SHORT),
    ("orf_regions short", lambda: H.orf_regions(np.zeros(0, N.REGION_DTYPE), SEQ[:7], OFF), SHORT),
    # no sequence, offsets = [3], no bytes: scan looks at offsets[-1] all the same (the others: below)
    ("scan no sequence", lambda: _Table().scan(b"", [3]), SHORT),
    # ---- signatures ----
    ("build 23 bytes", lambda: H.SignatureTable.build(b"x" * 23, 64), "signature bytes must be a multiple of 24"),
    ("build 23 uint8", lambda: H.SignatureTable.build(np.zeros(23, np.uint8), 64), "signature bytes must be a multiple of 24"),
    ("build strided tensor", lambda: H.SignatureTable.build(_Tensor(48, False), 64), "the signature tensor must be contiguous"),
    ("build 24n + 1 tensor", lambda: H.SignatureTable.build(_Tensor(49), 64), "the signature tensor must hold 24 * n bytes"),
    ("merge 23 bytes", lambda: _Table().merge_signatures(b"x" * 23), "signature bytes must be a multiple of 24"),
    ("merge 23 uint8", lambda: _Table().merge_signatures(np.zeros(23, np.uint8)), "signature bytes must be a multiple of 24"),
    ("merge strided tensor", lambda: _Table().merge_signatures(_Tensor(48, False)), "the signature tensor must be contiguous"),
    ("merge 24n + 1 tensor", lambda: _Table().merge_signatures(_Tensor(49)), "the signature tensor must hold 24 * n bytes"),
    ("merge policy", lambda: _Table().merge_signatures(None, on_conflict="both"), "on_conflict must be one of keep, replace, drop"),
    ("merge map rank", lambda: _Table().merge_signatures(None, fn_map=[[1]]),
     "a map must be a one-dimensional array of integers that fit in 32 bits"),
    ("merge map 33 bits", lambda: _Table().merge_signatures(None, otu_map=[2 ** 31]),
     "a map must be a one-dimensional array of integers that fit in 32 bits"),
    ("merge map floats", lambda: _Table().merge_signatures(None, fn_map=[0.5]),
     "a map must be a one-dimensional array of integers that fit in 32 bits"),
    ("derive fn length", lambda: H.derive_signatures(SEQ, OFF, [0], [0, 0]), "fn and otu must hold one entry per protein"),
    ("derive otu 33 bits", lambda: H.derive_signatures(SEQ, OFF, [0, 0], [0, 2 ** 31]), "fn and otu must fit in 32 bits"),
    # ---- closed objects ----
    ("closed table scan", lambda: _Table(None).scan(SEQ, OFF), "SignatureTable is closed"),
    ("closed table merge", lambda: _Table(None).merge_signatures(None), "SignatureTable is closed"),
    ("closed table save", lambda: _Table(None).save("x"), "SignatureTable is closed"),
    ("closed result", lambda: _Result(2, None).regions(OFF), "ScanResult is closed"),
    ("closed result orfs", lambda: _Result(2, None).orfs(SEQ, OFF), "ScanResult is closed"),
    # ---- the steps of orfs() / select() ----
    ("select free without orfs", lambda: _Result().select(OFF, free_min_res=100), "free_min_res needs orfs=True: the free candidates are ORFs"),
    ("select coding without orfs", lambda: _Result().select(OFF, coding=True), "coding needs orfs=True: the scores are the ORFs'"),
    ("select table without orfs", lambda: _Result().select(OFF, coding=T), "coding needs orfs=True: the scores are the ORFs'"),
    ("select repair without orfs", lambda: _Result().select(OFF, repair=True), "repair needs orfs=True: it rewrites ORFs"),
    ("select starts without coding", lambda: _Result().select(OFF, SEQ, orfs=True, starts=True),
     "starts needs coding: the start-site score's coding half is the coding step's table"),
    ("orfs starts without coding", lambda: _Result().orfs(SEQ, OFF, starts=W, coding=False),
     "starts needs coding: the start-site score's coding half is the coding step's table"),
    ("orfs table", lambda: _Result().orfs(SEQ, OFF, coding=np.zeros(10, np.int32)), TABLE),
    ("select table", lambda: _Result().select(OFF, SEQ, orfs=True, coding=np.zeros((2, N.CODING_BINS), np.int32)), TABLE),
    ("orfs weights", lambda: _Result().orfs(SEQ, OFF, coding=True, starts=(np.zeros(3), np.zeros(4))), WEIGHTS),
    ("select weights", lambda: _Result().select(OFF, SEQ, orfs=True, coding=True, starts=7), WEIGHTS),
    ("choose_starts table", lambda: H.choose_starts(T[:5], NO_ORFS, SEQ, OFF), TABLE),
    ("choose_starts weights", lambda: H.choose_starts(T, NO_ORFS, SEQ, OFF, weights=(W[0], W[1], W[1])), WEIGHTS),
    ("choose_starts limits", lambda: H.choose_starts(T, NO_ORFS, SEQ, OFF, limits=[1]), "limits are int32[n], one per record"),
    ("coding_scores table", lambda: H.coding_scores(T[:5], NO_ORFS, SEQ, OFF), TABLE),
    ("coding_table coding", lambda: H.coding_table(np.zeros(5), np.zeros(N.CODING_BINS)), "coding counts are int64[%d]" % N.CODING_BINS),
    ("coding_table background", lambda: H.coding_table(np.zeros(N.CODING_BINS), np.zeros(5)), "background counts are int64[%d]" % N.CODING_BINS),
    ("start_weights chosen", lambda: H.start_weights(np.zeros((4, 4)), W[0], W[1], W[1]), "chosen counts are int64[%d][4]" % N.START_WINDOW),
    ("start_weights type_cand", lambda: H.start_weights(W[0], W[0], W[1], np.zeros(3)), "type_cand counts are int64[4]"),
    # ---- alignment ----
    ("cluster ref", lambda: H.cluster_proteins(SEQ, OFF, align={"ref": "shorter"}), "ref must be 'longer' or 'member'"),
    ("search ref", lambda: H.search_proteins(SEQ, OFF, 1, align={"ref": "shorter"}), "ref must be 'longer' or 'member'"),
    ("align 20 x 21", lambda: H.align_proteins(SEQ, OFF, [[0, 1]], matrix=np.zeros((20, 21))), "matrix must be 21 x 21 and fit int8"),
    ("align int8", lambda: H.align_proteins(SEQ, OFF, [[0, 1]], matrix=np.full((21, 21), 128)), "matrix must be 21 x 21 and fit int8"),
    ("search 20 x 21", lambda: H.search_proteins(SEQ, OFF, 1, align={"matrix": np.zeros((20, 21))}), "matrix must be 21 x 21 and fit int8"),
    ("align 33-bit pairs", lambda: H.align_proteins(SEQ, OFF, [[0, 2 ** 32]]), "pair indices must fit in 32 bits"),
    ("align negative 33-bit pairs", lambda: H.align_proteins(SEQ, OFF, [[-2 ** 31 - 1, 0]]), "pair indices must fit in 32 bits"),
    # ---- the caller-held lists ----
    ("aggregate starts", lambda: H.aggregate_hits(NO_HITS, [0, 0], 1), "container_hit_start must have n_seqs * (1 or 6) + 1 entries"),
    ("assign_calls rank", lambda: H.assign_calls(NO_CALLS, [[0, 0]]), "call_start must be int64[n_prot + 1]"),
    ("assign_calls beyond", lambda: H.assign_calls(NO_CALLS, [0, 3]), "call_start[-1] is beyond the CALL records"),
    ("assign_calls otu", lambda: H.assign_calls(NO_CALLS, [0, 0], otu=np.zeros(2, N.OTU_DTYPE)), "otu must hold one record per protein"),
    ("otu_votes starts", lambda: _votes(chs=np.zeros(3, np.int64)),
     "container_hit_start and container_call_start must be int64[n_seqs * per + 1]"),
    ("otu_votes events", lambda: _votes(ev=np.zeros(2, np.uint8)),
     "the start arrays reach beyond the records, or hit_events is not one byte per hit"),
    ("otu_votes beyond", lambda: _votes(ccs=np.full(13, 1, np.int64)),
     "the start arrays reach beyond the records, or hit_events is not one byte per hit"),
    ("compose labels", lambda: H.compose_contigs(SEQ, OFF, labels=[0]), "labels must be int32[n_seqs]"),
    ("compose model", lambda: H.compose_contigs(SEQ, OFF, model=([0], np.zeros((1, N.COMP_BINS)))),
     "model counts are int64[n_models + 1][%d], the background row last" % N.COMP_BINS),
]


@pytest.mark.parametrize("call,text", [pytest.param(c, t, id=i) for i, c, t in CASES])
def test_refused_before_the_library(call, text):
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == text


# offsets = [3] and no bytes, no sequence: only SignatureTable.scan compares the buffer with offsets[-1] (above); every other
# caller leaves an empty batch to the library
NO_SEQUENCE = [
    ("derive", lambda: H.derive_signatures(b"", [3], [], [])),
    ("align", lambda: H.align_proteins(b"", [3], [])),
    ("cluster", lambda: H.cluster_proteins(b"", [3])),
    ("cluster aligned", lambda: H.cluster_proteins(b"", [3], align={})),
    ("search", lambda: H.search_proteins(b"", [3], 0)),
    ("compose", lambda: H.compose_contigs(b"", [3])),
    ("repair_orfs", lambda: H.repair_orfs(NO_CALLS, b"", [3])),
    ("choose_starts", lambda: H.choose_starts(T, NO_ORFS, b"", [3])),
    ("coding_counts", lambda: H.coding_counts(NO_ORFS, b"", [3])),
    ("coding_scores", lambda: H.coding_scores(T, NO_ORFS, b"", [3])),
    ("free_orfs", lambda: H.free_orfs(b"", [3])),
    ("orf_regions", lambda: H.orf_regions(np.zeros(0, N.REGION_DTYPE), b"", [3])),
]


@pytest.mark.parametrize("call", [pytest.param(c, id=i) for i, c in NO_SEQUENCE])
def test_no_sequence_is_left_to_the_library(call):
    with pytest.raises(_LibraryUsed):
        call()


def test_well_formed_arguments_reach_the_library():
    """The stubs and the good arguments of the cases above are good: each call gets as far as the library."""
    for call in (lambda: _Table().scan(SEQ, OFF), lambda: _Table().merge_signatures(None, fn_map=[1], otu_map=[]),
                 lambda: _Table().merge_signatures(_Tensor(48)), lambda: H.SignatureTable.build(_Tensor(48), 64),
                 lambda: H.SignatureTable.build(b"x" * 48, 64), lambda: _Result().regions(OFF), lambda: _Result().otu_votes(OFF),
                 lambda: _Result().orfs(SEQ, OFF, coding=T, starts=W), lambda: _Result().select(OFF),
                 lambda: _Result().select(OFF, SEQ, orfs=True, free_min_res=100, coding=True, starts=True, repair=True),
                 lambda: H.derive_signatures(SEQ, OFF, [0, 0], [0, 0]), lambda: H.align_proteins(SEQ, OFF, [[0, 1]], matrix=np.zeros((21, 21))),
                 lambda: H.cluster_proteins(SEQ, OFF, align={"ref": "member"}), lambda: H.search_proteins(SEQ, OFF, 1),
                 lambda: _votes(), lambda: H.assign_calls(NO_CALLS, [0, 0]), lambda: H.aggregate_hits(NO_HITS, np.zeros(7, np.int64), 1),
                 lambda: H.compose_contigs(SEQ, OFF, labels=[0, -1], model=([0], np.zeros((2, N.COMP_BINS)))),
                 lambda: H.choose_starts(T, NO_ORFS, SEQ, OFF, weights=W, limits=[]), lambda: H.coding_table(np.zeros(N.CODING_BINS), np.zeros(N.CODING_BINS)),
                 lambda: H.start_weights(W[0], W[0], W[1], W[1])):
        with pytest.raises(_LibraryUsed):
            call()
