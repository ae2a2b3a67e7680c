"""The ops of kg_proteins_align_ops and of the search calls with KG_TRACE_OPS / KG_TRACE_OPS_EQX on the GPU against
tests/ops_model.py: ops and op_start byte for byte (include/kmerguts_hip.h states the rule).  The shapes follow the constants of
kg_trace.hpp and kg_ops.hpp: the 64-row stripe, 16 columns to a staging word, the 1024 columns one wave stores at a time, and the
64 columns the fill kernel reads at a time."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import align_model as A
import cluster_model as M
import ops_model as O
import search_model as S
import trace_model as T
from test_gpu_trace import _relatives        # planted relatives with indels, as the paths tests make them
from kmergutsjava_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "kmergutsjava_amd", "csrc")
_DEV = open(os.path.join(_CSRC, "kg_trace.hpp")).read()
COLS_PER_WORD = int(re.search(r"constexpr int kTraceColsPerWord = (\d+);", _DEV).group(1))
M23 = np.full((21, 21), -3, dtype=np.int64)
np.fill_diagonal(M23, 2)
M23[20, 20] = -3


def test_the_constants():
    assert COLS_PER_WORD == 16 and N.OPS_MODES == {"m": 4, "eqx": 8}


def _ops(prots, pairs, mode, **kw):
    from kmergutsjava_amd import hotpath
    seq, off = M.pack(prots)
    return hotpath.align_proteins(seq, off, pairs, paths=True, ops=mode, **kw)


def _same(prots, pairs, matrix=None, gap_open=11, gap_extend=1, max_cells=N.ALIGN_DEFAULT_MAX_CELLS, max_trace_cells=N.TRACE_DEFAULT_MAX_CELLS,
          modes=O.MODES):
    """The device's records, op_start and ops == the model's, in both modes.  -> {mode: (path records, op_start, ops)}"""
    seq, off = M.pack(prots)
    Smat = A.S62 if matrix is None else np.asarray(matrix)
    aln = A.align_model(seq, off, pairs, Smat, gap_open, gap_extend, max_cells)
    out = {}
    for mode in modes:
        wpth, wstart, wops = O.ops_model(seq, off, pairs, aln, mode, Smat, gap_open, gap_extend, max_trace_cells)
        got, pth, start, ops = _ops(prots, pairs, mode, matrix=matrix, gap_open=gap_open, gap_extend=gap_extend, max_cells=max_cells,
                                    max_trace_cells=max_trace_cells)
        assert got.tobytes() == aln.tobytes() and pth.tobytes() == wpth.tobytes()
        assert start.dtype == np.int64 and ops.dtype == np.uint32
        bad = np.flatnonzero(start != wstart)
        assert start.tobytes() == wstart.tobytes(), (mode, bad[:5], start[bad[:5]], wstart[bad[:5]])
        assert ops.tobytes() == wops.tobytes(), (mode, np.flatnonzero(ops != wops)[:5])
        out[mode] = (pth, start, ops)
    return out


def _cigars(start, ops):
    from kmergutsjava_amd import hotpath
    return [hotpath.cigar(ops[start[k]:start[k + 1]]) for k in range(len(start) - 1)]


def _columns(aln, pth):
    return (aln["end_a"].astype(np.int64) - pth["start_a"] + 1) + pth["gap_cols_a"]


# ---- 1: borders ----------------------------------------------------------------------------------------------------------------

def test_every_box_of_70_by_80_of_a_pair_with_two_indels():
    """The prefixes of one protein against the prefixes of a relative with two planted indels: one pair of tables holds every
    box's, a path depends only on its end cell.  The boxes' walks have 1 to well over 64 columns: 15, 16, 17 (the staging word)
    and 63, 64, 65 (the fill kernel's chunk) among them, rows on both sides of the 64-row stripe."""
    rng = np.random.default_rng(61)
    a = M.random_protein(rng, 70)
    b = (A.mutate(rng, a[:22], 0.1) + M.random_protein(rng, 4) + A.mutate(rng, a[22:45], 0.1) + A.mutate(rng, a[48:], 0.1) + M.random_protein(rng, 20))[:80]
    assert len(b) == 80
    prots = [a[:n] for n in range(1, 71)] + [b[:m] for m in range(1, 81)]
    boxes = [(n, m) for n in range(1, 71) for m in range(1, 81)]
    pairs = np.array([(n - 1, 70 + m - 1) for n, m in boxes])
    ca, cb = T._codes(a), T._codes(b)
    H, E, F = T.tables_numpy(ca, cb, A.S62, 11, 1)
    Hn = np.asarray(H)
    H, E, F = Hn.tolist(), np.asarray(E).tolist(), np.asarray(F).tolist()
    memo, want = {}, {mode: ([0], []) for mode in O.MODES}
    n_cols = []
    for n, m in boxes:
        box = Hn[1:n + 1, 1:m + 1]
        i, j = divmod(int(np.argmax(box)), m)           # row-major: the smallest i, then the smallest j
        if box[i, j] > 0:
            if (i, j) not in memo:
                rec, cols = T.walk(H, E, F, ca, cb, A.S62, 11, 1, i, j)
                memo[(i, j)] = (len(cols),) + tuple(O.encode(O.kinds_of(a, b, rec, cols, mode)) for mode in O.MODES)
            n_cols.append(memo[(i, j)][0])
        for k, mode in enumerate(O.MODES):
            if box[i, j] > 0:
                want[mode][1].extend(memo[(i, j)][1 + k])
            want[mode][0].append(len(want[mode][1]))
    assert {15, 16, 17, 63, 64, 65} <= set(n_cols) and max(n_cols) > 70 and len(memo) >= 40
    for mode in O.MODES:
        got, pth, start, ops = _ops(prots, pairs, mode)
        wstart, wops = np.asarray(want[mode][0], dtype=np.int64), np.asarray(want[mode][1], dtype=np.uint32)
        bad = np.flatnonzero(start != wstart)
        assert start.tobytes() == wstart.tobytes(), (mode, bad[:5], pairs[bad[:5] - 1])
        assert ops.tobytes() == wops.tobytes(), (mode, np.flatnonzero(ops != wops)[:5])
        assert (_columns(got, pth)[pth["status"] == 0] == np.asarray(n_cols)).all()
    assert sum(1 for x in want["m"][1] if x & 15 in (N.OP_I, N.OP_D)) > 1000


def test_alignments_of_127_128_and_129_columns():
    rng = np.random.default_rng(62)
    p = M.random_protein(rng, 129).replace(b"W", b"A")
    prots = [p[:127], p[:128], p, p[:60] + p[61:], p[:60] + p[62:130], p[:50] + b"WW" + p[50:127]]
    pairs = [(0, 0), (1, 1), (2, 2), (2, 3), (4, 1), (0, 5), (5, 0)]
    got = _same(prots, pairs)
    seq, off = M.pack(prots)
    aln = A.align_model(seq, off, pairs)
    assert _columns(aln, got["m"][0]).tolist() == [127, 128, 129, 129, 128, 129, 129]
    assert _cigars(*got["m"][1:])[:3] == ["127M", "128M", "129M"] and _cigars(*got["eqx"][1:])[:3] == ["127=", "128=", "129="]


# ---- 2: runs across chunks -------------------------------------------------------------------------------------------------------

def test_runs_across_the_chunks_of_the_fill_kernel_and_the_blocks_of_the_walk():
    rng = np.random.default_rng(63)
    p = M.random_protein(rng, 200).replace(b"W", b"A")
    h100 = p[:80] + b"W" * 100 + p[80:]                  # W against anything but W, Y, F is negative: the insert is a gap
    v130 = p[:40] + b"W" * 130 + p[40:]
    subs = []
    for k in (62, 63, 64, 65, 127, 128):                # a run of '=' that ends exactly on column k - 1, an 'X' in column k
        x = bytearray(p[:140])
        x[k] = ord("W")
        subs.append(bytes(x))
    long_p = M.random_protein(rng, 1100)                 # more than the 1024 columns a wave stores at a time
    long_x = bytearray(long_p)
    long_x[1023], long_x[1024] = (ord("A") if long_x[1023] == ord("W") else ord("W")), (ord("A") if long_x[1024] == ord("W") else ord("W"))
    prots = [p, h100, v130, p[:140]] + subs + [b"W", long_p, bytes(long_x), long_p[:1024], long_p[:1025]]
    n = len(prots)
    pairs = [(0, 0), (0, 1), (1, 0), (2, 0), (0, 2)] + [(3, 4 + k) for k in range(6)] + [(10, 10), (11, 11), (11, 12), (13, 13), (14, 14), (13, 12)]
    assert n == 15
    got = _same(prots, pairs)
    cm, cx = _cigars(*got["m"][1:]), _cigars(*got["eqx"][1:])
    assert cm[:5] == ["200M", "80M100D120M", "80M100I120M", "40M130I160M", "40M130D160M"]
    assert cx[:5] == ["200=", "80=100D120=", "80=100I120=", "40=130I160=", "40=130D160="]
    assert cx[5:11] == ["%d=1X%d=" % (k, 139 - k) for k in (62, 63, 64, 65, 127, 128)] and cm[5:11] == ["140M"] * 6
    assert cm[11] == "1M" and cx[11] == "1=" and got["eqx"][2][got["eqx"][1][11]] == (1 << 4 | N.OP_EQ)
    # (the last pair's alignment stops in front of the two substitutions: exactly 1023 columns, one short of a full block)
    assert cx[12:] == ["1100=", "1023=2X75=", "1024=", "1025=", "1023="] and cm[12:] == ["1100M", "1100M", "1024M", "1025M", "1023M"]


# ---- 3: every lane a run start ---------------------------------------------------------------------------------------------------

def test_every_lane_a_run_start():
    """a = AC x 70 against b = AW x 70: A-A scores 4 and C-W -2, so the one local alignment is the whole diagonal and its columns
    alternate '=' and 'X': 140 ops of one column each in the =/X mode, one op in the M mode."""
    a, b = b"AC" * 70, b"AW" * 70
    end, rec, ops = O.ops_of(a, b, mode="eqx")
    assert ops == [1 << 4 | (N.OP_EQ if k % 2 == 0 else N.OP_X) for k in range(139)] and rec[:2] == (0, 0) and end[1:] == (138, 138)
    # (the last column, C against W, is not on a local alignment: 139 columns)
    assert O.ops_of(a, b, mode="m")[2] == [139 << 4]
    got = _same([a, b, a + a, b + b], [(0, 1), (1, 0), (2, 3), (0, 0)])
    assert got["eqx"][1].tolist() == [0, 139, 278, 278 + 279, 278 + 279 + 1] and got["m"][1].tolist() == [0, 1, 2, 3, 4]
    assert got["eqx"][2][:139].tolist() == ops


# ---- 4: gap_open = 0 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,gap_extend", [(M23, 1), (None, 1), (M23, 2)])
def test_three_letter_relatives_under_gap_open_0(matrix, gap_extend):
    rng = np.random.default_rng(64)
    prots = []
    for _ in range(6):
        base = bytes(rng.choice(np.frombuffer(b"ACD", dtype=np.uint8), size=int(rng.integers(100, 151))))
        cut = int(rng.integers(10, 80))
        prots += [base, base[:cut] + base[cut + int(rng.integers(1, 6)):], A.mutate(rng, base, 0.1)[int(rng.integers(0, 9)):]]
    pairs = [(3 * k + x, 3 * k + y) for k in range(6) for x, y in ((0, 1), (1, 0), (0, 2), (2, 1))]
    got = _same(prots, pairs, matrix=matrix, gap_open=0, gap_extend=gap_extend)
    kinds = (got["m"][2] & 15).tolist()
    beside = sum(1 for x, y in zip(kinds, kinds[1:]) if {x, y} == {N.OP_I, N.OP_D})
    assert beside >= (3 if matrix is M23 and gap_extend == 1 else 0), beside      # an I run directly beside a D run


# ---- 5: order and geometry -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed_pairs():
    """300 pairs: relatives with indels of 20 to 90 residues, pieces of them, pairs that score 0, pairs over max_cells (status 1)
    and, under the lowered max_trace_cells the test passes, boxes over the cap (status 2)."""
    rng = np.random.default_rng(65)
    base = M.random_protein(rng, 90)
    rel = []
    for _ in range(12):
        p = A.mutate(rng, base, 0.12)[int(rng.integers(0, 6)):]
        cut = int(rng.integers(10, 60))
        rel.append(p[:cut] + p[cut + int(rng.integers(0, 5)):])
    prots = rel + [p[int(rng.integers(0, 6)):][:int(rng.integers(20, 40))] for p in rel] + [b"XXXX", b"", M.random_protein(rng, 120)]
    pairs = np.concatenate([rng.integers(0, 24, size=(240, 2)), np.stack([rng.integers(0, 27, size=60), rng.integers(24, 27, size=60)], axis=1)])
    pairs = pairs[rng.permutation(len(pairs))]
    return prots, pairs


def test_forward_reversed_and_shuffled(mixed_pairs):
    prots, pairs = mixed_pairs
    seq, off = M.pack(prots)
    max_cells = 100 * 100                               # the 120-residue protein against itself is skipped: status 1
    aln = A.align_model(seq, off, pairs, A.S62, 11, 1, max_cells)
    box = np.where(aln["score"] > 0, (aln["end_a"].astype(np.int64) + 1) * (aln["end_b"].astype(np.int64) + 1), 0)
    cap = int(np.sort(box[box > 0])[int(0.8 * (box > 0).sum())]) - 1          # one cell under a box that occurs: that box is untraced
    assert (box == cap + 1).any()
    first = _same(prots, pairs, max_cells=max_cells, max_trace_cells=cap)
    status = first["m"][0]["status"]
    assert (status == N.PATH_UNTRACED).sum() >= 20 and (status == N.PATH_NONE).sum() >= 20 and (aln["status"] == 1).any() and (aln["score"] == 0).any()
    assert ((status == N.PATH_UNTRACED) == (box > cap)).all()
    perm = np.random.default_rng(66).permutation(len(pairs))
    for mode in O.MODES:
        pth, start, ops = first[mode]
        flat = start[1:] == start[:-1]
        assert (flat == (status != N.PATH_TRACED)).all()                      # flat across the records without a path, and only there
        mine = [ops[start[k]:start[k + 1]].tobytes() for k in range(len(pairs))]
        for order in (np.arange(len(pairs))[::-1], perm):
            _, p2, s2, o2 = _ops(prots, pairs[order], mode, max_cells=max_cells, max_trace_cells=cap)
            assert p2.tobytes() == pth[order].tobytes()
            assert [o2[s2[k]:s2[k + 1]].tobytes() for k in range(len(order))] == [mine[k] for k in order]
            assert s2[-1] == start[-1] == len(o2)


def test_a_3000_by_3000_pair_among_a_thousand_short_ones(mixed_pairs):
    """The long launch (b over the LDS carry, direction words over the short slab) and the wide launch both stage."""
    rng = np.random.default_rng(67)
    long_a = M.random_protein(rng, 3000)
    long_b = A.mutate(rng, long_a[:1400] + long_a[1420:] + M.random_protein(rng, 20), 0.2)
    assert len(long_b) == 3000 > N.ALIGN_LDS_COLS
    prots, pairs = mixed_pairs
    n = len(prots)
    short = pairs[np.random.default_rng(68).integers(0, len(pairs), size=1000)]
    mixed = np.concatenate([short[:417], [(n, n + 1)], short[417:]])
    got = _same(prots + [long_a, long_b], mixed)
    for mode in O.MODES:
        pth, start, ops = got[mode]
        mine = ops[start[417]:start[418]]
        assert pth["status"][417] == 0 and ((mine & 15) == N.OP_I).any() and int((mine >> 4).sum()) > 2900 > 1024
    assert len(got["eqx"][2]) > len(got["m"][2]) > 1000


# ---- 6: unchanged outputs --------------------------------------------------------------------------------------------------------------

def _search(seq, off, n_db, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.search_proteins(seq, off, n_db, **kw)


def test_everything_but_the_ops_is_the_paths_calls(mixed_pairs):
    from kmergutsjava_amd import hotpath
    prots, pairs = mixed_pairs
    seq, off = M.pack(prots)
    aln, pth = hotpath.align_proteins(seq, off, pairs, paths=True, max_trace_cells=3000)
    for mode in O.MODES:
        a2, p2, start, ops = hotpath.align_proteins(seq, off, pairs, paths=True, ops=mode, max_trace_cells=3000)
        assert a2.tobytes() == aln.tobytes() and p2.tobytes() == pth.tobytes() and len(start) == len(pairs) + 1
    sseq, soff = S.batch(_relatives(np.random.default_rng(69)))
    for trace in ("hits", "all"):
        hits, hstart, recs, st = _search(sseq, soff, 16, paths=trace)
        for mode in O.MODES:
            h2, s2, r2, st2, op_start, ops = _search(sseq, soff, 16, paths=trace, ops=mode)
            assert h2.tobytes() == hits.tobytes() and s2.tobytes() == hstart.tobytes() and r2.tobytes() == recs.tobytes()
            keys = [k for k in st if not k.startswith("ms_")]
            assert {k: st2[k] for k in keys} == {k: st[k] for k in keys} and set(st2) == set(st) | {"ops", "ms_ops"}
            assert st2["ops"] == len(ops) == op_start[-1] and 0 <= st2["ms_ops"] <= st2["ms_trace"]
    # no pairs, no records: op_start is [0]
    a2, p2, start, ops = hotpath.align_proteins(b"", np.zeros(1, dtype=np.int64), np.zeros((0, 2), dtype=np.int32), paths=True, ops="m")
    assert len(a2) == 0 and start.tolist() == [0] and len(ops) == 0
    got = _search(b"ACDEFGHIKLMN", np.array([0, 12]), 1, paths="all", ops="eqx")
    assert len(got[0]) == 0 and got[4].tolist() == [0] and len(got[5]) == 0


# ---- 7: errors and allocations -------------------------------------------------------------------------------------------------------

def _error():
    return N.load().kg_last_error().decode()


def _raw_search(seq, off, n_db, trace, cap=1 << 24):
    lib = N.load()
    h = C.c_void_p()
    arr = np.frombuffer(bytes(seq), dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    p, a = N.KgSearchParams(2, 8, 256, 0), N.KgAlignParams(50, 0, 11, 1, 1 << 26, None, 0)
    rc = lib.kg_proteins_search_paths(0, C.byref(p), C.byref(a), arr.ctypes.data, off.ctypes.data, len(off) - 1, n_db, 0, 0, trace, cap, C.byref(h))
    return rc, lib.kg_last_error().decode(), h


def test_every_error_of_the_modes_and_of_the_getters():
    lib = N.load()
    seq, off = S.batch([b"ACDEFGHIKLMN", b"ACDEFGHIKLMN"])
    own = "trace takes at most one of KG_TRACE_OPS and KG_TRACE_OPS_EQX"
    for trace, words in [(N.TRACE_HITS | 12, own), (N.TRACE_ALL | 12, own), (N.TRACE_HITS | 16, own), (N.TRACE_ALL | 4 | 32, own), (N.TRACE_HITS | 1 << 20, own),
                         (4, "trace must be KG_TRACE_HITS or KG_TRACE_ALL"), (8, "trace must be KG_TRACE_HITS or KG_TRACE_ALL"),
                         (3 | 4, "trace must be KG_TRACE_HITS or KG_TRACE_ALL"), (0, "trace must be KG_TRACE_HITS or KG_TRACE_ALL"),
                         (12, "trace must be KG_TRACE_HITS or KG_TRACE_ALL")]:
        rc, msg, h = _raw_search(seq, off, 1, trace)
        assert rc == N.KG_ERR_ARG and msg.startswith(words) and not h.value, (trace, rc, msg)
    # a set made without ops
    rc, msg, h = _raw_search(seq, off, 1, N.TRACE_ALL)
    assert rc == 0
    try:
        d64, d32, ms = np.zeros(2, dtype=np.int64), np.zeros(1, dtype=np.uint32), C.c_float()
        assert lib.kg_hitset_ops_count(h) == 0
        assert lib.kg_hitset_op_starts_copy(h, 0, 1, d64.ctypes.data) == N.KG_ERR_ARG and _error().startswith("kg_hitset_op_starts_copy: the set was made without ops")
        assert lib.kg_hitset_ops_copy(h, 0, 1, d32.ctypes.data) == N.KG_ERR_ARG and _error().startswith("kg_hitset_ops_copy: the set was made without ops")
        assert lib.kg_hitset_ms_ops(h, C.byref(ms)) == N.KG_ERR_ARG and _error().startswith("kg_hitset_ms_ops: the set was made without ops")
    finally:
        lib.kg_hitset_free(h)
    # a set made with them: the ranges
    rc, msg, h = _raw_search(seq, off, 1, N.TRACE_ALL | N.TRACE_OPS_EQX)
    assert rc == 0, msg
    try:
        assert lib.kg_hitset_ops_count(h) == 1 and lib.kg_hitset_count(h) == 1
        assert lib.kg_hitset_op_starts_copy(h, 0, 1, d64.ctypes.data) == 0 and d64.tolist() == [0, 1]
        assert lib.kg_hitset_op_starts_copy(h, 1, 0, d64.ctypes.data) == 0 and d64[0] == 1
        assert lib.kg_hitset_ops_copy(h, 0, 1, d32.ctypes.data) == 0 and d32[0] == (12 << 4 | N.OP_EQ)
        assert lib.kg_hitset_ms_ops(h, C.byref(ms)) == 0 and ms.value >= 0
        for call, words in [(lambda: lib.kg_hitset_op_starts_copy(h, 1, 1, d64.ctypes.data), "kg_hitset_op_starts_copy: range outside the set"),
                            (lambda: lib.kg_hitset_op_starts_copy(h, -1, 1, d64.ctypes.data), "kg_hitset_op_starts_copy: range outside the set"),
                            (lambda: lib.kg_hitset_ops_copy(h, 1, 1, d32.ctypes.data), "kg_hitset_ops_copy: range outside the set"),
                            (lambda: lib.kg_hitset_ops_copy(h, 0, 1, None), "null argument"),
                            (lambda: lib.kg_hitset_op_starts_copy(h, 0, 0, None), "null argument")]:
            assert call() == N.KG_ERR_ARG and _error().startswith(words), (words, _error())
    finally:
        lib.kg_hitset_free(h)
    assert lib.kg_hitset_ops_copy(None, 0, 0, None) == N.KG_ERR_ARG and lib.kg_opset_ops_copy(None, 0, 0, None) == N.KG_ERR_ARG
    assert lib.kg_opset_ops_count(None) == 0 and lib.kg_opset_ms_ops(None, None) == N.KG_ERR_ARG
    lib.kg_opset_free(None)
    # the align call: its mode and its set
    offs = np.array([0, 5, 10], dtype=np.int64)
    buf, pr = np.frombuffer(b"ACDEFACDEF", dtype=np.uint8), np.array([0, 1], dtype=np.int32)
    res, pth = np.zeros(1, dtype=N.ALIGNMENT_DTYPE), np.zeros(1, dtype=N.ALIGN_PATH_DTYPE)
    prm = N.KgAlignParams(50, 0, 11, 1, 1 << 26, None, 0)
    for mode, ops_arg, words in [(0, True, "ops_mode must be KG_TRACE_OPS or KG_TRACE_OPS_EQX"), (12, True, "ops_mode must be"), (1, True, "ops_mode must be"),
                                 (4, False, "null argument")]:
        h = C.c_void_p(7)
        rc = lib.kg_proteins_align_ops(0, C.byref(prm), buf.ctypes.data, offs.ctypes.data, 2, pr.ctypes.data, 1, 1 << 24, mode, res.ctypes.data,
                                       pth.ctypes.data, C.byref(h) if ops_arg else None)
        assert rc == N.KG_ERR_ARG and _error().startswith(words) and (not ops_arg or not h.value), (mode, _error())
    h = C.c_void_p()
    assert lib.kg_proteins_align_ops(0, C.byref(prm), buf.ctypes.data, offs.ctypes.data, 2, pr.ctypes.data, 1, 0, 4, res.ctypes.data, pth.ctypes.data,
                                     C.byref(h)) == N.KG_ERR_ARG and _error().startswith("max_trace_cells must be >= 1") and not h.value
    assert lib.kg_proteins_align_ops(0, C.byref(prm), buf.ctypes.data, offs.ctypes.data, 2, pr.ctypes.data, 1, 1 << 24, 8, res.ctypes.data,
                                     pth.ctypes.data, C.byref(h)) == 0
    try:
        assert lib.kg_opset_ops_count(h) == 1 and lib.kg_opset_op_starts_copy(h, 0, 1, d64.ctypes.data) == 0 and d64.tolist() == [0, 1]
        assert lib.kg_opset_ops_copy(h, 0, 1, d32.ctypes.data) == 0 and d32[0] == (5 << 4 | N.OP_EQ)
        assert lib.kg_opset_op_starts_copy(h, 0, 2, d64.ctypes.data) == N.KG_ERR_ARG and _error().startswith("kg_opset_op_starts_copy: range outside the set")
        assert lib.kg_opset_ops_copy(h, 0, 2, d32.ctypes.data) == N.KG_ERR_ARG and _error().startswith("kg_opset_ops_copy: range outside the set")
    finally:
        lib.kg_opset_free(h)


def test_failed_allocations_and_the_staging_limit_leave_nothing_behind(monkeypatch, mixed_pairs):
    import torch
    from kmergutsjava_amd import hotpath, synth
    prots, pairs = mixed_pairs
    prots = prots + [M.random_protein(np.random.default_rng(70), N.ALIGN_LDS_COLS + 1)]          # the carry of the second launch too
    pairs = np.concatenate([pairs[:50], [(len(prots) - 1, len(prots) - 1)]])
    seq, off = M.pack(prots)
    rec = synth.high_density_config(4, 100, 4001, 500, dna=False)[2]
    sseq, soff = S.batch(_relatives(np.random.default_rng(71)))
    with hotpath.SignatureTable.from_bytes(synth.table_image(rec), 0) as tab:
        first = hotpath.align_proteins(seq, off, pairs, paths=True, ops="eqx")
        sfirst = _search(sseq, soff, 16, paths="all", ops="m")
        counts = []
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        for call in (lambda: hotpath.align_proteins(seq, off, pairs, paths=True), lambda: hotpath.align_proteins(seq, off, pairs, paths=True, ops="eqx"),
                     lambda: _search(sseq, soff, 16, paths="all"), lambda: _search(sseq, soff, 16, paths="all", ops="m")):
            failed = 0
            for n in range(1, 700):
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
            counts.append(failed)
            del got
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0
        # the ops' own allocations: the arguments, the records, the staging, the counts, their scan, its partials and total, the block
        assert counts[1] == counts[0] + 8 and counts[3] == counts[2] + 8, counts
        again = hotpath.align_proteins(seq, off, pairs, paths=True, ops="eqx")
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
        # the staging limit, lowered by the test hook: the call names the bytes it needs and leaves nothing behind
        aln = first[0]
        traced = first[1]["status"] == 0
        need = 4 * int((-(-(aln["end_a"][traced].astype(np.int64) + aln["end_b"][traced] + 1) // COLS_PER_WORD)).sum())
        for limit, fits in ((need, True), (need - 1, False), (4, False)):
            monkeypatch.setenv("KG_TEST_OPS_STAGE_BYTES", str(limit))
            if fits:
                assert hotpath.align_proteins(seq, off, pairs, paths=True, ops="eqx")[3].tobytes() == first[3].tobytes()
                continue
            with pytest.raises(N.KmerGutsNativeError) as e:
                hotpath.align_proteins(seq, off, pairs, paths=True, ops="eqx")
            assert e.value.code == N.KG_ERR_LIMIT and "need %d bytes of staging" % need in str(e.value), e.value
            assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0
        with pytest.raises(N.KmerGutsNativeError) as e:
            _search(sseq, soff, 16, paths="all", ops="m")
        assert e.value.code == N.KG_ERR_LIMIT and "bytes of staging" in str(e.value)
        assert hotpath.align_proteins(seq, off, pairs, paths=True)[1].tobytes() == first[1].tobytes()      # the plain call stages nothing
        monkeypatch.delenv("KG_TEST_OPS_STAGE_BYTES")
        assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0
        assert _search(sseq, soff, 16, paths="all", ops="m")[5].tobytes() == sfirst[5].tobytes()


# ---- 8: search ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(24))
def test_random_batches_through_the_exact_and_the_seeded_entry_points(seed):
    """Planted relatives with indels, both trace modes and both op modes; the seeded entry point with the identity alphabet and
    the solid shape of eight, whose results are the exact call's (tests/test_gpu_seeded_search.py)."""
    rng = np.random.default_rng(300 + seed)
    prots = _relatives(rng)
    n_db = int(rng.integers(0, len(prots) + 1)) if seed % 6 else len(prots) // 2
    align = dict(min_ratio_pct=int(rng.choice([0, 30, 50, 100])), ref=str(rng.choice(["longer", "member"])),
                 max_cells=int(rng.choice([2000, 1 << 26])), gap_open=int(rng.choice([11, 0, 5])))
    kw = dict(min_shared=int(rng.integers(1, 4)), max_cand=int(rng.choice([1, 2, 3, 8, 64])), max_db_per_kmer=int(rng.choice([1, 2, 4, 256])))
    cap = int(rng.choice([1 << 24, 1500]))
    seq, off = S.batch(prots)
    searched = S.search_model(seq, off, n_db, **kw, **align)
    solid = dict(alphabet="identity", shapes=["11111111"])
    for trace in ("hits", "all"):
        for mode in O.MODES:
            whits, wstart, wpth, wop_start, wops = O.search_ops_model(seq, off, n_db, mode, trace, cap, searched=searched, **kw, **align)
            for more in ({}, dict(seeds=solid)):
                hits, start, pth, st, op_start, ops = _search(seq, off, n_db, align=align, paths=trace, ops=mode, max_trace_cells=cap, **kw, **more)
                assert hits.tobytes() == whits.tobytes() and start.tobytes() == wstart.tobytes() and pth.tobytes() == wpth.tobytes()
                assert op_start.tobytes() == wop_start.tobytes(), (trace, mode, more)
                assert ops.tobytes() == wops.tobytes(), (trace, mode, more)
                assert st["ops"] == len(wops)


# ---- 9: end to end -------------------------------------------------------------------------------------------------------------------

def _parse_alignments(text: str):
    """{(query id, target id): (header fields, the query row, the target row)} of an --alignments file."""
    out, key = {}, None
    for line in text.splitlines():
        if line.startswith(">"):
            f = line[1:].split()
            key = (f[0], f[1])
            out[key] = [dict(x.split("=") for x in f[2:]), "", "", None, None]
        elif line.startswith("Query ") or line.startswith("Target"):
            f = line.split()
            which = 1 if f[0] == "Query" else 2
            out[key][which] += f[2]
            if out[key][2 + which] is None:
                out[key][2 + which] = int(f[1])
    return out


def _ops_of_rows(qrow: str, trow: str) -> str:
    from kmergutsjava_amd import hotpath
    kinds = "".join("D" if x == "-" else "I" if y == "-" else "M" for x, y in zip(qrow, trow))
    return hotpath.cigar(O.encode(kinds))


def test_end_to_end_with_cigars_and_alignments(tmp_path):
    """The golden E. coli proteome as the database; 192 of its proteins as queries with a substitution at every 12th residue, and
    in every fourth of them three residues of the middle deleted (tests/test_gpu_trace.py's recipe); search_proteins --paths
    --cigar --alignments as a subprocess."""
    from kmergutsjava_amd import hotpath
    from kmergutsjava_amd.make_signatures import _read, parse_fasta
    faa = os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz")
    ids, seqs = parse_fasta(_read(faa), faa)
    pick = [k for k in range(0, len(ids), len(ids) // 260) if 60 <= len(seqs[k]) <= 700][:192]
    assert len(pick) == 192
    alpha = A.ALPHA
    queries, planted = [], {}
    for n, k in enumerate(pick):
        p = seqs[k]
        q = bytes(alpha[(alpha.index(ch) + 3) % 20] if i % 12 == 6 and ch in alpha else ch for i, ch in enumerate(p))
        deleted = n % 4 == 0
        if deleted:
            q = q[:len(q) // 2] + q[len(q) // 2 + 3:]
        queries.append(q)
        planted[b"m_" + ids[k]] = (p, q, deleted)
    (tmp_path / "q.faa").write_bytes(b"".join(b">m_%s\n%s\n" % (ids[k], q) for k, q in zip(pick, queries)))
    out, al = tmp_path / "hits.tsv", tmp_path / "al.txt"
    r = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.search_proteins", "-d", faa, "-q", str(tmp_path / "q.faa"), "-o", str(out),
                        "--paths", "--cigar", "--alignments", str(al)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = r.stderr.strip().splitlines()[-1]
    m = re.search(r"hits: (\d+), queries hit: (\d+), .*, traced: (\d+), untraced: 0, trace ms: [0-9.]+, ops: (\d+)$", line)
    assert m, line
    hits, q_hit, traced, n_ops = map(int, m.groups())
    rows = [x.split(b"\t") for x in out.read_bytes().splitlines()]
    # every hit record is traced and has ops; the rank-0 ones are written
    assert traced == hits >= q_hit == len(rows) >= 0.9 * len(pick) and all(len(x) == 21 and x[20] != b"-" for x in rows)
    assert n_ops >= sum(len(re.findall(rb"\d+[MID]", x[20])) for x in rows) >= len(rows) and n_ops >= traced
    blocks = _parse_alignments(al.read_text())
    assert len(blocks) == len(rows)
    seq_of = dict(zip(ids, seqs))
    own = with_gap = 0
    for x in rows:
        p, q, deleted = planted[x[0]]
        head, qrow, trow, qfirst, tfirst = blocks[(x[0].decode(), x[2].decode())]
        cig = x[20].decode()
        # the alignment file parses back to the same ops, and its residues are the proteins'
        assert _ops_of_rows(qrow, trow) == cig and (qfirst, tfirst) == (int(x[10]), int(x[11])), x
        assert qrow.replace("-", "").encode() == q[qfirst - 1:int(x[7])] and trow.replace("-", "").encode() == seq_of[x[2]][tfirst - 1:int(x[8])]
        assert int(head["score"]) == int(x[4]) and int(head["columns"]) == len(qrow) == int(x[12]) and head["identity"] == x[14].decode() + "%"
        if seq_of[x[2]] != p:
            continue
        own += 1
        end, rec, ops = O.ops_of(q, p, mode="m")
        assert cig == hotpath.cigar(ops), (x, hotpath.cigar(ops))
        gaps = re.findall(r"(\d+)([ID])", cig)
        # a planted deletion is exactly one op, 3D (the original's three residues face nothing), at the planted place: taking
        # the three residues it faces out of the original gives the original without the planted three, except where the query's
        # residue is a substituted one (a substitution beside the deletion matches neither neighbour: the gap may sit on either side)
        assert (gaps == [("3", "D")]) == deleted and (deleted or gaps == []), (x, cig)
        if deleted:
            with_gap += 1
            at = rec[1] + sum(int(n) for n, c in re.findall(r"(\d+)([MID])", cig.split("3D")[0]) if c != "I")
            h = len(p) // 2
            assert abs(at - h) <= 3 and all(u == v or w != v for u, v, w in zip(p[:at] + p[at + 3:], p[:h] + p[h + 3:], q)), (x, at, h)
    assert own >= 0.9 * len(pick) and with_gap >= 40
