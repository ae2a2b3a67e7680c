"""kg_proteins_align on the device against tests/align_model.py, byte for byte (include/kmerguts_hip.h states the rule).  The
shapes are the smallest at which a wave that walks 64-row stripes can go wrong: lengths around the stripe, the best cell and
gaps on and across stripe borders, a restart behind a border, the long-centre carry, and the order the pairs are handed out in."""
import ctypes as C

import numpy as np
import pytest

import align_model as A
import cluster_model as M
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import align_scores as AS

pytestmark = pytest.mark.gpu
STRIPE = 64                     # kg_align.hpp: the rows of one stripe = the lanes of a wave


def _align(prots, pairs, **kw):
    from kmergutsjava_amd import hotpath
    seq, off = M.pack(prots)
    return hotpath.align_proteins(seq, off, pairs, **kw)


def _same(prots, pairs, matrix=None, gap_open=11, gap_extend=1, max_cells=N.ALIGN_DEFAULT_MAX_CELLS):
    """The device's records == the model's.  -> the records"""
    seq, off = M.pack(prots)
    want = A.align_model(seq, off, pairs, A.S62 if matrix is None else np.asarray(matrix), gap_open, gap_extend, max_cells)
    got = _align(prots, pairs, matrix=matrix, gap_open=gap_open, gap_extend=gap_extend, max_cells=max_cells)
    bad = np.flatnonzero(got != want)
    assert got.tobytes() == want.tobytes(), (bad[:5], got[bad[:5]], want[bad[:5]])
    return got


def _filler(rng, n, letters):
    return bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), size=n))


FILL_A, FILL_B = b"DEK", b"LIV"             # every score between the two sets is negative: only what is planted aligns


def test_the_fillers_do_not_align():
    for x in FILL_A:
        for y in FILL_B:
            assert A.S62[AS.ALPHA.index(x), AS.ALPHA.index(y)] < 0


def test_lengths_around_the_stripe():
    rng = np.random.default_rng(1)
    base = M.random_protein(rng, 200)
    rows, cols = [1, 2, 8, 9, 63, 64, 65, 127, 128, 129, 191, 193], [1, 63, 64, 65, 200]
    prots, pairs = [], []
    for m in cols:
        prots.append(base[:m])
    for n in rows:
        rel = A.mutate(rng, (base + base)[:n], 0.15)            # a relative of every centre: a mutated copy
        prots += [rel, M.random_protein(rng, n)]
        for k in range(len(cols)):
            pairs += [(len(prots) - 2, k), (len(prots) - 1, k)]
    got = _same(prots, pairs)
    assert len(got) == 120 and (got["score"] > 0).sum() > 100 and (got["status"] == 0).all()
    rel = got[0::2]
    assert (rel["score"][-4:] > 3 * got[1::2]["score"][-4:]).all()          # the relatives do align (centres of 63 and more)


@pytest.mark.parametrize("row", [STRIPE - 1, STRIPE, 129])
@pytest.mark.parametrize("col", ["first", "last"])
def test_the_best_cell_by_construction(row, col):
    rng = np.random.default_rng(2)
    n, m = 130, 90
    if col == "first":                                          # one W in column 0 and in the row
        a = _filler(rng, row, FILL_A) + b"W" + _filler(rng, n - row - 1, FILL_A)
        b = b"W" + _filler(rng, m - 1, FILL_B)
        want = (11, row, 0)
    else:                                                       # six W that end in the row and in the last column
        a = _filler(rng, row - 5, FILL_A) + b"WWWWWW" + _filler(rng, n - row - 1, FILL_A)
        b = _filler(rng, m - 6, FILL_B) + b"WWWWWW"
        want = (66, row, m - 1)
    assert len(a) == n and len(b) == m and A.sw_numpy(a, b) == want
    got = _same([a, b], [(0, 1)])
    assert (int(got["score"][0]), int(got["end_a"][0]), int(got["end_b"][0])) == want


def test_gaps_across_stripe_borders():
    rng = np.random.default_rng(3)
    p = M.random_protein(rng, 200)
    ins = lambda k: _filler(rng, k, b"W")                       # W against anything but W, Y, F is negative: the insert is a gap
    v11 = p[:60] + ins(11) + p[60:]                             # a vertical gap (F) over rows 60 .. 70
    v130 = p[:40] + ins(130) + p[40:]                           # ... and one over rows 40 .. 169: two borders
    h100 = p[:80] + ins(100) + p[80:]                           # a horizontal gap (E) of 100 columns
    prots = [p, v11, v130, h100]
    got = _same(prots, [(1, 0), (2, 0), (0, 3), (3, 0), (0, 1), (0, 2)])
    full = A.self_score(p)
    assert got["score"].tolist() == [full - 22, full - 141, full - 111, full - 111, full - 22, full - 141]
    assert got["end_a"][:3].tolist() == [210, 329, 199] and got["end_b"][:3].tolist() == [199, 199, 299]


@pytest.mark.parametrize("start", [STRIPE - 1, STRIPE, STRIPE + 1, 2 * STRIPE])
def test_a_score_that_falls_to_zero_and_restarts_behind_a_border(start):
    rng = np.random.default_rng(4)
    q1, q2 = M.random_protein(rng, 6), M.random_protein(rng, 70)
    a = _filler(rng, start - 40, FILL_A) + q1 + _filler(rng, 34, FILL_A) + q2          # q2 starts in row `start`
    b = q1 + _filler(rng, 34, FILL_B) + q2
    assert a.index(q2) == start
    got = _same([a, b], [(0, 1), (1, 0)])
    assert got["score"].tolist() == [A.self_score(q2)] * 2 and int(got["end_a"][0]) == len(a) - 1
    assert A.self_score(q1) <= 6 * 11 < 34 * 2                  # the 34 mismatches (-2 at least each) bring H back to 0


def test_a_custom_matrix_and_other_gaps():
    mat = np.full((21, 21), -3, dtype=np.int64)
    np.fill_diagonal(mat, 2)
    p = b"ACDEFGHIKLMNPQRSTVWY"
    prots = [p[:10], p[:5] + b"W" + p[6:10], p, p[:10] + p[11:], p[:10] + p[13:], b"XXXX", b"XX"]
    got = _same(prots, [(0, 0), (0, 1), (2, 3), (3, 2), (2, 4), (5, 6), (2, 2)], matrix=mat, gap_open=5, gap_extend=2)
    # ten matches; nine and a mismatch; 19 matches and a gap of one (5 + 2), both ways; 17 and a gap of three (5 + 6) against
    # the longer flank alone (2 * 10); X against X is a match in this matrix; twenty matches
    assert got["score"].tolist() == [20, 15, 31, 31, 23, 4, 40]
    assert got["self_a"].tolist() == [20, 20, 40, 38, 40, 0, 40]
    rng = np.random.default_rng(5)
    base = M.random_protein(rng, 150)
    rel = [base, base[:50] + base[53:], A.mutate(rng, base[:70] + M.random_protein(rng, 4) + base[70:], 0.1), M.random_protein(rng, 140)]
    got = _same(rel, [(a, b) for a in range(4) for b in range(4)], gap_open=5, gap_extend=2)
    plain = _same(rel, [(a, b) for a in range(4) for b in range(4)])
    assert (got["score"] >= plain["score"]).all() and (got["score"] > plain["score"]).any()
    _same(rel, [(a, b) for a in range(4) for b in range(4)], gap_open=0, gap_extend=1)
    _same(rel, [(1, 0), (2, 0)], gap_open=2 ** 31 - 1, gap_extend=2 ** 31 - 1)          # no gap pays; nothing wraps


@pytest.fixture(scope="module")
def random_pairs():
    rng = np.random.default_rng(6)
    prots = []
    for _ in range(60):
        base = M.random_protein(rng, int(rng.integers(1, 201)))
        prots.append(base)
        if rng.random() < 0.5:
            cut = int(rng.integers(0, len(base)))
            prots.append((A.mutate(rng, base[:cut], 0.1) + M.random_protein(rng, int(rng.integers(0, 8))) + A.mutate(rng, base[cut:], 0.1))[:200])
    prots = [p.replace(b"A", b"X") if k % 7 == 0 else p for k, p in enumerate(prots)]
    pairs = rng.integers(0, len(prots), size=(500, 2))
    pairs[:40, 1] = np.minimum(pairs[:40, 0] + 1, len(prots) - 1)               # neighbours: often relatives
    seq, off = M.pack(prots)
    return prots, pairs, A.align_model(seq, off, pairs)


def test_500_random_pairs_in_any_order(random_pairs):
    prots, pairs, want = random_pairs
    got = _align(prots, pairs)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:5]
    assert (want["score"] > 0).sum() > 400
    assert _align(prots, pairs[::-1]).tobytes() == want[::-1].tobytes()
    assert _align(prots, np.repeat(pairs, 2, axis=0)).tobytes() == np.repeat(want, 2).tobytes()


def test_a_pair_both_ways_and_against_itself(random_pairs):
    prots, pairs, want = random_pairs
    ab = pairs[:100]
    got = _same(prots, np.concatenate([ab, ab[:, ::-1], np.stack([ab[:, 0], ab[:, 0]], axis=1)]))
    fwd, rev, own = got[:100], got[100:200], got[200:]
    assert (fwd["score"] == rev["score"]).all() and (fwd["self_a"] == rev["self_b"]).all()
    assert fwd.tobytes() == want[:100].tobytes()
    noX = np.array([b"X" not in prots[a] for a in ab[:, 0]])
    assert (own["score"][noX] == own["self_a"][noX]).all()


def test_max_cells_and_a_long_pair_among_a_thousand_short_ones():
    rng = np.random.default_rng(7)
    p64, p65 = M.random_protein(rng, 64), M.random_protein(rng, 65)
    got = _same([p64, p65], [(0, 0), (0, 1), (1, 0), (1, 1)], max_cells=4096)
    assert got["status"].tolist() == [0, 1, 1, 1] and got["score"].tolist()[1:] == [-1, -1, -1]
    assert got["self_b"].tolist() == [A.self_score(p) for p in (p64, p65, p64, p65)]           # the self-scores of a skipped pair too
    long_a = M.random_protein(rng, 3000)
    long_b = A.mutate(rng, long_a[:1400] + long_a[1420:] + M.random_protein(rng, 20), 0.2)
    assert len(long_b) == 3000 > N.ALIGN_LDS_COLS
    short = [M.random_protein(rng, int(rng.integers(1, 30))) for _ in range(12)]
    prots = [long_a, long_b] + short
    pairs = rng.integers(2, len(prots), size=(1001, 2))
    pairs[417] = (0, 1)
    seq, off = M.pack(prots)
    want = A.align_model(seq, off, pairs, max_cells=9_000_000)
    got = _align(prots, pairs, max_cells=9_000_000)
    assert got.tobytes() == want.tobytes() and want["score"][417] > 5000 and want["status"][417] == 0
    # the same long pair alone, and with the cap one cell short
    assert _align(prots, [(0, 1)], max_cells=9_000_000).tobytes() == want[417:418].tobytes()
    assert _align(prots, [(0, 1)], max_cells=8_999_999)["status"].tolist() == [1]
    # a short member against the long centre, and the long one as the member of a short centre: both carry paths
    _same(prots, [(2, 1), (0, 3), (1, 2)])


def test_nothing_to_align():
    from kmergutsjava_amd import hotpath
    assert len(hotpath.align_proteins(b"", np.zeros(1, dtype=np.int64), np.zeros((0, 2), dtype=np.int32))) == 0
    assert len(_align([b"ACDEF"], np.zeros((0, 2), dtype=np.int32))) == 0
    got = _same([b"", b"ACDEFW", b""], [(0, 1), (1, 0), (0, 0), (2, 0), (1, 1)])
    assert got["score"].tolist() == [0, 0, 0, 0, A.self_score(b"ACDEFW")] and got["end_a"].tolist() == [-1, -1, -1, -1, 5]
    assert (got["status"] == 0).all()


def _raw(params, seq=b"ACDEFGHIKL", off=(0, 5, 10), pairs=(0, 1), n_pairs=None, out=True):
    lib = N.load()
    off = np.asarray(off, dtype=np.int64)
    pr = np.asarray(pairs, dtype=np.int32)
    n_pairs = len(pr) // 2 if n_pairs is None else n_pairs
    res = np.zeros(max(n_pairs, 1), dtype=N.ALIGNMENT_DTYPE)
    buf = np.frombuffer(seq, dtype=np.uint8)
    return lib.kg_proteins_align(0, C.byref(params) if params is not None else None, buf.ctypes.data if seq else None, off.ctypes.data,
                                 len(off) - 1, pr.ctypes.data if len(pr) else None, n_pairs, res.ctypes.data if out else None)


def _error():
    return N.load().kg_last_error().decode()


def test_errors():
    ok = lambda **kw: N.KgAlignParams(**dict(dict(min_ratio_pct=50, ref=0, gap_open=11, gap_extend=1, max_cells=1 << 26, matrix=None, reserved=0), **kw))
    assert _raw(ok()) == 0
    for params, code, words in [
            (None, N.KG_ERR_ARG, "null kg_align_params"),
            (ok(min_ratio_pct=101), N.KG_ERR_ARG, "min_ratio_pct must be in 0..100"),
            (ok(min_ratio_pct=-1, ref=5), N.KG_ERR_ARG, "min_ratio_pct must be in 0..100"),        # the first bad one is named
            (ok(ref=2), N.KG_ERR_ARG, "ref must be KG_ALIGN_REF_LONGER or KG_ALIGN_REF_MEMBER"),
            (ok(gap_open=-1), N.KG_ERR_ARG, "gap_open must be >= 0"),
            (ok(gap_extend=0), N.KG_ERR_ARG, "gap_extend must be >= 1"),
            (ok(max_cells=0), N.KG_ERR_ARG, "max_cells must be >= 1"),
            (ok(reserved=1), N.KG_ERR_ARG, "kg_align_params.reserved must be 0")]:
        assert _raw(params) == code and _error().startswith(words), (words, _error())
    mat = np.array(AS.BLOSUM62, dtype=np.int8)
    bad = mat.copy(); bad[3, 7] += 1
    assert _raw(ok(matrix=bad.ctypes.data)) == N.KG_ERR_ARG and _error().startswith("matrix is not symmetric at (3, 7)")
    bad = mat.copy(); bad[4, 4] = 17
    assert _raw(ok(matrix=bad.ctypes.data)) == N.KG_ERR_ARG and _error().startswith("matrix entry (4, 4) is outside -16..16")
    assert _raw(ok(matrix=mat.ctypes.data)) == 0
    assert _raw(ok(), pairs=(0, 2)) == N.KG_ERR_ARG and _error().startswith("pair 0: protein index 2 is outside [0, n_prot)")
    assert _raw(ok(), pairs=(0, 1, -1, 0)) == N.KG_ERR_ARG and _error().startswith("pair 1: protein index -1 is outside")
    assert _raw(ok(), off=(0, 6, 5)) == N.KG_ERR_ARG and _error().startswith("protein 1: offsets decrease")
    assert _raw(ok(), pairs=(), n_pairs=1) == N.KG_ERR_ARG and _error().startswith("null argument")
    assert _raw(ok(), out=False) == N.KG_ERR_ARG and _error().startswith("null argument")
    assert _raw(ok(), seq=b"") == N.KG_ERR_ARG and _error().startswith("null sequence")
    assert _raw(ok(), n_pairs=-1) == N.KG_ERR_ARG and _error().startswith("n_pairs < 0")
    assert _raw(ok(), off=(0, 1 << 24, (1 << 24) + 5)) == N.KG_ERR_LIMIT and _error().startswith("protein 0: 2^24 or more characters")


def test_failed_allocations_leave_nothing_behind(monkeypatch, random_pairs):
    import torch
    from kmergutsjava_amd import hotpath, synth
    prots, pairs, want = random_pairs
    prots = prots + [M.random_protein(np.random.default_rng(8), N.ALIGN_LDS_COLS + 1)]          # the slab of the long launch too
    pairs = np.concatenate([pairs[:50], [(0, len(prots) - 1)]])
    seq, off = M.pack(prots)
    mat = np.array(AS.BLOSUM62)
    rec = synth.high_density_config(4, 100, 4001, 500, dna=False)[2]
    with hotpath.SignatureTable.from_bytes(synth.table_image(rec), 0) as tab:
        first = hotpath.align_proteins(seq, off, pairs, matrix=mat)
        assert first[:50].tobytes() == want[:50].tobytes()
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        failed = 0
        for n in range(1, 40):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got = hotpath.align_proteins(seq, off, pairs, matrix=mat)
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
                assert tab.live_device_bytes() == live0
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed == 8 and got.tobytes() == first.tobytes()          # the sequence, the offsets, and align_run's six blocks
        assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0
