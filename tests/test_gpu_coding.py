"""Coding potential on the GPU (kg_orfset_coding, kg_coding_counts_orfs, kg_coding_score_orfs): counts, scores, records and
statistics must equal the model of tests/coding_model.py byte for byte -- for records of 0, 1 and 2 residues, pair counts at the
wave and workgroup sizes, one very long ORF among short ones, both strands and every frame, ORFs at a contig's first and last
codon, unknown bases, the background at contig borders on either side of the lane, wave, workgroup-step and grid borders of its
kernel (_native.CODING_BG_PER_LANE, 64 lanes, CODING_BG_TILE, CODING_MAX_GRID), a homopolymer, the threshold, the untrained path,
a caller's table (of any int32 values), the selection behind the filter, batch neighbours, the errors, failed allocations, the
call_regions front end and the E. coli genome.

Two of the errors the header names are not provoked here.  KG_ERR_BUSY: no existing hook leaves a kg_scan* in flight on a table
without a second thread (the busy flag is taken and given back inside one call; tests/test_gpu_hygiene.py races four threads for
it on 20 Mbp scans, a coding call is too short to lose such a race reliably), so it is left to the code's own reading: the call
takes the set's table through the CallScope every other set call uses.  KG_ERR_LIMIT for 2^31 records or 2^40 bytes: neither
fits a test of a few seconds.

The 2^32-pair limit does, since the records of a caller's list may overlap: 2048 records over one frame of 2^21 + 1 codons hold
2^32 pairs and fill one chunk of the prefix sum (tests/scan_model.py); the pair kernels read the pair total first and touch
nothing when it is 2^32 or more.  Below the limit, 1025 such records carry the pair prefix past the sign bit."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import coding_model as K  # noqa: E402
import free_orfs_model as F  # noqa: E402
import orfs_model as O  # noqa: E402
import scan_model as SM  # noqa: E402
import select_model as S  # noqa: E402
import test_coding_host as TH  # noqa: E402
import test_orfs_host as HO  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
PER_LANE, WAVE, TILE, GRID = N.CODING_BG_PER_LANE, 64 * N.CODING_BG_PER_LANE, N.CODING_BG_TILE, N.CODING_MAX_GRID


def _batch(contigs):
    off = np.zeros(len(contigs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in contigs])
    return np.frombuffer(b"".join(bytes(c) for c in contigs), dtype=np.uint8), off


def _table(rng):
    return rng.integers(-3000, 3000, size=K.BINS).astype(np.int32)


def _twins_equal_the_model(orfs, seq, off, T):
    """kg_coding_counts_orfs and kg_coding_score_orfs against the numpy model."""
    from kmergutsjava_amd import hotpath
    Cd, Bd = hotpath.coding_counts(orfs, seq, off)
    Cm, Bm = K.counts_np(orfs, seq, off)
    assert Cd.tobytes() == Cm.tobytes(), "coding counts"
    assert Bd.tobytes() == Bm.tobytes(), "background counts"
    got, want = hotpath.coding_scores(T, orfs, seq, off), K.scores_np(T, orfs, seq, off)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), "scores"
    return Cm, Bm, want


# ---- records: the pair kernels --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
def test_residues_0_1_2_and_pair_counts_at_wave_and_workgroup_sizes(strand):
    """Records of n_res 0 (a stop codon alone), 1, 2 (0, 0 and 1 pair) and of 63, 64, 65, 255, 256, 257 pairs, in every frame,
    some free, some not kept, in an order that puts the empty ones between the others."""
    rng = np.random.default_rng(11 + strand)
    L = 3 * 300 + 2
    seq, off = _batch([rng.choice(ACGT, size=L), rng.choice(ACGT, size=40)])
    rows = []
    for k, pairs in enumerate((63, 0, 64, 65, -1, 255, 1, 256, 0, 257, -1)):
        f = k % 3
        rows.append(K.codon_orf(L, strand, f, int(rng.integers(0, 30)), pairs + 1, stop=bool(k & 1) or pairs < 0, flags=16 if k % 4 == 3 else 1,
                                kept=int(k != 5)))
    orfs = K.records(rows)
    assert sorted(np.maximum(orfs["n_res"] - 1, 0).tolist()) == [0, 0, 0, 0, 1, 63, 64, 65, 255, 256, 257]
    Cm, _, want = _twins_equal_the_model(orfs, seq, off, _table(rng))
    # the training records are the kept, not free ones: those of 63, 64, 1 and 257 pairs
    assert Cm.sum() == 63 + 64 + 1 + 257 and np.count_nonzero(want) == 7


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_orf_of_10000_codons_among_2000_of_100(where):
    rng = np.random.default_rng(5)
    L = 3 * 10001 + 5
    seq, off = _batch([rng.choice(ACGT, size=L)])
    rows = [K.codon_orf(L, int(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(0, 9800)), 100, flags=int(rng.choice([1, 16])))
            for _ in range(2000)]
    long_one = K.codon_orf(L, 1, 1, 0, 10000, stop=False)
    rows.insert({"first": 0, "middle": 1000, "last": 2000}[where], long_one)
    orfs = K.records(rows)
    _, _, want = _twins_equal_the_model(orfs, seq, off, _table(rng))
    assert orfs["n_res"].max() == 10000 and len(orfs) == 2001 and np.count_nonzero(want) > 1990


def test_both_strands_every_frame_first_and_last_codon():
    """A record on the contig's first codon and one that ends on its last codon, for the six containers and L mod 3 = 0, 1, 2."""
    rng = np.random.default_rng(9)
    contigs, rows = [], []
    for s, L in enumerate((60, 61, 62)):
        contigs.append(rng.choice(ACGT, size=L))
        for strand in (0, 1):
            for f in (0, 1, 2):
                nf = (L - f) // 3
                rows.append(K.codon_orf(L, strand, f, 0, 5, seq=s))
                rows.append(K.codon_orf(L, strand, f, nf - 7, 7, stop=False, seq=s))
                rows.append(K.codon_orf(L, strand, f, nf - 7, 6, stop=True, seq=s))
    seq, off = _batch(contigs)
    orfs = K.records(rows)
    assert orfs["left"].min() == 0 and (orfs["right"] == np.diff(off)[orfs["seq"]] - 1).sum() >= 6
    _, _, want = _twins_equal_the_model(orfs, seq, off, _table(rng))
    assert np.count_nonzero(want) == len(orfs)


def test_unknown_bases_u_and_lower_case():
    """ATG AAA CCC GGG TAA, pairs worth 1, 10 and 100: an unknown base in codon k takes away the pairs it is the second codon
    (k - 1) and the first codon (k) of, and no other; one in the stop codon takes none; u, U and lower case read as the
    upper-case bases."""
    idx = lambda s: sum("ACGT".index(ch) << (2 * (5 - i)) for i, ch in enumerate(s))    # noqa: E731
    clean = b"CATGAAACCCGGGTAAC"
    texts = [clean, b"CATNAAACCCGGGTAAC", b"CATGAANCCCGGGTAAC", b"CATGAAACCCGGNTAAC", b"caugaAaCcCgGGUAAc", b"CATGAAACCCGGG-AAC"]
    comp = bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa")
    contigs = texts + [t.translate(comp)[::-1] for t in texts]
    seq, off = _batch(contigs)
    rows = [K.codon_orf(len(clean), 0, 1, 0, 4, seq=s) for s in range(len(texts))]
    rows += [K.codon_orf(len(clean), 1, 1, 0, 4, seq=len(texts) + s) for s in range(len(texts))]
    orfs = K.records(rows)
    T = np.zeros(K.BINS, np.int32)
    T[idx("ATGAAA")], T[idx("AAACCC")], T[idx("CCCGGG")] = 1, 10, 100
    _, _, want = _twins_equal_the_model(orfs, seq, off, T)
    assert want.tolist() == [111, 110, 100, 11, 111, 111] * 2
    rng = np.random.default_rng(2)
    w = np.array([22, 22, 22, 16, 3, 2, 2, 2, 2, 1, 4, 2], float) / 100
    orfs, seq, off = K.random_batch(rng, 40, max_len=400, weights=w)
    assert len(orfs) > 60
    _twins_equal_the_model(orfs, seq, off, _table(rng))


def test_a_table_of_any_int32_values():
    """A caller's table is any int32[4096]: entries at both ends of the range and a -10^9 "forbidden hexamer" among random ones
    over the whole range.  64 lanes of 2^31 pass 32 bits, so every sum is carried in 64: the scores of 100-codon ORFs, of one of
    10^4 codons and of an all-A run (every pair the same entry) equal the model's, and so does the decision of a set."""
    rng = np.random.default_rng(31)
    L = 3 * 10001 + 5
    seq, off = _batch([rng.choice(ACGT, size=L), b"A" * 3000])
    rows = [K.codon_orf(L, int(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(0, 9800)), 100) for _ in range(300)]
    rows += [K.codon_orf(L, 0, 2, 0, 10000, stop=False), K.codon_orf(3000, 0, 0, 0, 1000, stop=False, seq=1),
             K.codon_orf(3000, 1, 1, 3, 900, stop=False, seq=1)]
    orfs = K.records(rows)
    lo, hi = -2 ** 31, 2 ** 31 - 1
    for T in (rng.integers(lo, hi, size=K.BINS, endpoint=True).astype(np.int32), np.full(K.BINS, hi, np.int32), np.full(K.BINS, lo, np.int32)):
        T[0], T[4095], T[1234] = hi, lo, -10 ** 9
        _, _, want = _twins_equal_the_model(orfs, seq, off, T)
        assert want[-2] == 999 * hi and want[-1] == 899 * lo and np.abs(want[:300]).max() > 2 ** 33
    s = _Set(np.zeros(0, N.REGION_DTYPE), seq, off, min_res=40)
    try:
        assert len(s.records) > 10
        _same_as_model(s.coding(T), K.coding(s.records, seq, off, T))
    finally:
        s.close()


# ---- the background pass ------------------------------------------------------------------------------------------------------------

def _background(seq, off):
    from kmergutsjava_amd import hotpath
    return hotpath.coding_counts(np.zeros(0, N.ORF_DTYPE), seq, off)[1]


def _valid_positions(seq, off):
    """the hexamer starts of the batch: x with x + 5 inside x's contig and six known bases"""
    bad = np.concatenate([[0], np.cumsum(K._CODE[seq] > 3)])
    total = 0
    for a, b in zip(off[:-1].tolist(), off[1:].tolist()):
        if b - a >= 6:
            total += int((bad[a + 6:b + 1] - bad[a:b - 5] == 0).sum())
    return total


def test_background_contigs_of_5_6_7_and_a_junction():
    idx = lambda s: sum("ACGT".index(ch) << (2 * (5 - i)) for i, ch in enumerate(s))    # noqa: E731
    for contigs, total in (([b"ACGTA"], 0), ([b"ACGTAC"], 2), ([b"ACGTACG"], 4), ([b"ACG", b"TAC"], 0), ([b"ACGTAC", b"GTACGT"], 4),
                           ([b"", b"ACGTAC", b"", b""], 2), ([b"ACGTNC", b"ACNNNNACGTAC"], 2)):
        seq, off = _batch(contigs)
        B = _background(seq, off)
        assert B.tobytes() == K.background_np(seq, off).tobytes() and B.sum() == total == 2 * _valid_positions(seq, off), contigs
    B = _background(*_batch([b"ACGTAC"]))
    assert B[idx("ACGTAC")] == 1 and B[idx("GTACGT")] == 1
    # two contigs whose junction would spell GGGCCC: the hexamer is counted only when they are one contig
    assert _background(*_batch([b"AAAGGG", b"CCCAAA"]))[idx("GGGCCC")] == 0 and _background(*_batch([b"AAAGGGCCCAAA"]))[idx("GGGCCC")] == 2


def test_background_borders_of_lanes_waves_workgroup_steps_and_the_grid():
    """Contig borders and unknown bases a few bytes on either side of every multiple of a lane's starts, of a wave's and of a
    workgroup step's near the start of the batch, and on either side of the byte where the grid wraps (CODING_MAX_GRID steps)."""
    rng = np.random.default_rng(21)
    wrap = GRID * TILE
    total = wrap + 3 * TILE + 17
    seq = rng.choice(ACGT, size=total).astype(np.uint8)
    cuts = set()
    for edge in (PER_LANE, 2 * PER_LANE, WAVE, 2 * WAVE, 4 * WAVE, TILE, 2 * TILE, 3 * TILE, wrap, wrap + TILE, wrap + 2 * TILE):
        for d in (-7, -5, -1, 0, 1, 6):
            cuts.add(edge + d)
    for edge in (5 * TILE, 6 * TILE + WAVE, 7 * TILE + PER_LANE, wrap - TILE, wrap + 3 * TILE):
        for d in (-6, -3, 0, 2, 5):
            seq[edge + d] = ord("N")
    off = np.array([0] + sorted(cuts) + [total], dtype=np.int64)
    B = _background(seq, off)
    want = K.background_np(seq, off)
    assert B.tobytes() == want.tobytes() and B.sum() == 2 * _valid_positions(seq, off)
    # one contig: the same bytes without the borders
    one = np.array([0, total], dtype=np.int64)
    B1 = _background(seq, one)
    assert B1.tobytes() == K.background_np(seq, one).tobytes() and B1.sum() > B.sum()


def test_background_homopolymer():
    """An all-A contig of 10^5 sends every count to one bin (and its reverse complement's)."""
    seq, off = _batch([b"A" * 100000, b"ACGTACGTAC"])
    B = _background(seq, off)
    assert B.tobytes() == K.background_np(seq, off).tobytes()
    assert B[0] == 99995 and B[4095] == 99995 and B.sum() == 2 * (99995 + 5)
    # ... and as an ORF: 33332 identical pairs of a training record
    orfs = K.records([K.codon_orf(100000, 0, 0, 0, 33333, stop=False), K.codon_orf(100000, 1, 2, 5, 1000, stop=False)])
    T = np.zeros(K.BINS, np.int32)
    T[0], T[4095] = 3, -7
    C_, _, want = _twins_equal_the_model(orfs, seq, off, T)
    assert C_[0] == 33332 and C_[4095] == 999 and want.tolist() == [3 * 33332, -7 * 999]


# ---- sets: kg_orfset_coding ---------------------------------------------------------------------------------------------------------

class _Set:
    """An ORF set of caller-held regions and the batch's free ORFs, and kg_orfset_coding on it."""

    def __init__(self, regs, seq, off, min_res=30, only_kept=0):
        self.lib, self.seq, self.off = N.load(), np.ascontiguousarray(seq), np.ascontiguousarray(off)
        ev, self.h = C.c_void_p(), C.c_void_p()
        N.check(self.lib.kg_orfs_regions(0, C.byref(N.KgOrfParams(7, only_kept, 0)), regs.ctypes.data if len(regs) else None, len(regs),
                                         self.seq.ctypes.data, self.off.ctypes.data, len(off) - 1, C.byref(ev)))
        self.ev = ev
        try:
            N.check(self.lib.kg_orfset_add_free(ev, C.byref(N.KgFreeParams(min_res, 7, 0)), self.seq.ctypes.data, 0, self.off.ctypes.data,
                                                len(off) - 1, C.byref(self.h)))
        except BaseException:
            self.lib.kg_orfset_free(ev)
            raise
        self.records = self.copy(self.h)

    def copy(self, h):
        n = int(self.lib.kg_orfset_count(h))
        out = np.zeros(n, dtype=N.ORF_DTYPE)
        N.check(self.lib.kg_orfset_copy(h, 0, n, out.ctypes.data if n else None))
        return out

    def coding(self, table=None, min_coding=0, min_train=100000, of=None, select=False):
        """-> (records, scores, statistics, (C, B), prot_start and residues bytes[, selection]) of a new set, which is freed."""
        from kmergutsjava_amd import hotpath
        new = C.c_void_p()
        t = None if table is None else np.ascontiguousarray(table, dtype=np.int32)
        N.check(self.lib.kg_orfset_coding(of or self.h, C.byref(N.KgCodingParams(min_coding, 0, min_train)), None if t is None else t.ctypes.data,
                                          self.seq.ctypes.data, 0, self.off.ctypes.data, len(self.off) - 1, C.byref(new)))
        scores, st, model = hotpath._coding_results(new)
        sel = None
        if select:
            sh = C.c_void_p()
            N.check(self.lib.kg_orfset_select(new, C.byref(N.KgSelectParams(60, 50, 0)), C.byref(sh)))
            sel = hotpath._take_selectset(sh, False)[0]
        recs, ps, res, _ = hotpath._take_orfset(new, False)
        return (recs, scores, {k: v for k, v in st.items() if not k.startswith("ms_")}, model, ps.tobytes() + res.tobytes()) + ((sel,) if select else ())

    def rest(self):
        from kmergutsjava_amd import hotpath
        _, ps, res, _ = hotpath._take_orfset(self.h, False)
        self.h = None
        return ps.tobytes() + res.tobytes()

    def close(self):
        if self.h:
            self.lib.kg_orfset_free(self.h)
        self.lib.kg_orfset_free(self.ev)


def _same_as_model(got, want):
    assert got[0].tobytes() == want[0].tobytes(), "records"
    assert got[1].dtype == want[1].dtype and got[1].tobytes() == want[1].tobytes(), "scores"
    assert got[2] == want[2], (got[2], want[2])
    assert got[3][0].tobytes() == want[3][0].tobytes() and got[3][1].tobytes() == want[3][1].tobytes(), "counts"


_SETS = {}


def _random_set():
    """30 random contigs with regions (some not kept, some multi-frame, their ORFs often interrupted) and free ORFs of 30 residues."""
    if "random" not in _SETS:
        rng = np.random.default_rng(5)
        w = np.array([4, 44, 44, 4, 0, 1, 1, 1, 0, 1, 0], float) / 100
        regs, seq, off = O.random_batch(rng, 30, max_len=2500, max_regions=6, weights=w)
        _SETS["random"] = (regs, seq, off)
    return _SETS["random"]


def test_own_training_the_threshold_and_the_untrained_path():
    regs, seq, off = _random_set()
    s = _Set(regs, seq, off)
    try:
        recs = s.records
        want = K.coding(recs, seq, off, None, 0, 0)
        n_pairs = want[2]["training_pairs"]
        free = np.flatnonzero((recs["flags"] & K.FREE) != 0)
        assert want[2]["trained"] == 1 and n_pairs > 300 and len(free) > 20 and want[2]["training_records"] > 5
        assert 0 < want[2]["noncoding"] < len(free) and (recs["kept"] == 0).any()
        got = s.coding(None, 0, 0)
        _same_as_model(got, want)
        # the threshold: S == min_coding is kept, min_coding - 1 ... S is dropped
        i = free[len(free) // 2]
        at = int(want[1][i])
        for mc in (at, at + 1):
            got = s.coding(None, mc, 0)
            _same_as_model(got, K.coding(recs, seq, off, None, mc, 0))
            assert bool(got[0]["kept"][i]) == (mc == at) and bool(got[0]["flags"][i] & K.NONCODING) == (mc != at)
        # evidence ORFs are scored and never dropped, whatever their score; nothing but kept and the flag changes
        hard = s.coding(None, 10 ** 9, 0)
        _same_as_model(hard, K.coding(recs, seq, off, None, 10 ** 9, 0))
        ev = (recs["flags"] & K.FREE) == 0
        assert hard[0][ev].tobytes() == recs[ev].tobytes() and (hard[0]["kept"][~ev] == 0).all() and hard[2]["noncoding"] == len(free)
        back = hard[0].copy()
        back["kept"][~ev] = 1
        back["flags"][~ev] &= ~np.uint32(K.NONCODING)
        assert back.tobytes() == recs.tobytes()
        # untrained: sum C = min_train_pairs - 1 against sum C = min_train_pairs
        un = s.coding(None, 10 ** 9, n_pairs + 1)
        _same_as_model(un, K.coding(recs, seq, off, None, 10 ** 9, n_pairs + 1))
        assert un[2]["trained"] == 0 and not un[1].any() and un[0].tobytes() == recs.tobytes() and un[2]["training_pairs"] == n_pairs
        assert s.coding(None, 0, n_pairs)[2]["trained"] == 1
        # prot_start and the residues are the given set's, and the given set is unchanged
        assert s.copy(s.h).tobytes() == recs.tobytes()
        assert got[4] == hard[4] == un[4] == s.rest()
    finally:
        s.close()


def test_a_callers_table_and_a_second_pass():
    from kmergutsjava_amd import hotpath
    regs, seq, off = _random_set()
    s = _Set(regs, seq, off)
    try:
        recs = s.records
        own = s.coding(None, 0, 0)
        T = hotpath.coding_table(*own[3])
        assert T.tobytes() == K.table(*own[3]).tobytes()
        got = s.coding(T, 0, 10 ** 12)                  # (min_train_pairs plays no part with a table)
        want = K.coding(recs, seq, off, T, 0, 10 ** 12)
        _same_as_model(got, want)
        assert got[2]["trained"] == 2 and not got[3][0].any() and not got[3][1].any() and got[2]["background"] == 0
        assert got[0].tobytes() == own[0].tobytes() and got[1].tobytes() == own[1].tobytes()
        # an evidence ORF with a very negative score is untouched; every free ORF goes
        low = np.full(K.BINS, -30000, np.int32)
        neg = s.coding(low)
        _same_as_model(neg, K.coding(recs, seq, off, low))
        ev = (recs["flags"] & K.FREE) == 0
        assert neg[1][ev].min() < -10 ** 6 and neg[0][ev].tobytes() == recs[ev].tobytes() and neg[2]["noncoding"] == (~ev).sum()
        # a second pass over a set that has dropped records: a free record with kept = 0 gets no (new) flag and is not counted
        first, second = C.c_void_p(), None
        N.check(s.lib.kg_orfset_coding(s.h, C.byref(N.KgCodingParams(0, 0, 0)), T.ctypes.data, s.seq.ctypes.data, 0, s.off.ctypes.data,
                                       len(off) - 1, C.byref(first)))
        try:
            mid = s.copy(first)
            assert mid.tobytes() == own[0].tobytes()
            second = s.coding(low, of=first)
            _same_as_model(second, K.coding(mid, seq, off, low))
            assert second[2]["noncoding"] == (~ev).sum() - own[2]["noncoding"]
        finally:
            s.lib.kg_orfset_free(first)
    finally:
        s.close()


def test_a_dropped_free_orf_no_longer_suppresses_a_weaker_one():
    rng = np.random.default_rng(8)
    seq, off = _batch([rng.choice(ACGT, size=30000), rng.choice(ACGT, size=9000)])
    T = _table(rng)
    s = _Set(np.zeros(0, N.REGION_DTYPE), seq, off, min_res=40)
    try:
        recs = s.records
        want = K.coding(recs, seq, off, T)
        got = s.coding(T, select=True)
        _same_as_model(got, want)
        before, after = S.select_fast(S.of_records(recs)), S.select_fast(S.of_records(want[0]))
        assert got[5].tobytes() == after.tobytes()
        dropped = (want[0]["flags"] & K.NONCODING) != 0
        freed = (before["state"] == 2) & dropped[np.maximum(before["by"], 0)] & (after["state"] == 1)
        assert freed.sum() > 0 and (after["state"][dropped] == 0).all() and len(recs) > 100
    finally:
        s.close()


def test_batch_neighbours_do_not_matter():
    rng = np.random.default_rng(12)
    T = _table(rng)
    contigs = [rng.choice(ACGT, size=n) for n in (700, 1501, 0, 902, 5, 1300)]
    rows = [[K.codon_orf(len(c), int(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(0, 20)), int(rng.integers(2, 150)))
             for _ in range(6)] if len(c) > 600 else [] for c in contigs]
    seq, off = _batch(contigs)
    orfs = K.records([r[:0] + (s,) + r[1:] for s, rs in enumerate(rows) for r in rs])
    Cm, Bm, want = _twins_equal_the_model(orfs, seq, off, T)
    sumC, sumB, at = np.zeros(K.BINS, np.int64), np.zeros(K.BINS, np.int64), 0
    for s, c in enumerate(contigs):
        alone = K.records(rows[s])
        one_seq, one_off = _batch([c])
        Ca, Ba, Sa = _twins_equal_the_model(alone, one_seq, one_off, T)
        assert Sa.tobytes() == want[at:at + len(alone)].tobytes()
        sumC, sumB, at = sumC + Ca, sumB + Ba, at + len(alone)
    assert sumC.tobytes() == Cm.tobytes() and sumB.tobytes() == Bm.tobytes()


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_errors_and_their_messages():
    from kmergutsjava_amd import hotpath
    lib = N.load()
    rng = np.random.default_rng(1)
    seq, off = _batch([rng.choice(ACGT, size=300), rng.choice(ACGT, size=90)])
    good = [K.codon_orf(300, 0, 0, 3, 20), K.codon_orf(90, 1, 1, 2, 10, seq=1), K.codon_orf(300, 1, 2, 0, 50)]
    T = _table(rng)
    _twins_equal_the_model(K.records(good), seq, off, T)
    for bad, word in ((K.orf(2, 0, 0, 29, 9), "seq outside"), (K.orf(-1, 0, 0, 29, 9), "seq outside"), (K.orf(0, 2, 0, 29, 9), "strand"),
                      (K.orf(0, 0, 30, 29, 9), "outside its contig"), (K.orf(1, 0, 0, 90, 9), "outside its contig"),
                      (K.orf(0, 0, -1, 29, 9), "outside its contig"), (K.orf(1, 0, 0, 29, 11), "n_res")):
        for where in (0, 2, 3):
            rows = list(good)
            rows.insert(where, bad)
            rows.append(K.orf(7, 0, 0, 29, 9))          # a later bad record: the message names the first
            for call in (lambda o: hotpath.coding_counts(o, seq, off), lambda o: hotpath.coding_scores(T, o, seq, off)):
                with pytest.raises(N.KmerGutsNativeError) as ei:
                    call(K.records(rows))
                assert ei.value.code == N.KG_ERR_ARG and "record %d:" % where in str(ei.value) and word in str(ei.value), str(ei.value)
    o = K.records(good)
    m, sc = N.KgCodingModel(), np.zeros(3, np.int64)
    args = (o.ctypes.data, 3, seq.ctypes.data, off.ctypes.data, 2)
    assert lib.kg_coding_counts_orfs(0, *args, None) == N.KG_ERR_ARG
    assert lib.kg_coding_counts_orfs(0, None, 3, seq.ctypes.data, off.ctypes.data, 2, C.byref(m)) == N.KG_ERR_ARG and b"records" in lib.kg_last_error()
    assert lib.kg_coding_counts_orfs(0, o.ctypes.data, -1, seq.ctypes.data, off.ctypes.data, 2, C.byref(m)) == N.KG_ERR_ARG
    assert lib.kg_coding_counts_orfs(0, o.ctypes.data, 3, None, off.ctypes.data, 2, C.byref(m)) == N.KG_ERR_ARG and b"sequence" in lib.kg_last_error()
    assert lib.kg_coding_counts_orfs(0, o.ctypes.data, 3, seq.ctypes.data, None, 2, C.byref(m)) == N.KG_ERR_ARG
    assert lib.kg_coding_score_orfs(0, None, *args, sc.ctypes.data) == N.KG_ERR_ARG
    assert lib.kg_coding_score_orfs(0, T.ctypes.data, *args, None) == N.KG_ERR_ARG
    down = np.array([0, 300, 200], np.int64)
    assert lib.kg_coding_counts_orfs(0, o.ctypes.data, 3, seq.ctypes.data, down.ctypes.data, 2, C.byref(m)) == N.KG_ERR_ARG and b"contig 1" in lib.kg_last_error()
    # zero records and zero sequences are valid
    none = np.zeros(1, np.int64)
    Cz, Bz = hotpath.coding_counts(np.zeros(0, N.ORF_DTYPE), b"", none)
    assert not Cz.any() and not Bz.any() and len(hotpath.coding_scores(T, np.zeros(0, N.ORF_DTYPE), b"", none)) == 0
    # the set calls
    s = _Set(np.zeros(0, N.REGION_DTYPE), seq, off, min_res=5)
    try:
        h2, p = C.c_void_p(), N.KgCodingParams(0, 0, 0)
        a = (seq.ctypes.data, 0, off.ctypes.data, 2)
        assert lib.kg_orfset_coding(None, C.byref(p), None, *a, C.byref(h2)) == N.KG_ERR_ARG and b"kg_orfset" in lib.kg_last_error()
        assert lib.kg_orfset_coding(s.h, None, None, *a, C.byref(h2)) == N.KG_ERR_ARG and b"kg_coding_params" in lib.kg_last_error()
        assert lib.kg_orfset_coding(s.h, C.byref(p), None, *a, None) == N.KG_ERR_ARG
        assert lib.kg_orfset_coding(s.h, C.byref(N.KgCodingParams(0, 1, 0)), None, *a, C.byref(h2)) == N.KG_ERR_ARG and b"reserved" in lib.kg_last_error()
        assert lib.kg_orfset_coding(s.h, C.byref(N.KgCodingParams(0, 0, -1)), None, *a, C.byref(h2)) == N.KG_ERR_ARG and b"min_train_pairs" in lib.kg_last_error()
        assert lib.kg_orfset_coding(s.h, C.byref(p), None, seq.ctypes.data, 0, off.ctypes.data, 1, C.byref(h2)) == N.KG_ERR_ARG and b"n_seqs" in lib.kg_last_error()
        assert lib.kg_orfset_coding(s.h, C.byref(p), None, None, 0, off.ctypes.data, 2, C.byref(h2)) == N.KG_ERR_ARG and b"sequence" in lib.kg_last_error()
        assert lib.kg_orfset_coding(s.h, C.byref(p), None, seq.ctypes.data, 0, None, 2, C.byref(h2)) == N.KG_ERR_ARG
        # other offsets than the set was made with: its records are checked against them, none is used as an index
        short = np.array([0, 30, 60], np.int64)
        assert lib.kg_orfset_coding(s.h, C.byref(p), None, seq.ctypes.data, 0, short.ctypes.data, 2, C.byref(h2)) == N.KG_ERR_ARG
        assert b"record " in lib.kg_last_error() and not h2.value
        # a set that has no scores
        st, one = N.KgCodingStats(), np.zeros(1, np.int64)
        assert lib.kg_orfset_coding_scores(s.h, 0, 1, one.ctypes.data) == N.KG_ERR_ARG and b"no scores" in lib.kg_last_error()
        assert lib.kg_orfset_coding_stats(s.h, C.byref(st)) == N.KG_ERR_ARG and lib.kg_orfset_coding_model(s.h, C.byref(m)) == N.KG_ERR_ARG
        N.check(lib.kg_orfset_coding(s.h, C.byref(p), None, *a, C.byref(h2)))
        try:
            n = int(lib.kg_orfset_count(h2))
            assert n == len(s.records) > 0
            assert lib.kg_orfset_coding_scores(h2, 0, n + 1, one.ctypes.data) == N.KG_ERR_ARG and b"range" in lib.kg_last_error()
            assert lib.kg_orfset_coding_scores(h2, -1, 1, one.ctypes.data) == N.KG_ERR_ARG
            assert lib.kg_orfset_coding_scores(h2, 0, 1, None) == N.KG_ERR_ARG and lib.kg_orfset_coding_stats(h2, None) == N.KG_ERR_ARG
            assert lib.kg_orfset_coding_scores(None, 0, 1, one.ctypes.data) == N.KG_ERR_ARG
            N.check(lib.kg_orfset_coding_scores(h2, n - 1, 1, one.ctypes.data))
            import torch
            dev = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            N.check(lib.kg_orfset_coding_scores(h2, 0, n, C.c_void_p(dev.data_ptr())))
            assert dev.cpu().numpy().tobytes() == K.coding(s.records, seq, off, None, 0, 0)[1].tobytes() and dev[n - 1].item() == one[0]
        finally:
            lib.kg_orfset_free(h2)
    finally:
        s.close()


# ---- the prefix sum under the pairs: the 2^32 limit at the wrap, and a legal prefix past the sign bit -----------------------------------

_LIMIT = {}


def _limit_rows():
    """The batch of tests/scan_model.py with 2^21 + 1 sense codons, and the three records of its lists.  coding_lens_kernel gives
    a record n_res - 1 pairs whatever its flags: the long record, the first 2^21 + 1 codons of the long contig, has 2^21, the
    short one, six codons of the short contig, has five, and a record of one codon has none."""
    if not _LIMIT:
        seq, off = SM.limit_batch(SM.LONG + 1)
        L0, L1 = int(off[1]), int(off[2] - off[1])
        _LIMIT["w"] = (seq, off, K.codon_orf(L1, 0, 0, 0, SM.LONG + 1, seq=1), K.codon_orf(L0, 0, 0, 1, 6, stop=False, seq=0),
                       K.codon_orf(L0, 0, 0, 2, 1, stop=False, seq=0))
    return _LIMIT["w"]


def test_pair_totals_that_wrap_a_chunk_of_the_prefix_sum_are_refused():
    """The lists of scan_model.families through kg_coding_counts_orfs and kg_coding_score_orfs: 2048 records of 2^21 pairs
    alone, behind 2048 short records, in reversed order, and -- the control, refused whatever the chunk sums' width -- half in
    each of two chunks.  tests/test_scan_model_host.py shows that 32-bit chunk sums gave the first three a total below 2^32.
    Every call is refused with the stage's own words, leaves no device memory behind, and the next call is an ordinary one."""
    import torch
    from kmergutsjava_amd import hotpath
    seq, off, long_row, short_row, none_row = _limit_rows()
    rng = np.random.default_rng(6)
    T = _table(rng)
    small, small_seq, small_off = K.random_batch(rng, 12, max_len=300)
    with hotpath.SignatureTable.from_bytes(_workload()[0], 0) as tab:
        _twins_equal_the_model(small, small_seq, small_off, T)          # once first: what the runtime sets up on first use is not counted
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        for name, (lens, _) in SM.families(5).items():
            orfs = SM.records_of(lens, long_row, short_row, none_row, N.ORF_DTYPE)
            assert np.maximum(orfs["n_res"].astype(np.int64) - 1, 0).tolist() == lens.tolist() and SM.scan_exact(lens)[1] >= SM.LIMIT
            for call in (lambda: hotpath.coding_counts(orfs, seq, off), lambda: hotpath.coding_scores(T, orfs, seq, off)):
                with pytest.raises(N.KmerGutsNativeError) as ei:
                    call()
                assert ei.value.code == N.KG_ERR_LIMIT, name
                assert SM.message_of(ei.value).startswith("2^32 or more codon pairs"), (name, str(ei.value))
                assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0, name
        _twins_equal_the_model(small, small_seq, small_off, T)


def test_1025_records_of_2_21_pairs_carry_the_prefix_past_the_sign_bit():
    """scan_model.LEGAL: 2^31 + 2^21 pairs, legal, nothing allocated per pair; the last record's prefix is 2^31, inside the
    prefix sum's first chunk.  All records are the same training record, so the coding counts are 1025 times the model's counts
    of one, and the background is the batch's.
    Measured on the MI355X: 0.15 s for the test, the model's counts of one record included; the slowest test of this file,
    test_call_regions_coding_end_to_end, took 6.6 s in the same suite."""
    from kmergutsjava_amd import hotpath
    seq, off, long_row, _, _ = _limit_rows()
    n = len(SM.LEGAL)
    orfs = K.records([long_row] * n)
    assert n == 1025 and (orfs["n_res"].astype(np.int64) - 1).tolist() == SM.LEGAL.tolist()
    one, B = K.counts_np(orfs[:1], seq, off)
    assert one.sum() == SM.LONG and K.is_training(orfs[0])
    Cd, Bd = hotpath.coding_counts(orfs, seq, off)
    assert Cd.dtype == one.dtype and Cd.tobytes() == (n * one).tobytes(), "coding counts"
    assert Bd.tobytes() == B.tobytes(), "background counts"


# ---- behind a scan ------------------------------------------------------------------------------------------------------------------

_WORK = {}


def _workload():
    if not _WORK:
        _WORK["w"] = HO.planted_orf_contigs()
    return _WORK["w"]


def test_behind_a_scan_from_host_and_device_bytes():
    import torch
    from kmergutsjava_amd import hotpath
    img, dna, off, genes = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    d_seq = torch.from_numpy(sb.copy()).cuda()
    torch.cuda.synchronize()
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        live0 = tab.live_device_bytes()
        for ptr in (None, d_seq.data_ptr()):
            with tab.scan(None if ptr else sb, off, hotpath.Params(min_hits=4), device_ptr=ptr) as r:
                live1 = tab.live_device_bytes()
                plain = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, free_min_res=100)
                got = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, free_min_res=100, coding=True, min_train_pairs=1000)
                want = K.coding(plain[2], dna, off, None, 0, 1000)
                st = {k: v for k, v in r.coding_stats.items() if not k.startswith("ms_")}
                _same_as_model((got[2], r.coding_scores, st, r.coding_model), want)
                assert want[2]["trained"] == 1 and 0 < want[2]["noncoding"] and got[3].tobytes() == plain[3].tobytes() and got[4].tobytes() == plain[4].tobytes()
                assert r.coding_stats["ms_count"] > 0 and r.coding_stats["ms_score"] > 0 and tab.live_device_bytes() == live1
                sel = r.select(off, None if ptr else sb, 300, 12, 100, orfs=True, device_ptr=ptr, free_min_res=100, coding=True, min_train_pairs=1000)
                assert sel[2].tobytes() == want[0].tobytes() and sel[5].tobytes() == S.select_fast(S.of_records(want[0])).tobytes()
                T = hotpath.coding_table(*want[3])
                with_table = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, free_min_res=100, coding=T)
                assert with_table[2].tobytes() == want[0].tobytes() and r.coding_stats["trained"] == 2 and tab.live_device_bytes() == live1
                with pytest.raises(ValueError):
                    r.select(off, coding=True)
                # a table of the wrong shape is refused before any set is made, and nothing is left in the table's context;
                # coding=False is coding=None
                for call in (r.orfs, lambda *a, **kw: r.select(off, a[0], *a[2:], orfs=True, **kw)):
                    with pytest.raises(ValueError):
                        call(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, free_min_res=100, coding=np.zeros(10, np.int32))
                    assert tab.live_device_bytes() == live1
                off_run = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, free_min_res=100, coding=False)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(off_run, plain)) and tab.live_device_bytes() == live1
        assert tab.live_device_bytes() == live0


def test_orfs_and_select_run_the_same_steps():
    """ScanResult.orfs and select(orfs=True) with every step on -- repair, free ORFs, coding, starts -- leave the same five
    arrays and the same side results, byte for byte (the device times apart)."""
    from kmergutsjava_amd import hotpath
    img, dna, off, _ = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    kw = dict(repair=True, free_min_res=100, coding=True, min_train_pairs=1000, starts=True, min_train_starts=1)
    sides = ("coding_scores", "coding_stats", "coding_model", "start_shifts", "start_stats", "start_model", "junctions", "junction_start",
             "repair_stats", "orf_stats", "region_stats")

    def flat(x):
        """arrays as their bytes, statistics without their device times"""
        if isinstance(x, dict):
            return {k: v for k, v in x.items() if k != "ms" and not k.startswith("ms_")}
        return x.tobytes() if isinstance(x, np.ndarray) else [flat(y) for y in x]

    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        with tab.scan(sb, off, hotpath.Params(min_hits=4)) as r:
            live1 = tab.live_device_bytes()
            a = r.orfs(sb, off, 300, 12, 100, **kw)
            side_a = {k: flat(getattr(r, k)) for k in sides}
            for k in sides + ("select_stats",):
                if hasattr(r, k):
                    delattr(r, k)
            b = r.select(off, sb, 300, 12, 100, orfs=True, **kw)
            side_b = {k: flat(getattr(r, k)) for k in sides}
            assert len(a) == 5 and len(b) == 6 and flat(a) == flat(b[:5])
            assert side_a == side_b
            n = len(a[2])
            assert n > len(a[0]) > 0 and r.repair_stats["repaired"] > 0 and r.coding_stats["trained"] == 1 and r.start_stats["trained"] == 1
            assert len(r.coding_scores) == len(r.start_shifts) == len(b[5]) == n and r.select_stats["ms"] > 0
            assert tab.live_device_bytes() == live1
        assert tab.live_device_bytes() == 0


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    """Every allocation of the three calls fails once.  The set call runs beside an open table, on an ORF set made from a scan
    of it: after every failure the table's live bytes are what they were, and 0 when the sets and the result are freed."""
    import torch
    from kmergutsjava_amd import hotpath
    lib = N.load()
    rng = np.random.default_rng(4)
    orfs, seq, off = K.random_batch(rng, 30, max_len=600)
    T = _table(rng)
    want_c, want_s = K.counts_np(orfs, seq, off), K.scores_np(T, orfs, seq, off)
    hotpath.coding_counts(orfs, seq, off)               # once first: what the runtime sets up on first use is not counted
    hotpath.coding_scores(T, orfs, seq, off)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for which in ("counts", "scores"):
        failed = 0
        for n in range(1, 50):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got = hotpath.coding_counts(orfs, seq, off) if which == "counts" else hotpath.coding_scores(T, orfs, seq, off)
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= 9                              # records, bytes, offsets, words, three of the prefix sum, two or more of the pass
        if which == "counts":
            assert got[0].tobytes() == want_c[0].tobytes() and got[1].tobytes() == want_c[1].tobytes()
        else:
            assert got.tobytes() == want_s.tobytes()
    img, dna, doff, _ = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        with tab.scan(sb, doff, hotpath.Params(min_hits=4)) as r:
            rh, oh, fh, ch = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            batch = (sb.ctypes.data, 0, doff.ctypes.data, len(doff) - 1)
            N.check(lib.kg_result_regions(r._h, C.byref(N.KgRegionParams(300, 12, 100)), doff.ctypes.data, C.byref(rh)))
            try:
                N.check(lib.kg_regionset_orfs(rh, C.byref(N.KgOrfParams(7, 1, 0)), *batch, C.byref(oh)))
                N.check(lib.kg_orfset_add_free(oh, C.byref(N.KgFreeParams(100, 7, 0)), *batch, C.byref(fh)))
                n_recs = int(lib.kg_orfset_count(fh))
                recs = np.zeros(n_recs, dtype=N.ORF_DTYPE)
                N.check(lib.kg_orfset_copy(fh, 0, n_recs, recs.ctypes.data))
                live1 = tab.live_device_bytes()
                failed, p = 0, N.KgCodingParams(0, 0, 1000)
                for n in range(1, 50):
                    monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
                    rc = lib.kg_orfset_coding(fh, C.byref(p), None, *batch, C.byref(ch))
                    if rc == 0:
                        break
                    assert rc == N.KG_ERR_NOMEM and not ch.value and b"KG_TEST_FAIL_ALLOC" in lib.kg_last_error()
                    failed += 1
                    assert tab.live_device_bytes() == live1
                monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
                # the bytes, the new set's four arrays, offsets, words, three of the prefix sum, three histograms, the table
                assert failed == 14 and ch.value
                scores, st, model = hotpath._coding_results(ch)
                got = hotpath._take_orfset(ch, False)
                want = K.coding(recs, dna, doff, None, 0, 1000)
                _same_as_model((got[0], scores, {k: v for k, v in st.items() if not k.startswith("ms_")}, model), want)
                assert want[2]["trained"] == 1 and tab.live_device_bytes() == live1
            finally:
                for h, free in ((fh, lib.kg_orfset_free), (oh, lib.kg_orfset_free), (rh, lib.kg_regionset_free)):
                    if h.value:
                        free(h)
        assert tab.live_device_bytes() == 0


# ---- the front end --------------------------------------------------------------------------------------------------------------------

def test_call_regions_coding_end_to_end(tmp_path):
    """call_regions --free-orfs --coding --select --orfs --faa with and without --all on the planted contigs: every line against
    the model's records through the writers (which tests/test_coding_host.py checks line by line, as it checks --coding-model
    and the untrained warning), the saved model against the model's counts, and without --coding the bytes the writers gave
    before: the writers on the library's records, and the digests recorded from the writers of the commit before --coding
    (tests/golden/call_regions_planted_before_coding.json)."""
    from kmergutsjava_amd import call_regions as CR
    from kmergutsjava_amd import hotpath, synth
    img, dna, off, genes = _workload()
    n = len(off) - 1
    ids = [b"contig_%d" % k for k in range(n)]
    q = tmp_path / "c.fna"
    q.write_bytes(b"".join(b">%s planted genes\n%s\n" % (ids[k], dna[off[k]:off[k + 1]]) for k in range(n)))
    d = tmp_path / "d"
    synth.write_data_dir(str(d), img, 50)
    fnames = [b"synthetic function %d" % i for i in range(50)]
    base = [sys.executable, "-m", "kmergutsjava_amd.call_regions", "-D", str(d), "-q", str(q), "-m", "4", "--merge-gap", "300",
            "--min-score", "12", "--min-len", "100"]

    def run(tag, *extra):
        p = subprocess.run(base + ["-o", str(tmp_path / (tag + ".tsv")), "--orfs", str(tmp_path / (tag + ".orfs")), "--faa",
                                   str(tmp_path / (tag + ".faa"))] + list(extra), capture_output=True, text=True, cwd=ROOT)
        assert p.returncode == 0, p.stderr
        warnings = [ln for ln in p.stderr.splitlines() if ln.startswith("Warning: ")]
        return p.stdout.strip(), [(tmp_path / (tag + ext)).read_bytes() for ext in (".tsv", ".orfs", ".faa")], warnings

    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(np.frombuffer(dna, np.uint8), off, hotpath.Params(min_hits=4)) as r:
        plain = {ok: r.select(off, dna, 300, 12, 100, orfs=True, only_kept=ok, free_min_res=100) for ok in (True, False)}
    model = str(tmp_path / "model.txt")
    for write_all in (False, True):
        regs, start, orfs0, ps, res, sel0 = plain[not write_all]
        nr = len(regs)
        orfs, scores, st, counts = K.coding(orfs0, dna, off, None, 0, 1000)
        sel = S.select_fast(S.of_records(orfs))
        dropped = int(((orfs["flags"] & K.NONCODING) != 0).sum())
        assert st["trained"] == 1 and 0 < dropped < len(orfs) - nr
        line, files, err = run("all" if write_all else "sel", "--select", "--free-orfs", "--coding", "--min-train", "1000",
                               "--save-coding-model", model, *(["--all"] if write_all else []))
        assert err == []
        assert line == (CR.summary_of(regs, start) + CR.orf_summary(orfs[:nr]) + CR.select_summary(sel) + ", free: %d" % (len(orfs) - nr) +
                        ", coding: own, noncoding: %d" % dropped)
        assert files[0] == CR.format_regions(ids, regs, fnames, write_all, sel=sel[:nr], cands=orfs)
        assert files[1] == CR.format_orfs(ids, regs, orfs[:nr], fnames, write_all, sel[:nr], orfs[nr:], sel[nr:], orfs, scores[:nr], scores[nr:])
        assert files[2] == CR.format_faa(ids, regs, orfs[:nr], ps[:nr + 1], res[:ps[nr]], fnames, write_all, sel[:nr], orfs[nr:], sel[nr:],
                                         ps[nr:] - ps[nr], res[ps[nr]:])
        hyp = [ln.split(b"\t") for ln in files[1].splitlines() if b"\thypothetical protein\t" in ln]
        if write_all:
            assert len(hyp) == len(orfs) - nr and sum(f[10] == b"noncoding" for f in hyp) == dropped
            assert all((f[10] == b"noncoding") == (b"noncoding" in f[9].split(b",")) == (int(f[12]) < 0) for f in hyp)
        else:
            assert len(hyp) == int((sel["state"][nr:] == 1).sum()) and all(int(f[10]) >= 0 and b"noncoding" not in f[9] for f in hyp)
        Cc, Bb = CR.parse_coding_model(open(model, "rb").read())
        assert Cc.tobytes() == counts[0].tobytes() and Bb.tobytes() == counts[1].tobytes()
    # without --coding: the bytes the writers gave before
    regs, start, orfs0, ps, res, sel0 = plain[True]
    nr = len(regs)
    line0, files0, _ = run("plain", "--select", "--free-orfs")
    assert line0 == CR.summary_of(regs, start) + CR.orf_summary(orfs0[:nr]) + CR.select_summary(sel0) + ", free: %d" % (len(orfs0) - nr)
    assert files0[0] == CR.format_regions(ids, regs, fnames, sel=sel0[:nr], cands=orfs0)
    assert files0[1] == CR.format_orfs(ids, regs, orfs0[:nr], fnames, sel=sel0[:nr], free=orfs0[nr:], free_sel=sel0[nr:], cands=orfs0)
    assert files0[2] == CR.format_faa(ids, regs, orfs0[:nr], ps[:nr + 1], res[:ps[nr]], fnames, sel=sel0[:nr], free=orfs0[nr:], free_sel=sel0[nr:],
                                      free_prot_start=ps[nr:] - ps[nr], free_residues=res[ps[nr]:])
    # ... and, independent of the writers under test, the bytes recorded from the writers before this option existed
    TH.same_as_recorded("written_select", files0)
    p = subprocess.run(base + ["-o", str(tmp_path / "x.tsv"), "--coding"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode != 0 and "--coding" in p.stderr


# ---- E. coli: a finding, not a threshold ------------------------------------------------------------------------------------------------

def test_ecoli_genome_equals_the_model_and_what_the_filter_drops():
    """The genome's free ORFs of 100 residues, scored with a model trained on its own six-frame ORFs of 300 residues (a stand-in
    for evidence ORFs: the fixture has no table).  Counts, scores and records equal the model; how many free ORFs go, and how
    many of them end in the last 30 residues of a protein of the .faa fixture, is printed and recorded in DESIGN.md 9k."""
    from kmergutsjava_amd import hotpath
    from kmergutsjava_amd.make_signatures import parse_fasta
    _, contigs = parse_fasta(gzip.decompress(open(os.path.join(HERE, "golden", "Ecoli_K12_W3110.fna.gz"), "rb").read()))
    _, prots = parse_fasta(gzip.decompress(open(os.path.join(HERE, "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))
    seq, off = _batch(contigs)
    free = F.free_orfs(seq, off)
    train = free[0][free[0]["n_res"] >= 300].copy()
    train["flags"] &= ~np.uint32(K.FREE)
    Cd, Bd = hotpath.coding_counts(train, seq, off)
    Cm, Bm = K.counts_np(train, seq, off)
    assert Cd.tobytes() == Cm.tobytes() and Bd.tobytes() == Bm.tobytes()
    T = hotpath.coding_table(Cd, Bd)
    assert T.tobytes() == K.table(Cm, Bm).tobytes()
    s = _Set(np.zeros(0, N.REGION_DTYPE), seq, off, min_res=100)
    try:
        assert s.records.tobytes() == free[0].tobytes()
        got = s.coding(T)
        want = K.coding(free[0], seq, off, T)
        _same_as_model(got, want)
    finally:
        s.close()
    tails = {p[-30:] for p in prots if len(p) >= 30}
    rb, ps = free[2].tobytes(), free[1]
    known = np.array([rb[ps[i + 1] - 30:ps[i + 1]] in tails for i in range(len(free[0]))])
    dropped = (got[0]["flags"] & K.NONCODING) != 0
    print("E. coli: %d nt, %d training pairs, %d free ORFs of 100 residues; %d end in a known protein, %d of them dropped; %d do not, "
          "%d of them dropped" % (len(seq), Cm.sum(), len(known), known.sum(), (known & dropped).sum(), (~known).sum(), (~known & dropped).sum()))
    assert dropped.sum() == got[2]["noncoding"] == (want[1] < 0).sum()
