"""Start codons on the GPU (kg_orfset_starts, kg_starts_orfs): records, shifts, counts, statistics, proteins and coding scores
must equal the model of tests/starts_model.py byte for byte -- for records of 1, 2 and 3 residues, candidate counts at the wave
and workgroup sizes, one ORF of 10^4 ATG codons among short ones, suffix sums beyond 32 bits across the chunk borders of the
codon passes (_native.START_CHUNK), the six containers with a contig's first and last codon, windows that leave the contig,
unknown bases, the masks, the min_res bound, limits, the region-set form, non-movable records, rounds, the training threshold,
caller's weights, a second call, the selection behind it, batch neighbours, the errors, failed allocations, host and device
bytes, the call_regions front end and the E. coli genome.

Two of the errors the header names are not provoked here, as in tests/test_gpu_coding.py.  KG_ERR_BUSY: no hook leaves a
kg_scan* in flight on a table without a second thread, and the call takes the set's table through the CallScope every other set
call uses.  KG_ERR_LIMIT for 2^31 records or 2^40 bytes: neither fits a test of a few seconds.

The 2^32-codon limit does, since the records of a caller's list may overlap: 2048 movable records over one frame of 2^21 codons
hold 2^32 codons and fill one chunk of the prefix sum (tests/scan_model.py); the codon total is read on the host before any
codon pass is launched.  kg_orfset_starts lays the proteins out again without a limit of its own: no record grows, which
test_a_set_non_movable_records_proteins_scores_and_a_second_call asserts."""
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
import starts_model as M  # noqa: E402
import test_coding_host as TH  # noqa: E402
import test_orfs_host as HO  # noqa: E402
import test_starts_host as SH  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CHUNK = N.START_CHUNK


def _check(orfs, seq, off, T, weights=None, limits=None, **kw):
    """kg_starts_orfs against the numpy model -> the model's result."""
    from kmergutsjava_amd import hotpath
    st, model = {}, []
    got = hotpath.choose_starts(T, orfs, seq, off, weights, limits, stats=st, model=model, **kw)
    want = M.starts(orfs, seq, off, T, weights, limits, **kw)
    assert got[0].dtype == want["orfs"].dtype and got[0].tobytes() == want["orfs"].tobytes(), "records"
    assert got[1].dtype == want["shifts"].dtype and got[1].tobytes() == want["shifts"].tobytes(), "shifts"
    assert {k: v for k, v in st.items() if not k.startswith("ms_")} == want["stats"], (st, want["stats"])
    for name, a, b in zip(("chosen", "cand", "type_chosen", "type_cand"), model, want["model"]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    return want


def _table(rng):
    return rng.integers(-3000, 3000, size=K.BINS).astype(np.int32)


# ---- caller-held lists: the kernels ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
def test_residues_1_2_3_and_candidate_counts_at_wave_and_workgroup_sizes(strand):
    """Records of 1, 2 and 3 residues, and records with 0 (not movable), 1, 63, 64, 65, 255, 256 and 257 candidates, so that the
    compaction and the per-record maximum meet the wave and workgroup borders at every offset."""
    rng = np.random.default_rng(21 + strand)
    genes = [SH.gene(rng, n, {0: b"ATG"}, strand=strand, frame=n % 3) for n in (1, 2, 3)]
    for c in (0, 1, 63, 64, 65, 255, 256, 257):
        at = {int(k): (b"ATG", b"GTG", b"TTG")[int(k) % 3] for k in rng.choice(np.arange(1, c + 40), size=max(c - 1, 0), replace=False)}
        at[0] = b"ATG"
        genes.append(SH.gene(rng, c + 45, at, strand=strand, frame=c % 3, kept=int(c != 0), random_codons=True))
    orfs, seq, off = SH.batch(genes)
    T = _table(rng)
    for rounds in (1, 4):
        want = _check(orfs, seq, off, T, min_res=1, rounds=rounds, min_train_starts=1)
        assert want["stats"]["candidates"] == 3 + 1 + 63 + 64 + 65 + 255 + 256 + 257 and want["stats"]["movable"] == 10
        assert want["stats"]["moved"] >= 3 and not want["shifts"][:4].any()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_orf_of_10000_atg_codons_among_2000_of_100(where):
    """Every codon of the long ORF is a candidate, every window is ATGATG..., all scores tie away from the ends: with a table
    of zeros and weights of zeros the answer is the smallest k, 0; with a table that pays for ATGATG it is the largest k that
    K allows -- one maximum among 10^4 lanes."""
    rng = np.random.default_rng(5)
    genes = [SH.gene(rng, 100, {0: b"ATG", int(rng.integers(1, 60)): b"GTG"}, strand=int(rng.integers(0, 2)), frame=int(rng.integers(0, 3)),
                     flags=int(rng.choice([1, 17]))) for _ in range(2000)]
    long_one = SH.gene(rng, 10000, {k: b"ATG" for k in range(10000)}, strand=1, frame=1, up=b"ATG" * 10)
    genes.insert({"first": 0, "middle": 1000, "last": 2000}[where], long_one)
    orfs, seq, off = SH.batch(genes)
    i = {"first": 0, "middle": 1000, "last": 2000}[where]
    zero = (np.zeros((20, 4), np.int32), np.zeros(4, np.int32))
    want = _check(orfs, seq, off, np.zeros(K.BINS, np.int32), zero, min_res=1)
    assert want["stats"]["candidates"] >= 10000 + 2000 and not want["shifts"].any()
    T = np.zeros(K.BINS, np.int32)
    T[int("032032", 4)] = -7                            # ATGATG: the shorter the ORF, the better
    want = _check(orfs, seq, off, T, zero, min_res=100)
    assert want["shifts"][i] == 9900
    want = _check(orfs, seq, off, T, None, min_res=100, rounds=2, min_train_starts=10)
    assert want["stats"]["trained"] == 1 and want["shifts"][i] > 0


def test_suffix_sums_beyond_32_bits_across_every_chunk_border():
    """A table of any int32 values, both ends of the range: records whose codon lists end just before, at and just behind the
    borders of the codon passes' workgroups, so that a record's sum is the difference of carries of other chunks."""
    rng = np.random.default_rng(8)
    T = rng.choice(np.array([-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 0, 12345], dtype=np.int64), size=K.BINS).astype(np.int32)
    genes = []
    for n in (CHUNK - 1, 1, CHUNK, 2, CHUNK + 1, 3 * CHUNK - 7, 5, CHUNK // 4, 64, 63, 2 * CHUNK):
        at = {int(k): b"ATG" for k in rng.choice(np.arange(1, n), size=min(n - 1, 12), replace=False)} if n > 1 else {}
        at[0] = b"TTG"
        genes.append(SH.gene(rng, n, at, strand=len(genes) % 2, frame=len(genes) % 3, random_codons=True))
    orfs, seq, off = SH.batch(genes)
    zero = (np.zeros((20, 4), np.int32), np.zeros(4, np.int32))
    want = _check(orfs, seq, off, T, zero, min_res=1)
    sums = K.scores_np(T, orfs, seq, off)
    assert (np.abs(sums) > 2 ** 33).sum() >= 3 and want["stats"]["moved"] >= 5
    _check(orfs, seq, off, T, None, min_res=1, rounds=3, min_train_starts=1)
    # the largest sums a table can give: every pair at one end of the range
    for v in (-2 ** 31, 2 ** 31 - 1):
        _check(orfs, seq, off, np.full(K.BINS, v, dtype=np.int32), zero, min_res=1)


def test_six_containers_first_and_last_codon_and_windows_off_the_contig():
    """A record on the contig's first codon (its window leaves the contig: off the start on '+', off the end on '-'), one whose
    stop codon is the contig's last, for both strands, every frame and L mod 3 = 0, 1, 2; a contig alone gives the same records
    as among neighbours."""
    rng = np.random.default_rng(9)
    genes = []
    for strand in (0, 1):
        for f in (0, 1, 2):
            for up_codons in (0, 1, 6, 7):          # 0 to 21 window positions inside the contig
                genes.append(SH.gene(rng, 30, {0: b"GTG", 4: b"ATG", 9: b"TTG", 20: b"ATG"}, strand=strand, up=3 * up_codons + f, down=(len(genes) % 3),
                                     random_codons=True))
    orfs, seq, off = SH.batch(genes)
    assert set((np.diff(off) % 3).tolist()) == {0, 1, 2}
    W = (rng.integers(-400, 400, size=(20, 4)).astype(np.int32), rng.integers(-400, 400, size=4).astype(np.int32))
    T = _table(rng)
    want = _check(orfs, seq, off, T, W, min_res=3)
    assert 0 < want["stats"]["moved"] < len(orfs)
    _check(orfs, seq, off, T, None, min_res=3, rounds=4, min_train_starts=1)
    for i in (0, 7, len(genes) - 1):                    # alone: the neighbours' bytes are not in the window
        one = orfs[i:i + 1].copy()
        one["seq"] = 0
        alone = _check(one, seq[off[i]:off[i + 1]], np.array([0, off[i + 1] - off[i]], np.int64), T, W, min_res=3)
        assert alone["shifts"][0] == want["shifts"][i]


def test_unknown_bases_u_and_lower_case_in_the_window_and_in_a_candidate():
    rng = np.random.default_rng(10)
    genes = []
    for strand in (0, 1):
        for spell in (b"ATG", b"atg", b"AUG", b"aug", b"ANG", b"A-G", b"NTG", b"gUG", b"uuG"):
            genes.append(SH.gene(rng, 40, {0: b"ATG", 10: spell, 20: b"GTG"}, strand=strand, frame=len(genes) % 3,
                                 up=b"acgunNACGU-TtGgCcAaUuN-acgtACGTNN", random_codons=True, unknowns=0.05))
    orfs, seq, off = SH.batch(genes)
    W = (rng.integers(-400, 400, size=(20, 4)).astype(np.int32), rng.integers(-400, 400, size=4).astype(np.int32))
    want = _check(orfs, seq, off, _table(rng), W, min_res=3)
    assert want["stats"]["candidates"] >= 2 * (3 * 6 + 2 * 3) and want["stats"]["moved"] > 0
    _check(orfs, seq, off, _table(rng), None, min_res=3, rounds=2, min_train_starts=1)


def test_masks_the_min_res_bound_and_limits():
    rng = np.random.default_rng(12)
    genes = [SH.gene(rng, 60, {0: (b"ATG", b"GTG", b"TTG")[g % 3], 10: b"ATG", 20: b"GTG", 30: b"TTG", 40: b"ATG"}, strand=g % 2, frame=g % 3)
             for g in range(12)]
    orfs, seq, off = SH.batch(genes)
    T = np.zeros(K.BINS, np.int32)
    # weights that pay for the position behind: the chosen k is the largest candidate
    W = (np.zeros((20, 4), np.int32), np.array([0, 5, 7, 9], np.int32))
    T[:] = -1
    want = {m: _check(orfs, seq, off, T, W, min_res=1, start_codons=m)["shifts"] for m in (1, 2, 4, 7, 0)}
    assert set(want[1]) == {40} and set(want[2]) == {20} and set(want[4]) == {30} and set(want[7]) == {40} and set(want[0]) == {0}
    # K = n_res - min_res exactly at a candidate and one beyond it
    assert set(_check(orfs, seq, off, T, W, min_res=20)["shifts"]) == {40}
    assert set(_check(orfs, seq, off, T, W, min_res=21)["shifts"]) == {30}
    assert set(_check(orfs, seq, off, T, W, min_res=61)["shifts"]) == {0}
    # limits: 0, at a candidate, one below a candidate, none
    lim = np.array([0, 20, 19, -1] * 3, dtype=np.int32)
    got = _check(orfs, seq, off, T, W, lim, min_res=1)["shifts"]
    assert got.tolist() == [0, 20, 10, 40] * 3


def test_rounds_the_training_threshold_and_callers_weights():
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(13)
    orfs, seq, off = SH.sd_genes(rng, 300)
    T = _table(rng)
    n_train = int(sum(M.is_training(o) for o in orfs))
    r1 = _check(orfs, seq, off, T, None, min_res=10, rounds=1, min_train_starts=n_train)
    r4 = _check(orfs, seq, off, T, None, min_res=10, rounds=4, min_train_starts=n_train)
    assert r1["stats"]["trained"] == r4["stats"]["trained"] == 1 and r4["stats"]["rounds_run"] == 4
    assert r1["shifts"].tobytes() != r4["shifts"].tobytes() and r4["stats"]["moved"] > 50
    un = _check(orfs, seq, off, T, None, min_res=10, rounds=4, min_train_starts=n_train + 1)
    assert un["stats"]["trained"] == 0 and not un["shifts"].any() and un["orfs"].tobytes() == orfs.tobytes()
    # the last round's weights given by the caller choose what the last round chose
    chosen, cand, tc, td = hotpath.start_counts(T, orfs, seq, off, min_res=10, rounds=4)
    assert chosen.tobytes() == r4["model"][0].tobytes() and cand.tobytes() == r4["model"][1].tobytes()
    W = hotpath.start_weights(chosen, cand, tc, td)
    wm = M.weights_from(chosen, cand, tc, td)
    assert W[0].tobytes() == wm[0].tobytes() and W[1].tobytes() == wm[1].tobytes()
    cw = _check(orfs, seq, off, T, W, min_res=10)
    assert cw["stats"]["trained"] == 2 and cw["stats"]["rounds_run"] == 1 and cw["shifts"].tobytes() == r4["shifts"].tobytes()
    # a second call on its own output
    again = _check(r4["orfs"], seq, off, T, W, min_res=10)
    assert (again["orfs"]["flags"] & M.MOVED).sum() >= (r4["orfs"]["flags"] & M.MOVED).sum()


def test_codon_totals_that_wrap_a_chunk_of_the_prefix_sum_are_refused():
    """The lists of scan_model.families through kg_starts_orfs.  starts_lens_kernel gives a movable record its n_res codons and
    any other record none; kcap, min_res and the limits bound the candidates among them, not the codons.  So the long record, the
    2^21 sense codons of the long contig with a start codon on record, has 2^21, the short one six, and a record that is not
    kept none: 2048 long ones alone, behind 2048 short ones, in reversed order, and -- the control, refused whatever the chunk
    sums' width -- half in each of two chunks.  tests/test_scan_model_host.py shows that 32-bit chunk sums gave the first
    three a total below 2^32.  Every call is refused with the stage's own words, leaves no device memory behind, and the next
    call is an ordinary one."""
    import torch
    from kmergutsjava_amd import hotpath
    seq, off = SM.limit_batch(SM.LONG)
    right = 3 * (SM.LONG + 1) - 1                       # the stop codon inside the coordinates
    long_row, short_row = K.orf(1, 0, 0, right, SM.LONG, start_codon=1), K.orf(0, 0, 3, 3 + 3 * 7 - 1, 6, start_codon=1)
    none_row = K.orf(1, 0, 0, right, SM.LONG, start_codon=1, kept=0)
    rng = np.random.default_rng(17)
    T = _table(rng)
    genes = [SH.gene(rng, n, {0: b"ATG", 3: b"GTG", 7: b"TTG"}, strand=n % 2, frame=n % 3, random_codons=True) for n in (30, 41, 52, 9)]
    small, small_seq, small_off = SH.batch(genes)
    kw = dict(min_res=5, rounds=2, min_train_starts=1)
    with hotpath.SignatureTable.from_bytes(_workload()[0], 0) as tab:
        _check(small, small_seq, small_off, T, **kw)    # once first: what the runtime sets up on first use is not counted
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        for name, (lens, _) in SM.families(6).items():
            orfs = SM.records_of(lens, long_row, short_row, none_row, N.ORF_DTYPE)
            assert np.where(orfs["kept"] != 0, orfs["n_res"], 0).tolist() == lens.tolist() and SM.scan_exact(lens)[1] >= SM.LIMIT
            with pytest.raises(N.KmerGutsNativeError) as ei:
                hotpath.choose_starts(T, orfs, seq, off, min_res=100)
            assert ei.value.code == N.KG_ERR_LIMIT, name
            assert SM.message_of(ei.value).startswith("2^32 or more codons"), (name, str(ei.value))
            assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0, name
        want = _check(small, small_seq, small_off, T, **kw)
        assert want["stats"]["movable"] == 4


# ---- sets: kg_orfset_starts -----------------------------------------------------------------------------------------------------------

class _Set:
    """An ORF set of caller-held regions and the batch's free ORFs with coding scores, and kg_orfset_starts on it."""

    def __init__(self, regs, seq, off, T, min_res=30, only_kept=0):
        self.lib, self.seq, self.off = N.load(), np.ascontiguousarray(seq), np.ascontiguousarray(off)
        self.T = np.ascontiguousarray(T, dtype=np.int32)
        self.hs = []
        batch = (self.seq.ctypes.data, 0, self.off.ctypes.data, len(off) - 1)
        h = C.c_void_p()
        N.check(self.lib.kg_orfs_regions(0, C.byref(N.KgOrfParams(7, only_kept, 0)), regs.ctypes.data if len(regs) else None, len(regs),
                                         self.seq.ctypes.data, self.off.ctypes.data, len(off) - 1, C.byref(h)))
        self.hs.append(h)
        try:
            for call, prm in ((self.lib.kg_orfset_add_free, (C.byref(N.KgFreeParams(min_res, 7, 0)),)),
                              (self.lib.kg_orfset_coding, (C.byref(N.KgCodingParams(0, 0, 0)), self.T.ctypes.data))):
                new = C.c_void_p()
                N.check(call(self.hs[-1], *prm, *batch, C.byref(new)))
                self.hs.append(new)
        except BaseException:
            self.close()
            raise
        self.h = self.hs[-1]
        self.records, self.scores, self.ps, self.res = self.read(self.h)

    def read(self, h):
        n = int(self.lib.kg_orfset_count(h))
        recs, scores, ps = np.zeros(n, dtype=N.ORF_DTYPE), np.zeros(n, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        N.check(self.lib.kg_orfset_copy(h, 0, n, recs.ctypes.data if n else None))
        N.check(self.lib.kg_orfset_coding_scores(h, 0, n, scores.ctypes.data if n else None))
        N.check(self.lib.kg_orfset_prot_start(h, ps.ctypes.data))
        res = np.zeros(int(ps[-1]), dtype=np.uint8)
        N.check(self.lib.kg_orfset_residues(h, 0, len(res), res.ctypes.data if len(res) else None))
        return recs, scores, ps, res

    def starts(self, weights=None, of=None, select=False, keep=False, **kw):
        """-> the new set as the model's dict[, the selection]; the new set is freed unless `keep`."""
        from kmergutsjava_amd import hotpath
        p = N.KgStartParams(kw.get("min_res", 100), kw.get("start_codons", 7), kw.get("rounds", 4), 0, kw.get("min_train_starts", 200))
        w = None if weights is None else hotpath._weights_arg(weights)
        new = C.c_void_p()
        N.check(self.lib.kg_orfset_starts(of or self.h, C.byref(p), self.T.ctypes.data, None if w is None else C.addressof(w), None,
                                          self.seq.ctypes.data, 0, self.off.ctypes.data, len(self.off) - 1, C.byref(new)))
        try:
            recs, scores, ps, res = self.read(new)
            shifts, st, model = hotpath._starts_results(new)
            out = {"orfs": recs, "shifts": shifts, "stats": {k: v for k, v in st.items() if not k.startswith("ms_")}, "model": model,
                   "prot_start": ps, "residues": res, "scores": scores}
            if select:
                sh = C.c_void_p()
                N.check(self.lib.kg_orfset_select(new, C.byref(N.KgSelectParams(60, 50, 0)), C.byref(sh)))
                out["selection"] = hotpath._take_selectset(sh, False)[0]
        except BaseException:
            self.lib.kg_orfset_free(new)
            raise
        if keep:
            self.hs.append(new)
            out["handle"] = new
        else:
            self.lib.kg_orfset_free(new)
        return out

    def close(self):
        for h in reversed(self.hs):
            self.lib.kg_orfset_free(h)
        self.hs = []


def _same_as_model(got, want):
    for key in ("orfs", "shifts", "prot_start", "residues", "scores"):
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    for a, b in zip(got["model"], want["model"]):
        assert a.tobytes() == b.tobytes(), "counts"


def _model(s, recs=None, scores=None, ps=None, res=None, weights=None, **kw):
    recs = s.records if recs is None else recs
    return M.starts(recs, s.seq, s.off, s.T, weights, None, prot_start=s.ps if ps is None else ps, residues=s.res if res is None else res,
                    scores=s.scores if scores is None else scores, **kw)


def test_a_set_non_movable_records_proteins_scores_and_a_second_call():
    """30 random contigs with regions (some not kept, multi-frame, interrupted, without a start) and free ORFs of 30 residues,
    only_kept zero lengths among them; no region set is given, so min_res bounds every record."""
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(5)
    w = np.array([4, 44, 44, 4, 0, 1, 1, 1, 0, 1, 0], float) / 100
    regs, seq, off = O.random_batch(rng, 30, max_len=2500, max_regions=6, weights=w)
    s = _Set(regs, seq, off, _table(rng), only_kept=1)
    try:
        recs = s.records
        kw = dict(min_res=20, rounds=4, min_train_starts=3)
        want = _model(s, **kw)
        got = s.starts(keep=True, **kw)
        _same_as_model(got, want)
        moved = got["shifts"] > 0
        assert want["stats"]["trained"] == 1 and moved.sum() > 10 and (recs["kept"] == 0).any() and (np.diff(s.ps) == 0).any()
        # non-movable records: not kept, no start, interrupted, non-coding -- unchanged, shift 0
        fixed = (recs["kept"] == 0) | (recs["start_codon"] == 0) | ((recs["flags"] & (M.INTERRUPTED | M.NONCODING)) != 0)
        assert fixed.sum() > 5 and got["orfs"][fixed].tobytes() == recs[fixed].tobytes() and not got["shifts"][fixed].any()
        assert ((got["orfs"]["flags"] & M.MOVED) != 0).tolist() == moved.tolist() and (got["orfs"]["first_inner"][moved] == -1).all()
        # no record grows, so the new set needs no residue limit of its own: record by record and in all, it holds no more
        # residues than the given set, whose total passed the 2^32 limit when it was made
        assert (np.diff(got["prot_start"]) <= np.diff(s.ps)).all() and len(got["residues"]) < len(s.res)
        # proteins: the old suffix with M; the scores: a fresh coding_scores of the new records
        for i in np.flatnonzero(moved)[:20]:
            old = s.res[s.ps[i]:s.ps[i + 1]].tobytes()
            assert got["residues"][got["prot_start"][i]:got["prot_start"][i + 1]].tobytes() == b"M" + old[got["shifts"][i] + 1:]
        assert got["scores"].tobytes() == hotpath.coding_scores(s.T, got["orfs"], seq, off).tobytes()
        # the given set is unchanged; a second call on the output equals the model on the output
        assert s.read(s.h)[0].tobytes() == recs.tobytes()
        again = s.starts(of=got["handle"], **kw)
        _same_as_model(again, _model(s, got["orfs"], got["scores"], got["prot_start"], got["residues"], **kw))
        # untrained: min_train_starts - 1 against min_train_starts
        nt = want["stats"]["training_records"]
        un = s.starts(min_res=20, min_train_starts=nt + 1)
        _same_as_model(un, _model(s, min_res=20, min_train_starts=nt + 1))
        assert un["stats"]["trained"] == 0 and un["orfs"].tobytes() == recs.tobytes() and un["residues"].tobytes() == s.res.tobytes()
        assert s.starts(min_res=20, min_train_starts=nt)["stats"]["trained"] == 1
    finally:
        s.close()


def test_an_orf_shortened_out_of_a_conflict_no_longer_loses():
    regs, seq, off, W = SH.conflict_case()
    s = _Set(regs, seq, off, np.zeros(K.BINS, np.int32), min_res=10 ** 6)       # (no free ORF is that long)
    try:
        assert len(s.records) == 2
        before = S.select_fast(S.of_records(s.records))
        got = s.starts(W, select=True, min_res=30)
        want = _model(s, weights=W, min_res=30)
        _same_as_model(got, want)
        after = S.select_fast(S.of_records(want["orfs"]))
        assert got["selection"].tobytes() == after.tobytes()
        assert before["state"].tolist() == [1, 2] and after["state"].tolist() == [1, 1] and got["shifts"].tolist() == [0, 60]
    finally:
        s.close()


def test_errors_and_their_messages():
    from kmergutsjava_amd import hotpath
    lib = N.load()
    rng = np.random.default_rng(3)
    orfs, seq, off = SH.batch([SH.gene(rng, 40, {0: b"ATG", 9: b"GTG"}, strand=g % 2) for g in range(4)])
    T = _table(rng)

    def fails(code, word, **kw):
        args = dict(table=T, orfs=orfs, seq=seq, offsets=off)
        args.update(kw)
        with pytest.raises(N.KmerGutsNativeError) as ei:
            hotpath.choose_starts(args.pop("table"), args.pop("orfs"), args.pop("seq"), args.pop("offsets"), **args)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    fails(N.KG_ERR_ARG, "min_res", min_res=0)
    fails(N.KG_ERR_ARG, "start_codons", start_codons=8)
    fails(N.KG_ERR_ARG, "rounds", rounds=0)
    fails(N.KG_ERR_ARG, "rounds", rounds=17)
    fails(N.KG_ERR_ARG, "min_train_starts", min_train_starts=-1)
    for field, value, word in (("seq", 4, "record 2: seq"), ("strand", 2, "record 2: strand"), ("right", 10 ** 6, "record 2: outside"),
                               ("n_res", 10 ** 5, "record 2: 3 * n_res")):
        bad = orfs.copy()
        bad[field][2:] = value
        fails(N.KG_ERR_ARG, word, orfs=bad)
    p = N.KgStartParams(100, 7, 4, 0, 200)
    out, sh = np.zeros(4, N.ORF_DTYPE), np.zeros(4, np.int32)
    rest = (orfs.ctypes.data, 4, None, seq.ctypes.data, off.ctypes.data, 4, out.ctypes.data, sh.ctypes.data, None, None)
    assert lib.kg_starts_orfs(0, C.byref(p), None, None, *rest) == N.KG_ERR_ARG and b"coding table" in lib.kg_last_error()
    assert lib.kg_starts_orfs(0, None, T.ctypes.data, None, *rest) == N.KG_ERR_ARG
    p.reserved = 1
    assert lib.kg_starts_orfs(0, C.byref(p), T.ctypes.data, None, *rest) == N.KG_ERR_ARG and b"reserved" in lib.kg_last_error()
    with pytest.raises(ValueError):
        hotpath.choose_starts(T, orfs, seq, off, weights=(np.zeros((20, 3)), np.zeros(4)))
    with pytest.raises(ValueError):
        hotpath.choose_starts(T, orfs, seq, off, limits=np.zeros(3, np.int32))
    # a set: the getters on a set without shifts, n_seqs, a null table
    s = _Set(np.zeros(0, N.REGION_DTYPE), seq, off, T, min_res=30)
    try:
        buf = np.zeros(64, np.int32)
        assert lib.kg_orfset_start_shifts(s.h, 0, 0, buf.ctypes.data) == N.KG_ERR_ARG and b"not from kg_orfset_starts" in lib.kg_last_error()
        assert lib.kg_orfset_start_stats(s.h, C.byref(N.KgStartStats())) == N.KG_ERR_ARG
        assert lib.kg_orfset_start_model(s.h, C.byref(N.KgStartModel())) == N.KG_ERR_ARG
        new, p = C.c_void_p(), N.KgStartParams(100, 7, 4, 0, 200)
        assert lib.kg_orfset_starts(s.h, C.byref(p), T.ctypes.data, None, None, seq.ctypes.data, 0, off.ctypes.data, 3,
                                    C.byref(new)) == N.KG_ERR_ARG and b"n_seqs" in lib.kg_last_error() and not new.value
        assert lib.kg_orfset_starts(s.h, C.byref(p), None, None, None, seq.ctypes.data, 0, off.ctypes.data, 4,
                                    C.byref(new)) == N.KG_ERR_ARG and b"coding table" in lib.kg_last_error()
        got = s.starts(keep=True, min_res=30)
        n = len(got["orfs"])
        assert lib.kg_orfset_start_shifts(got["handle"], 0, n + 1, buf.ctypes.data) == N.KG_ERR_ARG and b"range" in lib.kg_last_error()
    finally:
        s.close()


# ---- behind a scan ----------------------------------------------------------------------------------------------------------------------

_WORK = {}


def _workload():
    if not _WORK:
        _WORK["w"] = HO.planted_orf_contigs()
    return _WORK["w"]


def test_behind_a_scan_the_region_limits_from_host_and_device_bytes():
    """ScanResult.orfs / select with starts=: the region-set form of rule 3 against the model's limits and against the
    explicit-limit twin, from host bytes and from device bytes."""
    import torch
    from kmergutsjava_amd import hotpath
    img, dna, off, genes = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    d_seq = torch.from_numpy(sb.copy()).cuda()
    torch.cuda.synchronize()
    kw = dict(free_min_res=100, coding=True, min_train_pairs=1000)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        live0 = tab.live_device_bytes()
        for ptr in (None, d_seq.data_ptr()):
            with tab.scan(None if ptr else sb, off, hotpath.Params(min_hits=4), device_ptr=ptr) as r:
                live1 = tab.live_device_bytes()
                plain = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, **kw)
                scores0, T = r.coding_scores.copy(), hotpath.coding_table(*r.coding_model)
                got = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, starts=True, min_train_starts=50, **kw)
                lim = M.region_limits(plain[2], plain[0], off)
                want = M.starts(plain[2], dna, off, T, None, lim, min_train_starts=50, prot_start=plain[3], residues=plain[4], scores=scores0)
                st = {k: v for k, v in r.start_stats.items() if not k.startswith("ms_")}
                _same_as_model({"orfs": got[2], "shifts": r.start_shifts, "prot_start": got[3], "residues": got[4], "scores": r.coding_scores,
                                "stats": st, "model": r.start_model}, want)
                assert st["trained"] == 1 and st["training_records"] >= 50 and st["moved"] > 0 and (lim[:len(plain[0])] >= 0).all()
                assert r.start_stats["ms_count"] > 0 and r.start_stats["ms_choose"] > 0 and tab.live_device_bytes() == live1
                twin = hotpath.choose_starts(T, plain[2], dna, off, limits=lim, min_train_starts=50)
                assert twin[0].tobytes() == got[2].tobytes() and twin[1].tobytes() == r.start_shifts.tobytes()
                sel = r.select(off, None if ptr else sb, 300, 12, 100, orfs=True, device_ptr=ptr, starts=True, min_train_starts=50, **kw)
                assert sel[2].tobytes() == want["orfs"].tobytes() and sel[5].tobytes() == S.select_fast(S.of_records(want["orfs"])).tobytes()
                # caller's weights; an untrained coding step leaves the starts untrained
                W = hotpath.start_weights(*r.start_model)
                with_w = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, starts=W, **kw)
                assert with_w[2].tobytes() == want["orfs"].tobytes() and r.start_stats["trained"] == 2
                un = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, starts=True, min_train_starts=1, free_min_res=100,
                            coding=True, min_train_pairs=10 ** 9)
                assert r.start_stats["trained"] == 0 and not r.start_shifts.any() and tab.live_device_bytes() == live1
                with pytest.raises(ValueError):
                    r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, free_min_res=100, starts=True)
                with pytest.raises(ValueError):
                    r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, starts=(np.zeros(3), np.zeros(4)), **kw)
                assert tab.live_device_bytes() == live1
                off_run = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, starts=False, **kw)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(off_run, plain))
        assert tab.live_device_bytes() == live0


def test_a_region_that_does_not_fit_its_record_is_an_error():
    lib = N.load()
    img, dna, off, genes = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    from kmergutsjava_amd import hotpath
    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(sb, off, hotpath.Params(min_hits=4)) as r:
        rh, oh, new = C.c_void_p(), C.c_void_p(), C.c_void_p()
        batch = (sb.ctypes.data, 0, off.ctypes.data, len(off) - 1)
        N.check(lib.kg_result_regions(r._h, C.byref(N.KgRegionParams(300, 12, 100)), off.ctypes.data, C.byref(rh)))
        try:
            # the free ORFs alone are not index-aligned with the regions
            N.check(lib.kg_orfs_free(0, C.byref(N.KgFreeParams(100, 7, 0)), *batch, C.byref(oh)))
            p, T = N.KgStartParams(100, 7, 4, 0, 50), np.zeros(K.BINS, np.int32)
            rc = lib.kg_orfset_starts(oh, C.byref(p), T.ctypes.data, None, rh, *batch, C.byref(new))
            assert rc == N.KG_ERR_ARG and not new.value and b": its region has another seq or strand" in lib.kg_last_error(), lib.kg_last_error()
        finally:
            lib.kg_orfset_free(oh)
            lib.kg_regionset_free(rh)


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    """Every allocation of the two calls fails once.  The set call runs beside an open table, on an ORF set made from a scan of
    it: after every failure the table's live bytes are what they were, and 0 when the sets and the result are freed."""
    import torch
    from kmergutsjava_amd import hotpath
    lib = N.load()
    rng = np.random.default_rng(4)
    orfs, seq, off = SH.sd_genes(rng, 60)
    T = _table(rng)
    kw = dict(min_res=10, rounds=2, min_train_starts=5)
    want = M.starts(orfs, seq, off, T, **kw)
    hotpath.choose_starts(T, orfs, seq, off, **kw)      # once first: what the runtime sets up on first use is not counted
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    failed = 0
    for n in range(1, 80):
        monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
        try:
            got = hotpath.choose_starts(T, orfs, seq, off, **kw)
            break
        except N.KmerGutsNativeError as e:
            assert e.code == N.KG_ERR_NOMEM, e
            failed += 1
            assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
    monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
    assert failed >= 20 and got[0].tobytes() == want["orfs"].tobytes()     # records, bytes, two outputs, 7 + 15 of the passes
    img, dna, doff, _ = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        with tab.scan(sb, doff, hotpath.Params(min_hits=4)) as r:
            hs = [C.c_void_p() for _ in range(5)]
            rh, oh, fh, ch, sh = hs
            batch = (sb.ctypes.data, 0, doff.ctypes.data, len(doff) - 1)
            N.check(lib.kg_result_regions(r._h, C.byref(N.KgRegionParams(300, 12, 100)), doff.ctypes.data, C.byref(rh)))
            try:
                N.check(lib.kg_regionset_orfs(rh, C.byref(N.KgOrfParams(7, 1, 0)), *batch, C.byref(oh)))
                N.check(lib.kg_orfset_add_free(oh, C.byref(N.KgFreeParams(100, 7, 0)), *batch, C.byref(fh)))
                N.check(lib.kg_orfset_coding(fh, C.byref(N.KgCodingParams(0, 0, 1000)), None, *batch, C.byref(ch)))
                scores, _, cmodel = hotpath._coding_results(ch)
                Tc = hotpath.coding_table(*cmodel)
                live1 = tab.live_device_bytes()
                failed, p = 0, N.KgStartParams(100, 7, 4, 0, 50)
                for n in range(1, 80):
                    monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
                    rc = lib.kg_orfset_starts(ch, C.byref(p), Tc.ctypes.data, None, rh, *batch, C.byref(sh))
                    if rc == 0:
                        break
                    assert rc == N.KG_ERR_NOMEM and not sh.value and b"KG_TEST_FAIL_ALLOC" in lib.kg_last_error()
                    failed += 1
                    assert tab.live_device_bytes() == live1
                monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
                assert failed >= 25 and sh.value        # the bytes, six of the new set, 7 + 15 of the passes, the residues
                shifts, st, _ = hotpath._starts_results(sh)
                assert st["trained"] == 1 and st["moved"] == int((shifts > 0).sum()) > 0
                lib.kg_orfset_free(sh)
                sh.value = None
                assert tab.live_device_bytes() == live1
            finally:
                for h, free in ((sh, lib.kg_orfset_free), (ch, lib.kg_orfset_free), (fh, lib.kg_orfset_free), (oh, lib.kg_orfset_free),
                                (rh, lib.kg_regionset_free)):
                    if h.value:
                        free(h)
        assert tab.live_device_bytes() == 0


# ---- the front end ----------------------------------------------------------------------------------------------------------------------

def test_call_regions_starts_end_to_end(tmp_path):
    """call_regions --free-orfs --coding --starts --select --orfs --faa on the planted contigs (fewer than 200 training records:
    --min-train-starts 50): every line against the model's records through the writers (which tests/test_starts_host.py checks
    line by line, as it checks --all, --start-model, the untrained warning and the options' errors), the saved model against the
    model's counts, and without --starts the digests recorded from the writers of the commit before --starts
    (tests/golden/call_regions_planted_before_starts.json).  Two runs of the command line: each costs an interpreter's start."""
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
        plain = r.select(off, dna, 300, 12, 100, orfs=True, free_min_res=100)
    model = str(tmp_path / "start_model.txt")
    regs, start, orfs0, ps0, res0, _ = plain
    nr = len(regs)
    coded, scores0, cst, counts = K.coding(orfs0, dna, off, None, 0, 1000)
    want = M.starts(coded, dna, off, K.table(*counts), None, M.region_limits(coded, regs, off), min_train_starts=50,
                    prot_start=ps0, residues=res0, scores=scores0)
    orfs, ps, res, scores, shifts = want["orfs"], want["prot_start"], want["residues"], want["scores"], want["shifts"]
    sel = S.select_fast(S.of_records(orfs))
    dropped = int(((orfs["flags"] & K.NONCODING) != 0).sum())
    assert want["stats"]["trained"] == 1 and want["stats"]["training_records"] >= 50 and want["stats"]["moved"] > 0
    line, files, err = run("sel", "--select", "--free-orfs", "--coding", "--min-train", "1000", "--starts", "--min-train-starts", "50",
                           "--save-start-model", model)
    assert err == []
    assert line == (CR.summary_of(regs, start) + CR.orf_summary(orfs[:nr]) + CR.select_summary(sel) + ", free: %d" % (len(orfs) - nr) +
                    ", coding: own, noncoding: %d" % dropped + ", starts: own, moved: %d" % want["stats"]["moved"])
    assert files[0] == CR.format_regions(ids, regs, fnames, sel=sel[:nr], cands=orfs)
    assert files[1] == CR.format_orfs(ids, regs, orfs[:nr], fnames, False, sel[:nr], orfs[nr:], sel[nr:], orfs, scores[:nr], scores[nr:],
                                      shifts[:nr], shifts[nr:])
    assert files[2] == CR.format_faa(ids, regs, orfs[:nr], ps[:nr + 1], res[:ps[nr]], fnames, False, sel[:nr], orfs[nr:], sel[nr:],
                                     ps[nr:] - ps[nr], res[ps[nr]:])
    got_model = CR.parse_start_model(open(model, "rb").read())
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got_model, want["model"]))
    # without --starts: the bytes recorded from the writers before this option existed
    _, files0, _ = run("coding_written_select", "--select", "--free-orfs", "--coding", "--min-train", "1000")
    SH.same_as_recorded("coding_written_select", files0)


# ---- E. coli: a finding plus one condition ------------------------------------------------------------------------------------------------

def test_ecoli_genome_equals_the_model_and_more_orfs_get_the_annotated_length():
    """The genome's free ORFs of 100 residues; those of 300 residues, FREE cleared, are the training records of the coding table
    and of the start model (a stand-in for evidence ORFs: the fixture has no table).  No region set: min_res bounds every
    record.  rounds = 4.  Records, shifts, counts and weights equal the model's.  How many of the ORFs that end in a known
    protein's last 30 residues have exactly a known protein's length, before and after, is printed and recorded in DESIGN.md 9l;
    asserted is only that the count grows.  Model (the authority), 3945 such ORFs: 2656 before, see DESIGN.md 9l for after."""
    from kmergutsjava_amd import hotpath
    from kmergutsjava_amd.make_signatures import parse_fasta
    _, contigs = parse_fasta(gzip.decompress(open(os.path.join(HERE, "golden", "Ecoli_K12_W3110.fna.gz"), "rb").read()))
    _, prots = parse_fasta(gzip.decompress(open(os.path.join(HERE, "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))
    seq, off = SH.batch_of(contigs)
    free = F.free_orfs(seq, off)
    recs = free[0].copy()
    big = recs["n_res"] >= 300
    recs["flags"][big] &= ~np.uint32(K.FREE)
    T = hotpath.coding_table(*hotpath.coding_counts(recs[big], seq, off))
    st, model = {}, []
    got = hotpath.choose_starts(T, recs, seq, off, rounds=4, stats=st, model=model)
    want = M.starts(recs, seq, off, T, rounds=4)
    assert got[0].tobytes() == want["orfs"].tobytes() and got[1].tobytes() == want["shifts"].tobytes()
    assert {k: v for k, v in st.items() if not k.startswith("ms_")} == want["stats"] and st["trained"] == 1
    assert all(a.tobytes() == b.tobytes() for a, b in zip(model, want["model"]))
    Wd, Wm = hotpath.start_weights(*model), M.weights_from(*want["model"])
    assert Wd[0].tobytes() == Wm[0].tobytes() and Wd[1].tobytes() == Wm[1].tobytes()
    before, after, known = SH.annotated_lengths(prots, free, recs, got[0])
    print("E. coli: %d free ORFs of 100 residues, %d training records, %d candidates, %d moved; of %d ORFs that end in a known protein "
          "%d have a known protein's length before and %d after" % (len(recs), st["training_records"], st["candidates"], st["moved"],
                                                                    known, before, after))
    assert after > before
