"""kg_contigs_search_translated on the GPU.  The composition law: the fragments are free_orfs(start_codons=0)'s, the hit records
and paths are db.search's on the fragments' proteins, and the CALLs and call_hits are translated_model.calls_of's, each byte for
byte.  Then the flag / prefix sum / emit stage at lane and workgroup borders, the whole call against translated_model, the
planted frameshift through orfs(repair=True) and select(), device input, the room, the error words and the allocation sweep."""
import ctypes as C

import numpy as np
import pytest

import orfs_model as O
import regions_model as R
import repair_model as RP
import search_model as S
import select_model as SL
import translated_model as TM
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import synth
from test_translated_host import _contig, _frameshift_case, _protein, _revcomp

pytestmark = pytest.mark.gpu

ALPHA = "ACDEFGHIKLMNPQRSTVWY"
STOP = "TAA"


def _counts(st):
    return {k: (_counts(v) if isinstance(v, dict) else v) for k, v in st.items() if not k.startswith("ms_") and k != "db"}


def _equal(one, got):
    assert len(one) == len(got)
    for a, b in zip(one, got):
        if isinstance(a, dict):
            assert _counts(a) == _counts(b)
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _mutated(rng, prot: str, pct: int = 10) -> str:
    out = list(prot)
    for i in rng.choice(len(out), size=max(1, len(out) * pct // 100), replace=False):
        out[int(i)] = ALPHA[(ALPHA.index(out[int(i)]) + 1 + int(rng.integers(0, 19))) % 20]
    return "".join(out)


def _random_dna(rng, n: int) -> str:
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def _block(rng, prot: str, strand: int) -> str:
    dna = STOP + synth.back_translate(prot) + STOP
    return dna if strand == 0 else _revcomp(dna)


def _check(ev, db, seq, off, min_res, max_hits, target_fn, **search):
    """The composition law on one evidence; -> the model's drop counts."""
    from kmergutsjava_amd import hotpath
    frags = hotpath.free_orfs(seq, off, min_res=min_res, start_codons=0)
    _equal(frags, ev.fragments)
    recs, pstart, res = ev.fragments
    _equal(db.search(res, pstart, paths="hits", **search), ev.search)
    hits, start, paths = ev.search[:3]
    calls, call_hits, drops = TM.calls_of(recs, hits, paths, off, max_hits, target_fn)
    assert ev.calls.dtype == calls.dtype and ev.calls.tobytes() == calls.tobytes()
    assert ev.call_hits.dtype == call_hits.dtype and ev.call_hits.tobytes() == call_hits.tobytes()
    assert (np.diff(ev.calls["container"].astype(np.int64)) >= 0).all()
    st = ev.stats
    assert (st["fragments"], st["fragment_residues"], st["records"], st["calls"]) == (len(recs), len(res), len(hits), len(calls))
    assert {k: st[k] for k in TM.DROPS} == drops
    assert st["ms_total"] == pytest.approx(st["ms_fragments"] + st["ms_search"] + st["ms_calls"])
    return drops


# ---- the composition law ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    """About 30 targets (a family of near-duplicates among them) and 40 contigs of 0 to 2000 nt with genes planted from them,
    mutated at 10 %, on both strands; one contig holds a gene in each of its six containers."""
    rng = np.random.default_rng(2024)
    # the first seven are short enough to be traced under the cap the test sets; the rest are 40 to 120 residues long
    targets = [_protein(rng, 60)] + [_protein(rng, 50) for _ in range(6)] + [_protein(rng, int(n)) for n in rng.integers(40, 121, 19)]
    targets += [_mutated(rng, targets[0], 5) for _ in range(4)]               # a family: more hits than max_hits
    tseq, toff = S.batch([t.encode() for t in targets])
    contigs = [b"", b"AC", b"N" * 300]
    six = _random_dna(rng, 7)
    for strand in (0, 1):
        for k in range(3):
            six += _block(rng, _mutated(rng, targets[1 + 3 * strand + k]), strand) + _random_dna(rng, 1)
    contigs.append(six.encode())
    while len(contigs) < 40:
        dna = _random_dna(rng, int(rng.integers(0, 200)))
        while len(dna) < 1200 and rng.random() < 0.8:
            t = targets[int(rng.integers(0, len(targets)))]
            piece = t if rng.random() < 0.7 else t[:max(30, len(t) * 2 // 5)]  # a piece of a target: below with ref longer
            dna += _block(rng, _mutated(rng, piece), int(rng.integers(0, 2))) + _random_dna(rng, int(rng.integers(0, 90)))
        contigs.append(dna[:2000].encode())
    seq, off = S.batch(contigs)
    assert int(np.diff(off).max()) <= 2000 and len(contigs) == 40
    return tseq, toff, seq, off


@pytest.fixture(scope="module")
def mixed_db(mixed):
    from kmergutsjava_amd import hotpath
    with hotpath.SearchDb.build(mixed[0], mixed[1]) as db:
        yield db


@pytest.mark.parametrize("min_res", [1, 30])
@pytest.mark.parametrize("max_hits", [1, 3])
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("named", [False, True])
def test_fragments_hits_and_calls_are_those_of_the_parts(mixed, mixed_db, min_res, max_hits, filtered, named):
    tseq, toff, seq, off = mixed
    n_db = len(toff) - 1
    fn = (np.arange(n_db, dtype=np.int32) // 3 + 100) if named else None
    search = dict(ungapped={"min_score": 20}, band=16) if filtered else {}
    search["max_trace_cells"] = 70 * 70              # some boxes fit and some do not
    with mixed_db.search_contigs(seq, off, min_res=min_res, max_hits=max_hits, target_fn=fn, **search) as ev:
        drops = _check(ev, mixed_db, seq, off, min_res, max_hits, fn, **search)
        calls = ev.calls
    # the input does what it is for: every drop reason occurs, and some contig has CALLs in all six containers
    assert all(drops[k] > 0 for k in TM.DROPS), drops
    per = {}
    for c in calls["container"].astype(np.int64):
        per.setdefault(int(c) // 6, set()).add(int(c) % 6)
    assert any(len(v) == 6 for v in per.values())
    if named:
        assert set(calls["fI"].tolist()) <= set(fn.tolist()) and calls["fI"].min() >= 100


# ---- kept and dropped records across lane and workgroup borders ------------------------------------------------------------------------

def _runs_case():
    """One target per kind: `keep` (its copies are hits), `pair` and its near-duplicate (a copy gives a kept and a rank-dropped
    record), `long` (a piece of it is below).  Contigs of gene blocks, all in frame 0 of '+', so the records follow the blocks."""
    rng = np.random.default_rng(77)
    keep, pair, long_ = _protein(rng, 40), _protein(rng, 40), _protein(rng, 120)
    pair2 = pair[:11] + ("W" if pair[11] != "W" else "Y") + pair[12:]
    tseq, toff = S.batch([t.encode() for t in (keep, pair, pair2, long_)])
    kinds = []
    for k, run in enumerate((64, 1, 63, 128, 257, 2, 1, 30, 130, 3, 200, 65, 90, 5, 70, 40, 31, 20, 20, 130)):   # kept and dropped runs in turn
        kinds += ["piece" if k % 2 else "keep"] * run
    kinds += ["pair"] * 100
    blocks = {"keep": STOP + synth.back_translate(keep) + STOP, "piece": STOP + synth.back_translate(long_[:36]) + STOP,
              "pair": STOP + synth.back_translate(pair) + STOP}
    contigs, at = [], 0
    while at < len(kinds):
        n = 97
        contigs.append("".join(blocks[k] for k in kinds[at:at + n]).encode())
        at += n
    return tseq, toff, S.batch(contigs), kinds


def test_kept_and_dropped_runs_across_lane_and_workgroup_borders():
    from kmergutsjava_amd import hotpath
    tseq, toff, (seq, off), kinds = _runs_case()
    with hotpath.SearchDb.build(tseq, toff) as db:
        with db.search_contigs(seq, off) as ev:
            _check(ev, db, seq, off, 30, 1, None)
            hits, _, paths = ev.search[:3]
            kept = np.zeros(len(hits), dtype=bool)
            kept[ev.call_hits] = True
            assert len(hits) >= 600 and 0.25 <= 1 - kept.mean() <= 0.45, (len(hits), kept.mean())
            edges = np.flatnonzero(np.diff(kept.astype(np.int8))) + 1
            runs = np.diff(np.concatenate([[0], edges, [len(kept)]]))
            assert (edges % 64 != 0).any() and runs.max() > 256 and (runs == 1).any() and (runs > 64).sum() >= 6
            assert kept[:256].any() and (~kept[:256]).any() and len(hits) > 3 * 256
        # every record dropped; no record at all; no fragment; no contig
        with db.search_contigs(seq, off, max_trace_cells=1) as ev:
            assert ev.stats["records"] >= 600 and ev.stats["calls"] == 0 == len(ev.calls) == len(ev.call_hits)
            assert ev.stats["dropped_untraced"] + ev.stats["dropped_status"] + ev.stats["dropped_rank"] == ev.stats["records"]
            _check(ev, db, seq, off, 30, 1, None, max_trace_cells=1)
            assert ev.regions(off)[0].size == 0
        for contigs, frags in (([b"N" * 400, b"A" * 200], 12), ([b"", b"AC", b"TAATAA"], 0), ([], 0)):
            s, o = S.batch(contigs)
            with db.search_contigs(s, o) as ev:
                assert ev.stats["fragments"] == frags and ev.stats["records"] == 0 == ev.stats["calls"] and ev.calls.size == 0
                _check(ev, db, s, o, 30, 1, None)


# ---- the whole call against the CPU model ---------------------------------------------------------------------------------------------

def test_the_gpu_s_calls_are_the_model_s():
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(9)
    targets = [_protein(rng, int(n)) for n in rng.integers(35, 61, 10)]
    tseq, toff = S.batch([t.encode() for t in targets])
    contigs = [b"", b"NNNNNNNNNNNN"]
    while len(contigs) < 18:
        dna = _random_dna(rng, int(rng.integers(0, 60)))
        for _ in range(int(rng.integers(1, 3))):
            t = targets[int(rng.integers(0, 10))]
            dna += _block(rng, _mutated(rng, t if rng.random() < 0.8 else t[:32]), int(rng.integers(0, 2))) + _random_dna(rng, int(rng.integers(0, 40)))
        contigs.append(dna[:600].encode())
    seq, off = S.batch(contigs)
    fn = np.arange(10, dtype=np.int32)[::-1].copy()
    with hotpath.SearchDb.build(tseq, toff) as db:
        for kw in (dict(), dict(max_hits=2, target_fn=fn, align=dict(ref="member", min_ratio_pct=30)), dict(max_trace_cells=45 * 45)):
            mkw = dict(kw)
            mkw.update(mkw.pop("align", None) or {})
            want = TM.translated_model(seq, off, tseq, toff, **mkw)
            with db.search_contigs(seq, off, **kw) as ev:
                _equal(want["fragments"], ev.fragments)
                _equal((want["hits"], want["hit_start"], want["paths"]), ev.search[:3])
                assert ev.calls.tobytes() == want["calls"].tobytes() and ev.call_hits.tobytes() == want["call_hits"].tobytes()
                assert {k: ev.stats[k] for k in TM.DROPS} == want["drops"] and len(want["calls"]) > 0


# ---- end to end: the planted frameshift ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
def test_the_planted_frameshift_is_repaired_and_selected(strand):
    from kmergutsjava_amd import hotpath
    gene, contig = _frameshift_case(strand)
    rng = np.random.default_rng(3)
    other = _protein(rng, 50)
    tseq, toff = S.batch([other.encode(), gene.encode()])
    seq, off = S.batch([_contig(synth.back_translate(other), 31, 35, 1 - strand), contig])
    with hotpath.SearchDb.build(tseq, toff) as db, db.search_contigs(seq, off, align=dict(ref="member", min_ratio_pct=20)) as ev:
        calls = ev.calls
        assert len(calls) == 3 and calls["fI"].tolist() == [0, 1, 1]
        regs, rstart = R.regions(calls, off)
        got = ev.regions(off)
        assert got[0].tobytes() == regs.tobytes() and got[1].tobytes() == rstart.tobytes()
        assert sorted(regs["frames"].tolist()) == [0b010, 0b101] and ev.region_stats["multi_frame"] == 1
        orfs, ps, rs = O.orfs(regs, seq, off)
        new, nps, nrs, junc, jstart, stats = RP.repair(regs, orfs, ps, rs, calls, seq, off)
        g = ev.orfs(seq, off, repair=True)
        _equal((regs, rstart, new, nps, nrs), g)
        assert ev.junctions.tobytes() == junc.tobytes() and ev.junction_start.tobytes() == jstart.tobytes()
        assert {k: ev.repair_stats[k] for k in RP.STAT_KEYS} == {k: stats[k] for k in RP.STAT_KEYS} and stats["repaired"] == 1
        i = int(np.flatnonzero(new["flags"] & N.ORF_REPAIRED)[0])
        prot = g[4][g[3][i]:g[3][i + 1]].tobytes().decode()
        assert gene[1:30] in prot and gene[-30:] in prot
        plain = ev.orfs(seq, off)
        _equal((regs, rstart, orfs, ps, rs), plain)
        s = ev.select(off, seq, orfs=True, repair=True, free_min_res=30)
        assert s[0].tobytes() == regs.tobytes() and s[2][:2].tobytes() == new.tobytes()
        sel, _ = SL.select(SL.of_records(s[2]))
        assert s[5].tobytes() == sel.tobytes() and (s[5]["state"][:2] == N.SEL_SELECTED).all()
        s3 = ev.select(off)
        assert s3[2].tobytes() == SL.select(SL.of_records(regs))[0].tobytes()


# ---- device input, the room, the error words, the allocation sweep ----------------------------------------------------------------------------

def _small():
    rng = np.random.default_rng(41)
    targets = [_protein(rng, 45) for _ in range(4)]
    tseq, toff = S.batch([t.encode() for t in targets])
    contigs = [(_random_dna(rng, 20 + k) + _block(rng, _mutated(rng, targets[k]), k % 2) + _random_dna(rng, 33)).encode() for k in range(4)]
    return tseq, toff, S.batch(contigs)


def test_a_device_input_gives_the_host_input_s_bytes():
    import torch
    from kmergutsjava_amd import hotpath
    tseq, toff, (seq, off) = _small()
    d = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    with hotpath.SearchDb.build(tseq, toff) as db, db.search_contigs(seq, off) as a, db.search_contigs(None, off, device_ptr=d.data_ptr()) as b:
        assert len(a.calls) == 4 and a.calls.tobytes() == b.calls.tobytes() and a.call_hits.tobytes() == b.call_hits.tobytes()
        _equal(a.fragments, b.fragments)
        _equal(a.search, b.search)
        assert _counts(a.stats) == _counts(b.stats)


def test_a_batch_over_the_room_is_refused_and_fits_after_reserve():
    from kmergutsjava_amd import hotpath
    tseq, toff, (seq, off) = _small()
    with hotpath.SearchDb.build(tseq, toff, query_room=100) as db:
        live = db.live_device_bytes()
        with pytest.raises(N.KmerGutsNativeError) as e:
            db.search_contigs(seq, off)
        frags = hotpath.free_orfs(seq, off, min_res=30, start_codons=0)
        n_res = len(frags[2])
        assert e.value.code == N.KG_ERR_LIMIT and 100 < n_res <= 2 * len(seq)
        assert "%d residues of queries do not fit the room of 100 residues" % n_res in str(e.value)
        assert db.live_device_bytes() == live
        assert len(db.search(tseq[:45], toff[:2])[0]) == 1              # the handle is usable
        db.reserve(2 * len(seq))                                        # the bound a caller can reserve beforehand
        with db.search_contigs(seq, off) as ev:
            assert len(ev.calls) == 4
            _check(ev, db, seq, off, 30, 1, None)


def test_parameter_and_null_errors_by_their_words():
    from kmergutsjava_amd import hotpath
    lib = N.load()
    tseq, toff, (seq, off) = _small()
    arr = np.frombuffer(seq, dtype=np.uint8)
    with hotpath.SearchDb.build(tseq, toff) as db:
        live = db.live_device_bytes()

        def call(p=(2, 8, 256, 0), tp=(30, 1, (0, 0)), al=True, seq_ptr=arr.ctypes.data, offs=off, n=len(off) - 1, trace=0, cells=1 << 24, fn=None,
                 ung=None, band=None, out=True, handle=True, max_windows=0):
            h = C.c_void_p()
            sp = N.KgSearchParams(*p)
            ap = hotpath._align_params()[0]
            t = N.KgTranslateParams(tp[0], tp[1], (C.c_int32 * 2)(*tp[2])) if tp is not None else None
            rc = lib.kg_contigs_search_translated(db._h if handle else None, C.byref(sp), C.byref(ap) if al else None,
                                                   C.byref(t) if t is not None else None, seq_ptr, 0, offs.ctypes.data if offs is not None else None, n,
                                                   max_windows, 0, trace, cells, None, C.byref(ung) if ung is not None else None,
                                                   C.byref(band) if band is not None else None, fn.ctypes.data if fn is not None else None,
                                                   C.byref(h) if out else None)
            assert not h.value
            return rc, lib.kg_last_error().decode()

        bad_fn = np.array([0, 1, -1, 2], dtype=np.int32)
        dec = np.array([0, 5, 3], dtype=np.int64)
        for kw, code, text in (
                (dict(out=False), N.KG_ERR_ARG, "null argument"),
                (dict(handle=False), N.KG_ERR_ARG, "null kg_searchdb"),
                (dict(p=(0, 8, 256, 0)), N.KG_ERR_ARG, "min_shared must be >= 1"),
                (dict(p=(2, 65, 256, 0)), N.KG_ERR_ARG, "max_cand must be in 1..64"),
                (dict(al=False), N.KG_ERR_ARG, "null kg_align_params"),
                (dict(band=N.KgBandParams(8, (C.c_int32 * 3)(0, 0, 0))), N.KG_ERR_ARG, "null kg_ungapped_params"),
                (dict(max_windows=-1), N.KG_ERR_ARG, "max_windows must be >= 0"),
                (dict(trace=3), N.KG_ERR_ARG, "trace must be KG_TRACE_HITS or KG_TRACE_ALL"),
                (dict(trace=16), N.KG_ERR_ARG, "trace takes at most one of KG_TRACE_OPS and KG_TRACE_OPS_EQX beside its mode, and no bit above 15"),
                (dict(cells=0), N.KG_ERR_ARG, "max_trace_cells must be >= 1"),
                (dict(tp=None), N.KG_ERR_ARG, "null kg_translate_params"),
                (dict(tp=(0, 1, (0, 0))), N.KG_ERR_ARG, "min_res must be >= 1"),
                (dict(tp=(30, 0, (0, 0))), N.KG_ERR_ARG, "max_hits must be in 1..64"),
                (dict(tp=(30, 65, (0, 0))), N.KG_ERR_ARG, "max_hits must be in 1..64"),
                (dict(tp=(30, 1, (0, 1))), N.KG_ERR_ARG, "kg_translate_params.reserved must be 0"),
                (dict(fn=bad_fn), N.KG_ERR_ARG, "target_fn[2] < 0"),
                (dict(n=-1), N.KG_ERR_ARG, "n_seqs < 0"),
                (dict(offs=None), N.KG_ERR_ARG, "null offsets"),
                (dict(offs=dec, n=2), N.KG_ERR_ARG, "contig 1: offsets decrease (offsets[s+1] < offsets[s])"),
                (dict(seq_ptr=None), N.KG_ERR_ARG, "null sequence bytes")):
            assert call(**kw) == (code, text), kw
            assert db.live_device_bytes() == live
        with db.search_contigs(seq, off) as ev:
            assert len(ev.calls) == 4


def test_busy_is_the_search_s_answer(monkeypatch):
    from kmergutsjava_amd import hotpath
    tseq, toff, (seq, off) = _small()
    with hotpath.SearchDb.build(tseq, toff) as db:
        live = db.live_device_bytes()
        monkeypatch.setenv("KG_TEST_SEARCHDB_REENTER", "1")
        with pytest.raises(N.KmerGutsNativeError) as e:
            db.search_contigs(seq, off)
        monkeypatch.delenv("KG_TEST_SEARCHDB_REENTER")
        assert e.value.code == N.KG_ERR_BUSY and "another call is in flight on this kg_searchdb" in str(e.value)
        assert db.live_device_bytes() == live
        with db.search_contigs(seq, off) as ev:
            assert len(ev.calls) == 4


def test_every_failing_allocation_is_nomem_and_leaves_the_handle_as_it_was(monkeypatch):
    import torch
    from kmergutsjava_amd import hotpath
    tseq, toff, (seq, off) = _small()
    fn = np.array([3, 2, 1, 0], dtype=np.int32)
    with hotpath.SearchDb.build(tseq, toff) as db:
        with db.search_contigs(seq, off, target_fn=fn) as ev:
            want = (ev.calls.copy(), ev.call_hits.copy())
        torch.cuda.synchronize()
        live, free = db.live_device_bytes(), torch.cuda.mem_get_info()[0]
        failed, got = 0, None
        for n in range(1, 900):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got = db.search_contigs(seq, off, target_fn=fn)
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert db.live_device_bytes() == live and torch.cuda.mem_get_info()[0] == free, n
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= 30 and got is not None
        with got:
            assert got.calls.tobytes() == want[0].tobytes() and got.call_hits.tobytes() == want[1].tobytes()
        assert db.live_device_bytes() == live and torch.cuda.mem_get_info()[0] == free
        with db.search_contigs(seq, off, target_fn=fn) as ev:
            assert ev.calls.tobytes() == want[0].tobytes()
