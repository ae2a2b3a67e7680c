"""kg_contigs_search_residual / kg_result_search_residual on the GPU.  The composition law, byte for byte on every array: the
fragments are free_orfs(start_codons=0)'s, explain is residual_model.explain_of's, the searched records, prot_start and residues
are the numpy subset, the hit records are db.search's on exactly those, the homology CALLs translated_model.calls_of's and the
merged list, kinds, sources and call_hits residual_model.merge_of's.  Then the two identities with what exists, the mark, layout
and copy kernels at lane, workgroup, chunk and alignment borders, a real table's CALLs where they lie on the device, the planted
frameshift with one half from each source, the room, the error words and the allocation sweep."""
import ctypes as C

import numpy as np
import pytest

import orfs_model as O
import regions_model as R
import repair_model as RP
import residual_model as RM
import search_model as S
import select_model as SL
import translated_model as TM
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import synth
from test_gpu_translated import _block, _counts, _equal, _mutated, _random_dna, _small, mixed, mixed_db  # noqa: F401
from test_translated_host import _contig, _frameshift_case, _protein

pytestmark = pytest.mark.gpu

STOP = "TAA"


def _sig(rows):
    out = np.zeros(len(rows), dtype=N.CALL_DTYPE)
    for k, (container, start, end, count, fi) in enumerate(rows):
        out[k] = (container, start, end, count, fi, np.float32(count))
    return out


def _span(f, off):
    """(container, first codon, last codon) of a fragment record."""
    s = int(f["seq"])
    b = TM.first_codon(f, int(off[s + 1] - off[s]))
    return 6 * s + 3 * int(f["strand"]) + int(f["frame"]), b, b + int(f["n_res"]) - 1


def _plant(frags, off, which, count=3, fi=0):
    """One signature CALL on the first codon of every fragment of `which` (ascending: container order)."""
    return _sig([(_span(frags[k], off)[0], _span(frags[k], off)[1], _span(frags[k], off)[1], count, fi) for k in which])


def _check(ev, db, seq, off, sig, fn, min_res, max_hits, explain_min=1, min_db_count=0, **search):
    """The composition law on one evidence; -> what the model found on the way."""
    from kmergutsjava_amd import hotpath
    frags = hotpath.free_orfs(seq, off, min_res=min_res, start_codons=0)
    _equal(frags, ev.fragments)
    recs, pstart, res = ev.fragments
    explain = RM.explain_of(recs, off, sig)
    assert ev.explain.dtype == np.int64 and ev.explain.tobytes() == explain.tobytes()
    searched, srecs, sstart, sres = RM.subset_of(recs, pstart, res, explain, explain_min)
    assert ev.searched.dtype == np.int64 and ev.searched.tobytes() == searched.tobytes()
    _equal((srecs, sstart, sres), ev.searched_fragments)
    if len(searched):
        _equal(db.search(sres, sstart, paths="hits", **search), ev.search)
    else:                                                   # no query: no search was launched, the hit set is a valid empty one
        assert len(ev.search[0]) == 0 == len(ev.search[2]) and ev.search[1].tolist() == [0]
        assert ev.search[3]["queries"] == 0 == ev.search[3]["hits"] and ev.search[3]["ms_total"] == 0 == ev.stats["ms_search"]
    hits, start, paths = ev.search[:3]
    db_calls, db_hits, drops = TM.calls_of(srecs, hits, paths, off, max_hits, fn)
    merged, kind, source, hit, dropped = RM.merge_of(sig, db_calls, db_hits, min_db_count)
    for name, got, want in (("calls", ev.calls, merged), ("call_kind", ev.call_kind, kind), ("call_source", ev.call_source, source),
                            ("call_hits", ev.call_hits, hit)):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), name
    assert (np.diff(ev.calls["container"].astype(np.int64)) >= 0).all()
    st, rs = ev.stats, ev.residual_stats
    assert (st["fragments"], st["fragment_residues"], st["records"], st["calls"]) == (len(recs), len(res), len(hits), len(db_calls))
    assert {k: st[k] for k in TM.DROPS} == drops
    assert st["ms_total"] == pytest.approx(st["ms_fragments"] + st["ms_search"] + st["ms_calls"])
    assert {k: v for k, v in rs.items() if not k.startswith("ms_")} == dict(
        sig_calls=len(sig), explained=len(recs) - len(searched), explained_residues=len(res) - len(sres), searched=len(searched),
        searched_residues=len(sres), db_calls=len(db_calls), dropped_min_count=dropped, merged=len(merged))
    assert rs["explained"] + rs["searched"] == st["fragments"] and rs["merged"] == rs["sig_calls"] + rs["db_calls"] - rs["dropped_min_count"]
    assert rs["ms_total"] == pytest.approx(st["ms_total"] + rs["ms_explain"] + rs["ms_compact"] + rs["ms_merge"])
    return dict(explain=explain, searched=searched, kind=kind, dropped=dropped, db_calls=db_calls, frags=recs)


# ---- the composition law ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed_sig(mixed, mixed_db):
    """Signature CALLs for the `mixed` contigs: every second homology CALL of the plain call as a table would name it (counts 1
    to 7), and CALLs that reach from the end of one fragment across the stop into the next."""
    from kmergutsjava_amd import hotpath
    tseq, toff, seq, off = mixed
    with mixed_db.search_contigs(seq, off) as ev:
        base = ev.calls.copy()
    rows = [(int(c["container"]), int(c["start"]), int(c["end"]), 1 + k % 7, 200 + k % 5) for k, c in enumerate(base) if k % 2 == 0]
    frags = hotpath.free_orfs(seq, off, min_res=30, start_codons=0)[0]
    spans = [_span(f, off) for f in frags]
    across = [(a[0], a[2] - 1, b[1] + 1, 5, 300) for a, b in zip(spans, spans[1:]) if a[0] == b[0]][::7]
    assert len(rows) >= 20 and len(across) >= 3
    rows = sorted(rows + across, key=lambda r: r[0])
    return _sig(rows)


@pytest.mark.parametrize("min_res", [1, 30])
@pytest.mark.parametrize("max_hits", [1, 3])
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("explain_min,min_db_count", [(1, 0), (4, 200)])
def test_every_array_is_that_of_the_parts(mixed, mixed_db, mixed_sig, min_res, max_hits, filtered, explain_min, min_db_count):
    tseq, toff, seq, off = mixed
    fn = np.arange(len(toff) - 1, dtype=np.int32) // 3 + 100
    search = dict(ungapped={"min_score": 20}, band=16) if filtered else {}
    search["max_trace_cells"] = 70 * 70
    with mixed_db.search_contigs(seq, off, min_res=min_res, max_hits=max_hits, target_fn=fn, explained_by=mixed_sig, explain_min=explain_min,
                                 min_db_count=min_db_count, **search) as ev:
        m = _check(ev, mixed_db, seq, off, mixed_sig, fn, min_res, max_hits, explain_min, min_db_count, **search)
        calls, kind = ev.calls, ev.call_kind
    # the input does what it is for: both kinds occur, some CALL touches two fragments, some container holds merged CALLs of both
    # kinds, and the two parameters cut where they are meant to
    assert (kind == 0).sum() == len(mixed_sig) and (kind == 1).sum() > 0
    spans = [_span(f, off) for f in m["frags"]]
    touched = [sum(1 for cont, b, last in spans if cont == int(c["container"]) and int(c["start"]) <= last and int(c["end"]) >= b)
               for c in mixed_sig[mixed_sig["fI"] == 300]]
    assert max(touched) >= 2
    both = {int(c) for c in calls["container"][kind == 0]} & {int(c) for c in calls["container"][kind == 1]}
    assert both
    low = (m["explain"] > 0) & (m["explain"] < 4)
    assert low.any() and (m["explain"] >= 4).any()
    if min_db_count:
        assert m["dropped"] > 0 and (kind == 1).sum() == len(m["db_calls"]) - m["dropped"]


def test_without_signature_calls_it_is_the_plain_call_and_with_every_fragment_explained_nothing_is_searched(mixed, mixed_db):
    from kmergutsjava_amd import hotpath
    tseq, toff, seq, off = mixed
    fn = np.arange(len(toff) - 1, dtype=np.int32)
    with mixed_db.search_contigs(seq, off, target_fn=fn) as plain, \
            mixed_db.search_contigs(seq, off, target_fn=fn, explained_by=np.zeros(0, dtype=N.CALL_DTYPE)) as ev:
        assert ev.calls.tobytes() == plain.calls.tobytes() and ev.call_hits.tobytes() == plain.call_hits.tobytes() and len(plain.calls) > 20
        _equal(plain.fragments, ev.fragments)
        _equal(plain.search, ev.search)
        _equal(plain.fragments, ev.searched_fragments)
        assert (ev.call_kind == 1).all() and ev.call_source.tolist() == list(range(len(plain.calls))) and not ev.explain.any()
        assert _counts(plain.stats) == _counts(ev.stats) and ev.searched.tolist() == list(range(len(plain.fragments[0])))
        assert not hasattr(plain, "explain") and not hasattr(plain, "call_kind") and not hasattr(plain, "residual_stats")
        frags = plain.fragments[0]
    sig = _plant(frags, off, range(len(frags)), count=1, fi=7)
    live = mixed_db.live_device_bytes()
    with mixed_db.search_contigs(seq, off, target_fn=fn, explained_by=sig) as ev:
        _check(ev, mixed_db, seq, off, sig, fn, 30, 1)
        assert ev.residual_stats["searched"] == 0 == ev.stats["records"] == ev.residual_stats["db_calls"] and ev.stats["ms_search"] == 0
        assert ev.calls.tobytes() == sig.tobytes() and (ev.call_kind == 0).all() and (ev.call_hits == -1).all()
        assert len(ev.searched_fragments[0]) == 0 and ev.searched_fragments[1].tolist() == [0] and len(ev.searched) == 0
        regs, rstart = R.regions(sig, off)
        got = ev.regions(off)
        assert got[0].tobytes() == regs.tobytes() and got[1].tobytes() == rstart.tobytes()
    assert mixed_db.live_device_bytes() == live
    # the same with ops, the ungapped stage and a band asked for: the empty hit set answers every getter the options imply
    with mixed_db.search_contigs(seq, off, target_fn=fn, explained_by=sig, paths="all", ops="eqx", ungapped=True, band=8) as ev:
        assert len(ev.search[0]) == 0 and ev.search[4].tolist() == [0] and len(ev.search[5]) == 0 and len(ev.search[6]) == 0
        assert ev.search[3]["band"]["band"] == 8 and ev.search[3]["ungapped"]["scored"] == 0


# ---- explained and searched runs across lane and workgroup borders ---------------------------------------------------------------------------

def test_explained_and_searched_runs_across_lane_and_workgroup_borders():
    """Gene blocks in one frame, as test_gpu_translated._runs_case lays them; CALLs planted fragment by fragment, so that explained
    and searched fragments come in runs of 1, 63, 64, 65, 128, 257, ... in turn."""
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(78)
    keep, other = _protein(rng, 31), _protein(rng, 31)
    tseq, toff = S.batch([keep.encode(), other.encode()])
    blocks = [STOP + synth.back_translate(p) for p in (keep, other)]
    contigs = ["".join(blocks[int(x)] for x in rng.integers(0, 2, 32)) + STOP for _ in range(34)]
    seq, off = S.batch([c.encode() for c in contigs])
    assert int(np.diff(off).max()) <= 3500
    frags = hotpath.free_orfs(seq, off, min_res=30, start_codons=0)[0]
    n = len(frags)
    explained, at, k = np.zeros(n, dtype=bool), 0, 0
    runs = (1, 63, 64, 65, 128, 257, 2, 1, 130, 3, 65, 1, 1, 70)
    while at < n:
        explained[at:at + runs[k % len(runs)]] = k % 2 == 0
        at += runs[k % len(runs)]
        k += 1
    sig = _plant(frags, off, np.flatnonzero(explained))
    fn = np.array([5, 6], dtype=np.int32)
    with hotpath.SearchDb.build(tseq, toff) as db, db.search_contigs(seq, off, target_fn=fn, explained_by=sig) as ev:
        m = _check(ev, db, seq, off, sig, fn, 30, 1)
        got = ev.explain >= 1
        assert got.tolist() == explained.tolist() and n > 1000 and (ev.call_kind == 1).sum() > 300
        edges = np.flatnonzero(np.diff(got.astype(np.int8))) + 1
        lens = np.diff(np.concatenate([[0], edges, [n]]))
        assert {1, 63, 64, 65, 128, 257} <= set(lens.tolist()) and (edges % 64 != 0).any()
        assert got[:256].any() and (~got[:256]).any() and len(m["searched"]) > 256 and (~got).sum() > 256


# ---- the residues' copy: fragment lengths and every source and destination alignment -------------------------------------------------------------

SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1100)


def test_searched_fragments_of_every_length_at_every_alignment():
    """min_res = 1: every stop-to-stop run of every frame is a fragment.  Frame 0 of '+' holds stop-free runs of the lengths above,
    each twice; every third fragment is explained unless it has one of those lengths, so searched fragments are neighbours here
    and separated by explained ones there, and their residues start at every offset mod 16 on both sides of the copy."""
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(79)
    long_, short = _protein(rng, 1100), _protein(rng, 64)        # (lengths of SIZES: never explained below)
    tseq, toff = S.batch([long_.encode(), short.encode()])
    contigs, cur = [], ""
    for n in SIZES[:-1] + SIZES[:-1]:
        cur += STOP + synth.back_translate(_protein(rng, n))
        if len(cur) > 2400:
            contigs.append(cur + STOP)
            cur = ""
    contigs += [cur + STOP + synth.back_translate(short) + STOP, _random_dna(rng, 5) + STOP + synth.back_translate(long_) + STOP]
    seq, off = S.batch([c.encode() for c in contigs])
    assert int(np.diff(off).max()) <= 3500
    recs, pstart, _ = hotpath.free_orfs(seq, off, min_res=1, start_codons=0)
    which = [k for k in range(len(recs)) if k % 3 == 1 and int(recs[k]["n_res"]) not in SIZES]
    sig = _plant(recs, off, which)
    fn = np.array([0, 1], dtype=np.int32)
    with hotpath.SearchDb.build(tseq, toff) as db, db.search_contigs(seq, off, min_res=1, target_fn=fn, explained_by=sig) as ev:
        m = _check(ev, db, seq, off, sig, fn, 1, 1)
        searched, new_start = ev.searched, ev.searched_fragments[1]
        assert set(SIZES) <= set(recs["n_res"][searched].tolist()) and len(which) > 100
        src, dst = pstart[searched], new_start[:-1]
        assert set((src % 16).tolist()) == set(range(16)) == set((dst % 16).tolist())
        assert {(int(a) % 4, int(b) % 4) for a, b in zip(src, dst)} == {(a, b) for a in range(4) for b in range(4)}
        gaps = np.diff(searched)
        assert (gaps == 1).any() and (gaps == 2).any()
        # chunks of the copy inside one fragment, across two and across many: N.RESIDUAL_CHUNK destination bytes a lane
        ends = new_start[1:]
        per_chunk = np.bincount(((ends - 1) // N.RESIDUAL_CHUNK), minlength=1)
        assert per_chunk.max() >= 3 and (per_chunk == 0).any()
        assert {0, 1} <= set(m["db_calls"]["fI"].tolist())           # the longest fragment and a short one are found


# ---- the mark kernel's walk: one CALL over many fragments; CALLs in the last container only; empty inputs ------------------------------------------

def test_one_call_over_eighty_fragments_and_calls_in_the_last_container_only():
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(80)
    target = _protein(rng, 40)
    tseq, toff = S.batch([target.encode()])
    many = (STOP + "GCTGCAGCC") * 90 + STOP                  # frame 0 of '+': 90 fragments of 3 residues
    tail = _contig(synth.back_translate(target), 30, 35, 1)   # '-' strand, frame 30 % 3 = 0 ... the last contig
    seq, off = S.batch([many.encode(), b"N" * 50, tail])
    fn = np.array([9], dtype=np.int32)
    with hotpath.SearchDb.build(tseq, toff) as db:
        sig = _sig([(0, 2, 4 * 80 + 1, 11, 1)])
        with db.search_contigs(seq, off, min_res=1, target_fn=fn, explained_by=sig) as ev:
            m = _check(ev, db, seq, off, sig, fn, 1, 1)
            assert 70 <= int((m["explain"] == 11).sum()) <= 81 and int(m["explain"].sum()) == 11 * int((m["explain"] == 11).sum())
        last = 6 * 3 - 1                                      # container 17: '-' frame 2 of the last contig
        L = int(off[3] - off[2])
        sig = _sig([(last, 0, 3, 2, 1), (last, (L - 2) // 3 - 2, (L - 2) // 3 - 1, 2, 1)])
        with db.search_contigs(seq, off, min_res=1, target_fn=fn, explained_by=sig) as ev:
            m = _check(ev, db, seq, off, sig, fn, 1, 1)
            assert m["explain"][:-1].sum() < m["explain"].sum() and m["explain"][-1] > 0 and (ev.call_kind[-2:] == 0).all()
        for contigs, frags in (([b"N" * 400], 6), ([b"", b"AC", b"TAATAA"], 0), ([], 0)):
            s, o = S.batch(contigs)
            with db.search_contigs(s, o, target_fn=fn, explained_by=np.zeros(0, dtype=N.CALL_DTYPE)) as ev:
                _check(ev, db, s, o, np.zeros(0, dtype=N.CALL_DTYPE), fn, 30, 1)
                assert ev.stats["fragments"] == frags and ev.calls.size == 0 == ev.call_kind.size
        s, o = S.batch([b"N" * 400])
        sig = _sig([(1, 5, 9, 4, 0)])
        with db.search_contigs(s, o, target_fn=fn, explained_by=sig) as ev:
            _check(ev, db, s, o, sig, fn, 30, 1)
            assert ev.residual_stats["explained"] == 1 and ev.residual_stats["searched"] == 5
            assert ev.residual_stats["searched_residues"] % N.RESIDUAL_CHUNK != 0       # the copy's last chunk is a partial one


# ---- the CALLs of a real scan, where they lie on the device ------------------------------------------------------------------------------------

def _table_case():
    """Eight targets; the table knows the first four (signatures derived from them), the contigs hold exact copies of those and
    mutated copies of the others."""
    rng = np.random.default_rng(81)
    targets = [_protein(rng, int(n)) for n in rng.integers(45, 90, 8)]
    tseq, toff = S.batch([t.encode() for t in targets])
    contigs = []
    for k in range(10):
        dna = _random_dna(rng, 10 + k)
        for t in rng.permutation(8)[:3]:
            copy = targets[int(t)] if t < 4 else _mutated(rng, targets[int(t)])
            dna += _block(rng, copy, int(rng.integers(0, 2))) + _random_dna(rng, int(rng.integers(0, 50)))
        contigs.append(dna.encode())
    return targets, tseq, toff, S.batch(contigs)


def test_a_scan_result_gives_the_bytes_of_its_calls_from_host_and_device_input():
    import torch
    from kmergutsjava_amd import hotpath
    from kmergutsjava_amd.make_table import default_num_sigs
    targets, tseq, toff, (seq, off) = _table_case()
    known_seq, known_off = S.batch([t.encode() for t in targets[:4]])
    fn = np.arange(8, dtype=np.int32)
    with hotpath.derive_signatures(known_seq, known_off, np.arange(4, dtype=np.int32), np.zeros(4, dtype=np.int32), min_proteins=1) as s:
        with hotpath.SignatureTable.build(s.device_tensor(), default_num_sigs(s.count)) as tab, hotpath.SearchDb.build(tseq, toff) as db:
            with tab.scan(seq, off, hotpath.Params(aa=False)) as r:
                sig = r.calls()
                assert len(sig) >= 4 and set(sig["fI"].tolist()) <= {0, 1, 2, 3}
                live, tlive = db.live_device_bytes(), tab.live_device_bytes()
                with db.search_contigs(seq, off, target_fn=fn, explained_by=r) as a, db.search_contigs(seq, off, target_fn=fn, explained_by=sig) as b:
                    m = _check(a, db, seq, off, sig, fn, 30, 1)
                    for name in ("calls", "call_hits", "call_kind", "call_source", "explain", "searched"):
                        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
                    _equal(a.search, b.search)
                    _equal(a.searched_fragments, b.searched_fragments)
                    assert _counts(a.stats) == _counts(b.stats) and _counts(a.residual_stats) == _counts(b.residual_stats)
                    assert (a.call_kind == 0).sum() == len(sig) and (a.call_kind == 1).sum() >= 4 and a.residual_stats["explained"] >= 4
                    assert set(a.calls["fI"][a.call_kind == 1].tolist()) <= {4, 5, 6, 7}      # what the table named was not searched
                    d = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
                    torch.cuda.synchronize()
                    with db.search_contigs(None, off, target_fn=fn, explained_by=r, device_ptr=d.data_ptr()) as c:
                        assert c.calls.tobytes() == a.calls.tobytes() and c.call_kind.tobytes() == a.call_kind.tobytes()
                        _equal(a.search, c.search)
                assert (db.live_device_bytes(), tab.live_device_bytes()) == (live, tlive)
                # a result of another batch, and a protein scan's, are refused
                with pytest.raises(N.KmerGutsNativeError) as e:
                    db.search_contigs(seq[:int(off[3])], off[:4], target_fn=fn, explained_by=r)
                assert e.value.code == N.KG_ERR_ARG and "n_seqs is not the result's number of sequences" in str(e.value)
            with tab.scan(known_seq, known_off, hotpath.Params(aa=True)) as r:
                with pytest.raises(N.KmerGutsNativeError) as e:
                    db.search_contigs(known_seq, known_off, target_fn=fn, explained_by=r)
                assert e.value.code == N.KG_ERR_ARG and "a protein (-a) result" in str(e.value)
            with tab.scan(seq, off, hotpath.Params(aa=False, skip_aggregate=True)) as r:
                with pytest.raises(N.KmerGutsNativeError) as e:
                    db.search_contigs(seq, off, target_fn=fn, explained_by=r)
                assert e.value.code == N.KG_ERR_ARG and "a KG_F_SKIP_AGGREGATE result has no CALL records" in str(e.value)
            assert (db.live_device_bytes(), tab.live_device_bytes()) == (live, 0)          # (every result is closed by now)


# ---- the point of it: one half of a frameshifted gene from each source ------------------------------------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
def test_the_planted_frameshift_with_one_half_from_each_source_is_repaired_and_selected(strand):
    from kmergutsjava_amd import hotpath
    gene, contig = _frameshift_case(strand)
    rng = np.random.default_rng(3)
    other = _protein(rng, 50)
    tseq, toff = S.batch([other.encode(), gene.encode()])
    seq, off = S.batch([_contig(synth.back_translate(other), 31, 35, 1 - strand), contig])
    fn = np.array([4, 7], dtype=np.int32)                   # one function name, 7, for the table's half and the database's
    kw = dict(align=dict(ref="member", min_ratio_pct=20), target_fn=fn)
    with hotpath.SearchDb.build(tseq, toff) as db:
        with db.search_contigs(seq, off, **kw) as plain:
            assert plain.calls["fI"].tolist() == [4, 7, 7]
            first = plain.calls[1:2].copy()
        first["count"], first["weightedHits"] = 9, 9.0
        with db.search_contigs(seq, off, explained_by=first, **kw) as ev:
            _check(ev, db, seq, off, first, fn, 30, 1, align=dict(ref="member", min_ratio_pct=20))
            calls = ev.calls
            assert len(calls) == 3 and sorted(ev.call_kind.tolist()) == [0, 1, 1] and ev.residual_stats["explained"] == 1
            regs, rstart = R.regions(calls, off)
            got = ev.regions(off)
            assert got[0].tobytes() == regs.tobytes() and got[1].tobytes() == rstart.tobytes()
            assert sorted(regs["frames"].tolist()) == [0b010, 0b101] and ev.region_stats["multi_frame"] == 1
            assert RM.evidence_of(regs, calls, ev.call_kind, off) == (["db", "table+db"] if int(regs[0]["seq"]) == 0 else ["table+db", "db"])
            orfs, ps, rs = O.orfs(regs, seq, off)
            new, nps, nrs, junc, jstart, stats = RP.repair(regs, orfs, ps, rs, calls, seq, off)
            g = ev.orfs(seq, off, repair=True)
            _equal((regs, rstart, new, nps, nrs), g)
            assert ev.junctions.tobytes() == junc.tobytes() and ev.junction_start.tobytes() == jstart.tobytes() and stats["repaired"] == 1
            i = int(np.flatnonzero(new["flags"] & N.ORF_REPAIRED)[0])
            prot = g[4][g[3][i]:g[3][i + 1]].tobytes().decode()
            assert gene[1:30] in prot and gene[-30:] in prot
            s = ev.select(off, seq, orfs=True, repair=True, free_min_res=30)
            assert s[0].tobytes() == regs.tobytes() and s[2][:2].tobytes() == new.tobytes()
            sel, _ = SL.select(SL.of_records(s[2]))
            assert s[5].tobytes() == sel.tobytes() and (s[5]["state"][:2] == N.SEL_SELECTED).all()


# ---- the room, the error words, busy, the allocation sweep -----------------------------------------------------------------------------------------

def test_the_room_counts_the_searched_residues_only():
    from kmergutsjava_amd import hotpath
    tseq, toff, (seq, off) = _small()
    fn = np.arange(4, dtype=np.int32)
    recs, pstart, res = hotpath.free_orfs(seq, off, min_res=30, start_codons=0)
    lens = np.diff(pstart)
    keep = int(np.argmax(lens))                             # every fragment but the longest is explained
    sig = _plant(recs, off, [k for k in range(len(recs)) if k != keep])
    room = int(lens[keep]) + 3
    assert room < len(res)
    with hotpath.SearchDb.build(tseq, toff, query_room=room) as db:
        live = db.live_device_bytes()
        with db.search_contigs(seq, off, target_fn=fn, explained_by=sig) as ev:
            _check(ev, db, seq, off, sig, fn, 30, 1)
            assert ev.residual_stats["searched_residues"] == int(lens[keep]) <= room
        with pytest.raises(N.KmerGutsNativeError) as e:
            db.search_contigs(seq, off, target_fn=fn, explained_by=sig[:0])
        assert e.value.code == N.KG_ERR_LIMIT
        assert "%d residues of queries do not fit the room of %d residues; kg_searchdb_reserve regrows it" % (len(res), room) in str(e.value)
        assert db.live_device_bytes() == live
        with db.search_contigs(seq, off, target_fn=fn, explained_by=sig) as ev:
            assert ev.residual_stats["searched"] == 1


def test_parameter_and_list_errors_by_their_words():
    from kmergutsjava_amd import hotpath
    lib = N.load()
    tseq, toff, (seq, off) = _small()
    arr = np.frombuffer(seq, dtype=np.uint8)
    good_fn = np.arange(4, dtype=np.int32)
    L0 = int(off[1])
    with hotpath.SearchDb.build(tseq, toff) as db:
        live = db.live_device_bytes()

        def call(sig=None, n=None, rp=(1, 0, 0), fn=good_fn, tp=(30, 1, (0, 0)), out=True, n_seqs=len(off) - 1):
            h = C.c_void_p()
            sp, ap = N.KgSearchParams(2, 8, 256, 0), hotpath._align_params()[0]
            t = N.KgTranslateParams(tp[0], tp[1], (C.c_int32 * 2)(*tp[2]))
            r = N.KgResidualParams(*rp) if rp is not None else None
            rc = lib.kg_contigs_search_residual(db._h, C.byref(sp), C.byref(ap), C.byref(t), arr.ctypes.data, 0, off.ctypes.data, n_seqs, 0, 0, 0, 1 << 24,
                                                None, None, None, fn.ctypes.data if fn is not None else None,
                                                sig.ctypes.data if sig is not None and len(sig) else None, 0,
                                                (len(sig) if sig is not None else 0) if n is None else n, C.byref(r) if r is not None else None,
                                                C.byref(h) if out else None)
            assert not h.value
            return rc, lib.kg_last_error().decode()

        ok = (0, 1, 2, 3, 0)
        for kw, code, text in (
                (dict(out=False), N.KG_ERR_ARG, "null argument"),
                (dict(rp=None), N.KG_ERR_ARG, "null kg_residual_params"),
                (dict(rp=(0, 0, 0)), N.KG_ERR_ARG, "explain_min must be >= 1"),
                (dict(rp=(1, -1, 0)), N.KG_ERR_ARG, "min_db_count must be >= 0"),
                (dict(rp=(1, 0, 1)), N.KG_ERR_ARG, "kg_residual_params.reserved must be 0"),
                (dict(tp=(0, 1, (0, 0))), N.KG_ERR_ARG, "min_res must be >= 1"),
                (dict(fn=None), N.KG_ERR_ARG, "null target_fn: the two kinds of CALL need one function index space"),
                (dict(fn=np.array([0, 1, -1, 2], dtype=np.int32)), N.KG_ERR_ARG, "target_fn[2] < 0"),
                (dict(n=-1), N.KG_ERR_ARG, "n_calls < 0"),
                (dict(n=3), N.KG_ERR_ARG, "null CALL records"),
                (dict(sig=_sig([ok]), n_seqs=0), N.KG_ERR_ARG, "CALL 0: container >= 6 * n_seqs"),
                (dict(sig=_sig([ok, (7, 1, 2, 3, 0), (6, 1, 2, 3, 0)])), N.KG_ERR_ARG,
                 "CALL 2: container below its predecessor's (calls[] must be in container order)"),
                (dict(sig=_sig([ok, (24, 1, 2, 3, 0)])), N.KG_ERR_ARG, "CALL 1: container >= 6 * n_seqs"),
                (dict(sig=_sig([ok, ok, (1, 1, 2, -3, 0)])), N.KG_ERR_ARG, "CALL 2: negative count"),
                (dict(sig=_sig([(0, 5, 4, 3, 0)])), N.KG_ERR_ARG, "CALL 0: start > end"),
                (dict(sig=_sig([ok, (0, 1, L0 // 3, 3, 0)])), N.KG_ERR_ARG, "CALL 1: outside its contig (0 <= x0 <= x1 <= L - 1 does not hold)"),
                (dict(sig=_sig([(0, -1, 2, 3, 0)])), N.KG_ERR_ARG, "CALL 0: outside its contig (0 <= x0 <= x1 <= L - 1 does not hold)"),
                (dict(sig=_sig([(0xFFFFFFFF, -(2 ** 31), 2 ** 31 - 1, -1, 0)])), N.KG_ERR_ARG, "CALL 0: container >= 6 * n_seqs")):
            assert call(**kw) == (code, text), kw
            assert db.live_device_bytes() == live
        with db.search_contigs(seq, off, target_fn=good_fn) as plain:
            st = N.KgResidualStats()
            assert lib.kg_residual_stats_of(plain._h, C.byref(st)) == N.KG_ERR_ARG
            assert lib.kg_last_error().decode() == "kg_residual_stats_of: the evidence was made without signature CALLs"
            buf = np.zeros(4, dtype=np.int64)
            for name in ("kg_residual_searched_copy", "kg_residual_explain_copy", "kg_residual_call_kinds_copy", "kg_residual_call_sources_copy"):
                assert getattr(lib, name)(plain._h, 0, 1, buf.ctypes.data) == N.KG_ERR_ARG
                assert lib.kg_last_error().decode() == name + ": the evidence was made without signature CALLs"
            assert not lib.kg_residual_searched_fragments(plain._h)
        with db.search_contigs(seq, off, target_fn=good_fn, explained_by=_sig([ok])) as ev:
            assert len(ev.calls) == 5
            buf = np.zeros(8, dtype=np.int64)
            assert lib.kg_residual_explain_copy(ev._h, 0, len(ev.explain) + 1, buf.ctypes.data) == N.KG_ERR_ARG
            assert lib.kg_last_error().decode() == "kg_residual_explain_copy: range outside the set"


def test_busy_is_the_search_s_answer(monkeypatch):
    from kmergutsjava_amd import hotpath
    tseq, toff, (seq, off) = _small()
    fn = np.arange(4, dtype=np.int32)
    with hotpath.SearchDb.build(tseq, toff) as db:
        live = db.live_device_bytes()
        monkeypatch.setenv("KG_TEST_SEARCHDB_REENTER", "1")
        with pytest.raises(N.KmerGutsNativeError) as e:
            db.search_contigs(seq, off, target_fn=fn, explained_by=_sig([(0, 1, 2, 3, 0)]))
        monkeypatch.delenv("KG_TEST_SEARCHDB_REENTER")
        assert e.value.code == N.KG_ERR_BUSY and "another call is in flight on this kg_searchdb" in str(e.value)
        assert db.live_device_bytes() == live
        with db.search_contigs(seq, off, target_fn=fn, explained_by=_sig([(0, 1, 2, 3, 0)])) as ev:
            assert len(ev.calls) == 5


def test_every_failing_allocation_is_nomem_and_leaves_the_handle_as_it_was(monkeypatch):
    import torch
    from kmergutsjava_amd import hotpath
    tseq, toff, (seq, off) = _small()
    fn = np.array([3, 2, 1, 0], dtype=np.int32)
    recs = hotpath.free_orfs(seq, off, min_res=30, start_codons=0)[0]
    sig = _plant(recs, off, [0, len(recs) - 1], count=2, fi=1)
    with hotpath.SearchDb.build(tseq, toff) as db:
        with db.search_contigs(seq, off, target_fn=fn, explained_by=sig, min_db_count=1) as ev:
            want = (ev.calls.copy(), ev.call_hits.copy(), ev.call_kind.copy())
            assert set(want[2].tolist()) == {0, 1}
        torch.cuda.synchronize()
        live, free = db.live_device_bytes(), torch.cuda.mem_get_info()[0]
        failed, got = 0, None
        for n in range(1, 900):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got = db.search_contigs(seq, off, target_fn=fn, explained_by=sig, min_db_count=1)
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert db.live_device_bytes() == live and torch.cuda.mem_get_info()[0] == free, n
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= 40 and got is not None
        with got:
            assert got.calls.tobytes() == want[0].tobytes() and got.call_hits.tobytes() == want[1].tobytes() and got.call_kind.tobytes() == want[2].tobytes()
        assert db.live_device_bytes() == live and torch.cuda.mem_get_info()[0] == free
