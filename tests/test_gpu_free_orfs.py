"""Evidence-free open reading frames on the GPU (kg_orfs_free / kg_orfset_add_free): records, prot_start and residues must equal
the model of tests/free_orfs_model.py byte for byte -- at the edges of the tile summaries (T = _native.ORF_TILE_CODONS), on both
strands and in every frame, wherever the start lies, at the min_res boundary, across contig borders, on random batches, behind
kg_orfs_regions and behind a DNA scan under both strategies, on the E. coli genome, and through the call_regions front end and
annotate; the selection over evidence + free ORFs leaves the evidence ORFs' states alone; errors carry their messages and failed
allocations leave nothing behind."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import free_orfs_model as F  # noqa: E402
import orfs_model as O  # noqa: E402
import select_model as S  # noqa: E402
import test_orfs_host as HO  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
T = N.ORF_TILE_CODONS
ROOT = os.path.dirname(HERE)


def _dev(seq, off, min_res=100, sc=7, dst="host", stats=None):
    from kmergutsjava_amd import hotpath
    o, ps, res = hotpath.free_orfs(seq, off, min_res, sc, device_out=dst == "device", stats=stats)
    if dst == "device":
        o, ps, res = o.cpu().numpy().view(N.ORF_DTYPE), ps.cpu().numpy(), res.cpu().numpy()
    return o, ps, res


def _same(got, want):
    for g, w, what in zip(got, want, ("records", "prot_start", "residues")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), what


def _batch(contigs):
    off = np.zeros(len(contigs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in contigs])
    return b"".join(contigs), off


def _planted(n_codons, stops=(), starts=(), strand=0, f=0, tail=0, fill=b"AAA"):
    """A contig whose strand `strand`, frame f reads `fill` everywhere but TAA at `stops` and ATG at `starts`, plus `tail` loose
    bases behind the last codon."""
    cod = [fill] * n_codons
    for j in stops:
        cod[j] = b"TAA"
    for j in starts:
        cod[j] = b"ATG"
    text = b"A" * f + b"".join(cod) + b"A" * tail
    return HO._rc(text) if strand else text


def _of(o, s, strand, f):
    return o[(o["seq"] == s) & (o["strand"] == strand) & (o["frame"] == f)]


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("f", [0, 1, 2])
def test_u_and_e_at_the_tile_edges(strand, f):
    """One run (u, e) per contig in a poly-A frame: u on the last codon of a tile, the first of the next, inside one and absent,
    e at distances that span 0, 1, 2 and 3 tile borders.  With start_codons = 0 the run's candidate is codons u + 1 .. e whenever
    it is long enough; the runs in front of u and behind e are candidates of their own."""
    contigs, want = [], []
    for u in (T - 1, T, 5, 2 * T - 1, -1):
        for d in (1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 1):
            e = u + d
            n = e + 1 + d % 3
            c = _planted(n, stops=(u, e) if u >= 0 else (e,), strand=strand, f=f, tail=(d + u) % 3)
            xs, xe = f + 3 * (u + 1), f + 3 * e + 2
            want.append(((xs, xe) if not strand else (len(c) - 1 - xe, len(c) - 1 - xs), d - 1))
            contigs.append(c)
    seq, off = _batch(contigs)
    for min_res in (1, T - 2, T, 2 * T):
        got = _dev(seq, off, min_res, 0)
        _same(got, F.free_orfs(seq, off, min_res, 0))
        for s, ((left, right), n_res) in enumerate(want):
            mine = _of(got[0], s, strand, f)
            hit = mine[(mine["left"] == left) & (mine["right"] == right)]
            assert len(hit) == (1 if n_res >= min_res else 0), (s, min_res)
            if len(hit):
                assert hit["n_res"][0] == n_res and hit["flags"][0] & O.HAS_STOP
    _same(_dev(seq, off, 3, 7), F.free_orfs(seq, off, 3, 7))


@pytest.mark.parametrize("strand", [0, 1])
def test_where_the_start_lies(strand):
    """u = 3, e = 6T + 40, a second stop at e2 = e + T + 50.  The start in u's tile, in the following tile, several tiles on
    (found by the scanned key), two of them (the first wins), and only behind e: then (u, e) gives nothing and the start belongs
    to the next run alone."""
    u, e = 3, 6 * T + 40
    e2 = e + T + 50
    contigs, want = [], []
    for starts in ([10], [T + 7], [4 * T + 9], [5 * T + 120, 6 * T + 1], [T - 1, T], [e - 1], [e + 5], [u + 1]):
        contigs.append(_planted(e2 + 3, stops=(u, e, e2), starts=starts, strand=strand, f=2, tail=1, fill=b"CCC"))
        first = [x for x in starts if x < e]
        want.append([e - min(first)] if first else [])
        behind = [x for x in starts if x > e]
        want[-1] += [e2 - min(behind)] if behind else []
    seq, off = _batch(contigs)
    got = _dev(seq, off, 1, 1)
    _same(got, F.free_orfs(seq, off, 1, 1))
    for s, w in enumerate(want):
        mine = _of(got[0], s, strand, 2)
        # (-1, u) has no start: partial5 from codon 0, three residues; the run behind e2 holds two codons and no start
        assert mine["n_res"].tolist() == [3] + w, s
        assert (mine["start_codon"][1:] == 1).all() and mine["start_codon"][0] == 0 and mine["flags"][0] == F.FREE | O.HAS_STOP | O.PARTIAL5
    for min_res, sc in ((40, 7), (T + 45, 1), (1, 6), (1, 0)):
        _same(_dev(seq, off, min_res, sc), F.free_orfs(seq, off, min_res, sc))


@pytest.mark.parametrize("strand", [0, 1])
def test_length_edges_across_a_tile_border(strand):
    """n_res of min_res - 1, min_res and min_res + 1 with the border between b and e, with and without a start search."""
    min_res = 10
    contigs = []
    for n_res in (min_res - 1, min_res, min_res + 1):
        for b in (T - 4, T - 1, T - min_res, 2 * T - 9):
            contigs.append(_planted(b + n_res + 2, stops=(b - 2, b + n_res), starts=(b,), strand=strand, f=1, fill=b"CCC"))
    seq, off = _batch(contigs)
    got = _dev(seq, off, min_res, 7)
    _same(got, F.free_orfs(seq, off, min_res, 7))
    found = [int(((_of(got[0], s, strand, 1)["start_codon"] == 1)).sum()) for s in range(len(contigs))]
    assert found == [0] * 4 + [1] * 8
    # without a start search the run begins one codon earlier: min_res - 1 passes too
    got = _dev(seq, off, min_res, 0)
    _same(got, F.free_orfs(seq, off, min_res, 0))
    assert [int((_of(got[0], s, strand, 1)["n_res"] == k).sum()) for s, k in ((0, min_res), (4, min_res + 1), (8, min_res + 2))] == [1, 1, 1]


def test_every_stop_owns_a_candidate_at_min_res_one():
    """Alternating ATG TAA over several tiles: the densest case.  '+' frame 0 holds one candidate "M" per pair, in order."""
    pairs = 2 * T + 3
    c = b"ATGTAA" * pairs
    seq, off = _batch([c, HO._rc(c), b"A" + c])
    got = _dev(seq, off, 1, 7)
    _same(got, F.free_orfs(seq, off, 1, 7))
    for s, strand, f in ((0, 0, 0), (1, 1, 0), (2, 0, 1)):
        mine = _of(got[0], s, strand, f)
        assert len(mine) == pairs and (mine["n_res"] == 1).all() and (mine["start_codon"] == 1).all()
        key = mine["left"] if not strand else -mine["left"]
        assert (np.diff(key) == 6).all()
    assert bytes(got[2][:pairs]) == b"M" * pairs
    _same(_dev(seq, off, 1, 0), F.free_orfs(seq, off, 1, 0))
    _same(_dev(seq, off, 2, 7), F.free_orfs(seq, off, 2, 7))


def test_stopless_contig_and_the_smallest_contigs():
    n = 3 * T + 2
    body = b"ACC" * n                       # T, P, H / G, W, V: no stop in any frame of either strand
    contigs = [body, b"", b"A", b"AC", b"ATG", b"ATGA", b"TAAAT", b"TAAATG", b"CATTTAC", b"ACGTACGT", b"N" * 40, b"ATGCCC", b"ACC" * 1000,
               b"TAA", b"TTATTA", body + b"AC"]
    seq, off = _batch(contigs)
    for min_res, sc in ((1, 7), (2, 7), (1, 0), (3, 1), (n, 0), (n - 1, 0)):
        got = _dev(seq, off, min_res, sc)
        _same(got, F.free_orfs(seq, off, min_res, sc))
    first = got[0][got[0]["seq"] == 0]
    assert len(first) == 6 and (first["flags"] == F.FREE | O.PARTIAL5).all() and sorted(first["n_res"].tolist()) == [n - 1] * 4 + [n] * 2
    assert list(zip(first["strand"].tolist(), first["frame"].tolist())) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]


def test_segments_do_not_leak_across_contigs_strands_or_frames():
    """Neighbouring contigs end and begin with stops and starts of both strands in every frame; the contigs between hold none, so
    each gives its six whole frames, with PARTIAL5 and without HAS_STOP and a start."""
    edges = [b"TAA", b"TAG", b"TGA", b"TTA", b"CTA", b"TCA", b"ATG", b"CAT"]
    body = b"ACC" * (T + 3)
    contigs, plain = [], []
    for k in range(16):
        edge = edges[k % 8]
        if k % 2:
            contigs.append(body + b"C" * (k % 4))
            plain.append(k)
        else:
            contigs.append(edge * 2 + body[:k] + edge * 3 + b"A" * (k % 3))
    seq, off = _batch(contigs)
    for min_res, sc in ((T, 7), (1, 7), (1, 0)):
        got = _dev(seq, off, min_res, sc)
        _same(got, F.free_orfs(seq, off, min_res, sc))
        for k in plain if sc == 0 else []:      # (the '-' strand of the body reads GTG: with a start search b may move)
            mine = got[0][got[0]["seq"] == k]
            L = len(contigs[k])
            assert mine["n_res"].tolist() == [(L - f) // 3 for f in (0, 1, 2)] * 2
            assert (mine["flags"] == F.FREE | O.PARTIAL5).all() and (mine["start_codon"] == 0).all()
    # a stop of frame 1 only: frames 0 and 2 do not see it, nor does the other strand
    c = b"A" + _planted(3 * T, stops=(T + 1,))
    got = _dev(c, np.array([0, len(c)], np.int64), 1, 0)
    _same(got, F.free_orfs(c, np.array([0, len(c)], np.int64), 1, 0))
    assert [len(_of(got[0], 0, s, f)) for s in (0, 1) for f in (0, 1, 2)] == [1, 2, 1, 1, 1, 1]


def test_one_long_run_beside_ten_thousand_one_codon_runs():
    """The bounded-work case: no lane's work grows with the 10^5 codons of the long run, and the 10^4 stops beside it each own
    their one-codon candidate."""
    contigs = [b"ACC" * 100_000, b"AAATAA" * 10_000]
    seq, off = _batch(contigs)
    st = {}
    got = _dev(seq, off, 1, 0, stats=st)
    want = F.free_orfs(seq, off, 1, 0)
    _same(got, want)
    assert st["orfs"] == len(want[0]) >= 10_006 and st["residues"] == len(want[2]) >= 600_000
    assert 0 < st["ms"] < 1000, st
    print("balance: %d candidates, %d residues, %.3f ms on the device" % (st["orfs"], st["residues"], st["ms"]))


@pytest.mark.parametrize("seed", range(24))
def test_random_batches_equal_the_model(seed):
    rng = np.random.default_rng(2000 + seed)
    weights = [None, np.array([30, 10, 10, 30, 2, 2, 2, 2, 2, 5, 5], float) / 100,
               np.array([4, 44, 44, 4, 0, 1, 1, 1, 0, 1, 0], float) / 100][seed % 3]         # the last: GC-rich, stops far apart
    _, seq, off = O.random_batch(rng, int(rng.choice([1, 7, 60])), max_len=int(rng.choice([30, 500, 5 * 3 * T])), max_regions=0,
                                 weights=weights)
    sc = [7, 1, 0, 5][seed % 4]
    for min_res in (1, int(rng.choice([2, 5, 30, T]))):
        want = F.free_orfs(seq, off, min_res, sc)
        for dst in ("host", "device"):
            st = {}
            _same(_dev(seq, off, min_res, sc, dst, st), want)
            fl = want[0]["flags"]
            assert st["orfs"] == len(want[0]) and st["residues"] == len(want[2]) and st["interrupted"] == 0
            assert st["partial5"] == ((fl & O.PARTIAL5) != 0).sum()
            assert st["complete"] == (((fl & O.HAS_STOP) != 0) & (want[0]["start_codon"] != 0)).sum()


def test_empty_inputs():
    for seq, off in ((b"", np.zeros(1, np.int64)), (b"ACGTACGT", np.array([0, 2, 2, 4], np.int64))):
        o, ps, res = _dev(seq, off, 1)
        assert len(o) == 0 and ps.tolist() == [0] and len(res) == 0


def test_a_contigs_records_are_the_same_alone_as_in_a_batch():
    rng = np.random.default_rng(78)
    _, seq, off = O.random_batch(rng, 40, max_len=4 * 3 * T, max_regions=0)
    whole = _dev(seq, off, 4)
    for s in range(0, 40, 3):
        idx = np.flatnonzero(whole[0]["seq"] == s)
        o, ps, res = _dev(seq[off[s]:off[s + 1]], np.array([0, off[s + 1] - off[s]], np.int64), 4)
        o["seq"] = s
        assert o.tobytes() == whole[0][idx].tobytes()
        assert bytes(res) == bytes(whole[2][whole[1][idx[0]]:whole[1][idx[-1] + 1]] if len(idx) else b"")


# ---- kg_orfset_add_free -------------------------------------------------------------------------------------------------------

def _add_free(oh, seq, off, min_res, sc=7):
    """kg_orfset_add_free on an open ORF set -> the new set's handle"""
    lib, out = N.load(), C.c_void_p()
    sb = np.frombuffer(seq, dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq
    N.check(lib.kg_orfset_add_free(oh, C.byref(N.KgFreeParams(min_res, sc, 0)), sb.ctypes.data if sb.size else None, 0,
                                   off.ctypes.data, len(off) - 1, C.byref(out)))
    return out


def _select(oh, mo=60, pct=50):
    from kmergutsjava_amd import hotpath
    sh = C.c_void_p()
    N.check(N.load().kg_orfset_select(oh, C.byref(N.KgSelectParams(mo, pct, 0)), C.byref(sh)))
    return hotpath._take_selectset(sh, False)[0]


def test_add_free_behind_caller_held_regions():
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(5)
    w = np.array([4, 44, 44, 4, 0, 1, 1, 1, 0, 1, 0], float) / 100
    regs, seq, off = O.random_batch(rng, 30, max_len=5 * 3 * T, max_regions=6, weights=w)
    lib, oh = N.load(), C.c_void_p()
    for only_kept in (1, 0):
        parent = O.orfs(regs, seq, off, 7, bool(only_kept))
        free = F.free_orfs(seq, off, 20, 3)
        assert len(free[0]) > 10 and len(parent[0]) > 10
        N.check(lib.kg_orfs_regions(0, C.byref(N.KgOrfParams(7, only_kept, 0)), regs.ctypes.data, len(regs), seq.ctypes.data, off.ctypes.data,
                                    len(off) - 1, C.byref(oh)))
        try:
            both = _add_free(oh, seq, off, 20, 3)
            try:
                ev_sel = _select(oh)
                sel = _select(both)
                st = N.KgOrfStats()
                N.check(lib.kg_orfset_stats(both, C.byref(st)))
            finally:
                got = hotpath._take_orfset(both, False)
            _same(got[:3], F.concat(parent, free))
            assert got[0][:len(regs)].tobytes() == parent[0].tobytes() and got[0][len(regs):].tobytes() == free[0].tobytes()
            assert st.orfs == len(regs) + len(free[0]) and st.residues == len(parent[2]) + len(free[2])
            assert st.interrupted == ((parent[0]["flags"] & O.INTERRUPTED) != 0).sum()
            assert sel.tobytes() == S.select_fast(S.of_records(got[0])).tobytes()
            assert sel[:len(regs)].tobytes() == ev_sel.tobytes() == S.select_fast(S.of_records(parent[0])).tobytes()
        finally:
            _same(hotpath._take_orfset(oh, False)[:3], parent)          # the given set stayed valid and unchanged


@pytest.fixture(params=["direct", "partitioned"])
def strategy(request, monkeypatch):
    monkeypatch.setenv("KG_PARTITION", "0" if request.param == "direct" else "1")
    monkeypatch.setenv("KG_DIRECT_FILTER", "2")
    return request.param


_WORK = {}


def _workload():
    if not _WORK:
        _WORK["w"] = HO.planted_orf_contigs()
    return _WORK["w"]


def _planted_genes_found(orfs, ps, res, genes):
    """the unshifted planted genes that have a free candidate on their strand that ends on the planted stop and whose protein
    ends with the planted one, and how many unshifted genes there are"""
    text = res.tobytes().decode()
    free = np.flatnonzero((orfs["flags"] & F.FREE) != 0)
    found = total = 0
    for c, left, right, strand, _, shifted, prot in genes:
        if shifted:
            continue
        total += 1
        o = orfs[free]
        hit = free[(o["seq"] == c) & (o["strand"] == strand) & ((o["left"] if strand else o["right"]) == (left if strand else right)) &
                   ((o["flags"] & O.HAS_STOP) != 0)]
        found += any(text[ps[k]:ps[k + 1]].endswith(prot) for k in hit)
    return found, total


def test_add_free_behind_a_scan_and_the_selection(strategy):
    from kmergutsjava_amd import hotpath
    img, dna, off, genes = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    d_seq = torch.from_numpy(sb.copy()).cuda()
    torch.cuda.synchronize()
    free = F.free_orfs(dna, off, 100, 7)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        live0 = tab.live_device_bytes()
        for ptr in (None, d_seq.data_ptr()):
            with tab.scan(None if ptr else sb, off, hotpath.Params(), device_ptr=ptr) as r:
                live1 = tab.live_device_bytes()
                for only_kept in (True, False):
                    ev = r.orfs(None if ptr else sb, off, 300, 10, 90, only_kept=only_kept, device_ptr=ptr)
                    ev_stats = dict(r.orf_stats)
                    got = r.orfs(None if ptr else sb, off, 300, 10, 90, only_kept=only_kept, device_ptr=ptr, free_min_res=100)
                    assert got[0].tobytes() == ev[0].tobytes() and got[1].tobytes() == ev[1].tobytes() and len(ev[0]) > 20
                    _same(got[2:], F.concat(ev[2:], free))
                    assert r.orf_stats["orfs"] == len(ev[2]) + len(free[0]) and r.orf_stats["interrupted"] == ev_stats["interrupted"]
                    assert r.orf_stats["complete"] == ev_stats["complete"] + int(((free[0]["flags"] & O.HAS_STOP != 0) & (free[0]["start_codon"] != 0)).sum())
                    assert tab.live_device_bytes() == live1
                ev_sel = r.select(off, None if ptr else sb, 300, 10, 90, orfs=True, device_ptr=ptr)
                sel = r.select(off, None if ptr else sb, 300, 10, 90, orfs=True, device_ptr=ptr, free_min_res=100)
                n = len(ev_sel[0])
                assert all(a.tobytes() == b.tobytes() for a, b in zip(sel[:2], ev_sel[:2]))
                _same(sel[2:5], F.concat(ev_sel[2:5], free))
                assert sel[5].tobytes() == S.select_fast(S.of_records(sel[2])).tobytes()
                assert sel[5][:n].tobytes() == ev_sel[5].tobytes()              # the evidence states and winners stay
                assert r.select_stats["candidates"] == n + len(free[0]) and tab.live_device_bytes() == live1
                with pytest.raises(ValueError):
                    r.select(off, free_min_res=100)
        assert tab.live_device_bytes() == live0
    found, total = _planted_genes_found(sel[2], sel[3], sel[4], genes)
    assert (found, total) == (80, 80)


def test_ecoli_genome_equals_the_model_and_is_selected():
    from kmergutsjava_amd import hotpath
    from kmergutsjava_amd.make_signatures import parse_fasta
    _, contigs = parse_fasta(gzip.decompress(open(os.path.join(HERE, "golden", "Ecoli_K12_W3110.fna.gz"), "rb").read()))
    seq, off = _batch(contigs)
    want = F.free_orfs(seq, off)
    lib, oh = N.load(), C.c_void_p()
    sb = np.frombuffer(seq, dtype=np.uint8)
    N.check(lib.kg_orfs_free(0, C.byref(N.KgFreeParams(100, 7, 0)), sb.ctypes.data, 0, off.ctypes.data, len(off) - 1, C.byref(oh)))
    try:
        sel = _select(oh)
    finally:
        st = N.KgOrfStats()
        lib.kg_orfset_stats(oh, C.byref(st))
        got = hotpath._take_orfset(oh, False)
    _same(got[:3], want)
    print("E. coli: %d nt, %d free candidates, %d residues, %d selected, %.3f ms on the device" %
          (len(seq), len(want[0]), len(want[2]), int((sel["state"] == 1).sum()), st.ms))
    assert 7000 < len(want[0]) < 8500
    assert sel.tobytes() == S.select_fast(S.of_records(got[0])).tobytes() and (sel["state"] == 1).sum() > 3000


# ---- errors ---------------------------------------------------------------------------------------------------------------------

def test_errors_and_their_messages():
    from kmergutsjava_amd import hotpath
    seq, off = _batch([HO.A, b"ACGTACGTAC"])
    sb = np.frombuffer(seq, dtype=np.uint8)
    assert len(_dev(seq, off, 1)[0]) > 0

    def err(s=seq, o=off, **kw):
        with pytest.raises(N.KmerGutsNativeError) as ei:
            hotpath.free_orfs(s, o, **kw)
        return ei.value

    for kw, word in (({"min_res": 0}, "min_res"), ({"min_res": -5}, "min_res"), ({"start_codons": 8}, "start_codons"),
                     ({"start_codons": -1}, "start_codons")):
        e = err(**kw)
        assert e.code == N.KG_ERR_ARG and word in str(e), str(e)
    e = err(o=np.array([0, 30, 20], np.int64))
    assert e.code == N.KG_ERR_ARG and "contig 1" in str(e)
    lib, h, h2 = N.load(), C.c_void_p(), C.c_void_p()
    good = N.KgFreeParams(1, 7, 0)
    args = (sb.ctypes.data, 0, off.ctypes.data, len(off) - 1)
    assert lib.kg_orfs_free(0, C.byref(N.KgFreeParams(1, 7, 1)), *args, C.byref(h)) == N.KG_ERR_ARG and b"reserved" in lib.kg_last_error()
    assert lib.kg_orfs_free(0, None, *args, C.byref(h)) == N.KG_ERR_ARG and b"kg_free_params" in lib.kg_last_error()
    assert lib.kg_orfs_free(0, C.byref(good), None, 0, off.ctypes.data, len(off) - 1, C.byref(h)) == N.KG_ERR_ARG and b"sequence" in lib.kg_last_error()
    assert lib.kg_orfs_free(0, C.byref(good), sb.ctypes.data, 0, None, len(off) - 1, C.byref(h)) == N.KG_ERR_ARG
    assert lib.kg_orfs_free(0, C.byref(good), *args, None) == N.KG_ERR_ARG
    assert lib.kg_orfset_add_free(None, C.byref(good), *args, C.byref(h)) == N.KG_ERR_ARG and b"kg_orfset" in lib.kg_last_error()
    assert not h.value
    N.check(lib.kg_orfs_free(0, C.byref(good), *args, C.byref(h)))
    try:
        assert lib.kg_orfset_add_free(h, C.byref(good), *args, None) == N.KG_ERR_ARG
        assert lib.kg_orfset_add_free(h, C.byref(N.KgFreeParams(0, 7, 0)), *args, C.byref(h2)) == N.KG_ERR_ARG and b"min_res" in lib.kg_last_error()
        assert lib.kg_orfset_add_free(h, C.byref(good), sb.ctypes.data, 0, off.ctypes.data, len(off) - 2, C.byref(h2)) == N.KG_ERR_ARG
        assert b"n_seqs" in lib.kg_last_error() and not h2.value
        # a free set is an ORF set: free candidates behind free candidates
        N.check(lib.kg_orfset_add_free(h, C.byref(good), *args, C.byref(h2)))
        twice = hotpath._take_orfset(h2, False)
        once = F.free_orfs(seq, off, 1, 7)
        _same(twice[:3], F.concat(once, once))
    finally:
        lib.kg_orfset_free(h)


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(4)
    _, seq, off = O.random_batch(rng, 50, max_len=3000, max_regions=0)
    want = F.free_orfs(seq, off, 10)
    img, dna, doff, _ = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(sb, doff, hotpath.Params()) as r:
        want_r = r.orfs(sb, doff, free_min_res=100)
        assert len(want_r[2]) > 80
        _same(_dev(seq, off, 10), want)             # once first: what the runtime sets up on first use is not counted
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        live0 = tab.live_device_bytes()
        for which in ("alone", "result"):
            failed = 0
            for n in range(1, 200):
                monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
                try:
                    got = _dev(seq, off, 10) if which == "alone" else r.orfs(sb, doff, free_min_res=100)
                    break
                except N.KmerGutsNativeError as e:
                    assert e.code == N.KG_ERR_NOMEM, e
                    failed += 1
                    assert tab.live_device_bytes() == live0
                    if which == "alone":
                        assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
            monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
            assert failed >= 15
            if which == "alone":
                _same(got, want)
            else:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want_r))
            assert tab.live_device_bytes() == live0


# ---- the front end --------------------------------------------------------------------------------------------------------------

def test_call_regions_free_orfs_select_and_annotate(tmp_path):
    """call_regions --orfs --faa --free-orfs --select on the planted contigs writes what the model and the writers give, every
    unshifted planted gene's stop is in the gene set, annotate reads the protein file, and without --free-orfs the output is
    what a run without the flag gives."""
    from kmergutsjava_amd import annotate as AN
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
        return p.stdout.strip(), [(tmp_path / (tag + ext)).read_bytes() for ext in (".tsv", ".orfs", ".faa")]

    # the records the front end works on, from the library calls the other tests have checked against the models
    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(np.frombuffer(dna, np.uint8), off, hotpath.Params(min_hits=4)) as r:
        regs, start, orfs, ps, res, sel = r.select(off, dna, 300, 12, 100, orfs=True, free_min_res=100)
        ev = r.select(off, dna, 300, 12, 100, orfs=True)
    nr = len(regs)
    free = F.free_orfs(dna, off)
    _same((orfs[nr:], ps[nr:] - ps[nr], res[ps[nr]:]), free)
    line, files = run("sel", "--select", "--free-orfs")
    want_line = CR.summary_of(regs, start) + CR.orf_summary(orfs[:nr]) + CR.select_summary(sel) + ", free: %d" % len(free[0])
    assert line == want_line
    assert files[0] == CR.format_regions(ids, regs, fnames, sel=sel[:nr], cands=orfs)
    fps = ps[nr:] - ps[nr]
    assert files[1] == CR.format_orfs(ids, regs, orfs[:nr], fnames, sel=sel[:nr], free=orfs[nr:], free_sel=sel[nr:], cands=orfs)
    assert files[2] == CR.format_faa(ids, regs, orfs[:nr], ps[:nr + 1], res[:ps[nr]], fnames, sel=sel[:nr], free=orfs[nr:], free_sel=sel[nr:],
                                     free_prot_start=fps, free_residues=res[ps[nr]:])
    assert files[1].count(b"hypothetical protein") == int((sel["state"][nr:] == 1).sum()) > 0 and b",free\n" in files[1]
    assert files[2].count(b" hypothetical protein\n") > 0
    # every unshifted planted gene's stop is the end of a written line (an evidence ORF or a free one)
    ends = set()
    for row in files[1].splitlines():
        f = row.split(b"\t")
        ends.add((f[0], int(f[1]) - 1 if f[3] == b"-" else int(f[2]) - 1, f[3]))
    have = sum((ids[c], left if strand else right, b"-" if strand else b"+") in ends for c, left, right, strand, _, shifted, _ in genes if not shifted)
    print("planted unshifted genes whose stop ends a line of the selected gene set: %d of 80" % have)
    # --all: every candidate with its status; without --select: every free ORF
    line_all, files_all = run("all", "--select", "--free-orfs", "--all", "--min-res", "100")
    assert files_all[1].count(b"hypothetical protein") == len(free[0]) and b"\toverlapped\t" in files_all[1]
    line_ns, files_ns = run("ns", "--free-orfs")
    assert files_ns[1].count(b"hypothetical protein") == len(free[0]) and line_ns.endswith(", free: %d" % len(free[0]))
    # without the flag: what it was
    line0, files0 = run("plain", "--select")
    assert line0 == CR.summary_of(regs, start) + CR.orf_summary(ev[2]) + CR.select_summary(ev[5])
    assert files0[0] == CR.format_regions(ids, regs, fnames, sel=ev[5], cands=ev[2]) and files0[1] == CR.format_orfs(ids, regs, ev[2], fnames, sel=ev[5])
    assert files0[2] == CR.format_faa(ids, regs, ev[2], ev[3], ev[4], fnames, sel=ev[5])
    assert b"hypothetical" not in files0[1] + files0[2]
    # --free-orfs needs --orfs or --faa
    p = subprocess.run(base + ["-o", str(tmp_path / "x.tsv"), "--free-orfs"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode != 0 and "--free-orfs" in p.stderr
    # annotate reads the protein file: every id once
    AN.annotate(str(d), str(tmp_path / "sel.faa"), str(tmp_path / "a.tsv"), min_hits=4, write_all=True)
    pids = [b.partition(b"\n")[0].partition(b" ")[0] for b in files[2].split(b">")[1:]]
    seen = [row.split(b"\t")[0] for row in (tmp_path / "a.tsv").read_bytes().splitlines()]
    assert len(set(pids)) == len(pids) and set(seen) == set(pids)
