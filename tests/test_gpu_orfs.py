"""Open reading frames on the GPU (kg_regionset_orfs / kg_orfs_regions): records, prot_start and residues must equal the numpy
model of tests/orfs_model.py byte for byte -- at the edges of the tile summaries (T = _native.ORF_TILE_CODONS), on both strands
and in every frame, across contig borders, on random batches, behind a DNA scan under both strategies, and through the
call_regions front end and annotate; errors name the region and failed allocations leave nothing behind.

The 2^32-residue limit is met through kg_orfs_regions, whose regions may overlap: 2048 regions inside one stop-free frame of
2^21 codons are 2048 ORFs of 2^21 residues, which fill one chunk of the prefix sum (tests/scan_model.py) with exactly 2^32.
prot_start is held to the cumulative sum at the region counts where the prefix sum's chunks and the carry loop over them end.

The free ORFs (kg_orfs_free, kg_orfset_add_free) and kg_regionset_repair have the same limit behind the same prefix sum and are
left out: their records are found by the kernels, an ORF per closing stop and a repaired protein per region, so at most about
six of them -- one per frame and strand -- cover any position, and 2048 neighbours that hold 2^32 residues need gigabases of
input."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import orfs_model as O  # noqa: E402
import regions_model as R  # noqa: E402
import scan_model as SM  # noqa: E402
import test_orfs_host as HO  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
T = N.ORF_TILE_CODONS
ROOT = os.path.dirname(HERE)


def _dev(regs, seq, off, sc=7, ok=True, dst="host", stats=None):
    from kmergutsjava_amd import hotpath
    o, ps, res = hotpath.orf_regions(regs, seq, off, sc, ok, device_out=dst == "device", stats=stats)
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


def _planted(n_codons, stops=(), starts=(), strand=0, f=0, tail=0):
    """A contig whose strand `strand`, frame f reads AAA everywhere but TAA at `stops` and ATG at `starts`, plus `tail` loose
    bases behind the last codon."""
    cod = [b"AAA"] * n_codons
    for j in stops:
        cod[j] = b"TAA"
    for j in starts:
        cod[j] = b"ATG"
    text = b"A" * f + b"".join(cod) + b"A" * tail
    return HO._rc(text) if strand else text


DISTANCES = (1, T - 1, T, T + 1, 2 * T + 1)


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("f", [0, 1, 2])
def test_stop_distances_at_the_tile_edges(strand, f):
    """Poly-A contigs with one stop in front of the region and one behind it, at every pair of distances of DISTANCES, with the
    front stop on the first codon of a tile, on the last one and inside one: the ORF runs from u + 1 to e whatever tiles lie
    between."""
    contigs, rows, want = [], [], []
    for base in (0, T - 1, T, 5):
        for du in DISTANCES:
            for de in DISTANCES:
                u, j0 = base, base + du
                j1 = j0 + 2
                e = j1 + de
                n = e + 1 + (du + de) % 3                   # the stop is the last codon or nearly
                c = _planted(n, stops=(u, e), strand=strand, f=f, tail=(du + base) % 3)
                rows.append(O.codon_region(len(c), strand, f, j0, j1, seq=len(contigs)))
                xs, xe = f + 3 * (u + 1), f + 3 * e + 2
                want.append((xs, xe) if not strand else (len(c) - 1 - xe, len(c) - 1 - xs))
                contigs.append(c)
    seq, off = _batch(contigs)
    regs = O.regions_of(rows)
    got = _dev(regs, seq, off)
    assert list(zip(got[0]["left"].tolist(), got[0]["right"].tolist())) == want
    assert (got[0]["flags"] == O.HAS_STOP).all() and (got[0]["start_codon"] == 0).all()
    _same(got, O.orfs(regs, seq, off))


@pytest.mark.parametrize("strand", [0, 1])
def test_stop_on_the_first_and_last_codon_of_a_tile_behind_the_region(strand):
    """e exactly on the first and on the last codon of a tile, the region ending right in front of it and a tile away."""
    contigs, rows = [], []
    for e in (T, 2 * T - 1, 2 * T, 3 * T - 1):
        for j1 in (e - 1, e - T, max(e - T - 1, 0), 0):
            c = _planted(e + 2, stops=(e,), strand=strand, f=1)
            rows.append(O.codon_region(len(c), strand, 1, max(j1 - 1, 0), j1, seq=len(contigs)))
            contigs.append(c)
    seq, off = _batch(contigs)
    regs = O.regions_of(rows)
    got = _dev(regs, seq, off)
    assert (got[0]["flags"] == (O.HAS_STOP | O.PARTIAL5)).all()
    _same(got, O.orfs(regs, seq, off))


@pytest.mark.parametrize("strand", [0, 1])
def test_starts_in_the_tile_of_u_between_and_in_the_tile_of_j0(strand):
    u, j0 = 3, 2 * T + 5
    places = {"u": 10, "between": T + 7, "j0": 2 * T + 2, "behind j0": 2 * T + 6}
    contigs, rows, want_b = [], [], []
    for names in (["u"], ["between"], ["j0"], ["behind j0"], ["between", "j0"], ["u", "between", "j0"], ["j0", "behind j0"], []):
        starts = [places[k] for k in names]
        c = _planted(3 * T, stops=(u, 2 * T + 40), starts=starts, strand=strand, f=2, tail=1)
        rows.append(O.codon_region(len(c), strand, 2, j0, j0 + 3, seq=len(contigs)))
        ok = [s for s in starts if s <= j0]
        want_b.append(min(ok) if ok else u + 1)
        contigs.append(c)
    seq, off = _batch(contigs)
    regs = O.regions_of(rows)
    got = _dev(regs, seq, off)
    assert got[0]["n_res"].tolist() == [2 * T + 40 - b for b in want_b]
    assert got[0]["start_codon"].tolist() == [1, 1, 1, 0, 1, 1, 1, 0]
    _same(got, O.orfs(regs, seq, off))
    for sc in (0, 6):                       # ATG is not asked for
        g = _dev(regs, seq, off, sc=sc)
        assert (g[0]["start_codon"] == 0).all()
        _same(g, O.orfs(regs, seq, off, sc))


def test_stopless_contig_and_the_smallest_contigs():
    """3T + 2 codons without a stop (and one of N's), contigs with n_f = 0, 1, 2, regions on the first and on the last codon."""
    n = 3 * T + 2
    contigs = [_planted(n, f=0, tail=2), _planted(n, strand=1, f=1), b"N" * (3 * n), b"", b"A", b"AC", b"ATG", b"ATGA", b"TAAATG",
               b"CATTTA", b"ACGTACGT", _planted(n, stops=(0, n - 1))]
    rows = []
    for s, strand, f in ((0, 0, 0), (1, 1, 1), (2, 0, 2), (2, 1, 0)):
        L = len(contigs[s])
        nf = (L - f) // 3
        rows += [O.codon_region(L, strand, f, a, b, seq=s) for a, b in ((0, 0), (nf - 1, nf - 1), (T, T + 1), (T - 1, T), (0, nf - 1))]
    rows += [O.region(6, 0, 0, 2, 0), O.region(6, 1, 0, 2, 0), O.region(7, 0, 1, 3, 1), O.region(7, 0, 0, 3, 0),
             O.region(8, 0, 0, 2, 0), O.region(8, 0, 3, 5, 0), O.region(8, 0, 0, 5, 0), O.region(9, 1, 0, 2, 0), O.region(9, 1, 3, 5, 0),
             O.region(10, 0, 2, 7, 2), O.region(10, 1, 0, 6, 1)]
    L = len(contigs[11])
    rows += [O.codon_region(L, 0, 0, 0, 0, seq=11), O.codon_region(L, 0, 0, n - 1, n - 1, seq=11), O.codon_region(L, 0, 0, 1, n - 2, seq=11)]
    seq, off = _batch(contigs)
    regs = O.regions_of(rows)
    for sc in (7, 1):
        got = _dev(regs, seq, off, sc=sc)
        _same(got, O.orfs(regs, seq, off, sc))
    o = got[0]
    assert (o["flags"][:20] == O.PARTIAL5).all() and (o["n_res"][:5] == n).all() and o["n_res"][4] == n
    assert bytes(got[2][:n]) == b"K" * n and bytes(got[2][got[1][10]:got[1][11]]) == b"X" * (n - 1)


def test_segments_do_not_leak_across_contigs_strands_or_frames():
    """Neighbouring contigs end and begin with stops (of both strands, in every frame); the contigs between hold none, so every
    ORF on them is the whole frame, with PARTIAL5 and without HAS_STOP."""
    stops_f = [b"TAA", b"TAG", b"TGA"]
    stops_r = [b"TTA", b"CTA", b"TCA"]
    body = b"ACC" * (T + 3)                  # T, P, H / G, W, V: no stop in any frame of either strand
    contigs, rows, plain = [], [], []
    for k in range(12):
        edge = (stops_f + stops_r)[k % 6]
        contigs.append(body[:k] + edge * 3 + b"A" * (k % 3) if k % 2 == 0 else body + b"C" * (k % 4))
        if k % 2:
            L = len(contigs[-1])
            for strand in (0, 1):
                for f in (0, 1, 2):
                    nf = (L - f) // 3
                    for j in (0, nf - 1, T):
                        rows.append(O.codon_region(L, strand, f, j, j, seq=k))
                        plain.append(nf)
        else:
            contigs[-1] = edge * 2 + contigs[-1]
    seq, off = _batch(contigs)
    regs = O.regions_of(rows)
    got = _dev(regs, seq, off, sc=0)
    assert got[0]["n_res"].tolist() == plain and (got[0]["flags"] == O.PARTIAL5).all()
    _same(got, O.orfs(regs, seq, off, 0))
    # a stop of frame 1 only: frames 0 and 2 do not see it, nor does the other strand
    c = b"A" + _planted(3 * T, stops=(T + 1,))
    regs = O.regions_of([O.codon_region(len(c), s, f, 2, 3) for s in (0, 1) for f in (0, 1, 2)])
    got = _dev(regs, c, np.array([0, len(c)], np.int64))
    assert [bool(x & O.HAS_STOP) for x in got[0]["flags"]] == [False, True, False, False, False, False]
    _same(got, O.orfs(regs, c, np.array([0, len(c)], np.int64)))


def test_one_long_orf_beside_ten_thousand_one_codon_orfs():
    n_long = 30_000
    contigs = [b"TAAAAATAA"] * 5000 + [_planted(n_long, strand=1, f=1)] + [b"TAAAAATAA"] * 5000
    rows = [O.region(s, 0, 3, 5, 0, kept=int(s % 7 != 0)) if s != 5000 else O.codon_region(len(contigs[s]), 1, 1, 17, 20, seq=s)
            for s in range(len(contigs))]
    seq, off = _batch(contigs)
    regs = O.regions_of(rows)
    st = {}
    got = _dev(regs, seq, off, stats=st)
    want = O.orfs(regs, seq, off)
    _same(got, want)
    assert st["residues"] == n_long + 10_000 - len(range(0, 10_001, 7)) and st["orfs"] == 10_001 and st["ms"] > 0
    _same(_dev(regs, seq, off, ok=False), O.orfs(regs, seq, off, only_kept=False))


@pytest.mark.parametrize("seed", range(24))
def test_random_batches_equal_the_model(seed):
    rng = np.random.default_rng(1000 + seed)
    weights = [None, np.array([30, 10, 10, 30, 2, 2, 2, 2, 2, 5, 5], float) / 100,
               np.array([4, 44, 44, 4, 0, 1, 1, 1, 0, 1, 0], float) / 100][seed % 3]         # the last: GC-rich, stops far apart
    regs, seq, off = O.random_batch(rng, int(rng.choice([1, 7, 60])), max_len=int(rng.choice([30, 500, 5 * 3 * T])),
                                    max_regions=int(rng.choice([2, 12])), weights=weights)
    sc = [7, 1, 0, 5][seed % 4]
    for ok in (True, False):
        want = O.orfs(regs, seq, off, sc, ok)
        for dst in ("host", "device"):
            st = {}
            _same(_dev(regs, seq, off, sc, ok, dst, st), want)
            fl = want[0]["flags"]
            assert st["orfs"] == len(regs) and st["residues"] == len(want[2]) and st["interrupted"] == ((fl & O.INTERRUPTED) != 0).sum()
            assert st["complete"] == (((fl & O.HAS_STOP) != 0) & ((fl & O.INTERRUPTED) == 0) & (want[0]["start_codon"] != 0)).sum()


def test_empty_inputs():
    none = np.zeros(0, N.REGION_DTYPE)
    for seq, off in ((b"", np.zeros(1, np.int64)), (b"ACGTACGT", np.array([0, 3, 3, 8], np.int64))):
        o, ps, res = _dev(none, seq, off)
        assert len(o) == 0 and ps.tolist() == [0] and len(res) == 0


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


def test_scan_result_orfs_equal_the_model_on_the_device_regions(strategy):
    from kmergutsjava_amd import hotpath
    img, dna, off, genes = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    d_seq = torch.from_numpy(sb.copy()).cuda()
    torch.cuda.synchronize()
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        live0 = tab.live_device_bytes()
        for ptr in (None, d_seq.data_ptr()):
            with tab.scan(None if ptr else sb, off, hotpath.Params(), device_ptr=ptr) as r:
                live1 = tab.live_device_bytes()
                want_regs = r.regions(off, 300, 10, 90)
                regs, start, orfs, ps, res = r.orfs(None if ptr else sb, off, 300, 10, 90, start_codons=3, only_kept=False, device_ptr=ptr)
                assert regs.tobytes() == want_regs[0].tobytes() and start.tobytes() == want_regs[1].tobytes() and len(regs) > 20
                _same((orfs, ps, res), O.orfs(regs, dna, off, 3, False))
                assert r.orf_stats["ms"] > 0 and r.orf_stats["orfs"] == len(regs) and tab.live_device_bytes() == live1
                regs, start, orfs, ps, res = r.orfs(None if ptr else sb, off, device_ptr=ptr)
                _same((orfs, ps, res), O.orfs(regs, dna, off))
                checked, unshifted = HO.recovered_genes(regs, start, *O.orfs(regs, dna, off, only_kept=False), genes)
                assert checked >= 1
        assert tab.live_device_bytes() == live0


def test_a_contigs_records_are_the_same_alone_as_in_a_batch():
    rng = np.random.default_rng(77)
    regs, seq, off = O.random_batch(rng, 40, max_len=4 * 3 * T, max_regions=5)
    whole = _dev(regs, seq, off, ok=False)
    for s in range(0, 40, 3):
        mine = regs["seq"] == s
        if not mine.any():
            continue
        sub = regs[mine].copy()
        sub["seq"] = 0
        o, ps, res = _dev(sub, seq[off[s]:off[s + 1]], np.array([0, off[s + 1] - off[s]], np.int64), ok=False)
        o["seq"] = s
        assert o.tobytes() == whole[0][mine].tobytes()
        idx = np.flatnonzero(mine)
        assert [bytes(res[ps[k]:ps[k + 1]]) for k in range(len(idx))] == [bytes(whole[2][whole[1][i]:whole[1][i + 1]]) for i in idx]


def test_errors_name_the_first_offending_region():
    from kmergutsjava_amd import hotpath
    seq, off = _batch([HO.A, b"ACGTACGTAC"])
    good = O.regions_of([O.region(0, 0, 12, 17, 0), O.region(1, 1, 0, 8, 1), O.region(0, 0, 12, 17, 0), O.region(0, 1, 3, 20, 2)])
    assert len(_dev(good, seq, off)[0]) == 4

    def err(regs=good, s=seq, o=off, **kw):
        with pytest.raises(N.KmerGutsNativeError) as ei:
            hotpath.orf_regions(regs, s, o, **kw)
        return ei.value

    for field, value, which, word in (("seq", 2, 1, "seq"), ("seq", -1, 3, "seq"), ("strand", 2, 2, "strand"), ("best_frame", 3, 1, "best_frame"),
                                      ("best_frame", -1, 0, "best_frame"), ("left", 18, 2, "outside"), ("right", 30, 0, "outside"),
                                      ("right", 10, 1, "outside"), ("left", -1, 3, "outside")):
        bad = good.copy()
        bad[field][which] = value
        bad[field][3 if which < 3 else 2] = value if which < 3 else bad[field][2]      # a later offender does not change the name
        e = err(regs=bad)
        assert e.code == N.KG_ERR_ARG and "region %d:" % which in str(e) and word in str(e), str(e)
    bad = good.copy()
    bad["left"][1], bad["right"][1] = 0, 1          # two nucleotides: no whole codon
    e = err(regs=bad)
    assert e.code == N.KG_ERR_ARG and "region 1:" in str(e) and "codon" in str(e)
    bad = good.copy()
    bad["left"][2], bad["right"][2], bad["best_frame"][2] = 13, 16, 0       # x 13..16 holds no codon of frame 0
    e = err(regs=bad)
    assert e.code == N.KG_ERR_ARG and "region 2:" in str(e) and "codon" in str(e)
    e = err(o=np.array([0, 30, 20], np.int64))
    assert e.code == N.KG_ERR_ARG and "contig 1" in str(e)
    assert err(regs=good[:1], s=b"", o=np.zeros(1, np.int64)).code == N.KG_ERR_ARG
    for kw in ({"start_codons": 8}, {"start_codons": -1}):
        assert err(**kw).code == N.KG_ERR_ARG
    # through the C ABI: only_kept outside 0..1 (the wrapper makes it a bool), and an n_seqs that is not the region set's
    import ctypes as C
    lib, h, oh = N.load(), C.c_void_p(), C.c_void_p()
    sb = np.frombuffer(seq, dtype=np.uint8)
    for only_kept in (2, -1):
        rc = lib.kg_orfs_regions(0, C.byref(N.KgOrfParams(7, only_kept, 0)), good.ctypes.data, len(good), sb.ctypes.data,
                                 off.ctypes.data, len(off) - 1, C.byref(oh))
        assert rc == N.KG_ERR_ARG and not oh.value and b"only_kept" in lib.kg_last_error()
    none = np.zeros(0, N.CALL_DTYPE)
    N.check(lib.kg_regions_calls(0, C.byref(N.KgRegionParams(600, 0, 0)), None, 0, off.ctypes.data, len(off) - 1, C.byref(h)))
    try:
        for n_seqs in (len(off) - 2, len(off)):
            o2 = np.ascontiguousarray(np.arange(n_seqs + 1, dtype=np.int64) * 10)
            rc = lib.kg_regionset_orfs(h, C.byref(N.KgOrfParams(7, 1, 0)), sb.ctypes.data, 0, o2.ctypes.data, n_seqs, C.byref(oh))
            assert rc == N.KG_ERR_ARG and not oh.value and b"n_seqs" in lib.kg_last_error()
        N.check(lib.kg_regionset_orfs(h, C.byref(N.KgOrfParams(7, 1, 0)), sb.ctypes.data, 0, off.ctypes.data, len(off) - 1, C.byref(oh)))
        assert lib.kg_orfset_count(oh) == 0 and len(none) == 0
        lib.kg_orfset_free(oh)
    finally:
        lib.kg_regionset_free(h)


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(4)
    regs, seq, off = O.random_batch(rng, 50, max_len=3000, max_regions=8)
    want = O.orfs(regs, seq, off)
    img, dna, doff, _ = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(sb, doff, hotpath.Params()) as r:
        want_r = r.orfs(sb, doff)
        assert len(want_r[2]) > 0
        _same(_dev(regs, seq, off), want)           # once first: what the runtime sets up on first use is not counted
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        live0 = tab.live_device_bytes()
        for which in ("regions", "result"):
            failed = 0
            for n in range(1, 200):
                monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
                try:
                    got = _dev(regs, seq, off) if which == "regions" else r.orfs(sb, doff)
                    break
                except N.KmerGutsNativeError as e:
                    assert e.code == N.KG_ERR_NOMEM, e
                    failed += 1
                    assert tab.live_device_bytes() == live0
                    if which == "regions":
                        assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
            monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
            assert failed >= 12
            if which == "regions":
                _same(got, want)
            else:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want_r))
            assert tab.live_device_bytes() == live0
        # an ORF set that is still open holds its three blocks, and gives them back when it is freed
        import ctypes as C
        lib, h, oh = N.load(), C.c_void_p(), C.c_void_p()
        o = np.ascontiguousarray(doff, dtype=np.int64)
        N.check(lib.kg_result_regions(r._h, C.byref(N.KgRegionParams(600, 0, 0)), o.ctypes.data, C.byref(h)))
        live_set = tab.live_device_bytes()
        N.check(lib.kg_regionset_orfs(h, C.byref(N.KgOrfParams(7, 1, 0)), sb.ctypes.data, 0, o.ctypes.data, len(o) - 1, C.byref(oh)))
        assert tab.live_device_bytes() > live_set and lib.kg_orfset_count(oh) == len(want_r[2])
        lib.kg_orfset_free(oh)
        assert tab.live_device_bytes() == live_set
        lib.kg_regionset_free(h)
        assert tab.live_device_bytes() == live0


# ---- the prefix sum under prot_start: the 2^32 limit at the wrap, and the chunk and carry borders ------------------------------------

_LIMIT = {}


def _limit_rows():
    """The batch of tests/scan_model.py with 2^21 sense codons, and the three regions of its lists.  Without start codons an
    ORF runs from behind the stop in front of its region (orf_region_kernel: u + 1, here the contig's first codon) to the stop
    behind it, so every region inside the long frame is the whole frame, 2^21 residues, and the region of the short contig is
    its SHORT_CODONS codons; a region that is not kept gives no residues under only_kept."""
    if not _LIMIT:
        seq, off = SM.limit_batch(SM.LONG)
        L0, L1 = int(off[1]), int(off[2] - off[1])
        _LIMIT["w"] = (seq, off, O.codon_region(L1, 0, 0, 1000, 1003, seq=1), O.codon_region(L0, 0, 0, 3, 3, seq=0),
                       O.codon_region(L1, 0, 0, 7, 9, seq=1, kept=0))
    return _LIMIT["w"]


def test_residue_totals_that_wrap_a_chunk_of_the_prefix_sum_are_refused():
    """The lists of scan_model.families: 2048 ORFs of 2^21 residues alone, behind 2048 short ORFs, in reversed order, and --
    the control, refused whatever the chunk sums' width -- half in each of two chunks.  tests/test_scan_model_host.py shows that
    32-bit chunk sums gave the first three a total below 2^32.  Every call is refused with the stage's own words, leaves no
    device memory behind, and the next call is an ordinary one."""
    from kmergutsjava_amd import hotpath
    seq, off, long_row, short_row, none_row = _limit_rows()
    small = O.regions_of([short_row, long_row, none_row, short_row])
    img = _workload()[0]
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        want = O.orfs(small, seq, off, 0)
        _same(_dev(small, seq, off, sc=0), want)        # once first: what the runtime sets up on first use is not counted
        assert want[0]["n_res"].tolist() == [SM.SHORT_CODONS, SM.LONG, SM.LONG, SM.SHORT_CODONS] and np.diff(want[1])[2] == 0
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        for name, (lens, _) in SM.families(SM.SHORT_CODONS).items():
            regs = SM.records_of(lens, long_row, short_row, none_row, N.REGION_DTYPE)
            assert len(regs) == len(lens) and SM.scan_exact(lens)[1] >= SM.LIMIT
            with pytest.raises(N.KmerGutsNativeError) as ei:
                hotpath.orf_regions(regs, seq, off, 0)
            assert ei.value.code == N.KG_ERR_LIMIT, name
            assert SM.message_of(ei.value).startswith("2^32 or more residues"), (name, str(ei.value))
            assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0, name
        _same(_dev(small, seq, off, sc=0), want)


_EXACT = {}


def _exact_case():
    """A contig of three ORFs between stops -- 1, 257 and 300 codons -- behind a short one, one region inside each, and the
    model's record and protein of each."""
    if not _EXACT:
        rng = np.random.default_rng(2048)
        sense = lambda n: SM._SENSE[rng.integers(0, len(SM._SENSE), size=n)].tobytes()       # noqa: E731
        contig = b"TAA" + sense(1) + b"TAA" + sense(257) + b"TAA" + sense(300) + b"TAA" + b"G"
        seq, off = _batch([b"ACGTA", contig])
        L = len(contig)
        kinds = O.regions_of([O.codon_region(L, 0, 0, 1, 1, seq=1), O.codon_region(L, 0, 0, 100, 120, seq=1), O.codon_region(L, 0, 0, 300, 301, seq=1)])
        recs, ps, res = O.orfs(kinds, seq, off, 0)
        assert recs["n_res"].tolist() == [1, 257, 300]
        _EXACT["w"] = (seq, off, kinds, recs, ps, res)
    return _EXACT["w"]


@pytest.mark.parametrize("n", [SM.CHUNK - 1, SM.CHUNK, SM.CHUNK + 1, 2 * SM.CHUNK, SM.TOP * SM.CHUNK - 1, SM.TOP * SM.CHUNK,
                               SM.TOP * SM.CHUNK + 1])
def test_prot_start_is_the_cumulative_sum_at_the_chunk_and_carry_borders(n):
    """Region counts that end one short of a chunk of the prefix sum, on it and one behind it, and the same about the 256
    chunks of one trip of scan_top_kernel's carry loop.  ORFs of one codon, with those of a few hundred at the last slot of
    every chunk, at the first of the next and at one slot in 300: prot_start is np.cumsum of the lengths, the residues are the
    model's proteins in that order, the records the model's."""
    seq, off, kinds, recs, ps, res = _exact_case()
    rng = np.random.default_rng(n)
    i = np.arange(n)
    kind = np.where(rng.integers(0, 300, size=n) == 0, 1, 0)
    kind[i % SM.CHUNK == SM.CHUNK - 1] = 1
    kind[i % SM.CHUNK == 0] = 2
    lens = recs["n_res"].astype(np.int64)[kind]
    want_start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=want_start[1:])
    total = int(want_start[-1])
    assert n + 256 * (n // SM.CHUNK) < total < 8 << 20
    at = np.arange(total, dtype=np.int64) - np.repeat(want_start[:-1], lens) + np.repeat(ps[:-1][kind], lens)
    st = {}
    got = _dev(kinds[kind], seq, off, sc=0, stats=st)
    _same(got, (recs[kind], want_start, res[at]))
    assert st["residues"] == total and st["orfs"] == n


def test_call_regions_orfs_faa_and_annotate(oracle, tmp_path):
    """call_regions --orfs --faa writes the model's text, without the flags its output is what it was, and the .faa goes through
    annotate: every written protein without * and X is assigned its region's function or gets status none."""
    from kmergutsjava_amd import call_regions as CR
    from kmergutsjava_amd import synth
    img, dna, off, _ = _workload()
    n = len(off) - 1
    ids = [b"contig_%d" % k for k in range(n)]
    q = tmp_path / "c.fna"
    q.write_bytes(b"".join(b">%s planted genes\n%s\n" % (ids[k], dna[off[k]:off[k + 1]]) for k in range(n)))
    d = tmp_path / "d"
    synth.write_data_dir(str(d), img, 50)
    fnames = [b"synthetic function %d" % i for i in range(50)]
    calls = oracle.run(img, np.frombuffer(dna, dtype=np.uint8), off, lookup_mode=1, min_hits=4)["calls"]
    regs, start = R.regions(calls, off, 300, 12, 100)
    kw = dict(min_hits=4, merge_gap=300, min_score=12, min_len=100)
    plain = CR.call_regions(str(d), str(q), str(tmp_path / "plain.tsv"), **kw)
    assert plain == CR.summary_of(regs, start) and 0 < regs["kept"].sum() < len(regs)
    orfs, ps, res = O.orfs(regs, dna, off)
    # the command line, default start codons
    p = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.call_regions", "-D", str(d), "-q", str(q), "-m", "4", "--merge-gap", "300",
                        "--min-score", "12", "--min-len", "100", "-o", str(tmp_path / "o.tsv"), "--orfs", str(tmp_path / "orfs.tsv"),
                        "--faa", str(tmp_path / "p.faa")], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip() == CR.summary_of(regs, start) + CR.orf_summary(orfs)
    assert (tmp_path / "o.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes() == CR.format_regions(ids, regs, fnames)
    assert (tmp_path / "orfs.tsv").read_bytes() == CR.format_orfs(ids, regs, orfs, fnames)
    faa = (tmp_path / "p.faa").read_bytes()
    assert faa == CR.format_faa(ids, regs, orfs, ps, res, fnames) and faa.count(b">") > 10
    # --all --start-codons ATG, and --faa alone
    o1 = O.orfs(regs, dna, off, 1, False)
    line = CR.call_regions(str(d), str(q), str(tmp_path / "o1.tsv"), write_all=True, orfs_out=str(tmp_path / "orfs1.tsv"),
                           faa_out=str(tmp_path / "p1.faa"), start_codons=CR.parse_start_codons("ATG"), **kw)
    assert line == CR.summary_of(regs, start) + CR.orf_summary(o1[0])
    assert (tmp_path / "o1.tsv").read_bytes() == CR.format_regions(ids, regs, fnames, True)
    assert (tmp_path / "orfs1.tsv").read_bytes() == CR.format_orfs(ids, regs, o1[0], fnames, True)
    assert (tmp_path / "p1.faa").read_bytes() == CR.format_faa(ids, regs, *o1, fnames, True)
    CR.call_regions(str(d), str(q), str(tmp_path / "o2.tsv"), faa_out=str(tmp_path / "p2.faa"), **kw)
    assert (tmp_path / "p2.faa").read_bytes() == faa
    # the default run's proteins through annotate
    from kmergutsjava_amd import annotate as AN
    AN.annotate(str(d), str(tmp_path / "p.faa"), str(tmp_path / "a.tsv"), min_hits=4, write_all=True)
    want_fn, clean = {}, set()
    for block in (tmp_path / "p.faa").read_bytes().split(b">")[1:]:
        head, _, body = block.partition(b"\n")
        pid, _, fname = head.partition(b" ")
        assert pid not in want_fn, "two proteins under one id"
        want_fn[pid] = fname
        if b"*" not in body and b"X" not in body:
            clean.add(pid)
    split = {"assigned": 0, "none": 0}
    seen = set()
    for line in (tmp_path / "a.tsv").read_bytes().splitlines():
        pid, status, fname = line.split(b"\t")[:3]
        seen.add(pid)
        if pid in clean:
            assert status == b"none" or (status == b"assigned" and fname == want_fn[pid]), line
            split[status.decode()] += 1
    assert seen == set(want_fn) and split["assigned"] > 0
    print("annotate over the .faa: %d proteins, %d clean: %s" % (len(want_fn), len(clean), split))
