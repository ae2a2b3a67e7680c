"""Frameshift repair on the GPU (kg_regionset_repair / kg_result_repair): the device's records, prot_start, residues, junctions
and statistics must equal the numpy form of tests/repair_model.py byte for byte -- on the hand-made chains of
tests/repair_cases.py, random batches, CALL and region counts at wave and workgroup sizes, one region of 10^4 CALLs among 2000
small ones, stops at tile distances, part borders at a residue lane's border, behind a scan under both strategies, and with the
later stages on the new set.  Foreign CALL lists are named; failed allocations leave nothing behind."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import coding_model as K  # noqa: E402
import orfs_model as O  # noqa: E402
import regions_model as R  # noqa: E402
import repair_cases as RC  # noqa: E402
import repair_model as M  # noqa: E402
import select_model as S  # noqa: E402
import test_orfs_host as HO  # noqa: E402
from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
T = N.ORF_TILE_CODONS
NAMES = ("orfs", "prot_start", "residues", "junctions", "junction_start")


def _check(calls, seq, off, merge_gap=600, min_score=0, only_kept=True, device_inputs=False, **kw):
    """The device against the models: regions and given ORFs too.  -> (the model's result, the given ORF set)"""
    from kmergutsjava_amd import hotpath
    sc = kw.get("start_codons", 7)
    regs, rstart = R.regions(calls, off, merge_gap=merge_gap, min_score=min_score)
    o, ps, res = O.orfs(regs, seq, off, start_codons=sc, only_kept=only_kept)
    want = M.repair(regs, o, ps, res, calls, seq, off, **kw)
    st = {}
    got = hotpath.repair_orfs(calls, seq, off, merge_gap=merge_gap, min_score=min_score, only_kept=only_kept, device_inputs=device_inputs,
                              stats=st, **kw)
    assert got[0].tobytes() == regs.tobytes() and got[1].tobytes() == rstart.tobytes()
    for name, g, w in zip(NAMES, got[2:], want[:5]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, g, w)
    assert {k: st["repair"][k] for k in M.STAT_KEYS} == want[5], (st["repair"], want[5])
    assert st["orfs"]["residues"] == want[2].size and st["orfs"]["orfs"] == len(regs)
    f = want[0]["flags"]
    assert st["orfs"]["interrupted"] == int(((f & O.INTERRUPTED) != 0).sum()) and st["orfs"]["partial5"] == int(((f & O.PARTIAL5) != 0).sum())
    assert st["orfs"]["complete"] == int((((f & O.HAS_STOP) != 0) & (want[0]["start_codon"] != 0) & ((f & O.INTERRUPTED) == 0)).sum())
    return want, (regs, o, ps, res)


def _batch(items):
    """[(text, strand, calls on the strand)] -> one CALL list, bytes and offsets: a contig per item."""
    rows, parts, off = [], [], [0]
    for s, (text, strand, calls) in enumerate(items):
        c, seq, _ = RC.lay(text, strand, calls)
        c = c.copy()
        c["container"] += 6 * s
        rows.append(c)
        parts.append(seq)
        off.append(off[-1] + len(seq))
    return np.concatenate(rows), np.concatenate(parts), np.array(off, dtype=np.int64)


@pytest.mark.parametrize("strand", [0, 1])
def test_known_answers_on_the_device(strand):
    """Every hand-made chain (2 and 3 segments, segments of one CALL, every failure kind, skipped, single, min_count), alone and
    all in one batch; tests/test_repair_host.py checks the model's answers for them against the ones worked out by hand."""
    cases = RC.cases()
    for k, case in enumerate(cases):
        calls, seq, off = RC.lay(case["text"], strand, case["calls"])
        want, _ = _check(calls, seq, off, start_codons=1, device_inputs=bool(k & 1), **case["params"])
        assert want[5][case["state"]] == 1
    plain = [c for c in cases if not c["params"]]
    want, _ = _check(*_batch([(c["text"], (strand + i) & 1, c["calls"]) for i, c in enumerate(plain)]), start_codons=1)
    assert want[5]["repaired"] == sum(c["state"] == "repaired" for c in plain) and want[5]["failed"] == sum(c["state"] == "failed" for c in plain)


@pytest.mark.parametrize("seed", range(3))
def test_random_batches(seed):
    rng = np.random.default_rng(40 + seed)
    tot = dict.fromkeys(M.STAT_KEYS, 0)
    for it in range(40):
        calls, seq, off = M.random_case(rng, n_seqs=int(rng.integers(1, 8)), max_len=int(rng.choice([300, 1500])))
        kw = dict(start_codons=int(rng.choice([7, 7, 1, 0])), min_count=int(rng.choice([0, 0, 2, 4])), max_junctions=int(rng.choice([1, 2, 4, 8])))
        want, _ = _check(calls, seq, off, merge_gap=int(rng.choice([30, 600])), min_score=int(rng.choice([0, 6])),
                         only_kept=bool(rng.integers(0, 2)), device_inputs=bool(it & 1), **kw)
        for k in tot:
            tot[k] += want[5][k]
    assert all(tot[k] > 0 for k in M.STAT_KEYS), tot


def _long_text(n_codons):
    return b"ATG" + b"GCA" * (n_codons - 1)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_calls_of_one_region_at_the_wave_size(n):
    """n overlapping CALLs, the first half in frame 0 and the rest in frame 2: two segments whose C_k is the maximum over a wave's
    worth of CALLs (the longest CALL of a segment is not its last)."""
    h = n // 2
    calls = [(0, 1 + k, 3 + k + (40 if k == 1 else 0), 3) for k in range(h)] + [(2, 60 + k, 62 + k + (30 if k == 0 else 0), 3) for k in range(n - h)]
    for strand in (0, 1):
        want, _ = _check(*RC.lay(_long_text(200), strand, calls), start_codons=1)
        assert want[5]["repaired"] == 1 and want[3]["gap"][0] == (2 + 3 * 60) - (3 * 44 + 2) - 1


@pytest.mark.parametrize("n", [255, 256, 257])
def test_regions_at_the_workgroup_size(n):
    cases = [c for c in RC.cases() if not c["params"]]
    want, _ = _check(*_batch([(cases[i % len(cases)]["text"], i & 1, cases[i % len(cases)]["calls"]) for i in range(n)]), start_codons=1)
    assert len(want[0]) == n and want[5]["candidates"] == n and want[5]["repaired"] > n // 2


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_region_of_10000_alternating_calls_among_2000_small_ones(where):
    """The large region is skipped, not walked: its 10^4 segments are more than max_junctions + 1."""
    big = (_long_text(10010), 0, [(k % 2, 2 + k, 2 + k, 2) for k in range(10000)])
    case = RC.cases()[0]
    small = [(case["text"], i & 1, case["calls"]) for i in range(2000)]
    at = {"first": 0, "middle": 1000, "last": 2000}[where]
    want, _ = _check(*_batch(small[:at] + [big] + small[at:]), start_codons=1)
    assert want[5] == {"candidates": 2001, "repaired": 2000, "failed": 0, "single": 0, "skipped": 1, "junctions": 2000,
                       "residues": 2000 * len(case["protein"])}
    assert not want[0][at]["flags"] & M.REPAIRED and want[4][at] == want[4][at + 1] == at


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("d", [1, T - 1, T, T + 1, 2 * T + 1])
def test_stops_at_tile_distances_from_the_evidence(strand, d):
    """A frame-0 stop d codons behind lp with the next evidence far away clamps J to hi; a frame-2 stop d codons in front of gq
    with the evidence far away clamps J to lo.  lp and gq lie two codons into a tile, so d walks through the in-tile search, the
    tile's last codon, the next tile's first one and the scanned key two tiles on."""
    n = 8 * T
    lp, far = T + 2, T + 2 + 2 * (2 * T + 1) + 40
    text = bytearray(_long_text(n))
    text[3 * (lp + d):3 * (lp + d) + 3] = b"TAA"                       # frame 0, codon lp + d
    calls = [(0, lp - 5, lp, 3), (2, far, far + 5, 3)]
    want, _ = _check(*RC.lay(bytes(text), strand, calls), merge_gap=3000, start_codons=1)
    J = 3 * (lp + d)
    assert want[5]["repaired"] == 1 and want[3]["pos"][0] == (J if not strand else 3 * n - 1 - J)
    gq = 5 * T + 2
    text = bytearray(_long_text(n))
    text[2 + 3 * (gq - d):2 + 3 * (gq - d) + 3] = b"TAA"               # frame 2, codon gq - d
    calls = [(0, gq - 2 * (2 * T + 1) - 40, gq - 2 * (2 * T + 1) - 35, 3), (2, gq, gq + 5, 3)]
    want, _ = _check(*RC.lay(bytes(text), strand, calls), merge_gap=3000, start_codons=1)
    J = 2 + 3 * (gq - d + 1)
    assert want[5]["repaired"] == 1 and want[3]["pos"][0] == (J if not strand else 3 * n - 1 - J)


@pytest.mark.parametrize("c", [7, 9, 11])
def test_a_part_border_on_each_side_of_a_residue_lane_border(c):
    """Frame 0 codons 1..6 and frame 2 from codon c: part 1 has 7, 8 and 9 residues, so the protein's second part begins one
    residue in front of, at and one behind the border between two lanes of the residues kernel (8 residues each)."""
    text = RC.text_with([(0, b"ATG"), (77, b"TAA")])
    for strand in (0, 1):
        want, _ = _check(*_batch([(text, strand, [(0, 1, 6, 4), (2, c, 19, 4)])] * 3), start_codons=1)
        assert want[3]["res"].tolist() == [{7: 7, 9: 8, 11: 9}[c]] * 3 and want[5]["repaired"] == 3


def test_not_kept_single_frame_and_only_kept_stay_byte_for_byte():
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(9)
    calls, seq, off = M.random_case(rng, n_seqs=12)
    for only_kept in (True, False):
        want, (regs, o, ps, res) = _check(calls, seq, off, min_score=8, only_kept=only_kept)
        rep = (want[0]["flags"] & M.REPAIRED) != 0
        assert rep.any() and (regs["kept"] == 0).any() and want[0][~rep].tobytes() == o[~rep].tobytes()
        assert (np.diff(want[1])[regs["kept"] == 0] == 0).all() == only_kept
        # no candidate at all: the new set is the given one
        got = hotpath.repair_orfs(calls, seq, off, min_score=10 ** 6, only_kept=only_kept)
        base = hotpath.orf_regions(got[0], seq, off, only_kept=only_kept)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[2:5], base)) and got[5].size == 0 and not got[6].any()


def test_empty_inputs():
    from kmergutsjava_amd import hotpath
    none = np.zeros(0, dtype=N.CALL_DTYPE)
    for seq, off in ((b"", [0]), (b"", [0, 0, 0]), (b"ACGTACGTAC", [0, 4, 10])):
        st = {}
        got = hotpath.repair_orfs(none, seq, np.array(off, dtype=np.int64), stats=st)
        assert [len(x) for x in got] == [0, len(off), 0, 1, 0, 0, 1] and st["repair"]["candidates"] == 0
    # CALLs, but no multi-frame region
    case = RC.cases()[0]
    calls, seq, off = RC.lay(case["text"], 0, case["calls"][:1])
    want, _ = _check(calls, seq, off)
    assert want[5]["candidates"] == 0 and want[3].size == 0


def test_a_foreign_call_list_is_named():
    from kmergutsjava_amd import hotpath
    case = RC.cases()[10]
    assert case["name"] == "three"
    calls, seq, off = _batch([(case["text"], 0, case["calls"]), (case["text"], 1, case["calls"])])

    def fails(word, other, **kw):
        with pytest.raises(N.KmerGutsNativeError) as ei:
            hotpath.repair_orfs(calls, seq, off, repair_calls=other, **kw)
        assert ei.value.code == N.KG_ERR_ARG and word in str(ei.value), str(ei.value)

    moved = calls.copy()
    moved["end"][4] += 3                         # CALL 4 (contig 1, frame 1) now ends behind its region
    fails("CALL 4: lies in no region of its group", moved, merge_gap=5)
    other_fn = calls.copy()
    other_fn["fI"][2] = 3
    fails("CALL 2: lies in no region of its group", other_fn)
    count = calls.copy()
    count["count"][5] += 1
    fails("region 1: the CALLs inside it do not add up", count)
    fails("region 1: the CALLs inside it do not add up", calls[:-1])
    fails("region 1: the CALLs inside it do not add up", np.concatenate([calls, calls[5:]]))
    fails("region 0: seq, strand or first_call", calls[:0])
    fails("CALL 1: container below", calls[::-1].copy())
    bad = calls.copy()
    bad["container"][5] = 12
    fails("CALL 5: container >= 6 * n_seqs", bad)
    for kw, word in ((dict(min_count=-1), "min_count"), (dict(max_junctions=0), "max_junctions"), (dict(max_junctions=9), "max_junctions"),
                     (dict(start_codons=8), "start_codons")):
        fails(word, calls, **kw)
    lib = N.load()
    assert lib.kg_orfset_junctions_count(None) == 0
    # a set that is not from the repair has no junction list
    oh = C.c_void_p()
    sb = np.frombuffer(seq, dtype=np.uint8)
    N.check(lib.kg_orfs_free(0, C.byref(N.KgFreeParams(10, 7, 0)), sb.ctypes.data, 0, off.ctypes.data, len(off) - 1, C.byref(oh)))
    try:
        buf = np.zeros(4, np.int64)
        assert lib.kg_orfset_junctions_start(oh, buf.ctypes.data) == N.KG_ERR_ARG and b"not from kg_regionset_repair" in lib.kg_last_error()
        assert lib.kg_orfset_junctions_stats(oh, C.byref(N.KgRepairStats())) == N.KG_ERR_ARG
        assert lib.kg_orfset_junctions_copy(oh, 0, 0, None) == N.KG_ERR_ARG
        # ... and is not index-aligned with any region set
        rh, new = C.c_void_p(), C.c_void_p()
        N.check(lib.kg_regions_calls(0, C.byref(N.KgRegionParams(600, 0, 0)), calls.ctypes.data, calls.size, off.ctypes.data, len(off) - 1, C.byref(rh)))
        try:
            rc = lib.kg_regionset_repair(rh, oh, calls.ctypes.data, 0, calls.size, C.byref(N.KgRepairParams(7, 0, 4, 0)), sb.ctypes.data, 0,
                                         off.ctypes.data, len(off) - 1, C.byref(new))
            assert rc == N.KG_ERR_ARG and not new.value and b"ORF set" in lib.kg_last_error()
        finally:
            lib.kg_regionset_free(rh)
    finally:
        lib.kg_orfset_free(oh)


# ---- behind a scan ----------------------------------------------------------------------------------------------------------------------

_WORK = {}


def _workload():
    if not _WORK:
        _WORK["w"] = HO.planted_orf_contigs()
    return _WORK["w"]


@pytest.fixture(params=["direct", "partitioned"])
def strategy(request, monkeypatch):
    monkeypatch.setenv("KG_PARTITION", "0" if request.param == "direct" else "1")
    monkeypatch.setenv("KG_DIRECT_FILTER", "2")
    return request.param


def test_behind_a_scan_and_in_front_of_the_later_stages(strategy):
    """ScanResult.orfs / select with repair=: kg_result_repair on the result's device CALLs, from host and device bytes; then
    kg_orfset_add_free, kg_orfset_coding, kg_orfset_starts and kg_orfset_select on the new set.  Repaired records are neither
    trained on nor moved, and the selection sees their extents."""
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
                plain = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr)
                want = M.repair(plain[0], plain[2], plain[3], plain[4], r.calls(), dna, off)
                got = r.orfs(None if ptr else sb, off, 300, 12, 100, device_ptr=ptr, repair=True)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:2], plain[:2]))
                for name, g, w in zip(NAMES, got[2:] + (r.junctions, r.junction_start), want[:5]):
                    assert g.tobytes() == w.tobytes(), name
                assert {k: r.repair_stats[k] for k in M.STAT_KEYS} == want[5] and want[5]["repaired"] >= 20 and r.repair_stats["ms"] > 0
                assert tab.live_device_bytes() == live1
                kw = dict(free_min_res=100, coding=True, min_train_pairs=1000, starts=True, min_train_starts=50)
                full = r.select(off, None if ptr else sb, 300, 12, 100, orfs=True, device_ptr=ptr, repair=True, **kw)
                nr = len(plain[0])
                rep = np.flatnonzero((want[0]["flags"] & M.REPAIRED) != 0)
                assert full[2][:nr][rep].tobytes() == want[0][rep].tobytes() and not r.start_shifts[rep].any()
                assert r.coding_stats["trained"] == 1 and r.start_stats["trained"] == 1
                assert r.coding_stats["training_records"] == sum(K.is_training(o) for o in full[2]) and not any(K.is_training(o) for o in want[0][rep])
                assert full[5].tobytes() == S.select_fast(S.of_records(full[2])).tobytes() and (full[5]["state"][rep] == 1).sum() > 0
                assert tab.live_device_bytes() == live1
                with pytest.raises(ValueError):
                    r.select(off, None if ptr else sb, 300, 12, 100, repair=True)
        assert tab.live_device_bytes() == live0


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    """Every allocation of the call fails once, beside an open table on sets made from a scan of it: after every failure the
    table's live bytes are what they were, and 0 when the sets and the result are freed."""
    from kmergutsjava_amd import hotpath
    lib = N.load()
    img, dna, off, _ = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        with tab.scan(sb, off, hotpath.Params(min_hits=4)) as r:
            rh, oh, new = C.c_void_p(), C.c_void_p(), C.c_void_p()
            batch = (sb.ctypes.data, 0, off.ctypes.data, len(off) - 1)
            N.check(lib.kg_result_regions(r._h, C.byref(N.KgRegionParams(300, 12, 100)), off.ctypes.data, C.byref(rh)))
            try:
                N.check(lib.kg_regionset_orfs(rh, C.byref(N.KgOrfParams(7, 1, 0)), *batch, C.byref(oh)))
                live1 = tab.live_device_bytes()
                failed, p = 0, N.KgRepairParams(7, 0, 4, 0)
                for n in range(1, 200):
                    monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
                    rc = lib.kg_result_repair(r._h, rh, oh, C.byref(p), *batch, C.byref(new))
                    if rc == 0:
                        break
                    assert rc == N.KG_ERR_NOMEM and not new.value and b"KG_TEST_FAIL_ALLOC" in lib.kg_last_error()
                    failed += 1
                    assert tab.live_device_bytes() == live1
                monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
                assert failed >= 40 and new.value        # the bytes, the planes, the checks' arrays, two sorts, 17 of the chain, two outputs
                _, _, st = hotpath._junctions(new)
                assert st["repaired"] >= 20
                lib.kg_orfset_free(new)
                new.value = None
                assert tab.live_device_bytes() == live1
            finally:
                for h, free in ((new, lib.kg_orfset_free), (oh, lib.kg_orfset_free), (rh, lib.kg_regionset_free)):
                    if h.value:
                        free(h)
        assert tab.live_device_bytes() == 0


# ---- the front end ----------------------------------------------------------------------------------------------------------------------

def test_call_regions_repair_end_to_end(tmp_path):
    """call_regions --repair --shifts --orfs --faa on the planted contigs: the files against the model's records through the
    writers (which tests/test_repair_frontend.py checks line by line), and without --repair the summary and digests recorded from
    the commit before the option (tests/golden/call_regions_planted_before_repair.json).  Two runs of the command line: each
    costs an interpreter's start."""
    import subprocess
    import test_repair_frontend as FE
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
                                   str(tmp_path / (tag + ".faa"))] + list(extra), capture_output=True, text=True, cwd=os.path.dirname(HERE))
        assert p.returncode == 0, p.stderr
        return p.stdout.strip(), [(tmp_path / (tag + ext)).read_bytes() for ext in (".tsv", ".orfs", ".faa")]

    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(np.frombuffer(dna, np.uint8), off, hotpath.Params(min_hits=4)) as r:
        regs, start, o, ps, res = r.orfs(dna, off, 300, 12, 100)
        calls = r.calls().copy()
    orfs, ps, res, junc, jstart, st = M.repair(regs, o, ps, res, calls, dna, off)
    line, files = run("rep", "--repair", "--shifts", str(tmp_path / "rep.shifts"))
    assert st["repaired"] >= 20
    assert line == CR.summary_of(regs, start) + CR.orf_summary(orfs) + CR.repair_summary(st["repaired"], st["candidates"])
    assert files[0] == CR.format_regions(ids, regs, fnames) and files[1] == CR.format_orfs(ids, regs, orfs, fnames)
    assert files[2] == CR.format_faa(ids, regs, orfs, ps, res, fnames)
    assert (tmp_path / "rep.shifts").read_bytes() == CR.format_shifts(ids, regs, orfs, fnames, junc)
    line0, files0 = run("plain", "--select", "--free-orfs", "--coding", "--min-train", "1000", "--starts", "--min-train-starts", "50")
    FE.same_as_recorded("starts_written_select", line0, files0)
