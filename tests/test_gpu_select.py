"""The gene-set selection on the GPU (kg_regionset_select / kg_orfset_select / kg_select_intervals): the device's bytes must
equal the model of tests/select_model.py -- on random lists, known answers, at the edges of the expansion's pair slots
(PPL = _native.SELECT_PAIRS_PER_LANE), on shapes with one huge degree, many rounds or a contig border inside a lane, alone and
among batch neighbours, behind a DNA scan under both strategies, and through the call_regions front end; errors name the
candidate, the pair limit is found before anything is allocated for it and failed allocations leave nothing behind."""
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
import select_model as S  # noqa: E402
import test_orfs_host as HO  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
PPL = N.SELECT_PAIRS_PER_LANE
ROOT = os.path.dirname(HERE)
COUNTS = ("candidates", "eligible", "selected", "overlapped", "pairs", "conflicts")


def _dev(iv, n_seqs, mo=60, pct=50, dst="host", stats=None):
    from kmergutsjava_amd import hotpath
    out = hotpath.select_intervals(iv, n_seqs, mo, pct, device_out=dst == "device", stats=stats)
    return out.cpu().numpy().view(N.SELECTION_DTYPE) if dst == "device" else out


def _check(iv, n_seqs, mo=60, pct=50, dst="host", fast=False):
    """device == model, records and counts; -> the device's statistics"""
    st = {}
    got = _dev(iv, n_seqs, mo, pct, dst, st)
    if fast:
        want = S.select_fast(iv, mo, pct)
    else:
        want, counts = S.select(iv, mo, pct)
        assert {k: st[k] for k in COUNTS} == counts
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert st["candidates"] == len(iv) and st["selected"] == int((want["state"] == 1).sum()) and st["overlapped"] == int((want["state"] == 2).sum())
    return st


@pytest.mark.parametrize("pct", [0, 50, 100])
@pytest.mark.parametrize("mo", [0, 1, 60, 10 ** 6])
def test_random_lists_equal_the_model(mo, pct):
    rng = np.random.default_rng(1000 * pct + mo % 997)
    for k, n in enumerate((0, 1, 2, 3, 17, 64, 65, 300, 1000, 3000)):
        iv = S.random_list(rng, n, n_seqs=1 + k % 4, span=max(40, 30 * n), max_len=int(rng.integers(2, 400)))
        st = _check(iv, 1 + k % 4, mo, pct, "device" if k % 3 == 2 else "host")
        assert st["rounds"] >= (1 if st["eligible"] else 0)
    assert st["pairs"] > 0 and st["ms"] > 0


def test_known_answers():
    def states(rows, mo=60, pct=50, n_seqs=1):
        iv = S.intervals(rows)
        _check(iv, n_seqs, mo, pct)
        got = _dev(iv, n_seqs, mo, pct)
        return got["state"].tolist(), got["by"].tolist()

    # A > B > C, A conflicts with B, B with C, A not with C
    assert states([(0, 0, 99, 30), (0, 50, 149, 20), (0, 100, 199, 10)], 10, 100) == ([1, 2, 1], [-1, 0, -1])
    assert states([(0, 100, 199, 10), (0, 50, 149, 20), (0, 0, 99, 30)], 10, 100) == ([1, 2, 1], [-1, 2, -1])
    # a score tie goes to the longer one, then to the smaller index
    assert states([(0, 0, 99, 5), (0, 0, 119, 5)], 0, 0) == ([2, 1], [1, -1])
    assert states([(0, 0, 99, 5), (0, 0, 99, 5), (0, 0, 99, 5)], 0, 0) == ([1, 2, 2], [-1, 0, 0])
    # ov == max_overlap is no conflict, one more nucleotide is
    assert states([(0, 0, 999, 9), (0, 940, 1939, 8)], 60, 100)[0] == [1, 1]
    assert states([(0, 0, 999, 9), (0, 939, 1938, 8)], 60, 100)[0] == [1, 2]
    # 100 * ov == pct * shorter is no conflict (shorter = 40, ov = 20), ov = 21 is
    assert states([(0, 0, 999, 9), (0, 980, 1019, 8)], 10 ** 6, 50)[0] == [1, 1]
    assert states([(0, 0, 999, 9), (0, 979, 1018, 8)], 10 ** 6, 50)[0] == [1, 2]
    assert states([(0, 0, 999, 9), (0, 999, 1038, 8)], 10 ** 6, 0)[0] == [1, 2]
    assert states([(0, 0, 999, 9), (0, 1000, 1039, 8)], 0, 0)[0] == [1, 1]
    # the last candidate of contig 0 and the first of contig 1 overlap in numbers only
    assert states([(0, 5, 20, 1), (0, 900, 1500, 9), (1, 0, 1400, 3), (1, 2000, 2100, 1)], n_seqs=2)[0] == [1, 1, 1, 1]
    # a non-eligible giant suppresses nothing
    assert states([(0, 0, 10 ** 6, 99, 0), (0, 100, 500, 3), (0, 300, 700, 2)]) == ([0, 1, 2], [-1, -1, 1])
    # by = the smallest index among the winners
    assert states([(0, 300, 399, 1), (0, 350, 600, 8), (0, 100, 349, 9)], 10, 100) == ([2, 1, 1], [1, -1, -1])


def _groups(counts, leader_wins, seq=0, base=0):
    """One group per entry c of counts: a leader with exactly c later candidates overlapping it, which are short, disjoint and
    have no pairs of their own; the groups lie 5000 apart."""
    rows = []
    for g, c in enumerate(counts):
        at = base + 5000 * g
        rows.append((seq, at, at + 30 * c + 40, 50 if leader_wins else 1))
        rows += [(seq, at + 10 + 30 * t, at + 10 + 30 * t + 7, 9 + t % 3) for t in range(c)]
    return rows


@pytest.mark.parametrize("leader_wins", [True, False])
def test_pair_counts_at_the_edges_of_a_lanes_slots(leader_wins):
    counts = (0, 1, PPL - 1, PPL, PPL + 1, 2 * PPL + 1, 0, 0, 1, 1, PPL, 3)
    iv = S.intervals(_groups(counts, leader_wins))
    st = _check(iv, 1)
    assert st["pairs"] == st["conflicts"] == sum(counts)
    rng = np.random.default_rng(5)
    for order in (counts[::-1], tuple(rng.permutation(counts))):
        _check(S.shuffled(rng, S.intervals(_groups(order, leader_wins)))[0], 1, 3, 20)


def test_a_contig_border_inside_a_lanes_pair_slots():
    """Contig 0 ends with a group of 3 pairs and contig 1 begins with one of PPL + 2: the first lane's slots hold both, and the
    coordinates of the two groups overlap in numbers."""
    rows = _groups((3,), True, seq=0) + _groups((PPL + 2, 1), False, seq=1) + _groups((2,), True, seq=3, base=10)
    iv = S.intervals(rows)
    st = _check(iv, 4)
    assert st["pairs"] == 3 + PPL + 2 + 1 + 2
    _check(S.shuffled(np.random.default_rng(1), iv)[0], 4)


@pytest.mark.parametrize("big_wins", [True, False])
def test_one_interval_over_ten_thousand_short_ones(big_wins):
    n = 10 ** 4
    iv = np.zeros(n + 1, dtype=N.INTERVAL_DTYPE)
    iv["left"][1:] = 50 + 20 * np.arange(n)
    iv["right"][1:] = iv["left"][1:] + 11
    iv["score"][1:] = 5 + np.arange(n) % 7
    iv["eligible"] = 1
    iv[0] = (0, 0, 20 * n + 200, 1000 if big_wins else 1, 1)
    iv = np.roll(iv, 4321)                      # the big one somewhere in the middle of the list
    st = _check(iv, 1, fast=True)
    assert st["pairs"] == st["conflicts"] == n and st["selected"] == (1 if big_wins else n) and st["rounds"] <= 3


def test_three_hundred_identical_intervals():
    st = _check(S.identical(300), 1)
    assert st["selected"] == 1 and st["pairs"] == 300 * 299 // 2


def test_a_staircase_of_two_thousand():
    """Every decision waits for the one in front: many rounds, the same result."""
    iv = S.staircase(2000)
    got = _dev(iv, 1, 0, 0)
    assert got["state"].tolist() == [1, 2] * 1000 and got["by"][1::2].tolist() == list(range(0, 2000, 2))
    rng = np.random.default_rng(2)
    mixed, perm = S.shuffled(rng, iv)
    assert _dev(mixed, 1, 0, 0).tobytes() == S.select_fast(mixed, 0, 0).tobytes()


def test_two_to_the_31_pairs_are_refused_before_they_are_allocated():
    from kmergutsjava_amd import hotpath
    iv = np.zeros(70_000, dtype=N.INTERVAL_DTYPE)
    iv["right"], iv["score"], iv["eligible"] = 500, 3, 1
    _check(S.identical(5), 1)                   # once first: what the runtime sets up on first use is not counted
    img, dna, off, _ = _workload()
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        live0 = tab.live_device_bytes()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        with pytest.raises(N.KmerGutsNativeError) as ei:
            hotpath.select_intervals(iv, 1)
        assert ei.value.code == N.KG_ERR_LIMIT and "pairs" in str(ei.value)
        assert tab.live_device_bytes() == live0 and torch.cuda.mem_get_info()[0] == free0


def test_pair_counts_that_wrap_a_32_bit_partial_sum_are_refused():
    """2048 long intervals with lefts 0 .. 2047 over 2^21 disjoint short ones: each long one has 2^21 later overlaps or more, so
    the 2048 counts of the prefix sum's first chunk add up to 2^32 and more, and the true total is 2^32 + 2^21 + 2047 * 1024."""
    from kmergutsjava_amd import hotpath
    n_long, n_short = 2048, 1 << 21
    iv = np.zeros(n_long + n_short, dtype=N.INTERVAL_DTYPE)
    iv["left"][:n_long] = np.arange(n_long)
    iv["right"][:n_long] = 2 * n_short + 10 * n_long
    iv["left"][n_long:] = n_long + 2 * np.arange(n_short)
    iv["right"][n_long:] = iv["left"][n_long:]
    iv["score"], iv["eligible"] = 3, 1
    _check(S.identical(5), 1)                   # once first: what the runtime sets up on first use is not counted
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for order in (iv, iv[::-1].copy()):
        with pytest.raises(N.KmerGutsNativeError) as ei:
            hotpath.select_intervals(order, 1)
        assert ei.value.code == N.KG_ERR_LIMIT and "pairs" in str(ei.value)
        assert torch.cuda.mem_get_info()[0] == free0
    # half as many short ones: 2^31 + 2047 * 1024 pairs, no partial sum wraps, still refused
    half = np.concatenate([iv[:n_long], iv[n_long:n_long + n_short // 2]])
    with pytest.raises(N.KmerGutsNativeError) as ei:
        hotpath.select_intervals(half, 1)
    assert ei.value.code == N.KG_ERR_LIMIT


def test_a_contigs_selection_is_the_same_alone_as_in_a_batch():
    rng = np.random.default_rng(31)
    iv = S.random_list(rng, 2500, n_seqs=12, span=4000, max_len=500)
    whole = _dev(iv, 12, 30, 40)
    for s in range(12):
        idx = np.flatnonzero(iv["seq"] == s)
        sub = iv[idx].copy()
        sub["seq"] = 0
        alone = _dev(sub, 1, 30, 40)
        alone["by"][alone["by"] >= 0] = idx[alone["by"][alone["by"] >= 0]]
        assert alone.tobytes() == whole[idx].tobytes(), s


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


def _after_a_scan(img, dna, off, region_params, min_candidates):
    from kmergutsjava_amd import hotpath
    sb = np.frombuffer(dna, dtype=np.uint8)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        live0 = tab.live_device_bytes()
        with tab.scan(sb, off, hotpath.Params()) as r:
            live1 = tab.live_device_bytes()
            want_regs = r.regions(off, *region_params)
            for mo, pct in ((60, 50), (0, 0)):
                regs, start, sel = r.select(off, None, *region_params, max_overlap=mo, max_overlap_pct=pct)
                assert regs.tobytes() == want_regs[0].tobytes() and start.tobytes() == want_regs[1].tobytes()
                assert sel.tobytes() == S.select_fast(S.of_records(regs), mo, pct).tobytes()
                assert r.select_stats["candidates"] == len(regs) >= min_candidates and r.select_stats["eligible"] == int((regs["kept"] != 0).sum())
                assert r.select_stats["ms"] > 0 and tab.live_device_bytes() == live1
                want_orfs = r.orfs(sb, off, *region_params, only_kept=False)
                got = r.select(off, sb, *region_params, orfs=True, only_kept=False, max_overlap=mo, max_overlap_pct=pct)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:5], want_orfs))
                assert got[5].tobytes() == S.select_fast(S.of_records(got[2]), mo, pct).tobytes()
                assert r.select_stats["selected"] == int((got[5]["state"] == 1).sum()) and tab.live_device_bytes() == live1
        assert tab.live_device_bytes() == live0
    return got


def test_scan_result_select_equals_the_model_on_the_device_records(strategy):
    img, dna, off, genes = _workload()
    got = _after_a_scan(img, dna, off, (300, 10, 90), 20)
    assert (got[5]["state"] == 1).sum() > 20


def test_scan_result_select_on_the_ecoli_genome():
    import test_gpu_regions as GR
    img, dna, off, _ = GR._workload("ecoli")
    got = _after_a_scan(img, dna, off, (600, 0, 0), 100)
    assert (got[5]["state"] == 1).sum() > 100


def test_errors_name_the_first_offending_candidate():
    from kmergutsjava_amd import hotpath
    good = S.intervals([(0, 5, 20, 1), (1, 0, 1400, 3), (0, 900, 1500, 9), (1, 2000, 2100, 1, 0)])
    assert _dev(good, 2)["state"].tolist() == [1, 1, 1, 0]

    def err(iv=good, n_seqs=2, **kw):
        with pytest.raises(N.KmerGutsNativeError) as ei:
            hotpath.select_intervals(iv, n_seqs, **kw)
        return ei.value

    for field, value, which in (("seq", 2, 1), ("seq", -1, 0), ("left", -1, 2), ("right", 4, 0), ("left", 1401, 1), ("seq", 7, 3)):
        bad = good.copy()
        bad[field][which] = value
        if which < 3:
            bad["seq"][3] = -5                  # a later offender does not change the name
        e = err(iv=bad)
        assert e.code == N.KG_ERR_ARG and "candidate %d:" % which in str(e), str(e)
    assert err(n_seqs=0).code == N.KG_ERR_ARG and "candidate 0:" in str(err(n_seqs=0))
    for kw in ({"max_overlap": -1}, {"max_overlap_pct": -1}, {"max_overlap_pct": 101}):
        assert err(**kw).code == N.KG_ERR_ARG
    # through the C ABI: reserved != 0, null pointers, and a range outside the set
    import ctypes as C
    lib, h = N.load(), C.c_void_p()
    assert lib.kg_select_intervals(0, C.byref(N.KgSelectParams(60, 50, 1)), good.ctypes.data, len(good), 2, C.byref(h)) == N.KG_ERR_ARG
    assert b"reserved" in lib.kg_last_error() and not h.value
    assert lib.kg_select_intervals(0, None, good.ctypes.data, len(good), 2, C.byref(h)) == N.KG_ERR_ARG
    assert lib.kg_select_intervals(0, C.byref(N.KgSelectParams(60, 50, 0)), None, len(good), 2, C.byref(h)) == N.KG_ERR_ARG
    assert lib.kg_select_intervals(0, C.byref(N.KgSelectParams(60, 50, 0)), good.ctypes.data, len(good), 2, None) == N.KG_ERR_ARG
    assert lib.kg_regionset_select(None, C.byref(N.KgSelectParams(60, 50, 0)), C.byref(h)) == N.KG_ERR_ARG
    assert lib.kg_orfset_select(None, C.byref(N.KgSelectParams(60, 50, 0)), C.byref(h)) == N.KG_ERR_ARG
    N.check(lib.kg_select_intervals(0, C.byref(N.KgSelectParams(60, 50, 0)), good.ctypes.data, len(good), 2, C.byref(h)))
    try:
        out = np.zeros(4, N.SELECTION_DTYPE)
        assert lib.kg_selectset_count(h) == 4 and lib.kg_selectset_device(h)
        assert lib.kg_selectset_copy(h, 2, 3, out.ctypes.data) == N.KG_ERR_ARG and lib.kg_selectset_copy(h, -1, 1, out.ctypes.data) == N.KG_ERR_ARG
        N.check(lib.kg_selectset_copy(h, 1, 3, out.ctypes.data))
        assert out["state"].tolist() == [1, 1, 0, 0]
    finally:
        lib.kg_selectset_free(h)


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(4)
    iv = S.random_list(rng, 1500, n_seqs=3, span=20000)
    want = S.select_fast(iv)
    img, dna, off, _ = _workload()
    sb = np.frombuffer(dna, dtype=np.uint8)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(sb, off, hotpath.Params()) as r:
        want_r = r.select(off, sb, orfs=True)
        assert len(want_r[5]) > 0
        assert _dev(iv, 3).tobytes() == want.tobytes()       # once first: what the runtime sets up on first use is not counted
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        live0 = tab.live_device_bytes()
        for which in ("list", "result"):
            failed = 0
            for n in range(1, 300):
                monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
                try:
                    got = _dev(iv, 3) if which == "list" else r.select(off, sb, orfs=True)
                    break
                except N.KmerGutsNativeError as e:
                    assert e.code == N.KG_ERR_NOMEM, e
                    failed += 1
                    assert tab.live_device_bytes() == live0
                    if which == "list":
                        assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
            monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
            assert failed >= 15
            if which == "list":
                assert got.tobytes() == want.tobytes()
            else:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want_r))
            assert tab.live_device_bytes() == live0
        # a select set that is still open holds its one block, and gives it back when it is freed
        import ctypes as C
        lib, h, sh = N.load(), C.c_void_p(), C.c_void_p()
        o = np.ascontiguousarray(off, dtype=np.int64)
        N.check(lib.kg_result_regions(r._h, C.byref(N.KgRegionParams(600, 0, 0)), o.ctypes.data, C.byref(h)))
        live_set = tab.live_device_bytes()
        N.check(lib.kg_regionset_select(h, C.byref(N.KgSelectParams(60, 50, 0)), C.byref(sh)))
        assert tab.live_device_bytes() > live_set and lib.kg_selectset_count(sh) == lib.kg_regionset_count(h)
        lib.kg_selectset_free(sh)
        assert tab.live_device_bytes() == live_set
        lib.kg_regionset_free(h)
        assert tab.live_device_bytes() == live0


def test_call_regions_select(oracle, tmp_path):
    """call_regions --select writes the model's text with and without --all, --gff and --faa, and without --select its output is
    what it was."""
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
    base = ["-D", str(d), "-q", str(q), "-m", "4", "--merge-gap", "300", "--min-score", "12", "--min-len", "100"]

    def run(*args):
        p = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.call_regions", *base, *args], capture_output=True, text=True, cwd=ROOT)
        assert p.returncode == 0, p.stderr
        return p.stdout.strip()

    # without --select: today's bytes
    assert run("-o", str(tmp_path / "plain.tsv")) == CR.summary_of(regs, start)
    assert (tmp_path / "plain.tsv").read_bytes() == CR.format_regions(ids, regs, fnames)
    # on the regions' extents, other bounds than the defaults
    rsel, _ = S.select(S.of_records(regs), 20, 10)
    assert run("-o", str(tmp_path / "r.tsv"), "--select", "--max-overlap", "20", "--max-overlap-pct", "10") == \
        CR.summary_of(regs, start) + CR.select_summary(rsel)
    assert (tmp_path / "r.tsv").read_bytes() == CR.format_regions(ids, regs, fnames, sel=rsel)
    assert run("-o", str(tmp_path / "r.gff"), "--select", "--all", "--gff", "--max-overlap", "20", "--max-overlap-pct", "10") == \
        CR.summary_of(regs, start) + CR.select_summary(rsel)
    assert (tmp_path / "r.gff").read_bytes() == CR.format_regions(ids, regs, fnames, True, True, sel=rsel)
    # on the ORFs' extents
    orfs, ps, res = O.orfs(regs, dna, off)
    sel, _ = S.select(S.of_records(orfs))
    assert (sel["state"] == 1).sum() > 10
    line = run("-o", str(tmp_path / "o.tsv"), "--select", "--orfs", str(tmp_path / "orfs.tsv"), "--faa", str(tmp_path / "p.faa"))
    assert line == CR.summary_of(regs, start) + CR.orf_summary(orfs) + CR.select_summary(sel)
    assert (tmp_path / "o.tsv").read_bytes() == CR.format_regions(ids, regs, fnames, sel=sel, cands=orfs)
    assert (tmp_path / "orfs.tsv").read_bytes() == CR.format_orfs(ids, regs, orfs, fnames, sel=sel)
    faa = (tmp_path / "p.faa").read_bytes()
    assert faa == CR.format_faa(ids, regs, orfs, ps, res, fnames, sel=sel) and 10 < faa.count(b">") <= int((sel["state"] == 1).sum())
    heads = [b.split(b" ")[0] for b in faa.split(b">")[1:]]
    assert len(set(heads)) == len(heads), "the writer's dedupe had something left to do"
    # --all: every candidate, three statuses and the winner
    oa = O.orfs(regs, dna, off, only_kept=False)
    sa, _ = S.select(S.of_records(oa[0]))
    line = CR.call_regions(str(d), str(q), str(tmp_path / "a.tsv"), write_all=True, orfs_out=str(tmp_path / "orfs_a.tsv"),
                           faa_out=str(tmp_path / "a.faa"), select=True, **kw)
    assert line == CR.summary_of(regs, start) + CR.orf_summary(oa[0]) + CR.select_summary(sa)
    text = (tmp_path / "a.tsv").read_bytes()
    assert text == CR.format_regions(ids, regs, fnames, True, sel=sa, cands=oa[0]) and len(text.splitlines()) == len(regs)
    assert (tmp_path / "orfs_a.tsv").read_bytes() == CR.format_orfs(ids, regs, oa[0], fnames, True, sel=sa)
    assert (tmp_path / "a.faa").read_bytes() == CR.format_faa(ids, regs, *oa, fnames, True, sel=sa)
    assert {line.split(b"\t")[-2] for line in text.splitlines()} <= {b"kept", b"below", b"overlapped"}
