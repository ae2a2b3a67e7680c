"""Function regions on the GPU (kg_result_regions / kg_regions_calls): the device records must equal the numpy model of
tests/regions_model.py byte for byte, on random CALL lists, known answers, edge shapes, DNA scans of planted contigs and of the
E. coli genome under every scan strategy, and through the call_regions front end, in one batch and in several; the records of a contig do not depend on its
batch; errors name the CALL or contig and failed allocations leave nothing behind."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import regions_model as R  # noqa: E402
import signature_model as M  # noqa: E402
import test_regions_host as H  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(calls, off, gap=600, ms=0, ml=0, dst="host", stats=None):
    from kmergutsjava_amd import hotpath
    regs, start = hotpath.region_calls(calls, off, gap, ms, ml, device_out=dst == "device", stats=stats)
    if dst == "device":
        regs = regs.cpu().numpy().view(N.REGION_DTYPE)
    return regs, start


def _same(got, want):
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("dst", ["host", "device"])
@pytest.mark.parametrize("seed", range(24))
def test_random_lists_equal_the_model(seed, dst):
    rng = np.random.default_rng(seed)
    gap = [0, 1, 10 ** 6][seed % 3]
    if seed % 4 == 3:
        calls, off = R.random_calls_large(rng, int(rng.choice([1, 7, 300])), int(rng.choice([5_000, 100_000])),
                                          int(rng.choice([1, 3, 5000])))
    else:
        calls, off = R.random_calls(rng, int(rng.integers(1, 300)), max_calls=[2, 8, 30][seed % 4],
                                    n_fn=int(rng.choice([1, 3, 60])), max_len=int(rng.choice([30, 100, 2000])))
    ms, ml = int(rng.choice([0, 4, 30])), int(rng.choice([0, 30, 200]))
    st = {}
    got = _dev(calls, off, gap, ms, ml, dst, st)
    want = R.regions(calls, off, gap, ms, ml)
    _same(got, want)
    assert st["calls"] == len(calls) and st["regions"] == len(want[0]) and st["kept"] == want[0]["kept"].sum()
    assert st["multi_frame"] == ((want[0]["frames"] & (want[0]["frames"] - 1)) != 0).sum()


@pytest.mark.parametrize("dst", ["host", "device"])
def test_known_answers(dst):
    off = H.KNOWN_OFF
    r, st = _dev(H._calls([(7, 2, 20, 5, 3, 1.0)]), off, dst=dst)
    assert (r["strand"][0], r["left"][0], r["right"][0]) == (0, 7, 63)
    r, st = _dev(H._calls([(9, 0, 9, 5, 3, 1.0)]), off, dst=dst)
    assert (r["strand"][0], r["left"][0], r["right"][0]) == (1, 70, 99) and st.tolist() == [0, 0, 1]
    c = H._calls([H._x(6, 0, 29, count=4), H._x(7, 40, 48, count=9)])
    r, _ = _dev(c, off, gap=10, dst=dst)
    assert len(r) == 1 and r["frames"][0] == 3
    _same(_dev(c, off, gap=10, dst=dst), R.regions(c, off, 10))
    c = H._calls([H._x(6, 0, 29), H._x(8, 41, 49)])
    assert len(_dev(c, off, gap=10, dst=dst)[0]) == 2
    off4 = np.array([0, 400], np.int64)
    c = H._calls([H._x(0, 0, 299), H._x(0, 30, 59), H._x(1, 310, 318)])
    r, _ = _dev(c, off4, gap=10, dst=dst)
    assert len(r) == 1 and (r["left"][0], r["right"][0], r["n_calls"][0]) == (0, 318, 3)
    assert len(_dev(c, off4, gap=9, dst=dst)[0]) == 2
    big = float(2 ** 24)
    c = H._calls([H._x(6, 60, 68, w=big), H._x(7, 1, 9, w=1.0), H._x(7, 31, 39, w=1.0)])
    r, _ = _dev(c, off, dst=dst)
    assert len(r) == 1 and r["weighted"][0] == np.float32(2 ** 24 + 2)
    _same(_dev(c, off, dst=dst), R.regions(c, off))


def test_edge_shapes():
    empty = np.zeros(0, N.CALL_DTYPE)
    r, st = _dev(empty, np.zeros(1, np.int64))
    assert len(r) == 0 and st.tolist() == [0]
    r, st = _dev(empty, np.arange(8, dtype=np.int64) * 10)
    assert len(r) == 0 and st.tolist() == [0] * 8
    # contigs without CALLs between: one contig of 1e5 CALLs of one function that merge into one region, its neighbour with 1e5
    # CALLs of distinct functions, and one with 1e5 CALLs nested under one long CALL
    n, L = 100_000, 1_000_000
    rng = np.random.default_rng(5)
    off = np.array([0, 0, L, L, 2 * L, 2 * L, 3 * L, 3 * L + 7], np.int64)

    def block(seq, a, b, fI):
        c = np.zeros(n, N.CALL_DTYPE)
        c["container"] = np.sort(6 * seq + rng.integers(0, 3, size=n))
        c["start"], c["end"] = a, b
        c["count"] = rng.integers(0, 9, size=n)
        c["fI"] = fI
        c["weightedHits"] = rng.choice(np.array([0.5, 1.0, 0.1, 2.0 ** 24], np.float32), size=n)
        return c

    a = rng.integers(0, L // 3 - 40, size=n)
    merged = block(1, a, a + 30, 7)
    distinct = block(3, a, a + 30, rng.permutation(n) * 5 - 70_000)
    nested = block(5, a, a + 30, 2)
    nested["container"][0], nested["start"][0], nested["end"][0] = 30, 0, L // 3 - 2
    calls = np.concatenate([merged, distinct, nested])
    st = {}
    got = _dev(calls, off, 600, stats=st)
    _same(got, R.regions(calls, off, 600))
    start = got[1]
    assert start.tolist() == [0, 0, 1, 1, 1 + n, 1 + n, 2 + n, 2 + n] and st["groups"] == n + 2
    assert got[0]["n_calls"][0] == n and got[0]["n_calls"][-1] == n
    # with merge_gap 0 the nested contig still is one region: the running maximum of the long CALL covers the rest
    got0 = _dev(calls, off, 0)
    _same(got0, R.regions(calls, off, 0))
    assert got0[1][-2] - got0[1][-3] == 1


def test_two_million_contigs():
    rng = np.random.default_rng(9)
    calls, off = R.random_calls_large(rng, 2_000_000, 3_000_000, 4000, contig_len=3000, span=200)
    _same(_dev(calls, off), R.regions(calls, off))


@pytest.fixture(params=["direct", "partitioned", "partitioned_tags"])
def strategy(request, monkeypatch):
    """The scan strategies of the parity tests (tests/test_gpu_parity.py)."""
    monkeypatch.setenv("KG_PARTITION", "0" if request.param == "direct" else "1")
    monkeypatch.setenv("KG_DIRECT_FILTER", "2")
    if request.param == "partitioned_tags":
        monkeypatch.setenv("KG_BIDX", "0")
    return request.param


_WORK = {}


def _workload(name):
    """(table image, dna, offsets), made once per session"""
    if name not in _WORK:
        if name == "planted":
            img, dna, off, _ = H.planted_contigs()
        else:
            from kmergutsjava_amd import synth
            from kmergutsjava_amd.make_signatures import parse_fasta
            from kmergutsjava_amd.make_table import default_num_sigs
            ids, seqs = parse_fasta(gzip.decompress(open(os.path.join(HERE, "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))
            poff = np.zeros(len(seqs) + 1, dtype=np.int64)
            poff[1:] = np.cumsum([len(s) for s in seqs])
            rng = np.random.default_rng(77)
            fn = rng.integers(0, 300, size=len(seqs)).astype(np.int32)
            fn[rng.random(len(seqs)) < 0.2] = -1
            otu = rng.integers(0, 4, size=len(seqs)).astype(np.int32)
            sigs = M.derive(b"".join(seqs), poff, fn, otu, 1, 1)
            rec, _ = synth.build_table(torch.from_numpy(sigs["kmer"].copy()),
                                       tuple(torch.from_numpy(sigs[k].copy()) for k in ("otuIndex", "avgFromEnd", "functionIndex", "functionWt")),
                                       default_num_sigs(len(sigs)))
            img = synth.table_image(rec)
            _, contigs = parse_fasta(gzip.decompress(open(os.path.join(HERE, "golden", "Ecoli_K12_W3110.fna.gz"), "rb").read()))
            dna = b"".join(contigs)
            off = np.zeros(len(contigs) + 1, dtype=np.int64)
            off[1:] = np.cumsum([len(s) for s in contigs])
        _WORK[name] = (img, dna, off, {})
    return _WORK[name]


@pytest.mark.parametrize("oc", [False, True])
@pytest.mark.parametrize("workload", ["planted", "ecoli"])
def test_scan_regions_equal_the_model_on_oracle_records(oracle, strategy, workload, oc):
    from kmergutsjava_amd import hotpath
    img, dna, off, ora_cache = _workload(workload)
    sb = np.frombuffer(dna, dtype=np.uint8)
    if oc not in ora_cache:
        ora_cache[oc] = oracle.run(img, sb, off, lookup_mode=1, order_constraint=oc)["calls"]
    calls = ora_cache[oc]
    assert len(calls) > 100
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        live0 = tab.live_device_bytes()
        with tab.scan(sb, off, hotpath.Params(order_constraint=oc)) as r:
            live1 = tab.live_device_bytes()
            for gap, ms, ml in ((600, 0, 0), (0, 10, 60), (30, 0, 300)):
                want = R.regions(calls, off, gap, ms, ml)
                got = r.regions(off, gap, ms, ml)
                _same(got, want)
                assert r.region_stats["ms"] > 0 and r.region_stats["regions"] == len(want[0])
                d, start = r.regions(off, gap, ms, ml, device_out=True)
                assert d.cpu().numpy().tobytes() == want[0].tobytes() and start.tobytes() == want[1].tobytes()
                assert tab.live_device_bytes() == live1
            assert len(got[0]) > 20
        assert tab.live_device_bytes() == live0


def test_records_do_not_depend_on_the_batch():
    from kmergutsjava_amd import hotpath
    img, dna, off, _ = _workload("planted")
    n = len(off) - 1
    contigs = [dna[off[k]:off[k + 1]] for k in range(n)]

    def scan(order):
        o = np.zeros(len(order) + 1, dtype=np.int64)
        o[1:] = np.cumsum([len(contigs[k]) for k in order])
        with tab.scan(np.frombuffer(b"".join(contigs[k] for k in order), dtype=np.uint8), o, hotpath.Params()) as r:
            regs, start = r.regions(o)
        out = {}
        for j, k in enumerate(order):
            x = regs[start[j]:start[j + 1]].copy()
            assert (x["seq"] == j).all()
            x["seq"] = k
            x["first_call"] = 0           # an index into the batch's calls[]
            out[k] = x.tobytes()
        return out

    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        whole = scan(list(range(n)))
        assert sum(len(v) for v in whole.values()) > 0
        shuffled = scan([int(k) for k in np.random.default_rng(3).permutation(n)])
        assert shuffled == whole
        for k in range(0, n, 5):
            assert scan([k])[k] == whole[k]


def test_errors_name_the_call_or_contig():
    from kmergutsjava_amd import hotpath
    off = H.KNOWN_OFF
    good = H._calls([H._x(0, 0, 29), H._x(6, 0, 29), H._x(7, 40, 48), H._x(9, 0, 29)])

    def err(calls=good, o=off, **kw):
        with pytest.raises(N.KmerGutsNativeError) as ei:
            hotpath.region_calls(calls, o, **kw)
        return ei.value

    assert len(hotpath.region_calls(good, off)[0]) == 3
    bad = good.copy()
    bad["container"][3] = 12
    e = err(calls=bad)
    assert e.code == N.KG_ERR_ARG and "CALL 3" in str(e) and "container" in str(e)
    bad = good.copy()
    bad["container"][2] = 5
    e = err(calls=bad)
    assert e.code == N.KG_ERR_ARG and "CALL 2" in str(e) and "order" in str(e)
    bad = good.copy()
    bad["count"][1] = -3
    e = err(calls=bad)
    assert e.code == N.KG_ERR_ARG and "CALL 1" in str(e) and "count" in str(e)
    for field, value, which in (("end", 40, 3), ("start", -1, 1), ("end", 16, 0), ("start", 16, 2)):
        bad = good.copy()                  # beyond the contig's end, before its start, beyond contig 0's 50 nt, end < start
        bad[field][which] = value
        e = err(calls=bad)
        assert e.code == N.KG_ERR_ARG and "CALL %d" % which in str(e) and "outside" in str(e), str(e)
    e = err(o=np.array([0, 50, 40], np.int64))
    assert e.code == N.KG_ERR_ARG and "contig 1" in str(e)
    huge = good.copy()
    huge["count"][1:3] = 2 ** 30
    e = err(calls=huge)
    assert e.code == N.KG_ERR_LIMIT and "CALL 1" in str(e)
    assert err(calls=good[:1], o=np.zeros(1, np.int64)).code == N.KG_ERR_ARG
    for kw in ({"merge_gap": -1}, {"min_score": -1}, {"min_len": -1}):
        assert err(**kw).code == N.KG_ERR_ARG


def test_protein_and_skip_aggregate_results_are_refused():
    from kmergutsjava_amd import hotpath
    seq, off, fn, otu = M.family_set(10, 4, 200, 0.04, 3)
    img, dna, doff, _ = _workload("planted")
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        with tab.scan(np.frombuffer(seq, dtype=np.uint8), off, hotpath.Params(aa=True)) as r:
            with pytest.raises(N.KmerGutsNativeError) as ei:
                r.regions(off)
            assert ei.value.code == N.KG_ERR_ARG and "protein" in str(ei.value)
        with tab.scan(np.frombuffer(dna, dtype=np.uint8), doff, hotpath.Params(skip_aggregate=True)) as r:
            with pytest.raises(N.KmerGutsNativeError) as ei:
                r.regions(doff)
            assert ei.value.code == N.KG_ERR_ARG and "SKIP_AGGREGATE" in str(ei.value)
        assert tab.live_device_bytes() == 0


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(4)
    calls, off = R.random_calls_large(rng, 50, 20_000, 30)
    want = R.regions(calls, off)
    img, dna, doff, _ = _workload("planted")
    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(np.frombuffer(dna, dtype=np.uint8), doff, hotpath.Params()) as r:
        want_r = r.regions(doff)
        assert len(want_r[0]) > 0
        # once on the device first, so that what the runtime sets up on first use is not counted
        _same(hotpath.region_calls(calls, off), want)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        live0 = tab.live_device_bytes()
        for which in ("calls", "result"):
            failed = 0
            for n in range(1, 200):
                monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
                try:
                    got = hotpath.region_calls(calls, off) if which == "calls" else r.regions(doff)
                    break
                except N.KmerGutsNativeError as e:
                    assert e.code == N.KG_ERR_NOMEM, e
                    failed += 1
                    assert tab.live_device_bytes() == live0
                    if which == "calls":
                        assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
            monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
            assert failed >= 20
            _same(got, want if which == "calls" else want_r)
            assert tab.live_device_bytes() == live0        # the freed set gave its two blocks back
        # a set that is still open holds its blocks, and gives them back when it is freed
        import ctypes as C
        lib, h = N.load(), C.c_void_p()
        o = np.ascontiguousarray(doff, dtype=np.int64)
        N.check(lib.kg_result_regions(r._h, C.byref(N.KgRegionParams(600, 0, 0)), o.ctypes.data, C.byref(h)))
        assert tab.live_device_bytes() > live0 and lib.kg_regionset_count(h) == len(want_r[0])
        lib.kg_regionset_free(h)
        assert tab.live_device_bytes() == live0


@pytest.mark.parametrize("gz", [False, True])
def test_call_regions_front_end(oracle, tmp_path, gz):
    from kmergutsjava_amd import call_regions as CR
    from kmergutsjava_amd import synth
    img, dna, off, _ = _workload("planted")
    n = len(off) - 1
    ids = [b"contig_%d" % k for k in range(n)]
    fa = b"".join(b">%s planted genes\n%s\n" % (ids[k], dna[off[k]:off[k + 1]]) for k in range(n))
    q = tmp_path / ("c.fna.gz" if gz else "c.fna")
    q.write_bytes(gzip.compress(fa) if gz else fa)
    d = tmp_path / "d"
    synth.write_data_dir(str(d), img, 50, gz=gz)
    fnames = [b"synthetic function %d" % i for i in range(50)]
    calls = oracle.run(img, np.frombuffer(dna, dtype=np.uint8), off, lookup_mode=1, min_hits=4)["calls"]
    root = os.path.dirname(HERE)
    for extra, kw in ((["--all"], {"write_all": True}), (["--gff"], {"gff": True}), ([], {}), (["--all", "--gff"], {"write_all": True, "gff": True})):
        want = R.regions(calls, off, 300, 12, 100)
        out = tmp_path / "o.txt"
        p = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.call_regions", "-D", str(d), "-q", str(q), "-o", str(out), "-m", "4",
                            "--merge-gap", "300", "--min-score", "12", "--min-len", "100"] + extra, capture_output=True, text=True,
                           cwd=root)
        assert p.returncode == 0, p.stderr
        assert out.read_bytes() == CR.format_regions(ids, want[0], fnames, **kw)
        assert p.stdout.strip() == CR.summary_of(*want)
        assert 0 < want[0]["kept"].sum() < len(want[0])
    p = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.call_regions", "-D", str(tmp_path / "nothing"), "-q", str(q), "-o",
                        str(tmp_path / "x")], capture_output=True, text=True, cwd=root)
    assert p.returncode == 1 and p.stderr.startswith("Error:")


def test_call_regions_front_end_in_several_batches(oracle, tmp_path):
    """call_regions cuts its input at KmerGutsJava.MAX_BATCH_CHARS, rebases seq and joins region_start: the file and the
    summary line do not depend on the cap, and equal the model's on the oracle's CALLs of the whole input."""
    from helpers import batch_caps, front_end_batches
    from kmergutsjava_amd import call_regions as CR
    from kmergutsjava_amd import synth
    from kmergutsjava_amd.kmer_guts_java import KmerGutsJava
    img, dna, off, _ = _workload("planted")
    rng = np.random.default_rng(11)
    seqs = [dna[off[k]:off[k + 1]] for k in range(len(off) - 1)]

    def spacer(n):
        return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))

    seqs.insert(10, spacer(3000))           # no gene: a batch without any region when it is alone
    seqs.insert(20, spacer(40_000))         # longer than the "several" cap
    seqs.append(spacer(700))
    n = len(seqs)
    lens = [len(x) for x in seqs]
    ids = [b"contig_%d" % k for k in range(n)]
    q = tmp_path / "c.fna"
    q.write_bytes(b"".join(b">%s planted genes\n%s\n" % (ids[k], seqs[k]) for k in range(n)))
    d = tmp_path / "d"
    synth.write_data_dir(str(d), img, 50)
    fnames = [b"synthetic function %d" % i for i in range(50)]
    off2 = np.zeros(n + 1, dtype=np.int64)
    off2[1:] = np.cumsum(lens)
    calls = oracle.run(img, np.frombuffer(b"".join(seqs), dtype=np.uint8), off2, lookup_mode=1, min_hits=4)["calls"]
    want = R.regions(calls, off2, 300, 12, 100)
    per = np.diff(want[1])
    assert per[10] == 0 and per[:10].sum() > 0 and per[11:20].sum() > 0 and 0 < want[0]["kept"].sum() < len(want[0])
    caps = batch_caps(lens)
    assert len(front_end_batches(lens, KmerGutsJava.MAX_BATCH_CHARS)) == 1
    assert (10, 11) in front_end_batches(lens, caps["one_each"]) and (20, 21) in front_end_batches(lens, caps["several"])
    keep = KmerGutsJava.MAX_BATCH_CHARS
    try:
        for what, cap in [("default", keep)] + sorted(caps.items()):
            KmerGutsJava.MAX_BATCH_CHARS = cap
            for kw in ({"write_all": True}, {"gff": True}):
                out = tmp_path / "o.txt"
                line = CR.call_regions(str(d), str(q), str(out), min_hits=4, merge_gap=300, min_score=12, min_len=100, **kw)
                assert out.read_bytes() == CR.format_regions(ids, want[0], fnames, **kw), (what, cap, kw)
                assert line == CR.summary_of(*want), (what, cap, kw)
    finally:
        KmerGutsJava.MAX_BATCH_CHARS = keep
