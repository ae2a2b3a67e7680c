"""Deriving signatures on the GPU (kg_signatures_derive / kg_signatures_derive_device): the device set must equal the torch
model of tests/signature_model.py byte for byte on every input, for any protein order, pass count and entry point; the set
must build a table that scans like the oracle; make_signatures -D must write a directory both front ends read."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import signature_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


def _derive(seq, off, fn, otu, entry="host", **kw):
    from kmergutsjava_amd import hotpath
    if entry == "device":
        d = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
        with hotpath.derive_signatures(None, off, fn, otu, device_ptr=d.data_ptr() if d.numel() else 0, **kw) as s:
            return s.numpy(), s.stats()
    with hotpath.derive_signatures(seq, off, fn, otu, **kw) as s:
        return s.numpy(), s.stats()


def _check(seq, off, fn, otu, minp=2, pur=80, entry="host", **kw):
    got, st = _derive(seq, off, fn, otu, entry, min_proteins=minp, purity_pct=pur, **kw)
    want = M.derive(seq, off, fn, otu, minp, pur)
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()
    assert st["signatures"] == len(want) and st["proteins"] == len(off) - 1
    return got, st


def _join(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return b"".join(seqs), off


@pytest.mark.parametrize("minp,pur", [(1, 1), (1, 100), (2, 80), (3, 50), (2, 100), (5, 67)])
def test_families_equal_the_model(minp, pur):
    seq, off, fn, otu = M.family_set(60, 12, 300, 0.04, 11 + minp * 7 + pur)
    got, st = _check(seq, off, fn, otu, minp, pur)
    assert len(got) > 100
    assert st["valid_windows"] >= st["pairs"] >= st["kmers"] >= st["signatures"]


def test_ties_of_function_and_otu():
    # one shared 9-mer prefix; fn counts 0:2, 1:2, 2:1 -> f* = 0 (tie, smallest); OTUs among fn 0: 7 and 4 -> 4
    base = b"MKVLAAGIWQ"
    seqs = [base + b"C" * k for k in range(5)]
    seq, off = _join(seqs)
    fn = np.array([1, 0, 2, 1, 0], np.int32)
    otu = np.array([9, 7, 9, 9, 4], np.int32)
    got, _ = _check(seq, off, fn, otu, 1, 1)
    assert set(got["functionIndex"]) <= {0, 1, 2} and (got["functionIndex"][:2] == 0).all()
    assert (got["otuIndex"][:2] == 4).all()


@pytest.mark.parametrize("case", ["unannotated", "empty", "short", "dirty", "no_proteins"])
def test_edge_inputs(case):
    rng = np.random.default_rng(3)
    if case == "no_proteins":
        got, st = _check(b"", np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
        assert len(got) == 0 and st["windows"] == 0
        return
    seq, off, fn, otu = M.family_set(20, 6, 120, 0.02, 4)
    if case == "unannotated":
        fn[:] = -1
    elif case == "empty":
        seq, off = _join([b""] * len(fn))
    elif case == "short":
        seqs = [seq[off[i]:off[i] + int(rng.integers(0, 10))] for i in range(len(fn))]
        seq, off = _join(seqs)
    elif case == "dirty":
        a = np.frombuffer(seq, dtype=np.uint8).copy()
        pos = rng.integers(0, a.size, size=a.size // 30)
        a[pos] = rng.choice(np.frombuffer(b"acdXx*B-", dtype=np.uint8), size=pos.size)
        seq = a.tobytes()
    got, _ = _check(seq, off, fn, otu, 1, 1)
    if case in ("unannotated", "empty"):
        assert len(got) == 0


def test_one_kmer_in_many_proteins():
    n = 120_000
    rng = np.random.default_rng(8)
    alpha = np.frombuffer(M.ALPHA, dtype=np.uint8)
    tails = alpha[rng.integers(0, 20, size=(n, 6))]
    seqs = [b"WWWWWWWWW" + t.tobytes() for t in tails]
    seq, off = _join(seqs)
    fn = rng.integers(-1, 4, size=n).astype(np.int32)
    fn[: n // 2] = 2
    otu = rng.integers(0, 5, size=n).astype(np.int32)
    got, st = _check(seq, off, fn, otu, 2, 50)
    w = got[got["kmer"] == 18 * sum(20 ** k for k in range(8))]            # WWWWWWWW (W is code 18)
    assert len(w) == 1 and int(w[0]["functionIndex"]) == 2


def test_many_passes_give_the_same_bytes():
    from kmergutsjava_amd import _native as N
    seq, off, fn, otu = M.family_set(80, 10, 400, 0.05, 21)
    one, st1 = _derive(seq, off, fn, otu)
    assert st1["passes"] == 1
    cap = st1["valid_windows"] // 7
    many, st = _derive(seq, off, fn, otu, max_windows_per_pass=cap)
    assert st["passes"] >= 5 and many.tobytes() == one.tobytes()
    assert one.tobytes() == M.derive(seq, off, fn, otu).tobytes()
    # one k-mer alone over the cap
    seq2, off2 = _join([b"AAAAAAAAAAAAAAAAAAAAAAAAAAAA"] * 3)
    with pytest.raises(N.KmerGutsNativeError) as ei:
        _derive(seq2, off2, np.zeros(3, np.int32), np.zeros(3, np.int32), max_windows_per_pass=50)
    assert ei.value.code == N.KG_ERR_LIMIT and "alone occurs in 60 valid windows" in str(ei.value)
    got, st = _derive(seq2, off2, np.zeros(3, np.int32), np.zeros(3, np.int32), max_windows_per_pass=60)
    assert len(got) == 1 and st["passes"] == 1


def test_protein_order_and_entry_points_do_not_matter():
    seq, off, fn, otu = M.family_set(50, 10, 250, 0.05, 31)
    a, _ = _check(seq, off, fn, otu, entry="host")
    b, _ = _check(seq, off, fn, otu, entry="device")
    perm = np.random.default_rng(2).permutation(len(fn))
    s2, o2 = _join([seq[off[i]:off[i + 1]] for i in perm])
    c, _ = _derive(s2, o2, fn[perm], otu[perm])
    assert a.tobytes() == b.tobytes() == c.tobytes()


def _ecoli():
    from kmergutsjava_amd.make_signatures import parse_fasta
    ids, seqs = parse_fasta(gzip.decompress(open(os.path.join(HERE, "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))
    seq, off = _join(seqs)
    rng = np.random.default_rng(77)
    n = len(seqs)
    fn = rng.integers(0, 300, size=n).astype(np.int32)
    fn[rng.random(n) < 0.2] = -1
    otu = rng.integers(0, 4, size=n).astype(np.int32)
    return seq, off, fn, otu


def test_ecoli_proteins():
    seq, off, fn, otu = _ecoli()
    for minp, pur in ((1, 1), (2, 80)):
        got, _ = _check(seq, off, fn, otu, minp, pur)
        got_d, _ = _check(seq, off, fn, otu, minp, pur, entry="device")
        assert got.tobytes() == got_d.tobytes()
    assert len(got) > 0


@pytest.mark.parametrize("entry", ["host", "device"])
def test_errors_name_the_protein(entry):
    from kmergutsjava_amd import _native as N
    seq, off = _join([b"ACDEFGHIKLMN"] * 4)
    z = np.zeros(4, np.int32)

    def err(fn=z, otu=z, off=off, **kw):
        with pytest.raises(N.KmerGutsNativeError) as ei:
            _derive(seq, off, fn, otu, entry, **kw)
        return ei.value

    e = err(fn=np.array([0, 0, -2, 0], np.int32))
    assert e.code == N.KG_ERR_ARG and "protein 2" in str(e)
    e = err(otu=np.array([0, 0, 0, -1], np.int32))
    assert e.code == N.KG_ERR_ARG and "protein 3" in str(e)
    _derive(seq, off, np.array([0, -1, 0, 0], np.int32), np.array([0, -5, 0, 0], np.int32), entry)   # ignored when fn = -1
    e = err(off=np.array([0, 12, 10, 36, 48], np.int64))
    assert e.code == N.KG_ERR_ARG and "protein 1" in str(e)
    for kw in ({"min_proteins": 0}, {"purity_pct": 0}, {"purity_pct": 101}, {"max_windows_per_pass": -1}):
        assert err(**kw).code == N.KG_ERR_ARG


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    from kmergutsjava_amd import _native as N
    seq, off, fn, otu = M.family_set(30, 8, 200, 0.05, 41)
    want, _ = _derive(seq, off, fn, otu, max_windows_per_pass=15000)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    failed = 0
    for n in range(1, 400):
        monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
        try:
            got, _ = _derive(seq, off, fn, otu, max_windows_per_pass=15000)
            break
        except N.KmerGutsNativeError as e:
            assert e.code == N.KG_ERR_NOMEM, e
            failed += 1
            assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
    monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
    assert failed >= 20 and got.tobytes() == want.tobytes()
    got, _ = _derive(seq, off, fn, otu, max_windows_per_pass=15000)
    assert got.tobytes() == want.tobytes()
    assert torch.cuda.mem_get_info()[0] == free0


@pytest.mark.parametrize("oc", [False, True])
def test_end_to_end_table_and_scans(oracle, oc):
    from helpers import assert_same_records
    from kmergutsjava_amd import hotpath, synth
    from kmergutsjava_amd.make_table import default_num_sigs
    seq, off, fn, otu = M.family_set(80, 10, 300, 0.04, 51)
    want = M.derive(seq, off, fn, otu)
    S = default_num_sigs(len(want))
    rec, placed = synth.build_table(torch.from_numpy(want["kmer"].copy()),
                                    tuple(torch.from_numpy(want[k].copy()) for k in ("otuIndex", "avgFromEnd", "functionIndex", "functionWt")), S)
    img = synth.table_image(rec)
    with hotpath.derive_signatures(seq, off, fn, otu) as s:
        with hotpath.SignatureTable.build(s.device_tensor(), S) as tab:
            assert tab.placed == placed
            body = tab.device_entries().cpu().numpy().tobytes()
            assert body == img[24:]
            sb = np.frombuffer(seq, dtype=np.uint8)
            ora = oracle.run(img, sb, off, aa=True, lookup_mode=1, order_constraint=oc)
            with tab.scan(sb, off, hotpath.Params(aa=True, order_constraint=oc)) as r:
                assert_same_records(r, ora, "derived table oc=%s" % oc)
            assert len(ora["calls"]) > 100


def test_make_signatures_directory_is_read_by_both_front_ends(tmp_path):
    from kmergutsjava_amd import build, KmerGutsJava
    from kmergutsjava_amd import make_table as MT
    seq, off, fn, otu = M.family_set(40, 8, 300, 0.04, 61, n_fn=12)
    names = [b"fn_%02d" % (11 - f) for f in range(12)]          # byte order reverses the numbering
    fa = b"".join(b">prot%d desc\n%s\n" % (i, seq[off[i]:off[i + 1]]) for i in range(len(fn)))
    (tmp_path / "p.faa.gz").write_bytes(gzip.compress(fa))
    tsv = b"".join(b"prot%d\t%s\tO%d\n" % (i, names[f], otu[i]) for i, f in enumerate(fn) if f >= 0)
    (tmp_path / "a.tsv").write_bytes(tsv)
    out = tmp_path / "d"
    p = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.make_signatures", "-p", str(tmp_path / "p.faa.gz"), "-A",
                        str(tmp_path / "a.tsv"), "-o", str(tmp_path / "s.txt"), "-D", str(out)], capture_output=True, text=True,
                       cwd=os.path.dirname(HERE))
    assert p.returncode == 0, p.stderr
    # the model on the front end's numbering
    fmap = {n: i for i, n in enumerate(sorted(set(names[f] for f in fn if f >= 0)))}
    fn2 = np.array([fmap[names[f]] if f >= 0 else -1 for f in fn], np.int32)
    onames = sorted(set(b"O%d" % otu[i] for i in range(len(fn)) if fn[i] >= 0))
    otu2 = np.array([onames.index(b"O%d" % otu[i]) if fn[i] >= 0 else 0 for i in range(len(fn))], np.int32)
    want = M.derive(seq, off, fn2, otu2)
    assert MT.parse_signatures((tmp_path / "s.txt").read_bytes()).tobytes() == want.tobytes()
    S = MT.default_num_sigs(len(want))
    assert p.stdout.strip() == "Proteins: %d, windows: %d, signatures: %d, slots: %d, placed: %d" % (
        len(fn), _derive(seq, off, fn2, otu2)[1]["valid_windows"], len(want), S, len(want))
    assert (out / "function.index").read_bytes() == b"".join(b"%d\t%s\n" % (i, n) for i, n in enumerate(sorted(fmap)))
    assert (out / "otu.index").read_bytes() == b"".join(b"%d\t%s\n" % (i, n) for i, n in enumerate(onames))
    (tmp_path / "q.fa").write_bytes(fa)
    cli = build.build_cli()
    subprocess.run([cli, "-D", str(out), "-a", "-q", str(tmp_path / "q.fa"), "-o", str(tmp_path / "cli.txt")], check=True,
                   stdout=subprocess.DEVNULL)
    KmerGutsJava.main(["-D", str(out), "-a", "-q", str(tmp_path / "q.fa"), "-o", str(tmp_path / "java.txt")])
    cli_txt, java_txt = (tmp_path / "cli.txt").read_text(), (tmp_path / "java.txt").read_text()
    assert "CALL" in cli_txt and cli_txt == java_txt
