"""Composition binning on the GPU (kg_contigs_compose): the classes, the per-contig counts, the label rows, the background and
the score matrix must equal the model of tests/compose_model.py byte for byte -- on random batches around the count pass's
step, with label sets around the score pass's LDS tile, with a caller's model, cut into two calls at every contig boundary, and
through classify_contigs --compose on a planted two-genome sample; errors name the first offender and failed allocations leave
nothing behind.  There is no tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compose_cases as KC  # noqa: E402
import compose_model as K  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

ARRAYS = ("classes", "counts", "row_labels", "rows", "background", "model_labels")


def _dev(seq, off, labels=None, model=None, dst="host", **kw):
    from kmergutsjava_amd import hotpath
    st = {}
    got = hotpath.compose_contigs(seq, off, labels, model, device_out=(dst == "device"), stats=st, **kw)
    if dst == "device":
        got["classes"] = got["classes"].cpu().numpy().view(N.COMP_CLASS_DTYPE)
        for name in ("counts", "scores"):
            if name in got:
                got[name] = got[name].cpu().numpy()
    return got, st


def _same(got, want, what="", scores=False):
    for name in ARRAYS + (("scores",) if scores else ()):
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            at = np.argwhere(np.atleast_1d(g != w))[:3].tolist()
            raise AssertionError((what, name, at, [(g[tuple(i)], w[tuple(i)]) for i in at]))


def _stats_same(st, want):
    for k, v in want["stats"].items():
        assert st[k] == v, (k, st[k], v)


_WANT = {}


def _want(name):
    if name not in _WANT:
        seq, off, lab = KC.case(name)
        _WANT[name] = ((seq, off, lab), K.compose(seq, off, lab, None, min_len=200, min_margin=100, min_train=1000))
    return _WANT[name]


@pytest.mark.parametrize("dst", ["host", "device"])
@pytest.mark.parametrize("name", KC.CASES)
def test_random_batches_equal_the_model(name, dst):
    (seq, off, lab), want = _want(name)
    got, st = _dev(seq, off, lab, None, dst, min_len=200, min_margin=100, min_train=1000, keep_scores=True)
    _same(got, want, name, scores=True)
    _stats_same(st, want)
    if name == "edges":
        assert np.diff(off).tolist()[:len(KC.EDGES)] == KC.EDGES and {KC.STEP - 1, KC.STEP, KC.STEP + 1} <= set(KC.EDGES)
        homo = want["counts"][len(off) - 3]
        assert homo[0] == homo[255] == 5000 - 3 and homo.sum() == 2 * (5000 - 3)
        assert want["stats"]["models"] == 3 and want["stats"]["decided"] > 0 and st["ms_count"] > 0 and st["ms_score"] > 0
    if name == "many_short":
        assert len(lab) == 70_000 and want["stats"]["models"] == 5
    if name == "four_mbp":
        assert want["classes"]["windows"][1] > 4_400_000 and len(seq) > N.COMP_TILE * N.COMP_MAX_GRID
    if name == "empty":
        assert st["seqs"] == 0 and got["scores"].shape == (0, 1) and got["background"].sum() == 0


@pytest.mark.parametrize("name", KC.LABEL_CASES)
def test_labels_and_models_equal_the_model(name):
    seq, off, lab, min_train = KC.label_case(name)
    kw = dict(min_len=100, min_margin=64, min_train=min_train)
    want = K.compose(seq, off, lab, None, **kw)
    got, st = _dev(seq, off, lab, None, keep_scores=True, **kw)
    _same(got, want, name, scores=True)
    _stats_same(st, want)
    M, R = st["models"], st["label_rows"]
    if name == "all_unlabelled":
        assert (M, R) == (0, 0) and (got["classes"]["best"] == -1).all() and st["decided"] == 0
        # labels=None is all -1
        _same(_dev(seq, off, None, None, keep_scores=True, **kw)[0], want, name, scores=True)
    elif name == "one_label":
        assert (M, R) == (1, 1) and got["model_labels"].tolist() == [12]
    elif name == "zero_and_top":
        assert got["model_labels"].tolist() == [0, 2 ** 31 - 1] and set(got["classes"]["best"].tolist()) <= {-1, 0, 2 ** 31 - 1}
    elif name.startswith("models_"):
        assert M == R == int(name.split("_")[1]) and got["scores"].shape == (len(lab), M + 1)
    else:
        assert 1 < M < R


def test_default_parameters_and_no_kept_scores():
    seq, off, lab, _ = KC.label_case("models_%d" % KC.TILE)
    want = K.compose(seq, off, lab)
    got, st = _dev(seq, off, lab)
    _same(got, want)
    assert "scores" not in got and st["models"] == 0         # (no row has 200 000 windows)
    # the matrix does not exist: the getter says so
    p = N.KgCompParams(1500, 2560, 200000, 0, 0)
    h = C.c_void_p()
    lib = N.load()
    N.check(lib.kg_contigs_compose(0, C.byref(p), seq.ctypes.data, 0, off.ctypes.data, len(lab), lab.ctypes.data, None, None, 0, C.byref(h)))
    try:
        one = np.zeros(1, np.int64)
        assert lib.kg_compset_copy_scores(h, 0, 1, one.ctypes.data) == N.KG_ERR_ARG and b"keep_scores" in lib.kg_last_error()
        part = np.zeros(3, N.COMP_CLASS_DTYPE)
        N.check(lib.kg_compset_copy_classes(h, 5, 3, part.ctypes.data))
        assert part.tobytes() == want["classes"][5:8].tobytes()
        cnt = np.zeros((2, 256), np.int32)
        N.check(lib.kg_compset_copy_counts(h, 699, 1, cnt.ctypes.data))
        assert np.array_equal(cnt[0], want["counts"][699])
        assert lib.kg_compset_copy_counts(h, 699, 2, cnt.ctypes.data) == N.KG_ERR_ARG
        assert lib.kg_compset_copy_rows(h, 0, KC.TILE + 1, None, None) == N.KG_ERR_ARG
        assert lib.kg_compset_rows(h) == KC.TILE and lib.kg_compset_models(h) == 0
    finally:
        lib.kg_compset_free(h)


def _nine():
    rng = np.random.default_rng(99)
    seq, off, lab = KC.batch(rng, [300, 0, 65, 4097, 1, 64, KC.STEP, 3, 257], 3)
    lab[:] = [0, 1, -1, 0, 2, 1, 2, -1, 1]
    return seq, off, lab


def test_launch_independence_two_calls_at_every_boundary():
    seq, off, lab = _nine()
    model = KC.callers_model(np.random.default_rng(3))
    kw = dict(min_len=60, min_margin=10, min_train=0, keep_scores=True)
    whole_m, _ = _dev(seq, off, lab, model, **kw)
    _same(whole_m, K.compose(seq, off, lab, model, 60, 10, 0), "model", scores=True)
    whole, _ = _dev(seq, off, lab, None, **kw)
    _same(whole, K.compose(seq, off, lab, None, 60, 10, 0), "own", scores=True)
    for b in range(1, 9):
        parts = [KC.cut(seq, off, lab, 0, b), KC.cut(seq, off, lab, b, 9)]
        # with a caller's model the per-contig rows concatenate to the whole
        g = [_dev(*p, model, **kw)[0] for p in parts]
        for name in ("classes", "counts", "scores"):
            assert np.concatenate([g[0][name], g[1][name]]).tobytes() == whole_m[name].tobytes(), (b, name)
        # without one the label rows and the background of the two calls add up to the whole's
        g = [_dev(*p, None, **kw)[0] for p in parts]
        acc = {}
        for x in g:
            for o, row in zip(x["row_labels"], x["rows"]):
                acc[int(o)] = acc.get(int(o), 0) + row
        assert sorted(acc) == whole["row_labels"].tolist(), b
        assert np.array_equal(np.stack([acc[o] for o in sorted(acc)]), whole["rows"]), b
        assert np.array_equal(g[0]["background"] + g[1]["background"], whole["background"]), b
        assert np.concatenate([g[0]["counts"], g[1]["counts"]]).tobytes() == whole["counts"].tobytes(), b


def test_a_callers_model():
    seq, off, lab = _want("edges")[0]
    rng = np.random.default_rng(4)
    for n_models in (3, KC.TILE + 3, 0):
        model = KC.callers_model(rng, n_models) if n_models else (np.zeros(0, np.int32), rng.integers(0, 9, size=(1, 256)))
        want = K.compose(seq, off, lab, model, 100, 0, 0)
        got, st = _dev(seq, off, lab, model, min_len=100, min_margin=0, min_train=1 << 40, keep_scores=True)   # (min_train is ignored)
        _same(got, want, n_models, scores=True)
        _stats_same(st, want)
        assert st["models"] == n_models and st["label_rows"] == 0 and got["background"].sum() == 0 and got["rows"].shape == (0, 256)
    labels, counts = KC.callers_model(rng, 3)
    assert int(counts[2].sum()) == 2 ** 62 - 1 and np.count_nonzero(counts[1]) == 1
    counts[2, 5] += 1                                       # a sum of 2^62
    e = _err(seq, off, lab, (labels, counts))
    assert e.code == N.KG_ERR_ARG and "model row 2" in str(e) and "2^62" in str(e)


# ---- errors, hygiene -------------------------------------------------------------------------------------------------------------

def _err(*a, **kw):
    from kmergutsjava_amd import hotpath
    with pytest.raises(N.KmerGutsNativeError) as ei:
        hotpath.compose_contigs(*a, **kw)
    return ei.value


def _raw(p, seq, off, n, lab=None, ml=None, mc=None, n_models=0):
    """The C call itself -> (return code, message); a set that comes back is freed."""
    lib = N.load()
    h = C.c_void_p()
    rc = lib.kg_contigs_compose(0, C.byref(p) if p is not None else None, seq, 0, off.ctypes.data if off is not None else None, n,
                                lab.ctypes.data if lab is not None else None, ml.ctypes.data if ml is not None else None,
                                mc.ctypes.data if mc is not None else None, n_models, C.byref(h))
    msg = lib.kg_last_error().decode()
    if rc == 0:
        lib.kg_compset_free(h)
    return rc, msg


def test_errors_name_the_first_offender():
    seq, off, lab = _nine()
    model = KC.callers_model(np.random.default_rng(3))
    for kw in ({"min_len": -1}, {"min_margin": -1}, {"min_train": -1}):
        assert _err(seq, off, lab, **kw).code == N.KG_ERR_ARG
    ok = N.KgCompParams(1500, 2560, 200000, 0, 0)
    assert _raw(N.KgCompParams(1500, 2560, 200000, 0, 1), seq.ctypes.data, off, 9)[0] == N.KG_ERR_ARG
    assert _raw(None, seq.ctypes.data, off, 9)[0] == N.KG_ERR_ARG
    assert _raw(ok, None, off, 9)[0] == N.KG_ERR_ARG and _raw(ok, seq.ctypes.data, None, 9)[0] == N.KG_ERR_ARG
    assert _raw(ok, seq.ctypes.data, off, -1)[0] == N.KG_ERR_ARG
    assert N.load().kg_contigs_compose(0, C.byref(ok), seq.ctypes.data, 0, off.ctypes.data, 9, None, None, None, 0, None) == N.KG_ERR_ARG
    bad = off.copy()
    bad[4] = bad[3] - 1
    e = _err(seq, bad, lab)
    assert e.code == N.KG_ERR_ARG and "contig 3" in str(e)
    # a label below -1 is refused on the host: it is never used as an index
    bad = lab.copy()
    bad[5], bad[7] = -2, -(2 ** 31)
    e = _err(seq, off, bad)
    assert e.code == N.KG_ERR_ARG and "contig 5" in str(e) and "-2" in str(e)
    e = _err(seq, off, bad, model)
    assert e.code == N.KG_ERR_ARG and "contig 5" in str(e)
    # a bad model
    labels, counts = model
    for change, word in ((lambda l, c: l.__setitem__(3, l[2]), "model row 3"), (lambda l, c: l.__setitem__(0, -1), "model row 0"),
                         (lambda l, c: c.__setitem__((4, 200), -1), "model row 4"), (lambda l, c: c.__setitem__((5, 0), -7), "background")):
        l, c = labels.copy(), counts.copy()
        change(l, c)
        e = _err(seq, off, lab, (l, c))
        assert e.code == N.KG_ERR_ARG and word in str(e), (word, e)
    rc, msg = _raw(ok, seq.ctypes.data, off, 9, lab, labels, None, 5)
    assert rc == N.KG_ERR_ARG and "model_counts" in msg
    rc, msg = _raw(ok, seq.ctypes.data, off, 9, lab, None, counts, 5)
    assert rc == N.KG_ERR_ARG and "model_labels" in msg
    assert _raw(ok, seq.ctypes.data, off, 9, lab, labels, counts, -1)[0] == N.KG_ERR_ARG
    # limits, all found on the host before a byte is read
    one = np.zeros(1, np.uint8)
    rc, msg = _raw(ok, one.ctypes.data, np.array([0, 5, 5 + 2 ** 30], np.int64), 2)
    assert rc == N.KG_ERR_LIMIT and "contig 1" in msg
    rc, msg = _raw(ok, one.ctypes.data, np.arange(1026, dtype=np.int64) * (2 ** 30 - 1), 1025)
    assert rc == N.KG_ERR_LIMIT and "2^40" in msg
    n = 2 ** 20 + 1
    rc, msg = _raw(ok, None, np.zeros(n + 1, np.int64), n, np.arange(n, dtype=np.int32))
    assert rc == N.KG_ERR_LIMIT and "2^20" in msg


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    seq, off, lab = _nine()
    model = KC.callers_model(np.random.default_rng(3))
    kw = dict(min_len=60, min_margin=10, min_train=0, keep_scores=True)
    want = {"own": K.compose(seq, off, lab, None, 60, 10, 0), "model": K.compose(seq, off, lab, model, 60, 10, 0)}
    _same(_dev(seq, off, lab, None, **kw)[0], want["own"])   # once first, so that what the runtime sets up on first use is not counted
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for which in ("own", "model"):
        failed = 0
        for n in range(1, 100):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got = _dev(seq, off, lab, model if which == "model" else None, **kw)[0]
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= (10 if which == "model" else 13), failed
        _same(got, want[which], which, scores=True)
        assert torch.cuda.mem_get_info()[0] == free0         # the set is freed: nothing of the call is left
    # a set the caller frees itself gives its arrays and its context back
    p = N.KgCompParams(60, 10, 0, 1, 0)
    h = C.c_void_p()
    lib = N.load()
    N.check(lib.kg_contigs_compose(0, C.byref(p), seq.ctypes.data, 0, off.ctypes.data, 9, lab.ctypes.data, None, None, 0, C.byref(h)))
    lib.kg_compset_free(h)
    assert torch.cuda.mem_get_info()[0] == free0


# ---- the planted sample through the front end ------------------------------------------------------------------------------------

def _planted(tmp_path):
    """The sample of compose_cases.planted_sample with its table: every 8-mer of a protein is a signature of its OTU with the
    protein's index as function, as in tests/test_gpu_otu_votes.py."""
    from kmergutsjava_amd import hotpath, synth
    from kmergutsjava_amd.make_table import default_num_sigs
    codes, contigs, kinds, genomes = KC.planted_sample()
    sigs = []
    for p, c in enumerate(codes):
        km = synth.encode_windows_aa(torch.from_numpy(c)).numpy()
        s = np.zeros(len(km), dtype=N.SIGNATURE_DTYPE)
        s["kmer"], s["otuIndex"], s["functionIndex"], s["functionWt"] = km, p // KC.PER_OTU, p, 1.0
        sigs.append(s)
    sigs = np.concatenate(sigs)
    sigs = sigs[np.unique(sigs["kmer"], return_index=True)[1]]
    d = tmp_path / "d"
    d.mkdir()
    with hotpath.SignatureTable.build(sigs, default_num_sigs(len(sigs))) as tab:
        tab.save(str(d / "kmer.table.mem_map"))
    onames = [b"genome A", b"genome B"]
    (d / "otu.index").write_bytes(b"".join(b"%d\t%s\n" % (i, o) for i, o in enumerate(onames)))
    ids = [b"contig_%d" % i for i in range(len(contigs))]
    (tmp_path / "c.fna").write_bytes(b"".join(b">%s\n%s\n" % (i, c) for i, c in zip(ids, contigs)))
    (tmp_path / "truth.tsv").write_bytes(b"".join(b"%s\t%s\n" % (i, onames[g]) for i, g in zip(ids, genomes) if g >= 0))
    return str(d), str(tmp_path / "c.fna"), ids, contigs, kinds, genomes, onames


def test_planted_sample_through_the_front_end(tmp_path):
    from helpers import batch_caps
    from kmergutsjava_amd import classify_contigs as CC
    from kmergutsjava_amd.kmer_guts_java import KmerGutsJava
    d, q, ids, contigs, kinds, genomes, onames = _planted(tmp_path)
    lens = [len(c) for c in contigs]

    def run(tag, **kw):
        out = {k: str(tmp_path / ("%s_%s" % (tag, k))) for k in ("o", "b", "s")}
        line = CC.classify_contigs(d, q, out["o"], write_all=True, bins_out=out["b"], split_dir=out["s"], truth=str(tmp_path / "truth.tsv"),
                                   compose=True, **kw)
        files = {k: open(out[k], "rb").read() for k in ("o", "b")}
        files.update({"s/" + f: open(os.path.join(out["s"], f), "rb").read() for f in sorted(os.listdir(out["s"]))})
        return line, files

    model_file = str(tmp_path / "model.txt")
    line, files = run("base", save_comp_model=model_file)
    rows = [ln.split(b"\t") for ln in files["o"].splitlines()]
    assert [r[0] for r in rows] == ids and [int(r[1]) for r in rows] == lens and all(len(r) == 14 for r in rows)
    composed = {0: [], 1: []}
    for n, (r, kind, g) in enumerate(zip(rows, kinds, genomes)):
        if kind == "voted":             # assigned as before, and the composition agrees
            assert r[2] == b"assigned" and r[3] == onames[g] and r[11] == onames[g], r
        elif kind == "unvoted":         # composed into its genome's bin
            assert r[2] == b"composed" and r[3] == onames[g] and r[11] == onames[g] and int(r[12]) >= 2560, r
            composed[g].append(n)
        elif kind == "short":           # below min_len: not composed
            assert r[2] == b"none" and r[3] == b"-" and int(r[1]) == 1000, r
        else:                           # the background is best
            assert r[2] == b"none" and r[3] == b"-" and r[11] == b"-", r
        assert int(r[13]) == 2 * (lens[n] - 3)
    voted = {g: [n for n, (k, x) in enumerate(zip(kinds, genomes)) if k == "voted" and x == g] for g in (0, 1)}
    assert all(len(voted[g]) == KC.N_VOTED and len(composed[g]) == KC.N_UNVOTED for g in (0, 1))
    bins = {ln.split(b"\t")[0]: [int(x) for x in ln.split(b"\t")[1:]] for ln in files["b"].splitlines()}
    assert sorted(bins) == onames
    for g in (0, 1):
        b = bins[onames[g]]
        assert (b[0], b[1], b[4], b[5]) == (KC.N_VOTED, sum(lens[n] for n in voted[g]), KC.N_UNVOTED, sum(lens[n] for n in composed[g]))
    n_comp, len_comp = 2 * KC.N_UNVOTED, sum(lens[n] for g in (0, 1) for n in composed[g])
    len_asg = sum(lens[n] for g in (0, 1) for n in voted[g])
    assert line == ("Sequences: %d, with votes: %d, assigned: %d, bins: 2, assigned length: %d of %d, votes: %d, "
                    "labelled: %d, agree: %d, disagree: 0, missed: %d, composed: %d, composed length: %d, conflicts: 0, models: 2, "
                    "composed agree: %d, composed disagree: 0"
                    % (len(ids), sum(1 for r in rows if int(r[8]) > 0), 2 * KC.N_VOTED, len_asg, sum(lens), sum(int(r[5]) for r in rows),
                       len(ids) - KC.N_FOREIGN, 2 * KC.N_VOTED, len(ids) - KC.N_FOREIGN - 2 * KC.N_VOTED, n_comp, len_comp, n_comp))
    assert sorted(f for f in files if f.startswith("s/")) == ["s/otu_0.fna", "s/otu_1.fna", "s/unassigned.fna"]
    for g in (0, 1):
        assert files["s/otu_%d.fna" % g] == b"".join(b">%s\n%s\n" % (ids[n], contigs[n]) for n in sorted(voted[g] + composed[g]))
    assert files["s/unassigned.fna"] == b"".join(b">%s\n%s\n" % (i, c) for i, c, k in zip(ids, contigs, kinds) if k in ("short", "foreign"))
    # the model file holds the two genomes' rows; scoring from it gives the same bytes
    labels, counts = CC.parse_comp_model(open(model_file, "rb").read(), model_file, onames)
    assert labels.tolist() == [0, 1] and (counts[:2].sum(axis=1) >= 200000).all()
    assert int(counts[2].sum()) == sum(2 * (n - 3) for n in lens)
    assert run("file", comp_model=model_file) == (line, files)
    # without the flag the voted lines are the same without the trailing fields
    plain = str(tmp_path / "plain.tsv")
    CC.classify_contigs(d, q, plain, write_all=True)
    for a, b in zip(open(plain, "rb").read().splitlines(), files["o"].splitlines()):
        if b.split(b"\t")[2] != b"composed":
            assert a == b.rsplit(b"\t", 3)[0]
    # byte-identical under every batch cap
    keep = KmerGutsJava.MAX_BATCH_CHARS
    try:
        for what, cap in sorted(batch_caps(lens).items()):
            KmerGutsJava.MAX_BATCH_CHARS = cap
            assert run(what) == (line, files), (what, cap)
    finally:
        KmerGutsJava.MAX_BATCH_CHARS = keep
