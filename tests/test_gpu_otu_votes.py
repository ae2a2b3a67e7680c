"""OTU votes on the GPU (kg_result_otu_votes / kg_otu_votes_hits): the four device arrays must equal the numpy model of
tests/otu_votes_model.py byte for byte -- on random caller-held lists around the lane, wave, scan-chunk and sort-tile edges,
cut into two calls at every sequence boundary, on scans under every strategy (where the votes per CALL are the CALL counts and,
with five OTUs, the pairs are the reference's buffer), at the list cap, and through the classify_contigs front end on a
planted sample; errors name the first offender and failed allocations leave nothing behind."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import otu_votes_cases as VC  # noqa: E402
import otu_votes_model as V  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

EDGES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097]


def _dev(args, dst="host", **kw):
    from kmergutsjava_amd import hotpath
    st = {}
    got = hotpath.otu_votes(*args, device_out=(dst == "device"), stats=st, **kw)
    if dst == "device":
        v, start, c, b = got
        got = (v.cpu().numpy().view(N.VOTE_DTYPE), start, c.cpu().numpy().view(N.OTU_CLASS_DTYPE), b.cpu().numpy().view(N.OTU_BIN_DTYPE))
    return got, st


def _same(got, want, what=""):
    for name, g, w in zip(("votes", "vote_start", "classes", "bins"), got, want):
        assert len(g) == len(w), (what, name, len(g), len(w))
        assert g.tobytes() == w.tobytes(), (what, name, [(i, g[i], w[i]) for i in range(len(g)) if g[i] != w[i]][:3])


def _case(name):
    rng = np.random.default_rng(sum(name.encode()))
    cyc = lambda n: [EDGES[i % len(EDGES)] for i in range(n)]        # noqa: E731
    if name == "one_seq_one_otu":
        return VC.random_lists(rng, 1, 1, 4097, (1, 2), 1)
    if name == "two_seqs":
        return VC.random_lists(rng, 2, 6, [0, 65], (0, 1, 2), 5)
    if name == "edges_dna":
        return VC.random_lists(rng, 70, 6, cyc(70), (0, 1, 2), 6)
    if name == "edges_aa_300_calls":
        return VC.random_lists(rng, 70, 1, cyc(70), (1, 300), 5)
    if name == "seventy_thousand":
        return VC.many_short(rng, 70_000)
    if name == "five_thousand_otus":                # one sequence holds every vote, between sequences that have none
        return VC.random_lists(rng, 3, 6, [0, 20_000, 0], (1, 2), 5000, max_oi=99_999)
    if name == "widest_key":
        return VC.random_lists(rng, 5, 1, 300, (1, 2), 6, max_oi=2 ** 31 - 1)
    raise KeyError(name)


CASES = ["one_seq_one_otu", "two_seqs", "edges_dna", "edges_aa_300_calls", "seventy_thousand", "five_thousand_otus", "widest_key"]
_WANT = {}


def _want(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _WANT:
        args = _case(name)
        _WANT[key] = (args, V.otu_votes(*args, **kw))
    return _WANT[key]


@pytest.mark.parametrize("dst", ["host", "device"])
@pytest.mark.parametrize("name", CASES)
def test_random_lists_equal_the_model(name, dst):
    kw = dict(min_votes=2, min_share_pct=30, min_calls=1)
    args, want = _want(name, **kw)
    got, st = _dev(args, dst, **kw)
    _same(got, want, name)
    votes, start, cls, bins = want
    assert st["hits"] == len(args[0]) and st["votes"] == int(cls["total"].sum()) and st["pairs"] == len(votes)
    assert st["accepted"] == int((args[2] & N.EV_ACCEPTED != 0).sum())
    assert st["seqs_with_votes"] == int((cls["n_otus"] > 0).sum()) and st["assigned"] == int(cls["assigned"].sum())
    assert st["bins"] == len(bins) and st["total_length"] == int(args[7][-1])
    assert st["assigned_length"] == int(np.diff(args[7])[cls["assigned"] != 0].sum()) == int(bins["length"].sum())
    if name == "widest_key":
        assert votes["oI"].min() == 0 and votes["oI"].max() == 2 ** 31 - 1
    if name == "five_thousand_otus":
        assert cls["n_otus"].tolist() == [0, 5000, 0]
    if name == "edges_dna":
        assert cls["total"].tolist()[:len(EDGES)] == EDGES and st["ms"] > 0


def test_default_parameters_and_the_binding():
    args, want = _want("edges_dna")
    _same(_dev(args)[0], want)


def test_launch_independence_two_calls_at_every_boundary():
    rng = np.random.default_rng(99)
    args = VC.random_lists(rng, 9, 6, [300, 0, 65, 4097, 1, 64, 2048, 0, 257], (0, 1, 2), 6)
    kw = dict(min_votes=1, min_share_pct=20, min_calls=1)
    whole, _ = _dev(args, **kw)
    _same(whole, V.otu_votes(*args, **kw))
    for b in range(1, 9):
        (v0, s0, c0, b0), _ = _dev(VC.cut(args, 0, b), **kw)
        (v1, s1, c1, b1), _ = _dev(VC.cut(args, b, 9), **kw)
        v1 = v1.copy()
        v1["seq"] += b
        assert np.concatenate([v0, v1]).tobytes() == whole[0].tobytes(), b
        assert np.concatenate([s0, s0[-1] + s1[1:]]).tobytes() == whole[1].tobytes(), b
        assert np.concatenate([c0, c1]).tobytes() == whole[2].tobytes(), b
        assert V.merge_bins([b0, b1]).tobytes() == whole[3].tobytes(), b


# ---- scans ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(params=["direct", "partitioned", "partitioned_tags"])
def strategy(request, monkeypatch):
    """The scan strategies of the parity tests (tests/test_gpu_parity.py)."""
    monkeypatch.setenv("KG_PARTITION", "0" if request.param == "direct" else "1")
    monkeypatch.setenv("KG_DIRECT_FILTER", "2")
    if request.param == "partitioned_tags":
        monkeypatch.setenv("KG_BIDX", "0")
    return request.param


SCAN_INPUTS = dict(VC.ORACLE_INPUTS, big=VC.BIG_DNA)


def _scan_input(name, modulo=None):
    from kmergutsjava_amd import synth
    a, kw, run = SCAN_INPUTS[name]
    seq, off, rec, _ = synth.high_density_config(*a, **kw)
    if modulo:
        rec[:, 2] %= modulo
    return synth.table_image(rec), seq.numpy(), np.asarray(off, dtype=np.int64), run


def _own_records(r):
    return {"hits": r.hits(), "container_hit_start": r.container_hit_start(), "hit_events": r.hit_events(), "calls": r.calls(),
            "container_call_start": r.container_call_start()}


@pytest.mark.parametrize("name", sorted(SCAN_INPUTS))
def test_scans_equal_the_model_on_their_own_records(strategy, name):
    from kmergutsjava_amd import hotpath
    img, sb, off, run = _scan_input(name)
    per = 1 if run.get("aa") else 6
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        live0 = tab.live_device_bytes()
        with tab.scan(sb, off, hotpath.Params(**run)) as r:
            live1 = tab.live_device_bytes()
            rec = _own_records(r)
            for kw in (dict(), dict(min_votes=3, min_share_pct=20, min_calls=2)):
                want = VC.model_on(rec, per, off, **kw)
                _same(r.otu_votes(off, **kw), want, name)
                assert r.vote_stats["votes"] == int(want[2]["total"].sum()) and r.vote_stats["ms"] > 0
                assert tab.live_device_bytes() == live1
            d = r.otu_votes(off, device_out=True)
            got = (d[0].cpu().numpy().view(N.VOTE_DTYPE), d[1], d[2].cpu().numpy().view(N.OTU_CLASS_DTYPE), d[3].cpu().numpy().view(N.OTU_BIN_DTYPE))
            _same(got, VC.model_on(rec, per, off))
            # the votes of every CALL are its count
            k = V.vote_calls(rec["hits"], rec["container_hit_start"], rec["hit_events"], rec["calls"], rec["container_call_start"])
            assert np.array_equal(np.bincount(k[k >= 0], minlength=len(rec["calls"])), rec["calls"]["count"])
            assert r.vote_stats["votes"] == int(rec["calls"]["count"].sum()) > 0
            if name in VC.RECORDED:
                assert (len(rec["calls"]), r.vote_stats["votes"]) == VC.RECORDED[name][:2]
            else:
                assert 25_000 < r.stats["n_hits"] < 40_000, r.stats["n_hits"]
        assert tab.live_device_bytes() == live0
    # five OTUs: the device kg_otu buffer is the pairs
    img, sb, off, run = _scan_input(name, 5)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(sb, off, hotpath.Params(**run)) as r:
        votes, start, cls, bins = r.otu_votes(off)
        assert (cls["n_otus"] > 0).sum() > 0 and cls["n_otus"].max() == 5
        assert VC.buffer_equals_pairs(r.otu(), votes, start)


def test_the_list_cap():
    """One protein with 40 010 hits of one function and one OTU at consecutive positions: the list takes
    KG_MAX_HITS_PER_SEQ - 2 of them (KGJ:495), the others are not accepted and do not vote."""
    from kmergutsjava_amd import hotpath
    n = 40_010
    hits = np.zeros(n, dtype=N.HIT_DTYPE)
    hits["from0InProt"] = np.arange(n)
    hits["oI"], hits["fI"], hits["functionWt"] = 3, 7, 1.0
    chs = np.array([0, n], np.int64)
    off = np.array([0, n + 7], np.int64)
    with hotpath.aggregate_hits(hits, chs, 1, hotpath.Params(aa=True)) as r:
        ev, calls, otu = r.hit_events(), r.calls(), r.otu()
        votes, start, cls, bins = r.otu_votes(off)
        _same((votes, start, cls, bins), V.otu_votes(hits, chs, ev, calls, r.container_call_start(), 1, 1, off))
    unaccepted = int((ev & N.EV_ACCEPTED == 0).sum())
    assert unaccepted == n - (40_000 - 2) and len(calls) == 1
    assert len(votes) == 1 and votes["votes"][0] == calls["count"][0] == otu["count"][0][0] == n - unaccepted
    assert tuple(cls[0]) == (3, 1, n - unaccepted, n - unaccepted, 1, 1, 1, -1, 0, 0)
    assert [tuple(int(x) for x in b) for b in bins] == [(3, 1, n + 7, n - unaccepted, 1)]


# ---- the planted sample through the front end ------------------------------------------------------------------------------

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _planted(tmp_path):
    """Seven OTUs of 40 random proteins; every 8-mer of a protein is a signature of its OTU with the protein's index as
    function.  A fifth of each OTU's proteins also occur in the next OTU's genome, labelled with the first.  Two contigs per
    OTU of twelve of its genome's proteins, back-translated, between random spacers, every other contig reverse-complemented;
    one more contig is half OTU 2 and half OTU 5."""
    from kmergutsjava_amd import hotpath, synth
    from kmergutsjava_amd.make_table import default_num_sigs
    rng = np.random.default_rng(2024)
    alpha = np.frombuffer(synth.PROT_ALPHA.encode(), dtype=np.uint8)
    n_otu, per_otu = 7, 40
    codes = [rng.integers(0, 20, size=int(rng.integers(90, 130))) for _ in range(n_otu * per_otu)]
    sigs = []
    for p, c in enumerate(codes):
        km = synth.encode_windows_aa(torch.from_numpy(c)).numpy()
        s = np.zeros(len(km), dtype=N.SIGNATURE_DTYPE)
        s["kmer"], s["otuIndex"], s["functionIndex"], s["functionWt"] = km, p // per_otu, p, 1.0
        sigs.append(s)
    sigs = np.concatenate(sigs)
    sigs = sigs[np.unique(sigs["kmer"], return_index=True)[1]]
    d = tmp_path / "d"
    d.mkdir()
    with hotpath.SignatureTable.build(sigs, default_num_sigs(len(sigs))) as tab:
        assert tab.placed >= len(sigs) - 16          # (a k-mer whose home is the table's last slots can be pushed past the end)
        tab.save(str(d / "kmer.table.mem_map"))
    onames = [b"genome %c" % (65 + o) for o in range(n_otu)]
    (d / "otu.index").write_bytes(b"".join(b"%d\t%s\n" % (i, o) for i, o in enumerate(onames)))
    # a genome: its own proteins and the first fifth of the previous OTU's
    genome = [list(range(o * per_otu, (o + 1) * per_otu)) + (list(range((o - 1) * per_otu, (o - 1) * per_otu + per_otu // 5)) if o else [])
              for o in range(n_otu)]

    def stretch(prots):
        parts = []
        for p in prots:
            parts.append(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(30, 200)))))
            parts.append(synth.back_translate(alpha[codes[p]].tobytes().decode()).encode())
        return b"".join(parts)

    contigs, truth = [], []
    for o in range(n_otu):
        for k in range(2):
            contigs.append(stretch(rng.choice(genome[o], size=12, replace=False)))
            truth.append(o)
    contigs.append(stretch(rng.choice(genome[2][:per_otu], size=6, replace=False)) + stretch(rng.choice(genome[5][:per_otu], size=6, replace=False)))
    truth.append(-1)
    contigs = [c.translate(_COMP)[::-1] if i % 2 else c for i, c in enumerate(contigs)]
    ids = [b"contig_%d" % i for i in range(len(contigs))]
    (tmp_path / "c.fna").write_bytes(b"".join(b">%s\n%s\n" % (i, c) for i, c in zip(ids, contigs)))
    (tmp_path / "truth.tsv").write_bytes(b"".join(b"%s\t%s\n" % (i, onames[t]) for i, t in zip(ids, truth) if t >= 0))
    return str(d), str(tmp_path / "c.fna"), ids, contigs, truth, onames


def test_planted_sample_through_the_front_end(tmp_path):
    from helpers import batch_caps
    from kmergutsjava_amd import classify_contigs as CC
    from kmergutsjava_amd.kmer_guts_java import KmerGutsJava
    d, q, ids, contigs, truth, onames = _planted(tmp_path)
    lens = [len(c) for c in contigs]

    def run(tag, **kw):
        out = {k: str(tmp_path / ("%s_%s" % (tag, k))) for k in ("o", "v", "b", "s")}
        line = CC.classify_contigs(d, q, out["o"], write_all=True, votes_out=out["v"], bins_out=out["b"], split_dir=out["s"],
                                   truth=str(tmp_path / "truth.tsv"), **kw)
        files = {k: open(out[k], "rb").read() for k in ("o", "v", "b")}
        files.update({"s/" + f: open(os.path.join(out["s"], f), "rb").read() for f in sorted(os.listdir(out["s"]))})
        return line, files

    line, files = run("base", min_share=67)
    rows = [ln.split(b"\t") for ln in files["o"].splitlines()]
    assert [r[0] for r in rows] == ids and [int(r[1]) for r in rows] == lens
    for r, t in zip(rows[:-1], truth[:-1]):                    # every pure contig is assigned to its OTU
        assert r[2] == b"assigned" and r[3] == onames[t], r
    chim = rows[-1]
    assert chim[2] == b"below" and {chim[3], chim[9]} == {onames[2], onames[5]}, chim
    bins = [ln.split(b"\t") for ln in files["b"].splitlines()]
    assert len(bins) == 7 and sorted(b[0] for b in bins) == sorted(onames)
    assert sum(int(b[2]) for b in bins) == sum(lens[:-1]) and all(int(b[1]) == 2 for b in bins)
    assert line == ("Sequences: 15, with votes: 15, assigned: 14, bins: 7, assigned length: %d of %d, votes: %d, "
                    "labelled: 14, agree: 14, disagree: 0, missed: 0" % (sum(lens[:-1]), sum(lens), sum(int(r[5]) for r in rows)))
    # the split files hold exactly the assigned contigs
    assert sorted(f for f in files if f.startswith("s/")) == sorted(["s/otu_%d.fna" % o for o in range(7)] + ["s/unassigned.fna"])
    for o in range(7):
        assert files["s/otu_%d.fna" % o] == b"".join(b">%s\n%s\n" % (i, c) for i, c, t in zip(ids, contigs, truth) if t == o)
    assert files["s/unassigned.fna"] == b">%s\n%s\n" % (ids[-1], contigs[-1])
    # at the default share the chimera goes to the half with more votes, or stays below on a tie: still no pure contig moves
    assert run("half")[1]["o"].splitlines()[:-1] == files["o"].splitlines()[:-1]
    # byte-identical under every batch cap
    keep = KmerGutsJava.MAX_BATCH_CHARS
    try:
        for what, cap in sorted(batch_caps(lens).items()):
            KmerGutsJava.MAX_BATCH_CHARS = cap
            assert run(what, min_share=67) == (line, files), (what, cap)
    finally:
        KmerGutsJava.MAX_BATCH_CHARS = keep


# ---- errors, empty inputs, hygiene -------------------------------------------------------------------------------------------

def _err(args, **kw):
    from kmergutsjava_amd import hotpath
    with pytest.raises(N.KmerGutsNativeError) as ei:
        hotpath.otu_votes(*args, **kw)
    return ei.value


def _small():
    b = VC.Lists(3, 1, [100, 200, 300])
    b.call(0, 5, 4, 1).call(1, 5, 6, 2).call(1, 20, 3, 2).call(2, 9, 5, 0)
    return b.build()


def test_errors_name_the_first_offender():
    from kmergutsjava_amd import hotpath
    args = _small()
    hits, chs, ev, calls, ccs, n, per, off = args
    _same(_dev(args)[0], V.otu_votes(*args))
    bad = chs.copy()
    bad[1], bad[2] = bad[2], bad[1]                             # [0, 13, 4, 18]
    e = _err((hits, bad, ev, calls, ccs, n, per, off))
    assert e.code == N.KG_ERR_ARG and "container 1" in str(e) and "container_hit_start" in str(e)
    bad = ccs.copy()
    bad[1], bad[2] = 3, 1
    e = _err((hits, chs, ev, calls, bad, n, per, off))
    assert e.code == N.KG_ERR_ARG and "container 1" in str(e) and "container_call_start" in str(e)
    bad = calls.copy()
    bad["start"][2] = bad["start"][1]                           # the second CALL of container 1 does not ascend
    e = _err((hits, chs, ev, bad, ccs, n, per, off))
    assert e.code == N.KG_ERR_ARG and "CALL 2" in str(e)
    bad = hits.copy()
    bad["oI"][6] = -5
    e = _err((bad, chs, ev, calls, ccs, n, per, off))
    assert e.code == N.KG_ERR_ARG and "hit 6" in str(e)
    # ... which is legal on a hit that does not vote
    quiet = ev.copy()
    quiet[6] = 0
    _same(_dev((bad, chs, quiet, calls, ccs, n, per, off))[0], V.otu_votes(bad, chs, quiet, calls, ccs, n, per, off))
    bad = hits.copy()
    bad["from0InProt"][5] = 2                                   # below its predecessor's in container 1
    e = _err((bad, chs, ev, calls, ccs, n, per, off))
    assert e.code == N.KG_ERR_ARG and "hit 5" in str(e)
    bad = hits.copy()
    bad["container"][4] = 0                                     # lies in container 1's slice
    e = _err((bad, chs, ev, calls, ccs, n, per, off))
    assert e.code == N.KG_ERR_ARG and "hit 4" in str(e)
    for kw in ({"min_votes": -1}, {"min_share_pct": -1}, {"min_share_pct": 101}, {"min_calls": -1}):
        assert _err(args, **kw).code == N.KG_ERR_ARG
    e = _err((hits[:0], np.zeros(10, np.int64), ev[:0], calls[:0], np.zeros(10, np.int64), 3, 3, off))
    assert e.code == N.KG_ERR_ARG and "per" in str(e)
    bad = off.copy()
    bad[2] = 50
    e = _err((hits, chs, ev, calls, ccs, n, per, bad))
    assert e.code == N.KG_ERR_ARG and "sequence 1" in str(e)
    p = N.KgVoteParams(10, 50, 1, 0)
    h = C.c_void_p()
    assert N.load().kg_otu_votes_hits(0, C.byref(p), None, None, None, None, None, 0, 1, off.ctypes.data, C.byref(h)) == N.KG_ERR_ARG


def test_a_skip_aggregate_result_is_refused():
    from kmergutsjava_amd import hotpath
    img, sb, off, run = _scan_input("aa")
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        with tab.scan(sb, off, hotpath.Params(aa=True, skip_aggregate=True)) as r:
            with pytest.raises(N.KmerGutsNativeError) as ei:
                r.otu_votes(off)
            assert ei.value.code == N.KG_ERR_ARG and "KG_F_SKIP_AGGREGATE" in str(ei.value)
        assert tab.live_device_bytes() == 0


@pytest.mark.parametrize("per", [1, 6])
def test_empty_inputs_return_empty_sets(per):
    none = (np.zeros(0, N.HIT_DTYPE), np.zeros(1, np.int64), np.zeros(0, np.uint8), np.zeros(0, N.CALL_DTYPE), np.zeros(1, np.int64), 0, per,
            np.zeros(1, np.int64))
    (votes, start, cls, bins), st = _dev(none)
    assert len(votes) == len(cls) == len(bins) == 0 and start.tolist() == [0] and st["hits"] == 0
    # sequences, but no hit; hits, but no CALL
    off = np.array([0, 10, 30, 60], np.int64)
    quiet = (none[0], np.zeros(3 * per + 1, np.int64), none[2], none[3], np.zeros(3 * per + 1, np.int64), 3, per, off)
    _same(_dev(quiet)[0], V.otu_votes(*quiet))
    hits = np.zeros(5, N.HIT_DTYPE)
    hits["container"], hits["from0InProt"] = per, np.arange(5)
    chs = np.zeros(3 * per + 1, np.int64)
    chs[per + 1:] = 5
    no_calls = (hits, chs, np.full(5, N.EV_ACCEPTED, np.uint8), none[3], quiet[4], 3, per, off)
    got, st = _dev(no_calls)
    _same(got, V.otu_votes(*no_calls))
    assert st["accepted"] == 5 and st["votes"] == 0 and (got[2]["otu"] == -1).all()


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    from kmergutsjava_amd import hotpath
    args, want = _want("edges_dna")
    img, sb, off, run = _scan_input("dna")
    with hotpath.SignatureTable.from_bytes(img, 0) as tab, tab.scan(sb, off, hotpath.Params(**run)) as r:
        want_r = r.otu_votes(off, min_votes=3, min_share_pct=20)
        assert len(want_r[3]) > 0
        _same(_dev(args)[0], want)              # once first, so that what the runtime sets up on first use is not counted
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        live0 = tab.live_device_bytes()
        for which in ("lists", "result"):
            failed = 0
            for n in range(1, 400):
                monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
                try:
                    got = _dev(args)[0] if which == "lists" else r.otu_votes(off, min_votes=3, min_share_pct=20)
                    break
                except N.KmerGutsNativeError as e:
                    assert e.code == N.KG_ERR_NOMEM, e
                    failed += 1
                    assert tab.live_device_bytes() == live0
                    if which == "lists":
                        assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
            monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
            assert failed >= 30, failed
            _same(got, want if which == "lists" else want_r)
            assert tab.live_device_bytes() == live0     # the set is freed: the table's live bytes are the result's own again
        # an open set holds blocks of the result's table until it is freed
        p = N.KgVoteParams(10, 50, 1, 0)
        h = C.c_void_p()
        lib = N.load()
        N.check(lib.kg_result_otu_votes(r._h, C.byref(p), off.ctypes.data, C.byref(h)))
        assert tab.live_device_bytes() > live0
        lib.kg_voteset_free(h)
        assert tab.live_device_bytes() == live0
