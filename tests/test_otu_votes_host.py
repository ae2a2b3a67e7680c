"""OTU votes without a GPU: known answers of the rule worked out by hand against the numpy model of tests/otu_votes_model.py,
the model against the CPU oracle (its votes per CALL are the CALL's count; with at most five OTUs in the table its pairs are
the reference's OTU-COUNTS buffer), how often the five-slot buffer misses the winner, the structures against the C layout, and
the classify_contigs front end on model output with the scan replaced."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import otu_votes_cases as VC  # noqa: E402
import otu_votes_model as V  # noqa: E402
from otu_votes_cases import BIG_DNA, ORACLE_INPUTS, RECORDED, buffer_equals_pairs, model_on, oracle_input  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

ROOT = os.path.dirname(HERE)


def _votes(v):
    return [tuple(int(x) for x in r) for r in v]


def test_known_answers_of_rule_1():
    """One protein (per = 1), one CALL of function 3 from 10 to 40.  The hits at 10 (OTU 1) and at 33 = end - 7 (OTU 2) vote; the
    hit at 5 lies before the first CALL, the one at 12 is of function 9, the one at 20 was not accepted, the one at 34 = end - 6
    reaches past the CALL's end."""
    b = VC.Lists(1, 1, [77])
    b.c.append((0, 10, 40, 2, 3, 2.0))
    b.hit(0, 5, 1, 3).hit(0, 10, 1, 3).hit(0, 12, 1, 9).hit(0, 20, 1, 3, ev=N.EV_RESET_BEFORE).hit(0, 33, 2, 3).hit(0, 34, 2, 3)
    args = b.build()
    assert V.vote_calls(*args[:5]).tolist() == [-1, 0, -1, -1, 0, -1]
    votes, start, cls, bins = V.otu_votes(*args)
    # a tie in the order: OTU 1 before OTU 2
    assert _votes(votes) == [(0, 1, 1, 1), (0, 2, 1, 1)] and start.tolist() == [0, 2]
    assert tuple(cls[0]) == (1, 0, 1, 2, 1, 1, 2, 2, 1, 0) and len(bins) == 0
    # 100 * 1 == 50 * 2: on the edge of min_share_pct, and votes == min_votes, n_calls == min_calls
    votes, start, cls, bins = V.otu_votes(*args, min_votes=1, min_share_pct=50, min_calls=1)
    assert cls["assigned"][0] == 1 and _votes(bins) == [(1, 1, 77, 1, 1)]
    for kw in ({"min_share_pct": 51}, {"min_votes": 2}, {"min_calls": 2}):
        p = dict(min_votes=1, min_share_pct=50, min_calls=1)
        p.update(kw)
        assert V.otu_votes(*args, **p)[2]["assigned"][0] == 0, kw


def test_known_answer_kept_two_carry():
    """The list of function 1 printed a CALL 0 .. 27 (its last member of function 1 at 20); its last two members, of function
    2 at 24 and 26, open the next list, whose CALL runs 24 .. 60.  The extents overlap by 4 residues.  The hits at 24 and 26
    vote in the second CALL (the largest start <= 24), and a hit of function 1 at 25 votes nowhere."""
    b = VC.Lists(1, 1)
    b.call(0, 0, 21, 4, fI=1)
    b.call(0, 24, 1, 4, fI=2, end=60).hit(0, 26, 4, 2).hit(0, 53, 6, 2).hit(0, 25, 4, 1).hit(0, 54, 6, 2)
    args = b.build()
    assert args[3]["end"].tolist() == [27, 60]
    k = V.vote_calls(*args[:5])
    pos = args[0]["from0InProt"]
    assert k[pos == 24][0] == 1 and k[pos == 26][0] == 1 and k[pos == 25][0] == -1 and k[pos == 53][0] == 1 and k[pos == 54][0] == -1
    votes, start, cls, bins = V.otu_votes(*args)
    assert _votes(votes) == [(0, 4, 23, 2), (0, 6, 1, 1)]
    assert tuple(cls[0]) == (4, 1, 23, 24, 2, 2, 2, 6, 1, 0)


def test_known_answers_order_classes_and_bins():
    """Four contigs (per = 6) and one without votes.  Contig 0: OTU 9 has 12 votes from containers 0, 3 and 5 (three CALLs), OTU 2
    and OTU 5 have 6 each -> order 9, 2, 5; 100 * 12 = 50 * 24, assigned on the edge.  Contig 1: 10 votes for OTU 2, one CALL.
    Contig 3: 10 votes for OTU 9 -> the bins of OTU 2 and OTU 9 ... contig 4: 12 votes for OTU 7 with length and votes equal to
    OTU 9's bin after the contigs' lengths are chosen so."""
    b = VC.Lists(5, 6, [300, 400, 50, 100, 400])
    b.call(0, 2, 4, 9).call(3, 7, 4, 9).call(5, 1, 4, [9, 9, 9, 9])
    b.call(1, 0, 6, 2).call(4, 9, 6, 5)
    b.call(7, 3, 10, 2)
    b.call(18, 0, 10, 9)
    b.call(24, 0, 11, 7).call(29, 0, 11, 7)
    args = b.build()
    votes, start, cls, bins = V.otu_votes(*args)
    assert start.tolist() == [0, 3, 4, 4, 5, 6]
    assert _votes(votes) == [(0, 9, 12, 3), (0, 2, 6, 1), (0, 5, 6, 1), (1, 2, 10, 1), (3, 9, 10, 1), (4, 7, 22, 2)]
    assert tuple(cls[0]) == (9, 1, 12, 24, 3, 5, 3, 2, 6, 0)
    assert tuple(cls[2]) == (-1, 0, 0, 0, 0, 0, 0, -1, 0, 0)                 # a sequence without votes
    assert cls["assigned"].tolist() == [1, 1, 0, 1, 1]
    # OTU 9: contigs 0 and 3, length 400, votes 22; OTU 7: contig 4, length 400, votes 22 -> tie down to oI; OTU 2: length 400, 10
    assert _votes(bins) == [(7, 1, 400, 22, 2), (9, 2, 400, 22, 4), (2, 1, 400, 10, 1)]
    # one vote fewer than 50 %: 100 * 12 < 51 * 24
    assert V.otu_votes(*args, min_share_pct=51)[2]["assigned"].tolist() == [0, 1, 0, 1, 1]
    # n_calls on its edge: contig 0 has three CALLs for OTU 9
    assert V.otu_votes(*args, min_calls=3)[2]["assigned"].tolist() == [1, 0, 0, 0, 0]
    assert V.otu_votes(*args, min_votes=12)[2]["assigned"].tolist() == [1, 0, 0, 0, 1]
    assert V.otu_votes(*args, min_votes=13)[2]["assigned"].tolist() == [0, 0, 0, 0, 1]


def test_model_refuses_what_the_library_refuses():
    b = VC.Lists(1, 1)
    b.call(0, 5, 3, [1, -1, 1])
    with pytest.raises(ValueError, match="hit 1"):
        V.otu_votes(*b.build())
    b = VC.Lists(1, 1)
    b.call(0, 5, 3, 1).call(0, 5, 2, 1)
    with pytest.raises(ValueError, match="ascend"):
        V.otu_votes(*b.build())


def test_random_lists_have_the_votes_they_were_built_with():
    """The generator of the GPU tests: the model finds exactly the planted votes, whatever noise lies around them."""
    rng = np.random.default_rng(3)
    for per in (1, 6):
        want = rng.integers(0, 300, size=40)
        args = VC.random_lists(rng, 40, per, want, calls_per_container=(1, 2, 5), n_otus=6)
        votes, start, cls, bins = V.otu_votes(*args)
        assert cls["total"].tolist() == want.tolist()
        assert (V.vote_calls(*args[:5]) < 0).sum() > 40
        k = V.vote_calls(*args[:5])
        assert np.array_equal(np.bincount(k[k >= 0], minlength=len(args[3])), args[3]["count"])
        # cut at a sequence boundary: the same records, the bins add up
        a, b = V.otu_votes(*VC.cut(args, 0, 17)), V.otu_votes(*VC.cut(args, 17, 40))
        assert np.concatenate([a[2], b[2]]).tobytes() == cls.tobytes()
        assert V.merge_bins([a[3], b[3]]).tobytes() == bins.tobytes()


# ---- the model against the oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ORACLE_INPUTS))
def test_votes_per_call_are_the_call_counts(oracle, name):
    img, seq, off, run = oracle_input(name)
    ora = oracle.run(img, seq, off, lookup_mode=1, **run)
    k = V.vote_calls(ora["hits"], ora["container_hit_start"], ora["hit_events"], ora["calls"], ora["container_call_start"])
    per_call = np.bincount(k[k >= 0], minlength=len(ora["calls"]))
    print(name, "CALLs", len(ora["calls"]), "votes", int(per_call.sum()))
    assert (len(ora["calls"]), int(per_call.sum())) == RECORDED[name][:2]
    assert np.array_equal(per_call, ora["calls"]["count"])


@pytest.mark.parametrize("modulo", [4, 5])
@pytest.mark.parametrize("name", sorted(ORACLE_INPUTS))
def test_pairs_are_the_reference_buffer_with_at_most_five_otus(oracle, name, modulo):
    img, seq, off, run = oracle_input(name, modulo)
    ora = oracle.run(img, seq, off, lookup_mode=1, **run)
    votes, start, cls, bins = model_on(ora, 1 if run.get("aa") else 6, off)
    with_votes, all_five = int((cls["n_otus"] > 0).sum()), int((cls["n_otus"] == 5).sum())
    print(name, modulo, "sequences with votes", with_votes, "with five OTUs", all_five)
    assert with_votes == RECORDED[name][2]
    if modulo == 5:
        assert all_five == RECORDED[name][3]
    assert buffer_equals_pairs(ora["otu"], votes, start)




def buffer_misses(oracle):
    """Over the five test inputs with their eight OTUs: (sequences with votes for more than five OTUs; those whose buffer's
    first OTU is not rule 4's OTU; those whose buffer's first OTU has fewer votes than rule 4's, i.e. not merely a tie)."""
    many = wrong = fewer = 0
    inputs = dict(ORACLE_INPUTS, big=BIG_DNA)
    for name in sorted(inputs):
        a, kw, run = inputs[name]
        from kmergutsjava_amd import synth
        seq, off, rec, _ = synth.high_density_config(*a, **kw)
        off = np.asarray(off, dtype=np.int64)
        ora = oracle.run(synth.table_image(rec), seq.numpy(), off, lookup_mode=1, **run)
        votes, start, cls, bins = model_on(ora, 1 if run.get("aa") else 6, off)
        for s in np.flatnonzero(cls["n_otus"] > 5):
            v = votes[start[s]:start[s + 1]]
            first = ora["otu"]["oI"][s, 0]
            many += 1
            wrong += int(first != cls["otu"][s])
            fewer += int(v["votes"][v["oI"] == first][0] < v["votes"][0])
    return many, wrong, fewer


def test_the_five_slot_buffer_misses_the_winner(oracle):
    """DESIGN.md 9n records these numbers."""
    many, wrong, fewer = buffer_misses(oracle)
    print("more than five OTUs:", many, "buffer's first OTU is not the winner:", wrong, "and has fewer votes:", fewer)
    assert (many, wrong, fewer) == (180, 54, 34)


# ---- layouts ---------------------------------------------------------------------------------------------------------------

def test_structures_match_the_gcc_layout(tmp_path):
    specs = [("kg_otu_vote", N.VOTE_DTYPE), ("kg_otu_class", N.OTU_CLASS_DTYPE), ("kg_otu_bin", N.OTU_BIN_DTYPE)]
    cts = [("kg_vote_params", N.KgVoteParams), ("kg_vote_stats", N.KgVoteStats)]
    src = tmp_path / "layout.c"
    body = ""
    for cname, dt in specs:
        body += 'printf("%%zu\\n", sizeof(%s));\n' % cname + "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in dt.names)
    for cname, ct in cts:
        body += 'printf("%%zu\\n", sizeof(%s));\n' % cname + "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f, _ in ct._fields_)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, dt in specs:
        want += [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    for _, ct in cts:
        want += [C.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_]
    assert out == want
    assert (N.VOTE_DTYPE.itemsize, N.OTU_CLASS_DTYPE.itemsize, N.OTU_BIN_DTYPE.itemsize) == (16, 40, 32)


# ---- the front end ---------------------------------------------------------------------------------------------------------

class _ModelScan:
    """What classify_contigs uses of a ScanResult, computed by the model from the oracle's records."""

    def __init__(self, ora, per):
        self.ora, self.per = ora, per

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def otu_votes(self, offsets, min_votes=10, min_share_pct=50, min_calls=1, device_out=False):
        return model_on(self.ora, self.per, np.asarray(offsets, dtype=np.int64), min_votes=min_votes, min_share_pct=min_share_pct,
                        min_calls=min_calls)


def _front_end(oracle, tmp_path, monkeypatch, name="dna", with_otu_index=True):
    from kmergutsjava_amd import kmer_guts_java as KGJ
    img, seq, off, run = oracle_input(name)
    seq = np.asarray(seq, dtype=np.uint8).tobytes() if not isinstance(seq, (bytes, bytearray)) else bytes(seq)
    off = np.asarray(off, dtype=np.int64)
    n = len(off) - 1
    ids = [b"seq_%d" % k for k in range(n)]
    (tmp_path / "q.fa").write_bytes(b"".join(b">%s\n%s\n" % (ids[k], seq[off[k]:off[k + 1]]) for k in range(n)))
    d = tmp_path / "d"
    d.mkdir()
    (d / "kmer.table.mem_map").write_bytes(b"not read: the scan is the model's")
    onames = [b"organism %d" % i for i in range(8)] if with_otu_index else None
    if onames:
        (d / "otu.index").write_bytes(b"".join(b"%d\t%s\n" % (i, o) for i, o in enumerate(onames)))
    aa = bool(run.get("aa"))

    class _Table:
        def scan(self, batch, boff, params):
            ora = oracle.run(img, np.frombuffer(batch, dtype=np.uint8), boff, lookup_mode=1, aa=params.aa,
                             order_constraint=params.order_constraint, min_hits=params.min_hits)
            return _ModelScan(ora, 1 if params.aa else 6)

    monkeypatch.setattr(KGJ, "_resident_table", lambda path, device: _Table())
    ora = oracle.run(img, np.frombuffer(seq, dtype=np.uint8), off, lookup_mode=1, **run)
    return ids, onames, seq, off, str(d), str(tmp_path / "q.fa"), ora, aa


def test_classify_contigs_writers_on_known_records():
    from kmergutsjava_amd import classify_contigs as CC
    b = VC.Lists(3, 6, [300, 50, 400])
    b.call(0, 2, 8, 1).call(3, 7, 4, 0).call(13, 0, 3, 1)
    votes, start, cls, bins = V.otu_votes(*b.build(), min_votes=5)
    ids, names = [b"c0", b"c1", b"c2"], [b"E. coli", b"B. subtilis"]
    assert CC.format_classes(ids, [300, 50, 400], cls, names) == b"c0\t300\tassigned\tB. subtilis\t8\t12\t1\t2\t2\tE. coli\t4\n"
    assert CC.format_classes(ids, [300, 50, 400], cls, None, write_all=True) == (
        b"c0\t300\tassigned\t1\t8\t12\t1\t2\t2\t0\t4\n" b"c1\t50\tnone\t-\t0\t0\t0\t0\t0\t-\t0\n" b"c2\t400\tbelow\t1\t3\t3\t1\t1\t1\t-\t0\n")
    assert CC.format_votes(ids, votes, start, names) == b"c0\tB. subtilis\t8\t1\nc0\tE. coli\t4\t1\nc2\tB. subtilis\t3\t1\n"
    assert CC.format_votes(ids, votes, start, names, top=1) == b"c0\tB. subtilis\t8\t1\nc2\tB. subtilis\t3\t1\n"
    assert CC.format_bins(bins, names) == b"B. subtilis\t1\t300\t8\t1\n"
    # an OTU index beyond otu.index is written as its number
    assert CC.format_bins(bins, names[:1]) == b"1\t1\t300\t8\t1\n"
    assert CC.summary_line([300, 50, 400], cls, bins) == "Sequences: 3, with votes: 2, assigned: 1, bins: 1, assigned length: 300 of 750, votes: 15"
    t = CC.compare_truth(ids, cls, names, {b"c0": b"B. subtilis", b"c2": b"B. subtilis", b"cX": b"E. coli"})
    assert t == {"labelled": 2, "agree": 1, "disagree": 0, "missed": 1}
    assert CC.summary_line([300, 50, 400], cls, bins, t).endswith(", votes: 15, labelled: 2, agree: 1, disagree: 0, missed: 1")
    assert CC.compare_truth(ids, cls, names, {b"c0": b"E. coli"}) == {"labelled": 1, "agree": 0, "disagree": 1, "missed": 0}


@pytest.mark.parametrize("name,with_otu_index", [("dna", True), ("aa", False)])
def test_classify_contigs_front_end_in_one_batch_and_in_several(oracle, tmp_path, monkeypatch, name, with_otu_index):
    """The files and the summary line do not depend on the batch cap, and equal the writers' output on the model's records of
    the whole input; the bins of the batches add up to the whole input's."""
    from helpers import batch_caps, front_end_batches
    from kmergutsjava_amd import classify_contigs as CC
    from kmergutsjava_amd.kmer_guts_java import KmerGutsJava
    ids, onames, seq, off, d, q, ora, aa = _front_end(oracle, tmp_path, monkeypatch, name, with_otu_index)
    kw = dict(min_votes=3, min_share_pct=20, min_calls=1)       # eight OTUs drawn evenly: a winner holds about a fifth
    votes, start, cls, bins = model_on(ora, 1 if aa else 6, off, **kw)
    lens = np.diff(off).tolist()
    assert 0 < cls["assigned"].sum() and len(bins) > 1 and (cls["n_otus"] > 2).any()
    labels = {ids[s]: CC.otu_name(onames, int(cls["otu"][s]) if s % 3 else 7) for s in range(0, len(ids), 2)}
    (tmp_path / "truth.tsv").write_bytes(b"".join(b"%s\t%s\n" % kv for kv in labels.items()))
    t = CC.compare_truth(ids, cls, onames, labels)
    assert t["agree"] > 0 and t["labelled"] == len(labels)
    want = {"o": CC.format_classes(ids, lens, cls, onames, True), "v": CC.format_votes(ids, votes, start, onames, 2),
            "b": CC.format_bins(bins, onames), "line": CC.summary_line(lens, cls, bins, t)}
    caps = batch_caps(lens)
    keep = KmerGutsJava.MAX_BATCH_CHARS
    assert len(front_end_batches(lens, keep)) == 1
    try:
        for what, cap in [("default", keep)] + sorted(caps.items()):
            KmerGutsJava.MAX_BATCH_CHARS = cap
            split = tmp_path / ("split_" + what)
            line = CC.classify_contigs(d, q, str(tmp_path / "o.tsv"), aa=aa, min_votes=3, min_share=20, min_calls=1, write_all=True,
                                       votes_out=str(tmp_path / "v.tsv"), top=2, bins_out=str(tmp_path / "b.tsv"),
                                       split_dir=str(split), truth=str(tmp_path / "truth.tsv"))
            assert (tmp_path / "o.tsv").read_bytes() == want["o"], (what, cap)
            assert (tmp_path / "v.tsv").read_bytes() == want["v"], (what, cap)
            assert (tmp_path / "b.tsv").read_bytes() == want["b"], (what, cap)
            assert line == want["line"], (what, cap)
            ext = "faa" if aa else "fna"
            assert sorted(os.listdir(split)) == sorted(["otu_%d.%s" % (b["oI"], ext) for b in bins] + ["unassigned." + ext])
            for b in bins:
                rec = (split / ("otu_%d.%s" % (b["oI"], ext))).read_bytes()
                assert rec == b"".join(b">%s\n%s\n" % (ids[s], seq[off[s]:off[s + 1]]) for s in range(len(ids))
                                       if cls["assigned"][s] and cls["otu"][s] == b["oI"])
            assert (split / ("unassigned." + ext)).read_bytes().count(b">") == int((cls["assigned"] == 0).sum())
    finally:
        KmerGutsJava.MAX_BATCH_CHARS = keep
    # only the assigned sequences without --all
    CC.classify_contigs(d, q, str(tmp_path / "o2.tsv"), aa=aa, min_votes=3, min_share=20, min_calls=1)
    assert (tmp_path / "o2.tsv").read_bytes() == CC.format_classes(ids, lens, cls, onames, False)
