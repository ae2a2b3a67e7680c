"""The composition rule's model (tests/compose_model.py) on hand-checked answers, the planted sample's expectations under that
model, and the host side of classify_contigs --compose: the formatters and the model file.  No GPU takes part."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compose_cases as KC  # noqa: E402
import compose_model as K  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import classify_contigs as CC  # noqa: E402
from kmergutsjava_amd.make_signatures import InputError  # noqa: E402


def _counts(text: bytes) -> np.ndarray:
    return K.contig_counts(np.frombuffer(text, np.uint8), np.array([0, len(text)], np.int64))[0]


def test_known_answers_of_the_counts():
    acgt, aaaa, tttt = K.index(b"ACGT"), K.index(b"AAAA"), K.index(b"TTTT")
    assert (acgt, aaaa, tttt) == (0b00011011, 0, 255) and K.rc(acgt) == acgt and K.rc(aaaa) == tttt
    n = _counts(b"ACGT")
    assert n[acgt] == 2 and n.sum() == 2                    # a palindrome counts twice
    n = _counts(b"AAAAA")
    assert n[aaaa] == 2 and n[tttt] == 2 and n.sum() == 4
    assert _counts(b"ACG").sum() == 0 and _counts(b"").sum() == 0
    # a tetramer holding N or x is absent; lower case and u count
    assert _counts(b"ACNGT").sum() == 0 and _counts(b"ACxGT").sum() == 0
    n = _counts(b"ACGTNACGT")
    assert n[acgt] == 4 and n.sum() == 4
    assert np.array_equal(_counts(b"acgu"), _counts(b"ACGT")) and np.array_equal(_counts(b"AcGtTa"), _counts(b"ACGTTA"))
    assert K.index(b"ACGN") == -1 and K.index(b"TTTU") == 255
    # a tetramer never spans two contigs
    both = K.contig_counts(np.frombuffer(b"ACGACG", np.uint8), np.array([0, 3, 6], np.int64))
    assert both.sum() == 0
    # the batch-wide restatement is the contig-by-contig one
    rng = np.random.default_rng(1)
    seq, off, _ = KC.batch(rng, [0, 7, 0, 0, 3, 4, 300, 1, 0, 64, 5, 0])
    assert np.array_equal(K.contig_counts(seq, off), K.contig_counts_loops(seq, off)) and K.contig_counts(seq, off).sum() > 400
    pad = np.concatenate([seq[:5], seq])                     # bytes in front of the first contig belong to none
    assert np.array_equal(K.contig_counts(pad, off + 5), K.contig_counts(seq, off))


def test_a_contig_and_its_reverse_complement_have_the_same_counts():
    rng = np.random.default_rng(5)
    comp = bytes.maketrans(b"ACGTacgtUuNn", b"TGCAtgcaAaNn")
    for n in (4, 5, 64, 1000):
        text = bytes(rng.choice(np.frombuffer(b"ACGTacgtUuNn", np.uint8), size=n))
        a, b = _counts(text), _counts(text.translate(comp)[::-1])
        assert np.array_equal(a, b) and a.sum() % 2 == 0
        assert np.array_equal(a, a[K._RC])


def test_ties_and_the_background_alone():
    rng = np.random.default_rng(6)
    seq, off, _ = KC.batch(rng, [300, 2000, 5])
    row = rng.integers(0, 1000, size=256)
    far = np.zeros(256, np.int64)                           # a background no random contig looks like
    far[0] = 10 ** 6
    # two identical models tie: the smaller index wins with margin 0, and nothing is decided at a margin above 0
    model = (np.array([4, 9], np.int32), np.stack([row, row, far]))
    got = K.compose(seq, off, None, model, min_len=0, min_margin=0)
    c = got["classes"][1]
    assert (c["best"], c["second"], c["score_best"] - c["score_second"], c["decided"]) == (4, 9, 0, 1)
    assert K.compose(seq, off, None, model, min_len=0, min_margin=1)["classes"]["decided"].sum() == 0
    # a bin that ties with the background comes first
    model = (np.array([4], np.int32), np.stack([row, row]))
    c = K.compose(seq, off, None, model, min_len=0, min_margin=0)["classes"][1]
    assert (c["best"], c["second"], c["decided"]) == (4, -1, 1)
    # M = 0: only the background
    got = K.compose(seq, off, None, None)
    assert got["stats"]["models"] == 0 and got["scores"].shape == (3, 1)
    for c in got["classes"]:
        assert (c["best"], c["second"], c["decided"]) == (-1, -1, 0) and c["score_best"] == c["score_second"]
    # min_len, and a contig without windows scores 0 everywhere: the first model is best with margin 0
    model = (np.array([4], np.int32), np.stack([row, far]))
    cls = K.compose(seq, off, None, model, min_len=301, min_margin=0)["classes"]
    assert cls["decided"][0] == 0 and cls["windows"].tolist() == [int(x) for x in K.contig_counts(seq, off).sum(axis=1)]
    assert K.compose(b"NNNNNN", [0, 6], None, model, 0, 0)["classes"][0]["score_best"] == 0


def test_label_rows_add_up_and_min_train_selects_models():
    seq, off, lab, min_train = KC.label_case("min_train_drops_rows")
    whole = K.compose(seq, off, lab, None, min_train=min_train)
    R, M = len(whole["row_labels"]), len(whole["model_labels"])
    assert 1 < M < R and 4 in whole["model_labels"]
    assert np.array_equal(whole["rows"].sum(axis=1) >= min_train, np.isin(whole["row_labels"], whole["model_labels"]))
    assert np.array_equal(whole["background"], whole["counts"].astype(np.int64).sum(axis=0))
    acc, bg = {}, np.zeros(256, np.int64)
    for a, b in ((0, 300), (300, 301), (301, len(lab))):
        part = K.compose(*KC.cut(seq, off, lab, a, b), None, min_train=1 << 62)
        assert part["stats"]["models"] == 0
        CC.add_label_rows(acc, part["row_labels"], part["rows"])
        bg += part["background"]
    labels, counts = CC.model_of_rows(acc, bg, min_train)
    assert np.array_equal(labels, whole["model_labels"]) and np.array_equal(counts[-1], whole["background"])
    assert np.array_equal(K.scores(whole["counts"], counts), whole["scores"])
    assert whole["stats"]["conflicts"] == int(((whole["classes"]["decided"] != 0) & (lab >= 0) & (whole["classes"]["best"] != lab)).sum())


def test_the_planted_sample_meets_its_expectations_under_the_model():
    """The conditions tests/test_gpu_compose.py puts on the planted sample, checked where no GPU is needed: with the voted
    contigs labelled, the rule puts every unvoted contig of 1500 bp or more into its genome's bin, leaves the 1000 bp contigs
    and the foreign contigs alone (the background is best for every foreign one), and makes no conflict."""
    _, contigs, kinds, genomes = KC.planted_sample()
    off = KC.offsets_of([len(c) for c in contigs])
    lab = np.array([g if k == "voted" else -1 for k, g in zip(kinds, genomes)], np.int32)
    got = K.compose(np.frombuffer(b"".join(contigs), np.uint8), off, lab)
    assert got["model_labels"].tolist() == [0, 1] and (got["rows"].sum(axis=1) >= 200000).all()
    margins = []
    for c, kind, g in zip(got["classes"], kinds, genomes):
        if kind == "voted":
            assert c["decided"] and c["best"] == g
        elif kind == "unvoted":
            assert c["decided"] and c["best"] == g
            margins.append(int(c["score_best"] - c["score_second"]))
        elif kind == "short":
            assert not c["decided"] and c["best"] == g
        else:
            assert not c["decided"] and c["best"] == -1
    assert got["stats"]["conflicts"] == 0 and got["stats"]["decided_unlabelled"] == 2 * KC.N_UNVOTED
    assert min(margins) >= 10 * 2560, min(margins)          # far from the threshold: no expectation hangs on a near tie


def _records():
    cls = np.zeros(4, dtype=N.OTU_CLASS_DTYPE)
    cls[0] = (1, 1, 8, 12, 1, 2, 2, 0, 4, 0)
    cls[1] = (-1, 0, 0, 0, 0, 0, 0, -1, 0, 0)
    cls[2] = (1, 0, 3, 3, 1, 1, 1, -1, 0, 0)
    cls[3] = (0, 1, 20, 20, 2, 2, 1, -1, 0, 0)
    comp = np.zeros(4, dtype=N.COMP_CLASS_DTYPE)
    comp[0] = (1, 1, -1, 1, 594, -4000, -9000)
    comp[1] = (-1, 0, 1, 1, 3994, -30000, -33000)           # composed into OTU 0
    comp[2] = (-1, -1, 1, 0, 94, -700, -720)                # the background is best
    comp[3] = (0, 1, 0, 1, 7994, -60000, -70000)            # assigned to 0, decided for 1: a conflict
    return [b"c0", b"c1", b"c2", b"c3"], [300, 2000, 50, 4000], cls, comp, [b"E. coli", b"B. subtilis"]


def test_formatters_with_composition():
    ids, lens, cls, comp, names = _records()
    assert CC.format_classes(ids, lens, cls, names, comp=comp) == (
        b"c0\t300\tassigned\tB. subtilis\t8\t12\t1\t2\t2\tE. coli\t4\tB. subtilis\t5000\t594\n"
        b"c1\t2000\tcomposed\tE. coli\t0\t0\t0\t0\t0\t-\t0\tE. coli\t3000\t3994\n"
        b"c3\t4000\tassigned\tE. coli\t20\t20\t2\t2\t1\t-\t0\tB. subtilis\t10000\t7994\n")
    full = CC.format_classes(ids, lens, cls, names, True, comp).splitlines()
    assert len(full) == 4 and full[2] == b"c2\t50\tbelow\tB. subtilis\t3\t3\t1\t1\t1\t-\t0\t-\t20\t94"
    # without the flag nothing changes
    assert CC.format_classes(ids, lens, cls, names) == b"".join(ln.rsplit(b"\t", 3)[0] + b"\n" for ln in full if b"assigned" in ln)
    composed = CC.composed_bins(lens, cls, comp)
    assert composed == {0: [1, 2000]}
    bins = np.zeros(1, dtype=N.OTU_BIN_DTYPE)
    bins[0] = (1, 1, 300, 8, 1)
    assert CC.format_bins(bins, names, composed) == b"B. subtilis\t1\t300\t8\t1\t0\t0\nE. coli\t0\t0\t0\t0\t1\t2000\n"
    assert CC.format_bins(bins, names, {}) == b"B. subtilis\t1\t300\t8\t1\t0\t0\n"
    assert CC.format_bins(bins, names) == b"B. subtilis\t1\t300\t8\t1\n"
    assert CC.comp_summary(lens, cls, comp, 2) == ", composed: 1, composed length: 2000, conflicts: 1, models: 2"
    t = CC.compare_truth_composed(ids, cls, comp, names, {b"c1": b"E. coli", b"c0": b"E. coli", b"c2": b"E. coli"})
    assert t == {"agree": 1, "disagree": 0}
    assert CC.compare_truth_composed(ids, cls, comp, names, {b"c1": b"B. subtilis"}) == {"agree": 0, "disagree": 1}
    assert CC.comp_summary(lens, cls, comp, 2, t).endswith(", models: 2, composed agree: 1, composed disagree: 0")


def test_split_puts_composed_contigs_into_their_bin(tmp_path):
    ids, lens, cls, comp, names = _records()
    seqs = [b"A" * 3, b"C" * 4, b"G" * 5, b"T" * 6]
    bins = np.zeros(1, dtype=N.OTU_BIN_DTYPE)
    bins[0] = (1, 1, 300, 8, 1)
    cls[3]["assigned"] = 0                                  # (c3 unassigned: decided for OTU 1, which has a bin already)
    CC.write_split(str(tmp_path / "s"), ids, seqs, cls, bins, False, comp)
    got = {f: (tmp_path / "s" / f).read_bytes() for f in sorted(os.listdir(tmp_path / "s"))}
    assert got == {"otu_0.fna": b">c1\nCCCC\n", "otu_1.fna": b">c0\nAAA\n>c3\nTTTTTT\n", "unassigned.fna": b">c2\nGGGGG\n"}


def test_model_file_round_trip_and_error_lines():
    rng = np.random.default_rng(8)
    names = [b"E. coli", b"B. subtilis", b"third"]
    labels, counts = KC.callers_model(rng, 3)
    labels = np.array([0, 2, 7], np.int32)
    data = CC.format_comp_model(labels, counts, names)
    lines = data.split(b"\n")
    assert lines[0] == b"#kmerguts composition model 1" and len(lines) == 6 and lines[-1] == b""
    assert lines[1].startswith(b"0\tE. coli\t") and lines[2].startswith(b"2\tthird\t") and lines[3].startswith(b"7\t-\t")
    assert lines[4].startswith(b"-1\tbackground\t") and all(len(ln.split(b"\t")) == 258 for ln in lines[1:5])
    got = CC.parse_comp_model(data, "m.txt", names)
    assert np.array_equal(got[0], labels) and np.array_equal(got[1], counts) and got[1].dtype == np.int64
    assert int(got[1][2].sum()) == (1 << 62) - 1
    # a model of the background alone; a directory without otu.index takes any name
    only = CC.format_comp_model([], counts[-1:], None)
    got = CC.parse_comp_model(only, "m.txt", None)
    assert len(got[0]) == 0 and np.array_equal(got[1], counts[-1:])
    assert CC.parse_comp_model(data, "m.txt", None)[0].tolist() == [0, 2, 7]

    def bad(text, word):
        with pytest.raises(InputError) as ei:
            CC.parse_comp_model(text, "m.txt", names)
        assert word in str(ei.value), ei.value

    bad(b"", "m.txt line 1")
    bad(b"#kmerguts composition model 2\n" + b"\n".join(lines[1:]), "m.txt line 1")
    bad(data.replace(b"2\tthird", b"2\tE. coli"), "m.txt line 3: otu 2 is E. coli here and third in otu.index")
    bad(b"\n".join(lines[:4]) + b"\n", "background row")
    bad(b"\n".join(lines[:5] + lines[1:2]) + b"\n", "m.txt line 6: a row behind the background row")
    bad(data.replace(b"0\tE. coli\t", b"0\tE. coli\t5\t", 1), "m.txt line 2: expected otu_index")
    bad(data.replace(b"0\tE. coli\t", b"x\tE. coli\t", 1), "m.txt line 2: otu_index and the counts are integers")
    bad(data.replace(b"7\t-\t", b"7\t-\t-", 1), "m.txt line 4: a count outside")
    bad(data.replace(b"-1\tbackground", b"-1\tthird"), "m.txt line 5")
    bad(data.replace(b"7\t-\t", b"-2\t-\t", 1), "m.txt line 4")


def test_compose_is_dna_only_and_the_model_flags_need_it(tmp_path, capsys):
    with pytest.raises(ValueError):
        CC.classify_contigs(str(tmp_path), "q.faa", str(tmp_path / "o"), aa=True, compose=True)
    with pytest.raises(ValueError):
        CC.classify_contigs(str(tmp_path), "q.fna", str(tmp_path / "o"), comp_model="m.txt")
    for argv in (["-D", "d", "-p", "q.faa", "-o", "o", "--compose"], ["-D", "d", "-q", "q.fna", "-o", "o", "--save-comp-model", "m"]):
        with pytest.raises(SystemExit):
            CC.main(argv)
    assert "--compose" in capsys.readouterr().err
