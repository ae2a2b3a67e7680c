"""Signature derivation without a GPU: the torch model (tests/signature_model.py) against a pure-Python brute force, the
make_signatures front end's parsing, numbering and errors, and its text writer through make_table.parse_signatures."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import signature_model as M  # noqa: E402

from kmergutsjava_amd import make_signatures as MS  # noqa: E402
from kmergutsjava_amd import make_table as MT  # noqa: E402


def _tiny(rng):
    """A tiny input with many shared k-mers: proteins cut from a few short templates over a 4-letter alphabet (plus
    repeats inside a protein, invalid letters, short proteins), random functions / OTUs from small sets (ties)."""
    letters = np.frombuffer(rng.choice([b"ACDE", b"AAAC", b"ACDEFGHIKL"]), dtype=np.uint8)
    n = int(rng.integers(0, 12))
    seqs = []
    for _ in range(n):
        L = int(rng.integers(0, 24))
        s = letters[rng.integers(0, len(letters), size=L)].copy()
        if L and rng.random() < 0.2:
            s[rng.integers(0, L)] = rng.choice(np.frombuffer(b"Xx*a", dtype=np.uint8))
        seqs.append(s.tobytes())
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    fn = rng.integers(-1, 3, size=n).astype(np.int32)
    otu = rng.integers(0, 3, size=n).astype(np.int32)
    return b"".join(seqs), offsets, fn, otu


@pytest.mark.parametrize("seed", range(300))
def test_model_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    seq, off, fn, otu = _tiny(rng)
    minp = int(rng.choice([1, 2, 3]))
    pur = int(rng.choice([1, 50, 67, 80, 100]))
    want = M.brute_force(seq, list(off), list(fn), list(otu), minp, pur)
    got = M.derive(seq, off, fn, otu, minp, pur)
    assert got.tobytes() == want.tobytes()


def test_model_semantics_by_hand():
    # "ACDEFGHIK" (9 letters) has one window (i in [0, 1)); proteins 0..2 share it; fn 0, 0, 1: f* = 0, c = 2, n = 3
    seq = b"ACDEFGHIK" + b"ACDEFGHIKL" + b"ACDEFGHIK"
    off = [0, 9, 19, 28]
    got = M.derive(seq, off, [0, 0, 1], [5, 3, 0], 2, 60)
    assert len(got) == 1
    r = got[0]
    assert int(r["kmer"]) == MT.encode_kmers(np.frombuffer(b"ACDEFGHI", dtype=np.uint8)[None])[0]
    assert int(r["functionIndex"]) == 0 and int(r["otuIndex"]) == 3           # OTU tie 5 / 3: the smallest
    assert int(r["avgFromEnd"]) == (9 + 10) // 2
    assert r["functionWt"] == np.float32(2) / np.float32(3)
    assert len(M.derive(seq, off, [0, 0, 1], [5, 3, 0], 2, 67)) == 0           # 200 < 67 * 3
    assert len(M.derive(seq, off, [-1, -1, -1], [0, 0, 0], 1, 1)) == 0          # no f*
    assert len(M.derive(b"ACDEFGHI", [0, 8], [0], [0], 1, 1)) == 0              # length 8: no window


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_fasta_and_tsv_parsing_and_numbering():
    ids, seqs = MS.parse_fasta(b">p2 some text\nACDE\n FGHI \n\n>p1\r\nKLMN\r\n>p3\n")
    assert ids == [b"p2", b"p1", b"p3"] and seqs == [b"ACDEFGHI", b"KLMN", b""]
    ann = MS.parse_annotations(b"p1\tzeta\tB\n\np2\talpha\r\np9\tbeta\tA\n")
    assert ann == {b"p1": (b"zeta", b"B"), b"p2": (b"alpha", b""), b"p9": (b"beta", b"A")}
    seq, off, fn, otu, fnames, onames = MS.number_inputs(ids, seqs, ann)
    assert fnames == [b"alpha", b"beta", b"zeta"] and onames == [b"", b"A", b"B"]   # byte order; p9 is not a protein
    assert seq == b"ACDEFGHIKLMN" and list(off) == [0, 8, 12, 12]
    assert list(fn) == [0, 2, -1] and list(otu) == [0, 2, 0]


@pytest.mark.parametrize("data,what", [
    (b">a\nAC\n>b\nDE\n>a\nFF\n", "line 5: duplicate protein id a (first on line 1)"),
    (b"ACDE\n>a\nAC\n", "line 1: sequence text before"),
    (b">a\nAC\n> \nDE\n", "line 3: caption without an id"),
])
def test_fasta_errors_name_the_line(data, what):
    with pytest.raises(MS.InputError, match=what.replace("(", r"\(").replace(")", r"\)")):
        MS.parse_fasta(data)


@pytest.mark.parametrize("data,what", [
    (b"a\tf\nb\n", "line 2: malformed line"),
    (b"a\tf\tx\ty\n", "line 1: malformed line"),
    (b"a\t\n", "line 1: malformed line"),
    (b"a\tf\n\nb\tg\na\th\n", r"line 4: protein id a repeated \(first on line 1\)"),
])
def test_tsv_errors_name_the_line(data, what):
    with pytest.raises(MS.InputError, match=what):
        MS.parse_annotations(data)


def test_cli_reports_input_errors(tmp_path, capsys):
    p = _write(tmp_path, "p.faa", b">a\nACDEFGHIKL\n>a\nAC\n")
    a = _write(tmp_path, "a.tsv", b"a\tf\n")
    assert MS.main(["-p", p, "-A", a, "-o", str(tmp_path / "o.txt")]) == 1
    assert "line 3: duplicate protein id a" in capsys.readouterr().err
    p = _write(tmp_path, "q.faa", b">a\nACDEFGHIKL\n")
    a = _write(tmp_path, "b.tsv", b"a\n")
    assert MS.main(["-p", p, "-A", a, "-o", str(tmp_path / "o.txt")]) == 1
    assert "line 1: malformed line" in capsys.readouterr().err


def test_text_writer_round_trips_through_parse_signatures():
    rng = np.random.default_rng(5)
    n = 5000
    sigs = np.zeros(n, dtype=M.N.SIGNATURE_DTYPE)
    sigs["kmer"] = np.sort(rng.integers(0, 20 ** 8, size=n))
    sigs["otuIndex"] = rng.integers(0, 2 ** 31, size=n)
    sigs["avgFromEnd"] = rng.integers(1, 2 ** 31, size=n)
    sigs["functionIndex"] = rng.integers(0, 2 ** 31, size=n)
    c = rng.integers(1, 10 ** 6, size=n)
    sigs["functionWt"] = np.float32(c) / np.float32(c + rng.integers(0, 10 ** 6, size=n))
    sigs["functionWt"][:3] = [np.float32(1), np.float32(1) / np.float32(3), np.nextafter(np.float32(1), np.float32(0))]
    back = MT.parse_signatures(MS.signature_text(sigs).encode())
    assert back.tobytes() == sigs.tobytes()
