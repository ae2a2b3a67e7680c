"""The ops rule (include/kmerguts_hip.h, "the alignments themselves") on the host: tests/ops_model.py against a second, independent
statement that walks the two proteins along the ops and rebuilds the path record and the score from the columns it covers;
answers worked out by hand; the constants against gcc; and the front end's --cigar field and --alignments file with the device
call replaced by the model."""
import os
import subprocess

import numpy as np
import pytest

import align_model as A
import cluster_model as M
import ops_model as O
import search_model as S
import trace_model as T
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import hotpath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M23 = np.full((21, 21), -3, dtype=np.int64)             # +2 / -3, a non-residue scores -3 against everything
np.fill_diagonal(M23, 2)
M23[20, 20] = -3


def rebuilt(a, b, end, ops, S_, go, ge):
    """The second statement: from the end cell and the ops alone -> (the record's seven fields, the score of the columns)."""
    ca, cb = A.codes(a), A.codes(b)
    na = sum(int(x) >> 4 for x in ops if int(x) & 15 != N.OP_D)            # residues of a the ops consume
    nb = sum(int(x) >> 4 for x in ops if int(x) & 15 != N.OP_I)
    i, j = end[1] + 1 - na, end[2] + 1 - nb
    start = (i, j)
    identical = positive = opens = gca = gcb = score = 0
    for x in ops:
        ln, code = int(x) >> 4, int(x) & 15
        if code == N.OP_I:
            opens, gcb, score, i = opens + 1, gcb + ln, score - go - ge * ln, i + ln
        elif code == N.OP_D:
            opens, gca, score, j = opens + 1, gca + ln, score - go - ge * ln, j + ln
        else:
            for _ in range(ln):
                same = ca[i] == cb[j] and ca[i] < 20
                assert code == N.OP_M or (code == N.OP_EQ) == bool(same), (a, b, ops)
                identical += int(same)
                positive += int(S_[ca[i]][cb[j]] > 0)
                score += int(S_[ca[i]][cb[j]])
                i, j = i + 1, j + 1
    assert (i, j) == (end[1] + 1, end[2] + 1)
    return start + (identical, positive, opens, gca, gcb), score


def _check(a, b, S_=A.S62, go=11, ge=1):
    """Both modes of the model against the second statement and the header's invariants.  -> (end, rec, M ops, =/X ops)"""
    end, rec, ops_m = O.ops_of(a, b, S_, go, ge, "m")
    end_x, rec_x, ops_x = O.ops_of(a, b, S_, go, ge, "eqx")
    assert (end, rec) == (end_x, rec_x) == T.trace_loops(a, b, S_, go, ge)
    if rec is None:
        assert ops_m == ops_x == []
        return end, rec, ops_m, ops_x
    for ops in (ops_m, ops_x):
        assert rebuilt(a, b, end, ops, S_, min(go, T.GAP_CAP), min(ge, T.GAP_CAP)) == (rec, end[0]), (a, b, ops)
        assert all(int(p) & 15 != int(q) & 15 for p, q in zip(ops, ops[1:]))          # maximal runs
    O.check_invariants(end, rec, ops_m, ops_x)
    # the box's tables give the same ops (what the device computes)
    assert O.ops_of(a, b, S_, go, ge, "m", end=end)[2] == ops_m and O.ops_of(a, b, S_, go, ge, "eqx", end=end)[2] == ops_x
    return end, rec, ops_m, ops_x


def _cigar(ops):
    return hotpath.cigar(ops)


# ---- the model against the second statement -----------------------------------------------------------------------------------------

def test_model_against_the_rebuilt_record_on_random_pairs():
    rng = np.random.default_rng(31)
    traced = gapped = mixed = 0
    for k in range(300):
        la, lb = int(rng.integers(0, 61)), int(rng.integers(0, 61))
        letters = (b"ACX", b"ACDX", b"ACDEFGHIKLX")[k % 3]
        a = bytes(rng.choice(list(letters), la).tolist())
        b = bytes(rng.choice(list(letters), lb).tolist())
        if k % 4 == 0 and la > 12:
            cut = int(rng.integers(1, 4))
            b = a[:la // 2] + a[la // 2 + cut:]
        S_, go, ge = ((A.S62, 11, 1), (M23, 5, 2), (M23, 0, 1), (A.S62, 0, 1), (M23, 0, 2))[k % 5]
        end, rec, ops_m, ops_x = _check(a, b, S_, go, ge)
        traced += rec is not None
        gapped += rec is not None and rec[4] > 0
        mixed += any(int(x) & 15 == N.OP_X for x in ops_x)
    assert traced > 250 and gapped > 60 and mixed > 60


# ---- known answers ------------------------------------------------------------------------------------------------------------------

def test_a_protein_against_itself():
    p = M.random_protein(np.random.default_rng(32), 50)
    end, rec, ops_m, ops_x = _check(p, p)
    assert _cigar(ops_m) == "50M" and _cigar(ops_x) == "50=" and ops_x == [50 << 4 | 7]


def test_one_substitution():
    p = M.random_protein(np.random.default_rng(33), 41)
    x = bytearray(p)
    x[20] = ord("A") if x[20] == ord("W") else ord("W")
    end, rec, ops_m, ops_x = _check(p, bytes(x))
    assert _cigar(ops_m) == "41M" and _cigar(ops_x) == "20=1X20="


@pytest.mark.parametrize("cut", [1, 3, 10])
def test_a_deletion_each_way(cut):
    """b is a without `cut` residues behind its first 30: a's extra residues face nothing, (a_i, -): I.  Swapped, D."""
    a = M.random_protein(np.random.default_rng(34), 70)
    b = a[:30] + a[30 + cut:]
    end, rec, ops_m, ops_x = _check(a, b)
    assert rec == (0, 0, 70 - cut, 70 - cut, 1, 0, cut)
    # the gap may sit anywhere the residues around it repeat: its place is the model's, its length and the sums are fixed
    assert [int(x) & 15 for x in ops_m] == [N.OP_M, N.OP_I, N.OP_M] and int(ops_m[1]) >> 4 == cut
    assert [int(x) & 15 for x in ops_x] == [N.OP_EQ, N.OP_I, N.OP_EQ]
    end, rec, ops_m, ops_x = _check(b, a)
    assert rec == (0, 0, 70 - cut, 70 - cut, 1, cut, 0)
    assert [int(x) & 15 for x in ops_m] == [N.OP_M, N.OP_D, N.OP_M] and int(ops_m[1]) >> 4 == cut
    assert (int(ops_m[0]) >> 4) + (int(ops_m[2]) >> 4) == 70 - cut


def test_all_x_aligned_under_a_matrix_that_rewards_it():
    """X against X scores -1 in BLOSUM62: no path and no ops.  Under a matrix with S[X][X] = 1 the twelve columns are a path whose
    columns are not identical by the record's definition (code 20): 12X, identical 0."""
    assert _check(b"X" * 12, b"X" * 9)[1:] == (None, [], [])
    S1 = np.array(A.S62, dtype=np.int64)
    S1[20, 20] = 1
    end, rec, ops_m, ops_x = _check(b"X" * 12, b"X" * 12, S1)
    assert rec[2] == 0 and _cigar(ops_x) == "12X" and _cigar(ops_m) == "12M"


def test_an_i_run_next_to_a_d_run_under_gap_open_0():
    """a = AACDD (rows), b = AAEEDD..: with +2 / -3 and a gap of k costing k, C against E is worse (-3) than a gap each way
    (-2): between the A's and the D's the path has one (a_i, -) column and two (-, b_j) columns side by side, two ops and two
    openings."""
    a, b = b"AAAACDDDD", b"AAAAEEDDDD"
    end, rec, ops_m, ops_x = _check(a, b, M23, 0, 1)
    assert end[0] == 8 + 8 - 1 - 2 and rec == (0, 0, 8, 8, 2, 2, 1)
    kinds = [int(x) & 15 for x in ops_m]
    assert sorted(kinds[1:3]) == [N.OP_I, N.OP_D] and kinds[0] == kinds[3] == N.OP_M and len(ops_m) == 4
    assert _cigar(ops_m) in ("4M1I2D4M", "4M2D1I4M") and _cigar(ops_x) == _cigar(ops_m).replace("M", "=")


def test_cigar_and_merged():
    assert hotpath.cigar(np.array([5 << 4 | 7, 1 << 4 | 8, 3 << 4 | 2, 2 << 4 | 7], dtype=np.uint32)) == "5=1X3D2="
    assert hotpath.cigar([]) == "*"
    assert O.merged([5 << 4 | 7, 1 << 4 | 8, 3 << 4 | 2, 2 << 4 | 7]) == [6 << 4, 3 << 4 | 2, 2 << 4]


# ---- the header --------------------------------------------------------------------------------------------------------------------

def test_constants_and_sizes_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "kmerguts_hip.h"\nint main(void){\n'
                   'printf("%d %d %d %d %d %d %d %d %d\\n", KG_TRACE_OPS, KG_TRACE_OPS_EQX, KG_OP_M, KG_OP_I, KG_OP_D, KG_OP_EQ, KG_OP_X, '
                   'KG_TRACE_HITS, KG_TRACE_ALL);\n'
                   'printf("%zu %zu %zu\\n", sizeof(kg_alignment_path), sizeof(kg_trace_stats), sizeof(uint32_t));\n'
                   'kg_opset *s = 0; (void)s; return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:9] == [N.TRACE_OPS, N.TRACE_OPS_EQX, N.OP_M, N.OP_I, N.OP_D, N.OP_EQ, N.OP_X, N.TRACE_HITS, N.TRACE_ALL] == [4, 8, 0, 1, 2, 7, 8, 1, 2]
    assert out[9:] == [32, 32, 4]
    assert N.OPS_MODES == {"m": 4, "eqx": 8} and (N.TRACE_OPS | N.TRACE_OPS_EQX) & 3 == 0
    assert {"kg_proteins_align_ops", "kg_proteins_align_ops_device", "kg_opset_ops_count", "kg_opset_op_starts_copy", "kg_opset_ops_copy",
            "kg_opset_ms_ops", "kg_opset_free", "kg_hitset_ops_count", "kg_hitset_op_starts_copy", "kg_hitset_ops_copy",
            "kg_hitset_ms_ops"} <= set(N.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "kmerguts_hip.h")).read()
    for name in ("kg_proteins_align_ops", "kg_hitset_op_starts_copy", "n_ops <= 2 * gap_opens + 1", "len << 4 | code"):
        assert name in hdr, name
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "kg_proteins_align_ops" in open(os.path.join(ROOT, doc)).read(), doc
    assert "9t" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "kg_proteins_align_ops" in open(os.path.join(ROOT, "java", "kmergutsjava", "KmerGutsHip.java")).read()


# ---- the front end ----------------------------------------------------------------------------------------------------------------

def _model_search(seq, offsets, n_db, min_shared=2, max_cand=8, max_db_per_kmer=256, align=None, device=0, paths=None,
                  max_trace_cells=N.TRACE_DEFAULT_MAX_CELLS, ops=None):
    kw = dict(min_shared=min_shared, max_cand=max_cand, max_db_per_kmer=max_db_per_kmer, **(align or {}))
    if paths is None:
        assert ops is None
        return S.search_model(seq, offsets, n_db, **kw)
    hits, start, recs, counts = T.search_paths_model(seq, offsets, n_db, paths, max_trace_cells, **kw)
    st = dict(counts, ms_trace=0.25)
    if ops is None:
        return hits, start, recs, st
    _, _, recs2, op_start, op = O.search_ops_model(seq, offsets, n_db, ops, paths, max_trace_cells, **kw)
    assert recs2.tobytes() == recs.tobytes()
    return hits, start, recs, dict(st, ops=len(op), ms_ops=0.125), op_start, op


def _fasta(path, ids, seqs):
    path.write_bytes(b"".join(b">%s some words\n%s\n" % (i, s) for i, s in zip(ids, seqs)))
    return str(path)


def _files(tmp_path):
    rng = np.random.default_rng(37)
    a, b, c = (M.random_protein(rng, 60) for _ in range(3))
    a_del = a[5:30] + a[33:]                             # a without its first five residues and three of its middle
    b_half = b[:20] + M.random_protein(rng, 30)          # shares 8-mers with b, scores under half of it
    db = _fasta(tmp_path / "db.faa", [b"dA", b"dB", b"dC"], [a, b, c])
    qs = _fasta(tmp_path / "q.faa", [b"q1", b"q2", b"q3", b"q4"], [a_del, b, b_half, M.random_protein(rng, 40)])
    (tmp_path / "ann.tsv").write_bytes(b"dA\tkinase\tE\ndB\tligase\n")
    return db, qs, str(tmp_path / "ann.tsv"), (a, a_del, b)


def test_front_end_cigar_field_order_and_flags_off(tmp_path):
    from kmergutsjava_amd import search_proteins as SP
    db, qs, ann, (a, a_del, b) = _files(tmp_path)
    out, old = str(tmp_path / "hits.tsv"), str(tmp_path / "old.tsv")
    line_old = SP.search_proteins([db], [qs], old, annotations=ann, write_all=True, search=_model_search, paths="hits")
    olds = [r.split(b"\t") for r in open(old, "rb").read().splitlines()]
    assert all(len(r) == 21 for r in olds) and ", ops" not in line_old
    # flags off: the bytes are those of a call that never heard of the flags
    line = SP.search_proteins([db], [qs], out, annotations=ann, write_all=True, search=_model_search, paths="hits", cigar=None, alignments=None)
    assert open(out, "rb").read() == open(old, "rb").read() and line == line_old
    # --cigar: one field behind the ten path fields and in front of the function
    line = SP.search_proteins([db], [qs], out, annotations=ann, write_all=True, search=_model_search, paths="hits", cigar="m")
    rows = [r.split(b"\t") for r in open(out, "rb").read().splitlines()]
    assert [r[:20] + r[21:] for r in rows] == olds and all(len(r) == 22 for r in rows)
    want = hotpath.cigar(O.ops_of(a_del, a, mode="m")[2]).encode()
    assert rows[0][20] == want and want.count(b"D") == 1 and b"3D" in want and rows[0][21] == b"kinase"
    assert rows[1][20] == b"60M" and rows[2][20] == b"-" and rows[2][10:20] == [b"-"] * 10       # below the ratio: no path, `-`
    assert line == line_old + ", ops: %d" % (3 + 1)
    SP.search_proteins([db], [qs], out, write_all=True, search=_model_search, paths="all", cigar="eqx")
    rows = [r.split(b"\t") for r in open(out, "rb").read().splitlines()]
    assert all(len(r) == 21 for r in rows) and rows[1][20] == b"60=" and rows[2][20] == b"20="    # q3 shares b's first twenty residues
    assert rows[0][20] == hotpath.cigar(O.ops_of(a_del, a, mode="eqx")[2]).encode()
    # refused without --paths, by the function and by the command line
    for kw in (dict(cigar="m"), dict(alignments=str(tmp_path / "x.txt")), dict(cigar="eqx", alignments=str(tmp_path / "x.txt"))):
        with pytest.raises(ValueError, match="need --paths"):
            SP.search_proteins([db], [qs], out, search=_model_search, **kw)
    with pytest.raises(ValueError, match="--cigar"):
        SP.search_proteins([db], [qs], out, search=_model_search, paths="hits", cigar="some")
    assert not os.path.exists(tmp_path / "x.txt")
    for extra in (["--cigar"], ["--cigar", "eqx"], ["--alignments", str(tmp_path / "x.txt")]):
        with pytest.raises(SystemExit):
            SP.main(["-d", db, "-q", qs, "-o", out] + extra)


def test_front_end_flag_defaults(tmp_path, monkeypatch):
    from kmergutsjava_amd import search_proteins as SP
    seen = []

    def fake(database, queries, out, *args, **kw):
        seen.append((kw.get("paths"), kw.get("cigar"), kw.get("alignments")))
        return "line"

    monkeypatch.setattr(SP, "search_proteins", fake)
    base = ["-d", "d.faa", "-q", "q.faa", "-o", str(tmp_path / "o.tsv")]
    for extra in ([], ["--paths"], ["--paths", "--cigar"], ["--paths", "--cigar", "eqx"], ["--paths", "--alignments", "al.txt"],
                  ["--paths", "--cigar", "m", "--alignments", "al.txt", "--all"]):
        assert SP.main(base + extra) == 0
    assert seen == [(None, None, None), ("hits", None, None), ("hits", "m", None), ("hits", "eqx", None), ("hits", None, "al.txt"),
                    ("all", "m", "al.txt")]


def test_which_ops_the_device_is_asked_for(tmp_path):
    """--alignments alone asks for eqx and adds no field; with --cigar m the device is asked for M ops and the host compares."""
    from kmergutsjava_amd import search_proteins as SP
    db, qs, ann, _ = _files(tmp_path)
    asked = []

    def search(*args, **kw):
        asked.append(kw.get("ops"))
        return _model_search(*args, **kw)

    out, al = str(tmp_path / "hits.tsv"), str(tmp_path / "al.txt")
    SP.search_proteins([db], [qs], out, search=search, paths="hits", alignments=al)
    assert all(len(r.split(b"\t")) == 20 for r in open(out, "rb").read().splitlines())
    first = open(al, "rb").read()
    SP.search_proteins([db], [qs], out, search=search, paths="hits", alignments=al, cigar="m")
    SP.search_proteins([db], [qs], out, search=search, paths="hits", cigar="m")
    SP.search_proteins([db], [qs], out, search=search, paths="hits")
    assert asked == ["eqx", "m", "m", None]
    assert open(al, "rb").read() == first and first.count(b">") == 2     # the same text from either mode: one block per written hit


def test_the_alignments_block_of_a_pair_with_a_gap_across_the_wrap():
    """Made by hand: 58 identical columns, a gap of four target residues that begins at column 59 and ends in the second row, one
    substitution (I for L: positive), and 10 more identical columns.  Query 71 residues, target 74; the alignment starts at
    query residue 3 and target residue 2."""
    core = b"MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQAPILSRVGDGTQDNLSGAEKAVQVKVK"      # 60
    q = b"GG" + core[:58] + b"L" + b"ALPDAQFEVV"
    t = b"W" + core[:58] + b"PPPP" + b"I" + b"ALPDAQFEVV"
    ops = np.array([58 << 4 | N.OP_EQ, 4 << 4 | N.OP_D, 1 << 4 | N.OP_X, 10 << 4 | N.OP_EQ], dtype=np.uint32)
    path = np.zeros(1, dtype=N.ALIGN_PATH_DTYPE)[0]
    path["start_a"], path["start_b"], path["identical"] = 2, 1, 68
    hit = {"score": 321}
    text = hotpath.alignment_text(q, t, hit, path, ops, query_id="q1", target_id="dA")
    want = "\n".join([
        ">q1 dA score=321 identity=93% columns=73",
        "Query   3  " + core[:58].decode() + "--" + "  60",
        "           " + core[:58].decode() + "  ",
        "Target  2  " + core[:58].decode() + "PP" + "  61",
        "",
        "Query  61  --LALPDAQFEVV  71",
        "             +ALPDAQFEVV",
        "Target 62  PPIALPDAQFEVV  74",
        ""])
    assert text == want, text
    # the same text from M ops: the host compares the residues
    ops_m = np.array(O.merged(ops), dtype=np.uint32)
    assert hotpath.alignment_text(q, t, hit, path, ops_m, query_id="q1", target_id="dA") == want
    assert hotpath.cigar(ops_m) == "58M4D11M"
    # a narrower row wraps the same columns
    narrow = hotpath.alignment_text(q, t, hit, path, ops, width=30, query_id="q1", target_id="dA").splitlines()
    assert len(narrow) == 3 * 4 and narrow[1].endswith("  32") and narrow[9].startswith("Query  61  ")
