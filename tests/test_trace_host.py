"""The traceback rule (include/kmerguts_hip.h, kg_proteins_align_paths) on the host: the two forms of tests/trace_model.py against
each other on random pairs in which ties are common, answers worked out by hand (one per preference of the rule), the record
layouts against gcc and the JNA source, and the front end's --paths fields with the device call replaced by the model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import align_model as A
import cluster_model as M
import search_model as S
import test_java_binding as H
import trace_model as T
from kmergutsjava_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M23 = np.full((21, 21), -3, dtype=np.int64)             # +2 / -3, a non-residue scores -3 against everything
np.fill_diagonal(M23, 2)
M23[20, 20] = -3


def _check(a, b, S_, go, ge, ties=None):
    """Both forms agree; the invariants of a traced record hold.  -> (end, record)"""
    end, rec, cols = T.trace_loops(a, b, S_, go, ge, with_columns=True, ties=ties)
    assert (end, rec, cols) == T.trace_numpy(a, b, S_, go, ge, with_columns=True), (a, b, go, ge)
    assert end == A.sw_loops(a, b, S_, min(go, T.GAP_CAP), min(ge, T.GAP_CAP)) == A.sw_numpy(a, b, S_, min(go, T.GAP_CAP), min(ge, T.GAP_CAP))
    if rec is None:
        assert end == (0, -1, -1)
        return end, rec
    ra, rb, columns = T.columns_of(end, rec)
    assert ra == rb >= 1 and columns == len(cols) and cols[0] == "M" and cols[-1] == "M", (a, b, rec, cols)
    assert 0 <= rec[0] <= end[1] and 0 <= rec[1] <= end[2] and 0 <= rec[2] <= rec[3] + cols.count("M") and rec[3] <= ra
    # the piece the path covers scores what the whole pair scores, and its own path is the same path
    pa, pb = a[rec[0]:end[1] + 1], b[rec[1]:end[2] + 1]
    sub_end, sub_rec = T.trace_numpy(pa, pb, S_, go, ge)
    assert sub_end[0] == end[0] and A.sw_numpy(pa, pb, S_, min(go, T.GAP_CAP), min(ge, T.GAP_CAP))[0] == end[0], (a, b, rec)
    # with the box known, the box's tables give the same record (what the device computes)
    assert T.trace_numpy(a, b, S_, go, ge, end=end) == (end, rec) == T.trace_loops(a, b, S_, go, ge, end=end)
    return end, rec


# ---- the two forms ----------------------------------------------------------------------------------------------------------

def test_loops_against_numpy_on_random_pairs_with_common_ties():
    rng = np.random.default_rng(31)
    ties, traced, gapped, empty = {}, 0, 0, 0
    for k in range(300):
        la, lb = int(rng.integers(0, 61)), int(rng.integers(0, 61))
        letters = (b"ACX", b"ACDX", b"ACDEFGHIKLX")[k % 3]              # few letters: equal scores, so ties, are common
        a = bytes(rng.choice(list(letters), la).tolist())
        b = bytes(rng.choice(list(letters), lb).tolist())
        if k % 4 == 0 and la > 12:                                      # a relative with a deletion: a gap on the path
            cut = int(rng.integers(1, 4))
            b = a[:la // 2] + a[la // 2 + cut:]
        S_, go, ge = ((A.S62, 11, 1), (M23, 5, 2), (M23, 0, 1), (A.S62, 0, 1), (M23, 0, 2))[k % 5]
        end, rec = _check(a, b, S_, go, ge, ties)
        traced += rec is not None
        gapped += rec is not None and rec[4] > 0
        empty += la == 0 or lb == 0
    assert traced > 250 and gapped > 60 and empty >= 3
    # every kind of tie on many paths, not on a few
    assert min(ties.get(k, 0) for k in ("diagonal = E", "diagonal = F", "E = F", "E open = extend", "F open = extend")) >= 20, ties
    assert ties.get("all three", 0) >= 3, ties


# ---- known answers ------------------------------------------------------------------------------------------------------------

def test_a_protein_against_itself():
    p = M.random_protein(np.random.default_rng(32), 50)
    end, rec = _check(p, p, A.S62, 11, 1)
    assert end == (A.self_score(p), 49, 49) and rec == (0, 0, 50, 50, 0, 0, 0)


def test_one_substitution():
    """W for the residue in the middle of 41 (A when it is W): every pair of the diagonal stays on the path, one is not identical;
    W against anything else is negative in BLOSUM62, so it is not positive either."""
    p = M.random_protein(np.random.default_rng(33), 41)
    x = bytearray(p)
    x[20] = ord("A") if x[20] == ord("W") else ord("W")
    end, rec = _check(p, bytes(x), A.S62, 11, 1)
    assert (end[1], end[2]) == (40, 40) and rec == (0, 0, 40, 40, 0, 0, 0)


@pytest.mark.parametrize("cut", [1, 3, 10])
def test_a_deletion_in_the_middle(cut):
    """b is a without `cut` residues of its middle.  Thirty residues on either side score well over a hundred each, a gap of ten
    costs 21: one gap.  a's extra residues face nothing: columns (a_i, -), counted in gap_cols_b.  Swapped, gap_cols_a."""
    a = M.random_protein(np.random.default_rng(34), 70)
    b = a[:30] + a[30 + cut:]
    end, rec = _check(a, b, A.S62, 11, 1)
    assert end == (A.self_score(b) - 11 - cut, 69, 69 - cut) and rec == (0, 0, 70 - cut, 70 - cut, 1, 0, cut)
    end, rec = _check(b, a, A.S62, 11, 1)
    assert end == (A.self_score(b) - 11 - cut, 69 - cut, 69) and rec == (0, 0, 70 - cut, 70 - cut, 1, cut, 0)


def test_all_x_has_no_path():
    assert _check(b"X" * 12, b"X" * 9, A.S62, 11, 1) == ((0, -1, -1), None)
    assert _check(b"", b"ACD", A.S62, 11, 1) == ((0, -1, -1), None)
    seq, off = S.batch([b"X" * 12, b"X" * 9])
    aln = A.align_model(seq, off, [(0, 1)])
    assert T.paths_model(seq, off, [(0, 1)], aln).tolist() == [T.NO_PATH + (N.PATH_NONE,)]


def test_the_diagonal_is_preferred_to_e():
    """a = ACAA (rows), b = ACCAA (columns), +2 / -3, a gap of k costs 2k.
        H      A  C  C  A  A
           A   2  0  0  2  2
           C   0  4  2  0  0        H[2][3] = 2 both ways: H[1][2] + S[C][C] = 0 + 2 and E[2][3] = H[2][2] - 2
           A   2  0  1  4  2
           A   2  0  0  3  6
    From (4, 5): (A, A), (A, A), then (2, 3) with the tie.  The diagonal wins: (C, C), and (1, 2) has H = 0, so the path starts
    at (2, 3) = 0-based (1, 2) with three columns.  E first would give (-, C), (C, C), (A, A) as well: start (0, 0), a gap."""
    ties = {}
    end, rec = _check(b"ACAA", b"ACCAA", M23, 0, 2, ties)
    assert end == (6, 3, 4) and rec == (1, 2, 3, 3, 0, 0, 0) and ties == {"diagonal = E": 1}


def test_the_diagonal_is_preferred_to_f():
    """The case above transposed."""
    ties = {}
    end, rec = _check(b"ACCAA", b"ACAA", M23, 0, 2, ties)
    assert end == (6, 4, 3) and rec == (2, 1, 3, 3, 0, 0, 0) and ties == {"diagonal = F": 1}


def test_e_is_preferred_to_f():
    """a = ACD (rows), b = CAD (columns), +2 / -3, a gap of k costs k.
        H      C  A  D
           A   0  2  1
           C   2  1  0        H[2][2] = 1 both ways: E[2][2] = H[2][1] - 1 and F[2][2] = H[1][2] - 1; the diagonal gives -3
           D   0  0  3
    From (3, 3): (D, D), then (2, 2) with the tie.  E wins: (-, A), opened from H[2][1] = 2, which is (C, C) from the boundary:
    start (2, 1) = 0-based (1, 0), one gap column of kind (-, b_j).  F first would give (C, -) and (A, A): start (0, 1)."""
    ties = {}
    end, rec = _check(b"ACD", b"CAD", M23, 0, 1, ties)
    assert end == (3, 2, 2) and rec == (1, 0, 2, 2, 1, 1, 0) and ties == {"E = F": 1}


def test_all_three_equal():
    """a = CACDAACC, b = CADCCAAC, +2 / -3, a gap of k costs 1 + k.  The path is
            a  C A - C D A A C
            b  C A D C C A A C        six identical pairs, D against C, one gap of one: 12 - 3 - 2 = 7
    and at the cell of (D, C) the diagonal, E and F all give H: the diagonal is taken."""
    ties = {}
    end, rec = _check(b"CACDAACC", b"CADCCAAC", M23, 1, 1, ties)
    assert end == (7, 6, 7) and rec == (0, 0, 6, 6, 1, 1, 0) and ties == {"all three": 1}


def test_an_opening_is_preferred_to_an_extension():
    """a = AAAA, b = AACCAA, +2 / -3, gap_open = 0 and a gap of k costs k: H[2][3] = 3 = E[2][3], H[2][4] = 2 = E[2][4], and
    E[2][4] is both E[2][3] - 1 and H[2][3] - 0 - 1.  The opening wins: the walk passes through state H at (2, 3), which sends
    it on into E.  The two columns (-, C) are one run: one opening, counted from the column string.  Transposed for F."""
    ties = {}
    end, rec, cols = T.trace_loops(b"AAAA", b"AACCAA", M23, 0, 1, with_columns=True, ties=ties)
    assert _check(b"AAAA", b"AACCAA", M23, 0, 1) == (end, rec)
    assert end == (6, 3, 5) and rec == (0, 0, 4, 4, 1, 2, 0) and cols == "MMEEMM" and ties == {"E open = extend": 1}
    ties = {}
    end, rec, cols = T.trace_loops(b"AACCAA", b"AAAA", M23, 0, 1, with_columns=True, ties=ties)
    assert _check(b"AACCAA", b"AAAA", M23, 0, 1) == (end, rec)
    assert end == (6, 5, 3) and rec == (0, 0, 4, 4, 1, 0, 2) and cols == "MMFFMM" and ties == {"F open = extend": 1}


def test_gap_costs_are_the_capped_ones():
    """2^31 - 1 is capped at 2^29 as the kernel caps it: no gap pays, the path is the best diagonal run."""
    big = (1 << 31) - 1
    p = M.random_protein(np.random.default_rng(35), 30)
    end, rec = _check(p, p[:15] + p[16:], A.S62, big, big)
    assert rec[4:] == (0, 0, 0)


def test_max_trace_cells_at_the_box_and_one_below():
    rng = np.random.default_rng(36)
    p = M.random_protein(rng, 40)
    seq, off = S.batch([p, p[:25] + M.random_protein(rng, 9)])
    aln = A.align_model(seq, off, [(0, 1), (1, 0), (0, 0)])
    assert (aln["end_a"][0], aln["end_b"][0]) == (24, 24)
    at = T.paths_model(seq, off, [(0, 1), (1, 0), (0, 0)], aln, max_trace_cells=625)
    below = T.paths_model(seq, off, [(0, 1), (1, 0), (0, 0)], aln, max_trace_cells=624)
    assert at["status"].tolist() == [N.PATH_TRACED, N.PATH_TRACED, N.PATH_UNTRACED]
    assert below["status"].tolist() == [N.PATH_UNTRACED] * 3 and below[0].tolist() == T.NO_PATH + (N.PATH_UNTRACED,)
    assert at[0].tolist() == (0, 0, 25, 25, 0, 0, 0, N.PATH_TRACED)
    # a pair the alignment skipped has no path
    skipped = A.align_model(seq, off, [(0, 1)], max_cells=100)
    assert T.paths_model(seq, off, [(0, 1)], skipped).tolist() == [T.NO_PATH + (N.PATH_NONE,)]


# ---- layouts -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,jname,py", [("kg_alignment_path", "KgAlignmentPath", N.ALIGN_PATH_DTYPE), ("kg_trace_stats", "KgTraceStats", N.KgTraceStats)])
def test_jna_structures_match_the_c_layout(cname, jname, py):
    width = {"int32_t": "int", "uint32_t": "int", "int64_t": "long", "float": "float"}
    cf = H._c_struct(cname)
    jf, order = H._java_struct(jname)
    assert [n for n, _ in jf] == [n for n, _ in cf] == order
    assert [t for _, t in jf] == [width[t] for _, t in cf]
    names = list(py.names) if isinstance(py, np.dtype) else [n for n, _ in py._fields_]
    assert names == [n for n, _ in cf]


def test_dtypes_match_gcc_layout_and_old_structures_keep_their_sizes(tmp_path):
    sn = [n for n, _ in N.KgTraceStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(kg_alignment_path), sizeof(kg_trace_stats), sizeof(kg_alignment), '
                   'sizeof(kg_align_params), sizeof(kg_search_hit), sizeof(kg_search_params), sizeof(kg_search_stats));\n' +
                   'printf("%d %d %lld\\n", KG_TRACE_HITS, KG_TRACE_ALL, (long long)KG_TRACE_DEFAULT_MAX_CELLS);\n' +
                   "".join('printf("%%zu\\n", offsetof(kg_alignment_path, %s));\n' % f for f in N.ALIGN_PATH_DTYPE.names) +
                   "".join('printf("%%zu\\n", offsetof(kg_trace_stats, %s));\n' % f for f in sn) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:7] == [32, C.sizeof(N.KgTraceStats), 24, 40, 40, 16, 136] and C.sizeof(N.KgTraceStats) == 32
    assert out[7:10] == [N.TRACE_HITS, N.TRACE_ALL, N.TRACE_DEFAULT_MAX_CELLS] == [1, 2, 1 << 24]
    assert out[10:] == ([N.ALIGN_PATH_DTYPE.fields[f][1] for f in N.ALIGN_PATH_DTYPE.names] + [getattr(N.KgTraceStats, f).offset for f in sn])
    assert {"kg_proteins_align_paths", "kg_proteins_align_paths_device", "kg_proteins_search_paths", "kg_proteins_search_paths_device",
            "kg_hitset_paths_copy", "kg_hitset_trace_stats"} <= set(N.EXPORTS)


def test_the_constants_of_the_kernel_and_the_documents():
    text = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_trace.hpp")).read()
    assert int(re.search(r"constexpr int kTraceCellBits = (\d+);", text).group(1)) == 4
    assert int(re.search(r"constexpr int kTraceCellsPerWord = (\d+);", text).group(1)) == 8
    assert "asm" not in re.sub(r"//[^\n]*", "", text)
    hdr = open(os.path.join(ROOT, "include", "kmerguts_hip.h")).read()
    for words in ("If H[i][j] == H[i-1][j-1] + S[a_i][b_j]: emit the column (a_i, b_j) and step to (i-1, j-1).",
                  "If E[i][j] == H[i][j-1] - open - ext: go to state H at (i, j-1).",
                  "If F[i][j] == H[i-1][j] - open - ext: go to state H at (i-1, j).", "The preference order is diagonal, then E, then F."):
        assert words in hdr, words
    for name in ("README.md", "DESIGN.md"):
        doc = open(os.path.join(ROOT, name)).read()
        assert "kg_proteins_search_paths" in doc and "--paths" in doc, name
    assert "9r" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- the front end ----------------------------------------------------------------------------------------------------------

def _model_search(seq, offsets, n_db, min_shared=2, max_cand=8, max_db_per_kmer=256, align=None, device=0, paths=None,
                  max_trace_cells=N.TRACE_DEFAULT_MAX_CELLS):
    kw = dict(min_shared=min_shared, max_cand=max_cand, max_db_per_kmer=max_db_per_kmer, **(align or {}))
    if paths is None:
        return S.search_model(seq, offsets, n_db, **kw)
    hits, start, recs, counts = T.search_paths_model(seq, offsets, n_db, paths, max_trace_cells, **kw)
    return hits, start, recs, dict(counts, ms_trace=0.25)


def _fasta(path, ids, seqs):
    path.write_bytes(b"".join(b">%s some words\n%s\n" % (i, s) for i, s in zip(ids, seqs)))
    return str(path)


def test_front_end_path_fields_and_flags_off(tmp_path):
    from kmergutsjava_amd import search_proteins as SP
    rng = np.random.default_rng(37)
    a, b, c = (M.random_protein(rng, 60) for _ in range(3))
    a_del = a[5:30] + a[33:]                             # a without its first five residues and three of its middle
    b_half = b[:20] + M.random_protein(rng, 30)          # shares 8-mers with b, scores under half of it
    db = _fasta(tmp_path / "db.faa", [b"dA", b"dB", b"dC"], [a, b, c])
    qs = _fasta(tmp_path / "q.faa", [b"q1", b"q2", b"q3", b"q4"], [a_del, b, b_half, M.random_protein(rng, 40)])
    (tmp_path / "ann.tsv").write_bytes(b"dA\tkinase\tE\ndB\tligase\n")
    out, old = str(tmp_path / "hits.tsv"), str(tmp_path / "old.tsv")
    ann = str(tmp_path / "ann.tsv")
    # flags off: the line and the file in the old format, written out here; q1 shares the 18 windows inside its first 25 residues
    # and the 19 counted windows of its last 27 (that no other byte of the old output moved rests on
    # tests/test_search_host.py, which this change leaves as it was)
    line_old = SP.search_proteins([db], [qs], old, annotations=ann, write_all=True, search=_model_search)
    sb = A.self_score(b)
    q1 = T.trace_numpy(a_del, a)[0]
    q3 = A.sw_numpy(b_half, b)
    assert open(old, "rb").read() == (
        b"q1\t0\tdA\t%d\t%d\t%d\t%d\t52\t60\thit\tkinase\n" % ((25 - 8 + 1) + (27 - 8), q1[0], A.self_score(a), 100 * q1[0] // A.self_score(a)) +
        b"q2\t0\tdB\t52\t%d\t%d\t100\t60\t60\thit\tligase\n" % (sb, sb) +
        b"q3\t0\tdB\t13\t%d\t%d\t%d\t%d\t%d\tbelow\tligase\n" % (q3[0], sb, 100 * q3[0] // sb, q3[1] + 1, q3[2] + 1))
    assert line_old.startswith("Queries: 4, targets: 3, candidates: 3, aligned: 3, hits: 2, queries hit: 2, transferred: 2, masked k-mers: 0, ms: encode ")
    assert line_old.endswith(", total 0.000") and "traced" not in line_old
    # --paths, hits only
    line = SP.search_proteins([db], [qs], out, annotations=ann, write_all=True, search=_model_search, paths="hits")
    rows = [r.split(b"\t") for r in open(out, "rb").read().splitlines()]
    olds = [r.split(b"\t") for r in open(old, "rb").read().splitlines()]
    assert [r[:10] + r[20:] for r in rows] == olds and all(len(r) == 21 for r in rows)
    assert [(r[0], r[2], r[9], r[20]) for r in rows] == [(b"q1", b"dA", b"hit", b"kinase"), (b"q2", b"dB", b"hit", b"ligase"), (b"q3", b"dB", b"below", b"ligase")]
    # q1: a_del[0] is a[5]; 52 residue columns and a gap of three in the query's row: columns (-, b_j); 52 of 55 columns identical;
    # the query is covered whole, the target from its sixth residue on: 55 of 60
    assert rows[0][10:20] == [b"1", b"6", b"55", b"52", b"94", b"52", b"1", b"3", b"100", b"91"]
    assert rows[1][10:20] == [b"1", b"1", b"60", b"60", b"100", b"60", b"0", b"0", b"100", b"100"]
    assert rows[2][10:20] == [b"-"] * 10                 # below the ratio: not traced with --trace hits
    assert line == line_old + ", traced: 2, untraced: 0, trace ms: 0.250"
    # --trace all traces the record below the ratio; a cap under the boxes leaves every field `-` and counts the records
    SP.search_proteins([db], [qs], out, write_all=True, search=_model_search, paths="all")
    rows = [r.split(b"\t") for r in open(out, "rb").read().splitlines()]
    assert all(len(r) == 20 for r in rows) and rows[2][10:12] == [b"1", b"1"] and rows[2][13] == b"20" and rows[2][18] != b"-"
    line = SP.search_proteins([db], [qs], out, write_all=True, search=_model_search, paths="all", max_trace_cells=100)
    assert line.endswith(", traced: 0, untraced: 3, trace ms: 0.250")
    assert all(r.split(b"\t")[10:] == [b"-"] * 10 for r in open(out, "rb").read().splitlines())
    with pytest.raises(ValueError, match="--trace"):
        SP.search_proteins([db], [qs], out, search=_model_search, paths="some")


def test_front_end_flag_defaults(tmp_path, monkeypatch):
    """--trace defaults to hits, with --all to all; --trace and --max-trace-cells need --paths."""
    from kmergutsjava_amd import search_proteins as SP
    seen = []

    def fake(database, queries, out, *args, **kw):
        seen.append((kw.get("paths"), kw.get("max_trace_cells")))
        return "line"

    monkeypatch.setattr(SP, "search_proteins", fake)
    base = ["-d", "d.faa", "-q", "q.faa", "-o", str(tmp_path / "o.tsv")]
    for extra in ([], ["--paths"], ["--paths", "--all"], ["--paths", "--all", "--trace", "hits"], ["--paths", "--trace", "all", "--max-trace-cells", "4096"]):
        assert SP.main(base + extra) == 0
    assert seen == [(None, None), ("hits", None), ("all", None), ("hits", None), ("all", 4096)]
    for extra in (["--trace", "all"], ["--max-trace-cells", "9"]):
        with pytest.raises(SystemExit):
            SP.main(base + extra)
