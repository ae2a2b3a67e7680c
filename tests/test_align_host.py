"""The alignment rule (include/kmerguts_hip.h, kg_proteins_align) on the host: the typing of the score table, the two forms of
tests/align_model.py against each other and against answers worked out by hand, the ratio test at its bound, the record
layouts against gcc and the JNA source, and the front end's writers with the device call replaced by the model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import align_model as A
import cluster_model as M
import test_java_binding as H
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import align_scores as AS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = A.S62


def _s(x: str, y: str) -> int:
    return int(S[AS.ALPHA.index(x.encode()), AS.ALPHA.index(y.encode())])


# ---- the table -------------------------------------------------------------------------------------------------------------

def test_blosum62_is_typed_right():
    assert AS.ALPHA == b"ACDEFGHIKLMNPQRSTVWY" == M.ALPHA and S.shape == (21, 21)
    assert (S == S.T).all()
    assert int(np.trace(S[:20, :20])) == 116
    want = dict(A=-16, R=-21, N=-18, D=-26, C=-31, Q=-12, E=-17, G=-34, H=-17, I=-27, L=-25, K=-17, M=-13, F=-25, P=-32, S=-11, T=-14,
                W=-32, Y=-16, V=-22)
    got = {chr(AS.ALPHA[i]): int(S[i, :20].sum()) for i in range(20)}
    assert got == want
    assert int(S[:20, :20].sum()) == -426
    assert (S[20] == -1).all() and (S[:, 20] == -1).all()
    assert S.min() >= -16 and S.max() <= 16
    # a few entries by letter: a permutation by position instead of by letter would move them
    assert (_s("W", "W"), _s("C", "C"), _s("A", "R"), _s("D", "E"), _s("F", "Y"), _s("I", "V"), _s("G", "I")) == (11, 9, -1, 2, 3, 3, -4)


def test_the_c_table_is_the_python_table():
    text = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_align.hpp")).read()
    body = re.search(r"kBlosum62\[21 \* 21\] = \{(.*?)\};", text, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    vals = [int(v) for v in re.findall(r"-?\d+", body)]
    assert vals == [int(v) for v in S.reshape(-1)]


# ---- the two forms -----------------------------------------------------------------------------------------------------------

def _random_seq(rng, length, x_rate=0.05):
    s = np.frombuffer(AS.ALPHA, dtype=np.uint8)[rng.integers(0, 20, size=length)].copy()
    s[rng.random(length) < x_rate] = ord("X")
    return s.tobytes()


def test_loops_against_numpy_on_random_pairs():
    rng = np.random.default_rng(1)
    n_pos = 0
    for k in range(300):
        a = _random_seq(rng, int(rng.integers(0, 61)))
        if k % 3 == 0:                                      # a relative: a mutated piece with an insertion
            cut = int(rng.integers(0, len(a) + 1))
            b = A.mutate(rng, a[:cut], 0.2) + _random_seq(rng, int(rng.integers(0, 6))) + A.mutate(rng, a[cut:], 0.2)
        else:
            b = _random_seq(rng, int(rng.integers(0, 61)))
        go, ge = [(11, 1), (5, 2), (0, 1), (3, 3)][k % 4]
        want = A.sw_loops(a, b, S, go, ge)
        assert A.sw_numpy(a, b, S, go, ge) == want, (a, b, go, ge)
        n_pos += want[0] > 0
    assert n_pos > 200


# ---- known answers -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def prot():
    return M.random_protein(np.random.default_rng(2), 200)


def test_a_protein_against_itself(prot):
    for p in (prot, prot[:1], prot[:64]):
        assert A.sw_loops(p, p) == (A.self_score(p), len(p) - 1, len(p) - 1) == A.sw_numpy(p, p)
    # X aside: X against X scores -1.  The leading A is worth the two X behind it (4 - 2 > 0), the trailing X only loses
    p = b"AXXA" + prot[:30] + b"X"
    assert A.sw_loops(p, p) == (A.self_score(p) - 2, len(p) - 2, len(p) - 2) == A.sw_numpy(p, p)


def test_symmetry():
    rng = np.random.default_rng(3)
    for _ in range(30):
        a, b = _random_seq(rng, int(rng.integers(1, 50))), _random_seq(rng, int(rng.integers(1, 50)))
        assert A.sw_loops(a, b)[0] == A.sw_loops(b, a)[0]


def test_one_substitution(prot):
    p = prot[:40]
    x = chr(p[20])
    for y in "ACW":
        if y == x:
            continue
        q = p[:20] + y.encode() + p[21:]
        assert A.sw_loops(p, q)[0] == A.self_score(p) - _s(x, x) + _s(x, y)


@pytest.mark.parametrize("k", [1, 3, 10])
def test_a_deletion_in_the_middle(prot, k):
    short = prot[:100] + prot[100 + k:]
    assert A.sw_loops(prot, short)[0] == A.self_score(short) - (11 + k) == A.sw_numpy(short, prot)[0]


@pytest.mark.parametrize("k", [1, 3, 10])
def test_a_deletion_near_an_end_gives_the_longer_flank(prot, k):
    """The flank alone is the answer when the 5 residues in front of the gap score less than the gap costs.  Five residues score
    at least 20 (the smallest diagonal entry is 4), more than a gap of 1 or 3, so the head here has two X: 4 + 4 - 1 - 1 + 4 = 10.
    With a head that pays for the gap the answer is the alignment through it."""
    weak = b"ASXXA" + prot[5:]
    short = weak[:5] + weak[5 + k:]
    assert A.sw_loops(weak[:5], weak[:5])[0] == 10 < 11 + k
    assert A.sw_loops(weak, short) == (A.self_score(prot[5 + k:]), 199, 199 - k) == A.sw_numpy(weak, short)
    short = prot[:5] + prot[5 + k:]
    head, flank = A.self_score(prot[:5]), A.self_score(prot[5 + k:])
    assert A.sw_loops(prot, short)[0] == max(flank, flank + head - (11 + k)) == A.sw_numpy(prot, short)[0]


def test_all_x_scores_nothing(prot):
    for other in (prot[:30], b"XXXX", b""):
        assert A.sw_loops(b"XXXXXXXX", other) == (0, -1, -1) == A.sw_numpy(other, b"XXXXXXXX")
    assert A.self_score(b"XXXX") == 0 and A.self_score(b"AXW") == 15


def test_two_equal_maxima_give_the_first_end():
    assert A.sw_loops(b"WWWW", b"WWWWAAAAWWWW") == (44, 3, 3) == A.sw_numpy(b"WWWW", b"WWWWAAAAWWWW")
    assert A.sw_loops(b"WWWWAAAAWWWW", b"WWWW") == (44, 3, 3) == A.sw_numpy(b"WWWWAAAAWWWW", b"WWWW")
    # the same score in a later row but an earlier column: the smaller i wins
    a, b = b"WY" + b"DDDDDD" + b"YW", b"YW" + b"LLLL" + b"WY"
    assert A.sw_loops(a, b) == (18, 1, 7) == A.sw_numpy(a, b) and A.sw_loops(a[8:], b[:2]) == (18, 1, 1)


def test_the_ratio_test_at_its_bound():
    assert A.kept(50, 100, 50) and not A.kept(49, 100, 50)
    assert A.kept(1, 2, 50) and not A.kept(0, 0, 0)         # score >= 1 whatever the percentage
    assert A.kept(33, 100, 33) and not A.kept(32, 100, 33)
    assert A.kept(2 ** 30, 2 ** 31 - 1, 50)                 # 100 * score needs 64 bits
    # the model's cut uses it: a pair exactly at 50 % with a custom matrix (+2 / -3): 10 of 20 residues match
    mat = np.full((21, 21), -3, dtype=np.int64)
    np.fill_diagonal(mat, 2)
    a, b = b"ACDEFGHIKL" + b"MMMMMMMMMM", b"ACDEFGHIKL" + b"WWWWWWWWWW"
    assert A.sw_loops(a, b, mat, 5, 2)[0] == 20 and A.self_score(a, mat) == 40
    assert A.kept(20, 40, 50) and not A.kept(20, 40, 51)


# ---- layouts -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,jname,py", [("kg_alignment", "KgAlignment", N.ALIGNMENT_DTYPE), ("kg_family_edge", "KgFamilyEdge", N.FAMILY_EDGE_DTYPE),
                                            ("kg_align_stats", "KgAlignStats", N.KgAlignStats)])
def test_jna_structures_match_the_c_layout(cname, jname, py):
    width = {"int32_t": "int", "uint32_t": "int", "int64_t": "long", "float": "float"}
    cf = H._c_struct(cname)
    jf, order = H._java_struct(jname)
    assert [n for n, _ in jf] == [n for n, _ in cf] == order
    assert [t for _, t in jf] == [width[t] for _, t in cf]
    names = list(py.names) if isinstance(py, np.dtype) else [n for n, _ in py._fields_]
    assert names == [n for n, _ in cf]


def test_the_parameter_structure_with_its_pointer():
    want = ["min_ratio_pct", "ref", "gap_open", "gap_extend", "max_cells", "matrix", "reserved"]
    assert [n for n, _ in N.KgAlignParams._fields_] == want
    j = H._strip_comments(H.JAVA)
    body = re.search(r"class KgAlignParams extends Structure \{(.*?)\n    \}", j, flags=re.S).group(1)
    assert re.findall(r'"([a-z_0-9]+)"', re.search(r"setFieldOrder\(new String\[\]\s*\{(.*?)\}\)", body, flags=re.S).group(1)) == want
    assert re.search(r"public\s+Pointer\s+matrix;", body) and re.search(r"public\s+long\s+max_cells;", body)


def test_dtypes_match_gcc_layout(tmp_path):
    pn, sn = [n for n, _ in N.KgAlignParams._fields_], [n for n, _ in N.KgAlignStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(kg_alignment), sizeof(kg_family_edge), sizeof(kg_align_params), '
                   'sizeof(kg_align_stats), sizeof(kg_cluster_params), sizeof(kg_family));\n' +
                   "".join('printf("%%zu\\n", offsetof(kg_alignment, %s));\n' % f for f in N.ALIGNMENT_DTYPE.names) +
                   "".join('printf("%%zu\\n", offsetof(kg_family_edge, %s));\n' % f for f in N.FAMILY_EDGE_DTYPE.names) +
                   "".join('printf("%%zu\\n", offsetof(kg_align_params, %s));\n' % f for f in pn) +
                   "".join('printf("%%zu\\n", offsetof(kg_align_stats, %s));\n' % f for f in sn) +
                   'printf("%d %d %lld\\n", KG_ALIGN_REF_LONGER, KG_ALIGN_REF_MEMBER, (long long)KG_ALIGN_DEFAULT_MAX_CELLS);\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:6] == [24, 32, C.sizeof(N.KgAlignParams), C.sizeof(N.KgAlignStats), 12, 16] and out[2:4] == [40, 40]
    assert out[6:-3] == ([N.ALIGNMENT_DTYPE.fields[f][1] for f in N.ALIGNMENT_DTYPE.names] +
                         [N.FAMILY_EDGE_DTYPE.fields[f][1] for f in N.FAMILY_EDGE_DTYPE.names] +
                         [getattr(N.KgAlignParams, f).offset for f in pn] + [getattr(N.KgAlignStats, f).offset for f in sn])
    assert out[-3:] == [N.ALIGN_REF_LONGER, N.ALIGN_REF_MEMBER, N.ALIGN_DEFAULT_MAX_CELLS]


def test_the_documents_name_the_step():
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "kg_proteins_cluster_aligned" in text or "--align" in text, name
    hdr = open(os.path.join(ROOT, "include", "kmerguts_hip.h")).read()
    assert hdr.count("Known weakness") == 1 and "kg_proteins_cluster_aligned" in hdr.split("Known weakness")[1][:400]


# ---- the model of the aligned clustering, and the front end -------------------------------------------------------------------------

def test_the_domain_chain_in_the_model():
    prots = A.domain_chain(np.random.default_rng(5))
    seq, off = M.pack(prots)
    plain, counts = M.cluster_loops(seq, off)
    assert counts["families"] == 1 and counts["edges"] == 2
    rec, counts, edges, st = A.cluster_aligned_model(seq, off)
    assert counts["families"] == 3 and counts["edges"] == 0 and (rec["best"] == -1).all() and (rec["shared"] == 0).all()
    assert edges["status"].tolist() == [N.EDGE_CUT, N.EDGE_CUT] and st == dict(aligned=2, cut=2, skipped=0, cells=2 * 120 * 270)
    assert edges["member"].tolist() == [1, 2] and edges["centre"].tolist() == [0, 0] and (edges["shared"] >= 5).all()
    for e in edges:                                         # clearly under 50 against the longer, well over against the member's
        own = A.self_score(prots[int(e["member"])])
        assert 100 * int(e["score"]) < 45 * int(e["ref"]) and 100 * int(e["score"]) > 80 * own and int(e["ref"]) == A.self_score(prots[0])
    rec, counts, edges, st = A.cluster_aligned_model(seq, off, ref="member")
    assert counts["families"] == 1 and st["cut"] == 0 and rec.tobytes() == plain.tobytes()


def _aligned_model(seq, offsets, min_shared=5, min_cover_pct=20, device=0, align=None):
    rec, counts, edges, st = A.cluster_aligned_model(seq, offsets, min_shared, min_cover_pct, **(align or {}))
    return rec, dict(counts, rounds=1, ms_total=0.0, edge_records=edges, align=dict(st, ms_align=0.0))


def _plain_model(seq, offsets, min_shared=5, min_cover_pct=20, device=0):
    rec, counts = M.cluster_numpy(seq, offsets, min_shared, min_cover_pct)
    return rec, dict(counts, rounds=1, ms_total=0.0)


def test_front_end_writers(tmp_path, capsys):
    from kmergutsjava_amd import cluster_proteins as CP
    prots = A.domain_chain(np.random.default_rng(5))
    copy = A.mutate(np.random.default_rng(6), prots[0], 0.05)
    faa = tmp_path / "p.faa"
    faa.write_bytes(b"".join(b">%s\n%s\n" % (pid, s) for pid, s in zip((b"centre", b"dom_a", b"dom_b", b"copy"), prots + [copy])))
    out, edges = tmp_path / "families.tsv", tmp_path / "edges.tsv"
    # flags off: today's bytes and today's summary line
    line = CP.cluster_proteins([str(faa)], str(out), cluster=_plain_model)
    plain = out.read_bytes()
    assert all(len(r.split(b"\t")) == 6 for r in plain.splitlines()) and len(plain.splitlines()) == 4
    assert re.fullmatch(r"Proteins: 4, families: 1, multi: 1, largest: 4, edges: 3, rounds: 1, ms: [0-9.]+", line)
    # --align
    line = CP.cluster_proteins([str(faa)], str(out), cluster=_aligned_model, align={}, edges=str(edges))
    assert re.fullmatch(r"Proteins: 4, families: 3, multi: 1, largest: 2, edges: 1, rounds: 1, ms: [0-9.]+, aligned: 3, cut: 2, skipped: 0, "
                        r"align ms: [0-9.]+", line)
    rows = [r.split(b"\t") for r in out.read_bytes().splitlines()]
    seq, off = M.pack(prots + [copy])
    score = A.sw_loops(copy, prots[0])[0]
    ref = max(A.self_score(copy), A.self_score(prots[0]))
    assert [r[0] for r in rows] == [b"centre", b"copy"] and all(len(r) == 8 for r in rows)
    assert rows[0][4:] == [b"-", b"0", b"-", b"-"] and rows[1][4] == b"centre" and rows[1][6:] == [b"%d" % score, b"%d" % (100 * score // ref)]
    erows = [r.split(b"\t") for r in edges.read_bytes().splitlines()]
    assert [(r[0], r[1], r[8]) for r in erows] == [(b"dom_a", b"centre", b"cut"), (b"dom_b", b"centre", b"cut"), (b"copy", b"centre", b"kept")]
    assert all(len(r) == 9 for r in erows)
    assert erows[2][2:8] == [rows[1][5], b"%d" % score, b"%d" % ref, b"%d" % (100 * score // ref), b"%d" % len(copy), b"%d" % len(prots[0])]
    end = A.sw_loops(prots[1], prots[0])
    assert erows[0][3] == b"%d" % end[0] and erows[0][6:8] == [b"%d" % (end[1] + 1), b"%d" % (end[2] + 1)]
    # a skipped pair: kept, no score
    CP.cluster_proteins([str(faa)], str(out), cluster=_aligned_model, align=dict(max_cells=120 * 270), edges=str(edges), write_all=True)
    erows = [r.split(b"\t") for r in edges.read_bytes().splitlines()]
    assert [r[8] for r in erows] == [b"cut", b"cut", b"skipped"] and erows[2][3:8] == [b"-1", b"%d" % ref, b"-", b"0", b"0"]
    assert out.read_bytes().splitlines()[3].split(b"\t")[4:] == [b"centre", rows[1][5], b"-", b"-"]
    # --edges needs --align; the command line passes the flags on
    with pytest.raises(ValueError):
        CP.cluster_proteins([str(faa)], str(out), cluster=_plain_model, edges=str(edges))
    assert CP.main(["-p", str(faa), "-o", str(out), "--edges", str(edges)]) == 1 and "--edges needs --align" in capsys.readouterr().err
