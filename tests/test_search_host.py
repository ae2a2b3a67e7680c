"""The search rule (include/kmerguts_hip.h, kg_proteins_search) on the host: the two forms of tests/search_model.py against each
other on random small batches and against answers worked out by hand, the record layouts against gcc and the JNA source, and
the front end's writers, --transfer and --truth with the device call replaced by the model."""
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
from kmergutsjava_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_seq(rng, n: int) -> bytes:
    """Residues of a two-letter alphabet (so that 8-mers repeat between proteins), one X in 40."""
    return bytes(b"X"[0] if x == 0 else b"AC"[int(x) % 2] for x in rng.integers(0, 40, n))


def _fields(hits, *names):
    return [tuple(int(h[n]) for n in names) for h in hits]


# ---- the two forms ----------------------------------------------------------------------------------------------------------

def test_loops_against_numpy_on_random_small_batches():
    rng = np.random.default_rng(11)
    n_shared = n_masked = n_empty_db = n_empty_q = 0
    for k in range(300):
        n = int(rng.integers(0, 9))
        n_db = int(rng.integers(0, n + 1))
        if k % 25 == 0:
            n_db = 0
        if k % 25 == 1:
            n_db = n
        prots = [_random_seq(rng, int(rng.integers(0, 31))) for _ in range(n)]
        if n >= 2 and k % 3 == 0:                       # a planted relative: the last protein repeats a piece of the first
            prots[-1] = prots[0][:20] + prots[-1][:8]
        seq, off = S.batch(prots)
        max_db = int(rng.integers(1, 4))
        a, ca = S.shared_loops(seq, off, n_db, max_db)
        b, cb = S.shared_numpy(seq, off, n_db, max_db)
        assert a == b and ca == cb, (k, prots, n_db, max_db)
        n_shared += len(a)
        n_masked += ca["kmers_masked"]
        n_empty_db += n_db == 0
        n_empty_q += n_db == n
        if k % 10 == 0:
            kw = dict(min_shared=int(rng.integers(1, 3)), max_cand=int(rng.integers(1, 4)), max_db_per_kmer=max_db)
            ha, sa, xa = S.search_model(seq, off, n_db, shared=S.shared_loops, sw=A.sw_loops, **kw)
            hb, sb, xb = S.search_model(seq, off, n_db, **kw)
            assert ha.tobytes() == hb.tobytes() and (sa == sb).all() and xa == xb
    assert n_shared > 50 and n_masked > 20 and n_empty_db >= 12 and n_empty_q >= 12


# ---- known answers ------------------------------------------------------------------------------------------------------------

def test_an_identical_protein_is_its_own_first_hit_at_ratio_100():
    rng = np.random.default_rng(12)
    p, other = M.random_protein(rng, 60), M.random_protein(rng, 60)
    seq, off = S.batch([other, p, p])
    hits, start, st = S.search_model(seq, off, 2)
    assert list(start) == [0, 1] and st["queries_hit"] == 1 and st["hits"] == 1
    h = hits[0]
    assert _fields(hits, "query", "target", "shared", "status", "rank") == [(0, 1, 52, N.SEARCH_HIT, 0)]
    assert h["score"] == h["self_query"] == h["self_target"] == A.self_score(p) and (h["end_query"], h["end_target"]) == (59, 59)


@pytest.mark.parametrize("min_shared", [1, 2, 3])
def test_the_shared_count_at_min_shared(min_shared):
    """Targets that share min_shared - 1, min_shared and min_shared + 1 of the query's planted 8-mers."""
    rng = np.random.default_rng(13)
    km = S.distinct_kmers(rng, 12)
    own = km[:6]
    targets = [S.protein_of(own[:min_shared - 1] + [km[6]]), S.protein_of(own[:min_shared] + [km[7]]),
               S.protein_of(own[:min_shared + 1] + [km[8]])]
    seq, off = S.batch(targets + [S.protein_of(own)])
    s_of, counts = S.shared_loops(seq, off, 3)
    assert s_of == {(0, d): s for d, s in ((0, min_shared - 1), (1, min_shared), (2, min_shared + 1)) if s}
    hits, start, st = S.search_model(seq, off, 3, min_shared=min_shared, min_ratio_pct=0)
    assert _fields(hits, "target", "shared") == [(2, min_shared + 1), (1, min_shared)] and st["candidates"] == 2


def test_the_mask_at_max_db_per_kmer_and_one_more():
    rng = np.random.default_rng(14)
    u, v, w = S.distinct_kmers(rng, 3)
    extra = S.distinct_kmers(rng, 4, avoid=(u, v, w))
    # u is in 3 targets, v in 4: with max_db_per_kmer = 3 v takes no part; w is the query's and target 0's alone
    targets = [S.protein_of([u, v, w]), S.protein_of([u, v, extra[0]]), S.protein_of([u, v, extra[1]]), S.protein_of([v, extra[2]])]
    seq, off = S.batch(targets + [S.protein_of([u, v, w])])
    for form in (S.shared_loops, S.shared_numpy):
        s3, c3 = form(seq, off, 4, 3)
        assert s3 == {(0, 0): 2, (0, 1): 1, (0, 2): 1} and c3["kmers_masked"] == 1 and c3["kmers_joined"] == 2 and c3["join_pairs"] == 4
        s4, c4 = form(seq, off, 4, 4)
        assert s4 == {(0, 0): 3, (0, 1): 2, (0, 2): 2, (0, 3): 1} and c4["kmers_masked"] == 0 and c4["join_pairs"] == 8
        s2, c2 = form(seq, off, 4, 2)
        assert s2 == {(0, 0): 1} and c2["kmers_masked"] == 2 and c2["join_pairs"] == 1


@pytest.mark.parametrize("n_cand", [2, 3, 4])
def test_the_cut_at_max_cand_keeps_the_smaller_targets(n_cand):
    """max_cand = 3 and 2, 3, 4 candidates that all share the same two 8-mers."""
    rng = np.random.default_rng(15)
    u, v = S.distinct_kmers(rng, 2)
    seq, off = S.batch([S.protein_of([u, v])] * n_cand + [S.protein_of([u, v])])
    hits, start, st = S.search_model(seq, off, n_cand, max_cand=3)
    assert st["candidates"] == n_cand and sorted(_fields(hits, "target")) == [(d,) for d in range(min(n_cand, 3))]


def test_the_ratio_test_at_its_bound():
    """+2 / -3 with 10 of 20 residues equal: score 20 against self-scores of 40; 100 * 20 == 50 * 40 is a hit, 51 is below."""
    mat = np.full((21, 21), -3, dtype=np.int64)
    np.fill_diagonal(mat, 2)
    a, b = b"ACDEFGHIKL" + b"MMMMMMMMMM", b"ACDEFGHIKL" + b"WWWWWWWWWW"
    seq, off = S.batch([b, a])
    kw = dict(matrix=mat, gap_open=5, gap_extend=2)
    at, _, _ = S.search_model(seq, off, 1, min_ratio_pct=50, **kw)
    over, _, _ = S.search_model(seq, off, 1, min_ratio_pct=51, **kw)
    assert _fields(at, "shared", "score", "self_query", "self_target", "status") == [(3, 20, 40, 40, N.SEARCH_HIT)]
    assert _fields(over, "score", "status") == [(20, N.SEARCH_BELOW)]
    # the query's own self-score as ref: a target twice as long does not lower the ratio
    seq, off = S.batch([b + b"W" * 20, a])
    longer, _, _ = S.search_model(seq, off, 1, min_ratio_pct=50, **kw)
    member, _, _ = S.search_model(seq, off, 1, min_ratio_pct=50, ref="member", **kw)
    assert _fields(longer, "score", "self_target", "status") == [(20, 80, N.SEARCH_BELOW)]
    assert _fields(member, "score", "status") == [(20, N.SEARCH_HIT)]


def test_the_output_order():
    """Larger score first whatever s; equal score: larger s; equal score and s: the smaller target."""
    rng = np.random.default_rng(16)
    p = M.random_protein(rng, 40)
    half = p[:20] + (b"W" if p[20:21] != b"W" else b"A") + M.random_protein(rng, 19)     # 13 shared 8-mers and a smaller score
    x = bytearray(p)
    x[20] = ord("W") if x[20] != ord("W") else ord("A") # one substitution in the middle: 8 windows lost
    x = bytes(x)
    seq, off = S.batch([half, x, p, x, p, p])
    hits, start, st = S.search_model(seq, off, 5, min_ratio_pct=0)
    assert _fields(hits, "target", "rank") == [(2, 0), (4, 1), (1, 2), (3, 3), (0, 4)]
    assert hits["score"][0] == hits["score"][1] > hits["score"][2] == hits["score"][3] > hits["score"][4]
    assert list(hits["shared"]) == [32, 32, 24, 24, 13]
    # the candidates are chosen by s, the records ordered by score: a target with more shared 8-mers and a smaller score
    rep = p[:16] + p[:16] + p[:16]                       # shares the 8 windows of p[:16] only ... and scores 16 residues
    many = M.random_protein(rng, 30)
    q = p[:16] + many
    t_long = p[:16] + b"X" + many[:9] + b"X" + many[10:19] + b"X" + many[20:]      # more 8-mers, broken by non-residues
    seq, off = S.batch([rep, t_long, q])
    hits, _, _ = S.search_model(seq, off, 2, min_ratio_pct=0)
    assert hits["shared"][0] > hits["shared"][1] or hits["score"][0] >= hits["score"][1]
    assert list(hits["rank"]) == [0, 1] and hits["score"][0] >= hits["score"][1]


def test_a_skipped_pair_is_last():
    rng = np.random.default_rng(17)
    p = M.random_protein(rng, 30)
    long_t = p + M.random_protein(rng, 40)               # 70 x 30 = 2100 cells: over the cap; it shares the most 8-mers
    seq, off = S.batch([long_t, p[:20] + (b"W" if p[20:21] != b"W" else b"A") + M.random_protein(rng, 9), p])
    hits, start, st = S.search_model(seq, off, 2, max_cells=1000, min_ratio_pct=0)
    assert _fields(hits, "target", "shared", "score", "end_query", "end_target", "status", "rank") == [
        (1, 13, int(hits["score"][0]), int(hits["end_query"][0]), int(hits["end_target"][0]), N.SEARCH_HIT, 0),
        (0, 22, -1, -1, -1, N.SEARCH_SKIPPED, 1)]
    assert st["skipped"] == 1 and st["aligned"] == 1 and st["cells"] == 900 and st["queries_hit"] == 1
    only, _, st = S.search_model(seq, off, 2, max_cells=100)
    assert list(only["status"]) == [N.SEARCH_SKIPPED] * 2 and list(only["target"]) == [0, 1] and st["queries_hit"] == 0


# ---- layouts -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,jname,py", [("kg_search_hit", "KgSearchHit", N.SEARCH_HIT_DTYPE), ("kg_search_params", "KgSearchParams", N.KgSearchParams),
                                            ("kg_search_stats", "KgSearchStats", N.KgSearchStats)])
def test_jna_structures_match_the_c_layout(cname, jname, py):
    width = {"int32_t": "int", "uint32_t": "int", "int64_t": "long", "float": "float"}
    cf = H._c_struct(cname)
    jf, order = H._java_struct(jname)
    assert [n for n, _ in jf] == [n for n, _ in cf] == order
    assert [t for _, t in jf] == [width[t] for _, t in cf]
    names = list(py.names) if isinstance(py, np.dtype) else [n for n, _ in py._fields_]
    assert names == [n for n, _ in cf]


def test_dtypes_match_gcc_layout(tmp_path):
    pn, sn = [n for n, _ in N.KgSearchParams._fields_], [n for n, _ in N.KgSearchStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%zu %zu %zu\\n", sizeof(kg_search_hit), sizeof(kg_search_params), sizeof(kg_search_stats));\n' +
                   "".join('printf("%%zu\\n", offsetof(kg_search_hit, %s));\n' % f for f in N.SEARCH_HIT_DTYPE.names) +
                   "".join('printf("%%zu\\n", offsetof(kg_search_params, %s));\n' % f for f in pn) +
                   "".join('printf("%%zu\\n", offsetof(kg_search_stats, %s));\n' % f for f in sn) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [40, C.sizeof(N.KgSearchParams), C.sizeof(N.KgSearchStats)] == [40, 16, 136]
    assert out[3:] == ([N.SEARCH_HIT_DTYPE.fields[f][1] for f in N.SEARCH_HIT_DTYPE.names] +
                       [getattr(N.KgSearchParams, f).offset for f in pn] + [getattr(N.KgSearchStats, f).offset for f in sn])


def test_the_constants_of_the_kernels():
    text = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_search.hpp")).read()
    assert int(re.search(r"constexpr int kSearchTile = (\d+);", text).group(1)) == N.SEARCH_TILE
    assert int(re.search(r"constexpr int kSearchMaxCand = (\d+);", text).group(1)) == N.SEARCH_MAX_CAND == 64
    assert S.STAT_KEYS == tuple(n for n, _ in N.KgSearchStats._fields_ if not n.startswith(("ms_", "reserved")))


def test_the_documents_name_the_step():
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "search_proteins" in text and "kg_proteins_search" in text, name


# ---- the front end ----------------------------------------------------------------------------------------------------------

def _model_search(seq, offsets, n_db, min_shared=2, max_cand=8, max_db_per_kmer=256, align=None, device=0):
    return S.search_model(seq, offsets, n_db, min_shared, max_cand, max_db_per_kmer, **(align or {}))


def _fasta(path, ids, seqs):
    path.write_bytes(b"".join(b">%s some words\n%s\n" % (i, s) for i, s in zip(ids, seqs)))
    return str(path)


def test_front_end_writers(tmp_path):
    from kmergutsjava_amd import search_proteins as SP
    rng = np.random.default_rng(18)
    a, b, c = (M.random_protein(rng, 50) for _ in range(3))
    a2 = A.mutate(np.random.default_rng(19), a, 0.05)
    b_half = b[:20] + M.random_protein(rng, 30)          # shares 8-mers with b, scores under half of it
    db = _fasta(tmp_path / "db.faa", [b"dA", b"dB", b"dC"], [a, b, c])
    qs = _fasta(tmp_path / "q.faa", [b"q1", b"dB", b"q3", b"q4", b"q5"], [a2, b, b_half, M.random_protein(rng, 40), c])
    (tmp_path / "ann.tsv").write_bytes(b"dA\tkinase\tE\ndB\tligase\n")
    (tmp_path / "truth.tsv").write_bytes(b"q1\tkinase\ndB\tkinase\nq4\tkinase\nq5\tkinase\n")
    out, tr = str(tmp_path / "hits.tsv"), str(tmp_path / "transfer.tsv")
    line = SP.search_proteins([db], [qs], out, annotations=str(tmp_path / "ann.tsv"), transfer=tr, truth=str(tmp_path / "truth.tsv"),
                              search=_model_search)
    rows = [r.split(b"\t") for r in open(out, "rb").read().splitlines()]
    sa, sb, sc = A.self_score(a), A.self_score(b), A.self_score(c)
    assert [(r[0], r[1], r[2], r[9], r[10]) for r in rows] == [(b"q1", b"0", b"dA", b"hit", b"kinase"), (b"dB", b"0", b"dB", b"hit", b"ligase"),
                                                              (b"q5", b"0", b"dC", b"hit", b"-")]
    assert rows[1][3:9] == [b"42", b"%d" % sb, b"%d" % sb, b"100", b"50", b"50"] and rows[2][4:7] == [b"%d" % sc, b"%d" % sc, b"100"]
    assert int(rows[0][5]) == max(sa, A.self_score(a2)) and int(rows[0][6]) == 100 * int(rows[0][4]) // int(rows[0][5])
    assert open(tr, "rb").read() == b"q1\tkinase\ndB\tligase\n"
    assert line.startswith("Queries: 5, targets: 3, candidates: 4, aligned: 4, hits: 3, queries hit: 3, transferred: 2, masked k-mers: 0, ms: ")
    assert line.endswith(", labelled: 4, agree: 1, disagree: 1, missed: 2")
    # make_signatures reads the transfer file
    from kmergutsjava_amd.make_signatures import parse_annotations
    assert parse_annotations(open(tr, "rb").read()) == {b"q1": (b"kinase", b""), b"dB": (b"ligase", b"")}
    # --all: the record below the ratio as well, with its status; no -A: no function field
    SP.search_proteins([db], [qs], out, write_all=True, search=_model_search)
    rows = [r.split(b"\t") for r in open(out, "rb").read().splitlines()]
    assert [(r[0], r[2], r[9]) for r in rows] == [(b"q1", b"dA", b"hit"), (b"dB", b"dB", b"hit"), (b"q3", b"dB", b"below"), (b"q5", b"dC", b"hit")]
    assert all(len(r) == 10 for r in rows)
    # the query's own self-score as ref
    SP.search_proteins([db], [qs], out, align=dict(ref="query"), write_all=True, search=_model_search)
    rows = [r.split(b"\t") for r in open(out, "rb").read().splitlines()]
    assert int(rows[0][5]) == A.self_score(a2)


def test_front_end_errors(tmp_path):
    from kmergutsjava_amd import search_proteins as SP
    from kmergutsjava_amd.make_signatures import InputError
    p = M.random_protein(np.random.default_rng(20), 30)
    db = _fasta(tmp_path / "db.faa", [b"x", b"y"], [p, p])
    db2 = _fasta(tmp_path / "db2.faa", [b"x"], [p])
    q = _fasta(tmp_path / "q.faa", [b"x"], [p])
    out = str(tmp_path / "o.tsv")
    with pytest.raises(InputError, match="duplicate protein id x"):
        SP.search_proteins([db, db2], [q], out, search=_model_search)
    with pytest.raises(InputError, match="duplicate protein id x"):
        SP.search_proteins([db], [q, q], out, search=_model_search)
    with pytest.raises(ValueError, match="--transfer needs -A"):
        SP.search_proteins([db], [q], out, transfer=out, search=_model_search)
    with pytest.raises(ValueError, match="--max-hits"):
        SP.search_proteins([db], [q], out, max_hits=0, search=_model_search)
    SP.search_proteins([db], [q], out, max_hits=2, search=_model_search)         # the same id on both sides is allowed
    assert [r.split(b"\t")[:3] for r in open(out, "rb").read().splitlines()] == [[b"x", b"0", b"x"], [b"x", b"1", b"y"]]
