"""The ungapped filter's two model forms against each other and against answers worked out by hand, u <= score against the
alignment model, the new structures against gcc's layout and the JNA source, and the front end's writers and option errors with
the device call replaced by the model.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import align_model as A
import mask_model as MM
import search_model as S
import seed_model as SD
import ungapped_model as UM
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import search_proteins as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = (SD.IDENTITY, [1])


def _random_batch(rng, small_alphabet: bool):
    """A few short proteins over few letters, so that seeds repeat inside a protein and between them; X and empty ones among them."""
    letters = np.frombuffer(b"ACDX" if small_alphabet else b"ACDEFGHIKLX", dtype=np.uint8)
    n = int(rng.integers(2, 7))
    prots = [letters[rng.integers(0, len(letters), int(rng.integers(0, 40)))].tobytes() for _ in range(n)]
    if rng.random() < 0.3:
        prots[int(rng.integers(0, n))] = b""
    return prots, int(rng.integers(0, n + 1))


# ---- the rule -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", range(4))
def test_the_two_forms_agree_on_random_small_batches(block):
    rng = np.random.default_rng(500 + block)
    seeds = [SD.EXACT, ONE, (SD.IDENTITY, [0b101]), (SD.REDUCED11, [0b1011, 0b11001])]
    seen = 0
    for k in range(80):
        prots, n_db = _random_batch(rng, small_alphabet=k % 2 == 0)
        seq, off = S.batch(prots)
        seed = seeds[k % len(seeds)]
        max_db = int(rng.integers(1, 4))
        a, b = UM.diagonals_loops(seq, off, n_db, seed, max_db), UM.diagonals_numpy(seq, off, n_db, seed, max_db)
        assert a == b
        shared, _ = SD.shared_numpy(seed)(seq, off, n_db, max_db)
        assert {qd: v[0] for qd, v in a.items()} == shared              # the sum of m over the diagonals is s
        for (q, d), (s, g, m) in a.items():
            qa, db = prots[n_db + q], prots[d]
            assert UM.ungapped_loops(qa, db, g) == UM.ungapped_numpy(qa, db, g) >= 0 and 1 <= m <= s
            assert UM.cells_of(len(qa), len(db), g) >= 2
            seen += 1
        x = UM.filtered_model(seq, off, n_db, seed=seed, min_shared=1, max_cand=2, max_db_per_kmer=max_db, min_ungapped=int(rng.integers(0, 12)))
        y = UM.filtered_model(seq, off, n_db, seed=seed, min_shared=1, max_cand=2, max_db_per_kmer=max_db, form="loops",
                              min_ungapped=0)
        assert x[4]["scored"] == y[4]["scored"] == x[3]["candidates"] == x[4]["dropped"] + x[4]["cut"] + len(x[0]) and x[4]["cells"] == y[4]["cells"]
        ok = x[0]["status"] != N.SEARCH_SKIPPED
        assert (x[2]["ungapped"][ok] <= x[0]["score"][ok]).all()         # an ungapped run is an alignment
    assert seen > 40


def test_hand_worked_first_position_tie_and_negative_diagonal():
    target, query = b"DDWDDWDDYDD", b"IIIIWIIYIII"
    seq, off = S.batch([target, query])
    assert UM.first_positions_loops(target, ONE)[A.codes(b"W")[0]] == 2          # W at 2 and 5: the first
    v, p, x = UM.first_positions_numpy(seq, off, ONE)
    assert {(int(a), int(b)): int(c) for a, b, c in zip(v, p, x)}[(int(A.codes(b"W")[0]), 0)] == 2
    # W: 4 - 2 = 2 and Y: 7 - 8 = -1, one seed each: the smaller diagonal
    assert UM.diagonals_loops(seq, off, 1, ONE) == UM.diagonals_numpy(seq, off, 1, ONE) == {(0, 0): (2, -1, 1)}
    # a seed's diagonal holds the seed's own match, so under BLOSUM62 and identity seeds no diagonal is all negative: the matrix
    # of -1 everywhere makes every run negative, and u = 0
    minus = np.full((21, 21), -1)
    assert UM.ungapped_loops(query, target, -1, minus) == UM.ungapped_numpy(query, target, -1, minus) == 0
    assert UM.ungapped_loops(query, target, -1) == UM.ungapped_numpy(query, target, -1) == 12      # W/W I/D I/D Y/Y: 11 - 3 - 3 + 7
    assert UM.ungapped_loops(query, target, 2) == 11                             # W/W alone, between negative cells
    assert UM.best_of([3, 3, -2, -2, 7]) == (5, -2, 2) and UM.best_of([0]) == (1, 0, 1)
    assert UM.cells_of(8, 8, -6) == 2 and UM.cells_of(8, 8, 7) == 1 and UM.cells_of(5, 9, 0) == 5 and UM.cells_of(3, 3, 3) == 0


def test_hand_worked_cut_order_and_threshold():
    cands = {(0, 5): (2, 0, 1, 40), (0, 3): (4, 0, 1, 40), (0, 9): (4, 0, 1, 40), (0, 1): (9, 0, 1, 39), (1, 2): (2, 0, 1, 7)}
    kept, dropped, n_cut = UM.cut(cands, 2, 0, 2)
    assert [c[0] for c in kept[0]] == [3, 9] and [c[0] for c in kept[1]] == [2] and (dropped, n_cut) == (0, 2)    # larger s, then smaller d
    kept, dropped, n_cut = UM.cut(cands, 2, 40, 8)
    assert [c[0] for c in kept[0]] == [3, 9, 5] and kept[1] == [] and (dropped, n_cut) == (2, 0)                  # u = 40 is kept at 40
    kept, dropped, n_cut = UM.cut(cands, 2, 41, 8)
    assert kept == [[], []] and dropped == 5                                                                       # ... and dropped at 41


def test_the_maximum_sum_run_by_hand():
    q, d = b"WWIWW", b"WWDWW"                      # 11 11 -3 11 11
    assert UM.ungapped_loops(q, d, 0) == UM.ungapped_numpy(q, d, 0) == 41
    q, d = b"WIIIIW", b"WDDDDW"                    # 11 -3 -3 -3 -3 11: a run that does not pay
    assert UM.ungapped_loops(q, d, 0) == UM.ungapped_numpy(q, d, 0) == 11
    assert UM.ungapped_loops(b"WX", b"WX", 0) == 11 and UM.ungapped_numpy(b"xW", b"XW", 0) == 11       # non-residues: code 20, -1
    mat = np.full((21, 21), -3)
    np.fill_diagonal(mat, 5)
    assert UM.ungapped_numpy(b"ACDA", b"ACDC", 0, mat) == UM.ungapped_loops(b"ACDA", b"ACDC", 0, mat) == 15


def test_u_is_at_most_the_score_on_planted_batches():
    prots, n_db = MM.planted_search(seed=3, n_targets=8, n_related=4, length=80)
    seq, off = S.batch(prots)
    hits, start, ung, counts, ucounts = UM.filtered_model(seq, off, n_db)
    assert len(hits) > 0 and (ung["ungapped"] <= hits["score"]).all() and (ung["on_diagonal"] <= hits["shared"]).all()
    plain = S.search_model(seq, off, n_db, max_cand=64)
    same = UM.filtered_model(seq, off, n_db, max_cand=64)
    assert same[0].tobytes() == plain[0].tobytes() and same[1].tobytes() == plain[1].tobytes() and same[3] == plain[2]


# ---- the ABI --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,binding,size", [("kg_ungapped_params", N.KgUngappedParams, 16), ("kg_ungapped_stats", N.KgUngappedStats, 40),
                                                ("kg_search_ungapped", None, 16)])
def test_the_bindings_match_the_c_structs(cname, binding, size, tmp_path):
    fields = [f for f, _ in binding._fields_] if binding is not None else list(N.SEARCH_UNGAPPED_DTYPE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%%zu\\n", sizeof(%s));\n' % cname +
                   "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    if binding is not None:
        assert out[0] == ctypes.sizeof(binding) == size and out[1:] == [getattr(binding, f).offset for f in fields]
    else:
        assert out[0] == N.SEARCH_UNGAPPED_DTYPE.itemsize == size
        assert out[1:] == [N.SEARCH_UNGAPPED_DTYPE.fields[f][1] for f in fields]


def test_exports_the_jna_source_and_the_documents():
    names = {"kg_proteins_search_filtered", "kg_proteins_search_filtered_device", "kg_hitset_ungapped_copy", "kg_hitset_ungapped_stats"}
    assert names <= set(N.EXPORTS)
    java = open(os.path.join(ROOT, "java", "kmergutsjava", "KmerGutsHip.java")).read()
    for name in names:
        assert re.search(r"\bint %s\(" % name, java), name
    for cls, order in (("KgUngappedParams", ["min_ungapped", "reserved"]), ("KgSearchUngapped", ["ungapped", "diagonal", "on_diagonal", "reserved"]),
                       ("KgUngappedStats", ["scored", "dropped", "cut", "cells", "ms_ungapped", "reserved"])):
        body = java[java.index("class %s " % cls):]
        got = re.search(r"setFieldOrder\(new String\[\] \{([^}]*)\}\)", body).group(1)
        assert [x.strip().strip('"') for x in got.split(",")] == order, cls
    assert "public int[] reserved = new int[3];" in java
    hdr = open(os.path.join(ROOT, "include", "kmerguts_hip.h")).read()
    for words in ("g(v) = i_q(v) - i_d(v)", "on a\n *   tie the smallest g", "u <= score", "about 200 bytes per join pair"):
        assert words in hdr, words
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "kg_proteins_search_filtered" in open(os.path.join(ROOT, name)).read() or "--ungapped" in open(os.path.join(ROOT, name)).read(), name


# ---- the front end ---------------------------------------------------------------------------------------------------------------

def _fasta(ids, prots) -> bytes:
    return b"".join(b">" + i + b"\n" + p + b"\n" for i, p in zip(ids, prots))


def _model_search(seen):
    def search(seq, offsets, n_db, ungapped=None, min_shared=2, max_cand=8, max_db_per_kmer=256, align=None, device=0, **kw):
        seen.clear()
        seen.update(kw, ungapped=ungapped)
        if ungapped is None:
            hits, start, counts = S.search_model(seq, offsets, n_db, min_shared=min_shared, max_cand=max_cand)
            return hits, start, dict(counts)
        hits, start, ung, counts, ucounts = UM.filtered_model(seq, offsets, n_db, min_ungapped=ungapped["min_score"], min_shared=min_shared,
                                                              max_cand=max_cand)
        return hits, start, dict(counts, ungapped=dict(ucounts, ms_ungapped=0.5)), ung
    return search


def test_the_writers_with_the_model_in_the_device_s_place(tmp_path):
    prots, n_db = MM.planted_search(seed=4, n_targets=6, n_related=3, length=70)
    ids = [b"p%d" % k for k in range(len(prots))]
    db, qs = tmp_path / "db.faa", tmp_path / "q.faa"
    db.write_bytes(_fasta(ids[:n_db], prots[:n_db]))
    qs.write_bytes(_fasta(ids[n_db:], prots[n_db:]))
    seen = {}
    plain_out, out = tmp_path / "plain.tsv", tmp_path / "u.tsv"
    plain = SP.search_proteins([str(db)], [str(qs)], str(plain_out), write_all=True, search=_model_search(seen))
    assert seen["ungapped"] is None and ", ungapped:" not in plain
    line = SP.search_proteins([str(db)], [str(qs)], str(out), write_all=True, search=_model_search(seen), ungapped=dict(min_score=20))
    assert seen["ungapped"] == dict(min_score=20)
    seq, off = S.batch(prots)
    want = UM.filtered_model(seq, off, n_db, min_ungapped=20)
    assert line.endswith(", ungapped: scored %d, dropped %d, cut %d, ungapped ms: 0.500" % (want[4]["scored"], want[4]["dropped"], want[4]["cut"]))
    rows = [r.split(b"\t") for r in out.read_bytes().splitlines()]
    assert len(rows) == len(want[0]) > 0 and all(len(r) == 13 for r in rows)
    assert [tuple(int(x) for x in r[10:]) for r in rows] == [(int(u["ungapped"]), int(u["diagonal"]), int(u["on_diagonal"])) for u in want[2]]
    assert all(len(r.split(b"\t")) == 10 for r in plain_out.read_bytes().splitlines())
    assert out.read_bytes() == SP.format_hits(ids[n_db:], ids[:n_db], want[0], want[1], write_all=True, ungapped=want[2])
    # in front of -A's function
    fn = {ids[0]: (b"kinase", b"")}
    with_fn = SP.format_hits(ids[n_db:], ids[:n_db], want[0], want[1], write_all=True, ungapped=want[2], functions=fn).splitlines()
    assert all(len(r.split(b"\t")) == 14 and r.split(b"\t")[13] in (b"kinase", b"-") for r in with_fn)
    with pytest.raises(ValueError):
        SP.search_proteins([str(db)], [str(qs)], str(out), search=_model_search(seen), ungapped=dict(min_score=-1))


def test_command_line_parsing_of_the_ungapped_flags(tmp_path, monkeypatch):
    src = tmp_path / "in.faa"
    src.write_bytes(_fasta([b"a"], [b"ACDEFGHIKLMNPQRSTVWY"]))
    got = {}
    monkeypatch.setattr(SP, "search_proteins", lambda *a, **kw: got.update(kw) or "ok")
    base = ["-d", str(src), "-q", str(src), "-o", str(tmp_path / "h.tsv")]
    assert SP.main(base) == 0 and got["ungapped"] is None
    assert SP.main(base + ["--ungapped"]) == 0 and got["ungapped"] == dict(min_score=0)
    assert SP.main(base + ["--ungapped", "--min-ungapped", "40", "--seeds", "reduced"]) == 0 and got["ungapped"] == dict(min_score=40)
    for bad in (["--min-ungapped", "40"], ["--ungapped", "--min-ungapped", "-1"]):
        with pytest.raises(SystemExit):
            SP.main(base + bad)


def test_the_python_ungapped_argument():
    from kmergutsjava_amd import hotpath
    for bad in (3, dict(score=1), "yes"):
        with pytest.raises(ValueError):
            hotpath.search_proteins(b"", np.zeros(1, dtype=np.int64), 0, ungapped=bad)
