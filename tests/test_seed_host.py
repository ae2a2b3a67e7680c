"""The seed rule (include/kmerguts_hip.h, kg_proteins_search_seeded) on the CPU: the two forms of tests/seed_model.py against each
other and against answers worked out by hand, the identity set against the exact rule, the written forms of a seed set
(kmergutsjava_amd/seeds.py), the layouts, and the front end's writers with the device call replaced by the model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_model as M
import search_model as S
import seed_model as SD
import test_java_binding as H
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import seeds as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mask(text):
    return sum(1 << j for j, ch in enumerate(text) if ch == "1")


def _protein(rng, length, x_rate=0.03):
    p = bytearray(M.random_protein(rng, length))
    for i in range(length):
        if rng.random() < x_rate:
            p[i] = ord("X")
    return bytes(p)


# ---- the two forms ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("part", range(4))
def test_loops_against_numpy_on_random_small_batches(part):
    """75 batches a part: random class maps, one to four shapes of differing spans, X, empty proteins, and proteins one shorter
    than, as long as and one longer than every span (the first has no window, the second none either: the last position is left
    out; the third has one)."""
    rng = np.random.default_rng(700 + part)
    for it in range(75):
        seed = SD.random_seed(rng, n_shapes=1 + it % 4, max_span=(32 if it % 3 else 12))
        fam = [_protein(rng, int(rng.integers(10, 70))) for _ in range(3)]
        prots = [fam[int(rng.integers(0, 3))][int(rng.integers(0, 6)):] for _ in range(8)] + [b"", _protein(rng, 5)]
        for m in seed[1]:
            prots += [fam[0][:SD.span(m) + d] for d in (-1, 0, 1)]
        prots = [prots[i] for i in rng.permutation(len(prots))]
        seq, off = S.batch(prots)
        n_db = int(rng.integers(0, len(prots) + 1))
        mask = int(rng.choice([1, 2, 256]))
        a, b = SD.shared_loops(seed)(seq, off, n_db, mask), SD.shared_numpy(seed)(seq, off, n_db, mask)
        assert a == b, (seed, prots, n_db)


def test_the_identity_set_is_the_exact_rule():
    rng = np.random.default_rng(710)
    for it in range(60):
        fam = [_protein(rng, int(rng.integers(8, 60))) for _ in range(3)]
        prots = [fam[int(rng.integers(0, 3))][int(rng.integers(0, 4)):] for _ in range(10)] + [b"", b"ACDEFGHI", b"ACDEFGHIK"]
        seq, off = S.batch(prots)
        n_db = int(rng.integers(0, len(prots) + 1))
        want = S.shared_numpy(seq, off, n_db, 2)
        assert SD.shared_numpy(SD.EXACT)(seq, off, n_db, 2) == want == SD.shared_loops(SD.EXACT)(seq, off, n_db, 2)
    full = S.search_model(seq, off, 6)
    mine = SD.search_model(seq, off, 6, SD.EXACT)
    assert mine[0].tobytes() == full[0].tobytes() and mine[1].tobytes() == full[1].tobytes() and mine[2] == full[2]


# ---- answers worked out by hand -------------------------------------------------------------------------------------------------

def test_x_on_a_dont_care_position_and_on_a_care_position():
    seed = (SD.IDENTITY, [_mask("1101")])                    # span 4, weight 3
    assert SD.seed_ids(b"ACXDE", seed) == [0 * 400 + 1 * 20 + 2]          # window 0: A C . D; X on the don't-care position
    assert SD.seed_ids(b"AXCDE", seed) == []                 # X on position 1: a care position
    assert SD.seed_ids(b"ACXD", seed) == []                  # length = span: the last position is left out
    for shared in (SD.shared_loops(seed), SD.shared_numpy(seed)):
        s_of, counts = shared(*S.batch([b"ACXDE", b"ACWDE", b"AXCDE"]), 1)
        assert s_of == {(0, 0): 1} and counts["valid_windows"] == 2 and counts["kmers"] == 1 and counts["pairs"] == 2


def test_the_same_value_under_two_shapes_counts_twice():
    seed = (SD.IDENTITY, [_mask("11"), _mask("101")])
    # AAAAA: under 11 the windows 0..2 are (A, A) = value 0; under 101 the windows 0, 1 are value 0 as well: ids 0 and 400
    assert SD.seed_ids(b"AAAAA", seed) == [0, 0, 0, 400, 400]
    for shared in (SD.shared_loops(seed), SD.shared_numpy(seed)):
        s_of, counts = shared(*S.batch([b"AAAAA", b"AAAAA"]), 1)
        assert s_of == {(0, 0): 2} and counts["valid_windows"] == 10 and counts["pairs"] == 4 and counts["kmers"] == 2
        assert counts["join_pairs"] == 2


def test_a_window_valid_for_the_short_shape_only_at_the_proteins_end():
    seed = (SD.IDENTITY, [_mask("11"), _mask("1001")])
    # ACDEF, len 5: 11 (span 2) has windows 0, 1, 2; 1001 (span 4) has window 0 only (0 + 4 < 5)
    assert SD.seed_ids(b"ACDEF", seed) == [0 * 20 + 1, 1 * 20 + 2, 2 * 20 + 3, 400 + 0 * 20 + 3]
    assert SD.seed_ids(b"ACDE", seed) == [1, 22]             # the long shape has no window at all
    v, p = SD.seed_pairs(*S.batch([b"ACDEF", b"ACDE"]), seed)
    assert sorted(zip(p.tolist(), v.tolist())) == [(0, 1), (0, 22), (0, 43), (0, 403), (1, 1), (1, 22)]


def test_i_and_l_share_a_seed_under_reduced11_only():
    a, b = b"ACDEFGHIKLMNPQRSTVWY", b"ACDEFGHLKLMNPQRSTVWY"     # I -> L at position 7
    assert SD.REDUCED11[7] == SD.REDUCED11[9] == 6
    shape = [0xFF]
    for shared in (SD.shared_loops, SD.shared_numpy):
        assert shared((SD.REDUCED11, shape))(*S.batch([a, b]), 1)[0] == {(0, 0): 12}
        assert shared((SD.IDENTITY, shape))(*S.batch([a, b]), 1)[0] == {(0, 0): 4}        # the windows 8..11, behind the I
    assert set(SD.seed_ids(a[:9], (SD.REDUCED11, shape))) == set(SD.seed_ids(b[:9], (SD.REDUCED11, shape)))
    assert not set(SD.seed_ids(a[:9], SD.EXACT)) & set(SD.seed_ids(b[:9], SD.EXACT))


def test_the_input_that_shows_the_feature():
    targets, queries = SD.conservative_pairs(np.random.default_rng(720), 6)
    seq, off = S.batch(targets + queries)
    assert S.shared_numpy(seq, off, 6)[0] == {}
    hits, start, counts = SD.search_model(seq, off, 6, SD.REDUCED)
    assert counts["queries_hit"] == 6 and [int(hits[start[q]]["target"]) for q in range(6)] == list(range(6))


# ---- the written forms ----------------------------------------------------------------------------------------------------------

def test_the_group_string_parser():
    assert P.parse_alphabet("reduced11") == (SD.REDUCED11, 11) == P.parse_alphabet(P.REDUCED11)
    assert P.parse_alphabet("identity") == (SD.IDENTITY, 20)
    assert P.parse_alphabet("WY,ACDEFGHIKLMNPQRSTV") == ([1] * 18 + [0, 0], 2)
    for text, words in (("AST,C,DEKNQR,F,G,H,ILV,M,P,W", "residue Y is in no group"), ("ACDEFGHIKLMNPQRSTVWY", "at least 2 groups"),
                        ("ACDEFGHIKLMNPQRSTVW,Y,", "group 2 is empty"), ("ACDEFGHIKLMNPQRSTVW,YA", "residue A is in two groups"),
                        ("ACDEFGHIKLMNPQRSTVW,YB", "'B' is not one of the residues"), ("", "group 0 is empty"),
                        ("ACDEFGHIKLMNPQRSTVW,y", "'y' is not one of the residues")):
        with pytest.raises(ValueError, match=re.escape(words)):
            P.parse_alphabet(text)


def test_the_mask_parser():
    assert P.parse_shape("11111111") == 0xFF and P.parse_shape("1") == 1 and P.parse_shape("1" + "0" * 30 + "1") == 0x80000001
    assert [P.parse_shape(s) for s in P.REDUCED["shapes"]] == SD.REDUCED[1] == [0xD6F, 0x659B]
    assert SD.as_dict(SD.REDUCED)["shapes"] == P.REDUCED["shapes"]
    for text, words in (("", "written with the characters 1 and 0"), ("1x1", "written with the characters 1 and 0"),
                        ("011", "the first and the last position must be 1"), ("110", "the first and the last position must be 1"),
                        ("1" * 33, "at most 32 positions")):
        with pytest.raises(ValueError, match=re.escape(words)):
            P.parse_shape(text)


def test_resolving_a_seed_set():
    assert P.resolve(None) is None and P.resolve("exact") is None
    cls, n_cls, masks, alphabet, shapes = P.resolve("reduced")
    assert (cls, masks) == tuple(SD.REDUCED) and n_cls == 11 and P.describe("reduced") == "reduced11 x 111101101011,110110011010011"
    assert P.resolve(dict(shapes=["101"]))[:3] == (SD.IDENTITY, 20, [5]) and P.resolve(dict(alphabet="reduced11"))[2] == [0xFF]
    assert P.resolve(SD.as_dict(SD.REDUCED))[:3] == (SD.REDUCED11, 11, SD.REDUCED[1])
    for seeds, words in (("fast", "seeds must be"), (dict(shape=["1"]), "unknown key 'shape'"), (dict(shapes=[]), "1 to 4 shapes"),
                         (dict(shapes=["1"] * 5), "1 to 4 shapes"), (dict(shapes=["111", "1001"]), "shape '1001': 2 care positions"),
                         (dict(shapes=["1" * 9]), "is over 2^35"), (dict(alphabet="A,C"), "is in no group")):
        with pytest.raises(ValueError, match=re.escape(words)):
            P.resolve(seeds)
    assert P.resolve(dict(alphabet="reduced11", shapes=["1" * 10]))[1] == 11           # 11^10 < 2^35


def test_the_librarys_built_in_sets_are_the_written_ones():
    lib = N.load()
    for which, want in ((N.SEEDS_EXACT, SD.EXACT), (N.SEEDS_REDUCED, SD.REDUCED)):
        p = N.KgSeedParams()
        assert lib.kg_seed_params_builtin(which, C.byref(p)) == N.KG_OK
        assert (list(p.cls), list(p.shape)[:p.n_shapes], p.alphabet_size, p.reserved) == (want[0], want[1], max(want[0]) + 1, 0)
        assert list(p.shape)[p.n_shapes:] == [0] * (4 - p.n_shapes)
    assert lib.kg_seed_params_builtin(2, C.byref(p)) == N.KG_ERR_ARG and lib.kg_seed_params_builtin(0, None) == N.KG_ERR_ARG


# ---- layouts --------------------------------------------------------------------------------------------------------------------

def test_kg_seed_params_against_gcc_and_the_jna_source(tmp_path):
    names = [n for n, _ in N.KgSeedParams._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%zu\\n", sizeof(kg_seed_params));\n' +
                   "".join('printf("%%zu\\n", offsetof(kg_seed_params, %s));\n' % f for f in names) +
                   'printf("%d %d\\n", KG_SEEDS_EXACT, KG_SEEDS_REDUCED);\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(N.KgSeedParams) == 48
    assert out[1:6] == [getattr(N.KgSeedParams, f).offset for f in names] == [0, 4, 8, 28, 44]
    assert out[6:] == [N.SEEDS_EXACT, N.SEEDS_REDUCED]
    body = re.search(r"class KgSeedParams extends Structure \{(.*?)\n    \}", H._strip_comments(H.JAVA), flags=re.S).group(1)
    fields = re.findall(r"public\s+(?:int|byte\[\]|int\[\])\s+([^;=]+?)\s*(?:=[^;]*)?;", body)
    assert [n.strip() for f in fields for n in f.split(",")] == names
    assert re.search(r"public\s+byte\[\]\s+cls\s*=\s*new\s+byte\[20\]", body) and re.search(r"public\s+int\[\]\s+shape\s*=\s*new\s+int\[4\]", body)
    assert re.findall(r'"([a-z_0-9]+)"', re.search(r"setFieldOrder\(new String\[\]\s*\{(.*?)\}\)", body, flags=re.S).group(1)) == names
    assert {"kg_seed_params_builtin", "kg_proteins_search_seeded", "kg_proteins_search_seeded_device"} <= set(N.EXPORTS)


def test_the_kernels_constants_and_the_documents():
    text = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_seed.hpp")).read()
    assert int(re.search(r"constexpr int kSeedMaxShapes = (\d+);", text).group(1)) == P.MAX_SHAPES == 4
    assert int(re.search(r"constexpr int kSeedMaxSpan = (\d+);", text).group(1)) == P.MAX_SPAN == 32
    hdr = open(os.path.join(ROOT, "include", "kmerguts_hip.h")).read()
    for words in ("AST, C, DEKNQR, F, G,", "111101101011 (span 12) and 110110011010011 (span 15)", "equal kg_proteins_search's byte for byte"):
        assert words in hdr, words
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "kg_proteins_search_seeded" in open(os.path.join(ROOT, name)).read(), name


# ---- the front end --------------------------------------------------------------------------------------------------------------

def _fasta(path, ids, seqs):
    path.write_bytes(b"".join(b">%s some words\n%s\n" % (i, s) for i, s in zip(ids, seqs)))
    return str(path)


def _model_search(calls):
    def search(seq, offsets, n_db, min_shared=2, max_cand=8, max_db_per_kmer=256, align=None, device=0, seeds=None):
        calls.append(seeds)
        got = P.resolve(seeds)
        shared = S.shared_numpy if got is None else SD.shared_numpy((got[0], got[2]))
        return S.search_model(seq, offsets, n_db, min_shared, max_cand, max_db_per_kmer, shared=shared, **(align or {}))
    return search


def test_front_end_writers_and_options(tmp_path, monkeypatch, capsys):
    from kmergutsjava_amd import hotpath, search_proteins as SP
    targets, queries = SD.conservative_pairs(np.random.default_rng(730), 3)
    db = _fasta(tmp_path / "db.faa", [b"d0", b"d1", b"d2"], targets)
    qs = _fasta(tmp_path / "q.faa", [b"q0", b"q1", b"q2", b"same"], queries + [targets[1]])
    (tmp_path / "ann.tsv").write_bytes(b"d0\tkinase\nd1\tligase\nd2\tlyase\n")
    out, tr = str(tmp_path / "hits.tsv"), str(tmp_path / "transfer.tsv")
    calls = []
    search = _model_search(calls)
    # the default: the call carries no seeds argument at all, and the line has no seeds words
    line0 = SP.search_proteins([db], [qs], out, annotations=str(tmp_path / "ann.tsv"), transfer=tr, search=search)
    assert calls == [None] and "seeds" not in line0 and line0.startswith("Queries: 4, targets: 3, candidates: 1, aligned: 1, hits: 1,")
    exact_out, exact_tr = open(out, "rb").read(), open(tr, "rb").read()
    assert exact_tr == b"same\tligase\n" and [r.split(b"\t")[0] for r in exact_out.splitlines()] == [b"same"]
    # reduced: every query is found; the files keep their format and the line gains its words at the end
    line = SP.search_proteins([db], [qs], out, annotations=str(tmp_path / "ann.tsv"), transfer=tr, search=search, seeds="reduced")
    assert calls[-1] == "reduced" and line.endswith(", seeds: reduced11 x 111101101011,110110011010011")
    assert line.startswith("Queries: 4, targets: 3, candidates: 4, aligned: 4, hits: 4, queries hit: 4, transferred: 4,")
    rows = [r.split(b"\t") for r in open(out, "rb").read().splitlines()]
    assert [(r[0], r[1], r[2], r[9], r[10]) for r in rows] == [(b"q0", b"0", b"d0", b"hit", b"kinase"), (b"q1", b"0", b"d1", b"hit", b"ligase"),
                                                              (b"q2", b"0", b"d2", b"hit", b"lyase"), (b"same", b"0", b"d1", b"hit", b"ligase")]
    assert all(len(r) == 11 for r in rows) and open(tr, "rb").read() == b"q0\tkinase\nq1\tligase\nq2\tlyase\nsame\tligase\n"
    # the command line: exact and no override passes no seeds; either override makes a seed set of the chosen one
    monkeypatch.setattr(hotpath, "search_proteins", search)
    base = ["-d", db, "-q", qs, "-o", out]
    assert SP.main(base) == 0 and calls[-1] is None and open(out, "rb").read() != exact_out      # (no -A: one field fewer)
    assert capsys.readouterr().err.strip() == re.sub(r"transferred: 1", "transferred: 0", line0)
    assert SP.main(base + ["--seeds", "exact"]) == 0 and calls[-1] is None
    assert SP.main(base + ["--seeds", "reduced"]) == 0 and calls[-1] == P.REDUCED
    assert capsys.readouterr().err.strip().endswith(", seeds: reduced11 x 111101101011,110110011010011")
    assert SP.main(base + ["--alphabet", "reduced11"]) == 0 and calls[-1] == dict(alphabet="reduced11", shapes=["11111111"])
    assert capsys.readouterr().err.strip().endswith(", seeds: reduced11 x 11111111")
    assert SP.main(base + ["--seeds", "reduced", "--shape", "1101", "--shape", "1011"]) == 0
    assert calls[-1] == dict(alphabet="reduced11", shapes=["1101", "1011"])
    assert SP.main(base + ["--shape", "11111111"]) == 0 and calls[-1] == P.EXACT          # written out, the exact set is a seed set
    assert capsys.readouterr().err.strip().endswith(", seeds: identity x 11111111")
    n_calls = len(calls)
    assert SP.main(base + ["--shape", "110"]) == 1 and "the first and the last position must be 1" in capsys.readouterr().err
    assert SP.main(base + ["--alphabet", "AC,DE"]) == 1 and "is in no group" in capsys.readouterr().err and len(calls) == n_calls
    with pytest.raises(SystemExit):
        SP.main(base + ["--shape", "1"] * 5)
    with pytest.raises(SystemExit):
        SP.main(base + ["--seeds", "fast"])
