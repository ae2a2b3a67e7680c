"""The family rule (include/kmerguts_hip.h, kg_proteins_cluster) on the CPU: the two forms of tests/cluster_model.py against each
other, answers worked out by hand, the layouts of the new records, and the front end's writers with the device call replaced
by the model."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cluster_model as M  # noqa: E402
import test_regions_host as H  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("seed", range(300))
def test_the_two_forms_agree(seed):
    rng = np.random.default_rng(seed)
    prots = M.random_batch(rng, n_fam=int(rng.integers(0, 8)))
    seq, off = M.pack(prots)
    ms, pct = int(rng.integers(1, 7)), int(rng.choice([0, 10, 20, 50, 100]))
    a, ca = M.cluster_loops(seq, off, ms, pct)
    b, cb = M.cluster_numpy(seq, off, ms, pct)
    assert a.tobytes() == b.tobytes() and ca == cb
    assert cb["families"] == len(M.partition(b)) and (b["root"] <= np.arange(len(b))).all()
    assert (b["family"][b["root"]] == b["family"]).all() and cb["edges"] <= cb["links"] <= cb["pairs"] <= cb["valid_windows"]


def _rec(prots, ms=5, pct=20):
    seq, off = M.pack(prots)
    a, ca = M.cluster_loops(seq, off, ms, pct)
    b, cb = M.cluster_numpy(seq, off, ms, pct)
    assert a.tobytes() == b.tobytes() and ca == cb
    return b, cb


def test_two_identical_proteins():
    """A tie of the lengths: the centre is the smaller index, and s = d."""
    p = M.random_protein(np.random.default_rng(1), 40)
    rec, st = _rec([p, p])
    assert rec.tolist() == [(0, 0, -1, 0), (0, 0, 0, 32)] and st["pairs"] == 64 and st["kmers"] == 32 and st["links"] == st["edges"] == 1


def test_min_shared_bound():
    rng = np.random.default_rng(7)
    for s, edge in ((4, False), (5, True), (6, True)):
        rec, st = _rec(M.shared_pair(rng, s, 12), 5, 0)
        assert st["links"] == 1 and st["edges"] == int(edge) and st["families"] == 2 - int(edge)
        assert rec[0].tolist() == ((0, 0, 1, s) if edge else (0, 0, -1, 0)) and rec[1]["best"] == -1


def test_min_cover_bound():
    rng = np.random.default_rng(7)
    rec, st = _rec(M.shared_pair(rng, 5, 25), 1, 20)            # 100 * 5 == 20 * 25
    assert st["edges"] == 1 and rec.tolist() == [(0, 0, 1, 5), (0, 0, -1, 0)]
    rec, st = _rec(M.shared_pair(rng, 5, 26), 1, 20)            # 100 * 5 < 20 * 26
    assert st["links"] == 1 and st["edges"] == 0 and rec.tolist() == [(0, 0, -1, 0), (1, 1, -1, 0)]


def test_a_short_protein_inside_a_long_one():
    """The cover is the member's: the fragment shares all its k-mers, whatever the long protein's length."""
    rng = np.random.default_rng(2)
    long = M.random_protein(rng, 400)
    rec, st = _rec([long[100:130], long], 5, 100)
    assert rec.tolist() == [(0, 0, 1, 22), (0, 0, -1, 0)]


def test_a_chain_is_one_family():
    """A-B and B-C are edges, A-C is not: single linkage gives one family."""
    rng = np.random.default_rng(3)
    x, y, z, w = (M.random_protein(rng, 30) for _ in range(4))
    a, b, c = x + y, y + z + b"ACD", z + w
    rec, st = _rec([a, b, c])
    assert st["edges"] == 2 and M.partition(rec) == {frozenset({0, 1, 2})} and (rec["root"] == 0).all()
    assert rec["best"].tolist() == [1, -1, 1]                   # b is the longest: both links end there, none joins a and c


def test_proteins_without_windows_are_families_of_one():
    rec, st = _rec([b"", b"ACDEFGHI", b"XXXXXXXXXXXXXXXX", b"ACDEFGHIK"])
    assert st["valid_windows"] == 1 and rec["family"].tolist() == [0, 1, 2, 3] and (rec["best"] == -1).all()


# ---- layouts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,jname,py", [("kg_cluster_params", "KgClusterParams", N.KgClusterParams), ("kg_family", "KgFamily", N.FAMILY_DTYPE),
                                            ("kg_cluster_stats", "KgClusterStats", N.KgClusterStats)])
def test_jna_structures_match_the_c_layout(cname, jname, py):
    width = {"int32_t": "int", "uint32_t": "int", "int64_t": "long", "float": "float"}
    cf = H._c_struct(cname)
    jf, order = H._java_struct(jname)
    assert [n for n, _ in jf] == [n for n, _ in cf] == order
    assert [t for _, t in jf] == [width[t] for _, t in cf]
    names = list(py.names) if isinstance(py, np.dtype) else [n for n, _ in py._fields_]
    assert names == [n for n, _ in cf]


def test_dtypes_match_gcc_layout(tmp_path):
    snames = [n for n, _ in N.KgClusterStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%zu %zu %zu\\n", sizeof(kg_family), sizeof(kg_cluster_params), sizeof(kg_cluster_stats));\n' +
                   "".join('printf("%%zu\\n", offsetof(kg_family, %s));\n' % f for f in N.FAMILY_DTYPE.names) +
                   "".join('printf("%%zu\\n", offsetof(kg_cluster_stats, %s));\n' % f for f in snames) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [16, C.sizeof(N.KgClusterParams), C.sizeof(N.KgClusterStats)] and C.sizeof(N.KgClusterParams) == 12
    assert out[3:] == [N.FAMILY_DTYPE.fields[f][1] for f in N.FAMILY_DTYPE.names] + [getattr(N.KgClusterStats, f).offset for f in snames]


def test_the_documents_name_the_rule():
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "kg_proteins_cluster" in text or "cluster_proteins" in text, name


# ---- the front end ---------------------------------------------------------------------------------------------------------

def _model(seq, offsets, min_shared=5, min_cover_pct=20, device=0):
    rec, counts = M.cluster_numpy(seq, offsets, min_shared, min_cover_pct)
    return rec, dict(counts, rounds=1, ms_total=0.0)


def _fasta(path, named):
    with open(path, "wb") as f:
        for pid, s in named:
            f.write(b">" + pid + b" some words\n" + s[:17] + b"\n" + s[17:] + b"\n")


def test_front_end_writers_and_known_merging(tmp_path, capsys):
    from kmergutsjava_amd import cluster_proteins as CP
    rng = np.random.default_rng(4)
    a, b = M.random_protein(rng, 60), M.random_protein(rng, 50)
    one, two = tmp_path / "one.faa", tmp_path / "two.faa"
    _fasta(one, [(b"g1_a", a), (b"g1_lone", M.random_protein(rng, 45)), (b"g1_b", b)])
    _fasta(two, [(b"g2_a", a[3:] + b"KLM"), (b"g2_b", b[:40]), (b"g2_known", a[:50])])
    known = tmp_path / "known.tsv"
    known.write_bytes(b"g2_known\tsome enzyme\tgenome 2\nelsewhere\tanother enzyme")
    out, ann = tmp_path / "families.tsv", tmp_path / "ann.tsv"
    line = CP.cluster_proteins([str(one), str(two)], str(out), annotations=str(ann), known=str(known), cluster=_model)
    assert line.startswith("Proteins: 6, families: 3, multi: 2, largest: 3, edges: 3, rounds: 1, ms: ")
    assert out.read_bytes() == (b"g1_a\tfamily_g1_a\t3\tg1_a\t-\t0\n" b"g1_b\tfamily_g1_b\t2\tg1_b\t-\t0\n"
                                b"g2_a\tfamily_g1_a\t3\tg1_a\tg1_a\t49\n" b"g2_b\tfamily_g1_b\t2\tg1_b\tg1_b\t32\n"
                                b"g2_known\tfamily_g1_a\t3\tg1_a\tg1_a\t42\n")
    assert ann.read_bytes() == (b"g2_known\tsome enzyme\tgenome 2\nelsewhere\tanother enzyme\n"
                                b"g1_a\thypothetical protein family_g1_a\n" b"g1_b\thypothetical protein family_g1_b\n"
                                b"g2_a\thypothetical protein family_g1_a\n" b"g2_b\thypothetical protein family_g1_b\n")
    # what -A wrote is what make_signatures -A reads
    from kmergutsjava_amd.make_signatures import parse_annotations
    assert parse_annotations(ann.read_bytes())[b"g2_a"] == (b"hypothetical protein family_g1_a", b"")
    CP.cluster_proteins([str(one), str(two)], str(out), write_all=True, min_size=3, annotations=str(ann), cluster=_model)
    assert out.read_bytes().count(b"\n") == 6 and b"g1_lone\tfamily_g1_lone\t1\tg1_lone\t-\t0\n" in out.read_bytes()
    assert ann.read_bytes() == (b"g1_a\thypothetical protein family_g1_a\n" b"g2_a\thypothetical protein family_g1_a\n"
                                b"g2_known\thypothetical protein family_g1_a\n")
    # a duplicate id across inputs is an error naming it
    with pytest.raises(CP.InputError) as ei:
        CP.cluster_proteins([str(one), str(one)], str(out), cluster=_model)
    assert "g1_a" in str(ei.value)
    assert CP.main(["-p", str(one), "-p", str(one), "-o", str(out)]) == 1 and "duplicate protein id g1_a" in capsys.readouterr().err
    with pytest.raises(ValueError):
        CP.cluster_proteins([str(one)], str(out), known=str(known), cluster=_model)
