"""The family rule (include/kmerguts_hip.h, kg_proteins_cluster) on the CPU: the two forms of tests/cluster_model.py against each
other, answers worked out by hand, the layouts of the new records, and the front end's writers with the device call replaced
by the model."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cluster_edge_cases as E  # noqa: E402
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


# ---- the inputs of tests/test_gpu_cluster_edges.py: the model against the answers of tests/cluster_edge_cases.py -------------

LOOPS_CHARS = 20000     # cluster_loops runs on every input of at most this many characters (20 ms), and on a larger one when it
                        # is the first of its test case: the 32 inputs of one large lane layout would take it 5 s


def _both(batch, answer, ms=1, pct=0, first=True, what=""):
    """cluster_numpy == the answer worked out without it (and == cluster_loops, see LOOPS_CHARS).  -> its records, counts"""
    seq, off = batch
    rec, counts = M.cluster_numpy(seq, off, ms, pct)
    if answer is not None:
        assert rec.tobytes() == answer[0].tobytes() and counts == answer[1], what
    if first or len(seq) <= LOOPS_CHARS:
        a, ca = M.cluster_loops(seq, off, ms, pct)
        assert a.tobytes() == rec.tobytes() and ca == counts, what
    return rec, counts


def test_the_constants_the_edge_cases_are_built_around():
    csrc = os.path.join(ROOT, "kmergutsjava_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("kg_device.hpp", "kg_derive.hpp", "kg_build.hpp", "kg_cluster.hpp",
                                                                     "kg_host.hpp", "kg_host_cluster.hpp")}

    def const(name, var):
        return int(re.search(r"constexpr int %s = (\d+);" % var, text[name]).group(1))

    assert const("kg_derive.hpp", "kDeriveChunk") == E.LANE == 16
    assert re.search(r"constexpr int kScanChunk = kScanThreads \* kScanPerThread;", text["kg_device.hpp"])
    assert const("kg_device.hpp", "kScanThreads") * const("kg_device.hpp", "kScanPerThread") == E.SCAN == 2048
    assert re.search(r"constexpr int kBuildTile = kBuildThreads \* kBuildItems;", text["kg_build.hpp"])
    assert const("kg_build.hpp", "kBuildThreads") * const("kg_build.hpp", "kBuildItems") == E.TILE == 4096
    assert const("kg_device.hpp", "kAaWinPerBlock") == 64 and {64 + 8 - 1, 64 + 8, 64 + 8 + 1, 2 * 64 + 8, 2 * 64 + 8 + 1} < set(E.BLOCK_LENGTHS)
    # every cluster kernel is launched 256 wide: its bound, the launches' block size and grid_of's divisor
    bounds = {name: width for width, name in re.findall(r"__launch_bounds__\((\w+)\) void (cluster_\w+_kernel)", text["kg_cluster.hpp"])}
    assert "cluster_centre_kernel" in bounds and len(bounds) == text["kg_cluster.hpp"].count("__global__")
    assert set(bounds.values()) == {str(E.THREADS)}
    launches = {name: width for name, width in re.findall(r"hipLaunchKernelGGL\(kg::(cluster_\w+_kernel), dim3\(grid_of\([^;]*?\)\), dim3\((\d+)\)",
                                                          text["kg_host_cluster.hpp"])}
    assert set(launches) == set(bounds) and set(launches.values()) == {str(E.THREADS)}
    assert text["kg_host_cluster.hpp"].count("kg::cluster_") == len(launches)           # every launch was read
    assert int(re.search(r"uint32_t grid_of\(uint64_t n, uint32_t threads = (\d+)\)", text["kg_host.hpp"]).group(1)) == E.THREADS
    assert E.THREADS * E.LANE == E.TILE


def test_tokens_and_the_union_find():
    assert M.token(0) == b"AAAAAAAA" and M.token(20 ** 8 - 1) == b"YYYYYYYY" and M.token(20 * 3 + 1) == b"AAAAAAEC"
    seq, off = M.token_batch([[5, 0], [], [0]], [0, 3, 2])
    assert seq == M.token(5) + b"X" + M.token(0) + b"X" + b"XXX" + M.token(0) + b"XXX" and off.tolist() == [0, 18, 21, 32]
    assert M.token_batch(np.array([[5], [0]]))[0] == M.token(5) + b"X" + M.token(0) + b"X"
    rec, counts = _both((seq, off), None)
    assert counts["valid_windows"] == counts["pairs"] == 3 and counts["kmers"] == 2 and rec.tolist() == [(0, 0, -1, 0), (1, 1, -1, 0), (0, 0, 0, 1)]
    seq, off = M.graph_batch(4, [(3, 1), (1, 0)])
    assert seq == M.token(1) + b"X" + M.token(1) + b"X" + M.token(0) + b"X" + b"X" * 9 + M.token(0) + b"X" and off.tolist() == [0, 9, 27, 36, 45]
    assert M.components(6, [(5, 3), (4, 2), (3, 1), (0, 0)]).tolist() == [0, 1, 2, 1, 2, 1]
    assert M.components(0, []).tolist() == [] and M.components(3, [(2, 1), (1, 0), (0, 2)]).tolist() == [0, 0, 0]


def test_the_lane_grid_is_the_one_stated():
    assert sorted(set(l for l, _ in E.LANE_GRID)) == [0, 1, 15, 16, 17, 4095, 4096, 4097]
    assert sorted(set(r for _, r in E.LANE_GRID)) == [1, 2, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8192]
    assert E.lane_places(0, 1) == [0] and E.lane_places(15, 33) == [0, 1, 16, 17, 32] and E.lane_places(1, 17) == [0, 14, 15, 16]
    at = E.lane_places(17, 8192)                                # pairs 17 .. 8208
    assert at == [0, 14, 15, 30, 31, 46, 47, 4078, 4079, 8158, 8159, 8174, 8175, 8190, 8191]


@pytest.mark.parametrize("lead,run", E.LANE_GRID)
def test_kmer_runs_at_lane_and_workgroup_borders(lead, run):
    for k, (name, batch, answer) in enumerate(E.lane_cases(lead, run)):
        rec, counts = _both(batch, answer, first=k == 0, what=name)
        assert counts["kmers"] == (lead > 0) + 1 + int(name.startswith("tail 1"))


@pytest.mark.parametrize("name,lead,sizes", E.SHORT_RUNS, ids=[c[0] for c in E.SHORT_RUNS])
def test_many_short_kmer_runs(name, lead, sizes):
    batch, answer = E.short_runs_case(lead, sizes)
    rec, counts = _both(batch, answer)
    assert counts["kmers"] == len(sizes) + (lead > 0) and counts["pairs"] == lead + sum(sizes)


@pytest.mark.parametrize("lead_links", E.LINK_LEAD)
@pytest.mark.parametrize("s", E.LINK_S)
def test_link_runs_at_the_scan_chunk(s, lead_links):
    batch, answer = E.link_case(s, lead_links)
    rec, _ = _both(batch, answer)
    assert rec[lead_links].tolist()[2:] == (lead_links + 1, s)
    if s >= 2047:
        for name, (ms, pct), batch, answer, edge in E.link_threshold_cases(s, lead_links):
            rec, counts = _both(batch, answer, ms, pct, first=False, what=name)
            assert rec[lead_links].tolist()[2:] == ((lead_links + 1, s) if edge else (-1, 0))


@pytest.mark.parametrize("s,third,m_first", E.THREE_CENTRES)
def test_one_member_between_three_centres(s, third, m_first):
    batch, answer = E.three_centres_case(s, third, m_first)
    rec, _ = _both(batch, answer, first=(s, third) == (2048, 2049))
    m = 0 if m_first else 3
    assert rec[m]["best"] == ((3 if m_first else 2) if third > s else (1 if m_first else 0)) and rec[m]["shared"] == max(s, third)


@pytest.mark.parametrize("n", E.KEY_WIDTH_N)
def test_key_width_inputs(n):
    members, pad = E.key_width_case(n)
    rec, counts = _both(M.token_batch(members, pad), E.token_answer(members, pad))
    assert counts["families"] == 1 and counts["kmers"] == min(n, 2) + {1: 0, 2: 1, 3: 3}.get(n, 4)


@pytest.mark.parametrize("length", E.BLOCK_LENGTHS)
def test_window_block_inputs(length):
    prots = E.block_edge_batch(length)
    rec, counts = _both(M.pack(prots), None, 5, 20)
    E.check_block_edge_records(length, rec, counts)


@pytest.mark.parametrize("shape", E.COMPONENT_SHAPES)
def test_component_shapes_against_the_union_find(shape):
    n, edges = E.component_shapes()[shape]
    assert set(E.component_shapes()) == set(E.COMPONENT_SHAPES) and 10000 <= n <= 20000
    rec, counts = _both(M.graph_batch(n, edges), None)
    E.check_component_records(n, edges, rec, counts)
