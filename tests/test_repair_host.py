"""Frameshift repair on the CPU (no GPU): the two forms of the model (tests/repair_model.py) against each other and against
chains worked out by hand (tests/repair_cases.py), the structures against gcc and the JNA source, the kernels' resource report.

Two cases a reader may look for cannot be built.  lo == hi: lo = q + 3 (sq + 1) and hi = p + 3 tp differ by q - p modulo 3, and
p != q.  lo == hi + 1: frame q's stop would end on the nucleotide frame p's stop begins with, an A or G that is a T; the same
clash of letters rules out lo - hi = 2, 4 and 5, and 3 and 6 are one frame.  The narrowest window is hi = lo + 1 and the
narrowest failure lo = hi + 7; both are among the cases."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import orfs_model  # noqa: E402
import regions_model  # noqa: E402
import repair_cases as RC  # noqa: E402
import repair_model as M  # noqa: E402
import test_java_binding as H  # noqa: E402
from kmergutsjava_amd import _native as N  # noqa: E402


def given(calls, seq, off, merge_gap=600, start_codons=7, only_kept=True, **region_kw):
    regs, _ = regions_model.regions(calls, off, merge_gap=merge_gap, **region_kw)
    return (regs,) + orfs_model.orfs(regs, seq, off, start_codons=start_codons, only_kept=only_kept)


def same(a, b, what=""):
    for name, x, y in zip(("orfs", "prot_start", "residues", "junctions", "junction_start"), a[:5], b[:5]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, name, x, y)
    assert a[5] == b[5], (what, a[5], b[5])


@pytest.mark.parametrize("seed", range(6))
def test_plain_loops_match_numpy(seed):
    """Sixty random small batches a seed: contigs of 0..30 among longer ones, N, u and lower case, both strands, chains of 2 to 6
    and more segments, overlapping and nested CALLs, min_count, max_junctions, start masks, two merge gaps, min_score."""
    rng = np.random.default_rng(100 + seed)
    tot = dict.fromkeys(M.STAT_KEYS, 0)
    segments = set()
    for _ in range(60):
        calls, seq, off = M.random_case(rng, n_seqs=int(rng.integers(1, 7)))
        kw = dict(start_codons=int(rng.choice([7, 7, 1, 0])), min_count=int(rng.choice([0, 0, 2, 4])), max_junctions=int(rng.choice([1, 2, 4, 8])))
        regs, o, ps, res = given(calls, seq, off, merge_gap=int(rng.choice([30, 600])), start_codons=kw["start_codons"],
                                 only_kept=bool(rng.integers(0, 2)), min_score=int(rng.choice([0, 6])))
        a = M.repair(regs, o, ps, res, calls, seq, off, **kw)
        same(a, M.brute_force(regs, o, ps, res, calls, seq, off, **kw))
        for k in tot:
            tot[k] += a[5][k]
        segments |= set((np.diff(a[4]) + 1).tolist())
        # what is not repaired is the given set's, byte for byte; what is repaired satisfies the later stages' record check
        rep = (a[0]["flags"] & M.REPAIRED) != 0
        assert a[0][~rep].tobytes() == o[~rep].tobytes() and rep.sum() == a[5]["repaired"]
        for i in np.flatnonzero(~rep):
            assert a[2][a[1][i]:a[1][i + 1]].tobytes() == res[ps[i]:ps[i + 1]].tobytes()
        r = a[0][rep]
        assert (3 * r["n_res"].astype(np.int64) <= r["right"].astype(np.int64) - r["left"] + 1).all()
        assert ((r["flags"] & (M.INTERRUPTED | M.MULTI_FRAME)) == (M.INTERRUPTED | M.MULTI_FRAME)).all() and (r["kept"] != 0).all()
    assert all(tot[k] > 0 for k in M.STAT_KEYS), tot
    assert {2, 3, 4, 5} <= segments, segments


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("case", RC.cases(), ids=lambda c: c["name"])
def test_known_answers(case, strand):
    calls, seq, off = RC.lay(case["text"], strand, case["calls"])
    regs, o, ps, res = given(calls, seq, off, start_codons=1)
    assert len(regs) == 1 and regs[0]["strand"] == strand and regs[0]["kept"] == 1
    kw = dict(start_codons=1, **case["params"])
    for form in (M.repair, M.brute_force):
        orfs, pstart, residues, junc, jstart, st = form(regs, o, ps, res, calls, seq, off, **kw)
        assert st["candidates"] == 1 and st[case["state"]] == 1 and sum(st[k] for k in ("repaired", "failed", "single", "skipped")) == 1
        if case["state"] != "repaired":
            assert orfs.tobytes() == o.tobytes() and residues.tobytes() == res.tobytes() and junc.size == 0 and jstart.tolist() == [0, 0]
            continue
        want_j, (left, right) = RC.expected_on(case, strand)
        assert [tuple(int(v) for v in j) for j in junc] == [(0,) + j for j in want_j], (form.__name__, junc)
        assert jstart.tolist() == [0, len(want_j)]
        r = orfs[0]
        assert (r["seq"], r["strand"], r["frame"], r["left"], r["right"]) == (0, strand, case["frame"], left, right), r
        assert residues.tobytes() == case["protein"] and r["n_res"] == len(case["protein"]) and pstart.tolist() == [0, r["n_res"]]
        assert (r["start_codon"], r["first_inner"], r["flags"]) == (case["start_codon"], case["first_inner"], case["flags"]), r
        assert (r["fI"], r["score"], r["kept"]) == (regs[0]["fI"], regs[0]["score"], 1)
        assert st["junctions"] == len(want_j) and st["residues"] == r["n_res"]


def test_the_given_orf_of_a_shifted_gene_is_half_garbage():
    """What the repair is for: the unrepaired record of the deletion case reads frame 0 straight through."""
    case = RC.cases()[0]
    calls, seq, off = RC.lay(case["text"], 0, case["calls"])
    regs, o, ps, res = given(calls, seq, off, start_codons=1)
    assert o[0]["frame"] == 0 and (o[0]["flags"] & M.MULTI_FRAME) and res.tobytes()[:10] == case["protein"][:10]
    assert res.tobytes()[-20:] != case["protein"][-20:]


def test_structs_match_the_c_layout_and_the_jna_source(tmp_path):
    width = {"int32_t": "int", "uint32_t": "int", "int64_t": "long", "float": "float"}
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    lines = []
    for cname, jname, py in (("kg_repair_params", "KgRepairParams", N.KgRepairParams), ("kg_repair_stats", "KgRepairStats", N.KgRepairStats)):
        cf = H._c_struct(cname)
        jf, order = H._java_struct(jname)
        assert [n for n, _ in jf] == [n for n, _ in cf] == order == [n for n, _ in py._fields_], cname
        assert [t for _, t in jf] == [width[t] for _, t in cf] and [t for _, t in py._fields_] == [ctype[t] for _, t in cf], cname
        lines.append('printf("%%zu\\n", sizeof(%s));\n' % cname)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f, _ in cf]
    jf = H._c_struct("kg_junction")
    assert [n for n, _ in jf] == list(N.JUNCTION_DTYPE.names) and all(t == "int32_t" for _, t in jf)
    lines.append('printf("%zu\\n", sizeof(kg_junction));\n')
    lines += ['printf("%%zu\\n", offsetof(kg_junction, %s));\n' % f for f, _ in jf]
    lines.append('printf("%u\\n", KG_ORF_REPAIRED);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for py in (N.KgRepairParams, N.KgRepairStats):
        want += [C.sizeof(py)] + [getattr(py, f).offset for f, _ in py._fields_]
    want += [N.JUNCTION_DTYPE.itemsize] + [N.JUNCTION_DTYPE.fields[f][1] for f in N.JUNCTION_DTYPE.names] + [N.ORF_REPAIRED]
    assert out == want and C.sizeof(N.KgRepairParams) == 16 and C.sizeof(N.KgRepairStats) == 64 and N.JUNCTION_DTYPE.itemsize == 24
    assert N.ORF_REPAIRED == M.REPAIRED == 128
    assert {"kg_regionset_repair", "kg_result_repair", "kg_orfset_junctions_count", "kg_orfset_junctions_copy", "kg_orfset_junctions_start",
            "kg_orfset_junctions_stats"} <= set(N.EXPORTS)


def test_constants_match_the_kernels():
    src = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_repair.hpp")).read()
    assert "constexpr int kRepairMaxJunctions = %d;" % N.REPAIR_MAX_JUNCTIONS in src
    hdr = open(os.path.join(ROOT, "include", "kmerguts_hip.h")).read()
    assert "#define KG_ORF_REPAIRED   128u" in hdr


def test_the_kernels_use_no_scratch_and_do_not_spill():
    """From the compiler's own report (tools/kernel_resources.py), as tests/test_kernel_resources.py reads it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not found")
    res = kr.resources()
    for k in ("repair_inverse_kernel", "repair_owner_kernel", "repair_runs_kernel", "repair_calls_kernel", "repair_sums_kernel",
              "repair_compact_kernel", "repair_seg_heads_kernel", "repair_segments_kernel", "repair_junction_kernel", "repair_parts_kernel",
              "repair_record_kernel", "repair_junction_records_kernel", "repair_residues_kernel"):
        assert k in res, (k, sorted(res))
        assert res[k]["sgpr_spills"] == 0 and res[k]["vgpr_spills"] == 0 and res[k]["scratch"] == 0, (k, res[k])
