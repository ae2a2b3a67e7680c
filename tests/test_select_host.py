"""The gene-set selection rule (include/kmerguts_hip.h, kg_regionset_select) on the CPU: the model of tests/select_model.py
against a brute force, the rule's properties, known answers, the layouts of the new records, the front end's writers, and a
round trip over planted genes with decoy regions."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import orfs_model as O  # noqa: E402
import regions_model as R  # noqa: E402
import select_model as S  # noqa: E402
import test_orfs_host as HO  # noqa: E402
import test_regions_host as H  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

ROOT = os.path.dirname(HERE)
PARAMS = [(0, 0), (0, 100), (1, 50), (60, 50), (60, 0), (10 ** 6, 100), (10 ** 6, 0), (5, 30)]


def _random_case(seed):
    rng = np.random.default_rng(seed)
    kind = seed % 5
    n = int(rng.integers(0, 60))
    if kind == 0:
        iv = S.nested(n, score_up=bool(seed & 8))
    elif kind == 1:
        iv = S.staircase(n, descending=bool(seed & 8))
    elif kind == 2:
        iv = S.identical(n)
    else:
        iv = S.random_list(rng, n, n_seqs=int(rng.integers(1, 4)), span=int(rng.integers(50, 1500)),
                           max_len=int(rng.integers(1, 400)), max_score=int(rng.integers(1, 30)))
    if kind < 3 and n:
        iv["eligible"] = rng.random(n) < 0.9
        iv, _ = S.shuffled(rng, iv)
    return iv, PARAMS[int(rng.integers(0, len(PARAMS)))]


@pytest.mark.parametrize("seed", range(300))
def test_model_matches_brute_force_and_has_the_properties(seed):
    iv, (mo, pct) = _random_case(seed)
    out, st = S.select(iv, mo, pct)
    assert out.tobytes() == S.brute_force(iv, mo, pct).tobytes()
    assert out.tobytes() == S.select_fast(iv, mo, pct).tobytes()
    S.check_properties(iv, out, mo, pct)
    assert st["selected"] + st["overlapped"] == st["eligible"] <= st["candidates"] == len(iv) and st["conflicts"] <= st["pairs"]


def _states(iv, mo=60, pct=50):
    out, _ = S.select(iv, mo, pct)
    return out["state"].tolist(), out["by"].tolist()


def test_known_answer_a_loser_suppresses_nothing():
    """A > B > C, A conflicts with B, B with C, A not with C: A and C are selected and B lost to A."""
    iv = S.intervals([(0, 0, 99, 30), (0, 50, 149, 20), (0, 100, 199, 10)])
    assert _states(iv, 10, 100) == ([1, 2, 1], [-1, 0, -1])


def test_known_answer_ties_go_to_length_then_index():
    assert _states(S.intervals([(0, 0, 99, 5), (0, 0, 119, 5)]), 0, 0) == ([2, 1], [1, -1])
    assert _states(S.intervals([(0, 0, 99, 5), (0, 0, 99, 5), (0, 0, 99, 5)]), 0, 0) == ([1, 2, 2], [-1, 0, 0])


def test_known_answer_overlap_bounds():
    """ov == max_overlap is no conflict, one more nucleotide is; 100 * ov == pct * shorter is no conflict, one more is."""
    two = lambda left: S.intervals([(0, 0, 999, 9), (0, left, left + 999, 8)])  # noqa: E731
    assert _states(two(940), 60, 100)[0] == [1, 1] and _states(two(939), 60, 100)[0] == [1, 2]
    short = lambda left: S.intervals([(0, 0, 999, 9), (0, left, left + 39, 8)])  # noqa: E731   shorter = 40, half = 20
    assert _states(short(980), 10 ** 6, 50)[0] == [1, 1] and _states(short(979), 10 ** 6, 50)[0] == [1, 2]
    assert _states(short(999), 10 ** 6, 0)[0] == [1, 2] and _states(short(1000), 0, 0)[0] == [1, 1]


def test_known_answer_contigs_and_non_eligible():
    """The same coordinates on two contigs do not conflict; a non-eligible giant suppresses nothing and is (0, -1)."""
    assert _states(S.intervals([(0, 100, 500, 9), (1, 100, 500, 3)]))[0] == [1, 1]
    assert _states(S.intervals([(0, 0, 10 ** 6, 99, 0), (0, 100, 500, 3), (0, 300, 700, 2)])) == ([0, 1, 2], [-1, -1, 1])


def test_by_is_the_smallest_index_among_the_winners():
    iv = S.intervals([(0, 300, 399, 1), (0, 350, 600, 8), (0, 100, 349, 9)])    # 0 loses to both 1 and 2; 1 and 2 do not overlap
    assert _states(iv, 10, 100) == ([2, 1, 1], [1, -1, -1])


def test_staircase_alternates():
    out, st = S.select(S.staircase(41), 0, 0)
    assert out["state"].tolist() == [1, 2] * 20 + [1] and st["pairs"] == st["conflicts"] == 40


# ---- layouts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,jname,py", [("kg_select_params", "KgSelectParams", N.KgSelectParams), ("kg_interval", "KgInterval", N.INTERVAL_DTYPE),
                                            ("kg_selection", "KgSelection", N.SELECTION_DTYPE), ("kg_select_stats", "KgSelectStats", N.KgSelectStats)])
def test_jna_structures_match_the_c_layout(cname, jname, py):
    width = {"int32_t": "int", "uint32_t": "int", "int64_t": "long", "float": "float"}
    cf = H._c_struct(cname)
    jf, order = H._java_struct(jname)
    assert [n for n, _ in jf] == [n for n, _ in cf] == order
    assert [t for _, t in jf] == [width[t] for _, t in cf]
    names = list(py.names) if isinstance(py, np.dtype) else [n for n, _ in py._fields_]
    assert names == [n for n, _ in cf]


def test_dtypes_match_gcc_layout(tmp_path):
    import ctypes as C
    snames = [n for n, _ in N.KgSelectStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%zu %zu %zu %zu\\n", sizeof(kg_interval), sizeof(kg_selection), sizeof(kg_select_params), sizeof(kg_select_stats));\n' +
                   'printf("%d %d %d\\n", KG_SEL_NOT_ELIGIBLE, KG_SEL_SELECTED, KG_SEL_OVERLAPPED);\n' +
                   "".join('printf("%%zu\\n", offsetof(kg_interval, %s));\n' % f for f in N.INTERVAL_DTYPE.names) +
                   "".join('printf("%%zu\\n", offsetof(kg_selection, %s));\n' % f for f in N.SELECTION_DTYPE.names) +
                   "".join('printf("%%zu\\n", offsetof(kg_select_stats, %s));\n' % f for f in snames) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:4] == [20, 8, C.sizeof(N.KgSelectParams), C.sizeof(N.KgSelectStats)] and C.sizeof(N.KgSelectParams) == 12
    assert out[4:7] == [N.SEL_NOT_ELIGIBLE, N.SEL_SELECTED, N.SEL_OVERLAPPED]
    want = ([N.INTERVAL_DTYPE.fields[f][1] for f in N.INTERVAL_DTYPE.names] + [N.SELECTION_DTYPE.fields[f][1] for f in N.SELECTION_DTYPE.names] +
            [getattr(N.KgSelectStats, f).offset for f in snames])
    assert out[7:] == want


def test_pairs_per_lane_matches_the_kernels():
    text = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_select.hpp")).read()
    assert int(re.search(r"constexpr int kSelectPairsPerLane = (\d+);", text).group(1)) == N.SELECT_PAIRS_PER_LANE


# ---- the front end's writers -----------------------------------------------------------------------------------------------

def test_call_regions_select_writers():
    """Regions 0 and 1 give the same ORF (region 1, the stronger, wins it), region 2 stands alone, region 3 is not kept."""
    from kmergutsjava_amd import call_regions as CR
    c1 = HO.A + b"GCT" * 150 + b"TAA"
    off = np.array([0, 7, 7 + len(c1)], np.int64)
    seq = b"ACGTACG" + c1
    regs = O.regions_of([O.region(1, 0, 12, 17, 0, fI=1, score=9), O.region(1, 0, 9, 14, 0, fI=0, score=13, frames=5),
                         O.region(1, 0, 30, 35, 0, fI=1, score=4), O.region(1, 0, 12, 14, 0, fI=1, score=1, kept=0)])
    orfs, ps, res = O.orfs(regs, seq, off, only_kept=False)
    ids, fnames = [b"c0", b"c1"], [b"alpha", b"beta gamma"]
    sel, _ = S.select(S.of_records(orfs))
    assert sel.tolist() == [(2, 1), (1, -1), (1, -1), (0, -1)]
    assert CR.select_summary(sel) == ", selected: 2, overlapped: 1"
    plain = CR.format_regions(ids, regs, fnames).splitlines(True)
    assert len(plain) == 3 and plain[1].startswith(b"c1\t10\t15\t+\talpha\t13\t") and plain[1].endswith(b"\t0,2\tkept\n")
    assert CR.format_regions(ids, regs, fnames, sel=sel, cands=orfs) == plain[1] + plain[2]
    every = CR.format_regions(ids, regs, fnames, True, sel=sel, cands=orfs).splitlines()
    assert [line.split(b"\t")[-2:] for line in every] == [[b"overlapped", b"7..24:+"], [b"kept", b"-"], [b"kept", b"-"], [b"below", b"-"]]
    gff = CR.format_regions(ids, regs, fnames, True, True, sel=sel, cands=orfs).splitlines()
    assert gff[1].endswith(b";status=overlapped;overlapped_by=7..24:+") and gff[4].endswith(b";status=below;overlapped_by=-")
    # on the regions' own extents (no ORFs): 12..17 and 9..14 share 3 of 6 nucleotides, which is not over 50 %
    rsel, _ = S.select(S.of_records(regs))
    assert rsel["state"].tolist() == [1, 1, 1, 0]
    assert CR.format_regions(ids, regs, fnames, sel=rsel) == CR.format_regions(ids, regs, fnames)
    assert CR.format_orfs(ids, regs, orfs, fnames, sel=sel) == (b"c1\t7\t24\t+\t0\talpha\t13\t5\tATG\tstop,multi-frame\n"
                                                                b"c1\t25\t483\t+\t0\tbeta gamma\t4\t152\t-\tstop\n")
    assert len(CR.format_orfs(ids, regs, orfs, fnames, True, sel=sel).splitlines()) == 4
    # under --select the writer's own dedupe by equal coordinates finds nothing left to do
    faa = CR.format_faa(ids, regs, orfs, ps, res, fnames, sel=sel)
    assert faa == CR.format_faa(ids, regs, O.orfs(regs, seq, off)[0], *O.orfs(regs, seq, off)[1:], fnames) and faa.count(b">") == 2


# ---- round trip ------------------------------------------------------------------------------------------------------------

def with_decoys(regs, start, off, seed=3):
    """The regions plus, per kept region, a short decoy inside it on the other strand with a tenth of its score, in the
    library's output order.  -> (records, is_decoy)."""
    rng = np.random.default_rng(seed)
    kept = regs[regs["kept"] != 0]
    dec = kept.copy()
    length = kept["right"] - kept["left"] + 1
    dl = np.maximum(length // 4, 1)
    dec["left"] = kept["left"] + rng.integers(0, np.maximum(length - dl, 1))
    dec["right"] = np.minimum(dec["left"] + dl - 1, kept["right"])
    dec["strand"] ^= 1
    dec["score"] = kept["score"] // 10
    dec["fI"] = 10 ** 6
    both = np.concatenate([regs, dec])
    is_decoy = np.concatenate([np.zeros(len(regs), bool), np.ones(len(dec), bool)])
    order = np.lexsort((both["fI"], both["strand"], both["right"], both["left"], both["seq"]))
    return both[order], is_decoy[order]


def planted_selection(img, dna, off, genes, calls):
    """-> (records with decoys, is_decoy, selection, planted genes with a kept region, of those still selected)."""
    regs, start = R.regions(calls, off, 300, 10, 90)
    both, is_decoy = with_decoys(regs, start, off)
    sel, _ = S.select(S.of_records(both))
    found = still = 0
    for c, left, right, strand, f, shifted, prot in genes:
        hit = np.flatnonzero((both["seq"] == c) & ~is_decoy & (both["kept"] != 0) & (both["strand"] == strand) & (both["fI"] == f) &
                             (both["left"] <= right) & (both["right"] >= left))
        found += bool(len(hit))
        still += bool((sel["state"][hit] == 1).any())
    return both, is_decoy, sel, found, still


def test_round_trip_planted_genes_outlive_their_decoys(oracle):
    img, dna, off, genes = HO.planted_orf_contigs()
    calls = oracle.run(img, np.frombuffer(dna, dtype=np.uint8), off, lookup_mode=1)["calls"]
    both, is_decoy, sel, found, still = planted_selection(img, dna, off, genes, calls)
    iv = S.of_records(both)
    print("planted genes %d, with a kept region %d, of those still selected %d; decoys %d, removed %d; regions %d, kept %d, selected %d" %
          (len(genes), found, still, int(is_decoy.sum()), int((sel["state"][is_decoy] == 2).sum()), int((~is_decoy).sum()),
           int((both["kept"][~is_decoy] != 0).sum()), int((sel["state"][~is_decoy] == 1).sum())))
    S.check_properties(iv, sel, 60, 50)
    # a candidate that is the strongest among everything it conflicts with is never overlapped (by construction of the rule)
    rank = {i: k for k, i in enumerate(S.strength_order(iv))}
    for i in rank:
        if is_decoy[i]:
            continue
        rivals = np.flatnonzero((iv["seq"] == iv["seq"][i]) & (iv["eligible"] != 0) & (iv["left"] <= iv["right"][i]) & (iv["right"] >= iv["left"][i]))
        if all(rank[j] >= rank[i] for j in rivals if S.conflict(iv[i], iv[j], 60, 50)):
            assert sel["state"][i] == 1, i
    assert is_decoy.sum() > 20 and found > 20
