"""Evidence-free open reading frames without a GPU: the numpy form of tests/free_orfs_model.py against its plain loops, known
answers worked out by hand, kg_free_params against the C layout and the JNA source, the planted genes (every unshifted one must
come back, 80 of 80), the call_regions writers, and the selection invariant (free ORFs never change an evidence ORF's state)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import free_orfs_model as F  # noqa: E402
import orfs_model as O  # noqa: E402
import regions_model as R  # noqa: E402
import select_model as S  # noqa: E402
import test_orfs_host as HO  # noqa: E402
import test_regions_host as H  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

ROOT = os.path.dirname(HERE)
A = HO.A                                # codons 0 TAA 1 CCC 2 ATG 3 AAA 4 GGG 5 CCC 6 TTT 7 TAG 8 AAA 9 CCC


def _both(seq, off, min_res, sc=7):
    a, b = F.free_orfs(seq, off, min_res, sc), F.brute_force(seq, off, min_res, sc)
    assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))
    return a


def _one(contig: bytes, strand: int, f: int, min_res: int, sc: int = 7):
    """[(left, right, n_res, start_codon, flags, protein)] of one container of one contig"""
    o, ps, res = _both(contig, np.array([0, len(contig)], np.int64), min_res, sc)
    text = res.tobytes().decode()
    return [(int(r["left"]), int(r["right"]), int(r["n_res"]), int(r["start_codon"]), int(r["flags"]), text[ps[i]:ps[i + 1]])
            for i, r in enumerate(o) if r["strand"] == strand and r["frame"] == f]


@pytest.mark.parametrize("seed", range(300))
def test_numpy_form_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    # GC-rich: stops are rare enough to give candidates at small min_res
    weights = None if seed % 3 == 0 else np.array([6, 40, 40, 6, 1, 2, 2, 2, 0, 1, 0], float) / 100
    _, seq, off = O.random_batch(rng, int(rng.integers(0, 8)), max_len=int(rng.choice([8, 60, 400])), max_regions=0, weights=weights)
    min_res, sc = int(rng.choice([1, 2, 3, 5, 10, 30])), int(rng.integers(0, 8))
    o, ps, res = _both(seq, off, min_res, sc)
    assert ps[0] == 0 and ps[-1] == len(res) and (np.diff(ps) == o["n_res"]).all() and (o["n_res"] >= min_res).all()
    assert ((o["flags"] & F.FREE) != 0).all() and ((o["flags"] & (O.INTERRUPTED | O.MULTI_FRAME)) == 0).all() and b"*" not in res.tobytes()
    assert (o["score"] == 0).all() and (o["kept"] == 1).all() and (o["fI"] == -1).all() and (o["first_inner"] == -1).all()
    key = np.stack([o["seq"], o["strand"], o["frame"], np.where(o["strand"] == 0, o["left"], -o["right"])])
    assert all(tuple(key[:, i]) < tuple(key[:, i + 1]) for i in range(len(o) - 1)), "rule 6: container order, then increasing b"


@pytest.mark.parametrize("n", range(9))
def test_contigs_of_length_0_to_8(n):
    for text in (b"ATGAAATA"[:n], b"TAAATGCC"[:n], b"NNNNNNNN"[:n], b"CATTTACA"[:n]):
        for min_res in (1, 2):
            o, _, _ = _both(text, np.array([0, n], np.int64), min_res, 7)
            assert len(o) <= 6 * (n // 3 + 1)


def test_known_answers_plus_and_minus_of_one_contig():
    """A, frame 0, min_res 1.  Runs: (-1, 0) is empty.  (0, 7): b = 2 (ATG), codons 2..7 = x 6..23, M K G P F, HAS_STOP.
    (7, n_f = 10): no start and u >= 0: nothing.  The reverse complement's '-' strand reads the same text: left 29 - 23 = 6,
    right 29 - 6 = 23."""
    want = [(6, 23, 5, 1, F.FREE | O.HAS_STOP, "MKGPF")]
    assert _one(A, 0, 0, 1) == want and _one(A, 0, 0, 5) == want and _one(A, 0, 0, 6) == []
    assert _one(HO._rc(A), 1, 0, 1) == want
    # start_codons = 0: the same runs begin behind their stop.  (0, 7): codons 1..7 = x 3..23, P M K G P F; (7, 10): codons
    # 8..9 = x 24..29, K P, no HAS_STOP (e = n_f)
    assert _one(A, 0, 0, 1, 0) == [(3, 23, 6, 0, F.FREE | O.HAS_STOP, "PMKGPF"), (24, 29, 2, 0, F.FREE, "KP")]
    assert _one(HO._rc(A), 1, 0, 1, 0) == [(6, 26, 6, 0, F.FREE | O.HAS_STOP, "PMKGPF"), (0, 5, 2, 0, F.FREE, "KP")]


def test_known_answer_first_run_without_a_start_is_partial5_from_codon_0():
    """CCC AAA GGG TAA CCC (+ A): (-1, 3) has no start and u == -1: b = 0, codons 0..3 = x 0..11, P K G, PARTIAL5 | HAS_STOP.
    (3, n_f = 5): CCC alone, no start, u >= 0: nothing.  With a GTG in the first run b moves to it and PARTIAL5 stays."""
    assert _one(b"CCCAAAGGGTAACCCA", 0, 0, 1) == [(0, 11, 3, 0, F.FREE | O.HAS_STOP | O.PARTIAL5, "PKG")]
    assert _one(b"CCCGTGGGGTAACCCA", 0, 0, 1) == [(3, 11, 2, 2, F.FREE | O.HAS_STOP | O.PARTIAL5, "MG")]


def test_known_answer_the_run_that_reaches_the_end_has_no_stop_flag():
    """TAA ATG CCC AA: (0, n_f = 3): b = 1, codons 1..2 = x 3..8 (right on the last whole codon), M P, flags FREE alone.
    A stopless contig: one run (-1, n_f), PARTIAL5 without HAS_STOP."""
    assert _one(b"TAAATGCCCAA", 0, 0, 1) == [(3, 8, 2, 1, F.FREE, "MP")]
    assert _one(b"CCC" * 5 + b"AA", 0, 0, 1) == [(0, 14, 5, 0, F.FREE | O.PARTIAL5, "PPPPP")]
    assert _one(b"CCC" * 5 + b"AA", 0, 0, 6) == []


def test_known_answer_n_in_a_stop_is_no_stop():
    """TAA ATG TNA AAA TAG: TNA is unknown, neither stop nor start: one run (0, 4), M X K."""
    assert _one(b"TAAATGTNAAAATAG", 0, 0, 1) == [(3, 14, 3, 1, F.FREE | O.HAS_STOP, "MXK")]
    # a run of N's is a run (stated, not repaired)
    assert _one(b"N" * 12, 0, 0, 1) == [(0, 11, 4, 0, F.FREE | O.PARTIAL5, "XXXX")]


def test_known_answer_min_res_boundary():
    """TAA CCC ATG + k x AAA + TAG: n_res = k + 1 from the ATG."""
    for k in (3, 4, 5):
        got = _one(b"TAACCCATG" + b"AAA" * k + b"TAG", 0, 0, 5)
        assert got == ([(6, 11 + 3 * k, k + 1, 1, F.FREE | O.HAS_STOP, "M" + "K" * k)] if k + 1 >= 5 else [])


# ---- layouts ---------------------------------------------------------------------------------------------------------------

def test_free_params_match_the_c_layout_and_the_jna_source(tmp_path):
    import ctypes as C
    cf = H._c_struct("kg_free_params")
    jf, order = H._java_struct("KgFreeParams")
    assert [n for n, _ in jf] == [n for n, _ in cf] == order == [n for n, _ in N.KgFreeParams._fields_] == ["min_res", "start_codons", "reserved"]
    assert [t for _, t in jf] == ["int"] * 3 and [t for _, t in cf] == ["int32_t"] * 3 and N.FREE_PARAMS is N.KgFreeParams
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n'
                   'printf("%zu %u\\n", sizeof(kg_free_params), KG_ORF_FREE);\n' +
                   "".join('printf("%%zu\\n", offsetof(kg_free_params, %s));\n' % f for f, _ in cf) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(N.KgFreeParams), N.ORF_FREE] + [getattr(N.KgFreeParams, f).offset for f, _ in cf] == [12, 16, 0, 4, 8]
    assert N.ORF_FREE == F.FREE and {"kg_orfs_free", "kg_orfset_add_free"} <= set(N.EXPORTS)


# ---- planted genes -----------------------------------------------------------------------------------------------------------

_WORK = {}


def _planted():
    if not _WORK:
        img, dna, off, genes = HO.planted_orf_contigs()
        _WORK["w"] = (img, dna, off, genes, F.free_orfs(dna, off, 100, 7))
    return _WORK["w"]


def test_every_unshifted_planted_gene_has_a_free_candidate():
    """The genes are ATG + stop-free back-translation + TAA and the table plays no part: 80 of 80, not a share."""
    _, dna, off, genes, (orfs, ps, res) = _planted()
    text = res.tobytes().decode()
    found = total = 0
    for c, left, right, strand, _, shifted, prot in genes:
        if shifted:
            continue
        total += 1
        hit = np.flatnonzero((orfs["seq"] == c) & (orfs["strand"] == strand) & ((orfs["left"] if strand else orfs["right"]) == (left if strand else right)))
        assert len(hit) == 1 and orfs["flags"][hit[0]] & O.HAS_STOP, (c, left, right, strand)
        assert text[ps[hit[0]]:ps[hit[0] + 1]].endswith(prot), (c, left, right, strand)
        found += 1
    assert (found, total) == (80, 80)


def test_free_orfs_never_change_an_evidence_orfs_selection(oracle):
    img, dna, off, genes, free = _planted()
    ora = oracle.run(img, np.frombuffer(dna, dtype=np.uint8), off, lookup_mode=1)
    regs, start = R.regions(ora["calls"], off, 300, 10, 90)
    ev = O.orfs(regs, dna, off)
    assert len(regs) > 20 and regs["score"][regs["kept"] != 0].min() >= 2
    both = F.concat(ev, free)
    selected_stops = None
    for mo, pct in ((60, 50), (0, 0), (1000, 100)):
        alone = S.select_fast(S.of_records(ev[0]), mo, pct)
        sel = S.select_fast(S.of_records(both[0]), mo, pct)
        assert sel[:len(regs)].tobytes() == alone.tobytes()
        S.check_properties(S.of_records(both[0]), sel, mo, pct)
        if (mo, pct) == (60, 50):
            o = both[0][sel["state"] == 1]
            ends = set(zip(o["seq"].tolist(), o["strand"].tolist(), np.where(o["strand"] == 1, o["left"], o["right"]).tolist()))
            selected_stops = sum((c, strand, left if strand else right) in ends for c, left, right, strand, _, shifted, _ in genes if not shifted)
    print("planted unshifted genes with a selected candidate ending on their stop: %d of 80 (evidence ORFs: %d, free ORFs: %d)" %
          (selected_stops, len(regs), len(free[0])))


# ---- the front end's writers -----------------------------------------------------------------------------------------------

def test_call_regions_free_writers():
    """Contigs c0 (no region) and c1 = A + 150 x GCT + TAA with two regions.  Free ORFs of min_res 5 on c1 '+' frame 0: the run
    (0, 7) = x 6..23 (the extent region 0's ORF has: the FASTA keeps the region's name) and (7, 159) = x 24..479 without a
    start: nothing; on other frames whatever the model gives."""
    from kmergutsjava_amd import call_regions as CR
    c1 = A + b"GCT" * 150 + b"TAA"
    off = np.array([0, 7, 7 + len(c1)], np.int64)
    seq = b"ACGTACG" + c1
    regs = O.regions_of([O.region(1, 0, 12, 17, 0, fI=1, score=9), O.region(1, 0, 30, 35, 0, fI=0, score=4)])
    orfs, ps, res = O.orfs(regs, seq, off)
    free, fps, fres = F.free_orfs(seq, off, 5, 7)
    ids, fnames = [b"c0", b"c1"], [b"alpha", b"beta gamma"]
    assert len(free) >= 2 and (free["seq"] == 1).all()
    same = np.flatnonzero((free["strand"] == 0) & (free["left"] == 6) & (free["right"] == 23))
    assert len(same) == 1
    text = CR.format_orfs(ids, regs, orfs, fnames, free=free)
    lines = text.splitlines()
    assert lines[:2] == CR.format_orfs(ids, regs, orfs, fnames).splitlines() and len(lines) == 2 + len(free)
    assert b"c1\t7\t24\t+\t0\thypothetical protein\t0\t5\tATG\tstop,free" in lines[2:]
    assert all(ln.split(b"\t")[5] == b"hypothetical protein" and ln.split(b"\t")[6] == b"0" and b"free" in ln.split(b"\t")[9].split(b",")
               for ln in lines[2:])
    faa = CR.format_faa(ids, regs, orfs, ps, res, fnames, free=free, free_prot_start=fps, free_residues=fres)
    assert faa.startswith(CR.format_faa(ids, regs, orfs, ps, res, fnames))
    assert faa.count(b">") == 2 + len(free) - 1 and faa.count(b">c1_7_24_+ ") == 1 and b">c1_7_24_+ beta gamma\nMKGPF\n" in faa
    assert faa.count(b" hypothetical protein\n") == len(free) - 1
    # with a selection: only the selected are written; with --all every line and the free ones' status and winner
    cands = np.concatenate([orfs, free])
    sel = S.select_fast(S.of_records(cands))
    assert sel["state"][len(regs) + same[0]] == 2 and sel["by"][len(regs) + same[0]] == 0
    chosen = CR.format_orfs(ids, regs, orfs, fnames, sel=sel[:2], free=free, free_sel=sel[2:], cands=cands).splitlines()
    assert len(chosen) == int((sel["state"] == 1).sum())
    every = CR.format_orfs(ids, regs, orfs, fnames, True, sel[:2], free, sel[2:], cands).splitlines()
    assert len(every) == 2 + len(free)
    assert b"c1\t7\t24\t+\t0\thypothetical protein\t0\t5\tATG\tstop,free\toverlapped\t7..24:+" in every
    assert sum(ln.endswith(b"\tkept\t-") for ln in every) == int((sel["state"][2:] == 1).sum())
    # contig order: a free ORF of c0 stands in front of c1's lines
    free0 = free[:1].copy()
    free0["seq"] = 0
    mixed = CR.format_orfs(ids, regs, orfs, fnames, free=np.concatenate([free0, free])).splitlines()
    assert mixed[0].startswith(b"c0\t") and mixed[1:3] == lines[:2]
    # without free ORFs every writer gives what it gave
    assert CR.format_orfs(ids, regs, orfs, fnames, free=None) == CR.format_orfs(ids, regs, orfs, fnames)
    with pytest.raises(ValueError):
        CR.call_regions("nowhere", "none.fna", "out.tsv", free_min_res=100)
    assert CR.main(["-D", "d", "-q", "q", "-o", "o", "--orfs", "x", "--free-orfs", "--min-res", "0"]) == 1     # (no data directory either)
