"""Open reading frames without a GPU: the numpy model of tests/orfs_model.py against plain loops, known answers worked out by
hand, the new structures against the C layout, the call_regions writers, and the round trip on the CPU (planted genes -> the
oracle's DNA scan -> regions_model -> orfs_model gives back the planted stop and protein)."""
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
import test_regions_host as H  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

ROOT = os.path.dirname(HERE)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _rc(dna: bytes) -> bytes:
    return dna.translate(_COMP)[::-1]


def _one(contig: bytes, reg, **kw):
    """(record, protein text) of one region on one contig, from the model, checked against the plain loops"""
    off = np.array([0, len(contig)], np.int64)
    regs = O.regions_of([reg])
    a = O.orfs(regs, contig, off, **kw)
    b = O.brute_force(regs, contig, off, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    return a[0][0], a[2].tobytes().decode()


@pytest.mark.parametrize("seed", range(300))
def test_model_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    weights = None if seed % 3 else np.array([30, 10, 10, 30, 2, 2, 2, 2, 2, 5, 5], float) / 100     # AT-rich: more stops and starts
    regs, seq, off = O.random_batch(rng, int(rng.integers(0, 8)), max_len=int(rng.choice([12, 60, 400])), weights=weights)
    sc, ok = int(rng.integers(0, 8)), bool(seed % 2)
    a = O.orfs(regs, seq, off, sc, ok)
    b = O.brute_force(regs, seq, off, sc, ok)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert a[1][0] == 0 and a[1][-1] == len(a[2]) and (np.diff(a[1]) >= 0).all()
    assert (np.diff(a[1]) == np.where(a[0]["kept"] | (not ok), a[0]["n_res"], 0)).all()


A = b"TAACCCATGAAAGGGCCCTTTTAGAAACCC"          # codons 0 TAA 1 CCC 2 ATG 3 AAA 4 GGG 5 CCC 6 TTT 7 TAG 8 AAA 9 CCC


def test_known_answer_plus_and_minus_of_one_contig():
    """'+', frame 1 of G + A (L = 31): the region is codons 4..5 = x 13..18.  u = 0 (TAA), e = 7 (TAG), b = the first start in
    (0, 4] = 2 (ATG).  ORF = codons 2..7 = x 7..24; n_res = 7 - 2 = 5: M K G P F; flags = HAS_STOP.
    '-' of the reverse complement (the same strand text): the region x 13..18 is left 30 - 18 = 12, right 30 - 13 = 17; the ORF
    x 7..24 is left 30 - 24 = 6, right 30 - 7 = 23."""
    c = b"G" + A
    o, p = _one(c, O.region(0, 0, 13, 18, 1))
    assert (o["strand"], o["frame"], o["left"], o["right"], o["n_res"], o["start_codon"], o["first_inner"], o["flags"]) == \
        (0, 1, 7, 24, 5, 1, -1, O.HAS_STOP)
    assert p == "MKGPF"
    o, p = _one(_rc(c), O.region(0, 1, 12, 17, 1))
    assert (o["strand"], o["frame"], o["left"], o["right"], o["n_res"], o["start_codon"], o["flags"]) == (1, 1, 6, 23, 5, 1, O.HAS_STOP)
    assert p == "MKGPF"


def test_known_answer_gtg_start_reads_m():
    """A with codon 2 = GTG: b = 2 as before, start_codon = 2, and residue 0 is M although GTG codes for V."""
    o, p = _one(A.replace(b"ATG", b"GTG"), O.region(0, 0, 12, 17, 0))
    assert (o["left"], o["right"], o["start_codon"]) == (6, 23, 2) and p == "MKGPF"


def test_known_answer_no_start_begins_behind_the_stop():
    """A with codon 2 = CTG: no start in (0, 4], so b = u + 1 = 1.  ORF = codons 1..7 = x 3..23, n_res = 6: P L K G P F."""
    o, p = _one(A.replace(b"ATG", b"CTG"), O.region(0, 0, 12, 17, 0))
    assert (o["left"], o["right"], o["n_res"], o["start_codon"], o["flags"]) == (3, 23, 6, 0, O.HAS_STOP) and p == "PLKGPF"


def test_known_answer_no_stop_either_side():
    """CCC x 5 + AA (L = 17, frame 0, n_f = 5), region = codon 2 = x 6..8: u = -1, e = n_f = 5, b = 0.  ORF = codons 0..4, right
    on the last whole codon = 14 (not 16); n_res = 5; PARTIAL5 and no HAS_STOP."""
    o, p = _one(b"CCC" * 5 + b"AA", O.region(0, 0, 6, 8, 0))
    assert (o["left"], o["right"], o["n_res"], o["start_codon"], o["flags"]) == (0, 14, 5, 0, O.PARTIAL5) and p == "PPPPP"


def test_known_answer_inner_stop():
    """A with codon 5 = TGA, region = codons 4..6 = x 12..20: i* = 5 <= j1 = 6, first_inner = 5 - b = 3; e = 7 still (the first
    stop behind j1).  Protein M K G * F."""
    c = A[:15] + b"TGA" + A[18:]
    o, p = _one(c, O.region(0, 0, 12, 20, 0))
    assert (o["left"], o["right"], o["n_res"], o["first_inner"], o["flags"]) == (6, 23, 5, 3, O.HAS_STOP | O.INTERRUPTED)
    assert p == "MKG*F"


def test_known_answer_start_codon_mask():
    """TAA TTG CCC ATG AAA GGG TAG, region = codon 4 = x 12..14.  With 7: b = 1 (TTG), start_codon 3, n_res = 6 - 1 = 5,
    M P M K G.  With 1 (ATG only): b = 3, n_res = 3, M K G.  With 0: b = u + 1 = 1 and TTG reads L."""
    c = b"TAATTGCCCATGAAAGGGTAG"
    o, p = _one(c, O.region(0, 0, 12, 14, 0), start_codons=7)
    assert (o["left"], o["n_res"], o["start_codon"]) == (3, 5, 3) and p == "MPMKG"
    o, p = _one(c, O.region(0, 0, 12, 14, 0), start_codons=1)
    assert (o["left"], o["n_res"], o["start_codon"]) == (9, 3, 1) and p == "MKG"
    o, p = _one(c, O.region(0, 0, 12, 14, 0), start_codons=0)
    assert (o["left"], o["n_res"], o["start_codon"]) == (3, 5, 0) and p == "LPMKG"


def test_known_answer_n_in_a_stop_is_no_stop():
    """TAA CCC TNA AAA TAG, region = codon 3 = x 9..11: TNA is unknown, not a stop, so u = 0 and b = 1; residues P X K."""
    o, p = _one(b"TAACCCTNAAAATAG", O.region(0, 0, 9, 11, 0))
    assert (o["left"], o["right"], o["n_res"], o["flags"]) == (3, 14, 3, O.HAS_STOP) and p == "PXK"


def test_multi_frame_flag_and_only_kept():
    off = np.array([0, len(A)], np.int64)
    regs = O.regions_of([O.region(0, 0, 12, 17, 0, frames=3, kept=0), O.region(0, 0, 12, 17, 0, kept=1)])
    o, ps, res = O.orfs(regs, A, off)
    assert o["flags"].tolist() == [O.HAS_STOP | O.MULTI_FRAME, O.HAS_STOP] and ps.tolist() == [0, 0, 5] and o["n_res"].tolist() == [5, 5]
    assert O.orfs(regs, A, off, only_kept=False)[1].tolist() == [0, 5, 10]


# ---- layouts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,jname,py", [("kg_orf_params", "KgOrfParams", "KgOrfParams"), ("kg_orf", "KgOrf", None),
                                            ("kg_orf_stats", "KgOrfStats", "KgOrfStats")])
def test_jna_structures_match_the_c_layout(cname, jname, py):
    width = {"int32_t": "int", "uint32_t": "int", "int64_t": "long", "float": "float"}
    cf = H._c_struct(cname)
    jf, order = H._java_struct(jname)
    assert [n for n, _ in jf] == [n for n, _ in cf] == order
    assert [t for _, t in jf] == [width[t] for _, t in cf]
    if py:
        assert [n for n, _ in getattr(N, py)._fields_] == [n for n, _ in cf]
    else:
        assert list(N.ORF_DTYPE.names) == [n for n, _ in cf] and N.ORF_DTYPE.itemsize == 48


def test_orf_dtype_matches_gcc_layout(tmp_path):
    import ctypes as C
    names = list(N.ORF_DTYPE.names)
    snames = [n for n, _ in N.KgOrfStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%zu %zu %zu\\n", sizeof(kg_orf), sizeof(kg_orf_params), sizeof(kg_orf_stats));\n' +
                   'printf("%u %u %u %u\\n", KG_ORF_HAS_STOP, KG_ORF_PARTIAL5, KG_ORF_INTERRUPTED, KG_ORF_MULTI_FRAME);\n' +
                   "".join('printf("%%zu\\n", offsetof(kg_orf, %s));\n' % f for f in names) +
                   "".join('printf("%%zu\\n", offsetof(kg_orf_stats, %s));\n' % f for f in snames) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [48, 12, C.sizeof(N.KgOrfStats)] and C.sizeof(N.KgOrfParams) == 12
    assert out[3:7] == [N.ORF_HAS_STOP, N.ORF_PARTIAL5, N.ORF_INTERRUPTED, N.ORF_MULTI_FRAME] == [O.HAS_STOP, O.PARTIAL5, O.INTERRUPTED, O.MULTI_FRAME]
    assert out[7:7 + len(names)] == [N.ORF_DTYPE.fields[f][1] for f in names]
    assert out[7 + len(names):] == [getattr(N.KgOrfStats, f).offset for f in snames]


def test_tile_constant_and_genetic_code_match_the_kernels():
    csrc = os.path.join(ROOT, "kmergutsjava_amd", "csrc")
    assert int(re.search(r"constexpr int kOrfTile = (\d+);", open(os.path.join(csrc, "kg_orfs.hpp")).read()).group(1)) == N.ORF_TILE_CODONS
    assert re.search(r'kGeneticCode\[65\] = "([A-Z*]{64})"', open(os.path.join(csrc, "kg_device.hpp")).read()).group(1) == O.GENETIC_CODE


# ---- the front end's writers -----------------------------------------------------------------------------------------------

def test_call_regions_orf_writers():
    """Contig c1 = A + 150 x GCT + TAA: region 0 (fI 1, score 9) and region 1 (fI 0, score 13) give the same ORF (the second
    wins the FASTA header), region 2 lies behind the TAG and runs to the end (a 152-residue protein: three FASTA lines), region 3
    is not kept."""
    from kmergutsjava_amd import call_regions as CR
    c1 = A + b"GCT" * 150 + b"TAA"
    off = np.array([0, 7, 7 + len(c1)], np.int64)
    seq = b"ACGTACG" + c1
    regs = O.regions_of([O.region(1, 0, 12, 17, 0, fI=1, score=9), O.region(1, 0, 9, 14, 0, fI=0, score=13, frames=5),
                         O.region(1, 0, 30, 35, 0, fI=1, score=4), O.region(1, 0, 12, 14, 0, fI=1, score=1, kept=0)])
    orfs, ps, res = O.orfs(regs, seq, off)
    ids, fnames = [b"c0", b"c1"], [b"alpha", b"beta gamma"]
    assert CR.format_orfs(ids, regs, orfs, fnames) == (b"c1\t7\t24\t+\t0\tbeta gamma\t9\t5\tATG\tstop\n"
                                                       b"c1\t7\t24\t+\t0\talpha\t13\t5\tATG\tstop,multi-frame\n"
                                                       b"c1\t25\t483\t+\t0\tbeta gamma\t4\t152\t-\tstop\n")
    assert CR.format_orfs(ids, regs, orfs, fnames, write_all=True).endswith(b"c1\t7\t24\t+\t0\tbeta gamma\t1\t5\tATG\tstop\n")
    long = b"KP" + b"A" * 150
    want = b">c1_7_24_+ alpha\nMKGPF\n>c1_25_483_+ beta gamma\n" + long[:60] + b"\n" + long[60:120] + b"\n" + long[120:] + b"\n"
    assert CR.format_faa(ids, regs, orfs, ps, res, fnames) == want
    assert CR.orf_summary(orfs) == ", orfs: 4, complete: 3, interrupted: 0"
    # no stop in front, N inside: words joined by commas, no start
    o2 = O.orfs(O.regions_of([O.region(0, 0, 0, 5, 0)]), b"CCNCCCC", np.array([0, 7], np.int64))
    assert CR.format_orfs([b"x"], O.regions_of([O.region(0, 0, 0, 5, 0)]), o2[0], []) == b"x\t1\t6\t+\t0\t7\t5\t2\t-\tpartial5\n"
    assert CR.parse_start_codons("ATG,GTG,TTG") == 7 and CR.parse_start_codons("ttg") == 4 and CR.parse_start_codons("none") == 0
    with pytest.raises(ValueError):
        CR.parse_start_codons("CTG")


# ---- round trip ------------------------------------------------------------------------------------------------------------

def planted_orf_contigs(seed=5, n_fam=40, per=8, n_contigs=30, genes_per=4):
    """test_regions_host.planted_contigs with every gene planted as ATG + back-translation + TAA.
    -> (image, dna, offsets, genes) with genes = (contig, left, right, strand, function, shifted, protein)."""
    import torch
    import signature_model as M
    from kmergutsjava_amd import synth
    from kmergutsjava_amd.make_table import default_num_sigs
    seq, off, fn, otu = M.family_set(n_fam, per, 300, 0.04, 71 + seed)
    sigs = M.derive(seq, off, fn, otu)
    rec, _ = synth.build_table(torch.from_numpy(sigs["kmer"].copy()),
                               tuple(torch.from_numpy(sigs[k].copy()) for k in ("otuIndex", "avgFromEnd", "functionIndex", "functionWt")),
                               default_num_sigs(len(sigs)))
    fam = np.arange(len(fn)) // per
    fam_fn = np.array([np.bincount(fn[(fam == k) & (fn >= 0)]).argmax() for k in range(n_fam)])
    rng = np.random.default_rng(seed)
    contigs, genes = [], []
    for c in range(n_contigs):
        parts, at = [], 0
        for g in range(genes_per):
            sp = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(700, 1500))))
            parts.append(sp)
            at += len(sp)
            p = int(rng.integers(0, len(fn)))
            prot = seq[off[p]:off[p + 1]].decode()
            dna = b"ATG" + synth.back_translate(prot).encode() + b"TAA"
            shifted = (c * genes_per + g) % 3 == 0
            if shifted:
                mid = len(dna) // 2
                dna = dna[:mid] + dna[mid + 1:]
            strand = int(rng.integers(0, 2))
            if strand:
                dna = _rc(dna)
            genes.append((c, at, at + len(dna) - 1, strand, int(fam_fn[fam[p]]), shifted, "M" + prot))
            parts.append(dna)
            at += len(dna)
        contigs.append(b"".join(parts))
    coff = np.zeros(n_contigs + 1, dtype=np.int64)
    coff[1:] = np.cumsum([len(x) for x in contigs])
    return synth.table_image(rec), b"".join(contigs), coff, genes


def recovered_genes(regs, start, orfs, pstart, res, genes):
    """(checked, planted unshifted genes): a gene is checked when a single-frame region of its strand and function overlaps it;
    its ORF must then end on the planted stop and its protein must end with the planted one."""
    text = res.tobytes().decode()
    checked = unshifted = 0
    for c, left, right, strand, f, shifted, prot in genes:
        if shifted:
            continue
        unshifted += 1
        sl = slice(int(start[c]), int(start[c + 1]))
        r = regs[sl]
        hit = np.flatnonzero((r["strand"] == strand) & (r["fI"] == f) & (r["left"] <= right) & (r["right"] >= left) &
                             ((r["frames"] & (r["frames"] - 1)) == 0))
        if not len(hit):
            continue
        checked += 1
        for k in hit + sl.start:
            o = orfs[k]
            assert o["flags"] & O.HAS_STOP and not o["flags"] & O.INTERRUPTED, (c, left, right, strand, o)
            assert (o["left"] if strand else o["right"]) == (left if strand else right), (c, left, right, strand, o)
            assert text[pstart[k]:pstart[k + 1]].endswith(prot), (c, left, right, strand, o)
    return checked, unshifted


def test_round_trip_gives_back_planted_stop_and_protein(oracle):
    img, dna, off, genes = planted_orf_contigs()
    ora = oracle.run(img, np.frombuffer(dna, dtype=np.uint8), off, lookup_mode=1)
    regs, start = R.regions(ora["calls"], off)
    orfs, pstart, res = O.orfs(regs, dna, off, only_kept=False)
    checked, unshifted = recovered_genes(regs, start, orfs, pstart, res, genes)
    print("planted genes %d, unshifted %d, checked (single-frame region found) %d = %.3f of the planted" %
          (len(genes), unshifted, checked, checked / len(genes)))
    assert checked >= 1
