"""The rule of kg_contigs_search_translated on the host: translated_model against answers known by hand.  A target is planted
into a contig with synth.back_translate, a stop codon directly in front of it and behind it, so its fragment is the target and the
CALL's span is the gene's; the contig's ends are runs of A (K on '+', F on '-': no stop in any frame).  The argument checks of
hotpath's wrappers and of the C entry point run without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orfs_model as O
import regions_model as R
import repair_model as RP
import search_model as S
import translated_model as TM
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import hotpath as H
from kmergutsjava_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = "ACDEFGHIKLMNPQRSTVWY"
STOP = "TAA"


def _protein(rng, n: int) -> str:
    return "".join(ALPHA[int(x)] for x in rng.integers(0, 20, n))


def _revcomp(dna: str) -> str:
    return dna[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _contig(gene_dna: str, lead: int, tail: int, strand: int, stop_behind: bool = True) -> bytes:
    """lead A's, a stop, the gene, a stop, tail A's, read on `strand`: the gene's first nucleotide is strand position lead + 3."""
    dna = "A" * lead + STOP + gene_dna + (STOP + "A" * tail if stop_behind else "")
    return (dna if strand == 0 else _revcomp(dna)).encode()


def _batch(contigs):
    return S.batch(list(contigs))


# ---- one planted gene: both strands, the three frames, L mod 3 ------------------------------------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("lead", [30, 31, 32])
@pytest.mark.parametrize("tail", [33, 34, 35])
def test_a_planted_gene_is_one_call_at_its_coordinates(strand, lead, tail):
    rng = np.random.default_rng(100 * strand + 10 * lead + tail)
    target = _protein(rng, 40)
    tseq, toff = S.batch([target.encode()])
    seq, off = _batch([_contig(synth.back_translate(target), lead, tail, strand)])
    L = int(off[1])
    assert L % 3 == (lead + tail) % 3 and {(30 + t) % 3 for t in (33, 34, 35)} == {0, 1, 2}
    m = TM.translated_model(seq, off, tseq, toff)
    assert len(m["calls"]) == 1 and m["call_hits"].tolist() == [0] and sum(m["drops"].values()) == 0
    c = m["calls"][0]
    assert int(c["container"]) == 3 * strand + lead % 3 and int(c["fI"]) == 0
    assert int(c["count"]) == int(m["hits"][0]["score"]) == int(m["hits"][0]["self_target"]) and float(c["weightedHits"]) == float(c["count"])
    sq, st, fr, x0, x1, Ls = R.spans(m["calls"], off)
    assert (int(sq[0]), int(st[0]), int(fr[0]), int(x0[0]), int(x1[0]), int(Ls[0])) == (0, strand, lead % 3, lead + 3, lead + 3 + 119, L)
    # the fragment is the target, between its two stops
    frags, pstart, res = m["fragments"]
    q = int(m["hits"][0]["query"])
    assert res[pstart[q]:pstart[q + 1]].tobytes() == target.encode()
    regs, _ = R.regions(m["calls"], off)
    want = (lead + 3, lead + 122) if strand == 0 else (L - 1 - (lead + 122), L - 1 - (lead + 3))
    assert len(regs) == 1 and (int(regs[0]["left"]), int(regs[0]["right"])) == want and int(regs[0]["strand"]) == strand


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("dangling", [0, 1, 2])
def test_a_gene_cut_by_the_contig_s_end_is_found_with_its_extent(strand, dangling):
    """The first 35 residues of a 40-residue target, then 0, 1 or 2 nucleotides of the next codon, then the contig's 3' end: no
    stop behind it, and it is still a fragment (the run that reaches the end)."""
    rng = np.random.default_rng(7 + dangling)
    target = _protein(rng, 40)
    tseq, toff = S.batch([target.encode()])
    dna = synth.back_translate(target)[:105 + dangling]
    seq, off = _batch([_contig(dna, 31, 0, strand, stop_behind=False)])
    L = int(off[1])
    m = TM.translated_model(seq, off, tseq, toff, ref="query")
    assert len(m["calls"]) == 1
    sq, st, fr, x0, x1, Ls = R.spans(m["calls"], off)
    assert (int(st[0]), int(fr[0]), int(x0[0]), int(x1[0])) == (strand, 1, 34, 34 + 104) and L - 1 - int(x1[0]) == dangling
    assert int(m["hits"][0]["end_target"]) == 34 and int(m["paths"][0]["start_b"]) == 0


# ---- a frameshifted gene: two CALLs of one fI in two frames, one region, repaired ---------------------------------------------------

def _frameshift_case(strand: int):
    rng = np.random.default_rng(11)
    gene = _protein(rng, 80)
    dna = synth.back_translate(gene)
    dna = dna[:120] + dna[121:]                      # codon 40 loses its first base: residues 41 .. 79 are read in the next frame
    contig = _contig(dna, 30, 33, strand)
    return gene, contig


@pytest.mark.parametrize("strand", [0, 1])
def test_a_frameshifted_gene_is_two_calls_one_region_and_one_repaired_protein(strand):
    gene, contig = _frameshift_case(strand)
    tseq, toff = S.batch([gene.encode()])
    seq, off = _batch([contig])
    m = TM.translated_model(seq, off, tseq, toff, ref="query", min_ratio_pct=20)
    frags, pstart, res = m["fragments"]
    calls = m["calls"]
    assert len(calls) == 2 and set(calls["fI"].tolist()) == {0}
    assert sorted((calls["container"] % 3).tolist()) == [0, 2] and set((calls["container"] // 3).tolist()) == {strand}
    for c, r in zip(calls, m["call_hits"]):          # both halves are fragments of at least min_res
        assert int(frags[int(m["hits"][r]["query"])]["n_res"]) >= TM.MIN_RES
    regs, _ = R.regions(calls, off)
    assert len(regs) == 1 and int(regs[0]["frames"]) == 0b101 and int(regs[0]["n_calls"]) == 2 and int(regs[0]["kept"]) == 1
    orfs, ps, rs = O.orfs(regs, seq, off)
    new, nps, nrs, junc, jstart, stats = RP.repair(regs, orfs, ps, rs, calls, seq, off)
    assert stats["repaired"] == 1 and len(junc) == 1 and int(new[0]["flags"]) & N.ORF_REPAIRED
    prot = nrs[nps[0]:nps[1]].tobytes().decode()
    assert gene[1:30] in prot and gene[-30:] in prot
    assert gene[1:30] not in rs[ps[0]:ps[1]].tobytes().decode() or gene[-30:] not in rs[ps[0]:ps[1]].tobytes().decode()


# ---- the drops, the rank cut and target_fn ----------------------------------------------------------------------------------------------

def _two_targets_case():
    rng = np.random.default_rng(5)
    target = _protein(rng, 40)
    seq, off = _batch([_contig(synth.back_translate(target), 30, 33, 0)])
    return target, seq, off


def test_a_below_record_is_no_call():
    rng = np.random.default_rng(21)
    long_target = _protein(rng, 120)
    tseq, toff = S.batch([long_target.encode()])
    seq, off = _batch([_contig(synth.back_translate(long_target[:36]), 30, 33, 0)])
    m = TM.translated_model(seq, off, tseq, toff, min_ratio_pct=90)          # ref longer: 36 of 120 residues is far below 90 %
    assert m["hits"]["status"].tolist() == [N.SEARCH_BELOW] and len(m["calls"]) == 0
    assert m["drops"] == dict(dropped_status=1, dropped_rank=0, dropped_untraced=0)
    assert len(TM.translated_model(seq, off, tseq, toff, min_ratio_pct=90, ref="query")["calls"]) == 1


def test_a_skipped_record_is_no_call():
    target, seq, off = _two_targets_case()
    tseq, toff = S.batch([target.encode()])
    m = TM.translated_model(seq, off, tseq, toff, max_cells=100)              # 40 x 40 cells do not fit
    assert m["hits"]["status"].tolist() == [N.SEARCH_SKIPPED] and len(m["calls"]) == 0 and m["drops"]["dropped_status"] == 1


def test_an_untraced_record_is_no_call():
    target, seq, off = _two_targets_case()
    tseq, toff = S.batch([target.encode()])
    m = TM.translated_model(seq, off, tseq, toff, max_trace_cells=1)
    assert m["hits"]["status"].tolist() == [N.SEARCH_HIT] and m["paths"]["status"].tolist() == [N.PATH_UNTRACED]
    assert len(m["calls"]) == 0 and m["drops"] == dict(dropped_status=0, dropped_rank=0, dropped_untraced=1)


def test_a_record_of_rank_max_hits_or_more_is_no_call_and_target_fn_is_applied():
    target, seq, off = _two_targets_case()
    other = target[:20] + ("W" if target[20] != "W" else "Y") + target[21:]      # a second target, one substitution away
    tseq, toff = S.batch([other.encode(), target.encode()])
    m = TM.translated_model(seq, off, tseq, toff)
    assert m["hits"]["rank"].tolist() == [0, 1] and m["hits"]["target"].tolist() == [1, 0]
    assert m["calls"]["fI"].tolist() == [1] and m["call_hits"].tolist() == [0]
    assert m["drops"] == dict(dropped_status=0, dropped_rank=1, dropped_untraced=0)
    two = TM.translated_model(seq, off, tseq, toff, max_hits=2)
    assert two["calls"]["fI"].tolist() == [1, 0] and two["call_hits"].tolist() == [0, 1] and sum(two["drops"].values()) == 0
    assert (two["calls"]["container"] == two["calls"]["container"][0]).all()
    named = TM.translated_model(seq, off, tseq, toff, max_hits=2, target_fn=[7, 9])
    assert named["calls"]["fI"].tolist() == [9, 7]
    same = TM.translated_model(seq, off, tseq, toff, max_hits=2, target_fn=[4, 4])
    regs, _ = R.regions(same["calls"], off)
    assert same["calls"]["fI"].tolist() == [4, 4] and len(regs) == 1 and int(regs[0]["n_calls"]) == 2


# ---- the ABI, the bindings and the wrappers' argument checks ---------------------------------------------------------------------------

@pytest.mark.parametrize("cname,cls,size", [("kg_translate_params", "KgTranslateParams", 16), ("kg_translate_stats", "KgTranslateStats", 72)])
def test_the_new_structures_sit_where_gcc_puts_them(tmp_path, cname, cls, size):
    struct_ = getattr(N, cls)
    fields = [f for f, _ in struct_._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%%zu\\n", sizeof(%s));\n' % cname +
                   "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(struct_) == size
    assert out[1:] == [getattr(struct_, f).offset for f in fields]


def test_the_new_symbols_are_exported_and_null_arguments_are_refused_before_the_device():
    lib, h = N.load(), C.c_void_p()
    new = [n for n in N.EXPORTS if n.startswith("kg_evidence_")] + ["kg_contigs_search_translated"]
    assert len(new) == 9 and all(hasattr(lib, n) for n in new)
    none = (None, None, None, None, None, 0, None, 0, 0, 0, 0, 0, None, None, None, None)
    assert lib.kg_contigs_search_translated(*none, None) == N.KG_ERR_ARG and lib.kg_last_error().decode() == "null argument"
    assert lib.kg_contigs_search_translated(*none, C.byref(h)) == N.KG_ERR_ARG and lib.kg_last_error().decode() == "null kg_searchdb"
    st = N.KgTranslateStats()
    assert lib.kg_evidence_stats(None, C.byref(st)) == N.KG_ERR_ARG
    assert lib.kg_evidence_calls_copy(None, 0, 0, None) == N.KG_ERR_ARG and lib.kg_evidence_call_hits_copy(None, 0, 0, None) == N.KG_ERR_ARG
    assert lib.kg_evidence_calls_count(None) == 0 and not lib.kg_evidence_calls_device(None)
    assert not lib.kg_evidence_fragments(None) and not lib.kg_evidence_hits(None)
    lib.kg_evidence_free(None)
    assert (N.TRANSLATE_MIN_RES, N.TRANSLATE_MAX_HITS) == (30, 1)


class _LibraryUsed(Exception):
    pass


class _NoLibrary:
    def __getattr__(self, name):
        raise _LibraryUsed(name)


@pytest.mark.parametrize("kw,text", [
    (dict(min_res=0), "min_res must be >= 1"),
    (dict(max_hits=0), "max_hits must be in 1..64"),
    (dict(max_hits=65), "max_hits must be in 1..64"),
    (dict(band=8), "band needs ungapped"),
    (dict(ungapped={"score": 1}), "ungapped must be None, True or {'min_score': N}"),
    (dict(paths="some"), "paths must be None, 'hits' or 'all'"),
    (dict(ops="x"), "ops must be None, 'm' or 'eqx'"),
    (dict(offsets=[]), "offsets must be int64[n_seqs + 1]"),
    (dict(offsets=[0, 9]), "sequence buffer shorter than offsets[-1]"),
])
def test_search_contigs_checks_its_arguments_before_the_library(monkeypatch, kw, text):
    monkeypatch.setattr(N, "load", lambda: _NoLibrary())
    db = H.SearchDb(C.c_void_p(1))
    kw = dict(kw)
    off = kw.pop("offsets", [0, 4])
    with pytest.raises(ValueError) as e:
        db.search_contigs(b"ACGT", off, **kw)
    assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        H.SearchDb(None).search_contigs(b"ACGT", [0, 4])
    assert str(e.value) == "the SearchDb is closed"


def test_the_evidence_shares_scanresult_s_steps_and_checks_like_it(monkeypatch):
    monkeypatch.setattr(N, "load", lambda: _NoLibrary())
    assert H.Evidence.orfs is H.ScanResult.orfs and H.Evidence.select is H.ScanResult.select and H.Evidence.regions is H.ScanResult.regions
    assert H.Evidence._orf_steps is H.ScanResult._orf_steps

    class _Evidence(H.Evidence):
        def __init__(self):
            self._h, self._seqs, self._dev = C.c_void_p(1), 2, 0
            self.calls = np.zeros(0, dtype=N.CALL_DTYPE)

        def close(self):
            pass

    e = _Evidence()
    for call in (lambda: e.regions([0, 4]), lambda: e.orfs(b"ACGT", [0, 4]), lambda: e.select([0, 4])):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == "offsets must be the int64[n_seqs + 1] the scan was given"
    for kw, text in ((dict(free_min_res=50), "free_min_res needs orfs=True: the free candidates are ORFs"),
                     (dict(coding=True), "coding needs orfs=True: the scores are the ORFs'"),
                     (dict(repair=True), "repair needs orfs=True: it rewrites ORFs")):
        with pytest.raises(ValueError) as err:
            e.select([0, 2, 4], **kw)
        assert str(err.value) == text
    e._h = C.c_void_p(None)
    with pytest.raises(ValueError) as err:
        e.regions([0, 2, 4])
    assert str(err.value) == "the Evidence is closed"
