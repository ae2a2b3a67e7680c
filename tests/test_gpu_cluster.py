"""kg_proteins_cluster on the device against tests/cluster_model.py, byte for byte (include/kmerguts_hip.h states the rule)."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import cluster_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_BLOCK = 16 * 256          # kg_cluster.hpp: 16 pairs per lane, 256 lanes per workgroup in the segmented maximum


def _cluster(seq, off, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.cluster_proteins(seq, off, **kw)


def _same(prots_or_packed, min_shared=5, min_cover_pct=20):
    seq, off = M.pack(prots_or_packed) if isinstance(prots_or_packed, list) else prots_or_packed
    got, st = _cluster(seq, off, min_shared=min_shared, min_cover_pct=min_cover_pct)
    want, counts = M.cluster_numpy(seq, off, min_shared, min_cover_pct)
    assert {k: st[k] for k in M.COUNTS} == counts
    assert got.tobytes() == want.tobytes()
    return got, st


@pytest.mark.parametrize("run", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_one_kmer_shared_by_a_run_of_proteins(run):
    lens = 9 + np.arange(run)
    for order in (lens, lens[::-1], np.full(run, 9)):
        got, st = _same(M.one_kmer_batch(order), 1, 0)
        assert st["links"] == st["edges"] == run - 1 and st["families"] == 1 and st["kmers"] == 1
        assert got.tobytes() == M.one_kmer_answer(order).tobytes()
        got, st = _same(M.one_kmer_batch(order))                # the defaults: one shared k-mer is no edge
        assert st["edges"] == 0 and st["families"] == run


def test_a_run_of_100000_with_the_longest_at_every_border():
    run = 100000
    base = 9 + (np.arange(run) * 7919) % 23
    places = sorted({0, run - 1} | {b + d for b in range(CHUNK_BLOCK, run, CHUNK_BLOCK) for d in (-1, 0)})
    assert len(places) == 50
    for k, at in enumerate(places):
        lens = base.copy()
        lens[at] = 40                                           # the one longest protein
        seq, off = M.one_kmer_batch(lens)
        got, st = _cluster(seq, off, min_shared=1, min_cover_pct=0)
        assert got.tobytes() == M.one_kmer_answer(lens).tobytes(), at
        assert (st["pairs"], st["kmers"], st["links"], st["edges"], st["families"], st["largest"]) == (run, 1, run - 1, run - 1, 1, run)
        if k in (0, 1):
            assert M.cluster_numpy(seq, off, 1, 0)[0].tobytes() == got.tobytes()
    # all lengths equal: the tie goes to the smallest index
    seq, off = M.one_kmer_batch(np.full(run, 9))
    got, st = _same((seq, off), 1, 0)
    assert (got["best"][1:] == 0).all() and got["best"][0] == -1 and st["families"] == 1


def test_thresholds():
    rng = np.random.default_rng(7)
    for s, edge in ((4, False), (5, True), (6, True)):          # min_shared - 1, min_shared, min_shared + 1
        got, st = _same(M.shared_pair(rng, s, 12), 5, 0)
        assert st["links"] == 1 and st["edges"] == int(edge) and got["shared"][0] == (s if edge else 0)
    got, st = _same(M.shared_pair(rng, 5, 25), 1, 20)           # 100 * 5 == 20 * 25
    assert st["edges"] == 1 and got[0].tolist() == (0, 0, 1, 5)
    got, st = _same(M.shared_pair(rng, 5, 26), 1, 20)           # 100 * 5 < 20 * 26
    assert st["links"] == 1 and st["edges"] == 0 and st["families"] == 2


def test_a_path_of_4096_under_a_permutation():
    got, st = _same(M.path_batch(np.random.default_rng(11), 4096))
    assert st["families"] == 1 and (got["root"] == 0).all() and st["largest"] == 4096
    print("path of 4096: rounds = %d, links = %d, edges = %d" % (st["rounds"], st["links"], st["edges"]))
    assert 1 <= st["rounds"] <= 4096


def test_a_star_of_10000():
    got, st = _same(M.star_batch(np.random.default_rng(12), 10000))
    assert st["families"] == 1 and st["largest"] == 10001 and (got["best"][1:] == 0).all()


def test_edge_inputs():
    got, st = _same([])
    assert len(got) == 0 and st["families"] == 0
    got, st = _same([b"ACDEFGHIKLMNPQ"])
    assert got[0].tolist() == (0, 0, -1, 0)
    got, st = _same([b"", b"ACDEFGHI", b"ACDEFGH", b"A", b"ACDEFGHI"])     # nine residues give the first window
    assert st["valid_windows"] == 0 and got["family"].tolist() == [0, 1, 2, 3, 4]
    got, st = _same([b"ACDXFGHIKLMXPQRSTVWXAC", b"XXXXXXXXXXXXXXXXXXXXXXXXXXXXXX", b"ACDEFGHJK"], 1, 0)
    assert st["valid_windows"] == 0 and st["families"] == 3


def test_no_link_across_a_concatenation_border():
    rng = np.random.default_rng(13)
    h = M.random_protein(rng, 30)
    prots = [M.random_protein(rng, 25) + h[:15], h[15:] + M.random_protein(rng, 25), M.random_protein(rng, 31) + h[:15],
             h[15:] + M.random_protein(rng, 31)]
    got, st = _same(prots, 1, 0)
    assert M.partition(got) == {frozenset({0, 2}), frozenset({1, 3})}


def test_random_batches():
    for seed in range(24):
        rng = np.random.default_rng(1000 + seed)
        prots = M.random_batch(rng, n_fam=int(rng.integers(1, 40)))
        _same(prots, int(rng.integers(1, 7)), int(rng.choice([0, 10, 20, 50, 100])))


def test_batch_independence():
    rng = np.random.default_rng(14)
    mine = M.random_batch(rng, n_fam=12)
    others = [M.random_protein(rng, int(rng.integers(9, 200))) for _ in range(300)]
    alone, _ = _same(mine)
    for lead in (0, 137):
        inside, _ = _same(others[:lead] + mine + others[lead:])
        part = {frozenset(i - lead for i in g) for g in M.partition(inside) if any(lead <= i < lead + len(mine) for i in g)}
        assert part == M.partition(alone)


def test_the_ecoli_proteome():
    from kmergutsjava_amd.make_signatures import parse_fasta
    ids, seqs = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))
    got, st = _same(seqs)
    print("E. coli K-12 W3110: %d proteins, %d families, %d of two or more, largest %d, %d links, %d edges, %d rounds" %
          (st["proteins"], st["families"], st["families_multi"], st["largest"], st["links"], st["edges"], st["rounds"]))
    assert st["proteins"] == len(ids) > 4000


def test_errors():
    from kmergutsjava_amd import _native as N
    seq, off = M.pack(M.random_batch(np.random.default_rng(15)))
    for kw, word in ((dict(min_shared=0), "min_shared"), (dict(min_cover_pct=101), "min_cover_pct"), (dict(min_cover_pct=-1), "min_cover_pct"),
                     (dict(max_windows=-1), "max_windows")):
        with pytest.raises(N.KmerGutsNativeError) as ei:
            _cluster(seq, off, **kw)
        assert ei.value.code == N.KG_ERR_ARG and word in str(ei.value)
    lib, h = N.load(), C.c_void_p()
    p = N.KgClusterParams(5, 20, 1)
    arr = np.frombuffer(seq, dtype=np.uint8)
    assert lib.kg_proteins_cluster(0, C.byref(p), arr.ctypes.data, off.ctypes.data, off.size - 1, 0, C.byref(h)) == N.KG_ERR_ARG
    assert b"reserved" in lib.kg_last_error() and not h.value
    bad = off.copy()
    bad[4] = bad[3] - 1
    with pytest.raises(N.KmerGutsNativeError) as ei:
        _cluster(seq, bad)
    assert ei.value.code == N.KG_ERR_ARG and "protein 3" in str(ei.value)
    _, st = _cluster(seq, off)
    with pytest.raises(N.KmerGutsNativeError) as ei:
        _cluster(seq, off, max_windows=st["valid_windows"] - 1)
    assert ei.value.code == N.KG_ERR_LIMIT and "%d valid windows do not fit" % st["valid_windows"] in str(ei.value)
    got, _ = _cluster(seq, off, max_windows=st["valid_windows"])
    assert got.tobytes() == M.cluster_numpy(seq, off)[0].tobytes()


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    import torch
    from kmergutsjava_amd import _native as N, hotpath, synth
    seq, off = M.pack(M.random_batch(np.random.default_rng(16), n_fam=30))
    want = M.cluster_numpy(seq, off)[0]
    rec = synth.high_density_config(4, 100, 4001, 500, dna=False)[2]
    with hotpath.SignatureTable.from_bytes(synth.table_image(rec), 0) as tab:
        assert _cluster(seq, off)[0].tobytes() == want.tobytes()
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        failed = 0
        for n in range(1, 400):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got, _ = _cluster(seq, off)
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
                assert tab.live_device_bytes() == live0
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= 20 and got.tobytes() == want.tobytes()
        assert _cluster(seq, off)[0].tobytes() == want.tobytes()
        assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0


# ---- end to end: unknown genes of two genomes become signatures that find them in a third ----------------------------------------

def _rc(dna: bytes) -> bytes:
    return dna.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def _planted(rng, genes, copy, length=20000):
    """A random contig with copy `copy` of every gene (a substitution at every 12th residue, the same positions in every copy)
    as TAA ATG codons TAA, on alternating strands.  -> (contig, [(left, right, strand)] 0-based of ATG .. TAA)"""
    from kmergutsjava_amd import synth
    parts, at, where = [], 0, []
    gap = (length - len(genes) * (3 * 302 + 3)) // (len(genes) + 1)
    for g, base in enumerate(genes):
        prot = bytearray(base)
        for i in range(5, len(prot), 12):
            prot[i] = M.ALPHA[(M.ALPHA.index(prot[i]) + 1 + copy) % 20]
        sp = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=gap))
        orf = b"ATG" + synth.back_translate(prot.decode()).encode() + b"TAA"
        dna = b"TAA" + orf if g % 2 == 0 else _rc(b"TAA" + orf)
        parts += [sp, dna]
        left = at + gap + (3 if g % 2 == 0 else 0)
        where.append((left, left + len(orf) - 1, g % 2))
        at += gap + len(dna)
    parts.append(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=length - at)))
    return b"".join(parts), where


def test_end_to_end_unknown_genes_become_signatures(tmp_path):
    from kmergutsjava_amd import call_regions as CR, cluster_proteins as CP, make_signatures as MS, synth
    rng = np.random.default_rng(17)
    genes = [M.random_protein(rng, 300) for _ in range(3)]
    contigs = [_planted(rng, genes, k) for k in range(3)]
    d = tmp_path / "d"
    synth.write_data_dir(str(d), synth.table_image(synth.high_density_config(4, 100, 4001, 500, dna=True)[2]), 1000)
    (tmp_path / "two.fna").write_bytes(b"".join(b">genome%d\n%s\n" % (k, contigs[k][0]) for k in range(2)))
    (tmp_path / "third.fna").write_bytes(b">genome2\n%s\n" % contigs[2][0])
    faa, fam, ann = tmp_path / "two.faa", tmp_path / "families.tsv", tmp_path / "ann.tsv"
    assert CR.main(["-D", str(d), "-q", str(tmp_path / "two.fna"), "-o", str(tmp_path / "two.tsv"), "--faa", str(faa), "--free-orfs"]) == 0
    assert CP.main(["-p", str(faa), "-o", str(fam), "-A", str(ann)]) == 0
    ids = [[b"genome%d_%d_%d_%s" % (k, left + 1, right + 1, b"-" if strand else b"+") for left, right, strand in contigs[k][1]] for k in range(2)]
    rows = [r.split(b"\t") for r in fam.read_bytes().splitlines()]
    families = {}
    for r in rows:
        families.setdefault(r[1], set()).add(r[0])
    # the three planted families, each with its two members (ORFs on the genes' other strands and frames, which the copies
    # share as well, make further families: the clustering does not know which frame codes)
    mine = {name: who for name, who in families.items() if who & set(ids[0] + ids[1])}
    assert sorted(map(sorted, mine.values())) == sorted(sorted([ids[0][g], ids[1][g]]) for g in range(3))
    assert all(len(who) >= 2 for who in families.values())
    assert sorted(ann.read_bytes().splitlines()) == sorted(b"%s\thypothetical protein %s" % (r[0], r[1]) for r in rows)
    out = tmp_path / "KmerData"
    r = MS.make_signatures(str(faa), str(ann), str(tmp_path / "sigs.txt"), str(out))
    assert r["signatures"] > 3 * 50
    p = subprocess.run([os.path.join(ROOT, "kmergutsjava_amd", "kmer_guts"), "-D", str(out), "-q", str(tmp_path / "third.fna"), "-o",
                        str(tmp_path / "report.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    called = {line.split(b"\t")[5] for line in (tmp_path / "report.txt").read_bytes().splitlines() if line.startswith(b"CALL\t")}
    assert called >= {b"hypothetical protein " + name for name in mine}
