"""The start-codon rule (kg_orfset_starts, include/kmerguts_hip.h) on the CPU: the plain-loop form of tests/starts_model.py
against its numpy form, hand-made known answers, kg_start_weights_from (host code of the library: no GPU) against the model, the
struct layouts, the model file, and the call_regions front end with the device calls replaced by the models.  Also the input
builders tests/test_gpu_starts.py shares."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import coding_model as K  # noqa: E402
import select_model as S  # noqa: E402
import starts_model as M  # noqa: E402
import test_coding_host as TH  # noqa: E402
import test_java_binding as H  # noqa: E402
import test_orfs_host as HO  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

ROOT = os.path.dirname(HERE)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
FILL = (b"GCA", b"CCG", b"AAA", b"GAC", b"CTC", b"TCT", b"ACC")     # neither start nor stop
_SENSE = [bytes(c) for c in (np.array([[a, b, c] for a in b"ACGT" for b in b"ACGT" for c in b"ACGT"], dtype=np.uint8))
          if bytes(c) not in (b"TAA", b"TAG", b"TGA", b"ATG", b"GTG", b"TTG")]


# ---- input builders -------------------------------------------------------------------------------------------------------------------

_COMP = bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa")


def _rc(dna: bytes) -> bytes:
    """The reverse complement; lower case stays lower case, U is read as T, everything else stays what it is."""
    return dna.translate(_COMP)[::-1]


def gene(rng, n_res, starts, strand=0, frame=0, up=30, down=7, flags=1, kept=1, random_codons=False, unknowns=0.0, start_codon=None):
    """One contig with one ORF: `frame` random bases, `up` (a count of random bases, or the bases), n_res codons -- those of
    `starts` {k: spelling}, the others no start and no stop --, TAA, `down` random bases.  On '-' the contig is the reverse
    complement.  -> (contig bytes, the record as a tuple of seq 0)."""
    lead = bytes(rng.choice(ACGT, size=frame))
    upb = bytes(rng.choice(ACGT, size=up)) if isinstance(up, int) else up
    codons = []
    for k in range(n_res):
        if k in starts:
            codons.append(starts[k])
        elif random_codons:
            c = bytearray(_SENSE[int(rng.integers(0, len(_SENSE)))])
            if unknowns and rng.random() < unknowns:
                c[int(rng.integers(0, 3))] = ord("N")
            codons.append(bytes(c))
        else:
            codons.append(FILL[k % len(FILL)])
    text = lead + upb + b"".join(codons) + b"TAA" + bytes(rng.choice(ACGT, size=down))
    xs, L = len(lead) + len(upb), len(text)
    xe = xs + 3 * (n_res + 1) - 1
    left, right = (xs, xe) if not strand else (L - 1 - xe, L - 1 - xs)
    first = starts.get(0, b"")
    sc = start_codon if start_codon is not None else {b"ATG": 1, b"GTG": 2, b"TTG": 3}.get(first.upper().replace(b"U", b"T"), 1)
    rec = K.orf(0, strand, left, right, n_res, flags=flags, kept=kept, frame=xs % 3, start_codon=sc,
                fI=-1 if flags & 16 else 3, score=0 if flags & 16 else 9)
    return (text if not strand else _rc(text)), rec


def batch(genes):
    """gene() results -> (records, bytes, offsets), one contig per gene."""
    rows = [(k,) + tuple(rec[1:]) for k, (_, rec) in enumerate(genes)]
    seq, off = batch_of([g[0] for g in genes])
    return K.records(rows), seq, off


def batch_of(contigs):
    off = np.zeros(len(contigs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in contigs])
    return np.frombuffer(b"".join(bytes(c) for c in contigs), dtype=np.uint8), off


def sd_genes(rng, n):
    """n genes whose true start, a few codons behind a decoy start at codon 0, has AGGAGG some bases in front of it: something
    for the rounds to learn.  A third are free, a few partial5."""
    out = []
    for g in range(n):
        true = int(rng.integers(3, 12))
        n_res = int(rng.integers(30, 70))
        starts = {0: (b"ATG", b"GTG", b"TTG")[int(rng.integers(0, 3))], true: b"ATG" if rng.random() < 0.8 else b"GTG"}
        if rng.random() < 0.5:
            starts[int(rng.integers(true + 1, n_res - 12))] = b"TTG"
        contig, rec = gene(rng, n_res, starts, strand=g % 2, frame=g % 3, random_codons=True,
                           flags=(17 if g % 3 == 0 else 3 if g % 11 == 0 else 1))
        # AGGAGG 6 to 9 bases in front of the true start, written over the codons there (on the strand)
        text = bytearray(contig if not g % 2 else _rc(contig))
        xs = (g % 3) + 30
        at = xs + 3 * true - int(rng.integers(12, 16))
        if at >= xs + 3:
            cod = (at - xs) // 3
            text[xs + 3 * cod:xs + 3 * cod + 9] = b"GAGGAGGCA"[:9]
        out.append((bytes(text) if not g % 2 else _rc(bytes(text)), rec))
    return batch(out)


def conflict_case():
    """One contig, two evidence regions on '+'.  A (score 50) is a gene of 200 codons.  B (score 5), in the next frame, begins
    with an ATG 150 nt inside A's end and has a GTG 60 codons further down, behind A's end; its region lies behind the GTG, so
    its ORF reaches back to the ATG and loses to A.  With weights that pay for GTG, B moves out of the conflict.
    -> (regions, bytes, offsets, weights)."""
    import orfs_model as O
    a = b"ATG" + b"".join(FILL[k % 7] for k in range(199)) + b"TAA"                # 603 nt at 2 .. 604
    b = b"ATG" + b"".join(FILL[(k + 2) % 7] for k in range(59)) + b"GTG" + b"".join(FILL[k % 7] for k in range(80)) + b"TAA"
    text = bytearray(b"CC" + a + b"C" * 400)
    at = 2 + len(a) - 150 + 1                           # 456: B's frame is A's + 1 (mod 3)
    text[at:at + len(b)] = b
    text[2 + len(a) - 3:2 + len(a)] = b"TAA"            # A's stop again: ??T AA? in B's frame, neither stop nor start
    seq, off = batch_of([bytes(text)])
    L = len(text)
    regs = O.regions_of([O.codon_region(L, 0, 2, 10, 190, score=50), O.codon_region(L, 0, at % 3, at // 3 + 63, at // 3 + 130, score=5)])
    W = (np.zeros((20, 4), np.int32), np.array([0, 0, 10 ** 6, 0], np.int32))
    return regs, seq, off, W


def same_as_recorded(key: str, files) -> None:
    """tests/golden/call_regions_planted_before_starts.json: sha256, bytes and lines of the three files the front end wrote with
    --coding for the planted contigs before it knew --starts (recorded from that commit's writers), for run `key`."""
    want = json.load(open(os.path.join(HERE, "golden", "call_regions_planted_before_starts.json")))["runs"][key]
    for name, data in zip(("tsv", "orfs", "faa"), files):
        got = {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data), "lines": data.count(b"\n")}
        assert got == want[name], (key, name, got, want[name])


def annotated_lengths(prots, free, before, after):
    """-> (ORFs of `before` with a known protein's length, ORFs of `after` with one, ORFs that end in a known protein's last 30
    residues): free = (records, prot_start, residues) of the ORFs as they were."""
    tails = {}
    for p in prots:
        if len(p) >= 30:
            tails.setdefault(bytes(p[-30:]), set()).add(len(p))
    rb, ps = free[2].tobytes(), free[1]
    known = [tails.get(rb[ps[i + 1] - 30:ps[i + 1]]) for i in range(len(before))]
    count = lambda recs: sum(1 for i, kn in enumerate(known) if kn and int(recs["n_res"][i]) in kn)     # noqa: E731
    return count(before), count(after), sum(1 for kn in known if kn)


# ---- the two forms of the model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(5))
def test_plain_loops_match_numpy(seed):
    """50 random small batches per seed: contigs of length 0 to 30 among longer ones, N, -, u and lower case, both strands, all
    frames, limits, masks, rounds, own training and caller's weights."""
    rng = np.random.default_rng(300 + seed)
    cands = moved = trained = 0
    for it in range(50):
        if it % 10 == 0:
            lens = rng.permutation(list(range(0, 31, 3)) + [150, 200, 181])
            orfs, seq, off = K.random_batch(rng, 0, lens=lens)
            orfs["start_codon"] = rng.integers(0, 4, size=len(orfs))
        elif it % 3 == 0:
            orfs, seq, off = sd_genes(rng, int(rng.integers(1, 12)))
            for _ in range(int(rng.integers(0, 4))):        # unknown bases and other spellings anywhere
                seq = seq.copy()
                seq[int(rng.integers(0, len(seq)))] = rng.choice(np.frombuffer(b"N-uUacgt", np.uint8))
        else:
            orfs, seq, off = M.random_batch(rng, int(rng.integers(0, 7)), max_len=150)
        T = rng.integers(-3000, 3000, size=K.BINS).astype(np.int32)
        kw = dict(min_res=int(rng.integers(1, 12)), start_codons=int(rng.choice([7, 7, 7, 1, 2, 4, 5, 0])), rounds=int(rng.integers(1, 5)),
                  min_train_starts=int(rng.integers(0, 4)))
        lim = rng.integers(-1, 9, size=len(orfs)).astype(np.int32) if rng.random() < 0.4 else None
        W = (rng.integers(-500, 500, size=(20, 4)).astype(np.int32), rng.integers(-500, 500, size=4).astype(np.int32)) if rng.random() < 0.3 else None
        a = M.starts(orfs, seq, off, T, W, lim, loops=True, **kw)
        b = M.starts(orfs, seq, off, T, W, lim, **kw)
        assert a["orfs"].tobytes() == b["orfs"].tobytes() and a["shifts"].tobytes() == b["shifts"].tobytes() and a["stats"] == b["stats"]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a["model"], b["model"]))
        cands, moved, trained = cands + a["stats"]["candidates"], moved + a["stats"]["moved"], trained + (a["stats"]["trained"] == 1)
        # what never changes
        same = a["shifts"] == 0
        assert a["orfs"][same].tobytes() == orfs[same].tobytes()
        for f in ("seq", "strand", "frame", "first_inner", "fI", "score", "kept"):
            assert (a["orfs"][f] == orfs[f]).all()
        assert ((a["orfs"]["right"] - a["orfs"]["left"]) == (orfs["right"] - orfs["left"]) - 3 * a["shifts"]).all()
    print(cands, moved, trained)
    assert cands > 150 and moved > 5 and trained > 5


def _one(contig, strand, xs, n_res, **kw):
    L = len(contig)
    xe = xs + 3 * (n_res + 1) - 1
    left, right = (xs, xe) if not strand else (L - 1 - xe, L - 1 - xs)
    return K.records([K.orf(0, strand, left, right, n_res, start_codon=1, frame=xs % 3, **kw)])


def test_known_answers_of_one_contig():
    """GG ATG AAA GTG CCC TTG ACC TAA G on '+', and its reverse complement on '-'."""
    text = b"GGATGAAAGTGCCCTTGACCTAAG"
    off = np.array([0, len(text)], np.int64)
    idx = lambda s: sum("ACGT".index(ch) << (2 * (5 - i)) for i, ch in enumerate(s))    # noqa: E731
    T = np.zeros(K.BINS, np.int32)
    T[idx("ATGAAA")], T[idx("AAAGTG")], T[idx("GTGCCC")], T[idx("CCCTTG")], T[idx("TTGACC")] = 1, 10, 100, 1000, 10000
    for strand, contig in ((0, text), (1, HO._rc(text))):
        o = _one(contig, strand, 2, 6)
        for fn in (M.candidates_loops, lambda *a: [(int(k), int(s), list(w), int(t)) for k, s, w, t in zip(*M.candidates_np(*a))]):
            c = fn(o[0], np.frombuffer(contig, np.uint8), off, T, 5, 7)
            assert [(k, s, t) for k, s, w, t in c] == [(0, 11111, 1), (2, 11100, 2), (4, 10000, 3)]
            # the window: 20 positions in front of the codon; those in front of the contig are 4
            code = lambda s: ["ACGT".index(ch) for ch in s]     # noqa: E731
            assert c[0][2] == [4] * 18 + code("GG") and c[1][2] == [4] * 12 + code("GGATGAAA") and c[2][2] == [4] * 6 + code("GGATGAAAGTGCCC")
        zero = (np.zeros((20, 4), np.int32), np.zeros(4, np.int32))
        # the largest score; K exactly at a candidate and one below it; the masks
        assert M.starts(o, contig, off, T, zero, min_res=1)["shifts"].tolist() == [0]
        assert M.starts(o, contig, off, -T, zero, min_res=1)["shifts"].tolist() == [4]
        assert M.starts(o, contig, off, -T, zero, min_res=2)["shifts"].tolist() == [4]         # K = 4
        assert M.starts(o, contig, off, -T, zero, min_res=3)["shifts"].tolist() == [2]         # K = 3
        assert M.starts(o, contig, off, -T, zero, np.array([1], np.int32), min_res=1)["shifts"].tolist() == [0]
        assert M.starts(o, contig, off, -T, zero, min_res=1, start_codons=3)["shifts"].tolist() == [2]
        got = M.starts(o, contig, off, -T, zero, min_res=1)
        r = got["orfs"][0]
        assert (r["n_res"], r["start_codon"], r["flags"]) == (2, 3, 1 | M.MOVED)
        assert (r["left"], r["right"]) == ((14, 22) if not strand else (len(text) - 1 - 22, len(text) - 1 - 14))
        # a tie takes the smaller k
        assert M.starts(o, contig, off, np.zeros(K.BINS, np.int32), zero, min_res=1)["shifts"].tolist() == [0]
        tie = (np.zeros((20, 4), np.int32), np.array([0, -5, 0, 0], np.int32))         # GTG and TTG tie above ATG
        assert M.starts(o, contig, off, np.zeros(K.BINS, np.int32), tie, min_res=1)["shifts"].tolist() == [2]
        # a weight on the window: G at position 19 (the base in front of the codon) is in front of codons 0 (G) and ... only
        wpos = np.zeros((20, 4), np.int32)
        wpos[19, 1] = 7                                     # C in front of TTG (CCC TTG)
        assert M.starts(o, contig, off, np.zeros(K.BINS, np.int32), (wpos, np.zeros(4, np.int32)), min_res=1)["shifts"].tolist() == [4]
        # an unknown base in the window adds 0; in a pair it takes the pair away; in a candidate codon the candidate
        unk = contig.replace(b"CCC", b"CCN") if not strand else contig.replace(b"GGG", b"NGG")
        assert M.starts(o, unk, off, np.zeros(K.BINS, np.int32), (wpos, np.zeros(4, np.int32)), min_res=1)["shifts"].tolist() == [0]
        c = M.candidates_loops(o[0], np.frombuffer(unk, np.uint8), off, T, 5, 7)
        assert [(k, s) for k, s, w, t in c] == [(0, 10011), (2, 10000), (4, 10000)] and c[2][2][-1] == 4
        nog = contig.replace(b"AAAGTG", b"AAAGNG") if not strand else contig.replace(b"CACTTT", b"CNCTTT")
        assert [k for k, s, w, t in M.candidates_loops(o[0], np.frombuffer(nog, np.uint8), off, T, 5, 7)] == [0, 4]
    # a window off the contig's end on '-': the record on the reverse strand's first codon
    contig = HO._rc(b"ATGAAAGTGCCCTAAGG")
    o = _one(contig, 1, 0, 4)
    c = M.candidates_loops(o[0], np.frombuffer(contig, np.uint8), np.array([0, len(contig)], np.int64), T, 3, 7)
    assert c[0][2] == [4] * 20 and c[1][2] == [4] * 14 + [0, 3, 2, 0, 0, 0]
    # among neighbours the window does not read the neighbour's bytes
    two = np.array([0, 9, 9 + len(contig)], np.int64)
    o2 = o.copy()
    o2["seq"] = 1
    assert M.candidates_loops(o2[0], np.frombuffer(b"ACGTACGTA" + contig, np.uint8), two, T, 3, 7)[0][2] == [4] * 20


def test_the_counts_and_the_rounds_by_hand():
    """Two training records and a free one: cand counts every candidate of the training records, chosen the current one."""
    rng = np.random.default_rng(2)
    genes = [gene(rng, 12, {0: b"ATG", 5: b"GTG"}, up=b"A" * 30), gene(rng, 12, {0: b"TTG", 3: b"ATG"}, strand=1, up=b"C" * 30),
             gene(rng, 12, {0: b"ATG", 4: b"ATG"}, flags=17, up=b"G" * 30), gene(rng, 12, {0: b"ATG", 4: b"ATG"}, flags=3, up=b"G" * 30)]
    orfs, seq, off = batch(genes)
    got = M.starts(orfs, seq, off, np.zeros(K.BINS, np.int32), min_res=1, rounds=1, min_train_starts=2)
    chosen, cand, tch, tca = got["model"]
    assert got["stats"] == {"movable": 4, "training_records": 2, "candidates": 8, "moved": got["stats"]["moved"], "rounds_run": 1, "trained": 1}
    assert tch.tolist() == [0, 1, 0, 1] and tca.tolist() == [0, 2, 1, 1] and chosen.sum() == 2 * 20 and cand.sum() == 4 * 20
    assert chosen[19].tolist() == [1, 1, 0, 0] and chosen[0].tolist() == [1, 1, 0, 0]
    W = M.weights_from(chosen, cand, tch, tca)
    assert W[1][0] == 0 and W[1][1] == K.lg(2) - K.lg(5) - K.lg(3) + K.lg(7) and W[0][0][0] == K.lg(2) - K.lg(6) - K.lg(3) + K.lg(8)
    assert M.starts(orfs, seq, off, np.zeros(K.BINS, np.int32), min_res=1, min_train_starts=3)["stats"]["trained"] == 0


# ---- kg_start_weights_from ------------------------------------------------------------------------------------------------------------

def _lib_weights(model):
    lib = N.load()
    m = N.KgStartModel()
    for name, a in zip(("chosen", "cand", "type_chosen", "type_cand"), model):
        a = np.ascontiguousarray(a, dtype=np.int64)
        C.memmove(getattr(m, name), a.ctypes.data, a.nbytes)
    w = N.KgStartWeights()
    rc = lib.kg_start_weights_from(C.byref(m), C.byref(w))
    return rc, np.array(w.pos, dtype=np.int32).reshape(20, 4), np.array(w.type, dtype=np.int32)


def test_kg_start_weights_from_matches_the_model(native):
    from kmergutsjava_amd import hotpath
    rc, pos, typ = _lib_weights(M.zero_model())
    assert rc == 0 and not pos.any() and not typ.any()
    one = M.zero_model()
    one[0][7][2] = 1 << 40
    rc, pos, typ = _lib_weights(one)
    wm = M.weights_from(*one)
    assert rc == 0 and pos.tobytes() == wm[0].tobytes() and typ.tobytes() == wm[1].tobytes()
    # Lg(2^40 + 1) = Lg(2^40 + 4) = 10240, Lg(4) = 512: 512 in the bin, -10240 + 512 beside it, 0 in every other row
    assert pos[7].tolist() == [-9728, -9728, 512, -9728] and not np.delete(pos, 7, axis=0).any()
    rng = np.random.default_rng(3)
    for hi in (2, 1000, 1 << 30, 1 << 59):
        m = (rng.integers(0, hi, size=(20, 4)), rng.integers(0, hi, size=(20, 4)), rng.integers(0, hi, size=4), rng.integers(0, hi, size=4))
        rc, pos, typ = _lib_weights(m)
        wm = M.weights_from(*m)
        assert rc == 0 and pos.tobytes() == wm[0].tobytes() and typ.tobytes() == wm[1].tobytes() and typ[0] == 0
        hp = hotpath.start_weights(*m)
        assert hp[0].tobytes() == pos.tobytes() and hp[1].tobytes() == typ.tobytes()


def test_kg_start_weights_from_errors(native):
    lib = N.load()
    neg = M.zero_model()
    neg[1][3][1] = -1
    assert _lib_weights(neg)[0] == N.KG_ERR_ARG and b"candidate count of position 3" in lib.kg_last_error()
    neg = M.zero_model()
    neg[2][2] = -1
    assert _lib_weights(neg)[0] == N.KG_ERR_ARG and b"chosen count of the types" in lib.kg_last_error()
    big = M.zero_model()
    big[0][5][0] = big[0][5][1] = 1 << 61
    assert _lib_weights(big)[0] == N.KG_ERR_ARG and b"2^62" in lib.kg_last_error()
    with pytest.raises(ValueError):
        M.weights_from(*big)
    ignored = M.zero_model()
    ignored[2][0] = -5                                   # index 0 of the type arrays takes no part
    assert _lib_weights(ignored)[0] == 0
    m, w = N.KgStartModel(), N.KgStartWeights()
    assert lib.kg_start_weights_from(None, C.byref(w)) == N.KG_ERR_ARG and lib.kg_start_weights_from(C.byref(m), None) == N.KG_ERR_ARG
    from kmergutsjava_amd import hotpath
    with pytest.raises(ValueError):
        hotpath.start_weights(np.zeros((20, 3)), np.zeros((20, 4)), np.zeros(4), np.zeros(4))


# ---- layouts --------------------------------------------------------------------------------------------------------------------------

def test_structs_match_the_c_layout_and_the_jna_source(tmp_path):
    width = {"int32_t": "int", "uint32_t": "int", "int64_t": "long", "float": "float"}
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    lines = []
    for cname, jname, py in (("kg_start_params", "KgStartParams", N.KgStartParams), ("kg_start_stats", "KgStartStats", N.KgStartStats)):
        cf = H._c_struct(cname)
        jf, order = H._java_struct(jname)
        assert [n for n, _ in jf] == [n for n, _ in cf] == order == [n for n, _ in py._fields_], cname
        assert [t for _, t in jf] == [width[t] for _, t in cf] and [t for _, t in py._fields_] == [ctype[t] for _, t in cf], cname
        lines.append('printf("%%zu\\n", sizeof(%s));\n' % cname)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f, _ in cf]
    arrays = (("kg_start_model", N.KgStartModel, ("chosen", "cand", "type_chosen", "type_cand")), ("kg_start_weights", N.KgStartWeights, ("pos", "type")))
    for cname, py, fields in arrays:
        lines.append('printf("%%zu\\n", sizeof(%s));\n' % cname)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in fields]
    lines.append('printf("%u\\n", KG_ORF_START_MOVED);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for py in (N.KgStartParams, N.KgStartStats):
        want += [C.sizeof(py)] + [getattr(py, f).offset for f, _ in py._fields_]
    for _, py, fields in arrays:
        want += [C.sizeof(py)] + [getattr(py, f).offset for f in fields]
    want.append(N.ORF_START_MOVED)
    assert out == want and C.sizeof(N.KgStartParams) == 24 and C.sizeof(N.KgStartStats) == 48
    assert C.sizeof(N.KgStartModel) == 8 * 168 and C.sizeof(N.KgStartWeights) == 4 * 84 and N.ORF_START_MOVED == M.MOVED == 64
    j = H._strip_comments(H.JAVA)
    for decl in ("public long[] chosen = new long[80]", "public long[] cand = new long[80]", "public long[] type_chosen = new long[4]",
                 "public long[] type_cand = new long[4]", "public int[] pos = new int[80]", "public int[] type = new int[4]"):
        assert decl in j, decl
    assert {"kg_orfset_starts", "kg_orfset_start_shifts", "kg_orfset_start_stats", "kg_orfset_start_model", "kg_start_weights_from",
            "kg_starts_orfs"} <= set(N.EXPORTS)


def test_constants_match_the_kernels():
    src = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_starts.hpp")).read()
    assert "constexpr int kStartThreads = 256;" in src and "constexpr int kStartSteps = 4;" in src and N.START_CHUNK == 256 * 4
    assert "constexpr int kStartWin = %d;" % N.START_WINDOW in src and M.WIN == N.START_WINDOW


def test_the_kernels_use_no_scratch_and_do_not_spill():
    """From the compiler's own report (tools/kernel_resources.py), as tests/test_kernel_resources.py reads it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not found")
    res = kr.resources()
    for k in ("starts_lens_kernel", "starts_pairs_kernel", "starts_top_kernel", "starts_cands_kernel", "starts_window_kernel", "starts_count_kernel",
              "starts_choose_kernel<false>", "starts_choose_kernel<true>", "starts_chosen_kernel", "starts_apply_kernel"):
        assert k in res, (k, sorted(res))
        assert res[k]["sgpr_spills"] == 0 and res[k]["vgpr_spills"] == 0 and res[k]["scratch"] == 0, (k, res[k])


# ---- the model file -------------------------------------------------------------------------------------------------------------------

def test_model_file_round_trip():
    from kmergutsjava_amd import call_regions as CR
    from kmergutsjava_amd.make_signatures import InputError
    rng = np.random.default_rng(1)
    m = (rng.integers(0, 1 << 50, size=(20, 4)), rng.integers(0, 1 << 50, size=(20, 4)), rng.integers(0, 1 << 20, size=4), rng.integers(0, 1 << 20, size=4))
    text = CR.format_start_model(*m)
    lines = text.split(b"\n")
    assert lines[0] == b"#kmerguts start model 1" and len(lines) == 85 and lines[-1] == b""
    assert lines[1] == b"0\tA\t%d\t%d" % (m[0][0][0], m[1][0][0]) and lines[80] == b"19\tT\t%d\t%d" % (m[0][19][3], m[1][19][3])
    assert lines[81] == b"type\tATG\t%d\t%d" % (m[2][1], m[3][1]) and lines[83].startswith(b"type\tTTG\t")
    back = CR.parse_start_model(text)
    assert back[0].tobytes() == m[0].astype(np.int64).tobytes() and back[1].tobytes() == m[1].astype(np.int64).tobytes()
    assert back[2].tolist() == [0] + m[2][1:].tolist() and back[3].tolist() == [0] + m[3][1:].tolist()
    assert CR.parse_start_model(text.replace(b"\n", b"\r\n"))[0].tobytes() == back[0].tobytes()
    for bad, word in ((b"#kmerguts start model 2\n" + text.partition(b"\n")[2], "first line"), (text[:-12], "line 84"),
                      (text + b"type\tATG\t1\t1\n", "84 lines"), (text.replace(b"\n0\tC\t", b"\n0\tG\t", 1), "line 3"),
                      (text.replace(b"\n0\tG\t", b"\n0\tG\tx", 1), "line 4"), (text.replace(b"type\tGTG", b"type\tCTG"), "line 83"), (b"", "first line")):
        with pytest.raises(InputError) as ei:
            CR.parse_start_model(bad, "m.txt")
        assert word in str(ei.value) and "m.txt" in str(ei.value), (word, str(ei.value))


# ---- the front end, the device calls replaced by the models -------------------------------------------------------------------------------

class _ModelScan(TH._ModelScan):
    """test_coding_host's stand-in for a ScanResult with starts= added, as hotpath has it."""

    def orfs(self, seq, offsets, merge_gap=600, min_score=0, min_len=0, start_codons=7, only_kept=True, device_ptr=None,
             free_min_res=None, coding=None, min_coding=0, min_train_pairs=100000, starts=None, start_min_res=100, start_rounds=4,
             min_train_starts=200):
        got = TH._ModelScan.orfs(self, seq, offsets, merge_gap, min_score, min_len, start_codons, only_kept, device_ptr, free_min_res, coding,
                                 min_coding, min_train_pairs)
        if starts is not None and starts is not False:
            assert coding is not None
            regs, recs, ps, res = got[0], got[2], got[3], got[4]
            trained = self.coding_stats["trained"] != 0
            T = (K.table(*self.coding_model) if trained else np.zeros(K.BINS, np.int32)) if coding is True else coding
            mts = (1 << 62) if (coding is True and not trained and starts is True) else min_train_starts
            out = M.starts(recs, self.seq, self.off, T, None if starts is True else starts, M.region_limits(recs, regs, self.off), start_min_res,
                           start_codons, start_rounds, mts, prot_start=ps, residues=res, scores=self.coding_scores)
            self.start_shifts, self.start_stats, self.start_model = out["shifts"], out["stats"], out["model"]
            self.coding_scores = out["scores"]
            got = got[:2] + (out["orfs"], out["prot_start"], out["residues"])
        return got

    def select(self, offsets, seq=None, merge_gap=600, min_score=0, min_len=0, orfs=False, start_codons=7, only_kept=True,
               device_ptr=None, max_overlap=60, max_overlap_pct=50, free_min_res=None, coding=None, min_coding=0, min_train_pairs=100000,
               starts=None, start_min_res=100, start_rounds=4, min_train_starts=200):
        assert orfs
        got = self.orfs(seq, offsets, merge_gap, min_score, min_len, start_codons, only_kept, None, free_min_res, coding, min_coding,
                        min_train_pairs, starts, start_min_res, start_rounds, min_train_starts)
        return got + (S.select_fast(S.of_records(got[2]), max_overlap, max_overlap_pct),)


def _front_end(oracle, tmp_path, monkeypatch):
    ids, fnames, dna, off, d, q, made = TH._front_end(oracle, tmp_path, monkeypatch)
    from kmergutsjava_amd import kmer_guts_java as KGJ
    img = TH._WORK["w"][0]

    class _Table:
        def scan(self, batch, boff, params):
            ora = oracle.run(img, np.frombuffer(batch, dtype=np.uint8), boff, lookup_mode=1, min_hits=params.min_hits)
            made.append(_ModelScan(ora["calls"], batch, np.asarray(boff, dtype=np.int64)))
            return made[-1]

    monkeypatch.setattr(KGJ, "_resident_table", lambda path, device: _Table())
    return ids, fnames, dna, off, d, q, made


def test_call_regions_with_starts_against_the_models(oracle, tmp_path, monkeypatch, capsys):
    from kmergutsjava_amd import call_regions as CR
    ids, fnames, dna, off, d, q, made = _front_end(oracle, tmp_path, monkeypatch)
    kw = dict(min_hits=4, merge_gap=300, min_score=12, min_len=100, free_min_res=100, coding=True, min_train=1000)

    def run(tag, **more):
        line = CR.call_regions(d, q, str(tmp_path / (tag + ".tsv")), orfs_out=str(tmp_path / (tag + ".orfs")),
                               faa_out=str(tmp_path / (tag + ".faa")), **kw, **more)
        return line, [(tmp_path / (tag + ext)).read_bytes() for ext in (".tsv", ".orfs", ".faa")]

    model = str(tmp_path / "start_model.txt")
    line, files = run("sel", select=True, starts=True, min_train_starts=50, save_start_model=model)
    skw = dict(free_min_res=100, coding=True, min_train_pairs=1000, starts=True, min_train_starts=50)
    regs, start, orfs, ps, res, sel = made[-1].select(off, dna, 300, 12, 100, True, 7, True, **skw)
    nr, scores, shifts, st = len(regs), made[-1].coding_scores, made[-1].start_shifts, made[-1].start_stats
    plain = made[-1].select(off, dna, 300, 12, 100, True, 7, True, free_min_res=100, coding=True, min_train_pairs=1000)
    moved = shifts > 0
    assert st["trained"] == 1 and st["training_records"] >= 50 and 0 < moved.sum() == st["moved"] and (shifts[:nr] >= 0).all()
    dropped = int(((orfs["flags"] & K.NONCODING) != 0).sum())
    assert line == (CR.summary_of(regs, start) + CR.orf_summary(orfs[:nr]) + CR.select_summary(sel) + ", free: %d" % (len(orfs) - nr) +
                    ", coding: own, noncoding: %d" % dropped + ", starts: own, moved: %d" % moved.sum())
    assert files[1] == CR.format_orfs(ids, regs, orfs[:nr], fnames, sel=sel[:nr], free=orfs[nr:], free_sel=sel[nr:], cands=orfs,
                                      coding=scores[:nr], free_coding=scores[nr:], shifts=shifts[:nr], free_shifts=shifts[nr:])
    # line by line: the last field is the shift, in front of it the score; a moved ORF has the flag word, the new extent and start
    rows = [ln.split(b"\t") for ln in files[1].splitlines()]
    by_extent = {(ids[int(o["seq"])], int(o["left"]) + 1, int(o["right"]) + 1, b"-" if o["strand"] else b"+", int(o["fI"])): i
                 for i, o in enumerate(orfs)}
    n_moved = 0
    for f in rows:
        assert len(f) == 12
        fi = -1 if f[5] == b"hypothetical protein" else fnames.index(f[5])
        i = by_extent[(f[0], int(f[1]), int(f[2]), f[3], fi)]
        assert int(f[11]) == shifts[i] and int(f[10]) == scores[i] and (b"moved" in f[9].split(b",")) == (shifts[i] > 0)
        assert int(f[7]) == orfs[i]["n_res"] == plain[2][i]["n_res"] - shifts[i] and f[8] == (b"-", b"ATG", b"GTG", b"TTG")[orfs[i]["start_codon"]]
        n_moved += int(shifts[i] > 0)
    assert n_moved > 0
    # the protein file and --select see the new extents
    assert files[2] == CR.format_faa(ids, regs, orfs[:nr], ps[:nr + 1], res[:ps[nr]], fnames, sel=sel[:nr], free=orfs[nr:], free_sel=sel[nr:],
                                     free_prot_start=ps[nr:] - ps[nr], free_residues=res[ps[nr]:])
    i = int(np.flatnonzero(moved & (sel["state"] == 1))[0])
    o = orfs[i]
    head = b">%s_%d_%d_%s " % (ids[int(o["seq"])], o["left"] + 1, o["right"] + 1, b"-" if o["strand"] else b"+")
    assert head in files[2] and files[2].split(head)[1].split(b"\n")[1][:1] == b"M"
    assert sel.tobytes() == S.select_fast(S.of_records(orfs)).tobytes()
    # --all and no --select
    line_all, files_all = run("all", select=True, write_all=True, starts=True, min_train_starts=50)
    assert line_all.endswith(", starts: own, moved: %d" % made[-1].start_stats["moved"])
    assert all(len(ln.split(b"\t")) in (12, 14) for ln in files_all[1].splitlines())
    line_ns, files_ns = run("ns", starts=True, min_train_starts=50)
    assert files_ns[1].count(b"moved") == moved.sum()      # (a moved record is kept and coding: it is written)
    # the saved model: the last round's counts; reading it back chooses the same starts under `model`
    got_model = CR.parse_start_model(open(model, "rb").read())
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got_model, made[0].start_model)) and got_model[1].sum() > 0
    line_m, files_m = run("model", select=True, starts=True, start_model_in=model)
    assert files_m == files and line_m == line.replace("starts: own", "starts: model")
    assert made[-1].start_stats["trained"] == 2 and not made[-1].start_model[0].any()
    # untrained: one warning line, nothing moved; the files are the ones without --starts but for the shift field
    capsys.readouterr()
    line_u, files_u = run("untrained", select=True, starts=True)
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("Warning: ") and "--min-train-starts" in err
    line0, files0 = run("plain", select=True)
    assert line_u == line0 + ", starts: untrained, moved: 0"
    assert files_u[0] == files0[0] and files_u[2] == files0[2]
    assert files_u[1] == b"".join(ln + b"\t0\n" for ln in files0[1].splitlines())
    assert capsys.readouterr().err == ""


@pytest.mark.parametrize("write_all", [False, True])
@pytest.mark.parametrize("select", [False, True])
def test_call_regions_without_starts_writes_the_recorded_bytes(oracle, tmp_path, monkeypatch, write_all, select):
    """Regions, ORF and protein file with --coding and without --starts against the bytes recorded from the writers as they were
    before this option existed: independent of the writers under test."""
    from kmergutsjava_amd import call_regions as CR
    ids, fnames, dna, off, d, q, made = _front_end(oracle, tmp_path, monkeypatch)
    line = CR.call_regions(d, q, str(tmp_path / "p.tsv"), orfs_out=str(tmp_path / "p.orfs"), faa_out=str(tmp_path / "p.faa"), min_hits=4,
                           merge_gap=300, min_score=12, min_len=100, free_min_res=100, coding=True, min_train=1000, write_all=write_all,
                           select=select)
    assert "starts" not in line
    same_as_recorded("coding_" + ("all" if write_all else "written") + ("_select" if select else ""),
                     [(tmp_path / ("p" + ext)).read_bytes() for ext in (".tsv", ".orfs", ".faa")])


def test_starts_options_need_their_partners():
    from kmergutsjava_amd import call_regions as CR
    with pytest.raises(ValueError):
        CR.call_regions("nowhere", "none.fna", "out.tsv", orfs_out="x", starts=True)
    with pytest.raises(ValueError):
        CR.call_regions("nowhere", "none.fna", "out.tsv", orfs_out="x", coding=True, save_start_model="m")
    for argv in (["--orfs", "x", "--starts"], ["--orfs", "x", "--coding", "--start-rounds", "5"], ["--orfs", "x", "--coding", "--start-model", "m"],
                 ["--orfs", "x", "--coding", "--save-start-model", "m"], ["--orfs", "x", "--coding", "--min-train-starts", "5"]):
        with pytest.raises(SystemExit):
            CR.main(["-D", "d", "-q", "q", "-o", "o"] + argv)
    assert CR.starts_summary([1, 0], 3) == ", starts: own, moved: 3" and CR.starts_summary([], 0) == ", starts: untrained, moved: 0"
    assert CR.starts_summary([2], 1) == ", starts: model, moved: 1"
