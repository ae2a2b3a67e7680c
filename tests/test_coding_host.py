"""The coding-potential rule (kg_orfset_coding, include/kmerguts_hip.h) on the CPU: the plain-loop form of tests/coding_model.py
against its numpy form, Lg's known answers, kg_coding_table (host code of the library: no GPU) against the model, the struct
layouts, the model file, and the call_regions front end with the device calls replaced by the models."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import coding_model as K  # noqa: E402
import free_orfs_model as F  # noqa: E402
import orfs_model as O  # noqa: E402
import regions_model as R  # noqa: E402
import select_model as S  # noqa: E402
import test_java_binding as H  # noqa: E402
import test_orfs_host as HO  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

ROOT = os.path.dirname(HERE)


# ---- the two forms of the model ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_plain_loops_match_numpy(seed):
    """50 random small batches per seed: contigs of length 0 to 8 among longer ones, N, lower case and u, both strands, all
    frames, L mod 3 in 0, 1, 2 (asserted over the seeds' batches below)."""
    rng = np.random.default_rng(100 + seed)
    seen_mod, pairs = set(), 0
    for k in range(50):
        if k == 0:                      # every length from 0 to 8, in a random order, among three longer contigs
            orfs, seq, off = K.random_batch(rng, 0, lens=rng.permutation(list(range(9)) + [40, 41, 42]))
        else:
            orfs, seq, off = K.random_batch(rng, int(rng.integers(0, 7)), max_len=120)
        lens = np.diff(off)
        seen_mod |= set((lens % 3).tolist())
        Cl, Bl = K.counts_loops(orfs, seq, off)
        Cn, Bn = K.counts_np(orfs, seq, off)
        assert Cl.tobytes() == Cn.tobytes() and Bl.tobytes() == Bn.tobytes()
        valid = sum(1 for s in range(len(off) - 1) for x in range(int(off[s]), int(off[s + 1]) - 5)
                    if all(K._CODE[seq[x + i]] < 4 for i in range(6)))
        assert Bl.sum() == 2 * valid
        T = rng.integers(-3000, 3000, size=K.BINS).astype(np.int32)
        assert K.scores_loops(T, orfs, seq, off).tobytes() == K.scores_np(T, orfs, seq, off).tobytes()
        mc, mt = int(rng.integers(-50, 50)), int(rng.integers(0, 30))
        a = K.coding(orfs, seq, off, None, mc, mt, loops=True)
        b = K.coding(orfs, seq, off, None, mc, mt)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
        pairs += int(Cl.sum())
        for o in orfs:
            assert len(K.pairs_loops(o, seq, off)) == max(int(o["n_res"]) - 1, 0)
    assert seen_mod == {0, 1, 2} and pairs > 50


def test_known_answers_of_one_contig():
    """ATG AAA CCC TAA on '+' and its reverse complement on '-': pairs ATGAAA, AAACCC; the stop is in no pair."""
    idx = lambda s: sum("ACGT".index(ch) << (2 * (5 - i)) for i, ch in enumerate(s))    # noqa: E731
    contig = b"GGATGAAACCCTAAG"
    off = np.array([0, len(contig)], np.int64)
    plus = K.records([K.orf(0, 0, 2, 13, 3)])
    assert K.pairs_loops(plus[0], contig, off) == [idx("ATGAAA"), idx("AAACCC")]
    rcb = HO._rc(contig)
    minus = K.records([K.orf(0, 1, len(contig) - 1 - 13, len(contig) - 1 - 2, 3)])
    assert K.pairs_loops(minus[0], rcb, off) == [idx("ATGAAA"), idx("AAACCC")]
    assert K.pairs_np(minus[0], np.frombuffer(rcb, np.uint8), off).tolist() == [idx("ATGAAA"), idx("AAACCC")]
    # an unknown base in the first or the second codon of a pair takes the pair away; u / U and lower case are T and known
    assert K.pairs_loops(plus[0], b"GGATNAAACCCTAAG", off) == [-1, idx("AAACCC")]
    assert K.pairs_loops(plus[0], b"GGATGAAACNCTAAG", off) == [idx("ATGAAA"), -1]
    assert K.pairs_loops(plus[0], b"GGaugAaAcCCUAAG", off) == [idx("ATGAAA"), idx("AAACCC")]
    assert K.rc(idx("ATGAAA")) == idx("TTTCAT") and K.rc(idx("AAAAAA")) == idx("TTTTTT") and K.rc(K.rc(1234)) == 1234
    # background: 10 hexamer starts, every one counted with its reverse complement; contigs of 5 give none, a junction none
    C_, B = K.counts_loops(plus, contig, off)
    assert C_.sum() == 2 and B.sum() == 20 and B[idx("GGATGA")] == 1 and B[idx("TCATCC")] == 1
    two = np.array([0, 5, 10], np.int64)
    assert K.background_np(b"ACGTAACGTA", two).sum() == 0 and K.background_np(b"ACGTAACGTA", np.array([0, 10], np.int64)).sum() == 10


# ---- Lg and the table ---------------------------------------------------------------------------------------------------------------

def test_lg_known_answers():
    assert [K.lg(x) for x in (1, 2, 3, 4096, (1 << 63) - 1)] == [0, 256, 405, 3072, 16127]
    rng = np.random.default_rng(7)
    xs = list(range(1, 300)) + [int(x) for x in rng.integers(1, 1 << 62, size=300)] + [int(rng.integers(1, 1 << b)) for b in range(1, 63) for _ in range(3)]
    for x in xs:
        exact = (x ** 256).bit_length() - 1             # floor(256 log2 x)
        assert abs(K.lg(x) - exact) <= 1, x


def _lib_table(coding, background):
    lib = N.load()
    m = N.KgCodingModel()
    C.memmove(m.coding, np.ascontiguousarray(coding, dtype=np.int64).ctypes.data, 8 * K.BINS)
    C.memmove(m.background, np.ascontiguousarray(background, dtype=np.int64).ctypes.data, 8 * K.BINS)
    out = np.full(K.BINS, 12345, dtype=np.int32)
    return lib.kg_coding_table(C.byref(m), out.ctypes.data), out


def test_kg_coding_table_matches_the_model(native):
    from kmergutsjava_amd import hotpath
    zero = np.zeros(K.BINS, np.int64)
    rc, T = _lib_table(zero, zero)
    assert rc == 0 and not T.any()
    one = zero.copy()
    one[777] = 1 << 40
    for Cc, Bb in ((one, zero), (zero, one), (one, one)):
        rc, T = _lib_table(Cc, Bb)
        assert rc == 0 and T.tobytes() == K.table(Cc, Bb).tobytes()
    # Lg(2^40 + 1) = Lg(2^40 + 4096) = 10240 and SB = 4096: T = 3072 in the bin and -10240 + 3072 elsewhere
    T = _lib_table(one, zero)[1]
    assert T[777] == 3072 and T[0] == -7168 and (np.delete(T, 777) == -7168).all()
    rng = np.random.default_rng(3)
    for hi in (2, 1000, 1 << 30, 1 << 49):
        Cc, Bb = rng.integers(0, hi, size=K.BINS), rng.integers(0, hi, size=K.BINS)
        rc, T = _lib_table(Cc, Bb)
        assert rc == 0 and T.tobytes() == K.table(Cc, Bb).tobytes()
        assert hotpath.coding_table(Cc, Bb).tobytes() == T.tobytes()
    top = zero.copy()
    top[0] = top[4095] = (1 << 61) - 1                  # the largest sum the rule takes: 2^62 - 2
    rc, T = _lib_table(top, top)
    assert rc == 0 and T.tobytes() == K.table(top, top).tobytes()


def test_kg_coding_table_errors(native):
    lib = N.load()
    zero = np.zeros(K.BINS, np.int64)
    neg = zero.copy()
    neg[9] = -1
    rc, T = _lib_table(neg, zero)
    assert rc == N.KG_ERR_ARG and b"coding count 9" in lib.kg_last_error() and (T == 12345).all()
    rc, _ = _lib_table(zero, neg)
    assert rc == N.KG_ERR_ARG and b"background count 9" in lib.kg_last_error()
    big = zero.copy()
    big[1] = big[2] = 1 << 61
    rc, _ = _lib_table(big, zero)
    assert rc == N.KG_ERR_ARG and b"2^62" in lib.kg_last_error()
    rc, _ = _lib_table(zero, big)
    assert rc == N.KG_ERR_ARG and b"2^62" in lib.kg_last_error()
    m, out = N.KgCodingModel(), np.zeros(K.BINS, np.int32)
    assert lib.kg_coding_table(None, out.ctypes.data) == N.KG_ERR_ARG and lib.kg_coding_table(C.byref(m), None) == N.KG_ERR_ARG
    from kmergutsjava_amd import hotpath
    with pytest.raises(ValueError):
        hotpath.coding_table(np.zeros(10, np.int64), zero)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------

def test_structs_match_the_c_layout_and_the_jna_source(tmp_path):
    width = {"int32_t": "int", "uint32_t": "int", "int64_t": "long", "float": "float"}
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    lines = []
    for cname, jname, py in (("kg_coding_params", "KgCodingParams", N.KgCodingParams), ("kg_coding_stats", "KgCodingStats", N.KgCodingStats)):
        cf = H._c_struct(cname)
        jf, order = H._java_struct(jname)
        assert [n for n, _ in jf] == [n for n, _ in cf] == order == [n for n, _ in py._fields_], cname
        assert [t for _, t in jf] == [width[t] for _, t in cf] and [t for _, t in py._fields_] == [ctype[t] for _, t in cf], cname
        lines.append('printf("%%zu\\n", sizeof(%s));\n' % cname)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f, _ in cf]
    lines.append('printf("%zu %zu %zu %u\\n", sizeof(kg_coding_model), offsetof(kg_coding_model, coding), offsetof(kg_coding_model, background), KG_ORF_NONCODING);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for py in (N.KgCodingParams, N.KgCodingStats):
        want += [C.sizeof(py)] + [getattr(py, f).offset for f, _ in py._fields_]
    want += [C.sizeof(N.KgCodingModel), N.KgCodingModel.coding.offset, N.KgCodingModel.background.offset, N.ORF_NONCODING]
    assert out == want and C.sizeof(N.KgCodingParams) == 16 and C.sizeof(N.KgCodingStats) == 56 and C.sizeof(N.KgCodingModel) == 65536
    assert N.ORF_NONCODING == K.NONCODING == 32 and N.CODING_BINS == K.BINS
    j = H._strip_comments(H.JAVA)
    assert "public long[] coding = new long[4096]" in j and "public long[] background = new long[4096]" in j
    assert {"kg_orfset_coding", "kg_orfset_coding_scores", "kg_orfset_coding_stats", "kg_orfset_coding_model", "kg_coding_table",
            "kg_coding_counts_orfs", "kg_coding_score_orfs"} <= set(N.EXPORTS)


def test_constants_match_the_kernels():
    src = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_coding.hpp")).read()
    assert "constexpr int kCodingBgPerLane = %d;" % N.CODING_BG_PER_LANE in src
    assert "constexpr int kCodingThreads = 256;" in src and N.CODING_BG_TILE == 256 * N.CODING_BG_PER_LANE
    assert "constexpr uint32_t kCodingMaxGrid = %d;" % N.CODING_MAX_GRID in src


def test_the_kernels_use_no_scratch_and_do_not_spill():
    """From the compiler's own report (tools/kernel_resources.py), as tests/test_kernel_resources.py reads it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not found")
    res = kr.resources()
    for k in ("coding_background_kernel", "coding_fold_kernel", "coding_lens_kernel", "coding_count_kernel", "coding_score_kernel",
              "coding_decide_kernel"):
        assert k in res, (k, sorted(res))
        assert res[k]["sgpr_spills"] == 0 and res[k]["vgpr_spills"] == 0 and res[k]["scratch"] == 0, (k, res[k])


# ---- the model file ---------------------------------------------------------------------------------------------------------------

def test_model_file_round_trip():
    from kmergutsjava_amd import call_regions as CR
    from kmergutsjava_amd.make_signatures import InputError
    rng = np.random.default_rng(1)
    Cc, Bb = rng.integers(0, 1 << 50, size=K.BINS), rng.integers(0, 1 << 20, size=K.BINS)
    text = CR.format_coding_model(Cc, Bb)
    lines = text.split(b"\n")
    assert lines[0] == b"#kmerguts coding model 1" and len(lines) == 4098 and lines[-1] == b""
    assert lines[1] == b"AAAAAA\t%d\t%d" % (Cc[0], Bb[0]) and lines[2].startswith(b"AAAAAC\t") and lines[4096].startswith(b"TTTTTT\t")
    assert lines[1 + 0b000110110001].startswith(b"ACGTAC\t")          # the first base is the most significant digit
    c2, b2 = CR.parse_coding_model(text)
    assert c2.tobytes() == Cc.astype(np.int64).tobytes() and b2.tobytes() == Bb.astype(np.int64).tobytes()
    assert CR.parse_coding_model(text.replace(b"\n", b"\r\n"))[0].tobytes() == c2.tobytes()
    for bad, word in ((b"#kmerguts coding model 2\n" + text.partition(b"\n")[2], "first line"), (text[:-20], "line 4097"),
                      (text + b"AAAAAA\t1\t1\n", "4097 lines"), (text.replace(b"AAAAAC\t", b"AAAACA\t", 1), "line 3"),
                      (text.replace(b"\nAAAAAG\t", b"\nAAAAAG\tx", 1), "line 4"), (b"", "first line")):
        with pytest.raises(InputError) as ei:
            CR.parse_coding_model(bad, "m.txt")
        assert word in str(ei.value) and "m.txt" in str(ei.value), (word, str(ei.value))


# ---- the front end, the device calls replaced by the models -------------------------------------------------------------------------

class _ModelScan:
    """What call_regions uses of a ScanResult, computed by the models from the oracle's CALL records."""

    def __init__(self, calls, seq, off):
        self.calls, self.seq, self.off = calls, seq, off
        self.stats = {"n_seqs": len(off) - 1}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def regions(self, offsets, merge_gap=600, min_score=0, min_len=0):
        return R.regions(self.calls, self.off, merge_gap, min_score, min_len)

    def orfs(self, seq, offsets, merge_gap=600, min_score=0, min_len=0, start_codons=7, only_kept=True, device_ptr=None,
             free_min_res=None, coding=None, min_coding=0, min_train_pairs=100000):
        regs, start = self.regions(offsets, merge_gap, min_score, min_len)
        got = O.orfs(regs, self.seq, self.off, start_codons, only_kept)
        if free_min_res is not None:
            got = F.concat(got, F.free_orfs(self.seq, self.off, free_min_res, start_codons))
        if coding is not None:
            recs, self.coding_scores, self.coding_stats, self.coding_model = K.coding(
                got[0], self.seq, self.off, None if coding is True else coding, min_coding, min_train_pairs)
            got = (recs,) + tuple(got[1:])
        return (regs, start) + tuple(got)

    def select(self, offsets, seq=None, merge_gap=600, min_score=0, min_len=0, orfs=False, start_codons=7, only_kept=True,
               device_ptr=None, max_overlap=60, max_overlap_pct=50, free_min_res=None, coding=None, min_coding=0, min_train_pairs=100000):
        assert orfs
        got = self.orfs(seq, offsets, merge_gap, min_score, min_len, start_codons, only_kept, None, free_min_res, coding, min_coding,
                        min_train_pairs)
        return got + (S.select_fast(S.of_records(got[2]), max_overlap, max_overlap_pct),)


_WORK = {}


def _front_end(oracle, tmp_path, monkeypatch):
    from kmergutsjava_amd import kmer_guts_java as KGJ
    if not _WORK:
        img, dna, off, genes = HO.planted_orf_contigs()
        _WORK["w"] = (img, dna, off)
    img, dna, off = _WORK["w"]
    n = len(off) - 1
    ids = [b"contig_%d" % k for k in range(n)]
    (tmp_path / "c.fna").write_bytes(b"".join(b">%s\n%s\n" % (ids[k], dna[off[k]:off[k + 1]]) for k in range(n)))
    d = tmp_path / "d"
    d.mkdir()
    (d / "kmer.table.mem_map").write_bytes(b"not read: the scan is the model's")
    fnames = [b"synthetic function %d" % i for i in range(50)]
    (d / "function.index").write_bytes(b"".join(b"%d\t%s\n" % (i, f) for i, f in enumerate(fnames)))
    made = []

    class _Table:
        def scan(self, batch, boff, params):
            ora = oracle.run(img, np.frombuffer(batch, dtype=np.uint8), boff, lookup_mode=1, min_hits=params.min_hits)
            made.append(_ModelScan(ora["calls"], batch, np.asarray(boff, dtype=np.int64)))
            return made[-1]

    monkeypatch.setattr(KGJ, "_resident_table", lambda path, device: _Table())
    return ids, fnames, dna, off, str(d), str(tmp_path / "c.fna"), made


def test_call_regions_with_coding_against_the_models(oracle, tmp_path, monkeypatch, capsys):
    from kmergutsjava_amd import call_regions as CR
    ids, fnames, dna, off, d, q, made = _front_end(oracle, tmp_path, monkeypatch)
    kw = dict(min_hits=4, merge_gap=300, min_score=12, min_len=100)

    def run(tag, **more):
        line = CR.call_regions(d, q, str(tmp_path / (tag + ".tsv")), orfs_out=str(tmp_path / (tag + ".orfs")),
                               faa_out=str(tmp_path / (tag + ".faa")), **kw, **more)
        return line, [(tmp_path / (tag + ext)).read_bytes() for ext in (".tsv", ".orfs", ".faa")]

    model = str(tmp_path / "model.txt")
    line, files = run("sel", select=True, free_min_res=100, coding=True, min_train=1000, save_coding_model=model)
    regs, start, orfs, ps, res, sel = made[-1].select(off, dna, 300, 12, 100, True, 7, True, free_min_res=100, coding=True, min_train_pairs=1000)
    nr, scores, st = len(regs), made[-1].coding_scores, made[-1].coding_stats
    free = orfs[nr:]
    dropped = (free["flags"] & K.NONCODING) != 0
    assert st["trained"] == 1 and 0 < dropped.sum() < len(free) and (scores[nr:][dropped] < 0).all() and (free["kept"][dropped] == 0).all()
    assert (sel["state"][nr:][dropped] == 0).all()
    assert line == (CR.summary_of(regs, start) + CR.orf_summary(orfs[:nr]) + CR.select_summary(sel) + ", free: %d" % len(free) +
                    ", coding: own, noncoding: %d" % dropped.sum())
    assert files[1] == CR.format_orfs(ids, regs, orfs[:nr], fnames, sel=sel[:nr], free=free, free_sel=sel[nr:], cands=orfs,
                                      coding=scores[:nr], free_coding=scores[nr:])
    # line by line: the written free ORFs are the selected ones, none of them non-coding, the last field is the record's score
    rows = [ln.split(b"\t") for ln in files[1].splitlines()]
    by_extent = {(ids[int(o["seq"])], int(o["left"]) + 1, int(o["right"]) + 1, b"-" if o["strand"] else b"+"): (i, o) for i, o in enumerate(orfs)
                 if i >= nr}
    n_free_lines = 0
    for f in rows:
        assert len(f) == 11
        if f[5] == b"hypothetical protein":
            i, o = by_extent[(f[0], int(f[1]), int(f[2]), f[3])]
            assert sel["state"][i] == 1 and not o["flags"] & K.NONCODING and int(f[10]) == scores[i] >= 0 and b"noncoding" not in f[9]
            n_free_lines += 1
    assert n_free_lines == int((sel["state"][nr:] == 1).sum()) > 0
    assert files[2] == CR.format_faa(ids, regs, orfs[:nr], ps[:nr + 1], res[:ps[nr]], fnames, sel=sel[:nr], free=free, free_sel=sel[nr:],
                                     free_prot_start=ps[nr:] - ps[nr], free_residues=res[ps[nr]:])
    # a dropped free ORF suppresses nothing: the selection without the filter selects fewer or other free ORFs
    plain = made[-1].select(off, dna, 300, 12, 100, True, 7, True, free_min_res=100)
    assert plain[5][:nr].tobytes() == sel[:nr].tobytes() and plain[5].tobytes() != sel.tobytes()
    # --all: every candidate; a non-coding one with its flag word and status
    line_all, files_all = run("all", select=True, free_min_res=100, coding=True, min_train=1000, write_all=True)
    rows = [ln.split(b"\t") for ln in files_all[1].splitlines()]
    hyp = [f for f in rows if f[5] == b"hypothetical protein"]
    assert len(hyp) == len(free) and all(len(f) == 13 for f in hyp)
    assert sum(f[10] == b"noncoding" for f in hyp) == sum(b"noncoding" in f[9].split(b",") for f in hyp) == dropped.sum()
    assert all((f[10] == b"noncoding") == (int(f[12]) < 0) for f in hyp) and all(f[11] == b"-" for f in hyp if f[10] == b"noncoding")
    assert line_all.endswith(", coding: own, noncoding: %d" % dropped.sum())
    # without --select: every coding free ORF, no non-coding one, in both files
    line_ns, files_ns = run("ns", free_min_res=100, coding=True, min_train=1000)
    assert files_ns[1].count(b"hypothetical protein") == len(free) - dropped.sum()
    # the saved model: the counts of the one batch; reading it back gives the same scores under `model`
    Cc, Bb = CR.parse_coding_model(open(model, "rb").read())
    assert Cc.tobytes() == made[-1].coding_model[0].tobytes() and Bb.tobytes() == made[-1].coding_model[1].tobytes() and Cc.sum() == st["training_pairs"]
    line_m, files_m = run("model", select=True, free_min_res=100, coding=True, coding_model_in=model)
    assert files_m == files and line_m == line.replace("coding: own", "coding: model")
    assert made[-1].coding_stats["trained"] == 2 and not made[-1].coding_model[0].any()
    # untrained: one warning line, scores 0, nothing dropped; the files are the ones without --coding but for the score field
    capsys.readouterr()
    line_u, files_u = run("untrained", select=True, free_min_res=100, coding=True, min_train=10 ** 9)
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("Warning: ") and "--min-train" in err
    line0, files0 = run("plain", select=True, free_min_res=100)
    assert line_u == line0 + ", coding: untrained, noncoding: 0"
    assert files_u[0] == files0[0] and files_u[2] == files0[2]
    assert files_u[1] == b"".join(ln + b"\t0\n" for ln in files0[1].splitlines())
    assert capsys.readouterr().err == ""


def recorded_before_coding(key: str) -> dict:
    """tests/golden/call_regions_planted_before_coding.json: sha256, bytes and lines of the three files the front end wrote for
    the planted contigs before it knew --coding (recorded from that commit's writers), for run `key`."""
    import json
    return json.load(open(os.path.join(HERE, "golden", "call_regions_planted_before_coding.json")))["runs"][key]


def same_as_recorded(key: str, files) -> None:
    import hashlib
    want = recorded_before_coding(key)
    for name, data in zip(("tsv", "orfs", "faa"), files):
        got = {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data), "lines": data.count(b"\n")}
        assert got == want[name], (key, name, got, want[name])


@pytest.mark.parametrize("write_all", [False, True])
@pytest.mark.parametrize("select", [False, True])
def test_call_regions_without_coding_writes_the_recorded_bytes(oracle, tmp_path, monkeypatch, write_all, select):
    """Regions, ORF and protein file without --coding against the bytes recorded from the writers as they were before this
    option existed: independent of the writers under test."""
    from kmergutsjava_amd import call_regions as CR
    ids, fnames, dna, off, d, q, made = _front_end(oracle, tmp_path, monkeypatch)
    line = CR.call_regions(d, q, str(tmp_path / "p.tsv"), orfs_out=str(tmp_path / "p.orfs"), faa_out=str(tmp_path / "p.faa"), min_hits=4,
                           merge_gap=300, min_score=12, min_len=100, free_min_res=100, write_all=write_all, select=select)
    assert "coding" not in line
    same_as_recorded(("all" if write_all else "written") + ("_select" if select else ""),
                     [(tmp_path / ("p" + ext)).read_bytes() for ext in (".tsv", ".orfs", ".faa")])


def test_call_regions_without_coding_writes_what_it_wrote(oracle, tmp_path, monkeypatch):
    """The writers with the new arguments left out give the bytes of the ones this change found (their code paths restated
    here from the records)."""
    from kmergutsjava_amd import call_regions as CR
    ids, fnames, dna, off, d, q, made = _front_end(oracle, tmp_path, monkeypatch)
    line = CR.call_regions(d, q, str(tmp_path / "p.tsv"), orfs_out=str(tmp_path / "p.orfs"), faa_out=str(tmp_path / "p.faa"), min_hits=4,
                           merge_gap=300, min_score=12, min_len=100, free_min_res=100, write_all=True, select=True)
    assert "coding" not in line
    regs, start, orfs, ps, res, sel = made[-1].select(off, dna, 300, 12, 100, True, 7, False, free_min_res=100)
    nr = len(regs)
    want = []
    for i, o in enumerate(orfs):
        words = b",".join(w for bit, w in ((1, b"stop"), (2, b"partial5"), (4, b"interrupted"), (8, b"multi-frame"), (16, b"free")) if o["flags"] & bit)
        row = b"%s\t%d\t%d\t%s\t%d\t%s\t%d\t%d\t%s\t%s" % (
            ids[o["seq"]], o["left"] + 1, o["right"] + 1, b"-" if o["strand"] else b"+", o["frame"],
            fnames[o["fI"]] if i < nr else b"hypothetical protein", o["score"], o["n_res"],
            (b"ATG", b"GTG", b"TTG")[o["start_codon"] - 1] if o["start_codon"] else b"-", words or b"-")
        if i >= nr:
            by = sel["by"][i]
            w = orfs[by] if by >= 0 else None
            row += b"\t%s\t%s" % (b"overlapped" if sel["state"][i] == 2 else b"kept",
                                  b"-" if w is None else b"%d..%d:%s" % (w["left"] + 1, w["right"] + 1, b"-" if w["strand"] else b"+"))
        want.append((int(o["seq"]), i >= nr, row + b"\n"))
    assert (tmp_path / "p.orfs").read_bytes() == b"".join(t for _, _, t in sorted(want, key=lambda x: x[:2]))


def test_coding_options_need_their_partners():
    from kmergutsjava_amd import call_regions as CR
    with pytest.raises(ValueError):
        CR.call_regions("nowhere", "none.fna", "out.tsv", coding=True)
    with pytest.raises(ValueError):
        CR.call_regions("nowhere", "none.fna", "out.tsv", orfs_out="x", save_coding_model="m")
    for argv in (["--coding"], ["--orfs", "x", "--min-coding", "5"], ["--orfs", "x", "--coding-model", "m"],
                 ["--orfs", "x", "--save-coding-model", "m"], ["--orfs", "x", "--min-train", "5"]):
        with pytest.raises(SystemExit):
            CR.main(["-D", "d", "-q", "q", "-o", "o"] + argv)
    assert CR.coding_summary([1, 0], 3) == ", coding: own, noncoding: 3" and CR.coding_summary([], 0) == ", coding: untrained, noncoding: 0"
    assert CR.coding_summary([2], 1) == ", coding: model, noncoding: 1"
