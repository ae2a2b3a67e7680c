"""The band rule's two model forms (tests/band_model.py) against each other, against align_model and ungapped_model at the band's
two ends and against answers that follow from how the inputs are made; the three structures against gcc's layout and the JNA
source; the front end with the model in the device's place; and the carry bound of kg_band.hpp.  CPU-only."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import align_model as A
import band_model as B
import ops_model as O
import search_model as S
import trace_model as T
import ungapped_model as UM
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import search_proteins as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = np.frombuffer(A.ALPHA + b"X", dtype=np.uint8)


def _random_pair(rng):
    n, m = int(rng.integers(0, 41)), int(rng.integers(0, 41))
    a = LETTERS[rng.integers(0, 21, n)].tobytes()
    if rng.random() < 0.6 and n:                       # related: a window of a, mutated, so that alignments are long
        at = int(rng.integers(0, n))
        b = (A.mutate(rng, a[at:], 0.15) + LETTERS[rng.integers(0, 21, m)].tobytes())[:m]
    else:
        b = LETTERS[rng.integers(0, 21, m)].tobytes()
    return a, b


def test_loops_numpy_and_the_four_consequences_on_random_pairs():
    rng = np.random.default_rng(2025)
    positive = traced = 0
    for _ in range(300):
        a, b = _random_pair(rng)
        n, m = len(a), len(b)
        g, W = int(rng.integers(-45, 46)), int(rng.integers(0, 13))
        got = B.band_numpy(a, b, g, W)
        assert got == B.band_loops(a, b, g, W), (a, b, g, W)
        full = A.sw_numpy(a, b)
        assert got[0] <= full[0]                                                            # banded <= full
        cover = B.covering(n, m, g)
        assert B.band_numpy(a, b, g, cover) == full == B.band_loops(a, b, g, cover)         # a covering band is the full alignment
        assert B.band_numpy(a, b, g, 0)[0] == UM.ungapped_numpy(a, b, g) == UM.ungapped_loops(a, b, g)     # W = 0 is u
        assert B.band_numpy(a, b, n + W, W) == (0, -1, -1) == B.band_numpy(a, b, -(m + W), W)             # a band that misses
        if got[0] > 0:
            positive += 1
            assert B.in_band(got[1], got[2], g, W)
            end, rec, cols = B.band_trace(a, b, g, W)
            assert end == got and B.band_trace(a, b, g, W, tables=B.tables_loops) == (end, rec, cols)
            if full[0] > 0 and cover <= 40:
                traced += 1
                assert B.band_trace(a, b, g, cover) == T.trace_numpy(a, b, with_columns=True)      # paths and columns at a covering W
                for mode in O.MODES:
                    _, rec_c, cols_c = B.band_trace(a, b, g, cover)
                    assert O.encode(O.kinds_of(a[:end[1] + 1], b[:end[2] + 1], rec, cols, mode)) is not None
                    assert O.encode(O.kinds_of(a[:full[1] + 1], b[:full[2] + 1], rec_c, cols_c, mode)) == O.ops_of(a, b, mode=mode)[2]
            # every column of the walk lies in the band
            i, j = end[1], end[2]
            for c in cols:
                assert B.in_band(i, j, g, W)
                i, j = (i - 1, j - 1) if c == "M" else (i, j - 1) if c == "E" else (i - 1, j)
    assert positive > 100 and traced > 50


def test_the_hand_made_cases():
    for lp in (30, 61):
        for mirror in (False, True):
            a, b, joined, half = B.insert_case(6, lp, mirror)
            assert A.sw_numpy(a, b)[0] == joined and B.band_numpy(a, b, 0, 6)[0] == joined == B.band_loops(a, b, 0, 6)[0]
            assert B.band_numpy(a, b, 0, 5)[0] == half == B.band_loops(a, b, 0, 5)[0] == 11 * lp
            _, rec, cols = B.band_trace(a, b, 0, 6)
            assert cols.count("E" if mirror else "F") == 6 and rec[4] == 1
    a, b, x_score, joined = B.feature_case()
    assert tuple(A.sw_numpy(a, b)) == (joined, 89, 129) and B.band_numpy(a, b, 0, 8) == (x_score, 59, 59)
    end, rec, cols = B.band_trace(a, b, 0, 8)
    assert cols == "M" * 60 and rec == (0, 0, 60, 60, 0, 0, 0)
    for case, want in B.tie_cases():
        assert B.band_numpy(*case) == want == B.band_loops(*case), case


def test_the_cap_and_the_batch_model():
    assert B.band_cells(300, 300, 8) == 5100 and B.band_cells(5, 300, 8) == 85 and B.band_cells(5, 300, 256) == 1500
    assert B.band_cells(0, 10, 3) == 0 and B.band_cells(1 << 23, 1 << 23, 256) == 513 << 23
    rng = np.random.default_rng(3)
    p = A.M.random_protein(rng, 60)
    seq, off = S.batch([p, A.mutate(rng, p, 0.1)])
    aln = B.align_model(seq, off, [(0, 1), (0, 1)], [0, 90], 4, max_cells=60 * 9)
    assert list(aln["status"]) == [N.ALIGN_ALIGNED] * 2 and aln[0]["score"] > 0 and tuple(aln[1])[:5:3] == (0, -1)
    assert list(B.align_model(seq, off, [(0, 1)], [0], 4, max_cells=60 * 9 - 1)["status"]) == [N.ALIGN_SKIPPED]
    pth, starts, ops = B.ops_model(seq, off, [(0, 1), (0, 1)], [0, 90], 4, aln, "eqx")
    assert list(pth["status"]) == [N.PATH_TRACED, N.PATH_NONE] and list(starts) == [0, len(ops), len(ops)] and len(ops) > 0


def test_the_search_model_against_the_filtered_model():
    prots, n_db = B.indel_search(7)
    seq, off = S.batch(prots)
    full = UM.filtered_model(seq, off, n_db)
    wide = B.search_model(seq, off, n_db, 256)
    assert wide[0].tobytes() == full[0].tobytes() and wide[2].tobytes() == full[2].tobytes() and wide[3] == full[3] and wide[4] == full[4]
    narrow = B.search_model(seq, off, n_db, 2)
    by_pair = {(int(h["query"]), int(h["target"])): int(h["score"]) for h in full[0]}
    assert len(narrow[0]) == len(full[0]) > 0
    for h, u in zip(narrow[0], narrow[2]):
        assert int(u["ungapped"]) <= int(h["score"]) <= by_pair[(int(h["query"]), int(h["target"]))]
    assert any(int(h["score"]) < by_pair[(int(h["query"]), int(h["target"]))] for h in narrow[0])          # the indels cost something
    zero = B.search_model(seq, off, n_db, 0)
    assert list(zero[0]["score"]) == list(zero[2]["ungapped"])
    assert narrow[5]["full_cells"] == narrow[3]["cells"] and 0 < narrow[5]["band_cells"] < narrow[5]["full_cells"]


# ---- the ABI --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,binding,size", [("kg_band_params", N.KgBandParams, 16), ("kg_band_stats", N.KgBandStats, 24)])
def test_the_bindings_match_the_c_structs(cname, binding, size, tmp_path):
    fields = [f for f, _ in binding._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%%zu\\n%%d\\n", sizeof(%s), KG_BAND_MAX);\n' % cname +
                   "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(binding) == size and out[1] == N.BAND_MAX == B.BAND_MAX == 256
    assert out[2:] == [getattr(binding, f).offset for f in fields]


def test_exports_the_jna_source_and_the_documents():
    names = {"kg_proteins_align_banded", "kg_proteins_align_banded_device", "kg_proteins_search_banded", "kg_proteins_search_banded_device",
             "kg_hitset_band_stats"}
    assert names <= set(N.EXPORTS)
    java = open(os.path.join(ROOT, "java", "kmergutsjava", "KmerGutsHip.java")).read()
    for name in names:
        assert re.search(r"\bint %s\(" % name, java), name
    for cls, order in (("KgBandParams", ["band", "reserved"]), ("KgBandStats", ["band_cells", "full_cells", "band", "reserved"])):
        body = java[java.index("class %s " % cls):]
        got = re.search(r"setFieldOrder\(new String\[\] \{([^}]*)\}\)", body).group(1)
        assert [x.strip().strip('"') for x in got.split(",")] == order, cls
    assert "public int[] reserved = new int[3];" in java[java.index("class KgBandParams "):java.index("class KgBandStats ")]
    hdr = open(os.path.join(ROOT, "include", "kmerguts_hip.h")).read()
    for words in ("|(i - j) - g| <= W", "band must be in [0, 256]", "min(n * m, min(n, m) * (2 W + 1))", "kg_band_params.reserved must be 0"):
        assert words in hdr, words
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "--band" in open(os.path.join(ROOT, name)).read() or "kg_proteins_search_banded" in open(os.path.join(ROOT, name)).read(), name


def test_the_carry_bound_of_the_kernel_fits_the_alignment_kernel_s_lds():
    band = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_band.hpp")).read()
    align = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_align.hpp")).read()
    band_max = int(re.search(r"constexpr int kBandMax = (\d+);", band).group(1))
    assert band_max == N.BAND_MAX
    assert re.search(r"constexpr int kBandCarryCols = 2 \* kBandMax \+ kWave;", band)
    lds_cols = int(re.search(r"constexpr int kAlignLdsCols = (\d+);", align).group(1))
    # one stripe's window: columns i0 - g - W .. i0 + 63 - g + W
    assert (64 - 1 + band_max) - (0 - band_max) + 1 == 2 * band_max + 64 <= lds_cols
    assert "__shared__ int2 lds_carry[kBandCarryCols];" in band


# ---- the front end ---------------------------------------------------------------------------------------------------------------

def _fasta(ids, prots) -> bytes:
    return b"".join(b">" + i + b"\n" + p + b"\n" for i, p in zip(ids, prots))


def _model_search(seen):
    def search(seq, offsets, n_db, ungapped=None, band=None, min_shared=2, max_cand=8, max_db_per_kmer=256, align=None, device=0, paths=None,
               ops=None, **kw):
        seen.clear()
        seen.update(kw, ungapped=ungapped, band=band, paths=paths, ops=ops)
        if band is None:
            hits, start, ung, counts, ucounts = UM.filtered_model(seq, offsets, n_db, min_ungapped=ungapped["min_score"], min_shared=min_shared,
                                                                  max_cand=max_cand)
            return hits, start, dict(counts, ungapped=dict(ucounts, ms_ungapped=0.5)), ung
        hits, start, ung, counts, ucounts, bcounts = B.search_model(seq, offsets, n_db, band, min_ungapped=ungapped["min_score"],
                                                                    min_shared=min_shared, max_cand=max_cand)
        st = dict(counts, ungapped=dict(ucounts, ms_ungapped=0.5), band=bcounts)
        if paths is None:
            return hits, start, st, ung
        pth, starts, opsv = B.search_ops_model(seq, offsets, n_db, band, hits, ung, ops or "m", paths)
        st.update(traced=int((pth["status"] == N.PATH_TRACED).sum()), untraced=0)
        return (hits, start, pth, st) + ((starts, opsv) if ops else ()) + (ung,)
    return search


def test_the_writers_and_the_summary_line_with_the_model_in_the_device_s_place(tmp_path):
    prots, n_db = B.indel_search(11, n_targets=6, n_related=4, length=80)
    ids = [b"p%d" % k for k in range(len(prots))]
    db, qs = tmp_path / "db.faa", tmp_path / "q.faa"
    db.write_bytes(_fasta(ids[:n_db], prots[:n_db]))
    qs.write_bytes(_fasta(ids[n_db:], prots[n_db:]))
    seen = {}
    plain_out, out = tmp_path / "plain.tsv", tmp_path / "b.tsv"
    plain = SP.search_proteins([str(db)], [str(qs)], str(plain_out), write_all=True, search=_model_search(seen), ungapped=dict(min_score=0))
    assert seen["band"] is None and ", band:" not in plain
    line = SP.search_proteins([str(db)], [str(qs)], str(out), write_all=True, search=_model_search(seen), ungapped=dict(min_score=0), band=4)
    assert seen["band"] == 4
    seq, off = S.batch(prots)
    want = B.search_model(seq, off, n_db, 4)
    assert line.endswith(", band: 4, band cells: %d of %d" % (want[5]["band_cells"], want[5]["full_cells"]))
    assert out.read_bytes() == SP.format_hits(ids[n_db:], ids[:n_db], want[0], want[1], write_all=True, ungapped=want[2])
    assert [len(r.split(b"\t")) for r in out.read_bytes().splitlines()] == [len(r.split(b"\t")) for r in plain_out.read_bytes().splitlines()]
    # with --paths and --cigar: the banded paths and ops
    line = SP.search_proteins([str(db)], [str(qs)], str(out), write_all=True, search=_model_search(seen), ungapped=dict(min_score=0), band=4,
                              paths="all", cigar="m")
    pth, starts, ops = B.search_ops_model(seq, off, n_db, 4, want[0], want[2], "m", "all")
    assert out.read_bytes() == SP.format_hits(ids[n_db:], ids[:n_db], want[0], want[1], write_all=True, paths=pth,
                                              qlens=[len(p) for p in prots[n_db:]], dlens=[len(p) for p in prots[:n_db]], cigars=(starts, ops),
                                              ungapped=want[2])
    assert ", band: 4, band cells: " in line and seen["ops"] == "m"
    for bad in (dict(band=4), dict(band=257, ungapped=dict(min_score=0)), dict(band=-1, ungapped=dict(min_score=0))):
        with pytest.raises(ValueError):
            SP.search_proteins([str(db)], [str(qs)], str(out), search=_model_search(seen), **bad)


def test_command_line_parsing_of_the_band_flag(tmp_path, monkeypatch):
    src = tmp_path / "in.faa"
    src.write_bytes(_fasta([b"a"], [b"ACDEFGHIKLMNPQRSTVWY"]))
    got = {}
    monkeypatch.setattr(SP, "search_proteins", lambda *a, **kw: got.update(kw) or "ok")
    base = ["-d", str(src), "-q", str(src), "-o", str(tmp_path / "h.tsv")]
    assert SP.main(base + ["--ungapped"]) == 0 and got["band"] is None
    assert SP.main(base + ["--ungapped", "--band", "32"]) == 0 and got["band"] == 32 and got["ungapped"] == dict(min_score=0)
    assert SP.main(base + ["--ungapped", "--band", "0", "--seeds", "reduced", "--mask", "--paths", "--cigar"]) == 0 and got["band"] == 0
    for bad in (["--band", "8"], ["--ungapped", "--band", "257"], ["--ungapped", "--band", "-1"]):
        with pytest.raises(SystemExit):
            SP.main(base + bad)


def test_the_python_band_arguments():
    from kmergutsjava_amd import hotpath
    none = np.zeros(1, dtype=np.int64)
    with pytest.raises(ValueError):
        hotpath.search_proteins(b"", none, 0, band=8)
    with pytest.raises(ValueError):
        hotpath.align_proteins(b"", none, [], band=8)
    with pytest.raises(ValueError):
        hotpath.align_proteins(b"", none, [], diagonals=[])
