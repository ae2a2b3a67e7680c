"""The masking rule's two model forms against each other and against the header's known answers, the three front ends with an
injected device call, the FASTA writer, and the layouts of the three new structs against gcc.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cluster_model as CM
import mask_model as MM
import search_model as S
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import cluster_proteins as CP
from kmergutsjava_amd import hotpath
from kmergutsjava_amd import mask_proteins as MP
from kmergutsjava_amd import search_proteins as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _equal(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3]


# ---- the rule -------------------------------------------------------------------------------------------------------------------

def test_lg_and_the_three_example_windows():
    assert tuple(MM.lg(k) for k in range(1, 13)) == MM.LG_1_TO_12 == (0, 256, 405, 512, 594, 661, 718, 768, 811, 850, 885, 917)
    assert 12 * MM.lg(12) == MM.FULL_12 == 11004
    assert MM.deficit(b"QEQEQEQEQEQE") == 3072 and MM.deficit(b"ACDEFGHIKLMN") == 11004 and MM.deficit(b"QQQQQQQQQQQQ") == 0
    assert MM.KAT_D == {b"QEQEQEQEQEQE": 3072, b"ACDEFGHIKLMN": 11004, b"QQQQQQQQQQQQ": 0}
    assert 12 * MM.TRIGGER == MM.LOW_MAX_DEFAULT == 6756 and 12 * MM.EXTEND == MM.EXT_MAX_DEFAULT == 7680
    assert (N.MASK_WINDOW, N.MASK_TRIGGER, N.MASK_EXTEND) == (MM.WINDOW, MM.TRIGGER, MM.EXTEND) == (MP.WINDOW, MP.TRIGGER, MP.EXTEND)
    import coding_model
    assert all(MM.lg(x) == coding_model.lg(x) for x in list(range(1, 40)) + [4096, (1 << 63) - 1])
    assert MM.deficit(b"xX*qe\x00\xffBJ-ZO") == 0           # every other byte is the one letter 20


@pytest.mark.parametrize("window,trigger,extend", [(12, 563, 640), (4, 300, 400), (32, 700, 800), (12, 256, 256), (12, 0, 916), (9, 0, 0)])
def test_the_two_forms_agree_on_random_and_planted_inputs(window, trigger, extend):
    rng = np.random.default_rng(window * 1000 + trigger)
    prots = MM.low_complexity_batch(rng, 25) + [b"", b"Q" * (window - 1), b"Q" * window, (b"QE" * 40), MM.INSERT]
    seq, off = S.batch(prots)
    a, b = MM.mask_loops(seq, off, window, trigger, extend), MM.mask_numpy(seq, off, window, trigger, extend)
    assert _equal(a, b)
    assert a[3]["low_windows"] <= a[3]["masking_windows"] <= a[3]["ext_windows"] <= a[3]["windows"]
    assert a[3]["masked_residues"] == int(a[0].sum()) and a[2][-1] == len(a[1]) == a[3]["segments"]


def test_hand_worked_segments():
    """Q * 12 inside 12-distinct-letter flanks: the 11 windows with at least 7 Q are low (D = 5978 at 7), the 13 with at least 6 Q
    ext (7038; 5 Q: 8034 is not), so the masking windows are 24 .. 36 and the masked residues 24 .. 47."""
    hc = MM.ALPHA * 3
    p = hc[20:50] + b"Q" * 12 + hc[:30]            # (the flanks hold one Q each, at distance > 12 from the run)
    f, segs, start, c = MM.mask_loops(*S.batch([p, b"", hc]))
    assert [(s["protein"], s["start"], s["end"]) for s in segs] == [(0, 24, 47)] and list(start) == [0, 1, 1, 1]
    assert c["low_windows"] == 11 and c["ext_windows"] == c["masking_windows"] == 13 and c["masked_residues"] == 24 and c["proteins_masked"] == 1
    assert f[24:48].all() and f.sum() == 24


def test_soft_mask_and_the_masked_models():
    prots, n_db = [b"ACDEFGHIKL" + MM.INSERT + b"MNPQRSTVWY", b"XX" + b"q" * 14, b"ACDEFGHIKLMNPQRSTVWY" * 2], 1
    seq, off = S.batch(prots)
    flags = MM.mask_numpy(seq, off)[0]
    soft = MM.soft_mask(seq, off, flags)
    assert len(soft) == len(seq) and soft[:6] == seq[:6] and soft[10:36] == MM.INSERT.lower() and soft[off[2]:] == seq[off[2]:]
    assert soft[off[1]:off[2]] == b"xx" + b"q" * 14                     # a masked non-letter stays a non-residue
    assert MM.soft_mask(seq, off, flags, 1, 3)[:off[1]] == seq[:off[1]]  # only the side asked for
    assert MM.side_range("queries", 1, 3) == (1, 3) and MM.side_range("targets", 1, 3) == (0, 1) and MM.side_range("both", 1, 3) == (0, 3)


def test_the_planted_search_example_on_the_model():
    """24 targets and 24 queries that all hold the insert QE * 8 + Q * 10: unmasked every query is a candidate of every target (576,
    192 aligned); masked only the 12 related pairs are left, with the scores they had."""
    prots, n_db = MM.planted_search()
    seq, off = S.batch(prots)
    s_of, counts = S.shared_numpy(seq, off, n_db)
    assert len([1 for s in s_of.values() if s >= 2]) == 576
    flags = MM.mask_numpy(seq, off)[0]
    m_of, _ = S.shared_numpy(MM.soft_mask(seq, off, flags), off, n_db)
    assert sorted(k for k, s in m_of.items() if s >= 2) == [(q, q) for q in range(12)]


# ---- the front ends -------------------------------------------------------------------------------------------------------------

FASTA = b">p1 first\nACDEFGHIKLMNPQRSTVWYACDEFGHIKL\nQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQQACDEFGHIKLMNPQRSTVWY\n>p2\nACDEFGHIKLMNPQRSTVWY\n>p3\nXXXXXXXXXXXXXXXX\n"


def _model_mask(seq, offsets, window=12, trigger=563, extend=640, device=0):
    return MM.mask_numpy(seq, offsets, window, trigger, extend)


def test_the_fasta_writer_lowercase_x_and_wrapping(tmp_path):
    src, out, segs = tmp_path / "in.faa", tmp_path / "out.faa", tmp_path / "segs.tsv"
    src.write_bytes(FASTA)
    line = MP.mask_proteins([str(src)], str(out), segments=str(segs), mask=_model_mask)
    text = out.read_bytes().split(b"\n")
    p1 = b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKL" + b"Q" * 40 + b"ACDEFGHIKLMNPQRSTVWY"
    f = MM.mask_numpy(p1, [0, len(p1)])[0]
    want = bytes(ch | 0x20 if on else ch for ch, on in zip(p1, f))
    assert text[0] == b">p1" and text[1] == want[:60] and text[2] == want[60:] and len(text[1]) == 60
    assert text[3:] == [b">p2", b"ACDEFGHIKLMNPQRSTVWY", b">p3", b"x" * 16, b""]      # a masked X is a letter too
    assert b"q" * 30 in want and want.upper() == p1
    a, b = int(np.flatnonzero(f)[0]), int(np.flatnonzero(f)[-1])
    assert segs.read_bytes() == b"p1\t%d\t%d\t%d\np3\t1\t16\t16\n" % (a + 1, b + 1, b - a + 1)
    assert line.startswith("Proteins: 3, residues: 126, masked: %d (%.1f %%), segments: 2, proteins touched: 2, ms: " % (
        int(f.sum()) + 16, 100.0 * (int(f.sum()) + 16) / 126))
    MP.mask_proteins([str(src)], str(out), x=True, mask=_model_mask)
    assert out.read_bytes().split(b"\n")[1] == bytes(ord("X") if on else ch for ch, on in zip(p1, f))[:60]
    assert MP.masked_sequence(b"AC*x", [1, 0, 1, 1]) == b"aC*x" and MP.masked_sequence(b"AC*x", [1, 0, 1, 1], x=True) == b"XCXX"


def test_mask_proteins_passes_its_three_values(tmp_path, capsys):
    src = tmp_path / "in.faa"
    src.write_bytes(FASTA)
    seen = {}

    def fake(seq, offsets, **kw):
        seen.update(kw)
        return _model_mask(seq, offsets, kw["window"], kw["trigger"], kw["extend"])

    MP.mask_proteins([str(src)], str(tmp_path / "o.faa"), window=8, trigger=300, extend=500, mask=fake)
    assert (seen["window"], seen["trigger"], seen["extend"]) == (8, 300, 500)
    assert MP.main(["-p", str(tmp_path / "missing.faa"), "-o", str(tmp_path / "o.faa")]) == 1
    assert "Error:" in capsys.readouterr().err


def _fake_search(seen):
    def search(seq, offsets, n_db, **kw):
        seen.clear()
        seen.update(kw)
        n_q = len(offsets) - 1 - n_db
        st = dict(queries=n_q, targets=n_db, candidates=0, aligned=0, hits=0, queries_hit=0, kmers_masked=0)
        if "mask" in kw:
            st["mask"] = dict(masked_residues=41)
        return np.zeros(0, dtype=N.SEARCH_HIT_DTYPE), np.zeros(n_q + 1, dtype=np.int64), st
    return search


def test_search_proteins_mask_option_and_summary(tmp_path):
    src = tmp_path / "in.faa"
    src.write_bytes(FASTA)
    seen = {}
    plain = SP.search_proteins([str(src)], [str(src)], str(tmp_path / "h.tsv"), search=_fake_search(seen))
    assert "mask" not in seen and ", mask:" not in plain
    line = SP.search_proteins([str(src)], [str(src)], str(tmp_path / "h.tsv"), search=_fake_search(seen),
                              mask=dict(window=12, trigger=563, extend=640, sides="queries"))
    assert seen["mask"] == dict(window=12, trigger=563, extend=640, sides="queries")
    assert line == plain + ", mask: 12/563/640 queries, masked residues: 41"
    with pytest.raises(ValueError):
        SP.search_proteins([str(src)], [str(src)], str(tmp_path / "h.tsv"), search=_fake_search(seen), mask=dict(sides="left"))


def test_cluster_proteins_mask_option_and_summary(tmp_path):
    src = tmp_path / "in.faa"
    src.write_bytes(FASTA)
    seen = {}

    def cluster(seq, offsets, **kw):
        seen.clear()
        seen.update(kw)
        rec, counts = CM.cluster_numpy(seq, offsets)
        st = dict(counts, rounds=0)
        if "mask" in kw:
            st["mask"] = dict(masked_residues=7)
        return rec, st

    plain = CP.cluster_proteins([str(src)], str(tmp_path / "f.tsv"), cluster=cluster)
    assert "mask" not in seen
    line = CP.cluster_proteins([str(src)], str(tmp_path / "f.tsv"), cluster=cluster, mask=dict(window=10, trigger=500, extend=600))
    assert seen["mask"] == dict(window=10, trigger=500, extend=600) and line == plain + ", mask: 10/500/600, masked residues: 7"


def test_command_line_parsing_of_the_mask_flags(tmp_path, monkeypatch):
    src = tmp_path / "in.faa"
    src.write_bytes(FASTA)
    got = {}
    monkeypatch.setattr(SP, "search_proteins", lambda *a, **kw: got.update(kw) or "ok")
    base = ["-d", str(src), "-q", str(src), "-o", str(tmp_path / "h.tsv")]
    assert SP.main(base) == 0 and got["mask"] is None
    assert SP.main(base + ["--mask"]) == 0 and got["mask"] == dict(window=12, trigger=563, extend=640, sides="both")
    assert SP.main(base + ["--mask", "targets", "--mask-window", "16", "--mask-extend", "700"]) == 0
    assert got["mask"] == dict(window=16, trigger=563, extend=700, sides="targets")
    for bad in (["--mask", "left"], ["--mask-trigger", "5"]):
        with pytest.raises(SystemExit):
            SP.main(base + bad)
    monkeypatch.setattr(CP, "cluster_proteins", lambda *a, **kw: got.update(kw) or "ok")
    base = ["-p", str(src), "-o", str(tmp_path / "f.tsv")]
    assert CP.main(base) == 0 and got["mask"] is None
    assert CP.main(base + ["--mask", "--mask-trigger", "500"]) == 0 and got["mask"] == dict(window=12, trigger=500, extend=640)
    with pytest.raises(SystemExit):
        CP.main(base + ["--mask-window", "9"])


def test_the_python_mask_argument():
    assert hotpath._mask_params(None) is None and hotpath._mask_params(False) is None
    p, sides = hotpath._mask_params(True)
    assert (p.window, p.trigger, p.extend, p.reserved, sides) == (12, 563, 640, 0, 3)
    p, sides = hotpath._mask_params(dict(window=20, sides="targets"), sides_too=True)
    assert (p.window, p.trigger, p.extend, sides) == (20, 563, 640, N.MASK_TARGETS)
    assert hotpath._mask_params(dict(sides="queries"), sides_too=True)[1] == N.MASK_QUERIES
    for bad, kw in ((dict(sides="queries"), {}), (dict(width=3), {}), (dict(sides="left"), dict(sides_too=True))):
        with pytest.raises(ValueError):
            hotpath._mask_params(bad, **kw)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,binding", [("kg_mask_params", N.KgMaskParams), ("kg_mask_segment", N.KgMaskSegment),
                                           ("kg_mask_stats", N.KgMaskStats)])
def test_the_bindings_match_the_c_structs(cname, binding, tmp_path):
    """Every field of the ctypes structures sits where gcc puts it for include/kmerguts_hip.h."""
    fields = [f for f, _ in binding._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%%zu\\n", sizeof(%s));\n' % cname +
                   "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(binding) == {"kg_mask_params": 16, "kg_mask_segment": 16, "kg_mask_stats": 80}[cname]
    assert out[1:] == [getattr(binding, f).offset for f in fields]
    if cname == "kg_mask_segment":
        assert N.MASK_SEGMENT_DTYPE.itemsize == 16 and list(N.MASK_SEGMENT_DTYPE.names) == fields


def test_exports_and_documents():
    assert {"kg_proteins_mask", "kg_proteins_mask_device", "kg_maskset_count", "kg_maskset_copy", "kg_maskset_starts_copy",
            "kg_maskset_flags_copy", "kg_maskset_stats", "kg_maskset_free", "kg_proteins_search_masked",
            "kg_proteins_search_masked_device", "kg_hitset_mask_stats", "kg_proteins_cluster_masked",
            "kg_proteins_cluster_masked_device", "kg_familyset_mask_stats"} <= set(N.EXPORTS)
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "kg_proteins_mask" in text or "mask_proteins" in text, name
    import re
    dev = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_device.hpp")).read()
    krn = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_mask.hpp")).read()
    assert int(re.search(r"constexpr int kAaWinPerBlock = (\d+);", dev).group(1)) == N.MASK_TILE == 64
    assert int(re.search(r"constexpr int kMaskMaxWindow = (\d+);", krn).group(1)) == 32
    hdr = open(os.path.join(ROOT, "include", "kmerguts_hip.h")).read()
    assert "#define KG_MASK_QUERIES 1" in hdr and "#define KG_MASK_TARGETS 2" in hdr and "11004" in hdr
