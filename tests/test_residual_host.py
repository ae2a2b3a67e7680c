"""The rule of kg_contigs_search_residual on the host: residual_model's explain_of and merge_of against answers known by hand, the
new structures against gcc, the argument checks of hotpath's wrapper and of the C entry points without a GPU, and call_regions
--fill-db with the models in the device's place (the name map, the evidence field, the summary, the batch cuts, the flag errors)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import regions_model as R
import residual_model as RM
import test_repair_frontend as RF
import translated_model as TM
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import call_regions as CR
from kmergutsjava_amd import hotpath as H
from kmergutsjava_amd import synth
from kmergutsjava_amd.make_search_db import pack_names
from test_translated_host import _contig, _frameshift_case, _protein

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _calls(rows):
    out = np.zeros(len(rows), dtype=N.CALL_DTYPE)
    for k, (container, start, end, count, fi) in enumerate(rows):
        out[k] = (container, start, end, count, fi, np.float32(count))
    return out


def _frag(seq, strand, frame, left, right, n_res):
    f = np.zeros(1, dtype=N.ORF_DTYPE)
    f[0]["seq"], f[0]["strand"], f[0]["frame"], f[0]["left"], f[0]["right"], f[0]["n_res"] = seq, strand, frame, left, right, n_res
    return f


# ---- explain_of: the touch rule at a fragment's two ends, both strands, the three frames, L mod 3 ---------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("frame", [0, 1, 2])
@pytest.mark.parametrize("L", [300, 301, 302])
def test_a_call_touches_a_fragment_from_its_first_codon_to_its_last(strand, frame, L):
    b, n_res = 10, 20                                   # the fragment covers codons 10 .. 29 of its container
    x, y = frame + 3 * b, frame + 3 * (b + n_res) - 1   # its nucleotides on its own strand
    left, right = (x, y) if strand == 0 else (L - 1 - y, L - 1 - x)
    f = _frag(0, strand, frame, left, right, n_res)
    off = [0, L]
    assert TM.first_codon(f[0], L) == b
    c = 3 * strand + frame
    for start, end, touches in ((3, 10, True), (3, 9, False), (29, 40, True), (30, 40, False), (12, 14, True), (0, 90, True), (10, 10, True)):
        assert RM.explain_of(f, off, _calls([(c, start, end, 7, 0)])).tolist() == [7 if touches else 0], (start, end)
    # another container of the same contig, or the same codons of another contig's container, touch nothing
    assert RM.explain_of(f, off, _calls([((c + 1) % 6, 10, 29, 7, 0)])).tolist() == [0]
    assert RM.explain_of(f, [0, L, 2 * L], _calls([(6 + c, 10, 29, 7, 0)])).tolist() == [0]


def test_a_call_across_a_stop_explains_both_fragments_and_counts_add_up():
    frags = np.concatenate([_frag(0, 0, 0, 0, 59, 20), _frag(0, 0, 0, 63, 122, 20), _frag(0, 0, 1, 1, 60, 20)])     # codons 0..19, 21..40
    off = [0, 200]
    ex = RM.explain_of(frags, off, _calls([(0, 15, 25, 5, 0), (0, 30, 33, 2, 1), (0, 20, 20, 9, 1)]))
    assert ex.tolist() == [5, 7, 0] and ex.dtype == np.int64          # the third CALL lies on the stop codon: in no fragment
    # explain == explain_min - 1 is searched, == explain_min is explained
    for explain_min, searched in ((5, [2]), (6, [0, 2]), (7, [0, 2]), (8, [0, 1, 2])):
        assert RM.subset_of(frags, np.array([0, 20, 40, 60]), np.arange(60, dtype=np.uint8), ex, explain_min)[0].tolist() == searched
    s, recs, start, res = RM.subset_of(frags, np.array([0, 20, 40, 60]), np.arange(60, dtype=np.uint8), ex, 6)
    assert start.tolist() == [0, 20, 40] and res.tolist() == list(range(20)) + list(range(40, 60)) and recs.tobytes() == frags[[0, 2]].tobytes()


def test_a_call_in_a_run_shorter_than_min_res_explains_nothing():
    """A gene of 40 residues with a stop 12 codons in front of it: at min_res 30 the short run is no fragment, and a CALL inside it
    changes no explain; at min_res 1 it is one, and the CALL explains it alone."""
    rng = np.random.default_rng(4)
    gene = _protein(rng, 40)
    dna = "TAA" + synth.back_translate(_protein(rng, 12)) + "TAA" + synth.back_translate(gene) + "TAA" + "A" * 30
    off = [0, len(dna)]
    sig = _calls([(0, 2, 9, 6, 0)])
    for min_res, want in ((30, 0), (1, 1)):
        m = RM.residual_model(dna.encode(), off, gene.encode(), [0, 40], sig, [0], min_res=min_res)
        assert int((m["explain"] > 0).sum()) == want
        assert len(m["searched"]) == len(m["fragments"][0]) - want
        assert m["call_kind"].tolist().count(1) == 1 and m["calls"][0].tobytes() == sig[0].tobytes()


# ---- merge_of -----------------------------------------------------------------------------------------------------------------------------

def test_the_merge_by_container_with_every_mix_and_the_cut():
    # containers 0 (sig only), 2 (db only), 3 (both), 4 (neither), 11 the last (both); db CALL 1 is below the cut
    sig = _calls([(0, 1, 2, 5, 0), (0, 0, 1, 6, 1), (3, 4, 5, 7, 2), (11, 1, 1, 8, 3)])
    db = _calls([(2, 0, 9, 50, 4), (3, 0, 9, 19, 5), (3, 10, 19, 60, 6), (11, 0, 0, 70, 7), (11, 5, 6, 20, 8)])
    hits = np.array([0, 2, 3, 7, 9], dtype=np.int64)
    merged, kind, source, hit, dropped = RM.merge_of(sig, db, hits, 20)
    assert merged["fI"].tolist() == [0, 1, 4, 2, 6, 3, 7, 8] and dropped == 1
    assert kind.tolist() == [0, 0, 1, 0, 1, 0, 1, 1] and kind.dtype == np.uint8
    assert source.tolist() == [0, 1, 0, 2, 2, 3, 3, 4] and hit.tolist() == [-1, -1, 0, -1, 3, -1, 7, 9]
    assert (np.diff(merged["container"].astype(np.int64)) >= 0).all()
    # only one kind, and none
    m, k, s, h, d = RM.merge_of(sig, db[:0], hits[:0], 0)
    assert m.tobytes() == sig.tobytes() and k.tolist() == [0] * 4 and s.tolist() == [0, 1, 2, 3] and h.tolist() == [-1] * 4 and d == 0
    m, k, s, h, d = RM.merge_of(sig[:0], db, hits, 0)
    assert m.tobytes() == db.tobytes() and k.tolist() == [1] * 5 and s.tolist() == [0, 1, 2, 3, 4] and h.tolist() == hits.tolist()
    m, k, s, h, d = RM.merge_of(sig[:0], db, hits, 1000)
    assert len(m) == 0 and d == 5 and m.dtype == N.CALL_DTYPE and h.dtype == np.int64


# ---- the point of it: one half named by the table, the other by the database -----------------------------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
def test_a_frameshifted_gene_with_one_half_from_each_source_is_one_region(strand):
    gene, contig = _frameshift_case(strand)
    off = [0, len(contig)]
    alone = TM.translated_model(contig, off, gene.encode(), [0, 80], ref="query", min_ratio_pct=20, target_fn=[3])
    assert len(alone["calls"]) == 2
    first = alone["calls"][:1].copy()
    first["count"] = 9                                                  # the first half as a table names it: k-mer hits
    m = RM.residual_model(contig, off, gene.encode(), [0, 80], first, [3], ref="query", min_ratio_pct=20)
    assert len(m["searched"]) == len(m["fragments"][0]) - 1 and int(m["explain"].sum()) == 9
    assert m["call_kind"].tolist() == [0, 1] and m["calls"][1].tobytes() == alone["calls"][1].tobytes()
    assert m["hits"]["query"].max() < len(m["searched"])
    regs, _ = R.regions(m["calls"], off)
    assert len(regs) == 1 and int(regs[0]["frames"]) == 0b101 and int(regs[0]["score"]) == 9 + int(alone["calls"][1]["count"])
    assert RM.evidence_of(regs, m["calls"], m["call_kind"], off) == ["table+db"]
    assert CR.region_evidence(regs, m["calls"], m["call_kind"], np.asarray(off)) == [b"table+db"]


# ---- the ABI, the bindings and the wrappers' argument checks ---------------------------------------------------------------------------

@pytest.mark.parametrize("cname,cls,size", [("kg_residual_params", "KgResidualParams", 16), ("kg_residual_stats", "KgResidualStats", 80)])
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
    new = [n for n in N.EXPORTS if n.startswith("kg_residual_")] + ["kg_contigs_search_residual", "kg_result_search_residual"]
    assert len(new) == 8 and all(hasattr(lib, n) for n in new)
    none = (None, None, None, None, None, 0, None, 0, 0, 0, 0, 0, None, None, None, None)
    rp = N.KgResidualParams(1, 0, 0)
    assert lib.kg_contigs_search_residual(*none, None, 0, 0, C.byref(rp), None) == N.KG_ERR_ARG and lib.kg_last_error().decode() == "null argument"
    assert lib.kg_contigs_search_residual(*none, None, 0, 0, C.byref(rp), C.byref(h)) == N.KG_ERR_ARG
    assert lib.kg_last_error().decode() == "null kg_searchdb"
    assert lib.kg_result_search_residual(None, *none, C.byref(rp), None) == N.KG_ERR_ARG and lib.kg_last_error().decode() == "null argument"
    assert lib.kg_result_search_residual(None, *none, C.byref(rp), C.byref(h)) == N.KG_ERR_ARG and lib.kg_last_error().decode() == "null kg_result"
    st = N.KgResidualStats()
    assert lib.kg_residual_stats_of(None, C.byref(st)) == N.KG_ERR_ARG and lib.kg_last_error().decode() == "null argument"
    for name in ("kg_residual_searched_copy", "kg_residual_explain_copy", "kg_residual_call_kinds_copy", "kg_residual_call_sources_copy"):
        assert getattr(lib, name)(None, 0, 0, None) == N.KG_ERR_ARG
    assert not lib.kg_residual_searched_fragments(None) and not h.value


class _LibraryUsed(Exception):
    pass


class _NoLibrary:
    def __getattr__(self, name):
        raise _LibraryUsed(name)


@pytest.mark.parametrize("kw,text", [
    (dict(explained_by=np.zeros(0, dtype=N.CALL_DTYPE)), "explained_by needs target_fn: the two kinds of CALL share one function index space"),
    (dict(explain_min=2), "explain_min and min_db_count need explained_by"),
    (dict(min_db_count=1), "explain_min and min_db_count need explained_by"),
    (dict(explained_by=np.zeros(0, dtype=N.CALL_DTYPE), target_fn=[0], explain_min=0), "explain_min must be >= 1"),
    (dict(explained_by=np.zeros(0, dtype=N.CALL_DTYPE), target_fn=[0], min_db_count=-1), "min_db_count must be >= 0"),
])
def test_search_contigs_checks_the_new_arguments_before_the_library(monkeypatch, kw, text):
    monkeypatch.setattr(N, "load", lambda: _NoLibrary())
    with pytest.raises(ValueError) as e:
        H.SearchDb(C.c_void_p(1)).search_contigs(b"ACGT", [0, 4], **kw)
    assert str(e.value) == text


# ---- call_regions --fill-db with the models in the device's place -----------------------------------------------------------------------------

class _ModelTable:
    """What call_regions scans: planted signature CALLs per contig id, handed out as test_repair_frontend's stand-in."""

    def __init__(self, planted, ids):
        self.planted, self.ids, self.at, self.batches = planted, ids, 0, []

    def __call__(self, path, device):
        self.at = 0
        return self

    def scan(self, batch, off, params):
        n = len(off) - 1
        rows = []
        for k in range(n):
            for frame_c, start, end, count, fi in self.planted.get(self.ids[self.at + k], ()):
                rows.append((6 * k + frame_c, start, end, count, fi))
        self.at += n
        self.batches.append(n)
        return RF._ModelScan(_calls(rows), batch, np.asarray(off, dtype=np.int64))


class _ModelDb:
    """hotpath.SearchDb as call_regions --fill-db uses it, over residual_model."""

    def __init__(self, prots, functions, room):
        self.tseq = "".join(prots).encode()
        self.toff = np.concatenate([[0], np.cumsum([len(p) for p in prots])]).astype(np.int64)
        self.blob = pack_names([b"t%d" % k for k in range(len(prots))], functions)
        self.room, self.reserved, self.batches, self.target_fn = room, [], [], None

    def __call__(self, path, device=0):
        return self

    def info(self):
        return {"targets": len(self.toff) - 1, "query_room": self.room}

    def names(self):
        return self.blob

    def reserve(self, room):
        self.reserved.append(room)
        self.room = max(self.room, room)

    def close(self):
        pass

    def search_contigs(self, batch, off, min_res=30, max_hits=1, target_fn=None, explained_by=None, explain_min=1, min_db_count=0, **kw):
        assert 2 * len(batch) <= self.room and explained_by is not None
        self.batches.append(len(off) - 1)
        self.target_fn = np.asarray(target_fn)
        kw.update(kw.pop("align", None) or {})
        m = RM.residual_model(batch, off, self.tseq, self.toff, explained_by.calls, target_fn, min_res, max_hits, explain_min, min_db_count, **kw)
        ev = RF._ModelScan(m["calls"], batch, np.asarray(off, dtype=np.int64))
        ev.calls, ev.call_hits, ev.call_kind, ev.call_source = m["calls"], m["call_hits"], m["call_kind"], m["call_source"]
        ev.fragments, ev.searched_fragments = m["fragments"], m["searched_fragments"]
        ev.search = (m["hits"], m["hit_start"], m["paths"], {"hits": int((m["hits"]["status"] == 0).sum())})
        ev.stats = dict(fragments=len(m["fragments"][0]), calls=len(m["db_calls"]))
        n_q = len(m["searched"])
        ev.residual_stats = dict(explained=len(m["fragments"][0]) - n_q, searched=n_q, db_calls=len(m["db_calls"]),
                                 dropped_min_count=m["dropped_min_count"])
        return ev


def _fill_case(tmp_path):
    """Four contigs: c0 a gene the table names whole (the database holds it too, under the table's name), c1 a gene only the
    database knows (a new function name), c2 one of a target without a function, c3 the frameshifted gene whose first half the
    table names and whose second half is left to the database, both under `ligase`."""
    rng = np.random.default_rng(12)
    gene, shifted = _frameshift_case(0)
    prots = [_protein(rng, 40), _protein(rng, 55), _protein(rng, 45), gene]
    functions = {b"t0": (b"kinase", None), b"t1": (b"lyase", None), b"t3": (b"ligase", None)}
    contigs = [_contig(synth.back_translate(prots[0]), 30, 33, 0), _contig(synth.back_translate(prots[1]), 31, 34, 1),
               _contig(synth.back_translate(prots[2]), 32, 35, 1), shifted]
    d = tmp_path / "data"
    d.mkdir()
    (d / "kmer.table.mem_map").write_bytes(b"")
    (d / "function.index").write_text("0\thypothetical\n1\tkinase\n2\tligase\n3\tkinase\n")
    q = tmp_path / "c.fna"
    q.write_text("".join(">c%d\n%s\n" % (k, c.decode()) for k, c in enumerate(contigs)))
    half = TM.translated_model(shifted, [0, len(shifted)], gene.encode(), [0, 80], ref="query", min_ratio_pct=20)["calls"][0]
    planted = {b"c0": [(0, 11, 11 + 39, 12, 1)],                                   # container 0 = '+' frame 0: lead 30, stop, the gene
               b"c3": [(int(half["container"]), int(half["start"]), int(half["end"]), 9, 2)]}
    return prots, functions, contigs, planted, str(d), str(q)


def _fill_run(tmp_path, tag, case, **kw):
    prots, functions, contigs, planted, d, q = case
    table, db = _ModelTable(planted, [b"c%d" % k for k in range(4)]), _ModelDb(prots, functions, kw.pop("room", 1 << 20))
    names = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in ("tsv", "orfs", "faa", "shifts", "hits")}
    line = CR.call_regions(d, q, names["tsv"], orfs_out=names["orfs"], faa_out=names["faa"], repair=True, shifts_out=names["shifts"],
                           hits_out=names["hits"], fill_db="model.kgsdb", open_db=db, open_table=table,
                           search=dict(align=dict(ref="query", min_ratio_pct=20)), **kw)
    return line, {k: open(p, "rb").read() for k, p in names.items()}, table, db


def test_fill_function_names_keep_the_table_s_indices():
    fnames, fn = CR.fill_function_names([b"hypothetical", b"kinase", b"ligase", b"kinase"], [b"t0", b"t1", b"t2", b"t3"],
                                        {b"t0": (b"kinase", None), b"t1": (b"lyase", None), b"t3": (b"ligase", None)})
    assert fnames == [b"hypothetical", b"kinase", b"ligase", b"kinase", b"lyase", b"t2"]       # the table's list, then first appearances
    assert fn.tolist() == [1, 4, 5, 2] and fn.dtype == np.int32                                # same name: the table's first index
    fnames, fn = CR.fill_function_names([b"a"], [b"x", b"a"], None)
    assert fnames == [b"a", b"x"] and fn.tolist() == [1, 0]


def test_the_names_the_evidence_field_the_hits_and_the_summary_of_a_fill_run(tmp_path):
    case = _fill_case(tmp_path)
    line, out, table, db = _fill_run(tmp_path, "one", case)
    rows = [ln.split(b"\t") for ln in out["tsv"].splitlines()]
    assert [r[0] for r in rows] == [b"c0", b"c1", b"c2", b"c3"]
    assert [r[4] for r in rows] == [b"kinase", b"lyase", b"t2", b"ligase"]
    assert [r[-1] for r in rows] == [b"table", b"db", b"db", b"table+db"] and all(len(r) == 11 for r in rows)
    assert rows[3][8] == b"0,2" and db.target_fn.tolist() == [1, 4, 5, 2]
    assert "Contigs: 4, with calls: 4, regions: 4, kept: 4, multi-frame: 1" in line and ", repaired: 1, unrepaired: 0" in line
    tail = line[line.index(", fill: index"):]
    assert tail.startswith(", fill: index (4 targets), fragments: ") and ", explained: 2, searched: " in tail
    assert tail.endswith(", translated hits: 3, db calls: 3")
    hits = [ln.split(b"\t") for ln in out["hits"].splitlines()]
    assert [h[0] for h in hits] == [b"c1", b"c2", b"c3"] and [h[7] for h in hits] == [b"t1", b"t2", b"t3"]
    assert [h[15] for h in hits] == [b"lyase", b"-", b"ligase"] and all(h[1:4] == r[1:4] for h, r in zip(hits[:2], rows[1:3]))
    gene = case[0][3]
    faa = out["faa"].replace(b"\n", b"")                              # (the FASTA wraps its lines)
    assert gene[1:30].encode() in faa and gene[-30:].encode() in faa
    # GFF: the attribute, in front of what the selection adds
    prots, functions, contigs, planted, d, q = case
    gff = str(tmp_path / "g.gff")
    CR.call_regions(d, q, gff, gff=True, fill_db="m", open_db=_ModelDb(prots, functions, 1 << 20),
                    open_table=_ModelTable(planted, [b"c%d" % k for k in range(4)]), search=dict(align=dict(ref="query", min_ratio_pct=20)))
    attrs = [ln.split(b"\t")[8] for ln in open(gff, "rb").read().splitlines()[1:]]
    assert [a.split(b";")[-1] for a in attrs] == [b"evidence=table", b"evidence=db", b"evidence=db", b"evidence=table+db"]
    # a cut that drops every homology CALL leaves the table's regions, all `table`
    line2, out2, _, _ = _fill_run(tmp_path, "cut", case, fill_min_score=10 ** 6)
    rows2 = [ln.split(b"\t") for ln in out2["tsv"].splitlines()]
    assert [r[0] for r in rows2] == [b"c0", b"c3"] and [r[-1] for r in rows2] == [b"table", b"table"] and line2.endswith(", db calls: 0")
    assert out2["hits"] == b""


def test_no_output_byte_depends_on_the_batch_cuts_and_the_room_is_reserved(tmp_path):
    case = _fill_case(tmp_path)
    line, one, _, _ = _fill_run(tmp_path, "whole", case)
    for n, batches in ((1, [1, 1, 1, 1]), (500, [2, 1, 1]), (10 ** 6, [4])):
        cut_line, cut, table, db = _fill_run(tmp_path, "cut%d" % n, case, batch_nt=n)
        assert cut == one and cut_line == line and db.batches == batches == table.batches
    small_line, got, _, small = _fill_run(tmp_path, "small", case, room=400)
    assert got == one and small_line == line and small.batches == [1, 1, 1, 1]
    room, want = 400, []
    for c in case[2]:
        if 2 * len(c) > room:
            room = 2 * len(c)
            want.append(room)
    assert small.reserved == want and len(want) >= 1


def test_the_new_flag_errors_by_their_words(tmp_path, capsys):
    base = ["-q", "x.fna", "-o", str(tmp_path / "o.tsv")]
    for argv, text in ((["-D", "x", "--db", "y"], "give -D or --db, not both"),
                       (["--db", "y", "--fill-db", "z"], "--fill-db beside --db"),
                       (["--fill-db", "z"], "--fill-db needs -D"),
                       (["-D", "x", "--min-frag", "20"], "--min-frag needs --db"),
                       (["-D", "x", "--explain-min", "2"], "--explain-min and --fill-min-score need --fill-db"),
                       (["-D", "x", "--fill-min-score", "2"], "--explain-min and --fill-min-score need --fill-db"),
                       (["-D", "x", "--fill-db", "z", "--explain-min", "0"], "--explain-min must be >= 1"),
                       (["-D", "x", "--fill-db", "z", "--fill-min-score", "-1"], "--fill-min-score must be >= 0"),
                       (["-D", "x", "--fill-db", "z", "--min-frag", "0"], "--min-frag must be >= 1"),
                       (["-D", "x", "--fill-db", "z", "--band", "8"], "--band needs --ungapped")):
        with pytest.raises(SystemExit):
            CR.main(argv + base)
        assert text in capsys.readouterr().err, argv
    for kw, text in ((dict(db="y", fill_db="z", data_dir=None), "--fill-db beside --db"), (dict(fill_db="z", data_dir=None), "--fill-db needs -D"),
                     (dict(explain_min=2), "--explain-min and --fill-min-score need --fill-db"),
                     (dict(hits_out="h"), "--hits needs --db")):
        kw = dict(kw)
        d = kw.pop("data_dir", "x")
        with pytest.raises(ValueError) as e:
            CR.call_regions(d, "x.fna", "o.tsv", **kw)
        assert text in str(e.value)
