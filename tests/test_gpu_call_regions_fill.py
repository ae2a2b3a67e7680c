"""call_regions -D ... --fill-db ... end to end on the GPU: make_signatures writes a table of some of the proteins, make_search_db an
index of all of them, and one run names the planted genes from both: the regions lie at the planted coordinates, the `evidence`
field says where each came from, --hits holds the homology CALLs, the frameshifted gene whose halves come from the two sources
is joined by --repair, no byte depends on the batch cuts, and the regions the table names are those of a plain -D run."""
import contextlib
import importlib
import io
from types import SimpleNamespace

import numpy as np
import pytest

from kmergutsjava_amd import synth
from test_translated_host import _contig, _frameshift_case, _protein

pytestmark = pytest.mark.gpu


def _run(mod, *args):
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            rc = importlib.import_module("kmergutsjava_amd." + mod).main([str(a) for a in args])
        except SystemExit as e:
            rc = e.code
    return SimpleNamespace(returncode=rc, stdout=out.getvalue(), stderr=err.getvalue())


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """Five proteins.  The table is made from t0 (`kinase`) and the first 42 residues of the frameshifted gene t4 (`ligase`): its
    first half.  The index holds all five: t0 `kinase` again, t1 `kinase`, t2 `pump` (a name the table does not have), t3 without a
    function, t4 `ligase`.  Contigs c0..c3 hold t0..t3, c4 the frameshifted gene."""
    d = tmp_path_factory.mktemp("fill")
    rng = np.random.default_rng(12)
    gene, shifted = _frameshift_case(1)
    prots = [_protein(rng, 40), _protein(rng, 55), _protein(rng, 70), _protein(rng, 45), gene]
    (d / "known.faa").write_text(">k0\n%s\n>k4\n%s\n" % (prots[0], gene[:42]))
    (d / "known.tsv").write_text("k0\tkinase\tO1\nk4\tligase\tO1\n")
    got = _run("make_signatures", "-p", d / "known.faa", "-A", d / "known.tsv", "-o", d / "sigs.txt", "-D", d / "data", "--min-proteins", "1")
    assert got.returncode == 0, got.stderr
    (d / "t.faa").write_text("".join(">t%d\n%s\n" % (k, p) for k, p in enumerate(prots)))
    (d / "t.tsv").write_text("t0\tkinase\nt1\tkinase\nt2\tpump\nt4\tligase\n")
    got = _run("make_search_db", "-d", d / "t.faa", "-A", d / "t.tsv", "-o", d / "t.kgsdb")
    assert got.returncode == 0, got.stderr
    plan = [(0, 30, 33, 0), (1, 31, 34, 1), (2, 32, 35, 0), (3, 30, 34, 1)]         # target, lead, tail, strand
    contigs = [_contig(synth.back_translate(prots[t]), lead, tail, strand) for t, lead, tail, strand in plan] + [shifted]
    (d / "c.fna").write_text("".join(">c%d\n%s\n" % (k, c.decode()) for k, c in enumerate(contigs)))
    return d, prots, plan, contigs


def _outputs(d, tag, *more):
    names = {k: d / ("%s.%s" % (tag, k)) for k in ("tsv", "orfs", "faa", "shifts", "hits")}
    got = _run("call_regions", "-D", d / "data", "--fill-db", d / "t.kgsdb", "-q", d / "c.fna", "-o", names["tsv"], "--orfs", names["orfs"],
               "--faa", names["faa"], "--repair", "--shifts", names["shifts"], "--hits", names["hits"], "--min-ratio", "20", *more)
    assert got.returncode == 0, got.stderr
    return got.stdout.strip(), {k: p.read_bytes() for k, p in names.items()}


def test_coordinates_names_and_the_evidence_field(planted):
    d, prots, plan, contigs = planted
    line, out = _outputs(d, "one")
    rows = [ln.split("\t") for ln in out["tsv"].decode().splitlines()]
    assert [r[0] for r in rows] == ["c%d" % k for k in range(5)]
    assert [r[4] for r in rows] == ["kinase", "kinase", "pump", "t3", "ligase"]
    assert [r[10] for r in rows] == ["table", "db", "db", "db", "table+db"] and all(len(r) == 11 and r[9] == "kept" for r in rows)
    for r, (t, lead, tail, strand), c in zip(rows[1:4], plan[1:], contigs[1:]):      # the database's: the whole gene
        L, n = len(c), 3 * len(prots[t])
        want = (lead + 3 + 1, lead + 3 + n) if strand == 0 else (L - (lead + 3 + n) + 1, L - (lead + 3))
        assert (int(r[1]), int(r[2]), r[3], r[8]) == (want[0], want[1], "+-"[strand], str(lead % 3)), r
    # the table's: from the gene's first codon to its last signature 8-mer, which a protein's last windows need not be (what a plain
    # -D run gives is compared below)
    t, lead, tail, strand = plan[0]
    end = lead + 3 + 3 * len(prots[0])
    assert (int(rows[0][1]), rows[0][3], rows[0][8]) == (lead + 4, "+", str(lead % 3)) and end - 3 * 8 <= int(rows[0][2]) <= end
    assert rows[4][3] == "-" and rows[4][8] == "0,2" and int(rows[4][7]) >= 2
    tail_words = line[line.index(", fill: index"):]
    assert tail_words.startswith(", fill: index (5 targets), fragments: ") and ", explained: 2, searched: " in tail_words
    assert tail_words.endswith(", translated hits: 4, db calls: 4")
    assert "Contigs: 5, with calls: 5, regions: 5, kept: 5, multi-frame: 1" in line and ", repaired: 1, unrepaired: 0" in line
    # --hits: the homology CALLs that were merged
    hits = [ln.split("\t") for ln in out["hits"].decode().splitlines()]
    assert [h[0] for h in hits] == ["c1", "c2", "c3", "c4"] and [h[7] for h in hits] == ["t1", "t2", "t3", "t4"]
    assert [h[15] for h in hits] == ["kinase", "pump", "-", "ligase"] and all(h[1:4] == r[1:4] for h, r in zip(hits[:3], rows[1:4]))
    # --repair --faa: the joined protein holds both ends of the gene
    faa = out["faa"].decode().split(">")[1:]
    seqs = ["".join(x.splitlines()[1:]) for x in faa]
    assert len(seqs) == 5 and prots[4][1:30] in seqs[4] and prots[4][-30:] in seqs[4]
    assert len(out["shifts"].splitlines()) == 1 and out["shifts"].split(b"\t")[4] == b"ligase"
    # GFF: the attribute
    got = _run("call_regions", "-D", d / "data", "--fill-db", d / "t.kgsdb", "-q", d / "c.fna", "-o", d / "g.gff", "--gff", "--min-ratio", "20")
    assert got.returncode == 0, got.stderr
    attrs = [ln.split("\t")[8] for ln in (d / "g.gff").read_text().splitlines()[1:]]
    assert [a.split(";")[-1] for a in attrs] == ["evidence=table", "evidence=db", "evidence=db", "evidence=db", "evidence=table+db"]


def test_no_byte_depends_on_the_batch_cuts(planted):
    d, prots, plan, contigs = planted
    line, one = _outputs(d, "whole")
    for n in (1, 250, 400):
        cut_line, cut = _outputs(d, "cut%d" % n, "--batch-nt", n)
        assert cut == one and cut_line == line
    _, sel = _outputs(d, "sel", "--select", "--free-orfs", "--min-res", "30")
    _, sel_cut = _outputs(d, "selcut", "--select", "--free-orfs", "--min-res", "30", "--batch-nt", 1)
    assert sel == sel_cut and sel["tsv"] == one["tsv"]


def test_the_table_s_regions_are_those_of_a_plain_run_and_the_parameters_cut(planted):
    d, prots, plan, contigs = planted
    _, fill = _outputs(d, "fill")
    got = _run("call_regions", "-D", d / "data", "-q", d / "c.fna", "-o", d / "plain.tsv")
    assert got.returncode == 0, got.stderr
    plain = (d / "plain.tsv").read_bytes().splitlines()
    table_only = [ln.rsplit(b"\t", 1)[0] for ln in fill["tsv"].splitlines() if ln.endswith(b"\ttable")]
    assert len(plain) == 2 and table_only == plain[:1] and plain[1].split(b"\t")[0] == b"c4"
    # a score no homology CALL reaches: the table's regions alone, both `table`; --hits is empty
    line, cut = _outputs(d, "cut", "--fill-min-score", 100000)
    assert [ln.rsplit(b"\t", 1)[0] for ln in cut["tsv"].splitlines()] == plain and cut["hits"] == b"" and line.endswith(", db calls: 0")
    # an --explain-min no CALL reaches: every fragment is searched, and the genes the table names are named twice over
    line, all_ = _outputs(d, "all", "--explain-min", 100000)
    assert ", explained: 0, " in line and [ln.split(b"\t")[10] for ln in all_["tsv"].splitlines()] == [b"table+db", b"db", b"db", b"db", b"table+db"]


@pytest.mark.parametrize("args,word", [
    (("--db", "y", "--fill-db", "z"), "--fill-db beside --db"),
    (("--fill-db", "z"), "--fill-db needs -D"),
    (("-D", "x", "--explain-min", "2"), "--explain-min and --fill-min-score need --fill-db"),
    (("-D", "x", "--fill-db", "z", "--explain-min", "0"), "--explain-min must be >= 1"),
    (("-D", "x", "--fill-db", "z", "--max-hits", "0"), "--max-hits must be in 1..64"),
])
def test_flag_errors_name_the_flag(tmp_path, args, word):
    got = _run("call_regions", "-q", "q.fna", "-o", tmp_path / "o.tsv", *args)
    assert got.returncode == 2 and word in got.stderr, got.stderr


def test_a_missing_index_is_an_error_that_names_it(planted):
    d = planted[0]
    got = _run("call_regions", "-q", d / "c.fna", "-o", d / "e.tsv", "-D", d / "data", "--fill-db", d / "missing.kgsdb")
    assert got.returncode == 1 and "missing.kgsdb" in got.stderr
