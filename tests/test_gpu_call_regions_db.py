"""call_regions --db end to end on the GPU: make_search_db writes an index of annotated proteins, call_regions --db locates the genes
planted from them on contigs: the regions lie at the planted coordinates under the index's function names, --hits agrees with the
CALLs, the outputs do not depend on where the batches are cut, a frameshifted gene is repaired, and flag errors name the flag."""
import contextlib
import importlib
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest

from kmergutsjava_amd import synth
from test_translated_host import _contig, _frameshift_case, _protein

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(mod, *args):
    """The front end's main() in this process (a process per run would cost seconds each): -> returncode, stdout, stderr."""
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            rc = importlib.import_module("kmergutsjava_amd." + mod).main([str(a) for a in args])
        except SystemExit as e:
            rc = e.code
    return SimpleNamespace(returncode=rc, stdout=out.getvalue(), stderr=err.getvalue())


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """Six targets: t0 and t1 share the function `kinase`, t2 has `pump`, t3 has none (named by its id), t4 is the frameshifted
    gene's (`ligase`), t5 is planted nowhere.  Five contigs with known leads, strands and frames."""
    d = tmp_path_factory.mktemp("db")
    rng = np.random.default_rng(12)
    gene, shifted = _frameshift_case(1)
    prots = [_protein(rng, 40), _protein(rng, 55), _protein(rng, 70), _protein(rng, 45), gene, _protein(rng, 60)]
    (d / "t.faa").write_text("".join(">t%d\n%s\n" % (k, p) for k, p in enumerate(prots)))
    (d / "t.tsv").write_text("t0\tkinase\nt1\tkinase\nt2\tpump\nt4\tligase\n")
    plan = [(0, 30, 33, 0), (1, 31, 34, 1), (2, 32, 35, 0), (3, 30, 34, 1)]         # target, lead, tail, strand
    contigs = [_contig(synth.back_translate(prots[t]), lead, tail, strand) for t, lead, tail, strand in plan] + [shifted]
    (d / "c.fna").write_text("".join(">c%d\n%s\n" % (k, c.decode()) for k, c in enumerate(contigs)))
    got = _run("make_search_db", "-d", d / "t.faa", "-A", d / "t.tsv", "-o", d / "t.kgsdb")
    assert got.returncode == 0, got.stderr
    (d / "plain.faa").write_text("".join(">t%d\n%s\n" % (k, p) for k, p in enumerate(prots)))
    got = _run("make_search_db", "-d", d / "plain.faa", "-o", d / "plain.kgsdb")
    assert got.returncode == 0, got.stderr
    return d, prots, plan, contigs


def _outputs(d, tag, *more, db="t.kgsdb"):
    names = {k: d / ("%s.%s" % (tag, k)) for k in ("tsv", "orfs", "faa", "shifts", "hits")}
    got = _run("call_regions", "--db", d / db, "-q", d / "c.fna", "-o", names["tsv"], "--orfs", names["orfs"], "--faa", names["faa"],
               "--repair", "--shifts", names["shifts"], "--hits", names["hits"], "--min-ratio", "20", *more)
    assert got.returncode == 0, got.stderr
    return got.stdout.strip(), {k: p.read_bytes() for k, p in names.items()}


def test_regions_at_the_planted_coordinates_under_the_index_s_names(planted):
    d, prots, plan, contigs = planted
    line, out = _outputs(d, "one")
    rows = [ln.split("\t") for ln in out["tsv"].decode().splitlines()]
    want_names = ["kinase", "kinase", "pump", "t3", "ligase"]
    assert [r[0] for r in rows] == ["c%d" % k for k in range(5)] and [r[4] for r in rows] == want_names
    for r, (t, lead, tail, strand), c in zip(rows, plan, contigs):
        L, n = len(c), 3 * len(prots[t])
        want = (lead + 3 + 1, lead + 3 + n) if strand == 0 else (L - (lead + 3 + n) + 1, L - (lead + 3))
        assert (int(r[1]), int(r[2]), r[3], r[8], r[9]) == (want[0], want[1], "+-"[strand], str(lead % 3), "kept"), r
        assert int(r[5]) > 0 and int(r[7]) == 1
    assert rows[4][3] == "-" and rows[4][8] == "0,2" and rows[4][7] == "2"
    assert line.endswith(", db: index (6 targets), fragments: %d, translated hits: 6, calls: 6" % int(line.split("fragments: ")[1].split(",")[0]))
    assert "Contigs: 5, with calls: 5, regions: 5, kept: 5, multi-frame: 1" in line and ", repaired: 1, unrepaired: 0" in line
    # the proteins: the planted ones as they are, the frameshifted one with both its ends
    faa = out["faa"].decode().split(">")[1:]
    seqs = ["".join(x.splitlines()[1:]) for x in faa]
    heads = [x.splitlines()[0] for x in faa]
    assert len(seqs) == 5 and [h.split(" ", 1)[1] for h in heads] == want_names
    for k, (t, lead, tail, strand) in enumerate(plan):
        assert seqs[k][1:] == prots[t][1:]
    assert prots[4][1:30] in seqs[4] and prots[4][-30:] in seqs[4]
    assert len(out["shifts"].splitlines()) == 1 and out["shifts"].split(b"\t")[4] == b"ligase"
    assert b"repaired" in out["orfs"].splitlines()[4]


def test_the_hits_file_agrees_with_the_calls(planted):
    d, prots, plan, contigs = planted
    _, out = _outputs(d, "hits")
    rows = [ln.split("\t") for ln in out["hits"].decode().splitlines()]
    assert len(rows) == 6 and all(len(r) == 16 for r in rows)
    assert [r[0] for r in rows] == ["c0", "c1", "c2", "c3", "c4", "c4"] and [r[7] for r in rows] == ["t0", "t1", "t2", "t3", "t4", "t4"]
    assert [r[15] for r in rows] == ["kinase", "kinase", "pump", "-", "ligase", "ligase"] and all(r[14] == "hit" and r[6] == "0" for r in rows)
    regions = [ln.split("\t") for ln in out["tsv"].decode().splitlines()]
    for r, (t, lead, tail, strand) in zip(rows, plan):
        reg = regions[int(r[0][1:])]
        # the fragment is the gene and its stop codon
        frag = (int(r[1]), int(r[2]) + 3) if strand == 0 else (int(r[1]) - 3, int(r[2]))
        assert r[1:4] == reg[1:4] and r[4] == str(lead % 3) and r[5] == "%s_%d_%d_%s" % (r[0], frag[0], frag[1], r[3])
        assert int(r[12]) == len(prots[t]) == int(r[13]) and r[9] == reg[5] and r[11] == "100"
    # the two halves of the frameshifted gene: inside its region, in two frames, their scores the region's
    a, b = rows[4], rows[5]
    reg = regions[4]
    assert {a[4], b[4]} == {"0", "2"} and int(a[9]) + int(b[9]) == int(reg[5])
    assert min(int(a[1]), int(b[1])) == int(reg[1]) and max(int(a[2]), int(b[2])) == int(reg[2])


def test_the_outputs_do_not_depend_on_where_the_batches_are_cut(planted):
    d, prots, plan, contigs = planted
    line, one = _outputs(d, "whole")
    for n in (1, 250, 400):
        cut_line, cut = _outputs(d, "cut%d" % n, "--batch-nt", n)
        assert cut == one and cut_line == line
    _, sel = _outputs(d, "sel", "--select", "--free-orfs", "--min-res", "30")
    _, sel_cut = _outputs(d, "selcut", "--select", "--free-orfs", "--min-res", "30", "--batch-nt", 1)
    assert sel == sel_cut and sel["tsv"] == one["tsv"]


def test_an_index_without_functions_names_by_target(planted):
    d, prots, plan, contigs = planted
    _, out = _outputs(d, "plain", db="plain.kgsdb")
    rows = [ln.split("\t") for ln in out["tsv"].decode().splitlines()]
    assert [r[4] for r in rows] == ["t0", "t1", "t2", "t3", "t4"]
    assert all(len(ln.split(b"\t")) == 15 for ln in out["hits"].splitlines())


@pytest.mark.parametrize("args,word", [
    ((), "one of -D and --db is required"),
    (("-D", "x", "--db", "y"), "give -D or --db, not both"),
    (("--db", "y", "-m", "4"), "-m beside --db"),
    (("--db", "y", "-M", "1"), "-M beside --db"),
    (("--db", "y", "-g", "100"), "-g beside --db"),
    (("--db", "y", "-O"), "-O beside --db"),
    (("-D", "x", "--hits", "h"), "--hits needs --db"),
    (("-D", "x", "--min-frag", "20"), "--min-frag needs --db"),
    (("-D", "x", "--batch-nt", "20"), "--batch-nt needs --db"),
    (("-D", "x", "--align-ref", "query"), "--align-ref needs --db"),
    (("--db", "y", "--max-hits", "0"), "--max-hits must be in 1..64"),
    (("--db", "y", "--min-frag", "0"), "--min-frag must be >= 1"),
    (("--db", "y", "--band", "8"), "--band needs --ungapped"),
])
def test_flag_errors_name_the_flag(tmp_path, args, word):
    got = _run("call_regions", "-q", "q.fna", "-o", tmp_path / "o.tsv", *args)
    assert got.returncode == 2 and word in got.stderr, got.stderr


def test_a_missing_index_is_an_error_that_names_it(planted):
    d = planted[0]
    got = _run("call_regions", "-q", d / "c.fna", "-o", d / "e.tsv", "--db", d / "missing.kgsdb")
    assert got.returncode == 1 and "missing.kgsdb" in got.stderr
