"""Cluster proteins into families by shared 8-mers on the GPU (kg_proteins_cluster), and name the families: the step between
`call_regions --free-orfs --faa` and `make_signatures -A`.

    python -m kmergutsjava_amd.cluster_proteins -p proteins.faa[.gz] [-p more.faa ...] -o families.tsv [--min-shared 5]
                                                [--min-cover 20] [--min-size 2] [--all] [-A annotations.tsv] [--known known.tsv]
                                                [--align [--min-ratio 50] [--align-ref longer|member] [--gap-open 11]
                                                 [--gap-extend 1] [--max-cells N] [--edges edges.tsv]]
                                                [--mask [--mask-window 12] [--mask-trigger 563] [--mask-extend 640]]

The proteins of all -p files form one batch, in the order given (FASTA as make_signatures reads it); a protein id that occurs
twice, in one file or across files, is an error.  include/kmerguts_hip.h states the rule: every protein of a k-mer is linked to
the k-mer's longest protein, a link is an edge when the two share at least --min-shared distinct 8-mers and at least
--min-cover percent of the member's distinct 8-mers, a family is a connected component.  The defaults 5 and 20 are this
project's choice (a fifth of the exact 8-mers shared is roughly 80 % identity).  Single linkage chains, and a repeat or a
domain can join two families: --min-cover is the lever, and --align the repair.

--align verifies every link that passed the two 8-mer tests by a local alignment of its two proteins (kg_proteins_cluster_aligned;
BLOSUM62 in align_scores.py, a gap of k residues costs --gap-open + k * --gap-extend, no traceback): the link stays an edge only
if 100 * score >= --min-ratio * ref, where ref is the larger of the two proteins' self-scores (--align-ref longer, the default) or
the member's own (--align-ref member).  Against the larger self-score both proteins must be covered, which cuts the chain through
a shared domain; the price is that a true fragment, such as a partial5 ORF at a contig end, falls out of its family, and
--align-ref member is the lever.  A pair of more than --max-cells cells (default 2^26) is not aligned and its link is kept.  The
defaults 50 and longer are this project's choice.

-o lines: `protein_id<TAB>family_<root id><TAB>size<TAB>root id<TAB>best id or -<TAB>shared`, in FASTA order; only the proteins
of families of at least --min-size (default 2) are written, every protein with --all.  With --align every line gains two fields:
the score and the ratio in percent (100 * score / ref, rounded down) of the protein's link to its best, `-` and `-` without one
or when that pair was not aligned.
--edges lines (needs --align), one per link that passed the 8-mer tests, in ascending (member, centre) order:
`member id<TAB>centre id<TAB>shared<TAB>score<TAB>ref<TAB>ratio<TAB>member end<TAB>centre end<TAB>kept|cut|skipped`, the ends 1-based
(0 without one).
-A writes make_signatures' annotation format, `protein_id<TAB>function`: first the lines of --known, copied unchanged, then for
each protein absent from --known and in a family of at least --min-size one line `id<TAB>hypothetical protein family_<root id>`.
--mask keeps low-complexity segments (a poly-Q, a QEQEQE linker, a charged tail) from linking proteins (kg_proteins_cluster_masked;
mask_proteins states the rule and writes the same mask to a file): the 8-mer pass reads every protein with its masked residues
taken for non-residues, so a protein's distinct 8-mers in --min-cover are those outside its segments; --align reads the proteins
as they are.  --mask-window, --mask-trigger and --mask-extend are mask_proteins' --window, --trigger and --extend.  The summary
line then gains `, mask: W/T/E, masked residues: N`; without --mask every byte is as before.
"""
from __future__ import annotations

import argparse
import sys
from typing import Optional

import numpy as np

from .make_signatures import InputError, _read, parse_annotations, parse_fasta

FAMILY_PREFIX = b"family_"
FUNCTION_PREFIX = b"hypothetical protein "


def read_proteins(paths):
    """-> (ids, sequences) of all files in order.  Raises InputError naming an id that occurs twice."""
    ids, seqs, where = [], [], {}
    for path in paths:
        i, s = parse_fasta(_read(path), path)
        for pid in i:
            if pid in where:
                raise InputError("%s: duplicate protein id %s (first in %s)" % (path, pid.decode("latin-1"), where[pid]))
            where[pid] = path
        ids += i
        seqs += s
    return ids, seqs


def family_sizes(rec) -> np.ndarray:
    """The size of every protein's family."""
    return np.bincount(rec["root"], minlength=len(rec))[rec["root"]] if len(rec) else np.zeros(0, dtype=np.int64)


EDGE_STATUS = (b"kept", b"cut", b"skipped")


def _ratio(score: int, ref: int) -> bytes:
    return b"%d" % (100 * score // ref) if score >= 0 and ref > 0 else b"-"


def format_families(ids, rec, min_size: int = 2, write_all: bool = False, edges=None) -> bytes:
    """edges: None, or the edge records of an aligned run: every line gains the score and the ratio of the link to best."""
    size = family_sizes(rec)
    link = None if edges is None else {(int(e["member"]), int(e["centre"])): e for e in edges}
    out = []
    for k, pid in enumerate(ids):
        if not write_all and size[k] < min_size:
            continue
        best = int(rec["best"][k])
        line = b"%s\t%s%s\t%d\t%s\t%s\t%d" % (pid, FAMILY_PREFIX, ids[int(rec["root"][k])], int(size[k]), ids[int(rec["root"][k])],
                                             ids[best] if best >= 0 else b"-", int(rec["shared"][k]))
        if link is not None:
            e = link.get((k, best))
            if e is None or int(e["score"]) < 0:
                line += b"\t-\t-"
            else:
                line += b"\t%d\t%s" % (int(e["score"]), _ratio(int(e["score"]), int(e["ref"])))
        out.append(line + b"\n")
    return b"".join(out)


def format_edges(ids, edges) -> bytes:
    """One line per edge record, in their order."""
    return b"".join(b"%s\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%s\n" % (
        ids[int(e["member"])], ids[int(e["centre"])], int(e["shared"]), int(e["score"]), int(e["ref"]),
        _ratio(int(e["score"]), int(e["ref"])), int(e["end_member"]) + 1, int(e["end_centre"]) + 1, EDGE_STATUS[int(e["status"])])
        for e in edges)


def format_annotations(ids, rec, known: bytes = b"", min_size: int = 2, known_name: str = "known") -> bytes:
    """The --known lines unchanged, then one line per protein absent from them whose family has at least min_size members."""
    have = parse_annotations(known, known_name)
    size = family_sizes(rec)
    out = [known if not known or known.endswith(b"\n") else known + b"\n"]
    for k, pid in enumerate(ids):
        if pid not in have and size[k] >= min_size:
            out.append(b"%s\t%s%s%s\n" % (pid, FUNCTION_PREFIX, FAMILY_PREFIX, ids[int(rec["root"][k])]))
    return b"".join(out)


def cluster_proteins(proteins, out: str, min_shared: int = 5, min_cover: int = 20, min_size: int = 2, write_all: bool = False,
                     annotations: Optional[str] = None, known: Optional[str] = None, device: int = 0, cluster=None,
                     align: Optional[dict] = None, edges: Optional[str] = None, mask: Optional[dict] = None) -> str:
    """Write the files; returns the summary line.  `cluster` replaces hotpath.cluster_proteins (tests).  align: None, or the
    alignment parameters of hotpath.cluster_proteins; edges: the --edges file; mask: None, or a dict of window, trigger, extend as
    hotpath.cluster_proteins takes it (--mask)."""
    if min_size < 1:
        raise ValueError("--min-size must be >= 1")
    if edges is not None and align is None:
        raise ValueError("--edges needs --align")
    if known is not None and annotations is None:
        raise ValueError("--known needs -A")
    ids, seqs = read_proteins(proteins)
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        offsets[1:] = np.cumsum([len(s) for s in seqs])
    if cluster is None:
        from . import hotpath
        cluster = hotpath.cluster_proteins
    more = {} if mask is None else {"mask": mask}
    if align is None:
        rec, st = cluster(b"".join(seqs), offsets, min_shared=min_shared, min_cover_pct=min_cover, device=device, **more)
    else:
        rec, st = cluster(b"".join(seqs), offsets, min_shared=min_shared, min_cover_pct=min_cover, device=device, align=align, **more)
    with open(out, "wb") as f:
        f.write(format_families(ids, rec, min_size, write_all, st["edge_records"] if align is not None else None))
    if edges is not None:
        with open(edges, "wb") as f:
            f.write(format_edges(ids, st["edge_records"]))
    if annotations is not None:
        text = format_annotations(ids, rec, _read(known) if known is not None else b"", min_size, known or "known")
        with open(annotations, "wb") as f:
            f.write(text)
    line = "Proteins: %d, families: %d, multi: %d, largest: %d, edges: %d, rounds: %d, ms: %.3f" % (
        st["proteins"], st["families"], st["families_multi"], st["largest"], st["edges"], st["rounds"], st.get("ms_total", 0.0))
    if align is not None:
        a = st["align"]
        line += ", aligned: %d, cut: %d, skipped: %d, align ms: %.3f" % (a["aligned"], a["cut"], a["skipped"], a.get("ms_align", 0.0))
    if mask is not None:
        from .mask_proteins import mask_words
        line += ", mask: %s, masked residues: %d" % (mask_words(mask), st["mask"]["masked_residues"])
    return line


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.cluster_proteins",
                                 description="Cluster proteins into families by shared 8-mers on the GPU.")
    ap.add_argument("-p", required=True, action="append", metavar="PROTEINS", help="protein FASTA (.gz allowed); may be given several times")
    ap.add_argument("-o", required=True, metavar="FAMILIES", help="families TSV to write")
    ap.add_argument("--min-shared", type=int, default=5, help="distinct 8-mers an edge shares at least (default 5, this project's choice)")
    ap.add_argument("--min-cover", type=int, default=20, help="... and percent of the member's distinct 8-mers (default 20, this project's choice)")
    ap.add_argument("--min-size", type=int, default=2, help="families of fewer proteins are not written (default 2)")
    ap.add_argument("--all", action="store_true", help="write every protein to -o, whatever its family's size")
    ap.add_argument("-A", default=None, metavar="ANNOTATIONS", help="also write protein_id<TAB>function lines for make_signatures -A")
    ap.add_argument("--known", default=None, metavar="KNOWN", help="with -A: annotations to copy unchanged; their proteins get no family line")
    ap.add_argument("--align", action="store_true", help="verify every link that passed the 8-mer tests by local alignment (BLOSUM62)")
    ap.add_argument("--min-ratio", type=int, default=50, help="with --align: an edge needs 100 * score >= this * ref (default 50, this project's choice)")
    ap.add_argument("--align-ref", choices=("longer", "member"), default="longer",
                    help="with --align: ref is the larger self-score of the two proteins (default) or the member's")
    ap.add_argument("--gap-open", type=int, default=11, help="with --align: a gap of k residues costs gap-open + k * gap-extend (default 11)")
    ap.add_argument("--gap-extend", type=int, default=1, help="(default 1)")
    ap.add_argument("--max-cells", type=int, default=1 << 26, help="with --align: a pair of more cells is not aligned and its link kept (default 2^26)")
    ap.add_argument("--edges", default=None, metavar="EDGES", help="with --align: write one line per link that passed the 8-mer tests")
    ap.add_argument("--mask", action="store_true", help="keep low-complexity segments out of the 8-mer pass (mask_proteins states the rule)")
    from .mask_proteins import add_mask_options, mask_from_options
    add_mask_options(ap, "--align reads the proteins as they are")
    a = ap.parse_args(argv)
    from . import _native as N
    align = dict(min_ratio_pct=a.min_ratio, ref=a.align_ref, gap_open=a.gap_open, gap_extend=a.gap_extend,
                 max_cells=a.max_cells) if a.align else None
    try:
        line = cluster_proteins(a.p, a.o, a.min_shared, a.min_cover, a.min_size, a.all, a.A, a.known, align=align, edges=a.edges,
                                mask=mask_from_options(ap, a, None))
    except (N.KmerGutsNativeError, InputError, OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print(line, file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
