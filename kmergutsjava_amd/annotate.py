"""Assign one function per protein from an -a scan on the GPU (kg_result_assign), and optionally compare with known
annotations.

    python -m kmergutsjava_amd.annotate -D KmerData -p proteins.faa[.gz] -o assignments.tsv [-m 5] [-M 0] [-g 200] [-O]
                                        [--min-score 0] [--min-share 50] [--all] [--truth annotations.tsv]

Proteins are read with make_signatures.parse_fasta (a duplicate id is an error), so a protein's windows are the ones
make_signatures derived from, and scanned -a in batches of whole proteins of at most KmerGutsJava.MAX_BATCH_CHARS residues.
The table and function.index[.gz] are loaded the way the front ends load them.  Output lines, in FASTA order:
    protein_id<TAB>status<TAB>function<TAB>score<TAB>total<TAB>weighted<TAB>otu
status is assigned, below (CALLs, but the thresholds fail) or none (no CALL); function is the best function's name ("-" when
there is none); weighted is %.9g; otu is the name from otu.index when the directory has one, otherwise the number.  Only
assigned proteins are written unless --all is given.  Stdout: `Proteins: N, with calls: K, assigned: A`, and with --truth
(the make_signatures -A format) `, annotated: T, agree: C, disagree: D, missed: M`, compared by function name: of the T
annotated proteins, C are assigned their annotated function, D another one, M are not assigned.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Optional

import numpy as np

from .make_signatures import InputError, _read, parse_annotations, parse_fasta


def parse_index(data: bytes, name: str = "index"):
    """`<i>\\t<name>` lines, dense and in order (the layout of function.index and otu.index)."""
    out = []
    for raw in data.split(b"\n"):
        line = raw.rstrip(b"\r")
        if not line:
            continue
        tab = line.find(b"\t")
        if tab < 0 or not line[:tab].strip().isdigit() or int(line[:tab]) != len(out):
            raise ValueError("%s: the index must be dense and in order (see line %d)" % (name, len(out) + 1))
        out.append(line[tab + 1:])
    return out


def summary_line(n: int, with_calls: int, assigned: int, truth: Optional[dict] = None) -> str:
    line = "Proteins: %d, with calls: %d, assigned: %d" % (n, with_calls, assigned)
    if truth is not None:
        line += ", annotated: %d, agree: %d, disagree: %d, missed: %d" % (truth["annotated"], truth["agree"], truth["disagree"],
                                                                          truth["missed"])
    return line


def _data_file(d: str, name: str) -> Optional[str]:
    p = os.path.join(d, name)
    if os.path.exists(p + ".gz"):
        return p + ".gz"
    return p if os.path.exists(p) else None


def annotate(data_dir: str, proteins: str, out: str, min_hits: int = 5, min_weighted_hits: int = 0, max_gap: int = 200,
             order_constraint: bool = False, min_score: int = 0, min_share: int = 50, write_all: bool = False,
             truth: Optional[str] = None, device: int = 0) -> str:
    """Write the assignments; returns the summary line."""
    from . import hotpath
    from .kmer_guts_java import KmerGutsJava, _resident_table
    table_path = _data_file(data_dir, "kmer.table.mem_map")
    fn_path = _data_file(data_dir, "function.index")
    if table_path is None or fn_path is None:
        raise FileNotFoundError("%s holds no kmer.table.mem_map[.gz] or function.index[.gz]" % data_dir)
    fnames = parse_index(_read(fn_path), fn_path)
    otu_path = _data_file(data_dir, "otu.index")
    onames = parse_index(_read(otu_path), otu_path) if otu_path else None
    ann = parse_annotations(_read(truth), truth) if truth else None
    ids, seqs = parse_fasta(_read(proteins), proteins)
    tab = _resident_table(table_path, device)
    params = hotpath.Params(aa=True, order_constraint=order_constraint, min_hits=min_hits, min_weighted_hits=min_weighted_hits,
                            max_gap=max_gap)
    res = np.zeros(len(ids), dtype=hotpath.N.ASSIGNMENT_DTYPE)
    k = 0
    while k < len(ids):
        j, size = k, 0
        while j < len(ids) and (j == k or size + len(seqs[j]) <= KmerGutsJava.MAX_BATCH_CHARS):
            size += len(seqs[j])
            j += 1
        off = np.zeros(j - k + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs[k:j]])
        with tab.scan(b"".join(seqs[k:j]), off, params) as r:
            res[k:j] = r.assign(min_score, min_share)
        k = j

    def fname(f):
        return fnames[f] if 0 <= f < len(fnames) else b"%d" % f

    def oname(o):
        return onames[o] if onames is not None and 0 <= o < len(onames) else b"%d" % o

    lines = []
    for pid, a in zip(ids, res):
        status = b"assigned" if a["assigned"] else (b"below" if a["n_calls"] else b"none")
        if not (a["assigned"] or write_all):
            continue
        lines.append(b"%s\t%s\t%s\t%d\t%d\t%s\t%s\n" % (pid, status, fname(int(a["fI"])) if a["fI"] >= 0 else b"-", a["score"],
                                                       a["total"], (b"%.9g" % float(a["weighted"])), oname(int(a["otu"]))))
    with open(out, "wb") as f:
        f.write(b"".join(lines))
    t = None
    if ann is not None:
        t = {"annotated": 0, "agree": 0, "disagree": 0, "missed": 0}
        for pid, a in zip(ids, res):
            want = ann.get(pid)
            if want is None:
                continue
            t["annotated"] += 1
            if not a["assigned"]:
                t["missed"] += 1
            elif fname(int(a["fI"])) == want[0]:
                t["agree"] += 1
            else:
                t["disagree"] += 1
    return summary_line(len(ids), int((res["n_calls"] > 0).sum()), int(res["assigned"].sum()), t)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.annotate",
                                 description="Assign one function per protein from an -a scan on the GPU.")
    ap.add_argument("-D", required=True, metavar="DATADIR", help="data directory (kmer.table.mem_map[.gz], function.index[.gz])")
    ap.add_argument("-p", required=True, metavar="PROTEINS", help="protein FASTA (.gz allowed)")
    ap.add_argument("-o", required=True, metavar="OUT", help="assignments TSV to write")
    ap.add_argument("-m", type=int, default=5, help="minHits (default 5)")
    ap.add_argument("-M", type=int, default=0, help="minWeightedHits (default 0)")
    ap.add_argument("-g", type=int, default=200, help="maxGap (default 200)")
    ap.add_argument("-O", action="store_true", help="order constraint")
    ap.add_argument("--min-score", type=int, default=0, help="S_best >= this (default 0, this project's choice)")
    ap.add_argument("--min-share", type=int, default=50, help="100 S_best >= this * T (default 50, this project's choice)")
    ap.add_argument("--all", action="store_true", help="write every protein, not only the assigned ones")
    ap.add_argument("--truth", default=None, metavar="ANNOTATIONS", help="protein_id<TAB>function[<TAB>otu] lines to compare with")
    a = ap.parse_args(argv)
    from . import _native as N
    try:
        line = annotate(a.D, a.p, a.o, a.m, a.M, a.g, a.O, a.min_score, a.min_share, a.all, a.truth)
    except (N.KmerGutsNativeError, InputError, OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
