"""Say which OTU every contig (or protein) comes from: all OTU votes of a scan tallied per sequence on the GPU
(kg_result_otu_votes), one OTU per sequence, and the sample's bins.

    python -m kmergutsjava_amd.classify_contigs -D KmerData (-q contigs.fna[.gz] | -p proteins.faa[.gz]) -o classes.tsv
        [-m 5] [-M 0] [-g 200] [-O] [--min-votes 10] [--min-share 50] [--min-calls 1] [--all]
        [--votes votes.tsv [--top N]] [--bins bins.tsv] [--split DIR] [--truth seq_otu.tsv]

Sequences are read with make_signatures.parse_fasta (a duplicate id is an error) and scanned (-q: DNA, six frames; -p: -a) in
batches of whole sequences of at most KmerGutsJava.MAX_BATCH_CHARS characters.  The table and otu.index[.gz] are loaded the way
the front ends load them.  Output lines of -o, in FASTA order:
    seq_id<TAB>length<TAB>status<TAB>otu<TAB>votes<TAB>total<TAB>n_calls<TAB>total_calls<TAB>n_otus<TAB>second<TAB>second_votes
status is assigned, below (votes, but the thresholds fail) or none (no vote); otu and second are names from otu.index when the
directory has one, otherwise numbers, and "-" when there is none.  Only assigned sequences are written unless --all is given.
--votes: seq_id, otu, votes, n_calls for every (sequence, OTU) pair in the library's order (most votes first), at most --top a
sequence.  --bins: otu, n_seqs, length, votes, n_calls, the batches' bins added up, longest first (then most votes, then the
smaller OTU index).  --split: DIR/otu_<index>.fna per bin and DIR/unassigned.fna (both .faa with -p), `>id` and the sequence on one
line -- feed each to call_regions on its own.  Stdout:
`Sequences: N, with votes: K, assigned: A, bins: B, assigned length: L of T, votes: V`, and with --truth (seq_id<TAB>otu name
lines) `, labelled: T, agree: C, disagree: D, missed: M`, compared by OTU name: of the T labelled sequences, C are assigned their
OTU, D another one, M are not assigned.  No output depends on where the batches are cut.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Optional

import numpy as np

from .annotate import _data_file, parse_index
from .make_signatures import InputError, _read, parse_fasta


def otu_name(onames, o: int) -> bytes:
    return onames[o] if onames is not None and 0 <= o < len(onames) else b"%d" % o


def status_of(c) -> bytes:
    return b"assigned" if c["assigned"] else (b"below" if c["n_otus"] else b"none")


def format_classes(ids, lens, classes, onames=None, write_all: bool = False) -> bytes:
    lines = []
    for sid, length, c in zip(ids, lens, classes):
        if not (c["assigned"] or write_all):
            continue
        lines.append(b"%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%d\n" % (
            sid, length, status_of(c), otu_name(onames, int(c["otu"])) if c["otu"] >= 0 else b"-", c["votes"], c["total"],
            c["n_calls"], c["total_calls"], c["n_otus"], otu_name(onames, int(c["second_otu"])) if c["second_otu"] >= 0 else b"-",
            c["second_votes"]))
    return b"".join(lines)


def format_votes(ids, votes, vote_start, onames=None, top: Optional[int] = None) -> bytes:
    lines = []
    for s, sid in enumerate(ids):
        a, b = int(vote_start[s]), int(vote_start[s + 1])
        if top is not None:
            b = min(b, a + max(int(top), 0))
        for v in votes[a:b]:
            lines.append(b"%s\t%s\t%d\t%d\n" % (sid, otu_name(onames, int(v["oI"])), v["votes"], v["n_calls"]))
    return b"".join(lines)


def merge_bins(parts) -> np.ndarray:
    """The bins of several batches added up and put in the library's order: length and votes descending, oI ascending."""
    from . import _native as N
    acc = {}
    for bins in parts:
        for b in bins:
            a = acc.setdefault(int(b["oI"]), [0, 0, 0, 0])
            a[0] += int(b["n_seqs"])
            a[1] += int(b["length"])
            a[2] += int(b["votes"])
            a[3] += int(b["n_calls"])
    rows = sorted(((o, *v) for o, v in acc.items()), key=lambda r: (-r[2], -r[3], r[0]))
    out = np.zeros(len(rows), dtype=N.OTU_BIN_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def format_bins(bins, onames=None) -> bytes:
    return b"".join(b"%s\t%d\t%d\t%d\t%d\n" % (otu_name(onames, int(b["oI"])), b["n_seqs"], b["length"], b["votes"], b["n_calls"])
                    for b in bins)


def parse_truth(data: bytes, name: str) -> dict:
    out = {}
    for n, raw in enumerate(data.split(b"\n"), 1):
        line = raw.rstrip(b"\r")
        if not line:
            continue
        f = line.split(b"\t")
        if len(f) < 2 or not f[0] or not f[1]:
            raise InputError("%s line %d: expected seq_id<TAB>otu name" % (name, n))
        if f[0] in out:
            raise InputError("%s line %d: sequence %s is labelled twice" % (name, n, f[0].decode("utf-8", "replace")))
        out[f[0]] = f[1]
    return out


def compare_truth(ids, classes, onames, labels: dict) -> dict:
    t = {"labelled": 0, "agree": 0, "disagree": 0, "missed": 0}
    for sid, c in zip(ids, classes):
        want = labels.get(sid)
        if want is None:
            continue
        t["labelled"] += 1
        if not c["assigned"]:
            t["missed"] += 1
        elif otu_name(onames, int(c["otu"])) == want:
            t["agree"] += 1
        else:
            t["disagree"] += 1
    return t


def summary_line(lens, classes, bins, truth: Optional[dict] = None) -> str:
    lens = np.asarray(lens, dtype=np.int64)
    asg = classes["assigned"] != 0
    line = "Sequences: %d, with votes: %d, assigned: %d, bins: %d, assigned length: %d of %d, votes: %d" % (
        len(classes), int((classes["n_otus"] > 0).sum()), int(asg.sum()), len(bins), int(lens[asg].sum()), int(lens.sum()),
        int(classes["total"].astype(np.int64).sum()))
    if truth is not None:
        line += ", labelled: %d, agree: %d, disagree: %d, missed: %d" % (truth["labelled"], truth["agree"], truth["disagree"],
                                                                         truth["missed"])
    return line


def write_split(split_dir: str, ids, seqs, classes, bins, aa: bool) -> None:
    os.makedirs(split_dir, exist_ok=True)
    ext = "faa" if aa else "fna"
    parts = {int(b["oI"]): [] for b in bins}
    rest = []
    for sid, s, c in zip(ids, seqs, classes):
        (parts[int(c["otu"])] if c["assigned"] else rest).append(b">%s\n%s\n" % (sid, s))
    for o, recs in parts.items():
        with open(os.path.join(split_dir, "otu_%d.%s" % (o, ext)), "wb") as f:
            f.write(b"".join(recs))
    with open(os.path.join(split_dir, "unassigned.%s" % ext), "wb") as f:
        f.write(b"".join(rest))


def classify_contigs(data_dir: str, query: str, out: str, aa: bool = False, min_hits: int = 5, min_weighted_hits: int = 0,
                     max_gap: int = 200, order_constraint: bool = False, min_votes: int = 10, min_share: int = 50,
                     min_calls: int = 1, write_all: bool = False, votes_out: Optional[str] = None, top: Optional[int] = None,
                     bins_out: Optional[str] = None, split_dir: Optional[str] = None, truth: Optional[str] = None,
                     device: int = 0) -> str:
    """Write the classes (and what else was asked for); returns the summary line."""
    from . import _native as N
    from . import hotpath
    from .kmer_guts_java import KmerGutsJava, _resident_table
    table_path = _data_file(data_dir, "kmer.table.mem_map")
    if table_path is None:
        raise FileNotFoundError("%s holds no kmer.table.mem_map[.gz]" % data_dir)
    otu_path = _data_file(data_dir, "otu.index")
    onames = parse_index(_read(otu_path), otu_path) if otu_path else None
    labels = parse_truth(_read(truth), truth) if truth else None
    ids, seqs = parse_fasta(_read(query), query)
    lens = [len(s) for s in seqs]
    tab = _resident_table(table_path, device)
    params = hotpath.Params(aa=aa, order_constraint=order_constraint, min_hits=min_hits, min_weighted_hits=min_weighted_hits,
                            max_gap=max_gap)
    classes = np.zeros(len(ids), dtype=N.OTU_CLASS_DTYPE)
    vote_parts, bin_parts = [], []
    vote_start = np.zeros(len(ids) + 1, dtype=np.int64)
    k = 0
    while k < len(ids):
        j, size = k, 0
        while j < len(ids) and (j == k or size + lens[j] <= KmerGutsJava.MAX_BATCH_CHARS):
            size += lens[j]
            j += 1
        off = np.zeros(j - k + 1, dtype=np.int64)
        off[1:] = np.cumsum(lens[k:j])
        with tab.scan(b"".join(seqs[k:j]), off, params) as r:
            votes, start, cls, bins = r.otu_votes(off, min_votes, min_share, min_calls)
        classes[k:j] = cls
        vote_start[k + 1:j + 1] = vote_start[k] + start[1:]
        if votes_out:
            vote_parts.append(votes)
        bin_parts.append(bins)
        k = j
    bins = merge_bins(bin_parts)
    with open(out, "wb") as f:
        f.write(format_classes(ids, lens, classes, onames, write_all))
    if votes_out:
        votes = np.concatenate(vote_parts) if vote_parts else np.zeros(0, dtype=N.VOTE_DTYPE)
        with open(votes_out, "wb") as f:
            f.write(format_votes(ids, votes, vote_start, onames, top))
    if bins_out:
        with open(bins_out, "wb") as f:
            f.write(format_bins(bins, onames))
    if split_dir:
        write_split(split_dir, ids, seqs, classes, bins, aa)
    t = compare_truth(ids, classes, onames, labels) if labels is not None else None
    return summary_line(lens, classes, bins, t)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.classify_contigs",
                                 description="One OTU per contig (or protein) from all OTU votes of a scan, on the GPU.")
    ap.add_argument("-D", required=True, metavar="DATADIR", help="data directory (kmer.table.mem_map[.gz], otu.index[.gz])")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("-q", metavar="CONTIGS", help="DNA FASTA (.gz allowed)")
    src.add_argument("-p", metavar="PROTEINS", help="protein FASTA (.gz allowed): an -a scan")
    ap.add_argument("-o", required=True, metavar="OUT", help="classes TSV to write")
    ap.add_argument("-m", type=int, default=5, help="minHits (default 5)")
    ap.add_argument("-M", type=int, default=0, help="minWeightedHits (default 0)")
    ap.add_argument("-g", type=int, default=200, help="maxGap (default 200)")
    ap.add_argument("-O", action="store_true", help="order constraint")
    ap.add_argument("--min-votes", type=int, default=10, help="best votes >= this (default 10, this project's choice)")
    ap.add_argument("--min-share", type=int, default=50, help="100 best votes >= this * all votes (default 50)")
    ap.add_argument("--min-calls", type=int, default=1, help="the best OTU's votes come from at least this many CALLs (default 1)")
    ap.add_argument("--all", action="store_true", help="write every sequence, not only the assigned ones")
    ap.add_argument("--votes", default=None, metavar="VOTES", help="also write every (sequence, OTU) tally")
    ap.add_argument("--top", type=int, default=None, metavar="N", help="at most N --votes lines a sequence")
    ap.add_argument("--bins", default=None, metavar="BINS", help="also write the sample's OTU table")
    ap.add_argument("--split", default=None, metavar="DIR", help="also write one FASTA per bin and unassigned.fna")
    ap.add_argument("--truth", default=None, metavar="LABELS", help="seq_id<TAB>otu name lines to compare with")
    a = ap.parse_args(argv)
    from . import _native as N
    try:
        line = classify_contigs(a.D, a.q or a.p, a.o, a.p is not None, a.m, a.M, a.g, a.O, a.min_votes, a.min_share, a.min_calls,
                                a.all, a.votes, a.top, a.bins, a.split, a.truth)
    except (N.KmerGutsNativeError, InputError, OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
