"""Say which OTU every contig (or protein) comes from: all OTU votes of a scan tallied per sequence on the GPU
(kg_result_otu_votes), one OTU per sequence, and the sample's bins.

    python -m kmergutsjava_amd.classify_contigs -D KmerData (-q contigs.fna[.gz] | -p proteins.faa[.gz]) -o classes.tsv
        [-m 5] [-M 0] [-g 200] [-O] [--min-votes 10] [--min-share 50] [--min-calls 1] [--all]
        [--votes votes.tsv [--top N]] [--bins bins.tsv] [--split DIR] [--truth seq_otu.tsv]
        [--compose [--comp-min-len 1500] [--comp-min-margin 2560] [--comp-min-train 200000] [--comp-model IN] [--save-comp-model OUT]]

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

--compose (DNA only) bins the contigs the votes cannot name by tetranucleotide composition (kg_contigs_compose): the assigned
contigs are the training set, their OTU the label.  Without --comp-model the label rows are made batch by batch, added up on the
host, --comp-min-train is applied once and every batch is scored with that model; with --comp-model the model comes from a file
--save-comp-model wrote.  A contig that is not assigned and is decided gets status composed and its otu column names the bin;
every -o line gains three trailing fields: comp_bin (the best bin, or - when the background is best), margin (best score minus
second) and windows.  An assigned contig that composition decides for another OTU is a conflict: it keeps its vote-based line and
is counted.  --bins lines gain n_composed and composed_length (a bin with composed contigs only comes behind the others, by OTU
index); --split puts composed contigs into their bin's file.  The summary line gains
`, composed: N, composed length: L, conflicts: K, models: M`, and with --truth `, composed agree: A, composed disagree: D`.
Model file: `#kmerguts composition model 1`, then one line per row, otu_index<TAB>otu name or -<TAB>256 counts, the background
last as -1<TAB>background; a name that disagrees with the directory's otu.index is an error.
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


def is_composed(c, k) -> bool:
    """A contig the votes did not assign and the composition decided."""
    return bool(not c["assigned"] and k["decided"])


def format_classes(ids, lens, classes, onames=None, write_all: bool = False, comp=None) -> bytes:
    """comp: the COMP_CLASS_DTYPE records of --compose, one per sequence (None: without the flag)."""
    lines = []
    for s, (sid, length, c) in enumerate(zip(ids, lens, classes)):
        k = comp[s] if comp is not None else None
        composed = k is not None and is_composed(c, k)
        if not (c["assigned"] or write_all or composed):
            continue
        otu = int(k["best"]) if composed else int(c["otu"])
        line = b"%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%d" % (
            sid, length, b"composed" if composed else status_of(c), otu_name(onames, otu) if otu >= 0 else b"-", c["votes"], c["total"],
            c["n_calls"], c["total_calls"], c["n_otus"], otu_name(onames, int(c["second_otu"])) if c["second_otu"] >= 0 else b"-",
            c["second_votes"])
        if k is not None:
            line += b"\t%s\t%d\t%d" % (otu_name(onames, int(k["best"])) if k["best"] >= 0 else b"-",
                                       int(k["score_best"]) - int(k["score_second"]), k["windows"])
        lines.append(line + b"\n")
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


def composed_bins(lens, classes, comp) -> dict:
    """OTU index -> [n_composed, composed_length]."""
    out = {}
    for length, c, k in zip(lens, classes, comp):
        if is_composed(c, k):
            a = out.setdefault(int(k["best"]), [0, 0])
            a[0] += 1
            a[1] += int(length)
    return out


def format_bins(bins, onames=None, composed: Optional[dict] = None) -> bytes:
    """composed: composed_bins() of --compose (None: without the flag)."""
    if composed is None:
        return b"".join(b"%s\t%d\t%d\t%d\t%d\n" % (otu_name(onames, int(b["oI"])), b["n_seqs"], b["length"], b["votes"], b["n_calls"])
                        for b in bins)
    lines = [b"%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((otu_name(onames, int(b["oI"])), b["n_seqs"], b["length"], b["votes"], b["n_calls"])
                                                 + tuple(composed.get(int(b["oI"]), (0, 0)))) for b in bins]
    have = {int(b["oI"]) for b in bins}
    lines += [b"%s\t0\t0\t0\t0\t%d\t%d\n" % (otu_name(onames, o), composed[o][0], composed[o][1]) for o in sorted(composed) if o not in have]
    return b"".join(lines)


COMP_MODEL_HEADER = b"#kmerguts composition model 1"


def format_comp_model(labels, counts, onames=None) -> bytes:
    """The model file: labels int32[M] ascending, counts int64[M + 1][256] with the background row last."""
    counts = np.asarray(counts, dtype=np.int64).reshape(len(labels) + 1, 256)
    lines = [COMP_MODEL_HEADER + b"\n"]
    for o, row in zip(list(labels) + [-1], counts):
        name = b"background" if o < 0 else (onames[o] if onames is not None and 0 <= o < len(onames) else b"-")
        lines.append(b"%d\t%s\t%s\n" % (o, name, b"\t".join(b"%d" % int(x) for x in row)))
    return b"".join(lines)


def parse_comp_model(data: bytes, name: str, onames=None):
    """-> (labels int32[M], counts int64[M + 1][256]); the library checks the rows themselves."""
    lines = [ln.rstrip(b"\r") for ln in data.split(b"\n")]
    while lines and not lines[-1]:
        lines.pop()
    if not lines or lines[0] != COMP_MODEL_HEADER:
        raise InputError("%s line 1: expected %s" % (name, COMP_MODEL_HEADER.decode()))
    labels, rows = [], []
    for n, line in enumerate(lines[1:], 2):
        f = line.split(b"\t")
        if len(f) != 258:
            raise InputError("%s line %d: expected otu_index<TAB>otu name<TAB>256 counts" % (name, n))
        try:
            o, row = int(f[0]), [int(x) for x in f[2:]]
        except ValueError:
            raise InputError("%s line %d: otu_index and the counts are integers" % (name, n)) from None
        if rows and labels[-1] < 0:
            raise InputError("%s line %d: a row behind the background row" % (name, n))
        if o < -1 or o >= 1 << 31 or (o == -1) != (f[1] == b"background"):
            raise InputError("%s line %d: the background row is -1<TAB>background, every other otu_index is >= 0" % (name, n))
        if o >= 0 and f[1] != b"-" and onames is not None and f[1] != otu_name(onames, o):
            raise InputError("%s line %d: otu %d is %s here and %s in otu.index" % (
                name, n, o, f[1].decode("utf-8", "replace"), otu_name(onames, o).decode("utf-8", "replace")))
        if min(row) < 0 or max(row) >= 1 << 62:
            raise InputError("%s line %d: a count outside 0 .. 2^62" % (name, n))
        labels.append(o)
        rows.append(row)
    if not rows or labels[-1] != -1:
        raise InputError("%s: the background row (-1<TAB>background) must come last" % name)
    return np.array(labels[:-1], dtype=np.int32), np.array(rows, dtype=np.int64).reshape(len(rows), 256)


def add_label_rows(acc: dict, row_labels, rows) -> None:
    """The label rows of one batch into acc (label -> int64[256])."""
    for o, row in zip(row_labels, rows):
        o = int(o)
        acc[o] = acc[o] + row if o in acc else np.array(row, dtype=np.int64)


def model_of_rows(acc: dict, background, min_train: int):
    """Rule 4 on the added-up rows -> (labels, counts) as format_comp_model takes them."""
    labels = [o for o in sorted(acc) if int(acc[o].sum()) >= min_train]
    counts = np.zeros((len(labels) + 1, 256), dtype=np.int64)
    for i, o in enumerate(labels):
        counts[i] = acc[o]
    counts[-1] = background
    return np.array(labels, dtype=np.int32), counts


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


def compare_truth_composed(ids, classes, comp, onames, labels: dict) -> dict:
    t = {"agree": 0, "disagree": 0}
    for sid, c, k in zip(ids, classes, comp):
        want = labels.get(sid)
        if want is not None and is_composed(c, k):
            t["agree" if otu_name(onames, int(k["best"])) == want else "disagree"] += 1
    return t


def comp_summary(lens, classes, comp, n_models: int, truth: Optional[dict] = None) -> str:
    """What --compose adds to the summary line."""
    done = [is_composed(c, k) for c, k in zip(classes, comp)]
    conflicts = sum(1 for c, k in zip(classes, comp) if c["assigned"] and k["decided"] and int(k["best"]) != int(c["otu"]))
    line = ", composed: %d, composed length: %d, conflicts: %d, models: %d" % (
        sum(done), sum(int(n) for n, d in zip(lens, done) if d), conflicts, n_models)
    if truth is not None:
        line += ", composed agree: %d, composed disagree: %d" % (truth["agree"], truth["disagree"])
    return line


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


def write_split(split_dir: str, ids, seqs, classes, bins, aa: bool, comp=None) -> None:
    os.makedirs(split_dir, exist_ok=True)
    ext = "faa" if aa else "fna"
    parts = {int(b["oI"]): [] for b in bins}
    rest = []
    for n, (sid, s, c) in enumerate(zip(ids, seqs, classes)):
        if comp is not None and is_composed(c, comp[n]):
            parts.setdefault(int(comp[n]["best"]), []).append(b">%s\n%s\n" % (sid, s))
            continue
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
                     device: int = 0, compose: bool = False, comp_min_len: int = 1500, comp_min_margin: int = 2560,
                     comp_min_train: int = 200000, comp_model: Optional[str] = None, save_comp_model: Optional[str] = None) -> str:
    """Write the classes (and what else was asked for); returns the summary line."""
    if (comp_model or save_comp_model) and not compose:
        raise ValueError("--comp-model and --save-comp-model need --compose")
    if compose and aa:
        raise ValueError("--compose bins DNA contigs: it cannot be combined with -p")
    from . import _native as N
    from . import hotpath
    from .kmer_guts_java import KmerGutsJava, _resident_table
    table_path = _data_file(data_dir, "kmer.table.mem_map")
    if table_path is None:
        raise FileNotFoundError("%s holds no kmer.table.mem_map[.gz]" % data_dir)
    otu_path = _data_file(data_dir, "otu.index")
    onames = parse_index(_read(otu_path), otu_path) if otu_path else None
    truth_labels = parse_truth(_read(truth), truth) if truth else None
    ids, seqs = parse_fasta(_read(query), query)
    lens = [len(s) for s in seqs]
    tab = _resident_table(table_path, device)
    params = hotpath.Params(aa=aa, order_constraint=order_constraint, min_hits=min_hits, min_weighted_hits=min_weighted_hits,
                            max_gap=max_gap)
    classes = np.zeros(len(ids), dtype=N.OTU_CLASS_DTYPE)
    vote_parts, bin_parts = [], []
    vote_start = np.zeros(len(ids) + 1, dtype=np.int64)
    model = parse_comp_model(_read(comp_model), comp_model, onames) if comp_model else None
    batches = []
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
        batches.append((k, j, off))
        k = j
    bins = merge_bins(bin_parts)
    comp = None
    if compose:
        # the assigned contigs are the training set; the label rows of the batches add up, min_train is applied once
        labels = np.where(classes["assigned"] != 0, classes["otu"], -1).astype(np.int32)
        if model is None:
            acc, background = {}, np.zeros(256, dtype=np.int64)
            for k, j, off in batches:
                part = hotpath.compose_contigs(b"".join(seqs[k:j]), off, labels[k:j], None, comp_min_len, comp_min_margin,
                                               1 << 62, device=device)     # (no row is a model yet: nothing but the background is scored)
                add_label_rows(acc, part["row_labels"], part["rows"])
                background += part["background"]
            model = model_of_rows(acc, background, comp_min_train)
        comp = np.zeros(len(ids), dtype=N.COMP_CLASS_DTYPE)
        for k, j, off in batches:
            comp[k:j] = hotpath.compose_contigs(b"".join(seqs[k:j]), off, labels[k:j], model, comp_min_len, comp_min_margin,
                                                device=device)["classes"]
        if save_comp_model:
            with open(save_comp_model, "wb") as f:
                f.write(format_comp_model(model[0], model[1], onames))
    with open(out, "wb") as f:
        f.write(format_classes(ids, lens, classes, onames, write_all, comp))
    if votes_out:
        votes = np.concatenate(vote_parts) if vote_parts else np.zeros(0, dtype=N.VOTE_DTYPE)
        with open(votes_out, "wb") as f:
            f.write(format_votes(ids, votes, vote_start, onames, top))
    if bins_out:
        with open(bins_out, "wb") as f:
            f.write(format_bins(bins, onames, composed_bins(lens, classes, comp) if comp is not None else None))
    if split_dir:
        write_split(split_dir, ids, seqs, classes, bins, aa, comp)
    t = compare_truth(ids, classes, onames, truth_labels) if truth_labels is not None else None
    line = summary_line(lens, classes, bins, t)
    if comp is not None:
        line += comp_summary(lens, classes, comp, len(model[0]),
                             compare_truth_composed(ids, classes, comp, onames, truth_labels) if truth_labels is not None else None)
    return line


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
    ap.add_argument("--compose", action="store_true", help="bin the contigs without an OTU by tetranucleotide composition (DNA only)")
    ap.add_argument("--comp-min-len", type=int, default=1500, metavar="N", help="a composed contig has at least N nt (default 1500)")
    ap.add_argument("--comp-min-margin", type=int, default=2560, metavar="N", help="best score minus second >= N, in 1/256 bit (default 2560)")
    ap.add_argument("--comp-min-train", type=int, default=200000, metavar="N", help="an OTU is a model from N training windows on (default 200000)")
    ap.add_argument("--comp-model", default=None, metavar="IN", help="score with the model of this file instead of the sample's own")
    ap.add_argument("--save-comp-model", default=None, metavar="OUT", help="write the model the contigs were scored with")
    a = ap.parse_args(argv)
    if a.compose and a.p is not None:
        ap.error("--compose bins DNA contigs: it cannot be combined with -p")
    if (a.comp_model or a.save_comp_model) and not a.compose:
        ap.error("--comp-model and --save-comp-model need --compose")
    from . import _native as N
    try:
        line = classify_contigs(a.D, a.q or a.p, a.o, a.p is not None, a.m, a.M, a.g, a.O, a.min_votes, a.min_share, a.min_calls,
                                a.all, a.votes, a.top, a.bins, a.split, a.truth, 0, a.compose, a.comp_min_len, a.comp_min_margin,
                                a.comp_min_train, a.comp_model, a.save_comp_model)
    except (N.KmerGutsNativeError, InputError, OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
