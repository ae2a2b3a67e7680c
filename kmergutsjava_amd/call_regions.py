"""Locate function calls on contigs: a DNA scan whose CALL records are merged into function regions on the GPU
(kg_result_regions).

    python -m kmergutsjava_amd.call_regions -D KmerData -q contigs.fna[.gz] -o regions.tsv [-m 5] [-M 0] [-g 200] [-O]
                                            | --db DB.kgsdb [--min-frag 30] [--max-hits 1] [--batch-nt N] [--hits HITS.tsv]
                                              [the search's flags]
                                            [--merge-gap 600] [--min-score 0] [--min-len 0] [--all] [--gff]
                                            [--orfs ORFS.tsv] [--faa PROTEINS.faa] [--start-codons ATG,GTG,TTG]
                                            [--repair [--repair-min-count 0] [--max-junctions 4] [--shifts SHIFTS.tsv]]
                                            [--select [--max-overlap 60] [--max-overlap-pct 50]]
                                            [--free-orfs [--min-res 100]]
                                            [--coding [--min-coding 0] [--min-train 100000] [--coding-model IN]
                                             [--save-coding-model OUT]]
                                            [--starts [--start-rounds 4] [--min-train-starts 200] [--start-model IN]
                                             [--save-start-model OUT]]

The table and function.index[.gz] are loaded the way annotate loads them.  Contigs are read with
make_signatures.parse_fasta (a duplicate id is an error) and scanned whole, in batches of at most
KmerGutsJava.MAX_BATCH_CHARS characters.  Output, in FASTA order and inside a contig in the library's output order
(left, right, strand, function index), one line per kept region (every region with --all):
    contig_id<TAB>left+1<TAB>right+1<TAB>strand<TAB>function<TAB>score<TAB>weighted<TAB>n_calls<TAB>frames<TAB>status
with 1-based inclusive coordinates on the contig as given, strand + or -, weighted as %.9g, frames the frames of the region's
CALLs (e.g. `0` or `0,2`; more than one: a frameshift candidate) and status kept or below.  --gff writes GFF3 lines with the
same content instead.  Stdout: `Contigs: N, with calls: K, regions: R, kept: A, multi-frame: F`.

--orfs and --faa extend every region to its open reading frame on the GPU (kg_regionset_orfs; include/kmerguts_hip.h states the
rule) with the start codons of --start-codons (default ATG,GTG,TTG; `none` for no start search).  --orfs writes one line per
written region:
    contig_id<TAB>left+1<TAB>right+1<TAB>strand<TAB>frame<TAB>function<TAB>score<TAB>n_res<TAB>start<TAB>flags
with start the start codon or `-`, and flags the words stop, partial5, interrupted, multi-frame joined by commas (or `-`).
--faa writes `>contig_left+1_right+1_strand function` and the protein in 60-column lines, what annotate -p and
make_signatures -p read; an ORF with the contig, strand, left and right of an earlier written one is written once, under the
region with the largest score (ties: the first).  With either flag the summary line gains `, orfs: N, complete: C,
interrupted: I` (complete: stop, start and not interrupted).

--repair (with --orfs or --faa) repairs frameshifted genes on the GPU (kg_result_repair; include/kmerguts_hip.h states the
rule, integers only): a kept region with CALLs in more than one frame gets, in place of its best frame's ORF, the chain that
follows its CALLs from frame to frame, each junction put between the stops that bound it, as near the middle of the evidence gap
as they allow.  CALLs with fewer than --repair-min-count hits take no part; a region that changes frame more than
--max-junctions times (default 4, at most 8) is left alone.  The step runs before --free-orfs, so --select, --coding and --starts
see the new extents.  A repaired ORF's line gains the flag word `repaired` (and always has `interrupted`: it does not read in
one frame, so --coding does not train on it and --starts does not move it); the coding score printed for it is that of its first
frame read straight through its extent.  --shifts writes one line per junction of a written repaired ORF:
    contig_id<TAB>left+1<TAB>right+1<TAB>strand<TAB>function<TAB>junction pos+1<TAB>from_frame<TAB>to_frame<TAB>residue<TAB>gap
with residue the 1-based protein position of the first residue behind the junction and gap the nucleotides between the two
frames' evidence (negative: it overlaps).  The summary line gains `, repaired: N, unrepaired: M` behind the ORF counts
(unrepaired: multi-frame regions whose chain failed, had one frame left or too many junctions).  Without --repair every output
is byte for byte what it was.

--select makes the output a gene set: among the kept candidates -- the ORFs' extents with --orfs or --faa, else the regions'
extents -- the non-overlapping selection is taken on the GPU (kg_orfset_select / kg_regionset_select; include/kmerguts_hip.h
states the rule: two candidates of a contig conflict when they share more than --max-overlap nucleotides or more than
--max-overlap-pct percent of the shorter one, whatever their strands and functions, and the stronger one -- score, then
length, then position in the output -- wins).  Only selected candidates are written to the three outputs.  With --all every
candidate is written, the status is kept, below or overlapped, and the TSV and GFF lines gain one trailing field (GFF: the
attribute overlapped_by) that names the winner an overlapped candidate lost to as left+1..right+1:strand, or `-`.  The summary
line gains `, selected: S, overlapped: V`.

--free-orfs (with --orfs or --faa) fills the output with evidence-free candidates: every stop-free run of the six frames that
gives at least --min-res residues (default 100, this project's choice) from its first start codon of --start-codons, found on
the GPU (kg_orfset_add_free; include/kmerguts_hip.h states the rule).  The regions file never gains a line.  In the ORF file a
contig's lines are followed by its free ORFs in the library's order (strand, frame, position), each with function
`hypothetical protein`, score 0 and the extra flag word `free`; the protein file gets them as
`>contig_left+1_right+1_strand hypothetical protein` behind the contig's other proteins, an extent that is already written
being written once.  With --select they are candidates like the others: their score is 0, so a free ORF never beats a region's
ORF (raise --min-score to let long free ORFs replace weak regions) and among free ORFs the longer wins; with --all a free ORF's
line gains two trailing fields, its status kept or overlapped and the winner as in the regions file.  The summary line counts
the free ORFs among selected and overlapped and gains `, free: F` at its end.

--coding (with --orfs or --faa) scores every ORF by its in-frame hexamer log-odds on the GPU (kg_orfset_coding;
include/kmerguts_hip.h states the rule, integers only) and drops the free ORFs that score below --min-coding (default 0: the
genome's background explains the ORF at least as well as its genes do).  Without --coding-model every batch trains on its own
evidence ORFs; a batch is 1.5 * 10^9 characters, so that is one model for nearly every input.  A batch whose evidence ORFs hold
fewer than --min-train codon pairs (default 100000) is untrained: it prints one warning line on stderr, its scores are 0 and it
drops nothing.  --save-coding-model writes the counts summed over the batches as text: the line `#kmerguts coding model 1`, then
4096 lines HEXAMER<TAB>coding<TAB>background in index order.  --coding-model reads such a file and scores with its table
(kg_coding_table) instead of training: a draft with few known genes can borrow a relative's model.  Every line of the ORF file
gains its coding score as the last field.  A non-coding free ORF is written to neither the ORF nor the protein file; with --all
it is written with the flag word `noncoding`, and where --select adds a status the status is `noncoding`.  It is not a
candidate of --select, so it suppresses nothing.  The summary line gains `, coding: own|model|untrained, noncoding: N` (own: at
least one batch trained on itself).  Without --coding every output is byte for byte what it was.

--starts (with --coding) chooses the start codon of every complete, kept ORF by a start-site score on the GPU (kg_orfset_starts;
include/kmerguts_hip.h states the rule, integers only): the coding score of the ORF behind the candidate start, plus weights of
the 20 bases in front of it and of the start codon's spelling, trained in --start-rounds rounds (default 4) on the batch's own
evidence ORFs.  An evidence ORF's start is never moved into its region, any other start only as far as --min-res residues
remain.  A batch with fewer than --min-train-starts evidence ORFs with a start and an upstream stop (default 200), or whose
coding step was untrained, is untrained: it prints one warning line on stderr and moves nothing.  --save-start-model writes
the counts of the last round summed over the batches as text: the line `#kmerguts start model 1`, then 80 lines
position<TAB>base<TAB>chosen<TAB>candidates (position 0 is 20 bases in front of the start) and 3 lines
type<TAB>ATG|GTG|TTG<TAB>chosen<TAB>candidates.  --start-model reads such a file and chooses with its weights
(kg_start_weights_from) instead of training.  Every line of the ORF file gains the ORF's shift in codons as its last field, and
a moved ORF the flag word `moved`; the protein file and --select see the new extents.  The summary line gains
`, starts: own|model|untrained, moved: N`.  Without --starts every output is byte for byte what it was.

--db DB.kgsdb in place of -D calls genes by homology, without a signature table: every stop-to-stop run of the six frames with at
least --min-frag residues (default 30) is searched against the index of make_search_db on the GPU, and a fragment's best
--max-hits hits (default 1) are the CALLs (kg_contigs_search_translated; include/kmerguts_hip.h states the rule).  Exactly one
of -D and --db is given; -m, -M, -g and -O belong to the table scan and are errors beside --db.  A region's function is the
target's function where the index carries functions (make_search_db -A), targets of one function sharing it, and the target's
id otherwise; its score is a sum of alignment scores, so --min-score is then in alignment-score units.  The search takes
--min-shared, --max-cand, --max-db-per-kmer, --min-ratio, --align-ref, --gap-open, --gap-extend, --max-cells, --ungapped,
--min-ungapped and --band as search_proteins does, except that --align-ref defaults to `query`: a fragment is often a piece of a
gene, so it is the fragment that must be covered (this project's choice).  Contigs are searched in batches of at most --batch-nt
nucleotides (default: half the index's query room, since a batch's fragments hold at most two residues per nucleotide); a longer
contig is a batch of its own and the room is reserved for it.  Without --coding and --starts, which train per batch, no byte of
-o, --orfs, --faa and --shifts depends on where the batches are cut.  --hits FILE writes one line per hit record that became a
CALL:
    contig_id<TAB>left+1<TAB>right+1<TAB>strand<TAB>frame<TAB>fragment<TAB>rank<TAB>target<TAB>shared<TAB>score<TAB>ref<TAB>ratio
    <TAB>end in fragment<TAB>end in target<TAB>status[<TAB>function]
with left and right the aligned stretch in nucleotides, the fragment named contig_left+1_right+1_strand and the fields behind it
those of search_proteins -o.  Every other flag works as with -D: a gene whose halves hit one target in two frames is a
multi-frame region, and --repair joins it.  The summary line gains `, db: index (N targets), fragments: F, translated hits: H,
calls: C` (H: the records with status hit).  Without --db every byte of every output is as before.

-D KmerData --fill-db DB.kgsdb uses both sources in one run (include/kmerguts_hip.h, "signature and homology evidence in one run"):
every batch is scanned against the table (-m/-M/-g/-O), a stop-to-stop fragment that a table CALL touches is explained (the
touching CALLs' hits sum to --explain-min or more, default 1), only the other fragments are searched against the index (the --db
flags above, --min-frag, --max-hits, --batch-nt and --hits among them), homology CALLs of a score below --fill-min-score (default
0) are left out, and the regions are those of the two kinds of CALL merged.  function.index keeps its indices; a database function
whose name equals a table name takes the table's first index for it, the others are appended by first appearance, and a target
without a function is named by its id.  A region's score is the plain sum of its CALLs' counts, k-mer hits for a table CALL and
alignment score for a homology CALL: the two units are not brought to a common one.  Every regions line gains a last field,
`table`, `db` or `table+db` (GFF: the attribute evidence=), in front of what --select adds; --hits writes the homology CALLs; the
summary line gains `, fill: index (N targets), fragments: F, explained: E, searched: S, translated hits: H, db calls: C`.  A
batch holds at most the smaller of the scan's and the index's limit.  Without --fill-db every byte of every output is as before.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from .annotate import _data_file, parse_index
from .make_signatures import InputError, _read, parse_fasta


def summary_line(n: int, with_calls: int, n_regions: int, kept: int, multi: int) -> str:
    return "Contigs: %d, with calls: %d, regions: %d, kept: %d, multi-frame: %d" % (n, with_calls, n_regions, kept, multi)


def summary_of(regs, region_start) -> str:
    """The summary line of region records (REGION_DTYPE) and their region_start."""
    start = np.asarray(region_start)
    return summary_line(start.size - 1, int((start[1:] > start[:-1]).sum()), len(regs), int(regs["kept"].sum()),
                        int(((regs["frames"] & (regs["frames"] - 1)) != 0).sum()))


def _frames(bits: int) -> bytes:
    return b",".join(b"%d" % f for f in range(3) if bits >> f & 1)


def _fname(fnames, f: int) -> bytes:
    return fnames[f] if 0 <= f < len(fnames) else b"%d" % f


def _gff_escape(s: bytes) -> bytes:
    for ch in b"%;=&,\t":
        s = s.replace(bytes([ch]), b"%%%02X" % ch)
    return s


def select_summary(sel) -> str:
    """What the summary line gains with --select, from selection records (SELECTION_DTYPE)."""
    return ", selected: %d, overlapped: %d" % (int((sel["state"] == 1).sum()), int((sel["state"] == 2).sum()))


def _written(r, write_all: bool, sel, i: int) -> bool:
    return bool(write_all or (r["kept"] if sel is None else sel["state"][i] == 1))


def _winner(sel, i: int, cands) -> bytes:
    """`left+1..right+1:strand` of the candidate (a region or ORF record of cands) that candidate i lost to, or `-`."""
    by = int(sel["by"][i])
    if by < 0:
        return b"-"
    w = cands[by]
    return b"%d..%d:%s" % (w["left"] + 1, w["right"] + 1, b"-" if w["strand"] else b"+")


def format_regions(ids, regs, fnames, write_all: bool = False, gff: bool = False, sel=None, cands=None, evidence=None) -> bytes:
    """Region records (REGION_DTYPE, `seq` indexing ids) as text, in the order given.  sel: the selection records of --select,
    index-aligned with regs; cands: the records the selection ran on (the ORFs, default the regions); evidence (--fill-db): per
    region b"table", b"db" or b"table+db", a last field in front of what the selection adds (GFF: the attribute evidence=)."""
    lines = [b"##gff-version 3\n"] if gff else []
    cands = regs if cands is None else cands
    for i, r in enumerate(regs):
        if not _written(r, write_all, sel, i):
            continue
        status = b"kept" if r["kept"] else b"below"
        if sel is not None and sel["state"][i] == 2:
            status = b"overlapped"
        if evidence is not None:
            status += (b";evidence=" if gff else b"\t") + evidence[i]
        if sel is not None and write_all:
            status += (b";overlapped_by=" if gff else b"\t") + _winner(sel, i, cands)
        strand = b"-" if r["strand"] else b"+"
        name, w = _fname(fnames, int(r["fI"])), b"%.9g" % float(r["weighted"])
        cid = ids[int(r["seq"])]
        if gff:
            lines.append(b"%s\tkmerguts\tregion\t%d\t%d\t%d\t%s\t.\tName=%s;weighted=%s;n_calls=%d;frames=%s;status=%s\n" %
                         (cid, r["left"] + 1, r["right"] + 1, r["score"], strand, _gff_escape(name), w, r["n_calls"],
                          _gff_escape(_frames(int(r["frames"]))), status))
        else:
            lines.append(b"%s\t%d\t%d\t%s\t%s\t%d\t%s\t%d\t%s\t%s\n" % (cid, r["left"] + 1, r["right"] + 1, strand, name, r["score"], w,
                                                                    r["n_calls"], _frames(int(r["frames"])), status))
    return b"".join(lines)


START_NAMES = (b"ATG", b"GTG", b"TTG")
FLAG_WORDS = ((1, b"stop"), (2, b"partial5"), (4, b"interrupted"), (8, b"multi-frame"), (16, b"free"), (32, b"noncoding"), (64, b"moved"), (128, b"repaired"))
FREE_NAME = b"hypothetical protein"
NONCODING = 32
MOVED = 64
MODEL_HEADER = b"#kmerguts coding model 1"


def hexamer_text(h: int) -> bytes:
    """The six letters of hexamer index h, the first base most significant."""
    return bytes(b"ACGT"[(h >> (2 * (5 - i))) & 3] for i in range(6))


def format_coding_model(coding, background) -> bytes:
    """The text of --save-coding-model: the header line, then HEXAMER<TAB>coding<TAB>background in index order."""
    return MODEL_HEADER + b"\n" + b"".join(b"%s\t%d\t%d\n" % (hexamer_text(h), int(coding[h]), int(background[h])) for h in range(4096))


def parse_coding_model(text: bytes, where: str = "coding model"):
    """The counts of a --save-coding-model file -> (coding, background), int64[4096] each."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if not lines or lines[0].rstrip(b"\r") != MODEL_HEADER:
        raise InputError("%s: the first line is not `%s`" % (where, MODEL_HEADER.decode()))
    if len(lines) != 4097:
        raise InputError("%s: %d lines behind the header, 4096 expected" % (where, len(lines) - 1))
    out = np.zeros((2, 4096), dtype=np.int64)
    for h, line in enumerate(lines[1:]):
        f = line.rstrip(b"\r").split(b"\t")
        try:
            if len(f) != 3 or f[0] != hexamer_text(h):
                raise ValueError
            out[0, h], out[1, h] = int(f[1]), int(f[2])
        except (ValueError, OverflowError):
            raise InputError("%s, line %d: expected `%s<TAB>coding<TAB>background`" % (where, h + 2, hexamer_text(h).decode())) from None
    return out[0], out[1]


def coding_summary(trained, noncoding: int) -> str:
    """What the summary line gains with --coding: trained the kg_coding_stats.trained of every batch."""
    word = "model" if 2 in trained else "own" if 1 in trained else "untrained"
    return ", coding: %s, noncoding: %d" % (word, noncoding)


START_MODEL_HEADER = b"#kmerguts start model 1"


def format_start_model(chosen, cand, type_chosen, type_cand) -> bytes:
    """The text of --save-start-model: the header line, 80 lines position<TAB>base<TAB>chosen<TAB>candidates, 3 lines
    type<TAB>ATG|GTG|TTG<TAB>chosen<TAB>candidates."""
    lines = [START_MODEL_HEADER + b"\n"]
    for i in range(20):
        lines += [b"%d\t%s\t%d\t%d\n" % (i, b"ACGT"[c:c + 1], int(chosen[i][c]), int(cand[i][c])) for c in range(4)]
    lines += [b"type\t%s\t%d\t%d\n" % (START_NAMES[t - 1], int(type_chosen[t]), int(type_cand[t])) for t in (1, 2, 3)]
    return b"".join(lines)


def parse_start_model(text: bytes, where: str = "start model"):
    """The counts of a --save-start-model file -> (chosen int64[20][4], cand int64[20][4], type_chosen int64[4], type_cand
    int64[4])."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if not lines or lines[0].rstrip(b"\r") != START_MODEL_HEADER:
        raise InputError("%s: the first line is not `%s`" % (where, START_MODEL_HEADER.decode()))
    if len(lines) != 84:
        raise InputError("%s: %d lines behind the header, 83 expected" % (where, len(lines) - 1))
    chosen, cand = np.zeros((20, 4), dtype=np.int64), np.zeros((20, 4), dtype=np.int64)
    tchosen, tcand = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    for q, line in enumerate(lines[1:]):
        f = line.rstrip(b"\r").split(b"\t")
        want = (b"%d" % (q // 4), b"ACGT"[q % 4:q % 4 + 1]) if q < 80 else (b"type", START_NAMES[q - 80])
        try:
            if len(f) != 4 or (f[0], f[1]) != want:
                raise ValueError
            if q < 80:
                chosen[q // 4, q % 4], cand[q // 4, q % 4] = int(f[2]), int(f[3])
            else:
                tchosen[q - 79], tcand[q - 79] = int(f[2]), int(f[3])
        except (ValueError, OverflowError):
            raise InputError("%s, line %d: expected `%s<TAB>%s<TAB>chosen<TAB>candidates`" %
                             (where, q + 2, want[0].decode(), want[1].decode())) from None
    return chosen, cand, tchosen, tcand


def starts_summary(trained, moved: int) -> str:
    """What the summary line gains with --starts: trained the kg_start_stats.trained of every batch."""
    word = "model" if 2 in trained else "own" if 1 in trained else "untrained"
    return ", starts: %s, moved: %d" % (word, moved)


def parse_start_codons(text: str) -> int:
    """`ATG,GTG,TTG` -> the start_codons mask (1 ATG, 2 GTG, 4 TTG); `none` or an empty text -> 0."""
    mask = 0
    for word in text.split(","):
        w = word.strip().upper().encode()
        if not w or w == b"NONE":
            continue
        if w not in START_NAMES:
            raise ValueError("--start-codons: %r is none of ATG, GTG, TTG" % word)
        mask |= 1 << START_NAMES.index(w)
    return mask


def orf_summary(orfs) -> str:
    """What the summary line gains with --orfs / --faa, from ORF records (ORF_DTYPE)."""
    fl = orfs["flags"]
    complete = ((fl & 1) != 0) & (orfs["start_codon"] != 0) & ((fl & 4) == 0)
    return ", orfs: %d, complete: %d, interrupted: %d" % (len(orfs), int(complete.sum()), int(((fl & 4) != 0).sum()))


def _orf_line(ids, o, name: bytes) -> bytes:
    words = b",".join(w for bit, w in FLAG_WORDS if int(o["flags"]) & bit) or b"-"
    start = START_NAMES[int(o["start_codon"]) - 1] if o["start_codon"] else b"-"
    return b"%s\t%d\t%d\t%s\t%d\t%s\t%d\t%d\t%s\t%s" % (ids[int(o["seq"])], o["left"] + 1, o["right"] + 1, b"-" if o["strand"] else b"+",
                                                        o["frame"], name, o["score"], o["n_res"], start, words)


def _by_contig(first, second) -> list:
    """Two lists of (contig, text), each in contig order -> the texts contig by contig, the first list's in front."""
    return [x[2] for x in sorted([(c, 0, t) for c, t in first] + [(c, 1, t) for c, t in second], key=lambda x: x[:2])]


def format_orfs(ids, regs, orfs, fnames, write_all: bool = False, sel=None, free=None, free_sel=None, cands=None, coding=None,
                free_coding=None, shifts=None, free_shifts=None) -> bytes:
    """ORF records (ORF_DTYPE, index-aligned with regs) as text, one line per written region.  free: the free ORFs of
    --free-orfs, written behind their contig's lines; free_sel: their selection records; cands: the records the selection ran on
    (the winners of --all are named from them); coding, free_coding: the coding scores of --coding, each line's last field;
    shifts, free_shifts: the shifts of --starts, the last field behind the score."""
    lines = []
    for i, (r, o) in enumerate(zip(regs, orfs)):
        if not _written(r, write_all, sel, i):
            continue
        tail = b"" if coding is None else b"\t%d" % int(coding[i])
        if shifts is not None:
            tail += b"\t%d" % int(shifts[i])
        lines.append((int(o["seq"]), _orf_line(ids, o, _fname(fnames, int(o["fI"]))) + tail + b"\n"))
    if free is None:
        return b"".join(t for _, t in lines)
    flines = []
    for i, o in enumerate(free):
        noncoding = int(o["flags"]) & NONCODING != 0
        if not (write_all or ((free_sel is None or free_sel["state"][i] == 1) and not noncoding)):
            continue
        tail = b""
        if free_sel is not None and write_all:
            status = b"noncoding" if noncoding else b"overlapped" if free_sel["state"][i] == 2 else b"kept"
            tail = b"\t%s\t%s" % (status, _winner(free_sel, i, cands))
        if free_coding is not None:
            tail += b"\t%d" % int(free_coding[i])
        if free_shifts is not None:
            tail += b"\t%d" % int(free_shifts[i])
        flines.append((int(o["seq"]), _orf_line(ids, o, FREE_NAME) + tail + b"\n"))
    return b"".join(_by_contig(lines, flines))


def repair_summary(repaired: int, candidates: int) -> str:
    """What the summary line gains with --repair."""
    return ", repaired: %d, unrepaired: %d" % (repaired, candidates - repaired)


def format_shifts(ids, regs, orfs, fnames, junctions, write_all: bool = False, sel=None) -> bytes:
    """The junction records of --repair (JUNCTION_DTYPE, `orf` indexing orfs) as text: one line per junction of a written ORF."""
    lines = []
    for j in junctions:
        i = int(j["orf"])
        if not _written(regs[i], write_all, sel, i):
            continue
        o = orfs[i]
        lines.append(b"%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\n" % (ids[int(o["seq"])], o["left"] + 1, o["right"] + 1, b"-" if o["strand"] else b"+",
                                                                     _fname(fnames, int(o["fI"])), j["pos"] + 1, j["from_frame"], j["to_frame"],
                                                                     j["res"] + 1, j["gap"]))
    return b"".join(lines)


def _fasta(ids, key, name: bytes, p: bytes) -> bytes:
    head = b">%s_%d_%d_%s %s\n" % (ids[key[0]], key[2] + 1, key[3] + 1, b"-" if key[1] else b"+", name)
    return head + b"".join(p[k:k + 60] + b"\n" for k in range(0, len(p), 60))


def format_faa(ids, regs, orfs, prot_start, residues, fnames, write_all: bool = False, sel=None, free=None, free_sel=None,
               free_prot_start=None, free_residues=None) -> bytes:
    """The proteins of the written regions as FASTA: an ORF with the (contig, strand, left, right) of an earlier written one is
    written once, where the first of them stands, under the region with the largest score (ties: the first).  free, free_sel,
    free_prot_start, free_residues: the free ORFs of --free-orfs, written behind their contig's proteins unless their extent is
    there already."""
    res = np.asarray(residues, dtype=np.uint8).tobytes()
    best, order = {}, []
    for i, (r, o) in enumerate(zip(regs, orfs)):
        if not _written(r, write_all, sel, i) or prot_start[i + 1] == prot_start[i]:
            continue
        key = (int(o["seq"]), int(o["strand"]), int(o["left"]), int(o["right"]))
        if key not in best:
            best[key] = i
            order.append(key)
        elif o["score"] > orfs[best[key]]["score"]:
            best[key] = i
    out = []
    for key in order:
        i = best[key]
        out.append((key[0], _fasta(ids, key, _fname(fnames, int(orfs[i]["fI"])), res[int(prot_start[i]):int(prot_start[i + 1])])))
    if free is None:
        return b"".join(t for _, t in out)
    fres = np.asarray(free_residues, dtype=np.uint8).tobytes()
    fout = []
    for i, o in enumerate(free):
        key = (int(o["seq"]), int(o["strand"]), int(o["left"]), int(o["right"]))
        written = write_all or ((free_sel is None or free_sel["state"][i] == 1) and int(o["flags"]) & NONCODING == 0)
        if not written or key in best:
            continue
        best[key] = -1
        fout.append((key[0], _fasta(ids, key, FREE_NAME, fres[int(free_prot_start[i]):int(free_prot_start[i + 1])])))
    return b"".join(_by_contig(out, fout))


def function_names(dids, functions):
    """What --db names its regions by: the targets' functions where the index carries them, else their ids.
    -> (fnames, target_fn): target_fn[d] indexes fnames; targets of one function share an index, numbered by first appearance."""
    fnames, index_of = [], {}
    target_fn = np.zeros(len(dids), dtype=np.int32)
    for d, did in enumerate(dids):
        name = functions[did][0] if functions is not None and did in functions else did
        if name not in index_of:
            index_of[name] = len(fnames)
            fnames.append(name)
        target_fn[d] = index_of[name]
    return fnames, target_fn


def fill_function_names(table_fnames, dids, functions):
    """What --fill-db names its regions by: function.index keeps its indices; a database function whose name equals a table name
    takes the table's first index for it, the others are appended by first appearance (as merge_tables does), and a target
    without a function is named by its id.  -> (fnames, target_fn)."""
    fnames = list(table_fnames)
    index_of = {}
    for f, name in enumerate(fnames):
        index_of.setdefault(name, f)
    target_fn = np.zeros(len(dids), dtype=np.int32)
    for d, did in enumerate(dids):
        name = functions[did][0] if functions is not None and did in functions else did
        if name not in index_of:
            index_of[name] = len(fnames)
            fnames.append(name)
        target_fn[d] = index_of[name]
    return fnames, target_fn


def region_evidence(regs, calls, call_kind, off):
    """The `evidence` field of a batch's regions (REGION_DTYPE, seq within the batch) from the merged CALLs and their kinds: a CALL
    belongs to the region of its (seq, strand, fI) group that contains its x0.  -> a list of b"table", b"db" or b"table+db"."""
    groups = {}
    for i, r in enumerate(regs):
        groups.setdefault((int(r["seq"]), int(r["strand"]), int(r["fI"])), []).append((int(r["left"]), int(r["right"]), i))
    seen = [0] * len(regs)
    for c, kind in zip(calls, call_kind):
        cont = int(c["container"])
        s, strand, frame = cont // 6, cont % 6 // 3, cont % 3
        x0 = frame + 3 * int(c["start"])
        pos = x0 if strand == 0 else int(off[s + 1] - off[s]) - 1 - x0
        for left, right, i in groups.get((s, strand, int(c["fI"])), ()):
            if left <= pos <= right:
                seen[i] |= 2 if kind else 1
                break
    return [(b"table", b"table", b"db", b"table+db")[k] for k in seen]


def format_call_hits(ids, dids, ev, off, align_ref: str = "longer", functions=None) -> bytes:
    """--hits: one line per CALL of an evidence (hotpath.Evidence; ids: the batch's contig ids; off: its offsets): the contig, the
    aligned stretch left+1 and right+1 in nucleotides, strand and frame, then the fields of search_proteins -o for the hit record,
    the fragment named contig_left+1_right+1_strand as --faa names a protein.  Of a merged list (--fill-db) the homology CALLs are
    written, whose hit records name the searched fragments."""
    from .search_proteins import STATUS, _ref
    hits, frags = ev.search[0], getattr(ev, "searched_fragments", ev.fragments)[0]
    out = []
    for c, r in zip(ev.calls, ev.call_hits):
        if int(r) < 0:
            continue
        h = hits[int(r)]
        fr = frags[int(h["query"])]
        s, strand, frame = int(c["container"]) // 6, int(c["container"]) % 6 // 3, int(c["container"]) % 3
        L = int(off[s + 1] - off[s])
        x0, x1 = frame + 3 * int(c["start"]), frame + 3 * int(c["end"]) + 2
        left, right = (x0, x1) if strand == 0 else (L - 1 - x1, L - 1 - x0)
        sign = b"-" if strand else b"+"
        ref, score, did = _ref(h, align_ref), int(h["score"]), dids[int(h["target"])]
        line = b"%s\t%d\t%d\t%s\t%d\t%s_%d_%d_%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s" % (
            ids[s], left + 1, right + 1, sign, frame, ids[s], int(fr["left"]) + 1, int(fr["right"]) + 1, sign, int(h["rank"]), did,
            int(h["shared"]), score, ref, 100 * score // ref if ref > 0 else 0, int(h["end_query"]) + 1, int(h["end_target"]) + 1,
            STATUS[int(h["status"])])
        if functions is not None:
            line += b"\t" + (functions[did][0] if did in functions else b"-")
        out.append(line + b"\n")
    return b"".join(out)


def call_regions(data_dir: str, contigs: str, out: str, min_hits: int = 5, min_weighted_hits: int = 0, max_gap: int = 200,
                 order_constraint: bool = False, merge_gap: int = 600, min_score: int = 0, min_len: int = 0,
                 write_all: bool = False, gff: bool = False, device: int = 0, orfs_out: str = None, faa_out: str = None,
                 start_codons: int = 7, select: bool = False, max_overlap: int = 60, max_overlap_pct: int = 50,
                 free_min_res: int = None, coding: bool = False, min_coding: int = 0, min_train: int = 100000,
                 coding_model_in: str = None, save_coding_model: str = None, starts: bool = False, start_rounds: int = 4,
                 min_train_starts: int = 200, start_model_in: str = None, save_start_model: str = None, repair: bool = False,
                 repair_min_count: int = 0, max_junctions: int = 4, shifts_out: str = None, db: str = None, min_frag: int = 30,
                 max_hits: int = 1, batch_nt: int = None, hits_out: str = None, search: dict = None, open_db=None, fill_db: str = None,
                 explain_min: int = 1, fill_min_score: int = 0, open_table=None) -> str:
    """Write the regions (and, with orfs_out / faa_out, their open reading frames and proteins; with free_min_res also the
    evidence-free ORFs of at least that many residues; with coding the ORFs' coding scores, the non-coding free ORFs dropped;
    with starts the start codons chosen by the start-site score; with repair the multi-frame regions' ORFs joined across their
    frames first, and their junctions written to shifts_out); returns the summary line.
    db: in place of data_dir, the index file of make_search_db: the CALLs are translated search hits (SearchDb.search_contigs with
    min_frag, max_hits and the keywords of `search`), batches hold at most batch_nt nucleotides and hits_out gets one line per
    CALL.  open_db replaces hotpath.SearchDb.open (tests).
    fill_db: beside data_dir, the index file whose targets fill what the table left unnamed: every batch is scanned, the fragments
    its CALLs do not explain (explain_min) are searched (SearchDb.search_contigs with explained_by), homology CALLs of a score
    below fill_min_score are left out, and the regions are those of the merged CALLs, each with an `evidence` field.
    open_table(path, device) replaces the resident table (tests)."""
    if fill_db is not None and db is not None:
        raise ValueError("--fill-db beside --db: --db searches every fragment, --fill-db only what the table of -D left unnamed")
    if fill_db is not None and data_dir is None:
        raise ValueError("--fill-db needs -D: it fills the unnamed stretches of a table scan")
    if (data_dir is None) == (db is None):
        raise ValueError("exactly one of -D and --db must be given")
    if db is None and fill_db is None and hits_out is not None:
        raise ValueError("--hits needs --db")
    if fill_db is None and (explain_min != 1 or fill_min_score != 0):
        raise ValueError("--explain-min and --fill-min-score need --fill-db")
    if explain_min < 1:
        raise ValueError("--explain-min must be >= 1")
    if fill_min_score < 0:
        raise ValueError("--fill-min-score must be >= 0")
    want_orfs = orfs_out is not None or faa_out is not None
    if free_min_res is not None and not want_orfs:
        raise ValueError("--free-orfs needs --orfs or --faa: free ORFs are written to those files only")
    if coding and not want_orfs:
        raise ValueError("--coding needs --orfs or --faa: the scores are the ORFs'")
    if (coding_model_in is not None or save_coding_model is not None) and not coding:
        raise ValueError("--coding-model and --save-coding-model need --coding")
    if repair and not want_orfs:
        raise ValueError("--repair needs --orfs or --faa: it rewrites ORFs")
    if shifts_out is not None and not repair:
        raise ValueError("--shifts needs --repair")
    if starts and not coding:
        raise ValueError("--starts needs --coding: the start-site score's coding half is the coding step's table")
    if (start_model_in is not None or save_start_model is not None) and not starts:
        raise ValueError("--start-model and --save-start-model need --starts")
    from . import hotpath
    from .kmer_guts_java import KmerGutsJava, _resident_table
    ids, seqs = parse_fasta(_read(contigs), contigs)
    index = None
    if db is None:
        table_path = _data_file(data_dir, "kmer.table.mem_map")
        fn_path = _data_file(data_dir, "function.index")
        if table_path is None or fn_path is None:
            raise FileNotFoundError("%s holds no kmer.table.mem_map[.gz] or function.index[.gz]" % data_dir)
        fnames = parse_index(_read(fn_path), fn_path)
        tab = (open_table or _resident_table)(table_path, device)
        params = hotpath.Params(aa=False, order_constraint=order_constraint, min_hits=min_hits, min_weighted_hits=min_weighted_hits,
                                max_gap=max_gap)
        batch_limit = KmerGutsJava.MAX_BATCH_CHARS

        def scan(batch, off, k):
            return tab.scan(batch, off, params)
        if fill_db is not None:
            index = (open_db or hotpath.SearchDb.open)(fill_db, device=device)
    else:
        index = (open_db or hotpath.SearchDb.open)(db, device=device)
    note = None
    try:
        if fill_db is not None:
            from .make_search_db import unpack_names
            info = index.info()
            dids, functions = unpack_names(index.names(), int(info["targets"]))
            fnames, target_fn = fill_function_names(fnames, dids, functions)
            room = [int(info["query_room"])]
            batch_limit = min(batch_limit, max(room[0] // 2, 1) if batch_nt is None else int(batch_nt))
            skw = dict(search or {})
            if skw.get("align", {}).get("ref") == "query":
                skw["align"] = dict(skw["align"], ref="member")
            ev_sum = dict(fragments=0, explained=0, searched=0, hits=0, calls=0)
            hit_lines = []
            scan_table = scan

            def scan(batch, off, k):        # noqa: F811
                # a fill batch reserves the unfiltered bound, 2 * nucleotides, as the --db path does
                if 2 * len(batch) > room[0]:
                    index.reserve(2 * len(batch))
                    room[0] = 2 * len(batch)
                with scan_table(batch, off, k) as r:
                    ev = index.search_contigs(batch, off, min_res=min_frag, max_hits=max_hits, target_fn=target_fn, explained_by=r,
                                              explain_min=explain_min, min_db_count=fill_min_score, **skw)
                rs = ev.residual_stats
                ev_sum["fragments"] += ev.stats["fragments"]
                ev_sum["explained"] += rs["explained"]
                ev_sum["searched"] += rs["searched"]
                ev_sum["hits"] += ev.search[3]["hits"]
                ev_sum["calls"] += rs["db_calls"] - rs["dropped_min_count"]
                if hits_out is not None:
                    hit_lines.append(format_call_hits(ids[k:], dids, ev, off, skw.get("align", {}).get("ref", "longer"), functions))
                return ev

            def note(ev, regs, off):
                return region_evidence(regs, ev.calls, ev.call_kind, off)
        elif index is not None:
            from .make_search_db import unpack_names
            info = index.info()
            dids, functions = unpack_names(index.names(), int(info["targets"]))
            fnames, target_fn = function_names(dids, functions)
            room = [int(info["query_room"])]
            batch_limit = max(room[0] // 2, 1) if batch_nt is None else int(batch_nt)
            skw = dict(search or {})
            if skw.get("align", {}).get("ref") == "query":
                skw["align"] = dict(skw["align"], ref="member")
            ev_sum = dict(fragments=0, hits=0, calls=0)
            hit_lines = []

            def scan(batch, off, k):
                # 2 * nucleotides bounds the fragments' residues: a batch over half the room has the room reserved for it
                if 2 * len(batch) > room[0]:
                    index.reserve(2 * len(batch))
                    room[0] = 2 * len(batch)
                ev = index.search_contigs(batch, off, min_res=min_frag, max_hits=max_hits, target_fn=target_fn, **skw)
                ev_sum["fragments"] += ev.stats["fragments"]
                ev_sum["hits"] += ev.search[3]["hits"]
                ev_sum["calls"] += ev.stats["calls"]
                if hits_out is not None:
                    hit_lines.append(format_call_hits(ids[k:], dids, ev, off, skw.get("align", {}).get("ref", "longer"), functions))
                return ev
        line = _call_regions(ids, seqs, scan, batch_limit, fnames, out, merge_gap, min_score, min_len, write_all, gff, orfs_out, faa_out,
                             start_codons, select, max_overlap, max_overlap_pct, free_min_res, coding, min_coding, min_train,
                             coding_model_in, save_coding_model, starts, start_rounds, min_train_starts, start_model_in,
                             save_start_model, repair, repair_min_count, max_junctions, shifts_out, note)
        if index is not None and hits_out is not None:
            with open(hits_out, "wb") as f:
                f.write(b"".join(hit_lines))
        if fill_db is not None:
            line += ", fill: index (%d targets), fragments: %d, explained: %d, searched: %d, translated hits: %d, db calls: %d" % (
                int(info["targets"]), ev_sum["fragments"], ev_sum["explained"], ev_sum["searched"], ev_sum["hits"], ev_sum["calls"])
        elif index is not None:
            line += ", db: index (%d targets), fragments: %d, translated hits: %d, calls: %d" % (
                int(info["targets"]), ev_sum["fragments"], ev_sum["hits"], ev_sum["calls"])
        return line
    finally:
        if index is not None:
            index.close()


def _call_regions(ids, seqs, scan, batch_limit, fnames, out, merge_gap, min_score, min_len, write_all, gff, orfs_out, faa_out, start_codons,
                  select, max_overlap, max_overlap_pct, free_min_res, coding, min_coding, min_train, coding_model_in, save_coding_model,
                  starts, start_rounds, min_train_starts, start_model_in, save_start_model, repair, repair_min_count, max_junctions,
                  shifts_out, note=None) -> str:
    """call_regions behind its source of CALLs: scan(batch, off) gives what holds a batch's CALLs (a ScanResult or an Evidence:
    regions(), orfs() and select() with the same arguments; k: the batch's first contig), batch_limit the characters a batch holds at most.
    note(r, regs, off): the `evidence` field of a batch's regions (--fill-db), or None."""
    from . import hotpath
    want_orfs = orfs_out is not None or faa_out is not None
    coding_arg = None                   # what ScanResult.orfs / select take: None, True (own training) or a score table
    if coding:
        coding_arg = True
        if coding_model_in is not None:
            coding_arg = hotpath.coding_table(*parse_coding_model(_read(coding_model_in), coding_model_in))
    ckw = {"coding": coding_arg, "min_coding": min_coding, "min_train_pairs": min_train} if coding else {}
    if starts:
        starts_arg = True                                       # ... and their starts=: True or a weights pair
        if start_model_in is not None:
            starts_arg = hotpath.start_weights(*parse_start_model(_read(start_model_in), start_model_in))
        ckw.update(starts=starts_arg, start_min_res=100 if free_min_res is None else free_min_res, start_rounds=start_rounds,
                   min_train_starts=min_train_starts)
    if repair:
        ckw.update(repair=True, repair_min_count=repair_min_count, max_junctions=max_junctions)
    jparts, n_repaired, n_candidates = [], 0, 0                 # the junction records, `orf` counted over all batches
    shparts, fshparts, strained = [], [], []                    # the shifts, and every batch's kg_start_stats.trained
    start_sum = [np.zeros((20, 4), np.int64), np.zeros((20, 4), np.int64), np.zeros(4, np.int64), np.zeros(4, np.int64)]
    cparts, fcparts, trained = [], [], []                       # the coding scores, and every batch's kg_coding_stats.trained
    model_sum = np.zeros((2, 4096), dtype=np.int64)
    parts, rstarts = [], [np.zeros(1, dtype=np.int64)]
    oparts, lens, residues, sparts = [], [], [], []
    fparts, flens, fresidues, fsparts = [], [], [], []          # the free ORFs, and per batch (selection, first free record)
    notes = []
    k = n_before = n_free = 0
    while k < len(ids):
        j, size = k, 0
        while j < len(ids) and (j == k or size + len(seqs[j]) <= batch_limit):
            size += len(seqs[j])
            j += 1
        off = np.zeros(j - k + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs[k:j]])
        batch = b"".join(seqs[k:j])
        with scan(batch, off, k) as r:
            if select:
                got = r.select(off, batch, merge_gap, min_score, min_len, want_orfs, start_codons, not write_all,
                               max_overlap=max_overlap, max_overlap_pct=max_overlap_pct, free_min_res=free_min_res, **ckw)
                regs, start, sel = got[0], got[1], got[-1]
                # (selection is per contig: a batch's winners are its own records; a free winner is marked by -2 - its index
                # among all free ORFs until the regions of every batch are counted)
                by, nr = sel["by"], len(regs)
                by[by >= nr] = -2 - (by[by >= nr] - nr + n_free)
                by[by >= 0] += n_before
                sparts.append(sel[:nr])
                fsparts.append(sel[nr:])
                if want_orfs:
                    orfs, pstart, res = got[2:5]
            elif want_orfs:
                regs, start, orfs, pstart, res = r.orfs(batch, off, merge_gap, min_score, min_len, start_codons, not write_all,
                                                        free_min_res=free_min_res, **ckw)
            if want_orfs:
                nr = len(regs)                              # the regions' ORFs, then the batch's free ones
                orfs["seq"] += k
                oparts.append(orfs[:nr])
                lens.append(np.diff(pstart[:nr + 1]))
                residues.append(res[:pstart[nr]])
                fparts.append(orfs[nr:])
                flens.append(np.diff(pstart[nr:]))
                fresidues.append(res[pstart[nr]:])
                n_free += len(orfs) - nr
                if repair:
                    junc = r.junctions.copy()
                    junc["orf"] += n_before
                    jparts.append(junc)
                    n_repaired += r.repair_stats["repaired"]
                    n_candidates += r.repair_stats["candidates"]
                if coding:
                    cparts.append(r.coding_scores[:nr])
                    fcparts.append(r.coding_scores[nr:])
                    trained.append(r.coding_stats["trained"])
                    model_sum += np.stack(r.coding_model)
                    if r.coding_stats["trained"] == 0:
                        print("Warning: contigs %d..%d: %d codon pairs in evidence ORFs, fewer than --min-train %d: no coding model, "
                              "no ORF scored" % (k + 1, j, r.coding_stats["training_pairs"], min_train), file=sys.stderr)
                if starts:
                    shparts.append(r.start_shifts[:nr])
                    fshparts.append(r.start_shifts[nr:])
                    strained.append(r.start_stats["trained"])
                    for total, part in zip(start_sum, r.start_model):
                        total += part
                    if r.start_stats["trained"] == 0:
                        print("Warning: contigs %d..%d: %d evidence ORFs to train the start model on, fewer than --min-train-starts %d, "
                              "or no coding model: no start moved" % (k + 1, j, r.start_stats["training_records"], min_train_starts),
                              file=sys.stderr)
            else:
                regs, start = r.regions(off, merge_gap, min_score, min_len)
            if note is not None:
                notes += note(r, regs, off)
        regs["seq"] += k
        n_before += len(regs)
        parts.append(regs)
        rstarts.append(start[1:] + rstarts[-1][-1])
        k = j
    regs = np.concatenate(parts) if parts else np.zeros(0, dtype=hotpath.N.REGION_DTYPE)
    sel = None
    if select:
        sel = np.concatenate(sparts) if sparts else np.zeros(0, dtype=hotpath.N.SELECTION_DTYPE)
    orfs = free = free_sel = cands = None
    if want_orfs:
        orfs = cands = np.concatenate(oparts) if oparts else np.zeros(0, dtype=hotpath.N.ORF_DTYPE)
    if free_min_res is not None:
        free = np.concatenate(fparts) if fparts else np.zeros(0, dtype=hotpath.N.ORF_DTYPE)
        cands = np.concatenate([orfs, free])
        if select:
            free_sel = np.concatenate(fsparts) if fsparts else np.zeros(0, dtype=hotpath.N.SELECTION_DTYPE)
            for part in (sel, free_sel):
                by = part["by"]
                by[by <= -2] = len(orfs) + (-2 - by[by <= -2])
    with open(out, "wb") as f:
        f.write(format_regions(ids, regs, fnames, write_all, gff, sel, cands, notes if note is not None else None))
    line = summary_of(regs, np.concatenate(rstarts))
    if want_orfs:
        pstart = np.zeros(len(orfs) + 1, dtype=np.int64)
        if lens:
            np.cumsum(np.concatenate(lens), out=pstart[1:])
        fstart = None
        if free is not None:
            fstart = np.zeros(len(free) + 1, dtype=np.int64)
            if flens:
                np.cumsum(np.concatenate(flens), out=fstart[1:])
        scores = fscores = None
        if coding:
            scores = np.concatenate(cparts) if cparts else np.zeros(0, np.int64)
            fscores = np.concatenate(fcparts) if fcparts and free is not None else None
        shifts = fshifts = None
        if starts:
            shifts = np.concatenate(shparts) if shparts else np.zeros(0, np.int32)
            fshifts = np.concatenate(fshparts) if fshparts and free is not None else None
        if orfs_out is not None:
            with open(orfs_out, "wb") as f:
                f.write(format_orfs(ids, regs, orfs, fnames, write_all, sel, free, free_sel, cands, scores, fscores, shifts, fshifts))
        if faa_out is not None:
            with open(faa_out, "wb") as f:
                f.write(format_faa(ids, regs, orfs, pstart, np.concatenate(residues) if residues else np.zeros(0, np.uint8),
                                   fnames, write_all, sel, free, free_sel, fstart,
                                   np.concatenate(fresidues) if fresidues else np.zeros(0, np.uint8)))
        line += orf_summary(orfs)
        if repair:
            line += repair_summary(n_repaired, n_candidates)
            if shifts_out is not None:
                with open(shifts_out, "wb") as f:
                    f.write(format_shifts(ids, regs, orfs, fnames, np.concatenate(jparts) if jparts else np.zeros(0, hotpath.N.JUNCTION_DTYPE),
                                          write_all, sel))
    if select:
        line += select_summary(sel if free_sel is None else np.concatenate([sel, free_sel]))
    if free is not None:
        line += ", free: %d" % len(free)
    if coding:
        line += coding_summary(trained, 0 if free is None else int(((free["flags"] & NONCODING) != 0).sum()))
        if save_coding_model is not None:
            with open(save_coding_model, "wb") as f:
                f.write(format_coding_model(model_sum[0], model_sum[1]))
    if starts:
        moved = int(((orfs["flags"] & MOVED) != 0).sum()) + (0 if free is None else int(((free["flags"] & MOVED) != 0).sum()))
        line += starts_summary(strained, moved)
        if save_start_model is not None:
            with open(save_start_model, "wb") as f:
                f.write(format_start_model(*start_sum))
    return line


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.call_regions",
                                 description="Merge the CALLs of a DNA scan into function regions on the contigs, on the GPU.")
    ap.add_argument("-D", default=None, metavar="DATADIR", help="data directory (kmer.table.mem_map[.gz], function.index[.gz])")
    ap.add_argument("--db", default=None, metavar="DB.kgsdb",
                    help="in place of -D: the index file make_search_db wrote; the CALLs are the hits of a translated search against it")
    ap.add_argument("-q", required=True, metavar="CONTIGS", help="contig FASTA (.gz allowed)")
    ap.add_argument("-o", required=True, metavar="OUT", help="regions TSV (or GFF3) to write")
    ap.add_argument("-m", type=int, default=None, help="minHits (default 5)")
    ap.add_argument("-M", type=int, default=None, help="minWeightedHits (default 0)")
    ap.add_argument("-g", type=int, default=None, help="maxGap (default 200)")
    ap.add_argument("-O", action="store_true", help="order constraint")
    ap.add_argument("--merge-gap", type=int, default=600, help="nucleotides two CALLs of one function may lie apart (default 600, this project's choice)")
    ap.add_argument("--min-score", type=int, default=0, help="a region is kept with score >= this (default 0); with --db the score is in alignment-score units")
    ap.add_argument("--min-len", type=int, default=0, help="... and at least this many nucleotides long (default 0)")
    ap.add_argument("--all", action="store_true", help="write every region, not only the kept ones")
    ap.add_argument("--gff", action="store_true", help="write GFF3 instead of TSV")
    ap.add_argument("--orfs", metavar="ORFS.tsv", help="also write the open reading frame around every written region")
    ap.add_argument("--faa", metavar="PROTEINS.faa", help="also write the translated proteins (FASTA, for annotate -p / make_signatures -p)")
    ap.add_argument("--start-codons", default="ATG,GTG,TTG", help="start codons of the ORF extension (default ATG,GTG,TTG; none: no start search)")
    ap.add_argument("--repair", action="store_true",
                    help="with --orfs / --faa: join the frames of every kept multi-frame region into one ORF and protein (frameshift repair)")
    ap.add_argument("--repair-min-count", type=int, default=0, help="CALLs with fewer hits take no part in a chain (default 0, this project's choice)")
    ap.add_argument("--max-junctions", type=int, default=4, help="frame changes a repaired region has at most (default 4, this project's choice; 1..8)")
    ap.add_argument("--shifts", metavar="SHIFTS.tsv", help="with --repair: write the junctions of the repaired ORFs")
    ap.add_argument("--select", action="store_true", help="write a gene set: only the non-overlapping selection among the kept candidates")
    ap.add_argument("--max-overlap", type=int, default=60, help="nucleotides two selected candidates may share (default 60, this project's choice)")
    ap.add_argument("--max-overlap-pct", type=int, default=50, help="... and percent of the shorter one (default 50)")
    ap.add_argument("--free-orfs", action="store_true", help="with --orfs / --faa: also write the evidence-free ORFs (hypothetical protein)")
    ap.add_argument("--min-res", type=int, default=100, help="residues a free ORF has at least (default 100, this project's choice)")
    ap.add_argument("--coding", action="store_true",
                    help="with --orfs / --faa: score every ORF by in-frame hexamer log-odds and drop the non-coding free ORFs; without "
                         "--coding-model each batch (1.5e9 characters: one model for nearly every input) trains on its own evidence ORFs")
    ap.add_argument("--min-coding", type=int, default=0, help="a free ORF is dropped with a coding score below this (default 0, this project's choice)")
    ap.add_argument("--min-train", type=int, default=100000,
                    help="codon pairs of evidence ORFs a batch needs to train (default 100000, this project's choice); below: untrained, nothing dropped")
    ap.add_argument("--coding-model", metavar="IN", help="score with the counts of this file (--save-coding-model of a relative) instead of training")
    ap.add_argument("--save-coding-model", metavar="OUT", help="write the coding and background hexamer counts, summed over the batches")
    ap.add_argument("--starts", action="store_true",
                    help="with --coding: choose every complete ORF's start codon by a start-site score trained on the batch's evidence ORFs")
    ap.add_argument("--start-rounds", type=int, default=4, help="training rounds of --starts (default 4, this project's choice; 1..16)")
    ap.add_argument("--min-train-starts", type=int, default=200,
                    help="evidence ORFs a batch needs to train the start model (default 200, this project's choice); below: untrained, nothing moved")
    ap.add_argument("--start-model", metavar="IN", help="choose with the counts of this file (--save-start-model of a relative) instead of training")
    ap.add_argument("--save-start-model", metavar="OUT", help="write the start model's counts of the last round, summed over the batches")
    ap.add_argument("--fill-db", default=None, metavar="DB.kgsdb",
                    help="beside -D: the index file make_search_db wrote; the fragments the table's CALLs do not explain are searched against "
                         "it and both kinds of CALL make the regions (the --db flags below govern the search)")
    ap.add_argument("--explain-min", type=int, default=None, metavar="N",
                    help="with --fill-db: a fragment is explained when the hits of the table CALLs that touch it sum to N or more "
                         "(default 1, this project's choice, not tuned)")
    ap.add_argument("--fill-min-score", type=int, default=None, metavar="N",
                    help="with --fill-db: a homology CALL with an alignment score below N is left out (default 0)")
    ap.add_argument("--min-frag", type=int, default=None, metavar="N",
                    help="with --db: residues a stop-to-stop fragment has at least to be searched (default 30, this project's choice, not tuned)")
    ap.add_argument("--max-hits", type=int, default=None, metavar="N",
                    help="with --db: hits of a fragment that become CALLs, 1..64 (default 1, this project's choice)")
    ap.add_argument("--batch-nt", type=int, default=None, metavar="N",
                    help="with --db: contigs are searched in batches of at most N nucleotides (default: half the index's query room); a longer "
                         "contig is a batch of its own")
    ap.add_argument("--hits", default=None, metavar="FILE", help="with --db: write one line per hit record that became a CALL")
    ap.add_argument("--min-shared", type=int, default=None, help="with --db: as in search_proteins (default 2)")
    ap.add_argument("--max-cand", type=int, default=None, help="with --db: as in search_proteins (default 8)")
    ap.add_argument("--max-db-per-kmer", type=int, default=None, help="with --db: as in search_proteins (default 256)")
    ap.add_argument("--min-ratio", type=int, default=None, help="with --db: a hit needs 100 * score >= this * ref (default 50)")
    ap.add_argument("--align-ref", choices=("longer", "query"), default=None,
                    help="with --db: ref is the fragment's self-score (query, the default here: a fragment is often a piece of a gene, so "
                         "it is the fragment that must be covered; this project's choice) or the larger of the two (longer)")
    ap.add_argument("--gap-open", type=int, default=None, help="with --db: as in search_proteins (default 11)")
    ap.add_argument("--gap-extend", type=int, default=None, help="with --db: as in search_proteins (default 1)")
    ap.add_argument("--max-cells", type=int, default=None, help="with --db: as in search_proteins (default 2^26)")
    ap.add_argument("--ungapped", action="store_true", help="with --db: as in search_proteins")
    ap.add_argument("--min-ungapped", type=int, default=None, metavar="N", help="with --ungapped: as in search_proteins")
    ap.add_argument("--band", type=int, default=None, metavar="W", help="with --ungapped: as in search_proteins, 0..256")
    a = ap.parse_args(argv)
    if a.D is not None and a.db is not None:
        ap.error("give -D or --db, not both")
    if a.fill_db is not None and a.db is not None:
        ap.error("--fill-db beside --db: --db searches every fragment, --fill-db only what the table of -D left unnamed")
    if a.fill_db is not None and a.D is None:
        ap.error("--fill-db needs -D")
    if a.D is None and a.db is None:
        ap.error("one of -D and --db is required")
    if a.fill_db is None and (a.explain_min is not None or a.fill_min_score is not None):
        ap.error("--explain-min and --fill-min-score need --fill-db")
    if a.explain_min is not None and a.explain_min < 1:
        ap.error("--explain-min must be >= 1")
    if a.fill_min_score is not None and a.fill_min_score < 0:
        ap.error("--fill-min-score must be >= 0")
    search_flags = (("--min-frag", a.min_frag), ("--max-hits", a.max_hits), ("--batch-nt", a.batch_nt), ("--hits", a.hits),
                    ("--min-shared", a.min_shared), ("--max-cand", a.max_cand), ("--max-db-per-kmer", a.max_db_per_kmer),
                    ("--min-ratio", a.min_ratio), ("--align-ref", a.align_ref), ("--gap-open", a.gap_open), ("--gap-extend", a.gap_extend),
                    ("--max-cells", a.max_cells), ("--ungapped", a.ungapped or None), ("--min-ungapped", a.min_ungapped), ("--band", a.band))
    if a.db is None and a.fill_db is None:
        for flag, given in search_flags:
            if given is not None:
                ap.error("%s needs --db" % flag)
    else:
        for flag, given in (("-m", a.m), ("-M", a.M), ("-g", a.g), ("-O", a.O or None)):
            if given is not None and a.db is not None:
                ap.error("%s beside --db: it belongs to the table scan of -D" % flag)
        if a.min_frag is not None and a.min_frag < 1:
            ap.error("--min-frag must be >= 1")
        if a.max_hits is not None and not 1 <= a.max_hits <= 64:
            ap.error("--max-hits must be in 1..64")
        if a.batch_nt is not None and a.batch_nt < 1:
            ap.error("--batch-nt must be >= 1")
        if a.band is not None and not a.ungapped:
            ap.error("--band needs --ungapped")
        if a.band is not None and not 0 <= a.band <= 256:
            ap.error("--band must be in 0..256")
        if a.min_ungapped is not None and not a.ungapped:
            ap.error("--min-ungapped needs --ungapped")
        if a.min_ungapped is not None and a.min_ungapped < 0:
            ap.error("--min-ungapped must be >= 0")
    if a.free_orfs and a.orfs is None and a.faa is None:
        ap.error("--free-orfs needs --orfs or --faa")
    if a.coding and a.orfs is None and a.faa is None:
        ap.error("--coding needs --orfs or --faa")
    if not a.coding and (a.coding_model is not None or a.save_coding_model is not None or a.min_coding != 0 or a.min_train != 100000):
        ap.error("--min-coding, --min-train, --coding-model and --save-coding-model need --coding")
    if a.repair and a.orfs is None and a.faa is None:
        ap.error("--repair needs --orfs or --faa")
    if not a.repair and (a.shifts is not None or a.repair_min_count != 0 or a.max_junctions != 4):
        ap.error("--repair-min-count, --max-junctions and --shifts need --repair")
    if a.starts and not a.coding:
        ap.error("--starts needs --coding")
    if not a.starts and (a.start_model is not None or a.save_start_model is not None or a.start_rounds != 4 or a.min_train_starts != 200):
        ap.error("--start-rounds, --min-train-starts, --start-model and --save-start-model need --starts")
    from . import _native as N
    try:
        dflt = lambda v, d: d if v is None else v      # noqa: E731
        search = None
        if a.db is not None or a.fill_db is not None:
            search = dict(min_shared=dflt(a.min_shared, 2), max_cand=dflt(a.max_cand, 8), max_db_per_kmer=dflt(a.max_db_per_kmer, 256),
                          align=dict(min_ratio_pct=dflt(a.min_ratio, 50), ref=dflt(a.align_ref, "query"), gap_open=dflt(a.gap_open, 11),
                                     gap_extend=dflt(a.gap_extend, 1), max_cells=dflt(a.max_cells, 1 << 26)))
            if a.ungapped:
                search["ungapped"] = dict(min_score=a.min_ungapped or 0)
            if a.band is not None:
                search["band"] = a.band
        line = call_regions(a.D, a.q, a.o, dflt(a.m, 5), dflt(a.M, 0), dflt(a.g, 200), a.O, a.merge_gap, a.min_score, a.min_len, a.all, a.gff,
                            orfs_out=a.orfs, faa_out=a.faa, start_codons=parse_start_codons(a.start_codons), select=a.select,
                            max_overlap=a.max_overlap, max_overlap_pct=a.max_overlap_pct,
                            free_min_res=a.min_res if a.free_orfs else None, coding=a.coding, min_coding=a.min_coding,
                            min_train=a.min_train, coding_model_in=a.coding_model, save_coding_model=a.save_coding_model,
                            starts=a.starts, start_rounds=a.start_rounds, min_train_starts=a.min_train_starts,
                            start_model_in=a.start_model, save_start_model=a.save_start_model, repair=a.repair,
                            repair_min_count=a.repair_min_count, max_junctions=a.max_junctions, shifts_out=a.shifts, db=a.db,
                            min_frag=dflt(a.min_frag, 30), max_hits=dflt(a.max_hits, 1), batch_nt=a.batch_nt, hits_out=a.hits, search=search,
                            fill_db=a.fill_db, explain_min=dflt(a.explain_min, 1), fill_min_score=dflt(a.fill_min_score, 0))
    except (N.KmerGutsNativeError, InputError, OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
