"""Search proteins against a set of known proteins on the GPU (kg_proteins_search): which known protein is this protein like, and
how much.  The step that names what `annotate` leaves at `none`.

    python -m kmergutsjava_amd.search_proteins (-d database.faa[.gz] [-d more.faa ...] | --db DB.kgsdb [--batch-residues N])
                                               -q queries.faa[.gz] [-q more ...] -o hits.tsv
                                               [--min-shared 2] [--max-cand 8] [--max-hits 1] [--max-db-per-kmer 256]
                                               [--min-ratio 50] [--align-ref longer|query] [--gap-open 11] [--gap-extend 1]
                                               [--max-cells N] [--all] [-A db_annotations.tsv [--transfer out.tsv]]
                                               [--truth query_annotations.tsv]
                                               [--paths [--trace hits|all] [--max-trace-cells N] [--cigar [m|eqx]] [--alignments FILE]]
                                               [--seeds exact|reduced] [--alphabet identity|reduced11|GROUPS] [--shape MASK ...]
                                               [--mask [both|queries|targets]] [--mask-window 12] [--mask-trigger 563] [--mask-extend 640]

The proteins of all -d files are the database, those of all -q files the queries, each in the order given (FASTA as
make_signatures reads it).  An id that occurs twice within the database or within the queries is an error; the same id in both
is allowed.  include/kmerguts_hip.h states the rule: a target is a candidate of a query when the two share at least --min-shared
distinct exact 8-mers, not counting the 8-mers that more than --max-db-per-kmer targets have (repeats and low complexity); the
--max-cand candidates with the most shared 8-mers (on a tie the earlier target) are aligned (BLOSUM62 in align_scores.py, a gap of
k residues costs --gap-open + k * --gap-extend, no traceback without --paths); an aligned pair is a hit when 100 * score >= --min-ratio * ref,
where ref is the larger of the two proteins' self-scores (--align-ref longer, the default) or the query's own (--align-ref
query).  A pair of more than --max-cells cells (default 2^26) is not aligned: skipped.  The defaults 2, 8, 256, 50 and longer are
this project's choice.

-o lines, in query FASTA order and within a query by rank (not skipped first, then larger score, then more shared 8-mers, then
the earlier target): `query_id<TAB>rank<TAB>target_id<TAB>shared<TAB>score<TAB>ref<TAB>ratio<TAB>query end<TAB>target end<TAB>
hit|below|skipped`, the ratio in percent (100 * score / ref, rounded down; `-` for a skipped pair), the ends 1-based (0 without
one).  With -A one more field: the target's function, or `-`.  Only `hit` records of rank below --max-hits (default 1) are
written; --all writes every record.
--transfer (needs -A) writes make_signatures' annotation format: one `query_id<TAB>function` line per query whose rank-0 record is
a hit and whose target has a function in -A.
--truth (the same format, for the queries) adds `labelled, agree, disagree, missed` to the summary, compared by function name: of
the labelled queries, those that got their own function, another one, or none.
--paths runs the traceback pass behind the alignment (kg_proteins_search_paths): where the alignment starts, how many columns it
has, and how many of them are identical, positive or gaps.  --trace hits (the default) traces the hit records only, --trace all
every aligned record with a score (the default with --all).  A record whose prefix box (query end * target end) has more than
--max-trace-cells cells (default 2^24) is not traced.  Every -o line then gains, behind the status and in front of the function
field of -A: `query start<TAB>target start<TAB>columns<TAB>identical<TAB>identity %<TAB>positive<TAB>gap opens<TAB>gap columns<TAB>
query cover %<TAB>target cover %`: the starts 1-based, identity % = 100 * identical // columns, the covers 100 * (end - start
+ 1) // length of the protein; each field is `-` for a record without a traced path.  The summary line gains `, traced: N,
untraced: M, trace ms: X`.  Without --paths every byte is as before.
--cigar (needs --paths) writes the alignment itself (the ops of include/kmerguts_hip.h, run-length encoded on the GPU): every -o
line gains one field behind the ten path fields and in front of the function field of -A, the CIGAR string with the query as the
read (`I` consumes the query only, `D` the target only), or `-` for a record without a traced path.  --cigar m (the default)
writes M for every residue column, --cigar eqx `=` for an identical one and `X` for any other.
--alignments FILE (needs --paths) writes one block per written record that has a path: a header line `>query_id target_id
score=N identity=N% columns=N`, then the alignment in rows of 60 columns, `Query  <first residue>  <residues and ->  <last
residue>`, a midline (the letter when identical, `+` when the BLOSUM62 score is positive, else a space) and `Target ...`
likewise, positions 1-based.  The text is made on the host from the ops and the sequences; the device is asked for `=`/`X` ops
unless --cigar m was given.  With either flag the summary line gains `, ops: N`; without them every byte is as before.
--seeds reduced finds the relatives that share no exact 8-mers with the query (kg_proteins_search_seeded): the prefilter then
counts shared seeds of a reduced alphabet (reduced11: AST, C, DEKNQR, F, G, H, ILV, M, P, W, Y; a substitution inside a class
keeps a seed) under two spaced shapes of nine care positions (111101101011 and 110110011010011; a substitution on a `0`
keeps a seed), and everything behind it, --min-shared and --max-db-per-kmer included, reads "seed" for "8-mer".  --alphabet
(identity, reduced11, or comma-separated groups of residues such as AST,C,DEKNQR,...) and --shape (a string of 1 and 0, at most
32 long, first and last 1; up to four, all with the same number of 1) each replace that part of the chosen seed set.  The
built-in set is this project's choice and is not tuned.  The summary line then gains `, seeds: <alphabet> x <shape,shape>`;
nothing else in any output changes, and with --seeds exact and neither override every byte is as before.
--mask keeps low-complexity segments (a poly-Q, a QEQEQE linker, a charged tail) from seeding candidates
(kg_proteins_search_masked; mask_proteins states the rule and writes the same mask to a file): the prefilter, and nothing else,
reads the proteins with the masked residues taken for non-residues; the alignment, --paths and --cigar read the proteins as they
are, so a hit's score is what it is without --mask.  --mask both (the default of the flag) masks the database and the queries,
--mask queries or --mask targets one side.  --mask-window, --mask-trigger and --mask-extend are mask_proteins' --window, --trigger
and --extend.  Under a spaced shape a masked residue on a `0` position keeps the seed.  The summary line then gains `, mask:
W/T/E <sides>, masked residues: N`; without --mask every byte is as before.
--db DB.kgsdb in place of -d searches an index that make_search_db has prepared once (kg_searchdb_open, kg_searchdb_search):
the targets' residues, their sorted seeds and their ids are the index's and are not made again, and the queries are searched in
batches of at most --batch-residues residues (default: the index's query room), so that the database and all queries need not fit
one call.  Giving both -d and --db is an error.  The seeds and the targets' mask are the index's: --seeds, --alphabet, --shape,
--mask both and --mask targets beside --db are errors that name the flag.  --mask queries masks the queries, with the index's
mask values when it has them, else with the flags'.  -A is optional when the index carries functions (make_search_db -A).  With
the same options the -o, --transfer and --alignments bytes are those of the -d run on the same FASTA files, wherever the batches
are cut.  The summary line sums the batches' counts (the database's and the masked k-mers are counted once) and gains `, db:
index (N targets)`.  Without --db every byte is as before.
The summary line goes to stderr.
"""
from __future__ import annotations

import argparse
import sys
from typing import Optional

import numpy as np

from .cluster_proteins import read_proteins
from .make_signatures import InputError, _read, parse_annotations

STATUS = (b"hit", b"below", b"skipped")
HIT = 0


def _ref(h, align_ref: str) -> int:
    return int(h["self_query"]) if align_ref in ("query", "member") else max(int(h["self_query"]), int(h["self_target"]))


PATH_FIELDS = 10
TRACED = 0


def path_fields(h, p, len_query: int, len_target: int) -> bytes:
    """The ten fields --paths adds to a line: h the hit record, p its path record."""
    if int(p["status"]) != TRACED:
        return b"\t-" * PATH_FIELDS
    sq, st_, eq, et = int(p["start_a"]), int(p["start_b"]), int(h["end_query"]), int(h["end_target"])
    ga, gb, ident = int(p["gap_cols_a"]), int(p["gap_cols_b"]), int(p["identical"])
    columns = (eq - sq + 1) - gb + ga + gb              # residue columns + gap columns
    return b"\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % (sq + 1, st_ + 1, columns, ident, 100 * ident // columns, int(p["positive"]),
                                                          int(p["gap_opens"]), ga + gb, 100 * (eq - sq + 1) // len_query,
                                                          100 * (et - st_ + 1) // len_target)


def cigar_field(p, op_start, ops, k: int) -> bytes:
    """The field --cigar adds to a line: record k's CIGAR, `-` without a traced path."""
    if int(p["status"]) != TRACED:
        return b"\t-"
    from .hotpath import cigar
    return b"\t" + cigar(ops[int(op_start[k]):int(op_start[k + 1])]).encode()


def written(hits, hit_start, q: int, max_hits: int, write_all: bool):
    """The records of query q that -o writes, as indices into hits."""
    for k in range(int(hit_start[q]), int(hit_start[q + 1])):
        if write_all or (int(hits[k]["status"]) == HIT and int(hits[k]["rank"]) < max_hits):
            yield k


def format_alignments(qids, dids, qseqs, dseqs, hits, hit_start, paths, op_start, ops, max_hits: int = 1, write_all: bool = False,
                      width: int = 60) -> bytes:
    """--alignments: one block (hotpath.alignment_text) per written record that has a path."""
    from .hotpath import alignment_text
    out = []
    for q, qid in enumerate(qids):
        for k in written(hits, hit_start, q, max_hits, write_all):
            if int(paths[k]["status"]) == TRACED:
                d = int(hits[k]["target"])
                out.append(alignment_text(qseqs[q], dseqs[d], hits[k], paths[k], ops[int(op_start[k]):int(op_start[k + 1])], width,
                                          qid.decode(), dids[d].decode()).encode() + b"\n")
    return b"".join(out)


def format_hits(qids, dids, hits, hit_start, max_hits: int = 1, write_all: bool = False, align_ref: str = "longer", functions=None,
                paths=None, qlens=None, dlens=None, cigars=None, ungapped=None) -> bytes:
    """functions: None, or {target id: (function, otu)}: every line gains the target's function or `-`.  paths: None, or one
    path record per hit record with the proteins' lengths in qlens / dlens: every line gains path_fields in front of it.
    cigars: None, or (op_start, ops) of the path records: every line gains cigar_field behind the path fields.  ungapped: None,
    or one ungapped record per hit record: every line gains ungapped, diagonal and on diagonal in front of the function."""
    out = []
    for q, qid in enumerate(qids):
        for k in range(int(hit_start[q]), int(hit_start[q + 1])):
            h = hits[k]
            status = int(h["status"])
            if not write_all and (status != HIT or int(h["rank"]) >= max_hits):
                continue
            ref, score, did = _ref(h, align_ref), int(h["score"]), dids[int(h["target"])]
            ratio = b"%d" % (100 * score // ref) if score >= 0 and ref > 0 else b"-"
            line = b"%s\t%d\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%s" % (qid, int(h["rank"]), did, int(h["shared"]), score, ref, ratio,
                                                               int(h["end_query"]) + 1, int(h["end_target"]) + 1, STATUS[status])
            if paths is not None:
                line += path_fields(h, paths[k], qlens[q], dlens[int(h["target"])])
            if cigars is not None:
                line += cigar_field(paths[k], cigars[0], cigars[1], k)
            if ungapped is not None:
                u = ungapped[k]
                line += b"\t%d\t%d\t%d" % (int(u["ungapped"]), int(u["diagonal"]), int(u["on_diagonal"]))
            if functions is not None:
                line += b"\t" + (functions[did][0] if did in functions else b"-")
            out.append(line + b"\n")
    return b"".join(out)


def transferred(qids, dids, hits, hit_start, functions):
    """-> {query id: function} of the queries whose rank-0 record is a hit on a target with a function."""
    out = {}
    for q, qid in enumerate(qids):
        if hit_start[q + 1] > hit_start[q]:
            h = hits[int(hit_start[q])]
            did = dids[int(h["target"])]
            if int(h["status"]) == HIT and did in functions:
                out[qid] = functions[did][0]
    return out


def format_transfer(qids, got) -> bytes:
    return b"".join(b"%s\t%s\n" % (qid, got[qid]) for qid in qids if qid in got)


def compare_truth(qids, got, truth) -> dict:
    t = {"labelled": 0, "agree": 0, "disagree": 0, "missed": 0}
    for qid in qids:
        want = truth.get(qid)
        if want is None:
            continue
        t["labelled"] += 1
        if qid not in got:
            t["missed"] += 1
        elif got[qid] == want[0]:
            t["agree"] += 1
        else:
            t["disagree"] += 1
    return t


def batch_cuts(lengths, batch_residues: int):
    """Cuts [0, .., n] of the queries into consecutive batches of at most batch_residues residues, one query at least each."""
    cuts, total = [0], 0
    for k, n in enumerate(lengths):
        if k > cuts[-1] and total + n > batch_residues:
            cuts.append(k)
            total = 0
        total += n
    if len(lengths) > cuts[-1] or len(cuts) == 1:
        cuts.append(len(lengths))
    return cuts


def _sum_stats(parts, index_mask):
    """The batches' statistics as one call's: counts and times summed; the targets, the masked k-mers and the index's share of the
    mask's counts once; the band as it is."""
    st = {}
    for part in parts:
        for k, v in part.items():
            if isinstance(v, dict):
                d = st.setdefault(k, {})
                for kk, vv in v.items():
                    d[kk] = vv if (k, kk) == ("band", "band") else d.get(kk, 0) + vv
            else:
                st[k] = v if k in ("targets", "kmers_masked") else st.get(k, 0) + v
    if "mask" in st and index_mask is not None:
        for kk, vv in index_mask.items():
            if kk in st["mask"] and not kk.startswith("ms_"):
                st["mask"][kk] -= (len(parts) - 1) * vv
    return st


def _search_index(handle, qseqs, batch_residues, paths, ops_mode, ungapped, kw):
    """The queries against an opened index, batch by batch -> what one call gives: (hits, hit_start, path records or None,
    statistics, op_start or None, ops or None, ungapped records or None), `query` counted over all queries."""
    info = handle.info()
    lengths = [len(s) for s in qseqs]
    room = int(info["query_room"])
    if batch_residues is None:
        batch_residues = room
    if batch_residues < 1:
        raise ValueError("--batch-residues must be >= 1")
    need = max([min(batch_residues, room)] + lengths)        # (a query longer than the batch is a batch of its own)
    if need > room:
        handle.reserve(need)
    cuts = batch_cuts(lengths, min(batch_residues, need))
    hits, starts, recs, op_starts, opsv, urecs, stats = [], [np.zeros(1, dtype=np.int64)], [], [np.zeros(1, dtype=np.int64)], [], [], []
    n_hits = n_ops = 0
    for a, b in zip(cuts, cuts[1:]):
        off = np.zeros(b - a + 1, dtype=np.int64)
        off[1:] = np.cumsum(lengths[a:b])
        got = handle.search(b"".join(qseqs[a:b]), off, paths=paths, **kw)
        h = got[0].copy()
        h["query"] += a
        hits.append(h)
        starts.append(got[1][1:] + n_hits)
        n_hits += len(h)
        if paths is None:
            stats.append(got[2])
        else:
            recs.append(got[2])
            stats.append(got[3])
            if ops_mode is not None:
                op_starts.append(got[4][1:] + n_ops)
                opsv.append(got[5])
                n_ops += len(got[5])
        if ungapped is not None:
            urecs.append(got[-1])
    return (np.concatenate(hits), np.concatenate(starts), np.concatenate(recs) if paths is not None else None,
            _sum_stats(stats, info.get("mask_stats")), np.concatenate(op_starts) if ops_mode is not None else None,
            np.concatenate(opsv) if ops_mode is not None else None, np.concatenate(urecs) if ungapped is not None else None)


def search_proteins(database, queries, out: str, min_shared: int = 2, max_cand: int = 8, max_hits: int = 1, max_db_per_kmer: int = 256,
                    align: Optional[dict] = None, write_all: bool = False, annotations: Optional[str] = None,
                    transfer: Optional[str] = None, truth: Optional[str] = None, device: int = 0, search=None,
                    paths: Optional[str] = None, max_trace_cells: Optional[int] = None, seeds=None, cigar: Optional[str] = None,
                    alignments: Optional[str] = None, mask: Optional[dict] = None, ungapped: Optional[dict] = None,
                    band: Optional[int] = None, db: Optional[str] = None, batch_residues: Optional[int] = None, open_db=None) -> str:
    """Write the files; returns the summary line.  `search` replaces hotpath.search_proteins (tests).  align: None, or the
    alignment parameters of hotpath.search_proteins (ref "query" is its "member").  paths: None, "hits" or "all" (--paths with
    its --trace); max_trace_cells: None for the library's default.  seeds: None (the exact 8-mers), "reduced" or a
    dict(alphabet=..., shapes=[...]) as hotpath.search_proteins takes it.  cigar: None, "m" or "eqx" (--cigar); alignments: None
    or the file --alignments writes; both need paths.  mask: None, or a dict of window, trigger, extend and sides as
    hotpath.search_proteins takes it (--mask).  ungapped: None, or {"min_score": N} (--ungapped, --min-ungapped): the candidates
    are ranked by the ungapped score of their best seed diagonal and those below N dropped.  band: None, or W (--band): every
    candidate is aligned in the band of half-width W around that diagonal; needs ungapped.  db: None, or the file of an index
    (--db) in the database's place: `database` must then be empty, seeds None and mask None or of sides "queries";
    batch_residues: None (the index's query room) or the residues of a batch of queries; `open_db` replaces
    hotpath.SearchDb.open (tests)."""
    from . import seeds as SD
    if band is not None and ungapped is None:
        raise ValueError("--band needs --ungapped")
    if band is not None and not 0 <= int(band) <= 256:
        raise ValueError("--band must be in 0..256")
    if ungapped is not None and int(ungapped.get("min_score", 0)) < 0:
        raise ValueError("--min-ungapped must be >= 0")
    seed_words = SD.describe(seeds) if SD.resolve(seeds) is not None else None
    if paths not in (None, "hits", "all"):
        raise ValueError("--trace must be hits or all")
    if cigar not in (None, "m", "eqx"):
        raise ValueError("--cigar must be m or eqx")
    if paths is None and (cigar is not None or alignments is not None):
        raise ValueError("--cigar and --alignments need --paths")
    ops_mode = cigar if cigar is not None else "eqx" if alignments is not None else None
    if max_hits < 1:
        raise ValueError("--max-hits must be >= 1")
    if transfer is not None and annotations is None and db is None:
        raise ValueError("--transfer needs -A")
    if truth is not None and annotations is None and db is None:
        raise ValueError("--truth needs -A")
    if db is not None and database:
        raise ValueError("give -d or --db, not both")
    if db is None and batch_residues is not None:
        raise ValueError("--batch-residues needs --db")
    if db is not None and seeds is not None:
        raise ValueError("--seeds beside --db: the seeds are the index's")
    if db is not None and mask is not None and mask.get("sides", "both") != "queries":
        raise ValueError("--mask %s beside --db: the targets' mask is the index's; --mask queries masks the queries" % mask.get("sides", "both"))
    if db is not None:
        return _search_proteins_index(db, queries, out, min_shared, max_cand, max_hits, max_db_per_kmer, align, write_all, annotations,
                                      transfer, truth, device, paths, max_trace_cells, cigar, alignments, mask, ungapped, band,
                                      batch_residues, open_db, ops_mode)
    dids, dseqs = read_proteins(database)
    qids, qseqs = read_proteins(queries)
    seqs = dseqs + qseqs
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        offsets[1:] = np.cumsum([len(s) for s in seqs])
    align = dict(align or {})
    align_ref = align.get("ref", "longer")
    if align_ref == "query":
        align["ref"] = "member"
    functions = parse_annotations(_read(annotations), annotations) if annotations is not None else None
    want = parse_annotations(_read(truth), truth) if truth is not None else None
    if search is None:
        from . import hotpath
        search = hotpath.search_proteins
    recs = op_start = ops = None
    more = {} if seed_words is None else {"seeds": seeds}
    if mask is not None:
        if mask.get("sides", "both") not in ("both", "queries", "targets"):
            raise ValueError("--mask must be both, queries or targets")
        more["mask"] = mask
    urecs = None
    if ungapped is not None:
        more["ungapped"] = dict(ungapped)
    if band is not None:
        more["band"] = int(band)
    if paths is None:
        got = search(b"".join(seqs), offsets, len(dids), min_shared=min_shared, max_cand=max_cand,
                     max_db_per_kmer=max_db_per_kmer, align=align, device=device, **more)
        hits, hit_start, st = got[:3]
    else:
        if max_trace_cells is not None:
            more["max_trace_cells"] = max_trace_cells
        if ops_mode is not None:
            more["ops"] = ops_mode
        got = search(b"".join(seqs), offsets, len(dids), min_shared=min_shared, max_cand=max_cand, max_db_per_kmer=max_db_per_kmer,
                     align=align, device=device, paths=paths, **more)
        hits, hit_start, recs, st = got[:4]
        if ops_mode is not None:
            op_start, ops = got[4:6]
    if ungapped is not None:
        urecs = got[-1]                     # (the ungapped records end the tuple)
    return _write_and_summarise(out, qids, dids, qseqs, dseqs, hits, hit_start, st, recs, op_start, ops, urecs, max_hits, write_all, align_ref,
                                functions, want, transfer, alignments, cigar, paths, ops_mode, seed_words, mask, ungapped, band)


def _write_and_summarise(out, qids, dids, qseqs, dseqs, hits, hit_start, st, recs, op_start, ops, urecs, max_hits, write_all, align_ref,
                         functions, want, transfer, alignments, cigar, paths, ops_mode, seed_words, mask, ungapped, band) -> str:
    """The files of a search and its summary line, from one call's results or from the batches' put together."""
    with open(out, "wb") as f:
        f.write(format_hits(qids, dids, hits, hit_start, max_hits, write_all, align_ref, functions, recs, [len(x) for x in qseqs],
                            [len(x) for x in dseqs], (op_start, ops) if cigar is not None else None, urecs))
    if alignments is not None:
        with open(alignments, "wb") as f:
            f.write(format_alignments(qids, dids, qseqs, dseqs, hits, hit_start, recs, op_start, ops, max_hits, write_all))
    got = transferred(qids, dids, hits, hit_start, functions) if functions is not None else {}
    if transfer is not None:
        with open(transfer, "wb") as f:
            f.write(format_transfer(qids, got))
    line = ("Queries: %d, targets: %d, candidates: %d, aligned: %d, hits: %d, queries hit: %d, transferred: %d, masked k-mers: %d, "
            "ms: encode %.3f, sort %.3f, join %.3f, align %.3f, total %.3f") % (
        st["queries"], st["targets"], st["candidates"], st["aligned"], st["hits"], st["queries_hit"], len(got), st["kmers_masked"],
        st.get("ms_encode", 0.0), st.get("ms_sort", 0.0), st.get("ms_join", 0.0), st.get("ms_align", 0.0), st.get("ms_total", 0.0))
    if want is not None:
        t = compare_truth(qids, got, want)
        line += ", labelled: %d, agree: %d, disagree: %d, missed: %d" % (t["labelled"], t["agree"], t["disagree"], t["missed"])
    if paths is not None:
        line += ", traced: %d, untraced: %d, trace ms: %.3f" % (st["traced"], st["untraced"], st.get("ms_trace", 0.0))
    if ops_mode is not None:
        line += ", ops: %d" % len(ops)
    if seed_words is not None:
        line += ", seeds: " + seed_words
    if mask is not None:
        from .mask_proteins import mask_words
        line += ", mask: %s, masked residues: %d" % (mask_words(mask, mask.get("sides", "both")), st["mask"]["masked_residues"])
    if ungapped is not None:
        u = st["ungapped"]
        line += ", ungapped: scored %d, dropped %d, cut %d, ungapped ms: %.3f" % (u["scored"], u["dropped"], u["cut"], u.get("ms_ungapped", 0.0))
    if band is not None:
        b = st["band"]
        line += ", band: %d, band cells: %d of %d" % (b["band"], b["band_cells"], b["full_cells"])
    return line


def _search_proteins_index(db, queries, out, min_shared, max_cand, max_hits, max_db_per_kmer, align, write_all, annotations, transfer,
                           truth, device, paths, max_trace_cells, cigar, alignments, mask, ungapped, band, batch_residues, open_db,
                           ops_mode) -> str:
    """search_proteins with --db: the checked arguments of search_proteins, the index in the database's place."""
    from . import seeds as SD
    from .make_search_db import seeds_of, unpack_names
    if open_db is None:
        from . import hotpath
        open_db = hotpath.SearchDb.open
    qids, qseqs = read_proteins(queries)
    align = dict(align or {})
    align_ref = align.get("ref", "longer")
    if align_ref == "query":
        align["ref"] = "member"
    want = parse_annotations(_read(truth), truth) if truth is not None else None
    with open_db(db, device=device) as handle:
        info = handle.info()
        dids, functions = unpack_names(handle.names(), int(info["targets"]))
        if annotations is not None:
            functions = parse_annotations(_read(annotations), annotations)
        if functions is None and (transfer is not None or truth is not None):
            raise ValueError("--transfer and --truth need -A, or an index made with make_search_db -A")
        dseq, doff = handle.targets()
        dseqs = [bytes(dseq[int(doff[k]):int(doff[k + 1])]) for k in range(len(doff) - 1)]
        kw = dict(min_shared=min_shared, max_cand=max_cand, max_db_per_kmer=max_db_per_kmer, align=align)
        qmask = None
        if mask is not None:                            # --mask queries: the index's values when it has them, else the flags'
            qmask = dict(info["mask"]) if info["mask"] is not None else {k: v for k, v in mask.items() if k != "sides"}
            kw["mask"] = qmask
        if ungapped is not None:
            kw["ungapped"] = dict(ungapped)
        if band is not None:
            kw["band"] = int(band)
        if paths is not None and max_trace_cells is not None:
            kw["max_trace_cells"] = max_trace_cells
        if paths is not None and ops_mode is not None:
            kw["ops"] = ops_mode
        hits, hit_start, recs, st, op_start, ops, urecs = _search_index(handle, qseqs, batch_residues, paths, ops_mode, ungapped, kw)
    seeds = seeds_of(info["seeds"])
    seed_words = SD.describe(seeds) if seeds is not None else None
    words = None                                        # what the summary says of the mask: the values and whose residues
    if info["mask"] is not None or qmask is not None:
        sides = "both" if info["mask"] is not None and qmask is not None else "targets" if qmask is None else "queries"
        words = dict(info["mask"] if info["mask"] is not None else qmask, sides=sides)
    line = _write_and_summarise(out, qids, dids, qseqs, dseqs, hits, hit_start, st, recs, op_start, ops, urecs, max_hits, write_all, align_ref,
                                functions, want, transfer, alignments, cigar, paths, ops_mode, seed_words, words, ungapped, band)
    return line + ", db: index (%d targets)" % int(info["targets"])


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.search_proteins",
                                 description="Search proteins against a set of known proteins on the GPU: shared 8-mers, then alignment.")
    ap.add_argument("-d", default=None, action="append", metavar="DATABASE", help="database protein FASTA (.gz allowed); may be given several times")
    ap.add_argument("-q", required=True, action="append", metavar="QUERIES", help="query protein FASTA (.gz allowed); may be given several times")
    ap.add_argument("-o", required=True, metavar="HITS", help="hits TSV to write")
    ap.add_argument("--db", default=None, metavar="DB", help="in place of -d: the index file make_search_db wrote; its seeds and target mask hold")
    ap.add_argument("--batch-residues", type=int, default=None, metavar="N",
                    help="with --db: search the queries in batches of at most N residues (default: the index's query room)")
    ap.add_argument("--min-shared", type=int, default=2, help="distinct unmasked 8-mers a candidate shares at least (default 2, this project's choice)")
    ap.add_argument("--max-cand", type=int, default=8, help="candidates aligned per query, 1..64 (default 8, this project's choice)")
    ap.add_argument("--max-hits", type=int, default=1, help="hits written per query (default 1)")
    ap.add_argument("--max-db-per-kmer", type=int, default=256, help="an 8-mer of more targets takes no part (default 256, this project's choice)")
    ap.add_argument("--min-ratio", type=int, default=50, help="a hit needs 100 * score >= this * ref (default 50, this project's choice)")
    ap.add_argument("--align-ref", choices=("longer", "query"), default="longer",
                    help="ref is the larger self-score of the two proteins (default) or the query's")
    ap.add_argument("--gap-open", type=int, default=11, help="a gap of k residues costs gap-open + k * gap-extend (default 11)")
    ap.add_argument("--gap-extend", type=int, default=1, help="(default 1)")
    ap.add_argument("--max-cells", type=int, default=1 << 26, help="a pair of more cells is not aligned: skipped (default 2^26)")
    ap.add_argument("--all", action="store_true", help="write every record to -o: below, skipped and every rank")
    ap.add_argument("-A", default=None, metavar="ANNOTATIONS", help="protein_id<TAB>function[<TAB>otu] lines of the database")
    ap.add_argument("--transfer", default=None, metavar="OUT", help="with -A: write query_id<TAB>function lines for make_signatures -A")
    ap.add_argument("--truth", default=None, metavar="ANNOTATIONS", help="with -A: the queries' own annotations to compare with")
    ap.add_argument("--paths", action="store_true", help="trace the alignments: start, columns, identity, gaps and coverage on every -o line")
    ap.add_argument("--trace", choices=("hits", "all"), default=None,
                    help="with --paths: trace the hit records only (default), or every aligned record with a score (default with --all)")
    ap.add_argument("--max-trace-cells", type=int, default=None,
                    help="with --paths: a record whose prefix box has more cells is not traced (default 2^24, this project's choice)")
    ap.add_argument("--cigar", nargs="?", const="m", choices=("m", "eqx"), default=None,
                    help="with --paths: one more field on every -o line, the alignment's CIGAR (m: M, I, D, the default; eqx: = and X for M)")
    ap.add_argument("--alignments", default=None, metavar="FILE", help="with --paths: write the alignments as text, 60 columns a row")
    ap.add_argument("--seeds", choices=("exact", "reduced"), default="exact",
                    help="what the prefilter counts: exact 8-mers (default), or reduced-alphabet spaced seeds for remote relatives")
    ap.add_argument("--alphabet", default=None, metavar="identity|reduced11|GROUPS",
                    help="replaces the seed set's alphabet: comma-separated groups of residues, e.g. AST,C,DEKNQR,F,G,H,ILV,M,P,W,Y")
    ap.add_argument("--shape", action="append", default=None, metavar="MASK",
                    help="replaces the seed set's shapes: 1 = care, 0 = don't care, first and last 1; up to four, of equal weight")
    ap.add_argument("--mask", nargs="?", const="both", choices=("both", "queries", "targets"), default=None,
                    help="keep low-complexity segments out of the prefilter: of both sides (default of the flag), the queries or the targets")
    from .mask_proteins import add_mask_options, mask_from_options
    add_mask_options(ap, "the alignment reads the proteins as they are")
    ap.add_argument("--ungapped", action="store_true",
                    help="rank a query's candidates by the ungapped score of their best seed diagonal, not by shared seeds alone; every -o "
                         "line gains ungapped, diagonal and on diagonal")
    ap.add_argument("--min-ungapped", type=int, default=None, metavar="N",
                    help="with --ungapped: a candidate whose ungapped score is below N is not aligned (default 0: none is dropped)")
    ap.add_argument("--band", type=int, default=None, metavar="W",
                    help="with --ungapped: align every candidate only within W diagonals of its best seed diagonal, 0..256 (no default: "
                         "without the flag the whole matrix is filled)")
    a = ap.parse_args(argv)
    if a.db is not None and a.d is not None:
        ap.error("give -d or --db, not both")
    if a.db is None and a.d is None:
        ap.error("one of -d and --db is required")
    if a.db is None and a.batch_residues is not None:
        ap.error("--batch-residues needs --db")
    if a.batch_residues is not None and a.batch_residues < 1:
        ap.error("--batch-residues must be >= 1")
    if a.db is not None:
        for flag, given in (("--seeds", a.seeds != "exact"), ("--alphabet", a.alphabet is not None), ("--shape", a.shape is not None)):
            if given:
                ap.error("%s beside --db: the seeds are the index's" % flag)
        if a.mask in ("both", "targets"):
            ap.error("--mask %s beside --db: the targets' mask is the index's; --mask queries masks the queries" % a.mask)
    if a.band is not None and not a.ungapped:
        ap.error("--band needs --ungapped")
    if a.band is not None and not 0 <= a.band <= 256:
        ap.error("--band must be in 0..256")
    if a.min_ungapped is not None and not a.ungapped:
        ap.error("--min-ungapped needs --ungapped")
    if a.min_ungapped is not None and a.min_ungapped < 0:
        ap.error("--min-ungapped must be >= 0")
    if a.shape is not None and len(a.shape) > 4:
        ap.error("at most 4 --shape")
    if not a.paths and (a.trace is not None or a.max_trace_cells is not None):
        ap.error("--trace and --max-trace-cells need --paths")
    if not a.paths and (a.cigar is not None or a.alignments is not None):
        ap.error("--cigar and --alignments need --paths")
    paths = (a.trace or ("all" if a.all else "hits")) if a.paths else None
    from . import _native as N
    align = dict(min_ratio_pct=a.min_ratio, ref=a.align_ref, gap_open=a.gap_open, gap_extend=a.gap_extend, max_cells=a.max_cells)
    from . import seeds as SD
    seeds = None
    if a.seeds != "exact" or a.alphabet is not None or a.shape is not None:
        seeds = dict(SD.BUILTIN[a.seeds])
        if a.alphabet is not None:
            seeds["alphabet"] = a.alphabet
        if a.shape is not None:
            seeds["shapes"] = a.shape
    try:
        line = search_proteins(a.d or [], a.q, a.o, a.min_shared, a.max_cand, a.max_hits, a.max_db_per_kmer, align, a.all, a.A, a.transfer,
                               a.truth, paths=paths, max_trace_cells=a.max_trace_cells, seeds=seeds, cigar=a.cigar, alignments=a.alignments,
                               mask=mask_from_options(ap, a, a.mask),
                               ungapped=dict(min_score=a.min_ungapped or 0) if a.ungapped else None, band=a.band, db=a.db,
                               batch_residues=a.batch_residues)
    except (N.KmerGutsNativeError, InputError, OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print(line, file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
