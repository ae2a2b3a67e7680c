"""Locate function calls on contigs: a DNA scan whose CALL records are merged into function regions on the GPU
(kg_result_regions).

    python -m kmergutsjava_amd.call_regions -D KmerData -q contigs.fna[.gz] -o regions.tsv [-m 5] [-M 0] [-g 200] [-O]
                                            [--merge-gap 600] [--min-score 0] [--min-len 0] [--all] [--gff]

The table and function.index[.gz] are loaded the way annotate loads them.  Contigs are read with
make_signatures.parse_fasta (a duplicate id is an error) and scanned whole, in batches of at most
KmerGutsJava.MAX_BATCH_CHARS characters.  Output, in FASTA order and inside a contig in the library's output order
(left, right, strand, function index), one line per kept region (every region with --all):
    contig_id<TAB>left+1<TAB>right+1<TAB>strand<TAB>function<TAB>score<TAB>weighted<TAB>n_calls<TAB>frames<TAB>status
with 1-based inclusive coordinates on the contig as given, strand + or -, weighted as %.9g, frames the frames of the region's
CALLs (e.g. `0` or `0,2`; more than one: a frameshift candidate) and status kept or below.  --gff writes GFF3 lines with the
same content instead.  Stdout: `Contigs: N, with calls: K, regions: R, kept: A, multi-frame: F`.
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


def format_regions(ids, regs, fnames, write_all: bool = False, gff: bool = False) -> bytes:
    """Region records (REGION_DTYPE, `seq` indexing ids) as text, in the order given."""
    lines = [b"##gff-version 3\n"] if gff else []
    for r in regs:
        if not (r["kept"] or write_all):
            continue
        status = b"kept" if r["kept"] else b"below"
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


def call_regions(data_dir: str, contigs: str, out: str, min_hits: int = 5, min_weighted_hits: int = 0, max_gap: int = 200,
                 order_constraint: bool = False, merge_gap: int = 600, min_score: int = 0, min_len: int = 0,
                 write_all: bool = False, gff: bool = False, device: int = 0) -> str:
    """Write the regions; returns the summary line."""
    from . import hotpath
    from .kmer_guts_java import KmerGutsJava, _resident_table
    table_path = _data_file(data_dir, "kmer.table.mem_map")
    fn_path = _data_file(data_dir, "function.index")
    if table_path is None or fn_path is None:
        raise FileNotFoundError("%s holds no kmer.table.mem_map[.gz] or function.index[.gz]" % data_dir)
    fnames = parse_index(_read(fn_path), fn_path)
    ids, seqs = parse_fasta(_read(contigs), contigs)
    tab = _resident_table(table_path, device)
    params = hotpath.Params(aa=False, order_constraint=order_constraint, min_hits=min_hits, min_weighted_hits=min_weighted_hits,
                            max_gap=max_gap)
    parts, starts = [], [np.zeros(1, dtype=np.int64)]
    k = 0
    while k < len(ids):
        j, size = k, 0
        while j < len(ids) and (j == k or size + len(seqs[j]) <= KmerGutsJava.MAX_BATCH_CHARS):
            size += len(seqs[j])
            j += 1
        off = np.zeros(j - k + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs[k:j]])
        with tab.scan(b"".join(seqs[k:j]), off, params) as r:
            regs, start = r.regions(off, merge_gap, min_score, min_len)
        regs["seq"] += k
        parts.append(regs)
        starts.append(start[1:] + starts[-1][-1])
        k = j
    regs = np.concatenate(parts) if parts else np.zeros(0, dtype=hotpath.N.REGION_DTYPE)
    with open(out, "wb") as f:
        f.write(format_regions(ids, regs, fnames, write_all, gff))
    return summary_of(regs, np.concatenate(starts))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.call_regions",
                                 description="Merge the CALLs of a DNA scan into function regions on the contigs, on the GPU.")
    ap.add_argument("-D", required=True, metavar="DATADIR", help="data directory (kmer.table.mem_map[.gz], function.index[.gz])")
    ap.add_argument("-q", required=True, metavar="CONTIGS", help="contig FASTA (.gz allowed)")
    ap.add_argument("-o", required=True, metavar="OUT", help="regions TSV (or GFF3) to write")
    ap.add_argument("-m", type=int, default=5, help="minHits (default 5)")
    ap.add_argument("-M", type=int, default=0, help="minWeightedHits (default 0)")
    ap.add_argument("-g", type=int, default=200, help="maxGap (default 200)")
    ap.add_argument("-O", action="store_true", help="order constraint")
    ap.add_argument("--merge-gap", type=int, default=600, help="nucleotides two CALLs of one function may lie apart (default 600, this project's choice)")
    ap.add_argument("--min-score", type=int, default=0, help="a region is kept with score >= this (default 0)")
    ap.add_argument("--min-len", type=int, default=0, help="... and at least this many nucleotides long (default 0)")
    ap.add_argument("--all", action="store_true", help="write every region, not only the kept ones")
    ap.add_argument("--gff", action="store_true", help="write GFF3 instead of TSV")
    a = ap.parse_args(argv)
    from . import _native as N
    try:
        line = call_regions(a.D, a.q, a.o, a.m, a.M, a.g, a.O, a.merge_gap, a.min_score, a.min_len, a.all, a.gff)
    except (N.KmerGutsNativeError, InputError, OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
