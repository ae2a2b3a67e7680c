"""Derive KmerGuts signatures from annotated proteins on the GPU (kg_signatures_derive), and optionally write a data directory.

    python -m kmergutsjava_amd.make_signatures -p proteins.faa[.gz] -A annotations.tsv -o sigs.txt [-D OUTDIR [-s NUM_SIGS] [-z]]
                                               [--min-proteins 2] [--purity 80]

proteins.faa: FASTA; a protein's id is the first token after '>', its sequence the following lines with surrounding
whitespace removed.  annotations.tsv: lines `protein_id<TAB>function[<TAB>otu]` (blank lines skipped); a missing OTU column
means the OTU named "".  Proteins absent from the file are unannotated (they still count in n_v).  Function and OTU names are
numbered in byte order of the names.

-o writes the signatures in the text format `make_table -i` reads (KMER, otuIndex, avgFromEnd, functionIndex, functionWt;
weights with 9 significant digits, which round-trip through float32).  -D also writes OUTDIR/function.index and
OUTDIR/otu.index (`<i>\\t<name>` lines; the scanners read only the former) and the table, placed on the GPU from the device
signature set (kg_table_build_device) with make_table's default size (the smallest prime >= 2 * signatures): the layout
`kmer_guts -D` and KmerGutsJava.run read.  The defaults --min-proteins 2 and --purity 80 are this project's choice.
"""
from __future__ import annotations

import argparse
import gzip
import os
import sys
from typing import Optional

import numpy as np

from .make_table import default_num_sigs, kmer_letters


class InputError(ValueError):
    """A malformed input line: the message names the file and the line."""


def _read(path: str) -> bytes:
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    return data


def parse_fasta(data: bytes, name: str = "proteins"):
    """FASTA bytes -> (ids, sequences), in file order.  Raises InputError on a duplicate id or sequence text before the first
    caption."""
    ids, seqs, where = [], [], {}
    cur = None
    for ln, raw in enumerate(data.split(b"\n"), 1):
        line = raw.strip()
        if line.startswith(b">"):
            toks = line[1:].split()
            if not toks:
                raise InputError("%s line %d: caption without an id" % (name, ln))
            pid = toks[0]
            if pid in where:
                raise InputError("%s line %d: duplicate protein id %s (first on line %d)" % (name, ln, pid.decode("latin-1"), where[pid]))
            where[pid] = ln
            ids.append(pid)
            cur = []
            seqs.append(cur)
        elif line:
            if cur is None:
                raise InputError("%s line %d: sequence text before the first '>' caption" % (name, ln))
            cur.append(line)
    return ids, [b"".join(s) for s in seqs]


def parse_annotations(data: bytes, name: str = "annotations"):
    """TSV bytes -> {protein id: (function name, otu name)}.  Raises InputError on a malformed line or a repeated id."""
    out, where = {}, {}
    for ln, raw in enumerate(data.split(b"\n"), 1):
        line = raw.rstrip(b"\r")
        if not line.strip():
            continue
        f = line.split(b"\t")
        if len(f) not in (2, 3) or not f[0] or not f[1]:
            raise InputError("%s line %d: malformed line (want protein_id<TAB>function[<TAB>otu])" % (name, ln))
        if f[0] in where:
            raise InputError("%s line %d: protein id %s repeated (first on line %d)" % (name, ln, f[0].decode("latin-1"), where[f[0]]))
        where[f[0]] = ln
        out[f[0]] = (f[1], f[2] if len(f) == 3 else b"")
    return out


def number_inputs(ids, seqs, ann):
    """-> seq bytes, offsets, fn, otu, function names, otu names (names numbered in byte order)."""
    fnames = sorted({a[0] for pid, a in ann.items()})
    onames = sorted({a[1] for pid, a in ann.items()})
    fidx = {n: i for i, n in enumerate(fnames)}
    oidx = {n: i for i, n in enumerate(onames)}
    fn = np.full(len(ids), -1, dtype=np.int32)
    otu = np.zeros(len(ids), dtype=np.int32)
    for k, pid in enumerate(ids):
        a = ann.get(pid)
        if a is not None:
            fn[k] = fidx[a[0]]
            otu[k] = oidx[a[1]]
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return b"".join(seqs), offsets, fn, otu, fnames, onames


def signature_text(sigs: np.ndarray) -> str:
    """SIGNATURE_DTYPE records -> make_table -i text (weights with 9 significant digits: they round-trip through float32)."""
    return "".join("%s\t%d\t%d\t%d\t%.9g\n" % (kmer_letters(int(r["kmer"])), int(r["otuIndex"]), int(r["avgFromEnd"]),
                                               int(r["functionIndex"]), float(r["functionWt"])) for r in sigs)


def _index_text(names) -> bytes:
    return b"".join(b"%d\t%s\n" % (i, n) for i, n in enumerate(names))


def make_signatures(proteins: str, annotations: str, out: str, out_dir: Optional[str] = None, num_sigs: Optional[int] = None,
                    gz: bool = False, min_proteins: int = 2, purity: int = 80, device: int = 0) -> dict:
    """Write the files; returns the counts that the command line prints."""
    from . import hotpath
    ids, seqs = parse_fasta(_read(proteins), proteins)
    ann = parse_annotations(_read(annotations), annotations)
    seq, offsets, fn, otu, fnames, onames = number_inputs(ids, seqs, ann)
    r = {"proteins": len(ids), "slots": None, "placed": None}
    with hotpath.derive_signatures(seq, offsets, fn, otu, min_proteins, purity, device=device) as s:
        st = s.stats()
        r["windows"], r["signatures"] = st["valid_windows"], s.count
        with open(out, "w") as f:
            f.write(signature_text(s.numpy()))
        if out_dir is not None:
            table_name = "kmer.table.mem_map" + (".gz" if gz else "")
            if not gz and os.path.exists(os.path.join(out_dir, table_name + ".gz")):
                raise FileExistsError("%s already holds %s.gz, which the readers would take instead of the new %s" %
                                      (out_dir, table_name, table_name))
            if os.path.exists(os.path.join(out_dir, "function.index.gz")):
                raise FileExistsError("%s already holds function.index.gz, which the readers would take instead of the new "
                                      "function.index" % out_dir)
            os.makedirs(out_dir, exist_ok=True)
            S = default_num_sigs(s.count) if num_sigs is None else int(num_sigs)
            with hotpath.SignatureTable.build(s.device_tensor(), S, device) as tab:
                r["slots"], r["placed"] = S, tab.placed
                tab.save(os.path.join(out_dir, table_name))
            with open(os.path.join(out_dir, "function.index"), "wb") as f:
                f.write(_index_text(fnames))
            with open(os.path.join(out_dir, "otu.index"), "wb") as f:
                f.write(_index_text(onames))
    return r


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.make_signatures",
                                 description="Derive KmerGuts signatures from annotated proteins on the GPU.")
    ap.add_argument("-p", required=True, metavar="PROTEINS", help="protein FASTA (.gz allowed)")
    ap.add_argument("-A", required=True, metavar="ANNOTATIONS", help="protein_id<TAB>function[<TAB>otu] lines")
    ap.add_argument("-o", required=True, metavar="SIGNATURES", help="signature text to write (make_table -i format)")
    ap.add_argument("-D", default=None, metavar="OUTDIR", help="also write a data directory (table, function.index, otu.index)")
    ap.add_argument("-s", type=int, default=None, metavar="NUM_SIGS", help="table slots (default: smallest prime >= 2n)")
    ap.add_argument("-z", action="store_true", help="write kmer.table.mem_map.gz")
    ap.add_argument("--min-proteins", type=int, default=2, help="n_v >= this (default 2, this project's choice)")
    ap.add_argument("--purity", type=int, default=80, help="100 c_f* >= purity * n_v (default 80, this project's choice)")
    a = ap.parse_args(argv)
    from . import _native as N
    try:
        if a.D is None and (a.s is not None or a.z):
            raise ValueError("-s and -z need -D")
        if a.s is not None and a.s <= 0:
            raise ValueError("-s must be positive")
        r = make_signatures(a.p, a.A, a.o, a.D, a.s, a.z, a.min_proteins, a.purity)
    except N.KmerGutsNativeError as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    except (OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    line = "Proteins: %d, windows: %d, signatures: %d" % (r["proteins"], r["windows"], r["signatures"])
    if r["slots"] is not None:
        line += ", slots: %d, placed: %d" % (r["slots"], r["placed"])
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
