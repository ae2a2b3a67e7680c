"""Prepare a protein database for search_proteins --db once: build the resident index on the GPU (kg_searchdb_build) and write its
file (kg_searchdb_save).

    python -m kmergutsjava_amd.make_search_db -d database.faa[.gz] [-d more ...] -o DB.kgsdb [--seeds exact|reduced]
                                              [--alphabet identity|reduced11|GROUPS] [--shape MASK ...]
                                              [--mask [--mask-window 12] [--mask-trigger 563] [--mask-extend 640]] [-A db_annotations.tsv]

The proteins of all -d files are the targets, in the order given (FASTA as make_signatures reads it); an id that occurs twice is
an error.  --seeds, --alphabet and --shape choose what the prefilter counts, as in search_proteins; --mask keeps the targets'
low-complexity segments from seeding candidates.  Both are fixed in the index: a search against it uses them.  include/
kmerguts_hip.h states the file's format.
The names blob of the file is this front end's own: the targets' ids joined by newlines; with -A a NUL byte follows and then, again
joined by newlines and in the same order, each target's function (empty for a target without one).  An index without -A has no
NUL byte: search_proteins --db then needs its own -A to name functions.
The summary line goes to stderr.
"""
from __future__ import annotations

import argparse
import sys
from typing import Optional

import numpy as np

from .cluster_proteins import read_proteins
from .make_signatures import InputError, _read, parse_annotations


def pack_names(ids, functions=None) -> bytes:
    """ids: the targets' ids in order; functions: None, or {id: (function, otu)} as parse_annotations gives it."""
    blob = b"\n".join(ids)
    if functions is not None:
        blob += b"\0" + b"\n".join(functions[i][0] if i in functions else b"" for i in ids)
    return blob


def unpack_names(blob: bytes, n: int):
    """-> (ids, functions): functions is None for a blob without them, else {id: (function, None)} of the targets that have one."""
    head, nul, tail = blob.partition(b"\0")
    ids = head.split(b"\n") if n else []
    if len(ids) != n:
        raise InputError("the index names %d targets and holds %d" % (len(ids), n))
    if not nul:
        return ids, None
    fns = tail.split(b"\n") if n else []
    if len(fns) != n:
        raise InputError("the index has %d function entries for %d targets" % (len(fns), n))
    return ids, {i: (f, None) for i, f in zip(ids, fns) if f}


def seeds_of(info_seeds) -> Optional[dict]:
    """SearchDb.info()["seeds"] -> the dict(alphabet=..., shapes=[...]) seeds.describe reads; None for the exact 8-mers."""
    if info_seeds is None:
        return None
    from .align_scores import ALPHA
    groups = [bytes(ALPHA[c] for c in range(20) if info_seeds["cls"][c] == k).decode() for k in range(info_seeds["alphabet_size"])]
    shapes = ["".join("1" if m >> j & 1 else "0" for j in range(int(m).bit_length())) for m in info_seeds["shape"]]
    return dict(alphabet=",".join(groups), shapes=shapes)


def make_search_db(database, out: str, seeds=None, mask: Optional[dict] = None, annotations: Optional[str] = None, device: int = 0,
                   build=None) -> str:
    """Write the file; returns the summary line.  `build` replaces hotpath.SearchDb.build (tests): it is given the same arguments
    and returns an object with info() and save(path)."""
    ids, seqs = read_proteins(database)
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        offsets[1:] = np.cumsum([len(s) for s in seqs])
    functions = parse_annotations(_read(annotations), annotations) if annotations is not None else None
    if build is None:
        from . import hotpath
        build = hotpath.SearchDb.build
    db = build(b"".join(seqs), offsets, seeds=seeds, mask=mask, names=pack_names(ids, functions), device=device)
    try:
        db.save(out)
        info = db.info()
    finally:
        db.close()
    line = "Targets: %d, residues: %d, valid windows: %d, pairs: %d, k-mers: %d, device bytes: %d, ms: upload %.3f, encode %.3f, sort %.3f, index %.3f, total %.3f" % (
        info["targets"], info["residues"], info["valid_windows"], info["pairs"], info["kmers"], info["device_bytes"],
        info.get("ms_upload", 0.0), info.get("ms_encode", 0.0), info.get("ms_sort", 0.0), info.get("ms_index", 0.0), info.get("ms_total", 0.0))
    if info["seeds"] is not None:
        from . import seeds as SD
        line += ", seeds: " + SD.describe(seeds_of(info["seeds"]))
    if info["mask"] is not None:
        from .mask_proteins import mask_words
        line += ", mask: %s, masked residues: %d" % (mask_words(info["mask"]), info["mask_stats"]["masked_residues"])
    if functions is not None:
        line += ", functions: %d" % sum(1 for i in ids if i in functions)
    return line


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.make_search_db",
                                 description="Build the resident index of a protein database on the GPU and write its file.")
    ap.add_argument("-d", required=True, action="append", metavar="DATABASE", help="database protein FASTA (.gz allowed); may be given several times")
    ap.add_argument("-o", required=True, metavar="DB", help="index file to write")
    ap.add_argument("--seeds", choices=("exact", "reduced"), default="exact", help="what the prefilter counts (search_proteins --seeds)")
    ap.add_argument("--alphabet", default=None, metavar="identity|reduced11|GROUPS", help="replaces the seed set's alphabet")
    ap.add_argument("--shape", action="append", default=None, metavar="MASK", help="replaces the seed set's shapes; up to four, of equal weight")
    ap.add_argument("--mask", action="store_true", help="keep the targets' low-complexity segments out of the prefilter")
    from .mask_proteins import add_mask_options, mask_from_options
    add_mask_options(ap, "the alignment reads the proteins as they are")
    ap.add_argument("-A", default=None, metavar="ANNOTATIONS", help="protein_id<TAB>function[<TAB>otu] lines of the database: the functions go into the index")
    a = ap.parse_args(argv)
    if a.shape is not None and len(a.shape) > 4:
        ap.error("at most 4 --shape")
    from . import _native as N
    from . import seeds as SD
    seeds = None
    if a.seeds != "exact" or a.alphabet is not None or a.shape is not None:
        seeds = dict(SD.BUILTIN[a.seeds])
        if a.alphabet is not None:
            seeds["alphabet"] = a.alphabet
        if a.shape is not None:
            seeds["shapes"] = a.shape
    try:
        line = make_search_db(a.d, a.o, seeds=seeds, mask=mask_from_options(ap, a, None), annotations=a.A)
    except (N.KmerGutsNativeError, InputError, OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print(line, file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
