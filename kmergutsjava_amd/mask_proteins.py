"""Mask the low-complexity segments of proteins on the GPU (kg_proteins_mask): the poly-Q, the QEQEQE linker and the charged tail
that would otherwise seed candidates in search_proteins and edges in cluster_proteins.

    python -m kmergutsjava_amd.mask_proteins -p proteins.faa[.gz] [-p more.faa ...] -o masked.faa [--x] [--segments segments.tsv]
                                             [--window 12] [--trigger 563] [--extend 640]

The proteins of all -p files form one batch, in the order given (FASTA as make_signatures reads it); a protein id that occurs
twice is an error.  include/kmerguts_hip.h states the rule, which follows SEG's first two stages: a window of --window residues
whose composition has at most --trigger / 256 bits of entropy triggers, the run of windows around it with at most --extend / 256
bits is the extension, and every residue of those windows is masked.  The thresholds are integers in units of 1/256 bit; the
defaults 12, 563 and 640 (SEG's 2.2 and 2.5 bits) are this project's choice and are not tuned.

-o is the proteins again, `>id` and the sequence in 60-column lines, with the masked residues in lowercase, or as `X` with --x.
(A residue that was lowercase in the input counts as a non-residue for the rule, as it does everywhere in this package.)
--segments lines, in (protein, start) order: `protein_id<TAB>start<TAB>end<TAB>length`, 1-based and inclusive.
The summary line goes to stderr: proteins, residues, masked, share in percent, segments, proteins touched, ms.
search_proteins --mask and cluster_proteins --mask apply the same mask inside their own calls, to the seeding pass only.
"""
from __future__ import annotations

import argparse
import sys
from typing import Optional

import numpy as np

from .cluster_proteins import read_proteins
from .make_signatures import InputError

WINDOW, TRIGGER, EXTEND = 12, 563, 640


def masked_sequence(p: bytes, flags, x: bool = False) -> bytes:
    """One protein with its masked residues in lowercase (0x20 set on a letter; any other byte as it is), or as X."""
    a = np.frombuffer(p, dtype=np.uint8).copy()
    on = np.asarray(flags, dtype=bool)
    if x:
        a[on] = ord("X")
    else:
        letter = ((a >= ord("A")) & (a <= ord("Z")))
        a[on & letter] |= 0x20
    return a.tobytes()


def format_fasta(ids, seqs, flags, offsets, x: bool = False) -> bytes:
    out = []
    for k, pid in enumerate(ids):
        p = masked_sequence(seqs[k], flags[int(offsets[k]):int(offsets[k + 1])], x)
        out.append(b">" + pid + b"\n" + b"".join(p[j:j + 60] + b"\n" for j in range(0, len(p), 60)))
    return b"".join(out)


def format_segments(ids, segments) -> bytes:
    return b"".join(b"%s\t%d\t%d\t%d\n" % (ids[int(s["protein"])], int(s["start"]) + 1, int(s["end"]) + 1,
                                           int(s["end"]) - int(s["start"]) + 1) for s in segments)


def mask_words(mask: dict, sides: Optional[str] = None) -> str:
    """`W/T/E` of a mask dict (and the sides behind it): what the summary lines of search_proteins and cluster_proteins gain."""
    w = "%d/%d/%d" % (mask.get("window", WINDOW), mask.get("trigger", TRIGGER), mask.get("extend", EXTEND))
    return w if sides is None else w + " " + sides


def mask_proteins(proteins, out: str, x: bool = False, segments: Optional[str] = None, window: int = WINDOW, trigger: int = TRIGGER,
                  extend: int = EXTEND, device: int = 0, mask=None) -> str:
    """Write the files; returns the summary line.  `mask` replaces hotpath.mask_proteins (tests)."""
    ids, seqs = read_proteins(proteins)
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        offsets[1:] = np.cumsum([len(s) for s in seqs])
    if mask is None:
        from . import hotpath
        mask = hotpath.mask_proteins
    flags, segs, _seg_start, st = mask(b"".join(seqs), offsets, window=window, trigger=trigger, extend=extend, device=device)
    with open(out, "wb") as f:
        f.write(format_fasta(ids, seqs, flags, offsets, x))
    if segments is not None:
        with open(segments, "wb") as f:
            f.write(format_segments(ids, segs))
    return "Proteins: %d, residues: %d, masked: %d (%.1f %%), segments: %d, proteins touched: %d, ms: %.3f" % (
        st["proteins"], st["residues"], st["masked_residues"], 100.0 * st["masked_residues"] / max(st["residues"], 1), st["segments"],
        st["proteins_masked"], st.get("ms_mask", 0.0))


def add_mask_options(ap, what: str) -> None:
    """--mask-window / --mask-trigger / --mask-extend of search_proteins and cluster_proteins."""
    ap.add_argument("--mask-window", type=int, default=None, metavar="W", help="with --mask: residues of a window, 4..32 (default 12)")
    ap.add_argument("--mask-trigger", type=int, default=None, metavar="T",
                    help="with --mask: a window of at most T / 256 bits triggers (default 563, SEG's 2.2 bits; this project's choice)")
    ap.add_argument("--mask-extend", type=int, default=None, metavar="E",
                    help="with --mask: ... and the windows around it of at most E / 256 bits extend it (default 640, SEG's 2.5 bits); " + what)


def mask_from_options(ap, a, sides: Optional[str]):
    """The mask dict of parsed options (None without --mask); the three values need --mask."""
    given = {k: v for k, v in (("window", a.mask_window), ("trigger", a.mask_trigger), ("extend", a.mask_extend)) if v is not None}
    if a.mask is None or a.mask is False:
        if given:
            ap.error("--mask-window, --mask-trigger and --mask-extend need --mask")
        return None
    mask = dict(window=WINDOW, trigger=TRIGGER, extend=EXTEND)
    mask.update(given)
    if sides is not None:
        mask["sides"] = sides
    return mask


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.mask_proteins",
                                 description="Mask the low-complexity segments of proteins on the GPU.")
    ap.add_argument("-p", required=True, action="append", metavar="PROTEINS", help="protein FASTA (.gz allowed); may be given several times")
    ap.add_argument("-o", required=True, metavar="MASKED", help="masked protein FASTA to write")
    ap.add_argument("--x", action="store_true", help="write masked residues as X instead of lowercase")
    ap.add_argument("--segments", default=None, metavar="SEGMENTS", help="also write protein_id<TAB>start<TAB>end<TAB>length lines, 1-based")
    ap.add_argument("--window", type=int, default=WINDOW, help="residues of a window, 4..32 (default 12)")
    ap.add_argument("--trigger", type=int, default=TRIGGER, help="a window of at most this / 256 bits triggers (default 563, this project's choice)")
    ap.add_argument("--extend", type=int, default=EXTEND, help="... and the windows around it of at most this / 256 bits extend it (default 640)")
    a = ap.parse_args(argv)
    from . import _native as N
    try:
        line = mask_proteins(a.p, a.o, a.x, a.segments, a.window, a.trigger, a.extend)
    except (N.KmerGutsNativeError, InputError, OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print(line, file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
