"""Hand-made chains for kg_regionset_repair with their answers worked out by hand, in strand coordinates, and a builder that
lays each one on either strand of a contig.  Shared by the CPU tests (both model forms) and the GPU tests.

The background is GCA repeated: without a T no frame of the strand has a stop or a start, and without an A neither has the other
strand.  Stops and the ATG are then put where a case wants them (every case uses start_codons = 1, ATG alone).  L = 90; the
frame-0 CALL covers codons 1..8 (x 3..26) in every two-segment case."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd._native import CALL_DTYPE

from orfs_model import GENETIC_CODE

L = 90
_COMP = {65: 84, 67: 71, 71: 67, 84: 65}


def text_with(puts):
    t = bytearray(b"GCA" * (L // 3))
    for x, s in puts:
        t[x:x + len(s)] = s
    return bytes(t)


def translate(t: bytes) -> bytes:
    assert len(t) % 3 == 0
    return bytes(ord(GENETIC_CODE["ACGT".index(chr(t[i])) * 16 + "ACGT".index(chr(t[i + 1])) * 4 + "ACGT".index(chr(t[i + 2]))])
                 for i in range(0, len(t), 3))


def lay(text: bytes, strand: int, calls):
    """calls: (frame, first codon, last codon, count) on the strand -> (CALL_DTYPE in container order, contig bytes, offsets)."""
    contig = text if not strand else bytes(_COMP[c] for c in reversed(text))
    rows = sorted((3 * strand + f, a, z, cnt, 7, 1.0) for f, a, z, cnt in calls)
    out = np.zeros(len(rows), dtype=CALL_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out, np.frombuffer(contig, dtype=np.uint8).copy(), np.array([0, len(contig)], dtype=np.int64)


_ATG = (0, b"ATG")
_END2 = (77, b"TAA")            # frame 2, codon 25
_TWO = [(0, 1, 8, 5), (2, 12, 19, 5)]          # x 3..26 in frame 0, x 38..61 in frame 2: mid = (26 + 1 + 38) // 2 = 32, gap 11


def _case(name, puts, calls, state, junctions=(), extent=None, protein=None, start_codon=1, flags=None, first_inner=-1, frame=0, **params):
    return dict(name=name, text=text_with(puts), calls=calls, state=state, junctions=list(junctions), extent=extent, protein=protein,
                start_codon=start_codon, flags=flags, first_inner=first_inner, frame=frame, params=params)


def cases():
    """Each: text, calls, state ('repaired' / 'failed' / 'single' / 'skipped'), and for a repaired one the junctions
    (J, from, to, res, gap), the extent (xs, xe), the protein, start_codon, flags and first_inner -- all on the strand."""
    out = []
    # a deletion: frame 0 then frame 2.  No stop behind the frame-0 evidence (tp = n_0 = 30, hi = 90), none in front of the
    # frame-2 evidence (sq = -1, lo = 2): J = mid = 32.  Part 1 is codons 0..9 of frame 0 (3j + 3 <= 32), part 2 codons 10..24 of
    # frame 2 (2 + 3j >= 32, the stop is codon 25).  u = -1: PARTIAL5.  flags = HAS_STOP | PARTIAL5 | INTERRUPTED | MULTI_FRAME | REPAIRED.
    td = text_with([_ATG, _END2])
    out.append(_case("deletion", [_ATG, _END2], _TWO, "repaired", [(32, 0, 2, 10, 11)], (0, 79),
                     b"M" + translate(td[3:30]) + translate(td[32:77]), flags=1 | 2 | 4 | 8 | 128))
    # an insertion: frame 0 then frame 1 (x 37..60).  mid = (26 + 1 + 37) // 2 = 32; part 2 is codons 11..24 of frame 1
    # (1 + 3j >= 32 -> x = 34): nucleotides 32 and 33 give no residue.  The stop is codon 25 of frame 1 (x 76..78).
    ti = text_with([_ATG, (76, b"TAA")])
    out.append(_case("insertion", [_ATG, (76, b"TAA")], [(0, 1, 8, 5), (1, 12, 19, 5)], "repaired", [(32, 0, 1, 10, 10)], (0, 78),
                     b"M" + translate(ti[3:30]) + translate(ti[34:76]), flags=1 | 2 | 4 | 8 | 128))
    # no stop anywhere and no ATG: b = u + 1 = 0 without a start, e = n_2 = 29: the extent ends at the last whole codon
    tn = text_with([])
    out.append(_case("open_ends", [], _TWO, "repaired", [(32, 0, 2, 10, 11)], (0, 88), translate(tn[0:30]) + translate(tn[32:89]),
                     start_codon=0, flags=2 | 4 | 8 | 128))
    # mid clamped to hi: a frame-0 stop at codon 9 (x 27..29) -> hi = 27 < mid.  Part 1 codons 0..8, part 2 from x = 29.
    th = text_with([_ATG, _END2, (27, b"TAA")])
    out.append(_case("clamp_hi", [_ATG, _END2, (27, b"TAA")], _TWO, "repaired", [(27, 0, 2, 9, 11)], (0, 79),
                     b"M" + translate(th[3:27]) + translate(th[29:77]), flags=1 | 2 | 4 | 8 | 128))
    # mid clamped to lo: a frame-2 stop at codon 11 (x 35..37) -> lo = 38 = A_2 > mid.  Part 1 codons 0..11, part 2 from x = 38.
    tl = text_with([_ATG, _END2, (35, b"TAA")])
    out.append(_case("clamp_lo", [_ATG, _END2, (35, b"TAA")], _TWO, "repaired", [(38, 0, 2, 12, 11)], (0, 79),
                     b"M" + translate(tl[3:36]) + translate(tl[38:77]), flags=1 | 2 | 4 | 8 | 128))
    # the narrowest window there is, hi = lo + 1: frame-2 stop at codon 9 (x 29..31, lo = 32), frame-0 stop at codon 11
    # (x 33..35, hi = 33).  J = mid = 32 = lo.
    tw = text_with([_ATG, _END2, (29, b"TAA"), (33, b"TAA")])
    out.append(_case("narrow", [_ATG, _END2, (29, b"TAA"), (33, b"TAA")], _TWO, "repaired", [(32, 0, 2, 10, 11)], (0, 79),
                     b"M" + translate(tw[3:30]) + translate(tw[32:77]), flags=1 | 2 | 4 | 8 | 128))
    # the narrowest failure there is, lo = hi + 7: frame-0 stop at codon 10 (x 30..32, hi = 30), frame-1 stop at codon 11
    # (x 34..36, lo = 37 = A_2)
    out.append(_case("empty_window", [_ATG, (76, b"TAA"), (30, b"TAA"), (34, b"TAA")], [(0, 1, 8, 5), (1, 12, 19, 5)], "failed"))
    # a '*' inside a segment: a frame-0 stop at codon 5 (x 15..17), inside the frame-0 CALL
    ts = text_with([_ATG, _END2, (15, b"TAA")])
    out.append(_case("inner_stop", [_ATG, _END2, (15, b"TAA")], _TWO, "repaired", [(32, 0, 2, 10, 11)], (0, 79),
                     b"M" + translate(ts[3:15]) + b"*" + translate(ts[18:30]) + translate(ts[32:77]), flags=1 | 2 | 4 | 8 | 128, first_inner=5))
    # three segments with overlapping evidence: frame 0 codons 1..12 (x 3..38), frame 1 codon 11 (x 34..36), frame 2 from codon
    # 12 (x 38).  J_1 = (38 + 1 + 34) // 2 = 36 and J_2 = (36 + 1 + 38) // 2 = 37: no codon of frame 1 has 36 <= x and x + 3 <= 37.
    out.append(_case("empty_part", [_ATG, _END2], [(0, 1, 12, 5), (1, 11, 11, 5), (2, 12, 19, 5)], "failed"))
    # the same with frame 2 from codon 11 (x 35): J_2 = (36 + 1 + 35) // 2 = 36 = J_1
    out.append(_case("equal_junctions", [_ATG, _END2], [(0, 1, 12, 5), (1, 11, 11, 5), (2, 11, 19, 5)], "failed"))
    # three segments that hold: frame 0 codons 1..5 (x 3..17), frame 1 codons 8..12 (x 25..39), frame 2 codons 15..19 (x 47..61).
    # J_1 = (17 + 1 + 25) // 2 = 21, J_2 = (39 + 1 + 47) // 2 = 43.  Parts: frame 0 codons 0..6; frame 1 codons 7..13 (22 <= x, x + 3 <= 43);
    # frame 2 codons 14..24 (x >= 44).
    t3 = text_with([_ATG, _END2])
    three = [(0, 1, 5, 5), (1, 8, 12, 5), (2, 15, 19, 5)]
    out.append(_case("three", [_ATG, _END2], three, "repaired", [(21, 0, 1, 7, 7), (43, 1, 2, 14, 7)], (0, 79),
                     b"M" + translate(t3[3:21]) + translate(t3[22:43]) + translate(t3[44:77]), flags=1 | 2 | 4 | 8 | 128))
    # ... skipped with max_junctions = 1
    out.append(_case("skipped", [_ATG, _END2], three, "skipped", max_junctions=1))
    # min_count = 3 hides the middle CALL (count 2): frames 0 and 2 are left, one junction, J = (17 + 1 + 47) // 2 = 32
    hidden = [(0, 1, 5, 5), (1, 8, 12, 2), (2, 15, 19, 5)]
    out.append(_case("min_count", [_ATG, _END2], hidden, "repaired", [(32, 0, 2, 10, 29)], (0, 79),
                     b"M" + translate(t3[3:30]) + translate(t3[32:77]), flags=1 | 2 | 4 | 8 | 128, min_count=3))
    # ... and single when it hides all but one frame
    out.append(_case("single", [_ATG, _END2], [(0, 1, 5, 5), (1, 8, 12, 2), (2, 15, 19, 2)], "single", min_count=3))
    return out


def expected_on(case, strand: int):
    """The case's answers as the records hold them on the given strand: junctions (pos, from, to, res, gap), (left, right)."""
    m = (lambda x: x) if not strand else (lambda x: L - 1 - x)
    junc = [(m(J), a, b, res, gap) for J, a, b, res, gap in case["junctions"]]
    ext = None
    if case["extent"] is not None:
        xs, xe = case["extent"]
        ext = (xs, xe) if not strand else (L - 1 - xe, L - 1 - xs)
    return junc, ext
