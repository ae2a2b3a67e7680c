"""Frameshift repair (kg_regionset_repair) at the edges its first tests leave alone, as builders shared by
tests/test_repair_edges_host.py (which shows on the CPU that every case is what it says) and tests/test_gpu_repair_edges.py:

  A  chains at the junction bound: 8, 9 and 10 segments, a ninth part that is empty, junctions 7 and 8 out of order
  B  residue lanes across ORF borders: the end of a nine-part protein, not-kept regions and a copied protein in one lane
  C  searches over one tile row and more for every end of a chain (start, no start, first inner stop of parts 1 and 2, end)
     on contigs of 8 T codons with all three lengths mod 3, behind and in front of fillers of three tile rows
  D  a second call on a set that already holds repaired records

Every case is (text on its strand, strand, CALLs on the strand) for repair_cases.lay, with the answers it claims by
construction.  The background is GCA repeated as in repair_cases.py: no stop and no start in any frame of the strand until one
is planted.  Imports nothing from kmergutsjava_amd but the record dtypes and two constants."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd import _native as N

import repair_cases as RC
import repair_model as M

T = N.ORF_TILE_CODONS
MAX_J = N.REPAIR_MAX_JUNCTIONS
LANE = 8                            # kg_orfs.hpp kOrfResPerLane: the residues one lane of repair_residues_kernel writes
TAILS = (b"", b"G", b"GC")
CYCLES = ((0, 1, 2), (0, 2, 1))


def put(text: bytearray, f: int, j: int, codon: bytes) -> None:
    text[f + 3 * j:f + 3 * j + 3] = codon


def on_contig(L: int, strand: int, xs: int, xe: int):
    """a strand extent as (left, right) of the record"""
    return (xs, xe) if not strand else (L - 1 - xe, L - 1 - xs)


def _case(name, text, strand, calls, state, **kw):
    return dict(name="%s%s" % (name, "-" if strand else "+"), text=bytes(text), strand=strand, calls=list(calls), state=state, **kw)


def assert_answers(c, rec, junc) -> None:
    """The record and the junction records of a repaired case against what the case states; a failure names the case."""
    name = c["name"]
    assert int(rec["flags"]) & M.REPAIRED, (name, "not repaired", rec)
    assert junc["pos"].tolist() == c["pos"] and junc["res"].tolist() == c["res"], (name, junc, c["pos"], c["res"])
    assert (int(rec["left"]), int(rec["right"])) == (c["left"], c["right"]), (name, rec, c["left"], c["right"])
    assert (int(rec["start_codon"]), int(rec["first_inner"])) == (c["start_codon"], c["first_inner"]), (name, rec)
    assert bool(int(rec["flags"]) & M.PARTIAL5) == c["partial5"] and bool(int(rec["flags"]) & M.HAS_STOP) == c["has_stop"], (name, rec)
    assert "n_res" not in c or int(rec["n_res"]) == c["n_res"], (name, rec)


def assert_states(states, orfs, jstart, what) -> None:
    """One region per contig: region k is repaired, with junctions, exactly when states[k] says so."""
    assert len(orfs) == len(states), (what, len(orfs), len(states))
    for k, state in enumerate(states):
        rep = bool(int(orfs["flags"][k]) & M.REPAIRED)
        assert rep == (state == "repaired") and (jstart[k + 1] > jstart[k]) == rep, (what, k, state, orfs[k])


# ---- A: chains at the bound -------------------------------------------------------------------------------------------------------------

def chain_text(tail: bytes) -> bytearray:
    return bytearray(b"ATG" + b"GCA" * 99 + tail)


def chain_calls(m: int, cyc):
    return [(cyc[k % 3], 2 + 8 * k, 6 + 8 * k, 3) for k in range(m)]


def by_mid(L: int, calls, e=None):
    """A chain whose every CALL is a segment of its own, on a text without a stop that bounds a junction and with ATG at codon 0
    of the first frame (which is 0): J_k is the middle of the evidence gap, b = 0, and e as given or n_f.
    -> (J, [(first codon, length) of every part])"""
    segs = [(f, f + 3 * a, f + 3 * z + 2) for f, a, z, _ in calls]
    J = [(segs[k][2] + 1 + segs[k + 1][1]) // 2 for k in range(len(segs) - 1)]
    parts = []
    for k, (f, _, _) in enumerate(segs):
        jf = 0 if k == 0 else -((f - J[k - 1]) // 3)
        je = ((L - f) // 3 if e is None else e) if k == len(segs) - 1 else (J[k] - f) // 3
        parts.append((jf, je - jf))
    return J, parts


def _chain(name, tail, strand, calls, state, puts=(), e=None, max_junctions=MAX_J, **extra):
    text = chain_text(tail)
    for f, j, codon in puts:
        put(text, f, j, codon)
    L = len(text)
    J, parts = by_mid(L, calls, e)
    c = _case(name, text, strand, calls, state, params=dict(max_junctions=max_junctions), J=J, parts=parts, **extra)
    if state == "repaired":
        fm = calls[-1][0]
        left, right = on_contig(L, strand, 0, fm + 3 * ((L - fm) // 3 - 1) + 2)
        c.update(pos=[x if not strand else L - 1 - x for x in J], res=np.cumsum([n for _, n in parts])[:-1].tolist(), left=left, right=right,
                 n_res=sum(n for _, n in parts), start_codon=1, first_inner=-1, partial5=True, has_stop=False)
    return c


def chain_cases(tail: bytes, strand: int):
    """The chains of one (tail, strand): 8 and 9 segments repair with max_junctions = 8 (7 and 8 junctions), 10 are skipped and so
    are 9 with max_junctions = 7; for the cycle 0, 1, 2 also three nine-segment chains that fail at the chain's end."""
    tag = "tail%d" % len(tail)
    out = []
    for cyc in CYCLES:
        cn = "%s-%d%d%d" % (tag, *cyc)
        out.append(_chain("chain8-" + cn, tail, strand, chain_calls(8, cyc), "repaired"))
        out.append(_chain("chain9-" + cn, tail, strand, chain_calls(9, cyc), "repaired"))
        out.append(_chain("chain10-" + cn, tail, strand, chain_calls(10, cyc), "skipped"))
        out.append(_chain("chain9-of-7-" + cn, tail, strand, chain_calls(9, cyc), "skipped", max_junctions=MAX_J - 1))
    base = chain_calls(6, CYCLES[0])                  # frames 0 1 2 0 1 2; the last one ends at x = 142
    # frame 1 codons 58..68 (C = 207) reach over the ninth segment, frame 2 codon 66 alone (A = 200, C = 202), and frame 2 stops at
    # codon 67: J_8 = (207 + 1 + 200) // 2 = 204, the ninth part would begin at codon 68 and e = 67.  The first eight parts hold, so
    # the record loop fails on its ninth trip.
    out.append(_chain("empty-ninth-" + tag, tail, strand, base + [(0, 50, 54, 3), (1, 58, 68, 3), (2, 66, 66, 3)], "failed",
                      puts=[(2, 67, b"TAA")], e=67, bad_part=8))
    # repair_cases' empty_part at the chain's end: frame 0 codons 50..61 (C = 185), frame 1 codon 60 (x 181..183), frame 2 from
    # codon 61 (A = 185): J_7 = 183, J_8 = 184, and no codon of frame 1 has 183 <= x and x + 3 <= 184
    out.append(_chain("empty-eighth-" + tag, tail, strand, base + [(0, 50, 61, 3), (1, 60, 60, 3), (2, 61, 70, 3)], "failed", bad_part=7))
    # ... and its equal_junctions: frame 2 from codon 60 (A = 182) gives J_8 = (183 + 1 + 182) // 2 = 183 = J_7
    out.append(_chain("junctions-7-8-" + tag, tail, strand, base + [(0, 50, 61, 3), (1, 60, 60, 3), (2, 60, 70, 3)], "failed", bad_junction=6))
    return out


def interleaved(cases, strand: int):
    """The chains that take max_junctions = 8 between repair_cases' parameter-free ones on alternating strands: eight-junction
    ORFs between copied and one-junction ones.  -> (items for test_gpu_repair._batch, the state of every contig's region)"""
    plain = [c for c in RC.cases() if not c["params"]]
    items, states = [], []
    for k, c in enumerate(c for c in cases if c["params"] == dict(max_junctions=MAX_J)):
        p = plain[k % len(plain)]
        items += [(p["text"], (strand + k) & 1, p["calls"]), (c["text"], c["strand"], c["calls"])]
        states += [p["state"], c["state"]]
    return items, states


# ---- B: lanes across ORF borders --------------------------------------------------------------------------------------------------------

LANE_MIN_SCORE = 5


def lane_batch(p: int):
    """p one-junction ORFs of 25 residues (25 = 1 mod 8: the next protein begins at p mod 8), a nine-part chain, two regions below
    min_score = 5 (not kept: zero-length proteins under only_kept), a single-frame region.
    -> (items, index of the chain, its answers)"""
    one = RC.cases()[0]
    assert one["name"] == "deletion" and len(one["protein"]) == 25
    chain = _chain("lane-chain-%d" % p, b"", p & 1, chain_calls(9, CYCLES[0]), "repaired")
    items = [(one["text"], k & 1, one["calls"]) for k in range(p)]
    items.append((chain["text"], chain["strand"], chain["calls"]))
    items += [(one["text"], k & 1, [(0, 1, 8, 1), (2, 12, 19, 1)]) for k in range(2)]          # score 2
    items.append((one["text"], 0, [(0, 1, 8, 5)]))
    return items, p, chain


# ---- C: far ends ------------------------------------------------------------------------------------------------------------------------

FILLER = b"GCA" * (2 * T + 7) + b"TAATGA"         # 2 T + 9 codons: three tile rows
N_TARGET = 8 * T


def _target(tail: bytes) -> bytearray:
    return bytearray(b"GCA" * N_TARGET + tail)


def _far(name, tail, strand, text, calls, xs, xe, search, d, **kw):
    """search: (frame, the search's first codon, its answer or None) on the strand"""
    L = len(text)
    (f1, _, z1, _), (f2, a2, _, _) = calls
    J = (f1 + 3 * z1 + 2 + 1 + f2 + 3 * a2) // 2              # no stop bounds the junction in any of these
    left, right = on_contig(L, strand, xs, xe)
    return _case("%s-d%s-tail%d" % (name, d, len(tail)), text, strand, calls, "repaired", left=left, right=right,
                 pos=[J if not strand else L - 1 - J], search=search, d=d, **kw)


def far_cases(tail: bytes, strand: int):
    """Every family and distance of one (tail, strand), for start_codons = 1."""
    out = []
    n2 = (3 * N_TARGET + len(tail) - 2) // 3
    for d in (0, T - 1, T, T + 1, 2 * T + 1):
        # start: frame 0 stops at u, ATG d codons behind u + 1, evidence 2 T + 32 codons behind u
        u = T + 1
        j0 = u + 2 * T + 32
        t = _target(tail)
        put(t, 0, u, b"TAA")
        put(t, 0, u + 1 + d, b"ATG")
        put(t, 2, j0 + 57, b"TAA")
        out.append(_far("start", tail, strand, t, [(0, j0, j0 + 5, 3), (2, j0 + 12, j0 + 17, 3)], 3 * (u + 1 + d), 2 + 3 * (j0 + 57) + 2,
                        (0, u + 1, u + 1 + d), d, start_codon=1, first_inner=-1, partial5=False, has_stop=True, res=[j0 + 9 - (u + 1 + d)]))
        # inner stop of part 1: ATG at b0 (no stop in front of it), a frame-0 CALL of 2 T + 22 codons from b0, a stop d codons in
        b0 = T + 2
        z = b0 + 2 * T + 21
        t = _target(tail)
        put(t, 0, b0, b"ATG")
        if d:
            put(t, 0, b0 + d, b"TAA")
        put(t, 2, z + 57, b"TAA")
        out.append(_far("inner1", tail, strand, t, [(0, b0, z, 3), (2, z + 12, z + 17, 3)], 3 * b0, 2 + 3 * (z + 57) + 2,
                        (0, b0, b0 + d if d else None), d, start_codon=1, first_inner=d if d else -1, partial5=True, has_stop=True,
                        res=[z + 6 - b0]))          # C = 3 z + 2, A = 3 z + 38: J = 3 z + 20
        # inner stop of part 2: frame 0 codons T - 4 .. T + 1, frame 2 from codon T + 2 on: C = 3 T + 5, A = 3 T + 8, J = 3 T + 7
        # and part 2 begins at codon ceil((J - 2) / 3) = T + 2, six residues into the protein
        g = T + 2
        z = g + 2 * T + 21
        t = _target(tail)
        put(t, 0, T - 4, b"ATG")
        if d:
            put(t, 2, g + d, b"TAA")
        put(t, 2, z + 40, b"TAA")
        out.append(_far("inner2", tail, strand, t, [(0, T - 4, T + 1, 3), (2, g, z, 3)], 3 * (T - 4), 2 + 3 * (z + 40) + 2,
                        (2, g, g + d if d else None), d, start_codon=1, first_inner=6 + d if d else -1, partial5=True, has_stop=True, res=[6]))
    for d in (1, T - 1, T, T + 1, 2 * T + 1, None):
        # no start: the last frame-0 stop d codons in front of j0 (None: no stop at all), and no ATG
        j0 = 3 * T + 33
        t = _target(tail)
        if d:
            put(t, 0, j0 - d, b"TAA")
        put(t, 2, j0 + 57, b"TAA")
        b = j0 - d + 1 if d else 0
        out.append(_far("nostart", tail, strand, t, [(0, j0, j0 + 5, 3), (2, j0 + 12, j0 + 17, 3)], 3 * b, 2 + 3 * (j0 + 57) + 2,
                        (0, j0 - 1, j0 - d if d else None), d, start_codon=0, first_inner=-1, partial5=d is None, has_stop=True,
                        res=[j0 + 9 - b]))
        # end: the first frame-2 stop d codons behind jl = T + 2 (None: no stop, the extent ends at the last whole codon)
        a = T - 15
        jl = a + 17
        t = _target(tail)
        put(t, 0, a, b"ATG")
        if d:
            put(t, 2, jl + d, b"TAA")
        last = jl + d if d else n2 - 1
        out.append(_far("end", tail, strand, t, [(0, a, a + 5, 3), (2, a + 12, jl, 3)], 3 * a, 2 + 3 * last + 2,
                        (2, jl + 1, jl + d if d else None), d, start_codon=1, first_inner=-1, partial5=True, has_stop=d is not None,
                        res=[9]))
    return out


def far_batch(cases, strand: int):
    """One contig per case, each between two fillers: every target's tile_base and tile count are larger than one."""
    items = [(FILLER, strand, [])]
    for c in cases:
        items += [(c["text"], c["strand"], c["calls"]), (FILLER, strand, [])]
    return items


# ---- D: a second pass -------------------------------------------------------------------------------------------------------------------

def second_pass_cases():
    """Each: the items of a batch, the parameters of the second call, and the state of every region in it.  The first call runs
    with the defaults and start_codons = 1 and repairs every region."""
    by_name = {c["name"]: c for c in RC.cases()}
    three, single, two = by_name["three"], by_name["single"], by_name["deletion"]
    i3 = lambda s: (three["text"], s, three["calls"])            # noqa: E731
    i2 = lambda s: (two["text"], s, two["calls"])                # noqa: E731
    out = []
    for s in (0, 1):
        out.append(dict(name="skipped%d" % s, items=[i3(s)], params=dict(max_junctions=1), states=["skipped"]))
        out.append(dict(name="single%d" % s, items=[(single["text"], s, single["calls"])], params=dict(min_count=3), states=["single"]))
        out.append(dict(name="again%d" % s, items=[i3(s)], params=dict(), states=["repaired"]))
        out.append(dict(name="two-three%d" % s, items=[i2(s), i3(1 - s)], params=dict(max_junctions=1), states=["repaired", "skipped"]))
        out.append(dict(name="three-two%d" % s, items=[i3(s), i2(1 - s)], params=dict(max_junctions=1), states=["skipped", "repaired"]))
    return out


def segments_of(calls, min_count: int) -> int:
    """the number of segments of a region whose CALLs these all are: (frame, first codon, last codon, count) on the strand"""
    frames = [f for _, f, cnt in sorted((f + 3 * a, f, cnt) for f, a, _, cnt in calls) if cnt >= min_count]
    return sum(1 for k, f in enumerate(frames) if k == 0 or frames[k - 1] != f)


assert M.REPAIRED == N.ORF_REPAIRED
