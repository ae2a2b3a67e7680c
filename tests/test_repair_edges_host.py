"""The cases of tests/repair_edge_cases.py on the CPU (no GPU): both forms of the model agree on every one to the byte, every
case takes the path it names, and two restatements show that the cases can see what they are aimed at.

`residues_by_rule` is repair_residues_kernel's rule in numpy, from the records and junction records alone: with the kernel's
bound of 8 junction records it gives the model's residues everywhere; with 7 it differs on the nine-part chains and on nothing
else.  Keyed on the record's KG_ORF_REPAIRED flag instead of on the ORF's junction count, the same rule re-translates a record
that a second call leaves alone, and `junction_slots`, the guard of repair_junction_records_kernel, addresses slots that belong
to the next ORF or to nobody; keyed on the junction count both give the model's bytes."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import orfs_model as O  # noqa: E402
import regions_model as R  # noqa: E402
import repair_cases as RC  # noqa: E402
import repair_edge_cases as E  # noqa: E402
import repair_model as M  # noqa: E402
from test_gpu_repair import _batch  # noqa: E402
from test_repair_host import same  # noqa: E402

T = E.T
TAIL_STRAND = [(t, s) for t in E.TAILS for s in (0, 1)]
IDS = ["tail%d%s" % (len(t), "-" if s else "+") for t, s in TAIL_STRAND]


def both(calls, seq, off, min_score=0, only_kept=True, what="", **kw):
    """-> (the model's result, the given set): both forms of the model, byte for byte"""
    regs, _ = R.regions(calls, off, min_score=min_score)
    o, ps, res = O.orfs(regs, seq, off, start_codons=kw.get("start_codons", 7), only_kept=only_kept)
    a = M.repair(regs, o, ps, res, calls, seq, off, **kw)
    same(a, M.brute_force(regs, o, ps, res, calls, seq, off, **kw), what)
    return a, (regs, o, ps, res)


def residues_by_rule(orfs, ps, junc, jstart, given_ps, given_res, seq, off, bound=E.MAX_J, key="junctions"):
    out = np.zeros(int(ps[-1]), dtype=np.uint8)
    for i, o in enumerate(orfs):
        n = int(ps[i + 1] - ps[i])
        js, je = int(jstart[i]), int(jstart[i + 1])
        if n == 0:
            continue
        if not (je > js if key == "junctions" else int(o["flags"]) & M.REPAIRED):
            out[ps[i]:ps[i + 1]] = given_res[given_ps[i]:given_ps[i] + n]
            continue
        s, strand = int(o["seq"]), int(o["strand"])
        L = int(off[s + 1] - off[s])
        codes = O.strand_codes(seq[off[s]:off[s + 1]], strand)
        recs = junc[js:min(je, js + bound)]
        q = np.arange(n, dtype=np.int64)
        part = (recs["res"].astype(np.int64)[None, :] <= q[:, None]).sum(axis=1)
        x = (L - 1 - int(o["right"]) if strand else int(o["left"])) + 3 * q
        if len(recs):
            jr = recs[np.maximum(part, 1) - 1]
            to = jr["to_frame"].astype(np.int64)
            J = L - 1 - jr["pos"].astype(np.int64) if strand else jr["pos"].astype(np.int64)
            x = np.where(part > 0, to + 3 * ((J - to + 2) // 3 + q - jr["res"]), x)
        c0, c1, c2 = codes[x], codes[x + 1], codes[x + 2]
        ch = np.where((c0 < 4) & (c1 < 4) & (c2 < 4), O._LETTER[(c0 % 4) * 16 + (c1 % 4) * 4 + c2 % 4], ord("X")).astype(np.uint8)
        if int(o["start_codon"]):
            ch[0] = ord("M")
        out[ps[i]:ps[i + 1]] = ch
    return out


def junction_slots(orfs, jstart, n_segments, key):
    """(ORF, slot) of every junction record the kernel's guard lets through: one lane per segment in front of its region's last"""
    out = []
    for i, o in enumerate(orfs):
        if (jstart[i + 1] > jstart[i] if key == "junctions" else int(o["flags"]) & M.REPAIRED):
            out += [(i, int(jstart[i]) + k) for k in range(n_segments[i] - 1)]
    return out


def rule_holds(a, given, seq, off, what, nine_parts=()):
    """bound 8 gives the model's residues; bound 7 differs in exactly the ORFs of nine parts"""
    _, _, gps, gres = given
    assert residues_by_rule(a[0], a[1], a[3], a[4], gps, gres, seq, off).tobytes() == a[2].tobytes(), what
    short = residues_by_rule(a[0], a[1], a[3], a[4], gps, gres, seq, off, bound=E.MAX_J - 1)
    differs = [i for i in range(len(a[0])) if short[a[1][i]:a[1][i + 1]].tobytes() != a[2][a[1][i]:a[1][i + 1]].tobytes()]
    assert differs == list(nine_parts) == [i for i in range(len(a[0])) if a[4][i + 1] - a[4][i] == E.MAX_J], (what, differs)


def test_constants_match_the_kernels():
    src = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_orfs.hpp")).read()
    assert "constexpr int kOrfResPerLane = %d;" % E.LANE in src and "constexpr int kOrfTile = %d;" % T in src
    assert E.MAX_J == 8 and len(E.FILLER) // 3 > 2 * T


@pytest.mark.parametrize("tail,strand", TAIL_STRAND, ids=IDS)
def test_chains_at_the_bound(tail, strand):
    cases = E.chain_cases(tail, strand)
    assert sorted(c["state"] for c in cases) == ["failed"] * 3 + ["repaired"] * 4 + ["skipped"] * 4
    for c in cases:
        calls, seq, off = RC.lay(c["text"], strand, c["calls"])
        a, given = both(calls, seq, off, start_codons=1, what=c["name"], **c["params"])
        st = a[5]
        assert st["candidates"] == 1 and st[c["state"]] == 1, (c["name"], st)
        lens = [n for _, n in c["parts"]]
        if c["state"] == "repaired":
            E.assert_answers(c, a[0][0], a[3])
            assert st["junctions"] == len(c["calls"]) - 1 and min(lens) > 0 and c["J"] == sorted(set(c["J"]))
            if len(c["calls"]) == 9 and "012" in c["name"]:
                assert c["res"] == [8, 15, 22, 29, 36, 43, 50, 57] and {r % E.LANE for r in c["res"]} == set(range(E.LANE))
        elif c["state"] == "skipped":
            assert len(c["calls"]) - 1 > c["params"]["max_junctions"] and len(c["calls"]) in (9, 10)
        elif "bad_part" in c:
            # the junctions are in order and the named part is the only empty one
            assert len(c["calls"]) == 9 and c["J"] == sorted(set(c["J"])) and [k for k, n in enumerate(lens) if n <= 0] == [c["bad_part"]]
        else:
            k = c["bad_junction"]
            assert len(c["calls"]) == 9 and k == 6 and c["J"][k] >= c["J"][k + 1] and c["J"][:k + 1] == sorted(set(c["J"][:k + 1]))
        nine = [0] if c["state"] == "repaired" and len(c["calls"]) == 9 else []
        rule_holds(a, given, seq, off, c["name"], nine)
        if c["state"] == "failed":
            # without what makes it fail the same CALLs repair: it is the chain's end that fails, not its layout
            plain = RC.lay(bytes(E.chain_text(tail)), strand, c["calls"][:7] + E.chain_calls(9, E.CYCLES[0])[7:])
            assert both(*plain, start_codons=1, **c["params"])[0][5]["repaired"] == 1
    items, states = E.interleaved(cases, strand)
    calls, seq, off = _batch(items)
    a, given = both(calls, seq, off, start_codons=1, max_junctions=E.MAX_J, what="interleaved")
    E.assert_states(states, a[0], a[4], "interleaved")
    assert (np.diff(a[4]) == E.MAX_J).sum() == 2 and a[5]["skipped"] == 2 and a[5]["failed"] >= 3
    # the eight-junction ORFs stand between one-junction ones where junction_start is not 0, and copied records are among them
    d = np.diff(a[4]).tolist()
    assert all(a[4][k] > 0 and d[k - 1] == 1 and d[k + 1] == 1 for k in range(len(d)) if d[k] == E.MAX_J) and d.count(0) >= 5, d
    rule_holds(a, given, seq, off, "interleaved", [k for k, n in enumerate(d) if n == E.MAX_J])


@pytest.mark.parametrize("only_kept", [True, False])
def test_lanes_across_orf_borders(only_kept):
    shared = 0
    for p in range(E.LANE):
        items, at, chain = E.lane_batch(p)
        calls, seq, off = _batch(items)
        a, given = both(calls, seq, off, min_score=E.LANE_MIN_SCORE, only_kept=only_kept, start_codons=1, max_junctions=E.MAX_J, what="lane %d" % p)
        regs = given[0]
        assert a[5] == dict(candidates=p + 1, repaired=p + 1, failed=0, single=0, skipped=0, junctions=p + E.MAX_J, residues=25 * p + chain["n_res"])
        assert regs["kept"].tolist() == [1] * (p + 1) + [0, 0, 1] and a[1][at] % E.LANE == p
        E.assert_answers(chain, a[0][at], a[3][a[4][at]:a[4][at + 1]])
        lens = np.diff(a[1])
        assert (lens[at + 1:at + 3] == 0).all() == only_kept and lens[at + 3] > 0 and not a[0]["flags"][at + 3] & M.REPAIRED
        # one lane holds the chain's last residue, the not-kept regions' proteins (of length 0 under only_kept) and the first residue
        # of the copied one -- unless the chain ends on a lane border, which it does for exactly one p
        end = int(a[1][at + 1])
        assert not only_kept or a[1][at + 3] == end
        shared += end % E.LANE != 0
        rule_holds(a, given, seq, off, "lane %d" % p, [at])
    assert shared == E.LANE - 1


def _tiles_of_search(c):
    """the tiles (of the forward phase the device walks) of the search's first codon and of its answer, and that phase"""
    L, strand = len(c["text"]), c["strand"]
    f, first, answer = c["search"]
    n = (L - f) // 3
    g = (L - f) % 3 if strand else f
    fwd = (lambda j: n - 1 - j) if strand else (lambda j: j)
    return fwd(first) // T, None if answer is None else fwd(answer) // T, g, f


@pytest.mark.parametrize("tail,strand", TAIL_STRAND, ids=IDS)
def test_far_ends(tail, strand):
    cases = E.far_cases(tail, strand)
    assert len(cases) == 27 and all(len(c["text"]) == 3 * 8 * T + len(tail) for c in cases)
    for sc, sel in ((1, cases), (0, [c for c in cases if c["name"].startswith("nostart")])):
        calls, seq, off = _batch(E.far_batch(sel, strand))
        a, given = both(calls, seq, off, start_codons=sc, what="far ends, start_codons %d" % sc)
        E.assert_states(["repaired"] * len(sel), a[0], a[4], "far ends")
        assert a[0]["seq"].tolist() == list(range(1, 2 * len(sel), 2))         # every target between two fillers
        for k, c in enumerate(sel):
            E.assert_answers(c, a[0][k], a[3][a[4][k]:a[4][k + 1]])
        rule_holds(a, given, seq, off, "far ends")
    for c in cases:
        t0, t1, g, f = _tiles_of_search(c)
        if c["d"] is not None and c["d"] >= T - 1:
            assert t1 is not None and t0 != t1, (c["name"], t0, t1)
        if c["d"] == 2 * T + 1:
            assert abs(t0 - t1) >= 2, (c["name"], t0, t1)
        if strand and tail:
            assert g != (-f) % 3, c["name"]
    # the rows of a filler and of a target: tile_base and the tile count of every target are larger than one
    rows = (np.diff(off) // 3 + T - 1) // T
    assert rows[0] == 3 and rows[1] >= 8 and (rows > 1).all()


@pytest.mark.parametrize("case", E.second_pass_cases(), ids=lambda c: c["name"])
@pytest.mark.parametrize("key", ["junctions", "flag"])
def test_a_second_pass(case, key):
    calls, seq, off = _batch(case["items"])
    first, given = both(calls, seq, off, start_codons=1, what=case["name"])
    regs = given[0]
    assert first[5]["repaired"] == len(case["items"]) and (first[0]["flags"] & M.REPAIRED).all()
    kw = dict(start_codons=1, **case["params"])
    a = M.repair(regs, first[0], first[1], first[2], calls, seq, off, **kw)
    same(a, M.brute_force(regs, first[0], first[1], first[2], calls, seq, off, **kw), case["name"])
    for k, state in enumerate(case["states"]):
        # the record and the protein stay whatever the state; the junction list is the second call's alone
        assert a[0][k].tobytes() == first[0][k].tobytes() and a[4][k + 1] - a[4][k] == (first[4][k + 1] - first[4][k] if state == "repaired" else 0)
    assert a[1].tobytes() == first[1].tobytes() and a[2].tobytes() == first[2].tobytes()
    assert [a[5][s] for s in ("repaired", "skipped", "single")] == [case["states"].count(s) for s in ("repaired", "skipped", "single")]
    n_segments = [E.segments_of(it[2], kw.get("min_count", 0)) for it in case["items"]]
    slots = junction_slots(a[0], a[4], n_segments, key)
    res = residues_by_rule(a[0], a[1], a[3], a[4], first[1], first[2], seq, off, key=key)
    left_alone = [k for k, s in enumerate(case["states"]) if s != "repaired"]
    if key == "junctions" or not left_alone:
        assert slots == [(int(j["orf"]), k) for k, j in enumerate(a[3])] and res.tobytes() == a[2].tobytes()
    else:
        # keyed on the flag: a record left alone is translated straight through, and a skipped one's junction records go to
        # slots behind its own (empty) range: the next ORF's, or behind the array's end
        assert res.tobytes() != a[2].tobytes()
        for k in left_alone:
            assert res[a[1][k]:a[1][k + 1]].tobytes() != first[2][first[1][k]:first[1][k + 1]].tobytes()
        wild = [(i, s) for i, s in slots if s >= a[4][i + 1]]
        assert len(wild) == sum(n_segments[k] - 1 for k in left_alone)
        if "skipped" in case["states"]:
            assert wild and max(s for _, s in wild) >= len(a[3])


def test_the_kernel_that_keeps_repaired_proteins_uses_no_scratch():
    """From the compiler's own report (tools/kernel_resources.py), as tests/test_kernel_resources.py reads it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not found")
    res = kr.resources()
    for k in ("orf_keep_repaired_kernel", "repair_junction_records_kernel", "repair_residues_kernel"):
        assert k in res, (k, sorted(res))
        assert res[k]["sgpr_spills"] == 0 and res[k]["vgpr_spills"] == 0 and res[k]["scratch"] == 0, (k, res[k])
