"""The batches of tests/orf_scan_cases.py are what they say they are, without a GPU: the layout arithmetic puts the source and the
read on the stated items with the border between them, the tiles between hold nothing of the class, the numpy models and their
plain-loop twins give the answers the cases state by construction, and a scan with a broken carry would give other ones.

The broken-carry twins work on one plane's per-tile keys (orf_scan_cases.plane_keys) and their prefix maximum:
  reset   the running value is dropped at every multiple of B.  It changes the key read at r for tight and far, and leaves the
          no_leak ones alone (there the key in front of the border must NOT arrive).  For superseded it cannot change anything
          at the named border: the second codon sits in the tile at item B, which is where a scan that drops its carry at B
          begins afresh.  What superseded is sensitive to is asserted in its place:
  stale   the key carried into B is handed on unchanged (the nearer key does not replace it): the carried, farther codon answers;
  reset at THREAD  the second codon's key has to pass the thread border at B + 16 in front of r = B + 16."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import free_orfs_model as F  # noqa: E402
import orf_scan_cases as E  # noqa: E402
import orfs_model as O  # noqa: E402
import regions_model as R  # noqa: E402
import repair_model as M  # noqa: E402

ROOT = os.path.dirname(HERE)
T = E.T


def test_the_constants_the_cases_are_built_around():
    csrc = os.path.join(ROOT, "kmergutsjava_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("kg_device.hpp", "kg_build.hpp", "kg_orfs.hpp", "kg_host_orfs.hpp")}

    def const(name, var):
        return int(re.search(r"constexpr int %s = (\d+);" % var, text[name]).group(1))

    assert const("kg_build.hpp", "kBuildItems") == E.THREAD == 16
    assert const("kg_device.hpp", "kWave") * const("kg_build.hpp", "kBuildItems") == E.WAVE == 1024
    assert re.search(r"constexpr int kBuildTile = kBuildThreads \* kBuildItems;", text["kg_build.hpp"])
    assert const("kg_build.hpp", "kBuildThreads") * const("kg_build.hpp", "kBuildItems") == E.TILE == 4096
    assert const("kg_build.hpp", "kBuildThreads") * E.TILE == E.STEP            # build_tile_scan_kernel: kBuildThreads tiles a step
    assert "for (uint32_t b = 0; b < n_tiles; b += kBuildThreads)" in text["kg_build.hpp"]
    assert const("kg_orfs.hpp", "kOrfTile") == E.T
    # the planes' numbers, and which of them are stored mirrored
    enum = re.search(r"enum \{ kOrfDownFStop = 0, kOrfDownRStop = 1, kOrfDownRStart = 2, kOrfUpFStop = 3, kOrfUpFStart = 4, kOrfUpRStop = 5 \}",
                     text["kg_orfs.hpp"])
    assert enum and E.PLANE_NAMES == ("DownFStop", "DownRStop", "DownRStart", "UpFStop", "UpFStart", "UpRStop")
    assert "keys[(uint64_t)(3 + a) * geo.n_tiles + mgt]" in text["kg_orfs.hpp"] and E.MIRRORED == (False,) * 3 + (True,) * 3
    # a thread of the apply kernel takes kBuildItems consecutive items, a scan tile kBuildTile
    assert "(uint64_t)blockIdx.x * kBuildTile + (uint64_t)threadIdx.x * kBuildItems" in text["kg_orfs.hpp"]
    assert "(offsets[k + 1] - offsets[k]) / 3 + kg::kOrfTile - 1) / kg::kOrfTile" in text["kg_host_orfs.hpp"]
    assert max(len(f) for f in E.FILLERS) <= 8 and min(len(f) for f in E.FILLERS) >= 3 and 8 // 3 < E.MIN_RES


def _reset_scan(keys, B):
    """the prefix maximum with the running value dropped at every multiple of B"""
    pad = (-keys.size) % B
    k = np.concatenate([keys, np.full(pad, -1, dtype=np.int64)]).reshape(-1, B)
    return np.maximum.accumulate(k, axis=1).reshape(-1)[:keys.size]


def _check_layout_and_twins(c, seq, off, contig, s, start_codons):
    """what the region / free cases and the repair cases share: c has plane, B, g, src, r, R, t_src, t_sup, t_read, t_query, found"""
    mirrored, n_seqs = E.MIRRORED[c.plane], len(off) - 1
    rows, tb, n_tiles = E.layout(off)
    assert rows[s] == c.R and (np.delete(rows, s) == 1).all()
    assert c.src < c.B <= c.r < n_tiles
    assert E.item_of(off, c.plane, s, c.g, c.t_read) == c.r
    step = -1 if mirrored else 1                            # plane order in forward tiles
    assert c.t_query == c.t_read + step and c.t_query == (0 if mirrored else c.R - 1)
    w = E.wanted_codons(contig, c.plane, c.g, start_codons)
    if c.t_src is None:
        assert w.size == 0 and c.found is None
    else:
        assert E.item_of(off, c.plane, s, c.g, c.t_src) == c.src
        tiles = [c.t_src] + ([c.t_sup] if c.t_sup is not None else [])
        assert sorted((w // T).tolist()) == sorted(tiles) and c.found in w.tolist()
        # nothing of the class strictly between the answer's tile and the query's, nor in the query's
        assert c.found // T == tiles[-1] and (c.t_query - tiles[-1]) * step >= 2
        assert all((c.t_query - t) * step > (c.t_query - tiles[-1]) * step for t in tiles[:-1])
        if c.t_sup is not None:
            assert E.item_of(off, c.plane, s, c.g, c.t_sup) == c.B
    if c.B == E.STEP:
        assert n_tiles > E.STEP
    keys = E.plane_keys(seq, off, c.plane, start_codons)
    assert keys.size == n_tiles
    true = np.maximum.accumulate(keys)
    read = lambda scanned: E.decode(scanned[c.r], c.plane, n_seqs, s, c.g)      # noqa: E731
    assert read(true) == c.found
    assert int(keys[c.src]) & 0x7FFFFFFF, "the source tile holds nothing"
    broken = read(_reset_scan(keys, c.B))
    if c.family in ("tight", "far"):
        assert broken != c.found and broken is None
    elif c.family == "superseded":
        assert broken == (c.found if c.B > E.THREAD else None)                  # (see the module's docstring; r = 48 is a border too)
        stale = E.decode(true[c.B - 1], c.plane, n_seqs, s, c.g)
        assert stale is not None and stale // T == c.t_src and stale != c.found
        assert read(_reset_scan(keys, E.THREAD)) is None
    else:
        assert broken is None and c.found is None
        assert int(true[c.src]) >> 31 != int(true[c.r]) >> 31                   # the key in front is another segment's


@pytest.mark.parametrize("family,plane,B", E.ALL, ids=["%s-%s-%d" % (f, E.PLANE_NAMES[p], B) for f, p, B in E.ALL])
def test_region_and_free_cases(family, plane, B):
    c = E.make(family, plane, B)
    seq, off = c.batch()
    s, L = c.target_seq, len(c.target)
    assert seq[off[s]:off[s + 1]] == c.target and c.front + c.back + bool(c.near_front) + bool(c.near_back) + 1 == len(off) - 1
    lens = np.diff(off)
    assert (np.delete(lens, s) >= 3).all() and (np.delete(lens, s) <= 8).all()          # every filler lies where the case says
    mirrored = E.MIRRORED[plane]
    if family.startswith("no_leak"):
        # the segment in front in plane order, and its last tile there
        if family == "no_leak_phase":
            sp, gp, tp = s, c.g + (1 if mirrored else -1), (0 if mirrored else c.R - 1)
            assert E.item_of(off, plane, s, c.g, c.R - 1 if mirrored else 0) == B
        else:
            sp, gp, tp = (s + 1, 0, 0) if mirrored else (s - 1, 2, 0)
            assert E.item_of(off, plane, s, c.g, c.R - 1 if mirrored else 0) == B - B % 3 and c.g == (2 if mirrored else 0)
        assert E.item_of(off, plane, sp, gp, tp) == c.src == E.item_of(off, plane, s, c.g, c.R - 1 if mirrored else 0) - 1
        assert E.wanted_codons(seq[off[sp]:off[sp + 1]], plane, gp, c.start_codons).size > 0
    _check_layout_and_twins(c, seq, off, c.target, s, c.start_codons)
    # the models: the numpy form on the batch, the plain loops on the target alone
    regs = c.regions()
    want = O.orfs(regs, seq, off, c.start_codons, False)
    for k, exp in enumerate(c.expect):
        assert {name: int(want[0][name][k]) for name in exp} == exp, (c.name, k)
    alone = regs.copy()
    alone["seq"] = 0
    brute = O.brute_force(alone, c.target, np.array([0, L]), c.start_codons, False)
    brute[0]["seq"] = s
    assert all(a.tobytes() == b.tobytes() for a, b in zip(brute, want))
    if E.HAS_FREE[plane]:
        free = F.free_orfs(c.target, np.array([0, L]), E.MIN_RES, c.start_codons)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(F.brute_force(c.target, np.array([0, L]), E.MIN_RES, c.start_codons), free))
        strand, f = c.rows[0][:2]
        mine = free[0][(free[0]["strand"] == strand) & (free[0]["frame"] == f)]
        hit = [o for o in mine if all(int(o[name]) == v for name, v in c.free.items())]
        assert len(hit) == 1 and int(hit[0]["fI"]) == -1, c.name
    else:
        assert c.free is None


@pytest.mark.parametrize("family,clamp,strand,B", E.REPAIR_ALL, ids=["%s-%s-%d-%d" % x for x in E.REPAIR_ALL])
def test_repair_cases(family, clamp, strand, B):
    import test_gpu_repair as TG
    c = E.repair_case(family, clamp, strand, B)
    calls, seq, off = TG._batch(c.items())
    s = c.target_seq
    contig = seq[off[s]:off[s + 1]].tobytes()
    _check_layout_and_twins(c, seq, off, contig, s, 0)
    regs, _ = R.regions(calls, off, merge_gap=c.merge_gap, min_score=0)
    assert len(regs) == 1 and regs["seq"][0] == s
    o, ps, res = O.orfs(regs, seq, off, start_codons=1)
    want = M.repair(regs, o, ps, res, calls, seq, off, start_codons=1)
    brute = M.brute_force(regs, o, ps, res, calls, seq, off, start_codons=1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(want[:5], brute[:5])) and want[5] == brute[5]
    assert want[5]["repaired"] == 1 and want[3]["pos"].tolist() == [c.pos], c.name
