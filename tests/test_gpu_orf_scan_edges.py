"""The six scanned planes of the ORF stage (kg_orfs.hpp) with a carried key across every border of their prefix maximum: a thread's
16 items, a wave's 1024, a scan tile's 4096 (and two of them), and the 256 scan tiles of one step of build_tile_scan_kernel.
The batches are those of tests/orf_scan_cases.py, which tests/test_orf_scan_cases_host.py shows to be what they say and to be
sensitive to a broken carry.  Here the device answers them through every reader of the planes: the region kernel (u, e, b, i*),
the free enumerator (outer and its start search, alone and behind caller-held regions) and the repair's two clamps -- byte for
byte against the numpy models, and field by field against the answers the cases state by construction, so that a failure names
the plane and the border."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import free_orfs_model as F  # noqa: E402
import orf_scan_cases as E  # noqa: E402
import orfs_model as O  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    for g, w, name in zip(got, want, ("records", "prot_start", "residues")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, name)


def _host(o, ps, res):
    return o.cpu().numpy().view(N.ORF_DTYPE), ps.cpu().numpy(), res.cpu().numpy()


def _free_of_target(c):
    """the model's free candidates of the batch: the target's alone, since no filler has MIN_RES codons in a frame"""
    want = F.free_orfs(c.target, np.array([0, len(c.target)], np.int64), E.MIN_RES, c.start_codons)
    want[0]["seq"] = c.target_seq
    return want


@pytest.mark.parametrize("family,plane,B", E.ALL, ids=["%s-%s-%d" % (f, E.PLANE_NAMES[p], B) for f, p, B in E.ALL])
def test_a_carried_key_across_the_border(family, plane, B):
    from kmergutsjava_amd import hotpath
    c = E.make(family, plane, B)
    what = "%s: plane %s, border %d, source item %d, read item %d" % (c.name, E.PLANE_NAMES[plane], B, c.src, c.r)
    seq, off = c.batch()
    regs = c.regions()
    want = O.orfs(regs, seq, off, c.start_codons, False)
    got = hotpath.orf_regions(regs, seq, off, c.start_codons, False)
    for k, exp in enumerate(c.expect):
        assert {name: int(got[0][name][k]) for name in exp} == exp, (what, "region %d (%s)" % (k, "i*" if k else E.ROLE[plane]))
    _same(got, want, what)
    _same(_host(*hotpath.orf_regions(regs, seq, off, c.start_codons, False, device_out=True)), want, what)
    if c.free is None:
        return
    want = _free_of_target(c)
    got = hotpath.free_orfs(seq, off, E.MIN_RES, c.start_codons)
    assert (got[0]["seq"] == c.target_seq).all(), (what, "a filler gave a candidate")
    strand, f = c.rows[0][:2]
    mine = got[0][(got[0]["strand"] == strand) & (got[0]["frame"] == f)]
    hit = [o for o in mine if all(int(o[name]) == v for name, v in c.free.items())]
    assert len(hit) == 1, (what, "free candidate", c.free, mine)
    _same(got, want, what)
    _same(_host(*hotpath.free_orfs(seq, off, E.MIN_RES, c.start_codons, device_out=True)), want, what)


@pytest.mark.parametrize("plane", [E.DOWN_FSTOP, E.UP_FSTART])
def test_add_free_behind_caller_held_regions_reads_the_same_planes(plane):
    """kg_orfset_add_free on the TILE batch: the free records behind the regions' are those of kg_orfs_free."""
    from kmergutsjava_amd import hotpath
    import test_gpu_free_orfs as TF
    c = E.make("far", plane, E.TILE)
    seq, off = c.batch()
    sb = np.frombuffer(seq, dtype=np.uint8)
    regs = c.regions()
    parent = O.orfs(regs, seq, off, c.start_codons, False)
    alone = hotpath.free_orfs(seq, off, E.MIN_RES, c.start_codons)
    lib, oh = N.load(), C.c_void_p()
    N.check(lib.kg_orfs_regions(0, C.byref(N.KgOrfParams(c.start_codons, 0, 0)), regs.ctypes.data, len(regs), sb.ctypes.data, off.ctypes.data,
                                len(off) - 1, C.byref(oh)))
    try:
        got = hotpath._take_orfset(TF._add_free(oh, sb, off, E.MIN_RES, c.start_codons), False)
    finally:
        lib.kg_orfset_free(oh)
    assert got[0][len(regs):].tobytes() == alone[0].tobytes() and len(alone[0]) > 0
    _same(got[:3], F.concat(parent, _free_of_target(c)), c.name)


@pytest.mark.parametrize("family,clamp,strand,B", E.REPAIR_ALL, ids=["%s-%s-%d-%d" % x for x in E.REPAIR_ALL])
def test_the_repairs_clamps_across_the_border(family, clamp, strand, B):
    """repair_stop_after (J clamped to hi) and repair_stop_before (J clamped to lo) of a two-segment chain whose stop is a
    carried key: everything against the model as tests/test_gpu_repair.py does it, the junction by construction."""
    import test_gpu_repair as TG
    c = E.repair_case(family, clamp, strand, B)
    want, _ = TG._check(*TG._batch(c.items()), merge_gap=c.merge_gap, start_codons=1)
    assert want[5]["repaired"] == 1 and want[3]["pos"].tolist() == [c.pos], (c.name, E.PLANE_NAMES[c.plane], c.src, c.r)
