"""Deterministic CALL lists at the size edges of the region stage (kg_regions.hpp / kg_host_regions.hpp), shared by
tests/test_regions_host.py (the numpy model against plain loops, no GPU) and tests/test_gpu_size_edges.py (the device against
those references).  Imports nothing from kmergutsjava_amd but the record dtype.

The edges: region_heads_kernel carries the running maximum over thread slices of 16 items, wave slices of 1024 and tiles of
4096, and build_tile_scan_kernel over steps of 256 tiles; region_walk_kernel loads 16 items ahead and takes everything past n
for a head; the four sorts take left_bits = bits_for(l_max), 32 + bits_for(2 n_seqs), 33 + left_bits and
left_bits + bits_for(n_seqs) key bits, eight or fewer a pass.

An item's position in group order is controlled the way the derive tests control theirs.  Group order is (contig, strand, fI,
x0, index): `lead` filler CALLs, each with an fI of its own, lie on contig 0, and the group under test lies on contig 1, so it
starts at item `lead` exactly.  calls[] order is container order and otherwise shuffled, so that it is never group order.

A family is a function of the values of its edge; make(family, values) -> Case, CASES[family] lists the values the tests run."""
from typing import NamedTuple

import numpy as np

from kmergutsjava_amd._native import CALL_DTYPE

THREAD, WAVE, TILE = 16, 1024, 4096       # items per thread and per wave of region_heads_kernel, per workgroup
STEP = 256 * TILE                         # items per step of build_tile_scan_kernel
WALK = 16                                 # kRegionWalk
WEIGHTS = np.array([2.0 ** 24, 1.0, 0.5, 0.1], np.float32)      # float32 sums of these depend on the order
INT_MAX = 2 ** 31 - 1
FI = 7                                    # the function of the group under test


class Case(NamedTuple):
    name: str
    calls: np.ndarray
    offsets: np.ndarray
    merge_gap: int
    min_score: int
    min_len: int
    expect: dict        # "regions": their number; "group": (n_calls, left, right) of the regions of (contig 1, '+', FI) in order

    @property
    def args(self):
        return self.calls, self.offsets, self.merge_gap, self.min_score, self.min_len


def bits_for(n: int) -> int:
    """bits needed to write every value below n (kg_host.hpp)"""
    return (n - 1).bit_length() if n > 1 else 0


def _group(x0, x1, seq, strand, fI, rng):
    """CALLs that cover strand nucleotides x0[i] .. x1[i] of contig `seq` (the frame is x0 % 3, the length a multiple of 3);
    counts 0..8 with ties, weights out of WEIGHTS"""
    x0, x1 = np.asarray(x0, np.int64), np.asarray(x1, np.int64)
    assert ((x1 - x0 + 1) % 3 == 0).all() and (x0 >= 0).all() and (x1 > x0).all()
    f = x0 % 3
    c = np.zeros(x0.size, dtype=CALL_DTYPE)
    c["container"] = 6 * np.asarray(seq, np.int64) + 3 * strand + f
    c["start"], c["end"] = (x0 - f) // 3, (x1 - 2 - f) // 3
    c["count"] = rng.integers(0, 9, size=x0.size)
    c["fI"] = fI
    c["weightedHits"] = WEIGHTS[rng.integers(0, len(WEIGHTS), size=x0.size)]
    return c


def _finish(parts, rng):
    """calls[] order: by container, shuffled inside one"""
    c = np.concatenate(parts)
    c = c[rng.permutation(c.size)]
    return c[np.argsort(c["container"], kind="stable")]


LEAD_LEN = 6          # contig 0 of the filler CALLs


def _lead(lead, rng):
    """`lead` one-codon CALLs on contig 0, '+', every one a group of its own: items 0 .. lead - 1 of the group order"""
    x0 = rng.integers(0, 3, size=lead)
    return _group(x0, x0 + 2, 0, 0, rng.permutation(lead) * 3 - lead, rng)


def _shorts(base, k, rng):
    """x0 of k one-codon CALLs behind `base`, 4 to 8 nt apart: without a longer CALL over them, each opens a region at
    merge_gap 0 (x0' - (x0 + 2) - 1 >= 1)"""
    return base + 6 * np.arange(1, k + 1) + rng.integers(0, 3, size=k)


# ---- a. a nested run across a boundary ------------------------------------------------------------------------------------

def nested(lead, run, follow=False):
    """One group of `run` CALLs at items lead .. lead + run - 1: the first covers 0 .. 6 run + 8, the others lie inside it.
    merge_gap 0: one region of `run` CALLs.  follow: the next group (FI + 1) has three CALLs 0..2, 9..11, 18..20 inside the
    span the run carries: three regions."""
    rng = np.random.default_rng(100_000 * lead + 2 * run + follow)
    top = 6 * run + 8
    x0 = np.concatenate([[0], _shorts(0, run - 1, rng)])
    x1 = np.concatenate([[top], x0[1:] + 2])
    assert x1[1:].max(initial=0) < top
    parts = [_lead(lead, rng), _group(x0, x1, 1, 0, FI, rng)]
    if follow:
        parts.append(_group([0, 9, 18], [2, 11, 20], 1, 0, FI + 1, rng))
    off = np.cumsum([0, LEAD_LEN, top + 13])
    return Case("nested-lead%d-run%d%s" % (lead, run, "-follow" if follow else ""), _finish(parts, rng), off, 0, 0, 0,
                {"regions": lead + 1 + 3 * follow, "group": [(run, 0, top)]})


LEADS = [0, THREAD - 1, THREAD, THREAD + 1, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1]
RUNS = [2, THREAD, THREAD + 1, 2 * THREAD + 1, WAVE + 1, TILE + 1, 2 * TILE + 1]


# ---- b. a split run across a boundary -------------------------------------------------------------------------------------

SPLIT_RUN, SPLIT_FRONT = 40, 7


def split(boundary, where, merge_gap, twin):
    """The layout of `nested` with the group at item boundary - 7; the CALL at item `boundary` (where = "behind") or
    boundary - 1 ("front") starts merge_gap + 2 nt behind the largest x1 in front of it (twin = "split": it opens a region)
    or merge_gap + 1 nt ("merge": it does not) and covers the rest of the group."""
    lead, run = boundary - SPLIT_FRONT, SPLIT_RUN
    p = SPLIT_FRONT if where == "behind" else SPLIT_FRONT - 1
    rng = np.random.default_rng(1000 * boundary + 10 * merge_gap + 2 * (where == "front") + (twin == "merge"))
    top = 6 * run + 8
    xs = top + merge_gap + (2 if twin == "split" else 1)
    x0 = np.concatenate([[0], _shorts(0, p - 1, rng), [xs], _shorts(xs, run - p - 1, rng)])
    x1 = x0 + 2
    x1[0], x1[p] = top, xs + top
    parts = [_lead(lead, rng), _group(x0, x1, 1, 0, FI, rng)]
    off = np.cumsum([0, LEAD_LEN, xs + top + 13])
    group = [(p, 0, top), (run - p, xs, xs + top)] if twin == "split" else [(run, 0, xs + top)]
    return Case("split-at%d-%s-gap%d-%s" % (boundary, where, merge_gap, twin), _finish(parts, rng), off, merge_gap, 0, 0,
                {"regions": lead + len(group), "group": group})


# ---- c. the tile scan's step ----------------------------------------------------------------------------------------------

STEP_RUN = 4001


def step():
    """STEP - 2000 filler CALLs, two a contig (one group, merging on every second contig), then on the next contig a nested run
    of 4001 CALLs that crosses item STEP with its maximum in front, and one CALL 2 nt behind the run: n = STEP + 2002."""
    rng = np.random.default_rng(256)
    n_fill = (STEP - 2000) // 2
    seq = np.repeat(np.arange(n_fill), 2)
    x0 = np.tile([0, 9], n_fill) + rng.integers(0, 3, size=2 * n_fill)
    even = np.arange(n_fill) % 2 == 0
    x0[1::2] = np.where(even, x0[0::2] + 3, x0[1::2])         # (even contigs: the second CALL abuts the first and merges)
    fill = _group(x0, x0 + 2, seq, np.repeat(np.arange(n_fill) % 2, 2), np.repeat(rng.integers(-3, 50, size=n_fill), 2), rng)
    run, top = STEP_RUN, 6 * STEP_RUN + 8
    x0 = np.concatenate([[0], _shorts(0, run - 1, rng), [top + 2]])
    x1 = x0 + 2
    x1[0] = top
    calls = _finish([fill, _group(x0, x1, n_fill, 0, FI, rng)], rng)
    assert calls.size == STEP + 2002
    off = np.concatenate([np.arange(n_fill + 1) * 18, [n_fill * 18 + top + 13]])
    return Case("step", calls, off, 0, 0, 0, {"contig": n_fill, "lead": 2 * n_fill, "group": [(run, 0, top), (1, top + 2, top + 4)]})


# ---- d. walk edges --------------------------------------------------------------------------------------------------------

WALK_BASE = (WALK - 1, WALK, WALK + 1, 2 * WALK, 2 * WALK + 1)


def walk(lead, tail):
    """One group of consecutive regions of 15, 16, 17, 32, 33 CALLs and then `tail`, at the end of the list: the last region
    ends at n.  tail (1,): a one-CALL region at n - 1; (): the region of 33 ends at n; (16,): its head j has j + 16 = n;
    (15,): j + 16 = n + 1; (17,): one item in the walk's second load.  Inside a region every second CALL has 9 nt and starts
    merge_gap + 1 nt behind the largest x1 so far, the one behind it has 3 nt inside it; a region starts merge_gap + 2 behind."""
    merge_gap = 600 if lead in (0, WALK) else 0
    rng = np.random.default_rng(100 * lead + sum(tail) + len(tail))
    lens = WALK_BASE + tuple(tail)
    x0, x1, group, top = [], [], [], -1
    for m in lens:
        left = top + merge_gap + 2 if x0 else 0
        for k in range(m):
            if k % 2 == 0:
                a = left if k == 0 else top + merge_gap + 1
                x0.append(a)
                x1.append(a + 8)
                top = a + 8
            else:
                x0.append(x0[-1] + 1)
                x1.append(x0[-1] + 2)
        group.append((m, left, top))
    parts = [_lead(lead, rng), _group(x0, x1, 1, 0, FI, rng)]
    off = np.cumsum([0, LEAD_LEN, top + 1])
    return Case("walk-lead%d-tail%s" % (lead, "_".join(map(str, tail)) or "none"), _finish(parts, rng), off, merge_gap, 0, 0,
                {"regions": lead + len(lens), "group": group})


# ---- e. list sizes --------------------------------------------------------------------------------------------------------

def sizes(n, flavour):
    """n CALLs over three contigs of 3 nt, both strands: every x0 is 0 and left_bits 2.  flavour "one": one function, so a
    region per contig and strand whose float32 sum is in calls[] order by the sorts' stability alone; "distinct": n functions."""
    rng = np.random.default_rng(2 * n + (flavour == "one"))
    k = np.arange(n) * 6 // n                                  # (contig, strand) of CALL i, non-decreasing
    c = _group(np.zeros(n, np.int64), np.full(n, 2), k // 2, k % 2, FI, rng)
    if flavour == "distinct":
        c["fI"] = rng.permutation(n) * 3 - n
    off = np.array([0, 3, 6, 9], np.int64)
    return Case("sizes-n%d-%s" % (n, flavour), c, off, 600, 0, 0,
                {"regions": len(np.unique(c["container"])) if flavour == "one" else n})


SIZES_N = [1, 2, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1]


# ---- f. the longest contig ------------------------------------------------------------------------------------------------

# 2^k - 1, 2^k, 2^k + 1: left_bits passes k, so `left` and `right` need another bit (right = L - 1 = 2^k); 2^k + 8: an x0 needs
# it as well (x0 <= L - 3).  k = 28 is the one width of four passes at which a sort by one bit less is not rounded back up.
LMAX = ([3, 4, 5] + [2 ** k + d for k in (7, 8, 15, 16, 23, 24) for d in (-1, 0, 1, 8)] + [2 ** 28 + 8] +
        [2 ** 30, 2 ** 30 + 1, INT_MAX])
LMAX_FI = [-2 ** 31, -1, 0, INT_MAX]


def lmax_positions(L):
    """x0 of the one-codon CALLs on the long contig: both ends, and 3 nt to either side of the highest bit of left_bits (a
    sort by fewer bits swaps those two), as far as they fit"""
    half = 1 << (bits_for(L) - 1)
    return sorted({0, L - 3} | {x for x in (half - 3, half + 3) if 0 < x < L - 3})


def lmax(L, merge_gap, min_len):
    """Contigs of 3, L and 3 nt.  On the long one, on both strands and for four functions, CALLs at x0 = 0 and ending at
    x1 = L - 1 ('-': left 0 and right L - 1) and next to the key's highest bit; merge_gap 2^31 - 1 makes each group one region
    over the whole contig, kept when L >= min_len."""
    rng = np.random.default_rng(L % 1_000_003 + merge_gap % 1000 + min_len % 7)
    pos = np.array(lmax_positions(L), np.int64)
    parts = [_group([0], [2], s, strand, 0, rng) for s in (0, 2) for strand in (0, 1)]
    parts += [_group(pos, pos + 2, 1, strand, f, rng) for strand in (0, 1) for f in LMAX_FI]
    off = np.cumsum([0, 3, L, 3])
    expect = {"whole": (len(pos), 0, L - 1, int(L >= min_len))} if merge_gap == INT_MAX else {}
    return Case("lmax-L%d-gap%d-minlen%d" % (L, merge_gap, min_len), _finish(parts, rng), off, merge_gap, 0, min_len, expect)


def lmax_values():
    return [(L, gap, ml) for L in LMAX for gap in (0, 600, INT_MAX) for ml in (0, L, INT_MAX)]


# ---- g. the number of contigs ---------------------------------------------------------------------------------------------

NSEQS = [1, 2, 3, 4, 5, 127, 128, 129, 32767, 32768, 32769]
NSEQS_LEN = [200, 300]         # left_bits 8: left_bits + bits_for(n_seqs) = 8 | 9 at n_seqs 1 | 2; left_bits 9: 16 | 17 at
                               # 128 | 129 and 24 | 25 at 32768 | 32769, where 32 + bits_for(2 n_seqs) passes 40 and 48 too


def nseqs(n_seqs, L):
    """n_seqs contigs of L nt; CALLs of two functions on the first and the last, on both strands, at both ends and in the
    middle; merge_gap 50"""
    rng = np.random.default_rng(1000 * n_seqs + L)
    pos = np.array([0, 3 * (L // 6) + 1, L - 3], np.int64)
    parts = [_group(pos, pos + 2 + 3 * (pos == 0), s, strand, f, rng)
             for s in sorted({0, n_seqs - 1}) for strand in (0, 1) for f in (-1, 3)]
    off = np.arange(n_seqs + 1, dtype=np.int64) * L
    return Case("nseqs-%d-len%d" % (n_seqs, L), _finish(parts, rng), off, 50, 0, 0, {"regions": 3 * len(parts)})


# ---- the values the tests run ----------------------------------------------------------------------------------------------

FAMILIES = {"nested": nested, "split": split, "step": step, "walk": walk, "sizes": sizes, "lmax": lmax, "nseqs": nseqs}
CASES = {
    "nested": [(lead, run, follow) for lead in LEADS for run in RUNS for follow in (False, True)],
    "split": [(b, where, gap, twin) for b in (THREAD, WAVE, TILE) for where in ("behind", "front") for gap in (0, 1, 600)
              for twin in ("split", "merge")],
    "step": [()],
    "walk": [(lead, tail) for lead in (0, 1, WALK - 1, WALK) for tail in ((1,), (), (WALK,), (WALK - 1,), (WALK + 1,))],
    "sizes": [(n, flavour) for n in SIZES_N for flavour in ("one", "distinct")],
    "lmax": lmax_values(),
    "nseqs": [(n, L) for n in NSEQS for L in NSEQS_LEN],
}


def make(family, values) -> Case:
    return FAMILIES[family](*values)


def case_id(values) -> str:
    """a test id that names the edge"""
    return "-".join(("_".join(map(str, v)) or "none") if isinstance(v, tuple) else str(v) for v in values) or "all"


def counted(calls, regs):
    """the statistics of a call, counted from its CALLs and the reference's records"""
    keys = np.stack([calls["container"].astype(np.int64) // 3, calls["fI"].astype(np.int64)], axis=1)
    groups = len(np.unique(keys, axis=0))
    return {"calls": len(calls), "groups": groups, "regions": len(regs), "kept": int(regs["kept"].sum()),
            "multi_frame": int(((regs["frames"] & (regs["frames"] - 1)) != 0).sum())}


def check_expect(case: Case, regs, start):
    """the answers a case states, against records in output order"""
    e = case.expect
    if "regions" in e:
        assert len(regs) == e["regions"], (case.name, len(regs), e["regions"])
    if "group" in e:
        s = e.get("contig", 1)
        g = regs[start[s]:start[s + 1]]
        g = g[(g["strand"] == 0) & (g["fI"] == FI)]
        assert [(int(r["n_calls"]), int(r["left"]), int(r["right"])) for r in g] == e["group"], case.name
    if "whole" in e:
        g = regs[start[1]:start[2]]
        assert len(g) == 2 * len(LMAX_FI), case.name
        assert {(int(r["n_calls"]), int(r["left"]), int(r["right"]), int(r["kept"])) for r in g} == {e["whole"]}, case.name
