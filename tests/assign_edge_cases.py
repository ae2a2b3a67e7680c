"""Inputs that put kg_assign_calls / kg_result_assign (kg_assign.hpp, kg_host_assign.hpp) on their internal borders, and what
they must give: tests/test_assign_edges_host.py checks both forms of tests/assign_model.py against these answers on the CPU,
tests/test_gpu_assign_edges.py checks the device against the model and the answers.

The borders: a protein of at most SHORT = 16 CALLs is grouped by one lane, a longer one is sorted by (rank << 32 | fI ^ 2^31) and
each run of equal keys is walked by the lane at its head, WALK = 16 items at a time; a wave then merges the top two runs of its
protein, run k of the protein in lane k % WAVE; the sort takes (32 + bits_for(n_long) + 7) / 8 passes over tiles of TILE = 4096
items, the prefix sums that number the long proteins work on chunks of SCAN = 2048, and the two one-wave-per-protein kernels run
on min((n_long + 3) / 4, GRID) workgroups.  Every case is (calls, call_start, otu, (min_score, min_share_pct), answer); `answer`
is the whole ASSIGNMENT_DTYPE array, written down from the construction in plain arithmetic.  Only the padded random lists of
(a) and the shifted lists of (i) take their answer from assign_model.brute_force, on the lists before they were padded or
shifted.  Nothing here calls assign_model.assign."""
from __future__ import annotations

import os
import re

import numpy as np

import assign_model as A
import signature_model as SM
from kmergutsjava_amd._native import ASSIGNMENT_DTYPE, CALL_DTYPE, OTU_DTYPE

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kmergutsjava_amd", "csrc")


def _text(name):
    return open(os.path.join(_CSRC, name)).read()


def _const(text, name):
    """A constant of the headers: `N`, `A * B` or `A << B`, with or without a u / ull suffix; anything else is an error."""
    expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, text).group(1)
    m = re.fullmatch(r"(\d+)(?:ull|u)?(?: (\*|<<) (\d+)(?:ull|u)?)?", expr.strip())
    assert m, (name, expr)
    a, op, b = int(m.group(1)), m.group(2), m.group(3)
    return a if op is None else a * int(b) if op == "*" else a << int(b)


ASSIGN_TEXT, _DEVICE, _BUILD, HOST_TEXT = _text("kg_assign.hpp"), _text("kg_device.hpp"), _text("kg_build.hpp"), _text("kg_host_assign.hpp")
SHORT = _const(ASSIGN_TEXT, "kAssignShort")                                         # CALLs one lane groups on its own
WALK = _const(ASSIGN_TEXT, "kAssignWalk")                                           # items a run walk loads ahead
WAVE = _const(_DEVICE, "kWave")
SCAN = _const(_DEVICE, "kScanThreads") * _const(_DEVICE, "kScanPerThread")      # kScanChunk
TILE = _const(_BUILD, "kBuildThreads") * _const(_BUILD, "kBuildItems")          # kBuildTile
# the grid of the two kernels that give a long protein a wave: four waves to a workgroup, at most GRID workgroups
_GRID = re.search(r"const uint32_t wgrid = \(uint32_t\)std::min<uint64_t>\(\(n_long \+ 3\) / 4, (\d+)ull \* (\d+)\);", HOST_TEXT)
assert _GRID, "the grid expression of kg_host_assign.hpp is not the one these cases were built around"
GRID = int(_GRID.group(1)) * int(_GRID.group(2))
WAVES_PER_WG = 4

BIG = float(2 ** 24)            # BIG + 1.0 == BIG in float32: a sum that took the ones first, or in blocks, is larger
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
DEFAULT = (0, 50)


def key_bits(n_long: int) -> int:
    """32 + bits_for(n_long), the width of the sort key"""
    return 32 + (0 if n_long <= 1 else (n_long - 1).bit_length())


def passes(n_long: int) -> int:
    return (key_bits(n_long) + 7) // 8


# ---- records ------------------------------------------------------------------------------------------------------------------

def calls_of(rows) -> np.ndarray:
    """[(fI, count, weightedHits)] -> CALL_DTYPE"""
    c = np.zeros(len(rows), dtype=CALL_DTYPE)
    if len(rows):
        f, k, w = zip(*rows)
        c["fI"], c["count"], c["weightedHits"] = f, k, w
    return c


def pack(lists):
    """one CALL array per protein -> (calls, call_start)"""
    cs = np.zeros(len(lists) + 1, dtype=np.int64)
    cs[1:] = np.cumsum([len(x) for x in lists])
    calls = np.concatenate(lists) if lists else np.zeros(0, dtype=CALL_DTYPE)
    calls["container"] = np.repeat(np.arange(len(lists), dtype=np.uint32), np.diff(cs))
    return calls, cs


def record(n_calls, nf=0, total=0, best=None, second=None, params=DEFAULT, otu=-1):
    """One kg_assignment from what the construction fixes: best = (f, S, W), second = (f, S) or None."""
    rec = np.zeros(1, dtype=ASSIGNMENT_DTYPE)[0]
    rec["fI"], rec["second_fi"], rec["otu"], rec["n_calls"], rec["n_functions"], rec["total"] = -1, -1, otu, n_calls, nf, total
    if n_calls:
        f, s, w = best
        rec["fI"], rec["score"], rec["weighted"] = f, s, np.float32(w)
        rec["assigned"] = int(s >= params[0] and 100 * s >= params[1] * total)
        assert nf >= 1 and (second is None) == (nf == 1)
        if second is not None:
            rec["second_fi"], rec["second_score"] = second
    return rec


def _case(prots, params=DEFAULT, otu=None):
    """[(CALL array, record)] -> a case"""
    calls, cs = pack([c for c, _ in prots])
    answer = np.array([r for _, r in prots], dtype=ASSIGNMENT_DTYPE)
    return calls, cs, otu, params, answer


def filler(n: int, f: int = 1, params=DEFAULT):
    """n CALLs of one function, count 1, weight 0.5 (n of them add up exactly)"""
    return calls_of([(f, 1, 0.5)] * n), record(n, 1 if n else 0, n, (f, n, 0.5 * n), None, params)


def long17_rows(r: int):
    """The 17 CALLs of long protein r of (e) and (f): nine of r % 7 (BIG, then ones) and eight of 7 + r % 3, interleaved."""
    return [(r % 7, 2, BIG if k == 0 else 1.0) if k % 2 == 0 else (7 + r % 3, 2, 1.0) for k in range(SHORT + 1)]


def long17(r: int, params=DEFAULT):
    return calls_of(long17_rows(r)), record(17, 2, 34, (r % 7, 18, BIG), (7 + r % 3, 16), params)


# ---- a. path independence at the split ------------------------------------------------------------------------------------------

SPLIT_LISTS = 200
SPLIT_TOTALS = (16, 17, 18, 64, 65)


def split_lists():
    """200 lists of 1 to 16 CALLs with many ties -> ([CALL array], otu records)"""
    rng = np.random.default_rng(1601)
    lists, otus = [], []
    for n_fn in (3, 8):
        calls, cs, otu = A.random_lists(rng, 150, max_calls=SHORT, n_fn=n_fn)
        keep = [p for p in range(150) if cs[p + 1] > cs[p]][:SPLIT_LISTS // 2]
        assert len(keep) == SPLIT_LISTS // 2
        lists += [calls[cs[p]:cs[p + 1]].copy() for p in keep]
        otus += [otu[p] for p in keep]
    return lists, np.array(otus, dtype=OTU_DTYPE)


def split_case():
    """Every list as it is, and padded with zero CALLs (the first CALL's fI, count 0, weight +0.0) to each of SPLIT_TOTALS, once
    behind and once in front: the record is the list's own but for n_calls, whichever path the length puts it on.
    -> (case, the index of the unpadded list of every protein)"""
    lists, otu = split_lists()
    cs = np.zeros(len(lists) + 1, dtype=np.int64)
    cs[1:] = np.cumsum([len(x) for x in lists])
    own = A.brute_force(np.concatenate(lists), cs, otu, *DEFAULT)
    prots, source = [], []
    for k, lst in enumerate(lists):
        prots.append((lst, own[k]))
        source.append(k)
        for total in SPLIT_TOTALS:
            if total <= len(lst):
                continue                                        # (16 only when the list is shorter than 16)
            zero = calls_of([(int(lst["fI"][0]), 0, 0.0)] * (total - len(lst)))
            rec = own[k].copy()
            rec["n_calls"] = total
            prots += [(np.concatenate([lst, zero]), rec), (np.concatenate([zero, lst]), rec)]
            source += [k, k]
    calls, cs2, _, params, answer = _case(prots)
    return (calls, cs2, otu[source], params, answer), np.array(source)


# ---- b. rank grid for the merge ---------------------------------------------------------------------------------------------------

GRID_LONG = dict(n=130, ranks=(0, 1, 31, 32, 63, 64, 65, 127, 128, 129), above=40)
GRID_SHORT = dict(n=16, ranks=(0, 1, 7, 8, 14, 15), above=5)
GRID_MODES = (1, 2, 3, 4, 5)


def grid_functions(n: int) -> np.ndarray:
    """n distinct int32 function indices in ascending order, with INT32_MIN, -1, 0 and INT32_MAX among them"""
    rng = np.random.default_rng(n)
    f = {I32_MIN, -1, 0, I32_MAX}
    while len(f) < n:
        f.add(int(rng.integers(I32_MIN, I32_MAX)))
    return np.array(sorted(f), dtype=np.int64)


def grid_plan(mode: int):
    """The proteins of one mode in their order: (grid, i, j), the long grid first."""
    if mode == 4:
        return [(GRID_LONG, None, None), (GRID_SHORT, None, None)]
    return [(g, i, j) for g in (GRID_LONG, GRID_SHORT) for i in g["ranks"] for j in g["ranks"] if i != j]


def grid_protein(mode: int, g, i, j, rng):
    """One CALL per function, the function of sorted rank k with count[k] and weight[k], emitted in shuffled order."""
    n, F = g["n"], grid_functions(g["n"])
    count, weight = np.ones(n, dtype=np.int64), np.ones(n, dtype=np.float32)
    lo = None if i is None else min(i, j)
    if mode == 1:                                   # S decides
        count[i], count[j] = 3, 2
        best, second = (F[i], 3, 1.0), (F[j], 2)
    elif mode == 2:                                 # W decides between i and j; the larger W of a smaller S must not win
        count[i] = count[j] = 2
        weight[:] = 4.0
        weight[i], weight[j] = 2.0, 1.5
        best, second = (F[i], 2, 2.0), (F[j], 2)
    elif mode == 3:                                 # f decides
        count[i] = count[j] = 2
        best, second = (F[lo], 2, 1.0), (F[i + j - lo], 2)
    elif mode == 4:                                 # f decides among all
        best, second = (F[0], 1, 1.0), (F[1], 1)
    else:                                           # f decides the runner-up below a unique best
        count[i] = count[j] = 2
        count[g["above"]] = 3
        best, second = (F[g["above"]], 3, 1.0), (F[lo], 2)
    order = rng.permutation(n)
    c = calls_of(list(zip(F[order].tolist(), count[order].tolist(), weight[order].tolist())))
    return c, record(n, n, int(count.sum()), best, second)


def grid_case(mode: int):
    rng = np.random.default_rng(7000 + mode)
    return _case([grid_protein(mode, g, i, j, rng) for g, i, j in grid_plan(mode)])


# ---- c. the walk ------------------------------------------------------------------------------------------------------------------

WALK_L = (1, 2, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49, 255, 256, 257)
WALK_ORDERS = ("big first", "big last")
RUN_F = 1000                    # the function of the run under test
NEIGHBOURS = ((17, 17), (32, 17), (33, 48), (48, 33))


def walk_weights(L: int, order: str):
    """The run's weights in emission order and their float32 sum taken in that order."""
    if order == "big first":
        return [BIG] + [1.0] * (L - 1), np.float32(BIG)                         # every 1.0 is lost: BIG + 1 rounds back to BIG
    w = np.float32(L - 1) + np.float32(BIG)                                     # L - 1 ones add up exactly, then one rounded add
    if (L - 1) % 2 == 0:
        assert float(w) == BIG + L - 1
    return [1.0] * (L - 1) + [BIG], w


def behind(L: int) -> int:
    """how many items stand behind the run in the `behind` arrangement: 1 .. 15, both ends taken"""
    return {1: 1, 16: WALK - 1, 257: 1, 256: WALK - 1}.get(L, 1 + (7 * L) % (WALK - 1))


def walk_protein(L: int, order: str, arrangement: str):
    """A run of L CALLs of RUN_F, count 1, among one-CALL functions of count 1 and weight 1.0 (17 of them when L <= 16, so that
    the protein is long).  contiguous: the run, then the others, which sort to both sides of it.  even: the run on the even
    emission positions, L - 1 other functions on the odd ones.  last: every other function is smaller, so the run is the last
    of its protein.  behind: as last, with behind(L) larger functions."""
    weights, W = walk_weights(L, order)
    run = [(RUN_F, 1, w) for w in weights]
    below = [(RUN_F - 1 - 3 * k, 1, 1.0) for k in range(SHORT + 1)]
    if arrangement == "contiguous":
        others = (below[:8] + [(RUN_F + 2 + 5 * k, 1, 1.0) for k in range(9)]) if L <= SHORT else []
        rows = run + others[::-1]
    elif arrangement == "even":
        between = [(RUN_F + (k + 1) * (11 if k % 2 else -11), 1, 1.0) for k in range(L - 1)]
        others = between + ([(RUN_F - 6 - 22 * k, 1, 1.0) for k in range(SHORT + 1)] if L <= SHORT else [])
        rows = [x for pair in zip(run, between) for x in pair] + [run[-1]] + others[L - 1:]
    else:
        others = below if L <= SHORT else below[:3]
        if arrangement == "behind":
            others = others + [(RUN_F + 1 + k, 1, 1.0) for k in range(behind(L))]
        else:
            assert arrangement == "last"
        rows = others + run
    assert len(rows) == L + len(others) > SHORT and len({f for f, _, _ in others}) == len(others)
    second = (min(f for f, _, _ in others), 1) if others else None
    return calls_of(rows), record(len(rows), 1 + len(others), len(rows), (RUN_F, L, W), second)


def walk_inner_case():
    """Every run contiguous and on the even positions, both weight orders, in one call."""
    return _case([walk_protein(L, order, arr) for arr in ("contiguous", "even") for order in WALK_ORDERS for L in WALK_L])


def walk_end_case(L: int, order: str, arrangement: str):
    """The protein under test as the last long protein of its call (short and empty ones follow): with `last` its run ends on
    the sorted array's last item, with `behind` 1 to 15 items before it."""
    return _case([filler(3), long17(0), filler(0), walk_protein(L, order, arrangement), filler(2, -4), filler(0)])


def neighbours_case(lengths):
    """Adjacent long proteins that consist of function 7 only, count 1, weight 1.0: only the key's rank half separates their
    runs.  An empty protein stands between them, so that rank is not index."""
    prots = []
    for n in lengths:
        prots += [(calls_of([(7, 1, 1.0)] * n), record(n, 1, n, (7, n, float(n)), None)), filler(0)]
    return _case(prots[:-1])


# ---- d. the sort's tiles ------------------------------------------------------------------------------------------------------------

def tiles_case():
    """One protein of 2 * TILE + 1000 CALLs: function 3 on both sides of each tile border and at both ends, BIG first; every
    other CALL a function of its own, on both sides of 3."""
    n = 2 * TILE + 1000
    at = [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n - 1]
    others = np.concatenate([np.arange(-4000, 3), np.arange(4, 4 + n - 6 - 4003)])
    assert others.size == n - 6 and 3 not in others
    f = np.zeros(n, dtype=np.int64)
    own = np.ones(n, dtype=bool)
    own[at] = False
    f[at], f[own] = 3, np.random.default_rng(4096).permutation(others)
    c = np.zeros(n, dtype=CALL_DTYPE)
    c["fI"], c["count"], c["weightedHits"] = f, 1, 1.0
    c["weightedHits"][0] = BIG
    return _case([(c, record(n, n - 5, n, (3, 6, BIG), (-4000, 1)))])


# ---- e, f. many long proteins: key widths, buffer parity, the second grid trip, the prefix sum's chunk --------------------------------

KEY_WIDTH_N_LONG = (1, 2, 3, 256, 257, 65536, 65537)
KEY_WIDTHS = {1: (32, 4), 2: (33, 5), 3: (34, 5), 256: (40, 5), 257: (41, 6), 65536: (48, 6), 65537: (49, 7)}  # n_long: (bits, passes)


def mixed_case(n_prot: int, long_at, params=DEFAULT):
    """Long protein r (in index order) is long17(r); every other protein p has p % 4 CALLs of one function (2 or -3), count 1,
    weight 0.5; otu n = p % 3, oI[0] = p % 11.  Built and answered with array arithmetic, as the largest has 10^6 CALLs."""
    p = np.arange(n_prot, dtype=np.int64)
    is_long = np.zeros(n_prot, dtype=bool)
    is_long[np.asarray(long_at, dtype=np.int64)] = True
    r = np.cumsum(is_long) - 1
    cnt = np.where(is_long, SHORT + 1, p % 4)
    cs = np.zeros(n_prot + 1, dtype=np.int64)
    cs[1:] = np.cumsum(cnt)
    prot = np.repeat(p, cnt)
    pos = np.arange(int(cs[-1]), dtype=np.int64) - cs[prot]
    lg, rr, even = is_long[prot], r[prot], pos % 2 == 0
    ffill = np.where(p % 2 == 1, -3, 2)
    calls = np.zeros(int(cs[-1]), dtype=CALL_DTYPE)
    calls["container"] = prot
    calls["fI"] = np.where(lg, np.where(even, rr % 7, 7 + rr % 3), ffill[prot])
    calls["count"] = np.where(lg, 2, 1)
    calls["weightedHits"] = np.where(lg, np.where(pos == 0, BIG, 1.0), 0.5).astype(np.float32)
    otu = np.zeros(n_prot, dtype=OTU_DTYPE)
    otu["n"], otu["oI"][:, 0], otu["count"][:, 0] = p % 3, p % 11, 1
    ans = np.zeros(n_prot, dtype=ASSIGNMENT_DTYPE)
    some = cnt > 0
    ans["fI"] = np.where(is_long, r % 7, np.where(some, ffill, -1))
    ans["score"] = np.where(is_long, 18, cnt)
    ans["total"] = np.where(is_long, 34, cnt)
    ans["weighted"] = np.where(is_long, BIG, 0.5 * cnt).astype(np.float32)
    ans["assigned"] = some & (ans["score"] >= params[0]) & (100 * ans["score"].astype(np.int64) >= params[1] * ans["total"].astype(np.int64))
    ans["n_calls"] = cnt
    ans["n_functions"] = np.where(is_long, 2, some.astype(np.int64))
    ans["second_fi"] = np.where(is_long, 7 + r % 3, -1)
    ans["second_score"] = np.where(is_long, 16, 0)
    ans["otu"] = np.where(p % 3 > 0, p % 11, -1)
    return calls, cs, otu, params, ans


def key_width_layout(n_long: int):
    """In front of long protein r stand r % 5 others.  -> (n_prot, the indices of the long proteins)"""
    r = np.arange(n_long, dtype=np.int64)
    at = r + np.cumsum(r % 5)
    return int(at[-1]) + 1, at


def key_width_case(n_long: int):
    return mixed_case(*key_width_layout(n_long))


CHUNK_N_PROT = 3 * SCAN + 3
CHUNK_LONG_AT = (0, SCAN - 1, SCAN, SCAN + 1, 2 * SCAN - 1, 2 * SCAN, CHUNK_N_PROT - 1)
CHUNK_VARIANTS = ("borders", "all long", "one protein")


def chunk_case(variant: str):
    if variant == "borders":
        return mixed_case(CHUNK_N_PROT, CHUNK_LONG_AT)
    if variant == "all long":
        return mixed_case(SCAN + 1, np.arange(SCAN + 1))
    assert variant == "one protein"
    return mixed_case(1, [0])


# ---- g. the 2^31 limit, on both paths -------------------------------------------------------------------------------------------------

TOP = 2 ** 31 - 1
ZERO_PAD = [(10 + k, 0, 0.0) for k in range(SHORT + 1)]         # 17 zero-count CALLs of other functions: the list's long form


def below_limit_case(share: int):
    """T = 2^31 - 1 as one CALL and as 2^30 + (2^30 - 1) of two functions, short and long: accepted, score and total exact.
    100 * S_best and share * T need 64 bits: at share 100 only the first is assigned, at 50 both are (by 50)."""
    params = (0, share)
    one, two = [(4, TOP, 1.0)], [(4, 2 ** 30, 1.0), (6, 2 ** 30 - 1, 1.0)]
    assert 100 * 2 ** 30 - 50 * TOP == 50 and 100 * 2 ** 30 < 100 * TOP and 100 * TOP >= 2 ** 32
    return _case([(calls_of(one), record(1, 1, TOP, (4, TOP, 1.0), None, params)),
                  (calls_of(two), record(2, 2, TOP, (4, 2 ** 30, 1.0), (6, 2 ** 30 - 1), params)),
                  (calls_of(ZERO_PAD + one), record(18, 18, TOP, (4, TOP, 1.0), (10, 0), params)),
                  (calls_of(two[:1] + ZERO_PAD + two[1:]), record(19, 19, TOP, (4, 2 ** 30, 1.0), (6, 2 ** 30 - 1), params))], params)


def limit_error_cases():
    """T = 2^31 with S_best = 2^30: KG_ERR_LIMIT naming the first such protein.  Yields (name, calls, call_start, protein)."""
    bad = [(4, 2 ** 30, 1.0), (6, 2 ** 30, 1.0)]
    short_bad, long_bad = calls_of(bad), calls_of(bad[:1] + ZERO_PAD + bad[1:])
    fine = [filler(2)[0], long17(1)[0], filler(0)[0]]
    for name, prots, at in (("short", [fine[0], short_bad], 1), ("long", [fine[1], fine[0], long_bad, fine[2]], 2),
                            ("long at 3, short at 5", fine + [long_bad, fine[1], short_bad, fine[0]], 3),
                            ("short at 3, long at 5", fine + [short_bad, fine[1], long_bad, fine[0]], 3)):
        calls, cs = pack(prots)
        yield name, calls, cs, at


def totals(calls, cs):
    """T of every protein in Python integers"""
    return [sum(int(k) for k in calls["count"][cs[p]:cs[p + 1]]) for p in range(len(cs) - 1)]


# ---- h. thresholds at their bound ---------------------------------------------------------------------------------------------------

def _both_paths(rows, nf, total, best, second, params, pad_second=None):
    """The list on the short path and, with ZERO_PAD in the middle of it, on the long one."""
    half = len(rows) // 2
    padded = rows[:half] + ZERO_PAD + rows[half:]
    return _case([(calls_of(rows), record(len(rows), nf, total, best, second, params)),
                  (calls_of(padded), record(len(padded), nf + len(ZERO_PAD), total, best, second or pad_second, params))], params)


def threshold_cases():
    """Yields (name, case, assigned)."""
    half = [(5, 1, 0.5), (2, 1, 1.0)]                               # S = 1 of T = 2; W makes 2 the best
    for share, ok in ((50, 1), (51, 0)):
        yield "1 of 2 at %d" % share, _both_paths(half, 2, 2, (2, 1, 1.0), (5, 1), (0, share)), ok
    for s, ok in ((33, 0), (34, 1)):
        rows = [(6, 33, 1.0), (2, s, 2.0), (5, 33, 1.0), (8, 100 - 66 - s, 1.0)]
        yield "%d of 100 at 34" % s, _both_paths(rows, 4, 100, (2, s, 2.0), (5, 33), (0, 34)), ok
    seven = [(3, 4, 1.0), (3, 3, 1.0)]
    for ms, ok in ((7, 1), (8, 0)):
        yield "S = 7 at min_score %d" % ms, _both_paths(seven, 1, 7, (3, 7, 2.0), None, (ms, 50), (10, 0)), ok
    zeros = [(9, 0, 0.0), (4, 0, 0.0), (6, 0, 0.0)]
    for ms, ok in ((0, 1), (1, 0)):
        yield "T = 0 at min_score %d" % ms, _both_paths(zeros, 3, 0, (4, 0, 0.0), (6, 0), (ms, 50)), ok


# ---- i. call_start[0] = 5 ---------------------------------------------------------------------------------------------------------------

def shifted(case):
    """Five records in front of the first protein's, one with a negative count: they belong to no protein."""
    calls, cs, otu, params, answer = case
    front = calls_of([(3, 9, 1.0), (int(calls["fI"][0]), 2 ** 30, BIG), (7, -5, 2.0), (I32_MIN, 1, 1.0), (int(calls["fI"][0]), 1, 0.5)])
    return np.concatenate([front, calls]), cs + 5, otu, params, answer


def shifted_cases():
    """A closed-form case on both paths, and random lists (their answer: brute_force on the unshifted lists)."""
    yield "rank grid", shifted(grid_case(2))
    calls, cs, otu = A.random_lists(np.random.default_rng(55), 60, max_calls=40, n_fn=6)
    yield "random lists", shifted((calls, cs, otu, (5, 34), A.brute_force(calls, cs, otu, 5, 34)))


# ---- j. behind a scan -----------------------------------------------------------------------------------------------------------------

SEGMENTS, SEGMENT = 150, 60


def scan_inputs():
    """A family set to derive the table from, and the proteins to scan: the set itself, then a chimera of 150 segments of 60
    residues that cycles through the first member of every annotated function, an empty protein, and a chimera that alternates
    between two functions.  -> (seq, offsets, fn, otu of the family set), (seq, offsets of the query), the two chimeras' indices"""
    seq, off, fn, otu = SM.family_set(80, 10, 300, 0.04, 91)
    first = [int(np.flatnonzero(fn == f)[0]) for f in sorted(set(fn[fn >= 0].tolist()))]

    def segment(member):                                        # the member's first 60 residues
        assert off[member + 1] - off[member] >= SEGMENT
        return seq[int(off[member]):int(off[member]) + SEGMENT]

    cycle = b"".join(segment(first[k % len(first)]) for k in range(SEGMENTS))
    two = b"".join(segment(first[k % 2]) for k in range(SEGMENTS))
    n = len(fn)
    qoff = np.concatenate([off, off[-1] + np.cumsum([len(cycle), 0, len(two)])]).astype(np.int64)
    return (seq, off, fn, otu), (seq + cycle + two, qoff), (n, n + 2)
