"""The long-protein inputs of tests/test_gpu_band_long.py and tests/test_band_long_host.py: pairs whose stripe windows lie right
of align_band_kernel's carry, whose traced boxes go to trace_run's second launch by their columns or by their direction words,
a launch with more long boxes than workgroups, a pair over the default cell cap, and a search with diagonals of more than 1024
cells.  Every border is read from the headers; trace_run's launch choice and align_band_kernel's stripe windows are restated
here, so that each case can say which path it takes; and a row-wise form of band_model's tables can be told to lose what a carry
addressed by absolute column would lose, which shows what the shorter inputs of tests/test_gpu_band.py cannot see.  No GPU."""
from __future__ import annotations

import functools
import os
import re
from typing import NamedTuple

import numpy as np

from kmergutsjava_amd import _native as N
from kmergutsjava_amd.align_scores import GAP_EXTEND, GAP_OPEN

import align_model as A
import band_model as B
import trace_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "kmergutsjava_amd", "csrc")


def _text(name):
    return open(os.path.join(_CSRC, name)).read()


def _const(text, name, known=None):
    """A constant of the headers: `A << B`, or a sum of products, of numbers (with or without a u / ull suffix) and constants
    already read (`known`); anything else is an error."""
    expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, text).group(1).strip()
    assert re.fullmatch(r"\w+ << \w+|\w+(?: [*+] \w+)*", expr), (name, expr)

    def value(tok):
        m = re.fullmatch(r"(\d+)(?:ull|u)?", tok)
        if m:
            return int(m.group(1))
        assert known is not None and tok in known, (name, tok)
        return known[tok]

    if " << " in expr:
        x, y = expr.split(" << ")
        return value(x) << value(y)
    return sum(int(np.prod([value(tok) for tok in term.split(" * ")], dtype=object)) for term in expr.split(" + "))


WAVE = _const(_text("kg_device.hpp"), "kWave")
LDS_COLS = _const(_text("kg_align.hpp"), "kAlignLdsCols")
BAND_MAX = _const(_text("kg_band.hpp"), "kBandMax")
CARRY_COLS = _const(_text("kg_band.hpp"), "kBandCarryCols", dict(kBandMax=BAND_MAX, kWave=WAVE))
DIAG_CAP = _const(_text("kg_band.hpp"), "kBandDiagCap")
WORD = _const(_text("kg_trace.hpp"), "kTraceCellsPerWord")
GRID, LONG_GRID = _const(_text("kg_host_trace.hpp"), "kTraceGrid"), _const(_text("kg_host_trace.hpp"), "kTraceLongGrid")
SHORT_SLAB, SLAB = _const(_text("kg_host_trace.hpp"), "kTraceShortSlabBytes"), _const(_text("kg_host_trace.hpp"), "kTraceSlabBytes")
MAX_CELLS, MAX_TRACE_CELLS = N.ALIGN_DEFAULT_MAX_CELLS, N.TRACE_DEFAULT_MAX_CELLS
FILL_A = b"KR"


# ---- the rules restated -------------------------------------------------------------------------------------------------------

def trace_stripe_words(mb: int) -> int:
    """kg_trace.hpp: the direction words of one stripe of a box with mb columns."""
    return (mb + WAVE - 1 + WORD - 1) // WORD * WAVE


def trace_launch(na: int, mb: int):
    """trace_run's choice for a traced box of na rows and mb columns: None (the wide launch), "columns" (mb over the LDS carry) or
    "slab" (its direction words over the short slab): the last two go to the second launch, the <true> kernels."""
    if mb > LDS_COLS:
        return "columns"
    return "slab" if (na + WAVE - 1) // WAVE * trace_stripe_words(mb) * 4 > SHORT_SLAB else None


def trace_long_grid(boxes) -> tuple:
    """trace_run's second launch for the traced boxes [(na, mb)] of one call: -> (its boxes, its workgroups)."""
    lng = [(na, mb) for na, mb in boxes if trace_launch(na, mb)]
    if not lng:
        return 0, 0
    words = max((na + WAVE - 1) // WAVE * trace_stripe_words(mb) for na, mb in lng)
    carry_cols = max((mb + 63) // 64 * 64 for _, mb in lng)
    return len(lng), min(len(lng), LONG_GRID, max(1, SLAB // (words * 4 + carry_cols * 8)))


@functools.lru_cache(maxsize=None)
def model(a: bytes, b: bytes, g: int, W: int):
    """band_model.band_trace, kept: -> ((score, end_a, end_b), the path's seven fields or None, the columns)."""
    return B.band_trace(a, b, g, W)


def boxes_of(case) -> list:
    """(na, mb) of every pair of a case that the model traces."""
    ends = [model(case.prots[pa], case.prots[pb], g, case.W)[0] for (pa, pb), g in zip(case.pairs, case.diags)]
    return [(e[1] + 1, e[2] + 1) for e in ends if e[0] > 0]


class Stripe(NamedTuple):
    i0: int
    c_lo: int
    c_hi: int
    c_lo_prev: object       # None for the first walked stripe: nothing is carried into it


def band_stripes(n: int, m: int, g: int, W: int):
    """align_band_kernel's walked stripes of an n x m pair with diagonal g and half-width W, and their column windows."""
    g = min(max(g, -DIAG_CAP), DIAG_CAP)
    r_lo, r_hi = max(0, g - W), min(n - 1, m - 1 + g + W)
    if m <= 0 or r_lo > r_hi:
        return []
    i_start = r_lo & ~(WAVE - 1)
    return [Stripe(i0, max(0, i0 - g - W), min(m - 1, min(i0 + WAVE - 1, n - 1) - g + W), max(0, i0 - WAVE - g - W) if i0 > i_start else None)
            for i0 in range(i_start, r_hi + 1, WAVE)]


def carried_right_of_the_carry(n: int, m: int, g: int, W: int) -> int:
    """The stripes that read a carry whose columns all lie at or beyond kBandCarryCols."""
    return sum(1 for s in band_stripes(n, m, g, W) if s.c_lo_prev is not None and s.c_lo_prev >= CARRY_COLS)


# ---- the cases ----------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    prots: list
    pairs: list
    diags: list
    W: int
    reach: str              # what the case is meant to reach; tests/test_band_long_host.py asserts it


def _filler(rng, n, letters=FILL_A):
    return bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), size=n))


@functools.lru_cache(maxsize=None)
def _a_proteins():
    rng = np.random.default_rng(1150)
    base = A.M.random_protein(rng, 1300)
    return A.mutate(rng, base[1150:1280], 0.1), base


A_WIDTHS = (0, 16, 256)
A_DIAG = -1150


def case_a(W: int) -> Case:
    """130 rows against columns 1150 .. 1279 of 1300: three stripes whose windows start right of the carry; and the pair
    exchanged, whose rows begin at 1150 against 130 columns."""
    a, b = _a_proteins()
    return Case([a, b], [(0, 1)] * 3 + [(1, 0)], [A_DIAG, A_DIAG + 3, A_DIAG - 3, -A_DIAG], W,
                "windows right of the carry; end column >= kAlignLdsCols; exchanged: i_start = 1088, the window clipped at both ends")


# LDS_COLS + 1 is the first box of the second launch.  Its path steps onto column LDS_COLS from column LDS_COLS - 1, so the only
# carried value it reads beyond the LDS carry's size is an H-up that no path takes; at LDS_COLS + 2 the path's own diagonal step
# reads column LDS_COLS of the carry (rows 63 -> 64 of the 65-row a, rows 127 -> 128 of the 129-row one)
B_COLS = (LDS_COLS - 1, LDS_COLS, LDS_COLS + 1, LDS_COLS + 2)
B_ROWS = (1, 64, 65, 129)
B_WIDTH = 8


@functools.lru_cache(maxsize=None)
def case_b(m: int) -> Case:
    """b of m residues, the only tryptophan its last; a of 1, 64, 65 and 129 residues whose last (at most 30) are b's last, on
    the diagonal n - m of the last cell."""
    rng = np.random.default_rng(45)
    b = A.M.random_protein(rng, m - 1).replace(b"W", b"A") + b"W"
    prots, pairs, diags = [b], [], []
    for n in B_ROWS:
        tail = b[-min(n, 30):]
        prots.append(_filler(rng, n - len(tail)) + tail)
        pairs.append((len(prots) - 1, 0))
        diags.append(n - m)
    return Case(prots, pairs, diags, B_WIDTH, "box columns m: at the border of the LDS carry")


C_LENGTHS = (700, 1100)


def case_c_insert(lp: int, mirror: bool):
    """band_model.insert_case with a prefix of lp: -> (a, b, joined score, the prefix's score); the gap lies past column lp."""
    return B.insert_case(6, lp, mirror)


C_INDEL_WIDTHS = (32, 64)


@functools.lru_cache(maxsize=None)
def case_c_indels(W: int) -> Case:
    rng = np.random.default_rng(1100)
    base = A.M.random_protein(rng, 1100)
    return Case([base, B.with_indels(rng, base, every=100, longest=4)], [(0, 1)], [0], W, "a path with several gaps across column kAlignLdsCols")


D_COLS, D_WIDTH = 1000, 16


def d_rows():
    """The largest row count whose direction words fit the short slab at D_COLS columns, and the next stripe's."""
    stripes = SHORT_SLAB // (trace_stripe_words(D_COLS) * 4)
    return stripes * WAVE, (stripes + 1) * WAVE


@functools.lru_cache(maxsize=None)
def case_d() -> Case:
    """b of 1000 residues; a of the two row counts, 10 % mutated windows of b that end where b ends, the last 30 residues exact:
    the end cell is the last row and column, which lies on the diagonal n - m."""
    rng = np.random.default_rng(1000)
    lo, hi = d_rows()
    b = A.M.random_protein(rng, D_COLS)
    prots, pairs, diags = [b], [], []
    for n in (lo, hi):
        body = b[max(D_COLS - n, 0):D_COLS - 30]
        prots.append(A.M.random_protein(rng, n - len(body) - 30) + A.mutate(rng, body, 0.1) + b[D_COLS - 30:])
        assert len(prots[-1]) == n
        pairs.append((len(prots) - 1, 0))
        diags.append(n - D_COLS)
    return Case(prots, pairs, diags, D_WIDTH, "direction words on both sides of kTraceShortSlabBytes with mb <= kAlignLdsCols")


E_LONG, E_SHORT, E_WIDTH = LONG_GRID + 8, 300, 16


@functools.lru_cache(maxsize=None)
def case_e(shift: int = 0) -> Case:
    """kTraceLongGrid + 8 long boxes (case A's pair on three diagonals) with 150 short pairs in front and 150 behind."""
    a, b = _a_proteins()
    short, n_db = B.indel_search(77)
    prots = [a, b] + short
    kinds = [((2 + n_db + q, 2 + q), d) for q in range(5) for d in (0, 2, -3)] + [((2 + q, 2 + n_db + q), 1) for q in range(5)]
    some = [kinds[k % len(kinds)] for k in range(E_SHORT)]
    long_jobs = [((0, 1), A_DIAG + (0, 3, -3)[k % 3] + shift) for k in range(E_LONG)]
    jobs = some[:E_SHORT // 2] + long_jobs + some[E_SHORT // 2:]
    return Case(prots, [p for p, _ in jobs], [d for _, d in jobs], E_WIDTH, "more long boxes than workgroups of the second launch")


F_N = 8193              # the smallest n with n * n over KG_ALIGN_DEFAULT_MAX_CELLS
F_WIDTHS = (0, 32)


@functools.lru_cache(maxsize=None)
def f_protein(n: int = F_N) -> bytes:
    return A.M.random_protein(np.random.default_rng(8193), n)


G_WIDTHS = (8, 64)


@functools.lru_cache(maxsize=None)
def case_g():
    """-> (proteins, n_db): targets of 1100 and 1300 residues and four short ones; queries that are 8 %-substituted copies with
    indels of the two long targets, and two short relatives."""
    rng = np.random.default_rng(1300)
    short, n_short = B.indel_search(78)
    long_t = [A.M.random_protein(rng, 1100), A.M.random_protein(rng, 1300)]
    long_q = [B.with_indels(rng, A.mutate(rng, t, 0.08), every=150, longest=2) for t in long_t]
    return long_t + short[:4] + long_q + short[n_short:n_short + 2], 6


# ---- the model's tables row by row, and what a carry addressed by absolute column would lose ------------------------------------

def tables_rows(ca, cb, g, W, S, gap_open, gap_extend, lost_from=None):
    """band_model.tables_numpy filled row by row, with each cell's four direction bits as kg_trace.hpp keeps them (the source of
    H: 0 none, 1 diagonal, 2 E, 3 F; 4: E opened here; 8: F opened here).  -> (H, E, F, bits).
    lost_from (test code only, a deliberately wrong variant): where a row i with i % 64 == 0 reads row i - 1, the columns at or
    beyond lost_from read as (H, F) = (0, NEG): what a stripe carry of lost_from slots addressed by absolute column would hold.
    Within a row E[j] = max over k < j of H[k] - open - (j - k) ext, and the H of a cell whose best is E adds nothing to that
    maximum (open >= 0), so it is a running maximum over max(0, diagonal, F)."""
    ca, cb = np.asarray(ca, dtype=np.int64), np.asarray(cb, dtype=np.int64)
    n, m = ca.size, cb.size
    S = np.asarray(S, dtype=np.int64)
    assert gap_open >= 0 and gap_extend >= 0
    H = np.zeros((n + 1, m + 1), dtype=np.int64)
    E = np.full((n + 1, m + 1), B.NEG, dtype=np.int64)
    F = np.full((n + 1, m + 1), B.NEG, dtype=np.int64)
    bits = np.zeros((n + 1, m + 1), dtype=np.uint8)
    j = np.arange(1, m + 1)
    for i in range(1, n + 1):
        up_h, up_f = H[i - 1].copy(), F[i - 1].copy()
        if lost_from is not None and i > 1 and (i - 1) % WAVE == 0:
            up_h[lost_from + 1:] = 0
            up_f[lost_from + 1:] = B.NEG
        inside = np.abs((i - j) - g) <= W
        f = np.maximum(up_f[1:], up_h[1:] - gap_open) - gap_extend
        d = up_h[:-1] + S[ca[i - 1], cb]
        base = np.r_[0, np.where(inside, np.maximum(np.maximum(0, d), f), 0)]          # column 0 and the cells without E
        e = np.maximum.accumulate(base + np.arange(m + 1) * gap_extend)[:-1] - gap_open - j * gap_extend
        h = np.where(inside, np.maximum(base[1:], e), 0)
        H[i, 1:], E[i, 1:], F[i, 1:] = h, e, f
        src = np.where(h == 0, 0, np.where(h == d, 1, np.where(h == e, 2, 3)))
        e_open = (H[i, :-1] - gap_open >= E[i, :-1]) * 4
        f_open = (up_h[1:] - gap_open >= up_f[1:]) * 8
        bits[i, 1:] = src | e_open | f_open
    return H, E, F, bits


def walk_bits(bits, ca, cb, S, end_a, end_b):
    """kg_trace.hpp's walk over the direction bits: -> (the record's first seven fields, the column string), as trace_model.walk
    gives them; None where the device would report a walk that left the rule."""
    gi, j, state, cols = end_a, end_b, 0, []
    identical = positive = 0
    start = None
    for _ in range(2 * (end_a + end_b + 2) + 2):
        b4 = int(bits[gi + 1][j + 1])
        if state == 0:
            src = b4 & 3
            if src == 0:
                if not cols or cols[-1] != "M":
                    return None
                start = (gi + 1, j + 1)
                break
            if src == 1:
                cols.append("M")
                identical += int(ca[gi] == cb[j] and ca[gi] < 20)
                positive += int(S[ca[gi]][cb[j]] > 0)
                if gi == 0 or j == 0:
                    start = (gi, j)
                    break
                gi, j = gi - 1, j - 1
            else:
                state = src - 1
        elif state == 1:
            cols.append("E")
            state = 0 if b4 & 4 else 1
            if j == 0:
                return None
            j -= 1
        else:
            cols.append("F")
            state = 0 if b4 & 8 else 2
            if gi == 0:
                return None
            gi -= 1
    if start is None:
        return None
    s = "".join(cols)
    opens = sum(1 for k, c in enumerate(s) if c != "M" and (k == 0 or s[k - 1] != c))
    return (start[0], start[1], identical, positive, opens, s.count("E"), s.count("F")), s


def rows_result(a: bytes, b: bytes, g: int, W: int, lost_align=None, lost_trace=None):
    """What the two passes give with the row-wise tables: -> ((score, end_a, end_b), the path's seven fields and its columns, or
    None).  lost_align: the alignment pass loses its carry from that column on (variant i); lost_trace: the traced box does
    (variant ii).  A box whose end cell does not reproduce the score is the device's KG_ERR_DEVICE: the string "score"."""
    go, ge = min(GAP_OPEN, T.GAP_CAP), min(GAP_EXTEND, T.GAP_CAP)
    ca, cb = T._codes(a), T._codes(b)
    H = tables_rows(ca, cb, g, W, A.S62, go, ge, lost_align)[0]
    end = B._end(H, len(ca), len(cb))
    if end[0] <= 0:
        return end, None
    ca, cb = ca[:end[1] + 1], cb[:end[2] + 1]
    H, _, _, bits = tables_rows(ca, cb, g, W, A.S62, go, ge, lost_trace)
    if int(H[end[1] + 1][end[2] + 1]) != end[0]:
        return end, "score"
    return end, walk_bits(bits, ca, cb, A.S62, end[1], end[2])
