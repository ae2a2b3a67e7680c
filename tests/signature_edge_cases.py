"""Inputs that put kg_signatures_derive (kg_derive.hpp, kg_host_derive.hpp) on its internal borders, and what they must give,
stated here from the construction without the model's code: tests/test_signature_edges_host.py checks tests/signature_model.py
against these answers on the CPU, tests/test_gpu_signature_edges.py checks the device against both.

The borders: derive_collapse_kernel and derive_run_sums_kernel give a lane LANE = 16 consecutive items and a workgroup
WG = 4096; the runs of the three levels (k-mer, fn, OTU) and the signatures are numbered by prefix sums over SCAN = 2048 items;
the window key is k-mer << b | rank with b = ceil(log2 n_prot); the pass plan cuts the k-mer space into bins of BIN0 = 2^23
k-mers, a bin over the cap into pieces of BIN1 = 2^11 and those into single k-mers; a window block is BLOCK = 64 windows of one
protein.  Almost every batch is made of tokens (cluster_model.token_batch): token j of a protein is its one valid window at
position 9 j, so the window list, the pair list and every run are known item by item.

A case is a Case tuple: the batch, the call's parameters, the records it must give (`want`) and the call's counts."""
from __future__ import annotations

import collections

import numpy as np

import cluster_edge_cases as CE
import cluster_model as M
from kmergutsjava_amd import _native as N

LANE = 16                       # kDeriveChunk
WG = 4096                       # 256 lanes of kDeriveChunk items: a workgroup of the two segmented kernels
SCAN = 2048                     # kScanChunk = kScanThreads * kScanPerThread
BLOCK = 64                      # kAaWinPerBlock
BINS = 4096                     # kDeriveBins
BIN0 = 2 ** 23                  # k-mers in a top-level bin: Deriver::shift_for(20^8) = 23
BIN1 = 2 ** 11                  # k-mers in a piece of a refined top-level bin: Deriver::shift_for(2^23) = 11
TOP = 20 ** 8 - 1               # the largest token
MAXI = 2 ** 31 - 1              # the largest fn and otu

T_LEAD, T_RUN = 7, 20 ** 8 // 3             # the lead run's token and the token under test; the tail's is TOP
COUNTS = ("proteins", "windows", "valid_windows", "pairs", "kmers", "signatures")

# passes: None = one pass, an int = exactly that many (forced by the cap), ("min", k) = at least k
Case = collections.namedtuple("Case", "name seq off fn otu want counts minp pur cap passes tok marks")


def sig(kmer, otu, avg, fn, c, n):
    """Records of signatures with c proteins of f* among n: functionWt is the float32 quotient.  Scalars or arrays."""
    kmer = np.atleast_1d(np.asarray(kmer, dtype=np.int64))
    out = np.zeros(kmer.size, dtype=N.SIGNATURE_DTYPE)
    out["kmer"], out["otuIndex"], out["avgFromEnd"], out["functionIndex"] = kmer, otu, avg, fn
    out["functionWt"] = np.asarray(c, dtype=np.float32) / np.asarray(n, dtype=np.float32)
    return out


def _case(name, batch, fn, otu, rows, valid, pairs, kmers, minp=1, pur=1, cap=0, passes=None, tok=None, marks=None):
    seq, off = batch
    want = np.concatenate(rows) if rows else np.zeros(0, dtype=N.SIGNATURE_DTYPE)
    assert (np.diff(want["kmer"]) > 0).all()                    # the answer is stated in k-mer order
    windows = int(np.maximum(np.diff(off) - 8, 0).sum())        # the positions [0, len - 8) of every protein
    counts = dict(proteins=len(fn), windows=windows, valid_windows=valid, pairs=pairs, kmers=kmers, signatures=len(want))
    return Case(name, seq, off, np.asarray(fn, dtype=np.int32), np.asarray(otu, dtype=np.int32), want, counts, minp, pur, cap,
                passes, tok, marks or {})


def pair_list(tok, fn, otu):
    """The sorted (k-mer, protein) pairs of a token batch as the device lists them: by k-mer, then by the protein's rank in
    (fn, otu, index) order, otu counting only where fn >= 0.  -> (k-mer of every pair, protein of every pair)"""
    fn, otu = np.asarray(fn, dtype=np.int64), np.asarray(otu, dtype=np.int64)
    order = np.lexsort((np.arange(fn.size), np.where(fn >= 0, otu, 0), fn))
    rank = np.empty(fn.size, dtype=np.int64)
    rank[order] = np.arange(fn.size)
    pairs = sorted({(int(v), int(rank[p])) for p, m in enumerate(tok) for v in m})
    return np.array([v for v, _ in pairs], dtype=np.int64), order[np.array([r for _, r in pairs], dtype=np.int64)]


# ---- a. fn-run sums against lane and workgroup borders (derive_run_sums_kernel, derive_fn_best_kernel) ----------------------

LANE_GRID = CE.LANE_GRID                    # (lead, run): leads (0, 1, 15, 16, 17 | 4095, 4096, 4097), runs (1 .. 33 | 4095 .. 8192)
lane_places = CE.lane_places                # the offsets into the run next to a lane border, thinned for the long runs
REVERSED = ((0, 17), (15, 33), (17, 16), (4095, 17), (16, 4097))       # the (lead, run) run once more in reversed protein order


def run_sum_case(lead: int, run: int, at: int, tail: int = 3, reverse: bool = False):
    """`lead` proteins hold token 7, `run` hold 20^8 // 3, `tail` hold the largest token; all have fn 0 and otu 0, so rank is the
    protein index and the run under test is pair indices lead .. lead + run - 1, one fn run per k-mer.  The member at pair index
    lead + at has pad = run and every other pad is 0: the run's sum is 9 run + run, so avgFromEnd = 10 exactly (8 or 9 or less
    without that member, 11 or more with it twice).  Reversed, the same proteins in the opposite order give the same bytes."""
    n = lead + run + tail
    tok = np.concatenate([np.full(lead, T_LEAD), np.full(run, T_RUN), np.full(tail, TOP)]).astype(np.int64)
    pad = np.zeros(n, dtype=np.int64)
    pad[lead + at] = run
    marks = dict(token=T_RUN, first=lead, length=run, padded=lead + at)
    if reverse:
        tok, pad = tok[::-1].copy(), pad[::-1].copy()
        marks = dict(token=T_RUN, first=lead, length=run, padded=lead + run - 1 - at)
    rows = ([sig(T_LEAD, 0, 9, 0, lead, lead)] if lead else []) + [sig(T_RUN, 0, 10, 0, run, run)] + \
           ([sig(TOP, 0, 9, 0, tail, tail)] if tail else [])
    name = "lead %d run %d tail %d%s: pad on pair %d" % (lead, run, tail, " reversed" if reverse else "", marks["padded"])
    z = np.zeros(n, dtype=np.int32)
    return _case(name, M.token_batch(tok.reshape(-1, 1), pad), z, z, rows, n, n, len(rows), tok=tok.reshape(-1, 1), marks=marks)


def inner_run_case(lead: int, run: int, at: int):
    """One k-mer whose middle fn run is the run under test: `lead` proteins with fn -1 (their otu of 6 does not count), `run` with
    fn 5, one with fn 9; pair indices as in run_sum_case.  f* = 5 at every run (at run = 1 a tie with fn 9: the smaller f),
    c = run, n_v = lead + run + 1.  The member at pair index lead + at has pad = run, the other members of the run pad 0, and the
    two pairs next to the run (the last fn -1 protein, the fn 9 protein) pad = run as well, so a sum that takes either of them in
    gives 11 or more.  With purity_pct = 1 the k-mer is a signature only where 100 run >= n_v."""
    n = lead + run + 1
    fn = np.concatenate([np.full(lead, -1), np.full(run, 5), [9]]).astype(np.int32)
    otu = np.where(fn < 0, 6, 0).astype(np.int32)
    pad = np.zeros(n, dtype=np.int64)
    pad[lead + at] = pad[lead + run] = run
    if lead:
        pad[lead - 1] = run
    tok = np.full((n, 1), T_RUN, dtype=np.int64)
    rows = [sig(T_RUN, 0, 10, 5, run, n)] if 100 * run >= n else []
    marks = dict(fn_run=5, first=lead, length=run, padded=lead + at, signature=bool(rows))
    return _case("inside a k-mer: lead %d run %d: pad on pair %d" % (lead, run, lead + at), M.token_batch(tok, pad), fn, otu, rows,
                 n, n, 1, tok=tok, marks=marks)


def run_sum_cases(lead: int, run: int):
    """Every input of one (lead, run): the padded member at each of lane_places, as a k-mer of its own and inside a k-mer; once
    with nothing behind the run, so that the run ends where the list ends (end == n in its last, partial lane)."""
    for at in lane_places(lead, run):
        yield run_sum_case(lead, run, at)
        yield inner_run_case(lead, run, at)
    yield run_sum_case(lead, run, run - 1, tail=0)
    if (lead, run) in REVERSED:
        for at in lane_places(lead, run)[:4]:
            yield run_sum_case(lead, run, at, reverse=True)


# ---- b. equal keys against lane and workgroup borders (derive_collapse_kernel) ----------------------------------------------

COLLAPSE_R2 = (1, 17)


def collapse_case(lead: int, r: int, r2: int):
    """`lead` proteins hold token 7; protein X holds the token under test r times and protein Y, behind it, r2 times; three
    proteins hold the largest token.  All have fn 0 and otu 0.  The sorted window list is the lead's items, X's run of r equal keys
    from item lead, Y's run of r2 equal keys abutting it from item lead + r, and the tail.  pairs = lead + 2 + 3, the k-mer has
    n_v = c = 2, and a pair keeps its protein's largest len - i, the first occurrence's: 9 r and 9 r2.

    The order in which a protein's windows are emitted is not fixed, so the order inside an equal-key run is not either: a case
    fixes where a run lies among the lanes, but not where its largest value lies."""
    tok = [[T_LEAD]] * lead + [[T_RUN] * r, [T_RUN] * r2] + [[TOP]] * 3
    rows = ([sig(T_LEAD, 0, 9, 0, lead, lead)] if lead else []) + [sig(T_RUN, 0, (9 * r + 9 * r2) // 2, 0, 2, 2), sig(TOP, 0, 9, 0, 3, 3)]
    z = np.zeros(lead + 5, dtype=np.int32)
    marks = dict(token=T_RUN, first=lead, length=2, windows=(lead, r, r2))
    return _case("lead %d: runs of %d and %d equal keys from item %d" % (lead, r, r2, lead), M.token_batch(tok), z, z, rows,
                 lead + r + r2 + 3, lead + 5, len(rows), tok=tok, marks=marks)


# ---- c. run numbers across the scan chunks ----------------------------------------------------------------------------------

SCAN_BORDERS = (SCAN, 2 * SCAN)
SCAN_HEADS = [(border, at, which) for border in SCAN_BORDERS for at in (border - 1, border, border + 1) for which in (0, 1, 2)]
TIE_BORDERS = (LANE, SCAN, 2 * SCAN)
TIE_SIZES = (1, 3)


def _lead_protein(lead: int):
    """One protein of `lead` distinct tokens below the token under test, fn 0: pair j is a k-mer, an fn run and an OTU run of its
    own and a signature, so all four numberings equal the pair index.  -> (tokens, their records)"""
    tok = 100 + 3 * np.arange(lead, dtype=np.int64)
    return tok, sig(tok, 0, 9 * lead - 9 * np.arange(lead), 0, 1, 1)


def scan_heads_case(border: int, at: int, which: int):
    """The lead protein, then one k-mer of three fn runs (fn 2, 5, 9; two proteins each, three in run `which`), then a protein of
    the three largest tokens.  lead = at - 2 which, so the head of fn run `which` is pair index `at`; with which = 0 the leads are
    2047, 2048, 2049, 4095, 4096, 4097.  f* is run `which` (c = 3, n_v = 7); its OTUs are 1, 4, 4, so the mode is its second OTU
    run; member j of the k-mer has pad j + 1, so each run has a sum of its own.  lead + 1 + 3 records: the compaction crosses the
    same item."""
    sizes = [2, 2, 2]
    sizes[which] = 3
    lead = at - 2 * which
    lead_tok, lead_rows = _lead_protein(lead)
    fn_k = np.repeat([2, 5, 9], sizes)
    first = 2 * which                                           # the f* run's first member
    otu_k = np.zeros(7, dtype=np.int64)
    otu_k[first:first + 3] = (1, 4, 4)
    pad = np.concatenate([[0], 1 + np.arange(7), [0]])
    avg = (3 * 9 + int(pad[1 + first:1 + first + 3].sum())) // 3
    tok = [lead_tok] + [[T_RUN]] * 7 + [[TOP - 2, TOP - 1, TOP]]
    rows = [lead_rows, sig(T_RUN, 4, avg, (2, 5, 9)[which], 3, 7), sig([TOP - 2, TOP - 1, TOP], 0, [27, 18, 9], 0, 1, 1)]
    fn = np.concatenate([[0], fn_k, [0]])
    otu = np.concatenate([[0], otu_k, [0]])
    marks = dict(token=T_RUN, first=lead, length=7, head=at)
    return _case("the head of fn run %d on item %d (border %d)" % (which, at, border), M.token_batch(tok, pad), fn, otu, rows,
                 lead + 10, lead + 10, lead + 4, tok=tok, marks=marks)


def fn_tie_case(border: int, s: int):
    """The lead protein with border - s tokens, then one k-mer of two fn runs of s proteins each, fn 3 on items border - s ..
    border - 1 and fn 8 on items border .. border + s - 1.  The counts tie: f* = 3, the smaller.  The first run's pads are 1, the
    second's 5, so avgFromEnd says whose sum was taken: 10."""
    lead = border - s
    lead_tok, lead_rows = _lead_protein(lead)
    tok = [lead_tok] + [[T_RUN]] * (2 * s)
    fn = np.concatenate([[0], np.full(s, 3), np.full(s, 8)])
    pad = np.concatenate([[0], np.full(s, 1), np.full(s, 5)])
    marks = dict(token=T_RUN, first=lead, length=2 * s, head=border)
    return _case("two fn runs of %d either side of item %d" % (s, border), M.token_batch(tok, pad), fn, np.zeros(fn.size), [lead_rows, sig(T_RUN, 0, 10, 3, s, 2 * s)],
                 lead + 2 * s, lead + 2 * s, lead + 1, tok=tok, marks=marks)


def otu_tie_case(border: int, s: int):
    """As fn_tie_case with one fn run (fn 3) of two OTU runs of s proteins each, OTU 2 before item `border` and OTU 6 from it:
    the smaller OTU, 2.  c = n_v = 2 s and the sum is the whole run's: avgFromEnd = (10 s + 14 s) / 2 s = 12."""
    lead = border - s
    lead_tok, lead_rows = _lead_protein(lead)
    tok = [lead_tok] + [[T_RUN]] * (2 * s)
    fn = np.concatenate([[0], np.full(2 * s, 3)])
    otu = np.concatenate([[0], np.full(s, 2), np.full(s, 6)])
    pad = np.concatenate([[0], np.full(s, 1), np.full(s, 5)])
    marks = dict(token=T_RUN, first=lead, length=2 * s, head=border)
    return _case("two OTU runs of %d either side of item %d" % (s, border), M.token_batch(tok, pad), fn, otu, [lead_rows, sig(T_RUN, 2, 12, 3, 2 * s, 2 * s)],
                 lead + 2 * s, lead + 2 * s, lead + 1, tok=tok, marks=marks)


# ---- d. thresholds and the quotient -----------------------------------------------------------------------------------------

PURITY = [(4, 5, 80, True), (3, 4, 80, False), (2, 3, 66, True), (2, 3, 67, False), (1, 1, 100, True)]     # (c, n, purity_pct, in)
MIN_PROTEINS = [(3, 3, True), (3, 4, False), (1, 1, True), (1, 2, False)]                                # (n_v, min_proteins, in)
# (c, n) of the quotient.  purity_pct >= 1 lets no k-mer with 100 c < n through, so (3, 4099) is by rule absent and (41, 4099)
# stands in for it: the same n_v across the scan chunk, with a quotient that is no exact float32
QUOTIENTS = [(1, 3), (2, 3), (1, 7), (5, 6), (1, 10), (3, 4099), (41, 4099)]


def share_case(c: int, n: int, minp: int = 1, pur: int = 1):
    """One k-mer in n proteins, c of them with fn 3 and otu 2 and n - c unannotated, every pad 0: a signature iff n >= minp and
    100 c >= pur n, and then (k-mer, 2, 9, 3, float32(c) / float32(n)).  -> (case, whether it is one)"""
    fn = np.concatenate([np.full(n - c, -1), np.full(c, 3)])
    otu = np.full(n, 2)
    tok = np.full((n, 1), T_RUN, dtype=np.int64)
    is_sig = n >= minp and 100 * c >= pur * n
    rows = [sig(T_RUN, 2, 9, 3, c, n)] if is_sig else []
    return _case("c %d of n %d, min_proteins %d, purity %d" % (c, n, minp, pur), M.token_batch(tok), fn, otu, rows, n, n, 1, minp, pur,
                 tok=tok, marks=dict(token=T_RUN, first=0, length=n)), is_sig


# ---- e. the rank width ------------------------------------------------------------------------------------------------------

RANK_N = (1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097)
PRIVATE = 2 ** 34                           # the first private token: the top bit of a k-mer, 20^8 < 2^35


def rank_width_case(n: int):
    """n proteins: each holds token 7 and, behind it, a private token 2^34 + p; pad p % 5.  Protein 0 has fn 0 and otu 0, every
    other fn = otu = 2^31 - 1: the rank key (fn + 1) << 31 | otu is 63 bits wide, ~otu is packed from 2^31 - 1, and b is
    ceil(log2 n), 0 for one protein.  The one pass spans the k-mer space, so its key is 35 + b bits wide, and without the top one
    private token p would sort as k-mer p: before token 7, or onto it.  Token 7: n_v = n; alone, protein 0's; of two, a tie that
    fn 0 wins; of more, f* = 2^31 - 1 with c = n - 1.  A private token is its protein's second window: len - 9."""
    p = np.arange(n, dtype=np.int64)
    fn = np.where(p == 0, 0, MAXI)
    tok = np.stack([np.full(n, T_LEAD), PRIVATE + p], axis=1)
    pad = p % 5
    length = 18 + pad
    if n <= 2:
        first = sig(T_LEAD, 0, 18, 0, 1, n)
    else:
        first = sig(T_LEAD, MAXI, int(length[1:].sum()) // (n - 1), MAXI, n - 1, n)
    rows = [first, sig(PRIVATE + p, fn, length - 9, fn, 1, 1)]
    return _case("%d proteins" % n, M.token_batch(tok, pad), fn, fn, rows, 2 * n, 2 * n, n + 1, tok=tok, marks=dict(token=T_LEAD, first=0, length=n))


def lone_protein_case(fn: int, otu: int):
    """One protein of one token alone (b = 0, and a pass of one window): no signature unannotated, (token, otu, 9, fn, 1.0) else."""
    tok = np.array([[T_RUN]], dtype=np.int64)
    rows = [sig(T_RUN, otu, 9, fn, 1, 1)] if fn >= 0 else []
    return _case("one protein alone, fn %d otu %d" % (fn, otu), M.token_batch(tok), [fn], [otu], rows, 1, 1, 1, tok=tok)


LONE = [(-1, 0), (-1, 5), (0, 0), (3, 8), (MAXI, MAXI)]


# ---- f. the k-mer space and the pass plan -----------------------------------------------------------------------------------

SPACE_TOKENS = (0, 1, BIN0 - 1, BIN0, BIN0 + 1, TOP - 1, TOP)
# either side of each of a k-mer's top three bits: a one-pass sort that leaves a top bit out puts 2^k on k-mer 0 and 2^k + 1 on 1
TOP_BIT_TOKENS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 33 - 1, 2 ** 33, 2 ** 33 + 1, 2 ** 34 - 1, 2 ** 34, 2 ** 34 + 1, TOP)
LAST_BIN = (20 ** 8 - 1) // BIN0 * BIN0     # the first k-mer of the last top-level bin, which 20^8 clips


def shared_tokens_case(name, tokens, n_prot: int, cap: int = 0, passes=None):
    """n_prot proteins (fn 0, otu p % 2) that each hold all of `tokens`, ascending, in that order: token j is window 9 j of every
    protein, so every k-mer has n_v = c = n_prot, avgFromEnd = 9 (len(tokens) - j) and the OTU mode 0 (the smaller on a tie).
    passes: an int where the cap forces that many, "min" where only ceil(valid / cap) is known."""
    tokens = np.asarray(tokens, dtype=np.int64)
    t = tokens.size
    tok = np.tile(tokens, (n_prot, 1))
    rows = [sig(tokens, 0, 9 * (t - np.arange(t)), 0, n_prot, n_prot)]
    if passes == "min":                                         # no pass holds more windows than the cap
        passes = ("min", -(-t * n_prot // cap))
    return _case(name, M.token_batch(tok), np.zeros(n_prot), np.arange(n_prot) % 2, rows, t * n_prot, t * n_prot, t, cap=cap,
                 passes=passes, tok=tok)


def pass_cases():
    """Every input of the pass plan, each with the cap it is run under (0: one pass)."""
    yield shared_tokens_case("the ends of the k-mer space and of the first top-level bin, one pass", SPACE_TOKENS, 2)
    yield shared_tokens_case("either side of the top bits of a k-mer, one pass", TOP_BIT_TOKENS, 2)
    for c in (1, 3):
        # six k-mers of c windows each in the first BIN1 piece of the first top-level bin: both levels are refined
        yield shared_tokens_case("tokens 0..5 in %d proteins, cap %d: every k-mer a pass of its own, its count equal to the cap" % (c, c),
                                 np.arange(6), c, cap=c, passes=6)
        yield shared_tokens_case("tokens 0..5 in %d proteins, cap %d" % (c, 2 * c), np.arange(6), c, cap=2 * c, passes="min")
        yield shared_tokens_case("tokens 0..5 in %d proteins, cap %d: all in one pass" % (c, 6 * c), np.arange(6), c, cap=6 * c, passes="min")
    spread = 5 * BIN0 + np.arange(3500, dtype=np.int64) * (BIN0 // 3500)        # at most two tokens to a BIN1 piece
    yield shared_tokens_case("3500 tokens spread over top-level bin 5, cap a seventh", spread, 2, cap=1000, passes="min")
    piece = 5 * BIN0 + 7 * BIN1 + np.flatnonzero(np.arange(BIN1) % 41 != 0)     # 1998 of the 2048 k-mers of one BIN1 piece
    yield shared_tokens_case("%d tokens in one BIN1 piece of top-level bin 5, cap a seventh" % piece.size, piece, 3,
                             cap=3 * piece.size // 7, passes="min")
    last = np.arange(TOP - 5000, TOP + 1, dtype=np.int64)
    assert last[0] >= LAST_BIN and LAST_BIN + BIN0 > 20 ** 8
    yield shared_tokens_case("tokens TOP - 5000 .. TOP in the last, partial top-level bin, cap a seventh", last, 2,
                             cap=2 * last.size // 7, passes="min")


def over_the_cap_case():
    """Tokens 0..5 in 3 proteins under cap 2: k-mer 0 alone is over it.  -> (case, the error's text)"""
    return shared_tokens_case("tokens 0..5 in 3 proteins, cap 2", np.arange(6), 3, cap=2), "k-mer 0 alone occurs in 3 valid windows"


# ---- g. window blocks: built by hand ----------------------------------------------------------------------------------------

BLOCK_AT = (0, 55, 56, 63, 64, 65, 127, 128)
BLOCK_LENGTHS = (8, 9, 72, 73)


def window_case(length: int, i: int):
    """Protein 0 is `length` residues, all 'X' but the token under test at position i (fn 4, otu 1); protein 1 is the largest
    token and an 'X'.  Position i is a window iff i < length - 8: a protein that ends in the token (i = length - 8) does not give
    it.  avgFromEnd = length - i."""
    assert 0 <= i <= length - 8
    p0 = b"X" * i + M.token(T_RUN) + b"X" * (length - i - 8)
    is_window = i < length - 8
    rows = ([sig(T_RUN, 1, length - i, 4, 1, 1)] if is_window else []) + [sig(TOP, 0, 9, 0, 1, 1)]
    case = _case("length %d, the token at position %d: %s" % (length, i, "window" if is_window else "no window"),
                 M.pack([p0, M.token(TOP) + b"X"]), [4, 0], [1, 0], rows, len(rows), len(rows), len(rows), marks=dict(length=length, at=i))
    return case, is_window


def window_cases():
    """The token on window 0, 55, 56, 63, 64, 65, 127, 128 of a protein (the borders of the 64-window blocks and of the 64
    residues a lane of the encode reads), with five residues behind it, as the last window (i = length - 9) and as the protein's
    end (i = length - 8); and the lengths 8, 9, 72 and 73 with the token first, as the last window and at the end."""
    seen = set()
    for i in BLOCK_AT:
        for length in (i + 13, i + 9, i + 8):
            seen.add((length, i))
    for length in BLOCK_LENGTHS:
        seen |= {(length, j) for j in (0, length - 9, length - 8) if j >= 0}
    for length, i in sorted(seen):
        yield window_case(length, i)
