"""The coding-potential rule of kg_orfset_coding (include/kmerguts_hip.h) restated twice: with plain loops over a materialised
strand (`*_loops`), word for word as the header has it, and in numpy (`*_np`), the exact reference the GPU tests compare against,
byte for byte.  Imports nothing from kmergutsjava_amd but the record dtype."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd._native import ORF_DTYPE

INTERRUPTED, FREE, NONCODING = 4, 16, 32
BINS = 4096
_CODE = np.full(256, 4, dtype=np.int64)
for _i, _chars in enumerate(("aA", "cC", "gG", "tTuU")):
    for _ch in _chars:
        _CODE[ord(_ch)] = _i
_POW = 4 ** np.arange(5, -1, -1, dtype=np.int64)


def _bytes(seq) -> np.ndarray:
    return np.frombuffer(seq, dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq.view(np.uint8).reshape(-1)


# ---- rule 5: Lg and the table ---------------------------------------------------------------------------------------------------

def lg(x: int) -> int:
    assert 1 <= x < 1 << 63
    n = x.bit_length() - 1
    y, f = x << (63 - n), 0
    for _ in range(8):
        y = (y * y) >> 63
        if y >= 1 << 64:
            y >>= 1
            f = 2 * f + 1
        else:
            f = 2 * f
    return 256 * n + f


def table(coding, background) -> np.ndarray:
    C, B = [int(x) for x in coding], [int(x) for x in background]
    assert len(C) == len(B) == BINS and min(C) >= 0 and min(B) >= 0 and sum(C) < 1 << 62 and sum(B) < 1 << 62
    lsc, lsb = lg(sum(C) + BINS), lg(sum(B) + BINS)
    return np.array([lg(C[h] + 1) - lsc - lg(B[h] + 1) + lsb for h in range(BINS)], dtype=np.int32)


def rc(h: int) -> int:
    d = [(h >> (2 * (5 - i))) & 3 for i in range(6)]
    return sum((3 - b) << (2 * (5 - i)) for i, b in enumerate(reversed(d)))


_RC = np.array([rc(h) for h in range(BINS)], dtype=np.int64)


# ---- plain loops ----------------------------------------------------------------------------------------------------------------

def _strand(contig, strand: int) -> list:
    """Rule 1 of the ORF section: the dna_code values of the strand, 5' to 3'."""
    L = len(contig)
    if not strand:
        return [int(_CODE[contig[x]]) for x in range(L)]
    out = []
    for x in range(L):
        c = int(_CODE[contig[L - 1 - x]])
        out.append(3 - c if c < 4 else 4)
    return out


def _hexamer(b) -> int:
    """Rule 1: the index of six bases, or -1 when one of them has code 4."""
    if any(x > 3 for x in b):
        return -1
    h = 0
    for x in b:
        h = h * 4 + x
    return h


def pairs_loops(o, seq, off) -> list:
    """Rule 2: the hexamer index (or -1) of every pair of one record."""
    sb = _bytes(seq)
    s = int(o["seq"])
    contig = sb[int(off[s]):int(off[s + 1])]
    L = len(contig)
    text = _strand(contig, int(o["strand"]))
    xs = int(o["left"]) if not o["strand"] else L - 1 - int(o["right"])
    out = []
    for k in range(int(o["n_res"]) - 1):
        out.append(_hexamer(text[xs + 3 * k:xs + 3 * k + 6]))
        assert len(text[xs + 3 * k:xs + 3 * k + 6]) == 6
    return out


def is_training(o) -> bool:
    return bool(o["kept"] != 0 and (int(o["flags"]) & (FREE | INTERRUPTED)) == 0)


def counts_loops(orfs, seq, off):
    """Rules 3 and 4 -> (C, B), int64[4096] each."""
    sb = _bytes(seq)
    C, B = np.zeros(BINS, np.int64), np.zeros(BINS, np.int64)
    for o in orfs:
        if is_training(o):
            for h in pairs_loops(o, sb, off):
                if h >= 0:
                    C[h] += 1
    for s in range(len(off) - 1):
        text = _strand(sb[int(off[s]):int(off[s + 1])], 0)
        for x in range(0, len(text) - 5):
            h = _hexamer(text[x:x + 6])
            if h >= 0:
                B[h] += 1
                B[rc(h)] += 1
    return C, B


def scores_loops(T, orfs, seq, off) -> np.ndarray:
    """Rule 6."""
    return np.array([sum(int(T[h]) for h in pairs_loops(o, seq, off) if h >= 0) for o in orfs], dtype=np.int64)


# ---- numpy ----------------------------------------------------------------------------------------------------------------------

def pairs_np(o, sb, off) -> np.ndarray:
    n = int(o["n_res"])
    if n < 2:
        return np.zeros(0, np.int64)
    a = int(off[int(o["seq"])])
    if not o["strand"]:
        seg = _CODE[sb[a + int(o["left"]):a + int(o["left"]) + 3 * n]]
    else:
        seg = _CODE[sb[a + int(o["right"]) - 3 * n + 1:a + int(o["right"]) + 1]][::-1]
        seg = np.where(seg < 4, 3 - seg, 4)
    assert seg.size == 3 * n
    t = seg.reshape(n, 3)
    cod = np.where((t < 4).all(axis=1), t[:, 0] * 16 + t[:, 1] * 4 + t[:, 2], -1)
    return np.where((cod[:-1] >= 0) & (cod[1:] >= 0), cod[:-1] * 64 + cod[1:], -1)


def background_np(seq, off) -> np.ndarray:
    sb = _bytes(seq)
    F = np.zeros(BINS, np.int64)
    for s in range(len(off) - 1):
        c = _CODE[sb[int(off[s]):int(off[s + 1])]]
        if c.size < 6:
            continue
        n = c.size - 5
        h, ok = np.zeros(n, np.int64), np.ones(n, bool)
        for i in range(6):
            h += c[i:i + n] * _POW[i]
            ok &= c[i:i + n] < 4
        F += np.bincount(h[ok], minlength=BINS)
    return F + F[_RC]


def counts_np(orfs, seq, off):
    sb = _bytes(seq)
    C = np.zeros(BINS, np.int64)
    for o in orfs:
        if is_training(o):
            h = pairs_np(o, sb, off)
            C += np.bincount(h[h >= 0], minlength=BINS)
    return C, background_np(sb, off)


def scores_np(T, orfs, seq, off) -> np.ndarray:
    sb = _bytes(seq)
    T = np.asarray(T, dtype=np.int64)
    out = np.zeros(len(orfs), dtype=np.int64)
    for i, o in enumerate(orfs):
        h = pairs_np(o, sb, off)
        out[i] = T[h[h >= 0]].sum()
    return out


# ---- rules 7 and 8: the whole call ------------------------------------------------------------------------------------------------

def decide(orfs, scores, min_coding: int = 0) -> np.ndarray:
    out = np.array(orfs, dtype=ORF_DTYPE, copy=True)
    drop = ((out["flags"] & FREE) != 0) & (out["kept"] != 0) & (np.asarray(scores) < min_coding)
    out["kept"][drop] = 0
    out["flags"][drop] |= NONCODING
    return out


def coding(orfs, seq, off, tab=None, min_coding: int = 0, min_train_pairs: int = 100000, loops: bool = False):
    """kg_orfset_coding -> (records, scores, statistics without the times, (C, B)).  `noncoding` counts what this call dropped:
    a record that came with the flag and kept = 0 is not dropped again."""
    orfs = np.asarray(orfs, dtype=ORF_DTYPE)
    n_train = int(sum(is_training(o) for o in orfs))
    if tab is None:
        C, B = (counts_loops if loops else counts_np)(orfs, seq, off)
        trained = 1 if int(C.sum()) >= min_train_pairs else 0
        if trained:
            tab = table(C, B)
    else:
        C, B, trained = np.zeros(BINS, np.int64), np.zeros(BINS, np.int64), 2
    scores = (scores_loops if loops else scores_np)(tab, orfs, seq, off) if trained else np.zeros(len(orfs), np.int64)
    out = decide(orfs, scores, min_coding) if trained else orfs.copy()
    st = {"scored": len(orfs), "training_records": n_train, "training_pairs": int(C.sum()), "background": int(B.sum()),
          "noncoding": int((((out["flags"] & NONCODING) != 0) & ((orfs["flags"] & NONCODING) == 0)).sum()), "trained": trained}
    return out, scores, st, (C, B)


# ---- test inputs ------------------------------------------------------------------------------------------------------------------

def orf(seq, strand, left, right, n_res, flags=1, kept=1, fI=3, score=9, frame=0, start_codon=0):
    """One ORF_DTYPE record as a tuple."""
    return (seq, strand, frame, left, right, n_res, start_codon, -1, flags, fI, score, kept)


def records(rows) -> np.ndarray:
    out = np.zeros(len(rows), dtype=ORF_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def codon_orf(L: int, strand: int, f: int, b: int, n_res: int, stop: bool = True, seq: int = 0, **kw):
    """The record whose codons are b .. b + n_res - 1 of frame f of a strand of a contig of L nucleotides, with the stop codon
    behind them inside its coordinates when `stop`."""
    xs, xe = f + 3 * b, f + 3 * (b + n_res + (1 if stop else 0)) - 1
    assert 0 <= xs and xe < L
    left, right = (xs, xe) if not strand else (L - 1 - xe, L - 1 - xs)
    return orf(seq, strand, left, right, n_res, frame=f, **kw)


ALPHABET = np.frombuffer(b"ACGTUacgtuN-", dtype=np.uint8)


def random_batch(rng, n_seqs: int, max_len: int = 60, max_orfs: int = 5, weights=None, lens=None):
    """Random contigs over ACGTUacgtuN- (lengths 0 .. max_len, some of 0 .. 8) with random valid records on them: both strands,
    all frames, with and without a stop inside the coordinates, n_res from 0, evidence and free, kept and not.  lens: the
    contigs' lengths instead of random ones.  -> (records, bytes, offsets)."""
    if lens is None:
        lens = rng.integers(0, max_len + 1, size=n_seqs)
        for k in range(n_seqs):
            if rng.random() < 0.3:
                lens[k] = int(rng.integers(0, 9))
    lens = np.asarray(lens, dtype=np.int64)
    n_seqs = len(lens)
    off = np.zeros(n_seqs + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    seq = rng.choice(ALPHABET, size=int(off[-1]), p=weights).astype(np.uint8)
    rows = []
    for s in range(n_seqs):
        L = int(lens[s])
        for _ in range(int(rng.integers(0, max_orfs + 1))):
            strand, f = int(rng.integers(0, 2)), int(rng.integers(0, 3))
            nf = (L - f) // 3 if L >= f else 0
            if nf < 1:
                continue
            b = int(rng.integers(0, nf))
            stop = bool(rng.integers(0, 2)) and b + 1 < nf
            n_res = int(rng.integers(0, nf - b - (1 if stop else 0) + 1))
            if n_res == 0 and not stop:
                continue
            flags = int(rng.choice([1, 3, 5, 9, 16, 17, 19]))
            rows.append(codon_orf(L, strand, f, b, n_res, stop, seq=s, flags=flags, kept=int(rng.random() < 0.8),
                                  fI=-1 if flags & FREE else int(rng.integers(0, 5)), score=0 if flags & FREE else int(rng.integers(2, 40))))
    return records(rows), seq, off
