"""The ORF rule of kg_regionset_orfs / kg_orfs_regions (include/kmerguts_hip.h) restated in numpy: the exact reference the GPU
tests compare against, byte for byte.  `orfs` uses a prefix maximum and suffix minima over each (contig, strand, frame) it needs;
`brute_force` walks a materialised strand with plain loops.  Imports nothing from kmergutsjava_amd but the record dtypes."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd._native import ORF_DTYPE, REGION_DTYPE

HAS_STOP, PARTIAL5, INTERRUPTED, MULTI_FRAME = 1, 2, 4, 8
GENETIC_CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"      # KGJ:88-93, index c1*16 + c2*4 + c3
_LETTER = np.frombuffer(GENETIC_CODE.encode(), dtype=np.uint8)
_CODE = np.full(256, 4, dtype=np.int64)
for _i, _chars in enumerate(("aA", "cC", "gG", "tTuU")):
    for _ch in _chars:
        _CODE[ord(_ch)] = _i
STOPS = (3 * 16 + 0 * 4 + 0, 3 * 16 + 0 * 4 + 2, 3 * 16 + 2 * 4 + 0)           # TAA TAG TGA
STARTS = (0 * 16 + 3 * 4 + 2, 2 * 16 + 3 * 4 + 2, 3 * 16 + 3 * 4 + 2)          # ATG GTG TTG: bits 1, 2, 4; start_codon 1, 2, 3


def strand_codes(contig: np.ndarray, strand: int) -> np.ndarray:
    """Rule 1: the dna_code values of the strand, 5' to 3'."""
    c = _CODE[contig]
    if strand:
        c = c[::-1]
        c = np.where(c < 4, 3 - c, 4)
    return c


def _codons(codes: np.ndarray, f: int):
    """(codon index 0..63 or -1 for unknown) of every codon of frame f"""
    n = (len(codes) - f) // 3 if len(codes) >= f else 0
    if n <= 0:
        return np.zeros(0, np.int64)
    t = codes[f:f + 3 * n].reshape(n, 3)
    return np.where((t < 4).all(axis=1), t[:, 0] * 16 + t[:, 1] * 4 + t[:, 2], -1)


def anchor(r, L: int):
    """Rule 2: (f, n_f, j0, j1) of a region on a contig of L nucleotides."""
    f = int(r["best_frame"])
    nf = (L - f) // 3 if L >= f else 0
    xa, xb = (int(r["left"]), int(r["right"])) if not r["strand"] else (L - 1 - int(r["right"]), L - 1 - int(r["left"]))
    j0 = -((f - xa) // 3)               # ceil((xa - f) / 3)
    j1 = (xb - 2 - f) // 3
    return f, nf, max(j0, 0), j1


def _check(r, n_seqs, off):
    assert 0 <= r["seq"] < n_seqs and r["strand"] in (0, 1) and 0 <= r["best_frame"] <= 2
    L = int(off[r["seq"] + 1] - off[r["seq"]])
    assert 0 <= r["left"] <= r["right"] < L
    f, nf, j0, j1 = anchor(r, L)
    assert 0 <= j0 <= j1 < nf
    return L, f, nf, j0, j1


def _record(r, L, f, nf, u, e, b, istar, start_codon):
    last = min(e, nf - 1)
    xs, xe = f + 3 * b, f + 3 * last + 2
    left, right = (xs, xe) if not r["strand"] else (L - 1 - xe, L - 1 - xs)
    flags = ((HAS_STOP if e < nf else 0) | (PARTIAL5 if u == -1 else 0) | (INTERRUPTED if istar >= 0 else 0) |
             (MULTI_FRAME if int(r["frames"]) & (int(r["frames"]) - 1) else 0))
    return (r["seq"], r["strand"], f, left, right, min(e, nf) - b, start_codon, istar - b if istar >= 0 else -1, flags, r["fI"],
            r["score"], r["kept"])


def _protein(cod, b, n_res, start_codon):
    c = cod[b:b + n_res]
    p = np.where(c >= 0, _LETTER[np.maximum(c, 0)], ord("X")).astype(np.uint8)
    if n_res and start_codon:
        p[0] = ord("M")
    return p


def _finish(recs, prots, only_kept):
    out = np.zeros(len(recs), dtype=ORF_DTYPE)
    for i, rec in enumerate(recs):
        out[i] = rec
    lens = np.array([len(p) if (o["kept"] or not only_kept) else 0 for p, o in zip(prots, out)], dtype=np.int64)
    start = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum(lens, out=start[1:])
    res = (np.concatenate([p[:n] for p, n in zip(prots, lens)]) if len(recs) else np.zeros(0, np.uint8)).astype(np.uint8)
    return out, start, res


def orfs(regs, seq, offsets, start_codons: int = 7, only_kept: bool = True):
    """regs REGION_DTYPE, seq bytes / uint8 array, offsets int64[n_seqs + 1] -> (ORF_DTYPE records, prot_start int64[n + 1],
    residues uint8)."""
    regs = np.asarray(regs, dtype=REGION_DTYPE)
    sb = np.frombuffer(seq, dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq.view(np.uint8).reshape(-1)
    off = np.asarray(offsets, dtype=np.int64)
    n_seqs = off.size - 1
    starts = [c for k, c in enumerate(STARTS) if start_codons >> k & 1]
    cache = {}
    recs, prots = [], []
    for r in regs:
        L, f, nf, j0, j1 = _check(r, n_seqs, off)
        key = (int(r["seq"]), int(r["strand"]), f)
        if key not in cache:
            if cache and next(iter(cache))[0] != key[0]:
                cache.clear()               # one contig's arrays at a time: region lists come sorted by contig
            cod = _codons(strand_codes(sb[off[key[0]]:off[key[0] + 1]], key[1]), f)
            idx = np.arange(nf, dtype=np.int64)
            is_stop = np.isin(cod, STOPS)
            is_start = np.isin(cod, starts) if starts else np.zeros(nf, bool)
            last_stop = np.maximum.accumulate(np.where(is_stop, idx, -1))                      # the largest stop <= j
            next_stop = np.minimum.accumulate(np.where(is_stop, idx, nf)[::-1])[::-1]          # the smallest stop >= j
            next_start = np.minimum.accumulate(np.where(is_start, idx, nf)[::-1])[::-1]
            cache[key] = (cod, last_stop, next_stop, next_start)
        cod, last_stop, next_stop, next_start = cache[key]
        u = int(last_stop[j0 - 1]) if j0 > 0 else -1
        e = int(next_stop[j1 + 1]) if j1 + 1 < nf else nf
        s = int(next_start[u + 1])
        b = s if s <= j0 else u + 1
        i = int(next_stop[j0])
        istar = i if i <= j1 else -1
        sc = STARTS.index(int(cod[b])) + 1 if s <= j0 else 0
        rec = _record(r, L, f, nf, u, e, b, istar, sc)
        recs.append(rec)
        prots.append(_protein(cod, b, rec[5], sc))
    return _finish(recs, prots, only_kept)


def brute_force(regs, seq, offsets, start_codons: int = 7, only_kept: bool = True):
    """The same rule with plain loops over a materialised strand."""
    sb = bytes(seq)
    off = [int(x) for x in offsets]
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    names = {"ATG": 1, "GTG": 2, "TTG": 3}
    recs, prots = [], []
    for r in regs:
        L, f, nf, j0, j1 = _check(r, len(off) - 1, off)
        text = "".join("ACGTN"[_CODE[ch]] for ch in sb[off[r["seq"]]:off[r["seq"] + 1]])
        if r["strand"]:
            text = "".join(comp[ch] for ch in reversed(text))
        codon = [text[f + 3 * j:f + 3 * j + 3] for j in range(nf)]

        def stop(j):
            return codon[j] in ("TAA", "TAG", "TGA")

        def start(j):
            return codon[j] in names and (start_codons >> (names[codon[j]] - 1)) & 1

        u = j0 - 1
        while u >= 0 and not stop(u):
            u -= 1
        e = j1 + 1
        while e < nf and not stop(e):
            e += 1
        b = u + 1
        while b <= j0 and not start(b):
            b += 1
        sc = names[codon[b]] if b <= j0 else 0
        if b > j0:
            b = u + 1
        istar = -1
        for j in range(j0, j1 + 1):
            if stop(j):
                istar = j
                break
        rec = _record(r, L, f, nf, u, e, b, istar, sc)
        recs.append(rec)
        p = []
        for j in range(b, b + rec[5]):
            c = codon[j]
            p.append("X" if "N" in c else GENETIC_CODE["ACGT".index(c[0]) * 16 + "ACGT".index(c[1]) * 4 + "ACGT".index(c[2])])
        if p and sc:
            p[0] = "M"
        prots.append(np.frombuffer("".join(p).encode(), dtype=np.uint8))
    return _finish(recs, prots, only_kept)


def region(seq, strand, left, right, best_frame, fI=7, score=5, kept=1, frames=None):
    """One REGION_DTYPE record as a tuple (weighted 1.0, one CALL)."""
    return (seq, strand, left, right, fI, score, 1.0, 1, (1 << best_frame) if frames is None else frames, best_frame, 0, kept)


def regions_of(rows) -> np.ndarray:
    out = np.zeros(len(rows), dtype=REGION_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def codon_region(L, strand, f, j0, j1, seq=0, **kw):
    """The region that covers exactly codons j0 .. j1 of frame f of a strand of a contig of L nucleotides."""
    xa, xb = f + 3 * j0, f + 3 * j1 + 2
    left, right = (xa, xb) if not strand else (L - 1 - xb, L - 1 - xa)
    return region(seq, strand, left, right, f, **kw)


ALPHABET = np.frombuffer(b"ACGTUacgtN-", dtype=np.uint8)


def random_batch(rng, n_seqs: int, max_len: int = 400, max_regions: int = 6, alphabet=ALPHABET, weights=None):
    """Random contigs over ACGTUacgtN- with lengths 0 .. max_len (L < 3 + f included: such a frame gets no region) and random
    valid regions on them, some with ragged ends, some unkept, some multi-frame.  -> (regions, bytes, offsets)."""
    lens = rng.integers(0, max_len + 1, size=n_seqs)
    if n_seqs:
        lens[rng.integers(0, n_seqs)] = int(rng.integers(0, 6))
    off = np.zeros(n_seqs + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    seq = rng.choice(alphabet, size=int(off[-1]), p=weights).astype(np.uint8)
    rows = []
    for s in range(n_seqs):
        L = int(lens[s])
        for _ in range(int(rng.integers(0, max_regions + 1))):
            strand, f = int(rng.integers(0, 2)), int(rng.integers(0, 3))
            nf = (L - f) // 3 if L >= f else 0
            if nf < 1:
                continue
            j0 = int(rng.integers(0, nf))
            j1 = min(nf - 1, j0 + int(rng.integers(0, 12)) * int(rng.choice([0, 1, 1, 5])))
            xa = max(0, f + 3 * j0 - int(rng.integers(0, 3)))            # ragged ends stay inside the same codons
            xb = min(L - 1, f + 3 * j1 + 2 + int(rng.integers(0, 3)))
            left, right = (xa, xb) if not strand else (L - 1 - xb, L - 1 - xa)
            frames = (1 << f) | (int(rng.integers(0, 8)) if rng.random() < 0.3 else 0)
            rows.append(region(s, strand, left, right, f, fI=int(rng.integers(-1, 4)), score=int(rng.integers(0, 50)),
                               kept=int(rng.random() < 0.7), frames=frames))
    return regions_of(rows), seq, off
