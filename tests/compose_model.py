"""The composition rule of kg_contigs_compose (include/kmerguts_hip.h) restated in plain numpy and Python integers, rules 1 to 8:
the exact reference the GPU tests compare against, byte for byte.  Lg is the coding model's.  Imports nothing from
kmergutsjava_amd but the record dtype."""
from __future__ import annotations

import numpy as np

from coding_model import _CODE, _bytes, lg
from kmergutsjava_amd._native import COMP_CLASS_DTYPE

BINS = 256
_POW = 4 ** np.arange(3, -1, -1, dtype=np.int64)


def rc(t: int) -> int:
    d = [(t >> (2 * (3 - i))) & 3 for i in range(4)]
    return sum((3 - b) << (2 * (3 - i)) for i, b in enumerate(reversed(d)))


_RC = np.array([rc(t) for t in range(BINS)], dtype=np.int64)
PALINDROMES = [t for t in range(BINS) if rc(t) == t]
assert len(PALINDROMES) == 16


def index(four: bytes) -> int:
    """Rule 1: the index of four bases, or -1 when one of them has code 4."""
    c = [int(_CODE[b]) for b in four]
    assert len(c) == 4
    return -1 if max(c) > 3 else sum(b * 4 ** (3 - i) for i, b in enumerate(c))


def forward(contig) -> np.ndarray:
    """F: the forward tetramers of one contig, int64[256]."""
    c = _CODE[_bytes(contig)]
    if c.size < 4:
        return np.zeros(BINS, np.int64)
    n = c.size - 3
    t, ok = np.zeros(n, np.int64), np.ones(n, bool)
    for i in range(4):
        t += c[i:i + n] * _POW[i]
        ok &= c[i:i + n] < 4
    return np.bincount(t[ok], minlength=BINS).astype(np.int64)


def contig_counts_loops(seq, off) -> np.ndarray:
    """Rule 2, contig by contig: N, int32[n_seqs][256]."""
    sb = _bytes(seq)
    out = np.zeros((len(off) - 1, BINS), dtype=np.int32)
    for s in range(len(off) - 1):
        assert int(off[s + 1]) - int(off[s]) < 1 << 30
        F = forward(sb[int(off[s]):int(off[s + 1])])
        out[s] = F + F[_RC]
    return out


def contig_counts(seq, off) -> np.ndarray:
    """Rule 2 over the whole batch at once (70 000 contigs take no longer than one): every window start, the contig that holds
    it, and whether the window ends inside it."""
    sb, off = _bytes(seq), np.asarray(off, dtype=np.int64)
    n, total = len(off) - 1, int(off[-1])
    F = np.zeros((n, BINS), dtype=np.int64)
    if n and total >= 4:
        assert int(np.diff(off).max()) < 1 << 30
        c = _CODE[sb[:total]]
        m = total - 3
        t, ok = np.zeros(m, np.int64), np.ones(m, bool)
        for i in range(4):
            t += c[i:i + m] * _POW[i]
            ok &= c[i:i + m] < 4
        pos = np.arange(m, dtype=np.int64)
        s = np.searchsorted(off, pos, side="right") - 1         # the last contig that begins at or before pos
        ok &= (s >= 0) & (s < n)
        s = np.clip(s, 0, n - 1)
        ok &= pos + 4 <= off[s + 1]
        F = np.bincount(s[ok] * BINS + t[ok], minlength=n * BINS).reshape(n, BINS)
    return (F + F[:, _RC]).astype(np.int32)


def label_rows(N, labels):
    """Rule 3 -> (row labels int32[R] ascending, C int64[R][256], G int64[256])."""
    labels = np.asarray(labels, dtype=np.int64)
    assert (labels >= -1).all()
    rows = np.unique(labels[labels >= 0]).astype(np.int32)
    N64 = np.asarray(N, dtype=np.int64).reshape(-1, BINS)
    C = np.zeros((len(rows), BINS), dtype=np.int64)
    for r, b in enumerate(rows):
        C[r] = N64[labels == b].sum(axis=0)
    return rows, C, N64.sum(axis=0)


def weights(row) -> np.ndarray:
    """Rule 5: one row of W."""
    c = [int(x) for x in row]
    assert len(c) == BINS and min(c) >= 0 and sum(c) < 1 << 62
    ls = lg(sum(c) + BINS)
    return np.array([lg(x + 1) - ls for x in c], dtype=np.int32)


def models_of(rows, C, G, min_train: int):
    """Rule 4 for the rows a call made -> (model labels int32[M], counts int64[M + 1][256], the background last)."""
    keep = [r for r in range(len(rows)) if int(C[r].sum()) >= min_train]
    return np.asarray(rows, np.int32)[keep], np.concatenate([np.asarray(C, np.int64).reshape(-1, BINS)[keep], np.asarray(G, np.int64).reshape(1, BINS)])


def scores(N, counts) -> np.ndarray:
    """Rule 6: S int64[n_seqs][M + 1] under the model rows `counts` (the background last)."""
    W = np.stack([weights(r) for r in counts]).astype(np.int64)
    return np.asarray(N, dtype=np.int64).reshape(-1, BINS) @ W.T


def classes(S, lens, labels, model_labels, min_len: int = 1500, min_margin: int = 2560, windows=None) -> np.ndarray:
    """Rules 7 and 8."""
    n, M = len(lens), len(model_labels)
    out = np.zeros(n, dtype=COMP_CLASS_DTYPE)
    name = [int(x) for x in model_labels] + [-1]
    for s in range(n):
        row = [int(x) for x in S[s]]
        order = sorted(range(M + 1), key=lambda m: (-row[m], m))
        c = out[s]
        c["label"] = labels[s]
        c["windows"] = 0 if windows is None else windows[s]
        c["score_best"] = row[order[0]]
        if M == 0:
            c["best"] = c["second"] = -1
            c["score_second"] = c["score_best"]
            continue
        b, z = order[0], order[1]
        c["best"], c["second"], c["score_second"] = name[b], name[z], row[z]
        c["decided"] = int(lens[s] >= min_len and b < M and row[b] - row[z] >= min_margin)
    return out


def compose(seq, off, labels=None, model=None, min_len: int = 1500, min_margin: int = 2560, min_train: int = 200000):
    """kg_contigs_compose -> dict(classes, counts, row_labels, rows, background, model_labels, scores, stats without the times).
    model: (labels, counts int64[M + 1][256]) or None."""
    off = np.asarray(off, dtype=np.int64)
    n = len(off) - 1
    labels = np.full(n, -1, np.int32) if labels is None else np.asarray(labels, dtype=np.int32)
    N = contig_counts(seq, off)
    if model is None:
        rows, C, G = label_rows(N, labels)
        mlab, counts = models_of(rows, C, G, min_train)
    else:
        rows, C, G = np.zeros(0, np.int32), np.zeros((0, BINS), np.int64), np.zeros(BINS, np.int64)
        mlab, counts = np.asarray(model[0], np.int32), np.asarray(model[1], np.int64).reshape(-1, BINS)
        assert len(counts) == len(mlab) + 1 and (np.diff(mlab.astype(np.int64)) > 0).all() and (mlab >= 0).all()
    S = scores(N, counts)
    windows = N.astype(np.int64).sum(axis=1)
    cls = classes(S, np.diff(off), labels, mlab, min_len, min_margin, windows)
    dec = cls["decided"] != 0
    st = {"seqs": n, "labelled": int((labels >= 0).sum()), "label_rows": len(rows), "models": len(mlab), "windows": int(windows.sum()),
          "decided": int(dec.sum()), "decided_unlabelled": int((dec & (labels < 0)).sum()),
          "conflicts": int((dec & (labels >= 0) & (cls["best"] != labels)).sum())}
    return {"classes": cls, "counts": N, "row_labels": rows, "rows": C, "background": G, "model_labels": mlab, "scores": S, "stats": st}
