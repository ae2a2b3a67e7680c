"""The seed rule of kg_proteins_search_seeded (include/kmerguts_hip.h) restated twice: as plain loops over windows and as sorted
numpy arrays.  Both forms are made for one seed set by shared_loops(seed) / shared_numpy(seed) and have search_model's
`shared(seq, offsets, n_db, max_db_per_kmer)` shape, so search_model.search_model(..., shared=...) runs the whole rule.

A seed set here is (cls, masks): cls the class of each residue in code order ACDEFGHIKLMNPQRSTVWY, masks the shapes, bit j = a
care position.  Nothing of kmergutsjava_amd/seeds.py is used: the written forms are parsed there and checked against this."""
from __future__ import annotations

import numpy as np

import align_model as AM
import search_model as SM

ALPHA = SM.ALPHA
IDENTITY = list(range(20))
REDUCED11_GROUPS = ("AST", "C", "DEKNQR", "F", "G", "H", "ILV", "M", "P", "W", "Y")
REDUCED11 = [next(k for k, g in enumerate(REDUCED11_GROUPS) if chr(ch) in g) for ch in ALPHA]
EXACT = (IDENTITY, [0xFF])
REDUCED = (REDUCED11, [sum(1 << j for j, ch in enumerate(s) if ch == "1") for s in ("111101101011", "110110011010011")])


def span(mask: int) -> int:
    return int(mask).bit_length()


def weight(mask: int) -> int:
    return bin(mask).count("1")


def alphabet_size(cls) -> int:
    return max(cls) + 1


def space(seed) -> int:
    cls, masks = seed
    return len(masks) * alphabet_size(cls) ** weight(masks[0])


def seed_ids(p: bytes, seed):
    """The rule one window at a time: -> the seed id of every valid (window, shape) pair of protein p, in (shape, window) order."""
    cls, masks = seed
    A, w = alphabet_size(cls), weight(masks[0])
    code = {ch: k for k, ch in enumerate(ALPHA)}
    out = []
    for k, mask in enumerate(masks):
        care = [j for j in range(32) if mask >> j & 1]
        for i in range(len(p)):
            if not i + span(mask) < len(p):
                continue
            if any(p[i + j] not in code for j in care):
                continue
            value = 0
            for j in care:                                  # the lowest position is the most significant digit
                value = value * A + cls[code[p[i + j]]]
            out.append(k * A ** w + value)
    return out


def _join(sets_of, n, n_db, max_db_per_kmer, valid):
    """search_model.shared_loops' second half over per-protein sets of seed ids."""
    D, Q, pairs = {}, {}, 0
    for p in range(n):
        pairs += len(sets_of[p])
        for v in sets_of[p]:
            (D if p < n_db else Q).setdefault(v, []).append(p if p < n_db else p - n_db)
    s_of, joined, masked, join_pairs = {}, 0, 0, 0
    for v, ds in D.items():
        if len(ds) > max_db_per_kmer:
            masked += 1
            continue
        qs = Q.get(v, ())
        if not qs:
            continue
        joined += 1
        join_pairs += len(ds) * len(qs)
        for q in qs:
            for d in ds:
                s_of[(q, d)] = s_of.get((q, d), 0) + 1
    counts = dict(targets=n_db, queries=n - n_db, valid_windows=valid, pairs=pairs, kmers=len(set(D) | set(Q)), kmers_joined=joined,
                  kmers_masked=masked, join_pairs=join_pairs)
    return s_of, counts


def shared_loops(seed):
    def shared(seq: bytes, offsets, n_db: int, max_db_per_kmer: int = SM.MAX_DB_PER_KMER):
        seq = bytes(seq)
        n = len(offsets) - 1
        ids = [seed_ids(seq[offsets[p]:offsets[p + 1]], seed) for p in range(n)]
        return _join([set(x) for x in ids], n, n_db, max_db_per_kmer, sum(len(x) for x in ids))
    return shared


def seed_pairs(seq: bytes, offsets, seed):
    """-> (seed ids, protein indices) of every valid (window, shape) pair, by arrays."""
    cls, masks = seed
    A, w = alphabet_size(cls), weight(masks[0])
    seq = bytes(seq)
    n = len(offsets) - 1
    c = AM.codes(seq)
    L = len(c)
    off = np.asarray(offsets, dtype=np.int64)
    length = np.diff(off)
    prot = np.repeat(np.arange(n), length)
    pos = np.arange(L) - off[prot]
    klass = np.r_[np.asarray(cls, dtype=np.int64), -1][np.minimum(c, 20)]         # -1: not a residue
    vs, ps = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for k, mask in enumerate(masks):
        care = np.array([j for j in range(32) if mask >> j & 1], dtype=np.int64)
        at = np.flatnonzero(pos + span(mask) < length[prot])                      # windows wholly inside their own protein
        if at.size == 0:
            continue
        digits = klass[at[:, None] + care[None, :]]
        ok = (digits >= 0).all(axis=1)
        v = (digits[ok] * (A ** np.arange(w - 1, -1, -1, dtype=np.int64))).sum(axis=1)
        vs.append(k * A ** w + v)
        ps.append(prot[at][ok])
    return np.concatenate(vs), np.concatenate(ps)


def shared_numpy(seed):
    def shared(seq: bytes, offsets, n_db: int, max_db_per_kmer: int = SM.MAX_DB_PER_KMER):
        """search_model.shared_numpy with seed_pairs in kmer_pairs' place."""
        n = len(offsets) - 1
        v, p = seed_pairs(seq, offsets, seed)
        counts = dict(targets=n_db, queries=n - n_db, valid_windows=int(v.size), pairs=0, kmers=0, kmers_joined=0, kmers_masked=0,
                      join_pairs=0)
        if v.size == 0:
            return {}, counts
        key = np.unique(v * (n + 1) + p)
        kv, kp = key // (n + 1), key % (n + 1)
        counts["pairs"] = int(key.size)
        head = np.flatnonzero(np.r_[True, kv[1:] != kv[:-1]])
        start = np.r_[head, key.size]
        counts["kmers"] = int(head.size)
        nd = np.add.reduceat((kp < n_db).astype(np.int64), head)
        nq = np.diff(start) - nd
        counts["kmers_masked"] = int((nd > max_db_per_kmer).sum())
        use = np.flatnonzero((nd >= 1) & (nd <= max_db_per_kmer) & (nq >= 1))
        counts["kmers_joined"] = int(use.size)
        wt = nd[use] * nq[use]
        counts["join_pairs"] = int(wt.sum())
        if use.size == 0:
            return {}, counts
        run = np.repeat(np.arange(use.size), wt)
        t = np.arange(int(wt.sum())) - np.repeat(np.cumsum(wt) - wt, wt)
        d = kp[start[use][run] + t % nd[use][run]]
        q = kp[start[use][run] + nd[use][run] + t // nd[use][run]] - n_db
        qd, s = np.unique(q * (n_db + 1) + d, return_counts=True)
        return {(int(x // (n_db + 1)), int(x % (n_db + 1))): int(c) for x, c in zip(qd, s)}, counts
    return shared


def search_model(seq, offsets, n_db, seed, **kw):
    """search_model.search_model under a seed set: -> (records, hit_start, counts)."""
    return SM.search_model(seq, offsets, n_db, shared=shared_numpy(seed), **kw)


def as_dict(seed) -> dict:
    """The seed set as hotpath.search_proteins(seeds=...) takes it."""
    cls, masks = seed
    groups = ["".join(chr(ALPHA[c]) for c in range(20) if cls[c] == a) for a in range(alphabet_size(cls))]
    return dict(alphabet=",".join(groups), shapes=["".join("1" if m >> j & 1 else "0" for j in range(span(m))) for m in masks])


def random_seed(rng, n_shapes=None, max_span: int = 32):
    """A legal seed set: a random class map with every class used, n_shapes shapes of one weight and differing spans."""
    A = int(rng.integers(2, 21))
    cls = list(rng.permutation(np.r_[np.arange(A), rng.integers(0, A, 20 - A)]))
    n_shapes = int(rng.integers(1, 5)) if n_shapes is None else n_shapes
    w = int(rng.integers(1, 9))
    while n_shapes * A ** w > 1 << 35:
        w -= 1
    masks = []
    for _ in range(n_shapes):
        sp = int(rng.integers(w, max_span + 1)) if w > 1 else 1
        inner = rng.choice(np.arange(1, sp - 1), w - 2, replace=False) if w > 2 else []
        masks.append(1 | (1 << (sp - 1) if w > 1 else 0) | sum(1 << int(j) for j in inner))
    return [int(x) for x in cls], masks


def conservative_pairs(rng, n: int, length: int = 200, every: int = 6):
    """The input that shows the feature: n targets of `length` random residues whose every `every`-th position holds a residue
    with company in its reduced11 class, and per target a query that is the target with each of those residues replaced by
    another member of its class.  Five residues in a row survive and never eight, and under reduced11 the two are the same.
    -> (targets, queries).  The caller asserts what it needs of them with the models."""
    others = {ch: [x for x in g.encode() if x != ch] for g in REDUCED11_GROUPS for ch in g.encode()}
    company = [ch for ch in ALPHA if others[ch]]
    targets, queries = [], []
    for _ in range(n):
        t = bytearray(ALPHA[int(x)] for x in rng.integers(0, 20, length))
        for i in range(every // 2, length, every):
            t[i] = company[int(rng.integers(0, len(company)))]
        q = bytearray(t)
        for i in range(every // 2, length, every):
            q[i] = others[t[i]][int(rng.integers(0, len(others[t[i]])))]
        targets.append(bytes(t))
        queries.append(bytes(q))
    return targets, queries
