"""The rule of kg_orfs_free / kg_orfset_add_free (include/kmerguts_hip.h) restated in Python: the exact reference the GPU tests
compare against, byte for byte.  `brute_force` walks every codon of every container with plain loops; `free_orfs` works per
container on flatnonzero of the stops and starts plus searchsorted.  Strand, codons and the genetic code are orfs_model's."""
from __future__ import annotations

import numpy as np

import orfs_model as O
from kmergutsjava_amd._native import ORF_DTYPE

FREE = 16


def _bytes(seq) -> np.ndarray:
    return np.frombuffer(seq, dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq.view(np.uint8).reshape(-1)


def _record(s, strand, f, L, nf, u, e, b, sc):
    last = min(e, nf - 1)
    xs, xe = f + 3 * b, f + 3 * last + 2
    left, right = (xs, xe) if not strand else (L - 1 - xe, L - 1 - xs)
    flags = FREE | (O.HAS_STOP if e < nf else 0) | (O.PARTIAL5 if u == -1 else 0)
    return (s, strand, f, left, right, min(e, nf) - b, sc, -1, flags, -1, 0, 1)


def _finish(recs, prots):
    out = np.zeros(len(recs), dtype=ORF_DTYPE)
    for i, rec in enumerate(recs):
        out[i] = rec
    start = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in prots], out=start[1:])
    res = np.concatenate(prots).astype(np.uint8) if prots else np.zeros(0, np.uint8)
    return out, start, res


def brute_force(seq, offsets, min_res: int = 100, start_codons: int = 7):
    """Rules 1-6 with plain loops over every codon of every container."""
    sb, off = _bytes(seq), [int(x) for x in offsets]
    starts = {c: k + 1 for k, c in enumerate(O.STARTS) if start_codons >> k & 1}
    recs, prots = [], []
    for s in range(len(off) - 1):
        contig = sb[off[s]:off[s + 1]]
        L = len(contig)
        for strand in (0, 1):
            codes = O.strand_codes(contig, strand)
            for f in range(3):
                cod = [int(x) for x in O._codons(codes, f)]
                nf = len(cod)
                u = -1
                for e in range(nf + 1):
                    if e < nf and cod[e] not in O.STOPS:
                        continue
                    if nf == 0:
                        break
                    b = u + 1
                    while b < e and cod[b] not in starts:
                        b += 1
                    sc = starts[cod[b]] if b < e else 0
                    if b == e and (u == -1 or start_codons == 0):
                        b = u + 1                                   # (an empty run stays at b == e and gives nothing)
                    if b < e and min(e, nf) - b >= min_res:
                        recs.append(_record(s, strand, f, L, nf, u, e, b, sc))
                        prots.append(O._protein(np.array(cod, np.int64), b, min(e, nf) - b, sc))
                    u = e
    return _finish(recs, prots)


def free_orfs(seq, offsets, min_res: int = 100, start_codons: int = 7):
    """seq bytes / uint8 array, offsets int64[n_seqs + 1] -> (ORF_DTYPE records, prot_start int64[n + 1], residues uint8)."""
    sb, off = _bytes(seq), np.asarray(offsets, dtype=np.int64)
    starts = [c for k, c in enumerate(O.STARTS) if start_codons >> k & 1]
    parts, prots = [], []
    for s in range(off.size - 1):
        contig = sb[off[s]:off[s + 1]]
        L = len(contig)
        for strand in (0, 1):
            codes = O.strand_codes(contig, strand)
            for f in range(3):
                cod = O._codons(codes, f)
                nf = len(cod)
                if nf == 0:
                    continue
                e = np.append(np.flatnonzero(np.isin(cod, O.STOPS)), nf)           # every run's end
                u = np.append(-1, e[:-1])
                e, u = e[e - u - 1 >= min_res], u[e - u - 1 >= min_res]             # the cheap necessary test
                if not e.size:
                    continue
                st = np.flatnonzero(np.isin(cod, starts)) if starts else np.zeros(0, np.int64)
                k = np.searchsorted(st, u + 1)
                found = k < st.size
                b = np.where(found, st[np.minimum(k, max(st.size - 1, 0))] if st.size else 0, nf + 1)
                found = found & (b < e)
                ok = found | (u == -1) | (start_codons == 0)
                b = np.where(found, b, u + 1)
                ok &= np.minimum(e, nf) - b >= min_res
                e, u, b, found = e[ok], u[ok], b[ok], found[ok]
                n = e.size
                if not n:
                    continue
                last = np.minimum(e, nf - 1)
                xs, xe = f + 3 * b, f + 3 * last + 2
                rec = np.zeros(n, dtype=ORF_DTYPE)
                rec["seq"], rec["strand"], rec["frame"] = s, strand, f
                rec["left"] = xs if not strand else L - 1 - xe
                rec["right"] = xe if not strand else L - 1 - xs
                rec["n_res"] = np.minimum(e, nf) - b
                scs = np.zeros(n, np.int32)
                for idx, c in enumerate(O.STARTS):
                    scs[found & (cod[b] == c)] = idx + 1
                rec["start_codon"] = scs
                rec["first_inner"], rec["fI"], rec["score"], rec["kept"] = -1, -1, 0, 1
                rec["flags"] = FREE | np.where(e < nf, O.HAS_STOP, 0) | np.where(u == -1, O.PARTIAL5, 0)
                parts.append(rec)
                prots += [O._protein(cod, int(bb), int(nn), int(cc)) for bb, nn, cc in zip(b, rec["n_res"], scs)]
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=ORF_DTYPE)
    start = np.zeros(len(out) + 1, dtype=np.int64)
    np.cumsum(out["n_res"], out=start[1:])
    res = np.concatenate(prots).astype(np.uint8) if prots else np.zeros(0, np.uint8)
    return out, start, res


def concat(parent, free):
    """(records, prot_start, residues) of kg_orfset_add_free from the parent's and the free candidates' triples."""
    return (np.concatenate([parent[0], free[0]]), np.concatenate([parent[1], parent[1][-1] + free[1][1:]]),
            np.concatenate([parent[2], free[2]]))
