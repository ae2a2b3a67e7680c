"""The start-codon rule of kg_orfset_starts (include/kmerguts_hip.h) restated twice: with plain loops over a materialised strand
(`loops=True`), word for word as the header has it, and in numpy on top of coding_model, the exact reference the GPU tests
compare against, byte for byte.  Imports nothing from kmergutsjava_amd but the record dtype."""
from __future__ import annotations

import numpy as np

import coding_model as cm
from kmergutsjava_amd._native import ORF_DTYPE

PARTIAL5, INTERRUPTED, FREE, NONCODING, MOVED = 2, 4, 16, 32, 64
WIN = 20
_TYPES = {(0, 3, 2): 1, (2, 3, 2): 2, (3, 3, 2): 3}         # ATG, GTG, TTG


def is_movable(o) -> bool:
    return bool(o["kept"] != 0 and o["start_codon"] != 0 and (int(o["flags"]) & (INTERRUPTED | NONCODING)) == 0 and o["n_res"] >= 1)


def is_training(o) -> bool:
    return is_movable(o) and (int(o["flags"]) & (FREE | PARTIAL5)) == 0


def zero_model():
    return (np.zeros((WIN, 4), np.int64), np.zeros((WIN, 4), np.int64), np.zeros(4, np.int64), np.zeros(4, np.int64))


# ---- rule 7 -----------------------------------------------------------------------------------------------------------------------

def weights_from(chosen, cand, type_chosen, type_cand):
    """-> (pos int32[20][4], type int32[4]); ValueError where kg_start_weights_from gives KG_ERR_ARG."""
    pos, typ = np.zeros((WIN, 4), np.int32), np.zeros(4, np.int32)

    def row(ch, ca, first):
        ch, ca = [int(x) for x in ch[first:]], [int(x) for x in ca[first:]]
        if min(ch) < 0 or min(ca) < 0 or sum(ch) >= 1 << 62 or sum(ca) >= 1 << 62:
            raise ValueError("bad counts")
        w = len(ch)
        ls, lc = cm.lg(sum(ch) + w), cm.lg(sum(ca) + w)
        return [cm.lg(ch[c] + 1) - ls - cm.lg(ca[c] + 1) + lc for c in range(w)]

    for i in range(WIN):
        pos[i] = row(chosen[i], cand[i], 0)
    typ[1:] = row(type_chosen, type_cand, 1)
    return pos, typ


# ---- rule 3 -----------------------------------------------------------------------------------------------------------------------

def region_limits(orfs, regions, off) -> np.ndarray:
    """limit_i of every record (-1: none); ValueError naming the first record whose region does not fit it."""
    if len(orfs) < len(regions):
        raise ValueError("the ORF set is shorter than the region set")
    lim = np.full(len(orfs), -1, dtype=np.int32)
    for i, r in enumerate(regions):
        o = orfs[i]
        L = int(off[int(o["seq"]) + 1] - off[int(o["seq"])])
        if r["seq"] != o["seq"] or r["strand"] != o["strand"]:
            raise ValueError("record %d" % i)
        xa = int(r["left"]) if not r["strand"] else L - 1 - int(r["right"])
        xs = int(o["left"]) if not o["strand"] else L - 1 - int(o["right"])
        lim[i] = -((xs - xa) // 3)             # ceil((xa - xs) / 3)
        if lim[i] < 0:
            raise ValueError("record %d" % i)
    return lim


# ---- the candidates of one record -----------------------------------------------------------------------------------------------------

def _cap(o, limit, min_res):
    return int(limit) if limit is not None and int(limit) >= 0 else int(o["n_res"]) - min_res


def candidates_loops(o, seq, off, T, K, start_codons):
    """Rules 2, 4 and 5 with plain loops -> [(k, Suf(k), the 20 window codes, type)] in increasing k."""
    sb = cm._bytes(seq)
    s = int(o["seq"])
    contig = sb[int(off[s]):int(off[s + 1])]
    L = len(contig)
    text = cm._strand(contig, int(o["strand"]))
    xs = int(o["left"]) if not o["strand"] else L - 1 - int(o["right"])
    n = int(o["n_res"])
    hexes = cm.pairs_loops(o, sb, off)
    out = []
    for k in range(n):
        typ = _TYPES.get(tuple(text[xs + 3 * k:xs + 3 * k + 3]), 0)
        is_start = typ != 0 and (start_codons >> (typ - 1)) & 1
        if not (k == 0 or (is_start and k <= K)):
            continue
        suf = 0
        for j in range(k, n - 1):
            if hexes[j] >= 0:
                suf += int(T[hexes[j]])
        win = []
        for i in range(WIN):
            x = xs + 3 * k - WIN + i
            win.append(text[x] if 0 <= x < L else 4)
        out.append((k, suf, win, typ))
    return out


def candidates_np(o, sb, off, T, K, start_codons, cache=None):
    """The same in numpy -> (k int64[c], suf int64[c], win int64[c][20], type int64[c]).  cache: a dict that keeps the strands'
    codes from one record to the next."""
    s, n = int(o["seq"]), int(o["n_res"])
    a, L = int(off[s]), int(off[s + 1] - off[s])
    key = (s, int(o["strand"]))
    code = None if cache is None else cache.get(key)
    if code is None:
        code = cm._CODE[sb[a:a + L]]
        if o["strand"]:
            code = np.where(code < 4, 3 - code, 4)[::-1]
        if cache is not None:
            cache[key] = code
    xs = int(o["left"]) if not o["strand"] else L - 1 - int(o["right"])
    t = code[xs:xs + 3 * n].reshape(n, 3)
    typ = np.where((t[:, 1] == 3) & (t[:, 2] == 2), np.select([t[:, 0] == 0, t[:, 0] == 2, t[:, 0] == 3], [1, 2, 3], 0), 0)
    is_start = (typ != 0) & (((start_codons >> np.maximum(typ - 1, 0)) & 1) != 0)
    ks = np.arange(n)
    k = ks[(ks == 0) | (is_start & (ks <= K))]
    h = cm.pairs_np(o, sb, off)
    v = np.where(h >= 0, np.asarray(T, dtype=np.int64)[np.maximum(h, 0)], 0)
    suf_all = np.concatenate([np.cumsum(v[::-1])[::-1], [0]]) if n > 1 else np.zeros(n, np.int64)
    at = (xs + 3 * k - WIN)[:, None] + np.arange(WIN)[None, :]
    win = np.where(at >= 0, code[np.maximum(at, 0)], 4)
    return k.astype(np.int64), suf_all[k].astype(np.int64), win, typ[k].astype(np.int64)


# ---- the whole call -------------------------------------------------------------------------------------------------------------------

def starts(orfs, seq, off, T, weights=None, limits=None, min_res: int = 100, start_codons: int = 7, rounds: int = 4,
           min_train_starts: int = 200, prot_start=None, residues=None, scores=None, loops: bool = False):
    """kg_orfset_starts / kg_starts_orfs -> a dict: orfs, shifts, stats (without the times), model (the last round's counts), and
    when given the old ones, prot_start, residues and scores under rule 9."""
    orfs = np.asarray(orfs, dtype=ORF_DTYPE)
    sb = cm._bytes(seq)
    n = len(orfs)
    movable = [i for i in range(n) if is_movable(orfs[i])]
    train = np.array([is_training(o) for o in orfs], dtype=bool) if n else np.zeros(0, bool)
    st = {"movable": len(movable), "training_records": int(train.sum()), "candidates": 0, "moved": 0, "rounds_run": 0,
          "trained": 2 if weights is not None else 1 if int(train.sum()) >= min_train_starts else 0}
    shifts = np.zeros(n, dtype=np.int32)
    model = zero_model()
    new_type, new_suf = {}, {}
    if st["trained"]:
        rec, k, suf, win, typ, cache = [], [], [], [], [], {}
        for i in movable:
            o = orfs[i]
            K = _cap(o, None if limits is None else limits[i], min_res)
            if loops:
                cs = candidates_loops(o, sb, off, T, K, start_codons)
                ck, cs_, cw, ct = ([c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs])
            else:
                ck, cs_, cw, ct = candidates_np(o, sb, off, T, K, start_codons, cache)
            rec += [i] * len(ck)
            k += list(ck); suf += [int(x) for x in cs_]; win += [list(w) for w in cw]; typ += list(ct)
        rec, k, typ = np.array(rec, np.int64), np.array(k, np.int64), np.array(typ, np.int64)
        suf = np.array(suf, dtype=np.int64)
        win = np.array(win, dtype=np.int64).reshape(len(rec), WIN)
        st["candidates"] = len(rec)
        cur = np.zeros(n, dtype=np.int64)
        R = 1 if weights is not None else rounds
        for _ in range(R):
            if weights is None:
                model = zero_model()
                for which, mask in ((1, train[rec]), (0, train[rec] & (k == cur[rec]))):
                    for i in range(WIN):
                        model[which][i] = np.bincount(win[mask, i], minlength=5)[:4]
                    model[2 + which][:] = np.bincount(typ[mask], minlength=4)
                    model[2 + which][0] = 0
                pos, wt = weights_from(*model)
            else:
                pos, wt = np.asarray(weights[0], np.int64), np.asarray(weights[1], np.int64)
            if loops:
                score = []
                for q in range(len(rec)):
                    sc = int(suf[q]) + int(wt[typ[q]])
                    for i in range(WIN):
                        if win[q, i] < 4:
                            sc += int(pos[i][win[q, i]])
                    score.append(sc)
                best = {}
                for q in range(len(rec)):           # the largest score, on a tie the smallest k
                    i = int(rec[q])
                    if i not in best or score[q] > best[i][0] or (score[q] == best[i][0] and k[q] < best[i][1]):
                        best[i] = (score[q], int(k[q]), q)
                chosen_q = {i: b[2] for i, b in best.items()}
            else:
                wp = np.zeros((WIN, 5), np.int64)
                wp[:, :4] = pos
                score = suf + wp[np.arange(WIN)[None, :], win].sum(axis=1) + np.asarray(wt, np.int64)[typ]
                order = np.lexsort((k, -score, rec))
                first = np.ones(len(order), bool)
                first[1:] = rec[order][1:] != rec[order][:-1]
                chosen_q = {int(rec[q]): int(q) for q in order[first]}
            for i, q in chosen_q.items():
                cur[i] = k[q]
                new_type[i], new_suf[i] = int(typ[q]), int(suf[q])
        st["rounds_run"] = R
        shifts = cur.astype(np.int32)
    out = orfs.copy()
    for i in np.flatnonzero(shifts):
        kk = int(shifts[i])
        if out[i]["strand"] == 0:
            out[i]["left"] += 3 * kk
        else:
            out[i]["right"] -= 3 * kk
        out[i]["n_res"] -= kk
        out[i]["start_codon"] = new_type[int(i)]
        out[i]["flags"] |= MOVED
    st["moved"] = int((shifts > 0).sum())
    res = {"orfs": out, "shifts": shifts, "stats": st, "model": model}
    if prot_start is not None:
        lens = np.diff(np.asarray(prot_start, dtype=np.int64))
        parts = []
        for i in range(n):
            p = np.array(residues[int(prot_start[i]):int(prot_start[i + 1])], dtype=np.uint8, copy=True)
            if shifts[i] > 0:
                p = p[int(shifts[i]):]
                p[0] = ord("M")
            parts.append(p)
        new_lens = np.array([len(p) for p in parts], dtype=np.int64)
        assert (new_lens == lens - np.minimum(shifts, lens)).all()
        res["prot_start"] = np.concatenate([[0], np.cumsum(new_lens)]).astype(np.int64)
        res["residues"] = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    if scores is not None:
        sc = np.array(scores, dtype=np.int64, copy=True)
        for i in np.flatnonzero(shifts):
            sc[i] = new_suf[int(i)]
        res["scores"] = sc
    return res


# ---- test inputs ----------------------------------------------------------------------------------------------------------------------

def random_batch(rng, n_seqs: int, max_len: int = 90, max_orfs: int = 5, p_start: float = 0.5):
    """coding_model.random_batch with start codons given to most records and sown into the contigs, so that records are movable
    and have candidates.  -> (records, bytes, offsets)."""
    orfs, seq, off = cm.random_batch(rng, n_seqs, max_len=max_len, max_orfs=max_orfs)
    seq = seq.copy()
    for spell in (b"ATG", b"GTG", b"TTG", b"atg", b"uTG", b"CAT", b"CAC", b"CAA"):
        for _ in range(int(len(seq) * p_start / 24)):
            at = int(rng.integers(0, max(len(seq) - 2, 1)))
            if at + 3 <= len(seq):
                seq[at:at + 3] = np.frombuffer(spell, np.uint8)
    for i in range(len(orfs)):
        if rng.random() < 0.85:
            orfs[i]["start_codon"] = int(rng.integers(1, 4))
        if rng.random() < 0.1:
            orfs[i]["flags"] |= NONCODING
    return orfs, seq, off
