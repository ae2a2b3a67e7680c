"""The frameshift-repair rule of kg_regionset_repair (include/kmerguts_hip.h) restated twice: `repair` finds every region's CALLs
through the group-order sort and answers the stop and start questions from prefix maxima and suffix minima in numpy;
`brute_force` finds them by containment and walks a materialised strand with plain loops.  The GPU tests compare the device's
bytes against `repair`.  Imports nothing from kmergutsjava_amd but the record dtypes."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd._native import CALL_DTYPE, JUNCTION_DTYPE, ORF_DTYPE, REGION_DTYPE

from orfs_model import _CODE, _LETTER, GENETIC_CODE, STARTS, STOPS, _codons, strand_codes

HAS_STOP, PARTIAL5, INTERRUPTED, MULTI_FRAME, REPAIRED = 1, 2, 4, 8, 128
STAT_KEYS = ("candidates", "repaired", "failed", "single", "skipped", "junctions", "residues")


def _inputs(regs, orfs, prot_start, residues, calls, seq, offsets):
    sb = np.frombuffer(seq, dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq.view(np.uint8).reshape(-1)
    return (np.asarray(regs, dtype=REGION_DTYPE), np.asarray(orfs, dtype=ORF_DTYPE), np.asarray(prot_start, dtype=np.int64),
            np.asarray(residues, dtype=np.uint8), np.asarray(calls, dtype=CALL_DTYPE), sb, np.asarray(offsets, dtype=np.int64))


def _is_candidate(r) -> bool:
    fr = int(r["frames"])
    return bool(r["kept"]) and (fr & (fr - 1)) != 0


def _segments(items, min_count):
    """items: (x0, index, x1, frame, count) in group order -> [[f, A, C], ...] (rule 2)."""
    segs = []
    for x0, _, x1, f, cnt in items:
        if cnt < min_count:
            continue
        if segs and segs[-1][0] == f:
            segs[-1][2] = max(segs[-1][2], x1)
        else:
            segs.append([f, x0, x1])
    return segs


def _finish(out, prots, junc, stats):
    lens = np.array([len(p) for p in prots], dtype=np.int64)
    start = np.zeros(len(prots) + 1, dtype=np.int64)
    np.cumsum(lens, out=start[1:])
    res = np.concatenate(prots).astype(np.uint8) if len(prots) else np.zeros(0, np.uint8)
    j = np.zeros(len(junc), dtype=JUNCTION_DTYPE)
    for k, rec in enumerate(junc):
        j[k] = rec
    jstart = np.searchsorted(j["orf"], np.arange(len(prots) + 1), side="left").astype(np.int64)
    stats["junctions"] = len(junc)
    return out, start, res, j, jstart, stats


def _apply(out, prots, junc, stats, i, r, L, segs, J, b, sc, u, e, nfm, parts, protein):
    """Rules 6 and 7 for a chain that holds: parts = [(first codon, length)] per segment, protein = its bytes."""
    f1, fm = segs[0][0], segs[-1][0]
    last = e if e < nfm else nfm - 1
    xs, xe = f1 + 3 * b, fm + 3 * last + 2
    left, right = (xs, xe) if not r["strand"] else (L - 1 - xe, L - 1 - xs)
    n_res = sum(n for _, n in parts)
    star = np.flatnonzero(protein == ord("*"))
    flags = (HAS_STOP if e < nfm else 0) | (PARTIAL5 if u == -1 else 0) | INTERRUPTED | MULTI_FRAME | REPAIRED
    out[i] = (r["seq"], r["strand"], f1, left, right, n_res, sc, int(star[0]) if star.size else -1, flags, r["fI"], r["score"], r["kept"])
    prots[i] = protein
    at = 0
    for k in range(len(segs) - 1):
        at += parts[k][1]
        junc.append((i, J[k] if not r["strand"] else L - 1 - J[k], segs[k][0], segs[k + 1][0], at, segs[k + 1][1] - segs[k][2] - 1))
    stats["repaired"] += 1
    stats["residues"] += n_res
    assert 3 * n_res <= right - left + 1


def repair(regs, orfs, prot_start, residues, calls, seq, offsets, start_codons: int = 7, min_count: int = 0, max_junctions: int = 4):
    """-> (ORF_DTYPE records, prot_start int64[n + 1], residues uint8, JUNCTION_DTYPE records, junction_start int64[n + 1], stats)."""
    regs, orfs, ps, res, calls, sb, off = _inputs(regs, orfs, prot_start, residues, calls, seq, offsets)
    n = calls.size
    out = orfs.copy()
    prots = [res[ps[i]:ps[i + 1]] for i in range(orfs.size)]
    junc, stats = [], dict.fromkeys(STAT_KEYS, 0)
    # the group order of the region stage, and where every CALL of calls[] stands in it
    cont = calls["container"].astype(np.int64)
    cseq, ck = cont // 6, cont % 6
    cstrand, cframe = (ck >= 3).astype(np.int64), ck % 3
    x0 = cframe + 3 * calls["start"].astype(np.int64)
    x1 = cframe + 3 * calls["end"].astype(np.int64) + 2
    order = np.lexsort((np.arange(n), x0, calls["fI"].astype(np.int64), cstrand, cseq))
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    sx0, sx1, sfr, scnt = x0[order], x1[order], cframe[order], calls["count"].astype(np.int64)[order]
    starts = [c for k, c in enumerate(STARTS) if start_codons >> k & 1]
    cache = {}

    def frame_arrays(s, strand, f):
        key = (s, strand, f)
        if key not in cache:
            cod = _codons(strand_codes(sb[off[s]:off[s + 1]], strand), f)
            nf = cod.size
            idx = np.arange(nf, dtype=np.int64)
            is_stop = np.isin(cod, STOPS)
            is_start = np.isin(cod, starts) if starts else np.zeros(nf, bool)
            cache[key] = (cod, np.maximum.accumulate(np.where(is_stop, idx, -1)),               # the largest stop <= j
                          np.minimum.accumulate(np.where(is_stop, idx, nf)[::-1])[::-1],        # the smallest stop >= j
                          np.minimum.accumulate(np.where(is_start, idx, nf)[::-1])[::-1])
        return cache[key]

    for i, r in enumerate(regs):
        if not _is_candidate(r):
            continue
        stats["candidates"] += 1
        s, strand = int(r["seq"]), int(r["strand"])
        L = int(off[s + 1] - off[s])
        p0 = int(pos[r["first_call"]])
        sl = slice(p0, p0 + int(r["n_calls"]))
        segs = _segments(zip(sx0[sl].tolist(), range(p0, p0 + int(r["n_calls"])), sx1[sl].tolist(), sfr[sl].tolist(), scnt[sl].tolist()),
                         min_count)
        if len(segs) <= 1:
            stats["single"] += 1
            continue
        if len(segs) > max_junctions + 1:
            stats["skipped"] += 1
            continue
        J, ok = [], True
        for k in range(len(segs) - 1):
            (p, _, C), (q, A, _) = segs[k], segs[k + 1]
            _, _, next_stop_p, _ = frame_arrays(s, strand, p)
            _, last_stop_q, _, _ = frame_arrays(s, strand, q)
            lp, gq = (C - 2 - p) // 3, (A - q) // 3
            tp = int(next_stop_p[lp + 1]) if lp + 1 < next_stop_p.size else next_stop_p.size
            sq = int(last_stop_q[gq - 1]) if gq > 0 else -1
            hi, lo, mid = p + 3 * tp, q + 3 * (sq + 1), (C + 1 + A) // 2
            if lo > hi:
                ok = False
                break
            J.append(min(max(mid, lo), hi))
        if ok and any(J[k] >= J[k + 1] for k in range(len(J) - 1)):
            ok = False
        if ok:
            f1, A1, _ = segs[0]
            fm, _, Cm = segs[-1]
            cod1, last_stop, _, next_start = frame_arrays(s, strand, f1)
            codm, _, next_stop, _ = frame_arrays(s, strand, fm)
            j0 = (A1 - f1) // 3
            u = int(last_stop[j0 - 1]) if j0 > 0 else -1
            st = int(next_start[u + 1])
            b = st if st <= j0 else u + 1
            sc = STARTS.index(int(cod1[b])) + 1 if st <= j0 else 0
            jl, nfm = (Cm - 2 - fm) // 3, codm.size
            e = int(next_stop[jl + 1]) if jl + 1 < nfm else nfm
            parts = []
            for k, (f, _, _) in enumerate(segs):
                jf = b if k == 0 else -((f - J[k - 1]) // 3)             # ceil((J - f) / 3)
                je = min(e, nfm) if k == len(segs) - 1 else (J[k] - f) // 3
                parts.append((jf, je - jf))
            ok = all(n > 0 for _, n in parts)
        if not ok:
            stats["failed"] += 1
            continue
        pieces = []
        for (f, _, _), (jf, cnt) in zip(segs, parts):
            c = frame_arrays(s, strand, f)[0][jf:jf + cnt]
            pieces.append(np.where(c >= 0, _LETTER[np.maximum(c, 0)], ord("X")).astype(np.uint8))
        protein = np.concatenate(pieces)
        if sc:
            protein[0] = ord("M")
        _apply(out, prots, junc, stats, i, r, L, segs, J, b, sc, u, e, nfm, parts, protein)
    return _finish(out, prots, junc, stats)


def brute_force(regs, orfs, prot_start, residues, calls, seq, offsets, start_codons: int = 7, min_count: int = 0, max_junctions: int = 4):
    """The same rule with plain loops over a materialised strand; a region's CALLs are those of its group that lie inside it."""
    regs, orfs, ps, res, calls, sb, off = _inputs(regs, orfs, prot_start, residues, calls, seq, offsets)
    out = orfs.copy()
    prots = [res[ps[i]:ps[i + 1]] for i in range(orfs.size)]
    junc, stats = [], dict.fromkeys(STAT_KEYS, 0)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    names = {"ATG": 1, "GTG": 2, "TTG": 3}
    for i, r in enumerate(regs):
        if not _is_candidate(r):
            continue
        stats["candidates"] += 1
        s, strand = int(r["seq"]), int(r["strand"])
        L = int(off[s + 1] - off[s])
        xa, xb = (int(r["left"]), int(r["right"])) if not strand else (L - 1 - int(r["right"]), L - 1 - int(r["left"]))
        items = []
        for idx, c in enumerate(calls):
            k = int(c["container"]) % 6
            if int(c["container"]) // 6 != s or k // 3 != strand or int(c["fI"]) != int(r["fI"]):
                continue
            f = k % 3
            a, z = f + 3 * int(c["start"]), f + 3 * int(c["end"]) + 2
            if xa <= a and z <= xb:
                items.append((a, idx, z, f, int(c["count"])))
        items.sort()
        segs = _segments(items, min_count)
        if len(segs) <= 1:
            stats["single"] += 1
            continue
        if len(segs) > max_junctions + 1:
            stats["skipped"] += 1
            continue
        text = "".join("ACGTN"[_CODE[ch]] for ch in sb[off[s]:off[s + 1]])
        if strand:
            text = "".join(comp[ch] for ch in reversed(text))

        def nf(f):
            return (L - f) // 3 if L >= f else 0

        def codon(f, j):
            return text[f + 3 * j:f + 3 * j + 3]

        def stop(f, j):
            return codon(f, j) in ("TAA", "TAG", "TGA")

        def start(f, j):
            return codon(f, j) in names and (start_codons >> (names[codon(f, j)] - 1)) & 1

        J, ok = [], True
        for k in range(len(segs) - 1):
            (p, _, C), (q, A, _) = segs[k], segs[k + 1]
            tp = (C - 2 - p) // 3 + 1
            while tp < nf(p) and not stop(p, tp):
                tp += 1
            sq = (A - q) // 3 - 1
            while sq >= 0 and not stop(q, sq):
                sq -= 1
            hi, lo, mid = p + 3 * tp, q + 3 * (sq + 1), (C + 1 + A) // 2
            if lo > hi:
                ok = False
                break
            J.append(min(max(mid, lo), hi))
        for k in range(len(J) - 1):
            if ok and J[k] >= J[k + 1]:
                ok = False
        if not ok:
            stats["failed"] += 1
            continue
        f1, A1, _ = segs[0]
        fm, _, Cm = segs[-1]
        j0 = (A1 - f1) // 3
        u = j0 - 1
        while u >= 0 and not stop(f1, u):
            u -= 1
        b = u + 1
        while b <= j0 and not start(f1, b):
            b += 1
        sc = names[codon(f1, b)] if b <= j0 else 0
        if b > j0:
            b = u + 1
        e = (Cm - 2 - fm) // 3 + 1
        while e < nf(fm) and not stop(fm, e):
            e += 1
        parts, letters = [], []
        for k, (f, _, _) in enumerate(segs):
            js = []
            for j in range(nf(f)):
                x = f + 3 * j
                if k == 0:
                    inside = j >= b and x + 3 <= J[0]
                elif k == len(segs) - 1:
                    inside = x >= J[-1] and j < min(e, nf(f))
                else:
                    inside = J[k - 1] <= x and x + 3 <= J[k]
                if inside:
                    js.append(j)
            parts.append((js[0] if js else 0, len(js)))
            for j in js:
                c = codon(f, j)
                letters.append("X" if "N" in c else GENETIC_CODE["ACGT".index(c[0]) * 16 + "ACGT".index(c[1]) * 4 + "ACGT".index(c[2])])
        if any(n == 0 for _, n in parts):
            stats["failed"] += 1
            continue
        if sc:
            letters[0] = "M"
        protein = np.frombuffer("".join(letters).encode(), dtype=np.uint8).copy()
        _apply(out, prots, junc, stats, i, r, L, segs, J, b, sc, u, e, nf(fm), parts, protein)
    return _finish(out, prots, junc, stats)


def random_case(rng, n_seqs: int = 4, max_len: int = 300, n_fn: int = 2, p_stop: float = 0.02):
    """Random contigs (lengths 0..30 among longer ones; N, u and lower case) with few stops, and CALL lists made for chains:
    runs of CALLs that change frame 1 to 5 times, some overlapping, some nested, counts 0..6.  -> (calls, seq, offsets)."""
    lens = np.where(rng.random(n_seqs) < 0.3, rng.integers(0, 31, size=n_seqs), rng.integers(60, max_len + 1, size=n_seqs))
    off = np.zeros(n_seqs + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    alphabet = np.frombuffer(b"ACGTacgtuN", dtype=np.uint8)
    w = np.array([1, 1, 1, 1, .05, .05, .05, .05, .05, .03])
    seq = rng.choice(alphabet, size=int(off[-1]), p=w / w.sum()).astype(np.uint8)
    # thin the stops out so that chains have room: a T that would open TAA / TAG / TGA becomes C most of the time
    up = np.char.upper(seq.view("S1")).view(np.uint8)
    for x in range(seq.size - 2):
        if up[x] in (84, 85) and ((up[x + 1] == 65 and up[x + 2] in (65, 71)) or (up[x + 1] == 71 and up[x + 2] == 65)) and rng.random() > p_stop * 10:
            seq[x] = up[x] = 67
    rows = []
    for s in range(n_seqs):
        L = int(lens[s])
        for _ in range(int(rng.integers(0, 4))):
            strand, fi = int(rng.integers(0, 2)), int(rng.integers(0, n_fn))
            f = int(rng.integers(0, 3))
            at = int(rng.integers(0, max(1, L // 2)))
            for _ in range(int(rng.integers(1, 9))):
                res = (L - f) // 3 if L >= f else 0
                a = (at - f + 2) // 3
                if a < 0 or a >= res:
                    break
                z = min(res - 1, a + int(rng.integers(0, 14)))
                rows.append((6 * s + 3 * strand + f, a, z, int(rng.integers(0, 7)), fi, 1.0))
                at = f + 3 * z + 2 + int(rng.integers(-12, 20))
                if rng.random() < 0.6:
                    f = (f + int(rng.integers(1, 3))) % 3
    rows.sort(key=lambda r: r[0])
    calls = np.zeros(len(rows), dtype=CALL_DTYPE)
    for i, r in enumerate(rows):
        calls[i] = r
    return calls, seq, off
