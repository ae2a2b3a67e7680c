"""The masking rule of kg_proteins_mask (include/kmerguts_hip.h) restated twice: as plain loops, one window at a time, and with
numpy on whole arrays; and the masked search and cluster models, which run search_model / cluster_model's shared-k-mer counts
over the soft-masked bytes and the alignment over the original.  The GPU tests compare the device's bytes with the numpy form;
the CPU tests compare the two forms with each other and with the known answers below."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd import _native as N

import cluster_model as CM
import search_model as SM
import seed_model as SD

ALPHA = b"ACDEFGHIKLMNPQRSTVWY"
WINDOW, TRIGGER, EXTEND = 12, 563, 640
COUNTS = ("proteins", "residues", "windows", "low_windows", "ext_windows", "masking_windows", "segments", "masked_residues",
          "proteins_masked")
# known answers (the header's): Lg(1..12), W * Lg(W) for W = 12, and D of three windows
LG_1_TO_12 = (0, 256, 405, 512, 594, 661, 718, 768, 811, 850, 885, 917)
FULL_12 = 11004
KAT_D = {b"QEQEQEQEQEQE": 3072, b"ACDEFGHIKLMN": 11004, b"QQQQQQQQQQQQ": 0}
LOW_MAX_DEFAULT, EXT_MAX_DEFAULT = 6756, 7680          # 12 * 563 and 12 * 640

_LUT = np.full(256, 20, dtype=np.int64)
_LUT[np.frombuffer(ALPHA, dtype=np.uint8)] = np.arange(20)


def lg(x: int) -> int:
    """The header's Lg (rule 5 of the coding section), restated here."""
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


def deficit(window: bytes) -> int:
    """D of one window: W * Lg(W) minus the sum of n_a * Lg(n_a) over its letters 0..20."""
    count = {}
    for ch in window:
        a = ALPHA.find(bytes([ch]))
        a = 20 if a < 0 else a
        count[a] = count.get(a, 0) + 1
    return len(window) * lg(len(window)) - sum(n * lg(n) for n in count.values())


def check_params(window: int, trigger: int, extend: int) -> None:
    assert 4 <= window <= 32 and 0 <= trigger <= extend < lg(window), (window, trigger, extend)


def _result(n, flags_per, segs, counts):
    seg_start = np.zeros(n + 1, dtype=np.int64)
    rec = np.zeros(len(segs), dtype=N.MASK_SEGMENT_DTYPE)
    for k, (p, a, b) in enumerate(segs):
        rec[k] = (p, a, b, 0)
        seg_start[p + 1] += 1
    seg_start = np.cumsum(seg_start)
    flags = np.concatenate(flags_per) if flags_per else np.zeros(0, dtype=np.uint8)
    counts.update(proteins=n, residues=int(flags.size), segments=len(segs), masked_residues=int(flags.sum()),
                  proteins_masked=len({p for p, _, _ in segs}))
    return flags.astype(np.uint8), rec, seg_start, {k: int(counts[k]) for k in COUNTS}


def mask_loops(seq: bytes, offsets, window: int = WINDOW, trigger: int = TRIGGER, extend: int = EXTEND):
    """The header's words, one window at a time.  -> (flags uint8[residues], MASK_SEGMENT_DTYPE records, seg_start, counts)."""
    check_params(window, trigger, extend)
    seq = bytes(seq)
    n = len(offsets) - 1
    W = window
    counts = dict(windows=0, low_windows=0, ext_windows=0, masking_windows=0)
    flags_per, segs = [], []
    for p in range(n):
        s = seq[offsets[p]:offsets[p + 1]]
        nwin = max(len(s) - W + 1, 0)
        D = [deficit(s[i:i + W]) for i in range(nwin)]
        low = [d <= W * trigger for d in D]
        ext = [d <= W * extend for d in D]
        masking = [False] * nwin
        i = 0
        while i < nwin:
            if not ext[i]:
                i += 1
                continue
            j = i
            while j < nwin and ext[j]:
                j += 1
            if any(low[i:j]):
                for k in range(i, j):
                    masking[k] = True
            i = j
        f = np.zeros(len(s), dtype=np.uint8)
        for i in range(nwin):
            if masking[i]:
                f[i:i + W] = 1
        j = 0
        while j < len(s):
            if not f[j]:
                j += 1
                continue
            k = j
            while k + 1 < len(s) and f[k + 1]:
                k += 1
            segs.append((p, j, k))
            j = k + 1
        counts["windows"] += nwin
        counts["low_windows"] += sum(low)
        counts["ext_windows"] += sum(ext)
        counts["masking_windows"] += sum(masking)
        flags_per.append(f)
    return _result(n, flags_per, segs, counts)


def mask_numpy(seq, offsets, window: int = WINDOW, trigger: int = TRIGGER, extend: int = EXTEND):
    """The same with whole arrays, protein by protein."""
    check_params(window, trigger, extend)
    arr = np.frombuffer(bytes(seq), dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq.view(np.uint8).reshape(-1)
    off = np.asarray(offsets, dtype=np.int64)
    n = off.size - 1
    W = window
    nlg = np.array([0] + [k * lg(k) for k in range(1, W + 1)], dtype=np.int64)
    full = W * lg(W)
    counts = dict(windows=0, low_windows=0, ext_windows=0, masking_windows=0)
    flags_per, segs = [], []
    for p in range(n):
        c = _LUT[arr[off[p]:off[p + 1]]]
        L = c.size
        f = np.zeros(L, dtype=np.uint8)
        nwin = max(L - W + 1, 0)
        if nwin:
            onehot = np.zeros((L + 1, 21), dtype=np.int64)
            onehot[np.arange(1, L + 1), c] = 1
            cs = np.cumsum(onehot, axis=0)
            D = full - nlg[cs[W:] - cs[:-W]].sum(axis=1)
            low, ext = D <= W * trigger, D <= W * extend
            head = ext & ~np.r_[False, ext[:-1]]                        # the first window of every ext run
            run = np.cumsum(head) - 1                                   # the run of every ext window
            has_low = np.bincount(run[low], minlength=int(head.sum())) > 0 if head.any() else np.zeros(0, dtype=bool)
            masking = np.zeros(nwin, dtype=bool)
            masking[ext] = has_low[run[ext]]
            step = np.zeros(L + 1, dtype=np.int64)
            at = np.flatnonzero(masking)
            np.add.at(step, at, 1)
            np.add.at(step, at + W, -1)
            f = (np.cumsum(step)[:L] > 0).astype(np.uint8)
            edge = np.diff(np.r_[0, f.astype(np.int64), 0])
            for a, b in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1) - 1):
                segs.append((p, int(a), int(b)))
            counts["windows"] += nwin
            counts["low_windows"] += int(low.sum())
            counts["ext_windows"] += int(ext.sum())
            counts["masking_windows"] += int(masking.sum())
        flags_per.append(f)
    return _result(n, flags_per, segs, counts)


def soft_mask(seq: bytes, offsets, flags, first: int = 0, last=None) -> bytes:
    """The seeding copy: the masked residues of proteins [first, last) with 0x20 set (a letter in lowercase), every other byte as
    it is.  flags: one byte per residue of the whole batch."""
    off = np.asarray(offsets, dtype=np.int64)
    last = off.size - 1 if last is None else last
    out = np.frombuffer(bytes(seq), dtype=np.uint8).copy()
    lo, hi = int(off[first]), int(off[last])
    body = out[int(off[0]):int(off[-1])]
    on = np.asarray(flags, dtype=bool).copy()
    on[:lo - int(off[0])] = False
    on[hi - int(off[0]):] = False
    body[on] |= 0x20
    return out.tobytes()


def side_range(sides: str, n_db: int, n: int):
    """The proteins [first, last) a search masks: the targets are [0, n_db), the queries [n_db, n)."""
    return {"both": (0, n), "queries": (n_db, n), "targets": (0, n_db)}[sides]


def masked_search_model(seq: bytes, offsets, n_db: int, window: int = WINDOW, trigger: int = TRIGGER, extend: int = EXTEND,
                        sides: str = "both", seed=None, **kw):
    """kg_proteins_search_masked: the shared counts of search_model (seed: of seed_model) over the soft-masked bytes, everything
    behind them over the original.  -> (records, hit_start, counts, the mask's counts of the masked side)."""
    off = np.asarray(offsets, dtype=np.int64)
    n = off.size - 1
    first, last = side_range(sides, n_db, n)
    flags, _, _, _ = mask_numpy(seq, off, window, trigger, extend)
    _, _, _, mcounts = mask_numpy(seq, off[first:last + 1], window, trigger, extend)
    soft = soft_mask(seq, off, flags, first, last)
    inner = SM.shared_numpy if seed is None else SD.shared_numpy(seed)

    def shared(_seq, offsets_, n_db_, max_db_per_kmer=SM.MAX_DB_PER_KMER):
        return inner(soft, offsets_, n_db_, max_db_per_kmer)

    hits, start, counts = SM.search_model(seq, off, n_db, shared=shared, **kw)
    return hits, start, counts, mcounts


def masked_cluster_model(seq: bytes, offsets, window: int = WINDOW, trigger: int = TRIGGER, extend: int = EXTEND, **kw):
    """kg_proteins_cluster_masked without alignment: cluster_model over the soft-masked bytes.  -> (records, counts, mask counts)."""
    flags, _, _, mcounts = mask_numpy(seq, offsets, window, trigger, extend)
    rec, counts = CM.cluster_numpy(soft_mask(seq, offsets, flags), offsets, **kw)
    return rec, counts, mcounts


# ---- inputs the tests share ---------------------------------------------------------------------------------------------------

INSERT = b"QE" * 8 + b"Q" * 10          # the planted low-complexity insert: 26 residues


def random_protein(rng, length: int) -> bytes:
    return np.frombuffer(ALPHA, dtype=np.uint8)[rng.integers(0, 20, size=length)].tobytes()


def with_insert(rng, p: bytes, insert: bytes = INSERT) -> bytes:
    at = int(rng.integers(0, len(p) + 1))
    return p[:at] + insert + p[at:]


def mutate(rng, p: bytes, rate: float) -> bytes:
    a = np.frombuffer(p, dtype=np.uint8).copy()
    hit = np.flatnonzero(rng.random(a.size) < rate)
    a[hit] = np.frombuffer(ALPHA, dtype=np.uint8)[rng.integers(0, 20, size=hit.size)]
    return a.tobytes()


def planted_search(seed: int = 1, n_targets: int = 24, n_related: int = 12, length: int = 150):
    """The issue's example: n_targets random targets with the insert at a random place; n_related queries that are 5 %-mutated
    copies of targets 0 .. n_related - 1 (insert and all) and n_related unrelated random queries with the same insert.
    -> (proteins, n_db)."""
    rng = np.random.default_rng(seed)
    targets = [with_insert(rng, random_protein(rng, length)) for _ in range(n_targets)]
    related = [mutate(rng, targets[k], 0.05) for k in range(n_related)]
    unrelated = [with_insert(rng, random_protein(rng, length)) for _ in range(n_related)]
    return targets + related + unrelated, n_targets


def low_complexity_batch(rng, n: int = 40):
    """Random proteins of many lengths with repeats, homopolymers, X and lowercase runs planted: most have a segment, some several."""
    out = []
    for _ in range(n):
        L = int(rng.integers(0, 260))
        p = bytearray(random_protein(rng, L))
        for _ in range(int(rng.integers(0, 4))):
            kind = int(rng.integers(0, 5))
            m = int(rng.integers(3, 40))
            unit = [random_protein(rng, 1), random_protein(rng, 2), random_protein(rng, 3), b"X", b"q"][kind]
            run = (unit * m)[:m]
            at = int(rng.integers(0, len(p) + 1))
            p[at:at] = run
        out.append(bytes(p))
    return out
