"""The signature semantics of kg_signatures_derive (include/kmerguts_hip.h) restated in torch: the exact reference the GPU
tests compare against, byte for byte.  Runs on whatever device the sequence tensor is on (CPU or GPU)."""
from __future__ import annotations

import numpy as np
import torch

from kmergutsjava_amd import _native as N

ALPHA = b"ACDEFGHIKLMNPQRSTVWY"
K = 8


def _lut(device):
    lut = torch.full((256,), 20, dtype=torch.uint8, device=device)
    lut[torch.tensor(list(ALPHA), dtype=torch.int64, device=device)] = torch.arange(20, dtype=torch.uint8, device=device)
    return lut


def _runs(key: torch.Tensor):
    """Runs of equal consecutive values: (run id of every item, first item of every run, length of every run)."""
    n = key.numel()
    head = torch.ones(n, dtype=torch.bool, device=key.device)
    if n > 1:
        head[1:] = key[1:] != key[:-1]
    rid = torch.cumsum(head.to(torch.int64), 0) - 1
    first = torch.nonzero(head).flatten()
    ends = torch.cat([first[1:], torch.tensor([n], dtype=torch.int64, device=key.device)])
    return rid, first, ends - first


def derive(seq, offsets, fn, otu, min_proteins: int = 2, purity_pct: int = 80) -> np.ndarray:
    """seq: uint8 tensor (any device) or bytes; offsets int64[n + 1]; fn / otu int[n].  Returns SIGNATURE_DTYPE records in
    ascending k-mer order."""
    if not torch.is_tensor(seq):
        seq = torch.from_numpy(np.frombuffer(bytes(seq), dtype=np.uint8).copy())
    dev = seq.device
    off = torch.as_tensor(np.asarray(offsets, dtype=np.int64), device=dev)
    fn = torch.as_tensor(np.asarray(fn, dtype=np.int64), device=dev)
    otu = torch.as_tensor(np.asarray(otu, dtype=np.int64), device=dev)
    n_prot = off.numel() - 1
    empty = np.zeros(0, dtype=N.SIGNATURE_DTYPE)
    if n_prot <= 0:
        return empty
    otu = torch.where(fn >= 0, otu, torch.zeros_like(otu))
    lens = off[1:] - off[:-1]
    nwin = torch.clamp(lens - K, min=0)                        # positions i in [0, len - 8) (KGJ:912)
    total = int(nwin.sum())
    if total == 0:
        return empty
    # protein rank by (fn, otu, p)
    rk = (fn + 1) * (1 << 31) + otu
    order = torch.sort(rk, stable=True).indices
    rank_of = torch.empty_like(order)
    rank_of[order] = torch.arange(n_prot, dtype=torch.int64, device=dev)
    fn_r, otu_r = fn[order], otu[order]
    # windows
    prot = torch.repeat_interleave(torch.arange(n_prot, device=dev), nwin)
    wstart = torch.cumsum(nwin, 0) - nwin
    i = torch.arange(total, dtype=torch.int64, device=dev) - wstart[prot]
    del wstart
    start = off[prot] + i
    codes = _lut(dev)[seq.to(dev).to(torch.int64)]
    v = torch.zeros(total, dtype=torch.int64, device=dev)
    bad = torch.zeros(total, dtype=torch.bool, device=dev)
    for k in range(K):
        c = codes[start + k]
        v = v * 20 + c.to(torch.int64)
        bad |= c >= 20
    del start, codes
    ok = ~bad
    v, prot, dist = v[ok], prot[ok], (lens[prot] - i)[ok]
    del ok, bad, i
    if v.numel() == 0:
        return empty
    # (k-mer, rank) pairs, keeping the largest len_p - i
    key = v * n_prot + rank_of[prot]
    del v, prot
    key, perm = torch.sort(key)
    dist = dist[perm]
    del perm
    rid, first, _ = _runs(key)
    pk = key[first]
    pv = torch.zeros(first.numel(), dtype=torch.int64, device=dev).scatter_reduce(0, rid, dist, "amax", include_self=False)
    del key, dist, rid, first
    pv_kmer, pr = pk // n_prot, pk % n_prot
    pf, po = fn_r[pr], otu_r[pr]
    # k-mer runs
    kid, kfirst, n_v = _runs(pv_kmer)
    nk = kfirst.numel()
    # (k-mer, fn) runs
    fkey = kid * (int(fn.max()) + 2) + (pf + 1)
    fid, ffirst, fcount = _runs(fkey)
    f_of = pf[ffirst]
    k_of = kid[ffirst]
    fsum = torch.zeros(ffirst.numel(), dtype=torch.int64, device=dev).index_add_(0, fid, pv)
    score = torch.where(f_of >= 0, fcount * (1 << 32) + ((1 << 31) - 1 - f_of), torch.zeros_like(fcount))
    kbest = torch.zeros(nk, dtype=torch.int64, device=dev).scatter_reduce(0, k_of, score, "amax", include_self=True)
    best_run = (f_of >= 0) & (score == kbest[k_of])
    # OTU mode inside the best (k-mer, fn) run
    okey = fid * (int(otu.max()) + 1) + po
    oid, ofirst, ocount = _runs(okey)
    o_frun = fid[ofirst]
    ok_best = best_run[o_frun]
    oscore = torch.where(ok_best, ocount * (1 << 32) + ((1 << 31) - 1 - po[ofirst]), torch.zeros_like(ocount))
    kotu = torch.zeros(nk, dtype=torch.int64, device=dev).scatter_reduce(0, kid[ofirst], oscore, "amax", include_self=True)
    # the best run's sum per k-mer
    ksum = torch.zeros(nk, dtype=torch.int64, device=dev).index_add_(0, k_of, torch.where(best_run, fsum, torch.zeros_like(fsum)))
    kfn = torch.full((nk,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, k_of, torch.where(best_run, f_of, torch.full_like(f_of, -1)),
                                                                             "amax", include_self=True)
    c = kbest >> 32
    sig = (kbest > 0) & (n_v >= min_proteins) & (100 * c >= purity_pct * n_v)
    sel = torch.nonzero(sig).flatten()
    out = np.zeros(sel.numel(), dtype=N.SIGNATURE_DTYPE)
    if sel.numel() == 0:
        return out
    cs = c[sel]
    out["kmer"] = pv_kmer[kfirst[sel]].cpu().numpy()
    out["otuIndex"] = ((1 << 31) - 1 - (kotu[sel] & 0xFFFFFFFF)).cpu().numpy()
    out["avgFromEnd"] = (ksum[sel] // cs).cpu().numpy()
    out["functionIndex"] = kfn[sel].cpu().numpy()
    out["functionWt"] = np.float32(cs.cpu().numpy()) / np.float32(n_v[sel].cpu().numpy())
    return out


def brute_force(seq: bytes, offsets, fn, otu, min_proteins: int = 2, purity_pct: int = 80) -> np.ndarray:
    """The same semantics with Python dicts, one window at a time (tiny inputs only)."""
    code = {ch: j for j, ch in enumerate(ALPHA)}
    first_pos = {}                                       # v -> {p: smallest i}
    for p in range(len(offsets) - 1):
        s = seq[offsets[p]:offsets[p + 1]]
        for i in range(0, len(s) - K):
            w = s[i:i + K]
            if any(ch not in code for ch in w):
                continue
            v = 0
            for ch in w:
                v = v * 20 + code[ch]
            first_pos.setdefault(v, {}).setdefault(p, i)
    rows = []
    for v in sorted(first_pos):
        P = first_pos[v]
        n = len(P)
        cf = {}
        for p in P:
            if fn[p] >= 0:
                cf[fn[p]] = cf.get(fn[p], 0) + 1
        if not cf or n < min_proteins:
            continue
        fstar = min(cf, key=lambda f: (-cf[f], f))
        c = cf[fstar]
        if 100 * c < purity_pct * n:
            continue
        members = [p for p in P if fn[p] == fstar]
        oc = {}
        for p in members:
            oc[otu[p]] = oc.get(otu[p], 0) + 1
        o = min(oc, key=lambda x: (-oc[x], x))
        total = sum((offsets[p + 1] - offsets[p]) - P[p] for p in members)
        rows.append((v, o, total // c, fstar, np.float32(c) / np.float32(n)))
    out = np.zeros(len(rows), dtype=N.SIGNATURE_DTYPE)
    for j, r in enumerate(rows):
        out[j] = r
    return out


def family_set(n_fam: int, per_fam: int, length: int, mut: float, seed: int, n_fn: int = 50, n_otu: int = 7,
               unannotated: float = 0.1):
    """Seeded protein families with point mutations: (seq bytes, offsets, fn, otu).  Members of one family mostly share the
    family's function; some are unannotated, some carry another function."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(ALPHA, dtype=np.uint8)
    seqs, fns, otus = [], [], []
    for f in range(n_fam):
        base = alpha[rng.integers(0, 20, size=length)]
        fam_fn = int(rng.integers(0, n_fn))
        for _ in range(per_fam):
            s = base.copy()
            m = rng.random(length) < mut
            s[m] = alpha[rng.integers(0, 20, size=int(m.sum()))]
            cut = int(rng.integers(0, max(1, length // 10)))
            s = s[cut:length - int(rng.integers(0, max(1, length // 10)))]
            seqs.append(s.tobytes())
            u = rng.random()
            fns.append(-1 if u < unannotated else (int(rng.integers(0, n_fn)) if u < unannotated + 0.1 else fam_fn))
            otus.append(int(rng.integers(0, n_otu)))
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return b"".join(seqs), offsets, np.array(fns, dtype=np.int32), np.array(otus, dtype=np.int32)


def family_device(n_prot: int, length: int, seed: int, device, per_fam: int = 8, mut: float = 0.03, n_fn: int = 5000,
                  n_otu: int = 64):
    """A seeded family training set generated on `device`: proteins of length - [0, length / 8) residues, per_fam to a
    family, point mutations at rate mut.  -> (uint8 sequence tensor, int64 offsets ndarray, int32 fn, int32 otu ndarrays)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    n_fam = (n_prot + per_fam - 1) // per_fam
    alpha = torch.tensor(list(ALPHA), dtype=torch.uint8, device=device)
    base = torch.randint(0, 20, (n_fam, length), generator=g, device=device, dtype=torch.uint8)
    lens = length - torch.randint(0, max(1, length // 8), (n_prot,), generator=g, device=device)
    parts = []
    step = max(1, (1 << 27) // length)
    for a in range(0, n_prot, step):
        b = min(n_prot, a + step)
        fam = torch.arange(a, b, device=device) // per_fam
        codes = base[fam]
        m = torch.rand((b - a, length), generator=g, device=device) < mut
        codes = torch.where(m, torch.randint(0, 20, (b - a, length), generator=g, device=device, dtype=torch.uint8), codes)
        keep = torch.arange(length, device=device)[None, :] < lens[a:b, None]
        parts.append(alpha[codes[keep].to(torch.int64)])
    seq = torch.cat(parts)
    offsets = np.zeros(n_prot + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(lens.cpu().numpy())
    rng = np.random.default_rng(seed)
    fn = ((np.arange(n_prot) // per_fam) % n_fn).astype(np.int32)
    u = rng.random(n_prot)
    fn[u < 0.1] = -1
    noisy = (u >= 0.1) & (u < 0.15)
    fn[noisy] = rng.integers(0, n_fn, size=int(noisy.sum()))
    otu = rng.integers(0, n_otu, size=n_prot).astype(np.int32)
    return seq, offsets, fn, otu
