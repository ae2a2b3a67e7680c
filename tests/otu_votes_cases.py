"""Caller-held record lists for the OTU vote tests: a small builder for known answers, and random lists whose sizes aim at the
lane, wave, scan-chunk and sort-tile edges of kg_votes.hpp.  Shared by the host and the GPU tests; needs no GPU."""
import numpy as np

from kmergutsjava_amd import _native as N

import otu_votes_model as V

K = 8


class Lists:
    """Hits and CALLs added in any order; build() sorts them into (container, position) order and returns the arguments of
    otu_votes_model.otu_votes / hotpath.otu_votes."""

    def __init__(self, n_seqs, per, lens=None):
        self.n_seqs, self.per = n_seqs, per
        self.lens = [1000] * n_seqs if lens is None else list(lens)
        self.h, self.c = [], []

    def hit(self, cont, pos, oI, fI, ev=N.EV_ACCEPTED):
        self.h.append((cont, pos, oI, 0, fI, 1.0, ev))
        return self

    def call(self, cont, start, n, oI, fI=1, end=None):
        """A CALL of n voting hits at start, start + 1, ...; oI one value or one per hit."""
        ois = [oI] * n if np.isscalar(oI) else list(oI)
        assert len(ois) == n
        for k in range(n):
            self.hit(cont, start + k, ois[k], fI)
        self.c.append((cont, start, start + n - 1 + (K - 1) if end is None else end, n, fI, float(n)))
        return self

    def build(self):
        n_cont = self.n_seqs * self.per
        h = sorted(self.h, key=lambda r: (r[0], r[1]))
        c = sorted(self.c, key=lambda r: (r[0], r[1]))
        hits = np.zeros(len(h), dtype=N.HIT_DTYPE)
        ev = np.zeros(len(h), dtype=np.uint8)
        for i, r in enumerate(h):
            hits[i] = r[:6]
            ev[i] = r[6]
        calls = np.zeros(len(c), dtype=N.CALL_DTYPE)
        for i, r in enumerate(c):
            calls[i] = r
        chs = np.zeros(n_cont + 1, dtype=np.int64)
        np.cumsum(np.bincount(hits["container"], minlength=n_cont), out=chs[1:])
        ccs = np.zeros(n_cont + 1, dtype=np.int64)
        np.cumsum(np.bincount(calls["container"], minlength=n_cont), out=ccs[1:])
        off = np.zeros(self.n_seqs + 1, dtype=np.int64)
        off[1:] = np.cumsum(self.lens)
        return hits, chs, ev, calls, ccs, self.n_seqs, self.per, off


def random_lists(rng, n_seqs, per, votes, calls_per_container=(0, 1, 2), n_otus=5, max_oi=None, noise=True):
    """votes: the votes of every sequence (one value for all, or one per sequence).  Each sequence's votes are dealt to its
    containers and to their CALLs (calls_per_container: the choices; a container without CALLs gets no votes); around the voting
    hits lie hits that must not vote: before the first CALL, of another function, unaccepted, one position past the last voter
    (end - 6), and with oI = -1.  n_otus: distinct OTUs a sequence draws from (all of them, when it has that many votes); max_oi: the largest oI value."""
    votes = np.full(n_seqs, votes, dtype=np.int64) if np.isscalar(votes) else np.asarray(votes, dtype=np.int64)
    n_cont = n_seqs * per
    max_oi = max(n_otus - 1, 0) if max_oi is None else max_oi
    m = rng.choice(np.asarray(calls_per_container), size=n_cont)          # CALLs per container
    hc, hp, ho, hf, he = [], [], [], [], []
    cc, cs, ce, cn, cf = [], [], [], [], []
    for s in range(n_seqs):
        conts = [s * per + k for k in range(per) if m[s * per + k] > 0]
        pool = rng.choice(max_oi + 1, size=min(n_otus, max_oi + 1), replace=False) if max_oi < (1 << 20) else \
            np.unique(np.concatenate([[0, max_oi], rng.integers(0, max_oi, size=max(n_otus - 2, 0))]))
        left = int(votes[s])
        slots = [(c, j) for c in conts for j in range(int(m[c]))]
        share = rng.multinomial(left, np.full(len(slots), 1.0 / len(slots))) if slots else []
        draw = pool[rng.integers(0, len(pool), size=left)]
        if left >= len(pool):
            draw[:len(pool)] = pool                 # every OTU of the pool has a vote
            rng.shuffle(draw)
        at, used = {}, 0
        for (c, j), nv in zip(slots, share):
            pos = at.get(c, int(rng.integers(3, 9)))
            fI = int(rng.integers(1, 6))
            if noise and j == 0:
                hc.append(c); hp.append(pos - 2); ho.append(int(pool[0])); hf.append(fI); he.append(N.EV_ACCEPTED)   # before the CALL
            start = pos
            nv = int(nv)
            ois = draw[used:used + nv]
            used += nv
            for k in range(nv):
                hc.append(c); hp.append(pos); ho.append(int(ois[k])); hf.append(fI); he.append(N.EV_ACCEPTED | (int(rng.integers(0, 64)) << 1))
                pos += 1
                if noise and k % 7 == 3:
                    kind = int(rng.integers(0, 3))
                    # another function; unaccepted; another function with a negative OTU
                    hc.append(c); hp.append(pos); ho.append(-1 if kind == 2 else int(pool[0]))
                    hf.append(fI if kind == 1 else fI + 10); he.append(0 if kind == 1 else N.EV_ACCEPTED)
                    pos += 1
            last = pos - 1 if nv else start
            cc.append(c); cs.append(start); ce.append(last + K - 1); cn.append(nv); cf.append(fI)
            if noise:
                hc.append(c); hp.append(last + 1); ho.append(int(pool[0])); hf.append(fI); he.append(N.EV_ACCEPTED)  # end - 6
            at[c] = last + 2 + int(rng.integers(0, 5))
    hits = np.zeros(len(hc), dtype=N.HIT_DTYPE)
    hits["container"], hits["from0InProt"], hits["oI"], hits["fI"] = hc, hp, ho, hf
    hits["functionWt"] = 1.0
    ev = np.asarray(he, dtype=np.uint8)
    calls = np.zeros(len(cc), dtype=N.CALL_DTYPE)
    calls["container"], calls["start"], calls["end"], calls["count"], calls["fI"] = cc, cs, ce, cn, cf
    chs = np.zeros(n_cont + 1, dtype=np.int64)
    np.cumsum(np.bincount(hits["container"], minlength=n_cont), out=chs[1:])
    ccs = np.zeros(n_cont + 1, dtype=np.int64)
    np.cumsum(np.bincount(calls["container"], minlength=n_cont), out=ccs[1:])
    off = np.zeros(n_seqs + 1, dtype=np.int64)
    off[1:] = np.cumsum(rng.integers(50, 5000, size=n_seqs))
    return hits, chs, ev, calls, ccs, n_seqs, per, off


def cut(args, a, b):
    """The records of sequences [a, b) as a list of their own."""
    hits, chs, ev, calls, ccs, n_seqs, per, off = args
    h0, h1, c0, c1 = int(chs[a * per]), int(chs[b * per]), int(ccs[a * per]), int(ccs[b * per])
    h, c = hits[h0:h1].copy(), calls[c0:c1].copy()
    h["container"] -= a * per
    c["container"] -= a * per
    return h, chs[a * per:b * per + 1] - h0, ev[h0:h1].copy(), c, ccs[a * per:b * per + 1] - c0, b - a, per, off[a:b + 1] - off[a]


def many_short(rng, n_seqs, n_otus=5):
    """Proteins (per = 1) with 0 .. 3 votes each in one CALL, and a hit at end - 6 behind it: millions of short tallies in
    small.  Built with numpy alone, so that 70 000 sequences cost no time."""
    v = rng.integers(0, 4, size=n_seqs)
    n_h = v + 1
    chs = np.zeros(n_seqs + 1, dtype=np.int64)
    np.cumsum(n_h, out=chs[1:])
    hits = np.zeros(int(chs[-1]), dtype=N.HIT_DTYPE)
    seq = np.repeat(np.arange(n_seqs), n_h)
    hits["container"] = seq
    hits["from0InProt"] = 5 + np.arange(len(hits)) - chs[seq]
    hits["oI"] = rng.integers(0, n_otus, size=len(hits))
    hits["fI"] = 2
    ev = np.full(len(hits), N.EV_ACCEPTED, dtype=np.uint8)
    has = v > 0
    calls = np.zeros(int(has.sum()), dtype=N.CALL_DTYPE)
    calls["container"] = np.flatnonzero(has)
    calls["start"] = 5
    calls["end"] = 5 + v[has] - 1 + (K - 1)
    calls["count"] = v[has]
    calls["fI"] = 2
    ccs = np.zeros(n_seqs + 1, dtype=np.int64)
    np.cumsum(has, out=ccs[1:])
    off = np.zeros(n_seqs + 1, dtype=np.int64)
    off[1:] = np.cumsum(rng.integers(30, 400, size=n_seqs))
    return hits, chs, ev, calls, ccs, n_seqs, 1, off


# ---- the scan inputs of the host and the GPU tests --------------------------------------------------------------------------

ORACLE_INPUTS = {"dna": ((37, 30, 8009, 2500), dict(seed=778, dna=True), dict()),
                 "dna_oc": ((37, 30, 8009, 2500), dict(seed=778, dna=True), dict(order_constraint=True)),
                 "aa": ((60, 200, 8009, 2500), dict(seed=12, dna=False), dict(aa=True)),
                 "aa_oc": ((60, 200, 8009, 2500), dict(seed=12, dna=False), dict(aa=True, order_constraint=True, min_hits=2))}
# CALLs and votes of the four inputs, sequences with votes (OTU column modulo 4 and 5) and with votes for all five OTUs
# (modulo 5): recorded from the oracle, so that the checks below cannot pass on empty records
RECORDED = {"dna": (123, 1100, 37, 33), "dna_oc": (15, 98, 15, 2), "aa": (1244, 10774, 60, 60), "aa_oc": (355, 1626, 60, 52)}


def oracle_input(name, modulo=None):
    """-> (table image, sequence bytes, offsets, keyword arguments of oracle.run / hotpath.Params)"""
    from kmergutsjava_amd import synth
    a, kw, run = ORACLE_INPUTS[name]
    seq, off, rec, _ = synth.high_density_config(*a, **kw)
    if modulo:
        rec[:, 2] %= modulo
    return synth.table_image(rec), seq.numpy(), np.asarray(off, dtype=np.int64), run


def model_on(res, per, off, **kw):
    return V.otu_votes(res["hits"], res["container_hit_start"], res["hit_events"], res["calls"], res["container_call_start"],
                       len(off) - 1, per, off, **kw)


def buffer_equals_pairs(otu, votes, start):
    """Every sequence's kg_otu record, read as a multiset of (count, oI), equals the model's pairs."""
    for s in range(len(otu)):
        n = int(otu["n"][s])
        buf = sorted(zip(otu["count"][s][:n].tolist(), otu["oI"][s][:n].tolist()))
        v = votes[start[s]:start[s + 1]]
        if buf != sorted(zip(v["votes"].tolist(), v["oI"].tolist())):
            return False
    return True


BIG_DNA = ((20, 1500, 20011, 9000), dict(seed=5, dna=True), dict())     # the GPU tests' scan input of about 30 000 hits
