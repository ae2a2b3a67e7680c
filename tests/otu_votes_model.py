"""The OTU vote rule of include/kmerguts_hip.h (kg_result_otu_votes, rules 1 to 5) in plain numpy: what the device stage
must reproduce byte for byte.  Written from the rule, not from the kernels; it takes the event bytes as input."""
import numpy as np

from kmergutsjava_amd import _native as N

K = 8


def vote_calls(hits, container_hit_start, hit_events, calls, container_call_start):
    """Rule 1 -> int64[n_hits]: the index in calls[] of the CALL every hit votes in, -1 for a hit that does not vote."""
    chs = np.asarray(container_hit_start, dtype=np.int64)
    ccs = np.asarray(container_call_start, dtype=np.int64)
    n_cont = chs.size - 1
    n, m = int(chs[-1]) if chs.size else 0, int(ccs[-1]) if ccs.size else 0
    out = np.full(n, -1, dtype=np.int64)
    if n == 0 or m == 0:
        return out
    hits, calls, ev = hits[:n], calls[:m], np.asarray(hit_events[:n], dtype=np.uint8)
    h_cont = np.repeat(np.arange(n_cont, dtype=np.int64), np.diff(chs))
    c_cont = np.repeat(np.arange(n_cont, dtype=np.int64), np.diff(ccs))
    start = calls["start"].astype(np.int64)
    same = c_cont[1:] == c_cont[:-1]
    if np.any(same & (start[1:] <= start[:-1])):
        raise ValueError("the CALL starts of a container must ascend strictly")
    pos = hits["from0InProt"].astype(np.int64)
    bias = 1 << 31
    c_key = (c_cont << 32) | (start + bias)
    h_key = (h_cont << 32) | (pos + bias)
    k = np.searchsorted(c_key, h_key, side="right") - 1          # the last CALL of the container that starts at or before the hit
    exists = k >= ccs[h_cont]
    kk = np.where(exists, k, 0)
    vote = (exists & ((ev & N.EV_ACCEPTED) != 0) & (calls["fI"][kk] == hits["fI"]) &
            (pos + (K - 1) <= calls["end"][kk].astype(np.int64)))
    out[vote] = k[vote]
    if np.any(hits["oI"][vote] < 0):
        raise ValueError("hit %d: a voting hit with oI < 0" % int(np.flatnonzero(vote & (hits["oI"] < 0))[0]))
    return out


def otu_votes(hits, container_hit_start, hit_events, calls, container_call_start, n_seqs, per, offsets,
              min_votes=10, min_share_pct=50, min_calls=1):
    """Rules 1 to 5 -> (votes VOTE_DTYPE, vote_start int64[n_seqs + 1], classes OTU_CLASS_DTYPE[n_seqs], bins OTU_BIN_DTYPE)."""
    chs = np.asarray(container_hit_start, dtype=np.int64)
    ccs = np.asarray(container_call_start, dtype=np.int64)
    off = np.asarray(offsets, dtype=np.int64)
    assert per in (1, 6) and chs.size == n_seqs * per + 1 and ccs.size == chs.size and off.size == n_seqs + 1
    k = vote_calls(hits, chs, hit_events, calls, ccs)
    idx = np.flatnonzero(k >= 0)
    h_cont = np.repeat(np.arange(n_seqs * per, dtype=np.int64), np.diff(chs))
    seq = h_cont[idx] // per
    oi = hits["oI"][:k.size][idx].astype(np.int64)
    # rule 2: the votes ordered by (seq, oI, CALL); a pair is a run of (seq, oI), its n_calls the distinct CALLs in the run
    pair_key = seq * (1 << 31) + oi
    order = np.lexsort((k[idx], pair_key))
    pair_key, kv = pair_key[order], k[idx][order]
    new_pair = np.ones(len(pair_key), dtype=bool)
    new_pair[1:] = pair_key[1:] != pair_key[:-1]
    new_call = new_pair.copy()
    new_call[1:] |= kv[1:] != kv[:-1]
    first = np.flatnonzero(new_pair)
    n_votes = np.diff(np.append(first, len(pair_key)))
    n_calls = np.add.reduceat(new_call.astype(np.int64), first) if first.size else np.zeros(0, np.int64)
    p_seq, p_oi = pair_key[first] >> 31, pair_key[first] & ((1 << 31) - 1)
    # rule 3
    order = np.lexsort((p_oi, -n_votes, p_seq))
    votes = np.zeros(first.size, dtype=N.VOTE_DTYPE)
    votes["seq"], votes["oI"], votes["votes"], votes["n_calls"] = p_seq[order], p_oi[order], n_votes[order], n_calls[order]
    vote_start = np.zeros(n_seqs + 1, dtype=np.int64)
    np.cumsum(np.bincount(votes["seq"], minlength=n_seqs), out=vote_start[1:])
    # rule 4
    classes = np.zeros(n_seqs, dtype=N.OTU_CLASS_DTYPE)
    classes["otu"] = classes["second_otu"] = -1
    classes["total_calls"] = ccs[per::per] - ccs[:-1:per] if n_seqs else 0
    n_otus = np.diff(vote_start)
    classes["n_otus"] = n_otus
    total = np.zeros(n_seqs, dtype=np.int64)
    np.add.at(total, votes["seq"], votes["votes"].astype(np.int64))
    if np.any(total >= 1 << 31):
        raise OverflowError("sequence %d: 2^31 or more votes" % int(np.flatnonzero(total >= 1 << 31)[0]))
    classes["total"] = total
    has, two = n_otus > 0, n_otus > 1
    best = votes[vote_start[:-1][has]]
    classes["otu"][has], classes["votes"][has], classes["n_calls"][has] = best["oI"], best["votes"], best["n_calls"]
    second = votes[vote_start[:-1][two] + 1]
    classes["second_otu"][two], classes["second_votes"][two] = second["oI"], second["votes"]
    classes["assigned"][has] = ((best["votes"] >= min_votes) & (best["n_calls"] >= min_calls) &
                                (100 * best["votes"].astype(np.int64) >= min_share_pct * total[has]))
    # rule 5
    asg = np.flatnonzero(classes["assigned"])
    o, which = np.unique(classes["otu"][asg], return_inverse=True)
    acc = np.zeros((4, len(o)), dtype=np.int64)
    for row, val in enumerate((np.ones(len(asg), np.int64), np.diff(off)[asg], classes["votes"][asg], classes["n_calls"][asg])):
        np.add.at(acc[row], which, val.astype(np.int64))
    order = np.lexsort((o, -acc[2], -acc[1]))
    bins = np.zeros(len(o), dtype=N.OTU_BIN_DTYPE)
    bins["oI"], bins["n_seqs"], bins["length"], bins["votes"], bins["n_calls"] = o[order], acc[0][order], acc[1][order], acc[2][order], acc[3][order]
    return votes, vote_start, classes, bins


def merge_bins(parts):
    """The bins of several batches added up and put in rule 5's order."""
    acc = {}
    for bins in parts:
        for b in bins:
            a = acc.setdefault(int(b["oI"]), [0, 0, 0, 0])
            a[0] += int(b["n_seqs"]); a[1] += int(b["length"]); a[2] += int(b["votes"]); a[3] += int(b["n_calls"])
    rows = sorted(((o, *v) for o, v in acc.items()), key=lambda r: (-r[2], -r[3], r[0]))
    out = np.zeros(len(rows), dtype=N.OTU_BIN_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out
