"""Inputs that put kg_proteins_cluster (kg_cluster.hpp, kg_host_cluster.hpp) on its internal borders, and what they must give,
worked out here without the model's code: tests/test_cluster_host.py checks tests/cluster_model.py against these answers on
the CPU, tests/test_gpu_cluster_edges.py checks the device against both.

The borders: cluster_centre_kernel gives a lane LANE = 16 consecutive (k-mer, protein) pairs and a workgroup TILE = 4096; the
shared count of a link is a difference of run starts placed by a prefix sum over SCAN = 2048 items; both sorts take their
width from ceil(log2 n_prot); a window block is 64 windows of one protein.  Every batch is made of tokens
(cluster_model.token_batch), so the pair list and the link list are known item by item."""
from __future__ import annotations

import numpy as np

import cluster_model as M
from kmergutsjava_amd import _native as N

LANE = 16                       # kDeriveChunk
THREADS = 256                   # lanes of a workgroup in every cluster kernel
TILE = LANE * THREADS           # = kBuildTile, the sort's tile
SCAN = 2048                     # kScanChunk = kScanThreads * kScanPerThread
TOP = 20 ** 8 - 1               # the largest token


def _records(n, root, best, shared):
    root = np.asarray(root, dtype=np.int64)
    out = np.zeros(n, dtype=N.FAMILY_DTYPE)
    is_root = root == np.arange(n)
    assert is_root[root].all()
    out["family"] = (np.cumsum(is_root) - 1)[root]
    out["root"], out["best"], out["shared"] = root, best, shared
    return out


def family_counts(root) -> dict:
    """families, families_multi and largest of a root array."""
    size = np.bincount(np.asarray(root, dtype=np.int64))
    return dict(families=int((size > 0).sum()), families_multi=int((size >= 2).sum()), largest=int(size.max()) if size.size else 0)


# ---- a. k-mer runs against lane and workgroup borders: one token per protein ----------------------------------------------

SMALL_LEAD, LARGE_LEAD = (0, 1, 15, 16, 17), (4095, 4096, 4097)
SMALL_RUN, LARGE_RUN = (1, 2, 15, 16, 17, 31, 32, 33), (4095, 4096, 4097, 8192)
# (lead, run): the full product of the small values, the large leads with every run, the small leads with the large runs
LANE_GRID = ([(lead, run) for lead in SMALL_LEAD for run in SMALL_RUN] +
             [(lead, run) for lead in LARGE_LEAD for run in SMALL_RUN + LARGE_RUN] +
             [(lead, run) for lead in SMALL_LEAD for run in LARGE_RUN])
assert len(LANE_GRID) == 40 + 36 + 20 and len(set(LANE_GRID)) == 96
LANE_TOKENS = (7, 20 ** 8 // 3, TOP)        # the lead run's token, the token of the run under test, the tail's
LONGEST = 40                                # the pad of the one longest member; every other pad is below 23


def lane_places(lead: int, run: int):
    """Where in the run under test the one longest member goes, as offsets into the run: the first pair, the last, and the
    offsets on pair index 16 k - 1 and 16 k.  A run of at most 33 pairs gets all of them.  A run of 4095 or more has 500 or
    more, and a lane wholly inside a run executes the same instructions whichever lane it is (the maximum of its 16 pairs, one
    atomicMax), so of those the run keeps the ones within three lanes of either end and the ones on a workgroup border (pair
    index 4096 k - 1 and 4096 k), where the lane's and the workgroup's index change together."""
    at = {0, run - 1} | {a for a in range(run) if (lead + a) % LANE in (0, LANE - 1)}
    if run > 3 * 2 * LANE:
        at = {a for a in at if a < 3 * LANE or a >= run - 3 * LANE or (lead + a) % TILE in (0, TILE - 1)} | {0, run - 1}
    return sorted(at)


def one_token_groups(sizes, tokens, seed):
    """len(sizes) k-mers, k-mer g held by sizes[g] proteins that hold nothing else, the proteins dealt to the k-mers at random
    so that pair order is not protein order.  -> (token of every protein, [the sorted members of each k-mer])"""
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    perm = np.random.default_rng(seed).permutation(n)
    ends = np.cumsum(sizes)
    groups = [np.sort(perm[e - s:e]) for s, e in zip(sizes, ends)]
    tok = np.zeros(n, dtype=np.int64)
    for g, t in zip(groups, tokens):
        tok[g] = t
    return tok, groups


def lane_layout(lead: int, run: int, tail: int):
    """The three runs of one layout: `lead` proteins on the smallest token, `run` on the token under test, `tail` on a larger
    one.  -> (tokens, groups, base pads); groups[1] holds the run under test in pair order."""
    tok, groups = one_token_groups((lead, run, tail), LANE_TOKENS, 1000003 * lead + 101 * run + tail)
    pad = (np.arange(tok.size, dtype=np.int64) * 7919) % 23
    return tok, groups, pad


def one_token_batch(tok, pad):
    return M.token_batch(np.asarray(tok, dtype=np.int64).reshape(-1, 1), pad)


def one_token_answer(groups, pad):
    """min_shared = 1, min_cover_pct = 0 on proteins of one token each: every k-mer is a family, its centre the longest member
    (the smallest index on a tie), every other member has best = the centre and shared = 1.  -> (records, counts)"""
    pad = np.asarray(pad, dtype=np.int64)
    n = pad.size
    root, best, shared = np.arange(n), np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    groups = [g for g in groups if len(g)]
    for g in groups:                                        # g ascends: argmax returns the first, so the smallest index
        c = g[int(np.argmax(pad[g]))]
        root[g], best[g], shared[g] = g[0], c, 1
        best[c], shared[c] = -1, 0
    counts = dict(proteins=n, valid_windows=n, pairs=n, kmers=len(groups), links=n - len(groups), edges=n - len(groups))
    counts.update(family_counts(root))
    return _records(n, root, best, shared), counts


def lane_cases(lead: int, run: int):
    """Every input of one (lead, run): tail 0 and 1, the longest member at each of lane_places, and all lengths equal.
    Yields (name, (seq, offsets), (records, counts))."""
    for tail in (0, 1):
        tok, groups, base = lane_layout(lead, run, tail)
        for a in lane_places(lead, run):
            pad = base.copy()
            pad[groups[1][a]] = LONGEST
            yield "tail %d longest at %d" % (tail, a), one_token_batch(tok, pad), one_token_answer(groups, pad)
        pad = np.zeros(tok.size, dtype=np.int64)
        yield "tail %d equal lengths" % tail, one_token_batch(tok, pad), one_token_answer(groups, pad)


# many short runs: (name, lead, the lengths of the runs behind it)
SHORT_RUNS = [
    ("600 runs of 16 from pair 0", 0, (16,) * 600),             # every lane holds exactly one run: plain stores only
    ("600 runs of 16 from pair 8", 8, (16,) * 600),             # every run straddles one lane border
    ("5000 runs of one pair", 0, (1,) * 5000),
    ("lanes that close 5, 5 and 6", 0, (5, 5, 6) * 300),        # three runs end in every lane
    ("lanes that close 5, 5 and 6 from pair 3", 3, (5, 5, 6) * 300),
]


def short_runs_case(lead: int, sizes):
    """-> ((seq, offsets), (records, counts)); the k-mers' tokens ascend with the run's place in the pair list"""
    sizes = ((lead,) if lead else ()) + tuple(sizes)
    tokens = 11 + 104729 * np.arange(len(sizes), dtype=np.int64)
    tok, groups = one_token_groups(sizes, tokens, 17 * lead + len(sizes))
    pad = (np.arange(tok.size, dtype=np.int64) * 7919) % 5      # many ties
    return one_token_batch(tok, pad), one_token_answer(groups, pad)


# ---- b. link runs against the scan chunk ------------------------------------------------------------------------------------

LINK_S = (1, 2047, 2048, 2049, 4097)
LINK_LEAD = (0, 2047, 2048)


def link_case(s: int, lead_links: int, extra: int = 0, min_shared: int = 1, min_cover_pct: int = 0):
    """Proteins 0 .. lead_links - 1 hold one token each, m = lead_links holds s tokens and `extra` private ones, and
    c = lead_links + 1, the longest, holds the lead tokens and the s.  The sorted link list is the lead_links links (i, c) and
    then m's run of s items, which so starts at item lead_links.  -> ((seq, offsets), (records, counts))"""
    L, m, c = lead_links, lead_links, lead_links + 1
    shared_tok = L + np.arange(s, dtype=np.int64)
    members = [[i] for i in range(L)] + [np.concatenate([shared_tok, L + s + np.arange(extra, dtype=np.int64)]),
                                         np.concatenate([np.arange(L, dtype=np.int64), shared_tok])]
    pad = np.zeros(L + 2, dtype=np.int64)
    pad[c] = max(0, 9 * (extra - L)) + 1                        # c is longer than m, and than every lead member
    edge_m = s >= min_shared and 100 * s >= min_cover_pct * (s + extra)
    edge_lead = 1 >= min_shared                                 # 100 * 1 >= pct * 1 always holds
    n = L + 2
    root, best, shared = np.arange(n), np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    if edge_lead:
        best[:L], shared[:L] = c, 1
    if edge_m:
        best[m], shared[m] = c, s
    joined = ([m] if edge_m else []) + (list(range(L)) if edge_lead else [])
    if joined:
        root[joined + [c]] = min(joined)
    pairs = L + s + extra + L + s
    counts = dict(proteins=n, valid_windows=pairs, pairs=pairs, kmers=L + s + extra, links=L + 1, edges=L * int(edge_lead) + int(edge_m))
    counts.update(family_counts(root))
    return M.token_batch(members, pad), (_records(n, root, best, shared), counts)


def link_threshold_cases(s: int, lead_links: int):
    """At the two tests' bounds: min_shared = s and s + 1; 100 s == pct d_m for pct 50 and 100, and one private token more.
    Yields (name, (min_shared, pct), batch, answer, whether m's link is an edge)."""
    for name, extra, ms, pct, edge in (("min_shared = s", 0, s, 0, True), ("min_shared = s + 1", 0, s + 1, 0, False),
                                       ("100 s == 50 d", s, 1, 50, True), ("100 s < 50 (d + 1)", s + 1, 1, 50, False),
                                       ("100 s == 100 d", 0, 1, 100, True), ("100 s < 100 (d + 1)", 1, 1, 100, False)):
        batch, answer = link_case(s, lead_links, extra, ms, pct)
        yield name, (ms, pct), batch, answer, edge


THREE_CENTRES = [(s, third, m_first) for s in (2047, 2048, 2049) for third in (s - 1, s + 1) for m_first in (True, False)]


def three_centres_case(s: int, third: int, m_first: bool):
    """One member m with s tokens in common with each of two centres and `third` with the highest-indexed centre; every
    centre is longer than m.  m's three link runs start at items 0, s and 2 s.  best[m] is the smaller of the two equal
    centres unless third > s.  min_shared = 1, min_cover_pct = 0.  -> ((seq, offsets), (records, counts))"""
    m = 0 if m_first else 3
    cs = [1, 2, 3] if m_first else [0, 1, 2]
    sizes = (s, s, third)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    blocks = [np.arange(starts[k], starts[k + 1], dtype=np.int64) for k in range(3)]
    members, pad = [None] * 4, np.zeros(4, dtype=np.int64)
    members[m] = np.concatenate(blocks)
    for k, c in enumerate(cs):
        members[c] = blocks[k]
        pad[c] = 9 * (int(starts[3]) - sizes[k]) + 1 + k        # longer than m, and all three lengths differ
    best, shared = np.full(4, -1, dtype=np.int64), np.zeros(4, dtype=np.int64)
    best[m], shared[m] = (cs[2], third) if third > s else (cs[0], s)
    total = int(starts[3])
    counts = dict(proteins=4, valid_windows=2 * total, pairs=2 * total, kmers=total, links=3, edges=3, families=1, families_multi=1, largest=4)
    return M.token_batch(members, pad), (_records(4, np.zeros(4, dtype=np.int64), best, shared), counts)


# ---- the rule on tokens, in plain loops (for batches whose answer has no closed form) -------------------------------------

def token_answer(members, pad, min_shared: int = 1, min_cover_pct: int = 0):
    """The family rule applied to the token sets themselves, with dicts and cluster_model.components: no windows, no sort,
    no rounds.  -> (records, counts)"""
    n = len(members)
    length = [9 * len(members[p]) + int(pad[p]) for p in range(n)]
    holders = {}
    for p in range(n):
        for v in set(int(v) for v in members[p]):
            holders.setdefault(v, []).append(p)
    s_of = {}
    for v, ps in holders.items():
        c = ps[0]
        for p in ps[1:]:                                        # ps ascends: a later protein wins only when it is longer
            if length[p] > length[c]:
                c = p
        for p in ps:
            if p != c:
                s_of[(p, c)] = s_of.get((p, c), 0) + 1
    best, shared, edges = [-1] * n, [0] * n, []
    for (m, c), s in s_of.items():
        if s >= min_shared and 100 * s >= min_cover_pct * len(set(int(v) for v in members[m])):
            edges.append((m, c))
            if s > shared[m] or (s == shared[m] and c < best[m]):
                best[m], shared[m] = c, s
    root = M.components(n, edges)
    pairs = sum(len(ps) for ps in holders.values())
    counts = dict(proteins=n, valid_windows=sum(len(m) for m in members), pairs=pairs, kmers=len(holders), links=len(s_of), edges=len(edges))
    counts.update(family_counts(root))
    return _records(n, root, best, shared), counts


# ---- c. key widths ----------------------------------------------------------------------------------------------------------

KEY_WIDTH_N = (1, 2, 3, 4, 5, 8, 9, 64, 65, 1024, 1025, 65536, 65537, 131073)


def key_width_case(n: int):
    """Every protein holds token 0 (even index) or the largest token (odd index), so the window key's top bits are used; the
    private tokens of the edges among n - 1, n - 2, n - 3 and of (0, n - 1) put the top bit of the protein index into both
    sorts' keys.  min_shared = 1, min_cover_pct = 0.  -> (members, pad)"""
    members = [[0 if p % 2 == 0 else TOP] for p in range(n)]
    wanted = [(n - 1, n - 2), (n - 2, n - 3), (n - 1, n - 3), (0, n - 1)]
    extra = sorted({(min(a, b), max(a, b)) for a, b in wanted if min(a, b) >= 0 and a != b})
    for e, (a, b) in enumerate(extra):
        members[a].append(20 ** 8 // 2 + e)
        members[b].append(20 ** 8 // 2 + e)
    return members, (np.arange(n, dtype=np.int64) * 7) % 5


# ---- d. window blocks -------------------------------------------------------------------------------------------------------

BLOCK_LENGTHS = (8, 9, 71, 72, 73, 136, 137)


def block_edge_batch(length: int):
    """Six families of four proteins of one length: a random base, an exact copy and two copies with about 3 % of the residues
    replaced.  -> list of bytes; protein 4 f + k is copy k of base f"""
    rng = np.random.default_rng(length)
    alpha = np.frombuffer(M.ALPHA, dtype=np.uint8)
    prots = []
    for _ in range(6):
        base = alpha[rng.integers(0, 20, size=length)]
        prots += [base.tobytes(), base.tobytes()]
        for _ in range(2):
            s = base.copy()
            mut = rng.random(length) < 0.03
            s[mut] = alpha[rng.integers(0, 20, size=int(mut.sum()))]
            prots.append(s.tobytes())
    return prots


def check_block_edge_records(length: int, rec, counts):
    """What the defaults (5, 20) must give whatever the mutations were."""
    assert counts["valid_windows"] == 24 * max(length - 8, 0)
    groups = M.partition(rec)
    assert all(len({i // 4 for i in g}) == 1 for g in groups)               # random bases share no 8-mer
    if length <= 12:                                                        # fewer than 5 windows: no link passes min_shared
        assert counts["families"] == 24 and counts["edges"] == 0
    else:
        for f in range(6):                                                  # the exact copy shares every k-mer with its base
            assert rec["root"][4 * f + 1] == rec["root"][4 * f] == 4 * f
            assert rec[4 * f + 1]["best"] == 4 * f and rec[4 * f + 1]["shared"] == length - 8


# ---- e. component shapes ----------------------------------------------------------------------------------------------------

def _bit_reverse(i: int, bits: int) -> int:
    return int(format(i, "0%db" % bits)[::-1], 2)


def component_shapes():
    """name -> (n, edges).  The cliques and the bipartite block lie spread among proteins without any k-mer."""
    shapes = {}
    n = 20000
    path = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    shapes["path ascending"] = (n, path)
    shapes["path descending"] = (n, n - 1 - path)
    order = np.array([_bit_reverse(i, 14) for i in range(16384)])
    shapes["path bit-reversed"] = (16384, np.stack([order[:-1], order[1:]], axis=1))
    shapes["ring"] = (n, np.concatenate([path, [[n - 1, 0]]]))
    tree = np.stack([np.arange(1, n), (np.arange(1, n) - 1) // 2], axis=1)
    shapes["binary tree heap order"] = (n, tree)
    shapes["binary tree reversed"] = (n, n - 1 - tree)
    node = np.arange(128 * 128).reshape(128, 128)
    shapes["grid 128 x 128"] = (128 * 128, np.concatenate([np.stack([node[:, :-1].ravel(), node[:, 1:].ravel()], axis=1),
                                                            np.stack([node[:-1, :].ravel(), node[1:, :].ravel()], axis=1)]))
    half = np.stack([np.arange(4999), np.arange(1, 5000)], axis=1)
    shapes["two paths of 5000 joined at their far ends"] = (10000, np.concatenate([half, half + 5000, [[4999, 9999]]]))
    shapes["10000 disjoint pairs"] = (n, np.stack([np.arange(10000), np.arange(10000) + 10000], axis=1))
    left, right = 5 + 128 * np.arange(64), 16383 - 128 * np.arange(64)
    shapes["bipartite 64 x 64"] = (16384, np.array([(a, b) for a in left for b in right]))
    nodes = 3 + 128 * np.arange(128)
    shapes["clique of 128"] = (16384, np.array([(nodes[i], nodes[j]) for i in range(128) for j in range(i + 1, 128)]))
    small = []
    for k in range(200):
        nodes = 7 + k + 1000 * np.arange(16)                    # clique k: 16 proteins 1000 apart, the cliques interleaved
        small += [(nodes[i], nodes[j]) for i in range(16) for j in range(i + 1, 16)]
    shapes["200 cliques of 16"] = (16384, np.array(small))
    return shapes


COMPONENT_SHAPES = ("path ascending", "path descending", "path bit-reversed", "ring", "binary tree heap order", "binary tree reversed",
                    "grid 128 x 128", "two paths of 5000 joined at their far ends", "10000 disjoint pairs", "bipartite 64 x 64",
                    "clique of 128", "200 cliques of 16")


def check_component_records(n, edges, rec, counts):
    """root, the numbering of the families and the three family counts against the sequential union-find."""
    root = M.components(n, edges)
    assert (rec["root"] == root).all()
    assert (rec["family"] == (np.cumsum(root == np.arange(n)) - 1)[root]).all()
    want = family_counts(root)
    assert {k: counts[k] for k in want} == want
    assert counts["links"] == counts["edges"] == len(edges) and counts["kmers"] == len(edges) and counts["pairs"] == 2 * len(edges)
    return want
