"""One window-pairs pass under three hosts (kg_host_derive.hpp: Deriver::window_pairs): kg_proteins_cluster, kg_proteins_search,
kg_proteins_search_seeded with the exact seed set and kg_signatures_derive, in one pass and in several, count the same valid
windows, distinct (k-mer, protein) pairs and k-mers on one batch, and they are what the models count.  Raw ctypes through
_native, so nothing of hotpath.py stands between the test and the four entry points."""
import ctypes as C

import numpy as np
import pytest

import cluster_model as M
import search_model as S
import seed_model as SD
import signature_model as G
from kmergutsjava_amd import _native as N

LENGTHS = (0, 8, 9, 71, 72, 73, 136, 137)               # no window, no window, one; 63, 64, 65 and 128, 129: the 64-window blocks
N_DB = 20
SMALL_PASS = 800                                        # of the 2000 valid windows: three passes at least
ALIGN = (50, 0, 11, 1, 1 << 26, None, 0)


def _batch():
    """40 proteins, five of each length.  Planted: one 8-mer at the head of every protein that has a window, a second one twice in
    protein 7 and once in proteins 15 and 39, a third across the target / query border; X in the tails of the long proteins."""
    rng = np.random.default_rng(20261)
    prots = [bytearray(rng.choice(np.frombuffer(M.ALPHA, dtype=np.uint8), size=LENGTHS[p % 8]).tobytes()) for p in range(40)]
    everywhere, twice, border = b"ACDEFGHI", b"WYWYKLMN", b"PQRSTVWC"
    for p, s in enumerate(prots):
        if len(s) >= 9:
            s[0:8] = everywhere
        if len(s) >= 136:
            for at in (64 + 8 - 1, 64 + 8, 100 + p % 7, 127):       # around the first block's last window, and further on
                s[at] = ord("X")
    prots[7][10:18] = twice
    prots[7][40:48] = twice
    prots[15][20:28] = twice
    prots[39][30:38] = twice
    prots[6][12:20] = border
    prots[N_DB + 2][12:20] = border
    return M.pack([bytes(s) for s in prots])


SEQ, OFF = _batch()
WANT = {k: v for k, v in M.cluster_numpy(SEQ, OFF)[1].items() if k in ("valid_windows", "pairs", "kmers")}


def test_the_models_agree_on_the_batch():
    """Before any device code: the four models count the same windows, pairs and k-mers, and the planted 8-mers are in them."""
    assert len(OFF) - 1 == 40 and sorted(set(np.diff(OFF).tolist())) == list(LENGTHS)
    keys = ("valid_windows", "pairs", "kmers")
    assert {k: M.cluster_loops(SEQ, OFF)[1][k] for k in keys} == WANT
    assert {k: S.shared_numpy(SEQ, OFF, N_DB)[1][k] for k in keys} == WANT
    assert {k: SD.shared_numpy(SD.EXACT)(SEQ, OFF, N_DB)[1][k] for k in keys} == WANT
    fn = otu = [0] * 40
    assert len(G.brute_force(SEQ, OFF, fn, otu, min_proteins=1, purity_pct=100)) == WANT["kmers"]       # one function: every k-mer signs
    total = int(np.maximum(np.diff(OFF) - 8, 0).sum())
    assert WANT["kmers"] < WANT["pairs"] < WANT["valid_windows"] < total and total > 2 * SMALL_PASS
    v, p = S.kmer_pairs(SEQ, OFF)
    planted = int(v[(p == 7)][10])
    assert planted == int(v[p == 7][40]) and sorted(p[v == planted].tolist()) == [7, 7, 15, 39]           # twice in 7: one pair


def _arrays():
    return np.frombuffer(SEQ, dtype=np.uint8), np.ascontiguousarray(OFF, dtype=np.int64)


def _stats(rc, lib, h, stats, getter, free):
    assert rc == 0, lib.kg_last_error().decode()
    try:
        assert getter(h, C.byref(stats)) == 0
        return stats.as_dict()
    finally:
        free(h)


def _cluster():
    lib, h, (arr, off) = N.load(), C.c_void_p(), _arrays()
    prm = N.KgClusterParams(5, 20, 0)
    rc = lib.kg_proteins_cluster(0, C.byref(prm), arr.ctypes.data, off.ctypes.data, len(off) - 1, 0, C.byref(h))
    return _stats(rc, lib, h, N.KgClusterStats(), lib.kg_familyset_stats, lib.kg_familyset_free)


def _search(seeded):
    lib, h, (arr, off) = N.load(), C.c_void_p(), _arrays()
    prm, al = N.KgSearchParams(2, 8, 256, 0), N.KgAlignParams(*ALIGN)
    if seeded:
        sp = N.KgSeedParams()
        assert lib.kg_seed_params_builtin(N.SEEDS_EXACT, C.byref(sp)) == 0
        rc = lib.kg_proteins_search_seeded(0, C.byref(prm), C.byref(sp), C.byref(al), arr.ctypes.data, off.ctypes.data, len(off) - 1, N_DB, 0,
                                           0, 0, 0, C.byref(h))
    else:
        rc = lib.kg_proteins_search(0, C.byref(prm), C.byref(al), arr.ctypes.data, off.ctypes.data, len(off) - 1, N_DB, 0, 0, C.byref(h))
    return _stats(rc, lib, h, N.KgSearchStats(), lib.kg_hitset_stats, lib.kg_hitset_free)


def _derive(max_windows_per_pass):
    lib, h, (arr, off) = N.load(), C.c_void_p(), _arrays()
    prm = N.KgDeriveParams(1, 100, max_windows_per_pass)
    fn = np.zeros(len(off) - 1, dtype=np.int32)
    rc = lib.kg_signatures_derive(0, C.byref(prm), arr.ctypes.data, off.ctypes.data, len(off) - 1, fn.ctypes.data, fn.ctypes.data, C.byref(h))
    return _stats(rc, lib, h, N.KgDeriveStats(), lib.kg_sigset_stats, lib.kg_sigset_free)


@pytest.mark.gpu
def test_five_runs_of_one_pass_count_the_same():
    runs = {"cluster": _cluster(), "search": _search(False), "seeded": _search(True), "derive": _derive(0), "derive, passes": _derive(SMALL_PASS)}
    for name, st in runs.items():
        print(name, {k: st[k] for k in ("valid_windows", "pairs", "kmers")}, st.get("passes", ""))
    assert runs["derive"]["passes"] == 1 and runs["derive, passes"]["passes"] >= 3
    for name, st in runs.items():
        # (a derive call's pairs and k-mers are sums over its passes: a pair, and a k-mer, lies in exactly one k-mer range)
        assert {k: st[k] for k in WANT} == WANT, name
    assert runs["search"]["targets"] == N_DB and runs["search"]["queries"] == 40 - N_DB and runs["search"]["join_pairs"] > 0
    assert runs["seeded"]["join_pairs"] == runs["search"]["join_pairs"]
    for name in ("derive", "derive, passes"):
        assert runs[name]["signatures"] == WANT["kmers"], name                      # min_proteins 1, one function: every k-mer signs
