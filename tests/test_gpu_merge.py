"""kg_table_merge_signatures on the device against tests/merge_model.py, byte for byte (include/kmerguts_hip.h states the rule):
the merged set and its counts against merge_numpy, the table placed from it against synth.build_table.

KG_ERR_BUSY is not checked here: no existing hook leaves a kg_scan* in flight on a table without a second thread (the busy flag is
taken and given back inside one call), so the second of the ordered errors is left to the code's own reading."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import merge_model as M  # noqa: E402

MAX = M.MAX
TILE = 4096                 # kg_build.hpp kBuildTile


def _N():
    from kmergutsjava_amd import _native
    return _native


def _hot():
    from kmergutsjava_amd import hotpath
    return hotpath


def _random_sigs(n, seed, lo=0, hi=MAX, n_fn=50, n_otu=9):
    rng = np.random.default_rng(seed)
    k = np.unique(rng.integers(lo, hi, size=n, dtype=np.int64))
    out = np.zeros(len(k), dtype=_N().SIGNATURE_DTYPE)
    out["kmer"] = k
    out["otuIndex"] = rng.integers(0, n_otu, len(k))
    out["avgFromEnd"] = rng.integers(0, 500, len(k))
    out["functionIndex"] = rng.integers(0, n_fn, len(k))
    out["functionWt"] = (1 + rng.integers(0, 64, len(k))).astype(np.float32) / 16
    return out[rng.permutation(len(k))]


def _dev(sigs):
    import torch
    return torch.from_numpy(np.ascontiguousarray(sigs).view(np.uint8).copy()).cuda()


def _saved(tab, tmp_path, name="t.mem_map"):
    p = tmp_path / name
    tab.save(str(p))
    return p.read_bytes()


def _check(tab, stream, new, fn_map=None, otu_map=None, policy="keep", entry="host"):
    """one merge call == merge_numpy on the table's record stream: the set's bytes, its counts, the other set calls -> U"""
    want, counts = M.merge_numpy(stream, new, fn_map, otu_map, policy)
    with tab.merge_signatures(_dev(new) if entry == "device" else new, fn_map, otu_map, policy) as u:
        got, st = u.numpy(), u.merge_stats()
        assert got.tobytes() == want.tobytes(), (policy, entry)
        assert {k: st[k] for k in M.COUNTS} == counts, (policy, entry)
        assert u.count == len(want) and u.stats() == dict(dict.fromkeys(u.stats(), 0), signatures=len(want))
        assert bytes(u.device_tensor().cpu().numpy()) == want.tobytes()
        assert st["ms_total"] >= 0
    return want


def _error(tab, stream, new, fn_map=None, otu_map=None, policy="keep", entry="host"):
    """the call fails with the error the model raises first, naming the same index or k-mer"""
    N = _N()
    with pytest.raises(M.MergeError) as want:
        M.merge_numpy(stream, new, fn_map, otu_map, policy)
    with pytest.raises(N.KmerGutsNativeError) as ei:
        tab.merge_signatures(_dev(new) if entry == "device" else new, fn_map, otu_map, policy)
    assert ei.value.code == N.KG_ERR_ARG
    for part in want.value.message_parts():
        assert part in str(ei.value), (part, str(ei.value))
    return want.value


@pytest.fixture(scope="module")
def line_base():
    """k-mers 0 .. 8999 in a 10 007-slot table: sorted position == k-mer"""
    N = _N()
    s = np.zeros(9000, dtype=N.SIGNATURE_DTYPE)
    s["kmer"] = np.arange(9000)
    s["otuIndex"], s["avgFromEnd"], s["functionIndex"], s["functionWt"] = s["kmer"] % 7, s["kmer"] % 400, s["kmer"] % 5, 0.5
    image, placed = M.place(s, 10_007)
    assert placed == 9000
    tab = _hot().SignatureTable.build(s[np.random.default_rng(1).permutation(9000)], 10_007)
    yield tab, M.records_of_image(image)[1]
    tab.close()


# ---- 1. export round trip -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_sigs", [1, 2, 7, 64, 4095, 4096, 4097, 50_021])
@pytest.mark.parametrize("load", [0, 0.5, 1.0])
def test_export_round_trip(tmp_path, num_sigs, load):
    sigs = _random_sigs(int(num_sigs * load), 3 + num_sigs)
    image, placed = M.place(sigs, num_sigs)             # at load 1.0 some are dropped at the end: the records say which
    stream = M.records_of_image(image)[1]
    with _hot().SignatureTable.build(sigs, num_sigs) as tab:
        assert tab.placed == placed and _saved(tab, tmp_path) == image
        want = _check(tab, stream, M.sigs([]))
        assert len(want) == placed and (np.diff(want["kmer"]) > 0).all()
        with tab.signatures() as u, _hot().SignatureTable.build(u.device_tensor(), num_sigs) as again:
            assert u.numpy().tobytes() == want.tobytes() and again.placed == placed
            assert _saved(again, tmp_path, "again.mem_map") == image
        assert tab.live_device_bytes() == 0


# ---- 2. one conflict at every border ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [0, 62, 63, 64, 4094, 4095, 4096, 8191, 8999])
def test_one_conflict_at_wave_and_tile_borders(line_base, v):
    """the base pair of k-mer v sorts to position v, the new pair to v + 1: inside a wave, across a wave border (63 | 64) and
    across a kBuildTile border (4095 | 4096)"""
    tab, stream = line_base
    for policy in M.POLICIES:
        for fn in (v % 5, v % 5 + 1):
            new = M.sigs([(v, 3, 1, fn, 2.0)])
            U = _check(tab, stream, new, policy=policy, entry="device" if v % 2 else "host")
            assert len(U) == (8999 if policy == "drop" and fn != v % 5 else 9000)


# ---- 3. sizes -------------------------------------------------------------------------------------------------------------------
def _ordered(sigs, how):
    o = np.argsort(sigs["kmer"], kind="stable")
    return sigs[o] if how == "sorted" else sigs[o[::-1]].copy() if how == "reversed" else sigs


@pytest.mark.parametrize("n_base", [0, 1, 4095, 4096, 4097])
def test_sizes_overlaps_orders_and_entries(n_base):
    S = max(2 * n_base + 1, 3)
    base = _random_sigs(n_base * 4, 100 + n_base)
    base = base[base["kmer"] % S < S - n_base][:n_base]          # homes that leave room behind them: nothing is dropped at the end
    assert len(base) == n_base
    image, placed = M.place(base, S)
    stream = M.records_of_image(image)[1]
    assert placed == n_base
    combos = [(e, o) for e in ("host", "device") for o in ("sorted", "reversed", "shuffled")]
    with _hot().SignatureTable.build(base, S) as tab:
        k = 0
        for n in (0, 1, 63, 64, 65, 4096, 4097):
            fresh = _random_sigs(n * 2 + 8, 7 + n, n_fn=3)
            fresh = fresh[~np.isin(fresh["kmer"], base["kmer"])][:n]
            assert len(fresh) == n
            for overlap in ("none", "half", "all"):
                shared = min({"none": 0, "half": n // 2, "all": n}[overlap], n_base)
                new = fresh.copy()
                new["kmer"][:shared] = base["kmer"][:shared]
                new["functionIndex"][:shared:2] = base["functionIndex"][:shared:2]      # every other conflict names the same function
                entry, order = combos[k % 6]
                k += 1
                for policy in M.POLICIES:
                    U = _check(tab, stream, _ordered(new, order), policy=policy, entry=entry)
                    assert len(U) >= n_base - shared
        assert tab.live_device_bytes() == 0 and k == 21 and _check(tab, stream, M.sigs([])).tobytes() == np.sort(base, order="kmer").tobytes()


# ---- 4. maps --------------------------------------------------------------------------------------------------------------------
def test_maps(line_base):
    tab, stream = line_base
    rng = np.random.default_rng(8)
    fn_map = rng.permutation(40).astype(np.int32) - 11            # non-monotone, negative values among them
    otu_map = np.array([5, -2, 1000, 0, 3], dtype=np.int32)
    new = _random_sigs(3000, 9, 0, 20_000, n_fn=40, n_otu=5)      # about half of them below 9000: conflicts
    for policy in M.POLICIES:
        for fm, om in ((fn_map, otu_map), (fn_map, None), (None, otu_map), (None, None)):
            _check(tab, stream, new, fm, om, policy, "device" if om is None else "host")
    # drop compares after mapping: k-mer 10 (base function 0) and k-mer 11 (base function 1)
    new = M.sigs([(10, 0, 0, 3, 1.0), (11, 0, 0, 1, 1.0)])
    swap = np.array([9, 8, 7, 0], dtype=np.int32)                 # raw 3 != 0 but mapped 3 -> 0 agrees; raw 1 == 1 but mapped 1 -> 8 differs
    U = _check(tab, stream, new, swap, None, "drop")
    assert 10 in U["kmer"] and 11 not in U["kmer"] and len(U) == 8999
    U = _check(tab, stream, new, None, None, "drop")
    assert 10 not in U["kmer"] and 11 in U["kmer"]
    U = _check(tab, stream, new, swap, None, "replace")
    assert U[U["kmer"] == 10]["functionIndex"][0] == 0 and U[U["kmer"] == 11]["functionIndex"][0] == 8


# ---- 5. bytes -------------------------------------------------------------------------------------------------------------------
def test_the_record_bytes_survive_unchanged():
    base = M.sigs([(100, -7, -9, 1, 0), (200, -(2 ** 31), 2 ** 31 - 1, 2, 0), (300, 0, 0, 3, 1.5)])
    base.view(np.uint32).reshape(-1, 6)[0, 5] = 0x7FC00001        # a NaN with a payload
    base.view(np.uint32).reshape(-1, 6)[1, 5] = 0x80000000        # -0.0
    new = M.sigs([(150, 1, -4, 0, 0), (250, 0, 5, 1, 0), (300, 1, 1, 1, 0)])
    new.view(np.uint32).reshape(-1, 6)[:, 5] = [0x7FC00001, 0x80000000, 0xFFFFFFFF]
    image, _ = M.place(base, 11)
    stream = M.records_of_image(image)[1]
    with _hot().SignatureTable.build(base, 11) as tab:
        for policy in M.POLICIES:
            for entry in ("host", "device"):
                U = _check(tab, stream, new, np.array([4, 6], dtype=np.int32), None, policy, entry)
                bits = dict(zip(U["kmer"].tolist(), U.view(np.uint32).reshape(-1, 6)[:, 5].tolist()))
                assert bits[100] == 0x7FC00001 and bits[200] == 0x80000000 and bits[150] == 0x7FC00001 and bits[250] == 0x80000000
                assert bits.get(300) == {"keep": 0x3FC00000, "replace": 0xFFFFFFFF, "drop": None}[policy]
                assert U[0]["otuIndex"] == -7 and U[0]["avgFromEnd"] == -9 and U[2]["otuIndex"] == -(2 ** 31)


# ---- 6. foreign base tables -----------------------------------------------------------------------------------------------------
def _image(num_sigs, records):
    return struct.pack("<qqq", num_sigs, 24, 1) + records.tobytes()


def test_foreign_base_tables():
    E = M.MAX + 1
    rec = M.sigs([(E, 0, 0, 0, 0), (-1, 4, 4, 4, 4), (9 * 13 + 5, 1, 2, 3, 0.5), (MAX, 5, 5, 5, 5), (E + 9, 0, 0, 0, 0), (4, 7, 8, 9, 1.0),
                  (-MAX, 0, 0, 0, 0), (6, 1, 1, 1, 1.0), (E, 0, 0, 0, 0), (8, 2, 2, 2, 2.0), (E, 0, 0, 0, 0), (E, 0, 0, 0, 0), (E, 0, 0, 0, 0)])
    new = M.sigs([(4, 0, 0, 9, 3.0), (122, 0, 0, 0, 3.0), (12, 0, 0, 0, 3.0)])
    with _hot().SignatureTable.from_bytes(_image(13, rec)) as tab:
        U = _check(tab, rec, M.sigs([]))
        # k-mer 122 (home 5) sits at slot 2, in front of its home: the lookup cannot reach it, the export has it
        assert U["kmer"].tolist() == [4, 6, 8, 122]
        for policy in M.POLICIES:
            for entry in ("host", "device"):
                with tab.merge_signatures(_dev(new) if entry == "device" else new, on_conflict=policy) as u:
                    st = u.merge_stats()
                    assert (st["base"], st["base_ignored"], st["conflicts"], st["conflicts_same_function"], st["added"]) == (4, 3, 2, 1, 1)
                _check(tab, rec, new, policy=policy, entry=entry)
    # a stream shorter than num_sigs: only the resident records, the 7 whole ones of 7.5
    with _hot().SignatureTable.from_bytes(_image(13, rec)[:24 + 24 * 7 + 12]) as tab:
        U = _check(tab, rec[:7], new)
        assert U["kmer"].tolist() == [4, 12, 122]
    with _hot().SignatureTable.from_bytes(_image(13, rec)[:24]) as tab:
        assert len(_check(tab, rec[:0], new)) == 3
    # a stream longer than num_sigs: every resident record
    with _hot().SignatureTable.from_bytes(_image(5, rec)) as tab:
        assert len(_check(tab, rec, new)) == 5
    # a k-mer twice: the smallest such k-mer is named, after every error of the new signatures
    twice = rec.copy()
    twice[0], twice[4], twice[8], twice[10] = rec[9], rec[7], rec[9], rec[7]
    with _hot().SignatureTable.from_bytes(_image(13, twice)) as tab:
        for entry in ("host", "device"):
            e = _error(tab, twice, new, entry=entry)
            assert (e.kind, e.value) == ("dup_base", 6)
            e = _error(tab, twice, M.sigs([(3, 0, 0, 0, 1), (3, 0, 0, 0, 1)]), entry=entry)
            assert (e.kind, e.value) == ("dup_new", 3)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def test_errors_and_their_precedence(line_base):
    tab, stream = line_base
    N = _N()
    bad = M.sigs([(30_000, 0, 0, 0, 1), (30_000, 5, 0, 7, 1), (-1, 0, 0, 0, 1), (MAX, 0, 0, 9, 1), (20_000, 0, 0, 0, 1), (20_000, 0, 0, 0, 1)])
    m2 = np.zeros(2, dtype=np.int32)
    for entry in ("host", "device"):
        e = _error(tab, stream, bad, m2, m2, entry=entry)
        assert (e.kind, e.value) == ("kmer", 2)
        ok = bad[[0, 1, 4, 5]]
        e = _error(tab, stream, ok, m2, m2, entry=entry)
        assert (e.kind, e.value) == ("fn", 1)
        e = _error(tab, stream, ok, None, m2, entry=entry)
        assert (e.kind, e.value) == ("otu", 1)
        e = _error(tab, stream, ok, entry=entry)
        assert (e.kind, e.value) == ("dup_new", 20_000)
        e = _error(tab, stream, M.sigs([(1, 0, 0, 0, 1)]), np.zeros(0, dtype=np.int32), entry=entry)
        assert (e.kind, e.value) == ("fn", 0)
    with pytest.raises(N.KmerGutsNativeError) as ei:
        tab.merge_signatures(M.sigs([(5, 0, 0, 0, 1), (MAX + 5, 0, 0, 0, 1)]))
    assert "signature 1: k-mer %d is outside [0, 20^8) (the smallest such input index)" % (MAX + 5) in str(ei.value)
    # the argument errors come before everything else, the limit before the array is read
    lib = N.load()
    out = C.c_void_p(1)
    one = M.sigs([(-1, 0, 0, 0, 1)])
    p, pbad = N.KgMergeParams(0, 0), N.KgMergeParams(3, 0)
    call = lambda fn, *a: getattr(lib, fn)(*a, C.byref(out))
    h = tab._h
    assert call("kg_table_merge_signatures", None, C.byref(p), one.ctypes.data, 1, None, 0, None, 0) == N.KG_ERR_ARG and not out.value
    assert lib.kg_table_merge_signatures(h, C.byref(p), one.ctypes.data, 1, None, 0, None, 0, None) == N.KG_ERR_ARG
    assert call("kg_table_merge_signatures", h, None, one.ctypes.data, 1, None, 0, None, 0) == N.KG_ERR_ARG
    assert call("kg_table_merge_signatures", h, C.byref(pbad), one.ctypes.data, 1 << 32, None, 0, None, 0) == N.KG_ERR_ARG
    assert call("kg_table_merge_signatures", h, C.byref(N.KgMergeParams(0, 1)), one.ctypes.data, 1, None, 0, None, 0) == N.KG_ERR_ARG
    assert call("kg_table_merge_signatures", h, C.byref(p), one.ctypes.data, -1, None, 0, None, 0) == N.KG_ERR_ARG
    assert call("kg_table_merge_signatures", h, C.byref(p), None, 1, None, 0, None, 0) == N.KG_ERR_ARG
    d = _dev(np.concatenate([one, one]))
    assert call("kg_table_merge_signatures_device", h, C.byref(p), C.c_void_p(d.data_ptr() + 4), 1, None, 0, None, 0) == N.KG_ERR_ARG
    assert "8-byte aligned" in lib.kg_last_error().decode()
    assert call("kg_table_merge_signatures", h, C.byref(p), one.ctypes.data, 1 << 32, None, 0, None, 0) == N.KG_ERR_LIMIT
    assert call("kg_table_merge_signatures", h, C.byref(p), one.ctypes.data, 1, None, 0, None, 0) == N.KG_ERR_ARG       # the k-mer -1
    assert not out.value
    # a derived set has no merge statistics
    hot = _hot()
    with hot.derive_signatures(b"ACDEFGHIKLMNP" * 2, [0, 13, 26], [0, 0], [0, 0]) as s:
        with pytest.raises(N.KmerGutsNativeError) as ei:
            s.merge_stats()
        assert ei.value.code == N.KG_ERR_ARG
    with pytest.raises(ValueError):
        tab.merge_signatures(one, on_conflict="both")
    assert tab.live_device_bytes() == 0


# ---- 8. failed allocations ------------------------------------------------------------------------------------------------------
def _protein_queries(keys, n_seqs=30, per=20, seed=9):
    from kmergutsjava_amd import synth
    rng = np.random.default_rng(seed)
    seqs = ["".join(synth.decode_kmer(int(k)) for k in rng.choice(keys, size=per)) for _ in range(n_seqs)]
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return "".join(seqs).encode(), off


def _records(r):
    return r.hits().tobytes(), r.calls().tobytes(), r.otu().tobytes(), r.container_hit_start().tobytes()


@pytest.mark.parametrize("entry", ["host", "device"])
def test_failed_allocations_leave_the_base_as_it_was(monkeypatch, line_base, entry):
    tab, stream = line_base
    N, hot = _N(), _hot()
    new = _random_sigs(6000, 21, 0, 20_000, n_fn=3, n_otu=2)
    maps = (np.array([2, 0, 1], dtype=np.int32), np.array([1, 0], dtype=np.int32))
    arg = _dev(new) if entry == "device" else new
    seq, off = _protein_queries(stream["kmer"][stream["kmer"] < MAX])
    params = hot.Params(aa=True, min_hits=2)
    with tab.scan(seq, off, params) as r0:              # an open result: its blocks are the table's live bytes
        before, live = _records(r0), tab.live_device_bytes()
        assert live > 0 and r0.stats["n_hits"] > 0
        failed = 0
        for n in range(1, 40):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                with tab.merge_signatures(arg, *maps, "replace") as u:
                    got = u.numpy()
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert tab.live_device_bytes() == live, n
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= 8 and got.tobytes() == M.merge_numpy(stream, new, *maps, "replace")[0].tobytes()
        assert tab.live_device_bytes() == live
        with tab.scan(seq, off, params) as r1:
            assert _records(r1) == before
    assert tab.live_device_bytes() == 0


# ---- 9. mid-size ----------------------------------------------------------------------------------------------------------------
def test_mid_size_merge_builds_a_table_that_scans_like_the_synth_image(tmp_path):
    import torch
    from kmergutsjava_amd import synth
    hot = _hot()
    S = 1_000_003
    rec, placed, keys = synth.random_table(S, 0.5, 41)
    image = synth.table_image(rec)
    stream = M.records_of_image(image)[1]
    base_kmers = np.sort(stream["kmer"][(stream["kmer"] >= 0) & (stream["kmer"] < MAX)])
    assert len(base_kmers) == placed
    new = _random_sigs(72_000, 43, n_fn=1000, n_otu=64)
    new = new[~np.isin(new["kmer"], base_kmers)][:70_000]
    hit = _random_sigs(31_000, 44, n_fn=1000, n_otu=64)[:30_000]
    hit["kmer"] = np.random.default_rng(45).choice(base_kmers, size=30_000, replace=False)      # 30 % of the new ones are conflicts
    by_kmer = stream[np.argsort(stream["kmer"], kind="stable")]
    by_kmer = by_kmer[(by_kmer["kmer"] >= 0) & (by_kmer["kmer"] < MAX)]
    hit["functionIndex"][::3] = by_kmer["functionIndex"][np.searchsorted(base_kmers, hit["kmer"][::3])]   # a third name the same function
    new = np.concatenate([new, hit])
    assert len(new) == 100_000
    new = new[np.random.default_rng(46).permutation(len(new))]
    seq, off = _protein_queries(np.concatenate([base_kmers[:2000], new["kmer"][:2000]]), 40, 25)
    params = hot.Params(aa=True, min_hits=2)
    with hot.SignatureTable.from_bytes(image) as tab:
        for policy, entry in zip(M.POLICIES, ("device", "host", "device")):
            want, counts = M.merge_numpy(stream, new, None, None, policy)
            assert counts["conflicts"] == 30_000 and counts["conflicts_same_function"] >= 10_000
            with tab.merge_signatures(_dev(new) if entry == "device" else new, on_conflict=policy) as u:
                assert {k: u.merge_stats()[k] for k in M.COUNTS} == counts and u.numpy().tobytes() == want.tobytes()
                with hot.SignatureTable.build(u.device_tensor(), S) as built:
                    want_image, want_placed = M.place(want, S)
                    assert built.placed == want_placed and _saved(built, tmp_path) == want_image
                    with hot.SignatureTable.from_bytes(want_image) as ref, built.scan(seq, off, params) as r, ref.scan(seq, off, params) as r0:
                        assert _records(r) == _records(r0) and r.stats["n_hits"] > 0
        assert tab.live_device_bytes() == 0
    torch.cuda.synchronize()


# ---- 10. end to end -------------------------------------------------------------------------------------------------------------
def _protein(seed, n=70):
    rng = np.random.default_rng(seed)
    return "".join("ACDEFGHIKLMNPQRSTVWY"[i] for i in rng.integers(0, 20, n))


def _run(main, argv, capsys):
    capsys.readouterr()
    rc = main(argv)
    cap = capsys.readouterr()
    assert rc == 0, cap.err
    return cap.out.strip()


def test_end_to_end_two_annotated_sets_merged_and_scanned(tmp_path, capsys):
    from kmergutsjava_amd import build, make_signatures, make_table, merge_tables, synth, KmerGutsJava
    shared, only_a, only_b = _protein(1), _protein(2), _protein(3)
    sets = {"a": [("a1", shared, "shared enzyme", "genome A"), ("a2", shared, "shared enzyme", "genome A"),
                  ("a3", only_a, "base-only kinase", "genome A"), ("a4", only_a, "base-only kinase", "genome X")],
            "b": [("b1", shared[5:] + "ACDEF", "shared enzyme", "genome B"), ("b2", shared[5:] + "ACDEF", "shared enzyme", "genome B"),
                  ("b3", only_b, "new-only ligase", "genome A"), ("b4", only_b, "new-only ligase", "genome B")]}
    dirs = {}
    for name, prots in sets.items():
        (tmp_path / (name + ".faa")).write_text("".join(">%s\n%s\n" % (p[0], p[1]) for p in prots))
        (tmp_path / (name + ".tsv")).write_text("".join("%s\t%s\t%s\n" % (p[0], p[2], p[3]) for p in prots))
        dirs[name] = str(tmp_path / name)
        _run(make_signatures.main, ["-p", str(tmp_path / (name + ".faa")), "-A", str(tmp_path / (name + ".tsv")), "-o",
                                    str(tmp_path / (name + ".txt")), "-D", dirs[name]], capsys)
    out = str(tmp_path / "merged")
    line = _run(merge_tables.main, ["-D", dirs["a"], "--add", dirs["b"], "-o", out, "--on-conflict", "replace", "--sigs",
                                    str(tmp_path / "merged.txt")], capsys)
    # the model on the same files
    read = lambda d, f: open(os.path.join(d, f), "rb").read()
    fn_bytes, fn_map = merge_tables.unite_names(read(dirs["a"], "function.index"), read(dirs["b"], "function.index"))
    otu_bytes, otu_map = merge_tables.unite_names(read(dirs["a"], "otu.index"), read(dirs["b"], "otu.index"))
    assert fn_bytes == b"0\tbase-only kinase\n1\tshared enzyme\n2\tnew-only ligase\n" and fn_map.tolist() == [2, 1]
    assert otu_bytes == b"0\tgenome A\n1\tgenome X\n2\tgenome B\n" and otu_map.tolist() == [0, 2]
    base_slots, base_stream = M.records_of_image(read(dirs["a"], "kmer.table.mem_map"))
    new_sigs = M.merge_numpy(M.records_of_image(read(dirs["b"], "kmer.table.mem_map"))[1], M.sigs([]))[0]
    U, c = M.merge_numpy(base_stream, new_sigs, fn_map, otu_map, "replace")
    assert c["conflicts"] == c["conflicts_same_function"] == c["replaced"] > 0 and c["added"] > 0
    S = max(base_slots, make_table.default_num_sigs(len(U)))
    want_image, placed = M.place(U, S)
    assert line == ("Base: %d (ignored 0), new: %d, added: %d, conflicts: %d (same function: %d), replaced: %d, dropped: 0, merged: %d, "
                    "slots: %d, placed: %d, dropped at the end: %d" % (c["base"], len(new_sigs), c["added"], c["conflicts"], c["conflicts"],
                                                                      c["conflicts"], len(U), S, placed, len(U) - placed))
    assert read(out, "kmer.table.mem_map") == want_image
    assert read(out, "function.index") == fn_bytes and read(out, "function.index").startswith(read(dirs["a"], "function.index"))
    assert read(out, "otu.index") == otu_bytes
    assert make_table.parse_signatures(open(str(tmp_path / "merged.txt"), "rb").read()).tobytes() == U.tobytes()
    # both front ends print the same report on a contig back-translated from proteins of both sets
    (tmp_path / "q.fa").write_text(">contig\n%s\n" % synth.back_translate(only_a + shared + only_b))
    cli = build.build_cli()
    subprocess.run([cli, "-D", out, "-q", str(tmp_path / "q.fa"), "-o", str(tmp_path / "cli.txt")], check=True, stdout=subprocess.DEVNULL)
    KmerGutsJava.main(["-D", out, "-q", str(tmp_path / "q.fa"), "-o", str(tmp_path / "java.txt")])
    capsys.readouterr()
    report = (tmp_path / "cli.txt").read_text()
    assert report == (tmp_path / "java.txt").read_text()
    calls = [ln.split("\t") for ln in report.splitlines() if ln.startswith("CALL")]
    assert {"base-only kinase", "new-only ligase", "shared enzyme"} <= {c[5] for c in calls}
    # a dump of BASE fed to make_table with the same -s reproduces BASE's table
    _run(merge_tables.main, ["-D", dirs["a"], "--sigs", str(tmp_path / "dump.txt.gz")], capsys)
    _run(make_table.main, ["-i", str(tmp_path / "dump.txt.gz"), "-f", os.path.join(dirs["a"], "function.index"), "-D", str(tmp_path / "again"),
                           "-s", str(base_slots)], capsys)
    assert read(str(tmp_path / "again"), "kmer.table.mem_map") == read(dirs["a"], "kmer.table.mem_map")
