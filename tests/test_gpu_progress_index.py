"""KG_F_PROGRESS on the partitioned strategy's byte home index: the index pass summarises the walks of the k-mers it rules
out (certain misses: home slot .. first empty slot), the verify and overflow passes note the rest, and a one-workgroup
kernel turns the misses' summaries into the slots their walks reach.  Every scan here is checked three ways: records equal
the plain scan's, progress() and hit_slots() equal the counting kernels' (KG_F_COUNTERS | KG_F_PROGRESS on the tags), and
the "Processed" lines / kmersFound / EOF equal the C oracle's literal merge-join (KGJ:959-1029)."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import plant

pytestmark = pytest.mark.gpu

MAX_ENCODED = 20 ** 8


def _lines(pr):
    return [(f, pr["found_upto"][f]) for f in range(1, 11) if pr["first_visited"][f] >= 0]


def _lo(n):
    """lo[k]: the smallest slot whose tenth (KGJ:1018, double arithmetic) is >= k."""
    out = []
    for k in range(11):
        s = max(0, -(-n * k // 10) - 3)
        while int(10.0 * ((s + 1) / n)) < k:
            s += 1
        out.append(s)
    return out


def _workload(seed, num_sigs, load, n_contigs, contig_len, dna=True):
    from kmergutsjava_amd import synth
    rec, placed, keys = synth.random_table(num_sigs, load, seed)
    img = synth.table_image(rec)
    if dna:
        seq, off = synth.dna_uniform_config(n_contigs, contig_len, seed + 1)
        sb = plant(seq.numpy().tobytes(), off, keys.tolist(), every=61)
    else:
        lens = np.full(n_contigs, contig_len, dtype=np.int64)
        off = synth.offsets_of(lens)
        sb = plant(synth.random_protein(int(off[-1]), seed + 1).numpy().tobytes(), off, keys.tolist(), every=23, dna=False)
    return img, sb, off, rec


def _three_way(oracle, img, sb, off, aa=False, stream_slots=None):
    from kmergutsjava_amd import hotpath
    ora = oracle.run(img, sb, off, aa=aa, lookup_mode=0, min_hits=2)
    P = lambda **kw: hotpath.Params(aa=aa, min_hits=2, **kw)      # noqa: E731
    with hotpath.SignatureTable.from_bytes(img) as tab:
        with tab.scan(sb, off, P()) as r0:
            plain = [r0.hits().tobytes(), r0.calls().tobytes(), r0.otu().tobytes(), r0.hit_events().tobytes(),
                     r0.container_tail_events().tobytes(), r0.container_hit_start().tobytes(), r0.container_call_start().tobytes()]
        with tab.scan(sb, off, P(counters=True, progress=True)) as r1:
            assert r1.stats["part_levels"] == 1
            old_pr, old_slots = r1.progress(), r1.hit_slots().copy()
        with tab.scan(sb, off, P(progress=True)) as r:
            st = r.stats
            assert st["partitioned"] == 1 and st["fallback"] == 0, st
            assert st["part_levels"] == 4, st
            assert st["windows_valid"] == -1 and st["slots_inspected"] == -1, st
            got = [r.hits().tobytes(), r.calls().tobytes(), r.otu().tobytes(), r.hit_events().tobytes(),
                   r.container_tail_events().tobytes(), r.container_hit_start().tobytes(), r.container_call_start().tobytes()]
            assert got == plain
            assert r.hits().tobytes() == ora["hits"].tobytes() and r.calls().tobytes() == ora["calls"].tobytes()
            assert np.array_equal(r.hit_slots(), old_slots)
            pr = r.progress()
            assert pr == old_pr, (pr, old_pr)
            assert _lines(pr) == ora["processed"], (pr, ora["processed"])
            assert pr["kmers_found"] == ora["kmers_found"]
            if stream_slots is not None:
                assert pr["stream_slots"] == stream_slots
            if ora["read_eof"]:
                assert pr["walk_ran_off"] == 1 or pr["first_beyond"] == pr["stream_slots"], pr
            elif ora["skip_failed_bytes"] >= 0:
                assert pr["walk_ran_off"] == 0 and 24 * (pr["first_beyond"] - (pr["last_visited"] + 1)) == ora["skip_failed_bytes"]
            else:
                assert pr["walk_ran_off"] == 0 and pr["first_beyond"] == -1
            if pr["first_beyond"] < 0:          # (lookup_ran_off also counts home slots behind the end of a short stream)
                assert bool(pr["walk_ran_off"]) == bool(st["lookup_ran_off"])
    return pr, ora


@pytest.mark.parametrize("case", [(31, 1009, 0.6, 5, 1500, True), (32, 50021, 0.9, 12, 4000, True), (33, 200003, 0.5, 40, 3000, False),
                                  (34, 3_000_017, 0.5, 30, 200_000, True)])
def test_progress_runs_on_the_byte_home_index(oracle, monkeypatch, case):
    """The workloads of test_gpu_progress.py: a KG_F_PROGRESS scan no longer leaves the byte home index."""
    seed, num_sigs, load, n, ln, dna = case
    img, sb, off, rec = _workload(seed, num_sigs, load, n, ln, dna)
    monkeypatch.setenv("KG_PARTITION", "1")
    pr, ora = _three_way(oracle, img, sb, off, aa=not dna, stream_slots=num_sigs)
    assert len(ora["processed"]) >= (9 if num_sigs < 1_000_000 else 5)


# ---- hand-made tables aimed at the new logic (protein queries: only the planted 8-mers are valid windows) ----

def _rec_table(num_sigs, load, seed):
    from kmergutsjava_amd import synth
    rec, placed, keys = synth.random_table(num_sigs, load, seed)
    return rec.numpy().copy()


def _key_of(rec, s):
    return (int(rec[s, 1]) << 32) | (int(rec[s, 0]) & 0xFFFFFFFF)


def _set(rec, s, key):
    """slot s holds `key` (negative: occupied, matches nothing; > 20^8: empty)."""
    key &= (1 << 64) - 1
    lo, hi = key & 0xFFFFFFFF, key >> 32
    rec[s, 0] = lo - (1 << 32) if lo >= (1 << 31) else lo
    rec[s, 1] = hi - (1 << 32) if hi >= (1 << 31) else hi
    rec[s, 2:5] = (s % 64, s % 500, s % 1000)
    rec[s, 5] = np.float32(1.0).view(np.int32)


NEG = -12345
EMPTY = MAX_ENCODED + 1


def _miss_value(rec, n, home, salt=0):
    """a k-mer value homed at `home` that the table does not hold"""
    keys = set(_key_of(rec, s) for s in range(max(0, home - 64), min(len(rec), home + 2048)))
    q = 7 + salt
    while True:
        v = q * n + home
        assert v < MAX_ENCODED
        if v not in keys:
            return v
        q += 1


def _protein(values, seps=1):
    from kmergutsjava_amd import synth
    return "".join(synth.decode_kmer(v) + "X" * seps for v in values)


def _query(seqs):
    sb = "".join(seqs).encode()
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return sb, off


def _hits_from(rec, count, seed):
    rng = np.random.default_rng(seed)
    occ = [s for s in range(len(rec)) if 0 <= _key_of(rec, s) <= MAX_ENCODED]
    return [_key_of(rec, int(s)) for s in rng.choice(occ, size=min(count, len(occ)), replace=False)]


def _image(rec, num_sigs=None):
    from kmergutsjava_amd import synth
    import torch
    return synth.table_image(torch.from_numpy(rec), num_sigs)


def test_tiny_dense_table_buckets_span_tenths(oracle, monkeypatch):
    """load 0.9, ~1000 slots: buckets of 2^7 slots against tenths of ~100 (the per-entry segment notes)."""
    monkeypatch.setenv("KG_PARTITION", "1")
    img, sb, off, rec = _workload(61, 1013, 0.9, 4, 3000, True)
    _three_way(oracle, img, sb, off, stream_slots=1013)
    # protein: queries only where planted, misses at every slot
    r = _rec_table(1013, 0.9, 62)
    vals = [_miss_value(r, 1013, h) for h in range(0, 1013, 3)] + _hits_from(r, 40, 63)
    sb, off = _query([_protein(vals[i::4]) for i in range(4)])
    _three_way(oracle, _image(r), sb, off, aa=True, stream_slots=1013)


@pytest.mark.parametrize("variant", ["crosses", "empty_at_lo", "ends_below_lo"])
def test_misses_just_below_a_tenth_boundary(oracle, monkeypatch, variant):
    """A miss homed at lo[k] - 5 inside an occupied run (negative keys): the run crosses lo[k] (the walk reaches tenth k),
    ends with an empty record AT lo[k] (read: reached), or ends at lo[k] - 1 (not reached)."""
    monkeypatch.setenv("KG_PARTITION", "1")
    n = 50021
    rec = _rec_table(n, 0.4, 71)
    lo = _lo(n)
    vals = []
    for k in range(1, 10):
        for s in range(lo[k] - 8, lo[k] + 3):
            _set(rec, s, NEG)
        if variant == "empty_at_lo":
            _set(rec, lo[k], EMPTY)
        elif variant == "ends_below_lo":
            _set(rec, lo[k] - 1, EMPTY)
        _set(rec, lo[k] - 9, EMPTY)
        vals.append(_miss_value(rec, n, lo[k] - 5))
    vals += _hits_from(rec, 30, 72)
    sb, off = _query([_protein(vals)])
    pr, ora = _three_way(oracle, _image(rec), sb, off, aa=True, stream_slots=n)
    reached = [pr["first_visited"][k] == lo[k] for k in range(1, 10)]
    assert all(reached) if variant != "ends_below_lo" else not any(reached), (variant, pr["first_visited"], lo)


def test_long_runs_and_a_run_at_the_end_of_the_stream(oracle, monkeypatch):
    """An occupied run of 1500 slots (index code 255: every query homed there is walked) with real keys deep inside it and
    misses along it, and an occupied run up to the last record (a miss there walks off the stream: walk_ran_off)."""
    monkeypatch.setenv("KG_PARTITION", "1")
    n = 50021
    rec = _rec_table(n, 0.5, 81)
    a = 20000
    _set(rec, a - 1, EMPTY)
    for s in range(a, a + 1500):
        _set(rec, s, NEG)
    _set(rec, a + 1500, EMPTY)
    deep = [(a + 10 + 7 * n, a + 1200), (a + 600 + 3 * n, a + 1450)]   # (key, slot): homed early in the run, stored late
    for key, s in deep:
        _set(rec, s, key)
    for s in range(n - 40, n):
        _set(rec, s, NEG)
    _set(rec, n - 41, EMPTY)
    vals = [key for key, _ in deep] + [_miss_value(rec, n, h) for h in (a + 5, a + 700, a + 1499, n - 20)]
    vals += _hits_from(rec, 30, 82)
    sb, off = _query([_protein(vals[:3]), _protein(vals[3:])])
    pr, ora = _three_way(oracle, _image(rec), sb, off, aa=True, stream_slots=n)
    assert pr["walk_ran_off"] == 1 and pr["last_visited"] == n - 1 and ora["read_eof"]


@pytest.mark.parametrize("gz", [False, True])
def test_short_and_long_table_streams(oracle, monkeypatch, tmp_path, gz):
    """A table file cut short of numSigs records (plain and .gz: first_beyond, EOF inside a walk) and one longer than numSigs."""
    from kmergutsjava_amd import hotpath
    monkeypatch.setenv("KG_PARTITION", "1")
    img, sb, off, rec = _workload(91, 50021, 0.5, 8, 5000)
    for cut in (40000, 25013, 12000):
        short = img[:24 + 24 * cut]
        if not gz:
            _three_way(oracle, short, sb, off, stream_slots=cut)
            continue
        # the .gz image through kg_table_open against the plain image's scan
        path = tmp_path / ("t%d.gz" % cut)
        path.write_bytes(gzip.compress(short))
        P = lambda **kw: hotpath.Params(min_hits=2, **kw)      # noqa: E731
        with hotpath.SignatureTable.open(str(path)) as tab:
            with tab.scan(sb, off, P(progress=True)) as r, tab.scan(sb, off, P(progress=True, counters=True)) as rc:
                assert r.stats["part_levels"] == 4 and rc.stats["part_levels"] == 1
                assert r.hits().tobytes() == rc.hits().tobytes() and r.progress() == rc.progress()
                assert np.array_equal(r.hit_slots(), rc.hit_slots()) and r.progress()["stream_slots"] == cut
                assert _lines(r.progress()) == oracle.run(short, sb, off, lookup_mode=0, min_hits=2)["processed"]
    if not gz:
        from kmergutsjava_amd import synth
        rec2 = synth.random_table(50021 + 700, 0.5, 92)[0]
        long_img = synth.table_image(rec2, 50021)
        _three_way(oracle, long_img, sb, off)


def test_low_complexity_contig_through_overflow_groups(oracle, monkeypatch):
    """Homopolymer and tandem-repeat contigs: thousands of entries of one home slot overflow their regions (overflow groups)."""
    monkeypatch.setenv("KG_PARTITION", "1")
    from kmergutsjava_amd import synth
    rec, placed, keys = synth.random_table(200003, 0.5, 101)
    img = synth.table_image(rec)
    seq, off = synth.dna_uniform_config(6, 6000, 102)
    sb = plant(seq.numpy().tobytes(), off, keys.tolist(), every=61)
    word = synth.back_translate(synth.decode_kmer(int(keys[5])))
    extra = ["A" * 60000, word * 2500, "ACG" * 20000]
    sb = sb + "".join(extra).encode()
    off = np.concatenate([off, off[-1] + np.cumsum([len(x) for x in extra])])
    _three_way(oracle, img, sb, off, stream_slots=200003)


# ---- front ends: one scan per batch, report and info lines ----

def _info_lines(text):
    return [re.sub(r"time=\d+ ms\.", "time=0 ms.", ln) for ln in text.splitlines()
            if ln.startswith(("Processed: ", "Error: ", "Kmers found: "))]


def test_front_ends_one_scan_with_duplicate_ids_and_batches(tmp_path):
    from kmergutsjava_amd import synth, build, KmerGutsJava
    from oracle import kgj_model as M
    rec, placed, keys = synth.random_table(50021, 0.5, 111)
    img = synth.table_image(rec)
    seq, off = synth.dna_uniform_config(7, 4000, 112)
    sb = plant(seq.numpy().tobytes(), off, keys.tolist(), every=61)
    names = ["c0", "c1", "c0", "c2", "c1", "c3", "c0"]           # shadowed records: scanned, not reported
    fa = "".join(">%s\n%s\n" % (names[k], sb[off[k]:off[k + 1]].decode()) for k in range(len(off) - 1))
    (tmp_path / "q.fa").write_text(fa)
    fn = ["function %d" % i for i in range(1000)]
    d = tmp_path / "data"
    synth.write_data_dir(str(d), img, 1000)
    m = M.Model(min_hits=2, debug=True)
    m.run(img, fn, fa)
    want = [ln for ln in m.info_lines if ln.startswith(("Processed: ", "Error: "))]
    assert sum(ln.startswith("Processed: ") for ln in want) >= 9
    cli = build.build_cli()
    args = ["-D", str(d), "-q", str(tmp_path / "q.fa"), "-m", "2"]
    plain = subprocess.run([cli] + args, check=True, capture_output=True, text=True).stdout       # stdout: records only
    assert plain.count("OTU-COUNTS") == 4 and "Processed" not in plain
    for batch in (None, "9000", "4500"):
        env = dict(os.environ)
        if batch:
            env["KG_CLI_BATCH_CHARS"] = batch
        out = subprocess.run([cli] + args + ["-o", str(tmp_path / "cli.txt")], check=True, capture_output=True, text=True, env=env).stdout
        assert _info_lines(out) == want, (batch, out)
        assert (tmp_path / "cli.txt").read_text() == plain, batch
        keep = KmerGutsJava.MAX_BATCH_CHARS
        try:
            if batch:
                KmerGutsJava.MAX_BATCH_CHARS = int(batch)
            KmerGutsJava.main(args + ["-o", str(tmp_path / "py.txt")])
        finally:
            KmerGutsJava.MAX_BATCH_CHARS = keep
        assert (tmp_path / "py.txt").read_text() == plain, batch
