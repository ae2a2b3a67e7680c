"""The scan's records do not depend on launch geometry (include/kmerguts_hip.h).  Every geometry knob of the partitioned
pipeline and of the direct kernel is swept over its smallest legal value, odd values, its default and a large value, on
small inputs where a small grid makes every workgroup take many tickets / grid-stride steps.  Every scan must equal the C
oracle record for record; progress scans must equal the default geometry's progress() and hit_slots(); where the scan
reports a knob's effect (part_shift, part_chunks, part_buckets) it must show.  Out-of-range values (0, below the
minimum, beyond 2^32) are held to a legal geometry by the library and give the same records."""
import numpy as np
import pytest

from helpers import assert_same_records, plant

pytestmark = pytest.mark.gpu

MAX_ENCODED = 20 ** 8

# every knob the sweep touches: cleared before each test so that the runner's environment cannot leak in
KNOBS = ("KG_PARTITION", "KG_BIDX", "KG_PROBE_GRID", "KG_INDEX_GRID", "KG_VERIFY_GRID", "KG_LOWC_GRID", "KG_OVF_GRID",
         "KG_ORDER_GRID", "KG_PART_WGS", "KG_PROBE_GRAB", "KG_PART_SHIFT", "KG_PART_TAPER", "KG_EARLY_TOTALS",
         "KG_ORDER_STREAMS", "KG_SCATTER_PRIO", "KG_INDEX_PRIO", "KG_VERIFY_PRIO", "KG_PART_CHUNKS", "KG_PART_MIN_CHUNK_BLOCKS",
         "KG_SCAN_GRID", "KG_STAGE_CHUNK", "KG_SCAN_RPG", "KG_DIRECT_FILTER", "KG_PART_SLACK", "KG_PART_OVF_GROUPS",
         "KG_INDEX_R", "KG_TEST_TINY_LISTS")

GRAB_UNIT = 256 * 4          # 256 x max(kProbeN, kIndexN) (kg_partition.hpp)

# knob -> values: smallest legal, odd / not a power of two, default, large
SWEEP = {
    "KG_PROBE_GRID": ["8", "24", "2048", "8192"],
    "KG_INDEX_GRID": ["8", "24", "1024", "8192"],
    "KG_VERIFY_GRID": ["1", "24", "512", "8192"],
    "KG_LOWC_GRID": ["1", "24", "256", "8192"],
    "KG_OVF_GRID": ["1", "24", "256", "8192"],
    "KG_ORDER_GRID": ["1", "24", "768", "8192"],
    "KG_PART_WGS": ["1", "3", "7", "256"],
    "KG_PROBE_GRAB": [str(GRAB_UNIT), str(3 * GRAB_UNIT), str(16 * GRAB_UNIT), str(1 << 24)],
    "KG_PART_SHIFT": ["4", "9", "21", "31"],
    "KG_PART_TAPER": ["10,90", "70,20,10", "0,100", "30,30,25,15"],
    "KG_SCATTER_PRIO": ["0", "3"],
    "KG_INDEX_PRIO": ["0", "3"],
    "KG_VERIFY_PRIO": ["0", "3"],
}

# 0, below the minimum, beyond 2^32 (strtol's long), and 2^32 - 1
OUT_OF_RANGE = {
    "KG_PROBE_GRID": ["0", "1", "7", "13", "99999999999", "4294967295"],
    "KG_INDEX_GRID": ["0", "1", "7", "13", "99999999999", "4294967295"],
    "KG_VERIFY_GRID": ["0", "99999999999", "4294967295"],
    "KG_LOWC_GRID": ["0", "99999999999", "4294967295"],
    "KG_OVF_GRID": ["0", "99999999999", "4294967295"],
    "KG_ORDER_GRID": ["0", "99999999999", "4294967295"],
    "KG_PART_WGS": ["0", "99999999999", "4294967295"],
    "KG_PROBE_GRAB": ["0", "1", "1023", "99999999999", "4294967295"],
    "KG_PART_SHIFT": ["0", "3", "32", "40", "99999999999", "4294967295"],
    "KG_SCATTER_PRIO": ["4", "99999999999"],
    "KG_INDEX_PRIO": ["4", "99999999999"],
    "KG_VERIFY_PRIO": ["4", "99999999999"],
    "KG_ORDER_STREAMS": ["5", "99999999999"],
}
OUT_OF_RANGE_DIRECT = {
    "KG_SCAN_GRID": ["0", "99999999999", "4294967295"],
    "KG_STAGE_CHUNK": ["0", "99999999999", "4294967295"],
    "KG_SCAN_RPG": ["0", "4", "99999999999"],
}


def _clamp(v, lo, hi, mult=1):
    """kg_host.hpp env_knob"""
    x = min(hi, max(lo, int(v)))
    return (x + mult - 1) // mult * mult


def _expected_shift(start, num_sigs, limit, aa):
    """the partitioned scan's bucket shift (kg_host_plan.hpp, plan_partition) from KG_PART_SHIFT = start"""
    shift = _clamp(start, 4, 31)
    qmax = MAX_ENCODED // num_sigs + 1
    while shift > 4 and qmax >= (1 << (32 - shift)):
        shift -= 1
    while ((limit + (1 << shift) - 1) >> shift) > 1024:
        shift += 1
    enc = 720 * 16 + 512 if aa else 80 * 16 + 256
    while enc + ((limit + (1 << shift) - 1) >> shift) * 140 > 160 * 1024:
        shift += 1
    return shift


def _expected_chunks(taper, ibase):
    """chunks of a KG_PART_TAPER scan: cuts at the first sequence start at or behind each cumulative share"""
    vals = [float(x) for x in taper.split(",")]
    cum = list(np.cumsum(vals))
    acc = cum[-1]
    nblocks = int(ibase[-1])
    if not (2 <= len(cum) <= 8 and acc > 0):
        return None
    cum = [x / acc for x in cum]
    clo = [0]
    for c in range(1, len(cum)):
        target = int(nblocks * cum[c - 1])
        cut = int(ibase[int(np.searchsorted(ibase, target, side="left"))])
        if clo[-1] < cut < nblocks:
            clo.append(cut)
    return len(clo)


def _ibase(off, aa):
    L = np.asarray(off[1:] - off[:-1], dtype=np.int64)
    nb = (np.maximum(L - 8, 0) + 63) // 64 if aa else (np.maximum(L - 23, 0) + 191) // 192
    ib = np.zeros(len(L) + 1, dtype=np.int64)
    np.cumsum(nb, out=ib[1:])
    return ib


class _W:
    def __init__(self, name, img, sb, off, aa, num_sigs, limit, ora):
        self.name, self.img, self.sb, self.off, self.aa = name, img, sb, off, aa
        self.num_sigs, self.limit, self.ora = num_sigs, limit, ora
        self.ibase = _ibase(off, aa)


@pytest.fixture(scope="module")
def workloads(oracle):
    """DNA against a table of seven buckets (with low-complexity contigs that fill overflow groups), the same queries
    against the table's first 8000 records (one bucket), and proteins (-a)."""
    from kmergutsjava_amd import synth
    rng = np.random.default_rng(5)
    out = {}
    P = dict(lookup_mode=0, min_hits=2)

    def batch(dense_seq, dense_off, keys, dna, ragged, extra):
        """dense contigs of signature k-mers (CALLs), ragged random sequences with planted k-mers, low-complexity runs"""
        gen = synth.random_dna if dna else synth.random_protein
        roff = synth.offsets_of(np.asarray(ragged, dtype=np.int64))
        rsb = plant(gen(int(roff[-1]), 302).numpy().tobytes(), roff, keys.tolist()[::7], every=47 if dna else 19, dna=dna,
                    start=0)
        sb = dense_seq.numpy().tobytes()
        lens = list(np.diff(dense_off))
        parts, out_lens = [], []
        for k in range(max(len(lens), len(ragged))):          # interleaved: every chunk holds some of each
            if k < len(lens):
                parts.append(sb[dense_off[k]:dense_off[k + 1]]); out_lens.append(lens[k])
            if k < len(ragged):
                parts.append(rsb[roff[k]:roff[k + 1]]); out_lens.append(ragged[k])
        parts += [x.encode() for x in extra]
        out_lens += [len(x) for x in extra]
        return b"".join(parts), synth.offsets_of(np.asarray(out_lens, dtype=np.int64))

    S = 50021
    seq, doff, rec, keys = synth.high_density_config(16, 60, S, 20000, seed=301)
    img = synth.table_image(rec)
    word = synth.back_translate(synth.decode_kmer(int(keys[3])))
    sb, off = batch(seq, doff, keys, True, list(rng.choice([24, 191, 192, 193, 900, 3000], size=20)),
                    ["A" * 9000, word * 300, "ACG" * 3000, "AT" * 2500])
    out["dna"] = _W("dna", img, sb, off, False, S, S, oracle.run(img, sb, off, **P))
    short = img[:24 + 24 * 8000]
    out["dna_one_bucket"] = _W("dna_one_bucket", short, sb, off, False, S, 8000, oracle.run(short, sb, off, **P))
    S2 = 200003
    seq2, doff2, rec2, keys2 = synth.high_density_config(24, 120, S2, 60000, seed=303, dna=False)
    img2 = synth.table_image(rec2)
    psb, poff = batch(seq2, doff2, keys2, False, list(rng.choice([8, 9, 71, 72, 73, 640, 2000], size=30)),
                      ["K" * 3000, synth.decode_kmer(int(keys2[5])) * 200])
    out["aa"] = _W("aa", img2, psb, poff, True, S2, S2, oracle.run(img2, psb, poff, aa=True, **P))
    for w in out.values():
        assert len(w.ora["hits"]) > 200 and len(w.ora["calls"]) > 20, w.name
    return out


@pytest.fixture(scope="module")
def tables(workloads):
    from kmergutsjava_amd import hotpath
    tabs = {k: hotpath.SignatureTable.from_bytes(w.img) for k, w in workloads.items()}
    yield tabs
    for t in tabs.values():
        t.close()


@pytest.fixture
def env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _params(w, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.Params(aa=w.aa, min_hits=2, **kw)


def _scan_check(tab, w, what, progress=False, counters=False):
    """one scan checked against the oracle; returns (stats, progress summary or None, hit slots or None)"""
    with tab.scan(w.sb, w.off, _params(w, progress=progress, counters=counters)) as r:
        assert_same_records(r, w.ora, "%s %s" % (w.name, what))
        pr = r.progress() if progress else None
        slots = r.hit_slots().copy() if progress else None
        return dict(r.stats), pr, slots


BASES = {"one_chunk": {}, "four_chunks": {"KG_PART_CHUNKS": "4", "KG_PART_MIN_CHUNK_BLOCKS": "1"}}


def _set(env, d):
    for k, v in d.items():
        env.setenv(k, v)


@pytest.fixture(scope="module")
def default_progress(workloads, tables):
    """progress() and hit_slots() of the default geometry (one chunk and four), per workload and tag-pass source"""
    import os
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    out = {}
    try:
        os.environ["KG_PARTITION"] = "1"
        for name, w in workloads.items():
            for base, bd in BASES.items():
                for bidx in ("0", "1"):
                    os.environ["KG_BIDX"] = bidx
                    os.environ.update(bd)
                    st, pr, slots = _scan_check(tables[name], w, "default progress", progress=True)
                    for k in bd:
                        del os.environ[k]
                    out[name, base, bidx] = (pr, slots)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(saved)
    return out


def _check_effect(knob, value, w, st, base):
    assert st["partitioned"] == 1 and st["fallback"] == 0, (knob, value, w.name, st)
    if knob == "KG_PART_SHIFT":
        assert st["part_shift"] == _expected_shift(value, w.num_sigs, w.limit, w.aa), (value, w.name, st["part_shift"])
        assert st["part_buckets"] == (w.limit + (1 << st["part_shift"]) - 1) >> st["part_shift"]
    elif knob == "KG_PART_TAPER":
        assert st["part_chunks"] == _expected_chunks(value, w.ibase), (value, w.name, st["part_chunks"])
    elif base == "four_chunks":
        assert st["part_chunks"] >= 3, (knob, value, w.name, st["part_chunks"])
    else:
        assert st["part_chunks"] == 1
    if w.name == "dna_one_bucket" and knob != "KG_PART_SHIFT":
        assert st["part_buckets"] == 1


@pytest.mark.parametrize("knob", sorted(SWEEP))
def test_partitioned_knob_sweep(env, workloads, tables, default_progress, knob):
    """Each knob at each of its values, on every workload, on the byte home index and on the tags, in one chunk and in
    three or more; a progress scan per value (equal to the default geometry's) and one KG_F_COUNTERS scan."""
    env.setenv("KG_PARTITION", "1")
    for value in SWEEP[knob]:
        env.setenv(knob, value)
        for name, w in workloads.items():
            for base, bd in BASES.items():
                _set(env, bd)
                for bidx in ("1", "0"):
                    env.setenv("KG_BIDX", bidx)
                    what = "%s=%s %s bidx=%s" % (knob, value, base, bidx)
                    st, _, _ = _scan_check(tables[name], w, what)
                    _check_effect(knob, value, w, st, base)
                    assert st["part_levels"] == (4 if bidx == "1" else 1), what
                    st, pr, slots = _scan_check(tables[name], w, what + " progress", progress=True)
                    _check_effect(knob, value, w, st, base)
                    want_pr, want_slots = default_progress[name, base, bidx]
                    assert pr == want_pr, (what, pr, want_pr)
                    assert np.array_equal(slots, want_slots), what
                st, _, _ = _scan_check(tables[name], w, "%s=%s %s counters" % (knob, value, base), counters=True)
                _check_effect(knob, value, w, st, base)
                assert st["part_levels"] == 1 and st["windows_valid"] >= 0
                for k in bd:
                    env.delenv(k)


@pytest.mark.parametrize("order_streams", ["0", "2"])
def test_early_totals_off(env, workloads, tables, default_progress, order_streams):
    """KG_EARLY_TOTALS=0 (the totals after the whole ordering) with the orderings on stream 3 or on two streams of their own."""
    env.setenv("KG_PARTITION", "1")
    env.setenv("KG_EARLY_TOTALS", "0")
    env.setenv("KG_ORDER_STREAMS", order_streams)
    for name, w in workloads.items():
        for base, bd in BASES.items():
            _set(env, bd)
            for bidx in ("1", "0"):
                env.setenv("KG_BIDX", bidx)
                what = "early totals off, %s order streams, %s bidx=%s" % (order_streams, base, bidx)
                st, _, _ = _scan_check(tables[name], w, what)
                _check_effect("KG_EARLY_TOTALS", "0", w, st, base)
                st, pr, slots = _scan_check(tables[name], w, what + " progress", progress=True)
                assert (pr, slots.tobytes()) == (default_progress[name, base, bidx][0], default_progress[name, base, bidx][1].tobytes())
            for k in bd:
                env.delenv(k)


ALL_MIN = [
    {"KG_PROBE_GRID": "8", "KG_INDEX_GRID": "8", "KG_VERIFY_GRID": "1", "KG_LOWC_GRID": "1", "KG_OVF_GRID": "1",
     "KG_ORDER_GRID": "1", "KG_PART_WGS": "1", "KG_PROBE_GRAB": str(GRAB_UNIT)},
    {"KG_PROBE_GRID": "8", "KG_INDEX_GRID": "8", "KG_VERIFY_GRID": "8", "KG_LOWC_GRID": "8", "KG_OVF_GRID": "8",
     "KG_ORDER_GRID": "8", "KG_PART_WGS": "3"},
    {"KG_PROBE_GRID": "8", "KG_INDEX_GRID": "8", "KG_VERIFY_GRID": "1", "KG_LOWC_GRID": "1", "KG_OVF_GRID": "1",
     "KG_ORDER_GRID": "1", "KG_PART_WGS": "1", "KG_PART_SHIFT": "4", "KG_EARLY_TOTALS": "0", "KG_ORDER_STREAMS": "2"},
    {"KG_PROBE_GRID": "8", "KG_INDEX_GRID": "8", "KG_VERIFY_GRID": "1", "KG_LOWC_GRID": "1", "KG_OVF_GRID": "1",
     "KG_ORDER_GRID": "1", "KG_PART_WGS": "7", "KG_PART_TAPER": "70,20,10", "KG_SCATTER_PRIO": "0", "KG_INDEX_PRIO": "3",
     "KG_VERIFY_PRIO": "3"},
]


@pytest.mark.parametrize("combo", range(len(ALL_MIN)))
def test_every_grid_at_its_minimum(env, workloads, tables, default_progress, combo):
    env.setenv("KG_PARTITION", "1")
    _set(env, ALL_MIN[combo])
    for name, w in workloads.items():
        for base, bd in BASES.items():
            _set(env, bd)
            for bidx in ("1", "0"):
                env.setenv("KG_BIDX", bidx)
                what = "all minimum #%d %s bidx=%s" % (combo, base, bidx)
                st, _, _ = _scan_check(tables[name], w, what)
                assert st["partitioned"] == 1 and st["fallback"] == 0, (what, st)
                if "KG_PART_TAPER" not in ALL_MIN[combo]:
                    assert st["part_chunks"] == 1 if base == "one_chunk" else st["part_chunks"] >= 3, (what, st["part_chunks"])
                st, pr, slots = _scan_check(tables[name], w, what + " progress", progress=True)
                if "KG_PART_TAPER" not in ALL_MIN[combo]:
                    want_pr, want_slots = default_progress[name, base, bidx]
                    assert pr == want_pr and np.array_equal(slots, want_slots), what
            _scan_check(tables[name], w, "all minimum #%d %s counters" % (combo, base), counters=True)
            for k in bd:
                env.delenv(k)


def test_direct_kernel_geometry(env, workloads, tables):
    """KG_SCAN_GRID x KG_STAGE_CHUNK x KG_SCAN_RPG x KG_DIRECT_FILTER on the direct kernel (KG_PARTITION=0)."""
    env.setenv("KG_PARTITION", "0")
    for grid in ("8", "24", "2048"):
        for chunk in ("1", "64", "256"):
            for filt in ("0", "2"):
                env.setenv("KG_SCAN_GRID", grid)
                env.setenv("KG_STAGE_CHUNK", chunk)
                env.setenv("KG_DIRECT_FILTER", filt)
                for name, w in workloads.items():
                    for rpg in (("1", "2", "3", "6") if not w.aa else ("1",)):
                        env.setenv("KG_SCAN_RPG", rpg)
                        what = "grid %s stage chunk %s rpg %s filter %s" % (grid, chunk, rpg, filt)
                        st, _, _ = _scan_check(tables[name], w, what)
                        assert st["partitioned"] == 0, what
                    if name == "dna":
                        _scan_check(tables[name], w, what + " progress", progress=True)
                        _scan_check(tables[name], w, what + " counters", counters=True)


@pytest.mark.parametrize("knob", sorted(OUT_OF_RANGE))
def test_out_of_range_partitioned_knobs(env, workloads, tables, knob):
    """0, a value below the minimum and huge values: a legal geometry, the partitioned path, the oracle's records (before
    the clamp: empty launches of the ticketed grids, a division by zero on the host, a wrapped shift that sent the scan
    to the direct path, and a grab size that wrapped round to 0)."""
    env.setenv("KG_PARTITION", "1")
    for value in OUT_OF_RANGE[knob]:
        env.setenv(knob, value)
        for name, w in workloads.items():
            for bidx in ("1", "0"):
                env.setenv("KG_BIDX", bidx)
                for base, bd in BASES.items():
                    _set(env, bd)
                    what = "%s=%s %s bidx=%s" % (knob, value, base, bidx)
                    st, _, _ = _scan_check(tables[name], w, what)
                    assert st["partitioned"] == 1 and st["fallback"] == 0, (what, st)
                    if knob == "KG_PART_SHIFT":
                        assert 4 <= st["part_shift"] <= 31
                        assert st["part_shift"] == _expected_shift(value, w.num_sigs, w.limit, w.aa), what
                    for k in bd:
                        env.delenv(k)


@pytest.mark.parametrize("knob", sorted(OUT_OF_RANGE_DIRECT))
def test_out_of_range_direct_knobs(env, workloads, tables, knob):
    env.setenv("KG_PARTITION", "0")
    for value in OUT_OF_RANGE_DIRECT[knob]:
        env.setenv(knob, value)
        for name, w in workloads.items():
            for filt in ("0", "2"):
                env.setenv("KG_DIRECT_FILTER", filt)
                st, _, _ = _scan_check(tables[name], w, "%s=%s filter %s" % (knob, value, filt))
                assert st["partitioned"] == 0
        _scan_check(tables["dna"], workloads["dna"], "%s=%s progress" % (knob, value), progress=True)
