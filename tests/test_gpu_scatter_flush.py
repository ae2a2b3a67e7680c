"""The scatter pass's flush (kg_partition.hpp: part_scatter_kernel): a wave lists every group its lanes completed in a round and
copies them in one pass, a group's place in its region comes from the bucket's running entry count (written[]), and fill[] is
derived from that count at the end.  The cases are the smallest at which each of these can go wrong: one wave that owns all the
groups of a round, a list too short for them (KG_SCATTER_FLUSH_LIST), the protein kernel's 20-entry list, regions that fill up
(overflow list, fallback) and low-complexity blocks appended behind fill[].  Everything is byte-identical against the C oracle,
through the partitioned strategy (KG_PARTITION=1) on a table of 200 003 slots cut into 13 buckets (KG_PART_SHIFT=14)."""
import numpy as np
import pytest

from helpers import assert_same_records, plant

pytestmark = pytest.mark.gpu

NUM_SIGS = 200_003


@pytest.fixture(scope="module")
def hp():
    from kmergutsjava_amd import hotpath
    return hotpath


@pytest.fixture(scope="module")
def table():
    """(image, keys): 100 000 signatures, 7 functions, 5 OTUs."""
    from kmergutsjava_amd import synth
    keys = synth.random_keys(100_000, 7201)
    rec, _ = synth.build_table(keys, synth.payload_of(keys, 7202, n_otu=5, n_fn=7), NUM_SIGS)
    return synth.table_image(rec), keys.tolist()


@pytest.fixture(autouse=True)
def partitioned(monkeypatch):
    monkeypatch.setenv("KG_PARTITION", "1")
    monkeypatch.setenv("KG_PART_SHIFT", "14")
    monkeypatch.delenv("KG_SCATTER_FLUSH_LIST", raising=False)


def _offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return off


def _scan_and_compare(hp, ora, img, sb, off, what, aa=False, **kw):
    with hp.SignatureTable.from_bytes(img) as tab, tab.scan(sb, off, hp.Params(aa=aa, **kw)) as r:
        assert r.stats["partitioned"] == 1 and r.stats["fallback"] == 0 and r.stats["part_buckets"] == 13, (what, r.stats)
        assert_same_records(r, ora, what)
        return dict(r.stats)


@pytest.fixture(scope="module")
def short_contigs(oracle, table):
    """Contigs of one and two window blocks (192 forward positions a block), each alone and all three together: with one
    scatter workgroup a block is one wave's, and its 384 windows complete a group in most of the 13 buckets in one round."""
    from kmergutsjava_amd import synth
    img, keys = table
    cases = []
    for k, lens in enumerate(([215], [216], [407], [215, 216, 407])):
        off = _offsets(lens)
        sb = plant(synth.random_dna(int(off[-1]), 7210 + k).numpy().tobytes(), off, keys, every=37, start=0)
        cases.append((lens, sb, off, oracle.run(img, sb, off, lookup_mode=1, min_hits=2)))
    return cases


@pytest.mark.parametrize("flush_list", [None, "1", "3"])
def test_one_wave_owns_every_group(hp, table, short_contigs, monkeypatch, flush_list):
    """A single wave fills all 13 buckets and owns up to 13 groups of a round, several lanes two or more; with a list of one or
    three entries the same groups go in several passes (the owners left over read their group numbers again)."""
    img, _ = table
    monkeypatch.setenv("KG_PART_WGS", "1")
    if flush_list is not None:
        monkeypatch.setenv("KG_SCATTER_FLUSH_LIST", flush_list)
    for lens, sb, off, ora in short_contigs:
        _scan_and_compare(hp, ora, img, sb, off, "one wave %s list %s" % (lens, flush_list), min_hits=2)
    assert len(short_contigs[-1][3]["hits"]) > 10


def test_list_overflow_with_two_workgroups(hp, oracle, table, monkeypatch):
    """50 kbp on two workgroups, two list entries: waves of 32 share the buffers, every round leaves owners over."""
    from kmergutsjava_amd import synth
    img, keys = table
    off = _offsets([50_000])
    sb = plant(synth.random_dna(50_000, 7220).numpy().tobytes(), off, keys, every=37, start=0)
    ora = oracle.run(img, sb, off, lookup_mode=1, min_hits=2)
    monkeypatch.setenv("KG_PART_WGS", "2")
    monkeypatch.setenv("KG_SCATTER_FLUSH_LIST", "2")
    _scan_and_compare(hp, ora, img, sb, off, "50 kbp, list 2", min_hits=2)
    assert len(ora["hits"]) > 500


def test_protein_list_of_one(hp, oracle, table, monkeypatch):
    """part_scatter_kernel<true> (one row a block, 20 list entries in its 80-byte scratch): one window, one block and a
    window, many blocks; one list entry."""
    from kmergutsjava_amd import synth
    img, keys = table
    off = _offsets([9, 73, 20_000])
    sb = plant(synth.random_protein(int(off[-1]), 7230).numpy().tobytes(), off, keys, every=19, dna=False, start=0)
    ora = oracle.run(img, sb, off, aa=True, lookup_mode=1, min_hits=2)
    for flush_list in (None, "1"):
        if flush_list is not None:
            monkeypatch.setenv("KG_SCATTER_FLUSH_LIST", flush_list)
        _scan_and_compare(hp, ora, img, sb, off, "protein, list %s" % flush_list, aa=True, min_hits=2)
    assert len(ora["hits"]) > 500


def test_region_offsets_from_the_counter(hp, oracle, table, monkeypatch):
    """Regions a tenth of their usual size and a contig that repeats one 24-mer: the groups whose number is beyond cap / 16 go to
    the overflow list, fill[] stops at cap; with a list of one group the scan falls back to direct probing, records identical."""
    from kmergutsjava_amd import synth
    img, keys = table
    word = synth.back_translate(synth.decode_kmer(keys[5])).encode()
    rnd = synth.random_dna(60_000, 7240).numpy().tobytes()
    parts = [rnd[:30_000], word * 400, rnd[30_000:]]
    off = _offsets([len(p) for p in parts])
    sb = plant(b"".join(parts), off, keys, every=45)
    ora = oracle.run(img, sb, off, lookup_mode=1, min_hits=2)
    monkeypatch.setenv("KG_PART_SLACK", "10")
    for flush_list in (None, "1"):
        if flush_list is not None:
            monkeypatch.setenv("KG_SCATTER_FLUSH_LIST", flush_list)
        _scan_and_compare(hp, ora, img, sb, off, "overflow list, flush list %s" % flush_list, min_hits=2)
    monkeypatch.delenv("KG_SCATTER_FLUSH_LIST")
    monkeypatch.setenv("KG_PART_OVF_GROUPS", "1")
    with hp.SignatureTable.from_bytes(img) as tab, tab.scan(sb, off, hp.Params(min_hits=2)) as r:
        assert r.stats["fallback"] == 1 and r.stats["partitioned"] == 0, r.stats
        assert_same_records(r, ora, "fallback")


def test_low_complexity_behind_fill(hp, oracle, table):
    """A homopolymer after random sequence: its blocks are set aside, lowc_blocks_kernel appends their entries behind the fill[]
    the scatter pass wrote from its counters, and counts their query k-mers."""
    from kmergutsjava_amd import synth
    img, keys = table
    rnd = synth.random_dna(30_000, 7250).numpy().tobytes()
    parts = [rnd[:20_000] + b"A" * 5000 + rnd[20_000:], rnd[:217]]
    off = _offsets([len(p) for p in parts])
    sb = plant(b"".join(parts), off, keys, every=4001)
    ora = oracle.run(img, sb, off, lookup_mode=1, min_hits=2)
    st = _scan_and_compare(hp, ora, img, sb, off, "low complexity, counted", min_hits=2, counters=True)
    assert st["windows_valid"] == ora["windows_valid"]
    _scan_and_compare(hp, ora, img, sb, off, "low complexity", min_hits=2)
