"""The scatter pass's instantiations and reshaped branches (kg_partition.hpp: part_scatter_kernel<AA, SHORT, PROG>, its cold
paths behind the per-chunk parameter block, lowc_blocks_kernel) and the CALL pass (kg_aggregate.hpp: calls_wave_kernel), at the
smallest shapes where each can go wrong.  Everything is byte-identical against the C oracle, through the partitioned strategy
(KG_PARTITION=1) on a table of 200 003 slots cut into 13 buckets (KG_PART_SHIFT=14)."""
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
    keys = synth.random_keys(100_000, 7101)
    rec, _ = synth.build_table(keys, synth.payload_of(keys, 7102, n_otu=5, n_fn=7), NUM_SIGS)
    return synth.table_image(rec), keys.tolist()


@pytest.fixture(autouse=True)
def partitioned(monkeypatch):
    monkeypatch.setenv("KG_PARTITION", "1")
    monkeypatch.setenv("KG_PART_SHIFT", "14")


def _offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return off


def _dna_blocks(lens):
    return int(sum((max(n - 23, 0) + 191) // 192 for n in lens))


def _scan_and_compare(hp, oracle, img, sb, off, what, aa=False, **kw):
    ora = oracle.run(img, sb, off, aa=aa, lookup_mode=1, **kw)
    with hp.SignatureTable.from_bytes(img) as tab, tab.scan(sb, off, hp.Params(aa=aa, **kw)) as r:
        assert r.stats["partitioned"] == 1 and r.stats["part_buckets"] >= 8, r.stats
        assert_same_records(r, ora, what)
        return ora, dict(r.stats)


def test_block_and_tail_geometry(hp, oracle, table, monkeypatch):
    """One and two blocks, a last dword that is loaded byte by byte, and two workgroups whose waves walk many blocks each
    through the next-descriptor prefetch (the block count is no multiple of the 32 waves)."""
    from kmergutsjava_amd import synth
    img, keys = table
    monkeypatch.setenv("KG_PART_WGS", "2")
    lens = [23, 24, 25, 214, 215, 216, 217, 407, 408, 50_000]
    off = _offsets(lens)
    assert _dna_blocks(lens) % 32 != 0 and _dna_blocks(lens) > 4 * 32
    s = bytearray(plant(synth.random_dna(int(off[-1]), 7110).numpy().tobytes(), off, keys, every=37, start=0))
    big = int(off[-2])
    s[big + 1000:big + 1030] = b"N" * 30                                 # inside the 50 kbp contig
    s[big + 5000:big + 5600] = bytes(s[big + 5000:big + 5600]).lower()
    s[big + 9000] = ord("*")
    s[big + 9400] = 0xFF
    ora, st = _scan_and_compare(hp, oracle, img, bytes(s), off, "geometry", min_hits=2)
    assert len(ora["hits"]) > 500


@pytest.mark.parametrize("progress", [False, True])
def test_stream_shorter_than_num_sigs(hp, oracle, table, progress):
    """A record stream that ends before some home slots: those queries are never looked up, lookup_ran_off and (with
    KG_F_PROGRESS) the progress lines and the first slot beyond the stream are the oracle's."""
    from kmergutsjava_amd import synth
    img, keys = table
    off = _offsets([30_000, 217, 20_000])
    sb = plant(synth.random_dna(int(off[-1]), 7120).numpy().tobytes(), off, keys, every=61)
    for cut in (NUM_SIGS - 1, 150_000, 100_007, 40_000):
        short = img[:24 + 24 * cut]
        ora = oracle.run(short, sb, off, lookup_mode=0, min_hits=2)
        with hp.SignatureTable.from_bytes(short) as tab, tab.scan(sb, off, hp.Params(min_hits=2, progress=progress)) as r:
            assert r.stats["partitioned"] == 1 and r.stats["fallback"] == 0
            assert r.hits().tobytes() == ora["hits"].tobytes() and r.calls().tobytes() == ora["calls"].tobytes(), cut
            assert r.stats["lookup_ran_off"] == int(ora["lookup_aborted"]), cut
            if progress:
                pr = r.progress()
                lines = [(f, pr["found_upto"][f]) for f in range(1, 11) if pr["first_visited"][f] >= 0]
                assert pr["stream_slots"] == cut and lines == ora["processed"], (cut, pr, ora["processed"])
                assert pr["kmers_found"] == ora["kmers_found"]
                if ora["read_eof"]:
                    assert pr["walk_ran_off"] == 1 or pr["first_beyond"] == cut, (cut, pr)
                elif ora["skip_failed_bytes"] >= 0:
                    assert pr["walk_ran_off"] == 0 and pr["first_beyond"] > cut, (cut, pr)
                    assert 24 * (pr["first_beyond"] - (pr["last_visited"] + 1)) == ora["skip_failed_bytes"], (cut, pr)
                else:
                    assert pr["walk_ran_off"] == 0 and pr["first_beyond"] == -1


def test_overflow_list_and_fallback(hp, oracle, table, monkeypatch):
    """Regions a tenth of their usual size and a contig that repeats one 24-mer: its groups go to the overflow list; with a list
    of one group the scan falls back to direct probing.  The records are the same."""
    from kmergutsjava_amd import synth
    img, keys = table
    word = synth.back_translate(synth.decode_kmer(keys[5])).encode()
    rnd = synth.random_dna(60_000, 7130).numpy().tobytes()
    parts = [rnd[:30_000], word * 400, rnd[30_000:]]
    off = _offsets([len(p) for p in parts])
    sb = plant(b"".join(parts), off, keys, every=45)
    ora = oracle.run(img, sb, off, lookup_mode=1, min_hits=2)
    monkeypatch.setenv("KG_PART_SLACK", "10")
    with hp.SignatureTable.from_bytes(img) as tab, tab.scan(sb, off, hp.Params(min_hits=2)) as r:
        assert r.stats["partitioned"] == 1 and r.stats["fallback"] == 0, r.stats
        assert_same_records(r, ora, "overflow list")
    monkeypatch.setenv("KG_PART_OVF_GROUPS", "1")
    with hp.SignatureTable.from_bytes(img) as tab, tab.scan(sb, off, hp.Params(min_hits=2)) as r:
        assert r.stats["fallback"] == 1 and r.stats["partitioned"] == 0, r.stats
        assert_same_records(r, ora, "fallback")


def test_low_complexity_blocks(hp, oracle, table):
    """A homopolymer and a dinucleotide repeat inside random sequence: their blocks are set aside for lowc_blocks_kernel, which
    also counts their query k-mers."""
    from kmergutsjava_amd import synth
    img, keys = table
    rnd = synth.random_dna(40_000, 7140).numpy().tobytes()
    parts = [rnd[:15_000] + b"A" * 5000 + rnd[15_000:28_000] + b"AC" * 1500 + rnd[28_000:], rnd[:217]]
    off = _offsets([len(p) for p in parts])
    sb = plant(b"".join(parts), off, keys, every=4001)
    ora = oracle.run(img, sb, off, lookup_mode=1, min_hits=2)
    with hp.SignatureTable.from_bytes(img) as tab:
        with tab.scan(sb, off, hp.Params(min_hits=2, counters=True)) as r:
            assert r.stats["partitioned"] == 1
            assert_same_records(r, ora, "low complexity, counted")
            assert r.stats["windows_valid"] == ora["windows_valid"]
        with tab.scan(sb, off, hp.Params(min_hits=2)) as r:
            assert_same_records(r, ora, "low complexity")


def test_protein_lengths(hp, oracle, table):
    """part_scatter_kernel<true>: no window, one window, one block and one window more, and many blocks."""
    from kmergutsjava_amd import synth
    img, keys = table
    lens = [8, 9, 72, 73, 20_000]
    off = _offsets(lens)
    sb = plant(synth.random_protein(int(off[-1]), 7150).numpy().tobytes(), off, keys, every=19, dna=False, start=0)
    ora, st = _scan_and_compare(hp, oracle, img, sb, off, "protein lengths", aa=True, min_hits=2)
    assert len(ora["hits"]) > 500


@pytest.fixture(scope="module")
def dense_batch():
    """200 kbp assembled from signature k-mers of 8 functions: CALLs every few hundred records."""
    from kmergutsjava_amd import synth
    seq, off, rec = synth.high_density_device(3, 2800, NUM_SIGS, 60_000, 7160, True)
    rec[:, 4] %= 8                                                       # the functions of the runs: 32 -> 8
    return synth.table_image(rec), seq.numpy().tobytes(), off


@pytest.mark.parametrize("pairs", ["0", "1"])
def test_call_pass_in_pieces(hp, oracle, dense_batch, monkeypatch, pairs):
    """calls_wave_kernel over pieces of 64 records, gap pieces only and with pair pieces, default parameters and the
    order-constrained mode (the slow path); the event bytes of the -d stream are compared with the records."""
    img, sb, off = dense_batch
    monkeypatch.setenv("KG_AGG_BLOCK_SHIFT", "6")
    monkeypatch.setenv("KG_AGG_PAIRS", pairs)
    for kw in (dict(), dict(order_constraint=True)):
        ora, st = _scan_and_compare(hp, oracle, img, sb, off, "CALL pass pairs=%s %s" % (pairs, kw), **kw)
        # (3 x 2800 assembled k-mers: a hit each in their own frame; a CALL per run of >= 5 of one function)
        assert len(ora["hits"]) >= 3 * 2800 and len(ora["calls"]) > 50, (len(ora["hits"]), len(ora["calls"]))
        if not kw and pairs == "1":
            assert st["agg_pieces"] > 0, st                              # (no gaps in a dense batch: pair pieces only)
