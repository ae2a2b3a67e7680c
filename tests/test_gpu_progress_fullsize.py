"""KG_F_PROGRESS at BASELINE config 3 (1 Gbp contig mix against the 33.6 GB table, production geometry: 668 buckets of 2^21
slots, four chunks): the scan on the byte home index leaves the plain scan's records in HBM and the counting kernels'
progress summary and hit slots (KG_F_COUNTERS | KG_F_PROGRESS, the tags)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NUM_SIGS = 1_400_303_159          # the full-size table, 33.6 GB at load 0.5


def test_config3_progress_scan_on_the_byte_home_index(monkeypatch):
    from kmergutsjava_amd import hotpath as hp, synth
    monkeypatch.delenv("KG_PARTITION", raising=False)
    monkeypatch.delenv("KG_BIDX", raising=False)
    dev = torch.device("cuda", 0)
    rec, placed, keys = synth.random_table(NUM_SIGS, 0.5, 202, dev)
    del keys
    lens = synth.contig_mix_lengths(1_000_000_000, 301)
    off = synth.offsets_of(lens)
    seq = synth.random_dna(int(off[-1]), 302, dev)
    torch.cuda.synchronize()
    try:
        with hp.SignatureTable.from_device_ptr(rec.data_ptr(), NUM_SIGS, 0, keepalive=rec) as tab:
            with tab.scan(None, off, hp.Params(), device_ptr=seq.data_ptr()) as r0, \
                    tab.scan(None, off, hp.Params(progress=True), device_ptr=seq.data_ptr()) as rp:
                st = rp.stats
                assert st["partitioned"] == 1 and st["fallback"] == 0 and st["part_levels"] == 4, st
                assert st["windows_valid"] == -1 and st["slots_inspected"] == -1
                for name in ("hits", "container_hit_start", "calls", "container_call_start", "otu"):
                    x, y = r0.device_view(name), rp.device_view(name)
                    assert x.numel() == y.numel() and torch.equal(x, y), name
                assert st["n_hits"] == r0.stats["n_hits"] > 10_000_000 and st["n_calls"] == r0.stats["n_calls"]
                pr, slots = rp.progress(), rp.hit_slots()
            with tab.scan(None, off, hp.Params(counters=True, progress=True), device_ptr=seq.data_ptr()) as rc:
                assert rc.stats["partitioned"] == 1 and rc.stats["fallback"] == 0 and rc.stats["part_levels"] == 1
                assert rc.progress() == pr, (rc.progress(), pr)
                assert np.array_equal(rc.hit_slots(), slots)
            assert pr["kmers_found"] > 1_000_000 and all(pr["first_visited"][f] >= 0 for f in range(10))
    finally:
        del rec, seq
        torch.cuda.empty_cache()
