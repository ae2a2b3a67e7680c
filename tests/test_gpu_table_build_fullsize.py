"""kg_table_build_device at the full size: the 1 400 303 159-slot table of bench.py (about 7e8 signatures, 33.6 GB of
records) and a table of more than 2^31 slots, rebuilt from their signatures in a shuffled order and compared with
synth.build_table's records on the device."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NUM_SIGS = 1_400_303_159


def _device_signatures(keys, seed, shuffle_seed):
    """24-byte signature records (the table record layout) made on the device, in a shuffled order"""
    from kmergutsjava_amd import synth
    otu, avg, fn, wt = synth.payload_of(keys, seed)
    sig = torch.stack([(keys & 0xFFFFFFFF).to(torch.int32), (keys >> 32).to(torch.int32), otu, avg, fn,
                       wt.contiguous().view(torch.int32)], dim=1)
    del otu, avg, fn, wt
    g = torch.Generator(device=keys.device)
    g.manual_seed(shuffle_seed)
    perm = torch.randperm(keys.numel(), device=keys.device, generator=g)
    sig = sig[perm]
    del perm
    return sig


@pytest.mark.parametrize("num_sigs, load, seed", [(NUM_SIGS, 0.5, 202), ((1 << 31) + 11, 0.01, 909)])
def test_device_build_equals_synth_at_full_size(num_sigs, load, seed):
    from kmergutsjava_amd import hotpath, synth
    dev = torch.device("cuda", 0)
    rec, placed, keys = synth.random_table(num_sigs, load, seed, dev)
    sig = _device_signatures(keys, seed + 3, 7)
    del keys
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    with hotpath.SignatureTable.build(sig.view(torch.uint8).reshape(-1), num_sigs) as tab:
        del sig
        assert tab.placed == placed and tab.info()["occupied"] == placed
        assert tab.info()["numSigs"] == num_sigs
        got = tab.device_entries()
        assert got.numel() == num_sigs * 24
        assert torch.equal(got, rec.view(torch.uint8).reshape(-1))
        assert tab.live_device_bytes() == 0
        del got
    del rec
    torch.cuda.empty_cache()
