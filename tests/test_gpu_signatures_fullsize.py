"""About 10^9 windows derived on the device (kg_signatures_derive_device) and compared with the torch model of
tests/signature_model.py run on the same GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import signature_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


def test_a_billion_windows_equal_the_model():
    from kmergutsjava_amd import hotpath
    seq, off, fn, otu = M.family_device(3_450_000, 320, 901, "cuda")
    torch.cuda.synchronize()
    with hotpath.derive_signatures(None, off, fn, otu, device_ptr=seq.data_ptr()) as s:
        st = s.stats()
        got = s.numpy()
    assert st["windows"] >= 10 ** 9
    want = M.derive(seq, off, fn, otu)
    assert len(got) == len(want) and len(got) > 10 ** 6
    assert got.tobytes() == want.tobytes()
