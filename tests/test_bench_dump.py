"""bench.py --dump-outputs, host side: dump_records writes the records a scan returns as float64 arrays that hold every
field exactly, samples an array that is too large at fixed seeded rows (the same rows on every run), and stays within
the size budget.  The records come from the CPU oracle on a high-density workload (hits, CALLs and OTU votes)."""
import os

import numpy as np
import pytest
import torch

import bench


def _records(oracle):
    from kmergutsjava_amd import synth
    seq, off, rec, keys = synth.high_density_config(6, 150, 20011, 4000, dna=True)
    o = oracle.run(synth.table_image(rec), seq.numpy().tobytes(), off, lookup_mode=0)
    assert len(o["hits"]) > 500 and len(o["calls"]) > 0
    recs = {"calls": o["calls"], "container_call_start": o["container_call_start"], "otu": o["otu"],
            "hits": torch.from_numpy(o["hits"].view(np.int32).reshape(-1, 6).copy()),
            "container_hit_start": torch.from_numpy(o["container_hit_start"].copy())}
    return o, recs


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _fields(rows, dtype):
    """float64 rows -> the record array they were made of."""
    out = np.zeros(len(rows), dtype=dtype)
    j = 0
    for f in dtype.names:
        k = int(np.prod(dtype[f].shape))
        out[f] = rows[:, j:j + k].reshape(out[f].shape)
        j += k
    assert j == rows.shape[1]
    return out


def test_dump_is_exact(oracle, tmp_path):
    o, recs = _records(oracle)
    bench.dump_records(str(tmp_path), recs)
    got = _load(tmp_path)
    assert sorted(got) == ["calls", "container_call_start", "container_hit_start", "hits", "otu"]
    assert all(a.dtype == np.float64 and a.ndim == 2 for a in got.values())
    for k in ("hits", "calls", "otu"):
        assert _fields(got[k], o[k].dtype).tobytes() == o[k].tobytes(), k
    for k in ("container_hit_start", "container_call_start"):
        assert np.array_equal(got[k][:, 0], o[k]), k


def test_dump_samples_large_arrays_at_fixed_rows(oracle, tmp_path, monkeypatch):
    o, recs = _records(oracle)
    monkeypatch.setattr(bench, "DUMP_BYTES_PER_ARRAY", 8 * 7 * 100)       # 100 rows of a 6-field record
    bench.dump_records(str(tmp_path / "a"), recs)
    bench.dump_records(str(tmp_path / "b"), recs)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["hits_index"].astype(np.int64)
    assert len(idx) == 100 and np.all(np.diff(idx) > 0) and idx[-1] < len(o["hits"])
    assert _fields(a["hits"], o["hits"].dtype).tobytes() == o["hits"][idx].tobytes()


def test_dump_budget():
    """Five arrays at the cap each, sample index included, stay under 64 MB."""
    assert 5 * bench.DUMP_BYTES_PER_ARRAY < 64_000_000


@pytest.mark.gpu
def test_bench_dump_outputs_equal_a_direct_scan(tmp_path):
    """bench.py --dump-outputs at a small size: --steps is the number of timed steps, the dump holds the records of the
    timed path (a direct scan of the same seeded table and contigs returns the same records) and fits the budget."""
    import json
    import subprocess
    import sys
    from kmergutsjava_amd import hotpath, synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("KG_")}
    total_bp, num_sigs = 20_000_000, 20_000_003
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--total-bp", str(total_bp), "--num-sigs", str(num_sigs), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:] + r.stderr.decode()[-4000:]
    line = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert "cpu_baseline" not in line and "extra_configs" not in line and line["roofline"] is None
    got = _load(tmp_path / "out")
    assert sum(os.path.getsize(os.path.join(tmp_path / "out", f)) for f in os.listdir(tmp_path / "out")) < 64_000_000
    assert all(a.dtype == np.float64 for a in got.values())

    dev = torch.device("cuda", 0)
    rec, _, keys = synth.random_table(num_sigs, 0.5, 202, dev)
    del keys
    lens = synth.contig_mix_lengths(total_bp, 301)
    off = synth.offsets_of(lens)
    seq = synth.random_dna(int(off[-1]), 302, dev)
    torch.cuda.synchronize()
    with hotpath.SignatureTable.from_device_ptr(rec.data_ptr(), num_sigs, 0, keepalive=rec) as tab, \
            tab.scan(None, off, hotpath.Params(), device_ptr=seq.data_ptr()) as s:
        assert s.stats["n_hits"] == line["config"]["hits_rank0"] > 0
        hits = s.hits()
        for k, want in (("calls", s.calls()), ("otu", s.otu())):
            assert _fields(got[k], want.dtype).tobytes() == want.tobytes(), k
        assert np.array_equal(got["container_hit_start"][:, 0], s.container_hit_start())
        assert np.array_equal(got["container_call_start"][:, 0], s.container_call_start())
    idx = got["hits_index"].astype(np.int64) if "hits_index" in got else np.arange(len(hits))
    assert _fields(got["hits"], hits.dtype).tobytes() == hits[idx].tobytes()
