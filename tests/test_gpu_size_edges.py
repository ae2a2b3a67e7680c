"""Size boundaries of the device primitives that the table build, signature derivation, assignment and function regions
share: the radix sort's 4096-item tiles, 1024-item waves and 64-item ballot steps, the tile scan's steps of 256 tiles, the 16
items per thread of the derive's segmented passes, the key width ceil(log2 n_prot), the 64-window blocks, and kAssignShort /
kAssignWalk.  Each case sits on, or next to, one of those edges and is checked against an exact reference written here with
Python integers (and against the torch / numpy models of tests/).

The region stage (kg_regions.hpp, kg_host_regions.hpp) adds edges of its own, with the cases of tests/region_cases.py: the
running maximum of region_heads_kernel carried over a thread's 16 items, a wave's 1024, a tile's 4096 and the tile scan's step at
item 256 * 4096, by nested runs and by runs that split, or just do not, at the boundary; region_walk_kernel's loads of 16
items, with regions of 15, 16, 17, 32 and 33 CALLs and a last region that ends at n; list sizes at the sort's edges where
every x0 is equal; and the key widths of its four sorts, with contigs of 3 to 2^31 - 1 nt (left_bits up to 31, 33 + left_bits
up to 64) and 1 to 32769 contigs."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import assign_model as A  # noqa: E402
import region_cases as RC  # noqa: E402
import regions_model as R  # noqa: E402
import signature_model as M  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

MAX = 20 ** 8
EMPTY = MAX + 1
TILE = 4096


# ---------------------------------------------------------------- table build ----

def _keys(n, how, seed):
    rng = np.random.default_rng(seed)
    if how == "random":
        k = np.unique(rng.integers(0, MAX, size=n + n // 8 + 16))
        k = rng.permutation(k)[:n]
    else:           # every radix digit: k-mers near 0 and near 20^8 - 1
        lo = np.arange(0, (n + 1) // 2, dtype=np.int64)
        hi = MAX - 1 - np.arange(0, n // 2, dtype=np.int64)
        k = rng.permutation(np.concatenate([lo, hi]))
    assert len(k) == n and len(np.unique(k)) == n
    return k.astype(np.int64)


def _sigs(keys, seed):
    from kmergutsjava_amd import synth
    otu, avg, fn, wt = (x.numpy() for x in synth.payload_of(torch.from_numpy(keys), seed))
    s = np.zeros(len(keys), dtype=N.SIGNATURE_DTYPE)
    s["kmer"], s["otuIndex"], s["avgFromEnd"], s["functionIndex"], s["functionWt"] = keys, otu, avg, fn, wt
    return s


def _synth_body(sigs, num_sigs):
    from kmergutsjava_amd import synth
    pay = tuple(torch.from_numpy(sigs[k].copy()) for k in ("otuIndex", "avgFromEnd", "functionIndex", "functionWt"))
    rec, placed = synth.build_table(torch.from_numpy(sigs["kmer"].copy()), pay, num_sigs)
    return synth.table_image(rec)[24:], placed


def _probe_body(sigs, num_sigs):
    """plain linear-probing insertion in (home, k-mer) order, no wrap-around: the layout the lookup reads"""
    body = np.zeros(num_sigs, dtype=N.SIGNATURE_DTYPE)
    body["kmer"] = EMPTY
    order = sorted(range(len(sigs)), key=lambda i: (int(sigs["kmer"][i]) % num_sigs, int(sigs["kmer"][i])))
    nxt, placed = 0, 0
    for i in order:
        pos = max(int(sigs["kmer"][i]) % num_sigs, nxt)
        if pos >= num_sigs:
            continue
        body[pos] = sigs[i]
        nxt = pos + 1
        placed += 1
    return body.tobytes(), placed


def _built(sigs, num_sigs, entry):
    from kmergutsjava_amd import hotpath
    src = torch.from_numpy(sigs.view(np.uint8).copy()).cuda() if entry == "device" else sigs
    with hotpath.SignatureTable.build(src, num_sigs) as tab:
        return tab.device_entries().cpu().numpy().tobytes(), tab.placed


BUILD_N = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 256 * TILE - 1, 256 * TILE + 1, 257 * TILE]


@pytest.mark.parametrize("n", BUILD_N)
def test_table_build_at_tile_edges(n):
    """n signatures at the sort's and the tile scan's edges; num_sigs a little above n (load near 1: long runs and drops at
    the end) and about 2n; random k-mers and k-mers at both ends of the range; both entry points."""
    small = n <= 100_000
    for how in ("random", "extremes"):
        sigs = _sigs(_keys(n, how, n), 7 + n)
        for num_sigs in (n + 1 + n // 64, 2 * n + 1):
            want, placed = _synth_body(sigs, num_sigs)
            if small:
                ref, ref_placed = _probe_body(sigs, num_sigs)
                assert ref == want and ref_placed == placed, (n, how, num_sigs)
            for entry in ("host", "device"):
                got, got_placed = _built(sigs, num_sigs, entry)
                assert got_placed == placed, (n, how, num_sigs, entry)
                assert got == want, (n, how, num_sigs, entry)


def test_table_build_drops_at_the_end():
    """every k-mer homed in the last slots: the run is pushed past the end and all but a few are dropped"""
    for n, S in ((TILE + 1, 5003), (TILE, 4099), (65, 67)):
        keys = (S - 3) + S * np.arange(n, dtype=np.int64)
        keys = keys[keys < MAX]
        sigs = _sigs(np.random.default_rng(n).permutation(keys), n)
        want, placed = _synth_body(sigs, S)
        ref, ref_placed = _probe_body(sigs, S)
        assert (ref, ref_placed) == (want, placed) and placed == 3
        for entry in ("host", "device"):
            assert _built(sigs, S, entry) == (want, placed)


# ---------------------------------------------------------------- signature derivation ----

ALPHA = M.ALPHA


def _f32(fr):
    """the float32 nearest to the Fraction fr (ties to even)"""
    x = np.float32(float(fr))
    best = None
    for c in (np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))):
        d = abs(Fraction(float(c)) - fr)
        key = (d, int(c.view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, c)
    return best[1]


def _exact_derive(seq, off, fn, otu, minp, pur):
    """the header's rule with Python integers: a k-mer's proteins P (first window i_p), f* the most frequent function
    (smallest on ties), c its count; kept when |P| >= min_proteins and 100 c >= purity |P|; OTU the most frequent among
    f*'s proteins (smallest on ties); avgFromEnd = floor(sum(len_p - i_p) / c); functionWt = float32(c / |P|) rounded once"""
    code = {ch: j for j, ch in enumerate(ALPHA)}
    first = {}
    for p in range(len(off) - 1):
        s = seq[off[p]:off[p + 1]]
        for i in range(0, len(s) - 8):
            w = s[i:i + 8]
            if any(ch not in code for ch in w):
                continue
            v = 0
            for ch in w:
                v = v * 20 + code[ch]
            first.setdefault(v, {}).setdefault(p, i)
    rows = []
    for v in sorted(first):
        P = first[v]
        n = len(P)
        cf = {}
        for p in P:
            if fn[p] >= 0:
                cf[int(fn[p])] = cf.get(int(fn[p]), 0) + 1
        if not cf or n < minp:
            continue
        f = min(cf, key=lambda x: (-cf[x], x))
        c = cf[f]
        if 100 * c < pur * n:
            continue
        mem = [p for p in P if fn[p] == f]
        oc = {}
        for p in mem:
            oc[int(otu[p])] = oc.get(int(otu[p]), 0) + 1
        o = min(oc, key=lambda x: (-oc[x], x))
        tot = sum(int(off[p + 1] - off[p]) - P[p] for p in mem)
        rows.append((v, o, tot // c, f, _f32(Fraction(c, n))))
    out = np.zeros(len(rows), dtype=N.SIGNATURE_DTYPE)
    for j, r in enumerate(rows):
        out[j] = r
    return out


def _join(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return b"".join(seqs), off


def _derive(seq, off, fn, otu, minp, pur, **kw):
    from kmergutsjava_amd import hotpath
    with hotpath.derive_signatures(seq, off, fn, otu, min_proteins=minp, purity_pct=pur, **kw) as s:
        return s.numpy().copy(), s.stats()


def _check_derive(seq, off, fn, otu, minp=1, pur=50, **kw):
    want = _exact_derive(seq, off, fn, otu, minp, pur)
    assert want.tobytes() == M.derive(seq, off, fn, otu, minp, pur).tobytes()
    got, st = _derive(seq, off, fn, otu, minp, pur, **kw)
    assert got.tobytes() == want.tobytes(), (len(got), len(want))
    d = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    from kmergutsjava_amd import hotpath
    with hotpath.derive_signatures(None, off, fn, otu, min_proteins=minp, purity_pct=pur,
                                   device_ptr=d.data_ptr() if d.numel() else 0, **kw) as s:
        assert s.numpy().tobytes() == want.tobytes()
    return got, st


def _rand_prot(rng, n):
    return np.frombuffer(ALPHA, dtype=np.uint8)[rng.integers(0, 20, size=n)].tobytes()


def _mutate(rng, s, rate):
    a = np.frombuffer(s, dtype=np.uint8).copy()
    m = rng.random(a.size) < rate
    a[m] = np.frombuffer(ALPHA, dtype=np.uint8)[rng.integers(0, 20, size=int(m.sum()))]
    return a.tobytes()


@pytest.mark.parametrize("length", [8, 9, 71, 72, 73, 136, 137])
def test_derive_protein_lengths_at_block_edges(length):
    """proteins of one length at the 64-window block edges (len - 8 windows), in families with shared k-mers"""
    rng = np.random.default_rng(length)
    seqs, fn, otu = [], [], []
    for fam in range(6):
        base = _rand_prot(rng, length)
        for k in range(4):
            seqs.append(_mutate(rng, base, 0.03) if k else base)
            fn.append(int(rng.integers(-1, 3)))
            otu.append(int(rng.integers(0, 3)))
    seq, off = _join(seqs)
    got, st = _check_derive(seq, off, np.array(fn, np.int32), np.array(otu, np.int32))
    assert st["windows"] == len(seqs) * max(length - 8, 0)
    if length > 8:
        assert len(got) > 0


@pytest.mark.parametrize("n_prot", [1, 2, 3, 4, 5, 8, 9, 64, 65, 1024, 1025])
def test_derive_key_width_edges(n_prot):
    """n_prot where the key width ceil(log2 n_prot) changes: a shared core in every protein, random tails"""
    rng = np.random.default_rng(n_prot)
    core = _rand_prot(rng, 20)
    seqs = [_mutate(rng, core, 0.02) + _rand_prot(rng, int(rng.integers(0, 12))) for _ in range(n_prot)]
    fn = rng.integers(-1, 4, size=n_prot).astype(np.int32)
    fn[0] = 1
    otu = rng.integers(0, 5, size=n_prot).astype(np.int32)
    seq, off = _join(seqs)
    for minp, pur in ((1, 1), (2, 50)):
        _check_derive(seq, off, fn, otu, minp, pur)


def _one_window(kmer_str):
    assert len(kmer_str) == 8
    return kmer_str.encode() + b"A"          # length 9: exactly one window, the first 8 residues


@pytest.mark.parametrize("lead", [0, 15, 16, 17])
@pytest.mark.parametrize("run", [15, 16, 17, 32, 33])
def test_derive_pair_runs_at_thread_edges(lead, run):
    """one k-mer in exactly `run` proteins, behind a smaller k-mer in `lead` proteins: its run of (k-mer, protein) pairs is
    `run` items long and starts at item `lead` of the sorted list (16 items a thread)"""
    rng = np.random.default_rng(100 * lead + run)
    seqs = [_one_window("AAAAAAAC")] * lead + [_one_window("CDEFGHIK")] * run
    perm = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in perm]
    n = len(seqs)
    fn = rng.integers(-1, 3, size=n).astype(np.int32)
    otu = rng.integers(0, 4, size=n).astype(np.int32)
    seq, off = _join(seqs)
    got, st = _check_derive(seq, off, fn, otu, 1, 1)
    assert st["pairs"] == n
    # one protein repeating a k-mer in `run` windows (equal keys that collapse into one pair), behind `lead` other pairs
    seq2, off2 = _join([_one_window("AAAAAAAC")] * lead + [b"C" * (8 + run)])
    _check_derive(seq2, off2, np.zeros(lead + 1, np.int32), np.arange(lead + 1, dtype=np.int32), 1, 1)


def test_derive_windows_per_pass_at_the_cap():
    """max_windows_per_pass equal to the windows to split, one below and one above"""
    seq, off, fn, otu = M.family_set(12, 6, 200, 0.04, 91)
    one, st = _check_derive(seq, off, fn, otu, 2, 80)
    V = st["valid_windows"]
    for cap in (V - 1, V, V + 1, V // 3, V // 3 + 1):
        got, st2 = _check_derive(seq, off, fn, otu, 2, 80, max_windows_per_pass=cap)
        assert got.tobytes() == one.tobytes()
        assert (st2["passes"] == 1) == (cap >= V), (cap, V, st2["passes"])
    # one k-mer alone in 60 windows: a pass must hold it whole
    seq2, off2 = _join([b"W" * 28] * 3)
    z = np.zeros(3, np.int32)
    for cap in (60, 61):
        got, st3 = _check_derive(seq2, off2, z, z, 1, 1, max_windows_per_pass=cap)
        assert len(got) == 1 and st3["passes"] == 1
    with pytest.raises(N.KmerGutsNativeError) as ei:
        _derive(seq2, off2, z, z, 1, 1, max_windows_per_pass=59)
    assert ei.value.code == N.KG_ERR_LIMIT
    # two bins of one k-mer each (60 windows of W x 8, 40 of A x 8): the cap at the larger bin, one above, at the sum, one
    # below and one above
    seq3, off3 = _join([b"W" * 28] * 3 + [b"A" * 28] * 2)
    z = np.zeros(5, np.int32)
    for cap, want_passes in ((60, 2), (61, 2), (99, 2), (100, 1), (101, 1)):
        got, st4 = _check_derive(seq3, off3, z, z, 1, 1, max_windows_per_pass=cap)
        assert len(got) == 2 and st4["passes"] == want_passes, (cap, st4["passes"])


# ---------------------------------------------------------------- assignment ----

def _exact_assign(calls, cs, ms=0, share=50):
    """S and T in Python ints, W by float32 adds in emission order; ranked by S desc, W desc, f asc"""
    out = np.zeros(len(cs) - 1, dtype=N.ASSIGNMENT_DTYPE)
    for p in range(len(cs) - 1):
        grp, order, T = {}, [], 0
        for r in calls[int(cs[p]):int(cs[p + 1])]:
            f = int(r["fI"])
            if f not in grp:
                grp[f] = [0, np.float32(0)]
                order.append(f)
            grp[f][0] += int(r["count"])
            grp[f][1] = np.float32(grp[f][1] + np.float32(r["weightedHits"]))
            T += int(r["count"])
        rk = sorted(order, key=lambda f: (-grp[f][0], -float(grp[f][1]), f))
        o = out[p]
        o["n_calls"], o["otu"], o["n_functions"] = int(cs[p + 1] - cs[p]), -1, len(rk)
        o["fI"], o["second_fi"] = (rk[0] if rk else -1), (rk[1] if len(rk) > 1 else -1)
        if rk:
            S = grp[rk[0]][0]
            o["score"], o["weighted"], o["total"] = S, grp[rk[0]][1], T
            o["assigned"] = int(S >= ms and 100 * S >= share * T)
            if len(rk) > 1:
                o["second_score"] = grp[rk[1]][0]
        out[p] = o
    return out


def _assign_dev(calls, cs, dst):
    from kmergutsjava_amd import hotpath
    if dst == "host":
        return hotpath.assign_calls(calls, cs)
    import ctypes as C
    n = len(cs) - 1
    out = torch.full((max(n, 1) * 40,), 0xAB, dtype=torch.uint8, device="cuda")
    c = np.ascontiguousarray(calls, dtype=N.CALL_DTYPE)
    csa = np.ascontiguousarray(cs, dtype=np.int64)
    p = N.KgAssignParams(0, 50)
    torch.cuda.synchronize()
    N.check(N.load().kg_assign_calls(0, C.byref(p), c.ctypes.data if c.size else None, csa.ctypes.data, n, None,
                                     out.data_ptr() if n else None))
    return out[:n * 40].cpu().numpy().view(N.ASSIGNMENT_DTYPE)


WEIGHTS = np.array([float(2 ** 24), 1.0, 0.1, 3.0, 0.5, 1e-3], np.float32)


def _protein(rng, fns):
    c = np.zeros(len(fns), dtype=N.CALL_DTYPE)
    c["fI"] = fns
    c["count"] = rng.integers(2, 5, size=len(fns))
    c["weightedHits"] = WEIGHTS[rng.integers(0, len(WEIGHTS), size=len(fns))]
    return c


def _batch(prots):
    cs = np.zeros(len(prots) + 1, np.int64)
    cs[1:] = np.cumsum([len(p) for p in prots])
    calls = np.concatenate(prots) if prots else np.zeros(0, N.CALL_DTYPE)
    return calls, cs


def _check_assign(calls, cs):
    want = _exact_assign(calls, cs)
    assert want.tobytes() == A.assign(calls, cs).tobytes()
    for dst in ("host", "device"):
        got = _assign_dev(calls, cs, dst)
        assert got.tobytes() == want.tobytes(), dst


def test_assign_protein_lengths_at_the_short_edge():
    """proteins of exactly 15, 16, 17 and 33 CALLs (short lane / sorted path), with ties and few functions"""
    rng = np.random.default_rng(1)
    prots = []
    for n in (15, 16, 17, 33, 1, 0, 16, 17):
        for n_fn in (1, 2, 5, n or 1):
            prots.append(_protein(rng, rng.integers(0, n_fn, size=n)))
    _check_assign(*_batch(prots))


def test_assign_function_runs_at_the_walk_edge():
    """one function's run of 15, 16, 17, 32 and 33 CALLs inside long proteins (kAssignWalk items a load)"""
    rng = np.random.default_rng(2)
    prots = []
    for run in (15, 16, 17, 32, 33):
        fns = np.concatenate([np.full(run, 7), rng.integers(0, 4, size=20)])
        prots.append(_protein(rng, rng.permutation(fns)))
        prots.append(_protein(rng, np.full(run, 3)))                         # the whole protein one run
        prots.append(_protein(rng, np.concatenate([np.full(run, 2), np.full(run + 1, 9)])))
    _check_assign(*_batch(prots))


@pytest.mark.parametrize("n_long", [63, 64, 65])
def test_assign_long_proteins_per_batch(n_long):
    """63, 64 and 65 long proteins in one batch (one wave each), with CALL-less proteins between them, one long protein
    whose runs all have length 1"""
    rng = np.random.default_rng(n_long)
    prots = []
    for k in range(n_long):
        n = int(rng.choice([17, 18, 33, 64, 65, 200]))
        if k == n_long // 2:
            prots.append(_protein(rng, rng.permutation(300) * 5 - 700))       # every run of length 1
        else:
            prots.append(_protein(rng, rng.integers(0, 6, size=n)))
        if k % 3 == 0:
            prots.append(np.zeros(0, N.CALL_DTYPE))
            prots.append(np.zeros(0, N.CALL_DTYPE))
        if k % 5 == 0:
            prots.append(_protein(rng, rng.integers(0, 3, size=int(rng.integers(1, 17)))))
    calls, cs = _batch(prots)
    assert int(((cs[1:] - cs[:-1]) > 16).sum()) == n_long
    _check_assign(calls, cs)


# ---------------------------------------------------------------- function regions ----

REGION_BRUTE_MAX = 20_000          # CALLs up to which the plain loops are the reference; the numpy model above


def _check_regions(case):
    from kmergutsjava_amd import hotpath
    want = (R.brute_force if len(case.calls) <= REGION_BRUTE_MAX else R.regions)(*case.args)
    RC.check_expect(case, *want)
    counted = RC.counted(case.calls, want[0])
    for device_out in (False, True):
        st = {}
        regs, start = hotpath.region_calls(*case.args, device_out=device_out, stats=st)
        if device_out:
            regs = regs.cpu().numpy().view(N.REGION_DTYPE)
        assert regs.tobytes() == want[0].tobytes(), (case.name, device_out, len(regs), len(want[0]))
        assert start.tobytes() == want[1].tobytes(), (case.name, device_out)
        assert {k: st[k] for k in counted} == counted, (case.name, device_out)


def _region_params(family):
    return [pytest.param(v, id=RC.case_id(v)) for v in RC.CASES[family]]


@pytest.mark.parametrize("values", _region_params("nested"))
def test_regions_nested_run_across_slices(values):
    """(lead, run, follow): one CALL covers the `run` - 1 behind it, from item `lead` on: one region, whose maximum comes over
    every thread, wave and tile edge inside the run; follow: the next group starts under that maximum and is three regions"""
    _check_regions(RC.make("nested", values))


@pytest.mark.parametrize("values", _region_params("split"))
def test_regions_split_run_at_a_slice_edge(values):
    """(boundary, where, merge_gap, twin): the first item behind the boundary, or the last in front, lies merge_gap + 2 nt
    behind the maximum (a new region) or merge_gap + 1 (none)"""
    _check_regions(RC.make("split", values))


def test_regions_run_across_the_tile_scan_step():
    """a nested run of 4001 CALLs over item 256 * 4096, its maximum in front: tile_pre of the tile scan's second step"""
    _check_regions(RC.make("step", ()))


@pytest.mark.parametrize("values", _region_params("walk"))
def test_regions_walk_lengths_and_list_end(values):
    """(lead, tail): regions of 15, 16, 17, 32, 33 CALLs and `tail`, the last one ending at n"""
    _check_regions(RC.make("walk", values))


@pytest.mark.parametrize("values", _region_params("sizes"))
def test_regions_list_sizes_with_equal_keys(values):
    """(n, flavour): n CALLs with x0 = 0 on contigs of 3 nt: the order inside a region is the sorts' stability"""
    _check_regions(RC.make("sizes", values))


@pytest.mark.parametrize("values", _region_params("lmax"))
def test_regions_contig_length_key_widths(values):
    """(L, merge_gap, min_len): the longest contig where the pass counts of the x0 sort (left_bits) and of the
    (right, strand, fI) sort (33 + left_bits) change, up to 2^31 - 1 nt"""
    _check_regions(RC.make("lmax", values))


@pytest.mark.parametrize("values", _region_params("nseqs"))
def test_regions_contig_count_key_widths(values):
    """(n_seqs, L): the number of contigs where 32 + bits_for(2 n_seqs) and left_bits + bits_for(n_seqs) pass 8, 16, 24,
    40 and 48 bits"""
    _check_regions(RC.make("nseqs", values))


def test_regions_contig_length_limit():
    """2^31 nt in one contig is KG_ERR_LIMIT and names the contig; 2^31 - 1 nt with a CALL ending at L - 1 is fine; a CALL
    ending at L is outside its contig"""
    from kmergutsjava_amd import hotpath
    L = RC.INT_MAX
    c = np.zeros(2, dtype=N.CALL_DTYPE)                 # contig 1, '+': frame 0 codon 0, and frame 1 up to x1 = L - 1
    c["container"], c["start"], c["end"], c["count"], c["fI"] = [6, 7], [0, (L - 4) // 3], [0, (L - 4) // 3], 3, 1
    assert 1 + 3 * int(c["end"][1]) + 2 == L - 1
    off = np.array([0, 5, 5 + L], np.int64)
    regs, start = hotpath.region_calls(c, off, 0)
    assert regs["right"].tolist() == [2, L - 1] and start.tolist() == [0, 0, 2]
    assert regs.tobytes() == R.brute_force(c, off, 0)[0].tobytes()
    with pytest.raises(N.KmerGutsNativeError) as ei:
        hotpath.region_calls(c, np.array([0, 5, 5 + L + 1], np.int64), 0)
    assert ei.value.code == N.KG_ERR_LIMIT and "contig 1" in str(ei.value) and "2^31" in str(ei.value)
    bad = c.copy()
    bad["container"][1], bad["start"][1], bad["end"][1] = 8, (L - 4) // 3, (L - 4) // 3          # frame 2: x1 = L
    assert 2 + 3 * int(bad["end"][1]) + 2 == L
    with pytest.raises(N.KmerGutsNativeError) as ei:
        hotpath.region_calls(bad, off, 0)
    assert ei.value.code == N.KG_ERR_ARG and "CALL 1" in str(ei.value) and "outside" in str(ei.value)
