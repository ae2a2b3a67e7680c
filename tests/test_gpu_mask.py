"""kg_proteins_mask on the GPU against tests/mask_model.py: flags, segments, starts and counts byte for byte.  The border cases
are derived from the kernels' geometry (kg_mask.hpp): one wave per block of 64 window positions (the tile is 64, _native.MASK_TILE,
which is also one word of the run pass), characters 64 .. 64 + W - 2 of a block from the lanes' second load, the W - 1 residues
behind a protein's last window from the last block's second step, and the run pass's carry from word to word in both directions."""
import ctypes as C

import numpy as np
import pytest

import mask_model as MM
import search_model as S
from kmergutsjava_amd import _native as N

pytestmark = pytest.mark.gpu

TILE = N.MASK_TILE
W, T, E = MM.WINDOW, MM.TRIGGER, MM.EXTEND
HC = MM.ALPHA * 8                       # high complexity: every window of 12 has 12 distinct letters, D = 11004


def _mask(seq, off, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.mask_proteins(seq, off, **kw)


def _same(prots, window=W, trigger=T, extend=E):
    seq, off = S.batch(prots)
    flags, segs, start, st = _mask(seq, off, window=window, trigger=trigger, extend=extend)
    wf, ws, wstart, wst = MM.mask_numpy(seq, off, window, trigger, extend)
    assert {k: st[k] for k in MM.COUNTS} == wst
    assert start.tobytes() == wstart.tobytes() and segs.tobytes() == ws.tobytes() and flags.tobytes() == wf.tobytes()
    return flags, segs, start, st


def _qe(n: int) -> bytes:
    return (b"QE" * n)[:n]


# ---- lengths around the window and the tile -----------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [4, 12, 32])
def test_lengths_at_the_window_and_at_the_tile(window):
    """W - 1 (no window), W, W + 1; 63, 64, 65 windows and residues; 64 + W - 2, 64 + W - 1 (the last residue of a full block's
    second load), 64 + W (the first window of a second block) -- each as a low-complexity protein, as a high-complexity one and
    with a homopolymer at either end."""
    t, e = {4: (300, 400), 12: (T, E), 32: (700, 800)}[window]
    lens = sorted({window - 1, window, window + 1, 63, 64, 65, 64 + window - 2, 64 + window - 1, 64 + window, 63 + window - 1,
                   2 * TILE + window - 1, 2 * TILE + window})
    prots = []
    for L in lens:
        prots += [_qe(L), HC[:L], (b"Q" * window + HC)[:L], HC[:max(L - window, 0)] + b"Q" * min(window, L), b""]
    _, _, _, st = _same(prots, window, t, e)
    assert st["segments"] >= 3 * len(lens) - 3 and st["proteins"] == len(prots)


def test_zero_proteins_and_only_empty_or_short_proteins():
    for prots in ([], [b""], [b"", b"QQQQQQQQQQQ", b""]):
        flags, segs, start, st = _same(prots)
        assert len(segs) == 0 and not flags.any() and st["windows"] == 0


def test_empty_proteins_between_others():
    _, segs, start, _ = _same([b"", b"Q" * 20, b"", b"", HC[:30], b"", _qe(70), b""])
    assert list(segs["protein"]) == [1, 6] and list(np.diff(start)) == [0, 1, 0, 0, 0, 0, 1, 0]


def test_a_low_window_first_and_last():
    _, segs, _, _ = _same([b"Q" * W + HC[:50], HC[:50] + b"Q" * W, b"Q" * W + HC[:TILE + 20] + b"Q" * W])
    assert (segs[0]["protein"], segs[0]["start"]) == (0, 0) and (segs[1]["protein"], segs[1]["end"]) == (1, 50 + W - 1)
    assert [(s["start"] == 0, s["end"] == TILE + 20 + 2 * W - 1) for s in segs[2:]] == [(True, False), (False, True)]


def test_no_leak_across_the_border_of_two_proteins():
    """Both low at their shared border: each has its own segment.  Half a homopolymer on each side: together they would be a low
    window, apart neither has one."""
    _, segs, _, _ = _same([HC[:40] + b"Q" * W, b"Q" * W + HC[:40]])
    assert [(s["protein"], s["start"] == 0, s["end"] == 40 + W - 1) for s in segs] == [(0, False, True), (1, True, False)]
    half = [HC[:40] + b"Q" * 4, b"Q" * 4 + HC[:40]]
    assert MM.mask_numpy(*S.batch([b"".join(half)]))[3]["segments"] == 1
    _, segs, _, _ = _same(half)
    assert len(segs) == 0


def test_a_segment_across_a_block_border():
    for at in (TILE - 6, TILE - W + 1, TILE - 1, TILE, 2 * TILE - 3):
        _, segs, _, _ = _same([HC[:at] + b"Q" * 14 + HC[:40]])
        assert len(segs) == 1 and segs[0]["start"] <= at and segs[0]["end"] >= at + 13


# ---- the run pass's carry -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["left", "right", "middle", "both"])
def test_a_long_ext_run_with_its_only_low_windows_at_one_place(where):
    """A QE repeat of 500 residues has D = 3072 in every window: ext under extend = 256, not low under trigger = 251 (3012).  One E
    turned into Q makes the windows over it (7 Q, 5 E: D = 3008) low.  The model confirms one run of 489 windows, more than seven
    words: the fill has to carry upwards from the left, downwards from the right, and both ways from the middle."""
    p = bytearray(_qe(500))
    for at in {"left": [1], "right": [497], "middle": [251], "both": [1, 497]}[where]:
        p[at] = ord("Q")
    seq, off = S.batch([bytes(p)])
    _, ws, _, wst = MM.mask_numpy(seq, off, W, 251, 256)
    assert wst["ext_windows"] == wst["masking_windows"] == 489 and 0 < wst["low_windows"] <= 2 * W and len(ws) == 1
    assert MM.mask_numpy(*S.batch([_qe(500)]), W, 251, 256)[3]["segments"] == 0
    _, segs, _, _ = _same([HC[:30], bytes(p), _qe(500), bytes(p)[::-1]], W, 251, 256)
    assert [(s["protein"], s["start"], s["end"]) for s in segs] == [(1, 0, 499), (3, 0, 499)]


def test_two_qualifying_runs_one_window_apart_give_one_segment():
    """Q * 14 + ACDFGH + E * 14: a window over the six middle letters holds a Q and 6 - a E beside them, and D is largest, 8574, only
    at a = 3 (8444 at a = 2 and 4).  With extend = 704 (8448) that one window is not ext, every other is, and both runs hold a
    homopolymer window: two qualifying runs one window apart, whose residues overlap, so one segment."""
    p, ext = b"Q" * 14 + b"ACDFGH" + b"E" * 14, 704
    assert sorted(MM.deficit(p[i:i + W]) for i in range(len(p) - W + 1))[-3:] == [8444, 8444, 8574]
    seq, off = S.batch([p])
    _, ws, _, wst = MM.mask_numpy(seq, off, W, T, ext)
    assert wst["ext_windows"] == wst["masking_windows"] == wst["windows"] - 1 and len(ws) == 1
    _, segs, _, _ = _same([HC[:20], p, HC[:TILE - 20] + p], W, T, ext)
    assert len(segs) == 2 and (segs[0]["start"], segs[0]["end"]) == (0, len(p) - 1)


# ---- thresholds -----------------------------------------------------------------------------------------------------------------

def test_thresholds_hit_exactly():
    """QEQEQEQEQEQE has D = 3072 = 12 * 256: low at trigger 256 and not at 255, ext at extend 256 and not at 255; trigger == extend."""
    prots = [_qe(40), HC[:20] + b"Q" * 12 + _qe(30), HC[:70], b"Q" * 5 + _qe(80) + b"Q" * 12]
    seq, off = S.batch(prots)
    seen = {}
    for t, e in ((256, 256), (255, 255), (0, 256), (0, 255), (255, 256), (0, 0)):
        seen[(t, e)] = _same(prots, W, t, e)[3]
    assert seen[(256, 256)]["low_windows"] > seen[(255, 255)]["low_windows"] > 0
    assert seen[(0, 256)]["ext_windows"] > seen[(0, 255)]["ext_windows"] and seen[(0, 256)]["low_windows"] == seen[(0, 255)]["low_windows"] > 0
    assert seen[(0, 256)]["masked_residues"] > seen[(0, 255)]["masked_residues"] > 0


@pytest.mark.parametrize("window,trigger,extend", [(4, 300, 400), (4, 0, 511), (32, 700, 800), (32, 0, 1279), (12, 0, 916), (7, 400, 500)])
def test_other_windows_on_a_mixed_batch(window, trigger, extend):
    _same(MM.low_complexity_batch(np.random.default_rng(50 + window), 40), window, trigger, extend)


def test_the_defaults_on_a_mixed_batch_with_several_blocks_per_protein():
    rng = np.random.default_rng(61)
    prots = MM.low_complexity_batch(rng, 30) + [MM.with_insert(rng, MM.random_protein(rng, 700))]
    _, _, _, st = _same(prots)
    assert st["segments"] > 20 and st["proteins_masked"] > 10


def test_non_residue_bytes_are_letter_20():
    """X, *, lowercase, 0 and 255 are all the 21st letter: a run of any mix of them is a homopolymer."""
    other = bytes([ord("X"), ord("*"), ord("q"), 0, 255, ord("x"), ord("B"), ord("-")])
    prots = [HC[:30] + other * 2 + HC[:30], other * 3, HC[:10] + b"X" * 6 + b"\x00" * 6 + HC[:10], HC[:25] + b"qeqeqeqeqeqe" + HC[:25]]
    flags, segs, _, _ = _same(prots)
    assert list(segs["protein"]) == [0, 1, 2, 3] and flags[30:46].all()


# ---- the batch, the entry points, the failures ----------------------------------------------------------------------------------

def test_a_batch_cut_differently_and_the_device_sequence_give_the_same():
    import torch
    rng = np.random.default_rng(62)
    prots = MM.low_complexity_batch(rng, 36)
    seq, off = S.batch(prots)
    flags, segs, start, st = _same(prots)
    per = [(flags[off[p]:off[p + 1]].tobytes(), [(s["start"], s["end"]) for s in segs[start[p]:start[p + 1]]]) for p in range(len(prots))]
    order = rng.permutation(len(prots))
    for part in (order[:7], order[7:20], order[20:]):
        sub = [prots[i] for i in part]
        s2, o2 = S.batch(sub)
        f2, g2, st2, _ = _mask(s2, o2)
        assert [(f2[o2[k]:o2[k + 1]].tobytes(), [(s["start"], s["end"]) for s in g2[st2[k]:st2[k + 1]]]) for k in range(len(sub))] == \
            [per[i] for i in part]
    dev = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    got = _mask(None, off, device_ptr=dev.data_ptr())
    assert got[0].tobytes() == flags.tobytes() and got[1].tobytes() == segs.tobytes() and got[2].tobytes() == start.tobytes()
    assert {k: got[3][k] for k in MM.COUNTS} == {k: st[k] for k in MM.COUNTS}
    # offsets that do not begin at 0: residue 0 of the flags is offsets[0]
    got = _mask(seq, off[5:])
    assert got[0].tobytes() == flags[off[5]:].tobytes() and got[2].tobytes() == (start[5:] - start[5]).tobytes()


def test_a_failed_allocation_returns_nomem_and_leaks_nothing(monkeypatch):
    import torch
    prots = MM.low_complexity_batch(np.random.default_rng(63), 20)
    seq, off = S.batch(prots)
    want = MM.mask_numpy(seq, off)
    assert _mask(seq, off)[0].tobytes() == want[0].tobytes()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    failed = 0
    for n in range(1, 100):
        monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
        try:
            got = _mask(seq, off)
            break
        except N.KmerGutsNativeError as e:
            assert e.code == N.KG_ERR_NOMEM, e
            failed += 1
            assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
    monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
    assert failed >= 15 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert torch.cuda.mem_get_info()[0] == free0


def test_each_argument_error():
    lib = N.load()
    seq = np.frombuffer(b"Q" * 30, dtype=np.uint8).copy()
    off = np.array([0, 30], dtype=np.int64)

    def call(prm, seq_ptr=seq.ctypes.data, off_ptr=off.ctypes.data, n=1, out=True):
        h = C.c_void_p()
        rc = lib.kg_proteins_mask(0, C.byref(prm) if prm is not None else None, seq_ptr, off_ptr, n, C.byref(h) if out else None)
        assert not h.value or rc == N.KG_OK
        if h.value:
            lib.kg_maskset_free(h)
        return rc, lib.kg_last_error().decode()

    P = N.KgMaskParams
    assert call(P(W, T, E, 0))[0] == N.KG_OK
    for prm, word in ((P(3, T, E, 0), "window"), (P(33, T, E, 0), "window"), (P(W, -1, E, 0), "trigger"), (P(W, 600, 599, 0), "extend"),
                      (P(W, T, 917, 0), "Lg(window)"), (P(4, 0, 512, 0), "Lg(window)"), (P(W, T, E, 1), "reserved"),
                      (P(3, -1, -2, 1), "window"), (None, "kg_mask_params")):
        rc, msg = call(prm)
        assert rc == N.KG_ERR_ARG and word in msg, (rc, msg)
    assert call(P(W, T, 916, 0))[0] == N.KG_OK
    assert call(P(W, T, E, 0), n=-1)[0] == N.KG_ERR_ARG
    assert call(P(W, T, E, 0), off_ptr=None)[0] == N.KG_ERR_ARG
    assert call(P(W, T, E, 0), seq_ptr=None)[0] == N.KG_ERR_ARG
    assert call(P(W, T, E, 0), out=False)[0] == N.KG_ERR_ARG
    bad = np.array([0, 30, 20], dtype=np.int64)
    rc, msg = call(P(W, T, E, 0), off_ptr=bad.ctypes.data, n=2)
    assert rc == N.KG_ERR_ARG and "protein 1" in msg
    # the getters' ranges
    h = C.c_void_p()
    assert lib.kg_proteins_mask(0, C.byref(P(W, T, E, 0)), seq.ctypes.data, off.ctypes.data, 1, C.byref(h)) == N.KG_OK
    try:
        buf = np.zeros(64, dtype=np.uint8)
        assert lib.kg_maskset_count(h) == 1
        assert lib.kg_maskset_flags_copy(h, 0, 31, buf.ctypes.data) == N.KG_ERR_ARG
        assert lib.kg_maskset_flags_copy(h, 10, 20, buf.ctypes.data) == N.KG_OK and buf[:20].all() and not buf[20:].any()
        assert lib.kg_maskset_copy(h, 0, 2, buf.ctypes.data) == N.KG_ERR_ARG
        assert lib.kg_maskset_stats(h, None) == N.KG_ERR_ARG and lib.kg_maskset_stats(None, None) == N.KG_ERR_ARG
    finally:
        lib.kg_maskset_free(h)
