"""kg_proteins_search_seeded on the GPU against tests/seed_model.py: records, starts and counts byte for byte.  The border cases
are derived from the kernel's geometry (kg_seed.hpp): one wave per block of 64 window positions, characters 64..94 of a block
from the lanes' second load, up to four shapes walked per block."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import align_model as A
import cluster_model as M
import search_model as S
import seed_model as SD
import trace_model as T
from kmergutsjava_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 64
NO_ALIGN = dict(max_cells=1)            # every pair skipped: the order is (s, target) and the model aligns nothing
SHAPE12 = SD.REDUCED[1][0]


def _mask(text):
    return sum(1 << j for j, ch in enumerate(text) if ch == "1")


def _search(seq, off, n_db, seed, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.search_proteins(seq, off, n_db, seeds=SD.as_dict(seed), **kw)


def _model(seq, off, n_db, seed, **kw):
    kw = dict(kw)
    kw.update(kw.pop("align", None) or {})
    for k in ("max_windows", "max_pairs"):
        kw.pop(k, None)
    return SD.search_model(seq, off, n_db, seed, **kw)


def _same(seq, off, n_db, seed, **kw):
    hits, start, st = _search(seq, off, n_db, seed, **kw)
    want, wstart, wst = _model(seq, off, n_db, seed, **kw)
    assert {k: st[k] for k in S.STAT_KEYS} == wst
    assert start.tobytes() == wstart.tobytes() and hits.tobytes() == want.tobytes()
    return hits, start, st


def _relatives(rng, n: int = 24, x_rate: float = 0.02):
    fam = [M.random_protein(rng, int(rng.integers(30, 150))) for _ in range(4)]
    prots = []
    for _ in range(n):
        p = bytearray(A.mutate(rng, fam[int(rng.integers(0, 4))], float(rng.choice([0.0, 0.05, 0.15, 0.3])))[int(rng.integers(0, 5)):])
        for i in range(len(p)):
            if rng.random() < x_rate:
                p[i] = ord("X")
        prots.append(bytes(p))
    prots += [M.random_protein(rng, int(rng.integers(0, 40))) for _ in range(5)] + [b"ACDEFGHIKX" * 3, b""]
    return [prots[i] for i in rng.permutation(len(prots))]


# ---- the test that shows the feature ------------------------------------------------------------------------------------------

def test_conservative_substitutions_are_found_by_reduced_seeds_and_not_by_exact_8mers():
    """16 targets of 200 residues; each query is its target with every 6th residue replaced inside its reduced11 class.  The
    conditions are on the input: no exact 8-mer is shared, and the model's rank-0 record is a hit on the query's own target at
    min_ratio 50.  The exact call then has no record at all; the reduced call has that hit."""
    from kmergutsjava_amd import hotpath
    n = 16
    targets, queries = SD.conservative_pairs(np.random.default_rng(800), n)
    seq, off = S.batch(targets + queries)
    assert S.shared_numpy(seq, off, n)[0] == {}
    want, wstart, wst = SD.search_model(seq, off, n, SD.REDUCED)
    for q in range(n):
        h = want[wstart[q]]
        assert (h["target"], h["status"], h["rank"]) == (q, N.SEARCH_HIT, 0) and 100 * int(h["score"]) >= 50 * max(h["self_query"], h["self_target"])
    hits, start, st = hotpath.search_proteins(seq, off, n)
    assert len(hits) == 0 and not start.any() and st["candidates"] == 0 and st["join_pairs"] == 0
    hits, start, st = hotpath.search_proteins(seq, off, n, seeds="reduced")
    assert hits.tobytes() == want.tobytes() and start.tobytes() == wstart.tobytes() and {k: st[k] for k in S.STAT_KEYS} == wst
    assert st["queries_hit"] == n and [int(hits[start[q]]["target"]) for q in range(n)] == list(range(n))


# ---- equivalence and end to end -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_the_identity_set_is_the_exact_call_on_random_planted_batches(seed):
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(810 + seed)
    prots = _relatives(rng)
    n_db = int(rng.integers(0, len(prots) + 1)) if seed % 3 else len(prots) // 2
    kw = dict(min_shared=int(rng.integers(1, 4)), max_cand=int(rng.choice([1, 3, 8, 64])), max_db_per_kmer=int(rng.choice([1, 2, 256])),
              align=dict(min_ratio_pct=int(rng.choice([0, 50])), ref=str(rng.choice(["longer", "member"]))))
    seq, off = S.batch(prots)
    exact = hotpath.search_proteins(seq, off, n_db, **kw)
    mine = hotpath.search_proteins(seq, off, n_db, seeds=dict(alphabet="identity", shapes=["11111111"]), **kw)
    assert mine[0].tobytes() == exact[0].tobytes() and mine[1].tobytes() == exact[1].tobytes()
    assert {k: mine[2][k] for k in S.STAT_KEYS} == {k: exact[2][k] for k in S.STAT_KEYS}


def _golden():
    from kmergutsjava_amd.make_signatures import _read, parse_fasta
    faa = os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz")
    return (faa,) + tuple(parse_fasta(_read(faa), faa))


def test_the_identity_set_is_the_exact_call_on_the_golden_proteome():
    """192 proteins of the golden proteome file with a substitution at every 12th residue, against the file."""
    from kmergutsjava_amd import hotpath
    _, ids, seqs = _golden()
    pick = [k for k in range(0, len(ids), len(ids) // 192) if len(seqs[k]) >= 60][:192]
    alpha = A.ALPHA
    qs = [bytes(alpha[(alpha.index(ch) + 3) % 20] if i % 12 == 6 and ch in alpha else ch for i, ch in enumerate(seqs[k])) for k in pick]
    seq, off = S.batch(list(seqs) + qs)
    exact = hotpath.search_proteins(seq, off, len(seqs))
    mine = hotpath.search_proteins(seq, off, len(seqs), seeds=dict(alphabet="identity", shapes=["11111111"]))
    assert len(exact[0]) >= 192 and mine[0].tobytes() == exact[0].tobytes() and mine[1].tobytes() == exact[1].tobytes()
    assert {k: mine[2][k] for k in S.STAT_KEYS} == {k: exact[2][k] for k in S.STAT_KEYS}


def test_end_to_end_with_reduced_seeds_and_transfer(tmp_path):
    targets, queries = SD.conservative_pairs(np.random.default_rng(820), 12)
    (tmp_path / "db.faa").write_bytes(b"".join(b">d%d\n%s\n" % (k, p) for k, p in enumerate(targets)))
    (tmp_path / "q.faa").write_bytes(b"".join(b">q%d\n%s\n" % (k, p) for k, p in enumerate(queries)))
    (tmp_path / "ann.tsv").write_bytes(b"".join(b"d%d\tfunction %d\n" % (k, k % 5) for k in range(12)))
    out, tr = tmp_path / "hits.tsv", tmp_path / "transfer.tsv"
    r = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.search_proteins", "-d", str(tmp_path / "db.faa"), "-q", str(tmp_path / "q.faa"),
                        "-o", str(out), "-A", str(tmp_path / "ann.tsv"), "--transfer", str(tr), "--seeds", "reduced"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = r.stderr.strip().splitlines()[-1]
    assert re.match(r"Queries: 12, targets: 12, candidates: \d+, aligned: \d+, hits: \d+, queries hit: 12, transferred: 12, ", line), line
    assert line.endswith(", seeds: reduced11 x 111101101011,110110011010011")
    assert tr.read_bytes() == b"".join(b"q%d\tfunction %d\n" % (k, k % 5) for k in range(12))
    rows = [x.split(b"\t") for x in out.read_bytes().splitlines()]
    assert [(x[0], x[1], x[2], x[9]) for x in rows] == [(b"q%d" % k, b"0", b"d%d" % k, b"hit") for k in range(12)]


@pytest.mark.parametrize("seed", range(10))
def test_random_batches_under_random_seed_sets(seed):
    rng = np.random.default_rng(830 + seed)
    sset = SD.REDUCED if seed == 0 else SD.random_seed(rng, n_shapes=1 + seed % 4)
    prots = _relatives(rng)
    n_db = int(rng.integers(1, len(prots)))
    kw = dict(min_shared=int(rng.integers(1, 4)), max_cand=int(rng.choice([1, 3, 8])), max_db_per_kmer=int(rng.choice([2, 4, 256])),
              align=dict(min_ratio_pct=int(rng.choice([0, 50])), max_cells=int(rng.choice([1, 3000, 1 << 26]))))
    _same(*S.batch(prots), n_db, sset, **kw)


# ---- block and protein borders ------------------------------------------------------------------------------------------------

def test_a_seed_planted_on_both_sides_of_a_block_border_and_in_the_second_block():
    """Target k is X everywhere but for 15 residues at window position 0, 63, 64, 65, 127 or 128; query k is those residues and
    one more.  The shape of span 15 has one window in them and the shape of span 12 four: s = 5, on the own target only."""
    rng = np.random.default_rng(840)
    at = [0, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK]
    plants = [M.random_protein(rng, 15) for _ in at]
    targets = [b"X" * pos + p + b"X" * int(rng.integers(1, 40)) for pos, p in zip(at, plants)]
    seq, off = S.batch(targets + [p + b"A" for p in plants])
    hits, start, st = _same(seq, off, len(at), SD.REDUCED, min_shared=1, align=NO_ALIGN)
    assert [(int(h["query"]), int(h["target"]), int(h["shared"])) for h in hits] == [(k, k, 5) for k in range(len(at))]
    assert st["valid_windows"] == 10 * len(at) == st["pairs"]


def test_span_32_reads_the_characters_of_the_second_load():
    """The care positions 0, 5, 17 and 31: lane 63 reads characters 63, 68, 80 and 94 of its block."""
    rng = np.random.default_rng(841)
    sset = (SD.IDENTITY, [_mask("1" + "0" * 4 + "1" + "0" * 11 + "1" + "0" * 13 + "1")])
    targets = [M.random_protein(rng, L) for L in (95, 96, 97, 128, 129, 200)]
    queries = [A.mutate(rng, t, 0.03) for t in targets]
    hits, start, st = _same(*S.batch(targets + queries), len(targets), sset, min_shared=1, align=NO_ALIGN)
    assert st["valid_windows"] == 2 * sum(max(L - 32, 0) for L in (95, 96, 97, 128, 129, 200)) and len(hits) >= 6


@pytest.mark.parametrize("sset", [SD.REDUCED, (SD.REDUCED11, [SHAPE12]), (SD.REDUCED11, [0x8000007F])], ids=["two", "one", "span32"])
def test_protein_lengths_at_the_span_and_at_the_blocks_last_lane(sset):
    """Lengths span, span + 1, span + 2 (no window, one, two: the last position is left out) and 64 + span, 64 + span + 1, 64 + span
    + 2 (the last valid window is lane 63 of the first block, then lane 0 and lane 1 of the second), for every span of the set."""
    rng = np.random.default_rng(842)
    lengths = sorted({SD.span(m) + d for m in sset[1] for d in (0, 1, 2, BLOCK, BLOCK + 1, BLOCK + 2)})
    targets = [M.random_protein(rng, L) for L in lengths]
    hits, start, st = _same(*S.batch(targets + targets), len(targets), sset, min_shared=1, align=NO_ALIGN)
    assert st["valid_windows"] == 2 * sum(max(L - SD.span(m), 0) for L in lengths for m in sset[1])


def test_no_residue_of_the_next_protein_leaks_into_a_window():
    """W is one long protein, the only target.  Query p is W[:L] and the protein behind it in the batch is W[L:]: a window that
    read behind p's end would read W on, and find a seed the target has.  L puts p's end on both sides of a block border, and
    below a span: a short protein in front of a long one."""
    rng = np.random.default_rng(843)
    W = M.random_protein(rng, 400)
    prots = [W]
    cuts = [5, 11, 12, 14, 15, 16, 62, 63, 64, 65, 66, 70, 75, 76, 79, 127, 128, 129, 140]
    for L in cuts:
        prots += [W[:L], W[L:]]
    seq, off = S.batch(prots)
    hits, start, st = _same(seq, off, 1, SD.REDUCED, min_shared=1, align=NO_ALIGN)
    for k, L in enumerate(cuts):
        rows = hits[start[2 * k]:start[2 * k + 1]]
        assert [int(r["shared"]) for r in rows] == ([max(L - 12, 0) + max(L - 15, 0)] if L > 12 else []), L


# ---- validity and shapes --------------------------------------------------------------------------------------------------------

def test_x_on_care_and_dont_care_positions_at_the_blocks_first_and_last_lanes():
    """Shape 111101101011: position 4 is a don't-care, position 5 a care position.  An X at lane + 4 leaves the lane's window valid,
    an X at lane + 5 does not; lanes 0 and 63 of the first block, 0 and 63 of the second."""
    rng = np.random.default_rng(844)
    sset = (SD.REDUCED11, [SHAPE12])
    base = M.random_protein(rng, 220)
    targets = []
    for lane in (0, BLOCK - 1, BLOCK, 2 * BLOCK - 1):
        for j in (4, 5):
            t = bytearray(base)
            t[lane + j] = ord("X")
            targets.append(bytes(t))
    seq, off = S.batch(targets + [base])
    hits, start, st = _same(seq, off, len(targets), sset, min_shared=1, max_cand=64, align=NO_ALIGN)
    full = 220 - 12
    by_target = {int(h["target"]): int(h["shared"]) for h in hits}
    k = 0
    for lane in (0, BLOCK - 1, BLOCK, 2 * BLOCK - 1):
        for j in (4, 5):
            at = lane + j                                   # window i loses its seed iff at - i is a care position of the shape
            lost = [i for i in range(full) if 0 <= at - i < 12 and SHAPE12 >> (at - i) & 1]
            assert by_target[k] == full - len(lost) and (lane in lost) == (j == 5)
            k += 1


def test_four_shapes_of_four_spans_at_a_proteins_end():
    rng = np.random.default_rng(845)
    sset = (SD.REDUCED11, [_mask("111"), _mask("11001"), _mask("100010001"), _mask("10000010000001")])
    targets = [M.random_protein(rng, L) for L in range(2, 18)] + [M.random_protein(rng, L) for L in (BLOCK + 2, BLOCK + 4, BLOCK + 9, BLOCK + 15)]
    hits, start, st = _same(*S.batch(targets + targets), len(targets), sset, min_shared=1, max_db_per_kmer=2, align=NO_ALIGN)
    assert st["valid_windows"] == 2 * sum(max(len(t) - s, 0) for t in targets for s in (3, 5, 9, 14))


@pytest.mark.parametrize("n_shapes", [1, 2, 3, 4])
def test_the_same_value_under_each_shape_counts_once_per_shape(n_shapes):
    sset = (SD.REDUCED11, [_mask("111"), _mask("1011"), _mask("11001"), _mask("1000101")][:n_shapes])
    hits, start, st = _same(*S.batch([b"A" * 40, b"C" * 40, b"S" * 30]), 2, sset, min_shared=1, align=NO_ALIGN)
    assert [(int(h["target"]), int(h["shared"])) for h in hits] == [(0, n_shapes)] and st["kmers"] == 2 * n_shapes


# ---- capacity and limits --------------------------------------------------------------------------------------------------------

def test_max_windows_at_the_number_of_valid_seeds_and_one_below():
    rng = np.random.default_rng(846)
    seq, off = S.batch(_relatives(rng))
    want, wstart, wst = _model(seq, off, 16, SD.REDUCED)
    assert wst["valid_windows"] > 1000 and len(want) > 4
    hits, start, st = _search(seq, off, 16, SD.REDUCED, max_windows=wst["valid_windows"])
    assert hits.tobytes() == want.tobytes() and st["valid_windows"] == wst["valid_windows"]
    with pytest.raises(N.KmerGutsNativeError) as ei:
        _search(seq, off, 16, SD.REDUCED, max_windows=wst["valid_windows"] - 1)
    assert ei.value.code == N.KG_ERR_LIMIT and "%d valid windows do not fit the one pass of this call, which holds %d (max_windows)" % (
        wst["valid_windows"], wst["valid_windows"] - 1) in str(ei.value)


def _raw(seq, off, n_db, seeds=None, prm=(2, 8, 256, 0), al=(50, 0, 11, 1, 1 << 26, None, 0), trace=0, max_trace_cells=0, null=()):
    """-> (rc, message).  seeds: the fields' values: n_shapes, alphabet_size, cls, shape, reserved."""
    lib = N.load()
    h = C.c_void_p()
    arr = np.frombuffer(bytes(seq), dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    p, a = N.KgSearchParams(*prm), N.KgAlignParams(*al)
    sp = N.KgSeedParams(seeds[0], seeds[1], (C.c_uint8 * 20)(*seeds[2]), (C.c_uint32 * 4)(*seeds[3]), seeds[4]) if seeds else None
    rc = lib.kg_proteins_search_seeded(0, C.byref(p), None if "seeds" in null else C.byref(sp), C.byref(a), arr.ctypes.data if arr.size else None,
                                       off.ctypes.data, len(off) - 1, n_db, 0, 0, trace, max_trace_cells, C.byref(h))
    msg = lib.kg_last_error().decode()
    if h.value:
        lib.kg_hitset_free(h)
    return rc, msg


def test_a_seed_space_of_exactly_2_to_the_35_and_one_over():
    """2 shapes * 4^17 and 4 shapes * 8^11 are 2^35: the key takes 35 bits and the protein's; 3 * 4^17 and 2 * 11^10 are over."""
    rng = np.random.default_rng(847)
    four = [c % 4 for c in range(20)]
    eight = [c % 8 for c in range(20)]
    w17 = [(1 << 17) - 1, ((1 << 16) - 1) | 1 << 20]
    w11 = [(1 << 11) - 1, ((1 << 10) - 1) | 1 << 12, ((1 << 10) - 1) | 1 << 20, ((1 << 10) - 1) | 1 << 31]
    prots = _relatives(rng, 12, 0.0)
    seq, off = S.batch(prots)
    for sset in ((four, w17), (eight, w11)):
        assert SD.space(sset) == 1 << 35
        hits, start, st = _same(seq, off, 8, sset, min_shared=1)
        assert len(hits) > 0
    top = bytes([A.ALPHA[7]]) * 40                               # class 7 everywhere: under the last shape the id is 2^35 - 1
    hits, start, st = _same(*S.batch([top, top]), 1, (eight, w11), min_shared=1, align=NO_ALIGN)
    assert max(SD.seed_ids(top, (eight, w11))) == (1 << 35) - 1 and int(hits[0]["shared"]) == 4
    for n_shapes, a_size, cls, shapes in ((3, 4, four, w17 + [((1 << 16) - 1) | 1 << 25]), (2, 11, SD.REDUCED11, [(1 << 10) - 1, (1 << 9) - 1 | 1 << 12])):
        rc, msg = _raw(seq, off, 8, (n_shapes, a_size, cls, shapes, 0))
        assert rc == N.KG_ERR_ARG and msg.startswith("seed space over 2^35"), msg


# ---- errors, determinism, paths, allocations, the device entry point ------------------------------------------------------------

def test_every_seed_error_with_its_first_words():
    seq, off = S.batch([b"ACDEFGHIKLMNPQRSTVWY", b"ACDEFGHIKLMNPQRSTVWY"])
    ident, r11 = SD.IDENTITY, SD.REDUCED11
    cases = [
        (dict(null=("seeds",), seeds=(1, 20, ident, [0xFF], 0)), "null kg_seed_params"),
        (dict(seeds=(0, 20, ident, [], 0)), "n_shapes must be in 1..4"),
        (dict(seeds=(5, 20, ident, [0xFF] * 4, 0)), "n_shapes must be in 1..4"),
        (dict(seeds=(1, 1, [0] * 20, [0xFF], 0)), "alphabet_size must be in 2..20"),
        (dict(seeds=(1, 21, ident, [0xFF], 0)), "alphabet_size must be in 2..20"),
        (dict(seeds=(1, 11, r11[:7] + [11] + r11[8:], [0xFF], 0)), "cls[7] must be below alphabet_size"),
        (dict(seeds=(1, 12, r11, [0xFF], 0)), "class 11 is used by no residue"),
        (dict(seeds=(1, 11, [c if c != 4 else 0 for c in r11], [0xFF], 0)), "class 4 is used by no residue"),
        (dict(seeds=(2, 11, r11, [0xFF, 0x1FE], 0)), "shape[1] must have bit 0 set"),
        (dict(seeds=(1, 11, r11, [0], 0)), "shape[0] must have bit 0 set"),
        (dict(seeds=(3, 11, r11, [0xFF, 0x17F, 0x7F], 0)), "shapes must have equal weights: shape[2]"),
        (dict(seeds=(2, 11, r11, [0xFF, 0x17F, 0, 1], 0)), "shape[3] must be 0"),
        (dict(seeds=(1, 11, r11, [0xFF], 1)), "kg_seed_params.reserved must be 0"),
        (dict(seeds=(1, 20, ident, [0x1FF], 0)), "seed space over 2^35"),
        (dict(seeds=(1, 20, ident, [0xFFFFFFFF], 0)), "seed space over 2^35"),
        # the first offender of several, and the checks that are kg_proteins_search's
        (dict(seeds=(0, 1, [30] * 20, [0], 1)), "n_shapes must be in 1..4"),
        (dict(seeds=(1, 11, r11, [0xFF], 0), prm=(2, 8, 256, 1)), "kg_search_params.reserved must be 0"),
        (dict(seeds=(1, 11, r11, [0xFF], 0), trace=3, max_trace_cells=1), "trace must be"),
        (dict(seeds=(1, 11, r11, [0xFF], 0), trace=N.TRACE_HITS, max_trace_cells=0), "max_trace_cells must be >= 1"),
    ]
    for kw, words in cases:
        rc, msg = _raw(seq, off, 1, **kw)
        assert rc == N.KG_ERR_ARG and msg.startswith(words), (kw, rc, msg)
    assert _raw(seq, off, 1, seeds=(1, 11, r11, [0xFF], 0), trace=0, max_trace_cells=-5)[0] == N.KG_OK       # ignored without a trace


def test_the_same_call_twice_and_the_database_reversed():
    rng = np.random.default_rng(848)
    prots = _relatives(rng)
    n_db = 20
    seq, off = S.batch(prots)
    first = _same(seq, off, n_db, SD.REDUCED, max_cand=3)
    again = _search(seq, off, n_db, SD.REDUCED, max_cand=3)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    rseq, roff = S.batch(prots[:n_db][::-1] + prots[n_db:])
    rev = _same(rseq, roff, n_db, SD.REDUCED, max_cand=3)
    s_of, _ = SD.shared_numpy(SD.REDUCED)(seq, off, n_db)
    for q in range(len(prots) - n_db):
        if sum(1 for (qq, d), s in s_of.items() if qq == q and s >= 2) <= 3:
            a = first[0][first[1][q]:first[1][q + 1]]
            b = rev[0][rev[1][q]:rev[1][q + 1]]
            assert sorted(zip(a["target"].tolist(), a["shared"].tolist(), a["score"].tolist(), a["status"].tolist())) == \
                sorted(zip((n_db - 1 - b["target"]).tolist(), b["shared"].tolist(), b["score"].tolist(), b["status"].tolist()))


def test_traced_hits_of_a_seeded_call():
    targets, queries = SD.conservative_pairs(np.random.default_rng(849), 4, length=90)
    rng = np.random.default_rng(850)
    queries = [A.mutate(rng, q, 0.04)[3:] for q in queries]
    seq, off = S.batch(targets + queries)
    searched = SD.search_model(seq, off, 4, SD.REDUCED)
    want = T.search_paths_model(seq, off, 4, "hits", searched=searched)
    hits, start, paths, st = _search(seq, off, 4, SD.REDUCED, paths="hits")
    assert searched[2]["queries_hit"] == 4 and want[3]["traced"] >= 4
    assert hits.tobytes() == want[0].tobytes() and start.tobytes() == want[1].tobytes() and paths.tobytes() == want[2].tobytes()
    assert {k: st[k] for k in S.STAT_KEYS + ("traced", "untraced", "trace_cells")} == want[3]


def test_failed_allocations_leave_nothing_behind(monkeypatch):
    import torch
    from kmergutsjava_amd import hotpath, synth
    seq, off = S.batch(_relatives(np.random.default_rng(851)))
    want, wstart, _ = _model(seq, off, 16, SD.REDUCED)
    assert len(want) > 4
    rec = synth.high_density_config(4, 100, 4001, 500, dna=False)[2]
    with hotpath.SignatureTable.from_bytes(synth.table_image(rec), 0) as tab:
        assert _search(seq, off, 16, SD.REDUCED)[0].tobytes() == want.tobytes()
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        failed = 0
        for n in range(1, 600):
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                got = _search(seq, off, 16, SD.REDUCED)
                break
            except N.KmerGutsNativeError as e:
                assert e.code == N.KG_ERR_NOMEM, e
                failed += 1
                assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
                assert tab.live_device_bytes() == live0
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        assert failed >= 60 and got[0].tobytes() == want.tobytes() and got[1].tobytes() == wstart.tobytes()
        assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0


def test_the_device_sequence_entry_point():
    import torch
    seq, off = S.batch(_relatives(np.random.default_rng(852)))
    want = _same(seq, off, 12, SD.REDUCED)
    dev = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    got = _search(None, off, 12, SD.REDUCED, device_ptr=dev.data_ptr())
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert {k: got[2][k] for k in S.STAT_KEYS} == {k: want[2][k] for k in S.STAT_KEYS}
    got = _search(None, off, 12, SD.REDUCED, device_ptr=dev.data_ptr(), paths="all")
    assert got[0].tobytes() == want[0].tobytes() and len(got[2]) == len(want[0])
