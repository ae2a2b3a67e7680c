"""Inputs of the composition tests (tests/test_compose_host.py, tests/test_gpu_compose.py): random batches around the count
pass's step, label sets around the score pass's LDS tile, caller's models, and the planted two-genome sample."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd import _native as N

# ACGTacgtuUNn- and a few arbitrary values; the bases are frequent enough that most windows exist
ALPHABET = np.frombuffer(b"ACGTacgtuUNn-" + bytes([0, 7, 64, 91, 200, 255]), dtype=np.uint8)
_WEIGHT = np.array([20] * 4 + [6] * 4 + [2, 2] + [1] * 9, dtype=np.float64)
_WEIGHT /= _WEIGHT.sum()
STEP = N.COMP_TILE
EDGES = sorted({0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, STEP - 1, STEP, STEP + 1})


def offsets_of(lens) -> np.ndarray:
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.asarray(lens, dtype=np.int64))
    return off


def random_bytes(rng, n: int) -> np.ndarray:
    return rng.choice(ALPHABET, size=int(n), p=_WEIGHT).astype(np.uint8)


def batch(rng, lens, n_labels: int = 3, homopolymer=()):
    """Random contigs of these lengths (those whose index is in `homopolymer` are all one base), labels -1 .. n_labels - 1.
    -> (bytes, offsets, labels)."""
    off = offsets_of(lens)
    seq = random_bytes(rng, off[-1])
    for s in homopolymer:
        seq[off[s]:off[s + 1]] = ord("A")
    labels = rng.integers(-1, n_labels, size=len(lens)).astype(np.int32)
    return seq, off, labels


def case(name: str):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "edges":             # every edge three times, a homopolymer of 5000, a contig of about 300 kbp
        lens = EDGES * 3 + [5000, 300_011]
        return batch(rng, lens, 3, homopolymer=[len(lens) - 2])
    if name == "many_short":        # 70 000 contigs of 4 to 12 bp: some thirty contigs in every lane group of a step
        return batch(rng, rng.integers(4, 13, size=70_000), 5)
    if name == "four_mbp":          # more steps than workgroups: a workgroup keeps a contig's histogram over its steps
        lens = [100, 4_400_000, 0, 2049, 7]
        assert sum(lens) > N.COMP_TILE * N.COMP_MAX_GRID
        return batch(rng, lens, 2)
    if name == "empty":
        return np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.int32)
    raise KeyError(name)


CASES = ["edges", "many_short", "four_mbp", "empty"]
TILE = N.COMP_SCORE_TILE
# (labels of the batch, min_train): the models are TILE - 1, TILE, TILE + 1 and 300 with the background one more row
LABEL_CASES = ["all_unlabelled", "one_label", "zero_and_top", "models_1", "models_%d" % (TILE - 1), "models_%d" % TILE,
               "models_%d" % (TILE + 1), "models_300", "min_train_drops_rows"]


def label_case(name: str):
    """-> (bytes, offsets, labels, min_train) on one batch of 700 contigs of 0 .. 400 nt."""
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 401, size=700)
    lens[:len(EDGES)] = [min(e, 4097) for e in EDGES]
    seq, off, _ = batch(rng, lens)
    n = len(lens)
    if name == "all_unlabelled":
        return seq, off, np.full(n, -1, np.int32), 0
    if name == "one_label":
        lab = np.full(n, -1, np.int32)
        lab[5::3] = 12
        return seq, off, lab, 0
    if name == "zero_and_top":
        lab = rng.choice(np.array([-1, 0, 2 ** 31 - 1], dtype=np.int64), size=n).astype(np.int32)
        return seq, off, lab, 0
    if name.startswith("models_"):
        m = int(name.split("_")[1])
        lab = (rng.integers(0, m, size=n) * 7 + 3).astype(np.int32)
        lab[rng.random(n) < 0.2] = -1
        lab[:m] = np.arange(m) * 7 + 3                                  # every label occurs
        return seq, off, lab, 0
    if name == "min_train_drops_rows":
        lab = rng.integers(-1, 12, size=n).astype(np.int32)
        lab[rng.random(n) < 0.5] = 4                                     # one row far above the threshold, the others about it
        return seq, off, lab, 10_500
    raise KeyError(name)


def callers_model(rng, n_models: int = 5):
    """Arbitrary rows: one with a single non-zero bin, one whose sum is 2^62 - 1, a background of small counts."""
    labels = np.sort(rng.choice(1000, size=n_models, replace=False)).astype(np.int32)
    counts = rng.integers(0, 1 << 20, size=(n_models + 1, 256)).astype(np.int64)
    counts[1] = 0
    counts[1, 77] = 123456
    counts[2] = (1 << 62) // 256
    counts[2, 0] += (1 << 62) - 1 - int(counts[2].sum())
    assert int(counts[2].sum()) == (1 << 62) - 1
    return labels, counts


def cut(seq, off, labels, a: int, b: int):
    """Contigs a .. b - 1 as a batch of their own."""
    return seq[int(off[a]):int(off[b])], off[a:b + 1] - off[a], labels[a:b]


# ---- the planted sample -----------------------------------------------------------------------------------------------------------

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
SAMPLE_GC = (0.35, 0.65)
FOREIGN_GC = 0.50
N_VOTED, N_UNVOTED, N_SHORT, N_FOREIGN, PER_OTU = 40, 20, 3, 10, 40


def gc_bases(rng, n: int, gc: float) -> bytes:
    p = np.array([(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2])
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(n), p=p))


def planted_sample(seed: int = 2025):
    """Two genomes of i.i.d. bases with GC 0.35 and 0.65.  Per genome: N_VOTED contigs of about 5 kbp that carry four of the
    genome's 40 random proteins, back-translated, between spacers of about 1 kbp of the genome's GC; N_UNVOTED contigs of 1500
    to 5000 bp with no protein; N_SHORT of 1000 bp.  N_FOREIGN contigs of GC 0.50.  Every other contig is reverse-complemented.
    -> (protein codes, contigs, kinds, genomes): kind is voted / unvoted / short / foreign, genome 0, 1 or -1."""
    from kmergutsjava_amd import synth
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(synth.PROT_ALPHA.encode(), dtype=np.uint8)
    codes = [rng.integers(0, 20, size=int(rng.integers(90, 130))) for _ in range(2 * PER_OTU)]
    contigs, kinds, genomes = [], [], []
    for g, gc in enumerate(SAMPLE_GC):
        for _ in range(N_VOTED):
            parts = []
            for p in rng.choice(np.arange(g * PER_OTU, (g + 1) * PER_OTU), size=4, replace=False):
                parts.append(gc_bases(rng, rng.integers(950, 1050), gc))
                parts.append(synth.back_translate(alpha[codes[p]].tobytes().decode()).encode())
            contigs.append(b"".join(parts))
            kinds.append("voted")
            genomes.append(g)
        for _ in range(N_UNVOTED):
            contigs.append(gc_bases(rng, rng.integers(1500, 5001), gc))
            kinds.append("unvoted")
            genomes.append(g)
        for _ in range(N_SHORT):
            contigs.append(gc_bases(rng, 1000, gc))
            kinds.append("short")
            genomes.append(g)
    for _ in range(N_FOREIGN):
        contigs.append(gc_bases(rng, rng.integers(1500, 5001), FOREIGN_GC))
        kinds.append("foreign")
        genomes.append(-1)
    order = rng.permutation(len(contigs))
    contigs = [contigs[i].translate(_COMP)[::-1] if n % 2 else contigs[i] for n, i in enumerate(order)]
    return codes, contigs, [kinds[i] for i in order], [genomes[i] for i in order]
