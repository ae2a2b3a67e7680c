"""prefix_sum (kg_host.hpp over scan_partials_kernel, scan_top_kernel, scan_final_kernel of kg_device.hpp) restated in numpy,
twice: as the kernels were while a chunk's items were added in 32 bits (`scan_wrapping`), and as they are with 64-bit chunk sums
(`scan_kernels`), beside the plain cumulative sum in Python integers (`scan_exact`).  All three return (excl, total).

excl is the same in the three whenever the total is below 2^32, and the same modulo 2^32 always; what differed is the total,
which the batch stages compare with 2^32: a chunk whose items add up to 2^32 or more lost that carry before the 64-bit sum over
the chunks saw it.

`families()` are the record lengths of the limit tests of tests/test_gpu_orfs.py, test_gpu_coding.py and test_gpu_starts.py: the
lists whose total the wrapping scan got wrong, and the controls it got right.  tests/test_scan_model_host.py holds them to that,
so that those tests cannot go soft when kScanChunk changes."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TEXT = open(os.path.join(ROOT, "kmergutsjava_amd", "csrc", "kg_device.hpp")).read()


def _const(name: str) -> int:
    return int(re.search(r"constexpr int %s = (\d+);" % name, _TEXT).group(1))


assert re.search(r"constexpr int kScanChunk = kScanThreads \* kScanPerThread;", _TEXT)
CHUNK = _const("kScanThreads") * _const("kScanPerThread")          # kScanChunk: the items of one workgroup
TOP = _const("kScanThreads")                                        # the chunk sums of one trip of scan_top_kernel's carry loop
LIMIT = 1 << 32
LONG = 1 << 21                                                      # the items of a long record
N_LONG = LIMIT // LONG                                              # ... and how many of them make 2^32


def _chunk_sums(lens) -> list:
    """the exact sum of every aligned chunk, as Python integers (one chunk of no items for an empty list, as the host launches)"""
    a = np.asarray(lens, dtype=np.uint32).astype(np.uint64)
    nb = max((len(a) + CHUNK - 1) // CHUNK, 1)
    return [int(a[b * CHUNK:(b + 1) * CHUNK].sum(dtype=np.uint64)) for b in range(nb)]


def _scan(lens, chunk_bits: int):
    """scan_partials_kernel with chunk sums of chunk_bits bits, scan_top_kernel in 64 bits, scan_final_kernel in 32"""
    a = np.asarray(lens, dtype=np.uint32)
    partial = [s & ((1 << chunk_bits) - 1) for s in _chunk_sums(a)]
    base, total = [], 0
    for s in partial:                                   # scan_top_kernel: exclusive in place, the carry in 64 bits
        base.append(total)
        total = (total + s) & ((1 << 64) - 1)
    excl = np.zeros(len(a), dtype=np.uint32)
    for b in range(0, len(a), CHUNK):                   # scan_final_kernel: (uint32_t)partial[block] + the workgroup's 32-bit scan
        part = a[b:b + CHUNK].astype(np.uint64)
        inner = np.concatenate([[0], np.cumsum(part, dtype=np.uint64)[:-1]]).astype(np.uint64)
        excl[b:b + CHUNK] = ((inner + np.uint64(base[b // CHUNK] & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return excl, total


def scan_wrapping(lens):
    """The kernels while scan_partials_kernel added a chunk in uint32_t and widened the sum afterwards."""
    return _scan(lens, 32)


def scan_kernels(lens):
    """The kernels as they are: 64-bit chunk sums, so the total is exact; excl is the prefix modulo 2^32."""
    return _scan(lens, 64)


def scan_exact(lens):
    """np.cumsum in Python integers -> (excl as an object array, total)."""
    a = np.asarray(lens, dtype=np.uint32).astype(object)
    incl = np.cumsum(a) if len(a) else a
    excl = np.concatenate([[0], incl[:-1]]).astype(object) if len(a) else a
    return excl, int(incl[-1]) if len(a) else 0


def chunk_wraps(lens) -> bool:
    """Some aligned chunk sums to 2^32 or more."""
    return any(s >= LIMIT for s in _chunk_sums(lens))


def families(short: int = 1):
    """name -> (lengths, wraps): the lists of the limit tests.  A long record has LONG items, a short one `short`, a filler none.
    wraps: the wrapping scan's total is below 2^32 although the items are 2^32 or more."""
    long_, short_, none = (np.full(N_LONG, v, dtype=np.uint32) for v in (LONG, short, 0))
    behind = np.concatenate([short_, long_])
    return {
        "chunk 0 is exactly 2^32": (long_, True),
        "chunk 1 wraps behind short records": (behind, True),
        "reversed": (behind[::-1].copy(), True),
        # the same long records, half in each of two chunks behind fillers without items: refused by either scan
        "control: two chunks of 2^31": (np.concatenate([none[:N_LONG // 2], long_]), False),
    }


_SENSE = np.array([[ord(a), ord(b), ord(c)] for a in "ACGT" for b in "ACGT" for c in "ACGT" if a + b + c not in ("TAA", "TAG", "TGA")],
                  dtype=np.uint8)
SHORT_CODONS = 7                                                    # the sense codons of the short contig


def limit_batch(n_sense: int, seed: int = 2032):
    """The batch of the limit tests -> (bytes, offsets): a short contig -- TAA, SHORT_CODONS sense codons, TAA, two loose bases,
    so that the long contig's offset is neither 0 nor a multiple of 3 -- and a long one whose frame 0 of '+' is n_sense sense
    codons, TAA and three more sense codons.  Records of the long contig may overlap: 2048 of them over these 6.3 MB hold 2^32
    items."""
    rng = np.random.default_rng(seed)
    stop = np.frombuffer(b"TAA", dtype=np.uint8)
    short = np.concatenate([stop, _SENSE[rng.integers(0, len(_SENSE), size=SHORT_CODONS)].reshape(-1), stop, np.frombuffer(b"AC", dtype=np.uint8)])
    long_ = np.concatenate([_SENSE[rng.integers(0, len(_SENSE), size=n_sense)].reshape(-1), stop, _SENSE[rng.integers(0, len(_SENSE), size=3)].reshape(-1)])
    off = np.array([0, len(short), len(short) + len(long_)], dtype=np.int64)
    return np.concatenate([short, long_]), off


def message_of(error) -> str:
    """the library's own words of a KmerGutsNativeError"""
    return str(error).split(": ", 1)[1]


def records_of(lens, long_row, short_row, none_row, dtype) -> np.ndarray:
    """One record per entry of a family's lengths: long_row where it is LONG, none_row where it is 0, short_row elsewhere."""
    rows = np.zeros(3, dtype=dtype)
    rows[0], rows[1], rows[2] = long_row, short_row, none_row
    lens = np.asarray(lens)
    return rows[np.where(lens == LONG, 0, np.where(lens == 0, 2, 1))].copy()


# the list of the legal case of tests/test_gpu_coding.py: 2^31 + 2^21 items, excl passes the sign bit inside chunk 0
LEGAL = np.full(N_LONG // 2 + 1, LONG, dtype=np.uint32)
