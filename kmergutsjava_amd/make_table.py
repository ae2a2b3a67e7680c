"""Write a KmerGuts data directory from a signature list: the table placed on the GPU (kg_table_build), then saved.

    python -m kmergutsjava_amd.make_table -i SIGNATURES[.gz|-] -f FUNCTION_INDEX -D OUTDIR [-s NUM_SIGS] [-z]

OUTDIR receives kmer.table.mem_map (kmer.table.mem_map.gz with -z) and a byte-for-byte copy of FUNCTION_INDEX (as
function.index.gz when its name ends in .gz): the layout `kmer_guts -D` and KmerGutsJava.run read (KGJ:749-759).

The signature text is this project's own format (no other tool's): one signature per line,

    KMER<TAB>otuIndex<TAB>avgFromEnd<TAB>functionIndex<TAB>functionWt

KMER = 8 letters of ACDEFGHIKLMNPQRSTVWY, encoded as the reference's encodedKmer (KGJ:274-292, the inverse of
synth.decode_kmer); blank lines are skipped.  The default NUM_SIGS is the smallest prime >= 2 * signatures (a modulus
that shares a factor with 20 clusters the base-20 keys on few home slots).
"""
from __future__ import annotations

import argparse
import gzip
import os
import re
import shutil
import sys
from typing import Optional

import numpy as np

ALPHA = b"ACDEFGHIKLMNPQRSTVWY"
K = 8
_CODE = np.full(256, 255, dtype=np.uint8)
_CODE[np.frombuffer(ALPHA, dtype=np.uint8)] = np.arange(20, dtype=np.uint8)
_POW = 20 ** np.arange(K - 1, -1, -1, dtype=np.int64)       # the first letter is the most significant digit
_MAX_FIELD = 64


class SignatureFormatError(ValueError):
    def __init__(self, line: int, what: str):
        super().__init__("line %d: %s" % (line, what))
        self.line = line


def kmer_letters(v: int) -> str:
    s = []
    for _ in range(K):
        s.append(chr(ALPHA[v % 20]))
        v //= 20
    return "".join(reversed(s))


def encode_kmers(letters: np.ndarray) -> np.ndarray:
    """uint8[n, 8] letters -> int64 encodedKmer (raises ValueError on a letter outside the alphabet)."""
    codes = _CODE[letters]
    if (codes == 255).any():
        raise ValueError("letter outside %s" % ALPHA.decode())
    return codes.astype(np.int64) @ _POW


def _parse_column(strings: np.ndarray, dtype, lines: np.ndarray, what: str) -> np.ndarray:
    """numpy's vectorised string -> number conversion; on failure, bisect for the first bad entry to name its line."""
    try:
        return strings.astype(dtype)
    except (ValueError, OverflowError):
        pass
    lo, hi = 0, len(strings)                 # the first bad entry lies in [lo, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        try:
            strings[lo:mid].astype(dtype)
            lo = mid
        except (ValueError, OverflowError):
            hi = mid
    raise SignatureFormatError(int(lines[lo]), "%s is not a number: %r" % (what, strings[lo].decode("latin-1")))


def parse_signatures(data: bytes):
    """Signature text -> numpy array of _native.SIGNATURE_DTYPE (input order).  Vectorised over the whole buffer."""
    from . import _native as N
    buf = np.frombuffer(data, dtype=np.uint8)
    if buf.size and buf[-1] != 10:
        buf = np.concatenate([buf, np.array([10], dtype=np.uint8)])
    nl = np.flatnonzero(buf == 10)
    starts = np.concatenate([[0], nl[:-1] + 1]).astype(np.int64)
    ends = nl.astype(np.int64)
    cr = (ends > starts) & (buf[np.maximum(ends - 1, 0)] == 13)
    ends = ends - cr
    line_no = np.arange(1, len(starts) + 1, dtype=np.int64)
    # blank = nothing but spaces / tabs / CR
    nonblank_c = np.concatenate([[0], np.cumsum((buf != 32) & (buf != 9) & (buf != 13) & (buf != 10))])
    keep = (nonblank_c[ends] - nonblank_c[starts]) > 0
    tab_c = np.concatenate([[0], np.cumsum(buf == 9)])
    n_tabs = tab_c[ends] - tab_c[starts]
    starts, ends, line_no, n_tabs = starts[keep], ends[keep], line_no[keep], n_tabs[keep]
    n = len(starts)
    out = np.zeros(n, dtype=N.SIGNATURE_DTYPE)
    if n == 0:
        return out
    bad = np.flatnonzero(n_tabs != 4)
    if bad.size:
        raise SignatureFormatError(int(line_no[bad[0]]), "expected 5 tab-separated fields, found %d" % (int(n_tabs[bad[0]]) + 1))
    # the tabs of the kept lines, 4 per line, in order
    tabs = np.flatnonzero(buf == 9)
    tab_line = np.searchsorted(nl, tabs)                   # index of the line each tab is on
    kept_line = np.flatnonzero(keep)
    tabs = tabs[np.isin(tab_line, kept_line)].reshape(n, 4)
    bad = np.flatnonzero(tabs[:, 0] - starts != K)
    if bad.size:
        raise SignatureFormatError(int(line_no[bad[0]]), "the k-mer must be %d letters" % K)
    letters = buf[starts[:, None] + np.arange(K)]
    codes = _CODE[letters]
    bad = np.flatnonzero((codes == 255).any(axis=1))
    if bad.size:
        raise SignatureFormatError(int(line_no[bad[0]]), "k-mer %r has a letter outside %s" %
                                   (bytes(letters[bad[0]]).decode("latin-1"), ALPHA.decode()))
    out["kmer"] = codes.astype(np.int64) @ _POW
    f_start = tabs + 1                                                  # fields 2..5 start behind tabs 1..4
    f_end = np.concatenate([tabs[:, 1:], ends[:, None]], axis=1)
    widths = f_end - f_start
    bad = np.flatnonzero((widths > _MAX_FIELD).any(axis=1))
    if bad.size:
        raise SignatureFormatError(int(line_no[bad[0]]), "field longer than %d characters" % _MAX_FIELD)
    W = max(int(widths.max()), 1)
    for j, (name, dtype) in enumerate((("otuIndex", np.int64), ("avgFromEnd", np.int64), ("functionIndex", np.int64),
                                       ("functionWt", np.float64))):
        idx = f_start[:, j, None] + np.arange(W)
        mask = np.arange(W)[None, :] < widths[:, j, None]
        mat = np.zeros((n, W), dtype=np.uint8)                          # NUL padding: not part of an S string
        mat[mask] = buf[idx[mask]]
        vals = _parse_column(mat.view("S%d" % W).reshape(n), dtype, line_no, name)
        if dtype is np.int64:
            bad = np.flatnonzero((vals < -2 ** 31) | (vals >= 2 ** 31))
            if bad.size:
                raise SignatureFormatError(int(line_no[bad[0]]), "%s does not fit in 32 bits" % name)
        out[name] = vals
    return out


# ---- default table size: the smallest prime >= 2n (deterministic Miller-Rabin for 64-bit values) ----
_MR_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)           # exact for every n < 3.3e24


def is_prime(n: int) -> bool:
    if n < 2:
        return False
    for p in _MR_BASES:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in _MR_BASES:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def next_prime(n: int) -> int:
    """The smallest prime >= n."""
    n = max(n, 2)
    while not is_prime(n):
        n += 1
    return n


def default_num_sigs(n_signatures: int) -> int:
    return next_prime(2 * n_signatures)


def _read_input(path: str) -> bytes:
    if path == "-":
        data = sys.stdin.buffer.read()
    else:
        with open(path, "rb") as f:
            data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    return data


def make_table(signatures: str, function_index: str, out_dir: str, num_sigs: Optional[int] = None, gz: bool = False,
               device: int = 0) -> dict:
    """Write the data directory; returns the counts that the command line prints."""
    from . import hotpath
    sigs = parse_signatures(_read_input(signatures))
    S = default_num_sigs(len(sigs)) if num_sigs is None else int(num_sigs)
    table_name = "kmer.table.mem_map" + (".gz" if gz else "")
    fn_name = "function.index" + (".gz" if function_index.endswith(".gz") else "")
    for name in (table_name, fn_name):           # the readers take the .gz when both are there (KGJ:750-753)
        if not name.endswith(".gz") and os.path.exists(os.path.join(out_dir, name + ".gz")):
            raise FileExistsError("%s already holds %s.gz, which the readers would take instead of the new %s" % (out_dir, name, name))
    os.makedirs(out_dir, exist_ok=True)
    with hotpath.SignatureTable.build(sigs, S, device) as tab:
        placed = tab.placed
        tab.save(os.path.join(out_dir, table_name))
    shutil.copyfile(function_index, os.path.join(out_dir, fn_name))
    return {"signatures": len(sigs), "slots": S, "placed": placed, "dropped": len(sigs) - placed}


def _letters_in(msg: str) -> str:
    """The library names a k-mer by its value: add its letters."""
    return re.sub(r"(k-mer )(\d+)", lambda m: "%s%s (%s)" % (m.group(1), kmer_letters(int(m.group(2))), m.group(2))
                  if int(m.group(2)) < 20 ** K else m.group(0), msg)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.make_table",
                                 description="Build a KmerGuts signature table on the GPU and write a data directory.")
    ap.add_argument("-i", required=True, metavar="SIGNATURES", help="signature text (.gz allowed; - = stdin)")
    ap.add_argument("-f", required=True, metavar="FUNCTION_INDEX", help="function.index[.gz], copied unchanged")
    ap.add_argument("-D", required=True, metavar="OUTDIR", help="data directory to write")
    ap.add_argument("-s", type=int, default=None, metavar="NUM_SIGS", help="table slots (default: smallest prime >= 2n)")
    ap.add_argument("-z", action="store_true", help="write kmer.table.mem_map.gz")
    a = ap.parse_args(argv)
    from . import _native as N
    try:
        if a.s is not None and a.s <= 0:
            raise ValueError("-s must be positive")
        r = make_table(a.i, a.f, a.D, a.s, a.z)
    except SignatureFormatError as e:
        print("Error: %s: %s" % (a.i, e), file=sys.stderr)
        return 1
    except N.KmerGutsNativeError as e:
        print("Error: %s" % _letters_in(str(e)), file=sys.stderr)
        return 1
    except (OSError, ValueError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print("Signatures: %d, slots: %d, placed: %d, dropped: %d" % (r["signatures"], r["slots"], r["placed"], r["dropped"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
