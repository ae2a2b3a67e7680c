"""Merge the signatures of a second data directory into an existing one on the GPU (kg_table_merge_signatures), or dump a table.

    python -m kmergutsjava_amd.merge_tables -D BASE [--add NEWDIR] [-o OUTDIR] [-s NUM_SIGS] [-z]
                                            [--on-conflict keep|replace|drop] [--sigs merged.txt[.gz]]

BASE and NEWDIR are data directories as `make_table` / `make_signatures -D` write them (kmer.table.mem_map, function.index and
optionally otu.index; a .gz member wins over the plain one, as for the readers, KGJ:750-753).  At least one of -o and --sigs is
required.

Function names: BASE's function.index is read by the rules of loadIndexedArray (KGJ:345-369).  A NEWDIR name that BASE has gets
BASE's first index for it; the others are appended in NEWDIR's order, numbered on from BASE's last index.  OUTDIR's
function.index is BASE's bytes followed by the appended lines, so every index in BASE's table stays valid.  otu.index is handled
the same way when BASE has one; when it has none, NEWDIR's OTU indices are kept unmapped, no otu.index is written and one
warning line goes to stderr.

Table: NEWDIR's table is opened and exported on the device, merged into BASE's with the two maps (include/kmerguts_hip.h states
the rule; --on-conflict says what happens to a k-mer both tables hold), placed with kg_table_build_device and saved.  NUM_SIGS
defaults to max(BASE's, the smallest prime >= 2 * merged).  --sigs writes the merged signatures as `make_table -i` text; without
--add that is a dump of BASE.
"""
from __future__ import annotations

import argparse
import gzip
import os
import sys
from typing import Optional

import numpy as np

from .kmer_guts_java import load_indexed_array
from .make_signatures import signature_text
from .make_table import _letters_in, default_num_sigs

TABLE = "kmer.table.mem_map"


def _member(directory: str, name: str) -> Optional[str]:
    """The member the readers take: NAME.gz when it is there, else NAME, else None."""
    for cand in (name + ".gz", name):
        p = os.path.join(directory, cand)
        if os.path.exists(p):
            return p
    return None


def _read(path: str) -> bytes:
    with open(path, "rb") as f:
        data = f.read()
    return gzip.decompress(data) if path.endswith(".gz") else data


def _names(data: bytes):
    return load_indexed_array(data.decode("latin-1"))


def unite_names(base: bytes, new: Optional[bytes]):
    """BASE's index bytes and NEWDIR's -> (OUTDIR's bytes, int32 map from NEWDIR's indices; None without NEWDIR).  A name BASE
    has keeps BASE's first index for it; the others are appended in NEWDIR's order."""
    names = _names(base)
    if new is None:
        return base, None
    first = {}
    for i, name in enumerate(names):
        first.setdefault(name, i)
    out = [base if not base or base.endswith((b"\n", b"\r")) else base + b"\n"]
    mapping = []
    for name in _names(new):
        if name not in first:
            first[name] = len(names)
            names.append(name)
            out.append(("%d\t%s\n" % (first[name], name)).encode("latin-1"))
        mapping.append(first[name])
    return b"".join(out), np.asarray(mapping, dtype=np.int32)


class DeviceOps:
    """The device calls of one run (tests put a model in their place)."""

    def __init__(self, device: int = 0):
        self.device = device

    def export(self, table_path: str):
        """NEWDIR's table -> its signatures, resident on the device"""
        from . import hotpath
        with hotpath.SignatureTable.open(table_path, self.device) as tab:
            return tab.signatures()

    def merge(self, table_path: str, new, fn_map, otu_map, on_conflict: str):
        """-> the merged set, its kg_merge_stats, BASE's num_sigs"""
        from . import hotpath
        with hotpath.SignatureTable.open(table_path, self.device) as tab:
            u = tab.merge_signatures(None if new is None else new.device_tensor(), fn_map, otu_map, on_conflict)
            return u, u.merge_stats(), tab.info()["numSigs"]

    def place(self, u, num_sigs: int, path: str) -> int:
        from . import hotpath
        with hotpath.SignatureTable.build(u.device_tensor(), num_sigs, self.device) as tab:
            tab.save(path)
            return tab.placed

    def records(self, u) -> np.ndarray:
        return u.numpy()

    def close(self, s) -> None:
        if s is not None:
            s.close()


def merge_tables(base: str, out_dir: Optional[str] = None, add: Optional[str] = None, num_sigs: Optional[int] = None, gz: bool = False,
                 on_conflict: str = "keep", sigs_out: Optional[str] = None, device: int = 0, ops=None) -> dict:
    """Write the files; returns the counts that the command line prints."""
    if out_dir is None and sigs_out is None:
        raise ValueError("at least one of -o and --sigs is required")
    if out_dir is None and (num_sigs is not None or gz):
        raise ValueError("-s and -z need -o")
    ops = ops or DeviceOps(device)
    dirs = [("BASE", base)] + ([("NEWDIR", add)] if add is not None else [])
    tables = {}
    for what, d in dirs:
        tables[what] = _member(d, TABLE)
        if tables[what] is None:
            raise FileNotFoundError("%s holds no %s[.gz]" % (d, TABLE))
        if _member(d, "function.index") is None:
            raise FileNotFoundError("%s holds no function.index[.gz]" % d)
        if out_dir is not None and os.path.realpath(out_dir) == os.path.realpath(d):
            raise ValueError("OUTDIR is %s (%s): the merge does not write into its inputs" % (what, d))
    base_fn, base_otu = _member(base, "function.index"), _member(base, "otu.index")
    fn_bytes, fn_map = unite_names(_read(base_fn), _read(_member(add, "function.index")) if add is not None else None)
    otu_bytes, otu_map = None, None
    if base_otu is not None:
        new_otu = _member(add, "otu.index") if add is not None else None
        if add is not None and new_otu is None:
            print("Warning: %s has no otu.index: its OTU indices are kept as they are" % add, file=sys.stderr)
        otu_bytes, otu_map = unite_names(_read(base_otu), _read(new_otu) if new_otu is not None else None)
    elif add is not None:
        print("Warning: %s has no otu.index: the OTU indices of %s are kept as they are and no otu.index is written" % (base, add),
              file=sys.stderr)
    members = []                                        # (name in OUTDIR, bytes or None for the table)
    if out_dir is not None:
        members.append((TABLE + (".gz" if gz else ""), None))
        members.append(("function.index" + (".gz" if base_fn.endswith(".gz") else ""), fn_bytes))
        if otu_bytes is not None:
            members.append(("otu.index" + (".gz" if base_otu.endswith(".gz") else ""), otu_bytes))
        for name, _ in members:                         # the readers take the .gz when both are there (KGJ:750-753)
            if not name.endswith(".gz") and os.path.exists(os.path.join(out_dir, name + ".gz")):
                raise FileExistsError("%s already holds %s.gz, which the readers would take instead of the new %s" % (out_dir, name, name))
    new = u = None
    try:
        if add is not None:
            new = ops.export(tables["NEWDIR"])
        u, st, base_slots = ops.merge(tables["BASE"], new, fn_map, otu_map, on_conflict)
        r = {k: int(st[k]) for k in ("base", "base_ignored", "added_in", "added", "conflicts", "conflicts_same_function", "replaced",
                                     "dropped", "merged")}
        r["slots"] = r["placed"] = None
        if sigs_out is not None:
            text = signature_text(ops.records(u)).encode()
            with (gzip.open(sigs_out, "wb") if sigs_out.endswith(".gz") else open(sigs_out, "wb")) as f:
                f.write(text)
        if out_dir is not None:
            S = max(int(base_slots), default_num_sigs(r["merged"])) if num_sigs is None else int(num_sigs)
            os.makedirs(out_dir, exist_ok=True)
            r["slots"], r["placed"] = S, int(ops.place(u, S, os.path.join(out_dir, members[0][0])))
            for name, data in members[1:]:
                with (gzip.open if name.endswith(".gz") else open)(os.path.join(out_dir, name), "wb") as f:
                    f.write(data)
    finally:
        ops.close(u)
        ops.close(new)
    return r


def summary_line(r: dict) -> str:
    line = "Base: %d (ignored %d), new: %d, added: %d, conflicts: %d (same function: %d), replaced: %d, dropped: %d, merged: %d" % (
        r["base"], r["base_ignored"], r["added_in"], r["added"], r["conflicts"], r["conflicts_same_function"], r["replaced"], r["dropped"],
        r["merged"])
    if r["slots"] is not None:                          # (without -o no table is placed)
        line += ", slots: %d, placed: %d, dropped at the end: %d" % (r["slots"], r["placed"], r["merged"] - r["placed"])
    return line


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmergutsjava_amd.merge_tables",
                                 description="Merge the signatures of a data directory into another on the GPU, or dump a table.")
    ap.add_argument("-D", required=True, metavar="BASE", help="the data directory to merge into (not modified)")
    ap.add_argument("--add", default=None, metavar="NEWDIR", help="the data directory whose signatures are added")
    ap.add_argument("-o", default=None, metavar="OUTDIR", help="data directory to write")
    ap.add_argument("-s", type=int, default=None, metavar="NUM_SIGS", help="table slots (default: max(BASE's, smallest prime >= 2 * merged))")
    ap.add_argument("-z", action="store_true", help="write kmer.table.mem_map.gz")
    ap.add_argument("--on-conflict", default="keep", choices=("keep", "replace", "drop"),
                    help="a k-mer in both tables: keep BASE's record (default), replace it, or drop both unless they name the same function")
    ap.add_argument("--sigs", default=None, metavar="TEXT", help="also write the merged signatures as make_table -i text (.gz allowed)")
    a = ap.parse_args(argv)
    from . import _native as N
    try:
        if a.s is not None and a.s <= 0:
            raise ValueError("-s must be positive")
        r = merge_tables(a.D, a.o, a.add, a.s, a.z, a.on_conflict, a.sigs)
    except N.KmerGutsNativeError as e:
        print("Error: %s" % _letters_in(str(e)), file=sys.stderr)
        return 1
    except (OSError, ValueError, IndexError) as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    print(summary_line(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
