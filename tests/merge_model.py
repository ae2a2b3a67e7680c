"""The merge rule of kg_table_merge_signatures (include/kmerguts_hip.h) restated twice: `merge_numpy` vectorised with one sort and a
neighbour compare, the exact reference the GPU tests compare with byte for byte, and `merge_dicts` with plain loops over Python
dicts, which tests/test_merge_host.py holds the first against.  Integers only; the 24 record bytes are moved, never reinterpreted.

Both take the table's resident record stream (every whole record, SIGNATURE_DTYPE), the new signatures in input order, the two
maps (or None) and the policy, and return (U in ascending k-mer order, counts) or raise MergeError with the error the library
raises first and the index or k-mer it names."""
import gzip
import struct

import numpy as np
import torch

from kmergutsjava_amd import _native as N
from kmergutsjava_amd import synth

MAX = 20 ** 8
POLICIES = ("keep", "replace", "drop")
COUNTS = ("base", "base_ignored", "added_in", "added", "conflicts", "conflicts_same_function", "replaced", "dropped", "merged")


class MergeError(ValueError):
    """kind: 'kmer' / 'fn' / 'otu' (value = the smallest offending input index), 'dup_new' / 'dup_base' (value = the smallest
    k-mer that occurs twice)."""

    def __init__(self, kind, value):
        super().__init__("%s %d" % (kind, value))
        self.kind, self.value = kind, int(value)

    def message_parts(self):
        """what the library's message must contain"""
        return {"kmer": ["signature %d:" % self.value, "is outside [0, 20^8) (the smallest such input index)"],
                "fn": ["signature %d: function_index" % self.value, "of the function map"],
                "otu": ["signature %d: otu_index" % self.value, "of the OTU map"],
                "dup_new": ["duplicate k-mer %d among the new signatures" % self.value],
                "dup_base": ["duplicate k-mer %d in the table" % self.value]}[self.kind]


def sigs(rows):
    """[(kmer, otu, avg, fn, wt), ...] -> SIGNATURE_DTYPE"""
    return np.array([tuple(r) for r in rows], dtype=N.SIGNATURE_DTYPE) if len(rows) else np.zeros(0, dtype=N.SIGNATURE_DTYPE)


def records_of_image(image: bytes):
    """a kmer.table.mem_map image -> (num_sigs of the header, the whole records that follow it)"""
    num_sigs = struct.unpack_from("<q", image, 0)[0]
    body = image[24:]
    return num_sigs, np.frombuffer(body[:len(body) // 24 * 24], dtype=N.SIGNATURE_DTYPE).copy()


def read_image(path: str) -> bytes:
    with open(path, "rb") as f:
        data = f.read()
    return gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data


def _check_new(new, fn_map, otu_map):
    k = new["kmer"]
    bad = np.flatnonzero((k < 0) | (k >= MAX))
    if bad.size:
        raise MergeError("kmer", bad[0])
    for kind, field, m in (("fn", "functionIndex", fn_map), ("otu", "otuIndex", otu_map)):
        if m is not None:
            bad = np.flatnonzero((new[field] < 0) | (new[field].astype(np.int64) >= len(m)))
            if bad.size:
                raise MergeError(kind, bad[0])


def _mapped(new, fn_map, otu_map):
    out = new.copy()
    if fn_map is not None and len(new):
        out["functionIndex"] = np.asarray(fn_map, dtype=np.int32)[new["functionIndex"]]
    if otu_map is not None and len(new):
        out["otuIndex"] = np.asarray(otu_map, dtype=np.int32)[new["otuIndex"]]
    return out


def merge_numpy(base_records, new, fn_map=None, otu_map=None, policy="keep"):
    assert policy in POLICIES
    k = base_records["kmer"]
    in_b = (k >= 0) & (k < MAX)
    B = base_records[in_b]
    _check_new(new, fn_map, otu_map)
    Nw = _mapped(new, fn_map, otu_map)
    keys = np.concatenate([B["kmer"] << 1, Nw["kmer"] << 1 | 1])
    order = np.argsort(keys, kind="stable")
    ks, rec = keys[order], np.concatenate([B, Nw])[order]
    is_new = (ks & 1) == 1
    twice = np.zeros(len(ks), dtype=bool)
    twice[1:] = ks[1:] == ks[:-1]
    for kind, sel in (("dup_new", twice & is_new), ("dup_base", twice & ~is_new)):
        if sel.any():
            raise MergeError(kind, (ks[sel] >> 1).min())
    conflict = np.zeros(len(ks), dtype=bool)            # on the base record: the new record of the same k-mer follows it
    conflict[:-1] = ~is_new[:-1] & (ks[1:] == (ks[:-1] | 1))
    met = np.zeros(len(ks), dtype=bool)                 # on the new record
    met[1:] = conflict[:-1]
    same = np.zeros(len(ks), dtype=bool)
    same[:-1] = conflict[:-1] & (rec["functionIndex"][:-1] == rec["functionIndex"][1:])
    if policy == "keep":
        keep = ~met
    elif policy == "replace":
        keep = ~conflict
    else:
        keep = ~met & (~conflict | same)
    U = rec[keep]
    c, s = int(conflict.sum()), int(same.sum())
    counts = {"base": len(B), "base_ignored": int(((k < 0) | (k == MAX)).sum()), "added_in": len(new), "added": int((is_new & ~met).sum()),
              "conflicts": c, "conflicts_same_function": s, "replaced": c if policy == "replace" else 0,
              "dropped": c - s if policy == "drop" else 0, "merged": len(U)}
    return U, counts


def merge_dicts(base_records, new, fn_map=None, otu_map=None, policy="keep"):
    """The rule read aloud: one record at a time into Python dicts."""
    first_bad = {}
    for i, r in enumerate(new):
        if not 0 <= int(r["kmer"]) < MAX:
            first_bad.setdefault("kmer", i)
        if fn_map is not None and not 0 <= int(r["functionIndex"]) < len(fn_map):
            first_bad.setdefault("fn", i)
        if otu_map is not None and not 0 <= int(r["otuIndex"]) < len(otu_map):
            first_bad.setdefault("otu", i)
    for kind in ("kmer", "fn", "otu"):
        if kind in first_bad:
            raise MergeError(kind, first_bad[kind])
    n_dict, n_twice = {}, []
    for r in new:
        r = r.copy()
        if fn_map is not None:
            r["functionIndex"] = fn_map[int(r["functionIndex"])]
        if otu_map is not None:
            r["otuIndex"] = otu_map[int(r["otuIndex"])]
        if int(r["kmer"]) in n_dict:
            n_twice.append(int(r["kmer"]))
        n_dict[int(r["kmer"])] = r
    if n_twice:
        raise MergeError("dup_new", min(n_twice))
    b_dict, b_twice, ignored = {}, [], 0
    for r in base_records:
        v = int(r["kmer"])
        if v < 0 or v == MAX:
            ignored += 1
        elif v < MAX:
            if v in b_dict:
                b_twice.append(v)
            b_dict[v] = r
    if b_twice:
        raise MergeError("dup_base", min(b_twice))
    out, c = [], dict.fromkeys(COUNTS, 0)
    for v in sorted(set(b_dict) | set(n_dict)):
        if v not in n_dict:
            out.append(b_dict[v])
        elif v not in b_dict:
            out.append(n_dict[v])
            c["added"] += 1
        else:
            c["conflicts"] += 1
            same = int(b_dict[v]["functionIndex"]) == int(n_dict[v]["functionIndex"])
            c["conflicts_same_function"] += same
            if policy == "keep" or (policy == "drop" and same):
                out.append(b_dict[v])
            elif policy == "replace":
                out.append(n_dict[v])
                c["replaced"] += 1
            else:
                c["dropped"] += 1
    c.update(base=len(b_dict), base_ignored=ignored, added_in=len(new), merged=len(out))
    U = np.array(out, dtype=N.SIGNATURE_DTYPE) if out else np.zeros(0, dtype=N.SIGNATURE_DTYPE)
    return U, c


def place(U, num_sigs: int):
    """U placed as kg_table_build places it -> (the file image, signatures placed): synth.build_table on U's own bytes"""
    raw = torch.from_numpy(np.ascontiguousarray(U).view(np.int32).reshape(-1, 6).copy())
    keys = torch.from_numpy(U["kmer"].astype(np.int64))
    payload = (raw[:, 2], raw[:, 3], raw[:, 4], raw[:, 5].contiguous().view(torch.float32))
    rec, placed = synth.build_table(keys, payload, num_sigs)
    return synth.table_image(rec), placed


def random_sigs(rng, n, universe, n_fn=4, n_otu=3):
    """n signatures with distinct k-mers drawn from `universe`, input order shuffled"""
    k = rng.choice(universe, size=min(n, len(universe)), replace=False)
    out = np.zeros(len(k), dtype=N.SIGNATURE_DTYPE)
    out["kmer"] = k
    out["otuIndex"] = rng.integers(0, n_otu, len(k))
    out["avgFromEnd"] = rng.integers(-5, 500, len(k))
    out["functionIndex"] = rng.integers(0, n_fn, len(k))
    out["functionWt"] = (1 + rng.integers(0, 64, len(k))).astype(np.float32) / 16
    return out


def random_stream(rng, n, universe, slots):
    """a record stream of `slots` records: n signatures at random slots, the rest empty, negative or 20^8"""
    rec = np.zeros(slots, dtype=N.SIGNATURE_DTYPE)
    rec["kmer"] = rng.choice([synth.EMPTY_KEY, synth.EMPTY_KEY, synth.EMPTY_KEY + 7, -1, -MAX, MAX], size=slots)
    s = random_sigs(rng, min(n, slots), universe)
    rec[rng.choice(slots, size=len(s), replace=False)] = s
    return rec
