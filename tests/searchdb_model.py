"""The file form of a kg_searchdb restated in numpy, from the header's statement of the format (include/kmerguts_hip.h) and from
the existing models alone: seed_model's seed ids, ungapped_model's first positions, mask_model's seeding copy.  write() makes the
bytes kg_searchdb_save must write for the same targets; read() takes a file apart; checksum() is the header's definition."""
from __future__ import annotations

import struct

import numpy as np

import mask_model as MK
import seed_model as SD
import ungapped_model as UM

MAGIC = b"KGSRCHDB"
VERSION, HEADER_BYTES, ALIGN, CHECKED = 1, 448, 64, 360
AT_SEEDS, AT_MASK, AT_MASK_STATS, AT_SECTIONS, AT_CHECKSUM = 72, 120, 136, 216, 360
SECTIONS = ("offsets", "residues", "pairs", "values", "run_starts", "names")
MASK_STAT_KEYS = ("proteins", "residues", "windows", "low_windows", "ext_windows", "masking_windows", "segments", "masked_residues",
                  "proteins_masked")
COUNTS = ("n_db", "residues", "pairs", "kmers", "valid_windows", "names_bytes")      # the header's i64 fields from byte 16 on


def checksum(data: bytes) -> int:
    """(sum of w_i * (2 i + 1) + len) mod 2^64 over the little-endian u64 words of data padded with zero bytes."""
    n = len(data)
    w = np.frombuffer(bytes(data) + b"\0" * (-n % 8), dtype="<u8")
    with np.errstate(over="ignore"):
        s = int((w * (2 * np.arange(w.size, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64)) if w.size else 0
    return (s + n) % (1 << 64)


def bits_for(n: int) -> int:
    return (n - 1).bit_length() if n > 1 else 0


def pairs_of(seq: bytes, offsets, seed=None, mask=None):
    """The index's arrays for targets seq / offsets (offsets[0] = 0): pk u64, pv u32, run starts u32, the valid windows and the
    mask's counts (None without a mask).  seed: (cls, masks) of seed_model or None for the exact 8-mers; mask: None or a dict of
    window, trigger, extend."""
    off = np.asarray(offsets, dtype=np.int64)
    n_db = off.size - 1
    seed = SD.EXACT if seed is None else seed
    seeding, mcounts = bytes(seq), None
    if mask is not None:
        flags, _, _, mcounts = MK.mask_numpy(seq, off, mask["window"], mask["trigger"], mask["extend"])
        seeding = MK.soft_mask(seq, off, flags)
    v, p, x = UM.first_positions_numpy(seeding, off, seed)
    valid = 0
    for k in range(n_db):                                  # every valid (window, shape), one protein at a time
        prot = seeding[int(off[k]):int(off[k + 1])]
        valid += _valid_windows(prot, seed)
    pk = (v.astype(np.uint64) << np.uint64(bits_for(n_db))) | p.astype(np.uint64)
    pv = (np.diff(off)[p] - x).astype(np.uint32)
    head = np.r_[True, v[1:] != v[:-1]] if v.size else np.zeros(0, dtype=bool)
    starts = np.r_[np.flatnonzero(head), v.size].astype(np.uint32)
    return pk, pv, starts, valid, mcounts


def _valid_windows(p: bytes, seed) -> int:
    cls, masks = seed
    code = set(SD.ALPHA)
    n = 0
    for mask in masks:
        care = [j for j in range(32) if mask >> j & 1]
        for i in range(len(p)):
            if i + SD.span(mask) < len(p) and all(p[i + j] in code for j in care):
                n += 1
    return n


def seed_bytes(seed) -> bytes:
    """struct kg_seed_params, 48 bytes."""
    cls, masks = seed
    return struct.pack("<ii20B4Ii", len(masks), SD.alphabet_size(cls), *cls, *(list(masks) + [0] * (4 - len(masks))), 0)


def assemble(counts: dict, sections: dict, seed_raw: bytes = b"", mask_raw: bytes = b"", mask_stats_raw: bytes = b"") -> bytes:
    """A file from its parts: the header's counts, the six sections' bytes, and the raw parameter blocks (empty: absent)."""
    at, places, body = HEADER_BYTES, [], b""
    for name in SECTIONS:
        data = sections[name]
        places.append((at, len(data), checksum(data)))
        padded = data + b"\0" * (-(at + len(data)) % ALIGN)
        body += padded
        at += len(padded)
    hdr = bytearray(HEADER_BYTES)
    hdr[0:8] = MAGIC
    struct.pack_into("<II", hdr, 8, VERSION, HEADER_BYTES)
    struct.pack_into("<6q", hdr, 16, *(counts[k] for k in COUNTS))
    struct.pack_into("<II", hdr, 64, 1 if seed_raw else 0, 1 if mask_raw else 0)
    hdr[AT_SEEDS:AT_SEEDS + len(seed_raw)] = seed_raw
    hdr[AT_MASK:AT_MASK + len(mask_raw)] = mask_raw
    hdr[AT_MASK_STATS:AT_MASK_STATS + len(mask_stats_raw)] = mask_stats_raw
    for k, (a, n, c) in enumerate(places):
        struct.pack_into("<QQQ", hdr, AT_SECTIONS + 24 * k, a, n, c)
    struct.pack_into("<Q", hdr, AT_CHECKSUM, checksum(bytes(hdr[:CHECKED])))
    return bytes(hdr) + body


def write(seq: bytes, offsets, seed=None, mask=None, names: bytes = b"") -> bytes:
    """The file of the targets seq / offsets built with seed (None: exact) and mask (None, or window / trigger / extend)."""
    off = np.asarray(offsets, dtype=np.int64)
    seq = bytes(seq)[int(off[0]):int(off[-1])]
    off = off - off[0]
    pk, pv, starts, valid, mcounts = pairs_of(seq, off, seed, mask)
    counts = dict(n_db=off.size - 1, residues=len(seq), pairs=int(pk.size), kmers=int(starts.size - 1), valid_windows=valid,
                  names_bytes=len(names))
    sections = dict(offsets=off.astype("<i8").tobytes(), residues=seq, pairs=pk.astype("<u8").tobytes(), values=pv.astype("<u4").tobytes(),
                    run_starts=starts.astype("<u4").tobytes(), names=bytes(names))
    mask_raw = struct.pack("<4i", mask["window"], mask["trigger"], mask["extend"], 0) if mask is not None else b""
    stats_raw = struct.pack("<9qfi", *(mcounts[k] for k in MASK_STAT_KEYS), 0.0, 0) if mask is not None else b""
    return assemble(counts, sections, seed_bytes(seed) if seed is not None else b"", mask_raw, stats_raw)


def read(data: bytes) -> dict:
    """A file's counts, flags, raw parameter blocks and sections ({name: bytes}); asserts what the header's statement fixes."""
    assert data[:8] == MAGIC and struct.unpack_from("<II", data, 8) == (VERSION, HEADER_BYTES)
    assert struct.unpack_from("<Q", data, AT_CHECKSUM)[0] == checksum(data[:CHECKED])
    counts = dict(zip(COUNTS, struct.unpack_from("<6q", data, 16)))
    has_seeds, has_mask = struct.unpack_from("<II", data, 64)
    sections, at = {}, HEADER_BYTES
    for k, name in enumerate(SECTIONS):
        a, n, c = struct.unpack_from("<QQQ", data, AT_SECTIONS + 24 * k)
        assert a == at and checksum(data[a:a + n]) == c
        sections[name] = data[a:a + n]
        at = a + n + (-(a + n) % ALIGN)
        assert not any(data[a + n:at])
    assert at == len(data)
    return dict(counts=counts, has_seeds=has_seeds, has_mask=has_mask, seeds=data[AT_SEEDS:AT_MASK], mask=data[AT_MASK:AT_MASK_STATS],
                mask_stats=data[AT_MASK_STATS:AT_SECTIONS], sections=sections)
