"""Python face of the C ABI: the signature table resident in HBM and one scan of a batch.

Replaces, for a batch of sequences, the reference's prepareQuery/addKmers -> sort -> lookup ->
gatherHits/processSetOfHits chain (KGJ:1051-1074, 900-922, 1076-1095, 944-1034, 385-514;
"KGJ:n" = reference lib/src/kmergutsjava/KmerGutsJava.java line n).  All arithmetic happens in
libkmerguts_hip.so on the GPU; this file only moves pointers.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native as N


@dataclass
class Params:
    """The instance fields the hot path reads (KGJ:102-106)."""
    aa: bool = False
    order_constraint: bool = False
    min_hits: int = 5
    min_weighted_hits: int = 0
    max_gap: int = 200
    counters: bool = False
    skip_aggregate: bool = False
    progress: bool = False          # KG_F_PROGRESS: ScanResult.progress() / .hit_slots() (the "Processed: NN%" lines, KGJ:1016-1025)

    def to_native(self) -> N.KgParams:
        flags = ((N.KG_F_COUNTERS if self.counters else 0) | (N.KG_F_SKIP_AGGREGATE if self.skip_aggregate else 0) |
                 (N.KG_F_PROGRESS if self.progress else 0))
        return N.KgParams(int(self.aa), int(self.order_constraint), int(self.min_hits),
                          int(self.min_weighted_hits), int(self.max_gap), flags)


class _DevMem:
    """`count` items of `typestr` at a raw HBM address, exposed through __cuda_array_interface__ (version 2)."""

    def __init__(self, ptr: int, count: int, typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 2,
                                         "strides": None}
        self._owner = owner


def device_tensor(ptr: int, count: int, typestr: str = "|u1", owner=None, device: Optional[int] = None):
    """torch tensor over library-owned device memory (no copy).  `owner` is kept alive by the tensor."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    if count == 0 or not ptr:
        return torch.empty(0, dtype=torch.uint8 if typestr == "|u1" else torch.int64, device=dev)
    t = torch.as_tensor(_DevMem(ptr, count, typestr, owner), device=dev)
    t._kg_owner = owner
    return t


def _ptr(a):
    """The address of a numpy array's elements for the library; None for an array of none (and for None)."""
    return a.ctypes.data if a is not None and a.size else None


def _offsets(offsets, text: str, n: Optional[int] = None) -> np.ndarray:
    """offsets as contiguous int64: one-dimensional and not empty, or with n exactly n + 1 entries; `text` says what they must be."""
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    if (off.ndim != 1 or off.size < 1) if n is None else off.shape != (n + 1,):
        raise ValueError("offsets must be " + text)
    return off


def _seq_bytes(seq, off, no_sequence_too: bool = False) -> np.ndarray:
    """The batch's bytes (bytes-like or an ndarray) as contiguous uint8, at least offsets[-1] of them; when there is no sequence
    offsets[-1] is looked at only with no_sequence_too."""
    arr = np.frombuffer(seq, dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq
    arr = np.ascontiguousarray(arr.view(np.uint8).reshape(-1))
    if (off.size > 1 or no_sequence_too) and arr.size < int(off[-1]):
        raise ValueError("sequence buffer shorter than offsets[-1]")
    return arr


def _signature_arg(sigs):
    """The signatures SignatureTable.build / merge_signatures are given: a contiguous CUDA tensor of 24 * n bytes, or a numpy
    array of _native.SIGNATURE_DTYPE or raw bytes of 24-byte records.  -> (the records are on the device, their address or None
    for none, n, what keeps them alive for the call)."""
    if hasattr(sigs, "is_cuda") and sigs.is_cuda:
        if not sigs.is_contiguous():
            raise ValueError("the signature tensor must be contiguous")
        nbytes = sigs.numel() * sigs.element_size()
        if nbytes % 24:
            raise ValueError("the signature tensor must hold 24 * n bytes")
        return True, C.c_void_p(sigs.data_ptr() if nbytes else None), nbytes // 24, sigs
    arr = sigs if isinstance(sigs, np.ndarray) else np.frombuffer(sigs, dtype=np.uint8)
    arr = np.ascontiguousarray(arr)
    if arr.dtype != N.SIGNATURE_DTYPE:
        arr = arr.reshape(-1).view(np.uint8)
        if arr.size % 24:
            raise ValueError("signature bytes must be a multiple of 24")
    n = arr.nbytes // 24
    return False, _ptr(arr), n, arr


def _copy_records(copy, h, n: int, dtype, shape=(), device_out: bool = False):
    """Records [0, n) of a set, each `shape` elements of `dtype`, through the set's range getter `copy`.  -> a numpy array
    of (n,) + shape; or with device_out a CUDA tensor: uint8 of itemsize bytes per record for a record dtype, the typed
    (n,) + shape tensor for a plain one."""
    dtype = np.dtype(dtype)
    if not device_out:
        a = np.zeros((n,) + tuple(shape), dtype=dtype)
        N.check(copy(h, 0, n, _ptr(a)))
        return a
    import torch
    if dtype.names:
        a = torch.empty(n * dtype.itemsize, dtype=torch.uint8, device="cuda")
    else:
        a = torch.empty((n,) + tuple(shape), dtype=getattr(torch, dtype.name), device="cuda")
    torch.cuda.synchronize()            # the library works on its own stream
    N.check(copy(h, 0, n, C.c_void_p(a.data_ptr() if n else None)))
    return a


class _OrfChain:
    """Owns the kg_orfset at the head of a chain of ORF steps (`h`, null when there is none).  Every step makes a new set from
    the current one, which is then freed whether the step failed or not: the new set holds copies and lives in the same
    context.  release() passes the set on (to _take_orfset, which frees it); close() frees what is still held."""

    def __init__(self, lib):
        self.lib, self.h = lib, C.c_void_p()

    def step(self, call) -> None:
        """call(the current set, byref(the new set)) -> the library's return code."""
        old, self.h = self.h, C.c_void_p()
        try:
            N.check(call(old, C.byref(self.h)))
        finally:
            if old:
                self.lib.kg_orfset_free(old)

    def release(self):
        h, self.h = self.h, C.c_void_p()
        return h

    def close(self) -> None:
        if self.h:
            self.lib.kg_orfset_free(self.release())


class _GeneSteps:
    """regions(), orfs() and select() of a holder of DNA CALL records, and the ORF steps the latter two share.  A subclass says
    where the CALLs are: _need() (the library, or an error when the holder is closed), _n_seqs(), _regions_call (the region set
    of its CALLs) and _repair_call (kg_regionset_repair, or its twin, with its CALLs)."""

    def regions(self, offsets, merge_gap: int = 600, min_score: int = 0, min_len: int = 0, device_out: bool = False):
        """The CALL records of a DNA result merged into function regions in contig coordinates, on the GPU
        (include/kmerguts_hip.h kg_result_regions states the rule).  offsets: the int64[n_seqs + 1] the scan was given.
        -> (records, region_start): records a numpy array of _native.REGION_DTYPE in output order, or with device_out=True a
        CUDA uint8 tensor of 48 bytes per region; region_start int64[n_seqs + 1], contig s owning records
        [region_start[s], region_start[s + 1]).  The call's counts and device time are left in `region_stats`."""
        lib = self._need()
        off = _offsets(offsets, "the int64[n_seqs + 1] the scan was given", self._n_seqs())
        p = N.KgRegionParams(int(merge_gap), int(min_score), int(min_len))
        h = C.c_void_p()
        N.check(self._regions_call(lib, p, off, h))
        out, start, self.region_stats = _take_regionset(h, self._n_seqs(), device_out)
        return out, start

    def orfs(self, seq, offsets, merge_gap: int = 600, min_score: int = 0, min_len: int = 0, start_codons: int = 7,
             only_kept: bool = True, device_ptr: Optional[int] = None, free_min_res: Optional[int] = None, coding=None,
             min_coding: int = 0, min_train_pairs: int = 100000, starts=None, start_min_res: int = 100, start_rounds: int = 4,
             min_train_starts: int = 200, repair: bool = False, repair_min_count: int = 0, max_junctions: int = 4):
        """regions() and then the open reading frame around every region with its translated protein, on the GPU, without a
        host trip between the two (include/kmerguts_hip.h kg_regionset_orfs states the rule).  seq / offsets: what the scan was
        given; device_ptr: the address of the bytes in HBM instead of seq.
        -> (regions, region_start, orfs, prot_start, residues): orfs a numpy array of _native.ORF_DTYPE, index-aligned with
        regions; the protein of ORF i is residues[prot_start[i] : prot_start[i + 1]] (uint8).  The two calls' counts and device
        times are left in `region_stats` and `orf_stats`.
        free_min_res: when given, the evidence-free candidates of at least that many residues (kg_orfset_add_free, flag
        _native.ORF_FREE) follow the regions' ORFs in orfs, prot_start and residues; `orf_stats` is then the whole set's.
        coding: None (or False: off), True or an int32[4096] score table (coding_table): every record is scored by its in-frame hexamer
        log-odds and a free ORF below min_coding loses kept and gains _native.ORF_NONCODING (kg_orfset_coding, after
        free_min_res); True trains on the set's own evidence ORFs when they have min_train_pairs codon pairs.  The scores
        (int64 per record), the statistics and the counts of an own training are left in `coding_scores`, `coding_stats` and
        `coding_model`.
        starts: None (or False: off), True or a (pos int32[20][4], type int32[4]) weights pair (start_weights): the start codon of
        every movable record is chosen by the start-site score (kg_orfset_starts, after coding, which it needs: the score's
        coding half is the coding step's table).  True trains on the set's own evidence ORFs in start_rounds rounds when there
        are min_train_starts of them; when the coding step was untrained, so are the starts.  The regions bound the evidence
        ORFs' moves, start_min_res everything else.  The shifts in codons (int32 per record), the statistics and the last
        round's counts are left in `start_shifts`, `start_stats` and `start_model`; `coding_scores` are then the new set's.
        repair: the record and protein of every kept multi-frame region are replaced by the chain through its frames
        (kg_result_repair, before free_min_res, so every later step sees the new extents; flag _native.ORF_REPAIRED).  CALLs
        below repair_min_count take no part in a chain; a region of more than max_junctions + 1 segments is left alone.  The
        junction records (_native.JUNCTION_DTYPE), junction_start int64[n_regions + 1] and the statistics are left in
        `junctions`, `junction_start` and `repair_stats`."""
        lib = self._need()
        coding = _coding_arg(coding)
        starts = _starts_arg(starts, coding)
        off = _offsets(offsets, "the int64[n_seqs + 1] the scan was given", self._n_seqs())
        p = N.KgRegionParams(int(merge_gap), int(min_score), int(min_len))
        h, chain = C.c_void_p(), _OrfChain(lib)
        N.check(self._regions_call(lib, p, off, h))
        try:
            self._orf_steps(chain, h, seq, device_ptr, off, start_codons, only_kept, repair, repair_min_count, max_junctions, free_min_res,
                            coding, min_coding, min_train_pairs, starts, start_min_res, start_rounds, min_train_starts)
            orfs, prot_start, residues, self.orf_stats = _take_orfset(chain.release(), False)
        except BaseException:
            chain.close()
            lib.kg_regionset_free(h)
            raise
        regs, start, self.region_stats = _take_regionset(h, self._n_seqs(), False)
        return regs, start, orfs, prot_start, residues

    def select(self, offsets, seq=None, merge_gap: int = 600, min_score: int = 0, min_len: int = 0, orfs: bool = False,
               start_codons: int = 7, only_kept: bool = True, device_ptr: Optional[int] = None, max_overlap: int = 60,
               max_overlap_pct: int = 50, free_min_res: Optional[int] = None, coding=None, min_coding: int = 0,
               min_train_pairs: int = 100000, starts=None, start_min_res: int = 100, start_rounds: int = 4,
               min_train_starts: int = 200, repair: bool = False, repair_min_count: int = 0, max_junctions: int = 4):
        """regions() -- with orfs=True, orfs() -- and then the non-overlapping selection among the kept records, on the GPU and
        without a host trip or a second scan in between (include/kmerguts_hip.h kg_regionset_select states the rule).  The
        candidates are the regions' extents, or with orfs=True the ORFs' extents.
        -> (regions, region_start, selection), or with orfs=True (regions, region_start, orfs, prot_start, residues, selection):
        selection a numpy array of _native.SELECTION_DTYPE, index-aligned with the regions (and the ORFs).  The calls' counts and
        device times are left in `region_stats`, `orf_stats` and `select_stats`.
        free_min_res (with orfs=True): the evidence-free candidates are appended on the device before the selection, as orfs()
        appends them; orfs, prot_start, residues and selection then hold them behind the regions' records.
        coding, min_coding, min_train_pairs (with orfs=True): as orfs() takes them, applied after free_min_res and before the
        selection, so a non-coding free ORF is not eligible and suppresses nothing.
        starts, start_min_res, start_rounds, min_train_starts (with coding): as orfs() takes them, applied after coding and before
        the selection, which therefore sees the new extents.
        repair, repair_min_count, max_junctions (with orfs=True): as orfs() takes them, applied before free_min_res."""
        lib = self._need()
        if free_min_res is not None and not orfs:
            raise ValueError("free_min_res needs orfs=True: the free candidates are ORFs")
        coding = _coding_arg(coding)
        if coding is not None and not orfs:
            raise ValueError("coding needs orfs=True: the scores are the ORFs'")
        if repair and not orfs:
            raise ValueError("repair needs orfs=True: it rewrites ORFs")
        starts = _starts_arg(starts, coding)
        off = _offsets(offsets, "the int64[n_seqs + 1] the scan was given", self._n_seqs())
        p = N.KgRegionParams(int(merge_gap), int(min_score), int(min_len))
        sp = N.KgSelectParams(int(max_overlap), int(max_overlap_pct), 0)
        h, sh, chain = C.c_void_p(), C.c_void_p(), _OrfChain(lib)
        N.check(self._regions_call(lib, p, off, h))
        try:
            if orfs:
                self._orf_steps(chain, h, seq, device_ptr, off, start_codons, only_kept, repair, repair_min_count, max_junctions,
                                free_min_res, coding, min_coding, min_train_pairs, starts, start_min_res, start_rounds, min_train_starts)
                N.check(lib.kg_orfset_select(chain.h, C.byref(sp), C.byref(sh)))
            else:
                N.check(lib.kg_regionset_select(h, C.byref(sp), C.byref(sh)))
            taken, sh = sh, C.c_void_p()                # (_take_* frees what it is given, also when it raises)
            sel, self.select_stats = _take_selectset(taken, False)      # a select set is freed before the set it came from
            if orfs:
                orf_recs, prot_start, residues, self.orf_stats = _take_orfset(chain.release(), False)
        except BaseException:
            if sh:
                lib.kg_selectset_free(sh)
            chain.close()
            lib.kg_regionset_free(h)
            raise
        regs, start, self.region_stats = _take_regionset(h, self._n_seqs(), False)
        if orfs:
            return regs, start, orf_recs, prot_start, residues, sel
        return regs, start, sel

    def _orf_steps(self, chain, rh, seq, device_ptr, off, start_codons, only_kept, repair, repair_min_count, max_junctions, free_min_res,
                   coding, min_coding, min_train_pairs, starts, start_min_res, start_rounds, min_train_starts):
        """The steps of orfs() and select(orfs=True) behind the region set rh, each on the set the one before it left in `chain`:
        kg_regionset_orfs, then kg_result_repair, kg_orfset_add_free, kg_orfset_coding and kg_orfset_starts where they are asked
        for (coding and starts: what _coding_arg and _starts_arg gave).  The steps' side results go into self."""
        lib = chain.lib
        keep = None if device_ptr is not None else _seq_bytes(seq, off)        # (alive while the steps read it)
        batch = (C.c_void_p(device_ptr) if keep is None else _ptr(keep), int(keep is None), off.ctypes.data, off.size - 1)
        op = N.KgOrfParams(int(start_codons), int(bool(only_kept)), 0)
        chain.step(lambda oh, new: lib.kg_regionset_orfs(rh, C.byref(op), *batch, new))
        if repair:
            rp = N.KgRepairParams(int(start_codons), int(repair_min_count), int(max_junctions), 0)
            chain.step(lambda oh, new: self._repair_call(lib, rh, oh, rp, batch, new))
            self.junctions, self.junction_start, self.repair_stats = _junctions(chain.h)
        if free_min_res is not None:
            fp = N.KgFreeParams(int(free_min_res), int(start_codons), 0)
            chain.step(lambda oh, new: lib.kg_orfset_add_free(oh, C.byref(fp), *batch, new))
        if coding is not None:
            cp = N.KgCodingParams(int(min_coding), 0, int(min_train_pairs))
            chain.step(lambda oh, new: lib.kg_orfset_coding(oh, C.byref(cp), None if coding is True else coding.ctypes.data, *batch, new))
            self.coding_scores, self.coding_stats, self.coding_model = _coding_results(chain.h)
        if starts is not None:
            table = coding
            if coding is True:
                # the table the coding step trained and used; none when it was untrained, and then the starts are untrained too
                trained = self.coding_stats["trained"] != 0
                table = coding_table(*self.coding_model) if trained else np.zeros(N.CODING_BINS, dtype=np.int32)
                if not trained and starts is True:
                    min_train_starts = 1 << 62
            sp = N.KgStartParams(int(start_min_res), int(start_codons), int(start_rounds), 0, int(min_train_starts))
            chain.step(lambda oh, new: lib.kg_orfset_starts(oh, C.byref(sp), table.ctypes.data, None if starts is True else C.addressof(starts),
                                                            rh, *batch, new))
            self.start_shifts, self.start_stats, self.start_model = _starts_results(chain.h)
            self.coding_scores = _coding_results(chain.h)[0]


class ScanResult(_GeneSteps):
    """Owns one kg_result.  Record arrays are numpy structured arrays (copies)."""

    def __init__(self, handle: int, table=None):
        self._h = C.c_void_p(handle)
        self._table = table              # a result must be freed before its table (kg_result_free uses the table's caches)
        st = N.KgStats()
        N.check(N.load().kg_result_stats(self._h, C.byref(st)))
        self.stats = st.as_dict()

    def _n_seqs(self) -> int:
        return self.stats["n_seqs"]

    def _regions_call(self, lib, p, off, h):
        return lib.kg_result_regions(self._h, C.byref(p), off.ctypes.data, C.byref(h))

    def _repair_call(self, lib, rh, oh, rp, batch, new):
        return lib.kg_result_repair(self._h, rh, oh, C.byref(rp), *batch, new)

    def _need(self):
        if not self._h:
            raise ValueError("ScanResult is closed")
        return N.load()

    def hits(self, copy: bool = True) -> np.ndarray:
        """Hit records ordered by (container, from0InProt).  copy=False: zero-copy view of the library's pinned
        buffer, valid until close()."""
        lib = self._need()
        return N.view(lib.kg_result_hits(self._h), self.stats["n_hits"], N.HIT_DTYPE, None if copy else self)

    def copy_hits(self, first: int = 0, count: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """hits[first : first + count] into caller-owned memory (a new array unless `out` is given)."""
        lib = self._need()
        count = self.stats["n_hits"] - first if count is None else count
        if out is None:
            out = np.empty(count, dtype=N.HIT_DTYPE)
        assert out.dtype == N.HIT_DTYPE and out.flags.c_contiguous and len(out) >= count
        N.check(lib.kg_result_copy_hits(self._h, first, count, out.ctypes.data if count else None))
        return out[:count]

    def container_hit_start(self) -> np.ndarray:
        lib = self._need()
        return N.view(lib.kg_result_container_hit_start(self._h), self.stats["n_containers"] + 1, np.dtype("<i8"))

    def calls(self, copy: bool = True) -> np.ndarray:
        lib = self._need()
        return N.view(lib.kg_result_calls(self._h), self.stats["n_calls"], N.CALL_DTYPE, None if copy else self)

    def container_call_start(self) -> np.ndarray:
        lib = self._need()
        return N.view(lib.kg_result_container_call_start(self._h), self.stats["n_containers"] + 1, np.dtype("<i8"))

    def otu(self, copy: bool = True) -> np.ndarray:
        lib = self._need()
        return N.view(lib.kg_result_otu(self._h), self.stats["n_seqs"], N.OTU_DTYPE, None if copy else self)

    def hit_events(self) -> np.ndarray:
        """One KG_EV_* byte per hit record: what gatherHits did there (for the -d stream)."""
        lib = self._need()
        return N.view(lib.kg_result_hit_events(self._h), self.stats["n_hits"], np.dtype("u1"))

    def container_tail_events(self) -> np.ndarray:
        lib = self._need()
        return N.view(lib.kg_result_container_tail_events(self._h), self.stats["n_containers"], np.dtype("u1"))

    def hit_slots(self) -> np.ndarray:
        """KG_F_PROGRESS scans: the table slot every hit record was found at (uint32, parallel to hits())."""
        lib = self._need()
        ptr = lib.kg_result_hit_slots(self._h)
        if not ptr and self.stats["n_hits"]:
            raise N.KmerGutsNativeError(-1, (lib.kg_last_error() or b"").decode())
        return N.view(ptr, self.stats["n_hits"], np.dtype("<u4"))

    def progress(self) -> dict:
        """KG_F_PROGRESS scans: kg_progress as a dict (first slot visited per tenth of the table, last slot visited, first
        home slot behind the end of a short table stream, whether a walk ran off its end, records in the stream)."""
        lib = self._need()
        p = N.KgProgress()
        N.check(lib.kg_result_progress(self._h, C.byref(p)))
        return p.as_dict()

    def device_hits_ptr(self) -> int:
        return self._need().kg_result_device_hits(self._h) or 0

    def device_calls_ptr(self) -> int:
        return self._need().kg_result_device_calls(self._h) or 0

    def device_otu_ptr(self) -> int:
        return self._need().kg_result_device_otu(self._h) or 0

    def device_view(self, what: str):
        """Zero-copy torch view (uint8, or int64 for the two start arrays) of a record array where the library left
        it in HBM: "hits", "calls", "otu", "container_hit_start", "container_call_start".  Valid until close();
        plumbing for callers that keep working on the device (RCCL gather, on-device comparisons)."""
        lib = self._need()
        st = self.stats
        n_cont = st["n_containers"]
        spec = {"hits": (lib.kg_result_device_hits, st["n_hits"] * N.HIT_DTYPE.itemsize, "|u1"),
                "calls": (lib.kg_result_device_calls, st["n_calls"] * N.CALL_DTYPE.itemsize, "|u1"),
                "otu": (lib.kg_result_device_otu, st["n_seqs"] * N.OTU_DTYPE.itemsize, "|u1"),
                "container_hit_start": (lib.kg_result_device_container_hit_start, n_cont + 1, "<i8"),
                "container_call_start": (lib.kg_result_device_container_call_start, n_cont + 1, "<i8")}[what]
        return device_tensor(spec[0](self._h) or 0, spec[1], spec[2], owner=self)

    def subset(self, seq_idx, events: bool = False) -> dict:
        """The records of the sequences seq_idx (ascending indices into the batch), renumbered as if those sequences
        had been scanned as a batch of their own: legal because every sequence is independent (hits depend on its own
        k-mers and the table only, the aggregation state is per sequence, KGJ:528, 540).  The hit records are sliced
        where they are (HBM) and only the slices come to the host."""
        import torch
        st = self.stats
        idx = np.asarray(seq_idx, dtype=np.int64)
        per = st["n_containers"] // st["n_seqs"] if st["n_seqs"] else 1
        chs, ccs = self.container_hit_start(), self.container_call_start()
        cont = (idx[:, None] * per + np.arange(per)[None, :]).reshape(-1)               # old container ids, in order
        h_n = chs[cont + 1] - chs[cont]
        c_n = ccs[cont + 1] - ccs[cont]
        new_chs = np.zeros(len(cont) + 1, dtype=np.int64); np.cumsum(h_n, out=new_chs[1:])
        new_ccs = np.zeros(len(cont) + 1, dtype=np.int64); np.cumsum(c_n, out=new_ccs[1:])
        dv = self.device_view("hits").view(torch.int32).view(-1, 6)
        # the containers of one sequence are adjacent in hits[]: one slice per sequence
        parts = [dv[int(chs[i * per]):int(chs[i * per + per])] for i in idx]
        hits = (torch.cat(parts).cpu().numpy() if parts else np.zeros((0, 6), np.int32)).reshape(-1).view(N.HIT_DTYPE).copy()
        hits["container"] = np.repeat(np.arange(len(cont), dtype=np.uint32), h_n)
        allc = self.calls()
        calls = (np.concatenate([allc[int(ccs[i * per]):int(ccs[i * per + per])] for i in idx]) if len(idx)
                 else np.zeros(0, N.CALL_DTYPE))
        calls["container"] = np.repeat(np.arange(len(cont), dtype=np.uint32), c_n)
        out = {"hits": hits, "container_hit_start": new_chs, "calls": calls, "container_call_start": new_ccs,
               "otu": self.otu()[idx]}
        if events:
            ev = self.hit_events()
            out["hit_events"] = (np.concatenate([ev[int(chs[i * per]):int(chs[i * per + per])] for i in idx]) if len(idx)
                                 else np.zeros(0, np.uint8))
            out["container_tail_events"] = self.container_tail_events()[cont]
        return out

    def assign(self, min_score: int = 0, min_share_pct: int = 50, device_out: bool = False):
        """One function per protein of an -a result, on the GPU (include/kmerguts_hip.h kg_result_assign states the rule):
        a numpy array of _native.ASSIGNMENT_DTYPE, or with device_out=True a CUDA uint8 tensor of 40 bytes per protein.  The
        device time of the assignment kernels is left in `assign_ms`."""
        lib = self._need()
        n = self.stats["n_seqs"]
        p = N.KgAssignParams(int(min_score), int(min_share_pct))
        ms = C.c_float()
        if device_out:
            import torch
            out = torch.empty(n * N.ASSIGNMENT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()            # the library works on its own stream
            N.check(lib.kg_result_assign(self._h, C.byref(p), C.c_void_p(out.data_ptr() if n else None), C.byref(ms)))
        else:
            out = np.zeros(n, dtype=N.ASSIGNMENT_DTYPE)
            N.check(lib.kg_result_assign(self._h, C.byref(p), _ptr(out), C.byref(ms)))
        self.assign_ms = float(ms.value)
        return out

    def otu_votes(self, offsets, min_votes: int = 10, min_share_pct: int = 50, min_calls: int = 1, device_out: bool = False):
        """Every OTU vote of the result tallied per sequence, one OTU per sequence and the batch's bins, on the GPU
        (include/kmerguts_hip.h kg_result_otu_votes states the rule).  offsets: the int64[n_seqs + 1] the scan was given.
        -> (votes, vote_start, classes, bins): votes _native.VOTE_DTYPE, sequence s owning votes[vote_start[s] :
        vote_start[s + 1]] (most votes first); classes _native.OTU_CLASS_DTYPE[n_seqs]; bins _native.OTU_BIN_DTYPE (longest
        first).  With device_out=True the three record arrays are CUDA uint8 tensors.  The call's counts and device time are
        left in `vote_stats`."""
        lib = self._need()
        off = _offsets(offsets, "the int64[n_seqs + 1] the scan was given", self.stats["n_seqs"])
        p = N.KgVoteParams(int(min_votes), int(min_share_pct), int(min_calls), 0)
        h = C.c_void_p()
        N.check(lib.kg_result_otu_votes(self._h, C.byref(p), off.ctypes.data, C.byref(h)))
        votes, start, classes, bins, self.vote_stats = _take_voteset(h, self.stats["n_seqs"], device_out)
        return votes, start, classes, bins

    def close(self) -> None:
        if self._h:
            N.load().kg_result_free(self._h)
            self._h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def aggregate_hits(hits: np.ndarray, container_hit_start, n_seqs: int, params: Optional[Params] = None,
                   otu_init: Optional[np.ndarray] = None, device: int = 0) -> ScanResult:
    """gatherHits / processSetOfHits / the OTU buffer (KGJ:385-524) on the GPU over caller-held hit records (HIT_DTYPE,
    ordered by container and from0InProt).  otu_init: OTU_DTYPE[n_seqs], the oICounts buffers to start from."""
    params = params or Params()
    p = params.to_native()
    h = np.ascontiguousarray(hits, dtype=N.HIT_DTYPE)
    chs = np.ascontiguousarray(np.asarray(container_hit_start, dtype=np.int64))
    if chs.size != n_seqs * (1 if params.aa else 6) + 1:
        raise ValueError("container_hit_start must have n_seqs * (1 or 6) + 1 entries")
    init = None if otu_init is None else np.ascontiguousarray(otu_init, dtype=N.OTU_DTYPE)
    out = C.c_void_p()
    N.check(N.load().kg_aggregate_hits(device, C.byref(p), _ptr(h), chs.ctypes.data, n_seqs,
                                       _ptr(init), C.byref(out)))
    return ScanResult(out.value)


class SignatureTable:
    """kmer.table.mem_map resident on one GPU (KGJ:749-753, 924-942)."""

    def __init__(self, handle: int, keepalive=None, device: Optional[int] = None):
        self._h = C.c_void_p(handle)
        self._keep = keepalive
        self.device = device                   # None: not recorded (a handle adopted without it), torch's current device is used
        self._results = weakref.WeakSet()      # results still open: closed with the table, before it

    @classmethod
    def open(cls, path: str, device: int = 0) -> "SignatureTable":
        out = C.c_void_p()
        N.check(N.load().kg_table_open(path.encode(), device, C.byref(out)))
        return cls(out.value, device=device)

    @classmethod
    def from_bytes(cls, image, device: int = 0) -> "SignatureTable":
        """image: bytes-like / uint8 ndarray holding the whole (uncompressed) file."""
        arr = np.frombuffer(image, dtype=np.uint8) if not isinstance(image, np.ndarray) else image
        arr = np.ascontiguousarray(arr.view(np.uint8).reshape(-1))
        out = C.c_void_p()
        N.check(N.load().kg_table_from_memory(arr.ctypes.data, arr.nbytes, device, C.byref(out)))
        return cls(out.value, device=device)

    @classmethod
    def from_device_ptr(cls, ptr: int, num_sigs: int, device: int = 0, keepalive=None) -> "SignatureTable":
        """Adopt num_sigs 24-byte records already in HBM (e.g. a torch tensor's data_ptr())."""
        out = C.c_void_p()
        N.check(N.load().kg_table_from_device(C.c_void_p(ptr), num_sigs, device, C.byref(out)))
        return cls(out.value, keepalive, device=device)

    @classmethod
    def build(cls, signatures, num_sigs: int, device: int = 0) -> "SignatureTable":
        """Place a signature list into a table of num_sigs slots the way the reference's lookup finds them (no-wrap linear
        probing in (kmer % num_sigs, kmer) order; include/kmerguts_hip.h kg_table_build).  signatures: a numpy array of
        _native.SIGNATURE_DTYPE or raw bytes of 24-byte records (kg_table_build), or a contiguous CUDA tensor of 24 * n
        bytes (kg_table_build_device).  The number placed is `placed` on the result (= info()["occupied"])."""
        out, placed = C.c_void_p(), C.c_int64()
        lib = N.load()
        dev = device
        on_device, ptr, n, _keep = _signature_arg(signatures)
        if on_device:
            dev = signatures.device.index if signatures.device.index is not None else device
            N.check(lib.kg_table_build_device(ptr, n, int(num_sigs), dev, C.byref(placed), C.byref(out)))
        else:
            N.check(lib.kg_table_build(ptr, n, int(num_sigs), device, C.byref(placed), C.byref(out)))
        tab = cls(out.value, device=dev)
        tab.placed = int(placed.value)
        return tab

    def merge_signatures(self, sigs, fn_map=None, otu_map=None, on_conflict: str = "keep") -> "SignatureSet":
        """This table's findable records united with new signatures, one record per k-mer, in ascending k-mer order
        (include/kmerguts_hip.h kg_table_merge_signatures states the rule).  sigs: a numpy array of _native.SIGNATURE_DTYPE or
        raw bytes of 24-byte records, or a contiguous CUDA tensor of 24 * n bytes, as for build; None is no signature.
        fn_map / otu_map: int32 arrays that rename the new signatures' function_index / otu_index, None keeps the field.
        on_conflict (a k-mer in both): "keep" the table's record, "replace" it by the new one, "drop" both unless they name the
        same function.  The table is not modified; SignatureTable.build takes the result's device_tensor()."""
        if not self._h:
            raise ValueError("SignatureTable is closed")
        if on_conflict not in N.MERGE_POLICIES:
            raise ValueError("on_conflict must be one of keep, replace, drop")
        p = N.KgMergeParams(N.MERGE_POLICIES[on_conflict], 0)
        maps = []
        for m in (fn_map, otu_map):
            if m is None:
                maps += [None, 0]
                continue
            a = np.asarray(m)
            if a.ndim != 1 or (a.size and (a.dtype.kind not in "iu" or a.min() < -2 ** 31 or a.max() >= 2 ** 31)):
                raise ValueError("a map must be a one-dimensional array of integers that fit in 32 bits")
            a = np.ascontiguousarray(a.astype(np.int32))
            maps += [a, a.size]
        fm, n_fn, om, n_otu = maps
        none = np.zeros(1, dtype=np.int32)     # (an empty map is still a map: every index is outside it)
        fp = None if fm is None else (fm.ctypes.data if fm.size else none.ctypes.data)
        op = None if om is None else (om.ctypes.data if om.size else none.ctypes.data)
        out = C.c_void_p()
        lib = N.load()
        on_device, ptr, n, _keep = _signature_arg(np.zeros(0, dtype=N.SIGNATURE_DTYPE) if sigs is None else sigs)
        merge = lib.kg_table_merge_signatures_device if on_device else lib.kg_table_merge_signatures
        N.check(merge(self._h, C.byref(p), ptr, n, fp, n_fn, op, n_otu, C.byref(out)))
        return SignatureSet(out.value, self.device)

    def signatures(self) -> "SignatureSet":
        """The table's findable records (0 <= kmer < 20^8) in ascending k-mer order: merge_signatures with no new signature."""
        return self.merge_signatures(None)

    def save(self, path: str) -> None:
        """Write kmer.table.mem_map (gzip when path ends in .gz): the header and every whole record that is resident."""
        if not self._h:
            raise ValueError("SignatureTable is closed")
        N.check(N.load().kg_table_save(self._h, os.fspath(path).encode()))

    def device_entries(self):
        """Zero-copy torch view (uint8, 24 bytes per record) of the resident records, valid until close()."""
        if not self._h:
            raise ValueError("SignatureTable is closed")
        lib = N.load()
        return device_tensor(lib.kg_table_device_entries(self._h) or 0, int(lib.kg_table_records(self._h)) * 24, "|u1", owner=self)

    def info(self) -> dict:
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        N.check(N.load().kg_table_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"numSigs": a.value, "entrySize": b.value, "version": c.value, "occupied": d.value}

    def live_device_bytes(self) -> int:
        """Device bytes of scratch / result blocks handed out by the table's block cache and not yet returned."""
        return int(N.load().kg_table_live_device_bytes(self._h))

    def scan(self, seq, offsets, params: Optional[Params] = None, device_ptr: Optional[int] = None) -> ScanResult:
        """seq: bytes / uint8 ndarray with the concatenated raw sequence characters, or None when
        device_ptr gives their address in HBM.  offsets: int64[n_seqs + 1]."""
        if not self._h:
            raise ValueError("SignatureTable is closed")
        params = params or Params()
        p = params.to_native()
        off = _offsets(offsets, "int64[n_seqs + 1]")
        n = off.size - 1
        out = C.c_void_p()
        lib = N.load()
        if device_ptr is not None:
            N.check(lib.kg_scan_device(self._h, C.byref(p), C.c_void_p(device_ptr), off.ctypes.data, n, C.byref(out)))
        else:
            arr = _seq_bytes(seq, off, no_sequence_too=True)
            N.check(lib.kg_scan(self._h, C.byref(p), _ptr(arr), off.ctypes.data, n, C.byref(out)))
        r = ScanResult(out.value, self)
        self._results.add(r)
        return r

    def close(self) -> None:
        if self._h:
            for r in list(self._results):
                r.close()
            N.load().kg_table_close(self._h)
            self._h = C.c_void_p(None)
            self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SignatureSet:
    """The signatures kg_signatures_derive* made from annotated proteins, resident on the GPU, in ascending k-mer order."""

    def __init__(self, handle: int, device: int):
        self._h = C.c_void_p(handle)
        self.device = device

    def _need(self):
        if not self._h:
            raise ValueError("SignatureSet is closed")

    @property
    def count(self) -> int:
        self._need()
        return int(N.load().kg_sigset_count(self._h))

    def numpy(self) -> np.ndarray:
        """The records as a numpy array of _native.SIGNATURE_DTYPE."""
        self._need()
        return _copy_records(N.load().kg_sigset_copy, self._h, self.count, N.SIGNATURE_DTYPE)

    def device_tensor(self):
        """Zero-copy torch view (uint8, 24 bytes per record) of the records, valid until close(); SignatureTable.build
        takes it as it is (kg_table_build_device)."""
        self._need()
        return device_tensor(N.load().kg_sigset_device(self._h) or 0, self.count * 24, "|u1", owner=self, device=self.device)

    def stats(self) -> dict:
        self._need()
        st = N.KgDeriveStats()
        N.check(N.load().kg_sigset_stats(self._h, C.byref(st)))
        return st.as_dict()

    def merge_stats(self) -> dict:
        """struct kg_merge_stats of a set made by SignatureTable.merge_signatures / signatures (an error for a derived set)."""
        self._need()
        st = N.KgMergeStats()
        N.check(N.load().kg_sigset_merge_stats(self._h, C.byref(st)))
        return st.as_dict()

    def close(self) -> None:
        if self._h:
            N.load().kg_sigset_free(self._h)
            self._h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def derive_signatures(seq, offsets, fn, otu, min_proteins: int = 2, purity_pct: int = 80, max_windows_per_pass: int = 0,
                      device: int = 0, device_ptr: Optional[int] = None) -> SignatureSet:
    """Annotated proteins -> their signature k-mers, on the GPU (include/kmerguts_hip.h kg_signatures_derive states the
    semantics).  seq: bytes / uint8 ndarray of the concatenated protein characters, or None when device_ptr gives their
    address in HBM; offsets: int64[n_prot + 1]; fn / otu: int32[n_prot] (fn = -1: unannotated).  The defaults
    min_proteins = 2 and purity_pct = 80 are this project's choice (the reference only reads signatures);
    max_windows_per_pass = 0 sizes the passes from free device memory."""
    off = _offsets(offsets, "int64[n_prot + 1]")
    n = off.size - 1
    f = np.ascontiguousarray(np.asarray(fn, dtype=np.int64))
    o = np.ascontiguousarray(np.asarray(otu, dtype=np.int64))
    if f.shape != (n,) or o.shape != (n,):
        raise ValueError("fn and otu must hold one entry per protein")
    if n and (f.min() < -2 ** 31 or f.max() >= 2 ** 31 or o.min() < -2 ** 31 or o.max() >= 2 ** 31):
        raise ValueError("fn and otu must fit in 32 bits")
    f32, o32 = f.astype(np.int32), o.astype(np.int32)
    p = N.KgDeriveParams(int(min_proteins), int(purity_pct), int(max_windows_per_pass))
    out = C.c_void_p()
    lib = N.load()
    fp, op = _ptr(f32), _ptr(o32)
    if device_ptr is not None:
        N.check(lib.kg_signatures_derive_device(device, C.byref(p), C.c_void_p(device_ptr), off.ctypes.data, n, fp, op, C.byref(out)))
    else:
        arr = _seq_bytes(seq, off)
        N.check(lib.kg_signatures_derive(device, C.byref(p), _ptr(arr), off.ctypes.data, n, fp, op, C.byref(out)))
    return SignatureSet(out.value, device)


def _align_params(min_ratio_pct: int = 50, ref="longer", gap_open: int = 11, gap_extend: int = 1,
                  max_cells: int = N.ALIGN_DEFAULT_MAX_CELLS, matrix=None):
    """-> (KgAlignParams, the matrix array it points into: keep it alive for the call)."""
    if isinstance(ref, str):
        if ref not in N.ALIGN_REFS:
            raise ValueError("ref must be 'longer' or 'member'")
        ref = N.ALIGN_REFS[ref]
    mat = None
    if matrix is not None:
        mat = np.ascontiguousarray(np.asarray(matrix, dtype=np.int64))
        if mat.shape != (21, 21) or mat.min() < -128 or mat.max() > 127:
            raise ValueError("matrix must be 21 x 21 and fit int8")
        mat = np.ascontiguousarray(mat.astype(np.int8))
    return N.KgAlignParams(int(min_ratio_pct), int(ref), int(gap_open), int(gap_extend), int(max_cells),
                           _ptr(mat), 0), mat


def _copy_ops(count_of, starts_copy, ops_copy, h, n: int):
    """(op_start int64[n + 1], ops uint32[op_start[-1]]) of a set made with ops."""
    starts = np.zeros(n + 1, dtype=np.int64)
    N.check(starts_copy(h, 0, n, starts.ctypes.data))
    ops = np.zeros(int(count_of(h)), dtype=np.uint32)
    N.check(ops_copy(h, 0, ops.size, _ptr(ops)))
    return starts, ops


def cigar(ops) -> str:
    """The CIGAR string of one record's ops (len << 4 | code, BAM's codes): "12M3D40M", or "12=1X..." from the eqx mode; "*" for
    none."""
    return "".join("%d%s" % (int(x) >> 4, N.OP_LETTERS[int(x) & 15]) for x in ops) or "*"


def alignment_text(query, target, hit, path, ops, width: int = 60, query_id: str = "query", target_id: str = "target") -> str:
    """The alignment of one traced record as text, made on the host from its ops and the two sequences.  hit: a record with a
    score; path: its _native.ALIGN_PATH_DTYPE record; ops in either mode: with
    M ops the residues are compared here.  A header line ">query_id target_id score=.. identity=..% columns=..", then rows of
    `width` columns: "Query  <first residue>  <residues / ->  <last residue>", a midline (the letter when identical, "+" when
    S > 0 under align_scores.BLOSUM62, else a space) and "Target ..." likewise; positions are 1-based."""
    from .align_scores import ALPHA, BLOSUM62

    def code_of(x: int) -> int:
        k = ALPHA.find(bytes([x]))
        return k if k >= 0 else 20

    q, t = bytes(query), bytes(target)
    i, j = int(path["start_a"]), int(path["start_b"])
    top, mid, bot = [], [], []
    for x in ops:
        ln, code = int(x) >> 4, int(x) & 15
        for _ in range(ln):
            if code == N.OP_I:
                top.append(chr(q[i])); mid.append(" "); bot.append("-"); i += 1
            elif code == N.OP_D:
                top.append("-"); mid.append(" "); bot.append(chr(t[j])); j += 1
            else:
                ca, cb = code_of(q[i]), code_of(t[j])
                top.append(chr(q[i])); bot.append(chr(t[j]))
                mid.append(chr(q[i]) if ca == cb and ca < 20 else "+" if BLOSUM62[ca][cb] > 0 else " ")
                i += 1; j += 1
    columns = len(top)
    lines = [">%s %s score=%d identity=%d%% columns=%d" % (query_id, target_id, int(hit["score"]),
                                                            100 * int(path["identical"]) // max(columns, 1), columns)]
    qi, tj = int(path["start_a"]), int(path["start_b"])     # residues consumed so far
    pw = len(str(max(i, j, 1)))
    for c0 in range(0, columns, width):
        qa, ma, ta = "".join(top[c0:c0 + width]), "".join(mid[c0:c0 + width]), "".join(bot[c0:c0 + width])
        nq, nt = len(qa) - qa.count("-"), len(ta) - ta.count("-")
        # a row without a residue of one sequence shows the position of the residue before it
        lines.append("Query  %*d  %s  %d" % (pw, qi + 1 if nq else qi, qa, qi + nq))
        lines.append("       %*s  %s" % (pw, "", ma))
        lines.append("Target %*d  %s  %d" % (pw, tj + 1 if nt else tj, ta, tj + nt))
        lines.append("")
        qi += nq
        tj += nt
    return "\n".join(lines)


def align_proteins(seq, offsets, pairs, gap_open: int = 11, gap_extend: int = 1, max_cells: int = N.ALIGN_DEFAULT_MAX_CELLS, matrix=None,
                   device: int = 0, device_ptr: Optional[int] = None, paths: bool = False,
                   max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS, ops: Optional[str] = None, band: Optional[int] = None, diagonals=None):
    """Local alignment scores of protein pairs, on the GPU (include/kmerguts_hip.h kg_proteins_align states the rule): affine
    gaps, the built-in matrix is BLOSUM62 (align_scores.BLOSUM62); matrix: 21 x 21 in code order.  seq / offsets /
    device_ptr as for cluster_proteins; pairs: int32[n_pairs][2] of (a, b) protein indices, any order, repeats allowed.
    -> _native.ALIGNMENT_DTYPE[n_pairs] in pair order (status 1 and score -1: more than max_cells cells, not aligned).
    paths=True: the traceback pass runs behind the scores (kg_proteins_align_paths): -> (the same records,
    _native.ALIGN_PATH_DTYPE[n_pairs]: start, identical, positive and gap counts; status 2: a box of more than max_trace_cells
    cells, not traced).
    ops="m" | "eqx" (needs paths=True): the alignments themselves (kg_proteins_align_ops): -> (records, paths, op_start
    int64[n_pairs + 1], ops uint32[op_start[-1]]); pair k's ops are ops[op_start[k] : op_start[k + 1]], each len << 4 | code, in
    alignment order; "m" writes M, I and D, "eqx" writes = and X for M.  cigar() gives the string.
    band=W with diagonals=int32[n_pairs] (kg_proteins_align_banded): pair k is aligned, and traced, over the cells (i, j) with
    |(i - j) - diagonals[k]| <= W only; 0 <= W <= _native.BAND_MAX.  A pair is then skipped iff min(n m, min(n, m) (2 W + 1)) is
    over max_cells.  The results have the shapes above."""
    if (band is None) != (diagonals is None):
        raise ValueError("band and diagonals go together")
    if ops is not None and ops not in N.OPS_MODES:
        raise ValueError("ops must be None, 'm' or 'eqx'")
    if ops is not None and not paths:
        raise ValueError("ops needs paths=True")
    off = _offsets(offsets, "int64[n_prot + 1]")
    n = off.size - 1
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pr.size and (pr.min() < -2 ** 31 or pr.max() >= 2 ** 31):
        raise ValueError("pair indices must fit in 32 bits")
    pr = np.ascontiguousarray(pr.astype(np.int32))
    p, _keep = _align_params(gap_open=gap_open, gap_extend=gap_extend, max_cells=max_cells, matrix=matrix)
    out = np.zeros(len(pr), dtype=N.ALIGNMENT_DTYPE)
    lib = N.load()
    pp, op = _ptr(pr), _ptr(out)
    if band is not None:
        dg = np.asarray(diagonals, dtype=np.int64).reshape(-1)
        if dg.size != len(pr):
            raise ValueError("diagonals must hold one value per pair")
        if dg.size and (dg.min() < -2 ** 31 or dg.max() >= 2 ** 31):
            raise ValueError("diagonals must fit in 32 bits")
        dg = np.ascontiguousarray(dg.astype(np.int32))
        bp = N.KgBandParams(int(band), (C.c_int32 * 3)(0, 0, 0))
        pth = np.zeros(len(pr), dtype=N.ALIGN_PATH_DTYPE) if paths else None
        h = C.c_void_p()
        tail = (off.ctypes.data, n, pp, len(pr), int(max_trace_cells), N.OPS_MODES[ops] if ops is not None else 0, op,
                _ptr(pth) if paths else None, C.byref(h) if ops is not None else None, C.byref(bp), _ptr(dg))
        if device_ptr is not None:
            N.check(lib.kg_proteins_align_banded_device(device, C.byref(p), C.c_void_p(device_ptr), *tail))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_proteins_align_banded(device, C.byref(p), _ptr(arr), *tail))
        if ops is None:
            return (out, pth) if paths else out
        try:
            return (out, pth) + _copy_ops(lib.kg_opset_ops_count, lib.kg_opset_op_starts_copy, lib.kg_opset_ops_copy, h, len(pr))
        finally:
            lib.kg_opset_free(h)
    if ops is not None:
        pth = np.zeros(len(pr), dtype=N.ALIGN_PATH_DTYPE)
        h = C.c_void_p()
        if device_ptr is not None:
            N.check(lib.kg_proteins_align_ops_device(device, C.byref(p), C.c_void_p(device_ptr), off.ctypes.data, n, pp, len(pr),
                                                     int(max_trace_cells), N.OPS_MODES[ops], op, _ptr(pth), C.byref(h)))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_proteins_align_ops(device, C.byref(p), _ptr(arr), off.ctypes.data, n, pp, len(pr), int(max_trace_cells),
                                              N.OPS_MODES[ops], op, _ptr(pth), C.byref(h)))
        try:
            return (out, pth) + _copy_ops(lib.kg_opset_ops_count, lib.kg_opset_op_starts_copy, lib.kg_opset_ops_copy, h, len(pr))
        finally:
            lib.kg_opset_free(h)
    if paths:
        pth = np.zeros(len(pr), dtype=N.ALIGN_PATH_DTYPE)
        if device_ptr is not None:
            N.check(lib.kg_proteins_align_paths_device(device, C.byref(p), C.c_void_p(device_ptr), off.ctypes.data, n, pp, len(pr),
                                                       int(max_trace_cells), op, _ptr(pth)))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_proteins_align_paths(device, C.byref(p), _ptr(arr), off.ctypes.data, n, pp, len(pr), int(max_trace_cells), op,
                                                _ptr(pth)))
        return out, pth
    if device_ptr is not None:
        N.check(lib.kg_proteins_align_device(device, C.byref(p), C.c_void_p(device_ptr), off.ctypes.data, n, pp, len(pr), op))
    else:
        arr = _seq_bytes(seq, off)
        N.check(lib.kg_proteins_align(device, C.byref(p), _ptr(arr), off.ctypes.data, n, pp, len(pr), op))
    return out


def _mask_params(mask, sides_too: bool = False):
    """mask= of search_proteins / cluster_proteins: None -> None; True or a dict of window, trigger, extend (and, with sides_too,
    sides: "both" | "queries" | "targets") -> (KgMaskParams, KG_MASK_* sides)."""
    if mask is None or mask is False:
        return None
    m = {} if mask is True else dict(mask)
    sides = m.pop("sides", "both") if sides_too else "both"
    unknown = set(m) - {"window", "trigger", "extend"}
    if unknown:
        raise ValueError("mask takes window, trigger, extend%s: not %s" % (" and sides" if sides_too else "", ", ".join(sorted(unknown))))
    if sides not in N.MASK_SIDES:
        raise ValueError("mask sides must be 'both', 'queries' or 'targets'")
    return N.KgMaskParams(int(m.get("window", N.MASK_WINDOW)), int(m.get("trigger", N.MASK_TRIGGER)),
                          int(m.get("extend", N.MASK_EXTEND)), 0), N.MASK_SIDES[sides]


def mask_proteins(seq, offsets, window: int = N.MASK_WINDOW, trigger: int = N.MASK_TRIGGER, extend: int = N.MASK_EXTEND, device: int = 0,
                  device_ptr: Optional[int] = None):
    """The low-complexity segments of proteins, on the GPU (include/kmerguts_hip.h kg_proteins_mask states the rule: SEG's trigger
    window and extension, in Lg's integers).  seq / offsets / device_ptr as for cluster_proteins; the thresholds are in units of
    1/256 bit, and the defaults 12, 563 and 640 (SEG's 2.2 and 2.5 bits) are this project's choice.
    -> (flags uint8[offsets[-1] - offsets[0]], one 0/1 per residue; segments _native.MASK_SEGMENT_DTYPE in (protein, start) order,
    0-based and inclusive; seg_start int64[n_prot + 1]; the call's statistics)."""
    off = _offsets(offsets, "int64[n_prot + 1]")
    n = off.size - 1
    p = N.KgMaskParams(int(window), int(trigger), int(extend), 0)
    h = C.c_void_p()
    lib = N.load()
    if device_ptr is not None:
        N.check(lib.kg_proteins_mask_device(device, C.byref(p), C.c_void_p(device_ptr), off.ctypes.data, n, C.byref(h)))
    else:
        arr = _seq_bytes(seq, off)
        N.check(lib.kg_proteins_mask(device, C.byref(p), _ptr(arr), off.ctypes.data, n, C.byref(h)))
    try:
        st = N.KgMaskStats()
        N.check(lib.kg_maskset_stats(h, C.byref(st)))
        starts = np.zeros(n + 1, dtype=np.int64)
        N.check(lib.kg_maskset_starts_copy(h, starts.ctypes.data))
        return (_copy_records(lib.kg_maskset_flags_copy, h, int(st.residues), np.uint8),
                _copy_records(lib.kg_maskset_copy, h, int(lib.kg_maskset_count(h)), N.MASK_SEGMENT_DTYPE), starts, st.as_dict())
    finally:
        lib.kg_maskset_free(h)


def cluster_proteins(seq, offsets, min_shared: int = 5, min_cover_pct: int = 20, max_windows: int = 0, device: int = 0,
                     device_ptr: Optional[int] = None, align: Optional[dict] = None, mask=None):
    """Proteins -> families by shared 8-mers, on the GPU (include/kmerguts_hip.h kg_proteins_cluster states the rule): a link
    from every protein of a k-mer to the k-mer's longest protein, an edge where a link's shared k-mers pass min_shared and
    min_cover_pct of the member's distinct k-mers, a family per connected component.  seq: bytes / uint8 ndarray of the
    concatenated protein characters, or None when device_ptr gives their address in HBM; offsets: int64[n_prot + 1].  The
    defaults 5 and 20 are this project's choice; max_windows = 0 sizes the one pass from free device memory.
    align: None, or a dict of min_ratio_pct (50), ref ("longer" | "member"), gap_open (11), gap_extend (1), max_cells (2^26),
    matrix (None: BLOSUM62): every link that passed the two tests is aligned (kg_proteins_cluster_aligned) and stays an edge
    only if 100 * score >= min_ratio_pct * ref; the statistics then also hold "edge_records" (_native.FAMILY_EDGE_DTYPE, one per
    such link in (member, centre) order) and "align" (aligned, cut, skipped, cells, ms_align).
    mask: None, True (the defaults of mask_proteins) or a dict of window, trigger, extend: the 8-mer pass reads a copy of the
    proteins in which the low-complexity segments are no residues (kg_proteins_cluster_masked; the alignment reads the original);
    the statistics then also hold "mask" (the statistics of mask_proteins).
    -> (numpy records of _native.FAMILY_DTYPE in protein order, the call's statistics)."""
    off = _offsets(offsets, "int64[n_prot + 1]")
    n = off.size - 1
    p = N.KgClusterParams(int(min_shared), int(min_cover_pct), 0)
    h = C.c_void_p()
    lib = N.load()
    mp = _mask_params(mask)
    if mp is not None:
        ap = None
        if align is not None:
            ap, _keep = _align_params(**align)
        apr = C.byref(ap) if ap is not None else None
        if device_ptr is not None:
            N.check(lib.kg_proteins_cluster_masked_device(device, C.byref(p), apr, C.c_void_p(device_ptr), off.ctypes.data, n,
                                                          int(max_windows), C.byref(mp[0]), C.byref(h)))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_proteins_cluster_masked(device, C.byref(p), apr, _ptr(arr), off.ctypes.data, n, int(max_windows),
                                                   C.byref(mp[0]), C.byref(h)))
    elif align is not None:
        ap, _keep = _align_params(**align)
        if device_ptr is not None:
            N.check(lib.kg_proteins_cluster_aligned_device(device, C.byref(p), C.byref(ap), C.c_void_p(device_ptr), off.ctypes.data, n,
                                                           int(max_windows), C.byref(h)))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_proteins_cluster_aligned(device, C.byref(p), C.byref(ap), _ptr(arr), off.ctypes.data,
                                                    n, int(max_windows), C.byref(h)))
    elif device_ptr is not None:
        N.check(lib.kg_proteins_cluster_device(device, C.byref(p), C.c_void_p(device_ptr), off.ctypes.data, n, int(max_windows), C.byref(h)))
    else:
        arr = _seq_bytes(seq, off)
        N.check(lib.kg_proteins_cluster(device, C.byref(p), _ptr(arr), off.ctypes.data, n, int(max_windows),
                                        C.byref(h)))
    try:
        st = N.KgClusterStats()
        N.check(lib.kg_familyset_stats(h, C.byref(st)))
        stats = st.as_dict()
        if align is not None:
            ast = N.KgAlignStats()
            N.check(lib.kg_familyset_align_stats(h, C.byref(ast)))
            stats["align"] = ast.as_dict()
            stats["edge_records"] = _copy_records(lib.kg_familyset_edges_copy, h, int(lib.kg_familyset_edges_count(h)), N.FAMILY_EDGE_DTYPE)
        if mp is not None:
            mst = N.KgMaskStats()
            N.check(lib.kg_familyset_mask_stats(h, C.byref(mst)))
            stats["mask"] = mst.as_dict()
        return _copy_records(lib.kg_familyset_copy, h, int(lib.kg_familyset_count(h)), N.FAMILY_DTYPE), stats
    finally:
        lib.kg_familyset_free(h)


def _seed_params(seeds):
    """None for the exact call, else the kg_seed_params of a seed set as seeds.resolve reads it."""
    from . import seeds as SD
    got = SD.resolve(seeds)
    if got is None:
        return None
    cls, n_cls, masks = got[:3]
    return N.KgSeedParams(len(masks), n_cls, (C.c_uint8 * 20)(*cls), (C.c_uint32 * 4)(*masks), 0)


def _take_hitset(h, has_mask: bool, has_ung: bool, band, paths, ops, db: bool = False, free: bool = True):
    """Copy a kg_hitset out in search_proteins' return shape and free it (free=False: the set is lent, and stays)."""
    lib = N.load()
    try:
        st = N.KgSearchStats()
        N.check(lib.kg_hitset_stats(h, C.byref(st)))
        starts = np.zeros(int(st.queries) + 1, dtype=np.int64)
        N.check(lib.kg_hitset_starts_copy(h, starts.ctypes.data))
        more = {}
        if has_mask:
            mst = N.KgMaskStats()
            N.check(lib.kg_hitset_mask_stats(h, C.byref(mst)))
            more["mask"] = mst.as_dict()
        extra = ()
        if has_ung:
            ust = N.KgUngappedStats()
            N.check(lib.kg_hitset_ungapped_stats(h, C.byref(ust)))
            more["ungapped"] = ust.as_dict()
            extra = (_copy_records(lib.kg_hitset_ungapped_copy, h, int(lib.kg_hitset_count(h)), N.SEARCH_UNGAPPED_DTYPE),)
        if db:
            dst = N.KgSearchDbStats()
            N.check(lib.kg_hitset_db_stats(h, C.byref(dst)))
            more["db"] = dst.as_dict()
        if band is not None:
            bst = N.KgBandStats()
            N.check(lib.kg_hitset_band_stats(h, C.byref(bst)))
            more["band"] = bst.as_dict()
        if paths is not None:
            tst = N.KgTraceStats()
            N.check(lib.kg_hitset_trace_stats(h, C.byref(tst)))
            stats = dict(st.as_dict(), traced=tst.traced, untraced=tst.untraced, trace_cells=tst.cells, ms_trace=tst.ms_trace, **more)
            count = int(lib.kg_hitset_count(h))
            got = (_copy_records(lib.kg_hitset_copy, h, count, N.SEARCH_HIT_DTYPE), starts,
                   _copy_records(lib.kg_hitset_paths_copy, h, count, N.ALIGN_PATH_DTYPE), stats)
            if ops is not None:
                ms = C.c_float()
                N.check(lib.kg_hitset_ms_ops(h, C.byref(ms)))
                stats.update(ops=int(lib.kg_hitset_ops_count(h)), ms_ops=ms.value)
                got += _copy_ops(lib.kg_hitset_ops_count, lib.kg_hitset_op_starts_copy, lib.kg_hitset_ops_copy, h, count)
            return got + extra
        return (_copy_records(lib.kg_hitset_copy, h, int(lib.kg_hitset_count(h)), N.SEARCH_HIT_DTYPE), starts, dict(st.as_dict(), **more)) + extra
    finally:
        if free:
            lib.kg_hitset_free(h)


def search_proteins(seq, offsets, n_db: int, min_shared: int = 2, max_cand: int = 8, max_db_per_kmer: int = 256,
                    align: Optional[dict] = None, max_windows: int = 0, max_pairs: int = 0, device: int = 0,
                    device_ptr: Optional[int] = None, paths: Optional[str] = None, max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS,
                    seeds=None, ops: Optional[str] = None, mask=None, ungapped=None, band: Optional[int] = None):
    """Proteins [n_db, n_prot) searched against proteins [0, n_db), on the GPU (include/kmerguts_hip.h kg_proteins_search states
    the rule): the targets that share at least min_shared distinct unmasked 8-mers with a query, the max_cand with the most
    aligned, a hit where 100 * score >= min_ratio_pct * ref.  seq / offsets / device_ptr as for cluster_proteins; align: None
    (the defaults) or a dict as for cluster_proteins; max_windows = 0 and max_pairs = 0 size the one pass and the join from
    free device memory.  The defaults 2, 8 and 256 are this project's choice.
    -> (numpy records of _native.SEARCH_HIT_DTYPE in (query, rank) order, hit_start int64[n_q + 1], the call's statistics).
    paths: None, "hits" (the records with status hit are traced) or "all" (every aligned record with score >= 1):
    kg_proteins_search_paths; -> (records, hit_start, _native.ALIGN_PATH_DTYPE records of the same indices, statistics), the
    statistics with traced, untraced, trace_cells and ms_trace as well.
    seeds: None (the exact 8-mers: the calls above), "reduced" (the built-in reduced-alphabet spaced seeds) or a
    dict(alphabet="identity" | "reduced11" | "AST,C,DEKNQR,...", shapes=["1111...", ...]) as seeds.py reads it:
    kg_proteins_search_seeded, the same results with "seed id" read for "8-mer".
    ops: None, "m" or "eqx" (needs paths): the traced records' ops as in align_proteins; -> (records, hit_start, path records,
    statistics, op_start int64[count + 1], ops), the statistics with ops and ms_ops as well.
    mask: None, True (the defaults of mask_proteins) or a dict of window, trigger, extend and sides ("both", the default,
    "queries" or "targets"): the seeding pass reads a copy in which that side's low-complexity segments are no residues
    (kg_proteins_search_masked); the alignment, the trace and the ops read the original.  The statistics then also hold "mask".
    ungapped: None, True (min_score 0: rank only) or {"min_score": N}: kg_proteins_search_filtered, with seeds and mask as above.
    Every candidate's best seed diagonal is scored without gaps, candidates with a score below N are dropped and a query's
    candidates are cut by (larger ungapped score, larger s, smaller target).  The result tuple then ends with one more array,
    _native.SEARCH_UNGAPPED_DTYPE records of the hit records' indices, and the statistics hold "ungapped" (scored, dropped,
    cut, cells, ms_ungapped).
    band: None or W (needs ungapped): kg_proteins_search_banded.  Every aligned candidate is aligned, and traced, in the band of
    half-width W around its best seed diagonal (align_proteins' band).  The results keep their shapes and the statistics hold
    "band" (band_cells, full_cells, band)."""
    if band is not None and (ungapped is None or ungapped is False):
        raise ValueError("band needs ungapped")
    up = None
    if ungapped is not None and ungapped is not False:
        if ungapped is True:
            ungapped = {}
        if not isinstance(ungapped, dict) or set(ungapped) - {"min_score"}:
            raise ValueError("ungapped must be None, True or {'min_score': N}")
        up = N.KgUngappedParams(int(ungapped.get("min_score", 0)), (C.c_int32 * 3)(0, 0, 0))
    if paths is not None and paths not in N.TRACE_MODES:
        raise ValueError("paths must be None, 'hits' or 'all'")
    if ops is not None and ops not in N.OPS_MODES:
        raise ValueError("ops must be None, 'm' or 'eqx'")
    if ops is not None and paths is None:
        raise ValueError("ops needs paths")
    trace = (N.TRACE_MODES[paths] if paths is not None else 0) | (N.OPS_MODES[ops] if ops is not None else 0)
    seed_set = _seed_params(seeds)
    off = _offsets(offsets, "int64[n_prot + 1]")
    n = off.size - 1
    p = N.KgSearchParams(int(min_shared), int(max_cand), int(max_db_per_kmer), 0)
    ap, _keep = _align_params(**(align or {}))
    h = C.c_void_p()
    lib = N.load()
    mp = _mask_params(mask, sides_too=True)
    if up is not None and band is not None:
        sp = C.byref(seed_set) if seed_set is not None else None
        bp = N.KgBandParams(int(band), (C.c_int32 * 3)(0, 0, 0))
        tail = (int(max_windows), int(max_pairs), trace, int(max_trace_cells), C.byref(mp[0]) if mp is not None else None,
                mp[1] if mp is not None else 0, C.byref(up), C.byref(bp), C.byref(h))
        if device_ptr is not None:
            N.check(lib.kg_proteins_search_banded_device(device, C.byref(p), sp, C.byref(ap), C.c_void_p(device_ptr), off.ctypes.data, n,
                                                         int(n_db), *tail))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_proteins_search_banded(device, C.byref(p), sp, C.byref(ap), _ptr(arr), off.ctypes.data, n, int(n_db), *tail))
    elif up is not None:
        sp = C.byref(seed_set) if seed_set is not None else None
        tail = (int(max_windows), int(max_pairs), trace, int(max_trace_cells), C.byref(mp[0]) if mp is not None else None,
                mp[1] if mp is not None else 0, C.byref(up), C.byref(h))
        if device_ptr is not None:
            N.check(lib.kg_proteins_search_filtered_device(device, C.byref(p), sp, C.byref(ap), C.c_void_p(device_ptr), off.ctypes.data, n,
                                                           int(n_db), *tail))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_proteins_search_filtered(device, C.byref(p), sp, C.byref(ap), _ptr(arr), off.ctypes.data, n, int(n_db), *tail))
    elif mp is not None:
        sp = C.byref(seed_set) if seed_set is not None else None
        tail = (int(max_windows), int(max_pairs), trace, int(max_trace_cells), C.byref(mp[0]), mp[1], C.byref(h))
        if device_ptr is not None:
            N.check(lib.kg_proteins_search_masked_device(device, C.byref(p), sp, C.byref(ap), C.c_void_p(device_ptr), off.ctypes.data, n,
                                                         int(n_db), *tail))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_proteins_search_masked(device, C.byref(p), sp, C.byref(ap), _ptr(arr), off.ctypes.data, n, int(n_db), *tail))
    elif seed_set is not None:
        tail = (int(max_windows), int(max_pairs), trace, int(max_trace_cells), C.byref(h))
        if device_ptr is not None:
            N.check(lib.kg_proteins_search_seeded_device(device, C.byref(p), C.byref(seed_set), C.byref(ap), C.c_void_p(device_ptr),
                                                         off.ctypes.data, n, int(n_db), *tail))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_proteins_search_seeded(device, C.byref(p), C.byref(seed_set), C.byref(ap), _ptr(arr), off.ctypes.data, n,
                                                  int(n_db), *tail))
    elif paths is not None:
        tail = (int(max_windows), int(max_pairs), trace, int(max_trace_cells), C.byref(h))
        if device_ptr is not None:
            N.check(lib.kg_proteins_search_paths_device(device, C.byref(p), C.byref(ap), C.c_void_p(device_ptr), off.ctypes.data, n,
                                                        int(n_db), *tail))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_proteins_search_paths(device, C.byref(p), C.byref(ap), _ptr(arr), off.ctypes.data, n, int(n_db), *tail))
    elif device_ptr is not None:
        N.check(lib.kg_proteins_search_device(device, C.byref(p), C.byref(ap), C.c_void_p(device_ptr), off.ctypes.data, n, int(n_db),
                                              int(max_windows), int(max_pairs), C.byref(h)))
    else:
        arr = _seq_bytes(seq, off)
        N.check(lib.kg_proteins_search(device, C.byref(p), C.byref(ap), _ptr(arr), off.ctypes.data, n,
                                       int(n_db), int(max_windows), int(max_pairs), C.byref(h)))
    return _take_hitset(h, mp is not None, up is not None, band, paths, ops)


def _search_options(ungapped, band, paths, ops):
    """The checks SearchDb.search and search_contigs share -> (kg_ungapped_params or None, the trace word)."""
    if band is not None and (ungapped is None or ungapped is False):
        raise ValueError("band needs ungapped")
    up = None
    if ungapped is not None and ungapped is not False:
        if ungapped is True:
            ungapped = {}
        if not isinstance(ungapped, dict) or set(ungapped) - {"min_score"}:
            raise ValueError("ungapped must be None, True or {'min_score': N}")
        up = N.KgUngappedParams(int(ungapped.get("min_score", 0)), (C.c_int32 * 3)(0, 0, 0))
    if paths is not None and paths not in N.TRACE_MODES:
        raise ValueError("paths must be None, 'hits' or 'all'")
    if ops is not None and ops not in N.OPS_MODES:
        raise ValueError("ops must be None, 'm' or 'eqx'")
    if ops is not None and paths is None:
        raise ValueError("ops needs paths")
    trace = (N.TRACE_MODES[paths] if paths is not None else 0) | (N.OPS_MODES[ops] if ops is not None else 0)
    return up, trace


class SearchDb:
    """A resident protein database (include/kmerguts_hip.h kg_searchdb): the targets' half of search_proteins' work, made once and
    kept on the device.  build() makes it from the targets, save() writes its file and open() reads one; search() gives, for a
    batch of queries, what search_proteins gives for "the targets, then these queries" with the same options, byte for byte.
    One call at a time per handle.  Use as a context manager or call close()."""

    def __init__(self, handle, path: Optional[str] = None, device: int = 0):
        self._h = handle
        self._path = path               # open(): the file, which targets() reads
        self._device = int(device)      # search_contigs: the device the evidence's table-less stages run on

    @classmethod
    def build(cls, seq, offsets, seeds=None, mask=None, names: bytes = b"", max_windows: int = 0, query_room: int = 0, device: int = 0,
              device_ptr: Optional[int] = None) -> "SearchDb":
        """seq / offsets / device_ptr: the targets, as for search_proteins; seeds and mask (window, trigger, extend; no sides: the
        targets are the masked side) as there; names: an opaque blob handed back by names(); query_room: the residues of the
        largest query batch (0: the library's default)."""
        seed_set = _seed_params(seeds)
        mp = _mask_params(mask)
        off = _offsets(offsets, "int64[n_db + 1]")
        blob = np.frombuffer(bytes(names), dtype=np.uint8)
        h = C.c_void_p()
        lib = N.load()
        tail = (off.ctypes.data, off.size - 1, C.byref(seed_set) if seed_set is not None else None,
                C.byref(mp[0]) if mp is not None else None, _ptr(blob), blob.size, int(max_windows), int(query_room), C.byref(h))
        if device_ptr is not None:
            N.check(lib.kg_searchdb_build_device(device, C.c_void_p(device_ptr), *tail))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_searchdb_build(device, _ptr(arr), *tail))
        return cls(h, device=device)

    @classmethod
    def open(cls, path: str, query_room: int = 0, device: int = 0) -> "SearchDb":
        h = C.c_void_p()
        N.check(N.load().kg_searchdb_open(device, os.fsencode(path), int(query_room), C.byref(h)))
        return cls(h, path, device)

    def targets(self):
        """(residues uint8, offsets int64[n_db + 1]) of an opened index, read from its file's first two sections (the file has
        passed kg_searchdb_open's checks); a front end needs the targets' lengths and residues to write alignments."""
        if self._path is None:
            raise ValueError("targets() reads the file of an opened SearchDb")
        with open(self._path, "rb") as f:
            hdr = f.read(N.SEARCHDB_HEADER_BYTES)
            at = np.frombuffer(hdr, dtype="<u8", count=4, offset=216).copy()       # two section entries: offset, bytes, checksum
            f.seek(int(at[0]))
            off = np.frombuffer(f.read(int(at[1])), dtype="<i8").astype(np.int64)
            f.seek(int(at[3]))
            seq = np.frombuffer(f.read(int(off[-1])), dtype=np.uint8)
        return seq, off

    def _handle(self):
        if self._h is None:
            raise ValueError("the SearchDb is closed")
        return self._h

    def save(self, path: str) -> None:
        N.check(N.load().kg_searchdb_save(self._handle(), os.fsencode(path)))

    def info(self) -> dict:
        """targets, residues, pairs, kmers, valid_windows, names_bytes, query_room, device_bytes, seeds (None: the exact 8-mers, else
        n_shapes, alphabet_size, cls, shape), mask (None or window, trigger, extend), mask_stats, and the build's ms_* by stage."""
        d = N.KgSearchDbDesc()
        N.check(N.load().kg_searchdb_info(self._handle(), C.byref(d)))
        out = {k: getattr(d, k) for k in ("targets", "residues", "pairs", "kmers", "valid_windows", "names_bytes", "query_room",
                                          "device_bytes", "ms_upload", "ms_encode", "ms_sort", "ms_index", "ms_total")}
        out["seeds"] = (dict(n_shapes=d.seeds.n_shapes, alphabet_size=d.seeds.alphabet_size, cls=list(d.seeds.cls),
                             shape=list(d.seeds.shape)[:d.seeds.n_shapes]) if d.has_seeds else None)
        out["mask"] = dict(window=d.mask.window, trigger=d.mask.trigger, extend=d.mask.extend) if d.has_mask else None
        out["mask_stats"] = d.mask_stats.as_dict() if d.has_mask else None
        return out

    def names(self) -> bytes:
        n = self.info()["names_bytes"]
        buf = np.zeros(n, dtype=np.uint8)
        N.check(N.load().kg_searchdb_names_copy(self._handle(), _ptr(buf)))
        return buf.tobytes()

    def live_device_bytes(self) -> int:
        return int(N.load().kg_searchdb_live_device_bytes(self._handle()))

    def reserve(self, query_room: int) -> None:
        N.check(N.load().kg_searchdb_reserve(self._handle(), int(query_room)))

    def search(self, seq, offsets, min_shared: int = 2, max_cand: int = 8, max_db_per_kmer: int = 256, align: Optional[dict] = None,
               max_windows: int = 0, max_pairs: int = 0, device_ptr: Optional[int] = None, paths: Optional[str] = None,
               max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS, ops: Optional[str] = None, mask=None, ungapped=None,
               band: Optional[int] = None):
        """search_proteins' keyword arguments and return shape, with seq / offsets the queries alone; the seeds are the handle's and
        mask (window, trigger, extend) masks the queries.  The statistics also hold "db" (query_kmers, found, ms_probe, ms_upload)."""
        up, trace = _search_options(ungapped, band, paths, ops)
        off = _offsets(offsets, "int64[n_q + 1]")
        p = N.KgSearchParams(int(min_shared), int(max_cand), int(max_db_per_kmer), 0)
        ap, _keep = _align_params(**(align or {}))
        mp = _mask_params(mask)
        bp = N.KgBandParams(int(band), (C.c_int32 * 3)(0, 0, 0)) if band is not None else None
        h = C.c_void_p()
        lib = N.load()
        tail = (off.ctypes.data, off.size - 1, int(max_windows), int(max_pairs), trace, int(max_trace_cells),
                C.byref(mp[0]) if mp is not None else None, C.byref(up) if up is not None else None,
                C.byref(bp) if bp is not None else None, C.byref(h))
        if device_ptr is not None:
            N.check(lib.kg_searchdb_search_device(self._handle(), C.byref(p), C.byref(ap), C.c_void_p(device_ptr), *tail))
        else:
            arr = _seq_bytes(seq, off)
            N.check(lib.kg_searchdb_search(self._handle(), C.byref(p), C.byref(ap), _ptr(arr), *tail))
        has_mask = mp is not None or self.info()["mask"] is not None
        return _take_hitset(h, has_mask, up is not None, band, paths, ops, db=True)

    def search_contigs(self, seq, offsets, min_res: int = N.TRANSLATE_MIN_RES, max_hits: int = N.TRANSLATE_MAX_HITS, target_fn=None,
                       device_ptr: Optional[int] = None, min_shared: int = 2, max_cand: int = 8, max_db_per_kmer: int = 256,
                       align: Optional[dict] = None, max_windows: int = 0, max_pairs: int = 0, paths: Optional[str] = None,
                       max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS, ops: Optional[str] = None, mask=None, ungapped=None,
                       band: Optional[int] = None, explained_by=None, explain_min: int = 1, min_db_count: int = 0) -> "Evidence":
        """Genes by homology (include/kmerguts_hip.h kg_contigs_search_translated states the rule): every stop-to-stop run of the
        six frames of the contigs with at least min_res residues is a query of search(); a hit of rank below max_hits with a
        traced path becomes a CALL record in contig coordinates whose fI is the target, or target_fn[target] (int32[n_db]).
        seq / offsets: the contigs, as a scan takes them; device_ptr: the address of the bytes in HBM instead of seq.  The other
        keywords are search()'s; paths=None is read as "hits", since a CALL needs the path's start.  -> an Evidence.
        explained_by: the signature CALLs of the same batch, a ScanResult of a DNA scan (read where its CALLs lie on the device)
        or a _native.CALL_DTYPE array in container order (kg_contigs_search_residual states the rule; target_fn is then
        required).  Only the fragments whose touching CALLs' counts sum to less than explain_min are searched, homology CALLs of
        a count below min_db_count are left out, and the Evidence's calls are the two kinds merged by container."""
        hd = self._handle()
        if explained_by is None and (int(explain_min) != 1 or int(min_db_count) != 0):
            raise ValueError("explain_min and min_db_count need explained_by")
        if explained_by is not None:
            if target_fn is None:
                raise ValueError("explained_by needs target_fn: the two kinds of CALL share one function index space")
            if int(explain_min) < 1:
                raise ValueError("explain_min must be >= 1")
            if int(min_db_count) < 0:
                raise ValueError("min_db_count must be >= 0")
        up, trace = _search_options(ungapped, band, "hits" if paths is None else paths, ops)
        if int(min_res) < 1:
            raise ValueError("min_res must be >= 1")
        if not 1 <= int(max_hits) <= 64:
            raise ValueError("max_hits must be in 1..64")
        off = _offsets(offsets, "int64[n_seqs + 1]")
        fn = None
        if target_fn is not None:
            fn = np.ascontiguousarray(np.asarray(target_fn, dtype=np.int32))
            if fn.shape != (self.info()["targets"],):
                raise ValueError("target_fn must hold one function per target")
            if fn.size and int(fn.min()) < 0:
                raise ValueError("target_fn must be >= 0")
        p = N.KgSearchParams(int(min_shared), int(max_cand), int(max_db_per_kmer), 0)
        ap, _keep = _align_params(**(align or {}))
        tp = N.KgTranslateParams(int(min_res), int(max_hits), (C.c_int32 * 2)(0, 0))
        mp = _mask_params(mask)
        bp = N.KgBandParams(int(band), (C.c_int32 * 3)(0, 0, 0)) if band is not None else None
        keep = None if device_ptr is not None else _seq_bytes(seq, off)
        h = C.c_void_p()
        lib = N.load()
        args = (hd, C.byref(p), C.byref(ap), C.byref(tp), C.c_void_p(device_ptr) if keep is None else _ptr(keep), int(keep is None),
                off.ctypes.data, off.size - 1, int(max_windows), int(max_pairs), trace, int(max_trace_cells),
                C.byref(mp[0]) if mp is not None else None, C.byref(up) if up is not None else None, C.byref(bp) if bp is not None else None,
                _ptr(fn))
        if explained_by is None:
            N.check(lib.kg_contigs_search_translated(*args, C.byref(h)))
        else:
            rp = N.KgResidualParams(int(explain_min), int(min_db_count), 0)
            if isinstance(explained_by, ScanResult):
                explained_by._need()
                N.check(lib.kg_result_search_residual(explained_by._h, *args, C.byref(rp), C.byref(h)))
            else:
                sig = np.ascontiguousarray(explained_by)
                if sig.dtype != N.CALL_DTYPE or sig.ndim != 1:
                    raise ValueError("explained_by must be a ScanResult or a _native.CALL_DTYPE array")
                N.check(lib.kg_contigs_search_residual(*args, _ptr(sig), 0, sig.size, C.byref(rp), C.byref(h)))
        has_mask = mp is not None or self.info()["mask"] is not None
        return Evidence(h, off.size - 1, self._device, has_mask, up is not None, band, "hits" if paths is None else paths, ops,
                        residual=explained_by is not None)

    def close(self) -> None:
        if self._h is not None:
            N.load().kg_searchdb_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Evidence(_GeneSteps):
    """Owns one kg_evidence, what SearchDb.search_contigs returns: `calls` (_native.CALL_DTYPE, in the hit records' order),
    `call_hits` (int64: the hit record of every CALL), `fragments` ((records _native.ORF_DTYPE, prot_start, residues), what
    free_orfs(start_codons=0) gives), `search` (what SearchDb.search returns for the fragments' proteins) and `stats`
    (fragments, fragment_residues, records, calls, dropped_status, dropped_rank, dropped_untraced, ms_*).
    regions(), orfs() and select() are ScanResult's, arguments, results and side attributes, on these CALLs; the repair step is
    kg_regionset_repair with the evidence's device CALLs.  Use as a context manager or call close(); the evidence may outlive
    its SearchDb.
    With explained_by (kg_contigs_search_residual) `calls` is the merged list, `call_hits` holds -1 for a signature CALL,
    `fragments` are all fragments and `search` is the search of the searched ones; there are also `explain` (int64 per
    fragment), `searched` (int64: every query's index among the fragments), `searched_fragments` (records, prot_start, residues),
    `call_kind` (uint8: 0 signature, 1 homology), `call_source` (int64: the CALL's index in its own list) and `residual_stats`
    (sig_calls, explained, explained_residues, searched, searched_residues, db_calls, dropped_min_count, merged, ms_*).
    Without it none of these attributes exists."""

    def __init__(self, handle, n_seqs: int, device: int, has_mask: bool, has_ung: bool, band, paths, ops, residual: bool = False):
        self._h = handle
        self._seqs, self._dev = int(n_seqs), int(device)
        lib = N.load()
        try:
            st = N.KgTranslateStats()
            N.check(lib.kg_evidence_stats(self._h, C.byref(st)))
            self.stats = st.as_dict()
            n = int(lib.kg_evidence_calls_count(self._h))
            self.calls = _copy_records(lib.kg_evidence_calls_copy, self._h, n, N.CALL_DTYPE)
            self.call_hits = _copy_records(lib.kg_evidence_call_hits_copy, self._h, n, np.int64)
            frags = _take_orfset(C.c_void_p(lib.kg_evidence_fragments(self._h)), False, free=False)
            self.fragments, self.fragment_stats = frags[:3], frags[3]
            self.search = _take_hitset(C.c_void_p(lib.kg_evidence_hits(self._h)), has_mask, has_ung, band, paths, ops, db=True, free=False)
            if residual:
                rst = N.KgResidualStats()
                N.check(lib.kg_residual_stats_of(self._h, C.byref(rst)))
                self.residual_stats = rst.as_dict()
                self.explain = _copy_records(lib.kg_residual_explain_copy, self._h, len(self.fragments[0]), np.int64)
                self.searched = _copy_records(lib.kg_residual_searched_copy, self._h, int(rst.searched), np.int64)
                self.searched_fragments = _take_orfset(C.c_void_p(lib.kg_residual_searched_fragments(self._h)), False, free=False)[:3]
                self.call_kind = _copy_records(lib.kg_residual_call_kinds_copy, self._h, n, np.uint8)
                self.call_source = _copy_records(lib.kg_residual_call_sources_copy, self._h, n, np.int64)
        except BaseException:
            self.close()
            raise

    def _need(self):
        if not self._h:
            raise ValueError("the Evidence is closed")
        return N.load()

    def _n_seqs(self) -> int:
        return self._seqs

    def _regions_call(self, lib, p, off, h):
        return lib.kg_regions_calls(self._dev, C.byref(p), _ptr(self.calls), self.calls.size, off.ctypes.data, off.size - 1, C.byref(h))

    def _repair_call(self, lib, rh, oh, rp, batch, new):
        return lib.kg_regionset_repair(rh, oh, C.c_void_p(lib.kg_evidence_calls_device(self._h)), 1, self.calls.size, C.byref(rp), *batch, new)

    def close(self) -> None:
        if self._h:
            N.load().kg_evidence_free(self._h)
            self._h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def assign_calls(calls, call_start, otu=None, min_score: int = 0, min_share_pct: int = 50, device: int = 0) -> np.ndarray:
    """One function per protein from caller-held CALL lists, on the GPU (kg_assign_calls): calls CALL_DTYPE[call_start[-1]],
    call_start int64[n_prot + 1] (protein p's CALLs are calls[call_start[p] : call_start[p + 1]], in emission order), otu
    OTU_DTYPE[n_prot] or None.  -> ASSIGNMENT_DTYPE[n_prot]."""
    cs = np.ascontiguousarray(np.asarray(call_start, dtype=np.int64))
    if cs.ndim != 1 or cs.size < 1:
        raise ValueError("call_start must be int64[n_prot + 1]")
    n = cs.size - 1
    c = np.ascontiguousarray(calls, dtype=N.CALL_DTYPE)
    if n and cs[-1] > c.size:
        raise ValueError("call_start[-1] is beyond the CALL records")
    o = None if otu is None else np.ascontiguousarray(otu, dtype=N.OTU_DTYPE)
    if o is not None and o.shape != (n,):
        raise ValueError("otu must hold one record per protein")
    out = np.zeros(n, dtype=N.ASSIGNMENT_DTYPE)
    p = N.KgAssignParams(int(min_score), int(min_share_pct))
    N.check(N.load().kg_assign_calls(device, C.byref(p), _ptr(c), cs.ctypes.data, n,
                                     _ptr(o), _ptr(out)))
    return out


def _take_regionset(h, n_seqs: int, device_out: bool):
    """Copy a kg_regionset out (records to the host or into a CUDA tensor, region_start to the host) and free it.
    -> (records, region_start, statistics)."""
    lib = N.load()
    try:
        st = N.KgRegionStats()
        N.check(lib.kg_regionset_stats(h, C.byref(st)))
        n = int(lib.kg_regionset_count(h))
        start = np.zeros(n_seqs + 1, dtype=np.int64)
        N.check(lib.kg_regionset_seq_start(h, start.ctypes.data))
        return _copy_records(lib.kg_regionset_copy, h, n, N.REGION_DTYPE, device_out=device_out), start, st.as_dict()
    finally:
        lib.kg_regionset_free(h)


def region_calls(calls, offsets, merge_gap: int = 600, min_score: int = 0, min_len: int = 0, device: int = 0,
                 device_out: bool = False, stats: Optional[dict] = None):
    """Function regions from caller-held CALL records of a DNA scan, on the GPU (kg_regions_calls): calls CALL_DTYPE in
    non-decreasing container order, offsets int64[n_seqs + 1].  -> (records, region_start) as ScanResult.regions; `stats`, when
    given, receives the call's counts and device time."""
    off = _offsets(offsets, "int64[n_seqs + 1]")
    c = np.ascontiguousarray(calls, dtype=N.CALL_DTYPE)
    p = N.KgRegionParams(int(merge_gap), int(min_score), int(min_len))
    h = C.c_void_p()
    N.check(N.load().kg_regions_calls(device, C.byref(p), _ptr(c), c.size, off.ctypes.data,
                                      off.size - 1, C.byref(h)))
    out, start, st = _take_regionset(h, off.size - 1, device_out)
    if stats is not None:
        stats.update(st)
    return out, start


def _take_voteset(h, n_seqs: int, device_out: bool):
    """Copy a kg_voteset out (the three record arrays to the host or into CUDA tensors, vote_start to the host) and free it.
    -> (votes, vote_start, classes, bins, statistics)."""
    lib = N.load()
    try:
        st = N.KgVoteStats()
        N.check(lib.kg_voteset_stats(h, C.byref(st)))
        start = np.zeros(n_seqs + 1, dtype=np.int64)
        N.check(lib.kg_voteset_seq_start(h, start.ctypes.data))
        votes = _copy_records(lib.kg_voteset_copy_votes, h, int(lib.kg_voteset_count(h)), N.VOTE_DTYPE, device_out=device_out)
        classes = _copy_records(lib.kg_voteset_copy_classes, h, n_seqs, N.OTU_CLASS_DTYPE, device_out=device_out)
        bins = _copy_records(lib.kg_voteset_copy_bins, h, int(lib.kg_voteset_bins(h)), N.OTU_BIN_DTYPE, device_out=device_out)
        return votes, start, classes, bins, st.as_dict()
    finally:
        lib.kg_voteset_free(h)


def otu_votes(hits, container_hit_start, hit_events, calls, container_call_start, n_seqs: int, per: int, offsets,
              min_votes: int = 10, min_share_pct: int = 50, min_calls: int = 1, device: int = 0, device_out: bool = False,
              stats: Optional[dict] = None):
    """The OTU votes of caller-held records, on the GPU (kg_otu_votes_hits): hits HIT_DTYPE in (container, from0InProt) order
    with container_hit_start int64[n_seqs * per + 1], hit_events one KG_EV_* byte per hit, calls CALL_DTYPE with
    container_call_start, per 6 (DNA) or 1 (-a), offsets int64[n_seqs + 1].  -> (votes, vote_start, classes, bins) as
    ScanResult.otu_votes; `stats`, when given, receives the call's counts and device time."""
    chs = np.ascontiguousarray(np.asarray(container_hit_start, dtype=np.int64))
    ccs = np.ascontiguousarray(np.asarray(container_call_start, dtype=np.int64))
    n_seqs, per = int(n_seqs), int(per)
    off = _offsets(offsets, "int64[n_seqs + 1]", n_seqs)
    n_cont = n_seqs * per if per > 0 else 0
    if chs.shape != (n_cont + 1,) or ccs.shape != (n_cont + 1,):
        raise ValueError("container_hit_start and container_call_start must be int64[n_seqs * per + 1]")
    hh = np.ascontiguousarray(hits, dtype=N.HIT_DTYPE)
    ev = np.ascontiguousarray(hit_events, dtype=np.uint8)
    c = np.ascontiguousarray(calls, dtype=N.CALL_DTYPE)
    if ev.shape != hh.shape or (chs.size and chs[-1] > hh.size) or (ccs.size and ccs[-1] > c.size):
        raise ValueError("the start arrays reach beyond the records, or hit_events is not one byte per hit")
    p = N.KgVoteParams(int(min_votes), int(min_share_pct), int(min_calls), 0)
    h = C.c_void_p()
    N.check(N.load().kg_otu_votes_hits(device, C.byref(p), _ptr(hh), chs.ctypes.data,
                                       _ptr(ev), _ptr(c), ccs.ctypes.data,
                                       n_seqs, per, off.ctypes.data, C.byref(h)))
    votes, start, classes, bins, st = _take_voteset(h, n_seqs, device_out)
    if stats is not None:
        stats.update(st)
    return votes, start, classes, bins


def compose_contigs(seq, offsets, labels=None, model=None, min_len: int = 1500, min_margin: int = 2560, min_train: int = 200000,
                    keep_scores: bool = False, device: int = 0, device_out: bool = False, stats: Optional[dict] = None) -> dict:
    """Bin contigs by tetranucleotide composition, on the GPU and without a table (kg_contigs_compose; include/kmerguts_hip.h
    states the rule).  seq the batch's bytes, offsets int64[n_seqs + 1], labels int32[n_seqs] (>= 0 the bin of a training contig,
    -1 unlabelled; None = all -1), model None or (labels int32[M], counts int64[M + 1][256], the background row last).
    -> {"classes": COMP_CLASS_DTYPE[n_seqs], "counts": int32[n_seqs][256], "row_labels": int32[R], "rows": int64[R][256],
    "background": int64[256], "model_labels": int32[M]} and with keep_scores "scores": int64[n_seqs][M + 1]; classes, counts and
    scores are CUDA tensors with device_out=True (classes as uint8 of 40 bytes per contig).  `stats`, when given, receives the
    call's counts and device times."""
    off = _offsets(offsets, "int64[n_seqs + 1]")
    n = off.size - 1
    arr = _seq_bytes(seq, off)
    lab = None
    if labels is not None:
        lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32))
        if lab.shape != (n,):
            raise ValueError("labels must be int32[n_seqs]")
    ml = mc = None
    n_models = 0
    if model is not None:
        ml = np.ascontiguousarray(np.asarray(model[0], dtype=np.int32).reshape(-1))
        mc = np.ascontiguousarray(np.asarray(model[1], dtype=np.int64))
        n_models = ml.size
        if mc.size != (n_models + 1) * N.COMP_BINS:
            raise ValueError("model counts are int64[n_models + 1][%d], the background row last" % N.COMP_BINS)
    p = N.KgCompParams(int(min_len), int(min_margin), int(min_train), 1 if keep_scores else 0, 0)
    lib = N.load()
    h = C.c_void_p()
    N.check(lib.kg_contigs_compose(device, C.byref(p), _ptr(arr), 0, off.ctypes.data, n,
                                   _ptr(lab), _ptr(ml),
                                   _ptr(mc), n_models, C.byref(h)))
    try:
        st = N.KgCompStats()
        N.check(lib.kg_compset_stats(h, C.byref(st)))
        R, M = int(lib.kg_compset_rows(h)), int(lib.kg_compset_models(h))
        out = {"row_labels": np.zeros(R, dtype=np.int32), "rows": np.zeros((R, N.COMP_BINS), dtype=np.int64),
               "background": np.zeros(N.COMP_BINS, dtype=np.int64),
               "model_labels": _copy_records(lib.kg_compset_model_labels, h, M, np.int32)}
        N.check(lib.kg_compset_copy_rows(h, 0, R, _ptr(out["row_labels"]), _ptr(out["rows"])))
        N.check(lib.kg_compset_background(h, out["background"].ctypes.data))
        out["classes"] = _copy_records(lib.kg_compset_copy_classes, h, n, N.COMP_CLASS_DTYPE, device_out=device_out)
        out["counts"] = _copy_records(lib.kg_compset_copy_counts, h, n, np.int32, (N.COMP_BINS,), device_out)
        if keep_scores:
            out["scores"] = _copy_records(lib.kg_compset_copy_scores, h, n, np.int64, (M + 1,), device_out)
        if stats is not None:
            stats.update(st.as_dict())
        return out
    finally:
        lib.kg_compset_free(h)


def _take_orfset(h, device_out: bool, free: bool = True):
    """Copy a kg_orfset out (to the host, or into CUDA tensors) and free it (free=False: the set is lent, and stays).
    -> (records, prot_start, residues, statistics)."""
    lib = N.load()
    try:
        st = N.KgOrfStats()
        N.check(lib.kg_orfset_stats(h, C.byref(st)))
        n, n_res = int(lib.kg_orfset_count(h)), int(st.residues)
        out = _copy_records(lib.kg_orfset_copy, h, n, N.ORF_DTYPE, device_out=device_out)
        res = _copy_records(lib.kg_orfset_residues, h, n_res, np.uint8, device_out=device_out)
        if device_out:
            import torch
            start = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            N.check(lib.kg_orfset_prot_start(h, C.c_void_p(start.data_ptr())))
        else:
            start = np.zeros(n + 1, dtype=np.int64)
            N.check(lib.kg_orfset_prot_start(h, start.ctypes.data))
        return out, start, res, st.as_dict()
    finally:
        if free:
            lib.kg_orfset_free(h)


def _junctions(h):
    """The junction list of a set made by kg_regionset_repair -> (records, junction_start, statistics); the set stays."""
    lib = N.load()
    st = N.KgRepairStats()
    N.check(lib.kg_orfset_junctions_stats(h, C.byref(st)))
    n, nj = int(lib.kg_orfset_count(h)), int(lib.kg_orfset_junctions_count(h))
    rec = _copy_records(lib.kg_orfset_junctions_copy, h, nj, N.JUNCTION_DTYPE)
    start = np.zeros(n + 1, dtype=np.int64)
    N.check(lib.kg_orfset_junctions_start(h, start.ctypes.data))
    return rec, start, st.as_dict()


def repair_orfs(calls, seq, offsets, merge_gap: int = 600, min_score: int = 0, min_len: int = 0, start_codons: int = 7,
                only_kept: bool = True, min_count: int = 0, max_junctions: int = 4, device: int = 0, device_inputs: bool = False,
                repair_calls=None, stats: Optional[dict] = None):
    """Function regions, their ORFs and the frameshift repair from caller-held CALL records of a DNA scan, on the GPU
    (kg_regions_calls, kg_regionset_orfs, kg_regionset_repair; include/kmerguts_hip.h states the rule): calls CALL_DTYPE in
    non-decreasing container order, seq / offsets the batch.
    -> (regions, region_start, orfs, prot_start, residues, junctions, junction_start): orfs index-aligned with regions, the
    record and protein of every repaired region replaced by the chain through its frames (flag _native.ORF_REPAIRED);
    junctions _native.JUNCTION_DTYPE in (orf, k) order, ORF i owning [junction_start[i], junction_start[i + 1]).
    device_inputs: the CALLs and the bytes are handed to the repair step as device memory (uploaded with torch first).
    repair_calls: the CALL list the repair step is given, when it is not `calls` (it must describe the same regions, or the
    call fails with KG_ERR_ARG).  `stats`, when given, receives "regions", "orfs" (the new set's) and "repair"."""
    lib = N.load()
    off = _offsets(offsets, "int64[n_seqs + 1]")
    c = np.ascontiguousarray(calls, dtype=N.CALL_DTYPE)
    rc = c if repair_calls is None else np.ascontiguousarray(repair_calls, dtype=N.CALL_DTYPE)
    keep = _seq_bytes(seq, off)
    n_seqs = off.size - 1
    p = N.KgRegionParams(int(merge_gap), int(min_score), int(min_len))
    op = N.KgOrfParams(int(start_codons), int(bool(only_kept)), 0)
    rp = N.KgRepairParams(int(start_codons), int(min_count), int(max_junctions), 0)
    h, chain = C.c_void_p(), _OrfChain(lib)
    N.check(lib.kg_regions_calls(device, C.byref(p), _ptr(c), c.size, off.ctypes.data, n_seqs, C.byref(h)))
    try:
        chain.step(lambda oh, new: lib.kg_regionset_orfs(h, C.byref(op), _ptr(keep), 0, off.ctypes.data, n_seqs, new))
        cptr, sptr, on_device = _ptr(rc), _ptr(keep), 0
        if device_inputs:
            import torch
            with torch.cuda.device(device):
                d_calls = torch.from_numpy(rc.view(np.uint8).reshape(-1).copy()).cuda()
                d_seq = torch.from_numpy(keep.copy()).cuda()
                torch.cuda.synchronize()
            cptr, sptr, on_device = C.c_void_p(d_calls.data_ptr() if rc.size else None), C.c_void_p(d_seq.data_ptr() if keep.size else None), 1
        chain.step(lambda oh, new: lib.kg_regionset_repair(h, oh, cptr, on_device, rc.size, C.byref(rp), sptr, on_device, off.ctypes.data,
                                                           n_seqs, new))
        junc, jstart, rst = _junctions(chain.h)
        orfs, prot_start, residues, ost = _take_orfset(chain.release(), False)
    except BaseException:
        chain.close()                           # (the ORF set first: it holds blocks of the region set's context)
        lib.kg_regionset_free(h)
        raise
    regs, start, rgst = _take_regionset(h, n_seqs, False)
    if stats is not None:
        stats.update({"regions": rgst, "orfs": ost, "repair": rst})
    return regs, start, orfs, prot_start, residues, junc, jstart


def _table_arg(table) -> np.ndarray:
    t = np.ascontiguousarray(table, dtype=np.int32)
    if t.shape != (N.CODING_BINS,):
        raise ValueError("a coding score table is int32[%d]" % N.CODING_BINS)
    return t


def _coding_arg(coding):
    """The coding= of ScanResult.orfs / select, checked before any set is made: None or False -> None (off), True -> True (train
    on the set), anything else -> the int32[4096] table it is."""
    if coding is None or coding is False:
        return None
    return True if coding is True else _table_arg(coding)


def _coding_results(h):
    """-> (scores int64[n], statistics, (coding, background) counts) of a set made by kg_orfset_coding; the set is freed when a
    call fails."""
    lib = N.load()
    try:
        n = int(lib.kg_orfset_count(h))
        scores = _copy_records(lib.kg_orfset_coding_scores, h, n, np.int64)
        st, m = N.KgCodingStats(), N.KgCodingModel()
        N.check(lib.kg_orfset_coding_stats(h, C.byref(st)))
        N.check(lib.kg_orfset_coding_model(h, C.byref(m)))
        return scores, st.as_dict(), (np.array(m.coding, dtype=np.int64), np.array(m.background, dtype=np.int64))
    except BaseException:
        lib.kg_orfset_free(h)
        h.value = None
        raise


def _weights_arg(weights):
    """A (pos, type) weights pair -> a KgStartWeights."""
    try:
        pos, typ = weights
    except (TypeError, ValueError):
        raise ValueError("start weights are a pair (pos int32[%d][4], type int32[4])" % N.START_WINDOW) from None
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    typ = np.ascontiguousarray(typ, dtype=np.int32)
    if pos.shape != (N.START_WINDOW, 4) or typ.shape != (4,):
        raise ValueError("start weights are a pair (pos int32[%d][4], type int32[4])" % N.START_WINDOW)
    w = N.KgStartWeights()
    C.memmove(w.pos, pos.ctypes.data, pos.nbytes)
    C.memmove(w.type, typ.ctypes.data, typ.nbytes)
    return w


def _starts_arg(starts, coding):
    """The starts= of ScanResult.orfs / select, checked before any set is made: None or False -> None (off), True -> True (train
    on the set), anything else -> the KgStartWeights of the pair it is.  coding: what _coding_arg gave."""
    if starts is None or starts is False:
        return None
    if coding is None:
        raise ValueError("starts needs coding: the start-site score's coding half is the coding step's table")
    return True if starts is True else _weights_arg(starts)


def _start_model_arrays(m):
    return (np.array(m.chosen, dtype=np.int64).reshape(N.START_WINDOW, 4), np.array(m.cand, dtype=np.int64).reshape(N.START_WINDOW, 4),
            np.array(m.type_chosen, dtype=np.int64), np.array(m.type_cand, dtype=np.int64))


def _starts_results(h):
    """-> (shifts int32[n], statistics, (chosen, cand, type_chosen, type_cand) counts) of a set made by kg_orfset_starts; the set is
    freed when a call fails."""
    lib = N.load()
    try:
        n = int(lib.kg_orfset_count(h))
        shifts = _copy_records(lib.kg_orfset_start_shifts, h, n, np.int32)
        st, m = N.KgStartStats(), N.KgStartModel()
        N.check(lib.kg_orfset_start_stats(h, C.byref(st)))
        N.check(lib.kg_orfset_start_model(h, C.byref(m)))
        return shifts, st.as_dict(), _start_model_arrays(m)
    except BaseException:
        lib.kg_orfset_free(h)
        h.value = None
        raise


def start_weights(chosen, cand, type_chosen, type_cand):
    """The weights of a start model's counts (kg_start_weights_from; include/kmerguts_hip.h states the rule: integer log-odds of
    the chosen starts' upstream bases and types against all candidates').  Host code: no GPU takes part.
    -> (pos int32[20][4], type int32[4])."""
    m = N.KgStartModel()
    for name, src, shape in (("chosen", chosen, (N.START_WINDOW, 4)), ("cand", cand, (N.START_WINDOW, 4)),
                             ("type_chosen", type_chosen, (4,)), ("type_cand", type_cand, (4,))):
        a = np.ascontiguousarray(src, dtype=np.int64)
        if a.shape != shape:
            raise ValueError("%s counts are int64%s" % (name, "".join("[%d]" % d for d in shape)))
        C.memmove(getattr(m, name), a.ctypes.data, a.nbytes)
    w = N.KgStartWeights()
    N.check(N.load().kg_start_weights_from(C.byref(m), C.byref(w)))
    return np.array(w.pos, dtype=np.int32).reshape(N.START_WINDOW, 4), np.array(w.type, dtype=np.int32)


def choose_starts(table, orfs, seq, offsets, weights=None, limits=None, min_res: int = 100, start_codons: int = 7, rounds: int = 4,
                  min_train_starts: int = 200, device: int = 0, stats: Optional[dict] = None, model: Optional[list] = None):
    """The start codon of every movable caller-held ORF record, chosen by the start-site score on the GPU and without a table
    (kg_starts_orfs; include/kmerguts_hip.h states the rule).  table: the int32[4096] coding table; weights: None to train on the
    records in `rounds` rounds, or a (pos, type) pair; limits: None or int32[n], the largest k of every record, -1 for none.
    -> (orfs, shifts): the records after the move and the shift of each in codons.  `stats`, when given, receives the call's
    counts and device times; `model`, when given, is extended by the last round's (chosen, cand, type_chosen, type_cand)."""
    off = _offsets(offsets, "int64[n_seqs + 1]")
    t = _table_arg(table)
    o = np.ascontiguousarray(orfs, dtype=N.ORF_DTYPE)
    arr = _seq_bytes(seq, off)
    w = None if weights is None else _weights_arg(weights)
    lim = None
    if limits is not None:
        lim = np.ascontiguousarray(limits, dtype=np.int32)
        if lim.shape != o.shape:
            raise ValueError("limits are int32[n], one per record")
    sp = N.KgStartParams(int(min_res), int(start_codons), int(rounds), 0, int(min_train_starts))
    out = np.zeros(o.size, dtype=N.ORF_DTYPE)
    shifts = np.zeros(o.size, dtype=np.int32)
    st, m = N.KgStartStats(), N.KgStartModel()
    N.check(N.load().kg_starts_orfs(device, C.byref(sp), t.ctypes.data, None if w is None else C.addressof(w),
                                    _ptr(o), o.size, _ptr(lim),
                                    _ptr(arr), off.ctypes.data, off.size - 1,
                                    _ptr(out), _ptr(shifts), C.byref(m), C.byref(st)))
    if stats is not None:
        stats.update(st.as_dict())
    if model is not None:
        model.extend(_start_model_arrays(m))
    return out, shifts


def start_counts(table, orfs, seq, offsets, limits=None, min_res: int = 100, start_codons: int = 7, rounds: int = 4, device: int = 0):
    """The counts of a start model trained on caller-held ORF records in `rounds` rounds (kg_starts_orfs without weights and
    with min_train_starts = 0): -> (chosen int64[20][4], cand int64[20][4], type_chosen int64[4], type_cand int64[4]), what the
    last round counted before it chose."""
    model: list = []
    choose_starts(table, orfs, seq, offsets, None, limits, min_res, start_codons, rounds, 0, device, None, model)
    return tuple(model)


def coding_table(coding, background) -> np.ndarray:
    """The int32[4096] score table of a coding model's counts (kg_coding_table; include/kmerguts_hip.h states the rule: integer
    log-odds of the in-frame hexamers against the background's).  Host code: no GPU takes part."""
    m = N.KgCodingModel()
    for name, src in (("coding", coding), ("background", background)):
        a = np.ascontiguousarray(src, dtype=np.int64)
        if a.shape != (N.CODING_BINS,):
            raise ValueError("%s counts are int64[%d]" % (name, N.CODING_BINS))
        C.memmove(getattr(m, name), a.ctypes.data, a.nbytes)
    out = np.zeros(N.CODING_BINS, dtype=np.int32)
    N.check(N.load().kg_coding_table(C.byref(m), out.ctypes.data))
    return out


def coding_counts(orfs, seq, offsets, device: int = 0):
    """The coding and background hexamer counts of caller-held ORF records and their batch, on the GPU and without a table
    (kg_coding_counts_orfs): orfs ORF_DTYPE, seq the batch's bytes, offsets int64[n_seqs + 1].  -> (coding, background), int64[4096]
    each; a record trains when it is kept and neither free nor interrupted."""
    off = _offsets(offsets, "int64[n_seqs + 1]")
    o = np.ascontiguousarray(orfs, dtype=N.ORF_DTYPE)
    arr = _seq_bytes(seq, off)
    m = N.KgCodingModel()
    N.check(N.load().kg_coding_counts_orfs(device, _ptr(o), o.size, _ptr(arr),
                                           off.ctypes.data, off.size - 1, C.byref(m)))
    return np.array(m.coding, dtype=np.int64), np.array(m.background, dtype=np.int64)


def coding_scores(table, orfs, seq, offsets, device: int = 0) -> np.ndarray:
    """The hexamer log-odds score of every caller-held ORF record under an int32[4096] table, on the GPU (kg_coding_score_orfs).
    -> int64[n]."""
    off = _offsets(offsets, "int64[n_seqs + 1]")
    t = _table_arg(table)
    o = np.ascontiguousarray(orfs, dtype=N.ORF_DTYPE)
    arr = _seq_bytes(seq, off)
    out = np.zeros(o.size, dtype=np.int64)
    N.check(N.load().kg_coding_score_orfs(device, t.ctypes.data, _ptr(o), o.size,
                                          _ptr(arr), off.ctypes.data, off.size - 1,
                                          _ptr(out)))
    return out


def free_orfs(seq, offsets, min_res: int = 100, start_codons: int = 7, device: int = 0, device_out: bool = False,
              stats: Optional[dict] = None):
    """The evidence-free open reading frames of a batch and their proteins, on the GPU and without a table (kg_orfs_free;
    include/kmerguts_hip.h states the rule): every stop-free run of the six frames that gives at least min_res residues from
    its first start codon.  seq the batch's bytes, offsets int64[n_seqs + 1].  -> (orfs, prot_start, residues) as orf_regions;
    `stats`, when given, receives the call's counts and device time."""
    off = _offsets(offsets, "int64[n_seqs + 1]")
    arr = _seq_bytes(seq, off)
    p = N.KgFreeParams(int(min_res), int(start_codons), 0)
    h = C.c_void_p()
    N.check(N.load().kg_orfs_free(device, C.byref(p), _ptr(arr), 0, off.ctypes.data, off.size - 1,
                                  C.byref(h)))
    out, start, res, st = _take_orfset(h, device_out)
    if stats is not None:
        stats.update(st)
    return out, start, res


def orf_regions(regs, seq, offsets, start_codons: int = 7, only_kept: bool = True, device: int = 0, device_out: bool = False,
                stats: Optional[dict] = None):
    """The open reading frame around every caller-held region and its translated protein, on the GPU (kg_orfs_regions): regs
    REGION_DTYPE, seq the batch's bytes, offsets int64[n_seqs + 1].  -> (orfs, prot_start, residues): numpy arrays of
    _native.ORF_DTYPE, int64[n + 1] and uint8, or with device_out=True CUDA tensors (uint8 of 48 bytes per ORF, int64, uint8);
    `stats`, when given, receives the call's counts and device time."""
    off = _offsets(offsets, "int64[n_seqs + 1]")
    r = np.ascontiguousarray(regs, dtype=N.REGION_DTYPE)
    arr = _seq_bytes(seq, off)
    p = N.KgOrfParams(int(start_codons), int(bool(only_kept)), 0)
    h = C.c_void_p()
    N.check(N.load().kg_orfs_regions(device, C.byref(p), _ptr(r), r.size,
                                     _ptr(arr), off.ctypes.data, off.size - 1, C.byref(h)))
    out, start, res, st = _take_orfset(h, device_out)
    if stats is not None:
        stats.update(st)
    return out, start, res


def _take_selectset(h, device_out: bool):
    """Copy a kg_selectset out (to the host, or into a CUDA tensor) and free it.  -> (records, statistics)."""
    lib = N.load()
    try:
        st = N.KgSelectStats()
        N.check(lib.kg_selectset_stats(h, C.byref(st)))
        return _copy_records(lib.kg_selectset_copy, h, int(lib.kg_selectset_count(h)), N.SELECTION_DTYPE, device_out=device_out), st.as_dict()
    finally:
        lib.kg_selectset_free(h)


def select_intervals(iv, n_seqs: int, max_overlap: int = 60, max_overlap_pct: int = 50, device_out: bool = False,
                     stats: Optional[dict] = None, device: int = 0):
    """The non-overlapping selection among caller-held candidates, on the GPU (kg_select_intervals): iv INTERVAL_DTYPE in any
    order, `seq` in [0, n_seqs).  -> a numpy array of _native.SELECTION_DTYPE index-aligned with iv, or with device_out=True a
    CUDA uint8 tensor of 8 bytes per candidate; `stats`, when given, receives the call's counts, rounds and device time."""
    a = np.ascontiguousarray(iv, dtype=N.INTERVAL_DTYPE)
    p = N.KgSelectParams(int(max_overlap), int(max_overlap_pct), 0)
    h = C.c_void_p()
    N.check(N.load().kg_select_intervals(device, C.byref(p), _ptr(a), a.size, int(n_seqs), C.byref(h)))
    out, st = _take_selectset(h, device_out)
    if stats is not None:
        stats.update(st)
    return out
