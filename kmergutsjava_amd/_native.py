"""ctypes binding of libkmerguts_hip.so (C ABI: include/kmerguts_hip.h).

The library is the product path.  If it is missing or cannot be loaded this module raises:
there is no CPU fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KG_LIB_PATH") or os.path.join(HERE, "libkmerguts_hip.so")   # KG_LIB_PATH: tuning builds only

KG_OK = 0
KG_ERR_ARG = -1
KG_ERR_IO = -2
KG_ERR_FORMAT = -3
KG_ERR_DEVICE = -4
KG_ERR_NOMEM = -5
KG_ERR_LIMIT = -7
KG_ERR_BUSY = -8
KG_F_COUNTERS = 1
KG_F_SKIP_AGGREGATE = 2
KG_F_PROGRESS = 4
KG_OI_BUFSZ = 5

# every symbol include/kmerguts_hip.h declares
EXPORTS = (
    "kg_table_open", "kg_table_from_memory", "kg_table_from_device", "kg_table_build", "kg_table_build_device", "kg_table_save",
    "kg_table_device_entries", "kg_table_records", "kg_table_info", "kg_table_live_device_bytes", "kg_table_close",
    "kg_scan", "kg_scan_device", "kg_aggregate_hits", "kg_process_set_of_hits", "kg_result_stats", "kg_result_hits", "kg_result_container_hit_start",
    "kg_result_calls", "kg_result_container_call_start", "kg_result_otu", "kg_result_hit_events",
    "kg_result_container_tail_events", "kg_result_copy_hits", "kg_result_hit_slots", "kg_result_progress", "kg_result_device_hits", "kg_result_device_calls", "kg_result_device_otu",
    "kg_result_device_container_hit_start", "kg_result_device_container_call_start", "kg_result_free", "kg_restore_hits_device",
    "kg_signatures_derive", "kg_signatures_derive_device", "kg_sigset_count", "kg_sigset_device", "kg_sigset_copy",
    "kg_sigset_stats", "kg_sigset_free", "kg_result_assign", "kg_assign_calls",
    "kg_table_merge_signatures", "kg_table_merge_signatures_device", "kg_sigset_merge_stats",
    "kg_proteins_cluster", "kg_proteins_cluster_device", "kg_familyset_count", "kg_familyset_copy", "kg_familyset_stats",
    "kg_familyset_free",
    "kg_proteins_align", "kg_proteins_align_device", "kg_proteins_cluster_aligned", "kg_proteins_cluster_aligned_device",
    "kg_familyset_edges_count", "kg_familyset_edges_copy", "kg_familyset_align_stats",
    "kg_proteins_align_paths", "kg_proteins_align_paths_device",
    "kg_proteins_align_ops", "kg_proteins_align_ops_device", "kg_opset_ops_count", "kg_opset_op_starts_copy", "kg_opset_ops_copy",
    "kg_opset_ms_ops", "kg_opset_free",
    "kg_hitset_ops_count", "kg_hitset_op_starts_copy", "kg_hitset_ops_copy", "kg_hitset_ms_ops",
    "kg_proteins_search", "kg_proteins_search_device", "kg_hitset_count", "kg_hitset_copy", "kg_hitset_starts_copy",
    "kg_hitset_stats", "kg_hitset_free",
    "kg_proteins_search_paths", "kg_proteins_search_paths_device", "kg_hitset_paths_copy", "kg_hitset_trace_stats",
    "kg_seed_params_builtin", "kg_proteins_search_seeded", "kg_proteins_search_seeded_device",
    "kg_proteins_mask", "kg_proteins_mask_device", "kg_maskset_count", "kg_maskset_copy", "kg_maskset_starts_copy",
    "kg_maskset_flags_copy", "kg_maskset_stats", "kg_maskset_free",
    "kg_proteins_search_masked", "kg_proteins_search_masked_device", "kg_hitset_mask_stats",
    "kg_proteins_cluster_masked", "kg_proteins_cluster_masked_device", "kg_familyset_mask_stats",
    "kg_proteins_search_filtered", "kg_proteins_search_filtered_device", "kg_hitset_ungapped_copy", "kg_hitset_ungapped_stats",
    "kg_proteins_align_banded", "kg_proteins_align_banded_device", "kg_proteins_search_banded", "kg_proteins_search_banded_device",
    "kg_hitset_band_stats",
    "kg_searchdb_build", "kg_searchdb_build_device", "kg_searchdb_save", "kg_searchdb_open", "kg_searchdb_info",
    "kg_searchdb_names_copy", "kg_searchdb_live_device_bytes", "kg_searchdb_reserve", "kg_searchdb_free",
    "kg_searchdb_search", "kg_searchdb_search_device", "kg_hitset_db_stats",
    "kg_contigs_search_translated", "kg_evidence_fragments", "kg_evidence_hits", "kg_evidence_calls_count", "kg_evidence_calls_copy",
    "kg_evidence_calls_device", "kg_evidence_call_hits_copy", "kg_evidence_stats", "kg_evidence_free",
    "kg_contigs_search_residual", "kg_result_search_residual", "kg_residual_searched_fragments", "kg_residual_searched_copy",
    "kg_residual_explain_copy", "kg_residual_call_kinds_copy", "kg_residual_call_sources_copy", "kg_residual_stats_of",
    "kg_result_regions", "kg_regions_calls", "kg_regionset_count", "kg_regionset_device", "kg_regionset_copy",
    "kg_regionset_seq_start", "kg_regionset_stats", "kg_regionset_free",
    "kg_regionset_orfs", "kg_orfs_regions", "kg_orfset_count", "kg_orfset_device", "kg_orfset_copy", "kg_orfset_prot_start",
    "kg_orfset_residues", "kg_orfset_stats", "kg_orfset_free", "kg_orfs_free", "kg_orfset_add_free",
    "kg_regionset_repair", "kg_result_repair", "kg_orfset_junctions_count", "kg_orfset_junctions_copy", "kg_orfset_junctions_start",
    "kg_orfset_junctions_stats",
    "kg_orfset_coding", "kg_orfset_coding_scores", "kg_orfset_coding_stats", "kg_orfset_coding_model", "kg_coding_table",
    "kg_coding_counts_orfs", "kg_coding_score_orfs",
    "kg_orfset_starts", "kg_orfset_start_shifts", "kg_orfset_start_stats", "kg_orfset_start_model", "kg_start_weights_from",
    "kg_starts_orfs",
    "kg_regionset_select", "kg_orfset_select", "kg_select_intervals", "kg_selectset_count", "kg_selectset_device",
    "kg_selectset_copy", "kg_selectset_stats", "kg_selectset_free",
    "kg_result_otu_votes", "kg_otu_votes_hits", "kg_voteset_count", "kg_voteset_bins", "kg_voteset_copy_votes",
    "kg_voteset_copy_classes", "kg_voteset_copy_bins", "kg_voteset_seq_start", "kg_voteset_stats", "kg_voteset_free",
    "kg_contigs_compose", "kg_compset_rows", "kg_compset_models", "kg_compset_copy_classes", "kg_compset_copy_counts",
    "kg_compset_copy_rows", "kg_compset_background", "kg_compset_model_labels", "kg_compset_copy_scores", "kg_compset_stats",
    "kg_compset_free",
    "kg_last_error", "kg_version",
)

# event bits (include/kmerguts_hip.h KG_EV_*)
EV_ACCEPTED, EV_RESET_BEFORE, EV_CALL_BEFORE, EV_KEEP2_BEFORE = 0x01, 0x02, 0x04, 0x08
EV_RESET_AFTER, EV_CALL_AFTER, EV_KEEP2_AFTER = 0x10, 0x20, 0x40
EV_TAIL_CALL = 0x01

HIT_DTYPE = np.dtype([("container", "<u4"), ("from0InProt", "<i4"), ("oI", "<i4"),
                      ("avgOffFromEnd", "<i4"), ("fI", "<i4"), ("functionWt", "<f4")])
CALL_DTYPE = np.dtype([("container", "<u4"), ("start", "<i4"), ("end", "<i4"), ("count", "<i4"),
                       ("fI", "<i4"), ("weightedHits", "<f4")])
OTU_DTYPE = np.dtype([("n", "<i4"), ("count", "<i4", (KG_OI_BUFSZ,)), ("oI", "<i4", (KG_OI_BUFSZ,))])
# struct kg_signature: the field layout of one kmer.table.mem_map record (KGJ:995-999)
SIGNATURE_DTYPE = np.dtype([("kmer", "<i8"), ("otuIndex", "<i4"), ("avgFromEnd", "<i4"), ("functionIndex", "<i4"),
                            ("functionWt", "<f4")])
assert SIGNATURE_DTYPE.itemsize == 24
# struct kg_assignment (kg_result_assign / kg_assign_calls): one function per protein of an -a scan
ASSIGNMENT_DTYPE = np.dtype([("fI", "<i4"), ("assigned", "<i4"), ("score", "<i4"), ("total", "<i4"), ("weighted", "<f4"),
                             ("n_calls", "<i4"), ("n_functions", "<i4"), ("second_fi", "<i4"), ("second_score", "<i4"),
                             ("otu", "<i4")])
assert ASSIGNMENT_DTYPE.itemsize == 40
# struct kg_region (kg_result_regions / kg_regions_calls): one function region of a contig
REGION_DTYPE = np.dtype([("seq", "<i4"), ("strand", "<i4"), ("left", "<i4"), ("right", "<i4"), ("fI", "<i4"), ("score", "<i4"),
                         ("weighted", "<f4"), ("n_calls", "<i4"), ("frames", "<u4"), ("best_frame", "<i4"),
                         ("first_call", "<u4"), ("kept", "<i4")])
assert REGION_DTYPE.itemsize == 48
# struct kg_orf (kg_regionset_orfs / kg_orfs_regions): the open reading frame around one function region
ORF_DTYPE = np.dtype([("seq", "<i4"), ("strand", "<i4"), ("frame", "<i4"), ("left", "<i4"), ("right", "<i4"), ("n_res", "<i4"),
                      ("start_codon", "<i4"), ("first_inner", "<i4"), ("flags", "<u4"), ("fI", "<i4"), ("score", "<i4"),
                      ("kept", "<i4")])
assert ORF_DTYPE.itemsize == 48
ORF_HAS_STOP, ORF_PARTIAL5, ORF_INTERRUPTED, ORF_MULTI_FRAME = 1, 2, 4, 8
ORF_FREE = 16               # an evidence-free candidate (kg_orfs_free / kg_orfset_add_free)
ORF_NONCODING = 32          # a free ORF that kg_orfset_coding dropped (its kept is 0)
ORF_START_MOVED = 64        # a record whose start kg_orfset_starts moved downstream
ORF_REPAIRED = 128          # a record kg_regionset_repair replaced by the chain through its region's frames
# struct kg_junction (kg_regionset_repair): where a repaired ORF changes frame
JUNCTION_DTYPE = np.dtype([("orf", "<i4"), ("pos", "<i4"), ("from_frame", "<i4"), ("to_frame", "<i4"), ("res", "<i4"), ("gap", "<i4")])
assert JUNCTION_DTYPE.itemsize == 24
REPAIR_MAX_JUNCTIONS = 8    # kg_repair.hpp kRepairMaxJunctions: the largest max_junctions
START_WINDOW = 20           # upstream positions of a start model
START_CHUNK = 1024          # kg_starts.hpp kStartChunk: the codons of one workgroup of the codon passes (tests aim at its edges)
CODING_BINS = 4096          # hexamer indices: the entries of a coding model's two count arrays and of a score table
CODING_BG_TILE = 2048       # kg_coding.hpp kCodingBgTile: the hexamer starts of one workgroup step (tests aim at its edges) ...
CODING_BG_PER_LANE = 8      # ... kCodingBgPerLane: of one lane ...
CODING_MAX_GRID = 2048      # ... and kCodingMaxGrid: the workgroups the striding kernels have at most
ORF_TILE_CODONS = 128       # kg_orfs.hpp kOrfTile: the codons of one tile summary (tests aim at its edges)
# struct kg_interval (kg_select_intervals) and struct kg_selection (kg_*_select): a candidate and what became of it
INTERVAL_DTYPE = np.dtype([("seq", "<i4"), ("left", "<i4"), ("right", "<i4"), ("score", "<i4"), ("eligible", "<i4")])
SELECTION_DTYPE = np.dtype([("state", "<i4"), ("by", "<i4")])
assert INTERVAL_DTYPE.itemsize == 20 and SELECTION_DTYPE.itemsize == 8
SEL_NOT_ELIGIBLE, SEL_SELECTED, SEL_OVERLAPPED = 0, 1, 2
SELECT_PAIRS_PER_LANE = 8   # kg_select.hpp kSelectPairsPerLane: the pair slots of one lane (tests aim at its edges)
# struct kg_otu_vote, kg_otu_class and kg_otu_bin (kg_result_otu_votes / kg_otu_votes_hits): one (sequence, OTU) tally, one
# sequence's classification, one OTU's bin
VOTE_DTYPE = np.dtype([("seq", "<i4"), ("oI", "<i4"), ("votes", "<i4"), ("n_calls", "<i4")])
OTU_CLASS_DTYPE = np.dtype([("otu", "<i4"), ("assigned", "<i4"), ("votes", "<i4"), ("total", "<i4"), ("n_calls", "<i4"),
                            ("total_calls", "<i4"), ("n_otus", "<i4"), ("second_otu", "<i4"), ("second_votes", "<i4"),
                            ("reserved", "<i4")])
OTU_BIN_DTYPE = np.dtype([("oI", "<i4"), ("n_seqs", "<i4"), ("length", "<i8"), ("votes", "<i8"), ("n_calls", "<i8")])
assert VOTE_DTYPE.itemsize == 16 and OTU_CLASS_DTYPE.itemsize == 40 and OTU_BIN_DTYPE.itemsize == 32
# struct kg_comp_class (kg_contigs_compose): one contig's bin by tetranucleotide composition
COMP_CLASS_DTYPE = np.dtype([("label", "<i4"), ("best", "<i4"), ("second", "<i4"), ("decided", "<i4"), ("windows", "<i8"),
                             ("score_best", "<i8"), ("score_second", "<i8")])
assert COMP_CLASS_DTYPE.itemsize == 40
COMP_BINS = 256             # tetramer indices: the entries of a contig's counts and of a model row
COMP_TILE = 2048            # kg_compose.hpp kCompTile: the tetramer starts of one workgroup step (tests aim at its edges) ...
COMP_MAX_GRID = 2048        # ... kCompMaxGrid: the workgroups the count pass has at most ...
COMP_SCORE_TILE = 16        # ... and kCompScoreTile: the models of one LDS tile of the score pass
# struct kg_family (kg_proteins_cluster*): one protein's family
FAMILY_DTYPE = np.dtype([("family", "<i4"), ("root", "<i4"), ("best", "<i4"), ("shared", "<i4")])
assert FAMILY_DTYPE.itemsize == 16
# struct kg_alignment (kg_proteins_align*) and struct kg_family_edge (kg_proteins_cluster_aligned*)
ALIGNMENT_DTYPE = np.dtype([("score", "<i4"), ("self_a", "<i4"), ("self_b", "<i4"), ("end_a", "<i4"), ("end_b", "<i4"), ("status", "<i4")])
FAMILY_EDGE_DTYPE = np.dtype([("member", "<i4"), ("centre", "<i4"), ("shared", "<i4"), ("score", "<i4"), ("ref", "<i4"),
                              ("end_member", "<i4"), ("end_centre", "<i4"), ("status", "<i4")])
assert ALIGNMENT_DTYPE.itemsize == 24 and FAMILY_EDGE_DTYPE.itemsize == 32
ALIGN_REF_LONGER, ALIGN_REF_MEMBER = 0, 1
ALIGN_REFS = {"longer": ALIGN_REF_LONGER, "member": ALIGN_REF_MEMBER}
ALIGN_DEFAULT_MAX_CELLS = 1 << 26
ALIGN_ALIGNED, ALIGN_SKIPPED = 0, 1                     # kg_alignment.status
EDGE_KEPT, EDGE_CUT, EDGE_SKIPPED = 0, 1, 2             # kg_family_edge.status
ALIGN_LDS_COLS = 1024       # kg_align.hpp kAlignLdsCols: a longer second protein carries its stripes in device memory (tests aim at it)
# struct kg_alignment_path (kg_proteins_align_paths*): where a traced alignment starts and what its columns are
ALIGN_PATH_DTYPE = np.dtype([("start_a", "<i4"), ("start_b", "<i4"), ("identical", "<i4"), ("positive", "<i4"), ("gap_opens", "<i4"),
                             ("gap_cols_a", "<i4"), ("gap_cols_b", "<i4"), ("status", "<i4")])
assert ALIGN_PATH_DTYPE.itemsize == 32
PATH_TRACED, PATH_NONE, PATH_UNTRACED = 0, 1, 2         # kg_alignment_path.status
TRACE_DEFAULT_MAX_CELLS = 1 << 24
TRACE_HITS, TRACE_ALL = 1, 2
TRACE_MODES = {"hits": TRACE_HITS, "all": TRACE_ALL}
TRACE_OPS, TRACE_OPS_EQX = 4, 8                         # OR-ed into a search's trace; kg_proteins_align_ops' ops_mode
OPS_MODES = {"m": TRACE_OPS, "eqx": TRACE_OPS_EQX}
OP_M, OP_I, OP_D, OP_EQ, OP_X = 0, 1, 2, 7, 8           # an op is len << 4 | code
OP_LETTERS = {OP_M: "M", OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
# struct kg_search_hit (kg_proteins_search*): one aligned or skipped candidate of a query
SEARCH_HIT_DTYPE = np.dtype([("query", "<i4"), ("target", "<i4"), ("shared", "<i4"), ("score", "<i4"), ("self_query", "<i4"),
                             ("self_target", "<i4"), ("end_query", "<i4"), ("end_target", "<i4"), ("status", "<i4"), ("rank", "<i4")])
assert SEARCH_HIT_DTYPE.itemsize == 40
SEARCH_HIT, SEARCH_BELOW, SEARCH_SKIPPED = 0, 1, 2      # kg_search_hit.status
SEARCH_TILE = 2048          # kg_search.hpp kSearchTile: the join items of one workgroup (tests aim at its edges) ...
SEARCH_MAX_CAND = 64        # ... and kSearchMaxCand: the largest max_cand, one lane per candidate
# struct kg_mask_segment (kg_proteins_mask*): one low-complexity segment, residues start .. end of its protein, inclusive
MASK_SEGMENT_DTYPE = np.dtype([("protein", "<i4"), ("start", "<i4"), ("end", "<i4"), ("reserved", "<i4")])
assert MASK_SEGMENT_DTYPE.itemsize == 16
MASK_WINDOW, MASK_TRIGGER, MASK_EXTEND = 12, 563, 640   # the defaults: SEG's 2.2 and 2.5 bits in units of 1/256 bit
MASK_QUERIES, MASK_TARGETS = 1, 2                       # KG_MASK_*: the sides of kg_proteins_search_masked
MASK_SIDES = {"queries": MASK_QUERIES, "targets": MASK_TARGETS, "both": MASK_QUERIES | MASK_TARGETS}
MASK_TILE = 64              # kg_device.hpp kAaWinPerBlock: the window positions of one block and of one word (tests aim at its edges)
assert HIT_DTYPE.itemsize == 24 and CALL_DTYPE.itemsize == 24 and OTU_DTYPE.itemsize == 44


class KgParams(C.Structure):
    _fields_ = [("aa", C.c_int32), ("order_constraint", C.c_int32), ("min_hits", C.c_int32),
                ("min_weighted_hits", C.c_int32), ("max_gap", C.c_int32), ("flags", C.c_uint32)]


class KgStats(C.Structure):
    _fields_ = [("n_seqs", C.c_int64), ("n_containers", C.c_int64), ("n_blocks", C.c_int64),
                ("n_hits", C.c_int64), ("n_calls", C.c_int64), ("residues", C.c_int64),
                ("windows", C.c_int64), ("windows_valid", C.c_int64), ("slots_inspected", C.c_int64),
                ("table_bytes", C.c_int64), ("ms_scan", C.c_float), ("ms_order", C.c_float),
                ("ms_aggregate", C.c_float), ("ms_total", C.c_float), ("scan_launches", C.c_int32),
                ("partitioned", C.c_int32), ("ms_part_scatter", C.c_float), ("ms_part_tag", C.c_float),
                ("ms_part_verify", C.c_float), ("fallback", C.c_int32), ("part_chunks", C.c_int32),
                ("part_buckets", C.c_int32), ("part_shift", C.c_int32), ("lookup_ran_off", C.c_int32),
                ("agg_pieces", C.c_int32), ("part_levels", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class KgProgress(C.Structure):
    """struct kg_progress (KG_F_PROGRESS scans): what the reference's table stream would have reported (KGJ:1016-1049)."""
    _fields_ = [("first_visited", C.c_int64 * 11), ("last_visited", C.c_int64), ("first_beyond", C.c_int64),
                ("walk_ran_off", C.c_int64), ("stream_slots", C.c_int64), ("found_upto", C.c_int64 * 11), ("kmers_found", C.c_int64)]

    def as_dict(self):
        return {"first_visited": [int(x) for x in self.first_visited], "last_visited": int(self.last_visited),
                "first_beyond": int(self.first_beyond), "walk_ran_off": int(self.walk_ran_off), "stream_slots": int(self.stream_slots),
                "found_upto": [int(x) for x in self.found_upto], "kmers_found": int(self.kmers_found)}


class KgDeriveParams(C.Structure):
    """struct kg_derive_params (kg_signatures_derive*)."""
    _fields_ = [("min_proteins", C.c_int32), ("purity_pct", C.c_int32), ("max_windows_per_pass", C.c_int64)]


class KgDeriveStats(C.Structure):
    """struct kg_derive_stats."""
    _fields_ = [("proteins", C.c_int64), ("windows", C.c_int64), ("valid_windows", C.c_int64), ("pairs", C.c_int64),
                ("kmers", C.c_int64), ("signatures", C.c_int64), ("passes", C.c_int32), ("ms_encode", C.c_float),
                ("ms_sort", C.c_float), ("ms_reduce", C.c_float), ("ms_total", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


MERGE_KEEP, MERGE_REPLACE, MERGE_DROP = 0, 1, 2
MERGE_POLICIES = {"keep": MERGE_KEEP, "replace": MERGE_REPLACE, "drop": MERGE_DROP}


class KgMergeParams(C.Structure):
    """struct kg_merge_params (kg_table_merge_signatures*)."""
    _fields_ = [("on_conflict", C.c_int32), ("reserved", C.c_int32)]


class KgMergeStats(C.Structure):
    """struct kg_merge_stats."""
    _fields_ = [("base", C.c_int64), ("base_ignored", C.c_int64), ("added_in", C.c_int64), ("added", C.c_int64),
                ("conflicts", C.c_int64), ("conflicts_same_function", C.c_int64), ("replaced", C.c_int64), ("dropped", C.c_int64),
                ("merged", C.c_int64), ("ms_extract", C.c_float), ("ms_sort", C.c_float), ("ms_resolve", C.c_float),
                ("ms_total", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KgAssignParams(C.Structure):
    """struct kg_assign_params (kg_result_assign / kg_assign_calls)."""
    _fields_ = [("min_score", C.c_int32), ("min_share_pct", C.c_int32)]


class KgRegionParams(C.Structure):
    """struct kg_region_params (kg_result_regions / kg_regions_calls)."""
    _fields_ = [("merge_gap", C.c_int32), ("min_score", C.c_int32), ("min_len", C.c_int32)]


class KgRegionStats(C.Structure):
    """struct kg_region_stats."""
    _fields_ = [("calls", C.c_int64), ("groups", C.c_int64), ("regions", C.c_int64), ("kept", C.c_int64),
                ("multi_frame", C.c_int64), ("ms", C.c_float), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class KgOrfParams(C.Structure):
    """struct kg_orf_params (kg_regionset_orfs / kg_orfs_regions)."""
    _fields_ = [("start_codons", C.c_int32), ("only_kept", C.c_int32), ("reserved", C.c_int32)]


class KgOrfStats(C.Structure):
    """struct kg_orf_stats."""
    _fields_ = [("orfs", C.c_int64), ("complete", C.c_int64), ("interrupted", C.c_int64), ("partial5", C.c_int64),
                ("residues", C.c_int64), ("tiles", C.c_int64), ("ms", C.c_float), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class KgFreeParams(C.Structure):
    """struct kg_free_params (kg_orfs_free / kg_orfset_add_free)."""
    _fields_ = [("min_res", C.c_int32), ("start_codons", C.c_int32), ("reserved", C.c_int32)]


FREE_PARAMS = KgFreeParams


class KgRepairParams(C.Structure):
    """struct kg_repair_params (kg_regionset_repair / kg_result_repair)."""
    _fields_ = [("start_codons", C.c_int32), ("min_count", C.c_int32), ("max_junctions", C.c_int32), ("reserved", C.c_int32)]


class KgRepairStats(C.Structure):
    """struct kg_repair_stats."""
    _fields_ = [("candidates", C.c_int64), ("repaired", C.c_int64), ("failed", C.c_int64), ("single", C.c_int64),
                ("skipped", C.c_int64), ("junctions", C.c_int64), ("residues", C.c_int64), ("ms", C.c_float), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class KgCodingParams(C.Structure):
    """struct kg_coding_params (kg_orfset_coding)."""
    _fields_ = [("min_coding", C.c_int32), ("reserved", C.c_int32), ("min_train_pairs", C.c_int64)]


class KgCodingModel(C.Structure):
    """struct kg_coding_model: the coding and the background count of every hexamer index."""
    _fields_ = [("coding", C.c_int64 * 4096), ("background", C.c_int64 * 4096)]


class KgCodingStats(C.Structure):
    """struct kg_coding_stats."""
    _fields_ = [("scored", C.c_int64), ("training_records", C.c_int64), ("training_pairs", C.c_int64), ("background", C.c_int64),
                ("noncoding", C.c_int64), ("trained", C.c_int32), ("ms_count", C.c_float), ("ms_score", C.c_float),
                ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class KgStartParams(C.Structure):
    """struct kg_start_params (kg_orfset_starts / kg_starts_orfs)."""
    _fields_ = [("min_res", C.c_int32), ("start_codons", C.c_int32), ("rounds", C.c_int32), ("reserved", C.c_int32),
                ("min_train_starts", C.c_int64)]


class KgStartModel(C.Structure):
    """struct kg_start_model: the chosen and the candidate counts of every window base and of every start type."""
    _fields_ = [("chosen", C.c_int64 * 4 * 20), ("cand", C.c_int64 * 4 * 20), ("type_chosen", C.c_int64 * 4),
                ("type_cand", C.c_int64 * 4)]


class KgStartWeights(C.Structure):
    """struct kg_start_weights."""
    _fields_ = [("pos", C.c_int32 * 4 * 20), ("type", C.c_int32 * 4)]


class KgStartStats(C.Structure):
    """struct kg_start_stats."""
    _fields_ = [("movable", C.c_int64), ("training_records", C.c_int64), ("candidates", C.c_int64), ("moved", C.c_int64),
                ("rounds_run", C.c_int32), ("trained", C.c_int32), ("ms_count", C.c_float), ("ms_choose", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KgSelectParams(C.Structure):
    """struct kg_select_params (kg_regionset_select / kg_orfset_select / kg_select_intervals)."""
    _fields_ = [("max_overlap", C.c_int32), ("max_overlap_pct", C.c_int32), ("reserved", C.c_int32)]


class KgSelectStats(C.Structure):
    """struct kg_select_stats."""
    _fields_ = [("candidates", C.c_int64), ("eligible", C.c_int64), ("selected", C.c_int64), ("overlapped", C.c_int64),
                ("pairs", C.c_int64), ("conflicts", C.c_int64), ("rounds", C.c_int32), ("ms", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KgClusterParams(C.Structure):
    """struct kg_cluster_params (kg_proteins_cluster*)."""
    _fields_ = [("min_shared", C.c_int32), ("min_cover_pct", C.c_int32), ("reserved", C.c_int32)]


class KgClusterStats(C.Structure):
    """struct kg_cluster_stats."""
    _fields_ = [("proteins", C.c_int64), ("valid_windows", C.c_int64), ("pairs", C.c_int64), ("kmers", C.c_int64),
                ("links", C.c_int64), ("edges", C.c_int64), ("families", C.c_int64), ("families_multi", C.c_int64),
                ("largest", C.c_int64), ("rounds", C.c_int32), ("ms_encode", C.c_float), ("ms_sort", C.c_float),
                ("ms_link", C.c_float), ("ms_components", C.c_float), ("ms_total", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KgAlignParams(C.Structure):
    """struct kg_align_params (kg_proteins_align* / kg_proteins_cluster_aligned*)."""
    _fields_ = [("min_ratio_pct", C.c_int32), ("ref", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32),
                ("max_cells", C.c_int64), ("matrix", C.c_void_p), ("reserved", C.c_int64)]


class KgAlignStats(C.Structure):
    """struct kg_align_stats."""
    _fields_ = [("aligned", C.c_int64), ("cut", C.c_int64), ("skipped", C.c_int64), ("cells", C.c_int64), ("ms_align", C.c_float),
                ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class KgTraceStats(C.Structure):
    """struct kg_trace_stats."""
    _fields_ = [("traced", C.c_int64), ("untraced", C.c_int64), ("cells", C.c_int64), ("ms_trace", C.c_float), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class KgSearchParams(C.Structure):
    """struct kg_search_params (kg_proteins_search*)."""
    _fields_ = [("min_shared", C.c_int32), ("max_cand", C.c_int32), ("max_db_per_kmer", C.c_int32), ("reserved", C.c_int32)]


class KgSeedParams(C.Structure):
    """struct kg_seed_params (kg_proteins_search_seeded*): the class map in code order ACDEFGHIKLMNPQRSTVWY and up to four shapes."""
    _fields_ = [("n_shapes", C.c_int32), ("alphabet_size", C.c_int32), ("cls", C.c_uint8 * 20), ("shape", C.c_uint32 * 4),
                ("reserved", C.c_int32)]


SEEDS_EXACT, SEEDS_REDUCED = 0, 1       # KG_SEEDS_*: kg_seed_params_builtin


class KgSearchStats(C.Structure):
    """struct kg_search_stats."""
    _fields_ = [("targets", C.c_int64), ("queries", C.c_int64), ("valid_windows", C.c_int64), ("pairs", C.c_int64),
                ("kmers", C.c_int64), ("kmers_joined", C.c_int64), ("kmers_masked", C.c_int64), ("join_pairs", C.c_int64),
                ("candidates", C.c_int64), ("aligned", C.c_int64), ("hits", C.c_int64), ("skipped", C.c_int64),
                ("queries_hit", C.c_int64), ("cells", C.c_int64), ("ms_encode", C.c_float), ("ms_sort", C.c_float),
                ("ms_join", C.c_float), ("ms_align", C.c_float), ("ms_total", C.c_float), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class KgMaskParams(C.Structure):
    """struct kg_mask_params (kg_proteins_mask*, kg_proteins_search_masked*, kg_proteins_cluster_masked*)."""
    _fields_ = [("window", C.c_int32), ("trigger", C.c_int32), ("extend", C.c_int32), ("reserved", C.c_int32)]


class KgMaskSegment(C.Structure):
    """struct kg_mask_segment."""
    _fields_ = [("protein", C.c_int32), ("start", C.c_int32), ("end", C.c_int32), ("reserved", C.c_int32)]


class KgMaskStats(C.Structure):
    """struct kg_mask_stats."""
    _fields_ = [("proteins", C.c_int64), ("residues", C.c_int64), ("windows", C.c_int64), ("low_windows", C.c_int64),
                ("ext_windows", C.c_int64), ("masking_windows", C.c_int64), ("segments", C.c_int64), ("masked_residues", C.c_int64),
                ("proteins_masked", C.c_int64), ("ms_mask", C.c_float), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class KgUngappedParams(C.Structure):
    """struct kg_ungapped_params (kg_proteins_search_filtered*)."""
    _fields_ = [("min_ungapped", C.c_int32), ("reserved", C.c_int32 * 3)]


class KgUngappedStats(C.Structure):
    """struct kg_ungapped_stats."""
    _fields_ = [("scored", C.c_int64), ("dropped", C.c_int64), ("cut", C.c_int64), ("cells", C.c_int64), ("ms_ungapped", C.c_float),
                ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


BAND_MAX = 256                          # KG_BAND_MAX


class KgBandParams(C.Structure):
    """struct kg_band_params (kg_proteins_align_banded*, kg_proteins_search_banded*)."""
    _fields_ = [("band", C.c_int32), ("reserved", C.c_int32 * 3)]


class KgBandStats(C.Structure):
    """struct kg_band_stats."""
    _fields_ = [("band_cells", C.c_int64), ("full_cells", C.c_int64), ("band", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


SEARCHDB_VERSION, SEARCHDB_HEADER_BYTES, SEARCHDB_DEFAULT_ROOM = 1, 448, 1 << 24      # KG_SEARCHDB_*


class KgSearchDbDesc(C.Structure):
    """struct kg_searchdb_desc (kg_searchdb_info)."""
    _fields_ = [("targets", C.c_int64), ("residues", C.c_int64), ("pairs", C.c_int64), ("kmers", C.c_int64),
                ("valid_windows", C.c_int64), ("names_bytes", C.c_int64), ("query_room", C.c_int64), ("device_bytes", C.c_int64),
                ("has_seeds", C.c_int32), ("has_mask", C.c_int32), ("seeds", KgSeedParams), ("mask", KgMaskParams),
                ("mask_stats", KgMaskStats), ("ms_upload", C.c_float), ("ms_encode", C.c_float), ("ms_sort", C.c_float),
                ("ms_index", C.c_float), ("ms_total", C.c_float), ("reserved", C.c_int32)]


class KgSearchDbStats(C.Structure):
    """struct kg_search_db_stats (kg_hitset_db_stats)."""
    _fields_ = [("query_kmers", C.c_int64), ("found", C.c_int64), ("ms_probe", C.c_float), ("ms_upload", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KgTranslateParams(C.Structure):
    """struct kg_translate_params (kg_contigs_search_translated)."""
    _fields_ = [("min_res", C.c_int32), ("max_hits", C.c_int32), ("reserved", C.c_int32 * 2)]


class KgTranslateStats(C.Structure):
    """struct kg_translate_stats (kg_evidence_stats)."""
    _fields_ = [("fragments", C.c_int64), ("fragment_residues", C.c_int64), ("records", C.c_int64), ("calls", C.c_int64),
                ("dropped_status", C.c_int64), ("dropped_rank", C.c_int64), ("dropped_untraced", C.c_int64),
                ("ms_fragments", C.c_float), ("ms_search", C.c_float), ("ms_calls", C.c_float), ("ms_total", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


TRANSLATE_MIN_RES, TRANSLATE_MAX_HITS = 30, 1       # the defaults of kg_translate_params


class KgResidualParams(C.Structure):
    """struct kg_residual_params (kg_contigs_search_residual / kg_result_search_residual)."""
    _fields_ = [("explain_min", C.c_int64), ("min_db_count", C.c_int32), ("reserved", C.c_int32)]


class KgResidualStats(C.Structure):
    """struct kg_residual_stats (kg_residual_stats_of)."""
    _fields_ = [("sig_calls", C.c_int64), ("explained", C.c_int64), ("explained_residues", C.c_int64), ("searched", C.c_int64),
                ("searched_residues", C.c_int64), ("db_calls", C.c_int64), ("dropped_min_count", C.c_int64), ("merged", C.c_int64),
                ("ms_explain", C.c_float), ("ms_compact", C.c_float), ("ms_merge", C.c_float), ("ms_total", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


RESIDUAL_CHUNK = 16         # kg_residual.hpp kResidualChunk: the destination bytes of one lane of the residues' copy (tests aim at its edges)


# struct kg_search_ungapped (kg_hitset_ungapped_copy): one per hit record of a filtered search, same index
SEARCH_UNGAPPED_DTYPE = np.dtype([("ungapped", "<i4"), ("diagonal", "<i4"), ("on_diagonal", "<i4"), ("reserved", "<i4")])
assert SEARCH_UNGAPPED_DTYPE.itemsize == 16


class KgVoteParams(C.Structure):
    """struct kg_vote_params (kg_result_otu_votes / kg_otu_votes_hits)."""
    _fields_ = [("min_votes", C.c_int32), ("min_share_pct", C.c_int32), ("min_calls", C.c_int32), ("reserved", C.c_int32)]


class KgVoteStats(C.Structure):
    """struct kg_vote_stats."""
    _fields_ = [("hits", C.c_int64), ("accepted", C.c_int64), ("votes", C.c_int64), ("pairs", C.c_int64),
                ("seqs_with_votes", C.c_int64), ("assigned", C.c_int64), ("bins", C.c_int64), ("assigned_length", C.c_int64),
                ("total_length", C.c_int64), ("ms", C.c_float), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class KgCompParams(C.Structure):
    """struct kg_comp_params (kg_contigs_compose)."""
    _fields_ = [("min_len", C.c_int32), ("min_margin", C.c_int32), ("min_train", C.c_int64), ("keep_scores", C.c_int32),
                ("reserved", C.c_int32)]


class KgCompStats(C.Structure):
    """struct kg_comp_stats."""
    _fields_ = [("seqs", C.c_int64), ("labelled", C.c_int64), ("label_rows", C.c_int64), ("models", C.c_int64),
                ("windows", C.c_int64), ("decided", C.c_int64), ("decided_unlabelled", C.c_int64), ("conflicts", C.c_int64),
                ("ms_count", C.c_float), ("ms_score", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KmerGutsNativeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("libkmerguts_hip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load() -> C.CDLL:
    """Load the HIP library; raise loudly when it is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # libkmerguts_hip.so is linked against the system's libamdhip64; PyTorch ships a copy of its own under the same
    # SONAME.  Whichever is loaded first serves both, and torch.cuda only comes up on its own copy (measured on the GPU
    # box: library first, torch second -> torch.cuda.is_available() is False).  The package uses torch for device
    # tensors and torch.distributed, so torch's runtime goes first; KG_NO_TORCH_PRELOAD=1 skips the ~1.5 s import for
    # processes that never touch torch.cuda.
    if not os.environ.get("KG_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -m kmergutsjava_amd.build` "
            "(hipcc --offload-arch=gfx950).  kmergutsjava_amd has no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i64p = C.c_void_p, C.POINTER(C.c_int64)
    lib.kg_table_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    lib.kg_table_from_memory.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(vp)]
    lib.kg_table_from_device.argtypes = [vp, C.c_int64, C.c_int, C.POINTER(vp)]
    lib.kg_table_build.argtypes = [vp, C.c_int64, C.c_int64, C.c_int, i64p, C.POINTER(vp)]
    lib.kg_table_build_device.argtypes = [vp, C.c_int64, C.c_int64, C.c_int, i64p, C.POINTER(vp)]
    lib.kg_table_save.argtypes = [vp, C.c_char_p]
    lib.kg_table_device_entries.argtypes = [vp]
    lib.kg_table_device_entries.restype = vp
    lib.kg_table_records.argtypes = [vp]
    lib.kg_table_records.restype = C.c_int64
    lib.kg_table_info.argtypes = [vp, i64p, i64p, i64p, i64p]
    lib.kg_table_live_device_bytes.argtypes = [vp]
    lib.kg_table_live_device_bytes.restype = C.c_int64
    lib.kg_table_close.argtypes = [vp]
    lib.kg_table_close.restype = None
    lib.kg_scan.argtypes = [vp, C.POINTER(KgParams), vp, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_scan_device.argtypes = [vp, C.POINTER(KgParams), vp, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_aggregate_hits.argtypes = [C.c_int, C.POINTER(KgParams), vp, vp, C.c_int64, vp, C.POINTER(vp)]
    i32p = C.POINTER(C.c_int32)
    lib.kg_process_set_of_hits.argtypes = [C.c_int, C.POINTER(KgParams), vp, C.c_int32, C.c_int32, vp, vp, i32p, i32p, i32p]
    lib.kg_result_stats.argtypes = [vp, C.POINTER(KgStats)]
    for name in ("kg_result_hits", "kg_result_container_hit_start", "kg_result_calls",
                 "kg_result_container_call_start", "kg_result_otu", "kg_result_hit_events",
                 "kg_result_container_tail_events", "kg_result_device_hits", "kg_result_device_calls", "kg_result_device_otu",
                 "kg_result_device_container_hit_start", "kg_result_device_container_call_start"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = vp
    lib.kg_result_copy_hits.argtypes = [vp, C.c_int64, C.c_int64, vp]
    lib.kg_result_hit_slots.argtypes = [vp]
    lib.kg_result_hit_slots.restype = vp
    lib.kg_result_progress.argtypes = [vp, C.POINTER(KgProgress)]
    lib.kg_restore_hits_device.argtypes = [C.c_int, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp]
    lib.kg_result_free.argtypes = [vp]
    lib.kg_result_free.restype = None
    for name in ("kg_signatures_derive", "kg_signatures_derive_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgDeriveParams), vp, vp, C.c_int64, vp, vp, C.POINTER(vp)]
    lib.kg_sigset_stats.argtypes = [vp, C.POINTER(KgDeriveStats)]
    for name in ("kg_table_merge_signatures", "kg_table_merge_signatures_device"):
        getattr(lib, name).argtypes = [vp, C.POINTER(KgMergeParams), vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_sigset_merge_stats.argtypes = [vp, C.POINTER(KgMergeStats)]
    lib.kg_result_assign.argtypes = [vp, C.POINTER(KgAssignParams), vp, C.POINTER(C.c_float)]
    lib.kg_assign_calls.argtypes = [C.c_int, C.POINTER(KgAssignParams), vp, vp, C.c_int64, vp, vp]
    lib.kg_result_regions.argtypes = [vp, C.POINTER(KgRegionParams), vp, C.POINTER(vp)]
    lib.kg_regions_calls.argtypes = [C.c_int, C.POINTER(KgRegionParams), vp, C.c_int64, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_regionset_stats.argtypes = [vp, C.POINTER(KgRegionStats)]
    lib.kg_regionset_orfs.argtypes = [vp, C.POINTER(KgOrfParams), vp, C.c_int, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_orfs_regions.argtypes = [C.c_int, C.POINTER(KgOrfParams), vp, C.c_int64, vp, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_orfset_stats.argtypes = [vp, C.POINTER(KgOrfStats)]
    lib.kg_orfs_free.argtypes = [C.c_int, C.POINTER(KgFreeParams), vp, C.c_int, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_orfset_add_free.argtypes = [vp, C.POINTER(KgFreeParams), vp, C.c_int, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_regionset_repair.argtypes = [vp, vp, vp, C.c_int, C.c_int64, C.POINTER(KgRepairParams), vp, C.c_int, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_result_repair.argtypes = [vp, vp, vp, C.POINTER(KgRepairParams), vp, C.c_int, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_orfset_junctions_stats.argtypes = [vp, C.POINTER(KgRepairStats)]
    lib.kg_orfset_coding.argtypes = [vp, C.POINTER(KgCodingParams), vp, vp, C.c_int, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_orfset_coding_stats.argtypes = [vp, C.POINTER(KgCodingStats)]
    lib.kg_orfset_coding_model.argtypes = [vp, C.POINTER(KgCodingModel)]
    lib.kg_coding_table.argtypes = [C.POINTER(KgCodingModel), vp]
    lib.kg_coding_counts_orfs.argtypes = [C.c_int, vp, C.c_int64, vp, vp, C.c_int64, C.POINTER(KgCodingModel)]
    lib.kg_coding_score_orfs.argtypes = [C.c_int, vp, vp, C.c_int64, vp, vp, C.c_int64, vp]
    lib.kg_orfset_starts.argtypes = [vp, C.POINTER(KgStartParams), vp, vp, vp, vp, C.c_int, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_orfset_start_stats.argtypes = [vp, C.POINTER(KgStartStats)]
    lib.kg_orfset_start_model.argtypes = [vp, C.POINTER(KgStartModel)]
    lib.kg_start_weights_from.argtypes = [C.POINTER(KgStartModel), C.POINTER(KgStartWeights)]
    lib.kg_starts_orfs.argtypes = [C.c_int, C.POINTER(KgStartParams), vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, vp, vp, vp, vp]
    lib.kg_regionset_select.argtypes = [vp, C.POINTER(KgSelectParams), C.POINTER(vp)]
    lib.kg_orfset_select.argtypes = [vp, C.POINTER(KgSelectParams), C.POINTER(vp)]
    lib.kg_select_intervals.argtypes = [C.c_int, C.POINTER(KgSelectParams), vp, C.c_int64, C.c_int64, C.POINTER(vp)]
    lib.kg_selectset_stats.argtypes = [vp, C.POINTER(KgSelectStats)]
    lib.kg_result_otu_votes.argtypes = [vp, C.POINTER(KgVoteParams), vp, C.POINTER(vp)]
    lib.kg_otu_votes_hits.argtypes = [C.c_int, C.POINTER(KgVoteParams), vp, vp, vp, vp, vp, C.c_int64, C.c_int32, vp, C.POINTER(vp)]
    lib.kg_voteset_stats.argtypes = [vp, C.POINTER(KgVoteStats)]
    lib.kg_contigs_compose.argtypes = [C.c_int, C.POINTER(KgCompParams), vp, C.c_int, vp, C.c_int64, vp, vp, vp, C.c_int64, C.POINTER(vp)]
    lib.kg_compset_copy_rows.argtypes = [vp, C.c_int64, C.c_int64, vp, vp]
    lib.kg_compset_stats.argtypes = [vp, C.POINTER(KgCompStats)]
    for name in ("kg_proteins_cluster", "kg_proteins_cluster_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgClusterParams), vp, vp, C.c_int64, C.c_int64, C.POINTER(vp)]
    lib.kg_familyset_stats.argtypes = [vp, C.POINTER(KgClusterStats)]
    for name in ("kg_proteins_align", "kg_proteins_align_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgAlignParams), vp, vp, C.c_int64, vp, C.c_int64, vp]
    for name in ("kg_proteins_align_paths", "kg_proteins_align_paths_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgAlignParams), vp, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp]
    for name in ("kg_proteins_align_ops", "kg_proteins_align_ops_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgAlignParams), vp, vp, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int, vp, vp,
                                       C.POINTER(vp)]
    for name in ("kg_opset_ms_ops", "kg_hitset_ms_ops"):
        getattr(lib, name).argtypes = [vp, C.POINTER(C.c_float)]
    for name in ("kg_proteins_cluster_aligned", "kg_proteins_cluster_aligned_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgClusterParams), C.POINTER(KgAlignParams), vp, vp, C.c_int64, C.c_int64,
                                       C.POINTER(vp)]
    lib.kg_familyset_align_stats.argtypes = [vp, C.POINTER(KgAlignStats)]
    for name in ("kg_proteins_search", "kg_proteins_search_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgSearchParams), C.POINTER(KgAlignParams), vp, vp, C.c_int64, C.c_int64,
                                       C.c_int64, C.c_int64, C.POINTER(vp)]
    lib.kg_hitset_stats.argtypes = [vp, C.POINTER(KgSearchStats)]
    for name in ("kg_proteins_search_paths", "kg_proteins_search_paths_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgSearchParams), C.POINTER(KgAlignParams), vp, vp, C.c_int64, C.c_int64,
                                       C.c_int64, C.c_int64, C.c_int, C.c_int64, C.POINTER(vp)]
    lib.kg_hitset_trace_stats.argtypes = [vp, C.POINTER(KgTraceStats)]
    lib.kg_seed_params_builtin.argtypes = [C.c_int, C.POINTER(KgSeedParams)]
    for name in ("kg_proteins_search_seeded", "kg_proteins_search_seeded_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgSearchParams), C.POINTER(KgSeedParams), C.POINTER(KgAlignParams), vp, vp,
                                       C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.POINTER(vp)]
    for name in ("kg_proteins_mask", "kg_proteins_mask_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgMaskParams), vp, vp, C.c_int64, C.POINTER(vp)]
    for name in ("kg_maskset_stats", "kg_hitset_mask_stats", "kg_familyset_mask_stats"):
        getattr(lib, name).argtypes = [vp, C.POINTER(KgMaskStats)]
    for name in ("kg_proteins_search_masked", "kg_proteins_search_masked_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgSearchParams), C.POINTER(KgSeedParams), C.POINTER(KgAlignParams), vp, vp,
                                       C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.POINTER(KgMaskParams), C.c_int,
                                       C.POINTER(vp)]
    for name in ("kg_proteins_search_filtered", "kg_proteins_search_filtered_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgSearchParams), C.POINTER(KgSeedParams), C.POINTER(KgAlignParams), vp, vp,
                                       C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.POINTER(KgMaskParams), C.c_int,
                                       C.POINTER(KgUngappedParams), C.POINTER(vp)]
    lib.kg_hitset_ungapped_stats.argtypes = [vp, C.POINTER(KgUngappedStats)]
    for name in ("kg_proteins_align_banded", "kg_proteins_align_banded_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgAlignParams), vp, vp, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int, vp, vp,
                                       C.POINTER(vp), C.POINTER(KgBandParams), vp]
    for name in ("kg_proteins_search_banded", "kg_proteins_search_banded_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgSearchParams), C.POINTER(KgSeedParams), C.POINTER(KgAlignParams), vp, vp,
                                       C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.POINTER(KgMaskParams), C.c_int,
                                       C.POINTER(KgUngappedParams), C.POINTER(KgBandParams), C.POINTER(vp)]
    lib.kg_hitset_band_stats.argtypes = [vp, C.POINTER(KgBandStats)]
    for name in ("kg_searchdb_build", "kg_searchdb_build_device"):
        getattr(lib, name).argtypes = [C.c_int, vp, vp, C.c_int64, C.POINTER(KgSeedParams), C.POINTER(KgMaskParams), vp, C.c_int64,
                                       C.c_int64, C.c_int64, C.POINTER(vp)]
    lib.kg_searchdb_save.argtypes = [vp, C.c_char_p]
    lib.kg_searchdb_open.argtypes = [C.c_int, C.c_char_p, C.c_int64, C.POINTER(vp)]
    lib.kg_searchdb_info.argtypes = [vp, C.POINTER(KgSearchDbDesc)]
    lib.kg_searchdb_names_copy.argtypes = [vp, vp]
    lib.kg_searchdb_live_device_bytes.argtypes = [vp]
    lib.kg_searchdb_live_device_bytes.restype = C.c_int64
    lib.kg_searchdb_reserve.argtypes = [vp, C.c_int64]
    lib.kg_searchdb_free.argtypes = [vp]
    lib.kg_searchdb_free.restype = None
    for name in ("kg_searchdb_search", "kg_searchdb_search_device"):
        getattr(lib, name).argtypes = [vp, C.POINTER(KgSearchParams), C.POINTER(KgAlignParams), vp, vp, C.c_int64, C.c_int64, C.c_int64,
                                       C.c_int, C.c_int64, C.POINTER(KgMaskParams), C.POINTER(KgUngappedParams), C.POINTER(KgBandParams),
                                       C.POINTER(vp)]
    lib.kg_hitset_db_stats.argtypes = [vp, C.POINTER(KgSearchDbStats)]
    lib.kg_contigs_search_translated.argtypes = [vp, C.POINTER(KgSearchParams), C.POINTER(KgAlignParams), C.POINTER(KgTranslateParams), vp,
                                                  C.c_int, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.POINTER(KgMaskParams),
                                                  C.POINTER(KgUngappedParams), C.POINTER(KgBandParams), vp, C.POINTER(vp)]
    for name in ("kg_evidence_fragments", "kg_evidence_hits", "kg_evidence_calls_device", "kg_residual_searched_fragments"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = vp
    lib.kg_evidence_stats.argtypes = [vp, C.POINTER(KgTranslateStats)]
    translated = list(lib.kg_contigs_search_translated.argtypes)
    lib.kg_contigs_search_residual.argtypes = translated[:-1] + [vp, C.c_int, C.c_int64, C.POINTER(KgResidualParams), C.POINTER(vp)]
    lib.kg_result_search_residual.argtypes = [vp] + translated[:-1] + [C.POINTER(KgResidualParams), C.POINTER(vp)]
    lib.kg_residual_stats_of.argtypes = [vp, C.POINTER(KgResidualStats)]
    for name in ("kg_proteins_cluster_masked", "kg_proteins_cluster_masked_device"):
        getattr(lib, name).argtypes = [C.c_int, C.POINTER(KgClusterParams), C.POINTER(KgAlignParams), vp, vp, C.c_int64, C.c_int64,
                                       C.POINTER(KgMaskParams), C.POINTER(vp)]
    # the sets' accessors, by signature: (set) -> count, (set) -> device address, (set, first, count, dst), (set, dst), (set)
    for name in ("kg_sigset_count", "kg_familyset_count", "kg_familyset_edges_count", "kg_maskset_count", "kg_hitset_count", "kg_hitset_ops_count", "kg_opset_ops_count", "kg_regionset_count", "kg_orfset_count", "kg_orfset_junctions_count",
                 "kg_selectset_count", "kg_voteset_count", "kg_voteset_bins", "kg_compset_rows", "kg_compset_models",
                 "kg_evidence_calls_count"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = C.c_int64
    for name in ("kg_sigset_device", "kg_regionset_device", "kg_orfset_device", "kg_selectset_device"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = vp
    for name in ("kg_sigset_copy", "kg_familyset_copy", "kg_familyset_edges_copy", "kg_maskset_copy", "kg_maskset_flags_copy", "kg_hitset_copy", "kg_hitset_paths_copy", "kg_hitset_ungapped_copy", "kg_hitset_op_starts_copy", "kg_hitset_ops_copy", "kg_opset_op_starts_copy", "kg_opset_ops_copy", "kg_regionset_copy", "kg_orfset_copy", "kg_orfset_residues",
                 "kg_orfset_junctions_copy", "kg_orfset_coding_scores", "kg_orfset_start_shifts", "kg_selectset_copy",
                 "kg_voteset_copy_votes", "kg_voteset_copy_classes", "kg_voteset_copy_bins", "kg_compset_copy_classes",
                 "kg_compset_copy_counts", "kg_compset_model_labels", "kg_compset_copy_scores", "kg_evidence_calls_copy",
                 "kg_evidence_call_hits_copy", "kg_residual_searched_copy", "kg_residual_explain_copy", "kg_residual_call_kinds_copy",
                 "kg_residual_call_sources_copy"):
        getattr(lib, name).argtypes = [vp, C.c_int64, C.c_int64, vp]
    for name in ("kg_regionset_seq_start", "kg_orfset_prot_start", "kg_orfset_junctions_start", "kg_voteset_seq_start",
                 "kg_compset_background", "kg_hitset_starts_copy", "kg_maskset_starts_copy"):
        getattr(lib, name).argtypes = [vp, vp]
    for name in ("kg_sigset_free", "kg_familyset_free", "kg_maskset_free", "kg_hitset_free", "kg_opset_free", "kg_regionset_free", "kg_orfset_free", "kg_selectset_free",
                 "kg_voteset_free", "kg_compset_free", "kg_evidence_free"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = None
    lib.kg_last_error.restype = C.c_char_p
    lib.kg_version.restype = C.c_char_p
    for name in EXPORTS:
        getattr(lib, name)          # AttributeError if a declared symbol is not exported
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != KG_OK:
        raise KmerGutsNativeError(rc, load().kg_last_error().decode("utf-8", "replace"))


def view(ptr: int, count: int, dtype: np.dtype, owner=None) -> np.ndarray:
    """`count` records at `ptr` (library-owned pinned host memory) as a numpy array.  With `owner` the array is a
    zero-copy read-only view that keeps `owner` (the ScanResult) alive; without, a private copy."""
    if count == 0:
        return np.zeros(0, dtype=dtype)
    if not ptr:
        raise KmerGutsNativeError(-1, load().kg_last_error().decode("utf-8", "replace"))
    buf = (C.c_uint8 * (count * dtype.itemsize)).from_address(ptr)
    arr = np.frombuffer(buf, dtype=dtype, count=count)
    if owner is None:
        return arr.copy()
    buf._owner = owner                      # the ctypes buffer is the array's base: keeps the result alive
    arr.flags.writeable = False
    return arr
