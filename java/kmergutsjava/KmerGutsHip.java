package kmergutsjava;

import com.sun.jna.Library;
import com.sun.jna.Native;
import com.sun.jna.Pointer;
import com.sun.jna.Structure;
import com.sun.jna.ptr.IntByReference;
import com.sun.jna.ptr.FloatByReference;
import com.sun.jna.ptr.PointerByReference;

/**
 * JNA binding of libkmerguts_hip.so (C ABI: include/kmerguts_hip.h), the MI355X implementation of the
 * kmer_guts hot path.  jna-3.4.0.jar is already on the reference's classpath (build.xml:27), so a
 * maintainer adds this one file and the call site shown in INTEGRATION.md.
 *
 * Written against the JNA level the reference ships, 3.4.0: a Structure's field order is given with
 * setFieldOrder(String[]) in its constructor (the abstract getFieldOrder() only exists from JNA 3.5.0 on),
 * Native.loadLibrary(String, Class) loads the library.
 *
 * NOT COMPILED IN THIS REPOSITORY'S BUILD IMAGE (no JDK there); it is kept mechanical on purpose:
 * one Java method per exported C function, structures field for field -- tests/test_java_binding.py parses this
 * file and checks method names, arities and structure fields against include/kmerguts_hip.h.
 */
public interface KmerGutsHip extends Library {
    KmerGutsHip LIB = (KmerGutsHip) Native.loadLibrary("kmerguts_hip", KmerGutsHip.class);

    int KG_OK = 0;
    int KG_ERR_ARG = -1, KG_ERR_IO = -2, KG_ERR_FORMAT = -3, KG_ERR_DEVICE = -4, KG_ERR_NOMEM = -5, KG_ERR_UNSUPPORTED = -6,
        KG_ERR_LIMIT = -7, KG_ERR_BUSY = -8;
    int KG_F_COUNTERS = 1;
    int KG_F_SKIP_AGGREGATE = 2;
    int KG_F_PROGRESS = 4;

    /** struct kg_params: the instance fields the hot path reads (KmerGutsJava.java:102-106). */
    class KgParams extends Structure {
        public int aa, order_constraint, min_hits, min_weighted_hits, max_gap, flags;
        public KgParams() {
            setFieldOrder(new String[] {"aa", "order_constraint", "min_hits", "min_weighted_hits", "max_gap", "flags"});
        }
    }

    /** struct kg_stats */
    class KgStats extends Structure {
        public long n_seqs, n_containers, n_blocks, n_hits, n_calls, residues, windows, windows_valid,
                slots_inspected, table_bytes;
        public float ms_scan, ms_order, ms_aggregate, ms_total;
        public int scan_launches, partitioned;
        public float ms_part_scatter, ms_part_tag, ms_part_verify;
        public int fallback, part_chunks, part_buckets, part_shift, lookup_ran_off, agg_pieces, part_levels;
        public KgStats() {
            setFieldOrder(new String[] {"n_seqs", "n_containers", "n_blocks", "n_hits", "n_calls", "residues", "windows",
                    "windows_valid", "slots_inspected", "table_bytes", "ms_scan", "ms_order", "ms_aggregate",
                    "ms_total", "scan_launches", "partitioned", "ms_part_scatter", "ms_part_tag", "ms_part_verify", "fallback",
                    "part_chunks", "part_buckets", "part_shift", "lookup_ran_off", "agg_pieces", "part_levels"});
        }
    }

    /** struct kg_progress (KG_F_PROGRESS scans): what lookup's table stream reports and where it fails (KmerGutsJava.java:1016-1049). */
    class KgProgress extends Structure {
        public long[] first_visited = new long[11];
        public long last_visited, first_beyond, walk_ran_off, stream_slots;
        public long[] found_upto = new long[11];
        public long kmers_found;
        public KgProgress() {
            setFieldOrder(new String[] {"first_visited", "last_visited", "first_beyond", "walk_ran_off", "stream_slots", "found_upto",
                    "kmers_found"});
        }
    }

    /** struct kg_derive_params (kg_signatures_derive*). */
    class KgDeriveParams extends Structure {
        public int min_proteins, purity_pct;
        public long max_windows_per_pass;
        public KgDeriveParams() {
            setFieldOrder(new String[] {"min_proteins", "purity_pct", "max_windows_per_pass"});
        }
    }

    /** struct kg_derive_stats */
    class KgDeriveStats extends Structure {
        public long proteins, windows, valid_windows, pairs, kmers, signatures;
        public int passes;
        public float ms_encode, ms_sort, ms_reduce, ms_total;
        public KgDeriveStats() {
            setFieldOrder(new String[] {"proteins", "windows", "valid_windows", "pairs", "kmers", "signatures", "passes", "ms_encode",
                    "ms_sort", "ms_reduce", "ms_total"});
        }
    }

    /** struct kg_assign_params (kg_result_assign / kg_assign_calls); this project's defaults: 0 and 50. */
    class KgAssignParams extends Structure {
        public int min_score, min_share_pct;
        public KgAssignParams() {
            setFieldOrder(new String[] {"min_score", "min_share_pct"});
        }
    }

    /** struct kg_assignment (40 B): one function per protein of an -a scan. */
    class KgAssignment extends Structure {
        public int fI, assigned, score, total;
        public float weighted;
        public int n_calls, n_functions, second_fi, second_score, otu;
        public KgAssignment() {
            setFieldOrder(new String[] {"fI", "assigned", "score", "total", "weighted", "n_calls", "n_functions", "second_fi",
                    "second_score", "otu"});
        }
    }

    /** struct kg_region_params (kg_result_regions / kg_regions_calls); this project's defaults: 600, 0 and 0. */
    class KgRegionParams extends Structure {
        public int merge_gap, min_score, min_len;
        public KgRegionParams() {
            setFieldOrder(new String[] {"merge_gap", "min_score", "min_len"});
        }
    }

    /** struct kg_region (48 B): one function region of a contig, 0-based inclusive left / right. */
    class KgRegion extends Structure {
        public int seq, strand, left, right, fI, score;
        public float weighted;
        public int n_calls, frames, best_frame, first_call, kept;
        public KgRegion() {
            setFieldOrder(new String[] {"seq", "strand", "left", "right", "fI", "score", "weighted", "n_calls", "frames",
                    "best_frame", "first_call", "kept"});
        }
    }

    /** struct kg_region_stats. */
    class KgRegionStats extends Structure {
        public long calls, groups, regions, kept, multi_frame;
        public float ms;
        public int reserved;
        public KgRegionStats() {
            setFieldOrder(new String[] {"calls", "groups", "regions", "kept", "multi_frame", "ms", "reserved"});
        }
    }

    /** struct kg_orf_params (kg_regionset_orfs / kg_orfs_regions); this project's defaults: 7 (ATG, GTG, TTG), 1 and 0. */
    class KgOrfParams extends Structure {
        public int start_codons, only_kept, reserved;
        public KgOrfParams() {
            setFieldOrder(new String[] {"start_codons", "only_kept", "reserved"});
        }
    }

    /** struct kg_orf (48 B): the open reading frame around one function region, 0-based inclusive left / right. */
    class KgOrf extends Structure {
        public int seq, strand, frame, left, right, n_res, start_codon, first_inner, flags, fI, score, kept;
        public KgOrf() {
            setFieldOrder(new String[] {"seq", "strand", "frame", "left", "right", "n_res", "start_codon", "first_inner", "flags",
                    "fI", "score", "kept"});
        }
    }

    /** struct kg_orf_stats. */
    class KgOrfStats extends Structure {
        public long orfs, complete, interrupted, partial5, residues, tiles;
        public float ms;
        public int reserved;
        public KgOrfStats() {
            setFieldOrder(new String[] {"orfs", "complete", "interrupted", "partial5", "residues", "tiles", "ms", "reserved"});
        }
    }

    /** struct kg_free_params (kg_orfs_free / kg_orfset_add_free); this project's defaults: 100, 7 (ATG, GTG, TTG) and 0. */
    class KgFreeParams extends Structure {
        public int min_res, start_codons, reserved;
        public KgFreeParams() {
            setFieldOrder(new String[] {"min_res", "start_codons", "reserved"});
        }
    }

    /** struct kg_coding_params (kg_orfset_coding); this project's defaults: 0, 0 and 100000. */
    class KgCodingParams extends Structure {
        public int min_coding, reserved;
        public long min_train_pairs;
        public KgCodingParams() {
            setFieldOrder(new String[] {"min_coding", "reserved", "min_train_pairs"});
        }
    }

    /** struct kg_coding_model: the coding and the background count of every hexamer index (first base most significant). */
    class KgCodingModel extends Structure {
        public long[] coding = new long[4096];
        public long[] background = new long[4096];
        public KgCodingModel() {
            setFieldOrder(new String[] {"coding", "background"});
        }
    }

    /** struct kg_coding_stats; trained: 0 untrained, 1 on its own set, 2 the caller's table. */
    class KgCodingStats extends Structure {
        public long scored, training_records, training_pairs, background, noncoding;
        public int trained;
        public float ms_count, ms_score;
        public int reserved;
        public KgCodingStats() {
            setFieldOrder(new String[] {"scored", "training_records", "training_pairs", "background", "noncoding", "trained",
                    "ms_count", "ms_score", "reserved"});
        }
    }

    /** struct kg_repair_params (kg_regionset_repair / kg_result_repair); this project's defaults: 7, 0, 4 and 0. */
    class KgRepairParams extends Structure {
        public int start_codons, min_count, max_junctions, reserved;
        public KgRepairParams() {
            setFieldOrder(new String[] {"start_codons", "min_count", "max_junctions", "reserved"});
        }
    }

    /** struct kg_repair_stats */
    class KgRepairStats extends Structure {
        public long candidates, repaired, failed, single, skipped, junctions, residues;
        public float ms;
        public int reserved;
        public KgRepairStats() {
            setFieldOrder(new String[] {"candidates", "repaired", "failed", "single", "skipped", "junctions", "residues", "ms",
                    "reserved"});
        }
    }

    /** struct kg_start_params (kg_orfset_starts / kg_starts_orfs); this project's defaults: 100, 7, 4, 0 and 200. */
    class KgStartParams extends Structure {
        public int min_res, start_codons, rounds, reserved;
        public long min_train_starts;
        public KgStartParams() {
            setFieldOrder(new String[] {"min_res", "start_codons", "rounds", "reserved", "min_train_starts"});
        }
    }

    /** struct kg_start_model: int64 chosen[20][4], cand[20][4] (JNA has no nested arrays: entry 4 * position + base) and the
     *  types' type_chosen[4], type_cand[4] (0 unused, 1 ATG, 2 GTG, 3 TTG). */
    class KgStartModel extends Structure {
        public long[] chosen = new long[80];
        public long[] cand = new long[80];
        public long[] type_chosen = new long[4];
        public long[] type_cand = new long[4];
        public KgStartModel() {
            setFieldOrder(new String[] {"chosen", "cand", "type_chosen", "type_cand"});
        }
    }

    /** struct kg_start_weights: int32 pos[20][4] (entry 4 * position + base) and type[4]. */
    class KgStartWeights extends Structure {
        public int[] pos = new int[80];
        public int[] type = new int[4];
        public KgStartWeights() {
            setFieldOrder(new String[] {"pos", "type"});
        }
    }

    /** struct kg_start_stats; trained: 0 untrained, 1 on its own set, 2 the caller's weights. */
    class KgStartStats extends Structure {
        public long movable, training_records, candidates, moved;
        public int rounds_run, trained;
        public float ms_count, ms_choose;
        public KgStartStats() {
            setFieldOrder(new String[] {"movable", "training_records", "candidates", "moved", "rounds_run", "trained", "ms_count",
                    "ms_choose"});
        }
    }

    /** struct kg_select_params (kg_regionset_select / kg_orfset_select / kg_select_intervals); this project's defaults: 60, 50 and 0. */
    class KgSelectParams extends Structure {
        public int max_overlap, max_overlap_pct, reserved;
        public KgSelectParams() {
            setFieldOrder(new String[] {"max_overlap", "max_overlap_pct", "reserved"});
        }
    }

    /** struct kg_vote_params (kg_result_otu_votes / kg_otu_votes_hits); the defaults are 10, 50 and 1. */
    class KgVoteParams extends Structure {
        public int min_votes, min_share_pct, min_calls, reserved;
        public KgVoteParams() {
            setFieldOrder(new String[] {"min_votes", "min_share_pct", "min_calls", "reserved"});
        }
    }

    /** struct kg_vote_stats. */
    class KgVoteStats extends Structure {
        public long hits, accepted, votes, pairs, seqs_with_votes, assigned, bins, assigned_length, total_length;
        public float ms;
        public int reserved;
        public KgVoteStats() {
            setFieldOrder(new String[] {"hits", "accepted", "votes", "pairs", "seqs_with_votes", "assigned", "bins", "assigned_length",
                                        "total_length", "ms", "reserved"});
        }
    }

    /** struct kg_comp_params (kg_contigs_compose); the defaults are 1500, 2560 and 200000. */
    class KgCompParams extends Structure {
        public int min_len, min_margin;
        public long min_train;
        public int keep_scores, reserved;
        public KgCompParams() {
            setFieldOrder(new String[] {"min_len", "min_margin", "min_train", "keep_scores", "reserved"});
        }
    }

    /** struct kg_comp_stats. */
    class KgCompStats extends Structure {
        public long seqs, labelled, label_rows, models, windows, decided, decided_unlabelled, conflicts;
        public float ms_count, ms_score;
        public KgCompStats() {
            setFieldOrder(new String[] {"seqs", "labelled", "label_rows", "models", "windows", "decided", "decided_unlabelled",
                                        "conflicts", "ms_count", "ms_score"});
        }
    }

    /** struct kg_interval (20 B): one candidate of kg_select_intervals, 0-based inclusive left / right. */
    class KgInterval extends Structure {
        public int seq, left, right, score, eligible;
        public KgInterval() {
            setFieldOrder(new String[] {"seq", "left", "right", "score", "eligible"});
        }
    }

    /** struct kg_selection (8 B): state 0 not eligible, 1 selected, 2 overlapped; by = the winner's index in the set or -1. */
    class KgSelection extends Structure {
        public int state, by;
        public KgSelection() {
            setFieldOrder(new String[] {"state", "by"});
        }
    }

    /** struct kg_select_stats. */
    class KgSelectStats extends Structure {
        public long candidates, eligible, selected, overlapped, pairs, conflicts;
        public int rounds;
        public float ms;
        public KgSelectStats() {
            setFieldOrder(new String[] {"candidates", "eligible", "selected", "overlapped", "pairs", "conflicts", "rounds", "ms"});
        }
    }

    /** struct kg_cluster_params (kg_proteins_cluster*); this project's defaults: 5, 20 and 0. */
    class KgClusterParams extends Structure {
        public int min_shared, min_cover_pct, reserved;
        public KgClusterParams() {
            setFieldOrder(new String[] {"min_shared", "min_cover_pct", "reserved"});
        }
    }

    /** struct kg_family (16 B): the family's dense number and root, the centre of the protein's strongest edge or -1, its shared k-mers. */
    class KgFamily extends Structure {
        public int family, root, best, shared;
        public KgFamily() {
            setFieldOrder(new String[] {"family", "root", "best", "shared"});
        }
    }

    /** struct kg_cluster_stats. */
    class KgClusterStats extends Structure {
        public long proteins, valid_windows, pairs, kmers, links, edges, families, families_multi, largest;
        public int rounds;
        public float ms_encode, ms_sort, ms_link, ms_components, ms_total;
        public KgClusterStats() {
            setFieldOrder(new String[] {"proteins", "valid_windows", "pairs", "kmers", "links", "edges", "families", "families_multi",
                    "largest", "rounds", "ms_encode", "ms_sort", "ms_link", "ms_components", "ms_total"});
        }
    }

    /** struct kg_align_params (kg_proteins_align*, kg_proteins_cluster_aligned*); this project's defaults: 50, KG_ALIGN_REF_LONGER (0;
     *  KG_ALIGN_REF_MEMBER is 1), 11, 1, 2^26 cells, matrix null (the built-in BLOSUM62; else 441 bytes, 21 x 21 in code order), 0. */
    class KgAlignParams extends Structure {
        public int min_ratio_pct, ref, gap_open, gap_extend;
        public long max_cells;
        public Pointer matrix;
        public long reserved;
        public KgAlignParams() {
            setFieldOrder(new String[] {"min_ratio_pct", "ref", "gap_open", "gap_extend", "max_cells", "matrix", "reserved"});
        }
    }

    /** struct kg_alignment (24 B): the local alignment score (-1: skipped), the two self-scores, the 0-based end cell or (-1, -1),
     *  status 0 aligned / 1 skipped. */
    class KgAlignment extends Structure {
        public int score, self_a, self_b, end_a, end_b, status;
        public KgAlignment() {
            setFieldOrder(new String[] {"score", "self_a", "self_b", "end_a", "end_b", "status"});
        }
    }

    /** struct kg_family_edge (32 B): one link that passed the 8-mer tests; status 0 kept, 1 cut, 2 skipped. */
    class KgFamilyEdge extends Structure {
        public int member, centre, shared, score, ref, end_member, end_centre, status;
        public KgFamilyEdge() {
            setFieldOrder(new String[] {"member", "centre", "shared", "score", "ref", "end_member", "end_centre", "status"});
        }
    }

    /** struct kg_align_stats. */
    class KgAlignStats extends Structure {
        public long aligned, cut, skipped, cells;
        public float ms_align;
        public int reserved;
        public KgAlignStats() {
            setFieldOrder(new String[] {"aligned", "cut", "skipped", "cells", "ms_align", "reserved"});
        }
    }

    /** struct kg_alignment_path (32 B): where a traced alignment starts (0-based, -1 without a path) and what its columns are; status
     *  0 traced, 1 none, 2 untraced (the prefix box has more than max_trace_cells cells; KG_TRACE_DEFAULT_MAX_CELLS is 2^24). */
    class KgAlignmentPath extends Structure {
        public int start_a, start_b, identical, positive, gap_opens, gap_cols_a, gap_cols_b, status;
        public KgAlignmentPath() {
            setFieldOrder(new String[] {"start_a", "start_b", "identical", "positive", "gap_opens", "gap_cols_a", "gap_cols_b", "status"});
        }
    }

    /** struct kg_trace_stats (kg_hitset_trace_stats). */
    class KgTraceStats extends Structure {
        public long traced, untraced, cells;
        public float ms_trace;
        public int reserved;
        public KgTraceStats() {
            setFieldOrder(new String[] {"traced", "untraced", "cells", "ms_trace", "reserved"});
        }
    }

    /** struct kg_search_params (kg_proteins_search*); this project's defaults: 2, 8 (at most 64), 256 and 0. */
    class KgSearchParams extends Structure {
        public int min_shared, max_cand, max_db_per_kmer, reserved;
        public KgSearchParams() {
            setFieldOrder(new String[] {"min_shared", "max_cand", "max_db_per_kmer", "reserved"});
        }
    }

    /** struct kg_seed_params (48 B, kg_proteins_search_seeded*): cls = the class of each residue in code order ACDEFGHIKLMNPQRSTVWY
     *  (values below alphabet_size, every class used), shape = up to four masks of equal weight, bit j = position j is a care
     *  position, bit 0 set, entries from n_shapes on zero; reserved 0.  kg_seed_params_builtin fills one. */
    class KgSeedParams extends Structure {
        public int n_shapes, alphabet_size;
        public byte[] cls = new byte[20];
        public int[] shape = new int[4];
        public int reserved;
        public KgSeedParams() {
            setFieldOrder(new String[] {"n_shapes", "alphabet_size", "cls", "shape", "reserved"});
        }
    }

    /** struct kg_search_hit (40 B): one aligned or skipped candidate of a query; status 0 hit, 1 below, 2 skipped; rank from 0. */
    class KgSearchHit extends Structure {
        public int query, target, shared, score, self_query, self_target, end_query, end_target, status, rank;
        public KgSearchHit() {
            setFieldOrder(new String[] {"query", "target", "shared", "score", "self_query", "self_target", "end_query", "end_target",
                    "status", "rank"});
        }
    }

    /** struct kg_search_stats. */
    class KgSearchStats extends Structure {
        public long targets, queries, valid_windows, pairs, kmers, kmers_joined, kmers_masked, join_pairs, candidates, aligned, hits,
                skipped, queries_hit, cells;
        public float ms_encode, ms_sort, ms_join, ms_align, ms_total;
        public int reserved;
        public KgSearchStats() {
            setFieldOrder(new String[] {"targets", "queries", "valid_windows", "pairs", "kmers", "kmers_joined", "kmers_masked",
                    "join_pairs", "candidates", "aligned", "hits", "skipped", "queries_hit", "cells", "ms_encode", "ms_sort", "ms_join",
                    "ms_align", "ms_total", "reserved"});
        }
    }

    /** struct kg_mask_params (kg_proteins_mask*, kg_proteins_search_masked*, kg_proteins_cluster_masked*): 4 <= window <= 32,
     *  0 <= trigger <= extend < Lg(window) in units of 1/256 bit; the defaults are 12, 563, 640; reserved 0. */
    class KgMaskParams extends Structure {
        public int window, trigger, extend, reserved;
        public KgMaskParams() {
            setFieldOrder(new String[] {"window", "trigger", "extend", "reserved"});
        }
    }

    /** struct kg_mask_stats. */
    class KgMaskStats extends Structure {
        public long proteins, residues, windows, low_windows, ext_windows, masking_windows, segments, masked_residues, proteins_masked;
        public float ms_mask;
        public int reserved;
        public KgMaskStats() {
            setFieldOrder(new String[] {"proteins", "residues", "windows", "low_windows", "ext_windows", "masking_windows", "segments",
                    "masked_residues", "proteins_masked", "ms_mask", "reserved"});
        }
    }

    /** struct kg_ungapped_params (kg_proteins_search_filtered*): a candidate whose best seed diagonal scores below min_ungapped
     *  without gaps is not aligned; min_ungapped >= 0, default 0 (rank only); reserved 0. */
    class KgUngappedParams extends Structure {
        public int min_ungapped;
        public int[] reserved = new int[3];
        public KgUngappedParams() {
            setFieldOrder(new String[] {"min_ungapped", "reserved"});
        }
    }

    /** struct kg_search_ungapped (16 B): one per hit record of a filtered search, same index. */
    class KgSearchUngapped extends Structure {
        public int ungapped, diagonal, on_diagonal, reserved;
        public KgSearchUngapped() {
            setFieldOrder(new String[] {"ungapped", "diagonal", "on_diagonal", "reserved"});
        }
    }

    /** struct kg_ungapped_stats. */
    class KgUngappedStats extends Structure {
        public long scored, dropped, cut, cells;
        public float ms_ungapped;
        public int reserved;
        public KgUngappedStats() {
            setFieldOrder(new String[] {"scored", "dropped", "cut", "cells", "ms_ungapped", "reserved"});
        }
    }

    /** struct kg_band_params (kg_proteins_align_banded*, kg_proteins_search_banded*): only the cells (i, j) with
     *  |(i - j) - diagonal| <= band are filled; 0 <= band <= KG_BAND_MAX = 256; no default; reserved 0. */
    class KgBandParams extends Structure {
        public int band;
        public int[] reserved = new int[3];
        public KgBandParams() {
            setFieldOrder(new String[] {"band", "reserved"});
        }
    }

    /** struct kg_searchdb_desc (240 B, kg_searchdb_info): a resident protein database's counts, parameters, device bytes and
     *  build times; seeds, mask and mask_stats are nested by value. */
    class KgSearchDbDesc extends Structure {
        public long targets, residues, pairs, kmers, valid_windows, names_bytes, query_room, device_bytes;
        public int has_seeds, has_mask;
        public KgSeedParams seeds;
        public KgMaskParams mask;
        public KgMaskStats mask_stats;
        public float ms_upload, ms_encode, ms_sort, ms_index, ms_total;
        public int reserved;
        public KgSearchDbDesc() {
            setFieldOrder(new String[] {"targets", "residues", "pairs", "kmers", "valid_windows", "names_bytes", "query_room",
                    "device_bytes", "has_seeds", "has_mask", "seeds", "mask", "mask_stats", "ms_upload", "ms_encode", "ms_sort",
                    "ms_index", "ms_total", "reserved"});
        }
    }

    /** struct kg_search_db_stats (24 B, kg_hitset_db_stats): the probe's counts and times of a search against a kg_searchdb. */
    class KgSearchDbStats extends Structure {
        public long query_kmers, found;
        public float ms_probe, ms_upload;
        public KgSearchDbStats() {
            setFieldOrder(new String[] {"query_kmers", "found", "ms_probe", "ms_upload"});
        }
    }

    /** struct kg_translate_params (16 B, kg_contigs_search_translated): fragments of at least min_res residues (default 30), the
     *  hits of rank below max_hits become CALLs (1..64, default 1); reserved 0. */
    class KgTranslateParams extends Structure {
        public int min_res, max_hits;
        public int[] reserved = new int[2];
        public KgTranslateParams() {
            setFieldOrder(new String[] {"min_res", "max_hits", "reserved"});
        }
    }

    /** struct kg_residual_params (16 B, kg_contigs_search_residual): a fragment is explained when the counts of the signature
     *  CALLs that touch it sum to explain_min or more (default 1); homology CALLs below min_db_count are left out (default 0). */
    class KgResidualParams extends Structure {
        public long explain_min;
        public int min_db_count, reserved;
        public KgResidualParams() {
            setFieldOrder(new String[] {"explain_min", "min_db_count", "reserved"});
        }
    }

    /** struct kg_residual_stats (80 B, kg_residual_stats_of): the counts of the new stages and their device times. */
    class KgResidualStats extends Structure {
        public long sig_calls, explained, explained_residues, searched, searched_residues, db_calls, dropped_min_count, merged;
        public float ms_explain, ms_compact, ms_merge, ms_total;
        public KgResidualStats() {
            setFieldOrder(new String[] {"sig_calls", "explained", "explained_residues", "searched", "searched_residues", "db_calls",
                    "dropped_min_count", "merged", "ms_explain", "ms_compact", "ms_merge", "ms_total"});
        }
    }

    /** struct kg_translate_stats (72 B, kg_evidence_stats): the counts of a translated search and its device times by stage. */
    class KgTranslateStats extends Structure {
        public long fragments, fragment_residues, records, calls, dropped_status, dropped_rank, dropped_untraced;
        public float ms_fragments, ms_search, ms_calls, ms_total;
        public KgTranslateStats() {
            setFieldOrder(new String[] {"fragments", "fragment_residues", "records", "calls", "dropped_status", "dropped_rank",
                    "dropped_untraced", "ms_fragments", "ms_search", "ms_calls", "ms_total"});
        }
    }

    /** struct kg_band_stats: band cells against full cells over the aligned pairs of a banded search. */
    class KgBandStats extends Structure {
        public long band_cells, full_cells;
        public int band, reserved;
        public KgBandStats() {
            setFieldOrder(new String[] {"band_cells", "full_cells", "band", "reserved"});
        }
    }

    /** struct kg_merge_params (kg_table_merge_signatures*): on_conflict = KG_MERGE_KEEP (0), KG_MERGE_REPLACE (1) or KG_MERGE_DROP (2). */
    class KgMergeParams extends Structure {
        public int on_conflict, reserved;
        public KgMergeParams() {
            setFieldOrder(new String[] {"on_conflict", "reserved"});
        }
    }

    /** struct kg_merge_stats. */
    class KgMergeStats extends Structure {
        public long base, base_ignored, added_in, added, conflicts, conflicts_same_function, replaced, dropped, merged;
        public float ms_extract, ms_sort, ms_resolve, ms_total;
        public KgMergeStats() {
            setFieldOrder(new String[] {"base", "base_ignored", "added_in", "added", "conflicts", "conflicts_same_function", "replaced",
                    "dropped", "merged", "ms_extract", "ms_sort", "ms_resolve", "ms_total"});
        }
    }

    // replaces readKmerTableHeader + the table stream of lookup (KmerGutsJava.java:924-942, 944-1034)
    int kg_table_open(String path, int device, PointerByReference out);
    int kg_table_from_memory(Pointer image, long nbytes, int device, PointerByReference out);
    int kg_table_from_device(Pointer dEntries, long numSigs, int device, PointerByReference out);
    /** sigs: n packed 24-byte kg_signature records (long kmer, int otu_index, avg_from_end, function_index, float function_wt). */
    int kg_table_build(Pointer sigs, long n, long numSigs, int device, long[] nPlaced, PointerByReference out);
    int kg_table_build_device(Pointer dSigs, long n, long numSigs, int device, long[] nPlaced, PointerByReference out);
    int kg_table_save(Pointer table, String path);
    /** annotated proteins -> signature set: fn[p] = -1 for an unannotated protein, otu[p] >= 0 where fn[p] >= 0. */
    int kg_signatures_derive(int device, KgDeriveParams params, byte[] seq, long[] offsets, long nProt, int[] fn, int[] otu,
                             PointerByReference out);
    int kg_signatures_derive_device(int device, KgDeriveParams params, Pointer dSeq, long[] offsets, long nProt, int[] fn, int[] otu,
                                    PointerByReference out);
    long kg_sigset_count(Pointer set);
    Pointer kg_sigset_device(Pointer set);                   // kg_signature[count] in device memory: kg_table_build_device takes it
    int kg_sigset_copy(Pointer set, long first, long count, Pointer dst);
    int kg_sigset_stats(Pointer set, KgDeriveStats out);
    void kg_sigset_free(Pointer set);
    /** a resident table united with n new signatures (fnMap / otuMap: null keeps the field) -> a signature set in k-mer order; n = 0
     *  exports the table */
    int kg_table_merge_signatures(Pointer base, KgMergeParams params, Pointer sigs, long n, int[] fnMap, long nFn, int[] otuMap, long nOtu,
                                  PointerByReference out);
    int kg_table_merge_signatures_device(Pointer base, KgMergeParams params, Pointer dSigs, long n, int[] fnMap, long nFn, int[] otuMap,
                                         long nOtu, PointerByReference out);
    int kg_sigset_merge_stats(Pointer set, KgMergeStats out);
    /** proteins -> families by shared 8-mers (connected components): maxWindows = 0 sizes the one pass from free device memory */
    int kg_proteins_cluster(int device, KgClusterParams params, byte[] seq, long[] offsets, long nProt, long maxWindows,
                            PointerByReference out);
    int kg_proteins_cluster_device(int device, KgClusterParams params, Pointer dSeq, long[] offsets, long nProt, long maxWindows,
                                   PointerByReference out);
    long kg_familyset_count(Pointer set);
    int kg_familyset_copy(Pointer set, long first, long count, Pointer dst);   // kg_family[count], 16 B each, protein order
    int kg_familyset_stats(Pointer set, KgClusterStats out);
    void kg_familyset_free(Pointer set);
    /** local alignment scores of protein pairs: pairs = int[2 * nPairs] of (a, b) indices, out = kg_alignment[nPairs], 24 B each */
    int kg_proteins_align(int device, KgAlignParams params, byte[] seq, long[] offsets, long nProt, int[] pairs, long nPairs, Pointer out);
    int kg_proteins_align_device(int device, KgAlignParams params, Pointer dSeq, long[] offsets, long nProt, int[] pairs, long nPairs,
                                 Pointer out);
    /** kg_proteins_align with the traceback pass behind it: paths = kg_alignment_path[nPairs], 32 B each, beside out */
    int kg_proteins_align_paths(int device, KgAlignParams params, byte[] seq, long[] offsets, long nProt, int[] pairs, long nPairs,
                                long maxTraceCells, Pointer out, Pointer paths);
    int kg_proteins_align_paths_device(int device, KgAlignParams params, Pointer dSeq, long[] offsets, long nProt, int[] pairs, long nPairs,
                                       long maxTraceCells, Pointer out, Pointer paths);
    /** kg_proteins_align_paths with the alignments themselves: opsMode = KG_TRACE_OPS (4: M, I, D) or KG_TRACE_OPS_EQX (8: = and X for
     *  M); ops receives a kg_opset: opStart[nPairs + 1] and the ops, each len << 4 | code with BAM's codes (M 0, I 1, D 2, = 7, X 8),
     *  in alignment order; free it with kg_opset_free */
    int kg_proteins_align_ops(int device, KgAlignParams params, byte[] seq, long[] offsets, long nProt, int[] pairs, long nPairs,
                              long maxTraceCells, int opsMode, Pointer out, Pointer paths, PointerByReference ops);
    int kg_proteins_align_ops_device(int device, KgAlignParams params, Pointer dSeq, long[] offsets, long nProt, int[] pairs, long nPairs,
                                     long maxTraceCells, int opsMode, Pointer out, Pointer paths, PointerByReference ops);
    /** kg_proteins_align_ops in a band around one diagonal per pair; paths and ops may both be null (the records alone, opsMode 0) */
    int kg_proteins_align_banded(int device, KgAlignParams params, byte[] seq, long[] offsets, long nProt, int[] pairs, long nPairs,
                                 long maxTraceCells, int opsMode, Pointer out, Pointer paths, PointerByReference ops, KgBandParams band,
                                 int[] diagonals);
    int kg_proteins_align_banded_device(int device, KgAlignParams params, Pointer dSeq, long[] offsets, long nProt, int[] pairs, long nPairs,
                                        long maxTraceCells, int opsMode, Pointer out, Pointer paths, PointerByReference ops,
                                        KgBandParams band, int[] diagonals);
    long kg_opset_ops_count(Pointer set);
    int kg_opset_op_starts_copy(Pointer set, long first, long count, Pointer dst);   // long[count + 1]: opStart[first .. first + count]
    int kg_opset_ops_copy(Pointer set, long firstOp, long count, Pointer dst);       // int[count]
    int kg_opset_ms_ops(Pointer set, FloatByReference out);                          // the ops' own device time (prefix sum and fill), ms
    void kg_opset_free(Pointer set);
    /** kg_proteins_cluster with every link that passed the 8-mer tests verified by alignment; align = null: kg_proteins_cluster */
    int kg_proteins_cluster_aligned(int device, KgClusterParams params, KgAlignParams align, byte[] seq, long[] offsets, long nProt,
                                    long maxWindows, PointerByReference out);
    int kg_proteins_cluster_aligned_device(int device, KgClusterParams params, KgAlignParams align, Pointer dSeq, long[] offsets, long nProt,
                                           long maxWindows, PointerByReference out);
    long kg_familyset_edges_count(Pointer set);
    int kg_familyset_edges_copy(Pointer set, long first, long count, Pointer dst);   // kg_family_edge[count], 32 B each, (member, centre) order
    int kg_familyset_align_stats(Pointer set, KgAlignStats out);
    /** proteins [nDb, nProt) searched against proteins [0, nDb): shared 8-mers, the best maxCand targets per query aligned; align must
     *  not be null; maxWindows = 0 and maxPairs = 0 size the one pass and the join from free device memory */
    int kg_proteins_search(int device, KgSearchParams params, KgAlignParams align, byte[] seq, long[] offsets, long nProt, long nDb,
                           long maxWindows, long maxPairs, PointerByReference out);
    int kg_proteins_search_device(int device, KgSearchParams params, KgAlignParams align, Pointer dSeq, long[] offsets, long nProt, long nDb,
                                  long maxWindows, long maxPairs, PointerByReference out);
    long kg_hitset_count(Pointer set);
    int kg_hitset_copy(Pointer set, long first, long count, Pointer dst);   // kg_search_hit[count], 40 B each, (query, rank) order
    int kg_hitset_starts_copy(Pointer set, long[] dst);                     // hit_start[nQ + 1]
    int kg_hitset_stats(Pointer set, KgSearchStats out);
    void kg_hitset_free(Pointer set);
    /** kg_proteins_search with the traceback pass behind it: trace = KG_TRACE_HITS (1: the hit records) or KG_TRACE_ALL (2: every
     *  aligned record with a score) */
    int kg_proteins_search_paths(int device, KgSearchParams params, KgAlignParams align, byte[] seq, long[] offsets, long nProt, long nDb,
                                 long maxWindows, long maxPairs, int trace, long maxTraceCells, PointerByReference out);
    int kg_proteins_search_paths_device(int device, KgSearchParams params, KgAlignParams align, Pointer dSeq, long[] offsets, long nProt,
                                        long nDb, long maxWindows, long maxPairs, int trace, long maxTraceCells, PointerByReference out);
    int kg_hitset_paths_copy(Pointer set, long first, long count, Pointer dst);   // kg_alignment_path[count], 32 B each, same indices
    int kg_hitset_trace_stats(Pointer set, KgTraceStats out);
    /** the ops of the traced records, for a set made with trace | KG_TRACE_OPS (4) or trace | KG_TRACE_OPS_EQX (8) in
     *  kg_proteins_search_paths* or kg_proteins_search_seeded*; one opStart entry per hit record, plus one */
    long kg_hitset_ops_count(Pointer set);
    int kg_hitset_op_starts_copy(Pointer set, long first, long count, Pointer dst);  // long[count + 1]
    int kg_hitset_ops_copy(Pointer set, long firstOp, long count, Pointer dst);      // int[count], len << 4 | code
    int kg_hitset_ms_ops(Pointer set, FloatByReference out);
    /** a built-in seed set into out: which = KG_SEEDS_EXACT (0: the identity map and the shape 0xFF) or KG_SEEDS_REDUCED (1) */
    int kg_seed_params_builtin(int which, KgSeedParams out);
    /** kg_proteins_search with reduced-alphabet spaced seeds in the 8-mers' place; trace = 0 (no paths; maxTraceCells is ignored),
     *  KG_TRACE_HITS or KG_TRACE_ALL; the set is read with the kg_hitset getters */
    int kg_proteins_search_seeded(int device, KgSearchParams params, KgSeedParams seeds, KgAlignParams align, byte[] seq, long[] offsets,
                                  long nProt, long nDb, long maxWindows, long maxPairs, int trace, long maxTraceCells, PointerByReference out);
    int kg_proteins_search_seeded_device(int device, KgSearchParams params, KgSeedParams seeds, KgAlignParams align, Pointer dSeq,
                                         long[] offsets, long nProt, long nDb, long maxWindows, long maxPairs, int trace, long maxTraceCells,
                                         PointerByReference out);
    /** proteins -> their low-complexity segments (SEG's trigger window and extension; the header states the rule).  The set holds
     *  kg_mask_segment[count] (16 B each: protein, start, end inclusive, reserved), segStart[nProt + 1] and one 0/1 byte per residue */
    int kg_proteins_mask(int device, KgMaskParams params, byte[] seq, long[] offsets, long nProt, PointerByReference out);
    int kg_proteins_mask_device(int device, KgMaskParams params, Pointer dSeq, long[] offsets, long nProt, PointerByReference out);
    long kg_maskset_count(Pointer set);
    int kg_maskset_copy(Pointer set, long first, long count, Pointer dst);         // kg_mask_segment[count]
    int kg_maskset_starts_copy(Pointer set, long[] dst);                           // segStart[nProt + 1]
    int kg_maskset_flags_copy(Pointer set, long first, long count, Pointer dst);   // byte[count], residue 0 = offsets[0]
    int kg_maskset_stats(Pointer set, KgMaskStats out);
    void kg_maskset_free(Pointer set);
    /** kg_proteins_search_seeded (seeds = null: the exact 8-mers) with the seeding pass on a soft-masked copy of the sequence:
     *  sides = KG_MASK_QUERIES (1), KG_MASK_TARGETS (2) or both (3); the alignment reads the original */
    int kg_proteins_search_masked(int device, KgSearchParams params, KgSeedParams seeds, KgAlignParams align, byte[] seq, long[] offsets,
                                  long nProt, long nDb, long maxWindows, long maxPairs, int trace, long maxTraceCells, KgMaskParams mask,
                                  int sides, PointerByReference out);
    int kg_proteins_search_masked_device(int device, KgSearchParams params, KgSeedParams seeds, KgAlignParams align, Pointer dSeq,
                                         long[] offsets, long nProt, long nDb, long maxWindows, long maxPairs, int trace, long maxTraceCells,
                                         KgMaskParams mask, int sides, PointerByReference out);
    int kg_hitset_mask_stats(Pointer set, KgMaskStats out);
    /** kg_proteins_search_masked (seeds and mask nullable) with the ungapped stage between the join and the alignment: each
     *  candidate's best seed diagonal is scored without gaps, and the per-query cut is by (larger score, larger s, smaller target) */
    int kg_proteins_search_filtered(int device, KgSearchParams params, KgSeedParams seeds, KgAlignParams align, byte[] seq, long[] offsets,
                                    long nProt, long nDb, long maxWindows, long maxPairs, int trace, long maxTraceCells, KgMaskParams mask,
                                    int sides, KgUngappedParams ungapped, PointerByReference out);
    int kg_proteins_search_filtered_device(int device, KgSearchParams params, KgSeedParams seeds, KgAlignParams align, Pointer dSeq,
                                           long[] offsets, long nProt, long nDb, long maxWindows, long maxPairs, int trace,
                                           long maxTraceCells, KgMaskParams mask, int sides, KgUngappedParams ungapped,
                                           PointerByReference out);
    int kg_hitset_ungapped_copy(Pointer set, long first, long count, Pointer dst);   // kg_search_ungapped[count]
    int kg_hitset_ungapped_stats(Pointer set, KgUngappedStats out);
    /** kg_proteins_search_filtered with every candidate aligned, and traced, in the band around its best seed diagonal */
    int kg_proteins_search_banded(int device, KgSearchParams params, KgSeedParams seeds, KgAlignParams align, byte[] seq, long[] offsets,
                                  long nProt, long nDb, long maxWindows, long maxPairs, int trace, long maxTraceCells, KgMaskParams mask,
                                  int sides, KgUngappedParams ungapped, KgBandParams band, PointerByReference out);
    int kg_proteins_search_banded_device(int device, KgSearchParams params, KgSeedParams seeds, KgAlignParams align, Pointer dSeq,
                                         long[] offsets, long nProt, long nDb, long maxWindows, long maxPairs, int trace,
                                         long maxTraceCells, KgMaskParams mask, int sides, KgUngappedParams ungapped, KgBandParams band,
                                         PointerByReference out);
    int kg_hitset_band_stats(Pointer set, KgBandStats out);
    /** a resident protein database: built once from the targets (seeds, mask: null for the exact 8-mers / no mask; names: an
     *  opaque blob), saved, opened, and searched with batches of queries; the records are the one-batch search's, byte for byte */
    int kg_searchdb_build(int device, byte[] seq, long[] offsets, long nDb, KgSeedParams seeds, KgMaskParams mask, byte[] names,
                          long namesBytes, long maxWindows, long queryRoom, PointerByReference out);
    int kg_searchdb_build_device(int device, Pointer dSeq, long[] offsets, long nDb, KgSeedParams seeds, KgMaskParams mask, byte[] names,
                                 long namesBytes, long maxWindows, long queryRoom, PointerByReference out);
    int kg_searchdb_save(Pointer db, String path);
    int kg_searchdb_open(int device, String path, long queryRoom, PointerByReference out);
    int kg_searchdb_info(Pointer db, KgSearchDbDesc out);
    int kg_searchdb_names_copy(Pointer db, byte[] dst);
    long kg_searchdb_live_device_bytes(Pointer db);
    int kg_searchdb_reserve(Pointer db, long queryRoom);
    void kg_searchdb_free(Pointer db);
    int kg_searchdb_search(Pointer db, KgSearchParams params, KgAlignParams align, byte[] seq, long[] offsets, long nQ, long maxWindows,
                           long maxPairs, int trace, long maxTraceCells, KgMaskParams queryMask, KgUngappedParams ungapped,
                           KgBandParams band, PointerByReference out);
    int kg_searchdb_search_device(Pointer db, KgSearchParams params, KgAlignParams align, Pointer dSeq, long[] offsets, long nQ,
                                  long maxWindows, long maxPairs, int trace, long maxTraceCells, KgMaskParams queryMask,
                                  KgUngappedParams ungapped, KgBandParams band, PointerByReference out);
    int kg_hitset_db_stats(Pointer set, KgSearchDbStats out);
    /** genes by homology: the stop-to-stop fragments of a batch of contigs searched against a kg_searchdb and the hits made
     *  into CALL records (targetFn: int[n_db] or null); the evidence lends its fragments (a kg_orfset) and hits (a kg_hitset) */
    int kg_contigs_search_translated(Pointer db, KgSearchParams params, KgAlignParams align, KgTranslateParams translate, Pointer seq,
                                     int seqOnDevice, long[] offsets, long nSeqs, long maxWindows, long maxPairs, int trace,
                                     long maxTraceCells, KgMaskParams queryMask, KgUngappedParams ungapped, KgBandParams band,
                                     int[] targetFn, PointerByReference out);
    Pointer kg_evidence_fragments(Pointer evidence);
    Pointer kg_evidence_hits(Pointer evidence);
    long kg_evidence_calls_count(Pointer evidence);
    int kg_evidence_calls_copy(Pointer evidence, long first, long count, Pointer dst);
    Pointer kg_evidence_calls_device(Pointer evidence);
    int kg_evidence_call_hits_copy(Pointer evidence, long first, long count, long[] dst);
    int kg_evidence_stats(Pointer evidence, KgTranslateStats out);
    void kg_evidence_free(Pointer evidence);
    /** signature and homology evidence in one run: the fragments the signature CALLs (sigCalls: host or device kg_call records in
     *  container order) do not explain are searched, and the two kinds of CALL are merged by container; targetFn is required */
    int kg_contigs_search_residual(Pointer db, KgSearchParams params, KgAlignParams align, KgTranslateParams translate, Pointer seq,
                                   int seqOnDevice, long[] offsets, long nSeqs, long maxWindows, long maxPairs, int trace,
                                   long maxTraceCells, KgMaskParams queryMask, KgUngappedParams ungapped, KgBandParams band,
                                   int[] targetFn, Pointer sigCalls, int callsOnDevice, long nSigCalls, KgResidualParams residual,
                                   PointerByReference out);
    /** the same with the CALLs of a DNA scan's result, read where they lie on the device */
    int kg_result_search_residual(Pointer result, Pointer db, KgSearchParams params, KgAlignParams align, KgTranslateParams translate,
                                  Pointer seq, int seqOnDevice, long[] offsets, long nSeqs, long maxWindows, long maxPairs, int trace,
                                  long maxTraceCells, KgMaskParams queryMask, KgUngappedParams ungapped, KgBandParams band,
                                  int[] targetFn, KgResidualParams residual, PointerByReference out);
    Pointer kg_residual_searched_fragments(Pointer evidence);
    int kg_residual_searched_copy(Pointer evidence, long first, long count, long[] dst);
    int kg_residual_explain_copy(Pointer evidence, long first, long count, long[] dst);
    int kg_residual_call_kinds_copy(Pointer evidence, long first, long count, byte[] dst);
    int kg_residual_call_sources_copy(Pointer evidence, long first, long count, long[] dst);
    int kg_residual_stats_of(Pointer evidence, KgResidualStats out);
    /** kg_proteins_cluster_aligned (align = null: no alignment step) with every protein soft-masked for the 8-mer pass */
    int kg_proteins_cluster_masked(int device, KgClusterParams params, KgAlignParams align, byte[] seq, long[] offsets, long nProt,
                                   long maxWindows, KgMaskParams mask, PointerByReference out);
    int kg_proteins_cluster_masked_device(int device, KgClusterParams params, KgAlignParams align, Pointer dSeq, long[] offsets, long nProt,
                                          long maxWindows, KgMaskParams mask, PointerByReference out);
    int kg_familyset_mask_stats(Pointer set, KgMaskStats out);
    Pointer kg_table_device_entries(Pointer table);
    long kg_table_records(Pointer table);
    int kg_table_info(Pointer table, long[] numSigs, long[] entrySize, long[] version, long[] occupied);
    long kg_table_live_device_bytes(Pointer table);
    void kg_table_close(Pointer table);

    // replaces prepareQuery/addKmers, the query sort, lookup and gatherHits/processSetOfHits
    // (KmerGutsJava.java:1051-1074, 900-922, 1076-1095, 944-1034, 385-514) for a batch of sequences
    int kg_scan(Pointer table, KgParams params, byte[] seq, long[] offsets, long nSeqs, PointerByReference out);
    int kg_scan_device(Pointer table, KgParams params, Pointer dSeq, long[] offsets, long nSeqs, PointerByReference out);

    int kg_aggregate_hits(int device, KgParams params, Pointer hits, Pointer containerHitStart, long nSeqs, Pointer otuInit,
                          PointerByReference out);
    int kg_process_set_of_hits(int device, KgParams params, Pointer hits, int nHits, int currentFI, Pointer otu, Pointer call,
                               IntByReference called, IntByReference newCurrentFI, IntByReference keepsLastTwo);
    int kg_result_stats(Pointer result, KgStats out);
    Pointer kg_result_hits(Pointer result);                  // kg_hit[n_hits]   24 B each
    Pointer kg_result_container_hit_start(Pointer result);   // int64[n_containers + 1]
    Pointer kg_result_calls(Pointer result);                 // kg_call[n_calls] 24 B each
    Pointer kg_result_container_call_start(Pointer result);  // int64[n_containers + 1]
    Pointer kg_result_otu(Pointer result);                   // kg_otu[n_seqs]   44 B each
    Pointer kg_result_hit_events(Pointer result);            // byte[n_hits]        KG_EV_* (for the -d stream)
    Pointer kg_result_container_tail_events(Pointer result); // byte[n_containers]  KG_EV_TAIL_CALL
    Pointer kg_result_device_hits(Pointer result);
    Pointer kg_result_device_calls(Pointer result);
    int kg_result_copy_hits(Pointer result, long first, long count, Pointer dst);
    Pointer kg_result_hit_slots(Pointer result);             // uint32[n_hits]      KG_F_PROGRESS scans
    int kg_result_progress(Pointer result, KgProgress out);
    Pointer kg_result_device_otu(Pointer result);
    Pointer kg_result_device_container_hit_start(Pointer result);
    Pointer kg_result_device_container_call_start(Pointer result);
    /** one function per protein: dst = kg_assignment[n_seqs] (40 B each; host or device memory), ms = float[1] or null */
    int kg_result_assign(Pointer result, KgAssignParams params, Pointer dst, float[] ms);
    int kg_assign_calls(int device, KgAssignParams params, Pointer calls, long[] callStart, long nProt, Pointer otu, Pointer dst);
    /** the CALLs of a DNA result -> function regions on the contigs; offsets = the long[nSeqs + 1] the scan was given */
    int kg_result_regions(Pointer result, KgRegionParams params, long[] offsets, PointerByReference out);
    int kg_regions_calls(int device, KgRegionParams params, Pointer calls, long nCalls, long[] offsets, long nSeqs,
                         PointerByReference out);
    long kg_regionset_count(Pointer set);
    Pointer kg_regionset_device(Pointer set);                // kg_region[count] in device memory, output order
    int kg_regionset_copy(Pointer set, long first, long count, Pointer dst);
    int kg_regionset_seq_start(Pointer set, long[] dst);     // long[nSeqs + 1]
    int kg_regionset_stats(Pointer set, KgRegionStats out);
    void kg_regionset_free(Pointer set);
    /** function regions -> the open reading frame around each and its protein; seq = the bytes the scan was given */
    int kg_regionset_orfs(Pointer set, KgOrfParams params, Pointer seq, int seqOnDevice, long[] offsets, long nSeqs,
                          PointerByReference out);
    int kg_orfs_regions(int device, KgOrfParams params, Pointer regions, long nRegions, Pointer seq, long[] offsets, long nSeqs,
                        PointerByReference out);
    long kg_orfset_count(Pointer set);
    Pointer kg_orfset_device(Pointer set);                   // kg_orf[count] in device memory, index-aligned with the regions
    int kg_orfset_copy(Pointer set, long first, long count, Pointer dst);
    int kg_orfset_prot_start(Pointer set, long[] dst);       // long[count + 1]
    int kg_orfset_residues(Pointer set, long first, long count, Pointer dst);
    int kg_orfset_stats(Pointer set, KgOrfStats out);
    void kg_orfset_free(Pointer set);
    /** the evidence-free open reading frames of a batch (flag 16 = KG_ORF_FREE): alone, or behind the records of an ORF set */
    int kg_orfs_free(int device, KgFreeParams params, Pointer seq, int seqOnDevice, long[] offsets, long nSeqs,
                     PointerByReference out);
    int kg_orfset_add_free(Pointer set, KgFreeParams params, Pointer seq, int seqOnDevice, long[] offsets, long nSeqs,
                           PointerByReference out);
    /** the hexamer log-odds score of every ORF of a set; a free ORF below min_coding loses kept and gains flag 32 =
     *  KG_ORF_NONCODING.  table: int[4096] or null to train on the set.  Free the new set before the given one. */
    int kg_orfset_coding(Pointer set, KgCodingParams params, int[] table, Pointer seq, int seqOnDevice, long[] offsets, long nSeqs,
                         PointerByReference out);
    int kg_orfset_coding_scores(Pointer set, long first, long count, Pointer dst);   // long[count]
    int kg_orfset_coding_stats(Pointer set, KgCodingStats out);
    int kg_orfset_coding_model(Pointer set, KgCodingModel out);
    int kg_coding_table(KgCodingModel model, int[] table);   // host only: int[4096]
    int kg_coding_counts_orfs(int device, Pointer orfs, long n, Pointer seq, long[] offsets, long nSeqs, KgCodingModel out);
    int kg_coding_score_orfs(int device, int[] table, Pointer orfs, long n, Pointer seq, long[] offsets, long nSeqs, long[] scores);
    /** the start codon of every movable ORF of a set, chosen by the start-site score; a moved ORF gains flag 64 =
     *  KG_ORF_START_MOVED.  table: int[4096]; weights: null to train on the set; regions: null or the region set the ORFs
     *  came from.  Free the new set before the given one. */
    int kg_orfset_starts(Pointer set, KgStartParams params, int[] table, KgStartWeights weights, Pointer regions, Pointer seq,
                         int seqOnDevice, long[] offsets, long nSeqs, PointerByReference out);
    int kg_orfset_start_shifts(Pointer set, long first, long count, Pointer dst);    // int[count]
    int kg_orfset_start_stats(Pointer set, KgStartStats out);
    int kg_orfset_start_model(Pointer set, KgStartModel out);
    int kg_start_weights_from(KgStartModel model, KgStartWeights weights);           // host only
    /** limits: int[n] (-1: none) or null; out: n packed 48-byte kg_orf records; model, stats: may be null */
    int kg_starts_orfs(int device, KgStartParams params, int[] table, KgStartWeights weights, Pointer orfs, long n, int[] limits,
                       Pointer seq, long[] offsets, long nSeqs, Pointer out, int[] shifts, KgStartModel model, KgStartStats stats);
    /** Frameshift repair (run before kg_orfset_add_free): a NEW ORF set in which the record and protein of every multi-frame
     *  region are the chain through its frames (flag KG_ORF_REPAIRED = 128), and the junction list.  calls: the region set's
     *  packed 24-byte kg_call records, in device memory when callsOnDevice != 0.  Free the new set before the given ones. */
    int kg_regionset_repair(Pointer set, Pointer orfs, Pointer calls, int callsOnDevice, long nCalls, KgRepairParams params, Pointer seq,
                            int seqOnDevice, long[] offsets, long nSeqs, PointerByReference out);
    int kg_result_repair(Pointer result, Pointer set, Pointer orfs, KgRepairParams params, Pointer seq, int seqOnDevice, long[] offsets,
                         long nSeqs, PointerByReference out);
    long kg_orfset_junctions_count(Pointer set);
    /** dst: count packed 24-byte kg_junction records (int orf, pos, from_frame, to_frame, res, gap) */
    int kg_orfset_junctions_copy(Pointer set, long first, long count, Pointer dst);
    int kg_orfset_junctions_start(Pointer set, long[] dst);                          // long[n_orfs + 1]
    int kg_orfset_junctions_stats(Pointer set, KgRepairStats out);
    /** the non-overlapping selection among the kept regions / ORFs of a set; free the select set before the set it came from */
    int kg_regionset_select(Pointer set, KgSelectParams params, PointerByReference out);
    int kg_orfset_select(Pointer set, KgSelectParams params, PointerByReference out);
    /** iv: n packed 20-byte kg_interval records (int seq, left, right, score, eligible) in host memory, any order */
    int kg_select_intervals(int device, KgSelectParams params, Pointer iv, long n, long nSeqs, PointerByReference out);
    long kg_selectset_count(Pointer set);
    Pointer kg_selectset_device(Pointer set);                // kg_selection[count] in device memory, index-aligned with the candidates
    int kg_selectset_copy(Pointer set, long first, long count, Pointer dst);
    int kg_selectset_stats(Pointer set, KgSelectStats out);
    void kg_selectset_free(Pointer set);
    /** every OTU vote per sequence, one OTU per sequence, the batch's bins; offsets = the long[nSeqs + 1] the scan was given.
     *  Free the vote set before the result's table. */
    int kg_result_otu_votes(Pointer result, KgVoteParams params, long[] offsets, PointerByReference out);
    /** caller-held host lists: packed 24-byte kg_hit and kg_call records, one event byte per hit, per = 6 (DNA) or 1 (-a) */
    int kg_otu_votes_hits(int device, KgVoteParams params, Pointer hits, long[] containerHitStart, Pointer hitEvents, Pointer calls,
                          long[] containerCallStart, long nSeqs, int per, long[] offsets, PointerByReference out);
    long kg_voteset_count(Pointer set);                      // (sequence, OTU) pairs
    long kg_voteset_bins(Pointer set);
    /** dst: count packed 16-byte kg_otu_vote records (int seq, oI, votes, n_calls) */
    int kg_voteset_copy_votes(Pointer set, long first, long count, Pointer dst);
    /** dst: count packed 40-byte kg_otu_class records, one per sequence */
    int kg_voteset_copy_classes(Pointer set, long first, long count, Pointer dst);
    /** dst: count packed 32-byte kg_otu_bin records (int oI, n_seqs; long length, votes, n_calls) */
    int kg_voteset_copy_bins(Pointer set, long first, long count, Pointer dst);
    int kg_voteset_seq_start(Pointer set, long[] dst);       // long[nSeqs + 1]
    int kg_voteset_stats(Pointer set, KgVoteStats out);
    void kg_voteset_free(Pointer set);
    /** bins by tetranucleotide composition: labels = int[nSeqs] (>= 0 a training contig's bin, -1 unlabelled) or null; a caller's
     *  model = modelLabels int[nModels] and modelCounts long[(nModels + 1) * 256], the background row last, or both null */
    int kg_contigs_compose(int device, KgCompParams params, Pointer seq, int seqOnDevice, long[] offsets, long nSeqs, int[] labels,
                           int[] modelLabels, long[] modelCounts, long nModels, PointerByReference out);
    long kg_compset_rows(Pointer set);                       // label rows the call made
    long kg_compset_models(Pointer set);                     // models the scores are under (the background comes behind them)
    /** dst: count packed 40-byte kg_comp_class records (int label, best, second, decided; long windows, score_best, score_second) */
    int kg_compset_copy_classes(Pointer set, long first, long count, Pointer dst);
    /** dst: count * 256 ints, the tetramer counts of contigs first .. */
    int kg_compset_copy_counts(Pointer set, long first, long count, Pointer dst);
    /** labelsDst: count ints; countsDst: count * 256 longs (either may be null) */
    int kg_compset_copy_rows(Pointer set, long first, long count, Pointer labelsDst, Pointer countsDst);
    int kg_compset_background(Pointer set, long[] dst);      // long[256]
    int kg_compset_model_labels(Pointer set, long first, long count, Pointer dst);
    /** dst: count * (models + 1) longs; only when keep_scores was set */
    int kg_compset_copy_scores(Pointer set, long first, long count, Pointer dst);
    int kg_compset_stats(Pointer set, KgCompStats out);
    void kg_compset_free(Pointer set);
    void kg_result_free(Pointer result);
    int kg_restore_hits_device(int device, Pointer dSrc, long nHits, Pointer dSeqFirst, long nSeqs, Pointer dDstFirst,
                               Pointer dContainerShift, Pointer dDst, Pointer stream);

    String kg_last_error();
    String kg_version();
}
