/*
 * kmerguts_hip.h -- C ABI of libkmerguts_hip.so, the MI355X (gfx950) implementation of the
 * kmer_guts hot path of rsutormin/KmerGutsJava.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own (it is one Java class);
 * every entry point below names the reference interface it replaces.  "KGJ:n" =
 * lib/src/kmergutsjava/KmerGutsJava.java line n of the reference.  The Java (JNA) and Python
 * (ctypes) bindings that call these are shown in INTEGRATION.md.  Beyond the reference, the library also makes the
 * tables it reads: kg_table_build* places a signature list the way the lookup finds it, kg_table_save writes a resident
 * table back to kmer.table.mem_map[.gz], and kg_signatures_derive* makes that list from annotated proteins.
 * kg_table_merge_signatures* unites a resident table with new signatures (and exports a table's own).
 * kg_result_assign / kg_assign_calls turn the CALL records of an -a scan into one function per protein.
 * kg_result_regions / kg_regions_calls merge the CALL records of a DNA scan into function regions in contig coordinates.
 * kg_regionset_orfs / kg_orfs_regions extend every region to its open reading frame and extract the translated protein.
 * kg_orfs_free / kg_orfset_add_free enumerate the evidence-free open reading frames of the six frames.
 * kg_orfset_coding scores every ORF by its in-frame hexamers against the genome's background and drops the non-coding free ones.
 *
 * Conventions: plain pointers and sizes only; every function returns an int status
 * (KG_OK == 0, negative == error) and never throws or aborts across the boundary; the text
 * of the last error on the calling thread is kg_last_error().  All memory returned by the
 * library is owned by the library and released by kg_result_free / kg_table_close.
 * A kg_table is read-only after creation and may be shared by host threads; at most one
 * kg_scan* may be in flight per kg_table at a time (the reference's instance is not
 * re-entrant either, KGJ:838): a second concurrent kg_scan* on the same table returns
 * KG_ERR_BUSY without touching anything.
 *
 * Environment variables read by kg_scan* (tuning and test hooks, none needed in production; every
 * one is read at the start of each call, so a test can change them between calls):
 *   KG_PARTITION (0 direct / 1 partitioned whenever possible / 2 auto), KG_BIDX (0: probe the tags, not the byte home index),
 *   KG_PART_SHIFT, KG_PART_CHUNKS, KG_PART_MIN_CHUNK_BLOCKS, KG_PART_WGS, KG_PART_SLACK, KG_PART_OVF_GROUPS, KG_PART_TAPER,
 *   KG_PROBE_GRID, KG_INDEX_GRID, KG_INDEX_R, KG_PROBE_GRAB, KG_VERIFY_GRID, KG_LOWC_GRID, KG_OVF_GRID,
 *   KG_ORDER_GRID, KG_ORDER_STREAMS, KG_EARLY_TOTALS, KG_PLACE_STAGED, KG_SCAN_GRID, KG_SCAN_RPG, KG_DIRECT_FILTER, KG_SCATTER_PRIO, KG_SCATTER_FLUSH_LIST, KG_INDEX_PRIO, KG_VERIFY_PRIO, KG_STAGE_CHUNK, KG_AGG_PIECES, KG_AGG_PAIRS, KG_AGG_BLOCK_SHIFT:
 *   geometry of the
 *   scan strategies (kg_host_plan.hpp: plan_partition, plan_direct, plan_aggregate); results never depend on them.  KG_DEBUG: one stderr line per attempt.
 *   TEST HOOKS (used by tests/ only; inert unless the process set KG_ENABLE_TEST_HOOKS=1 before its FIRST kg_scan* -- that
 *   one is read once, so a stray KG_TEST_* variable in a server's environment does nothing): KG_TEST_TINY_LISTS=1 starts the hit / candidate lists at one chunk, so that the
 *   resize-and-rerun path runs; KG_TEST_FAIL_ALLOC=n makes the n-th device allocation of the call fail with
 *   KG_ERR_NOMEM, so that the error paths can be checked for leaks (kg_table_live_device_bytes).
 */
#ifndef KMERGUTS_HIP_H
#define KMERGUTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KG_OK               0
#define KG_ERR_ARG         (-1)   /* bad argument                                                  */
#define KG_ERR_IO          (-2)   /* file could not be read                                        */
#define KG_ERR_FORMAT      (-3)   /* table image malformed (short header, entrySize != 24, ...)    */
#define KG_ERR_DEVICE      (-4)   /* HIP runtime error / no gfx950 device                          */
#define KG_ERR_NOMEM       (-5)
#define KG_ERR_UNSUPPORTED (-6)   /* parameters on which the reference itself throws (minHits < 2) */
#define KG_ERR_LIMIT       (-7)   /* one call exceeds 2^32-1 windows or 2^31-1 window blocks       */
#define KG_ERR_BUSY        (-8)   /* another kg_scan* is in flight on the same kg_table            */

/* KGJ:85-99 */
#define KG_K                8
#define KG_MAX_ENCODED      25600000000LL   /* 20^8; a table slot is empty iff whichKmer > this (KGJ:1000) */
#define KG_MAX_HITS_PER_SEQ 40000
#define KG_OI_BUFSZ         5
#define KG_TABLE_ENTRY_SIZE 24              /* KGJ:995-999: i64 whichKmer, i32 otuIndex, i32 avgFromEnd, i32 functionIndex, f32 functionWt */

/* The instance fields the hot path reads (KGJ:102-106), set by the CLI flags -a -O -m -M -g (KGJ:577-595). */
typedef struct kg_params {
    int32_t aa;                 /* -a : input is protein (1 container per sequence) instead of DNA (6)  */
    int32_t order_constraint;   /* -O */
    int32_t min_hits;           /* -m, reference default 5; must be >= 2                                */
    int32_t min_weighted_hits;  /* -M, reference default 0                                              */
    int32_t max_gap;            /* -g, reference default 200                                            */
    uint32_t flags;             /* KG_F_*                                                               */
} kg_params;

#define KG_F_COUNTERS        1u  /* also count windows_valid / slots_inspected, slower     */
#define KG_F_SKIP_AGGREGATE  2u  /* stop after the hit records (no CALL / OTU stage)                   */
#define KG_F_PROGRESS        4u  /* also record what the reference's table stream would have reported  */
                                 /* (kg_result_progress, kg_result_hit_slots): the "Processed: NN%"    */
                                 /* lines of KGJ:1016-1025 and where a short table file fails,          */
                                 /* KGJ:985-988 / 1036-1049.  Tables of < 2^32 records.  On the          */
                                 /* partitioned strategy with the table's byte home index (part_levels  */
                                 /* 4) the index pass summarises the walks of the k-mers it rules out    */
                                 /* and the verify pass notes the rest; otherwise (direct strategy,      */
                                 /* KG_BIDX=0, with KG_F_COUNTERS) the walking kernels of KG_F_COUNTERS  */
                                 /* run and the stats' counters are filled too                           */

/* Event byte per hit record (kg_result_hit_events) and per container (kg_result_container_tail_events):
 * what gatherHits (KGJ:457-514) did at that record, so that a host can print the -d stream (HIT, after-hit,
 * after-call; KGJ:376-383, 406-409, 470-473, 498-501) by replaying the list contents without deciding anything.
 * Order of the steps at one record: [RESET_BEFORE] -> [ACCEPTED] -> [RESET_AFTER]. */
#define KG_EV_ACCEPTED      0x01u  /* the record was appended to the hits list (KGJ:496-497)                      */
#define KG_EV_RESET_BEFORE  0x02u  /* gap rule (KGJ:477-484): the list was processed or cleared before the record */
#define KG_EV_CALL_BEFORE   0x04u  /*   ... and that printed the container's next CALL                            */
#define KG_EV_KEEP2_BEFORE  0x08u  /*   ... and the list kept its last two members (KGJ:441-449), else it is empty */
#define KG_EV_RESET_AFTER   0x10u  /* pair rule (KGJ:503-508): processSetOfHits ran after the append step         */
#define KG_EV_CALL_AFTER    0x20u
#define KG_EV_KEEP2_AFTER   0x40u
#define KG_EV_TAIL_CALL     0x01u  /* container byte: the final flush (KGJ:511-513) printed a CALL                */

/* Binary records.  Text formatting (KGJ:398-404, 518-548) stays in host code. */
typedef struct kg_hit {          /* replaces class Hit (KGJ:1213-1219) + its HitContainer id (KGJ:1262-1266) */
    uint32_t container;          /* running container index: seq*6 + {+0,+1,+2,-0,-1,-2} (DNA) or seq (AA), KGJ:907-911 */
    int32_t  from0InProt;
    int32_t  oI;
    int32_t  avgOffFromEnd;
    int32_t  fI;
    float    functionWt;
} kg_hit;

typedef struct kg_call {         /* one "CALL" line, KGJ:398-404 */
    uint32_t container;
    int32_t  start;              /* hits.get(0).from0InProt                 */
    int32_t  end;                /* hits.get(lastHit).from0InProt + (K-1)   */
    int32_t  count;              /* fICount                                 */
    int32_t  fI;                 /* currentFI                               */
    float    weightedHits;       /* float32, summed in list order           */
} kg_call;

typedef struct kg_otu {          /* the per-sequence oICounts buffer as printed by KGJ:516-524 */
    int32_t n;
    int32_t count[KG_OI_BUFSZ];
    int32_t oI[KG_OI_BUFSZ];
} kg_otu;

typedef struct kg_stats {
    int64_t n_seqs, n_containers, n_blocks;   /* blocks = wavefront work items ("contig window blocks") */
    int64_t n_hits, n_calls;
    int64_t residues;            /* translated positions (DNA: sum over 6 frames) or characters (AA)     */
    int64_t windows;             /* 8-residue windows enumerated (KGJ:912 loop trips, all frames)        */
    int64_t windows_valid;       /* windows that encode (KGJ:913-915); valid only with KG_F_COUNTERS     */
    int64_t slots_inspected;     /* table entries inspected under KGJ:944-1034 semantics; KG_F_COUNTERS  */
    int64_t table_bytes;         /* numSigs * 24                                                          */
    float   ms_scan;             /* HIP-event time of the scan kernel (encode + probe + compaction)      */
    float   ms_order;            /* prefix sums + ordered placement of the hit records                   */
    float   ms_aggregate;        /* gatherHits / processSetOfHits kernels                                */
    float   ms_total;            /* first kernel start -> last kernel end on the library's stream        */
    int32_t scan_launches;       /* >1 when the hit staging buffer had to grow and the scan was re-run   */
    int32_t partitioned;         /* 1: the scan stage ran as scatter + tag + verify passes (kg_partition.hpp), */
                                 /* 0: as the single direct-probing kernel                                    */
    float   ms_part_scatter;     /* partitioned only: start of ms_scan until the last chunk is scattered        */
    float   ms_part_tag;         /* (unused: the tag passes overlap the scatter passes of later chunks)         */
    float   ms_part_verify;      /* partitioned only: what remains of the tag / verify passes after that        */
    int32_t fallback;            /* why a partitioned attempt was thrown away and the direct kernel ran instead:  */
                                 /* 0 none (partitioned ran, or direct was chosen up front), 1 more overflow      */
                                 /* groups than provisioned (heavily repeated k-mers), 2 the scatter pass's spin  */
                                 /* guard fired (protocol failure; never expected)                                */
    int32_t part_chunks;         /* partitioned only: chunks of whole sequences the batch was cut into            */
    int32_t part_buckets;        /* partitioned only: slot-range buckets (each 2^part_shift slots)                */
    int32_t part_shift;
    int32_t lookup_ran_off;      /* 1: some query walked to the end of the record stream undecided -- where the     */
                                 /* reference's table stream throws EOFException and its lookup ends with            */
                                 /* "Error: null" instead of "Kmers found: ..." (KGJ:799-802, 1031-1033, 1097-1126); */
                                 /* the records are the same either way (EOF == not found)                           */
    int32_t agg_pieces;          /* pieces beyond the first that long containers were cut into for gatherHits (cuts  */
                                 /* at gaps > maxGap, where the reference's list restarts anyway: KGJ:477-484)       */
    int32_t part_levels;         /* partitioned only: what the tag pass probed in the L2 -- 1 = the tags (bucket_tag_kernel: scans  */
                                 /* with KG_F_COUNTERS, KG_BIDX=0, tables without the index), 4 = the table's byte home index      */
                                 /* (bucket_index_kernel, the default; KG_F_PROGRESS scans too).  (2 and 3 were round 3's second    */
                                 /* partition level, removed in round 4.)                                                           */
} kg_stats;

/* KG_F_PROGRESS: the slots the reference's merge-join (KGJ:959-1029) visits = the slots some query's walk reads, summed up
 * the way its progress lines and its failure modes need them.  The join runs in slot order and prints
 *     "Processed: <10 f>%, time=<ms> ms., found-so-far=<k-mers found at slots <= s>"
 * at every visited slot s whose tenth f = (int)(10.0 * ((double)(s + 1) / (double)numSigs)) differs from the last one printed
 * (KGJ:1017-1024), i.e. once per tenth, at the first slot visited in it. */
typedef struct kg_progress {
    int64_t first_visited[11];   /* [f]: the first slot visited in tenth f, -1 when none (f = 10: the slot numSigs - 1 and, for   */
                                 /* a table file longer than numSigs records, everything behind it)                               */
    int64_t last_visited;        /* the last slot visited, -1 when none                                                           */
    int64_t first_beyond;        /* the smallest home slot of a query k-mer at or behind the END of the record stream (a table    */
                                 /* file shorter than numSigs records), -1 when none: the join has to skip to it and fails --     */
                                 /* "Error skipping <24 x (first_beyond - last_visited - 1)> bytes" on a .gz stream when the slot */
                                 /* lies BEHIND the end (first_beyond > stream_slots; KGJ:1036-1049), EOFException ("Error: null") */
                                 /* at the read that follows the skip on a plain file, or when the slot is the end itself         */
    int64_t walk_ran_off;        /* 1: a walk reached the end of the stream undecided: EOFException before any such skip          */
    int64_t stream_slots;        /* records in the table stream (numSigs for a complete file)                                     */
    int64_t found_upto[11];      /* [f]: distinct k-mers found at slots <= first_visited[f] = the line's found-so-far (0 when the */
                                 /* tenth was not visited)                                                                        */
    int64_t kmers_found;         /* distinct k-mers found by this scan = the reference's kmersFound (KGJ:1004-1006, 1031-1033)     */
} kg_progress;

typedef struct kg_table  kg_table;
typedef struct kg_result kg_result;

/* ---- signature table: replaces readKmerTableHeader (KGJ:924-942) + the table stream of lookup (KGJ:944-1034) ---- */

/* Read <path> = kmer.table.mem_map or kmer.table.mem_map.gz (KGJ:749-753; told apart by the gzip magic), validate the
 * header (3 x int64 LE: numSigs, entrySize, version) and make the table resident on HIP device <device>.  The file is
 * streamed through pinned buffers (several reader threads for a plain file, one zlib stream for .gz): no host copy. */
int kg_table_open(const char *path, int device, kg_table **out);
/* Same from a file image in host memory (the host gunzips kmer.table.mem_map.gz, KGJ:750-753). */
int kg_table_from_memory(const void *image, size_t nbytes, int device, kg_table **out);
/* Adopt num_sigs 24-byte entries that already sit in device memory (not copied, not freed; must stay
 * unchanged while the table lives).  Synchronises the device once before reading them. */
int kg_table_from_device(const void *d_entries, int64_t num_sigs, int device, kg_table **out);
/* ---- building a table: a signature list -> the records of kmer.table.mem_map, and a resident table -> a file ---- */
typedef struct kg_signature {    /* 24 B: the layout of one kmer.table.mem_map record (KGJ:995-999) */
    int64_t kmer;                /* encodedKmer (KGJ:274-292), 0 <= kmer < 20^8 */
    int32_t otu_index, avg_from_end, function_index;
    float   function_wt;
} kg_signature;
/* Place n signatures (any order) into a table of num_sigs slots the way the reference's lookup finds them (KGJ:944-1034):
 * home = kmer % num_sigs; in (home, kmer) order each signature takes slot pos = max(home, previous pos + 1); a signature
 * with pos >= num_sigs is dropped; every other slot holds the empty record (whichKmer = 20^8 + 1, all other bytes 0).
 * Header {num_sigs, 24, 1}.  The records equal kmergutsjava_amd.synth.build_table's byte for byte.  *n_placed = signatures
 * placed (= kg_table_info's occupied).  KG_ERR_ARG: a k-mer outside [0, 20^8) (the message names the smallest such input
 * index), a k-mer that occurs twice (the message names the smallest one), num_sigs <= 0; KG_ERR_LIMIT: n >= 2^32;
 * KG_ERR_NOMEM.  n = 0 gives an all-empty table.  kg_table_build reads a host array (pageable or pinned), uploaded through
 * pinned pieces; kg_table_build_device an 8-byte aligned device array, complete before the call (the device is synchronised
 * once).  Scratch (about 24 bytes per signature) is returned to the driver before the call returns.  KG_TEST_FAIL_ALLOC
 * applies to the build's device allocations. */
int kg_table_build(const kg_signature *sigs, int64_t n, int64_t num_sigs, int device, int64_t *n_placed, kg_table **out);
int kg_table_build_device(const kg_signature *d_sigs, int64_t n, int64_t num_sigs, int device, int64_t *n_placed, kg_table **out);
/* Write the table to <path>: the header, then every whole record that is resident -- a table opened from a plain file saves
 * to that file's bytes cut to whole records.  gzip when <path> ends in ".gz".  Written under a temporary name next to
 * <path> and renamed: a failed save (KG_ERR_IO) leaves no file under <path>.  KG_ERR_BUSY while a kg_scan* is in flight. */
int kg_table_save(kg_table *t, const char *path);
/* ---- deriving the signatures: annotated proteins -> the signature k-mers of a table (kernels: kg_derive.hpp) ----
 *
 * Input: n_prot proteins as raw characters seq plus offsets[n_prot + 1] (host, non-decreasing), the layout of kg_scan.  Each
 * protein p has a function index fn[p] and an OTU index otu[p] (host arrays).  fn[p] is -1 for an unannotated protein,
 * otherwise >= 0.  otu[p] must be >= 0 where fn[p] >= 0, and is ignored otherwise.  len_p = offsets[p+1] - offsets[p].
 *
 *   Windows: exactly the windows an -a scan sees: toAminoAcidOff codes, positions i in [0, len_p - 8) (the reference's
 *   off-by-one bound, KGJ:912), windows containing a code >= 20 skipped (KGJ:283-285); the device encode is the scan's own
 *   (encode_init / encode_block<true>).
 *   For a k-mer v: P(v) is the set of distinct proteins with a window equal to v, and n_v = |P(v)|.  Unannotated proteins
 *   count in n_v.  i_p(v) is the smallest position of v in protein p.  c_f is the number of proteins in P(v) with fn = f.
 *   f* is the f >= 0 with the largest c_f.  On a tie, take the smallest f.
 *   v is a signature iff both of these hold: f* exists and n_v >= min_proteins; 100 * c_f* >= purity_pct * n_v, computed in
 *   int64.
 *   Fields of the emitted kg_signature:
 *     kmer = v;  function_index = f*;
 *     otu_index = the most frequent otu[p] among the proteins of P(v) with fn = f*.  On a tie, take the smallest.
 *     avg_from_end = floor(sum (len_p - i_p(v)) / c_f*) over the same proteins.  This is consistent with the -O check
 *       |dpos - (last.avgOffFromEnd - ph.avgOffFromEnd)| <= 20 (KGJ:490-494).
 *     function_wt = the float32 quotient (float)c_f* / (float)n_v, correctly rounded (numpy's np.float32(c) / np.float32(n);
 *       __fdiv_rn on the device).
 *   Output: the signatures in ascending kmer order.  The output depends only on the multiset of (sequence, fn, otu).  It does
 *   not depend on protein order, pass count or launch geometry.
 *
 * Parameters: min_proteins >= 1, 1 <= purity_pct <= 100.  max_windows_per_pass = 0: the library sizes the pass from free device
 * memory (about 160 bytes per valid window); any other value caps the valid windows held at once (values above 2^32 - 2^22 act
 * as that limit).  The k-mer space is then processed in several passes over k-mer ranges, with range bounds taken from a
 * histogram of the windows' leading digits (refined where one bin alone is over the cap).  If one k-mer alone exceeds the
 * cap, the call returns KG_ERR_LIMIT and says so.
 * Limits (KG_ERR_LIMIT): n_prot < 2^29, len_p < 2^31, fewer than 2^31 window blocks of 64 windows, fewer than 2^32 signatures.
 * KG_ERR_ARG: fn < -1, otu < 0 on an annotated protein, decreasing offsets (each message names the first offending protein),
 * bad parameters, null pointers.  KG_ERR_NOMEM.  KG_TEST_FAIL_ALLOC applies to the call's device allocations; scratch goes back
 * to the driver before the call returns.
 * kg_signatures_derive reads a host sequence, uploaded through pinned pieces; kg_signatures_derive_device a device sequence
 * (complete before the call: the device is synchronised once); offsets, fn and otu are host arrays in both. */
typedef struct kg_derive_params {
    int32_t min_proteins;            /* >= 1 (this project's default: 2)     */
    int32_t purity_pct;              /* 1..100 (this project's default: 80)  */
    int64_t max_windows_per_pass;    /* 0: sized from free device memory     */
} kg_derive_params;

typedef struct kg_derive_stats {
    int64_t proteins;                /* n_prot                                                        */
    int64_t windows;                 /* sum over proteins of max(len_p - 8, 0)                        */
    int64_t valid_windows;           /* windows without a code >= 20                                  */
    int64_t pairs;                   /* distinct (k-mer, protein) pairs                               */
    int64_t kmers;                   /* distinct k-mers                                               */
    int64_t signatures;
    int32_t passes;                  /* k-mer range passes                                            */
    float   ms_encode;               /* histograms + encode / emit kernels                            */
    float   ms_sort;                 /* protein ranking + the window sorts                            */
    float   ms_reduce;               /* collapse, run reductions, selection, compaction               */
    float   ms_total;                /* the call, after the upload of the sequence, to its last kernel */
} kg_derive_stats;

typedef struct kg_sigset kg_sigset;

int kg_signatures_derive(int device, const kg_derive_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                         const int32_t *fn, const int32_t *otu, kg_sigset **out);
int kg_signatures_derive_device(int device, const kg_derive_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                                const int32_t *fn, const int32_t *otu, kg_sigset **out);
int64_t kg_sigset_count(const kg_sigset *s);
/* device array of kg_sigset_count(s) kg_signature records (8-byte aligned), valid until kg_sigset_free: kg_table_build_device
 * takes it as it is */
const kg_signature *kg_sigset_device(const kg_sigset *s);
/* records [first, first + count) into dst (host or device memory) */
int kg_sigset_copy(const kg_sigset *s, int64_t first, int64_t count, kg_signature *dst);
int kg_sigset_stats(const kg_sigset *s, kg_derive_stats *out);
void kg_sigset_free(kg_sigset *s);

/* ---- merging: a resident table plus new signatures -> the signatures of the united table (kernels: kg_merge.hpp) ----
 *
 * The reference only reads a table; this rule is the project's own.  It closes the loop scan -> cluster -> derive: the new
 * signatures go into the table the genome was scanned with, instead of into a table of their own.  Integers only: the 24 record
 * bytes are moved, never reinterpreted.
 *   Base set B.  B is every resident record j < kg_table_records(base) with 0 <= kmer < 20^8, with its bytes unchanged.  Records
 *   with kmer < 0 or kmer == 20^8 are occupied for the reference but can never be found.  They are left out and counted in
 *   base_ignored.  Empty records (kmer > 20^8) are neither.  B includes records the reference's lookup could not reach, for
 *   example one in front of its home slot: the merge reads the records, it does not walk them.  Tables made by kg_table_build*
 *   have none.
 *   New set N.  N is the n inputs in any order.  function_index is replaced by fn_map[function_index] when fn_map is non-null,
 *   and otu_index by otu_map[otu_index] likewise.  With a null map the field is kept.  The maps are host arrays of n_fn and
 *   n_otu entries.
 *   Result U.
 *     A k-mer only in B gives B's record.
 *     A k-mer only in N gives N's mapped record.  These are counted in added.
 *     A k-mer in both is a conflict, resolved by on_conflict: KG_MERGE_KEEP gives the base's record, KG_MERGE_REPLACE the new
 *     record, KG_MERGE_DROP the base's record if both name the same function, else neither.  The function comparison is made
 *     after mapping.
 *     replaced counts the conflicts where the new record won.  dropped counts the conflicts where neither survived.
 *     merged = |U|.
 *   Output: a kg_sigset in ascending k-mer order, so kg_sigset_device, kg_sigset_copy and kg_table_build_device take it as it is.
 *   For such a set kg_sigset_stats gives zeros except signatures, and kg_sigset_merge_stats gives the counts above (KG_ERR_ARG
 *   for a derived set).  n = 0 is the table's export.  The output depends only on B, N, the maps and the policy: not on the input
 *   order, launch geometry or scheduling.
 * Errors, raised in this order:
 *   1. KG_ERR_ARG: null table, out or params; a bad policy or reserved != 0; n < 0; a null array with n > 0; a map with a
 *      negative length; an unaligned device array.
 *   2. KG_ERR_BUSY: a kg_scan* is in flight on base.
 *   3. KG_ERR_LIMIT: kg_table_records(base) >= 2^32, or |B| + n >= 2^32.
 *   4. KG_ERR_ARG: a new k-mer outside [0, 20^8).  The message names the smallest such input index, in kg_table_build's words.
 *   5. KG_ERR_ARG: a function_index outside [0, n_fn) with a map given, then the same for otu_index.  The message names the
 *      smallest such input index.
 *   6. KG_ERR_ARG: a k-mer twice in N.  The message names the smallest such k-mer.
 *   7. KG_ERR_ARG: a k-mer twice in B, named likewise.
 *   8. KG_ERR_NOMEM.
 * base is not modified.  Scratch (about 24 bytes per record of B and N, plus the host input's 24 per signature) comes from the
 * base table's block cache, so KG_TEST_FAIL_ALLOC applies.  It goes back to the driver before the call returns, together with
 * the blocks the table's earlier scans left in the cache, and kg_table_live_device_bytes(base) is what it was before the call.
 * The set's own array is owned by the set, as for a derived set.
 * kg_table_merge_signatures reads a host array (pageable or pinned), uploaded through pinned pieces;
 * kg_table_merge_signatures_device an 8-byte aligned device array, complete before the call (the device is synchronised once). */
#define KG_MERGE_KEEP    0   /* a k-mer in both: the base's record                                   */
#define KG_MERGE_REPLACE 1   /* ... the new record                                                   */
#define KG_MERGE_DROP    2   /* ... the base's record if both name the same function, else neither   */
typedef struct kg_merge_params { int32_t on_conflict; int32_t reserved; } kg_merge_params;
typedef struct kg_merge_stats {
    int64_t base;                    /* |B|                                                           */
    int64_t base_ignored;            /* resident records with kmer < 0 or kmer == 20^8                */
    int64_t added_in;                /* n                                                             */
    int64_t added;                   /* k-mers only in N                                              */
    int64_t conflicts;               /* k-mers in both                                                */
    int64_t conflicts_same_function; /* ... whose two records name the same function after mapping    */
    int64_t replaced;                /* conflicts the new record won (KG_MERGE_REPLACE: all)          */
    int64_t dropped;                 /* conflicts neither record survived (KG_MERGE_DROP)             */
    int64_t merged;                  /* |U|                                                           */
    float   ms_extract;              /* the pass over the table and the new signatures' keys          */
    float   ms_sort;                 /* the sort of the |B| + n pairs (and the call's error read-back) */
    float   ms_resolve;              /* neighbour compare, prefix sum, the set's allocation, gather   */
    float   ms_total;
} kg_merge_stats;
int kg_table_merge_signatures(kg_table *base, const kg_merge_params *p, const kg_signature *sigs, int64_t n, const int32_t *fn_map,
                              int64_t n_fn, const int32_t *otu_map, int64_t n_otu, kg_sigset **out);
int kg_table_merge_signatures_device(kg_table *base, const kg_merge_params *p, const kg_signature *d_sigs, int64_t n,
                                     const int32_t *fn_map, int64_t n_fn, const int32_t *otu_map, int64_t n_otu, kg_sigset **out);
int kg_sigset_merge_stats(const kg_sigset *s, kg_merge_stats *out);

/* ---- protein families: proteins -> connected components of shared 8-mers (kernels: kg_cluster.hpp) ----
 *
 * The reference only reads signatures; this rule is the project's own.  It is the step between the proteins of evidence-free
 * ORFs and kg_signatures_derive: it says which hypothetical proteins of several genomes are the same protein.  Integers only.
 * Input: as for kg_signatures_derive, without fn and otu: seq, offsets[n_prot + 1] (host, non-decreasing),
 * len_p = offsets[p+1] - offsets[p].
 *   Windows: exactly the derive windows: toAminoAcidOff codes, positions i in [0, len_p - 8), windows with a code >= 20 skipped;
 *   the device encode is the scan's own (encode_init / encode_block<true>).
 *   P(v) is the set of distinct proteins that have a window equal to v.  d_p is the number of distinct k-mers of protein p.
 *   Centre.  For a k-mer v with |P(v)| >= 2, c(v) is the member of P(v) with the largest len_p.  On a tie it is the smallest
 *   index.  Every other member m of P(v) gives one link (m, c(v)).  This is Linclust's star: the work is linear in the
 *   (k-mer, protein) pairs whatever the size of P(v).
 *   Shared count.  s(m, c) is the number of distinct k-mers v with m in P(v), c(v) = c and m != c.
 *   Edge.  {m, c} is an edge iff both hold, computed in int64: s(m, c) >= min_shared; 100 * s(m, c) >= min_cover_pct * d_m.
 *   Family.  A family is a connected component of the edge graph.  A protein without an edge is a family of one; proteins
 *   with d_p = 0 are included in that.  A family's root is its smallest member index.  Families are numbered densely, 0..,
 *   in ascending root.
 *   Output: one 16-byte kg_family per protein, in protein order: family; root; best = the centre c with the largest s(p, c)
 *   among p's links that pass both tests, on a tie the smaller c, -1 when none passes; shared = that s, else 0.
 * Parameters kg_cluster_params { min_shared, min_cover_pct, reserved }: min_shared >= 1 (default 5), 0 <= min_cover_pct <= 100
 * (default 20), reserved == 0; anything else is KG_ERR_ARG.  The defaults are this project's choice: with exact 8-mers, a fifth
 * of the k-mers shared means roughly 80 % identity, the identity at which signatures of one member still hit another.
 * Dependence on order.  The partition depends on protein order only through ties of len_p in the centre choice.  The numbering
 * (family, root, best) depends on order by definition.  Nothing depends on launch geometry or scheduling.
 * Known weakness: single linkage chains, and a repeat or a domain shared by two families can join them.  That is stated, not
 * repaired; min_cover_pct is the lever.  (kg_proteins_cluster_aligned, below, is the repair: it verifies every edge by aligning
 * its two proteins.  This call stays as it is.)
 * One pass.  A call whose valid windows do not fit the device returns KG_ERR_LIMIT and says so.  max_windows = 0: the capacity
 * is sized from free device memory as the derive call does (about 160 bytes per valid window, at most 2^32 - 2^22 windows); any
 * other value caps it.
 * Limits (KG_ERR_LIMIT): n_prot < 2^29, len_p < 2^31, fewer than 2^31 window blocks of 64 windows.  KG_ERR_ARG: decreasing
 * offsets (the message names the first offending protein), bad parameters (the message names the first), max_windows < 0, null
 * pointers.  KG_ERR_NOMEM.  KG_TEST_FAIL_ALLOC applies to the call's device allocations; everything but the result array goes
 * back to the driver before the call returns.  Zero proteins are valid.
 * kg_proteins_cluster reads a host sequence, uploaded through pinned pieces; kg_proteins_cluster_device a device sequence
 * (complete before the call: the device is synchronised once); offsets is a host array in both. */
typedef struct kg_cluster_params { int32_t min_shared; int32_t min_cover_pct; int32_t reserved; } kg_cluster_params;
typedef struct kg_family {       /* 16 B */
    int32_t family;        /* dense number, in ascending root                           */
    int32_t root;          /* the family's smallest member index                        */
    int32_t best;          /* the centre of the protein's strongest edge, -1 when none  */
    int32_t shared;        /* s(p, best), else 0                                        */
} kg_family;
typedef struct kg_cluster_stats {
    int64_t proteins;
    int64_t valid_windows;
    int64_t pairs;         /* distinct (k-mer, protein) pairs                           */
    int64_t kmers;         /* distinct k-mers                                           */
    int64_t links;         /* distinct (m, c)                                           */
    int64_t edges;         /* links that pass both tests                                */
    int64_t families;
    int64_t families_multi;/* families of two or more proteins                          */
    int64_t largest;       /* members of the largest family                             */
    int32_t rounds;        /* hook-and-jump rounds until nothing changed                */
    float   ms_encode;     /* the histogram + the encode / emit kernel                  */
    float   ms_sort;       /* the window sort                                           */
    float   ms_link;       /* collapse, d_p, centres, link emit and sort, the two tests */
    float   ms_components; /* the rounds, the compress, the numbering                   */
    float   ms_total;      /* the call, after the upload of the sequence, to its last kernel */
} kg_cluster_stats;
typedef struct kg_familyset kg_familyset;
int kg_proteins_cluster(int device, const kg_cluster_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                        int64_t max_windows, kg_familyset **out);
int kg_proteins_cluster_device(int device, const kg_cluster_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                               int64_t max_windows, kg_familyset **out);
int64_t kg_familyset_count(const kg_familyset *s);
/* records [first, first + count) into dst (host or device memory) */
int kg_familyset_copy(const kg_familyset *s, int64_t first, int64_t count, kg_family *dst);
int kg_familyset_stats(const kg_familyset *s, kg_cluster_stats *out);
void kg_familyset_free(kg_familyset *s);

/* ---- verifying family edges: local alignment of the two proteins of a link (kernels: kg_align.hpp) ----
 *
 * The reference only reads signatures; this rule is the project's own.  It repairs the known weakness above: behind the 8-mer
 * tests the two proteins of every link are aligned, and the link stays an edge only if the alignment covers them.  Integers only.
 *   Residues: toAminoAcidOff codes, ACDEFGHIKLMNPQRSTVWY -> 0..19, everything else -> 20.
 *   Substitution scores: a symmetric 21 x 21 int8 matrix S, row-major in code order, entries in [-16, 16].  params.matrix gives
 *   the caller's (441 bytes); NULL means the built-in one: BLOSUM62 permuted into code order, with row and column 20 all -1.
 *   (BLOSUM62's own X row has 0 and -2 entries as well; one value for every pair with a non-residue is this project's
 *   simplification.)
 *   Score: for proteins a (length n) and b (length m), 1-based, boundary rows and columns H = 0 and E = F = -infinity:
 *       E[i][j] = max(E[i][j-1], H[i][j-1] - gap_open) - gap_extend
 *       F[i][j] = max(F[i-1][j], H[i-1][j] - gap_open) - gap_extend
 *       H[i][j] = max(0, H[i-1][j-1] + S[a_i][b_j], E[i][j], F[i][j])
 *       score(a, b) = the maximum of H over all cells, 0 for an empty protein
 *   A gap of k residues costs gap_open + k * gap_extend; the defaults are 11 and 1, the usual pairing for this matrix;
 *   gap_open >= 0, gap_extend >= 1.  (end_a, end_b) is the 0-based cell with H = score that has the smallest i, then the
 *   smallest j; (-1, -1) when score = 0.  There is no traceback in this pass (the opt-in pass below traces): the score is a
 *   maximum and does not depend on how ties inside the recurrence are broken; the end has the tie rule above.
 *   self(p) = the sum of S[x][x] over p's residues with code < 20: what a protein scores against itself, X aside.
 *   Abstaining: a pair with n * m > max_cells is not aligned: score = -1, end = (-1, -1), status skipped.  The default is
 *   2^26 cells (8192 x 8192): this project's choice, it bounds the longest wave.  max_cells >= 1.
 *   Edge test: a link (m, c) that passed the two 8-mer tests is kept iff score >= 1 and 100 * score >= min_ratio_pct * ref,
 *   computed in int64; ref = max(self(m), self(c)) with KG_ALIGN_REF_LONGER (the default), ref = self(m) with
 *   KG_ALIGN_REF_MEMBER; 0 <= min_ratio_pct <= 100, default 50.  A skipped pair is kept.  The ratio is the BLAST score ratio.
 *   Measured against the larger self-score it demands that both proteins are covered, which is what cuts a chain through a
 *   shared domain.  The price: a true fragment, such as a partial5 ORF at a contig end, falls out of its family;
 *   KG_ALIGN_REF_MEMBER is the lever.  The defaults 50 and LONGER are this project's choice.
 *   Families, root, family, best and shared follow the definitions above over the kept edges only: best is the centre of the
 *   largest s among the member's kept edges.
 * Nothing depends on launch geometry, pair order or scheduling: the maximum and its end are reduced with a total order
 * (score, then -i, then -j).
 *
 * kg_proteins_align / kg_proteins_align_device: seq and offsets as for kg_proteins_cluster (a host or a device sequence, host
 * offsets); pairs is a host int32[2 * n_pairs] of (a, b) protein indices: any order, repeats and a == b allowed.  out is a
 * host array of n_pairs kg_alignment, in pair order; status is 0 for aligned and 1 for skipped; the ratio test is not applied.
 * KG_ERR_ARG: null pointers, bad parameters (the message names the first), an asymmetric or out-of-range matrix, an index
 * outside [0, n_prot), decreasing offsets.  KG_ERR_LIMIT: len_p >= 2^24 (so that no score can reach 2^31).  KG_ERR_NOMEM.
 * KG_TEST_FAIL_ALLOC applies; all scratch goes back to the driver before the call returns.  Zero pairs and zero proteins are
 * valid.
 *
 * kg_proteins_cluster_aligned / _device: kg_proteins_cluster with the alignment step between the edge test and the component
 * rounds.  align == NULL: the code path, the kernels launched and the result are kg_proteins_cluster's.  The set then also
 * holds one 32-byte kg_family_edge per link that passed the 8-mer tests, in ascending (member, centre): status 0 kept, 1 cut,
 * 2 skipped (kg_familyset_edges_count is 0 for a set made without alignment), and kg_familyset_align_stats (KG_ERR_ARG for a set
 * made without alignment).  kg_cluster_stats.edges counts the kept edges; ms_link does not include ms_align. */
#define KG_ALIGN_REF_LONGER 0
#define KG_ALIGN_REF_MEMBER 1
#define KG_ALIGN_DEFAULT_MAX_CELLS (1ll << 26)
typedef struct kg_align_params {
    int32_t min_ratio_pct;
    int32_t ref;
    int32_t gap_open;
    int32_t gap_extend;
    int64_t max_cells;
    const int8_t *matrix;
    int64_t reserved;
} kg_align_params;
typedef struct kg_alignment {    /* 24 B */
    int32_t score;         /* -1 when skipped                                           */
    int32_t self_a;
    int32_t self_b;
    int32_t end_a;         /* 0-based, -1 when score <= 0                               */
    int32_t end_b;
    int32_t status;        /* 0 aligned, 1 skipped                                      */
} kg_alignment;
typedef struct kg_family_edge {  /* 32 B */
    int32_t member;
    int32_t centre;
    int32_t shared;        /* s(member, centre)                                         */
    int32_t score;
    int32_t ref;           /* the self-score the ratio is measured against              */
    int32_t end_member;
    int32_t end_centre;
    int32_t status;        /* 0 kept, 1 cut, 2 skipped (kept)                           */
} kg_family_edge;
typedef struct kg_align_stats {
    int64_t aligned;       /* links that passed the 8-mer tests and were aligned        */
    int64_t cut;
    int64_t skipped;
    int64_t cells;         /* n * m summed over the aligned pairs                       */
    float   ms_align;      /* compaction, alignment kernels, the cut                    */
    int32_t reserved;
} kg_align_stats;
int kg_proteins_align(int device, const kg_align_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                      const int32_t *pairs, int64_t n_pairs, kg_alignment *out);
int kg_proteins_align_device(int device, const kg_align_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                             const int32_t *pairs, int64_t n_pairs, kg_alignment *out);
int kg_proteins_cluster_aligned(int device, const kg_cluster_params *p, const kg_align_params *align, const uint8_t *seq,
                                const int64_t *offsets, int64_t n_prot, int64_t max_windows, kg_familyset **out);
int kg_proteins_cluster_aligned_device(int device, const kg_cluster_params *p, const kg_align_params *align, const uint8_t *d_seq,
                                       const int64_t *offsets, int64_t n_prot, int64_t max_windows, kg_familyset **out);
int64_t kg_familyset_edges_count(const kg_familyset *s);
/* edge records [first, first + count) into dst (host or device memory) */
int kg_familyset_edges_copy(const kg_familyset *s, int64_t first, int64_t count, kg_family_edge *dst);
int kg_familyset_align_stats(const kg_familyset *s, kg_align_stats *out);

/* ---- tracing alignments: start, identity and gaps of a pair whose end cell is known (kernel: kg_trace.hpp) ----
 *
 * An opt-in second pass behind the alignment above; this rule is the project's own.  Integers only.  H, E, F and S, the gaps,
 * the codes and (end_a, end_b) are the alignment's; indices below are 1-based as in its recurrence; open and ext are the gap
 * costs capped as the alignment kernel caps them (at 2^29 each: a gap that costs as much never pays).  The pass runs the
 * recurrence again over the prefix box that ends in the end cell, rows 0..end_a and columns 0..end_b, which gives the box's
 * cells the values they have in the whole matrix, and walks back.
 *   The path is the sequence of columns found by this walk, which starts in state H at the end cell.
 *   State H at (i, j).  H[i][j] > 0 holds here.
 *     If H[i][j] == H[i-1][j-1] + S[a_i][b_j]: emit the column (a_i, b_j) and step to (i-1, j-1).  If that cell is on the
 *     boundary or has H == 0, stop: the start is (i, j).  Otherwise stay in state H.
 *     Else if H[i][j] == E[i][j]: go to state E at (i, j).
 *     Else go to state F at (i, j).
 *     The preference order is diagonal, then E, then F.
 *   State E at (i, j).  Emit the column (-, b_j).
 *     If E[i][j] == H[i][j-1] - open - ext: go to state H at (i, j-1).  An opening is preferred to an extension on a tie.
 *     Else go to state E at (i, j-1).
 *   State F at (i, j).  Emit the column (a_i, -).
 *     If F[i][j] == H[i-1][j] - open - ext: go to state H at (i-1, j).
 *     Else go to state F at (i-1, j).
 *   A gap never reaches a cell with H == 0, so the walk stops only behind a diagonal step, and the path begins and ends with
 *   a residue pair.  The record is computed from the column string, not from the state changes: with gap_open = 0 the walk may
 *   pass through state H inside one gap, which stays one opening.
 *   Record: start_a, start_b, 0-based, the cell of the walk's last column; identical: residue columns (a_i, b_j) whose codes are
 *   equal and below 20; positive: residue columns with S[a_i][b_j] > 0; gap_opens: maximal runs of columns of one gap kind
 *   (a run of (-, b_j) next to a run of (a_i, -) is two); gap_cols_a: columns (-, b_j); gap_cols_b: columns (a_i, -).
 *   What follows from the record and the end cell:
 *       residue columns = (end_a - start_a + 1) - gap_cols_b = (end_b - start_b + 1) - gap_cols_a   (always equal)
 *       columns         = residue columns + gap_cols_a + gap_cols_b
 *       identity %      = 100 * identical / columns
 *       coverage of a % = 100 * (end_a - start_a + 1) / len_a, of b likewise
 *   Abstaining: a pair whose box (end_a + 1) * (end_b + 1) exceeds max_trace_cells is not traced: status 2.  The default is
 *   2^24 cells (4096 x 4096): this project's choice; with four bits a cell it bounds one pair's direction store at about
 *   8.5 MB for a box that is not much flatter than a 64-row stripe.  The store is kept per stripe of 64 rows, 32 bytes per column
 *   whatever the stripe's rows: (ceil((end_a + 1) / 64)) * (end_b + 64) * 32 bytes, so the worst box under the default cap, one
 *   row of 2^24 columns, takes 537 MB, and a caller who raises the cap raises that in proportion.  One pair's store is not
 *   bounded otherwise: such a pair runs alone.  max_trace_cells >= 1.
 * Nothing depends on launch geometry, pair order, scheduling or what a slab of direction bits held before.
 *
 * kg_proteins_align_paths / _device: kg_proteins_align's arguments, max_trace_cells, and paths beside out: a host array of
 * n_pairs kg_alignment_path in pair order.  out is byte for byte kg_proteins_align's.  Errors as there, then
 * "max_trace_cells must be >= 1" and "null paths".  A walk that leaves the rule or a box that does not reproduce the pair's
 * score is KG_ERR_DEVICE ("internal: ...").  KG_TEST_FAIL_ALLOC applies; all scratch goes back to the driver. */
#define KG_TRACE_DEFAULT_MAX_CELLS (1ll << 24)
#define KG_TRACE_HITS 1
#define KG_TRACE_ALL 2
typedef struct kg_alignment_path {   /* 32 B */
    int32_t start_a;       /* 0-based, -1 without a path                                */
    int32_t start_b;
    int32_t identical;
    int32_t positive;
    int32_t gap_opens;
    int32_t gap_cols_a;    /* columns (-, b_j)                                          */
    int32_t gap_cols_b;    /* columns (a_i, -)                                          */
    int32_t status;        /* 0 traced, 1 none (pair skipped, not asked for, or score <= 0), 2 untraced (over the cap) */
} kg_alignment_path;
typedef struct kg_trace_stats {
    int64_t traced;
    int64_t untraced;      /* status 2                                                  */
    int64_t cells;         /* box cells summed over the traced pairs                    */
    float   ms_trace;      /* the traceback pass: its uploads and its kernels           */
    int32_t reserved;
} kg_trace_stats;
int kg_proteins_align_paths(int device, const kg_align_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                            const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, kg_alignment *out,
                            kg_alignment_path *paths);
int kg_proteins_align_paths_device(int device, const kg_align_params *p, const uint8_t *d_seq, const int64_t *offsets,
                                   int64_t n_prot, const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells,
                                   kg_alignment *out, kg_alignment_path *paths);

/* ---- the alignments themselves: ops of the traced path (kernels: kg_trace.hpp, kg_ops.hpp) ----
 *
 * Opt-in beside the path records; this rule is the project's own.  Integers only.  The path is the column sequence of the walk
 * above; a is the query and b the target.  Read from the alignment's start to its end, every column has a kind:
 *     (a_i, b_j), identical by the record's definition (codes equal and below 20)   '='
 *     any other (a_i, b_j)                                                          'X'
 *     (a_i, -), consumes a only                                                     'I'
 *     (-, b_j), consumes b only                                                     'D'
 * In mode KG_TRACE_OPS '=' and 'X' are both 'M'; mode KG_TRACE_OPS_EQX keeps them apart.
 *   An op is a maximal run of columns of one kind, stored as one uint32_t: len << 4 | code, with BAM's codes (KG_OP_M 0, KG_OP_I 1,
 *   KG_OP_D 2, KG_OP_EQ 7, KG_OP_X 8).  len fits: a traced box has fewer than 2^25 columns under any cap the pass accepts.
 *   A record's ops are in alignment order, start to end: ops[op_start[r] .. op_start[r + 1]).  A record without a traced path
 *   (status 1 or 2) has none: op_start[r + 1] == op_start[r].  For every traced record:
 *     KG_TRACE_OPS:      n_ops <= 2 * gap_opens + 1; the I lengths sum to gap_cols_b, the D lengths to gap_cols_a, the M lengths to
 *                        the residue columns.
 *     KG_TRACE_OPS_EQX:  the '=' lengths sum to identical; merging neighbouring '=' and 'X' ops gives exactly the KG_TRACE_OPS ops.
 * Nothing depends on launch geometry, pair order, scheduling or what scratch held before.
 *   How: the walk stages two bits per column (at most end_a + end_b + 1 columns a pair, 16 to a word) and counts the kind changes;
 *   the counts are summed in record order and a second kernel writes the ops.  The staging of one call is scratch and at most 2 GiB
 *   (the columns of a typical path take about 44 bytes; the region is sized by the box, 152 bytes for a 300 x 300 one): over it
 *   KG_ERR_LIMIT names the byte count, as 2^32 or more ops in one call are KG_ERR_LIMIT.  The test hook KG_TEST_OPS_STAGE_BYTES=n
 *   (with KG_ENABLE_TEST_HOOKS=1, as the hooks above) lowers the limit to n bytes.
 *   The ops block is of the exact size and belongs to the result.
 *
 * kg_proteins_align_ops / _device: kg_proteins_align_paths' arguments, ops_mode (KG_TRACE_OPS or KG_TRACE_OPS_EQX, else KG_ERR_ARG
 * "ops_mode must be ...") and *ops: a set of op_start[n_pairs + 1] and the ops, in pair order.  out and paths are byte for byte
 * kg_proteins_align_paths'.  KG_TEST_FAIL_ALLOC applies; on a failure *ops is NULL and all device memory is back.
 * kg_opset_op_starts_copy copies count + 1 values, op_start[first .. first + count]; kg_opset_ops_copy ops [first_op, first_op +
 * count); dst is host or device memory.  kg_opset_ms_ops: the device time of the ops' own part (prefix sum and fill), ms.
 * In the search calls below the two modes are OR-ed into `trace`. */
#define KG_TRACE_OPS 4
#define KG_TRACE_OPS_EQX 8
#define KG_OP_M 0
#define KG_OP_I 1
#define KG_OP_D 2
#define KG_OP_EQ 7
#define KG_OP_X 8
typedef struct kg_opset kg_opset;
int kg_proteins_align_ops(int device, const kg_align_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                          const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, int ops_mode, kg_alignment *out,
                          kg_alignment_path *paths, kg_opset **ops);
int kg_proteins_align_ops_device(int device, const kg_align_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                                 const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, int ops_mode, kg_alignment *out,
                                 kg_alignment_path *paths, kg_opset **ops);
int64_t kg_opset_ops_count(const kg_opset *s);
int kg_opset_op_starts_copy(const kg_opset *s, int64_t first, int64_t count, int64_t *dst);
int kg_opset_ops_copy(const kg_opset *s, int64_t first_op, int64_t count, uint32_t *dst);
int kg_opset_ms_ops(const kg_opset *s, float *out);
void kg_opset_free(kg_opset *s);

/* ---- searching proteins against a database: 8-mer join, top candidates, alignment (kernels: kg_search.hpp) ----
 *
 * The reference only reads signatures; this rule is the project's own.  It answers which known protein a protein is like, and
 * how much: the prefilter of a protein search (the targets that share exact 8-mers with a query, counted and ranked) in front
 * of the alignment above.  Integers only.
 *   Input: one batch of n_prot proteins as for kg_proteins_cluster: seq, offsets[n_prot + 1] (host, non-decreasing), and n_db
 *   with 0 <= n_db <= n_prot.  Proteins [0, n_db) are the database, the targets; proteins [n_db, n_prot) are the queries, and
 *   query number q is batch index n_db + q; n_q = n_prot - n_db.
 *   Windows: exactly the derive windows: toAminoAcidOff codes, positions i in [0, len_p - 8), windows with a code >= 20 skipped;
 *   the device encode is the scan's own.
 *   Sets.  D(v) is the set of distinct targets that have a window equal to v, Q(v) the set of distinct queries.
 *   Masking.  A k-mer v with |D(v)| > max_db_per_kmer takes no part: it is a repeat or a low-complexity k-mer.  It is counted
 *   in kmers_masked (whether or not a query has it).  max_db_per_kmer >= 1, default 256: this project's choice; it bounds the join.
 *   Shared count.  s(q, d) is the number of distinct unmasked k-mers v with q in Q(v) and d in D(v).
 *   Candidates.  The candidates of q are the targets d with s(q, d) >= min_shared (min_shared >= 1, default 2), ordered by
 *   larger s, then smaller d.  The first max_cand of them are aligned (1 <= max_cand <= 64, default 8).
 *   Alignment: the rule above with the same kg_align_params (matrix, gaps, max_cells, min_ratio_pct, ref); a is the query and b
 *   the target.  A pair over max_cells is `skipped`.  An aligned pair is a `hit` iff score >= 1 and
 *   100 * score >= min_ratio_pct * ref, computed in int64; ref = max(self(q), self(d)) with KG_ALIGN_REF_LONGER, ref = self(q)
 *   with KG_ALIGN_REF_MEMBER (the member is the query); otherwise the pair is `below`.
 *   Output order within a query: not-skipped before skipped, then larger score, then larger s, then smaller target.
 *   Output: one 40-byte kg_search_hit per aligned or skipped candidate, in (query, rank) order, rank counting from 0 within the
 *   query, and hit_start[n_q + 1]: query q's records are [hit_start[q], hit_start[q + 1]).
 * Nothing depends on launch geometry, scheduling or where a tile border falls.  A query's records depend only on the query, the
 * database and the parameters, not on which other queries are in the batch (`query` aside, which is its number in the batch).
 * The order of the targets matters only under ties: equal s at the max_cand cut, and equal (score, s) in the output order.
 * One pass.  A call whose valid windows do not fit the device returns KG_ERR_LIMIT and says so, as kg_proteins_cluster does
 * (max_windows = 0: sized from free device memory).  join_pairs is the sum over the unmasked k-mers of |D(v)| * |Q(v)|: the
 * items the join writes.  A call whose join_pairs exceed the capacity returns KG_ERR_LIMIT; the message gives the count and
 * names max_db_per_kmer as the lever.  max_pairs = 0: the capacity is sized from free device memory (about 112 bytes per join
 * pair, at most 2^32 - 2^22); any other value caps it.
 * Limits (KG_ERR_LIMIT): n_prot < 2^29, len_p < 2^24, fewer than 2^31 window blocks of 64 windows.  KG_ERR_ARG: decreasing
 * offsets (the message names the first offending protein), bad parameters (the message names the first), n_db outside
 * [0, n_prot], max_windows < 0, max_pairs < 0, null pointers (align must not be null).  KG_ERR_NOMEM.  KG_TEST_FAIL_ALLOC
 * applies to every device allocation of the call; everything but the result goes back to the driver before the call returns.
 * Zero targets, zero queries, zero proteins and proteins without a window are valid.
 * kg_proteins_search reads a host sequence, uploaded through pinned pieces; kg_proteins_search_device a device sequence
 * (complete before the call: the device is synchronised once); offsets is a host array in both. */
typedef struct kg_search_params { int32_t min_shared; int32_t max_cand; int32_t max_db_per_kmer; int32_t reserved; } kg_search_params;
typedef struct kg_search_hit {   /* 40 B */
    int32_t query;         /* q: the protein's batch index is n_db + q                  */
    int32_t target;        /* d                                                         */
    int32_t shared;        /* s(q, d)                                                   */
    int32_t score;         /* -1 when skipped                                           */
    int32_t self_query;
    int32_t self_target;
    int32_t end_query;     /* 0-based, -1 when score <= 0                               */
    int32_t end_target;
    int32_t status;        /* 0 hit, 1 below, 2 skipped                                 */
    int32_t rank;          /* the record's place within its query, from 0               */
} kg_search_hit;
typedef struct kg_search_stats {
    int64_t targets;
    int64_t queries;
    int64_t valid_windows;
    int64_t pairs;         /* distinct (k-mer, protein) pairs of the whole batch        */
    int64_t kmers;         /* distinct k-mers of the whole batch                        */
    int64_t kmers_joined;  /* unmasked k-mers with a query and a target                 */
    int64_t kmers_masked;  /* k-mers with |D(v)| > max_db_per_kmer                      */
    int64_t join_pairs;    /* sum of |D(v)| * |Q(v)| over the joined k-mers             */
    int64_t candidates;    /* (q, d) with s >= min_shared, before the max_cand cut      */
    int64_t aligned;       /* records that were aligned                                 */
    int64_t hits;
    int64_t skipped;
    int64_t queries_hit;   /* queries whose rank-0 record is a hit                      */
    int64_t cells;         /* n * m summed over the aligned pairs                       */
    float   ms_encode;     /* the histogram + the encode / emit kernel                  */
    float   ms_sort;       /* the window sort                                           */
    float   ms_join;       /* collapse, runs, the join, its sort, the counts, the top candidates */
    float   ms_align;      /* the candidates to the host, the alignment kernels, the order */
    float   ms_total;      /* the call, after the upload of the sequence, to its last kernel */
    int32_t reserved;
} kg_search_stats;
typedef struct kg_hitset kg_hitset;
int kg_proteins_search(int device, const kg_search_params *p, const kg_align_params *align, const uint8_t *seq, const int64_t *offsets,
                       int64_t n_prot, int64_t n_db, int64_t max_windows, int64_t max_pairs, kg_hitset **out);
int kg_proteins_search_device(int device, const kg_search_params *p, const kg_align_params *align, const uint8_t *d_seq,
                              const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows, int64_t max_pairs,
                              kg_hitset **out);
int64_t kg_hitset_count(const kg_hitset *s);
/* records [first, first + count) into dst (host or device memory) */
int kg_hitset_copy(const kg_hitset *s, int64_t first, int64_t count, kg_search_hit *dst);
/* hit_start: all n_q + 1 entries */
int kg_hitset_starts_copy(const kg_hitset *s, int64_t *dst);
int kg_hitset_stats(const kg_hitset *s, kg_search_stats *out);
void kg_hitset_free(kg_hitset *s);
/* kg_proteins_search_paths / _device: the search with the traceback pass (above) behind it.  trace = KG_TRACE_HITS traces the
 * records with status hit only, KG_TRACE_ALL every aligned record with score >= 1; a is the query, b the target.  The hit
 * records, hit_start and kg_search_stats are kg_proteins_search's, byte for byte; ms_align and ms_total exclude ms_trace.
 * kg_hitset_paths_copy: one kg_alignment_path per hit record, same index; a record that was not traced has status 1 (not asked
 * for, skipped) or 2 (over max_trace_cells).  It and kg_hitset_trace_stats return KG_ERR_ARG for a set made by kg_proteins_search.
 * KG_ERR_ARG also: "trace must be KG_TRACE_HITS or KG_TRACE_ALL", "max_trace_cells must be >= 1". */
int kg_proteins_search_paths(int device, const kg_search_params *p, const kg_align_params *align, const uint8_t *seq,
                             const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows, int64_t max_pairs, int trace,
                             int64_t max_trace_cells, kg_hitset **out);
int kg_proteins_search_paths_device(int device, const kg_search_params *p, const kg_align_params *align, const uint8_t *d_seq,
                                    const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows, int64_t max_pairs,
                                    int trace, int64_t max_trace_cells, kg_hitset **out);
int kg_hitset_paths_copy(const kg_hitset *s, int64_t first, int64_t count, kg_alignment_path *dst);
int kg_hitset_trace_stats(const kg_hitset *s, kg_trace_stats *out);
/* The ops of the traced records (the rule: "the alignments themselves" above): trace = mode | KG_TRACE_OPS or mode | KG_TRACE_OPS_EQX
 * in kg_proteins_search_paths* and kg_proteins_search_seeded*.  trace & 3 is the mode and fails as before; both op bits, or a
 * bit above 15, are KG_ERR_ARG "trace takes at most one of KG_TRACE_OPS and KG_TRACE_OPS_EQX ...".  Everything else the call
 * returns is byte for byte the call's without the bit; kg_trace_stats.ms_trace then covers the ops' work (it replaces the plain
 * trace), kg_hitset_ms_ops is the ops' own part.  One op_start entry per hit record, plus one.  The getters return KG_ERR_ARG
 * for a set made without ops. */
int64_t kg_hitset_ops_count(const kg_hitset *s);
int kg_hitset_op_starts_copy(const kg_hitset *s, int64_t first, int64_t count, int64_t *dst);   /* count + 1 values */
int kg_hitset_ops_copy(const kg_hitset *s, int64_t first_op, int64_t count, uint32_t *dst);
int kg_hitset_ms_ops(const kg_hitset *s, float *out);

/* ---- the search with reduced-alphabet spaced seeds (kernel: kg_seed.hpp) ----
 *
 * kg_proteins_search finds a target only where it shares exact 8-mers with the query.  Here the prefilter seeds on a reduced
 * amino-acid alphabet, in which a substitution inside a class does not break a seed, and on spaced shapes, in which a
 * substitution on a don't-care position does not break it.  This rule is the project's own.  Integers only.
 *   The seed set has three parts.
 *   Class map.  cls[20] in code order ACDEFGHIKLMNPQRSTVWY, with values in 0..A-1.  Every class 0..A-1 is used, and
 *   2 <= A <= 20 (A is alphabet_size).
 *   Shapes.  n_shapes in 1..4.  Each shape is a 32-bit mask in which bit j set means position j of the window is a care
 *   position.  Bit 0 must be set.
 *   Span and weight.  span_k is the index of the highest set bit plus 1, so 1 <= span_k <= 32.  All shapes have the same
 *   number w of set bits, the weight.
 *   Space.  The seed space n_shapes * A^w must be at most 2^35.  The window key id << b | p then fits 64 bits for the
 *   n_prot < 2^29 the search already allows.
 *   Windows.  Window i of protein p under shape k is valid iff i + span_k < len_p and every care position i + j has a residue
 *   code below 20.  The last position is left out, as for the derive windows.  This keeps the rule a superset of the existing
 *   one.  Don't-care positions may hold any byte.
 *   Seed id.  The id is k * A^w + value.  value is the base-A number of the classes at the care positions, with the lowest
 *   position as the most significant digit.
 *   The rest is unchanged.  Everything behind this is kg_proteins_search's rule with "k-mer v" read as "seed id": D(v), Q(v),
 *   masking by max_db_per_kmer, s(q, d), candidates, alignment, order and records.  s(q, d) counts the distinct unmasked seed
 *   ids the two proteins share.  The same value under two shapes counts as two.  kg_search_stats keeps its layout.
 *   valid_windows counts valid (window, shape) pairs.  pairs counts distinct (seed id, protein) pairs.  kmers, kmers_joined
 *   and kmers_masked count distinct seed ids.  max_windows and the bytes-per-window figure apply to emitted seeds.
 *   Identity.  With the identity class map (A = 20) and the one shape 0xFF, the records, hit_start and every count of
 *   kg_search_stats equal kg_proteins_search's byte for byte.
 *   Built-in seed set `reduced` (this project's choice, not tuned).  Alphabet reduced11: the classes are AST, C, DEKNQR, F, G,
 *   H, ILV, M, P, W, Y, numbered in that order.  Two shapes of weight 9, written with the leftmost character as position 0:
 *   111101101011 (span 12) and 110110011010011 (span 15).  Space 2 * 11^9, about 4.7 * 10^9.
 * kg_seed_params_builtin fills *out with KG_SEEDS_EXACT (the identity map and 0xFF) or KG_SEEDS_REDUCED.
 * kg_proteins_search_seeded / _device: kg_proteins_search's arguments, the seed set, and trace: 0 gives no paths, and
 * max_trace_cells is then ignored; KG_TRACE_HITS and KG_TRACE_ALL behave as in kg_proteins_search_paths.  The result is a
 * kg_hitset, read with the getters above.  Errors as kg_proteins_search, and KG_ERR_ARG, the message naming the first offender:
 * null seeds, n_shapes outside 1..4, alphabet_size outside 2..20, a class at or above alphabet_size, an unused class, a shape
 * without bit 0, unequal weights, shape entries at or above n_shapes not zero, reserved != 0, seed space over 2^35. */
#define KG_SEEDS_EXACT 0
#define KG_SEEDS_REDUCED 1
typedef struct kg_seed_params { int32_t n_shapes; int32_t alphabet_size; uint8_t cls[20]; uint32_t shape[4]; int32_t reserved; } kg_seed_params; /* 48 B */
int kg_seed_params_builtin(int which, kg_seed_params *out);
int kg_proteins_search_seeded(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                              const uint8_t *seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                              int64_t max_pairs, int trace, int64_t max_trace_cells, kg_hitset **out);
int kg_proteins_search_seeded_device(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                                     const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                                     int64_t max_pairs, int trace, int64_t max_trace_cells, kg_hitset **out);

/* ---- low-complexity segments: masking proteins for the search and the families (kernels: kg_mask.hpp) ----
 *
 * max_db_per_kmer drops a k-mer only when many targets hold it; a poly-Q, a QEQEQE linker or a charged tail still seeds
 * candidates, and under a reduced alphabet more so.  This rule follows Wootton and Federhen's SEG, stages one and two: a trigger
 * window and the extension by a second threshold.  The third stage, the trimming to the least probable sub-segment, is not
 * done.  The rule is the project's own.  Integers only.
 *   Parameters: window W, trigger and extend; the thresholds are in units of 1/256 bit, the units of Lg (the procedure of rule 5
 *   of the coding section).
 *   Codes.  toAminoAcidOff's codes 0..19; every other byte, lowercase, X and * among them, is letter 20.
 *   Windows.  Window i of protein p covers residues i .. i + W - 1 and exists for 0 <= i <= len_p - W.  A window never spans
 *   two proteins; a protein shorter than W has none.
 *   Deficit.  n_a is the number of positions of the window with letter a, a in 0..20.  C(i) is the sum of n_a * Lg(n_a) over
 *   the letters with n_a >= 1, and D(i) = W * Lg(W) - C(i) >= 0: 256 * W times the window's entropy in bits, in Lg arithmetic.
 *   For W = 12: W * Lg(W) = 11004, and Lg(1..12) = 0, 256, 405, 512, 594, 661, 718, 768, 811, 850, 885, 917.  QEQEQEQEQEQE has
 *   D = 3072, twelve distinct letters have D = 11004, a homopolymer has D = 0.
 *   Tests.  low(i) iff D(i) <= W * trigger; ext(i) iff D(i) <= W * extend.
 *   Runs.  A maximal run of consecutive window positions that all have ext qualifies iff at least one of them has low.  Every
 *   window of a qualifying run is a masking window.
 *   Mask.  Residue j of p is masked iff some masking window i has i <= j <= i + W - 1.
 *   Segments.  The maximal runs of masked residues of a protein, in (protein, start) order, 0-based and inclusive.  Two
 *   qualifying runs whose residues touch or overlap give one segment.
 *   Limits and defaults.  4 <= window <= 32, 0 <= trigger <= extend < Lg(window), reserved = 0; otherwise KG_ERR_ARG, the message
 *   naming the first offender.  The defaults are 12, 563 and 640: SEG's 2.2 and 2.5 bits.  They are this project's choice and
 *   are not tuned.
 * Nothing depends on launch geometry, on where a tile border falls, or on which other proteins are in the batch.
 * kg_proteins_mask / _device: seq, offsets and n_prot as for kg_proteins_search, and so are the limits (n_prot < 2^29,
 * len_p < 2^24, fewer than 2^31 window blocks, fewer than 2^32 segments), the argument errors, KG_ERR_NOMEM and
 * KG_TEST_FAIL_ALLOC; everything but the result goes back to the driver before the call returns.  Zero proteins and proteins
 * without a window are valid.  kg_maskset_copy gives segments [first, first + count), kg_maskset_starts_copy seg_start[n_prot + 1]
 * (protein p's segments are [seg_start[p], seg_start[p + 1])), kg_maskset_flags_copy one 0/1 byte per residue for residues
 * [first, first + count) of the batch, residue 0 being offsets[0]; dst is host or device memory in all three.
 * kg_proteins_search_masked / _device: kg_proteins_search_seeded's arguments with seeds nullable (NULL: the exact 8-mers), the
 * mask parameters and sides: KG_MASK_QUERIES, KG_MASK_TARGETS or both.  Soft masking: the mask of that side's proteins is
 * computed on the device, and the window pass (and nothing else) reads a copy of the sequence in which every masked residue has
 * 0x20 set, which makes a letter lowercase and so a non-residue.  The alignment, the self-scores, the trace and the ops read the
 * original.  kg_search_hit, hit_start and kg_search_stats keep their layout; valid_windows and every count behind it count what
 * the masked copy gives, and ms_total includes the mask's time.  Under a spaced shape a masked residue on a don't-care position
 * keeps the seed: that follows from the seed rule.  kg_hitset_mask_stats gives the mask's statistics (of the masked side), and
 * KG_ERR_ARG for a set made by any other call.  KG_ERR_ARG also: "sides must be KG_MASK_QUERIES, KG_MASK_TARGETS or both".
 * kg_proteins_cluster_masked / _device: kg_proteins_cluster_aligned's arguments with align nullable (NULL: no alignment step),
 * and the mask parameters; every protein is masked.  A protein's "distinct 8-mers" in min_cover_pct are those of the masked
 * copy.  kg_familyset_mask_stats likewise.
 * The entry points above and their results are unchanged, byte for byte. */
#define KG_MASK_QUERIES 1
#define KG_MASK_TARGETS 2
typedef struct kg_mask_params { int32_t window; int32_t trigger; int32_t extend; int32_t reserved; } kg_mask_params;
typedef struct kg_mask_segment { int32_t protein; int32_t start; int32_t end; int32_t reserved; } kg_mask_segment;   /* 16 B */
typedef struct kg_mask_stats {
    int64_t proteins;
    int64_t residues;
    int64_t windows;           /* window positions: the sum of max(len_p - W + 1, 0)        */
    int64_t low_windows;
    int64_t ext_windows;
    int64_t masking_windows;   /* the windows of the qualifying runs                        */
    int64_t segments;
    int64_t masked_residues;
    int64_t proteins_masked;   /* proteins with a segment                                   */
    float   ms_mask;           /* the mask's kernels; under a search or cluster call the seeding copy too */
    int32_t reserved;
} kg_mask_stats;
typedef struct kg_maskset kg_maskset;
int kg_proteins_mask(int device, const kg_mask_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot, kg_maskset **out);
int kg_proteins_mask_device(int device, const kg_mask_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                            kg_maskset **out);
int64_t kg_maskset_count(const kg_maskset *s);
int kg_maskset_copy(const kg_maskset *s, int64_t first, int64_t count, kg_mask_segment *dst);
int kg_maskset_starts_copy(const kg_maskset *s, int64_t *dst);
int kg_maskset_flags_copy(const kg_maskset *s, int64_t first, int64_t count, uint8_t *dst);
int kg_maskset_stats(const kg_maskset *s, kg_mask_stats *out);
void kg_maskset_free(kg_maskset *s);
int kg_proteins_search_masked(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                              const uint8_t *seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                              int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                              kg_hitset **out);
int kg_proteins_search_masked_device(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                                     const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                                     int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                                     kg_hitset **out);
int kg_hitset_mask_stats(const kg_hitset *s, kg_mask_stats *out);
int kg_proteins_cluster_masked(int device, const kg_cluster_params *p, const kg_align_params *align, const uint8_t *seq,
                               const int64_t *offsets, int64_t n_prot, int64_t max_windows, const kg_mask_params *mask,
                               kg_familyset **out);
int kg_proteins_cluster_masked_device(int device, const kg_cluster_params *p, const kg_align_params *align, const uint8_t *d_seq,
                                      const int64_t *offsets, int64_t n_prot, int64_t max_windows, const kg_mask_params *mask,
                                      kg_familyset **out);
int kg_familyset_mask_stats(const kg_familyset *s, kg_mask_stats *out);

/* ---- the search's ungapped filter: candidates ranked by the score of their best seed diagonal (kernels: kg_ungapped.hpp) ----
 *
 * The shared count s(q, d) ranks poorly under a reduced alphabet: scattered chance seeds count as much as a collinear run.  This
 * stage stands between the join and the alignment, opt-in: it chooses each candidate's best seed diagonal, scores that whole
 * diagonal without gaps, and cuts by the score.  The rule is the project's own.  Integers only.
 *   Position.  For a protein p and an unmasked seed id v, i_p(v) is the smallest valid window position of v in p.  Under a mask it
 *   is taken in the masked copy, which has the same coordinates.
 *   Diagonals.  For a candidate (q, d) with s(q, d) >= min_shared, every shared unmasked seed v has the diagonal
 *   g(v) = i_q(v) - i_d(v).  m(g) is the number of shared seeds with that diagonal.  g* is the diagonal with the largest m, on a
 *   tie the smallest g.  on_diagonal = m(g*).  The sum of m over all g is s(q, d).
 *   Ungapped score.  The cells of diagonal g* are the pairs (a, a - g*) with 0 <= a < len_q and 0 <= a - g* < len_d, in
 *   increasing a.  A cell's score is the alignment's own: kg_align_params.matrix, or BLOSUM62 when it is null.  It uses the
 *   alignment's codes, every non-residue being code 20, and is read from the original sequence as the alignment reads it.
 *   u(q, d) is the largest sum over a non-empty run of consecutive cells, and 0 if every run is negative.  No X-drop and no band:
 *   the whole diagonal.  The result does not depend on launch geometry.
 *   Consequence: for every aligned, not-skipped record, u <= score (the run is an alignment without gaps).
 *   Cut.  A candidate with u < min_ungapped is dropped.  min_ungapped >= 0.  The default is 0, which drops nothing.  The
 *   remaining candidates of a query are ordered by larger u, then larger s, then smaller d.  The first max_cand are aligned.
 *   Alignment, hit test, output order within the query and the 40-byte kg_search_hit are unchanged.  kg_search_stats.candidates
 *   still counts the pairs with s >= min_shared.
 * kg_proteins_search_filtered / _device: kg_proteins_search_masked's arguments, with mask nullable as well (NULL: no mask, sides
 * is not read), and the ungapped parameters.  A null `ungapped` is KG_ERR_ARG "null kg_ungapped_params"; so are
 * "min_ungapped must be >= 0" and "kg_ungapped_params.reserved must be 0".  kg_hitset_ungapped_copy gives one 16-byte
 * kg_search_ungapped per hit record, same index; kg_hitset_ungapped_stats the stage's counts: scored = candidates,
 * scored = dropped + cut + the hit records.  ms_ungapped is the time of the scoring kernel; kg_search_stats.ms_join excludes it and
 * ms_total includes it.  Both getters return KG_ERR_ARG for a set made by any other call.
 * Limits (KG_ERR_LIMIT) beside the search's: the join key (q, d, g + bias) takes bits(n_q) + bits(n_db) + bits(longest query +
 * longest target) bits, bits(n) being the bits that write every value below n; over 64 the call says which three widths do not
 * fit.  The cut key takes bits(n_q) + the bits of the largest u + the bits of the largest s, and is refused over 64 likewise.
 * max_pairs = 0 sizes the join at about 200 bytes per join pair on this path: per pair the sort's two sides 24, two levels of
 * heads and scans 16, two levels of run starts 8 and the best-diagonal word 8; per candidate 32; per candidate kept by
 * min_ungapped 68; per aligned candidate 28; 184 in all, and the sorts' histograms.
 * The entry points above and their results are unchanged, byte for byte. */
typedef struct kg_ungapped_params { int32_t min_ungapped; int32_t reserved[3]; } kg_ungapped_params;
typedef struct kg_search_ungapped {   /* 16 B */
    int32_t ungapped;      /* u(q, d)                                                   */
    int32_t diagonal;      /* g*                                                        */
    int32_t on_diagonal;   /* m(g*)                                                     */
    int32_t reserved;
} kg_search_ungapped;
typedef struct kg_ungapped_stats {
    int64_t scored;        /* candidates whose diagonal was scored: kg_search_stats.candidates */
    int64_t dropped;       /* of them, those with u < min_ungapped                      */
    int64_t cut;           /* of the rest, those behind the first max_cand of their query */
    int64_t cells;         /* diagonal cells scored                                     */
    float   ms_ungapped;   /* the scoring kernel                                        */
    int32_t reserved;
} kg_ungapped_stats;
int kg_proteins_search_filtered(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                                const uint8_t *seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                                int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                                const kg_ungapped_params *ungapped, kg_hitset **out);
int kg_proteins_search_filtered_device(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                                       const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                                       int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                                       const kg_ungapped_params *ungapped, kg_hitset **out);
int kg_hitset_ungapped_copy(const kg_hitset *s, int64_t first, int64_t count, kg_search_ungapped *dst);
int kg_hitset_ungapped_stats(const kg_hitset *s, kg_ungapped_stats *out);

/* ---- banded alignment: the cells of a band around one diagonal per pair (kernels: kg_band.hpp, kg_trace.hpp) ----
 *
 * kg_proteins_align fills all n * m cells of a pair.  A search candidate carries the diagonal g* on which its seeds lie, and an
 * alignment that follows them stays near it.  Opt-in; the rule is the project's own.  Integers only.
 *   Everything is kg_proteins_align's rule: H, E, F, S, the gap costs and their caps, the codes, self, and 0-based end_a and end_b.
 *   One thing is added.  For a pair (a, b) with diagonal g and half-width W, the cell (i, j) (0-based, a_i against b_j) is in the
 *   band iff |(i - j) - g| <= W.  A cell outside the band has H = 0, exactly as a cell outside the matrix has; E and F follow from
 *   the unchanged recurrence.  So the banded score is the best local alignment whose every column, gap columns included, lies in
 *   the band: a diagonal step never leaves it, and a positive E or F never has a source outside it.
 *   score is the maximum of H over the in-band cells; (end_a, end_b) is the in-band cell with that H, the smallest i, then the
 *   smallest j, and (-1, -1) at score 0.  A band that misses the matrix altogether gives score 0.
 *   0 <= W <= KG_BAND_MAX = 256 (KG_ERR_ARG "band must be in [0, 256]"): a band wider than 513 diagonals is not a band, and the
 *   limit keeps one 64-row stripe's carry, at most 2 W + 64 columns, in the workgroup's LDS.  g is any int32.
 *   Abstaining.  band_cells = min(n * m, min(n, m) * (2 W + 1)) in int64; the pair is skipped iff band_cells > max_cells.  A pair
 *   that kg_proteins_align skips can therefore be aligned under a band.
 *   Consequences: the banded score is <= the full score; with W >= max(n - 1 - g, m - 1 + g) every record is byte for byte
 *   kg_proteins_align's; with W = 0 the score is the ungapped score u of diagonal g (the rule above); in the search u <= score
 *   still holds for every aligned record.
 *   Tracing under a band is the walk of kg_proteins_align_paths, word for word, over the same prefix box with the cells outside
 *   the band forced to H = 0.  max_trace_cells still caps the whole box (end_a + 1) * (end_b + 1); a box that does not reproduce
 *   the record's score stays KG_ERR_DEVICE, which is what proves that the two passes agree about the band.  The ops follow from
 *   the walk unchanged.
 * kg_band_params: a null pointer is KG_ERR_ARG "null kg_band_params", non-zero reserved "kg_band_params.reserved must be 0".
 * kg_proteins_align_banded / _device: kg_proteins_align_ops' arguments, then the band and `diagonals` (host memory, one per pair,
 * "null diagonals" when n_pairs > 0).  paths and ops may both be null (the records only); ops without paths is KG_ERR_ARG "ops
 * without paths"; without ops, ops_mode must be 0 ("ops_mode must be 0 without ops"); max_trace_cells is read only with paths.
 * kg_proteins_search_banded / _device: kg_proteins_search_filtered's arguments, then the band.  Every aligned candidate is aligned
 * in the band around its g*.  The prefilter, the ungapped stage, the cut, the hit test, the record order, kg_search_hit,
 * kg_search_ungapped and trace (paths and ops) are otherwise unchanged; kg_search_stats.cells keeps its definition (n * m of the
 * aligned pairs).  kg_hitset_band_stats gives the band's own counts over the aligned pairs; it is KG_ERR_ARG for a set made by
 * any other call.
 * The entry points above and their results are unchanged, byte for byte. */
#define KG_BAND_MAX 256
typedef struct kg_band_params { int32_t band; int32_t reserved[3]; } kg_band_params;
typedef struct kg_band_stats {
    int64_t band_cells;    /* sum of band_cells over the aligned pairs                  */
    int64_t full_cells;    /* sum of n * m over the same pairs: kg_search_stats.cells   */
    int32_t band;          /* W                                                         */
    int32_t reserved;
} kg_band_stats;
int kg_proteins_align_banded(int device, const kg_align_params *p, const uint8_t *seq, const int64_t *offsets, int64_t n_prot,
                             const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, int ops_mode, kg_alignment *out,
                             kg_alignment_path *paths, kg_opset **ops, const kg_band_params *band, const int32_t *diagonals);
int kg_proteins_align_banded_device(int device, const kg_align_params *p, const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot,
                                    const int32_t *pairs, int64_t n_pairs, int64_t max_trace_cells, int ops_mode, kg_alignment *out,
                                    kg_alignment_path *paths, kg_opset **ops, const kg_band_params *band, const int32_t *diagonals);
int kg_proteins_search_banded(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                              const uint8_t *seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                              int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                              const kg_ungapped_params *ungapped, const kg_band_params *band, kg_hitset **out);
int kg_proteins_search_banded_device(int device, const kg_search_params *p, const kg_seed_params *seeds, const kg_align_params *align,
                                     const uint8_t *d_seq, const int64_t *offsets, int64_t n_prot, int64_t n_db, int64_t max_windows,
                                     int64_t max_pairs, int trace, int64_t max_trace_cells, const kg_mask_params *mask, int sides,
                                     const kg_ungapped_params *ungapped, const kg_band_params *band, kg_hitset **out);
int kg_hitset_band_stats(const kg_hitset *s, kg_band_stats *out);

/* ---- a resident protein database: build once, save, open, search (kernels: kg_searchdb.hpp) ----
 *
 * Every search above takes the targets with the queries and starts from nothing.  A kg_searchdb is the targets' half of that
 * work kept on the device: a long-lived handle with a context of its own, as kg_table is.  One call at a time runs per handle; a
 * second concurrent call returns KG_ERR_BUSY.
 * The rule.  The hit records, hit_start, paths, ops, ungapped records and band statistics of kg_searchdb_search are byte for byte
 * those of kg_proteins_search_banded / _filtered / _masked / _seeded / _paths / kg_proteins_search (whichever the same options
 * select) on the batch "the handle's targets, then these queries", with the handle's seeds and with mask / sides describing the
 * same masking (the handle's mask on the targets, query_mask on the queries; the two must then hold the same values).  The result
 * is an ordinary kg_hitset and every getter works on it under the same conditions.  kg_hitset_stats has the same values, ms_*
 * aside: valid_windows and pairs are the sums of the two sides, kmers is the targets' k-mers plus the queries' minus the queries'
 * k-mers found among the targets', kmers_masked counts the targets' runs longer than max_db_per_kmer whether or not a query has
 * them; ms_encode and ms_sort cover the queries only.  kg_hitset_mask_stats gives the sums of the masked sides' counts.
 * kg_searchdb_build / _device: the targets' seq and offsets[n_db + 1] (host; the residues are those from offsets[0] on); seeds
 * (NULL: the exact 8-mers); mask (NULL: the targets are not masked); names, an opaque blob of names_bytes bytes which the handle
 * stores and hands back untouched (NULL with names_bytes = 0); max_windows as in the search; query_room, the residues of the
 * largest query batch a search may bring (0: 2^24).  The handle keeps on the device the targets' residues and offsets with room
 * for a query batch behind them, the distinct (k-mer, target) pairs in sorted order, each pair's window value, the k-mer run
 * starts and the distinct k-mers; on the host the seeds, the mask parameters and statistics, and names.  Everything else goes
 * back to the driver before the call returns.  Limits and errors are the search's: n_db < 2^29, len < 2^24, window blocks,
 * KG_ERR_LIMIT when the windows do not fit.  n_db = 0 and targets without a window are valid.
 * kg_searchdb_search / _device: the queries' seq (host / device) and offsets[n_q + 1] (host), the search's parameters, trace
 * (0: no paths) with max_trace_cells, query_mask (NULL: the queries are not masked), ungapped and band (either may be NULL; a
 * band without the ungapped stage is KG_ERR_ARG "null kg_ungapped_params", as kg_proteins_search_banded has it).  The other
 * KG_ERR_ARG words are the one-batch calls'.  max_windows counts the queries' windows alone.  ms_join holds ms_probe.  KG_ERR_LIMIT: n_db + n_q >= 2^29, and a batch of more residues than the room ("... residues of queries do not fit the
 * room of ..."); kg_searchdb_reserve regrows the room (a device-to-device copy).  kg_hitset_db_stats gives the probe's own
 * counts and times; it is KG_ERR_ARG for a set made by any other call.
 * KG_TEST_FAIL_ALLOC applies to every device allocation of build, open, reserve and search.  After a failed search or reserve
 * the handle is usable and its live bytes are what they were; after a failed build or open nothing is live.
 * The file (kg_searchdb_save / kg_searchdb_open), the project's own format.  All integers little-endian.
 *   Header, 448 bytes:
 *        0  8 bytes   magic "KGSRCHDB"
 *        8  u32       version = 1
 *       12  u32       header bytes = 448
 *       16  i64       n_db            24  i64  residues         32  i64  P, the pairs        40  i64  K, the k-mers
 *       48  i64       valid windows   56  i64  names_bytes
 *       64  u32       1 iff built with seeds        68  u32  1 iff built with a mask
 *       72  48 bytes  kg_seed_params (all 0 without seeds)
 *      120  16 bytes  kg_mask_params (all 0 without a mask)
 *      136  80 bytes  kg_mask_stats of the targets with ms_mask = 0 (all 0 without a mask)
 *      216  6 section entries of 24 bytes: u64 file offset, u64 bytes, u64 checksum
 *      360  u64       checksum of header bytes [0, 360)
 *      368  80 bytes  0
 *   Sections, in this order, each at the next multiple of 64 bytes behind the one before (the first at 448), the gaps and the
 *   file's end (itself a multiple of 64) zero-filled: 0 offsets, (n_db + 1) * 8 bytes, i64, offsets[0] = 0; 1 residues, one byte
 *   each; 2 pairs, P * 8, u64 v << bits(n_db) | d ascending; 3 values, P * 4, u32 beside the pairs; 4 run starts, (K + 1) * 4,
 *   u32; 5 names.  The file's bytes are a function of the build's inputs alone (query_room is not in it).
 *   Checksum of a byte string: pad it with zero bytes to a multiple of 8, read it as u64 words w_0 .. w_(n-1); the checksum is
 *   (sum of w_i * (2 i + 1) + the unpadded length) mod 2^64.  A changed byte changes one word by a non-zero amount times an odd
 *   factor, which is not 0 mod 2^64: any single changed byte is caught.
 * kg_searchdb_open checks, in this order and before the device is touched: the file's length against the header's, the magic, the
 * version and header bytes, the header checksum, every count (ranges, the six sections' bytes against the counts, their offsets
 * against the layout above, the file length), each section's checksum, and the offsets (offsets[0] = 0, non-decreasing, the
 * last equal to residues, every length < 2^24).  Anything wrong is KG_ERR_FORMAT (an unreadable file KG_ERR_IO) with a message
 * naming the first thing that is wrong.  No kernel reads a section whose checksum failed.  Beyond that the file is trusted: a
 * file whose checksums hold but whose pairs are not what a build makes of its residues is not detected.
 * An opened handle is indistinguishable from a built one (its build times are 0), and kg_searchdb_save of it writes the same bytes.
 * KG_SEARCHDB_NO_VERIFY=1 in the environment skips the section checksums (a measuring aid, read only with KG_ENABLE_TEST_HOOKS=1).
 * KG_TEST_SEARCHDB_REENTER=1 (likewise) makes kg_searchdb_search, once it holds the handle, call kg_searchdb_reserve on the same
 * handle and return that call's answer: KG_ERR_BUSY with its words, without a second thread. */
#define KG_SEARCHDB_VERSION 1
#define KG_SEARCHDB_HEADER_BYTES 448
#define KG_SEARCHDB_DEFAULT_ROOM (1ll << 24)
typedef struct kg_searchdb kg_searchdb;
typedef struct kg_searchdb_desc {   /* 240 B */
    int64_t targets;
    int64_t residues;
    int64_t pairs;
    int64_t kmers;
    int64_t valid_windows;
    int64_t names_bytes;
    int64_t query_room;        /* residues                                                  */
    int64_t device_bytes;      /* what the handle holds on the device                       */
    int32_t has_seeds;         /* 0: the exact 8-mers, and `seeds` is all 0                 */
    int32_t has_mask;
    kg_seed_params seeds;
    kg_mask_params mask;
    kg_mask_stats mask_stats;  /* the targets'; ms_mask is 0 in an opened handle            */
    float   ms_upload;         /* the build by stage; all 0 in an opened handle             */
    float   ms_encode;
    float   ms_sort;
    float   ms_index;          /* collapse, the runs, the k-mers, the copies into the handle */
    float   ms_total;
    int32_t reserved;
} kg_searchdb_desc;
typedef struct kg_search_db_stats {   /* 24 B */
    int64_t query_kmers;       /* distinct k-mers of the queries                            */
    int64_t found;             /* ... that the targets have too                             */
    float   ms_probe;
    float   ms_upload;         /* the queries' residues and offsets into the room           */
} kg_search_db_stats;
int kg_searchdb_build(int device, const uint8_t *seq, const int64_t *offsets, int64_t n_db, const kg_seed_params *seeds,
                      const kg_mask_params *mask, const void *names, int64_t names_bytes, int64_t max_windows, int64_t query_room,
                      kg_searchdb **out);
int kg_searchdb_build_device(int device, const uint8_t *d_seq, const int64_t *offsets, int64_t n_db, const kg_seed_params *seeds,
                             const kg_mask_params *mask, const void *names, int64_t names_bytes, int64_t max_windows,
                             int64_t query_room, kg_searchdb **out);
int kg_searchdb_save(kg_searchdb *db, const char *path);
int kg_searchdb_open(int device, const char *path, int64_t query_room, kg_searchdb **out);
int kg_searchdb_info(const kg_searchdb *db, kg_searchdb_desc *out);
/* all names_bytes bytes into dst (host memory) */
int kg_searchdb_names_copy(const kg_searchdb *db, void *dst);
int64_t kg_searchdb_live_device_bytes(kg_searchdb *db);
int kg_searchdb_reserve(kg_searchdb *db, int64_t query_room);
void kg_searchdb_free(kg_searchdb *db);
int kg_searchdb_search(kg_searchdb *db, const kg_search_params *p, const kg_align_params *align, const uint8_t *seq,
                       const int64_t *offsets, int64_t n_q, int64_t max_windows, int64_t max_pairs, int trace, int64_t max_trace_cells,
                       const kg_mask_params *query_mask, const kg_ungapped_params *ungapped, const kg_band_params *band, kg_hitset **out);
int kg_searchdb_search_device(kg_searchdb *db, const kg_search_params *p, const kg_align_params *align, const uint8_t *d_seq,
                              const int64_t *offsets, int64_t n_q, int64_t max_windows, int64_t max_pairs, int trace,
                              int64_t max_trace_cells, const kg_mask_params *query_mask, const kg_ungapped_params *ungapped,
                              const kg_band_params *band, kg_hitset **out);
int kg_hitset_db_stats(const kg_hitset *s, kg_search_db_stats *out);

/* ---- assigning functions: the CALL records of an -a scan -> one function per protein (kernels: kg_assign.hpp) ----
 *
 * The reference stops at the CALL lines (KGJ:398-404, 526-536); this rule is the project's own.
 * Protein p is one container of an -a scan.  Its CALLs are calls[call_start[p] .. call_start[p+1]), in emission order.
 *   For each function f among those CALLs:
 *     S_f = the sum of count over the protein's CALLs with fI == f, computed in int64;
 *     W_f = the float32 sum of weightedHits over the same CALLs: start from 0.0f, add one CALL at a time in emission order,
 *           each add rounded to nearest.
 *   T = sum over f of S_f.
 *   The best function is the f with the largest S_f; ties go to the largest W_f, then to the smallest f.  The runner-up is
 *   the next function in that same order.
 *   The protein is assigned iff both hold: it has at least one CALL and S_best >= min_score; 100 * S_best >= min_share_pct * T,
 *   computed in int64.
 *   otu = oI[0] of the protein's kg_otu record (the bubble at KGJ:432-437 keeps the largest count first); -1 when n == 0 or
 *   when no OTU array was given.
 * The output depends only on each protein's CALL sequence: not on launch geometry, nor on how many proteins are in the batch.
 * Defaults (this project's choice): min_score = 0, min_share_pct = 50.  Valid: min_score >= 0, 0 <= min_share_pct <= 100;
 * anything else is KG_ERR_ARG.
 * Errors: KG_ERR_ARG for a decreasing call_start or a negative count (the message names the first such protein), for
 * kg_result_assign on a DNA result or a KG_F_SKIP_AGGREGATE result; KG_ERR_LIMIT when S_best or T of a protein is 2^31 or more
 * (the message names the first such protein), or kg_assign_calls gets 2^31 or more proteins or 2^32 or more CALLs.  KG_ERR_BUSY
 * while a kg_scan* is in flight on the result's table.  Device allocations come from the table's block cache (a table-less
 * context for kg_assign_calls), so KG_TEST_FAIL_ALLOC applies; scratch is back in the cache when the call returns
 * (kg_table_live_device_bytes reads the same before and after). */
typedef struct kg_assign_params { int32_t min_score; int32_t min_share_pct; } kg_assign_params;
typedef struct kg_assignment {   /* 40 B */
    int32_t fI;            /* best function, -1 when the protein has no CALL          */
    int32_t assigned;      /* 1 iff the thresholds above hold                          */
    int32_t score;         /* S_best                                                   */
    int32_t total;         /* T                                                        */
    float   weighted;      /* W_best                                                   */
    int32_t n_calls;
    int32_t n_functions;   /* distinct fI among its CALLs                              */
    int32_t second_fi;     /* runner-up, -1 when none                                  */
    int32_t second_score;
    int32_t otu;
} kg_assignment;
/* an -a result of kg_scan* / kg_aggregate_hits -> n_seqs records into dst (host or device memory); *ms = device time
   of the assignment kernels (may be NULL) */
int kg_result_assign(kg_result *r, const kg_assign_params *p, kg_assignment *dst, float *ms);
/* caller-held CALL lists: host arrays calls[call_start[n_prot]], call_start[n_prot + 1], otu[n_prot] or NULL */
int kg_assign_calls(int device, const kg_assign_params *p, const kg_call *calls, const int64_t *call_start,
                    int64_t n_prot, const kg_otu *otu, kg_assignment *dst);

/* ---- locating functions: the CALL records of a DNA scan -> function regions on the contigs (kernels: kg_regions.hpp) ----
 *
 * The reference stops at the CALL lines, one list per (contig, strand, frame); this rule is the project's own.
 * Input: the CALL records of a DNA scan (aa == 0) in calls[] order (by container, emission order inside one), and the contig
 * lengths L_s = offsets[s+1] - offsets[s].  Container 6s + c is sequence s, strand '+' for c in {0,1,2} and '-' for c in
 * {3,4,5}, frame f = c mod 3 (kg_hit.container, KGJ:907-911, 1064-1072).
 *   1. Strand coordinates.  A CALL with start = a, end = b (residues; end already includes the K-1, KGJ:399-400) covers
 *      nucleotides x0 = f + 3a to x1 = f + 3b + 2, inclusive, counted from the 5' end of its own strand.  For records that come
 *      from a scan 0 <= x0 <= x1 <= L_s - 1 always holds (translate, KGJ:320-343, never yields a valid residue from an
 *      incomplete codon); for caller-held lists a record that breaks it is an error.
 *   2. Groups.  CALLs are grouped by (sequence, strand, fI) -- the three frames of a strand together.  Inside a group they are
 *      ordered by x0, ties by their index in calls[] (which is frame, then emission order).
 *   3. Regions.  Walking a group in that order with R = the largest x1 seen so far in the current region, a CALL joins the
 *      current region iff x0 - R - 1 <= merge_gap (int64); otherwise it opens a new one.  R is a running maximum, not the
 *      predecessor's end: a long CALL that contains a later short one keeps the region open.
 *   4. A region's record (kg_region, fixed layout, all int32 / float32 / uint32): seq; strand (0 '+', 1 '-'); left, right --
 *      0-based inclusive positions on the contig as given ('+': min x0, R; '-': L_s - 1 - R, L_s - 1 - min x0); fI;
 *      score = sum of count (int64, must be below 2^31); weighted = the float32 sum of weightedHits from 0.0f, one CALL at a
 *      time in the group order, each add rounded to nearest; n_calls; frames = bit f set for every frame among its CALLs (more
 *      than one bit: a frameshift candidate); best_frame = the frame of its CALL with the largest count (ties: the first in
 *      group order); first_call = index in calls[] of its first CALL in group order; kept = 1 iff score >= min_score and
 *      right - left + 1 >= min_len.
 *   5. Output order: by (seq, left, right, strand, fI) ascending -- a total order, since two regions of one group are
 *      disjoint -- plus region_start[n_seqs + 1] so that a contig's regions are one slice.  Every region is written, kept or
 *      not.
 *   6. Parameters kg_region_params { merge_gap, min_score, min_len }, all >= 0, else KG_ERR_ARG.  Defaults (this project's
 *      choice): merge_gap = 600 -- the scan's default -g 200 residues in nucleotides, i.e. two CALLs the scan would have kept
 *      in one list had they been in one frame -- and min_score = 0, min_len = 0.
 *   7. The output depends only on the multiset of (CALL, index) and the lengths: not on launch geometry, not on how many
 *      contigs share the batch.
 * Errors: KG_ERR_ARG for a protein (-a) result, a KG_F_SKIP_AGGREGATE result, null pointers, decreasing offsets, calls[] not
 * in non-decreasing container order, a container >= 6 * n_seqs, a negative count, a record outside [0, L_s) -- each message
 * names the first offending CALL (or contig); KG_ERR_LIMIT for a region whose score reaches 2^31 (the message names its
 * first_call), for n_calls >= 2^32, for a contig of 2^31 or more nucleotides or 2^31 or more contigs; KG_ERR_BUSY while a
 * kg_scan* is in flight on the result's table; KG_ERR_NOMEM.  A bad record is clamped before it is used as an index, so it
 * cannot make a kernel read or write outside its arrays.  Zero CALLs and zero sequences are valid and give an empty set.
 * Device allocations come from the table's block cache (a table-less context for kg_regions_calls), so KG_TEST_FAIL_ALLOC
 * applies; everything but the region set is back in the cache when the call returns.  A set made by kg_result_regions holds
 * blocks of the result's table (kg_table_live_device_bytes counts them) and must be freed before that table is closed. */
typedef struct kg_region_params { int32_t merge_gap; int32_t min_score; int32_t min_len; } kg_region_params;
typedef struct kg_region {       /* 48 B */
    int32_t  seq;
    int32_t  strand;       /* 0 '+', 1 '-'                                              */
    int32_t  left;         /* 0-based, inclusive, on the contig as given                */
    int32_t  right;
    int32_t  fI;
    int32_t  score;        /* sum of count                                              */
    float    weighted;     /* float32 sum of weightedHits in group order                */
    int32_t  n_calls;
    uint32_t frames;       /* bit f: a CALL of frame f                                  */
    int32_t  best_frame;
    uint32_t first_call;   /* index in calls[]                                          */
    int32_t  kept;
} kg_region;
typedef struct kg_region_stats {
    int64_t calls, groups, regions, kept;
    int64_t multi_frame;   /* regions with more than one frame bit                      */
    float   ms;            /* device time of the call's kernels                         */
    int32_t reserved;
} kg_region_stats;
typedef struct kg_regionset kg_regionset;
/* a DNA result of kg_scan* / kg_aggregate_hits plus the host offsets[n_seqs + 1] the scan was given (the result does not keep
   the lengths) */
int kg_result_regions(kg_result *r, const kg_region_params *p, const int64_t *offsets, kg_regionset **out);
/* caller-held host lists: calls[n_calls] in non-decreasing container order, offsets[n_seqs + 1] */
int kg_regions_calls(int device, const kg_region_params *p, const kg_call *calls, int64_t n_calls, const int64_t *offsets,
                     int64_t n_seqs, kg_regionset **out);
int64_t kg_regionset_count(const kg_regionset *s);
/* device array of kg_regionset_count(s) kg_region records in output order, valid until kg_regionset_free */
const kg_region *kg_regionset_device(const kg_regionset *s);
/* records [first, first + count) into dst (host or device memory) */
int kg_regionset_copy(const kg_regionset *s, int64_t first, int64_t count, kg_region *dst);
/* region_start[n_seqs + 1] into dst (host or device memory): contig s owns records [region_start[s], region_start[s+1]) */
int kg_regionset_seq_start(const kg_regionset *s, int64_t *dst);
int kg_regionset_stats(const kg_regionset *s, kg_region_stats *out);
void kg_regionset_free(kg_regionset *s);

/* ---- open reading frames: function regions -> the ORF around each and its translated protein (kernels: kg_orfs.hpp) ----
 *
 * The reference stops at the CALL lines; this rule is the project's own.
 * Input: a region set in output order, the batch's sequence bytes exactly as the scan got them, and offsets[n_seqs + 1].
 * One ORF record per region, index-aligned: orf[i] belongs to region[i].
 *   1. Strand and frame.  The strand is the region's, the frame is f = best_frame.  L = offsets[s+1] - offsets[s].  Strand
 *      nucleotide x is seq[x] on '+'; on '-' it is the complement of seq[L-1-x], taken on dna_code values (3 - c for c < 4, and
 *      4 stays 4): the reverse complement is never materialised.  Codon j of frame f is x = f+3j .. f+3j+2, for
 *      0 <= j < n_f = floor((L-f)/3) (n_f = 0 when L < f).  Codon classes by dna_code (a/A c/C g/G t/T/u/U, as the scan reads
 *      them): stop = TAA, TAG, TGA; start = the members of start_codons, a bit mask with 1 = ATG, 2 = GTG, 4 = TTG (default 7;
 *      with 0 there is no start search); unknown = any base of code 4 -- an unknown codon is neither stop nor start.
 *   2. Anchor.  The region's strand extent is [xa, xb]: left and right on '+', mirrored with L - 1 - x on '-'.
 *      j0 = ceil((xa - f)/3) is the first codon of frame f that lies wholly inside the region, j1 = floor((xb - 2 - f)/3) the
 *      last.  A region that comes from kg_result_regions always has 0 <= j0 <= j1 < n_f, because its best-frame CALL lies
 *      inside it.  For caller-held regions, a region that breaks this is an error; so are a bad seq, strand or best_frame,
 *      left > right and right >= L.
 *   3. Extension.  u = the largest j < j0 that is a stop, else -1.  e = the smallest j > j1 that is a stop, else n_f.
 *      b = the smallest j in (u, j0] that is a start, else u + 1.  i* = the smallest j >= j0 that is a stop; the region is
 *      interrupted when i* <= j1.  The ORF is codons b .. e: the stop codon is inside the coordinates, not inside the protein.
 *      When e == n_f it is b .. n_f - 1.
 *   4. Record kg_orf (48 bytes, twelve 32-bit fields): seq, strand, frame; left, right -- 0-based inclusive on the contig as
 *      given, mirrored for '-'; n_res = min(e, n_f) - b; start_codon -- 0 none, 1 ATG, 2 GTG, 3 TTG; first_inner -- the index in
 *      the protein of codon i* when interrupted, else -1; flags -- KG_ORF_HAS_STOP when e < n_f, KG_ORF_PARTIAL5 when u == -1,
 *      KG_ORF_INTERRUPTED, KG_ORF_MULTI_FRAME when the region has more than one frame bit; fI, score, kept -- copied from the
 *      region.  A multi-frame region gets its best frame's ORF and will usually be interrupted: this stage reports
 *      frameshifts, kg_regionset_repair below repairs them.
 *   5. Protein.  The residues of codons b .. min(e, n_f) - 1: each is the genetic code's letter (KGJ:88-93), an inner stop is
 *      '*', an unknown codon is 'X', and residue 0 is 'M' whenever start_codon != 0.  Proteins are laid end to end in ORF order
 *      behind prot_start[n_orfs + 1] (int64).  With only_kept = 1 (the default), an ORF whose region is not kept has length 0
 *      there; its record is still written.
 *   6. Independence.  The output depends only on (regions, bytes, offsets): not on launch geometry, tile size or batch
 *      neighbours.  Identical ORFs from regions of different functions are not merged.
 * Errors: KG_ERR_ARG for bad params (start_codons outside 0..7, only_kept outside 0..1), null pointers, n_seqs that is not the
 * set's, decreasing offsets, and the region errors of rule 2 -- each message names the first offending region (or contig);
 * KG_ERR_LIMIT for 2^31 or more regions, contigs or nucleotides of one contig, or 2^32 or more residues; KG_ERR_BUSY while a
 * kg_scan* is in flight on the set's table; KG_ERR_NOMEM.  A bad region is never used as an index.  Zero regions and zero
 * sequences are valid.  Device allocations come from the block cache of the region set's context (a table-less one for
 * kg_orfs_regions), so KG_TEST_FAIL_ALLOC applies; everything but the ORF set's three arrays is back in the cache when the call
 * returns.  An ORF set made by kg_regionset_orfs holds blocks of the region set's context and must be freed before it. */
#define KG_ORF_HAS_STOP     1u
#define KG_ORF_PARTIAL5     2u
#define KG_ORF_INTERRUPTED  4u
#define KG_ORF_MULTI_FRAME  8u
typedef struct kg_orf_params { int32_t start_codons; int32_t only_kept; int32_t reserved; } kg_orf_params;
typedef struct kg_orf {          /* 48 B */
    int32_t  seq;
    int32_t  strand;       /* 0 '+', 1 '-'                                              */
    int32_t  frame;
    int32_t  left;         /* 0-based, inclusive, on the contig as given                */
    int32_t  right;
    int32_t  n_res;        /* residues of the protein (the stop codon is not one)       */
    int32_t  start_codon;  /* 0 none, 1 ATG, 2 GTG, 3 TTG                               */
    int32_t  first_inner;  /* protein index of the first stop inside the region, or -1  */
    uint32_t flags;        /* KG_ORF_*                                                  */
    int32_t  fI;
    int32_t  score;
    int32_t  kept;
} kg_orf;
typedef struct kg_orf_stats {
    int64_t orfs;
    int64_t complete;      /* stop, start and not interrupted                           */
    int64_t interrupted;
    int64_t partial5;
    int64_t residues;      /* bytes behind prot_start                                   */
    int64_t tiles;         /* tile summaries written per scanned array                  */
    float   ms;            /* device time of the call's kernels                         */
    int32_t reserved;
} kg_orf_stats;
typedef struct kg_orfset kg_orfset;
/* the regions stay in HBM; seq: the batch's bytes, in device memory when seq_on_device != 0; offsets: host, n_seqs + 1 */
int kg_regionset_orfs(kg_regionset *set, const kg_orf_params *p, const uint8_t *seq, int seq_on_device, const int64_t *offsets,
                      int64_t n_seqs, kg_orfset **out);
/* caller-held host lists: regions[n_regions] in any order, seq and offsets[n_seqs + 1] on the host */
int kg_orfs_regions(int device, const kg_orf_params *p, const kg_region *regions, int64_t n_regions, const uint8_t *seq,
                    const int64_t *offsets, int64_t n_seqs, kg_orfset **out);
int64_t kg_orfset_count(const kg_orfset *s);
/* device array of kg_orfset_count(s) kg_orf records, valid until kg_orfset_free */
const kg_orf *kg_orfset_device(const kg_orfset *s);
/* records [first, first + count) into dst (host or device memory) */
int kg_orfset_copy(const kg_orfset *s, int64_t first, int64_t count, kg_orf *dst);
/* prot_start[count + 1] into dst (host or device memory) */
int kg_orfset_prot_start(const kg_orfset *s, int64_t *dst);
/* residue bytes [first, first + count) of the concatenated proteins into dst (host or device memory) */
int kg_orfset_residues(const kg_orfset *s, int64_t first, int64_t count, uint8_t *dst);
int kg_orfset_stats(const kg_orfset *s, kg_orf_stats *out);
void kg_orfset_free(kg_orfset *s);

/* ---- frameshift repair: the frames of a multi-frame region joined into one protein (kernels: kg_repair.hpp) ----
 *
 * The reference stops at the CALL lines; this rule is the project's own.  Integers only: the device's bytes equal a plain-loop
 * model's.  kg_regionset_orfs gives a region with CALLs in two frames its best frame's ORF alone, half protein and half
 * read-through; this stage follows the CALLs from frame to frame instead.
 * Input: a region set, its index-aligned ORF set, the CALL list the region set was made from, the batch's bytes and
 * offsets[n_seqs + 1].  Strand coordinates, codon j of frame f, n_f and the codon classes are rules 1 of the regions and ORF
 * sections.
 *   1. Candidates.  A region is a candidate when it is kept and has more than one frame bit.  Its CALLs are taken in the region
 *      stage's group order, by x0 and then by index in calls[].  CALLs with count < min_count are ignored for the chain only.
 *   2. Segments.  A segment is a maximal run of consecutive remaining CALLs of one frame.  Segment k has frame f_k, with
 *      f_k != f_{k+1}; A_k, the x0 of its first CALL; C_k, the largest x1 among its CALLs.  One segment (or no remaining CALL):
 *      the region is `single`.  More than max_junctions + 1 segments: it is `skipped`.  Both are left untouched.
 *   3. Junction k, between segments k and k+1, with p = f_k and q = f_{k+1}.  lp = (C_k - 2 - p)/3.  tp is the smallest stop
 *      j > lp of frame p, else n_p.  hi = p + 3 tp.  gq = (A_{k+1} - q)/3.  sq is the largest stop j < gq of frame q, else -1.
 *      lo = q + 3 (sq + 1).  mid = floor((C_k + 1 + A_{k+1}) / 2) in int64: the middle of the evidence gap, or of the overlap.
 *      If lo > hi the chain has failed.  Otherwise J_k = min(max(mid, lo), hi).  The chain also fails when J_k >= J_{k+1} for
 *      some k, or when a part below is empty.
 *   4. Ends.  j0 = (A_1 - f_1)/3.  u is the largest stop < j0 of frame f_1, else -1.  b is the smallest start of the mask in
 *      (u, j0], else u + 1.  jl = (C_m - 2 - f_m)/3.  e is the smallest stop > jl of frame f_m, else n_{f_m}.
 *   5. Parts.  Part 1 is the codons j >= b of f_1 with f_1 + 3j + 3 <= J_1.  Part k is the codons of f_k with
 *      J_{k-1} <= f_k + 3j and f_k + 3j + 3 <= J_k.  Part m is the codons of f_m with f_m + 3j >= J_{m-1} and
 *      j < min(e, n_{f_m}).  The protein is the parts end to end under the ORF section's rule 5: 'M' first when a start was
 *      found, 'X' for an unknown codon, '*' for a stop.  A stop can only lie inside a segment's own evidence span.  The one or
 *      two nucleotides between two parts give no residue, and the parts are disjoint codons inside left .. right, so
 *      3 * n_res <= right - left + 1 still holds, and kg_orfset_coding and kg_orfset_starts accept the record.
 *   6. Record, 48 bytes as before.  frame = f_1.  The extent runs from codon b of f_1 to the stop codon e of f_m, or to
 *      n_f - 1 when e == n_f; it is mirrored on '-'.  n_res is the parts' total.  start_codon is as in rule 4 of the ORF section.
 *      first_inner is the first '*' of the new protein, or -1.  flags are KG_ORF_HAS_STOP and KG_ORF_PARTIAL5 from the new
 *      ends, KG_ORF_MULTI_FRAME, the new KG_ORF_REPAIRED, and KG_ORF_INTERRUPTED always set.  A repaired record does not read in
 *      one frame.  With INTERRUPTED set, coding_is_training and the movable test of kg_starts.hpp go on leaving it alone with
 *      their code unchanged.  fI, score and kept are copied.  A failed, single or skipped region keeps its given record and
 *      protein.
 *   7. Junction record.  kg_junction is six int32, 24 bytes: orf; pos, which is J_k as a 0-based contig coordinate,
 *      L - 1 - J_k on '-'; from_frame; to_frame; res, the protein index of the 3' part's first residue;
 *      gap = A_{k+1} - C_k - 1, negative when the evidence overlaps.  Records are in (orf, k) order, with
 *      junction_start[n_orfs + 1].
 *   8. Independence.  The output depends only on (regions, ORFs, CALLs, bytes, offsets, parameters): not on launch geometry,
 *      tile size or batch neighbours.  C_k is an integer maximum, so order cannot matter.
 * Parameters kg_repair_params { start_codons (0..7, default 7), min_count (>= 0, default 0), max_junctions (1..8, default 4),
 * reserved == 0 }; anything else is KG_ERR_ARG.  The defaults are this project's choice.
 * kg_regionset_repair gives a NEW ORF set in the region set's context, as kg_orfset_add_free does: in it the record and protein
 * of every repaired region are replaced by the chain; every other record, its protein bytes and the only_kept zero lengths are
 * unchanged byte for byte.  The given sets stay valid; the new one is freed before them.  It runs before kg_orfset_add_free:
 * the ORF set must have exactly the region set's records.  kg_orfset_stats of the new set is the given set's with residues,
 * complete, interrupted and partial5 brought up to date.  The junction list stays with the new set only: the sets that
 * kg_orfset_add_free, kg_orfset_coding and kg_orfset_starts make from it keep the records' indices, the repaired records and
 * their proteins, but not the list.  A given set may carry KG_ORF_REPAIRED records (it is one of those sets, or an earlier
 * call's): they are kept, record and protein, unless this call repairs them again, and the junction list is this call's alone.
 * kg_result_repair passes the result's device CALLs.  The coding score of a repaired record (rule 2 of the coding section) is
 * that of its first frame read straight through its extent.
 * Validation.  The CALL list must be the set's: every CALL has to fall inside exactly one region of its group, and every
 * region's count and summed count have to equal its n_calls and score; otherwise KG_ERR_ARG, and the message names the first
 * offending CALL or region.  The CALL errors of the regions section apply as well.
 * Errors: KG_ERR_ARG also for bad params, null pointers, an ORF set that is not index-aligned with the region set or of another
 * context, n_seqs that is not the set's, decreasing offsets; KG_ERR_LIMIT for 2^32 or more CALLs or residues; KG_ERR_BUSY
 * while a kg_scan* is in flight on the set's table; KG_ERR_NOMEM.  A bad record is never used as an index.  Zero regions,
 * CALLs and sequences are valid.  Device allocations come from the context's block cache, so KG_TEST_FAIL_ALLOC applies;
 * everything but the new set's arrays and the two junction arrays is back in the cache on every path out. */
#define KG_ORF_REPAIRED   128u
typedef struct kg_repair_params { int32_t start_codons; int32_t min_count; int32_t max_junctions; int32_t reserved; } kg_repair_params;
typedef struct kg_junction {     /* 24 B */
    int32_t  orf;          /* index in the ORF set                                     */
    int32_t  pos;          /* J_k: 0-based on the contig as given                      */
    int32_t  from_frame;
    int32_t  to_frame;
    int32_t  res;          /* protein index of the 3' part's first residue             */
    int32_t  gap;          /* A_{k+1} - C_k - 1                                        */
} kg_junction;
typedef struct kg_repair_stats {
    int64_t candidates;    /* kept regions with more than one frame bit                */
    int64_t repaired, failed, single, skipped;
    int64_t junctions;
    int64_t residues;      /* of the repaired proteins                                 */
    float   ms;            /* device time of the call's kernels                        */
    int32_t reserved;
} kg_repair_stats;
/* calls[n_calls]: the region set's CALL list, in device memory when calls_on_device != 0; seq, offsets as kg_regionset_orfs
   takes them */
int kg_regionset_repair(kg_regionset *set, kg_orfset *orfs, const kg_call *calls, int calls_on_device, int64_t n_calls,
                        const kg_repair_params *p, const uint8_t *seq, int seq_on_device, const int64_t *offsets, int64_t n_seqs,
                        kg_orfset **out);
/* the same with the device CALLs of the DNA result the region set was made from */
int kg_result_repair(kg_result *r, kg_regionset *set, kg_orfset *orfs, const kg_repair_params *p, const uint8_t *seq,
                     int seq_on_device, const int64_t *offsets, int64_t n_seqs, kg_orfset **out);
/* the junction list of a set made by kg_regionset_repair (KG_ERR_ARG on any other set, 0 for the count) */
int64_t kg_orfset_junctions_count(const kg_orfset *s);
/* records [first, first + count) into dst (host or device memory) */
int kg_orfset_junctions_copy(const kg_orfset *s, int64_t first, int64_t count, kg_junction *dst);
/* junction_start[count of ORFs + 1] into dst (host or device memory) */
int kg_orfset_junctions_start(const kg_orfset *s, int64_t *dst);
int kg_orfset_junctions_stats(const kg_orfset *s, kg_repair_stats *out);

/* ---- evidence-free open reading frames: every long stop-free run of the six frames (kernels: kg_orfs.hpp) ----
 *
 * The reference stops at the CALL lines; this rule is the project's own.  It fills a gene set with ab initio candidates
 * ("hypothetical protein") where the table knows no family.
 * Input: the batch's sequence bytes exactly as the scan got them, and offsets[n_seqs + 1].  No table and no region takes part.
 * Strand, frame, codon j of frame f, n_f and the codon classes (stop, start by the start_codons mask, unknown) are exactly
 * rule 1 of the ORF section above.
 *   1. Runs.  For every contig, strand and frame (the scan's six containers), the stops of the frame are the codons j that are
 *      stops.  A run is (u, e): e is a stop, or e = n_f once per container (the run that reaches the contig's end); u is the
 *      largest stop < e, else -1.  A container with n_f = 0 has no run.
 *   2. Start.  b is the smallest start in (u, e).  Without one, b = u + 1 when u == -1 or start_codons == 0; otherwise the run
 *      gives no candidate.
 *   3. Length.  n_res = min(e, n_f) - b.  The run gives a candidate iff n_res >= min_res.
 *   4. Record.  The candidate is a kg_orf with the fields and the coordinate rule of rule 4 of the ORF section: left .. right
 *      covers codons b .. e, or b .. n_f - 1 when e == n_f, mirrored on '-'; start_codon as there; first_inner = -1, fI = -1,
 *      score = 0, kept = 1; flags = KG_ORF_FREE, plus KG_ORF_HAS_STOP when e < n_f, plus KG_ORF_PARTIAL5 when u == -1.  It is
 *      never INTERRUPTED or MULTI_FRAME.
 *   5. Protein.  Exactly rule 5 of the ORF section: 'M' first when start_codon != 0, 'X' for an unknown codon.  By construction
 *      there is no '*'.  An unknown codon is neither stop nor start, so a run of N's is a run: that is stated, not repaired.
 *   6. Order.  By contig, then strand ('+' first), then frame 0, 1, 2, then increasing b: the scan's container order.
 *   7. Independence.  The output depends only on (bytes, offsets, parameters): not on launch geometry, tile size or batch
 *      neighbours.
 * Parameters kg_free_params { min_res, start_codons, reserved }: min_res >= 1 (default 100, this project's choice),
 * start_codons in 0..7 (default 7), reserved == 0; anything else is KG_ERR_ARG.
 * Selection.  score = 0 is this project's choice too.  Every kept evidence region has a score of at least minHits >= 2, so under
 * the selection rule below an evidence candidate never loses to a free one, and among free ones the longer wins: adding free
 * ORFs to an ORF set cannot change the selection state (or `by`) of any evidence ORF.  A weak evidence region therefore still
 * beats a long free ORF; the region stage's min_score is the caller's lever.
 * kg_orfs_free is table-less and gives an ordinary ORF set of the free candidates alone: every kg_orfset_* call works on it.
 * kg_orfset_add_free gives a NEW ORF set in the given set's context: the given set's records first, index-aligned and
 * unchanged (its only_kept zero lengths too), then the free candidates of the same batch in rule-6 order; prot_start and the
 * residues cover both parts.  The given set stays valid; the new one holds blocks of the same context, so it is freed before
 * the given set when that one owns its context (kg_orfs_regions, kg_orfs_free) and before the region set otherwise, as its
 * parent is.  kg_orfset_stats keeps its layout: orfs, complete, partial5 and residues count the whole set (the free ones are
 * the count minus the parent's), interrupted is the parent's.
 * Errors: KG_ERR_ARG for bad params, null pointers, n_seqs that is not the given set's, decreasing offsets; KG_ERR_LIMIT for
 * 2^31 or more contigs, nucleotides of one contig or candidates (the given set's included), or 2^32 or more residues;
 * KG_ERR_BUSY while a kg_scan* is in flight on the given set's table; KG_ERR_NOMEM.  Zero sequences are valid.  Device
 * allocations come from the context's block cache, so KG_TEST_FAIL_ALLOC applies; everything but the new set's three arrays is
 * back in the cache on every path out. */
#define KG_ORF_FREE        16u
typedef struct kg_free_params { int32_t min_res; int32_t start_codons; int32_t reserved; } kg_free_params;
/* seq: the batch's bytes, in device memory when seq_on_device != 0; offsets: host, n_seqs + 1 */
int kg_orfs_free(int device, const kg_free_params *p, const uint8_t *seq, int seq_on_device, const int64_t *offsets,
                 int64_t n_seqs, kg_orfset **out);
int kg_orfset_add_free(kg_orfset *set, const kg_free_params *p, const uint8_t *seq, int seq_on_device, const int64_t *offsets,
                       int64_t n_seqs, kg_orfset **out);

/* ---- coding potential: the in-frame hexamer (dicodon) log-odds of every ORF; non-coding free ORFs dropped (kernels: kg_coding.hpp) ----
 *
 * The reference stops at the CALL lines; this rule is the project's own.  Integers only: the device's bytes equal a plain-loop
 * model's.  It is the first filter between kg_orfset_add_free and the families learnt from its proteins: a free ORF on a gene's
 * other strand, or a random one, is explained better by the genome's background than by its genes.
 * Input: ORF records, the batch's sequence bytes exactly as the scan got them, and offsets[n_seqs + 1].  Nucleotide codes,
 * strands, codons and n_f are rule 1 of the ORF section.  The codes are dna_code: A 0, C 1, G 2, T/U 3, anything else 4.  The '-'
 * strand is read as 3 - c of seq[L-1-x] and is never materialised.
 *   1. Hexamer index.  Six bases of one strand, all of code < 4, give h = sum b_i * 4^(5-i), with the first base most
 *      significant.  0 <= h < 4096.  h = 64 * codon_k + codon_(k+1) with codon = 16 b0 + 4 b1 + b2.  A hexamer with a base of
 *      code 4 does not exist.  It is not counted and it scores 0.
 *   2. Pairs of an ORF record.  They are taken from the record alone (seq, strand, left, right, n_res), not from prot_start, so
 *      only_kept zero lengths play no part.  Codon k (0 <= k < n_res) starts at strand position xs + 3k.  xs = left on '+', and
 *      xs = L - 1 - right on '-'.  Pair k is codons k, k+1, for 0 <= k < n_res - 1.  The stop codon is in no pair.  A record
 *      with n_res < 2 has no pair.
 *   3. Coding counts C[4096] (int64).  A training record has kept != 0 and flags & (KG_ORF_FREE | KG_ORF_INTERRUPTED) == 0.
 *      C[h] is the number of pairs with index h over all training records.  Identical ORFs from regions of different functions
 *      are each counted.  This is stated, not repaired.
 *   4. Background counts B[4096] (int64).  For every contig and every x in [0, L - 6] whose six bases seq[x .. x+5] are all
 *      known, count B[h]++ and B[rc(h)]++.  rc(h) is the index of the reverse complement.  A hexamer never spans two contigs.
 *      A contig with L < 6 gives none.
 *   5. Score table T[4096] (int32).  Host code, integers only.  SC = sum C + 4096 and SB = sum B + 4096.
 *      T[h] = Lg(C[h] + 1) - Lg(SC) - Lg(B[h] + 1) + Lg(SB).  Lg(x) for 1 <= x < 2^63 is defined by this procedure, not by
 *      log2: n = floor(log2 x) is the bit length minus 1; y = x << (63 - n), f = 0; eight times: y = (y * y) >> 63 as a 128-bit
 *      product, and if y >= 2^64 then y >>= 1 and f = 2f + 1, else f = 2f; Lg = 256 n + f.  Lg(1) = 0, Lg(2) = 256, Lg(3) = 405,
 *      Lg(4096) = 3072, Lg(2^63 - 1) = 16127; the procedure is within 1 of floor(256 log2 x).
 *   6. Score.  S (int64) is the sum of T[h] over the record's pairs.  Every record of the set is scored, whatever its flags
 *      and kept.
 *   7. Decision.  A record with KG_ORF_FREE, kept != 0 and S < min_coding gets kept = 0 and the new flag KG_ORF_NONCODING.
 *      Nothing else in any record changes.  An evidence ORF is never dropped.  min_coding defaults to 0: the background explains
 *      the ORF at least as well as the coding model.  This is the project's choice.
 *   8. Trained or not.  A call without a caller's table trains on its own set (rules 3 to 5) when sum C >= min_train_pairs.
 *      min_train_pairs defaults to 100 000, roughly a hundred average genes.  This is the project's choice.  Below that, the
 *      call is untrained: all scores are 0 and no record changes.  That is a valid result and not an error.
 *   9. Independence.  The output depends only on (records, bytes, offsets, parameters, table).  It does not depend on launch
 *      geometry, tile size or batch neighbours.  All device sums are integer atomics or integer reductions, so order cannot
 *      matter.
 * kg_orfset_coding gives a NEW ORF set in the given set's context, as kg_orfset_add_free does: the given set's records under
 * rule 7, its prot_start and residues unchanged, and an int64 score per record.  The given set stays valid; the new one is
 * freed before it.  kg_orfset_select on the new set sees the lowered kept, so a non-coding free ORF suppresses nothing.  With
 * table == NULL the call trains on its own set; that path has one host wait in the middle (counts down, T on the host, T up).
 * With a table (int32[4096], host memory) no count is made and kg_orfset_coding_model gives zeros.  A caller's table may hold
 * any int32 values (a large negative entry as a "forbidden hexamer" too): every sum is carried in 64 bits and S is exact.
 * kg_coding_table is host-only and uses no GPU; a negative count, or counts whose sum is 2^62 or more, are KG_ERR_ARG.
 * kg_coding_counts_orfs and kg_coding_score_orfs are the table-less twins for caller-held host lists.  A caller-held record must
 * have seq in [0, n_seqs), strand 0 or 1, 0 <= left <= right < L and 3 * n_res <= right - left + 1; one that breaks any of
 * these is KG_ERR_ARG, the message names the first such record, and the record is never used as an index.  (The records of a
 * set are checked the same way against the offsets of the call.)
 * Errors: KG_ERR_ARG for null pointers, reserved != 0, min_train_pairs < 0, n_seqs that is not the set's, decreasing offsets;
 * KG_ERR_LIMIT for 2^31 or more records or contigs, 2^32 or more pairs, 2^40 or more bytes; KG_ERR_BUSY while a kg_scan* is in
 * flight on the set's table; KG_ERR_NOMEM.  Zero records and zero sequences are valid.  Device allocations come from the
 * context's block cache, so KG_TEST_FAIL_ALLOC applies; everything but the new set's arrays is back in the cache on every path
 * out. */
#define KG_ORF_NONCODING   32u
typedef struct kg_coding_params { int32_t min_coding; int32_t reserved; int64_t min_train_pairs; } kg_coding_params;
typedef struct kg_coding_model { int64_t coding[4096]; int64_t background[4096]; } kg_coding_model;
typedef struct kg_coding_stats {
    int64_t scored;            /* records of the set                                      */
    int64_t training_records;
    int64_t training_pairs;    /* sum C                                                   */
    int64_t background;        /* sum B                                                   */
    int64_t noncoding;         /* records that rule 7 dropped                             */
    int32_t trained;           /* 0 untrained, 1 on its own set, 2 the caller's table     */
    float   ms_count;          /* device time of the counting passes                      */
    float   ms_score;          /* ... of the scores and the decision                      */
    int32_t reserved;
} kg_coding_stats;
/* table: int32[4096] in host memory, or NULL to train on the set; seq, offsets as kg_orfset_add_free takes them */
int kg_orfset_coding(kg_orfset *set, const kg_coding_params *p, const int32_t *table, const uint8_t *seq, int seq_on_device,
                     const int64_t *offsets, int64_t n_seqs, kg_orfset **out);
/* scores [first, first + count) into dst (host or device memory); KG_ERR_ARG on a set that has no scores */
int kg_orfset_coding_scores(const kg_orfset *s, int64_t first, int64_t count, int64_t *dst);
int kg_orfset_coding_stats(const kg_orfset *s, kg_coding_stats *out);
/* the counts the call made: all zero when the caller gave a table */
int kg_orfset_coding_model(const kg_orfset *s, kg_coding_model *out);
/* rule 5 on the host: table = int32[4096] */
int kg_coding_table(const kg_coding_model *model, int32_t *table);
/* caller-held host lists: orfs[n] in any order, seq and offsets[n_seqs + 1] on the host */
int kg_coding_counts_orfs(int device, const kg_orf *orfs, int64_t n, const uint8_t *seq, const int64_t *offsets, int64_t n_seqs,
                          kg_coding_model *out);
int kg_coding_score_orfs(int device, const int32_t *table, const kg_orf *orfs, int64_t n, const uint8_t *seq, const int64_t *offsets,
                         int64_t n_seqs, int64_t *scores);

/* ---- start codons: the start of every complete ORF chosen by a trained start-site score (kernels: kg_starts.hpp) ----
 *
 * The reference stops at the CALL lines; this rule is the project's own.  Integers only: the device's bytes equal a plain-loop
 * model's.  Rule 3 of the ORF section and rule 2 of the free-ORF section take the first start behind the upstream stop (the
 * longest ORF); this stage moves that start downstream where a score trained on the batch's own evidence ORFs says so.
 * Input: ORF records, the batch's sequence bytes and offsets[n_seqs + 1] exactly as the scan got them, a coding table
 * T (int32[4096], rule 5 of the coding section), parameters, optionally start weights, optionally a limit per record.
 * Codes, strands, codons, xs and the pairs of a record are those of the ORF and coding sections.
 *   1. Movable records.  A record is movable when kept != 0, start_codon != 0, flags & (KG_ORF_INTERRUPTED | KG_ORF_NONCODING)
 *      == 0 and n_res >= 1.  Every other record is copied unchanged.
 *   2. Candidates.  Codon k of a movable record is a candidate when 0 <= k < n_res, codon k is a start of the start_codons mask
 *      and k <= K.  k = 0, the present start, is always a candidate.  K = limit_i when a limit is given for the record and is
 *      >= 0; otherwise K = n_res - min_res, and when that is negative k = 0 is the only candidate.  min_res defaults to 100 (the
 *      free-ORF section's default) and start_codons to 7; both are this project's choices.
 *   3. Limit of an evidence ORF.  With a region set, record i < n_regions belongs to region i (the sets made by
 *      kg_orfset_add_free and kg_orfset_coding keep that alignment) and limit_i = ceil((xa - xs_i) / 3) with xa the region's
 *      strand-left of rule 2 of the ORF section: this is j0 - b, so a start is never moved behind the first codon inside the
 *      region.  It is KG_ERR_ARG, naming the first such record, when the region's seq or strand differs from the record's or
 *      when the value is negative; a set shorter than the region set is KG_ERR_ARG too.  Records behind the regions have no
 *      limit.  Without a region set no record has a limit: evidence ORFs are then bounded by min_res alone.
 *   4. Upstream window.  The 20 strand positions xs + 3k - 20 + i, 0 <= i < 20; c_i is the dna_code there; a position outside
 *      the contig has code 4.
 *   5. Score.  score(k) = Suf(k) + sum_i Wpos[i][c_i] + Wtype[type(k)], carried in int64.  Suf(k) is the sum of T[h] over pairs
 *      k .. n_res - 2; a pair with an unknown base adds 0.  A code 4 in the window adds 0.  type is 1 for ATG, 2 for GTG, 3 for
 *      TTG, by the codon's spelling (0 for the k = 0 of a caller-held record whose codon 0 is none of them; type 0 is never
 *      counted).  The chosen start is the candidate of largest score, on a tie the smallest k.
 *   6. Counts kg_start_model.  A training record is movable, not KG_ORF_FREE and not KG_ORF_PARTIAL5.  cand and type_cand count
 *      the window bases and the type of every candidate of every training record; they do not depend on the round.  chosen and
 *      type_chosen count those of each training record's currently chosen candidate.  Code 4 is never counted; index 0 of the
 *      type arrays stays 0.
 *   7. Weights kg_start_weights.  Host code, with the Lg of rule 5 of the coding section.
 *      pos[i][c] = Lg(chosen[i][c] + 1) - Lg(sum_c chosen[i][c] + 4) - Lg(cand[i][c] + 1) + Lg(sum_c cand[i][c] + 4);
 *      type[t] likewise over t = 1..3 with + 3 in place of + 4; type[0] = 0.
 *   8. Rounds.  Without caller's weights, round 0 has every record at k = 0; each of `rounds` rounds counts rule 6, makes the
 *      weights of rule 7 and re-chooses every movable record by rule 5, the training records included.  rounds defaults to 4
 *      and must be between 1 and 16.  The call is untrained when fewer than min_train_starts training records exist (default
 *      200, roughly eighty window parameters at a couple of records each); an untrained call changes no record, sets every
 *      shift to 0 and is not an error.  With caller's weights there is one choice pass and no counting; any int32 values are
 *      allowed.  The defaults are this project's choices.
 *   9. Result.  A moved record is one with chosen k > 0.  It gets left += 3k on '+' and right -= 3k on '-', n_res -= k, the new
 *      start_codon and the new flag KG_ORF_START_MOVED.  first_inner is -1 for every movable record and stays.  Its protein is
 *      the old protein from residue k on, with residue 0 set to 'M'; prot_start and the residues are rebuilt (only_kept zero
 *      lengths stay zero: those records are not movable).  When the set carries coding scores, a moved record's score becomes
 *      Suf(k), its rule-6 score on the new extent; no record is re-decided against min_coding.  Nothing else changes.
 *  10. Independence.  The output depends only on (records, bytes, offsets, parameters, tables, limits): not on launch geometry,
 *      tile size or batch neighbours.  All device sums are integer.
 * kg_orfset_starts gives a NEW ORF set in the given set's context, as kg_orfset_coding does; the given set stays valid and the
 * new one is freed before it.  The new set keeps the given set's coding scores (under rule 9), model and statistics.  Without
 * weights the call has one host wait per round (counts down, weights up).  kg_starts_orfs is the table-less twin for caller-held
 * host lists; its records are checked as kg_coding_score_orfs checks them.  model and stats may be NULL there.
 * kg_start_weights_from is host-only and uses no GPU; a negative count, or counts of one position (or of the types) whose sum
 * is 2^62 or more, are KG_ERR_ARG.
 * Errors: KG_ERR_ARG for null pointers (a null table too), reserved != 0, min_res < 1, start_codons outside 0..7, rounds outside
 * 1..16, min_train_starts < 0, n_seqs that is not the set's, a region set of another n_seqs, decreasing offsets and rule 3;
 * KG_ERR_LIMIT for 2^31 or more records or contigs, 2^32 or more codons, 2^40 or more bytes; KG_ERR_BUSY while a kg_scan* is in
 * flight on the set's table; KG_ERR_NOMEM.  Zero records and zero sequences are valid.  Device allocations come from the
 * context's block cache, so KG_TEST_FAIL_ALLOC applies; everything but the new set's arrays is back in the cache on every path
 * out. */
#define KG_ORF_START_MOVED 64u
typedef struct kg_start_params { int32_t min_res; int32_t start_codons; int32_t rounds; int32_t reserved; int64_t min_train_starts; } kg_start_params;
typedef struct kg_start_model { int64_t chosen[20][4]; int64_t cand[20][4]; int64_t type_chosen[4]; int64_t type_cand[4]; } kg_start_model;
typedef struct kg_start_weights { int32_t pos[20][4]; int32_t type[4]; } kg_start_weights;
typedef struct kg_start_stats {
    int64_t movable;
    int64_t training_records;
    int64_t candidates;
    int64_t moved;
    int32_t rounds_run;        /* 0 untrained, 1 with the caller's weights                 */
    int32_t trained;           /* 0 untrained, 1 on its own set, 2 the caller's weights    */
    float   ms_count;          /* device time of the candidate list and the counts         */
    float   ms_choose;         /* ... of the choices, the move and the proteins            */
} kg_start_stats;
/* table: int32[4096] in host memory; weights: NULL to train on the set; regions: NULL, or the region set the ORFs were made
   from (rule 3); seq, offsets as kg_orfset_add_free takes them */
int kg_orfset_starts(kg_orfset *set, const kg_start_params *p, const int32_t *table, const kg_start_weights *weights,
                     const kg_regionset *regions, const uint8_t *seq, int seq_on_device, const int64_t *offsets, int64_t n_seqs,
                     kg_orfset **out);
/* the shift in codons of records [first, first + count) into dst (host or device memory); KG_ERR_ARG on a set that is not from
   kg_orfset_starts */
int kg_orfset_start_shifts(const kg_orfset *s, int64_t first, int64_t count, int32_t *dst);
int kg_orfset_start_stats(const kg_orfset *s, kg_start_stats *out);
/* the counts of the last round: all zero when the caller gave weights or the call is untrained */
int kg_orfset_start_model(const kg_orfset *s, kg_start_model *out);
/* rule 7 on the host */
int kg_start_weights_from(const kg_start_model *model, kg_start_weights *weights);
/* caller-held host lists: orfs[n] in any order, limits int32[n] (-1: none) or NULL, seq and offsets[n_seqs + 1] on the host;
   out[n] and shifts[n] are written */
int kg_starts_orfs(int device, const kg_start_params *p, const int32_t *table, const kg_start_weights *weights, const kg_orf *orfs,
                   int64_t n, const int32_t *limits, const uint8_t *seq, const int64_t *offsets, int64_t n_seqs, kg_orf *out,
                   int32_t *shifts, kg_start_model *model, kg_start_stats *stats);

/* ---- a gene set: the non-overlapping selection among regions or ORFs (kernels: kg_select.hpp) ----
 *
 * The reference stops at the CALL lines; this rule is the project's own.
 * Input: n candidates, index-aligned with a region set or an ORF set.  Each candidate has seq, left <= right (0-based,
 * inclusive, on the contig as given), score, and eligible.  eligible is the record's kept.
 *   1. Length and overlap.  len = right - left + 1.  Two candidates of the same seq overlap by
 *      ov = min(right_i, right_j) - max(left_i, left_j) + 1, when that is positive.
 *   2. Conflict.  Two eligible candidates conflict iff ov > max_overlap or 100 * ov > max_overlap_pct * min(len_i, len_j).
 *      The arithmetic is int64.  Strand and function play no part: two functions on one ORF conflict, and so do genes on
 *      opposite strands.  Candidates of different contigs never conflict.  A non-eligible candidate conflicts with nothing.
 *   3. Strength.  This is a total order: larger score first, then larger len, then smaller index in the set.
 *   4. Selection.  Going through the eligible candidates from strongest to weakest, a candidate is selected iff it conflicts
 *      with no stronger selected candidate.  This is the greedy fixed point.  It is unique and it is what the model computes
 *      with a plain loop.  It is not one-shot dominance: a candidate that conflicts only with a stronger candidate that itself
 *      lost is selected.
 *   5. Record.  kg_selection is 8 bytes: { int32 state; int32 by; }.  state is 0 for not eligible, 1 for selected, 2 for
 *      overlapped.  by is the smallest set index among the selected, stronger candidates the overlapped one conflicts with,
 *      and -1 otherwise.
 *   6. Parameters.  kg_select_params { max_overlap, max_overlap_pct, reserved }.  Both values must be at least 0,
 *      max_overlap_pct must be at most 100, and reserved must be 0.  Anything else is KG_ERR_ARG.  The defaults are 60
 *      nucleotides and 50 percent.  They are this project's choice.
 *   7. Independence.  The output depends only on the candidate list and the parameters.  It does not depend on launch
 *      geometry, on the number of rounds, or on batch neighbours.
 *   8. Errors.  KG_ERR_ARG for null pointers.  KG_ERR_ARG for a caller-held candidate with seq outside [0, n_seqs), left < 0 or
 *      right < left: the message names the first such candidate, and the candidate is never used as an index.  KG_ERR_LIMIT
 *      for 2^31 or more candidates, or 2^31 or more overlapping pairs (pairs of eligible candidates of one contig with ov > 0,
 *      conflicting or not): this is found from the counts, before the pair list is allocated.  KG_ERR_BUSY while a kg_scan* is
 *      in flight on the set's table.  KG_ERR_NOMEM.  Zero candidates are valid.
 * Device allocations come from the block cache of the set's context (a table-less one for kg_select_intervals), so
 * KG_TEST_FAIL_ALLOC applies; everything but the selection array is back in the cache on every path out.  A select set made
 * from a region set or an ORF set holds a block of that set's context and must be freed before it. */
#define KG_SEL_NOT_ELIGIBLE 0
#define KG_SEL_SELECTED     1
#define KG_SEL_OVERLAPPED   2
typedef struct kg_select_params { int32_t max_overlap; int32_t max_overlap_pct; int32_t reserved; } kg_select_params;
typedef struct kg_interval {     /* 20 B */
    int32_t  seq;
    int32_t  left;         /* 0-based, inclusive                                        */
    int32_t  right;
    int32_t  score;
    int32_t  eligible;     /* 0: takes no part                                          */
} kg_interval;
typedef struct kg_selection {    /* 8 B */
    int32_t  state;        /* KG_SEL_*                                                  */
    int32_t  by;           /* overlapped: the winner's index in the set, else -1        */
} kg_selection;
typedef struct kg_select_stats {
    int64_t candidates, eligible, selected, overlapped;
    int64_t pairs;         /* overlapping pairs of eligible candidates                  */
    int64_t conflicts;     /* ... of which conflict (rule 2)                            */
    int32_t rounds;        /* rounds until no candidate was undecided                   */
    float   ms;            /* device time of the call's kernels                         */
} kg_select_stats;
typedef struct kg_selectset kg_selectset;
/* interval = the region's left..right, eligible = its kept; selection[i] belongs to region[i] */
int kg_regionset_select(kg_regionset *set, const kg_select_params *p, kg_selectset **out);
/* interval = the ORF's left..right, eligible = its kept; selection[i] belongs to orf[i] */
int kg_orfset_select(kg_orfset *set, const kg_select_params *p, kg_selectset **out);
/* caller-held host list iv[n] in any order; selection[i] belongs to iv[i] */
int kg_select_intervals(int device, const kg_select_params *p, const kg_interval *iv, int64_t n, int64_t n_seqs, kg_selectset **out);
int64_t kg_selectset_count(const kg_selectset *s);
/* device array of kg_selectset_count(s) kg_selection records, valid until kg_selectset_free */
const kg_selection *kg_selectset_device(const kg_selectset *s);
/* records [first, first + count) into dst (host or device memory) */
int kg_selectset_copy(const kg_selectset *s, int64_t first, int64_t count, kg_selection *dst);
int kg_selectset_stats(const kg_selectset *s, kg_select_stats *out);
void kg_selectset_free(kg_selectset *s);

/* ---- whose contig: every OTU vote of a sequence tallied, one OTU per sequence, the sample's bins (kernels: kg_votes.hpp) ----
 *
 * The reference votes for OTUs inside processSetOfHits (KGJ:405-437) and keeps the tally in a buffer of KG_OI_BUFSZ slots
 * whose last slot every further OTU overwrites (KGJ:432-437); it stops at the OTU-COUNTS line.  Steps 1 and 2 are the
 * reference's own vote without that buffer; everything from step 3 on is this project's own.  Integers only.
 * Input: the hit records hits[] in (container, from0InProt) order with container_hit_start, the event byte of every hit,
 * the CALL records with container_call_start, per = the containers of one sequence (6 for DNA, 1 for -a), and the sequence
 * lengths L_s = offsets[s+1] - offsets[s].
 *   1. Votes.  Let c_0 .. c_{m-1} be the CALLs of hit h's container in emission order.  For records that come from a scan
 *      their start values are strictly ascending; for caller-held lists a container where they are not is an error.  Let k be
 *      the largest index with c_k.start <= h.from0InProt.  h is a vote iff its event byte has KG_EV_ACCEPTED, k exists,
 *      c_k.fI == h.fI and h.from0InProt + (KG_K - 1) <= c_k.end (int64).  The vote belongs to CALL c_k and goes to OTU h.oI of
 *      sequence container / per.  These are exactly the hits KGJ:405-437 feeds into oICounts: the members 0 .. lastHit of a
 *      list that printed a CALL, with the CALL's function -- so the votes of a CALL number its count.  A voting hit with
 *      oI < 0 is KG_ERR_ARG, and the message names the hit (a hit that does not vote may carry any oI).
 *   2. Tally.  For each (sequence, OTU) pair that has a vote: votes = the number of its votes, n_calls = the number of
 *      distinct CALLs they belong to.
 *   3. Order.  A sequence's pairs are ordered by votes descending, then oI ascending.  The pairs of all sequences lie end to
 *      end in sequence order (kg_otu_vote, 16 B), with vote_start[n_seqs + 1] (int64) so that a sequence's pairs are one slice.
 *   4. Class (kg_otu_class, 40 B, one per sequence): total = the sum of its votes, which must be below 2^31, else
 *      KG_ERR_LIMIT naming the sequence; total_calls = the CALLs in its containers; n_otus = its pairs; otu / votes / n_calls
 *      = its first pair, second_otu / second_votes = its second (-1 / 0 when there is none);
 *      assigned = 1 iff votes >= min_votes and n_calls >= min_calls and 100 * votes >= min_share_pct * total (int64) -- and
 *      there is a vote at all.  Without a vote otu = second_otu = -1 and everything else is 0 but total_calls.
 *   5. Bins (kg_otu_bin, 32 B): for each OTU at least one sequence is assigned to, n_seqs = those sequences, length = the
 *      int64 sum of their lengths, votes and n_calls = the int64 sums of their first-pair values.  Bins are ordered by length
 *      descending, then votes descending, then oI ascending.
 *   6. Parameters kg_vote_params { min_votes, min_share_pct, min_calls, reserved }: min_votes >= 0, 0 <= min_share_pct <= 100,
 *      min_calls >= 0, reserved 0, else KG_ERR_ARG.  Defaults (this project's choice): 10, 50 and 1.
 *   7. Independence.  The output depends only on the records and the lengths: not on launch geometry, tile sizes or batch
 *      neighbours.  A sequence's pairs and class are the same in whatever batch it sits; the bins of two batches add up.
 * Errors: KG_ERR_ARG for a KG_F_SKIP_AGGREGATE result, null pointers, per outside {1, 6}, decreasing container_hit_start,
 * container_call_start or offsets (or starts that do not begin at 0), a hit or CALL whose container field is not the
 * container whose slice it lies in, hits of a container not in non-decreasing from0InProt order, CALL starts of a container
 * that are not strictly ascending, a negative oI on a voting hit -- each message names the first offender; KG_ERR_LIMIT for
 * 2^32 or more hits, CALLs or pairs, 2^31 or more sequences, a sequence total (or CALL count) of 2^31 or more; KG_ERR_BUSY
 * while a kg_scan* is in flight on the result's table; KG_ERR_NOMEM.  A bad record is clamped before it is used as an index.
 * Zero hits, zero CALLs and zero sequences are valid inputs.
 * Device allocations come from the table's block cache (a table-less context for kg_otu_votes_hits), so KG_TEST_FAIL_ALLOC
 * applies; everything but the set's four arrays is back in the cache when the call returns.  A set made by
 * kg_result_otu_votes holds blocks of the result's table (kg_table_live_device_bytes counts them) and must be freed before
 * that table is closed. */
typedef struct kg_vote_params { int32_t min_votes, min_share_pct, min_calls, reserved; } kg_vote_params;
typedef struct kg_otu_vote {     /* 16 B */
    int32_t  seq;
    int32_t  oI;
    int32_t  votes;
    int32_t  n_calls;      /* distinct CALLs the votes belong to                        */
} kg_otu_vote;
typedef struct kg_otu_class {    /* 40 B */
    int32_t  otu;          /* the first pair's OTU, -1 without a vote                   */
    int32_t  assigned;     /* rule 4                                                    */
    int32_t  votes;        /* the first pair's                                          */
    int32_t  total;        /* all votes of the sequence                                 */
    int32_t  n_calls;      /* the first pair's                                          */
    int32_t  total_calls;  /* CALLs in the sequence's containers                        */
    int32_t  n_otus;       /* pairs of the sequence                                     */
    int32_t  second_otu;   /* the second pair's OTU, -1 when there is none              */
    int32_t  second_votes;
    int32_t  reserved;
} kg_otu_class;
typedef struct kg_otu_bin {      /* 32 B */
    int32_t  oI;
    int32_t  n_seqs;       /* sequences assigned to the OTU                             */
    int64_t  length;       /* ... the sum of their lengths                              */
    int64_t  votes;        /* ... of their first-pair votes                             */
    int64_t  n_calls;      /* ... of their first-pair n_calls                           */
} kg_otu_bin;
typedef struct kg_vote_stats {
    int64_t hits, accepted, votes, pairs, seqs_with_votes, assigned, bins;
    int64_t assigned_length, total_length;
    float   ms;            /* device time of the call's kernels                         */
    int32_t reserved;
} kg_vote_stats;
typedef struct kg_voteset kg_voteset;
/* a DNA or -a result of kg_scan* / kg_aggregate_hits plus the host offsets[n_seqs + 1] the scan was given */
int kg_result_otu_votes(kg_result *r, const kg_vote_params *p, const int64_t *offsets, kg_voteset **out);
/* caller-held host lists: hits[container_hit_start[n_seqs * per]] and hit_events (one byte per hit),
   calls[container_call_start[n_seqs * per]], both start arrays of n_seqs * per + 1 entries, offsets[n_seqs + 1] */
int kg_otu_votes_hits(int device, const kg_vote_params *p, const kg_hit *hits, const int64_t *container_hit_start,
                      const uint8_t *hit_events, const kg_call *calls, const int64_t *container_call_start, int64_t n_seqs,
                      int32_t per, const int64_t *offsets, kg_voteset **out);
/* the pairs (kg_otu_vote records) and the bins of the set; it holds one kg_otu_class per sequence */
int64_t kg_voteset_count(const kg_voteset *s);
int64_t kg_voteset_bins(const kg_voteset *s);
/* records [first, first + count) into dst (host or device memory) */
int kg_voteset_copy_votes(const kg_voteset *s, int64_t first, int64_t count, kg_otu_vote *dst);
int kg_voteset_copy_classes(const kg_voteset *s, int64_t first, int64_t count, kg_otu_class *dst);
int kg_voteset_copy_bins(const kg_voteset *s, int64_t first, int64_t count, kg_otu_bin *dst);
/* vote_start[n_seqs + 1] into dst (host or device memory): sequence s owns pairs [vote_start[s], vote_start[s+1]) */
int kg_voteset_seq_start(const kg_voteset *s, int64_t *dst);
int kg_voteset_stats(const kg_voteset *s, kg_vote_stats *out);
void kg_voteset_free(kg_voteset *s);

/* ---- whose contig, without a vote: tetranucleotide composition against the voted contigs' (kernels: kg_compose.hpp) ----
 *
 * The reference stops at the OTU-COUNTS line; this stage is this project's own.  A genome's tetranucleotide usage is shared
 * by its contigs whether or not a protein on them is known, and the contigs the votes stage assigned are a labelled training
 * set.  Integers only.  Input: the batch's bytes exactly as a scan gets them, offsets[n_seqs + 1], labels[n_seqs] (a value
 * >= 0 is the bin of a training contig, -1 means unlabelled, a value below -1 is KG_ERR_ARG naming the first such contig;
 * NULL = all -1), the parameters and optionally a caller's model.
 *   1. Tetramer index.  Four bases of dna_code < 4 give t = sum b_i * 4^(3-i), 0 <= t < 256.  A tetramer with a base of code 4
 *      does not exist, a tetramer never spans two contigs, a contig with L < 4 has none.
 *   2. Contig counts N_s[256] (int32).  F_s[t] = the forward tetramers of contig s with index t; N_s[t] = F_s[t] + F_s[rc(t)],
 *      where rc complements every 2-bit digit and reverses their order: both strands, so a contig and its reverse complement
 *      have the same N.  The 16 palindromic tetramers count twice (stated, not repaired).  windows_s = sum_t N_s[t].  A contig
 *      with L >= 2^30 is KG_ERR_LIMIT.
 *   3. Label rows.  For every distinct label b >= 0, in ascending order, C_b[t] = the int64 sum of N_s[t] over the contigs
 *      with label b, SC_b = sum_t C_b[t].  The background row G[t] = the sum of N_s[t] over all contigs, labelled or not.
 *   4. Models.  A label row is a model when SC_b >= min_train (windows); models keep the ascending label order and are indexed
 *      0 .. M-1, the background is always present as index M.  A caller's model is a set of rows (labels >= 0 and strictly
 *      ascending, counts >= 0, every row sum < 2^62, the background last; anything else is KG_ERR_ARG): every one of its rows
 *      is a model, min_train is ignored, and the call makes no label rows (its rows and its background are all zero).
 *   5. Weights (host code, the Lg of the coding section): W_m[t] = Lg(C_m[t] + 1) - Lg(SC_m + 256), int32, the same for the
 *      background row.
 *   6. Scores.  S[s][m] = sum_t N_s[t] * W_m[t] (int64, exact; |S| < 2^45) for every contig and every m in 0 .. M.
 *   7. Order.  A contig's rows are ordered by score descending, then m ascending, so on a tie a bin comes before the
 *      background; best and second are the first two.  With M = 0 there is only the background: best = second = -1,
 *      score_second = score_best, never decided.
 *   8. Decision.  decided = 1 iff L_s >= min_len and best is a model (not the background) and S_best - S_second >= min_margin.
 *      Defaults (this project's choice): min_len = 1500 nt, min_margin = 2560 (ten bits in Lg's units of 1/256 bit),
 *      min_train = 200000 windows (about 100 kbp).
 *   9. Labelled contigs are scored and decided like any other; their own tetramers are in their bin's model (stated, not
 *      corrected).  A labelled contig that is decided for another bin is a conflict: counted, nothing else.
 *  10. Independence.  The per-contig outputs depend only on that contig's bytes and the models; the label rows and the
 *      background of two batches add up; nothing depends on launch geometry, tile sizes or batch neighbours.
 * kg_comp_class: label = the contig's label as given, best / second = label values (-1 = the background).  keep_scores != 0
 * keeps the matrix S (int64 [n_seqs][M + 1]) for kg_compset_copy_scores; otherwise it does not exist.
 * Errors: KG_ERR_ARG for null pointers, reserved fields, negative parameters, decreasing offsets, a label below -1, a bad
 * model (model_labels and model_counts are both given or both NULL) -- each message names the first offender; KG_ERR_LIMIT for
 * 2^31 or more sequences, 2^40 or more bytes, a contig of 2^30 or more nucleotides, more than 2^20 label rows or model rows,
 * a kept score matrix of 2^40 bytes or more; KG_ERR_NOMEM.  A bad label is never used as an index.  Zero sequences, zero
 * labels and zero models are valid.  The call owns a table-less context as kg_otu_votes_hits does, so KG_TEST_FAIL_ALLOC
 * applies; everything but the set's arrays is back in the cache on every path out.  One host wait in the middle (the rows come
 * down, W is made on the host and goes up); none with a caller's model. */
typedef struct kg_comp_params { int32_t min_len; int32_t min_margin; int64_t min_train; int32_t keep_scores; int32_t reserved; } kg_comp_params;
typedef struct kg_comp_class {   /* 40 B */
    int32_t  label, best, second, decided;
    int64_t  windows, score_best, score_second;
} kg_comp_class;
typedef struct kg_comp_stats {
    int64_t seqs, labelled, label_rows, models, windows, decided, decided_unlabelled, conflicts;
    float   ms_count, ms_score;     /* device time: counts, fold and label rows; scores and decisions */
} kg_comp_stats;
typedef struct kg_compset kg_compset;
/* model_counts: (n_models + 1) * 256 counts, the background row last */
int kg_contigs_compose(int device, const kg_comp_params *p, const uint8_t *seq, int seq_on_device, const int64_t *offsets,
                       int64_t n_seqs, const int32_t *labels, const int32_t *model_labels, const int64_t *model_counts,
                       int64_t n_models, kg_compset **out);
/* the label rows the call made, and the models it scored with */
int64_t kg_compset_rows(const kg_compset *s);
int64_t kg_compset_models(const kg_compset *s);
/* records [first, first + count) into dst (host or device memory) */
int kg_compset_copy_classes(const kg_compset *s, int64_t first, int64_t count, kg_comp_class *dst);
/* N of contigs [first, first + count): int32[256] each */
int kg_compset_copy_counts(const kg_compset *s, int64_t first, int64_t count, int32_t *dst);
/* label rows [first, first + count): their labels and their int64[256] counts (either dst may be NULL) */
int kg_compset_copy_rows(const kg_compset *s, int64_t first, int64_t count, int32_t *labels_dst, int64_t *counts_dst);
/* G: int64[256] */
int kg_compset_background(const kg_compset *s, int64_t *dst);
int kg_compset_model_labels(const kg_compset *s, int64_t first, int64_t count, int32_t *dst);
/* S of contigs [first, first + count): int64[M + 1] each; KG_ERR_ARG when the call did not keep the matrix */
int kg_compset_copy_scores(const kg_compset *s, int64_t first, int64_t count, int64_t *dst);
int kg_compset_stats(const kg_compset *s, kg_comp_stats *out);
void kg_compset_free(kg_compset *s);

/* ---- genes by homology: a translated search of contigs whose hits are CALL records (kernels: kg_evidence.hpp) ----
 *
 * The reference stops at the CALL lines, and its CALLs come from the signature table; this rule is the project's own.  Integers
 * only.  It gives the region, ORF, repair, coding, start and selection stages above CALLs made from protein homology instead: a
 * caller with contigs and a kg_searchdb of labelled proteins, and no table, locates genes.  fI is a target (or the function
 * target_fn gives it) where the signature path has a function index; everything behind the CALL list is unchanged.
 *   1. Fragments.  The fragments of a batch of contigs are exactly the records, prot_start and residues of kg_orfs_free with
 *      kg_free_params { min_res, start_codons = 0, 0 }, in that call's order: every stop-to-stop run of the six frames (a run
 *      that reaches a contig's end included) of at least min_res residues, by contig, strand, frame and increasing first codon,
 *      the scan's container order.  Fragment q is query q of the search.  For a fragment F on a contig of length L,
 *      b = (x - F.frame) / 3 with x = F.left on '+' and x = L - 1 - F.right on '-': the fragment's first codon in its frame, so
 *      residue i of its protein is codon b + i (with start_codons = 0 no residue is rewritten to 'M').
 *   2. Search.  The hit records, hit_start, paths (and ops, ungapped records and band statistics when asked for) are byte for
 *      byte those of kg_searchdb_search_device on the fragments' proteins as queries, with the same options and `trace` as
 *      given, except that trace & 3 == 0 means KG_TRACE_HITS: a CALL needs the path's start.
 *   3. CALLs.  Hit record r with path p, of fragment F, becomes a CALL iff r.status == 0 (a hit), r.rank < max_hits and
 *      p.status == 0 (traced).  The first of the three tests that fails names the drop: status, rank, untraced.  The CALL:
 *      container = 6 * F.seq + 3 * F.strand + F.frame; start = b + p.start_a; end = b + r.end_query; count = r.score;
 *      fI = target_fn ? target_fn[r.target] : r.target; weightedHits = (float) r.score.  CALLs keep the hit records' order,
 *      which is the fragments' order, so containers are non-decreasing as kg_regions_calls wants.  call_hit[k] is the hit
 *      record of CALL k.
 *   4. Rule 1 of the regions section holds for every such CALL.  F is codons b .. b + n_res - 1 of frame f, all of them whole
 *      codons inside the contig (n_f counts whole codons only), and a traced path has 0 <= start_a <= end_query <= n_res - 1.
 *      So x0 = f + 3 (b + start_a) >= 0, x0 <= x1, and x1 = f + 3 (b + end_query) + 2 <= f + 3 (b + n_res - 1) + 2 <= L - 1.
 *      Two halves of a frameshifted gene hit one target in two frames of one strand: one group, one multi-frame region when
 *      they lie within merge_gap, and kg_regionset_repair joins them.
 *   5. Nothing depends on launch geometry or batch neighbours: a contig's fragments, a fragment's hit records and a record's
 *      CALL depend on the contig, the database and the parameters alone (`query`, call_hit and seq aside, which count within
 *      the batch).
 * Parameters kg_translate_params { min_res (>= 1, default 30), max_hits (1..64, default 1), reserved[2] == 0 }; anything else
 * is KG_ERR_ARG.  Both defaults are this project's choice and are not tuned: 30 residues is about the shortest piece the 8-mer
 * prefilter and a ratio test against the fragment can place, and one hit per fragment keeps one gene from being called under
 * every paralogue's name.  target_fn is a host int32[n_db] or NULL; a negative value is KG_ERR_ARG (the message names the
 * first).
 * kg_contigs_search_translated: seq, the batch's bytes exactly as a scan gets them, in device memory when seq_on_device != 0;
 * offsets[n_seqs + 1], host.  The other arguments are kg_searchdb_search's and their KG_ERR_ARG words are its words.
 * The fragments' residues go from the ORF set into the handle's room device to device; only prot_start travels to the host,
 * because the search takes host offsets.
 * Limits (KG_ERR_LIMIT): a fragment of 2^24 residues or more (a long run of N is a run), as the search has it; fragments whose
 * residues exceed the handle's query room ("... residues of queries do not fit the room of ... residues"; kg_searchdb_reserve
 * regrows it).  2 * (the nucleotides of the batch) is an upper bound on the fragments' residues: six frames of a third each.
 * A caller can reserve that beforehand.  Also the limits of kg_orfs_free and of the search, 2^32 or more hit records, and so
 * many contigs that a container index reaches 2^32.
 * KG_ERR_BUSY, KG_ERR_NOMEM and KG_TEST_FAIL_ALLOC behave as in kg_searchdb_search; the hook applies to every device allocation
 * of the three stages, each counted from 1.  After any failure the handle is usable and its live bytes are what they were.
 * Zero contigs, zero fragments, zero hit records and zero CALLs are valid.
 * The kg_evidence lends out the fragments as an ordinary kg_orfset and the hits as an ordinary kg_hitset, on which every getter
 * works (kg_hitset_db_stats too); both are valid until kg_evidence_free and must not be freed by the caller.  Its own arrays
 * live in the fragments' context, not in the handle's: an evidence may outlive the kg_searchdb. */
typedef struct kg_translate_params { int32_t min_res; int32_t max_hits; int32_t reserved[2]; } kg_translate_params;
typedef struct kg_translate_stats {   /* 72 B */
    int64_t fragments;
    int64_t fragment_residues;
    int64_t records;           /* hit records of the search                                */
    int64_t calls;
    int64_t dropped_status;    /* records that are not hits (below, skipped)               */
    int64_t dropped_rank;      /* hits of rank >= max_hits                                 */
    int64_t dropped_untraced;  /* hits of a kept rank whose path is over max_trace_cells   */
    float   ms_fragments;      /* device time of kg_orfs_free's kernels                    */
    float   ms_search;         /* ... of the search and its trace                          */
    float   ms_calls;          /* ... of flag, prefix sum and emit                         */
    float   ms_total;          /* the three together                                       */
} kg_translate_stats;
typedef struct kg_evidence kg_evidence;
int kg_contigs_search_translated(kg_searchdb *db, const kg_search_params *p, const kg_align_params *align,
                                 const kg_translate_params *tp, const uint8_t *seq, int seq_on_device, const int64_t *offsets,
                                 int64_t n_seqs, int64_t max_windows, int64_t max_pairs, int trace, int64_t max_trace_cells,
                                 const kg_mask_params *query_mask, const kg_ungapped_params *ungapped, const kg_band_params *band,
                                 const int32_t *target_fn, kg_evidence **out);
const kg_orfset *kg_evidence_fragments(const kg_evidence *e);
const kg_hitset *kg_evidence_hits(const kg_evidence *e);
int64_t kg_evidence_calls_count(const kg_evidence *e);
/* records [first, first + count) into dst (host or device memory) */
int kg_evidence_calls_copy(const kg_evidence *e, int64_t first, int64_t count, kg_call *dst);
/* device array of kg_evidence_calls_count(e) kg_call records, valid until kg_evidence_free: what kg_regionset_repair takes
   with calls_on_device = 1 */
const kg_call *kg_evidence_calls_device(const kg_evidence *e);
int kg_evidence_call_hits_copy(const kg_evidence *e, int64_t first, int64_t count, int64_t *dst);
int kg_evidence_stats(const kg_evidence *e, kg_translate_stats *out);
void kg_evidence_free(kg_evidence *e);

/* ---- signature and homology evidence in one run: the database fills what the table left unnamed (kernels: kg_residual.hpp) ----
 *
 * This rule is the project's own.  Integers only.  A caller with a signature table and a kg_searchdb has two sources of CALLs;
 * this call takes the CALLs of the first, searches only the fragments they do not explain, and hands back one CALL list.
 * Inputs: a batch of contigs (seq, offsets); a kg_searchdb; the signature CALLs of that batch in non-decreasing container order,
 * either the CALLs of a DNA kg_result or a caller-held array in host or device memory; target_fn, host int32[n_db], required
 * here (NULL is KG_ERR_ARG): the two kinds of CALL share one fI space, and only the caller can build that.
 *   1. Fragments.  Exactly those of kg_contigs_search_translated: the records, prot_start and residues of kg_orfs_free with
 *      { min_res, start_codons = 0 }.  For a fragment F, c(F) = 6 F.seq + 3 F.strand + F.frame, and b(F) as in that rule:
 *      (x - F.frame) / 3 with x = F.left on '+' and x = L - 1 - F.right on '-'.  F covers codons b .. b + n_res - 1 of its
 *      container.  Fragments are sorted by (c, b) and disjoint within a container.
 *   2. Explained.  A signature CALL s touches F iff s.container == c(F), s.start <= b(F) + F.n_res - 1 and s.end >= b(F); a CALL's
 *      start and end are residues of its frame, which are the same codon indices (rule 1 of the regions section).  explain[F] is
 *      an int64: the sum of s.count over the CALLs that touch F.  F is explained iff explain[F] >= explain_min.  A CALL may touch
 *      several fragments, because a CALL can span a stop; it explains each of them.  A CALL that touches no listed fragment
 *      changes nothing (it may lie in a run shorter than min_res).
 *   3. Searched fragments.  The fragments that are not explained, in fragment order.  Their kg_orf records, a new prot_start and
 *      their residues are compacted on the device into an ordinary, lendable ORF set in the fragments' context (its statistics
 *      hold orfs and residues alone).  Searched fragment q is query q; searched[q] is its index among all fragments.
 *   4. Search.  The hit records, hit_start, paths (and ops, ungapped records and band statistics when asked for) are byte for
 *      byte those of kg_searchdb_search_device on the searched fragments' proteins, with the same options; trace & 3 == 0 reads
 *      as KG_TRACE_HITS.  With zero searched fragments the search is not launched: the hit set is a valid empty one (zero
 *      queries, zero records, hit_start = {0}, statistics zero but for `targets`), and ms_search is 0.
 *   5. Homology CALLs.  The CALLs of rule 3 of "genes by homology" over the searched fragments' records and these hits (a hit's
 *      `query` indexes the compacted records).  A CALL whose count < min_db_count is then left out and counted.
 *   6. Merged list.  By container; inside a container the signature CALLs come first in their given order, then the homology
 *      CALLs in theirs.  Three arrays run parallel to it: call_kind[k], 0 for signature and 1 for homology; call_source[k], for a
 *      signature CALL its index in the signature list, for a homology CALL its index in the homology list before the
 *      min_db_count cut; call_hit[k], the hit record, or -1 for a signature CALL.  The list's containers are non-decreasing, as
 *      kg_regions_calls requires.  Counts stay in their own units, k-mer hits for a signature CALL and alignment score for a
 *      homology CALL, so the score of a region that holds both kinds is the plain sum of the two units: it ranks such a region
 *      against others only roughly.  A common unit is out of scope.
 *   7. Nothing depends on launch geometry or batch neighbours: explain[] is a sum of integers, and every compacted byte and
 *      every merged CALL has one writer.
 * Parameters kg_residual_params { explain_min (>= 1, default 1: any CALL explains, a scan's CALLs already have count >= minHits),
 * min_db_count (>= 0, default 0), reserved == 0 }; anything else is KG_ERR_ARG.  Both defaults are this project's choice and are
 * not tuned.
 * The caller-held list (KG_ERR_ARG, the message names the first offender as "CALL N: ..."): a container below its
 * predecessor's; a container >= 6 * n_seqs; a negative count; start > end; a record outside its contig.  A bad record is clamped
 * before it indexes anything and marks nothing.  kg_result_search_residual reads the result's device CALLs where they lie and
 * gives exactly the bytes of kg_contigs_search_residual on kg_result_calls(r); KG_ERR_ARG for a protein (-a) or
 * KG_F_SKIP_AGGREGATE result, for a result on another device than the index, or of another number of sequences than n_seqs;
 * KG_ERR_BUSY while a scan is in flight on its table.
 * Limits, KG_ERR_NOMEM, KG_TEST_FAIL_ALLOC and "after any failure the handle's live bytes are what they were" are those of
 * kg_contigs_search_translated; the room check counts the searched fragments' residues only, before they are copied.
 * The kg_evidence: kg_evidence_calls_* and kg_evidence_calls_device give the merged list, kg_evidence_call_hits_copy the hit
 * record or -1, kg_evidence_fragments all fragments, kg_evidence_hits the hit set of the searched ones.  kg_translate_stats keeps
 * its meaning: fragments counts all of them, calls the homology CALLs before the min_db_count cut, ms_total excludes the new
 * stages.  The getters below are KG_ERR_ARG (or NULL) on an evidence of kg_contigs_search_translated. */
typedef struct kg_residual_params { int64_t explain_min; int32_t min_db_count; int32_t reserved; } kg_residual_params;
typedef struct kg_residual_stats {   /* 80 B */
    int64_t sig_calls;
    int64_t explained;           /* fragments with explain >= explain_min                     */
    int64_t explained_residues;
    int64_t searched;            /* the others: the queries                                   */
    int64_t searched_residues;
    int64_t db_calls;            /* homology CALLs before the min_db_count cut                */
    int64_t dropped_min_count;
    int64_t merged;              /* sig_calls + db_calls - dropped_min_count                  */
    float   ms_explain;          /* device time of keys, mark, choose and the two sums        */
    float   ms_compact;          /* ... of the layout and the residues' copy                  */
    float   ms_merge;            /* ... of keep, its sum and the merge                        */
    float   ms_total;            /* kg_translate_stats.ms_total and the three together        */
} kg_residual_stats;
int kg_contigs_search_residual(kg_searchdb *db, const kg_search_params *p, const kg_align_params *align,
                               const kg_translate_params *tp, const uint8_t *seq, int seq_on_device, const int64_t *offsets,
                               int64_t n_seqs, int64_t max_windows, int64_t max_pairs, int trace, int64_t max_trace_cells,
                               const kg_mask_params *query_mask, const kg_ungapped_params *ungapped, const kg_band_params *band,
                               const int32_t *target_fn, const kg_call *sig_calls, int calls_on_device, int64_t n_sig_calls,
                               const kg_residual_params *rp, kg_evidence **out);
int kg_result_search_residual(kg_result *r, kg_searchdb *db, const kg_search_params *p, const kg_align_params *align,
                              const kg_translate_params *tp, const uint8_t *seq, int seq_on_device, const int64_t *offsets,
                              int64_t n_seqs, int64_t max_windows, int64_t max_pairs, int trace, int64_t max_trace_cells,
                              const kg_mask_params *query_mask, const kg_ungapped_params *ungapped, const kg_band_params *band,
                              const int32_t *target_fn, const kg_residual_params *rp, kg_evidence **out);
const kg_orfset *kg_residual_searched_fragments(const kg_evidence *e);
/* searched[first, first + count): every query's index among the fragments */
int kg_residual_searched_copy(const kg_evidence *e, int64_t first, int64_t count, int64_t *dst);
/* explain[first, first + count), one per fragment */
int kg_residual_explain_copy(const kg_evidence *e, int64_t first, int64_t count, int64_t *dst);
int kg_residual_call_kinds_copy(const kg_evidence *e, int64_t first, int64_t count, uint8_t *dst);
int kg_residual_call_sources_copy(const kg_evidence *e, int64_t first, int64_t count, int64_t *dst);
int kg_residual_stats_of(const kg_evidence *e, kg_residual_stats *out);

/* the resident 24-byte records, valid until kg_table_close, and how many there are: num_sigs for a built or adopted table, the
 * whole records of the file for an opened one (fewer than num_sigs for a truncated file, more for a longer one) */
const void *kg_table_device_entries(const kg_table *t);
int64_t kg_table_records(const kg_table *t);
/* header fields (KmerMemoryInfo, KGJ:1194-1198) and the number of occupied slots */
int kg_table_info(const kg_table *t, int64_t *num_sigs, int64_t *entry_size, int64_t *version, int64_t *occupied);
/* Bytes of device scratch / result blocks the table's block cache has handed out and not got back: the blocks of the
 * results still open, 0 when there are none (also after a failed kg_scan*: nothing may be left behind). */
int64_t kg_table_live_device_bytes(kg_table *t);
void kg_table_close(kg_table *t);

/* ---- the hot path: replaces prepareQuery/addKmers (KGJ:1051-1074, 900-922), the query sort
 *      (KGJ:1076-1095), lookup (KGJ:944-1034) and gatherHits/processSetOfHits (KGJ:385-514) for a
 *      batch of sequences.  seq = the raw concatenated sequence characters exactly as readFasta
 *      hands them to prepareQuery (KGJ:780-783); offsets[n_seqs+1] in host memory. ---- */
int kg_scan(kg_table *t, const kg_params *p, const uint8_t *seq, const int64_t *offsets,
            int64_t n_seqs, kg_result **out);
/* same with the sequence bytes already in device memory (offsets stay on the host).  The bytes must be
 * complete before the call: the library works on its own non-blocking stream. */
int kg_scan_device(kg_table *t, const kg_params *p, const uint8_t *d_seq, const int64_t *offsets,
                   int64_t n_seqs, kg_result **out);

/* ---- the aggregation alone: replaces the public gatherHits / processSetOfHits / processAASeq (KGJ:385-514, 526-536) for
 *      callers that hold hit records of their own.  hits[] ordered by (container, from0InProt), container_hit_start[n_seqs *
 *      (aa ? 1 : 6) + 1]; otu_init = the oICounts buffer every sequence starts with (n_seqs records) or NULL for empty
 *      buffers (KGJ:528, 540).  The result has the hit, CALL, OTU and event arrays (no table, no scan statistics). ---- */
int kg_aggregate_hits(int device, const kg_params *p, const kg_hit *hits, const int64_t *container_hit_start, int64_t n_seqs,
                      const kg_otu *otu_init, kg_result **out);

/* One step of that state machine, the public processSetOfHits (KGJ:385-455): votes for current_fi among hits[0..n_hits),
 * *called / *call = whether a CALL was made and its record, *otu = the caller's oICounts buffer (updated in place),
 * *new_current_fi = the method's return value, *keeps_last_two = the list keeps hits[n-2], hits[n-1] (else it is emptied). */
int kg_process_set_of_hits(int device, const kg_params *p, const kg_hit *hits, int32_t n_hits, int32_t current_fi, kg_otu *otu,
                           kg_call *call, int32_t *called, int32_t *new_current_fi, int32_t *keeps_last_two);

int kg_result_stats(const kg_result *r, kg_stats *out);
/* Host views, copied from the device on first use; NULL on failure (see kg_last_error). */
const kg_hit  *kg_result_hits(kg_result *r);                 /* n_hits, ordered by (container, from0InProt)   */
const int64_t *kg_result_container_hit_start(kg_result *r);  /* n_containers + 1                              */
const kg_call *kg_result_calls(kg_result *r);                /* n_calls, in the reference's emission order     */
const int64_t *kg_result_container_call_start(kg_result *r); /* n_containers + 1                              */
const kg_otu  *kg_result_otu(kg_result *r);                  /* n_seqs                                        */
const uint8_t *kg_result_hit_events(kg_result *r);           /* n_hits bytes of KG_EV_*                        */
const uint8_t *kg_result_container_tail_events(kg_result *r);/* n_containers bytes of KG_EV_TAIL_*             */
/* hits[first .. first + count) straight into caller-owned memory (e.g. a JNA Memory / numpy array); pageable
 * destinations are fed through the library's cached pinned blocks, the copy overlapped with the transfer. */
int kg_result_copy_hits(kg_result *r, int64_t first, int64_t count, kg_hit *dst);
/* KG_F_PROGRESS scans only (NULL / KG_ERR_ARG otherwise): the table slot every hit record was found at (n_hits entries,
 * parallel to kg_result_hits: distinct slots = distinct k-mers found, the reference's kmersFound, KGJ:1004-1006), and the
 * summary above.  Several scans of one run (batches): the slots combine by minimum / maximum; the two counts are per scan (a
 * k-mer found in two batches counts in both), a front end that needs them over several scans counts the distinct hit slots. */
const uint32_t *kg_result_hit_slots(kg_result *r);
int kg_result_progress(const kg_result *r, kg_progress *out);
/* Device views (valid until kg_result_free) for callers that keep working in HBM. */
const void    *kg_result_device_hits(const kg_result *r);
const void    *kg_result_device_calls(const kg_result *r);
const void    *kg_result_device_otu(const kg_result *r);
const void    *kg_result_device_container_hit_start(const kg_result *r);   /* int64[n_containers + 1] */
const void    *kg_result_device_container_call_start(const kg_result *r);  /* int64[n_containers + 1], NULL with KG_F_SKIP_AGGREGATE */
void kg_result_free(kg_result *r);

/* ---- multi-GPU exchange helper (no counterpart in the reference, which is one process; used by the host layer that
 *      gathers per-rank hit buffers, kmergutsjava_amd/distributed.py).  The n_hits records at d_src are ordered by a shard's
 *      LOCAL containers; the records of local sequence k are d_src[d_seq_first[k] .. d_seq_first[k + 1]) (d_seq_first has
 *      n_seqs + 1 entries) and go to d_dst[d_dst_first[k] ..) with d_container_shift[k] added to their container field.
 *      All pointers are device memory; the copy is enqueued on `stream` (a hipStream_t, NULL = the null stream) and not
 *      waited for. ---- */
int kg_restore_hits_device(int device, const kg_hit *d_src, int64_t n_hits, const int64_t *d_seq_first, int64_t n_seqs,
                           const int64_t *d_dst_first, const int32_t *d_container_shift, kg_hit *d_dst, void *stream);

const char *kg_last_error(void);
/* "libkmerguts_hip <version> gfx950" */
const char *kg_version(void);

#ifdef __cplusplus
}
#endif
#endif
