/*
 * uvaia_gpu.h -- C ABI of the MI355X (gfx950) nearest-neighbour engine.
 *
 * This is the drop-in boundary for uvaia's hot path.  The reference (quadram-institute-bioscience/uvaia,
 * paths below are under /root/reference) has no plugin/FFI layer: the seam is the three OpenMP loops of
 * src/nearest.c:293-306 (and src/ball.c:248-251) plus the serial per-batch bookkeeping around them.  A
 * maintainer replaces those loops by calls to this library and keeps everything else (CLI, FASTA streaming,
 * heap_t/query_t host structures, writers).  See INTEGRATION.md for the patch.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a negative UVAIA_GPU_E* code and never
 *     calls exit(); uvaia_gpu_last_error() gives the message (the reference's biomcmc_error() = message + exit,
 *     src/nearest.c:208,277: the caller turns a code into that behaviour).
 *   - sequences are nchar upper-case bytes (what readfasta_next() src/fastaseq.c:422-474 and upper_kseq()
 *     src/utils.c:22 produce).  Alphabet: ACGT, IUPAC partial codes MRWSYKVHDB, and the invalid set
 *     N X - ? O . (src/utils.c:263).  Any other byte is refused with UVAIA_GPU_EALPHABET (its treatment by the
 *     absent biomcmc kernel is not pinned by anything in the reference).
 *   - a "batch" is one pool of the reference (src/nearest.c:249-251): the consensus pre-score of every sequence
 *     in it is truncated at the largest per-query tolerance at batch start (src/nearest.c:290-291,431-432), so
 *     batch boundaries are part of the semantics and are chosen by the caller, exactly as --pool is.
 *   - references are identified by a 64-bit ordinal supplied by the caller; names stay on the host
 *     (the reference strdup()s names into the heaps, src/min_heap.c:101,112).
 *   - one context = one GPU = one host thread at a time.
 */
#ifndef UVAIA_GPU_H
#define UVAIA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UVAIA_GPU_NSCORE 6          /* q_item.score[6], src/min_heap.h:14-18 */

enum {
  UVAIA_GPU_OK         =  0,
  UVAIA_GPU_EINVAL     = -1,   /* bad argument */
  UVAIA_GPU_ENODEV     = -2,   /* no usable gfx950 device / HIP runtime error at start-up */
  UVAIA_GPU_ENOMEM     = -3,   /* device or host allocation failed */
  UVAIA_GPU_EHIP       = -4,   /* HIP runtime error (message in last_error) */
  UVAIA_GPU_EALPHABET  = -5,   /* a sequence holds a byte outside the supported alphabet */
  UVAIA_GPU_ESTATE     = -6    /* call sequence error (e.g. push larger than max_pool) */
};

typedef struct uvaia_gpu_ctx uvaia_gpu_ctx;

/* The prepared query set: the fields of struct query_struct (src/fastaseq.h:41-48) the hot path reads, after
 * create_query_indices()/reorder_query_structure() (src/fastaseq.c:732-795).  consensus[i] is 'N' where no query
 * is usable, '#' where queries disagree, else the shared character (src/fastaseq.c:742-756). */
typedef struct {
  int n_query;                 /* query->aln->ntax */
  int nchar;                   /* query->aln->nchar */
  const char *const *seq;      /* query->aln->character->string[i], nchar bytes each, upper-case */
  const char *consensus;       /* query->consensus, nchar bytes */
  const size_t *idx_c, *idx_m, *idx;   /* increasing site indices, as create_query_indices() builds them */
  int n_idx_c, n_idx_m, n_idx;
  size_t trim;                 /* query->trim */
  int acgt;                    /* query->acgt (--acgt) */
} uvaia_gpu_query;

/* Replaces new_queue() (src/nearest.c:367-390): per-query heaps of max(2,heap_size) slots (src/min_heap.c:58) with
 * max_incompatible = nchar (src/nearest.c:375,387), plus device buffers for batches of up to max_pool references.
 * device: HIP device index (-1 = current). */
int uvaia_gpu_open (uvaia_gpu_ctx **ctx, const uvaia_gpu_query *query, int heap_size, int device, size_t max_pool);

/* The same with tuning.  Every field 0 = the library's own choice; the values change speed, never results (the library reads no
 * environment variables). */
enum { UVAIA_GPU_SCAN_AUTO = 0,        /* by query count: packed planes up to 32 queries, column-compressed above */
       UVAIA_GPU_SCAN_PACKED = 1,      /* two-counter scan straight over the packed planes (nothing derived per query set) */
       UVAIA_GPU_SCAN_COMPRESSED = 2,  /* column-compressed scan over planes derived for the query set */
       UVAIA_GPU_SCAN_WIDE = 3 };      /* four 32-bit counters per pair (what alignments above 49 000 columns get) */
typedef struct {
  size_t subslice_refs;        /* resident search: references per scan launch (pools are cut into slices of about this length; >= 64) */
  int rare_max;                /* a polymorphic column counts as "rare" when all but at most this many queries carry the same base; -1 = no rare columns */
  int scan;                    /* UVAIA_GPU_SCAN_* */
  int serial;                  /* 1 = no overlap between the rebuild of the derived planes, the scans and the replays (isolated kernel timings) */
  int scan_tiles_per_wave;     /* column-compressed scan: 1, 2 or 4 tiles of 64 references per wave (default 2; 4 only with 8 waves per block) */
  int scan_waves_per_block;    /* column-compressed scan: 4 or 8 waves share a super-tile of 64 queries (default 8) */
  int rederive_streams;        /* uvaia_gpu_db_rederive: its chunks alternate over 1..3 streams (default: 3 for a rebuild of up to three chunks -- all in flight at once, the first still done first --, 1 from four chunks on) */
  int ball_gather;             /* radius search: the references' planes on the columns of query->idx are gathered 1 = by a pass of its own over the
                                  references that go on to the queries, 2 = by the consensus pass itself, for every reference (default 2) */
  int query_tables;            /* the scans' query-side tables (plane words, column classes, rare columns, compressed planes, item streams) are built
                                  1 = by host threads, 2 = on the device from the raw rows (default 2); same bytes either way */
  int replay_extras;           /* default mode: 0 = the library's choice (as 2 over the packed-plane scan, i.e. up to 32 queries; as 1 above), 2 = the scan also
                                  leaves text - ACGT and partial - text matches of every pair and the replay admits without a memory round trip (up to 128
                                  queries; over the column-compressed scan two kernels after the scan make them), 1 = the replay fetches them per admitted pair */
  int replay_cus;              /* compute units set aside for the replay's stream, the scans and the rebuild getting the others (CU masks): 0 = the
                                  library's choice (where replay_extras applies as many as hold one replay block per query at once, 8 up to 32 queries;
                                  none otherwise), -1 = none, n > 0 = n; 1000 * t + n also sets the replay's staging depth to t = 32, 16 or 8 tiles */
  int scan_streams;            /* resident search: consecutive slices' scans alternate over 1..3 streams (0 = the library's choice by launch size);
                                  100 + p (p = 1..98): a pool's first slice is p % of an equal share, 199: equal slices
                                  (the library's choice: equal slices in default mode with a large query set, else 70) */
  int pipeline;                /* reserved: accepted and ignored (the pipelined replay it selected was removed) */
  int head_scan;               /* reserved: accepted and ignored (the four-counter head it selected was removed) */
  int derive_waves;            /* the kernel that derives a tile's planes for the query set runs 4, 8 or 16 waves per tile (0 = the library's choice: 4;
                                  measured alike at config[1]); same arrays from every width */
} uvaia_gpu_tuning;
/* Diagnostics: a copy of one of the query-side tables the scans read, as the open call left it on the device (tests compare the two ways
 * of building them).  which: 0 query plane words, 1 recoded planes (default mode), 2 ambiguity-word lists, 3 column classes, 4 rare-column
 * mask, 5 compressed polymorphic planes, 6 planes on the rare columns, 7 item streams, 8 their directory, 9 the rebuild's column split,
 * 10 = eleven ints { polymorphic columns, rare columns, their word groups (2), rare_max, scan choice, groups needing E / V / counts /
 * rare planes, replay_lq }.  *n_bytes = size of the table; copied only when it fits cap. */
int uvaia_gpu_export_query_table (uvaia_gpu_ctx *ctx, int which, void *out, size_t cap, size_t *n_bytes);
int uvaia_gpu_open_tuned (uvaia_gpu_ctx **ctx, const uvaia_gpu_query *query, int heap_size, int device, size_t max_pool, const uvaia_gpu_tuning *tuning /* may be NULL */);
void uvaia_gpu_close (uvaia_gpu_ctx *ctx);
const char *uvaia_gpu_last_error (const uvaia_gpu_ctx *ctx);   /* ctx may be NULL: error of the last failed open */

/* Replaces one turn of the batch loop, src/nearest.c:288-306: snapshot of max_incompatible, the consensus pre-score
 * (queue_distance_to_consensus, :428-433), the per-query gate + heap update over the batch in order
 * (queue_update_min_heaps{,_full,_acgt}, :435-510) and the OR over is_best (:303-306).
 *   seq[i]     n_ref sequences of nchar bytes, in stream order (cq->seq[c]); entries must be non-NULL
 *   non_n[i]   quick_count_sequence_non_N() of each (cq->non_n[c], src/nearest.c:263); NULL = count on the device
 *   ordinal0   ordinal of seq[0]; seq[i] gets ordinal0+i
 *   entered[i] out, 1 if the sequence entered the heap of any query during this batch (cq->is_best[n_query*c],
 *              src/nearest.c:310: such sequences are written to the .aln dump by the caller) */
int uvaia_gpu_push (uvaia_gpu_ctx *ctx, const char *const *seq, const int *non_n, int n_ref, int64_t ordinal0,
                    uint8_t *entered);

/* Reads the heaps back.  All arrays are caller-allocated:
 *   n_items[q]                      heap[q]->n
 *   max_incompatible[q]             heap[q]->max_incompatible
 *   scores[(q*(slots+1)+s)*6 + i]   heap[q]->seq[s].score[i], s = 1..n in the reference's binary-heap layout
 *   ordinals[q*(slots+1)+s]         ordinal of heap[q]->seq[s]
 * with slots = uvaia_gpu_heap_slots().  Slot 0 is unused, as in src/min_heap.c.  The caller then runs
 * heap_finalise_heap_qsort() (src/min_heap.c:149-158) on its own heap_t copies. */
int uvaia_gpu_drain (uvaia_gpu_ctx *ctx, int *n_items, int *max_incompatible, int *scores, int64_t *ordinals);
int uvaia_gpu_heap_slots (const uvaia_gpu_ctx *ctx);      /* max(2,heap_size) */
int uvaia_gpu_n_query (const uvaia_gpu_ctx *ctx);
/* Back to the state right after uvaia_gpu_open() (heaps empty, entered flags of the resident database cleared); a resident database is
 * kept.  Asynchronous: one kernel launch, ordered before every later call on the context (pushes, searches, slice replays, state
 * import / export, uvaia_gpu_drain, uvaia_gpu_entered_flags) and behind the searches issued before it; it does not wait for the device. */
int uvaia_gpu_reset (uvaia_gpu_ctx *ctx);

/* ---- HBM-resident database (the measured configuration: references packed once, scanned many times) ----
 * Sequences are packed into bit-planes and appended to a device-resident database; they must already have passed
 * the caller's filters (src/nearest.c:255-278).  non_n as in uvaia_gpu_push (NULL = count on the device). */
int uvaia_gpu_db_reserve (uvaia_gpu_ctx *ctx, size_t n_ref_capacity);
int uvaia_gpu_db_append (uvaia_gpu_ctx *ctx, const char *const *seq, const int *non_n, int n_ref);
/* same, from one host block of n_ref rows of `pitch` bytes (pitch >= nchar) */
int uvaia_gpu_db_append_block (uvaia_gpu_ctx *ctx, const char *rows, size_t pitch, const int *non_n, int n_ref);
size_t uvaia_gpu_db_size (const uvaia_gpu_ctx *ctx);
/* Scans the resident database in batches of `pool` references (ordinals = position in the database + ordinal0),
 * i.e. the whole while-loop of src/nearest.c:249-330 for one reference file.  entered (may be NULL): db_size bytes.
 * Asynchronous with respect to the host unless entered != NULL; uvaia_gpu_sync() waits. */
int uvaia_gpu_search_resident (uvaia_gpu_ctx *ctx, size_t pool, int64_t ordinal0, uint8_t *entered);
int uvaia_gpu_sync (uvaia_gpu_ctx *ctx);

/* ---- ring mode for several GPUs (one context per GPU/process; the caller moves the state blob between ranks, e.g. with
 * RCCL send/recv).  A stripe = one batch of the reference (one pool) = the concatenation of one slice per rank, in rank
 * order; every rank holds its slices in its resident database.  Per stripe, on every rank:
 *     uvaia_gpu_slice_scan()                         (asynchronous; may be issued stripes ahead: two counter buffers)
 *     [rank > 0 or not the first stripe]  receive blob from the previous rank in the ring; uvaia_gpu_state_import()
 *     uvaia_gpu_slice_replay(stripe_start = (rank == 0))
 *     uvaia_gpu_state_export(); send blob to the next rank
 * The blob holds the batch snapshot of src/nearest.c:290-291 taken by rank 0, so truncation semantics are those of a
 * single process running the same stripes as pools.  After the last stripe the last rank holds the final heaps. */
size_t uvaia_gpu_state_bytes (const uvaia_gpu_ctx *ctx);
int uvaia_gpu_state_export (uvaia_gpu_ctx *ctx, void *dst);          /* device or host pointer; returns when dst is complete */
int uvaia_gpu_state_import (uvaia_gpu_ctx *ctx, const void *src);    /* src may be reused once this returns */
int uvaia_gpu_slice_scan (uvaia_gpu_ctx *ctx, size_t first, size_t n, int buf);      /* buf in [0, uvaia_gpu_slice_buffers()) */
int uvaia_gpu_slice_replay (uvaia_gpu_ctx *ctx, int buf, int64_t ordinal0, int stripe_start);
int uvaia_gpu_slice_buffers (void);     /* number of counter buffers: a scan may be issued that many slices ahead of its replay */
/* The per-query machines are independent, so the state can travel in several blobs, one per contiguous group of queries
 * [q0,q1): while one rank replays group j of a slice the next rank already replays group j-1 of its own slice.
 * take_snapshot: only on the rank that opens a stripe, once it holds the state of ALL queries (the snapshot is a maximum
 * over every query); it is a no-op for the results when the query set has no constant-and-complete column (n_idx_c == 0). */
size_t uvaia_gpu_state_range_bytes (const uvaia_gpu_ctx *ctx, int q0, int q1);
int uvaia_gpu_state_export_range (uvaia_gpu_ctx *ctx, void *dst, int q0, int q1);
int uvaia_gpu_state_import_range (uvaia_gpu_ctx *ctx, const void *src, int q0, int q1);
int uvaia_gpu_slice_replay_range (uvaia_gpu_ctx *ctx, int buf, int64_t ordinal0, int q0, int q1, int take_snapshot);
int uvaia_gpu_entered_flags (uvaia_gpu_ctx *ctx, uint8_t *out, int clear);   /* db_size bytes; see uvaia_gpu_search_resident */

/* ---- radius search: replaces the loop of src/ball.c:248-251 (seq_ball_against_query_structure,
 * src/fastaseq.c:660-696) for one batch.  radius = cq->dist + 1.  mindist[i] receives what the reference leaves in
 * cq->mindist[c]; the caller keeps sequence i iff mindist[i] <= radius-1 (src/ball.c:255). */
int uvaia_gpu_ball (uvaia_gpu_ctx *ctx, const char *const *seq, int n_ref, int radius, int *mindist);
/* the same for references [first, first+n) of the resident database.  Both stop where the reference stops: a reference whose
 * distance to the queries' consensus reaches the radius costs one pass over its packed planes, the queries are looked at only
 * for the references the reference's own loop would look at them for (twice the consensus distance >= radius). */
int uvaia_gpu_ball_resident (uvaia_gpu_ctx *ctx, size_t first, size_t n, int radius, int *mindist);
/* the same for a batch whose text is not in memory (replaces the loop of src/ball.c:248-259 for it): n_ref <= max_pool references
 * handed in as ceil(n_ref/64) whole tiles of the packed interchange form below (what uvaia_gpu_db_export writes and a packed database
 * file holds, uvaia_gpu_db_tile_bytes() per tile; lanes past n_ref in the last tile are ignored whatever they hold).  mindist[] as in
 * uvaia_gpu_ball.  Works in default-mode and --acgt contexts (the latter re-code the planes while importing).  The radius search reads
 * nothing of a reference but its planes, so no valid-site counts and no side rows are taken; nothing is derived for the
 * nearest-neighbour scans and the resident database is not touched.  Refused like uvaia_gpu_ball: a batch above max_pool, a context
 * with a restricted query range.  The four-plane tiles stay on the device until the next call replaces them (an --acgt context keeps
 * a coding of its own, from which the text cannot be rebuilt): */
int uvaia_gpu_ball_packed (uvaia_gpu_ctx *ctx, const void *planes, int n_ref, int radius, int *mindist);
/* ... and this writes the upper-case text of references index[0..n) of that batch (positions within the batch; any order, repeats
 * allowed) to host memory rows + k * pitch, pitch >= nchar: per site the IUPAC character of the set of bases the planes hold, 'N' for
 * the empty and for the full set.  Invalid characters other than 'N' ('-', '?', 'X', 'O', '.') are not in the planes: the caller puts
 * them back from its own record of them (uvdb_apply_exceptions for a packed database file).  Only nchar bytes of a row carry text, the
 * others up to pitch are unspecified afterwards; rows whose pitch is nchar rounded up to 16 come back in one plain copy (pinned memory
 * is the caller's choice).  An index outside the last batch, or a call with no batch, is an error return and leaves the context usable. */
int uvaia_gpu_unpack_rows (uvaia_gpu_ctx *ctx, const int *index, int n, char *rows, size_t pitch);
unsigned long long uvaia_gpu_ball_asked (uvaia_gpu_ctx *ctx, int reset);    /* references sent on to the queries since the last reset */
/* device time in ms since the last reset of the three kernels of the radius search: [0] the consensus pass, [1] the gather of the asked
   references' columns (with the read-back of their number), [2] the pair scan on the gathered tiles */
void uvaia_gpu_ball_kernel_ms (uvaia_gpu_ctx *ctx, double out[3], int reset);

/* Query preprocessing: the O(Q^2) test of exclude_redundant_query_sequences (src/fastaseq.c:797-841, the
 * call at :806-808).  For each of n_seq sequences (<= max_pool) and each query q of the open set,
 *   out[i * n_query + q] = 1  when quick_pairwise_score_truncated_idx_indelcheck (default; src/fastaseq.c:562-574) or
 *                             quick_pairwise_score_acgt (--acgt; :576-583) with maxdist 1 over query->idx would return 0,
 * i.e. no polymorphic column where both are valid (--acgt: both ACGT) and differ; 0 otherwise.  Handing in the query
 * sequences themselves gives the whole pair matrix; the host then walks it in the reference's order. */
int uvaia_gpu_agree_on_polymorphic (uvaia_gpu_ctx *ctx, const char *const *seq, int n_seq, uint8_t *out);

/* create_query_indices (src/fastaseq.c:732-777) on the device; no context needed (device < 0: the current one).  seq: n_query rows of
 * nchar bytes as the reference holds them at that point (upper-case).  Out, per column: consensus[i] as the reference defines it
 * ('N' outside the trimmed window or where no query is usable -- valid, with acgt != 0 ACGT --, '#' where two usable characters
 * differ, else the shared character) and some_missing[i] = 1 where some query is not usable (the reference's miss[], :744-756).
 * The caller builds idx / idx_m / idx_c from them exactly as src/fastaseq.c:763-770 does. */
int uvaia_gpu_query_columns (const char *const *seq, int n_query, int nchar, size_t trim, int acgt, int device, char *consensus, unsigned char *some_missing);

/* ---- introspection used by tests and bench.py ---- */
/* untruncated pair scores of the last batch: out[(i*n_query+q)*6 + s] = the score[] vector src/nearest.c:499-501
 * (or :464-469 with --acgt) assembles for (reference i of the batch, query q) when nothing is truncated. */
int uvaia_gpu_last_batch_scores (uvaia_gpu_ctx *ctx, int *out, int n_ref);
/* device time (ms) and launch count of the dominant kernel (the pair scan), measured with HIP events on the
 * context's stream since the last call with reset != 0; bytes = algorithmic bytes those launches covered. */
int uvaia_gpu_scan_stats (uvaia_gpu_ctx *ctx, double *ms, long long *launches, double *algorithmic_bytes, int reset);
/* counters of the ordered replay since the last reset: out[0] = admissions into heaps, out[1] = pairs whose remaining
 * counters were evaluated on demand, out[2] = of those, evaluated by a dense rescan (ambiguity lists overflowed) */
int uvaia_gpu_replay_stats (uvaia_gpu_ctx *ctx, unsigned long long out[3], int reset);
/* (query, tile of 64 references) pairs whose counters the replay of the packed-plane scan looked at since the last reset (up to 32 queries,
 * default mode: how sharp the per-tile bounds are) */
int uvaia_gpu_replay_tiles_opened (uvaia_gpu_ctx *ctx, unsigned long long *out, int reset);
/* Diagnostics of an engine built with -DREPLAY_TIMING (all zeros otherwise): wall-clock ticks (100 MHz) summed over the replay waves of the
 * packed-plane scan -- [0] waiting for staged counters, [1] requesting them, [2] inside opened tiles, [3] of that in admissions,
 * [4] late fetches, [5] their number, [6] whole waves, [7] their prologues (heap and tables into LDS), [8] waves; [9..11] unused.  (replay2_kernel:
 * [0] waits for on-demand words, [1] exact comparisons, [2] heap updates, [3] waits for a group's counters, [4] tolerance rises, [5] groups,
 * [6] whole waves, [7] the slowest wave.) */
int uvaia_gpu_replay_timing (uvaia_gpu_ctx *ctx, unsigned long long out[12], int reset);
/* The slices a resident search cuts references [first, first + n) into when it runs them in batches of `pool` (uvaia_gpu_search_resident
 * is first = 0, n = db_size; uvaia_gpu_db_rederive rebuilds along first = 0, n = db_size, pool = max_pool): slice i covers
 * [slice_first[i], slice_first[i] + slice_n[i]) and takes the batch snapshot first where pool_start[i] != 0.  Returns the number of
 * slices and writes the first `cap` of them (the arrays may be NULL with cap = 0), or a negative code: pool < 1 or pool > max_pool is
 * refused as uvaia_gpu_search_resident refuses it.  Host arithmetic only: the database is not looked at, nothing is allocated, the device
 * is not touched. */
int uvaia_gpu_search_plan (uvaia_gpu_ctx *ctx, size_t first, size_t n, size_t pool, size_t *slice_first, size_t *slice_n, unsigned char *pool_start, int cap);
/* tuning knob: queries held per pass of the packed-plane and four-counter scans (8, 16 or 32); 0 = default */
int uvaia_gpu_set_query_tile (uvaia_gpu_ctx *ctx, int qt);
/* ---- query shards: several GPUs, each holding the whole database and the heaps of a contiguous range of the queries.  The
 * per-query machines of src/nearest.c:435-510 are independent given the column classes of the WHOLE query set (which the context
 * was opened with), so a rank scans and replays only its range; no data-path exchange.  The one coupling between queries is the
 * batch snapshot cq->max_incompatible = max over ALL heaps (src/nearest.c:290-291), which matters only when the query set has
 * constant-and-complete columns (n_idx_c > 0): then the driver runs pool by pool, all-reduces (max) uvaia_gpu_max_tolerance()
 * over the ranks and passes the result as `snapshot`.
 *   set_active_queries: resident and slice calls act on queries [q0, q1) only (q0 a multiple of 64: the scan's super-tile of queries; any q0 under reference shards, where the range only selects tolerances); push/ball need the full range
 *   search_resident_pool: one batch [first, first+n) of the resident database, n <= max_pool; snapshot < 0 = take it from this
 *                         context's active queries */
int uvaia_gpu_set_active_queries (uvaia_gpu_ctx *ctx, int q0, int q1);
int uvaia_gpu_max_tolerance (uvaia_gpu_ctx *ctx, int *out);
int uvaia_gpu_search_resident_pool (uvaia_gpu_ctx *ctx, size_t first, size_t n, int64_t ordinal0, int snapshot);

/* ---- reference shards: several GPUs, each keeping, deriving and scanning 1/N of the references against ALL queries and replaying 1/N of
 * the queries over ALL references (the default layout for several GPUs; DESIGN.md "Multi-GPU").  The scores of a pair do not
 * depend on anything but the pair, so the scan -- more than nine tenths of a search -- shards by reference; the gate + heap machine
 * of a query is sequential in stream order (src/nearest.c:488,504-508) but independent of the other queries, so the replay shards
 * by query; in between, the pair counters of a slice move once: rank r sends to rank d the rows of d's queries (one all-to-all per
 * slice over RCCL between processes -- uvaia_amd/refshard.py -- or peer copies inside one process -- uvaia_gpu_group_*).
 *   - the stream is dealt in pieces of piece_refs references (a whole number of tiles of 64); piece p belongs to rank p % world
 *   - a rank KEEPS only its own pieces: packed planes, side rows, counts and the planes derived for the query set.  Appends are handed
 *     the whole stream in order (uvaia_gpu_db_append* keep the context's share and count the rest; uvaia_gpu_db_skip moves the
 *     stream position over references of other ranks without handing them over): every rank stages and packs 1/N of the database.
 *   - a replaying rank needs, of a piece scanned elsewhere: the rows of its queries (cnt, tmin), a small block per reference (`aux`:
 *     valid sites and, with constant-and-complete query columns, the untruncated consensus pre-score), and -- for the few pairs that
 *     reach the exact comparison -- words of the reference's packed planes and its side row, which it READS IN PLACE from the rank
 *     that keeps them: uvaia_gpu_shard_set_peer (one process: the other member's device pointers, peer access enabled) or
 *     uvaia_gpu_shard_ipc_handles / _open (one process per GPU: hipIpc mappings, over xGMI on a node)
 *   - the one coupling between queries, the batch snapshot cq->max_incompatible = max over ALL heaps (src/nearest.c:290-291), is
 *     exchanged per batch when it can matter (query sets with constant-and-complete columns): uvaia_gpu_max_tolerance on the
 *     active queries of every rank, maximum over the ranks, uvaia_gpu_set_snapshot.
 * set_shard: before the database is reserved.  shard_scan: references [first, first+n) inside ONE owned piece, n <= max_pool;
 *   cnt  uint32 [uvaia_gpu_shard_rows()][tiles * 64] pair counters as the scan kernels write them (first | second << 16: ACGT matches and
 *                                                    valid pairs, with --acgt mismatches and comparable sites), row = query, a reference
 *                                                    in column (position - 64 * (first / 64)); tiles = tiles the range touches
 *   tmin int2 [uvaia_gpu_shard_rows()][tiles]        the two bounds per (query, tile) the replay skips tiles by
 *   aux  uvaia_gpu_shard_aux_bytes(tiles) bytes      int valid_sites[tiles * 64], then (constant-and-complete columns) int4 prescore[tiles * 64]
 *   all caller-owned device buffers; asynchronous on the scan stream, uvaia_gpu_scan_wait() returns when they are complete.
 * shard_replay: gate + heaps of queries [q0, q1) over references [first, first+n) -- a piece of rank `owner` -- from buffers of the same
 *   layout that hold ONLY the rows q0 .. q1-1 and the piece's aux block; pieces must be replayed in stream order; asynchronous (uvaia_gpu_sync). */
int uvaia_gpu_db_set_shard (uvaia_gpu_ctx *ctx, int rank, int world, size_t piece_refs);
int uvaia_gpu_shard_rows (const uvaia_gpu_ctx *ctx);
size_t uvaia_gpu_shard_aux_bytes (const uvaia_gpu_ctx *ctx, size_t n_tiles);
int uvaia_gpu_shard_scan (uvaia_gpu_ctx *ctx, size_t first, size_t n, void *cnt, void *tmin, void *aux);
int uvaia_gpu_db_skip (uvaia_gpu_ctx *ctx, size_t n_ref);
int uvaia_gpu_shard_set_peer (uvaia_gpu_ctx *ctx, int rank, const void *planes, const void *side_rows);
const void *uvaia_gpu_shard_planes (const uvaia_gpu_ctx *ctx);
const void *uvaia_gpu_shard_side_rows (const uvaia_gpu_ctx *ctx);
int uvaia_gpu_shard_ipc_handle_bytes (void);
int uvaia_gpu_shard_ipc_handles (uvaia_gpu_ctx *ctx, void *out /* uvaia_gpu_shard_ipc_handle_bytes() bytes */);
int uvaia_gpu_shard_ipc_open (uvaia_gpu_ctx *ctx, int rank, const void *handles);
int uvaia_gpu_shard_ipc_close (uvaia_gpu_ctx *ctx);     /* unmaps them again: every rank closes, then a barrier, then the owners may free */
int uvaia_gpu_scan_wait (uvaia_gpu_ctx *ctx);
int uvaia_gpu_replay_wait (uvaia_gpu_ctx *ctx);      /* replays issued so far are complete: their counter buffers may be overwritten */
int uvaia_gpu_set_snapshot (uvaia_gpu_ctx *ctx, int snapshot);
/* Ordering against a stream the caller owns (a hipStream_t: the stream its collectives run on), by events, without the host: the
 * reference-shard driver queues scan -> exchange -> replay of stripe after stripe and never blocks.
 *   mark              remembers, under slot 0..7, the scans (or replays) issued so far
 *   stream_wait_mark  `stream` waits for that mark (the scan whose output the exchange sends; the replays that still read a buffer the
 *                     exchange is about to refill)
 *   wait_stream       the scans (or replays) issued from now on wait for what `stream` holds now (the exchange still reading the buffer a
 *                     scan overwrites; the exchange that delivers a replay's counters) */
enum { UVAIA_GPU_SCANS = 0, UVAIA_GPU_REPLAYS = 1 };
int uvaia_gpu_mark (uvaia_gpu_ctx *ctx, int what, int slot);
int uvaia_gpu_stream_wait_mark (uvaia_gpu_ctx *ctx, void *stream, int slot);
int uvaia_gpu_wait_stream (uvaia_gpu_ctx *ctx, int what, void *stream);
int uvaia_gpu_shard_replay (uvaia_gpu_ctx *ctx, const void *cnt, const void *tmin, const void *aux, int owner, size_t first, size_t n, int64_t ordinal0, int q0, int q1);

/* ---- a group of contexts driven by ONE host thread (the command line's --devices): the reference-shard protocol with peer copies
 * as the exchange; replaces the batch loop of src/nearest.c:245-330 for several GPUs.  devices[i] = HIP device of member i (a
 * device may be listed more than once); piece_refs = 0 picks a default.  Calls mirror the single-context ones: the database is
 * appended to every member, search_resident / push run the sharded search, drain collects every query's heap from the member
 * that replays it.  A group of one device is a plain context. */
typedef struct uvaia_gpu_group uvaia_gpu_group;
int  uvaia_gpu_group_open (uvaia_gpu_group **group, const uvaia_gpu_query *query, int heap_size, const int *devices, int n_devices, size_t max_pool, size_t piece_refs);
void uvaia_gpu_group_close (uvaia_gpu_group *group);
const char *uvaia_gpu_group_last_error (const uvaia_gpu_group *group);     /* group may be NULL: error of the last failed open */
int  uvaia_gpu_group_size (const uvaia_gpu_group *group);
uvaia_gpu_ctx *uvaia_gpu_group_member (uvaia_gpu_group *group, int i);
int  uvaia_gpu_group_query_shard (const uvaia_gpu_group *group, int i, int *q0, int *q1);
int  uvaia_gpu_group_db_reserve (uvaia_gpu_group *group, size_t n_ref_capacity);
int  uvaia_gpu_group_db_append (uvaia_gpu_group *group, const char *const *seq, const int *non_n, int n_ref);
int  uvaia_gpu_group_db_append_packed (uvaia_gpu_group *group, const void *planes, const int *non_n, const int *side_rows, int n_ref);
int  uvaia_gpu_group_db_clear (uvaia_gpu_group *group);
int  uvaia_gpu_group_db_rederive (uvaia_gpu_group *group);
size_t uvaia_gpu_group_db_size (const uvaia_gpu_group *group);
int  uvaia_gpu_group_reset (uvaia_gpu_group *group);
int  uvaia_gpu_group_search_resident (uvaia_gpu_group *group, size_t pool, int64_t ordinal0, uint8_t *entered);
int  uvaia_gpu_group_push (uvaia_gpu_group *group, const char *const *seq, const int *non_n, int n_ref, int64_t ordinal0, uint8_t *entered);
int  uvaia_gpu_group_drain (uvaia_gpu_group *group, int *n_items, int *max_incompatible, int *scores, int64_t *ordinals);
int  uvaia_gpu_group_sync (uvaia_gpu_group *group);

/* ---- packed interchange form (packed on-disk database).  Replaces, for a database that was packed once,
 * the serial text path of the reference (readfasta_next src/fastaseq.c:422-474 + the slot filling of src/nearest.c:251-286 +
 * quick_count_sequence_non_N src/fastaseq.c:642-648): tiles of 64 references, each uvaia_gpu_db_tile_bytes() long, laid out
 * [word group][plane A,C,G,T][lane] as 16-byte words (plane bit s of word w = site 32 w + s carries that IUPAC set bit), the
 * valid-site counts, and per reference a side row of uvaia_gpu_db_side_row_ints() ints (its partially ambiguous words).  The form
 * does not depend on the query set or on --acgt (an --acgt context re-codes the planes while importing).
 *   export:        from a default-mode (4-plane) context whose database was filled by uvaia_gpu_db_append*; arrays hold n_tiles*64
 *                  entries (lanes past the last reference are zero)
 *   append_packed: n_ref references = ceil(n_ref/64) tiles; the database must hold a whole number of tiles before the call */
size_t uvaia_gpu_db_tile_bytes (const uvaia_gpu_ctx *ctx);
int    uvaia_gpu_db_clear (uvaia_gpu_ctx *ctx);                      /* empties the resident database, keeps its capacity */
/* Rebuilds, for every resident reference, the planes the scan reads for the open query set (the appends build them for the rows
 * they add): the per-reference share of the work that depends on the query set (the reference does it implicitly, its loops
 * read the raw sequences through idx_c / idx_m / idx, src/nearest.c:428-510).  Asynchronous; later searches wait for it, and it
 * queues behind searches still in flight (after uvaia_gpu_sync there are none and its first launch is issued at once).  Call between
 * searches, e.g. to time a search of a resident database together with this work. */
int    uvaia_gpu_db_rederive (uvaia_gpu_ctx *ctx);
/* Introspection (tests compare the block widths of the deriving kernel array for array): what the column-compressed scan reads of the
 * first n_tiles tiles of 64 references, as the appends or the last uvaia_gpu_db_rederive left it (a rebuild in flight is waited for).
 * With G = ceil(ceil(nchar / 32) / 4) word groups and, from uvaia_gpu_export_query_table(.., 10, ..), P = word groups of the gathered
 * polymorphic + rare columns:  e [n_tiles][G][64] 16-byte words (the plane of matches with the constant query columns),
 * grp [n_tiles][G][64] uint32 (its and the valid-site plane's popcounts per group),  poly [n_tiles][P][3][64] 16-byte words (the gathered
 * columns),  tot [n_tiles * 64] int (matches with the constant columns per reference). */
int    uvaia_gpu_db_derived_export (uvaia_gpu_ctx *ctx, size_t n_tiles, void *e, uint32_t *grp, void *poly, int *tot);
int    uvaia_gpu_db_side_row_ints (void);
int    uvaia_gpu_db_export (uvaia_gpu_ctx *ctx, size_t first_tile, size_t n_tiles, void *planes, int *non_n, int *side_rows);
int    uvaia_gpu_db_append_packed (uvaia_gpu_ctx *ctx, const void *planes, const int *non_n, const int *side_rows, int n_ref);

/* ---- windowed search: a packed database larger than device memory (`uvaia --packed --window`).  Replaces, like the resident search, the
 * read/filter/fill loop of src/nearest.c:251-286 and the batch loop :288-306 -- for a file of which only a window of references is
 * resident at a time.  The machine is a serial walk over the stream whose state (heaps, tolerances) stays in the context, so the caller
 * walks the windows in stream order:
 *     stage_reserve (tiles of the largest span);  stage_packed (slot 0, first span)
 *     per window w:  load_staged (slot w % 2, sel, n);  search_resident (pool, ordinal0 = stream position of the window's first reference,
 *                    NULL);  stage_packed (slot (w + 1) % 2, next span);  sync;  entered_flags;  db_unpack_rows of those that entered
 * with windows that are a multiple of the pool (and of 64), so that the pools -- where the snapshot of the tolerances is retaken,
 * src/nearest.c:290-291 -- are the ones a search of the whole stream cuts.  Plain contexts only: a context of a reference shard gets
 * UVAIA_GPU_ESTATE, as from the other resident entries.
 *   stage_reserve  room for n_tiles whole tiles (planes, valid-site counts, side rows) in each of the two staging slots
 *   stage_packed   asynchronous copy of n_tiles whole file tiles (the arrays of uvaia_gpu_db_append_packed) into slot 0 or 1, on a copy
 *                  stream of the context's own: the bytes of the next window cross the bus while the current one is searched.  The
 *                  host arrays must stay as they are until the slot has been loaded.
 *   load_staged    waits for the slot's copy, empties the resident database (as uvaia_gpu_db_clear) and fills it with references
 *                  sel[0 .. n_ref) of the slot, in that order: sel[k] is a position within the slot (0 .. 64 * n_tiles - 1), NULL = positions
 *                  0 .. n_ref - 1.  Totals, the checks on side rows and counts and the planes derived for the query set are made as
 *                  uvaia_gpu_db_append_packed makes them.  A bad sel entry is refused with UVAIA_GPU_EINVAL before anything is
 *                  launched and leaves the database as it was.  Afterwards uvaia_gpu_db_size() is n_ref; heaps and tolerances are
 *                  not touched.  Returns when the window is complete.
 *   db_unpack_rows the contract of uvaia_gpu_unpack_rows for positions of the window loaded last, in default-mode and --acgt contexts
 *                  (the latter keep a four-plane image of the window for it).
 *   stage_packed_at  stage_packed for a piece of a slot: the n_tiles tiles land at tile `tile_offset` of the slot, so that spans of several
 *                  files sit one after another in one slot and sel indexes the slot.  A piece at tile 0 starts the slot afresh (its tile
 *                  count becomes n_tiles); a later piece leaves the count at the largest end reached.  A piece that ends beyond the
 *                  reserved capacity is refused with UVAIA_GPU_ESTATE.  Tiles of the slot no piece has filled hold whatever they held.
 *   append_staged  waits for the slot's copy and appends references sel[0 .. n_ref) of it (NULL: positions 0 .. n_ref - 1) BEHIND the
 *                  uvaia_gpu_db_size() references already resident, whatever that size is modulo 64: reference db_size + k goes to tile
 *                  (db_size + k) / 64, lane (db_size + k) % 64 with its plane words, valid-site count and side row.  The database is not
 *                  cleared and the resident lanes of the first tile are not written; lanes past the new end of the last tile are zero
 *                  (what uvaia_gpu_db_export promises).  Re-coding (--acgt), totals, the checks on side rows and counts and the derived
 *                  planes are made for the rows added, as uvaia_gpu_db_append_packed makes them; db_unpack_rows then decodes positions of
 *                  the whole resident database (--acgt: as long as all of it came through load_staged / append_staged since it was last
 *                  empty; db_clear, the other appends and db_drop_tiles end the image, and db_unpack_rows then answers UVAIA_GPU_ESTATE).  Refusals as
 *                  load_staged, before anything is launched; capacity as uvaia_gpu_db_append_packed (reserve before the first append).
 *                  Several packed files load as one stream this way, and a merge is stage -> append_staged -> export.
 *   stage_compact_at  the compact sibling of stage_packed_at, for a piece of a version 2 packed database (uvaia_amd/csrc/host/uvdb.h): same
 *                  slot and offset rules, same refusals, same ordering against the loads.  base: one reference's worth of planes;
 *                  head_idx / lit_idx: the n_tiles * 64 + 1 offsets of the staged lanes as the file holds them; heads / lits: the START
 *                  of the file's two record sections, which the offsets count from (only the records of the staged lanes are read);
 *                  non_n as for stage_packed_at.  The base, the piece's records and counts go to buffers the context owns, and
 *                  expand_tiles_kernel writes the dense tiles into the slot; the side rows are made there from the expanded planes in
 *                  the fixed form of uvaia_gpu_db_export (an --acgt context keeps none).  load_staged, append_staged and
 *                  db_unpack_rows cannot tell how a slot was filled.  The heads must have passed uvdb_open's checks; the kernel bounds
 *                  every access all the same.  The host arrays must stay as they are until the slot has been loaded.
 *   compact_ms     device time in ms since the last reset of [0] expand_tiles_kernel, [1] the side-row pass (waits for the last expansion)
 *   window_ms      device time in ms since the last reset of [0] the selection, [1] totals, checks and derived planes after it, [2] the decode
 *   stage_unpack_rows  the contract of uvaia_gpu_unpack_rows (any order, repeats, N for the empty and the full set, exception characters are
 *                  the caller's business, pitch >= nchar) for positions within staging slot `slot` -- the positions sel of load_staged
 *                  uses -- whatever stage_packed[_at] or stage_compact_at last put there: the text of a few references of a packed file
 *                  without loading them.  Waits for the slot's copy, decodes the slot's four planes where they lie (default-mode and --acgt
 *                  contexts alike: a slot holds the file's planes) and lets the next stage into the slot wait for the decode.  The resident
 *                  database, the loaded window, the derived planes, the heaps and the tolerances are not touched.  Refused, with the
 *                  context as usable as before: an index at or beyond 64 * (tiles filled in the slot) and a pitch below nchar
 *                  (UVAIA_GPU_EINVAL), a slot never staged and a context of a reference shard (UVAIA_GPU_ESTATE).
 *   stage_unpack_ms  device time in ms of stage_unpack_rows' kernel since the last reset
 *   free_bytes     free memory of the context's device as the runtime reports it (0: the runtime could not tell) */
int uvaia_gpu_db_stage_reserve (uvaia_gpu_ctx *ctx, size_t n_tiles);
int uvaia_gpu_db_stage_packed (uvaia_gpu_ctx *ctx, int slot, const void *planes, const int *non_n, const int *side_rows, int n_tiles);
int uvaia_gpu_db_load_staged (uvaia_gpu_ctx *ctx, int slot, const int *sel, int n_ref);
int uvaia_gpu_db_stage_packed_at (uvaia_gpu_ctx *ctx, int slot, size_t tile_offset, const void *planes, const int *non_n, const int *side_rows, int n_tiles);
int uvaia_gpu_db_append_staged (uvaia_gpu_ctx *ctx, int slot, const int *sel, int n_ref);
int uvaia_gpu_db_stage_compact_at (uvaia_gpu_ctx *ctx, int slot, size_t tile_offset, const void *base, const uint64_t *head_idx, const uint32_t *heads,
                                   const uint64_t *lit_idx, const void *lits, const int *non_n, int n_tiles);
void uvaia_gpu_compact_ms (uvaia_gpu_ctx *ctx, double out[2], int reset);
int uvaia_gpu_db_unpack_rows (uvaia_gpu_ctx *ctx, const int *index, int n, char *rows, size_t pitch);
void uvaia_gpu_window_ms (uvaia_gpu_ctx *ctx, double out[3], int reset);
int uvaia_gpu_db_stage_unpack_rows (uvaia_gpu_ctx *ctx, int slot, const int *index, int n, char *rows, size_t pitch);
double uvaia_gpu_stage_unpack_ms (uvaia_gpu_ctx *ctx, int reset);
size_t uvaia_gpu_free_bytes (uvaia_gpu_ctx *ctx);

/* ---- resident tiles written in the compact form of a packed database (version 2 of uvaia_amd/csrc/host/uvdb.h), the inverse of
 * stage_compact_at: per lane the 32-site words that differ from a base row, as the canonical fill and literal heads the host writer
 * (uvdb_create_compact) gives the same rows.  About a twelfth of what uvaia_gpu_db_export copies leaves the device.  Two steps, because the
 * sizes of the records are only known after the first:
 *   db_encode_compact   base: one reference's worth of planes in the file's [word group][plane A,C,G,T] order (16-byte words), any base --
 *                  correctness does not depend on it.  Counts the records of resident tiles first_tile .. first_tile + n_tiles - 1 and
 *                  fills head_idx and lit_idx (n_tiles * 64 + 1 offsets each, from 0; literal offsets in words of 16 bytes) and non_n
 *                  (n_tiles * 64 counts, as uvaia_gpu_db_export gives them).  Lanes at and past the last resident reference are encoded as
 *                  all-zero rows, which is what the index sections of a file hold for them.  The plan stays in the context.
 *   db_encoded_records  the records of the plan: head_idx[last] dwords to heads, 4 * lit_idx[last] dwords to lits (planes A, C, G, T of every
 *                  literal word).  Every store on the device is bounded by the extent the plan gives its lane.
 *   Refusals, all leaving the context usable: those of uvaia_gpu_db_export (an --acgt context, a context of a reference shard: UVAIA_GPU_ESTATE;
 *   tiles outside the database: UVAIA_GPU_EINVAL); an alignment of more than UVAIA_GPU_COMPACT_MAX_NCHAR sites, db_encoded_records without a
 *   plan or after any call that changed the database (appends, loads, db_skip, db_clear, db_drop_tiles): UVAIA_GPU_ESTATE.
 *   encode_ms      device time in ms since the last reset of [0] the count and prefix passes, [1] the emit pass */
#define UVAIA_GPU_COMPACT_MAX_NCHAR 2097152
int uvaia_gpu_db_encode_compact (uvaia_gpu_ctx *ctx, size_t first_tile, size_t n_tiles, const void *base, uint64_t *head_idx, uint64_t *lit_idx, int *non_n);
int uvaia_gpu_db_encoded_records (uvaia_gpu_ctx *ctx, uint32_t *heads, void *lits);
void uvaia_gpu_encode_ms (uvaia_gpu_ctx *ctx, double out[2], int reset);

/* ---- rows that are already in device memory (what the aligner leaves behind, include/uvaia_align.h; a tensor of the caller): into the
 * resident database and a packed database file without a round trip of their text.  A block is n rows of nchar bytes, `pitch` bytes apart
 * (pitch >= nchar; neither the pitch nor the first row need any alignment).  Every d_rows below must be memory of the context's device: the
 * runtime is asked, and a pointer of another device, a host pointer or rows that end beyond their allocation are refused with
 * UVAIA_GPU_EINVAL before anything reads them.  Plain contexts only (no reference shards).
 *
 * rows_census: replaces, for such a block, quick_count_sequence_non_N (uvaia_amd/csrc/host/seq_query.c:105-115, the call of pack_main.c:86)
 *   and the counting half of the exception pass of uvdb_add_reference (host/uvdb.c:79-94).  non_n[i] = valid sites of row i, n_exc[i] = the
 *   exception records its text gives (maximal stretches of one of - ? X O . , cut every 0xFFFFFF sites).  One kernel, one copy back.  A
 *   byte uvaia_gpu_db_append refuses fails the call with UVAIA_GPU_EALPHABET (the counts are filled in all the same).
 * db_append_device: replaces the staging of uvaia_gpu_db_append (the copy of every row into pinned memory and over the bus): appends rows
 *   row_index[0 .. n_sel) of the block (NULL: rows 0 .. n_sel - 1), in that order; non_n[k] belongs to the k-th appended row (NULL = count on
 *   the device).  Planes, valid-site counts, side rows and totals are what uvaia_gpu_db_append leaves for the same rows, in default-mode
 *   and --acgt contexts, from any database size on.  Returns when the rows have been read.
 * rows_exceptions: replaces the record-writing half of the exception pass (host/uvdb.c:79-94).  offsets: n_sel + 1 increasing record
 *   positions, offsets[k + 1] - offsets[k] = n_exc of the k-th selected row; exc_out: host array of (uint32 pos, uint32 len << 8 | char)
 *   records, row k's at exc_out + offsets[k], by position.  One kernel, one copy back; offsets that do not fit the rows fail with
 *   UVAIA_GPU_EINVAL and write nothing outside their ranges.
 * db_drop_tiles: removes the first n_tiles tiles of the resident database; what follows them moves to the front (a caller that exports whole
 *   tiles as they fill keeps the unfinished one resident and goes on appending to it). */
int uvaia_gpu_rows_census (uvaia_gpu_ctx *ctx, const void *d_rows, size_t pitch, int n, int *non_n, int *n_exc);
int uvaia_gpu_db_append_device (uvaia_gpu_ctx *ctx, const void *d_rows, size_t pitch, const int *row_index, int n_sel, const int *non_n);
int uvaia_gpu_rows_exceptions (uvaia_gpu_ctx *ctx, const void *d_rows, size_t pitch, const int *row_index, int n_sel, const uint64_t *offsets, void *exc_out);
int uvaia_gpu_db_drop_tiles (uvaia_gpu_ctx *ctx, size_t n_tiles);
/* device time in ms since the last reset of [0] the census, [1] the gathers of db_append_device, [2] the exception fill */
void uvaia_gpu_rows_kernel_ms (uvaia_gpu_ctx *ctx, double out[3], int reset);
/* diagnostics: the length exception runs are cut at (0 = the file format's 0xFFFFFF), so that tests reach the cut with short rows */
int uvaia_gpu_rows_set_run_cut (uvaia_gpu_ctx *ctx, unsigned cut);

/* ---- text row store: the text of rows that came from device memory, kept on the device as text next to the resident database (`uvaia -r
 * --device-parse`).  Replaces, for such rows, the host copies of the sequences that the dump of src/nearest.c:299-304 writes from: a reference
 * appended by uvaia_gpu_db_append_device has no text on the host, uvaia_gpu_db_unpack_rows answers only for windows that came through
 * load_staged / append_staged, and an --acgt context keeps no four-plane image of other rows.  Store rows are nchar rounded up to 16 bytes
 * apart and 16-byte aligned.  Plain contexts only (no reference shards: UVAIA_GPU_ESTATE).
 *   text_append_device  rows row_index[0 .. n_sel) of a block in device memory (NULL: rows 0 .. n_sel - 1) are appended to the store in that
 *                  order.  The block has the contract of uvaia_gpu_db_append_device (any pitch >= nchar, any alignment; the pointer is
 *                  checked the same way).  The store grows on its own and keeps its content.  Returns when the rows have been read.
 *   text_size      rows in the store
 *   text_rows      store rows index[0 .. n) to host memory at rows + k * pitch: any order, repeats allowed, pitch >= nchar; nchar bytes of
 *                  each row are defined.  Gathered on the device, one copy back per round of a pool of rows.
 *   text_clear     empties the store, keeps its capacity
 *   text_reserve   room for n_rows rows in all (the content is kept)
 *   text_ms        device time in ms since the last reset of [0] the gathers in, [1] the gathers out
 * Refused with UVAIA_GPU_EINVAL, nothing copied, the store unchanged and the context usable: a host pointer, another device's memory or a
 * block that ends beyond its allocation; a negative count or row index; an index[k] at or beyond text_size; a pitch below nchar. */
int uvaia_gpu_text_append_device (uvaia_gpu_ctx *ctx, const void *d_rows, size_t pitch, const int *row_index, int n_sel);
size_t uvaia_gpu_text_size (const uvaia_gpu_ctx *ctx);
int uvaia_gpu_text_rows (uvaia_gpu_ctx *ctx, const int *index, int n, char *rows, size_t pitch);
int uvaia_gpu_text_clear (uvaia_gpu_ctx *ctx);
int uvaia_gpu_text_reserve (uvaia_gpu_ctx *ctx, size_t n_rows);
void uvaia_gpu_text_ms (uvaia_gpu_ctx *ctx, double out[2], int reset);

/* ---- FASTA text split into rows on the device (`uvaiapack --device-parse`).  Replaces, for a block of decompressed text, the line loop of
 * readfasta_next (uvaia_amd/csrc/host/seq_query.c:54-80: getline, realloc, the cleaning pass), quick_count_sequence_non_N and the copy of
 * every row into pinned memory: the rows are made where uvaia_gpu_rows_census and uvaia_gpu_db_append_device read them.  The rules of a
 * regular stream and what counts as irregular are stated in uvaia_amd/csrc/kernels_fasta.inc and restated in plain C by fasta_scan_host
 * (uvaia_amd/csrc/host/fasta_blocks.h).  A handle of its own: the parser runs before the alignment length, and with it any uvaia_gpu_ctx,
 * exists.  Offsets are positions in the text handed to the last scan.
 *
 * fasta_open:    device (-1 = the current one); block_bytes = the most text one scan takes (up to 1 GiB); max_records = the most records one
 *                scan returns.
 * fasta_scan:    pass 1 over text[0 .. n_bytes), host memory (pinned or not, any alignment; the copy keeps the alignment modulo 16).  final:
 *                the text ends the stream, so its last record is complete; otherwise a record is complete once a later header line begins
 *                in the text.  n_records = the complete records found, at most max_records; consumed = where the header line of the first
 *                record not returned begins (n_bytes when everything was taken).  n_records == 0 with consumed == 0 on text that is not
 *                final: its first record does not fit.  Irregular input among what would be returned -- a NUL byte, a line that is not
 *                blank before the first header line, a record without one sequence byte -- fails with UVAIA_GPU_EINVAL, the message naming
 *                the kind and the byte offset; nothing is returned or consumed and the handle stays usable.
 * fasta_bad:     what the last scan refused: the kind (UVAIA_GPU_FASTA_NUL, _EMPTY or _TEXT; 0 when it refused nothing of the text) and, in
 *                *offset, the byte of the text the message names.
 * fasta_records: the table of the last scan, n_records entries.
 * fasta_rows:    pass 2: the cleaned sequences of the records of the last scan whose length is nchar, in record order, at d_rows + k * pitch
 *                in device memory (pitch = nchar rounded up to 16; valid until the next scan).  row_of_record[i] = the row of record i, or
 *                -1 for a record of another length (may be NULL).
 * fasta_rows_host: diagnostics: the rows of the last fasta_rows, n_rows * pitch bytes, copied to host memory.
 * fasta_kernel_ms: device time in ms since the last reset of [0] pass 1, [1] pass 2.
 *
 * For sequences that are not aligned yet (`uvaialign --device-parse`), on the records of the last scan:
 * fasta_acgt:    acgt[k] = the body bytes of record k that are one of A C G T a c g t: the first counter of biomcmc_count_sequence_acgt
 *                (uvaia_amd/csrc/host/biomcmc_lite.c:378-392), n_records entries.  Its second counter, the "N etc." set, needs no kernel: it
 *                is seq_len - non_n of the record table, the same nine characters N n X x O o - ? . in both functions.
 * fasta_sequences: the cleaned sequences of records record[0 .. n_sel) (NULL: records 0 .. n_sel - 1), each at its own length, back to back
 *                in device memory: sequence k at d_bytes + offsets[k], offsets[k + 1] - offsets[k] = seq_len of that record, offsets[0] = 0
 *                (offsets: n_sel + 1 entries, host memory) -- the bytes + offsets form of uvaia_align_load_block, for
 *                uvaia_align_load_device.  Valid until the next scan or the next fasta_sequences; the call returns when the kernel is
 *                done.  An index outside the last scan or one that is repeated fails with UVAIA_GPU_EINVAL before anything is launched.
 * fasta_sequences_host: diagnostics: the buffer of the last fasta_sequences, offsets[n_sel] bytes and the 64 guard bytes behind them, which
 *                fasta_sequences sets to 0xEE before its launch and the kernel leaves alone; n_bytes must be offsets[n_sel] + 64.
 * fasta_sequences_ms: device time in ms since the last reset of [0] fasta_acgt, [1] fasta_sequences. */
typedef struct uvaia_gpu_fasta uvaia_gpu_fasta;
typedef struct {
  uint32_t name_off, name_len;   /* the bytes after the first '>' of the header line up to the end of that line */
  uint32_t body_off, body_len;   /* from behind the header line to where the next header line begins (or the text ends) */
  uint32_t seq_len;              /* bytes of the body that are no white space */
  int32_t non_n;                 /* of those, the valid sites (quick_count_sequence_non_N) */
  uint32_t flags;                /* UVAIA_GPU_FASTA_*: 0 in every record a successful scan returns */
  uint32_t bad_off;              /* UVAIA_GPU_FASTA_NUL: where the first NUL of the record is */
} uvaia_gpu_fasta_record;
#define UVAIA_GPU_FASTA_NUL   1u   /* the record holds a NUL byte */
#define UVAIA_GPU_FASTA_EMPTY 2u   /* the record has no sequence byte */
#define UVAIA_GPU_FASTA_TEXT  4u   /* (the text before the first header line only) a line that is not blank */
int uvaia_gpu_fasta_open (uvaia_gpu_fasta **out, int device, size_t block_bytes, int max_records);
void uvaia_gpu_fasta_close (uvaia_gpu_fasta *fasta);
const char *uvaia_gpu_fasta_last_error (const uvaia_gpu_fasta *fasta);   /* fasta may be NULL: error of the last failed open */
int uvaia_gpu_fasta_scan (uvaia_gpu_fasta *fasta, const void *text, size_t n_bytes, int final, int *n_records, size_t *consumed);
unsigned uvaia_gpu_fasta_bad (const uvaia_gpu_fasta *fasta, size_t *offset);
int uvaia_gpu_fasta_records (uvaia_gpu_fasta *fasta, uvaia_gpu_fasta_record *out);
int uvaia_gpu_fasta_rows (uvaia_gpu_fasta *fasta, int nchar, const void **d_rows, size_t *pitch, int *n_rows, int *row_of_record);
int uvaia_gpu_fasta_rows_host (uvaia_gpu_fasta *fasta, void *out);
void uvaia_gpu_fasta_kernel_ms (uvaia_gpu_fasta *fasta, double out[2], int reset);
int uvaia_gpu_fasta_acgt (uvaia_gpu_fasta *fasta, int *acgt);
int uvaia_gpu_fasta_sequences (uvaia_gpu_fasta *fasta, const int *record, int n_sel, const void **d_bytes, int64_t *offsets /* n_sel + 1 */);
int uvaia_gpu_fasta_sequences_host (uvaia_gpu_fasta *fasta, void *out, size_t n_bytes);
void uvaia_gpu_fasta_sequences_ms (uvaia_gpu_fasta *fasta, double out[2], int reset);
/* the bytes of text one block of pass 1 covers (tests place line ends and headers around its multiples) */
size_t uvaia_gpu_fasta_chunk_bytes (void);
/* page-locked host memory for the text blocks (NULL when there is none to be had), and its release */
void *uvaia_gpu_fasta_pinned_alloc (size_t bytes);
void uvaia_gpu_fasta_pinned_free (void *p);

/* ---- all pairs of the resident database against each other (`uvaiadist`).  What users of the reference do next with a set of aligned
 * genomes -- pairwise distances for trees and transmission clusters -- computed where the rows already are.  The counters of two resident
 * references a, b are taken over the sites [trim, nchar - trim), with nothing truncated:
 *   count[0] ACGT_matches            equal and ACGT             (first counter of the biomcmc 4-count kernel)
 *   count[1] text_matches            equal and both valid       (its second)
 *   count[2] partial_matches         IUPAC sets intersect       (its third)
 *   count[3] valid_pair_comparisons  both valid                 (its fourth)
 *   count[4] ACGT_pair_comparisons   both ACGT                  (second score of src/fastaseq.c:585-596)
 * and two distances come from them: snp = count[4] - count[0] (both ACGT and different: what snp-dists prints), uvaia = count[3] - count[2].
 *
 * db_pairs:        rows [row0, row0 + n_rows) against columns [col0, col0 + n_cols) of the resident database; out is host memory:
 *                    UVAIA_GPU_PAIRS_SNP     out[i * ld + j]           = snp distance
 *                    UVAIA_GPU_PAIRS_COUNTS  out[(i * ld + j) * 5 + c] = count[c]                  (ld >= n_cols, in pairs)
 *                  (UVAIA_GPU_PAIRS_SNP_ALT: the numbers of _SNP by the kernel's other row-tile height, for measurements).  Elements of out
 *                  between n_cols and ld are not written.
 * db_pairs_within: the pairs of that rectangle whose distance under `metric` is <= max_dist, upper != 0: only those with row < col (database
 *                  positions); sorted by (row, col); *n_found = how many there are; when *n_found > cap, out[0 .. cap) is unspecified and
 *                  nothing past cap is written.
 * pairs_ms:        device time in ms since the last reset of [0] the row operands, [1] the dense kernels, [2] the threshold kernels (and the
 *                  host's sort of the list).
 * Only a plain default-mode context is accepted: an --acgt context and a context of a reference shard answer UVAIA_GPU_ESTATE.  A rectangle
 * outside the database, 2 * trim > nchar, an unknown `what` or `metric`, a negative max_dist, a NULL out with something to write and
 * ld < n_cols are UVAIA_GPU_EINVAL, refused before anything is launched.  2 * trim == nchar gives all zeros; empty ranges succeed and write
 * nothing.  The database, the derived planes, the heaps and the tolerances are not touched; the calls wait for searches in flight and return when
 * out is complete.  Working memory is the context's, bounded by the rectangle of one launch: large rectangles are cut into launches. */
enum { UVAIA_GPU_PAIRS_SNP = 1, UVAIA_GPU_PAIRS_COUNTS = 2, UVAIA_GPU_PAIRS_SNP_ALT = 3 };   /* what */
enum { UVAIA_GPU_DIST_SNP = 1, UVAIA_GPU_DIST_UVAIA = 2 };                                   /* metric */
#define UVAIA_GPU_PAIR_NCOUNT 5
typedef struct { uint32_t row, col; int32_t count[UVAIA_GPU_PAIR_NCOUNT]; } uvaia_gpu_pair;
int uvaia_gpu_db_pairs (uvaia_gpu_ctx *ctx, size_t row0, size_t n_rows, size_t col0, size_t n_cols, size_t trim, int what, int32_t *out, size_t ld);
int uvaia_gpu_db_pairs_within (uvaia_gpu_ctx *ctx, size_t row0, size_t n_rows, size_t col0, size_t n_cols, size_t trim, int metric, int max_dist, int upper,
                               uvaia_gpu_pair *out, size_t cap, unsigned long long *n_found);
void uvaia_gpu_pairs_ms (uvaia_gpu_ctx *ctx, double out[3], int reset);

/* ---- single-linkage clusters within a distance (`uvaiadist -d D --clusters`): the cluster every resident reference belongs to, labelled on
 * the device.  Take the rows [0, n) of the resident database, a trim, a metric, a distance max_dist >= 0 and a floor min_compared >= 0.  Two
 * rows a < b are LINKED iff  dist(a, b) <= max_dist  and  compared(a, b) >= min_compared,  where under UVAIA_GPU_DIST_SNP dist = count[4] -
 * count[0] and compared = count[4] (ACGT_pair_comparisons), under UVAIA_GPU_DIST_UVAIA dist = count[3] - count[2] and compared = count[3]
 * (valid_pair_comparisons), the counters above over [trim, nchar - trim).  A cluster is a connected component of that graph and its label
 * the smallest database position among its members: a function of the rows alone, whatever the order of the calls, of the launches or of
 * the waves, and however the caller cut the matrix.
 *   The floor is part of the definition, not a repair: under snp a row with no ACGT site (all N, all gaps) is at distance 0 from EVERY row,
 * so with min_compared = 0 one such row joins all clusters into one.  min_compared >= 1 is what a caller sets against it.
 *
 * db_link_begin:  checks as db_pairs does (over the whole database), sets every resident reference to a cluster of its own and remembers
 *                 the parameters and the size of the database.
 * db_link:        links the pairs row < col (database positions) of rows [row0, row0 + n_rows) x columns [col0, col0 + n_cols) and ADDS
 *                 their number to *n_links (a pair linked by two calls is counted twice; the clusters do not change).  Cut into the launches
 *                 of db_pairs; launches wholly at or below the diagonal are skipped.  The whole matrix needs every pair row < col covered
 *                 once, e.g. one call per band of rows against all columns.
 * db_link_labels: labels[i] for the references resident at `begin`; may be called more than once, and between db_link calls (the
 *                 components of the links made so far).
 * link_ms:        device time in ms of the link and label kernels since the last reset (the row operands go to pairs_ms [0]); pairs_ms
 *                 is unchanged.
 * db_link and db_link_labels answer UVAIA_GPU_ESTATE without a db_link_begin and once the database changed after it; contexts are refused
 * as by db_pairs; an unknown metric, negative max_dist or min_compared, 2 * trim > nchar, a rectangle outside the database and a NULL
 * n_links or labels are UVAIA_GPU_EINVAL.  Nothing dense is written and nothing but *n_links and the labels crosses the bus. */
int uvaia_gpu_db_link_begin (uvaia_gpu_ctx *ctx, size_t trim, int metric, int max_dist, int min_compared);
int uvaia_gpu_db_link (uvaia_gpu_ctx *ctx, size_t row0, size_t n_rows, size_t col0, size_t n_cols, unsigned long long *n_links);
int uvaia_gpu_db_link_labels (uvaia_gpu_ctx *ctx, uint32_t *labels);
void uvaia_gpu_link_ms (uvaia_gpu_ctx *ctx, double *ms, int reset);

/* ---- minimum spanning tree and closest row (`uvaiadist --mst`, `--nearest`): for every resident reference its closest reference of ANOTHER
 * component, and around that the minimum spanning forest of the database by Boruvka rounds.  Nothing dense is written.
 *   dist and compared of two database positions a != b over the sites [trim, nchar - trim) are those of db_link_begin: under
 * UVAIA_GPU_DIST_SNP dist = count[4] - count[0] and compared = count[4], under UVAIA_GPU_DIST_UVAIA dist = count[3] - count[2] and
 * compared = count[3].
 *   EDGES.  {a, b} is an edge iff compared(a, b) >= min_compared.  With min_compared = 0 the graph is complete; with a floor it may fall
 * apart, and the answer is then a spanning FOREST.
 *   ORDER.  Edges are ordered by the triple (dist, lo, hi), lexicographically, lo < hi the two positions.  The order is strict and total,
 * so the minimum spanning forest is unique: it is what Kruskal's algorithm builds when it takes the edges in that order.  Every tie is
 * decided by it; nothing in the output depends on the order of launches, of atomics or on how the matrix was cut.
 *   NEAREST.  Given comp[] (one value per reference), near(x) is the smallest key (dist(x, y), y) over the y with {x, y} an edge and
 * comp[y] != comp[x], packed as (uint64_t) dist << 32 | y; UVAIA_GPU_NEAR_NONE says there is no such y.  For a fixed x the order of
 * (dist, y) agrees with the order of (dist, lo, hi), so a component's minimum outgoing edge is the minimum, under the edge order, of its
 * members' near.
 *   As under db_link_begin, a row with no ACGT site is under snp at distance 0 from every row: with min_compared = 0 it is the hub of the
 * tree and everyone's nearest.  min_compared >= 1 is what a caller sets against it.
 *
 * db_near_begin:      checks as db_link_begin does, remembers the parameters and the size of the database, sets every reference to a
 *                     component of its own and every key to NONE.  12 bytes of device memory per reference.
 * db_near_components: comp[i] for the references resident at `begin` (NULL: every reference its own), and every key back to NONE.
 * db_near:            lowers the keys of BOTH ends of every counting pair row < col (database positions) of rows [row0, row0 + n_rows) x
 *                     columns [col0, col0 + n_cols): the upper triangle, covered once, is the whole matrix.  Calls accumulate until the
 *                     next db_near_components.  Cut into the launches of db_link; launches wholly at or below the diagonal are skipped,
 *                     and so is a launch whose rows and columns all carry one comp.  Inside a launch a tile pair (32 rows under snp, 16
 *                     under uvaia, x one tile of 64 columns) whose rows and columns in range all carry one comp is skipped before any
 *                     site is counted.  stats (may be NULL): ADDS to stats[0] the tile pairs walked and to stats[1] the tile pairs skipped
 *                     (those of launches skipped for their comp included, those of launches at or below the diagonal not).
 * db_near_fetch:      best[i] = near(i) over the pairs covered so far, for the references resident at `begin`.
 * db_mst:             the minimum spanning forest under the order above: begins, then rounds of (components, near over the whole matrix,
 *                     fetch, and on the host every component's minimum and a union-find) until a round adds nothing or one tree is left.
 *                     edges has room for db_size - 1; *n_edges edges come back sorted by (dist, a, b), a < b; *n_rounds (may be NULL)
 *                     counts the passes of the matrix.  More than 64 rounds are an error (UVAIA_GPU_ESTATE), never a retry.  Leaves a
 *                     db_near_begin of its parameters open.
 * near_ms:            device time in ms of the near kernels since the last reset (the row operands go to pairs_ms [0]).
 * near_tiles:         out[0] the tile pairs walked and out[1] the tile pairs skipped by every db_near since the last reset, those that
 *                     db_mst made included.
 * db_near_components, db_near and db_near_fetch answer UVAIA_GPU_ESTATE without a db_near_begin and once the database changed after it;
 * contexts are refused as by db_pairs; an unknown metric, a negative min_compared, 2 * trim > nchar, a rectangle outside the database and
 * a NULL best, edges (with two references or more) or n_edges are UVAIA_GPU_EINVAL.  An empty database is fine and returns nothing.  The
 * database, the forest of db_link and everything of the searches are not touched. */
#define UVAIA_GPU_NEAR_NONE UINT64_MAX
typedef struct { uint32_t a, b; int32_t dist; } uvaia_gpu_edge;
int uvaia_gpu_db_near_begin (uvaia_gpu_ctx *ctx, size_t trim, int metric, int min_compared);
int uvaia_gpu_db_near_components (uvaia_gpu_ctx *ctx, const uint32_t *comp);
int uvaia_gpu_db_near (uvaia_gpu_ctx *ctx, size_t row0, size_t n_rows, size_t col0, size_t n_cols, unsigned long long stats[2]);
int uvaia_gpu_db_near_fetch (uvaia_gpu_ctx *ctx, uint64_t *best);
int uvaia_gpu_db_mst (uvaia_gpu_ctx *ctx, size_t trim, int metric, int min_compared, uvaia_gpu_edge *edges, size_t *n_edges, int *n_rounds);
void uvaia_gpu_near_ms (uvaia_gpu_ctx *ctx, double *ms, int reset);
void uvaia_gpu_near_tiles (uvaia_gpu_ctx *ctx, unsigned long long out[2], int reset);

/* bytes the pair scan reads per reference (the default scan reads planes derived from the packed record for this query set) */
size_t uvaia_gpu_scan_bytes_per_ref (const uvaia_gpu_ctx *ctx);
/* the pair scan of this context: 2 = column-compressed scan over planes derived for the query set (default above 32 queries),
 * 0 = two-counter scan straight over the packed planes (default up to 32 queries: nothing is derived), -1 = four-counter scan
 * (alignments above 49 000 columns) */
int uvaia_gpu_scan_variant (const uvaia_gpu_ctx *ctx);
/* bytes per reference uvaia_gpu_db_rederive writes (the planes that depend on the query set; the appends also write the
 * valid-site plane, which does not) */
size_t uvaia_gpu_derived_bytes_per_ref (const uvaia_gpu_ctx *ctx);
/* bytes per packed reference in HBM */
size_t uvaia_gpu_packed_bytes_per_ref (const uvaia_gpu_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
