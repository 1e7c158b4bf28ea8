/*
 * uvaia_align.h -- C ABI of the MI355X (gfx950) gap-affine wavefront aligner behind `uvaialign`.
 *
 * Drop-in boundary for the alignment loop of the reference (quadram-institute-bioscience/uvaia, paths under
 * /root/reference): src/align.c keeps one WFA aligner per thread (new_queue, src/align.c:286-313), and for every pool
 * of query sequences runs align_query (src/align.c:357-364: affine_wavefronts_clear, affine_wavefronts_align,
 * update_query_aligned) under `#pragma omp parallel for` (src/align.c:224-233).  A maintainer replaces that loop by
 * uvaia_align_batch() and keeps the rest of main() (readers, filters of src/align.c:199-213, writers).
 *
 * What one call computes per query, bit for bit the CPU restatement's result (oracle/wfa_oracle.h; the WFA library
 * itself is an absent submodule: parity UNPINNED beyond the optimal gap-affine score, see that header):
 *   - the gap-affine wavefront alignment of the reference sequence (pattern) against the query (text) with penalties
 *     {match 0, mismatch, gap opening, gap extension} and the adaptive wavefront reduction (minimum wavefront length,
 *     maximum distance threshold) of affine_wavefronts_new_reduced (src/align.c:305-309: {0,4,6,2}, 128, 512);
 *   - its projection on the reference's columns (update_query_aligned, src/align.c:366-390): M/X copy the query
 *     character, I drops it, D writes '-': a row of exactly ref_len characters.
 *
 * Conventions: plain C; 0 on success or a negative UVAIA_ALIGN_E* code, never exit(); uvaia_align_last_error() gives
 * the message.  Sequences are bytes compared for equality as they are (the reference's reader upper-cases them,
 * src/fastaseq.c:462-466).  One aligner = one GPU = one host thread at a time.  There is no CPU fallback:
 * uvaia_align_open fails with UVAIA_ALIGN_ENODEV without a gfx950 device.
 */
#ifndef UVAIA_ALIGN_H
#define UVAIA_ALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  UVAIA_ALIGN_OK      =  0,
  UVAIA_ALIGN_EINVAL  = -1,
  UVAIA_ALIGN_ENODEV  = -2,
  UVAIA_ALIGN_ENOMEM  = -3,   /* device/host allocation failed, or a query needs more wavefront memory than the workspace holds */
  UVAIA_ALIGN_EHIP    = -4,
  UVAIA_ALIGN_ESTATE  = -5
};

typedef struct uvaia_aligner uvaia_aligner;

/* affine_penalties_t + the reduction arguments of affine_wavefronts_new_reduced (src/align.c:305-309) */
typedef struct {
  int mismatch, gap_opening, gap_extension;      /* match is 0 (src/align.c:305); mismatch and extension > 0, opening >= 0, mismatch and opening + extension below 64 */
  int min_wavefront_length;                      /* <= 0: complete wavefronts (no reduction) */
  int max_distance_threshold;
  size_t workspace_bytes;                        /* device memory for the wavefronts of the queries in flight; 0 = starts at 4 GB and grows,
                                                    up to three quarters of the free memory, when queries find it exhausted */
  int max_blocks;                                /* queries in flight (one block of four wavefronts each); 0 = as many as the chip holds */
} uvaia_align_options;

/* the reference's values: {4, 6, 2, 128, 512, 0, 0} */
void uvaia_align_default_options (uvaia_align_options *opt);

/* new_queue (src/align.c:286-313): the reference sequence goes to the device once.  opt may be NULL (defaults). */
int  uvaia_align_open (uvaia_aligner **out, const char *ref, int ref_len, int device, const uvaia_align_options *opt);
void uvaia_align_close (uvaia_aligner *a);
const char *uvaia_align_last_error (const uvaia_aligner *a);

/* One pool (src/align.c:224-233 + :357-390): n queries, seq[i] of seq_len[i] bytes.
 *   aln   : n rows of ref_len + 1 bytes (row i = cq->aln[i], NUL-terminated)
 *   score : n alignment scores (the reference does not report them; nullable)
 * A query whose score would pass the reference's table size (ref_len * 4 + 6 + 4 * ref_len, the allocation of
 * affine_wavefronts_new_reduced (L, 3L, ..)) fails the call with UVAIA_ALIGN_EINVAL: the reference has no check there. */
int  uvaia_align_batch (uvaia_aligner *a, const char *const *seq, const int *seq_len, int n, char *aln, int *score);

/* The same in three steps, for callers that keep a pool resident (bench.py times uvaia_align_run with the queries in HBM):
 * load copies the queries to the device, run aligns the loaded pool and returns when its kernels are done (rows and scores stay
 * on the device), fetch copies them back (aln may be NULL when only the scores are wanted: the rows then stay on the device). */
int  uvaia_align_load (uvaia_aligner *a, const char *const *seq, const int *seq_len, int n);
int  uvaia_align_load_block (uvaia_aligner *a, const char *bytes, const int64_t *offsets /* n + 1 */, int n);
/* load_block with the bytes already in device memory (uvaia_gpu_fasta_sequences of include/uvaia_gpu.h gives this form): d_bytes must be
 * memory of the aligner's device and [offsets[0], offsets[n]) must lie inside its allocation -- a host pointer, memory of another device
 * and a range that ends beyond the allocation are refused with UVAIA_ALIGN_EINVAL before anything is read.  The queries are copied device
 * to device: the source may go once the call has returned. */
int  uvaia_align_load_device (uvaia_aligner *a, const void *d_bytes, const int64_t *offsets /* n + 1, host */, int n);
int  uvaia_align_run (uvaia_aligner *a);
int  uvaia_align_sync (uvaia_aligner *a);
int  uvaia_align_fetch (uvaia_aligner *a, char *aln, int *score);
/* Instead of the fetch (the copy in uvaia_align_fetch of uvaia_amd/csrc/uvaia_align.hip and everything a caller then does to the text to bring it back to a
 * GPU): where the rows of the last completed run lie in device memory -- *n rows of ref_len characters, *pitch = ref_len + 1 bytes apart,
 * on HIP device *device (any of the four may be NULL).  They stay valid from the end of the run (uvaia_align_run returns when its kernels
 * are done; uvaia_align_sync otherwise) until the next load or close, and go to the engine as they are (include/uvaia_gpu.h, "rows that
 * are already in device memory").  UVAIA_ALIGN_ESTATE before a run has completed. */
int  uvaia_align_device_rows (uvaia_aligner *a, const void **d_rows, size_t *pitch, int *n, int *device);

/* The characters the projection drops (the `I` operations of update_query_aligned, src/align.c:366-390; the reference has no such output).
 * An insertion run is a maximal stretch of I operations of one query's alignment: ref_pos reference sites (0 .. ref_len; M, X and D
 * operations) and seq_pos query characters (M, X and I operations) lie to its left, and its bases are seq[seq_pos .. seq_pos + length). */
typedef struct { int query, ref_pos, seq_pos, length; } uvaia_align_insertion;
/* src/align.c:366-390: keep the runs of the following runs of this aligner (off by default; rows, scores and the statistics do not change).
 * capacity_records is the record buffer of one kernel launch, 0 = the library's choice; a launch that fills it runs the queries concerned
 * again with a buffer as large as they need, so no capacity makes a call fail or lose a record (tests pass a tiny one to reach that path) */
int  uvaia_align_set_insertions (uvaia_aligner *a, int on, size_t capacity_records);
/* src/align.c:366-390: the runs of the last completed run (uvaia_align_run / _sync / _batch) with the option on, and all their bases;
 * UVAIA_ALIGN_ESTATE with the option off or before such a run has completed.  Either pointer may be NULL. */
int  uvaia_align_insertion_counts (uvaia_aligner *a, long long *n_records, long long *n_bases);
/* src/align.c:366-390: the records sorted by (query, ref_pos) and their bases one after the other in that order (n_records records, n_bases
 * bytes, no NUL; either may be NULL).  The bases are gathered on the device from the aligner's own copy of the pool, so they are there
 * after uvaia_align_load_device too.  Valid until the next load or close.  UVAIA_ALIGN_ESTATE as above. */
int  uvaia_align_fetch_insertions (uvaia_aligner *a, uvaia_align_insertion *rec, char *bases);

/* What a row on the reference's columns differs from the reference by (the rows update_query_aligned writes, src/align.c:366-390; the
 * reference has no such output).  Bytes are taken as they are: A C G T are bases, '-' is a gap, 'N' is unknown, every other byte is "other".
 *   substitution 'S': a site where the row holds a base that is not the reference's byte: ref_pos = the site, length = 1, ref and alt the
 *                     two bytes.  Neighbouring substitutions are not merged.
 *   deletion 'D':     a maximal run of gaps: ref_pos = its first site, length = its sites, ref = alt = 0.  Runs that touch the row's first
 *                     or last site are deletions like any other (first_site / last_site say where the row's coverage starts and ends).
 * The records of one row are in ascending ref_pos.  Per row: matches (a base equal to the reference's byte), substitutions, deletion_runs,
 * deleted_sites, unknown_sites, other_sites -- matches + substitutions + deleted_sites + unknown_sites + other_sites == ref_len -- and the
 * first and last site that is no gap (ref_len and -1 for a row of gaps). */
typedef struct { int query, ref_pos, length; uint32_t kind_ref_alt; } uvaia_align_variant;      /* 'S' or 'D' | ref << 8 | alt << 16 */
typedef struct { int matches, substitutions, deletion_runs, deleted_sites, unknown_sites, other_sites, first_site, last_site; } uvaia_align_row_qc;
/* src/align.c:366-390: derive the records and counts of the rows of the following runs of this aligner (uvaia_align_run / _sync / _batch,
 * whichever way the pool was loaded) on the device, after the projection (off by default; rows, scores, insertions and the statistics are
 * the same either way). */
int  uvaia_align_set_variants (uvaia_aligner *a, int on);
/* src/align.c:366-390: how many records and rows the last answer holds: that of the last completed run with the option on, or of
 * uvaia_align_variants_of, whichever came last.  UVAIA_ALIGN_ESTATE before either has happened, and after a load or a run with the option
 * off that followed a run's answer.  Either pointer may be NULL. */
int  uvaia_align_variant_counts (uvaia_aligner *a, long long *n_records, int *n_rows);
/* src/align.c:366-390: the n_records records, sorted by (query, ref_pos) as the device wrote them, and the n_rows counts; either may be NULL.
 * UVAIA_ALIGN_ESTATE as above. */
int  uvaia_align_fetch_variants (uvaia_aligner *a, uvaia_align_variant *rec, uvaia_align_row_qc *qc);
/* src/align.c:366-390, for rows aligned elsewhere: n rows of ref_len bytes in host memory, pitch >= ref_len bytes apart, are copied to a
 * buffer of the aligner's own and go through the same passes, whether or not the option is on.  The loaded pool, its rows, scores and
 * insertions are not touched.  n == 0 is an empty answer; pitch < ref_len, n < 0 and n > 0 with NULL rows are refused with
 * UVAIA_ALIGN_EINVAL. */
int  uvaia_align_variants_of (uvaia_aligner *a, const char *rows, size_t pitch, int n);
/* src/align.c:366-390: device time in ms of the passes since the aligner was opened or since the last call with reset != 0 (the count is
 * reset after it is read).  It is NOT part of the kernel_ms of uvaia_align_stats. */
double uvaia_align_variants_ms (uvaia_aligner *a, int reset);

/* work of the last run: M-wavefront cells computed, wavefront bytes written + read by the recurrences (13 + 20 per cell),
 * kernel passes (queries that find the workspace's pool empty are run again in a less crowded pass), kernel time in ms */
int  uvaia_align_stats (uvaia_aligner *a, unsigned long long *cells, double *wavefront_bytes, int *passes, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif
