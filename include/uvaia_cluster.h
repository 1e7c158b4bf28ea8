/*
 * uvaia_cluster.h -- C ABI of the MI355X (gfx950) one-pass canopy clustering behind `uvaiaclust`.
 *
 * What the reference's src/cluster.c computes (main 117-245, with src/fastaseq.c:127-260 and 522-560), restated from its code
 * and not from its comments ("uvaiaclust", has the derivation; tests/cluster_restatement.c is the CPU restatement):
 *
 *   1. The site tables of src/utils.c:255-295 are never initialised by this program (initialise_acgt() is only called by the
 *      query structure of uvaia/uvaiaball), so every pair of non-NUL bytes is "valid": every distance is the plain byte
 *      inequality count.  'N' against 'A' counts, '-' against '-' does not.  The non-N count is the sequence length.
 *   2. Hence the medoid-replacement test of add_seq_to_cluster (src/fastaseq.c:182) never holds: a cluster's medoid is its
 *      first member, in both phases.
 *   3. Phase 2 (check_seq_against_cluster, src/fastaseq.c:140-170), per queue, in push order.  A sequence's distance r to the
 *      reference over the trimmed sites [trim, nchar - trim) and the positions p[0..n_score) of its first n_score differences
 *      (relative to trim, -1 where there are fewer) are its scores.  Its candidates are, in medoid creation order: the first
 *      medoid i1 with |r - stored(i1)| <= dist, then every later medoid i with 1 <= stored(i) <= 2 dist + 1 (score[0] is
 *      overwritten by the truncated distance dist + 1 after the first failed comparison, src/fastaseq.c:158).  The first
 *      candidate within dist wins; with none, the sequence founds a cluster and stores dist + 1 if any comparison happened,
 *      else r.
 *   4. The comparison window of phase 2 is [trim + m, nchar - trim + m) with m = max(0, min(p0_s, p0_medoid) - 1) (0 when
 *      n_score is 0): the trimmed distance plus the differences in the tail [nchar - trim, nchar - trim + m).  Sites >= nchar
 *      never count (the reference reads past the buffer there: undefined, so this is a defined choice).
 *   5. The merge distance (merge_clusters, src/fastaseq.c:196-258) is the trimmed distance: equal, for the <= dist decision, to
 *      the reference's count over the sites where any sequence differed from the reference.
 *   6. The merge tree is for (c = Q; c > 1; c = c/2 + c%2): queue j < c/2 absorbs queue j + c/2 + c%2.  Both lists are stably
 *      sorted by their score vectors, descending.  Each cluster of the absorbed list joins the first cluster of the other list
 *      (sorted order, original clusters only) with |delta stored| <= dist and distance <= dist: its medoid, then its members,
 *      are appended to that cluster's members.  Otherwise it is appended to the list.
 *   7. The final order is the stable sort of queue 0 by member count descending, then the score vectors descending.
 *   Defined choices where the reference has none: an empty absorbed queue merges as a no-op (the reference dereferences the
 *   first element of the empty list) and an empty absorbing queue takes the other list as it is sorted; the out-of-bounds
 *   write of src/fastaseq.c:160 has no effect; bytes 0 and >= 0x80 are refused (they index the site tables out of range).
 *
 * Conventions: plain C; 0 on success or a negative UVAIA_GPU_E* code, never exit(); uvaia_clust_last_error() gives the
 * message.  One context = one GPU = one host thread at a time.  There is no CPU path: uvaia_clust_open fails with
 * UVAIA_GPU_ENODEV without a gfx950 device.  Lower-case letters are upper-cased on the device (upper_kseq, src/fastaseq.c:151).
 */
#ifndef UVAIA_CLUSTER_H
#define UVAIA_CLUSTER_H

#include <stddef.h>
#include <stdint.h>

#include "uvaia_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct uvaia_clust_ctx uvaia_clust_ctx;

/* new_cqueue (src/cluster.c:280-300) with its clamps already applied by the caller (dist <= nchar / 10, trim <= nchar / 2.1,
 * negative values 0): the reference sequence (nchar bytes), the distance, the trim, n_score (-s) and the number of queues. */
int  uvaia_clust_open (uvaia_clust_ctx **out, int device, const char *reference, int nchar, int dist, int trim, int n_score, int n_queues);
void uvaia_clust_close (uvaia_clust_ctx *c);
const char *uvaia_clust_last_error (const uvaia_clust_ctx *c);

/* The second residency mode, "keep medoids": call it after uvaia_clust_open and before the first push (UVAIA_GPU_ESTATE once a sequence was
 * pushed).  By default every pushed row stays in device memory as text, nchar rounded up to 64 bytes each, in one array that grows by
 * doubling (the old and the new array exist together while it grows).  After phase 2 has placed a sequence its text is read again only if
 * it founded a cluster (item 2: the medoid is the first member), so in this mode only those rows are kept: the rows of a push land in a
 * staging buffer of that push's size, and its founders are copied into slabs of slab_rows rows each, which are added one at a time and never
 * moved.  Device memory for row text is then bounded by (clusters founded in phase 2, rounded up to whole slabs) + (the largest push), and
 * no longer by the number of sequences; 16 bytes + 4 n_score bytes per pushed sequence (its scores, join and slot) still stay.
 * slab_rows: 0 = the default (65 536 rows, a design choice that has not been measured), else a power of two >= 1, or UVAIA_GPU_EINVAL.
 * Clusters, member lists and scores are those of the default mode for the same pushes; push, push_packed, finish, result and stats keep
 * their contracts.  What changes: uvaia_clust_rows answers for founders only, uvaia_clust_device_rows has no store to hand out. */
int  uvaia_clust_keep_medoids (uvaia_clust_ctx *c, int slab_rows);

/* Phase 2 for n sequences of nchar bytes each (seq[i]); queue[i] in [0, n_queues) is the queue sequence i goes to.  Within a
 * queue the order is push order.  Sequences are numbered by push ordinal from 0 across all calls.  A byte 0 or >= 0x80 fails
 * the call with UVAIA_GPU_EALPHABET and leaves the context unusable (UVAIA_GPU_ESTATE afterwards). */
int  uvaia_clust_push (uvaia_clust_ctx *c, int n, const char *const *seq, const int *queue);

/* The same for n sequences whose text is not on the host: ceil(n / 64) whole tiles of the packed interchange form (include/uvaia_gpu.h:
 * [word group][plane A,C,G,T][lane] 16-byte words, ((nchar + 31) / 32 + 3) / 4 * 4096 bytes per tile, the formula of
 * uvaia_gpu_db_tile_bytes; lanes past n in the last tile are ignored whatever they hold) and their exception runs, as a packed database
 * file holds both (uvaia_amd/csrc/host/uvdb.h).  The records of sequence i are exc[exc_offsets[i] .. exc_offsets[i + 1]) (n + 1 offsets, so
 * a file's exc_idx + first sequence and its exc array can be handed in as they are; exc_offsets NULL = no records), each (uint32 pos,
 * uint32 len << 8 | char).  The device rebuilds the exact upper-case text of every row -- per site the IUPAC character of the set the planes
 * hold, 'N' for the empty and the full set, then the runs written over it -- before any distance is taken: the planes alone cannot tell
 * N - ? X O . apart, and item 1 above counts '-' against 'N' as a difference.  Push ordinals, queues and errors are those of
 * uvaia_clust_push, both kinds of push may be mixed in one context and the result does not depend on how the sequences are cut into
 * pushes.  A record with a character other than - ? X O . , with pos + len > nchar, or that starts before the end of the row's previous
 * record fails the call with UVAIA_GPU_EINVAL before anything is copied: nothing is pushed and the context stays usable. */
int  uvaia_clust_push_packed (uvaia_clust_ctx *c, int n, const void *planes, const uint64_t *exc_offsets, const void *exc, const int *queue);

/* The same for n sequences whose text is already in the memory of the context's device (what the FASTA parser leaves behind,
 * uvaia_gpu_fasta_rows of include/uvaia_gpu.h; a tensor of the caller): replaces, for such rows, the host copy of uvaia_clust_push -- every
 * row into a padded host block and over the bus.  Sequence i of the push is row row_index[i] of the block (NULL: row i), the nchar bytes at
 * d_rows + row * pitch.  The block has the contract of uvaia_gpu_db_append_device: any pitch >= nchar, any alignment, and the pointer is
 * checked the same way before anything reads it.  Push ordinals, queues, the byte check (UVAIA_GPU_EALPHABET by push ordinal, the context
 * unusable afterwards) and keep-medoids staging are those of uvaia_clust_push; the three kinds of push may be mixed in one context and the
 * result does not depend on how the sequences are cut into pushes.  A host pointer, another device's memory, a block that ends beyond its
 * allocation, a negative row or a pitch below nchar fails the call with UVAIA_GPU_EINVAL before anything is launched: nothing is pushed and
 * the context stays usable.  Returns when the rows have been read and placed. */
int  uvaia_clust_push_device (uvaia_clust_ctx *c, int n, const void *d_rows, size_t pitch, const int *row_index, const int *queue);

/* The upper-case text of pushed sequences, before or after finish: row k of `rows` (pitch >= nchar bytes apart, nchar bytes written, no
 * NUL) = the sequence with push ordinal ordinal[k]; any order, repeats allowed.  Gathered on the device, one copy back per call: the caller
 * bounds its memory by the n of a call (the medoids of <prefix>.aln.xz are fetched in batches).
 * Keep medoids: every ordinal must be a sequence that founded a cluster in phase 2 -- the medoids of the result, and the founders the merge
 * tree absorbed into another cluster since; the bytes are those of the default mode.  Any other ordinal fails the call with
 * UVAIA_GPU_EINVAL before anything is copied, and the context stays usable. */
int  uvaia_clust_rows (uvaia_clust_ctx *c, const int64_t *ordinal, int n, char *rows, size_t pitch);

/* The row store where it lies: sequence o is the nchar bytes at *d_rows + o * *pitch in the memory of the context's device, upper-case
 * (uvaia_gpu_rows_census, uvaia_gpu_db_append_device and uvaia_gpu_rows_exceptions of include/uvaia_gpu.h read medoid rows in place,
 * row_index = push ordinals).  Valid until the next push or close.  Keep medoids: UVAIA_GPU_ESTATE, there is no such array; use
 * uvaia_clust_gather_device. */
int  uvaia_clust_device_rows (uvaia_clust_ctx *c, const void **d_rows, size_t *pitch);

/* Rows in device memory, in either mode: the rows of ordinal[0 .. n) (the ordinals uvaia_clust_rows accepts; any order, repeats allowed)
 * gathered into the context's gather buffer, row k = the nchar bytes at *d_rows + k * *pitch, upper-case, so that uvaia_gpu_rows_census,
 * uvaia_gpu_db_append_device and uvaia_gpu_rows_exceptions read them with row_index = 0 .. n - 1.  Valid until the next call on the context
 * (uvaia_clust_rows uses the same buffer).  n = 0: *d_rows NULL.  The caller bounds the buffer by the n of a call. */
int  uvaia_clust_gather_device (uvaia_clust_ctx *c, const int64_t *ordinal, int n, const void **d_rows, size_t *pitch);

/* Device memory (each pointer nullable): *row_bytes = bytes held for row text now -- the row store, or the slabs and the staging buffer --
 * *peak_row_bytes = the most they have been at once (the default mode's store holds old + new capacity while it grows), *free_bytes = the
 * free memory of the context's device as the runtime reports it. */
int  uvaia_clust_memory (uvaia_clust_ctx *c, size_t *row_bytes, size_t *peak_row_bytes, size_t *free_bytes);

/* The merge tree and the final order.  No push after it. */
int  uvaia_clust_finish (uvaia_clust_ctx *c);

/* After finish: the number of clusters, and (each array nullable, sized by the caller)
 *   medoid  [n_clusters]                   push ordinal of each cluster's medoid, in the final order
 *   offsets [n_clusters + 1]               members of cluster k are members[offsets[k] .. offsets[k + 1])
 *   members [pushed - n_clusters]          push ordinals of the other members, in member-list order (the csv line after the medoid)
 *   scores  [n_clusters * (n_score + 2)]   the stored score vectors: stored distance, p[0..n_score), nchar */
int  uvaia_clust_result (uvaia_clust_ctx *c, int *n_clusters, int64_t *medoid, int64_t *offsets, int64_t *members, int *scores);

/* Kernel milliseconds of each phase so far: prep (distance to the reference), queue (phase 2), merge (the tree), and the
 * number of sequences pushed. */
int  uvaia_clust_stats (uvaia_clust_ctx *c, double *prep_ms, double *queue_ms, double *merge_ms, int64_t *pushed);

/* Kernel milliseconds of the packed pushes so far: decoding the tiles to rows, writing the exception runs over them. */
int  uvaia_clust_unpack_ms (uvaia_clust_ctx *c, double *decode_ms, double *overlay_ms);

/* Kernel milliseconds of the device pushes so far: copying the rows out of the caller's block. */
int  uvaia_clust_push_device_ms (uvaia_clust_ctx *c, double *rows_in_ms);

#ifdef __cplusplus
}
#endif
#endif
