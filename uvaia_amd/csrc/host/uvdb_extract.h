/*
 * uvdb_extract.h -- the text of references at given positions of a set of packed databases (uvdb_set.h), decoded on the GPU straight out
 * of a staging slot (uvaia_gpu_db_stage_unpack_rows, include/uvaia_gpu.h): what `uvaia --packed --final-aln` and `uvaiapack --unpack`
 * write.  Own code, no counterpart in the reference, whose README (lines 266-293) sends users through xzcat | cut | sort | uniq and
 * `seqkit grep` for the same rows because a text stream has no second look at a row.
 *
 * Also here: the one copy of the staging of a range of a set (dense and compact files, a set may mix both), which the resident and the
 * windowed search of nearest_main.c, the merge loop of pack_main.c and the extraction use.
 */
#ifndef UVAIA_HOST_UVDB_EXTRACT_H
#define UVAIA_HOST_UVDB_EXTRACT_H

#include <stddef.h>
#include <stdint.h>

#include "uvdb_set.h"
#include "../../../include/uvaia_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UVDB_EXTRACT_CHUNK 256           /* positions decoded per round; a chunk never needs more than this many tiles of a slot */

enum { UVDB_STAGE_OK = 0, UVDB_STAGE_ESPAN = 1, UVDB_STAGE_EGPU = 2 };

/* pieces[0 .. n_pieces) into staging slot `slot`: whole tiles of their files, a dense file's as they are mapped, a compact file's
 * expanded in the slot.  UVDB_STAGE_OK, or UVDB_STAGE_EGPU with the engine's message in uvaia_gpu_last_error (gpu). */
int uvdb_stage_pieces (uvaia_gpu_ctx *gpu, uvdb_set set, int slot, const uvdb_set_piece *pieces, int n_pieces);

/* Kept positions [a, b) into staging slot `slot` as uvdb_set_span cuts them (per file one piece from its first to its last kept
 * reference of the range); pieces: UVDB_SET_MAX_FILES entries of scratch; sel (may be NULL; b - a entries) receives their positions
 * within the slot.  *identity (may be NULL): whether these are 0, 1, 2, ... for certain -- no keep list, one piece, the first at lane 0.
 * UVDB_STAGE_ESPAN: the range spans more file tiles than the engine counts. */
int uvdb_stage_range (uvaia_gpu_ctx *gpu, uvdb_set set, const uint64_t *keep, uint64_t a, uint64_t b, int slot, uvdb_set_piece *pieces, int *sel, int *identity);

/* The plan of one chunk of an extraction.  pos[a .. b) (pos == NULL: the stream positions a .. b - 1 themselves) are stream positions,
 * strictly ascending, b - a <= max_pieces.  Only the tiles that hold one of them are staged: consecutive tiles of a file form one piece,
 * the pieces follow each other in the slot, so a chunk needs at most b - a tiles however far apart its positions lie.
 * pieces[0 .. *n_pieces), *slot_tiles, sel[0 .. b - a) = position of each within the slot (strictly ascending).  pieces and sel may be
 * NULL to count.  0, or -1 for an empty range, a position outside the stream, positions that do not ascend (a repeat included) and more
 * pieces than max_pieces.  Pure host arithmetic. */
int uvdb_extract_plan (uvdb_set set, const uint64_t *pos, uint64_t a, uint64_t b, uvdb_set_piece *pieces, int max_pieces, int *n_pieces, uint64_t *slot_tiles, int *sel);

/* called once per position, in order: k = index into pos, stream = stream position, the stored name, the NUL-terminated upper-case row with
 * the exception runs put back.  A return value other than 0 ends the extraction (uvdb_extract then returns -1). */
typedef int (*uvdb_extract_fn) (void *user, uint64_t k, uint64_t stream, const char *name, const char *row);

typedef struct {
  uint64_t n_rows, n_chunks, n_pieces, n_tiles;            /* rows handed over; chunks; staging calls; tiles staged */
  double stage_ms, decode_ms, kernel_ms, exceptions_ms, write_ms;   /* wall time of the staging calls, of the decode calls (kernel and copy back), device
                                                              time of the decode kernel in them, wall time of the exception runs and of the callbacks */
} uvdb_extract_stats;

/* Rows pos[0 .. n) (pos == NULL: the whole stream, n = set->n_ref) of the set through `gpu`, a plain context (no reference shard) of the set's
 * alignment length and tile layout, whose search state and resident database are left as they are.  Chunks of UVDB_EXTRACT_CHUNK
 * positions: chunk k + 1 is staged into the other slot before chunk k is decoded, so its copy overlaps the decode, the exceptions and
 * the callbacks.  Host memory: one chunk of rows, two of selections and pieces.  Repeated positions are refused.  stats (may be NULL)
 * is added to.  0, or -1 with a message in errbuf. */
int uvdb_extract (uvdb_set set, uvaia_gpu_ctx *gpu, const uint64_t *pos, uint64_t n, uvdb_extract_fn fn, void *user, uvdb_extract_stats *stats, char *errbuf, size_t errlen);

/* ---- a list of names (`uvaiapack --unpack --names <file>`): one per line, a trailing carriage return dropped, empty lines skipped,
 * repeated lines counted once */
typedef struct uvdb_name_list_struct {
  size_t n;
  char **name;                           /* sorted (strcmp), distinct; point into text */
  uint64_t *hits;                        /* references found under each name (uvdb_name_list_find counts) */
  char *text;
} *uvdb_name_list;

uvdb_name_list uvdb_name_list_from_text (const char *text, size_t len);      /* NULL: out of memory */
uvdb_name_list uvdb_name_list_read (const char *filename, char *errbuf, size_t errlen);
/* index of `name` in the list and one more hit for it, or -1 */
long uvdb_name_list_find (uvdb_name_list l, const char *name);
void uvdb_name_list_free (uvdb_name_list l);

#ifdef __cplusplus
}
#endif
#endif
