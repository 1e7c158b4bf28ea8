/*
 * uvdb_set.h -- several packed databases (uvdb.h) read as ONE stream of references, in command-line order: the files of a repeated
 * `--packed` of uvaia, uvaiaball and uvaiaclust and the inputs of `uvaiapack --merge`.  Own code; it stands where the reference walks its
 * list of -r files (src/nearest.c:245, src/ball.c:174, src/cluster.c:150).  Pure host arithmetic over the mapped files, no GPU.
 *
 * A stream index counts the references of file 0, then those of file 1, and so on (a file may hold none).  Positions of the KEPT stream are
 * as in uvdb_window.h: keep[i] = stream index of the i-th kept reference, increasing; keep == NULL = every reference is kept.
 */
#ifndef UVAIA_HOST_UVDB_SET_H
#define UVAIA_HOST_UVDB_SET_H

#include <stddef.h>
#include <stdint.h>

#include "uvdb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UVDB_SET_MAX_FILES 1024          /* as the reference's -r (src/nearest.c:67) */
#define UVDB_SET_ANY_AMBIGUITY 1         /* uvdb_set_open: the files may have been filtered with different -A (uvaiapack --merge -A) */

typedef struct uvdb_set_struct {
  int n_files;
  uvdb_reader *db;                       /* the readers, in order */
  char **filename;
  uint64_t *first;                       /* n_files + 1 entries: stream index of a file's first reference; first[n_files] = n_ref */
  uint64_t n_ref;
  /* what all files agree on (ref_ambiguity: the LARGEST value, i.e. the loosest filter, when UVDB_SET_ANY_AMBIGUITY let them differ) */
  uint32_t nchar, side_row_ints; uint64_t tile_bytes; double ref_ambiguity;
} *uvdb_set;

/* Opens the files in order.  All must agree on nchar, tile_bytes, side_row_ints and (without UVDB_SET_ANY_AMBIGUITY) ref_ambiguity;
 * otherwise NULL and a message in errbuf that names both files, as for a file uvdb_open refuses (its message). */
uvdb_set uvdb_set_open (const char *const *filenames, int n_files, int flags, char *errbuf, size_t errlen);
void uvdb_set_close (uvdb_set s);

/* stream index -> file and position within it; 0, or -1 for an index outside the stream */
int uvdb_set_locate (uvdb_set s, uint64_t i, int *file, uint64_t *local);
/* by stream index, as the calls of uvdb.h by file position */
const char *uvdb_set_name (uvdb_set s, uint64_t i);
int32_t uvdb_set_non_n (uvdb_set s, uint64_t i);
void uvdb_set_apply_exceptions (uvdb_set s, uint64_t i, char *row);
void uvdb_set_unpack_reference (uvdb_set s, uint64_t i, char *out);
/* exception runs of reference i as the file holds them: *runs points into the mapping; returns their number */
size_t uvdb_set_runs (uvdb_set s, uint64_t i, const uvdb_exc **runs);

/* A piece of a staging slot: n_tiles whole tiles of `file` from first_tile on, which land at tile slot_tile of the slot
 * (uvaia_gpu_db_stage_packed_at; uvaia_gpu_db_stage_compact_at for a file of version 2). */
typedef struct { int file; uint64_t first_tile, n_tiles, slot_tile; } uvdb_set_piece;

/* The multi-file form of uvdb_window_span.  Kept-stream positions [a, b), a < b: per file that holds some of them, the contiguous tiles
 * from its first to its last kept reference of the range, as one piece; the pieces follow each other in the slot in file order.
 * pieces[0 .. *n_pieces) (pieces may be NULL to count; otherwise max_pieces entries, UVDB_SET_MAX_FILES always suffice), *slot_tiles = tiles
 * of the slot in use, sel_out[0 .. b - a) (may be NULL) = position of each kept reference within the slot -- strictly increasing, below
 * 64 * *slot_tiles.  0, or -1 for an empty range, a keep entry outside the stream or not increasing, more pieces than max_pieces, and a
 * slot beyond what an int counts. */
int uvdb_set_span (uvdb_set s, const uint64_t *keep, uint64_t a, uint64_t b, uvdb_set_piece *pieces, int max_pieces, int *n_pieces, uint64_t *slot_tiles, int *sel_out);

/* Whether kept positions [a, b) of the n kept can go into a resident store of `store` references as whole tiles straight from a mapping
 * (uvaia_gpu_db_append_packed: whole tiles behind whole tiles), without staging or gathering.  Yes (0, and *file, *first_tile: the b - a
 * references are the first of the tiles of that file from first_tile on) when nothing is left out (keep == NULL, n = references of the
 * stream), the range lies in one file and starts at lane 0 of one of its tiles, b - a is a multiple of 64 or b == n (the stream ends with
 * the range, so the lanes behind it in its last tile are the file's padding), store is a multiple of 64, and the file holds dense tiles
 * (version 1: the tiles of a compact file exist only once they are expanded in a staging slot).  Otherwise -1, as for an empty range and
 * for one past the stream. */
int uvdb_set_direct_tiles (uvdb_set s, const uint64_t *keep, uint64_t a, uint64_t b, uint64_t n, uint64_t store, int *file, uint64_t *first_tile);

#ifdef __cplusplus
}
#endif
#endif
