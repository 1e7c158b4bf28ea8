/*
 * uvdb_packer.h -- a packed database (uvdb.h) written from rows that lie in device memory: what `uvaialign --packed` does with the rows of
 * the aligner and `uvaiaclust --packed-out` with the medoid rows of the clusterer.  The file is the one `uvaiapack` writes from the same rows
 * as text: census, -A filter, packing and exception runs happen on the rows where they lie (include/uvaia_gpu.h, "rows that are already in
 * device memory").  Own code, no counterpart in the reference.
 */
#ifndef UVAIA_HOST_UVDB_PACKER_H
#define UVAIA_HOST_UVDB_PACKER_H

#include <stddef.h>
#include <stdint.h>

#include "uvdb.h"
#include "../../../include/uvaia_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UVDB_PACK_BATCH 4096      /* kept rows per engine round trip (a multiple of 64), as in pack_main.c */

/* The head of a packed database in the making.  A tile holds 64 consecutive kept rows of the whole stream, the caller's blocks end anywhere:
 * the resident database of the engine is the carry.  Rows are appended to it as they come, whole tiles are exported and dropped, the
 * unfinished tile stays resident for the next block (or the flush at the end), so that the file does not depend on how the rows are cut. */
/* The one step that moves resident tiles from an engine to a writer, for every command that writes a packed database.  A dense writer, and a
 * compact one whose base is not fixed yet, take dense tiles (uvaia_gpu_db_export + uvdb_add_tiles: the compact writer encodes them on the
 * host); a compact writer with a fixed base takes the records the engine encodes against that base (uvaia_gpu_db_encode_compact +
 * uvaia_gpu_db_encoded_records + uvdb_add_tiles_encoded), a twelfth of the bytes.  The file is the same either way.  A zeroed struct is
 * ready for use; the buffers grow on demand. */
struct uvdb_export {
  void *planes; int *non_n, *side; size_t cap_tiles;   /* dense tiles, and the counts of either route */
  uint64_t *head_idx, *lit_idx; uint32_t *heads, *lits; size_t heads_cap, lits_cap;   /* records (lits_cap in words of 16 bytes) */
  long tiles_device, tiles_host;                       /* tiles by route: encoded on the device, handed over dense */
  char err[640];
};
/* tiles first_tile .. first_tile + n_tiles - 1 of the engine's resident database to the writer; 0, or -1 with the message in x->err */
int uvdb_export_tiles (struct uvdb_export *x, uvaia_gpu_ctx *gpu, uvdb_writer w, size_t first_tile, size_t n_tiles);
void uvdb_export_free (struct uvdb_export *x);

struct uvdb_packer {
  uvaia_gpu_ctx *gpu;
  uvdb_writer w;
  int nchar, non_n_ref;
  struct uvdb_export exp;                              /* export buffers, tiles by route */
  int *non_n, *n_exc, *ident, *keep; size_t block_cap; /* per row of a block: census counts, rows 0 .. n - 1, the rows the filter keeps */
  int *sel, *sel_nn;                                   /* per row of a batch: its place in the block, its valid sites */
  uint64_t *off; uvdb_exc *exc; size_t exc_cap;
  long kept, dropped;
  double rows_ms[3];                                   /* device time, filled by close: census, gathers, exception fill */
  int compact; long tiles_device, tiles_host;          /* a version 2 file; filled by close: tiles encoded on the device, handed over dense */
  double encode_ms[2];                                 /* device time, filled by close: count + prefix, emit (uvaia_gpu_encode_ms) */
  char err[640];
};

/* every function: 0, or -1 with the message in p->err.  ambig_r: the -A filter, recorded in the header (rows with fewer than
 * (int) (nchar * (1 - ambig_r)) valid sites are dropped); block_cap: the most rows a call below hands in; compact: write version 2 of
 * the format (refused for nchar > UVDB_COMPACT_MAX_NCHAR). */
int uvdb_packer_open (struct uvdb_packer *p, const char *path, int nchar, double ambig_r, int device, int block_cap, int compact);
/* a block of n rows in the memory of the packer's device (d_rows + i * pitch): census, filter, append; name[i] belongs to row i */
int uvdb_packer_add_block (struct uvdb_packer *p, const void *d_rows, size_t pitch, int n, char *const *name);
/* the same for rows row[0 .. n) of a block, in that order, whose counts the caller took with uvaia_gpu_rows_census (p->gpu): non_n[k],
 * n_exc[k] and name[k] belong to row[k] */
int uvdb_packer_add_rows (struct uvdb_packer *p, const void *d_rows, size_t pitch, const int *row, const int *non_n, const int *n_exc, char *const *name, int n);
/* the unfinished tile, the index sections, the engine; 0 when the file is complete */
int uvdb_packer_close (struct uvdb_packer *p);

#ifdef __cplusplus
}
#endif
#endif
