/* uvdb_packer.c -- see uvdb_packer.h */
#include "uvdb_packer.h"

#include <stdlib.h>
#include <string.h>

#include "biomcmc_lite.h"

static int
packer_fail_gpu (struct uvdb_packer *p)
{
  snprintf (p->err, sizeof p->err, "%s", uvaia_gpu_last_error (p->gpu));
  return -1;
}

static int
export_room (struct uvdb_export *x, size_t n_tiles, size_t tile_bytes, int dense)
{
  if (n_tiles > x->cap_tiles) {
    free (x->planes); free (x->side); x->planes = NULL; x->side = NULL;       /* (made below for the route that needs them) */
    x->non_n = (int *) realloc (x->non_n, n_tiles * 64 * sizeof (int));
    x->head_idx = (uint64_t *) realloc (x->head_idx, (n_tiles * 64 + 1) * sizeof (uint64_t));
    x->lit_idx = (uint64_t *) realloc (x->lit_idx, (n_tiles * 64 + 1) * sizeof (uint64_t));
    if (!x->non_n || !x->head_idx || !x->lit_idx) return -1;
    x->cap_tiles = n_tiles;
  }
  if (dense && !x->planes) {
    x->planes = malloc (x->cap_tiles * tile_bytes);
    x->side = (int *) malloc (x->cap_tiles * 64 * (size_t) uvaia_gpu_db_side_row_ints () * sizeof (int));
    if (!x->planes || !x->side) return -1;
  }
  return 0;
}

int
uvdb_export_tiles (struct uvdb_export *x, uvaia_gpu_ctx *gpu, uvdb_writer w, size_t first_tile, size_t n_tiles)
{
  if (!n_tiles) return 0;
  const uint32_t *base = uvdb_compact_base (w);
  if (export_room (x, n_tiles, uvaia_gpu_db_tile_bytes (gpu), base == NULL)) { snprintf (x->err, sizeof x->err, "out of memory for %zu tiles on their way to the packed database", n_tiles); return -1; }
  if (!base) {      /* a dense writer, or a compact one that still collects the sample its base is the majority of */
    if (uvaia_gpu_db_export (gpu, first_tile, n_tiles, x->planes, x->non_n, x->side)) { snprintf (x->err, sizeof x->err, "%s", uvaia_gpu_last_error (gpu)); return -1; }
    if (uvdb_add_tiles (w, n_tiles, x->planes, x->non_n, x->side)) { snprintf (x->err, sizeof x->err, "cannot write the packed database"); return -1; }
    x->tiles_host += (long) n_tiles;
    return 0;
  }
  if (uvaia_gpu_db_encode_compact (gpu, first_tile, n_tiles, base, x->head_idx, x->lit_idx, x->non_n)) { snprintf (x->err, sizeof x->err, "%s", uvaia_gpu_last_error (gpu)); return -1; }
  const uint64_t nh = x->head_idx[n_tiles * 64], nl = x->lit_idx[n_tiles * 64];
  if (nh > x->heads_cap) {
    free (x->heads); x->heads_cap = 0;
    x->heads = (uint32_t *) malloc ((size_t) nh * 2 * sizeof (uint32_t));
    if (!x->heads) { snprintf (x->err, sizeof x->err, "out of memory for %llu compact heads", (unsigned long long) nh); return -1; }
    x->heads_cap = (size_t) nh * 2;
  }
  if (nl > x->lits_cap) {
    free (x->lits); x->lits_cap = 0;
    x->lits = (uint32_t *) malloc ((size_t) nl * 2 * 16);
    if (!x->lits) { snprintf (x->err, sizeof x->err, "out of memory for %llu compact literal words", (unsigned long long) nl); return -1; }
    x->lits_cap = (size_t) nl * 2;
  }
  if (uvaia_gpu_db_encoded_records (gpu, x->heads, x->lits)) { snprintf (x->err, sizeof x->err, "%s", uvaia_gpu_last_error (gpu)); return -1; }
  if (uvdb_add_tiles_encoded (w, n_tiles, x->non_n, x->head_idx, x->heads, x->lit_idx, x->lits)) { snprintf (x->err, sizeof x->err, "cannot write the packed database (or the device's compact records do not pass the writer's checks)"); return -1; }
  x->tiles_device += (long) n_tiles;
  return 0;
}

void
uvdb_export_free (struct uvdb_export *x)
{
  free (x->planes); free (x->non_n); free (x->side); free (x->head_idx); free (x->lit_idx); free (x->heads); free (x->lits);
  x->planes = NULL; x->non_n = x->side = NULL; x->head_idx = x->lit_idx = NULL; x->heads = x->lits = NULL;
  x->cap_tiles = x->heads_cap = x->lits_cap = 0;
}

int
uvdb_packer_open (struct uvdb_packer *p, const char *path, int nchar, double ambig_r, int device, int block_cap, int compact)
{
  memset (p, 0, sizeof *p);
  if (compact && nchar > UVDB_COMPACT_MAX_NCHAR) { snprintf (p->err, sizeof p->err, "--compact: alignments of more than %d sites have no compact form (%d sites)", UVDB_COMPACT_MAX_NCHAR, nchar); return -1; }
  p->nchar = nchar; p->compact = compact;
  p->non_n_ref = (int) (nchar * (1. - ambig_r));       /* src/nearest.c:263-268, as pack_main.c */
  char *dummy = (char *) biomcmc_malloc ((size_t) nchar + 1);   /* the engine needs some query to exist: a plain ACGT string */
  for (int s = 0; s < nchar; s++) dummy[s] = "ACGT"[s & 3];
  dummy[nchar] = '\0';
  const char *one[1] = {dummy};
  uvaia_gpu_query q;
  memset (&q, 0, sizeof q);
  q.n_query = 1; q.nchar = nchar; q.seq = one; q.consensus = dummy;
  const int rc = uvaia_gpu_open (&p->gpu, &q, 1, device, UVDB_PACK_BATCH);
  free (dummy);
  if (rc) { snprintf (p->err, sizeof p->err, "%s", uvaia_gpu_last_error (NULL)); return -1; }
  if (uvaia_gpu_db_reserve (p->gpu, UVDB_PACK_BATCH + 64)) return packer_fail_gpu (p);
  const size_t tb = uvaia_gpu_db_tile_bytes (p->gpu);
  p->block_cap = (size_t) block_cap;
  p->non_n = (int *) biomcmc_malloc (p->block_cap * sizeof (int)); p->n_exc = (int *) biomcmc_malloc (p->block_cap * sizeof (int));
  p->ident = (int *) biomcmc_malloc (p->block_cap * sizeof (int)); p->keep = (int *) biomcmc_malloc (p->block_cap * sizeof (int));
  for (int i = 0; i < block_cap; i++) p->ident[i] = i;
  p->sel = (int *) biomcmc_malloc (UVDB_PACK_BATCH * sizeof (int)); p->sel_nn = (int *) biomcmc_malloc (UVDB_PACK_BATCH * sizeof (int));
  p->off = (uint64_t *) biomcmc_malloc ((UVDB_PACK_BATCH + 1) * sizeof (uint64_t));
  p->w = compact ? uvdb_create_compact (path, nchar, tb, uvaia_gpu_db_side_row_ints (), ambig_r) : uvdb_create (path, nchar, tb, uvaia_gpu_db_side_row_ints (), ambig_r);
  if (!p->w) { snprintf (p->err, sizeof p->err, "cannot create %s", path); return -1; }
  return 0;
}

/* whole tiles (all = 0) or everything that is resident (all = 1: the flush) from the engine to the file */
static int
packer_write_tiles (struct uvdb_packer *p, int all)
{
  const size_t have = uvaia_gpu_db_size (p->gpu), nt = all ? (have + 63) / 64 : have / 64;
  if (!nt) return 0;
  if (uvdb_export_tiles (&p->exp, p->gpu, p->w, 0, nt)) { snprintf (p->err, sizeof p->err, "%s", p->exp.err); return -1; }
  if (uvaia_gpu_db_drop_tiles (p->gpu, nt)) return packer_fail_gpu (p);
  return 0;
}

int
uvdb_packer_add_rows (struct uvdb_packer *p, const void *d_rows, size_t pitch, const int *row, const int *non_n, const int *n_exc, char *const *name, int n)
{
  if (n < 0 || (size_t) n > p->block_cap) { snprintf (p->err, sizeof p->err, "%d rows in one call, the packer was opened for %zu", n, p->block_cap); return -1; }
  int nk = 0;
  for (int i = 0; i < n; i++) {                        /* the -A filter (pack_main.c:86-87) on a few KB of counts */
    if (non_n[i] < p->non_n_ref) { p->dropped++; continue; }
    p->keep[nk++] = i;
  }
  for (int a = 0; a < nk; a += UVDB_PACK_BATCH) {
    const int m = nk - a < UVDB_PACK_BATCH ? nk - a : UVDB_PACK_BATCH;
    p->off[0] = 0;
    for (int k = 0; k < m; k++) {
      const int i = p->keep[a + k];
      p->sel[k] = row[i]; p->sel_nn[k] = non_n[i];
      p->off[k + 1] = p->off[k] + (uint64_t) n_exc[i];
    }
    if (p->off[m] + 1 > p->exc_cap) {
      p->exc_cap = (size_t) (p->off[m] + 1) * 2;
      p->exc = (uvdb_exc *) biomcmc_realloc (p->exc, p->exc_cap * sizeof (uvdb_exc));
    }
    if (uvaia_gpu_rows_exceptions (p->gpu, d_rows, pitch, p->sel, m, p->off, p->exc) ||
        uvaia_gpu_db_append_device (p->gpu, d_rows, pitch, p->sel, m, p->sel_nn)) return packer_fail_gpu (p);
    for (int k = 0; k < m; k++) {                        /* (names only of rows the engine holds: the flush of close stays consistent) */
      const char *nm = name[p->keep[a + k]];
      if (uvdb_add_reference_runs (p->w, nm, p->exc + p->off[k], (size_t) (p->off[k + 1] - p->off[k]))) { snprintf (p->err, sizeof p->err, "out of memory while indexing %s", nm); return -1; }
    }
    p->kept += m;
    if (packer_write_tiles (p, 0)) return -1;
  }
  return 0;
}

int
uvdb_packer_add_block (struct uvdb_packer *p, const void *d_rows, size_t pitch, int n, char *const *name)
{
  if (n < 0 || (size_t) n > p->block_cap) { snprintf (p->err, sizeof p->err, "%d rows in one call, the packer was opened for %zu", n, p->block_cap); return -1; }
  if (uvaia_gpu_rows_census (p->gpu, d_rows, pitch, n, p->non_n, p->n_exc)) return packer_fail_gpu (p);
  return uvdb_packer_add_rows (p, d_rows, pitch, p->ident, p->non_n, p->n_exc, name, n);
}

int
uvdb_packer_close (struct uvdb_packer *p)
{
  int bad = 0;
  if (p->w) {
    bad = p->gpu ? packer_write_tiles (p, 1) : 0;
    if (uvdb_close (p->w) && !bad) { snprintf (p->err, sizeof p->err, "problem writing the packed database"); bad = -1; }
    p->w = NULL;
  }
  p->tiles_device = p->exp.tiles_device; p->tiles_host = p->exp.tiles_host;
  if (p->gpu) { uvaia_gpu_rows_kernel_ms (p->gpu, p->rows_ms, 0); uvaia_gpu_encode_ms (p->gpu, p->encode_ms, 0); uvaia_gpu_close (p->gpu); }
  p->gpu = NULL;
  uvdb_export_free (&p->exp);
  free (p->non_n); free (p->n_exc); free (p->ident); free (p->keep); free (p->sel); free (p->sel_nn); free (p->off); free (p->exc);
  p->non_n = p->n_exc = p->ident = p->keep = p->sel = p->sel_nn = NULL; p->off = NULL; p->exc = NULL;
  return bad;
}
