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

int
uvdb_packer_open (struct uvdb_packer *p, const char *path, int nchar, double ambig_r, int device, int block_cap)
{
  memset (p, 0, sizeof *p);
  p->nchar = nchar;
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
  const size_t tb = uvaia_gpu_db_tile_bytes (p->gpu), nt = UVDB_PACK_BATCH / 64 + 1;
  p->planes = biomcmc_malloc (nt * tb);
  p->tile_nonn = (int *) biomcmc_malloc (nt * 64 * sizeof (int));
  p->side = (int *) biomcmc_malloc (nt * 64 * (size_t) uvaia_gpu_db_side_row_ints () * sizeof (int));
  p->block_cap = (size_t) block_cap;
  p->non_n = (int *) biomcmc_malloc (p->block_cap * sizeof (int)); p->n_exc = (int *) biomcmc_malloc (p->block_cap * sizeof (int));
  p->ident = (int *) biomcmc_malloc (p->block_cap * sizeof (int)); p->keep = (int *) biomcmc_malloc (p->block_cap * sizeof (int));
  for (int i = 0; i < block_cap; i++) p->ident[i] = i;
  p->sel = (int *) biomcmc_malloc (UVDB_PACK_BATCH * sizeof (int)); p->sel_nn = (int *) biomcmc_malloc (UVDB_PACK_BATCH * sizeof (int));
  p->off = (uint64_t *) biomcmc_malloc ((UVDB_PACK_BATCH + 1) * sizeof (uint64_t));
  p->w = uvdb_create (path, nchar, tb, uvaia_gpu_db_side_row_ints (), ambig_r);
  if (!p->w) { snprintf (p->err, sizeof p->err, "cannot create %s", path); return -1; }
  return 0;
}

/* whole tiles (all = 0) or everything that is resident (all = 1: the flush) from the engine to the file */
static int
packer_write_tiles (struct uvdb_packer *p, int all)
{
  const size_t have = uvaia_gpu_db_size (p->gpu), nt = all ? (have + 63) / 64 : have / 64;
  if (!nt) return 0;
  if (uvaia_gpu_db_export (p->gpu, 0, nt, p->planes, p->tile_nonn, p->side) || uvaia_gpu_db_drop_tiles (p->gpu, nt)) return packer_fail_gpu (p);
  if (uvdb_add_tiles (p->w, nt, p->planes, p->tile_nonn, p->side)) { snprintf (p->err, sizeof p->err, "cannot write the packed database"); return -1; }
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
  if (p->gpu) { uvaia_gpu_rows_kernel_ms (p->gpu, p->rows_ms, 0); uvaia_gpu_close (p->gpu); }
  p->gpu = NULL;
  free (p->planes); free (p->tile_nonn); free (p->side); free (p->non_n); free (p->n_exc); free (p->ident); free (p->keep); free (p->sel); free (p->sel_nn); free (p->off); free (p->exc);
  p->planes = NULL; p->tile_nonn = p->side = p->non_n = p->n_exc = p->ident = p->keep = p->sel = p->sel_nn = NULL; p->off = NULL; p->exc = NULL;
  return bad;
}
