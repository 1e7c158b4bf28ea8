/*
 * uvdb_extract.c -- see uvdb_extract.h.  Own code.
 */
#define _GNU_SOURCE
#include "uvdb_extract.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static double
wall_ms (void)
{
  struct timespec ts;
  clock_gettime (CLOCK_MONOTONIC, &ts);
  return (double) ts.tv_sec * 1e3 + (double) ts.tv_nsec * 1e-6;
}

int
uvdb_stage_pieces (uvaia_gpu_ctx *gpu, uvdb_set set, int slot, const uvdb_set_piece *pieces, int n_pieces)
{
  for (int p = 0; p < n_pieces; p++) {
    uvdb_reader db = set->db[pieces[p].file];
    const uint64_t t0 = pieces[p].first_tile;
    const int rc = db->h.version == 2     /* a compact file's tiles are expanded in the slot, a set may mix both kinds */
      ? uvaia_gpu_db_stage_compact_at (gpu, slot, (size_t) pieces[p].slot_tile, db->base, db->head_idx + t0 * 64, db->heads, db->lit_idx + t0 * 64, db->lits, db->non_n + t0 * 64, (int) pieces[p].n_tiles)
      : uvaia_gpu_db_stage_packed_at (gpu, slot, (size_t) pieces[p].slot_tile, uvdb_tile_planes (db, t0), db->non_n + t0 * 64, uvdb_tile_side_rows (db, t0), (int) pieces[p].n_tiles);
    if (rc) return UVDB_STAGE_EGPU;
  }
  return UVDB_STAGE_OK;
}

int
uvdb_stage_range (uvaia_gpu_ctx *gpu, uvdb_set set, const uint64_t *keep, uint64_t a, uint64_t b, int slot, uvdb_set_piece *pieces, int *sel, int *identity)
{
  int np = 0;
  uint64_t st = 0;
  if (uvdb_set_span (set, keep, a, b, pieces, UVDB_SET_MAX_FILES, &np, &st, sel)) return UVDB_STAGE_ESPAN;
  if (identity) *identity = !keep && np == 1 && a - set->first[pieces[0].file] == pieces[0].first_tile * 64;
  return uvdb_stage_pieces (gpu, set, slot, pieces, np);
}

int
uvdb_extract_plan (uvdb_set set, const uint64_t *pos, uint64_t a, uint64_t b, uvdb_set_piece *pieces, int max_pieces, int *n_pieces, uint64_t *slot_tiles, int *sel)
{
  if (!set || b <= a || b - a > (uint64_t) max_pieces) return -1;
  if (!pos && b > set->n_ref) return -1;
  int np = 0, f = -1;
  uint64_t slot = 0, prev = 0;
  uvdb_set_piece cur = {0, 0, 0, 0};                 /* the piece being grown: pieces may be NULL */
  for (uint64_t k = a; k < b; k++) {
    const uint64_t i = pos ? pos[k] : k;
    uint64_t l = 0;
    if (i >= set->n_ref || (k > a && i <= prev)) return -1;
    if (f < 0 || i >= set->first[f + 1]) { if (uvdb_set_locate (set, i, &f, &l)) return -1; } else l = i - set->first[f];
    const uint64_t tile = l / 64;
    const int same_file = np && cur.file == f;         /* then tile is the piece's last one or lies behind it: the positions ascend */
    if (same_file && tile == cur.first_tile + cur.n_tiles) { cur.n_tiles++; slot++; }
    else if (!same_file || tile > cur.first_tile + cur.n_tiles) {
      if (np >= max_pieces) return -1;
      cur.file = f; cur.first_tile = tile; cur.n_tiles = 1; cur.slot_tile = slot;
      np++; slot++;
    }
    if (pieces) pieces[np - 1] = cur;
    if (sel) sel[k - a] = (int) ((cur.slot_tile + (tile - cur.first_tile)) * 64 + l % 64);
    prev = i;
  }
  if (n_pieces) *n_pieces = np;
  if (slot_tiles) *slot_tiles = slot;
  return 0;
}

#define EXTRACT_FAIL(...) do { if (errbuf && errlen) snprintf (errbuf, errlen, __VA_ARGS__); rc = -1; goto done; } while (0)

int
uvdb_extract (uvdb_set set, uvaia_gpu_ctx *gpu, const uint64_t *pos, uint64_t n, uvdb_extract_fn fn, void *user, uvdb_extract_stats *stats, char *errbuf, size_t errlen)
{
  enum { CH = UVDB_EXTRACT_CHUNK };
  int rc = 0;
  if (errbuf && errlen) errbuf[0] = '\0';
  if (!set || !gpu || !fn) { if (errbuf && errlen) snprintf (errbuf, errlen, "extraction without a set, a context or a receiver"); return -1; }
  if (!n) return 0;
  const size_t nchar = set->nchar, pitch = (nchar + 15) / 16 * 16;
  uvdb_set_piece *pieces[2] = {NULL, NULL};
  int *sel[2] = {NULL, NULL}, np[2] = {0, 0};
  char *rows = NULL;
  if (set->side_row_ints != (uint32_t) uvaia_gpu_db_side_row_ints () || set->tile_bytes != uvaia_gpu_db_tile_bytes (gpu))
    EXTRACT_FAIL ("packed database %s does not match this engine's tile layout", set->filename[0]);
  /* the largest slot a chunk needs; every position is checked here, before anything is staged */
  uint64_t max_tiles = 0;
  for (uint64_t a = 0; a < n; a += CH) {
    uint64_t st = 0;
    if (uvdb_extract_plan (set, pos, a, a + CH < n ? a + CH : n, NULL, CH, NULL, &st, NULL))
      EXTRACT_FAIL ("the positions to extract must ascend without repeats and lie inside the %llu references of the stream (positions %llu on)", (unsigned long long) set->n_ref, (unsigned long long) a);
    if (st > max_tiles) max_tiles = st;
  }
  if (uvaia_gpu_db_stage_reserve (gpu, (size_t) max_tiles)) EXTRACT_FAIL ("%s", uvaia_gpu_last_error (gpu));
  for (int i = 0; i < 2; i++) {
    pieces[i] = (uvdb_set_piece *) malloc (CH * sizeof (uvdb_set_piece));
    sel[i] = (int *) malloc (CH * sizeof (int));
  }
  rows = (char *) malloc (CH * pitch + 1);
  if (!pieces[0] || !pieces[1] || !sel[0] || !sel[1] || !rows) EXTRACT_FAIL ("out of memory");
  const uint64_t n_chunks = (n + CH - 1) / CH;
  const double kernel0 = uvaia_gpu_stage_unpack_ms (gpu, 0);
  double t;
#define STAGE(c_) do { const uint64_t a_ = (c_) * CH, b_ = a_ + CH < n ? a_ + CH : n; const int s_ = (int) ((c_) & 1); uint64_t st_ = 0; \
    t = wall_ms (); \
    uvdb_extract_plan (set, pos, a_, b_, pieces[s_], CH, &np[s_], &st_, sel[s_]); \
    if (uvdb_stage_pieces (gpu, set, s_, pieces[s_], np[s_])) EXTRACT_FAIL ("%s", uvaia_gpu_last_error (gpu)); \
    if (stats) { stats->stage_ms += wall_ms () - t; stats->n_pieces += (uint64_t) np[s_]; stats->n_tiles += st_; } } while (0)
  STAGE ((uint64_t) 0);
  for (uint64_t c = 0; c < n_chunks; c++) {
    const uint64_t a = c * CH, b = a + CH < n ? a + CH : n;
    const int s = (int) (c & 1), m = (int) (b - a);
    if (c + 1 < n_chunks) STAGE (c + 1);               /* its copy runs next to this chunk's decode, exceptions and callbacks */
    t = wall_ms ();
    if (uvaia_gpu_db_stage_unpack_rows (gpu, s, sel[s], m, rows, pitch)) EXTRACT_FAIL ("%s", uvaia_gpu_last_error (gpu));
    if (stats) { stats->decode_ms += wall_ms () - t; stats->n_chunks++; }
    for (int j = 0; j < m; j++) {
      const uint64_t i = pos ? pos[a + (uint64_t) j] : a + (uint64_t) j;
      char *row = rows + (size_t) j * pitch;
      const char after = row[nchar];
      t = wall_ms ();
      uvdb_set_apply_exceptions (set, i, row);
      row[nchar] = '\0';
      const double t1 = wall_ms ();
      const int stop = fn (user, a + (uint64_t) j, i, uvdb_set_name (set, i), row);
      row[nchar] = after;
      if (stats) { stats->exceptions_ms += t1 - t; stats->write_ms += wall_ms () - t1; stats->n_rows++; }
      if (stop) EXTRACT_FAIL ("the receiver of the rows gave up at reference %llu", (unsigned long long) i);
    }
  }
#undef STAGE
  if (stats) stats->kernel_ms += uvaia_gpu_stage_unpack_ms (gpu, 0) - kernel0;
done:
  free (pieces[0]); free (pieces[1]); free (sel[0]); free (sel[1]); free (rows);
  return rc;
}

/* ---- names */

static int
cmp_names (const void *a, const void *b)
{ return strcmp (*(char *const *) a, *(char *const *) b); }

uvdb_name_list
uvdb_name_list_from_text (const char *text, size_t len)
{
  uvdb_name_list l = (uvdb_name_list) calloc (1, sizeof *l);
  if (!l) return NULL;
  l->text = (char *) malloc (len + 1);
  if (!l->text) { free (l); return NULL; }
  memcpy (l->text, text, len);
  l->text[len] = '\0';
  size_t lines = 1;
  for (size_t i = 0; i < len; i++) if (l->text[i] == '\n') lines++;
  l->name = (char **) malloc (lines * sizeof (char *));
  l->hits = (uint64_t *) calloc (lines, sizeof (uint64_t));
  if (!l->name || !l->hits) { uvdb_name_list_free (l); return NULL; }
  for (size_t i = 0; i < len;) {
    size_t e = i;
    while (e < len && l->text[e] != '\n') e++;
    size_t end = e;
    if (end > i && l->text[end - 1] == '\r') end--;
    l->text[end] = '\0';                               /* (end <= len: the byte behind the text is ours) */
    if (end > i) l->name[l->n++] = l->text + i;
    i = e + 1;
  }
  qsort (l->name, l->n, sizeof (char *), cmp_names);
  size_t u = 0;
  for (size_t i = 0; i < l->n; i++) if (!u || strcmp (l->name[u - 1], l->name[i])) l->name[u++] = l->name[i];
  l->n = u;
  return l;
}

uvdb_name_list
uvdb_name_list_read (const char *filename, char *errbuf, size_t errlen)
{
  FILE *f = fopen (filename, "rb");
  if (!f) { if (errbuf && errlen) snprintf (errbuf, errlen, "cannot read the list of names %s", filename); return NULL; }
  size_t cap = 1 << 16, len = 0, got;
  char *text = (char *) malloc (cap);
  while (text && (got = fread (text + len, 1, cap - len, f)) > 0) {
    len += got;
    if (len == cap) { char *t2 = (char *) realloc (text, cap *= 2); if (!t2) free (text); text = t2; }
  }
  fclose (f);
  uvdb_name_list l = text ? uvdb_name_list_from_text (text, len) : NULL;
  free (text);
  if (!l && errbuf && errlen) snprintf (errbuf, errlen, "out of memory while reading the list of names %s", filename);
  return l;
}

long
uvdb_name_list_find (uvdb_name_list l, const char *name)
{
  if (!l || !name) return -1;
  size_t lo = 0, hi = l->n;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    const int c = strcmp (l->name[mid], name);
    if (!c) { l->hits[mid]++; return (long) mid; }
    if (c < 0) lo = mid + 1; else hi = mid;
  }
  return -1;
}

void
uvdb_name_list_free (uvdb_name_list l)
{
  if (!l) return;
  free (l->name); free (l->hits); free (l->text);
  free (l);
}
