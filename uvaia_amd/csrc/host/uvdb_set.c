/*
 * uvdb_set.c -- see uvdb_set.h.  Own code.
 */
#include "uvdb_set.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define SLOT_MAX ((uint64_t) 0x7FFFFFFF - 63)        /* references a staging slot may hold: the engine counts them in an int */

uvdb_set
uvdb_set_open (const char *const *filenames, int n_files, int flags, char *errbuf, size_t errlen)
{
  if (errbuf && errlen) errbuf[0] = '\0';
  if (n_files < 1 || n_files > UVDB_SET_MAX_FILES || !filenames) {
    if (errbuf && errlen) snprintf (errbuf, errlen, "between 1 and %d packed databases can be read together (%d given)", UVDB_SET_MAX_FILES, n_files);
    return NULL;
  }
  uvdb_set s = (uvdb_set) calloc (1, sizeof *s);
  if (s) {
    s->db = (uvdb_reader *) calloc ((size_t) n_files, sizeof (uvdb_reader));
    s->filename = (char **) calloc ((size_t) n_files, sizeof (char *));
    s->first = (uint64_t *) calloc ((size_t) n_files + 1, sizeof (uint64_t));
  }
  if (!s || !s->db || !s->filename || !s->first) { if (errbuf && errlen) snprintf (errbuf, errlen, "out of memory"); uvdb_set_close (s); return NULL; }
  for (int f = 0; f < n_files; f++) {
    uvdb_reader r = uvdb_open (filenames[f], errbuf, errlen);
    if (!r) { uvdb_set_close (s); return NULL; }
    s->db[f] = r;
    s->n_files = f + 1;
    s->filename[f] = strdup (filenames[f]);
    if (!s->filename[f]) { if (errbuf && errlen) snprintf (errbuf, errlen, "out of memory"); uvdb_set_close (s); return NULL; }
    if (f == 0) { s->nchar = r->h.nchar; s->side_row_ints = r->h.side_row_ints; s->tile_bytes = r->h.tile_bytes; s->ref_ambiguity = r->h.ref_ambiguity; }
    const struct uvdb_header *h0 = &s->db[0]->h, *h = &r->h;
    if (h->nchar != h0->nchar) {
      if (errbuf && errlen) snprintf (errbuf, errlen, "packed database %s has %u sites but %s has %u sites; all sequences must be aligned", filenames[f], h->nchar, filenames[0], h0->nchar);
      uvdb_set_close (s); return NULL;
    }
    if (h->tile_bytes != h0->tile_bytes || h->side_row_ints != h0->side_row_ints) {
      if (errbuf && errlen) snprintf (errbuf, errlen, "packed databases %s and %s differ in their tile layout", filenames[f], filenames[0]);
      uvdb_set_close (s); return NULL;
    }
    if (h->ref_ambiguity != h0->ref_ambiguity && !(flags & UVDB_SET_ANY_AMBIGUITY)) {
      if (errbuf && errlen) snprintf (errbuf, errlen, "packed database %s was filtered with -A %g but %s with -A %g: `uvaiapack --merge -A` brings them to one value",
                                      filenames[f], h->ref_ambiguity, filenames[0], h0->ref_ambiguity);
      uvdb_set_close (s); return NULL;
    }
    if (h->ref_ambiguity > s->ref_ambiguity) s->ref_ambiguity = h->ref_ambiguity;
    s->first[f + 1] = s->first[f] + h->n_ref;
  }
  s->n_ref = s->first[n_files];
  return s;
}

void
uvdb_set_close (uvdb_set s)
{
  if (!s) return;
  for (int f = 0; f < s->n_files; f++) { if (s->db) uvdb_close_reader (s->db[f]); if (s->filename) free (s->filename[f]); }
  free (s->db); free (s->filename); free (s->first);
  free (s);
}

int
uvdb_set_locate (uvdb_set s, uint64_t i, int *file, uint64_t *local)
{
  if (!s || i >= s->n_ref) return -1;
  int lo = 0, hi = s->n_files;                       /* the last file with first[f] <= i: it is not empty, since i < n_ref */
  while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; if (s->first[mid] <= i) lo = mid; else hi = mid; }
  if (file) *file = lo;
  if (local) *local = i - s->first[lo];
  return 0;
}

const char *
uvdb_set_name (uvdb_set s, uint64_t i)
{
  int f; uint64_t l;
  return uvdb_set_locate (s, i, &f, &l) ? NULL : uvdb_name (s->db[f], l);
}

int32_t
uvdb_set_non_n (uvdb_set s, uint64_t i)
{
  int f; uint64_t l;
  return uvdb_set_locate (s, i, &f, &l) ? -1 : s->db[f]->non_n[l];
}

void
uvdb_set_apply_exceptions (uvdb_set s, uint64_t i, char *row)
{
  int f; uint64_t l;
  if (!uvdb_set_locate (s, i, &f, &l)) uvdb_apply_exceptions (s->db[f], l, row);
}

void
uvdb_set_unpack_reference (uvdb_set s, uint64_t i, char *out)
{
  int f; uint64_t l;
  if (!uvdb_set_locate (s, i, &f, &l)) uvdb_unpack_reference (s->db[f], l, out);
}

size_t
uvdb_set_runs (uvdb_set s, uint64_t i, const uvdb_exc **runs)
{
  int f; uint64_t l;
  if (uvdb_set_locate (s, i, &f, &l)) { if (runs) *runs = NULL; return 0; }
  const uvdb_reader r = s->db[f];
  if (runs) *runs = r->exc + r->exc_idx[l];
  return (size_t) (r->exc_idx[l + 1] - r->exc_idx[l]);
}

int
uvdb_set_span (uvdb_set s, const uint64_t *keep, uint64_t a, uint64_t b, uvdb_set_piece *pieces, int max_pieces, int *n_pieces, uint64_t *slot_tiles, int *sel_out)
{
  if (!s || b <= a) return -1;
  if (!keep && b > s->n_ref) return -1;
  int np = 0, f = -1;
  uint64_t slot = 0, k = a, prev = 0;
  while (k < b) {
    const uint64_t i = keep ? keep[k] : k;
    if (i >= s->n_ref || (k > a && i <= prev)) return -1;
    if (uvdb_set_locate (s, i, &f, NULL)) return -1;
    /* the kept references of the range that lie in file f: positions [k, e) */
    const uint64_t end = s->first[f + 1];
    uint64_t e = k + 1;
    if (!keep) e = end < b ? end : b;
    else while (e < b && keep[e] < end) { if (keep[e] <= keep[e - 1]) return -1; e++; }
    const uint64_t lo = i - s->first[f], hi = (keep ? keep[e - 1] : e - 1) - s->first[f];
    const uint64_t t0 = lo / 64, nt = hi / 64 - t0 + 1;
    if (nt > SLOT_MAX / 64 || slot + nt > SLOT_MAX / 64) return -1;
    if (pieces) {
      if (np >= max_pieces) return -1;
      pieces[np].file = f; pieces[np].first_tile = t0; pieces[np].n_tiles = nt; pieces[np].slot_tile = slot;
    }
    if (sel_out) for (uint64_t x = k; x < e; x++) sel_out[x - a] = (int) (slot * 64 + ((keep ? keep[x] : x) - s->first[f] - t0 * 64));
    np++;
    slot += nt;
    prev = keep ? keep[e - 1] : e - 1;
    k = e;
  }
  if (n_pieces) *n_pieces = np;
  if (slot_tiles) *slot_tiles = slot;
  return 0;
}

int
uvdb_set_direct_tiles (uvdb_set s, const uint64_t *keep, uint64_t a, uint64_t b, uint64_t n, uint64_t store, int *file, uint64_t *first_tile)
{
  int f = 0;
  uint64_t l = 0;
  if (!s || keep || b <= a || b > n || n != s->n_ref || store % 64) return -1;
  if (uvdb_set_locate (s, a, &f, &l) || l % 64 || b > s->first[f + 1]) return -1;
  if (s->db[f]->h.version != 1) return -1;           /* a compact file holds no dense tiles: its chunks are staged and expanded */
  if ((b - a) % 64 && b != n) return -1;
  if (file) *file = f;
  if (first_tile) *first_tile = l / 64;
  return 0;
}
