/* uvdb.c -- see uvdb.h.  Own code. */
#define _GNU_SOURCE
#include "uvdb.h"

#include <fcntl.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

struct uvdb_writer_struct {
  FILE *f;
  struct uvdb_header h;
  uint64_t tiles_written;
  /* sections kept in memory until close (small next to the planes): valid-site counts, side rows, names, exception runs */
  int32_t *non_n; size_t nonn_cap;
  FILE *side_tmp;                      /* side rows go through a temporary file: 256 B per reference */
  uint64_t *name_idx; size_t idx_cap; char *names; size_t names_len, names_cap;
  uint64_t *exc_idx; uvdb_exc *exc; size_t exc_len, exc_cap;
  uvdb_exc *runs_tmp; size_t runs_cap;   /* the runs of one reference on their way from its text to the section (uvdb_add_reference) */
  /* version 2 (uvdb_create_compact): the tiles wait in `pend` until the base is fixed; heads and literals go through temporary files */
  int compact, base_fixed;
  unsigned char *pend; size_t pend_tiles, pend_cap;
  uint32_t *base;                      /* [W4][plane][4] */
  FILE *heads_tmp, *lits_tmp;
  uint64_t *head_idx, *lit_idx; size_t lanes, lane_cap;     /* lanes encoded so far; both arrays hold lanes + 1 offsets */
  uint32_t *hbuf, *lbuf;               /* heads and literals of one reference on their way to the files */
};

static uint64_t align64 (uint64_t x) { return (x + 63u) & ~(uint64_t) 63u; }

static int
pad_to (FILE *f, uint64_t off)
{
  static const char zero[64] = {0};
  long at = ftell (f);
  if (at < 0 || (uint64_t) at > off) return -1;
  while ((uint64_t) at < off) {
    size_t n = (size_t) ((off - (uint64_t) at) < sizeof zero ? (off - (uint64_t) at) : sizeof zero);
    if (fwrite (zero, 1, n, f) != n) return -1;
    at += (long) n;
  }
  return 0;
}

static void
free_writer (uvdb_writer w)
{
  if (w->side_tmp) fclose (w->side_tmp);
  if (w->heads_tmp) fclose (w->heads_tmp);
  if (w->lits_tmp) fclose (w->lits_tmp);
  free (w->non_n); free (w->name_idx); free (w->names); free (w->exc_idx); free (w->exc); free (w->runs_tmp);
  free (w->pend); free (w->base); free (w->head_idx); free (w->lit_idx); free (w->hbuf); free (w->lbuf);
  free (w);
}

uvdb_writer
uvdb_create_compact (const char *filename, int nchar, size_t tile_bytes, int side_row_ints, double ref_ambiguity)
{
  if (nchar < 1 || nchar > UVDB_COMPACT_MAX_NCHAR) return NULL;
  uvdb_writer w = (uvdb_writer) calloc (1, sizeof *w);
  if (!w) return NULL;
  const size_t W4 = (size_t) (((nchar + 31) / 32 + 3) / 4);
  w->compact = 1;
  w->f = fopen (filename, "wb");
  w->heads_tmp = tmpfile (); w->lits_tmp = tmpfile ();
  w->base = (uint32_t *) calloc (W4 * 16, sizeof (uint32_t));
  w->hbuf = (uint32_t *) malloc (W4 * 4 * sizeof (uint32_t)); w->lbuf = (uint32_t *) malloc (W4 * 16 * sizeof (uint32_t));
  w->head_idx = (uint64_t *) calloc (1, sizeof (uint64_t)); w->lit_idx = (uint64_t *) calloc (1, sizeof (uint64_t)); w->lane_cap = 1;
  if (!w->f || !w->heads_tmp || !w->lits_tmp || !w->base || !w->hbuf || !w->lbuf || !w->head_idx || !w->lit_idx || tile_bytes != W4 * 4 * 64 * 16) {
    if (w->f) fclose (w->f);
    free_writer (w); return NULL;
  }
  memcpy (w->h.magic, UVDB_MAGIC, 8);
  w->h.version = 2; w->h.nchar = (uint32_t) nchar; w->h.W4 = (uint32_t) W4;
  w->h.side_row_ints = (uint32_t) side_row_ints; w->h.tile_bytes = tile_bytes; w->h.ref_ambiguity = ref_ambiguity;
  w->h.off_planes = align64 (sizeof (struct uvdb_header));
  if (fwrite (&w->h, sizeof w->h, 1, w->f) != 1 || pad_to (w->f, w->h.off_planes)) { fclose (w->f); free_writer (w); return NULL; }
  return w;
}

/* the base of a version 2 file: the majority of the first m lanes of the pending tiles, bit by bit */
static void
compact_fix_base (uvdb_writer w, uint64_t m)
{
  const uint32_t W4 = w->h.W4, nchar = w->h.nchar;
  const uint32_t *t32 = (const uint32_t *) w->pend;
  const size_t tile_dwords = (size_t) W4 * 4 * 64 * 4;
#pragma omp parallel for schedule(static)
  for (uint32_t x = 0; x < W4 * 16; x++) {           /* x = (word group * 4 + plane) * 4 + j, the base's own order */
    const uint32_t row = x >> 2, j = x & 3, word = (row >> 2) * 4 + j;
    uint32_t cnt[32] = {0}, v = 0;
    for (uint64_t k = 0; k < m; k++) {
      const uint32_t d = t32[(k >> 6) * tile_dwords + ((size_t) row * 64 + (k & 63)) * 4 + j];
      for (int b = 0; b < 32; b++) cnt[b] += (d >> b) & 1u;
    }
    for (int b = 0; b < 32; b++) if ((uint64_t) cnt[b] * 2 > m && (uint64_t) word * 32 + (uint32_t) b < nchar) v |= 1u << b;
    w->base[x] = v;
  }
  w->base_fixed = 1;
}

/* room for n_lanes more offsets in both index arrays of a version 2 writer */
static int
compact_index_room (uvdb_writer w, size_t n_lanes)
{
  if (w->lanes + n_lanes + 1 <= w->lane_cap) return 0;
  size_t ncap = w->lane_cap * 2 > 4096 ? w->lane_cap * 2 : 4096;
  while (ncap < w->lanes + n_lanes + 1) ncap *= 2;
  w->head_idx = (uint64_t *) realloc (w->head_idx, ncap * sizeof (uint64_t));
  w->lit_idx = (uint64_t *) realloc (w->lit_idx, ncap * sizeof (uint64_t));
  if (!w->head_idx || !w->lit_idx) return -1;
  w->lane_cap = ncap;
  return 0;
}

/* heads and literals of every lane of n_tiles dense tiles, in the canonical encoding (uvdb.h) */
static int
compact_encode_tiles (uvdb_writer w, size_t n_tiles, const void *planes)
{
  const uint32_t W4 = w->h.W4, n_real = (w->h.nchar + 31) / 32;       /* the padding words behind them never differ from the base */
  const size_t tile_dwords = (size_t) W4 * 4 * 64 * 4;
  if (compact_index_room (w, n_tiles * 64)) return -1;
  for (size_t t = 0; t < n_tiles; t++) for (uint32_t lane = 0; lane < 64; lane++) {
    const uint32_t *t32 = (const uint32_t *) planes + t * tile_dwords + (size_t) lane * 4;
    uint32_t nh = 0, nl = 0, kind = 0, code = 0, first = 0, run = 0;      /* the open head: kind 1 = fill, 2 = literal */
    for (uint32_t word = 0; word < n_real; word++) {
      const uint32_t *x = t32 + (size_t) (word >> 2) * 1024 + (word & 3), *b = w->base + (size_t) (word >> 2) * 16 + (word & 3);
      uint32_t k = 0, c = 0;
      if (x[0] != b[0] || x[256] != b[4] || x[512] != b[8] || x[768] != b[12]) {
        k = 1;
        for (int p = 0; p < 4; p++) { if (x[p * 256] == 0xFFFFFFFFu) c |= 1u << p; else if (x[p * 256]) k = 2; }
        if (k == 2) c = 0;
      }
      if (!k || k != kind || c != code || run == UVDB_HEAD_MAX_WORDS) {
        if (kind) w->hbuf[nh++] = UVDB_HEAD (first, run, kind == 2, code);
        kind = k; code = c; first = word; run = 0;
      }
      if (k) run++;
      if (k == 2) { for (int p = 0; p < 4; p++) w->lbuf[nl * 4 + p] = x[p * 256]; nl++; }
    }
    if (kind) w->hbuf[nh++] = UVDB_HEAD (first, run, kind == 2, code);
    if ((nh && fwrite (w->hbuf, sizeof (uint32_t), nh, w->heads_tmp) != nh) || (nl && fwrite (w->lbuf, 16, nl, w->lits_tmp) != nl)) return -1;
    w->head_idx[w->lanes + 1] = w->head_idx[w->lanes] + nh;
    w->lit_idx[w->lanes + 1] = w->lit_idx[w->lanes] + nl;
    w->lanes++;
  }
  return 0;
}

static int
compact_flush_pending (uvdb_writer w)
{
  const uint64_t lanes = (uint64_t) w->pend_tiles * 64;
  uint64_t m = w->h.n_ref < lanes ? w->h.n_ref : lanes;
  if (m > UVDB_BASE_SAMPLE) m = UVDB_BASE_SAMPLE;
  compact_fix_base (w, m);
  const int rc = compact_encode_tiles (w, w->pend_tiles, w->pend);
  free (w->pend); w->pend = NULL; w->pend_tiles = w->pend_cap = 0;
  return rc;
}

static int
compact_add_tiles (uvdb_writer w, size_t n_tiles, const void *planes)
{
  if (w->base_fixed) return compact_encode_tiles (w, n_tiles, planes);
  if (w->pend_tiles + n_tiles > w->pend_cap) {
    size_t ncap = w->pend_cap ? w->pend_cap * 2 : UVDB_BASE_SAMPLE / 64;
    while (ncap < w->pend_tiles + n_tiles) ncap *= 2;
    w->pend = (unsigned char *) realloc (w->pend, ncap * (size_t) w->h.tile_bytes);
    if (!w->pend) return -1;
    w->pend_cap = ncap;
  }
  if (n_tiles) memcpy (w->pend + w->pend_tiles * (size_t) w->h.tile_bytes, planes, n_tiles * (size_t) w->h.tile_bytes);
  w->pend_tiles += n_tiles;
  /* the sample is complete once that many references have been named and their tiles are here */
  if (w->pend_tiles * 64 >= UVDB_BASE_SAMPLE && w->h.n_ref >= UVDB_BASE_SAMPLE) return compact_flush_pending (w);
  return 0;
}

const uint32_t *
uvdb_compact_base (uvdb_writer w)
{
  return w && w->compact && w->base_fixed ? w->base : NULL;
}

int
uvdb_add_tiles_encoded (uvdb_writer w, size_t n_tiles, const int *non_n, const uint64_t *head_idx, const uint32_t *heads, const uint64_t *lit_idx, const uint32_t *lits)
{
  if (!w || !w->compact || !w->base_fixed) return -1;
  if (!n_tiles) return 0;
  if (!non_n || !head_idx || !lit_idx) return -1;
  const size_t lanes = n_tiles * 64;
  const uint32_t n_words = w->h.W4 * 4;
  const uint64_t h0 = head_idx[0], l0 = lit_idx[0];
  if (head_idx[lanes] < h0 || lit_idx[lanes] < l0 || (head_idx[lanes] > h0 && !heads) || (lit_idx[lanes] > l0 && !lits)) return -1;
  /* what compact_check_heads asks of a file, before anything is appended */
  int bad = 0;
#pragma omp parallel for schedule(static) reduction(|:bad)
  for (size_t g = 0; g < lanes; g++) {
    const uint64_t hb = head_idx[g], he = head_idx[g + 1], lb = lit_idx[g], le = lit_idx[g + 1];
    if (hb > he || hb < h0 || he > head_idx[lanes] || lb > le || lb < l0 || le > lit_idx[lanes]) { bad |= 1; continue; }
    uint64_t lit = 0;
    uint32_t end = 0;
    for (uint64_t k = hb; k < he; k++) {
      const uint32_t head = heads[k], first = UVDB_HEAD_FIRST (head), nw = UVDB_HEAD_WORDS (head);
      if (!nw || first < end || first + nw > n_words) { bad |= 2; break; }
      end = first + nw;
      if (UVDB_HEAD_LITERAL (head)) lit += nw;
    }
    if (lit != le - lb) bad |= 2;
  }
  if (bad) return -1;
  if ((w->tiles_written + n_tiles) * 64 > w->nonn_cap) {
    size_t ncap = w->nonn_cap ? w->nonn_cap * 2 : (1u << 16);
    while (ncap < (w->tiles_written + n_tiles) * 64) ncap *= 2;
    int32_t *nn = (int32_t *) realloc (w->non_n, ncap * sizeof (int32_t));
    if (!nn) return -1;
    w->non_n = nn; w->nonn_cap = ncap;
  }
  if (compact_index_room (w, lanes)) return -1;
  const uint64_t nh = head_idx[lanes] - h0, nl = lit_idx[lanes] - l0;
  if ((nh && fwrite (heads + h0, sizeof (uint32_t), (size_t) nh, w->heads_tmp) != nh) || (nl && fwrite (lits + l0 * 4, 16, (size_t) nl, w->lits_tmp) != nl)) return -1;
  memcpy (w->non_n + w->tiles_written * 64, non_n, lanes * sizeof (int32_t));
  const uint64_t hbase = w->head_idx[w->lanes], lbase = w->lit_idx[w->lanes];      /* the file's running totals */
  for (size_t g = 1; g <= lanes; g++) {
    w->head_idx[w->lanes + g] = hbase + (head_idx[g] - h0);
    w->lit_idx[w->lanes + g] = lbase + (lit_idx[g] - l0);
  }
  w->lanes += lanes;
  w->tiles_written += n_tiles;
  return 0;
}

static int
copy_stream (FILE *src, FILE *dst)
{
  char buf[1 << 16];
  size_t n;
  int bad = 0;
  rewind (src);
  while ((n = fread (buf, 1, sizeof buf, src)) > 0) bad |= fwrite (buf, 1, n, dst) != n;
  return bad | (ferror (src) != 0);
}

uvdb_writer
uvdb_create (const char *filename, int nchar, size_t tile_bytes, int side_row_ints, double ref_ambiguity)
{
  uvdb_writer w = (uvdb_writer) calloc (1, sizeof *w);
  if (!w) return NULL;
  w->f = fopen (filename, "wb");
  w->side_tmp = tmpfile ();
  if (!w->f || !w->side_tmp) { if (w->f) fclose (w->f); if (w->side_tmp) fclose (w->side_tmp); free (w); return NULL; }
  memcpy (w->h.magic, UVDB_MAGIC, 8);
  w->h.version = 1; w->h.nchar = (uint32_t) nchar; w->h.W4 = (uint32_t) (((nchar + 31) / 32 + 3) / 4);
  w->h.side_row_ints = (uint32_t) side_row_ints; w->h.tile_bytes = tile_bytes; w->h.ref_ambiguity = ref_ambiguity;
  w->h.off_planes = align64 (sizeof (struct uvdb_header));
  if (fwrite (&w->h, sizeof w->h, 1, w->f) != 1 || pad_to (w->f, w->h.off_planes)) { fclose (w->f); fclose (w->side_tmp); free (w); return NULL; }
  return w;
}

int
uvdb_add_reference_runs (uvdb_writer w, const char *name, const uvdb_exc *runs, size_t n_runs)
{
  const uint64_t i = w->h.n_ref;
  if (i + 2 > w->idx_cap) {
    size_t ncap = w->idx_cap ? w->idx_cap * 2 : 4096;
    w->name_idx = (uint64_t *) realloc (w->name_idx, ncap * sizeof (uint64_t));
    w->exc_idx = (uint64_t *) realloc (w->exc_idx, ncap * sizeof (uint64_t));
    if (!w->name_idx || !w->exc_idx) return -1;
    w->idx_cap = ncap;
  }
  const size_t nl = strlen (name) + 1;
  if (w->names_len + nl > w->names_cap) {
    size_t ncap = w->names_cap ? w->names_cap * 2 : (1u << 20);
    while (ncap < w->names_len + nl) ncap *= 2;
    w->names = (char *) realloc (w->names, ncap);
    if (!w->names) return -1;
    w->names_cap = ncap;
  }
  if (w->exc_len + n_runs > w->exc_cap) {
    size_t ncap = w->exc_cap ? w->exc_cap * 2 : (1u << 16);
    while (ncap < w->exc_len + n_runs) ncap *= 2;
    w->exc = (uvdb_exc *) realloc (w->exc, ncap * sizeof (uvdb_exc));
    if (!w->exc) return -1;
    w->exc_cap = ncap;
  }
  w->name_idx[i] = w->names_len;
  memcpy (w->names + w->names_len, name, nl);
  w->names_len += nl;
  w->exc_idx[i] = w->exc_len;
  if (n_runs) memcpy (w->exc + w->exc_len, runs, n_runs * sizeof (uvdb_exc));
  w->exc_len += n_runs;
  w->h.n_ref++;
  w->name_idx[w->h.n_ref] = w->names_len;
  w->exc_idx[w->h.n_ref] = w->exc_len;
  return 0;
}

int
uvdb_add_reference (uvdb_writer w, const char *name, const char *seq)
{ /* the runs of the text, then the above */
  uvdb_exc *runs = w->runs_tmp;
  size_t n_runs = 0;
  for (uint32_t s = 0; s < w->h.nchar; ) {           /* runs of invalid characters other than N */
    const char ch = seq[s];
    if (ch == '-' || ch == '?' || ch == 'X' || ch == 'O' || ch == '.') {
      uint32_t e = s + 1;
      while (e < w->h.nchar && seq[e] == ch && e - s < 0xFFFFFFu) e++;
      if (n_runs + 1 > w->runs_cap) {
        size_t ncap = w->runs_cap ? w->runs_cap * 2 : 1024;
        runs = (uvdb_exc *) realloc (w->runs_tmp, ncap * sizeof (uvdb_exc));
        if (!runs) return -1;
        w->runs_tmp = runs; w->runs_cap = ncap;
      }
      runs[n_runs].pos = s; runs[n_runs].len_char = ((e - s) << 8) | (uint32_t) (unsigned char) ch;
      n_runs++;
      s = e;
    } else s++;
  }
  return uvdb_add_reference_runs (w, name, runs, n_runs);
}

int
uvdb_add_tiles (uvdb_writer w, size_t n_tiles, const void *planes, const int *non_n, const int *side_rows)
{
  if (!w->compact && fwrite (planes, w->h.tile_bytes, n_tiles, w->f) != n_tiles) return -1;
  const size_t n = n_tiles * 64;
  if ((w->tiles_written + n_tiles) * 64 > w->nonn_cap) {
    size_t ncap = w->nonn_cap ? w->nonn_cap * 2 : (1u << 16);
    while (ncap < (w->tiles_written + n_tiles) * 64) ncap *= 2;
    w->non_n = (int32_t *) realloc (w->non_n, ncap * sizeof (int32_t));
    if (!w->non_n) return -1;
    w->nonn_cap = ncap;
  }
  if (n) memcpy (w->non_n + w->tiles_written * 64, non_n, n * sizeof (int32_t));      /* (no tiles: the array may not exist yet) */
  if (w->compact) { if (compact_add_tiles (w, n_tiles, planes)) return -1; }     /* (the side rows are a function of the planes: not stored) */
  else if (fwrite (side_rows, (size_t) w->h.side_row_ints * sizeof (int32_t), n, w->side_tmp) != n) return -1;
  w->tiles_written += n_tiles;
  return 0;
}

int
uvdb_close (uvdb_writer w)
{
  int bad = 0;
  struct uvdb_header *h = &w->h;
  h->n_tiles = w->tiles_written;
  if (h->n_tiles != (h->n_ref + 63) / 64) bad = 1;           /* every reference named must have been packed */
  uint64_t at;
  if (w->compact) {           /* base, non_n, head_idx, heads, lit_idx, lits */
    if (!w->base_fixed) bad |= compact_flush_pending (w);
    const size_t lanes = (size_t) h->n_tiles * 64;
    if (w->lanes != lanes) bad = 1;
    bad |= fwrite (w->base, 64, h->W4, w->f) != h->W4;
    at = h->off_planes + (uint64_t) h->W4 * 64;
    h->off_nonn = align64 (at);
    bad |= pad_to (w->f, h->off_nonn);
    bad |= lanes && fwrite (w->non_n, sizeof (int32_t), lanes, w->f) != lanes;
    at = h->off_nonn + lanes * sizeof (int32_t);
    h->off_side = align64 (at);
    bad |= pad_to (w->f, h->off_side);
    bad |= fwrite (w->head_idx, sizeof (uint64_t), w->lanes + 1, w->f) != w->lanes + 1;
    at = h->off_side + (w->lanes + 1) * sizeof (uint64_t);
    h->reserved[0] = align64 (at);
    bad |= pad_to (w->f, h->reserved[0]);
    bad |= copy_stream (w->heads_tmp, w->f);
    at = h->reserved[0] + w->head_idx[w->lanes] * sizeof (uint32_t);
    h->reserved[1] = align64 (at);
    bad |= pad_to (w->f, h->reserved[1]);
    bad |= fwrite (w->lit_idx, sizeof (uint64_t), w->lanes + 1, w->f) != w->lanes + 1;
    at = align64 (h->reserved[1] + (w->lanes + 1) * sizeof (uint64_t));
    bad |= pad_to (w->f, at);
    bad |= copy_stream (w->lits_tmp, w->f);
    at += w->lit_idx[w->lanes] * 16;
  } else {
  at = h->off_planes + h->n_tiles * h->tile_bytes;
  h->off_nonn = align64 (at);
  bad |= pad_to (w->f, h->off_nonn);
  bad |= h->n_tiles && fwrite (w->non_n, sizeof (int32_t), (size_t) h->n_tiles * 64, w->f) != (size_t) h->n_tiles * 64;
  at = h->off_nonn + h->n_tiles * 64 * sizeof (int32_t);
  h->off_side = align64 (at);
  bad |= pad_to (w->f, h->off_side);
  rewind (w->side_tmp);
  {
    char buf[1 << 16];
    size_t n;
    while ((n = fread (buf, 1, sizeof buf, w->side_tmp)) > 0) bad |= fwrite (buf, 1, n, w->f) != n;
  }
  at = h->off_side + h->n_tiles * 64 * (uint64_t) h->side_row_ints * sizeof (int32_t);
  }
  uint64_t zero_idx[1] = {0};
  const uint64_t *nidx = h->n_ref ? w->name_idx : zero_idx, *eidx = h->n_ref ? w->exc_idx : zero_idx;
  h->off_name_idx = align64 (at);
  bad |= pad_to (w->f, h->off_name_idx);
  bad |= fwrite (nidx, sizeof (uint64_t), (size_t) h->n_ref + 1, w->f) != (size_t) h->n_ref + 1;
  at = h->off_name_idx + (h->n_ref + 1) * sizeof (uint64_t);
  h->off_names = align64 (at);
  bad |= pad_to (w->f, h->off_names);
  bad |= w->names_len && fwrite (w->names, 1, w->names_len, w->f) != w->names_len;
  at = h->off_names + w->names_len;
  h->off_exc_idx = align64 (at);
  bad |= pad_to (w->f, h->off_exc_idx);
  bad |= fwrite (eidx, sizeof (uint64_t), (size_t) h->n_ref + 1, w->f) != (size_t) h->n_ref + 1;
  at = h->off_exc_idx + (h->n_ref + 1) * sizeof (uint64_t);
  h->off_exc = align64 (at);
  bad |= pad_to (w->f, h->off_exc);
  bad |= w->exc_len && fwrite (w->exc, sizeof (uvdb_exc), w->exc_len, w->f) != w->exc_len;
  h->file_bytes = h->off_exc + w->exc_len * sizeof (uvdb_exc);
  bad |= fseek (w->f, 0, SEEK_SET) != 0 || fwrite (h, sizeof *h, 1, w->f) != 1;
  bad |= fclose (w->f) != 0;
  free_writer (w);
  return bad ? -1 : 0;
}

/* ------------------------------------------------------------------------------------------------ reader */
static void
set_err (char *errbuf, size_t errlen, const char *fmt, ...)
{
  if (!errbuf || !errlen) return;
  va_list ap;
  va_start (ap, fmt);
  vsnprintf (errbuf, errlen, fmt, ap);
  va_end (ap);
}

/* the sections of a version 2 file, in file order, each inside the file and in front of the next one; fills the reader's pointers and
 * *heads_cap / *lits_cap (records the two payload sections have room for).  0 = consistent */
static int
compact_layout (uvdb_reader r, uint64_t *heads_cap, uint64_t *lits_cap)
{
  const struct uvdb_header *h = &r->h;
  const uint64_t n = h->n_ref, flen = (uint64_t) r->map_len, off_heads = h->reserved[0], off_lidx = h->reserved[1];
  uint64_t sz_nonn = 0, sz_lidx = 0, sz_idx = 0, lanes = 0;
  int bad = h->file_bytes != flen || n > (UINT64_MAX >> 8) || h->n_tiles != (n + 63) / 64 || h->nchar == 0 || h->nchar > UVDB_COMPACT_MAX_NCHAR ||
            h->W4 != ((h->nchar + 31) / 32 + 3) / 4 || h->tile_bytes != (uint64_t) h->W4 * 4 * 64 * 16 || h->side_row_ints != UVDB_SIDE_ROW_INTS;
  bad = bad || __builtin_mul_overflow (h->n_tiles, (uint64_t) 64, &lanes) || __builtin_mul_overflow (h->n_tiles, (uint64_t) 64 * 4, &sz_nonn) ||
        __builtin_mul_overflow (lanes + 1, (uint64_t) 8, &sz_lidx) || __builtin_mul_overflow (n + 1, (uint64_t) 8, &sz_idx);
  if (bad) return -1;
  const uint64_t sz_base = (uint64_t) h->W4 * 64;
  bad = h->off_planes < sizeof (struct uvdb_header) || h->off_planes > flen || sz_base > flen - h->off_planes || h->off_planes + sz_base > h->off_nonn ||
        h->off_nonn > flen || sz_nonn > flen - h->off_nonn || h->off_nonn + sz_nonn > h->off_side ||
        h->off_side > flen || sz_lidx > flen - h->off_side || h->off_side + sz_lidx > off_heads ||
        off_heads > off_lidx || off_lidx > flen || sz_lidx > flen - off_lidx || off_lidx + sz_lidx > h->off_name_idx ||
        h->off_name_idx > flen || sz_idx > flen - h->off_name_idx || h->off_name_idx + sz_idx > h->off_names ||
        h->off_names > h->off_exc_idx || h->off_exc_idx > flen || sz_idx > flen - h->off_exc_idx || h->off_exc_idx + sz_idx > h->off_exc || h->off_exc > flen ||
        (h->off_planes | h->off_nonn | h->off_side | off_heads | off_lidx | h->off_name_idx | h->off_exc_idx | h->off_exc) % 8 != 0;
  if (bad) return -1;
  const uint64_t off_lits = align64 (off_lidx + sz_lidx);
  if (off_lits > h->off_name_idx) return -1;
  r->base = (const uint32_t *) (r->map + h->off_planes);
  r->head_idx = (const uint64_t *) (r->map + h->off_side);
  r->heads = (const uint32_t *) (r->map + off_heads);
  r->lit_idx = (const uint64_t *) (r->map + off_lidx);
  r->lits = (const uint32_t *) (r->map + off_lits);
  *heads_cap = (off_lidx - off_heads) / sizeof (uint32_t);
  *lits_cap = (h->off_name_idx - off_lits) / 16;
  return 0;
}

/* every index entry and every head of a version 2 file (a pass over the whole file, threaded): 0 = good, bit 0 = an index decreases or
 * leaves its section, bit 1 = a head is empty, leaves the alignment, overlaps or precedes the one before it, or the literal heads of a
 * lane do not add up to its extent of lits */
static int
compact_check_heads (uvdb_reader r, uint64_t heads_cap, uint64_t lits_cap)
{
  const uint64_t lanes = r->h.n_tiles * 64, nh = r->head_idx[lanes], nl = r->lit_idx[lanes];
  const uint32_t n_words = r->h.W4 * 4;
  if (r->head_idx[0] != 0 || r->lit_idx[0] != 0 || nh > heads_cap || nl > lits_cap) return 1;
  int bad = 0;
#pragma omp parallel for schedule(static) reduction(|:bad)
  for (uint64_t g = 0; g < lanes; g++) {
    const uint64_t hb = r->head_idx[g], he = r->head_idx[g + 1], lb = r->lit_idx[g], le = r->lit_idx[g + 1];
    if (hb > he || he > nh || lb > le || le > nl) { bad |= 1; continue; }
    uint64_t lit = 0;
    uint32_t end = 0;
    for (uint64_t k = hb; k < he; k++) {
      const uint32_t head = r->heads[k], first = UVDB_HEAD_FIRST (head), nw = UVDB_HEAD_WORDS (head);
      if (!nw || first < end || first + nw > n_words) { bad |= 2; break; }
      end = first + nw;
      if (UVDB_HEAD_LITERAL (head)) lit += nw;
    }
    if (lit != le - lb) bad |= 2;
  }
  return bad;
}

/* the records of lane g written over words that hold the base: word w, plane p lives at dst[(w / 4) * group_stride + p * plane_stride + w % 4] */
static void
compact_apply_lane (uvdb_reader r, uint64_t g, uint32_t *dst, size_t group_stride, size_t plane_stride)
{
  const uint32_t *lit = r->lits + r->lit_idx[g] * 4;
  for (uint64_t k = r->head_idx[g]; k < r->head_idx[g + 1]; k++) {
    const uint32_t head = r->heads[k], first = UVDB_HEAD_FIRST (head), nw = UVDB_HEAD_WORDS (head), code = UVDB_HEAD_CODE (head);
    for (uint32_t q = 0; q < nw; q++) {
      uint32_t *o = dst + (size_t) ((first + q) >> 2) * group_stride + ((first + q) & 3);
      for (int p = 0; p < 4; p++) o[p * plane_stride] = UVDB_HEAD_LITERAL (head) ? lit[q * 4 + p] : (((code >> p) & 1u) ? 0xFFFFFFFFu : 0u);
    }
    if (UVDB_HEAD_LITERAL (head)) lit += (size_t) nw * 4;
  }
}

uint32_t
uvdb_file_version (const char *filename)
{
  struct uvdb_header h;
  FILE *f = fopen (filename, "rb");
  if (!f) return 0;
  const int ok = fread (&h, sizeof h, 1, f) == 1 && memcmp (h.magic, UVDB_MAGIC, 8) == 0;
  fclose (f);
  return ok ? h.version : 0;
}

uvdb_reader
uvdb_open (const char *filename, char *errbuf, size_t errlen)
{
  uvdb_reader r = (uvdb_reader) calloc (1, sizeof *r);
  if (!r) return NULL;
  int fd = open (filename, O_RDONLY);
  struct stat st;
  if (fd < 0 || fstat (fd, &st) != 0) { set_err (errbuf, errlen, "cannot open %s", filename); if (fd >= 0) close (fd); free (r); return NULL; }
  if ((size_t) st.st_size < sizeof (struct uvdb_header)) { set_err (errbuf, errlen, "%s is not a packed uvaia database", filename); close (fd); free (r); return NULL; }
  r->map_len = (size_t) st.st_size;
  r->map = (const unsigned char *) mmap (NULL, r->map_len, PROT_READ, MAP_PRIVATE, fd, 0);
  close (fd);
  if (r->map == MAP_FAILED) { set_err (errbuf, errlen, "cannot map %s", filename); free (r); return NULL; }
  memcpy (&r->h, r->map, sizeof r->h);
  const struct uvdb_header *h = &r->h;
  if (memcmp (h->magic, UVDB_MAGIC, 8) != 0 || (h->version != 1 && h->version != 2)) {
    set_err (errbuf, errlen, "%s is not a packed uvaia database (version 1 or 2)", filename);
    uvdb_close_reader (r); return NULL;
  }
  const uint64_t n = h->n_ref, flen = (uint64_t) r->map_len;
  uint64_t heads_cap = 0, lits_cap = 0;
  if (h->version == 2) {
    if (compact_layout (r, &heads_cap, &lits_cap)) {
      set_err (errbuf, errlen, "%s is truncated or inconsistent", filename);
      uvdb_close_reader (r); return NULL;
    }
  } else {
  /* every section size is computed with overflow checks: a hostile header must not wrap a product into a small number */
  uint64_t sz_planes = 0, sz_nonn = 0, sz_side = 0, sz_idx = 0;
  int bad = h->file_bytes != flen || n > (UINT64_MAX >> 8) || h->n_tiles != (n + 63) / 64 || h->nchar == 0 ||
            h->W4 != ((h->nchar + 31) / 32 + 3) / 4 || h->tile_bytes != (uint64_t) h->W4 * 4 * 64 * 16 || h->side_row_ints != UVDB_SIDE_ROW_INTS;
  bad = bad || __builtin_mul_overflow (h->n_tiles, h->tile_bytes, &sz_planes) || __builtin_mul_overflow (h->n_tiles, (uint64_t) 64 * 4, &sz_nonn) ||
        __builtin_mul_overflow (h->n_tiles, (uint64_t) 64 * 4 * h->side_row_ints, &sz_side) || __builtin_mul_overflow (n + 1, (uint64_t) 8, &sz_idx);
  /* sections in file order, each inside the file and in front of the next one */
  bad = bad || h->off_planes < sizeof (struct uvdb_header) || h->off_planes > flen || sz_planes > flen - h->off_planes || h->off_planes + sz_planes > h->off_nonn ||
        h->off_nonn > flen || sz_nonn > flen - h->off_nonn || h->off_nonn + sz_nonn > h->off_side ||
        h->off_side > flen || sz_side > flen - h->off_side || h->off_side + sz_side > h->off_name_idx ||
        h->off_name_idx > flen || sz_idx > flen - h->off_name_idx || h->off_name_idx + sz_idx > h->off_names ||
        h->off_names > h->off_exc_idx || h->off_exc_idx > flen || sz_idx > flen - h->off_exc_idx || h->off_exc_idx + sz_idx > h->off_exc || h->off_exc > flen ||
        (h->off_planes | h->off_nonn | h->off_side | h->off_name_idx | h->off_exc_idx | h->off_exc) % 8 != 0;
  if (bad) {
    set_err (errbuf, errlen, "%s is truncated or inconsistent", filename);
    uvdb_close_reader (r); return NULL;
  }
  }
  r->non_n = (const int32_t *) (r->map + h->off_nonn);
  r->name_idx = (const uint64_t *) (r->map + h->off_name_idx);
  r->names = (const char *) (r->map + h->off_names);
  r->exc_idx = (const uint64_t *) (r->map + h->off_exc_idx);
  r->exc = (const uvdb_exc *) (r->map + h->off_exc);
  {  /* the two index arrays: start at 0, never decrease, end inside their sections; every name ends in NUL inside the names section */
    const uint64_t names_len = h->off_exc_idx - h->off_names, exc_cap = (flen - h->off_exc) / sizeof (uvdb_exc);
    int ok = r->name_idx[0] == 0 && r->exc_idx[0] == 0 && r->name_idx[n] <= names_len && r->exc_idx[n] <= exc_cap &&
             h->off_exc + r->exc_idx[n] * sizeof (uvdb_exc) == flen;
    for (uint64_t i = 0; ok && i < n; i++)
      ok = r->name_idx[i] < r->name_idx[i + 1] && r->name_idx[i + 1] <= names_len && r->exc_idx[i] <= r->exc_idx[i + 1] && r->exc_idx[i + 1] <= exc_cap &&
           r->names[r->name_idx[i + 1] - 1] == '\0';
    if (!ok) {
      set_err (errbuf, errlen, "%s has inconsistent index sections", filename);
      uvdb_close_reader (r); return NULL;
    }
  }
  if (h->version == 2) {  /* what goes to the device unchecked otherwise: valid-site counts within the alignment, every index entry and head */
    int ok = 1;
    for (uint64_t i = 0; ok && i < n; i++) ok = r->non_n[i] >= 0 && (uint32_t) r->non_n[i] <= h->nchar;
    if (!ok) {
      set_err (errbuf, errlen, "%s holds valid-site counts outside the alignment", filename);
      uvdb_close_reader (r); return NULL;
    }
    const int bad_heads = compact_check_heads (r, heads_cap, lits_cap);
    if (bad_heads) {
      set_err (errbuf, errlen, bad_heads & 1 ? "%s has inconsistent index sections" : "%s holds compact records that leave the alignment, overlap, descend or do not match their literals", filename);
      uvdb_close_reader (r); return NULL;
    }
  } else {  /* what goes to the device unchecked otherwise: valid-site counts within the alignment, side rows that list words of the alignment
      * (a count above the capacity only says "incomplete", as the engine writes it) */
    const uint32_t n_words = h->W4 * 4;
    const int32_t *side = (const int32_t *) (r->map + h->off_side);
    int ok = 1;
    for (uint64_t i = 0; ok && i < n; i++) {
      const int32_t *row = side + i * h->side_row_ints;
      ok = r->non_n[i] >= 0 && (uint32_t) r->non_n[i] <= h->nchar && row[0] >= 0;
      for (int k = 0; ok && k < UVDB_SIDE_LISTED && k < row[0]; k++) ok = row[1 + k] >= 0 && (uint32_t) row[1 + k] < n_words;
    }
    if (!ok) {
      set_err (errbuf, errlen, "%s holds valid-site counts or ambiguity rows outside the alignment", filename);
      uvdb_close_reader (r); return NULL;
    }
  }
  return r;
}

const char *
uvdb_name (uvdb_reader r, uint64_t i)
{
  return i < r->h.n_ref ? r->names + r->name_idx[i] : NULL;
}

const void *
uvdb_tile_planes (uvdb_reader r, uint64_t tile)
{
  return r->h.version == 1 && tile < r->h.n_tiles ? r->map + r->h.off_planes + tile * r->h.tile_bytes : NULL;
}

const int32_t *
uvdb_tile_side_rows (uvdb_reader r, uint64_t tile)
{
  return r->h.version == 1 && tile < r->h.n_tiles ? (const int32_t *) (r->map + r->h.off_side) + tile * 64 * r->h.side_row_ints : NULL;
}

int
uvdb_expand_tiles (uvdb_reader r, uint64_t first_tile, uint64_t n_tiles, void *planes_out, int32_t *side_rows_out)
{
  if (!r || !planes_out || first_tile > r->h.n_tiles || n_tiles > r->h.n_tiles - first_tile) return -1;
  const uint32_t W4 = r->h.W4;
  const size_t tile_dwords = (size_t) W4 * 4 * 64 * 4;
#pragma omp parallel for schedule(static)
  for (uint64_t t = 0; t < n_tiles; t++) {
    uint32_t *tile = (uint32_t *) planes_out + t * tile_dwords;
    if (r->h.version == 1) memcpy (tile, uvdb_tile_planes (r, first_tile + t), tile_dwords * 4);
    else {
      for (size_t row = 0; row < (size_t) W4 * 4; row++) for (int lane = 0; lane < 64; lane++) memcpy (tile + (row * 64 + lane) * 4, r->base + row * 4, 16);
      for (int lane = 0; lane < 64; lane++) compact_apply_lane (r, (first_tile + t) * 64 + lane, tile + lane * 4, 1024, 256);
    }
    if (side_rows_out) for (int lane = 0; lane < 64; lane++) {     /* as side_rows_canonical_kernel: ascending words, the first listed, the count as the total */
      int32_t *row = side_rows_out + (t * 64 + lane) * r->h.side_row_ints;
      int cnt = 0;
      memset (row, 0, (size_t) r->h.side_row_ints * sizeof (int32_t));
      for (uint32_t word = 0; word < W4 * 4; word++) {
        const uint32_t *x = tile + ((size_t) (word >> 2) * 256 + lane) * 4 + (word & 3);
        const uint32_t a = x[0], c = x[256], g = x[512], tt = x[768];
        if (((a & c) | (a & g) | (a & tt) | (c & g) | (c & tt) | (g & tt)) == 0) continue;
        if (cnt < UVDB_SIDE_LISTED) { row[1 + cnt] = (int32_t) word; row[12 + 4 * cnt] = (int32_t) a; row[13 + 4 * cnt] = (int32_t) c; row[14 + 4 * cnt] = (int32_t) g; row[15 + 4 * cnt] = (int32_t) tt; }
        cnt++;
      }
      row[0] = cnt;
    }
  }
  return 0;
}

void
uvdb_unpack_reference (uvdb_reader r, uint64_t i, char *out)
{
  /* IUPAC character of a set of bases (bit 0 = A, 1 = C, 2 = G, 3 = T); the empty set is 'N' unless an exception run says otherwise */
  static const char code[16] = {'N', 'A', 'C', 'M', 'G', 'R', 'S', 'V', 'T', 'W', 'Y', 'H', 'K', 'D', 'B', 'N'};
  const uint32_t nchar = r->h.nchar;
  if (r->h.version == 2) {      /* the reference's own words, [word group][plane][4]: the base with its records written over it */
    uint32_t *x = (uint32_t *) malloc ((size_t) r->h.W4 * 64);
    if (!x) { memset (out, 'N', nchar); out[nchar] = '\0'; return; }
    memcpy (x, r->base, (size_t) r->h.W4 * 64);
    compact_apply_lane (r, i, x, 16, 4);
    for (uint32_t s = 0; s < nchar; s++) {
      const uint32_t word = s >> 5, bit = s & 31;
      const uint32_t *b = x + (size_t) (word >> 2) * 16 + (word & 3);
      out[s] = code[((b[0] >> bit) & 1u) | (((b[4] >> bit) & 1u) << 1) | (((b[8] >> bit) & 1u) << 2) | (((b[12] >> bit) & 1u) << 3)];
    }
    free (x);
    out[nchar] = '\0';
    uvdb_apply_exceptions (r, i, out);
    return;
  }
  const uint32_t *w = (const uint32_t *) uvdb_tile_planes (r, i / 64);
  const unsigned lane = (unsigned) (i & 63);
  for (uint32_t s = 0; s < nchar; s++) {
    const uint32_t word = s >> 5, w4 = word >> 2, j = word & 3, bit = s & 31;
    const size_t base = ((size_t) w4 * 4 * 64 + lane) * 4 + j;          /* plane 0 of this lane: 16-byte words, 64 lanes per plane */
    const unsigned a = (w[base] >> bit) & 1u, c = (w[base + 256] >> bit) & 1u, g = (w[base + 512] >> bit) & 1u, t = (w[base + 768] >> bit) & 1u;
    out[s] = code[a | (c << 1) | (g << 2) | (t << 3)];
  }
  out[nchar] = '\0';
  uvdb_apply_exceptions (r, i, out);
}

void
uvdb_apply_exceptions (uvdb_reader r, uint64_t i, char *row)
{
  const uint32_t nchar = r->h.nchar;
  if (i >= r->h.n_ref) return;
  for (uint64_t e = r->exc_idx[i]; e < r->exc_idx[i + 1]; e++) {
    const uint32_t pos = r->exc[e].pos, len = r->exc[e].len_char >> 8;
    const char ch = (char) (r->exc[e].len_char & 0xFFu);
    for (uint32_t s = pos; s < nchar && s - pos < len; s++) row[s] = ch;
  }
}

int
uvdb_radius_filter_is_exact (int nchar, double ball_ambiguity, double pack_ambiguity)
{
  return (int) (nchar * ball_ambiguity) >= (int) (nchar * (1. - pack_ambiguity));
}

void
uvdb_close_reader (uvdb_reader r)
{
  if (!r) return;
  if (r->map && r->map != MAP_FAILED) munmap ((void *) r->map, r->map_len);
  free (r);
}
