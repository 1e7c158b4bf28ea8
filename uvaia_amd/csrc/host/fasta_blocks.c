/* fasta_blocks.c -- see fasta_blocks.h */
#define _GNU_SOURCE
#include "fasta_blocks.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "biomcmc_lite.h"

/* ------------------------------------------------------------------------------------------------ pass 1 in plain C */
static int
is_white (unsigned char c)
{ return c == ' ' || (c >= 9 && c <= 13); }

/* the record whose header line begins at start, with its first '>' at g, and that ends at end */
static void
record_fields (const char *text, size_t start, size_t g, size_t end, uvaia_gpu_fasta_record *r, size_t *first_nul)
{
  const char *nl = (const char *) memchr (text + g, '\n', end - g);
  const size_t nlpos = nl ? (size_t) (nl - text) : end;
  size_t last = g;                                     /* the last byte of the name that is no '\r' */
  for (size_t i = g + 1; i < nlpos; i++) if (text[i] != '\r') last = i;
  const size_t body = nlpos + 1 < end ? nlpos + 1 : end;
  size_t sites = 0, invalid = 0;
  for (size_t i = body; i < end; i++) {
    const unsigned char c = (unsigned char) text[i], up = c & 0xDF;
    if (is_white (c)) continue;
    sites++;
    invalid += (size_t) ((up == 'N') | (up == 'X') | (up == 'O') | (c == '-') | (c == '?') | (c == '.'));
  }
  const char *z = (const char *) memchr (text + start, 0, end - start);
  *first_nul = z ? (size_t) (z - text) : end;
  r->name_off = (uint32_t) (g + 1 < end ? g + 1 : end); r->name_len = (uint32_t) (last - g);
  r->body_off = (uint32_t) body; r->body_len = (uint32_t) (end - body);
  r->seq_len = (uint32_t) sites; r->non_n = (int32_t) (sites - invalid);
  r->flags = (z ? UVAIA_GPU_FASTA_NUL : 0u) | (sites ? 0u : UVAIA_GPU_FASTA_EMPTY);
  r->bad_off = z ? (uint32_t) (z - text) : 0u;
}

int
fasta_scan_host (const char *text, size_t n, int final, int max_records, uvaia_gpu_fasta_record *rec, int *n_records, size_t *consumed, int *bad_kind, size_t *bad_off)
{
  *n_records = 0; *consumed = 0; *bad_kind = FASTA_BAD_NONE; *bad_off = 0;
  if (max_records < 1 || n == 0) return 0;
  const size_t cap = (size_t) max_records + 1;
  size_t *hdr_gt = (size_t *) biomcmc_malloc (2 * cap * sizeof (size_t)), *hdr_line = hdr_gt + cap, known = 0;
  for (size_t ls = 0; ls < n && known < cap;) {       /* the header lines: a line with a '>' anywhere, also one the text cuts */
    const char *nl = (const char *) memchr (text + ls, '\n', n - ls);
    const size_t le = nl ? (size_t) (nl - text) : n;
    const char *gt = (const char *) memchr (text + ls, '>', le - ls);
    if (gt) { hdr_gt[known] = (size_t) (gt - text); hdr_line[known] = ls; known++; }
    ls = le + 1;
  }
  const size_t n_rec = known == cap ? (size_t) max_records : (final ? known : (known ? known - 1 : 0));
  const size_t pre_end = known ? hdr_line[0] : n;
  int kind = FASTA_BAD_NONE; size_t where = 0;
  const char *z = (const char *) memchr (text, 0, pre_end);
  if (z) { kind = FASTA_BAD_NUL; where = (size_t) (z - text); }
  else for (size_t i = 0; i < pre_end; i++) if (!is_white ((unsigned char) text[i])) { kind = FASTA_BAD_TEXT; where = i; break; }
  for (size_t k = 0; k < n_rec && !kind; k++) {
    const size_t end = k + 1 < known ? hdr_line[k + 1] : n;
    size_t nul;
    record_fields (text, hdr_line[k], hdr_gt[k], end, rec + k, &nul);
    if (rec[k].flags & UVAIA_GPU_FASTA_NUL) { kind = FASTA_BAD_NUL; where = nul; }
    else if (rec[k].flags & UVAIA_GPU_FASTA_EMPTY) { kind = FASTA_BAD_EMPTY; where = hdr_gt[k]; }
  }
  free (hdr_gt);
  if (kind) { *bad_kind = kind; *bad_off = where; return -1; }
  *n_records = (int) n_rec;
  *consumed = n_rec ? (size_t) rec[n_rec - 1].body_off + rec[n_rec - 1].body_len : pre_end;
  return 0;
}

size_t
fasta_clean_host (const char *text, const uvaia_gpu_fasta_record *rec, char *out)
{
  size_t w = 0;
  for (size_t i = rec->body_off; i < (size_t) rec->body_off + rec->body_len; i++) {
    const unsigned char c = (unsigned char) text[i];
    if (is_white (c)) continue;
    out[w++] = (char) ((c >= 'a' && c <= 'z') ? c - 32 : c);
  }
  return w;
}

int
fasta_count_acgt_host (const char *text, const uvaia_gpu_fasta_record *rec)
{
  int acgt = 0;
  for (size_t i = rec->body_off; i < (size_t) rec->body_off + rec->body_len; i++) {
    const unsigned char up = (unsigned char) text[i] & 0xDF;
    acgt += (up == 'A') | (up == 'C') | (up == 'G') | (up == 'T');
  }
  return acgt;
}

int
fasta_scan_host_step (void *user, const char *text, size_t n, int final, int *n_records, size_t *consumed, int *bad_kind, size_t *bad_off, char *err, size_t errlen)
{
  struct fasta_host_scan *h = (struct fasta_host_scan *) user;
  (void) err; (void) errlen;
  h->n_records = 0;
  if (fasta_scan_host (text, n, final, h->max_records, h->rec, n_records, consumed, bad_kind, bad_off)) return -1;
  h->n_records = *n_records;
  return 0;
}

/* ------------------------------------------------------------------------------------------------ the block reader */
struct fasta_blocks_struct {
  file_compress_t fc;
  char *path;
  size_t block_bytes;
  char *buf[2];
  void (*release) (void *);
  /* the fill under way: buffer, the bytes the tail left at its front, the bytes it holds when filled, did the stream end */
  pthread_t thread; int running, filling;
  size_t front, filled; int at_end;
};

static void *
fill_thread (void *arg)
{
  fasta_blocks fb = (fasta_blocks) arg;
  const size_t want = fb->block_bytes - fb->front;
  const size_t got = biomcmc_read_compress (fb->fc, fb->buf[fb->filling] + fb->front, want);
  fb->filled = fb->front + got;
  fb->at_end = got < want;
  return NULL;
}

static int
start_fill (fasta_blocks fb, int which, size_t front)
{
  fb->filling = which; fb->front = front;
  if (pthread_create (&fb->thread, NULL, fill_thread, fb)) return -1;
  fb->running = 1;
  return 0;
}

static void
wait_fill (fasta_blocks fb)
{
  if (fb->running) pthread_join (fb->thread, NULL);
  fb->running = 0;
}

fasta_blocks
fasta_blocks_open (const char *path, size_t block_bytes, void *(*alloc) (size_t), void (*release) (void *), char *err, size_t errlen)
{
  if (block_bytes < 2) { snprintf (err, errlen, "a text block of %zu bytes", block_bytes); return NULL; }
  FILE *probe = fopen (path, "rb");                    /* (biomcmc_open_compress ends the program where a library must not) */
  if (!probe) { snprintf (err, errlen, "cannot open file %s for reading", path); return NULL; }
  fclose (probe);
  fasta_blocks fb = (fasta_blocks) biomcmc_malloc (sizeof *fb);
  memset (fb, 0, sizeof *fb);
  fb->block_bytes = block_bytes; fb->release = alloc ? release : free;
  for (int i = 0; i < 2; i++) {                        /* one byte of room behind a block: the name of a last line without '\n' ends there */
    fb->buf[i] = (char *) (alloc ? alloc (block_bytes + 16) : malloc (block_bytes + 16));
    if (!fb->buf[i]) { snprintf (err, errlen, "no memory for two text blocks of %zu bytes", block_bytes); fasta_blocks_close (fb); return NULL; }
  }
  fb->path = strdup (path);
  fb->fc = biomcmc_open_compress (path, "r");
  return fb;
}

void
fasta_blocks_close (fasta_blocks fb)
{
  if (!fb) return;
  wait_fill (fb);
  for (int i = 0; i < 2; i++) if (fb->buf[i]) fb->release (fb->buf[i]);
  file_compress_t fc = fb->fc;
  free (fb->path); free (fb);
  if (fc) biomcmc_close_compress (fc);
}

int
fasta_blocks_finish (fasta_blocks fb, char *err, size_t errlen)
{
  if (!fb) return 0;
  wait_fill (fb);
  for (int i = 0; i < 2; i++) if (fb->buf[i]) fb->release (fb->buf[i]);
  const int bad = fb->fc ? biomcmc_close_compress_status (fb->fc) : 0;
  if (bad) snprintf (err, errlen, "reading %s failed: the decompressor reported an error (truncated or corrupt file?)", fb->path);
  free (fb->path); free (fb);
  return bad ? -1 : 0;
}

int
fasta_blocks_run (fasta_blocks fb, int max_records, fasta_scan_fn scan, void *scan_user, fasta_records_fn records, void *records_user, uint64_t *n_bytes, char *err, size_t errlen)
{
  static const char *const what[] = {"", "a NUL byte", "a line that is not blank before the first header line", "a record without sequence, its header"};
  char msg[512];
  uint64_t stream_off = 0;                             /* where the current block begins in the stream */
  if (n_bytes) *n_bytes = 0;
  if (start_fill (fb, 0, 0)) { snprintf (err, errlen, "%s: cannot start the reader thread", fb->path); return -1; }
  for (;;) {
    wait_fill (fb);
    const int cur = fb->filling, final = fb->at_end;
    char *text = fb->buf[cur];
    const size_t n = fb->filled;
    if (n_bytes) *n_bytes = stream_off + n;
    size_t off = 0;
    for (int last = 0; !last;) {
      int nr = 0, kind = FASTA_BAD_NONE; size_t consumed = 0, where = 0;
      msg[0] = '\0';
      if (off < n && scan (scan_user, text + off, n - off, final, &nr, &consumed, &kind, &where, msg, sizeof msg)) {
        if (kind > FASTA_BAD_NONE && kind <= FASTA_BAD_EMPTY) snprintf (err, errlen, "%s: FASTA text: %s at byte %llu of the text", fb->path, what[kind], (unsigned long long) (stream_off + off + where));
        else snprintf (err, errlen, "%s: %s", fb->path, msg);
        return -1;
      }
      if (off == 0 && !final && nr == 0 && consumed == 0) {     /* a full block without one complete record */
        const char *gt = (const char *) memchr (text, '>', n), *nl = gt ? (const char *) memchr (gt, '\n', (size_t) (text + n - gt)) : NULL;
        const int len = gt ? (int) ((nl ? (size_t) (nl - gt) : (size_t) (text + n - gt)) - 1) : 0;
        snprintf (err, errlen, "%s: the record '%.*s' at byte %llu of the text does not fit a block of %zu bytes", fb->path, len > 200 ? 200 : len, gt ? gt + 1 : "", (unsigned long long) stream_off, fb->block_bytes);
        return -1;
      }
      /* a scan that stayed below its cap has returned every complete record of the block: what it did not consume is the tail.  The tail
       * goes to the front of the other buffer and the reader thread fills that one NOW, while this block's records are still to be handed
       * over: reading (and the decompressor behind a pipe) overlaps rows, census, packing and the file's writes */
      last = nr < max_records || off + consumed >= n;
      if (last && !final) {
        const size_t tail = n - (off + consumed);
        memcpy (fb->buf[cur ^ 1], text + off + consumed, tail);
        stream_off += off + consumed;
        if (start_fill (fb, cur ^ 1, tail)) { snprintf (err, errlen, "%s: cannot start the reader thread", fb->path); return -1; }
      }
      if (nr && records (records_user, text + off, consumed, nr, msg, sizeof msg)) { wait_fill (fb); snprintf (err, errlen, "%s: %s", fb->path, msg); return -1; }
      off += consumed;
    }
    if (final) break;
  }
  return 0;
}

/* ------------------------------------------------------------------------------------------------ the whole of a file, for the tests */
struct normalise { struct fasta_host_scan scan; FILE *out; char *seq; size_t seq_cap; };

static int
normalise_records (void *user, char *text, size_t consumed, int n_records, char *err, size_t errlen)
{
  struct normalise *z = (struct normalise *) user;
  (void) consumed;
  for (int k = 0; k < n_records; k++) {
    const uvaia_gpu_fasta_record *r = z->scan.rec + k;
    if (r->seq_len + 1 > z->seq_cap) { z->seq_cap = 2 * (size_t) r->seq_len + 64; z->seq = (char *) biomcmc_realloc (z->seq, z->seq_cap); }
    const size_t len = fasta_clean_host (text, r, z->seq);
    if (len != r->seq_len) { snprintf (err, errlen, "record %d: %zu cleaned bytes, the table says %u", k, len, r->seq_len); return -1; }
    fputc ('>', z->out); fwrite (text + r->name_off, 1, r->name_len, z->out); fputc ('\n', z->out);
    fwrite (z->seq, 1, len, z->out); fputc ('\n', z->out);
  }
  return 0;
}

int
fasta_blocks_normalise_host (const char *path, size_t block_bytes, int max_records, const char *out_path, char *err, size_t errlen)
{
  struct normalise z;
  memset (&z, 0, sizeof z);
  fasta_blocks fb = fasta_blocks_open (path, block_bytes, NULL, NULL, err, errlen);
  if (!fb) return -1;
  z.out = fopen (out_path, "wb");
  if (!z.out) { snprintf (err, errlen, "cannot write %s", out_path); fasta_blocks_close (fb); return -1; }
  z.scan.max_records = max_records;
  z.scan.rec = (uvaia_gpu_fasta_record *) biomcmc_malloc ((size_t) max_records * sizeof (uvaia_gpu_fasta_record));
  int rc = fasta_blocks_run (fb, max_records, fasta_scan_host_step, &z.scan, normalise_records, &z, NULL, err, errlen);
  fclose (z.out);
  free (z.scan.rec); free (z.seq);
  if (rc) fasta_blocks_close (fb);
  else rc = fasta_blocks_finish (fb, err, errlen);
  return rc;
}
