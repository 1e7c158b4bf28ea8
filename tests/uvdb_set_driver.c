/*
 * uvdb_set_driver.c -- a stand-alone program (host code only, no GPU) that writes small packed databases with uvdb.c and drives
 * uvdb_set.c over them: tests/test_packed_set_cpu.py builds it with -fsanitize=address,undefined and runs it.  Every check restates
 * what the call promises by brute force; the first miss ends the program with status 1 and a line on stderr.
 *
 *   uvdb_set_driver <directory to write into>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uvdb.h"
#include "uvdb_set.h"

#define NCHAR 100
#define CHECK(cond) do { if (!(cond)) { fprintf (stderr, "line %d: %s\n", __LINE__, #cond); exit (1); } } while (0)

static size_t
tile_bytes (int nchar)
{
  return (size_t) (((nchar + 31) / 32 + 3) / 4) * 4 * 64 * 16;
}

/* file number f with n references of nchar sites: reference r reads A everywhere but a run of '-' of r % 7 sites at site r % 50 */
static void
write_file (const char *path, int f, int n, int nchar, double ambiguity)
{
  const size_t tb = tile_bytes (nchar), nt = ((size_t) n + 63) / 64;
  uvdb_writer w = uvdb_create (path, nchar, tb, UVDB_SIDE_ROW_INTS, ambiguity);
  CHECK (w);
  char *seq = (char *) malloc ((size_t) nchar + 1), name[64];
  unsigned char *planes = (unsigned char *) calloc (nt ? nt : 1, tb);
  int *non_n = (int *) calloc ((nt ? nt : 1) * 64, sizeof (int)), *side = (int *) calloc ((nt ? nt : 1) * 64 * UVDB_SIDE_ROW_INTS, sizeof (int));
  CHECK (seq && planes && non_n && side);
  for (int r = 0; r < n; r++) {
    memset (seq, 'A', (size_t) nchar); seq[nchar] = '\0';
    for (int s = 0; s < r % 7; s++) seq[r % 50 + s] = '-';
    snprintf (name, sizeof name, "f%d_r%d", f, r);
    CHECK (uvdb_add_reference (w, name, seq) == 0);
    non_n[r] = nchar - r % 7;
    for (int s = 0; s < nchar; s++) if (seq[s] == 'A') {      /* plane A, bit s of word s / 32 */
      const size_t word = (size_t) s / 32, at = (size_t) (r / 64) * tb + (((word / 4) * 4 + 0) * 64 + (size_t) (r % 64)) * 16 + (word % 4) * 4;
      planes[at + (size_t) (s % 32) / 8] |= (unsigned char) (1u << (s % 8));
    }
  }
  CHECK (uvdb_add_tiles (w, nt, planes, non_n, side) == 0);
  CHECK (uvdb_close (w) == 0);
  free (seq); free (planes); free (non_n); free (side);
}

static void
check_span (uvdb_set s, const uint64_t *keep, uint64_t a, uint64_t b)
{
  uvdb_set_piece pieces[UVDB_SET_MAX_FILES];
  int np = -1, counted = -1;
  uint64_t st = 0, st2 = 0;
  int *sel = (int *) malloc ((size_t) (b - a) * sizeof (int));
  CHECK (sel);
  CHECK (uvdb_set_span (s, keep, a, b, pieces, UVDB_SET_MAX_FILES, &np, &st, sel) == 0);
  CHECK (uvdb_set_span (s, keep, a, b, NULL, 0, &counted, &st2, NULL) == 0 && counted == np && st2 == st);
  uint64_t at = 0;
  for (int p = 0; p < np; p++) {         /* pieces: in file order, one after the other in the slot, inside their files */
    CHECK (pieces[p].slot_tile == at && pieces[p].n_tiles >= 1 && pieces[p].first_tile + pieces[p].n_tiles <= s->db[pieces[p].file]->h.n_tiles);
    CHECK (p == 0 || pieces[p].file > pieces[p - 1].file);
    at += pieces[p].n_tiles;
  }
  CHECK (at == st);
  for (uint64_t k = a; k < b; k++) {     /* every kept reference lies where its sel entry says, in the piece of its file */
    const uint64_t i = keep ? keep[k] : k;
    int f = -1, found = 0; uint64_t l = 0;
    CHECK (uvdb_set_locate (s, i, &f, &l) == 0);
    CHECK (sel[k - a] >= 0 && (uint64_t) sel[k - a] < st * 64 && (k == a || sel[k - a] > sel[k - a - 1]));
    for (int p = 0; p < np; p++) if (pieces[p].file == f) {
      found = 1;
      CHECK ((uint64_t) sel[k - a] == pieces[p].slot_tile * 64 + (l - pieces[p].first_tile * 64));
    }
    CHECK (found);
  }
  if (np >= 2) CHECK (uvdb_set_span (s, keep, a, b, pieces, np - 1, &np, &st, sel) == -1);      /* too few entries: refused, nothing past them written */
  free (sel);
}

/* uvdb_set_direct_tiles by brute force: yes exactly when every reference of [a, b) lies in one file at the lane of its place in the range,
 * the tile that is not filled ends the stream, and the store ends on a tile */
static void
check_direct (uvdb_set s, const uint64_t *keep, uint64_t a, uint64_t b, uint64_t n, uint64_t store)
{
  int f = -7, want = keep == NULL && a < b && b <= n && n == s->n_ref && store % 64 == 0 && ((b - a) % 64 == 0 || b == n);
  uint64_t t = 77, l0 = 0;
  int f0 = -1;
  for (uint64_t k = a; want && k < b; k++) {
    int fk = -1; uint64_t l = 0;
    CHECK (uvdb_set_locate (s, k, &fk, &l) == 0);
    if (k == a) { f0 = fk; l0 = l; }
    if (fk != f0 || l != l0 + (k - a) || l0 % 64) want = 0;
  }
  const int rc = uvdb_set_direct_tiles (s, keep, a, b, n, store, &f, &t);
  CHECK (rc == (want ? 0 : -1));
  if (want) {
    CHECK (f == f0 && t == l0 / 64 && t + (b - a + 63) / 64 <= s->db[f]->h.n_tiles);
    CHECK (uvdb_set_direct_tiles (s, keep, a, b, n, store, NULL, NULL) == 0);
  } else CHECK (f == -7 && t == 77);      /* nothing written with a no */
}

int
main (int argc, char **argv)
{
  if (argc != 2) { fprintf (stderr, "usage: %s <directory>\n", argv[0]); return 2; }
  static const int sizes[] = {1, 63, 64, 65, 0, 130, 5};
  enum { NF = sizeof sizes / sizeof sizes[0] };
  char path[NF + 2][1024], msg[1024];
  const char *files[NF + 2];
  uint64_t total = 0;
  for (int f = 0; f < NF; f++) {
    snprintf (path[f], sizeof path[f], "%s/set%d.uvdb", argv[1], f);
    write_file (path[f], f, sizes[f], NCHAR, 0.5);
    files[f] = path[f];
    total += (uint64_t) sizes[f];
  }
  snprintf (path[NF], sizeof path[NF], "%s/other_nchar.uvdb", argv[1]);
  write_file (path[NF], NF, 3, NCHAR + 29, 0.5);
  snprintf (path[NF + 1], sizeof path[NF + 1], "%s/other_a.uvdb", argv[1]);
  write_file (path[NF + 1], NF + 1, 3, NCHAR, 0.25);

  uvdb_set s = uvdb_set_open (files, NF, 0, msg, sizeof msg);
  CHECK (s && s->n_ref == total && s->n_files == NF && s->nchar == NCHAR && s->ref_ambiguity == 0.5);
  char text[NCHAR + 1], want[NCHAR + 1], name[64];
  uint64_t i = 0;
  for (int f = 0; f < NF; f++) for (int r = 0; r < sizes[f]; r++, i++) {
    int gf = -1; uint64_t gl = 0;
    const uvdb_exc *runs = NULL;
    CHECK (uvdb_set_locate (s, i, &gf, &gl) == 0 && gf == f && gl == (uint64_t) r);
    snprintf (name, sizeof name, "f%d_r%d", f, r);
    CHECK (strcmp (uvdb_set_name (s, i), name) == 0);
    CHECK (uvdb_set_non_n (s, i) == NCHAR - r % 7);
    memset (want, 'A', NCHAR); want[NCHAR] = '\0';
    for (int k = 0; k < r % 7; k++) want[r % 50 + k] = '-';
    uvdb_set_unpack_reference (s, i, text);
    CHECK (memcmp (text, want, NCHAR + 1) == 0);
    for (int k = 0; k < NCHAR; k++) if (text[k] == '-') text[k] = 'N';
    uvdb_set_apply_exceptions (s, i, text);
    CHECK (memcmp (text, want, NCHAR + 1) == 0);
    CHECK (uvdb_set_runs (s, i, &runs) == (size_t) (r % 7 ? 1 : 0) && (r % 7 == 0 || (runs && runs[0].pos == (uint32_t) (r % 50) && runs[0].len_char == (((uint32_t) (r % 7) << 8) | '-'))));
  }
  CHECK (uvdb_set_locate (s, total, NULL, NULL) == -1 && uvdb_set_name (s, total) == NULL && uvdb_set_non_n (s, total) == -1);

  /* spans: everything, every window of 64 and of 100, and kept lists with holes at the file boundaries */
  check_span (s, NULL, 0, total);
  for (uint64_t w = 64; w <= 100; w += 36) for (uint64_t a = 0; a < total; a += w) check_span (s, NULL, a, a + w < total ? a + w : total);
  /* chunks that go straight from a mapping: every chunk of 64, 100 and 128 into stores that end on a tile and inside one; the refusals */
  for (uint64_t w = 64; w <= 128; w += (w == 64 ? 36 : 28)) for (uint64_t a = 0; a < total; a += w) for (uint64_t store = 0; store <= 70; store += (store ? 6 : 64))
    check_direct (s, NULL, a, a + w < total ? a + w : total, total, store);
  check_direct (s, NULL, 0, 64, total, 0);
  check_direct (s, NULL, 64, 127, total, 64);          /* file 2 from its lane 0, one reference short of its tile */
  check_direct (s, NULL, 5, 5, total, 0);
  check_direct (s, NULL, total - 5, total, total, 0);  /* the last file, from its lane 0 to the end of the stream */
  check_direct (s, NULL, total, total + 64, total + 64, 0);
  check_direct (s, NULL, 0, total + 1, total + 1, 0);
  uint64_t *keep = (uint64_t *) malloc ((size_t) total * sizeof (uint64_t)), n = 0;
  CHECK (keep);
  for (i = 0; i < total; i++) {
    int f = -1; uint64_t l = 0;
    uvdb_set_locate (s, i, &f, &l);
    if (l == 0 || l + 1 == (uint64_t) sizes[f] || i % 11 == 3) continue;      /* the first and the last reference of every file, and some more */
    keep[n++] = i;
  }
  CHECK (n > 100 && n < total);
  check_span (s, keep, 0, n);
  for (uint64_t a = 0; a < n; a += 50) check_span (s, keep, a, a + 50 < n ? a + 50 : n);
  for (uint64_t a = 0; a < n; a += 64) check_direct (s, keep, a, a + 64 < n ? a + 64 : n, n, 0);       /* a keep list: never */
  CHECK (uvdb_set_span (s, keep, 3, 3, NULL, 0, NULL, NULL, NULL) == -1);
  CHECK (uvdb_set_span (s, NULL, 0, total + 1, NULL, 0, NULL, NULL, NULL) == -1);
  keep[5] = keep[4];                       /* not increasing */
  CHECK (uvdb_set_span (s, keep, 0, n, NULL, 0, NULL, NULL, NULL) == -1);
  keep[5] = total;                         /* outside the stream */
  CHECK (uvdb_set_span (s, keep, 0, n, NULL, 0, NULL, NULL, NULL) == -1);
  free (keep);
  uvdb_set_close (s);

  /* refusals name both files */
  files[2] = path[NF];
  CHECK (uvdb_set_open (files, NF, 0, msg, sizeof msg) == NULL && strstr (msg, path[NF]) && strstr (msg, path[0]) && strstr (msg, "sites"));
  files[2] = path[NF + 1];
  CHECK (uvdb_set_open (files, NF, 0, msg, sizeof msg) == NULL && strstr (msg, path[NF + 1]) && strstr (msg, path[0]) && strstr (msg, "-A 0.25") && strstr (msg, "uvaiapack --merge -A"));
  s = uvdb_set_open (files, NF, UVDB_SET_ANY_AMBIGUITY, msg, sizeof msg);
  CHECK (s && s->ref_ambiguity == 0.5 && s->n_ref == total - 64 + 3);
  uvdb_set_close (s);
  files[2] = "/nonexistent/file.uvdb";
  CHECK (uvdb_set_open (files, NF, 0, msg, sizeof msg) == NULL && strstr (msg, "/nonexistent/file.uvdb"));
  CHECK (uvdb_set_open (files, 0, 0, msg, sizeof msg) == NULL && uvdb_set_open (files, UVDB_SET_MAX_FILES + 1, 0, msg, sizeof msg) == NULL);
  uvdb_set_close (NULL);
  printf ("uvdb_set driver: ok\n");
  return 0;
}
