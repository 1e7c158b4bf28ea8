/*
 * uvdb_compact_check.c -- stand-alone host program for a sanitizer run of the compact packed database code (uvaia_amd/csrc/host/uvdb.c):
 * writes a compact file from dense tiles it packs itself, opens it (all of uvdb_open's checks), expands it and unpacks every reference,
 * and compares with what went in; then damages single fields of the file and expects each copy to be refused.  No GPU, no Python:
 *
 *   gcc -std=gnu11 -g -O1 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all -Iuvaia_amd/csrc/host \
 *       tools/uvdb_compact_check.c uvaia_amd/csrc/host/uvdb.c -o /tmp/uvdb_compact_check && /tmp/uvdb_compact_check /tmp/check.uvdb
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uvdb.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd (void) { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint32_t
code_of (char ch)
{
  static const char set[] = "NACMGRSVTWYHKDB";
  const char *p = strchr (set, ch);
  return (p && *p) ? (uint32_t) (p - set) : 0u;
}

#define FAIL(...) do { fprintf (stderr, __VA_ARGS__); fprintf (stderr, "\n"); return 1; } while (0)

static int
run (const char *path, int nchar, int n_ref, int chunk_tiles)
{
  const int W4 = ((nchar + 31) / 32 + 3) / 4, n_tiles = (n_ref + 63) / 64;
  const size_t tb = (size_t) W4 * 4 * 64 * 16;
  char **seq = (char **) malloc ((size_t) n_ref * sizeof (char *));
  uint32_t *planes = (uint32_t *) calloc ((size_t) (n_tiles ? n_tiles : 1), tb), *got = (uint32_t *) malloc ((size_t) (n_tiles ? n_tiles : 1) * tb);
  int32_t *non_n = (int32_t *) calloc ((size_t) (n_tiles ? n_tiles : 1) * 64, sizeof (int32_t)), *side = (int32_t *) malloc ((size_t) (n_tiles ? n_tiles : 1) * 64 * UVDB_SIDE_ROW_INTS * sizeof (int32_t));
  char *root = (char *) malloc ((size_t) nchar + 1), *text = (char *) malloc ((size_t) nchar + 1), name[32], err[512];
  for (int s = 0; s < nchar; s++) root[s] = "ACGT"[rnd () & 3];
  root[nchar] = '\0';
  for (int i = 0; i < n_ref; i++) {
    seq[i] = strdup (root);
    for (int k = (int) (rnd () % 6); k > 0; k--) seq[i][rnd () % (uint32_t) nchar] = "ACGTRYKMSWN-?"[rnd () % 13];
    if (i % 3 == 1) for (int s = 0, e = (int) (rnd () % 200); s < e && s < nchar; s++) seq[i][s] = 'N';
    if (i % 5 == 2) for (int s = (int) (rnd () % (uint32_t) nchar), e = s + 70; s < e && s < nchar; s++) seq[i][s] = '-';
    if (i % 11 == 7) memset (seq[i], 'N', (size_t) nchar);
    for (int s = 0; s < nchar; s++) {
      const uint32_t c = code_of (seq[i][s]), word = (uint32_t) s >> 5;
      uint32_t *x = planes + (size_t) (i / 64) * (tb / 4) + ((size_t) (word >> 2) * 256 + (size_t) (i % 64)) * 4 + (word & 3);
      for (int p = 0; p < 4; p++) if ((c >> p) & 1u) x[p * 256] |= 1u << (s & 31);
      non_n[i] += c != 0;
    }
  }
  uvdb_writer w = uvdb_create_compact (path, nchar, tb, UVDB_SIDE_ROW_INTS, 0.5);
  if (!w) FAIL ("cannot create %s", path);
  for (int t = 0; t < n_tiles; t += chunk_tiles) {
    const int e = t + chunk_tiles < n_tiles ? t + chunk_tiles : n_tiles;
    for (int i = t * 64; i < e * 64 && i < n_ref; i++) { snprintf (name, sizeof name, "ref%d", i); if (uvdb_add_reference (w, name, seq[i])) FAIL ("add_reference"); }
    if (uvdb_add_tiles (w, (size_t) (e - t), planes + (size_t) t * (tb / 4), non_n + t * 64, NULL)) FAIL ("add_tiles");
  }
  if (uvdb_close (w)) FAIL ("close");
  uvdb_reader r = uvdb_open (path, err, sizeof err);
  if (!r) FAIL ("uvdb_open: %s", err);
  if (r->h.version != 2 || r->h.n_ref != (uint64_t) n_ref || uvdb_tile_planes (r, 0) || uvdb_tile_side_rows (r, 0)) FAIL ("header");
  if (n_tiles && (uvdb_expand_tiles (r, 0, (uint64_t) n_tiles, got, side) || memcmp (got, planes, (size_t) n_tiles * tb))) FAIL ("expanded tiles differ (%d sites, %d references)", nchar, n_ref);
  if (n_tiles > 1 && (uvdb_expand_tiles (r, 1, (uint64_t) n_tiles - 1, got, NULL) || memcmp (got, planes + tb / 4, (size_t) (n_tiles - 1) * tb))) FAIL ("expanded tiles from tile 1 differ");
  for (int i = 0; i < n_ref; i++) {
    uvdb_unpack_reference (r, (uint64_t) i, text);
    if (strcmp (text, seq[i])) FAIL ("text of reference %d differs", i);
  }
  /* damaged copies: every one is refused, none is read out of bounds */
  const uint64_t off_hidx = r->h.off_side, off_heads = r->h.reserved[0], off_lidx = r->h.reserved[1], lanes = r->h.n_tiles * 64, len = r->map_len;
  const uint64_t n_heads = lanes ? r->head_idx[lanes] : 0;
  unsigned char *copy = (unsigned char *) malloc (len);
  char bad_path[4096];
  snprintf (bad_path, sizeof bad_path, "%s.bad", path);
  int refused = 0, tried = 0;
  for (int kind = 0; kind < 6 && n_heads > 2; kind++) {
    memcpy (copy, r->map, len);
    uint64_t big = UINT64_MAX / 3, cut = len;
    uint32_t h = 0;
    if (kind == 0) memcpy (copy + off_hidx + 8 * lanes, &big, 8);                         /* an index beyond its section */
    if (kind == 1) memcpy (copy + off_lidx + 8 * (lanes / 2), &big, 8);                   /* an index that jumps and falls back */
    if (kind == 2) { h = UVDB_HEAD (1, 0, 0, 0); memcpy (copy + off_heads, &h, 4); }        /* no words */
    if (kind == 3) { h = UVDB_HEAD (65535, 2047, 1, 0); memcpy (copy + off_heads + 4 * (n_heads - 1), &h, 4); }   /* far beyond the alignment */
    if (kind == 4) { memcpy (&h, copy + off_heads, 4); h ^= 1u << 4; memcpy (copy + off_heads, &h, 4); }          /* literal bit flipped */
    if (kind == 5) cut = len - 8;
    FILE *f = fopen (bad_path, "wb");
    if (!f || fwrite (copy, 1, cut, f) != cut || fclose (f)) FAIL ("cannot write %s", bad_path);
    uvdb_reader b = uvdb_open (bad_path, err, sizeof err);
    tried++;
    if (b) uvdb_close_reader (b); else refused++;
  }
  remove (bad_path);
  if (refused != tried) FAIL ("%d of %d damaged files were opened", tried - refused, tried);
  printf ("%d sites, %d references: round trip exact, %d damaged copies refused\n", nchar, n_ref, refused);
  uvdb_close_reader (r);
  for (int i = 0; i < n_ref; i++) free (seq[i]);
  free (seq); free (planes); free (got); free (non_n); free (side); free (root); free (text); free (copy);
  return 0;
}

int
main (int argc, char **argv)
{
  if (argc < 2) { fprintf (stderr, "usage: %s <scratch file>\n", argv[0]); return 2; }
  static const int shapes[][3] = {{29, 1, 1}, {130, 65, 1}, {1000, 130, 2}, {1000, 64, 64}, {70000, 5, 1}, {29, 4200, 16}, {2500, 4300, 7}};
  for (size_t k = 0; k < sizeof shapes / sizeof shapes[0]; k++) if (run (argv[1], shapes[k][0], shapes[k][1], shapes[k][2])) return 1;
  remove (argv[1]);
  return 0;
}
