/*
 * uvdb_encoded_check.c -- stand-alone host program for a sanitizer run of the writer's entry for compact records somebody else encoded
 * (uvdb_compact_base, uvdb_add_tiles_encoded in uvaia_amd/csrc/host/uvdb.c), sibling of uvdb_compact_check.c.  It writes a compact file of more
 * than UVDB_BASE_SAMPLE references with the host writer, then writes it again spliced -- dense tiles until the base is fixed, the rest as
 * records sliced out of the first file, in chunks of 1, 3 and all tiles -- and expects the same bytes; in between it hands in records
 * damaged in one place each and expects every one refused with nothing appended.  No GPU, no Python:
 *
 *   gcc -std=gnu11 -g -O1 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all -Iuvaia_amd/csrc/host \
 *       tools/uvdb_encoded_check.c uvaia_amd/csrc/host/uvdb.c -o /tmp/uvdb_encoded_check && /tmp/uvdb_encoded_check /tmp/check.uvdb
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uvdb.h"

static uint32_t rng_state = 4321u;
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
same_bytes (const char *a, const char *b)
{
  FILE *fa = fopen (a, "rb"), *fb = fopen (b, "rb");
  int same = fa && fb, ca, cb;
  while (same) { ca = fgetc (fa); cb = fgetc (fb); if (ca != cb) same = 0; if (ca == EOF || cb == EOF) break; }
  if (fa) fclose (fa);
  if (fb) fclose (fb);
  return same;
}

static int
run (const char *path, int nchar, int n_ref, int chunk)
{
  const int W4 = ((nchar + 31) / 32 + 3) / 4, n_tiles = (n_ref + 63) / 64;
  const size_t tb = (size_t) W4 * 4 * 64 * 16;
  char **seq = (char **) malloc ((size_t) n_ref * sizeof (char *));
  uint32_t *planes = (uint32_t *) calloc ((size_t) n_tiles, tb);
  int32_t *non_n = (int32_t *) calloc ((size_t) n_tiles * 64, sizeof (int32_t));
  char *root = (char *) malloc ((size_t) nchar + 1), name[32], err[512], spliced[4096];
  snprintf (spliced, sizeof spliced, "%s.spliced", path);
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
  /* the reference: the host writer, everything at once */
  uvdb_writer w = uvdb_create_compact (path, nchar, tb, UVDB_SIDE_ROW_INTS, 0.5);
  if (!w) FAIL ("cannot create %s", path);
  for (int i = 0; i < n_ref; i++) { snprintf (name, sizeof name, "ref%d", i); if (uvdb_add_reference (w, name, seq[i])) FAIL ("add_reference"); }
  if (uvdb_add_tiles (w, (size_t) n_tiles, planes, non_n, NULL) || uvdb_close (w)) FAIL ("host writer");
  uvdb_reader r = uvdb_open (path, err, sizeof err);
  if (!r) FAIL ("uvdb_open: %s", err);
  /* the splice */
  w = uvdb_create_compact (spliced, nchar, tb, UVDB_SIDE_ROW_INTS, 0.5);
  if (!w) FAIL ("cannot create %s", spliced);
  if (uvdb_compact_base (w) || uvdb_add_tiles_encoded (w, 1, r->non_n, r->head_idx, r->heads, r->lit_idx, r->lits) != -1) FAIL ("records taken before the base is fixed");
  int t = 0;
  for (; t < n_tiles && !uvdb_compact_base (w); t++) {
    for (int i = t * 64; i < (t + 1) * 64 && i < n_ref; i++) { snprintf (name, sizeof name, "ref%d", i); if (uvdb_add_reference (w, name, seq[i])) FAIL ("add_reference"); }
    if (uvdb_add_tiles (w, 1, planes + (size_t) t * (tb / 4), non_n + t * 64, NULL)) FAIL ("add_tiles");
  }
  if (!uvdb_compact_base (w) || t != UVDB_BASE_SAMPLE / 64 || t >= n_tiles) FAIL ("the base was fixed after %d tiles", t);
  if (memcmp (uvdb_compact_base (w), r->base, (size_t) W4 * 64)) FAIL ("the bases differ");
  for (int i = t * 64; i < n_ref; i++) { snprintf (name, sizeof name, "ref%d", i); if (uvdb_add_reference (w, name, seq[i])) FAIL ("add_reference"); }
  /* damaged records of the remaining tiles: each refused, nothing appended */
  const uint64_t lanes = (uint64_t) n_tiles * 64, l0 = (uint64_t) t * 64, n_heads = r->head_idx[lanes];
  const size_t rest = (size_t) (n_tiles - t);
  uint32_t *heads = (uint32_t *) malloc ((size_t) (n_heads + 1) * sizeof (uint32_t));
  uint64_t *idx = (uint64_t *) malloc ((size_t) (lanes + 1) * sizeof (uint64_t));
  uint64_t two = lanes, lit = lanes;             /* a lane with two heads or more; a lane with a literal head */
  for (uint64_t g = l0; g < lanes; g++) {
    const uint64_t hb = r->head_idx[g], he = r->head_idx[g + 1];
    if (two == lanes && he - hb >= 2) two = g;
    if (lit == lanes) for (uint64_t k = hb; k < he; k++) if (UVDB_HEAD_LITERAL (r->heads[k])) lit = g;
  }
  if ((two == lanes || lit == lanes) && n_ref >= 4200) FAIL ("the rows do not hold the lanes the damaged records need");   /* (a single lane behind the sample may not) */
  int refused = 0, tried = 0;
  for (int kind = 0; kind < 7; kind++) {
    memcpy (heads, r->heads, (size_t) n_heads * sizeof (uint32_t));
    memcpy (idx, r->head_idx, (size_t) (lanes + 1) * sizeof (uint64_t));
    const uint64_t *hidx = r->head_idx, *lidx = r->lit_idx;
    if ((kind != 4 && kind != 5 && two == lanes) || ((kind == 4 || kind == 5) && lit == lanes)) continue;
    const uint64_t k2 = r->head_idx[two < lanes ? two : l0];
    if (kind == 0) { const uint32_t h = heads[k2]; heads[k2] = heads[k2 + 1]; heads[k2 + 1] = h; }                                  /* descending */
    if (kind == 1) heads[k2] = UVDB_HEAD (UVDB_HEAD_FIRST (heads[k2]), UVDB_HEAD_FIRST (heads[k2 + 1]) - UVDB_HEAD_FIRST (heads[k2]) + 1, UVDB_HEAD_LITERAL (heads[k2]), UVDB_HEAD_CODE (heads[k2]));   /* overlap: reaches into the next head's first word */
    if (kind == 2) heads[k2] &= ~(0x7FFu << 5);                                                                                     /* no words */
    if (kind == 3) heads[r->head_idx[two + 1] - 1] = UVDB_HEAD ((uint32_t) W4 * 4 - 1, 2, 0, 0);                                     /* leaves the alignment */
    if (kind == 4) for (uint64_t k = r->head_idx[lit]; k < r->head_idx[lit + 1]; k++) if (UVDB_HEAD_LITERAL (heads[k])) { heads[k] &= ~(1u << 4); break; }   /* literal count */
    if (kind == 5) { memcpy (idx, r->lit_idx, (size_t) (lanes + 1) * sizeof (uint64_t)); for (uint64_t g = lit + 1; g <= lanes; g++) idx[g]++; lidx = idx; }   /* literal extent */
    if (kind == 6) { idx[two + 1] = idx[two] ? idx[two] - 1 : idx[lanes] + 1; hidx = idx; }                                          /* an index that falls back */
    tried++;
    if (uvdb_add_tiles_encoded (w, rest, r->non_n + l0, hidx + l0, heads, lidx + l0, r->lits) == -1) refused++;
  }
  if (refused != tried) FAIL ("%d of %d damaged sets of records were taken", tried - refused, tried);
  for (; t < n_tiles; ) {
    const int nt = chunk && t + chunk < n_tiles ? chunk : n_tiles - t;
    if (uvdb_add_tiles_encoded (w, (size_t) nt, r->non_n + (size_t) t * 64, r->head_idx + (size_t) t * 64, r->heads, r->lit_idx + (size_t) t * 64, r->lits)) FAIL ("good records refused at tile %d", t);
    t += nt;
  }
  if (uvdb_close (w)) FAIL ("close");
  if (!same_bytes (path, spliced)) FAIL ("the spliced file differs (%d sites, %d references, chunks of %d)", nchar, n_ref, chunk);
  printf ("%d sites, %d references, chunks of %d tiles: spliced file equal, %d damaged sets of records refused\n", nchar, n_ref, chunk, refused);
  uvdb_close_reader (r);
  remove (spliced);
  for (int i = 0; i < n_ref; i++) free (seq[i]);
  free (seq); free (planes); free (non_n); free (root); free (heads); free (idx);
  return 0;
}

int
main (int argc, char **argv)
{
  if (argc < 2) { fprintf (stderr, "usage: %s <scratch file>\n", argv[0]); return 2; }
  static const int shapes[][3] = {{300, 4097, 1}, {300, 4300, 3}, {300, 4200, 0}, {2500, 4200, 2}};
  for (size_t k = 0; k < sizeof shapes / sizeof shapes[0]; k++) if (run (argv[1], shapes[k][0], shapes[k][1], shapes[k][2])) return 1;
  remove (argv[1]);
  return 0;
}
