/*
 * uvdb_extract_check.c -- stand-alone host program for a sanitizer run of the extraction routine (uvaia_amd/csrc/host/uvdb_extract.c): its chunk
 * planner, its staging order over two slots and its name table, driven without a GPU.  The eight engine entries the routine calls are
 * restated here on the CPU: a slot is host memory that a stage call fills (a compact piece through uvdb_expand_tiles) and that is poisoned
 * wherever no piece landed, the decode reads the four planes of a lane, and every call checks what the engine's contract lets it assume --
 * capacity reserved first, indices inside the tiles filled, a slot not staged again before it has been read.  Three files (dense, compact,
 * dense) are written from rows packed here, read as one set and extracted whole, by sparse and dense position lists and across the chunk
 * edge; the rows must equal what went in.  No GPU, no Python:
 *
 *   gcc -std=gnu11 -g -O1 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all -Iuvaia_amd/csrc/host -Iinclude tools/uvdb_extract_check.c \
 *       uvaia_amd/csrc/host/uvdb_extract.c uvaia_amd/csrc/host/uvdb_set.c uvaia_amd/csrc/host/uvdb.c -o /tmp/uvdb_extract_check && /tmp/uvdb_extract_check /tmp/check
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uvdb_extract.h"

#define FAIL(...) do { fprintf (stderr, __VA_ARGS__); fprintf (stderr, "\n"); return 1; } while (0)

static uint32_t rng_state = 4711u;
static uint32_t rnd (void) { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint32_t
code_of (char ch)
{
  static const char set[] = "NACMGRSVTWYHKDB";
  const char *p = strchr (set, ch);
  return (p && *p) ? (uint32_t) (p - set) : 0u;
}

/* ---- the engine, restated */
struct uvaia_gpu_ctx {
  int nchar; size_t tb, cap_tiles;
  struct { uint32_t *planes; size_t n_tiles; int unread; } slot[2];
  uvdb_set set;                                        /* to find the reader a compact piece comes from */
  char err[256]; int broken;
  unsigned long stage_calls, decode_calls;
};

#define ENGINE_BUG(c, ...) do { snprintf ((c)->err, sizeof (c)->err, __VA_ARGS__); (c)->broken = 1; return -1; } while (0)

const char *uvaia_gpu_last_error (const uvaia_gpu_ctx *c) { return c ? c->err : "no context"; }
int uvaia_gpu_db_side_row_ints (void) { return UVDB_SIDE_ROW_INTS; }
size_t uvaia_gpu_db_tile_bytes (const uvaia_gpu_ctx *c) { return c->tb; }
double uvaia_gpu_stage_unpack_ms (uvaia_gpu_ctx *c, int reset) { (void) reset; return (double) c->decode_calls; }

int
uvaia_gpu_db_stage_reserve (uvaia_gpu_ctx *c, size_t n_tiles)
{
  if (n_tiles < 1) ENGINE_BUG (c, "staging capacity of %zu tiles", n_tiles);
  if (n_tiles <= c->cap_tiles) return 0;
  for (int s = 0; s < 2; s++) {
    free (c->slot[s].planes);
    c->slot[s].planes = (uint32_t *) malloc (n_tiles * c->tb);     /* exactly what was asked for: the sanitizer sees a byte too far */
    memset (c->slot[s].planes, 0xFF, n_tiles * c->tb);
    c->slot[s].n_tiles = 0; c->slot[s].unread = 0;
  }
  c->cap_tiles = n_tiles;
  return 0;
}

static int
stage_begin (uvaia_gpu_ctx *c, int slot, size_t tile_offset, int n_tiles)
{
  if (slot < 0 || slot > 1 || n_tiles < 1) ENGINE_BUG (c, "stage: slot %d, %d tiles", slot, n_tiles);
  if (tile_offset + (size_t) n_tiles > c->cap_tiles) ENGINE_BUG (c, "%d tiles at tile %zu exceed the staging capacity of %zu", n_tiles, tile_offset, c->cap_tiles);
  if (!tile_offset) {
    if (c->slot[slot].unread) ENGINE_BUG (c, "slot %d is staged again before its rows were decoded", slot);
    memset (c->slot[slot].planes, 0xFF, c->cap_tiles * c->tb);     /* what no piece fills reads as all T-C-G-A sets, i.e. 'N' rows of the wrong text */
    c->slot[slot].n_tiles = 0;
  } else if (tile_offset != c->slot[slot].n_tiles) ENGINE_BUG (c, "a piece at tile %zu of slot %d, which is filled up to %zu", tile_offset, slot, c->slot[slot].n_tiles);
  c->slot[slot].n_tiles = tile_offset + (size_t) n_tiles;
  c->slot[slot].unread = 1;
  c->stage_calls++;
  return 0;
}

int
uvaia_gpu_db_stage_packed_at (uvaia_gpu_ctx *c, int slot, size_t tile_offset, const void *planes, const int *non_n, const int *side_rows, int n_tiles)
{
  if (!planes || !non_n || !side_rows) ENGINE_BUG (c, "NULL packed arrays");
  if (stage_begin (c, slot, tile_offset, n_tiles)) return -1;
  memcpy ((char *) c->slot[slot].planes + tile_offset * c->tb, planes, (size_t) n_tiles * c->tb);
  return 0;
}

int
uvaia_gpu_db_stage_compact_at (uvaia_gpu_ctx *c, int slot, size_t tile_offset, const void *base, const uint64_t *head_idx, const uint32_t *heads,
                               const uint64_t *lit_idx, const void *lits, const int *non_n, int n_tiles)
{
  (void) heads; (void) lits; (void) lit_idx;
  if (!base || !head_idx || !non_n) ENGINE_BUG (c, "NULL compact arrays");
  if (stage_begin (c, slot, tile_offset, n_tiles)) return -1;
  for (int f = 0; f < c->set->n_files; f++) if ((const void *) c->set->db[f]->base == base) {
    const uvdb_reader r = c->set->db[f];
    const uint64_t t0 = (uint64_t) (head_idx - r->head_idx) / 64;
    if ((uint64_t) (head_idx - r->head_idx) % 64 || t0 + (uint64_t) n_tiles > r->h.n_tiles) ENGINE_BUG (c, "a compact piece that is not whole tiles of its file");
    if (uvdb_expand_tiles (r, t0, (uint64_t) n_tiles, (char *) c->slot[slot].planes + tile_offset * c->tb, NULL)) ENGINE_BUG (c, "uvdb_expand_tiles");
    return 0;
  }
  ENGINE_BUG (c, "a compact piece of no file of the set");
}

int
uvaia_gpu_db_stage_unpack_rows (uvaia_gpu_ctx *c, int slot, const int *index, int n, char *rows, size_t pitch)
{
  if (slot < 0 || slot > 1 || n < 0 || pitch < (size_t) c->nchar) ENGINE_BUG (c, "unpack: slot %d, %d rows, pitch %zu", slot, n, pitch);
  if (!c->slot[slot].n_tiles) ENGINE_BUG (c, "slot %d holds no tiles", slot);
  for (int k = 0; k < n; k++) {
    if (index[k] < 0 || (size_t) index[k] >= c->slot[slot].n_tiles * 64) ENGINE_BUG (c, "index[%d] = %d outside the %zu tiles of slot %d", k, index[k], c->slot[slot].n_tiles, slot);
    const uint32_t *tile = c->slot[slot].planes + (size_t) (index[k] / 64) * (c->tb / 4);
    for (int s = 0; s < c->nchar; s++) {
      const uint32_t word = (uint32_t) s >> 5;
      const uint32_t *x = tile + ((size_t) (word >> 2) * 256 + (size_t) (index[k] % 64)) * 4 + (word & 3);
      uint32_t code = 0;
      for (int p = 0; p < 4; p++) code |= ((x[p * 256] >> (s & 31)) & 1u) << p;
      rows[(size_t) k * pitch + (size_t) s] = "NACMGRSVTWYHKDBN"[code];
    }
  }
  c->slot[slot].unread = 0;
  c->decode_calls++;
  return 0;
}

/* ---- files */
static char **all_seq; static char **all_name; static uint64_t n_all;

static int
write_file (const char *path, int nchar, int n_ref, int compact, const char *tag)
{
  const int W4 = ((nchar + 31) / 32 + 3) / 4, n_tiles = (n_ref + 63) / 64;
  const size_t tb = (size_t) W4 * 4 * 64 * 16;
  uint32_t *planes = (uint32_t *) calloc ((size_t) n_tiles, tb);
  int32_t *non_n = (int32_t *) calloc ((size_t) n_tiles * 64, sizeof (int32_t)), *side = (int32_t *) calloc ((size_t) n_tiles * 64 * UVDB_SIDE_ROW_INTS, sizeof (int32_t));
  uvdb_writer w = compact ? uvdb_create_compact (path, nchar, tb, UVDB_SIDE_ROW_INTS, 0.5) : uvdb_create (path, nchar, tb, UVDB_SIDE_ROW_INTS, 0.5);
  if (!w) FAIL ("cannot create %s", path);
  for (int i = 0; i < n_ref; i++) {
    char *seq = (char *) malloc ((size_t) nchar + 1), name[64];
    for (int s = 0; s < nchar; s++) seq[s] = "ACGT"[(s + (s >> 3)) & 3];
    seq[nchar] = '\0';
    for (int k = (int) (rnd () % 9); k > 0; k--) seq[rnd () % (uint32_t) nchar] = "ACGTRYKMSWBDHVN-?XO."[rnd () % 20];
    if (i % 3 == 1) for (int s = 0, e = (int) (rnd () % 40); s < e && s < nchar; s++) seq[s] = '-';       /* an exception run at site 0 */
    if (i % 5 == 2) for (int s = nchar - 1 - (int) (rnd () % 40); s < nchar; s++) if (s >= 0) seq[s] = '?';  /* and one at the last site */
    if (i % 11 == 7) memset (seq, i % 2 ? 'N' : '-', (size_t) nchar);
    snprintf (name, sizeof name, "%s%d", tag, i % 7 == 3 ? 3 : i);                                          /* some names are shared */
    for (int s = 0; s < nchar; s++) {
      const uint32_t c = code_of (seq[s]), word = (uint32_t) s >> 5;
      uint32_t *x = planes + (size_t) (i / 64) * (tb / 4) + ((size_t) (word >> 2) * 256 + (size_t) (i % 64)) * 4 + (word & 3);
      for (int p = 0; p < 4; p++) if ((c >> p) & 1u) x[p * 256] |= 1u << (s & 31);
      non_n[i] += c != 0;
    }
    if (uvdb_add_reference (w, name, seq)) FAIL ("add_reference");
    all_seq[n_all] = seq; all_name[n_all++] = strdup (name);
  }
  if (n_tiles && uvdb_add_tiles (w, (size_t) n_tiles, planes, non_n, compact ? NULL : side)) FAIL ("add_tiles");
  if (uvdb_close (w)) FAIL ("close %s", path);
  free (planes); free (non_n); free (side);
  return 0;
}

/* ---- the receiver */
typedef struct { const uint64_t *pos; uint64_t next, stop_at; int bad; } receiver;

static int
receive (void *user, uint64_t k, uint64_t stream, const char *name, const char *row)
{
  receiver *r = (receiver *) user;
  if (k != r->next++ || stream != (r->pos ? r->pos[k] : k) || strcmp (name, all_name[stream]) || strcmp (row, all_seq[stream])) r->bad++;
  return r->stop_at && r->next == r->stop_at;
}

static int
extract_and_compare (uvdb_set set, uvaia_gpu_ctx *gpu, const uint64_t *pos, uint64_t n, const char *what)
{
  char err[512];
  receiver r = {pos, 0, 0, 0};
  uvdb_extract_stats st;
  memset (&st, 0, sizeof st);
  if (uvdb_extract (set, gpu, pos, n, receive, &r, &st, err, sizeof err)) FAIL ("%s: %s", what, err);
  if (gpu->broken) FAIL ("%s: the engine's contract was broken: %s", what, gpu->err);
  if (r.next != n || r.bad || st.n_rows != n || st.n_chunks != (n + UVDB_EXTRACT_CHUNK - 1) / UVDB_EXTRACT_CHUNK) FAIL ("%s: %llu of %llu rows, %d wrong", what, (unsigned long long) r.next, (unsigned long long) n, r.bad);
  if (st.n_tiles > n || st.n_pieces > st.n_tiles) FAIL ("%s: %llu tiles in %llu pieces for %llu rows", what, (unsigned long long) st.n_tiles, (unsigned long long) st.n_pieces, (unsigned long long) n);
  printf ("%s: %llu rows exact; %llu chunks, %llu tiles in %llu pieces, slots of %zu tiles\n", what, (unsigned long long) n, (unsigned long long) st.n_chunks,
          (unsigned long long) st.n_tiles, (unsigned long long) st.n_pieces, gpu->cap_tiles);
  return 0;
}

static int
run (const char *scratch, int nchar, const int n_ref[3])
{
  char path[3][4096], err[512];
  const char *paths[3] = {path[0], path[1], path[2]};
  const uint64_t total = (uint64_t) n_ref[0] + (uint64_t) n_ref[1] + (uint64_t) n_ref[2];
  all_seq = (char **) calloc ((size_t) total + 1, sizeof (char *)); all_name = (char **) calloc ((size_t) total + 1, sizeof (char *)); n_all = 0;
  for (int f = 0; f < 3; f++) {
    snprintf (path[f], sizeof path[f], "%s.%d.uvdb", scratch, f);
    if (write_file (path[f], nchar, n_ref[f], f == 1, f == 0 ? "a" : f == 1 ? "b" : "c")) return 1;
  }
  uvdb_set set = uvdb_set_open (paths, 3, 0, err, sizeof err);
  if (!set) FAIL ("uvdb_set_open: %s", err);
  struct uvaia_gpu_ctx gpu;
  memset (&gpu, 0, sizeof gpu);
  gpu.nchar = nchar; gpu.tb = (size_t) set->tile_bytes; gpu.set = set;
  uint64_t *pos = (uint64_t *) malloc ((size_t) (total + 1) * sizeof (uint64_t)), n = 0;
  /* sparse first, while the slots are small: a slot never has to be larger than its chunk's tiles */
  for (uint64_t i = 0; i < total; i += 97) pos[n++] = i;
  if (n && extract_and_compare (set, &gpu, pos, n, "every 97th")) return 1;
  n = 0;
  if (total) { pos[n++] = 0; if (total > 1) pos[n++] = total - 1; }
  if (n && extract_and_compare (set, &gpu, pos, n, "first and last")) return 1;
  n = 0;
  for (uint64_t i = 0; i < total; i++) if (rnd () % 3) pos[n++] = i;
  if (n && extract_and_compare (set, &gpu, pos, n, "two of three")) return 1;
  if (total && extract_and_compare (set, &gpu, NULL, total, "the whole stream")) return 1;
  /* the last lane of every file and the first of the next */
  n = 0;
  for (int f = 1; f <= 3; f++) for (uint64_t x = set->first[f] ? set->first[f] - 1 : 0; x <= set->first[f] && x < total; x++) if (!n || pos[n - 1] < x) pos[n++] = x;   /* (a file may be empty) */
  if (n && extract_and_compare (set, &gpu, pos, n, "file edges")) return 1;
  /* refused without a row handed over: a repeat, a descent, a position outside; and a receiver that gives up ends the run */
  if (total > 2) {
    receiver r = {pos, 0, 0, 0};
    const uint64_t bad[3][2] = {{1, 1}, {2, 1}, {0, total}};
    for (int k = 0; k < 3; k++) { r.pos = bad[k]; r.next = 0; if (!uvdb_extract (set, &gpu, bad[k], 2, receive, &r, NULL, err, sizeof err) || r.next) FAIL ("bad positions %d were accepted", k); }
    receiver q = {NULL, 0, 2, 0};
    if (!uvdb_extract (set, &gpu, NULL, total, receive, &q, NULL, err, sizeof err) || q.next != 2) FAIL ("the receiver could not end the extraction");
    gpu.slot[0].unread = gpu.slot[1].unread = 0;       /* (the chunk staged ahead is never decoded then) */
  }
  if (gpu.broken) FAIL ("the engine's contract was broken: %s", gpu.err);
  /* the plan of a chunk, by hand: two positions in one tile, the two tiles behind it, and one beyond a tile nobody asked for */
  if (n_ref[0] >= 264) {
    const uint64_t p[5] = {3, 60, 64, 130, 263};
    uvdb_set_piece pc[5]; int np = 0, sel[5]; uint64_t st = 0;
    if (uvdb_extract_plan (set, p, 0, 5, pc, 5, &np, &st, sel) || np != 2 || st != 4 || pc[0].n_tiles != 3 || pc[1].first_tile != 4 || pc[1].slot_tile != 3 ||
        sel[0] != 3 || sel[1] != 60 || sel[2] != 64 || sel[3] != 130 || sel[4] != 3 * 64 + 7) FAIL ("the plan of a chunk");
    if (!uvdb_extract_plan (set, p, 0, 5, pc, 4, &np, &st, sel)) FAIL ("more positions than pieces were planned");
  }
  free (gpu.slot[0].planes); free (gpu.slot[1].planes); free (pos);
  uvdb_set_close (set);
  for (uint64_t i = 0; i < n_all; i++) { free (all_seq[i]); free (all_name[i]); }
  free (all_seq); free (all_name);
  for (int f = 0; f < 3; f++) remove (path[f]);
  return 0;
}

static int
names (void)
{
  static const char text[] = "zeta\r\n\nalpha\nname with spaces|2020\nalpha\nno-newline-at-the-end";
  uvdb_name_list l = uvdb_name_list_from_text (text, sizeof text - 1);
  if (!l || l->n != 4) FAIL ("name list: %zu names", l ? l->n : (size_t) 0);
  for (size_t k = 1; k < l->n; k++) if (strcmp (l->name[k - 1], l->name[k]) >= 0) FAIL ("name list not sorted");
  if (uvdb_name_list_find (l, "alpha") != 0 || uvdb_name_list_find (l, "alpha") != 0 || uvdb_name_list_find (l, "zeta") != 3 || uvdb_name_list_find (l, "zeta\r") != -1 ||
      uvdb_name_list_find (l, "") != -1 || uvdb_name_list_find (l, "no-newline-at-the-end") != 2 || uvdb_name_list_find (l, "alph") != -1) FAIL ("name list lookups");
  if (l->hits[0] != 2 || l->hits[1] != 0 || l->hits[2] != 1 || l->hits[3] != 1) FAIL ("name list hits");
  uvdb_name_list_free (l);
  const char *edge[] = {"", "\n", "\n\n\r\n", "x", "x\n"};
  for (size_t k = 0; k < sizeof edge / sizeof edge[0]; k++) {
    l = uvdb_name_list_from_text (edge[k], strlen (edge[k]));
    if (!l || l->n != (k >= 3 ? 1u : 0u) || uvdb_name_list_find (l, "y") != -1) FAIL ("name list of %zu bytes", strlen (edge[k]));
    uvdb_name_list_free (l);
  }
  printf ("name list: lookups, repeats, line ends exact\n");
  return 0;
}

int
main (int argc, char **argv)
{
  if (argc < 2) { fprintf (stderr, "usage: %s <scratch prefix>\n", argv[0]); return 2; }
  /* sites; references of the dense, the compact and the second dense file: one reference; file ends inside tiles; an empty file in the
     middle; more than one chunk in every file, a compact file of exactly four tiles */
  static const int shapes[][4] = {{29, 1, 0, 0}, {29, 1, 1, 1}, {130, 70, 130, 65}, {300, 64, 0, 63}, {1000, 300, 256, 600}, {70, 700, 513, 1}};
  for (size_t k = 0; k < sizeof shapes / sizeof shapes[0]; k++) if (run (argv[1], shapes[k][0], shapes[k] + 1)) return 1;
  return names ();
}
