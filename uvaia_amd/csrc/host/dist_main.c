/*
 * dist_main.c -- `uvaiadist`: the all-pairs distance matrix of an alignment, from packed databases (uvdb.h, dense or compact, several read as
 * one stream) or aligned FASTA.  No counterpart in the reference: its README sends users to snp-dists for this step ("uvaia reports
 * matches, not distances").  The counters of every pair are taken on the GPU over the bit planes the engine keeps resident
 * (uvaia_gpu_db_pairs, uvaia_gpu_db_pairs_within); this file loads the rows, asks for the matrix in bands of rows and writes a band as
 * text while the next is computed.  `-d D --clusters` asks for no pairs at all: the engine unites the pairs within D on the device
 * (uvaia_gpu_db_link_*) and hands back one label per sequence.  `--mst` and `--nearest` ask for none either: the engine keeps every
 * sequence's closest sequence of another component on the device (uvaia_gpu_db_near_*) and builds the minimum spanning tree around that
 * (uvaia_gpu_db_mst); N numbers come back.  Own code.
 *
 *   snp   = both ACGT and different (what snp-dists prints)        uvaia = valid_pair_comparisons - partial_matches (README, line 302)
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <libgen.h>
#include <limits.h>
#include <omp.h>
#include <pthread.h>

#include "cli_common.h"
#include "fastaseq.h"
#include "uvdb.h"
#include "uvdb_set.h"
#include "uvdb_extract.h"
#include "../../../include/uvaia_gpu.h"

#define LOAD_BATCH 4096            /* references per engine round trip (a multiple of 64) */
#define BAND_BYTES ((size_t) 256 << 20)
#define ROW_GROUP 64               /* rows formatted together, one per thread at a time, and written in order */
#define MAX_THREADS 16
#define LIST_CAP0 ((size_t) 1 << 20)

enum { FORM_DENSE = 0, FORM_LONG = 1, FORM_COUNTS = 2 };

static void
usage (const char *prog)
{
  printf ("%s \n", UVAIA_PACKAGE_STRING);
  printf ("All-pairs distance matrix of aligned sequences, counted on the GPU over the packed bit planes.\n\n");
  printf (" %s [-hv] [--metric=snp|uvaia] [--trim=<int>] [-A <double>] [--long | --counts] [-d <int>] [--csv]\n", prog);
  printf ("          [--clusters [--min-compared=<int>] [--min-size=<int>]] [--band-rows=<int>] [--device=<int>] (-o <file> | --stdout)\n");
  printf ("          [(--mst | --nearest) [--min-compared=<int>]]\n");
  printf ("          (--packed <db.uvdb> [--packed <db.uvdb>]... | <aln.fa(.gz,.xz)> [<aln.fa(.gz,.xz)>]...)\n\n");
  printf ("  --metric=snp|uvaia               snp (default): sites where both sequences are one of ACGT and differ, the number snp-dists prints;\n");
  printf ("                                   uvaia: valid_pair_comparisons - partial_matches, sites where both are valid and their IUPAC sets do not meet\n");
  printf ("  -t, --trim=<int>                 number of sites to trim from both ends (default=0)\n");
  printf ("  -A, --ref_ambiguity=<double>     maximum allowed ambiguity for a sequence to be kept (default=1: every sequence)\n");
  printf ("  --long                           one line `a,b,dist` per pair a before b, instead of the square table\n");
  printf ("  --counts                         one line per pair a before b with the five counters and the snp distance\n");
  printf ("  -d <int>                         only the pairs with distance <= <int> under --metric; implies --long unless --counts is given\n");
  printf ("  --clusters                       with -d: single-linkage clusters instead of pairs, one line `sequence<tab>cluster<tab>size` per sequence in\n");
  printf ("                                   input order; two sequences are linked when their distance is <= -d, a cluster is a connected set, clusters\n");
  printf ("                                   are numbered 1, 2, ... by their first member.  Under snp a sequence with no ACGT site is at distance 0 from\n");
  printf ("                                   every other and joins all clusters into one: set --min-compared against that\n");
  printf ("  --mst                            the minimum spanning tree instead of the table, one line `a<tab>b<tab>dist` per edge, sorted by distance, then by\n");
  printf ("                                   the input order of a (the earlier sequence of the two), then of b.  Ties between edges are decided by that same\n");
  printf ("                                   order, so the tree is unique; its edges up to a distance D join exactly the clusters of -d D --clusters\n");
  printf ("  --nearest                        every sequence's closest other sequence instead of the table, one line `sequence<tab>nearest<tab>dist` per sequence\n");
  printf ("                                   in input order; ties go to the earliest sequence; with no comparable partner the nearest is empty and dist -1\n");
  printf ("                                   Under snp a sequence with no ACGT site is at distance 0 from every other: it is the hub of the tree and\n");
  printf ("                                   everyone's nearest.  Set --min-compared against that (the tree may then be a forest)\n");
  printf ("  --min-compared=<int>             with --clusters: link only pairs compared over at least <int> sites (snp: both ACGT; uvaia: both valid; default=0)\n");
  printf ("                                   with --mst, --nearest: only such pairs are edges, or can be nearest\n");
  printf ("  --min-size=<int>                 with --clusters: leave out the sequences of clusters smaller than <int> (default=1; the numbering does not change)\n");
  printf ("  --csv                            commas instead of tabs in the square table and the cluster lines\n");
  printf ("  --band-rows=<int>                rows of the matrix computed at a time (default: what keeps a band near 256 MiB)\n");
  printf ("  -o, --output=<file>              file to write, compressed by its suffix (.xz, .bz2, .gz)\n");
  printf ("  --stdout                         uncompressed text on standard output instead of -o\n");
  printf ("  --packed=<db.uvdb>               packed database written by uvaiapack, uvaialign --packed, uvaiaclust --packed-out (may be repeated)\n");
  printf ("  --device=<int>                   GPU to use (default: current device)\n");
}

/* the engine needs some query to exist: a plain ACGT string of the alignment's length */
static uvaia_gpu_ctx *
open_engine (int nchar, int device)
{
  uvaia_gpu_ctx *gpu = NULL;
  char *dummy = (char *) biomcmc_malloc ((size_t) nchar + 1);
  for (int s = 0; s < nchar; s++) dummy[s] = "ACGT"[s & 3];
  dummy[nchar] = '\0';
  const char *one[1] = {dummy};
  uvaia_gpu_query q;
  memset (&q, 0, sizeof q);
  q.n_query = 1; q.nchar = nchar; q.seq = one; q.consensus = dummy;
  if (uvaia_gpu_open (&gpu, &q, 1, device, LOAD_BATCH)) biomcmc_error ("%s", uvaia_gpu_last_error (NULL));
  free (dummy);
  return gpu;
}

static void
reserve_or_refuse (uvaia_gpu_ctx *gpu, size_t n)
{
  const size_t need = n * uvaia_gpu_packed_bytes_per_ref (gpu), have = uvaia_gpu_free_bytes (gpu);
  if (need > have || uvaia_gpu_db_reserve (gpu, n))
    biomcmc_error ("%zu sequences need about %zu MiB of device memory, %zu MiB are free: the alignment must fit the device (%s)", n, need >> 20, have >> 20, uvaia_gpu_last_error (gpu));
}

typedef struct { char **name; size_t n, count; int nchar; double load_ms; } loaded_rows;

static double
now_ms (void)
{
  struct timespec ts;
  clock_gettime (CLOCK_MONOTONIC, &ts);
  return (double) ts.tv_sec * 1e3 + (double) ts.tv_nsec * 1e-6;
}

/* packed databases: the kept references of every file, chunk by chunk through the staging slots (as `uvaiapack --merge` appends them) */
static uvaia_gpu_ctx *
load_packed (int n_in, char **in, double ambig, int device, loaded_rows *rows)
{
  enum { CHUNK_TILES = LOAD_BATCH / 64 };
  char msg[1024];
  if (n_in > UVDB_SET_MAX_FILES) biomcmc_error ("at most %d packed databases", UVDB_SET_MAX_FILES);
  uvdb_set set = uvdb_set_open ((const char *const *) in, n_in, UVDB_SET_ANY_AMBIGUITY, msg, sizeof msg);
  if (!set) biomcmc_error ("%s", msg);
  const int nchar = (int) set->nchar, non_n_ref = (int) (nchar * (1. - ambig));
  uvaia_gpu_ctx *gpu = open_engine (nchar, device);
  if (set->tile_bytes != uvaia_gpu_db_tile_bytes (gpu) || set->side_row_ints != (uint32_t) uvaia_gpu_db_side_row_ints ()) biomcmc_error ("packed database %s does not match this engine's tile layout", in[0]);
  size_t kept = 0;
  for (int f = 0; f < n_in; f++) for (uint64_t r = 0; r < set->db[f]->h.n_ref; r++) kept += set->db[f]->non_n[r] >= non_n_ref;
  rows->name = (char **) biomcmc_malloc ((kept ? kept : 1) * sizeof (char *));
  rows->nchar = nchar;
  if (!kept) { uvdb_set_close (set); return gpu; }
  reserve_or_refuse (gpu, kept);
  if (uvaia_gpu_db_stage_reserve (gpu, CHUNK_TILES)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
  int *sel = (int *) biomcmc_malloc (LOAD_BATCH * sizeof (int));
  int slot = 0;
  for (int f = 0; f < n_in; f++) {
    uvdb_reader db = set->db[f];
    for (uint64_t t = 0; t < db->h.n_tiles; t += CHUNK_TILES) {
      const uint64_t nt = db->h.n_tiles - t < CHUNK_TILES ? db->h.n_tiles - t : CHUNK_TILES;
      const uint64_t r0 = t * 64, r1 = r0 + nt * 64 < db->h.n_ref ? r0 + nt * 64 : db->h.n_ref;
      int m = 0;
      for (uint64_t r = r0; r < r1; r++) {
        rows->count++;
        if (db->non_n[r] < non_n_ref) continue;
        rows->name[rows->n++] = strdup (uvdb_name (db, r));
        sel[m++] = (int) (r - r0);
      }
      if (!m) continue;
      const uvdb_set_piece piece = {f, t, nt, 0};
      if (uvdb_stage_pieces (gpu, set, slot, &piece, 1) ||
          uvaia_gpu_db_append_staged (gpu, slot, (uint64_t) m == r1 - r0 ? NULL : sel, m)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
      slot ^= 1;
    }
  }
  free (sel);
  uvdb_set_close (set);
  return gpu;
}

/* aligned FASTA through the host reader: the rows are held as text until their number is known (the database is reserved once) */
static uvaia_gpu_ctx *
load_fasta (int n_in, char **in, double ambig, int device, loaded_rows *rows)
{
  char **seq = NULL;
  int *non_n = NULL;
  size_t cap = 0;
  int nchar = 0, non_n_ref = 0;
  for (int j = 0; j < n_in; j++) {
    readfasta_t rfas = new_readfasta (in[j]);
    while (readfasta_next (rfas) >= 0) {
      rows->count++;
      if (!nchar) { nchar = (int) rfas->seqlength; non_n_ref = (int) (nchar * (1. - ambig)); }
      if (rfas->seqlength != (size_t) nchar) biomcmc_error ("sequence '%s' has %zu sites but the first sequence has %d sites: all sequences must be aligned", rfas->name, rfas->seqlength, nchar);
      const int nn = quick_count_sequence_non_N (rfas->seq, rfas->seqlength);
      if (nn < non_n_ref) continue;
      if (rows->n == cap) {
        cap = cap ? 2 * cap : 1024;
        seq = (char **) biomcmc_realloc (seq, cap * sizeof (char *));
        non_n = (int *) biomcmc_realloc (non_n, cap * sizeof (int));
        rows->name = (char **) biomcmc_realloc (rows->name, cap * sizeof (char *));
      }
      rows->name[rows->n] = strdup (rfas->name);
      non_n[rows->n] = nn;
      seq[rows->n++] = rfas->seq; rfas->seq = NULL;
    }
    del_readfasta (rfas);
  }
  if (!nchar) biomcmc_error ("no sequence found");
  rows->nchar = nchar;
  uvaia_gpu_ctx *gpu = open_engine (nchar, device);
  if (rows->n) reserve_or_refuse (gpu, rows->n);
  for (size_t a = 0; a < rows->n; a += LOAD_BATCH) {
    const int m = (int) (rows->n - a < LOAD_BATCH ? rows->n - a : LOAD_BATCH);
    if (uvaia_gpu_db_append (gpu, (const char *const *) seq + a, non_n + a, m)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    for (int c = 0; c < m; c++) free (seq[a + c]);
  }
  free (seq); free (non_n);
  return gpu;
}

/* ---- the writer: text assembled in memory by own integer formatting, handed to the output in order */
typedef struct { char *p; size_t n, cap; } textbuf;

static inline void
text_room (textbuf *t, size_t more)
{
  if (t->n + more + 1 <= t->cap) return;
  while (t->n + more + 1 > t->cap) t->cap = t->cap ? 2 * t->cap : 1 << 16;
  t->p = (char *) biomcmc_realloc (t->p, t->cap);
}

static inline void
text_bytes (textbuf *t, const char *s, size_t len) { memcpy (t->p + t->n, s, len); t->n += len; }      /* (room was made) */

static inline void
text_int (textbuf *t, int v)
{ /* at most 11 characters; room was made */
  char tmp[12];
  int k = 0;
  unsigned u = v < 0 ? 0u - (unsigned) v : (unsigned) v;
  do { tmp[k++] = (char) ('0' + u % 10); u /= 10; } while (u);
  if (v < 0) t->p[t->n++] = '-';
  while (k) t->p[t->n++] = tmp[--k];
}

typedef struct { file_compress_t fc; double write_ms; } sink;

static void
sink_write (sink *s, textbuf *t)
{
  if (!t->n) return;
  const double t0 = now_ms ();
  size_t done = s->fc ? fwrite (t->p, 1, t->n, s->fc->fp) : fwrite (t->p, 1, t->n, stdout);
  if (done != t->n) biomcmc_error ("problem writing the output");
  s->write_ms += now_ms () - t0;
  t->n = 0;
}

typedef struct {
  uvaia_gpu_ctx *gpu;
  size_t n, trim, r0, nr;
  int what;
  int32_t *out;
  int rc;
} band_job;

static void *
band_compute (void *arg)
{
  band_job *b = (band_job *) arg;
  b->rc = uvaia_gpu_db_pairs (b->gpu, b->r0, b->nr, 0, b->n, b->trim, b->what, b->out, b->n);
  return NULL;
}

static inline int
pair_dist (const int32_t *c, int metric) { return metric == UVAIA_GPU_DIST_SNP ? c[4] - c[0] : c[3] - c[2]; }

/* one row of a band as text: the table's line, or the long / counts lines of the pairs (row, j > row) */
static void
format_row (textbuf *t, const loaded_rows *rows, const size_t *name_len, size_t total_names, size_t i, const int32_t *band_row, int per, int form, int metric, char sep)
{
  const size_t n = rows->n;
  t->n = 0;
  if (form == FORM_DENSE) {
    text_room (t, name_len[i] + n * 12 + 2);
    text_bytes (t, rows->name[i], name_len[i]);
    for (size_t j = 0; j < n; j++) { t->p[t->n++] = sep; text_int (t, per == 1 ? band_row[j] : pair_dist (band_row + j * 5, metric)); }
    t->p[t->n++] = '\n';
    return;
  }
  text_room (t, (n - i) * (name_len[i] + 2 + (form == FORM_COUNTS ? 6 * 12 : 12) + 1) + total_names);
  for (size_t j = i + 1; j < n; j++) {
    text_bytes (t, rows->name[i], name_len[i]); t->p[t->n++] = ',';
    text_bytes (t, rows->name[j], name_len[j]); t->p[t->n++] = ',';
    if (form == FORM_LONG) text_int (t, per == 1 ? band_row[j] : pair_dist (band_row + j * 5, metric));
    else {
      const int32_t *c = band_row + j * 5;
      for (int k = 0; k < 5; k++) { text_int (t, c[k]); t->p[t->n++] = ','; }
      text_int (t, c[4] - c[0]);
    }
    t->p[t->n++] = '\n';
  }
}

int
main (int argc, char **argv)
{
  double ambig = 1.;
  const char *out = NULL, *metric_name = "snp";
  char **packed = (char **) biomcmc_malloc ((size_t) (argc + 1) * sizeof (char *));
  int n_packed = 0, device = -1, ch, errors = 0, want_long = 0, want_counts = 0, want_dense = 0, have_d = 0, max_dist = 0, csv = 0, to_stdout = 0, want_clusters = 0, have_min_compared = 0, have_min_size = 0, want_mst = 0, want_nearest = 0;
  long trim = 0, band_rows = 0, min_compared = 0, min_size = 1;
  size_t list_cap = LIST_CAP0;
  static const struct option longopts[] = {{"help", no_argument, 0, 'h'}, {"version", no_argument, 0, 'v'}, {"ref_ambiguity", required_argument, 0, 'A'},
    {"output", required_argument, 0, 'o'}, {"trim", required_argument, 0, 't'}, {"metric", required_argument, 0, 1001}, {"device", required_argument, 0, 1002},
    {"long", no_argument, 0, 1003}, {"counts", no_argument, 0, 1004}, {"csv", no_argument, 0, 1005}, {"band-rows", required_argument, 0, 1006},
    {"stdout", no_argument, 0, 1007}, {"packed", required_argument, 0, 1008}, {"list-cap", required_argument, 0, 1009}, {"dense", no_argument, 0, 1010},
    {"clusters", no_argument, 0, 1011}, {"min-compared", required_argument, 0, 1012}, {"min-size", required_argument, 0, 1013},
    {"mst", no_argument, 0, 1014}, {"nearest", no_argument, 0, 1015}, {0, 0, 0, 0}};
  while ((ch = getopt_long (argc, argv, "hvA:o:t:d:", longopts, NULL)) != -1) switch (ch) {
    case 'h': usage (basename (argv[0])); return EXIT_SUCCESS;
    case 'v': printf ("%s\n", UVAIA_PACKAGE_VERSION); return EXIT_SUCCESS;
    case 'A': ambig = atof (optarg); break;
    case 'o': out = optarg; break;
    case 't': trim = atol (optarg); break;
    case 'd': have_d = 1; max_dist = atoi (optarg); break;
    case 1001: metric_name = optarg; break;
    case 1002: device = atoi (optarg); break;
    case 1003: want_long = 1; break;
    case 1004: want_counts = 1; break;
    case 1005: csv = 1; break;
    case 1006: band_rows = atol (optarg); break;
    case 1007: to_stdout = 1; break;
    case 1008: packed[n_packed++] = optarg; break;
    case 1009: list_cap = (size_t) strtoull (optarg, NULL, 10); break;      /* (for tests: the first capacity of the -d list, so that it has to grow) */
    case 1010: want_dense = 1; break;                                       /* the default form, spelled out */
    case 1011: want_clusters = 1; break;
    case 1012: have_min_compared = 1; min_compared = atol (optarg); break;
    case 1013: have_min_size = 1; min_size = atol (optarg); break;
    case 1014: want_mst = 1; break;
    case 1015: want_nearest = 1; break;
    default: errors++;
  }
  /* what does not go together is refused here, before a file is opened or a GPU touched */
  int metric = 0;
  if (!strcmp (metric_name, "snp")) metric = UVAIA_GPU_DIST_SNP;
  else if (!strcmp (metric_name, "uvaia")) metric = UVAIA_GPU_DIST_UVAIA;
  else { fprintf (stderr, "unknown metric '%s': --metric takes snp or uvaia\n", metric_name); return EXIT_FAILURE; }
  if (want_mst && want_nearest) { fprintf (stderr, "--mst and --nearest are two forms of the output: give one\n"); return EXIT_FAILURE; }
  if (want_mst || want_nearest) {
    const char *me = want_mst ? "--mst" : "--nearest", *writes = want_mst ? "one line per edge of the tree" : "one line per sequence";
    if (have_d) { fprintf (stderr, "%s does not go with -d: it looks at every pair, whatever its distance\n", me); return EXIT_FAILURE; }
    if (want_clusters) { fprintf (stderr, "%s does not go with --clusters: it writes %s, not clusters\n", me, writes); return EXIT_FAILURE; }
    if (want_long) { fprintf (stderr, "%s does not go with --long: it writes %s, not per pair\n", me, writes); return EXIT_FAILURE; }
    if (want_counts) { fprintf (stderr, "%s does not go with --counts: it writes %s, not per pair\n", me, writes); return EXIT_FAILURE; }
    if (want_dense) { fprintf (stderr, "%s does not go with --dense: it writes %s, not a table\n", me, writes); return EXIT_FAILURE; }
    if (have_min_size) { fprintf (stderr, "%s does not go with --min-size: there are no clusters to leave out\n", me); return EXIT_FAILURE; }
  }
  if (want_long && want_counts) { fprintf (stderr, "--long and --counts are two forms of the output: give one\n"); return EXIT_FAILURE; }
  if (want_dense && (want_long || want_counts)) { fprintf (stderr, "--dense does not go with --long or --counts\n"); return EXIT_FAILURE; }
  if (want_clusters && want_long) { fprintf (stderr, "--clusters does not go with --long: it writes one line per sequence, not per pair\n"); return EXIT_FAILURE; }
  if (want_clusters && want_counts) { fprintf (stderr, "--clusters does not go with --counts: it writes one line per sequence, not per pair\n"); return EXIT_FAILURE; }
  if (want_clusters && want_dense) { fprintf (stderr, "--clusters does not go with --dense: it writes one line per sequence, not a table\n"); return EXIT_FAILURE; }
  if (have_d && want_dense) { fprintf (stderr, "-d needs a long form (--long or --counts): a square table has a cell for every pair\n"); return EXIT_FAILURE; }
  if (have_d && max_dist < 0) { fprintf (stderr, "-d takes a distance of 0 or more\n"); return EXIT_FAILURE; }
  if (want_clusters && !have_d) { fprintf (stderr, "--clusters needs -d: clusters are the sequences connected by pairs within a distance\n"); return EXIT_FAILURE; }
  const int want_tree = want_mst || want_nearest;
  if (have_min_compared && !want_clusters && !want_tree) { fprintf (stderr, "--min-compared needs --clusters: it decides which pairs link two sequences\n"); return EXIT_FAILURE; }
  if (have_min_size && !want_clusters) { fprintf (stderr, "--min-size needs --clusters: it leaves out the sequences of small clusters\n"); return EXIT_FAILURE; }
  if (min_compared < 0 || min_compared > INT_MAX) { fprintf (stderr, "--min-compared takes a number of 0 or more\n"); return EXIT_FAILURE; }
  if (min_size < 0) { fprintf (stderr, "--min-size takes a number of 0 or more\n"); return EXIT_FAILURE; }
  if (n_packed && optind < argc) { fprintf (stderr, "packed databases and FASTA files cannot be mixed: give --packed files or alignments\n"); return EXIT_FAILURE; }
  if (!errors && !out && !to_stdout) { fprintf (stderr, "where to write: give -o <file> or --stdout\n"); return EXIT_FAILURE; }
  if (out && to_stdout) { fprintf (stderr, "both -o and --stdout were given: the output goes to one place\n"); return EXIT_FAILURE; }
  if (trim < 0 || band_rows < 0) { fprintf (stderr, "--trim and --band-rows take numbers of 0 or more\n"); return EXIT_FAILURE; }
  if (errors || (!n_packed && optind >= argc)) { printf ("Error when reading arguments from command line:\n"); usage (basename (argv[0])); return EXIT_FAILURE; }
  if (ambig < 0.001) ambig = 0.001;
  if (ambig > 1.) ambig = 1.;
  const int form = want_counts ? FORM_COUNTS : (want_long || have_d || want_tree) ? FORM_LONG : FORM_DENSE;      /* (--mst, --nearest: no header) */
  if (omp_get_max_threads () > MAX_THREADS) omp_set_num_threads (MAX_THREADS);

  int64_t time0[2];
  biomcmc_get_time (time0);
  loaded_rows rows;
  memset (&rows, 0, sizeof rows);
  double t0 = now_ms ();
  uvaia_gpu_ctx *gpu = n_packed ? load_packed (n_packed, packed, ambig, device, &rows) : load_fasta (argc - optind, argv + optind, ambig, device, &rows);
  rows.load_ms = now_ms () - t0;
  const size_t n = rows.n;
  if (2 * (size_t) trim > (size_t) rows.nchar) biomcmc_error ("--trim %ld on both sides leaves nothing of %d sites", trim, rows.nchar);

  size_t *name_len = (size_t *) biomcmc_malloc ((n ? n : 1) * sizeof (size_t)), total_names = 0;
  for (size_t i = 0; i < n; i++) { name_len[i] = strlen (rows.name[i]); total_names += name_len[i]; }
  sink snk = {out ? biomcmc_open_compress (out, "w") : NULL, 0.};
  const char sep = csv ? ',' : '\t';
  double format_ms = 0.;
  unsigned long long n_pairs = 0;
  size_t n_bands = 0;
  textbuf head = {NULL, 0, 0};
  if (form == FORM_DENSE) {
    text_room (&head, 16 + total_names + n + 2);
    text_bytes (&head, "uvaiadist", 9);
    for (size_t j = 0; j < n; j++) { head.p[head.n++] = sep; text_bytes (&head, rows.name[j], name_len[j]); }
    head.p[head.n++] = '\n';
  } else if (form == FORM_COUNTS) {
    static const char *h = "a,b,ACGT_matches,text_matches,partial_matches,valid_pair_comparisons,ACGT_pair_comparisons,snp_distance\n";
    text_room (&head, strlen (h));
    text_bytes (&head, h, strlen (h));
  }
  sink_write (&snk, &head);

  unsigned long long n_links = 0, tiles[2] = {0, 0};
  size_t n_clusters = 0, largest = 0, n_edges = 0;
  long long weight = 0;
  int n_rounds = 0;
  if (want_mst && n) {
    /* the tree: the engine's rounds hand back at most n - 1 edges, sorted as they are written */
    uvaia_gpu_edge *edge = (uvaia_gpu_edge *) biomcmc_malloc (n * sizeof (uvaia_gpu_edge));
    if (uvaia_gpu_db_mst (gpu, (size_t) trim, metric, (int) min_compared, edge, &n_edges, &n_rounds)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    uvaia_gpu_near_tiles (gpu, tiles, 0);
    t0 = now_ms ();
    textbuf t = {NULL, 0, 0};
    for (size_t k = 0; k < n_edges; k++) {
      const uvaia_gpu_edge *e = edge + k;
      if (e->a >= e->b || e->b >= n) biomcmc_error ("the engine handed back the edge %u - %u of %zu sequences", e->a, e->b, n);
      weight += e->dist;
      text_room (&t, name_len[e->a] + name_len[e->b] + 2 * 12);
      text_bytes (&t, rows.name[e->a], name_len[e->a]); t.p[t.n++] = sep;
      text_bytes (&t, rows.name[e->b], name_len[e->b]); t.p[t.n++] = sep;
      text_int (&t, e->dist); t.p[t.n++] = '\n';
      if (t.n > ((size_t) 1 << 24)) { format_ms += now_ms () - t0; sink_write (&snk, &t); t0 = now_ms (); }
    }
    format_ms += now_ms () - t0;
    sink_write (&snk, &t);
    free (t.p); free (edge);
  } else if (want_nearest && n) {
    /* one pass with every sequence a component of its own: a band of rows against all columns at a time, the keys come back once */
    const size_t band = band_rows ? (size_t) band_rows : 4096;
    if (uvaia_gpu_db_near_begin (gpu, (size_t) trim, metric, (int) min_compared)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    for (size_t r0 = 0; r0 < n; r0 += band, n_bands++)
      if (uvaia_gpu_db_near (gpu, r0, n - r0 < band ? n - r0 : band, 0, n, tiles)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    n_rounds = 1;
    uint64_t *best = (uint64_t *) biomcmc_malloc (n * sizeof (uint64_t));
    if (uvaia_gpu_db_near_fetch (gpu, best)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    t0 = now_ms ();
    textbuf t = {NULL, 0, 0};
    for (size_t i = 0; i < n; i++) {
      const int none = best[i] == UVAIA_GPU_NEAR_NONE;
      const size_t y = none ? 0 : (size_t) (best[i] & 0xFFFFFFFFu);
      if (!none && (y >= n || y == i)) biomcmc_error ("the engine named sequence %zu as the nearest of sequence %zu of %zu", y, i, n);
      if (!none) { n_edges++; weight += (long long) (best[i] >> 32); }
      text_room (&t, name_len[i] + (none ? 0 : name_len[y]) + 2 * 12);
      text_bytes (&t, rows.name[i], name_len[i]); t.p[t.n++] = sep;
      if (!none) text_bytes (&t, rows.name[y], name_len[y]);
      t.p[t.n++] = sep;
      text_int (&t, none ? -1 : (int) (best[i] >> 32)); t.p[t.n++] = '\n';
      if (t.n > ((size_t) 1 << 24)) { format_ms += now_ms () - t0; sink_write (&snk, &t); t0 = now_ms (); }
    }
    format_ms += now_ms () - t0;
    sink_write (&snk, &t);
    free (t.p); free (best);
  } else if (want_clusters && n) {
    /* clusters: a band of rows against all columns is linked on the device, nothing but the count of links comes back per band; the labels
     * (smallest member of every sequence's cluster) come back once, and are numbered here by first member */
    const size_t band = band_rows ? (size_t) band_rows : 4096;
    if (uvaia_gpu_db_link_begin (gpu, (size_t) trim, metric, max_dist, (int) min_compared)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    for (size_t r0 = 0; r0 < n; r0 += band, n_bands++)
      if (uvaia_gpu_db_link (gpu, r0, n - r0 < band ? n - r0 : band, 0, n, &n_links)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    uint32_t *label = (uint32_t *) biomcmc_malloc (n * sizeof (uint32_t));
    if (uvaia_gpu_db_link_labels (gpu, label)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    t0 = now_ms ();
    size_t *size = (size_t *) biomcmc_malloc (n * sizeof (size_t)), *number = (size_t *) biomcmc_malloc (n * sizeof (size_t));
    for (size_t i = 0; i < n; i++) size[i] = 0;
    for (size_t i = 0; i < n; i++) {
      if (label[i] > i) biomcmc_error ("the engine labelled sequence %zu with the later sequence %u", i, label[i]);
      if (label[i] == i) number[i] = ++n_clusters;      /* a cluster's label is its first member: numbered in that order */
      size[label[i]]++;
    }
    textbuf t = {NULL, 0, 0};
    for (size_t i = 0; i < n; i++) {
      const size_t sz = size[label[i]];
      if (sz > largest) largest = sz;
      if (sz < (size_t) min_size) continue;
      text_room (&t, name_len[i] + 2 * 24);
      text_bytes (&t, rows.name[i], name_len[i]); t.p[t.n++] = sep;
      text_int (&t, (int) number[label[i]]); t.p[t.n++] = sep;
      text_int (&t, (int) sz); t.p[t.n++] = '\n';
      if (t.n > ((size_t) 1 << 24)) { format_ms += now_ms () - t0; sink_write (&snk, &t); t0 = now_ms (); }
    }
    format_ms += now_ms () - t0;
    sink_write (&snk, &t);
    free (t.p); free (label); free (size); free (number);
  } else if (have_d && n) {
    /* the pairs within the distance: a band of rows against everything behind the diagonal; the list grows until a band fits */
    const size_t band = band_rows ? (size_t) band_rows : 4096;
    uvaia_gpu_pair *list = (uvaia_gpu_pair *) biomcmc_malloc ((list_cap ? list_cap : 1) * sizeof (uvaia_gpu_pair));
    textbuf t = {NULL, 0, 0};
    for (size_t r0 = 0; r0 < n; r0 += band, n_bands++) {
      const size_t nr = n - r0 < band ? n - r0 : band;
      unsigned long long found = 0;
      for (;;) {
        if (uvaia_gpu_db_pairs_within (gpu, r0, nr, 0, n, (size_t) trim, metric, max_dist, 1, list, list_cap, &found)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
        if (found <= list_cap) break;
        list_cap = (size_t) found;
        list = (uvaia_gpu_pair *) biomcmc_realloc (list, list_cap * sizeof (uvaia_gpu_pair));
      }
      n_pairs += found;
      t0 = now_ms ();
      for (unsigned long long k = 0; k < found; k++) {
        const uvaia_gpu_pair *p = list + k;
        text_room (&t, name_len[p->row] + name_len[p->col] + 8 * 12);
        text_bytes (&t, rows.name[p->row], name_len[p->row]); t.p[t.n++] = ',';
        text_bytes (&t, rows.name[p->col], name_len[p->col]); t.p[t.n++] = ',';
        if (form == FORM_LONG) text_int (&t, pair_dist (p->count, metric));
        else { for (int c = 0; c < 5; c++) { text_int (&t, p->count[c]); t.p[t.n++] = ','; } text_int (&t, p->count[4] - p->count[0]); }
        t.p[t.n++] = '\n';
        if (t.n > ((size_t) 1 << 24)) { format_ms += now_ms () - t0; sink_write (&snk, &t); t0 = now_ms (); }
      }
      format_ms += now_ms () - t0;
      sink_write (&snk, &t);
    }
    free (list); free (t.p);
  } else if (n) {
    /* every pair: two host buffers, a band is turned into text and written while the device counts the next one */
    const int per = (form == FORM_COUNTS || metric == UVAIA_GPU_DIST_UVAIA) ? UVAIA_GPU_PAIR_NCOUNT : 1;
    const int what = per == 1 ? UVAIA_GPU_PAIRS_SNP : UVAIA_GPU_PAIRS_COUNTS;
    size_t band = band_rows ? (size_t) band_rows : BAND_BYTES / (n * (size_t) per * sizeof (int32_t));
    if (band < 1) band = 1;
    if (band > n) band = n;
    const size_t band_bytes = band * n * (size_t) per * sizeof (int32_t);
    int32_t *buf[2];
    int pinned[2];
    for (int k = 0; k < 2; k++) {
      buf[k] = (int32_t *) uvaia_gpu_fasta_pinned_alloc (band_bytes);
      pinned[k] = buf[k] != NULL;
      if (!buf[k]) buf[k] = (int32_t *) biomcmc_malloc (band_bytes);
    }
    textbuf group[ROW_GROUP];
    memset (group, 0, sizeof group);
    band_job job[2];
    pthread_t th;
    n_bands = (n + band - 1) / band;
    for (size_t b = 0; b <= n_bands; b++) {
      int running = 0;
      if (b < n_bands) {
        band_job *j = job + (b & 1);
        j->gpu = gpu; j->n = n; j->trim = (size_t) trim; j->r0 = b * band; j->nr = n - j->r0 < band ? n - j->r0 : band; j->what = what; j->out = buf[b & 1]; j->rc = 0;
        if (pthread_create (&th, NULL, band_compute, j)) biomcmc_error ("cannot start the thread that drives the device");
        running = 1;
      }
      if (b > 0) {       /* band b - 1 is complete: rows in groups, a thread per row, written in order */
        const band_job *j = job + ((b - 1) & 1);
        for (size_t g = 0; g < j->nr; g += ROW_GROUP) {
          const size_t m = j->nr - g < ROW_GROUP ? j->nr - g : ROW_GROUP;
          t0 = now_ms ();
#pragma omp parallel for schedule(dynamic, 1)
          for (size_t k = 0; k < m; k++)
            format_row (group + k, &rows, name_len, total_names, j->r0 + g + k, j->out + (g + k) * n * (size_t) per, per, form, metric, sep);
          format_ms += now_ms () - t0;
          for (size_t k = 0; k < m; k++) sink_write (&snk, group + k);
        }
      }
      if (running) {
        pthread_join (th, NULL);
        if (job[b & 1].rc) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
      }
    }
    n_pairs = form == FORM_DENSE ? (unsigned long long) n * n : (unsigned long long) n * (n - 1) / 2;
    for (int k = 0; k < ROW_GROUP; k++) free (group[k].p);
    for (int k = 0; k < 2; k++) { if (pinned[k]) uvaia_gpu_fasta_pinned_free (buf[k]); else free (buf[k]); }
  }
  double t_close = now_ms ();
  if (snk.fc) biomcmc_close_compress (snk.fc);
  else if (fflush (stdout)) biomcmc_error ("problem writing to standard output");
  snk.write_ms += now_ms () - t_close;

  double ms[3] = {0., 0., 0.};
  uvaia_gpu_pairs_ms (gpu, ms, 0);
  fprintf (stderr, want_mst ? "Wrote the %s minimum spanning tree of %zu of %zu sequences (%d sites, trim %ld) to %s in %.3lf secs.\n"
                 : want_nearest ? "Wrote the %s nearest sequence of %zu of %zu sequences (%d sites, trim %ld) to %s in %.3lf secs.\n"
                 : want_clusters ? "Wrote the %s clusters of %zu of %zu sequences (%d sites, trim %ld) to %s in %.3lf secs.\n"
                                 : "Wrote the %s distances of %zu of %zu sequences (%d sites, trim %ld) to %s in %.3lf secs.\n", metric_name, n, rows.count, rows.nchar, trim,
           out ? out : "standard output", biomcmc_update_elapsed_time (time0));
  if (want_mst) {
    double near_ms = 0.;
    uvaia_gpu_near_ms (gpu, &near_ms, 0);
    fprintf (stderr, "dist report: {\"sequences\": %zu, \"edges\": %zu, \"trees\": %zu, \"rounds\": %d, \"weight\": %lld, \"tiles_walked\": %llu, \"tiles_skipped\": %llu, \"load_ms\": %.3f, \"kernel_ms\": %.3f, \"format_ms\": %.3f, \"write_ms\": %.3f}\n",
             n, n_edges, n - n_edges, n_rounds, weight, tiles[0], tiles[1], rows.load_ms, ms[0] + near_ms, format_ms, snk.write_ms);
  } else if (want_nearest) {
    double near_ms = 0.;
    uvaia_gpu_near_ms (gpu, &near_ms, 0);
    fprintf (stderr, "dist report: {\"sequences\": %zu, \"nearest\": %zu, \"rounds\": %d, \"weight\": %lld, \"tiles_walked\": %llu, \"tiles_skipped\": %llu, \"bands\": %zu, \"load_ms\": %.3f, \"kernel_ms\": %.3f, \"format_ms\": %.3f, \"write_ms\": %.3f}\n",
             n, n_edges, n_rounds, weight, tiles[0], tiles[1], n_bands, rows.load_ms, ms[0] + near_ms, format_ms, snk.write_ms);
  } else if (want_clusters) {
    double link_ms = 0.;
    uvaia_gpu_link_ms (gpu, &link_ms, 0);
    fprintf (stderr, "dist report: {\"sequences\": %zu, \"links\": %llu, \"clusters\": %zu, \"largest\": %zu, \"bands\": %zu, \"load_ms\": %.3f, \"kernel_ms\": %.3f, \"format_ms\": %.3f, \"write_ms\": %.3f}\n",
             n, n_links, n_clusters, largest, n_bands, rows.load_ms, ms[0] + link_ms, format_ms, snk.write_ms);
  } else
    fprintf (stderr, "dist report: {\"sequences\": %zu, \"pairs\": %llu, \"bands\": %zu, \"load_ms\": %.3f, \"kernel_ms\": %.3f, \"format_ms\": %.3f, \"write_ms\": %.3f}\n",
             n, n_pairs, n_bands, rows.load_ms, ms[0] + ms[1] + ms[2], format_ms, snk.write_ms);
  uvaia_gpu_close (gpu);
  for (size_t i = 0; i < n; i++) free (rows.name[i]);
  free (rows.name); free (name_len); free (head.p); free (packed);
  return EXIT_SUCCESS;
}
