/*
 * cluster_main.c -- `uvaiaclust`: one-pass canopy deduplication of aligned sequences.  Same options, queue assignment and output
 * files as the reference's src/cluster.c; phase 2 and the merge tree run on the GPU through include/uvaia_cluster.h, whose header
 * states what is computed.  The partial saves of src/cluster.c:197-199,228-229 (their timing decides them) are not made: only the
 * final <prefix>.csv.xz and <prefix>.aln.xz are written.
 *
 * --packed and --packed-out (no counterpart in the reference): the sequences come from a packed database (uvdb.h) whose tiles and
 * exception runs go to the device as they lie in the file's mapping, and the medoids leave as a packed database written from the rows in
 * device memory (uvdb_packer.h), the file `uvaiapack` makes of <prefix>.aln.xz.  No sequence text is held on the host on that path: the
 * medoids of <prefix>.aln.xz are fetched from the device in batches.  Own code.
 *
 * --keep-medoids (no counterpart in the reference): the clusterer keeps the rows of the sequences that found a cluster only
 * (uvaia_clust_keep_medoids), so device memory follows the number of clusters and not the number of sequences; same output files.  With
 * --packed it is chosen without being asked for when the file's sequence count says that the row store could not grow to hold them
 * (clust_plan.h).  Own code.
 *
 * --device-parse (no counterpart either, off by default): the alignment files are read in blocks (fasta_blocks.h), split into records and
 * rows on the GPU (uvaia_gpu_fasta_scan, uvaia_gpu_fasta_rows) and pushed from the parser's device memory (uvaia_clust_push_device).  Only
 * the names stay on the host; the medoids of <prefix>.aln.xz come back from the device in batches, as with --packed.  Same output files.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <libgen.h>
#include <omp.h>

#include "cli_common.h"
#include "fastaseq.h"
#include "uvdb.h"
#include "uvdb_packer.h"
#include "uvdb_set.h"
#include "clust_plan.h"
#include "fasta_blocks.h"
#include "../../../include/uvaia_cluster.h"

/* read_reference_sequence (src/cluster.c:260-277): the first record of the file, filled by up to nseqs - 1 more while Ns remain
   (accumulate_reference_sequence, src/fastaseq.c:488-512), remaining Ns replaced by A (src/fastaseq.c:514-520) */
/* one more record s into the reference in the making (*ref NULL: the first); returns the sites that are still N */
static int
accumulate_reference (char **ref, const char *s, int len)
{
  int count = 0;
  if (!*ref) {
    *ref = (char *) biomcmc_malloc ((size_t) len + 1);
    for (int k = 0; k < len; k++) {
      (*ref)[k] = s[k];
      if (s[k] != 'A' && s[k] != 'C' && s[k] != 'G' && s[k] != 'T') { (*ref)[k] = 'N'; count++; }
    }
    (*ref)[len] = '\0';
  } else for (int k = 0; k < len; k++) if ((*ref)[k] == 'N') {
    if (s[k] == 'A' || s[k] == 'C' || s[k] == 'G' || s[k] == 'T') (*ref)[k] = s[k];
    else count++;
  }
  return count;
}

static void
finish_reference (char *ref, int len)
{
  int count = 0;
  for (int k = 0; k < len; k++) if (ref[k] == 'N') { ref[k] = 'A'; count++; }
  if (count) fprintf (stderr, "Reference still had %d Ns or indels which were replaced arbitrarily (it only makes program a bit slower).", count);
}

static char *
read_reference (const char *filename, int nseqs, int *nchar)
{
  char *ref = NULL;
  int count = 0xff, len = -1;
  readfasta_t rfas = new_readfasta (filename);
  fprintf (stderr, "Generating a reference from up to %d sequences in %s\n", nseqs, filename);
  for (int i = 0; i < nseqs && count && readfasta_next (rfas) > 0; i++) {
    if (len < 0) len = (int) rfas->seqlength;
    else if (len != (int) rfas->seqlength) biomcmc_error ("Unaligned sequences: first seq has %d sites but %s has %lu sites\n", len, rfas->name, (unsigned long) rfas->seqlength);
    count = accumulate_reference (&ref, rfas->seq, len);
  }
  del_readfasta (rfas);
  if (!ref) biomcmc_error ("No sequence found in %s to build a reference from", filename);
  finish_reference (ref, len);
  *nchar = len;
  return ref;
}

/* the same rule over the records of a packed database: their exact text, one at a time, from uvdb_unpack_reference */
static char *
read_reference_packed (uvdb_reader db, const char *filename, int nseqs)
{
  char *ref = NULL;
  int count = 0xff;
  const int len = (int) db->h.nchar;
  char *text = (char *) biomcmc_malloc ((size_t) len + 1);
  fprintf (stderr, "Generating a reference from up to %d sequences in %s\n", nseqs, filename);
  for (uint64_t i = 0; i < (uint64_t) nseqs && count && i < db->h.n_ref; i++) {
    uvdb_unpack_reference (db, i, text);
    count = accumulate_reference (&ref, text, len);
  }
  free (text);
  if (!ref) biomcmc_error ("No sequence found in %s to build a reference from", filename);
  finish_reference (ref, len);
  return ref;
}

typedef struct { char **v; int64_t n, cap; } str_vec;

static void
str_vec_push (str_vec *s, char *x)
{
  if (s->n == s->cap) { s->cap = s->cap ? 2 * s->cap : 4096; s->v = (char **) biomcmc_realloc (s->v, (size_t) s->cap * sizeof (char *)); }
  s->v[s->n++] = x;
}

typedef struct { int device, nchar, dist, trim, snps, n_clust; char *refseq; uvaia_clust_ctx *ctx; int keep_medoids; } gpu_state;

/* the context is opened at the first push: errors in the input found by then are reported as such, GPU or not */
static void
open_context (gpu_state *g)
{
  if (g->ctx) return;
  if (uvaia_clust_open (&g->ctx, g->device, g->refseq, g->nchar, g->dist, g->trim, g->snps, g->n_clust)) biomcmc_error ("%s", uvaia_clust_last_error (NULL));
  if (g->keep_medoids && uvaia_clust_keep_medoids (g->ctx, 0)) biomcmc_error ("%s", uvaia_clust_last_error (g->ctx));
}

static void
push_batch (gpu_state *g, str_vec *seqs, int64_t from, int *queue, int n)
{
  if (!n) return;
  open_context (g);
  if (uvaia_clust_push (g->ctx, n, (const char *const *) seqs->v + from, queue)) biomcmc_error ("%s", uvaia_clust_last_error (g->ctx));
}

#define PACKED_CHUNK 4096    /* sequences of a packed database per push: whole tiles (a multiple of 64); a tuning value, the result does not depend on it */
#define ROWS_BATCH 256       /* medoids fetched from the device per round trip for <prefix>.aln.xz */

static void
packer_report (const struct uvdb_packer *pk, const char *path, int n_out, int nchar, long kept, long dropped)
{
  fprintf (stderr, "Packed %ld of %d medoids (%d sites) into %s; %ld too ambiguous. Device time: census %.3lf ms, gather %.3lf ms, exception runs %.3lf ms.\n",
           kept, n_out, nchar, path, dropped, pk->rows_ms[0], pk->rows_ms[1], pk->rows_ms[2]);
  if (pk->compact) fprintf (stderr, "Compact tiles: %ld encoded on the device (count and prefix %.3lf ms, emit %.3lf ms), %ld on the host.\n", pk->tiles_device, pk->encode_ms[0], pk->encode_ms[1], pk->tiles_host);
}

/* --packed-out with --keep-medoids: there is no row store to read in place, so each batch of medoids, in the final order, is gathered into
   consecutive rows of device memory (uvaia_clust_gather_device) and goes to the packer as a block: census, filter and append as below */
static void
write_packed_out_gathered (const char *path, uvaia_clust_ctx *ctx, int device, int nchar, double ambig_r, int compact, const int64_t *medoid, int n_out,
                           const char *(*name_of) (void *, int64_t), void *name_arg)
{
  struct uvdb_packer pk;
  if (uvdb_packer_open (&pk, path, nchar, ambig_r, device, UVDB_PACK_BATCH, compact)) biomcmc_error ("%s", pk.err);
  char **name = (char **) biomcmc_malloc (UVDB_PACK_BATCH * sizeof (char *));
  for (int a = 0; a < n_out; a += UVDB_PACK_BATCH) {
    const int m = n_out - a < UVDB_PACK_BATCH ? n_out - a : UVDB_PACK_BATCH;
    const void *d_rows = NULL; size_t pitch = 0;
    if (uvaia_clust_gather_device (ctx, medoid + a, m, &d_rows, &pitch)) { uvdb_packer_close (&pk); biomcmc_error ("%s", uvaia_clust_last_error (ctx)); }
    for (int k = 0; k < m; k++) name[k] = (char *) name_of (name_arg, medoid[a + k]);
    if (uvdb_packer_add_block (&pk, d_rows, pitch, m, name)) {
      char msg[640];
      snprintf (msg, sizeof msg, "%s", pk.err);
      uvdb_packer_close (&pk);
      biomcmc_error ("%s: %s", path, msg);
    }
  }
  const long kept = pk.kept, dropped = pk.dropped;
  if (uvdb_packer_close (&pk)) biomcmc_error ("%s", pk.err);
  packer_report (&pk, path, n_out, nchar, kept, dropped);
  free (name);
}

/* --packed-out: the medoids in their final order into a packed database, from the rows in the clusterer's device memory */
static void
write_packed_out (const char *path, uvaia_clust_ctx *ctx, int device, int nchar, double ambig_r, int compact, int64_t count, const int64_t *medoid, int n_out,
                  const char *(*name_of) (void *, int64_t), void *name_arg)
{
  const void *d_rows = NULL; size_t pitch = 0;
  if (uvaia_clust_device_rows (ctx, &d_rows, &pitch)) biomcmc_error ("%s", uvaia_clust_last_error (ctx));
  struct uvdb_packer pk;
  if (uvdb_packer_open (&pk, path, nchar, ambig_r, device, UVDB_PACK_BATCH, compact)) biomcmc_error ("%s", pk.err);
  /* the census takes consecutive rows: the whole store in blocks, the counts of the medoids are kept */
  int *slot = (int *) biomcmc_malloc ((size_t) (count + 1) * sizeof (int));
  int *m_nn = (int *) biomcmc_malloc ((size_t) (n_out + 1) * sizeof (int)), *m_exc = (int *) biomcmc_malloc ((size_t) (n_out + 1) * sizeof (int));
  for (int64_t i = 0; i < count; i++) slot[i] = -1;
  for (int c = 0; c < n_out; c++) slot[medoid[c]] = c;
  int *nn = (int *) biomcmc_malloc (UVDB_PACK_BATCH * sizeof (int)), *ne = (int *) biomcmc_malloc (UVDB_PACK_BATCH * sizeof (int)), *row = (int *) biomcmc_malloc (UVDB_PACK_BATCH * sizeof (int));
  char **name = (char **) biomcmc_malloc (UVDB_PACK_BATCH * sizeof (char *));
  for (int64_t a = 0; a < count && n_out; a += UVDB_PACK_BATCH) {
    const int m = (int) (count - a < UVDB_PACK_BATCH ? count - a : UVDB_PACK_BATCH);
    if (uvaia_gpu_rows_census (pk.gpu, (const char *) d_rows + (size_t) a * pitch, pitch, m, nn, ne)) {
      char msg[640];
      snprintf (msg, sizeof msg, "%s", uvaia_gpu_last_error (pk.gpu));
      uvdb_packer_close (&pk);
      biomcmc_error ("%s: %s", path, msg);
    }
    for (int k = 0; k < m; k++) if (slot[a + k] >= 0) { m_nn[slot[a + k]] = nn[k]; m_exc[slot[a + k]] = ne[k]; }
  }
  for (int a = 0; a < n_out; a += UVDB_PACK_BATCH) {
    const int m = n_out - a < UVDB_PACK_BATCH ? n_out - a : UVDB_PACK_BATCH;
    for (int k = 0; k < m; k++) { row[k] = (int) medoid[a + k]; name[k] = (char *) name_of (name_arg, medoid[a + k]); }
    if (uvdb_packer_add_rows (&pk, d_rows, pitch, row, m_nn + a, m_exc + a, name, m)) {
      char msg[640];
      snprintf (msg, sizeof msg, "%s", pk.err);
      uvdb_packer_close (&pk);
      biomcmc_error ("%s: %s", path, msg);
    }
  }
  const long kept = pk.kept, dropped = pk.dropped;
  if (uvdb_packer_close (&pk)) biomcmc_error ("%s", pk.err);
  packer_report (&pk, path, n_out, nchar, kept, dropped);
  free (slot); free (m_nn); free (m_exc); free (nn); free (ne); free (row); free (name);
}

/* `uvaiaclust --device-parse`: every record of a scan is a row (a record of another length ends the command, as on the default route), so the
 * rows of a scan are one push, sequence k of the FILE to queue k mod Q. */
#define PARSE_MAX_RECORDS (1 << 18)     /* records per scan, as in pack_main.c; a block that holds more is scanned in several steps */

struct clust_parse {
  gpu_state *g;
  uvaia_gpu_fasta *fasta;
  int max_records;
  uvaia_gpu_fasta_record *rec;          /* max_records of each */
  int *queue;
  str_vec *names;
  int64_t count, k;                     /* sequences pushed so far; of the file being read */
};

static int
clust_parse_scan (void *user, const char *text, size_t n, int final, int *n_records, size_t *consumed, int *bad_kind, size_t *bad_off, char *err, size_t errlen)
{
  struct clust_parse *d = (struct clust_parse *) user;
  if (!uvaia_gpu_fasta_scan (d->fasta, text, n, final, n_records, consumed)) return 0;
  const unsigned kind = uvaia_gpu_fasta_bad (d->fasta, bad_off);       /* irregular text: the block reader names the byte of the stream */
  *bad_kind = kind == UVAIA_GPU_FASTA_NUL ? FASTA_BAD_NUL : kind == UVAIA_GPU_FASTA_TEXT ? FASTA_BAD_TEXT : kind == UVAIA_GPU_FASTA_EMPTY ? FASTA_BAD_EMPTY : FASTA_BAD_NONE;
  snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta));
  return -1;
}

/* a push refused for a byte >= 0x80: the message of the default route, from the parser's rows */
static void
clust_parse_bad_byte (struct clust_parse *d, int n_rows, size_t pitch, int64_t first, char *err, size_t errlen)
{
  const int nchar = d->g->nchar;
  unsigned char *rows = (unsigned char *) biomcmc_malloc ((size_t) n_rows * pitch);
  if (!uvaia_gpu_fasta_rows_host (d->fasta, rows)) for (int r = 0; r < n_rows; r++) for (int i = 0; i < nchar; i++) if (rows[(size_t) r * pitch + i] >= 0x80) {
    snprintf (err, errlen, "sequence %s holds byte 0x%02x at site %d: only bytes 1-127 are defined", d->names->v[first + r], rows[(size_t) r * pitch + i], i + 1);
    free (rows);
    return;
  }
  free (rows);
}

static int
clust_parse_records (void *user, char *text, size_t consumed, int n_records, char *err, size_t errlen)
{
  struct clust_parse *d = (struct clust_parse *) user;
  gpu_state *g = d->g;
  const void *d_rows = NULL; size_t pitch = 0; int n_rows = 0;
  if (uvaia_gpu_fasta_records (d->fasta, d->rec)) { snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta)); return -1; }
  const int64_t first = d->count;
  for (int k = 0; k < n_records; k++) {
    const uvaia_gpu_fasta_record *r = d->rec + k;
    char *name = text + r->name_off;
    name[r->name_len] = '\0';                         /* the line end behind the name, or the byte of room behind the block */
    if ((int64_t) r->seq_len != g->nchar) {
      snprintf (err, errlen, "%s cannot work with unaligned sequences; sequence %s has %lu sites while reference has %d.", UVAIA_PACKAGE_STRING, name, (unsigned long) r->seq_len, g->nchar);
      return -1;
    }
    str_vec_push (d->names, strdup (name));           /* the block buffer is recycled */
    d->queue[k] = (int) (d->k++ % g->n_clust);
  }
  if (uvaia_gpu_fasta_rows (d->fasta, g->nchar, &d_rows, &pitch, &n_rows, NULL)) { snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta)); return -1; }
  open_context (g);
  const int rc = uvaia_clust_push_device (g->ctx, n_rows, d_rows, pitch, NULL, d->queue);
  if (rc) {
    snprintf (err, errlen, "%s", uvaia_clust_last_error (g->ctx));
    if (rc == UVAIA_GPU_EALPHABET) clust_parse_bad_byte (d, n_rows, pitch, first, err, errlen);
    return -1;
  }
  d->count += n_rows;
  return 0;
}

/* all files through the route above; returns the number of sequences pushed */
static int64_t
cluster_device_parse (gpu_state *g, const char **fasta, int n_fasta, size_t block_bytes, str_vec *names, int64_t *time0)
{
  char msg[1024], failed[1024];
  struct clust_parse d;
  memset (&d, 0, sizeof d);
  d.g = g; d.names = names;
  d.max_records = block_bytes / 4 + 1 < PARSE_MAX_RECORDS ? (int) (block_bytes / 4 + 1) : PARSE_MAX_RECORDS;      /* (a record has four bytes at least) */
  if (uvaia_gpu_fasta_open (&d.fasta, g->device, block_bytes, d.max_records)) biomcmc_error ("%s", uvaia_gpu_fasta_last_error (NULL));
  d.rec = (uvaia_gpu_fasta_record *) biomcmc_malloc ((size_t) d.max_records * sizeof (uvaia_gpu_fasta_record));
  d.queue = (int *) biomcmc_malloc ((size_t) d.max_records * sizeof (int));
  uint64_t bytes = 0;
  for (int j = 0; j < n_fasta; j++) {
    uint64_t nb = 0;
    d.k = 0;                                            /* sequence k of a file to queue k mod Q (src/cluster.c:164-181) */
    fasta_blocks fb = fasta_blocks_open (fasta[j], block_bytes, uvaia_gpu_fasta_pinned_alloc, uvaia_gpu_fasta_pinned_free, msg, sizeof msg);
    const int rc = fb ? fasta_blocks_run (fb, d.max_records, clust_parse_scan, &d, clust_parse_records, &d, &nb, msg, sizeof msg) : -1;
    if (fasta_blocks_finish (fb, failed, sizeof failed)) biomcmc_error ("%s", failed);      /* a decompressor that failed mid-stream: that is the finding */
    if (rc) {
      const int text = strstr (msg, "FASTA text:") || strstr (msg, "does not fit a block");     /* what the parser refuses, the line reader takes */
      biomcmc_error ("%s%s", msg, text ? " (--device-parse takes regular FASTA whose records fit a block: `uvaiaclust` without it reads this file line by line)" : "");
    }
    bytes += nb;
    fprintf (stderr, "Finished reading file %s in %.3lf secs; Commulative %ld sequences read\n", fasta[j], biomcmc_update_elapsed_time (time0), (long) d.count);
  }
  double ms[2] = {0., 0.}, rows_in_ms = 0.;
  uvaia_gpu_fasta_kernel_ms (d.fasta, ms, 0);
  if (g->ctx) uvaia_clust_push_device_ms (g->ctx, &rows_in_ms);
  fprintf (stderr, "device parse: {\"bytes\": %llu, \"block_bytes\": %zu, \"scan_ms\": %.3f, \"rows_ms\": %.3f, \"rows_in_ms\": %.3f}\n", (unsigned long long) bytes, block_bytes, ms[0], ms[1], rows_in_ms);
  uvaia_gpu_fasta_close (d.fasta);
  free (d.rec); free (d.queue);
  return d.count;
}

static const char *name_from_vec (void *v, int64_t i) { return ((str_vec *) v)->v[i]; }
static const char *name_from_db (void *v, int64_t i) { return uvdb_set_name ((uvdb_set) v, (uint64_t) i); }      /* i: position in the stream of all --packed files */

int
main (int argc, char **argv)
{
  int help = 0, version = 0, dist = 1, trim = 0, snps = 1, pool = 4 * omp_get_max_threads (), device = 0, errors = 0, keep_medoids = 0, compact = 0, device_parse = 0, ch;   /* src/cluster.c:57-64 */
  size_t parse_block = FASTA_BLOCK_BYTES;
  double ambig_r = -1.;
  const char *out = "cluster_uvaia", *ref_file = NULL, *packed = NULL, *packed_out = NULL;
  const char **packed_files = (const char **) biomcmc_malloc ((size_t) argc * sizeof (char *)); int n_packed = 0;
  static const struct option longopts[] = {
    {"help", no_argument, 0, 'h'}, {"version", no_argument, 0, 'v'}, {"distance", required_argument, 0, 'd'}, {"trim", required_argument, 0, 1000},
    {"pool", required_argument, 0, 'p'}, {"snps", required_argument, 0, 's'}, {"reference", required_argument, 0, 'r'},
    {"output", required_argument, 0, 'o'}, {"device", required_argument, 0, 1001}, {"packed", required_argument, 0, 1002},
    {"packed-out", required_argument, 0, 1003}, {"ref_ambiguity", required_argument, 0, 'A'}, {"keep-medoids", no_argument, 0, 1004}, {"compact", no_argument, 0, 1005},
    {"device-parse", no_argument, 0, 1006}, {"parse-block", required_argument, 0, 1007}, {0, 0, 0, 0}};
  while ((ch = getopt_long (argc, argv, "hvd:p:s:r:o:A:", longopts, NULL)) != -1) switch (ch) {
    case 'h': help = 1; break;
    case 'v': version = 1; break;
    case 'd': dist = atoi (optarg); break;
    case 1000: trim = atoi (optarg); break;
    case 'p': pool = atoi (optarg); break;
    case 's': snps = atoi (optarg); break;
    case 'r': if (ref_file) errors++; ref_file = optarg; break;
    case 'o': out = optarg; break;
    case 1001: device = atoi (optarg); break;
    case 1002: if (!packed) packed = optarg; packed_files[n_packed++] = optarg; break;
    case 1003: if (packed_out) errors++; packed_out = optarg; break;
    case 1004: keep_medoids = 1; break;
    case 1005: compact = 1; break;
    case 1006: device_parse = 1; break;
    case 1007: parse_block = (size_t) strtoull (optarg, NULL, 10); break;      /* (for tests: the block size of --device-parse in bytes) */
    case 'A': ambig_r = atof (optarg); if (ambig_r < 0.) ambig_r = 0.; break;
    default: errors++;
  }
  const char **fasta = (const char **) argv + optind;
  const int n_fasta = argc - optind;
  if (version) { printf ("%s\n", UVAIA_PACKAGE_VERSION); return EXIT_SUCCESS; }
  /* --device-parse: what does not go with it is refused here, before a file is opened or a GPU touched */
  if (!help && device_parse && packed) { fprintf (stderr, "--device-parse reads FASTA text: it does not go with --packed, which holds no text to parse\n"); return EXIT_FAILURE; }
  if (!help && device_parse && (parse_block < 64 || parse_block > ((size_t) 1 << 30))) { fprintf (stderr, "--parse-block: expected 64 to 1073741824 bytes\n"); return EXIT_FAILURE; }
  if (!help && !device_parse && parse_block != FASTA_BLOCK_BYTES) { fprintf (stderr, "--parse-block sets the block size of --device-parse: it needs that option\n"); return EXIT_FAILURE; }
  if (!help && !errors && packed && n_fasta > 0) {
    fprintf (stderr, "--packed %s takes the place of the alignment files: give one or the other, not both (%s was given as well)\n", packed, fasta[0]);
    errors++;
  }
  if (!help && !errors && compact && !packed_out) {
    fprintf (stderr, "--compact chooses the form of the packed database of medoids: it needs --packed-out <out.uvdb>\n");
    errors++;
  }
  if (help || errors || (!packed && n_fasta < 1) || n_fasta > 1024 || n_packed > UVDB_SET_MAX_FILES) {
    printf ("%s \nCluster and dedups alignments\nThe complete syntax is:\n\n", UVAIA_PACKAGE_STRING);
    printf (" %s [-hv] [-d <int>] [--trim=<int>] [-p <int>] [-s <int>] [-r <ref.fa(.gz,.xz)>] [--packed-out <out.uvdb> [--compact]] [-A <double>] [--keep-medoids] [--device-parse] [-o <without suffix>] <seqs.fa(.gz,.xz)> [<seqs.fa(.gz,.xz)>]... | --packed <in.uvdb> [--packed <in.uvdb>]...\n\n", basename (argv[0]));
    printf ("  -h, --help                       print a longer help and exit\n  -v, --version                    print version and exit\n");
    printf ("  -d, --distance=<int>             seqs with this SNP differences or less will be merged (default=1)\n");
    printf ("  --trim=<int>                     number of sites to trim from both ends (default=0, suggested for sarscov2=230)\n");
    printf ("  -p, --pool=<int>                 Pool size, i.e. number of clustering queues (should be larger than avail threads)\n");
    printf ("  -s, --snps=<int>                 how many SNPs w.r.t. reference it keeps track (default=1, should be small number)\n");
    printf ("  -r, --reference=<ref.fa(.gz,.xz)> reference sequence (medoids are furthest from it)\n");
    printf ("  <seqs.fa(.gz,.xz)>               alignments to merge\n");
    printf ("  -o, --output=<without suffix>    prefix of xzipped output alignment and cluster table files\n");
    printf ("  --device=<int>                   GPU to use (default 0)\n");
    printf ("  --packed=<in.uvdb>               cluster the sequences of a packed database (`uvaiapack`, `uvaialign --packed`) instead of alignment files:\n");
    printf ("                                   its tiles are decoded on the GPU, no text is parsed or held; same output files as from the same sequences as text;\n");
    printf ("                                   can be several files, clustered in the order given like several alignment files\n");
    printf ("  --packed-out=<out.uvdb>          also write the medoids as a packed database, the file `uvaiapack` makes of <prefix>.aln.xz (with either kind of input)\n");
    printf ("  --compact                        with --packed-out: write the compact form of that database, the file `uvaiapack --compact` makes of <prefix>.aln.xz\n");
    printf ("                                   (several times smaller; encoded on the GPU once its base row is fixed, after 4096 medoids)\n");
    printf ("  -A, --ref_ambiguity=<double>     with --packed-out: maximum allowed ambiguity for a medoid to be kept in that database, as in `uvaiapack`\n");
    printf ("                                   (default: the value recorded in the --packed database, 0.5 for alignment files)\n");
    printf ("  --keep-medoids                   keep only the sequences that found a cluster in GPU memory, not every sequence: memory follows the number of\n");
    printf ("                                   clusters; same output files (with --packed: chosen by itself when the sequences would not fit otherwise)\n");
    printf ("  --device-parse                   split the alignment files into sequences on the GPU instead of reading them line by line, and cluster them where\n");
    printf ("                                   they lie: no sequence text is held on the host (only names).  Same output files, from regular FASTA only (a NUL\n");
    printf ("                                   byte, text before the first header and a header without sequence are refused).  Not with --packed.  Behind .gz or\n");
    printf ("                                   .xz the decompressor sets the pace and little time is gained; the memory is saved all the same\n");
    printf ("  --parse-block=<bytes>            with --device-parse: the text is read in blocks of this size (64 to 1073741824, default 67108864); a record\n");
    printf ("                                   must fit a block\n");
    if (help) {
      printf ("One-pass clustering similar to canopy clustering with single, tight distance, computed on the GPU.\n");
      printf ("A pool of independent clustering queues is created, such that each sequence is compared to only one of them at first.\n\n");
    }
    return (help && !errors) ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  for (int f = 0; f < n_packed; f++) if (uvdb_file_version (packed_files[f]) == 2) {     /* the clustering decodes dense tiles from the mapping */
    fprintf (stderr, "uvaiaclust --packed: %s is a compact packed database (`uvaiapack --compact`), which the clustering does not read; convert it with `uvaiapack --merge -o dense.uvdb %s`\n", packed_files[f], packed_files[f]);
    return EXIT_FAILURE;
  }
  if (dist < 0) dist = 0;                                                  /* src/cluster.c:131-132 */
  if (snps < 0) snps = 0;
  fprintf (stderr, "Experimental program: %s package: %s\n", basename (argv[0]), UVAIA_PACKAGE_STRING);
  int n_clust = omp_get_max_threads ();                                    /* src/cluster.c:136-142 */
  if (pool >= n_clust) n_clust = pool;
  int64_t time0[2];
  biomcmc_get_time (time0);

  uvdb_reader db = NULL;          /* the first --packed file: the reference sequence comes from it, as from the first alignment file */
  uvdb_set set = NULL;            /* all of them, one stream */
  if (packed) {   /* a damaged file is refused here, before any GPU work */
    char msg[1024] = "";
    set = uvdb_set_open (packed_files, n_packed, UVDB_SET_ANY_AMBIGUITY, msg, sizeof msg);      /* (the filter of the inputs does not matter to the clustering) */
    if (!set) biomcmc_error ("%s", msg);
    db = set->db[0];
    if (db->h.nchar > 0x3fffffff) biomcmc_error ("%s: sequences of %u sites are too long", packed, db->h.nchar);
  }
  if (ambig_r < 0.) ambig_r = set ? set->ref_ambiguity : 0.5;
  if (ambig_r < 0.001) ambig_r = 0.001;                                    /* pack_main.c:46-47 */
  if (ambig_r > 1.) ambig_r = 1.;

  int nchar = 0;
  char *refseq = NULL;
  if (ref_file) refseq = read_reference (ref_file, 1, &nchar);
  else if (db) { refseq = read_reference_packed (db, packed, 1024); nchar = (int) db->h.nchar; }
  else refseq = read_reference (fasta[0], 1024, &nchar);
  if (compact && nchar > UVDB_COMPACT_MAX_NCHAR) biomcmc_error ("--compact: alignments of more than %d sites have no compact form (%d sites)", UVDB_COMPACT_MAX_NCHAR, nchar);
  if (db && (uint32_t) nchar != db->h.nchar)
    biomcmc_error ("%s cannot work with unaligned sequences; the sequences of %s have %u sites while reference has %d.", UVAIA_PACKAGE_STRING, packed, db->h.nchar, nchar);
  if (trim < 0) trim = 0;                                                  /* new_cqueue, src/cluster.c:287-289 */
  if (trim > nchar / 2.1) trim = (int) (nchar / 2.1);
  if (dist > nchar / 10) dist = nchar / 10;
  fprintf (stderr, "Creating a pool of %d cluster queues; maximum distance is %d, and %d SNP locations are kept\n", n_clust, dist, snps);
  gpu_state g = {device, nchar, dist, trim, snps, n_clust, refseq, NULL, keep_medoids};

  str_vec names = {0}, seqs = {0};
  int64_t count = 0;
  if (db) {
    /* sequence k of the database to queue k mod Q; chunks of whole tiles go to the device from the file's mapping as they are */
    int *queue = (int *) biomcmc_malloc (PACKED_CHUNK * sizeof (int));
    open_context (&g);
    if (!keep_medoids) {   /* the file says how many sequences come: would the store of every row reach that count in the memory there is? */
      size_t free_bytes = 0;
      const uint64_t row_bytes = ((uint64_t) nchar + 63) / 64 * 64;
      uint64_t peak = 0;
      if (uvaia_clust_memory (g.ctx, NULL, NULL, &free_bytes)) free_bytes = 0;   /* unknown: as without the option */
      uvclust_store_peak (set->n_ref, PACKED_CHUNK, row_bytes, &peak);
      if (uvclust_choose_keep_medoids (set->n_ref, PACKED_CHUNK, row_bytes, (uint64_t) free_bytes) == 1) {
        fprintf (stderr, "Keeping medoid rows only (as with --keep-medoids): the rows of the %llu sequences of %s would need %llu bytes of GPU memory while their store grows, %zu are free\n",
                 (unsigned long long) set->n_ref, n_packed > 1 ? "the --packed files" : packed, (unsigned long long) peak, free_bytes);
        if (uvaia_clust_keep_medoids (g.ctx, 0)) biomcmc_error ("%s", uvaia_clust_last_error (g.ctx));
        keep_medoids = g.keep_medoids = 1;
      }
    }
    /* file after file, sequence k of a FILE to queue k mod Q as for alignment files below; the result does not depend on how the
       sequences are cut into pushes (include/uvaia_cluster.h) */
    for (int f = 0; f < n_packed; f++) {
      uvdb_reader fd = set->db[f];
      for (uint64_t first = 0; first < fd->h.n_ref; first += PACKED_CHUNK) {
        const int n = (int) (fd->h.n_ref - first < PACKED_CHUNK ? fd->h.n_ref - first : PACKED_CHUNK);
        for (int i = 0; i < n; i++) queue[i] = (int) ((first + (uint64_t) i) % (uint64_t) n_clust);
        if (uvaia_clust_push_packed (g.ctx, n, uvdb_tile_planes (fd, first / 64), fd->exc_idx + first, fd->exc, queue)) biomcmc_error ("%s: %s", packed_files[f], uvaia_clust_last_error (g.ctx));
        count += n;
      }
      fprintf (stderr, "Finished reading file %s in %.3lf secs; Commulative %ld sequences read\n", packed_files[f], biomcmc_update_elapsed_time (time0), (long) count);
    }
    free (queue);
  } else if (device_parse) count = cluster_device_parse (&g, fasta, n_fasta, parse_block, &names, time0);
  else {
    /* read every file, sequence k of a file to queue k mod Q (src/cluster.c:164-181); push in batches of 4 Q */
    const int batch = 4 * n_clust;
    int *queue = (int *) biomcmc_malloc ((size_t) batch * sizeof (int));
    for (int j = 0; j < n_fasta; j++) {
      readfasta_t rfas = new_readfasta (fasta[j]);
      int64_t k = 0, from = seqs.n;
      int fill = 0;
      while (readfasta_next (rfas) >= 0) {
        if ((int64_t) rfas->seqlength != nchar)
          biomcmc_error ("%s cannot work with unaligned sequences; sequence %s has %lu sites while reference has %d.", UVAIA_PACKAGE_STRING, rfas->name ? rfas->name : "(unnamed)", (unsigned long) rfas->seqlength, nchar);
        for (int i = 0; i < nchar; i++) if ((unsigned char) rfas->seq[i] >= 0x80)   /* they index the reference's site tables out of range */
          biomcmc_error ("sequence %s holds byte 0x%02x at site %d: only bytes 1-127 are defined", rfas->name ? rfas->name : "(unnamed)", (unsigned char) rfas->seq[i], i + 1);
        str_vec_push (&seqs, rfas->seq); rfas->seq = NULL; rfas->seqlength = 0;
        str_vec_push (&names, rfas->name); rfas->name = NULL;
        queue[fill++] = (int) (k++ % n_clust);
        count++;
        if (fill == batch) { push_batch (&g, &seqs, from, queue, fill); from += fill; fill = 0; }
      }
      push_batch (&g, &seqs, from, queue, fill);
      del_readfasta (rfas);
      fprintf (stderr, "Finished reading file %s in %.3lf secs; Commulative %ld sequences read\n", fasta[j], biomcmc_update_elapsed_time (time0), (long) count);
    }
    free (queue);
  }
  open_context (&g);
  free (refseq);
  uvaia_clust_ctx *ctx = g.ctx;
  if (uvaia_clust_finish (ctx)) biomcmc_error ("%s", uvaia_clust_last_error (ctx));
  int n_out = 0;
  uvaia_clust_result (ctx, &n_out, NULL, NULL, NULL, NULL);
  int64_t *medoid = (int64_t *) biomcmc_malloc ((size_t) (n_out + 1) * sizeof (int64_t)), *offsets = (int64_t *) biomcmc_malloc ((size_t) (n_out + 1) * sizeof (int64_t));
  int64_t *members = (int64_t *) biomcmc_malloc ((size_t) (count - n_out + 1) * sizeof (int64_t));
  if (uvaia_clust_result (ctx, &n_out, medoid, offsets, members, NULL)) biomcmc_error ("%s", uvaia_clust_last_error (ctx));
  double prep_ms = 0, queue_ms = 0, merge_ms = 0, decode_ms = 0, overlay_ms = 0;
  uvaia_clust_stats (ctx, &prep_ms, &queue_ms, &merge_ms, NULL);
  uvaia_clust_unpack_ms (ctx, &decode_ms, &overlay_ms);
  size_t peak_row_bytes = 0;
  uvaia_clust_memory (ctx, NULL, &peak_row_bytes, NULL);
  const char *(*name_of) (void *, int64_t) = db ? name_from_db : name_from_vec;
  void *name_arg = db ? (void *) set : (void *) &names;

  /* save_neighbours_to_xz_file and save_cluster_to_xz_file (src/fastaseq.c:293-392) for the final order */
  size_t outlength = 0;
  char *outfilename = outfile_from_prefix (out, &outlength);
  strcpy (outfilename + outlength, ".csv.xz");
  file_compress_t csv = biomcmc_open_compress (outfilename, "w");
  int bad = 0;
  for (int c = 0; c < n_out; c++) {
    const char *nm = name_of (name_arg, medoid[c]);
    bad += biomcmc_write_compress (csv, nm) != (int) strlen (nm);
    for (int64_t m = offsets[c]; m < offsets[c + 1]; m++) {
      nm = name_of (name_arg, members[m]);
      bad += biomcmc_write_compress (csv, ",") != 1;
      bad += biomcmc_write_compress (csv, nm) != (int) strlen (nm);
    }
    bad += biomcmc_write_compress (csv, "\n") != 1;
  }
  biomcmc_close_compress (csv);
  if (bad) fprintf (stderr, "File %s may not be correctly compressed, %d error%s occurred.\n", outfilename, bad, bad > 1 ? "s" : "");
  strcpy (outfilename + outlength, ".aln.xz");
  file_compress_t aln = biomcmc_open_compress (outfilename, "w");
  if (db || device_parse) {   /* the text of the medoids exists on the device only: a bounded batch of it at a time */
    const size_t pitch = (size_t) nchar + 1;
    char *text = (char *) biomcmc_malloc (ROWS_BATCH * pitch);
    memset (text, 0, ROWS_BATCH * pitch);
    for (int a = 0; a < n_out; a += ROWS_BATCH) {
      const int m = n_out - a < ROWS_BATCH ? n_out - a : ROWS_BATCH;
      if (uvaia_clust_rows (ctx, medoid + a, m, text, pitch)) biomcmc_error ("%s", uvaia_clust_last_error (ctx));
      for (int k = 0; k < m; k++) write_fasta_record (aln, name_of (name_arg, medoid[a + k]), text + (size_t) k * pitch);
    }
    free (text);
  } else for (int c = 0; c < n_out; c++) write_fasta_record (aln, names.v[medoid[c]], seqs.v[medoid[c]]);
  biomcmc_close_compress (aln);
  if (packed_out && keep_medoids) write_packed_out_gathered (packed_out, ctx, device, nchar, ambig_r, compact, medoid, n_out, name_of, name_arg);
  else if (packed_out) write_packed_out (packed_out, ctx, device, nchar, ambig_r, compact, count, medoid, n_out, name_of, name_arg);
  uvaia_clust_close (ctx);
  fprintf (stderr, "GPU memory for sequence rows: %zu bytes at the peak (%s)\n", peak_row_bytes, keep_medoids ? "medoid rows in slabs and one push" : "every row kept");
  fprintf (stderr, "%d clusters from %ld sequences; GPU kernels: prep %.3lf ms, queues %.3lf ms, merge %.3lf ms, decode %.3lf ms, overlay %.3lf ms\n", n_out, (long) count,
           prep_ms, queue_ms, merge_ms, decode_ms, overlay_ms);
  fprintf (stderr, "Finished sorting clusters and saving files in %lf secs\n", biomcmc_update_elapsed_time (time0));

  for (int64_t i = 0; i < seqs.n; i++) free (seqs.v[i]);
  for (int64_t i = 0; i < names.n; i++) free (names.v[i]);
  free (seqs.v); free (names.v); free (medoid); free (offsets); free (members); free (outfilename);
  uvdb_set_close (set);
  free (packed_files);
  return EXIT_SUCCESS;
}
