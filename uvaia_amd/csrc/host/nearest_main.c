/*
 * nearest_main.c -- `uvaia`: for every query sequence, the closest neighbours in a (streamed) reference alignment.
 * Same options, status messages, output files and table columns as the reference's src/nearest.c; the batch loop
 * (src/nearest.c:288-306) runs on the GPU through include/uvaia_gpu.h.  Own code.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <libgen.h>
#include <omp.h>
#include <time.h>

#include "cli_common.h"
#include "gpu_glue.h"
#include "prepare.h"
#include "uvdb.h"
#include "uvdb_window.h"
#include "uvdb_set.h"
#include "uvdb_extract.h"
#include "fasta_blocks.h"

typedef struct {
  int help, version, acgt, keep_resolved, exclude_self, nbest, trim, pool, threads, threads_given, device, devices[64], n_devices;
  long long window; int window_given, window_report;
  int final_aln, final_rank, final_rank_given, final_only;
  double ambig_q, ambig_r;
  const char *out, *query;
  const char **ref; int n_ref;
  const char **packed_files; int n_packed;
  int device_parse, parse_block_given, parse_window_given;
  size_t parse_block; long long parse_window;
} options;

static void
usage (const char *prog, int long_help)
{
  printf ("%s \n", UVAIA_PACKAGE_STRING);
  printf ("For every query sequence, finds closest neighbours in reference alignment. \n");
  printf ("The score-distance scan and the neighbour heaps run on an AMD MI355X GPU.\n\n");
  printf ("The complete syntax is:\n\n %s [-hvkx] [--acgt] [-n <int>] [--trim=<int>] [-A <double>] [-a <double>] [-p <int>] [--device-parse] -r <ref.fa(.gz,.xz)> [-r <ref.fa(.gz,.xz)>]... <seqs.fa(.gz,.xz)> [-t <int>] [-o <without suffix>]\n\n", prog);
  printf ("  -h, --help                       print a longer help and exit\n");
  printf ("  -v, --version                    print version and exit\n");
  printf ("  --acgt                           considers only ACGT sites (i.e. unambiguous SNP differences) in query sequences (mismatch-based)\n");
  printf ("  -k, --keep_resolved              keep more resolved and exclude redundant query seqs (default is to keep all)\n");
  printf ("  -x, --exclude_self               Exclude reference sequences with same name as a query sequence\n");
  printf ("  -n, --nbest=<int>                number of best reference sequences per query to store (default=100)\n");
  printf ("  --trim=<int>                     number of sites to trim from both ends (default=0, suggested for sarscov2=230)\n");
  printf ("  -A, --ref_ambiguity=<double>     maximum allowed ambiguity for REFERENCE sequence to be excluded (default=0.5)\n");
  printf ("  -a, --query_ambiguity=<double>   maximum allowed ambiguity for QUERY sequence to be excluded (default=0.5)\n");
  printf ("  -p, --pool=<int>                 Pool size, i.e. how many reference seqs are sent to the GPU per batch (defaults to 64 per host thread; larger is faster)\n");
  printf ("  -r, --reference=<ref.fa(.gz,.xz)> aligned reference sequences (can be several files)\n");
  printf ("  --device-parse                   with -r: split the reference text into sequences on the GPU instead of reading it line by line; the references\n                                   are searched a window at a time and only those that become neighbours come back as text.  The same files,\n                                   from regular FASTA only (a NUL byte, text before the first header and a header without sequence are refused);\n                                   on one GPU, not with --packed.  Behind .gz or .xz the decompressor sets the pace and little is gained\n");
  printf ("  --parse-block=<bytes>            with --device-parse: the text is read in blocks of this size (64 to 1073741824, default 67108864); a record\n                                   must fit a block\n");
  printf ("  --parse-window=<refs>            with --device-parse: this many accepted references are resident before they are searched (rounded up to whole\n                                   pools; default: 65536, fewer when GPU memory is short)\n");
  printf ("  --packed=<db.uvdb>               reference database packed by `uvaiapack` (instead of -r): loaded as it is, no text parsing; can be several\n                                   files, searched in the order given as one database (all packed with the same -A: see `uvaiapack --merge -A`).\n                                   Compact files (`uvaiapack --compact`) are expanded on the GPU, on one device (not with a --devices list of several)\n");
  printf ("  --window=<refs>                  with --packed: keep only this many references on the GPU at a time (rounded up to whole pools and tiles\n                                   of 64), for a database larger than GPU memory; chosen automatically when the database does not fit\n");
  printf ("  --window-report                  with --packed: one line on stderr with the GPU's free memory before and after and the time of the window steps\n");
  printf ("  --final-aln                      with --packed: also write <prefix>.final.aln.xz, the alignment of exactly the references of the table (each once, in\n                                   stream order, chosen by position in the database and not by name), read back from the packed files on the GPU\n");
  printf ("  --final-rank=<int>               with --final-aln: only the references of rank <int> or better in some query's list (default: all, i.e. -n)\n");
  printf ("  --final-only                     with --final-aln: do not write <prefix>.aln.xz, the larger alignment of every reference that was a neighbour at\n                                   some moment of the search; the table is the same\n");
  printf ("  <seqs.fa(.gz,.xz)>               aligned query sequences\n");
  printf ("  -t, --nthreads=<int>             suggested number of host threads (only sets the default pool size here)\n");
  printf ("  -o, --output=<without suffix>    prefix of xzipped output alignment and table with nearest neighbour sequences\n");
  printf ("  --device=<int>                   GPU to use (default: current device)\n");
  printf ("  --devices=<list>                 several GPUs, e.g. 0-7 or 0,2,3: every GPU scans its share of the references against all\n                                   queries and keeps the neighbours of its share of the queries (same results as one GPU)\n");
  if (long_help) {
    printf ("\nNeighbours are sorted in the same order as the table columns, using the next column to break ties:\n");
    printf (" 1. ACGT_matches -- considering only ACGT \n 2. text_matches -- exact matches, thus M-M is a match but M-A is not\n");
    printf (" 3. partial_matches -- M-A is considered a match since the partially ambiguous `M` equals {A,C}. The fully ambiguous `N` is neglected\n");
    printf (" 4. valid_pair_comparisons -- the `effective` sequence length for the comparison (sites without gaps or N in any of the two sequences)\n");
    printf (" 5. ACGT_matches_unique -- matches outside the sites where all queries agree\n");
    printf (" 6. valid_ref_sites -- if everything else is the same, then sequences with less gaps and Ns are preferred\n");
    printf ("With '--acgt' only ACGT is considered and the columns are ACGT_matches, valid_ACGT_comparisons, ACGT_matches_unique, valid_ref_sites,\n dist_consensus and dist_unique (their sum is the usual SNP distance).\n");
  }
}

static options
parse_options (int argc, char **argv)
{
  options o;
  memset (&o, 0, sizeof o);
  o.nbest = 100; o.ambig_q = o.ambig_r = 0.5; o.pool = 64 * omp_get_max_threads (); o.device = -1;
  o.parse_block = FASTA_BLOCK_BYTES;
  o.ref = (const char **) biomcmc_malloc ((size_t) argc * sizeof (char *));
  o.packed_files = (const char **) biomcmc_malloc ((size_t) argc * sizeof (char *));
  static const struct option longopts[] = {
    {"help", no_argument, 0, 'h'}, {"version", no_argument, 0, 'v'}, {"acgt", no_argument, 0, 1000},
    {"keep_resolved", no_argument, 0, 'k'}, {"exclude_self", no_argument, 0, 'x'}, {"nbest", required_argument, 0, 'n'},
    {"trim", required_argument, 0, 1001}, {"query_ambiguity", required_argument, 0, 'a'}, {"ref_ambiguity", required_argument, 0, 'A'},
    {"pool", required_argument, 0, 'p'}, {"reference", required_argument, 0, 'r'}, {"nthreads", required_argument, 0, 't'},
    {"output", required_argument, 0, 'o'}, {"device", required_argument, 0, 1002}, {"packed", required_argument, 0, 1003}, {"devices", required_argument, 0, 1004},
    {"window", required_argument, 0, 1005}, {"window-report", no_argument, 0, 1006},
    {"final-aln", no_argument, 0, 1007}, {"final-rank", required_argument, 0, 1008}, {"final-only", no_argument, 0, 1009},
    {"device-parse", no_argument, 0, 1010}, {"parse-block", required_argument, 0, 1011}, {"parse-window", required_argument, 0, 1012}, {0, 0, 0, 0}};
  int ch, errors = 0;
  while ((ch = getopt_long (argc, argv, "hvkxn:a:A:p:r:t:o:", longopts, NULL)) != -1) switch (ch) {
    case 'h': o.help = 1; break;
    case 'v': o.version = 1; break;
    case 1000: o.acgt = 1; break;
    case 'k': o.keep_resolved = 1; break;
    case 'x': o.exclude_self = 1; break;
    case 'n': o.nbest = atoi (optarg); break;
    case 1001: o.trim = atoi (optarg); break;
    case 'a': o.ambig_q = atof (optarg); break;
    case 'A': o.ambig_r = atof (optarg); break;
    case 'p': o.pool = atoi (optarg); break;
    case 'r': o.ref[o.n_ref++] = optarg; break;
    case 't': o.threads = atoi (optarg); o.threads_given = 1; break;
    case 'o': o.out = optarg; break;
    case 1002: o.device = atoi (optarg); break;
    case 1004: o.n_devices = uvaia_parse_device_list (optarg, o.devices, 64); if (!o.n_devices) { fprintf (stderr, "--devices: expected a list such as 0-7 or 0,2,3\n"); exit (EXIT_FAILURE); } break;
    case 1003: o.packed_files[o.n_packed++] = optarg; break;
    case 1005: o.window = atoll (optarg); o.window_given = 1; break;
    case 1006: o.window_report = 1; break;
    case 1007: o.final_aln = 1; break;
    case 1008: o.final_rank = atoi (optarg); o.final_rank_given = 1; break;
    case 1009: o.final_only = 1; break;
    case 1010: o.device_parse = 1; break;
    case 1011: o.parse_block = (size_t) strtoull (optarg, NULL, 10); o.parse_block_given = 1; break;      /* (for tests: the block size of --device-parse in bytes) */
    case 1012: o.parse_window = atoll (optarg); o.parse_window_given = 1; break;                          /* (for tests: the window of --device-parse in references) */
    default: errors++;
  }
  if (optind < argc) o.query = argv[optind++];
  if (optind < argc) errors++;
  if (o.version) { printf ("%s\n", UVAIA_PACKAGE_VERSION); exit (EXIT_SUCCESS); }
  if (o.help) { usage (basename (argv[0]), 1); exit (EXIT_SUCCESS); }
  /* --device-parse: what does not go with it is refused here, before a GPU is touched or a file created */
  if (o.device_parse && o.n_packed) { fprintf (stderr, "--device-parse reads FASTA text (-r): it does not go with --packed, which holds no text to parse\n"); exit (EXIT_FAILURE); }
  if (o.device_parse && o.n_devices > 1) {
    fprintf (stderr, "--device-parse hands the references to the search in the memory of ONE GPU: give --device, or a --devices list of one device (%d were listed)\n", o.n_devices);
    exit (EXIT_FAILURE);
  }
  if (o.device_parse && (o.parse_block < 64 || o.parse_block > ((size_t) 1 << 30))) { fprintf (stderr, "--parse-block: expected 64 to 1073741824 bytes\n"); exit (EXIT_FAILURE); }
  if (!o.device_parse && o.parse_block_given) { fprintf (stderr, "--parse-block sets the block size of --device-parse: it needs that option\n"); exit (EXIT_FAILURE); }
  if (!o.device_parse && o.parse_window_given) { fprintf (stderr, "--parse-window sets the window of --device-parse: it needs that option\n"); exit (EXIT_FAILURE); }
  if (o.parse_window_given && o.parse_window < 1) { fprintf (stderr, "--parse-window: expected a positive number of references\n"); exit (EXIT_FAILURE); }
  if (errors || !o.query || (!o.n_ref && !o.n_packed) || (o.n_ref && o.n_packed)) {
    printf ("Error when reading arguments from command line:\n");
    usage (basename (argv[0]), 0);
    exit (EXIT_FAILURE);
  }
  /* --window: refused here, before anything touches a GPU */
  if (o.window_given && !o.n_packed) { fprintf (stderr, "--window needs --packed: only a packed database is searched a window at a time\n"); exit (EXIT_FAILURE); }
  if (o.window_given && o.window < 1) { fprintf (stderr, "--window: expected a positive number of references\n"); exit (EXIT_FAILURE); }
  if (o.n_packed > UVDB_SET_MAX_FILES) { fprintf (stderr, "--packed: at most %d files\n", UVDB_SET_MAX_FILES); exit (EXIT_FAILURE); }
  if (o.window_given && o.n_devices > 1) { fprintf (stderr, "--window works on one GPU: give --device, not a --devices list of several\n"); exit (EXIT_FAILURE); }
  /* --final-aln: refused here as well */
  if (o.final_aln && !o.n_packed) {
    fprintf (stderr, "--final-aln needs --packed: a reference read as text (-r) is gone once the search has passed it, only a packed database gives a second look at a row; pack the references with `uvaiapack`\n");
    exit (EXIT_FAILURE);
  }
  if (o.final_rank_given && !o.final_aln) { fprintf (stderr, "--final-rank needs --final-aln: it chooses what that file holds\n"); exit (EXIT_FAILURE); }
  if (o.final_only && !o.final_aln) { fprintf (stderr, "--final-only needs --final-aln: without it no alignment would be written at all\n"); exit (EXIT_FAILURE); }
  if (o.final_rank_given && o.final_rank < 1) { fprintf (stderr, "--final-rank: expected a rank of 1 or more\n"); exit (EXIT_FAILURE); }
  if (o.final_aln && o.n_devices > 1) { fprintf (stderr, "--final-aln works on one GPU: give --device, not a --devices list of several (the rows are read back through the staging slots of a plain context)\n"); exit (EXIT_FAILURE); }
  /* a compact file is expanded in a staging slot of one GPU; a group of devices gathers lanes on the host from the dense tiles of the mapping */
  for (int f = 0; o.n_devices > 1 && f < o.n_packed; f++) if (uvdb_file_version (o.packed_files[f]) == 2) {
    fprintf (stderr, "--devices with several GPUs: %s is a compact packed database (`uvaiapack --compact`), which is searched on one GPU only; convert it with `uvaiapack --merge -o dense.uvdb %s`\n", o.packed_files[f], o.packed_files[f]);
    exit (EXIT_FAILURE);
  }
  return o;
}

static double
wall_ms (void)
{
  struct timespec ts;
  clock_gettime (CLOCK_MONOTONIC, &ts);
  return (double) ts.tv_sec * 1e3 + (double) ts.tv_nsec * 1e-6;
}

/* ---- --packed: the files are one stream through uvdb_set.h, a single file as a set of one.  The tiles of every file are staged as the
 * file holds them, piece after piece of a staging slot, and the kept references of the pieces go into the resident store by position (a
 * file rarely ends on a tile boundary, -x leaves holes): appended behind what is resident (resident search), or as the next window
 * (windowed search). */

/* uvdb_stage_range (uvdb_extract.h) for the two searches: kept positions [a, b) into staging slot `slot`; returns whether sel is 0, 1, 2, ... */
static int
stage_range (uvaia_gpu_ctx *gpu, uvdb_set set, const uint64_t *keep, uint64_t a, uint64_t b, int slot, uvdb_set_piece *pieces, int *sel)
{
  int identity = 0;
  const int rc = uvdb_stage_range (gpu, set, keep, a, b, slot, pieces, sel, &identity);
  if (rc == UVDB_STAGE_ESPAN) biomcmc_error ("--packed: the references from %llu on span more file tiles than the engine counts", (unsigned long long) a);
  if (rc) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
  return identity;
}

/* the largest staging slot the ranges [w * step, (w + 1) * step) of n kept references need, in tiles (0: none is staged); resident: the
 * ranges are chunks of the resident load, of which those that go straight from the mapping need no slot */
static uint64_t
max_slot_tiles (uvdb_set set, const uint64_t *keep, uint64_t n, uint64_t step, int resident)
{
  uint64_t max_tiles = 0;
  for (uint64_t a = 0; a < n; a += step) {
    uint64_t st = 0;
    const uint64_t b = (a + step < n) ? a + step : n;
    if (resident && !uvdb_set_direct_tiles (set, keep, a, b, n, a, NULL, NULL)) continue;
    if (uvdb_set_span (set, keep, a, b, NULL, 0, NULL, &st, NULL)) biomcmc_error ("--packed: the references from %llu on span more file tiles than the engine counts", (unsigned long long) a);
    if (st > max_tiles) max_tiles = st;
  }
  return max_tiles;
}

/* The windowed search (include/uvaia_gpu.h, "windowed search"): stands where the resident search replaces the loops of
 * src/nearest.c:251-306, for a stream of which `window` references are on the GPU at a time.  The next window's tiles are handed to the
 * copy stream while the current one is searched; what entered a heap is decoded on the GPU.  Host memory: one window of flags, two of
 * selection entries and 256 rows of text, whatever the size of the files.  Returns the number of sequences written. */
static int
search_windowed (uvaia_gpu_ctx *gpu, uvdb_set set, const uint64_t *keep, uint64_t n, uint64_t window, uint64_t n_windows, size_t pool, int nchar,
                 file_compress_t outstream, name_table *names, double upload_ms[3])
{
  enum { ROUND = 256 };
  const uint64_t wmax = window < n ? window : n, slot_tiles = max_slot_tiles (set, keep, n, window, 0);
  const size_t pitch = ((size_t) nchar + 15) / 16 * 16;
  if (uvaia_gpu_db_reserve (gpu, (size_t) (wmax ? wmax : 1)) || uvaia_gpu_db_stage_reserve (gpu, (size_t) (slot_tiles ? slot_tiles : 1))) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
  uvdb_set_piece *pieces = (uvdb_set_piece *) biomcmc_malloc (UVDB_SET_MAX_FILES * sizeof (uvdb_set_piece));
  int *sel[2], identity[2] = {0, 0}, index[ROUND], n_output = 0;
  for (int i = 0; i < 2; i++) sel[i] = (int *) biomcmc_malloc ((size_t) (wmax ? wmax : 1) * sizeof (int));
  uint8_t *ent = (uint8_t *) biomcmc_malloc ((size_t) (wmax ? wmax : 1));
  char *rows = (char *) biomcmc_malloc (ROUND * pitch + 1);
  upload_ms[0] = upload_ms[1] = upload_ms[2] = 0.;
#define STAGE(w_) do { const uint64_t a_ = (w_) * window, b_ = (a_ + window < n) ? a_ + window : n; identity[(w_) & 1] = stage_range (gpu, set, keep, a_, b_, (int) ((w_) & 1), pieces, sel[(w_) & 1]); } while (0)
  double t = wall_ms ();
  if (n_windows) STAGE ((uint64_t) 0);
  upload_ms[0] = upload_ms[1] = wall_ms () - t;           /* the first window's upload has nothing to hide behind */
  for (uint64_t w = 0; w < n_windows; w++) {
    const uint64_t a = w * window, b = (a + window < n) ? a + window : n;
    if (uvaia_gpu_db_load_staged (gpu, (int) (w & 1), identity[w & 1] ? NULL : sel[w & 1], (int) (b - a))) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    if (uvaia_gpu_search_resident (gpu, pool, (int64_t) a, NULL)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    if (w + 1 < n_windows) {                              /* the search runs: the next window's tiles cross the bus next to it */
      t = wall_ms ();
      STAGE (w + 1);
      const double up = wall_ms () - t;
      t = wall_ms ();
      if (uvaia_gpu_sync (gpu)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
      upload_ms[0] += up;
      if (wall_ms () - t < 0.01 * up) upload_ms[1] += up;   /* the search had ended before the upload: counted as not hidden at all */
    } else if (uvaia_gpu_sync (gpu)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    if (!outstream) continue;                             /* --final-only: nothing is decoded during the search */
    if (uvaia_gpu_entered_flags (gpu, ent, 0)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    for (uint64_t k = 0; k < b - a;) {                    /* dump every sequence that entered some heap, in stream order */
      int m = 0;
      for (; k < b - a && m < ROUND; k++) if (ent[k]) index[m++] = (int) k;
      if (!m) break;
      if (uvaia_gpu_db_unpack_rows (gpu, index, m, rows, pitch)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
      for (int j = 0; j < m; j++) {
        const uint64_t i = a + (uint64_t) index[j], r = keep ? keep[i] : i;
        char *row = rows + (size_t) j * pitch, after = row[nchar];
        uvdb_set_apply_exceptions (set, r, row);
        row[nchar] = '\0';
        write_fasta_record (outstream, uvdb_set_name (set, r), row);
        row[nchar] = after;
        name_table_set (names, (int64_t) i, uvdb_set_name (set, r));
        n_output++;
      }
    }
  }
#undef STAGE
  upload_ms[2] = upload_ms[0] > 0. ? 1. - upload_ms[1] / upload_ms[0] : 0.;
  free (rows); free (ent); free (sel[0]); free (sel[1]); free (pieces);
  return n_output;
}

/* The n kept references into the resident store, in chunks of 16 384.  A chunk that is whole tiles of one file behind whole tiles
 * (uvdb_set_direct_tiles: without -x, every chunk of a single file) goes straight from the mapping.  Any other is staged piece by piece
 * and its lanes appended on the device; a group of devices takes whole host tiles, so for it the lanes are gathered here. */
static void
load_resident (uvaia_gpu_group *grp, uvaia_gpu_ctx *gpu, int n_devices, uvdb_set set, const uint64_t *keep, uint64_t n)
{
  const uint64_t chunk_tiles = 256, chunk = chunk_tiles * 64, slot_tiles = n_devices == 1 ? max_slot_tiles (set, keep, n, chunk, 1) : 0;
  const size_t tb = (size_t) set->tile_bytes, row = (size_t) set->side_row_ints, lane_pieces = tb / (64 * 16);   /* 16-byte pieces per lane */
  if (slot_tiles && uvaia_gpu_db_stage_reserve (gpu, (size_t) slot_tiles)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
  uvdb_set_piece *pieces = (uvdb_set_piece *) biomcmc_malloc (UVDB_SET_MAX_FILES * sizeof (uvdb_set_piece));
  int *sel = (int *) biomcmc_malloc ((size_t) chunk * sizeof (int));
  unsigned char *planes = NULL;                      /* the host tiles of a gathered chunk: allocated with the first one */
  int32_t *nn = NULL, *side = NULL;
  for (uint64_t a = 0; a < n; a += chunk) {
    const uint64_t b = (a + chunk < n) ? a + chunk : n, cnt = b - a;
    const int slot = (int) (a / chunk & 1);
    int f = 0; uint64_t t = 0;
    if (!uvdb_set_direct_tiles (set, keep, a, b, n, a, &f, &t)) {
      uvdb_reader db = set->db[f];
      if (uvaia_gpu_group_db_append_packed (grp, uvdb_tile_planes (db, t), db->non_n + t * 64, uvdb_tile_side_rows (db, t), (int) cnt)) biomcmc_error ("%s", uvaia_gpu_group_last_error (grp));
    } else if (n_devices == 1) {
      stage_range (gpu, set, keep, a, b, slot, pieces, sel);
      if (uvaia_gpu_db_append_staged (gpu, slot, sel, (int) cnt)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
    } else {
      if (!planes) {
        planes = (unsigned char *) biomcmc_malloc (chunk_tiles * tb);
        nn = (int32_t *) biomcmc_malloc (chunk * sizeof (int32_t)); side = (int32_t *) biomcmc_malloc (chunk * row * sizeof (int32_t));
      }
      memset (planes, 0, chunk_tiles * tb); memset (nn, 0, chunk * sizeof (int32_t)); memset (side, 0, chunk * row * sizeof (int32_t));
#pragma omp parallel for schedule(static)
      for (uint64_t k = 0; k < cnt; k++) {
        int fk = 0; uint64_t r = 0;
        uvdb_set_locate (set, keep ? keep[a + k] : a + k, &fk, &r);
        uvdb_reader db = set->db[fk];
        const unsigned char *src = (const unsigned char *) uvdb_tile_planes (db, r / 64) + (r % 64) * 16;
        unsigned char *dst = planes + (k / 64) * tb + (k % 64) * 16;
        for (size_t p = 0; p < lane_pieces; p++) memcpy (dst + p * 1024, src + p * 1024, 16);
        nn[k] = db->non_n[r];
        memcpy (side + k * row, uvdb_tile_side_rows (db, r / 64) + (r % 64) * row, row * sizeof (int32_t));
      }
      if (uvaia_gpu_group_db_append_packed (grp, planes, nn, side, (int) cnt)) biomcmc_error ("%s", uvaia_gpu_group_last_error (grp));
    }
  }
  free (planes); free (nn); free (side); free (sel); free (pieces);
}

/* the packed files as the search saw them: position i of the kept stream is reference keep[i] of the set (keep NULL: i itself), n of them */
typedef struct { uvdb_set set; uint64_t *keep; uint64_t n; } packed_stream;

/* the search over o->packed_files: replaces the read/filter/fill loop of main (src/nearest.c:251-286); returns the number of sequences written.
 * outstream NULL (--final-only): no sequence is decoded or written.  stream not NULL (--final-aln): the set and the keep list (NULL: every
 * reference is kept) stay with the caller, whose table and final alignment name references by their position in the kept stream. */
static int
search_packed (const options *o, query_t query, uvaia_gpu_group *grp, uvaia_gpu_ctx *gpu, file_compress_t outstream, name_table *names, int *count, int *same_name, int64_t *time0,
               packed_stream *stream)
{
  char msg[1024];
  const char *first = o->packed_files[0];
  const int one = o->n_packed == 1, nchar = query->aln->nchar;
  uvdb_set set = uvdb_set_open (o->packed_files, o->n_packed, 0, msg, sizeof msg);
  if (!set) biomcmc_error ("%s", msg);
  if ((int) set->nchar != nchar) biomcmc_error ("packed database %s has %u sites but query sequences have %d sites; all sequences must be aligned", first, set->nchar, nchar);
  if (set->ref_ambiguity != o->ambig_r)
    biomcmc_error (one ? "packed database %s was filtered with -A %g: search it with that value, or rewrite it with a tighter one by `uvaiapack --merge -A` (a filter cannot be undone)"
                       : "packed databases %s ... were filtered with -A %g: search them with that value, or rewrite them with a tighter one by `uvaiapack --merge -A` (a filter cannot be undone)", first, set->ref_ambiguity);
  if (set->side_row_ints != (uint32_t) uvaia_gpu_db_side_row_ints () || set->tile_bytes != uvaia_gpu_db_tile_bytes (gpu)) biomcmc_error ("packed database %s does not match this engine's tile layout", first);
  const uint64_t n_all = set->n_ref;
  int n_output = 0;
  /* -x: references named like a query leave the stream (src/nearest.c:257-262) */
  uint64_t *keep = NULL, n = n_all;
  if (o->exclude_self) {
    keep = (uint64_t *) biomcmc_malloc ((size_t) (n_all ? n_all : 1) * sizeof (uint64_t));
    n = 0;
    for (uint64_t i = 0; i < n_all; i++) { if (lookup_hashtable (query->aln->taxlabel_hash, (char *) uvdb_set_name (set, i)) > -1) (*same_name)++; else keep[n++] = i; }
    if (n == n_all) { free (keep); keep = NULL; }
  }
  /* a window at a time (--window, or a stream that does not fit the GPU's free memory), or resident as a whole */
  uint64_t window = 0, n_windows = 0;
  size_t mem_before = uvaia_gpu_free_bytes (gpu);
  if (o->window_given) {
    if (uvdb_window_plan (n, (uint64_t) o->pool, (uint64_t) o->window, &window, &n_windows)) biomcmc_error ("--window %lld with a pool of %d: the window is beyond what the engine counts", o->window, o->pool);
  } else if (o->n_devices == 1 && mem_before) {
    /* per resident reference: packed planes, the planes derived for the query set (with the valid-site plane the appends write), side
       row, counts and flag; an --acgt context also keeps the four-plane image of a window */
    const uint64_t bpr = uvaia_gpu_packed_bytes_per_ref (gpu) + uvaia_gpu_derived_bytes_per_ref (gpu) + uvaia_gpu_db_tile_bytes (gpu) / 256
                       + (uint64_t) uvaia_gpu_db_side_row_ints () * 4 + 20 + (o->acgt ? uvaia_gpu_db_tile_bytes (gpu) / 64 : 0);
    const int64_t w = uvdb_window_choose (n, (uint64_t) o->pool, bpr, (uint64_t) mem_before);
    if (w < 0) biomcmc_error (one ? "packed database %s: not even one window of %d references (%llu bytes each, and two staging slots) fits the %zu free bytes of the GPU; try a smaller --pool"
                                  : "packed databases %s ...: not even one window of %d references (%llu bytes each, and two staging slots) fits the %zu free bytes of the GPU; try a smaller --pool",
                              first, o->pool, (unsigned long long) bpr, mem_before);
    if (w > 0 && uvdb_window_plan (n, (uint64_t) o->pool, (uint64_t) w, &window, &n_windows))
      biomcmc_error (one ? "packed database %s: no window plan for %lld references" : "packed databases %s ...: no window plan for %lld references", first, (long long) w);
    if (w > 0) fprintf (stderr, one ? "The packed database does not fit the free memory of the GPU: searching it in %llu windows of %llu sequences.\n"
                                    : "The packed databases do not fit the free memory of the GPU: searching them in %llu windows of %llu sequences.\n", (unsigned long long) n_windows, (unsigned long long) window);
  }
  *count = (int) n_all;
  if (!window) {
    if (uvaia_gpu_group_db_reserve (grp, (size_t) (n ? n : 1))) biomcmc_error ("%s", uvaia_gpu_group_last_error (grp));
    load_resident (grp, gpu, o->n_devices, set, keep, n);
  }
  if (one) fprintf (stderr, "Loaded %d packed sequences from %s in %.3lf secs;\n", (int) n, first, biomcmc_update_elapsed_time (time0));
  else     fprintf (stderr, "Loaded %d packed sequences from %d files in %.3lf secs;\n", (int) n, o->n_packed, biomcmc_update_elapsed_time (time0));
  if (window) {
    double upload_ms[3], part_ms[3] = {0., 0., 0.};
    n_output = search_windowed (gpu, set, keep, n, window, n_windows, (size_t) o->pool, nchar, outstream, names, upload_ms);
    if (o->window_report) {
      uvaia_gpu_window_ms (gpu, part_ms, 0);
      fprintf (stderr, "window report: {\"window\": %llu, \"n_windows\": %llu, \"free_before\": %zu, \"free_after\": %zu, \"select_ms\": %.3f, \"derive_ms\": %.3f, \"decode_ms\": %.3f, \"upload_ms\": %.3f, \"upload_hidden_share\": %.3f}\n",
               (unsigned long long) window, (unsigned long long) n_windows, mem_before, uvaia_gpu_free_bytes (gpu), part_ms[0], part_ms[1], part_ms[2], upload_ms[0], upload_ms[2]);
    }
  } else {
    uint8_t *ent = outstream ? (uint8_t *) biomcmc_malloc ((size_t) (n ? n : 1)) : NULL;
    if (n && uvaia_gpu_group_search_resident (grp, (size_t) o->pool, 0, ent)) biomcmc_error ("%s", uvaia_gpu_group_last_error (grp));
    if (!ent && uvaia_gpu_group_sync (grp)) biomcmc_error ("%s", uvaia_gpu_group_last_error (grp));   /* (a search that hands no flags back does not wait) */
    char *text = (char *) biomcmc_malloc ((size_t) nchar + 1);
    for (uint64_t i = 0; outstream && i < n; i++) if (ent[i]) {     /* dump every sequence that entered some heap, in stream order */
      const uint64_t r = keep ? keep[i] : i;
      n_output++;
      uvdb_set_unpack_reference (set, r, text);
      write_fasta_record (outstream, uvdb_set_name (set, r), text);
      name_table_set (names, (int64_t) i, uvdb_set_name (set, r));
    }
    free (text); free (ent);
    if (o->window_report) fprintf (stderr, "window report: {\"window\": 0, \"n_windows\": 0, \"free_before\": %zu, \"free_after\": %zu}\n", mem_before, uvaia_gpu_free_bytes (gpu));
  }
  /* Without --final-aln (stream NULL) the set goes here, as it always did: the caller is about to wait for xz to finish the dump, and unmapping
     files the runtime has copied straight out of (over a second for 1.5 GB) is hidden behind that wait; at the end of main it would be exposed. */
  if (stream) { stream->set = set; stream->keep = keep; stream->n = n; }
  else { free (keep); uvdb_set_close (set); }
  return n_output;
}

/* name of a reference by its ordinal, straight from the set: what the dump loop otherwise leaves in the name table (--final-only) */
static const char *
packed_stream_name (int64_t ordinal, void *user)
{
  const packed_stream *ps = (const packed_stream *) user;
  if (ordinal < 0 || (uint64_t) ordinal >= ps->n) return NULL;
  return uvdb_set_name (ps->set, ps->keep ? ps->keep[ordinal] : (uint64_t) ordinal);
}

/* --final-aln.  Membership is by ordinal: the heaps are collected once more with the ordinal in place of the name and put in the table's
 * order by the same heap_finalise_heap_qsort, so rank j here is rank j there, also among references that share a name. */
static const char *
ordinal_as_name (int64_t ordinal, void *user)
{
  snprintf ((char *) user, 24, "%lld", (long long) ordinal);
  return (const char *) user;
}

static int
compare_positions (const void *a, const void *b)
{
  const uint64_t x = *(const uint64_t *) a, y = *(const uint64_t *) b;
  return (x > y) - (x < y);
}

static int
write_final_record (void *user, uint64_t k, uint64_t stream, const char *name, const char *row)
{
  write_fasta_record ((file_compress_t) user, name, row);
  return 0;
}

/* <prefix>.final.aln.xz: every reference of rank `rank` or better in some query's list, once, in stream order, as the regular dump writes
 * it; the rows come back from the packed files through the search's own context (uvdb_extract.h).  Returns their number. */
static uint64_t
save_final_alignment (const options *o, query_t query, uvaia_gpu_group *grp, uvaia_gpu_ctx *gpu, packed_stream *ps, const char *filename, uvdb_extract_stats *stats)
{
  const int nq = query->aln->ntax, rank = (o->final_rank_given && o->final_rank < o->nbest) ? o->final_rank : o->nbest;
  char text[24], msg[1024];
  heap_t *heap = (heap_t *) biomcmc_malloc ((size_t) nq * sizeof (heap_t));
  for (int i = 0; i < nq; i++) heap[i] = new_heap_t (o->nbest);
  if (uvaia_gpu_group_collect_heaps (grp, heap, ordinal_as_name, text)) biomcmc_error ("%s", uvaia_gpu_group_last_error (grp));
  uint64_t *pos = (uint64_t *) biomcmc_malloc (((size_t) nq * (size_t) rank + 1) * sizeof (uint64_t)), m = 0, u = 0;
  for (int i = 0; i < nq; i++) {
    heap_finalise_heap_qsort (heap[i]);
    for (int j = 0; j < heap[i]->n && j < rank; j++) {
      const long long ord = heap[i]->seq[j].name ? atoll (heap[i]->seq[j].name) : -1;
      if (ord < 0 || (uint64_t) ord >= ps->n) biomcmc_error ("--final-aln: a neighbour of query %s lies outside the %llu references searched", query->aln->taxlabel->string[i], (unsigned long long) ps->n);
      pos[m++] = ps->keep ? ps->keep[ord] : (uint64_t) ord;
    }
    del_heap_t (heap[i]);
  }
  free (heap);
  qsort (pos, (size_t) m, sizeof (uint64_t), compare_positions);
  for (uint64_t k = 0; k < m; k++) if (!u || pos[u - 1] != pos[k]) pos[u++] = pos[k];
  file_compress_t out = biomcmc_open_compress (filename, "w");
  if (uvdb_extract (ps->set, gpu, pos, u, write_final_record, out, stats, msg, sizeof msg)) biomcmc_error ("--final-aln: %s", msg);
  free (ps->keep); uvdb_set_close (ps->set);           /* the set has done its work: unmapped while xz finishes the file (see search_packed) */
  ps->keep = NULL; ps->set = NULL; ps->n = 0;
  biomcmc_close_compress (out);
  free (pos);
  return u;
}

/* ---- `uvaia -r --device-parse`.  The text is read in blocks (fasta_blocks.h) and split into records and rows on the GPU
 * (uvaia_gpu_fasta_scan, uvaia_gpu_fasta_rows); the filters of the fill loop in main run on the integers of the record table; the rows of the
 * survivors go from the parser's memory into the resident database and, as text, into the text row store.  When `window` references (a
 * multiple of the pool) are resident, and at the end of every file, they are searched in pools -- the pools of the fill loop, whose short
 * last pool also ends a file -- and those that entered a heap come back as text.  Only the names are taken from the host's copy of the text. */
#define PARSE_MAX_RECORDS (1 << 18)     /* records per scan, as in pack_main.c; a block that holds more is scanned in several steps */
#define PARSE_ROWS_BATCH 256            /* rows of text per copy back */

struct search_parse {
  const options *o;
  query_t query;
  uvaia_gpu_ctx *gpu;
  uvaia_gpu_fasta *fasta;
  file_compress_t outstream;
  name_table *names;
  int nchar, non_n_ref, max_records, resident, window;
  size_t row_pitch;
  uvaia_gpu_fasta_record *rec;          /* max_records of each */
  int *row_of, *sel, *nn;
  char **name;                          /* of the resident references: window */
  uint8_t *entered;
  char *rows; int index[PARSE_ROWS_BATCH];
  int count, n_invalid, same_name, n_output, last_print;
  int64_t ordinal, *time1;
};

static int
search_parse_scan (void *user, const char *text, size_t n, int final, int *n_records, size_t *consumed, int *bad_kind, size_t *bad_off, char *err, size_t errlen)
{
  struct search_parse *d = (struct search_parse *) user;
  if (!uvaia_gpu_fasta_scan (d->fasta, text, n, final, n_records, consumed)) return 0;
  const unsigned kind = uvaia_gpu_fasta_bad (d->fasta, bad_off);       /* irregular text: the block reader names the byte of the stream */
  *bad_kind = kind == UVAIA_GPU_FASTA_NUL ? FASTA_BAD_NUL : kind == UVAIA_GPU_FASTA_TEXT ? FASTA_BAD_TEXT : kind == UVAIA_GPU_FASTA_EMPTY ? FASTA_BAD_EMPTY : FASTA_BAD_NONE;
  snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta));
  return -1;
}

/* the resident references are searched, those that entered a heap written in stream order, and the window is emptied */
static int
search_parse_flush (struct search_parse *d, char *err, size_t errlen)
{
  const int n = d->resident, nchar = d->nchar;
  if (!n) return 0;
  if (uvaia_gpu_search_resident (d->gpu, (size_t) d->o->pool, d->ordinal, d->entered)) { snprintf (err, errlen, "%s", uvaia_gpu_last_error (d->gpu)); return -1; }
  for (int k = 0; k < n;) {
    int m = 0;
    for (; k < n && m < PARSE_ROWS_BATCH; k++) if (d->entered[k]) d->index[m++] = k;
    if (!m) break;
    if (uvaia_gpu_text_rows (d->gpu, d->index, m, d->rows, d->row_pitch)) { snprintf (err, errlen, "%s", uvaia_gpu_last_error (d->gpu)); return -1; }
    for (int j = 0; j < m; j++) {
      char *row = d->rows + (size_t) j * d->row_pitch, after = row[nchar];
      row[nchar] = '\0';
      write_fasta_record (d->outstream, d->name[d->index[j]], row);
      row[nchar] = after;
      name_table_set (d->names, d->ordinal + d->index[j], d->name[d->index[j]]);
      d->n_output++;
    }
  }
  d->ordinal += n;
  if (uvaia_gpu_db_clear (d->gpu) || uvaia_gpu_text_clear (d->gpu)) { snprintf (err, errlen, "%s", uvaia_gpu_last_error (d->gpu)); return -1; }
  for (int k = 0; k < n; k++) free (d->name[k]);
  d->resident = 0;
  if (d->count / 10000 > d->last_print / 10000) {       /* the progress line of the fill loop, per window */
    int highest = 0;
    uvaia_gpu_max_tolerance (d->gpu, &highest);
    fprintf (stderr, "Total: %d sequences analysed, %d saved, %d poorly resolved. Highest number of ACGT mismatches = %d in current neighbourhood. %.3lf secs elapsed. ",
             d->count, d->n_output, d->n_invalid, highest, biomcmc_update_elapsed_time (d->time1));
    if (d->o->exclude_self) fprintf (stderr, " %d already present in query alignment.\n", d->same_name); else fprintf (stderr, "\n");
    d->last_print = d->count;
  }
  return 0;
}

static int
search_parse_records (void *user, char *text, size_t consumed, int n_records, char *err, size_t errlen)
{
  struct search_parse *d = (struct search_parse *) user;
  const void *d_rows = NULL; size_t pitch = 0; int n_rows = 0, n_sel = 0;
  if (uvaia_gpu_fasta_records (d->fasta, d->rec) || uvaia_gpu_fasta_rows (d->fasta, d->nchar, &d_rows, &pitch, &n_rows, d->row_of)) {
    snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta));
    return -1;
  }
  for (int k = 0; k < n_records; k++) {               /* the filters of main's fill loop, in its order, on the counts the device made */
    const uvaia_gpu_fasta_record *r = d->rec + k;
    char *name = text + r->name_off;
    name[r->name_len] = '\0';                         /* the line end behind the name, or the byte of room behind the block */
    d->count++;
    if (d->o->exclude_self && lookup_hashtable (d->query->aln->taxlabel_hash, name) > -1) { d->same_name++; continue; }
    if (r->non_n < d->non_n_ref) { d->n_invalid++; continue; }
    if (d->row_of[k] < 0) {
      biomcmc_warning ("Reference sequence '%s' has %u sites but query sequences have %d sites\n", name, r->seq_len, d->nchar);
      snprintf (err, errlen, "all sequences must be aligned");
      return -1;
    }
    d->sel[n_sel] = d->row_of[k]; d->nn[n_sel] = r->non_n;
    d->rec[n_sel++].name_off = r->name_off;            /* (n_sel <= k: the table is read ahead of where it is written) */
  }
  for (int a = 0; a < n_sel;) {                        /* into the window, as much as it still takes; a full window is searched */
    const int room = d->window - d->resident, m = n_sel - a < room ? n_sel - a : room;
    if (uvaia_gpu_db_append_device (d->gpu, d_rows, pitch, d->sel + a, m, d->nn + a) || uvaia_gpu_text_append_device (d->gpu, d_rows, pitch, d->sel + a, m)) {
      snprintf (err, errlen, "%s", uvaia_gpu_last_error (d->gpu));
      return -1;
    }
    for (int c = 0; c < m; c++) d->name[d->resident + c] = strdup (text + d->rec[a + c].name_off);      /* the block buffer is recycled */
    d->resident += m; a += m;
    if (d->resident == d->window && search_parse_flush (d, err, errlen)) return -1;
  }
  return 0;
}

static void
search_parse_open (struct search_parse *d, const options *o, query_t query, uvaia_gpu_ctx *gpu, file_compress_t outstream, name_table *names, int64_t *time1)
{
  memset (d, 0, sizeof *d);
  d->o = o; d->query = query; d->gpu = gpu; d->outstream = outstream; d->names = names; d->time1 = time1;
  d->nchar = query->aln->nchar;
  d->non_n_ref = (int) (d->nchar * (1. - o->ambig_r));
  d->row_pitch = ((size_t) d->nchar + 15) / 16 * 16;
  d->max_records = o->parse_block / 4 + 1 < PARSE_MAX_RECORDS ? (int) (o->parse_block / 4 + 1) : PARSE_MAX_RECORDS;      /* (a record has four bytes at least) */
  if (uvaia_gpu_fasta_open (&d->fasta, o->devices[0], o->parse_block, d->max_records)) biomcmc_error ("%s", uvaia_gpu_fasta_last_error (NULL));
  /* per resident reference: what search_packed counts (packed planes, derived planes, side row, counts and flag) and its row of text; the
     parser's own rows, at most a block's worth, come out of the free memory first */
  const uint64_t bpr = uvaia_gpu_packed_bytes_per_ref (gpu) + uvaia_gpu_derived_bytes_per_ref (gpu) + uvaia_gpu_db_tile_bytes (gpu) / 256
                     + (uint64_t) uvaia_gpu_db_side_row_ints () * 4 + 20 + d->row_pitch;
  uint64_t mem = uvaia_gpu_free_bytes (gpu);
  if (mem) mem = mem > 2 * (uint64_t) o->parse_block ? mem - 2 * (uint64_t) o->parse_block : 1;
  d->window = (int) uvdb_parse_window ((uint64_t) o->pool, o->parse_window_given ? (uint64_t) o->parse_window : 0, bpr, mem);
  if (d->window < 1) biomcmc_error ("--device-parse: no window for a pool of %d", o->pool);
  if (uvaia_gpu_db_reserve (gpu, (size_t) d->window) || uvaia_gpu_text_reserve (gpu, (size_t) d->window)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
  d->rec = (uvaia_gpu_fasta_record *) biomcmc_malloc ((size_t) d->max_records * sizeof (uvaia_gpu_fasta_record));
  d->row_of = (int *) biomcmc_malloc ((size_t) d->max_records * sizeof (int));
  d->sel = (int *) biomcmc_malloc ((size_t) d->max_records * sizeof (int));
  d->nn = (int *) biomcmc_malloc ((size_t) d->max_records * sizeof (int));
  d->name = (char **) biomcmc_malloc ((size_t) d->window * sizeof (char *));
  d->entered = (uint8_t *) biomcmc_malloc ((size_t) d->window);
  d->rows = (char *) biomcmc_malloc (PARSE_ROWS_BATCH * d->row_pitch + 1);
}

/* one -r file; the window is searched at its end, so that no pool spans two files */
static uint64_t
search_parse_file (struct search_parse *d, const char *path)
{
  char msg[1024], failed[1024];
  uint64_t nb = 0;
  fasta_blocks fb = fasta_blocks_open (path, d->o->parse_block, uvaia_gpu_fasta_pinned_alloc, uvaia_gpu_fasta_pinned_free, msg, sizeof msg);
  int rc = fb ? fasta_blocks_run (fb, d->max_records, search_parse_scan, d, search_parse_records, d, &nb, msg, sizeof msg) : -1;
  if (fasta_blocks_finish (fb, failed, sizeof failed)) biomcmc_error ("%s", failed);      /* a decompressor that failed mid-stream: that is the finding */
  if (rc) {
    const int text = strstr (msg, "FASTA text:") || strstr (msg, "does not fit a block");     /* what the parser refuses, the line reader takes */
    biomcmc_error ("%s%s", msg, text ? " (--device-parse takes regular FASTA whose records fit a block: `uvaia` without it reads this file line by line)" : "");
  }
  if (search_parse_flush (d, msg, sizeof msg)) biomcmc_error ("%s: %s", path, msg);
  return nb;
}

static void
search_parse_close (struct search_parse *d, uint64_t bytes)
{
  double ms[2] = {0., 0.}, text_ms[2] = {0., 0.};
  uvaia_gpu_fasta_kernel_ms (d->fasta, ms, 0);
  uvaia_gpu_text_ms (d->gpu, text_ms, 0);
  fprintf (stderr, "device parse: {\"bytes\": %llu, \"block_bytes\": %zu, \"window\": %d, \"scan_ms\": %.3f, \"rows_ms\": %.3f, \"text_in_ms\": %.3f, \"text_out_ms\": %.3f}\n", (unsigned long long) bytes,
           d->o->parse_block, d->window, ms[0], ms[1], text_ms[0], text_ms[1]);
  uvaia_gpu_fasta_close (d->fasta);
  free (d->rec); free (d->row_of); free (d->sel); free (d->nn); free (d->name); free (d->entered); free (d->rows);
}

static void
save_distance_table (heap_t *heap, query_t query, const char *filename)
{
  file_compress_t xz = biomcmc_open_compress (filename, "w");
  const char *header = query->acgt
    ? "query,reference,rank,ACGT_matches,valid_ACGT_comparisons,ACGT_matches_unique,valid_ref_sites,dist_consensus,dist_unique\n"
    : "query,reference,rank,ACGT_matches,text_matches,partial_matches,valid_pair_comparisons,ACGT_matches_unique,valid_ref_sites\n";
  if (biomcmc_write_compress (xz, header) != (int) strlen (header)) biomcmc_warning ("problem saving header of compressed file %s;", xz->filename);
  int errors = 0;
  for (int i = 0; i < query->aln->ntax; i++) {
    heap_finalise_heap_qsort (heap[i]);
    /* the reference prints heap_size rows; a heap holding exactly heap_size-1 items makes it read an unused slot
       (src/min_heap.c:152-157, src/nearest.c:531-532): only the stored items are printed here */
    for (int j = 0; j < heap[i]->n; j++) {
      const q_item *it = &heap[i]->seq[j];
      size_t len = strlen (it->name ? it->name : "") + query->aln->taxlabel->nchars[i] + 96;
      char *line = (char *) biomcmc_malloc (len);
      int w = snprintf (line, len, "%s,%s,%d", query->aln->taxlabel->string[i], it->name ? it->name : "", j + 1);
      for (int k = 0; k < 6; k++) w += snprintf (line + w, len - (size_t) w, ",%d", it->score[k]);
      snprintf (line + w, len - (size_t) w, "\n");
      if (biomcmc_write_compress (xz, line) != (int) strlen (line)) errors++;
      free (line);
    }
  }
  if (errors) fprintf (stderr, "File %s may not have been correctly compressed, %d error%s occurred.\n", xz->filename, errors, errors > 1 ? "s" : "");
  biomcmc_close_compress (xz);
}

int
main (int argc, char **argv)
{
  int64_t time0[2], time1[2];
  biomcmc_get_time (time0);
  options o = parse_options (argc, argv);
  if (o.ambig_q < 0.001) o.ambig_q = 0.001;
  if (o.ambig_q > 1.) o.ambig_q = 1.;
  if (o.ambig_r < 0.001) o.ambig_r = 0.001;
  if (o.ambig_r > 1.) o.ambig_r = 1.;
  if (o.nbest < 1) o.nbest = 1;
  if (o.pool < 1) o.pool = 1;
  fprintf (stderr, "program: %s package: %s\n", basename (argv[0]), UVAIA_PACKAGE_STRING);
  if (o.threads_given) {
    int max_threads = omp_get_max_threads ();
    if (o.threads < 1 || o.threads > max_threads) o.threads = max_threads;
    omp_set_num_threads (o.threads);
  }
  fprintf (stderr, "Creating a queue of %d sequences; for each query, the %d closest sequences will be stored\n", o.pool, o.nbest);

  size_t outlength = 0;
  char *outfilename = outfile_from_prefix (o.out ? o.out : (o.acgt ? "nn_uvaia_acgt" : "nn_uvaia"), &outlength);

  /* 1. queries: read, quality filter, column classes, ordering, optional pruning */
  alignment aln = read_fasta_alignment_from_file (o.query, 0xf);
  fprintf (stderr, "Finished reading %d query references in %lf secs;\n", aln->ntax, biomcmc_update_elapsed_time (time0));
  uvaia_set_prepare_device (o.n_devices ? o.devices[0] : o.device);
  query_t query = uvaia_prepare_query (aln, o.trim, 1, o.acgt, o.ambig_q, o.keep_resolved, 0);
  fprintf (stderr, "Query database composed of %d valid references, after excluding low quality%s.\n", query->aln->ntax,
           o.keep_resolved ? " and redundant (less resolved) sequences" : "");
  if (query->aln->ntax < 1) biomcmc_error ("No valid reference sequences found. Please check file %s.", o.query);
  biomcmc_get_time (time1);
  if (query->acgt) fprintf (stderr, "Considering ACGT differences only (excluding all other characters). \n");
  else             fprintf (stderr, "Considering text match and partially ambiguous (excluding only gaps and Ns).\n");
  if (o.exclude_self) {
    fprintf (stderr, "Reference sequences with same name as query sequences will be excluded from the comparison.\n");
    query->aln->taxlabel_hash = new_hashtable (query->aln->ntax);
    for (int j = 0; j < query->aln->ntax; j++) insert_hashtable (query->aln->taxlabel_hash, query->aln->taxlabel->string[j], j);
  }

  /* 2. the engine and the host-side batch */
  /* one GPU (--device) or several (--devices): a group of one is a plain context */
  uvaia_gpu_group *grp = NULL;
  if (!o.n_devices) { o.n_devices = 1; o.devices[0] = o.device; }
  if (uvaia_gpu_group_open_query (&grp, query, o.nbest, o.devices, o.n_devices, (size_t) (o.n_devices > 1 && o.pool < 64 ? 64 : o.pool), 0)) biomcmc_error ("%s", o.n_devices > 1 ? uvaia_gpu_group_last_error (NULL) : uvaia_gpu_last_error (NULL));
  uvaia_gpu_ctx *gpu = uvaia_gpu_group_member (grp, 0);
  if (o.n_devices > 1) fprintf (stderr, "Using %d GPUs: references and queries are shared out among them.\n", o.n_devices);
  char **seq = (char **) biomcmc_malloc ((size_t) o.pool * sizeof (char *)), **name = (char **) biomcmc_malloc ((size_t) o.pool * sizeof (char *));
  int *non_n = (int *) biomcmc_malloc ((size_t) o.pool * sizeof (int));
  uint8_t *entered = (uint8_t *) biomcmc_malloc ((size_t) o.pool);
  name_table names = {NULL, 0};
  file_compress_t outstream = o.final_only ? NULL : biomcmc_open_compress (outfilename, "w");     /* --final-only: <prefix>.aln.xz is not even created */
  packed_stream packed = {NULL, NULL, 0};
  const int non_n_ref = (int) (query->aln->nchar * (1. - o.ambig_r));
  const int print_interval = 10000;
  int count = 0, n_invalid = 0, same_name = 0, n_output = 0;
  int64_t ordinal = 0;

  fprintf (stderr, "\n Notice that the number of sites used in the comparisons (i.e. non-indel and non-N in at least one query) is %d, and the total alignment length is %d",
           query->n_idx + query->n_idx_c + query->n_idx_m, query->aln->nchar);
  fprintf (stderr, "\n The next step is main comparison, which may take a while\n\n");

  if (o.n_packed) {     /* packed databases, one stream */
    n_output = search_packed (&o, query, grp, gpu, outstream, &names, &count, &same_name, time0, o.final_aln ? &packed : NULL);
    if (outstream) fprintf (stderr, "Total of %d sequences searched; %d saved sequences include closest neighbours and intermediate. %.3lf secs elapsed. \n", count, n_output, biomcmc_update_elapsed_time (time1));
    else           fprintf (stderr, "Total of %d sequences searched; none saved during the search (--final-only). %.3lf secs elapsed. \n", count, biomcmc_update_elapsed_time (time1));
    if (o.exclude_self) fprintf (stderr, " %d reference sequences already present in query alignment (based on name only).\n", same_name);
  }
  struct search_parse parse;
  uint64_t parse_bytes = 0;
  if (o.device_parse) search_parse_open (&parse, &o, query, gpu, outstream, &names, time1);
  for (int j = 0; j < o.n_ref; j++) {
    if (o.device_parse) {       /* the same filters, pools and files, from rows made on the GPU */
      parse.count = count; parse.n_invalid = n_invalid; parse.same_name = same_name; parse.n_output = n_output; parse.ordinal = ordinal;
      parse_bytes += search_parse_file (&parse, o.ref[j]);
      count = parse.count; n_invalid = parse.n_invalid; same_name = parse.same_name; n_output = parse.n_output; ordinal = parse.ordinal;
    } else {
      readfasta_t rfas = new_readfasta (o.ref[j]);
      bool end_of_file = false;
      while (!end_of_file) {
        int fill = 0;
        while (fill < o.pool && !end_of_file) {          /* the serial slot-filling loop of the reference (src/nearest.c:251-286) */
          if (readfasta_next (rfas) < 0) { end_of_file = true; break; }
          count++;
          if (o.exclude_self && lookup_hashtable (query->aln->taxlabel_hash, rfas->name) > -1) { same_name++; continue; }
          int nn = quick_count_sequence_non_N (rfas->seq, rfas->seqlength);
          if (nn < non_n_ref) { n_invalid++; continue; }
          if (rfas->seqlength != (size_t) query->aln->nchar) {
            biomcmc_warning ("Reference sequence '%s' has %zu sites but query sequences have %d sites\n", rfas->name, rfas->seqlength, query->aln->nchar);
            biomcmc_error ("all sequences must be aligned");
          }
          non_n[fill] = nn;
          seq[fill] = rfas->seq; rfas->seq = NULL;       /* steal the buffers, as the reference does */
          name[fill] = rfas->name; rfas->name = NULL;
          fill++;
        }
        if (fill) {
          if (uvaia_gpu_group_push (grp, (const char *const *) seq, non_n, fill, ordinal, entered)) biomcmc_error ("%s", uvaia_gpu_group_last_error (grp));
          for (int c = 0; c < fill; c++) if (entered[c]) {   /* dump every sequence that entered some heap, in stream order */
            n_output++;
            write_fasta_record (outstream, name[c], seq[c]);
            name_table_set (&names, ordinal + c, name[c]);
          }
          ordinal += fill;
          for (int c = 0; c < fill; c++) { free (seq[c]); free (name[c]); }
        }
        if (count >= print_interval && (count % print_interval) < o.pool) {
          int highest = 0;       /* cq->max_incompatible: the largest tolerance over all heaps (src/nearest.c:290-291,323-324) */
          for (int d = 0; d < o.n_devices; d++) {
            int v = 0, q0 = 0, q1 = query->aln->ntax;
            uvaia_gpu_ctx *cx = uvaia_gpu_group_member (grp, d);
            if (o.n_devices > 1) { uvaia_gpu_group_sync (grp); uvaia_gpu_group_query_shard (grp, d, &q0, &q1); if (q1 <= q0) continue; uvaia_gpu_set_active_queries (cx, q0, q1); }
            if (!uvaia_gpu_max_tolerance (cx, &v) && v > highest) highest = v;
            if (o.n_devices > 1) uvaia_gpu_set_active_queries (cx, 0, query->aln->ntax);
          }
          fprintf (stderr, "Total: %d sequences analysed, %d saved, %d poorly resolved. Highest number of ACGT mismatches = %d in current neighbourhood. %.3lf secs elapsed. ",
                   count, n_output, n_invalid, highest, biomcmc_update_elapsed_time (time1));
          if (o.exclude_self) fprintf (stderr, " %d already present in query alignment.\n", same_name); else fprintf (stderr, "\n");
        }
      }
      del_readfasta (rfas);
    }
    fprintf (stderr, "Finished reading file %s in %.3lf secs;\n", o.ref[j], biomcmc_update_elapsed_time (time0));
    fprintf (stderr, "Total of %d sequences read; %d saved sequences include closest neighbours and intermediate, %d too ambiguous (excluded). %.3lf secs elapsed. \n",
             count, n_output, n_invalid, biomcmc_update_elapsed_time (time1));
    if (o.exclude_self) fprintf (stderr, " %d reference sequences already present in query alignment (based on name only).\n", same_name);
  }
  if (o.device_parse) search_parse_close (&parse, parse_bytes);
  if (outstream) {
    biomcmc_close_compress (outstream);
    fprintf (stderr, "Saved %d sequences to file %s , %.3lf secs elapsed.\n", n_output, outfilename, biomcmc_update_elapsed_time (time0));
  }

  /* 3. heaps back to the host, table */
  heap_t *heap = (heap_t *) biomcmc_malloc ((size_t) query->aln->ntax * sizeof (heap_t));
  for (int i = 0; i < query->aln->ntax; i++) heap[i] = new_heap_t (o.nbest);
  /* (--final-only: the dump loop did not run, the names come from the set) */
  if (o.final_only ? uvaia_gpu_group_collect_heaps (grp, heap, packed_stream_name, &packed) : uvaia_gpu_group_collect_heaps (grp, heap, name_table_get, &names)) biomcmc_error ("%s", uvaia_gpu_group_last_error (grp));
  strcpy (outfilename + outlength, ".csv.xz");
  save_distance_table (heap, query, outfilename);
  fprintf (stderr, "Saved distance table to file %s , %.3lf secs elapsed.\n", outfilename, biomcmc_update_elapsed_time (time0));
  if (o.final_aln) {
    uvdb_extract_stats st;
    memset (&st, 0, sizeof st);
    strcpy (outfilename + outlength, ".final.aln.xz");
    const uint64_t n_final = save_final_alignment (&o, query, grp, gpu, &packed, outfilename, &st);
    fprintf (stderr, "Saved %llu sequences of the final neighbour lists to file %s , %.3lf secs elapsed.\n", (unsigned long long) n_final, outfilename, biomcmc_update_elapsed_time (time0));
    if (o.window_report)
      fprintf (stderr, "final report: {\"n_final\": %llu, \"n_dumped\": %d, \"chunks\": %llu, \"stage_calls\": %llu, \"tiles_staged\": %llu, \"stage_ms\": %.3f, \"decode_ms\": %.3f, \"decode_kernel_ms\": %.3f, \"exceptions_ms\": %.3f, \"write_ms\": %.3f}\n",
               (unsigned long long) n_final, n_output, (unsigned long long) st.n_chunks, (unsigned long long) st.n_pieces, (unsigned long long) st.n_tiles, st.stage_ms, st.decode_ms, st.kernel_ms, st.exceptions_ms, st.write_ms);
  }
  free (packed.keep);
  uvdb_set_close (packed.set);

  for (int i = 0; i < query->aln->ntax; i++) del_heap_t (heap[i]);
  free (heap); free (seq); free (name); free (non_n); free (entered); free (o.ref); free (o.packed_files);
  name_table_free (&names);
  uvaia_gpu_group_close (grp);
  del_query_structure (query);
  free (outfilename);
  return EXIT_SUCCESS;
}
