/*
 * ball_main.c -- `uvaiaball`: keeps the reference sequences within a distance radius of any query sequence.
 * Same options and output as the reference's src/ball.c; the per-batch loop (src/ball.c:248-251) runs on the GPU.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <libgen.h>
#include <omp.h>

#include <pthread.h>

#include "cli_common.h"
#include "gpu_glue.h"
#include "prepare.h"
#include "uvdb.h"
#include "uvdb_set.h"

#define PACKED_CHUNK 65536    /* references per round trip of the packed path without -p (1 024 tiles) */

/* ---- the packed path: the per-batch loop of src/ball.c:248-259 for a database whose text is not in memory.  Chunks of whole tiles
 * go from the mapping to the engine as they are; the text of the kept references comes back from the device.  Chunk c belongs to
 * member c mod n (one context and one host thread per member); records are written in chunk order.  Several files (a repeated --packed)
 * are searched one after the other: the chunks of the first, then those of the second, and so on -- a chunk never spans two files, and
 * uvaia_gpu_ball_packed ignores the lanes past a file's last reference. */
typedef struct { int file; uint64_t first, cnt; } packed_chunk;
typedef struct {
  uvdb_reader *dbs; int n_files;
  packed_chunk *chunks;
  uvaia_gpu_ctx **gpu;
  int n_members, dist, non_n_ref, nchar;
  uint64_t chunk, n_chunks;
  file_compress_t out;
  pthread_mutex_t lock;
  pthread_cond_t turn;
  uint64_t next_chunk;                  /* the chunk whose records are written next */
  int n_output, n_invalid;
  double t_search, t_unpack, t_write;   /* summed over the members */
} packed_run;

static void
packed_member (packed_run *run, int m)
{
  const size_t pitch = ((size_t) run->nchar + 16) / 16 * 16;       /* room for the NUL; the engine's own row pitch unless nchar is a multiple of 16 */
  int *mindist = (int *) biomcmc_malloc ((size_t) run->chunk * sizeof (int)), *keep = (int *) biomcmc_malloc ((size_t) run->chunk * sizeof (int));
  char *rows = NULL;
  size_t rows_cap = 0;
  for (uint64_t c = (uint64_t) m; c < run->n_chunks; c += (uint64_t) run->n_members) {
    const uint64_t first = run->chunks[c].first, cnt = run->chunks[c].cnt;
    uvdb_reader db = run->dbs[run->chunks[c].file];
    double t0 = omp_get_wtime ();
    if (uvaia_gpu_ball_packed (run->gpu[m], uvdb_tile_planes (db, first / 64), (int) cnt, run->dist + 1, mindist)) biomcmc_error ("%s", uvaia_gpu_last_error (run->gpu[m]));
    double t1 = omp_get_wtime ();
    int n_keep = 0, invalid = 0;
    for (uint64_t i = 0; i < cnt; i++) {
      if (db->non_n[first + i] < run->non_n_ref) invalid++;
      else if (mindist[i] <= run->dist) keep[n_keep++] = (int) i;
    }
    if ((size_t) n_keep > rows_cap) {
      free (rows);
      rows_cap = (size_t) n_keep;
      rows = (char *) biomcmc_malloc (rows_cap * pitch);
    }
    if (uvaia_gpu_unpack_rows (run->gpu[m], keep, n_keep, rows, pitch)) biomcmc_error ("%s", uvaia_gpu_last_error (run->gpu[m]));
    for (int k = 0; k < n_keep; k++) {
      rows[(size_t) k * pitch + (size_t) run->nchar] = '\0';
      uvdb_apply_exceptions (db, first + (uint64_t) keep[k], rows + (size_t) k * pitch);
    }
    double t2 = omp_get_wtime ();
    pthread_mutex_lock (&run->lock);
    while (run->next_chunk != c) pthread_cond_wait (&run->turn, &run->lock);
    pthread_mutex_unlock (&run->lock);
    double t3 = omp_get_wtime ();        /* it is this chunk's turn: nobody else writes */
    for (int k = 0; k < n_keep; k++) write_fasta_record (run->out, uvdb_name (db, first + (uint64_t) keep[k]), rows + (size_t) k * pitch);
    double t4 = omp_get_wtime ();
    pthread_mutex_lock (&run->lock);
    run->n_output += n_keep; run->n_invalid += invalid;
    run->t_search += t1 - t0; run->t_unpack += t2 - t1; run->t_write += t4 - t3;
    run->next_chunk = c + 1;
    pthread_cond_broadcast (&run->turn);
    pthread_mutex_unlock (&run->lock);
  }
  free (rows); free (mindist); free (keep);
}

typedef struct { packed_run *run; int member; pthread_t id; } packed_thread;

static void *
packed_thread_main (void *arg)
{
  packed_thread *t = (packed_thread *) arg;
  packed_member (t->run, t->member);
  return NULL;
}

static void
search_packed (const char *const *files, int n_files, query_t query, int dist, double ambig_r, int pool, const int *devices, int n_devices, file_compress_t outstream, int64_t *time0)
{
  char msg[1024];
  packed_run run;
  memset (&run, 0, sizeof run);
  /* the set checks that the files agree on the alignment length and the tile layout; the filter of the radius search is judged file by file */
  uvdb_set set = uvdb_set_open (files, n_files, UVDB_SET_ANY_AMBIGUITY, msg, sizeof msg);
  if (!set) biomcmc_error ("%s", msg);
  const char *packed = files[0];
  const struct uvdb_header *h = &set->db[0]->h;
  if ((int) h->nchar != query->aln->nchar) biomcmc_error ("packed database %s has %u sites but query sequences have %d sites; all sequences must be aligned", packed, h->nchar, query->aln->nchar);
  uint64_t max_tiles = 0;
  for (int f = 0; f < n_files; f++) {
    const struct uvdb_header *hf = &set->db[f]->h;
    if (!uvdb_radius_filter_is_exact ((int) hf->nchar, ambig_r, hf->ref_ambiguity))
      biomcmc_error ("packed database %s was filtered with -A %g (at least %d valid sites), this search with -A %g keeps references from %d valid sites: some are not in the file; pack with a larger -A or use -r",
                     files[f], hf->ref_ambiguity, (int) (hf->nchar * (1. - hf->ref_ambiguity)), ambig_r, (int) (hf->nchar * ambig_r));
    if (hf->n_tiles > max_tiles) max_tiles = hf->n_tiles;
  }
  if (n_files == 1) fprintf (stderr, "Loaded %d packed sequences from %s in %.3lf secs;\n", (int) set->n_ref, packed, biomcmc_update_elapsed_time (time0));
  else              fprintf (stderr, "Loaded %d packed sequences from %d files in %.3lf secs;\n", (int) set->n_ref, n_files, biomcmc_update_elapsed_time (time0));
  /* chunks of whole tiles: -p rounded down to a multiple of 64, never more than the (largest) database */
  uint64_t chunk = pool > 0 ? (uint64_t) (pool / 64) * 64 : PACKED_CHUNK;
  if (chunk > max_tiles * 64) chunk = max_tiles * 64;
  if (chunk < 64) chunk = 64;
  run.dbs = set->db; run.n_files = n_files; run.chunk = chunk;
  for (int f = 0; f < n_files; f++) run.n_chunks += (set->db[f]->h.n_ref + chunk - 1) / chunk;
  run.chunks = (packed_chunk *) biomcmc_malloc ((size_t) (run.n_chunks ? run.n_chunks : 1) * sizeof (packed_chunk));
  {
    uint64_t c = 0;
    for (int f = 0; f < n_files; f++) for (uint64_t first = 0; first < set->db[f]->h.n_ref; first += chunk, c++) {
      const uint64_t left = set->db[f]->h.n_ref - first;
      run.chunks[c].file = f; run.chunks[c].first = first; run.chunks[c].cnt = left < chunk ? left : chunk;
    }
  }
  run.n_members = n_devices; run.dist = query->dist; run.nchar = query->aln->nchar; run.out = outstream;
  run.non_n_ref = (int) (query->aln->nchar * ambig_r);                /* src/ball.c:201 */
  run.gpu = (uvaia_gpu_ctx **) biomcmc_malloc ((size_t) n_devices * sizeof (uvaia_gpu_ctx *));
  fprintf (stderr, "Searching in chunks of %d sequences on %d device context%s; radius distance is %d (refs more distant than this are excluded)\n", (int) chunk, n_devices, n_devices > 1 ? "s" : "", dist);
  for (int m = 0; m < n_devices; m++) {
    run.gpu[m] = NULL;
    if (uvaia_gpu_open_query (&run.gpu[m], query, 2, devices[m], (size_t) chunk)) biomcmc_error ("%s", uvaia_gpu_last_error (NULL));
    if (h->side_row_ints != (uint32_t) uvaia_gpu_db_side_row_ints () || h->tile_bytes != uvaia_gpu_db_tile_bytes (run.gpu[m])) biomcmc_error ("packed database %s does not match this engine's tile layout", packed);
  }
  pthread_mutex_init (&run.lock, NULL);
  pthread_cond_init (&run.turn, NULL);
  packed_thread *th = (packed_thread *) biomcmc_malloc ((size_t) n_devices * sizeof (packed_thread));
  for (int m = 0; m < n_devices; m++) { th[m].run = &run; th[m].member = m; }
  for (int m = 1; m < n_devices; m++) if (pthread_create (&th[m].id, NULL, packed_thread_main, &th[m])) biomcmc_error ("cannot start the host thread of device context %d", m);
  packed_member (&run, 0);
  for (int m = 1; m < n_devices; m++) pthread_join (th[m].id, NULL);
  free (th);
  pthread_cond_destroy (&run.turn);
  pthread_mutex_destroy (&run.lock);
  fprintf (stderr, "Finished searching packed database %s%s in %.3lf secs; Total of %d sequences read, %d sequences within radius (kept), %d too ambiguous (excluded)\n",
           packed, n_files > 1 ? " and the files after it" : "", biomcmc_update_elapsed_time (time0), (int) set->n_ref, run.n_output, run.n_invalid);
  fprintf (stderr, "Time in seconds, summed over the device contexts: %.3lf search (with the copy of the tiles), %.3lf unpack, %.3lf write\n", run.t_search, run.t_unpack, run.t_write);
  fprintf (stderr, "Saved %d sequences to file %s\n", run.n_output, outstream->filename);
  for (int m = 0; m < n_devices; m++) uvaia_gpu_close (run.gpu[m]);
  free (run.gpu); free (run.chunks);
  uvdb_set_close (set);
}

int
main (int argc, char **argv)
{
  int help = 0, version = 0, acgt = 0, keep_resolved = 0, dist = 1, trim = 0, pool = 0, device = -1, n_ref = 0, errors = 0, ch;
  int devices[64], n_devices = 0;
  double ambig_q = 0.5, ambig_r = 0.5;
  const char *out = NULL, *qfile = NULL, *packed = NULL;
  const char **packed_files = (const char **) biomcmc_malloc ((size_t) argc * sizeof (char *)); int n_packed = 0;
  const char **ref = (const char **) biomcmc_malloc ((size_t) argc * sizeof (char *));
  static const struct option longopts[] = {
    {"help", no_argument, 0, 'h'}, {"version", no_argument, 0, 'v'}, {"acgt", no_argument, 0, 1000}, {"keep_resolved", no_argument, 0, 'k'},
    {"distance", required_argument, 0, 'd'}, {"trim", required_argument, 0, 1001}, {"query_ambiguity", required_argument, 0, 'a'},
    {"ref_ambiguity", required_argument, 0, 'A'}, {"pool", required_argument, 0, 'p'}, {"reference", required_argument, 0, 'r'},
    {"nthreads", required_argument, 0, 't'}, {"output", required_argument, 0, 'o'}, {"device", required_argument, 0, 1002},
    {"packed", required_argument, 0, 1003}, {"devices", required_argument, 0, 1004}, {0, 0, 0, 0}};
  while ((ch = getopt_long (argc, argv, "hvkd:a:A:p:r:t:o:", longopts, NULL)) != -1) switch (ch) {
    case 'h': help = 1; break;
    case 'v': version = 1; break;
    case 1000: acgt = 1; break;
    case 'k': keep_resolved = 1; break;
    case 'd': dist = atoi (optarg); break;
    case 1001: trim = atoi (optarg); break;
    case 'a': ambig_q = atof (optarg); break;
    case 'A': ambig_r = atof (optarg); break;
    case 'p': pool = atoi (optarg); break;
    case 'r': ref[n_ref++] = optarg; break;
    case 't': break;                                  /* host threads do not matter here */
    case 'o': out = optarg; break;
    case 1002: device = atoi (optarg); break;
    case 1003: if (!packed) packed = optarg; packed_files[n_packed++] = optarg; break;
    case 1004: n_devices = uvaia_parse_device_list (optarg, devices, 64); if (!n_devices) { fprintf (stderr, "--devices: expected a list such as 0-7 or 0,2,3\n"); errors++; } break;
    default: errors++;
  }
  if (optind < argc) qfile = argv[optind++];
  if (version) { printf ("%s\n", UVAIA_PACKAGE_VERSION); return EXIT_SUCCESS; }
  if (n_devices && !packed && !help) { fprintf (stderr, "--devices goes with --packed; the text path takes --device\n"); errors++; }
  if (n_packed > UVDB_SET_MAX_FILES) { fprintf (stderr, "--packed: at most %d files\n", UVDB_SET_MAX_FILES); errors++; }
  if (help || errors || !qfile || (!n_ref && !packed) || (n_ref && packed)) {
    printf ("%s \nSearch reference alignment for sequences within a distance radius of the query sequences (experimental).\n\n", UVAIA_PACKAGE_STRING);
    printf (" %s [-hvk] [--acgt] [-d <int>] [--trim=<int>] [-A <double>] [-a <double>] [-p <int>] -r <ref.fa(.gz,.xz)>... <seqs.fa(.gz,.xz)> [-o <without suffix>]\n",
            basename (argv[0]));
    printf (" %s [same options] --packed=<db.uvdb> [--packed=<db.uvdb>]... [--devices=<list>] <seqs.fa(.gz,.xz)>\n\n", basename (argv[0]));
    printf ("  --packed=<db.uvdb>               reference database packed by `uvaiapack` (instead of -r): searched tile by tile as it is, no text parsing;\n");
    printf ("                                   -A must not be below one minus the -A it was packed with (both 0.5 by default); -p is rounded down to a multiple of 64;\n");
    printf ("                                   can be several files, searched one after the other as one database\n");
    printf ("  --devices=<list>                 with --packed: one GPU context per listed device (e.g. 0-3 or 0,0), chunks are dealt out among them\n");
    return help ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  for (int f = 0; f < n_packed; f++) if (uvdb_file_version (packed_files[f]) == 2) {     /* the radius search reads dense tiles from the mapping */
    fprintf (stderr, "uvaiaball --packed: %s is a compact packed database (`uvaiapack --compact`), which this search does not read; convert it with `uvaiapack --merge -o dense.uvdb %s`\n", packed_files[f], packed_files[f]);
    return EXIT_FAILURE;
  }
  if (ambig_q < 0.001) ambig_q = 0.001;
  if (ambig_q > 1.) ambig_q = 1.;
  if (ambig_r < 0.001) ambig_r = 0.001;
  if (ambig_r > 1.) ambig_r = 1.;
  int n_clust = omp_get_max_threads ();
  if (pool >= n_clust) n_clust = pool;                /* src/ball.c:161-166 */
  fprintf (stderr, "Experimental program: %s package: %s\n", basename (argv[0]), UVAIA_PACKAGE_STRING);
  if (!packed) fprintf (stderr, "Creating a queue of %d sequences; radius distance is %d (refs more distant than this are excluded)\n", n_clust, dist);

  size_t outlength = 0;
  char *outfilename = outfile_from_prefix (out ? out : "ball_uvaia", &outlength);
  int64_t time0[2];
  biomcmc_get_time (time0);
  alignment aln = read_fasta_alignment_from_file (qfile, 0xf);
  uvaia_set_prepare_device (n_devices ? devices[0] : device);
  query_t query = uvaia_prepare_query (aln, trim, dist, acgt, ambig_q, keep_resolved, 1);
  fprintf (stderr, "Query database now composed of %d valid references, after removing redundant (%s resolved) sequences.\n", query->aln->ntax, keep_resolved ? "less" : "more");
  if (query->aln->ntax < 1) biomcmc_error ("No valid reference sequences found. Please check file %s.", qfile);

  if (packed) {
    file_compress_t packed_out = biomcmc_open_compress (outfilename, "w");
    if (!n_devices) { n_devices = 1; devices[0] = device; }
    search_packed (packed_files, n_packed, query, dist, ambig_r, pool, devices, n_devices, packed_out, time0);
    biomcmc_close_compress (packed_out);
    del_query_structure (query);
    free (ref); free (packed_files); free (outfilename);
    return EXIT_SUCCESS;
  }

  uvaia_gpu_ctx *gpu = NULL;
  if (uvaia_gpu_open_query (&gpu, query, 2, device, (size_t) n_clust)) biomcmc_error ("%s", uvaia_gpu_last_error (NULL));
  char **seq = (char **) biomcmc_malloc ((size_t) n_clust * sizeof (char *)), **name = (char **) biomcmc_malloc ((size_t) n_clust * sizeof (char *));
  int *mindist = (int *) biomcmc_malloc ((size_t) n_clust * sizeof (int));
  file_compress_t outstream = biomcmc_open_compress (outfilename, "w");
  const int non_n_ref = (int) (query->aln->nchar * ambig_r);   /* src/ball.c:201 (note: not 1-A as in uvaia) */
  int count = 0, n_invalid = 0, n_output = 0;

  for (int j = 0; j < n_ref; j++) {
    readfasta_t rfas = new_readfasta (ref[j]);
    bool end_of_file = false;
    while (!end_of_file) {
      int fill = 0;
      while (fill < n_clust && !end_of_file) {
        if (readfasta_next (rfas) < 0) { end_of_file = true; break; }
        count++;
        if (quick_count_sequence_non_N (rfas->seq, rfas->seqlength) < non_n_ref) { n_invalid++; continue; }
        if (rfas->seqlength != (size_t) query->aln->nchar) {
          biomcmc_warning ("Reference sequence '%s' has %zu sites but query sequences have %d sites\n", rfas->name, rfas->seqlength, query->aln->nchar);
          biomcmc_error ("all sequences must be aligned");
        }
        seq[fill] = rfas->seq; rfas->seq = NULL;
        name[fill] = rfas->name; rfas->name = NULL;
        fill++;
      }
      if (fill) {
        if (uvaia_gpu_ball (gpu, (const char *const *) seq, fill, query->dist + 1, mindist)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
        for (int c = 0; c < fill; c++) {
          if (mindist[c] <= query->dist) { n_output++; write_fasta_record (outstream, name[c], seq[c]); }
          free (seq[c]); free (name[c]);
        }
      }
    }
    del_readfasta (rfas);
    fprintf (stderr, "Finished reading file %s in %.3lf secs; Total of %d sequences read, %d sequences within radius (kept), %d too ambiguous (excluded)\n",
             ref[j], biomcmc_update_elapsed_time (time0), count, n_output, n_invalid);
  }
  fprintf (stderr, "Saved %d sequences to file %s\n", n_output, outstream->filename);
  biomcmc_close_compress (outstream);
  uvaia_gpu_close (gpu);
  del_query_structure (query);
  free (seq); free (name); free (mindist); free (ref); free (outfilename);
  return EXIT_SUCCESS;
}
