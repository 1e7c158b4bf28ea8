/*
 * align_main.c -- `uvaialign`: aligns query sequences against one reference sequence and writes them on the reference's
 * columns.  Same options, filters, messages and output as the reference's src/align.c; the per-pool loop over align_query
 * (src/align.c:224-233,357-390) runs on the GPU through include/uvaia_align.h.
 *
 * --packed (no counterpart in the reference): the aligned rows go from the aligner's device memory straight into a packed database
 * (uvdb.h), the file `uvaiapack` would write from the text output: census, -A filter, packing and exception runs happen on the rows where
 * they lie (include/uvaia_gpu.h, "rows that are already in device memory").  Own code.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <inttypes.h>
#include <libgen.h>
#include <omp.h>

#include "cli_common.h"
#include "fastaseq.h"
#include "gpu_glue.h"
#include "uvdb.h"
#include "uvdb_packer.h"
#include "../../../include/uvaia_align.h"
#include "../../../include/uvaia_gpu.h"

/* one pool into the packed database in the making: the rows of the aligner's last run, where they lie */
static int
packer_add_pool (struct uvdb_packer *p, uvaia_aligner *al, char **name, int fill)
{
  const void *d_rows = NULL; size_t pitch = 0; int n = 0;
  if (uvaia_align_device_rows (al, &d_rows, &pitch, &n, NULL)) { snprintf (p->err, sizeof p->err, "%s", uvaia_align_last_error (al)); return -1; }
  if (n != fill) { snprintf (p->err, sizeof p->err, "the aligner holds %d rows, the pool %d", n, fill); return -1; }
  return uvdb_packer_add_block (p, d_rows, pitch, n, name);
}

int
main (int argc, char **argv)
{
  int help = 0, version = 0, to_screen = 0, pool = 256 * omp_get_max_threads (), device = 0, errors = 0, n_fasta = 0, compact = 0, ch;   /* src/align.c:59-63 */
  int devices[64], n_devices = 0;
  double ambig = 0.5, ambig_r = 0.5;
  const char *out = NULL, *ref_file = NULL, *packed = NULL;
  static const struct option longopts[] = {
    {"help", no_argument, 0, 'h'}, {"version", no_argument, 0, 'v'}, {"stdout", no_argument, 0, 1000}, {"ambiguity", required_argument, 0, 'a'},
    {"pool", required_argument, 0, 'p'}, {"reference", required_argument, 0, 'r'}, {"nthreads", required_argument, 0, 't'},
    {"output", required_argument, 0, 'o'}, {"device", required_argument, 0, 1001}, {"devices", required_argument, 0, 1002},
    {"packed", required_argument, 0, 1003}, {"ref_ambiguity", required_argument, 0, 'A'}, {"compact", no_argument, 0, 1004}, {0, 0, 0, 0}};
  while ((ch = getopt_long (argc, argv, "hva:p:r:t:o:A:", longopts, NULL)) != -1) switch (ch) {
    case 'h': help = 1; break;
    case 'v': version = 1; break;
    case 1000: to_screen = 1; break;
    case 'a': ambig = atof (optarg); break;
    case 'p': pool = atoi (optarg); break;
    case 'r': if (ref_file) errors++; ref_file = optarg; break;
    case 't': break;                                  /* the alignments run on the GPU: host threads do not matter */
    case 'o': out = optarg; break;
    case 1001: device = atoi (optarg); break;
    case 1002: n_devices = uvaia_parse_device_list (optarg, devices, 64); if (!n_devices) { fprintf (stderr, "--devices: expected a list such as 0-7 or 0,2,3\n"); exit (EXIT_FAILURE); } break;
    case 1003: packed = optarg; break;
    case 1004: compact = 1; break;
    case 'A': ambig_r = atof (optarg); break;
    default: errors++;
  }
  const char **fasta = (const char **) argv + optind;
  n_fasta = argc - optind;
  if (version) { printf ("%s\n", UVAIA_PACKAGE_VERSION); return EXIT_SUCCESS; }
  if (!help && !errors && compact && !packed) {
    fprintf (stderr, "--compact chooses the form of the packed database: it needs --packed <out.uvdb>\n");
    errors++;
  }
  if (help || errors || !ref_file || n_fasta < 1 || pool < 1) {
    printf ("%s \nAlign query sequences against a reference\nThe complete syntax is:\n\n", UVAIA_PACKAGE_STRING);
    printf (" %s [-hv] [--stdout] [-p <int>] [-t <int>] [-o <without suffix>] [-a <double>] [--packed <out.uvdb> [--compact]] [-A <double>] -r <ref.fa|ref.fa.xz> <seqs.fa|seqs.fa.xz> [<seqs.fa|seqs.fa.xz>]...\n\n", basename (argv[0]));
    printf ("  -h, --help                       print a longer help and exit\n  -v, --version                    print version and exit\n");
    printf ("  --stdout                         print alignment to stdout (to redirect/pipe) instead of compress to file; much faster but may generate a big output\n");
    printf ("  -p, --pool=<int>                 How many query sequences are read in batch, to be aligned in parallel (defaults to 256 per thread)\n");
    printf ("  -t, --nthreads=<int>             accepted for compatibility (the alignments run on the GPU)\n");
    printf ("  -o, --output=<without suffix>    prefix of xzipped output alignment\n");
    printf ("  -a, --ambiguity=<double>         maximum allowed ambiguity for sequence to be excluded (default=0.5)\n");
    printf ("  -r, --reference=<ref.fa|ref.fa.xz> reference sequence in fasta format, possibly compressed with gz, xz, bz2\n");
    printf ("  <seqs.fa|seqs.fa.xz>             sequences to align in fasta format, possibly compressed with gz, xz, bz2 (can be multiple files)\n");
    printf ("  --device=<int>                   GPU to use (default 0)\n");
    printf ("  --devices=<list>                 several GPUs, e.g. 0-7 or 0,2,3: every pool of queries is cut among them (same rows as one GPU)\n");
    printf ("  --packed=<out.uvdb>              write the aligned sequences straight into a packed database, the file `uvaiapack` makes of the text output;\n");
    printf ("                                   the text itself is then written only if -o or --stdout is given as well (one GPU only)\n");
    printf ("  --compact                        with --packed: write the compact form of the database, the file `uvaiapack --compact` makes of the text output\n");
    printf ("                                   (several times smaller; encoded on the GPU once its base row is fixed, after 4096 sequences)\n");
    printf ("  -A, --ref_ambiguity=<double>     with --packed: maximum allowed ambiguity for an ALIGNED sequence to be kept in the database (default=0.5), as in `uvaiapack`\n");
    if (help) {
      printf ("Based on the wavefront algorithm (WFA, https://github.com/smarco/WFA), computed on the GPU.\n");
      printf ("Since the sequences are assumed to be similar, sequences too short or too big w.r.t. the reference are rejected.\n\n");
      printf ("The reference sequence and the unaligned fasta files can be compressed with gz, xz, bz2. The alignment output will be compressed with xz, ");
      printf ("unless you miss the tool. In this case the next available compression is tried (then the file extension might not correspond to it).\n\n");
      printf ("The command `pool` is the number of unaligned sequences read into memory at once (the higher the better, given your memory constraints).\n");
    }
    return (help && !errors) ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  if (ambig < 0.001) ambig = 0.001;                   /* src/align.c:132-133 */
  if (ambig > 1.) ambig = 1.;
  if (ambig_r < 0.001) ambig_r = 0.001;               /* pack_main.c:46-47 */
  if (ambig_r > 1.) ambig_r = 1.;
  if (packed && n_devices > 1) {   /* the rows of a pool would lie on several cards and a tile takes 64 consecutive ones: not built */
    fprintf (stderr, "--packed writes the database from the rows on ONE GPU: give --device, or a --devices list of one device (%d were listed)\n", n_devices);
    return EXIT_FAILURE;
  }
  const bool write_text = !packed || out || to_screen;
  int64_t time0[2], time1[2];
  biomcmc_get_time (time0);
  fprintf (stderr, "program: %s package: %s\n", basename (argv[0]), UVAIA_PACKAGE_STRING);

  size_t outlength = 0;
  char *outfilename = NULL;
  if (to_screen) fprintf (stderr, "Sequences will be shown uncompressed in screen (to redirect to file or pipe into another software).\n");
  else if (write_text) {
    char randname[32];
    if (!out) { sprintf (randname, "uvaia.%" PRIx64, (uint64_t) time0[1] & 0xffffff); out = randname; }     /* src/align.c:155-159 */
    outfilename = outfile_from_prefix (out, &outlength);
    fprintf (stderr, "Sequences will be compressed (if possible) and saved into file %s.\n", outfilename);
  }

  /* 1. the reference sequence (src/align.c:163-175): first record of the file */
  readfasta_t rfas = new_readfasta (ref_file);
  if (readfasta_next (rfas) < 1) biomcmc_error ("Error reading reference sequence %s", ref_file);
  char *refseq = rfas->seq; rfas->seq = NULL;
  const size_t aln_length = rfas->seqlength;
  del_readfasta (rfas);
  if (aln_length > 0x3fffffff) biomcmc_error ("reference sequence of %zu sites is too long", aln_length);
  if (compact && aln_length > UVDB_COMPACT_MAX_NCHAR) biomcmc_error ("--compact: alignments of more than %d sites have no compact form (%zu sites)", UVDB_COMPACT_MAX_NCHAR, aln_length);
  /* alignments of different queries do not depend on each other: with several GPUs every pool is cut into contiguous shares, one
     aligner and one host thread per GPU (replicas of src/align.c's per-thread aligners, no exchange) */
  if (!n_devices) { n_devices = 1; devices[0] = device; }
  uvaia_aligner *gpu[64];
  for (int d = 0; d < n_devices; d++) if (uvaia_align_open (&gpu[d], refseq, (int) aln_length, devices[d], NULL)) biomcmc_error ("%s", uvaia_align_last_error (NULL));
  if (n_devices > 1) fprintf (stderr, "Batches of %d sequences will be read and aligned on %d GPUs.\n", pool, n_devices);
  else fprintf (stderr, "Batches of %d sequences will be read and aligned on GPU %d.\n", pool, devices[0]);

  struct uvdb_packer pk;
  double align_ms = 0.;
  if (packed) {
    if (uvdb_packer_open (&pk, packed, (int) aln_length, ambig_r, devices[0], pool, compact)) biomcmc_error ("%s", pk.err);
    fprintf (stderr, "Aligned sequences with at least %d valid sites will be packed into %s.\n", pk.non_n_ref, packed);
  }
  file_compress_t outstream = (to_screen || !write_text) ? NULL : biomcmc_open_compress (outfilename, "w");
  char **seq = (char **) biomcmc_malloc ((size_t) pool * sizeof (char *)), **name = (char **) biomcmc_malloc ((size_t) pool * sizeof (char *));
  int *len = (int *) biomcmc_malloc ((size_t) pool * sizeof (int));
  char *aln = write_text ? (char *) biomcmc_malloc ((size_t) pool * (aln_length + 1)) : NULL;
  int count = 0, n_output = 0, n_pool = 0;
  const int print_interval = 5000;
  double result[3];

  biomcmc_get_time (time1);
  for (int j = 0; j < n_fasta; j++) {
    fprintf (stderr, "Started  reading file %s\n", fasta[j]);
    rfas = new_readfasta (fasta[j]);
    bool end_of_file = false;
    while (!end_of_file) {
      int fill = 0;
      while (fill < pool) {                           /* the serial slot-filling loop with its filters (src/align.c:189-221) */
        if (readfasta_next (rfas) < 0) { end_of_file = true; break; }
        if (!rfas->seq) continue;                     /* a header without sequence lines */
        count++;
        bool seq_valid = true;
        if (((3 * rfas->seqlength) < (2 * aln_length)) || ((2 * rfas->seqlength) > (3 * aln_length))) {
          fprintf (stderr, "Sequence %s has size too different from reference (%lu vs %lu)\n", rfas->name, (unsigned long) rfas->seqlength, (unsigned long) aln_length);
          seq_valid = false;
        }
        if (seq_valid) biomcmc_count_sequence_acgt (rfas->seq, rfas->seqlength, result);
        if (seq_valid && (result[2] > ambig)) {
          fprintf (stderr, "Sequence %s has proportion of N etc. (=%lf) above threshold of %lf\n", rfas->name, result[2], ambig);
          seq_valid = false;
        }
        if (seq_valid && (result[0] < 1. - 1.1 * ambig)) {
          fprintf (stderr, "Sequence %s has proportion of ACGT (=%lf) below threshold of %lf\n", rfas->name, result[0], 1. - 1.1 * ambig);
          seq_valid = false;
        }
        if (!seq_valid) continue;                     /* readfasta_next frees what it still owns */
        seq[fill] = rfas->seq; rfas->seq = NULL;
        name[fill] = rfas->name; rfas->name = NULL;
        len[fill] = (int) rfas->seqlength;
        fill++;
      }
      if (fill) {
        int failed = -1;
        n_pool++;
        if (packed) {   /* one GPU: the steps of uvaia_align_batch, the copy of the text only if somebody reads it */
          double ms = 0.;
          if (uvaia_align_load (gpu[0], (const char *const *) seq, len, fill) || uvaia_align_run (gpu[0]) || (write_text && uvaia_align_fetch (gpu[0], aln, NULL))) failed = 0;
          else if (!uvaia_align_stats (gpu[0], NULL, NULL, NULL, &ms)) align_ms += ms;
        } else {
#pragma omp parallel for num_threads(n_devices) schedule(static, 1)
          for (int d = 0; d < n_devices; d++) {
            const int a = (int) ((long long) fill * d / n_devices), b = (int) ((long long) fill * (d + 1) / n_devices);
            if (b > a && uvaia_align_batch (gpu[d], (const char *const *) seq + a, len + a, b - a, aln + (size_t) a * (aln_length + 1), NULL)) {
#pragma omp critical
              failed = d;
            }
          }
        }
        if (failed >= 0) {   /* what was aligned so far stays a complete file: close the stream before giving up */
          const int a = (int) ((long long) fill * failed / n_devices), b = (int) ((long long) fill * (failed + 1) / n_devices);
          if (outstream) biomcmc_close_compress (outstream);
          if (packed) uvdb_packer_close (&pk);
          biomcmc_error ("%s (counted from sequence %s, the first of the %d handed to device %d; %d sequences were written before)",
                         uvaia_align_last_error (gpu[failed]), name[a], b - a, failed, n_output);
        }
        if (packed && packer_add_pool (&pk, gpu[0], name, fill)) {   /* both files stay complete: close them before giving up */
          char msg[640];
          snprintf (msg, sizeof msg, "%s", pk.err);
          if (outstream) biomcmc_close_compress (outstream);
          const long kept = pk.kept;
          uvdb_packer_close (&pk);
          biomcmc_error ("packing pool %d (%d sequences, the first is %s): %s; %ld sequences were packed before", n_pool, fill, name[0], msg, kept);
        }
        for (int c = 0; c < fill; c++) {
          n_output++;
          if (write_text) {
            const char *row = aln + (size_t) c * (aln_length + 1);
            if (to_screen) printf (">%s\n%s\n", name[c], row);
            else write_fasta_record (outstream, name[c], row);
          }
          free (seq[c]); free (name[c]);
        }
      }
      if ((count >= print_interval) && ((count % print_interval) < pool)) {
        fprintf (stderr, "%d\t sequences read, %d \t aligned. %.3lf secs elapsed.\n", count, n_output, biomcmc_update_elapsed_time (time1));
        fflush (stderr);
      }
    }
    del_readfasta (rfas);
    fprintf (stderr, "Finished reading file %s. In total %d sequences have been read.\n", fasta[j], count);
    fflush (stderr);
  }
  if (packed) {
    const long kept = pk.kept, dropped = pk.dropped;
    if (uvdb_packer_close (&pk)) biomcmc_error ("%s", pk.err);
    fprintf (stderr, "Packed %ld of %d aligned sequences (%zu sites) into %s; %ld too ambiguous.\n", kept, n_output, aln_length, packed, dropped);
    fprintf (stderr, "Device time: alignment %.3lf ms; census %.3lf ms, gather %.3lf ms, exception runs %.3lf ms.\n", align_ms, pk.rows_ms[0], pk.rows_ms[1], pk.rows_ms[2]);
    if (compact) fprintf (stderr, "Compact tiles: %ld encoded on the device (count and prefix %.3lf ms, emit %.3lf ms), %ld on the host.\n", pk.tiles_device, pk.encode_ms[0], pk.encode_ms[1], pk.tiles_host);
  }
  if (to_screen) fprintf (stderr, "Output %d aligned sequences. Total elapsed time: %.3lf secs\n", n_output, biomcmc_update_elapsed_time (time0));
  else if (!write_text) fprintf (stderr, "Aligned %d sequences. Total elapsed time: %.3lf secs\n", n_output, biomcmc_update_elapsed_time (time0));
  else {
    biomcmc_close_compress (outstream);
    fprintf (stderr, "Saved %d sequences to file %s\nTotal elapsed time: %.3lf secs\n", n_output, outfilename, biomcmc_update_elapsed_time (time0));
  }
  for (int d = 0; d < n_devices; d++) uvaia_align_close (gpu[d]);
  free (seq); free (name); free (len); free (aln); free (refseq); free (outfilename);
  return EXIT_SUCCESS;
}
